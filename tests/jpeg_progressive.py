"""Progressive (SOF2) scan writer, and the script cells built with it (a test
helper beside tests/jpeg_recode.py: tests import it, nothing else does).

``progressive`` writes a SOF2 file from quantised coefficients under any scan
script: any band split, any Ah/Al ladder, interleaved or per-component DC
scans, DHT / DQT / DRI between scans. It restates ITU T.81 Annex G:

* G.1.2.1 DC first: the point transform is an arithmetic shift right by Al,
  then differences per component, coded like sequential DC (F.1.2.1); DC
  refinement: bit Al of every block's DC value, no Huffman coding.
* G.1.2.2 AC first: magnitudes divided toward zero by 2^Al; (run, size)
  symbols with ZRL for runs above 15; a block that ends in zeros joins an EOB
  run, written as EOBn (symbol n << 4, n extra bits) before the next coded
  coefficient, when the run reaches 0x7FFF, before a restart marker and at
  the end of the scan.
* G.1.2.3 AC refinement: a coefficient that was already non-zero sends bit Al
  of its magnitude (a correction bit); one that becomes non-zero sends
  (run << 4 | 1) and a sign bit, the run counting only the zero-history
  coefficients passed; the correction bits passed on the way are written
  behind the symbol (and its sign bit), those of a block's tail behind the
  EOB run's symbol, in block order.
* A.2: a scan of one component walks that component's own
  ceil(w*H / (8*Hmax)) x ceil(h*V / (8*Vmax)) blocks; a scan of several walks
  MCUs. B.1.1.5 byte stuffing, 1-padding before RSTn, EOI.

Every scan's Huffman tables come from a ``shape(tc, histogram)`` function as in
``jpeg_recode.recode``: ``optimal`` (Annex K.2 lengths limited to 16 bits, the
all-ones word reserved) by default, or the hostile shapes of jpeg_recode on the
scan's own histogram, EOBn symbols included. Every table passes
``validate_table``.

The writer records what it emitted (``record=``): per scan the band, the
restart interval in force, the restart markers written, the longest code
used, the longest code of an EOBn symbol (n >= 1) and whether the code 0xFFFE (fifteen ones and a zero: the highest code a
table may hold, since libjpeg refuses the all-ones word itself) was used; per
file the scans of each chain, the largest EOB category, the most correction
bits written between two stops of one block and behind an EOB run for one
block, and the ZRL symbols inside refinement scans. The tests assert their
coverage from it.

``baseline`` writes the same coefficients as one sequential scan (F.1.2), the
twin a hand-made cell is compared with; cells cut from a Pillow file are
compared with ``jpeg_recode.reframe`` of that file instead.

``script_cells`` / ``refused_script_cells`` are the cells the tests share.
"""
import functools
import heapq
from collections import namedtuple

import numpy as np

import jpeg_recode as jr

JFIF = jr.JFIF


# ---------------------------------------------------------------------------
# coefficients
# ---------------------------------------------------------------------------
Source = namedtuple("Source", "coefs qtables tq")


@functools.lru_cache(maxsize=None)
def coefs_from_444(jpeg444: bytes) -> Source:
    """The quantised coefficients of a baseline 4:4:4 file, one
    int16[blocks high, blocks wide, 64] array per component in zigzag order,
    with the file's quantisation tables (by table id, zigzag order) and the
    table id of each component."""
    bw, bh, grids = jr.block_grids(jpeg444)
    coefs = []
    for g in grids:
        a = np.zeros((bh, bw, 64), np.int16)
        for (bx, by), (dc, ac) in g.items():
            a[by, bx, 0] = dc
            k = 1
            for sym, extra in ac:
                if sym & 15:
                    k += sym >> 4
                    a[by, bx, k] = jr._dc_value(sym & 15, extra)
                    k += 1
                elif sym == 0xF0:
                    k += 16
                else:
                    break
        a.setflags(write=False)
        coefs.append(a)
    segs = jr.parse(jpeg444)[0]
    qt = {}
    for m, p in segs:
        s = 0
        while m == 0xDB and s < len(p):
            if p[s] >> 4:
                qt[p[s] & 15] = tuple((p[s + 1 + 2 * k] << 8) | p[s + 2 + 2 * k] for k in range(64))
                s += 129
            else:
                qt[p[s] & 15] = tuple(p[s + 1:s + 65])
                s += 65
    sof = next(p for m, p in segs if m == 0xC0)
    tq = tuple(sof[8 + 3 * c] for c in range(3))
    return Source(tuple(coefs), tuple(qt[i] for i in range(max(qt) + 1)), tq)


def _ceil(a, b):
    return -(-a // b)


def _grids(coefs, factors, height, width):
    """Per component: (the coefficient grid over whole MCUs, wrapped where the
    source is smaller; (blocks wide, blocks high) of the component's own scans)."""
    nc = len(coefs)
    assert nc in (1, 3) and len(factors) == nc
    hmax, vmax = max(f[0] for f in factors), max(f[1] for f in factors)
    out = []
    for c, (h, v) in enumerate(factors):
        own = (_ceil(_ceil(width * h, hmax), 8), _ceil(_ceil(height * v, vmax), 8))
        full = own if nc == 1 else (_ceil(width, 8 * hmax) * h, _ceil(height, 8 * vmax) * v)
        src = np.asarray(coefs[c])
        assert src.ndim == 3 and src.shape[2] == 64
        g = src[(np.arange(full[1]) % src.shape[0])[:, None], (np.arange(full[0]) % src.shape[1])[None, :]]
        out.append((g.astype(np.int32), own))
    return out


# ---------------------------------------------------------------------------
# the default table shape
# ---------------------------------------------------------------------------
def optimal(tc, hist):
    """Huffman lengths of the histogram with one reserved code point (so no
    symbol gets the all-ones word), limited to 16 bits as T.81 K.3 does it."""
    heap = [(f, s, (s,)) for s, f in hist.items()] + [(0, 256, (256,))]
    heapq.heapify(heap)
    depth = dict.fromkeys([s for _, s, _ in heap], 0)
    while len(heap) > 1:
        fa, ta, sa = heapq.heappop(heap)
        fb, tb, sb = heapq.heappop(heap)
        for s in sa + sb:
            depth[s] += 1
        heapq.heappush(heap, (fa + fb, min(ta, tb), sa + sb))
    top = max(max(depth.values()), 16)
    bits = [0] * (top + 1)
    for d in depth.values():
        bits[d] += 1
    for i in range(top, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = max(l for l in range(1, 17) if bits[l])
    bits[i] -= 1  # the reserved code point
    syms = sorted(hist, key=lambda s: (depth[s], -hist[s], s))
    return bits[1:17], syms


def runs_or(other):
    """`runs` where the histogram fits that shape (at most 41 AC symbols, 15 DC
    symbols), `other` elsewhere."""
    def shape(tc, hist):
        if len(hist) + 1 <= (16 if tc == 0 else 42):
            return jr.runs(tc, hist)
        return other(tc, hist)
    return shape


SHAPES = dict(jr.SHAPES, runs=runs_or(jr.ones))


# ---------------------------------------------------------------------------
# the scans: each one a list of items
#   ("S", tc, scan component, symbol, extra bits)   a Huffman symbol and its bits
#   ("B", bits)                                     raw bits
#   ("R",)                                          a restart marker
# ---------------------------------------------------------------------------
def _bits(v: int, n: int) -> str:
    return format(v, "0%db" % n) if n else ""


def _units(grids, comps, nc):
    """The scan's units in order, each a list of (scan component, block)."""
    if len(comps) == 1:
        g, (ow, oh) = grids[comps[0]][0], grids[comps[0]][1]
        rows = g[:oh, :ow].reshape(-1, 64).tolist()
        return [[(0, b)] for b in rows]
    assert nc > 1
    out = []
    lists = [grids[c][0].tolist() for c in comps]
    h0, v0 = grids[comps[0]][2]
    mcux, mcuy = len(lists[0][0]) // h0, len(lists[0]) // v0
    for my in range(mcuy):
        for mx in range(mcux):
            u = []
            for i, c in enumerate(comps):
                h, v = grids[c][2]
                for by in range(v):
                    for bx in range(h):
                        u.append((i, lists[i][my * v + by][mx * h + bx]))
            out.append(u)
    return out


def _scan_items(units, ss, se, ah, al, ri, rec, srec):
    """The items of one scan (T.81 G.1.2); updates the file's record `rec`
    and the scan's `srec`."""
    items = []
    restarts = 0
    if ss == 0:
        pred = {}
        for n, u in enumerate(units):
            if ri and n and n % ri == 0:
                items.append(("R",))
                restarts += 1
                pred = {}
            for i, blk in u:
                if ah == 0:
                    v = blk[0] >> al  # arithmetic shift
                    size, extra = jr._dc_symbol(v - pred.get(i, 0))
                    pred[i] = v
                    items.append(("S", 0, i, size, extra))
                else:
                    items.append(("B", str((blk[0] >> al) & 1)))
        srec["restarts"] = restarts
        return items
    eobrun, be = 0, []  # the EOB run and the correction bits buffered behind it

    def flush():
        nonlocal eobrun, be
        if eobrun:
            n = eobrun.bit_length() - 1
            items.append(("S", 1, 0, n << 4, _bits(eobrun - (1 << n), n)))
            rec["eob_cat"] = max(rec["eob_cat"], n)
            srec["eob_cat"] = max(srec["eob_cat"], n)
            eobrun = 0
        if be:
            items.append(("B", "".join(be)))
            be = []

    for n, u in enumerate(units):
        if ri and n and n % ri == 0:
            flush()
            items.append(("R",))
            restarts += 1
        blk = u[0][1]
        if ah == 0:
            last = ss - 1
            for k in range(ss, se + 1):
                a = abs(blk[k]) >> al
                if a == 0:
                    continue
                flush()
                r = k - last - 1
                while r > 15:
                    items.append(("S", 1, 0, 0xF0, ""))
                    r -= 16
                size = a.bit_length()
                items.append(("S", 1, 0, r << 4 | size, _bits(a if blk[k] > 0 else (1 << size) - 1 - a, size)))
                last = k
            if last < se:
                eobrun += 1
                if eobrun == 0x7FFF:
                    flush()
            continue
        mags = [abs(blk[k]) >> al for k in range(se + 1)]
        newest = max([k for k in range(ss, se + 1) if mags[k] == 1], default=-1)
        r, br = 0, []
        for k in range(ss, se + 1):
            a = mags[k]
            if a == 0:
                r += 1
                continue
            while r > 15 and k <= newest:
                flush()
                items.append(("S", 1, 0, 0xF0, ""))
                rec["refine_zrl"] += 1
                srec["refine_zrl"] += 1
                r -= 16
                rec["corr_stop"] = max(rec["corr_stop"], len(br))
                if br:
                    items.append(("B", "".join(br)))
                    br = []
            if a > 1:
                br.append(str(a & 1))
                continue
            flush()
            items.append(("S", 1, 0, r << 4 | 1, ("0" if blk[k] < 0 else "1")))
            rec["corr_stop"] = max(rec["corr_stop"], len(br))
            if br:
                items.append(("B", "".join(br)))
                br = []
            r = 0
        if r > 0 or br:
            eobrun += 1
            rec["corr_eob"] = max(rec["corr_eob"], len(br))
            be += br
            if eobrun == 0x7FFF:
                flush()
    flush()
    srec["restarts"] = restarts
    return items


def _stuffed(bits: str) -> bytes:
    bits += "1" * (-len(bits) % 8)
    return int(bits, 2).to_bytes(len(bits) // 8, "big").replace(b"\xff", b"\xff\x00") if bits else b""


def _body(items, enc_of, rec):
    """The entropy-coded bytes of one scan; enc_of(tc, scan component) gives
    {symbol: code string}."""
    out, cur, nrst = bytearray(), [], 0
    for it in items:
        if it[0] == "S":
            code = enc_of(it[1], it[2])[it[3]]
            rec["max_len"] = max(rec["max_len"], len(code))
            rec["top_code"] = rec["top_code"] or code == "1" * 15 + "0"
            if it[1] == 1 and it[3] & 15 == 0 and 0x10 <= it[3] <= 0xE0:  # EOBn, n >= 1
                rec["eob_len"] = max(rec["eob_len"], len(code))
            cur.append(code)
            cur.append(it[4])
        elif it[0] == "B":
            cur.append(it[1])
        else:
            out += _stuffed("".join(cur)) + bytes([0xFF, 0xD0 + nrst % 8])
            cur, nrst = [], nrst + 1
    return bytes(out + _stuffed("".join(cur)))


def _seg(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def _dqt(tid: int, table) -> bytes:
    table = [int(x) for x in table]
    assert len(table) == 64 and all(1 <= x <= 65535 for x in table)
    if max(table) > 255:
        return _seg(0xDB, bytes([0x10 | tid]) + b"".join(x.to_bytes(2, "big") for x in table))
    return _seg(0xDB, bytes([tid]) + bytes(table))


def _header(marker, qtables, tq, factors, height, width, app, ids):
    nc = len(factors)
    out = bytearray(b"\xff\xd8" + app)
    for tid, t in enumerate(qtables):
        if t is not None:
            out += _dqt(tid, t)
    out += _seg(marker, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([nc]) + b"".join(
        bytes([ids[c], factors[c][0] << 4 | factors[c][1], tq[c]]) for c in range(nc)))
    return out


def _default_tq(qtables, nc):
    return tuple(min(c, 1, len(qtables) - 1) for c in range(nc))


def _make_tables(shape, hists):
    """{(tc, th): (counts, symbols, {symbol: code string})} from {(tc, th): histogram}."""
    out = {}
    for (tc, th), h in sorted(hists.items()):
        counts, symbols = shape(tc, h)
        counts, symbols = [int(c) for c in counts], [int(s) for s in symbols]
        jr.validate_table(tc, counts, symbols, h)
        out[tc, th] = (counts, symbols,
                       {sym: format(code, "0%db" % n) for sym, n, code in jr.canonical(counts, symbols)})
    return out


def _dht(tables) -> bytes:
    return _seg(0xC4, b"".join(bytes([tc << 4 | th]) + bytes(c) + bytes(s) for (tc, th), (c, s, _) in sorted(tables.items())))


def _new_record():
    return {"scans": [], "chains": {}, "eob_cat": 0, "corr_stop": 0, "corr_eob": 0, "refine_zrl": 0}


def progressive(coefs, qtables, factors, height, width, script, *, tables=optimal, app=JFIF, ids=(1, 2, 3),
                tq=None, record=None) -> bytes:
    """A SOF2 file of `width` x `height` with the sampling factors
    ``factors = ((H, V) per component)`` (one or three components).

    coefs: per component the quantised coefficients in zigzag order,
    [blocks high, blocks wide, 64]; wrapped where the target grid is larger,
    as ``jpeg_recode.reframe`` does. qtables: the tables written before the
    frame header, by table id (zigzag order; None: that id stays undefined);
    tq: each component's table id (default 0, 1, 1).

    script: a list of entries, in file order:
      (components, Ss, Se, Ah, Al) or (components, Ss, Se, Ah, Al, options)
          one scan; components are frame component indices. Options:
          "dri": N     a DRI segment before the scan (0 is written too: it
                       turns restarts off); it stays in force until the next
          "th": id(s)  the Huffman table id, one per scan component or one for
                       all (default: 0 for component 0, else 1)
          "dht": False no DHT before the scan: the tables defined at those
                       ids before an earlier scan are used again (they are
                       built from both scans' symbols)
          "shape": f   this scan's table shape, instead of `tables`
      ("DQT", id, table)
          a DQT segment at this place.
    tables: shape(tc, histogram) -> (counts[16], symbols), for every scan.
    record: a dict that receives what was written (see the module docstring).
    Nothing checks that a decoder accepts the script: refused files are built
    the same way."""
    nc = len(coefs)
    tq = _default_tq(qtables, nc) if tq is None else tq
    grids = [(g, own, factors[c]) for c, (g, own) in enumerate(_grids(coefs, factors, height, width))]
    rec = _new_record() if record is None else record
    rec.update(_new_record())
    # 1. the items and histograms of every scan
    scans, ri = [], 0
    for n, e in enumerate(script):
        if e[0] == "DQT":
            continue
        comps = (e[0],) if isinstance(e[0], int) else tuple(e[0])
        ss, se, ah, al = e[1:5]
        opt = dict(e[5]) if len(e) > 5 else {}
        if "dri" in opt:
            ri = opt["dri"]
        th = opt.get("th", tuple(min(c, 1) for c in comps))
        th = (th,) * len(comps) if isinstance(th, int) else tuple(th)
        srec = {"comps": comps, "ss": ss, "se": se, "ah": ah, "al": al, "restart": ri, "th": th,
                "kind": ("dc" if ss == 0 else "ac") + ("-first" if ah == 0 else "-refine"),
                "max_len": 0, "top_code": False, "eob_len": 0, "eob_cat": 0, "refine_zrl": 0}
        units = _units(grids, comps, nc)
        srec["units"] = len(units)
        items = _scan_items(units, ss, se, ah, al, ri, rec, srec)
        hists = {}
        for it in items:
            if it[0] == "S":
                h = hists.setdefault((it[1], th[it[2]]), {})
                h[it[3]] = h.get(it[3], 0) + 1
        scans.append({"entry": n, "comps": comps, "opt": opt, "items": items, "hists": hists, "rec": srec, "th": th})
        chain = "dc" if ss == 0 else comps[0]
        rec["chains"][chain] = rec["chains"].get(chain, 0) + 1
        rec["scans"].append(srec)
    # 2. the tables: a scan that writes a DHT covers the later scans that reuse its ids
    for i, s in enumerate(scans):
        if not s["opt"].get("dht", True):
            continue
        merged = {k: dict(h) for k, h in s["hists"].items()}
        for key in merged:
            for t in scans[i + 1:]:
                if key in t["hists"]:
                    if t["opt"].get("dht", True):
                        break
                    for sym, f in t["hists"][key].items():
                        merged[key][sym] = merged[key].get(sym, 0) + f
        s["tables"] = _make_tables(s["opt"].get("shape", tables), merged)
    # 3. the file
    out = _header(0xC2, qtables, tq, factors, height, width, app, ids)
    live, by_entry = {}, {s["entry"]: s for s in scans}
    for n, e in enumerate(script):
        if e[0] == "DQT":
            out += _dqt(e[1], e[2])
            continue
        s = by_entry[n]
        if "dri" in s["opt"]:
            out += _seg(0xDD, s["opt"]["dri"].to_bytes(2, "big"))
        if "tables" in s:
            if s["tables"]:
                out += _dht(s["tables"])
            live.update(s["tables"])
        ss, se, ah, al = e[1:5]
        sel = bytearray()
        for i, c in enumerate(s["comps"]):
            t = s["th"][i]
            sel += bytes([ids[c], (t << 4 if ss == 0 else t)])
        out += _seg(0xDA, bytes([len(s["comps"])]) + bytes(sel) + bytes([ss, se, ah << 4 | al]))
        th = s["th"]
        for key in s["hists"]:
            assert key in live and set(s["hists"][key]) <= set(live[key][2]), "a reused table lacks a symbol"
        out += _body(s["items"], lambda tc, i: live[tc, th[i]][2], s["rec"])
    return bytes(out + b"\xff\xd9")


def baseline(coefs, qtables, factors, height, width, *, tables=optimal, app=JFIF, ids=(1, 2, 3), tq=None,
             restart=0) -> bytes:
    """The same coefficients as a baseline file: one sequential scan of every
    component (T.81 F.1.2), DC table 0 / AC table 0 for the first component
    and 1 / 1 for the others."""
    nc = len(coefs)
    tq = _default_tq(qtables, nc) if tq is None else tq
    grids = [(g, own, factors[c]) for c, (g, own) in enumerate(_grids(coefs, factors, height, width))]
    units = _units(grids, tuple(range(nc)), nc)
    items, pred = [], {}
    for n, u in enumerate(units):
        if restart and n and n % restart == 0:
            items.append(("R",))
            pred = {}
        for i, blk in u:
            size, extra = jr._dc_symbol(blk[0] - pred.get(i, 0))
            pred[i] = blk[0]
            items.append(("S", 0, i, size, extra))
            last = 0
            for k in range(1, 64):
                if blk[k] == 0:
                    continue
                r = k - last - 1
                while r > 15:
                    items.append(("S", 1, i, 0xF0, ""))
                    r -= 16
                a = abs(blk[k])
                size = a.bit_length()
                items.append(("S", 1, i, r << 4 | size, _bits(a if blk[k] > 0 else (1 << size) - 1 - a, size)))
                last = k
            if last < 63:
                items.append(("S", 1, i, 0x00, ""))
    hists = {}
    for it in items:
        if it[0] == "S":
            h = hists.setdefault((it[1], min(it[2], 1)), {})
            h[it[3]] = h.get(it[3], 0) + 1
    tabs = _make_tables(tables, hists)
    out = _header(0xC0, qtables, tq, factors, height, width, app, ids)
    if restart:
        out += _seg(0xDD, restart.to_bytes(2, "big"))
    out += _dht(tabs)
    out += _seg(0xDA, bytes([nc]) + b"".join(bytes([ids[c], min(c, 1) * 0x11]) for c in range(nc)) + b"\x00\x3f\x00")
    rec = {"max_len": 0, "top_code": False, "eob_len": 0}
    out += _body(items, lambda tc, i: tabs[tc, min(i, 1)][2], rec)
    return bytes(out + b"\xff\xd9")


# ---------------------------------------------------------------------------
# the scripts (YCbCr: components 0, 1, 2)
# ---------------------------------------------------------------------------
ALL = (0, 1, 2)


def spectral_only():
    return [(ALL, 0, 0, 0, 0)] + [(c, 1, 63, 0, 0) for c in ALL]


def bands():
    """Per-component DC scans in the order Cr, Y, Cb; luma in five first
    scans with bands of one coefficient at both ends; chroma in one."""
    return [(2, 0, 0, 0, 0), (0, 0, 0, 0, 0), (1, 0, 0, 0, 0),
            (0, 1, 1, 0, 0), (0, 2, 5, 0, 0), (0, 6, 20, 0, 0), (0, 21, 62, 0, 0), (0, 63, 63, 0, 0),
            (1, 1, 63, 0, 0), (2, 1, 63, 0, 0)]


def deep():
    """DC at Al = 3 refined three times (interleaved, per component,
    interleaved); luma in two first scans at different Al, a refinement of
    the sub-band alone, one over both histories, then each band to 0; chroma
    from Al = 2 down."""
    return [(ALL, 0, 0, 0, 3),
            (0, 1, 10, 0, 3), (0, 11, 63, 0, 2), (1, 1, 63, 0, 2), (2, 1, 63, 0, 2),
            (ALL, 0, 0, 3, 2),
            (0, 1, 10, 3, 2), (0, 1, 63, 2, 1), (1, 1, 63, 2, 1), (2, 1, 63, 2, 1),
            (0, 0, 0, 2, 1), (1, 0, 0, 2, 1), (2, 0, 0, 2, 1),
            (0, 1, 10, 1, 0), (0, 11, 63, 1, 0), (1, 1, 63, 1, 0), (2, 1, 63, 1, 0),
            (ALL, 0, 0, 1, 0)]


def shuffled():
    """The chains interleaved in file order; each component's AC scans before
    the DC refinement, which comes last."""
    return [(ALL, 0, 0, 0, 1), (1, 1, 63, 0, 1), (0, 1, 5, 0, 2), (2, 1, 63, 0, 1), (0, 6, 63, 0, 2),
            (1, 1, 63, 1, 0), (0, 1, 63, 2, 1), (2, 1, 63, 1, 0), (0, 1, 63, 1, 0), (ALL, 0, 0, 1, 0)]


def sixtyfour(extra=False):
    """64 scans: DC, luma one coefficient per scan up to 59 and 60-63 (60
    scans), Cb in two bands, Cr in one; `extra` splits Cr too: 65."""
    s = [(ALL, 0, 0, 0, 0)] + [(0, k, k, 0, 0) for k in range(1, 60)] + [(0, 60, 63, 0, 0)]
    s += [(1, 1, 9, 0, 0), (1, 10, 63, 0, 0)]
    s += [(2, 1, 9, 0, 0), (2, 10, 63, 0, 0)] if extra else [(2, 1, 63, 0, 0)]
    return s


def latch(chroma_q, junk_q):
    """Table id 1 holds `junk_q` until luma's first scan has passed, then the
    real chroma table; once every component has latched its table both ids
    are overwritten with junk, which must change nothing."""
    return [(0, 0, 0, 0, 0), ("DQT", 1, chroma_q), (1, 0, 0, 0, 0), (2, 0, 0, 0, 0),
            ("DQT", 0, junk_q), ("DQT", 1, junk_q),
            (0, 1, 63, 0, 0), (1, 1, 63, 0, 0), (2, 1, 63, 0, 0)]


def restarts():
    """A DRI before every scan: 1, 3, 7, 33 and 0 after a non-zero one. AC
    first and refinement scans whose EOB runs the restarts cut; DC
    refinement with restarts (per component and interleaved) and without."""
    return [(ALL, 0, 0, 0, 1, {"dri": 1}),
            (0, 1, 63, 0, 1, {"dri": 3}),
            (1, 1, 63, 0, 1, {"dri": 7}),
            (2, 1, 63, 0, 1, {"dri": 0}),
            (0, 1, 63, 1, 0, {"dri": 33}),
            (1, 1, 63, 1, 0, {"dri": 3}),
            (2, 1, 63, 1, 0, {"dri": 1}),
            (0, 0, 0, 1, 0, {"dri": 7}),
            (1, 0, 0, 1, 0, {"dri": 0}),
            (2, 0, 0, 1, 0, {"dri": 33})]


def restarts_interleaved():
    """Interleaved DC refinement under a restart interval of 3 MCUs, then
    the AC scans with none."""
    return [(ALL, 0, 0, 0, 2, {"dri": 7}), (ALL, 0, 0, 2, 1, {"dri": 3}), (ALL, 0, 0, 1, 0, {"dri": 0})] + \
           [(c, 1, 63, 0, 0) for c in ALL]


def partial():
    """Coefficients 0..9 complete; chroma 10-63 never sent, luma 10-63 at Al = 1 for good."""
    return [(ALL, 0, 0, 0, 0), (0, 1, 9, 0, 0), (1, 1, 9, 0, 0), (2, 1, 9, 0, 0), (0, 10, 63, 0, 1)]


def tables_script():
    """`deep` under one hostile shape: table ids 0..3 all in use, an AC scan
    that reuses the table written before an earlier scan of its chain, and
    AC id 1 redefined between a Cb scan and a Cr scan."""
    s = [list(e) + [{}] for e in deep()]
    for e in s:
        comps, ss, ah = e[0], e[1], e[3]
        if ss == 0:
            e[5]["th"] = (3, 0, 2) if ah == 0 else 0
        else:
            e[5]["th"] = (0, 1, 3)[comps]
    s[2][5]["th"] = 2
    s[13][5]["dht"] = False
    s[9][5]["th"] = 1
    s[15][5]["dht"] = False
    return [tuple(e) for e in s]


def gray_script():
    return [(0, 0, 0, 0, 1, {"dri": 2}), (0, 1, 2, 0, 0), (0, 3, 20, 0, 1), (0, 21, 63, 0, 0), (0, 3, 20, 1, 0),
            (0, 0, 0, 1, 0)]


def eob_max_script():
    return [(0, 0, 0, 0, 1), (0, 0, 0, 1, 0), (0, 1, 63, 0, 1), (0, 1, 63, 1, 0)]


def dense_script():
    return [(ALL, 0, 0, 0, 0)] + [(c, 1, 63, 0, 1) for c in ALL] + [(c, 1, 63, 1, 0) for c in ALL]


# ---------------------------------------------------------------------------
# the cells
# ---------------------------------------------------------------------------
F444 = ((1, 1),) * 3
F420 = jr.F420
F422 = ((2, 1), (1, 1), (1, 1))
LAYOUTS = (("420", F420), ("422", F422), ("444", F444), ("440", ((1, 2), (1, 1), (1, 1))),
           ("411", ((4, 1), (1, 1), (1, 1))), ("3x1", ((3, 1), (1, 1), (1, 1))),
           ("22-21-12", ((2, 2), (2, 1), (1, 2))))
# (height, width): one block; a partial block both ways; odd luma block counts under 4:2:0;
# 99 luma blocks (three whole 32-block chunks and a partial one); tens of chunks
SIZES = ((1, 1), (8, 8), (9, 17), (40, 56), (72, 88), (200, 264))
UNSUPPORTED, CORRUPT = 2, 3

# data: the file; twin: the baseline file with the same coefficients (None for a refused
# cell); status: the planner's LDT_IMG_* code
ScriptCell = namedtuple("ScriptCell", "name data twin factors height width script record tags status")


@functools.lru_cache(maxsize=None)
def random_source() -> bytes:
    """Quality-100 4:4:4 file of uniform random bytes: nearly all 63 AC
    coefficients of every block are non-zero."""
    from PIL import Image

    r = np.random.RandomState(77)
    return jr._save(Image.fromarray(r.randint(0, 256, (40, 56, 3)).astype(np.uint8)), quality=100, subsampling="4:4:4")


def dense_blocks(src):
    """A copy of `src` (int16[bh, bw, 64]) with four hand-made blocks in its
    first row, for a refinement 1 -> 0 over 1-63:
    0: 40 history coefficients before the only new one (40 correction bits
       before a stop), then 22 more (under the EOB run);
    1: 63 history coefficients (all under the EOB run);
    2: 20 zeros before a new coefficient at 21 (a ZRL inside the block), with
       history coefficients from 22 to 58 and a new one at 59 (37 correction
       bits before a stop);
    3: history at the even positions only, new values at 7 odd ones."""
    a = np.array(src, np.int16)
    assert a.shape[1] >= 4
    b = np.zeros((4, 64), np.int16)
    b[:, 0] = a[0, :4, 0]
    b[0, 1:41], b[0, 41], b[0, 42:64] = 3, 1, -2
    b[1, 1:64] = np.where(np.arange(63) % 3 == 0, -5, 6)
    b[2, 21], b[2, 22:59], b[2, 59] = -1, 2, 1
    b[3, 2:64:2] = -3
    b[3, 9:64:8] = 1
    a[0, :4] = b
    return a


@functools.lru_cache(maxsize=None)
def script_cells():
    """The accepted cells, in a fixed order (a tuple of ScriptCell)."""
    src = jr.layout_source()  # the non-optimised 4:4:4 Pillow file of synth.field with noise
    S = coefs_from_444(src)
    rnd = random_source()
    R = coefs_from_444(rnd)
    cells = []

    def add(name, script, factors, h, w, *tags, source=S, src_file=src, twin="reframe", **kw):
        rec = {}
        ts = kw.pop("twin_source", source)
        data = progressive(source.coefs, kw.pop("qtables", source.qtables), factors, h, w, script,
                           tq=kw.pop("tq", source.tq), record=rec, **kw)
        if twin == "reframe":
            twin = jr.reframe(src_file, factors, h, w)
        elif twin == "baseline":
            twin = baseline(ts.coefs, ts.qtables, factors, h, w, tq=ts.tq)
        cells.append(ScriptCell(name, data, twin, factors, h, w, tuple(script), rec, frozenset(tags), 0))

    # deep and bands under every layout; between them every size but the largest
    sizes = {"deep": ((40, 56), (9, 17), (72, 88), (40, 56), (72, 88), (40, 56), (72, 88)),
             "bands": ((72, 88), (40, 56), (8, 8), (9, 17), (40, 56), (72, 88), (40, 56))}
    for sname, script in (("deep", deep()), ("bands", bands())):
        for (lname, factors), (h, w) in zip(LAYOUTS, sizes[sname]):
            add(f"{sname}-{lname}-{h}x{w}", script, factors, h, w, sname)
    add("bands-420-1x1", bands(), F420, 1, 1, "bands")
    add("deep-444-1x1", deep(), F444, 1, 1, "deep")
    add("deep-420-200x264", deep(), F420, 200, 264, "deep", "large")
    # dense scans over tens of chunks: window refills, bytes read past the window
    add("spectral-only-444-200x264", spectral_only(), F444, 200, 264, "spectral-only", "large", source=R, src_file=rnd)
    add("spectral-only-420-9x17", spectral_only(), F420, 9, 17, "spectral-only")
    add("shuffled-422-72x88", shuffled(), F422, 72, 88, "shuffled")
    add("sixtyfour-440-40x56", sixtyfour(), LAYOUTS[3][1], 40, 56, "sixtyfour")
    junk = tuple(255 - 3 * k for k in range(64))
    lq = (S.qtables[0], junk)
    add("latch-420-40x56", latch(S.qtables[1], junk), F420, 40, 56, "latch", qtables=lq, tq=(0, 1, 1))
    add("restarts-420-72x88", restarts(), F420, 72, 88, "restarts")
    add("restarts-411-40x56", restarts_interleaved(), LAYOUTS[4][1], 40, 56, "restarts")
    # the twin holds what the scans sent: chroma 10-63 zero, luma 10-63 without bit 0
    cut = [np.array(a) for a in S.coefs]
    cut[0][:, :, 10:] = np.sign(cut[0][:, :, 10:]) * (np.abs(cut[0][:, :, 10:]) >> 1 << 1)
    cut[1][:, :, 10:] = cut[2][:, :, 10:] = 0
    add("partial-444-40x56", partial(), F444, 40, 56, "partial", twin="baseline",
        twin_source=Source(tuple(cut), S.qtables, S.tq))
    for shname, shape in SHAPES.items():
        add(f"tables-{shname}-420-72x88", tables_script(), F420, 72, 88, "tables", shname, tables=shape)
    # one component
    G = Source(S.coefs[:1], S.qtables[:1], (0,))
    add("gray-9x17", gray_script(), ((1, 1),), 9, 17, "gray", source=G, twin="baseline")
    add("gray-72x88-runs", gray_script(), ((1, 1),), 72, 88, "gray", "runs", source=G, twin="baseline",
        tables=SHAPES["runs"])
    # EOB runs of category 14: 182 x 181 = 32942 blocks with every AC coefficient zero
    by, bx = np.indices((181, 182))
    ramp = np.zeros((181, 182, 64), np.int16)
    ramp[:, :, 0] = (3 * bx + 5 * by) % 121 - 60
    E = Source((ramp,), ((16,) * 64,), (0,))
    add("eob-max-gray-1448x1456", eob_max_script(), ((1, 1),), 1448, 1456, "eob-max", "large", source=E,
        twin="baseline")
    # long correction runs
    D = Source((dense_blocks(R.coefs[0]), R.coefs[1], R.coefs[2]), R.qtables, R.tq)
    add("dense-444-40x56", dense_script(), F444, 40, 56, "dense", source=D, twin="baseline")
    # mostly empty blocks: EOB runs of every length up to 7 are among the frequent symbols, so the
    # hostile shapes put EOBn on their 16-bit codes
    by, bx = np.indices(S.coefs[0].shape[:2])
    keep = ((5 * bx + 3 * by) % 8 == 0) | ((bx + by) % 11 == 0)
    thin = [np.where(keep[:, :, None] | (np.arange(64) == 0), a, 0).astype(np.int16) for a in S.coefs]
    T = Source(tuple(thin), S.qtables, S.tq)
    for shname in ("ones", "runs"):
        add(f"sparse-{shname}-444-72x88", deep(), F444, 72, 88, "sparse", shname, source=T, twin="baseline",
            tables=SHAPES[shname])
    assert len({c.name for c in cells}) == len(cells)
    return tuple(cells)


@functools.lru_cache(maxsize=None)
def refused_script_cells():
    """The refused cells (ScriptCell with the planner's status; the tag
    "pillow-refuses" where Pillow must refuse the file too)."""
    S = coefs_from_444(jr.layout_source())
    dc = (ALL, 0, 0, 0, 0)
    scripts = (
        ("cb5-at-al1", [dc, (0, 1, 63, 0, 0), (1, 1, 63, 0, 1), (1, 1, 4, 1, 0), (1, 6, 63, 1, 0), (2, 1, 63, 0, 0)],
         UNSUPPORTED, ()),
        ("cr-without-dc", [(0, 0, 0, 0, 0), (1, 0, 0, 0, 0)] + [(c, 1, 63, 0, 0) for c in ALL], UNSUPPORTED, ()),
        ("sixtyfive", sixtyfour(extra=True), UNSUPPORTED, ()),
        ("ah-not-al-plus-1", [(ALL, 0, 0, 0, 1)] + [(c, 1, 63, 0, 1) for c in ALL] +
         [(0, 1, 63, 2, 0), (1, 1, 63, 1, 0), (2, 1, 63, 1, 0), (ALL, 0, 0, 1, 0)], CORRUPT, ("pillow-refuses",)),
    )
    out = []
    for name, script, status, tags in scripts:
        rec = {}
        data = progressive(S.coefs, S.qtables, F444, 9, 17, script, tq=S.tq, record=rec)
        out.append(ScriptCell(name, data, None, F444, 9, 17, tuple(script), rec, frozenset(tags), status))
    return tuple(out)
