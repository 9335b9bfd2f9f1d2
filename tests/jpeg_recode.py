"""Lossless Huffman re-coder for baseline JPEGs, and the stress cells built
with it (a test helper: tests import it, nothing else does).

``recode`` takes a baseline Pillow JPEG (SOF0, one interleaved scan or
grayscale, with or without DRI), decodes its scan into the sequence of
(component, DC/AC, symbol, extra bits) with the file's own tables and emits
the same sequence under new Huffman tables: new DHT segments, new Td/Ta
selectors in the SOS, byte stuffing, 1-padding before each RSTn, EOI. Every
other segment stays byte for byte, so a decoder must produce the very same
pixels. It restates ITU T.81 Annex C (table derivation) and F.1.2 / F.2.2
(sequential entropy coding).

The new tables come from a ``shape(tc, histogram) -> (counts[16], symbols)``
function; the shapes below put an image's frequent symbols on the code paths
a standard (Annex K) table never reaches: long codes with many distinct
11-bit prefixes, codes of all ones, one-length codes. Every table is
validated the way libjpeg's jpeg_make_d_derived_tbl validates it, so a cell
can never carry a table Pillow would reject.

``reframe`` builds a baseline file with any sampling factors from the coded
blocks of a 4:4:4 file (no DCT: the blocks' symbols are emitted again in the
new MCU order, with the DC differences recomputed), and ``layout_cells`` the
cells of every MCU layout the planner accepts and Pillow never writes, with
the three frames it refuses (``refused_cells``).

``stress_cells`` builds the cells the stress tests share (re-coded images and
extreme files written by Pillow itself); the helpers at the end recompute a
file's properties (tables, long-code prefixes, stuffing density, symbol
sizes) from its bytes.

``sync_cells`` builds the streams on which the parallel decoder's guessed
starts meet the true trajectory late or never (flat images under ``zeros``,
textured ones, restart-segment geometries); tests/huffman_sync_model.py says
how many rounds each must take.
"""
import functools
import io
from collections import namedtuple

import numpy as np

LOOK_BITS = 11  # ldt_types.hpp kLookBits: the first-level lookup of the device tables


# ---------------------------------------------------------------------------
# parsing
# ---------------------------------------------------------------------------
def parse(jpeg: bytes):
    """([(marker, payload)] up to and including the first SOS, the bytes after it)."""
    assert jpeg[:2] == b"\xff\xd8", "no SOI"
    i, segs = 2, []
    while True:
        assert jpeg[i] == 0xFF, "marker expected"
        m, n = jpeg[i + 1], (jpeg[i + 2] << 8) | jpeg[i + 3]
        segs.append((m, bytes(jpeg[i + 4:i + 2 + n])))
        i += 2 + n
        if m == 0xDA:
            return segs, bytes(jpeg[i:])


def dht_tables(jpeg: bytes):
    """[(tc, th, counts[16], symbols)] of every DHT table before the first SOS."""
    out = []
    for m, p in parse(jpeg)[0]:
        s = 0
        while m == 0xC4 and s < len(p):
            counts = list(p[s + 1:s + 17])
            n = sum(counts)
            out.append((p[s] >> 4, p[s] & 15, counts, list(p[s + 17:s + 17 + n])))
            s += 17 + n
    return out


def canonical(counts, symbols):
    """T.81 C.2: [(symbol, length, code)] in table order."""
    out, code, k = [], 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out.append((symbols[k], length, code))
            code += 1
            k += 1
        code <<= 1
    return out


def validate_table(tc, counts, symbols, histogram=None):
    """The checks of jdhuff.c jpeg_make_d_derived_tbl (and of a usable
    encoder table); raises ValueError."""
    if len(counts) != 16 or sum(counts) != len(symbols) or not 1 <= len(symbols) <= 256:
        raise ValueError("bad counts")
    if len(set(symbols)) != len(symbols) or any(not 0 <= s <= 255 for s in symbols):
        raise ValueError("bad symbols")
    if tc == 0 and any(s > 15 for s in symbols):
        raise ValueError("DC symbol above 15")
    code = 0
    for length in range(1, 17):
        code += counts[length - 1]
        if counts[length - 1] and code >= (1 << length):  # Kraft sum exceeded, or the all-ones code
            raise ValueError("code of length %d overflows or is all ones" % length)
        code <<= 1
    if histogram is not None and not set(histogram) <= set(symbols):
        raise ValueError("an image symbol has no code")


Frame = namedtuple("Frame", "sof_marker precision height width comps restart sel n_mcu blocks")


def _frame(segs):
    sof = next((m, p) for m, p in segs if m in (0xC0, 0xC1))
    p = sof[1]
    nc = p[5]
    comps = [(p[6 + 3 * c], p[7 + 3 * c] >> 4, p[7 + 3 * c] & 15) for c in range(nc)]
    restart = 0
    for m, q in segs:
        if m == 0xDD:
            restart = (q[0] << 8) | q[1]
    sos = segs[-1][1]
    assert sos[0] == nc, "one scan with every component"
    sel = {sos[1 + 2 * k]: (sos[2 + 2 * k] >> 4, sos[2 + 2 * k] & 15) for k in range(nc)}
    h, w = (p[1] << 8) | p[2], (p[3] << 8) | p[4]
    if nc == 1:  # not interleaved: one block per MCU
        n_mcu, blocks = -(-w // 8) * -(-h // 8), [0]
    else:
        hm, vm = max(c[1] for c in comps), max(c[2] for c in comps)
        n_mcu = -(-w // (8 * hm)) * -(-h // (8 * vm))
        blocks = [ci for ci, c in enumerate(comps) for _ in range(c[1] * c[2])]
    return Frame(sof[0], p[0], h, w, comps, restart, sel, n_mcu, blocks)


def _intervals(ecs: bytes):
    """The destuffed restart intervals of the entropy-coded bytes (up to EOI)."""
    out, cur, i = [], bytearray(), 0
    while True:
        j = ecs.find(b"\xff", i)
        assert j >= 0 and j + 1 < len(ecs), "no EOI"
        cur += ecs[i:j]
        n = ecs[j + 1]
        if n == 0:
            cur.append(0xFF)
        elif 0xD0 <= n <= 0xD7:
            out.append(bytes(cur))
            cur = bytearray()
        elif n == 0xD9:
            out.append(bytes(cur))
            return out
        else:
            raise ValueError("marker %02X inside the scan" % n)
        i = j + 2


@functools.lru_cache(maxsize=None)
def scan_symbols(jpeg: bytes):
    """The scan as a tuple of restart intervals, each a tuple of
    (component, tc, symbol, extra-bit string) (T.81 F.2.2)."""
    segs, ecs = parse(jpeg)
    fr = _frame(segs)
    dec = {}
    for tc, th, counts, symbols in dht_tables(jpeg):
        codes = {format(code, "0%db" % length): sym for sym, length, code in canonical(counts, symbols)}
        dec[(tc, th)] = (codes, sorted({len(c) for c in codes}))
    out, done = [], 0
    for data in _intervals(ecs):
        bits = bin(int.from_bytes(b"\x01" + data, "big"))[3:]
        pos, syms = 0, []
        n = min(fr.restart, fr.n_mcu - done) if fr.restart else fr.n_mcu
        for _ in range(n):
            for ci in fr.blocks:
                td, ta = fr.sel[fr.comps[ci][0]]
                k = 0
                while k < 64:
                    tc = 0 if k == 0 else 1
                    codes, lengths = dec[(tc, ta if tc else td)]
                    for length in lengths:
                        sym = codes.get(bits[pos:pos + length])
                        if sym is not None:
                            break
                    else:
                        raise ValueError("no code at bit %d" % pos)
                    pos += length
                    size = sym if tc == 0 else sym & 15
                    syms.append((ci, tc, sym, bits[pos:pos + size]))
                    pos += size
                    if tc == 0:
                        k = 1
                    elif size == 0 and sym != 0xF0:
                        k = 64  # EOB
                    else:
                        k += 16 if size == 0 else (sym >> 4) + 1
        assert pos <= len(bits), "scan ran past its data"
        done += n
        out.append(tuple(syms))
    assert done == fr.n_mcu
    return tuple(out)


# ---------------------------------------------------------------------------
# re-coding
# ---------------------------------------------------------------------------
def recode(jpeg: bytes, shape, split_tables: bool = False, sof1: bool = False) -> bytes:
    """The same image under the Huffman tables ``shape(tc, histogram)`` gives.

    split_tables: one DC and one AC table per component (Th 0, 1, 2) instead
    of luma / chroma (Th 0, 1). sof1: the frame header becomes SOF1 (extended
    sequential, Huffman) and the highest table id becomes Th = 3."""
    segs, _ = parse(jpeg)
    fr = _frame(segs)
    assert fr.sof_marker == 0xC0 and fr.precision == 8, "baseline source expected"
    nc = len(fr.comps)
    th_of = [ci if split_tables else min(ci, 1) for ci in range(nc)]
    if sof1:
        top = max(th_of)
        th_of = [3 if t == top else t for t in th_of]
    intervals = scan_symbols(jpeg)
    hist = {}
    for syms in intervals:
        for ci, tc, sym, _ in syms:
            h = hist.setdefault((tc, th_of[ci]), {})
            h[sym] = h.get(sym, 0) + 1
    tables, enc = {}, {}
    for (tc, th), h in sorted(hist.items()):
        counts, symbols = shape(tc, h)
        counts, symbols = [int(c) for c in counts], [int(s) for s in symbols]
        validate_table(tc, counts, symbols, h)
        tables[(tc, th)] = (counts, symbols)
        enc[(tc, th)] = {sym: format(code, "0%db" % length) for sym, length, code in canonical(counts, symbols)}
    body = bytearray()
    for si, syms in enumerate(intervals):
        if si:
            body += bytes([0xFF, 0xD0 + (si - 1) % 8])
        bits = "".join([enc[(tc, th_of[ci])][sym] + extra for ci, tc, sym, extra in syms])
        bits += "1" * (-len(bits) % 8)
        if bits:
            body += int(bits, 2).to_bytes(len(bits) // 8, "big").replace(b"\xff", b"\xff\x00")
    out = bytearray(b"\xff\xd8")
    for m, p in segs:
        if m == 0xC4:
            continue
        if m == 0xC0 and sof1:
            m = 0xC1
        if m == 0xDA:
            d = b"".join(bytes([tc << 4 | th]) + bytes(c) + bytes(s) for (tc, th), (c, s) in sorted(tables.items()))
            out += b"\xff\xc4" + (len(d) + 2).to_bytes(2, "big") + d
            q = bytearray(p)
            for k in range(nc):
                ci = [c[0] for c in fr.comps].index(q[1 + 2 * k])
                q[2 + 2 * k] = th_of[ci] << 4 | th_of[ci]
            p = bytes(q)
        out += bytes([0xFF, m]) + (len(p) + 2).to_bytes(2, "big") + p
    return bytes(out + body + b"\xff\xd9")


# ---------------------------------------------------------------------------
# re-framing: the blocks of a 4:4:4 file under other sampling factors
# ---------------------------------------------------------------------------
def _dc_value(size: int, extra: str) -> int:
    """T.81 F.2.2.1 EXTEND."""
    if size == 0:
        return 0
    v = int(extra, 2)
    return v if v >= 1 << (size - 1) else v - (1 << size) + 1


def _dc_symbol(diff: int):
    """(size, extra-bit string) of a DC difference (T.81 F.1.2.1)."""
    size = abs(diff).bit_length()
    return size, format(diff if diff >= 0 else diff + (1 << size) - 1, "0%db" % size) if size else ""


@functools.lru_cache(maxsize=None)
def block_grids(jpeg444: bytes):
    """(blocks wide, blocks high, [grid of component 0, 1, 2]) of a baseline
    4:4:4 file; a grid maps (bx, by) to (absolute DC, ((AC symbol, extra bits), ...))."""
    fr = _frame(parse(jpeg444)[0])
    assert len(fr.comps) == 3 and all(c[1:] == (1, 1) for c in fr.comps), "4:4:4 source expected"
    bw, bh = -(-fr.width // 8), -(-fr.height // 8)
    grids, n = [{} for _ in range(3)], 0
    for syms in scan_symbols(jpeg444):
        pred = [0, 0, 0]  # reset at every restart interval
        for ci, tc, sym, extra in syms:
            if tc == 0:
                pred[ci] += _dc_value(sym, extra)
                cur = grids[ci][(n // 3) % bw, (n // 3) // bw] = [pred[ci], []]
                n += 1
            else:
                cur[1].append((sym, extra))
    assert n == 3 * bw * bh
    return bw, bh, [{k: (dc, tuple(ac)) for k, (dc, ac) in g.items()} for g in grids]


JFIF = b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"


def adobe(transform: int) -> bytes:
    """An APP14 Adobe segment (version 100, no flags) with the given colour transform."""
    return b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([transform])


def reframe(jpeg444: bytes, factors, height: int, width: int, restart: int = 0, app=JFIF,
            ids=(1, 2, 3)) -> bytes:
    """A baseline file of `width` x `height` whose components have the sampling
    factors ``factors = ((H, V) of Y, of Cb, of Cr)``, built from the coded
    blocks of a non-optimised 4:4:4 file (its Annex K tables carry every DC
    size, so the re-differenced DC values all have codes).

    Component c gets a grid of mcux * H_c by mcuy * V_c blocks, taken from the
    source component's grid and wrapped where the source is smaller. The file
    has the source's DQT and DHT segments, `app` (the bytes of the APPn
    segments, b"" for none), a new SOF0 with the component ids `ids`, a DRI if
    `restart` (in MCUs) is not 0, and one scan interleaved per T.81 A.2.3: DC
    differences per component, reset at each restart, byte stuffing, RSTn, EOI.
    Nothing checks that a decoder accepts the factors: refused frames are
    built the same way."""
    segs, _ = parse(jpeg444)
    fr = _frame(segs)
    assert fr.sof_marker == 0xC0 and fr.precision == 8, "baseline source expected"
    bw, bh, grids = block_grids(jpeg444)
    enc = {(tc, th): {sym: format(code, "0%db" % length) for sym, length, code in canonical(counts, symbols)}
           for tc, th, counts, symbols in dht_tables(jpeg444)}
    sel = [fr.sel[c[0]] for c in fr.comps]
    hmax, vmax = max(f[0] for f in factors), max(f[1] for f in factors)
    mcux, mcuy = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    body, bits, pred = bytearray(), [], [0, 0, 0]

    def flush():
        b = "".join(bits)
        b += "1" * (-len(b) % 8)
        if b:
            body.extend(int(b, 2).to_bytes(len(b) // 8, "big").replace(b"\xff", b"\xff\x00"))
        del bits[:]

    for m in range(mcux * mcuy):
        if restart and m and m % restart == 0:
            flush()
            body.extend(bytes([0xFF, 0xD0 + (m // restart - 1) % 8]))
            pred = [0, 0, 0]
        mx, my = m % mcux, m // mcux
        for ci, (h, v) in enumerate(factors):
            td, ta = sel[ci]
            for by in range(v):
                for bx in range(h):
                    dc, ac = grids[ci][(mx * h + bx) % bw, (my * v + by) % bh]
                    size, extra = _dc_symbol(dc - pred[ci])
                    pred[ci] = dc
                    bits.append(enc[0, td][size] + extra)
                    bits.extend(enc[1, ta][sym] + extra for sym, extra in ac)
    flush()
    out = bytearray(b"\xff\xd8" + app)
    for m, p in segs:
        if 0xE0 <= m <= 0xEF or m == 0xDD:
            continue
        if m == 0xC0:  # the source's quantisation table selectors
            p = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([3]) + b"".join(
                bytes([ids[ci], factors[ci][0] << 4 | factors[ci][1], p[8 + 3 * ci]]) for ci in range(3))
        if m == 0xDA:
            if restart:
                out += b"\xff\xdd\x00\x04" + restart.to_bytes(2, "big")
            p = bytes([3]) + b"".join(bytes([ids[ci], sel[ci][0] << 4 | sel[ci][1]]) for ci in range(3)) + b"\x00\x3f\x00"
        out += bytes([0xFF, m]) + (len(p) + 2).to_bytes(2, "big") + p
    return bytes(out + body + b"\xff\xd9")


# ---------------------------------------------------------------------------
# table shapes: shape(tc, histogram) -> (counts[16], symbols)
# ---------------------------------------------------------------------------
def _by_rarity(tc, hist, at_least=0):
    """The table's symbols, rarest first (ties by value); padded with valid
    symbols the image does not use (count 0, so they come first) up to
    `at_least`, which keeps a shape's structure on images with few symbols."""
    syms = sorted(hist, key=lambda s: (hist[s], s))
    if tc == 0:
        spare = [s for s in range(15, -1, -1) if s not in hist]
    else:  # run/size bytes with size 1..10, then ZRL and EOB
        spare = [r << 4 | s for r in range(15, -1, -1) for s in range(10, 0, -1) if r << 4 | s not in hist]
        spare += [s for s in (0xF0, 0x00) if s not in hist]
    pad = max(0, at_least - len(syms))
    assert pad <= len(spare)
    return sorted(spare[:pad]) + syms


def _table(lengths, symbols):
    """counts and canonical symbol order from one length per symbol (the
    symbols of one length keep their order)."""
    counts = [0] * 16
    for length in lengths:
        counts[length - 1] += 1
    order = sorted(range(len(symbols)), key=lambda i: lengths[i])
    return counts, [symbols[i] for i in order]


def _flat(symbols, length):
    assert len(symbols) < (1 << length)
    return _table([length] * len(symbols), symbols)


def _dc_flat(tc, hist, length):
    syms = _by_rarity(tc, hist)
    return _flat(syms, length if len(syms) < (1 << length) else length + 1)


def _dc_twelve(hist):
    """All 16 DC symbols at 12 bits: codes 0x000-0x00F, eight 11-bit prefixes
    with both halves of each in use (all eight l2 chunks of the device table)."""
    return _flat(_by_rarity(0, hist, at_least=16), 12)


def deep(tc, hist):
    """AC: the two rarest symbols at length 2, every other one at length 12,
    the most frequent last: the 12-bit codes run from 0x800 up, two per 11-bit
    prefix, so 24 symbols or more give more than 8 long-code prefixes and
    almost every symbol of the scan is a long code. DC: one length of 4-5 bits."""
    if tc == 0:
        return _dc_flat(tc, hist, 4)
    syms = _by_rarity(tc, hist, at_least=24)
    return _table([2, 2] + [12] * (len(syms) - 2), syms)


def _edge(tc, hist, extra):
    """AC: 20 (+ extra) long codes in one contiguous run that starts on an
    11-bit prefix boundary: 15 of 12 bits, one each of 13, 14 and 15 bits and
    2 + extra of 16 bits, 256 + extra sixteen-bit words, so exactly 8 prefixes
    and one more per started 32 words. The most frequent symbols take the long
    codes, dealt round over the five lengths (the most frequent one gets the
    last 16-bit code: with extra = 1 it is alone under the 9th prefix); every
    other symbol gets a 6-bit code (8 bits beyond 63 of them). DC: all 16 symbols at 12 bits."""
    if tc == 0:
        return _dc_twelve(hist)
    n_long = 20 + extra
    syms = _by_rarity(tc, hist, at_least=n_long + 1)
    short, hot = syms[:-n_long], syms[-n_long:][::-1]  # hot: most frequent first
    short_len = 6 if len(short) <= 63 else 8  # the long run starts at len(short) << (12 - short_len): even
    slots = {16: [], 12: [], 13: [], 14: [], 15: []}  # symbols per length, in canonical order
    room = {12: 15, 13: 1, 14: 1, 15: 1, 16: 2 + extra}
    k = 0
    while k < len(hot):
        for length in (16, 12, 13, 14, 15):
            if k < len(hot) and len(slots[length]) < room[length]:
                slots[length].append(hot[k])
                k += 1
    slots[16].reverse()  # the most frequent symbol last
    lengths, symbols = [short_len] * len(short), list(short)
    for length in (12, 13, 14, 15, 16):
        lengths += [length] * len(slots[length])
        symbols += slots[length]
    return _table(lengths, symbols)


def edge8(tc, hist):
    """Exactly kL2Chunks = 8 long-code prefixes: every l2 chunk in use."""
    return _edge(tc, hist, 0)


def edge9(tc, hist):
    """The 9th prefix that tips the table over to the canonical search."""
    return _edge(tc, hist, 1)


def ones(tc, hist):
    """Lengths 1..7 for the seven rarest symbols (0, 10, 110, ...), the most
    frequent symbol at 11111110 and every other one at 16 bits from 0xFF00:
    the scan is full of 1 bits, so of stuffed FF 00 pairs."""
    syms = _by_rarity(tc, hist)
    n = len(syms)
    if n <= 8:
        return _table(list(range(1, n + 1)), syms)
    return _table(list(range(1, 8)) + [16] * (n - 8) + [8], syms)


def flat8(tc, hist):
    """Every AC symbol at length 8 (up to the complete code less the all-ones
    word); DC symbols at one length of 5 bits."""
    if tc == 0:
        return _dc_flat(tc, hist, 5)
    return _flat(_by_rarity(tc, hist), 8)


def runs(tc, hist):
    """Lengths 1..k for the k rarest symbols and 2^(16-k) - 1 sixteen-bit
    codes that end at 0xFFFE, the most frequent symbol last (the table is
    padded with unused symbols to exactly that size): every symbol of the
    image is a 16-bit code that starts with k >= 11 ones, so whole bytes of
    ones follow each other and the stuffed FF 00 pairs come in runs."""
    most = 16 if tc == 0 else 162
    k = max(k for k in range(11, 16) if k + (1 << (16 - k)) - 1 >= min(len(hist) + 1, most) and
            k + (1 << (16 - k)) - 1 <= most)
    syms = _by_rarity(tc, hist, at_least=k + (1 << (16 - k)) - 1)
    assert len(syms) == k + (1 << (16 - k)) - 1, "more symbols than the shape holds"
    return _table(list(range(1, k + 1)) + [16] * (len(syms) - k), syms)


def zeros(tc, hist):
    """Lengths 1..n, the most frequent symbol first (0, 10, 110, ...): on a
    flat image DC size 0 and EOB are both the 1-bit code 0, so the scan is
    zero bits and a decoder at any bit position reads "DC 0, EOB" every 2
    bits. At most 16 symbols (a longer code does not exist)."""
    syms = sorted(hist, key=lambda s: (-hist[s], s))
    if len(syms) > 16:
        raise ValueError("zeros: %d symbols, the shape holds at most 16" % len(syms))
    return _table(list(range(1, len(syms) + 1)), syms)


SHAPES = {"deep": deep, "edge8": edge8, "edge9": edge9, "ones": ones, "flat8": flat8}


# ---------------------------------------------------------------------------
# properties of a file, from its bytes
# ---------------------------------------------------------------------------
def long_prefixes(counts) -> int:
    """Distinct LOOK_BITS-bit prefixes of the codes longer than LOOK_BITS bits."""
    pre = set()
    for _, length, code in canonical(counts, list(range(sum(counts)))):
        if length > LOOK_BITS:
            pre.add(code >> (length - LOOK_BITS))
    return len(pre)


def l2_widths(counts):
    """The numbers of bits after the 11-bit prefix among the long codes."""
    return sorted({length - LOOK_BITS for length in range(LOOK_BITS + 1, 17) if counts[length - 1]})


def scan_bytes(jpeg: bytes) -> bytes:
    """The entropy-coded bytes (stuffing and RSTn included, EOI not)."""
    ecs = parse(jpeg)[1]
    return ecs[:ecs.rindex(b"\xff\xd9")]


def stuffing_share(jpeg: bytes) -> float:
    """Stuffed FF 00 pairs per entropy-coded byte."""
    ecs = scan_bytes(jpeg)
    return ecs.count(b"\xff\x00") / len(ecs)


def max_sizes(jpeg: bytes):
    """(largest DC size, largest AC size) among the scan's symbols."""
    dc = ac = 0
    for syms in scan_symbols(jpeg):
        for _, tc, sym, _ in syms:
            if tc == 0:
                dc = max(dc, sym)
            else:
                ac = max(ac, sym & 15)
    return dc, ac


def frame_info(jpeg: bytes):
    """(SOF marker, [Pq of each DQT table])."""
    segs = parse(jpeg)[0]
    pq = []
    for m, p in segs:
        s = 0
        while m == 0xDB and s < len(p):
            pq.append(p[s] >> 4)
            s += 129 if p[s] >> 4 else 65
    return next(m for m, _ in segs if 0xC0 <= m <= 0xC2), pq


# ---------------------------------------------------------------------------
# the stress cells
# ---------------------------------------------------------------------------
# source: the file a re-coded cell must decode identically to (None: the cell
# is Pillow's own file); tags: what the cell is for (asserted by
# tests/test_jpeg_stress.py from the cell's bytes).
Cell = namedtuple("Cell", "name data source tags")


def _save(img, **kw) -> bytes:
    b = io.BytesIO()
    img.save(b, format="JPEG", **kw)
    return b.getvalue()


def _ycc(arr, **kw) -> bytes:
    """A (Y, Cb, Cr) array stored verbatim (Pillow does no colour conversion
    for a mode-"YCbCr" image)."""
    from PIL import Image

    arr = np.ascontiguousarray(arr, np.uint8)
    return _save(Image.frombytes("YCbCr", (arr.shape[1], arr.shape[0]), arr.tobytes()), **kw)


def corner_tiles() -> np.ndarray:
    """48x64 (Y, Cb, Cr) map of 16x16 tiles: the eight corners of the cube and
    four mid-luma / mid-chroma extremes, all far outside the RGB gamut."""
    tiles = [(y, cb, cr) for y in (0, 255) for cb in (0, 255) for cr in (0, 255)]
    tiles += [(128, 0, 255), (128, 255, 0), (255, 128, 0), (0, 128, 255)]
    a = np.zeros((48, 64, 3), np.uint8)
    for i, t in enumerate(tiles):
        a[(i // 4) * 16:(i // 4) * 16 + 16, (i % 4) * 16:(i % 4) * 16 + 16] = t
    return a


@functools.lru_cache(maxsize=None)
def stress_cells():
    """The stress cells, in a fixed order (a tuple of Cell)."""
    from PIL import Image

    from ldt_amd import synth

    rgb = lambda a, **kw: _save(Image.fromarray(np.ascontiguousarray(a)), **kw)
    cells = []

    def add(name, data, source=None, *tags):
        cells.append(Cell(name, data, source, frozenset(tags)))

    # 1. every shape on five kinds of baseline file
    sources = {
        "420": rgb(synth.field(64, 96, 7, 30.0), quality=90, subsampling="4:2:0"),
        "444": rgb(synth.field(96, 96, 8, 30.0), quality=90, subsampling="4:4:4"),
        "422": rgb(synth.field(40, 56, 9, 30.0), quality=85, subsampling="4:2:2"),
        "gray": rgb(synth.field(48, 64, 10, 30.0)[:, :, 0], quality=90),
        "rst3": rgb(synth.field(64, 96, 11, 30.0), quality=85, restart_marker_blocks=3),
    }
    for sname, src in sources.items():
        for shname, shape in SHAPES.items():
            add(f"{shname}-{sname}", recode(src, shape), src, shname)
    for sname in ("420", "444", "422", "rst3"):
        for shname in ("deep", "ones"):
            add(f"{shname}-{sname}-split", recode(sources[sname], SHAPES[shname], split_tables=True),
                sources[sname], shname, "split")
    add("deep-420-sof1", recode(sources["420"], deep, split_tables=True, sof1=True), sources["420"],
        "deep", "split", "sof1")
    # more than one 16 KB destuff tile of dense stuffing
    big = rgb(synth.field(128, 160, 12, 30.0), quality=90, subsampling="4:2:0")
    add("ones-big", recode(big, ones), big, "ones", "big")
    # runs of stuffed bytes, in a small file, over restart markers and over many tiles
    for sname, src in (("420", sources["420"]), ("rst3", sources["rst3"]), ("big", big)):
        add(f"runs-{sname}", recode(src, runs), src, "runs", *(["big"] if sname == "big" else []))
    # a progressive batch-mate from the split_tables source
    add("progressive-420", rgb(synth.field(64, 96, 7, 30.0), quality=90, subsampling="4:2:0", progressive=True),
        None, "progressive")

    # 2. extremes written by Pillow itself
    r = np.random.RandomState(21)
    for q in (50, 90, 100):
        add(f"optimize-q{q}", rgb(synth.field(64, 96, 13 + q, 40.0), quality=q, optimize=True), None, "optimize")
    chk = ((np.indices((64, 96)).sum(0) % 2) * 255).astype(np.uint8)
    two = np.stack([chk, chk, chk], -1)  # 2 grey levels: flat chroma planes
    add("optimize-flat-chroma", rgb(two, quality=90, subsampling="4:2:0", optimize=True), None,
        "optimize", "one-symbol")
    uni = r.randint(0, 256, (96, 96, 3)).astype(np.uint8)
    add("uniform-q100-444", rgb(uni, quality=100, subsampling="4:4:4"), None, "uniform")
    # 8x8 blocks in turn white, black and a 1-pixel checkerboard: DC differences
    # of +-2040 (size 11) next to AC coefficients of size 10
    by, bx = np.indices((96, 96)) // 8
    kind = (by + bx) % 3
    blk = np.where(kind == 0, 255, np.where(kind == 1, 0, ((np.indices((96, 96)).sum(0) % 2) * 255))).astype(np.uint8)
    add("checker-q100-444", rgb(np.stack([blk, blk, blk], -1), quality=100, subsampling="4:4:4"), None,
        "large-symbols")
    add("q1", rgb(synth.field(64, 96, 14, 30.0), quality=1), None, "q255")
    add("q5", rgb(synth.field(64, 96, 15, 30.0), quality=5), None, "q255")
    low = (128 + 20 * np.sin(np.arange(64)[:, None] / 9.0) + np.zeros((64, 96))).astype(np.uint8)
    low = np.stack([low, low, low], -1)
    add("qtables-16bit", rgb(low, qtables=[[16 * (i + 1) for i in range(64)]] * 2), None, "pq1")
    # the same tables on full-contrast content, 4:2:0: nonzero AC coefficients times quant values above 255
    add("qtables-16bit-uniform", rgb(uni, qtables=[[16 * (i + 1) for i in range(64)]] * 2, subsampling="4:2:0"),
        None, "pq1", "pq1-ac")
    add("qtables-ones", rgb(synth.field(40, 56, 16, 30.0), qtables=[[1] * 64] * 2), None, "q1s")
    rnd = r.randint(0, 256, (40, 56, 3)).astype(np.uint8)
    for aname, arr in (("corners", corner_tiles()), ("random", rnd)):
        for sub in ("4:4:4", "4:2:2", "4:2:0"):
            for q in (100, 90):
                add(f"ycc-{aname}-{sub.replace(':', '')}-q{q}", _ycc(arr, quality=q, subsampling=sub), None, "ycc")
    assert len({c.name for c in cells}) == len(cells)
    return tuple(cells)


# ---------------------------------------------------------------------------
# the layout cells: every MCU layout the planner accepts, and three it refuses
# ---------------------------------------------------------------------------
# factors are ((H, V) of Y, of Cb, of Cr)
LAYOUTS = (
    ("440", ((1, 2), (1, 1), (1, 1))),       # 4 blocks per MCU; chroma h1v2 fancy
    ("411", ((4, 1), (1, 1), (1, 1))),       # 6; box, hf 4
    ("1x4", ((1, 4), (1, 1), (1, 1))),       # 6; box, vf 4
    ("3x1", ((3, 1), (1, 1), (1, 1))),       # 5; box, hf 3
    ("1x3", ((1, 3), (1, 1), (1, 1))),       # 5; box, vf 3
    ("410", ((4, 2), (1, 1), (1, 1))),       # 10, the limit; box
    ("2x4", ((2, 4), (1, 1), (1, 1))),       # 10; box
    ("22-21-12", ((2, 2), (2, 1), (1, 2))),  # 8; Cb h1v2 fancy, Cr h2v1 fancy
    ("22-22-11", ((2, 2), (2, 2), (1, 1))),  # 9; Cb full size, Cr h2v2 fancy
    ("22-11-22", ((2, 2), (1, 1), (2, 2))),  # 9; Cb h2v2 fancy, Cr full size
    ("41-21-11", ((4, 1), (2, 1), (1, 1))),  # 7; Cb h2v1 fancy, Cr box
)
F420 = ((2, 2), (1, 1), (1, 1))
# (height, width): the downsampled width is <= 2 at the tiny ones, where h2v1 and h2v2 fall
# back to box and h1v2 does not, a one-row image has a single chroma row; a partial last MCU
# in both directions; whole MCUs
LAYOUT_SIZES = ((1, 1), (2, 3), (3, 2), (17, 5), (5, 17), (33, 40), (64, 96))
# frames the planner refuses (LDT_IMG_UNSUPPORTED): 12 blocks per MCU and a fractional ratio
# (Pillow refuses both), subsampled luma (Pillow decodes it: a pinned divergence)
REFUSED_LAYOUTS = (
    ("12-blocks", ((2, 2), (2, 2), (2, 2)), False),
    ("fractional", ((3, 1), (2, 1), (1, 1)), False),
    ("subsampled-luma", ((1, 1), (2, 2), (2, 2)), True),
)

# factors, ids: what the SOF says; rgb: libjpeg takes the components for R, G, B
LayoutCell = namedtuple("LayoutCell", "name data factors ids height width rgb tags")


def mcu_counts(factors, height: int, width: int):
    """(MCUs of an interleaved scan, [blocks of each component's own scan]) (T.81 A.2)."""
    hmax, vmax = max(f[0] for f in factors), max(f[1] for f in factors)
    return (-(-width // (8 * hmax)) * -(-height // (8 * vmax)),
            [-(-(-(-width * h // hmax)) // 8) * -(-(-(-height * v // vmax)) // 8) for h, v in factors])


def relabel_422_as_440(jpeg422: bytes) -> bytes:
    """The same bytes with luma's sampling factors 2x1 turned into 1x2: a
    valid 4:4:0 file (of another picture) wherever every scan has the same
    number of MCUs or blocks under both labels, which is asserted. Works for
    progressive files, whose scans the re-framer does not write."""
    i = 2
    while jpeg422[i + 1] not in (0xC0, 0xC2):
        i += 2 + ((jpeg422[i + 2] << 8) | jpeg422[i + 3])
    sof = jpeg422[i + 4:]
    height, width = (sof[1] << 8) | sof[2], (sof[3] << 8) | sof[4]
    f422 = tuple((sof[7 + 3 * c] >> 4, sof[7 + 3 * c] & 15) for c in range(sof[5]))
    assert f422 == ((2, 1), (1, 1), (1, 1)), f422
    assert mcu_counts(f422, height, width) == mcu_counts(LAYOUTS[0][1], height, width), \
        "the MCU or block counts differ at %dx%d" % (height, width)
    return jpeg422[:i + 11] + b"\x12" + jpeg422[i + 12:]


@functools.lru_cache(maxsize=None)
def layout_source() -> bytes:
    """The non-optimised 4:4:4 file whose blocks the layout cells are made of."""
    from PIL import Image

    from ldt_amd import synth

    return _save(Image.fromarray(synth.field(96, 96, 41, 30.0)), quality=90, subsampling="4:4:4")


@functools.lru_cache(maxsize=None)
def layout_cells():
    """The layout cells, in a fixed order (a tuple of LayoutCell), all at most 64x96."""
    from PIL import Image

    from ldt_amd import synth

    src = layout_source()
    cells = []

    def add(name, factors, h, w, *tags, rgb=False, ids=(1, 2, 3), data=None, **kw):
        data = reframe(src, factors, h, w, ids=ids, **kw) if data is None else data
        cells.append(LayoutCell(name, data, factors, ids, h, w, rgb, frozenset(tags)))

    for lname, factors in LAYOUTS:
        for h, w in LAYOUT_SIZES:
            add(f"{lname}-{h}x{w}", factors, h, w)
    # restart intervals of 1 and of 3 MCUs on the 5-, 7-, 9- and 10-block layouts
    by_name = dict(LAYOUTS)
    for lname in ("3x1", "41-21-11", "22-22-11", "410"):
        add(f"{lname}-33x40-rst1", by_name[lname], 33, 40, "restart", restart=1)
        add(f"{lname}-64x96-rst3", by_name[lname], 64, 96, "restart", restart=3)
    # progressive 4:4:0, from Pillow's own 4:2:2 scans
    for h, w in ((64, 64), (33, 40)):
        p422 = _save(Image.fromarray(synth.field(h, w, 43 + h, 30.0)), quality=90, subsampling="4:2:2",
                     progressive=True)
        add(f"440-{h}x{w}-progressive", by_name["440"], h, w, "progressive", data=relabel_422_as_440(p422))
    # colour spaces (jdapimin.c default_decompress_parms), subsampled both ways
    rgb_ids = (82, 71, 66)
    for lname, factors in (("420", F420), ("440", by_name["440"])):
        add(f"{lname}-adobe0", factors, 33, 40, "colour", rgb=True, app=adobe(0))
        add(f"{lname}-adobe1", factors, 33, 40, "colour", app=adobe(1))
        add(f"{lname}-rgb-ids-no-app", factors, 33, 40, "colour", rgb=True, app=b"", ids=rgb_ids)
        add(f"{lname}-rgb-ids-jfif", factors, 33, 40, "colour", ids=rgb_ids)
    add("420-adobe2", F420, 33, 40, "colour", app=adobe(2))
    add("420-jfif-adobe0", F420, 33, 40, "colour", app=JFIF + adobe(0))
    add("420-no-app", F420, 33, 40, "colour", app=b"")
    keep = _save(Image.fromarray(synth.field(33, 40, 47, 30.0)), quality=90, keep_rgb=True)
    add("pillow-keep-rgb", ((1, 1),) * 3, 33, 40, "colour", "pillow", rgb=True, ids=rgb_ids, data=keep)
    assert len({c.name for c in cells}) == len(cells)
    assert all(c.height <= 64 and c.width <= 96 for c in cells)
    return tuple(cells)


@functools.lru_cache(maxsize=None)
def refused_cells():
    """(name, data, Pillow decodes it) of the three frames the planner refuses."""
    return tuple((name, reframe(layout_source(), factors, 33, 40), pillow_decodes)
                 for name, factors, pillow_decodes in REFUSED_LAYOUTS)


# ---------------------------------------------------------------------------
# the sync cells: streams on which the parallel decoder's guesses meet the
# true trajectory late or never (tests/huffman_sync_model.py is the model)
# ---------------------------------------------------------------------------
SYNC_S = 96  # the planner's S for every sync cell under LDT_OPT_SUBSEQ_BITS = 64

# tags: what the cell is for; sub_bits, nseg: what the planner must say under subseq_bits = 64
SyncCell = namedtuple("SyncCell", "name data source tags sub_bits nseg")


def _flat_source(h, w, base, first, colour, restart_rows=0) -> bytes:
    """A flat image at grey level `base` whose first MCU of the image is at `first`."""
    from PIL import Image

    mcu = 16 if colour else 8
    a = np.full((h, w), base, np.uint8)
    a[:mcu, :mcu] = first
    kw = {"restart_marker_rows": restart_rows} if restart_rows else {}
    if colour:
        return _save(Image.fromarray(np.stack([a, a, a], -1)), quality=90, subsampling="4:2:0", **kw)
    return _save(Image.fromarray(a), quality=90, **kw)


def block_start_parities(jpeg: bytes):
    """Per restart segment, the set of p % 2 over the true trajectory's block
    starts (p, b, k = 0) in the segment's second half (its padding excluded)."""
    import huffman_sync_model as hm

    out = []
    for st in hm.streams(jpeg):
        par, s = set(), (0, 0, 0)
        while s[0] < st.bits - 8:
            if s[2] == 0 and s[0] >= st.bits // 2:
                par.add(s[0] % 2)
            s = st.step(*s)
        out.append(par)
    return out


def locked_levels(colour, restart, parity=1):
    """The first (base, first-MCU) grey levels, in a fixed order, for which
    every restart segment of the flat image re-coded under `zeros` has its
    block starts on bit parity `parity` (1: the other parity than every range
    start j*S, so no guess ever meets the truth). Searched on a small image
    of the same structure: the parity is that of the few symbols before the
    zero bits, whatever the size."""
    mcu = 16 if colour else 8
    for base in (128, 100, 160, 60, 200, 30, 230):
        for first in (16, 48, 80, 112, 144, 176, 208, 240):
            if first == base:
                continue
            small = recode(_flat_source(6 * mcu, 8 * mcu, base, first, colour, 2 if restart else 0), zeros)
            if all(p == {parity} for p in block_start_parities(small)):
                return base, first
    raise AssertionError("no levels give parity %d" % parity)


def _locked(h, w, colour, restart_rows=0) -> tuple:
    """(re-coded flat cell, its source): the levels searched, the parity asserted."""
    base, first = locked_levels(colour, restart_rows != 0)
    src = _flat_source(h, w, base, first, colour, restart_rows)
    data = recode(src, zeros)
    assert all(p == {1} for p in block_start_parities(data)), "block starts on the range starts' parity"
    return data, src


def _locked_with_slots(slots: int) -> tuple:
    """The grey locked cell of the fewest blocks (rows of at most 64) that has `slots` slots."""
    import huffman_sync_model as hm

    for n in range(max(1, (slots - 1) * SYNC_S // 2 - 32), slots * SYNC_S // 2 + 1):
        bw = next((d for d in range(min(n, 64), 0, -1) if n % d == 0 and n // d <= 4 * d), None)
        if bw is None:
            continue
        data, src = _locked(8 * (n // bw), 8 * bw, False)
        if hm.slot_counts(data, SYNC_S) == [slots]:
            return data, src
    raise AssertionError("no flat image has %d slots" % slots)


def _segment_bits(jpeg: bytes):
    """The destuffed length in bits of every restart segment."""
    return [8 * len(d) for d in _intervals(parse(jpeg)[1])]


def geometry_tags(jpeg: bytes, S: int = SYNC_S):
    """Which restart-segment geometries the file holds, from its bytes: a
    segment of exactly k*S bits, one of k*S + 8 (a last range of 8 bits), one
    shorter than S/3, one between S/3 and 2S/3."""
    bits = _segment_bits(jpeg)
    tags = set()
    if any(b % S == 0 for b in bits):
        tags.add("seg-kS")
    if any(b > S and b % S == 8 for b in bits):
        tags.add("seg-kS+8")
    if any(3 * b < S for b in bits):
        tags.add("seg-short")
    if any(S < 3 * b < 2 * S for b in bits):
        tags.add("seg-mid")
    return frozenset(tags)


def _ramp(h, w, seed, grey):
    """A field whose contrast grows from nothing (left) to full (right): with
    a restart marker per block its segments run from one byte to dozens."""
    from PIL import Image

    from ldt_amd import synth

    f = synth.field(h, w, seed, 1.0).astype(np.float32)
    amp = np.linspace(0, 1, w)[None, :, None] ** 2 * np.linspace(0.2, 1, h)[:, None, None]
    a = np.clip(128 + (f - 128) * amp * 0.5 + np.random.RandomState(seed).normal(0, 25, f.shape) * amp, 0, 255)
    a = a.astype(np.uint8)
    return Image.fromarray(a[:, :, 0] if grey else a)


@functools.lru_cache(maxsize=None)
def sync_cells():
    """The sync cells, in a fixed order (a tuple of SyncCell). Every one is
    planned with S = 96 under LDT_OPT_SUBSEQ_BITS = 64 (at most about 12 KB
    of scan), except the 257-segment cell, which the serial decoder takes.

    locked: flat images whose first MCU differs, re-coded under `zeros`; the
    true trajectory's block starts lie on the other bit parity than every
    range start, so no guess ever meets it and the truth moves one slot per
    round. zero-rounds: the even-parity twin. slow: textured images whose
    guesses converge over dozens of rounds, through the memo and work lists
    longer than a wave. seg-*: restart-segment geometries (geometry_tags);
    nseg256 / nseg257: the parallel decoder's segment limit and one beyond."""
    from PIL import Image

    from ldt_amd import synth

    cells = []

    def add(name, data, source, *tags, sub_bits=SYNC_S, nseg=1):
        cells.append(SyncCell(name, data, source, frozenset(tags), sub_bits, nseg))

    for slots in (2, 65, 66):
        data, src = _locked_with_slots(slots)
        add(f"locked-{slots}", data, src, "locked", f"slots{slots}")
    data, src = _locked(1424, 1440, True)
    add("locked-1000", data, src, "locked", "slots1000")
    # three segments of 100, 100 and 30 rows of 100 blocks: 209, 209 and 63 slots
    data, src = _locked(8 * 230, 800, False, restart_rows=100)
    add("locked-rst", data, src, "locked", "restart", nseg=3)
    base, first = locked_levels(False, False, parity=0)
    src = _flat_source(8 * 55, 8 * 56, base, first, False)
    add("even-twin", recode(src, zeros), src, "zero-rounds")

    field = synth.field(256, 256, 1)
    add("slow-std", _save(Image.fromarray(field), quality=60), None, "slow")
    src = _save(Image.fromarray(field), quality=30)
    add("slow-flat8", recode(src, flat8), src, "slow")
    quarter = np.full((256, 256, 3), 128, np.uint8)
    quarter[:64] = field[:64]
    add("slow-quarter", _save(Image.fromarray(quarter), quality=90), None, "slow")

    want = frozenset(("seg-kS", "seg-kS+8", "seg-short", "seg-mid"))
    for seed in range(5, 40):
        data = _save(_ramp(64, 128, seed, True), quality=90, restart_marker_blocks=1)
        if geometry_tags(data) == want:
            add("geometry-grey", data, None, *want, nseg=128)
            break
    else:
        raise AssertionError("no seed gives the four segment geometries")
    for seed in range(5, 40):
        data = _save(_ramp(64, 128, seed, False), quality=90, restart_marker_blocks=1)
        if want - {"seg-short"} <= geometry_tags(data):
            add("geometry-420", data, None, *geometry_tags(data), nseg=32)
            break
    else:
        raise AssertionError("no seed gives the segment geometries in 4:2:0")
    add("nseg-256", _save(_ramp(128, 128, 51, True), quality=90, restart_marker_blocks=1), None, "nseg256", nseg=256)
    add("nseg-257", _save(_ramp(8, 8 * 257, 52, True), quality=90, restart_marker_blocks=1), None, "nseg257",
        sub_bits=0, nseg=257)
    assert len({c.name for c in cells}) == len(cells)
    return tuple(cells)


# ---------------------------------------------------------------------------
# the twins: two files with the same scan bytes and the same length, so the
# same sync cache key (ldt_sync_cache.hpp sc_key), and other pixels
# ---------------------------------------------------------------------------
def strictly_valid(jpeg: bytes) -> bool:
    """A T.81 F.2.2 walk of a baseline file's scan under its own tables in
    which every code is a table code, no coefficient index passes 63, every
    MCU of every restart interval is there and fewer than 8 bits, all ones,
    remain after each interval's last MCU. What libjpeg decodes with a warning
    (a run past the block, data after the last MCU) is not strictly valid."""
    try:
        segs, ecs = parse(jpeg)
        fr = _frame(segs)
        dec = {}
        for tc, th, counts, symbols in dht_tables(jpeg):
            validate_table(tc, counts, symbols)
            codes = {format(code, "0%db" % length): sym for sym, length, code in canonical(counts, symbols)}
            dec[(tc, th)] = (codes, sorted({len(c) for c in codes}))
        intervals = _intervals(ecs)
    except (AssertionError, ValueError, IndexError, StopIteration):
        return False
    n_int = -(-fr.n_mcu // fr.restart) if fr.restart else 1
    if len(intervals) != n_int:
        return False
    done = 0
    for data in intervals:
        bits, pos = bin(int.from_bytes(b"\x01" + data, "big"))[3:], 0
        for _ in range(min(fr.restart, fr.n_mcu - done) if fr.restart else fr.n_mcu):
            for ci in fr.blocks:
                td, ta = fr.sel[fr.comps[ci][0]]
                k = 0
                while k < 64:
                    codes, lengths = dec[(1, ta) if k else (0, td)]
                    for length in lengths:
                        sym = codes.get(bits[pos:pos + length])
                        if sym is not None:
                            break
                    else:
                        return False
                    pos += length
                    if k == 0:
                        pos += sym
                        k = 1
                    elif sym == 0:
                        k = 64  # EOB
                    elif sym == 0xF0:
                        k += 16  # a coefficient must follow
                        if k > 63:
                            return False
                    else:
                        k += sym >> 4
                        if k > 63:
                            return False
                        pos += sym & 15
                        k += 1
                    if pos > len(bits):
                        return False
        if len(bits) - pos >= 8 or "0" in bits[pos:]:
            return False
        done += fr.restart
    return True


def _dht_value_offsets(jpeg: bytes):
    """{(tc, th): offset in the file of the table's first value byte}."""
    out, i = {}, 2
    while jpeg[i + 1] != 0xDA:
        n = (jpeg[i + 2] << 8) | jpeg[i + 3]
        if jpeg[i + 1] == 0xC4:
            s = i + 4
            while s < i + 2 + n:
                out[jpeg[s] >> 4, jpeg[s] & 15] = s + 17
                s += 17 + sum(jpeg[s + 1:s + 17])
        i += 2 + n
    return out


def swap_dht_symbols(jpeg: bytes, tc: int, th: int, a: int, b: int) -> bytes:
    """The same bytes with the symbols `a` and `b` of one DHT table exchanged
    in its value list. Both have the same size nibble, so every code keeps its
    length and every symbol its extra bits: all bit positions stay, the runs
    change, and with them the decoder's coefficient index at every boundary
    between subsequences.

    Whether the result is strictly valid depends on the file (a longer run may
    pass coefficient 63). The chroma-AC swaps that twin_cells uses are; the
    luma-AC swaps on 4:2:0 and 4:2:2 files are not, and on some of them the
    oracle differs from Pillow: that is libjpeg's warn-and-continue territory,
    which the project claims nothing about for baseline files, so no test uses
    them (tests/test_huffman_paths.py asserts strict validity of every twin)."""
    assert a & 15 == b & 15 and a != b
    tab = next((counts, symbols) for c, h, counts, symbols in dht_tables(jpeg) if (c, h) == (tc, th))
    off = _dht_value_offsets(jpeg)[tc, th]
    out = bytearray(jpeg)
    ia, ib = tab[1].index(a), tab[1].index(b)
    assert out[off + ia] == a and out[off + ib] == b
    out[off + ia], out[off + ib] = b, a
    return bytes(out)


def requantise_in_place(jpeg: bytes) -> bytes:
    """The same bytes with every DQT value but the first of each table raised
    or lowered by one: another picture from the very same Huffman walk."""
    out, i = bytearray(jpeg), 2
    while out[i + 1] != 0xDA:
        n = (out[i + 2] << 8) | out[i + 3]
        if out[i + 1] == 0xDB:
            s = i + 4
            while s < i + 2 + n:
                assert out[s] >> 4 == 0, "8-bit tables expected"
                for k in range(2, 65):
                    out[s + k] += 1 if out[s + k] < 255 and k % 2 else -1 if out[s + k] > 1 else 0
                s += 65
        i += 2 + n
    return bytes(out)


# same_walk: B's Huffman walk is A's (the cached states are B's own); otherwise
# only the bit positions are shared and the hints must be proven or dropped
Twin = namedtuple("Twin", "name a b same_walk")


@functools.lru_cache(maxsize=None)
def twin_cells():
    """The twins, in a fixed order (a tuple of Twin): equal length and equal
    scan bytes, so one sync cache key for two files."""
    from ldt_amd import synth

    f422 = synth.encode(synth.field(128, 128, 61, 6.0), quality=90, subsampling="4:2:2")
    twins = [Twin("relabel-440", f422, relabel_422_as_440(f422), True),
             Twin("requantised", f422, requantise_in_place(f422), True)]
    for h, w, q, ss, th, pair in ((512, 512, 90, "4:2:0", 1, (0x01, 0x11)),
                                  (96, 128, 90, "4:2:0", 1, (0x02, 0x12)),
                                  (64, 96, 75, "4:4:4", 0, (0x11, 0x21))):
        a = synth.encode(synth.field(h, w, 40, 6.0), quality=q, subsampling=ss)
        twins.append(Twin("swap-%dx%d-ac%d-%02x-%02x" % (h, w, th, *pair), a, swap_dht_symbols(a, 1, th, *pair), False))
    assert len({t.name for t in twins}) == len(twins)
    return tuple(twins)
