"""Fuzz of the host JPEG header planner under AddressSanitizer + UBSan (CPU).

The planner (lance-distributed-training_amd/csrc/ldt_plan.cpp: plan_batch over
walk_markers, build_huff, plan_progressive, then plan_layout / write_plan)
parses untrusted cell bytes on the product path and turns them into every
size and offset of the device workspace before anything reaches the GPU. This
test builds it alone for the CPU with ``-fsanitize=address,undefined``
(tests/fuzz/plan_fuzz.cpp calls the same plan_batch as libldt.so, each cell in
a heap buffer of exactly its size) and drives it with:

* targeted header corruptions (SOF/DHT/DQT/DRI/SOS fields), each rejected
  with the expected LDT_IMG_* code — and rejected by Pillow 12.2 too, except
  the one documented divergence (a baseline SOS with Ss != 0, which libjpeg
  decodes with a warning and this build reports as UNSUPPORTED);
* every truncation inside the headers (baseline and progressive files);
* random byte overwrites inside the marker segments of every golden image.

The test_batch_* tests plan one mixed batch (baseline, restart intervals,
gray, progressive, a repeated file, a truncated, an empty and a null cell) and
check the row statuses, the geometry against Pillow's reading of the files,
that no two rows share workspace memory, the decoder routing and destuff
chunks under each planning option, table dedupe, and the blob layout.

test_layout_cells_plan plans the layout cells of tests/jpeg_recode.py (4 to 10
blocks per MCU, chroma factors up to 4) with the three refused frames among
them: statuses, the per-MCU block tables, geometry, workspace, the fast 4:2:0
count.

Any sanitizer report fails the run (-fno-sanitize-recover=all, non-zero exit).
"""
import glob
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, REPO

NOT_JPEG, UNSUPPORTED, CORRUPT = 1, 2, 3
SRC = [os.path.join(REPO, "tests", "fuzz", "plan_fuzz.cpp"),
       os.path.join(REPO, "lance-distributed-training_amd", "csrc", "ldt_plan.cpp")]


def build_planner(tmp_path_factory):
    """The sanitized driver, built once per calling module: run(cells) -> statuses, run.exe."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("fuzz") / "plan_fuzz")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", *SRC, "-o", exe], check=True)

    def run(cells):
        inp = b"".join(struct.pack("<I", len(c)) + c for c in cells)
        r = subprocess.run([exe], input=inp, capture_output=True, timeout=300,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert r.returncode == 0 and not r.stderr, r.stderr.decode(errors="replace")[-4000:]
        out = [int(x) for x in r.stdout.split()]
        assert len(out) == len(cells)
        return out
    run.exe = exe
    return run


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return build_planner(tmp_path_factory)


def segments(b: bytes):
    """(marker, offset of 0xFF, length field) up to and including the first SOS."""
    i, out = 2, []
    while i + 4 <= len(b):
        m, L = b[i + 1], (b[i + 2] << 8) | b[i + 3]
        out.append((m, i, L))
        if m == 0xDA:
            break
        i += 2 + L
    return out


def _set(b: bytes, pos: int, val: int) -> bytes:
    x = bytearray(b)
    x[pos] = val
    return bytes(x)


def _pil_rejects(b: bytes) -> bool:
    from PIL import Image

    try:
        im = Image.open(io.BytesIO(b))
        im.load()
        return False
    except Exception:
        return True


def _golden(name):
    with open(os.path.join(GOLDEN, "jpeg", name), "rb") as f:
        return f.read()


def test_targeted_header_corruptions_rejected(planner):
    b = _golden("food_512x384_q75.jpg")
    seg = {m: (i, L) for m, i, L in reversed(segments(b))}  # first occurrence wins
    sof, sos, dht, dqt = seg[0xC0][0], seg[0xDA], seg[0xC4][0], seg[0xDB][0]
    x = bytearray(b)
    x[sof + 4 + 6 + 3 * 2] = x[sof + 4 + 6]  # component 3 reuses component 1's id
    dri = b[:sos[0]] + b"\xff\xdd\x00\x05\x00\x01\x00" + b[sos[0]:]  # DRI with length 5
    cases = {
        "sos_duplicate_selector": (_set(b, sos[0] + 4 + 1 + 2, b[sos[0] + 4 + 1]), {NOT_JPEG}),
        "sos_seglen_2": (b[:sos[0] + 2] + b"\x00\x02" + b[sos[0] + 4:], {NOT_JPEG}),
        "sos_ns_0": (_set(b, sos[0] + 4, 0), {NOT_JPEG}),
        "sof_precision_12": (_set(b, sof + 4, 12), {UNSUPPORTED}),
        "sof_ncomp_4": (_set(b, sof + 4 + 5, 4), {NOT_JPEG, UNSUPPORTED}),
        "sof_width_0": (_set(_set(b, sof + 7, 0), sof + 8, 0), {NOT_JPEG}),
        "sof_duplicate_id": (bytes(x), {NOT_JPEG}),
        "dht_class_2": (_set(b, dht + 4, 0x20), {NOT_JPEG}),
        "dht_counts_over_256": (_set(b, dht + 4 + 1 + 15, 200), {NOT_JPEG}),
        "dqt_table_5": (_set(b, dqt + 4, 0x05), {NOT_JPEG}),
        "dri_length_5": (dri, {NOT_JPEG}),
    }
    names = list(cases)
    got = planner([cases[k][0] for k in names])
    for k, st in zip(names, got):
        assert st in cases[k][1], (k, st)
        assert _pil_rejects(cases[k][0]), k  # Pillow/libjpeg-turbo rejects it as well
    # documented divergence: baseline SOS with Ss = 1 (libjpeg warns and decodes)
    assert planner([_set(b, sos[0] + 2 + sos[1] - 3, 1)]) == [UNSUPPORTED]


@pytest.mark.parametrize("name", ["food_512x384_q75.jpg", "c4_375x500_q90_rst.jpg", "gray_77x91.jpg",
                                  "prog_375x500_q90.jpg", "prog_rst_250x333_q90.jpg"])
def test_every_header_truncation(planner, name):
    b = _golden(name)
    segs = segments(b)
    m, i, L = segs[-1]
    end = i + 2 + L  # end of the first SOS header
    cuts = [b[:k] for k in range(0, end)]
    got = planner(cuts)
    for k, st in enumerate(got):
        assert st != 0, (name, k)
        if not name.startswith("prog"):
            assert st == NOT_JPEG, (name, k, st)


def test_random_header_overwrites(planner):
    rng = np.random.default_rng(1234)
    cells = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "jpeg", "*.jpg"))):
        with open(path, "rb") as f:
            b = f.read()
        segs = segments(b)
        if not segs:
            continue
        lo, hi = 2, segs[-1][1] + 2 + segs[-1][2]
        for _ in range(120):
            x = bytearray(b)
            for _ in range(int(rng.integers(1, 5))):
                x[int(rng.integers(lo, hi))] = int(rng.integers(0, 256))
            cells.append(bytes(x))
            # also a length field pushed past the cell
            y = bytearray(b)
            m, i, L = segs[int(rng.integers(0, len(segs)))]
            y[i + 2:i + 4] = struct.pack(">H", int(rng.integers(0, 65536)))
            cells.append(bytes(y))
    got = planner(cells)
    assert all(0 <= s <= 5 for s in got)
    assert sum(1 for s in got if s != 0) > len(got) // 4  # the mutations do reach the checks


def _all_marker_segments(b: bytes):
    """(offset, length) of every marker segment with a length field in the
    file, including the DHT/SOS headers between progressive scans."""
    out, i = [], 2
    while i + 4 <= len(b):
        if b[i] == 0xFF and b[i + 1] not in (0x00, 0xFF, 0xD8, 0xD9, 0x01) and not 0xD0 <= b[i + 1] <= 0xD7:
            L = (b[i + 2] << 8) | b[i + 3]
            out.append((i, L))
            i += 2 + L
        else:
            i += 1
    return out


def test_progressive_scan_header_overwrites(planner):
    """plan_progressive walks every scan header of a SOF2 file: mutate the
    DHT / SOS segments between scans, and cut the file inside each of them."""
    rng = np.random.default_rng(99)
    cells = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "jpeg", "prog_*.jpg"))):
        with open(path, "rb") as f:
            b = f.read()
        segs = [s for s in _all_marker_segments(b) if s[0] > segments(b)[-1][1]]  # after the first SOS
        assert segs, path
        for (i, L) in segs:
            cells.append(b[:i + 2 + int(rng.integers(0, L + 1))])
            for _ in range(8):
                x = bytearray(b)
                x[i + 2 + int(rng.integers(0, L))] = int(rng.integers(0, 256))
                cells.append(bytes(x))
    got = planner(cells)
    assert all(0 <= s <= 5 for s in got)


def test_progressive_scan_ranges(planner):
    """plan_progressive's scan byte ranges (the SSE2 end-of-scan search) against
    a byte-by-byte restatement: the first 0xFF followed by a byte that is not
    0x00, 0xFF or RSTn ends a scan. Progressive goldens, synthetic images with
    restart intervals, and copies whose scans were salted with 0xFF 0x00 /
    0xFF 0xFF / 0xFF RSTn pairs at random offsets (16-byte-boundary cases
    included)."""
    import subprocess as sp

    from ldt_amd import synth

    def ref_ranges(b):
        out, i = [], 2
        while i + 4 <= len(b):
            if b[i] != 0xFF:
                return None
            while i + 1 < len(b) and b[i + 1] == 0xFF:
                i += 1
            m = b[i + 1]
            if m == 0xD9:
                break
            if m == 0x01 or 0xD0 <= m <= 0xD7:
                i += 2
                continue
            n = (b[i + 2] << 8) | b[i + 3]
            if m != 0xDA:
                i += 2 + n
                continue
            s0 = i + 2 + n
            j = s0
            while j + 1 < len(b) and not (b[j] == 0xFF and b[j + 1] not in (0x00, 0xFF) and not 0xD0 <= b[j + 1] <= 0xD7):
                j += 1
            out.append((s0, j - s0))
            i = j
        return out

    cells = [open(e, "rb").read() for e in sorted(glob.glob(os.path.join(GOLDEN, "jpeg", "*.jpg")))
             if "prog" in os.path.basename(e)]
    assert len(cells) >= 5
    cells += [synth.encode(synth.field(96 + 17 * k, 80 + 9 * k, k, 12.0), quality=90, progressive=True,
                           **({"restart_marker_blocks": 2} if k % 2 else {})) for k in range(6)]
    rng = np.random.default_rng(7)
    salted = []
    for b in cells[:6]:
        rr = ref_ranges(b)
        bb = bytearray(b)
        for (s0, ln) in rr:
            for _ in range(6):
                if ln < 40:
                    break
                p = s0 + int(rng.integers(2, ln - 4))
                if bb[p - 1] == 0xFF:
                    continue
                bb[p:p + 2] = bytes([0xFF, int(rng.choice([0x00, 0xFF, 0xD3]))])
        salted.append(bytes(bb))
    cells += salted
    inp = b"".join(struct.pack("<I", len(c)) + c for c in cells)
    r = sp.run([planner.exe], input=inp, capture_output=True, timeout=300,
               env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", PLAN_SCANS="1"))
    assert r.returncode == 0 and not r.stderr, r.stderr.decode(errors="replace")[-2000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(cells)
    checked = 0
    for b, line in zip(cells, lines):
        parts = line.split()
        if parts[-1] != "0":
            continue
        got = [tuple(int(x) for x in t.split(":")) for t in parts[:-1]]
        assert got == ref_ranges(b), (got[:3], ref_ranges(b)[:3])
        checked += 1
    assert checked >= len(cells) - len(salted)


# ---------------------------------------------------------------------------
# plan_batch over one mixed batch (the driver's PLAN_BATCH mode): the sizes and
# offsets the device workspace is built from, checked against the files.
# ---------------------------------------------------------------------------
LDT_IMG_NULL = 5
BATCH_FILES = ["food_512x384_q75.jpg", "c4_375x500_q90_rst.jpg", "gray_77x91.jpg", "prog_375x500_q90.jpg",
               "prog_rst_250x333_q90.jpg", "food_512x384_q75.jpg"]
N_OK = len(BATCH_FILES)
DS_CHUNK = 4096  # ldt_types.hpp kDsChunkBytes


def _batch_cells():
    cells = [_golden(n) for n in BATCH_FILES]
    sof = next(i for m, i, L in segments(cells[0]) if m == 0xC0)
    cells.append(cells[0][:sof + 4 + 5])  # cut in the middle of the SOF segment
    cells.append(b"")                     # zero-length cell
    cells.append(cells[2])                # its validity bit is clear
    return cells


def _parse_plan(text):
    def val(v):
        return [int(x) for x in v.split(",")] if "," in v else int(v)

    def fields(line):
        return {k: val(v) for k, v in (t.split("=") for t in line.split()[1:])}

    plan = {"rows": [], "segs": [], "pscans": [], "hashes": [], "text": text}
    for line in text.splitlines():
        kind = line.split()[0]
        if kind in ("row", "seg", "pscan"):
            plan[kind + "s"].append(fields(line))
        elif kind in ("totals", "layout", "sizes"):
            plan[kind] = fields(line)
        elif kind == "hash":
            plan["hashes"].append(line.split()[1])
        else:
            plan[kind] = [int(x) for x in line.split()[1:]]
    return plan


@pytest.fixture(scope="module")
def batch_plans(planner):
    """The nine-row batch planned once per setting; every run is sanitized."""
    cells = _batch_cells()
    lead = b"\x00" * 37  # row 0 of the longer array, not part of the batch

    def run(cells, *args):
        inp = b"".join(struct.pack("<I", len(c)) + c for c in cells)
        r = subprocess.run([planner.exe, *args], input=inp, capture_output=True, timeout=300,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", PLAN_BATCH="1"))
        assert r.returncode == 0 and not r.stderr, r.stderr.decode(errors="replace")[-4000:]
        return _parse_plan(r.stdout.decode())

    v0 = "validity=ff00"  # rows 0..7 valid, row 8 null
    return {
        "cells": cells,
        "fused": run(cells, v0, "labels=1", "twice=1"),
        "off64": run([lead] + cells, "validity=ff01", "labels=1", "twice=1", "off64=1", "arr_offset=1"),
        "unfused": run(cells, v0, "labels=1", "fuse=0"),
        "win0": run(cells, v0, "labels=1", "win_cap=0"),
        "serial": run(cells, v0, "labels=1", "serial=1"),
    }


def _ceil(a, b):
    return -(-a // b)


def _region_bytes(src_len, nseg):
    return (src_len + 16 + 8 * nseg + 15) & ~15  # ldt_types.hpp destuff_region_bytes


def _expected_geometry(b):
    """ImgDesc geometry of a file from Pillow's view of its frame header."""
    from PIL import Image

    im = Image.open(io.BytesIO(b))
    w, h = im.size
    layers = im.layer  # (id, h, v, tq) per component
    ncomp = len(layers)
    # a single-component scan is not interleaved: one block per MCU whatever the factors
    hs = [1] if ncomp == 1 else [l[1] for l in layers]
    vs = [1] if ncomp == 1 else [l[2] for l in layers]
    hmax, vmax = max(hs), max(vs)
    mcux, mcuy = _ceil(w, 8 * hmax), _ceil(h, 8 * vmax)
    segs = segments(b)
    progressive = any(m == 0xC2 for m, i, L in segs)
    dri = [(b[i + 4] << 8) | b[i + 5] for m, i, L in segs if m == 0xDD]
    restart = dri[-1] if dri else 0
    pad = [0] * (3 - ncomp)
    return progressive, {
        "width": w, "height": h, "ncomp": ncomp, "mcux": mcux, "mcuy": mcuy,
        "bpm": sum(a * c for a, c in zip(hs, vs)),
        "ch": hs + pad, "cv": vs + pad,
        "hf": [hmax // a for a in hs] + pad, "vf": [vmax // a for a in vs] + pad,
        "plane_stride": [mcux * a * 8 for a in hs] + pad,
        "cdw": [_ceil(w * a, hmax) for a in hs] + pad, "cdh": [_ceil(h * a, vmax) for a in vs] + pad,
        # progressive images have no baseline segments (k_prog walks their scans)
        "nseg": 0 if progressive else (_ceil(mcux * mcuy, restart) if restart else 1),
    }


def _disjoint_inside(ranges, total):
    ranges = sorted(ranges)
    assert all(lo >= 0 and hi > lo for lo, hi in ranges), ranges
    assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:])), ranges
    assert ranges[-1][1] <= total, (ranges, total)


def test_batch_row_statuses(batch_plans):
    for key in ("fused", "off64", "unfused", "win0", "serial"):
        st = [r["status"] for r in batch_plans[key]["rows"]]
        assert len(st) == 9, (key, st)
        assert st[:6] == [0] * 6, (key, st)
        assert st[6] == NOT_JPEG and st[7] != 0 and st[8] == LDT_IMG_NULL, (key, st)
        assert sum(1 for s in st if s == 0) == N_OK
        assert batch_plans[key]["totals"]["any_bad"] == 1


def test_batch_geometry_matches_pillow(batch_plans):
    cells, rows = batch_plans["cells"], batch_plans["fused"]["rows"]
    off = 0
    for i in range(N_OK):
        progressive, exp = _expected_geometry(cells[i])
        got = {k: rows[i][k] for k in exp}
        assert got == exp, (i, got, exp)
        if not progressive:  # the scan bytes: from the end of the SOS header to the end of the cell
            m, sos, L = segments(cells[i])[-1]
            assert (rows[i]["src_off"], rows[i]["src_len"]) == (off + sos + 2 + L, len(cells[i]) - (sos + 2 + L)), i
        off += len(cells[i])
    assert [i for i in range(N_OK) if _expected_geometry(cells[i])[0]] == batch_plans["fused"]["prog_img"]


def _check_rows_share_no_memory(plan, ok, key):
    """Coefficients, planes and destuffed streams of the rows `ok` are disjoint
    and inside the batch totals; the segments tile each baseline image's MCUs."""
    rows, tot = plan["rows"], plan["totals"]
    npad = {i: (rows[i]["mcux"] * rows[i]["mcuy"] * rows[i]["bpm"] + 63) & ~63 for i in ok}
    prog = plan["prog_img"]
    base = [i for i in ok if i not in prog]
    _disjoint_inside([(rows[i]["coef_off"], rows[i]["coef_off"] + npad[i]) for i in ok], tot["coef_blocks"])
    if prog:
        _disjoint_inside([(rows[i]["pcoef_off"], rows[i]["pcoef_off"] + npad[i]) for i in prog], tot["pcoef_blocks"])
    planes = [(r["plane_off"][k], r["plane_off"][k] + r["plane_stride"][k] * r["mcuy"] * r["cv"][k] * 8)
              for r in (rows[i] for i in ok) for k in range(r["ncomp"])]
    _disjoint_inside(planes, tot["plane_total"])
    _disjoint_inside([(rows[i]["dst_off"], rows[i]["dst_off"] + _region_bytes(rows[i]["src_len"], rows[i]["nseg"]))
                      for i in base], tot["dst_total"])
    # the segments tile each image's MCUs exactly, in row order
    assert len(plan["segs"]) == sum(rows[i]["nseg"] for i in ok)
    for i in ok:
        r = rows[i]
        segs = plan["segs"][r["seg_base"]:r["seg_base"] + r["nseg"]]
        first = 0
        for s in segs:
            assert s["img"] == i and s["mcu_first"] == first and s["mcu_count"] > 0, (key, i, s)
            first += s["mcu_count"]
        assert first == (r["mcux"] * r["mcuy"] if i in base else 0), (key, i)
    return planes, prog, base


def test_batch_rows_share_no_memory(batch_plans):
    for key in ("fused", "unfused", "serial"):
        planes, prog, base = _check_rows_share_no_memory(batch_plans[key], list(range(N_OK)), key)
        assert len(prog) == 2 and len(base) == 4
        assert len(planes) == 5 * 3 + 1


# ---------------------------------------------------------------------------
# The layout cells (tests/jpeg_recode.py layout_cells): 4 to 10 blocks per MCU,
# chroma factors up to 4 and unequal between Cb and Cr, with the three refused
# frames between them.
# ---------------------------------------------------------------------------
def _plan_batch(planner, cells, *args):
    inp = b"".join(struct.pack("<I", len(c)) + c for c in cells)
    r = subprocess.run([planner.exe, *args], input=inp, capture_output=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", PLAN_BATCH="1"))
    assert r.returncode == 0 and not r.stderr, r.stderr.decode(errors="replace")[-4000:]
    return _parse_plan(r.stdout.decode())


def test_layout_cells_plan(planner):
    import jpeg_recode as jr

    cells = list(jr.layout_cells())
    refused = jr.refused_cells()
    data = [c.data for c in cells]
    at = [3, len(cells) // 2, len(cells) + 1]  # rows of the refused frames in the batch
    for k, (name, b, _) in zip(at, refused):
        data.insert(k, b)
    ok = [i for i in range(len(data)) if i not in at]
    assert planner(data) == [UNSUPPORTED if i in at else 0 for i in range(len(data))]  # each cell alone
    for args in ((), ("serial=1",), ("fuse=0",), ("sb=64", "win_cap=0")):
        plan = _plan_batch(planner, data, *args)
        rows = plan["rows"]
        assert [r["status"] for r in rows] == [UNSUPPORTED if i in at else 0 for i in range(len(data))], args
        _check_rows_share_no_memory(plan, ok, args)
        assert sorted(plan["prog_img"]) == [i for i, c in zip(ok, cells) if "progressive" in c.tags]
    assert max(r["bpm"] for r in rows) == 10
    for i, c in zip(ok, cells):
        progressive, exp = _expected_geometry(data[i])
        got = {k: rows[i][k] for k in exp}
        assert got == exp, (c.name, got, exp)
        assert rows[i]["restart"] == (0 if "restart" not in c.tags else 1 if c.name.endswith("rst1") else 3), c.name
        assert rows[i]["color"] == (1 if c.rgb else 0), c.name
        # the MCU's blocks: component by component, each component's blocks row by row (T.81 A.2.3)
        order = [(ci, bx, by) for ci, (h, v) in enumerate(c.factors) for by in range(v) for bx in range(h)]
        assert list(zip(rows[i]["bcomp"], rows[i]["bdx"], rows[i]["bdy"])) == order, c.name
    # the fast 4:2:0 staging takes YCbCr 2x2; 1x1; 1x1 only: not the 9-block layouts, whose
    # one subsampled chroma plane is h2v2 as well, and not an RGB file
    fast = [c.name for c in cells if c.factors == jr.F420 and not c.rgb]
    assert len(fast) == 5 and plan["totals"]["n_fast420"] == len(fast)
    nine = [c.data for c in cells if sum(h * v for h, v in c.factors) == 9]
    assert len(nine) >= 2 * len(jr.LAYOUT_SIZES)
    assert _plan_batch(planner, nine)["totals"]["n_fast420"] == 0


def test_batch_routing_and_destuff_chunks(batch_plans):
    for key in ("fused", "unfused", "win0", "serial"):
        plan = batch_plans[key]
        rows, tot = plan["rows"], plan["totals"]
        base = [i for i in range(N_OK) if i not in plan["prog_img"]]
        assert len(plan["par_img"]) + tot["n_serial"] + len(plan["prog_img"]) == N_OK, key
        assert sorted(plan["par_img"] + plan["prog_img"]) == sorted(set(plan["par_img"] + plan["prog_img"]))
        assert all((rows[i]["sub_bits"] > 0) == (i in plan["par_img"]) for i in base), key
        # chunk_img is what ds_first / ds_count say, over every row
        chunks = []
        for i, r in enumerate(rows):
            assert r["ds_first"] == len(chunks), (key, i)
            chunks += [i] * r["ds_count"]
        assert chunks == plan["chunk_img"] and tot["n_chunks"] == len(chunks), key
        assert all(rows[i]["ds_count"] == 0 for i in range(9) if i not in base), key
        full = {i: _ceil(rows[i]["src_len"] + 3, DS_CHUNK) for i in base}
        region = {i: _region_bytes(rows[i]["src_len"], rows[i]["nseg"]) for i in base}
        if key in ("fused", "serial"):  # fuse_destuff on
            fits = [i for i in base if region[i] + 16 <= tot["win_bytes"]]
            assert all(rows[i]["ds_count"] == 0 for i in fits), key
            if key == "fused":  # the batch has images on both sides of the window
                assert fits and len(fits) < len(base)
                assert all(rows[i]["ds_count"] == full[i] for i in base if i not in fits)
                assert tot["n_ds_img"] == len(base) - len(fits)
        else:  # fuse_destuff off, or no window at all
            assert all(rows[i]["ds_count"] == full[i] for i in base), key
            assert tot["n_ds_img"] == len(base), key
        if key == "win0":
            assert tot["win_bytes"] == 0
        if key == "serial":
            assert plan["par_img"] == [] and tot["n_serial"] == len(base)
            assert tot["win_bytes"] == 0 and tot["n_ds_img"] == len(base)


def test_batch_dedupe_and_determinism(batch_plans):
    plan = batch_plans["fused"]
    a, b = plan["rows"][0], plan["rows"][5]
    assert (a["qt"], a["dct"], a["act"]) == (b["qt"], b["dct"], b["act"])
    # the same batch through the same lifetime cache: the same blob
    assert len(plan["hashes"]) == 2 and plan["hashes"][0] == plan["hashes"][1]
    # int32 offsets at arr_offset 0 and int64 offsets at arr_offset 1 of a longer array
    assert batch_plans["off64"]["text"] == plan["text"]


def test_batch_blob_layout(batch_plans):
    for key in ("fused", "unfused", "serial"):
        plan = batch_plans[key]
        lay, sz, tot = plan["layout"], plan["sizes"], plan["totals"]
        n = len(plan["rows"])
        sections = [("off_desc", sz["desc"] * n), ("off_seg", sz["seg"] * len(plan["segs"])),
                    ("off_huff", sz["huff"] * tot["nhuff"]), ("off_quant", 128 * tot["nquant"]),
                    ("off_lut", 3 * 256 * 4), ("off_labels", 8 * n), ("off_status", 4 * n),
                    ("off_par", 4 * len(plan["par_img"])), ("off_chunk", 4 * len(plan["chunk_img"])),
                    ("off_redo", 64), ("off_pscan", sz["pscan"] * len(plan["pscans"])),
                    ("off_ptab", sz["ptab"] * tot["nptab"]), ("off_pimg", 4 * len(plan["prog_img"]))]
        assert list(lay) == [s[0] for s in sections] + ["plan_bytes"]  # today's order
        end = 0
        for name, size in sections:  # each section starts where the one before it ends, 64-aligned
            assert lay[name] % 64 == 0 and lay[name] == end, (key, name, lay)
            end = (lay[name] + size + 63) & ~63
        assert lay["plan_bytes"] == end, (key, lay)
        offs = [lay[s[0]] for s in sections]
        if all(size > 0 for name, size in sections):
            assert all(x < y for x, y in zip(offs, offs[1:])), (key, offs)
        else:  # an empty section shares its offset with the next one
            assert key == "serial" and all(x <= y for x, y in zip(offs, offs[1:]))


# ---------------------------------------------------------------------------
# The device Huffman tables (the driver's PLAN_HUFF mode): every table the
# planner derives, entry by entry against a plain canonical decoder.
# ---------------------------------------------------------------------------
def _huff_check(planner, cells, *args):
    inp = b"".join(struct.pack("<I", len(c)) + c for c in cells)
    r = subprocess.run([planner.exe, *args], input=inp, capture_output=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0", PLAN_BATCH="1", PLAN_HUFF="1"))
    lines = r.stdout.decode().splitlines()
    bad = [x for x in lines if x.startswith("MISMATCH")]
    assert r.returncode == 0 and not r.stderr and not bad, (bad, r.stderr.decode(errors="replace")[-4000:])
    assert lines[-1].startswith("huff_ok")
    tabs = [{k: int(v) for k, v in (t.split("=") for t in x.split()[1:])} for x in lines if x.startswith("tab ")]
    plan = _parse_plan("\n".join(x for x in lines if not x.startswith(("tab ", "huff_ok"))))
    return plan, tabs


def test_device_huffman_tables_match_canonical_decoder(planner):
    """Every HuffTab of one batch of all golden files and all stress cells
    (tests/jpeg_recode.py): all 65,536 words through l1 / l2 / the canonical
    search, and every count-mode entry, against a canonical decoder built from
    the file's own DHT bytes. The stress tables reach what the standard tables
    do not: the canonical search (more than 8 long-code prefixes), all eight
    l2 chunks, l2 sub-codes of 1 to 5 bits, one-symbol tables, six tables in
    one image."""
    import jpeg_recode as jr

    golden = [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(GOLDEN, "jpeg", "*.jpg")))]
    assert len(golden) >= 10
    stress = jr.stress_cells()
    cells = golden + [c.data for c in stress]
    plan, tabs = _huff_check(planner, cells)
    rows = plan["rows"]
    assert len(rows) == len(cells) and all(r["status"] == 0 for r in rows)
    baseline = [i for i, r in enumerate(rows) if r["prog_count"] == 0]
    assert len(baseline) >= len(cells) - 10
    # each distinct table of the batch was checked exactly once
    assert sorted(t["idx"] for t in tabs) == list(range(plan["totals"]["nhuff"]))
    by_idx = {t["idx"]: t for t in tabs}
    n_one = 0
    for k, c in enumerate(stress):
        r = rows[len(golden) + k]
        if "progressive" in c.tags:
            continue
        ncomp = r["ncomp"]
        ac = [by_idx[i] for i in r["act"][:ncomp]]
        dc = [by_idx[i] for i in r["dct"][:ncomp]]
        if "deep" in c.tags or "edge9" in c.tags:  # over the l2 capacity: the canonical search
            assert all(t["prefixes"] > 8 and t["chunks"] == 0 and t["words_canon"] > 0 and t["words_l2"] == 0
                       for t in ac), (c.name, ac)
        if "edge8" in c.tags or "edge9" in c.tags:  # the DC tables fill all eight chunks
            assert all(t["prefixes"] == 8 and t["chunks"] == 8 and t["words_canon"] == 0 for t in dc), (c.name, dc)
        if "edge8" in c.tags:
            assert all(t["prefixes"] == 8 and t["chunks"] == 8 and t["words_l2"] == 256 for t in ac), (c.name, ac)
        if "split" in c.tags:
            assert len(set(r["act"][:ncomp] + r["dct"][:ncomp])) == 6, c.name
        if "deep" in c.tags:  # routed to the parallel decoder, whose rounds use the count-mode entries
            assert r["sub_bits"] > 0, (c.name, r["sub_bits"])
        n_one += sum(1 for t in ac + dc if t["nsym"] == 1)
    assert n_one >= 2  # the flat chroma planes of the optimised file: one DC and one AC symbol
    assert plan["totals"]["max_tabs"] == 6
    # a 16 KB window cap: the small cells are destuffed by the decoder in its LDS window (also
    # six-table ones), the big ones by the destuff kernels
    plan16, _ = _huff_check(planner, cells, "win_cap=16384")
    ds = {c.name: plan16["rows"][len(golden) + k]["ds_count"] for k, c in enumerate(stress)}
    assert plan16["totals"]["win_bytes"] == 16384 and plan16["totals"]["max_tabs"] == 6
    assert ds["deep-420-split"] == 0 and ds["ones-420"] == 0 and ds["deep-420-sof1"] == 0
    assert all(ds[c.name] > 2 for c in stress if "big" in c.tags)
    # the same tables whatever the decoder routing
    for args in (("serial=1",), ("sb=64", "win_cap=0")):
        plan2, tabs2 = _huff_check(planner, cells, *args)
        assert [(t["idx"], t["words_l2"], t["words_canon"]) for t in tabs2] == \
               [(t["idx"], t["words_l2"], t["words_canon"]) for t in tabs]
