"""The sync cache of k_huff_image on the GPU.

A cell decoded before skips phase 1 and the convergence rounds: its slots'
converged exits come from the device's table and the write pass proves them,
or the image is redone by the full path in the same launch. Whatever the
table holds, the output is the oracle's, bit for bit: every test here holds
its tensors against oracle.jpeg_to_tensor and reads the kernel's own counters
(LDT_OPT_SYNC_CACHE = 2) to see which path produced them. Every test clears
the table first.

Cells: the goldens, synth.q90_512(6) (one segment, ~500 slots each),
synth.imagenet_like(6) (restart segments) and jpeg_recode.sync_cells() at
LDT_OPT_SUBSEQ_BITS = 64 (streams that never resynchronise).
"""
import contextlib

import numpy as np
import pytest

import jpeg_recode as jr
from conftest import read_golden
from oracle import oracle
from test_gpu_parity import _batch, _check

pytestmark = pytest.mark.gpu

COUNTERS = ("hits", "misses", "inserts", "refused", "rejected", "fallbacks")


def _ctx():
    import torch

    from ldt_amd import _lib

    return _lib.get_context(torch.cuda.current_device()), _lib


@contextlib.contextmanager
def _options(**opts):
    """The shared context's options for the block; the defaults after it."""
    ctx, _lib = _ctx()
    defaults = {"OPT_SYNC_CACHE": 1, "OPT_SUBSEQ_BITS": 256, "OPT_SYNC_WARM": 0, "OPT_DEBUG_COUNTERS": 0}
    assert set(opts) <= set(defaults)
    try:
        for k, v in opts.items():
            ctx.set_option(getattr(_lib, k), v)
        yield ctx
    finally:
        for k, v in defaults.items():
            ctx.set_option(getattr(_lib, k), v)


def _decode(cells):
    import ldt_amd

    return ldt_amd.decode_tensor_image(_batch(cells))["image"].cpu().numpy()


def _counted(ctx, cells):
    """(tensors, what the decode added to the six counters)."""
    a = ctx.sync_cache_stats()
    out = _decode(cells)
    b = ctx.sync_cache_stats()
    d = {k: b[k] - a[k] for k in COUNTERS}
    print({k: v for k, v in d.items() if v})
    return out, d


@pytest.fixture(scope="module")
def groups(manifest):
    """name -> (cells, expected tensors, SUBSEQ_BITS), computed once."""
    from ldt_amd import synth

    sync = [c.data for c in jr.sync_cells()]
    g = {
        "golden": ([read_golden(e["file"]) for e in manifest["images"]], 256),
        "q90": (synth.q90_512(6, seed=5)[0], 256),
        "inet": (synth.imagenet_like(6, seed=5)[0], 256),
        "sync": (sync, 64),
    }
    return {k: (cells, [oracle.jpeg_to_tensor(b) for b in cells], bits) for k, (cells, bits) in g.items()}


def _check_all(out, exp, what):
    for k in range(len(exp)):
        _check(out[k], exp[k], f"{what}[{k}]")


@pytest.mark.parametrize("group", ["golden", "q90", "inet", "sync"])
def test_cold_then_warm(group, groups):
    cells, exp, bits = groups[group]
    with _options(OPT_SYNC_CACHE=2, OPT_SUBSEQ_BITS=bits) as ctx:
        ctx.sync_cache_clear()
        cold, c = _counted(ctx, cells)
        warm, w = _counted(ctx, cells)
        ctx.set_option(_ctx()[1].OPT_SYNC_CACHE, 0)
        off, o = _counted(ctx, cells)
    _check_all(cold, exp, f"{group} cold")
    _check_all(warm, exp, f"{group} warm")
    _check_all(off, exp, f"{group} off")
    users = c["hits"] + c["misses"]  # the images that take the fused parallel decoder
    assert users > 0 and c["fallbacks"] == 0 and c["rejected"] == 0, c
    if group == "q90":
        assert c == dict(hits=0, misses=6, inserts=6, refused=0, rejected=0, fallbacks=0), c
    assert c["inserts"] + c["refused"] <= c["misses"], c
    # (a repeated file in a batch shares one entry: it may hit on the cold call)
    assert w["hits"] == users and w["misses"] == 0, (c, w)
    assert w["fallbacks"] == 0 and w["rejected"] == 0 and w["inserts"] == 0, w
    assert all(v == 0 for v in o.values()), o


def test_geometry_is_part_of_the_key():
    """Small cells, so that LDT_OPT_SUBSEQ_BITS decides their S: entries made at
    one S serve no decode at another, and the phase-1 warm-up (which changes
    how the rounds get there, not where) shares them."""
    from ldt_amd import synth

    cells = [synth.encode(synth.field(96 + 8 * k, 128, 40 + k, 6.0), quality=90) for k in range(4)]
    cells.append(synth.encode(synth.field(120, 160, 50, 6.0), quality=90, restart_marker_rows=1))
    exp = [oracle.jpeg_to_tensor(b) for b in cells]
    n = len(cells)
    ctx, _lib = _ctx()
    with _options(OPT_SYNC_CACHE=2):
        ctx.sync_cache_clear()
        for bits, hits in ((256, 0), (64, 0), (256, n)):
            ctx.set_option(_lib.OPT_SUBSEQ_BITS, bits)
            out, d = _counted(ctx, cells)
            _check_all(out, exp, f"S from {bits}")
            assert d["hits"] == hits and d["misses"] == n - hits and d["fallbacks"] == 0 and d["rejected"] == 0, d
        for warm in (0, 50, 200):
            ctx.set_option(_lib.OPT_SYNC_WARM, warm)
            out, d = _counted(ctx, cells)
            _check_all(out, exp, f"warm {warm}")
            assert d["hits"] == n and d["misses"] == 0 and d["fallbacks"] == 0, (warm, d)
        # entries made under a warm-up serve the default
        ctx.sync_cache_clear()
        ctx.set_option(_lib.OPT_SYNC_WARM, 50)
        out, d = _counted(ctx, cells)
        assert d["inserts"] == n, d
        ctx.set_option(_lib.OPT_SYNC_WARM, 0)
        out, d = _counted(ctx, cells)
        _check_all(out, exp, "warm 50 -> 0")
        assert d["hits"] == n and d["fallbacks"] == 0 and d["rejected"] == 0, d


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_corrupted_entries_fall_back_and_are_repaired(mode, groups):
    """ldt_sync_cache_corrupt rewrites the READY payloads. The q90 cells have
    one segment of hundreds of slots, so every mode changes every entry in a
    way the decode must notice: the write pass's verification (modes 2 and 3;
    mode 1 too where the foreign payload passes the validation) or the
    validation itself (mode 4)."""
    cells, exp, _ = groups["q90"]
    n = len(cells)
    with _options(OPT_SYNC_CACHE=2) as ctx:
        ctx.sync_cache_clear()
        clean, c = _counted(ctx, cells)
        assert c["inserts"] == n, c
        assert ctx.sync_cache_corrupt(mode) == n
        out, d = _counted(ctx, cells)
        again, a = _counted(ctx, cells)
    _check_all(clean, exp, "clean")
    _check_all(out, exp, f"mode {mode}")
    _check_all(again, exp, f"mode {mode}, repaired")
    assert d["hits"] == n and d["misses"] == 0 and d["inserts"] == 0, d
    if mode == 1:
        assert d["fallbacks"] + d["rejected"] == n, d
    elif mode == 4:
        assert d["rejected"] == n and d["fallbacks"] == 0, d
    else:
        assert d["fallbacks"] == n and d["rejected"] == 0, d
    assert a == dict(hits=n, misses=0, inserts=0, refused=0, rejected=0, fallbacks=0), a


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("group", ["inet", "sync", "golden"])
def test_corrupted_entries_other_geometries(mode, group, groups):
    """Restart segments (single-slot segments, whose exit positions no write
    pass reads, so mode 2 may leave nothing to notice), never-resynchronising
    streams and the goldens: exact whatever the corruption does, at most one
    fallback or rejection per changed entry, and clean hits afterwards."""
    cells, exp, bits = groups[group]
    with _options(OPT_SYNC_CACHE=2, OPT_SUBSEQ_BITS=bits) as ctx:
        ctx.sync_cache_clear()
        _, c = _counted(ctx, cells)
        changed = ctx.sync_cache_corrupt(mode)
        out, d = _counted(ctx, cells)
        again, a = _counted(ctx, cells)
    users = c["hits"] + c["misses"]
    _check_all(out, exp, f"{group} mode {mode}")
    _check_all(again, exp, f"{group} mode {mode}, repaired")
    assert 0 <= changed <= c["inserts"], (changed, c)
    assert d["hits"] == users and d["fallbacks"] + d["rejected"] <= d["hits"], (changed, d)
    if mode == 4:
        assert d["rejected"] >= 1 and d["fallbacks"] == 0, d
    assert a["hits"] == users and a["fallbacks"] == 0 and a["rejected"] == 0 and a["misses"] == 0, a


def test_bad_cells_are_never_inserted(groups):
    import ldt_amd

    good = groups["q90"][0][0]
    deep = next(c for c in jr.stress_cells() if c.name == "deep-420")
    cut = deep.data[:len(deep.data) - len(jr.scan_bytes(deep.data)) // 2]
    bad = [read_golden("jpeg/bad_truncated.bin"), cut, good[:len(good) * 2 // 3]]
    with _options(OPT_SYNC_CACHE=2) as ctx:
        ctx.sync_cache_clear()
        rows = []
        for rnd in range(2):
            a = ctx.sync_cache_stats()
            with pytest.raises(ldt_amd.ImageDecodeError) as ei:
                _decode([good] + bad)
            b = ctx.sync_cache_stats()
            rows.append(ei.value.rows)
            # the good cell is inserted by the first call and hits in the second
            assert b["inserts"] - a["inserts"] == (1 if rnd == 0 else 0), (rnd, a, b)
            assert b["hits"] - a["hits"] == (0 if rnd == 0 else 1), (rnd, a, b)
            assert b["fallbacks"] == 0 and b["rejected"] == 0, b
        assert rows[0] == rows[1] and set(rows[0]) == {1, 2, 3}, rows
        out = _decode([good])
    _check(out[0], groups["q90"][1][0], "good cell after the bad ones")


def test_capacity_no_eviction():
    """1 MiB: 128 entries in 32 sets. 200 distinct cells: a full set refuses,
    nothing is evicted, and the residents keep hitting."""
    from ldt_amd import synth

    cells = [synth.encode(synth.field(64, 96, 1000 + k, 6.0), quality=90) for k in range(200)]
    exp = [oracle.jpeg_to_tensor(b) for b in cells[:3]]
    ctx, _lib = _ctx()
    try:
        ctx.set_option(_lib.OPT_SYNC_CACHE_MB, 1)
        with _options(OPT_SYNC_CACHE=2):
            ctx.sync_cache_clear()
            out, c = _counted(ctx, cells)
            st = ctx.sync_cache_stats()
            assert st["capacity"] == 128, st
            assert c["misses"] == 200 and c["inserts"] + c["refused"] == 200, c
            assert 0 < c["inserts"] <= 128 and c["refused"] >= 72, c
            for _ in range(2):
                out, d = _counted(ctx, cells)
                assert d["hits"] == c["inserts"] and d["misses"] == c["refused"], (c, d)
                assert d["inserts"] == 0 and d["refused"] == c["refused"] and d["fallbacks"] == 0, d
            _check_all(out[:3], exp, "capacity")
            ctx.set_option(_lib.OPT_SYNC_CACHE_MB, 0)  # too small for one set: no table, no counters
            out, d = _counted(ctx, cells[:3])
            _check_all(out, exp, "no table")
            assert all(v == 0 for v in d.values()) and ctx.sync_cache_stats()["bytes"] == 0
    finally:
        ctx.set_option(_lib.OPT_SYNC_CACHE_MB, 1024)


def test_concurrent_streams_share_the_table():
    """DecodePipeline(depth=3): three contexts and streams, one table. Two
    alternating batches from cold: inserts race with lookups of the same cells
    on other streams; every step is exact."""
    import torch

    import ldt_amd
    from ldt_amd import _lib, synth

    c0, l0 = synth.q90_512(8, seed=31)
    c1, l1 = synth.imagenet_like(8, seed=32)
    batches = [ldt_amd.ResidentBatch(c0, l0), ldt_amd.ResidentBatch(c1, l1)]
    with _options(OPT_SYNC_CACHE=0):
        ref = [b.decode() for b in batches]
        torch.cuda.synchronize()
    for k in (0, 7):
        _check(ref[0][0][k].cpu().numpy(), oracle.jpeg_to_tensor(c0[k]), f"ref q90[{k}]")
        _check(ref[1][0][k].cpu().numpy(), oracle.jpeg_to_tensor(c1[k]), f"ref inet[{k}]")
    pipe = ldt_amd.DecodePipeline(depth=3)
    pipe.set_option(_lib.OPT_SYNC_CACHE, 2)
    ctx = pipe.ctxs[0]
    ctx.sync_cache_clear()
    a = ctx.sync_cache_stats()
    outs = [pipe.decode(batches[k % 2]) for k in range(12)]
    torch.cuda.synchronize()
    pipe.check()
    b = ctx.sync_cache_stats()
    for k, (img, lbl) in enumerate(outs):
        assert torch.equal(img, ref[k % 2][0]) and torch.equal(lbl, ref[k % 2][1]), k
    d = {k: b[k] - a[k] for k in COUNTERS}
    print(d)
    assert d["hits"] + d["misses"] == 12 * 8, d
    assert d["fallbacks"] == 0 and d["rejected"] == 0, d
    assert d["hits"] >= 8 * 8, d  # from the fourth step of each batch at the latest


def test_debug_counters_bypass_the_cache(groups):
    cells, exp, _ = groups["q90"]
    with _options(OPT_SYNC_CACHE=2) as ctx:
        ctx.sync_cache_clear()
        _decode(cells)
        warm, w = _counted(ctx, cells)
        assert w["hits"] == len(cells), w
        ctx.set_option(_ctx()[1].OPT_DEBUG_COUNTERS, 1)
        out, d = _counted(ctx, cells)
        cnt = ctx.debug_counters()
    _check_all(out, exp, "counters on")
    assert all(v == 0 for v in d.values()), d
    assert cnt[1] == len(cells) and cnt[2] >= len(cells), cnt  # the rounds ran
