"""Which path of k_huff_image runs, pinned (tests/huff_paths.py).

A cell whose key is in the device's sync cache goes from setup straight to a
hinted write pass; any other runs phase 1 and the convergence rounds; the
serial decoder, global reads, the unfused destuff and the debug counters never
consult the table. Here:

* the census: one batch of five kinds of cell under every setting that
  decides the route; which images consulted the table is what
  huff_paths.cache_users says (the planner's rule, held against the planner
  by tests/test_huffman_paths.py), and every tensor is the oracle's;
* entries serve across the settings the key leaves out (alone / in a batch,
  the window size) and not across S;
* real foreign entries: twins of equal scan bytes and length (jpeg_recode.
  twin_cells; valid files by tests/test_huffman_paths.py), decoded A, B, A, B
  from a cleared table: B's first decode hits A's entry, and every tensor is
  that file's own;
* the census batch in two row orders and split into two calls.

Counts asserted are the relations of huff_paths or follow from the batch.
"""
import contextlib

import numpy as np
import pytest

import huff_paths as hp
import jpeg_recode as jr
from oracle import oracle
from test_gpu_parity import _batch, _check

pytestmark = pytest.mark.gpu

# every option the tests touch, with its default (LDT_OPT_SYNC_CACHE is huff_paths' business)
DEFAULTS = {"OPT_HUFF_MODE": 0, "OPT_SUBSEQ_BITS": 256, "OPT_HUFF_WINDOW": -1, "OPT_FUSED_DESTUFF": 1,
            "OPT_SYNC_WARM": 0, "OPT_DEBUG_COUNTERS": 0, "OPT_SYNC_CACHE_MB": 1024}

# name -> (the context's options, what huff_paths.cache_users is told, the cells that must consult the table)
PAR = ("q90-512", "inet", "small-64x96", "ones-big")  # all but the 257-segment cell
SETTINGS = {
    "default": ({}, {}, PAR),
    "warm50": ({"OPT_SYNC_WARM": 50}, {}, PAR),
    "warm200": ({"OPT_SYNC_WARM": 200}, {}, PAR),
    "bits64": ({"OPT_SUBSEQ_BITS": 64}, {"bits": 64}, PAR),
    "window16384": ({"OPT_HUFF_WINDOW": 16384}, {"window": 16384}, ("small-64x96",)),
    "window0": ({"OPT_HUFF_WINDOW": 0}, {"window": 0}, ()),
    "window-1": ({"OPT_HUFF_WINDOW": -1}, {"window": -1}, PAR),
    "unfused": ({"OPT_FUSED_DESTUFF": 0}, {"fused": 0}, ()),
    "serial": ({"OPT_HUFF_MODE": 1}, {"mode": 1}, ()),
    "counters": ({"OPT_DEBUG_COUNTERS": 1}, {"counters": 1}, ()),
    "cache-off": ({}, {"cache": 0}, ()),
    "cache-0-mb": ({"OPT_SYNC_CACHE_MB": 0}, {"cache_mb": 0}, ()),
}


def _ctx():
    import torch

    from ldt_amd import _lib

    return _lib.get_context(torch.cuda.current_device()), _lib


@contextlib.contextmanager
def _options(**opts):
    """The shared context's options set for the block, every one restored after it."""
    ctx, _lib = _ctx()
    assert set(opts) <= set(DEFAULTS)
    try:
        for k, v in opts.items():
            ctx.set_option(getattr(_lib, k), v)
        yield ctx
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(getattr(_lib, k), v)


def _decode(cells):
    import ldt_amd

    return ldt_amd.decode_tensor_image(_batch(cells))["image"].cpu().numpy()


def _check_all(out, exp, what):
    assert len(out) == len(exp)
    for k in range(len(exp)):
        _check(out[k], exp[k], f"{what}[{k}]")


@pytest.fixture(scope="module")
def census():
    """(names, cells, expected tensors) of the census batch, computed once."""
    cells = hp.census_cells()
    return list(cells), list(cells.values()), [oracle.jpeg_to_tensor(b) for b in cells.values()]


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_path_census(setting, census):
    """Which images consult the table under each setting: sc_use, pinned. A
    routing change that moves decodes to another path fails here."""
    names, cells, exp = census
    opts, kw, want = SETTINGS[setting]
    users = hp.cache_users(cells, **kw)
    assert {n for n, u in zip(names, users) if u} == set(want), (setting, users)
    with _options(**opts) as ctx:
        if want:
            runs = hp.cold_then_warm(ctx, lambda: _decode(cells), users=len(want), what=f"census {setting}")
            assert runs[0].d["inserts"] == runs[1].d["hits"] == len(want), runs
        else:
            runs = (hp.uncached(ctx, lambda: _decode(cells), what=f"census {setting}", cache=kw.get("cache", 2)),)
        if setting == "counters":
            cnt = ctx.debug_counters()
            assert cnt[1] == len(PAR), cnt  # the four went through k_huff_image, and through its rounds
    for run, path in zip(runs, ("cold", "warm")):
        assert run.rows == {}
        _check_all(run.out, exp, f"census {setting}, {path}")


def _step(ctx, cells, exp, what, **want):
    """One counted decode in a sequence (the caller holds LDT_OPT_SYNC_CACHE = 2):
    exact, no fallback, no rejection, and the counters named in `want`."""
    run = hp._counted(ctx, lambda: _decode(cells), what)
    assert run.rows == {}
    _check_all(run.out, exp, what)
    assert run.d["fallbacks"] == 0 and run.d["rejected"] == 0, (what, run.d)
    for k, v in want.items():
        assert run.d[k] == v, (what, k, v, run.d)
    return run


@contextlib.contextmanager
def _counting(**opts):
    """LDT_OPT_SYNC_CACHE = 2 over a cleared table for the block."""
    import torch

    ctx, _lib = _ctx()
    with _options(**opts):
        try:
            ctx.set_option(_lib.OPT_SYNC_CACHE, 2)
            torch.cuda.synchronize()
            ctx.sync_cache_clear()
            yield ctx
        finally:
            ctx.set_option(_lib.OPT_SYNC_CACHE, 1)


def test_entries_made_alone_serve_the_batch_and_the_reverse(census):
    """Neither the batch's window nor its table count is in the key."""
    names, cells, exp = census
    n = len(PAR)
    with _counting() as ctx:
        for k in range(len(cells)):
            u = int(names[k] in PAR)
            _step(ctx, [cells[k]], [exp[k]], f"alone first: {names[k]}", hits=0, misses=u, inserts=u)
        _step(ctx, cells, exp, "batch on the entries made alone", hits=n, misses=0, inserts=0)
        ctx.sync_cache_clear()
        _step(ctx, cells, exp, "batch first", hits=0, misses=n, inserts=n)
        for k in range(len(cells)):
            u = int(names[k] in PAR)
            _step(ctx, [cells[k]], [exp[k]], f"alone on the batch's entries: {names[k]}", hits=u, misses=0, inserts=0)


def test_entries_serve_across_window_sizes():
    """LDT_OPT_HUFF_WINDOW is not in the key: cells that fit a 16 KB window
    and the default one are served by entries made under either."""
    from ldt_amd import synth

    stress = {c.name: c for c in jr.stress_cells()}
    cells = [synth.encode(synth.field(96 + 8 * k, 128, 80 + k, 6.0), quality=90) for k in range(3)]
    cells += [synth.encode(synth.field(120, 160, 83, 6.0), quality=90, restart_marker_rows=1), stress["ones-420"].data,
              stress["deep-420-split"].data]
    n = len(cells)
    assert all(hp.cache_users(cells)) and all(hp.cache_users(cells, window=16384)) and hp.key_dups(cells) == 0
    exp = [oracle.jpeg_to_tensor(b) for b in cells]
    ctx, _lib = _ctx()
    for first, second in ((16384, -1), (-1, 16384)):
        with _counting(OPT_HUFF_WINDOW=first):
            _step(ctx, cells, exp, f"window {first} first", hits=0, misses=n, inserts=n)
            ctx.set_option(_lib.OPT_HUFF_WINDOW, second)
            _step(ctx, cells, exp, f"window {second} on the entries of {first}", hits=n, misses=0, inserts=0)


def test_entries_of_another_s_do_not_serve_many_slot_cells():
    """S is in the key: cells of hundreds of slots whose S LDT_OPT_SUBSEQ_BITS
    decides (96 under 64, 288 under 256) keep one entry per S."""
    sync = {c.name: c for c in jr.sync_cells()}
    cells = [sync["slow-std"].data, sync["locked-1000"].data, sync["locked-rst"].data]
    n = len(cells)
    assert [hp.routing(c, 64).sub_bits for c in cells] == [96] * n
    assert [hp.routing(c, 256).sub_bits for c in cells] == [288] * n
    assert all(hp.routing(c, 256).src_len * 8 // 288 >= 150 for c in cells)  # many slots at either S (480+ at 96)
    exp = [oracle.jpeg_to_tensor(b) for b in cells]
    ctx, _lib = _ctx()
    with _counting():
        for bits, hits in ((64, 0), (256, 0), (64, n), (256, n)):
            ctx.set_option(_lib.OPT_SUBSEQ_BITS, bits)
            _step(ctx, cells, exp, f"S from {bits}", hits=hits, misses=n - hits, inserts=n - hits)


@pytest.fixture(scope="module")
def twins():
    """The twins and each file's own expected tensor, computed once."""
    return [(t, oracle.jpeg_to_tensor(t.a), oracle.jpeg_to_tensor(t.b)) for t in jr.twin_cells()]


@pytest.mark.parametrize("k", range(5))
def test_twins_one_key_two_files(k, twins):
    """A, B, A, B from a cleared table: B's first decode is a hit on A's
    entry, a real foreign entry under B's key. With A's Huffman walk the hints
    are B's own: no fallback. With another walk over the same bit positions
    the write pass must prove the hints or drop them: at most one fallback or
    rejection per decode, and every tensor is that file's own oracle tensor,
    and the one the same call gives without the cache."""
    t, exp_a, exp_b = twins[k]
    assert not np.array_equal(exp_a, exp_b)
    seq = [("A", t.a, exp_a), ("B", t.b, exp_b), ("A again", t.a, exp_a), ("B again", t.b, exp_b)]
    off = [hp.uncached(_ctx()[0], lambda: _decode([cell]), what=f"twin {t.name} {who}, cache off", cache=0).out
           for who, cell, _ in seq[:2]]
    runs = []
    with _counting() as ctx:
        for who, cell, exp in seq:
            run = hp._counted(ctx, lambda: _decode([cell]), f"twin {t.name} {who}")
            assert run.rows == {}
            _check(run.out[0], exp, f"twin {t.name} {who}")
            runs.append(run)
    for j, run in enumerate(runs):
        assert np.array_equal(run.out, off[j % 2]), (t.name, j)
    d = [r.d for r in runs]
    assert d[0] == dict(hits=0, misses=1, inserts=1, refused=0, rejected=0, fallbacks=0), d[0]
    for j in (1, 2, 3):  # the collision is real: one key, and an entry under it
        assert d[j]["hits"] == 1 and d[j]["misses"] == 0 and d[j]["refused"] == 0, (t.name, j, d[j])
        if t.same_walk:
            assert d[j]["fallbacks"] == 0 and d[j]["rejected"] == 0 and d[j]["inserts"] == 0, (t.name, j, d[j])
        else:
            assert d[j]["fallbacks"] + d[j]["rejected"] <= 1, (t.name, j, d[j])


def test_twins_in_one_batch(twins):
    """Every twin pair side by side in one batch, twice: whichever workgroup
    of a key comes first, each row is its own file's tensor."""
    cells = [x for t, _, _ in twins for x in (t.a, t.b)]
    exp = [x for _, ea, eb in twins for x in (ea, eb)]
    with _counting() as ctx:
        for rep in range(2):
            run = hp._counted(ctx, lambda: _decode(cells), f"twins in one batch, call {rep}")
            assert run.rows == {}
            _check_all(run.out, exp, f"twins in one batch, call {rep}")
            assert run.d["hits"] + run.d["misses"] == len(cells), run.d
            assert run.d["fallbacks"] + run.d["rejected"] <= run.d["hits"], run.d


def test_order_independence(census):
    """The census batch cold in two row orders and split into two calls: each
    image's tensor is the same in all three, and inserts by one call serve
    the next."""
    names, cells, exp = census
    n = len(PAR)
    rev = list(range(len(cells)))[::-1]
    with _counting() as ctx:
        a = _step(ctx, cells, exp, "order: as listed", hits=0, misses=n, inserts=n).out
        ctx.sync_cache_clear()
        b = _step(ctx, [cells[i] for i in rev], [exp[i] for i in rev], "order: reversed", hits=0, misses=n,
                  inserts=n).out
        ctx.sync_cache_clear()
        c1 = _step(ctx, cells[:2], exp[:2], "order: first call", hits=0, misses=2, inserts=2).out
        # the second call holds the first call's first cell again: served by that call's insert
        c2 = _step(ctx, cells[2:] + cells[:1], exp[2:] + exp[:1], "order: second call", hits=1, misses=n - 2,
                   inserts=n - 2).out
    for i in range(len(cells)):
        assert np.array_equal(a[i], b[rev.index(i)]), names[i]
        assert np.array_equal(a[i], (c1[i] if i < 2 else c2[i - 2])), names[i]
    assert np.array_equal(c2[-1], a[0])
