"""GPU decode of the stress cells (tests/jpeg_recode.py): valid JPEGs whose
Huffman tables, symbol sizes, quantisation tables, byte stuffing and colours
sit where the suite's synth.field() images never go -- tables with more than
8 long-code prefixes (the canonical search of lookup_canon), exactly 8 (every
l2 chunk), six tables per image, SOF1 and Th = 3, one-symbol tables, AC size
10 and DC size 11, 16-bit quantisation tables, a stuffed FF 00 about every 12
bytes, and YCbCr far outside the RGB gamut.

The bar is the project's: bit-exact against oracle.jpeg_to_tensor (max abs
<= 2/255 first), and against Pillow itself (oracle.pil_image_to_tensor).
tests/test_jpeg_stress.py asserts on the CPU that each cell has the property
it is named for; tests/test_plan_fuzz.py checks their device tables on the host.

The decodes whose subject is the parallel decoder run from a cleared sync
cache and then on its entries, the configurations that never consult it are
held to that (tests/huff_paths.py).
"""
import numpy as np
import pytest

import huff_paths as hp
import jpeg_recode as jr
from oracle import oracle
from test_gpu_parity import _batch, _check

pytestmark = pytest.mark.gpu

WINDOW_SMALL = 16384  # LDS window cap (bytes) that most cells fit and the 4:4:4 and 128x160 cells do not


@pytest.fixture(scope="module")
def stress():
    """The cells plus two standard-table images, and each one's expected
    tensor, computed once."""
    from ldt_amd import synth

    cells = list(jr.stress_cells())
    std = [jr.Cell("standard-q75", synth.encode(synth.field(96, 128, 31, 6.0)), None, frozenset()),
           jr.Cell("standard-q90-rst", synth.encode(synth.field(64, 96, 32, 6.0), quality=90, restart_marker_rows=1),
                   None, frozenset())]
    cells = cells[:len(cells) // 2] + std[:1] + cells[len(cells) // 2:] + std[1:]
    exp = {c.name: oracle.jpeg_to_tensor(c.data) for c in cells}
    return cells, exp


def _decode(cells, **kw):
    import ldt_amd

    return ldt_amd.decode_tensor_image(_batch([c.data for c in cells]), **kw)["image"].cpu().numpy()


def _check_all(out, cells, exp, what):
    for k, c in enumerate(cells):
        _check(out[k], exp[c.name], f"{what}: {c.name}")


def _ctx():
    import torch

    from ldt_amd import _lib

    return _lib.get_context(torch.cuda.current_device()), _lib


def _users(cells, **kw):
    """How many of the cells consult the sync cache (huff_paths.cache_users)."""
    return sum(hp.cache_users([c.data for c in cells], **kw))


def _cold_then_warm(cells, exp, what, **kw):
    """The batch from a cleared sync cache, then on its entries: both checked.
    How many stress cells fit the window is the planner's business: the
    relations of huff_paths and at least one user, not a number."""
    users = _users(cells, **kw)
    assert users > 0, what
    # (cells that share their scan bytes share an entry: deep-420-split and -sof1, the colour-space cells)
    dups = hp.key_dups([c.data for c in cells], **{k: v for k, v in kw.items() if k in ("bits", "mode")})
    runs = hp.cold_then_warm(_ctx()[0], lambda: _decode(cells), users=users, dups=dups, what=what)
    assert runs[1].d["hits"] == users and (dups or runs[0].d["inserts"] == users), (what, runs[0].d, runs[1].d)
    for run, path in zip(runs, ("cold", "warm")):
        _check_all(run.out, cells, exp, f"{what}, {path}")
    return runs[0].out


def test_mixed_batch_vs_oracle_and_pillow(stress):
    """All cells in one batch: hostile and standard tables deduped into one
    plan, baseline next to progressive."""
    cells, exp = stress
    out = _decode(cells)
    _check_all(out, cells, exp, "mixed")
    for k, c in enumerate(cells):  # Pillow itself
        assert np.array_equal(out[k], oracle.pil_image_to_tensor(c.data)), c.name
    nrm = _decode(cells, normalize=True)
    for k, c in enumerate(cells):
        _check(nrm[k], oracle.jpeg_to_tensor(c.data, normalize=True), f"normalize: {c.name}")


def test_each_cell_alone(stress):
    cells, exp = stress
    for c in cells:
        if "progressive" in c.tags:
            _check(hp.uncached(_ctx()[0], lambda: _decode([c]), what=f"alone: {c.name}").out[0], exp[c.name],
                   f"alone: {c.name}")
        else:
            _cold_then_warm([c], exp, f"alone: {c.name}")


@pytest.mark.parametrize("mode,bits", [(1, 256), (2, 64), (2, 256)])
def test_both_huffman_decoders(mode, bits, stress):
    """The serial decoder and the parallel one; at 64-bit subsequences a
    12-bit code often straddles a subsequence boundary, where a wrong table
    entry corrupts the synchronisation rounds but not the serial decode."""
    cells, exp = stress
    ctx, _lib = _ctx()
    ctx.set_option(_lib.OPT_HUFF_MODE, mode)
    ctx.set_option(_lib.OPT_SUBSEQ_BITS, bits)
    try:
        if mode == 2:
            _cold_then_warm(cells, exp, f"mode{mode}/S{bits}", bits=bits, mode=mode)
        else:
            _check_all(hp.uncached(ctx, lambda: _decode(cells), what=f"mode{mode}/S{bits}").out, cells, exp,
                       f"mode{mode}/S{bits}")
        if mode == 2:  # the canonical-search cells do run on the parallel decoder
            deep = [c for c in cells if "deep" in c.tags]
            ctx.set_option(_lib.OPT_DEBUG_COUNTERS, 1)
            _check_all(hp.uncached(ctx, lambda: _decode(deep), what=f"mode{mode}/S{bits} deep, counters").out, deep,
                       exp, f"mode{mode}/S{bits} deep")
            assert ctx.debug_counters()[1] == len(deep)
    finally:
        ctx.set_option(_lib.OPT_DEBUG_COUNTERS, 0)
        ctx.set_option(_lib.OPT_HUFF_MODE, 0)
        ctx.set_option(_lib.OPT_SUBSEQ_BITS, 256)


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("window", [0, WINDOW_SMALL, -1])
def test_window_and_destuff_paths(window, fused, stress):
    """The stream in the LDS window or in global memory, destuffed by the
    decoder itself or by the k_destuff_* kernels: dense FF 00 through both
    byte classifiers, six-table images on both table paths. With the window
    and the fused destuff the fitting cells consult the sync cache: cold, then
    hinted; every other combination never does."""
    cells, exp = stress
    ctx, _lib = _ctx()
    default = _decode(cells)
    ctx.set_option(_lib.OPT_HUFF_WINDOW, window)
    ctx.set_option(_lib.OPT_FUSED_DESTUFF, fused)
    try:
        big = [c for c in cells if "big" in c.tags or "split" in c.tags]
        if window != 0 and fused:
            assert 0 < _users(cells, window=WINDOW_SMALL) < _users(cells)  # cells on both sides of the small window
            out = _cold_then_warm(cells, exp, f"window {window} fused {fused}", window=window)
            alone = _cold_then_warm(big, exp, f"window {window} fused {fused}, big and six-table cells", window=window)
        else:
            what = f"window {window} fused {fused}"
            assert _users(cells, window=window, fused=fused) == 0
            out = hp.uncached(ctx, lambda: _decode(cells), what=what).out
            alone = hp.uncached(ctx, lambda: _decode(big), what=f"{what}, big and six-table cells").out
    finally:
        ctx.set_option(_lib.OPT_HUFF_WINDOW, -1)
        ctx.set_option(_lib.OPT_FUSED_DESTUFF, 1)
    assert np.array_equal(out, default)
    _check_all(out, cells, exp, f"window {window} fused {fused}")
    _check_all(alone, big, exp, f"window {window} fused {fused}, big and six-table cells")


def test_resize_stagings_on_colour_extremes(stress):
    """Out-of-gamut YCbCr through the packed 16-bit 4:2:0 staging, the 32-bit
    staging and the banded kernel: identical, and bit-exact vs the oracle."""
    cells, exp = stress
    ycc = [c for c in cells if "ycc" in c.tags]
    assert len(ycc) == 12
    ctx, _lib = _ctx()
    res = {}
    try:
        for impl in (0, 1, 2):
            ctx.set_option(_lib.OPT_RESIZE_IMPL, impl)
            res[impl] = _decode(ycc)
    finally:
        ctx.set_option(_lib.OPT_RESIZE_IMPL, 0)
    for impl in (0, 1, 2):
        _check_all(res[impl], ycc, exp, f"resize impl {impl}")
    assert np.array_equal(res[0], res[1]) and np.array_equal(res[0], res[2])


def test_failing_neighbour_through_canonical_search(stress):
    """A deep cell cut in the middle of its scan, between two good stress
    cells: status 3 on its row only, and a clean batch afterwards is bit-exact.
    The sync cache is cleared before the failing call, so that call and the
    clean batch after it run phase 1 and the rounds; then the clean batch
    again, on its entries."""
    cells, exp = stress
    ctx, _ = _ctx()
    by_name = {c.name: c for c in cells}
    victim = by_name["deep-420"]
    cut = len(victim.data) - len(jr.scan_bytes(victim.data)) // 2
    bad = jr.Cell("deep-420-cut", victim.data[:cut], None, frozenset())
    failing = [by_name["deep-444-split"], bad, by_name["ones-420"]]
    # the cut row is status 3, never kept, and misses again on the warm call
    runs = hp.cold_then_warm(ctx, lambda: _decode(failing), users=_users(failing), what="failing neighbour")
    assert runs[0].rows == runs[1].rows == {1: 3}
    assert runs[0].d["inserts"] == runs[1].d["hits"] == _users(failing) - 1 and runs[1].d["misses"] == 1, runs
    # none of the clean batch's cells was in the failing call: cold on the table as that call left it
    nxt = [by_name["deep-420"], by_name["edge9-422"], by_name["ones-gray"], by_name["standard-q75"]]
    users = _users(nxt)
    assert users > 0
    for run, path in zip(hp.cold_then_warm(ctx, lambda: _decode(nxt), users=users, clear=False,
                                           what="after the failing neighbour"), ("cold", "warm")):
        assert run.rows == {}
        _check_all(run.out, nxt, exp, f"after the failing neighbour, {path}")
