"""GPU decode of the layout cells (tests/jpeg_recode.py layout_cells): every
MCU layout the planner accepts and Pillow never writes -- 4:4:0, 4:1:1, 1x4,
factors of 3, 4:1:0 and 2x4 (10 blocks per MCU), chroma planes whose factors
differ (8, 9 and 7 blocks), from 1x1 to 64x96, with restart intervals of 1 and
3 MCUs, progressive 4:4:0, and the colour spaces libjpeg derives from JFIF /
Adobe / component ids. They exercise the per-MCU block tables, the DC
predictor scan per component, the IDCT's block placement, the packed-unit runs
at 5 and 7 to 10 blocks per MCU, and every branch of chroma_at (h2v1, h2v2 and
h1v2 fancy upsampling, box replication), in k_resize4's generic staging and in
the streaming kernel.

The bar is the project's: bit-exact against oracle.jpeg_to_tensor (max abs
<= 2/255 first), and against Pillow itself (oracle.pil_image_to_tensor).
tests/test_jpeg_stress.py asserts on the CPU that Pillow reads from each cell
the frame it is named for; tests/test_plan_fuzz.py checks their plans on the host.

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


@pytest.fixture(scope="module")
def layouts():
    """The cells with two files Pillow wrote among them, and each one's
    expected tensor, computed once."""
    from ldt_amd import synth

    cells = list(jr.layout_cells())
    std = [jr.Cell("pillow-420-q75", synth.encode(synth.field(96, 128, 51, 6.0)), None, frozenset()),
           jr.Cell("pillow-422-q90-rst", synth.encode(synth.field(64, 96, 52, 6.0), quality=90, subsampling="4:2:2",
                                                      restart_marker_rows=1), None, frozenset())]
    cells = cells[:len(cells) // 2] + std[:1] + cells[len(cells) // 2:] + std[1:]
    exp = {c.name: oracle.jpeg_to_tensor(c.data) for c in cells}
    return cells, exp


def _decode(cells, **kw):
    import ldt_amd

    return ldt_amd.decode_tensor_image(_batch([c.data for c in cells]), **kw)["image"].cpu().numpy()


def _check_all(out, cells, exp, what):
    assert len(out) == len(cells)
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
    """The batch from a cleared sync cache, then on its entries: both checked."""
    users = _users(cells, **kw)
    assert users > 0, what
    # (cells that share their scan bytes share an entry: deep-420-split and -sof1, the colour-space cells)
    dups = hp.key_dups([c.data for c in cells], **{k: v for k, v in kw.items() if k in ("bits", "mode")})
    runs = hp.cold_then_warm(_ctx()[0], lambda: _decode(cells), users=users, dups=dups, what=what)
    assert runs[1].d["hits"] == users and (dups or runs[0].d["inserts"] == users), (what, runs[0].d, runs[1].d)
    for run, path in zip(runs, ("cold", "warm")):
        assert run.rows == {}
        _check_all(run.out, cells, exp, f"{what}, {path}")
    return runs[0].out


def _blocks(c):
    return sum(h * v for h, v in c.factors) if hasattr(c, "factors") else 0


def test_one_440_cell_alone_first(layouts):
    """The smallest run of a layout no GPU test had: one 17x5 4:4:0 image
    (3 MCUs of 4 blocks, h1v2 fancy upsampling of 5x9 chroma planes)."""
    cells, exp = layouts
    c = next(c for c in cells if c.name == "440-17x5")
    out = _decode([c])
    _check(out[0], exp[c.name], c.name)
    assert np.array_equal(out[0], oracle.pil_image_to_tensor(c.data))


def test_mixed_batch_vs_oracle_and_pillow(layouts):
    """Every cell in one batch with two Pillow files: 4 to 10 blocks per MCU,
    baseline next to progressive, YCbCr next to RGB."""
    cells, exp = layouts
    out = _decode(cells)
    _check_all(out, cells, exp, "mixed")
    for k, c in enumerate(cells):  # Pillow itself
        assert np.array_equal(out[k], oracle.pil_image_to_tensor(c.data)), c.name
    nrm = _decode(cells, normalize=True)
    for k, c in enumerate(cells):
        _check(nrm[k], oracle.jpeg_to_tensor(c.data, normalize=True), f"normalize: {c.name}")


def test_each_cell_alone(layouts):
    cells, exp = layouts
    for c in cells:
        if "progressive" in c.tags:
            _check(hp.uncached(_ctx()[0], lambda: _decode([c]), what=f"alone: {c.name}").out[0], exp[c.name],
                   f"alone: {c.name}")
        else:
            _cold_then_warm([c], exp, f"alone: {c.name}")


@pytest.mark.parametrize("mode,bits", [(1, 256), (2, 64), (2, 256)])
def test_both_huffman_decoders(mode, bits, layouts):
    """The serial decoder and the parallel one: at 64-bit subsequences a
    10-block MCU spans many subsequences, and a wrong block or component
    sequence after a synchronisation point shows in the DC scan."""
    cells, exp = layouts
    ctx, _lib = _ctx()
    ctx.set_option(_lib.OPT_HUFF_MODE, mode)
    ctx.set_option(_lib.OPT_SUBSEQ_BITS, bits)
    try:
        if mode == 2:
            _cold_then_warm(cells, exp, f"mode{mode}/S{bits}", bits=bits, mode=mode)
        else:
            _check_all(hp.uncached(ctx, lambda: _decode(cells), what=f"mode{mode}/S{bits}").out, cells, exp,
                       f"mode{mode}/S{bits}")
        if mode == 2:  # the 5-, 7-, 8-, 9- and 10-block cells do run on the parallel decoder
            odd = [c for c in cells if _blocks(c) in (5, 7, 8, 9, 10) and "progressive" not in c.tags]
            assert {_blocks(c) for c in odd} == {5, 7, 8, 9, 10}
            ctx.set_option(_lib.OPT_DEBUG_COUNTERS, 1)
            _check_all(hp.uncached(ctx, lambda: _decode(odd), what=f"mode{mode}/S{bits} odd, counters").out, odd, exp,
                       f"mode{mode}/S{bits} 5 and 7-10 blocks")
            assert ctx.debug_counters()[1] == len(odd)
    finally:
        ctx.set_option(_lib.OPT_DEBUG_COUNTERS, 0)
        ctx.set_option(_lib.OPT_HUFF_MODE, 0)
        ctx.set_option(_lib.OPT_SUBSEQ_BITS, 256)


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("window", [0, -1])
def test_window_and_destuff_paths(window, fused, layouts):
    """The stream in the LDS window or in global memory, destuffed by the
    decoder itself or by the k_destuff_* kernels: equal to the default run
    and to the oracle. With the window and the fused destuff the cells consult
    the sync cache: cold, then hinted; every other combination never does."""
    cells, exp = layouts
    ctx, _lib = _ctx()
    default = _decode(cells)
    ctx.set_option(_lib.OPT_HUFF_WINDOW, window)
    ctx.set_option(_lib.OPT_FUSED_DESTUFF, fused)
    try:
        if window != 0 and fused:
            out = _cold_then_warm(cells, exp, f"window {window} fused {fused}", window=window)
        else:
            assert _users(cells, window=window, fused=fused) == 0
            out = hp.uncached(ctx, lambda: _decode(cells), what=f"window {window} fused {fused}").out
    finally:
        ctx.set_option(_lib.OPT_HUFF_WINDOW, -1)
        ctx.set_option(_lib.OPT_FUSED_DESTUFF, 1)
    assert np.array_equal(out, default)
    _check_all(out, cells, exp, f"window {window} fused {fused}")


def test_resize_implementations_agree(layouts):
    """k_resize4 (generic staging, and the 4:2:0 fast staging for the 4:2:0
    colour cells: packed at impl 0, 32-bit at impl 1) and the streaming
    kernel (impl 2) both call chroma_at: identical tensors, bit-exact vs the
    oracle. The 9-block layouts have one h2v2 chroma plane and one full-size
    one: they must not take the fast 4:2:0 staging, so a batch of them alone
    is the same under impl 0 and impl 1 and equals the oracle."""
    cells, exp = layouts
    nine = [c for c in cells if _blocks(c) == 9]
    assert {c.factors for c in nine} == {((2, 2), (2, 2), (1, 1)), ((2, 2), (1, 1), (2, 2))}
    ctx, _lib = _ctx()
    res, res9 = {}, {}
    try:
        for impl in (0, 1, 2):
            ctx.set_option(_lib.OPT_RESIZE_IMPL, impl)
            res[impl] = _decode(cells)
            res9[impl] = _decode(nine)
    finally:
        ctx.set_option(_lib.OPT_RESIZE_IMPL, 0)
    for impl in (0, 1, 2):
        _check_all(res[impl], cells, exp, f"resize impl {impl}")
        _check_all(res9[impl], nine, exp, f"resize impl {impl}, 9-block cells")
    assert np.array_equal(res[0], res[1]) and np.array_equal(res[0], res[2])
    assert np.array_equal(res9[0], res9[1]) and np.array_equal(res9[0], res9[2])


def test_refused_frames_between_good_cells(layouts):
    """12 blocks per MCU, a fractional ratio and subsampled luma: status 2 on
    that row only, and a clean batch of layout cells afterwards is bit-exact."""
    import ldt_amd

    cells, exp = layouts
    by_name = {c.name: c for c in cells}
    good = [by_name["410-33x40"], by_name["22-21-12-64x96"], by_name["41-21-11-33x40-rst1"], by_name["440-17x5"]]
    refused = jr.refused_cells()
    assert len(refused) == 3
    # from a cleared sync cache: the first failing call runs phase 1 and the rounds on its good rows
    _ctx()[0].sync_cache_clear()
    for k, (name, data, _) in enumerate(refused):
        batch = good[:k + 1] + [jr.Cell(name, data, None, frozenset())] + good[k + 1:]
        with pytest.raises(ldt_amd.ImageDecodeError) as ei:
            _decode(batch)
        assert ei.value.rows == {k + 1: 2}, name
        _check_all(_decode(good), good, exp, f"after {name}")
    nxt = [c for c in cells if c.name.endswith("-64x96") or "progressive" in c.tags]
    _cold_then_warm(nxt, exp, "after the refused frames")  # the table cleared again: two of `nxt` are in `good`
