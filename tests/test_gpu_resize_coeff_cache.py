"""GPU tests of the per-context cache of Pillow resample coefficient tables
that k_resize4 loads (one entry per input size, filled by k_fill_resample the
first time a batch brings the size): first use, reuse without a fill, mixed
sizes in one batch, a new size on a warm cache, the raw path, the option
paths (a tall image whose vertical coefficients are computed in the kernel,
LDT_OPT_RESIZE_IMPL 1 and 2) and independent contexts. Every result is
compared bit for bit with the CPU oracle."""
import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

SIZES = (8, 17, 223, 224, 225, 511, 512)  # up-scaling (3 taps), 224 +- 1, the fast path's 512 limit
SHAPES = ("4:2:0", "4:4:4", "grey")


def _cell(h, w, seed, shape="4:2:0", quality=90):
    from ldt_amd import synth

    img = synth.field(h, w, seed, 6.0)
    if shape == "grey":
        return synth.encode(img[..., 0].copy(), quality=quality)
    return synth.encode(img, quality=quality, subsampling=shape)


def _fresh_ctx():
    from ldt_amd import _lib

    return _lib.Context(0)


def _fills(ctx):
    return int(ctx.lib.ldt_debug_resample_fills(ctx.handle))


def _decode(cells, ctx=None):
    """float32 [n, 3, 224, 224] of the cells, on `ctx` (default: the shared one)."""
    import torch

    import ldt_amd

    out, _ = ldt_amd.ResidentBatch(cells, np.arange(len(cells))).decode(ctx=ctx)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def mixed():
    """21 cells: every size of SIZES as a width and as a height in each of the
    three shapes (width i pairs with height i + 2 k + 1 for shape k), and their
    oracle tensors."""
    cells = []
    for k, shape in enumerate(SHAPES):
        for i, w in enumerate(SIZES):
            h = SIZES[(i + 2 * k + 1) % len(SIZES)]
            cells.append(_cell(h, w, 500 + 10 * k + i, shape))
    return cells, [oracle.jpeg_to_tensor(c) for c in cells]


def test_first_use_and_reuse():
    """A fresh context fills the tables of 64 and 48 with the first batch and
    launches no fill for the second; both results equal the oracle."""
    cells = [_cell(48, 64, 40 + k) for k in range(4)]
    exp = [oracle.jpeg_to_tensor(c) for c in cells]
    ctx = _fresh_ctx()
    assert _fills(ctx) == 0
    a = _decode(cells, ctx)
    after_first = _fills(ctx)
    assert after_first == 1  # both sizes in one launch
    b = _decode(cells, ctx)
    assert _fills(ctx) == after_first
    for k in range(4):
        assert np.array_equal(a[k], exp[k]), f"first call, image {k}"
        assert np.array_equal(b[k], exp[k]), f"second call, image {k}"


def test_mixed_sizes_in_one_batch(mixed):
    """Widths and heights 8..512 in 4:2:0, 4:4:4 and grey: up-scaling (3 taps,
    both xmin clamps) to 7 taps, fast and generic staging in one batch. Each
    image alone (its own tap count sets the kernel) and in the batch (the
    widest image's tap count, the rows zero-padded)."""
    cells, exp = mixed
    ctx = _fresh_ctx()
    for k, c in enumerate(cells):
        assert np.array_equal(_decode([c], ctx)[0], exp[k]), f"image {k} alone"
    n = _fills(ctx)
    out = _decode(cells, ctx)
    assert _fills(ctx) == n  # every size was seen
    for k in range(len(cells)):
        assert np.array_equal(out[k], exp[k]), f"image {k} in the batch"
    cold = _decode(cells, _fresh_ctx())  # all sizes new in one batch
    assert np.array_equal(cold, out)


def test_new_size_after_warm_cache(mixed):
    cells, exp = mixed
    ctx = _fresh_ctx()
    first = _decode(cells[:7], ctx)
    n = _fills(ctx)
    new = _cell(200, 300, 77)
    assert np.array_equal(_decode([new, cells[0]], ctx)[0], oracle.jpeg_to_tensor(new))
    assert _fills(ctx) == n + 1
    again = _decode(cells[:7], ctx)
    assert _fills(ctx) == n + 1
    for k in range(7):
        assert np.array_equal(first[k], exp[k]) and np.array_equal(again[k], exp[k]), f"image {k}"


@pytest.mark.parametrize("h,w", [(1024, 1024), (230, 225)])
@pytest.mark.parametrize("normalize", [False, True])
def test_raw_path(h, w, normalize):
    """Raw uint8 HWC cells: 1024 x 1024 (11 taps; 16-byte aligned rows take
    k_resize4<1>) and 225 wide (k_resize4<3>), from a 16-byte aligned and from
    an odd address."""
    import torch

    import ldt_amd
    from ldt_amd import synth

    raw = synth.raw_hwc(2, h, w, seed=h + w)
    exp = [oracle.raw_to_tensor(raw[k], normalize=normalize) for k in range(2)]
    flat = torch.zeros(raw.size + 1, dtype=torch.uint8, device="cuda")
    for off in (0, 1):
        dev = flat[off:off + raw.size].view(2, h, w, 3)
        dev.copy_(torch.from_numpy(raw))
        assert dev.data_ptr() % 16 == (0 if off == 0 else 1)
        out = ldt_amd.resize_raw(dev, h, w, normalize=normalize).cpu().numpy()
        for k in range(2):
            assert np.array_equal(out[k], exp[k]), f"offset {off}, image {k}"


def test_option_paths():
    """A 5000-tall image (taller than the cache's limit: its vertical
    coefficients are computed in the kernel, with fewer waves per workgroup)
    next to cached sizes, and LDT_OPT_RESIZE_IMPL 1 (32-bit staging) and 2
    (streaming kernel): all equal the default run and the oracle."""
    from ldt_amd import _lib, synth

    ctx = _lib.get_context(0)
    tall = synth.encode(synth.field(5000, 512, 77, 6.0), quality=90)
    cells = [tall, _cell(512, 512, 78), _cell(375, 500, 79), _cell(48, 64, 80, "4:4:4")]
    base = _decode(cells)
    assert ctx.lib.ldt_debug_last_resize(ctx.handle) in (1, 2)
    for k, c in enumerate(cells):
        assert np.array_equal(base[k], oracle.jpeg_to_tensor(c)), f"image {k}"
    for impl in (1, 2):
        ctx.set_option(_lib.OPT_RESIZE_IMPL, impl)
        try:
            out = _decode(cells)
            small = _decode(cells[1:])
        finally:
            ctx.set_option(_lib.OPT_RESIZE_IMPL, 0)
        assert np.array_equal(out, base), f"RESIZE_IMPL {impl}"
        assert np.array_equal(small, base[1:]), f"RESIZE_IMPL {impl}, without the tall image"
    assert np.array_equal(_decode(cells[1:]), base[1:])
    assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 4


def test_contexts_keep_their_own_caches(mixed):
    """DecodePipeline(depth=3): three contexts on one device used in turn. Two
    batches of different sizes alternate, so the contexts meet the sizes in
    different orders; every result is correct, each context fills each size
    once, and none after it has seen both batches."""
    import torch

    import ldt_amd

    cells, exp = mixed
    groups = [(0, 7), (7, 21)]
    batches = [ldt_amd.ResidentBatch(cells[a:b], np.arange(a, b)) for a, b in groups]
    pipe = ldt_amd.DecodePipeline(depth=3)
    outs = [pipe.decode(batches[k % 2]) for k in range(6)]  # each context: both batches
    torch.cuda.synchronize()
    pipe.check()
    fills = [_fills(c) for c in pipe.ctxs]
    assert all(f >= 1 for f in fills), fills
    outs += [pipe.decode(batches[k % 2]) for k in range(6)]
    torch.cuda.synchronize()
    pipe.check()
    assert [_fills(c) for c in pipe.ctxs] == fills
    for k, (img, lbl) in enumerate(outs):
        a, b = groups[k % 2]
        img = img.cpu().numpy()
        assert lbl.cpu().numpy().tolist() == list(range(a, b))
        for j in range(b - a):
            assert np.array_equal(img[j], exp[a + j]), f"call {k}, image {a + j}"
