"""GPU tests of the band kernel (k_resize4) without the work no output pixel
depends on: no clip8 on its tap sums, vertical taps in straight-line groups
that may run past a row's count on zero weights, scalar output addresses, and
boundary rows of a band (the first pair's row below the band's first source
row, the last pair's row at or past its end) neither loaded, staged nor
filtered. None of it may change a bit, so every case is the oracle's tensor
and the streaming kernel's (LDT_OPT_RESIZE_IMPL 2) bit for bit, and every case
asserts that the band kernel ran. Small batches at 8-row bands: source heights
whose bands start on odd and on even rows, with an odd row count from the even
row below, odd heights (the last pair has no second row), upscales (windows of
2-3 rows shared between bands), 5 and 6 taps, a height past the vertical table;
the packed and the 32-bit 4:2:0 staging, the generic one, raw rows aligned and
not, a generic output size and a formatted output; and saturated inputs, whose
outputs must be the LUT's end values where the oracle's are.
tools/checks/trim_check.cpp is the CPU side (tests/test_resize4_trim.py).
"""
import numpy as np
import pyarrow as pa
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

# (id, [(W, H, subsampling)], (out_h, out_w), resize impls: 0 packed staging, 1 32-bit staging)
JPEG_CASES = [
    ("down-5-6-taps", [(512, 512, "4:2:0"), (640, 640, "4:2:0"), (496, 511, "4:2:0"), (512, 640, "4:2:0")], (224, 224), (0, 1)),
    ("odd-heights", [(333, 501, "4:2:0"), (448, 449, "4:2:0"), (224, 225, "4:2:0"), (256, 255, "4:2:0")], (224, 224), (0, 1)),
    ("upscales", [(64, 17, "4:2:0"), (100, 33, "4:2:0"), (130, 100, "4:2:0"), (224, 50, "4:2:0")], (224, 224), (0, 1)),
    ("past-the-table", [(300, 1200, "4:2:0"), (200, 1121, "4:2:0"), (64, 1300, "4:2:0"), (128, 2000, "4:2:0")], (224, 224), (0,)),
    ("444+grey", [(500, 375, "4:4:4"), (320, 201, "grey"), (100, 33, "4:4:4"), (512, 512, "4:4:4")], (224, 224), (0,)),
    # 96 x 96 (the generic-size kernel): widths up to 480 (11 taps); heights with a table row (300) and without
    ("to-96x96", [(480, 512, "4:2:0"), (333, 501, "4:4:4"), (64, 17, "4:2:0"), (448, 481, "4:2:0"), (200, 300, "4:2:0")],
     (96, 96), (0, 1)),
]


def _cell(w, h, sub, seed):
    from ldt_amd import synth

    img = synth.field(h, w, seed, 6.0)
    if sub == "grey":
        return synth.encode(img[..., 0].copy(), quality=90)
    return synth.encode(img, quality=90, subsampling=sub)


def _ctx():
    import torch

    from ldt_amd import _lib

    return _lib.get_context(torch.cuda.current_device()), _lib


def _decode(cells, size, impl, **kw):
    """(images on the CPU, the band kernel's waves per workgroup or 0, its bands per image)."""
    import torch

    from ldt_amd import transforms as T

    ctx, _lib = _ctx()
    ctx.set_option(_lib.OPT_RESIZE_IMPL, impl)
    try:
        out = T.decode_arrow(pa.array(cells, pa.binary()), size=size, **kw)[0]
        torch.cuda.synchronize()
        took = ctx.lib.ldt_debug_last_resize(ctx.handle)
        bands = ctx.lib.ldt_debug_last_resize_bands(ctx.handle)
    finally:
        ctx.set_option(_lib.OPT_RESIZE_IMPL, 0)
    return out.cpu(), took, bands


def _band_rows(h, oh, bands):
    """(ya, yb) of each band of a height-h source: its first source row and one past its last."""
    _, bounds, _ = oracle.resample_coeffs(h, oh)
    bh = -(-oh // bands)
    rows = []
    for oy0 in range(0, oh, bh):
        last = min(oy0 + bh, oh) - 1
        rows.append((int(bounds[oy0, 0]), int(bounds[last, 0] + bounds[last, 1])))
    return rows


@pytest.fixture(scope="module")
def jpeg_cells():
    return {name: [_cell(w, h, sub, 1300 + 11 * k + h) for k, (w, h, sub) in enumerate(shapes)]
            for name, shapes, _, _ in JPEG_CASES}


@pytest.fixture(scope="module")
def jpeg_expected(jpeg_cells):
    """The oracle's tensors, computed once per case."""
    return {name: [oracle.jpeg_to_tensor(c, size[0], size[1]) for c in jpeg_cells[name]]
            for name, _, size, _ in JPEG_CASES}


@pytest.mark.parametrize("name,shapes,size,impl",
                         [(n, s, z, i) for n, s, z, impls in JPEG_CASES for i in impls],
                         ids=[f"{n}-impl{i}" for n, _, _, impls in JPEG_CASES for i in impls])
def test_band_kernel_equals_oracle_and_streaming(name, shapes, size, impl, jpeg_cells, jpeg_expected):
    assert 4 <= len(shapes) <= 8
    cells = jpeg_cells[name]
    for c, (w, h, _) in zip(cells, shapes):
        assert oracle.jpeg_info(c)[:2] == (w, h)
    band, took, _ = _decode(cells, size, impl)
    assert took > 0, f"{name}: the band kernel did not run"
    stream, took2, _ = _decode(cells, size, 2)
    assert took2 == 0
    band, stream = band.numpy(), stream.numpy()
    for k, exp in enumerate(jpeg_expected[name]):
        assert np.array_equal(band[k], exp), f"{name}, image {k}: not the oracle's tensor " \
            f"(max abs {np.abs(band[k] - exp).max()}, {np.count_nonzero(band[k] != exp)} differ)"
        assert np.array_equal(band[k], stream[k]), f"{name}, image {k}: band and streaming kernels differ"


def test_the_cases_reach_the_skipped_rows(jpeg_cells):
    """The first case's bands, as the launch cut them: some start on an odd
    source row (the even row below is skipped), some on an even one, some span
    an odd number of rows from the even row below (the last pair's second row
    is skipped), and the odd height's last band ends at the image's last row."""
    name, shapes, size, _ = JPEG_CASES[0]
    _, took, bands = _decode(jpeg_cells[name], size, 0)
    assert took > 0 and bands >= 2
    odd = even = odd_span = 0
    for _, h, _ in shapes:
        for ya, yb in _band_rows(h, size[0], bands):
            odd += ya & 1
            even += 1 - (ya & 1)
            odd_span += (yb - (ya & ~1)) & 1
    assert odd and even and odd_span, (odd, even, odd_span, bands)
    assert _band_rows(511, size[0], bands)[-1][1] == 511


def test_formatted_output_uint8_nhwc(jpeg_cells):
    """One FMT case: uint8 channels_last, the resized bytes themselves."""
    import torch

    name = "down-5-6-taps"
    cells = jpeg_cells[name]
    kw = dict(dtype="uint8", memory_format="channels_last")
    band, took, _ = _decode(cells, (224, 224), 0, **kw)
    assert took > 0
    stream, took2, _ = _decode(cells, (224, 224), 2, **kw)
    assert took2 == 0
    assert band.dtype == torch.uint8 and band.stride() == (3 * 224 * 224, 1, 3 * 224, 3)
    for k, c in enumerate(cells):
        want = torch.from_numpy(np.rint(oracle.jpeg_to_tensor(c).astype(np.float64) * 255.0).astype(np.uint8))
        assert torch.equal(band[k].contiguous(), want), f"image {k}: not the resized bytes"
    assert torch.equal(band.contiguous(), stream.contiguous())


def _raw_both(raw, off):
    """resize_raw of uint8 [N, H, W, 3] placed `off` bytes past an aligned
    address: (band kernel's tensors, streaming kernel's), on the CPU."""
    import torch

    import ldt_amd

    ctx, _lib = _ctx()
    n, h, w, _ = raw.shape
    flat = torch.zeros(raw.size + 16, dtype=torch.uint8, device="cuda")
    dev = flat[off:off + raw.size].view(n, h, w, 3)
    dev.copy_(torch.from_numpy(raw))
    band = ldt_amd.resize_raw(dev, h, w, normalize=False).cpu().numpy()
    assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 2, "the band kernel did not run"
    ctx.set_option(_lib.OPT_RESIZE_IMPL, 2)
    try:
        stream = ldt_amd.resize_raw(dev, h, w, normalize=False).cpu().numpy()
        assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 0
    finally:
        ctx.set_option(_lib.OPT_RESIZE_IMPL, 0)
    return band, stream


@pytest.mark.parametrize("w,h,off", [(512, 511, 0), (640, 100, 0), (500, 37, 1), (333, 513, 3)],
                         ids=["512x511-aligned", "640x100-aligned", "500x37-unaligned", "333x513-unaligned"])
def test_raw_sources(w, h, off):
    """16-byte aligned rows (k_resize4<1>) and rows from an odd address
    (k_resize4<3>): a band's last pair without its second row, an odd height."""
    from ldt_amd import synth

    raw = synth.raw_hwc(4, h, w, seed=w + h)
    band, stream = _raw_both(raw, off)
    for k in range(raw.shape[0]):
        assert np.array_equal(band[k], oracle.raw_to_tensor(raw[k])), f"image {k}: not the oracle's tensor"
    assert np.array_equal(band, stream)


def test_saturated_raw_images():
    """All-255, all-0 and 0/255 checkerboards (1-pixel and 3-pixel squares):
    the tap sums at their largest and smallest. Where the oracle's output is
    the LUT's end value (1.0, 0.0), so is the kernel's."""
    h, w = 515, 512
    yy, xx = np.mgrid[0:h, 0:w]
    raw = np.empty((4, h, w, 3), np.uint8)
    raw[0] = 255
    raw[1] = 0
    raw[2] = (((yy + xx) & 1) * 255)[..., None]
    raw[3] = ((((yy // 3) + (xx // 3)) & 1) * 255)[..., None]
    band, stream = _raw_both(raw, 0)
    exp = np.stack([oracle.raw_to_tensor(raw[k]) for k in range(4)])
    assert np.all(exp[0] == 1.0) and np.all(exp[1] == 0.0)
    assert np.array_equal(band, exp)
    assert np.array_equal(band, stream)
    assert band.max() == 1.0 and band.min() == 0.0


def test_saturated_jpegs():
    """A white, a black, a 0/255 block-checkerboard and a pure red JPEG through the packed
    and the 32-bit staging: colour conversion and both tap passes at the ends
    of their ranges."""
    from ldt_amd import synth

    h, w = 511, 512
    yy, xx = np.mgrid[0:h, 0:w]
    red = np.zeros((h, w, 3), np.uint8)
    red[..., 0] = 255
    imgs = [np.full((h, w, 3), 255, np.uint8), np.zeros((h, w, 3), np.uint8),
            np.repeat(((((yy // 8) + (xx // 8)) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2), red]
    cells = [synth.encode(im, quality=90, subsampling="4:2:0") for im in imgs]
    exp = [oracle.jpeg_to_tensor(c) for c in cells]
    assert np.all(exp[0] == 1.0) and np.all(exp[1] == 0.0)
    for impl in (0, 1):
        band, took, _ = _decode(cells, (224, 224), impl)
        assert took > 0
        for k in range(len(cells)):
            assert np.array_equal(band[k].numpy(), exp[k]), f"impl {impl}, image {k}: not the oracle's tensor"
    stream, took2, _ = _decode(cells, (224, 224), 2)
    assert took2 == 0
    assert np.array_equal(band.numpy(), stream.numpy())
