"""GPU tests of the band kernel (k_resize4) sized by the real tap counts: its
KS, ring and staging rows follow the most taps any window of the batch's
widths and heights has (resample_taps_host), not Pillow's buffer length. Every
dropped product has a zero weight, so every case is bit for bit the Pillow
oracle's tensor and the streaming kernel's (LDT_OPT_RESIZE_IMPL 2) for the same
batch, and every case asserts that the band kernel ran. The shapes are those
where the sizing can go wrong: a last window ending at the row's last dword,
row ends off a 16-pixel boundary, different counts on the two axes, leading
zero weights (480), counts of 2 (identity, upscale), a mixed batch whose taps
come from different images per axis, a height past the table (computed
vertical coefficients), 10 of 11 taps, generic staging, raw sources, other
output sizes and a formatted output. tools/checks/taps_check.cpp is the CPU
side (tests/test_resize4_taps.py).
"""
import numpy as np
import pyarrow as pa
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

# (id, [(W, H, subsampling)], (out_h, out_w))
JPEG_CASES = [
    ("512x512", [(512, 512, "4:2:0")], (224, 224)),             # 5 of 7 taps, the last window ends the row
    ("496x512", [(496, 512, "4:2:0")], (224, 224)),             # row end off a 16-pixel boundary
    ("510x512", [(510, 512, "4:2:0")], (224, 224)),
    ("640x480", [(640, 480, "4:2:0")], (224, 224)),             # 6 / 5 taps, 480's leading zero weights
    ("480x640", [(480, 640, "4:2:0")], (224, 224)),
    ("384x512", [(384, 512, "4:2:0")], (224, 224)),
    ("333x500", [(333, 500, "4:2:0")], (224, 224)),
    ("224x224", [(224, 224, "4:2:0")], (224, 224)),             # identity: counts of 2
    ("100x60", [(100, 60, "4:2:0")], (224, 224)),               # upscale
    ("16x16", [(16, 16, "4:2:0")], (224, 224)),
    ("mixed", [(512, 100, "4:2:0"), (448, 448, "4:2:0"), (333, 640, "4:2:0")], (224, 224)),
    ("300x1200", [(300, 1200, "4:2:0")], (224, 224)),           # vertical coefficients computed in the kernel
    ("1120x64", [(1120, 64, "4:2:0")], (224, 224)),             # 10 of 11 taps
    ("444+grey", [(500, 375, "4:4:4"), (320, 200, "grey")], (224, 224)),  # the generic staging
    ("to-96x160", [(512, 512, "4:2:0"), (333, 500, "4:4:4")], (96, 160)),    # GEN, float4 stores
    ("to-250x255", [(512, 512, "4:2:0"), (333, 500, "4:4:4")], (250, 255)),  # GEN, single stores
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
    """(images on the CPU, the waves per workgroup of the band kernel or 0)."""
    import torch

    from ldt_amd import transforms as T

    ctx, _lib = _ctx()
    ctx.set_option(_lib.OPT_RESIZE_IMPL, impl)
    try:
        out = T.decode_arrow(pa.array(cells, pa.binary()), size=size, **kw)[0]
        torch.cuda.synchronize()
        took = ctx.lib.ldt_debug_last_resize(ctx.handle)
    finally:
        ctx.set_option(_lib.OPT_RESIZE_IMPL, 0)
    return out.cpu(), took


@pytest.mark.parametrize("name,shapes,size", JPEG_CASES, ids=[c[0] for c in JPEG_CASES])
def test_band_kernel_equals_oracle_and_streaming(name, shapes, size):
    assert len(shapes) <= 8
    cells = [_cell(w, h, sub, 900 + 7 * k + w) for k, (w, h, sub) in enumerate(shapes)]
    for c, (w, h, _) in zip(cells, shapes):
        assert oracle.jpeg_info(c)[:2] == (w, h)
    band, took = _decode(cells, size, 0)
    assert took > 0, f"{name}: the band kernel did not run"
    stream, took2 = _decode(cells, size, 2)
    assert took2 == 0
    band, stream = band.numpy(), stream.numpy()
    for k, c in enumerate(cells):
        exp = oracle.jpeg_to_tensor(c, size[0], size[1])
        assert np.array_equal(band[k], exp), f"{name}, image {k}: not the oracle's tensor " \
            f"(max abs {np.abs(band[k] - exp).max()}, {np.count_nonzero(band[k] != exp)} differ)"
        assert np.array_equal(band[k], stream[k]), f"{name}, image {k}: band and streaming kernels differ"


def test_formatted_output_fp16_nhwc():
    """One FMT case: float16 channels_last of a 512 x 512 and a 640 x 480 source."""
    import torch

    cells = [_cell(512, 512, "4:2:0", 31), _cell(640, 480, "4:2:0", 32)]
    kw = dict(dtype="float16", memory_format="channels_last")
    band, took = _decode(cells, (224, 224), 0, **kw)
    assert took > 0
    stream, took2 = _decode(cells, (224, 224), 2, **kw)
    assert took2 == 0
    assert band.dtype == torch.float16 and band.stride() == (3 * 224 * 224, 1, 3 * 224, 3)
    for k, c in enumerate(cells):
        want = torch.from_numpy(oracle.jpeg_to_tensor(c)).to(torch.float16)
        assert torch.equal(band[k].contiguous().view(torch.int16), want.view(torch.int16)), f"image {k}: not ref32.to(fp16)"
    assert torch.equal(band.contiguous().view(torch.int16), stream.contiguous().view(torch.int16))


@pytest.mark.parametrize("w,h", [(1024, 1024), (1000, 37)], ids=["1024x1024-aligned", "1000x37-unaligned"])
def test_raw_sources(w, h):
    """resize_raw: 16-byte aligned rows (k_resize4<1>) and 1000-pixel rows from
    an odd address (k_resize4<3>); 10 of 11 horizontal taps, skewed staging."""
    import torch

    import ldt_amd
    from ldt_amd import synth

    ctx, _lib = _ctx()
    raw = synth.raw_hwc(2, h, w, seed=w + h)
    off = 0 if w == 1024 else 1
    flat = torch.zeros(raw.size + 1, dtype=torch.uint8, device="cuda")
    dev = flat[off:off + raw.size].view(2, h, w, 3)
    dev.copy_(torch.from_numpy(raw))
    band = ldt_amd.resize_raw(dev, h, w, normalize=False).cpu().numpy()
    assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 2, "the band kernel did not run"
    ctx.set_option(_lib.OPT_RESIZE_IMPL, 2)
    try:
        stream = ldt_amd.resize_raw(dev, h, w, normalize=False).cpu().numpy()
        assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 0
    finally:
        ctx.set_option(_lib.OPT_RESIZE_IMPL, 0)
    for k in range(2):
        assert np.array_equal(band[k], oracle.raw_to_tensor(raw[k])), f"image {k}: not the oracle's tensor"
    assert np.array_equal(band, stream)
