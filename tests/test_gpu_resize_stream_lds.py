"""GPU tests of the streaming resize's launches with more than 64 KB of dynamic
LDS: every instantiation of k_resize (source x box x filter x format, 24) and
of k_resize_views (filter x sized x format, 8) launched once with a need
between 65 537 and 163 840 bytes, which takes the raised
``hipFuncAttributeMaxDynamicSharedMemorySize`` of that very instantiation: one
left out of the launcher's table makes its launch return an error.

A wide, flat source gets there at the smallest size: 8000 x 16 to 224 x 224 is
ceil(8000 / 224) = 36, 73 horizontal taps; BICUBIC (support 2) takes 4000 wide
for the same 73. Every case asserts its own need with the launcher's formula
(`_lds_bytes`: stream_lds_bytes in ldt_resize_stream.hip), so a later change of
constants cannot quietly turn it into a small-LDS test.

Expected values are the oracle composition of the neighbouring files,

    raw_to_tensor(src[box], res_h, res_w)[:, top:top+oh, left:left+ow], mirrored when flip,

``src`` being ``oracle.decode_rgb(cell)`` or the raw cell, and Pillow itself
for BICUBIC (`_pil_window` of tests/test_gpu_interpolation.py). Max abs <=
2/255 is asserted first, then bit equality (`_check_image` of
tests/test_gpu_views.py, which converts the float32 reference for the
formatted case). No row may fail; every row of every case has an expected
value: nothing is skipped or filtered.
"""
import numpy as np
import pyarrow as pa
import pytest

from oracle import oracle
from test_gpu_interpolation import _pil_window
from test_gpu_views import _check_image, _td
from test_interpolation import checkerboard

pytestmark = pytest.mark.gpu

SIZE = (224, 224)
WIDE = {"bilinear": 8000, "bicubic": 4000}  # ceil(support * width / 224) = 36 under either filter
FLAT = 16
BAND_ROWS, TILE_COLS = 8, 256  # kBandRows, kTileCols
FORMATS = [("float32", "contiguous"), ("float16", "channels_last")]
_FMT_ID = lambda f: "f32chw" if f[0] == "float32" else "f16nhwc"  # noqa: E731

_cells, _raw, _rgb, _exp = {}, {}, {}, {}


def _ksize(src, res, interp):
    """resample_ksize_host: Pillow's tap capacity of (src -> res)."""
    s = 2 if interp == "bicubic" else 1
    return 2 * max(-(-s * src // res), s) + 1


def _lds_bytes(sources, max_ow, interp):
    """stream_lds_bytes of a launch. sources: (width, height, res_w, res_h) of
    every source the launch resizes (each row's, each view's)."""
    ks_h = max(_ksize(w, rw, interp) for w, _, rw, _ in sources)
    ks_v = max(_ksize(h, rh, interp) for _, h, _, rh in sources)
    row_bytes = (max(w for w, _, _, _ in sources) * 3 + 15) // 16 * 16
    tcols = min(max_ow, TILE_COLS)
    return 3072 + 4 * (tcols * ks_h + BAND_ROWS * ks_v + 2 * tcols + 2 * BAND_ROWS) + 2 * row_bytes


def _assert_large_lds(sources, max_ow, interp):
    need = _lds_bytes(sources, max_ow, interp)
    assert 65536 < need <= 163840, f"the launch needs {need} bytes of LDS: not a large-LDS case"


def _jpeg_cells(interp):
    """The wide cell and one ordinary batch-mate: (name, data, (h, w))."""
    from ldt_amd import synth

    w = WIDE[interp]
    if w not in _cells:
        _cells[w] = [(f"420-{FLAT}x{w}", synth.encode(synth.field(FLAT, w, 211, 6.0)), (FLAT, w)),
                     ("420-48x64", synth.encode(synth.field(48, 64, 201, 6.0)), (48, 64))]
        for name, data, _ in _cells[w]:
            _rgb[name] = oracle.decode_rgb(data)
    return _cells[w]


def _raw_cells(interp):
    """Two raw HWC cells of the wide shape: (name, (h, w)); the pixels in `_rgb`."""
    w = WIDE[interp]
    if w not in _raw:
        _raw[w] = [(f"raw{k}-{FLAT}x{w}", (FLAT, w)) for k in range(2)]
        for k, (name, _) in enumerate(_raw[w]):
            _rgb[name] = checkerboard(FLAT, w, 310 + k)
    return _raw[w]


def _expected(name, size, crop, window, interp):
    """The float32 reference of one output image: computed once, never changed."""
    key = (name, size, tuple(int(v) for v in crop), tuple(int(v) for v in window), interp)
    if key not in _exp:
        top, left, bh, bw, flip = key[2]
        src = np.ascontiguousarray(_rgb[name][top:top + bh, left:left + bw])
        _exp[key] = _pil_window(src, size, key[3], flip, None, interp)
        _exp[key].setflags(write=False)
    return _exp[key]


def _geometry(box, shapes, size=SIZE):
    """Per cell the crop and the window of a case, and what the call is given.
    plain: neither; crops: the whole image, flipped; windows: res a little above
    the output and the window inside it."""
    crops = np.array([[0, 0, h, w, 1 if box == "crops" else 0] for h, w in shapes], np.int32)
    if box == "windows":
        windows = np.array([[size[0] + 6, size[1] + 6, 3 + k, 5 - k] for k in range(len(shapes))], np.int32)
    else:
        windows = np.array([[size[0], size[1], 0, 0]] * len(shapes), np.int32)
    return crops, windows, (crops if box == "crops" else None), (windows if box == "windows" else None)


def _torch_format(fmt):
    import torch

    return _td(fmt[0]), (torch.channels_last if fmt[1] == "channels_last" else None)


def _streamed():
    import torch

    from ldt_amd import _lib

    ctx = _lib.get_context(torch.cuda.current_device())
    return ctx.lib.ldt_debug_last_resize(ctx.handle) == 0


@pytest.mark.parametrize("fmt", FORMATS, ids=_FMT_ID)
@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
@pytest.mark.parametrize("box", ["plain", "crops", "windows"])
def test_k_resize_jpeg(box, interp, fmt):
    import torch

    from ldt_amd import transforms as T

    cells = _jpeg_cells(interp)
    crops, windows, arg_crops, arg_windows = _geometry(box, [hw for _, _, hw in cells])
    _assert_large_lds([(c[3], c[2], w[1], w[0]) for c, w in zip(crops, windows)], SIZE[1], interp)
    dtype, mf = _torch_format(fmt)
    labels = np.arange(100, 100 + len(cells), dtype=np.int64)
    img, lbl = T.decode_arrow(pa.array([d for _, d, _ in cells], pa.binary()), labels, size=SIZE, crops=arg_crops,
                              windows=arg_windows, interpolation=interp, dtype=dtype, memory_format=mf)
    torch.cuda.synchronize()  # a failed row would have raised ImageDecodeError
    assert _streamed() and tuple(img.shape) == (len(cells), 3) + SIZE
    assert lbl.cpu().tolist() == labels.tolist()
    img = img.cpu()
    for k, (name, _, _) in enumerate(cells):
        _check_image(img[k], _expected(name, SIZE, crops[k], windows[k], interp), fmt[0],
                     f"k_resize<0, {box}, {interp}, {_FMT_ID(fmt)}>: {name}")


@pytest.mark.parametrize("fmt", FORMATS, ids=_FMT_ID)
@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
@pytest.mark.parametrize("box", ["plain", "crops", "windows"])
def test_k_resize_raw(box, interp, fmt):
    import torch

    import ldt_amd

    cells = _raw_cells(interp)
    h, w = cells[0][1]
    crops, windows, arg_crops, arg_windows = _geometry(box, [hw for _, hw in cells])
    _assert_large_lds([(c[3], c[2], v[1], v[0]) for c, v in zip(crops, windows)], SIZE[1], interp)
    dtype, mf = _torch_format(fmt)
    hwc = torch.from_numpy(np.stack([_rgb[name] for name, _ in cells]))
    out = ldt_amd.resize_raw(hwc, h, w, normalize=False, size=SIZE, crops=arg_crops, windows=arg_windows,
                             interpolation=interp, dtype=dtype, memory_format=mf)
    torch.cuda.synchronize()
    assert _streamed() and tuple(out.shape) == (len(cells), 3) + SIZE
    out = out.cpu()
    for k, (name, _) in enumerate(cells):
        _check_image(out[k], _expected(name, SIZE, crops[k], windows[k], interp), fmt[0],
                     f"k_resize<1, {box}, {interp}, {_FMT_ID(fmt)}>: {name}")


@pytest.mark.parametrize("fmt", FORMATS, ids=_FMT_ID)
@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
@pytest.mark.parametrize("sizes", [None, [(224, 224), (96, 96)]], ids=["views2", "sized"])
def test_k_resize_views(sizes, interp, fmt):
    import torch

    from ldt_amd import transforms as T

    cells = _jpeg_cells(interp)
    view_sizes = sizes or [SIZE, SIZE]
    # view 0: the whole image; view 1: a flipped box at an odd origin, no wider than 37 x its 96 columns
    # over the filter's support (3552 under BILINEAR), so its reduction stays within kMaxReduce
    narrow = 96 * 37 // (2 if interp == "bicubic" else 1)
    crops = np.array([[[0, 0, h, w, 0], [1, 3, h - 2, min(w - 4, narrow), 1]] for _, _, (h, w) in cells], np.int32)
    windows = np.array([[[vh, vw, 0, 0] for vh, vw in view_sizes]] * len(cells), np.int32)
    assert crops[0, 1, 3] == narrow
    _assert_large_lds([(c[3], c[2], v[1], v[0]) for row, wrow in zip(crops, windows) for c, v in zip(row, wrow)],
                      max(vw for _, vw in view_sizes), interp)
    dtype, mf = _torch_format(fmt)
    labels = np.arange(100, 100 + len(cells), dtype=np.int64)
    arr = pa.array([d for _, d, _ in cells], pa.binary())
    if sizes is None:
        img, lbl = T.decode_arrow(arr, labels, size=SIZE, crops=crops, views=2, interpolation=interp, dtype=dtype,
                                  memory_format=mf)
        views = [img[0], img[1]]
    else:
        runs, lbl = T.decode_arrow(arr, labels, size=sizes, crops=crops, interpolation=interp, dtype=dtype,
                                   memory_format=mf)
        assert [tuple(r.shape) for r in runs] == [(1, len(cells), 3) + s for s in sizes]
        views = [r[0] for r in runs]
    torch.cuda.synchronize()
    assert _streamed() and lbl.cpu().tolist() == labels.tolist()
    for v, size in enumerate(view_sizes):
        got = views[v].cpu()
        assert tuple(got.shape) == (len(cells), 3) + size
        for k, (name, _, _) in enumerate(cells):
            _check_image(got[k], _expected(name, size, crops[k, v], windows[k, v], interp), fmt[0],
                         f"k_resize_views<{interp}, {'sized' if sizes else 'uniform'}, {_FMT_ID(fmt)}>: {name} view {v}")
