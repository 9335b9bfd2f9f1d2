"""GPU tests of the padded window (``pad=``, ldt_set_pad). Every row against the oracle's resized tensor
``raw_to_tensor(src, res_h, res_w)`` put through ``np.pad`` in the mode, then the window slice and the mirror
(``constant``: the oracle's tensor of a 1 x 1 image of the fill colour; BICUBIC: Pillow's bytes, as
tests/test_gpu_views.py takes them), with tests/test_gpu_window.py's check: max abs <= 2/255, then bit equality.
A source reduced by more than 37 against res fails with status 4; a failed row is zero with label -100."""
import numpy as np
import pyarrow as pa
import pytest
import torch

import jpeg_recode as jr
import ldt_amd
from conftest import read_golden
from ldt_amd import synth
from oracle import oracle
from test_gpu_window import _check

pytestmark = pytest.mark.gpu

MODES = ["constant", "edge", "reflect", "symmetric"]
FILL = (114, 7, 250)


@pytest.fixture(scope="module")
def cells():
    data = [synth.encode(synth.field(48, 64, 201, 6.0)), {c.name: c for c in jr.layout_cells()}["440-17x5"].data,
            read_golden("jpeg/gray_77x91.jpg"), read_golden("jpeg/prog_64x80.jpg"),
            synth.encode(synth.field(8, 8, 205, 6.0), subsampling="4:4:4")]
    return [(d, oracle.decode_rgb(d)) for d in data]


def _reference(src, size, window, flip, pad, normalize=None, interp="bilinear"):
    rh, rw, top, left = (int(v) for v in window)
    (oh, ow), s = size, 1 if interp == "bilinear" else 2
    if -(-s * src.shape[1] // rw) > 37 or -(-s * src.shape[0] // rh) > 37:
        return 4
    if interp == "bicubic":  # Pillow's bytes, then an identity resize: ToTensor
        from PIL import Image

        src = np.asarray(Image.fromarray(np.ascontiguousarray(src)).resize((rw, rh), Image.BICUBIC), dtype=np.uint8)
    R = oracle.raw_to_tensor(src, rh, rw, normalize=normalize)
    fill = oracle.raw_to_tensor(np.array(pad.fill, np.uint8).reshape(1, 1, 3), 1, 1, normalize=normalize)[:, 0, 0]
    pt, pb, pl, pr = max(0, -top), max(0, top + oh - rh), max(0, -left), max(0, left + ow - rw)
    kw = [{"constant_values": fill[c]} if pad.mode == "constant" else {} for c in range(3)]
    P = np.stack([np.pad(R[c], ((pt, pb), (pl, pr)), mode=pad.mode, **kw[c]) for c in range(3)])
    t = P[:, top + pt:top + pt + oh, left + pl:left + pl + ow]
    return np.ascontiguousarray(t[:, :, ::-1] if flip else t)


def _rows(cells, size, windows, pad, what, out=None, lbl=None, crops=None, normalize=None, interpolation=None, **fmt):
    """Every row of ``out`` / ``lbl`` (else: of a decode_arrow call in ``fmt``) against `_reference`; {row: status}."""
    n, got, want = len(cells), {}, {}
    if out is None:
        out = torch.full((n, 3) + tuple(size), 77, dtype=fmt.get("dtype") or torch.float32, device="cuda")
        if "memory_format" in fmt:
            out = out.contiguous(memory_format=torch.channels_last)
        lbl = torch.full((n,), -777, dtype=torch.int64, device="cuda")
        try:
            ldt_amd.decode_arrow(pa.array([c[0] for c in cells], pa.binary()), np.arange(100, 100 + n), out=out, out_lbl=lbl,
                           size=size, windows=windows, pad=pad, crops=crops, normalize=normalize,
                           interpolation=interpolation, **fmt)
        except ldt_amd.ImageDecodeError as e:
            got = dict(e.rows)
    img, lbl, scale = out.float().cpu().numpy(), lbl.cpu().numpy(), 255.0 if out.dtype == torch.uint8 else 1.0
    for k, (_, rgb) in enumerate(cells):
        exp = 1  # a cell without pixels: the golden not-a-JPEG one (LDT_IMG_NOT_JPEG)
        if rgb is not None:
            t, l, bh, bw, f = (int(v) for v in crops[k]) if crops is not None else (0, 0) + rgb.shape[:2] + (0,)
            exp = _reference(rgb[t:t + bh, l:l + bw], size, windows[k], f, pad, normalize, interpolation or "bilinear")
        if isinstance(exp, int):
            want[k] = exp
            assert not img[k].any() and lbl[k] == -100, f"{what}: failed row {k} is not zero with label -100"
            continue
        exp = torch.from_numpy(exp * scale).round().to(out.dtype) if scale > 1 else torch.from_numpy(exp).to(out.dtype)
        _check(img[k] / scale, exp.float().numpy() / scale, f"{what}: row {k} window {list(windows[k])} -> {size}")
        assert lbl[k] == 100 + k
    assert got == want, f"{what}: failed rows {got}, expected {want}"
    return want


def _overhangs(size, mode):
    """(res_h, res_w, top, left) of every case, the same for every cell."""
    oh, ow = size
    big = (oh + 5, ow + 5)
    return [big + (2, -3), big + (2, 9), big + (-3, 1),  # left; right; band 0 holds 3 pad rows and 5 image rows
            big + (9, 1), (max(1, oh - 5), max(1, ow - 7), -2, -3),  # bottom from mid-band; all four sides
            big + (-8, 0), big + (-11, 0),  # a whole band of pad, then a straddling one
            # (299, 299): tile 1 is partly fill at res_w 280 and, in constant mode, wholly fill at 200
            (oh + 5, ow - 19 if ow > 256 else ow + 1, 1, 0), (oh + 5, 200 if ow > 256 else max(1, ow - 2), 1, 0),
            (1, 1, -3, -2), (2, 3, -9, -11), (5, 5, -17, -13)  # several folds, every resized row more than once
            ] + ([(5, 5, -400, 700)] if mode == "constant" else [])  # wholly outside: all fill


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", [(7, 5), (30, 33), (299, 299)], ids=str)  # < a band; short last band; two tiles
def test_overhangs_on_every_cell(cells, size, mode):
    for w in _overhangs(size, mode):  # (the cells above 37 pixels per resized pixel fail alone, with status 4)
        _rows(cells, size, np.array([w] * len(cells), np.int32), ldt_amd.Pad(FILL, mode), f"{mode} {w}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt", ["f32", "bf16-cl", "u8"])
@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
def test_fill_flip_filter_format_and_box(cells, interp, fmt, mode):
    kw = {"f32": {}, "u8": {"dtype": torch.uint8},
          "bf16-cl": {"dtype": torch.bfloat16, "memory_format": torch.channels_last}}[fmt]
    # a box of every cell (odd origin where it fits), every other row flipped
    crops = np.array([[h > 8, w > 8, h - (h > 8), w - 2 * (w > 8), k & 1]
                      for k, (h, w) in enumerate(c[1].shape[:2] for c in cells)], np.int32)
    windows = np.array([[25, 28, -2, -3], [35, 38, -3, 1], [35, 38, 9, 9], [25, 40, -8, -1], [5, 5, -17, -13]], np.int32)
    for normalize in ((None,) if fmt == "u8" else (None, True)):
        assert _rows(cells, (30, 33), windows, ldt_amd.Pad(FILL, mode), f"{mode} {interp} {fmt} {normalize}", crops=crops,
                     normalize=normalize, interpolation=interp, **kw) == {}


@pytest.mark.parametrize("mode", MODES)
def test_views_size_list_raw_and_a_failed_row(cells, mode):
    pad, n = ldt_amd.Pad(FILL, mode), len(cells)
    arr, labels = pa.array([c[0] for c in cells], pa.binary()), np.arange(100, 100 + n)
    per_view = [np.array([[25, 28, -2, -3]] * n, np.int32), np.array([[35, 38, 9, -11]] * n, np.int32)]
    windows, sizes = np.stack(per_view, axis=1), [(30, 33), (7, 5)]  # [n, 2, 4]: a different window per view
    out, lbl = ldt_amd.decode_arrow(arr, labels, size=(30, 33), views=2, windows=windows, pad=pad)
    outs, lbl2 = ldt_amd.decode_arrow(arr, labels, size=sizes, windows=windows, pad=pad)  # one run per size: [1, n, 3, h, w]
    for v in range(2):
        assert _rows(cells, (30, 33), per_view[v], pad, f"{mode} view {v}", out[v], lbl) == {}
        assert _rows(cells, sizes[v], per_view[v], pad, f"{mode} size list {v}", outs[v][0], lbl2) == {}
    raw = np.stack([synth.raw_hwc_one(61, 83, 71 + k) for k in range(3)])
    wins = np.array([[25, 28, -2, -3], [35, 38, 9, 9], [5, 5, -17, -13]], np.int32)
    crops = np.array([[1, 3, 50, 70, 0], [0, 1, 61, 82, 1], [10, 20, 20, 30, 1]], np.int32)
    got = ldt_amd.resize_raw(torch.from_numpy(raw).cuda(), 61, 83, normalize=True, size=(30, 33), windows=wins,
                             crops=crops, pad=pad).cpu().numpy()
    for k, (t, l, bh, bw, f) in enumerate(crops.tolist()):
        _check(got[k], _reference(raw[k, t:t + bh, l:l + bw], (30, 33), wins[k], f, pad, True), f"raw {mode} {k}")
    # the golden not-a-JPEG cell (status 1) between good ones stays zero, its neighbours are exact
    batch = cells[:2] + [(read_golden("jpeg/bad_not_jpeg.bin"), None)] + cells[2:]
    assert _rows(batch, (30, 33), np.array([[25, 28, -2, -3]] * len(batch), np.int32), pad, "failed row") == {2: 1}


def test_recipes_later_stages_and_guards(cells):
    arr, n = pa.array([c[0] for c in cells], pa.binary()), len(cells)
    rb = pa.RecordBatch.from_arrays([arr, pa.array(np.arange(100, 100 + n), pa.int64())], names=["image", "label"])
    wh = np.array([c[1].shape[1::-1] for c in cells], np.int32)
    crop = lambda: ldt_amd.PadRandomCrop(4, True, torch.Generator().manual_seed(5))  # noqa: E731
    for make, size, pad in ((ldt_amd.Letterbox, (48, 48), ldt_amd.Pad(FILL)), (crop, (32, 32), ldt_amd.Pad(0, "reflect")),
                            (lambda: ldt_amd.ResizeCenterCrop(40, pad=True), (48, 48), ldt_amd.Pad(0))):
        windows = make().sample(wh, None, size)
        assert (windows[:, 2:] < 0).any()
        got = ldt_amd.decode_tensor_image(rb, size=size, window=make(), pad=pad)
        assert _rows(cells, size, windows, pad, repr(make()), got["image"], got["label"]) == {}
    # solarize alone: the colour stage sees the padded bytes, fill (114, 7, 250) -> (114, 7, 5)
    size, pad, windows = (30, 33), ldt_amd.Pad(FILL), np.array([[25, 28, -2, -3]] * n, np.int32)
    color = ldt_amd.ColorJitterParams(None, None, None, None, p=None, gray_p=None, solarize_p=1.0, solarize_threshold=128)
    out, _ = ldt_amd.decode_arrow(arr, size=size, windows=windows, pad=pad, colors=color)
    for k, (_, rgb) in enumerate(cells):
        u8 = np.rint(_reference(rgb, size, windows[k], 0, pad) * 255.0).astype(np.uint8)
        sol = np.where(u8 >= 128, 255 - u8, u8).transpose(1, 2, 0)
        _check(out[k].cpu().numpy(), oracle.raw_to_tensor(sol, *size), f"solarize row {k}")
    # pad=None: the overhang still fails every row with status 7, also right after a padded call
    with pytest.raises(ldt_amd.ImageDecodeError) as e:
        ldt_amd.decode_arrow(arr, size=size, windows=windows)
    assert e.value.rows == {k: 7 for k in range(n)}
    for call in (lambda: ldt_amd.decode_arrow(arr, size=size, pad=pad), lambda: ldt_amd.decode_native(arr, pad=pad)):
        with pytest.raises(ValueError):  # a pad without a window; a pad on a native call
            call()
