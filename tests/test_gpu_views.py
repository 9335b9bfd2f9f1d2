"""GPU tests of ``views=`` (ldt_set_views): several crops or windows of every
image from a single decode, through every decode entry point, against the
oracle composition

    raw_to_tensor(decode_rgb(cell)[box], res_h, res_w)[:, top:top+oh, left:left+ow], mirrored when flip,

per output image (v, i), which tests/test_views.py, tests/test_crop.py and
tests/test_window.py pin to Pillow's ``crop().resize().crop()`` on the CPU. Max
abs <= 2/255 is asserted first, then bit equality. The same views through V
single-view calls are a second cross-check only.

One rule (`_expected_row`) says what every row must be. Its views are taken in
order v = 0..V-1, each as a single-view call takes it: status 7 for a window
whose res is outside 1..65535, whose origin is negative or which is not inside
res; else status 6 for a bad box; else status 4 for a source reduced by more
than 37 against res on an axis (BICUBIC: twice the source). The first view that
fails gives the row its status; a failed row is all-zero bytes in all V outputs
with label -100; every other row is exact in every view. Every row of every
case has an expected value: nothing is skipped or filtered.
"""
import numpy as np
import pyarrow as pa
import pytest

import jpeg_recode as jr
from conftest import read_golden
from oracle import oracle

pytestmark = pytest.mark.gpu

TOL = 2.0 / 255.0
SENTINEL = 0xA5  # every byte of the guarded buffers
ES = {"float32": 4, "float16": 2, "bfloat16": 2, "uint8": 1}
_ID = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


def _td(dtype):
    import torch

    return {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16, "uint8": torch.uint8}[dtype]


@pytest.fixture(scope="module")
def mixed():
    """The eight-cell mixed batch of tests/test_gpu_crop.py and a ninth cell,
    so that the images cross the group of 8 of the resize's grid order:
    (name, data) in a fixed order; the names give height x width."""
    from ldt_amd import synth

    layout = {c.name: c for c in jr.layout_cells()}
    return [
        ("420-48x64", synth.encode(synth.field(48, 64, 201, 6.0))),
        ("420-375x500", synth.encode(synth.field(375, 500, 202, 6.0), quality=90, restart_marker_rows=1)),
        ("444-100x150", synth.encode(synth.field(100, 150, 204, 6.0), subsampling="4:4:4")),
        ("gray-77x91", read_golden("jpeg/gray_77x91.jpg")),
        ("prog-64x80", read_golden("jpeg/prog_64x80.jpg")),
        ("440-17x5", layout["440-17x5"].data),
        ("411-33x40", layout["411-33x40"].data),
        ("up-8x8", synth.encode(synth.field(8, 8, 205, 6.0), subsampling="4:4:4")),
        ("420-40x56", synth.encode(synth.field(40, 56, 207, 6.0))),
    ]


_rgb_cache, _exp_cache, _hw_cache = {}, {}, {}


def _hw(name, data):
    if name not in _hw_cache:
        w, h, _ = oracle.jpeg_info(data)
        _hw_cache[name] = (h, w)
    return _hw_cache[name]


def _expected_view(name, data, size, crop, window, normalize=None, interp="bilinear"):
    """The oracle's float32 tensor for one view of the row, or the status the
    view fails with. Computed once per distinct view and never changed."""
    h, w = _hw(name, data)
    btop, bleft, bh, bw, flip = (int(v) for v in crop) if crop is not None else (0, 0, h, w, 0)
    rh, rw, top, left = (int(v) for v in window) if window is not None else (size[0], size[1], 0, 0)
    key = (name, size, (btop, bleft, bh, bw, flip), (rh, rw, top, left), repr(normalize or None), interp)
    if key in _exp_cache:
        return _exp_cache[key]
    s = 2 if interp == "bicubic" else 1
    if not (1 <= rh <= 65535 and 1 <= rw <= 65535) or top < 0 or left < 0 or size[0] > rh - top or size[1] > rw - left:
        exp = 7
    elif btop < 0 or bleft < 0 or bh < 1 or bw < 1 or btop + bh > h or bleft + bw > w or flip not in (0, 1):
        exp = 6
    elif -(-s * bw // rw) > 37 or -(-s * bh // rh) > 37:
        exp = 4
    else:
        if name not in _rgb_cache:
            _rgb_cache[name] = oracle.decode_rgb(data)
        src = np.ascontiguousarray(_rgb_cache[name][btop:btop + bh, bleft:bleft + bw])
        if interp == "bilinear":
            t = oracle.raw_to_tensor(src, rh, rw, normalize=normalize)[:, top:top + size[0], left:left + size[1]]
            exp = np.ascontiguousarray(t[:, :, ::-1] if flip else t)
        else:  # Pillow itself, as tests/test_gpu_interpolation.py takes it
            from PIL import Image

            im = Image.fromarray(src).resize((rw, rh), Image.BICUBIC)
            u8 = np.asarray(im.crop((left, top, left + size[1], top + size[0])), dtype=np.uint8)
            u8 = np.ascontiguousarray(u8[:, ::-1] if flip else u8)
            exp = oracle.raw_to_tensor(u8, size[0], size[1], normalize=normalize)  # an identity resize: ToTensor
        exp.setflags(write=False)
    _exp_cache[key] = exp
    return exp


def _expected_row(name, data, size, V, crops, windows, normalize=None, interp="bilinear"):
    """A list of V tensors, or the status of the first view that fails."""
    views = [_expected_view(name, data, size, None if crops is None else crops[v],
                            None if windows is None else windows[v], normalize, interp) for v in range(V)]
    for e in views:
        if isinstance(e, int):
            return e
    return views


def _convert(exp32, dtype):
    import torch

    if dtype == "uint8":
        return torch.from_numpy(np.rint(exp32.astype(np.float64) * 255.0).astype(np.uint8))
    return torch.from_numpy(np.array(exp32)).to(_td(dtype))  # a writable copy


def _check_image(got, exp32, dtype, what):
    """got: a CPU tensor [3, h, w] of the dtype (any strides)."""
    import torch

    assert got.dtype == _td(dtype) and tuple(got.shape) == exp32.shape, (what, got.dtype, tuple(got.shape))
    got = got.contiguous()
    want = _convert(exp32, dtype)
    if dtype == "uint8":
        d = np.abs(got.numpy().astype(np.int32) - want.numpy().astype(np.int32))
        assert d.max() <= 2, f"{what}: {d.max()} levels off"
        assert torch.equal(got, want), f"{what}: not the resized byte ({np.count_nonzero(d)} differ)"
        return
    d = np.abs(got.to(torch.float64).numpy() - exp32.astype(np.float64))
    if dtype == "float32":
        assert d.max() <= TOL, f"{what}: max abs {d.max()} > 2/255 (mean {d.mean()})"
        assert np.array_equal(got.numpy(), exp32), f"{what}: not bit-exact (max abs {d.max()}, {np.count_nonzero(d)} differ)"
    else:
        # half an ulp of the 16-bit type on top of 2/255: 2^-8 relative covers bfloat16 and float16
        assert np.all(d <= TOL + np.abs(exp32.astype(np.float64)) * 2.0 ** -8 + 2.0 ** -24), f"{what}: max abs {d.max()}"
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"{what}: not ref32.to({dtype}) bit for bit"


def _arrow(cells):
    return pa.array([d for _, d in cells], pa.binary())


def _decode_guarded(cells, size, V, crops=None, windows=None, dtype="float32", mf="contiguous", guard=4096,
                    normalize=None, **kw):
    """decode_arrow(views=V) into the middle of a byte buffer full of a
    sentinel. Returns (out [V, n, 3, h, w] on the CPU, labels, {failed row:
    status}); asserts the guards on both sides of the images and of the labels."""
    import torch

    import ldt_amd
    from ldt_amd import transforms as T

    n, (h, w) = len(cells), size
    nbytes = V * n * 3 * h * w * ES[dtype]
    buf = torch.full((guard + nbytes + guard,), SENTINEL, dtype=torch.uint8, device="cuda")
    flat = buf[guard:guard + nbytes].view(_td(dtype))
    out = flat.view(V, n, h, w, 3).permute(0, 1, 4, 2, 3) if mf == "channels_last" else flat.view(V, n, 3, h, w)
    lflat = torch.full((n + 2,), -777, dtype=torch.int64, device="cuda")
    labels = np.arange(100, 100 + n, dtype=np.int64)
    failed = {}
    try:
        got, _ = T.decode_arrow(_arrow(cells), labels, out=out, out_lbl=lflat[1:n + 1], size=size, normalize=normalize,
                                crops=crops, windows=windows, views=V, dtype=_td(dtype),
                                memory_format=torch.channels_last if mf == "channels_last" else None, **kw)
        assert got is out
    except ldt_amd.ImageDecodeError as e:
        failed = dict(e.rows)
    finally:
        torch.cuda.synchronize()
        assert torch.all(buf[:guard] == SENTINEL).item(), f"{size} V={V}: wrote before the output"
        assert torch.all(buf[guard + nbytes:] == SENTINEL).item(), f"{size} V={V}: wrote past the output"
        assert int(lflat[0]) == -777 and int(lflat[n + 1]) == -777
    return out.cpu(), lflat[1:n + 1].cpu().numpy(), failed


def _check_rows(cells, size, V, out, lbl, failed, what, crops=None, windows=None, dtype="float32", normalize=None,
                interp="bilinear", other_failed=None, label0=100):
    """Every output image (v, i) against `_expected_row`; `other_failed`: rows
    that fail for a reason of their own (a corrupt or null cell), with their
    status. Returns the number of exact rows."""
    import torch

    other_failed = other_failed or {}
    n = len(cells)
    assert tuple(out.shape) == (V, n, 3) + tuple(size), (what, tuple(out.shape))
    assert crops is None or np.asarray(crops).shape == (n, V, 5)
    assert windows is None or np.asarray(windows).shape == (n, V, 4)
    want_failed, exact = {}, 0
    for i, (name, data) in enumerate(cells):
        exp = other_failed[i] if i in other_failed else \
            _expected_row(name, data, size, V, None if crops is None else crops[i],
                          None if windows is None else windows[i], normalize, interp)
        if isinstance(exp, int):
            want_failed[i] = exp
            for v in range(V):  # all-zero bytes in every format
                raw = out[v, i].contiguous().view(torch.uint8)
                assert not raw.any().item(), f"{what}: failed row {i} ({name}) view {v} is not all-zero bytes"
            assert lbl is None or lbl[i] == -100, f"{what}: failed row {i} label {lbl[i]}"
        else:
            for v in range(V):
                _check_image(out[v, i], exp[v], dtype, f"{what}: {name} view {v} -> {size}")
            assert lbl is None or lbl[i] == label0 + i
            exact += 1
    assert failed == want_failed, f"{what}: failed rows {failed}, expected {want_failed}"
    return exact


def _box(h, w, top, left, bh, bw, flip):
    """The box clamped into an h x w image (a small cell gets a smaller box, never none)."""
    top, left = min(top, h - 1), min(left, w - 1)
    return [top, left, max(1, min(bh, h - top)), max(1, min(bw, w - left)), flip]


def _view_crops(cells, V):
    """int32 [n, V, 5]: a different box per view, odd origins, boxes to the
    last row and column, a single row, and the whole image; flips alternate."""
    out = []
    for i, (name, data) in enumerate(cells):
        h, w = _hw(name, data)
        row = []
        for v in range(V):
            f = (i + v) & 1
            k = v % 5
            if k == 0:
                row.append(_box(h, w, 3 + v, 5 + 2 * v, h - 6 - v, w - 7 - 2 * v, f))
            elif k == 1:
                row.append(_box(h, w, ((h // 3) | 1) + v // 5, (w // 3) | 1, h, w, f))  # to the last row and column
            elif k == 2:
                row.append(_box(h, w, h // 2 + v // 5, 0, 1 + v // 5, w, f))  # a strip
            elif k == 3:
                row.append(_box(h, w, 0, v // 5, h, w, f))  # the whole image (view 3), or all but its first columns
            else:
                row.append(_box(h, w, (h // 4) + v, (w // 2) | 1, 2 + v, 3 + v, f))  # upscaled
        out.append(row)
    return np.array(out, np.int32)


def _view_windows(cells, V, size):
    """int32 [n, V, 4]: per view a different res and origin, every window inside its res."""
    oh, ow = size
    return np.array([[[oh + 3 * v + (i & 3), ow + 9 + 2 * v, (3 * v + (i & 3)) // (1 + (v & 1)), 9 + 2 * v - (v & 1)]
                      for v in range(V)] for i in range(len(cells))], np.int32)


# ---- crops and flips -----------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(224, 224), (7, 5), (299, 299)], ids=_ID)  # (299, 299): two column tiles
@pytest.mark.parametrize("V", [1, 2, 5, 16])
def test_crops_and_flips_per_view(mixed, V, size):
    import torch

    from ldt_amd import _lib

    crops = _view_crops(mixed, V)
    assert set(np.unique(crops[:, :, 4])) == ({0, 1})
    out, lbl, failed = _decode_guarded(mixed, size, V, crops)
    exact = _check_rows(mixed, size, V, out, lbl, failed, f"crops V={V}", crops=crops)
    ctx = _lib.get_context(torch.cuda.current_device())
    assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 0  # the streaming kernel
    # only the 500 x 375 cell has views over the limit, and only at (7, 5)
    assert set(failed) <= ({1} if size == (7, 5) else set()) and exact == len(mixed) - len(failed)
    # view-major placement: view v of row i is at out[v, i], and no other slot holds it
    if V > 1 and not failed:
        for i in (0, 1, 8):
            for v in range(V):
                for u in range(v + 1, V):
                    assert not torch.equal(out[v, i], out[u, i]), f"row {i}: views {v} and {u} are the same image"
        assert not torch.equal(out[0, 0], out[0, 8])


# ---- windows -----------------------------------------------------------------------------------------

def test_crops_windows_and_flips_together(mixed):
    V, size = 3, (30, 33)
    crops, windows = _view_crops(mixed, V), _view_windows(mixed, V, size)
    out, lbl, failed = _decode_guarded(mixed, size, V, crops, windows)
    assert _check_rows(mixed, size, V, out, lbl, failed, "crops + windows", crops=crops, windows=windows) == len(mixed)
    # windows alone: the whole image in every view
    out, lbl, failed = _decode_guarded(mixed, size, V, None, windows)
    assert _check_rows(mixed, size, V, out, lbl, failed, "windows alone", windows=windows) == len(mixed)
    # neither: all V views are the plain image
    out, lbl, failed = _decode_guarded(mixed, size, V)
    assert _check_rows(mixed, size, V, out, lbl, failed, "neither") == len(mixed)
    assert all(bool((out[v] == out[0]).all()) for v in range(V))


@pytest.mark.parametrize("edge,size,ten", [(64, (48, 48), False), (64, (48, 48), True), (40, (48, 40), True)],
                         ids=["five-64", "ten-64", "ten-40-short"])
def test_resize_five_crop_and_ten_crop(mixed, edge, size, ten):
    import ldt_amd

    fc = ldt_amd.ResizeFiveCrop(edge, ten=ten)
    V = fc.views
    wh = np.array([_hw(n, d)[::-1] for n, d in mixed], np.int32)
    windows = fc.sample(wh, None, size)
    crops = fc.boxes(wh) if ten else None
    out, lbl, failed = _decode_guarded(mixed, size, V, crops, windows)
    exact = _check_rows(mixed, size, V, out, lbl, failed, f"ResizeFiveCrop({edge}, ten={ten})", crops=crops,
                        windows=windows)
    # a cell whose resized size is below the window fails alone with status 7, in all its views
    short = {i: 7 for i, (w, h) in enumerate(wh.tolist())
             if (edge if w <= h else edge * w // h) < size[1] or (edge * h // w if w <= h else edge) < size[0]}
    assert failed == short and exact == len(mixed) - len(short)
    if edge == 40:
        assert 0 < len(short) < len(mixed)
    else:
        assert not short
        # the same through the argument itself: window=ResizeFiveCrop implies views
        items = [{"image": d, "label": 100 + k} for k, (_, d) in enumerate(mixed)]
        got = ldt_amd.collate_fn(items, size=size, window=fc)
        assert tuple(got["image"].shape) == (V, len(mixed), 3) + size
        _check_rows(mixed, size, V, got["image"].cpu(), got["label"].cpu().numpy(), {}, "collate_fn(window=fc)",
                    crops=crops, windows=windows)
        with pytest.raises(ValueError):
            ldt_amd.collate_fn(items, size=size, window=fc, views=3)


# ---- a bad view in the middle ---------------------------------------------------------------------

def test_a_bad_view_fails_its_row_alone(mixed):
    V, size = 3, (7, 2)  # two columns: a reduction above 37 needs a res of 2 on the 80-wide cell
    cells = mixed + [("truncated", read_golden("jpeg/bad_truncated.bin")), ("null", None)]
    n = len(cells)
    th, tw = _hw(*cells[9])
    _hw_cache["null"] = (1, 1)
    crops = np.concatenate([_view_crops(mixed, V),
                            np.array([[[0, 0, min(th, 64), min(tw, 64), v & 1] for v in range(V)]], np.int32),
                            np.array([[[0, 0, 1, 1, 0]] * V], np.int32)])
    windows = np.array([[[12 + v, 16 + v, v, v] for v in range(V)] for _ in range(n)], np.int32)
    h2, w2 = _hw(*cells[2])
    crops[2, 1] = [1, 0, h2, w2, 0]          # row 2, view 1 of 3: top + height == H + 1 -> 6
    crops[4, 2] = [0, 0, 64, 80, 1]
    windows[4, 2] = [12, 2, 3, 0]            # row 4, view 2: 80 -> 2 columns, reduced by 40 -> 4
    crops[6, 0] = [0, 0, 4, 4, 2]            # row 6: a bad crop in view 0 ...
    windows[6, 2] = [6, 16, 0, 0]            # ... and a bad window in view 2: the crop's status
    windows[7, 1] = [12, 16, 6, 0]           # row 7, view 1: 6 + 7 > 12 -> 7
    out, lbl, failed = _decode_guarded(cells, size, V, crops, windows)
    assert failed == {2: 6, 4: 4, 6: 6, 7: 7, 9: 3, 10: 5}
    exact = _check_rows(cells, size, V, out, lbl, failed, "bad views", crops=crops, windows=windows,
                        other_failed={9: 3, 10: 5})
    assert exact == n - 6


# ---- BICUBIC ---------------------------------------------------------------------------------------------

def test_bicubic_with_views(mixed):
    V, size = 2, (30, 33)
    crops, windows = _view_crops(mixed, V), _view_windows(mixed, V, size)
    out, lbl, failed = _decode_guarded(mixed, size, V, crops, windows, interpolation="bicubic")
    exact = _check_rows(mixed, size, V, out, lbl, failed, "bicubic", crops=crops, windows=windows, interp="bicubic")
    assert exact == len(mixed) and not failed
    plain, _, _ = _decode_guarded(mixed, size, V, crops, windows)
    assert not bool((plain == out).all()), "interpolation= was ignored"


# ---- formats -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,mf,normalize", [("bfloat16", "channels_last", None), ("uint8", "contiguous", None),
                                                ("float16", "contiguous", True), ("uint8", "channels_last", None)],
                         ids=["bf16-nhwc", "u8", "f16-normalize", "u8-nhwc"])
def test_formats_with_views(mixed, dtype, mf, normalize):
    V, size = 3, (7, 5)  # odd sizes: no image of a narrow type starts aligned
    crops = _view_crops(mixed, V)
    crops[3, 1] = [0, 0, 78, 91, 0]  # the grey cell's view 1 leaves the image: all-zero bytes in every view
    out, lbl, failed = _decode_guarded(mixed, size, V, crops, dtype=dtype, mf=mf, normalize=normalize)
    h, w = size
    for v in range(V):
        assert out[v].stride() == ((3 * h * w, 1, 3 * w, 3) if mf == "channels_last" else (3 * h * w, h * w, w, 1))
    assert out.stride(0) == len(mixed) * 3 * h * w
    exact = _check_rows(mixed, size, V, out, lbl, failed, f"{dtype} {mf}", crops=crops, dtype=dtype, normalize=normalize)
    assert failed.get(3) == 6 and exact == len(mixed) - len(failed)
    # an out= of the wrong shape, dtype or strides is refused before anything is enqueued
    import torch

    from ldt_amd import transforms as T

    for bad in (torch.empty((len(mixed), 3, h, w), dtype=_td(dtype), device="cuda"),
                torch.empty((V, len(mixed), 3, h, w), dtype=torch.float64, device="cuda"),
                torch.empty((V, len(mixed), 3, w, h), dtype=_td(dtype), device="cuda").transpose(3, 4)):
        with pytest.raises(ValueError):
            T.decode_arrow(_arrow(mixed), out=bad, size=size, views=V, dtype=_td(dtype),
                           memory_format=torch.channels_last if mf == "channels_last" else None)


# ---- entry points ------------------------------------------------------------------------------------------

ENTRY_SIZE = (30, 33)


def _rb(cells):
    return pa.RecordBatch.from_arrays([_arrow(cells), pa.array(np.arange(100, 100 + len(cells)), pa.int64())],
                                      names=["image", "label"])


def test_resident_batch_and_collate_fn(mixed):
    import ldt_amd

    V = 2
    crops, windows = _view_crops(mixed, V), _view_windows(mixed, V, ENTRY_SIZE)
    res = ldt_amd.ResidentBatch([d for _, d in mixed], np.arange(100, 100 + len(mixed)))
    img, lbl = res.decode(size=ENTRY_SIZE, crops=crops, windows=windows, views=V)
    _check_rows(mixed, ENTRY_SIZE, V, img.cpu(), lbl.cpu().numpy(), {}, "ResidentBatch.decode", crops=crops,
                windows=windows)
    img, _ = res.decode(size=ENTRY_SIZE, views=1)  # 1 is a view axis of one
    assert tuple(img.shape) == (1, len(mixed), 3) + ENTRY_SIZE
    _check_rows(mixed, ENTRY_SIZE, 1, img.cpu(), None, {}, "ResidentBatch.decode(views=1)")
    items = [{"image": d, "label": 100 + k} for k, (_, d) in enumerate(mixed)]
    for what, got in (("collate_fn", ldt_amd.collate_fn(items, size=ENTRY_SIZE, crop=crops, views=V)),
                      ("make_collate_fn", ldt_amd.make_collate_fn(size=ENTRY_SIZE, crop=crops, views=V)(items)),
                      ("collate_fn(RecordBatch)", ldt_amd.collate_fn(_rb(mixed), size=ENTRY_SIZE, crop=crops, views=V)),
                      ("decode_tensor_image", ldt_amd.decode_tensor_image(_rb(mixed), size=ENTRY_SIZE, crop=crops,
                                                                          views=V))):
        _check_rows(mixed, ENTRY_SIZE, V, got["image"].cpu(), got["label"].cpu().numpy(), {}, what, crops=crops)
    with pytest.raises(ValueError):  # a 2-D array with views
        ldt_amd.collate_fn(items, size=ENTRY_SIZE, crop=crops[:, 0], views=V)
    with pytest.raises(ValueError):
        ldt_amd.collate_fn(items, size=ENTRY_SIZE, crop=crops, views=3)


def test_pipeline_with_a_seeded_sampler_and_to_tensor_fn(mixed):
    import torch

    import ldt_amd

    V = 2
    rb = _rb(mixed)
    wh, st = ldt_amd.image_sizes(rb.column(0))
    assert not st.any()
    want = ldt_amd.RandomResizedCropFlip(generator=torch.Generator().manual_seed(17))
    first, second = want.sample(wh, views=V), want.sample(wh, views=V)
    sampler = ldt_amd.RandomResizedCropFlip(generator=torch.Generator().manual_seed(17))
    pipe = ldt_amd.DecodePipeline(depth=2, size=ENTRY_SIZE, views=V, crop=sampler)
    a, b = pipe.decode(rb), pipe.decode(rb)  # the generator moves on between the batches
    pipe.check()
    torch.cuda.synchronize()
    for what, (img, lbl), boxes in (("pipeline batch 0", a, first), ("pipeline batch 1", b, second)):
        _check_rows(mixed, ENTRY_SIZE, V, img.cpu(), lbl.cpu().numpy(), {}, what, crops=boxes)
    # make_to_tensor_fn, the prefetch path included
    crops = _view_crops(mixed, V)
    fn = ldt_amd.make_to_tensor_fn(depth=2, size=ENTRY_SIZE, views=V, prefetch=1)
    got = fn(rb, crop=crops)
    fn.check()
    _check_rows(mixed, ENTRY_SIZE, V, got["image"].cpu(), got["label"].cpu().numpy(), {}, "to_tensor_fn", crops=crops)
    s2 = ldt_amd.RandomResizedCropFlip(generator=torch.Generator().manual_seed(17))
    fn = ldt_amd.make_to_tensor_fn(depth=2, size=ENTRY_SIZE, views=V, crop=s2, prefetch=1)
    outs = list(fn.iterate([rb, rb]))
    for what, got, boxes in (("iterate 0", outs[0], first), ("iterate 1", outs[1], second)):
        _check_rows(mixed, ENTRY_SIZE, V, got["image"].cpu(), got["label"].cpu().numpy(), {}, what, crops=boxes)


def test_device_batch_decodes_views_in_the_main_process(mixed):
    import torch

    import ldt_amd
    from ldt_amd import transforms as T

    V = 2
    images = [d for _, d in mixed]
    labels = list(range(100, 100 + len(images)))
    wh, _ = ldt_amd.image_sizes(images)
    want = ldt_amd.RandomResizedCropFlip(generator=torch.Generator().manual_seed(23)).sample(wh, views=V)
    sampler = ldt_amd.RandomResizedCropFlip(generator=torch.Generator().manual_seed(23))
    batch = T.DeviceBatch(T._pack_list(images, labels), size=ENTRY_SIZE, crop=sampler, views=V)
    _check_rows(mixed, ENTRY_SIZE, V, batch["image"].cpu(), batch["label"].cpu().numpy(), {}, "DeviceBatch(sampler)",
                crops=want)
    fc = ldt_amd.ResizeFiveCrop(64, ten=True)
    batch = T.DeviceBatch(T._pack_list(images, labels), size=(48, 48), window=fc).pin_memory()
    whs = np.array([_hw(n, d)[::-1] for n, d in mixed], np.int32)
    _check_rows(mixed, (48, 48), 10, batch["image"].cpu(), batch["label"].cpu().numpy(), {}, "DeviceBatch(ten-crop)",
                crops=fc.boxes(whs), windows=fc.sample(whs, None, (48, 48)))


# ---- cross-check: V single-view calls ----------------------------------------------------------------------

@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
def test_views_equal_single_view_calls(mixed, interp):
    import torch

    from ldt_amd import transforms as T

    V, size = 4, (64, 48)
    crops, windows = _view_crops(mixed, V), _view_windows(mixed, V, size)
    arr = _arrow(mixed)
    out, _ = T.decode_arrow(arr, size=size, crops=crops, windows=windows, views=V, interpolation=interp)
    assert tuple(out.shape) == (V, len(mixed), 3) + size and out.is_contiguous()
    for v in range(V):
        one, _ = T.decode_arrow(arr, size=size, crops=np.ascontiguousarray(crops[:, v]),
                                windows=np.ascontiguousarray(windows[:, v]), interpolation=interp)
        assert tuple(one.shape) == (len(mixed), 3) + size
        assert torch.equal(out[v], one), f"{interp}: view {v} differs from the single-view call"


# ---- unchanged paths and errors --------------------------------------------------------------------------

def test_views_are_consumed_and_errors_enqueue_nothing(mixed):
    import torch

    import ldt_amd
    from ldt_amd import _lib, synth
    from ldt_amd import transforms as T

    ctx = _lib.get_context(torch.cuda.current_device())
    size = (30, 33)
    arr = _arrow(mixed)
    n = len(mixed)
    plain = T.decode_arrow(arr, size=size)[0]
    assert tuple(plain.shape) == (n, 3) + size
    three = T.decode_arrow(arr, size=size, views=3)[0]
    assert tuple(three.shape) == (3, n, 3) + size
    again = T.decode_arrow(arr, size=size)[0]  # views=None after views=3: consumed, not sticky
    assert tuple(again.shape) == (n, 3) + size and torch.equal(again, plain)
    # the default path's routing is the parent's: the band kernel at 224 x 224, before and after
    T.decode_arrow(arr)
    band = ctx.lib.ldt_debug_last_resize(ctx.handle)
    assert band > 0
    T.decode_arrow(arr, views=2)
    assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 0
    T.decode_arrow(arr)
    assert ctx.lib.ldt_debug_last_resize(ctx.handle) == band
    # the C ABI: values outside 1..16 are refused and change nothing
    for bad in (0, 17, -1):
        assert ctx.lib.ldt_set_views(ctx.handle, bad) == _lib.LDT_ERR_ARG
    assert torch.equal(T.decode_arrow(arr, size=size)[0], plain)
    # ldt_set_views(1) through the C ABI is the call of today: the same 4-D result
    with ctx.lock:
        ctx.check(ctx.lib.ldt_set_views(ctx.handle, 1), "ldt_set_views")
    assert torch.equal(T.decode_arrow(arr, size=size)[0], plain)
    # n crops with views = 2: LDT_ERR_ARG, nothing enqueued, output untouched, and the setting is consumed
    crops = np.ascontiguousarray(_view_crops(mixed, 2)[:, 0])
    flat = torch.full((4096 + 2 * n * 3 * 30 * 33 + 4096,), -12345.5, dtype=torch.float32, device="cuda")
    lbl = torch.full((n,), -777, dtype=torch.int64, device="cuda")
    with ctx.lock:
        ctx.check(ctx.lib.ldt_set_views(ctx.handle, 2), "ldt_set_views")
    with pytest.raises(_lib.LdtError, match=r"rc=-1"):
        T.decode_arrow(arr, np.arange(n), out=flat[4096:4096 + n * 3 * 30 * 33].view(n, 3, 30, 33), out_lbl=lbl,
                       size=size, crops=crops)
    torch.cuda.synchronize()
    assert torch.all(flat == -12345.5).item() and torch.all(lbl == -777).item(), "a refused call wrote its output"
    with pytest.raises(ValueError):  # and the Python layer refuses it by shape
        T.decode_arrow(arr, size=size, crops=crops, views=2)
    assert torch.equal(T.decode_arrow(arr, size=size)[0], plain)
    # resize_raw after ldt_set_views(2) is refused, and the call after it works
    raw = torch.from_numpy(np.stack([synth.raw_hwc_one(33, 47, 61 + k) for k in range(3)]))
    want = ldt_amd.resize_raw(raw, 33, 47, size=size)
    with ctx.lock:
        ctx.check(ctx.lib.ldt_set_views(ctx.handle, 2), "ldt_set_views")
    with pytest.raises(_lib.LdtError, match=r"rc=-1"):
        ldt_amd.resize_raw(raw, 33, 47, size=size)
    assert torch.equal(ldt_amd.resize_raw(raw, 33, 47, size=size), want)
    assert torch.equal(T.decode_arrow(arr, size=size)[0], plain)
    # the grid order is an A/B switch only: the output does not depend on it
    crops3 = _view_crops(mixed, 3)
    a = T.decode_arrow(arr, size=size, crops=crops3, views=3)[0]
    ctx.set_option(_lib.OPT_VIEW_ORDER, 1)
    try:
        b = T.decode_arrow(arr, size=size, crops=crops3, views=3)[0]
    finally:
        ctx.set_option(_lib.OPT_VIEW_ORDER, 0)
    assert torch.equal(a, b)


def test_grid_limit_is_refused_not_overflowed():
    """n = 1024, V = 16 at 1024 x 1024 is 8.4 M workgroups and fits; the check
    that refuses more is reached with a row count whose product with V leaves
    an int, without allocating an output for it."""
    import torch

    from ldt_amd import _lib

    assert ((1024 + 7) // 8) * 8 * 16 * (1024 // 8) * (1024 // 256) == 8388608 < 2 ** 31
    ctx = _lib.Context(torch.cuda.current_device())
    n = (1 << 31) // 16 + 8  # n * 16 > INT_MAX
    offsets = np.zeros(2, np.int64)
    data = np.zeros(8, np.uint8)
    status = np.zeros(1, np.int32)
    out = torch.zeros(16, device="cuda")
    ctx.check(ctx.lib.ldt_set_views(ctx.handle, 16), "ldt_set_views")
    rc = ctx.lib.ldt_decode_batch_large(ctx.handle, data.ctypes.data, offsets.ctypes.data, 0, n, None, None, 0,
                                        out.data_ptr(), None, None, None, status.ctypes.data)
    assert rc == _lib.LDT_ERR_ARG
    assert b"workgroups" in ctx.lib.ldt_last_error(ctx.handle)
