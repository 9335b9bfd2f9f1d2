"""GPU tests of the resize's filter selection (ldt_set_filter,
``interpolation=``): every decode / resize entry point and every composition
the library has (plain, crop box, window, box + window, flip, Normalize, JPEG
and raw sources) against Pillow itself:

    Image.fromarray(src).resize((res_w, res_h), Image.BICUBIC)
         .crop((left, top, left + ow, top + oh)), mirrored when flipped,

``src`` being ``oracle.decode_rgb(cell)`` or the row's box of it. ToTensor /
Normalize is then ``oracle.raw_to_tensor(that_uint8, oh, ow, normalize=...)``:
the oracle's bilinear resize to the same size is the identity
(tests/test_interpolation.py asserts it). Max abs <= 2/255 is asserted first,
then bit equality, for every row.

One rule (`_expected`) says what every row must be: status 7 for a bad window,
else 6 for a bad box, else 4 for a source (box or whole image) with
``ceil(support * src / res) > 37`` on an axis against res (the window's
resized size, or the output size), support 2 for bicubic and 1 for bilinear; a
failed row is all zero with label -100; every other row is exact. Nothing is
skipped or filtered.
"""
import numpy as np
import pyarrow as pa
import pytest

from oracle import oracle
from test_gpu_window import SIZES, _ID, _check, _decode_guarded, _hw, _wh, _window_status, mixed  # noqa: F401
from test_interpolation import InterpolationMode, checkerboard

pytestmark = pytest.mark.gpu

_rgb_cache, _exp_cache = {}, {}


def _pil_window(src, size, window, flip, normalize=None, interp="bicubic"):
    """Pillow's resize of the h x w x 3 source to res with the filter, the
    window of it, mirrored when flipped, as a tensor."""
    from PIL import Image

    rh, rw, top, left = (int(v) for v in window)
    if interp == "bilinear":  # the oracle's own resize, as tests/test_gpu_window.py takes it
        t = oracle.raw_to_tensor(src, rh, rw, normalize=normalize)[:, top:top + size[0], left:left + size[1]]
        return np.ascontiguousarray(t[:, :, ::-1] if flip else t)
    im = Image.fromarray(np.ascontiguousarray(src)).resize((rw, rh), Image.BICUBIC)
    u8 = np.asarray(im.crop((left, top, left + size[1], top + size[0])), dtype=np.uint8)
    if flip:
        u8 = u8[:, ::-1]
    return oracle.raw_to_tensor(np.ascontiguousarray(u8), size[0], size[1], normalize=normalize)


def _expected(name, data, size, window=None, crop=None, normalize=None, interp="bicubic"):
    """Pillow's tensor for the row, or the status it must fail with."""
    h, w = _hw(name, data)
    btop, bleft, bh, bw, flip = (int(v) for v in crop) if crop is not None else (0, 0, h, w, 0)
    rh, rw, top, left = (int(v) for v in window) if window is not None else (size[0], size[1], 0, 0)
    key = (name, size, (rh, rw, top, left), (btop, bleft, bh, bw, flip), repr(normalize or None), interp)
    if key not in _exp_cache:
        s = 2 if interp == "bicubic" else 1
        if _window_status((rh, rw, top, left), size):
            _exp_cache[key] = 7
        elif btop < 0 or bleft < 0 or bh < 1 or bw < 1 or btop + bh > h or bleft + bw > w or flip not in (0, 1):
            _exp_cache[key] = 6
        elif -(-s * bw // rw) > 37 or -(-s * bh // rh) > 37:
            _exp_cache[key] = 4
        else:
            if name not in _rgb_cache:
                _rgb_cache[name] = oracle.decode_rgb(data)
            _exp_cache[key] = _pil_window(_rgb_cache[name][btop:btop + bh, bleft:bleft + bw], size,
                                          (rh, rw, top, left), flip, normalize, interp)
    return _exp_cache[key]


def _check_rows(cells, size, img, lbl, failed, what, windows=None, crops=None, normalize=None, interp="bicubic",
                label0=100):
    want_failed, exact = {}, 0
    assert len(img) == len(cells)
    for k, (name, data) in enumerate(cells):
        exp = _expected(name, data, size, None if windows is None else windows[k],
                        None if crops is None else crops[k], normalize, interp)
        if isinstance(exp, int):
            want_failed[k] = exp
            assert not img[k].any(), f"{what}: failed row {k} ({name}) is not all zero"
            assert lbl is None or lbl[k] == -100, f"{what}: failed row {k} label {lbl[k]}"
        else:
            _check(img[k], exp, f"{what}: {name} -> {size} {interp}")
            assert lbl is None or lbl[k] == label0 + k
            exact += 1
    assert failed == want_failed, f"{what}: failed rows {failed}, expected {want_failed}"
    return exact


def _ctx():
    import torch

    from ldt_amd import _lib

    return _lib.get_context(torch.cuda.current_device()), _lib


def _odd_boxes(cells):
    """A box per cell at an odd origin where the cell has room, every other one flipped."""
    rows = []
    for k, c in enumerate(cells):
        h, w = _hw(*c)
        top, left = (1 if h > 2 else 0), (1 if w > 2 else 0)
        rows.append([top, left, h - top - (1 if h > 4 else 0), w - left - (1 if w > 4 else 0), k & 1])
    return np.array(rows, np.int32)


def _corner_windows(n, size, extra=(17, 23)):
    """Five-crop style: the four corners and the centre of res = size + extra, in turn."""
    oh, ow = size
    rh, rw = oh + extra[0], ow + extra[1]
    corners = [(0, 0), (0, rw - ow), (rh - oh, 0), (rh - oh, rw - ow), ((rh - oh) // 2, (rw - ow) // 2)]
    return np.array([[rh, rw, *corners[k % 5]] for k in range(n)], np.int32)


# ---- plain BICUBIC at every size ----------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=_ID)
def test_plain_bicubic_on_every_cell(mixed, size):
    ctx, _ = _ctx()
    names = [n for n, _ in mixed]
    img, lbl, failed = _decode_guarded(mixed, size, interpolation="bicubic")
    assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 0  # the streaming kernel
    exact = _check_rows(mixed, size, img, lbl, failed, "plain bicubic")
    # bicubic differs from bilinear: the argument is not ignored
    k = names.index("up-8x8")
    assert not np.array_equal(img[k], _expected(*mixed[k], size, interp="bilinear"))
    if size == (7, 5):
        # 500 wide fails under either filter; 150 wide under bicubic only (ceil(300 / 5) = 60); 91 wide is
        # at the limit exactly (ceil(182 / 5) = 37, 75 taps) and succeeds
        assert failed == {names.index("420-375x500"): 4, names.index("444-100x150"): 4}
        assert -(-2 * 91 // 5) == 37 and names.index("gray-77x91") not in failed
        img, lbl, failed = _decode_guarded(mixed, size, interpolation="bilinear")
        assert failed == {names.index("420-375x500"): 4}
        assert _check_rows(mixed, size, img, lbl, failed, "the same call, bilinear", interp="bilinear") == len(mixed) - 1
    else:
        assert failed == {} and exact == len(mixed)


# ---- crops, windows, both, flip -----------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=_ID)
def test_bicubic_with_odd_origin_boxes_and_flip(mixed, size):
    ctx, _ = _ctx()
    crops = _odd_boxes(mixed)
    assert set(crops[:, 4].tolist()) == {0, 1} and crops[1].tolist() == [1, 1, 373, 498, 1]
    img, lbl, failed = _decode_guarded(mixed, size, crops=crops, interpolation="bicubic")
    assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 0
    exact = _check_rows(mixed, size, img, lbl, failed, "boxes", crops=crops)
    assert exact == len(mixed) - len(failed) and set(failed.values()) <= {4}
    assert (len(failed) == 2) if size == (7, 5) else not failed


def test_bicubic_with_resize_center_crop_windows(mixed):
    import ldt_amd

    size = (224, 224)
    windows = ldt_amd.ResizeCenterCrop(256).sample(_wh(mixed), None, size)
    assert windows[1].tolist() == [256, 341, 16, 58]
    img, lbl, failed = _decode_guarded(mixed, size, windows, interpolation="bicubic")
    assert failed == {} and _check_rows(mixed, size, img, lbl, failed, "Resize(256) + CenterCrop(224)",
                                        windows=windows) == len(mixed)


@pytest.mark.parametrize("size", [(224, 224), (30, 33), (7, 5)], ids=_ID)
def test_bicubic_with_boxes_corner_windows_and_flip(mixed, size):
    import ldt_amd

    ctx, _ = _ctx()
    crops = _odd_boxes(mixed)
    for what, windows in (("corners", _corner_windows(len(mixed), size)),
                          ("ResizeCenterCrop of the boxes",
                           ldt_amd.ResizeCenterCrop(max(size) + 32).sample(crops[:, [3, 2]], None, size))):
        img, lbl, failed = _decode_guarded(mixed, size, windows, crops, interpolation="bicubic")
        assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 0
        exact = _check_rows(mixed, size, img, lbl, failed, what, windows=windows, crops=crops)
        assert exact == len(mixed) - len(failed) and set(failed.values()) <= {4}
        assert exact >= len(mixed) - 2, (what, failed)
    # corner windows without boxes
    windows = _corner_windows(len(mixed), size, extra=(31, 49))
    img, lbl, failed = _decode_guarded(mixed, size, windows, interpolation="bicubic")
    assert _check_rows(mixed, size, img, lbl, failed, "corners, whole images", windows=windows) == len(mixed) - len(failed)


def test_a_rows_errors_keep_their_order(mixed):
    """window 7, then crop 6, then too large 4, each on its own row."""
    size = (7, 5)
    n = len(mixed)
    crops = np.array([[0, 0, *_hw(nm, d), 0] for nm, d in mixed], np.int32)
    windows = np.array([[8, 8, 0, 0]] * n, np.int32)  # 375 x 500 and 100 x 150 -> 8 x 8: too large
    windows[0] = [8, 8, 2, 0]           # not inside res
    crops[3] = [0, 0, 78, 91, 0]        # top + height == H + 1
    windows[1] = [8, 8, 2, 0]           # bad window on a row that is too large as well
    crops[2] = [0, 0, 101, 150, 0]      # bad box on a row that is too large as well
    img, lbl, failed = _decode_guarded(mixed, size, windows, crops, interpolation="bicubic")
    assert failed == {0: 7, 1: 7, 2: 6, 3: 6}
    _check_rows(mixed, size, img, lbl, failed, "order", windows=windows, crops=crops)
    windows[1] = [8, 8, 0, 0]
    crops[2] = [0, 0, 100, 150, 0]
    img, lbl, failed = _decode_guarded(mixed, size, windows, crops, interpolation="bicubic")
    assert failed == {0: 7, 1: 4, 2: 4, 3: 6}
    _check_rows(mixed, size, img, lbl, failed, "order, one error each", windows=windows, crops=crops)
    # the boundary on a JPEG row: a box of 148 onto res 8 is exact (75 taps), 149 fails alone
    windows[:] = [8, 8, 1, 3]
    crops[:] = [0, 0, 5, 5, 0]
    crops[1] = [3, 5, 148, 148, 1]
    img, lbl, failed = _decode_guarded(mixed, size, windows, crops, interpolation="bicubic")
    assert failed == {} and _check_rows(mixed, size, img, lbl, failed, "148 -> 8", windows=windows, crops=crops) == n
    for box in ([3, 5, 148, 149, 1], [3, 5, 149, 148, 0]):
        crops[1] = box
        img, lbl, failed = _decode_guarded(mixed, size, windows, crops, interpolation="bicubic")
        assert failed == {1: 4}, (box, failed)
        assert _check_rows(mixed, size, img, lbl, failed, f"149 -> 8 {box}", windows=windows, crops=crops) == n - 1


# ---- Normalize ----------------------------------------------------------------------------------

def test_bicubic_with_normalize(mixed):
    size = (30, 33)
    for normalize in (True, ((0.5, 0.4, 0.3), (0.2, 0.25, 0.3))):
        img, lbl, failed = _decode_guarded(mixed, size, normalize=normalize, interpolation="bicubic")
        assert _check_rows(mixed, size, img, lbl, failed, "normalize", normalize=normalize) == len(mixed)
    crops, windows = _odd_boxes(mixed), _corner_windows(len(mixed), size)
    img, lbl, failed = _decode_guarded(mixed, size, windows, crops, normalize=True, interpolation="bicubic")
    assert _check_rows(mixed, size, img, lbl, failed, "normalize, boxes and windows", windows=windows, crops=crops,
                       normalize=True) == len(mixed)


# ---- raw sources --------------------------------------------------------------------------------

RAW_CASES = [
    # (h, w), size, boxes, windows
    ((8, 8), (224, 224), [[1, 1, 7, 7, 0], [0, 1, 8, 6, 1], [3, 2, 4, 5, 1]],
     [[256, 256, 16, 16], [224, 224, 0, 0], [230, 300, 6, 76]]),
    ((17, 5), (30, 33), [[1, 1, 15, 3, 0], [0, 0, 17, 5, 1], [2, 1, 9, 4, 1]],
     [[61, 82, 31, 49], [30, 33, 0, 0], [35, 40, 5, 7]]),
]


@pytest.mark.parametrize("case", RAW_CASES, ids=["8x8-224x224", "17x5-30x33"])
def test_resize_raw_bicubic(case):
    import torch

    import ldt_amd

    (h, w), size, boxes, windows = case
    raw = np.stack([checkerboard(h, w, 300 + k) for k in range(3)])
    boxes, windows = np.array(boxes, np.int32), np.array(windows, np.int32)
    arrow = pa.array([raw[k].tobytes() for k in range(3)], pa.binary(h * w * 3))
    zeros = ones = 0
    for src in (torch.from_numpy(raw), torch.from_numpy(raw).cuda(), arrow):
        for bx, wn, normalize in ((None, None, False), (boxes, None, True), (None, windows, False), (boxes, windows, True)):
            out = ldt_amd.resize_raw(src, h, w, normalize=normalize, size=size, crops=bx, windows=wn,
                                     interpolation="bicubic").cpu().numpy()
            assert out.shape == (3, 3) + size
            for k in range(3):
                t, l, bh, bw, f = boxes[k].tolist() if bx is not None else (0, 0, h, w, 0)
                win = windows[k] if wn is not None else (size[0], size[1], 0, 0)
                exp = _pil_window(raw[k, t:t + bh, l:l + bw], size, win, f, normalize=normalize or None)
                _check(out[k], exp, f"raw {type(src).__name__} row {k} boxes={bx is not None} windows={wn is not None}")
                if not normalize:
                    zeros += np.count_nonzero(exp == 0.0)
                    ones += np.count_nonzero(exp == 1.0)
    assert zeros > 0 and ones > 0  # the clamp at both ends is exercised
    # bilinear afterwards on the same context is the oracle's
    plain = ldt_amd.resize_raw(torch.from_numpy(raw), h, w, size=size, normalize=False).cpu().numpy()
    for k in range(3):
        _check(plain[k], oracle.raw_to_tensor(raw[k], *size), "raw bilinear after bicubic")
        assert not np.array_equal(plain[k], _pil_window(raw[k], size, (size[0], size[1], 0, 0), 0))


def test_resize_raw_bicubic_limit():
    import torch

    import ldt_amd

    wide = np.stack([checkerboard(9, 149, 77)])
    # 148 columns onto 8: ceil(296 / 8) = 37, 75 taps
    ok = np.ascontiguousarray(wide[:, :, :148])
    out = ldt_amd.resize_raw(torch.from_numpy(ok), 9, 148, size=(5, 8), normalize=False, interpolation="bicubic")
    _check(out.cpu().numpy()[0], _pil_window(ok[0], (5, 8), (5, 8, 0, 0), 0), "raw 148 -> 8")
    out = ldt_amd.resize_raw(torch.from_numpy(wide), 9, 149, size=(5, 8), normalize=False, interpolation="bicubic",
                             crops=[[0, 1, 9, 148, 1]])
    _check(out.cpu().numpy()[0], _pil_window(wide[0, :, 1:149], (5, 8), (5, 8, 0, 0), 1), "raw box of 148 -> 8")
    with pytest.raises(ldt_amd.LdtError, match=r"rc=-1"):  # 149: an argument error
        ldt_amd.resize_raw(torch.from_numpy(wide), 9, 149, size=(5, 8), interpolation="bicubic")
    with pytest.raises(ldt_amd.LdtError, match=r"rc=-1"):
        ldt_amd.resize_raw(torch.from_numpy(wide), 9, 149, size=(5, 8), interpolation="bicubic",
                           windows=[[5, 8, 0, 0]])
    with pytest.raises(ldt_amd.LdtError, match=r"rc=-1"):  # the vertical axis: 149 rows onto 8
        ldt_amd.resize_raw(torch.from_numpy(np.ascontiguousarray(wide.transpose(0, 2, 1, 3))), 149, 9, size=(8, 5),
                           interpolation="bicubic")
    # bilinear takes 149 columns onto 8 as before
    out = ldt_amd.resize_raw(torch.from_numpy(wide), 9, 149, size=(5, 8), normalize=False)
    _check(out.cpu().numpy()[0], oracle.raw_to_tensor(wide[0], 5, 8), "raw 149 -> 8 bilinear")


# ---- entry points -------------------------------------------------------------------------------

ENTRY_SIZE = (30, 33)


@pytest.fixture(scope="module")
def rb(mixed):
    return pa.RecordBatch.from_arrays([pa.array([d for _, d in mixed], pa.binary()),
                                       pa.array(np.arange(100, 100 + len(mixed)), pa.int64())], names=["image", "label"])


def _check_out(mixed, out, what, interp="bicubic", size=ENTRY_SIZE, **kw):
    keyed = isinstance(out, dict) or hasattr(out, "keys")
    img = (out["image"] if keyed else out[0]).cpu().numpy()
    lbl = (out["label"] if keyed else out[1]).cpu().numpy()
    assert img.shape == (len(mixed), 3) + size
    assert _check_rows(mixed, size, img, lbl, {}, what, interp=interp, **kw) == len(mixed)


def test_decode_tensor_image_and_collate_fn(mixed, rb):
    from PIL import Image

    import ldt_amd

    for spelling in ("bicubic", "BICUBIC", InterpolationMode.BICUBIC, Image.BICUBIC, 3):
        _check_out(mixed, ldt_amd.decode_tensor_image(rb, size=ENTRY_SIZE, interpolation=spelling), f"{spelling!r}")
    _check_out(mixed, ldt_amd.decode_tensor_image(rb, size=ENTRY_SIZE, interpolation=None), "None", interp="bilinear")
    _check_out(mixed, ldt_amd.decode_tensor_image(rb, size=ENTRY_SIZE), "default", interp="bilinear")
    with pytest.raises(ValueError, match="lanczos"):  # never a silent bilinear result
        ldt_amd.decode_tensor_image(rb, size=ENTRY_SIZE, interpolation="lanczos")
    items = [{"image": d, "label": 100 + k} for k, (_, d) in enumerate(mixed)]
    _check_out(mixed, ldt_amd.collate_fn(items, size=ENTRY_SIZE, interpolation="bicubic"), "collate_fn")
    _check_out(mixed, ldt_amd.collate_fn(rb, size=ENTRY_SIZE, interpolation="bicubic"), "collate_fn(RecordBatch)")
    _check_out(mixed, ldt_amd.make_collate_fn(size=ENTRY_SIZE, interpolation="bicubic")(items), "make_collate_fn")
    _check_out(mixed, ldt_amd.make_collate_fn(size=ENTRY_SIZE)(items), "make_collate_fn()", interp="bilinear")
    # with a window sampler and a crop array
    sampler = ldt_amd.ResizeCenterCrop(40)
    crops = _odd_boxes(mixed)
    want = sampler.sample(crops[:, [3, 2]], None, ENTRY_SIZE)
    out = ldt_amd.decode_tensor_image(rb, size=ENTRY_SIZE, interpolation="bicubic", window=sampler, crop=crops)
    _check_out(mixed, out, "crop + window sampler", windows=want, crops=crops)


def test_device_batch_decodes_with_the_filter_it_carries(mixed):
    from ldt_amd import transforms as T

    images = [d for _, d in mixed]
    labels = list(range(100, 100 + len(images)))
    batch = T.DeviceBatch(T._pack_list(images, labels), size=ENTRY_SIZE, interpolation="bicubic")
    _check_out(mixed, batch, "DeviceBatch(bicubic)")
    batch = T.DeviceBatch(T._pack_list(images, labels), size=ENTRY_SIZE)
    _check_out(mixed, batch.pin_memory(), "DeviceBatch()", interp="bilinear")


def test_resident_batch_and_pipeline(mixed, rb):
    import torch

    import ldt_amd

    res = ldt_amd.ResidentBatch([d for _, d in mixed], np.arange(100, 100 + len(mixed)))
    _check_out(mixed, res.decode(size=ENTRY_SIZE, interpolation="bicubic"), "ResidentBatch.decode")
    _check_out(mixed, res.decode(size=ENTRY_SIZE), "ResidentBatch.decode()", interp="bilinear")
    # the constructor's default, and a call's own filter in its place; depth 2, alternating filters in flight
    pipe = ldt_amd.DecodePipeline(depth=2, size=ENTRY_SIZE, interpolation="bicubic")
    assert pipe.interpolation == "bicubic"
    plan = [None, "bilinear", None, "bilinear", "bicubic", "bilinear"]
    outs = [pipe.decode(res if b % 3 == 0 else rb, interpolation=plan[b]) for b in range(len(plan))]
    pipe.check()
    torch.cuda.synchronize()
    for b, out in enumerate(outs):
        _check_out(mixed, out, f"pipeline batch {b}", interp=plan[b] or "bicubic")
    pipe = ldt_amd.DecodePipeline(depth=2, size=ENTRY_SIZE)
    assert pipe.interpolation == "bilinear"
    plan = ["bicubic", None, "bicubic", None, None, "bicubic"]
    windows = _corner_windows(len(mixed), ENTRY_SIZE)
    outs = [pipe.decode(rb, interpolation=plan[b], windows=windows if b >= 4 else None) for b in range(len(plan))]
    pipe.check()
    for b, out in enumerate(outs):
        _check_out(mixed, out, f"default pipeline batch {b}", interp=plan[b] or "bilinear",
                   windows=windows if b >= 4 else None)
    with pytest.raises(ValueError, match="hamming"):
        pipe.decode(rb, interpolation="hamming")
    with pytest.raises(ValueError, match="nearest"):
        ldt_amd.DecodePipeline(depth=1, interpolation="nearest")


def test_to_tensor_fn_bound_default_and_per_call(mixed, rb):
    import ldt_amd

    fn = ldt_amd.make_to_tensor_fn(depth=2, size=ENTRY_SIZE, interpolation="bicubic")
    a, b, c = fn(rb), fn(rb, interpolation="bilinear"), fn(rb)
    fn.check()
    _check_out(mixed, a, "to_tensor_fn(bicubic)")
    _check_out(mixed, b, "to_tensor_fn(bicubic), a bilinear call", interp="bilinear")
    _check_out(mixed, c, "to_tensor_fn(bicubic), third call")
    fn = ldt_amd.make_to_tensor_fn(depth=2, size=ENTRY_SIZE)
    a, b = fn(rb, interpolation=InterpolationMode.BICUBIC), fn(rb)
    fn.check()
    _check_out(mixed, a, "to_tensor_fn(), a bicubic call")
    _check_out(mixed, b, "to_tensor_fn(), default", interp="bilinear")


# ---- the filter is context state that no call leaks ---------------------------------------------

def test_bicubic_bilinear_bicubic_on_one_context(mixed):
    from ldt_amd import transforms as T

    ctx, _lib = _ctx()
    size = (224, 224)
    arr = pa.array([d for _, d in mixed], pa.binary())
    first = T.decode_arrow(arr, size=size, interpolation="bicubic")[0].cpu().numpy()
    assert ctx.filter() == "bicubic" and ctx.lib.ldt_debug_last_resize(ctx.handle) == 0
    plain = T.decode_arrow(arr, size=size)[0].cpu().numpy()
    assert ctx.filter() == "bilinear"
    assert ctx.lib.ldt_debug_last_resize(ctx.handle) > 0  # back on the band kernel
    again = T.decode_arrow(arr, size=size, interpolation="bicubic")[0].cpu().numpy()
    assert np.array_equal(first, again)
    for k, (name, data) in enumerate(mixed):
        _check(plain[k], oracle.raw_to_tensor(oracle.decode_rgb(data), *size), f"bilinear between: {name}")
        _check(first[k], _expected(name, data, size), f"bicubic: {name}")
    T.decode_arrow(arr, size=size)  # leave the shared context as the other tests expect it
    assert ctx.filter() == "bilinear"


def test_the_abi_filter_state():
    import ctypes

    import torch

    from ldt_amd import _lib

    ctx = _lib.Context(torch.cuda.current_device())  # a context of its own: the calls below go past use_filter
    f = ctypes.c_int(-1)
    assert ctx.lib.ldt_get_filter(ctx.handle, ctypes.byref(f)) == 0 and f.value == 0  # bilinear until set
    assert ctx.lib.ldt_set_filter(ctx.handle, 1) == 0 and ctx.filter() == "bicubic"
    for bad in (2, 3, -1, 1 << 20):
        assert ctx.lib.ldt_set_filter(ctx.handle, bad) == _lib.LDT_ERR_ARG
        assert ctx.filter() == "bicubic"  # a refused value changes nothing
    assert ctx.lib.ldt_get_filter(ctx.handle, None) == 0
    # sticky: a raw resize made now, with no filter named again, is bicubic
    raw = np.stack([checkerboard(8, 8, 5)])
    out = torch.empty((1, 3, 224, 224), dtype=torch.float32, device="cuda")
    src = torch.from_numpy(raw)
    for _ in range(2):
        rc = ctx.lib.ldt_resize_raw(ctx.handle, src.data_ptr(), 0, 1, 8, 8, 8 * 8 * 3, out.data_ptr(), None,
                                    torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        _check(out.cpu().numpy()[0], _pil_window(raw[0], (224, 224), (224, 224, 0, 0), 0), "sticky bicubic")
    assert ctx.lib.ldt_set_filter(ctx.handle, 0) == 0
    rc = ctx.lib.ldt_resize_raw(ctx.handle, src.data_ptr(), 0, 1, 8, 8, 8 * 8 * 3, out.data_ptr(), None,
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    _check(out.cpu().numpy()[0], oracle.raw_to_tensor(raw[0], 224, 224), "bilinear again")


def test_bicubic_takes_the_streaming_kernel_under_every_option(mixed):
    from ldt_amd import transforms as T

    ctx, _lib = _ctx()
    arr = pa.array([d for _, d in mixed], pa.binary())
    plain = T.decode_arrow(arr)[0].cpu().numpy()
    before = ctx.lib.ldt_debug_last_resize(ctx.handle)
    assert before > 0  # bilinear at 224 x 224: the band kernel
    want = None
    for impl in (0, 1, 2, 3):
        ctx.set_option(_lib.OPT_RESIZE_IMPL, impl)
        try:
            got = T.decode_arrow(arr, interpolation="bicubic")[0].cpu().numpy()
            assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 0
            want = got if want is None else want
            assert np.array_equal(got, want), f"LDT_OPT_RESIZE_IMPL {impl} gives another bicubic tensor"
        finally:
            ctx.set_option(_lib.OPT_RESIZE_IMPL, 0)
    for k, (name, data) in enumerate(mixed):
        _check(want[k], _expected(name, data, (224, 224)), f"bicubic under every option: {name}")
    again = T.decode_arrow(arr)[0].cpu().numpy()
    assert ctx.lib.ldt_debug_last_resize(ctx.handle) == before
    assert np.array_equal(again, plain)
