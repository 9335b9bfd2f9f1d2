"""GPU tests of the per-image resized size and window (ldt_set_windows,
``windows=`` / ``window=``): every decode / resize entry point against the
oracle composition

    raw_to_tensor(src, res_h, res_w)[:, top:top+oh, left:left+ow], mirrored when flip,

``src`` being the decoded image or the row's box of it, which
tests/test_window.py pins to Pillow's ``resize().crop()`` on the CPU. Max abs
<= 2/255 is asserted first, then bit equality.

One rule (`_expected`) says what every row must be: status 7 for a window
whose res is outside 1..65535, whose origin is negative or which is not inside
res; else status 6 for a bad box; else status 4 for a source (box or whole
image) reduced by more than 37 against res on an axis; a failed row is all
zero with label -100; every other row is exact. Every row of every case has
an expected value: nothing is skipped or filtered.
"""
import numpy as np
import pyarrow as pa
import pytest

import jpeg_recode as jr
from conftest import read_golden
from oracle import oracle

pytestmark = pytest.mark.gpu

TOL = 2.0 / 255.0
SIZES = [(224, 224), (7, 5), (30, 33), (299, 299)]  # (299, 299): two column tiles
SENTINEL = -12345.5
_ID = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


def _check(got, exp, what):
    diff = np.abs(got.astype(np.float64) - exp.astype(np.float64))
    assert diff.max() <= TOL, f"{what}: max abs {diff.max()} > 2/255 (mean {diff.mean()})"
    assert np.array_equal(got, exp), f"{what}: not bit-exact (max abs {diff.max()}, {np.count_nonzero(diff)} differ)"


@pytest.fixture(scope="module")
def mixed():
    """The mixed batch of tests/test_gpu_crop.py: (name, data) in a fixed
    order; the names give height x width."""
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
    ]


_rgb_cache, _exp_cache = {}, {}


def _hw(name, data):
    w, h, _ = oracle.jpeg_info(data)
    return h, w


def _window_status(window, size):
    rh, rw, top, left = (int(v) for v in window)
    if not (1 <= rh <= 65535 and 1 <= rw <= 65535) or top < 0 or left < 0 or size[0] > rh - top or size[1] > rw - left:
        return 7
    return 0


def _window_of(src, size, window, flip, normalize=None):
    """The oracle's window of the h x w x 3 source resized to res."""
    rh, rw, top, left = (int(v) for v in window)
    t = oracle.raw_to_tensor(src, rh, rw, normalize=normalize)[:, top:top + size[0], left:left + size[1]]
    return np.ascontiguousarray(t[:, :, ::-1] if flip else t)


def _expected(name, data, size, window, crop=None, normalize=None):
    """The oracle's tensor for the row, or the status it must fail with."""
    h, w = _hw(name, data)
    btop, bleft, bh, bw, flip = (int(v) for v in crop) if crop is not None else (0, 0, h, w, 0)
    rh, rw, top, left = (int(v) for v in window)
    key = (name, size, (rh, rw, top, left), (btop, bleft, bh, bw, flip), bool(normalize))
    if key not in _exp_cache:
        if _window_status(window, size):
            _exp_cache[key] = 7
        elif btop < 0 or bleft < 0 or bh < 1 or bw < 1 or btop + bh > h or bleft + bw > w or flip not in (0, 1):
            _exp_cache[key] = 6
        elif -(-bw // rw) > 37 or -(-bh // rh) > 37:
            _exp_cache[key] = 4
        else:
            if name not in _rgb_cache:
                _rgb_cache[name] = oracle.decode_rgb(data)
            _exp_cache[key] = _window_of(_rgb_cache[name][btop:btop + bh, bleft:bleft + bw], size, window, flip,
                                         normalize)
    return _exp_cache[key]


def _ctx():
    import torch

    from ldt_amd import _lib

    return _lib.get_context(torch.cuda.current_device()), _lib


def _decode_guarded(cells, size, windows=None, crops=None, guard=4096, normalize=None, **kw):
    """decode_arrow into the middle of a larger buffer full of a sentinel.
    Returns (images, labels, {failed row: status}); asserts the guards are
    untouched."""
    import torch

    import ldt_amd
    from ldt_amd import transforms as T

    n, (h, w) = len(cells), size
    cell = 3 * h * w
    flat = torch.full((guard + n * cell + guard,), SENTINEL, dtype=torch.float32, device="cuda")
    lflat = torch.full((n + 2,), -777, dtype=torch.int64, device="cuda")
    out = flat[guard:guard + n * cell].view(n, 3, h, w)
    labels = np.arange(100, 100 + n, dtype=np.int64)
    failed = {}
    try:
        T.decode_arrow(pa.array([d for _, d in cells], pa.binary()), labels, out=out, out_lbl=lflat[1:n + 1],
                       size=size, normalize=normalize, crops=crops, windows=windows, **kw)
    except ldt_amd.ImageDecodeError as e:
        failed = dict(e.rows)
    finally:
        torch.cuda.synchronize()
        assert torch.all(flat[:guard] == SENTINEL).item(), f"{size}: wrote before the output"
        assert torch.all(flat[guard + n * cell:] == SENTINEL).item(), f"{size}: wrote past the output"
        assert int(lflat[0]) == -777 and int(lflat[n + 1]) == -777
    return out.cpu().numpy(), lflat[1:n + 1].cpu().numpy(), failed


def _check_rows(cells, size, windows, img, lbl, failed, what, crops=None, normalize=None, other_failed=None,
                label0=100):
    """Every row against `_expected`; `other_failed`: rows that fail for a
    reason of their own (a corrupt cell), with their status."""
    other_failed = other_failed or {}
    want_failed, exact = {}, 0
    assert len(windows) == len(cells) == len(img) and (crops is None or len(crops) == len(cells))
    for k, (name, data) in enumerate(cells):
        exp = other_failed[k] if k in other_failed else \
            _expected(name, data, size, windows[k], None if crops is None else crops[k], normalize)
        assert exp is not None, f"{what}: row {k} ({name}) has no expected value"
        if isinstance(exp, int):
            want_failed[k] = exp
            assert not img[k].any(), f"{what}: failed row {k} ({name}) is not all zero"
            assert lbl is None or lbl[k] == -100, f"{what}: failed row {k} label {lbl[k]}"
        else:
            _check(img[k], exp, f"{what}: {name} window {list(windows[k])} -> {size}")
            assert lbl is None or lbl[k] == label0 + k
            exact += 1
    assert failed == want_failed, f"{what}: failed rows {failed}, expected {want_failed}"
    return exact


def _wh(cells):
    return np.array([_hw(n, d)[::-1] for n, d in cells], np.int32)


# ---- Resize(edge) + CenterCrop(size) -------------------------------------------------------------

@pytest.mark.parametrize("edge,size", [(256, (224, 224)), (8, (7, 5))], ids=["256-224", "8-7x5"])
def test_resize_center_crop_on_every_cell(mixed, edge, size):
    import ldt_amd

    ctx, _ = _ctx()
    windows = ldt_amd.ResizeCenterCrop(edge).sample(_wh(mixed), None, size)
    assert windows[1].tolist() == ([256, 341, 16, 58] if edge == 256 else [8, 10, 0, 2])
    img, lbl, failed = _decode_guarded(mixed, size, windows)
    exact = _check_rows(mixed, size, windows, img, lbl, failed, f"ResizeCenterCrop({edge})")
    assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 0
    # Resize(8) reduces the 500-wide cell by 50 (status 4, alone); every other row is exact
    assert failed == ({} if edge == 256 else {1: 4}) and exact == len(mixed) - len(failed)


# ---- window positions at every size ---------------------------------------------------------------

def _families(cells, size):
    """name -> int32 [n, 4], every window inside its res."""
    oh, ow = size
    n = len(cells)
    return {
        # flush with the bottom-right corner of res, at an odd top and left
        "flush-bottom-right": np.array([[oh + 31, ow + 49, 31, 49]] * n, np.int32),
        # each cell's own size as res: the window is a plain crop of an identity resize where it fits
        "own-size": np.array([[max(h, oh), max(w, ow), max(h, oh) - oh, (max(w, ow) - ow) // 2]
                              for h, w in (_hw(*c) for c in cells)], np.int32),
        # res far above out: an upscale of every cell on both axes, three taps
        "res_w-2000": np.array([[600 + oh, 2000, 599, 2000 - ow]] * n, np.int32),
        # a window in the first rows and columns of a reduced res
        "top-left-of-a-reduction": np.array([[oh + 3, ow + 9, 0, 0]] * n, np.int32),
    }


@pytest.mark.parametrize("size", SIZES, ids=_ID)
def test_window_families_on_every_cell(mixed, size):
    ctx, _ = _ctx()
    fams = _families(mixed, size)
    for fname, windows in fams.items():
        assert all(_window_status(w, size) == 0 for w in windows)
        img, lbl, failed = _decode_guarded(mixed, size, windows)
        exact = _check_rows(mixed, size, windows, img, lbl, failed, fname)
        assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 0
        assert exact == len(mixed) - len(failed)
        # only the 500 x 375 cell can be over the limit, and only against the small res of (7, 5)
        assert failed == ({1: 4} if size == (7, 5) and fname == "top-left-of-a-reduction" else {}), (fname, failed)
    flush = fams["flush-bottom-right"][0]
    assert flush[2] + size[0] == flush[0] and flush[3] + size[1] == flush[1] and flush[2] % 2 == 1 and flush[3] % 2 == 1
    assert fams["res_w-2000"][0, 3] == 2000 - size[1]


def test_sizes_have_a_short_last_band_and_two_column_tiles():
    assert [s[0] % 8 for s in SIZES] == [0, 7, 6, 3] and SIZES[-1][1] > 256


# ---- the limit is against res ---------------------------------------------------------------------

def test_reduction_of_37_is_exact_and_38_fails_alone(mixed):
    size = (7, 5)
    n = len(mixed)
    whole = np.array([[0, 0, *_hw(nm, d), k & 1] for k, (nm, d) in enumerate(mixed)], np.int32)
    # res == each cell's own size but for the 375 x 500 cell: a 370 x 370 box of it onto 10 x 10
    windows = np.array([[max(h, 7), max(w, 5), 0, 0] for h, w in (_hw(*c) for c in mixed)], np.int32)
    windows[1] = [10, 10, 3, 5]
    crops = whole.copy()
    crops[1] = [1, 3, 370, 370, 1]
    img, lbl, failed = _decode_guarded(mixed, size, windows, crops)
    assert failed == {}
    assert _check_rows(mixed, size, windows, img, lbl, failed, "reduction 37", crops=crops) == n
    for box in ([1, 3, 370, 371, 1], [1, 3, 371, 370, 0]):
        crops[1] = box
        img, lbl, failed = _decode_guarded(mixed, size, windows, crops)
        assert failed == {1: 4}, (box, failed)
        assert _check_rows(mixed, size, windows, img, lbl, failed, f"reduction 38 {box}", crops=crops) == n - 1
    # without crops the source is the whole image: 500 / 14 -> 36, 375 / 11 -> 35; 500 / 13 -> 39
    windows[1] = [11, 14, 4, 9]
    img, lbl, failed = _decode_guarded(mixed, size, windows)
    assert failed == {} and _check_rows(mixed, size, windows, img, lbl, failed, "whole image within the limit") == n
    windows[1] = [11, 13, 4, 8]
    img, lbl, failed = _decode_guarded(mixed, size, windows)
    assert failed == {1: 4}
    assert _check_rows(mixed, size, windows, img, lbl, failed, "whole image over the limit") == n - 1
    # the output size alone no longer decides: unwindowed, the cell is over the limit at (7, 5)
    assert _decode_guarded(mixed, size)[2] == {1: 4}


# ---- res == out is the unwindowed decode -----------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=_ID)
def test_identity_window_is_the_unwindowed_result(mixed, size):
    ctx, _ = _ctx()
    plain, lbl0, failed0 = _decode_guarded(mixed, size)
    band = ctx.lib.ldt_debug_last_resize(ctx.handle)
    if size == (224, 224):
        assert band > 0  # the default decode takes the band kernel: this ties the new variant to k_resize4
    if size[1] > 256:
        assert band == 0  # wider than one band-kernel tile: the streaming kernel either way
    windows = np.array([[size[0], size[1], 0, 0]] * len(mixed), np.int32)
    same, lbl, failed = _decode_guarded(mixed, size, windows)
    assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 0
    assert failed == failed0 and np.array_equal(lbl, lbl0)
    assert np.array_equal(same, plain), "res == out windows at (0, 0) differ from the call without windows"
    exact = _check_rows(mixed, size, windows, same, lbl, failed, "identity window")
    assert exact == len(mixed) - len(failed0) and len(failed0) == (1 if size == (7, 5) else 0)


# ---- with crops and flip ----------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=_ID)
def test_random_boxes_with_windows_and_flip(mixed, size):
    import torch

    import ldt_amd

    oh, ow = size
    rng = np.random.default_rng(1000 + oh)
    flips = []
    for draw in range(3):
        g = torch.Generator().manual_seed(50 + draw)
        crops = ldt_amd.RandomResizedCropFlip(generator=g).sample(_wh(mixed))
        if draw == 0:  # Resize(edge) + CenterCrop of the boxes, the edge just large enough
            windows = ldt_amd.ResizeCenterCrop(max(oh, ow) + 9).sample(crops[:, [3, 2]], None, size)
        else:  # a random res and a random window of it
            rh = rng.integers(oh, oh + 120, len(mixed))
            rw = rng.integers(ow, ow + 160, len(mixed))
            windows = np.stack([rh, rw, rng.integers(0, rh - oh + 1), rng.integers(0, rw - ow + 1)], axis=1).astype(np.int32)
        flips += crops[:, 4].tolist()
        img, lbl, failed = _decode_guarded(mixed, size, windows, crops)
        exact = _check_rows(mixed, size, windows, img, lbl, failed, f"draw {draw}", crops=crops)
        assert exact == len(mixed) - len(failed) and set(failed.values()) <= {4}
        assert exact >= len(mixed) // 2, (draw, failed)
    assert set(flips) == {0, 1}


# ---- bad windows -------------------------------------------------------------------------------------

def test_bad_windows_fail_their_own_rows(mixed):
    size = (30, 33)
    cells = mixed + [("truncated", read_golden("jpeg/bad_truncated.bin"))]
    good = np.array([[61, 82, 31, 49]] * len(cells), np.int32)
    bad = {0: [0, 82, 0, 0],           # res_h == 0
           1: [61, 65536, 0, 0],       # res_w above LDT_MAX_RES
           2: [61, 82, -1, 0],         # a negative top
           3: [61, 82, 0, -1],         # a negative left
           4: [61, 82, 32, 49],        # top + out_h == res_h + 1
           5: [61, 82, 31, 50],        # left + out_w == res_w + 1
           6: [29, 32, 0, 0],          # res smaller than the output: torchvision would pad
           7: [2147483647, 82, 2147483647, -2147483648]}
    for rows in ([0], [1], [2], [3], [4], [5], [6], [7], [0, 2, 4, 6], list(range(8))):
        windows = good.copy()
        for r in rows:
            windows[r] = bad[r]
        img, lbl, failed = _decode_guarded(cells, size, windows)
        assert failed == {**{r: 7 for r in rows}, 8: 3}, (rows, failed)
        assert _check_rows(cells, size, windows, img, lbl, failed, f"bad windows {rows}", other_failed={8: 3}) == \
            8 - len(rows)
    # a bad box beside a bad window: each row keeps its own status
    windows = good.copy()
    windows[2] = bad[2]
    crops = np.array([[0, 0, *_hw(n, d), 0] for n, d in cells], np.int32)
    crops[4] = [0, 0, 65, 80, 1]  # top + height == H + 1 on the 64 x 80 cell
    img, lbl, failed = _decode_guarded(cells, size, windows, crops)
    assert failed == {2: 7, 4: 6, 8: 3}
    assert _check_rows(cells, size, windows, img, lbl, failed, "bad box and bad window", crops=crops,
                       other_failed={8: 3}) == 6


def test_windows_apply_to_one_call(mixed):
    import torch

    from ldt_amd import transforms as T

    ctx, _lib = _ctx()
    size = (30, 33)
    plain, _, _ = _decode_guarded(mixed, size)
    band = ctx.lib.ldt_debug_last_resize(ctx.handle)
    windows = np.array([[61, 82, 31, 49]] * len(mixed), np.int32)
    img, lbl, failed = _decode_guarded(mixed, size, windows)
    _check_rows(mixed, size, windows, img, lbl, failed, "first call")
    assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 0
    # after a windowed batch a plain batch on the same context takes the path it took before and is exact
    # (at 224 x 224, the band kernel: test_windowed_batches_take_the_streaming_kernel_under_every_option)
    again, _, _ = _decode_guarded(mixed, size)
    assert ctx.lib.ldt_debug_last_resize(ctx.handle) == band
    assert np.array_equal(again, plain), "windows outlived their call"
    # windows for the wrong number of rows: LDT_ERR_ARG, nothing enqueued, and they are consumed
    n = len(mixed)
    flat = torch.full((4096 + n * 3 * 30 * 33 + 4096,), SENTINEL, dtype=torch.float32, device="cuda")
    lbl = torch.full((n,), -777, dtype=torch.int64, device="cuda")
    out = flat[4096:4096 + n * 3 * 30 * 33].view(n, 3, 30, 33)
    arr = pa.array([d for _, d in mixed], pa.binary())
    short = np.ascontiguousarray(windows[:-1])
    with ctx.lock:
        ctx.check(ctx.lib.ldt_set_windows(ctx.handle, short.ctypes.data, n - 1), "ldt_set_windows")
    with pytest.raises(_lib.LdtError, match=r"rc=-1"):
        T.decode_arrow(arr, np.arange(n), out=out, out_lbl=lbl, size=size)
    torch.cuda.synchronize()
    assert torch.all(flat == SENTINEL).item() and torch.all(lbl == -777).item(), "a refused call wrote its output"
    T.decode_arrow(arr, np.arange(n), out=out, out_lbl=lbl, size=size)  # the failed call consumed them
    assert np.array_equal(out.cpu().numpy(), plain)
    # a call that fails on a row consumes them too
    bad = windows.copy()
    bad[3] = [61, 82, -1, 0]
    _, _, failed = _decode_guarded(mixed, size, bad)
    assert failed == {3: 7}
    assert np.array_equal(T.decode_arrow(arr, size=size)[0].cpu().numpy(), plain)
    # NULL clears pending windows
    with ctx.lock:
        ctx.check(ctx.lib.ldt_set_windows(ctx.handle, short.ctypes.data, n - 1), "ldt_set_windows")
        ctx.check(ctx.lib.ldt_set_windows(ctx.handle, None, 0), "ldt_set_windows")
    assert np.array_equal(T.decode_arrow(arr, size=size)[0].cpu().numpy(), plain)


def test_windowed_batches_take_the_streaming_kernel_under_every_option(mixed):
    from ldt_amd import transforms as T

    ctx, _lib = _ctx()
    arr = pa.array([d for _, d in mixed], pa.binary())
    plain = T.decode_arrow(arr)[0].cpu().numpy()
    before = ctx.lib.ldt_debug_last_resize(ctx.handle)
    assert before > 0  # the band kernel at 224 x 224
    windows = np.array([[224, 224, 0, 0]] * len(mixed), np.int32)
    for impl in (0, 1, 2, 3):
        ctx.set_option(_lib.OPT_RESIZE_IMPL, impl)
        try:
            got = T.decode_arrow(arr, windows=windows)[0].cpu().numpy()
            assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 0
            assert np.array_equal(got, plain)
        finally:
            ctx.set_option(_lib.OPT_RESIZE_IMPL, 0)
    again = T.decode_arrow(arr)[0].cpu().numpy()
    assert ctx.lib.ldt_debug_last_resize(ctx.handle) == before
    assert np.array_equal(again, plain)


def test_normalize_with_windows(mixed):
    size = (30, 33)
    windows = np.array([[61, 82, 31, 49]] * len(mixed), np.int32)
    img, lbl, failed = _decode_guarded(mixed, size, windows, normalize=True)
    assert _check_rows(mixed, size, windows, img, lbl, failed, "normalize", normalize=True) == len(mixed)


# ---- entry points ---------------------------------------------------------------------------------

ENTRY_SIZE = (30, 33)


@pytest.fixture(scope="module")
def entry(mixed):
    import ldt_amd

    sampler = ldt_amd.ResizeCenterCrop(40)
    windows = sampler.sample(_wh(mixed), None, ENTRY_SIZE)
    rb = pa.RecordBatch.from_arrays([pa.array([d for _, d in mixed], pa.binary()),
                                     pa.array(np.arange(100, 100 + len(mixed)), pa.int64())], names=["image", "label"])
    return sampler, windows, rb


def _check_out(mixed, windows, out, what, size=ENTRY_SIZE, crops=None):
    img = out["image"].cpu().numpy() if isinstance(out, dict) or hasattr(out, "keys") else out[0].cpu().numpy()
    lbl = out["label"].cpu().numpy() if isinstance(out, dict) or hasattr(out, "keys") else out[1].cpu().numpy()
    assert img.shape == (len(mixed), 3) + size
    assert _check_rows(mixed, size, windows, img, lbl, {}, what, crops=crops) == len(mixed)


def test_decode_tensor_image_and_collate_fn(mixed, entry):
    import ldt_amd

    sampler, windows, rb = entry
    assert windows[1].tolist() == [40, 53, 5, 10]
    _check_out(mixed, windows, ldt_amd.decode_tensor_image(rb, size=ENTRY_SIZE, window=windows), "decode_tensor_image")
    _check_out(mixed, windows, ldt_amd.decode_tensor_image(rb, size=ENTRY_SIZE, window=sampler), "window=sampler")
    _check_out(mixed, windows, ldt_amd.decode_tensor_image(rb, size=ENTRY_SIZE, window=windows.tolist()), "as lists")
    items = [{"image": d, "label": 100 + k} for k, (_, d) in enumerate(mixed)]
    _check_out(mixed, windows, ldt_amd.collate_fn(items, size=ENTRY_SIZE, window=sampler), "collate_fn")
    _check_out(mixed, windows, ldt_amd.make_collate_fn(size=ENTRY_SIZE, window=sampler)(items), "make_collate_fn")
    _check_out(mixed, windows, ldt_amd.collate_fn(rb, size=ENTRY_SIZE, window=windows), "collate_fn(RecordBatch)")
    with pytest.raises(ValueError):
        ldt_amd.decode_tensor_image(rb, size=ENTRY_SIZE, window=windows[:-1])
    with pytest.raises((TypeError, ValueError)):  # a bare int as the size stays refused
        ldt_amd.decode_tensor_image(rb, size=256)
    # with a RandomResizedCropFlip the sampler sees the boxes' sizes
    import torch

    crops = ldt_amd.RandomResizedCropFlip(generator=torch.Generator().manual_seed(31)).sample(_wh(mixed))
    want = sampler.sample(crops[:, [3, 2]], None, ENTRY_SIZE)
    out = ldt_amd.decode_tensor_image(rb, size=ENTRY_SIZE, window=sampler,
                                      crop=ldt_amd.RandomResizedCropFlip(generator=torch.Generator().manual_seed(31)))
    _check_out(mixed, want, out, "crop sampler + window sampler", crops=crops)


def test_resident_batch_and_pipeline(mixed, entry):
    import torch

    import ldt_amd

    sampler, windows, rb = entry
    res = ldt_amd.ResidentBatch([d for _, d in mixed], np.arange(100, 100 + len(mixed)))
    _check_out(mixed, windows, res.decode(size=ENTRY_SIZE, windows=windows), "ResidentBatch.decode")
    _check_out(mixed, windows, res.decode(size=ENTRY_SIZE, windows=sampler), "ResidentBatch.decode(sampler)")
    # depth 3, five batches with different windows, a bad window in batch 3: check() reports it
    per_batch = [windows.copy(), np.array([[61, 82, 31, 49]] * len(mixed), np.int32),
                 ldt_amd.ResizeCenterCrop(64).sample(_wh(mixed), None, ENTRY_SIZE),
                 np.array([[35, 2000, 5, 1967]] * len(mixed), np.int32), np.array([[30, 33, 0, 0]] * len(mixed), np.int32)]
    per_batch[3][2] = [35, 2000, 6, 1967]  # top + out_h == res_h + 1
    pipe = ldt_amd.DecodePipeline(depth=3, size=ENTRY_SIZE)
    outs = [pipe.decode(res if b % 2 else rb, windows=per_batch[b]) for b in range(5)]
    with pytest.raises(ldt_amd.ImageDecodeError) as e:
        pipe.check()
    assert e.value.rows == {2: 7}
    torch.cuda.synchronize()
    for b, (img, lbl) in enumerate(outs):
        _check_rows(mixed, ENTRY_SIZE, per_batch[b], img.cpu().numpy(), lbl.cpu().numpy(), {2: 7} if b == 3 else {},
                    f"pipeline batch {b}")
    pipe.check()  # nothing left unchecked
    # unwindowed batches of the same pipeline afterwards are the plain result
    plain = ldt_amd.decode_tensor_image(rb, size=ENTRY_SIZE)["image"]
    assert torch.equal(pipe.decode(rb)[0], plain)
    pipe.check()
    # a pipeline-wide sampler
    pipe = ldt_amd.DecodePipeline(depth=3, size=ENTRY_SIZE, window=sampler)
    outs = [pipe.decode(res if b % 2 else rb) for b in range(3)]
    pipe.check()
    for b, out in enumerate(outs):
        _check_out(mixed, windows, out, f"DecodePipeline(window=sampler) batch {b}")


def test_to_tensor_fn_with_an_array_per_call_and_with_a_sampler(mixed, entry):
    import torch

    import ldt_amd

    sampler, windows, rb = entry
    fn = ldt_amd.make_to_tensor_fn(depth=2, size=ENTRY_SIZE)
    other = np.array([[61, 82, 31, 49]] * len(mixed), np.int32)
    a, b = fn(rb, window=windows), fn(rb, window=other)
    plain = fn(rb)
    fn.check()
    _check_out(mixed, windows, a, "to_tensor_fn(window=array)")
    _check_out(mixed, other, b, "to_tensor_fn(window=array), second call")
    assert torch.equal(plain["image"], ldt_amd.decode_tensor_image(rb, size=ENTRY_SIZE)["image"])
    fn = ldt_amd.make_to_tensor_fn(depth=2, size=ENTRY_SIZE, window=sampler)
    first, second = fn(rb), fn(rb)
    fn.check()
    _check_out(mixed, windows, first, "to_tensor_fn(window=sampler)")
    _check_out(mixed, windows, second, "to_tensor_fn(window=sampler), second batch")


def test_device_batch_computes_the_windows_where_it_decodes(mixed, entry):
    from ldt_amd import transforms as T

    sampler, windows, _ = entry
    images = [d for _, d in mixed]
    labels = list(range(100, 100 + len(images)))
    batch = T.DeviceBatch(T._pack_list(images, labels), size=ENTRY_SIZE, window=sampler)
    _check_out(mixed, windows, batch, "DeviceBatch(window=sampler)")
    other = np.array([[61, 82, 31, 49]] * len(mixed), np.int32)
    batch = T.DeviceBatch(T._pack_list(images, labels), size=ENTRY_SIZE, window=other)
    _check_out(mixed, other, batch.pin_memory(), "DeviceBatch(window=array)")


def test_resize_raw_with_windows():
    import torch

    import ldt_amd
    from ldt_amd import synth

    h, w = 301, 517
    raw = np.stack([synth.raw_hwc_one(h, w, 71 + k) for k in range(3)])
    crops = np.array([[1, 3, 290, 501, 0], [0, 1, 301, 516, 1], [150, 255, 2, 3, 1]], np.int32)
    for size, windows in [((30, 33), [[61, 82, 31, 49], [30, 33, 0, 0], [35, 2000, 5, 1967]]),
                          ((299, 299), [[330, 348, 31, 49], [299, 299, 0, 0], [301, 517, 1, 109]])]:
        windows = np.array(windows, np.int32)
        for src in (torch.from_numpy(raw), torch.from_numpy(raw).cuda()):
            for normalize, boxes in ((False, None), (True, crops)):
                out = ldt_amd.resize_raw(src, h, w, normalize=normalize, size=size, windows=windows,
                                         crops=boxes).cpu().numpy()
                assert out.shape == (3, 3) + size
                for k in range(3):
                    t, l, bh, bw, f = crops[k].tolist() if boxes is not None else (0, 0, h, w, 0)
                    exp = _window_of(raw[k, t:t + bh, l:l + bw], size, windows[k], f, normalize=normalize or None)
                    _check(out[k], exp, f"raw window {k} -> {size} crops={boxes is not None}")
    plain = ldt_amd.resize_raw(torch.from_numpy(raw), h, w, size=(30, 33)).cpu().numpy()
    for k in range(3):
        _check(plain[k], oracle.raw_to_tensor(raw[k], 30, 33, normalize=True), "raw after windows")
    # a bad window is an argument error here, and so is a row count that does not match
    good = np.array([[61, 82, 31, 49]] * 3, np.int32)
    for bad in ([0, 82, 0, 0], [61, 65536, 0, 0], [61, 82, -1, 0], [61, 82, 32, 49], [61, 82, 31, 50], [29, 32, 0, 0]):
        wn = good.copy()
        wn[1] = bad
        with pytest.raises(ldt_amd.LdtError):
            ldt_amd.resize_raw(torch.from_numpy(raw), h, w, size=(30, 33), windows=wn)
    with pytest.raises(ValueError):
        ldt_amd.resize_raw(torch.from_numpy(raw), h, w, size=(30, 33), windows=good[:2])
    # the limit is against res: 1221 columns onto 33 is a reduction of exactly 37, 1222 is over it
    wide = np.stack([synth.raw_hwc_one(31, 1222, 81)])
    out = ldt_amd.resize_raw(torch.from_numpy(wide), 31, 1222, size=(30, 33), normalize=False,
                             crops=[[1, 0, 30, 1221, 1]], windows=[[31, 33, 1, 0]]).cpu().numpy()
    _check(out[0], _window_of(wide[0, 1:31, :1221], (30, 33), [31, 33, 1, 0], 1), "raw reduction 37")
    with pytest.raises(ldt_amd.LdtError):
        ldt_amd.resize_raw(torch.from_numpy(wide), 31, 1222, size=(30, 33), windows=[[31, 33, 1, 0]])
    out = ldt_amd.resize_raw(torch.from_numpy(wide), 31, 1222, size=(30, 33), normalize=False,
                             windows=[[31, 34, 0, 1]]).cpu().numpy()
    _check(out[0], _window_of(wide[0], (30, 33), [31, 34, 0, 1], 0), "raw widened res within the limit")
