"""GPU tests of the per-image crop box and flip (ldt_set_crops, ``crops=`` /
``crop=``): every decode / resize entry point against the oracle composition

    raw_to_tensor(decode_rgb(cell)[top:top+bh, left:left+bw], oh, ow), mirrored when flip,

which tests/test_crop.py pins to Pillow's ``crop().resize()`` on the CPU.
Max abs <= 2/255 is asserted first, then bit equality.

One rule (`_expected`) says what every row must be: status 6 for a box that is
empty, has a negative origin, leaves the image or has a flip other than 0 / 1;
status 4 for a box reduced by more than 37 on an axis; a failed row is all
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
    """The mixed batch of tests/test_gpu_output_size.py (without its 512 x 512
    cell, with a 4:1:1 layout cell): (name, data) in a fixed order."""
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


def _expected(name, data, size, crop, normalize=None):
    """The oracle's tensor for the row, or the status it must fail with."""
    top, left, bh, bw, flip = (int(v) for v in crop)
    key = (name, size, (top, left, bh, bw, flip), bool(normalize))
    if key not in _exp_cache:
        h, w = _hw(name, data)
        if top < 0 or left < 0 or bh < 1 or bw < 1 or top + bh > h or left + bw > w or flip not in (0, 1):
            _exp_cache[key] = 6
        elif -(-bw // size[1]) > 37 or -(-bh // size[0]) > 37:
            _exp_cache[key] = 4
        else:
            if name not in _rgb_cache:
                _rgb_cache[name] = oracle.decode_rgb(data)
            t = oracle.raw_to_tensor(_rgb_cache[name][top:top + bh, left:left + bw], size[0], size[1],
                                     normalize=normalize)
            _exp_cache[key] = np.ascontiguousarray(t[:, :, ::-1]) if flip else t
    return _exp_cache[key]


def _ctx():
    import torch

    from ldt_amd import _lib

    return _lib.get_context(torch.cuda.current_device()), _lib


def _decode_guarded(cells, size, crops=None, guard=4096, normalize=None, **kw):
    """decode_arrow into the middle of a larger buffer full of a sentinel.
    Returns (images, labels, {failed row: status}, the whole buffer's tensor);
    asserts the guards are untouched."""
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
                       size=size, normalize=normalize, crops=crops, **kw)
    except ldt_amd.ImageDecodeError as e:
        failed = dict(e.rows)
    finally:
        torch.cuda.synchronize()
        assert torch.all(flat[:guard] == SENTINEL).item(), f"{size}: wrote before the output"
        assert torch.all(flat[guard + n * cell:] == SENTINEL).item(), f"{size}: wrote past the output"
        assert int(lflat[0]) == -777 and int(lflat[n + 1]) == -777
    return out.cpu().numpy(), lflat[1:n + 1].cpu().numpy(), failed


def _check_rows(cells, size, crops, img, lbl, failed, what, normalize=None, other_failed=None, label0=100):
    """Every row against `_expected`; `other_failed`: rows that fail for a
    reason of their own (a corrupt cell), with their status."""
    other_failed = other_failed or {}
    want_failed, exact = {}, 0
    assert len(crops) == len(cells) == len(img)
    for k, (name, data) in enumerate(cells):
        exp = other_failed[k] if k in other_failed else _expected(name, data, size, crops[k], normalize)
        assert exp is not None, f"{what}: row {k} ({name}) has no expected value"
        if isinstance(exp, int):
            want_failed[k] = exp
            assert not img[k].any(), f"{what}: failed row {k} ({name}) is not all zero"
            assert lbl is None or lbl[k] == -100, f"{what}: failed row {k} label {lbl[k]}"
        else:
            _check(img[k], exp, f"{what}: {name} crop {list(crops[k])} -> {size}")
            assert lbl is None or lbl[k] == label0 + k
            exact += 1
    assert failed == want_failed, f"{what}: failed rows {failed}, expected {want_failed}"
    return exact


def _whole(cells, flip=0):
    return np.array([[0, 0, *_hw(n, d), flip] for n, d in cells], np.int32)


def _box(h, w, top, left, bh, bw, flip):
    """The box clamped into an h x w image (a small cell gets a smaller box, never none)."""
    top, left = min(top, h - 1), min(left, w - 1)
    return [top, left, max(1, min(bh, h - top)), max(1, min(bw, w - left)), flip]


def _cases(cells):
    """name -> int32 [n, 5]: the chroma-phase and edge cases, one box per cell
    each; about half the rows are flipped."""
    hw = [_hw(n, d) for n, d in cells]
    f = lambda c, k: (c + k) & 1  # noqa: E731
    cases = {
        "odd-origin": [_box(h, w, 3, 5, h - 6, w - 7, f(0, k)) for k, (h, w) in enumerate(hw)],
        "to-the-end": [_box(h, w, (h // 3) | 1, (w // 3) | 1, h, w, f(1, k)) for k, (h, w) in enumerate(hw)],
        "one-row": [_box(h, w, h // 2, 0, 1, w, f(0, k)) for k, (h, w) in enumerate(hw)],
        "one-column": [_box(h, w, 0, (w // 2) | 1, h, 1, f(1, k)) for k, (h, w) in enumerate(hw)],
        "corner-tl": [[0, 0, 1, 1, f(0, k)] for k, (h, w) in enumerate(hw)],
        "corner-tr": [[0, w - 1, 1, 1, f(1, k)] for k, (h, w) in enumerate(hw)],
        "corner-bl": [[h - 1, 0, 1, 1, f(0, k)] for k, (h, w) in enumerate(hw)],
        "corner-br": [[h - 1, w - 1, 1, 1, f(1, k)] for k, (h, w) in enumerate(hw)],
        "3x2-upscaled": [_box(h, w, (h // 2) | 1, (w // 3) | 1, 2, 3, f(0, k)) for k, (h, w) in enumerate(hw)],
    }
    return {k: np.array(v, np.int32) for k, v in cases.items()}


# ---- identity ---------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=_ID)
def test_whole_image_box_is_the_uncropped_result(mixed, size):
    import torch

    plain, lbl0, failed0 = _decode_guarded(mixed, size)
    same, lbl, failed = _decode_guarded(mixed, size, _whole(mixed, 0))
    assert failed == failed0 and np.array_equal(lbl, lbl0)
    assert np.array_equal(same, plain), "whole-image boxes, flip 0: differs from the call without crops"
    flipped, lbl, failed = _decode_guarded(mixed, size, _whole(mixed, 1))
    assert failed == failed0 and np.array_equal(lbl, lbl0)
    assert np.array_equal(flipped, torch.flip(torch.from_numpy(plain), dims=[-1]).numpy())
    # and both are the oracle's (at (7, 5) the 500 x 375 cell is over the limit: status 4 either way)
    exact = _check_rows(mixed, size, _whole(mixed, 1), flipped, lbl, failed, "whole image flipped")
    assert exact == len(mixed) - len(failed0) and len(failed0) == (1 if size == (7, 5) else 0)


# ---- chroma phase and edges -----------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=_ID)
def test_boxes_on_every_cell(mixed, size):
    ctx, _ = _ctx()
    cases = _cases(mixed)
    assert len(cases) == 9
    flips = np.concatenate([c[:, 4] for c in cases.values()])
    assert 0.4 <= flips.mean() <= 0.6
    for cname, crops in cases.items():
        img, lbl, failed = _decode_guarded(mixed, size, crops)
        exact = _check_rows(mixed, size, crops, img, lbl, failed, cname)
        assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 0
        # only a strip of the 500 x 375 cell can pass the limit, and only at (7, 5)
        assert exact == len(mixed) - len(failed)
        assert set(failed) <= ({1} if size == (7, 5) else set()), (cname, failed)
    # the 500 x 375 cell is large enough for every case as stated: odd origin, a box to its last
    # row and column (not multiples of its 16 x 16 MCU), full-width row, full-height column
    assert cases["odd-origin"][1].tolist() == [3, 5, 369, 493, 1]
    assert cases["to-the-end"][1].tolist() == [125, 167, 250, 333, 0]
    assert cases["one-row"][1, :4].tolist() == [187, 0, 1, 500]
    assert cases["one-column"][1, :4].tolist() == [0, 251, 375, 1]
    assert cases["3x2-upscaled"][1, :4].tolist() == [187, 167, 2, 3]


# ---- the limit is on the box ---------------------------------------------------------------------

def test_reduction_limit_applies_to_the_box(mixed):
    size = (2, 3)
    _, _, failed = _decode_guarded(mixed, size)
    assert failed.get(1) == 4  # the 500 x 375 cell as a whole: ceil(500 / 3) > 37
    crops = np.array([_box(*_hw(n, d), 1, 1, 60, 100, k & 1) for k, (n, d) in enumerate(mixed)], np.int32)
    assert crops[1].tolist() == [1, 1, 60, 100, 1]
    img, lbl, failed = _decode_guarded(mixed, size, crops)
    assert failed == {}
    assert _check_rows(mixed, size, crops, img, lbl, failed, "100x60 boxes at (2, 3)") == len(mixed)
    # a 500 x 1 box at (7, 5): ceil(500 / 5) = 100 > 37 on that row alone
    size = (7, 5)
    crops = _cases(mixed)["odd-origin"]
    crops[1] = [200, 0, 1, 500, 1]
    crops[2] = [0, 0, 100, 150, 0]
    img, lbl, failed = _decode_guarded(mixed, size, crops)
    assert failed == {1: 4}
    assert _check_rows(mixed, size, crops, img, lbl, failed, "500x1 box at (7, 5)") == len(mixed) - 1


# ---- bad boxes -----------------------------------------------------------------------------------

def test_bad_boxes_fail_their_own_rows(mixed):
    size = (30, 33)
    cells = mixed + [("truncated", read_golden("jpeg/bad_truncated.bin"))]
    good = _cases(mixed)["to-the-end"]
    th, tw = _hw(*cells[-1])
    hw = [_hw(n, d) for n, d in mixed]
    bad = {1: [1, 0, hw[1][0], hw[1][1], 0],      # top + height == H + 1
           2: [0, 0, hw[2][0], 0, 1],             # width == 0
           4: [0, -1, 5, 5, 0],                   # a negative left
           6: [0, 0, 4, 4, 2]}                    # flip == 2
    for rows in ([1], [2], [4], [6], [1, 2, 4, 6]):
        crops = np.concatenate([good, [[0, 0, th, tw, 1]]]).astype(np.int32)
        for r in rows:
            crops[r] = bad[r]
        img, lbl, failed = _decode_guarded(cells, size, crops)
        assert failed == {**{r: 6 for r in rows}, 8: 3}, (rows, failed)
        assert _check_rows(cells, size, crops, img, lbl, failed, f"bad boxes {rows}", other_failed={8: 3}) == 8 - len(rows)


# ---- one-shot crops ---------------------------------------------------------------------------------

def test_crops_apply_to_one_call(mixed):
    import torch

    from ldt_amd import transforms as T

    ctx, _lib = _ctx()
    size = (30, 33)
    plain, _, _ = _decode_guarded(mixed, size)
    crops = _cases(mixed)["odd-origin"]
    img, lbl, failed = _decode_guarded(mixed, size, crops)
    _check_rows(mixed, size, crops, img, lbl, failed, "first call")
    again, _, _ = _decode_guarded(mixed, size)
    assert np.array_equal(again, plain), "crops outlived their call"
    # crops for the wrong number of rows: LDT_ERR_ARG, nothing enqueued, and they are consumed
    n = len(mixed)
    flat = torch.full((4096 + n * 3 * 30 * 33 + 4096,), SENTINEL, dtype=torch.float32, device="cuda")
    lbl = torch.full((n,), -777, dtype=torch.int64, device="cuda")
    out = flat[4096:4096 + n * 3 * 30 * 33].view(n, 3, 30, 33)
    arr = pa.array([d for _, d in mixed], pa.binary())
    short = np.ascontiguousarray(crops[:-1])
    with ctx.lock:
        ctx.check(ctx.lib.ldt_set_crops(ctx.handle, short.ctypes.data, n - 1), "ldt_set_crops")
    with pytest.raises(_lib.LdtError, match=r"rc=-1"):
        T.decode_arrow(arr, np.arange(n), out=out, out_lbl=lbl, size=size)
    torch.cuda.synchronize()
    assert torch.all(flat == SENTINEL).item() and torch.all(lbl == -777).item(), "a refused call wrote its output"
    T.decode_arrow(arr, np.arange(n), out=out, out_lbl=lbl, size=size)
    assert np.array_equal(out.cpu().numpy(), plain)
    # NULL clears pending crops
    with ctx.lock:
        ctx.check(ctx.lib.ldt_set_crops(ctx.handle, short.ctypes.data, n - 1), "ldt_set_crops")
        ctx.check(ctx.lib.ldt_set_crops(ctx.handle, None, 0), "ldt_set_crops")
    assert np.array_equal(T.decode_arrow(arr, size=size)[0].cpu().numpy(), plain)


def test_routing_is_unchanged_without_crops(mixed):
    from ldt_amd import transforms as T

    ctx, _lib = _ctx()
    arr = pa.array([d for _, d in mixed], pa.binary())
    plain = T.decode_arrow(arr)[0].cpu().numpy()
    before = ctx.lib.ldt_debug_last_resize(ctx.handle)
    assert before > 0  # the band kernel at 224 x 224
    for impl in (0, 1, 3):  # cropped batches take the streaming kernel whatever the option says
        ctx.set_option(_lib.OPT_RESIZE_IMPL, impl)
        try:
            T.decode_arrow(arr, crops=_whole(mixed))
            assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 0
        finally:
            ctx.set_option(_lib.OPT_RESIZE_IMPL, 0)
    again = T.decode_arrow(arr)[0].cpu().numpy()
    assert ctx.lib.ldt_debug_last_resize(ctx.handle) == before
    assert np.array_equal(again, plain)


def test_normalize_with_crops(mixed):
    size = (30, 33)
    crops = _cases(mixed)["to-the-end"]
    img, lbl, failed = _decode_guarded(mixed, size, crops, normalize=True)
    assert _check_rows(mixed, size, crops, img, lbl, failed, "normalize", normalize=True) == len(mixed)


# ---- entry points ---------------------------------------------------------------------------------

ENTRY_SIZE = (30, 33)


@pytest.fixture(scope="module")
def entry(mixed):
    crops = _cases(mixed)["odd-origin"]
    rb = pa.RecordBatch.from_arrays([pa.array([d for _, d in mixed], pa.binary()),
                                     pa.array(np.arange(100, 100 + len(mixed)), pa.int64())], names=["image", "label"])
    return crops, rb


def _check_out(mixed, crops, out, what, size=ENTRY_SIZE):
    img = out["image"].cpu().numpy() if isinstance(out, dict) or hasattr(out, "keys") else out[0].cpu().numpy()
    lbl = out["label"].cpu().numpy() if isinstance(out, dict) or hasattr(out, "keys") else out[1].cpu().numpy()
    assert img.shape == (len(mixed), 3) + size
    assert _check_rows(mixed, size, crops, img, lbl, {}, what) == len(mixed)


def test_decode_tensor_image_and_collate_fn(mixed, entry):
    import ldt_amd

    crops, rb = entry
    _check_out(mixed, crops, ldt_amd.decode_tensor_image(rb, size=ENTRY_SIZE, crop=crops), "decode_tensor_image")
    _check_out(mixed, crops, ldt_amd.decode_tensor_image(rb, size=ENTRY_SIZE, crop=crops.tolist()), "crop as lists")
    items = [{"image": d, "label": 100 + k} for k, (_, d) in enumerate(mixed)]
    _check_out(mixed, crops, ldt_amd.collate_fn(items, size=ENTRY_SIZE, crop=crops), "collate_fn")
    _check_out(mixed, crops, ldt_amd.make_collate_fn(size=ENTRY_SIZE, crop=crops)(items), "make_collate_fn")
    _check_out(mixed, crops, ldt_amd.collate_fn(rb, size=ENTRY_SIZE, crop=crops), "collate_fn(RecordBatch)")
    with pytest.raises(ValueError):
        ldt_amd.decode_tensor_image(rb, size=ENTRY_SIZE, crop=crops[:-1])


def test_resident_batch_and_pipeline(mixed, entry):
    import torch

    import ldt_amd

    crops, rb = entry
    res = ldt_amd.ResidentBatch([d for _, d in mixed], np.arange(100, 100 + len(mixed)))
    _check_out(mixed, crops, res.decode(size=ENTRY_SIZE, crops=crops), "ResidentBatch.decode")
    # depth 2, five batches with different crops, a bad box in batch 3: check() reports it
    names = ["odd-origin", "to-the-end", "one-row", "3x2-upscaled", "corner-br"]
    per_batch = [_cases(mixed)[k].copy() for k in names]
    per_batch[3][2] = [0, 0, 101, 150, 0]  # top + height == H + 1 on the 100 x 150 cell
    pipe = ldt_amd.DecodePipeline(depth=2, size=ENTRY_SIZE)
    outs = [pipe.decode(res if b % 2 else rb, crops=per_batch[b]) for b in range(5)]
    with pytest.raises(ldt_amd.ImageDecodeError) as e:
        pipe.check()
    assert e.value.rows == {2: 6}
    torch.cuda.synchronize()
    for b, (img, lbl) in enumerate(outs):
        _check_rows(mixed, ENTRY_SIZE, per_batch[b], img.cpu().numpy(), lbl.cpu().numpy(), {2: 6} if b == 3 else {},
                    f"pipeline batch {b}")
    pipe.check()  # nothing left unchecked
    # uncropped batches of the same pipeline afterwards are the plain result
    plain = ldt_amd.decode_tensor_image(rb, size=ENTRY_SIZE)["image"]
    assert torch.equal(pipe.decode(rb)[0], plain)
    pipe.check()


def test_to_tensor_fn_with_an_array_per_call_and_with_a_sampler(mixed, entry):
    import torch

    import ldt_amd

    crops, rb = entry
    fn = ldt_amd.make_to_tensor_fn(depth=2, size=ENTRY_SIZE)
    other = _cases(mixed)["to-the-end"]
    a, b = fn(rb, crop=crops), fn(rb, crop=other)
    plain = fn(rb)
    fn.check()
    _check_out(mixed, crops, a, "to_tensor_fn(crop=array)")
    _check_out(mixed, other, b, "to_tensor_fn(crop=array), second call")
    assert torch.equal(plain["image"], ldt_amd.decode_tensor_image(rb, size=ENTRY_SIZE)["image"])
    # a sampler: the boxes the same seed draws here from the same sizes
    wh, st = ldt_amd.image_sizes(rb.column(0))
    assert not st.any() and wh.tolist() == [[w, h] for h, w in (_hw(n, d) for n, d in mixed)]
    want = [ldt_amd.RandomResizedCropFlip(generator=torch.Generator().manual_seed(9)).sample(wh)]
    g = torch.Generator().manual_seed(9)
    fn = ldt_amd.make_to_tensor_fn(depth=2, size=ENTRY_SIZE, crop=ldt_amd.RandomResizedCropFlip(generator=g))
    first = fn(rb)
    second = fn(rb)  # the generator has moved on
    fn.check()
    _check_out(mixed, want[0], first, "to_tensor_fn(crop=sampler)")
    g2 = torch.Generator().manual_seed(9)
    s2 = ldt_amd.RandomResizedCropFlip(generator=g2)
    s2.sample(wh)
    _check_out(mixed, s2.sample(wh), second, "to_tensor_fn(crop=sampler), second batch")


def test_resize_raw_with_crops():
    import torch

    import ldt_amd
    from ldt_amd import synth

    h, w = 33, 47
    raw = np.stack([synth.raw_hwc_one(h, w, 61 + k) for k in range(5)])
    crops = np.array([[1, 3, 30, 41, 0], [0, 1, 33, 46, 1], [32, 45, 1, 1, 0], [5, 7, 2, 3, 1], [0, 0, 33, 47, 1]],
                     np.int32)
    for size in [(30, 33), (299, 299)]:
        for src in (torch.from_numpy(raw), torch.from_numpy(raw).cuda()):
            for normalize in (False, True):
                out = ldt_amd.resize_raw(src, h, w, normalize=normalize, size=size, crops=crops).cpu().numpy()
                assert out.shape == (5, 3) + size
                for k, (t, l, bh, bw, f) in enumerate(crops.tolist()):
                    exp = oracle.raw_to_tensor(raw[k, t:t + bh, l:l + bw], size[0], size[1], normalize=normalize or None)
                    _check(out[k], exp[:, :, ::-1] if f else exp, f"raw crop {k} -> {size} normalize={normalize}")
    plain = ldt_amd.resize_raw(torch.from_numpy(raw), h, w, size=(30, 33)).cpu().numpy()
    for k in range(5):
        _check(plain[k], oracle.raw_to_tensor(raw[k], 30, 33, normalize=True), "raw after crops")
    # a bad box is an argument error here, and the limit is on the box
    for bad in ([0, 0, 34, 47, 0], [0, 0, 33, 0, 0], [0, -1, 3, 3, 0], [0, 0, 3, 3, 2]):
        c = crops.copy()
        c[3] = bad
        with pytest.raises(ldt_amd.LdtError):
            ldt_amd.resize_raw(torch.from_numpy(raw), h, w, size=(30, 33), crops=c)
    wide = torch.zeros((1, 16, 4000, 3), dtype=torch.uint8)
    with pytest.raises(ldt_amd.LdtError):
        ldt_amd.resize_raw(wide, 16, 4000, size=(64, 64), crops=[[0, 0, 16, 4000, 0]])
    out = ldt_amd.resize_raw(wide, 16, 4000, size=(64, 64), crops=[[0, 1001, 16, 2000, 0]], normalize=False)
    assert not out.cpu().numpy().any()


def test_device_batch_samples_where_it_decodes(mixed):
    import torch

    import ldt_amd
    from ldt_amd import transforms as T

    images = [d for _, d in mixed]
    wh, _ = ldt_amd.image_sizes(images)
    want = ldt_amd.RandomResizedCropFlip(generator=torch.Generator().manual_seed(21)).sample(wh)
    sampler = ldt_amd.RandomResizedCropFlip(generator=torch.Generator().manual_seed(21))
    batch = T.DeviceBatch(T._pack_list(images, list(range(100, 100 + len(images)))), size=ENTRY_SIZE, crop=sampler)
    _check_out(mixed, want, batch, "DeviceBatch(crop=sampler)")
    # an array travels with the batch too
    crops = _cases(mixed)["one-column"]
    batch = T.DeviceBatch(T._pack_list(images, list(range(100, 100 + len(images)))), size=ENTRY_SIZE, crop=crops)
    _check_out(mixed, crops, batch.pin_memory(), "DeviceBatch(crop=array)")
