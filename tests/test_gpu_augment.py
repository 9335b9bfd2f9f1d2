"""GPU tests of ``augment=`` / ``augments=`` (ldt_set_augments): the op set of
TrivialAugmentWide / RandAugment and RandomErasing per output image, fused
behind the resize.

The expected value of every output image is computed on the host and compared
bit for bit in the call's dtype:

  1. the oracle's Pillow-exact resized bytes of that row and view, obtained as
     tests/test_gpu_color.py obtains them (its cache is shared);
  2. Pillow's own ops in the entry's order: ``Image.transform(AFFINE,
     NEAREST, fillcolor)``, ``ImageEnhance.Brightness`` / ``Color`` /
     ``Contrast`` / ``Sharpness``, ``ImageOps.posterize`` / ``solarize`` /
     ``autocontrast`` / ``equalize`` / ``invert``;
  3. the ToTensor / Normalize table (the oracle's identity resize), converted
     by torch to the call's dtype, then zeros inside the erase box.

A failed row is all-zero bytes with label -100. Every decode goes into the
middle of a buffer full of a sentinel, and the bytes around the output are
checked after it.
"""
import numpy as np
import pyarrow as pa
import pytest

import test_gpu_color as C
from conftest import read_golden
from oracle import oracle

pytestmark = pytest.mark.gpu

NAN = float("nan")
ABSENT = [NAN] * 10


@pytest.fixture(scope="module")
def cells():
    return [(name, read_golden("jpeg/" + name)) for name in C.NAMES]


def _row(op, *p, fill=(0, 0, 0)):
    return [float(op)] + [float(x) for x in p] + [NAN] * (6 - len(p)) + [float(x) for x in fill]


def _affine(name, magnitude, hw, fill=(0, 0, 0)):
    from ldt_amd import affine_matrix

    return _row(1, *affine_matrix(name, magnitude, hw), fill=fill)


def _pil_rows(u8, rows):
    """Step 2 on an [h, w, 3] uint8 image with rows of check_augments, by Pillow itself."""
    from PIL import Image, ImageEnhance, ImageOps

    im = Image.fromarray(u8, "RGB")
    enh = {2: ImageEnhance.Brightness, 3: ImageEnhance.Color, 4: ImageEnhance.Contrast, 5: ImageEnhance.Sharpness}
    for row in rows:
        if np.isnan(row[0]) or row[0] == 0:
            continue
        op, p = int(row[0]), [float(x) for x in row[1:7]]
        if op == 1:
            im = im.transform(im.size, Image.AFFINE, p, Image.NEAREST, fillcolor=tuple(int(x) for x in row[7:10]))
        elif op in enh:
            im = enh[op](im).enhance(p[0])
        elif op == 6:
            im = ImageOps.posterize(im, int(p[0])) if int(p[0]) else Image.new("RGB", im.size)
        elif op == 7:
            im = ImageOps.solarize(im, p[0])
        elif op == 8:
            im = ImageOps.autocontrast(im)
        elif op == 9:
            im = ImageOps.equalize(im)
        elif op == 10:
            im = ImageOps.invert(im)
    return np.asarray(im, dtype=np.uint8)


def _expected(u8, rows, box, dtype="float32", normalize=None):
    """Step 3: a CPU tensor [3, h, w] of the call's dtype."""
    import torch

    out = _pil_rows(u8, rows) if rows is not None else u8
    if dtype == "uint8":
        t = torch.from_numpy(np.ascontiguousarray(out.transpose(2, 0, 1))).clone()
    else:
        t = oracle.raw_to_tensor(np.ascontiguousarray(out), out.shape[0], out.shape[1], normalize=normalize)
        t = torch.from_numpy(np.array(t)).to(C._td(dtype))
    if box is not None and box[2]:
        t[:, box[0]:box[0] + box[2], box[1]:box[1] + box[3]] = 0
    return t


def _decode(cells, size, augments, erase=None, views=None, crops=None, windows=None, dtype="float32",
            mf="contiguous", normalize=None, interpolation=None, ctx=None):
    """decode_arrow into the middle of a sentinel buffer, as tests/test_gpu_color.py's _decode."""
    import torch

    import ldt_amd
    from ldt_amd import _lib
    from ldt_amd import transforms as T

    n = len(cells)
    sized = isinstance(size[0], (tuple, list))
    sizes = list(size) if sized else [size] * (views or 1)
    nbytes = sum(n * 3 * h * w for h, w in sizes) * C.ES[dtype]
    buf = torch.full((C.GUARD + nbytes + C.GUARD,), C.SENTINEL, dtype=torch.uint8, device="cuda")
    flat = buf[C.GUARD:C.GUARD + nbytes].view(C._td(dtype))
    cl = mf == "channels_last"
    if sized:
        out = flat
    elif views is None:
        out = flat.view(n, size[0], size[1], 3).permute(0, 3, 1, 2) if cl else flat.view(n, 3, *size)
    else:
        out = flat.view(views, n, size[0], size[1], 3).permute(0, 1, 4, 2, 3) if cl else flat.view(views, n, 3, *size)
    lflat = torch.full((n + 2,), -777, dtype=torch.int64, device="cuda")
    labels = np.arange(100, 100 + n, dtype=np.int64)
    failed = {}
    lsize = [tuple(s) for s in size] if sized else size
    if augments is not None or erase is not None:
        augments = _lib.check_augments(augments, n, len(size) if sized else views, lsize, erase)
    try:
        T.decode_arrow(pa.array([d for _, d in cells], pa.binary()), labels, out=out, out_lbl=lflat[1:n + 1],
                       size=lsize, normalize=normalize, crops=crops, windows=windows, views=None if sized else views,
                       augments=augments, dtype=C._td(dtype), memory_format=torch.channels_last if cl else None,
                       interpolation=interpolation, ctx=ctx)
    except ldt_amd.ImageDecodeError as e:
        failed = dict(e.rows)
    finally:
        torch.cuda.synchronize()
        assert torch.all(buf[:C.GUARD] == C.SENTINEL).item(), "wrote before the output"
        assert torch.all(buf[C.GUARD + nbytes:] == C.SENTINEL).item(), "wrote past the output"
        assert int(lflat[0]) == -777 and int(lflat[n + 1]) == -777
    res, at, host = [], 0, flat.cpu()
    for h, w in sizes:
        blk = host[at:at + n * 3 * h * w]
        res.append(blk.view(n, h, w, 3).permute(0, 3, 1, 2) if cl else blk.view(n, 3, h, w))
        at += n * 3 * h * w
    return res, lflat[1:n + 1].cpu().numpy(), failed


def _check(cells, size, augments, res, lbl, failed, what, erase=None, views=None, crops=None, windows=None,
           dtype="float32", normalize=None, interp="bilinear", bad=()):
    """Every output image (v, i) against the host's expected value. `augments`: [n, (V,) K, 10] or None."""
    import torch

    n = len(cells)
    sized = isinstance(size[0], (tuple, list))
    V = len(size) if sized else (views or 1)
    multi = sized or views is not None
    if augments is not None:
        augments = np.asarray(augments, np.float64)
        augments = augments.reshape(n, V, augments.shape[-2], 10)
    erase = None if erase is None else np.asarray(erase).reshape(n, V, 4)
    assert sorted(failed) == sorted(bad), (what, failed)
    for i, (name, data) in enumerate(cells):
        for v in range(V):
            sz = tuple(size[v]) if sized else tuple(size)
            got = res[v][i]
            if i in bad:
                assert int(lbl[i]) == -100, (what, i)
                assert not got.contiguous().view(torch.uint8).any().item(), f"{what}: failed row {i} is not zero"
                continue
            crop = None if crops is None else (np.asarray(crops)[i, v] if multi else np.asarray(crops)[i])
            win = None if windows is None else (np.asarray(windows)[i, v] if multi else np.asarray(windows)[i])
            u8 = C._resized_u8(name, data, sz, crop, win, interp)
            want = _expected(u8, None if augments is None else augments[i, v], None if erase is None else erase[i, v],
                             dtype, C._norm_arg(normalize))
            C._same(got, want, f"{what}: {name} view {v}")
            assert int(lbl[i]) == 100 + i


def _each_op(hw):
    """One row per op: the views of test_each_op_alone."""
    return [_affine("Rotate", 31.0, hw, (9, 8, 7)), _affine("ShearX", -0.66, hw),
            _affine("ShearY", 0.3, hw, (255,) * 3),
            _affine("TranslateX", -7.0, hw), _affine("TranslateY", 3.0, hw, (1, 2, 3)), _affine("Rotate", 180.0, hw),
            _row(2, 1.45), _row(3, 0.2), _row(4, 1.8), _row(5, 1.99), _row(5, 0.01), _row(6, 3), _row(7, 100.5),
            _row(8), _row(9), _row(10)]


def _random_rows(n, V, K, hw, seed):
    """Up to K random ops per output image (absent ones in between), every op code."""
    rng = np.random.default_rng(seed)
    out = np.full((n, V, K, 10), NAN, np.float64)
    for i in range(n):
        for v in range(V):
            for k in range(K):
                op = int(rng.integers(0, 11))
                if op == 1:
                    name = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")[int(rng.integers(5))]
                    mag = rng.uniform(-0.9, 0.9) if name[0] == "S" else rng.uniform(-20, 20) if name[0] == "T" \
                        else rng.uniform(-135, 135)
                    out[i, v, k] = _affine(name, mag, hw, tuple(int(x) for x in rng.integers(0, 256, 3)))
                elif op in (2, 3, 4, 5):
                    out[i, v, k] = _row(op, rng.uniform(0.01, 1.99))
                elif op == 6:
                    out[i, v, k] = _row(6, int(rng.integers(0, 9)))
                elif op == 7:
                    out[i, v, k] = _row(7, rng.uniform(0, 256))
                elif op:
                    out[i, v, k] = _row(op)
    return out


def _small_crops(cells, size):
    """Boxes (with a flip) that keep a tiny output inside the reduction limit of 37."""
    crops = np.zeros((len(cells), 5), np.int32)
    for i, (name, data) in enumerate(cells):
        w, h, _ = oracle.jpeg_info(data)
        crops[i] = (3, 5, min(h - 3, 30 * size[0]), min(w - 5, 30 * size[1]), i & 1)
    return crops


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (96, 96), (129, 257), (224, 224)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_each_op_alone(cells, size):
    """One view per op. 3 x 5 and 129 x 257: rows that are no multiple of 4 bytes; 224 x 224: 14 row tiles."""
    use = cells if size[0] < 96 else cells[:2]
    rows = _each_op(size)
    V, n = len(rows), len(use)
    aug = np.broadcast_to(np.array(rows, np.float64)[None, :, None, :], (n, V, 1, 10)).copy()
    crops = None
    if size[0] < 96:
        crops = np.repeat(_small_crops(use, size)[:, None, :], V, axis=1)
    res, lbl, failed = _decode(use, size, aug, views=V, crops=crops)
    _check(use, size, aug, res, lbl, failed, f"each op {size}", views=V, crops=crops)
    if size[0] >= 96:
        plain, _, _ = _decode(use, size, None, views=V)
        assert all((res[v] != plain[v]).any().item() for v in range(V)), "an op changed nothing"


def test_chains_cross_the_stats_boundary(cells):
    hw = (61, 47)
    rot, shear = _affine("Rotate", 31.5, hw, (9, 8, 7)), _affine("ShearX", -0.3, hw)
    chains = [[rot, _row(9), ABSENT, ABSENT], [_row(4, 1.7), _row(8), ABSENT, ABSENT],
              [_row(5, 1.9), shear, ABSENT, ABSENT], [_row(9), _row(9), ABSENT, ABSENT],
              [_row(4, 0.3), rot, _row(9), _row(5, 0.2)], [_row(8), _row(3, 1.8), _row(6, 3), _row(4, 1.2)],
              [_row(2, 1.6), ABSENT, _row(7, 100.5), _row(10)], [_row(9), _row(4, 1.9), _row(8), _row(9)]]
    V, n = len(chains), len(cells)
    aug = np.broadcast_to(np.array(chains, np.float64)[None], (n, V, 4, 10)).copy()
    res, lbl, failed = _decode(cells, hw, aug, views=V)
    _check(cells, hw, aug, res, lbl, failed, "chains", views=V)


def test_slot_alignment_counts_0_1_2_4(cells):
    """One batch, no views, whose entries have 0, 1, 2, 4 and 3 ops: each entry's last op lands in the last slot."""
    hw = (40, 36)
    aug = np.full((len(cells), 4, 10), NAN, np.float64)
    aug[1, 2] = _row(9)
    aug[2, 0], aug[2, 3] = _row(4, 1.6), _affine("Rotate", -20.0, hw)
    aug[3] = [_row(5, 1.7), _row(8), _affine("ShearY", 0.4, hw, (7, 7, 7)), _row(9)]
    aug[4, 1:] = [_row(10), _row(4, 0.4), _row(6, 2)]
    res, lbl, failed = _decode(cells, hw, aug)
    _check(cells, hw, aug, res, lbl, failed, "slot alignment")
    plain, _, _ = _decode(cells, hw, None)
    assert (res[0][0] == plain[0][0]).all().item()  # no ops: the plain table store


def test_uniform_image():
    """Every pixel in one bin: the histogram's adds all meet there."""
    import io

    from PIL import Image

    buf = io.BytesIO()
    Image.new("RGB", (256, 256), (200, 30, 90)).save(buf, "JPEG", quality=90)
    flat = [("uniform_200_30_90", buf.getvalue())]
    hw = (224, 224)
    rows = [[_row(9)], [_row(8)], [_row(4, 1.5)], [_row(5, 1.9)]]
    aug = np.array(rows, np.float64)[None]
    res, lbl, failed = _decode(flat, hw, aug, views=4)
    _check(flat, hw, aug, res, lbl, failed, "uniform", views=4)


def test_two_views_and_a_size_list(cells):
    two = cells[:2]
    aug = _random_rows(2, 2, 3, (48, 40), 11)
    res, lbl, failed = _decode(two, (48, 40), aug, views=2)
    _check(two, (48, 40), aug, res, lbl, failed, "views=2", views=2)
    sizes = [(224, 224), (96, 96)]
    aug = np.full((2, 2, 2, 10), NAN, np.float64)
    for i in range(2):
        for v, hw in enumerate(sizes):
            aug[i, v] = [_affine("TranslateX", 150.0 / 331.0 * hw[1] * 0.3, hw), _row(9) if i else _row(4, 1.3)]
    erase = np.array([[[10, 20, 100, 50], [0, 0, 0, 0]], [[0, 0, 0, 0], [90, 3, 6, 93]]])
    res, lbl, failed = _decode(two, sizes, aug, erase=erase)
    _check(two, sizes, aug, res, lbl, failed, "size list", erase=erase)
    with pytest.raises(ValueError):
        _decode(two, sizes, aug[:, 0])  # a 3-D array in a call with views


@pytest.mark.parametrize("mf", ["contiguous", "channels_last"])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16", "uint8"])
def test_dtypes_and_layouts(cells, dtype, mf):
    """Every dtype in both layouts, with and without Normalize, with an erase box in every other image."""
    size = (30, 41) if mf == "channels_last" else (28, 36)
    n = len(cells)
    aug = _random_rows(n, 2, 2, size, 77)
    erase = np.zeros((n, 2, 4), np.int64)
    erase[::2, 0], erase[1::2, 1] = (5, 7, 11, 13), (0, 30, 28, 6)
    for normalize in ((None,) if dtype == "uint8" else (None, True)):
        res, lbl, failed = _decode(cells, size, aug, erase=erase, views=2, dtype=dtype, mf=mf, normalize=normalize)
        _check(cells, size, aug, res, lbl, failed, f"{dtype} {mf}", erase=erase, views=2, dtype=dtype,
               normalize=normalize)


def test_crop_flip_and_bicubic_window(cells):
    """Progressive and grey sources among them."""
    n, size = len(cells), (32, 40)
    crops = _small_crops(cells, (8, 8))
    aug = _random_rows(n, 1, 2, size, 5)[:, 0]
    res, lbl, failed = _decode(cells, size, aug, crops=crops)
    _check(cells, size, aug, res, lbl, failed, "crop + flip", crops=crops)
    windows = np.array([[48, 56, 9, 7]] * n, np.int32)
    res, lbl, failed = _decode(cells, size, aug, windows=windows, interpolation="bicubic")
    _check(cells, size, aug, res, lbl, failed, "bicubic window", windows=windows, interp="bicubic")


def test_erase_boxes(cells):
    """Inside, at each edge, the whole image and absent; with an op and without."""
    two, hw = cells[:2], (33, 50)
    boxes = [(5, 6, 7, 9), (0, 10, 4, 20), (29, 10, 4, 20), (8, 0, 10, 3), (8, 47, 10, 3), (0, 0, 33, 50),
             (0, 0, 0, 0), (32, 49, 1, 1)]
    V = len(boxes)
    erase = np.broadcast_to(np.array(boxes)[None], (2, V, 4)).copy()
    aug = np.full((2, V, 1, 10), NAN, np.float64)
    aug[1, :, 0] = _row(9)
    res, lbl, failed = _decode(two, hw, aug, erase=erase, views=V, normalize=True)
    _check(two, hw, aug, res, lbl, failed, "erase", erase=erase, views=V, normalize=True)
    res, lbl, failed = _decode(two, hw, None, erase=erase, views=V, dtype="bfloat16", mf="channels_last",
                               normalize=True)
    _check(two, hw, None, res, lbl, failed, "erase only", erase=erase, views=V, dtype="bfloat16", normalize=True)
    with pytest.raises(ValueError):
        _decode(two, hw, None, erase=np.array([[30, 0, 4, 5]] * 2))  # leaves the image


def test_failed_row_between_good_ones(cells):
    mixed = [cells[0], ("bad", read_golden("jpeg/bad_not_jpeg.bin")), cells[1], cells[3]]
    hw = (36, 44)
    aug = np.broadcast_to(np.array([[_row(4, 1.6), _row(9)], [_affine("Rotate", 40.0, hw), _row(8)]])[None],
                          (4, 2, 2, 10)).copy()
    erase = np.broadcast_to(np.array([[3, 3, 9, 9], [0, 0, 0, 0]])[None], (4, 2, 4)).copy()
    res, lbl, failed = _decode(mixed, hw, aug, erase=erase, views=2)
    assert failed == {1: 1}
    _check(mixed, hw, aug, res, lbl, failed, "failed row", erase=erase, views=2, bad=(1,))
    res, lbl, failed = _decode(mixed, hw, aug[:, 0], dtype="bfloat16", mf="channels_last")
    _check(mixed, hw, aug[:, 0], res, lbl, failed, "failed row bf16", dtype="bfloat16", bad=(1,))


def test_samplers_end_to_end(cells):
    """A seeded TrivialAugmentWide + RandomErasing through make_collate_fn and a RandAugment through
    DecodePipeline: the sampler's rows, drawn again from the same seed, through Pillow."""
    import torch

    import ldt_amd
    from ldt_amd import augment as A

    n, size = len(cells), (48, 40)

    def rows_of(sampler, seed):
        """The float rows and boxes the sampler draws for this batch (what sample() hands to check_augments)."""
        g = torch.Generator()
        g.manual_seed(seed)
        sampler.generator = g
        if sampler.erase is not None:
            sampler.erase.generator = g
        rows, boxes = [], []
        for _ in range(n):
            rows.append(sampler._draw(*size))
            boxes.append(sampler.erase._box(*size) if sampler.erase is not None else (0, 0, 0, 0))
        g.manual_seed(seed)
        return np.array(rows, np.float64), np.array(boxes)

    ta = A.TrivialAugmentWide(fill=(3, 2, 1), erase=A.RandomErasing(p=0.7))
    rows, boxes = rows_of(ta, 2024)
    assert (boxes[:, 2] > 0).any()
    fn = ldt_amd.make_collate_fn(device="cuda:0", size=size, normalize=True, augment=ta,
                                 dtype=torch.bfloat16, memory_format=torch.channels_last)
    out = fn([{"image": d, "label": 100 + i} for i, (_, d) in enumerate(cells)])
    _check(cells, size, rows, [out["image"].cpu()], out["label"].cpu().numpy(), {}, "collate", erase=boxes,
           dtype="bfloat16", normalize=True)

    ra = A.RandAugment(num_ops=2, magnitude=9)
    rows, boxes = rows_of(ra, 77)
    rb = pa.RecordBatch.from_arrays([pa.array([d for _, d in cells], pa.binary()),
                                     pa.array(np.arange(100, 100 + n), pa.int64())], names=["image", "label"])
    pipe = ldt_amd.DecodePipeline(depth=2, device="cuda:0", size=size, augment=ra)
    img, lbl = pipe.decode(rb)
    plain, _ = pipe.decode(rb, augments=np.full((n, 1, 10), NAN))  # this batch's own: no ops
    pipe.check()
    torch.cuda.synchronize()
    _check(cells, size, rows, [img.cpu()], lbl.cpu().numpy(), {}, "pipeline")
    _check(cells, size, None, [plain.cpu()], lbl.cpu().numpy(), {}, "pipeline, no ops")
    with pytest.raises(ValueError):
        ldt_amd.DecodePipeline(depth=2, device="cuda:0", size=size, augment=ra, color=ldt_amd.ColorJitterParams())
    # a DeviceBatch carries the checked records, or the sampler, to where it is decoded
    from ldt_amd import transforms as T

    packed = T._pack_list([d for _, d in cells], list(range(100, 100 + n)))
    db = T.DeviceBatch(packed, "cuda:0", None, size=size, augment=rows, dtype=torch.float16)
    _check(cells, size, rows, [db["image"].cpu()], db["label"].cpu().numpy(), {}, "device batch", dtype="float16")
    rows, boxes = rows_of(ta, 9)
    db = T.DeviceBatch(T._pack_list([d for _, d in cells], list(range(100, 100 + n))), "cuda:0", None, size=size,
                       augment=ta)
    _check(cells, size, rows, [db["image"].cpu()], db["label"].cpu().numpy(), {}, "device batch sampler", erase=boxes)
    with pytest.raises(ValueError):
        T.DeviceBatch(packed, "cuda:0", None, size=size, augment=rows[:-1])
    # make_to_tensor_fn: the function's sampler, then a call's own array in its place
    rows, boxes = rows_of(ra, 5)
    fn = ldt_amd.make_to_tensor_fn(depth=2, device="cuda:0", size=size, augment=ra)
    out = fn(rb)
    own = fn(rb, augment=np.full((n, 1, 10), NAN))
    fn.check()
    torch.cuda.synchronize()
    _check(cells, size, rows, [out["image"].cpu()], out["label"].cpu().numpy(), {}, "to_tensor_fn")
    _check(cells, size, None, [own["image"].cpu()], own["label"].cpu().numpy(), {}, "to_tensor_fn, own")
