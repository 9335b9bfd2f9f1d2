"""GPU tests of the blur column of ``color=`` / ``colors=``: Pillow's
``ImageFilter.GaussianBlur(radius)`` between the grayscale and the solarize,
fused behind the resize (k_color_blur).

The method is tests/test_gpu_color.py's, whose helpers and cache of resized
bytes are shared: the oracle's Pillow-exact resized bytes of every row and
view, then Pillow's own chain with ``.filter(ImageFilter.GaussianBlur(radius))``
between ``convert("L")`` and ``ImageOps.solarize``, then the ToTensor /
Normalize table, compared bit for bit in the call's dtype. Every decode goes
into the middle of a sentinel buffer whose guards are checked.

The kernel's tile is 32 rows by 64 columns (``TH``, ``TW``): the shapes are one
pixel below, at and above it on both axes, images smaller than the halo, and
129 x 257 (several tiles on both axes, a width that is no multiple of 4). The
radii 0.5, 2.0 and 8.0 give the box radii 0, 1 and 7 (halos of 3, 6 and 24).
"""
import numpy as np
import pyarrow as pa
import pytest

import test_gpu_color as C
from conftest import read_golden
from oracle import oracle

pytestmark = pytest.mark.gpu

NAN = float("nan")
ORDER0123 = C.ORDER0123
TH, TW = 32, 64
RADII = (0.5, 2.0, 8.0)
PLAIN = (NAN, NAN, NAN, NAN, ORDER0123, 0, -1)


@pytest.fixture(scope="module")
def cells():
    return [(name, read_golden("jpeg/" + name)) for name in C.NAMES]


def _pil_chain(u8, row):
    """Pillow's chain on an [h, w, 3] uint8 image with one 8-column row: the jitter and the grayscale (the
    colour tests' chain without its solarize), the blur, the solarize."""
    from PIL import Image, ImageFilter, ImageOps

    head = np.array(row[:7], np.float64)
    head[6] = -1
    im = Image.fromarray(C._pil_chain(u8, head), "RGB")
    if not (np.isnan(row[7]) or row[7] == 0):
        im = im.filter(ImageFilter.GaussianBlur(float(row[7])))
    if row[6] >= 0:
        im = ImageOps.solarize(im, int(row[6]))
    return np.asarray(im, dtype=np.uint8)


def _check(cells, size, colors, res, lbl, failed, what, views=None, crops=None, windows=None, dtype="float32",
           normalize=None, interp="bilinear", bad=()):
    import torch

    n = len(cells)
    sized = isinstance(size[0], (tuple, list))
    V = len(size) if sized else (views or 1)
    multi = sized or views is not None
    colors = np.asarray(colors, np.float64).reshape(n, V, 8)
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
            out = _pil_chain(u8, colors[i, v])
            if dtype == "uint8":
                want = torch.from_numpy(np.ascontiguousarray(out.transpose(2, 0, 1)))
            else:
                t = oracle.raw_to_tensor(np.ascontiguousarray(out), out.shape[0], out.shape[1],
                                         normalize=C._norm_arg(normalize))
                want = torch.from_numpy(np.array(t)).to(C._td(dtype))
            C._same(got, want, f"{what}: {name} view {v} radius {colors[i, v, 7]}")
            assert int(lbl[i]) == 100 + i


def _rows(n, V, row, radii):
    a = np.empty((n, V, 8), np.float64)
    a[..., :7] = row
    a[..., 7] = radii
    return a


def _random_rows(n, V, seed, radii):
    a = np.empty((n, V, 8), np.float64)
    a[..., :7] = C._random_rows(n, V, seed)
    a[..., 7] = radii
    return a


def _small_crops(cells, size, V):
    """Boxes (every other one flipped) that keep a small output inside the resize's reduction limit."""
    crops = np.zeros((len(cells), V, 5), np.int32)
    for i, (name, data) in enumerate(cells):
        w, h, _ = oracle.jpeg_info(data)
        crops[i, :] = (3, 5, min(h - 3, 30 * size[0]), min(w - 5, 30 * size[1]), i & 1)
    return crops


SHAPES = [(1, 1), (1, 5), (3, 2)] + [(h, w) for h in (TH - 1, TH, TH + 1) for w in (TW - 1, TW, TW + 1)] + [(129, 257)]


@pytest.mark.parametrize("size", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_blur_alone(cells, size):
    """Nothing but the blur, one view per radius. The first two sources; all five at 129 x 257."""
    use = cells if size == (129, 257) else cells[:2]
    V = len(RADII)
    colors = _rows(len(use), V, PLAIN, RADII)
    crops = _small_crops(use, size, V) if size[0] < 100 else None
    res, lbl, failed = C._decode(use, size, colors, views=V, crops=crops)
    _check(use, size, colors, res, lbl, failed, f"blur {size}", views=V, crops=crops)
    if size == (TH + 1, TW + 1):  # the blur changes pixels, more at a larger radius
        plain, _, _ = C._decode(use, size, None, views=V)
        d = [(res[v].double() - plain[v].double()).abs().sum().item() for v in range(V)]
        assert 0 < d[0] < d[2]


@pytest.mark.parametrize("size", [(TH + 1, TW + 1), (129, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_full_chain(cells, size):
    """Every jitter op in a random order (the contrast mean is taken before the blur), some gray, some solarize."""
    use = cells if size[0] < 100 else cells[:3]
    V = len(RADII)
    colors = _random_rows(len(use), V, 40 + size[0], RADII)
    colors[0, :, 5:7] = (1, 128)  # gray, blur and solarize together at every radius
    res, lbl, failed = C._decode(use, size, colors, views=V)
    _check(use, size, colors, res, lbl, failed, f"chain {size}", views=V)


def test_blur_and_no_blur_mixed_in_one_batch(cells):
    """Rows without a blur (NaN and 0) go through k_color_apply, the others through k_color_blur."""
    n, size = len(cells), (40, 70)
    colors = _random_rows(n, 1, 8, 0.0)[:, 0]
    colors[:, 7] = [1.3, NAN, 0.0, 8.0, 0.4]
    res, lbl, failed = C._decode(cells, size, colors)
    _check(cells, size, colors, res, lbl, failed, "mixed")
    # the rows without a blur are what seven columns give
    res7, _, _ = C._decode(cells, size, colors[:, :7])
    for i in (1, 2):
        assert (res[0][i] == res7[0][i]).all().item()
    assert (res[0][0] != res7[0][0]).any().item()


def test_two_views(cells):
    n, size = len(cells), (36, 72)
    colors = _random_rows(n, 2, 21, [1.7, NAN])  # DINO's first global view always blurs
    colors[::2, 1, 7] = 0.9
    crops = _small_crops(cells, (8, 8), 2)
    crops[:, 1, :2] += 9  # the second view: a smaller box with the same far corner, mirrored the other way
    crops[:, 1, 2:4] -= 9
    crops[:, 1, 4] ^= 1
    res, lbl, failed = C._decode(cells, size, colors, views=2, crops=crops)
    _check(cells, size, colors, res, lbl, failed, "two views", views=2, crops=crops)


def test_size_list(cells):
    sizes = [(32, 32), (24, 40), (8, 8)]
    colors = _random_rows(len(cells), 3, 13, [2.0, 0.5, 8.0])
    crops = _small_crops(cells, (8, 8), 3)  # 240 pixels at the most: the 8 x 8 view reduces by 30
    res, lbl, failed = C._decode(cells, sizes, colors, crops=crops)
    _check(cells, sizes, colors, res, lbl, failed, "size list", crops=crops)


@pytest.mark.parametrize("mf", ["contiguous", "channels_last"])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16", "uint8"])
def test_dtypes_and_layouts(cells, dtype, mf):
    """Every dtype in both layouts; the float ones with Normalize under channels_last. 41 columns: rows that
    start at every alignment."""
    two = cells[:2]
    normalize = True if (mf == "channels_last" and dtype != "uint8") else None
    size = (34, 41)
    colors = _random_rows(2, 2, 77, [1.1, 8.0])
    res, lbl, failed = C._decode(two, size, colors, views=2, dtype=dtype, mf=mf, normalize=normalize)
    _check(two, size, colors, res, lbl, failed, f"{dtype} {mf}", views=2, dtype=dtype, normalize=normalize)


def test_normalize_224(cells):
    """The default size takes the band kernel for the resize; Normalize in float32."""
    two = cells[:2]
    colors = _random_rows(2, 1, 31, [[2.0], [0.7]])[:, 0]
    res, lbl, failed = C._decode(two, (224, 224), colors, normalize=True)
    _check(two, (224, 224), colors, res, lbl, failed, "224 normalize", normalize=True)


def test_bicubic_with_a_window(cells):
    n, size = len(cells), (32, 40)
    windows = np.array([[48, 56, 9, 7]] * n, np.int32)
    colors = _random_rows(n, 1, 99, 1.5)[:, 0]
    res, lbl, failed = C._decode(cells, size, colors, windows=windows, interpolation="bicubic")
    _check(cells, size, colors, res, lbl, failed, "bicubic", windows=windows, interp="bicubic")


def test_progressive_and_grey_sources(cells):
    two = [cells[2], cells[3]]
    size = (TH + 3, TW + 5)
    colors = _random_rows(2, 3, 55, RADII)
    res, lbl, failed = C._decode(two, size, colors, views=3)
    _check(two, size, colors, res, lbl, failed, "prog / grey", views=3)


def test_failed_row_between_good_ones(cells):
    """The failed row stays zero and does not disturb its neighbours."""
    mixed = [cells[0], ("bad", read_golden("jpeg/bad_not_jpeg.bin")), cells[1], cells[3]]
    colors = _rows(4, 2, (1.1, 1.6, 0.8, 0.2, 1 + 4 * 0 + 16 * 2 + 64 * 3, 0, 128), [2.0, 8.0])
    res, lbl, failed = C._decode(mixed, (36, 70), colors, views=2)
    assert failed == {1: 1}
    _check(mixed, (36, 70), colors, res, lbl, failed, "failed row", views=2, bad=(1,))
    res, lbl, failed = C._decode(mixed, (36, 70), colors[:, 0], dtype="bfloat16", mf="channels_last")
    _check(mixed, (36, 70), colors[:, 0], res, lbl, failed, "failed row bf16", dtype="bfloat16", bad=(1,))


def test_seeded_sampler(cells):
    """decode_tensor_image(views=2) with ColorJitterParams(blur_p=[1.0, 0.1]): the boxes are drawn first, then
    the colours, each from its own seeded generator."""
    import torch

    import ldt_amd

    def gens():
        a, b = torch.Generator(), torch.Generator()
        a.manual_seed(1234)
        b.manual_seed(4321)
        return a, b

    def color(g):
        return ldt_amd.ColorJitterParams(blur_p=[1.0, 0.1], solarize_p=[0.0, 0.2], generator=g)

    n, size = len(cells), (48, 72)
    rb = pa.RecordBatch.from_arrays([pa.array([d for _, d in cells], pa.binary()),
                                     pa.array(np.arange(100, 100 + n), pa.int64())], names=["image", "label"])
    ga, gb = gens()
    out = ldt_amd.decode_tensor_image(rb, size=size, views=2, device="cuda:0",
                                      crop=ldt_amd.RandomResizedCropFlip(scale=(0.3, 1.0), generator=ga),
                                      color=color(gb))
    ga, gb = gens()
    wh, status = ldt_amd.image_sizes([d for _, d in cells])
    crops = ldt_amd.RandomResizedCropFlip(scale=(0.3, 1.0), generator=ga).sample(wh, status, views=2)
    colors = color(gb).sample(n, views=2)
    assert colors.shape == (n, 2, 8) and not np.isnan(colors[:, 0, 7]).any()
    img = out["image"].cpu()
    assert tuple(img.shape) == (2, n, 3) + size
    _check(cells, size, colors, [img[0], img[1]], out["label"].cpu().numpy(), {}, "sampler", views=2, crops=crops)


def test_set_colors_and_the_stage_count(cells):
    """ldt_set_colors refuses a record whose blur fields are no pair ldt_blur_weights gives and leaves nothing
    pending; a zeroed tail is a record without blur; the blur runs inside the colour stage's one mark."""
    import ldt_amd
    from ldt_amd import _lib

    n, size = len(cells), (24, 70)
    good = _random_rows(n, 1, 3, 1.2)[:, 0]
    ctx = _lib.Context(0)
    ctx.set_option(_lib.OPT_PROFILE, 1)
    rec = _lib.check_colors(good, n)
    assert set(rec["blur_r"].tolist()) == {0}  # radius 1.2
    # (2r + 1) * ww > 2^24, (2r + 3) * ww < 2^24 twice
    for field, value in (("blur_r", 8), ("blur_ww", (1 << 24) + 1), ("blur_ww", (1 << 24) // 3 - 1), ("blur_ww", 1)):
        bad = rec.copy()
        bad[field][1] = value
        with pytest.raises(ldt_amd.LdtError, match="rc=-1"):
            ctx.use_colors(bad)
        res, lbl, failed = C._decode(cells, size, None, ctx=ctx)  # nothing was left pending
        C._check(cells, size, None, res, lbl, failed, f"after a refused {field}")
    assert ctx.stage_times()["color"][1] == 0
    bad = rec.copy()
    bad["blur_ww"][0] = 0
    bad["blur_r"][0] = 8  # out of range even without a blur
    with pytest.raises(ldt_amd.LdtError, match="rc=-1"):
        ctx.use_colors(bad)
    # a zeroed tail: the record of a library without blur
    plain = rec.copy()
    plain["blur_ww"] = 0
    plain["blur_r"] = 0
    res, lbl, failed = C._decode(cells, size, plain, ctx=ctx)
    C._check(cells, size, good[:, :7], res, lbl, failed, "zeroed tail")
    assert ctx.stage_times()["color"][1] == 1
    # with the blur: still one mark per call
    res, lbl, failed = C._decode(cells, size, rec, ctx=ctx)
    _check(cells, size, good, res, lbl, failed, "records")
    st = ctx.stage_times()
    assert st["color"][1] == 2 and st["resize"][1] == 6
