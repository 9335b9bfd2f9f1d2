"""GPU tests of ``color=`` / ``colors=`` (ldt_set_colors): ColorJitter,
RandomGrayscale and RandomSolarize per output image, fused behind the resize.

The expected value of every output image is computed on the host and compared
bit for bit in the call's dtype:

  1. the oracle's Pillow-exact resized bytes of that row and view
     (``oracle.decode_rgb``, then ``raw_to_tensor`` at the box and window;
     Pillow itself for bicubic), mirrored when the view is flipped;
  2. Pillow's own ``ImageEnhance.Brightness`` / ``Contrast`` / ``Color`` in the
     entry's order, and torchvision's ``adjust_hue`` restated on PIL
     (``convert("HSV")``, a uint8 wrap-add on H, ``convert("RGB")``);
  3. ``convert("L")`` stacked three times, then ``ImageOps.solarize``;
  4. the ToTensor / Normalize table (the oracle's identity resize), converted
     by torch to the call's dtype.

A failed row is all-zero bytes with label -100. Every decode goes into the
middle of a buffer full of a sentinel, and the bytes around the output are
checked after it.
"""
import itertools

import numpy as np
import pyarrow as pa
import pytest

from conftest import read_golden
from oracle import oracle

pytestmark = pytest.mark.gpu

NAN = float("nan")
ORDER0123 = 0 + 4 * 1 + 16 * 2 + 64 * 3
SENTINEL = 0xA5
GUARD = 4096
ES = {"float32": 4, "float16": 2, "bfloat16": 2, "uint8": 1}
NAMES = ("noisy_256x256_q50.jpg", "c4_250x333_q90_rstblk.jpg", "prog_64x80.jpg", "gray_77x91.jpg",
         "s444_100x300.jpg")  # baseline 4:2:0 (one with restarts), progressive, grey, 4:4:4


def _td(dtype):
    import torch

    return {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16, "uint8": torch.uint8}[dtype]


@pytest.fixture(scope="module")
def cells():
    return [(name, read_golden("jpeg/" + name)) for name in NAMES]


_rgb, _u8 = {}, {}


def _resized_u8(name, data, size, crop=None, window=None, interp="bilinear"):
    """Step 1: the resized bytes [h, w, 3] of one view. Computed once per distinct view, never changed."""
    key = (name, size, None if crop is None else tuple(int(v) for v in crop),
           None if window is None else tuple(int(v) for v in window), interp)
    if key not in _u8:
        if name not in _rgb:
            _rgb[name] = oracle.decode_rgb(data)
        rgb = _rgb[name]
        top, left, bh, bw, flip = key[2] if crop is not None else (0, 0, rgb.shape[0], rgb.shape[1], 0)
        rh, rw, wt, wl = key[3] if window is not None else (size[0], size[1], 0, 0)
        src = np.ascontiguousarray(rgb[top:top + bh, left:left + bw])
        if interp == "bilinear":
            t = oracle.raw_to_tensor(src, rh, rw)  # byte / 255 in float32: the byte comes back exactly
            u8 = np.rint(t.astype(np.float64) * 255.0).astype(np.uint8).transpose(1, 2, 0)
        else:
            from PIL import Image

            u8 = np.asarray(Image.fromarray(src).resize((rw, rh), Image.BICUBIC), dtype=np.uint8)
        u8 = u8[wt:wt + size[0], wl:wl + size[1]]
        u8 = np.ascontiguousarray(u8[:, ::-1] if flip else u8)
        u8.setflags(write=False)
        _u8[key] = u8
    return _u8[key]


def _pil_chain(u8, row):
    """Steps 2 and 3 on an [h, w, 3] uint8 image with one colour row, by Pillow itself."""
    from PIL import Image, ImageEnhance, ImageOps

    im = Image.fromarray(u8, "RGB")
    b, c, s, hue, order, gray, sol = (float(v) for v in row)
    for k in range(4):
        op = (int(order) >> (2 * k)) & 3
        if op == 0 and not np.isnan(b):
            im = ImageEnhance.Brightness(im).enhance(b)
        elif op == 1 and not np.isnan(c):
            im = ImageEnhance.Contrast(im).enhance(c)
        elif op == 2 and not np.isnan(s):
            im = ImageEnhance.Color(im).enhance(s)
        elif op == 3 and not np.isnan(hue):
            h, sat, v = im.convert("HSV").split()
            nh = (np.asarray(h, np.uint8).astype(np.int64) + int(hue * 255)).astype(np.uint8)  # uint8 wrap-add
            im = Image.merge("HSV", (Image.fromarray(nh, "L"), sat, v)).convert("RGB")
    if gray:
        lum = im.convert("L")
        im = Image.merge("RGB", (lum, lum, lum))
    if sol >= 0:
        im = ImageOps.solarize(im, int(sol))
    return np.asarray(im, dtype=np.uint8)


def _expected(u8, row, dtype="float32", normalize=None):
    """Step 4: a CPU tensor [3, h, w] of the call's dtype."""
    import torch

    out = _pil_chain(u8, row) if row is not None else u8
    if dtype == "uint8":
        return torch.from_numpy(np.ascontiguousarray(out.transpose(2, 0, 1)))
    t = oracle.raw_to_tensor(np.ascontiguousarray(out), out.shape[0], out.shape[1], normalize=normalize)
    return torch.from_numpy(np.array(t)).to(_td(dtype))


def _same(got, want, what):
    import torch

    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, tuple(got.shape))
    got = got.contiguous()
    if not torch.equal(got.view(torch.uint8), want.contiguous().view(torch.uint8)):
        d = (got.to(torch.float64) - want.to(torch.float64)).abs()
        raise AssertionError(f"{what}: {int((d > 0).sum())} of {d.numel()} elements differ, max abs {float(d.max())}")


def _norm_arg(normalize):
    from ldt_amd import IMAGENET_MEAN, IMAGENET_STD

    return (IMAGENET_MEAN, IMAGENET_STD) if normalize is True else normalize


def _decode(cells, size, colors, views=None, crops=None, windows=None, dtype="float32", mf="contiguous",
            normalize=None, interpolation=None, ctx=None):
    """decode_arrow into the middle of a sentinel buffer. Returns (list over views of CPU tensors [n, 3, h, w],
    labels, {failed row: status}); asserts the guards. `size`: a pair, or a list of pairs (one per view)."""
    import torch

    import ldt_amd
    from ldt_amd import transforms as T

    n = len(cells)
    sized = isinstance(size[0], (tuple, list))
    sizes = list(size) if sized else [size] * (views or 1)
    nbytes = sum(n * 3 * h * w for h, w in sizes) * ES[dtype]
    buf = torch.full((GUARD + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    flat = buf[GUARD:GUARD + nbytes].view(_td(dtype))
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
    try:
        T.decode_arrow(pa.array([d for _, d in cells], pa.binary()), labels, out=out, out_lbl=lflat[1:n + 1],
                       size=[tuple(s) for s in size] if sized else size, normalize=normalize, crops=crops,
                       windows=windows, views=None if sized else views, colors=colors, dtype=_td(dtype),
                       memory_format=torch.channels_last if cl else None, interpolation=interpolation, ctx=ctx)
    except ldt_amd.ImageDecodeError as e:
        failed = dict(e.rows)
    finally:
        torch.cuda.synchronize()
        assert torch.all(buf[:GUARD] == SENTINEL).item(), "wrote before the output"
        assert torch.all(buf[GUARD + nbytes:] == SENTINEL).item(), "wrote past the output"
        assert int(lflat[0]) == -777 and int(lflat[n + 1]) == -777
    res, at, host = [], 0, flat.cpu()
    for h, w in sizes:
        blk = host[at:at + n * 3 * h * w]
        res.append(blk.view(n, h, w, 3).permute(0, 3, 1, 2) if cl else blk.view(n, 3, h, w))
        at += n * 3 * h * w
    return res, lflat[1:n + 1].cpu().numpy(), failed


def _check(cells, size, colors, res, lbl, failed, what, views=None, crops=None, windows=None, dtype="float32",
           normalize=None, interp="bilinear", bad=()):
    """Every output image (v, i) against the host's expected value."""
    import torch

    n = len(cells)
    sized = isinstance(size[0], (tuple, list))
    V = len(size) if sized else (views or 1)
    multi = sized or views is not None
    colors = None if colors is None else np.asarray(colors, np.float64).reshape(n, V, 7)
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
            u8 = _resized_u8(name, data, sz, crop, win, interp)
            want = _expected(u8, None if colors is None else colors[i, v], dtype, _norm_arg(normalize))
            _same(got, want, f"{what}: {name} view {v}")
            assert int(lbl[i]) == 100 + i


def _rows(n, V, row):
    a = np.empty((n, V, 7), np.float64)
    a[:] = row
    return a


def _random_rows(n, V, seed, contrast=True):
    """A full jitter per output image, every order, some gray and some solarize."""
    rng = np.random.default_rng(seed)
    perms = list(itertools.permutations(range(4)))
    a = np.empty((n, V, 7), np.float64)
    for i in range(n):
        for v in range(V):
            p = perms[int(rng.integers(24))]
            a[i, v] = (rng.uniform(0.2, 1.9), rng.uniform(0.2, 1.9) if contrast else NAN, rng.uniform(0.0, 2.2),
                       rng.uniform(-0.5, 0.5), p[0] + 4 * p[1] + 16 * p[2] + 64 * p[3], int(rng.integers(4) == 0),
                       (-1, -1, 128, 77)[int(rng.integers(4))])
    return a


FACTORS = (0.0, 0.6, 1.0, 1.4, 2.5)


@pytest.mark.parametrize("col", [0, 1, 2], ids=["brightness", "contrast", "saturation"])
def test_each_op_alone(cells, col):
    """One view per factor; rows of 50 bytes, so no plane row but the first is dword-aligned."""
    size, V = (33, 50), len(FACTORS)
    colors = _rows(len(cells), V, (NAN, NAN, NAN, NAN, ORDER0123, 0, -1))
    colors[:, :, col] = FACTORS
    res, lbl, failed = _decode(cells, size, colors, views=V)
    _check(cells, size, colors, res, lbl, failed, f"op {col}", views=V)


def test_hue_alone(cells):
    size, hues = (33, 50), (-0.5, -0.1, 0.0, 0.1, 0.5)
    colors = _rows(len(cells), len(hues), (NAN, NAN, NAN, NAN, ORDER0123, 0, -1))
    colors[:, :, 3] = hues
    res, lbl, failed = _decode(cells, size, colors, views=len(hues))
    _check(cells, size, colors, res, lbl, failed, "hue", views=len(hues))
    # hue 0.0 is performed: the HSV round trip changes pixels
    plain, _, _ = _decode(cells, size, None, views=len(hues))
    assert (res[2] != plain[2]).any().item()


@pytest.mark.parametrize("half", [0, 1])
def test_all_24_orders(cells, half):
    """All four ops present in every order: the contrast mean depends on what preceded it."""
    perms = list(itertools.permutations(range(4)))[12 * half:12 * half + 12]
    two = cells[:2]
    colors = _rows(2, 12, (1.3, 0.7, 1.9, -0.1, 0, 0, -1))
    colors[:, :, 4] = [p[0] + 4 * p[1] + 16 * p[2] + 64 * p[3] for p in perms]
    res, lbl, failed = _decode(two, (32, 32), colors, views=12)
    _check(two, (32, 32), colors, res, lbl, failed, "orders", views=12)
    assert any((res[0] != res[v]).any().item() for v in range(1, 12))  # the order matters


def test_gray_and_solarize_alone_and_with_the_jitter(cells):
    jit = (1.2, 1.5, 0.4, 0.07, 2 + 4 * 0 + 16 * 3 + 64 * 1)
    none = (NAN, NAN, NAN, NAN, ORDER0123)
    per_view = [none + (1, -1), none + (0, 128), none + (0, 0), none + (0, 256), none + (1, 100), jit + (1, -1),
                jit + (0, 128), jit + (1, 1)]
    colors = _rows(len(cells), len(per_view), per_view[0])
    colors[:] = np.array(per_view)
    res, lbl, failed = _decode(cells, (32, 32), colors, views=len(per_view))
    _check(cells, (32, 32), colors, res, lbl, failed, "gray/solarize", views=len(per_view))


def test_nothing_present_equals_the_plain_call(cells):
    import torch

    colors = _rows(len(cells), 1, (NAN, NAN, NAN, NAN, ORDER0123, 0, -1))[:, 0]
    res, lbl, failed = _decode(cells, (40, 36), colors)
    plain, _, _ = _decode(cells, (40, 36), None)
    assert torch.equal(res[0], plain[0])
    _check(cells, (40, 36), colors, res, lbl, failed, "identity")


@pytest.mark.parametrize("size", [(1, 1), (5, 7), (13, 17), (129, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_output_sizes(cells, size):
    """Rows that are no multiple of 4 bytes, images smaller than a wave, and (129 x 257) a mean reduced over
    several workgroups with an odd width. The small sizes take a box (with a flip) to stay inside the reduction
    limit of 37."""
    n = len(cells)
    crops = None
    if size[0] < 100:
        crops = np.zeros((n, 5), np.int32)
        for i, (name, data) in enumerate(cells):
            w, h, _ = oracle.jpeg_info(data)
            crops[i] = (3, 5, min(h - 3, 30 * size[0]), min(w - 5, 30 * size[1]), i & 1)
    colors = _random_rows(n, 1, 1000 + size[1])[:, 0]
    res, lbl, failed = _decode(cells, size, colors, crops=crops)
    _check(cells, size, colors, res, lbl, failed, f"size {size}", crops=crops)


def test_size_list_with_different_entries_per_view(cells):
    sizes = [(32, 32), (17, 9)]
    colors = _random_rows(len(cells), 2, 5)
    res, lbl, failed = _decode(cells, sizes, colors)
    _check(cells, sizes, colors, res, lbl, failed, "size list")
    with pytest.raises(ValueError):
        _decode(cells, sizes, colors[:, 0])  # a 2-D array in a call with views


def test_two_views_with_seeded_samplers(cells):
    """decode_tensor_image(views=2) with a RandomResizedCropFlip and a ColorJitterParams: the boxes are drawn
    first, then the colours, each from its own seeded generator."""
    import torch

    import ldt_amd

    def gens():
        a, b = torch.Generator(), torch.Generator()
        a.manual_seed(1234)
        b.manual_seed(4321)
        return a, b

    n, size = len(cells), (48, 40)
    rb = pa.RecordBatch.from_arrays([pa.array([d for _, d in cells], pa.binary()),
                                     pa.array(np.arange(100, 100 + n), pa.int64())], names=["image", "label"])
    ga, gb = gens()
    out = ldt_amd.decode_tensor_image(rb, size=size, views=2, device="cuda:0",
                                      crop=ldt_amd.RandomResizedCropFlip(scale=(0.3, 1.0), generator=ga),
                                      color=ldt_amd.ColorJitterParams(solarize_p=[0.0, 0.5], generator=gb))
    ga, gb = gens()
    wh, status = ldt_amd.image_sizes([d for _, d in cells])
    crops = ldt_amd.RandomResizedCropFlip(scale=(0.3, 1.0), generator=ga).sample(wh, status, views=2)
    colors = ldt_amd.ColorJitterParams(solarize_p=[0.0, 0.5], generator=gb).sample(n, views=2)
    img = out["image"].cpu()
    assert tuple(img.shape) == (2, n, 3) + size
    _check(cells, size, colors, [img[0], img[1]], out["label"].cpu().numpy(), {}, "samplers", views=2, crops=crops)


@pytest.mark.parametrize("mf", ["contiguous", "channels_last"])
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16", "uint8"])
def test_dtypes_and_layouts(cells, dtype, mf):
    """Every dtype in both layouts; the float ones with Normalize under channels_last."""
    normalize = True if (mf == "channels_last" and dtype != "uint8") else None
    size = (30, 41) if mf == "channels_last" else (28, 36)
    colors = _random_rows(len(cells), 2, 77)
    res, lbl, failed = _decode(cells, size, colors, views=2, dtype=dtype, mf=mf, normalize=normalize)
    _check(cells, size, colors, res, lbl, failed, f"{dtype} {mf}", views=2, dtype=dtype, normalize=normalize)


def test_normalize_single_view_224(cells):
    """The default size takes the band kernel for the resize; Normalize in float32."""
    colors = _random_rows(len(cells), 1, 31)[:, 0]
    res, lbl, failed = _decode(cells, (224, 224), colors, normalize=True)
    _check(cells, (224, 224), colors, res, lbl, failed, "224 normalize", normalize=True)


def test_bicubic_with_a_window(cells):
    n, size = len(cells), (32, 40)
    windows = np.array([[48, 56, 9, 7]] * n, np.int32)
    colors = _random_rows(n, 1, 99)[:, 0]
    res, lbl, failed = _decode(cells, size, colors, windows=windows, interpolation="bicubic")
    _check(cells, size, colors, res, lbl, failed, "bicubic", windows=windows, interp="bicubic")


def test_failed_row_between_good_ones(cells):
    """The failed row stays zero and does not disturb its neighbours' means."""
    mixed = [cells[0], ("bad", read_golden("jpeg/bad_not_jpeg.bin")), cells[1], cells[3]]
    colors = _rows(4, 2, (1.1, 1.6, 0.8, 0.2, 1 + 4 * 0 + 16 * 2 + 64 * 3, 0, 128))
    res, lbl, failed = _decode(mixed, (36, 44), colors, views=2)
    assert failed == {1: 1}
    _check(mixed, (36, 44), colors, res, lbl, failed, "failed row", views=2, bad=(1,))
    res, lbl, failed = _decode(mixed, (36, 44), colors[:, 0], dtype="bfloat16", mf="channels_last")
    _check(mixed, (36, 44), colors[:, 0], res, lbl, failed, "failed row bf16", dtype="bfloat16", bad=(1,))


def test_pipeline_and_device_batch(cells):
    import torch

    import ldt_amd
    from ldt_amd import transforms as T

    n, size = len(cells), (32, 48)
    colors = _random_rows(n, 1, 12)[:, 0]
    rb = pa.RecordBatch.from_arrays([pa.array([d for _, d in cells], pa.binary()),
                                     pa.array(np.arange(100, 100 + n), pa.int64())], names=["image", "label"])
    pipe = ldt_amd.DecodePipeline(depth=2, device="cuda:0", size=size)
    img, lbl = pipe.decode(rb, colors=colors)
    plain, _ = pipe.decode(rb)  # the next batch of the pipeline has no colours
    pipe.check()
    torch.cuda.synchronize()
    _check(cells, size, colors, [img.cpu()], lbl.cpu().numpy(), {}, "pipeline")
    _check(cells, size, None, [plain.cpu()], lbl.cpu().numpy(), {}, "pipeline, plain")
    # a pipeline-wide sampler draws per batch
    g = torch.Generator()
    g.manual_seed(5)
    pipe2 = ldt_amd.DecodePipeline(depth=2, device="cuda:0", size=size, color=ldt_amd.ColorJitterParams(generator=g))
    img2, lbl2 = pipe2.decode(ldt_amd.ResidentBatch([d for _, d in cells], range(100, 100 + n), device="cuda:0"))
    pipe2.check()
    g.manual_seed(5)
    _check(cells, size, ldt_amd.ColorJitterParams(generator=g).sample(n), [img2.cpu()], lbl2.cpu().numpy(), {},
           "pipeline sampler")
    # a DeviceBatch carries the (checked) array to where it is decoded
    packed = T._pack_list([d for _, d in cells], list(range(100, 100 + n)))
    db = T.DeviceBatch(packed, "cuda:0", None, size=size, color=colors, dtype=torch.float16)
    _check(cells, size, colors, [db["image"].cpu()], db["label"].cpu().numpy(), {}, "device batch", dtype="float16")
    with pytest.raises(ValueError):
        T.DeviceBatch(packed, "cuda:0", None, size=size, color=colors[:-1])
    fn = ldt_amd.make_collate_fn(device="cuda:0", size=size, color=colors)
    out = fn([{"image": d, "label": 100 + i} for i, (_, d) in enumerate(cells)])
    _check(cells, size, colors, [out["image"].cpu()], out["label"].cpu().numpy(), {}, "collate")


def test_wrong_count_refused_and_pending_state_consumed(cells):
    """A colour array of the wrong count enqueues nothing; resize_raw refuses colours; the call after a call
    with colours is a plain call; the colour stage is profiled as a stage of its own."""
    import torch

    import ldt_amd
    from ldt_amd import _lib
    from ldt_amd import transforms as T

    n, size = len(cells), (24, 28)
    good = _random_rows(n, 1, 3)[:, 0]
    with pytest.raises(ValueError):
        _decode(cells, size, good[:-1])
    ctx = _lib.Context(0)
    ctx.set_option(_lib.OPT_PROFILE, 1)
    # pending colours for another count: LDT_ERR_ARG, the output keeps its sentinel
    short = _lib.check_colors(good[:-1], n - 1)
    ctx.use_colors(short)
    out = torch.full((n, 3) + size, -7.0, device="cuda")
    with pytest.raises(ldt_amd.LdtError, match="rc=-1"):
        T.decode_arrow(pa.array([d for _, d in cells], pa.binary()), None, out=out, size=size, ctx=ctx)
    torch.cuda.synchronize()
    assert torch.all(out == -7.0).item()
    # that call consumed them: the next one is plain
    res, lbl, failed = _decode(cells, size, None, ctx=ctx)
    _check(cells, size, None, res, lbl, failed, "after a refused call")
    assert ctx.stage_times()["color"][1] == 0
    # a call with colours, then one without
    res, lbl, failed = _decode(cells, size, good, ctx=ctx)
    _check(cells, size, good, res, lbl, failed, "with colours")
    assert ctx.stage_times()["color"][1] == 1
    res, lbl, failed = _decode(cells, size, None, ctx=ctx)
    _check(cells, size, None, res, lbl, failed, "after a call with colours")
    st = ctx.stage_times()
    assert st["color"][1] == 1 and st["resize"][1] == 3
    # views: n * V entries or nothing
    ctx.use_colors(_lib.check_colors(good, n))
    with pytest.raises(ldt_amd.LdtError, match="rc=-1"):
        T.decode_arrow(pa.array([d for _, d in cells], pa.binary()), None, size=size, views=2, ctx=ctx)
    # an entry the library refuses leaves nothing pending
    bad = _lib.check_colors(good, n).copy()
    bad["order"][0] = (0, 0, 1, 2)
    with pytest.raises(ldt_amd.LdtError, match="rc=-1"):
        ctx.use_colors(bad)
    res, lbl, failed = _decode(cells, size, None, ctx=ctx)
    _check(cells, size, None, res, lbl, failed, "after a refused entry")
    # raw sources are out of scope: resize_raw with colours pending is refused and consumes them
    shared = T._decoder("cuda:0").ctx
    raw = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    with shared.lock:
        shared.use_colors(_lib.check_colors(good[:2], 2))
    with pytest.raises(ldt_amd.LdtError, match="rc=-1"):
        T.resize_raw(raw, 16, 16, size=(8, 8), normalize=None)
    assert tuple(T.resize_raw(raw, 16, 16, size=(8, 8), normalize=None).shape) == (2, 3, 8, 8)
    with pytest.raises(TypeError):
        T.resize_raw(raw, 16, 16, size=(8, 8), normalize=None, colors=good[:2])
