"""GPU tests of the native decode (ldt_set_native, ``decode_native``): every row at its own size against
Pillow itself (``Image.open(b).convert("RGB")``, after ``draft`` for a drafted row, then ``.crop()`` and
``ImageOps.mirror``), every byte equal. k_emit_rgb's tile is 16 rows x 256 columns; sizes are width x height."""
import ctypes
import io

import numpy as np
import pyarrow as pa
import pytest

import jpeg_recode as jr
from conftest import read_golden
from draft_ref import drafted_rgb

pytestmark = pytest.mark.gpu

SUB = {"444": "4:4:4", "422": "4:2:2", "420": "4:2:0"}
# (width, height, layout): cdw <= 2, inside an MCU, one past an MCU edge, an exact MCU, one past the tile's edges
CASES = ([(w, h, lay) for w, h in ((1, 1), (3, 5)) for lay in ("420", "422")] +
         [(7, 5, lay) for lay in ("444", "422", "420")] +
         [(w, h, lay) for w, h in ((17, 9), (33, 31)) for lay in ("444", "422", "420", "440", "411")] +
         [(16, 16, "420"), (257, 17, "420"), (257, 17, "444"), (300, 20, "420"), (300, 20, "422"),
          (17, 9, "gray"), (17, 9, "adobe0"), (33, 31, "prog420")])


def _cell(w, h, layout, seed):
    from PIL import Image

    from ldt_amd import synth

    a = synth.field(h, w, seed, 12.0)
    if layout in ("440", "411"):
        return jr.reframe(jr.layout_source(), dict(jr.LAYOUTS)[layout], h, w)
    if layout == "adobe0":
        return jr.reframe(jr.layout_source(), ((1, 1),) * 3, h, w, app=jr.adobe(0))
    kw = dict(progressive=True, subsampling="4:2:0") if layout == "prog420" else \
        {} if layout == "gray" else dict(subsampling=SUB[layout])
    b = io.BytesIO()
    Image.fromarray(a[:, :, 0] if layout == "gray" else a).save(b, format="JPEG", quality=90, **kw)
    return b.getvalue()


def _pil(data, draft=1, box=None):
    """[3, h, w] uint8: Pillow's RGB image of the cell, drafted, cropped and mirrored as the row asks."""
    from PIL import Image, ImageOps

    im = Image.open(io.BytesIO(data)).convert("RGB") if draft == 1 else drafted_rgb(data, draft)
    if box is not None:
        top, left, h, w, flip = box
        im = im.crop((left, top, left + w, top + h))
        im = ImageOps.mirror(im) if flip else im
    return np.ascontiguousarray(np.asarray(im).transpose(2, 0, 1))


def _same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    bad = np.count_nonzero(got != want)
    assert bad == 0, f"{what}: {bad} of {want.size} bytes differ"


@pytest.fixture(scope="module")
def batch():
    """Every case decoded in one call: (cells, the call's tensors on the host)."""
    import torch

    import ldt_amd

    cells = [_cell(w, h, lay, 500 + k) for k, (w, h, lay) in enumerate(CASES)]
    labels = np.arange(len(cells), dtype=np.int64) + 7
    imgs, lbl = ldt_amd.decode_native(cells, labels)
    torch.cuda.synchronize()
    assert lbl.cpu().numpy().tolist() == labels.tolist()
    return cells, [t.cpu().numpy() for t in imgs]


@pytest.mark.parametrize("k", range(len(CASES)), ids=["%dx%d-%s" % c for c in CASES])
def test_sizes_and_layouts(batch, k):
    cells, got = batch
    w, h, lay = CASES[k]
    assert got[k].shape == (3, h, w)
    _same(got[k], _pil(cells[k]), CASES[k])


@pytest.mark.parametrize("dtype, mf, norm", [("uint8", "contiguous", None), ("uint8", "channels_last", None),
                                             ("float32", "contiguous", True), ("bfloat16", "channels_last", None)])
def test_formats(batch, dtype, mf, norm):
    import torch

    import ldt_amd

    pick = [CASES.index(c) for c in ((33, 31, "420"), (257, 17, "420"), (17, 9, "gray"))]
    cells = [batch[0][k] for k in pick]
    imgs, _ = ldt_amd.decode_native(pa.array(cells, pa.binary()), dtype=dtype, memory_format=mf, normalize=norm)
    torch.cuda.synchronize()
    for k, t in zip(pick, imgs):
        w, h, _ = CASES[k]
        assert t.shape == (3, h, w) and t.dtype == getattr(torch, dtype)
        if mf == "channels_last":
            assert t.stride() == (1, 3 * w, 3)
        if dtype == "uint8":
            _same(t, _pil(batch[0][k]), (CASES[k], dtype, mf))
            continue
        # torchvision's F.to_tensor (float32, div 255) and F.normalize (sub mean, div std, in float32), then .to(dtype)
        want = torch.from_numpy(_pil(batch[0][k])).to(torch.float32).div(255)
        if norm:
            mean, std = (torch.tensor(v, dtype=torch.float32)[:, None, None]
                         for v in (ldt_amd.IMAGENET_MEAN, ldt_amd.IMAGENET_STD))
            want = want.sub_(mean).div_(std)
        want = want.to(getattr(torch, dtype))
        bits = torch.int32 if dtype == "float32" else torch.int16
        assert torch.equal(t.cpu().contiguous().view(bits), want.view(bits)), (CASES[k], dtype, mf)


def test_crops():
    """Odd and even origins and sizes, flips, the whole image, a single pixel; 4:2:0 (two tile columns) and 4:2:2."""
    import torch

    import ldt_amd

    src = [_cell(300, 45, "420", 601), _cell(67, 45, "422", 602)]
    rows = [(0, b) for b in ((0, 0, 45, 300, 0), (0, 0, 45, 300, 1), (3, 5, 20, 290, 1), (1, 1, 17, 259, 0),
                             (44, 299, 1, 1, 0), (2, 4, 8, 6, 0), (7, 3, 5, 9, 1))] + \
        [(1, b) for b in ((0, 0, 45, 67, 1), (5, 7, 11, 13, 0), (6, 8, 12, 14, 1), (11, 33, 1, 1, 1))]
    imgs, _ = ldt_amd.decode_native([src[s] for s, _ in rows], crops=np.array([b for _, b in rows]))
    torch.cuda.synchronize()
    for (s, b), t in zip(rows, imgs):
        _same(t, _pil(src[s], box=b), ("crop", s, b))


def test_drafts():
    import torch

    import ldt_amd

    src = [_cell(67, 45, "420", 611), _cell(33, 31, "444", 612)]
    rows = [(s, d) for s in (0, 1) for d in (2, 4, 8)] + [(0, 1)]
    imgs, _ = ldt_amd.decode_native([src[s] for s, _ in rows], drafts=[d for _, d in rows])
    torch.cuda.synchronize()
    for (s, d), t in zip(rows, imgs):
        _same(t, _pil(src[s], draft=d), ("draft", s, d))
    # a box is in the drafted image's coordinates
    imgs, _ = ldt_amd.decode_native([src[0]], drafts=[2], crops=[[3, 5, 9, 11, 1]])
    _same(imgs[0], _pil(src[0], draft=2, box=(3, 5, 9, 11, 1)), "draft and crop")


def _abi_call(ctx, cells, flat, offsets, crops=None, norm=None, entry="batch"):
    """A decode entry point (batch, large or resident) with native offsets (and crops) armed by hand.
    Returns (rc, status)."""
    import torch

    bufs = pa.array(cells, pa.binary() if entry == "batch" else pa.large_binary()).buffers()
    st, s = np.zeros(len(cells), np.int32), torch.cuda.current_stream().cuda_stream
    dev = torch.from_numpy(np.frombuffer(bufs[2], np.uint8).copy()).cuda()
    with ctx.lock:
        ctx.use_format("uint8", "contiguous")
        ctx.use_crops(crops)
        ctx.use_native(offsets)
        if entry == "resident":
            rc = ctx.lib.ldt_decode_batch_resident(ctx.handle, bufs[2].address, dev.data_ptr(), bufs[1].address,
                                                   len(cells), None, flat.data_ptr(), None, norm, s, st.ctypes.data)
        else:
            rc = getattr(ctx.lib, "ldt_decode_" + entry)(ctx.handle, bufs[2].address, bufs[1].address, 0, len(cells),
                                                         None, None, 0, flat.data_ptr(), None, norm, s, st.ctypes.data)
    torch.cuda.synchronize()
    return rc, st


def test_failed_rows():
    import torch

    import ldt_amd
    from ldt_amd import _lib

    good = [_cell(33, 31, "420", 621), _cell(17, 9, "444", 622)]
    cut = good[0][:good[0].rfind(b"\xff\xda") + (len(good[0]) - good[0].rfind(b"\xff\xda")) // 2]
    cells = [good[0], read_golden("jpeg/bad_not_jpeg.bin"), cut, good[1], good[1]]
    boxes = _lib.check_crops([[0, 0, 31, 33, 0], [0, 0, 2, 3, 0], [0, 0, 31, 33, 0], [0, 0, 9, 17, 0],
                              [5, 5, 5, 13, 0]], 5)  # the last one leaves its 17 x 9 image
    codes = {1: 1, 2: 3, 4: 6}  # LDT_IMG_NOT_JPEG, LDT_IMG_CORRUPT, LDT_IMG_BAD_CROP
    with pytest.raises(ldt_amd.ImageDecodeError) as e:
        ldt_amd.decode_native(cells, crops=boxes)
    assert e.value.rows == codes
    # through the ABI, into a caller's buffer of 0xFF whose first and last byte belong to no row
    offsets = 1 + np.concatenate([[0], np.cumsum(3 * boxes[:, 2].astype(np.int64) * boxes[:, 3])])
    flat = torch.full((int(offsets[-1]) + 1,), 0xFF, dtype=torch.uint8, device="cuda")
    rc, st = _abi_call(_lib.get_context(0), cells, flat, offsets, boxes)
    assert rc == _lib.LDT_ERR_IMAGE and {i: int(s) for i, s in enumerate(st) if s} == codes
    host = flat.cpu().numpy()
    for i in range(5):
        region = host[offsets[i]:offsets[i + 1]]
        if i in codes:
            assert region.size and not region.any(), f"failed row {i} is not all zero"
        else:
            _same(region.reshape(3, boxes[i, 2], boxes[i, 3]), _pil(cells[i]), f"row {i}")
    assert host[0] == 0xFF and host[-1] == 0xFF


@pytest.mark.parametrize("what", ("offsets-decrease", "offsets-negative", "n-differs", "region-size", "windows", "views",
                                  "view-sizes", "colors", "augments", "affine-filters", "mix", "u8-norm", "resize-raw",
                                  "windows-batch_large", "windows-resident"))
def test_abi_refusals_leave_nothing_pending(what):
    import torch

    import ldt_amd
    from ldt_amd import _lib

    cells = [_cell(33, 31, "420", 631), _cell(17, 9, "444", 632)]
    ctx, lib = _lib.Context(0), _lib.load_library()
    offsets = np.array([0, 3 * 31 * 33, 3 * 31 * 33 + 3 * 9 * 17], np.int64)
    flat = torch.full((int(offsets[-1]),), 0xFF, dtype=torch.uint8, device="cuda")
    nan = float("nan")
    if what in ("offsets-decrease", "offsets-negative"):
        bad = np.array([5, 4, 9] if what == "offsets-decrease" else [-1, 4, 9], np.int64)
        assert lib.ldt_set_native(ctx.handle, bad.ctypes.data, 2) == _lib.LDT_ERR_ARG
    else:
        norm = None
        with ctx.lock:
            if what.startswith("windows"):
                ctx.use_windows(_lib.check_windows([[224, 224, 0, 0]] * 2, 2))
            elif what == "views":
                ctx.use_views(2)
            elif what == "view-sizes":
                ctx.use_size(_lib.check_view_sizes([(8, 8)]))
            elif what == "colors":
                ctx.use_colors(_lib.check_colors(np.array([[1.2, nan, nan, nan, 228, 0, -1]] * 2), 2))
            elif what == "augments":
                ctx.use_augments(_lib.check_augments(None, 2, None, (8, 8), np.array([[0, 0, 2, 2]] * 2)))
            elif what == "affine-filters":  # an affine op with the BILINEAR filter: augments and filters pending
                ctx.use_augments(_lib.check_augments(np.array([[[1, 1, 0, 1, 0, 1, 1, 0, 0, 0, 1.]]] * 2), 2, None, (8, 8)))
            elif what == "mix":
                rows, nc = _lib.check_mixes((np.array([[1, 1, 0, 0, 0, 0, 0, 1, 0.], [0, 1, 0, 0, 0, 0, 0, 1, 0.]]), 0), 2)
                ctx.use_mix((rows, nc, None))
            elif what == "u8-norm":
                norm = ctypes.byref(_lib.Norm())
        if what == "resize-raw":
            ctx.use_native(offsets)
            raw = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device="cuda")
            out = torch.empty((1, 3, 224, 224), device="cuda")
            rc = lib.ldt_resize_raw(ctx.handle, raw.data_ptr(), 1, 1, 8, 8, 192, out.data_ptr(), None, None)
        else:
            use = offsets[:2] if what == "n-differs" else offsets + np.array([0, 0, 3]) if what == "region-size" \
                else offsets
            rc, _ = _abi_call(ctx, cells, flat, np.ascontiguousarray(use), norm=norm,
                              entry=what.split("-")[1] if what.startswith("windows-") else "batch")
        assert rc == _lib.LDT_ERR_ARG, (what, rc)
        assert flat.cpu().numpy().min() == 0xFF, "a refused call wrote to the output"
    # nothing stayed pending: a plain call on the same context gives the plain result at its own size
    img, _ = ldt_amd.decode_arrow(pa.array(cells[:1], pa.binary()), size=(31, 33), dtype=torch.uint8, ctx=ctx)
    torch.cuda.synchronize()
    _same(img[0], _pil(cells[0]), f"plain call after {what}")
