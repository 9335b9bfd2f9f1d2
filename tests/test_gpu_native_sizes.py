"""GPU tests of ``decode_native(sizes=)`` (ldt_set_native_sizes, k_resize_ragged): every row resized to its own
size against Pillow itself, ``Image.open(b).convert("RGB").resize((w, h), filter)`` (after ``draft``, of the
``.crop()`` box, then ``ImageOps.mirror``), every byte equal. The kernel's tile is TR (8 or 16) rows x 256
columns; sources are 67 x 45, 33 x 31 and 300 x 20 (width x height)."""
import io

import numpy as np
import pyarrow as pa
import pytest

from draft_ref import drafted_rgb

pytestmark = pytest.mark.gpu

SRC = {"a": (67, 45), "b": (33, 31), "c": (300, 20)}
KINDS = ("420", "444", "gray", "prog420")
# (source, h, w): the tile's right edge from an upscale (the second tile's span starts inside the row), its bottom
# edge for TR 8 and 16, single rows and columns, a reduction above 8 on one axis only, the source's own size
CASES = [("a", 45, 255), ("a", 45, 256), ("a", 45, 257), ("b", 7, 33), ("b", 8, 33), ("b", 9, 33), ("b", 15, 20),
         ("b", 16, 20), ("b", 17, 20), ("b", 1, 1), ("b", 1, 257), ("c", 20, 33), ("a", 45, 67), ("c", 20, 300)]
# BICUBIC reduces by at most 18.5 (ceil(2 * src / res) <= 37): the one-row outputs take an 18 x 18 box of the source
ONE_ROW_BOX = (1, 1, 18, 18, 0)


def _box(case):
    s, h, _ = case
    return ONE_ROW_BOX if h == 1 else (0, 0, SRC[s][1], SRC[s][0], 0)


def _cell(name, kind, seed=700):
    from PIL import Image

    from ldt_amd import synth

    w, h = SRC[name]
    a = synth.field(h, w, seed + sum(map(ord, name + kind)), 12.0)
    kw = {} if kind == "gray" else dict(subsampling="4:4:4" if kind == "444" else "4:2:0", progressive=kind == "prog420")
    b = io.BytesIO()
    Image.fromarray(a[:, :, 0] if kind == "gray" else a).save(b, format="JPEG", quality=90, **kw)
    return b.getvalue()


def _pil(data, hw, interp, draft=1, box=None):
    """[3, h, w] uint8: Pillow's resize of the cell, drafted, cropped and mirrored as the row asks."""
    from PIL import Image, ImageOps

    im = Image.open(io.BytesIO(data)).convert("RGB") if draft == 1 else drafted_rgb(data, draft)
    if box is not None:
        im = im.crop((box[1], box[0], box[1] + box[3], box[0] + box[2]))
    im = im.resize((hw[1], hw[0]), Image.BILINEAR if interp == "bilinear" else Image.BICUBIC)
    im = ImageOps.mirror(im) if box is not None and box[4] else im
    return np.ascontiguousarray(np.asarray(im).transpose(2, 0, 1))


def _same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    assert np.count_nonzero(got != want) == 0, f"{what}: {np.count_nonzero(got != want)} of {want.size} bytes differ"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("interp", ("bilinear", "bicubic"))
def test_sizes(interp, kind):
    """All the sizes in one mixed batch per filter and source kind."""
    import torch

    import ldt_amd

    cells = [_cell(s, kind) for s, _, _ in CASES]
    sizes = [(h, w) for _, h, w in CASES]
    labels = np.arange(len(cells), dtype=np.int64) + 3
    imgs, lbl = ldt_amd.decode_native(cells, labels, sizes=sizes, interpolation=interp, crops=[_box(c) for c in CASES])
    plain, _ = ldt_amd.decode_native(cells[-2:])
    torch.cuda.synchronize()
    assert lbl.cpu().numpy().tolist() == labels.tolist()
    for c, cell, hw, t in zip(CASES, cells, sizes, imgs):
        _same(t, _pil(cell, hw, interp, box=_box(c)), (c, interp, kind))
    for t, p in zip(imgs[-2:], plain):  # a size equal to the source is k_emit_rgb's result
        _same(t, p.cpu().numpy(), ("identity", interp, kind))


@pytest.mark.parametrize("interp", ("bilinear", "bicubic"))
def test_crops_and_drafts(interp):
    """Odd origins (the h2v2 phase, the span's first column) with flip 1; a draft of 2 on the 4:2:0 file."""
    import torch

    import ldt_amd

    a, c = _cell("a", "420"), _cell("c", "420")
    rows = [(c, (3, 5, 17, 289, 1), (20, 300)), (c, (1, 1, 19, 259, 1), (9, 40)), (a, (7, 3, 31, 61, 1), (33, 257)),
            (a, (0, 0, 45, 67, 0), (17, 23))]
    imgs, _ = ldt_amd.decode_native([r[0] for r in rows], crops=[r[1] for r in rows], sizes=[r[2] for r in rows],
                                    interpolation=interp)
    drafted, _ = ldt_amd.decode_native([a, a], drafts=[2, 2], sizes=[(40, 50), (23, 34)], interpolation=interp)
    both, _ = ldt_amd.decode_native([a], drafts=[2], crops=[[3, 5, 9, 11, 1]], sizes=[(20, 21)], interpolation=interp)
    torch.cuda.synchronize()
    for (cell, box, hw), t in zip(rows, imgs):
        _same(t, _pil(cell, hw, interp, box=box), ("crop", box, hw))
    for hw, t in zip([(40, 50), (23, 34)], drafted):
        _same(t, _pil(a, hw, interp, draft=2), ("draft", hw))
    _same(both[0], _pil(a, (20, 21), interp, draft=2, box=(3, 5, 9, 11, 1)), "draft and crop")


@pytest.mark.parametrize("dtype, mf, norm", [("uint8", "contiguous", None), ("uint8", "channels_last", None),
                                             ("float32", "contiguous", True), ("bfloat16", "channels_last", None)])
def test_formats(dtype, mf, norm):
    import torch

    import ldt_amd

    rows = [("b", "420", (17, 20)), ("a", "420", (45, 257)), ("b", "gray", (9, 33)), ("c", "444", (20, 33))]
    cells = [_cell(s, k) for s, k, _ in rows]
    imgs, _ = ldt_amd.decode_native(pa.array(cells, pa.binary()), dtype=dtype, memory_format=mf, normalize=norm,
                                    sizes=[hw for _, _, hw in rows], crops=[[0, 0, SRC[s][1], SRC[s][0], i & 1]
                                                                            for i, (s, _, _) in enumerate(rows)])
    torch.cuda.synchronize()
    for i, ((s, k, (h, w)), cell, t) in enumerate(zip(rows, cells, imgs)):
        pil = _pil(cell, (h, w), "bilinear", box=(0, 0, SRC[s][1], SRC[s][0], i & 1))
        assert t.shape == (3, h, w) and t.dtype == getattr(torch, dtype)
        assert mf != "channels_last" or t.stride() == (1, 3 * w, 3)
        if dtype == "uint8":
            _same(t, pil, (rows[i], dtype, mf))
            continue
        want = torch.from_numpy(pil).to(torch.float32).div(255)  # F.to_tensor, F.normalize, then .to(dtype)
        if norm:
            mean, std = (torch.tensor(v, dtype=torch.float32)[:, None, None]
                         for v in (ldt_amd.IMAGENET_MEAN, ldt_amd.IMAGENET_STD))
            want = want.sub_(mean).div_(std)
        want = want.to(getattr(torch, dtype))
        bits = torch.int32 if dtype == "float32" else torch.int16
        assert torch.equal(t.cpu().contiguous().view(bits), want.view(bits)), (rows[i], dtype, mf)


def _abi_call(ctx, cells, flat, offsets, sizes, interp="bilinear", labels=None, crops=None):
    """ldt_decode_batch with native offsets and sizes (and crops) armed by hand; each may be None.
    Returns (rc, status, labels on the host)."""
    import torch

    bufs = pa.array(cells, pa.binary()).buffers()
    st, s = np.zeros(len(cells), np.int32), torch.cuda.current_stream().cuda_stream
    lbl = torch.full((len(cells),), 55, dtype=torch.int64, device="cuda")
    with ctx.lock:
        ctx.use_filter(interp)
        ctx.use_format("uint8", "contiguous")
        ctx.use_crops(crops)
        ctx.use_native(offsets, sizes)
        rc = ctx.lib.ldt_decode_batch(ctx.handle, bufs[2].address, bufs[1].address, 0, len(cells), None,
                                      None if labels is None else labels.ctypes.data, 0, flat.data_ptr(),
                                      None if labels is None else lbl.data_ptr(), None, s, st.ctypes.data)
    torch.cuda.synchronize()
    return rc, st, lbl.cpu().numpy()


@pytest.mark.parametrize("interp", ("bilinear", "bicubic"))
def test_failed_rows_between_good_ones(interp):
    """An empty cell and a LDT_IMG_TOO_LARGE row between good rows of every size, into a caller's buffer of 0xFF."""
    import torch

    from ldt_amd import _lib

    good = [(_cell(c[0], "420"), c[1:], _box(c)) for c in CASES]
    whole_c = (0, 0, 20, 300, 0)
    rows = good[:5] + [(b"", (4, 5), whole_c)] + good[5:10] + [(_cell("c", "420"), (20, 8), whole_c)] + good[10:]
    codes = {5: 1, 11: 4}  # LDT_IMG_NOT_JPEG; LDT_IMG_TOO_LARGE: ceil(300 / 8) = 38 > 37
    sizes = np.array([hw for _, hw, _ in rows], np.int32)
    offsets = 1 + np.concatenate([[0], np.cumsum(3 * sizes[:, 0].astype(np.int64) * sizes[:, 1])])
    flat = torch.full((int(offsets[-1]) + 1,), 0xFF, dtype=torch.uint8, device="cuda")
    labels = np.arange(len(rows), dtype=np.int64) + 9
    rc, st, lbl = _abi_call(_lib.get_context(0), [r[0] for r in rows], flat, offsets, sizes, interp, labels,
                            _lib.check_crops([r[2] for r in rows], len(rows)))
    assert rc == _lib.LDT_ERR_IMAGE and {i: int(s) for i, s in enumerate(st) if s} == codes
    host = flat.cpu().numpy()
    for i, (cell, hw, box) in enumerate(rows):
        region = host[offsets[i]:offsets[i + 1]]
        if i in codes:
            assert region.size and not region.any() and lbl[i] == -100, f"failed row {i}"
        else:
            _same(region.reshape(3, *hw), _pil(cell, hw, interp, box=box), f"row {i}")
            assert lbl[i] == labels[i]
    assert host[0] == 0xFF and host[-1] == 0xFF


@pytest.mark.parametrize("what", ("sizes-without-offsets", "n-differs", "region-size"))
def test_abi_refusals_leave_nothing_pending(what):
    import torch

    import ldt_amd
    from ldt_amd import _lib

    cells = [_cell("b", "420"), _cell("a", "444")]
    ctx = _lib.Context(0)
    sizes = np.array([[9, 20], [17, 40]], np.int32)
    offsets = np.concatenate([[0], np.cumsum(3 * sizes[:, 0].astype(np.int64) * sizes[:, 1])])
    flat = torch.full((int(offsets[-1]) + 8,), 0xFF, dtype=torch.uint8, device="cuda")
    if what == "sizes-without-offsets":
        offsets = None
    elif what == "n-differs":
        sizes = sizes[:1].copy()
    else:
        offsets = offsets + np.array([0, 0, 3])
    rc, _, _ = _abi_call(ctx, cells, flat, offsets, sizes)
    assert rc == _lib.LDT_ERR_ARG, (what, rc)
    assert flat.cpu().numpy().min() == 0xFF, "a refused call wrote to the output"
    # nothing stayed pending: the next plain native call stores what a plain call stores
    imgs, _ = ldt_amd.decode_native(cells[:1], ctx=ctx)
    torch.cuda.synchronize()
    _same(imgs[0], _pil(cells[0], (31, 33), "bilinear"), f"plain call after {what}")
