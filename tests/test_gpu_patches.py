"""GPU tests of ``decode_patches`` (ldt_decode_patches, k_resize_patches): every region bit for bit against Pillow's
resize followed by the numpy reshape / transpose of the Hugging Face Qwen2-VL image processor. The kernel's tile is
one block row (P * m pixel rows) by 252 (B = 14, 28) or 256 (B = 16, 32) columns; sources are 67 x 45, 33 x 31 and
300 x 20 (width x height), 4:2:0, 4:4:4 and grey in turn."""
import numpy as np
import pytest

from test_gpu_native_sizes import SRC, _cell, _pil

pytestmark = pytest.mark.gpu

# (P, m, T), memory_format, the rows' (h, w): one block; one block past a tile; several block rows; full tiles
SPECS = [((14, 2, 2), "contiguous", [(28, 28), (28, 280), (56, 28), (84, 532)]),
         ((16, 1, 1), "channels_last", [(16, 16), (16, 272), (48, 32)]),
         ((16, 2, 1), "contiguous", [(32, 288)])]
FORMATS = [("uint8", None), ("float32", True), ("bfloat16", None)]
KINDS = ("420", "444", "gray")


def _patches(x, spec, nhwc):
    """[3, h, w] -> [gh * gw, 3 * T * P * P], include/ldt.h's reshape and transpose."""
    (P, m, T), (C, h, w) = spec, x.shape
    X = np.stack([x] * T).reshape(1, T, C, h // P // m, m, P, w // P // m, m, P)
    X = X.transpose((0, 3, 6, 4, 7, 1, 5, 8, 2) if nhwc else (0, 3, 6, 4, 7, 2, 1, 5, 8))
    return np.ascontiguousarray(X.reshape((h // P) * (w // P), C * T * P * P))


def _bits(pil, dtype, norm):
    """The element bits the call stores for Pillow's bytes: F.to_tensor, F.normalize, then .to(dtype)."""
    import torch

    import ldt_amd

    if dtype == "uint8":
        return pil
    want = torch.from_numpy(pil).to(torch.float32).div(255)
    if norm:
        mean, std = (torch.tensor(v, dtype=torch.float32)[:, None, None]
                     for v in (ldt_amd.IMAGENET_MEAN, ldt_amd.IMAGENET_STD))
        want = want.sub_(mean).div_(std)
    return want.to(getattr(torch, dtype)).view(torch.int32 if dtype == "float32" else torch.int16).numpy()


def _rows(sizes):
    """(cell, box, draft, (h, w)) per row: the sizes over the sources in turn, then a crop at an odd origin with
    flip 1 and a row drafted by 2 (67 x 45 decodes to 34 x 23)."""
    rows = [(_cell("abc"[i % 3], KINDS[i % 3]), (0, 0, SRC["abc"[i % 3]][1], SRC["abc"[i % 3]][0], 0), 1, hw)
            for i, hw in enumerate(sizes)]
    a = _cell("a", "420")
    return rows + [(a, (7, 3, 31, 61, 1), 1, sizes[-1]), (a, (0, 0, 23, 34, 0), 2, sizes[0])]


@pytest.mark.parametrize("dtype, norm", FORMATS)
@pytest.mark.parametrize("interp", ("bilinear", "bicubic"))
@pytest.mark.parametrize("spec, mf, sizes", SPECS)
def test_patches(spec, mf, sizes, interp, dtype, norm):
    import torch

    import ldt_amd

    rows = _rows(sizes)
    labels = np.arange(len(rows), dtype=np.int64) + 3
    pv, grid, lbl = ldt_amd.decode_patches(
        [r[0] for r in rows], labels, sizes=[r[3] for r in rows], patch_size=spec[0], merge_size=spec[1],
        temporal_patch_size=spec[2], dtype=dtype, memory_format=mf, normalize=norm, interpolation=interp,
        crops=[r[1] for r in rows], drafts=[r[2] for r in rows])
    torch.cuda.synchronize()
    assert lbl.cpu().numpy().tolist() == labels.tolist()
    assert grid.cpu().numpy().tolist() == [[1, h // spec[0], w // spec[0]] for _, _, _, (h, w) in rows]
    assert pv.dtype == getattr(torch, dtype) and pv.shape[1] == 3 * spec[2] * spec[0] ** 2
    got = pv.cpu().view({"uint8": torch.uint8, "float32": torch.int32, "bfloat16": torch.int16}[dtype]).numpy()
    at = 0
    for i, (cell, box, draft, hw) in enumerate(rows):
        want = _patches(_bits(_pil(cell, hw, interp, draft, box), dtype, norm), spec, mf == "channels_last")
        part = got[at:at + len(want)]
        assert part.shape == want.shape and np.count_nonzero(part != want) == 0, (
            f"row {i} {hw}: {np.count_nonzero(part != want)} of {want.size} elements differ")
        at += len(want)
    assert at == len(got)


def test_a_bad_size_between_good_rows():
    """By hand: (30, 28) is no multiple of 28. That row alone fails, its region is zero, its neighbours are exact
    and the guard elements around the regions stay."""
    import ctypes

    import pyarrow as pa
    import torch

    from ldt_amd import _lib

    ctx, spec = _lib.get_context(0), _lib.LdtPatch(14, 2, 2, 0)
    cells = [_cell("b", "420"), _cell("a", "444"), _cell("c", "gray")]
    sizes = np.array([[28, 28], [30, 28], [28, 56]], np.int32)
    offsets = 1 + np.concatenate([[0], np.cumsum(6 * sizes[:, 0].astype(np.int64) * sizes[:, 1])])
    flat = torch.full((int(offsets[-1]) + 1,), 0xFF, dtype=torch.uint8, device="cuda")
    labels = np.array([4, 5, 6], np.int64)
    lbl = torch.full((3,), 55, dtype=torch.int64, device="cuda")
    bufs, st = pa.array(cells, pa.binary()).buffers(), np.zeros(3, np.int32)
    with ctx.lock:
        ctx.use_filter("bicubic")
        ctx.use_format("uint8", "contiguous")
        ctx.use_crops(None)
        ctx.use_native(offsets, sizes)
        rc = ctx.lib.ldt_decode_patches(ctx.handle, bufs[2].address, bufs[1].address, 0, 0, 3, None, labels.ctypes.data,
                                        0, flat.data_ptr(), lbl.data_ptr(), None, ctypes.byref(spec),
                                        torch.cuda.current_stream().cuda_stream, st.ctypes.data)
    torch.cuda.synchronize()
    assert rc == _lib.LDT_ERR_IMAGE and st.tolist() == [0, 7, 0]  # LDT_IMG_BAD_WINDOW
    host = flat.cpu().numpy()
    assert lbl.cpu().numpy().tolist() == [4, -100, 6]
    assert not host[offsets[1]:offsets[2]].any()
    for i in (0, 2):
        want = _patches(_pil(cells[i], tuple(sizes[i]), "bicubic"), (14, 2, 2), False)
        assert np.array_equal(host[offsets[i]:offsets[i + 1]].reshape(want.shape), want), f"row {i}"
    assert host[0] == 0xFF and host[-1] == 0xFF
