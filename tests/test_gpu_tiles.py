"""GPU tests of ``decode_tiles`` (ldt_decode_tiles, k_resize_tiles): every tile bit for bit against Pillow's resize
pasted on a filled canvas and cut into squares, the thumbnail after them. A workgroup serves TR (8 or 16) rows by
one column chunk of one output tile: S = 20 is one chunk, S = 260 two (256 and 4, or 130 each under the even split)."""
import numpy as np
import pytest

import call_kinds
from test_gpu_native_sizes import _pil
from test_gpu_patches import _bits

pytestmark = pytest.mark.gpu

GRIDS = [(1, 1), (3, 1), (1, 3), (2, 2), (2, 3)]
FORMATS = [("uint8", None, "contiguous"), ("float32", None, "contiguous"), ("bfloat16", True, "channels_last")]
VIEW = {"uint8": "uint8", "float32": "int32", "bfloat16": "int16"}


def _want(cell, g, S, interp, thumbnail, fill=(0, 0, 0), box=None, draft=1):
    """[T, 3, S, S] uint8: include/ldt.h's canvas, tiles and thumbnail from Pillow's resizes."""
    rows, cols = g[:2]
    rh, rw, top, left = g[2:] if len(g) == 6 else (rows * S, cols * S, 0, 0)
    canvas = np.empty((3, rows * S, cols * S), np.uint8)
    canvas[:] = np.array(fill, np.uint8)[:, None, None]
    canvas[:, top:top + rh, left:left + rw] = _pil(cell, (rh, rw), interp, draft, box)
    tiles = [canvas[:, a * S:(a + 1) * S, b * S:(b + 1) * S] for a in range(rows) for b in range(cols)]
    if thumbnail and rows * cols > 1:
        tiles.append(_pil(cell, (S, S), interp, draft, box))
    return np.stack(tiles)


def _check(rows, S, interp, thumbnail=True, fmt=FORMATS[0], fill=0, crops=False, **kw):
    """rows: (cell, grid, box or None, draft). One call; every row's region against _want."""
    import torch

    import ldt_amd

    dtype, norm, mf = fmt
    labels = np.arange(len(rows), dtype=np.int64) + 3
    if crops:
        kw.update(crops=[r[2] for r in rows], drafts=[r[3] for r in rows])
    pv, num, lbl = ldt_amd.decode_tiles([r[0] for r in rows], labels, grids=[r[1] for r in rows], tile_size=S,
                                        thumbnail=thumbnail, fill=fill, dtype=dtype, normalize=norm, memory_format=mf,
                                        interpolation=interp, **kw)
    torch.cuda.synchronize()
    assert lbl.cpu().numpy().tolist() == labels.tolist()
    assert pv.dtype == getattr(torch, dtype) and pv.shape[1:] == (3, S, S)
    assert mf == "contiguous" or pv.is_contiguous(memory_format=torch.channels_last)
    got, at, counts = pv.cpu().view(getattr(torch, VIEW[dtype])).numpy(), 0, []
    rgb = (fill,) * 3 if isinstance(fill, int) else fill
    for i, (cell, g, box, draft) in enumerate(rows):
        want = _bits(_want(cell, g, S, interp, thumbnail, rgb, box, draft), dtype, norm)
        part = got[at:at + len(want)]
        assert part.shape == want.shape and np.count_nonzero(part != want) == 0, (
            f"row {i} grid {g}: {np.count_nonzero(part != want)} of {want.size} elements differ")
        at += len(want)
        counts.append(len(want))
    assert at == len(got) and num.cpu().numpy().tolist() == counts
    return pv


@pytest.mark.parametrize("thumbnail", (True, False))
@pytest.mark.parametrize("fmt", FORMATS, ids=[f[0] for f in FORMATS])
@pytest.mark.parametrize("interp", ("bilinear", "bicubic"))
def test_one_chunk(interp, fmt, thumbnail):
    """S = 20, no multiple of 8: all five cells under every grid."""
    _check([(c, g, None, 1) for c, _ in call_kinds.cells() for g in GRIDS], 20, interp, thumbnail, fmt)


def test_two_chunks():
    """S = 260: a chunk edge inside a tile, 33 bands of 8 rows (the last of 4)."""
    cells = [call_kinds.cells()[k][0] for k in (0, 2, 3)]
    _check([(c, g, None, 1) for c in cells for g in ((1, 2), (2, 1))], 260, "bicubic")


@pytest.mark.parametrize("flip", (0, 1))
@pytest.mark.parametrize("interp", ("bilinear", "bicubic"))
def test_placement(interp, flip):
    """res smaller than the canvas at (0, 0) and at odd centred offsets; a row whose last two tiles are all fill."""
    data = call_kinds.cells()
    grids = [(2, 2, 31, 27, 0, 0), (2, 3, 25, 33, 7, 13), (1, 3, 20, 17, 0, 0), (3, 1, 9, 20, 25, 0), (1, 1, 11, 5, 3, 9)]
    rows = [(c, g, (0, 0, rgb.shape[0], rgb.shape[1], flip), 1) for (c, rgb), g in zip(data, grids)]
    _check(rows, 20, interp, fill=(7, 130, 255), crops=True)


def test_crops_and_a_draft():
    """Boxes at odd origins, flip on odd rows, and a draft of 2 on the 48 x 64 cell (24 x 32 decoded)."""
    data = call_kinds.cells()
    rows = [(data[0][0], (2, 2), (5, 3, 41, 57, 0), 1), (data[2][0], (1, 3), (7, 9, 61, 53, 1), 1),
            (data[0][0], (2, 3), (1, 1, 21, 29, 0), 2), (data[3][0], (3, 1), (3, 11, 59, 33, 1), 1)]
    _check(rows, 20, "bicubic", crops=True)


def test_abi_a_failed_row_and_a_wrong_length():
    """By hand: a truncated cell between good rows, into 0xFF. Its region is zero, its label -100, its neighbours
    exact, the bytes past the last region untouched; a region three elements too long is LDT_ERR_ARG, nothing written."""
    import ctypes

    import pyarrow as pa
    import torch

    from conftest import read_golden
    from ldt_amd import _lib

    ctx, good = _lib.get_context(0), call_kinds.cells()
    cells = [good[0][0], read_golden("jpeg/bad_truncated.bin"), good[2][0]]
    spec, sizes, grid = _lib.check_tiles([(2, 2), (1, 2), (1, 3)], 3, 20, True, 0)
    num, offsets = _lib.tile_layout(grid, spec)
    labels, bufs = np.array([4, 5, 6], np.int64), pa.array(cells, pa.binary()).buffers()

    def call(offsets):
        flat = torch.full((int(offsets[-1]) + 5,), 0xFF, dtype=torch.uint8, device="cuda")
        lbl, st = torch.full((3,), 55, dtype=torch.int64, device="cuda"), np.zeros(3, np.int32)
        with ctx.lock:
            ctx.use_filter("bicubic")
            ctx.use_format("uint8", "contiguous")
            ctx.use_crops(None)
            ctx.use_native(offsets, sizes)
            rc = ctx.lib.ldt_decode_tiles(ctx.handle, bufs[2].address, bufs[1].address, 0, 0, 3, None,
                                          labels.ctypes.data, 0, flat.data_ptr(), lbl.data_ptr(), None,
                                          ctypes.byref(spec), grid.ctypes.data,
                                          torch.cuda.current_stream().cuda_stream, st.ctypes.data)
        torch.cuda.synchronize()
        return rc, st.tolist(), flat.cpu().numpy(), lbl.cpu().numpy().tolist()

    rc, st, host, lbl = call(offsets)
    assert rc == _lib.LDT_ERR_IMAGE and st[0] == 0 and st[1] != 0 and st[2] == 0
    assert lbl == [4, -100, 6] and not host[offsets[1]:offsets[2]].any() and (host[offsets[3]:] == 0xFF).all()
    for i, g in ((0, (2, 2)), (2, (1, 3))):
        assert np.array_equal(host[offsets[i]:offsets[i + 1]], _want(cells[i], g, 20, "bicubic", True).ravel()), f"row {i}"
    longer = offsets.copy()
    longer[3] += 3
    rc, _, host, lbl = call(longer)
    assert rc == _lib.LDT_ERR_ARG and (host == 0xFF).all() and lbl == [55, 55, 55]


def test_sequence_on_one_context():
    """decode_native(sizes=), decode_tiles, then a plain decode_arrow on one context: each its fresh-context bytes."""
    import pyarrow as pa
    import torch

    import ldt_amd
    from ldt_amd import _lib

    cells = [c for c, _ in call_kinds.cells()[:4]]
    calls = [lambda ctx: ldt_amd.decode_native(cells, sizes=[(30, 40)] * 4, interpolation="bicubic", ctx=ctx)[0],
             lambda ctx: [ldt_amd.decode_tiles(cells, grids=[(2, 3)] * 4, tile_size=20, dtype="uint8",
                                               interpolation="bicubic", ctx=ctx)[0]],
             lambda ctx: [ldt_amd.decode_arrow(pa.array(cells, pa.binary()), ctx=ctx)[0]]]
    shared = _lib.Context(0)
    for k, call in enumerate(calls):
        got, fresh = call(shared), call(_lib.Context(0))
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, fresh)), f"call {k}"
