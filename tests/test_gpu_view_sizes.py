"""GPU tests of per-view output sizes: ``size=[(h, w), ...]`` (ldt_set_view_sizes),
several crops or windows of every image from a single decode, each view at its
own output size, against the oracle composition of tests/test_gpu_views.py
(its `_expected_view`, per output image (v, i) at ``size_v``). Max abs <= 2/255
is asserted first, then bit equality. The same views through single-size
``views=`` calls are a second cross-check.

Every decode_arrow call here writes into the middle of a flat buffer full of a
sentinel, and the guards on both sides must survive. The layout is checked by
cutting that buffer here, with the documented offsets: view v starts at element
``n * 3 * sum(h_u * w_u for u < v)``, image (v, i) ``i * 3 * h_v * w_v`` further.

Size lists: A the multi-crop shape (two runs); B the band edge 8 | 9, the tile
edge 256 | 257, two column tiles and a single pixel (five runs); C sixteen runs
of one; D one run; E a single view.
"""
import pickle

import numpy as np
import pytest

from conftest import read_golden
from test_gpu_views import (ES, SENTINEL, _arrow, _check_image, _expected_view, _hw, _hw_cache, _td, _view_crops,
                            mixed)  # noqa: F401  (mixed: the nine-cell fixture)

pytestmark = pytest.mark.gpu

A = [(224, 224)] * 2 + [(96, 96)] * 6
B = [(7, 5), (299, 260), (1, 1), (8, 256), (9, 257)]
C = [(32, 40), (16, 24)] * 8
D = [(64, 48)] * 3
E = [(40, 40)]


def _cut(flat, n, sizes, mf):
    """The per-view tensors [n, 3, h, w] of a flat output, by the documented offsets."""
    views, at = [], 0
    for h, w in sizes:
        piece = flat[at:at + n * 3 * h * w]
        views.append(piece.view(n, h, w, 3).permute(0, 3, 1, 2) if mf == "channels_last" else piece.view(n, 3, h, w))
        at += n * 3 * h * w
    assert at == flat.numel()
    return views


def _decode_sized(cells, sizes, crops=None, windows=None, dtype="float32", mf="contiguous", guard=4096, normalize=None,
                  **kw):
    """decode_arrow(size=sizes) into the middle of a byte buffer full of a
    sentinel. Returns (the V per-view CPU tensors [n, 3, h_v, w_v], labels,
    {failed row: status}, the tuple the call returned or None when it raised)."""
    import torch

    import ldt_amd
    from ldt_amd import transforms as T

    n = len(cells)
    nbytes = n * 3 * sum(h * w for h, w in sizes) * ES[dtype]
    buf = torch.full((guard + nbytes + guard,), SENTINEL, dtype=torch.uint8, device="cuda")
    flat = buf[guard:guard + nbytes].view(_td(dtype))
    lflat = torch.full((n + 2,), -777, dtype=torch.int64, device="cuda")
    labels = np.arange(100, 100 + n, dtype=np.int64)
    failed, runs = {}, None
    try:
        runs, _ = T.decode_arrow(_arrow(cells), labels, out=flat, out_lbl=lflat[1:n + 1], size=sizes,
                                 normalize=normalize, crops=crops, windows=windows, dtype=_td(dtype),
                                 memory_format=torch.channels_last if mf == "channels_last" else None, **kw)
    except ldt_amd.ImageDecodeError as e:
        failed = dict(e.rows)
    finally:
        torch.cuda.synchronize()
        assert torch.all(buf[:guard] == SENTINEL).item(), f"{sizes}: wrote before the output"
        assert torch.all(buf[guard + nbytes:] == SENTINEL).item(), f"{sizes}: wrote past the output"
        assert int(lflat[0]) == -777 and int(lflat[n + 1]) == -777
    views = _cut(flat, n, sizes, mf)
    if runs is not None:
        _check_runs(runs, views, n, sizes, mf)
    return [v.cpu() for v in views], lflat[1:n + 1].cpu().numpy(), failed, runs


def _run_list(sizes):
    runs = []
    for v, s in enumerate(sizes):
        if runs and runs[-1][2] == tuple(s):
            runs[-1][1] += 1
        else:
            runs.append([v, 1, tuple(s)])
    return runs


def _check_runs(runs, views, n, sizes, mf):
    """The returned tuple: one tensor per run of consecutive equal sizes,
    [V_run, n, 3, h, w], view-major and dense, each a view of the flat buffer."""
    want = _run_list(sizes)
    assert isinstance(runs, tuple) and len(runs) == len(want)
    for r, (first, count, (h, w)) in zip(runs, want):
        assert tuple(r.shape) == (count, n, 3, h, w)
        cell = 3 * h * w
        exp = (n * cell, cell, 1, 3 * w, 3) if mf == "channels_last" else (n * cell, cell, h * w, w, 1)
        assert all(r.stride(d) == exp[d] for d in range(5) if r.shape[d] > 1), (r.stride(), exp)
        assert r.data_ptr() == views[first].data_ptr()
        assert mf == "channels_last" or r.is_contiguous()


def _check_sized(cells, sizes, views, lbl, failed, what, crops=None, windows=None, dtype="float32", normalize=None,
                 interp="bilinear", other_failed=None):
    """Every output image (v, i) against `_expected_view` at size_v; a row's
    views are taken in order and the first that fails gives the row its status.
    Returns the number of exact rows."""
    import torch

    other_failed = other_failed or {}
    n, V = len(cells), len(sizes)
    assert len(views) == V
    want_failed, exact = {}, 0
    for i, (name, data) in enumerate(cells):
        exp = other_failed.get(i)
        if exp is None:
            exp = [_expected_view(name, data, tuple(sizes[v]), None if crops is None else crops[i][v],
                                  None if windows is None else windows[i][v], normalize, interp) for v in range(V)]
            exp = next((e for e in exp if isinstance(e, int)), exp)
        if isinstance(exp, int):
            want_failed[i] = exp
            for v in range(V):
                raw = views[v][i].contiguous().view(torch.uint8)
                assert not raw.any().item(), f"{what}: failed row {i} ({name}) view {v} is not all-zero bytes"
            assert lbl[i] == -100, f"{what}: failed row {i} label {lbl[i]}"
        else:
            for v in range(V):
                _check_image(views[v][i], exp[v], dtype, f"{what}: {name} view {v} -> {sizes[v]}")
            assert lbl[i] == 100 + i
            exact += 1
    assert failed == want_failed, f"{what}: failed rows {failed}, expected {want_failed}"
    return exact


def _windows(cells, sizes):
    """int32 [n, V, 4]: res = size_v + 32 + (3v, 2v) and an origin inside it.
    ceil(2 * 500 / res) <= 37 needs res >= 28 and res >= 33 here, so no view of
    the largest cell (375 x 500) passes the reduction limit under either filter."""
    return np.array([[[h + 32 + 3 * v, w + 32 + 2 * v, (5 * v + i) % (33 + 3 * v), (7 * v + 3 * i) % (33 + 2 * v)]
                      for v, (h, w) in enumerate(sizes)] for i in range(len(cells))], np.int32)


# ---- 1. the workload's shape -------------------------------------------------------------------------

def test_multi_crop_shape_with_crops_and_flips(mixed):
    import torch

    from ldt_amd import transforms as T

    crops = _view_crops(mixed, len(A))
    assert set(np.unique(crops[:, :, 4])) == {0, 1}
    views, lbl, failed, runs = _decode_sized(mixed, A, crops)
    assert _check_sized(mixed, A, views, lbl, failed, "A crops", crops=crops) == len(mixed)
    assert [tuple(r.shape) for r in runs] == [(2, 9, 3, 224, 224), (6, 9, 3, 96, 96)]
    # each run is what a single-size views= call gives
    arr = _arrow(mixed)
    g, _ = T.decode_arrow(arr, size=(224, 224), crops=np.ascontiguousarray(crops[:, :2]), views=2)
    l, _ = T.decode_arrow(arr, size=(96, 96), crops=np.ascontiguousarray(crops[:, 2:]), views=6)
    assert torch.equal(runs[0], g) and torch.equal(runs[1], l)
    assert torch.equal(runs[1].flatten(0, 1), torch.cat(list(l)))  # the torch.cat of the recipes


# ---- 2., 3. band and tile edges, sixteen runs, both grid orders ------------------------------------------

@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
@pytest.mark.parametrize("name,sizes", [("B", B), ("C", C)], ids=["B", "C"])
def test_crops_windows_and_flips_under_both_grid_orders(mixed, name, sizes, interp):
    import torch

    from ldt_amd import _lib

    crops, windows = _view_crops(mixed, len(sizes)), _windows(mixed, sizes)
    ctx = _lib.get_context(torch.cuda.current_device())
    outs = []
    for order in (0, 1):
        ctx.set_option(_lib.OPT_VIEW_ORDER, order)
        try:
            views, lbl, failed, _ = _decode_sized(mixed, sizes, crops, windows, interpolation=interp)
        finally:
            ctx.set_option(_lib.OPT_VIEW_ORDER, 0)
        exact = _check_sized(mixed, sizes, views, lbl, failed, f"{name} {interp} order {order}", crops=crops,
                             windows=windows, interp=interp)
        assert exact == 9 and not failed
        outs.append(views)
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 0  # the streaming kernel


def test_sixteen_runs_without_windows(mixed):
    # the smallest output edge is 16: ceil(500 / 24) = 21 and ceil(375 / 16) = 24, both <= 37
    views, lbl, failed, runs = _decode_sized(mixed, C)
    assert _check_sized(mixed, C, views, lbl, failed, "C plain") == 9 and len(runs) == 16


# ---- 4. one run, one view -----------------------------------------------------------------------------

def test_equal_sizes_and_a_single_view_equal_the_calls_of_today(mixed):
    import torch

    from ldt_amd import transforms as T

    arr, n = _arrow(mixed), len(mixed)
    crops = _view_crops(mixed, 3)
    _, _, failed, runs = _decode_sized(mixed, D, crops)
    want, _ = T.decode_arrow(arr, size=(64, 48), crops=crops, views=3)
    assert not failed and len(runs) == 1 and torch.equal(runs[0], want)
    # the whole output is today's [V, n, 3, h, w], byte for byte
    assert torch.equal(runs[0].reshape(-1).view(torch.uint8), want.reshape(-1).view(torch.uint8))
    # V = 1: the plain call at that size, with a box (the streaming kernel) and without (the band kernel)
    one = np.ascontiguousarray(crops[:, :1])
    _, _, failed, runs = _decode_sized(mixed, E, one)
    plain, _ = T.decode_arrow(arr, size=(40, 40), crops=np.ascontiguousarray(one[:, 0]))
    assert not failed and tuple(runs[0].shape) == (1, n, 3, 40, 40) and torch.equal(runs[0][0], plain)
    views, lbl, failed, runs = _decode_sized(mixed, E)
    plain, _ = T.decode_arrow(arr, size=(40, 40))
    assert not failed and torch.equal(runs[0][0], plain)
    assert _check_sized(mixed, E, views, lbl, failed, "E plain") == n


# ---- 5. formats ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,mf,normalize", [("bfloat16", "channels_last", None), ("uint8", "contiguous", None),
                                                ("float32", "contiguous", True)], ids=["bf16-nhwc", "u8", "f32-normalize"])
def test_formats_with_view_sizes(mixed, dtype, mf, normalize):
    crops, windows = _view_crops(mixed, len(B)), _windows(mixed, B)
    views, lbl, failed, runs = _decode_sized(mixed, B, crops, windows, dtype=dtype, mf=mf, normalize=normalize)
    n = len(mixed)
    assert len(runs) == 5
    for r, (h, w) in zip(runs, B):
        assert r.dtype == _td(dtype) and tuple(r.shape) == (1, n, 3, h, w)
        if mf == "channels_last":
            assert r.stride() == (n * 3 * h * w, 3 * h * w, 1, 3 * w, 3)
    exact = _check_sized(mixed, B, views, lbl, failed, f"B {dtype} {mf}", crops=crops, windows=windows, dtype=dtype,
                         normalize=normalize)
    assert exact == n and not failed


# ---- 6. failures --------------------------------------------------------------------------------------

def test_a_view_that_fails_at_its_own_size_fails_its_row_alone(mixed):
    cells = mixed + [("truncated", read_golden("jpeg/bad_truncated.bin")), ("null", None)]
    n, V = len(cells), len(B)
    _hw_cache["null"] = (1, 1)
    th, tw = _hw(*cells[9])
    crops = np.concatenate([_view_crops(mixed, V),
                            np.array([[[0, 0, min(th, 64), min(tw, 64), v & 1] for v in range(V)]], np.int32),
                            np.array([[[0, 0, 1, 1, 0]] * V], np.int32)])
    windows = _windows(cells, B)
    windows[2, 0] = windows[2, 1] = [20, 20, 3, 3]  # row 2: fits (7, 5) in view 0, not (299, 260) in view 1 -> 7
    crops[1, 0] = [0, 0, 375, 500, 0]               # row 1: the whole 375 x 500 image ...
    windows[1, 0] = [7, 5, 0, 0]                    # ... at (7, 5): reduced by 100 -> 4
    # that row's other views alone would pass
    assert all(not isinstance(_expected_view(*cells[1], tuple(B[v]), crops[1][v], windows[1][v]), int) for v in range(1, V))
    assert not isinstance(_expected_view(*cells[2], tuple(B[0]), crops[2][0], windows[2][0]), int)
    views, lbl, failed, runs = _decode_sized(cells, B, crops, windows)
    assert runs is None and failed == {1: 4, 2: 7, 9: 3, 10: 5}
    exact = _check_sized(cells, B, views, lbl, failed, "B failures", crops=crops, windows=windows,
                         other_failed={9: 3, 10: 5})
    assert exact == n - 4


# ---- 7. state -------------------------------------------------------------------------------------------

def test_sizes_are_consumed_and_errors_enqueue_nothing(mixed):
    import torch

    import ldt_amd
    from ldt_amd import _lib, synth
    from ldt_amd import transforms as T

    ctx = _lib.get_context(torch.cuda.current_device())
    arr, n = _arrow(mixed), len(mixed)
    plain = T.decode_arrow(arr, size=(30, 33))[0]
    before = ctx.output_size()
    assert before == (30, 33)
    runs, _ = T.decode_arrow(arr, size=D)
    assert ctx.output_size() == before  # the context's own size is not touched
    again = T.decode_arrow(arr, size=(30, 33))[0]  # and the next call without a list is plain
    assert tuple(again.shape) == (n, 3, 30, 33) and torch.equal(again, plain)
    hw = np.array(D, np.int32)
    # a call that fails on the host consumes the sizes: n crops where n * 3 are due
    flat = torch.full((4096 + n * 3 * 3 * 64 * 48 + 4096,), -12345.5, dtype=torch.float32, device="cuda")
    with ctx.lock:
        ctx.check(ctx.lib.ldt_set_view_sizes(ctx.handle, hw.ctypes.data, 3), "ldt_set_view_sizes")
    with pytest.raises(_lib.LdtError, match=r"rc=-1"):
        T.decode_arrow(arr, out=flat[4096:4096 + n * 3 * 30 * 33].view(n, 3, 30, 33), size=(30, 33),
                       crops=np.ascontiguousarray(_view_crops(mixed, 1)[:, 0]))
    torch.cuda.synchronize()
    assert torch.all(flat == -12345.5).item(), "a refused call wrote its output"
    assert torch.equal(T.decode_arrow(arr, size=(30, 33))[0], plain) and ctx.output_size() == before
    # views pending with another count: refused, both consumed
    with ctx.lock:
        ctx.check(ctx.lib.ldt_set_view_sizes(ctx.handle, hw.ctypes.data, 3), "ldt_set_view_sizes")
        ctx.check(ctx.lib.ldt_set_views(ctx.handle, 2), "ldt_set_views")
    with pytest.raises(_lib.LdtError, match=r"rc=-1"):
        T.decode_arrow(arr, out=flat[4096:4096 + n * 3 * 30 * 33].view(n, 3, 30, 33), size=(30, 33))
    torch.cuda.synchronize()
    assert torch.all(flat == -12345.5).item()
    assert torch.equal(T.decode_arrow(arr, size=(30, 33))[0], plain)
    # the same count pending is no contradiction
    assert torch.equal(T.decode_arrow(arr, size=D, views=3)[0][0], runs[0])
    # bad arguments are refused and change nothing
    bad_hw = np.array([[8, 8], [0, 8], [8, 1025]], np.int32)
    for ptr, cnt in ((hw.ctypes.data, 0), (hw.ctypes.data, 17), (hw.ctypes.data, -1), (None, 3),
                     (bad_hw.ctypes.data, 2), (bad_hw[1:].ctypes.data, 2)):
        assert ctx.lib.ldt_set_view_sizes(ctx.handle, ptr, cnt) == _lib.LDT_ERR_ARG
    assert torch.equal(T.decode_arrow(arr, size=(30, 33))[0], plain)
    # a wrong out= (shape, dtype, length): ValueError, nothing enqueued
    total = n * 3 * 3 * 64 * 48
    for bad in (torch.empty((3, n, 3, 64, 48), device="cuda"), torch.empty((total,), dtype=torch.float16, device="cuda"),
                torch.empty((total + 1,), device="cuda"), torch.empty((total - 1,), device="cuda"),
                torch.empty((2 * total,), device="cuda")[::2]):
        with pytest.raises(ValueError, match="out="):
            T.decode_arrow(arr, out=bad, size=D)
    # resize_raw: the Python layer refuses a list, the library refuses pending sizes and consumes them
    raw = torch.from_numpy(np.stack([synth.raw_hwc_one(33, 47, 61 + k) for k in range(3)]))
    want = ldt_amd.resize_raw(raw, 33, 47, size=(30, 33))
    with pytest.raises(ValueError, match="size list"):
        ldt_amd.resize_raw(raw, 33, 47, size=D)
    with ctx.lock:
        ctx.check(ctx.lib.ldt_set_view_sizes(ctx.handle, hw.ctypes.data, 3), "ldt_set_view_sizes")
    with pytest.raises(_lib.LdtError, match=r"rc=-1"):
        ldt_amd.resize_raw(raw, 33, 47, size=(30, 33))
    assert torch.equal(ldt_amd.resize_raw(raw, 33, 47, size=(30, 33)), want)
    assert torch.equal(T.decode_arrow(arr, size=(30, 33))[0], plain)


def test_grid_limit_of_a_size_list_is_refused_not_overflowed():
    """16 views of 1024 x 1024 are 8192 workgroups per image: 2^31 at n = 2^18.
    The refusal is reached without allocating an output for it."""
    import torch

    from ldt_amd import _lib

    ctx = _lib.Context(torch.cuda.current_device())
    hw = np.full((16, 2), 1024, np.int32)
    offsets = np.zeros(2, np.int64)
    data = np.zeros(8, np.uint8)
    status = np.zeros(1, np.int32)
    out = torch.zeros(16, device="cuda")
    for n in (1 << 18, (1 << 31) // 16 + 8):
        ctx.check(ctx.lib.ldt_set_view_sizes(ctx.handle, hw.ctypes.data, 16), "ldt_set_view_sizes")
        rc = ctx.lib.ldt_decode_batch_large(ctx.handle, data.ctypes.data, offsets.ctypes.data, 0, n, None, None, 0,
                                            out.data_ptr(), None, None, None, status.ctypes.data)
        assert rc == _lib.LDT_ERR_ARG
        assert b"workgroups" in ctx.lib.ldt_last_error(ctx.handle)
    assert ctx.output_size() == (224, 224)


# ---- 8. surfaces --------------------------------------------------------------------------------------

SCALES = [(0.4, 1.0)] * 2 + [(0.05, 0.4)] * 6


def _same(got, want, what):
    import torch

    assert isinstance(got, tuple) and len(got) == len(want), what
    for g, w in zip(got, want):
        assert tuple(g.shape) == tuple(w.shape) and g.dtype == w.dtype, what
        assert torch.equal(g, w), f"{what}: differs from decode_arrow with the same boxes"


def test_every_surface_gives_the_tuple(mixed):
    import pyarrow as pa
    import torch

    import ldt_amd
    from ldt_amd import transforms as T

    n = len(mixed)
    arr = _arrow(mixed)
    rb = pa.RecordBatch.from_arrays([arr, pa.array(np.arange(100, 100 + n), pa.int64())], names=["image", "label"])
    images = [d for _, d in mixed]
    items = [{"image": d, "label": 100 + k} for k, d in enumerate(images)]
    wh, st = ldt_amd.image_sizes(arr)
    draw = ldt_amd.RandomResizedCropFlip(scale=SCALES, generator=torch.Generator().manual_seed(31))
    first, second = draw.sample(wh, st, views=8), draw.sample(wh, st, views=8)
    assert first.shape == (n, 8, 5) and not np.array_equal(first, second)
    want = [T.decode_arrow(arr, size=A, crops=b)[0] for b in (first, second)]
    assert [tuple(t.shape) for t in want[0]] == [(2, n, 3, 224, 224), (6, n, 3, 96, 96)]

    def sampler():
        return ldt_amd.RandomResizedCropFlip(scale=SCALES, generator=torch.Generator().manual_seed(31))

    res = ldt_amd.ResidentBatch(images, np.arange(100, 100 + n))
    img, lbl = res.decode(size=A, crops=sampler())
    _same(img, want[0], "ResidentBatch.decode")
    assert lbl.cpu().tolist() == list(range(100, 100 + n))
    got = ldt_amd.collate_fn(items, size=A, crop=sampler())
    _same(got["image"], want[0], "collate_fn")
    assert all(isinstance(t, T.DeviceTensor) for t in got["image"]) and got["label"].cpu().tolist() == list(range(100, 100 + n))
    fn = pickle.loads(pickle.dumps(ldt_amd.make_collate_fn(size=A, crop=second)))
    _same(fn(items)["image"], want[1], "a pickled make_collate_fn")
    _same(ldt_amd.decode_tensor_image(rb, size=A, crop=first)["image"], want[0], "decode_tensor_image")
    batch = T.DeviceBatch(T._pack_list(images, list(range(100, 100 + n))), size=A, crop=sampler())
    _same(batch["image"], want[0], "DeviceBatch")
    batch = pickle.loads(pickle.dumps(T.DeviceBatch(T._pack_list(images, None), size=A, crop=second))).pin_memory()
    _same(batch["image"], want[1], "a pickled DeviceBatch")
    # the pipeline: the generator moves on between the batches
    pipe = ldt_amd.DecodePipeline(depth=2, size=A, crop=sampler())
    assert pipe.views == 8
    a, b = pipe.decode(rb), pipe.decode(res)
    pipe.check()
    torch.cuda.synchronize()
    _same(a[0], want[0], "DecodePipeline batch 0")
    _same(b[0], want[1], "DecodePipeline batch 1 (resident)")
    img, lbl, ready = pipe.decode(rb, crops=first, wait=False)
    ready()
    torch.cuda.synchronize()
    _same(img, want[0], "DecodePipeline wait=False")
    with pytest.raises(ValueError):
        ldt_amd.DecodePipeline(size=A, views=2)
    fn = ldt_amd.make_to_tensor_fn(depth=2, size=A, crop=sampler(), prefetch=1)
    outs = list(fn.iterate([rb, rb]))
    for k in range(2):
        _same(outs[k]["image"], want[k], f"make_to_tensor_fn iterate {k}")
        assert all(isinstance(t, T.DeviceTensor) for t in outs[k]["image"])
    got = ldt_amd.make_to_tensor_fn(depth=2, size=A)(rb, crop=second)
    _same(got["image"], want[1], "make_to_tensor_fn")
