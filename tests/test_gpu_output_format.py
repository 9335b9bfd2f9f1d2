"""dtype= and memory_format= on the GPU: the resize kernels' formatted store
(ldt_set_output_format) in every dtype x layout, against the existing
expectations (tests/test_gpu_interpolation.py ``_expected``: the oracle's
bilinear and Pillow's bicubic tensors, windows, boxes, flip and the failure
statuses) converted on the CPU as the semantics say: ``ref32.to(dtype)`` for
fp16 / bf16, ``rint(ref32 * 255)`` of the un-normalised tensor for uint8, the
same values at the same indices with strides ``(3*h*w, 1, 3*w, 3)`` for
channels_last.

Every guarded decode goes into the middle of a larger byte buffer full of a
sentinel: a narrow output written with a wide store would overrun it. The
assertions come in the order tolerance (2/255 plus the type's half-ulp at the
value; 2 levels for uint8), bit equality, strides.
"""
import numpy as np
import pyarrow as pa
import pytest

from oracle import oracle
from test_gpu_interpolation import _corner_windows, _expected, _odd_boxes, _pil_window
from test_gpu_window import _ID, _hw, mixed  # noqa: F401
from test_interpolation import checkerboard

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "float16", "bfloat16", "uint8")
LAYOUTS = ("contiguous", "channels_last")
FORMATS = [(d, m) for d in DTYPES for m in LAYOUTS]
ES = {"float32": 4, "float16": 2, "bfloat16": 2, "uint8": 1}
SENTINEL = 0xA5
TOL = 2.0 / 255.0
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))

# the sizes at which the store can go wrong
STORE_SIZES = [(224, 224),          # the fixed band kernel
               (7, 5), (3, 2),      # odd cells: images 1.. start off every vector alignment
               (30, 33),            # ow % 4 != 0: the last group is cut
               (8, 256),            # the widest band-kernel output
               (5, 300),            # streaming, two column tiles, the second 44 wide
               (1, 9), (9, 1)]      # the stride rule


def _td(dtype):
    import torch

    return {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16, "uint8": torch.uint8}[dtype]


def _strides(size, mf):
    h, w = size
    return (3 * h * w, 1, 3 * w, 3) if mf == "channels_last" else (3 * h * w, h * w, w, 1)


def _convert(exp32, dtype):
    """The float32 expectation [3, h, w] in the output's dtype, on the CPU."""
    import torch

    if dtype == "uint8":
        return torch.from_numpy(np.rint(exp32.astype(np.float64) * 255.0).astype(np.uint8))
    return torch.from_numpy(np.ascontiguousarray(exp32)).to(_td(dtype))


def _half_ulp(x, dtype):
    """Half a unit in the last place of `dtype` at each float32 value of x."""
    if dtype == "float32":
        return np.zeros_like(x, dtype=np.float64)
    _, e = np.frexp(np.abs(x).astype(np.float64))  # |x| = m * 2^e, m in [0.5, 1): the leading bit is 2^(e - 1)
    if dtype == "float16":
        return np.ldexp(1.0, np.maximum(e - 1 - 10, -24) - 1)  # 10 mantissa bits, subnormal spacing 2^-24
    return np.ldexp(1.0, e - 1 - 7 - 1)  # bfloat16: 7 mantissa bits


def _check_row(got, exp32, dtype, what, normalized=False):
    """got: the row as a CPU tensor [3, h, w] of the dtype, any strides."""
    import torch

    assert got.dtype == _td(dtype) and tuple(got.shape) == exp32.shape, (what, got.dtype, tuple(got.shape))
    want = _convert(exp32, dtype)
    got = got.contiguous()
    if dtype == "uint8":
        assert not normalized
        d = np.abs(got.numpy().astype(np.int32) - want.numpy().astype(np.int32))
        assert d.max() <= 2, f"{what}: {d.max()} levels off"
        assert torch.equal(got, want), f"{what}: not the resized byte ({np.count_nonzero(d)} differ, max {d.max()})"
        return
    d = np.abs(got.to(torch.float64).numpy() - exp32.astype(np.float64))
    lim = TOL + _half_ulp(exp32, dtype)
    assert np.all(d <= lim), f"{what}: max abs {d.max()} over 2/255 + half an ulp"
    if dtype == "float32":
        assert np.array_equal(got.numpy().view(np.uint32), exp32.view(np.uint32)), f"{what}: not bit-exact"
    else:
        g, w = got.view(torch.int16), want.view(torch.int16)
        assert torch.equal(g, w), f"{what}: not ref32.to({dtype}) bit for bit ({int((g != w).sum())} differ)"


def _guarded(n, size, dtype, mf, off=0, guard=4096):
    """(byte buffer, the output view in its middle, off bytes past a 16-byte boundary)."""
    import torch

    h, w = size
    nbytes = n * 3 * h * w * ES[dtype]
    buf = torch.full((guard + off + nbytes + guard,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0 and off % ES[dtype] == 0
    flat = buf[guard + off:guard + off + nbytes].view(_td(dtype))
    out = flat.view(n, h, w, 3).permute(0, 3, 1, 2) if mf == "channels_last" else flat.view(n, 3, h, w)
    assert out.data_ptr() == buf.data_ptr() + guard + off and out.stride() == _strides(size, mf)
    return buf, out, (guard + off, guard + off + nbytes)


def _guards_intact(buf, span, what):
    import torch

    torch.cuda.synchronize()
    assert torch.all(buf[:span[0]] == SENTINEL).item(), f"{what}: wrote before the output"
    assert torch.all(buf[span[1]:] == SENTINEL).item(), f"{what}: wrote past the output"


def _decode(cells, size, dtype, mf, off=0, **kw):
    """decode_arrow into a guarded byte buffer. Returns (image on the CPU with
    the output's strides, labels, {failed row: status})."""
    import torch

    import ldt_amd
    from ldt_amd import transforms as T

    n = len(cells)
    buf, out, span = _guarded(n, size, dtype, mf, off)
    lflat = torch.full((n + 2,), -777, dtype=torch.int64, device="cuda")
    failed = {}
    try:
        T.decode_arrow(pa.array([d for _, d in cells], pa.binary()), np.arange(100, 100 + n, dtype=np.int64), out=out,
                       out_lbl=lflat[1:n + 1], size=size, dtype=dtype, memory_format=mf, **kw)
    except ldt_amd.ImageDecodeError as e:
        failed = dict(e.rows)
    finally:
        _guards_intact(buf, span, f"{size} {dtype} {mf}")
        assert int(lflat[0]) == -777 and int(lflat[n + 1]) == -777
    img = out.cpu()
    assert img.stride() == _strides(size, mf) or n == 1
    return img, lflat[1:n + 1].cpu().numpy(), failed


def _check_batch(cells, size, dtype, mf, img, lbl, failed, what, windows=None, crops=None, normalize=None,
                 interp="bilinear", other_failed=None):
    other_failed = other_failed or {}
    want_failed, exact = {}, 0
    for k, (name, data) in enumerate(cells):
        exp = other_failed[k] if k in other_failed else \
            _expected(name, data, size, None if windows is None else windows[k], None if crops is None else crops[k],
                      normalize, interp)
        w = f"{what} {dtype} {mf} {size}: row {k} ({name})"
        if isinstance(exp, int):
            want_failed[k] = exp
            assert not img[k].contiguous().view(-1).view(_td("uint8")).any(), f"{w}: a failed row is not all-zero bytes"
            assert lbl is None or lbl[k] == -100, f"{w}: label {lbl[k]}"
        else:
            _check_row(img[k], exp, dtype, w, normalized=bool(normalize))
            assert lbl is None or lbl[k] == 100 + k
            exact += 1
    assert failed == want_failed, f"{what} {dtype} {mf} {size}: failed rows {failed}, expected {want_failed}"
    return exact


def _ctx():
    import torch

    from ldt_amd import _lib

    return _lib.get_context(torch.cuda.current_device()), _lib


# ---- 1. dtype x layout over the sizes where the store can go wrong, on each kernel ---------------

@pytest.fixture(scope="module")
def small(mixed):
    """Cells narrow enough for the band kernel (at most 11 horizontal taps: a
    source up to 5 x out_w wide) at the small output sizes too, where every
    wider cell of `mixed` takes the streaming kernel or fails."""
    from ldt_amd import synth

    by = dict(mixed)
    return [("440-17x5", by["440-17x5"]), ("up-8x8", by["up-8x8"]),
            ("444-6x10", synth.encode(synth.field(6, 10, 211, 6.0), subsampling="4:4:4")),
            ("420-12x9", synth.encode(synth.field(12, 9, 212, 6.0))),
            ("420-20x10", synth.encode(synth.field(20, 10, 213, 6.0), quality=90))]


def _band_serves(cells, size):
    """Whether the band kernel takes the batch: out_w <= 256, at most 11
    horizontal taps for the widest cell, and no row over the reduction limit."""
    hw = [_hw(*c) for c in cells]
    if any(-(-h // size[0]) > 37 or -(-w // size[1]) > 37 for h, w in hw):
        return None  # a failed row: either kernel may have served the rest
    return size[1] <= 256 and 2 * -(-max(w for _, w in hw) // size[1]) + 1 <= 11


@pytest.mark.parametrize("impl", [0, 2, 3], ids=["default", "streaming", "generic-band"])
@pytest.mark.parametrize("size", STORE_SIZES, ids=_ID)
def test_every_format_at_every_store_size(mixed, small, size, impl):
    import torch

    from ldt_amd import transforms as T

    ctx, _lib = _ctx()
    ctx.set_option(_lib.OPT_RESIZE_IMPL, impl)
    try:
        for cells, which in ((mixed, "mixed"), (small, "small")):
            arr = pa.array([d for _, d in cells], pa.binary())
            for dtype, mf in FORMATS:
                img, lbl, failed = _decode(cells, size, dtype, mf)
                band = _band_serves(cells, size)
                if band is not None:
                    assert (ctx.lib.ldt_debug_last_resize(ctx.handle) > 0) == (band and impl != 2), (which, dtype, mf)
                exact = _check_batch(cells, size, dtype, mf, img, lbl, failed, f"{which}, impl {impl}")
                assert exact == len(cells) - len(failed) and set(failed.values()) <= {4}
                # the library's own allocation (of the rows that decode): the same bytes, the exact strides
                ok = [k for k in range(len(cells)) if k not in failed]
                own = T.decode_arrow(arr.take(pa.array(ok)), size=size, dtype=dtype, memory_format=mf)[0]
                assert own.dtype == _td(dtype) and tuple(own.shape) == (len(ok), 3) + size
                assert own.stride() == _strides(size, mf), (own.stride(), size, mf)
                assert torch.equal(own.cpu().contiguous().view(torch.uint8), img[ok].contiguous().view(torch.uint8))
    finally:
        ctx.set_option(_lib.OPT_RESIZE_IMPL, 0)


def test_the_small_cells_meet_the_band_kernel_where_the_store_can_go_wrong(mixed, small):
    served = {size: _band_serves(small, size) for size in STORE_SIZES}
    assert all(served[s] for s in ((224, 224), (7, 5), (3, 2), (30, 33), (8, 256), (1, 9))), served
    assert _band_serves(mixed, (224, 224)) and _band_serves(mixed, (30, 33)) is False


# ---- 2. a misaligned out= ----------------------------------------------------------------------

@pytest.mark.parametrize("size", [(8, 8), (224, 224)], ids=_ID)
@pytest.mark.parametrize("dtype,off", [("uint8", 1), ("bfloat16", 2)])
def test_out_off_every_vector_alignment(mixed, small, size, dtype, off):
    ctx, _lib = _ctx()
    cells = mixed if size == (224, 224) else small  # each on the band kernel at that size
    assert _band_serves(cells, size)
    for mf in LAYOUTS:
        for impl in (0, 2):
            ctx.set_option(_lib.OPT_RESIZE_IMPL, impl)
            try:
                img, lbl, failed = _decode(cells, size, dtype, mf, off=off)
                assert (ctx.lib.ldt_debug_last_resize(ctx.handle) > 0) == (impl == 0)
            finally:
                ctx.set_option(_lib.OPT_RESIZE_IMPL, 0)
            assert _check_batch(cells, size, dtype, mf, img, lbl, failed, f"out= {off} bytes off, impl {impl}") \
                == len(cells) and not failed


# ---- 3. compositions ---------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(7, 5), (30, 33)], ids=_ID)
@pytest.mark.parametrize("dtype,mf", [("bfloat16", "channels_last"), ("uint8", "contiguous")])
def test_compositions(mixed, size, dtype, mf):
    n = len(mixed)
    crops = _odd_boxes(mixed)
    assert set(crops[:, 4].tolist()) == {0, 1}
    corners = _corner_windows(n, size)
    cases = [("boxes + flip", dict(crops=crops)), ("corner windows", dict(windows=corners)),
             ("boxes + windows", dict(crops=crops, windows=corners)),
             ("bicubic", dict(interpolation="bicubic")),
             ("bicubic boxes + windows", dict(crops=crops, windows=corners, interpolation="bicubic"))]
    if dtype != "uint8":
        cases += [("ImageNet", dict(normalize=True)),
                  ("ImageNet boxes + windows", dict(normalize=True, crops=crops, windows=corners))]
    total = 0
    for what, kw in cases:
        img, lbl, failed = _decode(mixed, size, dtype, mf, **kw)
        exact = _check_batch(mixed, size, dtype, mf, img, lbl, failed, what, windows=kw.get("windows"),
                             crops=kw.get("crops"), normalize=kw.get("normalize"),
                             interp=kw.get("interpolation", "bilinear"))
        assert exact == n - len(failed) and set(failed.values()) <= {4}, (what, failed)
        total += exact
    assert total >= len(cases) * (n - 2)


# ---- 4. failed rows ----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,mf", FORMATS, ids=[f"{d}-{m}" for d, m in FORMATS])
def test_failed_rows_are_zero_bytes_among_exact_neighbours(mixed, dtype, mf):
    by = dict(mixed)
    good = ["420-48x64", "gray-77x91", "prog-64x80", "440-17x5", "up-8x8"]
    cut = by["420-48x64"][:len(by["420-48x64"]) // 2]
    cells = [(good[0], by[good[0]]), ("null", None), (good[1], by[good[1]]), ("cut", cut), (good[2], by[good[2]]),
             (good[3], by[good[3]]), (good[4], by[good[4]]), (good[0], by[good[0]])]
    ctx, _lib = _ctx()
    # (7, 5): these sources take the streaming kernel there, whose failed rows k_fill_failed zeroes;
    # (30, 33): the band kernel, which zeroes its failed rows itself
    for size in ((7, 5), (30, 33)):
        # as today: the statuses of the float32 call
        _, _, today = _decode(cells, size, "float32", "contiguous")
        assert (ctx.lib.ldt_debug_last_resize(ctx.handle) > 0) == (size == (30, 33))
        assert today[1] == 5 and set(today) == {1, 3} and today[3] != 0
        for impl in (0, 2):
            ctx.set_option(_lib.OPT_RESIZE_IMPL, impl)
            try:
                img, lbl, failed = _decode(cells, size, dtype, mf)
            finally:
                ctx.set_option(_lib.OPT_RESIZE_IMPL, 0)
            assert failed == today
            assert _check_batch(cells, size, dtype, mf, img, lbl, failed, f"failed rows, impl {impl}",
                                other_failed=today) == 6
    size = (7, 5)
    # a bad box and a bad window among them (the streaming kernel)
    crops = np.array([[0, 0, *_hw(nm, d), 0] if d is not None and nm != "cut" else [0, 0, 1, 1, 0] for nm, d in cells],
                     np.int32)
    windows = np.array([[size[0] + 3, size[1] + 4, 1, 2]] * len(cells), np.int32)
    crops[2] = [0, 0, 78, 91, 0]             # top + height == H + 1
    windows[4] = [size[0] + 3, size[1] + 4, 4, 0]  # not inside res
    img, lbl, failed = _decode(cells, size, dtype, mf, crops=crops, windows=windows)
    assert failed == {1: 5, 2: 6, 3: today[3], 4: 7}
    assert _check_batch(cells, size, dtype, mf, img, lbl, failed, "bad box and window", windows=windows, crops=crops,
                        other_failed={1: 5, 3: today[3]}) == 4


# ---- 5. raw sources ----------------------------------------------------------------------------

@pytest.mark.parametrize("case", [((17, 5), (30, 33)), ((64, 80), (224, 224))], ids=["17x5-30x33", "64x80-224x224"])
def test_resize_raw_in_every_format(case):
    import torch

    import ldt_amd

    (h, w), size = case
    raw = np.stack([checkerboard(h, w, 300 + k) for k in range(3)])
    ctx, _lib = _ctx()
    exps = {}
    for impl in (0, 2):
        ctx.set_option(_lib.OPT_RESIZE_IMPL, impl)
        try:
            for src in (torch.from_numpy(raw), torch.from_numpy(raw).cuda()):
                for dtype, mf in FORMATS:
                    for normalize in ((False,) if dtype == "uint8" else (False, True)):
                        out = ldt_amd.resize_raw(src, h, w, normalize=normalize, size=size, dtype=dtype, memory_format=mf)
                        assert out.dtype == _td(dtype) and tuple(out.shape) == (3, 3) + size
                        assert out.stride() == _strides(size, mf)
                        got = out.cpu()
                        for k in range(3):
                            if (k, normalize) not in exps:
                                exps[k, normalize] = oracle.raw_to_tensor(raw[k], *size, normalize=normalize or None)
                            exp = exps[k, normalize]
                            _check_row(got[k], exp, dtype, f"raw {src.device} impl {impl} {dtype} {mf} norm={normalize} "
                                                           f"row {k}", normalized=normalize)
        finally:
            ctx.set_option(_lib.OPT_RESIZE_IMPL, 0)
    # boxes, windows and bicubic on the raw path, in one narrow format
    boxes = np.array([[1, 1, h - 2, w - 2, 0], [0, 0, h, w, 1], [2, 1, h - 3, w - 1, 1]], np.int32)
    wins = np.array([[size[0] + 5, size[1] + 7, 2, 3]] * 3, np.int32)
    out = ldt_amd.resize_raw(torch.from_numpy(raw), h, w, normalize=None, size=size, crops=boxes, windows=wins,
                             interpolation="bicubic", dtype="uint8", memory_format="channels_last").cpu()
    for k in range(3):
        t, l, bh, bw, f = boxes[k].tolist()
        _check_row(out[k], _pil_window(raw[k, t:t + bh, l:l + bw], size, wins[k], f), "uint8", f"raw composed row {k}")


# ---- 6. progressive ----------------------------------------------------------------------------

def test_a_progressive_cell_in_bf16_channels_last(mixed):
    cells = [c for c in mixed if c[0] == "prog-64x80"]
    assert len(cells) == 1
    for size in ((224, 224), (30, 33)):
        img, lbl, failed = _decode(cells, size, "bfloat16", "channels_last")
        assert _check_batch(cells, size, "bfloat16", "channels_last", img, lbl, failed, "progressive") == 1


# ---- 7. the entry points agree -----------------------------------------------------------------

ENTRY_SIZE = (30, 33)
ENTRY = dict(dtype="float16", memory_format="channels_last")


def _entry_bytes(out, n):
    import torch

    keyed = isinstance(out, dict) or hasattr(out, "keys")
    img, lbl = (out["image"], out["label"]) if keyed else (out[0], out[1])
    assert img.dtype == torch.float16 and tuple(img.shape) == (n, 3) + ENTRY_SIZE
    assert img.stride() == _strides(ENTRY_SIZE, "channels_last"), img.stride()
    assert lbl.cpu().tolist() == list(range(100, 100 + n))
    return img.cpu().contiguous().view(torch.int16)


def test_the_entry_points_agree(mixed, tmp_path):
    import torch
    from torch.utils.data import DataLoader

    import ldt_amd
    from ldt_amd import transforms as T

    n = len(mixed)
    images = [d for _, d in mixed]
    labels = np.arange(100, 100 + n)
    rb = pa.RecordBatch.from_arrays([pa.array(images, pa.binary()), pa.array(labels, pa.int64())],
                                    names=["image", "label"])
    items = [{"image": d, "label": 100 + k} for k, d in enumerate(images)]
    kw = dict(size=ENTRY_SIZE, dtype=torch.float16, memory_format=torch.channels_last)
    img, lbl, failed = _decode(mixed, ENTRY_SIZE, ENTRY["dtype"], ENTRY["memory_format"])
    assert _check_batch(mixed, ENTRY_SIZE, ENTRY["dtype"], ENTRY["memory_format"], img, lbl, failed, "guarded") == n
    want = img.contiguous().view(torch.int16)
    got = {"decode_tensor_image": ldt_amd.decode_tensor_image(rb, **kw),
           "collate_fn": ldt_amd.collate_fn(items, **kw),
           "collate_fn(RecordBatch)": ldt_amd.collate_fn(rb, **kw),
           "DeviceBatch": T.DeviceBatch(T._pack_list(images, labels.tolist()), **kw),
           "ResidentBatch.decode": ldt_amd.ResidentBatch(images, labels).decode(**kw)}
    pipe = ldt_amd.DecodePipeline(depth=2, **kw)
    assert (pipe.dtype, pipe.memory_format) == ("float16", "channels_last")
    got["DecodePipeline"] = pipe.decode(rb)
    got["DecodePipeline, second slot"] = pipe.decode(ldt_amd.ResidentBatch(images, labels))
    pipe.check()
    fn = ldt_amd.make_to_tensor_fn(depth=2, **kw)
    got["make_to_tensor_fn"] = fn(rb)
    fn.check()
    # make_collate_fn through a 1-worker DataLoader: a DeviceBatch decoded in the main process
    ds = ldt_amd.write_dataset(pa.table({"image": pa.array(images, pa.binary()), "label": pa.array(labels, pa.int64())}),
                               str(tmp_path / "ds"), max_rows_per_file=100)
    dl = DataLoader(ldt_amd.SafeLanceDataset(ds.uri), batch_size=n, shuffle=False, num_workers=1,
                    collate_fn=ldt_amd.make_collate_fn(**kw), pin_memory=False, multiprocessing_context="spawn")
    batches = list(dl)
    assert len(batches) == 1 and isinstance(batches[0], T.DeviceBatch)
    assert (batches[0]._dtype, batches[0]._memory_format) == ("float16", "channels_last")
    got["make_collate_fn in a worker"] = batches[0]
    torch.cuda.synchronize()
    for what, out in got.items():
        assert torch.equal(_entry_bytes(out, n), want), what


# ---- 8. format changes between calls -----------------------------------------------------------

def test_two_pipelines_of_different_formats_alternate(mixed):
    import torch

    import ldt_amd

    n = len(mixed)
    rb = pa.RecordBatch.from_arrays([pa.array([d for _, d in mixed], pa.binary()),
                                     pa.array(np.arange(100, 100 + n), pa.int64())], names=["image", "label"])
    size = (30, 33)
    fmts = [("bfloat16", "channels_last"), ("uint8", "contiguous")]
    pipes = [ldt_amd.DecodePipeline(depth=2, size=size, dtype=d, memory_format=m) for d, m in fmts]
    outs = [(b % 2, pipes[b % 2].decode(rb)) for b in range(6)]
    for p in pipes:
        p.check()
    torch.cuda.synchronize()
    for b, (which, (img, lbl)) in enumerate(outs):
        d, m = fmts[which]
        assert img.dtype == _td(d) and img.stride() == _strides(size, m)
        assert _check_batch(mixed, size, d, m, img.cpu(), lbl.cpu().numpy(), {}, f"batch {b}") == n
    # each slot's context kept its own format; the shared context none of them
    for p, f in zip(pipes, fmts):
        assert all(c.output_format() == f for c in p.ctxs)
    # and on the shared context: a change is a library call, a repeat is not
    ctx, _lib = _ctx()
    arr = pa.array([d for _, d in mixed], pa.binary())
    from ldt_amd import transforms as T

    for d, m in (fmts[0], fmts[0], fmts[1], ("float32", "contiguous"), fmts[1], ("float32", "contiguous")):
        img = T.decode_arrow(arr, size=size, dtype=d, memory_format=m)[0]
        assert ctx.output_format() == (d, m) and ctx._format == (d, m)
        assert _check_batch(mixed, size, d, m, img.cpu(), None, {}, "shared context") == n


# ---- 9. the defaults are unchanged -------------------------------------------------------------

@pytest.mark.parametrize("size", [(224, 224), (30, 33)], ids=_ID)
def test_the_defaults_are_the_call_without_the_arguments(mixed, size):
    import torch

    from ldt_amd import transforms as T

    ctx, _lib = _ctx()
    arr = pa.array([d for _, d in mixed], pa.binary())
    plain = T.decode_arrow(arr, size=size)[0]
    kernel = ctx.lib.ldt_debug_last_resize(ctx.handle)
    assert plain.dtype == torch.float32 and plain.is_contiguous()
    for k, (name, data) in enumerate(mixed):
        assert np.array_equal(plain[k].cpu().numpy(), _expected(name, data, size, interp="bilinear")), name
    for kw in (dict(dtype=None, memory_format=None), dict(dtype=torch.float32), dict(dtype="float32"),
               dict(memory_format=torch.contiguous_format), dict(dtype=torch.float32, memory_format="contiguous")):
        T.decode_arrow(arr, size=size, dtype="uint8", memory_format="channels_last")  # another format in between
        got = T.decode_arrow(arr, size=size, **kw)[0]
        assert got.dtype == torch.float32 and got.stride() == plain.stride() and got.is_contiguous()
        assert torch.equal(got.view(torch.int32), plain.view(torch.int32)), kw
        assert ctx.lib.ldt_debug_last_resize(ctx.handle) == kernel and ctx.output_format() == ("float32", "contiguous")


# ---- 10. argument errors -----------------------------------------------------------------------

def test_uint8_with_normalize_enqueues_nothing_and_a_wrong_out_raises(mixed):
    import ctypes

    import torch

    import ldt_amd
    from ldt_amd import transforms as T

    ctx, _lib = _ctx()
    arr = pa.array([d for _, d in mixed], pa.binary())
    n, size = len(mixed), (30, 33)
    T.decode_arrow(arr, size=size)
    ticket = ctx.lib.ldt_last_ticket(ctx.handle)
    with pytest.raises(ValueError, match="uint8.*normalize"):
        T.decode_arrow(arr, size=size, dtype=torch.uint8, normalize=True)
    res = ldt_amd.ResidentBatch([d for _, d in mixed])
    with pytest.raises(ValueError, match="uint8.*normalize"):
        res.decode(size=size, dtype="uint8", normalize=IMAGENET)
    pipe = ldt_amd.DecodePipeline(depth=1, size=size, dtype="uint8")
    with pytest.raises(ValueError, match="uint8.*normalize"):
        pipe.decode(res, normalize=True)
    assert ctx.lib.ldt_last_ticket(ctx.handle) == ticket
    assert all(c.lib.ldt_last_ticket(c.handle) == 0 for c in pipe.ctxs)
    # the C ABI says the same: LDT_ERR_ARG, nothing enqueued, and the state is as ldt_set_filter's
    c = _lib.Context(torch.cuda.current_device())
    d, m = ctypes.c_int(-1), ctypes.c_int(-1)
    assert c.lib.ldt_get_output_format(c.handle, ctypes.byref(d), ctypes.byref(m)) == 0 and (d.value, m.value) == (0, 0)
    for bad in ((4, 0), (-1, 0), (0, 2), (0, -1), (3, 7)):
        assert c.lib.ldt_set_output_format(c.handle, *bad) == _lib.LDT_ERR_ARG
    assert c.output_format() == ("float32", "contiguous")
    assert c.lib.ldt_set_output_format(c.handle, 3, 1) == 0
    assert c.lib.ldt_get_output_format(c.handle, None, ctypes.byref(m)) == 0 and m.value == 1
    assert c.lib.ldt_get_output_format(c.handle, ctypes.byref(d), None) == 0 and d.value == 3
    assert c.lib.ldt_set_output_format(c.handle, 9, 1) == _lib.LDT_ERR_ARG and c.output_format() == ("uint8", "channels_last")
    c._format = ("uint8", "channels_last")
    out = T._empty_image(n, size, "uint8", "channels_last", "cuda")
    status = np.zeros(n, np.int32)
    norm = T._norm_struct(True)
    bufs = arr.buffers()
    rc = c.lib.ldt_decode_batch(c.handle, bufs[2].address, bufs[1].address, 0, n, None, None, 0, out.data_ptr(), None,
                                ctypes.byref(norm), torch.cuda.current_stream().cuda_stream, status.ctypes.data)
    assert rc == _lib.LDT_ERR_ARG and c.lib.ldt_last_ticket(c.handle) == 0
    raw = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    rc = c.lib.ldt_resize_raw(c.handle, raw.data_ptr(), 0, 1, 8, 8, 192, out.data_ptr(), ctypes.byref(norm),
                              torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.LDT_ERR_ARG
    # without the Normalize the same context decodes
    got, _ = T.decode_arrow(arr, size=size, ctx=c, out=out, dtype="uint8", memory_format="channels_last")
    assert _check_batch(mixed, size, "uint8", "channels_last", got.cpu(), None, {}, "own context") == n
    # a caller's out= must be of the format
    for bad in (torch.empty((n, 3) + size, dtype=torch.float32, device="cuda"),              # dtype
                torch.empty((n, 3) + size, dtype=torch.uint8, device="cuda"),                # strides
                T._empty_image(n - 1, size, "uint8", "channels_last", "cuda"),               # shape
                T._empty_image(n, (33, 30), "uint8", "channels_last", "cuda")):
        with pytest.raises(ValueError, match="out="):
            T.decode_arrow(arr, size=size, out=bad, dtype="uint8", memory_format="channels_last")
        with pytest.raises(ValueError, match="out="):
            res.decode(bad, size=size, dtype="uint8", memory_format="channels_last")
    assert ctx.lib.ldt_last_ticket(ctx.handle) == ticket
