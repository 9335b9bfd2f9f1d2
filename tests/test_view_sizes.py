"""CPU tests of per-view output sizes: ``size=[(h, w), ...]``, one output size
per view of a call (ldt_set_view_sizes). What needs no GPU.

* ``check_view_sizes``: what it accepts, what it refuses, and that a plain
  ``(h, w)`` still gets ``check_size``'s answer.
* Every entry point refuses a size list that contradicts ``views=`` and a 2-D
  crops array before any context or device is asked for.
* ``RandomResizedCropFlip`` with one scale per view: the draw order, and that a
  single pair draws what it drew before (rows pinned from the code as it was).
* ``ResizeCenterCrop`` with a size list against its documented arithmetic;
  ``ResizeFiveCrop`` refuses one.
* The planner and the shared index arithmetic (csrc/ldt_view_index.hpp) under
  AddressSanitizer + UBSan, through the stand-alone driver
  tests/fuzz/view_sizes_plan_check.cpp (its own ``main``, run directly).
"""
import os
import pickle
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import REPO, read_golden
from oracle import oracle

A = [(224, 224)] * 2 + [(96, 96)] * 6


# ---- check_view_sizes ---------------------------------------------------------------------------

def test_check_view_sizes_accepts_lists_tuples_arrays_and_numpy_ints():
    from ldt_amd._lib import ViewSizes, check_view_sizes

    want = ((7, 5), (299, 260), (1, 1))
    for arg in ([(7, 5), (299, 260), (1, 1)], ((7, 5), [299, 260], (1, 1)), np.array(want), np.array(want, np.int16),
                [(np.int64(7), np.int32(5)), np.array([299, 260]), (1, 1)]):
        got = check_view_sizes(arg)
        assert isinstance(got, ViewSizes) and tuple(got) == want
        assert all(type(v) is int for p in got for v in p)
        assert check_view_sizes(got) is got
    assert tuple(check_view_sizes([(8, 8)])) == ((8, 8),)  # the form decides: a list of one view
    assert len(check_view_sizes([(1024, 1)] * 16)) == 16
    s = check_view_sizes(A)
    assert s.elements == 3 * (2 * 224 * 224 + 6 * 96 * 96)
    assert s.runs() == [(0, 2, (224, 224)), (2, 6, (96, 96))]
    assert check_view_sizes([(32, 40), (16, 24)] * 2).runs() == [(0, 1, (32, 40)), (1, 1, (16, 24)), (2, 1, (32, 40)),
                                                                 (3, 1, (16, 24))]
    back = pickle.loads(pickle.dumps(s))
    assert isinstance(back, ViewSizes) and back == s


@pytest.mark.parametrize("bad", [[], (), [(8, 8)] * 17, [(8, 8), (0, 8)], [(8, 8), (8, 1025)], [(8, 8, 8)],
                                 [(8, 8), (8, 8, 8)], [(8.0, 8)], [(8, 8.5)], 8, np.int32(8), [(8, 8), 8],
                                 [8, (8, 8)], [(8, 8), None], [[(8, 8)]], [(True, 8)], [("8", "8")], "ab",
                                 np.zeros((2, 3), int), np.zeros((0, 2), int), np.ones((17, 2), int)],
                         ids=repr)
def test_check_view_sizes_refuses(bad):
    from ldt_amd._lib import check_view_sizes

    with pytest.raises((TypeError, ValueError)):
        check_view_sizes(bad)


@pytest.mark.parametrize("plain", [None, (224, 224), [7, 5], (np.int64(1), 1024), np.array([30, 33])], ids=repr)
def test_a_plain_pair_still_goes_to_check_size(plain):
    from ldt_amd._lib import ViewSizes, check_size, check_view_sizes

    got = check_view_sizes(plain)
    assert got == check_size(plain) and type(got) is tuple and not isinstance(got, ViewSizes)


def test_check_size_itself_is_unchanged():
    from ldt_amd._lib import check_size

    for bad in ([(8, 8)], [(8, 8), (8, 8)], (), []):
        with pytest.raises((TypeError, ValueError)):
            check_size(bad)


# ---- every entry point, before any context ------------------------------------------------------

def test_every_entry_point_validates_a_size_list_before_any_context(monkeypatch):
    import pyarrow as pa

    import ldt_amd
    from ldt_amd import transforms as T

    def no_context(*a, **k):
        raise AssertionError("a context was requested before the size list was validated")

    monkeypatch.setattr(T, "_decoder", no_context)
    monkeypatch.setattr(T._lib, "get_context", no_context)
    rb = pa.RecordBatch.from_arrays([pa.array([b"x"], pa.binary()), pa.array([1], pa.int64())], ["image", "label"])
    arr = rb.column(0)
    three = [(8, 8)] * 3
    rbatch = object.__new__(T.ResidentBatch)
    rbatch.n = 1
    packed = T._pack_list([b"x"], [1])
    calls = [
        lambda **k: T.decode_arrow(arr, **k),
        lambda **k: ldt_amd.decode_tensor_image(rb, **k),
        lambda **k: ldt_amd.collate_fn([{"image": b"x", "label": 1}], **k),
        lambda **k: T.DeviceBatch(packed, **k),
        lambda **k: rbatch.decode(**k),
        lambda **k: T.make_collate_fn(**k),
        lambda **k: T.DecodePipeline(**k),
        lambda **k: T.make_to_tensor_fn(**k),
    ]
    for k, call in enumerate(calls):
        with pytest.raises(ValueError, match="views"):
            call(size=three, views=2)
        with pytest.raises((TypeError, ValueError)):
            call(size=[(8, 8), (0, 8)])
        if k == 0:  # decode_arrow takes arrays only
            continue
        with pytest.raises(ValueError, match="one size"):
            call(size=three, **{"windows" if k == 4 else "window": ldt_amd.ResizeFiveCrop(16)})
    crops2d = np.array([[0, 0, 1, 1, 0]], np.int32)
    for k, call in enumerate(calls[:5]):  # the ones that take an array
        with pytest.raises(ValueError, match=r"\[n, 3, 5\]"):
            call(size=three, **{"crops" if k in (0, 4) else "crop": crops2d})
    with pytest.raises(ValueError, match="size list"):
        T.resize_raw(np.zeros((1, 2, 2, 3), np.uint8), 2, 2, size=three)


def test_size_list_travels_through_pickle():
    from ldt_amd import transforms as T
    from ldt_amd._lib import ViewSizes

    fn = pickle.loads(pickle.dumps(T.make_collate_fn(device="cuda:0", size=A)))
    assert isinstance(fn.size, ViewSizes) and list(fn.size) == A and fn.views == 8
    b = pickle.loads(pickle.dumps(T.DeviceBatch(T._pack_list([b"abc", b"de"], [1, 2]), "cuda:0", None, size=A)))
    assert isinstance(b._size, ViewSizes) and list(b._size) == A and b._views == 8
    assert T.make_collate_fn(size=[(8, 8)]).views == 1 and T.make_collate_fn(size=(8, 8)).views is None


def test_view_sizes_symbol_declared_exported_bound():
    from ldt_amd import _lib

    assert "ldt_set_view_sizes" in _lib.EXPORTED
    with open(os.path.join(REPO, "include", "ldt.h")) as f:
        assert "int ldt_set_view_sizes(ldt_ctx *ctx, const int32_t *hw, int views);" in f.read()
    L = _lib.load_library()
    assert L.ldt_set_view_sizes.restype is not None
    hw = (np.ones(4, np.int32)).ctypes.data
    assert L.ldt_set_view_sizes(None, hw, 2) == _lib.LDT_ERR_ARG  # a null context


# ---- samplers -----------------------------------------------------------------------------------

def test_per_view_scales_draw_image_major_view_minor():
    import torch

    import ldt_amd

    scales = [(0.4, 1.0), (0.05, 0.4), (0.2, 0.3)]
    wh = np.array([[500, 375], [64, 48], [0, 0], [91, 77], [5, 17]], np.int32)
    status = np.array([0, 0, 2, 0, 0], np.int32)
    g = torch.Generator().manual_seed(77)
    got = ldt_amd.RandomResizedCropFlip(scale=scales, generator=g).sample(wh, status, views=3)
    assert got.shape == (5, 3, 5) and got.dtype == np.int32
    g1 = torch.Generator().manual_seed(77)
    singles = [ldt_amd.RandomResizedCropFlip(scale=s, generator=g1) for s in scales]
    for i in range(len(wh)):
        for v in range(3):
            if status[i] != 0:
                assert got[i, v].tolist() == [0, 0, 1, 1, 0]
            else:
                assert got[i, v].tolist() == singles[v].sample(wh[i:i + 1])[0].tolist(), (i, v)
    # the local views are the smaller ones
    big, small = got[0, 0], got[0, 1]
    assert big[2] * big[3] >= 0.4 * 500 * 375 * 0.9 and small[2] * small[3] <= 0.4 * 500 * 375 * 1.1
    s = ldt_amd.RandomResizedCropFlip(scale=scales)
    assert s.scale == scales[0] and s.scales == scales and "0.05" in repr(s)
    assert pickle.loads(pickle.dumps(s)).scales == scales
    for views in (None, 2, 4):
        with pytest.raises(ValueError, match="views"):
            s.sample(wh, status, views=views)
    for bad in ([], [(0.1, 0.2, 0.3)], [(0.5, 0.1)], [(0.1, 1.0)] * 17, (0.1,), [(0.0, 1.0)]):
        with pytest.raises(ValueError):
            ldt_amd.RandomResizedCropFlip(scale=bad)


def test_a_single_scale_pair_draws_what_it_drew():
    """Rows drawn by the sampler before per-view scales existed, seed 1234."""
    import torch

    import ldt_amd

    wh = np.array([[500, 375], [64, 48], [91, 77]])
    s = ldt_amd.RandomResizedCropFlip(scale=(0.25, 1.0), generator=torch.Generator().manual_seed(1234))
    assert s.scales is None
    assert s.sample(wh).tolist() == [[102, 185, 232, 219, 1], [1, 3, 41, 45, 0], [3, 6, 70, 84, 1]]
    assert s.sample(wh, None, views=2).tolist() == [[[44, 5, 321, 279, 0], [13, 21, 335, 330, 0]],
                                                    [[6, 20, 36, 43, 0], [0, 24, 48, 36, 1]],
                                                    [[0, 7, 76, 72, 0], [2, 6, 67, 85, 0]]]
    # a list of one pair is the per-view form with V = 1 and draws the same boxes
    g = torch.Generator().manual_seed(1234)
    one = ldt_amd.RandomResizedCropFlip(scale=[(0.25, 1.0)], generator=g)
    assert one.sample(wh, None, views=1)[:, 0].tolist() == [[102, 185, 232, 219, 1], [1, 3, 41, 45, 0], [3, 6, 70, 84, 1]]


def test_resize_center_crop_with_a_size_list():
    import ldt_amd

    sizes = [(224, 224), (96, 96), (7, 5), (300, 260)]
    wh = np.array([[500, 375], [48, 64], [0, 0], [91, 77]], np.int32)
    status = np.array([0, 0, 3, 0], np.int32)
    rc = ldt_amd.ResizeCenterCrop(256)
    got = rc.sample(wh, status, sizes, views=4)
    assert got.shape == (4, 4, 4) and got.dtype == np.int32
    for i, (w, h) in enumerate(wh.tolist()):
        for v, (oh, ow) in enumerate(sizes):
            if status[i]:
                assert got[i, v].tolist() == [oh, ow, 0, 0]
                continue
            short, long = (w, h) if w <= h else (h, w)
            new_long = int(256 * long / short)
            rw, rh = (256, new_long) if w <= h else (new_long, 256)
            assert got[i, v].tolist() == [rh, rw, int(round((rh - oh) / 2.0)), int(round((rw - ow) / 2.0))], (i, v)
            assert got[i, v].tolist() == rc.sample(wh[i:i + 1], None, (oh, ow))[0].tolist()
    # per-view boxes [n, V, 2] too
    whv = np.stack([wh, wh[:, ::-1], wh, wh], axis=1)
    gv = rc.sample(whv, status, sizes, views=4)
    assert gv[0, 1].tolist() == rc.sample(wh[0:1, ::-1], None, (96, 96))[0].tolist()
    with pytest.raises(ValueError, match="views"):
        rc.sample(wh, status, sizes, views=3)
    with pytest.raises(ValueError, match="views"):
        rc.sample(wh, status, sizes)
    with pytest.raises(ValueError, match="FiveCrop"):
        ldt_amd.ResizeFiveCrop(256).sample(wh, status, [(8, 8)] * 5)
    # a uniform call is untouched
    assert rc.sample(wh, status, (224, 224), views=2).tolist() == \
        np.repeat(rc.sample(wh, status, (224, 224))[:, None], 2, axis=1).tolist()


def test_split_views_layout():
    """The tuple a size list returns: one tensor per run, views of one flat
    allocation at the documented offsets."""
    import torch

    from ldt_amd import transforms as T
    from ldt_amd._lib import check_view_sizes

    n = 3
    sizes = check_view_sizes([(4, 6), (4, 6), (1, 1), (2, 5), (4, 6)])
    flat = torch.arange(n * sizes.elements, dtype=torch.float32)
    for mf in ("contiguous", "channels_last"):
        runs = T._split_views(flat, n, sizes, mf)
        assert [tuple(r.shape) for r in runs] == [(2, n, 3, 4, 6), (1, n, 3, 1, 1), (1, n, 3, 2, 5), (1, n, 3, 4, 6)]
        base = 0
        for r in runs:
            V, _, _, h, w = r.shape
            assert r.data_ptr() == flat.data_ptr() + 4 * base
            want = (n * 3 * h * w, 3 * h * w, 1, 3 * w, 3) if mf == "channels_last" else (n * 3 * h * w, 3 * h * w, h * w, w, 1)
            assert r.stride() == want
            # image (v, i) starts i * 3 * h * w elements after the view's base
            assert float(r[V - 1, 2, 0, 0, 0]) == base + (V - 1) * n * 3 * h * w + 2 * 3 * h * w
            base += V * n * 3 * h * w
        assert base == flat.numel()
        assert torch.equal(runs[0].flatten(0, 1), torch.cat([runs[0][0], runs[0][1]]))
    assert len(T._split_views(flat[:n * 3 * 16], n, check_view_sizes([(4, 4)]), "contiguous")) == 1


# ---- the planner and the index arithmetic under the sanitizers ----------------------------------

def test_planner_with_view_sizes_under_sanitizers(tmp_path):
    from ldt_amd import synth

    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "view_sizes_plan_check")
    src = [os.path.join(REPO, "tests", "fuzz", "view_sizes_plan_check.cpp"),
           os.path.join(REPO, "lance-distributed-training_amd", "csrc", "ldt_plan.cpp")]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", *src, "-o", exe], check=True)
    cells = [synth.encode(synth.field(375, 500, 202, 6.0), quality=90, restart_marker_rows=1),
             synth.encode(synth.field(100, 150, 204, 6.0), subsampling="4:4:4"),
             read_golden("jpeg/gray_77x91.jpg"), read_golden("jpeg/prog_64x80.jpg"),
             synth.encode(synth.field(8, 8, 205, 6.0), subsampling="4:4:4")]
    inp = b"".join(struct.pack("<I", len(c)) + c for c in cells)
    r = subprocess.run([exe], input=inp, capture_output=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    out = r.stdout.decode()
    assert r.returncode == 0 and not r.stderr and "FAIL" not in out, (out[-4000:], r.stderr.decode(errors="replace")[-4000:])
    lines = out.splitlines()
    assert lines[-1] == "view_sizes_plan_ok"
    sizes = [tuple(int(v) for v in x.split()[1:]) for x in lines if x.startswith("size ")]
    assert sizes == [oracle.jpeg_info(c)[:2] for c in cells]
