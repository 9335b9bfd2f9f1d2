"""CPU tests of the source pad (``Pad(source=True)``): the record, ``check_pad``, ``ExpandToSquare``, the GPU tests'
reference against ``ImageOps.expand``, and the planner under the flag (tools/checks/source_pad_host.cpp, plain g++)."""
import ctypes
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

import ldt_amd
from conftest import REPO, read_golden


def test_the_record():
    p = ldt_amd.Pad((1, 2, 3), "edge", source=True)
    assert (p.fill, p.mode, p.source) == ((1, 2, 3), "edge", True) and not ldt_amd.Pad().source
    assert p == ldt_amd.Pad((1, 2, 3), "edge", True) and p != ldt_amd.Pad((1, 2, 3), "edge")
    assert hash(p) != hash(ldt_amd.Pad((1, 2, 3), "edge")) and pickle.loads(pickle.dumps(p)) == p
    old = ldt_amd.Pad.__new__(ldt_amd.Pad)
    old.__setstate__(((4, 5, 6), "reflect"))  # a record pickled before the field existed
    assert old == ldt_amd.Pad((4, 5, 6), "reflect") and repr(old) == "Pad(fill=(4, 5, 6), mode='reflect')"
    assert repr(p) == "Pad(fill=(1, 2, 3), mode='edge', source=True)"
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="source"):
            ldt_amd.Pad(source=bad)


def test_check_pad_rules():
    src, crops, win = ldt_amd.Pad(7, source=True), np.array([[-1, -1, 4, 4, 0]]), ldt_amd.ResizeCenterCrop(8)
    assert ldt_amd.check_pad(src, crop=crops) is src and ldt_amd.check_pad(src, win, crop=crops) is src
    with pytest.raises(ValueError, match="without a crop"):
        ldt_amd.check_pad(src, win)
    with pytest.raises(ValueError, match="one pad"):
        ldt_amd.check_pad(src, ldt_amd.Letterbox(), crop=crops)
    with pytest.raises(ValueError, match="without a window"):  # a window pad keeps its rule, crop or not
        ldt_amd.check_pad(ldt_amd.Pad(7), crop=crops)
    spec = ldt_amd.transforms.CallSpec.make(size=(8, 8), crop=ldt_amd.ExpandToSquare(), pad=src)
    assert spec.pad is src and pickle.loads(pickle.dumps(spec)).pad == src
    with pytest.raises(ValueError, match="without a crop"):
        ldt_amd.transforms.CallSpec.make(size=(8, 8), pad=src)


def test_expand_to_square_is_expand2square():
    wh = np.array([[64, 48], [48, 64], [5, 10], [10, 5], [7, 7], [9, 4], [0, 3], [6, 6]])
    status = np.array([0, 0, 0, 0, 0, 0, 0, 3])
    got = pickle.loads(pickle.dumps(ldt_amd.ExpandToSquare())).sample(wh, status)
    assert got.dtype == np.int32 and got.shape == (8, 5)
    for (w, h), st, row in zip(wh.tolist(), status.tolist(), got.tolist()):
        if st or w == 0:
            assert row == [0, 0, 1, 1, 0]
            continue
        # expand2square: a (w, w) canvas with paste (0, (w - h) // 2), or an (h, h) one with ((h - w) // 2, 0)
        s, paste = (w, (0, (w - h) // 2)) if w > h else (h, ((h - w) // 2, 0)) if h > w else (w, (0, 0))
        assert row == [-paste[1], -paste[0], s, s, 0], (w, h)
    assert (ldt_amd.ExpandToSquare().sample(wh, status, views=2) == got[:, None]).all()


def test_np_pad_is_what_pillow_pads():
    from PIL import Image, ImageOps

    from test_gpu_source_pad import reference

    rgb = np.random.RandomState(3).randint(0, 256, (9, 13, 3), np.uint8)
    pad = ldt_amd.Pad((122, 116, 104), source=True)
    big = ImageOps.expand(Image.fromarray(rgb), border=80, fill=pad.fill)
    for box in [(-5, -7, 20, 30, 0), (2, 3, 4, 5, 0), (-20, 60, 10, 10, 0), (-3, 0, 15, 13, 1)]:
        t, l, h, w, flip = box
        want = np.asarray(big.crop((l + 80, t + 80, l + 80 + w, t + 80 + h)).resize((6, 5), Image.BICUBIC))
        assert np.array_equal(reference(rgb, box, (5, 6), pad, "bicubic"), want[:, ::-1] if flip else want), box


def test_planner_statuses_under_the_flag(tmp_path):
    from ldt_amd import synth

    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    so = str(tmp_path / "libsource_pad_host.so")
    src = [os.path.join(REPO, "tools", "checks", "source_pad_host.cpp"),
           os.path.join(REPO, "lance-distributed-training_amd", "csrc", "ldt_plan.cpp")]
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", *src,
                    "-o", so], check=True)
    host, M = ctypes.CDLL(so), 8192
    assert [m for m in range(-20, 40) if host.source_pad_host_mode_ok(m)] == [0, 1, 2, 3, 16, 17, 18, 19]
    for box, plain, padded in [  # (top, left, h, w, flip) on a 53 x 37 image resized to 30 x 33
            ((0, 0, 37, 53, 0), 0, 0), ((-5, -7, 50, 70, 1), 6, 0), ((-20, 60, 10, 10, 0), 6, 0), ((-M, M, M, M, 0), 6, 4),
            ((-M, M, 1000, 1000, 0), 6, 0), ((0, 0, 0, 5, 0), 6, 6), ((0, 0, 5, M + 1, 0), 6, 6), ((-M - 1, 0, 5, 5, 0), 6, 6),
            ((0, M + 1, 5, 5, 0), 6, 6), ((0, 0, 5, 5, 2), 6, 6), ((-2**31, 2**31 - 1, 2**31 - 1, 2**31 - 1, 0), 6, 6),
            ((0, 0, 1200, 20, 0), 6, 4)]:  # 1200 rows onto 30: over the reduction limit, as without the flag
        assert host.source_pad_host_check_crop(*box, 53, 37, 30, 33, 0, 0) == plain, box
        assert host.source_pad_host_check_crop(*box, 53, 37, 30, 33, 0, 1) == padded, box
    cells = [synth.encode(synth.field(37, 53, 202, 6.0)), read_golden("jpeg/gray_77x91.jpg"),
             read_golden("jpeg/bad_not_jpeg.bin"), synth.encode(synth.field(8, 8, 205, 6.0), subsampling="4:4:4")]
    data = np.frombuffer(b"".join(cells), np.uint8)
    off = np.cumsum([0] + [len(c) for c in cells]).astype(np.int64)
    crops = np.array([[-5, -7, 50, 100, 0], [0, 0, 77, 91, 0], [0, 0, 1, 1, 0], [-100, -100, 0, 8, 0]], np.int32)
    windows = np.array([[40, 40, 5, 3], [40, 40, -1, 0], [40, 40, 0, 0], [40, 40, 0, 0]], np.int32)

    def plan(src_padded, windows=None):  # the rows' statuses, then max_w, max_h, max_ks_h, max_ks_v
        out, ptr = np.zeros(8, np.int32), lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
        host.source_pad_host_plan(ptr(data), ptr(off), ctypes.c_int64(4), ptr(crops), ptr(windows), 30, 33, src_padded, ptr(out))
        return out.tolist()

    assert plan(0) == [6, 0, 1, 6, 91, 77, 7, 7]
    # the staged row and the taps come from the widest box, inside the image or not: 100 / 33 -> 9 taps, 77 / 30 -> 7
    assert plan(1) == [0, 0, 1, 6, 100, 77, 9, 7]
    # a window under a source pad keeps the unpadded rule (row 1: status 7, ahead of its box)
    assert plan(1, windows)[:4] == [0, 7, 1, 6]
