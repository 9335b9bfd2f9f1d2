"""CPU tests of ``pad=``: ``Pad`` / ``check_pad``, the window helpers against torchvision's rules (restated: it
is not installed where the tests run), the planner's statuses with and without a pad (tools/checks/pad_host.cpp
with ldt_plan.cpp), and a Pillow pin of the reference tests/test_gpu_pad.py uses."""
import ctypes
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO, read_golden

import ldt_amd
from oracle import oracle


def test_pad_record_and_check_pad():
    q = ldt_amd.Pad((114, 7, 250), "symmetric")
    assert (ldt_amd.Pad().fill, ldt_amd.Pad().mode, ldt_amd.Pad(7).fill) == ((0, 0, 0), "constant", (7, 7, 7))
    for args, match in [((b,), "fill") for b in (-1, 256, (1, 2), (1, 2, 300), 1.5, True, "red")] + \
                       [((0, m), "mode") for m in ("wrap", "CONSTANT", 0, None)]:
        with pytest.raises(ValueError, match=match):
            ldt_amd.Pad(*args)
    win = np.array([[8, 8, -1, 0]], np.int32)
    assert ldt_amd.check_pad(None) is None and ldt_amd.check_pad(q, win) is q and ldt_amd.check_pad(9, win) == ldt_amd.Pad(9)
    for match, args in (("without a window", (q,)), ("decode_native", (q, win, True)),
                        ("ResizeFiveCrop", (q, ldt_amd.ResizeFiveCrop(40)))):
        with pytest.raises(ValueError, match=match):
            ldt_amd.check_pad(*args)
    with pytest.raises(ValueError, match="without a window"):  # a surface refuses before any device is touched
        ldt_amd.make_collate_fn(size=(8, 8), pad=q)
    fn = pickle.loads(pickle.dumps(ldt_amd.make_collate_fn(size=(8, 8), window=ldt_amd.Letterbox(), pad=q)))
    assert fn.pad == q and fn.window.align == "center"


def test_window_helpers_follow_torchvision():
    wh = np.array([[64, 48], [5, 17], [91, 77], [8, 8], [0, 0]], np.int32)
    # CenterCrop pads (size - res) // 2 on the left / top, then crops at 0; round((res - size) / 2) where it fits
    rcc = ldt_amd.ResizeCenterCrop(40, pad=True)
    assert rcc.sample(wh, None, (47, 45)).tolist() == [[40, 53, -3, 4], [136, 40, 44, -2], [40, 47, -3, 1],
                                                        [40, 40, -3, -2], [47, 45, 0, 0]]
    assert rcc.sample(wh, None, (48, 48))[0].tolist() == [40, 53, -4, 2]  # an even difference
    assert ldt_amd.ResizeCenterCrop(40).sample(wh, None, (47, 45))[[0, 3]].tolist() == [[40, 53, -4, 4], [40, 40, -4, -2]]
    assert pickle.loads(pickle.dumps(rcc)).pad is True and repr(ldt_amd.ResizeCenterCrop(40)) == "ResizeCenterCrop(40)"
    got = ldt_amd.Letterbox().sample(wh, None, (48, 48))
    assert got.tolist() == [[36, 48, -6, 0], [48, 14, 0, -17], [41, 48, -3, 0], [48, 48, 0, 0], [48, 48, 0, 0]]
    tl = pickle.loads(pickle.dumps(ldt_amd.Letterbox("topleft"))).sample(wh, None, (48, 48))
    assert np.array_equal(tl[:, :2], got[:, :2]) and not tl[:, 2:].any()
    views = ldt_amd.Letterbox().sample(wh, None, [(48, 48), (7, 5)], views=2)
    assert np.array_equal(views[:, 0], got) and views[0, 1].tolist() == [4, 5, -1, 0]
    # RandomCrop(32, padding=4, pad_if_needed=True): 64 x 48 pads to 72 x 56; 5 x 17 to 13 x 25, then the width by
    # 19 a side and the height by 7: 51 x 39; 64 x 17 to 72 x 25, then the height alone by 7: 72 x 39.
    # randint(0, h - 32 + 1) for the row, then the column, image-major
    g, rows = torch.Generator().manual_seed(11), np.array([[64, 48], [5, 17], [64, 17]], np.int32)
    draw = lambda hi: torch.randint(0, hi, size=(1,), generator=g).item()  # noqa: E731
    want = [[48, 64, draw(25) - 4, draw(41) - 4], [17, 5, draw(8) - 11, draw(20) - 23], [17, 64, draw(8) - 11, draw(41) - 4]]
    crop = ldt_amd.PadRandomCrop(4, True, torch.Generator().manual_seed(11))
    assert crop.sample(rows, None, (32, 32)).tolist() == want
    two = ldt_amd.PadRandomCrop(4, True, torch.Generator().manual_seed(11)).sample(wh[[0, 1]], None, (32, 32), views=2)
    assert two[0, 0].tolist() == want[0] and two.shape == (2, 2, 4)  # one pair per image and per view
    state = g.get_state()  # exactly the size after padding: nothing is drawn
    assert ldt_amd.PadRandomCrop((1, 2, 7, 6), generator=g).sample([[24, 24]], None, (32, 32)).tolist() == [[24, 24, -2, -1]]
    assert torch.equal(g.get_state(), state)
    with pytest.raises(ValueError, match="larger"):
        ldt_amd.PadRandomCrop(4).sample([[5, 17]], None, (32, 32))
    assert pickle.loads(pickle.dumps(ldt_amd.PadRandomCrop((1, 2), True))).padding == (1, 2, 1, 2)


def test_planner_statuses_with_and_without_a_pad(tmp_path):
    from ldt_amd import synth

    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    so = str(tmp_path / "libpad_plan.so")
    src = [os.path.join(REPO, "tools", "checks", "pad_host.cpp"),
           os.path.join(REPO, "lance-distributed-training_amd", "csrc", "ldt_plan.cpp")]
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-DPAD_HOST_PLAN", "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", *src, "-o", so], check=True)
    planner, M = ctypes.CDLL(so), 65535
    for w, plain, padded in [  # (window, status without a pad, with one) for a 30 x 33 output
            ((61, 82, 31, 49), 0, 0), ((61, 82, 32, 49), 7, 0), ((61, 82, -1, 0), 7, 0), ((29, 32, 0, 0), 7, 0),
            ((5, 5, -400, 700), 7, 0), ((1, 1, -M, M), 7, 0), ((M, M, M, -M), 7, 0), ((0, 82, 0, 0), 7, 7),
            ((61, M + 1, 0, 0), 7, 7), ((61, 82, -M - 1, 0), 7, 7), ((61, 82, 0, M + 1), 7, 7),
            ((2**31 - 1, 82, 2**31 - 1, -2**31), 7, 7)]:
        assert planner.pad_host_check_window(*w, 30, 33, 0) == plain, w
        assert planner.pad_host_check_window(*w, 30, 33, 1) == padded, w
    cells = [synth.encode(synth.field(375, 500, 202, 6.0), quality=90), read_golden("jpeg/gray_77x91.jpg"),
             read_golden("jpeg/bad_not_jpeg.bin"), synth.encode(synth.field(8, 8, 205, 6.0), subsampling="4:4:4")]
    data = np.frombuffer(b"".join(cells), np.uint8)
    off = np.cumsum([0] + [len(c) for c in cells]).astype(np.int64)
    windows = np.array([[25, 28, -2, -3], [10, 10, -2, -3], [25, 28, -2, -3], [0, 28, 0, 0]], np.int32)
    crops = np.array([[0, 0, 375, 500, 0], [0, 0, 78, 91, 0], [0, 0, 1, 1, 0], [0, 0, 8, 8, 0]], np.int32)

    def plan(mode, crops=None):  # the rows' statuses, then max_w, max_ks_h, max_ks_v
        out, ptr = np.zeros(7, np.int32), lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
        planner.pad_host_plan(ptr(data), ptr(off), ctypes.c_int64(4), ptr(windows), ptr(crops), 30, 33, mode, ptr(out))
        return out.tolist()

    assert plan(-1) == [7, 7, 1, 7, 1, 3, 3]  # without a pad every overhang is refused
    # under one, max_w and the taps of (source -> res) are an unpadded plan's: 500 / 28 -> 18, 375 / 25 -> 15
    assert [plan(mode) for mode in range(4)] == [[0, 0, 1, 7, 500, 37, 31]] * 4
    assert plan(2, crops)[:4] == [0, 6, 1, 7]  # row 1's box is one row too tall: window, crop, too large
    windows[0] = [10, 10, -2, -3]  # 500 / 10 -> 50 > 37: the reduction limit is unchanged
    assert plan(0)[:4] == [4, 0, 1, 7]


@pytest.mark.parametrize("interp", ["bilinear", "bicubic"])
def test_reference_composition_is_pillows(interp):
    from PIL import Image, ImageOps

    from ldt_amd import synth

    src, fill = synth.raw_hwc_one(37, 53, 9), (114, 7, 250)
    resized = Image.fromarray(src).resize((28, 25), Image.BILINEAR if interp == "bilinear" else Image.BICUBIC)
    pil = ImageOps.expand(resized, 8, fill).crop((-3 + 8, -2 + 8, -3 + 8 + 33, -2 + 8 + 30))  # window (-2, -3), 30 x 33
    R = oracle.raw_to_tensor(src if interp == "bilinear" else np.asarray(resized), 25, 28)
    f = oracle.raw_to_tensor(np.array(fill, np.uint8).reshape(1, 1, 3), 1, 1)[:, 0, 0]
    P = np.stack([np.pad(R[c], ((2, 3), (3, 2)), constant_values=f[c]) for c in range(3)])
    assert np.array_equal(P, oracle.raw_to_tensor(np.asarray(pil), 30, 33))
