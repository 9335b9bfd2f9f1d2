"""CPU tests of the per-image resized size and window (Resize(int) +
CenterCrop inside the resize): what needs no GPU.

* The oracle pin: ``Resize(256)`` + ``CenterCrop(224)`` on a PIL image is
  ``img.resize((res_w, res_h), BILINEAR).crop((left, top, left + ow, top +
  oh))``, and the expected tensors of tests/test_gpu_window.py come from the
  oracle as ``raw_to_tensor(src, res_h, res_w)[:, top:top+oh, left:left+ow]``,
  mirrored when flipped, ``src`` being the decoded image or a box of it. The
  two must agree bit for bit.
* ``ResizeCenterCrop.sample`` against torchvision's expressions, evaluated
  literally (torchvision is not installed).
* ``check_windows``, the one validator of every ``windows=`` argument.
* The planner with windows under AddressSanitizer + UBSan, through the
  stand-alone driver tests/fuzz/window_plan_check.cpp (its own ``main``, run
  directly).
"""
import io
import os
import pickle
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_recode as jr
from conftest import REPO, read_golden
from oracle import oracle


def _c4():
    """A 500 x 375 4:2:0 cell with restart rows (not a multiple of its 16 x 16 MCU)."""
    from ldt_amd import synth

    return synth.encode(synth.field(375, 500, 202, 6.0), quality=90, restart_marker_rows=1)


# ---- the oracle composition is Pillow's resize().crop() ---------------------------------

def _pin_cases():
    from ldt_amd import synth

    c4 = _c4()
    l411 = next(c for c in jr.layout_cells() if c.name == "411-33x40")
    gray = read_golden("jpeg/gray_77x91.jpg")
    prog = read_golden("jpeg/prog_64x80.jpg")
    up = synth.encode(synth.field(8, 8, 205, 6.0), subsampling="4:4:4")
    # (name, cell, box (top, left, height, width) or None, (res_h, res_w, top, left), (oh, ow), flip)
    return [
        ("resize256-centre224", c4, None, (256, 341, 16, 58), (224, 224), 0),
        ("flush-bottom-right-odd", c4, None, (61, 82, 31, 49), (30, 33), 0),
        ("short-last-band", c4, None, (100, 133, 7, 9), (13, 21), 1),
        ("res_w-2000", c4, None, (30, 2000, 0, 1967), (30, 33), 0),
        ("res_w-1500-two-tiles", c4, None, (299, 1500, 0, 1201), (299, 299), 1),
        ("boxed", c4, (17, 33, 201, 311), (256, 396, 16, 86), (224, 224), 1),
        ("411-odd", l411.data, None, (48, 39, 9, 3), (30, 33), 1),
        ("411-boxed", l411.data, (5, 3, 20, 30), (12, 18, 5, 13), (7, 5), 0),
        ("gray", gray, None, (256, 302, 16, 39), (224, 224), 1),
        ("progressive", prog, (13, 9, 40, 51), (8, 10, 1, 5), (7, 5), 0),
        ("up-8x8", up, None, (256, 256, 16, 16), (224, 224), 0),
    ]


@pytest.mark.parametrize("case", _pin_cases(), ids=lambda c: c[0])
def test_oracle_composition_equals_pillow_resize_crop(case):
    from PIL import Image

    name, cell, box, (rh, rw, top, left), (oh, ow), flip = case
    im = Image.open(io.BytesIO(cell)).convert("RGB")
    rgb = oracle.decode_rgb(cell)
    if box is not None:
        bt, bl, bh, bw = box
        im = im.crop((bl, bt, bl + bw, bt + bh))
        rgb = rgb[bt:bt + bh, bl:bl + bw]
    assert 0 <= top <= rh - oh and 0 <= left <= rw - ow
    im = im.resize((rw, rh), Image.BILINEAR).crop((left, top, left + ow, top + oh))
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    pil = np.asarray(im, dtype=np.uint8)
    t = oracle.raw_to_tensor(rgb, rh, rw)[:, top:top + oh, left:left + ow]
    if flip:
        t = t[:, :, ::-1]
    assert t.shape == (3, oh, ow) and pil.shape == (oh, ow, 3)
    want = pil.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    assert np.array_equal(t, want), f"{name}: {np.count_nonzero(t != want)} values differ"


def test_pin_cases_cover_what_the_issue_names():
    cases = {c[0]: c for c in _pin_cases()}
    assert len(cases) >= 10
    assert max(c[3][1] for c in cases.values()) > 1024  # a res_w beyond the largest output size
    assert any(c[2] is not None for c in cases.values())


# ---- ResizeCenterCrop -------------------------------------------------------------------------

def _tv_resize(w, h, edge):
    """torchvision's _compute_resized_output_size(size=[edge]), literally."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = edge, int(edge * long / short)
    new_w, new_h = (new_short, new_long) if w <= h else (new_long, new_short)
    return new_h, new_w


def _tv_row(w, h, edge, size):
    """(res_h, res_w, top, left) of Resize(edge) + CenterCrop(size), literally."""
    res_h, res_w = _tv_resize(w, h, edge)
    top = int(round((res_h - size[0]) / 2.0))
    left = int(round((res_w - size[1]) / 2.0))
    return [res_h, res_w, top, left]


@pytest.mark.parametrize("edge", [7, 224, 256, 257])
def test_resize_center_crop_equals_the_python_expressions(edge):
    from ldt_amd import ResizeCenterCrop

    wh = np.array([(w, h) for w in range(1, 301) for h in range(1, 301)], np.int32)
    for size in [(224, 224), (7, 5)]:
        got = ResizeCenterCrop(edge).sample(wh, None, size)
        assert got.dtype == np.int32 and got.shape == (len(wh), 4)
        want = np.array([_tv_row(int(w), int(h), edge, size) for w, h in wh], np.int64)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (edge, size, wh[bad[:5]].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())


def test_resize_center_crop_large_sizes_and_rounding():
    from ldt_amd import ResizeCenterCrop

    rng = np.random.default_rng(17)
    wh = rng.integers(1, 8193, (4000, 2)).astype(np.int32)
    wh[:4] = [(8192, 8192), (8192, 1), (1, 8192), (8191, 8192)]
    for edge, size in [(256, (224, 224)), (257, (224, 224)), (7, (7, 5)), (1024, (1024, 1000)), (65535, (1, 1))]:
        got = ResizeCenterCrop(edge).sample(wh, None, size)
        want = np.array([_tv_row(int(w), int(h), edge, size) for w, h in wh], np.int64)
        assert np.array_equal(got, want), (edge, size)
    # half to even, as Python's round: a difference of 1 -> 0, 3 -> 2, 5 -> 2, 7 -> 4
    s = ResizeCenterCrop(10)
    for d, want in [(0, 0), (1, 0), (2, 1), (3, 2), (4, 2), (5, 2), (6, 3), (7, 4), (9, 4), (11, 6)]:
        assert int(round(d / 2.0)) == want
        row = s.sample(np.array([[10, 10]]), None, (10 - d, 10 - d) if d < 10 else (1, 1))
        if d < 10:
            assert row.tolist() == [[10, 10, want, want]], (d, row)
    # the default size is (224, 224), and a square image keeps the edge on both axes
    assert ResizeCenterCrop(256).sample(np.array([[500, 375], [375, 500], [300, 300]])).tolist() == \
        [[256, 341, 16, 58], [341, 256, 58, 16], [256, 256, 16, 16]]


def test_resize_center_crop_bad_rows_and_pickle():
    import ldt_amd
    from ldt_amd import ResizeCenterCrop

    s = ResizeCenterCrop(256)
    wh = np.array([[500, 375], [0, 0], [40, 40], [64, 80], [300, 100]], np.int32)
    st = np.array([0, 1, 3, 0, 0], np.int32)
    a = s.sample(wh, st, (224, 200))
    # a failed header: (out_h, out_w, 0, 0), whatever its size field says
    assert a[1].tolist() == [224, 200, 0, 0] and a[2].tolist() == [224, 200, 0, 0]
    assert a[0].tolist() == _tv_row(500, 375, 256, (224, 200))
    assert a[3].tolist() == [320, 256, 48, 28]
    # status None: a size of 0 alone marks the row unknown
    assert s.sample(wh, None, (224, 200))[1].tolist() == [224, 200, 0, 0]
    assert s.sample(wh, None, (224, 200))[2].tolist() == _tv_row(40, 40, 256, (224, 200))
    # a resized image smaller than the window: emitted as computed, negative origin (the decode refuses it)
    small = ResizeCenterCrop(100).sample(np.array([[300, 100], [100, 300]]), None, (224, 224))
    assert small.tolist() == [[100, 300, -62, 38], [300, 100, 38, -62]]
    assert small.tolist() == [_tv_row(300, 100, 100, (224, 224)), _tv_row(100, 300, 100, (224, 224))]
    assert ResizeCenterCrop(8).sample(np.array([[33, 40]]), None, (7, 5)).tolist() == [[9, 8, 1, 2]]
    t = pickle.loads(pickle.dumps(s))
    assert isinstance(t, ResizeCenterCrop) and t.edge == 256 and repr(t) == "ResizeCenterCrop(256)"
    assert np.array_equal(t.sample(wh, st, (224, 200)), a)
    fn = pickle.loads(pickle.dumps(ldt_amd.make_collate_fn(size=(224, 224), window=ResizeCenterCrop(256))))
    assert isinstance(fn.window, ResizeCenterCrop) and fn.window.edge == 256 and fn.size == (224, 224)
    for bad in (0, -1, 65536):
        with pytest.raises(ValueError):
            ResizeCenterCrop(bad)
    for bad in (256.0, "256", True, None, (256, 256)):
        with pytest.raises(TypeError):
            ResizeCenterCrop(bad)
    with pytest.raises(ValueError):
        s.sample(np.zeros((3,), np.int32))
    with pytest.raises((TypeError, ValueError)):
        s.sample(wh, None, 224)  # a bare int stays refused as a size


def test_window_sampler_takes_the_boxes_sizes_when_there_are_crops():
    from ldt_amd import ResizeCenterCrop
    from ldt_amd import transforms as T

    cells = [_c4(), read_golden("jpeg/gray_77x91.jpg"), read_golden("jpeg/bad_not_jpeg.bin")]
    s = ResizeCenterCrop(64)
    w = T._resolve_window(s, cells, None, (30, 33))
    assert w.tolist() == [_tv_row(500, 375, 64, (30, 33)), _tv_row(91, 77, 64, (30, 33)), [30, 33, 0, 0]]
    crops = [[3, 5, 100, 200, 1], [0, 0, 77, 40, 0], [0, 0, 1, 1, 0]]
    w = T._resolve_window(s, cells, crops, (30, 33))
    assert w.tolist() == [_tv_row(200, 100, 64, (30, 33)), _tv_row(40, 77, 64, (30, 33)), [30, 33, 0, 0]]
    arr = np.array([[64, 64, 1, 2]] * 3, np.int32)
    assert T._resolve_window(arr, cells, crops, (30, 33)) is arr and T._resolve_window(None, cells, None, (1, 1)) is None


# ---- check_windows -----------------------------------------------------------------------------

def test_check_windows():
    import torch

    from ldt_amd import check_windows

    assert check_windows(None, 3) is None
    a = check_windows([[256, 341, 16, 58], [8, 8, 0, 1]], 2)
    assert a.dtype == np.int32 and a.shape == (2, 4) and a.flags["C_CONTIGUOUS"]
    assert a.tolist() == [[256, 341, 16, 58], [8, 8, 0, 1]]
    wide = np.arange(16, dtype=np.int64).reshape(2, 8)[:, ::2]  # not contiguous, int64
    assert check_windows(wide, 2).tolist() == wide.tolist() and check_windows(wide, 2).flags["C_CONTIGUOUS"]
    assert check_windows(torch.tensor([[8, 8, 0, 0]]), 1).tolist() == [[8, 8, 0, 0]]
    assert check_windows(np.zeros((0, 4), np.int32), 0).shape == (0, 4)
    for bad in ([[8, 8, 0]], [8, 8, 0, 0], np.zeros((1, 4, 1), np.int32), np.zeros((1, 5), np.int32)):
        with pytest.raises(ValueError):
            check_windows(bad, 1)
    with pytest.raises(ValueError):  # n does not match
        check_windows([[8, 8, 0, 0]], 2)
    with pytest.raises(ValueError):
        check_windows(np.zeros((3, 4), np.int32), 2)
    for bad in (np.zeros((1, 4), np.float32), [[8.5, 8, 0, 0]], np.zeros((1, 4), np.bool_), [["a"] * 4]):
        with pytest.raises(TypeError):
            check_windows(bad, 1)
    with pytest.raises(ValueError):
        check_windows(np.array([[1 << 31, 8, 0, 0]], np.int64), 1)
    # negative origins and a zero size are the decode's to refuse (status 7), not the validator's
    assert check_windows([[0, -8, -1, -2]], 1).tolist() == [[0, -8, -1, -2]]


def test_window_arguments_default_to_none():
    """Every new argument is optional and named as documented."""
    import inspect

    import ldt_amd
    from ldt_amd import _lib
    from ldt_amd import transforms as T

    for fn, name in ((T.decode_arrow, "windows"), (T.ResidentBatch.decode, "windows"), (T.resize_raw, "windows"),
                     (T.DecodePipeline.decode, "windows"), (T.collate_fn, "window"), (T.make_collate_fn, "window"),
                     (T.DecodePipeline.__init__, "window"), (T.make_to_tensor_fn, "window"),
                     (T.DeviceBatch.__init__, "window")):
        assert inspect.signature(fn).parameters[name].default is None, (fn, name)
    for name in ("ResizeCenterCrop", "check_windows"):
        assert hasattr(ldt_amd, name)
    assert _lib.IMG_BAD_WINDOW == 7 and 7 in _lib.IMG_STATUS_TEXT
    assert hasattr(_lib.Context, "use_windows")
    lib = ldt_amd.load_library()
    assert "ldt_set_windows" in _lib.EXPORTED and hasattr(lib, "ldt_set_windows")
    # a bare int as the size stays refused: the shorter-edge scale is window=ResizeCenterCrop(edge)
    with pytest.raises((TypeError, ValueError)):
        _lib.check_size(256)


# ---- the planner with windows under sanitizers --------------------------------------------------

def test_planner_with_windows_under_sanitizers(tmp_path):
    from ldt_amd import synth

    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "window_plan_check")
    src = [os.path.join(REPO, "tests", "fuzz", "window_plan_check.cpp"),
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
    assert lines[-1] == "window_plan_ok"
    sizes = [tuple(int(v) for v in x.split()[1:]) for x in lines if x.startswith("size ")]
    assert sizes == [oracle.jpeg_info(c)[:2] for c in cells]
