"""CPU tests of ``views=``: several crops or windows per image from a single
decode. What needs no GPU.

* The oracle pin: the expected tensors of tests/test_gpu_views.py come from the
  oracle as ``raw_to_tensor(decode_rgb(cell)[box], res)`` -> window -> mirror.
  For the five and ten windows of ``ResizeFiveCrop`` that composition must be
  Pillow's ``resize().crop()`` of the image and of its mirror image
  (``transpose(FLIP_LEFT_RIGHT)``), in torchvision's order, bit for bit.
* ``ResizeFiveCrop``'s arithmetic, restated here.
* The samplers' draw order with ``views=V``.
* ``check_views`` and the ``views`` parameter of every entry point.
* The planner with views under AddressSanitizer + UBSan, through the
  stand-alone driver tests/fuzz/views_plan_check.cpp (its own ``main``, run
  directly).
"""
import inspect
import io
import os
import pickle
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import REPO, read_golden
from oracle import oracle


def _c420():
    from ldt_amd import synth

    return synth.encode(synth.field(48, 64, 201, 6.0))  # 48 high, 64 wide, 4:2:0


# ---- the oracle composition is Pillow's five_crop / ten_crop ------------------------------------

@pytest.mark.parametrize("ten", [False, True], ids=["five", "ten"])
@pytest.mark.parametrize("cell", ["gray_77x91", "420-48x64"])
def test_oracle_composition_equals_pillow_five_and_ten_crop(cell, ten):
    from PIL import Image

    import ldt_amd

    data = read_golden("jpeg/gray_77x91.jpg") if cell == "gray_77x91" else _c420()
    size = (32, 32)
    fc = ldt_amd.ResizeFiveCrop(40, ten=ten)
    w, h, _ = oracle.jpeg_info(data)
    wins = fc.sample(np.array([[w, h]], np.int32), None, size)[0]
    boxes = fc.boxes(np.array([[w, h]], np.int32))[0]
    assert wins.shape == (fc.views, 4) and boxes.shape == (fc.views, 5) and fc.views == (10 if ten else 5)
    # Pillow, as torchvision's Resize(40) + FiveCrop / TenCrop((32, 32)) drive it
    rh, rw = (40 * h // w, 40) if w <= h else (40, 40 * w // h)
    im = Image.open(io.BytesIO(data)).convert("RGB").resize((rw, rh), Image.BILINEAR)
    ct, cl = int(round((rh - 32) / 2.0)), int(round((rw - 32) / 2.0))

    def five(img):
        origins = [(0, 0), (0, rw - 32), (rh - 32, 0), (rh - 32, rw - 32), (ct, cl)]
        return [np.asarray(img.crop((l, t, l + 32, t + 32)), dtype=np.uint8) for t, l in origins]

    pil = five(im) + (five(im.transpose(Image.FLIP_LEFT_RIGHT)) if ten else [])
    assert (rw - 32) % 2 == 1  # an odd difference: the mirror image's centre crop is not the image's
    rgb = oracle.decode_rgb(data)
    for v in range(fc.views):
        top, left, bh, bw, flip = boxes[v].tolist()
        assert (top, left, bh, bw) == (0, 0, h, w) and flip == (1 if v >= 5 else 0)
        r_h, r_w, wt, wl = wins[v].tolist()
        assert (r_h, r_w) == (rh, rw)
        t = oracle.raw_to_tensor(rgb[top:top + bh, left:left + bw], r_h, r_w)[:, wt:wt + 32, wl:wl + 32]
        if flip:
            t = t[:, :, ::-1]
        want = pil[v].transpose(2, 0, 1).astype(np.float32) / np.float32(255)
        assert t.shape == want.shape == (3, 32, 32)
        assert np.array_equal(t, want), f"{cell} view {v}: {np.count_nonzero(t != want)} values differ from Pillow"


# ---- ResizeFiveCrop's arithmetic -----------------------------------------------------------------

def _five_rule(w, h, edge, oh, ow, ten):
    rh, rw = (edge * h // w, edge) if w <= h else (edge, edge * w // h)
    ct, cl = int(round((rh - oh) / 2.0)), int(round((rw - ow) / 2.0))
    b, r = rh - oh, rw - ow
    five = [(0, 0), (0, r), (b, 0), (b, r), (ct, cl)]
    mirrored = [(t, r - l) for t, l in five]  # crop (t, l) of the mirror image, in the image's own columns
    return [[rh, rw, t, l] for t, l in five + (mirrored if ten else [])]


def test_resize_five_crop_arithmetic():
    import ldt_amd

    wh = np.array([[500, 375], [375, 500], [300, 300], [64, 48], [91, 77]], np.int32)  # landscape, portrait, square
    for ten in (False, True):
        fc = ldt_amd.ResizeFiveCrop(256, ten=ten)
        got = fc.sample(wh, None, (224, 224))
        assert got.dtype == np.int32 and got.shape == (5, fc.views, 4)
        for i, (w, h) in enumerate(wh.tolist()):
            assert got[i].tolist() == _five_rule(w, h, 256, 224, 224, ten), (i, ten)
    assert ldt_amd.ResizeFiveCrop(256).sample(wh, None, (224, 224))[0].tolist() == [
        [256, 341, 0, 0], [256, 341, 0, 117], [256, 341, 32, 0], [256, 341, 32, 117], [256, 341, 16, 58]]
    # views 5..9 of ten-crop: (tr, tl, br, bl, centre'), where centre' mirrors an odd difference
    t = ldt_amd.ResizeFiveCrop(256, ten=True).sample(wh, None, (224, 224))[0].tolist()
    assert t[5:] == [[256, 341, 0, 117], [256, 341, 0, 0], [256, 341, 32, 117], [256, 341, 32, 0],
                     [256, 341, 16, 117 - 58]]
    # odd differences 1, 3, 5 give centres 0, 2, 2 (half to even)
    sq = np.array([[100, 100]], np.int32)
    for d, c in ((1, 0), (3, 2), (5, 2)):
        w5 = ldt_amd.ResizeFiveCrop(64).sample(sq, None, (64 - d, 64 - d))[0]
        assert w5[4].tolist() == [64, 64, c, c] and w5[3].tolist() == [64, 64, d, d]
        w10 = ldt_amd.ResizeFiveCrop(64, ten=True).sample(sq, None, (64 - d, 64 - d))[0]
        assert w10[9].tolist() == [64, 64, c, d - c]
    # a resized image smaller than the window: emitted negative, not clipped
    small = ldt_amd.ResizeFiveCrop(32).sample(np.array([[40, 40]], np.int32), None, (48, 48))[0].tolist()
    assert small == [[32, 32, 0, 0], [32, 32, 0, -16], [32, 32, -16, 0], [32, 32, -16, -16], [32, 32, -8, -8]]
    # unknown rows: (out_h, out_w, 0, 0) windows, (0, 0, 1, 1, 0) boxes, whatever ten says
    fc = ldt_amd.ResizeFiveCrop(64, ten=True)
    st = np.array([0, 3, 0], np.int32)
    whu = np.array([[100, 80], [40, 40], [0, 0]], np.int32)
    w = fc.sample(whu, st, (48, 48))
    assert w[1].tolist() == [[48, 48, 0, 0]] * 10 and w[2].tolist() == [[48, 48, 0, 0]] * 10
    b = fc.boxes(whu, st)
    assert b.dtype == np.int32 and b.shape == (3, 10, 5)
    assert b[0].tolist() == [[0, 0, 80, 100, 0]] * 5 + [[0, 0, 80, 100, 1]] * 5
    assert b[1].tolist() == [[0, 0, 1, 1, 0]] * 10 and b[2].tolist() == [[0, 0, 1, 1, 0]] * 10
    assert ldt_amd.ResizeFiveCrop(64).boxes(whu, st)[0].tolist() == [[0, 0, 80, 100, 0]] * 5
    # [n, V, 2] sizes (the whole-image boxes of ten-crop) are the [n, 2] ones
    assert np.array_equal(fc.sample(np.repeat(whu[:, None, :], 10, axis=1), st, (48, 48)), w)
    # pickle, no RNG, views
    import torch

    before = torch.get_rng_state()
    fc.sample(whu, st, (48, 48))
    assert torch.equal(before, torch.get_rng_state())
    back = pickle.loads(pickle.dumps(fc))
    assert (back.edge, back.ten, back.views) == (64, True, 10) and np.array_equal(back.sample(whu, st, (48, 48)), w)
    assert ldt_amd.ResizeFiveCrop(64).views == 5
    with pytest.raises(ValueError):
        fc.sample(whu, st, (48, 48), views=5)
    with pytest.raises(TypeError):
        ldt_amd.ResizeFiveCrop(64.0)
    with pytest.raises(ValueError):
        ldt_amd.ResizeFiveCrop(0)


def test_resize_center_crop_with_views():
    import ldt_amd

    rc = ldt_amd.ResizeCenterCrop(64)
    wh = np.array([[100, 80], [50, 60], [0, 0]], np.int32)
    one = rc.sample(wh, None, (48, 48))
    got = rc.sample(wh, None, (48, 48), views=3)
    assert got.shape == (3, 3, 4) and got.dtype == np.int32
    assert np.array_equal(got, np.repeat(one[:, None, :], 3, axis=1))  # [n, 2] is replicated
    # [n, V, 2]: the drawn boxes' sizes, one per view
    whv = np.array([[[100, 80], [30, 90], [64, 64]], [[50, 60], [10, 10], [200, 100]], [[5, 5], [6, 6], [7, 7]]], np.int32)
    st = np.array([0, 0, 2], np.int32)
    got = rc.sample(whv, st, (48, 48), views=3)
    for i in range(3):
        assert np.array_equal(got[i], rc.sample(whv[i], np.repeat(st[i], 3), (48, 48)))
    assert got[2].tolist() == [[48, 48, 0, 0]] * 3
    with pytest.raises(ValueError):
        rc.sample(whv, st, (48, 48), views=2)
    with pytest.raises(ValueError):
        rc.sample(whv, st, (48, 48))


# ---- the sampler's draw order --------------------------------------------------------------------

@pytest.mark.parametrize("views", [1, 2, 5])
def test_sampler_draw_order_with_views(views):
    import torch

    from ldt_amd import RandomResizedCropFlip

    wh = np.array([[500, 375], [64, 80], [0, 0], [33, 40], [1, 1], [8, 800], [13, 17]], np.int32)
    st = np.array([0, 0, 1, 0, 0, 0, 0], np.int32)
    n = len(wh)
    ga, gb = torch.Generator().manual_seed(31), torch.Generator().manual_seed(31)
    got = RandomResizedCropFlip(generator=ga).sample(wh, st, views=views)
    want = RandomResizedCropFlip(generator=gb).sample(np.repeat(wh, views, axis=0), np.repeat(st, views))
    assert got.dtype == np.int32 and got.shape == (n, views, 5)
    assert np.array_equal(got, want.reshape(n, views, 5))
    assert torch.equal(ga.get_state(), gb.get_state()), "views=V consumed the RNG differently"
    # an unknown row: (0, 0, 1, 1, 0) in every view, and nothing drawn for it
    assert got[2].tolist() == [[0, 0, 1, 1, 0]] * views
    gc = torch.Generator().manual_seed(31)
    keep = [0, 1, 3, 4, 5, 6]
    assert np.array_equal(RandomResizedCropFlip(generator=gc).sample(wh[keep], views=views), got[keep])
    assert torch.equal(gc.get_state(), ga.get_state())
    if views > 1:  # the views of an image differ: each has its own draws
        assert not np.array_equal(got[0, 0], got[0, 1])
    # views=None is the [n, 5] array of before
    gd = torch.Generator().manual_seed(31)
    assert RandomResizedCropFlip(generator=gd).sample(wh, st).shape == (n, 5)
    for bad in (0, 17, True, 2.0):
        with pytest.raises(ValueError):
            RandomResizedCropFlip().sample(wh, st, views=bad)


# ---- arguments -------------------------------------------------------------------------------------

def test_check_views():
    import ldt_amd
    from ldt_amd import _lib

    assert ldt_amd.check_views is _lib.check_views
    assert ldt_amd.check_views(None) is None
    for v in (1, 2, 16, np.int32(5), np.int64(10)):
        got = ldt_amd.check_views(v)
        assert got == int(v) and type(got) is int
    for bad in (True, False, 0, 17, -1, 2.0, 2.5, "2", [2], (2,), np.float32(2)):
        with pytest.raises(ValueError, match="views"):
            ldt_amd.check_views(bad)
    assert _lib.MAX_VIEWS == 16 and "ldt_set_views" in _lib.EXPORTED


def test_check_crops_and_windows_with_views():
    from ldt_amd import check_crops, check_windows

    c = np.zeros((3, 2, 5), np.int64)
    w = np.zeros((3, 2, 4), np.int64)
    assert check_crops(c, 3, 2).shape == (3, 2, 5) and check_crops(c, 3, 2).dtype == np.int32
    assert check_windows(w, 3, 2).shape == (3, 2, 4) and check_windows(w, 3, 2).flags["C_CONTIGUOUS"]
    assert check_crops(None, 3, 2) is None and check_windows(None, 3, 2) is None
    assert check_crops(np.zeros((3, 1, 5), np.int32), 3, 1).shape == (3, 1, 5)
    for bad in (np.zeros((3, 5), np.int32), np.zeros((6, 5), np.int32), np.zeros((3, 3, 5), np.int32),
                np.zeros((2, 2, 5), np.int32), np.zeros((3, 2, 4), np.int32)):
        with pytest.raises(ValueError):
            check_crops(bad, 3, 2)
    for bad in (np.zeros((3, 4), np.int32), np.zeros((6, 4), np.int32), np.zeros((3, 3, 4), np.int32),
                np.zeros((3, 2, 5), np.int32)):
        with pytest.raises(ValueError):
            check_windows(bad, 3, 2)
    with pytest.raises(ValueError):  # and a 3-D array without views
        check_crops(c, 3)
    with pytest.raises(ValueError):
        check_windows(w, 3)


def test_views_arguments_default_to_none():
    """Every entry point has a ``views`` parameter defaulting to None;
    ``resize_raw`` does not take it."""
    import ldt_amd
    from ldt_amd import transforms as T

    for fn in (T.decode_arrow, T.ResidentBatch.decode, T.collate_fn, T.make_collate_fn, T.DeviceBatch.__init__,
               T.make_to_tensor_fn, T.DecodePipeline.__init__, ldt_amd.RandomResizedCropFlip.sample,
               ldt_amd.ResizeCenterCrop.sample, ldt_amd.ResizeFiveCrop.sample):
        assert inspect.signature(fn).parameters["views"].default is None, fn
    assert "views" not in inspect.signature(T.resize_raw).parameters
    assert "views" in (T.decode_tensor_image.__doc__ or "")
    for name in ("ResizeFiveCrop", "check_views"):
        assert hasattr(ldt_amd, name)
    fn = pickle.loads(pickle.dumps(ldt_amd.make_collate_fn(views=2, crop=ldt_amd.RandomResizedCropFlip())))
    assert isinstance(fn.crop, ldt_amd.RandomResizedCropFlip) and fn.views == 2
    # a ResizeFiveCrop implies its views; a different explicit value, or a crop with ten-crop, is refused
    fn = pickle.loads(pickle.dumps(ldt_amd.make_collate_fn(window=ldt_amd.ResizeFiveCrop(64, ten=True), size=(48, 48))))
    assert fn.views == 10 and isinstance(fn.window, ldt_amd.ResizeFiveCrop)
    assert ldt_amd.make_collate_fn(window=ldt_amd.ResizeFiveCrop(64), views=5).views == 5
    with pytest.raises(ValueError):
        ldt_amd.make_collate_fn(window=ldt_amd.ResizeFiveCrop(64), views=2)
    with pytest.raises(ValueError):
        ldt_amd.make_collate_fn(window=ldt_amd.ResizeFiveCrop(64, ten=True), crop=ldt_amd.RandomResizedCropFlip())
    for bad in (0, 17, True, 1.0):
        with pytest.raises(ValueError):
            ldt_amd.make_collate_fn(views=bad)
    # a worker-side batch validates without a device, too
    packed = T._pack_list([b"x", b"y"], [1, 2])
    assert T.DeviceBatch(packed, views=3, crop=np.zeros((2, 3, 5), np.int32))._views == 3
    with pytest.raises(ValueError):
        T.DeviceBatch(packed, views=3, crop=np.zeros((2, 5), np.int32))


# ---- the planner with views under sanitizers -------------------------------------------------------

def test_planner_with_views_under_sanitizers(tmp_path):
    from ldt_amd import synth

    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "views_plan_check")
    src = [os.path.join(REPO, "tests", "fuzz", "views_plan_check.cpp"),
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
    assert lines[-1] == "views_plan_ok"
    sizes = [tuple(int(v) for v in x.split()[1:]) for x in lines if x.startswith("size ")]
    assert sizes == [oracle.jpeg_info(c)[:2] for c in cells]
