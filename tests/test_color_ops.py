"""CPU tests of the photometric stage's arithmetic: csrc/ldt_color.hpp, the one
source the colour kernels run, compiled for the host (tools/checks/
color_host.cpp, -ffp-contract=off) and called through ctypes on numpy arrays,
against Pillow itself. Zero mismatches are allowed anywhere:

  * ``convert("L")``, RGB -> HSV and HSV -> RGB on all 2^24 inputs;
  * ``ImageEnhance.Brightness`` / ``Color`` / ``Contrast`` (``Image.blend`` with
    a degenerate image) on a random 96 x 96 image at factors below, at and
    above 1;
  * the integer contrast mean against ``int(ImageStat.Stat(L).mean[0] + 0.5)``
    on 200 random images, 1 x 1 and all-255 included;
  * ``ImageOps.solarize`` at thresholds 0, 1, 128, 255, 256;
  * torchvision's ``adjust_hue`` restated on PIL (``convert("HSV")``, a uint8
    wrap-add on H, ``convert("RGB")``) and the grayscale.

A stand-alone build of the same file under ASan / UBSan sweeps the functions
once more (every RGB and HSV value, every blend class, every order). The GPU
side is tests/test_gpu_color.py.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

SRC = os.path.join(REPO, "tools", "checks", "color_host.cpp")
FACTORS = (0.0, 0.33333, 0.6, 0.61234567, 0.999, 1.0, 1.39999, 1.4, 1.7, 2.5)


def _cxx():
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("color_host") / "libcolor_host.so")
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so], check=True)
    L = ctypes.CDLL(so)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.color_host_l.argtypes = [vp, i64, vp]
    L.color_host_rgb2hsv.argtypes = [vp, i64, vp]
    L.color_host_hsv2rgb.argtypes = [vp, i64, vp]
    L.color_host_mean_round.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    L.color_host_mean.argtypes = [vp, i64, vp]
    L.color_host_chain.argtypes = [vp, i64, vp, ctypes.c_int, vp]
    for f in ("color_host_l", "color_host_rgb2hsv", "color_host_hsv2rgb", "color_host_chain"):
        getattr(L, f).restype = None
    return L


@pytest.fixture(scope="module")
def cube():
    """All 2^24 byte triples as a 4096 x 4096 x 3 image."""
    v = np.arange(1 << 24, dtype=np.uint32)
    a = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def image():
    return np.random.default_rng(20260).integers(0, 256, (96, 96, 3), dtype=np.uint8)


def _entry(**kw):
    """One ldt_color record from (brightness, contrast, saturation, hue, order, gray, solarize)."""
    from ldt_amd import _lib

    row = [kw.get("brightness", np.nan), kw.get("contrast", np.nan), kw.get("saturation", np.nan),
           kw.get("hue", np.nan), kw.get("order", 0 + 4 * 1 + 16 * 2 + 64 * 3), kw.get("gray", 0),
           kw.get("solarize", -1)]
    return _lib.check_colors(np.array([row], np.float64), 1)


def _chain(host, rgb, entry):
    """The kernels' two passes on an [h, w, 3] image: the mean, then the chain."""
    rgb = np.ascontiguousarray(rgb)
    n = rgb.shape[0] * rgb.shape[1]
    mean = host.color_host_mean(rgb.ctypes.data, n, entry.ctypes.data) if entry["mask"][0] & 2 else 0
    out = np.empty_like(rgb)
    host.color_host_chain(rgb.ctypes.data, n, entry.ctypes.data, mean, out.ctypes.data)
    return out


def test_l_all_rgb(host, cube):
    from PIL import Image

    got = np.empty((4096, 4096), np.uint8)
    host.color_host_l(cube.ctypes.data, 1 << 24, got.ctypes.data)
    want = np.asarray(Image.fromarray(cube, "RGB").convert("L"))
    assert np.count_nonzero(got != want) == 0


def test_rgb2hsv_all_rgb(host, cube):
    from PIL import Image

    got = np.empty_like(cube)
    host.color_host_rgb2hsv(cube.ctypes.data, 1 << 24, got.ctypes.data)
    want = np.asarray(Image.fromarray(cube, "RGB").convert("HSV"))
    assert np.count_nonzero(got != want) == 0


def test_hsv2rgb_all_hsv(host, cube):
    from PIL import Image

    got = np.empty_like(cube)
    host.color_host_hsv2rgb(cube.ctypes.data, 1 << 24, got.ctypes.data)
    want = np.asarray(Image.frombytes("HSV", (4096, 4096), cube.tobytes()).convert("RGB"))
    assert np.count_nonzero(got != want) == 0


@pytest.mark.parametrize("factor", FACTORS)
def test_blend_against_image_enhance(host, image, factor):
    from PIL import Image, ImageEnhance

    im = Image.fromarray(image, "RGB")
    for name, enh in (("brightness", ImageEnhance.Brightness), ("saturation", ImageEnhance.Color),
                      ("contrast", ImageEnhance.Contrast)):
        want = np.asarray(enh(im).enhance(factor))
        got = _chain(host, image, _entry(**{name: factor}))
        assert np.count_nonzero(got != want) == 0, (name, factor)


def test_contrast_mean_against_image_stat(host):
    from PIL import Image, ImageStat

    rng = np.random.default_rng(7)
    entry = _entry(contrast=1.0)
    images = [np.full((1, 1, 3), 255, np.uint8), np.zeros((1, 1, 3), np.uint8), np.full((33, 17, 3), 255, np.uint8),
              np.full((1024, 1024, 3), 255, np.uint8)]
    while len(images) < 200:
        h, w = (int(v) for v in rng.integers(1, 80, 2))
        lo = int(rng.integers(0, 255))
        images.append(rng.integers(lo, min(256, lo + int(rng.integers(1, 256))), (h, w, 3), dtype=np.uint8))
    for a in images:
        a = np.ascontiguousarray(a)
        want = int(ImageStat.Stat(Image.fromarray(a, "RGB").convert("L")).mean[0] + 0.5)
        got = host.color_host_mean(a.ctypes.data, a.shape[0] * a.shape[1], entry.ctypes.data)
        assert got == want, (a.shape, got, want)
    # the quotient itself, at the halves a 2 x 2 and a 1024 x 1024 image can reach
    for s, c in ((1, 2), (2, 4), (6, 4), (1 << 19, 1 << 20), ((1 << 19) - 1, 1 << 20), (255 << 20, 1 << 20)):
        assert host.color_host_mean_round(s, c) == int(s / c + 0.5)


@pytest.mark.parametrize("threshold", [0, 1, 128, 255, 256])
def test_solarize(host, image, threshold):
    from PIL import Image, ImageOps

    want = np.asarray(ImageOps.solarize(Image.fromarray(image, "RGB"), threshold))
    assert np.count_nonzero(_chain(host, image, _entry(solarize=threshold)) != want) == 0


@pytest.mark.parametrize("hue", [-0.5, -0.1, 0.0, 0.1, 0.5])
def test_hue_and_gray(host, image, hue):
    from PIL import Image

    im = Image.fromarray(image, "RGB")
    h, s, v = im.convert("HSV").split()
    nh = (np.asarray(h, np.uint8).astype(np.int64) + int(hue * 255)).astype(np.uint8)  # a uint8 wrap-add
    want = Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")
    assert np.count_nonzero(_chain(host, image, _entry(hue=hue)) != np.asarray(want)) == 0
    gray = np.asarray(want.convert("L"))
    got = _chain(host, image, _entry(hue=hue, gray=1))
    assert np.count_nonzero(got != np.stack([gray] * 3, axis=-1)) == 0


def test_all_orders_against_pillow(host, image):
    """All four ops in each of the 24 orders: the contrast mean depends on what preceded it."""
    import itertools

    from PIL import Image, ImageEnhance

    def hue_op(im, shift):
        h, s, v = im.convert("HSV").split()
        nh = (np.asarray(h, np.uint8).astype(np.int64) + shift).astype(np.uint8)
        return Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")

    ops = {0: lambda im: ImageEnhance.Brightness(im).enhance(1.3), 1: lambda im: ImageEnhance.Contrast(im).enhance(0.7),
           2: lambda im: ImageEnhance.Color(im).enhance(1.9), 3: lambda im: hue_op(im, int(-0.1 * 255))}
    for perm in itertools.permutations(range(4)):
        im = Image.fromarray(image, "RGB")
        for op in perm:
            im = ops[op](im)
        entry = _entry(brightness=1.3, contrast=0.7, saturation=1.9, hue=-0.1,
                       order=perm[0] + 4 * perm[1] + 16 * perm[2] + 64 * perm[3])
        assert np.count_nonzero(_chain(host, image, entry) != np.asarray(im)) == 0, perm


def test_sweep_under_sanitizers(tmp_path):
    exe = str(tmp_path / "color_host")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", "-DCOLOR_HOST_MAIN", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "color ok" in r.stdout
