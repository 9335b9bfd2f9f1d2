"""CPU tests of the blur's arithmetic: csrc/ldt_blur.hpp, the one source the
blur kernel and ``ldt_blur_weights`` run, compiled for the host (tools/checks/
blur_host.cpp, -ffp-contract=off) and called through ctypes on numpy arrays,
against Pillow's ``ImageFilter.GaussianBlur`` itself. Zero mismatched bytes are
allowed anywhere:

  * sizes 1x1, 1x7, 5x3, 2x2, 17x33, 96x96, 224x224 and 129x257 (the 1- and
    2-pixel axes are shorter than ``r + 1``) at radii 0, 0.01, 0.1, 0.3, 0.5,
    0.57, 0.9, 1.0 (where the float32 division of ``ww`` matters), 1.37, 1.4142
    (where ``l`` steps from 0 to 1), 1.5, 2, 3.3, 5 and 8.0, plus 30 radii
    drawn from U(0.1, 2), on random and on 0/255-only images;
  * a sweep of radii 0..8 in steps of 0.002 on a 9x11 image;
  * the weights of radii 0.1, 2.0 and 8.0;
  * blur commutes with a horizontal mirror.

A stand-alone build of the same file under ASan / UBSan runs the sweep once
more. The GPU side is tests/test_gpu_blur.py.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

SRC = os.path.join(REPO, "tools", "checks", "blur_host.cpp")
SIZES = ((1, 1), (1, 7), (5, 3), (2, 2), (17, 33), (96, 96), (224, 224), (129, 257))  # (h, w)
RADII = (0, 0.01, 0.1, 0.3, 0.5, 0.57, 0.9, 1.0, 1.37, 1.4142, 1.5, 2, 3.3, 5, 8.0)


def _cxx():
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("blur_host") / "libblur_host.so")
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so], check=True)
    L = ctypes.CDLL(so)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    L.blur_host_weights.argtypes = [ctypes.c_float, vp, vp]
    L.blur_host_pair_ok.argtypes = [i32, ctypes.c_uint32]
    L.blur_host_image.argtypes = [vp, i32, i32, i32, i32, ctypes.c_uint32, vp]
    L.blur_host_image.restype = None
    return L


def _weights(host, radius):
    r, ww = ctypes.c_int32(), ctypes.c_uint32()
    assert host.blur_host_weights(radius, ctypes.byref(r), ctypes.byref(ww)) == 0, radius
    return r.value, ww.value


def _blur(host, a, radius):
    a = np.ascontiguousarray(a)
    r, ww = _weights(host, radius)
    out = np.empty_like(a)
    host.blur_host_image(a.ctypes.data, a.shape[0], a.shape[1], a.shape[2], r, ww, out.ctypes.data)
    return out


def _pillow(a, radius):
    from PIL import Image, ImageFilter

    return np.asarray(Image.fromarray(a, "RGB").filter(ImageFilter.GaussianBlur(radius)))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_against_pillow(host, size):
    rng = np.random.default_rng(size[0] * 1000 + size[1])
    drawn = [float(v) for v in np.random.default_rng(5).uniform(0.1, 2.0, 30)]
    images = (rng.integers(0, 256, size + (3,), dtype=np.uint8),
              (rng.integers(0, 2, size + (3,), dtype=np.uint8) * 255).astype(np.uint8))
    for kind, a in enumerate(images):
        for radius in RADII + tuple(drawn):
            bad = np.count_nonzero(_blur(host, a, radius) != _pillow(a, radius))
            assert bad == 0, (size, kind, radius, bad)


def test_radius_sweep(host):
    a = np.random.default_rng(911).integers(0, 256, (9, 11, 3), dtype=np.uint8)
    for k in range(4001):
        radius = k * 0.002
        r, ww = _weights(host, radius)
        assert host.blur_host_pair_ok(r, ww) == 1, (radius, r, ww)
        bad = np.count_nonzero(_blur(host, a, radius) != _pillow(a, radius))
        assert bad == 0, (radius, bad)


def test_reference_weights(host):
    """(r, ww, fw) of the radii at the ends of the samplers' range and at the limit."""
    for radius, r, ww, fw in ((0.1, 0, 16721291, 27962), (2.0, 1, 4473924, 1677722), (8.0, 7, 1052688, 493448)):
        assert _weights(host, radius) == (r, ww)
        assert ((1 << 24) - (2 * r + 1) * ww) // 2 == fw
    assert _weights(host, 1.0) == (0, 11184811)  # the float32 quotient; 11184810 in double
    assert _weights(host, 0.0) == (0, 1 << 24)


def test_bad_radii(host):
    r, ww = ctypes.c_int32(), ctypes.c_uint32()
    for radius in (-0.5, 8.01, 9.0, 1e30, float("inf"), float("nan")):
        assert host.blur_host_weights(radius, ctypes.byref(r), ctypes.byref(ww)) == -1, radius
    assert host.blur_host_pair_ok(8, 900000) == 0
    assert host.blur_host_pair_ok(1, 4473924) == 1
    assert host.blur_host_pair_ok(1, (1 << 24) // 3 + 1) == 0  # (2r + 1) * ww > 2^24
    assert host.blur_host_pair_ok(1, (1 << 24) // 5 - 1) == 0  # (2r + 3) * ww < 2^24


def test_radius_zero_is_identity(host):
    a = np.random.default_rng(3).integers(0, 256, (17, 33, 3), dtype=np.uint8)
    assert np.array_equal(_blur(host, a, 0.0), a)


@pytest.mark.parametrize("radius", [0.4, 1.0, 1.9, 3.0])
def test_mirror_commutes(host, radius):
    """MoCo's "blur, then flip" is this library's "flip, then blur"."""
    a = np.random.default_rng(17).integers(0, 256, (33, 47, 3), dtype=np.uint8)
    assert np.array_equal(_blur(host, a[:, ::-1], radius), _blur(host, a, radius)[:, ::-1])
    assert np.array_equal(_pillow(np.ascontiguousarray(a[:, ::-1]), radius), _blur(host, a, radius)[:, ::-1])


def test_sweep_under_sanitizers(tmp_path):
    exe = str(tmp_path / "blur_host")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", "-DBLUR_HOST_MAIN", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "blur ok" in r.stdout
