"""CPU test of the filtered affine op's arithmetic: csrc/ldt_augment.hpp's
aug_filt_* compiled for the host (tools/checks/affine_filter_host.cpp,
-ffp-contract=off) against Pillow's own ``Image.transform(size, AFFINE, m,
BILINEAR | BICUBIC, fillcolor=fill)``: zero mismatched bytes, and no tap outside
the source box the kernel stages for its 16 x 64 tile. The GPU side is
tests/test_gpu_affine_filter.py.
"""
import ctypes
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

from conftest import REPO

FILTERS = {"bilinear": (1, Image.BILINEAR), "bicubic": (2, Image.BICUBIC)}
SIZES = ((1, 1), (2, 3), (9, 11), (33, 65))  # (h, w)
FILLS = ((0, 0, 0), (12, 200, 99))
MATRICES = ("identity", "half", "rot30", "rot45", "shearx", "shift3", "scale3", "scale1/3", "outside")


def matrix(name, h, w):
    """The issue's matrices, output -> input, for an (h, w) image."""
    from ldt_amd.augment import affine_matrix

    return [float(v) for v in {
        "identity": (1, 0, 0, 0, 1, 0), "half": (1, 0, 0.5, 0, 1, 0.5), "shift3": (1, 0, 3, 0, 1, 0),
        "scale3": (3, 0, 0, 0, 3, 0), "scale1/3": (1 / 3, 0, 0, 0, 1 / 3, 0), "outside": (1, 0, 1e6, 0, 1, 0),
        "rot30": affine_matrix("Rotate", 30.0, (h, w)), "rot45": affine_matrix("Rotate", 45.0, (h, w)),
        "shearx": affine_matrix("ShearX", 0.99, (h, w))}[name]]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("affine_filter_host") / "libaffine_filter_host.so")
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                    f"{REPO}/tools/checks/affine_filter_host.cpp", "-o", so], check=True)
    L = ctypes.CDLL(so)
    L.affine_filter_host_run.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p]
    L.affine_filter_host_run.restype = ctypes.c_int
    return L


def test_python_mirrors_the_kernels_tile_constants(host):
    """_lib.AFFINE_TILE and AFFINE_LDS_TEXELS, from which the GPU test shows that its fallback case runs."""
    from ldt_amd import _lib

    c = (ctypes.c_int * 3)()
    host.affine_filter_host_consts(c)
    assert (tuple(c[:2]), c[2]) == (_lib.AFFINE_TILE, _lib.AFFINE_LDS_TEXELS)


def test_filter_arguments_and_rows_are_validated():
    from ldt_amd import RandAugment, TrivialAugmentWide, _lib

    for value, code in ((None, 0), ("nearest", 0), (0, 0), ("Bilinear", 1), (2, 1), (Image.BICUBIC, 2), (3, 2)):
        assert _lib.check_affine_filter(value) == code
    for bad in (1, "lanczos", True, 2.5):
        with pytest.raises(ValueError):
            TrivialAugmentWide(affine_filter=bad)
    assert "affine_filter='bicubic'" in repr(RandAugment(affine_filter=3))
    assert "affine_filter" not in repr(RandAugment())
    row = [1.0, 3.0, 0, 0, 0, 3.0, 0, 1, 2, 3]  # a pure scale: refused as NEAREST, taken under a filter
    with pytest.raises(ValueError):
        _lib.check_augments(np.array([[row]]), 1)
    rec = _lib.check_augments(np.array([[row + [2.0]]]), 1)
    assert rec.dtype == _lib.aug_filt_dtype() and rec["filt"][0, 0]["filter"] == 2 and rec["op"][0, 0]["code"] == 1
    assert list(rec["filt"][0, 0]["m"]) == row[1:7] and list(rec["op"][0, 0]["fill"]) == [1, 2, 3]
    assert _lib.check_augments(np.array([[row[:1] + [1.0, 0, 0, 0, 1.0, 0, 1, 2, 3, 0.0]]]), 1).dtype == _lib.aug_dtype()
    for bad in (row + [3.0], row + [1.5], [2.0, 1.0] + row[2:] + [1.0], [1.0, float("inf")] + row[2:] + [1.0],
                [1.0, 2.0 ** 31] + row[2:] + [1.0]):
        with pytest.raises(ValueError):
            _lib.check_augments(np.array([[bad]]), 1)


@pytest.mark.parametrize("name", MATRICES)
@pytest.mark.parametrize("filt", sorted(FILTERS))
def test_filtered_affine_matches_pillow(host, filt, name):
    code, resample = FILTERS[filt]
    for h, w in SIZES:
        rgb = np.random.default_rng(977 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
        m = np.array(matrix(name, h, w), np.float64)
        for fill in FILLS:
            want = np.asarray(Image.fromarray(rgb).transform((w, h), Image.AFFINE, list(m), resample, fillcolor=fill))
            got = np.empty_like(rgb)
            escaped = host.affine_filter_host_run(rgb.ctypes.data, h, w, code, m.ctypes.data,
                                                  np.array(fill, np.uint8).ctypes.data, got.ctypes.data)
            assert escaped == 0, (filt, name, h, w)
            assert int((got != want).sum()) == 0, (filt, name, h, w, fill)
            if name == "outside":
                assert (want == np.array(fill, np.uint8)).all()
