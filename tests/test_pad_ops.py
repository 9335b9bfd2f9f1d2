"""CPU test of the padded window's index map (csrc/ldt_pad.hpp, compiled for the host through tools/checks/
pad_host.cpp) against ``np.pad``: sizes 1..9, offsets -25..25, zero mismatches. GPU side: tests/test_gpu_pad.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO


@pytest.mark.parametrize("mode", ["edge", "reflect", "symmetric"])
def test_against_np_pad(mode, tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    so = str(tmp_path / "libpad_host.so")
    subprocess.run([cxx, "-std=c++17", "-O2", "-shared", "-fPIC", os.path.join(REPO, "tools", "checks", "pad_host.cpp"),
                    "-o", so], check=True)
    host, m = ctypes.CDLL(so), ["constant", "edge", "reflect", "symmetric"].index(mode)
    for n in range(1, 10):  # indices -25 .. n + 24: several folds at every size
        got = np.empty(n + 50, np.int32)
        host.pad_host_indices(m, -25, got.size, n, ctypes.c_void_p(got.ctypes.data))
        assert np.array_equal(got, np.pad(np.arange(n), 25, mode=mode)), (mode, n)
