"""CPU test of what the band kernel (k_resize4) relies on without its clamps
and without the boundary rows no output row reads: tools/checks/trim_check.cpp,
stand-alone under ASan/UBSan. With resample_coeffs (csrc/ldt_resample.hpp) every
BILINEAR weight is >= 0 and every row of weights sums to at most 4,202,528, the
largest sum for which 255 * sum + 2^21 stays below 256 * 2^22 (so a tap sum's
bits 22..29 are the byte and Pillow's clip8 never fires); with make_geom4
(csrc/ldt_geom4.hpp) the rows a band skips (the first pair's row below the
band's first source row, the last pair's row at or past its end) lie in no
output row's window, and every row in a window is staged. The sweep is the one
the program's header lists. The GPU side is tests/test_gpu_resize4_trim.py.
"""
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def test_row_sums_and_skipped_rows(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "trim_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(REPO, "tools", "checks", "trim_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "trim ok" in r.stdout
