"""CPU test of the band kernel's sizing by real tap counts:
tools/checks/taps_check.cpp, stand-alone under ASan/UBSan. For every input size
1..1120 and output sizes 1, 7, 96, 224, 255 and 256 it checks that
resample_taps_host (csrc/ldt_resample.hpp) is the largest count
resample_coeffs returns, that a row computed with Pillow's ksize is zero from
its count on, that the count stays within ksize and floor(2 * support) + 1;
it replays k_resize4's row-pair schedule for every band height make_geom4
(csrc/ldt_geom4.hpp) can choose and asserts that no ring row is overwritten
while an unfinished output row needs it; it checks that every staged dword
the horizontal taps read lies inside the wave's own LDS bytes; and it pins
the flagship geometry: 9,472 B per wave, four 4-wave workgroups in 160 KB.
The GPU side is tests/test_gpu_resize4_taps.py.
"""
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def test_taps_ring_and_staging_reads(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "taps_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-ffp-contract=off", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(REPO, "tools", "checks", "taps_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "taps ok" in r.stdout
