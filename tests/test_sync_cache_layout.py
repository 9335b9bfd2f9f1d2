"""The sync cache's table layout, index and hint validation under
AddressSanitizer + UBSan (CPU).

lance-distributed-training_amd/csrc/ldt_sync_cache.hpp is HIP-free: the
budget-to-entries arithmetic, the byte ranges of headers and payloads, the set
index, the geometry and state words, and ``hints_plausible`` /
``hints_sum_ok``, which every hint passes before k_huff_image lets it place a
block or a reader. tests/fuzz/sync_cache_layout.cpp drives them alone, built
with ``-fsanitize=address,undefined`` in the manner of tests/test_plan_fuzz.py:

* budgets too small for one set, exactly one set, 1 MiB, the default 1024 MiB
  (131,072 entries), the cap; every header and payload range touched inside a
  buffer of exactly the table's size, each exactly once;
* slot counts 1, 2, 1023 and 1024, 1 and 256 segments, segments of a single
  slot (and of no bits), block counts at kRecCap and above, and 3000 random
  geometries: hints shaped like a converged decode are accepted, what the
  write pass derives from them (seek positions, first blocks, limits, units)
  stays inside the segment and the image, and every single-field damage
  outside the ranges is rejected.

Any sanitizer report fails the run (-fno-sanitize-recover=all).
"""
import os
import shutil
import subprocess

import pytest

from conftest import REPO

SRC = os.path.join(REPO, "tests", "fuzz", "sync_cache_layout.cpp")
INC = os.path.join(REPO, "lance-distributed-training_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("sync_cache") / "sync_cache_layout")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", INC, SRC, "-o", exe], check=True)
    return exe


def test_layout_and_validation(driver):
    r = subprocess.run([driver], capture_output=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and not r.stderr, (out[-2000:], r.stderr.decode(errors="replace")[-4000:])
    last = out.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 100000, out[-500:]


def test_header_is_hip_free():
    """The header compiles for the host alone, with no HIP include path."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", INC, "-x", "c++", "-"],
                       input=b'#include "ldt_sync_cache.hpp"\nint main() { return (int)ldt::sc_sets(0); }\n',
                       capture_output=True)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
