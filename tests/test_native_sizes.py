"""CPU tests of ``decode_native(sizes=)``: the two size helpers against the upstream rules, the argument
checks (no device), and the planner of a native call with per-row sizes through its host entry."""
import ctypes
import io
import math
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

# (width, height): upright, landscape, square, the max_size clamp both ways, SmartResize's min and max branches
GRID = [(480, 640), (640, 480), (512, 512), (500, 375), (3000, 500), (333, 2000), (33, 31), (20, 20), (8, 300),
        (8000, 6000), (1, 1), (57, 85), (1333, 800)]


def _tv_resize(w, h, edge, max_size):  # torchvision 0.2x _compute_resized_output_size, (h, w)
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = edge, int(edge * long / short)
    if max_size is not None and new_long > max_size:
        new_short, new_long = int(max_size * new_short / new_long), max_size
    return (new_long, new_short) if w <= h else (new_short, new_long)


def _smart_resize(h, w, factor, min_pixels, max_pixels):  # Qwen2-VL image_processing smart_resize
    if max(h, w) / min(h, w) > 200:
        raise ValueError("ratio")
    hb, wb = max(factor, round(h / factor) * factor), max(factor, round(w / factor) * factor)
    if hb * wb > max_pixels:
        beta = math.sqrt((h * w) / max_pixels)
        hb, wb = math.floor(h / beta / factor) * factor, math.floor(w / beta / factor) * factor
    elif hb * wb < min_pixels:
        beta = math.sqrt(min_pixels / (h * w))
        hb, wb = math.ceil(h * beta / factor) * factor, math.ceil(w * beta / factor) * factor
    return hb, wb


@pytest.mark.parametrize("edge, max_size", [(800, 1333), (256, None), (31, 32)])
def test_resize_shortest_edge(edge, max_size):
    import ldt_amd

    helper = pickle.loads(pickle.dumps(ldt_amd.ResizeShortestEdge(edge, max_size)))
    got = helper.sizes(np.array(GRID + [(0, 0)]), np.array([0] * len(GRID) + [1]))
    assert got.dtype == np.int32 and got.tolist() == [list(_tv_resize(w, h, edge, max_size)) for w, h in GRID] + [[1, 1]]
    with pytest.raises(ValueError):
        ldt_amd.ResizeShortestEdge(800, 800)


@pytest.mark.parametrize("kw", [{}, dict(factor=14, min_pixels=4 * 196, max_pixels=64 * 196)])
def test_smart_resize(kw):
    import ldt_amd

    helper = pickle.loads(pickle.dumps(ldt_amd.SmartResize(**kw)))
    p = dict(dict(factor=28, min_pixels=56 * 56, max_pixels=14 * 14 * 4 * 1280), **kw)
    want = [list(_smart_resize(h, w, **p)) for w, h in GRID]
    assert helper.sizes(np.array(GRID)).tolist() == want
    assert any(h * w > p["max_pixels"] for w, h in GRID) and any(h * w < p["min_pixels"] for w, h in GRID)
    with pytest.raises(ValueError, match="aspect ratio"):
        helper.sizes([[2010, 10]])


@pytest.mark.parametrize("kw", [dict(sizes=[[8, 8, 8]]), dict(sizes=[[8, 8], [8, 8]]), dict(sizes=[[8.0, 8.0]]),
                                dict(interpolation="bicubic"), dict(sizes=[[8, 8]], interpolation="lanczos"),
                                dict(sizes=[[8, 8]], interpolation=0)])
def test_bad_arguments_need_no_device(monkeypatch, kw):
    import ldt_amd
    from ldt_amd import synth, transforms as T

    class Asked(Exception):
        pass

    def no_device(device):
        raise Asked

    monkeypatch.setattr(T, "_decoder", no_device)
    cell = [synth.encode(synth.field(8, 8, 4, 12.0))]
    with pytest.raises((ValueError, TypeError)):
        ldt_amd.decode_native(cell, **kw)
    with pytest.raises(Asked):  # a good call gets as far as the device
        ldt_amd.decode_native(cell, sizes=ldt_amd.ResizeShortestEdge(16), interpolation=3, crops=[[0, 0, 4, 8, 1]])


def test_offsets_come_from_the_sizes():
    import ldt_amd
    from ldt_amd import synth, transforms as T

    cells = [synth.encode(synth.field(31, 33, 1, 12.0)), b"", synth.encode(synth.field(45, 67, 2, 12.0))]
    plan = T._native_plan(cells, None, [1, 1, 2], ldt_amd.ResizeShortestEdge(10))
    assert plan[5].tolist() == [[10, 10], [1, 1], [10, 14]]  # 23 x 34 after the draft: 10 * 34 // 23
    assert plan[3].tolist() == [[10, 10], [0, 0], [10, 14]] and plan[4].tolist() == [0, 300, 300, 720]
    plan = T._native_plan(cells, [[0, 0, 8, 16, 1]] * 3, None, ldt_amd.ResizeShortestEdge(10))
    assert plan[5].tolist() == [[10, 20], [1, 1], [10, 20]]  # the boxes' sizes are what the helper sees


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    so = str(tmp_path_factory.mktemp("native_sizes") / "libnative_sizes_plan.so")
    src = [os.path.join(REPO, "tools", "checks", "native_sizes_host.cpp"),
           os.path.join(REPO, "lance-distributed-training_amd", "csrc", "ldt_plan.cpp")]
    subprocess.run([cxx, "-std=c++17", "-O1", "-shared", "-fPIC", "-ffp-contract=off", "-I/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", *src, "-o", so], check=True)
    lib = ctypes.CDLL(so)

    def plan(cells, sizes, filt=0, regions=None):
        n = len(cells)
        data = np.frombuffer(b"".join(cells) + b"\0", np.uint8)
        off = np.cumsum([0] + [len(c) for c in cells]).astype(np.int64)
        sizes = np.ascontiguousarray(sizes, np.int32)
        elems = 3 * sizes[:, 0].astype(np.int64) * sizes[:, 1] if regions is None else np.asarray(regions, np.int64)
        native = np.concatenate([[0], np.cumsum(np.maximum(elems, 0))]).astype(np.int64)
        out, ptr = np.zeros(2 * n + 9, np.int32), lambda a: ctypes.c_void_p(a.ctypes.data)
        lib.native_sizes_host_plan(ptr(data), ptr(off), ctypes.c_int64(n), ptr(native), ptr(sizes), None, filt, ptr(out))
        keys = ("native_bad", "max_ks_h", "max_ks_v", "kh_words", "ks_v", "span", "lds", "tr")
        return out[:n].tolist(), out[n:2 * n + 1].tolist(), dict(zip(keys, out[2 * n + 1:].tolist()))

    return plan


def test_planner(planner):
    from ldt_amd import synth

    cells = [synth.encode(synth.field(h, w, seed, 12.0)) for seed, (h, w) in enumerate([(45, 67), (31, 33), (20, 300)])]
    # 67 -> 600 is an upscale of three tiles, 300 -> 33 a reduction of ceil(300 / 33) = 10
    status, tiles, m = planner(cells, [[45, 600], [31, 33], [20, 33]])
    tr = m["tr"]
    per_row = [-(-45 // tr) * 3, -(-31 // tr), -(-20 // tr)]
    assert status == [0, 0, 0] and tiles == [0] + np.cumsum(per_row).tolist() and not m["native_bad"]
    assert (m["max_ks_h"], m["max_ks_v"], m["ks_v"]) == (21, 3, 3)
    # a tile's words: 256 columns of 3 taps, 33 of 3, 33 of 21; the spans: ceil(255 * 67 / 600) + 2 + 2, 33, 300
    assert m["kh_words"] == 256 * 3 and m["span"] == 300
    assert planner(cells[2:], [[20, 33]])[2]["kh_words"] == 33 * 21
    assert planner(cells[:1], [[45, 600]], 1)[2]["span"] == 29 + 4 + 2 and planner(cells[:1], [[45, 600]])[2]["span"] == 33
    # a region that is not 3 * h * w of the requested size
    assert planner(cells, [[45, 600], [31, 33], [20, 33]], regions=[3 * 45 * 600, 3 * 31 * 33 + 3, 3 * 20 * 33])[2]["native_bad"]
    # a size of 0 or above LDT_MAX_DIM, a 38-fold reduction (BICUBIC: 19-fold and a half): that row alone
    status, tiles, m = planner(cells, [[0, 33], [31, 8193], [20, 7]], regions=[5, 0, 7])
    assert status == [7, 7, 4] and tiles == [0, 0, 0, 0] and not m["native_bad"]
    assert planner(cells, [[45, 67], [31, 33], [20, 9]])[0] == [0, 0, 0]  # ceil(300 / 8) = 38 > 37 > ceil(300 / 9)
    assert planner(cells, [[45, 67], [31, 33], [20, 8]], regions=[3 * 45 * 67, 3 * 31 * 33, 1])[0] == [0, 0, 4]
    assert planner(cells, [[45, 67], [31, 33], [20, 17]], 1)[0] == [0, 0, 0]  # BICUBIC: ceil(600 / 16) = 38
    assert planner(cells, [[45, 67], [31, 33], [20, 16]], 1, regions=[3 * 45 * 67, 3 * 31 * 33, 1])[0] == [0, 0, 4]


def test_planner_lds_fits_the_widest_rows(planner):
    """The two corners of the dynamic LDS: the most coefficient words and the widest span."""
    from PIL import Image

    b = io.BytesIO()
    Image.new("L", (8192, 16), 128).save(b, format="JPEG", quality=50)
    for sizes, filt in (([[16, 222]], 0), ([[16, 256]], 0), ([[16, 8192]], 1), ([[16, 886]], 1)):
        status, _, m = planner([b.getvalue()], sizes, filt)
        assert status == [0] and m["lds"] <= 160 * 1024, (sizes, m)
