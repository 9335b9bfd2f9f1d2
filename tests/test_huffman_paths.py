"""The helpers of tests/test_gpu_huffman_paths.py, on the CPU.

The twins of tests/jpeg_recode.py (twin_cells): two files of equal length and
equal scan bytes, which the sync cache of k_huff_image cannot
tell apart by its key. Each must be a file the project makes a claim about:
strictly valid (jpeg_recode.strictly_valid), decoded by Pillow to other pixels
than its twin, and decoded by the oracle as Pillow decodes it. The reference
alone then carries the case.

cache_users of tests/huff_paths.py (which images of a batch consult the sync
cache) restates the planner's routing; here it is held against the planner
itself (the sanitized driver of tests/test_plan_fuzz.py) on the census batch
under every planning option the GPU census uses.
"""
import io

import numpy as np
import pytest

import huff_paths as hp
import jpeg_recode as jr
from conftest import read_golden
from oracle import oracle
from test_plan_fuzz import _plan_batch, build_planner


def _pil_rgb(b: bytes) -> np.ndarray:
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return build_planner(tmp_path_factory)


def test_twins_share_the_key_and_not_the_pixels():
    twins = jr.twin_cells()
    assert [t.same_walk for t in twins] == [True, True, False, False, False]
    for t in twins:
        assert t.a != t.b and len(t.a) == len(t.b), t.name
        assert jr.scan_bytes(t.a) == jr.scan_bytes(t.b), t.name
        # the planner's src_len: from the end of the SOS header to the end of the cell
        assert len(jr.parse(t.a)[1]) == len(jr.parse(t.b)[1]), t.name
        for x in (t.a, t.b):
            assert jr.strictly_valid(x), t.name
            assert np.array_equal(oracle.decode_rgb(x), _pil_rgb(x)), t.name
            assert np.array_equal(oracle.jpeg_to_tensor(x), oracle.pil_image_to_tensor(x)), t.name
        if t.name == "relabel-440":  # another frame: the MCUs' blocks lie elsewhere
            assert _pil_rgb(t.a).shape == _pil_rgb(t.b).shape
        assert not np.array_equal(_pil_rgb(t.a), _pil_rgb(t.b)), t.name
        assert not np.array_equal(oracle.jpeg_to_tensor(t.a), oracle.jpeg_to_tensor(t.b)), t.name
        # the same Huffman walk, or another one over the same bit positions
        same = jr.scan_symbols(t.a) == jr.scan_symbols(t.b)
        assert same == t.same_walk, t.name
        ra, rb = hp.routing(t.a), hp.routing(t.b)
        assert ra == rb and ra.sub_bits > 0, (t.name, ra, rb)
    big = next(t for t in twins if t.name.startswith("swap-512x512"))
    r = hp.routing(big.a)
    assert r.nseg == 1 and r.src_len * 8 // r.sub_bits >= 300, r  # hundreds of slots, one segment


def test_strictly_valid_refuses_what_libjpeg_only_warns_about():
    from ldt_amd import synth

    a = synth.encode(synth.field(64, 96, 40, 6.0), quality=75, subsampling="4:4:4")
    assert jr.strictly_valid(a)
    scan = len(jr.scan_bytes(a))
    cut = a[:len(a) - 2 - scan // 2] + b"\xff\xd9"
    assert not jr.strictly_valid(cut)  # MCUs missing
    assert not jr.strictly_valid(a[:-2] + b"\x00\x00\xff\xd9")  # data after the last MCU
    # ZRL for EOB in the luma AC table: runs past coefficient 63
    assert not jr.strictly_valid(jr.swap_dht_symbols(a, 1, 0, 0x00, 0xF0))
    for c in jr.sync_cells()[:3] + jr.stress_cells()[:3]:
        if "progressive" not in c.tags:
            assert jr.strictly_valid(c.data), c.name


# name -> (planner arguments, cache_users arguments): the planning options of the census
PLAN_SETTINGS = {
    "default": ((), {}),
    "bits64": (("sb=64",), {"bits": 64}),
    "window16384": (("win_cap=16384",), {"window": 16384}),
    "window0": (("win_cap=0",), {"window": 0}),
    "unfused": (("fuse=0",), {"fused": 0}),
    "serial": (("serial=1",), {"mode": 1}),
}


@pytest.mark.parametrize("setting", list(PLAN_SETTINGS))
def test_cache_users_is_the_planners_routing(planner, setting, manifest):
    """On the census batch and on the batches of the GPU tests that count
    their users with it: the sync, stress and layout cells, the goldens."""
    cells = hp.census_cells()
    args, kw = PLAN_SETTINGS[setting]
    golden = [read_golden(e["file"]) for e in manifest["images"]]
    for batch in (list(cells.values()), list(cells.values())[::-1], [cells["small-64x96"], cells["ones-big"]],
                  [c.data for c in jr.sync_cells()], [c.data for c in jr.stress_cells()],
                  [c.data for c in jr.layout_cells()], golden + [cells["q90-512"], cells["inet"]]):
        plan = _plan_batch(planner, batch, *args)
        rows, tot = plan["rows"], plan["totals"]
        assert all(r["status"] == 0 for r in rows)
        routes = [hp.routing(c, kw.get("bits", 256), kw.get("mode", 0)) for c in batch]
        for i, (r, row) in enumerate(zip(routes, rows)):
            if r is None:
                assert i in plan["prog_img"]
                continue
            assert (r.sub_bits, r.nseg, r.src_len) == (row["sub_bits"], row["nseg"], row["src_len"]), (setting, i)
        assert tot["win_bytes"] == hp.window_bytes(routes, kw.get("window", -1)), setting
        assert tot["max_tabs"] == max(r.ntabs for r in routes if r), setting
        # sc_use: the parallel decoder's images that got no destuff chunks
        fused = [i in plan["par_img"] and row["ds_count"] == 0 for i, row in enumerate(rows)]
        assert hp.cache_users(batch, **kw) == fused, (setting, fused)
        assert not any(hp.cache_users(batch, counters=1, **kw))
        assert not any(hp.cache_users(batch, cache=0, **kw)) and not any(hp.cache_users(batch, cache_mb=0, **kw))


def test_the_census_batch_reaches_every_route():
    """What the GPU census relies on: under the defaults four cells consult
    the table and the 257-segment one takes the serial decoder; a 16 KB window
    keeps the small cell only; the big stress cell is a user at the default
    window and none at 16 KB."""
    cells = hp.census_cells()
    names, batch = list(cells), list(cells.values())
    users = lambda **kw: {n for n, u in zip(names, hp.cache_users(batch, **kw)) if u}
    assert users() == set(names) - {"nseg-257"}
    assert users(bits=64) == set(names) - {"nseg-257"}
    assert users(window=16384) == {"small-64x96"}
    assert users(window=0) == users(fused=0) == users(mode=1) == set()
    assert hp.routing(cells["inet"]).nseg > 1 and hp.routing(cells["q90-512"]).nseg == 1
