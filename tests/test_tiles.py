"""CPU tests of ``decode_tiles``' host side: ``DynamicTiles`` against InternVL's rule, ``check_tiles``' refusals
(no device is asked for) and ``tile_layout``."""
import pickle

import numpy as np
import pytest

SIZES = [(512, 512), (1024, 1024), (800, 600), (1920, 1080), (375, 500), (91, 77), (5, 17), (1000, 300)]
# (min_num, max_num, tile_size) -> (cols, rows) per size, computed with upstream's dynamic_preprocess
EXPECTED = {(1, 12, 448): [(1, 1), (3, 3), (4, 3), (4, 2), (3, 4), (4, 3), (1, 3), (3, 1)],
            (1, 6, 448): [(1, 1), (2, 2), (3, 2), (2, 1), (2, 3), (1, 1), (1, 3), (3, 1)],
            (1, 4, 16): [(2, 2), (2, 2), (2, 2), (2, 1), (2, 2), (2, 2), (1, 3), (3, 1)]}


@pytest.mark.parametrize("args", sorted(EXPECTED))
def test_dynamic_tiles(args):
    import ldt_amd

    helper = pickle.loads(pickle.dumps(ldt_amd.DynamicTiles(*args)))
    got = helper.grids(np.array(SIZES + [(0, 0)]), None)
    assert got[:-1, ::-1].tolist() == [list(e) for e in EXPECTED[args]]
    assert got[-1].tolist() == [1, 1]  # an unknown size


@pytest.mark.parametrize("kw, match", [
    (dict(grids=[[1, 1], [5, 13], [1, 1]]), "row 1"),                          # 65 tiles
    (dict(grids=[[1, 1], [1, 1], [1, 41]], tile_size=200), "row 2"),           # a canvas side of 8200
    (dict(grids=[[1, 1, 20, 20, 0, 0], [1, 2, 20, 30, 0, 11], [1, 1, 20, 20, 0, 0]], tile_size=20), "row 1"),
    (dict(grids=[[1, 1, 20, 20, 0, 0], [2, 1, 20, 20, -1, 0], [1, 1, 20, 20, 0, 0]], tile_size=20), "row 1"),
    (dict(grids="helper", tile_size=224), "tile_size"),
    (dict(grids=[[1, 1]] * 3, tile_size=7), "tile_size"),
    (dict(grids=[[1, 1]] * 3, tile_size=1025), "tile_size"),
    (dict(grids=[[1, 1]] * 3, fill=256), "fill"),
])
def test_refusals_need_no_device(monkeypatch, kw, match):
    import ldt_amd
    from ldt_amd import synth
    from ldt_amd import transforms as T

    def no_device(device):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(T, "_decoder", no_device)
    if kw["grids"] == "helper":
        kw["grids"] = ldt_amd.DynamicTiles(1, 12, 448)
    cells = [synth.encode(synth.field(31, 33, 4, 12.0))] * 3
    with pytest.raises(ValueError, match=match):
        ldt_amd.decode_tiles(cells, **kw)
    with pytest.raises(ValueError, match=match):
        ldt_amd.check_tiles(kw.pop("grids"), 3, **kw)


@pytest.mark.parametrize("thumbnail, counts", [(True, [1, 5, 0, 7]), (False, [1, 4, 0, 6])])
def test_tile_layout(thumbnail, counts):
    from ldt_amd import _lib

    assert _lib.check_tiles([[1, 1], [2, 3]], 2, 20)[1].tolist() == [[20, 20], [40, 60]]  # stretched to the canvas
    grids = [[1, 1, 20, 20, 0, 0], [2, 2, 40, 40, 0, 0], [3, 3, 60, 60, 0, 0], [2, 3, 30, 50, 5, 7]]
    spec, sizes, grid = _lib.check_tiles(grids, 4, 20, thumbnail, (7, 130, 255))
    assert (spec.tile, spec.thumbnail, list(spec.fill)) == (20, int(thumbnail), [7, 130, 255])
    assert sizes.tolist() == [[20, 20], [40, 40], [60, 60], [30, 50]]
    assert grid.tolist() == [[1, 1, 0, 0], [2, 2, 0, 0], [3, 3, 0, 0], [2, 3, 5, 7]]
    num, offsets = _lib.tile_layout(grid, spec, [0, 0, 1, 0])  # row 2's header walk failed: no tiles
    assert num.tolist() == counts
    assert offsets.tolist() == [0] + np.cumsum(1200 * np.array(counts)).tolist()
