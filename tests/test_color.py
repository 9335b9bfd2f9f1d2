"""CPU tests of the photometric stage's host side: ``ColorJitterParams`` (the
draw order of torchvision's RandomApply([ColorJitter]), RandomGrayscale and
RandomSolarize, restated with torch's RNG) and ``check_colors`` (the one
validator of every ``colors=`` / ``color=`` argument, which packs the library's
``ldt_color`` records). The arithmetic is tests/test_color_ops.py, the device
tests/test_gpu_color.py.
"""
import ctypes
import pickle

import numpy as np
import pytest
import torch

ORDER0123 = 0 + 4 * 1 + 16 * 2 + 64 * 3


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _replay(g, n, views, ranges, p, gray_p, sol_p, threshold):
    """The torch calls of the docstring, literally, image by image and view by view."""
    out = []
    for i in range(n):
        for v in range(views):
            row = [float("nan")] * 4 + [ORDER0123, 0.0, -1.0]
            pv = p[v] if isinstance(p, (list, tuple)) else p
            if pv is not None:
                r = torch.rand(1, generator=g)
                if not pv < r:
                    fn_idx = torch.randperm(4, generator=g)
                    row[4] = int(fn_idx[0]) + 4 * int(fn_idx[1]) + 16 * int(fn_idx[2]) + 64 * int(fn_idx[3])
                    for k, rng in enumerate(ranges):
                        if rng is not None:
                            row[k] = float(torch.empty(1).uniform_(rng[0], rng[1], generator=g))
            gv = gray_p[v] if isinstance(gray_p, (list, tuple)) else gray_p
            if gv is not None:
                row[5] = float(bool(torch.rand(1, generator=g) < gv))
            sv = sol_p[v] if isinstance(sol_p, (list, tuple)) else sol_p
            if sv is not None and bool(torch.rand(1, generator=g) < sv):
                row[6] = float(threshold)
            out.append(row)
    return np.array(out, np.float64).reshape(n, views, 7)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def test_draw_order_defaults():
    from ldt_amd import ColorJitterParams

    got = ColorJitterParams(generator=_gen(11)).sample(40)
    want = _replay(_gen(11), 40, 1, [(0.6, 1.4), (0.6, 1.4), (0.6, 1.4), (-0.1, 0.1)], 0.8, 0.2, None, 128)[:, 0]
    assert got.dtype == np.float64 and _same(got, want)
    # both outcomes of every coin occur in 40 rows
    assert np.isnan(got[:, 0]).any() and (~np.isnan(got[:, 0])).any()
    assert set(got[:, 5]) == {0.0, 1.0} and set(got[:, 6]) == {-1.0}
    applied = got[~np.isnan(got[:, 0])]
    assert len({int(o) for o in applied[:, 4]}) > 3  # the permutation is drawn
    assert np.all((applied[:, :3] >= 0.6) & (applied[:, :3] <= 1.4)) and np.all(np.abs(applied[:, 3]) <= 0.1)


def test_skipped_jitter_gives_nans_and_identity_order():
    from ldt_amd import ColorJitterParams

    got = ColorJitterParams(p=0.0, gray_p=None, generator=_gen(3)).sample(16)
    assert np.isnan(got[:, :4]).all() and np.all(got[:, 4] == ORDER0123)
    assert np.all(got[:, 5] == 0) and np.all(got[:, 6] == -1)


def test_views_and_per_view_probabilities():
    from ldt_amd import ColorJitterParams

    sol = [0.0, 0.2] + [0.0] * 6  # DINO: the second global view only
    p = [1.0, 0.8] + [0.8] * 6
    s = ColorJitterParams(0.4, 0.4, 0.2, 0.1, p=p, gray_p=0.2, solarize_p=sol, solarize_threshold=100, generator=_gen(5))
    got = s.sample(30, views=8)
    want = _replay(_gen(5), 30, 8, [(0.6, 1.4), (0.6, 1.4), (0.8, 1.2), (-0.1, 0.1)], p, 0.2, sol, 100)
    assert _same(got, want)
    assert not np.isnan(got[:, 0, 0]).any()  # p = 1.0 always applies
    assert np.all(got[:, [0, 2, 3, 4, 5, 6, 7], 6] == -1) and set(got[:, 1, 6]) == {-1.0, 100.0}
    with pytest.raises(ValueError):
        s.sample(4, views=2)
    with pytest.raises(ValueError):
        s.sample(4)
    # a scalar sampler serves any number of views, in the order sample(n * V) draws
    a = ColorJitterParams(generator=_gen(9)).sample(6, views=3)
    b = ColorJitterParams(generator=_gen(9)).sample(18)
    assert _same(a.reshape(18, 7), b)


def test_ranges_follow_check_input_and_pairs_are_taken_as_given():
    from ldt_amd import ColorJitterParams

    s = ColorJitterParams(brightness=1.5, contrast=(0.2, 0.3), saturation=0, hue=None, p=1.0, gray_p=None,
                          generator=_gen(2))
    assert s.brightness == (0.0, 2.5) and s.contrast == (0.2, 0.3) and s.saturation is None and s.hue is None
    got = s.sample(20)
    want = _replay(_gen(2), 20, 1, [(0.0, 2.5), (0.2, 0.3), None, None], 1.0, None, None, 128)[:, 0]
    assert _same(got, want)
    assert np.isnan(got[:, 2:4]).all() and not np.isnan(got[:, :2]).any()
    for bad in (dict(brightness=-1), dict(hue=0.6), dict(hue=(-0.6, 0.1)), dict(contrast=(0.5, 0.2)), dict(p=1.5),
                dict(gray_p=[0.1, 2.0]), dict(solarize_threshold=300), dict(saturation="x")):
        with pytest.raises((ValueError, TypeError)):
            ColorJitterParams(**bad)


def test_absent_transforms_draw_nothing():
    from ldt_amd import ColorJitterParams

    g = _gen(21)
    before = g.get_state()
    got = ColorJitterParams(p=None, gray_p=None, solarize_p=None, generator=g).sample(5, views=2)
    assert torch.equal(g.get_state(), before)
    assert np.isnan(got[..., :4]).all() and np.all(got[..., 4] == ORDER0123) and np.all(got[..., 6] == -1)
    # all four ops absent: an applied jitter draws its coin and the permutation only
    g2, g3 = _gen(4), _gen(4)
    ColorJitterParams(None, None, None, None, p=1.0, gray_p=None, generator=g2).sample(1)
    torch.rand(1, generator=g3)
    torch.randperm(4, generator=g3)
    assert torch.equal(g2.get_state(), g3.get_state())


def test_global_rng_and_pickle():
    from ldt_amd import ColorJitterParams

    s = ColorJitterParams(solarize_p=[0.0, 0.2])
    t = pickle.loads(pickle.dumps(s))
    assert repr(t) == repr(s) and t.solarize_p == (0.0, 0.2)
    torch.manual_seed(77)
    a = s.sample(7, views=2)
    torch.manual_seed(77)
    b = t.sample(7, views=2)
    assert _same(a, b)


def test_check_colors_shapes_and_records():
    from ldt_amd import _lib, check_colors

    assert check_colors(None, 3) is None
    dt = _lib.color_dtype()
    assert dt.itemsize == 32
    rows = np.array([[0.6, np.nan, 1.4, 0.1, ORDER0123, 0, -1],
                     [np.nan, 2.5, np.nan, -0.1, 3 + 4 * 2 + 16 * 1 + 64 * 0, 1, 128],
                     [np.nan, np.nan, np.nan, np.nan, ORDER0123, 0, 256]], np.float64)
    r = check_colors(rows, 3)
    assert r.dtype == dt and r.shape == (3,) and r.flags["C_CONTIGUOUS"]
    assert r["mask"].tolist() == [0b1101, 0b1010, 0] and r["gray"].tolist() == [0, 1, 0]
    assert r["solarize"].tolist() == [-1, 128, 256]
    assert r["order"].tolist() == [[0, 1, 2, 3], [3, 2, 1, 0], [0, 1, 2, 3]]
    assert r["hue_shift"].tolist() == [25, (-25) & 255, 0]  # int(hue * 255) truncated toward zero, mod 256
    # the float32 nearest to the factor, as Pillow's (float)alpha
    assert r["brightness"][0] == np.float32(0.6) and float(r["brightness"][0]) != 0.6
    assert r["contrast"][1] == np.float32(2.5)
    # hue 0.0 is present; -0.5 and 0.5 wrap to 129 and 127
    h = check_colors(np.array([[np.nan] * 3 + [v, ORDER0123, 0, -1] for v in (0.0, -0.5, 0.5)]), 3)
    assert h["mask"].tolist() == [8, 8, 8] and h["hue_shift"].tolist() == [0, (-127) & 255, 127]
    # records are accepted again, lists and torch tensors too
    assert check_colors(r, 3) is not None and np.array_equal(check_colors(r, 3), r)
    assert np.array_equal(check_colors(rows.tolist(), 3), r)
    assert np.array_equal(check_colors(torch.from_numpy(rows), 3), r)
    # views
    v = check_colors(np.stack([rows, rows[::-1]], axis=1), 3, 2)
    assert v.shape == (3, 2) and np.array_equal(v[:, 0], r) and np.array_equal(v[:, 1], r[::-1])
    with pytest.raises(ValueError):
        check_colors(rows, 3, 2)  # a 2-D array in a call with views
    with pytest.raises(ValueError):
        check_colors(np.stack([rows, rows], axis=1), 3)
    with pytest.raises(ValueError):
        check_colors(rows, 4)
    with pytest.raises(ValueError):
        check_colors(rows[:, :6], 3)
    with pytest.raises(ValueError):
        check_colors(r, 2)
    with pytest.raises(TypeError):
        check_colors(np.array([["a"] * 7]), 1)
    assert check_colors(np.zeros((0, 7)), 0).shape == (0,)


@pytest.mark.parametrize("col,value", [(0, -0.1), (1, np.inf), (2, 1e39), (3, 0.51), (3, -0.6), (3, np.inf),
                                        (4, 0), (4, 1 + 4 * 1 + 16 * 2 + 64 * 3), (4, 256), (4, 27.5), (4, np.nan),
                                        (5, 2), (5, 0.5), (5, np.nan), (6, -2), (6, 257), (6, 127.5), (6, np.nan)])
def test_check_colors_refuses(col, value):
    from ldt_amd import check_colors

    row = [1.0, 1.0, 1.0, 0.0, ORDER0123, 0, -1]
    assert check_colors(np.array([row]), 1) is not None
    row[col] = value
    with pytest.raises(ValueError):
        check_colors(np.array([row], np.float64), 1)


def test_sampler_output_passes_check_colors():
    from ldt_amd import ColorJitterParams, check_colors

    s = ColorJitterParams(solarize_p=0.5, generator=_gen(8))
    a = s.sample(50, views=2)
    r = check_colors(a, 50, 2)
    assert np.array_equal(r["mask"] == 0, np.isnan(a[..., 0]))
    assert np.array_equal(r["solarize"], a[..., 6].astype(np.int16))


def test_set_colors_without_a_context():
    """The one context-free path of ldt_set_colors: a null context is an argument error."""
    from ldt_amd import _lib

    L = _lib.load_library()
    rec = np.zeros(1, _lib.color_dtype())
    assert L.ldt_set_colors(None, rec.ctypes.data, 1) == _lib.LDT_ERR_ARG
    assert L.ldt_set_colors(None, None, 0) == _lib.LDT_ERR_ARG
    assert ctypes.sizeof(ctypes.c_float) * 3 + 4 + 4 + 1 + 1 + 2 + 8 == _lib.color_dtype().itemsize
