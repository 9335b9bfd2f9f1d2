"""CPU tests of the blur's host side: the eighth column of ``check_colors``
(Pillow's radius, packed as the weights ``ldt_blur_weights`` gives), the
``blur_p`` / ``blur_radius`` draws of ``ColorJitterParams`` and the record's
layout. The arithmetic is tests/test_blur_ops.py, the device (and
``ldt_set_colors``, which needs a context) tests/test_gpu_blur.py.
"""
import ctypes
import hashlib
import pickle

import numpy as np
import pytest
import torch

ORDER0123 = 0 + 4 * 1 + 16 * 2 + 64 * 3
ROW7 = [0.6, np.nan, 1.4, 0.1, ORDER0123, 0, -1]


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _replay(g, n, views, p, gray_p, blur_p, radius, sol_p, threshold=128):
    """The torch calls of ColorJitterParams' docstring, literally, for the default jitter ranges."""
    ranges = [(0.6, 1.4), (0.6, 1.4), (0.6, 1.4), (-0.1, 0.1)]
    at = lambda q, v: q[v] if isinstance(q, (list, tuple)) else q  # noqa: E731
    out = []
    for i in range(n):
        for v in range(views):
            row = [float("nan")] * 4 + [ORDER0123, 0.0, -1.0, float("nan")]
            if at(p, v) is not None:
                r = torch.rand(1, generator=g)
                if not at(p, v) < r:
                    f = torch.randperm(4, generator=g)
                    row[4] = int(f[0]) + 4 * int(f[1]) + 16 * int(f[2]) + 64 * int(f[3])
                    for k, rng in enumerate(ranges):
                        row[k] = float(torch.empty(1).uniform_(rng[0], rng[1], generator=g))
            if at(gray_p, v) is not None:
                row[5] = float(bool(torch.rand(1, generator=g) < at(gray_p, v)))
            if at(blur_p, v) is not None:  # after the grayscale draw, before the solarize draw
                r = torch.rand(1, generator=g)
                if not at(blur_p, v) < r:
                    row[7] = float(torch.empty(1).uniform_(radius[0], radius[1], generator=g))
            if at(sol_p, v) is not None and bool(torch.rand(1, generator=g) < at(sol_p, v)):
                row[6] = float(threshold)
            out.append(row)
    return np.array(out, np.float64).reshape(n, views, 8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ---- check_colors ----

def test_seven_columns_give_the_records_they_gave():
    from ldt_amd import _lib, check_colors

    dt = _lib.color_dtype()
    assert dt.itemsize == 32
    assert dt.names == ("brightness", "contrast", "saturation", "hue_shift", "order", "mask", "gray", "solarize",
                        "blur_ww", "blur_r", "pad")
    assert dt.fields["blur_ww"][1] == 24 and dt.fields["blur_r"][1] == 28 and dt.fields["pad"][1] == 30
    rows = np.array([ROW7, [np.nan, 2.5, np.nan, -0.1, 3 + 4 * 2 + 16 * 1 + 64 * 0, 1, 128]], np.float64)
    r = check_colors(rows, 2)
    # the record before the blur existed: the same 24 bytes, then 8 zero bytes
    raw = r.view(np.uint8).reshape(2, 32)
    assert not raw[:, 24:].any()
    old = np.dtype([("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"), ("hue_shift", "<i4"),
                    ("order", "u1", (4,)), ("mask", "u1"), ("gray", "u1"), ("solarize", "<i2"), ("pad", "u1", (8,))])
    o = r.view(old)
    assert o["mask"].tolist() == [0b1101, 0b1010] and o["solarize"].tolist() == [-1, 128]
    assert o["brightness"][0] == np.float32(0.6) and o["hue_shift"].tolist() == [25, (-25) & 255]
    # an absent blur column gives those bytes too
    for absent in (np.nan, 0.0):
        r8 = check_colors(np.concatenate([rows, np.full((2, 1), absent)], axis=1), 2)
        assert r8.tobytes() == r.tobytes()


def test_eight_columns_carry_the_weights():
    from ldt_amd import _lib, check_colors

    radii = [0.1, 2.0, 8.0, 1.0, np.nan, 0.0]
    rows = np.array([ROW7 + [v] for v in radii], np.float64)
    r = check_colors(rows, 6)
    assert r["blur_r"].tolist() == [0, 1, 7, 0, 0, 0]
    assert r["blur_ww"].tolist() == [16721291, 4473924, 1052688, 11184811, 0, 0]
    assert [_lib.blur_weights(v) for v in (0.1, 2.0, 8.0)] == [(0, 16721291), (1, 4473924), (7, 1052688)]
    # everything before the blur fields is what seven columns give
    r7 = check_colors(rows[:, :7], 6)
    assert np.array_equal(r.view(np.uint8).reshape(6, 32)[:, :24], r7.view(np.uint8).reshape(6, 32)[:, :24])
    # records are accepted again; views; lists and tensors
    assert np.array_equal(check_colors(r, 6), r)
    v = check_colors(np.stack([rows, rows[::-1]], axis=1), 6, 2)
    assert v.shape == (6, 2) and np.array_equal(v[:, 0], r) and np.array_equal(v[:, 1], r[::-1])
    assert np.array_equal(check_colors(torch.from_numpy(rows), 6), r)
    # the radius is rounded to float32 first, as Pillow rounds it
    near = check_colors(np.array([ROW7 + [float(np.float32(0.7)) + 1e-12]]), 1)
    assert (int(near["blur_r"][0]), int(near["blur_ww"][0])) == _lib.blur_weights(float(np.float32(0.7)))


@pytest.mark.parametrize("value", [-0.1, 8.0001, 9.0, 1e30, np.inf, -np.inf])
def test_bad_radius_is_refused(value):
    from ldt_amd import check_colors

    with pytest.raises(ValueError, match="8.0"):  # the message names the limit
        check_colors(np.array([ROW7 + [value]], np.float64), 1)


def test_bad_shapes_are_refused():
    from ldt_amd import check_colors

    rows = np.array([ROW7 + [1.0]] * 3, np.float64)
    for bad, n, views in ((rows, 4, None), (rows, 3, 2), (np.stack([rows, rows], axis=1), 3, None),
                          (np.concatenate([rows, rows[:, :1]], axis=1), 3, None), (rows[:, :6], 3, None),
                          (np.stack([rows, rows], axis=1), 3, 3)):
        with pytest.raises(ValueError):
            check_colors(bad, n, views)
    # the other columns are checked as they always were
    rows[1, 5] = 2
    with pytest.raises(ValueError):
        check_colors(rows, 3)


def test_blur_weights_symbol():
    """The C function itself: no context, no device."""
    from ldt_amd import _lib

    L = _lib.load_library()
    r, ww = ctypes.c_int32(-1), ctypes.c_uint32(1)
    assert L.ldt_blur_weights(1.0, ctypes.byref(r), ctypes.byref(ww)) == _lib.LDT_OK
    assert (r.value, ww.value) == (0, 11184811)  # the float32 quotient; a double's would truncate to ...810
    assert L.ldt_blur_weights(0.0, ctypes.byref(r), ctypes.byref(ww)) == _lib.LDT_OK
    assert (r.value, ww.value) == (0, 1 << 24)
    for bad in (-1.0, 8.5, float("nan"), float("inf")):
        assert L.ldt_blur_weights(bad, ctypes.byref(r), ctypes.byref(ww)) == _lib.LDT_ERR_ARG
    assert L.ldt_blur_weights(1.0, None, ctypes.byref(ww)) == _lib.LDT_ERR_ARG
    assert L.ldt_blur_weights(1.0, ctypes.byref(r), None) == _lib.LDT_ERR_ARG
    with pytest.raises(ValueError):
        _lib.blur_weights(8.5)


def test_record_layout():
    """sizeof(ldt_color) == 32 with the blur fields carved out of the old padding."""
    from ldt_amd import _lib

    class Rec(ctypes.Structure):  # include/ldt.h's ldt_color
        _fields_ = [("brightness", ctypes.c_float), ("contrast", ctypes.c_float), ("saturation", ctypes.c_float),
                    ("hue_shift", ctypes.c_int32), ("order", ctypes.c_uint8 * 4), ("mask", ctypes.c_uint8),
                    ("gray", ctypes.c_uint8), ("solarize", ctypes.c_int16), ("blur_ww", ctypes.c_uint32),
                    ("blur_r", ctypes.c_uint16), ("pad_", ctypes.c_uint8 * 2)]

    assert ctypes.sizeof(Rec) == 32 == _lib.color_dtype().itemsize
    dt = _lib.color_dtype()
    for name in ("solarize", "blur_ww", "blur_r"):
        assert getattr(Rec, name).offset == dt.fields[name][1]


# ---- the sampler ----

def test_draw_order():
    from ldt_amd import ColorJitterParams

    got = ColorJitterParams(blur_p=0.5, solarize_p=0.3, generator=_gen(11)).sample(60)
    want = _replay(_gen(11), 60, 1, 0.8, 0.2, 0.5, (0.1, 2.0), 0.3)[:, 0]
    assert got.dtype == np.float64 and got.shape == (60, 8) and _same(got, want)
    drawn = got[~np.isnan(got[:, 7]), 7]
    assert 0 < len(drawn) < 60 and np.all((drawn >= 0.1) & (drawn <= 2.0))
    # another range
    got = ColorJitterParams(blur_p=1.0, blur_radius=(3.0, 8.0), generator=_gen(2)).sample(20)
    assert _same(got, _replay(_gen(2), 20, 1, 0.8, 0.2, 1.0, (3.0, 8.0), None)[:, 0])
    assert np.all((got[:, 7] >= 3.0) & (got[:, 7] <= 8.0))


def test_no_blur_p_gives_the_array_it_gave():
    from ldt_amd import ColorJitterParams

    got = ColorJitterParams(solarize_p=0.2, generator=_gen(1234)).sample(64, views=2)
    assert got.shape == (64, 2, 7)
    want = _replay(_gen(1234), 64, 2, 0.8, 0.2, None, None, 0.2)[..., :7]
    assert _same(got, want)
    # the bytes that seed gave before blur_p existed
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == SEED_1234_SHA256
    # and blur_p=None consumes no draw
    g, h = _gen(5), _gen(5)
    ColorJitterParams(generator=g).sample(9)
    ColorJitterParams(blur_p=None, blur_radius=(1.0, 3.0), generator=h).sample(9)
    assert torch.equal(g.get_state(), h.get_state())


# sha256 of ColorJitterParams(solarize_p=0.2, generator=<seed 1234>).sample(64, views=2), taken from the sampler as it
# was before blur_p existed
SEED_1234_SHA256 = "0541303d2a2f20d52a12fa110850465b6452f0a1f3b20f361311ac3b6eb3f51d"


def test_per_view_blur_p():
    from ldt_amd import ColorJitterParams, check_colors

    s = ColorJitterParams(blur_p=[1.0, 0.1], solarize_p=[0.0, 0.2], generator=_gen(7))  # DINO's / BYOL's two views
    got = s.sample(80, views=2)
    assert _same(got, _replay(_gen(7), 80, 2, 0.8, 0.2, [1.0, 0.1], (0.1, 2.0), [0.0, 0.2]))
    assert not np.isnan(got[:, 0, 7]).any()  # p = 1.0 always applies
    rare = np.count_nonzero(~np.isnan(got[:, 1, 7]))
    assert 0 < rare < 40
    with pytest.raises(ValueError):
        s.sample(4, views=3)
    with pytest.raises(ValueError):
        s.sample(4)
    r = check_colors(got, 80, 2)
    assert np.array_equal(r["blur_ww"] != 0, ~np.isnan(got[..., 7]))
    assert set(r["blur_r"].ravel().tolist()) <= {0, 1}  # radii up to 2.0


def test_bad_arguments():
    from ldt_amd import ColorJitterParams

    for bad in (dict(blur_p=1.5), dict(blur_p=[0.5, -0.1]), dict(blur_radius=(0.0, 2.0)), dict(blur_radius=(2.0, 0.1)),
                dict(blur_radius=(0.1, 8.5)), dict(blur_radius=1.0), dict(blur_radius=(0.1, 1.0, 2.0))):
        with pytest.raises((ValueError, TypeError)):
            ColorJitterParams(**bad)


def test_pickle():
    from ldt_amd import ColorJitterParams

    s = ColorJitterParams(blur_p=[1.0, 0.1], blur_radius=(0.2, 1.5))
    t = pickle.loads(pickle.dumps(s))
    assert repr(t) == repr(s) and t.blur_p == (1.0, 0.1) and t.blur_radius == (0.2, 1.5)
    assert "blur_p" in repr(s) and "blur_p" not in repr(ColorJitterParams())
    torch.manual_seed(77)
    a = s.sample(7, views=2)
    torch.manual_seed(77)
    b = t.sample(7, views=2)
    assert _same(a, b) and a.shape == (7, 2, 8)
