"""CPU tests of the auto-augment stage's arithmetic: csrc/ldt_augment.hpp, the
one source the augment kernels run, compiled for the host (tools/checks/
augment_host.cpp, -ffp-contract=off) and called through ctypes on numpy arrays,
against Pillow itself. Zero mismatched bytes are allowed anywhere:

  * the affine op against ``Image.transform(AFFINE, NEAREST, fillcolor)`` and
    ``Image.rotate``: every bin and both signs of the five geometric ops in
    both magnitude spaces through ``affine_matrix``, the four right angles on a
    square and a non-square image, three fills, 200 random general matrices;
  * ``ImageEnhance.Sharpness`` (``ImageFilter.SMOOTH`` blended with the image),
    the filter's accumulation order confirmed with a non-symmetric
    ``ImageFilter.Kernel`` first;
  * ``ImageOps.posterize`` at bits 0..8 and ``ImageOps.invert``;
  * ``ImageOps.autocontrast``'s table for all 32 896 ``(lo, hi)`` pairs;
  * ``ImageOps.equalize`` on 300 random histograms and its edge cases;
  * chains of two and four ops in the kernels' slot order, the statistics
    recomputed between ops.

A stand-alone build of the same file under ASan / UBSan sweeps the functions
once more. The GPU side is tests/test_gpu_augment.py.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image, ImageEnhance, ImageFilter, ImageOps

from conftest import REPO

SRC = os.path.join(REPO, "tools", "checks", "augment_host.cpp")
SIZES = ((1, 1), (1, 7), (7, 1), (3, 3), (33, 20), (129, 257))  # (h, w)
FILLS = (None, (9, 8, 7), 255)


def _cxx():
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("augment_host") / "libaugment_host.so")
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so], check=True)
    L = ctypes.CDLL(so)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    L.augment_host_run.argtypes = [vp, i32, i32, vp, vp]
    L.augment_host_run.restype = None
    L.augment_host_autocontrast_lut.argtypes = [vp, vp]
    L.augment_host_autocontrast_lut.restype = None
    L.augment_host_equalize_lut.argtypes = [vp, vp]
    L.augment_host_equalize_lut.restype = None
    L.augment_host_kernel3x3.argtypes = [vp, vp, vp, vp]
    L.augment_host_kernel3x3.restype = i32
    L.augment_host_fix.argtypes = [vp, vp]
    L.augment_host_fix.restype = i32
    L.augment_host_walk_ok.argtypes = [vp, i32, i32]
    L.augment_host_walk_ok.restype = i32
    return L


def _image(h, w, seed=0):
    rng = np.random.default_rng(977 * h + w + seed)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def _run(host, rgb, rows):
    """The host driver on an [h, w, 3] image with ``rows`` of check_augments."""
    from ldt_amd import _lib

    rgb = np.ascontiguousarray(rgb)
    h, w = rgb.shape[:2]
    rec = _lib.check_augments(np.array([rows], np.float64), 1, size=(h, w) if max(h, w) <= 1024 else None)
    out = np.empty_like(rgb)
    host.augment_host_run(rgb.ctypes.data, h, w, rec.ctypes.data, out.ctypes.data)
    return out


def _row(op, *p, fill=None):
    row = [float(op)] + [float(x) for x in p] + [np.nan] * (6 - len(p))
    f = (0, 0, 0) if fill is None else (fill,) * 3 if isinstance(fill, int) else fill
    return row + [float(x) for x in f]


def _pil_fill(fill):
    return None if fill is None else (fill,) * 3 if isinstance(fill, int) else tuple(fill)


def _pil_geometric(img, name, magnitude, fill):
    """torchvision's _apply_op for the five geometric ops, on PIL (F.affine's
    matrix through affine_matrix for shear and translate, Image.rotate itself
    for Rotate)."""
    from ldt_amd.augment import affine_matrix

    if name == "Rotate":
        return img.rotate(magnitude, Image.NEAREST, fillcolor=_pil_fill(fill))
    return img.transform(img.size, Image.AFFINE, affine_matrix(name, magnitude, (img.height, img.width)),
                         Image.NEAREST, fillcolor=_pil_fill(fill))


def _spaces():
    """(name, magnitudes) of the geometric ops in the wide and the RandAugment
    space for an (h, w) image, as float lists."""
    import torch

    def both(h, w):
        lin = lambda hi: [float(x) for x in torch.linspace(0.0, hi, 31)]  # noqa: E731
        return (("ShearX", lin(0.99) + lin(0.3)), ("ShearY", lin(0.99) + lin(0.3)),
                ("TranslateX", lin(32.0) + lin(150.0 / 331.0 * w)), ("TranslateY", lin(32.0) + lin(150.0 / 331.0 * h)),
                ("Rotate", lin(135.0) + lin(30.0)))
    return both


@pytest.mark.parametrize("hw", SIZES)
def test_affine_bins_match_pillow(host, hw):
    from ldt_amd.augment import affine_matrix

    h, w = hw
    rgb = _image(h, w)
    img = Image.fromarray(rgb)
    bad = 0
    for k, (name, mags) in enumerate(_spaces()(h, w)):
        for i, m in enumerate(mags):
            for sign in (1.0, -1.0):
                fill = FILLS[(i + k) % 3]
                want = np.asarray(_pil_geometric(img, name, sign * m, fill))
                got = _run(host, rgb, [_row(1, *affine_matrix(name, sign * m, hw), fill=fill)])
                bad += int(np.count_nonzero(want != got))
    assert bad == 0


@pytest.mark.parametrize("hw", ((33, 33), (33, 20), (1, 1), (129, 257)))
def test_rotate_right_angles(host, hw):
    from ldt_amd.augment import affine_matrix

    rgb = _image(*hw)
    img = Image.fromarray(rgb)
    for angle in (0.0, 90.0, 180.0, 270.0, -90.0, 360.0, 450.0):
        for fill in FILLS:
            want = np.asarray(img.rotate(angle, Image.NEAREST, fillcolor=_pil_fill(fill)))
            got = _run(host, rgb, [_row(1, *affine_matrix("Rotate", angle, hw), fill=fill)])
            assert np.array_equal(want, got), (angle, fill)


def test_affine_random_matrices(host):
    rng = np.random.default_rng(4242)
    bad = 0
    for t in range(200):
        h, w = SIZES[2 + t % 4] if t % 4 else (20, 33)
        rgb = _image(h, w, t)
        img = Image.fromarray(rgb)
        ang = rng.uniform(-np.pi, np.pi)
        s = rng.uniform(0.4, 2.5, 2)
        m = [s[0] * np.cos(ang) + rng.normal(0, 0.2), -s[0] * np.sin(ang) + rng.normal(0, 0.2), rng.uniform(-w, w),
             s[1] * np.sin(ang) + rng.normal(0, 0.2), s[1] * np.cos(ang) + rng.normal(0, 0.2), rng.uniform(-h, h)]
        if m[1] == 0 and m[3] == 0:
            continue
        fill = FILLS[t % 3]
        want = np.asarray(img.transform(img.size, Image.AFFINE, m, Image.NEAREST, fillcolor=_pil_fill(fill)))
        got = _run(host, rgb, [_row(1, *m, fill=fill)])
        bad += int(np.count_nonzero(want != got))
    assert bad == 0


@pytest.mark.parametrize("hw", ((1, 1), (2, 3), (7, 6), (8, 9), (33, 20)))
def test_flips_and_integer_translations_match_pillow_transform(host, hw):
    """The matrices with p1 == 0 and p3 == 0 that check_augments lets through
    (unit scale of either sign, integer offsets), which Pillow routes through its
    scale routine and not the fixed-point walk: both must agree, on odd and even
    sizes, with offsets that move the image partly and wholly outside."""
    h, w = hw
    rgb = _image(h, w)
    img = Image.fromarray(rgb)
    mats = [(1, 0, 0, 0, 1, 0), (-1, 0, w, 0, 1, 0), (1, 0, 0, 0, -1, h), (-1, 0, w, 0, -1, h),
            (1, 0, -2, 0, 1, 3), (-1, 0, w + 1, 0, 1, -1), (1, 0, 3, 0, -1, h - 2), (-1, 0, w - 2, 0, -1, h + 2),
            (1, 0, w, 0, 1, 0), (-1, 0, 0, 0, -1, 0), (1, 0, -w - 3, 0, -1, 2 * h + 1)]
    for m in mats:
        for fill in FILLS:
            want = np.asarray(img.transform(img.size, Image.AFFINE, m, Image.NEAREST, fillcolor=_pil_fill(fill)))
            assert np.array_equal(want, _run(host, rgb, [_row(1, *m, fill=fill)])), (m, fill)


def test_python_fix_and_walk_check_equal_the_header(host):
    """check_augments' restatement of FIX and of the int32 walk check against the
    header's (aug_affine_fix, and aug_affine_walk_ok, which the decode call
    relies on): the same coefficients and the same verdict, at the edges too."""
    from ldt_amd import _lib

    rng = np.random.default_rng(7)
    mats = [(1, 0, 0, 0, 1, 0), (-1, 0, 1024, 0, -1, 1024), (0.5, -0.99, 3.25, 0.99, 0.5, -7.5),
            (32767.99, 0.25, -32767.99, -0.25, -32767.99, 32767.99), (31.9, 0.1, -32767, 0.1, 31.9, 0),
            (1, 0.5, 32000, 0.5, 1, 0), (1e-9, -1e-9, 0.49999, 1e-9, 1e-9, -0.50001), (32768, 0, 0, 0, 1, 0),
            (1, 0, 0, 0, -32768, 0), (32767.9, 32767.9, 32767.9, 1, 1, 1)]
    mats += [tuple(rng.uniform(-3, 3, 6) * 10.0 ** rng.integers(-3, 5, 6)) for _ in range(300)]
    refused = walks = 0
    for m in mats:
        md = np.array(m, np.float64)
        a = np.zeros(6, np.int32)
        ok = host.augment_host_fix(md.ctypes.data, a.ctypes.data)
        py_ok = all(abs(x) < 32768.0 for x in m) and all(-(1 << 31) <= x < (1 << 31) for x in _lib.affine_fix(m))
        assert bool(ok) == py_ok, m
        if not ok:
            refused += 1
            continue
        fix = _lib.affine_fix(m)
        assert a.tolist() == fix, m
        for h, w in ((1, 1), (7, 5), (224, 224), (1024, 1024), (1, 1024)):
            py_walk = all(-(1 << 31) <= fix[o + 2] + fix[o] * x + fix[o + 1] * y < (1 << 31)
                          for o in (0, 3) for x, y in ((0, 0), (w, h), (0, h), (w, 0)))
            assert bool(host.augment_host_walk_ok(a.ctypes.data, w, h)) == py_walk, (m, h, w)
            walks += not py_walk
            # check_augments itself: it refuses exactly when the corner test or the walk check does
            if m[1] != 0 or m[3] != 0:
                corner = all(abs(x * m[0] + y * m[1] + m[2]) < 32768.0 and abs(x * m[3] + y * m[4] + m[5]) < 32768.0
                             for x, y in ((0, 0), (w, h), (0, h), (w, 0)))
                try:
                    _lib.check_augments([[_row(1, *m)]], 1, size=(h, w))
                    took = True
                except ValueError:
                    took = False
                assert took == (corner and py_walk), (m, h, w)
    assert refused >= 3 and walks >= 3  # the edges were reached


def test_smooth_accumulation_order_probe(host):
    """A non-symmetric kernel shows the order Pillow sums the rows in (SMOOTH's
    symmetry would hide a wrong one): the restated order must match on every
    interior pixel."""
    rgb = _image(40, 37)
    k = (0.11, 0.07, 0.05, 0.13, 0.29, 0.03, 0.17, 0.02, 0.13)
    want = np.asarray(Image.fromarray(rgb).filter(ImageFilter.Kernel((3, 3), k, scale=1.0)))
    kf = np.array(k, np.float32)
    a = rgb.astype(np.int32)
    bad = 0
    for y in range(1, 39):
        for x in range(1, 36):
            for ch in range(3):
                rows = [np.ascontiguousarray(a[y + d, x - 1:x + 2, ch]) for d in (-1, 0, 1)]
                got = host.augment_host_kernel3x3(rows[0].ctypes.data, rows[1].ctypes.data, rows[2].ctypes.data,
                                                  kf.ctypes.data)
                bad += got != want[y, x, ch]
    assert bad == 0


@pytest.mark.parametrize("hw", ((1, 1), (2, 5), (3, 3), (96, 96)))
def test_sharpness_matches_pillow(host, hw):
    rgb = _image(*hw)
    img = Image.fromarray(rgb)
    for f in (0.01, 0.5, 1.0, 1.45, 1.99):
        want = np.asarray(ImageEnhance.Sharpness(img).enhance(f))
        assert np.array_equal(want, _run(host, rgb, [_row(5, f)])), f


def test_enhance_ops_match_pillow(host):
    rgb = _image(29, 37)
    img = Image.fromarray(rgb)
    for code, cls in ((2, ImageEnhance.Brightness), (3, ImageEnhance.Color), (4, ImageEnhance.Contrast)):
        for f in (0.01, 0.5, 1.0, 1.45, 1.99):
            assert np.array_equal(np.asarray(cls(img).enhance(f)), _run(host, rgb, [_row(code, f)])), (code, f)


def test_pointwise_match_pillow(host):
    rgb = np.arange(256 * 3, dtype=np.uint32).reshape(16, 16, 3).astype(np.uint8)
    rgb[..., 1] = rgb[..., 1][::-1]
    img = Image.fromarray(rgb)
    for bits in range(9):
        want = np.asarray(ImageOps.posterize(img, bits)) if bits else np.zeros_like(rgb)
        assert np.array_equal(want, _run(host, rgb, [_row(6, bits)])), bits
    assert np.array_equal(np.asarray(ImageOps.invert(img)), _run(host, rgb, [_row(10)]))
    for th in (0, 1, 127.5, 128, 246.5, 255, 256):
        assert np.array_equal(np.asarray(ImageOps.solarize(img, th)), _run(host, rgb, [_row(7, th)])), th


def test_autocontrast_every_pair(host):
    """All 32 896 (lo, hi) pairs: the table against ImageOps.autocontrast on a
    row holding lo..hi (an L image: one channel is one table)."""
    ramp = np.arange(256, dtype=np.uint8)
    bad = 0
    for lo in range(256):
        for hi in range(lo, 256):
            row = ramp[lo:hi + 1][None, :]
            want = np.asarray(ImageOps.autocontrast(Image.fromarray(row, "L")))[0]
            hist = np.zeros(256, np.uint32)
            hist[lo:hi + 1] = 1
            lut = np.empty(256, np.uint8)
            host.augment_host_autocontrast_lut(hist.ctypes.data, lut.ctypes.data)
            bad += int(np.count_nonzero(lut[lo:hi + 1] != want))
    assert bad == 0


def _equalize_images():
    rng = np.random.default_rng(99)
    yield np.full((5, 5, 3), 77, np.uint8)  # one value
    two = np.full((20, 20, 3), 3, np.uint8)
    two[7:, :, :] = 200
    yield two  # two values
    yield rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)  # fewer than 255 pixels: step == 0
    yield np.full((224, 224, 3), 255, np.uint8)  # all 255
    yield rng.integers(0, 256, (96, 96, 3), dtype=np.uint8)
    yield (rng.normal(128, 30, (224, 224, 3)).clip(0, 255)).astype(np.uint8)
    for t in range(294):
        h, w = int(rng.integers(1, 64)), int(rng.integers(1, 64))
        kind = t % 3
        if kind == 0:
            a = rng.integers(0, 256, (h, w, 3))
        elif kind == 1:  # a few values, skewed
            vals = rng.integers(0, 256, int(rng.integers(1, 6)))
            a = vals[rng.integers(0, len(vals), (h, w, 3))]
        else:  # a narrow band up to 255
            a = 255 - rng.geometric(0.3, (h, w, 3)).clip(0, 255)
        yield a.astype(np.uint8)


def test_equalize_matches_pillow(host):
    count = 0
    for rgb in _equalize_images():
        want = np.asarray(ImageOps.equalize(Image.fromarray(rgb)))
        assert np.array_equal(want, _run(host, rgb, [_row(9)])), rgb.shape
        count += 1
    assert count == 300


def test_autocontrast_image_matches_pillow(host):
    for rgb in list(_equalize_images())[:12]:
        want = np.asarray(ImageOps.autocontrast(Image.fromarray(rgb)))
        assert np.array_equal(want, _run(host, rgb, [_row(8)])), rgb.shape


def _pil_op(img, row):
    op, p = int(row[0]), row[1:7]
    fill = tuple(int(x) for x in row[7:10])
    if op == 1:
        return img.transform(img.size, Image.AFFINE, p, Image.NEAREST, fillcolor=fill)
    if op in (2, 3, 4, 5):
        cls = {2: ImageEnhance.Brightness, 3: ImageEnhance.Color, 4: ImageEnhance.Contrast, 5: ImageEnhance.Sharpness}
        return cls[op](img).enhance(p[0])
    return {6: lambda: ImageOps.posterize(img, int(p[0])), 7: lambda: ImageOps.solarize(img, p[0]),
            8: lambda: ImageOps.autocontrast(img), 9: lambda: ImageOps.equalize(img),
            10: lambda: ImageOps.invert(img)}[op]()


def test_chains_match_pillow(host):
    from ldt_amd.augment import affine_matrix

    hw = (61, 47)
    rot = _row(1, *affine_matrix("Rotate", 31.5, hw), fill=(9, 8, 7))
    shear = _row(1, *affine_matrix("ShearX", -0.3, hw))
    chains = ([rot, _row(9)], [_row(4, 1.7), _row(8)], [_row(5, 1.9), shear], [_row(9), _row(9)],
              [_row(4, 0.3), rot, _row(9), _row(5, 0.2)], [_row(8), _row(3, 1.8), _row(6, 3), _row(4, 1.2)],
              [_row(2, 1.6), [np.nan] * 10, _row(7, 100.5), _row(10)])
    rgb = _image(*hw)
    for rows in chains:
        img = Image.fromarray(rgb)
        for row in rows:
            if not np.isnan(row[0]):
                img = _pil_op(img, row)
        assert np.array_equal(np.asarray(img), _run(host, rgb, rows)), rows


def test_sanitizer_sweep(tmp_path):
    """The same file as a stand-alone program under ASan / UBSan, on the CPU."""
    exe = str(tmp_path / "augment_host")
    cxx = _cxx()
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-DAUGMENT_HOST_MAIN", SRC, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "augment ok" in run.stdout
