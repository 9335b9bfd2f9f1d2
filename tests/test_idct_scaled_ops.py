"""CPU tests of the drafted decode's arithmetic: csrc/ldt_idct_scaled.hpp, the
one source k_idct_scaled runs, compiled for the host (tools/checks/
idct_scaled_host.cpp) and called through ctypes, against Pillow itself.

The luma coefficient grids of 4:4:4 baseline files (``jpeg_recode.block_grids``)
and the file's luma quantisation table go through the 4x4, 2x2 and 1x1
transforms; the reference is ``np.asarray(im)`` after ``im.draft("L", req)`` on
the same file, which decodes Y alone at that scale: no colour conversion, no
upsampling. Zero mismatched bytes are allowed at scales 2, 4 and 8. Each case
asserts the size Pillow decoded at, so it cannot compare at another scale.

A stand-alone build of the same file under ASan / UBSan runs the transforms on
extreme coefficients (+-2047 and the int16 limits times quantisers up to 65535).
The GPU side is tests/test_gpu_draft.py.
"""
import ctypes
import functools
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_recode
from conftest import REPO
from draft_ref import draft_at

SRC = os.path.join(REPO, "tools", "checks", "idct_scaled_host.cpp")
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
          21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
          60, 61, 54, 47, 55, 62, 63)


def _cxx():
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("idct_scaled_host") / "libidct_scaled_host.so")
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-shared", "-fPIC", SRC, "-o", so], check=True)
    L = ctypes.CDLL(so)
    L.idct_scaled_host_plane.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p]
    L.idct_scaled_host_plane.restype = None
    return L


def _save(arr, **kw) -> bytes:
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(arr)).save(b, format="JPEG", **kw)
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def sources():
    """name -> a 4:4:4 baseline file."""
    out = {}
    for q in (50, 90, 100):
        noise = np.random.default_rng(100 + q).integers(0, 256, (67, 93, 3), dtype=np.uint8)
        out[f"noise-67x93-q{q}"] = _save(noise, quality=q, subsampling="4:4:4")
    for h, w in ((1, 1), (8, 8), (9, 17)):
        noise = np.random.default_rng(7 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
        out[f"noise-{h}x{w}-q90"] = _save(noise, quality=90, subsampling="4:4:4")
    out["flat-67x93"] = _save(np.full((67, 93, 3), 77, np.uint8), quality=90, subsampling="4:4:4")
    # the stress cells' size-10 coefficients and 16-bit quantisation tables, where 4:4:4 baseline
    for c in jpeg_recode.stress_cells():
        if not c.tags & {"large-symbols", "uniform", "pq1", "q1s"}:
            continue
        segs = jpeg_recode.parse(c.data)[0]
        if not any(m == 0xC0 for m, _ in segs):
            continue
        fr = jpeg_recode._frame(segs)
        if len(fr.comps) == 3 and all(cc[1:] == (1, 1) for cc in fr.comps):
            out["stress-" + c.name] = c.data
    # no stress cell has 16-bit tables at 4:4:4: the same tables on full-contrast 4:4:4 content
    uni = np.random.RandomState(21).randint(0, 256, (40, 56, 3)).astype(np.uint8)
    out["qtables-16bit-444"] = _save(uni, qtables=[[16 * (i + 1) for i in range(64)]] * 2, subsampling="4:4:4")
    assert any("checker" in k for k in out) and any("uniform" in k for k in out)
    return out


def _luma_qtable(jpeg: bytes) -> np.ndarray:
    """The quantisation table of component 0, natural order."""
    segs = jpeg_recode.parse(jpeg)[0]
    tabs = {}
    for m, p in segs:
        s = 0
        while m == 0xDB and s < len(p):
            pq, tq = p[s] >> 4, p[s] & 15
            n = 128 if pq else 64
            raw = np.frombuffer(p[s + 1:s + 1 + n], ">u2" if pq else "u1").astype(np.uint16)
            nat = np.zeros(64, np.uint16)
            nat[list(ZIGZAG)] = raw
            tabs[tq] = nat
            s += 1 + n
    sof = next(p for m, p in segs if m in (0xC0, 0xC1))  # 16-bit tables make the file SOF1
    return tabs[sof[8]]


def _luma_blocks(jpeg: bytes):
    """(bw, bh, int16 [bh * bw, 64] in natural order) of component 0."""
    bw, bh, grids = jpeg_recode.block_grids(jpeg)
    coef = np.zeros((bh * bw, 64), np.int16)
    for (bx, by), (dc, ac) in grids[0].items():
        blk = coef[by * bw + bx]
        blk[0] = dc
        k = 1
        for sym, extra in ac:
            r, s = sym >> 4, sym & 15
            if s == 0:
                if sym != 0xF0:
                    break
                k += 16
                continue
            k += r
            blk[ZIGZAG[k]] = jpeg_recode._dc_value(s, extra)
            k += 1
    return bw, bh, coef


@pytest.mark.parametrize("scale", [2, 4, 8])
@pytest.mark.parametrize("name", sorted(sources()))
def test_reduced_idct_equals_pillow_draft_l(host, name, scale):
    from PIL import Image

    data = sources()[name]
    im = Image.open(io.BytesIO(data))
    W, H = im.size
    draft_at(im, "L", scale)
    assert im.mode == "L" and im.size == (-(-W // scale), -(-H // scale)), (im.mode, im.size, scale)
    want = np.asarray(im)
    bw, bh, coef = _luma_blocks(data)
    q = _luma_qtable(data)
    sc = 8 // scale
    plane = np.zeros((bh * sc, bw * sc), np.uint8)
    host.idct_scaled_host_plane(coef.ctypes.data, q.ctypes.data, bw, bh, sc, plane.ctypes.data)
    got = plane[:want.shape[0], :want.shape[1]]
    assert got.shape == want.shape
    assert np.count_nonzero(got != want) == 0, (name, scale, int(np.abs(got.astype(int) - want).max()))


def test_extremes_under_sanitizers(tmp_path):
    exe = str(tmp_path / "idct_scaled_host")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DIDCT_SCALED_HOST_MAIN", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "idct scaled ok" in r.stdout
