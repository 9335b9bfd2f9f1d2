"""CPU tests of the drafted decode's Python and planner side (``draft=`` /
``drafts=``, ``Draft``, ``check_drafts``, ``ldt_set_draft``'s planning):

  * ``Draft((h, w))`` against what Pillow's own ``Image.draft`` picks for the
    same header sizes and request;
  * ``check_drafts`` refusals, each by name;
  * ``CallSpec`` carrying the field on every surface, through pickle;
  * ``CallSpec.resolve`` resolving the draft first and handing the drafted
    sizes to the box and window samplers, and ``Context.arm`` arming it;
  * the planner (csrc/ldt_plan.cpp, built for the host with ASan / UBSan):
    width, height, DCT_scaled_size, cdw, cdh, the upsampling factors, the
    no-fancy bit, strides and offsets for 4:4:4, 4:2:2, 4:2:0, 4:4:0, 4:1:1,
    4:1:0 and grey at each scale, against libjpeg's rules (jdmaster.c
    jpeg_calc_output_dimensions, jdsample.c) restated here.

The arithmetic is tests/test_idct_scaled_ops.py, the GPU side tests/test_gpu_draft.py.
"""
import io
import os
import pickle
import shutil
import struct
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import jpeg_recode as jr
import ldt_amd
from conftest import REPO
from ldt_amd import _lib
from ldt_amd import transforms as T

N = 3


def _save(arr, **kw) -> bytes:
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(arr)).save(b, format="JPEG", **kw)
    return b.getvalue()


def _with_size(jpeg: bytes, width: int, height: int) -> bytes:
    """The same file with another size in its SOF0: enough for a header walk (Pillow's draft reads no pixels)."""
    i = jpeg.index(b"\xff\xc0")
    return jpeg[:i + 5] + struct.pack(">HH", height, width) + jpeg[i + 9:]


TINY = _save(np.zeros((8, 8, 3), np.uint8), quality=50)
CELLS = [_with_size(TINY, w, h) for w, h in ((500, 375), (93, 67), (2048, 1536))]


# ---- Draft against Pillow ---------------------------------------------------------------------------

def test_draft_rule_is_pillows():
    from PIL import Image

    ratios = (0, 1, 2, 3, 4, 7, 8, 100)
    cases = []
    for w, h in ((1, 1), (3, 5), (64, 48), (81, 80)):
        for kw in ratios:
            for kh in (1, 2, 5, 8, 9):
                for rw, rh in ((0, 0), (w - 1, h // 2)):
                    W, H = kw * w + rw, kh * h + rh
                    if 1 <= W <= 8192 and 1 <= H <= 8192:
                        cases.append((W, H, w, h))
    assert {c[0] // c[2] for c in cases} >= set(ratios)
    for W, H, w, h in cases:
        im = Image.open(io.BytesIO(_with_size(TINY, W, H)))
        assert im.size == (W, H)
        mode, box = im.draft("RGB", (w, h))
        s = int(round(W / box[2]))
        assert s in (1, 2, 4, 8) and im.size == (-(-W // s), -(-H // s))
        got = ldt_amd.Draft((h, w)).sample(np.array([[W, H]], np.int32), np.zeros(1, np.int32))
        assert got.dtype == np.int32 and got.tolist() == [s], (W, H, w, h, s, got)
    # a failed row or an unknown size: scale 1
    d = ldt_amd.Draft((10, 10))
    assert d.sample(np.array([[100, 100], [0, 0], [100, 100]]), np.array([0, 1, 3])).tolist() == [8, 1, 1]
    assert pickle.loads(pickle.dumps(d)).size == (10, 10) and repr(d) == "Draft((10, 10))"
    with pytest.raises(TypeError, match="pair of ints"):
        ldt_amd.Draft(256)
    with pytest.raises(ValueError, match="at least 1 x 1"):
        ldt_amd.Draft((0, 5))


# ---- check_drafts -----------------------------------------------------------------------------------

def test_check_drafts_refusals_by_name():
    assert _lib.check_drafts(None, 5) is None
    ok = _lib.check_drafts([1, 2, 4, 8], 4)
    assert ok.dtype == np.int32 and ok.flags["C_CONTIGUOUS"] and ok.tolist() == [1, 2, 4, 8]
    assert _lib.check_drafts(np.array([8, 8], np.int64)[::1], 2).dtype == np.int32
    for bad in (0, 3, 5, 6, 7, 16, -2):
        with pytest.raises(ValueError, match=f"row 1 has scale {bad}, not 1, 2, 4 or 8"):
            _lib.check_drafts([1, bad, 2], 3)
    with pytest.raises(TypeError, match="must hold ints"):
        _lib.check_drafts([1.0, 2.0], 2)
    with pytest.raises(TypeError, match="must hold ints"):
        _lib.check_drafts([True, False], 2)
    with pytest.raises(ValueError, match=r"shape \[n\]"):
        _lib.check_drafts([[1, 2]], 1)
    with pytest.raises(ValueError, match="drafts for 2 rows, the batch has 3"):
        _lib.check_drafts([1, 2], 3)
    assert _lib.draft_sizes(np.array([[93, 67], [0, 0]], np.int32), np.array([4, 8])).tolist() == [[24, 17], [0, 0]]
    assert "ldt_set_draft" in _lib.EXPORTED


# ---- CallSpec ---------------------------------------------------------------------------------------

def _items():
    return [{"image": c, "label": i} for i, c in enumerate(CELLS)]


def _rb():
    return pa.RecordBatch.from_arrays([pa.array(CELLS, pa.binary()), pa.array(np.arange(N), pa.int64())],
                                      names=["image", "label"])


def _same_draft(a, b):
    if hasattr(a, "sample"):
        return type(a) is type(b) and a.size == b.size
    return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype == np.int32 and \
        np.array_equal(a, b)


@pytest.mark.parametrize("draft", [ldt_amd.Draft((256, 256)), np.array([2, 1, 8])], ids=["sampler", "array"])
def test_every_surface_carries_the_draft(draft, monkeypatch):
    monkeypatch.setattr(T, "_in_worker", lambda: True)
    opts = dict(draft=draft, window=ldt_amd.ResizeCenterCrop(256))
    want = T.CallSpec.make(**opts).check_arrays(N)
    assert "draft" in T.CallSpec.__slots__
    holders = {
        "DeviceBatch": T.DeviceBatch(T._pack_list(CELLS, list(range(N))), **opts),
        "make_collate_fn": T.make_collate_fn(**opts),
        "collate_fn": T.collate_fn(_items(), **opts),
        "decode_tensor_image": T.decode_tensor_image(_rb(), **opts),
        "make_collate_fn()()": T.make_collate_fn(**opts)(_items()),
    }
    for what, h in holders.items():
        spec = h._spec if what != "make_collate_fn" else h._spec.check_arrays(N)
        assert _same_draft(spec.draft, want.draft), what
        assert _same_draft(pickle.loads(pickle.dumps(h))._spec.check_arrays(N).draft, want.draft), what + " through pickle"
    assert _same_draft(holders["DeviceBatch"]._draft, want.draft)
    pipe = object.__new__(T.DecodePipeline)
    pipe._spec = T.CallSpec.make(draft=draft)
    assert pipe._spec.draft is draft and pipe._spec.override(interpolation="bicubic").draft is draft
    other = np.array([4, 4, 4])
    assert pipe._spec.override(drafts=other).draft is other
    # refused before any device or batch
    for name, call in (("decode_arrow", lambda **o: T.decode_arrow(pa.array(CELLS, pa.binary()), **o)),
                       ("collate_fn", lambda **o: T.collate_fn(_items(), **{k[:-1]: v for k, v in o.items()}))):
        with pytest.raises(ValueError, match="not 1, 2, 4 or 8"):
            call(drafts=np.array([1, 3, 1]))
        with pytest.raises(ValueError, match="the batch has 3"):
            call(drafts=np.array([1, 2]))
    with pytest.raises(ValueError, match="draft must be None"):
        T.CallSpec.make(draft=2)
    with pytest.raises(TypeError, match="drafts"):
        T.resize_raw(None, 8, 8, drafts=np.array([2]))


class _Rec:
    def __init__(self, log, name, value):
        self.log, self.name, self.value = log, name, value

    def sample(self, wh, status=None, *a, **k):
        self.log.append((self.name, np.asarray(wh).copy()))
        return self.value


def test_resolve_drafts_first_and_hands_the_drafted_sizes_on():
    wh = np.array([[500, 375], [93, 67], [2048, 1536]], np.int32)
    status = np.zeros(N, np.int32)
    log = []
    crops = np.tile(np.array([0, 0, 9, 9, 0], np.int32), (N, 1))
    windows = np.tile(np.array([30, 33, 0, 0], np.int32), (N, 1))
    spec = T.CallSpec.make(size=(30, 33), draft=ldt_amd.Draft((128, 128)), crop=_Rec(log, "crop", crops))
    got = spec.resolve(sizes=(wh, status), n=N)
    assert len(got) == 5 and got.drafts.tolist() == [2, 1, 8]
    drafted = [[250, 188], [93, 67], [256, 192]]
    assert [n for n, _ in log] == ["crop"] and log[0][1].tolist() == drafted
    # a window sampler without boxes gets the drafted sizes too; an array of scales serves as well
    del log[:]
    spec = T.CallSpec.make(size=(30, 33), draft=np.array([2, 1, 8]), window=_Rec(log, "window", windows))
    got = spec.resolve(sizes=(wh, status), n=N)
    assert got.drafts.dtype == np.int32 and log[0][1].tolist() == drafted
    # the real samplers: what torchvision computes on the drafted PIL image
    rcc = ldt_amd.ResizeCenterCrop(64)
    got = T.CallSpec.make(size=(56, 56), draft=ldt_amd.Draft((128, 128)), window=rcc).resolve(sizes=(wh, status), n=N)
    assert np.array_equal(got[1], rcc.sample(np.array(drafted), status, (56, 56)))
    import torch

    rrc = ldt_amd.RandomResizedCropFlip()
    torch.manual_seed(5)
    want = rrc.sample(np.array(drafted, np.int32), status)
    torch.manual_seed(5)
    got = T.CallSpec.make(size=(56, 56), draft=np.array([2, 1, 8]), crop=rrc).resolve(sizes=(wh, status), n=N)
    assert np.array_equal(got[0], want)
    assert (got[0][:, 0] + got[0][:, 2] <= np.array(drafted)[:, 1]).all()
    # no draft: nothing changes, the header walk is not asked for
    plain = T.CallSpec.make(crop=crops).resolve(sizes=lambda: 1 / 0, n=N)
    assert plain.drafts is None and plain[0] is crops
    # from the cells themselves
    got = T.CallSpec.make(draft=ldt_amd.Draft((128, 128))).resolve(pa.array(CELLS, pa.binary()))
    assert got.drafts.tolist() == [2, 1, 8]


def test_arm_arms_the_draft_last_and_disarms_it():
    import test_mix

    ctx = test_mix._fake_context()
    ctx.arm((224, 224), "bilinear", "float32", "contiguous", drafts=None)
    assert ctx.lib.calls == []
    d = _lib.check_drafts([2, 1, 8], 3)
    ctx.arm((224, 224), "bilinear", "float32", "contiguous", drafts=d)
    assert ctx.lib.calls == [("ldt_set_draft", 1234, d.ctypes.data, 3)]
    ctx = test_mix._fake_context("ldt_set_draft")
    crops = _lib.check_crops(np.tile(np.array([0, 0, 1, 1, 0]), (N, 1)), N)
    with pytest.raises(_lib.LdtError, match="rc=-1"):
        ctx.arm((224, 224), "bilinear", "float32", "contiguous", crops=crops, drafts=d)
    at = [c[0] for c in ctx.lib.calls].index("ldt_set_draft")
    assert ("ldt_set_draft", 1234, None, 0) in ctx.lib.calls[at + 1:]
    assert ("ldt_set_crops", 1234, None, 0) in ctx.lib.calls[at + 1:]


# ---- the planner ------------------------------------------------------------------------------------

LAYOUTS = {"444": ((1, 1),) * 3, "422": ((2, 1), (1, 1), (1, 1)), "420": ((2, 2), (1, 1), (1, 1)),
           "440": ((1, 2), (1, 1), (1, 1)), "411": ((4, 1), (1, 1), (1, 1)), "410": ((4, 2), (1, 1), (1, 1)),
           "gray": ((1, 1),)}
SIZES = ((67, 93), (9, 17))  # (height, width)


def _libjpeg(factors, W, H, s):
    """Per component (sc, cdw, cdh, hf, vf) by jdmaster.c / jdsample.c under scale 1 / s."""
    hmax, vmax, min_s = max(f[0] for f in factors), max(f[1] for f in factors), 8 // s
    out = []
    for h, v in factors:
        sc = min_s
        while sc < 8 and (hmax * min_s) % (h * sc * 2) == 0 and (vmax * min_s) % (v * sc * 2) == 0:
            sc *= 2
        out.append((sc, -(-W * h * sc // (hmax * 8)), -(-H * v * sc // (vmax * 8)), hmax * min_s // (h * sc),
                    vmax * min_s // (v * sc)))
    return out


def test_the_rules_give_the_known_consequences():
    for s in (2, 4, 8):
        assert all(c[3:] == (1, 1) for c in _libjpeg(LAYOUTS["420"], 93, 67, s))  # 4:2:0 never upsamples
    assert [c[0] for c in _libjpeg(LAYOUTS["420"], 93, 67, 2)] == [4, 8, 8]  # chroma: the full 8 x 8 ISLOW
    assert [(c[0], c[3], c[4]) for c in _libjpeg(LAYOUTS["422"], 93, 67, 2)] == [(4, 1, 1), (4, 2, 1), (4, 2, 1)]
    assert [(c[0], c[3], c[4]) for c in _libjpeg(LAYOUTS["410"], 93, 67, 2)] == [(4, 1, 1), (8, 2, 1), (8, 2, 1)]
    assert _libjpeg(LAYOUTS["422"], 9, 17, 4)[1][1] == 2  # cdw == 2: the fancy small-width exception
    assert [(c[0], c[3], c[4]) for c in _libjpeg(LAYOUTS["440"], 93, 67, 8)] == [(1, 1, 1), (1, 1, 2), (1, 1, 2)]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("draft_plan") / "draft_plan_check")
    src = [os.path.join(REPO, "tests", "fuzz", "draft_plan_check.cpp"),
           os.path.join(REPO, "lance-distributed-training_amd", "csrc", "ldt_plan.cpp")]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", *src, "-o", exe], check=True)
    return exe


def _plan(exe, cells, scales, size=(224, 224)):
    inp = b"".join(struct.pack("<I", len(c)) + c for c in cells)
    r = subprocess.run([exe, str(size[0]), str(size[1]), *[str(s) for s in scales]], input=inp, capture_output=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().split("\n")
    assert "draft_plan_ok" in lines
    rows, total = [], None
    for ln in lines:
        f = ln.split()
        if f[:1] == ["row"]:
            rows.append(dict(zip(f[2::2], (int(v) for v in f[3:19:2])), box=[int(v) for v in f[19:23]], comps=[]))
        elif f[:1] == ["comp"]:
            rows[-1]["comps"].append(tuple(int(v) for v in f[2:]))
        elif f[:1] == ["plane_total"]:
            total = int(f[1])
    return rows, total


@pytest.fixture(scope="module")
def layout_files():
    from ldt_amd import synth

    src = jr.layout_source()
    out = {}
    for h, w in SIZES:
        a = synth.field(h, w, 70 + h, 12.0)
        out["444", h, w] = _save(a, quality=90, subsampling="4:4:4")
        out["422", h, w] = _save(a, quality=90, subsampling="4:2:2")
        out["420", h, w] = _save(a, quality=90, subsampling="4:2:0")
        out["gray", h, w] = _save(a[:, :, 0], quality=90)
        for name in ("440", "411", "410"):
            out[name, h, w] = jr.reframe(src, LAYOUTS[name], h, w)
    return out


@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_planner_against_libjpegs_rules(planner, layout_files, s):
    keys = sorted(layout_files)
    rows, total = _plan(planner, [layout_files[k] for k in keys], [s] * len(keys))
    end = 0
    for (name, H, W), r in zip(keys, rows):
        factors = LAYOUTS[name]
        hmax, vmax = max(f[0] for f in factors), max(f[1] for f in factors)
        dw, dh = -(-W // s), -(-H // s)
        assert r["status"] == 0 and (r["width"], r["height"]) == (dw, dh), (name, r)
        assert r["draft"] == s and r["nofancy"] == (1 if s == 8 else 0), (name, r)
        assert r["n_draft"] == (0 if s == 1 else len(keys))
        assert r["box"] == [0, 0, dh, dw], (name, r)  # the whole-image default box is the drafted image
        assert (r["max_w"], r["max_h"]) == (-(-93 // s), -(-67 // s))
        mcux, mcuy = -(-W // (8 * hmax)), -(-H // (8 * vmax))
        for (h, v), (sc, cdw, cdh, hf, vf, stride, off), want in zip(factors, r["comps"], _libjpeg(factors, W, H, s)):
            assert (sc, cdw, cdh, hf, vf) == want, (name, s, (sc, cdw, cdh, hf, vf), want)
            bw, bh = mcux * h, mcuy * v
            # the staging's assumptions: rows of whole 8-byte groups, planes 256-aligned, nothing overlapping
            assert stride % 8 == 0 and bw * sc <= stride < bw * sc + 8 and off % 256 == 0 and off >= end, (name, s)
            assert cdw <= bw * sc and cdh <= bh * sc and (s > 1 or stride == bw * 8)
            end = off + stride * bh * sc
    assert total >= end


def test_planner_mixed_scales_limits_and_max_dim(planner, layout_files):
    cells = [layout_files["420", 67, 93], layout_files["444", 67, 93], _with_size(TINY, 8200, 8), _with_size(TINY, 600, 40)]
    rows, _ = _plan(planner, cells, [1, 4, 8, 8], size=(7, 5))
    assert [r["status"] for r in rows] == [0, 0, 4, 0]  # LDT_MAX_DIM bounds the file; 600 -> 75 passes the limit of 37
    assert [r["draft"] for r in rows] == [1, 4, 0, 8] and rows[0]["n_draft"] == 2
    assert (rows[3]["width"], rows[3]["height"]) == (75, 5)
    rows, _ = _plan(planner, cells[3:], [1], size=(7, 5))
    assert rows[0]["status"] == 4  # ceil(600 / 5) = 120 > 37 without the draft
