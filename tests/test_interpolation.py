"""CPU tests of the resize's filter selection (``interpolation=``, ldt_set_filter):
what needs no GPU.

* The coefficient arithmetic of csrc/ldt_resample.hpp, the code the streaming
  kernel runs, through the stand-alone program tools/checks/resample_check.cpp
  (its own ``main``, built with ASan + UBSan and run directly): its two-pass
  resize against Pillow's ``resize`` with BICUBIC and BILINEAR, bit for bit, on
  0/255 checkerboards over random bytes, whose overshoot is clamped at both
  ends; and the generalised tap count against the formula it had before.
* The oracle identity the expected tensors of tests/test_gpu_interpolation.py
  rest on: ``oracle.raw_to_tensor(img, h, w)`` of an h x w image is ToTensor
  [+ Normalize] of it, the bilinear resize to the same size being the identity.
* The planner with the bicubic filter under ASan + UBSan, through the
  stand-alone driver tests/fuzz/filter_plan_check.cpp.
* ``check_interpolation``, the one validator of every ``interpolation=``.
* Pickle round trips of what carries the filter to another process.
"""
import enum
import os
import pickle
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import REPO, read_golden
from oracle import oracle
from test_worker_paths import _cells, cell_ds  # noqa: F401  (the worker tests' dataset fixture)

SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
       "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")

# (H, W) -> (oh, ow)
SHAPES = [((8, 8), (224, 224)), ((17, 5), (30, 33)), ((48, 64), (7, 5)), ((77, 91), (13, 21)),
          ((375, 500), (30, 33)), ((100, 150), (224, 224)), ((64, 80), (3, 2)), ((200, 130), (5, 7))]


def _cxx():
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    return cxx


@pytest.fixture(scope="module")
def resample_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resample") / "resample_check")
    subprocess.run([_cxx(), *SAN, os.path.join(REPO, "tools", "checks", "resample_check.cpp"), "-o", exe], check=True)
    return exe


def checkerboard(h, w, seed):
    """0/255 checkerboard on two thirds of the pixels, random bytes elsewhere."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((yy + xx) & 1) * 255).astype(np.uint8)
    keep = rng.random((h, w)) < 2 / 3
    img[keep] = board[keep][:, None]
    return img


def _run_resize(exe, tmp_path, img, size, filt):
    h, w = img.shape[:2]
    src, dst = str(tmp_path / "in.rgb"), str(tmp_path / "out.rgb")
    img.tofile(src)
    r = subprocess.run([exe, "resize", str(h), str(w), str(size[0]), str(size[1]), str(filt), src, dst],
                       capture_output=True, timeout=120, env=ENV)
    assert r.returncode == 0 and not r.stderr and r.stdout.decode().strip() == "resize ok", \
        (r.returncode, r.stdout.decode()[-2000:], r.stderr.decode(errors="replace")[-4000:])
    return np.fromfile(dst, np.uint8).reshape(size[0], size[1], 3)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
def test_shared_coefficients_equal_pillow(resample_check, tmp_path, shape):
    from PIL import Image

    (h, w), (oh, ow) = shape
    img = checkerboard(h, w, 1000 + h * w)
    assert img.min() == 0 and img.max() == 255
    pil = {f: np.asarray(Image.fromarray(img).resize((ow, oh), r))
           for f, r in ((0, Image.BILINEAR), (1, Image.BICUBIC))}
    # otherwise the filter is not exercised
    assert not np.array_equal(pil[0], pil[1]), "BICUBIC equals BILINEAR on this image"
    if oh > h and ow > w:  # an upscale of a 0/255 board: the overshoot is clamped at both ends
        assert pil[1].min() == 0 and pil[1].max() == 255
    for f in (1, 0):
        got = _run_resize(resample_check, tmp_path, img, (oh, ow), f)
        diff = np.abs(got.astype(int) - pil[f].astype(int))
        assert diff.max() <= 2, f"filter {f}: max abs {diff.max()}"
        assert np.array_equal(got, pil[f]), f"filter {f}: {np.count_nonzero(diff)} values differ (max {diff.max()})"


def test_shapes_are_the_issues():
    assert len(SHAPES) == 8 and sum(1 for (h, w), (oh, ow) in SHAPES if oh > h and ow > w) >= 2


def test_generalised_tap_count_equals_the_old_formula(resample_check):
    r = subprocess.run([resample_check, "ksize"], capture_output=True, timeout=300, env=ENV)
    out = r.stdout.decode()
    assert r.returncode == 0 and not r.stderr and "FAIL" not in out, (out[-2000:], r.stderr.decode(errors="replace")[-4000:])
    assert out.startswith("ksize ok: 1440000 pairs")


def test_bilinear_resize_to_the_same_size_is_the_identity():
    """What lets the GPU tests apply ToTensor / Normalize to Pillow's BICUBIC
    result through the (bilinear) oracle: at the same size every output pixel
    has the single weight 1."""
    for (h, w), seed in (((30, 33), 1), ((7, 5), 2), ((224, 224), 3)):
        img = checkerboard(h, w, seed)
        t = oracle.raw_to_tensor(img, h, w)
        assert np.array_equal(t, img.transpose(2, 0, 1).astype(np.float32) / np.float32(255))
        n = oracle.raw_to_tensor(img, h, w, normalize=True)
        assert n.shape == t.shape and not np.array_equal(n, t)
        # Normalize is a function of the uint8 value alone: equal bytes, equal floats
        for c in range(3):
            for v in (0, 255):
                vals = n[c][img[:, :, c] == v]
                assert vals.size and np.all(vals == vals[0])


# ---- the planner with the bicubic filter under sanitizers ------------------------------------

def test_planner_with_the_bicubic_filter_under_sanitizers(tmp_path):
    from ldt_amd import synth

    exe = str(tmp_path / "filter_plan_check")
    src = [os.path.join(REPO, "tests", "fuzz", "filter_plan_check.cpp"),
           os.path.join(REPO, "lance-distributed-training_amd", "csrc", "ldt_plan.cpp")]
    subprocess.run([_cxx(), *SAN, *src, "-o", exe], check=True)
    cells = [synth.encode(synth.field(375, 500, 202, 6.0), quality=90, restart_marker_rows=1),
             synth.encode(synth.field(100, 150, 204, 6.0), subsampling="4:4:4"),
             read_golden("jpeg/gray_77x91.jpg"), read_golden("jpeg/prog_64x80.jpg"),
             synth.encode(synth.field(8, 8, 205, 6.0), subsampling="4:4:4")]
    inp = b"".join(struct.pack("<I", len(c)) + c for c in cells)
    r = subprocess.run([exe], input=inp, capture_output=True, timeout=300, env=ENV)
    out = r.stdout.decode()
    assert r.returncode == 0 and not r.stderr and "FAIL" not in out, (out[-4000:], r.stderr.decode(errors="replace")[-4000:])
    lines = out.splitlines()
    assert lines[-1] == "filter_plan_ok"
    sizes = [tuple(int(v) for v in x.split()[1:]) for x in lines if x.startswith("size ")]
    assert sizes == [oracle.jpeg_info(c)[:2] for c in cells]


# ---- check_interpolation ----------------------------------------------------------------------

class InterpolationMode(enum.Enum):
    """A stand-in for torchvision.transforms.InterpolationMode (not installed)."""
    NEAREST = "nearest"
    NEAREST_EXACT = "nearest-exact"
    BILINEAR = "bilinear"
    BICUBIC = "bicubic"
    BOX = "box"
    HAMMING = "hamming"
    LANCZOS = "lanczos"


def test_check_interpolation_accepts():
    from PIL import Image

    import ldt_amd
    from ldt_amd import _lib

    ok = _lib.check_interpolation
    assert ldt_amd.check_interpolation is ok
    for v in (None, "bilinear", "BILINEAR", "Bilinear", InterpolationMode.BILINEAR, Image.Resampling.BILINEAR,
              Image.BILINEAR, 2, np.int64(2).item()):
        assert ok(v) == "bilinear", v
    for v in ("bicubic", "BICUBIC", "BiCubic", InterpolationMode.BICUBIC, Image.Resampling.BICUBIC, Image.BICUBIC, 3):
        assert ok(v) == "bicubic", v
    assert ok(ok("bicubic")) == "bicubic" and ok(ok(None)) == "bilinear"
    assert int(Image.Resampling.BILINEAR) == 2 and int(Image.Resampling.BICUBIC) == 3
    assert _lib.FILTERS == {"bilinear": 0, "bicubic": 1} and _lib.FILTER_BICUBIC == 1


def test_check_interpolation_refuses_by_name():
    from PIL import Image

    from ldt_amd import _lib

    refused = ["nearest", "lanczos", "hamming", "box", "NEAREST", "Lanczos", "nearest-exact", "area", "", "bicubic ",
               0, 1, 4, 5, 6, -1, 2.0, 3.0, True, False, b"bicubic", ("bicubic",), object(),
               InterpolationMode.NEAREST, InterpolationMode.LANCZOS, InterpolationMode.HAMMING, InterpolationMode.BOX,
               InterpolationMode.NEAREST_EXACT, Image.Resampling.NEAREST, Image.Resampling.LANCZOS,
               Image.Resampling.HAMMING, Image.Resampling.BOX]
    for v in refused:
        with pytest.raises(ValueError) as e:
            _lib.check_interpolation(v)
        msg = str(e.value)
        assert repr(v) in msg and "'bilinear'" in msg and "'bicubic'" in msg, (v, msg)
    # Pillow's ints are named
    for v, name in ((0, "NEAREST"), (1, "LANCZOS"), (4, "BOX"), (5, "HAMMING"), (Image.Resampling.LANCZOS, "LANCZOS")):
        with pytest.raises(ValueError, match=name):
            _lib.check_interpolation(v)


def test_every_entry_point_validates_before_it_needs_a_device():
    """An unsupported filter is a ValueError, never a silent bilinear result,
    and every new argument is optional and named as documented."""
    import inspect

    import pyarrow as pa

    from ldt_amd import _lib
    from ldt_amd import transforms as T

    for fn in (T.decode_arrow, T.collate_fn, T.make_collate_fn, T.resize_raw, T.ResidentBatch.decode,
               T.DecodePipeline.__init__, T.DecodePipeline.decode, T.make_to_tensor_fn, T.DeviceBatch.__init__,
               T._BoundCollate.__init__):
        assert inspect.signature(fn).parameters["interpolation"].default is None, fn
    rb = pa.RecordBatch.from_arrays([pa.array([b"x"], pa.binary())], names=["image"])
    with pytest.raises(ValueError, match="lanczos"):
        T.decode_tensor_image(rb, interpolation="lanczos")
    with pytest.raises(ValueError, match="nearest"):
        T.collate_fn([{"image": b"x"}], interpolation="nearest")
    with pytest.raises(ValueError, match="hamming"):
        T.make_collate_fn(interpolation="hamming")
    with pytest.raises(ValueError, match="box"):
        T.DeviceBatch(T._pack_list([b"x"], None), interpolation="box")
    with pytest.raises(ValueError, match="NEAREST"):
        T.decode_arrow(pa.array([b"x"], pa.binary()), interpolation=0)
    assert hasattr(_lib.Context, "use_filter")
    for name in ("ldt_set_filter", "ldt_get_filter"):
        assert name in _lib.EXPORTED and hasattr(_lib.load_library(), name)


# ---- what carries the filter to another process -------------------------------------------------

def test_pickle_round_trips():
    import ldt_amd
    from ldt_amd import transforms as T

    fn = pickle.loads(pickle.dumps(ldt_amd.make_collate_fn(interpolation="bicubic", size=(30, 33))))
    assert fn.interpolation == "bicubic" and fn.size == (30, 33)
    fn = pickle.loads(pickle.dumps(ldt_amd.make_collate_fn(interpolation=InterpolationMode.BICUBIC)))
    assert fn.interpolation == "bicubic"
    assert pickle.loads(pickle.dumps(ldt_amd.make_collate_fn())).interpolation == "bilinear"
    cells = _cells(5)
    b = T.DeviceBatch(T._pack_list(cells, list(range(5))), size=(30, 33), interpolation="BICUBIC")
    b2 = pickle.loads(pickle.dumps(b))
    assert b2._interpolation == "bicubic" and b2._size == (30, 33)
    arr, lab = T._unpack(b2._packed)
    assert arr.to_pylist() == cells and lab.tolist() == list(range(5))
    assert pickle.loads(pickle.dumps(T.DeviceBatch(T._pack_list(cells, None))))._interpolation == "bilinear"


def test_the_filter_travels_with_the_cells_from_a_spawn_worker(cell_ds):  # noqa: F811
    """make_collate_fn(interpolation=...) in a stock DataLoader spawn worker:
    the DeviceBatch that reaches the main process names the filter."""
    from torch.utils.data import DataLoader

    from ldt_amd import SafeLanceDataset, make_collate_fn
    from ldt_amd import transforms as T

    ds, cells = cell_ds
    dl = DataLoader(SafeLanceDataset(ds.uri), batch_size=32, shuffle=False, num_workers=1,
                    collate_fn=make_collate_fn(interpolation="bicubic", size=(30, 33)), pin_memory=False,
                    multiprocessing_context="spawn")
    got = []
    for b in dl:
        assert isinstance(b, T.DeviceBatch) and b._interpolation == "bicubic" and b._size == (30, 33)
        got += T._unpack(b._packed)[0].to_pylist()
    assert got == cells
