"""CPU tests of the output-size parameter (Resize((h, w)) beyond 224 x 224):

* the yardstick: oracle.jpeg_to_tensor / raw_to_tensor at other sizes against
  Pillow itself, on a fixed subset of sources and sizes;
* the ``size=`` validator, with no device present;
* ``_BoundCollate`` and ``DeviceBatch`` keep ``size`` through pickle;
* the C ABI: ldt_set_output_size / ldt_get_output_size are declared,
  exported and bound, and refuse a null context;
* the band kernel's launch geometry (csrc/ldt_geom4.hpp) for every output
  size, by tools/checks/geom4_check.cpp under ASan/UBSan.
"""
import io
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from oracle import oracle

# (h, w) of the sources, each encoded as 4:4:4 and 4:2:0
SOURCES = [(1, 1), (13, 17), (64, 641), (600, 40), (200, 300), (512, 512)]
# (h, w) of the outputs: odd, non-square, up- and down-scaling, one row / one column
SIZES = [(1, 1), (2, 3), (7, 5), (30, 33), (128, 96), (225, 223), (255, 257), (299, 299), (513, 100), (1, 1024),
         (1024, 1)]


def _pil_tensor(data: bytes, oh: int, ow: int) -> np.ndarray:
    from PIL import Image

    img = Image.open(io.BytesIO(data)).convert("RGB").resize((ow, oh), Image.BILINEAR)
    return np.asarray(img, np.uint8).transpose(2, 0, 1).astype(np.float32) / np.float32(255)


@pytest.fixture(scope="module")
def source_cells():
    from ldt_amd import synth

    cells = []
    for k, (h, w) in enumerate(SOURCES):
        for sub in ("4:4:4", "4:2:0"):
            cells.append(((h, w, sub), synth.encode(synth.field(h, w, 100 + k, 8.0), quality=90, subsampling=sub)))
    return cells


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_equals_pillow_at_other_sizes(source_cells, size):
    oh, ow = size
    for name, data in source_cells:
        got = oracle.jpeg_to_tensor(data, oh, ow)
        assert got.shape == (3, oh, ow)
        assert np.array_equal(got, _pil_tensor(data, oh, ow)), f"{name} -> {size}"


def test_oracle_raw_equals_pillow_at_other_sizes():
    from PIL import Image

    from ldt_amd import synth

    for (h, w), (oh, ow) in [((300, 200), (64, 64)), ((301, 517), (299, 299)), ((301, 517), (513, 100))]:
        hwc = synth.raw_hwc_one(h, w, 7)
        exp = np.asarray(Image.fromarray(hwc).resize((ow, oh), Image.BILINEAR), np.uint8)
        exp = exp.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
        assert np.array_equal(oracle.raw_to_tensor(hwc, oh, ow), exp), f"{(h, w)} -> {(oh, ow)}"


# ---- the validator -------------------------------------------------------

def test_check_size_accepts_pairs_and_none():
    from ldt_amd._lib import check_size

    assert check_size(None) == (224, 224)
    assert check_size((1, 1)) == (1, 1)
    assert check_size([299, 331]) == (299, 331)
    assert check_size((1024, 1)) == (1024, 1)
    assert check_size((np.int64(160), np.int32(96))) == (160, 96)
    h, w = check_size(np.array([128, 96]))
    assert (h, w) == (128, 96) and type(h) is int and type(w) is int
    import torch

    assert check_size(torch.Size([64, 80])) == (64, 80)


def test_check_size_rejects_bare_int_with_a_message():
    from ldt_amd._lib import check_size

    for v in (224, np.int64(224), True):
        with pytest.raises((TypeError, ValueError), match="shorter-edge|pair"):
            check_size(v)


@pytest.mark.parametrize("bad", [(0, 224), (224, 0), (1025, 224), (224, 1025), (-1, 5), (224,), (1, 2, 3), (),
                                 (224.0, 224), ("224", "224"), "224", b"ab", (None, 224), (True, 224), 2.5,
                                 {"h": 1, "w": 2}.keys(), object()])
def test_check_size_rejects_everything_else(bad):
    from ldt_amd._lib import check_size

    with pytest.raises((TypeError, ValueError)):
        check_size(bad)


def test_every_entry_point_validates_before_any_context(monkeypatch):
    """A bad size raises from each public function before a context (or a
    device) is asked for."""
    import pyarrow as pa

    import ldt_amd
    from ldt_amd import transforms as T

    def no_context(*a, **k):
        raise AssertionError("a context was requested before the size was validated")

    monkeypatch.setattr(T, "_decoder", no_context)
    monkeypatch.setattr(T._lib, "get_context", no_context)
    rb = pa.RecordBatch.from_arrays([pa.array([b"x"], pa.binary()), pa.array([1], pa.int64())], ["image", "label"])
    arr = rb.column(0)
    bad = 224
    calls = [
        lambda: T.decode_arrow(arr, size=bad),
        lambda: ldt_amd.decode_tensor_image(rb, size=bad),
        lambda: ldt_amd.collate_fn([{"image": b"x", "label": 1}], size=bad),
        lambda: T.make_collate_fn(size=bad),
        lambda: T.resize_raw(np.zeros((1, 2, 2, 3), np.uint8), 2, 2, size=bad),
        lambda: T.DecodePipeline(size=bad),
        lambda: T.make_to_tensor_fn(size=bad),
        lambda: T.DeviceBatch({}, size=bad),
        lambda: T.ResidentBatch.decode(object.__new__(T.ResidentBatch), size=bad),
    ]
    for k, call in enumerate(calls):
        with pytest.raises((TypeError, ValueError), match="pair"):
            call()
    with pytest.raises(ValueError):  # out of range
        T.decode_arrow(arr, size=(0, 5))
    with pytest.raises(ValueError):
        T.make_collate_fn(size=(2000, 5))


# ---- pickling ------------------------------------------------------------

def test_bound_collate_keeps_size_through_pickle():
    from ldt_amd import transforms as T

    fn = pickle.loads(pickle.dumps(T.make_collate_fn(device="cuda:0", normalize=True, size=(128, 96))))
    assert fn.size == (128, 96) and fn.device == "cuda:0" and fn.normalize is True
    assert pickle.loads(pickle.dumps(T.make_collate_fn())).size == (224, 224)


def test_device_batch_keeps_size_through_pickle():
    from ldt_amd import transforms as T

    packed = T._pack_list([b"abc", b"de"], [1, 2])
    b = pickle.loads(pickle.dumps(T.DeviceBatch(packed, "cuda:0", None, size=(160, 200))))
    assert b._size == (160, 200) and b._device == "cuda:0"
    assert len(b._packed["offsets"]) == 3
    assert pickle.loads(pickle.dumps(T.DeviceBatch(packed)))._size == (224, 224)
    # positional use as before the keyword existed
    assert T.DeviceBatch(packed, None, True)._size == (224, 224)


# ---- C ABI ---------------------------------------------------------------

def test_output_size_entry_points_declared_exported_bound():
    import re

    from ldt_amd import _lib

    src = open(os.path.join(REPO, "include", "ldt.h")).read()
    assert re.search(r"#define\s+LDT_MAX_OUT\s+1024\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(ldt_[a-z_]+)\s*\(", code))
    L = _lib.load_library()
    for s in ("ldt_set_output_size", "ldt_get_output_size"):
        assert s in declared and s in _lib.EXPORTED and hasattr(L, s), s
    assert set(_lib.EXPORTED) == declared
    assert _lib.MAX_OUT == 1024


def test_output_size_null_context_is_rejected():
    import ctypes

    from ldt_amd import _lib

    L = _lib.load_library()
    assert L.ldt_set_output_size(None, 224, 224) == _lib.LDT_ERR_ARG
    h, w = ctypes.c_int(-7), ctypes.c_int(-7)
    assert L.ldt_get_output_size(None, ctypes.byref(h), ctypes.byref(w)) == _lib.LDT_ERR_ARG
    assert (h.value, w.value) == (-7, -7)


# ---- launch geometry -----------------------------------------------------

def test_band_geometry_for_every_output_size(tmp_path):
    """tools/checks/geom4_check.cpp under ASan/UBSan: bands cover every row
    once, ring >= ks_v + 1, LDS <= 160 KB or refused, 224 x 224 unchanged."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "geom4_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                    os.path.join(REPO, "tools", "checks", "geom4_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "geom4 ok" in r.stdout
