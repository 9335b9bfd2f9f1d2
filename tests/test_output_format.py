"""dtype= and memory_format= (ldt_set_output_format), the part that needs no
GPU:

* the planner's float32 -> fp16 / bf16 rounding and the 16-bit tables the
  resize kernels index, bit for bit against torch's ``Tensor.to(dtype)``,
  through the stand-alone program tools/checks/format_check.cpp built with
  ASan/UBSan together with the planner and run directly;
* ``check_dtype`` / ``check_memory_format``: every accepted spelling, every
  refusal by name, uint8 with a Normalize refused before a device is needed;
* what carries the two names to another process (pickling, a spawn worker);
* the C ABI: the header's two functions and six constants.

The GPU side is tests/test_gpu_output_format.py.
"""
import inspect
import os
import pickle
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from test_worker_paths import _cells, cell_ds  # noqa: F401  (the worker tests' dataset fixture)

SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
       "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
# a std small enough to take (v / 255 - mean) / std past fp16's 65504: +-inf entries
HOSTILE = ((0.5, 0.25, 0.75), (1e-6, 3e-6, 2.5e-6))


@pytest.fixture(scope="module")
def format_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("format") / "format_check")
    src = [os.path.join(REPO, "tools", "checks", "format_check.cpp"),
           os.path.join(REPO, "lance-distributed-training_amd", "csrc", "ldt_plan.cpp")]
    subprocess.run([cxx, *SAN, *src, "-o", exe], check=True)
    return exe


def _run(exe, args, word):
    r = subprocess.run([exe, *args], capture_output=True, timeout=600, env=ENV)
    assert r.returncode == 0 and not r.stderr and r.stdout.decode().strip() == word, \
        (r.returncode, r.stdout.decode()[-2000:], r.stderr.decode(errors="replace")[-4000:])


# ---- 1. the rounding ---------------------------------------------------------------------------

# Low half-words. bf16 drops all 16 of them: the tie is 0x8000. fp16 drops the
# low 13 bits of a normal value: ties at 0x1000 (even neighbour below) and
# 0x3000 (odd), and 0x5000 ... 0xF000 with the kept bits set; a subnormal
# result drops 14 to 24 bits: ties at 0x2000 / 0x6000, 0x4000 / 0xC000 and
# 0x8000 in this half, and in the high half-word (low half 0, which the sweep
# of every high half-word covers, with 0x0001 above it and 0xFFFF of the
# high half-word below as its neighbours).
_TIES = [0x1000, 0x3000, 0x5000, 0x7000, 0x9000, 0xB000, 0xD000, 0xF000, 0x2000, 0x6000, 0xA000, 0xE000,
         0x4000, 0xC000, 0x8000]
LOWS = sorted({0x0000, 0x0001, 0xFFFF, 0xFFFE} | {(t + d) & 0xFFFF for t in _TIES for d in (-1, 0, 1)})


def _rounding_inputs():
    hi = np.arange(1 << 16, dtype=np.uint32) << 16
    bits = (hi[:, None] | np.array(LOWS, np.uint32)[None, :]).reshape(-1)
    bits = bits[(bits & 0x7FFFFFFF) <= 0x7F800000]  # NaN inputs are excluded; +-inf stay
    return bits


def test_inputs_hit_what_the_rounding_can_get_wrong():
    bits = _rounding_inputs()
    for b in (0x477FE000,  # 65504, fp16's largest finite value
              0x477FEFFF, 0x477FF000, 0x477FF001,  # below, at and above the tie that overflows to inf
              0x47800000, 0xC77FF000,  # 65536; the negative tie
              0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF,  # bf16's largest finite value, and its overflow
              0x38800000, 0x387FFFFF, 0x387FF000,  # fp16's smallest normal 2^-14, just below: subnormal results
              0x33000000, 0x33000001, 0x32FFFFFF, 0x33800000,  # the tie 2^-25 -> 0, its neighbours, 2^-24
              0x33C00000, 0x34400000,  # 1.5 * 2^-24 (tie, up to even 2), 2.5 * 2^-24... (ties between subnormals)
              0x00000001, 0x00800000, 0x80000000,  # float32 subnormal, smallest normal, -0
              0x3F801000, 0x3F803000, 0x3F800FFF, 0x3F801001,  # fp16 ties around 1.0 and their neighbours
              0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001,  # bf16 ties around 1.0 and their neighbours
              0x7F800000, 0xFF800000):
        assert np.any(bits == np.uint32(b)), hex(b)
    assert len(bits) > 2_500_000 and len(np.unique(bits)) == len(bits)


def test_rounding_equals_torch_bit_for_bit(format_check, tmp_path):
    import torch

    bits = _rounding_inputs()
    src, o16, ob16 = (str(tmp_path / n) for n in ("in.f32", "out.f16", "out.bf16"))
    bits.tofile(src)
    _run(format_check, ["convert", src, o16, ob16], "convert ok")
    x = torch.from_numpy(bits.view(np.float32).copy())
    for path, dtype in ((o16, torch.float16), (ob16, torch.bfloat16)):
        got = np.fromfile(path, np.uint16)
        want = x.to(dtype).view(torch.int16).numpy().view(np.uint16)
        assert got.shape == want.shape
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (dtype, bad.size, [(hex(int(bits[i])), hex(int(got[i])), hex(int(want[i])))
                                                 for i in bad[:8]])


# ---- 2. the table ------------------------------------------------------------------------------

@pytest.mark.parametrize("norm", [None, IMAGENET, HOSTILE], ids=["none", "imagenet", "hostile"])
def test_tables_equal_torch_bit_for_bit(format_check, tmp_path, norm):
    import torch

    o32, o16, ob16 = (str(tmp_path / n) for n in ("lut.f32", "lut.f16", "lut.bf16"))
    args = ["none"] if norm is None else [f"{float(np.float32(v)):.9g}" for v in (*norm[0], *norm[1])]
    _run(format_check, ["table", *args, o32, o16, ob16], "table ok")
    f32 = np.fromfile(o32, np.float32)
    assert f32.shape == (768,)
    # build_lut itself: torchvision's to_tensor (float32(v) / 255), then sub_(mean).div_(std) in float32
    v = torch.arange(256, dtype=torch.float32).div(255).repeat(3, 1)
    if norm is not None:
        v = v.sub(torch.tensor(norm[0], dtype=torch.float32)[:, None]).div(
            torch.tensor(norm[1], dtype=torch.float32)[:, None])
    assert np.array_equal(f32.view(np.uint32), v.reshape(-1).numpy().view(np.uint32))
    for path, dtype in ((o16, torch.float16), (ob16, torch.bfloat16)):
        got = np.fromfile(path, np.uint16)
        want = torch.tensor(f32).to(dtype).view(torch.int16).numpy().view(np.uint16)
        assert np.array_equal(got, want), (dtype, np.nonzero(got != want)[0][:8])
    if norm is HOSTILE:
        h = torch.from_numpy(np.fromfile(o16, np.uint16).view(np.int16).copy()).view(torch.float16)
        assert torch.isinf(h).any() and (h == float("-inf")).any() and (h == float("inf")).any()
        assert not torch.isnan(h).any()


# ---- 3. the validators -------------------------------------------------------------------------

def test_check_dtype_and_memory_format_accept():
    import torch

    import ldt_amd
    from ldt_amd import _lib

    assert ldt_amd.check_dtype is _lib.check_dtype and ldt_amd.check_memory_format is _lib.check_memory_format
    for v in (None, torch.float32, torch.float, "float32"):
        assert _lib.check_dtype(v) == "float32", v
    for v in (torch.float16, torch.half, "float16", "half"):
        assert _lib.check_dtype(v) == "float16", v
    for v in (torch.bfloat16, "bfloat16"):
        assert _lib.check_dtype(v) == "bfloat16", v
    for v in (torch.uint8, "uint8"):
        assert _lib.check_dtype(v) == "uint8", v
    for v in (None, torch.contiguous_format, "contiguous"):
        assert _lib.check_memory_format(v) == "contiguous", v
    for v in (torch.channels_last, "channels_last"):
        assert _lib.check_memory_format(v) == "channels_last", v
    for name in _lib.DTYPES:
        assert _lib.check_dtype(_lib.check_dtype(name)) == name and pickle.loads(pickle.dumps(name)) == name
    for name in _lib.LAYOUTS:
        assert _lib.check_memory_format(_lib.check_memory_format(name)) == name
    assert _lib.DTYPES == {"float32": 0, "float16": 1, "bfloat16": 2, "uint8": 3}
    assert _lib.LAYOUTS == {"contiguous": 0, "channels_last": 1}


def test_check_dtype_and_memory_format_refuse_by_name():
    import torch

    from ldt_amd import _lib

    for v in (torch.float64, torch.int8, "fp8", "float64", "int8", torch.preserve_format, 3, 0, True, np.float32,
              "Float16", "", b"uint8", torch.int16, torch.channels_last, "channels_last"):
        with pytest.raises(ValueError) as e:
            _lib.check_dtype(v)
        assert repr(v) in str(e.value) and "torch.bfloat16" in str(e.value), (v, str(e.value))
    for v in (torch.preserve_format, torch.channels_last_3d, "nhwc", "preserve", 3, 1, True, torch.float16,
              "float16", "", "Channels_Last"):
        with pytest.raises(ValueError) as e:
            _lib.check_memory_format(v)
        assert repr(v) in str(e.value) and "torch.channels_last" in str(e.value), (v, str(e.value))


def test_every_entry_point_takes_the_arguments_and_validates_before_it_needs_a_device():
    import pyarrow as pa
    import torch

    from ldt_amd import _lib
    from ldt_amd import transforms as T

    for fn in (T.decode_arrow, T.collate_fn, T.make_collate_fn, T.resize_raw, T.ResidentBatch.decode,
               T.DecodePipeline.__init__, T.make_to_tensor_fn, T.DeviceBatch.__init__, T._BoundCollate.__init__):
        for name in ("dtype", "memory_format"):
            assert inspect.signature(fn).parameters[name].default is None, (fn, name)
    # per pipeline, like the size: not per call
    assert "dtype" not in inspect.signature(T.DecodePipeline.decode).parameters
    rb = pa.RecordBatch.from_arrays([pa.array([b"x"], pa.binary())], names=["image"])
    raw = torch.zeros((1, 4, 4, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="float64"):
        T.decode_tensor_image(rb, dtype=torch.float64)
    with pytest.raises(ValueError, match="int8"):
        T.collate_fn([{"image": b"x"}], dtype=torch.int8)
    with pytest.raises(ValueError, match="fp8"):
        T.make_collate_fn(dtype="fp8")
    with pytest.raises(ValueError, match="preserve_format"):
        T.DeviceBatch(T._pack_list([b"x"], None), memory_format=torch.preserve_format)
    with pytest.raises(ValueError, match="memory_format=3"):
        T.decode_arrow(pa.array([b"x"], pa.binary()), memory_format=3)
    with pytest.raises(ValueError, match="float64"):
        T.resize_raw(raw, 4, 4, dtype="float64")
    with pytest.raises(ValueError, match="preserve_format"):
        T.make_to_tensor_fn(memory_format=torch.preserve_format)
    # uint8 is the image before ToTensor: a Normalize cannot apply
    for norm in (True, IMAGENET):
        with pytest.raises(ValueError, match="uint8.*normalize"):
            T.decode_tensor_image(rb, dtype=torch.uint8, normalize=norm)
        with pytest.raises(ValueError, match="uint8.*normalize"):
            T.collate_fn([{"image": b"x"}], dtype="uint8", normalize=norm)
        with pytest.raises(ValueError, match="uint8.*normalize"):
            T.make_collate_fn(dtype=torch.uint8, normalize=norm)
        with pytest.raises(ValueError, match="uint8.*normalize"):
            T.decode_arrow(pa.array([b"x"], pa.binary()), dtype=torch.uint8, normalize=norm)
        with pytest.raises(ValueError, match="uint8.*normalize"):
            T.DeviceBatch(T._pack_list([b"x"], None), normalize=norm, dtype=torch.uint8)
        with pytest.raises(ValueError, match="uint8.*normalize"):
            T.make_to_tensor_fn(dtype=torch.uint8, normalize=norm)
    with pytest.raises(ValueError, match="uint8.*normalize"):
        T.resize_raw(raw, 4, 4, dtype=torch.uint8)  # resize_raw normalizes by default
    assert _lib.check_format(torch.uint8, None, None) == ("uint8", "contiguous")
    assert _lib.check_format("uint8", torch.channels_last, False) == ("uint8", "channels_last")
    assert hasattr(_lib.Context, "use_format")


def test_out_is_checked_under_a_non_default_format_only():
    import torch

    from ldt_amd import transforms as T

    good = torch.empty((2, 5, 4, 3), dtype=torch.bfloat16).permute(0, 3, 1, 2)
    assert good.stride() == (60, 1, 12, 3)
    T._check_out(good, 2, (5, 4), "bfloat16", "channels_last")
    for bad, fmt in ((good, ("float16", "channels_last")), (good, ("bfloat16", "contiguous")),
                     (good.contiguous(), ("bfloat16", "channels_last")), (good[:1], ("bfloat16", "channels_last")),
                     (torch.empty((2, 3, 5, 4)), ("uint8", "contiguous"))):
        with pytest.raises(ValueError, match="out="):
            T._check_out(bad, 2, (5, 4), *fmt)
    T._check_out(torch.empty((1,), dtype=torch.int64), 2, (5, 4), "float32", "contiguous")  # the defaults: on trust
    # the strides are exact where h or w is 1, too
    for size in ((1, 9), (9, 1), (1, 1)):
        t = T._empty_image(3, size, "uint8", "channels_last", "cpu")
        assert tuple(t.shape) == (3, 3) + size and t.stride() == (3 * size[0] * size[1], 1, 3 * size[1], 3)
        assert t.dtype == torch.uint8
    t = T._empty_image(3, (7, 5), "float32", "contiguous", "cpu")
    assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (3, 3, 7, 5)


# ---- 4. what carries the names to another process ----------------------------------------------

def test_pickle_round_trips():
    import torch

    import ldt_amd
    from ldt_amd import transforms as T

    fn = pickle.loads(pickle.dumps(ldt_amd.make_collate_fn(dtype=torch.bfloat16, memory_format=torch.channels_last,
                                                           size=(30, 33))))
    assert (fn.dtype, fn.memory_format, fn.size) == ("bfloat16", "channels_last", (30, 33))
    fn = pickle.loads(pickle.dumps(ldt_amd.make_collate_fn(dtype="half")))
    assert (fn.dtype, fn.memory_format) == ("float16", "contiguous")
    fn = pickle.loads(pickle.dumps(ldt_amd.make_collate_fn()))
    assert (fn.dtype, fn.memory_format) == ("float32", "contiguous")
    cells = _cells(5)
    b = T.DeviceBatch(T._pack_list(cells, list(range(5))), size=(30, 33), dtype=torch.uint8,
                      memory_format="channels_last")
    b2 = pickle.loads(pickle.dumps(b))
    assert (b2._dtype, b2._memory_format, b2._size) == ("uint8", "channels_last", (30, 33))
    arr, lab = T._unpack(b2._packed)
    assert arr.to_pylist() == cells and lab.tolist() == list(range(5))
    b3 = pickle.loads(pickle.dumps(T.DeviceBatch(T._pack_list(cells, None))))
    assert (b3._dtype, b3._memory_format) == ("float32", "contiguous")


def test_the_format_travels_with_the_cells_from_a_spawn_worker(cell_ds):  # noqa: F811
    """make_collate_fn(dtype=..., memory_format=...) in a stock DataLoader
    spawn worker: the DeviceBatch that reaches the main process names both."""
    import torch
    from torch.utils.data import DataLoader

    from ldt_amd import SafeLanceDataset, make_collate_fn
    from ldt_amd import transforms as T

    ds, cells = cell_ds
    dl = DataLoader(SafeLanceDataset(ds.uri), batch_size=32, shuffle=False, num_workers=1,
                    collate_fn=make_collate_fn(dtype=torch.float16, memory_format=torch.channels_last, size=(30, 33)),
                    pin_memory=False, multiprocessing_context="spawn")
    got = []
    for b in dl:
        assert isinstance(b, T.DeviceBatch)
        assert (b._dtype, b._memory_format, b._size) == ("float16", "channels_last", (30, 33))
        got += T._unpack(b._packed)[0].to_pylist()
    assert got == cells


# ---- 5. the C ABI ------------------------------------------------------------------------------

def test_the_header_declares_the_format_and_the_library_exports_it():
    from ldt_amd import _lib

    src = open(os.path.join(REPO, "include", "ldt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+ldt_set_output_format\s*\(\s*ldt_ctx\s*\*\s*\w*,\s*int\s+dtype,\s*int\s+layout\s*\)", code)
    assert re.search(r"\bint\s+ldt_get_output_format\s*\(\s*ldt_ctx\s*\*\s*\w*,\s*int\s*\*\s*dtype,\s*int\s*\*\s*layout\s*\)",
                     code)
    consts = dict(re.findall(r"#define\s+(LDT_(?:DTYPE|LAYOUT)_\w+)\s+(-?\d+)", code))
    assert consts == {"LDT_DTYPE_F32": "0", "LDT_DTYPE_F16": "1", "LDT_DTYPE_BF16": "2", "LDT_DTYPE_U8": "3",
                      "LDT_LAYOUT_NCHW": "0", "LDT_LAYOUT_NHWC": "1"}
    assert {k: str(v) for k, v in _lib.DTYPES.items()} == {"float32": consts["LDT_DTYPE_F32"],
                                                           "float16": consts["LDT_DTYPE_F16"],
                                                           "bfloat16": consts["LDT_DTYPE_BF16"],
                                                           "uint8": consts["LDT_DTYPE_U8"]}
    lib = _lib.load_library()
    for name in ("ldt_set_output_format", "ldt_get_output_format"):
        assert name in _lib.EXPORTED and hasattr(lib, name)
    assert lib.ldt_set_output_format(None, 1, 1) == _lib.LDT_ERR_ARG
    assert lib.ldt_get_output_format(None, None, None) == _lib.LDT_ERR_ARG
