"""CPU tests of the mix stage's arithmetic: csrc/ldt_mix.hpp, the one source
k_mix_apply and k_mix_labels run, compiled for the host (tools/checks/
mix_host.cpp, -ffp-contract=off) and called through ctypes on numpy arrays,
against torch on the CPU. Zero mismatched bits are allowed anywhere:

  * the element formula on all 256 x 256 byte pairs under ToTensor and under
    ImageNet Normalize (every channel's table), against torchvision v2's
    ``inpt.roll(1, 0).mul_(1.0 - lam).add_(inpt.mul(lam))`` and timm's
    ``x.mul_(lam).add_(x.flip(0).mul_(1. - lam))``, for lam in 0, 1, 0.5,
    0.123456789 and twenty Beta draws; weights (1, 0) return x itself;
  * the fp16 and bf16 conversions on every float32 whose low 13 bits are 0,
    0x0FFF, 0x1000 or 0x1001 (the ties and their neighbours, subnormals and the
    overflow edge included) against ``.to(dtype)``. A NaN must stay a NaN; its
    payload is not compared (torch's differs between its own code paths);
  * the soft-label closed form against ``one_hot(...).float()`` through the
    same roll / mul / add.

A stand-alone build of the same file under ASan / UBSan sweeps the functions
once more. The GPU side is tests/test_gpu_mix.py.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO

SRC = os.path.join(REPO, "tools", "checks", "mix_host.cpp")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
F16, BF16 = 1, 2  # LDT_DTYPE_*


def _cxx():
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    return cxx


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mix_host") / "libmix_host.so")
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", so], check=True)
    L = ctypes.CDLL(so)
    vp, i64, f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    L.mix_host_element.argtypes = [vp, vp, i64, f32, f32, ctypes.c_int, vp]
    L.mix_host_to16.argtypes = [vp, i64, ctypes.c_int, vp]
    L.mix_host_labels.argtypes = [vp, vp, i64, ctypes.c_int, f32, f32, vp]
    L.mix_host_in_box.argtypes = [ctypes.c_int] * 6
    for f in ("mix_host_element", "mix_host_to16", "mix_host_labels"):
        getattr(L, f).restype = None
    return L


def _tables():
    """name -> [tables of 256 float32]: ToTensor, and Normalize's three channels, as torch computes them."""
    v = torch.arange(256, dtype=torch.uint8)
    tt = v.to(torch.float32).div(255)
    return {"to_tensor": [tt], "normalize": [tt.clone().sub_(m).div_(s) for m, s in zip(MEAN, STD)]}


def _lams():
    g = torch.Generator().manual_seed(20261021)
    draws = []
    for alpha in (0.2, 0.8, 1.0, 4.0):
        for _ in range(5):
            draws.append(float(torch._sample_dirichlet(torch.tensor([[alpha, alpha]]), generator=g)[..., 0]))
    return [0.0, 1.0, 0.5, 0.123456789] + draws


def _element(host, x, p, ws, wp, boxed=0):
    x, p = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(p, np.float32)
    out = np.empty_like(x)
    host.mix_host_element(x.ctypes.data, p.ctypes.data, x.size, ws, wp, boxed, out.ctypes.data)
    return out


@pytest.mark.parametrize("name", ["to_tensor", "normalize"])
def test_element_formula_is_torchvisions_and_timms_on_every_byte_pair(host, name):
    lams = _lams()
    assert len(lams) == 24
    bad = 0
    for tab in _tables()[name]:
        x = tab.repeat_interleave(256)  # the row's value over all pairs
        p = tab.repeat(256)             # its partner's
        for lam in lams:
            got = _element(host, x.numpy(), p.numpy(), np.float32(lam), np.float32(1.0 - lam))
            tv = p.clone().mul_(1.0 - lam).add_(x.mul(lam))          # torchvision: rolled.mul_(1 - lam).add_(inpt.mul(lam))
            timm = x.clone().mul_(lam).add_(p.clone().mul_(1. - lam))  # timm: x.mul_(lam).add_(flipped.mul_(1 - lam))
            bad += int((got.view(np.int32) != tv.numpy().view(np.int32)).sum())
            bad += int((got.view(np.int32) != timm.numpy().view(np.int32)).sum())
        # CutMix's weights outside the box return x bit for bit; inside it the partner
        bad += int((_element(host, x.numpy(), p.numpy(), 1.0, 0.0).view(np.int32) != x.numpy().view(np.int32)).sum())
        bad += int((_element(host, x.numpy(), p.numpy(), 1.0, 0.0, 1).view(np.int32) != p.numpy().view(np.int32)).sum())
    assert bad == 0


@pytest.mark.parametrize("dtype,code", [(torch.float16, F16), (torch.bfloat16, BF16)])
def test_16_bit_conversions_on_every_tie_and_neighbour(host, dtype, code):
    hi = np.arange(1 << 19, dtype=np.uint32) << 13
    bits = np.concatenate([hi | lo for lo in (0x0000, 0x0FFF, 0x1000, 0x1001)]).astype(np.uint32)
    got = np.empty(bits.size, np.uint16)
    host.mix_host_to16(bits.ctypes.data, bits.size, code, got.ctypes.data)
    f = torch.from_numpy(bits.view(np.float32).copy())
    want = f.to(dtype).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(bits.view(np.float32))
    assert nan.any() and (~nan).sum() > 2_000_000
    assert int((got[~nan] != want[~nan]).sum()) == 0
    # a NaN stays one: exponent all ones, mantissa not zero
    emask, mmask = (0x7C00, 0x03FF) if code == F16 else (0x7F80, 0x007F)
    assert np.all((got[nan] & emask) == emask) and np.all((got[nan] & mmask) != 0)
    # the edges by name: subnormals kept, the overflow tie goes to inf
    if code == F16:
        probe = np.array([0x33000000, 0x33000001, 0x387FC000, 0x477FEFFF, 0x477FF000, 0xC77FF000], np.uint32)
        out = np.empty(probe.size, np.uint16)
        host.mix_host_to16(probe.ctypes.data, probe.size, code, out.ctypes.data)
        assert out.tolist() == [0x0000, 0x0001, 0x03FF, 0x7BFF, 0x7C00, 0xFC00]


def test_soft_label_closed_form_is_one_hot_through_the_same_ops(host):
    nc = 7
    rng = np.random.default_rng(5)
    lab = torch.from_numpy(np.concatenate([rng.integers(0, nc, 40), [3, 3, 0, 6, 6]]).astype(np.int64))
    bad = 0
    for lam in _lams():
        ls, lp = np.float32(lam), np.float32(1.0 - lam)
        a = lab.numpy()
        b = np.ascontiguousarray(lab.roll(1, 0).numpy())
        got = np.empty((len(a), nc), np.float32)
        host.mix_host_labels(a.ctypes.data, b.ctypes.data, len(a), nc, ls, lp, got.ctypes.data)
        hot = torch.nn.functional.one_hot(lab, nc).float()
        want = hot.roll(1, 0).mul_(1.0 - lam).add_(hot.mul(lam))
        bad += int((got.view(np.int32) != want.numpy().view(np.int32)).sum())
    assert (lab == lab.roll(1, 0)).any()  # rows of equal label are among them
    assert bad == 0


def test_box_test(host):
    inside = {(y, x) for y in range(-2, 8) for x in range(-2, 8) if host.mix_host_in_box(y, x, 1, 2, 3, 4)}
    assert inside == {(y, x) for y in range(1, 4) for x in range(2, 6)}
    assert not any(host.mix_host_in_box(y, x, 0, 0, 0, 5) for y in range(-1, 3) for x in range(-1, 3))  # height 0: none


def test_sanitizer_sweep(tmp_path):
    """The same file as a stand-alone program under ASan / UBSan, on the CPU."""
    exe = str(tmp_path / "mix_host")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-DMIX_HOST_MAIN", SRC, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "mix_host sweep" in run.stdout
