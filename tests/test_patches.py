"""CPU tests of ``decode_patches``: its argument checks (no device is asked for), the layout of a small mixed
batch, and ``ldt_decode_patches`` without a context."""
import ctypes

import numpy as np
import pytest


def _cells():
    from ldt_amd import synth

    return [synth.encode(synth.field(h, w, 4, 12.0)) for h, w in ((31, 33), (45, 67), (20, 300))]


@pytest.mark.parametrize("kw, exc, match", [
    (dict(sizes=[[28, 28], [28, 30], [56, 28]]), ValueError, "row 1"),
    (dict(sizes=[[28, 28], [28, 28], [28, 42]]), ValueError, "row 2"),  # a multiple of P, not of P * m
    (dict(sizes=[[32] * 2] * 3, patch_size=15), ValueError, "patch_size"),
    (dict(sizes=[[32] * 2] * 3, patch_size=16, merge_size=3), ValueError, "merge_size"),
    (dict(sizes=[[32] * 2] * 3, patch_size=16, temporal_patch_size=0), ValueError, "temporal_patch_size"),
    (dict(sizes=[[28] * 2] * 3, dtype="uint8", normalize=True), ValueError, None),
    (dict(sizes=None), ValueError, "sizes"),
    (dict(), TypeError, "sizes"),
])
def test_bad_arguments_need_no_device(monkeypatch, kw, exc, match):
    import ldt_amd
    from ldt_amd import transforms as T

    def no_device(device):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(T, "_decoder", no_device)
    with pytest.raises(exc, match=match):
        ldt_amd.decode_patches(_cells(), **kw)


def test_layout_of_a_mixed_batch():
    from ldt_amd import _lib

    spec = _lib.check_patch_spec(14, 2, 2)
    hw, _ = _lib.native_layout([[33, 31], [0, 0], [300, 20]], [0, 1, 0], None, np.array([[28, 56], [28, 28], [84, 532]]))
    grid, offsets = _lib.patch_layout(hw, spec)
    assert grid.tolist() == [[1, 2, 4], [1, 0, 0], [1, 6, 38]]  # the failed row has no patches
    assert offsets.tolist() == [0, 8 * 1176, 8 * 1176, (8 + 228) * 1176]
    assert _lib.patch_layout([[16, 48]], _lib.check_patch_spec(16, 1, 1))[1].tolist() == [0, 3 * 768]


def test_abi_without_a_context():
    from ldt_amd import _lib

    lib = _lib.load_library()
    spec = _lib.LdtPatch(14, 2, 2, 0)
    rc = lib.ldt_decode_patches(None, None, None, 0, 0, 1, None, None, 0, None, None, None, ctypes.byref(spec), None, None)
    assert rc == _lib.LDT_ERR_ARG
