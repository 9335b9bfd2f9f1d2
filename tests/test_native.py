"""CPU tests of ``decode_native``: its host-side sizes and offsets; bad arguments need no device."""
import io

import numpy as np
import pytest

from conftest import read_golden


def _jpeg(h, w, seed):
    from PIL import Image

    from ldt_amd import synth

    b = io.BytesIO()
    Image.fromarray(synth.field(h, w, seed, 12.0)).save(b, format="JPEG", quality=90)
    return b.getvalue()


def test_sizes_and_offsets():
    from ldt_amd import _lib, transforms as T

    assert "ldt_set_native" in _lib.EXPORTED and hasattr(_lib.load_library(), "ldt_set_native")
    cells = [_jpeg(31, 33, 1), _jpeg(45, 67, 2), b"", read_golden("jpeg/bad_cmyk.bin"), _jpeg(20, 300, 3)]
    drafts = [1, 4, 2, 1, 1]
    images, crops, d, hw, off = T._native_plan(cells, None, drafts)
    assert len(images) == 5 and crops is None and d.tolist() == drafts
    assert hw.tolist() == [[31, 33], [12, 17], [0, 0], [0, 0], [20, 300]]
    assert off.dtype == np.int64 and off.tolist() == [0, 3069, 3681, 3681, 3681, 21681]
    # with boxes the sizes are the boxes'; a failed row has no elements whatever its box says
    boxes = [[0, 0, 31, 33, 0], [1, 2, 3, 4, 1], [0, 0, 5, 5, 0], [0, 0, 5, 5, 0], [3, 7, 9, 11, 0]]
    _, crops, _, hw, off = T._native_plan(cells, boxes, drafts)
    assert crops.dtype == np.int32 and crops.tolist() == boxes
    assert hw.tolist() == [[31, 33], [3, 4], [0, 0], [0, 0], [9, 11]]
    assert off.tolist() == [0, 3069, 3105, 3105, 3105, 3402]
    assert T._native_plan([])[4].tolist() == [0]


@pytest.mark.parametrize("kw, exc", [
    (dict(crops=[[0, 0, 1, 1]]), ValueError),           # check_crops: [n, 5]
    (dict(drafts=[3]), ValueError),                     # check_drafts: 1, 2, 4 or 8
    (dict(dtype="int8"), ValueError),                   # check_format
    (dict(normalize=True), ValueError),                 # uint8, the default here, takes no Normalize
])
def test_bad_arguments_need_no_device(monkeypatch, kw, exc):
    import ldt_amd
    from ldt_amd import transforms as T

    class Asked(Exception):
        pass

    def no_device(device):
        raise Asked

    monkeypatch.setattr(T, "_decoder", no_device)
    cell = [_jpeg(8, 8, 4)]
    with pytest.raises(exc):
        ldt_amd.decode_native(cell, **kw)
    with pytest.raises(Asked):  # a good call gets as far as the device
        ldt_amd.decode_native(cell, dtype="float32", normalize=True, crops=[[0, 0, 1, 1, 0]], drafts=[1])
