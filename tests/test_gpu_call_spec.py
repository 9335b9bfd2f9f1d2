"""GPU tests of the one arming point and the one record of a call's options:
nothing stays pending in a context after ``Context.arm`` is refused, and one
batch with one set of options comes back the same, bit for bit, from every
decode surface.
"""
import numpy as np
import pyarrow as pa
import pytest

from conftest import read_golden
from oracle import oracle

pytestmark = pytest.mark.gpu

SIZE = (30, 33)
NAMES = ("prog_64x80.jpg", "q100_64x64.jpg", "s422_33x65.jpg", "odd_13x17.jpg")  # progressive, 4:4:4/4:2:0, 4:2:2, odd
NAN = float("nan")
ORDER0123 = 0 + 4 * 1 + 16 * 2 + 64 * 3


@pytest.fixture(scope="module")
def cells():
    return [read_golden("jpeg/" + name) for name in NAMES]


def _batch(cells):
    return pa.RecordBatch.from_arrays([pa.array(cells, pa.binary()), pa.array(range(len(cells)), pa.int64())],
                                      ["image", "label"])


def test_nothing_stays_pending_after_a_failed_arm(cells):
    import torch

    import ldt_amd
    from ldt_amd import _lib
    from ldt_amd import transforms as T

    n = len(cells)
    ctx = _lib.Context(0)
    crops = _lib.check_crops(np.tile(np.array([1, 1, 8, 9, 1]), (n, 1)), n)
    colors = _lib.check_colors(np.tile(np.array([1.2, NAN, NAN, NAN, ORDER0123, 0, -1]), (n, 1)), n).copy()
    colors["mask"][0] = 16  # Python's check never makes this; the library refuses it
    with ctx.lock, pytest.raises(ldt_amd.LdtError, match="rc=-1"):
        ctx.arm(SIZE, "bilinear", "float32", "contiguous", crops=crops, colors=colors)
    img, lbl = T.decode_arrow(pa.array(cells, pa.binary()), None, ctx=ctx, size=SIZE)
    torch.cuda.synchronize()
    assert lbl is None and tuple(img.shape) == (n, 3) + SIZE
    got = img.cpu().numpy()
    for i, data in enumerate(cells):  # the whole image, not the parked box
        assert np.array_equal(got[i], oracle.jpeg_to_tensor(data, *SIZE)), NAMES[i]


def _stage_options(stage, n):
    if stage == "colors":
        rows = np.array([[1.2, 0.7, NAN, 0.1, ORDER0123, 0, -1], [NAN, 1.4, 0.5, NAN, 27, 1, 128]])
        return np.tile(rows, (n, 1, 1))
    rows = np.full((2, 2, 10), NAN)
    rows[0, 0, :7], rows[0, 0, 7:] = (1, 1.0, 0.2, 0.0, -0.2, 1.0, 0.0), (128, 0, 255)  # an affine op
    rows[0, 1, 0] = 8  # then AutoContrast (a statistics pass)
    rows[1, 0, :2] = (4, 1.5)  # contrast, one op only
    return np.tile(rows, (n, 1, 1, 1))


@pytest.mark.parametrize("stage", ["colors", "augments"])
def test_one_batch_is_the_same_on_every_surface(cells, stage):
    import torch

    import ldt_amd
    from ldt_amd import transforms as T

    n = len(cells)
    rb = _batch(cells)
    items = [{"image": c, "label": k} for k, c in enumerate(cells)]
    crops = np.tile(np.array([[1, 1, 8, 9, 0], [2, 0, 10, 12, 1]], np.int32), (n, 1, 1))
    common = dict(size=SIZE, views=2, dtype=torch.float16, memory_format=torch.channels_last)
    plural = {"crops": crops, stage: _stage_options(stage, n)}  # decode_arrow's names
    single = {"crop": crops, stage[:-1]: plural[stage]}  # the plug-ins'
    ref, ref_lbl = T.decode_arrow(rb.column(0), list(range(n)), **common, **plural)
    assert tuple(ref.shape) == (2, n, 3) + SIZE and ref.dtype == torch.float16
    assert ref.stride() == (n * 3 * 30 * 33, 3 * 30 * 33, 1, 3 * 33, 3)
    assert not torch.equal(ref[0], ref[1])

    resident = T.ResidentBatch(cells, range(n))
    pipe = T.DecodePipeline(depth=2, **common)
    fn = T.make_to_tensor_fn(**common, **single)
    got = {
        "ResidentBatch.decode": resident.decode(**common, **plural),
        "DecodePipeline.decode(RecordBatch)": pipe.decode(rb, **plural),
        "DecodePipeline.decode(ResidentBatch)": pipe.decode(resident, **plural),
        "collate_fn": T.collate_fn(items, **common, **single),
        "decode_tensor_image": T.decode_tensor_image(rb, **common, **single),
        "make_to_tensor_fn": fn(rb),
    }
    pipe.check()
    fn.check()
    torch.cuda.synchronize()
    for what, res in got.items():
        img, lbl = (res["image"], res["label"]) if isinstance(res, dict) else res
        assert img.dtype == ref.dtype and img.stride() == ref.stride(), what
        assert torch.equal(img.contiguous().view(torch.uint8), ref.contiguous().view(torch.uint8)), what
        assert torch.equal(lbl, ref_lbl), what
