"""GPU tests of ldt_set_augments' pending state: refused entries leave nothing
pending, a wrong entry count enqueues nothing, augments and colours pending
together are refused and both consumed, ldt_resize_raw consumes pending
augments, and the call after a call with augments is a plain call. The stage is
profiled under the colour stage's entry.
"""
import numpy as np
import pyarrow as pa
import pytest

import test_gpu_augment as A
import test_gpu_color as C
from conftest import read_golden

pytestmark = pytest.mark.gpu

SIZE = (24, 28)


@pytest.fixture(scope="module")
def cells():
    return [(name, read_golden("jpeg/" + name)) for name in C.NAMES[:3]]


def _good(n):
    from ldt_amd import _lib

    rows = np.full((n, 2, 10), A.NAN, np.float64)
    rows[:, 0], rows[:, 1] = A._row(4, 1.5), A._row(9)
    return rows, _lib.check_augments(rows, n, None, SIZE)


def _arrow(cells):
    return pa.array([d for _, d in cells], pa.binary())


def test_refused_entries_leave_nothing_pending(cells):
    import ldt_amd
    from ldt_amd import _lib

    n = len(cells)
    _, good = _good(n)
    ctx = _lib.Context(0)

    def bad(edit):
        rec = good.copy()
        edit(rec)
        return rec

    def count5(r):
        r["count"][0] = 5

    def count_neg(r):
        r["count"][1] = -1

    def code11(r):
        r["op"]["code"][0, 0] = 11

    def factor_nan(r):
        r["op"]["factor"][0, 0] = np.nan

    def factor_neg(r):
        r["op"]["factor"][2, 0] = -0.5

    def bits9(r):
        r["op"]["code"][0, 1], r["op"]["param"][0, 1] = 6, 9

    def thr257(r):
        r["op"]["code"][0, 1], r["op"]["param"][0, 1] = 7, 257

    def box_neg(r):
        r["erase"][0] = (-1, 0, 3, 3)

    def box_w0(r):
        r["erase"][0] = (0, 0, 3, 0)

    for edit in (count5, count_neg, code11, factor_nan, factor_neg, bits9, thr257, box_neg, box_w0):
        ctx.use_augments(good)  # pending, then replaced by a refused set: nothing stays
        with pytest.raises(ldt_amd.LdtError, match="rc=-1"):
            ctx.use_augments(bad(edit))
        res, lbl, failed = A._decode(cells, SIZE, None, ctx=ctx)
        A._check(cells, SIZE, None, res, lbl, failed, f"after {edit.__name__}")


def test_wrong_count_size_dependent_refusals_and_plain_call_after(cells):
    import torch

    import ldt_amd
    from ldt_amd import _lib
    from ldt_amd import transforms as T

    n = len(cells)
    rows, good = _good(n)
    ctx = _lib.Context(0)
    ctx.set_option(_lib.OPT_PROFILE, 1)

    def refused(what):
        out = torch.full((n, 3) + SIZE, -7.0, device="cuda")
        with pytest.raises(ldt_amd.LdtError, match="rc=-1"):
            T.decode_arrow(_arrow(cells), None, out=out, size=SIZE, ctx=ctx)
        torch.cuda.synchronize()
        assert torch.all(out == -7.0).item(), what  # nothing enqueued

    ctx.use_augments(good[:-1])  # pending for another count
    refused("wrong count")
    res, lbl, failed = A._decode(cells, SIZE, None, ctx=ctx)  # that call consumed them
    A._check(cells, SIZE, None, res, lbl, failed, "after a wrong count")
    assert ctx.stage_times()["color"][1] == 0
    # an erase box that leaves this call's output, a walk that leaves int32 over it
    box = good.copy()
    box["erase"][1] = (20, 0, 5, 5)
    ctx.use_augments(box)
    refused("erase box outside")
    walk = good.copy()
    walk["op"]["code"][0, 0] = 1
    walk["op"]["a"][0, 0] = (2 ** 31 - 1, 0, 0, 0, 65536, 0)
    ctx.use_augments(walk)
    refused("walk leaves int32")
    # a call with augments, then one without: the stage is timed as the colour stage, once
    res, lbl, failed = A._decode(cells, SIZE, good, ctx=ctx)
    A._check(cells, SIZE, rows, res, lbl, failed, "with augments")
    assert ctx.stage_times()["color"][1] == 1
    res, lbl, failed = A._decode(cells, SIZE, None, ctx=ctx)
    A._check(cells, SIZE, None, res, lbl, failed, "after a call with augments")
    st = ctx.stage_times()
    assert st["color"][1] == 1 and st["resize"][1] == 3
    # NULL clears
    ctx.use_augments(good[:-1])
    assert ctx.lib.ldt_set_augments(ctx.handle, None, 0) == 0
    res, lbl, failed = A._decode(cells, SIZE, None, ctx=ctx)
    A._check(cells, SIZE, None, res, lbl, failed, "after a clear")


def test_augments_and_colours_together_and_resize_raw(cells):
    import torch

    import ldt_amd
    from ldt_amd import _lib
    from ldt_amd import transforms as T

    n = len(cells)
    _, good = _good(n)
    colors = _lib.check_colors(np.array([[1.2, C.NAN, C.NAN, C.NAN, C.ORDER0123, 0, -1]] * n), n)
    ctx = _lib.Context(0)
    ctx.use_augments(good)
    ctx.use_colors(colors)
    out = torch.full((n, 3) + SIZE, -7.0, device="cuda")
    with pytest.raises(ldt_amd.LdtError, match="rc=-1"):
        T.decode_arrow(_arrow(cells), None, out=out, size=SIZE, ctx=ctx)
    torch.cuda.synchronize()
    assert torch.all(out == -7.0).item()
    res, lbl, failed = A._decode(cells, SIZE, None, ctx=ctx)  # both consumed
    A._check(cells, SIZE, None, res, lbl, failed, "after augments + colours")
    # raw sources are out of scope: resize_raw with augments pending is refused and consumes them
    shared = T._decoder("cuda:0").ctx
    raw = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    with shared.lock:
        shared.use_augments(_lib.check_augments(None, 2, None, (8, 8), np.array([[0, 0, 2, 2]] * 2)))
    with pytest.raises(ldt_amd.LdtError, match="rc=-1"):
        T.resize_raw(raw, 16, 16, size=(8, 8), normalize=None)
    assert tuple(T.resize_raw(raw, 16, 16, size=(8, 8), normalize=None).shape) == (2, 3, 8, 8)
    with pytest.raises(TypeError):
        T.resize_raw(raw, 16, 16, size=(8, 8), normalize=None, augments=good[:2])
