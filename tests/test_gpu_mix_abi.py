"""GPU tests of ldt_set_mix's pending state: refused records leave nothing
pending, the mix is consumed by a failing call, NULL clears it, every
LDT_ERR_ARG case of the decode call enqueues nothing, ldt_resize_raw consumes
and refuses, and num_classes == 0 mixes the images and leaves the soft buffer
alone.
"""
import numpy as np
import pyarrow as pa
import pytest

import test_gpu_color as C
import test_gpu_mix as M
from conftest import read_golden

pytestmark = pytest.mark.gpu

SIZE = (17, 33)
NC = M.NC


@pytest.fixture(scope="module")
def cells():
    return [(name, read_golden("jpeg/" + name)) for name in C.NAMES[:3]]


def _arrow(cells):
    return pa.array([d for _, d in cells], pa.binary())


def _plain(cells, ctx):
    """A call without a mix on `ctx`; what it returns when nothing is pending."""
    return M._decode(cells, SIZE, None, ctx=ctx)[0]


def _soft(n):
    import torch

    return torch.full((n, NC), -7.0, device="cuda")


def test_refused_records_leave_nothing_pending_and_null_clears(cells):
    import torch

    import ldt_amd
    from ldt_amd import _lib

    n = len(cells)
    good = M._rows(n, box=(14, 2, 3, 5))
    ctx = _lib.Context(0)
    want = _plain(cells, ctx)
    soft = _soft(n)

    def partner_hi(r):
        r["partner"][0] = n

    def partner_neg(r):
        r["partner"][1] = -1

    def w_nan(r):
        r["w_self"][0] = np.nan

    def w_inf(r):
        r["w_partner"][2] = np.inf

    def lw_inf(r):
        r["lw_self"][1] = -np.inf

    def lw_nan(r):
        r["lw_partner"][1] = np.nan

    def box_neg(r):
        r["box"][0] = (-1, 0, 3, 3)

    def box_left(r):
        r["box"][0] = (0, -1, 3, 3)

    def box_w0(r):
        r["box"][0] = (0, 0, 3, 0)

    def box_hneg(r):
        r["box"][0] = (0, 0, -2, 3)

    for edit in (partner_hi, partner_neg, w_nan, w_inf, lw_inf, lw_nan, box_neg, box_left, box_w0, box_hneg):
        rec = good.copy()
        edit(rec)
        ctx.use_mix((good, NC, soft.data_ptr()))  # pending, then replaced by a refused set: nothing stays
        with pytest.raises(ldt_amd.LdtError, match="rc=-1"):
            ctx.use_mix((rec, NC, soft.data_ptr()))
        assert torch.equal(_plain(cells, ctx), want), edit.__name__
    for nc, ptr in ((-1, soft.data_ptr()), ((1 << 20) + 1, soft.data_ptr()), (NC, None)):
        ctx.use_mix((good, NC, soft.data_ptr()))
        with pytest.raises(ldt_amd.LdtError, match="rc=-1"):
            ctx.use_mix((good, nc, ptr))
        assert torch.equal(_plain(cells, ctx), want), (nc, ptr)
    # NULL clears
    ctx.use_mix((good, NC, soft.data_ptr()))
    assert ctx.lib.ldt_set_mix(ctx.handle, None, 0, 0, None) == 0
    assert torch.equal(_plain(cells, ctx), want)
    torch.cuda.synchronize()
    assert torch.all(soft == -7.0).item()


def test_every_refusal_of_the_decode_call_enqueues_nothing_and_consumes_the_mix(cells):
    import torch

    import ldt_amd
    from ldt_amd import _lib
    from ldt_amd import transforms as T

    n = len(cells)
    good = M._rows(n, box=(14, 2, 3, 5))
    ctx = _lib.Context(0)
    want = _plain(cells, ctx)
    soft = _soft(n)
    crops = M._crops(n, SIZE)

    def refused(what, labels=M.LABELS[:3], dtype=None, **kw):
        dt = torch.float32 if dtype is None else dtype
        shape = (kw.get("views") or 1) * n * 3 * SIZE[0] * SIZE[1]
        out = torch.full((shape,), 5, dtype=torch.uint8 if dt == torch.uint8 else dt, device="cuda")
        view = out.view(n, 3, *SIZE) if "views" not in kw and "size" not in kw else \
            (out.view(kw["views"], n, 3, *SIZE) if "views" in kw else out[:n * 3 * (8 * 8 + 4 * 4)])
        with pytest.raises(ldt_amd.LdtError, match="rc=-1"):
            T.decode_arrow(_arrow(cells), labels, out=view, ctx=ctx, dtype=dtype,
                           **({"size": SIZE, "crops": crops} | kw))
        torch.cuda.synchronize()
        assert torch.all(out == 5).item() and torch.all(soft == -7.0).item(), what  # nothing enqueued
        assert torch.equal(_plain(cells, ctx), want), what  # and the mix is gone

    ctx.use_mix((M._rows(n - 1), NC, soft.data_ptr()))
    refused("n differs from the batch")
    box = good.copy()
    box["box"][1] = (14, 30, 3, 4)
    ctx.use_mix((box, NC, soft.data_ptr()))
    refused("a box leaves the output size")
    ctx.use_mix((good, NC, soft.data_ptr()))
    refused("views pending as well", views=2, crops=np.repeat(crops[:, None], 2, axis=1))
    ctx.use_mix((good, NC, soft.data_ptr()))
    refused("a size list pending as well", size=[(8, 8), (4, 4)], crops=None)
    ctx.use_mix((good, NC, soft.data_ptr()))
    refused("uint8", dtype=torch.uint8)
    ctx.use_mix((good, NC, soft.data_ptr()))
    refused("classes without labels", labels=None)
    for bad in (-1, NC):
        ctx.use_mix((good, NC, soft.data_ptr()))
        refused(f"label {bad}", labels=np.array([3, bad, 7], np.int64))


def test_resize_raw_consumes_and_refuses_and_zero_classes_leave_the_soft_buffer(cells):
    import torch

    import ldt_amd
    from ldt_amd import transforms as T

    n = len(cells)
    good = M._rows(n, box=(14, 2, 3, 5))
    shared = T._decoder("cuda:0").ctx
    raw = torch.zeros((n, 16, 16, 3), dtype=torch.uint8)
    with shared.lock:
        shared.use_mix((good, 0, None))
    with pytest.raises(ldt_amd.LdtError, match="rc=-1"):
        T.resize_raw(raw, 16, 16, size=(8, 8), normalize=None)
    assert tuple(T.resize_raw(raw, 16, 16, size=(8, 8), normalize=None).shape) == (n, 3, 8, 8)
    with pytest.raises(TypeError):
        T.resize_raw(raw, 16, 16, size=(8, 8), normalize=None, mixes=(good, 0))
    # num_classes == 0 with a soft pointer given: images mixed, the buffer unwritten, the int64 labels as ever
    from ldt_amd import _lib

    ctx = _lib.Context(0)
    ref = _plain(cells, ctx)
    soft = _soft(n)
    ctx.use_mix((good, 0, soft.data_ptr()))
    img, none, lbl, failed = M._decode(cells, SIZE, None, ctx=ctx)
    torch.cuda.synchronize()
    assert none is None and not failed and np.array_equal(lbl, M.LABELS[:n])
    assert torch.equal(M._bits(img), M._bits(M._want(ref, good, "float32")))
    assert torch.all(soft == -7.0).item()
