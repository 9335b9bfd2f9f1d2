"""GPU tests of what a call inherits from the call before it on the same context: every ordered pair of the call
kinds of tests/call_kinds.py, the orders that shrink and grow every buffer, and unsynchronised random walks over two
streams. The second call of a pair is compared byte for byte with the same call on a context that has done nothing
else (its baseline), and the baseline itself with Pillow / the oracle (``Kind.reference``) under the bar of the
feature's own test: tests/test_gpu_window.py's ``_check`` (max abs <= 2/255, then bit equality) for float32 images,
every byte for the integer paths, the formats, the labels, the soft labels and the row statuses.

No test here waits or clears anything between two calls beyond what the calls do themselves.
"""
import numpy as np
import pytest

import call_kinds as ck

pytestmark = pytest.mark.gpu

NAMES = [k.name for k in ck.KINDS]
WALK = 40


def _against_reference(got, kind):
    from test_gpu_window import _check

    ref = kind.reference()
    assert len(got["images"]) == len(ref["images"]), (kind.name, len(got["images"]), len(ref["images"]))
    for k, (g, w) in enumerate(zip(got["images"], ref["images"])):
        if w.dtype == np.float32 and g.dtype == w.dtype and g.shape == w.shape:
            for i in range(len(w)):
                _check(g[i], w[i], f"{kind.name}: image {k} row {i}")
    ck.diff(got, ref, f"{kind.name} on a fresh context against its reference")


@pytest.fixture(scope="module")
def baselines():
    """{name: host arrays} of every kind on a fresh context of its own, and under ``"errors"`` what held a baseline
    against its reference did not hold (test_baseline reports it; the sequence tests compare with the arrays)."""
    from ldt_amd import _lib

    out, errors = {}, {}
    for kind in ck.KINDS:
        ctx = _lib.Context(0)
        out[kind.name] = kind.run(ctx)
        del ctx
        try:
            _against_reference(out[kind.name], kind)
        except AssertionError as e:
            errors[kind.name] = e
    out["errors"] = errors
    return out


@pytest.mark.parametrize("name", NAMES)
def test_baseline(baselines, name):
    if name in baselines["errors"]:
        raise baselines["errors"][name]
    if ck.BY_NAME[name].fails is not None:
        assert baselines[name]["status"] == ck.BY_NAME[name].fails


@pytest.mark.parametrize("first", NAMES)
def test_after(baselines, first):
    """A, B for every kind B on one context: the chain A, B1, A, B2, ..."""
    from ldt_amd import _lib

    ctx, a = _lib.Context(0), ck.BY_NAME[first]
    for b in ck.KINDS:
        ck.diff(a.run(ctx), baselines[a.name], f"{a.name} before {b.name} (after the chain so far)")
        ck.diff(b.run(ctx), baselines[b.name], f"{b.name} after {a.name}")


def test_shrinking_and_growing(baselines):
    """Outputs from the largest to the smallest and back, then the batch that makes every buffer larger than the
    others need between every two kinds."""
    from ldt_amd import _lib

    ctx = _lib.Context(0)
    size = lambda k: sum(a.nbytes for a in baselines[k.name]["images"])  # noqa: E731
    down = sorted(ck.KINDS, key=size, reverse=True)
    assert size(down[0]) > size(down[-2]) > 0  # (the refused call, last, has no output)
    order = down + down[::-1]
    for k in ck.KINDS:
        order += [ck.BY_NAME["big-first"], k]
    for step, k in enumerate(order):
        ck.diff(k.run(ctx), baselines[k.name], f"step {step}: {k.name} after {order[step - 1].name if step else None}")


def _walk(ctx, seed, baselines):
    """WALK calls drawn with ``seed`` from the kinds that can run without a wait, alternately on two streams, under
    LDT_OPT_SYNC_STATUS = 0; one synchronisation at the end, then every result against its baseline. A failing
    kind's statuses are read by ticket once the next call is enqueued (the context holds a call's status for two
    calls): that waits for the failing call alone, never for the newer one."""
    import torch

    from ldt_amd import _lib

    kinds = [k for k in ck.KINDS if k.asynchronous]
    assert len(kinds) == len(ck.KINDS) - 1
    rng = np.random.RandomState(seed)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    calls = []
    ctx.set_option(_lib.OPT_SYNC_STATUS, 0)
    try:
        for step in range(WALK):
            kind = kinds[rng.randint(len(kinds))]
            calls.append((kind, kind.launch(ctx, streams[step & 1])))
            if step:
                calls[-2][1].fetch_status()
        torch.cuda.synchronize()
    finally:
        ctx.set_option(_lib.OPT_SYNC_STATUS, 1)
    for step, (kind, pending) in enumerate(calls):
        ck.diff(pending.host(), baselines[kind.name],
                f"seed {seed} step {step}: {kind.name} after {calls[step - 1][0].name if step else None}")
    return [k.name for k, _ in calls]


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_unsynchronised_walk(baselines, seed):
    from ldt_amd import _lib

    names = _walk(_lib.Context(0), seed, baselines)
    assert len(names) == WALK and len(set(names)) > 10


def test_shared_context_after_the_walk(baselines):
    """The same walk on the context the rest of the suite shares, then the default call against the oracle: the
    shared context is left as the other files expect it."""
    import pyarrow as pa

    import ldt_amd
    from ldt_amd import _lib
    from oracle import oracle
    from test_gpu_window import _check

    ctx = _lib.get_context(0)
    _walk(ctx, 14, baselines)
    cells = [c[0] for c in ck.cells()]
    img, lbl = ldt_amd.decode_arrow(pa.array(cells, pa.binary()), ck.LABELS)
    assert ctx.output_size() == (224, 224) and ctx.filter() == "bilinear"
    assert ctx.output_format() == ("float32", "contiguous")
    assert lbl.cpu().numpy().tolist() == ck.LABELS.tolist()
    img = img.cpu().numpy()
    for i, data in enumerate(cells):
        _check(img[i], oracle.jpeg_to_tensor(data), f"plain 224 x 224 on the shared context, row {i}")
