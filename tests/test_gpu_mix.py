"""GPU tests of ``mix=`` / ``mixes=`` (ldt_set_mix): MixUp / CutMix with soft
labels, fused as the last stage before the store.

The reference of every case is the same call without ``mix=`` in float32 (held
against the oracle by the other suites), put through torchvision's ops on the
CPU (``partner.mul_(w_partner).add_(own.mul(w_self))``, the partner's pixels
inside the box) and ``.to(dtype)``; the soft labels are ``one_hot(...).float()``
through the same ops. Every comparison is bit for bit. A failed row is all-zero
bytes with a zero soft row and label -100; a row whose partner failed equals
the unmixed row with a one-hot soft row. Every decode goes into the middle of a
buffer full of a sentinel, and the bytes around the output are checked.
"""
import numpy as np
import pyarrow as pa
import pytest

import test_gpu_color as C
from conftest import read_golden

pytestmark = pytest.mark.gpu

NAN = float("nan")
NC = 11
LABELS = np.array([3, 7, 7, 0, 10], np.int64)  # rows 1 and 2 share a label; roll(1) pairs them
LAM = 0.123456789


@pytest.fixture(scope="module")
def cells():
    return [(name, read_golden("jpeg/" + name)) for name in C.NAMES]  # progressive and grey sources among them


def _crops(n, size):
    """A box per row small enough for every size here to stay inside the filter's reduction limit."""
    h, w = min(2 * size[0], 60), min(2 * size[1], 60)
    return np.array([[3, 5, h, w, i & 1] for i in range(n)], np.int32)


def _rows(n, lam=LAM, box=(0, 0, 0, 0), partner=None, cut=False):
    from ldt_amd import mix_dtype

    r = np.zeros(n, mix_dtype())
    r["partner"] = (np.arange(n) - 1) % n if partner is None else partner
    r["w_self"], r["w_partner"] = (1.0, 0.0) if cut else (np.float32(lam), np.float32(1.0 - lam))
    r["lw_self"], r["lw_partner"] = np.float32(lam), np.float32(1.0 - lam)
    r["box"] = box
    return r


def _decode(cells, size, mix, dtype="float32", mf="contiguous", labels=LABELS, ctx=None, **opts):
    """One call into the middle of a sentinel buffer. Returns (image CPU [n, 3, h, w], label CPU or None,
    int64 labels, failed rows)."""
    import torch

    import ldt_amd
    from ldt_amd import transforms as T

    n = len(cells)
    labels = None if labels is None else labels[:n]
    nbytes = n * 3 * size[0] * size[1] * C.ES[dtype]
    buf = torch.full((C.GUARD + nbytes + C.GUARD,), C.SENTINEL, dtype=torch.uint8, device="cuda")
    flat = buf[C.GUARD:C.GUARD + nbytes].view(C._td(dtype))
    cl = mf == "channels_last"
    out = flat.view(n, size[0], size[1], 3).permute(0, 3, 1, 2) if cl else flat.view(n, 3, *size)
    lbl = torch.full((n,), -777, dtype=torch.int64, device="cuda")
    nc = 0 if mix is None or labels is None else (mix.num_classes if hasattr(mix, "sample") else mix[1])
    soft = torch.full((n + 2, max(nc, 1)), -7.0, device="cuda")
    spec = T.CallSpec.make(opts.pop("normalize", None), size, opts.pop("interpolation", None), C._td(dtype),
                           torch.channels_last if cl else None, None, opts.pop("crops", _crops(n, size)), None,
                           opts.pop("colors", None), opts.pop("augments", None), mix)
    assert not opts
    failed = {}
    try:
        T._decode_cells(spec, pa.array([d for _, d in cells], pa.binary()), labels, None, None, ctx, out,
                        lbl if labels is not None else None, soft[1:n + 1] if nc else None)
    except ldt_amd.ImageDecodeError as e:
        failed = dict(e.rows)
    torch.cuda.synchronize()
    assert torch.all(buf[:C.GUARD] == C.SENTINEL).item(), "wrote before the output"
    assert torch.all(buf[C.GUARD + nbytes:] == C.SENTINEL).item(), "wrote past the output"
    assert torch.all(soft[0] == -7.0).item() and torch.all(soft[n + 1] == -7.0).item()
    host = flat.cpu()
    img = host.view(n, size[0], size[1], 3).permute(0, 3, 1, 2) if cl else host.view(n, 3, *size)
    return img, (soft[1:n + 1].cpu() if nc else None), lbl.cpu().numpy(), failed


def _bits(t):
    import torch

    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _want(ref, rows, dtype, failed=()):
    """torchvision's ops per row on the float32 reference [n, 3, h, w], then .to(dtype)."""
    import torch

    out = torch.zeros_like(ref)
    for i, m in enumerate(rows):
        p = int(m["partner"])
        if i in failed:
            continue
        if p in failed:
            out[i] = ref[i]
            continue
        out[i] = ref[p].clone().mul_(float(m["w_partner"])).add_(ref[i].mul(float(m["w_self"])))
        t, l, h, w = (int(v) for v in m["box"])
        if h:
            out[i][:, t:t + h, l:l + w] = ref[p][:, t:t + h, l:l + w]
    return out.to(C._td(dtype))


def _want_soft(labels, rows, failed=()):
    import torch

    hot = torch.nn.functional.one_hot(torch.from_numpy(labels), NC).float()
    out = torch.zeros_like(hot)
    for i, m in enumerate(rows):
        p = int(m["partner"])
        if i in failed:
            continue
        out[i] = hot[i] if p in failed else \
            hot[p].clone().mul_(float(m["lw_partner"])).add_(hot[i].mul(float(m["lw_self"])))
    return out


def _run(cells, size, rows, what, dtype="float32", mf="contiguous", **opts):
    """The call with the mix against the reference call without it."""
    import torch

    n = len(cells)
    ref, none, lbl0, failed0 = _decode(cells, size, None, **dict(opts))
    assert none is None and not failed0 and ref.dtype == torch.float32
    img, soft, lbl, failed = _decode(cells, size, (rows, NC), dtype, mf, **dict(opts))
    assert not failed, what
    assert torch.equal(_bits(img), _bits(_want(ref, rows, dtype))), what
    assert torch.equal(_bits(soft), _bits(_want_soft(LABELS[:n], rows))), what
    assert np.array_equal(lbl, LABELS[:n]) and np.array_equal(lbl0, LABELS[:n]), what  # the int64 labels as before


BOXES = {"none": lambda h, w: (0, 0, 0, 0), "whole": lambda h, w: (0, 0, h, w), "tl": lambda h, w: (0, 0, 1, 1),
         "tr": lambda h, w: (0, w - 1, 1, 1), "bl": lambda h, w: (h - 1, 0, 1, 1),
         "br": lambda h, w: (h - 1, w - 1, 1, 1)}


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (17, 33), (30, 33)])
def test_sizes_and_boxes(cells, size):
    """No whole quad (3 x 5), a second row tile and a quad tail (17 x 33); every box at every size, MixUp's
    weights outside it, and a box crossing rows 15 / 16 and a quad boundary where the size has them."""
    n = len(cells)
    for name, box in BOXES.items():
        _run(cells, size, _rows(n, box=box(*size)), f"{size} {name}")
        _run(cells, size, _rows(n, box=box(*size), cut=True), f"{size} {name} cutmix")
    if size[0] > 16:
        _run(cells, size, _rows(n, box=(14, 2, 3, 5), cut=True), f"{size} crossing")
        per_row = _rows(n, cut=True)
        per_row["box"] = [(14, 2, 3, 5), (0, 0, 0, 0), (15, 3, 1, 2), (16, 4, 1, 29), (0, 31, 17, 2)]
        per_row["partner"] = [4, 0, 0, 2, 4]  # timm's flip and a row that is its own partner
        _run(cells, size, per_row, f"{size} per-row boxes and partners")


@pytest.mark.parametrize("n", [1, 2, 5])
def test_batch_sizes(cells, n):
    """n = 1 is its own partner (no shortcut: 2 * lam-weighted sums, not x itself)."""
    for lam in (0.0, 1.0, 0.5, LAM):
        _run(cells[:n], (17, 33), _rows(n, lam), f"n={n} lam={lam}")


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("mf", ["contiguous", "channels_last"])
@pytest.mark.parametrize("normalize", [None, True])
def test_dtypes_layouts_and_normalize(cells, dtype, mf, normalize):
    n = len(cells)
    _run(cells, (17, 33), _rows(n, box=(14, 2, 3, 5)), f"{dtype} {mf} {normalize}", dtype, mf, normalize=normalize)
    _run(cells, (3, 5), _rows(n, 0.7), f"{dtype} {mf} {normalize} small", dtype, mf, normalize=normalize)


def _aug_rows(n, K):
    rows = np.full((n, max(K, 1), 10), NAN, np.float64)
    if K >= 1:
        rows[:, 0] = [4.0, 1.5] + [NAN] * 5 + [0.0] * 3  # contrast: the statistics pass
        rows[1, 0] = [5.0, 1.7] + [NAN] * 5 + [0.0] * 3  # sharpness reads its neighbours
    if K >= 2:
        rows[::2, 1] = [1.0, 1.0, 0.0, 2.0, 0.0, 1.0, -1.0, 9.0, 8.0, 7.0]  # a translation; odd rows keep one op
    return rows


@pytest.mark.parametrize("K", [0, 1, 2])
@pytest.mark.parametrize("dtype,normalize", [("float32", True), ("bfloat16", None)])
def test_augments_and_erase_boxes_under_the_mix(cells, K, dtype, normalize):
    """The erase box is the value 0, not the byte 0 (Normalize shows it), in the row and in its partner, and
    it overlaps the mix box. Rows with one op and rows with two end in different workspaces."""
    from ldt_amd import _lib

    n, size = len(cells), (17, 33)
    erase = np.array([[13, 1, 4, 8], [0, 0, 0, 0], [15, 4, 2, 3], [0, 0, 17, 33], [16, 30, 1, 3]])
    aug = _lib.check_augments(_aug_rows(n, K) if K else None, n, None, size, erase)
    assert int(aug["count"].max()) == K and (K < 2 or int(aug["count"].min()) == 1)
    _run(cells, size, _rows(n, box=(14, 2, 3, 5)), f"K={K} mixup", dtype, normalize=normalize, augments=aug)
    _run(cells, size, _rows(n, box=(14, 2, 3, 5), cut=True), f"K={K} cutmix", dtype, "channels_last",
         normalize=normalize, augments=aug)


@pytest.mark.parametrize("blur", [False, True])
def test_colours_under_the_mix(cells, blur):
    n, size = len(cells), (30, 33)
    rows = np.array([[1.2, 1.5, 0.4, 0.07, C.ORDER0123, i & 1, 128 if i == 2 else -1] for i in range(n)], np.float64)
    if blur:
        rows = np.concatenate([rows, np.array([[1.0], [NAN], [0.5], [NAN], [2.0]])], axis=1)
    _run(cells, size, _rows(n, box=(14, 2, 3, 5)), f"colours blur={blur}", "float16", normalize=True, colors=rows)


def test_bicubic(cells):
    _run(cells, (17, 33), _rows(len(cells), box=(14, 2, 3, 5)), "bicubic", "bfloat16", "channels_last",
         interpolation="bicubic")


def _tv_lam(alpha, g):
    import torch

    return float(torch._sample_dirichlet(torch.tensor([[alpha, alpha]]), generator=g)[..., 0])


@pytest.mark.parametrize("which", ["mixup", "cutmix", "choice"])
def test_seeded_samplers_are_torchvisions_batch_ops(cells, which):
    """The sampler's records through the kernel against the batch ops torchvision runs: roll(1, 0), mul_, add_
    with the same seeded draws, transliterated."""
    import math

    import torch

    import ldt_amd

    n, size = len(cells), (30, 33)
    H, W = size
    for seed in (1, 2, 3):
        g = torch.Generator().manual_seed(seed)
        mk = {"mixup": lambda: ldt_amd.MixUp(0.2, num_classes=NC, generator=g),
              "cutmix": lambda: ldt_amd.CutMix(1.0, num_classes=NC, generator=g),
              "choice": lambda: ldt_amd.MixChoice([ldt_amd.MixUp(0.2, num_classes=NC),
                                                   ldt_amd.CutMix(1.0, num_classes=NC)], generator=g)}[which]
        ref, _, _, _ = _decode(cells, size, None, normalize=True)
        img, soft, _, failed = _decode(cells, size, mk(), "bfloat16", normalize=True)
        assert not failed
        t = torch.Generator().manual_seed(seed)
        kind = which
        if which == "choice":
            kind = ("mixup", "cutmix")[int(torch.multinomial(torch.tensor([0.5, 0.5]), 1, generator=t))]
        hot = torch.nn.functional.one_hot(torch.from_numpy(LABELS), NC).float()
        if kind == "mixup":
            lam = _tv_lam(0.2, t)
            want = ref.roll(1, 0).mul_(1.0 - lam).add_(ref.mul(lam))
        else:
            lam = _tv_lam(1.0, t)
            r_x, r_y = int(torch.randint(W, (1,), generator=t)), int(torch.randint(H, (1,), generator=t))
            r = 0.5 * math.sqrt(1.0 - lam)
            x1, y1 = max(r_x - int(r * W), 0), max(r_y - int(r * H), 0)
            x2, y2 = min(r_x + int(r * W), W), min(r_y + int(r * H), H)
            want = ref.clone()
            want[..., y1:y2, x1:x2] = ref.roll(1, 0)[..., y1:y2, x1:x2]
            lam = float(1.0 - (x2 - x1) * (y2 - y1) / (W * H))
        want_soft = hot.roll(1, 0).mul_(1.0 - lam).add_(hot.mul(lam))
        assert torch.equal(_bits(img), _bits(want.to(torch.bfloat16))), (which, seed)
        assert torch.equal(_bits(soft), _bits(want_soft)), (which, seed)


def test_a_corrupt_cell_as_a_row_and_as_a_partner(cells):
    import torch

    mixed = [cells[0], ("bad", read_golden("jpeg/bad_not_jpeg.bin")), cells[1], cells[3], cells[4]]
    n, size = len(mixed), (17, 33)
    rows = _rows(n, box=(14, 2, 3, 5))  # row 2's partner is the corrupt row 1
    ref, _, _, failed0 = _decode(mixed, size, None, normalize=True)
    img, soft, lbl, failed = _decode(mixed, size, (rows, NC), "float16", "channels_last", normalize=True)
    assert set(failed) == {1} == set(failed0) and failed[1] != 0
    assert torch.equal(_bits(img), _bits(_want(ref, rows, "float16", failed={1})))
    assert not _bits(img[1]).any() and torch.equal(_bits(img[2]), _bits(ref[2].to(torch.float16)))
    want_soft = _want_soft(LABELS, rows, failed={1})
    assert torch.equal(_bits(soft), _bits(want_soft))
    assert not _bits(soft[1]).any() and soft[2].tolist() == [1.0 if c == LABELS[2] else 0.0 for c in range(NC)]
    assert lbl.tolist() == [3, -100, 7, 0, 10]


def test_images_only_without_labels_or_classes(cells):
    import torch

    n, size = len(cells), (17, 33)
    rows = _rows(n, box=(14, 2, 3, 5))
    ref, _, _, _ = _decode(cells, size, None)
    for mix, labels in (((rows, NC), None), ((rows, 0), LABELS)):
        img, soft, lbl, failed = _decode(cells, size, mix, labels=labels)
        assert soft is None and not failed
        assert torch.equal(_bits(img), _bits(_want(ref, rows, "float32")))
        assert labels is None or np.array_equal(lbl, LABELS)


def test_a_plain_call_after_a_mixed_one_and_the_public_surfaces(cells):
    import torch

    import ldt_amd

    n, size = len(cells), (17, 33)
    before, _, _, _ = _decode(cells, size, None, "bfloat16", normalize=True)
    _run(cells, size, _rows(n, box=(14, 2, 3, 5)), "between", "bfloat16", normalize=True)
    after, _, _, _ = _decode(cells, size, None, "bfloat16", normalize=True)
    assert torch.equal(_bits(before), _bits(after))
    # decode_tensor_image and collate_fn: the label is the soft tensor, a DeviceTensor in the dict
    rb = pa.RecordBatch.from_arrays([pa.array([d for _, d in cells], pa.binary()), pa.array(LABELS)],
                                    ["image", "label"])
    rows = _rows(n, box=(14, 2, 3, 5))
    ref = ldt_amd.decode_tensor_image(rb, size=size, crop=_crops(n, size))["image"].cpu()
    got = ldt_amd.decode_tensor_image(rb, size=size, crop=_crops(n, size), mix=(rows, NC))
    assert type(got["label"]).__name__ == "DeviceTensor" and got["label"].dtype == torch.float32
    assert torch.equal(_bits(got["image"].cpu()), _bits(_want(ref, rows, "float32")))
    assert torch.equal(_bits(got["label"].cpu()), _bits(_want_soft(LABELS, rows)))
    items = [{"image": d, "label": int(l)} for (_, d), l in zip(cells, LABELS)]
    col = ldt_amd.collate_fn(items, size=size, crop=_crops(n, size), mix=(rows, NC))
    assert torch.equal(_bits(col["image"].cpu()), _bits(got["image"].cpu()))
    assert torch.equal(_bits(col["label"].cpu()), _bits(got["label"].cpu()))
    with pytest.raises(ValueError, match="outside 0..6"):
        ldt_amd.decode_tensor_image(rb, size=size, crop=_crops(n, size), mix=(rows, 7))


def test_pipeline_of_depth_three_equals_the_synchronous_calls(cells):
    import torch

    import ldt_amd

    size = (17, 33)
    order = [[0, 1, 2, 3, 4], [4, 3, 2], [1, 0, 3, 4], [2, 2, 0, 1, 4]]
    pipe = ldt_amd.DecodePipeline(depth=3, size=size, dtype=torch.bfloat16, memory_format=torch.channels_last)
    outs = []
    for k, idx in enumerate(order):
        n = len(idx)
        rb = pa.RecordBatch.from_arrays([pa.array([cells[i][1] for i in idx], pa.binary()), pa.array(LABELS[idx])],
                                        ["image", "label"])
        rows = _rows(n, 0.1 + 0.2 * k, box=(14, 2 + k, 3, 5))
        img, lbl = pipe.decode(rb, normalize=True, crops=_crops(n, size), mixes=(rows, NC))
        outs.append((img, lbl))
    pipe.check()
    torch.cuda.synchronize()
    for k, (idx, (img, lbl)) in enumerate(zip(order, outs)):
        n = len(idx)
        rows = _rows(n, 0.1 + 0.2 * k, box=(14, 2 + k, 3, 5))
        sub = [cells[i] for i in idx]
        want, soft, _, _ = _decode(sub, size, (rows, NC), "bfloat16", "channels_last", labels=LABELS[idx],
                                   normalize=True)
        assert lbl.dtype == torch.float32 and tuple(lbl.shape) == (n, NC)
        assert torch.equal(_bits(img.cpu()), _bits(want)), k
        assert torch.equal(_bits(lbl.cpu()), _bits(soft)), k
