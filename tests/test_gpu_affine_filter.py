"""GPU tests of the filtered affine op (ldt_set_affine_filters, ``affine_filter=``):
Pillow's ``Image.transform(size, AFFINE, m, BILINEAR | BICUBIC, fillcolor)`` in
an op slot of an augment entry, bit for bit. The expected value is built as
tests/test_gpu_augment.py builds it (the oracle's resized bytes, Pillow's own
ops in the entry's order, the table, the erase box); rows here hold the filter
as an eleventh number.
"""
import numpy as np
import pytest

import test_gpu_augment as G
import test_gpu_color as C
from conftest import read_golden
from test_affine_filter_ops import MATRICES, matrix

pytestmark = pytest.mark.gpu

NAN = float("nan")
ABSENT = [NAN] * 11
FILL = (12, 200, 99)


@pytest.fixture(scope="module")
def cells():
    return [(name, read_golden("jpeg/" + name)) for name in C.NAMES]


def _filt(filt, m, fill=FILL):
    return [1.0] + [float(x) for x in m] + [float(x) for x in fill] + [float(filt)]


def _plain(row):
    return list(row) + [NAN]


def _pil(u8, row):
    from PIL import Image

    if not row[10] > 0:  # NaN or 0: the existing ops
        return G._pil_rows(u8, [row[:10]])
    im = Image.fromarray(u8, "RGB")
    resample = {1: Image.BILINEAR, 2: Image.BICUBIC}[int(row[10])]
    im = im.transform(im.size, Image.AFFINE, [float(x) for x in row[1:7]], resample,
                      fillcolor=tuple(int(x) for x in row[7:10]))
    return np.asarray(im, dtype=np.uint8)


def _check(cells, size, aug, res, lbl, failed, what, erase=None, views=None, crops=None, dtype="float32",
           normalize=None, bad=()):
    import torch

    n, V = len(cells), views or 1
    aug = np.asarray(aug, np.float64).reshape(n, V, -1, 11)
    erase = None if erase is None else np.asarray(erase).reshape(n, V, 4)
    assert sorted(failed) == sorted(bad), (what, failed)
    for i, (name, data) in enumerate(cells):
        for v in range(V):
            got = res[v][i]
            if i in bad:
                assert int(lbl[i]) == -100 and not got.contiguous().view(torch.uint8).any().item(), (what, i)
                continue
            crop = None if crops is None else (np.asarray(crops)[i, v] if views else np.asarray(crops)[i])
            u8 = C._resized_u8(name, data, tuple(size), crop)
            for row in aug[i, v]:
                u8 = _pil(u8, row)
            want = G._expected(u8, None, None if erase is None else erase[i, v], dtype, C._norm_arg(normalize))
            C._same(got, want, f"{what}: {name} view {v}")


@pytest.mark.parametrize("size", [(1, 1), (7, 5), (33, 65)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("filt", [1, 2], ids=["bilinear", "bicubic"])
def test_matrices(cells, filt, size):
    """One view per matrix. 33 x 65 crosses a 16 x 64 tile edge on both axes and leaves a partial tile."""
    use, V = cells[:2], len(MATRICES)
    aug = np.array([[[_filt(filt, matrix(name, *size))] for name in MATRICES]] * len(use))
    crops = np.repeat(G._small_crops(use, size)[:, None, :], V, axis=1)
    res, lbl, failed = G._decode(use, size, aug, views=V, crops=crops)
    _check(use, size, aug, res, lbl, failed, f"matrices {size}", views=V, crops=crops)


def test_box_beyond_lds_reads_the_workspace(cells):
    """Scale 3 on 64 x 200: the first tile's source box is wider than the LDS takes."""
    from ldt_amd import _lib

    size, (th, tw) = (64, 200), _lib.AFFINE_TILE
    assert min(3 * tw - 2, size[1]) * min(3 * th - 2, size[0]) > _lib.AFFINE_LDS_TEXELS
    use = cells[:1]
    aug = np.array([[[_filt(1, matrix("scale3", *size))], [_filt(2, matrix("scale3", *size))]]])
    res, lbl, failed = G._decode(use, size, aug, views=2)
    _check(use, size, aug, res, lbl, failed, "fallback", views=2)


def test_mixed_slots(cells):
    """Filtered ops in the first and in the last of two slots, beside a NEAREST entry and one with no op."""
    use, hw = cells[:4], (40, 70)
    aug = np.array([[_filt(1, matrix("rot30", *hw)), _plain(G._row(9))],
                    [_plain(G._row(4, 1.6)), _filt(2, matrix("shearx", *hw))],
                    [ABSENT, _plain(G._affine("Rotate", -20.0, hw, (7, 7, 7)))],
                    [ABSENT, ABSENT]])
    res, lbl, failed = G._decode(use, hw, aug)
    _check(use, hw, aug, res, lbl, failed, "mixed slots")


def test_bf16_channels_last_normalize_erase(cells):
    hw, n = (33, 65), len(cells)
    aug = np.array([[_filt(1 + (i & 1), matrix(("rot45", "shearx", "half")[i % 3], *hw))] for i in range(n)])
    erase = np.array([[5, 7, 20, 50]] * n)
    res, lbl, failed = G._decode(cells, hw, aug, erase=erase, dtype="bfloat16", mf="channels_last", normalize=True)
    _check(cells, hw, aug, res, lbl, failed, "bf16 nhwc", erase=erase, dtype="bfloat16", normalize=True)


def test_failed_row_between_good_ones(cells):
    mixed = [cells[0], ("bad", read_golden("jpeg/bad_not_jpeg.bin")), cells[1]]
    hw = (36, 70)
    aug = np.array([[_filt(2, matrix("rot30", *hw))]] * 3)
    res, lbl, failed = G._decode(mixed, hw, aug)
    assert failed == {1: 1}
    _check(mixed, hw, aug, res, lbl, failed, "failed row", bad=(1,))


def test_trivial_augment_wide_bilinear(cells):
    """The sampler's records through the decode, and the same seed's rows through Pillow."""
    import torch

    from ldt_amd import TrivialAugmentWide

    n, size = len(cells), (48, 70)
    ta = TrivialAugmentWide(fill=FILL, affine_filter="bilinear", generator=torch.Generator().manual_seed(5))
    records = ta.sample(n, size)
    ta.generator.manual_seed(5)
    rows = np.array([ta._draw(*size) for _ in range(n)])
    assert (rows[..., 10] == 1).any() and "filt" in records.dtype.names
    res, lbl, failed = G._decode(cells, size, records)
    _check(cells, size, rows, res, lbl, failed, "TrivialAugmentWide")


def test_two_views(cells):
    use, hw = cells[:2], (48, 40)
    aug = np.array([[[_filt(1, matrix("rot45", *hw)), _plain(G._row(10))],
                     [_plain(G._row(9)), _filt(2, matrix("scale1/3", *hw))]],
                    [[_filt(2, matrix("half", *hw)), ABSENT], [ABSENT, ABSENT]]])
    res, lbl, failed = G._decode(use, hw, aug, views=2)
    _check(use, hw, aug, res, lbl, failed, "views=2", views=2)


def test_setter_refusals_leave_nothing_pending(cells):
    import ldt_amd
    from ldt_amd import _lib

    use, hw = cells[:2], (20, 30)
    good = _lib.check_augments(np.array([[_filt(1, matrix("rot30", *hw)), _plain(G._row(9))]] * 2), 2, None, hw)
    ctx = _lib.Context(0)
    filt = np.ascontiguousarray(good["filt"])
    assert ctx.lib.ldt_set_affine_filters(ctx.handle, filt.ctypes.data, 2) == -1  # no augments pending

    def nan(r):
        r["filt"]["m"][1, 0, 3] = np.nan

    def filter3(r):
        r["filt"]["filter"][0, 0] = 3

    def on_equalize(r):
        r["filt"]["filter"][0, 1] = 1

    def beyond_count(r):
        r["filt"]["filter"][1, 2] = 2

    def fewer(r):
        ctx.use_augments(good[:1])  # one entry pending: the two entries' filters do not match it
        assert ctx.lib.ldt_set_affine_filters(ctx.handle, filt.ctypes.data, 2) == -1
        r["filt"]["m"][0, 0, 0] = np.inf

    for edit in (nan, filter3, on_equalize, beyond_count, fewer):
        bad = good.copy()
        edit(bad)
        with pytest.raises(ldt_amd.LdtError, match="rc=-1"):
            ctx.use_augments(bad)
        res, lbl, failed = G._decode(use, hw, None, ctx=ctx)  # neither filters nor augments stayed
        G._check(use, hw, None, res, lbl, failed, f"after {edit.__name__}")
