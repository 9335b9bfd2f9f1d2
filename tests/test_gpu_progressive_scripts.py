"""GPU decode of the script cells (tests/jpeg_progressive.py script_cells):
progressive files under scan scripts Pillow never writes. They reach what
Pillow's one script leaves idle in ldt_prog.hip: AC chains of 5, 6 and 60 scans
(a wave takes a second scan and waits on a scan another wave still runs),
per-component DC scans (their own unit grid, MCU-padding blocks no scan
covers, the 32-bit read of the DC refinement), ladders from Al = 3 and
refinements of sub-bands, bands of one coefficient, more than 32 correction
bits before a stop and behind an EOB run, EOB runs of category 14, a restart
interval of its own for every scan, 16-bit codes and the code 0xFFFE in the
register table lookup, a DQT between scans, 64 scans, seven MCU layouts.

The bar is the project's: bit-exact against Pillow itself
(oracle.pil_image_to_tensor) and against oracle.jpeg_to_tensor, max abs <=
2/255 first. tests/test_progressive_scripts.py checks on the CPU that every
cell decodes under Pillow to the pixels of its baseline twin, that the
planner reads each script back, and that the cells reach those paths.
"""
import numpy as np
import pytest

import jpeg_progressive as jp
import jpeg_recode as jr
from oracle import oracle
from test_gpu_parity import _batch, _check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scripts():
    """The accepted cells and each one's expected tensor from both references, computed once."""
    cells = list(jp.script_cells())
    exp = {c.name: (oracle.jpeg_to_tensor(c.data), oracle.pil_image_to_tensor(c.data)) for c in cells}
    for v in exp.values():
        v[0].setflags(write=False)
        v[1].setflags(write=False)
    return cells, exp


def _decode(cells, **kw):
    import ldt_amd

    return ldt_amd.decode_tensor_image(_batch([c.data for c in cells]), **kw)["image"].cpu().numpy()


def _expect(c, exp):
    if c.name not in exp:  # a batch-mate written by Pillow
        exp[c.name] = (oracle.jpeg_to_tensor(c.data), oracle.pil_image_to_tensor(c.data))
    return exp[c.name]


def _check_all(out, cells, exp, what):
    assert len(out) == len(cells)
    for k, c in enumerate(cells):
        orc, pil = _expect(c, exp)
        _check(out[k], pil, f"{what}: {c.name} vs Pillow")
        _check(out[k], orc, f"{what}: {c.name} vs the oracle")


def _small(cells):
    return [c for c in cells if "eob-max" not in c.tags]


def _mates():
    """Baseline and Pillow-script progressive files to put between the cells."""
    from ldt_amd import synth

    enc = lambda name, h, w, seed, **kw: jr.Cell(name, synth.encode(synth.field(h, w, seed, 12.0), **kw), None,
                                                 frozenset())
    return [enc("pillow-420-q75", 96, 128, 61), enc("pillow-prog-420-q90", 72, 88, 62, quality=90, progressive=True),
            enc("pillow-422-rst", 64, 96, 63, quality=90, subsampling="4:2:2", restart_marker_rows=1),
            enc("pillow-prog-444-rst", 40, 56, 64, quality=85, subsampling="4:4:4", progressive=True,
                restart_marker_blocks=3)]


def test_one_bands_cell_alone_first(scripts):
    """The narrowest run of what no GPU test had: one 9x17 4:4:0 image whose
    DC scans are per component (Cr, Y, Cb) and whose luma chain has five first
    scans, so wave 0 takes the chain's fifth scan behind wave 3."""
    cells, exp = scripts
    c = next(c for c in cells if c.name == "bands-440-9x17")
    _check_all(_decode([c]), [c], exp, "alone")


def test_each_accepted_cell_alone(scripts):
    """Every cell as a batch of one, the 1448x1456 EOB-run cell included (the only test it is in)."""
    cells, exp = scripts
    for c in cells:
        _check_all(_decode([c]), [c], exp, "alone")


def test_mixed_batch_twice_in_both_orders(scripts):
    """All the small cells with baseline files and Pillow's own progressive
    files between them, then the same batch reversed through the same
    context: every row lands on other blocks of the coefficient buffers, so a
    value pcoef or dcv kept from the first batch (a block no scan of the new
    owner covers, a coefficient it never sends) would show."""
    cells, exp = scripts
    small, mates = _small(cells), _mates()
    step = len(small) // len(mates)
    batch = []
    for k, c in enumerate(small):
        batch.append(c)
        if k % step == step - 1 and k // step < len(mates):
            batch.append(mates[k // step])
    assert len(batch) == len(small) + len(mates)
    first = _decode(batch)
    _check_all(first, batch, exp, "mixed")
    second = _decode(batch[::-1])
    _check_all(second, batch[::-1], exp, "mixed, reversed")
    assert np.array_equal(second[::-1], first)
    # cells whose per-component DC scans leave padding blocks, right after a batch that filled them
    sparse = [c for c in small if "bands" in c.tags or "latch" in c.tags]
    _check_all(_decode(sparse), sparse, exp, "per-component DC scans after a full batch")


def test_refused_cells_between_good_ones(scripts):
    """Cb's coefficient 5 left at Al = 1, a component without a DC scan and 65
    scans: status 2; Ah != Al + 1: status 3; each on its own row, the rows
    around them bit-exact, the refused rows zero with label -100."""
    import ldt_amd

    cells, exp = scripts
    by_name = {c.name: c for c in cells}
    good = [by_name[n] for n in ("deep-420-40x56", "bands-411-40x56", "sixtyfour-440-40x56", "restarts-420-72x88",
                                 "dense-444-40x56")]
    refused = jp.refused_script_cells()
    assert [c.status for c in refused] == [2, 2, 2, 3]
    batch, rows = list(good), {}
    for k, c in enumerate(refused):
        batch.insert(2 * k + 1, c)
    rows = {i: c.status for i, c in enumerate(batch) if c.status}
    assert len(rows) == 4 and len(batch) == 9
    with pytest.raises(ldt_amd.ImageDecodeError) as ei:
        _decode(batch)
    assert ei.value.rows == rows
    # the same batch into an output of the caller's: the refused rows are written as zeros
    import pyarrow as pa
    import torch

    from ldt_amd import transforms as T

    img = torch.full((len(batch), 3, 224, 224), float("nan"), device="cuda")
    lbl = torch.full((len(batch),), -777, dtype=torch.int64, device="cuda")
    with pytest.raises(ldt_amd.ImageDecodeError) as ei:
        T.decode_arrow(pa.array([c.data for c in batch], pa.binary()), np.arange(len(batch), dtype=np.int64), out=img,
                       out_lbl=lbl)
    torch.cuda.synchronize()
    assert ei.value.rows == rows
    assert lbl.cpu().tolist() == [-100 if c.status else i for i, c in enumerate(batch)]
    img = img.cpu().numpy()
    for i, c in enumerate(batch):
        if c.status:
            assert not img[i].any(), c.name
        else:
            _check_all(img[i:i + 1], [c], exp, "beside refused rows")
    _check_all(_decode(good), good, exp, "after the refused rows")


def test_pipeline_at_the_progressive_depth(scripts):
    """Two batches of script cells alternately through DecodePipeline at the
    depth the progressive benchmark uses, 4 times each: five contexts and
    streams, k_prog of one batch beside the IDCT and resize of others."""
    import torch

    import ldt_amd

    cells, exp = scripts
    small = _small(cells)
    halves = [small[0::2], small[1::2]]
    assert ldt_amd.PROGRESSIVE_DEPTH == 5
    pipe = ldt_amd.DecodePipeline(depth=ldt_amd.PROGRESSIVE_DEPTH)
    batches = [ldt_amd.ResidentBatch([c.data for c in h], list(range(len(h)))) for h in halves]
    outs = []
    for k in range(8):
        img, lbl = pipe.decode(batches[k % 2])
        outs.append((img.clone(), lbl.clone()))
    torch.cuda.synchronize()
    pipe.check()
    for k, (img, lbl) in enumerate(outs):
        assert lbl.cpu().tolist() == list(range(len(halves[k % 2])))
        _check_all(img.cpu().numpy(), halves[k % 2], exp, f"pipeline call {k}")
