"""GPU decode of the sync cells (tests/jpeg_recode.py sync_cells) with
LDT_OPT_SUBSEQ_BITS = 64, so that the planner cuts every scan into ranges of
S = 96 bits: flat files re-coded so that no guessed start of k_huff_image ever
meets the true trajectory (the truth moves one slot per round: about a
thousand rounds for the largest, next to the kernel's bound of kHuffThreads
+ 1 iterations), their even-parity twin that needs no re-decode, textured
files that converge over dozens of rounds through the memo and work lists
longer than a wave, and restart-segment geometries (segments of exactly k*S
bits, of k*S + 8, shorter than S/3, 256 and 257 segments).

The bar is the project's: bit-exact against oracle.jpeg_to_tensor (max abs
<= 2/255 first), under the defaults, the serial decoder, global reads with
both destuff paths and LDT_OPT_SYNC_WARM 0 / 50 / 200. Every decode whose
subject is phase 1, the rounds or the warm-up runs from a cleared sync cache
and then again on its entries (tests/huff_paths.py cold_then_warm); the
configurations that never consult the table run through uncached. The kernel's own
counters (LDT_OPT_DEBUG_COUNTERS) are held against the symbol-level model of
tests/huffman_sync_model.py; tests/test_huffman_sync.py asserts on the CPU
that each cell has the property it is named for and the plan it needs.
"""
import contextlib

import pytest

import huff_paths as hp
import huffman_sync_model as hm
import jpeg_recode as jr
from conftest import read_golden
from oracle import oracle
from test_gpu_parity import _batch, _check

pytestmark = pytest.mark.gpu

S = jr.SYNC_S

# every option the tests touch, with its default
DEFAULTS = {"OPT_HUFF_MODE": 0, "OPT_SUBSEQ_BITS": 256, "OPT_HUFF_WINDOW": -1, "OPT_FUSED_DESTUFF": 1,
            "OPT_SYNC_WARM": 0, "OPT_DEBUG_COUNTERS": 0}

# the configurations whose images consult the sync cache (the LDS window with the fused destuff)
CACHED = ("defaults", "warm50", "warm200")

CONFIGS = {
    "defaults": {},
    "serial": {"OPT_HUFF_MODE": 1},
    "global-unfused": {"OPT_HUFF_WINDOW": 0, "OPT_FUSED_DESTUFF": 0},
    "global-fused": {"OPT_HUFF_WINDOW": 0, "OPT_FUSED_DESTUFF": 1},
    "warm50": {"OPT_SYNC_WARM": 50},
    "warm200": {"OPT_SYNC_WARM": 200},
}


@contextlib.contextmanager
def _options(**opts):
    """The context's options set for the block, every one restored after it."""
    import torch

    from ldt_amd import _lib

    assert set(opts) <= set(DEFAULTS)
    ctx = _lib.get_context(torch.cuda.current_device())
    try:
        for k, v in opts.items():
            ctx.set_option(getattr(_lib, k), v)
        yield ctx
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(getattr(_lib, k), v)


@pytest.fixture(scope="module")
def sync():
    """The cells, each one's expected tensor and the model's figures, computed once."""
    cells = jr.sync_cells()
    exp = {c.name: oracle.jpeg_to_tensor(c.data) for c in cells}
    models = {c.name: hm.model(c.data, S) for c in cells if c.sub_bits}
    return cells, exp, models


def _decode(cells, **kw):
    import ldt_amd

    return ldt_amd.decode_tensor_image(_batch([c.data for c in cells]), **kw)["image"].cpu().numpy()


def _tagged(cells, tag):
    out = [c for c in cells if tag in c.tags]
    assert out, tag
    return out


def _counters(cell, exp, **opts):
    """The decoder's counters of `cell` decoded alone (and checked)."""
    with _options(OPT_SUBSEQ_BITS=64, OPT_DEBUG_COUNTERS=1, **opts) as ctx:
        out = _decode([cell])
        cnt = ctx.debug_counters()
    _check(out[0], exp[cell.name], f"counters: {cell.name}")
    assert cnt[1] == 1, (cell.name, cnt)  # one image through k_huff_image
    print(f"{cell.name}: rounds {cnt[3]} adoptions {cnt[4]} needy {cnt[13]} waves {cnt[14]}")
    return cnt


@pytest.mark.parametrize("config", list(CONFIGS))
def test_each_cell_alone_and_all_in_one_batch(config, sync):
    """Both decoders, the LDS window and global reads, both destuff paths and
    every warm-up give the oracle's tensors, so the same ones. Under the
    defaults and the warm-ups every cell alone and the batch run cold (phase
    1, the warm-up and the rounds) and then hinted; the 257-segment cell is
    the serial decoder's and never consults the table."""
    cells, exp, _ = sync
    users = sum(1 for c in cells if c.sub_bits != 0)
    assert users == len(cells) - 1
    with _options(OPT_SUBSEQ_BITS=64, **CONFIGS[config]) as ctx:
        if config in CACHED:
            alone = [hp.cold_then_warm(ctx, lambda: _decode([c]), users=int(c.sub_bits != 0),
                                       what=f"{config}, alone: {c.name}") for c in cells]
            batch = hp.cold_then_warm(ctx, lambda: _decode(cells), users=users, what=f"{config}, batch")
            for run in list(alone) + [batch]:  # every cell decodes, so every user is kept and hits
                assert run[0].d["inserts"] == run[0].d["misses"] == run[1].d["hits"], run
        else:
            alone = [(hp.uncached(ctx, lambda: _decode([c]), what=f"{config}, alone: {c.name}"),) for c in cells]
            batch = (hp.uncached(ctx, lambda: _decode(cells), what=f"{config}, batch"),)
    for k, c in enumerate(cells):
        for run, path in zip(alone[k], ("cold", "warm")):
            _check(run.out[0], exp[c.name], f"{config}, alone, {path}: {c.name}")
        for run, path in zip(batch, ("cold", "warm")):
            _check(run.out[k], exp[c.name], f"{config}, batch, {path}: {c.name}")


@pytest.fixture(scope="module")
def mode_cells(manifest):
    """The cells of test_gpu_parity.test_huffman_decoder_modes and their expected tensors."""
    from ldt_amd import synth

    cells = [read_golden(e["file"]) for e in manifest["images"]]
    cells += synth.q90_512(6, seed=5)[0] + synth.imagenet_like(6, seed=5)[0]
    return cells, [oracle.jpeg_to_tensor(b) for b in cells]


@pytest.mark.parametrize("bits", [64, 256])
@pytest.mark.parametrize("warm", [50, 200])
def test_sync_warm_on_the_decoder_mode_cells(warm, bits, mode_cells):
    """LDT_OPT_SYNC_WARM on natural images: phase 1 starts 50 % / 200 % of S
    before each range, entries are then symbol boundaries past the range
    start. From a cleared sync cache, so the warm-up runs in all four cases,
    then on the entries it made."""
    import ldt_amd

    cells, exp = mode_cells
    users = sum(hp.cache_users(cells, bits=bits))
    assert users >= 12  # the twelve config-shaped cells at the least
    with _options(OPT_SUBSEQ_BITS=bits, OPT_SYNC_WARM=warm) as ctx:
        runs = hp.cold_then_warm(ctx, lambda: ldt_amd.decode_tensor_image(_batch(cells))["image"].cpu().numpy(),
                                 users=users, what=f"warm{warm}/S{bits}")
        assert runs[0].d["inserts"] == runs[1].d["hits"] == users, runs
        for run, path in zip(runs, ("cold", "warm")):
            for k in range(len(cells)):
                _check(run.out[k], exp[k], f"warm{warm}/S{bits}, {path}[{k}]")
        # the truncated cell fails on both calls and is never kept
        bad = hp.cold_then_warm(ctx, lambda: ldt_amd.decode_tensor_image(
            _batch([cells[0], read_golden("jpeg/bad_truncated.bin")])), what=f"warm{warm}/S{bits}, truncated")
        assert bad[0].rows == bad[1].rows == {1: 3}


def test_locked_cells_take_one_round_per_slot(sync):
    """The kernel's round counter against the model, which is exact on these
    cells (every step is one symbol): within 2 (the last range's padding bits
    may cost or save a round). Every slot but a segment's first is needy at
    least once (slots - 1 for one segment), and no memo is ever adopted."""
    cells, exp, models = sync
    for c in _tagged(cells, "locked"):
        m = models[c.name]
        cnt = _counters(c, exp)
        assert abs(cnt[3] - m.rounds) <= 2, (c.name, cnt[3], m.rounds)
        assert cnt[2] == cnt[3]
        assert cnt[13] >= m.slots - c.nseg, (c.name, cnt[13], m.slots)
        assert cnt[4] == 0, (c.name, cnt[4])
    big = _tagged(cells, "slots1000")[0]
    assert models[big.name].rounds >= 1000
    # 2 S of warm-up take slots 1 and 2 back to the segment's start: two hand-overs fewer
    warm = _counters(big, exp, OPT_SYNC_WARM=200)
    assert abs(warm[3] - hm.model(big.data, S, warm_pct=200).rounds) <= 2 and warm[4] == 0, warm
    # the decoder's other instantiation (the stream read from global memory) counts the same
    c = _tagged(cells, "slots66")[0]
    glob = _counters(c, exp, OPT_HUFF_WINDOW=0, OPT_FUSED_DESTUFF=0)
    assert abs(glob[3] - models[c.name].rounds) <= 2 and glob[13] >= models[c.name].slots - 1 and glob[4] == 0, glob


def test_even_twin_takes_no_re_decode(sync):
    cells, exp, models = sync
    for c in _tagged(cells, "zero-rounds"):
        cnt = _counters(c, exp)
        assert cnt[13] == 0 and cnt[14] == 0 and cnt[4] == 0, (c.name, cnt)
        assert cnt[3] == models[c.name].rounds == 1, (c.name, cnt[3])


# The rounds of a slow cell against the model without the memo (an upper
# estimate: the memo only saves re-decodes). The model steps one symbol at a
# time; the kernel's count-mode steps take several AC symbols at once, so an
# exit may lie some symbols further and a stretch may converge a few rounds
# later than the model says. Recorded on an MI355X (profiles/huff_sync/
# counters.json): the kernel took 38 / 34 / 71 rounds on slow-std / -flat8 /
# -quarter, which is what the model with the memo says (38 / 34 / 71; without
# it 51 / 114 / 79), with needy slots within 12 of the model's ~6000. The
# recorded difference is 0; the margin is the 2 rounds the locked cells are
# allowed for their last range's padding bits.
SLOW_ROUNDS_MARGIN = 2


def test_slow_cells_use_the_memo_and_more_than_one_wave(sync):
    """Memo adoptions happen, some round's work list spans waves (more waves
    than rounds), and the rounds stay within the model's without the memo.
    No equality with the model: count-mode steps shift individual exits."""
    cells, exp, models = sync
    for c in _tagged(cells, "slow"):
        cnt = _counters(c, exp)
        assert cnt[4] > 0, (c.name, cnt)
        assert cnt[14] > cnt[2], (c.name, cnt[14], cnt[2])
        bound = hm.model(c.data, S, memo=False).rounds + SLOW_ROUNDS_MARGIN
        assert cnt[3] <= bound, (c.name, cnt[3], bound)


def test_geometry_cells_converge_within_their_segments(sync):
    """A segment's chain starts afresh and the truth moves at least one slot
    per round, so no cell takes more rounds than its longest segment has slots
    (one per hand-over after slot 0, and the round that finds nothing to do)."""
    cells, exp, models = sync
    for c in cells:
        if c.sub_bits and any(t.startswith(("seg-", "nseg")) for t in c.tags):
            cnt = _counters(c, exp)
            assert 1 <= cnt[3] <= max(s.slots for s in models[c.name].segments), (c.name, cnt[3])


def test_locked_cell_between_neighbours_and_truncated(sync):
    """A locked cell between two ordinary cells; then the 1000-slot cell cut
    in the middle of its scan between two good cells: status 3 on its row
    only, and the next clean batch is bit-exact. The table is cleared before
    the failing call, so that call and the clean batch after it both run phase
    1 and the rounds; the clean batch then runs again on its entries."""
    cells, exp, _ = sync
    by_name = {c.name: c for c in cells}
    with _options(OPT_SUBSEQ_BITS=64) as ctx:
        mix = [by_name["slow-std"], by_name["locked-1000"], by_name["geometry-420"]]
        for run, path in zip(hp.cold_then_warm(ctx, lambda: _decode(mix), users=3, what="neighbours"),
                             ("cold", "warm")):
            for k, c in enumerate(mix):
                _check(run.out[k], exp[c.name], f"neighbours, {path}: {c.name}")
        victim = by_name["locked-1000"]
        cut = len(victim.data) - len(jr.scan_bytes(victim.data)) // 2
        bad = jr.SyncCell("locked-1000-cut", victim.data[:cut], None, frozenset(), S, 1)
        failing = [by_name["slow-quarter"], bad, by_name["locked-66"]]
        # the truncated row is status 3, never kept, and misses again on the warm call
        runs = hp.cold_then_warm(ctx, lambda: _decode(failing), users=3, what="truncated cell")
        assert runs[0].rows == runs[1].rows == {1: 3}
        assert runs[0].d["inserts"] == 2 and runs[1].d["hits"] == 2 and runs[1].d["misses"] == 1, runs
        # none of the clean batch's cells was in the failing call: it runs cold on the table as that call left it
        nxt = [by_name["locked-rst"], by_name["slow-flat8"], by_name["locked-1000"], by_name["even-twin"]]
        for run, path in zip(hp.cold_then_warm(ctx, lambda: _decode(nxt), users=4, clear=False,
                                               what="after the truncated cell"), ("cold", "warm")):
            assert run.rows == {}
            for k, c in enumerate(nxt):
                _check(run.out[k], exp[c.name], f"after the truncated cell, {path}: {c.name}")
