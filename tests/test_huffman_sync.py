"""The sync cells of tests/jpeg_recode.py, on the CPU: streams on which the
parallel Huffman decoder (k_huff_image) converges late or, by construction,
never before the truth arrives slot by slot.

tests/huffman_sync_model.py restates the decoder's scheme at symbol
granularity; here it says, per cell, how many rounds the kernel must take,
whether the memo and a work list longer than one wave are reached, and that
the locked cells' guesses share no state with the true trajectory. The
planner (the sanitized driver of tests/test_plan_fuzz.py) must give every
cell the subsequence length, segment count and routing it is named for. The
GPU side, which holds the kernel's own counters against these figures, is
tests/test_gpu_huffman_sync.py.

If a property below fails, change the cell's input image or seed, not the
threshold.
"""
import io

import numpy as np
import pytest

import huffman_sync_model as hm
import jpeg_recode as jr
from oracle import oracle
from test_plan_fuzz import _plan_batch, build_planner

S = jr.SYNC_S
MAX_SLOTS, MAX_PAR_SEGS = 1024, 256  # ldt_types.hpp kHuffThreads, kMaxParSegs


def _pil_rgb(b: bytes) -> np.ndarray:
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))


@pytest.fixture(scope="module")
def cells():
    return jr.sync_cells()


@pytest.fixture(scope="module")
def models(cells):
    return {c.name: hm.model(c.data, S) for c in cells}


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return build_planner(tmp_path_factory)


def _tagged(cells, tag):
    out = [c for c in cells if tag in c.tags]
    assert out, tag
    return out


def test_zeros_shape():
    counts, symbols = jr.zeros(0, {0: 900, 3: 2, 5: 1})
    assert symbols == [0, 3, 5] and counts[:3] == [1, 1, 1] and sum(counts) == 3
    assert [(s, n, format(c, "0%db" % n)) for s, n, c in jr.canonical(counts, symbols)] == \
        [(0, 1, "0"), (3, 2, "10"), (5, 3, "110")]
    jr.validate_table(0, counts, symbols)
    counts, symbols = jr.zeros(1, {k: 100 - k for k in range(16)})  # 16 symbols: lengths 1..16
    jr.validate_table(1, counts, symbols)
    assert counts == [1] * 16
    with pytest.raises(ValueError):
        jr.zeros(1, {k: 1 for k in range(17)})


def test_cells_are_valid_files(cells):
    """Pillow decodes every re-coded cell to its source's pixels, with the same
    symbols; the oracle equals Pillow on every cell."""
    assert len([c for c in cells if c.source is not None]) >= 7
    for c in cells:
        if c.source is not None:
            assert c.data != c.source
            assert np.array_equal(_pil_rgb(c.data), _pil_rgb(c.source)), c.name
            assert jr.scan_symbols(c.data) == jr.scan_symbols(c.source), c.name
        assert np.array_equal(oracle.decode_rgb(c.data), _pil_rgb(c.data)), c.name
        assert np.array_equal(oracle.jpeg_to_tensor(c.data), oracle.pil_image_to_tensor(c.data)), c.name


def test_model_walks_the_files_own_symbols(cells):
    """The model's state machine against the re-coder's decoder (an
    independent restatement of T.81 F.2.2): after as many blocks as the
    segment holds, the true trajectory stands inside the segment's last byte."""
    for c in cells:
        for st, syms in zip(hm.streams(c.data), jr.scan_symbols(c.data)):
            s = (0, 0, 0)
            for _ in range(sum(1 for _, tc, _, _ in syms if tc == 0)):
                s = _next_block(st, s)
            assert st.bits - 8 < s[0] <= st.bits and s[2] == 0, (c.name, s, st.bits)
            assert s[0] == sum(len(bits) for bits in _code_bits(c.data, syms)), c.name


def _next_block(st, s):
    s = st.step(*s)
    while s[2] != 0:
        s = st.step(*s)
    return s


def _code_bits(jpeg, syms):
    """The bit string (code and extra bits) of each symbol of a segment."""
    fr = jr._frame(jr.parse(jpeg)[0])
    enc = {(tc, th): {sym: format(code, "0%db" % n) for sym, n, code in jr.canonical(counts, symbols)}
           for tc, th, counts, symbols in jr.dht_tables(jpeg)}
    for ci, tc, sym, extra in syms:
        yield enc[tc, fr.sel[fr.comps[ci][0]][tc]][sym] + extra


def test_locked_cells_never_merge(cells, models):
    """No guess of a locked cell shares a state with the truth, so the truth
    moves one slot per round: rounds = the longest segment's slots (one per
    hand-over after slot 0, and the last round that finds nothing to do), no
    memo adoption, one needy slot per round and segment. Each restart
    segment's chain starts afresh."""
    locked = _tagged(cells, "locked")
    want = {"slots2": 2, "slots65": 65, "slots66": 66}
    for c in locked:
        m = models[c.name]
        assert all(p == {1} for p in jr.block_start_parities(c.data)), c.name
        nm = hm.never_merges(c.data, S)
        assert [len(x) for x in nm] == [s.slots for s in m.segments]
        assert all(not x[0] and all(x[1:]) for x in nm), c.name
        assert hm.single_symbol_steps(c.data), c.name  # the model is exact here
        assert m.rounds == max(s.slots for s in m.segments), (c.name, m.rounds)
        assert m.adoptions == 0 and m.needy == m.slots - len(m.segments) and m.wide == 0, c.name
        for s in m.segments:
            assert s.rounds == s.slots and s.needy == [1] * (s.slots - 1) + [0], c.name
        for tag, n in want.items():
            if tag in c.tags:
                assert m.slots == n, c.name
        # the warm-up starts on the range starts' parity as well, so it cannot help, except that
        # 2 S of it take slots 1 and 2 back to the segment's start, which is the truth
        assert hm.model(c.data, S, warm_pct=50).rounds == m.rounds, c.name
        assert hm.model(c.data, S, warm_pct=200).rounds == max(max(s.slots for s in m.segments) - 2, 1), c.name
    assert {t for c in locked for t in c.tags if t.startswith("slots")} == {"slots2", "slots65", "slots66", "slots1000"}
    big = _tagged(cells, "slots1000")[0]
    assert 1000 <= models[big.name].slots <= MAX_SLOTS
    rst = _tagged(_tagged(cells, "locked"), "restart")[0]
    segs = models[rst.name].segments
    assert 2 <= len(segs) <= 16 and max(s.slots for s in segs) >= 200 and len({s.slots for s in segs}) > 1


def test_even_twin_needs_no_round(cells, models):
    """The same kind of file with its block starts on the range starts'
    parity: every guess is the truth, the first round finds nothing to do
    (the kernel counts that round: 1)."""
    for c in _tagged(cells, "zero-rounds"):
        m = models[c.name]
        assert all(p == {0} for p in jr.block_start_parities(c.data)), c.name
        assert m.slots >= 65 and m.needy == 0 and m.rounds == 1 and m.adoptions == 0, (c.name, m)
        assert not any(x for seg in hm.never_merges(c.data, S) for x in seg), c.name


def test_slow_cells_reach_the_memo_and_a_second_wave(cells, models):
    """At least 8 memo adoptions and a round with more than 64 needy slots
    (the margin: count-mode steps shift individual exits, which the model
    does not see), and more rounds without the memo than with it."""
    slow = _tagged(cells, "slow")
    assert len(slow) == 3
    for c in slow:
        m = models[c.name]
        assert m.adoptions >= 8 and m.wide >= 1, (c.name, m.adoptions, m.wide)
        assert m.rounds >= 8 and hm.model(c.data, S, memo=False).rounds > m.rounds, c.name
        assert not hm.single_symbol_steps(c.data), c.name
        assert len(jr.scan_bytes(c.data)) <= 12 * (MAX_SLOTS - 1), c.name  # S = 96 from the planner


def test_segment_geometries(cells):
    """The tags are recomputed from the bytes."""
    have = set()
    for c in cells:
        geo = {t for t in c.tags if t.startswith("seg-")}
        if geo:
            assert jr.geometry_tags(c.data) == geo, c.name
            have |= geo
    assert have == {"seg-kS", "seg-kS+8", "seg-short", "seg-mid"}
    a, b = _tagged(cells, "nseg256")[0], _tagged(cells, "nseg257")[0]
    assert len(jr._segment_bits(a.data)) == MAX_PAR_SEGS and len(jr._segment_bits(b.data)) == MAX_PAR_SEGS + 1


def test_model_warm_up_and_memo_keep_the_result(cells):
    """Whatever the warm-up and with or without the memo, the rounds end on
    the serial walk's entries (the model asserts it)."""
    for c in cells:
        for pct in (50, 200):
            assert hm.model(c.data, S, warm_pct=pct).slots == hm.model(c.data, S, memo=False).slots


@pytest.mark.parametrize("args", [("sb=64",), ("sb=64", "win_cap=0"), ("sb=64", "fuse=0")])
def test_planner_gives_the_cells_their_geometry(planner, cells, models, args):
    """Under subseq_bits = 64: S = 96 except on the serial decoder's cell,
    the tagged segment counts, 256 segments on the parallel decoder and 257 on
    the serial one, and the slots the model counts, at most 1024."""
    plan = _plan_batch(planner, [c.data for c in cells], *args)
    rows = plan["rows"]
    assert [r["status"] for r in rows] == [0] * len(cells)
    for i, (c, r) in enumerate(zip(cells, rows)):
        assert r["sub_bits"] == c.sub_bits, (c.name, r["sub_bits"])
        assert r["nseg"] == c.nseg == len(jr._segment_bits(c.data)), (c.name, r["nseg"])
        assert (i in plan["par_img"]) == (c.sub_bits > 0), c.name
        if r["sub_bits"]:
            slots = sum(max(1, -(-b // r["sub_bits"])) for b in jr._segment_bits(c.data))
            assert slots == models[c.name].slots == sum(hm.slot_counts(c.data, r["sub_bits"])), c.name
            assert slots <= MAX_SLOTS, (c.name, slots)
    serial = [c.name for c in cells if c.sub_bits == 0]
    assert serial == ["nseg-257"] and plan["totals"]["n_serial"] == 1
    assert rows[[c.name for c in cells].index("nseg-256")]["nseg"] == MAX_PAR_SEGS
    # each cell alone plans the same
    assert planner([c.data for c in cells]) == [0] * len(cells)
