"""Which path of k_huff_image a GPU test runs: cold, hinted or uncached
(a test helper: tests import it, nothing else does).

The sync cache is the device's, on by default and never evicts, so without
this helper what a decode checks of phase 1 and the convergence rounds depends
on the cells that earlier tests of the same process decoded. A test whose
subject is the decoder chooses its path here:

``cold_then_warm(ctx, decode)`` clears the table and runs ``decode()`` twice
under LDT_OPT_SYNC_CACHE = 2: the first call runs phase 1, the rounds and the
warm-up on every image that consults the table and inserts the converged
states, the second goes from setup to the hinted write pass. The kernel's own
counters say so: the relations asserted below follow from sc_probe and
image_decode (ldt_huffman.hip), none is a measurement.

``uncached(ctx, decode)`` is for the configurations that must not consult the
table (the serial decoder, global reads, the unfused destuff, the debug
counters): no counter moves.

``cache_users(cells, ...)`` restates the planner's routing (ldt_plan.cpp
plan_one / plan_destuff, as tests/test_plan_fuzz.py does for the window) and
sc_use (ldt_huffman.hip, ldt_abi.cpp sc_view): the images of a batch that
consult the table under the given options. tests/test_huffman_paths.py holds
it against the planner itself on the CPU.

Both runners work on the shared context (``_lib.get_context(device)``), pass a
failed batch's row statuses through (``Run.rows``) and leave
LDT_OPT_SYNC_CACHE at its default.
"""
from collections import namedtuple

import jpeg_recode as jr

COUNTERS = ("hits", "misses", "inserts", "refused", "rejected", "fallbacks")

# out: what decode() returned (None if it raised ImageDecodeError); rows: the
# failed rows' statuses ({} if none); d: what the call added to the six counters
Run = namedtuple("Run", "out rows d")


def _counted(ctx, decode, what):
    import torch

    import ldt_amd

    torch.cuda.synchronize()
    a = ctx.sync_cache_stats()
    out, rows = None, {}
    try:
        out = decode()
    except ldt_amd.ImageDecodeError as e:
        rows = dict(e.rows)
    torch.cuda.synchronize()
    b = ctx.sync_cache_stats()
    d = {k: b[k] - a[k] for k in COUNTERS}
    print(f"huff_paths {what}: {({k: v for k, v in d.items() if v})}" + (f" rows {rows}" if rows else ""))
    return Run(out, rows, d)


def cold_then_warm(ctx, decode, dups=0, users=None, what="", clear=True):
    """(cold Run, warm Run) of decode() from a cleared table.

    dups: how many rows of the batch repeat an earlier row's file (a repeated
    file shares its entry: it may hit on the cold call, or two workgroups may
    both miss and both insert). users: how many images must consult the table,
    where the test's point needs the parallel decoder. clear=False: the caller
    cleared the table itself (before a failing call that must run cold too)
    and nothing that this batch holds was decoded since."""
    import torch

    from ldt_amd import _lib

    try:
        ctx.set_option(_lib.OPT_SYNC_CACHE, 2)
        if clear:
            torch.cuda.synchronize()
            ctx.sync_cache_clear()
        cold = _counted(ctx, decode, f"{what} cold")
        warm = _counted(ctx, decode, f"{what} warm")
    finally:
        ctx.set_option(_lib.OPT_SYNC_CACHE, 1)
    c, w = cold.d, warm.d
    assert cold.rows == warm.rows, (what, cold.rows, warm.rows)
    assert c["hits"] <= dups, (what, c)
    assert c["fallbacks"] == 0 and c["rejected"] == 0, (what, c)
    assert c["refused"] == 0 or dups >= 4, (what, c)  # more workgroups of one key than its set has ways
    assert c["inserts"] <= c["misses"], (what, c)
    if users is not None:
        assert c["hits"] + c["misses"] == users, (what, users, c)
    assert w["fallbacks"] == 0 and w["rejected"] == 0, (what, w)
    if dups == 0:
        assert w["hits"] == c["inserts"], (what, c, w)
        assert w["misses"] == c["misses"] - c["inserts"], (what, c, w)  # failed rows: never kept
        assert w["inserts"] == 0, (what, w)
    else:
        assert w["hits"] + w["misses"] == c["hits"] + c["misses"], (what, c, w)
    return cold, warm


def uncached(ctx, decode, what="", cache=2):
    """The Run of decode() under a configuration that must not consult the
    table: no counter moves. cache: the LDT_OPT_SYNC_CACHE value of the call
    (0 where switching the cache off is the configuration)."""
    from ldt_amd import _lib

    try:
        ctx.set_option(_lib.OPT_SYNC_CACHE, cache)
        run = _counted(ctx, decode, f"{what} uncached")
    finally:
        ctx.set_option(_lib.OPT_SYNC_CACHE, 1)
    assert all(v == 0 for v in run.d.values()), (what, run.d)
    return run


# ---------------------------------------------------------------------------
# the planner's routing, restated
# ---------------------------------------------------------------------------
HUFF_THREADS, MAX_PAR_SEGS, MAX_PAR_S = 1024, 256, 32768  # ldt_types.hpp
HUFF_LDS_MAX, HUFF_STATIC_LDS = 160 * 1024, 42 * 1024
TAB_STRIDE = (2 << jr.LOOK_BITS) + (8 << (16 - jr.LOOK_BITS))  # uint16 per table
TAB_COMPACT_BYTES = (2 << jr.LOOK_BITS) + 2 * (8 << (16 - jr.LOOK_BITS))
HUFF_PLANE_BYTES = 16 * HUFF_THREADS + 4 * (HUFF_THREADS // 8)


def region_bytes(src_len, nseg):
    return (src_len + 16 + 8 * nseg + 15) & ~15  # ldt_types.hpp destuff_region_bytes


def tab_lds_image(max_tabs):
    t = max(max_tabs, 1)
    return max(t * TAB_STRIDE * 2, t * TAB_COMPACT_BYTES + HUFF_PLANE_BYTES)  # huff_tab_lds_image


Routing = namedtuple("Routing", "sub_bits nseg src_len ntabs")


def routing(cell, bits=256, mode=0):
    """A baseline cell's Routing (sub_bits 0: the serial decoder), None for a
    progressive one (ldt_plan.cpp plan_one)."""
    segs, ecs = jr.parse(cell)
    if any(m == 0xC2 for m, _ in segs):
        return None
    fr = jr._frame(segs)
    nseg = -(-fr.n_mcu // fr.restart) if fr.restart else 1
    tabs = {(tc, th): (tuple(counts), tuple(symbols)) for tc, th, counts, symbols in jr.dht_tables(cell)}
    used = {(tc, tabs[tc, fr.sel[cid][tc]]) for cid, _, _ in fr.comps for tc in (0, 1)}
    src_len = len(ecs)  # from the end of the SOS header to the end of the cell
    room = max(HUFF_THREADS - nseg, 1)
    min_s = -(-src_len * 8 // room)
    sub_bits = 0
    if mode != 1 and nseg <= MAX_PAR_SEGS and min_s <= MAX_PAR_S - 64:
        sub_bits = (max(min_s, bits, 64) + 31) & ~31
        if (sub_bits >> 5) & 1 == 0:
            sub_bits += 32  # an odd number of words per range
    return Routing(sub_bits, nseg, src_len, len(used))


def window_bytes(routes, window=-1):
    """The batch's LDS window (plan_destuff): the largest parallel image's
    need, under the LDS left beside the tables and the LDT_OPT_HUFF_WINDOW cap."""
    need = max((region_bytes(r.src_len, r.nseg) + 16 for r in routes if r and r.sub_bits), default=0)
    cap = HUFF_LDS_MAX - HUFF_STATIC_LDS - tab_lds_image(max((r.ntabs for r in routes if r), default=0))
    if window >= 0:
        cap = min(cap, window)
    return min(need, cap) & ~15


def key_dups(cells, bits=256, mode=0):
    """How many cells of the batch repeat an earlier cell's sync cache key
    (the `dups` of cold_then_warm). The key holds the scan bytes and their
    length, S and the segment count, nothing of the headers: the same file
    twice, and two files that differ before the scan (another APPn segment,
    other component or table ids), are one entry."""
    seen, n = set(), 0
    for c in cells:
        r = routing(c, bits, mode)
        if r and r.sub_bits:
            k = (jr.parse(c)[1], r.sub_bits, r.nseg)
            n += k in seen
            seen.add(k)
    return n


def cache_users(cells, bits=256, mode=0, window=-1, fused=1, counters=0, cache=1, cache_mb=1024):
    """Per cell of the batch: does its decode consult the sync cache? It does
    when the table exists and is handed to the kernel (sc_view: cache on, a
    budget of at least one set, no debug counters) and the image takes the
    fused destuff (sc_use): the parallel decoder, fusing on, and
    destuff_region_bytes(src_len, nseg) + 16 <= win_bytes."""
    routes = [routing(c, bits, mode) for c in cells]
    win = window_bytes(routes, window)
    table = cache != 0 and cache_mb > 0 and not counters
    return [bool(table and fused and r and r.sub_bits and region_bytes(r.src_len, r.nseg) + 16 <= win)
            for r in routes]


def census_cells():
    """name -> cell of the census batch (tests/test_gpu_huffman_paths.py): one
    segment of hundreds of slots, restart segments, a small cell, a stress
    cell that a 16 KB window does not hold, and the serial decoder's cell."""
    from ldt_amd import synth

    stress = {c.name: c for c in jr.stress_cells()}
    sync = {c.name: c for c in jr.sync_cells()}
    return {
        "q90-512": synth.q90_512(1, seed=71)[0][0],
        "inet": synth.imagenet_like(1, seed=72)[0][0],
        "small-64x96": synth.encode(synth.field(64, 96, 73, 6.0), quality=90),
        "ones-big": stress["ones-big"].data,
        "nseg-257": sync["nseg-257"].data,
    }
