"""The sync cache's cold path and its phases.

cold: N distinct c2 batches (different seeds), each decoded once through a
depth-3 DecodePipeline from a cleared table: every image misses and is
inserted. Alternated between LDT_OPT_SYNC_CACHE 0 and 1 on the same batches;
the difference is what the probe, the fingerprint and the 8 KB payload store
cost per image. (bench.py's timed region is the other end: all hits.)

stages: one batch in flight (HIP events around the stages, LDT_OPT_PROFILE):
the Huffman stage of one c2 batch with the cache off, cold (after a clear) and
warm. tools/probes/huff_rounds.py cannot see a hit: its counters bypass the
cache.

usage: sync_cache_rate.py [N batches = 8] [reps = 7]
"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..", "lance-distributed-training_amd"))
import torch  # noqa: E402

import ldt_amd  # noqa: E402
from ldt_amd import _lib, synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 8
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
BATCH = 256

batches = [ldt_amd.ResidentBatch(*synth.q90_512(BATCH, seed=2000 + i)) for i in range(N)]
pipe = ldt_amd.DecodePipeline(depth=3)
ctx0 = pipe.ctxs[0]


def cold_pass(opt):
    pipe.set_option(_lib.OPT_SYNC_CACHE, opt)
    ctx0.sync_cache_clear()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for b in batches:
        pipe.decode(b)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    pipe.check()
    return N * BATCH / dt


for opt in (0, 1):  # warm-up: allocations, the table itself
    cold_pass(opt)
rates = {0: [], 1: []}
for rep in range(REPS):
    for opt in (0, 1):
        rates[opt].append(cold_pass(opt))
        print(f"cold rep{rep + 1} sync_cache={opt} {rates[opt][-1]:.1f} img/s", flush=True)
pipe.set_option(_lib.OPT_SYNC_CACHE, 2)
ctx0.sync_cache_clear()
for b in batches:
    pipe.decode(b)
torch.cuda.synchronize()
print("cold counters", ctx0.sync_cache_stats(), flush=True)
med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
spread0 = max(rates[0]) - min(rates[0])
us = (1.0 / med[1] - 1.0 / med[0]) * 1e6
print(f"cold median: off {med[0]:.1f} on {med[1]:.1f} img/s; off spread (max - min) {spread0:.1f}; "
      f"on - off = {med[1] - med[0]:.1f}; insert cost {us * 1000:.1f} ns per image of pipeline time", flush=True)

# stages at depth 1
ctx = _lib.get_context(0)
ctx.set_option(_lib.OPT_PROFILE, 1)
rb = batches[0]


def stage(label, opt, clear):
    ctx.set_option(_lib.OPT_SYNC_CACHE, opt)
    rb.decode()
    torch.cuda.synchronize()
    ctx.stage_times(reset=True)
    for _ in range(8):
        if clear:
            ctx.sync_cache_clear()
        rb.decode()
        torch.cuda.synchronize()
    st = {k: round(v[0] / max(v[1], 1), 4) for k, v in ctx.stage_times(reset=True).items() if v[1]}
    print(f"stages {label}: {st}", flush=True)


stage("off", 0, False)
stage("cold (miss + insert)", 1, True)
stage("warm (hit)", 1, False)

# outputs: cold (first decode after a clear), warm and off, array for array
ctx.set_option(_lib.OPT_PROFILE, 0)
outs = {}
for label, opt, clear in (("off", 0, False), ("cold", 2, True), ("warm", 2, False)):
    ctx.set_option(_lib.OPT_SYNC_CACHE, opt)
    if clear:
        ctx.sync_cache_clear()
    a = ctx.sync_cache_stats()
    img, lbl = rb.decode()
    torch.cuda.synchronize()
    b = ctx.sync_cache_stats()
    outs[label] = (img.clone(), lbl.clone(), {k: b[k] - a[k] for k in ("hits", "misses", "inserts", "fallbacks")})
for label in ("cold", "warm"):
    same = torch.equal(outs[label][0], outs["off"][0]) and torch.equal(outs[label][1], outs["off"][1])
    print(f"outputs {label} == off: {same} {outs[label][2]}", flush=True)
