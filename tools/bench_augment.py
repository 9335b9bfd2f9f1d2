#!/usr/bin/env python
"""What the fused auto-augment stage (``augment=``) costs, on the c2-shaped
resident batch (256 x 512x512 q90 4:2:0, cells in HBM) decoded to 224 x 224
with ``RandomResizedCropFlip()`` boxes (seed 1234), output bfloat16,
channels_last, ImageNet Normalize: the supervised recipes' shape.

One process, one context and stream, the variants interleaved round by round
(the order rotates), HIP events around ``steps`` units, medians over the rounds:

  * ``plain``        the call without ``augment=``;
  * ``trivial``      ``TrivialAugmentWide()``'s draws for the batch;
  * ``trivial+erase``  the same with ``RandomErasing(0.25)``'s boxes;
  * ``rand``         ``RandAugment()``'s draws (two ops per image);
  * ``rand+erase``   the same with ``RandomErasing(0.25)``'s boxes;
  * ``uint8+torch``  what a user does without the stage, before any op of their
                     own: the ``dtype=uint8`` call, then ``.to(bfloat16)``, a
                     normalise and a ``channels_last`` copy in torch.

The draws are made once, before the timing, so the ms per call are the device
call's alone. What the samplers cost on the host is timed apart
(``sampler_host_ms``: ``time.perf_counter`` around ``sample(256, size)``, median
of ``rounds`` x 3 calls, one thread): serial Python in the thread that enqueues
the batch, as ``RandomResizedCropFlip.sample`` is (timed beside them). A second
pass with LDT_OPT_PROFILE 1 reads the stage's own time (the ``color`` entry of
``ldt_stage_times``) for the four augment variants.
``--only plain`` times the call without ``augment=`` alone: run it alternately
with LDT_LIBRARY set to a build of the parent commit to compare the two.

    python tools/bench_augment.py [--rounds 5] [--steps 40] [--only plain] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lance-distributed-training_amd"))

import torch  # noqa: E402

import ldt_amd  # noqa: E402
from ldt_amd import _lib, synth  # noqa: E402
from ldt_amd import transforms as T  # noqa: E402

SIZE, SEED = (224, 224), 1234


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--only", default=None, help="time this variant alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cells, labels = synth.q90_512(256, seed=1000)
    res = ldt_amd.ResidentBatch(cells, labels, device=dev)
    n = res.n
    wh, st = res.image_sizes()
    boxes = ldt_amd.RandomResizedCropFlip(generator=torch.Generator().manual_seed(SEED)).sample(wh, st)

    def gen():
        return torch.Generator().manual_seed(SEED)

    draws, host_ms = {}, {}

    def host_time(name, make):
        """Median host ms of one batch's draws by the sampler make(generator) builds."""
        g = gen()
        sampler = make(g)
        vals = []
        for _ in range(3 * a.rounds):
            t = time.perf_counter()
            sampler(n)
            vals.append((time.perf_counter() - t) * 1e3)
        host_ms[name] = statistics.median(vals)

    if a.only is None:
        E = ldt_amd.RandomErasing
        host_time("crop", lambda g: (lambda k, s=ldt_amd.RandomResizedCropFlip(generator=g): s.sample(wh, st)))
        host_time("trivial", lambda g: (lambda k, s=ldt_amd.TrivialAugmentWide(generator=g): s.sample(k, SIZE)))
        host_time("trivial+erase", lambda g: (
            lambda k, s=ldt_amd.TrivialAugmentWide(generator=g, erase=E(0.25, generator=g)): s.sample(k, SIZE)))
        host_time("rand", lambda g: (lambda k, s=ldt_amd.RandAugment(generator=g): s.sample(k, SIZE)))
        host_time("rand+erase", lambda g: (
            lambda k, s=ldt_amd.RandAugment(generator=g, erase=E(0.25, generator=g)): s.sample(k, SIZE)))
    if a.only in (None, "trivial", "trivial+erase", "rand", "rand+erase"):
        g = gen()
        draws["trivial"] = ldt_amd.TrivialAugmentWide(generator=g).sample(n, SIZE)
        g = gen()
        draws["trivial+erase"] = ldt_amd.TrivialAugmentWide(
            generator=g, erase=ldt_amd.RandomErasing(0.25, generator=g)).sample(n, SIZE)
        g = gen()
        draws["rand"] = ldt_amd.RandAugment(generator=g).sample(n, SIZE)
        g = gen()
        draws["rand+erase"] = ldt_amd.RandAugment(
            generator=g, erase=ldt_amd.RandomErasing(0.25, generator=g)).sample(n, SIZE)
    ctx = _lib.Context(dev.index)
    ctx.set_option(_lib.OPT_SYNC_STATUS, 0)
    out = T._empty_image(n, SIZE, "bfloat16", "channels_last", dev, None)
    out8 = T._empty_image(n, SIZE, "uint8", "contiguous", dev, None)
    lbl = torch.empty((n,), dtype=torch.int64, device=dev)
    mean = torch.tensor(ldt_amd.IMAGENET_MEAN, device=dev, dtype=torch.bfloat16).view(1, 3, 1, 1)
    std = torch.tensor(ldt_amd.IMAGENET_STD, device=dev, dtype=torch.bfloat16).view(1, 3, 1, 1)
    fmt = dict(dtype=torch.bfloat16, memory_format=torch.channels_last)

    def plain():
        res.decode(out, lbl, True, ctx=ctx, size=SIZE, crops=boxes, **fmt)

    def with_aug(rec):
        return lambda: res.decode(out, lbl, True, ctx=ctx, size=SIZE, crops=boxes, augments=rec, **fmt)

    def torch_way():
        res.decode(out8, lbl, None, ctx=ctx, size=SIZE, crops=boxes, dtype=torch.uint8)
        x = out8.to(torch.bfloat16).div_(255.0).sub_(mean).div_(std)
        return x.contiguous(memory_format=torch.channels_last)

    variants = [("plain", plain)] + [(k, with_aug(v)) for k, v in draws.items()] + [("uint8+torch", torch_way)]
    if a.only is not None:
        variants = [(k, fn) for k, fn in variants if k == a.only]
        if not variants:
            raise SystemExit(f"--only {a.only!r}: no such variant")

    def timed(fn, steps):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    ms = {k: [] for k, _ in variants}
    for r in range(a.rounds):
        for k, fn in variants[r % len(variants):] + variants[:r % len(variants)]:
            ms[k].append(timed(fn, a.steps))
    # the stage's own time, profiling on, in a pass of its own
    stage = {}
    ctx.set_option(_lib.OPT_PROFILE, 1)
    for k, fn in variants:
        if k not in draws:
            continue
        vals = []
        for _ in range(a.rounds):
            fn()
            torch.cuda.synchronize()
            ctx.stage_times(reset=True)
            for _ in range(a.steps):
                fn()
            t = ctx.stage_times(reset=True)
            vals.append({s: t[s][0] / max(1, t[s][1]) for s in ("resize", "color")})
        stage[k] = vals
    ctx.set_option(_lib.OPT_PROFILE, 0)
    result = {"workload": f"c2 resident batch {n} x 512x512 -> {SIZE[0]}x{SIZE[1]}, RandomResizedCropFlip, bf16 "
                          f"channels_last Normalize, seed {SEED}", "rounds": a.rounds, "steps": a.steps,
              "version": ldt_amd.version(), "library": os.environ.get("LDT_LIBRARY", ""),
              "sampler_host_ms": host_ms}
    for k, _ in variants:
        result[k] = {"ms_median": statistics.median(ms[k]), "ms_rounds": ms[k],
                     "img_per_s": n / (statistics.median(ms[k]) * 1e-3)}
        if k in stage:
            rec = draws[k]
            result[k].update({"stage_ms_median": statistics.median(v["color"] for v in stage[k]),
                              "stage_resize_ms_median": statistics.median(v["resize"] for v in stage[k]),
                              "stage_rounds": stage[k], "slots": int(max(1, rec["count"].max())),
                              "ops": int(rec["count"].sum()), "erase_boxes": int((rec["erase"][..., 2] > 0).sum())})
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
