#!/usr/bin/env python
"""What the fused mix stage (``mix=``) costs, on the conditions of
tools/bench_augment.py: the c2-shaped resident batch (256 x 512x512 q90 4:2:0,
cells in HBM) decoded to 224 x 224 with ``RandomResizedCropFlip()`` boxes and
``TrivialAugmentWide(erase=RandomErasing(0.1))`` records drawn once (seed 1234),
output bfloat16, channels_last, ImageNet Normalize: torchvision's reference
recipe up to its batch step.

One process, one context and stream, the variants interleaved round by round
(the order rotates), HIP events around ``steps`` units, medians over the rounds:

  * ``plain``        the call without ``mix=``;
  * ``mixup``        the call with ``MixUp(0.2)``'s rows (1000 classes);
  * ``cutmix``       the call with ``CutMix(1.0)``'s rows;
  * ``plain+torch``  what a user does without the stage: the same call without
                     ``mix=``, then ``roll`` / ``mul`` / ``add`` on the batch and
                     ``one_hot`` + the same three ops on the labels, in torch.

A second pass with LDT_OPT_PROFILE 1 reads the stage's own time (the ``color``
entry of ``ldt_stage_times``: the augment slot, k_mix_apply and k_mix_labels)
for ``plain``, ``mixup`` and ``cutmix``; the difference to ``plain``'s is the
mix kernels'. ``mix_bytes`` is what k_mix_apply moves, n * h * w * (6 + 3 * es)
bytes (two rows' uint8 planes read, one row of es-byte elements written), and
``mix_hbm_share`` that traffic over the stage's extra time as a share of
``--hbm-peak`` (GB/s, default 8000).
``--only plain`` times the call without ``mix=`` alone: run it alternately with
LDT_LIBRARY set to a build of the parent commit to compare the two.

    python tools/bench_mix.py [--rounds 5] [--steps 40] [--only plain] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lance-distributed-training_amd"))

import torch  # noqa: E402

import ldt_amd  # noqa: E402
from ldt_amd import _lib, synth  # noqa: E402
from ldt_amd import transforms as T  # noqa: E402

SIZE, SEED, NC = (224, 224), 1234, 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--only", default=None, help="time this variant alone")
    ap.add_argument("--hbm-peak", type=float, default=8000.0, help="GB/s")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cells, _ = synth.q90_512(256, seed=1000)
    labels = [(37 * i) % NC for i in range(len(cells))]
    res = ldt_amd.ResidentBatch(cells, labels, device=dev)
    n = res.n
    wh, st = res.image_sizes()
    g = torch.Generator().manual_seed(SEED)
    boxes = ldt_amd.RandomResizedCropFlip(generator=g).sample(wh, st)
    augs = ldt_amd.TrivialAugmentWide(generator=g, erase=ldt_amd.RandomErasing(0.1, generator=g)).sample(n, SIZE)
    draws = {}
    if a.only in (None, "mixup", "cutmix"):
        draws["mixup"] = ldt_amd.MixUp(0.2, num_classes=NC, generator=g).sample(n, SIZE)
        draws["cutmix"] = ldt_amd.CutMix(1.0, num_classes=NC, generator=g).sample(n, SIZE)
    ctx = _lib.Context(dev.index)
    ctx.set_option(_lib.OPT_SYNC_STATUS, 0)
    out = T._empty_image(n, SIZE, "bfloat16", "channels_last", dev, None)
    lbl = torch.empty((n,), dtype=torch.int64, device=dev)
    soft = torch.empty((n, NC), dtype=torch.float32, device=dev)
    fmt = dict(dtype=torch.bfloat16, memory_format=torch.channels_last)
    common = dict(ctx=ctx, size=SIZE, crops=boxes, augments=augs, **fmt)
    lam = 0.3

    def plain():
        res.decode(out, lbl, True, **common)

    def with_mix(mix):
        spec = T.CallSpec.make(True, SIZE, None, fmt["dtype"], fmt["memory_format"], None, boxes, None, None, augs, mix)
        return lambda: res._decode(spec, out, lbl, ctx, None, soft)

    def torch_way():
        res.decode(out, lbl, True, **common)
        x = out.roll(1, 0).mul_(1.0 - lam).add_(out.mul(lam))
        hot = torch.nn.functional.one_hot(lbl, NC).float()
        return x, hot.roll(1, 0).mul_(1.0 - lam).add_(hot.mul(lam))

    variants = [("plain", plain)] + [(k, with_mix(v)) for k, v in draws.items()] + [("plain+torch", torch_way)]
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
        if k == "plain+torch":
            continue
        vals = []
        for _ in range(a.rounds):
            fn()
            torch.cuda.synchronize()
            ctx.stage_times(reset=True)
            for _ in range(a.steps):
                fn()
            t = ctx.stage_times(reset=True)
            vals.append(t["color"][0] / max(1, t["color"][1]))
        stage[k] = vals
    ctx.set_option(_lib.OPT_PROFILE, 0)
    es = 2
    mix_bytes = n * SIZE[0] * SIZE[1] * (6 + 3 * es)
    result = {"workload": f"c2 resident batch {n} x 512x512 -> {SIZE[0]}x{SIZE[1]}, RandomResizedCropFlip, "
                          f"TrivialAugmentWide + RandomErasing(0.1), bf16 channels_last Normalize, seed {SEED}, "
                          f"{NC} classes", "rounds": a.rounds, "steps": a.steps, "version": ldt_amd.version(),
              "library": os.environ.get("LDT_LIBRARY", ""), "mix_bytes": mix_bytes, "hbm_peak_gbs": a.hbm_peak}
    for k, _ in variants:
        result[k] = {"ms_median": statistics.median(ms[k]), "ms_rounds": ms[k],
                     "img_per_s": n / (statistics.median(ms[k]) * 1e-3)}
        if k in stage:
            result[k].update({"stage_ms_median": statistics.median(stage[k]), "stage_rounds": stage[k]})
    for k in draws:
        if k in stage and "plain" in stage:
            extra = result[k]["stage_ms_median"] - result["plain"]["stage_ms_median"]
            result[k]["mix_stage_extra_ms"] = extra
            if extra > 0:
                result[k]["mix_gbs"] = mix_bytes / (extra * 1e-3) / 1e9
                result[k]["mix_hbm_share"] = result[k]["mix_gbs"] / a.hbm_peak
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
