#!/usr/bin/env python
"""What the filtered affine op (``affine_filter=``, k_aug_affine_filt) costs, on
tools/bench_augment.py's batch and conditions: the c2-shaped resident batch
(256 x 512x512 q90 4:2:0, cells in HBM) decoded to 224 x 224 with
``RandomResizedCropFlip()`` boxes (seed 1234), output bfloat16, channels_last,
ImageNet Normalize.

One process, one context and stream, the variants interleaved round by round
(the order rotates), HIP events around ``steps`` units, medians over the rounds:

  * ``plain``      the call without ``augment=``;
  * ``nearest``    ``TrivialAugmentWide()``'s draws for the batch (seed 1234);
  * ``bilinear``   the same draws with ``affine_filter="bilinear"``;
  * ``bicubic``    the same draws with ``affine_filter="bicubic"``;
  * ``uint8+torch``  what a user does without the op: the ``dtype=uint8`` call,
                   ``.float()``, torch's ``affine_grid`` + ``grid_sample``
                   (bilinear, zero fill) with the geometric entries' matrices
                   (the identity for the others), then ``.to(bfloat16)``, a
                   normalise and a ``channels_last`` copy. Torch's sampler is
                   not Pillow's: it stands for the cost, not for the pixels.

The records are drawn once, before the timing. A second pass with
LDT_OPT_PROFILE 1 reads the augment stage's own time (the ``color`` entry of
``ldt_stage_times``). ``--only plain`` or ``--only nearest`` times one variant
alone: run it alternately with LDT_LIBRARY set to a build of the parent commit
to compare the two (profiles/affine/ab_parent.txt).

    python tools/bench_affine.py [--rounds 5] [--steps 40] [--only nearest] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lance-distributed-training_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ldt_amd  # noqa: E402
from ldt_amd import _lib  # noqa: E402
from ldt_amd import transforms as T  # noqa: E402
from ldt_amd import synth  # noqa: E402

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

    def draw(**kw):
        return ldt_amd.TrivialAugmentWide(generator=torch.Generator().manual_seed(SEED), **kw).sample(n, SIZE)

    draws = {"nearest": draw()}
    if a.only in (None, "bilinear", "bicubic", "uint8+torch"):  # a parent's library has no filters
        draws.update(bilinear=draw(affine_filter="bilinear"), bicubic=draw(affine_filter="bicubic"))
    ctx = _lib.Context(dev.index)
    ctx.set_option(_lib.OPT_SYNC_STATUS, 0)
    out = T._empty_image(n, SIZE, "bfloat16", "channels_last", dev, None)
    out8 = T._empty_image(n, SIZE, "uint8", "contiguous", dev, None)
    lbl = torch.empty((n,), dtype=torch.int64, device=dev)
    mean = torch.tensor(ldt_amd.IMAGENET_MEAN, device=dev, dtype=torch.bfloat16).view(1, 3, 1, 1)
    std = torch.tensor(ldt_amd.IMAGENET_STD, device=dev, dtype=torch.bfloat16).view(1, 3, 1, 1)
    fmt = dict(dtype=torch.bfloat16, memory_format=torch.channels_last)
    theta = None
    if "bilinear" in draws:
        # affine_grid's normalised form of each entry's pixel matrix (align_corners=False)
        h, w = SIZE
        th = np.tile(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (n, 1, 1))
        f = draws["bilinear"]["filt"][:, 0]
        for i in np.nonzero(f["filter"])[0]:
            m = f["m"][i]
            th[i] = [[m[0], m[1] * h / w, m[0] + m[1] * h / w + 2 * m[2] / w - 1],
                     [m[3] * w / h, m[4], m[3] * w / h + m[4] + 2 * m[5] / h - 1]]
        theta = torch.tensor(th, dtype=torch.float32, device=dev)

    def plain():
        res.decode(out, lbl, True, ctx=ctx, size=SIZE, crops=boxes, **fmt)

    def with_aug(rec):
        return lambda: res.decode(out, lbl, True, ctx=ctx, size=SIZE, crops=boxes, augments=rec, **fmt)

    def torch_way():
        res.decode(out8, lbl, None, ctx=ctx, size=SIZE, crops=boxes, dtype=torch.uint8)
        grid = torch.nn.functional.affine_grid(theta, (n, 3) + SIZE, align_corners=False)
        x = torch.nn.functional.grid_sample(out8.float(), grid, mode="bilinear", padding_mode="zeros",
                                            align_corners=False)
        x = x.to(torch.bfloat16).div_(255.0).sub_(mean).div_(std)
        return x.contiguous(memory_format=torch.channels_last)

    variants = [("plain", plain)] + [(k, with_aug(v)) for k, v in draws.items()]
    if theta is not None:
        variants.append(("uint8+torch", torch_way))
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
            vals.append(t["color"][0] / max(1, t["color"][1]))
        stage[k] = vals
    ctx.set_option(_lib.OPT_PROFILE, 0)
    result = {"workload": f"c2 resident batch {n} x 512x512 -> {SIZE[0]}x{SIZE[1]}, RandomResizedCropFlip, bf16 "
                          f"channels_last Normalize, TrivialAugmentWide seed {SEED}", "rounds": a.rounds,
              "steps": a.steps, "version": ldt_amd.version(), "library": os.environ.get("LDT_LIBRARY", ""),
              "geometric_entries": int((draws["nearest"]["op"]["code"][:, 0] == _lib.AUG_AFFINE).sum())}
    if "bilinear" in draws:
        result["filtered_entries"] = int((draws["bilinear"]["filt"]["filter"] != 0).sum())
    for k, _ in variants:
        result[k] = {"ms_median": statistics.median(ms[k]), "ms_rounds": ms[k],
                     "img_per_s": n / (statistics.median(ms[k]) * 1e-3)}
        if k in stage:
            result[k].update({"stage_ms_median": statistics.median(stage[k]), "stage_rounds": stage[k]})
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
