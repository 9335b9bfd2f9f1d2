#!/usr/bin/env python
"""What the fused photometric stage (``color=``) costs, on the c2-shaped
resident batch (256 x 512x512 q90 4:2:0, cells in HBM) decoded to two 224 x 224
views with ``RandomResizedCropFlip()`` boxes and ``ColorJitterParams()``
defaults (seed 1234), output bfloat16, channels_last, ImageNet Normalize.

One process, one context and stream, the variants interleaved round by round
(the order rotates), HIP events around ``steps`` units, medians over the rounds:

  * ``plain``       the call without ``color=``;
  * ``color``       the call with the sampled colours;
  * ``color-nocontrast``  the same entries with contrast absent: k_color_mean is
                    not launched, so the stage is k_color_apply alone;
  * ``uint8+torch`` what a user does without the stage, colour ops of their own
                    aside: the ``dtype=uint8`` call, then ``.to(bfloat16)``, a
                    normalise and a ``channels_last`` copy in torch.

A second pass with LDT_OPT_PROFILE 1 reads the ``color`` stage's own time
(``ldt_stage_times``) for the two colour variants and derives the share of HBM
bandwidth from the bytes the stage moves: per output pixel 3 read + 3 *
elemsize written, plus 3 read again for entries with contrast. The parent
commit is not measured here: build it aside and run its ``tools/bench_views.py``
for the call without ``color=``.

    python tools/bench_color.py [--rounds 5] [--steps 40] [--out FILE]
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
from ldt_amd import _lib, synth  # noqa: E402
from ldt_amd import transforms as T  # noqa: E402

SIZE, V, SEED = (224, 224), 2, 1234
HBM_GBS = 8000.0  # MI355X peak, as bench.py's roofline takes it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cells, labels = synth.q90_512(256, seed=1000)
    res = ldt_amd.ResidentBatch(cells, labels, device=dev)
    n = res.n
    wh, st = res.image_sizes()
    boxes = ldt_amd.RandomResizedCropFlip(generator=torch.Generator().manual_seed(SEED)).sample(wh, st, views=V)
    rows = ldt_amd.ColorJitterParams(generator=torch.Generator().manual_seed(SEED)).sample(n, views=V)
    colors = _lib.check_colors(rows, n, V)
    rows_nc = rows.copy()
    rows_nc[..., 1] = np.nan
    colors_nc = _lib.check_colors(rows_nc, n, V)
    ctx = _lib.Context(dev.index)
    ctx.set_option(_lib.OPT_SYNC_STATUS, 0)
    out = T._empty_image(n, SIZE, "bfloat16", "channels_last", dev, V)
    out8 = T._empty_image(n, SIZE, "uint8", "contiguous", dev, V)
    lbl = torch.empty((n,), dtype=torch.int64, device=dev)
    mean = torch.tensor(ldt_amd.IMAGENET_MEAN, device=dev, dtype=torch.bfloat16).view(1, 1, 3, 1, 1)
    std = torch.tensor(ldt_amd.IMAGENET_STD, device=dev, dtype=torch.bfloat16).view(1, 1, 3, 1, 1)
    fmt = dict(dtype=torch.bfloat16, memory_format=torch.channels_last)

    def plain():
        res.decode(out, lbl, True, ctx=ctx, size=SIZE, crops=boxes, views=V, **fmt)

    def color():
        res.decode(out, lbl, True, ctx=ctx, size=SIZE, crops=boxes, views=V, colors=colors, **fmt)

    def color_nc():
        res.decode(out, lbl, True, ctx=ctx, size=SIZE, crops=boxes, views=V, colors=colors_nc, **fmt)

    def torch_way():
        res.decode(out8, lbl, None, ctx=ctx, size=SIZE, crops=boxes, views=V, dtype=torch.uint8)
        x = out8.to(torch.bfloat16).div_(255.0).sub_(mean).div_(std)
        return x.flatten(0, 1).contiguous(memory_format=torch.channels_last)

    variants = [("plain", plain), ("color", color), ("color-nocontrast", color_nc), ("uint8+torch", torch_way)]

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
    # the colour stage's own time, profiling on, in a pass of its own
    ctx.set_option(_lib.OPT_PROFILE, 1)
    stage = {}
    for k, fn in variants[1:3]:
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
    px = n * V * SIZE[0] * SIZE[1]
    with_contrast = int(np.count_nonzero(colors["mask"] & 2)) * SIZE[0] * SIZE[1]
    result = {"workload": f"c2 resident batch {n} x 512x512 -> {V} x {SIZE[0]}x{SIZE[1]}, bf16 channels_last Normalize, "
                          f"seed {SEED}", "rounds": a.rounds, "steps": a.steps, "version": ldt_amd.version()}
    for k, _ in variants:
        result[k] = {"ms_median": statistics.median(ms[k]), "ms_rounds": ms[k]}
    for k, bytes_moved in (("color", px * (3 + 3 * 2) + 3 * with_contrast), ("color-nocontrast", px * (3 + 3 * 2))):
        c = statistics.median(v["color"] for v in stage[k])
        result[k].update({"stage_color_ms_median": c, "stage_resize_ms_median": statistics.median(v["resize"] for v in stage[k]),
                          "stage_rounds": stage[k], "stage_bytes": bytes_moved,
                          "stage_gb_s": bytes_moved / (c * 1e-3) / 1e9 if c > 0 else None,
                          "stage_hbm_share": bytes_moved / (c * 1e-3) / 1e9 / HBM_GBS if c > 0 else None})
    result["entries_with_contrast"] = int(np.count_nonzero(colors["mask"] & 2))
    result["entries"] = n * V
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
