#!/usr/bin/env python
"""What the fused GaussianBlur costs, on tools/bench_color.py's case: the
c2-shaped resident batch (256 x 512x512 q90 4:2:0, cells in HBM) decoded to two
224 x 224 views with ``RandomResizedCropFlip()`` boxes (seed 1234), output
bfloat16, channels_last, ImageNet Normalize.

One process, one context and stream, the variants interleaved round by round
(the order rotates), HIP events around ``steps`` units, medians over the rounds:

  * ``color``        ``ColorJitterParams()``: no blur, the kernels of a call
                     before the blur existed;
  * ``blur-1.0-0.1`` ``ColorJitterParams(blur_p=[1.0, 0.1])``: DINO's and BYOL's
                     two global views;
  * ``blur-1.0``     ``ColorJitterParams(blur_p=1.0)``: every output blurred;
  * ``blur-1.0-off`` ``blur-1.0``'s entries with the blur fields zeroed: the same
                     jitter through k_color_apply, so the two differ by the
                     blur alone;
  * ``uint8+torch``  the un-fused alternative for ``blur-1.0``'s radii, the
                     colour ops aside: the ``dtype=uint8`` call, then a
                     depthwise ``conv2d`` Gaussian per axis in bfloat16 (one 13-tap
                     kernel per output image, replicate padding), a normalise
                     and a ``channels_last`` copy in torch. It is not
                     Pillow's blur; it is what it costs to blur at all.

The three samplers share the seed, but a sampler with ``blur_p`` draws more, so
their jitter entries differ; the entries with contrast are counted per variant.

A second pass with LDT_OPT_PROFILE 1 reads the ``color`` stage's own time
(``ldt_stage_times``); the blur's added stage time is the difference to
``color``'s and to ``blur-1.0-off``'s. k_color_blur runs inside the stage's one
mark: with every entry blurred k_color_apply does nothing, so the kernel's own
time is the stage's less the mean pass. Its device traffic per blurred output
image is the tile regions' bytes read (3 per pixel of every tile's region, halo
included) and 3 * elemsize per pixel written.

``--only color`` measures the first variant alone (for a run against the parent
commit's library through LDT_LIBRARY, which knows no blur).

    python tools/bench_blur.py [--rounds 5] [--steps 40] [--only color] [--out FILE]
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
TILE_H, TILE_W = 32, 64  # k_color_blur's tile


def region_pixels(h, w, r):
    """Pixels k_color_blur loads for one h x w image at box radius r: every tile with its clipped halo."""
    halo, total = 3 * (r + 1), 0
    for y0 in range(0, h, TILE_H):
        for x0 in range(0, w, TILE_W):
            y1, x1 = min(h, y0 + TILE_H), min(w, x0 + TILE_W)
            total += (min(h, y1 + halo) - max(0, y0 - halo)) * (min(w, x1 + halo) - max(0, x0 - halo))
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cells, labels = synth.q90_512(256, seed=1000)
    res = ldt_amd.ResidentBatch(cells, labels, device=dev)
    n = res.n
    wh, st = res.image_sizes()
    boxes = ldt_amd.RandomResizedCropFlip(generator=torch.Generator().manual_seed(SEED)).sample(wh, st, views=V)

    def sampled(**kw):
        rows = ldt_amd.ColorJitterParams(generator=torch.Generator().manual_seed(SEED), **kw).sample(n, views=V)
        return rows, _lib.check_colors(rows, n, V)

    ctx = _lib.Context(dev.index)
    ctx.set_option(_lib.OPT_SYNC_STATUS, 0)
    out = T._empty_image(n, SIZE, "bfloat16", "channels_last", dev, V)
    out8 = T._empty_image(n, SIZE, "uint8", "contiguous", dev, V)
    lbl = torch.empty((n,), dtype=torch.int64, device=dev)
    mean = torch.tensor(ldt_amd.IMAGENET_MEAN, device=dev, dtype=torch.bfloat16).view(1, 1, 3, 1, 1)
    std = torch.tensor(ldt_amd.IMAGENET_STD, device=dev, dtype=torch.bfloat16).view(1, 1, 3, 1, 1)
    fmt = dict(dtype=torch.bfloat16, memory_format=torch.channels_last)

    def call(colors):
        return lambda: res.decode(out, lbl, True, ctx=ctx, size=SIZE, crops=boxes, views=V, colors=colors, **fmt)

    recs = {"color": sampled()}
    torch_error = None
    if a.only is None:
        recs["blur-1.0-0.1"] = sampled(blur_p=[1.0, 0.1])
        recs["blur-1.0"] = sampled(blur_p=1.0)
        off = recs["blur-1.0"][1].copy()
        off["blur_ww"] = 0
        off["blur_r"] = 0
        recs["blur-1.0-off"] = (recs["blur-1.0"][0][..., :7], off)
    variants = [(k, call(v[1])) for k, v in recs.items()]
    if a.only is None:
        # the torch way: a Gaussian of sigma = radius per output image, 13 taps, as one grouped conv2d per axis
        radii = torch.from_numpy(np.nan_to_num(recs["blur-1.0"][0][..., 7], nan=1.0).T.reshape(-1)).to(dev)
        x = torch.arange(-6, 7, device=dev, dtype=torch.float32)
        k1 = torch.exp(-0.5 * (x[None, :] / radii[:, None].float()) ** 2)
        k1 = (k1 / k1.sum(1, keepdim=True)).to(torch.bfloat16)  # [V * n, 13]
        kh = k1.repeat_interleave(3, 0).view(V * n * 3, 1, 1, 13)
        kv = kh.view(V * n * 3, 1, 13, 1)

        def torch_way():
            res.decode(out8, lbl, None, ctx=ctx, size=SIZE, crops=boxes, views=V, dtype=torch.uint8)
            y = out8.to(torch.bfloat16).view(1, V * n * 3, *SIZE)
            y = torch.nn.functional.pad(y, (6, 6, 6, 6), mode="replicate")
            y = torch.nn.functional.conv2d(y, kh, groups=V * n * 3)
            y = torch.nn.functional.conv2d(y, kv, groups=V * n * 3).view(V, n, 3, *SIZE)
            y = y.div_(255.0).sub_(mean).div_(std)
            return y.flatten(0, 1).contiguous(memory_format=torch.channels_last)

        try:
            torch_way()
            torch.cuda.synchronize()
            variants.append(("uint8+torch", torch_way))
        except RuntimeError as e:  # a grouped bfloat16 conv2d the installed MIOpen does not serve
            torch_error = str(e)[:300]

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
    ctx.set_option(_lib.OPT_PROFILE, 1)
    stage = {}
    for k, fn in variants:
        if k not in recs:
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
    result = {"workload": f"c2 resident batch {n} x 512x512 -> {V} x {SIZE[0]}x{SIZE[1]}, bf16 channels_last Normalize, "
                          f"seed {SEED}", "rounds": a.rounds, "steps": a.steps, "version": ldt_amd.version(),
              "library": os.environ.get("LDT_LIBRARY", "")}
    for k, _ in variants:
        result[k] = {"ms_median": statistics.median(ms[k]), "ms_rounds": ms[k]}
    for k, (rows, rec) in recs.items():
        c = statistics.median(v["color"] for v in stage[k])
        info = {"stage_color_ms_median": c, "stage_resize_ms_median": statistics.median(v["resize"] for v in stage[k]),
                "stage_rounds": stage[k], "entries": n * V, "entries_with_contrast": int(np.count_nonzero(rec["mask"] & 2))}
        if "blur_ww" in rec.dtype.names and rows.shape[-1] == 8:
            blurred = rec["blur_ww"] != 0
            rs = rec["blur_r"][blurred]
            read = sum(3 * region_pixels(SIZE[0], SIZE[1], int(r)) for r in rs)
            written = int(blurred.sum()) * SIZE[0] * SIZE[1] * 3 * 2
            info.update({"entries_with_blur": int(blurred.sum()), "blur_r_counts": np.bincount(rs, minlength=2).tolist(),
                         "blur_bytes_read": read, "blur_bytes_written": written})
        result[k].update(info)
    if a.only is None:
        for k, base in (("blur-1.0-0.1", "color"), ("blur-1.0", "color"), ("blur-1.0", "blur-1.0-off")):
            result[k][f"added_ms_call_vs_{base}"] = result[k]["ms_median"] - result[base]["ms_median"]
            result[k][f"added_ms_stage_vs_{base}"] = (result[k]["stage_color_ms_median"] -
                                                      result[base]["stage_color_ms_median"])
        if torch_error:
            result["uint8+torch"] = {"error": torch_error}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
