#!/usr/bin/env python
"""What ``views=`` saves: V views of every image from one decode against V
single-view calls, on the c2-shaped resident batch (256 x 512x512 q90 4:2:0,
cells in HBM, output 224 x 224).

One process, the variants interleaved round by round (the order rotates each
round), each measured three ways per round:

  * ``ms``: HIP events around ``steps`` units on one context and one stream
    (a unit = everything that produces the V * 256 output images: one
    ``views=V`` call, or V single-view calls), profiling off;
  * ``stage_ms``: the per-stage times of a unit (``ldt_stage_times``: HIP
    events at the stage boundaries, LDT_OPT_PROFILE 1), in a pass of its own;
  * ``units_per_s``: a ``DecodePipeline(depth=3)`` fed the same units, host
    clock around a window that ends in a device synchronise: the overlapped
    rate a loader sees.

Cases: two random views (``RandomResizedCropFlip()`` boxes from a fixed seed),
five-crop and ten-crop (``ResizeFiveCrop(256, ten=...)``). Variants per case:
``views`` (one call, grid order 0: an image's views adjacent), ``views-order1``
(view-major launch order, LDT_OPT_VIEW_ORDER 1) and ``calls`` (V single-view
calls with the same boxes and windows). ``--parent-lib PATH`` measures the
variants once more in a child process that loads that libldt.so (a build of
the parent commit: the yardstick), before and after the main rounds: every
variant but the size list (``--parent-mode uniform``, the default), or the
``calls`` variants alone for a library that predates ``views=``.

The multi-crop case (DINO / SwAV / iBOT: two global views at 224 x 224 and six
local views at 96 x 96, boxes from ``RandomResizedCropFlip(scale=[(0.4, 1.0)] *
2 + [(0.05, 0.4)] * 6)`` with the fixed seed) has its own variants: ``sizes``
(one call with the size list: one decode), and ``calls`` (two ``views=`` calls,
2 at 224 and 6 at 96, with the same boxes: two decodes), which the parent
library runs too.

Prints one JSON line per (case, variant) with the median over the rounds and
every round's value, then a summary line.

    python tools/bench_views.py [--rounds 5] [--steps 40] [--parent-lib PATH] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lance-distributed-training_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ldt_amd  # noqa: E402
from ldt_amd import _lib, synth  # noqa: E402
from ldt_amd import transforms as T  # noqa: E402

SIZE = (224, 224)
SEED = 1234
DINO = "multi-crop 2x224 + 6x96"
DINO_SIZES = [(224, 224)] * 2 + [(96, 96)] * 6
DINO_SCALES = [(0.4, 1.0)] * 2 + [(0.05, 0.4)] * 6


def _cases(res):
    """name -> (V, crops [n, V, 5] or None, windows [n, V, 4] or None)."""
    wh, st = res.image_sizes()
    two = ldt_amd.RandomResizedCropFlip(generator=torch.Generator().manual_seed(SEED)).sample(wh, st, views=2)
    five, ten = ldt_amd.ResizeFiveCrop(256), ldt_amd.ResizeFiveCrop(256, ten=True)
    return {"two random views": (2, two, None),
            "five-crop": (5, None, five.sample(wh, st, SIZE)),
            "ten-crop": (10, ten.boxes(wh, st), ten.sample(wh, st, SIZE))}


def _col(a, v):
    return None if a is None else np.ascontiguousarray(a[:, v])


def _dino_units(res, dev, with_sizes):
    """The multi-crop case: ``calls`` = two views= calls (two decodes), ``sizes``
    = one call with the size list (one decode). The pipelined units take the
    list of their pipelines: one per output shape."""
    wh, st = res.image_sizes()
    boxes = ldt_amd.RandomResizedCropFlip(scale=DINO_SCALES, generator=torch.Generator().manual_seed(SEED)).sample(
        wh, st, views=8)
    big, small = np.ascontiguousarray(boxes[:, :2]), np.ascontiguousarray(boxes[:, 2:])
    g = T._empty_image(res.n, (224, 224), "float32", "contiguous", dev, 2)
    l = T._empty_image(res.n, (96, 96), "float32", "contiguous", dev, 6)
    lbl = torch.empty((res.n,), dtype=torch.int64, device=dev)

    def calls(ctx):
        res.decode(g, lbl, ctx=ctx, size=(224, 224), crops=big, views=2)
        res.decode(l, lbl, ctx=ctx, size=(96, 96), crops=small, views=6)

    def pcalls(pipes):
        pipes[0].decode(res, crops=big)
        pipes[1].decode(res, crops=small)

    out = {(DINO, "calls"): (calls, 8, pcalls, None, [((224, 224), 2), ((96, 96), 6)])}
    if with_sizes:
        sizes = _lib.check_view_sizes(DINO_SIZES)
        flat = T._empty_image(res.n, sizes, "float32", "contiguous", dev, 8)

        def sized(ctx):
            res.decode(flat, lbl, ctx=ctx, size=sizes, crops=boxes)

        def psized(pipes):
            pipes[0].decode(res, crops=boxes)

        out[(DINO, "sizes")] = (sized, 8, psized, 0, [(sizes, 8)])
    return out


def _units(res, dev, with_views, with_sizes):
    """(case, variant) -> (unit(ctx), V, pipeline unit(pipes), grid order or
    None, [(size, views) of each pipeline the unit needs])."""
    out = {}
    for name, (V, crops, windows) in _cases(res).items():
        one = T._empty_image(res.n, SIZE, "float32", "contiguous", dev)
        lbl = torch.empty((res.n,), dtype=torch.int64, device=dev)

        def calls(ctx, V=V, crops=crops, windows=windows, one=one, lbl=lbl):
            for v in range(V):
                res.decode(one, lbl, ctx=ctx, size=SIZE, crops=_col(crops, v), windows=_col(windows, v))

        def pcalls(pipes, V=V, crops=crops, windows=windows):
            for v in range(V):
                pipes[0].decode(res, crops=_col(crops, v), windows=_col(windows, v))

        out[(name, "calls")] = (calls, V, pcalls, None, [(SIZE, None)])
        if not with_views:
            continue
        many = T._empty_image(res.n, SIZE, "float32", "contiguous", dev, V)

        def views(ctx, V=V, crops=crops, windows=windows, many=many, lbl=lbl):
            res.decode(many, lbl, ctx=ctx, size=SIZE, crops=crops, windows=windows, views=V)

        def pviews(pipes, crops=crops, windows=windows):
            pipes[0].decode(res, crops=crops, windows=windows)

        out[(name, "views")] = (views, V, pviews, 0, [(SIZE, V)])
        out[(name, "views-order1")] = (views, V, pviews, 1, [(SIZE, V)])
    out.update(_dino_units(res, dev, with_sizes))
    return out


def _measure(args, with_views, tag, with_sizes=None):
    with_sizes = with_views if with_sizes is None else with_sizes
    dev = torch.device("cuda", torch.cuda.current_device())
    cells, labels = synth.q90_512(256, seed=1000)
    res = ldt_amd.ResidentBatch(cells, labels, device=dev)
    ctx = _lib.Context(dev.index)
    ctx.set_option(_lib.OPT_SYNC_STATUS, 0)
    units = _units(res, dev, with_views, with_sizes)
    # one pipeline per output shape: the variants that share it run one after another
    by_views = {}
    pipes = {}
    for key, (_, _, _, _, specs) in units.items():
        for size, pv in specs:
            if (size, pv) not in by_views:
                by_views[(size, pv)] = T.DecodePipeline(depth=3, device=dev, size=size, views=pv)
        pipes[key] = [by_views[spec] for spec in specs]
    keys = list(units)
    ms = {k: [] for k in keys}
    stage = {k: [] for k in keys}
    rate = {k: [] for k in keys}

    def set_order(order):
        if with_views:
            ctx.set_option(_lib.OPT_VIEW_ORDER, order or 0)
            for p in by_views.values():
                p.set_option(_lib.OPT_VIEW_ORDER, order or 0)

    for k in keys:  # warm every shape and kernel of the timed windows
        set_order(units[k][3])
        for _ in range(3):
            units[k][0](ctx)
            units[k][2](pipes[k])
        for p in pipes[k]:
            p.check()
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for k in keys[r % len(keys):] + keys[:r % len(keys)]:
            unit, V, punit, order, _ = units[k]
            set_order(order)
            ctx.set_option(_lib.OPT_PROFILE, 0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.steps):
                unit(ctx)
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / args.steps)
            ctx.set_option(_lib.OPT_PROFILE, 1)
            ctx.stage_times(reset=True)
            for _ in range(args.steps):
                unit(ctx)
            torch.cuda.synchronize()
            st = ctx.stage_times(reset=True)
            stage[k].append({s: st[s][0] / args.steps for s in _lib.STAGES})
            ctx.set_option(_lib.OPT_PROFILE, 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                punit(pipes[k])
            torch.cuda.synchronize()
            rate[k].append(args.steps / (time.perf_counter() - t0))
            for p in pipes[k]:
                p.check()
    rows = []
    for k in keys:
        V = units[k][1]
        med_stage = {s: round(statistics.median(x[s] for x in stage[k]), 4) for s in _lib.STAGES}
        rows.append({"build": tag, "case": k[0], "variant": k[1], "views": V, "images_per_unit": V * res.n,
                     "ms_per_unit": round(statistics.median(ms[k]), 4), "ms_rounds": [round(v, 4) for v in ms[k]],
                     "stage_ms_per_unit": med_stage,
                     "decode_stages_ms": round(sum(med_stage[s] for s in ("h2d", "destuff", "huffman", "idct")), 4),
                     "pipelined_units_per_s": round(statistics.median(rate[k]), 1),
                     "pipelined_images_per_s": round(statistics.median(rate[k]) * V * res.n),
                     "pipelined_rounds": [round(v, 1) for v in rate[k]], "steps": args.steps})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--parent-lib", default=None, help="a libldt.so built from the parent commit (the yardstick)")
    ap.add_argument("--calls-only", default=None, metavar="TAG", help="(child) only the single-view variants")
    ap.add_argument("--uniform-only", default=None, metavar="TAG",
                    help="(child) every variant but the size list: for a library with views= and without size lists")
    ap.add_argument("--parent-mode", default="uniform", choices=["calls", "uniform"],
                    help="what the parent library runs: 'uniform' (it has views=: its views variants are the "
                         "yardstick of this build's uniform cases) or 'calls' (it predates views=)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_views.py measures on the GPU only"
    if args.calls_only or args.uniform_only:
        for row in _measure(args, bool(args.uniform_only), args.calls_only or args.uniform_only, False):
            print(json.dumps(row), flush=True)
        return
    lines = []

    def emit(obj):
        s = json.dumps(obj)
        print(s, flush=True)
        lines.append(s)

    def parent(tag):
        if not args.parent_lib:
            return []
        # a fresh child process: one process loads one libldt.so
        r = subprocess.run([sys.executable, os.path.abspath(__file__), f"--{args.parent_mode}-only", tag, "--rounds", str(args.rounds),
                            "--steps", str(args.steps)], env=dict(os.environ, LDT_LIBRARY=os.path.abspath(args.parent_lib)),
                           capture_output=True, text=True, timeout=600, check=True)
        return [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]

    rows = parent("parent (before)")
    rows += _measure(args, True, "this build")
    rows += parent("parent (after)")
    for row in rows:
        emit(row)
    summary = {}
    for row in rows:
        summary.setdefault(row["case"], {})[f"{row['build']}: {row['variant']}"] = [
            row["ms_per_unit"], row["decode_stages_ms"], row["stage_ms_per_unit"]["resize"], row["pipelined_images_per_s"]]
    emit({"summary": summary, "columns": ["ms_per_unit", "decode_stages_ms", "resize_ms", "pipelined_images_per_s"],
          "batch": 256, "size": list(SIZE), "seed": SEED, "version": ldt_amd.version(),
          "device": torch.cuda.get_device_name(torch.cuda.current_device()), "rounds": args.rounds})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
