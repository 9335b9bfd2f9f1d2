#!/usr/bin/env python
"""Resize stage time and decode rate per output format (dtype x memory_format).

One process, the eight formats interleaved round by round (the order rotates
each round), every figure against float32 / contiguous of the same build:

  * c2: the c2-shaped resident batch (256 x 512x512 q90 4:2:0 -> 224 x 224),
    plain (the band kernel), with window=ResizeCenterCrop(256) and with
    interpolation="bicubic" (both the streaming kernel);
  * c5: the raw batch (1024 x 1024x1024 uint8 HWC in HBM -> 224 x 224 +
    Normalize; uint8 output: without the Normalize).

Per format: the resize stage's time per batch (LDT_STAGE_RESIZE from
stage_times, HIP events on the decode stream), the whole-decode rate (host
clock around `steps` calls ending in a device synchronise), and the time of
the conversion pass the format saves, `.to(dtype).contiguous(memory_format=)`
on the float32 result (HIP events). Prints one JSON line per (case, format)
with the median over the rounds and every round's value, then a summary line.

    python tools/format_bench.py [--rounds 5] [--steps 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lance-distributed-training_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ldt_amd  # noqa: E402
from ldt_amd import _lib, synth  # noqa: E402
from ldt_amd import transforms as T  # noqa: E402

DTYPES = ("float32", "float16", "bfloat16", "uint8")
LAYOUTS = ("contiguous", "channels_last")
FORMATS = [(d, m) for d in DTYPES for m in LAYOUTS]
SIZE = (224, 224)


def _events(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--c5-batch", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "format_bench.py measures on the GPU only"
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = []

    def emit(obj):
        s = json.dumps(obj)
        print(s, flush=True)
        lines.append(s)

    ctx = _lib.Context(dev.index)
    ctx.set_option(_lib.OPT_PROFILE, 1)
    ctx.set_option(_lib.OPT_SYNC_STATUS, 0)

    cells, labels = synth.q90_512(256, seed=1000)
    res = ldt_amd.ResidentBatch(cells, labels, device=dev)
    window = ldt_amd.ResizeCenterCrop(256).sample(*res.image_sizes(), SIZE)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    raw = torch.randint(0, 256, (args.c5_batch, 1024, 1024, 3), dtype=torch.uint8, device=dev, generator=g)

    def c2(dtype, mf, **kw):
        out = T._empty_image(res.n, SIZE, dtype, mf, dev)
        lbl = torch.empty((res.n,), dtype=torch.int64, device=dev)
        return (lambda: res.decode(out, lbl, ctx=ctx, size=SIZE, dtype=dtype, memory_format=mf, **kw)), res.n, out

    def c5(dtype, mf):
        # resize_raw allocates its output, as bench.py's c5 step does; on the device's shared context
        norm = None if dtype == "uint8" else True
        return (lambda: ldt_amd.resize_raw(raw, 1024, 1024, device=dev, normalize=norm, size=SIZE, dtype=dtype,
                                           memory_format=mf)), raw.shape[0], None

    shared = _lib.get_context(dev.index)
    shared.set_option(_lib.OPT_PROFILE, 1)
    cases = [("c2", lambda d, m: c2(d, m), ctx),
             ("c2 window=ResizeCenterCrop(256)", lambda d, m: c2(d, m, windows=window), ctx),
             ("c2 bicubic", lambda d, m: c2(d, m, interpolation="bicubic"), ctx),
             ("c5 raw", c5, shared)]
    summary = {}
    for name, make, pctx in cases:
        runs = {f: make(*f) for f in FORMATS}
        stage = {f: [] for f in FORMATS}
        rate = {f: [] for f in FORMATS}
        for f in FORMATS:  # warm every shape and kernel of the timed window
            for _ in range(3):
                runs[f][0]()
        torch.cuda.synchronize()
        steps = args.steps if name != "c5 raw" else max(4, args.steps // 2)
        for r in range(args.rounds):
            order = FORMATS[r % len(FORMATS):] + FORMATS[:r % len(FORMATS)]
            for f in order:
                fn, n, _ = runs[f]
                pctx.stage_times(reset=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    fn()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                ms, cnt = pctx.stage_times(reset=True)["resize"]
                stage[f].append(ms / max(cnt, 1))
                rate[f].append(n * steps / dt)
        # the conversion pass each format saves, on the float32 result
        ref = runs[("float32", "contiguous")]
        ref32 = ref[2] if ref[2] is not None else ref[0]()
        torch.cuda.synchronize()
        base = statistics.median(stage[("float32", "contiguous")])
        for f in FORMATS:
            d, m = f
            conv = None
            if f != ("float32", "contiguous"):
                td, tm = T._TORCH_DTYPES[d], (torch.channels_last if m == "channels_last" else torch.contiguous_format)
                if d == "uint8":
                    continue_fn = lambda: ref32.mul(255).round_().to(td).contiguous(memory_format=tm)  # noqa: E731
                else:
                    continue_fn = lambda: ref32.to(td).contiguous(memory_format=tm)  # noqa: E731
                for _ in range(3):
                    continue_fn()
                conv = statistics.median(_events(continue_fn, 10) for _ in range(args.rounds))
            med = statistics.median(stage[f])
            row = {"case": name, "dtype": d, "memory_format": m, "resize_ms": round(med, 4),
                   "resize_ms_rounds": [round(v, 4) for v in stage[f]], "vs_float32_contiguous": round(med / base, 3),
                   "img_per_s": round(statistics.median(rate[f])), "img_per_s_rounds": [round(v) for v in rate[f]],
                   "conversion_pass_ms": None if conv is None else round(conv, 4), "steps": steps, "batch": runs[f][1]}
            emit(row)
            summary.setdefault(name, {})[f"{d}/{m}"] = [row["resize_ms"], row["vs_float32_contiguous"],
                                                        row["img_per_s"], row["conversion_pass_ms"]]
        del runs
    emit({"summary": summary, "columns": ["resize_ms", "vs_float32_contiguous", "img_per_s", "conversion_pass_ms"],
          "version": ldt_amd.version(), "device": torch.cuda.get_device_name(dev), "rounds": args.rounds})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
