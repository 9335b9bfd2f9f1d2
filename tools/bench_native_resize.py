#!/usr/bin/env python
"""What ``decode_native(sizes=)`` (ldt_set_native_sizes, k_resize_ragged) costs,
on resident batches (cells in HBM), one context and one stream, uint8 NCHW.

Batches:

  * ``c2``: 256 x 512x512 q90 4:2:0 (bench.py's shape) at
    ``ResizeShortestEdge(256)``: every row 256 x 256;
  * ``mixed``: 64 rows of 480x640, 640x480, 512x512 and 375x500 (h x w) at
    ``ResizeShortestEdge(800, max_size=1333)``: 800 x 1066, 1066 x 800,
    800 x 800, 800 x 1066.

Variants:

  * ``sizes``: the new call;
  * ``native + interpolate``: the plain native call followed by the loop a user
    writes today, one ``torch.nn.functional.interpolate(mode="bilinear",
    antialias=True)`` per image on the float image (not Pillow's arithmetic:
    it is timed, not compared);
  * ``fixed size`` (c2 only, whose rows are all square): the same build's
    ``size=(256, 256), dtype=torch.uint8`` call, which is what a
    ``Letterbox(align="topleft")`` call launches for square images; its bytes
    are asserted equal to the new call's before anything is timed. The mixed
    batch's sizes exceed LDT_MAX_OUT, so no such call serves it.

One process, the variants interleaved round by round (the order rotates);
``ms``: HIP events around ``steps`` calls with profiling off; ``stage_ms``: the
per-stage times (LDT_OPT_PROFILE 1) in a pass of its own. For the resize stage
the bytes it must move at least (the source's plane bytes read once, 1.5 per
source pixel of a 4:2:0 file, and 3 output bytes per output pixel), the rate
that makes of its time and that rate's share of the HBM peak (``--hbm-gbs``).
``--tr``: the tile rows the library under LDT_LIBRARY was built with
(LDT_RAGGED_TR), recorded with the results.

    python tools/bench_native_resize.py [--rounds 5] [--steps 30] [--tr 16] [--out FILE]
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


def _native_unit(ctx, b, flat, lbl, offsets, status, sizes=None):
    """One native call on the resident batch: armed and made as decode_native does it."""
    def unit():
        with ctx.lock:
            ctx.arm(ctx._size, "bilinear", "uint8", "contiguous", native=offsets, native_sizes=sizes)
            rc = ctx.lib.ldt_decode_batch_resident(ctx.handle, b.host.ctypes.data, b.dev.data_ptr(),
                                                   b.offsets.ctypes.data, b.n, b.labels.ctypes.data, flat.data_ptr(),
                                                   lbl.data_ptr(), None, torch.cuda.current_stream().cuda_stream,
                                                   status.ctypes.data)
        ctx.check(rc, "ldt_decode_batch_resident")
    return unit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--mixed-n", type=int, default=64)
    ap.add_argument("--tr", type=int, default=16)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_native_resize.py measures on the GPU only"
    dev = torch.device("cuda", torch.cuda.current_device())
    cells, labels = synth.q90_512(256, seed=1000)
    shapes = [(480, 640), (640, 480), (512, 512), (375, 500)]
    files = [synth.encode(synth.field(h, w, 7100 + i, 6.0), quality=90) for i, (h, w) in enumerate(shapes)]
    batches = {"c2": (ldt_amd.ResidentBatch(cells, labels, device=dev), ldt_amd.ResizeShortestEdge(256)),
               "mixed": (ldt_amd.ResidentBatch([files[i % 4] for i in range(args.mixed_n)], list(range(args.mixed_n)),
                                               device=dev), ldt_amd.ResizeShortestEdge(800, max_size=1333))}
    ctx = _lib.Context(dev.index)
    units, floor = {}, {}
    for name, (b, helper) in batches.items():
        wh, st = b.image_sizes()
        sizes = helper.sizes(wh, st)
        hw, off = _lib.native_layout(wh, st, None, sizes)
        hw0, off0 = _lib.native_layout(wh, st)
        floor[name] = 1.5 * int(off0[-1]) // 3 + int(off[-1])
        flat = torch.empty((int(off[-1]),), dtype=torch.uint8, device=dev)
        flat0 = torch.empty((int(off0[-1]),), dtype=torch.uint8, device=dev)
        lbl = torch.empty((b.n,), dtype=torch.int64, device=dev)
        status = np.zeros(b.n, np.int32)
        units[name, "sizes"] = _native_unit(ctx, b, flat, lbl, off, status, sizes)
        plain = _native_unit(ctx, b, flat0, lbl, off0, status)
        views = [flat0[a:z].view(1, 3, h, w) for (h, w), a, z in zip(hw0.tolist(), off0[:-1].tolist(), off0[1:].tolist())]

        def loop(plain=plain, views=views, sizes=sizes.tolist()):
            plain()
            return [torch.nn.functional.interpolate(v.float(), size=s, mode="bilinear", antialias=True)
                    .round_().clamp_(0, 255).to(torch.uint8) for v, s in zip(views, sizes)]

        units[name, "native + interpolate"] = loop
        if name == "c2":
            out = T._empty_image(b.n, (256, 256), "uint8", "contiguous", dev)
            units[name, "fixed size"] = lambda b=b, out=out, lbl=lbl: b.decode(out, lbl, ctx=ctx, size=(256, 256),
                                                                               dtype=torch.uint8)
            units[name, "sizes"]()
            units[name, "fixed size"]()
            torch.cuda.synchronize()
            assert torch.equal(flat.view(b.n, 3, 256, 256), out), "the ragged and the fixed-size resize differ"
    ctx.set_option(_lib.OPT_SYNC_STATUS, 0)
    keys = list(units)
    for k in keys:
        for _ in range(3):
            units[k]()
    torch.cuda.synchronize()
    ms = {k: [] for k in keys}
    stage = {k: [] for k in keys}
    for r in range(args.rounds):
        for k in keys[r % len(keys):] + keys[:r % len(keys)]:
            steps = args.steps if k[0] == "c2" else max(3, args.steps // 3)
            ctx.set_option(_lib.OPT_PROFILE, 0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(steps):
                units[k]()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / steps)
            ctx.set_option(_lib.OPT_PROFILE, 1)
            ctx.stage_times(reset=True)
            for _ in range(steps):
                units[k]()
            torch.cuda.synchronize()
            st = ctx.stage_times(reset=True)
            stage[k].append({s: st[s][0] / steps for s in _lib.STAGES})
            ctx.set_option(_lib.OPT_PROFILE, 0)
    lines = []

    def emit(obj):
        s = json.dumps(obj)
        print(s, flush=True)
        lines.append(s)

    rows = []
    for k in keys:
        med = {x: round(statistics.median(y[x] for y in stage[k]), 4) for x in _lib.STAGES}
        gbs = floor[k[0]] / 1e9 / (med["resize"] / 1e3) if k[1] == "sizes" and med["resize"] > 0 else None
        rows.append({"case": k[0], "variant": k[1], "n": batches[k[0]][0].n, "tile_rows": args.tr,
                     "ms_per_call": round(statistics.median(ms[k]), 4), "ms_rounds": [round(x, 4) for x in ms[k]],
                     "stage_ms": med, "resize_floor_mb": round(floor[k[0]] / 1e6, 2),
                     "resize_floor_gbs": None if gbs is None else round(gbs, 1),
                     "resize_floor_share_of_hbm_peak": None if gbs is None else round(gbs / args.hbm_gbs, 4)})
        emit(rows[-1])
    emit({"summary": {f"{r['case']}: {r['variant']}": [r["ms_per_call"], r["stage_ms"]["resize"], r["resize_floor_gbs"]]
                      for r in rows},
          "columns": ["ms_per_call", "resize_stage_ms", "resize_floor_gbs"], "tile_rows": args.tr,
          "version": ldt_amd.version(), "device": torch.cuda.get_device_name(torch.cuda.current_device()),
          "rounds": args.rounds})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
