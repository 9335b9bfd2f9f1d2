#!/usr/bin/env python
"""What the native decode (ldt_set_native, ``decode_native``) costs: k_emit_rgb
against the identity resize, on resident batches (cells in HBM), one context
and one stream.

Cases, uint8 NCHW:

  * ``c2``: 256 x 512x512 q90 4:2:0 (bench.py's shape): the native call against
    the same build's ``size=(512, 512), dtype=torch.uint8`` call, whose output
    bytes are the same; that equality is asserted before anything is timed;
  * ``big``: 2048x1536 q90 4:2:0 rows (``--big-n`` of them, 64 by default, cut
    from 8 distinct files, so each file is decoded eight times per call: host
    time to synthesise them sets the number; the repeats may help the Huffman
    stage's caches, the emit stage reads planes that are distinct memory),
    native only: no other call serves that shape.

One process, the variants interleaved round by round (the order rotates), each
measured two ways per round: ``ms``, HIP events around ``steps`` calls with
profiling off, and ``stage_ms``, the per-stage times (LDT_OPT_PROFILE 1) in a
pass of its own. For the emit stage the bytes it must move at least (the plane
bytes it reads once, 1.5 per pixel of a 4:2:0 file, and the 3 output bytes per
pixel), the rate that makes of its time and that rate's share of the HBM peak
(``--hbm-gbs``, 8000 for MI355X).

Prints one JSON line per (case, variant), then a summary line.

    python tools/bench_native.py [--rounds 5] [--steps 30] [--out FILE]
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


def _native_unit(ctx, b, flat, lbl, offsets, status):
    """One native call on the resident batch: armed and made as decode_native does it."""
    def unit():
        with ctx.lock:
            ctx.arm(ctx._size, ctx._filter, "uint8", "contiguous", native=offsets)
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
    ap.add_argument("--big-n", type=int, default=64)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_native.py measures on the GPU only"
    dev = torch.device("cuda", torch.cuda.current_device())
    cells, labels = synth.q90_512(256, seed=1000)
    files = [synth.encode(synth.field(1536, 2048, 7000 + i, 6.0), quality=90) for i in range(8)]
    batches = {"c2": ldt_amd.ResidentBatch(cells, labels, device=dev),
               "big": ldt_amd.ResidentBatch([files[i % 8] for i in range(args.big_n)], list(range(args.big_n)), device=dev)}
    ctx = _lib.Context(dev.index)
    units, pixels = {}, {}
    for name, b in batches.items():
        wh, st = b.image_sizes()
        hw, offsets = _lib.native_layout(wh, st)
        pixels[name] = int(offsets[-1]) // 3
        flat = torch.empty((int(offsets[-1]),), dtype=torch.uint8, device=dev)
        lbl = torch.empty((b.n,), dtype=torch.int64, device=dev)
        units[name, "native"] = _native_unit(ctx, b, flat, lbl, offsets, np.zeros(b.n, np.int32))
        if name == "c2":
            out = T._empty_image(b.n, (512, 512), "uint8", "contiguous", dev)
            units[name, "identity resize"] = lambda b=b, out=out, lbl=lbl: b.decode(out, lbl, ctx=ctx, size=(512, 512),
                                                                                    dtype=torch.uint8)
            # the same bytes, before anything is timed (statuses are read: LDT_OPT_SYNC_STATUS is still on)
            units[name, "native"]()
            units[name, "identity resize"]()
            torch.cuda.synchronize()
            assert torch.equal(flat.view(b.n, 3, 512, 512), out), "native and the identity resize differ"
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
            steps = args.steps if k[0] == "c2" else max(3, args.steps // 4)
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
        floor = pixels[k[0]] * 4.5  # 1.5 plane bytes read and 3 bytes stored per pixel
        gbs = floor / 1e9 / (med["resize"] / 1e3) if med["resize"] > 0 else None
        rows.append({"case": k[0], "variant": k[1], "n": batches[k[0]].n, "ms_per_call": round(statistics.median(ms[k]), 4),
                     "ms_rounds": [round(x, 4) for x in ms[k]],
                     "images_per_s": round(batches[k[0]].n / statistics.median(ms[k]) * 1000), "stage_ms": med,
                     "store_floor_mb": round(floor / 1e6, 2), "store_floor_gbs": None if gbs is None else round(gbs, 1),
                     "store_floor_share_of_hbm_peak": None if gbs is None else round(gbs / args.hbm_gbs, 4)})
        emit(rows[-1])
    emit({"summary": {f"{r['case']}: {r['variant']}": [r["ms_per_call"], r["stage_ms"]["resize"], r["store_floor_gbs"]]
                      for r in rows},
          "columns": ["ms_per_call", "resize_stage_ms", "store_floor_gbs"], "version": ldt_amd.version(),
          "device": torch.cuda.get_device_name(torch.cuda.current_device()), "rounds": args.rounds})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
