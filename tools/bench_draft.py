#!/usr/bin/env python
"""What ``draft=`` saves: the DCT-domain 1/2, 1/4, 1/8 decode against the full
decode, on resident batches (cells in HBM), one context and one stream.

Cases, each -> 224 x 224 float32:

  * ``c2``: 256 x 512x512 q90 4:2:0 (bench.py's shape) at scales 1 and 2;
  * ``big``: 2048x1536 q90 4:2:0 files (``--big-n`` rows, 64 by default, cut
    from 8 distinct files: host time to synthesise them, not HBM, sets the
    number) at scales 1, 2, 4 and 8;
  * ``recipe``: ``draft=Draft((256, 256)), window=ResizeCenterCrop(256)`` on
    both batches against the same window without a draft.

One process, the variants interleaved round by round (the order rotates), each
measured two ways per round: ``ms``, HIP events around ``steps`` calls with
profiling off, and ``stage_ms``, the per-stage times (LDT_OPT_PROFILE 1) in a
pass of its own. For the IDCT stage the bytes it must move at least (the plane
bytes written, from the planner's rule restated here, plus one 4-byte record
per block; the coefficient groups it reads come on top and are not counted)
and that floor's share of the HBM peak (``--hbm-gbs``, 8000 for MI355X).

``--parent-lib PATH`` measures the default path (``c2`` at scale 1, no draft
argument at all) once more in child processes that load that libldt.so (a
build of the parent commit), before and after the main rounds.

Prints one JSON line per (case, variant), then a summary line.

    python tools/bench_draft.py [--rounds 5] [--steps 30] [--parent-lib PATH] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lance-distributed-training_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ldt_amd  # noqa: E402
from ldt_amd import _lib, synth  # noqa: E402
from ldt_amd import transforms as T  # noqa: E402

SIZE = (224, 224)


def _idct_floor_bytes(wh, scales):
    """Plane bytes written + block records read by the IDCT stage for 4:2:0 files."""
    total = 0
    for (w, h), s in zip(wh, scales):
        mcux, mcuy, min_s = -(-w // 16), -(-h // 16), 8 // s
        for (ch, cv) in ((2, 2), (1, 1), (1, 1)):
            sc = min_s
            while sc < 8 and (2 * min_s) % (ch * sc * 2) == 0 and (2 * min_s) % (cv * sc * 2) == 0:
                sc *= 2
            total += (mcux * ch * sc) * (mcuy * cv * sc) + 4 * mcux * ch * mcuy * cv
    return total


def _batches(args, only_c2):
    dev = torch.device("cuda", torch.cuda.current_device())
    cells, labels = synth.q90_512(256, seed=1000)
    out = {"c2": ldt_amd.ResidentBatch(cells, labels, device=dev)}
    if not only_c2:
        files = [synth.encode(synth.field(1536, 2048, 7000 + i, 6.0), quality=90) for i in range(8)]
        n = args.big_n
        out["big"] = ldt_amd.ResidentBatch([files[i % 8] for i in range(n)], list(range(n)), device=dev)
    return dev, out


def _variants(batches, parent_only):
    """(case, variant) -> (batch name, decode kwargs, scales per row or None)."""
    v = {("c2", "no draft"): ("c2", {}, None)}
    if parent_only:
        return v
    v[("c2", "scale 1")] = ("c2", {"drafts": np.ones(256, np.int32)}, None)
    v[("c2", "scale 2")] = ("c2", {"drafts": np.full(256, 2, np.int32)}, 2)
    # a mixed batch: one drafted row sends all 256 through k_idct_scaled, 255 of them through its ISLOW body
    one = np.ones(256, np.int32)
    one[0] = 2
    v[("c2", "one row at scale 2")] = ("c2", {"drafts": one}, "mixed")
    n = batches["big"].n
    v[("big", "no draft")] = ("big", {}, None)
    for s in (2, 4, 8):
        v[("big", f"scale {s}")] = ("big", {"drafts": np.full(n, s, np.int32)}, s)
    win = ldt_amd.ResizeCenterCrop(256)
    for name in ("c2", "big"):
        v[("recipe " + name, "window only")] = (name, {"windows": win}, None)
        v[("recipe " + name, "Draft((256, 256)) + window")] = (name, {"windows": win, "drafts": ldt_amd.Draft((256, 256))},
                                                               "draft")
    return v


def _measure(args, tag, parent_only=False):
    dev, batches = _batches(args, parent_only)
    ctx = _lib.Context(dev.index)
    ctx.set_option(_lib.OPT_SYNC_STATUS, 0)
    variants = _variants(batches, parent_only)
    keys = list(variants)
    outs = {name: (T._empty_image(b.n, SIZE, "float32", "contiguous", dev), torch.empty((b.n,), dtype=torch.int64, device=dev))
            for name, b in batches.items()}

    def unit(k):
        name, kw, _ = variants[k]
        batches[name].decode(outs[name][0], outs[name][1], ctx=ctx, size=SIZE, **kw)

    for k in keys:
        for _ in range(3):
            unit(k)
    torch.cuda.synchronize()
    ms = {k: [] for k in keys}
    stage = {k: [] for k in keys}
    for r in range(args.rounds):
        for k in keys[r % len(keys):] + keys[:r % len(keys)]:
            steps = args.steps if variants[k][0] == "c2" else max(3, args.steps // 4)
            ctx.set_option(_lib.OPT_PROFILE, 0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(steps):
                unit(k)
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / steps)
            ctx.set_option(_lib.OPT_PROFILE, 1)
            ctx.stage_times(reset=True)
            for _ in range(steps):
                unit(k)
            torch.cuda.synchronize()
            st = ctx.stage_times(reset=True)
            stage[k].append({s: st[s][0] / steps for s in _lib.STAGES})
            ctx.set_option(_lib.OPT_PROFILE, 0)
    rows = []
    for k in keys:
        name, kw, s = variants[k]
        b = batches[name]
        wh, st = b.image_sizes()
        scales = np.ones(b.n, np.int32) if s is None or "drafts" not in kw else \
            (kw["drafts"].sample(wh, st) if s == "draft" else kw["drafts"])
        med = {x: round(statistics.median(y[x] for y in stage[k]), 4) for x in _lib.STAGES}
        floor = _idct_floor_bytes(wh.tolist(), scales.tolist())
        rows.append({"build": tag, "case": k[0], "variant": k[1], "n": b.n, "scales": sorted(set(scales.tolist())),
                     "ms_per_call": round(statistics.median(ms[k]), 4), "ms_rounds": [round(x, 4) for x in ms[k]],
                     "images_per_s": round(b.n / statistics.median(ms[k]) * 1000), "stage_ms": med,
                     "idct_floor_mb": round(floor / 1e6, 2),
                     "idct_floor_share_of_hbm_peak": round(floor / 1e9 / (med["idct"] / 1e3) / args.hbm_gbs, 4)
                     if med["idct"] > 0 else None})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--big-n", type=int, default=64)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--parent-lib", default=None, help="a libldt.so built from the parent commit (the yardstick)")
    ap.add_argument("--parent-only", default=None, metavar="TAG", help="(child) the default path alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_draft.py measures on the GPU only"
    if args.parent_only:
        for row in _measure(args, args.parent_only, True):
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
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-only", tag, "--rounds", str(args.rounds),
                            "--steps", str(args.steps)], env=dict(os.environ, LDT_LIBRARY=os.path.abspath(args.parent_lib)),
                           capture_output=True, text=True, timeout=600, check=True)
        return [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]

    rows = parent("parent (before)")
    rows += _measure(args, "this build")
    rows += parent("parent (after)")
    for row in rows:
        emit(row)
    emit({"summary": {f"{r['build']}: {r['case']}: {r['variant']}": [r["ms_per_call"], r["stage_ms"]["idct"],
                                                                    r["stage_ms"]["resize"], r["images_per_s"]]
                      for r in rows},
          "columns": ["ms_per_call", "idct_ms", "resize_ms", "images_per_s"], "size": list(SIZE),
          "version": ldt_amd.version(), "device": torch.cuda.get_device_name(torch.cuda.current_device()),
          "rounds": args.rounds})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
