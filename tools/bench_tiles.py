#!/usr/bin/env python
"""What ``decode_tiles`` (ldt_decode_tiles, k_resize_tiles) costs against the
composition it replaces, on host cells (an Arrow array), one context and one
stream: bicubic, bfloat16, Normalize, S = 448, thumbnails.

Batches: ``mixed``, 64 rows of 480x640, 640x480, 512x512 and 375x500
(tools/bench_native_resize.py's) under ``DynamicTiles(1, 12, 448)``, and
``c2``, 256 x 512x512 q90 4:2:0 (bench.py's shape) under a fixed (2, 2) grid.

Variants:

  * ``tiles``: the whole ``decode_tiles`` call;
  * ``native x 2 + permute``: the same build's ``decode_native(sizes=canvas)``,
    the per-image ``reshape`` / ``permute`` a user writes today, a second
    ``decode_native(sizes=(S, S))`` for the thumbnails and one ``cat``.

The two tensors are asserted equal before anything is timed. One process, the
variants alternated round by round; ``ms``: HIP events around ``steps`` calls
with profiling off; ``stage_ms``: the per-stage times (LDT_OPT_PROFILE 1) in a
pass of its own. For the tile kernel the bytes it must move at least (the
source's plane bytes once, 1.5 per pixel of a 4:2:0 file, and 2 bytes per
output element), the rate that makes of its stage time and that rate's share
of the HBM peak (``--hbm-gbs``).

    python tools/bench_tiles.py [--rounds 5] [--steps 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lance-distributed-training_amd"))

import numpy as np  # noqa: E402
import pyarrow as pa  # noqa: E402
import torch  # noqa: E402

import ldt_amd  # noqa: E402
from ldt_amd import _lib, synth  # noqa: E402

S = 448


def _compose(cells, grid, kw):
    """Today's way to the same tensor: two native calls and a reshape / permute per image."""
    canvas = ldt_amd.decode_native(cells, sizes=grid * S, **kw)[0]
    thumbs = ldt_amd.decode_native(cells, sizes=np.full_like(grid, S), **kw)[0]
    out = []
    for x, t, (r, c) in zip(canvas, thumbs, grid.tolist()):
        out.append(x.reshape(3, r, S, c, S).permute(1, 3, 0, 2, 4).reshape(r * c, 3, S, S))
        if r * c > 1:
            out.append(t.unsqueeze(0))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--mixed-n", type=int, default=64)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tiles.py measures on the GPU only"
    dev = torch.device("cuda", torch.cuda.current_device())
    shapes = [(480, 640), (640, 480), (512, 512), (375, 500)]
    files = [synth.encode(synth.field(h, w, 7100 + i, 6.0), quality=90) for i, (h, w) in enumerate(shapes)]
    batches = {"mixed": pa.array([files[i % 4] for i in range(args.mixed_n)], pa.binary()),
               "c2": pa.array(synth.q90_512(256, seed=1000)[0], pa.binary())}
    ctx = _lib.Context(dev.index)
    kw = dict(dtype=torch.bfloat16, normalize=True, interpolation="bicubic", ctx=ctx, device=dev)
    units, floor, tiles = {}, {}, {}
    for name, cells in batches.items():
        wh, st = _lib.image_sizes(cells)
        grid = (ldt_amd.DynamicTiles(1, 12, S).grids(wh, st) if name == "mixed"
                else np.full((len(cells), 2), 2, np.int32))
        count = grid[:, 0].astype(np.int64) * grid[:, 1]
        tiles[name] = int((count + (count > 1)).sum())
        floor[name] = 1.5 * int((wh[:, 0].astype(np.int64) * wh[:, 1]).sum()) + 2 * 3 * S * S * tiles[name]
        units[name, "tiles"] = lambda cells=cells, grid=grid: ldt_amd.decode_tiles(cells, grids=grid, tile_size=S, **kw)[0]
        units[name, "native x 2 + permute"] = lambda cells=cells, grid=grid: _compose(cells, grid, kw)
        a, b = units[name, "tiles"](), units[name, "native x 2 + permute"]()
        torch.cuda.synchronize()
        assert a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{name}: the two differ"
    keys = list(units)
    for k in keys:
        for _ in range(2):
            units[k]()
    torch.cuda.synchronize()
    ms, stage = {k: [] for k in keys}, {k: [] for k in keys}
    for r in range(args.rounds):
        for k in keys[r % len(keys):] + keys[:r % len(keys)]:
            ctx.set_option(_lib.OPT_PROFILE, 0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.steps):
                units[k]()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / args.steps)
            ctx.set_option(_lib.OPT_PROFILE, 1)
            ctx.stage_times(reset=True)
            for _ in range(args.steps):
                units[k]()
            torch.cuda.synchronize()
            st = ctx.stage_times(reset=True)
            stage[k].append({s: st[s][0] / args.steps for s in _lib.STAGES})
            ctx.set_option(_lib.OPT_PROFILE, 0)
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    med = {}
    for k in keys:
        sm = {x: round(statistics.median(y[x] for y in stage[k]), 4) for x in _lib.STAGES}
        gbs = floor[k[0]] / 1e9 / (sm["resize"] / 1e3) if k[1] == "tiles" and sm["resize"] > 0 else None
        med[k] = statistics.median(ms[k])
        emit({"case": k[0], "variant": k[1], "n": len(batches[k[0]]), "tiles": tiles[k[0]],
              "ms_per_call": round(med[k], 4), "ms_rounds": [round(x, 4) for x in ms[k]], "stage_ms": sm,
              "resize_floor_mb": round(floor[k[0]] / 1e6, 2), "resize_floor_gbs": None if gbs is None else round(gbs, 1),
              "resize_floor_share_of_hbm_peak": None if gbs is None else round(gbs / args.hbm_gbs, 4)})
    for name in batches:
        base = ms[name, "native x 2 + permute"]
        gain, spread = med[name, "native x 2 + permute"] - med[name, "tiles"], max(base) - min(base)
        emit({"case": name, "gain_ms": round(gain, 4), "composition_min_max_range_ms": round(spread, 4),
              "fused_beats_composition_by_more_than_its_range": bool(gain > spread)})
    emit({"version": ldt_amd.version(), "device": torch.cuda.get_device_name(torch.cuda.current_device()),
          "rounds": args.rounds, "steps": args.steps, "tile_size": S, "library": os.path.basename(os.environ.get("LDT_LIBRARY", "libldt.so"))})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
