"""Measurement (not a test): the c2 batch (256 x 512^2 q90, bench.py's
generator) decoded resident at output sizes 128, 160, 192, 224, 256 and 384,
and 224 through LDT_OPT_RESIZE_IMPL 3 (the generic-width band kernel) beside
the default (the 224 x 224 instantiation). Per size: images/s of the whole
decode (host clock around a synchronised loop) and the resize stage's time
per batch from ldt_stage_times, taken in a second loop with the stage events
on. Each configuration is warmed up first, and the configurations are
measured in `--reps` alternated rounds so that the spread shows.

  python tools/probes/out_size_probe.py [--steps 60] [--reps 3] [--batch 256]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "..", "lance-distributed-training_amd"))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args()

    import numpy as np
    import torch

    import ldt_amd
    from ldt_amd import _lib, synth
    from oracle import oracle

    assert torch.cuda.is_available(), "needs a HIP device"
    cells, labels = synth.q90_512(a.batch, seed=0)
    res = ldt_amd.ResidentBatch(cells, labels)
    ctx = _lib.Context(0)
    ctx.set_option(_lib.OPT_SYNC_STATUS, 0)
    configs = [((128, 128), 0), ((160, 160), 0), ((192, 192), 0), ((224, 224), 0), ((224, 224), 3),
               ((256, 256), 0), ((384, 384), 0)]
    outs = {}

    def run(size, impl, steps, profile):
        ctx.set_option(_lib.OPT_RESIZE_IMPL, impl)
        ctx.set_option(_lib.OPT_PROFILE, 1 if profile else 0)
        out = outs.setdefault(size, torch.empty((a.batch, 3) + size, dtype=torch.float32, device="cuda"))
        lbl = torch.empty((a.batch,), dtype=torch.int64, device="cuda")
        if profile:
            ctx.stage_times(reset=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            res.decode(out, lbl, ctx=ctx, size=size)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        st = ctx.stage_times(reset=True) if profile else None
        return dt, st, out

    # warm-up and a correctness spot check of every configuration
    for size, impl in configs:
        _, _, out = run(size, impl, a.warmup, False)
        got = out[:2].cpu().numpy()
        for k in range(2):
            assert np.array_equal(got[k], oracle.jpeg_to_tensor(cells[k], *size)), (size, impl, k)
        path = ctx.lib.ldt_debug_last_resize(ctx.handle)
        print(f"# {size[0]}x{size[1]} impl {impl}: bit-exact on 2 images, resize path "
              f"{'k_resize4, %d waves per workgroup' % path if path > 0 else 'streaming k_resize'}", flush=True)
    print("size impl rep img_per_s resize_ms_per_batch decode_ms_per_batch", flush=True)
    for rep in range(a.reps):
        for size, impl in configs:
            dt, _, _ = run(size, impl, a.steps, False)
            _, st, _ = run(size, impl, max(10, a.steps // 3), True)
            rz_ms, rz_n = st["resize"]
            print(f"{size[0]}x{size[1]} {impl} {rep} {a.batch * a.steps / dt:.0f} {rz_ms / max(1, rz_n):.4f} "
                  f"{1e3 * dt / a.steps:.4f}", flush=True)
    ctx.set_option(_lib.OPT_RESIZE_IMPL, 0)


if __name__ == "__main__":
    main()
