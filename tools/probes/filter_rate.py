"""Measurement (not a test): what the bicubic filter costs. The c2 batch
(256 x 512^2 q90, bench.py's generator) decoded resident to 224 x 224 three
ways:

  default     bilinear, the default resize (the band kernel k_resize4);
  streaming   bilinear under LDT_OPT_RESIZE_IMPL 2 (the streaming k_resize,
              the kernel a bicubic batch takes);
  bicubic     interpolation="bicubic": k_resize's bicubic instantiation, 11 taps
              per axis at 512 -> 224 where bilinear has 7.

Per way: images/s of the whole decode (host clock around a synchronised loop,
one batch in flight) and the resize stage's time per batch from
ldt_stage_times, taken in a second loop with the stage events on. Each way is
warmed up and spot-checked first, the bilinear ways against the oracle and
bicubic against Pillow's resize(..., BICUBIC) of the oracle's decoded image,
and the ways are measured in `--reps` alternated rounds so that the spread
shows. No threshold: the `streaming` line of the same run is what `bicubic` is
compared with, and the gap to `default` is what bringing BICUBIC into
k_resize4 would be worth.

  python tools/probes/filter_rate.py [--steps 60] [--reps 3] [--batch 256]
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
    from PIL import Image

    import ldt_amd
    from ldt_amd import _lib, synth
    from oracle import oracle

    assert torch.cuda.is_available(), "needs a HIP device"
    size = (224, 224)
    cells, labels = synth.q90_512(a.batch, seed=0)
    res = ldt_amd.ResidentBatch(cells, labels)
    ctx = _lib.Context(0)
    ctx.set_option(_lib.OPT_SYNC_STATUS, 0)
    out = torch.empty((a.batch, 3) + size, dtype=torch.float32, device="cuda")
    lbl = torch.empty((a.batch,), dtype=torch.int64, device="cuda")
    ways = [("default", 0, "bilinear"), ("streaming", 2, "bilinear"), ("bicubic", 0, "bicubic")]

    def run(impl, interp, steps, profile):
        ctx.set_option(_lib.OPT_RESIZE_IMPL, impl)
        ctx.set_option(_lib.OPT_PROFILE, 1 if profile else 0)
        if profile:
            ctx.stage_times(reset=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            res.decode(out, lbl, ctx=ctx, size=size, interpolation=interp)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt, (ctx.stage_times(reset=True) if profile else None)

    for name, impl, interp in ways:
        run(impl, interp, a.warmup, False)
        got = out[:2].cpu().numpy()
        for k in range(2):
            if interp == "bilinear":
                exp = oracle.jpeg_to_tensor(cells[k], *size)
            else:
                u8 = np.asarray(Image.fromarray(oracle.decode_rgb(cells[k])).resize(size[::-1], Image.BICUBIC))
                exp = oracle.raw_to_tensor(u8, *size)
            assert np.array_equal(got[k], exp), (name, k)
        path = ctx.lib.ldt_debug_last_resize(ctx.handle)
        print(f"# {name}: bit-exact on 2 images, resize path "
              f"{'k_resize4, %d waves per workgroup' % path if path > 0 else 'streaming k_resize'}", flush=True)
    print("way rep img_per_s resize_ms_per_batch decode_ms_per_batch", flush=True)
    for rep in range(a.reps):
        for name, impl, interp in ways:
            dt, _ = run(impl, interp, a.steps, False)
            _, st = run(impl, interp, max(10, a.steps // 3), True)
            rz_ms, rz_n = st["resize"]
            print(f"{name} {rep} {a.batch * a.steps / dt:.0f} {rz_ms / max(1, rz_n):.4f} {1e3 * dt / a.steps:.4f}",
                  flush=True)
    ctx.set_option(_lib.OPT_RESIZE_IMPL, 0)


if __name__ == "__main__":
    main()
