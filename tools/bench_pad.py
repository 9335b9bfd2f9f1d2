#!/usr/bin/env python
"""What the padded window saves: the letterbox call on a resident batch of 2:1
sources (256 x 512 wide x 256 high, q90 4:2:0, written with ``synth.encode``;
cells in HBM, output 512 x 512 so that half of every output is fill) against

  * ``window``: the same build's unpadded windowed call to the same res (the
    resize alone: 256 x 512 out of res 256 x 512), and
  * ``window+F.pad``: that call followed by ``torch.nn.functional.pad`` into the
    ``size`` tensor (what a user does without ``pad=``),

and, for the A/B against a parent build, ``center-crop``: the
``ResizeCenterCrop(256)`` -> 224 windowed call without ``pad=`` on the square c2
batch (256 x 512 x 512), which must launch what it launched before.

One process, the variants alternated round by round (the order rotates), HIP
events around ``--steps`` calls on one context and one stream, the median of
``--rounds`` rounds and every round's value, one JSON line per variant.
``--lib PATH`` loads that libldt.so instead (a parent build has no ``pad=``:
only ``window`` and ``center-crop`` run); alternate the two processes in one
session for ``profiles/pad/ab_parent.txt``.

    python tools/bench_pad.py [--rounds 5] [--steps 40] [--lib PATH] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lance-distributed-training_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pad", "bench_pad.jsonl"))
    args = ap.parse_args()
    if args.lib:
        os.environ["LDT_LIBRARY"] = args.lib

    import numpy as np
    import torch

    import ldt_amd
    from ldt_amd import synth
    from ldt_amd import transforms as T

    n, dev = 256, torch.device("cuda", torch.cuda.current_device())
    has_pad = hasattr(ldt_amd.load_library(), "ldt_set_pad")
    wide = ldt_amd.ResidentBatch([synth.encode(synth.field(256, 512, 300 + k % 8, 6.0), quality=90) for k in range(n)],
                                 np.arange(n))
    square = ldt_amd.ResidentBatch([synth.encode(synth.field(512, 512, 400 + k % 8, 6.0), quality=90) for k in range(n)],
                                   np.arange(n))
    big = torch.empty((n, 3, 512, 512), device=dev)
    half = torch.empty((n, 3, 256, 512), device=dev)
    small = torch.empty((n, 3, 224, 224), device=dev)
    lbl = torch.empty((n,), dtype=torch.int64, device=dev)
    box = ldt_amd.Letterbox().sample(*wide.image_sizes(), (512, 512))
    assert box[0].tolist() == [256, 512, -128, 0]
    inside = np.array([[256, 512, 0, 0]] * n, np.int32)
    centre = ldt_amd.ResizeCenterCrop(256).sample(*square.image_sizes(), (224, 224))

    def window():
        wide.decode(half, lbl, size=(256, 512), windows=inside)

    def window_fpad():
        wide.decode(half, lbl, size=(256, 512), windows=inside)
        big.copy_(torch.nn.functional.pad(half, (0, 0, 128, 128), value=114.0 / 255.0))

    def letterbox():
        wide.decode(big, lbl, size=(512, 512), windows=box, pad=ldt_amd.Pad(114))

    def center_crop():
        square.decode(small, lbl, size=(224, 224), windows=centre)

    variants = {"window": window, "center-crop": center_crop}
    if has_pad:
        variants.update({"window+F.pad": window_fpad, "letterbox": letterbox})
        letterbox()
        window_fpad()
        torch.cuda.synchronize()
        assert torch.equal(big[:, :, 128:384], half), "the letterbox's image rows are not the windowed call's"
    names = list(variants)
    ms = {k: [] for k in names}
    for r in range(args.rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            fn = variants[k]
            for _ in range(3):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.steps):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b) / args.steps)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:  # a fresh file: one run's lines, never mixed with an earlier run's
        for k in names:
            line = json.dumps({"variant": k, "lib": args.lib or "this build", "ms_median": statistics.median(ms[k]),
                               "ms_rounds": ms[k], "img_per_s": n / statistics.median(ms[k]) * 1e3})
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
