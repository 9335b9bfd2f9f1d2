#!/usr/bin/env python
"""What the source pad costs and saves: LLaVA's ``expand2square`` + CLIP resize
on a batch of 256 2:1 sources (512 wide x 256 high, q90 4:2:0, written with
``synth.encode``), ``ExpandToSquare`` to 336 x 336, BICUBIC, bfloat16, CLIP's
Normalize:

  * ``source-pad``: the call, ``crop=ExpandToSquare(), pad=Pad(fill,
    source=True)``, on cells resident in HBM;
  * ``clipped-crop``: the unpadded crop call of the same boxes clipped to the
    image on the same resident batch: the same decode and the same output size,
    so the difference is the cost of the feature;
  * ``native+F.pad``: what a user does without it: ``decode_native`` (from host
    cells, the only form it takes, so the copy of 256 small files is in it),
    then ``torch.nn.functional.pad`` and a bicubic ``interpolate`` per image;

and, for the A/B against a parent build, ``crop``: a ``RandomResizedCropFlip``
call to 224 x 224 without ``pad=`` on the same batch, which must launch what it
launched before.

One process, the variants alternated round by round (the order rotates), HIP
events around ``--steps`` calls, the median of ``--rounds`` rounds and every
round's value, one JSON line per variant. ``--lib PATH`` loads that libldt.so
instead (a parent build has no source pad: only ``clipped-crop`` and ``crop``
run); alternate the two processes in one session for
``profiles/source_pad/ab_parent.txt``.

    python tools/bench_source_pad.py [--rounds 5] [--steps 20] [--lib PATH] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lance-distributed-training_amd"))

CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
FILL = (122, 116, 104)  # int(255 * mean), LLaVA's fill


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--parent", action="store_true", help="the library has no source pad: run what it can")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "source_pad", "bench_source_pad.jsonl"))
    args = ap.parse_args()
    if args.lib:
        os.environ["LDT_LIBRARY"] = args.lib

    import numpy as np
    import pyarrow as pa
    import torch

    import ldt_amd

    from ldt_amd import synth

    n, dev = 256, torch.device("cuda", torch.cuda.current_device())
    cells = [synth.encode(synth.field(256, 512, 300 + k % 8, 6.0), quality=90) for k in range(n)]
    arr, wide = pa.array(cells, pa.binary()), ldt_amd.ResidentBatch(cells, np.arange(n))
    norm = (CLIP_MEAN, CLIP_STD)
    out = torch.empty((n, 3, 336, 336), dtype=torch.bfloat16, device=dev)
    ref = torch.empty_like(out)
    small = torch.empty((n, 3, 224, 224), device=dev)
    lbl = torch.empty((n,), dtype=torch.int64, device=dev)
    boxes = ldt_amd.ExpandToSquare().sample(*wide.image_sizes())
    assert boxes[0].tolist() == [-128, 0, 512, 512, 0]
    clipped = np.array([[0, 0, 256, 512, 0]] * n, np.int32)
    rrc = ldt_amd.RandomResizedCropFlip(generator=torch.Generator().manual_seed(1)).sample(*wide.image_sizes())
    fill = torch.tensor([(f / 255.0 - m) / s for f, m, s in zip(FILL, CLIP_MEAN, CLIP_STD)], device=dev).view(3, 1, 1)

    def source_pad():
        wide.decode(out, lbl, norm, size=(336, 336), crops=boxes, pad=ldt_amd.Pad(FILL, source=True),
                    interpolation="bicubic", dtype=torch.bfloat16)

    def clipped_crop():
        wide.decode(out, lbl, norm, size=(336, 336), crops=clipped, interpolation="bicubic", dtype=torch.bfloat16)

    def native_fpad():
        imgs, _ = ldt_amd.decode_native(arr, dtype=torch.float32, normalize=norm)
        for k, t in enumerate(imgs):
            h, w = t.shape[1:]
            s = max(h, w)
            sq = fill.expand(3, s, s).clone()
            sq[:, (s - h) // 2:(s - h) // 2 + h, (s - w) // 2:(s - w) // 2 + w] = t
            ref[k] = torch.nn.functional.interpolate(sq[None], size=(336, 336), mode="bicubic", antialias=True)[0]

    def crop():
        wide.decode(small, lbl, size=(224, 224), crops=rrc)

    variants = {"clipped-crop": clipped_crop, "crop": crop}
    if not args.parent:
        variants.update({"source-pad": source_pad, "native+F.pad": native_fpad})
    names = list(variants)
    ms = {k: [] for k in names}
    for r in range(args.rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            fn = variants[k]
            for _ in range(2):
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
