"""Training-time augmentation parameters for the decode path.

``RandomResizedCropFlip`` draws, per image, the box of torchvision's
``RandomResizedCrop`` and the coin of ``RandomHorizontalFlip``; the decode
takes them as ``crops=`` / ``crop=`` and applies both inside the fused resize
kernel (``ldt_set_crops``), bit-exact with ``F.resized_crop`` + ``hflip`` on
the PIL image. Only the parameters are drawn here, on the host, from the
headers' sizes (``image_sizes``): no pixel is touched.
"""
from __future__ import annotations

import math

import numpy as np
import torch


class RandomResizedCropFlip:
    """``RandomResizedCrop(size, scale, ratio)`` + ``RandomHorizontalFlip(flip_p)``
    as parameters: ``sample(wh)`` returns int32 ``[n, 5]`` rows of
    ``(top, left, height, width, flip)`` for images of ``wh[i] = (width,
    height)``; the output size is the decode's ``size=``.

    The draws restate torchvision 0.2x's ``RandomResizedCrop.get_params``
    followed by ``RandomHorizontalFlip.forward``, per image in row order, with
    torch's RNG (``generator``, else the global one). Per image, up to 10
    tries of: ``target_area = W * H * torch.empty(1).uniform_(scale[0],
    scale[1])``; ``aspect = exp(torch.empty(1).uniform_(log ratio[0], log
    ratio[1]))`` (the logs in float32, as ``torch.log(torch.tensor(ratio))``
    gives them); ``w = int(round(sqrt(target_area * aspect)))``, ``h =
    int(round(sqrt(target_area / aspect)))``; accepted if ``0 < w <= W and 0 <
    h <= H``, then ``top = torch.randint(0, H - h + 1, (1,))`` and ``left =
    torch.randint(0, W - w + 1, (1,))``. After 10 failures the centre crop:
    the whole image, narrowed to ``ratio`` (``W / H < min(ratio)``: ``w = W, h
    = round(w / min(ratio))``; ``> max(ratio)``: ``h = H, w = round(h *
    max(ratio))``), ``top = (H - h) // 2``, ``left = (W - w) // 2``. The flip
    comes last: ``torch.rand(1) < flip_p``.

    torchvision is not a dependency of this package and is not installed where
    its tests run, so this order is restated from torchvision's source and is
    not tested against torchvision itself: the tests pin the rule above.

    A row whose size is unknown (``status[i] != 0``, or a size of 0: a cell the
    header walk rejects) draws nothing and gets ``(0, 0, 1, 1, 0)``; its decode
    fails with its own status. Picklable when ``generator`` is None.
    """

    def __init__(self, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip_p=0.5, generator=None):
        self.scale = (float(scale[0]), float(scale[1]))
        self.ratio = (float(ratio[0]), float(ratio[1]))
        if not (0.0 < self.scale[0] <= self.scale[1]) or not (0.0 < self.ratio[0] <= self.ratio[1]):
            raise ValueError(f"scale {scale!r} and ratio {ratio!r} must be increasing pairs of positive numbers")
        self.flip_p = float(flip_p)
        if not 0.0 <= self.flip_p <= 1.0:
            raise ValueError(f"flip_p must be in [0, 1], got {flip_p!r}")
        self.generator = generator

    def _box(self, width: int, height: int):
        g = self.generator
        area = height * width
        log_ratio = torch.log(torch.tensor(self.ratio))
        for _ in range(10):
            target_area = area * torch.empty(1).uniform_(self.scale[0], self.scale[1], generator=g).item()
            aspect = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=g)).item()
            w = int(round(math.sqrt(target_area * aspect)))
            h = int(round(math.sqrt(target_area / aspect)))
            if 0 < w <= width and 0 < h <= height:
                top = torch.randint(0, height - h + 1, size=(1,), generator=g).item()
                left = torch.randint(0, width - w + 1, size=(1,), generator=g).item()
                return top, left, h, w
        in_ratio = float(width) / float(height)
        if in_ratio < min(self.ratio):
            w = width
            h = int(round(w / min(self.ratio)))
        elif in_ratio > max(self.ratio):
            h = height
            w = int(round(h * max(self.ratio)))
        else:
            w, h = width, height
        w, h = max(1, min(w, width)), max(1, min(h, height))
        return (height - h) // 2, (width - w) // 2, h, w

    def sample(self, wh, status=None) -> np.ndarray:
        wh = np.asarray(wh)
        if wh.ndim != 2 or wh.shape[1] != 2:
            raise ValueError(f"wh must have shape [n, 2] (width, height), got {wh.shape}")
        n = wh.shape[0]
        out = np.zeros((n, 5), np.int32)
        for i in range(n):
            width, height = int(wh[i, 0]), int(wh[i, 1])
            if (status is not None and int(status[i]) != 0) or width <= 0 or height <= 0:
                out[i] = (0, 0, 1, 1, 0)
                continue
            top, left, h, w = self._box(width, height)
            flip = int(torch.rand(1, generator=self.generator).item() < self.flip_p)
            out[i] = (top, left, h, w, flip)
        return out

    def __repr__(self) -> str:
        return f"RandomResizedCropFlip(scale={self.scale}, ratio={self.ratio}, flip_p={self.flip_p})"
