"""Augmentation and evaluation transform parameters for the decode path.

``RandomResizedCropFlip`` draws, per image, the box of torchvision's
``RandomResizedCrop`` and the coin of ``RandomHorizontalFlip``; the decode
takes them as ``crops=`` / ``crop=`` and applies both inside the fused resize
kernel (``ldt_set_crops``), bit-exact with ``F.resized_crop`` + ``hflip`` on
the PIL image. Only the parameters are drawn here, on the host, from the
headers' sizes (``image_sizes``): no pixel is touched.

``ResizeCenterCrop`` computes, per image, the resized size of ``Resize(edge)``
(the shorter edge scaled to ``edge``) and the window of ``CenterCrop(size)``;
the decode takes them as ``windows=`` / ``window=`` (``ldt_set_windows``).

``ResizeFiveCrop`` computes the five (or, mirrored too, ten) windows of
``Resize(edge)`` + ``FiveCrop(size)`` / ``TenCrop(size)``; a decode call takes
them as the ``views`` of each image (``ldt_set_views``): one decode, five or
ten outputs.

``ColorJitterParams`` draws, per output image, the parameters of
``RandomApply([ColorJitter])``, ``RandomGrayscale`` and ``RandomSolarize``; the
decode takes them as ``colors=`` / ``color=`` (``ldt_set_colors``) and applies
them to the resized uint8 image before ``ToTensor`` / ``Normalize``, bit-exact
with Pillow.

``TrivialAugmentWide`` and ``RandAugment`` draw, per output image, the ops of
torchvision's transforms of those names, and ``RandomErasing`` its box; the
decode takes them as ``augments=`` / ``augment=`` (``ldt_set_augments``) and
applies the ops to the resized uint8 image, bit-exact with Pillow, and the box
after ``Normalize``. ``affine_matrix`` gives the matrix of one geometric op.
"""
from __future__ import annotations

import functools
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

    ``sample(wh, status, views=V)`` returns ``[n, V, 5]``: V views of every
    image for a decode call with ``views=V``. The draws go image by image, and
    view by view within the image (box tries, then the flip, per view): the
    order in which a two-crop wrapper that calls the torchvision transform V
    times per sample consumes the RNG, and the one ``sample(np.repeat(wh, V,
    axis=0))`` gives. An unknown row gets ``(0, 0, 1, 1, 0)`` in every view and
    draws nothing.

    ``scale`` may also be a sequence of V pairs, one per view (multi-crop:
    ``[(0.4, 1.0)] * 2 + [(0.05, 0.4)] * 6`` for two global and six local
    views). ``sample(wh, status, views=V)`` then draws view ``v`` from
    ``scale[v]``, in the same order (image by image, view by view, box tries and
    then the flip); a ``views`` other than V, or none, is a ``ValueError``. A
    single pair draws what it always drew. ``.scale`` stays a pair (the first
    view's) and ``.scales`` is the list, or None.
    """

    def __init__(self, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip_p=0.5, generator=None):
        self.scales = None
        if len(scale) > 0 and all(hasattr(p, "__len__") and not isinstance(p, (str, bytes)) for p in scale):
            from ._lib import MAX_VIEWS

            if not 1 <= len(scale) <= MAX_VIEWS or any(len(p) != 2 for p in scale):
                raise ValueError(f"scale {scale!r}: a pair, or 1..{MAX_VIEWS} pairs (one per view)")
            self.scales = [(float(p[0]), float(p[1])) for p in scale]
            if any(not (0.0 < a <= b) for a, b in self.scales):
                raise ValueError(f"scale {scale!r}: every view's scale must be an increasing pair of positive numbers")
            scale = self.scales[0]
        elif len(scale) != 2:
            raise ValueError(f"scale {scale!r}: a pair, or a sequence of pairs (one per view)")
        self.scale = (float(scale[0]), float(scale[1]))
        self.ratio = (float(ratio[0]), float(ratio[1]))
        if not (0.0 < self.scale[0] <= self.scale[1]) or not (0.0 < self.ratio[0] <= self.ratio[1]):
            raise ValueError(f"scale {scale!r} and ratio {ratio!r} must be increasing pairs of positive numbers")
        self.flip_p = float(flip_p)
        if not 0.0 <= self.flip_p <= 1.0:
            raise ValueError(f"flip_p must be in [0, 1], got {flip_p!r}")
        self.generator = generator

    def _box(self, width: int, height: int, scale=None):
        g = self.generator
        scale = self.scale if scale is None else scale
        area = height * width
        log_ratio = torch.log(torch.tensor(self.ratio))
        for _ in range(10):
            target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=g).item()
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

    def sample(self, wh, status=None, views=None) -> np.ndarray:
        from ._lib import check_views

        views = check_views(views)
        if self.scales is not None and views != len(self.scales):
            raise ValueError(f"views={views} with {self!r}, whose scale lists {len(self.scales)} views")
        wh = np.asarray(wh)
        if wh.ndim != 2 or wh.shape[1] != 2:
            raise ValueError(f"wh must have shape [n, 2] (width, height), got {wh.shape}")
        n = wh.shape[0]
        nv = 1 if views is None else views
        out = np.zeros((n, nv, 5), np.int32)
        for i in range(n):
            width, height = int(wh[i, 0]), int(wh[i, 1])
            if (status is not None and int(status[i]) != 0) or width <= 0 or height <= 0:
                out[i] = (0, 0, 1, 1, 0)
                continue
            for v in range(nv):
                top, left, h, w = self._box(width, height, None if self.scales is None else self.scales[v])
                flip = int(torch.rand(1, generator=self.generator).item() < self.flip_p)
                out[i, v] = (top, left, h, w, flip)
        return out[:, 0] if views is None else out

    def __repr__(self) -> str:
        scale = self.scale if self.scales is None else self.scales
        return f"RandomResizedCropFlip(scale={scale}, ratio={self.ratio}, flip_p={self.flip_p})"


class ColorJitterParams:
    """``RandomApply([ColorJitter(brightness, contrast, saturation, hue)], p)``
    + ``RandomGrayscale(gray_p)`` + ``RandomApply([GaussianBlur], blur_p)`` +
    ``RandomSolarize(solarize_threshold, solarize_p)`` as parameters:
    ``sample(n, views=None)`` returns float64
    ``[n, 7]`` (``[n, V, 7]`` with ``views=V``) rows of ``(brightness,
    contrast, saturation, hue, order, gray, solarize)``, or, when ``blur_p`` is
    set, ``[n, 8]`` (``[n, V, 8]``) rows with ``blur`` (the radius, NaN = not
    applied) as the last column, which the decode takes
    as ``colors=`` / ``color=`` (``check_colors`` says what each column means)
    and applies to the resized uint8 image, after crop, resize, window and flip
    and before ``ToTensor`` / ``Normalize``, bit-exact with Pillow. Only the
    parameters are drawn here, on the host: no pixel is touched.

    Ranges follow torchvision's ``ColorJitter._check_input``: a number ``x``
    for brightness, contrast or saturation means ``[max(0, 1 - x), 1 + x]``,
    for hue ``[-x, x]``; a pair is taken as given; ``None`` or 0 means the op is
    absent (its column is NaN and it draws nothing).

    ``p``, ``gray_p``, ``blur_p`` and ``solarize_p`` may each be a float,
    ``None`` (the transform is absent and draws nothing) or a sequence of V
    values, one per view, which ``sample(n, views=V)`` then requires (DINO:
    ``blur_p=[1.0, 0.1] + [0.5] * 6``, ``solarize_p=[0.0, 0.2] + [0.0] * 6``).

    The blur is Pillow's ``ImageFilter.GaussianBlur(radius)`` with ``radius``
    drawn uniformly from ``blur_radius`` (a pair within (0, 8.0]; the DINO,
    MoCo and BYOL loaders' ``(0.1, 2.0)`` is the default), the blur those
    loaders apply to the PIL image; torchvision's own float ``GaussianBlur`` is
    a different filter and is not offered. Blur commutes with the mirror, so
    MoCo's "blur, then flip" is this library's "flip, then blur".

    The draws use torch's RNG (``generator``, else the global one) and go
    image by image and view by view, restating torchvision 0.2x in this order:

    1. ``RandomApply``: ``r = torch.rand(1)``; the jitter is skipped iff ``p <
       r``. A skipped jitter gives NaN factors and the order 0123.
    2. If applied, ``ColorJitter.get_params``: ``torch.randperm(4)``, then
       ``float(torch.empty(1).uniform_(lo, hi))`` for brightness, contrast,
       saturation and hue, in that order; an absent op draws nothing.
    3. ``RandomGrayscale``: ``torch.rand(1) < gray_p``.
    4. The blur, by ``RandomApply``'s rule: ``r = torch.rand(1)``; skipped
       iff ``blur_p < r``. If applied, ``float(torch.empty(1).uniform_(lo,
       hi))`` is the radius (those loaders draw it with ``random.uniform``:
       the same distribution from another generator).
    5. ``RandomSolarize``: ``torch.rand(1) < solarize_p``.

    With ``blur_p=None`` step 4 draws nothing and a seed gives the array it
    gave before the blur existed.

    torchvision is not a dependency of this package and is not installed where
    its tests run, so this order is restated from torchvision's source and is
    not tested against torchvision itself: the tests pin the rule above. A
    ``Compose`` interleaves these draws with the crop's, sample by sample,
    while this library draws all boxes of a batch first and the colours after
    them, so a seeded run does not reproduce a seeded ``Compose`` draw for
    draw; the distributions are the same.

    Picklable when ``generator`` is None.
    """

    def __init__(self, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, p=0.8, gray_p=0.2, solarize_p=None,
                 solarize_threshold=128, generator=None, blur_p=None, blur_radius=(0.1, 2.0)):
        self.brightness = self._range(brightness, "brightness")
        self.contrast = self._range(contrast, "contrast")
        self.saturation = self._range(saturation, "saturation")
        self.hue = self._range(hue, "hue", center=0.0, bound=(-0.5, 0.5), clip_first_on_zero=False)
        self.p = self._prob(p, "p")
        self.gray_p = self._prob(gray_p, "gray_p")
        self.solarize_p = self._prob(solarize_p, "solarize_p")
        if isinstance(solarize_threshold, bool) or int(solarize_threshold) != solarize_threshold or \
                not 0 <= int(solarize_threshold) <= 256:
            raise ValueError(f"solarize_threshold must be an int in 0..256, got {solarize_threshold!r}")
        self.solarize_threshold = int(solarize_threshold)
        self.generator = generator
        self.blur_p = self._prob(blur_p, "blur_p")
        from ._lib import BLUR_MAX_RADIUS

        if not hasattr(blur_radius, "__len__") or len(blur_radius) != 2:
            raise TypeError(f"blur_radius should be a pair (lo, hi), got {blur_radius!r}")
        lo, hi = float(blur_radius[0]), float(blur_radius[1])
        if not 0.0 < lo <= hi <= BLUR_MAX_RADIUS:
            raise ValueError(f"blur_radius values should be in (0, {BLUR_MAX_RADIUS}] (the limit: box radius 7) and "
                             f"ordered, got {(lo, hi)}")
        self.blur_radius = (lo, hi)

    @staticmethod
    def _range(value, name, center=1.0, bound=(0.0, float("inf")), clip_first_on_zero=True):
        """torchvision's ``ColorJitter._check_input``: the (lo, hi) of the op, or None when it is absent."""
        if value is None:
            return None
        if isinstance(value, (int, float)) and not isinstance(value, bool):
            if value < 0:
                raise ValueError(f"if {name} is a single number, it must be non negative")
            lo, hi = center - float(value), center + float(value)
            if clip_first_on_zero:
                lo = max(lo, 0.0)
        elif hasattr(value, "__len__") and len(value) == 2:
            lo, hi = float(value[0]), float(value[1])
        else:
            raise TypeError(f"{name} should be a single number or a pair, got {value!r}")
        if not bound[0] <= lo <= hi <= bound[1]:
            raise ValueError(f"{name} values should be between {bound}, got {(lo, hi)}")
        return None if lo == hi == center else (lo, hi)

    @staticmethod
    def _prob(p, name):
        """None, a float in [0, 1], or a tuple of them (one per view)."""
        if p is None:
            return None
        many = hasattr(p, "__len__")
        vals = tuple(float(x) for x in p) if many else (float(p),)
        if not vals or any(not 0.0 <= x <= 1.0 for x in vals):
            raise ValueError(f"{name} must be None, a probability in [0, 1] or a sequence of them, got {p!r}")
        return vals if many else vals[0]

    def _at(self, p, v):
        return p[v] if isinstance(p, tuple) else p

    def sample(self, n, views=None) -> np.ndarray:
        from ._lib import check_views

        views = check_views(views)
        for name in ("p", "gray_p", "blur_p", "solarize_p"):
            q = getattr(self, name)
            if isinstance(q, tuple) and views != len(q):
                raise ValueError(f"views={views} with {self!r}, whose {name} lists {len(q)} views")
        g = self.generator
        nv = 1 if views is None else views
        out = np.zeros((int(n), nv, 7 if self.blur_p is None else 8), np.float64)
        out[..., :4] = np.nan
        out[..., 7:] = np.nan
        out[..., 4] = 0 + 4 * 1 + 16 * 2 + 64 * 3
        out[..., 6] = -1
        ranges = (self.brightness, self.contrast, self.saturation, self.hue)
        for i in range(int(n)):
            for v in range(nv):
                p = self._at(self.p, v)
                if p is not None and not p < torch.rand(1, generator=g).item():
                    perm = torch.randperm(4, generator=g).tolist()
                    out[i, v, 4] = perm[0] + 4 * perm[1] + 16 * perm[2] + 64 * perm[3]
                    for k, r in enumerate(ranges):
                        if r is not None:
                            out[i, v, k] = float(torch.empty(1).uniform_(r[0], r[1], generator=g))
                gp = self._at(self.gray_p, v)
                if gp is not None:
                    out[i, v, 5] = float(torch.rand(1, generator=g).item() < gp)
                bp = self._at(self.blur_p, v)
                if bp is not None and not bp < torch.rand(1, generator=g).item():
                    out[i, v, 7] = float(torch.empty(1).uniform_(self.blur_radius[0], self.blur_radius[1],
                                                                 generator=g))
                sp = self._at(self.solarize_p, v)
                if sp is not None and torch.rand(1, generator=g).item() < sp:
                    out[i, v, 6] = self.solarize_threshold
        return out[:, 0] if views is None else out

    def __repr__(self) -> str:
        return (f"ColorJitterParams(brightness={self.brightness}, contrast={self.contrast}, "
                f"saturation={self.saturation}, hue={self.hue}, p={self.p}, gray_p={self.gray_p}, "
                f"solarize_p={self.solarize_p}, solarize_threshold={self.solarize_threshold}"
                + ("" if self.blur_p is None else f", blur_p={self.blur_p}, blur_radius={self.blur_radius}") + ")")


class ResizeCenterCrop:
    """``Resize(edge)`` + ``CenterCrop(size)`` as parameters: the evaluation
    transform. ``sample(wh, status, size)`` returns int32 ``[n, 4]`` rows of
    ``(res_h, res_w, top, left)`` for images of ``wh[i] = (width, height)``:
    the decode takes them as ``windows=`` / ``window=`` (``ldt_set_windows``),
    resizes each image to ``res_h x res_w`` and keeps the ``size`` window at
    ``(top, left)``, bit-exact with Pillow's ``resize().crop()``. No RNG;
    picklable.

    torchvision is not a dependency of this package and is not installed where
    its tests run, so its arithmetic is restated here (torchvision 0.2x) and
    the tests pin these expressions, not torchvision itself:

    ``Resize(edge)``, ``_compute_resized_output_size``: ``short, long = (w, h)
    if w <= h else (h, w)``; ``new_short, new_long = edge, int(edge * long /
    short)``; ``new_w, new_h = (new_short, new_long) if w <= h else (new_long,
    new_short)``. For sizes up to LDT_MAX_DIM and edges up to 65535 the float
    quotient is never within rounding of an integer it does not equal, so
    ``int(edge * long / short) == edge * long // short``, which is what is
    computed.

    ``CenterCrop(size)``: ``top = int(round((res_h - out_h) / 2.0))``, ``left =
    int(round((res_w - out_w) / 2.0))``. Python's ``round`` is half-to-even: a
    difference of 1 gives 0, 3 gives 2, 5 gives 2.

    A row whose size is unknown (``status[i] != 0``, or a size of 0) gets
    ``(out_h, out_w, 0, 0)`` and its decode fails with its own status. A row
    whose resized image is smaller than ``size`` is emitted as computed, with
    a negative ``top`` / ``left``: torchvision would pad it, the decode pads
    nothing and fails that row alone (``LDT_IMG_BAD_WINDOW``). With a
    ``RandomResizedCropFlip`` in the same call ``wh`` is the drawn boxes'
    sizes.

    ``sample(wh, status, size, views=V)`` returns ``[n, V, 4]`` for a decode
    call with ``views=V``: ``wh`` is then ``[n, V, 2]`` (the sizes of each
    view's drawn box, when a crop sampler is in the same call) or ``[n, 2]``,
    which every view shares. ``size`` may then be a size list of V pairs (a
    decode call with one output size per view): view ``v``'s window is centred
    for ``size[v]``.
    """

    def __init__(self, edge):
        if isinstance(edge, bool) or not isinstance(edge, (int, np.integer)):
            raise TypeError(f"edge must be an int (the shorter edge after the resize), got {edge!r}")
        if not 1 <= int(edge) <= 65535:
            raise ValueError(f"edge must be in 1..65535, got {edge!r}")
        self.edge = int(edge)

    def sample(self, wh, status=None, size=None, views=None) -> np.ndarray:
        from ._lib import ViewSizes, check_size, check_view_sizes, check_views

        views = check_views(views)
        size = check_view_sizes(size)
        sized = isinstance(size, ViewSizes)
        if sized and views != len(size):
            raise ValueError(f"views={views} with a size list of {len(size)} views")
        wh = np.asarray(wh)
        if views is not None:
            if wh.ndim == 2 and wh.shape[1] == 2:
                wh = np.repeat(wh[:, None, :], views, axis=1)
            if wh.ndim != 3 or wh.shape[1] != views or wh.shape[2] != 2:
                raise ValueError(f"wh must have shape [n, 2] or [n, {views}, 2] (width, height), got {wh.shape}")
            n = wh.shape[0]
            if sized:  # every view for its own size
                return np.stack([self.sample(wh[:, v], status, size[v]) for v in range(views)], axis=1)
            st = None if status is None else np.repeat(np.asarray(status), views)
            return self.sample(wh.reshape(n * views, 2), st, size).reshape(n, views, 4)
        out_h, out_w = size
        if wh.ndim != 2 or wh.shape[1] != 2:
            raise ValueError(f"wh must have shape [n, 2] (width, height), got {wh.shape}")
        w, h = wh[:, 0].astype(np.int64), wh[:, 1].astype(np.int64)
        known = (w > 0) & (h > 0)
        if status is not None:
            known &= np.asarray(status) == 0
        ws, hs = np.where(known, w, 1), np.where(known, h, 1)
        upright = ws <= hs  # the width is the shorter edge
        short, long = np.where(upright, ws, hs), np.where(upright, hs, ws)
        new_long = self.edge * long // short
        res_w = np.where(upright, self.edge, new_long)
        res_h = np.where(upright, new_long, self.edge)

        def centre(d):  # int(round(d / 2.0)), half to even
            q = d // 2
            return q + ((d & 1) & (q & 1))

        out = np.stack([res_h, res_w, centre(res_h - out_h), centre(res_w - out_w)], axis=1)
        out[~known] = (out_h, out_w, 0, 0)
        return np.clip(out, -(1 << 31), (1 << 31) - 1).astype(np.int32)

    def __repr__(self) -> str:
        return f"ResizeCenterCrop({self.edge})"


class Draft:
    """Pillow's ``Image.draft(mode, size)`` as parameters: the libjpeg scale a
    drafted decode takes per image. ``Draft((h, w))`` asks for the smallest
    DCT-domain decode that still covers ``h x w`` (this package's order; Pillow
    takes ``(w, h)``): ``sample(wh, status)`` returns int32 ``[n]`` scales for
    images of ``wh[i] = (width, height)`` by Pillow's rule, ``k = min(W // w,
    H // h)`` and the largest of 8, 4, 2, 1 that is not above ``k`` (1 when
    ``k`` is 0: the image is smaller than the request). The decode takes them
    as ``draft=`` / ``drafts=`` (``ldt_set_draft``) and row i decodes to
    ``ceil(W / s) x ceil(H / s)``, bit for bit what Pillow's ``draft`` +
    ``convert("RGB")`` gives; crops, windows and the samplers that draw them
    then see that size. ``draft=Draft((256, 256)), window=ResizeCenterCrop(256),
    size=(224, 224)`` is the thumbnail / evaluation recipe. A row whose size is
    unknown (``status[i] != 0``, or a size of 0) gets 1 and fails with its own
    status. No RNG; picklable."""

    def __init__(self, size):
        ok = isinstance(size, (tuple, list)) and len(size) == 2 and all(
            isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in size)
        if not ok:
            raise TypeError(f"Draft takes the requested size as a pair of ints (h, w), got {size!r}")
        if min(size) < 1:
            raise ValueError(f"Draft: the requested size must be at least 1 x 1, got {size!r}")
        self.size = (int(size[0]), int(size[1]))

    def sample(self, wh, status=None) -> np.ndarray:
        wh = np.asarray(wh)
        if wh.ndim != 2 or wh.shape[1] != 2:
            raise ValueError(f"wh must have shape [n, 2] (width, height), got {wh.shape}")
        h, w = self.size
        k = np.minimum(wh[:, 0].astype(np.int64) // w, wh[:, 1].astype(np.int64) // h)
        if status is not None:
            k = np.where(np.asarray(status) == 0, k, 0)
        scale = np.where(k >= 8, 8, np.where(k >= 4, 4, np.where(k >= 2, 2, 1)))
        return scale.astype(np.int32)

    def __repr__(self) -> str:
        return f"Draft({self.size})"


class ResizeFiveCrop:
    """``Resize(edge)`` + ``FiveCrop(size)`` (``ten=True``: ``TenCrop(size)``)
    as parameters: five or ten windows of every image from one decode. Passing
    it as ``window=`` implies ``views = .views`` (5 or 10; a different explicit
    ``views=`` is a ``ValueError``), and the output is ``[views, n, 3, h, w]``:
    ``out[v]`` is the batch of crop ``v``. ``sample(wh, status, size)`` returns
    int32 ``[n, views, 4]`` rows of ``(res_h, res_w, top, left)``. No RNG;
    picklable.

    torchvision's arithmetic (0.2x), restated because torchvision is not
    installed where the tests run; the tests pin these expressions and Pillow's
    result, not torchvision itself:

    ``Resize(edge)``: as in ``ResizeCenterCrop`` (the shorter edge becomes
    ``edge``, the longer ``edge * long // short``).

    ``FiveCrop(size)``, ``F.five_crop``, in its order: ``tl = crop(0, 0)``,
    ``tr = crop(0, res_w - out_w)``, ``bl = crop(res_h - out_h, 0)``, ``br =
    crop(res_h - out_h, res_w - out_w)`` (top, left), then ``center_crop``:
    ``top = int(round((res_h - out_h) / 2.0))``, ``left = int(round((res_w -
    out_w) / 2.0))``, half to even as in ``ResizeCenterCrop``.

    ``TenCrop(size)``, ``F.ten_crop`` with ``vertical_flip=False``: the five
    crops of the image, then the five crops of ``hflip(image)`` in the same
    order. The decode applies window, then flip, and crop ``(top, left)`` of
    the mirrored image is the mirror of crop ``(top, res_w - out_w - left)``
    of the image: views 5..9 are the windows ``(tr, tl, br, bl, centre')`` with
    flip 1, where ``centre'`` has ``left = res_w - out_w - centre.left`` (the
    same window unless the difference is odd). The flips travel as crops:
    ``boxes(wh, status)`` gives whole-image boxes ``(0, 0, height, width,
    flip)`` with flip 0 for views 0..4 and 1 for views 5..9, which the decode
    uses when ``crop=`` is None; ``ten=True`` together with a ``crop=`` is a
    ``ValueError``.

    A row whose size is unknown gets ``(out_h, out_w, 0, 0)`` windows (and
    ``(0, 0, 1, 1, 0)`` boxes) and fails with its own status. A resized image
    smaller than ``size`` is emitted as computed, with negative origins:
    torchvision raises for it, the decode fails that row alone
    (``LDT_IMG_BAD_WINDOW``) in all its views.
    """

    def __init__(self, edge, ten=False):
        self._resize = ResizeCenterCrop(edge)  # validates the edge
        self.edge = self._resize.edge
        self.ten = bool(ten)
        self.views = 10 if self.ten else 5

    def sample(self, wh, status=None, size=None, views=None) -> np.ndarray:
        from ._lib import check_views

        views = check_views(views)
        if views is not None and views != self.views:
            raise ValueError(f"views={views} with {self!r}, which has {self.views} views")
        wh = np.asarray(wh)
        if wh.ndim == 3 and wh.shape[1] == self.views and wh.shape[2] == 2:
            if (wh != wh[:, :1]).any():
                raise ValueError("ResizeFiveCrop takes one size per image: its views are windows of one resized image")
            wh = wh[:, 0]
        from ._lib import ViewSizes, check_size, check_view_sizes

        if isinstance(check_view_sizes(size), ViewSizes):
            raise ValueError(f"{self!r} takes one size (h, w): torchvision's FiveCrop has one size")
        out_h, out_w = check_size(size)
        c = self._resize.sample(wh, status, size).astype(np.int64)  # res_h, res_w, centre top, centre left
        res_h, res_w, ct, cl = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
        zero, bottom, right = np.zeros_like(ct), res_h - out_h, res_w - out_w
        tl, tr, bl, br, ce = (zero, zero), (zero, right), (bottom, zero), (bottom, right), (ct, cl)
        order = [tl, tr, bl, br, ce]
        if self.ten:
            order += [tr, tl, br, bl, (ct, right - cl)]
        out = np.stack([np.stack([res_h, res_w, t, l], axis=1) for t, l in order], axis=1)
        known = (wh[:, 0] > 0) & (wh[:, 1] > 0)
        if status is not None:
            known &= np.asarray(status) == 0
        out[~known] = (out_h, out_w, 0, 0)
        return np.clip(out, -(1 << 31), (1 << 31) - 1).astype(np.int32)

    def boxes(self, wh, status=None) -> np.ndarray:
        """int32 ``[n, views, 5]``: the whole image in every view, flip 0 for
        views 0..4 and 1 for views 5..9; ``(0, 0, 1, 1, 0)`` for unknown rows."""
        wh = np.asarray(wh)
        if wh.ndim != 2 or wh.shape[1] != 2:
            raise ValueError(f"wh must have shape [n, 2] (width, height), got {wh.shape}")
        n = wh.shape[0]
        known = (wh[:, 0] > 0) & (wh[:, 1] > 0)
        if status is not None:
            known &= np.asarray(status) == 0
        out = np.zeros((n, self.views, 5), np.int32)
        out[:, :, 2] = np.where(known, wh[:, 1], 1)[:, None]
        out[:, :, 3] = np.where(known, wh[:, 0], 1)[:, None]
        out[:, 5:, 4] = known[:, None]
        return out

    def __repr__(self) -> str:
        return f"ResizeFiveCrop({self.edge}, ten={self.ten})"


# ---- the auto-augment family: ops on the resized image (``augment=``) ----

_AFFINE_OPS = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")
# torchvision's op names in the order of ``_augmentation_space`` (the op is
# drawn as an index into it), with ``check_augments``' op code; None: Identity
# (absent), "affine": through ``affine_matrix``.
_AUG_OPS = (("Identity", None), ("ShearX", "affine"), ("ShearY", "affine"), ("TranslateX", "affine"),
            ("TranslateY", "affine"), ("Rotate", "affine"), ("Brightness", 2), ("Color", 3), ("Contrast", 4),
            ("Sharpness", 5), ("Posterize", 6), ("Solarize", 7), ("AutoContrast", 8), ("Equalize", 9))


def _inverse_affine(center, angle, translate, scale, shear):
    """torchvision's ``_get_inverse_affine_matrix`` (inverted=True), step for
    step in Python floats: the output -> input matrix ``F.affine`` hands to
    ``Image.transform``."""
    rot = math.radians(angle)
    sx = math.radians(shear[0])
    sy = math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    matrix = [d, -b, 0.0, -c, a, 0.0]
    matrix = [x / scale for x in matrix]
    matrix[2] += matrix[0] * (-cx - tx) + matrix[1] * (-cy - ty)
    matrix[5] += matrix[3] * (-cx - tx) + matrix[4] * (-cy - ty)
    matrix[2] += cx
    matrix[5] += cy
    return matrix


def affine_matrix(op, magnitude, size):
    """The output -> input matrix ``(p0..p5)`` of one geometric op of the
    auto-augment family on a PIL image of ``size = (h, w)``, as torchvision's
    ``_apply_op`` reaches Pillow's ``Image.transform(size, AFFINE, matrix)``;
    the six floats ``check_augments`` takes for op 1.

    ``"ShearX"`` / ``"ShearY"``: ``F.affine`` with the shear in degrees of
    ``atan(magnitude)`` about the centre ``[0, 0]``. ``"TranslateX"`` /
    ``"TranslateY"``: ``F.affine`` with ``translate = int(magnitude)`` about the
    image's centre, an integer translation. ``"Rotate"``: Pillow's
    ``Image.rotate(magnitude)``: the angle modulo 360, ``round(cos, 15)`` and
    ``round(sin, 15)`` about ``(w / 2, h / 2)``; 0 is a copy, 180 a transpose,
    90 and 270 transposes on a square image only, and a transpose is an exact
    integer matrix (180: ``(-1, 0, w, 0, -1, h)``). Needs no device."""
    h, w = int(size[0]), int(size[1])
    magnitude = float(magnitude)
    if op == "ShearX":
        return _inverse_affine([0, 0], 0.0, [0, 0], 1.0, [math.degrees(math.atan(magnitude)), 0.0])
    if op == "ShearY":
        return _inverse_affine([0, 0], 0.0, [0, 0], 1.0, [0.0, math.degrees(math.atan(magnitude))])
    if op == "TranslateX":
        return _inverse_affine([w * 0.5, h * 0.5], 0.0, [int(magnitude), 0], 1.0, [0.0, 0.0])
    if op == "TranslateY":
        return _inverse_affine([w * 0.5, h * 0.5], 0.0, [0, int(magnitude)], 1.0, [0.0, 0.0])
    if op != "Rotate":
        raise ValueError(f"affine_matrix: op must be one of {_AFFINE_OPS}, got {op!r}")
    angle = magnitude % 360.0
    if angle == 0:
        return [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    if angle == 180:
        return [-1.0, 0.0, float(w), 0.0, -1.0, float(h)]
    if angle == 90 and w == h:  # Image.Transpose.ROTATE_90: out(x, y) = in(w - 1 - y, x)
        return [0.0, -1.0, float(w), 1.0, 0.0, 0.0]
    if angle == 270 and w == h:  # ROTATE_270: out(x, y) = in(y, h - 1 - x)
        return [0.0, 1.0, 0.0, -1.0, 0.0, float(h)]
    center = (w / 2, h / 2)
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0,
         round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]

    def transform(x, y):
        return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]

    m[2], m[5] = transform(-center[0], -center[1])
    m[2] += center[0]
    m[5] += center[1]
    return m


def _check_fill(fill):
    """None, a number or three of them, as torchvision's ``fill`` reaches a
    PIL RGB image: ints 0..255. Returns a 3-tuple."""
    if fill is None:
        return (0, 0, 0)
    vals = tuple(fill) if hasattr(fill, "__len__") else (fill,) * 3
    if len(vals) == 1:
        vals = vals * 3
    if len(vals) != 3 or any(isinstance(x, bool) or int(x) != x or not 0 <= int(x) <= 255 for x in vals):
        raise ValueError(f"fill must be None, an integer in 0..255 or three of them, got {fill!r}")
    return tuple(int(x) for x in vals)


def _check_nearest(interpolation):
    if interpolation is None:
        return
    v = getattr(interpolation, "value", interpolation)
    if not (v == 0 or (isinstance(v, str) and v.lower() == "nearest")):
        raise ValueError(f"interpolation={interpolation!r}: the fused affine op is Pillow's NEAREST, the recipes' "
                         "default; bilinear and bicubic are not built")


class RandomErasing:
    """torchvision's ``RandomErasing(p, scale, ratio, value=0)`` after
    ``ToTensor`` / ``Normalize``: per output image one box whose stored
    elements are zero. ``value=0`` only. Pass it as ``erase=`` of
    ``TrivialAugmentWide`` / ``RandAugment``, which draw its box after their
    own ops, or alone as ``augment=``.

    The draws follow ``forward`` and ``get_params`` with torch's RNG
    (``generator``, else the global one): ``rand(1) < p`` first; then up to 10
    attempts of the area (``uniform_``), the log-ratio (``uniform_``), ``h =
    int(round(sqrt(area * ratio)))``, ``w = int(round(sqrt(area / ratio)))``,
    accepted when ``h < H and w < W``, then ``randint(0, H - h + 1)`` and
    ``randint(0, W - w + 1)``; after 10 failures, no box. Picklable when
    ``generator`` is None."""

    def __init__(self, p=0.5, scale=(0.02, 0.33), ratio=(0.3, 3.3), value=0, generator=None):
        if value != 0 or isinstance(value, bool):
            raise ValueError(f"value={value!r}: only RandomErasing(value=0) is built")
        if not hasattr(scale, "__len__") or len(scale) != 2 or not hasattr(ratio, "__len__") or len(ratio) != 2:
            raise TypeError("scale and ratio should be pairs")
        self.p = float(p)
        self.scale = (float(scale[0]), float(scale[1]))
        self.ratio = (float(ratio[0]), float(ratio[1]))
        if not 0.0 <= self.p <= 1.0:
            raise ValueError("p should be in [0, 1]")
        if not 0.0 <= self.scale[0] <= self.scale[1] <= 1.0:
            raise ValueError("scale should be ordered and between 0 and 1")
        if not 0.0 < self.ratio[0] <= self.ratio[1]:
            raise ValueError("ratio should be positive and ordered")
        self.generator = generator

    def _box(self, H: int, W: int):
        """(top, left, height, width) for one H x W output image, height 0 = none."""
        g = self.generator
        if not torch.rand(1, generator=g).item() < self.p:
            return (0, 0, 0, 0)
        area = H * W
        log_ratio = torch.log(torch.tensor(self.ratio))
        for _ in range(10):
            erase_area = area * torch.empty(1).uniform_(self.scale[0], self.scale[1], generator=g).item()
            aspect = torch.exp(torch.empty(1).uniform_(float(log_ratio[0]), float(log_ratio[1]), generator=g)).item()
            h = int(round(math.sqrt(erase_area * aspect)))
            w = int(round(math.sqrt(erase_area / aspect)))
            if not (h < H and w < W):
                continue
            i = torch.randint(0, H - h + 1, size=(1,), generator=g).item()
            j = torch.randint(0, W - w + 1, size=(1,), generator=g).item()
            return (i, j, h, w) if h > 0 and w > 0 else (0, 0, 0, 0)
        return (0, 0, 0, 0)

    def sample(self, n, size, views=None) -> np.ndarray:
        """``aug_dtype()`` records ``[n]`` (``[n, V]``) with no ops and this
        batch's erase boxes."""
        return _sample_augments(None, self, n, size, views)

    def __repr__(self) -> str:
        return f"RandomErasing(p={self.p}, scale={self.scale}, ratio={self.ratio}, value=0)"


def _sample_augments(ops, erase, n, size, views):
    """The records of a batch: per image and view, ``ops``' draws (a sampler
    with ``_draw(h, w)`` giving rows of ``check_augments``, or None), then
    ``erase``'s box (a ``RandomErasing`` or None)."""
    from ._lib import MAX_AUG_OPS, ViewSizes, check_augments, check_view_sizes, check_views

    size = check_view_sizes(size)
    views = len(size) if isinstance(size, ViewSizes) else check_views(views)
    nv = 1 if views is None else views
    sizes = list(size) if isinstance(size, ViewSizes) else [size] * nv
    K = max(1, min(MAX_AUG_OPS, getattr(ops, "num_ops", 1)))
    arr = np.full((int(n), nv, K, 10), np.nan, np.float64)
    boxes = np.zeros((int(n), nv, 4), np.int64)
    for i in range(int(n)):
        for v, (h, w) in enumerate(sizes):
            if ops is not None:
                for k, row in enumerate(ops._draw(h, w)):
                    arr[i, v, k] = row
            if erase is not None:
                boxes[i, v] = erase._box(h, w)
    if views is None:
        arr, boxes = arr[:, 0], boxes[:, 0]
    return check_augments(arr, n, views, size, None if erase is None else boxes)


class _AutoAugmentBase:
    """What TrivialAugmentWide and RandAugment share: the op table, the row of
    one drawn op and the batch's records."""

    def _row(self, name, code, magnitude, h, w):
        """One row ``(op, p0..p5, fill_r, fill_g, fill_b)`` of ``check_augments``
        for torchvision's ``_apply_op(img, name, magnitude, NEAREST, fill)``."""
        row = [float("nan")] * 10
        if code is None:
            return row
        if code == "affine":
            row[0] = 1.0
            row[1:7] = affine_matrix(name, magnitude, (h, w))
            row[7:10] = [float(x) for x in self.fill]
        elif code in (2, 3, 4, 5):
            row[0], row[1] = float(code), 1.0 + magnitude
        elif code == 6:
            row[0], row[1] = 6.0, float(int(magnitude))
        elif code == 7:
            row[0], row[1] = 7.0, magnitude
        else:
            row[0] = float(code)
        return row

    def sample(self, n, size, views=None) -> np.ndarray:
        """``aug_dtype()`` records ``[n]`` (``[n, V]`` with ``views=V`` or a
        size list) for a batch of ``n`` images whose output size is ``size``
        (a pair ``(h, w)`` or one per view), drawn per image and view: the ops,
        then ``erase``'s box."""
        return _sample_augments(self, self.erase, n, size, views)


class TrivialAugmentWide(_AutoAugmentBase):
    """torchvision's ``TrivialAugmentWide(num_magnitude_bins, NEAREST, fill)``
    on the resized uint8 image, as ``augment=`` of the decode: one op per
    output image, bit-exact with the PIL path. Only the parameters are drawn
    here, with torch's RNG (``generator``, else the global one) in
    torchvision's order: ``randint(14)`` for the op over Identity, ShearX,
    ShearY, TranslateX, TranslateY, Rotate, Brightness, Color, Contrast,
    Sharpness, Posterize, Solarize, AutoContrast, Equalize; ``randint(bins)``
    for the magnitude when the op has bins; ``randint(2)`` for the sign when
    the op is signed. ``fill``: None, an int 0..255 or three. ``erase``: an
    optional ``RandomErasing`` whose box is drawn after the op, per output
    image. Picklable when ``generator`` is None."""

    num_ops = 1

    def __init__(self, num_magnitude_bins=31, interpolation=None, fill=None, generator=None, erase=None):
        _check_nearest(interpolation)
        if isinstance(num_magnitude_bins, bool) or int(num_magnitude_bins) != num_magnitude_bins or \
                num_magnitude_bins < 2:
            raise ValueError(f"num_magnitude_bins must be an int >= 2, got {num_magnitude_bins!r}")
        self.num_magnitude_bins = int(num_magnitude_bins)
        self.fill = _check_fill(fill)
        self.generator = generator
        if erase is not None and not isinstance(erase, RandomErasing):
            raise TypeError(f"erase must be a RandomErasing or None, got {erase!r}")
        self.erase = erase

    @staticmethod
    @functools.lru_cache(maxsize=8)  # built once per bin count, not per image; the tensors are only read
    def _space(num_bins, h=None, w=None):
        lin = torch.linspace
        return (
            (torch.tensor(0.0), False),
            (lin(0.0, 0.99, num_bins), True), (lin(0.0, 0.99, num_bins), True),
            (lin(0.0, 32.0, num_bins), True), (lin(0.0, 32.0, num_bins), True),
            (lin(0.0, 135.0, num_bins), True),
            (lin(0.0, 0.99, num_bins), True), (lin(0.0, 0.99, num_bins), True),
            (lin(0.0, 0.99, num_bins), True), (lin(0.0, 0.99, num_bins), True),
            (8 - (torch.arange(num_bins) / ((num_bins - 1) / 6)).round().int(), False),
            (lin(255.0, 0.0, num_bins), False),
            (torch.tensor(0.0), False), (torch.tensor(0.0), False),
        )

    def _draw(self, h, w):
        g = self.generator
        space = self._space(self.num_magnitude_bins)  # the wide space does not depend on the size
        idx = int(torch.randint(len(space), (1,), generator=g).item())
        magnitudes, signed = space[idx]
        magnitude = float(magnitudes[torch.randint(len(magnitudes), (1,), dtype=torch.long, generator=g)].item()) \
            if magnitudes.ndim > 0 else 0.0
        if signed and torch.randint(2, (1,), generator=g):
            magnitude *= -1.0
        name, code = _AUG_OPS[idx]
        return [self._row(name, code, magnitude, h, w)]

    def __repr__(self) -> str:
        return (f"TrivialAugmentWide(num_magnitude_bins={self.num_magnitude_bins}, fill={self.fill}"
                + ("" if self.erase is None else f", erase={self.erase!r}") + ")")


class RandAugment(_AutoAugmentBase):
    """torchvision's ``RandAugment(num_ops, magnitude, num_magnitude_bins,
    NEAREST, fill)`` on the resized uint8 image, as ``augment=`` of the decode:
    ``num_ops`` (at most 4) ops per output image at one magnitude bin,
    bit-exact with the PIL path. Per op it draws ``randint(14)`` for the op,
    then ``randint(2)`` for the sign when the op is signed. The bins are
    torchvision's: shear 0.3, translate ``150 / 331`` of the view's width /
    height, rotate 30, the enhance ops 0.9, posterize ``8 - round(i / ((bins -
    1) / 4))``, solarize from 255 down to 0. ``fill``, ``erase``,
    ``generator``: as for ``TrivialAugmentWide``."""

    def __init__(self, num_ops=2, magnitude=9, num_magnitude_bins=31, interpolation=None, fill=None, generator=None,
                 erase=None):
        from ._lib import MAX_AUG_OPS

        _check_nearest(interpolation)
        for name, v, lo in (("num_ops", num_ops, 0), ("num_magnitude_bins", num_magnitude_bins, 2)):
            if isinstance(v, bool) or int(v) != v or v < lo:
                raise ValueError(f"{name} must be an int >= {lo}, got {v!r}")
        if num_ops > MAX_AUG_OPS:
            raise ValueError(f"num_ops={num_ops!r}: an output image takes at most {MAX_AUG_OPS} ops")
        if isinstance(magnitude, bool) or int(magnitude) != magnitude or not 0 <= magnitude < num_magnitude_bins:
            raise ValueError(f"magnitude must be an int in 0..{int(num_magnitude_bins) - 1}, got {magnitude!r}")
        self.num_ops = int(num_ops)
        self.magnitude = int(magnitude)
        self.num_magnitude_bins = int(num_magnitude_bins)
        self.fill = _check_fill(fill)
        self.generator = generator
        if erase is not None and not isinstance(erase, RandomErasing):
            raise TypeError(f"erase must be a RandomErasing or None, got {erase!r}")
        self.erase = erase

    @staticmethod
    @functools.lru_cache(maxsize=64)  # built once per bin count and view size, not per image
    def _space(num_bins, h, w):
        lin = torch.linspace
        return (
            (torch.tensor(0.0), False),
            (lin(0.0, 0.3, num_bins), True), (lin(0.0, 0.3, num_bins), True),
            (lin(0.0, 150.0 / 331.0 * w, num_bins), True), (lin(0.0, 150.0 / 331.0 * h, num_bins), True),
            (lin(0.0, 30.0, num_bins), True),
            (lin(0.0, 0.9, num_bins), True), (lin(0.0, 0.9, num_bins), True),
            (lin(0.0, 0.9, num_bins), True), (lin(0.0, 0.9, num_bins), True),
            (8 - (torch.arange(num_bins) / ((num_bins - 1) / 4)).round().int(), False),
            (lin(255.0, 0.0, num_bins), False),
            (torch.tensor(0.0), False), (torch.tensor(0.0), False),
        )

    def _draw(self, h, w):
        g = self.generator
        space = self._space(self.num_magnitude_bins, h, w)
        rows = []
        for _ in range(self.num_ops):
            idx = int(torch.randint(len(space), (1,), generator=g).item())
            magnitudes, signed = space[idx]
            magnitude = float(magnitudes[self.magnitude].item()) if magnitudes.ndim > 0 else 0.0
            if signed and torch.randint(2, (1,), generator=g):
                magnitude *= -1.0
            name, code = _AUG_OPS[idx]
            rows.append(self._row(name, code, magnitude, h, w))
        return rows

    def __repr__(self) -> str:
        return (f"RandAugment(num_ops={self.num_ops}, magnitude={self.magnitude}, "
                f"num_magnitude_bins={self.num_magnitude_bins}, fill={self.fill}"
                + ("" if self.erase is None else f", erase={self.erase!r}") + ")")


def _mix_lam(alpha, g) -> float:
    """``Beta(alpha, alpha)`` as torchvision v2's MixUp / CutMix draw it
    (``torch.distributions.Beta.sample`` is one ``_sample_dirichlet`` call)."""
    return float(torch._sample_dirichlet(torch.tensor([[alpha, alpha]]), generator=g)[..., 0])


def _mix_rows(n, w_self, w_partner, box, lw_self, lw_partner):
    from ._lib import mix_dtype

    rows = np.zeros(n, mix_dtype())
    rows["partner"] = (np.arange(n) - 1) % max(n, 1)  # inpt.roll(1, 0): row i gets row i - 1
    rows["w_self"], rows["w_partner"] = np.float32(w_self), np.float32(w_partner)
    rows["box"] = np.asarray(box, np.int32)
    rows["lw_self"], rows["lw_partner"] = np.float32(lw_self), np.float32(lw_partner)
    return rows


class _MixBase:
    def __init__(self, alpha=1.0, num_classes=None, generator=None):
        from ._lib import MIX_MAX_CLASSES

        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not (alpha > 0 and math.isfinite(alpha)):
            raise ValueError(f"alpha must be a positive number, got {alpha!r}")
        if num_classes is None:
            raise ValueError("num_classes is needed for the soft labels (0: mix the images only)")
        if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or \
                not 0 <= int(num_classes) <= MIX_MAX_CLASSES:
            raise ValueError(f"num_classes must be an integer in 0..{MIX_MAX_CLASSES}, got {num_classes!r}")
        self.alpha = float(alpha)
        self.num_classes = int(num_classes)
        self.generator = generator

    def sample(self, n, size):
        """``(records, num_classes)`` for a batch of ``n`` rows whose output
        size is ``size`` = (h, w): what ``check_mixes`` takes."""
        return self._rows(int(n), size), self.num_classes

    def __repr__(self) -> str:
        return f"{type(self).__name__}(alpha={self.alpha}, num_classes={self.num_classes})"


class MixUp(_MixBase):
    """torchvision v2's ``MixUp(alpha, num_classes)`` for ``mix=``: one draw
    per batch with torch's RNG (``generator``, else the global one), ``lam =
    Beta(alpha, alpha)`` as one ``torch._sample_dirichlet`` call; every row is
    mixed with the row before it (``inpt.roll(1, 0)``), image and label weights
    ``float32(lam)`` for the row and ``float32(1.0 - lam)`` for its partner, no
    box. Picklable when ``generator`` is None."""

    def _rows(self, n, size):
        lam = _mix_lam(self.alpha, self.generator)
        return _mix_rows(n, lam, 1.0 - lam, (0, 0, 0, 0), lam, 1.0 - lam)


class CutMix(_MixBase):
    """torchvision v2's ``CutMix(alpha, num_classes)`` for ``mix=``: one draw
    per batch in torchvision's order: ``lam = Beta(alpha, alpha)``, ``r_x =
    randint(W)``, ``r_y = randint(H)``; the box of half sides ``int(0.5 *
    sqrt(1 - lam) * W)`` and ``... * H`` around ``(r_x, r_y)`` clipped to the
    image takes the partner's pixels (the row before, ``inpt.roll(1, 0)``), and
    the label weights are the area's share: ``float32(lam_adj)`` and
    ``float32(1.0 - lam_adj)`` with ``lam_adj = 1 - box area / (W * H)``. An
    empty box is no box. Picklable when ``generator`` is None."""

    def _rows(self, n, size):
        g = self.generator
        H, W = int(size[0]), int(size[1])
        lam = _mix_lam(self.alpha, g)
        r_x = int(torch.randint(W, (1,), generator=g))
        r_y = int(torch.randint(H, (1,), generator=g))
        r = 0.5 * math.sqrt(1.0 - lam)
        r_w_half, r_h_half = int(r * W), int(r * H)
        x1, y1 = max(r_x - r_w_half, 0), max(r_y - r_h_half, 0)
        x2, y2 = min(r_x + r_w_half, W), min(r_y + r_h_half, H)
        lam_adj = float(1.0 - (x2 - x1) * (y2 - y1) / (W * H))
        box = (y1, x1, y2 - y1, x2 - x1) if y2 > y1 and x2 > x1 else (0, 0, 0, 0)
        return _mix_rows(n, 1.0, 0.0, box, lam_adj, 1.0 - lam_adj)


class MixChoice:
    """torchvision's ``RandomChoice([MixUp(...), CutMix(...)], p)`` for
    ``mix=``: per batch ``idx = int(torch.multinomial(tensor([q / sum(p) for q
    in p]), 1, generator=g))``, then that member's own draws. ``p=None`` is
    uniform. The members must agree on ``num_classes``. ``generator``: None
    leaves each member its own; otherwise it is used for the choice and handed
    to every member. Picklable when every generator is None."""

    def __init__(self, mixes, p=None, generator=None):
        mixes = list(mixes)
        if not mixes or not all(isinstance(m, _MixBase) for m in mixes):
            raise ValueError("MixChoice takes a non-empty list of MixUp / CutMix samplers")
        if len({m.num_classes for m in mixes}) != 1:
            raise ValueError(f"MixChoice: the members disagree on num_classes "
                             f"({[m.num_classes for m in mixes]})")
        if p is None:
            p = [1.0] * len(mixes)
        p = [float(q) for q in p]
        if len(p) != len(mixes) or any(not (q >= 0 and math.isfinite(q)) for q in p) or not sum(p) > 0:
            raise ValueError(f"MixChoice: p must hold one non-negative weight per member with a positive sum, got {p}")
        self.mixes, self.p = mixes, p
        self.num_classes = mixes[0].num_classes
        self.generator = generator
        if generator is not None:
            for m in mixes:
                m.generator = generator

    def sample(self, n, size):
        total = sum(self.p)
        idx = int(torch.multinomial(torch.tensor([q / total for q in self.p]), 1, generator=self.generator))
        return self.mixes[idx].sample(n, size)

    def __repr__(self) -> str:
        return f"MixChoice({self.mixes!r}, p={self.p})"
