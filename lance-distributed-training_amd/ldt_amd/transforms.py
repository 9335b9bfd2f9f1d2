"""Drop-in replacements for the reference's batch transforms.

* ``decode_tensor_image(batch, **kwargs)`` — the iterable ``to_tensor_fn``
  (reference ``lance_iterable.py:38-50``, registered with
  ``LanceDataset(..., to_tensor_fn=decode_tensor_image)`` at ``:53-59``).
* ``collate_fn(batch_of_dicts)`` — the map-style ``collate_fn``
  (reference ``lance_map_style.py:21-44``, passed to ``get_safe_loader`` at
  ``:60-69``).

Both return ``{"image": float32[N,3,224,224], "label": int64[N]}`` exactly
like the reference (PIL ``open -> convert("RGB") -> Resize((224,224)) ->
ToTensor -> stack``), bit-exact, except that the tensors are already on the
GPU, and that ``size=(h, w)`` (torchvision's ``Resize((h, w))`` order, each in
1..1024; ``None`` = (224, 224)) selects another output size, bit-exact with
Pillow's BILINEAR resize to it, and ``interpolation="bicubic"`` (torchvision's
``interpolation=``; None = bilinear) selects Pillow's BICUBIC, bit-exact too.
``dtype=`` (``torch.float16``, ``torch.bfloat16``, ``torch.uint8``; None =
float32) and ``memory_format=torch.channels_last`` have the resize kernel store
the image in that element type and layout itself, bit-identical to the float32
result converted by torch, so no conversion pass follows the decode.
The tensors are on the GPU
(``cuda:{LOCAL_RANK}``), so the consumer's ``.to(device)``
(``lance_iterable.py:108-109``) is a no-op. All arithmetic runs in libldt.so's
gfx950 kernels; Python only hands over Arrow buffer addresses.

Inside a torch DataLoader worker (``num_workers > 0``: lance_map_style.py:60-69
with 8 spawn workers, lance_iterable.py:71-72 under ``--no_ddp``) the workers
never touch the GPU. There the plug-ins return a ``DeviceBatch``: the batch's
compressed cells packed into shared-memory tensors, which the DataLoader moves
to the main process. The GPU decode then runs in the main process — in the
DataLoader's pin-memory thread when ``pin_memory=True`` (so it overlaps the
training step), otherwise when the batch is first indexed. Decoded tensors are
``DeviceTensor``s, whose ``pin_memory()`` is the identity, so
``pin_memory=True`` also works when the collate runs in the main process.
"""
from __future__ import annotations

import ctypes
import os
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np
import pyarrow as pa
import torch

from . import _lib
from ._lib import (ImageDecodeError, Norm, check_augments, check_colors, check_crops, check_drafts, check_format,
                   check_interpolation, check_mix_labels, check_mixes, check_view_sizes, check_views, check_windows,
                   draft_sizes, ViewSizes)

IMAGENET_MEAN = (0.485, 0.456, 0.406)  # lance_iterable.py:31 (commented out there)
IMAGENET_STD = (0.229, 0.224, 0.225)


def default_device() -> torch.device:
    """cuda:{LOCAL_RANK} as the reference training loop picks (lance_iterable.py:83)."""
    if not torch.cuda.is_available():
        raise RuntimeError("ldt_amd needs a HIP device (MI355X); no CPU fallback exists")
    return torch.device("cuda", int(os.environ.get("LOCAL_RANK", torch.cuda.current_device())))


def _norm_struct(normalize) -> Optional[Norm]:
    if not normalize:
        return None
    if normalize is True:
        mean, std = IMAGENET_MEAN, IMAGENET_STD
    else:
        mean, std = normalize
    n = Norm()
    for c in range(3):
        n.mean[c] = float(mean[c])
        n.std[c] = float(std[c])
    return n


def _column(batch, name: str):
    if isinstance(batch, pa.RecordBatch):
        return batch.column(batch.schema.get_field_index(name))
    if isinstance(batch, pa.Table):
        col = batch.column(name)
        return col.combine_chunks() if col.num_chunks != 1 else col.chunk(0)
    raise TypeError(f"expected pyarrow.RecordBatch, got {type(batch).__name__}")


def _labels_buffer(batch, label_column: str):
    """(address, offset, keepalive) of an int64 label column, or None."""
    if label_column is None:
        return None
    names = batch.schema.names
    if label_column not in names:
        return None
    lab = _column(batch, label_column)
    if lab.null_count:
        raise ValueError(f"null values in label column {label_column!r}")
    if lab.type != pa.int64():
        lab = lab.cast(pa.int64())
    bufs = lab.buffers()
    return bufs[1].address, lab.offset, lab


class _Decoder:
    def __init__(self, device: torch.device):
        self.device = device
        self.ctx = _lib.get_context(device.index)


_decoders: dict = {}


def _decoder(device) -> _Decoder:
    dev = torch.device(device) if device is not None else default_device()
    if dev.type != "cuda":
        raise ValueError(f"ldt_amd decodes on a HIP device, got {dev}")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    d = _decoders.get(dev.index)
    if d is None:
        d = _Decoder(dev)
        _decoders[dev.index] = d
    return d


_TORCH_DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16,
                 "uint8": torch.uint8}


def _default_format(dtype: str, memory_format: str) -> bool:
    return dtype == _lib.DEFAULT_DTYPE and memory_format == _lib.DEFAULT_MEMORY_FORMAT


def _format_strides(n: int, size, memory_format: str):
    h, w = size
    return (3 * h * w, 1, 3 * w, 3) if memory_format == "channels_last" else (3 * h * w, h * w, w, 1)


def _empty_image(n: int, size, dtype: str, memory_format: str, device, views=None) -> torch.Tensor:
    """The output tensor of a decode / resize call: ``[n, 3, h, w]`` of
    ``dtype``, contiguous, or with channels_last's strides exactly
    ``(3*h*w, 1, 3*w, 3)`` (a permuted view of an ``[n, h, w, 3]``
    allocation, so they hold when h or w is 1 too). ``views`` (an int):
    ``[views, n, 3, h, w]``, one allocation, each ``out[v]`` as above. A
    ``ViewSizes`` as ``size``: the flat allocation of ``n * 3 * sum(h * w)``
    elements that ``_split_views`` cuts into the result."""
    if isinstance(size, ViewSizes):
        return torch.empty((n * size.elements,), dtype=_TORCH_DTYPES[dtype], device=device)
    if views is not None:
        if memory_format == "channels_last":
            return torch.empty((views, n, size[0], size[1], 3), dtype=_TORCH_DTYPES[dtype],
                               device=device).permute(0, 1, 4, 2, 3)
        return torch.empty((views, n, 3) + tuple(size), dtype=_TORCH_DTYPES[dtype], device=device)
    if memory_format == "channels_last":
        return torch.empty((n, size[0], size[1], 3), dtype=_TORCH_DTYPES[dtype], device=device).permute(0, 3, 1, 2)
    return torch.empty((n, 3) + tuple(size), dtype=_TORCH_DTYPES[dtype], device=device)


def _split_views(flat: torch.Tensor, n: int, sizes, memory_format: str, wrap=None):
    """The result of a call with a size list: a tuple of tensors, one per run
    of consecutive equal sizes, each ``[V_run, n, 3, h, w]``, view-major and
    dense (with channels_last's strides under that format), each a view into
    ``flat`` (1-D, ``n * 3 * sum(h * w)`` elements): view ``v`` starts at
    element ``n * 3 * sum(h_u * w_u for u < v)``. ``wrap``: a tensor subclass
    for the pieces."""
    out, at = [], 0
    for _, count, (h, w) in sizes.runs():
        cell = 3 * h * w
        shape = (count, n, 3, h, w)
        strides = (n * cell, cell, 1, 3 * w, 3) if memory_format == "channels_last" else (n * cell, cell, h * w, w, 1)
        t = flat.as_strided(shape, strides, flat.storage_offset() + at)
        out.append(t if wrap is None else t.as_subclass(wrap))
        at += count * n * cell
    return tuple(out)


def _check_out(out, n: int, size, dtype: str, memory_format: str, views=None) -> None:
    """A caller's ``out=`` under a non-default format: its dtype, shape and
    strides must be the format's (the library writes ``n * 3 * h * w``
    elements from ``out.data_ptr()`` in that layout). Under the defaults it is
    taken on trust, as it always was. With ``views`` (an int) it is always
    checked: ``[views, n, 3, h, w]`` of the call's dtype, the views
    ``n * 3 * h * w`` elements apart and each ``out[v]`` with the format's
    strides. With a ``ViewSizes`` as ``size``: a 1-D contiguous tensor of the
    call's dtype with exactly ``n * 3 * sum(h * w)`` elements."""
    if isinstance(size, ViewSizes):
        if not isinstance(out, torch.Tensor) or out.dim() != 1 or (out.numel() > 1 and out.stride(0) != 1):
            raise ValueError(f"out= with a size list must be a 1-D dense tensor, got shape "
                             f"{tuple(getattr(out, 'shape', ()))}")
        if out.dtype != _TORCH_DTYPES[dtype]:
            raise ValueError(f"out= has dtype {out.dtype}, the call's dtype is {_TORCH_DTYPES[dtype]}")
        if out.numel() != n * size.elements:
            raise ValueError(f"out= has {out.numel()} elements, the call writes n * 3 * sum(h * w) = "
                             f"{n * size.elements} (n={n}, size={list(size)})")
        return
    if views is not None:
        shape = (views, n, 3) + tuple(size)
        if out.dtype != _TORCH_DTYPES[dtype]:
            raise ValueError(f"out= has dtype {out.dtype}, the call's dtype is {_TORCH_DTYPES[dtype]}")
        if tuple(out.shape) != shape:
            raise ValueError(f"out= has shape {tuple(out.shape)}, the call writes {shape} (views={views})")
        want = (n * 3 * size[0] * size[1],) + _format_strides(n, size, memory_format)
        bad = [d for d in range(5) if shape[d] > 1 and out.stride(d) != want[d]]
        if bad:
            raise ValueError(f"out= has strides {tuple(out.stride())}, views={views} with "
                             f"memory_format={memory_format!r} needs {want}")
        return
    if _default_format(dtype, memory_format):
        return
    shape = (n, 3) + tuple(size)
    if out.dtype != _TORCH_DTYPES[dtype]:
        raise ValueError(f"out= has dtype {out.dtype}, the call's dtype is {_TORCH_DTYPES[dtype]}")
    if tuple(out.shape) != shape:
        raise ValueError(f"out= has shape {tuple(out.shape)}, the call writes {shape}")
    want = _format_strides(n, size, memory_format)
    bad = [d for d in range(4) if shape[d] > 1 and out.stride(d) != want[d]]
    if bad:
        raise ValueError(f"out= has strides {tuple(out.stride())}, memory_format={memory_format!r} needs {want}")


def _resolve_views(views, crop, window, size=None):
    """The ``views`` of a call from its ``views=``, ``crop=`` and ``window=``
    arguments: ``check_views(views)``, or the ``.views`` of a window object
    that has them (``ResizeFiveCrop``), which an explicit ``views=`` must
    equal. A window object that supplies the boxes too (``ten=True``) excludes
    a ``crop=``. ``size``: the call's validated size; a size list
    (``ViewSizes``) implies its own length, which an explicit ``views=`` must
    equal, and excludes a ``ResizeFiveCrop`` (torchvision's has one size)."""
    views = check_views(views)
    wv = getattr(window, "views", None) if hasattr(window, "sample") else None
    if isinstance(size, ViewSizes):
        if views is not None and views != len(size):
            raise ValueError(f"views={views} with a size list of {len(size)} views")
        if wv is not None:
            raise ValueError(f"window={window!r} takes its {wv} views at one size: size= must be a pair (h, w)")
        return len(size)
    if wv is not None:
        if views is not None and views != wv:
            raise ValueError(f"views={views} with window={window!r}, which has {wv} views")
        if getattr(window, "ten", False) and crop is not None:
            raise ValueError(f"window={window!r} supplies the flips of its mirrored views as crops: crop= must be None")
        views = wv
    return views


def _resolve_crop(crop, images, views=None, window=None, sizes=None):
    """What a ``crop=`` argument means for the cells ``images`` (an Arrow
    array or a list of bytes): None, the caller's ``[n, 5]`` array as it is,
    or the boxes a sampler (``RandomResizedCropFlip``: anything with
    ``sample``) draws for the cells' header sizes, here and now, in the
    process that decodes. ``views`` (an int): the sampler draws ``[n, views,
    5]``. ``window``: the call's window argument; without a ``crop`` a
    ``ResizeFiveCrop(ten=True)`` supplies the boxes (whole image, the mirrored
    views flipped). ``sizes``: ``image_sizes(images)`` when the caller has it."""
    if crop is None and getattr(window, "ten", False) and hasattr(window, "boxes"):
        wh, status = sizes if sizes is not None else _lib.image_sizes(images)
        return window.boxes(wh, status)
    if crop is None or not hasattr(crop, "sample"):
        return crop
    wh, status = sizes if sizes is not None else _lib.image_sizes(images)
    return crop.sample(wh, status) if views is None else crop.sample(wh, status, views=views)


def _resolve_window(window, images, crops, size, sizes=None, views=None):
    """What a ``window=`` argument means for the cells ``images``: None, the
    caller's ``[n, 4]`` array as it is, or the windows a ``ResizeCenterCrop``
    (anything with ``sample``) computes for output size ``size`` from the
    sizes of what is resized: the rows' boxes when ``crops`` (already
    resolved, see ``_resolve_crop``) is given, else the cells' header sizes
    (``sizes``: ``image_sizes(images)`` when the caller has it already).
    ``views`` (an int): the boxes are ``[n, views, 5]`` and the result ``[n,
    views, 4]``."""
    if window is None or not hasattr(window, "sample"):
        return window
    wh, status = sizes if sizes is not None else _lib.image_sizes(images)
    if crops is not None:
        boxes = check_crops(crops, len(wh), views)
        wh = np.stack([boxes[..., 3], boxes[..., 2]], axis=-1)
    return window.sample(wh, status, size) if views is None else window.sample(wh, status, size, views=views)


def _resolve_color(color, n: int, views=None):
    """What a ``color=`` argument means for a batch of ``n`` cells: None, the
    caller's ``[n, 7]`` (``[n, views, 7]``) array as it is, or the rows a
    sampler (``ColorJitterParams``: anything with ``sample``) draws, here and
    now, in the process that decodes."""
    if color is None or not hasattr(color, "sample"):
        return color
    return color.sample(n) if views is None else color.sample(n, views=views)


def _resolve_augment(augment, n: int, size, views=None, color=None):
    """What an ``augment=`` argument means for a batch of ``n`` cells whose
    output size is ``size`` (validated): None, the caller's array or records
    through ``check_augments``, or the records a sampler
    (``TrivialAugmentWide``, ``RandAugment``, ``RandomErasing``: anything with
    ``sample``) draws, here and now, in the process that decodes. With
    ``color`` too it is a ``ValueError``: the two stages do not compose. Needs
    no device."""
    if augment is None:
        return None
    if color is not None:
        raise ValueError(_COLOR_AND_AUGMENT)
    if hasattr(augment, "sample"):
        augment = augment.sample(n, size, views=None if isinstance(size, ViewSizes) else views)
    return check_augments(augment, n, views, size)


def _resolve_mix(mix, n: int, size):
    """What a ``mix=`` argument means for a batch of ``n`` cells whose output
    size is ``size`` (validated): None, the caller's ``(rows, num_classes)``
    through ``check_mixes``, or what a sampler (``MixUp``, ``CutMix``,
    ``MixChoice``: anything with ``sample``) draws, here and now, in the
    process that decodes. Needs no device."""
    if mix is None:
        return None
    if hasattr(mix, "sample"):
        mix = mix.sample(n, size)
    return check_mixes(mix, n, size)


def _check_mix_call(mix, size, views, window, dtype) -> None:
    """A call's ``mix=`` against its other options (``CallSpec.make``)."""
    if mix is None:
        return
    if isinstance(size, ViewSizes) or views is not None:
        raise ValueError("mix= with views=, a size list or a ResizeFiveCrop: the mix stage pairs the rows of a "
                         "single-view batch")
    if dtype == "uint8":
        raise ValueError("mix= with dtype=torch.uint8: the mix is float32 arithmetic on the ToTensor / Normalize values")
    if not hasattr(mix, "sample") and (not isinstance(mix, (tuple, list)) or len(mix) != 2):
        raise ValueError(f"mix must be None, a sampler or a pair (rows, num_classes), got {type(mix).__name__}")


def _resolve_draft(draft, n: int, sizes=None):
    """What a ``draft=`` argument means for a batch of ``n`` cells: None, the
    caller's ``[n]`` array of scales through ``check_drafts``, or the scales a
    ``Draft`` (anything with ``sample``) computes from the cells' header sizes
    ``sizes = image_sizes(images)``. No RNG."""
    if draft is not None and hasattr(draft, "sample"):
        draft = draft.sample(*sizes)
    return check_drafts(draft, n)


class _Drawn(tuple):
    """``CallSpec.resolve``'s result: the five-tuple ``(crops, windows,
    colors, augments, mixes)`` it always was, with the batch's draft scales
    (``check_drafts``'s array, or None) as ``.drafts``."""

    drafts = None

    def __new__(cls, items, drafts=None):
        self = super().__new__(cls, items)
        self.drafts = drafts
        return self


_COLOR_AND_AUGMENT = ("color= and augment= in one call: the photometric stage and the auto-augment stage do not "
                      "compose (timm switches its colour jitter off under auto-augment)")


class CallSpec:
    """The validated options of one decode call, gathered once: what every
    surface builds from its keywords, what travels with a ``DeviceBatch`` to
    the process that decodes, and what the decode itself reads. ``normalize``
    as given; ``size`` a pair or a ``ViewSizes``; ``interpolation``, ``dtype``,
    ``memory_format`` names; ``views`` None or an int; ``crop``, ``window``,
    ``color``, ``augment`` None, an array (checked against a batch by
    ``check_arrays`` / ``resolve``) or a sampler (anything with ``sample``),
    which draws in ``resolve``, in the process that decodes; ``mix`` None, a
    pair ``(rows, num_classes)`` or a sampler likewise; ``draft`` None, an int
    ``[n]`` array of libjpeg scales (``check_drafts``) or a ``Draft``, which
    computes them from the header sizes in ``resolve``. Picklable."""

    __slots__ = ("normalize", "size", "interpolation", "dtype", "memory_format", "views", "draft", "crop", "window",
                 "color", "augment", "mix")

    @classmethod
    def make(cls, normalize=None, size=None, interpolation=None, dtype=None, memory_format=None, views=None,
             crop=None, window=None, color=None, augment=None, mix=None, draft=None) -> "CallSpec":
        """The one constructor: validates in the order every surface reports a
        call's bad options in. Needs no device and no batch."""
        spec = cls()
        spec.normalize = normalize
        spec.size = check_view_sizes(size)
        spec.interpolation = check_interpolation(interpolation)
        spec.dtype, spec.memory_format = check_format(dtype, memory_format, normalize)
        spec.views = _resolve_views(views, crop, window, spec.size)
        if color is not None and augment is not None:
            raise ValueError(_COLOR_AND_AUGMENT)
        _check_mix_call(mix, spec.size, spec.views, window, spec.dtype)
        spec.crop, spec.window, spec.color, spec.augment, spec.mix = crop, window, color, augment, mix
        if draft is not None and not hasattr(draft, "sample") and np.ndim(draft) != 1:
            raise ValueError(f"draft must be None, a Draft or an int array [n] of scales 1, 2, 4 or 8, got {draft!r}")
        spec.draft = draft
        return spec

    def _replace(self, **fields) -> "CallSpec":
        spec = CallSpec()
        for name in self.__slots__:
            setattr(spec, name, fields.get(name, getattr(self, name)))
        return spec

    def check_arrays(self, n: int) -> "CallSpec":
        """The spec with its arrays checked for a batch of ``n`` cells, before
        any device is asked for (they travel as the checked arrays and
        records); samplers are left alone: they draw in the process that
        decodes."""
        keep = lambda x: hasattr(x, "sample")  # noqa: E731
        return self._replace(
            draft=self.draft if keep(self.draft) else check_drafts(self.draft, n),
            crop=self.crop if keep(self.crop) else check_crops(self.crop, n, self.views),
            window=self.window if keep(self.window) else check_windows(self.window, n, self.views),
            color=self.color if keep(self.color) else check_colors(self.color, n, self.views),
            augment=self.augment if keep(self.augment) else check_augments(self.augment, n, self.views, self.size),
            mix=self.mix if keep(self.mix) else check_mixes(self.mix, n, self.size))

    def resolve(self, images=None, sizes=None, n=None):
        """``(crops, windows, colors, augments, mixes)`` of one batch, checked and
        ready for ``Context.arm``, with the batch's draft scales as the
        result's ``.drafts``: arrays as they are, samplers drawn here and
        now, each exactly once and in this order, which is part of the
        contract (seeded samplers reproduce torchvision's draw order): first
        the draft (a ``Draft`` reads the header sizes and draws nothing), whose
        drafted sizes ``ceil(size / scale)`` are what every sampler below is
        handed, so each draws and computes what torchvision would on the
        drafted PIL image; then the
        boxes (a ``ResizeFiveCrop(ten=True)`` window supplies them), the
        windows, the colours, the augments, the mix (last, as a collate-time
        transform draws). ``images``: the cells (an Arrow
        array or a list of bytes), or ``sizes``: their ``image_sizes`` when the
        caller has them, or a callable that gives them (called only when a
        sampler wants them); ``n``: their number."""
        wanted = hasattr(self.crop, "sample") or hasattr(self.window, "sample") or hasattr(self.draft, "sample")
        if callable(sizes):
            sizes = sizes() if wanted else None
        elif sizes is None and wanted:
            sizes = _lib.image_sizes(images)
        if n is None:
            n = len(images) if images is not None else len(sizes[0])
        drafts = _resolve_draft(self.draft, n, sizes)
        if drafts is not None and sizes is not None:
            sizes = (draft_sizes(sizes[0], drafts), sizes[1])  # the samplers see the drafted image
        crops = check_crops(_resolve_crop(self.crop, images, self.views, self.window, sizes), n, self.views)
        windows = check_windows(_resolve_window(self.window, images, crops, self.size, sizes, self.views), n,
                                self.views)
        colors = check_colors(_resolve_color(self.color, n, self.views), n, self.views)
        augments = _resolve_augment(self.augment, n, self.size, self.views)
        return _Drawn((crops, windows, colors, augments, _resolve_mix(self.mix, n, self.size)), drafts)

    def override(self, crops=None, windows=None, interpolation=None, colors=None, augments=None,
                 normalize=None, mixes=None, drafts=None) -> "CallSpec":
        """The spec of one batch of a pipeline: the call's own crops, windows,
        filter, colours, augments and Normalize in place of the pipeline's
        where given. A window object of the call's must have the views the
        pipeline was built with (it allocates the outputs)."""
        if all(x is None for x in (crops, windows, interpolation, colors, augments, normalize, mixes, drafts)):
            return self  # nothing of the call's own: the pipeline's spec, validated when it was built
        spec = CallSpec.make(self.normalize if normalize is None else normalize, self.size,
                             self.interpolation if interpolation is None else interpolation,
                             self.dtype, self.memory_format, self.views,
                             self.crop if crops is None else crops, self.window if windows is None else windows,
                             self.color if colors is None else colors, self.augment if augments is None else augments,
                             self.mix if mixes is None else mixes, self.draft if drafts is None else drafts)
        if spec.views != self.views:
            raise ValueError(f"windows={windows!r} has {spec.views} views, the pipeline was built with "
                             f"views={self.views}")
        return spec


def _spec_fields(cls, prefix: str = "") -> None:
    """Give ``cls`` (which holds a ``CallSpec`` as ``_spec``) the spec's fields
    as read-only attributes ``prefix + name``."""
    import operator

    for name in CallSpec.__slots__:
        setattr(cls, prefix + name, property(operator.attrgetter("_spec." + name)))


def decode_arrow(images: pa.Array, labels=None, *, device=None, normalize=None,
                 stream: Optional[torch.cuda.Stream] = None, ctx=None, out=None, out_lbl=None, size=None,
                 crops=None, windows=None, interpolation=None, dtype=None, memory_format=None, views=None,
                 colors=None, augments=None, mixes=None, drafts=None):
    """Decode an Arrow ``binary``/``large_binary`` array of JPEG cells.

    ``labels``: optional (address, offset, keepalive) as from ``_labels_buffer``
    or an int64 sequence. ``ctx``: a libldt context (default: the device's
    shared one). ``size``: the output size (h, w), None = (224, 224).
    ``crops``: None, or int ``[N, 5]`` rows of (top, left, height, width,
    flip): each row's box of the decoded image is resized to ``size`` as
    torchvision's ``F.resized_crop`` does, then mirrored when flip is 1; a
    row with a bad box fails alone (status 6).
    ``windows``: None, or int ``[N, 4]`` rows of (res_h, res_w, top, left):
    each row's source (its box with ``crops``, else the whole image) is resized
    to res_h x res_w and the output is the ``size`` window of that result at
    (top, left), as Pillow's ``resize().crop()`` gives it (``Resize(256)`` +
    ``CenterCrop(224)``: see ``ResizeCenterCrop``); with a flip the window is
    mirrored. Nothing is padded: a row whose window is not inside res fails
    alone (status 7). Windowed batches take the streaming resize kernel, and
    the whole image is still decoded.
    ``interpolation``: the resize's filter, ``"bilinear"`` (None, the default)
    or ``"bicubic"`` (``check_interpolation`` lists every accepted spelling),
    each bit-exact with Pillow's ``resize`` with that filter in every
    composition above. A bicubic batch takes the streaming resize kernel, and a
    row fails (status 4) when ``ceil(2 * src / res) > 37`` on an axis.
    ``dtype``: the image's element type, ``torch.float32`` (None, the
    default), ``torch.float16`` or ``torch.bfloat16`` (bit-identical to the
    float32 result's ``.to(dtype)``: round to nearest even, fp16 overflow
    +-inf), or ``torch.uint8`` (the Pillow-exact resized byte itself, the
    image before ``ToTensor``; with a ``normalize`` it is a ``ValueError``);
    ``check_dtype`` lists every accepted spelling.
    ``memory_format``: ``torch.contiguous_format`` (None, the default) or
    ``torch.channels_last``: the same values at the same indices with strides
    exactly ``(3*h*w, 1, 3*w, 3)``. Both are stored by the resize kernel
    itself, so no conversion pass follows; a failed row is all zeros. With a
    non-default format a caller's ``out=`` must have that dtype, shape and
    strides (``ValueError`` otherwise).
    ``views``: None, or an int V in 1..16: V crops / windows of every image
    from a single decode (two random views for contrastive training, five-crop
    evaluation). The image is then ``[V, N, 3, h, w]`` (1 included), view-major:
    ``out[v]`` is the dense batch of view ``v``, with channels_last's strides
    under that format. ``crops`` / ``windows`` must be ``[N, V, 5]`` /
    ``[N, V, 4]`` (a 2-D array is a ``ValueError``); a missing one means the
    whole image, no flip / res = size, origin 0 for every view. Size, filter,
    dtype, layout and Normalize apply to every view. Status and labels stay
    ``[N]``: a row's views are checked in order and the first that fails gives
    the row its status; a failed row is zero in all V outputs. ``out[v, i]`` is
    bit for bit what a single-view call with ``crops[:, v]``, ``windows[:, v]``
    gives. A caller's ``out=`` must then have that shape, the dtype and the
    strides. Each image is decoded once; only the streaming resize runs per
    view.
    ``size`` may also be a size list: a non-empty sequence of V pairs
    ``[(h, w), ...]`` (V in 1..16, ``check_view_sizes``), one output size per
    view (multi-crop: ``[(224, 224)] * 2 + [(96, 96)] * 6`` from one decode).
    It implies ``views=V`` (a different explicit ``views`` is a
    ``ValueError``); ``crops`` / ``windows`` are ``[N, V, 5]`` / ``[N, V, 4]``
    as with ``views``, view ``v``'s window and reduction limit are checked
    against ``size[v]``, and a missing window is ``(h_v, w_v, 0, 0)``. The
    image is then a tuple of tensors, one per run of consecutive equal sizes,
    each ``[V_run, N, 3, h, w]``, view-major and dense (channels_last's strides
    under that format), each a view into one flat allocation in which view
    ``v`` starts at element ``N * 3 * sum(h_u * w_u for u < v)``; a list of
    equal sizes gives a 1-tuple. A caller's ``out=`` must then be a 1-D tensor
    of the call's dtype with exactly ``N * 3 * sum(h * w)`` elements, and the
    result is views of it. Output ``(v, i)`` is bit for bit what a single-size
    call at ``size[v]`` gives.
    ``colors``: None, a float ``[N, 7]`` array (``[N, V, 7]`` in a call with
    views or a size list; a 2-D array is then a ``ValueError``) of
    ``(brightness, contrast, saturation, hue, order, gray, solarize)`` per
    output image (eight columns add ``blur``, the radius of Pillow's
    ``ImageFilter.GaussianBlur``), or a ``ColorJitterParams``, which draws
    them here: torchvision's ``RandomApply([ColorJitter])``,
    ``RandomGrayscale`` and ``RandomSolarize``, and the PIL GaussianBlur of the
    DINO / MoCo / BYOL loaders, on the resized uint8 image, bit-exact with Pillow
    (``check_colors`` says what each column means; a bad value is a
    ``ValueError`` before any device is touched). The stage order per output
    image is fixed: crop -> resize -> window -> flip, then the jitter ops in
    ``order``, then grayscale, then the blur, then solarize, then ``ToTensor`` /
    ``Normalize`` and the store in the call's dtype and layout (with
    ``torch.uint8`` the stored byte is the colour-processed byte). The resize
    then runs as it does for a uint8 output, into a workspace, and two more
    kernels follow, and a third when some row has a blur (its six passes run
    in LDS); a call without ``colors`` launches what it always did.

    ``augments``: None, a float ``[N, K, 10]`` array (``[N, V, K, 10]`` in a
    call with views) of up to K <= 4 ops ``(op, p0..p5, fill_r, fill_g,
    fill_b)`` per output image, records from ``check_augments`` (which also
    carry an erase box), or a sampler (``TrivialAugmentWide``, ``RandAugment``,
    ``RandomErasing``), which draws them here: the op set of torchvision's
    auto-augment family (the five NEAREST affine ops, Brightness, Color,
    Contrast, Sharpness, Posterize, Solarize, AutoContrast, Equalize, Invert)
    on the resized uint8 image, bit-exact with Pillow, then ``ToTensor`` /
    ``Normalize`` and ``RandomErasing(value=0)``'s box of zeros
    (``check_augments`` says what each column means; a bad value is a
    ``ValueError``). The ops run in up to K more launches after the resize
    (``ldt_set_augments``); not together with ``colors`` (``ValueError``); a
    call without ``augments`` launches what it always did.

    ``mixes``: None, a pair ``(rows, num_classes)`` as ``check_mixes`` takes it
    (records of ``mix_dtype()`` or a float ``[N, 9]`` array of ``(partner,
    w_self, w_partner, top, left, height, width, lw_self, lw_partner)``), or a
    ``MixUp`` / ``CutMix`` / ``MixChoice``, which draws here: the batch step of
    the supervised recipes as the last stage before the store (``ldt_set_mix``).
    Outside its box a row's element is ``partner * w_partner + own * w_self``
    in float32 on the ToTensor / Normalize values (the erase box's zeros
    included), inside it the partner's, then ``.to(dtype)``: bit for bit
    torchvision's ``MixUp`` / ``CutMix``. With labels and ``num_classes > 0``
    the returned label is the soft float32 ``[N, num_classes]`` tensor
    (``CrossEntropyLoss`` takes it); a label outside ``0..num_classes-1`` is a
    ``ValueError``. Not with ``views``, a size list or ``torch.uint8``
    (``ValueError``). A failed row is zero with a zero soft row; a row whose
    partner failed is stored unmixed with a one-hot soft row. A call without
    ``mixes`` launches what it always did.
    ``drafts``: None, an int ``[N]`` array of libjpeg scales, each 1, 2, 4 or 8
    (``check_drafts``; anything else is a ``ValueError`` before any device is
    touched), or a ``Draft((h, w))``, which computes them from the header sizes
    by Pillow's ``Image.draft`` rule. Row i is decoded in the DCT domain at
    scale ``1 / s`` (libjpeg's 4x4, 2x2 or 1x1 IDCT per block) to the ``ceil(W
    / s) x ceil(H / s)`` image Pillow gives after ``im.draft("RGB", req)``
    picked that scale and ``im.convert("RGB")``, bit for bit; those are not
    the full decode's pixels, which is ``draft``'s documented behaviour. That
    image is the decoded image for everything else in the call: ``crops`` and
    ``windows`` are in its coordinates and checked against its size, the
    samplers draw for it, the reduction limit is that of the drafted source
    (so a source that fails status 4 at a small ``size`` can pass with a
    draft), ``views`` and a size list share the one drafted decode, and the
    filter, dtype, layout, Normalize, ``colors``, ``augments`` and ``mixes``
    apply unchanged. ``LDT_MAX_DIM`` still bounds the file's own size, and the
    Huffman stage still walks the whole stream. A call without ``drafts``, or
    with every scale 1, launches what it always did.
    Returns (image dtype[N,3,h,w], label int64[N] or None).
    The host cells are only borrowed for the call (copied into the context's
    pinned ring, then sent to HBM on ``stream``).
    """
    spec = CallSpec.make(normalize, size, interpolation, dtype, memory_format, views, crops, windows, colors, augments,
                         mixes, drafts)
    return _decode_cells(spec, images, labels, device, stream, ctx, out, out_lbl)


def _decode_cells(spec: CallSpec, images, labels=None, device=None, stream=None, ctx=None, out=None, out_lbl=None,
                  out_soft=None):
    """``decode_arrow`` for a call's ``CallSpec``: draws what the spec's
    samplers draw for these cells, then decodes them."""
    if isinstance(images, pa.ChunkedArray):
        images = images.combine_chunks()
    n = len(images)
    drawn = spec.resolve(images, n=n)  # checked (and drawn) before a device is asked for
    if labels is not None and not isinstance(labels, tuple):
        arr = np.ascontiguousarray(np.asarray(labels, dtype=np.int64))
        labels = (arr.ctypes.data, 0, arr)
    if labels is None:
        out_lbl = None
    elif drawn[4] is not None and n:
        # the rows' labels where they are, on the host, against the mix's classes
        check_mix_labels(np.ctypeslib.as_array((ctypes.c_int64 * n).from_address(labels[0] + 8 * labels[1])),
                         drawn[4][1])
    call = None  # an empty batch: the outputs, and nothing to enqueue
    if n:
        t = images.type
        if t == pa.binary() or t == pa.string():
            name = "ldt_decode_batch"
        elif t == pa.large_binary() or t == pa.large_string():
            name = "ldt_decode_batch_large"
        else:
            raise TypeError(f"image column must be binary or large_binary, got {t}")
        bufs = images.buffers()
        validity = bufs[0].address if (bufs[0] is not None and images.null_count) else None
        # all-empty cells have no data buffer: give the library a valid pointer
        data = bufs[2] if bufs[2] is not None else pa.py_buffer(bytes(8))

        def call(c, img, lbl, norm, s, status):
            return getattr(c.lib, name)(c.handle, data.address, bufs[1].address, images.offset, n, validity,
                                        labels[0] if labels is not None else None,
                                        labels[1] if labels is not None else 0, img, lbl, norm, s, status)
    return _decode_tail(spec, n, drawn, _decoder(device), ctx, stream, out, out_lbl, labels is not None, call,
                        "ldt_decode_batch", out_soft)


def _mix_soft(drawn, n: int, want_lbl: bool, device, out_soft=None):
    """The soft-label tensor of a call whose ``drawn`` has a mix with classes
    and whose batch has labels (float32 ``[n, num_classes]``, every element
    written by the call), else None."""
    if drawn[4] is None or not want_lbl or drawn[4][1] == 0:
        return None
    if out_soft is not None:
        return out_soft
    return torch.empty((n, drawn[4][1]), dtype=torch.float32, device=device)


def _decode_tail(spec: CallSpec, n: int, drawn, dec, ctx, stream, out, out_lbl, want_lbl: bool, call, what: str,
                 out_soft=None):
    """The one tail of every synchronous decode: the output allocated (or the
    caller's ``out`` checked) and cut into its runs under a size list, the
    labels and the status array, the Normalize struct; then, with the
    context's lock held, ``ctx.arm`` with ``drawn`` (``spec.resolve``'s result)
    and ``call(ctx, image ptr, label ptr, norm, stream, status ptr)``, the
    library entry point with its own pointer arguments bound; then the rows'
    statuses as an ``ImageDecodeError``. Returns ``(image, labels)``; with a
    mix that has classes the labels are the soft float32 ``[n, num_classes]``
    tensor (``out_soft``, or allocated here)."""
    ctx = ctx or dec.ctx
    if out is None:
        out = _empty_image(n, spec.size, spec.dtype, spec.memory_format, dec.device, spec.views)
    else:
        _check_out(out, n, spec.size, spec.dtype, spec.memory_format, spec.views)
    flat = out
    if isinstance(spec.size, ViewSizes):
        # what the call returns: the flat allocation cut into its runs
        out = _split_views(flat, n, spec.size, spec.memory_format)
    if want_lbl and out_lbl is None:
        out_lbl = torch.empty((n,), dtype=torch.int64, device=dec.device)
    soft = _mix_soft(drawn, n, want_lbl, dec.device, out_soft)
    if call is None:
        return out, out_lbl if soft is None else soft
    mixes = None
    if drawn[4] is not None:  # a batch without labels mixes the images only
        mixes = (drawn[4][0], 0 if soft is None else drawn[4][1], None if soft is None else soft.data_ptr())
    status = np.zeros(n, np.int32)
    norm = _norm_struct(spec.normalize)
    s = stream if stream is not None else torch.cuda.current_stream(dec.device)
    with ctx.lock:
        ctx.arm(spec.size, spec.interpolation, spec.dtype, spec.memory_format, drawn[0], drawn[1], spec.views,
                drawn[2], drawn[3], mixes, drawn.drafts)
        rc = call(ctx, flat.data_ptr(), out_lbl.data_ptr() if out_lbl is not None else None,
                  ctypes.byref(norm) if norm is not None else None, s.cuda_stream, status.ctypes.data)
    if rc == _lib.LDT_ERR_IMAGE:
        raise ImageDecodeError({int(i): int(status[i]) for i in np.nonzero(status)[0]})
    ctx.check(rc, what)
    return out, out_lbl if soft is None else soft


class DeviceTensor(torch.Tensor):
    """A decoded batch tensor on the GPU. Behaves as a plain ``torch.Tensor``
    (ops on it return plain tensors); its ``pin_memory()`` returns itself, so
    a DataLoader with ``pin_memory=True`` (lance_map_style.py:67) passes the
    device tensors through instead of failing to pin them (torch pins dense
    CPU tensors only)."""

    __torch_function__ = torch._C._disabled_torch_function_impl

    def pin_memory(self, device=None):
        return self


def _as_device_batch(img: torch.Tensor, lbl: Optional[torch.Tensor]) -> dict:
    # a size list's result: the tuple of its runs
    out = {"image": tuple(t.as_subclass(DeviceTensor) for t in img) if isinstance(img, tuple)
           else img.as_subclass(DeviceTensor)}
    if lbl is not None:
        out["label"] = lbl.as_subclass(DeviceTensor)
    return out


def _in_worker() -> bool:
    """True inside a torch DataLoader worker process."""
    return torch.utils.data.get_worker_info() is not None


def _shm_uint8(nbytes: int) -> torch.Tensor:
    t = torch.empty((nbytes,), dtype=torch.uint8)
    t.share_memory_()  # the DataLoader then sends a handle, not the bytes
    return t


def _pack_list(images: Sequence, labels) -> dict:
    """Worker side: a list of JPEG ``bytes`` (None = null cell) packed into one
    shared-memory byte tensor + int64 offsets (one copy per cell)."""
    n = len(images)
    lens = np.fromiter((0 if b is None else len(b) for b in images), dtype=np.int64, count=n)
    offs = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    data = _shm_uint8(int(offs[-1]))
    buf = data.numpy()
    for i, b in enumerate(images):
        if b:
            buf[offs[i]:offs[i + 1]] = np.frombuffer(b, dtype=np.uint8)
    packed = {"offsets": torch.from_numpy(offs), "data": data}
    if any(b is None for b in images):
        packed["valid"] = torch.from_numpy(np.fromiter((b is not None for b in images), dtype=np.bool_, count=n))
    if labels is not None:
        packed["label"] = torch.from_numpy(np.ascontiguousarray(np.asarray(labels, dtype=np.int64)))
    return packed


def _pack_arrow(images: pa.Array, labels) -> dict:
    """Worker side: an Arrow ``binary``/``large_binary`` column (any offset)
    packed like ``_pack_list`` with one memcpy of its data range."""
    if isinstance(images, pa.ChunkedArray):
        images = images.combine_chunks()
    n = len(images)
    bufs = images.buffers()
    odt = np.int64 if pa.types.is_large_binary(images.type) or pa.types.is_large_string(images.type) else np.int32
    offs = np.frombuffer(bufs[1], dtype=odt, count=n + 1, offset=images.offset * np.dtype(odt).itemsize)
    offs = offs.astype(np.int64)
    lo, hi = int(offs[0]), int(offs[-1])
    data = _shm_uint8(hi - lo)
    if hi > lo:
        data.numpy()[:] = np.frombuffer(bufs[2], dtype=np.uint8, count=hi - lo, offset=lo)
    packed = {"offsets": torch.from_numpy(offs - lo), "data": data}
    if images.null_count:
        packed["valid"] = torch.from_numpy(np.asarray(images.is_valid().to_numpy(zero_copy_only=False), np.bool_))
    if labels is not None:
        packed["label"] = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int64))
    return packed


def _unpack(packed: dict) -> Tuple[pa.Array, Optional[np.ndarray]]:
    """Main-process side: a ``large_binary`` Arrow array over the shared
    tensors (no copy) and the labels."""
    offs = packed["offsets"].numpy()
    n = len(offs) - 1
    valid = None
    if "valid" in packed:
        valid = pa.array(packed["valid"].numpy()).buffers()[1]
    data = packed["data"].numpy()
    arr = pa.Array.from_buffers(pa.large_binary(), n, [valid, pa.py_buffer(offs), pa.py_buffer(data)])
    lab = packed["label"].numpy() if "label" in packed else None
    return arr, lab


class DeviceBatch:
    """What ``collate_fn`` / ``decode_tensor_image`` return inside a DataLoader
    worker: the batch's compressed cells in shared memory, decoded on the GPU
    in the main process on first use.

    Indexing (``batch["image"]``, ``batch["label"]``), ``keys()``/``items()``
    and ``pin_memory()`` trigger the decode; ``pin_memory()`` — called by the
    DataLoader's pin-memory thread when ``pin_memory=True`` — returns the plain
    ``{"image", "label"}`` dict. Deliberately not a ``Mapping``: torch's
    ``pin_memory`` would otherwise pin the values one by one instead of calling
    ``pin_memory()`` on the batch. Decode errors raise ``ImageDecodeError``
    where the decode runs (re-raised in the main thread by the DataLoader when
    it runs in the pin-memory thread)."""

    __slots__ = ("_packed", "_device", "_out", "_spec")

    def __init__(self, packed: dict, device=None, normalize=None, *, size=None, crop=None, window=None,
                 interpolation=None, dtype=None, memory_format=None, views=None, color=None, augment=None, mix=None,
                 draft=None):
        self._set(packed, device, CallSpec.make(normalize, size, interpolation, dtype, memory_format, views, crop,
                                                window, color, augment, mix,
                                                draft).check_arrays(len(packed["offsets"]) - 1))

    def _set(self, packed: dict, device, spec: CallSpec) -> "DeviceBatch":
        self._packed = packed
        self._device = None if device is None else str(device)
        self._out = None
        # the call's options travel with the cells to the main process: arrays
        # checked for these cells, samplers to draw there
        self._spec = spec
        return self

    @classmethod
    def _of(cls, packed: dict, device, spec: CallSpec) -> "DeviceBatch":
        """A batch for a surface's own spec, already checked for these cells."""
        return cls.__new__(cls)._set(packed, device, spec)

    def decode(self) -> dict:
        if self._out is None:
            arr, lab = _unpack(self._packed)
            img, lbl = _decode_cells(self._spec, arr, lab, self._device)
            self._out = _as_device_batch(img, lbl)
            self._packed = None
        return self._out

    def pin_memory(self, device=None) -> dict:
        return self.decode()

    def __getitem__(self, key):
        return self.decode()[key]

    def __contains__(self, key) -> bool:
        return key in self.decode()

    def __iter__(self):
        return iter(self.decode())

    def __len__(self) -> int:
        return len(self.decode())

    def keys(self):
        return self.decode().keys()

    def values(self):
        return self.decode().values()

    def items(self):
        return self.decode().items()

    def get(self, key, default=None):
        return self.decode().get(key, default)

    def __repr__(self) -> str:
        state = "decoded" if self._out is not None else f"{len(self._packed['offsets']) - 1} cells pending"
        return f"DeviceBatch({state})"


_spec_fields(DeviceBatch, "_")  # ._size, ._views, ._interpolation, ...: the spec's fields

def decode_tensor_image(batch, **kwargs):
    """to_tensor_fn: ``pa.RecordBatch`` -> ``{"image", "label"}`` (lance_iterable.py:38-50).

    Unknown keyword arguments from LanceDataset are accepted and ignored, as
    the reference's ``**kwargs`` does. Optional keywords of this build:
    ``image_column`` ("image"), ``label_column`` ("label"), ``device``,
    ``normalize`` (False; True = ImageNet mean/std, lance_iterable.py:31),
    ``size`` (the output size (h, w); None = (224, 224)), ``crop`` (None; an
    int ``[N, 5]`` array of (top, left, height, width, flip) per row, or a
    ``RandomResizedCropFlip``, which draws the boxes from the cells' header
    sizes in the process that decodes), ``window`` (None; an int ``[N, 4]``
    array of (res_h, res_w, top, left) per row, or a ``ResizeCenterCrop``:
    ``window=ResizeCenterCrop(256), size=(224, 224)`` is torchvision's
    ``Resize(256)`` + ``CenterCrop(224)``), ``interpolation`` (None =
    ``"bilinear"``; ``"bicubic"``, torchvision's ``InterpolationMode.BICUBIC``
    or Pillow's ``Image.BICUBIC``: the resize's filter, see ``decode_arrow``;
    any other filter raises ``ValueError``), ``dtype`` (None =
    ``torch.float32``; ``torch.float16``, ``torch.bfloat16`` or
    ``torch.uint8``) and ``memory_format`` (None = ``torch.contiguous_format``;
    ``torch.channels_last``): the image tensor's element type and layout,
    stored by the resize itself, see ``decode_arrow``, and ``views`` (None; an
    int V in 1..16: V crops / windows per image from one decode, the image
    ``[V, N, 3, h, w]``, ``crop`` / ``window`` arrays ``[N, V, 5]`` / ``[N, V,
    4]``, a ``RandomResizedCropFlip`` drawing V boxes per image; a
    ``ResizeFiveCrop`` as ``window`` implies its own 5 or 10), and ``color``
    (None; a float ``[N, 7]`` / ``[N, V, 7]`` array of (brightness, contrast,
    saturation, hue, order, gray, solarize) per output image, with an eighth
    column for the radius of Pillow's GaussianBlur if wanted, or a
    ``ColorJitterParams``, which draws them in the process that decodes:
    ColorJitter, RandomGrayscale, GaussianBlur and RandomSolarize on the resized uint8 image,
    bit-exact with Pillow, see ``decode_arrow``), and ``augment`` (None; a
    ``TrivialAugmentWide`` or ``RandAugment``, with a ``RandomErasing`` as its
    ``erase=`` if wanted, which draws in the process that decodes, or the
    array / records ``check_augments`` takes: the auto-augment ops on the
    resized uint8 image, bit-exact with Pillow, and the erase box after
    Normalize, see ``decode_arrow``; not together with ``color``), and ``mix``
    (None; a ``MixUp``, ``CutMix`` or ``MixChoice``, which draws in the process
    that decodes, or a pair ``(rows, num_classes)`` as ``check_mixes`` takes
    it: the batch's MixUp / CutMix fused before the store, the label then the
    soft float32 ``[N, num_classes]`` tensor, see ``decode_arrow``), and
    ``draft`` (None; a ``Draft((h, w))`` or an int ``[N]`` array of scales 1,
    2, 4, 8: the DCT-domain 1/2, 1/4, 1/8 decode, Pillow's ``Image.draft``;
    ``crop`` and ``window`` then refer to the drafted image, see
    ``decode_arrow``).
    In a DataLoader worker it returns a ``DeviceBatch`` (decoded in the main
    process).
    """
    return _decode_record_batch(CallSpec.make(**{k: kwargs.get(k) for k in CallSpec.__slots__}), batch,
                                kwargs.get("device"), kwargs.get("stream"), kwargs.get("image_column", "image"),
                                kwargs.get("label_column", "label"))


def _decode_record_batch(spec: CallSpec, batch, device=None, stream=None, image_column="image",
                         label_column="label"):
    """``decode_tensor_image`` for a call's ``CallSpec``."""
    images = _column(batch, image_column)
    spec = spec.check_arrays(len(images))
    if _in_worker():
        labels = None
        if label_column is not None and label_column in batch.schema.names:
            lab = _column(batch, label_column)
            if lab.null_count:
                raise ValueError(f"null values in label column {label_column!r}")
            labels = lab.to_numpy(zero_copy_only=False)
        return DeviceBatch._of(_pack_arrow(images, labels), device, spec)
    return _as_device_batch(*_decode_cells(spec, images, _labels_buffer(batch, label_column), device, stream))


def collate_fn(batch_of_dicts, *, device=None, normalize=None, size=None, crop=None, window=None,
               interpolation=None, dtype=None, memory_format=None, views=None, color=None, augment=None, mix=None,
               draft=None):
    """collate_fn: list of ``{"image": bytes, "label": int}`` -> stacked tensors
    (lance_map_style.py:21-44). The bytes are packed into one buffer (zero-copy
    of the Python ``bytes`` objects is impossible; this is the one host copy)
    and decoded on the GPU — in a DataLoader worker, packed into shared memory
    and returned as a ``DeviceBatch`` for the main process to decode. A
    ``pa.RecordBatch`` is accepted too. ``size``: the output size (h, w),
    None = (224, 224). ``crop``, ``window``, ``interpolation``, ``dtype``,
    ``memory_format``, ``views``, ``color``, ``augment``, ``mix``, ``draft``: as for ``decode_tensor_image``."""
    return _collate(CallSpec.make(normalize, size, interpolation, dtype, memory_format, views, crop, window, color,
                                  augment, mix, draft), batch_of_dicts, device)


def _collate(spec: CallSpec, batch_of_dicts, device=None):
    """``collate_fn`` for a call's ``CallSpec``."""
    if isinstance(batch_of_dicts, pa.RecordBatch):
        return _decode_record_batch(spec, batch_of_dicts, device)
    images = [item["image"] for item in batch_of_dicts]
    labels = [item["label"] for item in batch_of_dicts] if batch_of_dicts and "label" in batch_of_dicts[0] \
        else None
    spec = spec.check_arrays(len(images))
    if _in_worker():
        return DeviceBatch._of(_pack_list(images, labels), device, spec)
    return _as_device_batch(*_decode_cells(spec, pa.array(images, type=pa.binary()), labels, device))


def make_collate_fn(device=None, normalize=None, size=None, crop=None, window=None, interpolation=None,
                    dtype=None, memory_format=None, views=None, color=None, augment=None, mix=None, draft=None):
    """A picklable collate_fn bound to a device / Normalize setting / output
    size / crop / window / interpolation / dtype / memory_format / views (for ``DataLoader(collate_fn=...)`` with spawn workers;
    a ``RandomResizedCropFlip`` or ``ResizeCenterCrop`` travels with each batch
    and is evaluated in the main process, where the batch is decoded; so does a ``ColorJitterParams`` as
    ``color``, which draws there, and a ``TrivialAugmentWide`` / ``RandAugment`` / ``RandomErasing`` as
    ``augment``, and a ``MixUp`` / ``CutMix`` / ``MixChoice`` as ``mix``, and a ``Draft`` as ``draft``)."""
    return _BoundCollate(device, normalize, size, crop, window, interpolation, dtype, memory_format, views, color,
                         augment, mix, draft)


class _BoundCollate:
    def __init__(self, device, normalize, size=None, crop=None, window=None, interpolation=None, dtype=None,
                 memory_format=None, views=None, color=None, augment=None, mix=None, draft=None):
        self.device = None if device is None else str(device)
        # validated before any batch, and picklable: names, ints, samplers (or
        # arrays for batches of their length)
        self._spec = CallSpec.make(normalize, size, interpolation, dtype, memory_format, views, crop, window, color,
                                   augment, mix, draft)

    def __call__(self, batch_of_dicts):
        return _collate(self._spec, batch_of_dicts, self.device)


_spec_fields(_BoundCollate)  # .size, .views, .interpolation, ...: the spec's fields


def resize_raw(hwc, height: int, width: int, *, device=None, normalize=True, size=None, crops=None,
               windows=None, interpolation=None, dtype=None, memory_format=None):
    """Config 5: raw uint8 HWC cells -> Resize(size) [+Normalize] -> float32[N,3,h,w]
    (``size`` = (h, w), None = (224, 224)). ``crops``: None, or int ``[N, 5]``
    rows of (top, left, height, width, flip) as for ``decode_arrow``; a bad box
    is an argument error here. ``windows``: None, or int ``[N, 4]`` rows of
    (res_h, res_w, top, left) as for ``decode_arrow``; a bad window is an
    argument error too. ``interpolation``: as for ``decode_arrow``; a source
    over the filter's reduction limit is an argument error here. ``dtype``,
    ``memory_format``: the output's element type and layout, as for
    ``decode_arrow`` (``torch.uint8`` needs ``normalize=None``).

    ``hwc`` is a uint8 torch tensor [N, H, W, 3] (host or device) or an Arrow
    ``binary`` / ``fixed_size_binary(H*W*3)`` array of cells."""
    spec = CallSpec.make(normalize, size, interpolation, dtype, memory_format)
    if isinstance(spec.size, ViewSizes):
        raise ValueError("resize_raw takes one output size (h, w): a size list shares a decode, and a raw source has none")
    dec = _decoder(device)
    ctx = dec.ctx
    keep = None
    if isinstance(hwc, torch.Tensor):
        if hwc.dtype != torch.uint8 or hwc.dim() != 4 or tuple(hwc.shape[1:]) != (height, width, 3):
            raise ValueError("expected uint8 [N, H, W, 3]")
        t = hwc.contiguous()
        keep = t
        n = t.shape[0]
        ptr, is_dev, stride = t.data_ptr(), 1 if t.is_cuda else 0, height * width * 3
    else:
        arr = hwc.combine_chunks() if isinstance(hwc, pa.ChunkedArray) else hwc
        n = len(arr)
        bufs = arr.buffers()
        cell = height * width * 3
        if pa.types.is_fixed_size_binary(arr.type):
            if arr.type.byte_width != cell:
                raise ValueError("fixed_size_binary width != H*W*3")
            ptr = bufs[1].address + arr.offset * cell
        else:
            offs = np.frombuffer(bufs[1], dtype=np.int64 if pa.types.is_large_binary(arr.type) else np.int32,
                                 count=len(arr) + 1 + arr.offset)[arr.offset:]
            if np.any(np.diff(offs) != cell):
                raise ValueError("every raw cell must be H*W*3 bytes")
            ptr = bufs[2].address + int(offs[0])
        is_dev, stride = 0, cell
        keep = arr
    crops = check_crops(crops, n)
    windows = check_windows(windows, n)
    out = _empty_image(n, spec.size, spec.dtype, spec.memory_format, dec.device)
    if n == 0:
        return out
    norm = _norm_struct(normalize)
    s = torch.cuda.current_stream(dec.device)
    with ctx.lock:
        ctx.arm(spec.size, spec.interpolation, spec.dtype, spec.memory_format, crops, windows)
        rc = ctx.lib.ldt_resize_raw(ctx.handle, ptr, is_dev, n, height, width, stride,
                                    out.data_ptr(), ctypes.byref(norm) if norm is not None else None,
                                    s.cuda_stream)
    ctx.check(rc, "ldt_resize_raw")
    del keep
    return out


def _parse_cpulist(s: str):
    out = set()
    for part in s.split(","):
        part = part.strip()
        if not part:
            continue
        a, _, b = part.partition("-")
        out.update(range(int(a), int(b or a) + 1))
    return out


def bind_numa(device=None):
    """Restrict the calling thread (and the threads and processes it starts
    later) to the CPUs local to `device`'s NUMA node, within its current
    affinity — `numactl --cpunodebind` for one rank. Host buffers the thread
    allocates afterwards (Arrow batches read in it) then land on the GPU's
    node by first touch, so the copy pool (bound there, ldt_host_info) reads
    them locally: from a remote node its copy runs at the inter-socket link's
    ~48 GB/s instead of ~170 GB/s. Returns the CPUs now allowed
    (unchanged if the GPU's local CPUs are unknown or outside the affinity)."""
    import os

    info = _decoder(device).ctx.host_info()
    cur = os.sched_getaffinity(0)
    local = _parse_cpulist(info.get("local_cpulist", "")) & cur
    if local and local != cur:
        os.sched_setaffinity(0, local)
        return local
    return cur


def _host_range(obj):
    """(address, size) of the host bytes behind a pa.Buffer, the data buffer of
    a binary/large_binary/fixed_size_binary pa.Array / ChunkedArray chunk, or
    a numpy array."""
    if isinstance(obj, pa.ChunkedArray):
        if obj.num_chunks != 1:
            raise ValueError("register one chunk at a time")
        obj = obj.chunk(0)
    if isinstance(obj, pa.Array):
        bufs = obj.buffers()
        obj = bufs[1] if pa.types.is_fixed_size_binary(obj.type) else bufs[2]
    if isinstance(obj, pa.Buffer):
        return obj.address, obj.size
    if isinstance(obj, np.ndarray):
        return obj.ctypes.data, obj.nbytes
    raise TypeError(f"cannot register {type(obj).__name__}")


_registered: dict = {}


def register_host(obj, device=None):
    """Page-lock the host bytes of `obj` in place (ldt_register_host), so that
    every later decode of cells inside them copies to HBM by DMA without the
    memcpy into the pinned ring: for a memory-mapped Arrow IPC / Lance
    fragment, register the `image` column's data buffer once. The bytes must
    stay alive until unregister_host(obj). Returns the registered (address,
    size)."""
    addr, size = _host_range(obj)
    if size == 0 or addr in _registered:
        return addr, size
    dec = _decoder(device)
    dec.ctx.check(dec.ctx.lib.ldt_register_host(dec.ctx.handle, addr, size), "ldt_register_host")
    _registered[addr] = (size, obj, dec)  # keeps `obj` alive while registered
    return addr, size


def unregister_host(obj):
    """Undo register_host (waits for the device first)."""
    addr, _ = _host_range(obj)
    ent = _registered.pop(addr, None)
    if ent is None:
        return
    dec = ent[2]
    dec.ctx.check(dec.ctx.lib.ldt_unregister_host(dec.ctx.handle, addr), "ldt_unregister_host")


class ResidentBatch:
    """A batch of JPEG cells staged once into HBM (bench / pre-staged loaders).

    ``decode()`` runs the full decode path with the compressed bytes already
    resident, so a timed loop measures the GPU path, not PCIe."""

    def __init__(self, cells: Sequence[bytes], labels: Iterable[int] | None = None, *, device=None):
        dec = _decoder(device)
        self.dec = dec
        self.n = len(cells)
        lens = np.fromiter((len(c) for c in cells), dtype=np.int64, count=self.n)
        self.offsets = np.zeros(self.n + 1, np.int64)
        np.cumsum(lens, out=self.offsets[1:])
        self.host = np.frombuffer(b"".join(cells), dtype=np.uint8).copy() if self.n else np.zeros(1, np.uint8)
        self.dev = torch.from_numpy(self.host).to(dec.device)
        self.labels = None if labels is None else np.ascontiguousarray(np.asarray(list(labels), np.int64))
        self.bytes = int(self.offsets[-1])
        self._sizes = None

    def image_sizes(self):
        """``_lib.image_sizes`` of the batch's cells (computed once)."""
        if self._sizes is None:
            arr = pa.Array.from_buffers(pa.large_binary(), self.n,
                                        [None, pa.py_buffer(self.offsets), pa.py_buffer(self.host)])
            self._sizes = _lib.image_sizes(arr)
        return self._sizes

    def decode(self, out=None, out_lbl=None, normalize=None, *, ctx=None, stream=None, size=None, crops=None,
               windows=None, interpolation=None, dtype=None, memory_format=None, views=None, colors=None,
               augments=None, mixes=None, drafts=None):
        """Decode on `stream` (default: the current stream) with context `ctx`
        (default: the device's shared context) to ``size`` = (h, w), None =
        (224, 224). ``crops``: as for ``decode_arrow``, or a
        ``RandomResizedCropFlip``. ``windows``: as for ``decode_arrow``, or a
        ``ResizeCenterCrop``. ``interpolation``, ``dtype``, ``memory_format``
        (and what they ask of ``out``): as for ``decode_arrow``. ``views``: as
        for ``decode_arrow`` (a ``ResizeFiveCrop`` as ``windows`` implies its
        own); the image is then ``[views, n, 3, h, w]``. ``colors``: as for
        ``decode_arrow`` (an array, or a ``ColorJitterParams``). ``augments``:
        as for ``decode_arrow`` (an array, records, or a sampler). ``mixes``:
        as for ``decode_arrow`` (a pair ``(rows, num_classes)`` or a sampler);
        the returned label is then the soft float32 tensor. ``drafts``: as
        for ``decode_arrow`` (an int ``[n]`` array of scales or a ``Draft``)."""
        return self._decode(CallSpec.make(normalize, size, interpolation, dtype, memory_format, views, crops, windows,
                                          colors, augments, mixes, drafts), out, out_lbl, ctx, stream)

    def _decode(self, spec: CallSpec, out=None, out_lbl=None, ctx=None, stream=None, out_soft=None):
        """``decode`` for a call's ``CallSpec``."""
        drawn = spec.resolve(sizes=self.image_sizes, n=self.n)  # the header sizes only when a sampler wants them
        if drawn[4] is not None:
            check_mix_labels(self.labels, drawn[4][1])

        def call(c, img, lbl, norm, s, status):
            return c.lib.ldt_decode_batch_resident(
                c.handle, self.host.ctypes.data, self.dev.data_ptr(), self.offsets.ctypes.data, self.n,
                self.labels.ctypes.data if self.labels is not None else None, img, lbl, norm, s, status)

        return _decode_tail(spec, self.n, drawn, self.dec, ctx, stream, out, out_lbl, self.labels is not None, call,
                            "ldt_decode_batch_resident", out_soft)


def slot_streams(depth: int, queues: int, env: Optional[str] = None) -> Tuple[int, bool]:
    """DecodePipeline's stream plan for ``depth`` slots on a process with
    ``queues`` HIP hardware queues per priority (GPU_MAX_HW_QUEUES): returns
    (slots on high-priority streams, cells' DMA on the slots' own streams).

    Normal priority while the slots and the consumer's stream fit the queues;
    deeper pipelines put up to ``queues`` slots on high-priority streams (their
    own queues) and the rest beside the consumer. The copy stream needs a
    normal queue of its own beside normal slots, and beside high-priority slots
    it measured slower when normal slots share the pool too (c2p depth 6: host
    input 35k vs 50k at depth 7 with the DMA on the slots' streams).
    ``env`` (LDT_SLOT_PRIORITY) "0"/"1" forces every slot's priority."""
    if env is not None:
        n_high = depth if int(env) else 0
    else:
        n_high = 0 if depth + 1 <= queues else min(depth, queues)
    n_normal = depth - n_high
    slot_dma = (n_normal + 2 > queues or n_high > 0) if n_normal else (n_high > queues)
    return n_high, slot_dma


# Batches in flight for progressive (SOF2) datasets: make_to_tensor_fn(depth=
# PROGRESSIVE_DEPTH). A c2p batch spends ~13 ms in k_prog, so several must be
# in flight. At 5 (4 slots on high-priority streams, 1 beside the consumer) the
# rate is the same in a clean process and in a DDP process in the reference's
# order (62k img/s both); at 7 the clean rate is 5% higher but the DDP order
# costs 23% (three normal-priority slots share queues with the comm and
# consumer streams, whose per-step waits then block them). DESIGN.md §6.
PROGRESSIVE_DEPTH = 5

_slot_stream_sets: dict = {}  # (device index, priority) -> [torch.cuda.Stream]


def _slot_stream(dev, priority: int, i: int):
    """The device's process-wide slot stream i of `priority` (0 normal, -1
    high), created on first request: DecodePipelines share them (a process's
    pipelines decode one after another; two used at once serialise on the
    shared slots, still in order)."""
    lst = _slot_stream_sets.setdefault((dev.index, priority), [])
    while len(lst) <= i:
        lst.append(torch.cuda.Stream(dev, priority=priority))
    return lst[i]


class DecodePipeline:
    """`depth` batches in flight: each slot owns a libldt context (its own HBM
    workspace and pinned staging ring) and a HIP stream. ``decode(batch)``
    enqueues on the next slot's stream without waiting for the caller's stream
    and makes the caller's current stream wait for the result, so the
    latency-bound Huffman stages of one batch overlap the resize/IDCT of the
    previous one — the GPU-side analogue of the reference DataLoader's
    prefetching workers (lance_map_style.py:137, num_workers=8).

    ``adaptive=True`` (``depth`` 3, what ``make_to_tensor_fn()`` builds):
    the batches in flight follow each call's batch size, with the process's
    four hardware queues held by the consumer's stream and the three slot
    streams throughout. A host batch of at least 8 MB of encoded cells takes
    slots 0 and 1 in turn with its DMA on slot 2's stream (two in flight, the
    transfer overlapping the previous batches' kernels); smaller batches and
    resident ones rotate over all three slots with the DMA on the slot's own
    stream (three in flight: a batch of 128 small images does not fill the
    GPU). DESIGN.md §7a.

    Errors are asynchronous: every decode gets its context's ticket
    (ldt_last_ticket), and ``check()`` waits for every unchecked batch and
    raises ImageDecodeError with its failing rows (per-image status, as
    ldt_fetch_status_ticket reports). ``check_slot(i)`` checks slot i's
    batches older than its most recent one — a batch two uses of the slot ago,
    long finished — so checking before each reuse never waits for the batch
    just enqueued."""

    def __init__(self, depth: int = 2, device=None, profile: bool = False, adaptive: bool = False, size=None,
                 crop=None, window=None, interpolation=None, dtype=None, memory_format=None, views=None, color=None,
                 augment=None, mix=None, draft=None):
        from collections import deque

        # what every batch gets, validated before a device is asked for (.size,
        # .views, .color, ...: its fields). size (a pair, or a size list: the
        # image then the tuple of its runs), dtype, memory_format and views
        # (None: the 4-D tensor; an int V, or the 5 / 10 of a ResizeFiveCrop
        # window: [V, n, 3, h, w]) are fixed per pipeline, which allocates the
        # outputs; crop, window, color, augment and draft (samplers drawn per
        # batch, at decode, or arrays) and the filter serve every batch that
        # names none of its own
        self._spec = CallSpec.make(None, size, interpolation, dtype, memory_format, views, crop, window, color,
                                   augment, mix, draft)
        self.dec = _decoder(device)
        self.depth = 3 if adaptive else max(1, int(depth))
        self.adaptive = bool(adaptive)
        self.ctxs = [_lib.Context(self.dec.device.index) for _ in range(self.depth)]
        for c in self.ctxs:
            c.set_option(_lib.OPT_SYNC_STATUS, 0)
            if profile:
                c.set_option(_lib.OPT_PROFILE, 1)
        # the cells' DMA of host batches goes on the device's copy stream when
        # the process has a hardware queue for it beside the slots' streams and
        # the consumer's (otherwise two streams would share a queue and the
        # slots' kernels serialise): else on the slot's own stream
        # slot streams: normal priority while the slots and the consumer's
        # stream fit the process's hardware queues (GPU_MAX_HW_QUEUES, 4 by
        # default); deeper pipelines (progressive batches take ~15 ms each, so
        # they want 4 in flight) take high-priority streams, which ROCm serves
        # from their own set of queues, so no slot shares a queue with the
        # consumer's stream (a shared queue serialises the slots: measured
        # c2p depth 4: 26k img/s on normal streams vs 44k). LDT_SLOT_PRIORITY
        # = 0 / 1 forces either.
        n_high, slot_dma = slot_streams(self.depth, _lib.hw_queues(), os.environ.get("LDT_SLOT_PRIORITY"))
        if self.adaptive:
            env = os.environ.get("LDT_SLOT_PRIORITY")
            n_high, slot_dma = (self.depth if env is not None and int(env) else 0), True
        self.high_priority = n_high > 0
        if slot_dma:
            for c in self.ctxs:
                c.set_option(_lib.OPT_COPY_MODE, 1)
        # the slot streams are taken at the first decode (see _streams_now)
        self._n_high = n_high
        self._streams = None
        self._copy_mode = [1 if slot_dma else 0] * self.depth
        self._k_large = self._k_small = 0
        self.pending = [deque() for _ in range(self.depth)]  # per slot: (ticket, n), oldest first
        self.last_ticket = None  # (slot, ticket) of the most recent decode
        self.k = 0

    @property
    def streams(self):
        """The slots' HIP streams (taken at the first decode)."""
        return self._streams_now()

    def _streams_now(self):
        """Slot i's stream is the device's process-wide slot stream i of its
        priority (_slot_stream), taken at the first decode rather than at
        construction. The HIP runtime maps a process's streams onto
        GPU_MAX_HW_QUEUES hardware queues per priority in the order they
        come to it, and a slot whose queue also carries a stream the process
        made afterwards lost up to 30% (tools/probes/stream_env.py, DESIGN.md
        §6): pipelines built before a DDP process group and model (the
        reference's order, lance_iterable.py:78-95) run their first batch
        after them, and every pipeline of the process shares the same few
        slot streams instead of adding new ones that the runtime would place
        on the queues of the live pipeline's slots."""
        if self._streams is None:
            st = [_slot_stream(self.dec.device, -1, i) if i < self._n_high
                  else _slot_stream(self.dec.device, 0, i - self._n_high) for i in range(self.depth)]
            self._streams = st
            # adaptive: slots 0 and 1 DMA large batches on slot 2's stream
            if self.adaptive:
                for c in self.ctxs[:2]:
                    c.set_copy_stream(st[2])
        return self._streams

    def decode(self, batch, normalize=None, image_column: str = "image", label_column: str = "label",
               wait: bool = True, crops=None, windows=None, interpolation=None, colors=None, augments=None,
               mixes=None, drafts=None):
        """Enqueue one batch: a ``ResidentBatch`` (cells already in HBM) or a
        host ``pa.RecordBatch`` as LanceDataset yields it (its buffers are
        copied into the slot's pinned ring during the call, then to HBM
        asynchronously on the slot's stream).

        ``wait=True``: torch's current stream waits for the result now;
        returns ``(image, label)``. ``wait=False``: nothing waits yet; returns
        ``(image, label, ready)`` and the consumer calls ``ready()`` on the
        stream that will use the tensors, so work enqueued there in between
        (a training step) overlaps this decode (see ``prefetch``).

        ``crops``: this batch's crops (an ``[n, 5]`` array or a
        ``RandomResizedCropFlip``); None = the pipeline's ``crop``. A bad box
        (and any other row of a batch with crops that fails) is reported by
        ``check()``, not raised here. ``windows``: this batch's windows (an
        ``[n, 4]`` array or a ``ResizeCenterCrop``); None = the pipeline's
        ``window``. A bad window is reported by ``check()`` in the same way.
        ``interpolation``: this batch's filter; None = the pipeline's. Every
        call carries its own, so batches in flight may differ. With the
        pipeline's ``views=V`` the image is ``[V, n, 3, h, w]`` and a call's
        own ``crops`` / ``windows`` arrays are ``[n, V, 5]`` / ``[n, V, 4]``.
        ``colors``: this batch's colours (an ``[n, 7]`` / ``[n, V, 7]`` array
        or a ``ColorJitterParams``); None = the pipeline's ``color``.
        ``augments``: this batch's augments (as for ``decode_arrow``); None =
        the pipeline's ``augment``. ``mixes``: this batch's mix (as for
        ``decode_arrow``); None = the pipeline's ``mix``. With a mix that has
        classes the label is the soft float32 ``[n, num_classes]`` tensor,
        allocated per batch on the slot's stream like the image. ``drafts``:
        this batch's draft scales (an int ``[n]`` array or a ``Draft``, as for
        ``decode_arrow``); None = the pipeline's ``draft``."""
        # this batch's spec, refused before anything is enqueued (uint8 with a Normalize too)
        spec = self._spec.override(crops, windows, interpolation, colors, augments, normalize, mixes, drafts)
        if self.adaptive:
            large = not isinstance(batch, ResidentBatch) and \
                auto_host_depth(_cell_bytes(batch, image_column)) == 2
            if large:
                slot = self._k_large % 2
                self._k_large += 1
            else:
                slot = self._k_small % 3
                self._k_small += 1
            mode = 0 if large else 1
            if self._copy_mode[slot] != mode:
                self.ctxs[slot].set_option(_lib.OPT_COPY_MODE, mode)
                self._copy_mode[slot] = mode
        else:
            slot = self.k % self.depth
        # the slot's context holds the status of its last two calls: check the
        # older one before this call replaces it (it finished long ago)
        self.check_slot(slot)
        self.k += 1
        s = self.streams[slot]
        cur = torch.cuda.current_stream(self.dec.device)
        if isinstance(batch, ResidentBatch):
            n, has_lbl = batch.n, batch.labels is not None
        else:
            images = _column(batch, image_column)
            lab = _labels_buffer(batch, label_column)
            n, has_lbl = len(images), lab is not None
        with torch.cuda.stream(s):
            out = _empty_image(n, spec.size, spec.dtype, spec.memory_format, self.dec.device, spec.views)
            lbl = torch.empty((n,), dtype=torch.int64, device=self.dec.device) if has_lbl else None
            # the soft labels of a batch with a mix: the classes are the spec's when
            # it holds a pair or a sampler that names them, which every mix does
            nc = 0 if spec.mix is None or not has_lbl else \
                int(spec.mix.num_classes if hasattr(spec.mix, "sample") else spec.mix[1])
            soft = torch.empty((n, nc), dtype=torch.float32, device=self.dec.device) if nc else None
        ctx = self.ctxs[slot]
        before = ctx.lib.ldt_last_ticket(ctx.handle)
        try:
            if isinstance(batch, ResidentBatch):
                batch._decode(spec, out, lbl, ctx, s, soft)
            else:
                _decode_cells(spec, images, lab, self.dec.device, s, ctx, out, lbl, soft)
        except ImageDecodeError:
            # rows refused on the host (header walk, crop and window check).
            # Without crops or windows that raises here, as it always has; a
            # batch with either is enqueued all the same (those rows zero, label
            # -100) and its ticket's status holds them, so a bad box or window
            # surfaces through check() like every other per-image error of the
            # pipeline
            if spec.crop is None and spec.window is None:
                raise
        t = ctx.lib.ldt_last_ticket(ctx.handle)
        self.last_ticket = (slot, t) if t != before else None
        if t != before:
            self.pending[slot].append((t, n))
        # a size list: the caller gets the runs, the streams are recorded on the
        # allocation they share
        img = _split_views(out, n, self.size, self.memory_format) if isinstance(self.size, ViewSizes) else out
        if soft is not None:
            lbl = soft  # the call's label; the int64 one was the library's to write
        if wait:
            cur.wait_stream(s)
            out.record_stream(cur)
            if lbl is not None:
                lbl.record_stream(cur)
            return img, lbl
        ev = torch.cuda.Event()
        ev.record(s)

        def ready():
            use = torch.cuda.current_stream(self.dec.device)
            use.wait_event(ev)
            out.record_stream(use)
            if lbl is not None:
                lbl.record_stream(use)

        return img, lbl, ready

    def prefetch(self, batches, ahead: int = 2, normalize=None, image_column: str = "image",
                 label_column: str = "label"):
        """Iterate ``batches`` (host RecordBatches or ResidentBatches) yielding
        ``{"image", "label"}`` dicts, with the decode of the next ``ahead``
        batches enqueued before each yield: while the consumer's step k runs on
        torch's stream, batches k+1..k+ahead decode on the slots' streams
        (decode overlapped with the training step, so
        ``.to(device)`` at lance_iterable.py:108-109 is a no-op). A batch's
        per-image status is checked before it is yielded: ImageDecodeError is
        raised instead of yielding a batch with a failed row."""
        from collections import deque

        ahead = max(0, min(int(ahead), self.depth - 1))
        q = deque()

        def emit():
            img, lbl, ready, tk = q.popleft()
            # the batch itself is checked before it is yielded, so a bad row
            # raises here (as PIL would) instead of reaching the consumer; it
            # waits only for this batch, enqueued `ahead` batches ago
            if tk is not None:
                self.check_ticket(*tk)
            ready()
            return _as_device_batch(img, lbl)

        for b in batches:
            q.append(self.decode(b, normalize=normalize, image_column=image_column,
                                 label_column=label_column, wait=False) + (self.last_ticket,))
            if len(q) > ahead:
                yield emit()
        while q:
            yield emit()
        self.check()

    def stage_times(self, reset: bool = False):
        tot: dict = {}
        for c in self.ctxs:
            for k, (ms, n) in c.stage_times(reset=reset).items():
                a = tot.get(k, (0.0, 0))
                tot[k] = (a[0] + ms, a[1] + n)
        return tot

    def host_times(self, reset: bool = False):
        """Host phase times summed over the slots' contexts (LDT_OPT_HOST_TIMING)."""
        tot: dict = {}
        calls = 0
        for c in self.ctxs:
            us, n = c.host_times(reset=reset)
            calls += n
            for k, v in us.items():
                tot[k] = tot.get(k, 0.0) + v
        return tot, calls

    def set_option(self, opt: int, value: int):
        for c in self.ctxs:
            c.set_option(opt, value)

    def _ticket_status(self, i: int, ticket: int, n: int) -> dict:
        c = self.ctxs[i]
        st = np.zeros(n, np.int32)
        rc = c.lib.ldt_fetch_status_ticket(c.handle, ticket, st.ctypes.data, n)
        if rc != _lib.LDT_ERR_IMAGE:
            c.check(rc, "ldt_fetch_status_ticket")
        return {int(j): int(st[j]) for j in np.nonzero(st)[0]}

    def check_ticket(self, i: int, ticket: int):
        """Wait for slot i's batch `ticket` (if still unchecked); raise
        ImageDecodeError on failures."""
        p = self.pending[i]
        for j, (t, n) in enumerate(p):
            if t == ticket:
                del p[j]
                bad = self._ticket_status(i, t, n)
                if bad:
                    raise ImageDecodeError(bad)
                return

    def check_slot(self, i: int):
        """Check slot i's batches older than its most recent one (they finished
        long ago: the slot's context has been used since); raise
        ImageDecodeError on failures. Called before the slot is reused, so the
        context's two held statuses are never overwritten unchecked."""
        p = self.pending[i]
        while len(p) > 1:
            t, n = p.popleft()
            bad = self._ticket_status(i, t, n)
            if bad:
                raise ImageDecodeError(bad)

    def check(self):
        """Wait for every unchecked batch; raise ImageDecodeError with the
        failing rows of all of them."""
        bad = {}
        for i in range(self.depth):
            p = self.pending[i]
            while p:
                t, n = p.popleft()
                bad.update(self._ticket_status(i, t, n))
        if bad:
            raise ImageDecodeError(bad)


_spec_fields(DecodePipeline)  # .size, .crop, .window, .interpolation, ...: the spec's fields


# make_to_tensor_fn(depth=None): batches with fewer cell bytes than this run 3
# deep (DMA on the slot streams), larger ones 2 deep beside the copy stream
# (profiles/r4/host_depth_ab_r4hd.txt: 3.3 MB batches of 128 +10% at depth 3,
# 17 MB batches of 256 steady only at depth 2)
AUTO_DEPTH_SMALL_BYTES = 8 << 20


def auto_host_depth(cell_bytes: int) -> int:
    """Batches in flight that make_to_tensor_fn(depth=None) (an adaptive
    DecodePipeline) runs a host batch of `cell_bytes` bytes of encoded cells
    at: 2 (its DMA on a stream of its own) from AUTO_DEPTH_SMALL_BYTES on, 3
    below."""
    return 3 if 0 < cell_bytes < AUTO_DEPTH_SMALL_BYTES else 2


def _cell_bytes(batch, col: str) -> int:
    """Encoded bytes of a host RecordBatch's image cells (0 if unknown)."""
    try:
        if col not in batch.schema.names:
            return 0
        col_ = batch.column(col)  # a Table's column stays chunked here
        # a chunked column: the chunks' byte spans summed (no combine_chunks copy)
        chunks = col_.chunks if isinstance(col_, pa.ChunkedArray) else [col_]
        tot = 0
        for arr in chunks:
            if pa.types.is_fixed_size_binary(arr.type):
                tot += len(arr) * arr.type.byte_width
                continue
            if len(arr) == 0:
                continue
            dt = np.int64 if pa.types.is_large_binary(arr.type) else np.int32
            o = np.frombuffer(arr.buffers()[1], dtype=dt)
            tot += int(o[arr.offset + len(arr)] - o[arr.offset])
        return tot
    except Exception:  # not a host binary column: keep the default
        return 0


def make_to_tensor_fn(depth: Optional[int] = None, device=None, normalize=None, prefetch: int = 0,
                      register: bool = False, register_cap: int = 8, size=None, crop=None, window=None,
                      interpolation=None, dtype=None, memory_format=None, views=None, color=None, augment=None,
                      mix=None, draft=None, **fixed):
    """A pipelined ``to_tensor_fn`` for ``LanceDataset(..., to_tensor_fn=...)``
    (lance_iterable.py:53-59): each call enqueues its RecordBatch on one of
    `depth` contexts/streams and returns at once, so batch k+1's host copy and
    kernels overlap batch k's. The tensors are ready on torch's current stream
    (it waits for the slot's stream). Per-image errors are reported
    asynchronously: by ``fn.check()``, and at the latest when the slot is
    reused a second time (2 * `depth` calls later, when that batch finished
    long ago, so the check never stalls the host) — unlike the synchronous
    ``decode_tensor_image``.

    ``depth=None`` (the default): the batches in flight follow each call's
    batch (``DecodePipeline(adaptive=True)``): 2 with the DMA on a stream of
    its own for batches of at least 8 MB of encoded cells (c2-shaped batches
    of 256), 3 with the DMA on the slot's stream below that (FOOD101-shaped
    batches of 128), ``auto_host_depth``. With
    ``register=True`` it means 3 (registered sources: DESIGN.md §8).

    ``size=(h, w)``: the output size of every batch (None = (224, 224)).

    ``crop``: a ``RandomResizedCropFlip`` that draws every batch's boxes when
    it is enqueued (None = none); a call's own ``crop=`` keyword (an ``[n, 5]``
    array or a sampler) takes its place for that batch.

    ``window``: a ``ResizeCenterCrop`` evaluated for every batch when it is
    enqueued (None = none); a call's own ``window=`` keyword (an ``[n, 4]``
    array or a ``ResizeCenterCrop``) takes its place for that batch.

    ``interpolation``: the filter of every batch (None = ``"bilinear"``;
    ``"bicubic"``: see ``decode_arrow``); a call's own ``interpolation=``
    keyword takes its place for that batch.

    ``dtype``, ``memory_format``: the element type and layout of every
    batch's image tensor (None = ``torch.float32``, contiguous; see
    ``decode_arrow``), fixed for the function: its pipeline allocates the
    outputs.

    ``views``: None, or an int V in 1..16: V crops / windows of every image
    from one decode, every batch's image ``[V, n, 3, h, w]`` (see
    ``decode_arrow``), the ``fn.iterate`` prefetch path included; a
    ``ResizeFiveCrop`` as ``window`` implies its own. Fixed for the function,
    like the format.

    ``color``: a ``ColorJitterParams`` that draws every batch's colours when
    it is enqueued, after its boxes (None = none), the ``fn.iterate`` prefetch
    path included; a call's own ``color=`` keyword (an ``[n, 7]`` / ``[n, V,
    7]`` array or a sampler) takes its place for that batch. See
    ``decode_arrow``.

    ``augment``: a ``TrivialAugmentWide``, ``RandAugment`` or
    ``RandomErasing`` that draws every batch's augments when it is enqueued,
    after its boxes (None = none), the ``fn.iterate`` prefetch path included; a
    call's own ``augment=`` keyword takes its place for that batch. Not
    together with ``color``. See ``decode_arrow``.

    ``mix``: a ``MixUp``, ``CutMix`` or ``MixChoice`` that draws every batch's
    mix when it is enqueued, last of the call's draws (None = none), the
    ``fn.iterate`` prefetch path included; a call's own ``mix=`` keyword takes
    its place for that batch. The batch's label is then the soft float32
    tensor. See ``decode_arrow``.

    ``draft``: a ``Draft((h, w))`` evaluated for every batch when it is
    enqueued, before its boxes and windows, which then refer to the drafted
    image (None = none), the ``fn.iterate`` prefetch path included; a call's
    own ``draft=`` keyword (an ``[n]`` array of scales or a ``Draft``) takes
    its place for that batch. See ``decode_arrow``.

    ``prefetch=k`` (k < depth): ``LanceDataset`` iterates through
    ``fn.iterate`` instead, enqueueing the next k batches before yielding each
    one, so their decode overlaps the consumer's training step.

    ``register=True``: the first batch seen from each underlying `image` data
    buffer page-locks that whole buffer in place (``register_host``), so the
    batches sliced from a memory-mapped fragment reach HBM by DMA without a
    host memcpy. Only for long-lived buffers (a mapped dataset), not for
    batches built anew each step. At most ``register_cap`` buffers stay
    registered by this function (least recently used ones are unregistered),
    and a buffer the driver refuses to lock (memlock limit, overlapping
    registration) switches the function to the copying path instead of
    raising (ldt.h: such a range stays on the copying path)."""
    from collections import OrderedDict

    # (registered sources have no size-independent best depth: LanceDataset
    # over registered c2 fragments 436-475k img/s at depth 3 vs 297-308k at 2,
    # two alternating registered c2 batches 389k at 3 vs 572-583k at 2;
    # profiles/r4/dataset_depth_ab_r4dd.txt: 3 for them)
    if depth is None and register:
        depth = 3
    # the default size is not passed on, so a pipeline class that predates the
    # argument (a subclass or stand-in of the caller's) still serves
    spec = CallSpec.make(normalize, size, interpolation, dtype, memory_format, views, crop, window, color, augment,
                         mix, draft)
    given = {"size": size, "crop": crop, "window": window, "interpolation": interpolation, "color": color,
             "augment": augment, "mix": mix, "draft": draft}
    size_kw = {k: getattr(spec, k) for k, v in given.items() if v is not None}
    if not _default_format(spec.dtype, spec.memory_format):
        size_kw["dtype"], size_kw["memory_format"] = spec.dtype, spec.memory_format
    if spec.views is not None:
        size_kw["views"] = spec.views
    pipe =DecodePipeline(depth=depth or 3, device=device, adaptive=depth is None, **size_kw)
    image_column = fixed.get("image_column", "image")
    owned: "OrderedDict[int, object]" = OrderedDict()  # registrations made here, LRU order
    reg_on = [bool(register)]
    # churn guard: unregistering synchronises the device, so a loader that hands
    # out fresh buffers every batch (instead of slices of mapped fragments)
    # must not evict on every call; `evictions` holds the batch numbers of the
    # recent evictions
    seen = [0]  # batches offered to maybe_register (to_tensor_fn and the fn.iterate path)
    evictions: list = []

    def maybe_register(batch, col):
        seen[0] += 1
        if not reg_on[0] or not isinstance(batch, pa.RecordBatch):
            return
        arr = _column(batch, col)
        addr, size = _host_range(arr)
        if size == 0:
            return
        if addr in owned:
            owned.move_to_end(addr)
            return
        if addr in _registered:  # registered by the caller: theirs to manage
            return
        try:
            register_host(arr, device=device)
        except _lib.LdtError:
            reg_on[0] = False  # copying path from here on
            return
        owned[addr] = arr
        cap = max(1, int(register_cap))
        while len(owned) > cap:
            _, old = owned.popitem(last=False)
            unregister_host(old)
            evictions.append(seen[0])
        # more evictions than the cap within 4 x cap batches: the buffers do not
        # repeat, so registration cannot amortise; the copying path from here
        # on (the ranges still registered are released at once)
        while evictions and evictions[0] < seen[0] - 4 * cap:
            evictions.pop(0)
        if len(evictions) > cap:
            reg_on[0] = False
            release()

    def to_tensor_fn(batch, **kwargs):
        maybe_register(batch, kwargs.get("image_column", image_column))
        img, lbl = pipe.decode(batch, normalize=kwargs.get("normalize", normalize),
                               image_column=kwargs.get("image_column", fixed.get("image_column", "image")),
                               label_column=kwargs.get("label_column", fixed.get("label_column", "label")),
                               # a call's own options, by the names decode (CallSpec.override) takes them
                               **{to: kwargs[k] for k, to in (("crop", "crops"), ("window", "windows"),
                                                              ("interpolation", "interpolation"), ("color", "colors"),
                                                              ("augment", "augments"), ("mix", "mixes"),
                                                              ("draft", "drafts"))
                                  if kwargs.get(k) is not None})
        return _as_device_batch(img, lbl)

    def release():
        """Unregister the buffers this function registered (waits for the device)."""
        while owned:
            _, old = owned.popitem(last=False)
            unregister_host(old)

    to_tensor_fn.check = pipe.check
    to_tensor_fn.registering = lambda: reg_on[0]
    to_tensor_fn.pipeline = pipe
    to_tensor_fn.release = release
    to_tensor_fn.prefetch = max(0, min(int(prefetch), pipe.depth - 1))
    def registered(batches):
        for b in batches:
            maybe_register(b, image_column)
            yield b

    to_tensor_fn.iterate = lambda batches: pipe.prefetch(
        registered(batches), ahead=to_tensor_fn.prefetch, normalize=normalize,
        image_column=fixed.get("image_column", "image"), label_column=fixed.get("label_column", "label"))
    return to_tensor_fn
