"""ctypes binding of libldt.so (include/ldt.h) and the per-device context.

This is the Python side of the C-ABI boundary: the same stub a maintainer of
the reference would add. It owns no compute: every decode,
resize and shard computation runs in the gfx950 kernels of libldt.so. If the
library is missing or cannot be loaded, importing the product raises — there
is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch  # noqa: F401  (must load torch's HIP runtime before libldt.so)


def hw_queues() -> int:
    """Hardware queues per process the HIP runtime uses (ROCclr's
    GPU_MAX_HW_QUEUES, default 4): streams beyond it share a queue."""
    try:
        return int(os.environ.get("GPU_MAX_HW_QUEUES", "4"))
    except ValueError:
        return 4

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libldt.so")

LDT_OK = 0
LDT_ERR_ARG = -1
LDT_ERR_HIP = -2
LDT_ERR_NOMEM = -3
LDT_ERR_IMAGE = -4

IMG_OK = 0
IMG_NOT_JPEG = 1
IMG_UNSUPPORTED = 2
IMG_CORRUPT = 3
IMG_TOO_LARGE = 4
IMG_NULL = 5
IMG_BAD_CROP = 6
IMG_BAD_WINDOW = 7
IMG_STATUS_TEXT = {
    IMG_NOT_JPEG: "cannot identify image file (not a baseline JPEG)",
    IMG_UNSUPPORTED: "unsupported JPEG (arithmetic/lossless/12-bit/CMYK/multi-scan sequential/unsupported sampling factors)",
    IMG_CORRUPT: "image file is truncated or corrupt",
    IMG_TOO_LARGE: "image dimensions exceed LDT_MAX_DIM, or the output size reduces them by more than 37 "
                   "(bicubic: by more than 18.5)",
    IMG_NULL: "null image cell",
    IMG_BAD_CROP: "crop box empty, outside the decoded image, or flip not 0 or 1",
    IMG_BAD_WINDOW: "window outside the resized image (nothing is padded), or a resized size outside 1..65535",
}

OPT_SYNC_STATUS = 1
OPT_HUFF_MODE = 2
OPT_SUBSEQ_BITS = 3
OPT_PROFILE = 4
OPT_RESIZE_IMPL = 5
OPT_SYNC_WARM = 7
OPT_COPY_THREADS = 8
OPT_HOST_TIMING = 9
OPT_RESIZE_WAVES_PCT = 10
OPT_FUSED_DESTUFF = 11
OPT_COPY_MODE = 12
OPT_COPY_BIND = 13
OPT_COPY_NT = 14
OPT_RESIZE_WG_WAVES = 15
OPT_DEBUG_COUNTERS = 16
OPT_HUFF_WINDOW = 17
OPT_VIEW_ORDER = 18
OPT_SYNC_CACHE = 19
OPT_SYNC_CACHE_MB = 20
SYNC_CACHE_STATS = ("hits", "misses", "inserts", "refused", "rejected", "fallbacks", "capacity", "bytes")

MAX_OUT = 1024  # LDT_MAX_OUT
DEFAULT_SIZE = (224, 224)


def check_size(size):
    """The one validator of every ``size=`` argument: ``None`` (224, 224), or
    a pair ``(h, w)`` of ints in 1..1024 in torchvision's ``Resize((h, w))``
    order. Returns the pair as a tuple of ints. Needs no device."""
    import operator

    if size is None:
        return DEFAULT_SIZE
    if isinstance(size, bool) or isinstance(size, int) or (hasattr(size, "__index__") and not hasattr(size, "__len__")):
        raise TypeError(
            f"size={size!r}: a bare int means shorter-edge scaling in torchvision's Resize(int), which this "
            "build does not do; pass the output size as a pair (h, w)")
    if isinstance(size, (str, bytes)) or not hasattr(size, "__len__") or not hasattr(size, "__getitem__"):
        raise TypeError(f"size must be a pair (h, w) of ints or None, got {size!r}")
    if len(size) != 2:
        raise ValueError(f"size must be a pair (h, w), got {len(size)} values: {size!r}")
    out = []
    for v in (size[0], size[1]):
        if isinstance(v, bool):
            raise TypeError(f"size must hold ints, got {v!r}")
        try:
            v = operator.index(v)
        except TypeError:
            raise TypeError(f"size must hold ints, got {v!r}") from None
        if not 1 <= v <= MAX_OUT:
            raise ValueError(f"size {tuple(size)!r}: each of (h, w) must be in 1..{MAX_OUT}")
        out.append(v)
    return out[0], out[1]


class ViewSizes(tuple):
    """What ``check_view_sizes`` makes of a size list: a tuple of ``(h, w)``
    pairs of ints, one per view. Its type is what tells a size list from a
    plain ``(h, w)`` everywhere a validated size travels (it pickles as
    itself)."""

    __slots__ = ()

    def __reduce__(self):
        return (ViewSizes, (tuple(self),))

    def __repr__(self):
        return f"ViewSizes({list(self)!r})"

    @property
    def elements(self) -> int:
        """Elements of one row over all views: ``3 * sum(h * w)``."""
        return 3 * sum(h * w for h, w in self)

    def runs(self):
        """The runs of consecutive equal sizes: ``[(first view, count, (h, w)), ...]``."""
        out = []
        for v, hw in enumerate(self):
            if out and out[-1][2] == hw:
                out[-1][1] += 1
            else:
                out.append([v, 1, hw])
        return [tuple(r) for r in out]


def _is_seq(x) -> bool:
    return not isinstance(x, (str, bytes)) and hasattr(x, "__len__") and hasattr(x, "__getitem__")


def check_view_sizes(size):
    """The validator of a ``size=`` argument that may be a size list. ``None``
    or a plain pair ``(h, w)`` goes to ``check_size`` and gives what it gives
    (so everything ``check_size`` refuses stays refused, ``()`` and a bare int
    included). A non-empty sequence of V pairs ``[(h, w), ...]`` (list, tuple
    or ``[V, 2]`` array; V in 1..16, every pair as ``check_size`` wants it) is
    one output size per view: returns a ``ViewSizes``. The form of the
    argument decides, not its values: ``[(8, 8)]`` is a size list of one view.
    Needs no device."""
    if isinstance(size, ViewSizes):
        return size
    if size is None or not _is_seq(size) or len(size) == 0 or not any(_is_seq(v) for v in size):
        return check_size(size)
    if len(size) > MAX_VIEWS:
        raise ValueError(f"size lists {len(size)} views, at most {MAX_VIEWS} (one (h, w) per view)")
    out = []
    for v in size:
        if not _is_seq(v):
            raise TypeError(f"size={size!r}: a size list holds pairs (h, w) only, got {v!r}")
        if len(v) != 2:
            raise ValueError(f"size={size!r}: a size list holds pairs (h, w), got {len(v)} values: {v!r}")
        if any(_is_seq(x) for x in v):
            raise TypeError(f"size={size!r}: a size list holds pairs (h, w) of ints, got {v!r}")
        out.append(check_size(v))
    return ViewSizes(out)


FILTER_BILINEAR = 0  # LDT_FILTER_BILINEAR
FILTER_BICUBIC = 1  # LDT_FILTER_BICUBIC
FILTERS = {"bilinear": FILTER_BILINEAR, "bicubic": FILTER_BICUBIC}
DEFAULT_INTERPOLATION = "bilinear"
_PIL_FILTERS = {0: "nearest", 1: "lanczos", 2: "bilinear", 3: "bicubic", 4: "box", 5: "hamming"}  # Image.Resampling


def check_interpolation(interpolation):
    """The one validator of every ``interpolation=`` argument. Accepts ``None``
    or ``"bilinear"`` (the default), ``"bicubic"`` (any letter case), an object
    whose ``.value`` is one of those strings (torchvision's
    ``InterpolationMode``), and Pillow's ``Image.Resampling.BILINEAR`` /
    ``BICUBIC`` or the ints 2 / 3 they equal. Returns ``"bilinear"`` or
    ``"bicubic"``, which it accepts again. Every other filter is refused by
    name: LANCZOS and HAMMING need sin / cos, whose last bit differs between
    the device and glibc, and NEAREST is not a convolution in Pillow. Needs no
    device."""
    v = interpolation
    if v is None:
        return DEFAULT_INTERPOLATION
    if not isinstance(v, (str, int)) or (isinstance(v, int) and hasattr(v, "value")):
        v = getattr(v, "value", v)  # an enum member: InterpolationMode (str), Image.Resampling (int)
    name = None
    if isinstance(v, str):
        name = v.lower()
    elif isinstance(v, int) and not isinstance(v, bool):
        name = _PIL_FILTERS.get(v)
    if name in FILTERS:
        return name
    what = f"{interpolation!r}" + (f" (Pillow's {name.upper()})" if name and not isinstance(v, str) else "")
    raise ValueError(f"interpolation={what} is not supported: this build resizes with 'bilinear' (the default; "
                     "Pillow's Image.BILINEAR, 2) or 'bicubic' (Image.BICUBIC, 3), each bit-exact with Pillow")


DTYPES = {"float32": 0, "float16": 1, "bfloat16": 2, "uint8": 3}  # LDT_DTYPE_*
LAYOUTS = {"contiguous": 0, "channels_last": 1}  # LDT_LAYOUT_NCHW, LDT_LAYOUT_NHWC
DEFAULT_DTYPE = "float32"
DEFAULT_MEMORY_FORMAT = "contiguous"
DTYPE_BYTES = {"float32": 4, "float16": 2, "bfloat16": 2, "uint8": 1}


def check_dtype(dtype):
    """The one validator of every ``dtype=`` argument. Accepts ``None`` or
    ``torch.float32`` (the default), ``torch.float16`` / ``torch.half``,
    ``torch.bfloat16``, ``torch.uint8`` and the strings ``"float32"``,
    ``"float16"``, ``"half"``, ``"bfloat16"``, ``"uint8"``. Returns one of
    ``"float32"``, ``"float16"``, ``"bfloat16"``, ``"uint8"`` (a picklable
    name, which it accepts again). Anything else is refused by name: nothing
    falls back to float32. Needs no device."""
    if dtype is None:
        return DEFAULT_DTYPE
    name = None
    if isinstance(dtype, str):
        name = "float16" if dtype == "half" else dtype
    elif type(dtype).__module__ == "torch" and type(dtype).__name__ == "dtype":
        name = str(dtype)[len("torch."):]
    if name in DTYPES:
        return name
    raise ValueError(f"dtype={dtype!r} is not supported: the output is torch.float32 (the default), torch.float16, "
                     "torch.bfloat16 or torch.uint8")


def check_memory_format(memory_format):
    """The one validator of every ``memory_format=`` argument. Accepts
    ``None`` or ``torch.contiguous_format`` (the default),
    ``torch.channels_last`` and the strings ``"contiguous"`` and
    ``"channels_last"``. Returns ``"contiguous"`` or ``"channels_last"`` (a
    picklable name, which it accepts again). ``torch.preserve_format`` and
    anything else is refused by name. Needs no device."""
    if memory_format is None:
        return DEFAULT_MEMORY_FORMAT
    name = None
    if isinstance(memory_format, str):
        name = memory_format
    elif type(memory_format).__module__ == "torch" and type(memory_format).__name__ == "memory_format":
        name = {"torch.contiguous_format": "contiguous", "torch.channels_last": "channels_last"}.get(str(memory_format))
    if name in LAYOUTS:
        return name
    raise ValueError(f"memory_format={memory_format!r} is not supported: the output is torch.contiguous_format "
                     "(the default) or torch.channels_last")


def check_format(dtype, memory_format, normalize=None):
    """``(check_dtype(dtype), check_memory_format(memory_format))``, and the
    one rule that joins them to a call's ``normalize``: a uint8 output is the
    resized byte itself, the image before ``ToTensor``, so a Normalize cannot
    apply to it. Needs no device."""
    dtype, memory_format = check_dtype(dtype), check_memory_format(memory_format)
    if dtype == "uint8" and normalize is not None and normalize is not False:
        raise ValueError(f"dtype=torch.uint8 is the resized image before ToTensor: normalize={normalize!r} cannot "
                         "apply to it (pass normalize=None, or a float dtype)")
    return dtype, memory_format


MAX_VIEWS = 16  # LDT_MAX_VIEWS


def check_views(views):
    """The one validator of every ``views=`` argument: ``None`` (one output
    per image, the 4-D tensor) passes through; otherwise an int in 1..16, the
    number of crops / windows taken of every image from a single decode, which
    makes the output ``[views, n, 3, h, w]`` (1 included). Anything else (a
    bool, 0, 17, a float) is refused by name. Returns ``None`` or the int.
    Needs no device."""
    import operator

    if views is None:
        return None
    if isinstance(views, bool):
        raise ValueError(f"views={views!r}: views must be None or an int in 1..{MAX_VIEWS}")
    try:
        v = operator.index(views)
    except TypeError:
        raise ValueError(f"views={views!r}: views must be None or an int in 1..{MAX_VIEWS}") from None
    if not 1 <= v <= MAX_VIEWS:
        raise ValueError(f"views={views!r}: views must be None or an int in 1..{MAX_VIEWS}")
    return v


def check_crops(crops, n, views=None):
    """The one validator of every ``crops=`` argument: ``None`` passes through;
    otherwise an int array-like ``[n, 5]`` of ``(top, left, height, width,
    flip)`` per row, returned as a C-contiguous int32 array (the library's
    ``ldt_crop`` layout). With ``views=V`` (an int from ``check_views``) the
    array must be ``[n, V, 5]``, row ``i``'s view ``v`` at ``[i, v]``; a 2-D
    array is then a ``ValueError``. Whether each box lies inside its image is the
    decode's to say (``LDT_IMG_BAD_CROP`` on that row). Needs no device."""
    import numpy as np

    if crops is None:
        return None
    if hasattr(crops, "detach"):  # a torch tensor
        crops = crops.detach().cpu().numpy()
    a = np.asarray(crops)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"crops must hold ints (top, left, height, width, flip), got dtype {a.dtype}")
    if views is not None:
        if a.ndim != 3 or a.shape[1] != views or a.shape[2] != 5:
            raise ValueError(f"crops must have shape [n, {views}, 5] (views={views}; top, left, height, width, "
                             f"flip), got {a.shape}")
    elif a.ndim != 2 or a.shape[1] != 5:
        raise ValueError(f"crops must have shape [n, 5] (top, left, height, width, flip), got {a.shape}")
    if a.shape[0] != int(n):
        raise ValueError(f"crops for {a.shape[0]} rows, the batch has {int(n)}")
    if a.size and (a.min() < -(1 << 31) or a.max() >= (1 << 31)):
        raise ValueError("crops: a value does not fit int32")
    return np.ascontiguousarray(a, dtype=np.int32)


DRAFT_SCALES = (1, 2, 4, 8)


def check_drafts(drafts, n):
    """The one validator of every ``drafts=`` / ``draft=`` array: ``None``
    passes through; else an int array ``[n]`` of libjpeg scales, each 1, 2, 4
    or 8 (row i decodes to ``ceil(W / s) x ceil(H / s)``, see ``decode_arrow``),
    returned as a contiguous int32 array. Anything else is a ``TypeError`` /
    ``ValueError`` here, before any device is touched."""
    import numpy as np

    if drafts is None:
        return None
    if hasattr(drafts, "detach"):  # a torch tensor
        drafts = drafts.detach().cpu().numpy()
    a = np.asarray(drafts)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"drafts must hold ints (a scale 1, 2, 4 or 8 per row), got dtype {a.dtype}")
    if a.ndim != 1:
        raise ValueError(f"drafts must have shape [n] (one scale per row), got {a.shape}")
    if a.shape[0] != int(n):
        raise ValueError(f"drafts for {a.shape[0]} rows, the batch has {int(n)}")
    bad = ~np.isin(a, DRAFT_SCALES)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise ValueError(f"drafts: row {i} has scale {int(a[i])}, not 1, 2, 4 or 8")
    return np.ascontiguousarray(a, dtype=np.int32)


def draft_sizes(wh, drafts):
    """``wh`` (int ``[n, 2]`` of (width, height), as ``image_sizes`` gives it)
    after the rows' drafts: ``ceil(wh / scale)``, a failed row's (0, 0) staying
    (0, 0). ``drafts`` None: ``wh`` itself."""
    import numpy as np

    if drafts is None:
        return wh
    s = np.asarray(drafts, np.int64)[:, None]
    return ((np.asarray(wh, np.int64) + s - 1) // s).astype(np.int32)


def check_windows(windows, n, views=None):
    """The one validator of every ``windows=`` argument: ``None`` passes
    through; otherwise an int array-like ``[n, 4]`` of ``(res_h, res_w, top,
    left)`` per row, returned as a C-contiguous int32 array (the library's
    ``ldt_window`` layout). With ``views=V`` the array must be ``[n, V, 4]``,
    as ``check_crops`` has it. Whether each window lies inside its resized image
    is the decode's to say (``LDT_IMG_BAD_WINDOW`` on that row). Needs no
    device."""
    import numpy as np

    if windows is None:
        return None
    if hasattr(windows, "detach"):  # a torch tensor
        windows = windows.detach().cpu().numpy()
    a = np.asarray(windows)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"windows must hold ints (res_h, res_w, top, left), got dtype {a.dtype}")
    if views is not None:
        if a.ndim != 3 or a.shape[1] != views or a.shape[2] != 4:
            raise ValueError(f"windows must have shape [n, {views}, 4] (views={views}; res_h, res_w, top, left), "
                             f"got {a.shape}")
    elif a.ndim != 2 or a.shape[1] != 4:
        raise ValueError(f"windows must have shape [n, 4] (res_h, res_w, top, left), got {a.shape}")
    if a.shape[0] != int(n):
        raise ValueError(f"windows for {a.shape[0]} rows, the batch has {int(n)}")
    if a.size and (a.min() < -(1 << 31) or a.max() >= (1 << 31)):
        raise ValueError("windows: a value does not fit int32")
    return np.ascontiguousarray(a, dtype=np.int32)


def color_dtype():
    """The numpy structured dtype of the library's ``ldt_color`` (32 bytes)."""
    import numpy as np

    return np.dtype([("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"), ("hue_shift", "<i4"),
                     ("order", "u1", (4,)), ("mask", "u1"), ("gray", "u1"), ("solarize", "<i2"), ("blur_ww", "<u4"), ("blur_r", "<u2"), ("pad", "u1", (2,))])


BLUR_MAX_RADIUS = 8.0  # Pillow's radius whose box radius is 7, the largest the blur kernel's halo takes


def blur_weights(radius):
    """``(r, ww)`` of Pillow's ``ImageFilter.GaussianBlur(radius)`` as the
    library computes them (``ldt_blur_weights``, the one implementation): the
    whole box radius and the 24-bit tap weight of each of the three extended
    box blurs per axis. ``radius`` in [0, 8.0]; anything else is a
    ``ValueError``. Needs no device."""
    r, ww = ctypes.c_int32(), ctypes.c_uint32()
    if load_library().ldt_blur_weights(float(radius), ctypes.byref(r), ctypes.byref(ww)) != LDT_OK:
        raise ValueError(f"blur radius must be in [0, {BLUR_MAX_RADIUS}] (box radius 7), got {radius!r}")
    return r.value, ww.value


def check_colors(colors, n, views=None):
    """The one validator of every ``colors=`` argument: ``None`` passes
    through; otherwise a float array-like ``[n, 7]`` of ``(brightness,
    contrast, saturation, hue, order, gray, solarize)`` or ``[n, 8]`` with
    ``blur`` as the last column per row, returned as a
    C-contiguous array of ``color_dtype()`` records (the library's
    ``ldt_color`` layout), shape ``[n]``. With ``views=V`` (an int from
    ``check_views``) the array must be ``[n, V, 7]`` or ``[n, V, 8]`` and the
    result is ``[n, V]``; a 2-D array is then a ``ValueError``. A result of
    this function is accepted again and returned as it is. Seven columns give
    the records they always gave, with the blur fields zero.

    ``brightness``, ``contrast``, ``saturation``: the factor, NaN = the op is
    absent, else finite and >= 0; it is stored as the float32 nearest to the
    value, as Pillow's ``(float)alpha`` does. ``hue``: torchvision's
    ``hue_factor`` in [-0.5, 0.5], NaN = absent (0.0 is not absent: the HSV
    round trip is lossy and is performed); stored as ``int(hue * 255)``
    (truncated toward zero) modulo 256. ``order``: ``f0 + 4 * f1 + 16 * f2 + 64
    * f3`` for the permutation ``(f0, f1, f2, f3)`` in which the jitter ops are
    applied (0 brightness, 1 contrast, 2 saturation, 3 hue: torchvision's
    ``fn_idx``), a permutation even when ops are absent. ``gray``: 0 or 1.
    ``solarize``: an integer threshold 0..256, or -1 for none. ``blur``: the
    radius of Pillow's ``ImageFilter.GaussianBlur``, applied after the
    grayscale and before the solarize; NaN or 0 = absent, else finite and in
    (0, 8.0] (8.0 gives the box radius 7, the kernel's limit); stored as the
    weights ``blur_weights`` gives for the float32 nearest to it, as Pillow
    rounds it. A bad value is a ``ValueError``. Needs no device (the blur
    column needs the built library, not a device)."""
    import numpy as np

    if colors is None:
        return None
    dt = color_dtype()
    if hasattr(colors, "detach"):  # a torch tensor
        colors = colors.detach().cpu().numpy()
    a = np.asarray(colors)
    shape = (int(n),) if views is None else (int(n), views)
    if a.dtype == dt:
        if a.shape != shape:
            raise ValueError(f"colors must have shape {list(shape)} (records), got {a.shape}")
        return np.ascontiguousarray(a)
    if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise TypeError("colors must hold numbers (brightness, contrast, saturation, hue, order, gray, solarize), "
                        f"got dtype {a.dtype}")
    if views is not None:
        if a.ndim != 3 or a.shape[1] != views or a.shape[2] not in (7, 8):
            raise ValueError(f"colors must have shape [n, {views}, 7] (views={views}; brightness, contrast, "
                             f"saturation, hue, order, gray, solarize) or [n, {views}, 8] (then blur), got {a.shape}")
    elif a.ndim != 2 or a.shape[1] not in (7, 8):
        raise ValueError("colors must have shape [n, 7] (brightness, contrast, saturation, hue, order, gray, "
                         f"solarize) or [n, 8] (then blur), got {a.shape}")
    if a.shape[0] != int(n):
        raise ValueError(f"colors for {a.shape[0]} rows, the batch has {int(n)}")
    a = a.astype(np.float64)
    out = np.zeros(shape, dt)
    mask = np.zeros(shape, np.uint8)
    for k, name in enumerate(("brightness", "contrast", "saturation")):
        f = a[..., k]
        present = ~np.isnan(f)
        if np.any(present & ~(np.isfinite(f) & (f >= 0))):
            raise ValueError(f"colors: {name} must be NaN (absent) or finite and >= 0")
        with np.errstate(over="ignore"):
            f32 = np.where(present, f, 1.0).astype(np.float32)
        if not np.all(np.isfinite(f32)):
            raise ValueError(f"colors: {name} does not fit float32")
        out[name] = f32
        mask |= present.astype(np.uint8) << k
    hue = a[..., 3]
    present = ~np.isnan(hue)
    if np.any(present & ~((hue >= -0.5) & (hue <= 0.5))):
        raise ValueError("colors: hue must be NaN (absent) or in [-0.5, 0.5]")
    out["hue_shift"] = np.trunc(np.where(present, hue, 0.0) * 255.0).astype(np.int64) & 255
    mask |= present.astype(np.uint8) << 3
    out["mask"] = mask
    for k, name, lo, hi in ((4, "order", 0, 255), (5, "gray", 0, 1), (6, "solarize", -1, 256)):
        v = a[..., k]
        if np.any(~np.isfinite(v)) or np.any(v != np.floor(v)) or np.any((v < lo) | (v > hi)):
            raise ValueError(f"colors: {name} must be an integer in {lo}..{hi}")
    order = a[..., 4].astype(np.int64)
    ops = np.stack([(order >> (2 * k)) & 3 for k in range(4)], axis=-1)
    if np.any(np.sort(ops, axis=-1) != np.arange(4)):
        raise ValueError("colors: order must encode a permutation of the ops 0..3 as f0 + 4*f1 + 16*f2 + 64*f3")
    out["order"] = ops.astype(np.uint8)
    out["gray"] = a[..., 5].astype(np.uint8)
    out["solarize"] = a[..., 6].astype(np.int16)
    if a.shape[-1] == 8:
        blur = a[..., 7]
        present = ~np.isnan(blur) & (blur != 0)
        if np.any(present & ~(np.isfinite(blur) & (blur > 0) & (blur <= BLUR_MAX_RADIUS))):
            raise ValueError(f"colors: blur must be NaN or 0 (absent) or a radius in (0, {BLUR_MAX_RADIUS}] "
                             f"(the limit: box radius 7)")
        for radius in np.unique(blur[present]):
            r, ww = blur_weights(radius)
            at = present & (blur == radius)
            out["blur_r"][at] = r
            out["blur_ww"][at] = ww
    return np.ascontiguousarray(out)


MAX_AUG_OPS = 4  # LDT_MAX_AUG_OPS
# ldt_aug's op codes (LDT_AUG_*)
AUG_IDENTITY, AUG_AFFINE, AUG_BRIGHTNESS, AUG_COLOR, AUG_CONTRAST, AUG_SHARPNESS = 0, 1, 2, 3, 4, 5
AUG_POSTERIZE, AUG_SOLARIZE, AUG_AUTOCONTRAST, AUG_EQUALIZE, AUG_INVERT = 6, 7, 8, 9, 10


def aug_dtype():
    """The numpy structured dtype of the library's ``ldt_aug`` (192 bytes)."""
    import numpy as np

    op = np.dtype([("code", "<i4"), ("param", "<i4"), ("factor", "<f4"), ("fill", "u1", (3,)), ("pad", "u1"),
                   ("a", "<i4", (6,))])
    return np.dtype([("count", "<i4"), ("erase", "<i4", (4,)), ("pad", "<i4", (3,)), ("op", op, (MAX_AUG_OPS,))])


def affine_fix(matrix):
    """Pillow's 16.16 fixed-point form of an output -> input affine matrix
    ``(m0..m5)``, as ``Image.transform(AFFINE, NEAREST)`` walks it and as
    ``ldt_aug`` holds it: ``FIX(v) = floor(v * 65536 + 0.5)`` of ``m0, m1, m2 +
    m0 / 2 + m1 / 2, m3, m4, m5 + m3 / 2 + m4 / 2``. Six Python ints."""
    import math

    m = [float(v) for v in matrix]
    v = (m[0], m[1], m[2] + m[0] * 0.5 + m[1] * 0.5, m[3], m[4], m[5] + m[3] * 0.5 + m[4] * 0.5)
    return [int(math.floor(x * 65536.0 + 0.5)) for x in v]


def _aug_sizes(size, views):
    """[(h, w)] per view from a ``size`` (a pair or a ``ViewSizes``), or None."""
    if size is None:
        return None
    size = check_view_sizes(size)
    nv = 1 if views is None else views
    if isinstance(size, ViewSizes):
        if len(size) != nv:
            raise ValueError(f"augments: the size lists {len(size)} views, the call has {nv}")
        return list(size)
    return [size] * nv


def check_augments(augments, n, views=None, size=None, erase=None):
    """The one validator of every ``augments=`` argument: ``None`` passes
    through (with ``erase`` given it is an array of no ops); a record array
    (``aug_dtype()``, shape ``[n]`` or ``[n, V]``) is returned as it is.
    Otherwise a float array-like ``[n, K, 10]``, K in 1..4, of rows ``(op,
    p0..p5, fill_r, fill_g, fill_b)``: up to K ops per output image, applied in
    order. With ``views=V`` (an int from ``check_views``; a size list implies
    it) the array must be ``[n, V, K, 10]`` and the 3-D form is a
    ``ValueError``. The result is a C-contiguous array of ``aug_dtype()``
    records.

    ``op``: NaN or 0 = absent (absent ops may sit anywhere; the present ones
    keep their order), else an integer code 1..10: 1 affine, 2 brightness,
    3 color, 4 contrast, 5 sharpness, 6 posterize, 7 solarize, 8 autocontrast,
    9 equalize, 10 invert. Affine: ``p0..p5`` is the output -> input matrix that
    Pillow's ``Image.transform(size, AFFINE, data, NEAREST, fillcolor=fill)``
    takes, and ``fill_*`` integers 0..255 (NaN = 0). It is refused when a
    coefficient's magnitude is >= 32768 or, with ``size`` known, a corner of
    the output maps beyond +-32768 or the fixed-point walk leaves int32
    (Pillow leaves its fixed-point path there); and when ``p1 == 0 and p3 ==
    0`` unless ``p0`` and ``p4`` are +-1 and ``p2``, ``p5`` integers (Pillow
    routes pure-scale matrices through another routine; integer translations
    and flips agree on both). The enhance ops (2..5): ``p0`` is the factor,
    finite and >= 0, stored as the float32 nearest to it as Pillow's
    ``(float)alpha`` does. Posterize: ``p0`` = bits, an integer 0..8.
    Solarize: ``p0`` = the threshold, 0 <= p0 <= 256, stored as its ceiling
    (``v < t`` for an integer v). The others take no parameter.

    ``erase``: None, or an int array ``[n, 4]`` (``[n, V, 4]``) of ``(top,
    left, height, width)`` per output image: the box whose stored elements are
    zero (``RandomErasing(value=0)`` after ``Normalize``). ``height == 0`` =
    none; otherwise height and width >= 1, top and left >= 0 and, with ``size``
    known, the box inside that view's output. ``size``: the call's output size
    (a pair, or a ``ViewSizes``); None leaves the checks that need it to the
    decode call. A bad value is a ``ValueError``. Needs no device."""
    import numpy as np

    if augments is None and erase is None:
        return None
    dt = aug_dtype()
    n = int(n)
    shape = (n,) if views is None else (n, views)
    sizes = _aug_sizes(size, views)
    if hasattr(augments, "detach"):
        augments = augments.detach().cpu().numpy()
    a = None if augments is None else np.asarray(augments)
    if a is not None and a.dtype == dt:
        if a.shape != shape:
            raise ValueError(f"augments must have shape {list(shape)} (records), got {a.shape}")
        out = np.ascontiguousarray(a)
        if erase is not None:
            out = out.copy()
    else:
        out = np.zeros(shape, dt)
        if a is not None:
            if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
                raise TypeError(f"augments must hold numbers (op, p0..p5, fill_r, fill_g, fill_b), got dtype {a.dtype}")
            want = 3 if views is None else 4
            if a.ndim != want or a.shape[-1] != 10 or not 1 <= a.shape[-2] <= MAX_AUG_OPS or \
                    (views is not None and a.shape[1] != views):
                raise ValueError(f"augments must have shape [n, {'' if views is None else f'{views}, '}K, 10] with K in "
                                 f"1..{MAX_AUG_OPS} (op, p0..p5, fill_r, fill_g, fill_b), got {a.shape}")
            if a.shape[0] != n:
                raise ValueError(f"augments for {a.shape[0]} rows, the batch has {n}")
            a = a.astype(np.float64).reshape(n, -1, a.shape[-2], 10)
            flat = out.reshape(n, -1)
            for i in range(n):
                for v in range(a.shape[1]):
                    hw = None if sizes is None else sizes[v]
                    k = 0
                    for row in a[i, v]:
                        if np.isnan(row[0]) or row[0] == 0:
                            continue
                        _aug_fill_op(flat[i, v]["op"][k], row, hw)
                        k += 1
                    flat[i, v]["count"] = k
    if erase is not None:
        e = np.asarray(erase.detach().cpu().numpy() if hasattr(erase, "detach") else erase)
        if e.dtype == np.bool_ or not (np.issubdtype(e.dtype, np.floating) or np.issubdtype(e.dtype, np.integer)):
            raise TypeError(f"erase must hold integers (top, left, height, width), got dtype {e.dtype}")
        if e.shape != shape + (4,):
            raise ValueError(f"erase must have shape {list(shape + (4,))} (top, left, height, width), got {e.shape}")
        if e.size and (np.any(~np.isfinite(e.astype(np.float64))) or np.any(e != np.floor(e))):
            raise ValueError("erase: top, left, height and width must be integers")
        e = e.astype(np.int64)
        on = e[..., 2] != 0
        if np.any(on & ((e[..., 0] < 0) | (e[..., 1] < 0) | (e[..., 2] < 1) | (e[..., 3] < 1))) or \
                (e.size and (e.min() < -(1 << 31) or e.max() >= (1 << 31))):
            raise ValueError("erase: a box needs top >= 0, left >= 0, height >= 1 and width >= 1 (height 0 = none)")
        if sizes is not None:
            ev = e.reshape(n, -1, 4)
            for v, (h, w) in enumerate(sizes):
                b = ev[:, v]
                if np.any((b[:, 2] != 0) & ((b[:, 0] + b[:, 2] > h) | (b[:, 1] + b[:, 3] > w))):
                    raise ValueError(f"erase: a box leaves its {h} x {w} output image")
        e = np.where(on[..., None], e, 0)
        out["erase"] = e.astype(np.int32)
    elif sizes is not None and out.size:
        ev = out["erase"].reshape(n, -1, 4).astype(np.int64)
        for v, (h, w) in enumerate(sizes):
            b = ev[:, v]
            if np.any((b[:, 2] != 0) & ((b[:, 0] + b[:, 2] > h) | (b[:, 1] + b[:, 3] > w))):
                raise ValueError(f"erase: a box leaves its {h} x {w} output image")
    return np.ascontiguousarray(out)


MIX_MAX_CLASSES = 1 << 20


def mix_dtype():
    """The numpy structured dtype of the library's ``ldt_mix`` (40 bytes)."""
    import numpy as np

    return np.dtype([("partner", "<i4"), ("w_self", "<f4"), ("w_partner", "<f4"), ("box", "<i4", (4,)),
                     ("lw_self", "<f4"), ("lw_partner", "<f4"), ("pad", "<i4")])


def check_mixes(mix, n, size=None):
    """The one validator of every ``mix=`` / ``mixes=`` argument: ``None``
    passes through; otherwise a pair ``(rows, num_classes)`` and the result is
    ``(records, num_classes)``, the records a C-contiguous ``mix_dtype()`` array
    ``[n]``. ``rows``: such a record array, or a float array-like ``[n, 9]`` of
    ``(partner, w_self, w_partner, top, left, height, width, lw_self,
    lw_partner)`` per row, the weights cast by ``np.float32``. Row ``i`` is
    mixed with row ``partner`` (an integer in ``0..n-1``): inside the box
    ``(top, left, height, width)`` of the output image (``height == 0`` = none)
    the element is the partner's, elsewhere ``partner * w_partner + own *
    w_self`` in float32 (two rounded products, one add); the soft label is
    ``lw_self`` at the row's class and ``lw_partner`` at its partner's.
    ``num_classes``: an integer in ``0..1 << 20``; 0 mixes images only.
    ``size``: the call's output size (a pair), which a box must not leave; None
    leaves that check to the decode call. A bad value is a ``ValueError``.
    Needs no device."""
    import numpy as np

    if mix is None:
        return None
    if isinstance(size, ViewSizes):
        raise ValueError("mix: a size list has several outputs per image; the mix stage serves single-view calls")
    if not isinstance(mix, (tuple, list)) or len(mix) != 2:
        raise ValueError(f"mix must be None, a sampler or a pair (rows, num_classes), got {type(mix).__name__}")
    rows, num_classes = mix
    if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or \
            not 0 <= int(num_classes) <= MIX_MAX_CLASSES:
        raise ValueError(f"mix: num_classes must be an integer in 0..{MIX_MAX_CLASSES}, got {num_classes!r}")
    dt = mix_dtype()
    n = int(n)
    if hasattr(rows, "detach"):
        rows = rows.detach().cpu().numpy()
    a = np.asarray(rows)
    if a.dtype == dt:
        if a.shape != (n,):
            raise ValueError(f"mix rows must have shape [{n}] (records), got {a.shape}")
        out = np.ascontiguousarray(a)
    else:
        if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
            raise TypeError(f"mix rows must hold numbers (partner, w_self, w_partner, top, left, height, width, "
                            f"lw_self, lw_partner), got dtype {a.dtype}")
        if a.ndim != 2 or a.shape[1] != 9:
            raise ValueError(f"mix rows must have shape [n, 9] (partner, w_self, w_partner, top, left, height, width, "
                             f"lw_self, lw_partner), got {a.shape}")
        if a.shape[0] != n:
            raise ValueError(f"mix for {a.shape[0]} rows, the batch has {n}")
        a = a.astype(np.float64)
        ints = a[:, [0, 3, 4, 5, 6]]
        if ints.size and (np.any(~np.isfinite(ints)) or np.any(ints != np.floor(ints)) or
                          np.any(np.abs(ints) >= (1 << 31))):
            raise ValueError("mix: partner, top, left, height and width must be integers")
        out = np.zeros(n, dt)
        out["partner"] = ints[:, 0].astype(np.int64)
        out["box"] = ints[:, 1:].astype(np.int64)
        with np.errstate(over="ignore"):
            for k, name in ((1, "w_self"), (2, "w_partner"), (7, "lw_self"), (8, "lw_partner")):
                out[name] = a[:, k].astype(np.float32)
    if np.any((out["partner"] < 0) | (out["partner"] >= n)):
        raise ValueError(f"mix: a partner is outside 0..{n - 1}")
    for name in ("w_self", "w_partner", "lw_self", "lw_partner"):
        if np.any(~np.isfinite(out[name])):
            raise ValueError(f"mix: {name} must be finite (as float32)")
    box = out["box"].astype(np.int64).reshape(n, 4)
    on = box[:, 2] != 0
    if np.any(on & ((box[:, 0] < 0) | (box[:, 1] < 0) | (box[:, 2] < 1) | (box[:, 3] < 1))):
        raise ValueError("mix: a box needs top >= 0, left >= 0, height >= 1 and width >= 1 (height 0 = none)")
    if size is not None:
        h, w = size
        if np.any(on & ((box[:, 0] + box[:, 2] > h) | (box[:, 1] + box[:, 3] > w))):
            raise ValueError(f"mix: a box leaves the {h} x {w} output image")
    return out, int(num_classes)


def check_mix_labels(labels, num_classes):
    """The int64 ``labels`` of a batch whose mix has ``num_classes`` classes:
    each must be in ``0..num_classes-1`` (``ValueError``)."""
    import numpy as np

    if num_classes > 0 and labels is not None and len(labels):
        lab = np.asarray(labels)
        bad = np.nonzero((lab < 0) | (lab >= num_classes))[0]
        if len(bad):
            raise ValueError(f"mix: row {int(bad[0])} has label {int(lab[bad[0]])}, outside 0..{num_classes - 1}")


def _aug_fill_op(rec, row, hw):
    """One present row ``(op, p0..p5, fill_r, fill_g, fill_b)`` of
    ``check_augments`` into the op record ``rec``; ``hw`` the view's output
    size or None."""
    import math

    op = row[0]
    if not math.isfinite(op) or op != math.floor(op) or not 1 <= op <= AUG_INVERT:
        raise ValueError(f"augments: op must be NaN or 0 (absent) or an integer code in 1..{AUG_INVERT}, got {op!r}")
    op = int(op)
    rec["code"] = op
    p0 = row[1]
    if op == AUG_AFFINE:
        m = [float(x) for x in row[1:7]]
        if not all(math.isfinite(x) and abs(x) < 32768.0 for x in m):
            raise ValueError("augments: an affine coefficient must be finite and of magnitude below 32768")
        if m[1] == 0 and m[3] == 0 and not (abs(m[0]) == 1 and abs(m[4]) == 1 and m[2] == math.floor(m[2])
                                            and m[5] == math.floor(m[5])):
            raise ValueError("augments: an affine matrix with p1 == 0 and p3 == 0 must be an integer translation "
                             "with unit scale (Pillow routes pure-scale matrices through another routine)")
        fix = affine_fix(m)
        if any(not -(1 << 31) <= x < (1 << 31) for x in fix):
            raise ValueError("augments: an affine matrix does not fit Pillow's 16.16 fixed point")
        if hw is not None:
            h, w = hw
            for x, y in ((0, 0), (w, h), (0, h), (w, 0)):
                if not (abs(x * m[0] + y * m[1] + m[2]) < 32768.0 and abs(x * m[3] + y * m[4] + m[5]) < 32768.0):
                    raise ValueError(f"augments: an affine matrix maps a corner of its {h} x {w} output beyond "
                                     "+-32768, where Pillow leaves the fixed-point walk")
                for o in (0, 3):
                    if not -(1 << 31) <= fix[o + 2] + fix[o] * x + fix[o + 1] * y < (1 << 31):
                        raise ValueError(f"augments: an affine matrix's fixed-point walk over its {h} x {w} output "
                                         "leaves int32")
        rec["a"] = fix
        fill = [0.0 if math.isnan(x) else x for x in row[7:10]]
        if not all(math.isfinite(x) and x == math.floor(x) and 0 <= x <= 255 for x in fill):
            raise ValueError("augments: fill must hold integers in 0..255 (NaN = 0)")
        rec["fill"] = [int(x) for x in fill]
    elif op in (AUG_BRIGHTNESS, AUG_COLOR, AUG_CONTRAST, AUG_SHARPNESS):
        import numpy as np

        if not (math.isfinite(p0) and p0 >= 0):
            raise ValueError("augments: an enhance factor must be finite and >= 0")
        with np.errstate(over="ignore"):
            f32 = np.float32(p0)
        if not np.isfinite(f32):
            raise ValueError("augments: an enhance factor does not fit float32")
        rec["factor"] = f32
    elif op == AUG_POSTERIZE:
        if not (math.isfinite(p0) and p0 == math.floor(p0) and 0 <= p0 <= 8):
            raise ValueError("augments: posterize bits must be an integer in 0..8")
        rec["param"] = int(p0)
    elif op == AUG_SOLARIZE:
        if not (math.isfinite(p0) and 0 <= p0 <= 256):
            raise ValueError("augments: the solarize threshold must be in [0, 256]")
        rec["param"] = int(math.ceil(p0))


def image_sizes(cells):
    """``(wh int32 [n, 2], status int32 [n])`` of an Arrow ``binary`` /
    ``large_binary`` array (any offset, nulls allowed) or a sequence of
    ``bytes`` (``None`` = null cell): each JPEG's (width, height) and the
    ``LDT_IMG_*`` code the decode's header walk gives it (``ldt_image_sizes``);
    a failed row has size (0, 0). Host only: no device, no context. For
    sampling crop boxes before the decode."""
    import numpy as np
    import pyarrow as pa

    if isinstance(cells, pa.ChunkedArray):
        cells = cells.combine_chunks()
    if not isinstance(cells, pa.Array):
        cells = pa.array(list(cells), type=pa.binary())
    t = cells.type
    if t == pa.binary() or t == pa.string():
        off64 = 0
    elif t == pa.large_binary() or t == pa.large_string():
        off64 = 1
    else:
        raise TypeError(f"image column must be binary or large_binary, got {t}")
    n = len(cells)
    wh = np.zeros((n, 2), np.int32)
    status = np.zeros(n, np.int32)
    if n == 0:
        return wh, status
    bufs = cells.buffers()
    validity = bufs[0].address if (bufs[0] is not None and cells.null_count) else None
    keep = np.zeros(8, np.uint8)  # all-empty cells: a valid pointer
    data_addr = bufs[2].address if bufs[2] is not None else keep.ctypes.data
    rc = load_library().ldt_image_sizes(data_addr, bufs[1].address, off64, cells.offset, n, validity,
                                        wh.ctypes.data, status.ctypes.data)
    if rc != LDT_OK:
        raise LdtError(f"ldt_image_sizes failed (rc={rc})")
    return wh, status


STAGES = ("h2d", "destuff", "huffman", "idct", "resize", "color")
HOST_PHASES = ("slot", "parse", "plan", "copy_join", "launch", "status", "copy_wake", "copy_span")

# Every symbol include/ldt.h declares (checked by tests/test_abi.py).
EXPORTED = (
    "ldt_create", "ldt_destroy", "ldt_last_error", "ldt_set_option", "ldt_set_copy_stream", "ldt_version",
    "ldt_set_output_size", "ldt_get_output_size", "ldt_set_filter", "ldt_get_filter", "ldt_set_output_format",
    "ldt_get_output_format", "ldt_set_crops", "ldt_set_draft",
    "ldt_set_windows", "ldt_set_views", "ldt_set_view_sizes", "ldt_set_colors", "ldt_blur_weights", "ldt_set_augments", "ldt_set_mix", "ldt_image_sizes", "ldt_decode_batch", "ldt_decode_batch_large", "ldt_decode_batch_resident",
    "ldt_register_host", "ldt_unregister_host", "ldt_fetch_status", "ldt_last_ticket", "ldt_fetch_status_ticket",
    "ldt_stage_times", "ldt_host_times", "ldt_host_info", "ldt_resize_raw", "ldt_shard_ranges",
    "ldt_shard_fragments", "ldt_distributed_indices", "ldt_debug_counters",
    "ldt_sync_cache_stats", "ldt_sync_cache_clear", "ldt_sync_cache_corrupt",
)


class LdtError(RuntimeError):
    """A libldt call failed (argument, HIP runtime or allocation error)."""


class ImageDecodeError(ValueError, OSError):
    """One or more rows could not be decoded.

    Subclasses OSError so code written against the reference (PIL raises
    UnidentifiedImageError / OSError from Image.open at lance_iterable.py:42)
    keeps working, and ValueError per SURVEY.md §8b. ``rows`` maps row index ->
    LDT_IMG_* status. Also constructible from a message string alone, which is
    how torch's DataLoader re-raises an exception caught in a worker or in the
    pin-memory thread (``ExceptionWrapper.reraise``)."""

    def __init__(self, rows):
        if isinstance(rows, str):
            self.rows = {}
            super().__init__(rows)
            return
        self.rows = dict(rows)
        first = sorted(self.rows)[:8]
        desc = "; ".join(f"row {i}: {IMG_STATUS_TEXT.get(self.rows[i], self.rows[i])}" for i in first)
        more = "" if len(self.rows) <= 8 else f" (+{len(self.rows) - 8} more)"
        super().__init__(f"{len(self.rows)} image(s) failed to decode: {desc}{more}")


class Norm(ctypes.Structure):
    _fields_ = [("mean", ctypes.c_float * 3), ("std", ctypes.c_float * 3)]


_lib = None
_lib_lock = threading.Lock()


def load_library(path: str | None = None) -> ctypes.CDLL:
    """Load libldt.so and declare its signatures. Raises if it is missing."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        p = path or os.environ.get("LDT_LIBRARY") or LIB_PATH  # override: experiment builds
        if not os.path.exists(p):
            raise ImportError(
                f"libldt.so not found at {p}: build it with `make -C lance-distributed-training_amd` "
                "or __graft_entry__.build(); the HIP path has no CPU fallback")
        L = ctypes.CDLL(p)
        vp, i64, i32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
        L.ldt_create.argtypes = [i32, sz, i32]
        L.ldt_create.restype = vp
        L.ldt_destroy.argtypes = [vp]
        L.ldt_destroy.restype = None
        L.ldt_last_error.argtypes = [vp]
        L.ldt_last_error.restype = ctypes.c_char_p
        L.ldt_set_option.argtypes = [vp, i32, i64]
        L.ldt_set_copy_stream.argtypes = [vp, vp]
        L.ldt_version.argtypes = []
        L.ldt_version.restype = ctypes.c_char_p
        L.ldt_set_output_size.argtypes = [vp, i32, i32]
        L.ldt_get_output_size.argtypes = [vp, vp, vp]
        L.ldt_set_filter.argtypes = [vp, i32]
        L.ldt_get_filter.argtypes = [vp, vp]
        L.ldt_set_output_format.argtypes = [vp, i32, i32]
        L.ldt_get_output_format.argtypes = [vp, vp, vp]
        L.ldt_set_crops.argtypes = [vp, vp, i64]
        L.ldt_set_windows.argtypes = [vp, vp, i64]
        if hasattr(L, "ldt_set_views"):  # absent from an LDT_LIBRARY built before views (tools/bench_views.py)
            L.ldt_set_views.argtypes = [vp, i32]
            L.ldt_set_views.restype = ctypes.c_int
        if hasattr(L, "ldt_set_view_sizes"):  # absent from an LDT_LIBRARY built before per-view sizes
            L.ldt_set_view_sizes.argtypes = [vp, vp, i32]
            L.ldt_set_view_sizes.restype = ctypes.c_int
        if hasattr(L, "ldt_set_colors"):  # absent from an LDT_LIBRARY built before the photometric stage
            L.ldt_set_colors.argtypes = [vp, vp, i64]
            L.ldt_set_colors.restype = ctypes.c_int
        if hasattr(L, "ldt_set_augments"):  # absent from an LDT_LIBRARY built before the auto-augment stage
            L.ldt_set_augments.argtypes = [vp, vp, i64]
            L.ldt_set_augments.restype = ctypes.c_int
        if hasattr(L, "ldt_set_mix"):  # absent from an LDT_LIBRARY built before the mix stage
            L.ldt_set_mix.argtypes = [vp, vp, i64, ctypes.c_int32, vp]
            L.ldt_set_mix.restype = ctypes.c_int
        if hasattr(L, "ldt_set_draft"):  # absent from an LDT_LIBRARY built before the drafted decode
            L.ldt_set_draft.argtypes = [vp, vp, i64]
            L.ldt_set_draft.restype = ctypes.c_int
        if hasattr(L, "ldt_blur_weights"):  # absent from an LDT_LIBRARY built before the blur
            L.ldt_blur_weights.argtypes = [ctypes.c_float, vp, vp]
            L.ldt_blur_weights.restype = ctypes.c_int
        L.ldt_image_sizes.argtypes = [vp, vp, i32, i64, i64, vp, vp, vp]
        L.ldt_decode_batch.argtypes = [vp, vp, vp, i64, i64, vp, vp, i64, vp, vp, vp, vp, vp]
        L.ldt_decode_batch_large.argtypes = [vp, vp, vp, i64, i64, vp, vp, i64, vp, vp, vp, vp, vp]
        L.ldt_decode_batch_resident.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp]
        L.ldt_fetch_status.argtypes = [vp, vp, vp, i64]
        L.ldt_last_ticket.argtypes = [vp]
        L.ldt_last_ticket.restype = i64
        L.ldt_fetch_status_ticket.argtypes = [vp, i64, vp, i64]
        L.ldt_stage_times.argtypes = [vp, vp, vp, i32]
        L.ldt_host_times.argtypes = [vp, vp, vp, i32]
        L.ldt_host_info.argtypes = [vp, ctypes.c_char_p, sz]
        L.ldt_resize_raw.argtypes = [vp, vp, i32, i64, i32, i32, i64, vp, vp, vp]
        L.ldt_shard_ranges.argtypes = [vp, i64, i64, i32, i32, vp, i64, vp, vp]
        L.ldt_shard_fragments.argtypes = [vp, vp, i32, i64, i32, i32, i64, vp, i64, vp, vp, vp]
        L.ldt_distributed_indices.argtypes = [vp, i64, i32, i32, i32, ctypes.c_uint64, i32, vp, i64,
                                              vp, vp]
        L.ldt_debug_resample_coeffs.argtypes = [vp, i32, i32, vp, vp, vp]
        L.ldt_debug_counters.argtypes = [vp, vp, vp]
        if hasattr(L, "ldt_sync_cache_stats"):  # (an LDT_LIBRARY build from before the sync cache: A/B runs)
            L.ldt_sync_cache_stats.argtypes = [vp, vp]
            L.ldt_sync_cache_clear.argtypes = [vp]
            L.ldt_sync_cache_corrupt.argtypes = [vp, i32]
            for name in ("ldt_sync_cache_stats", "ldt_sync_cache_clear", "ldt_sync_cache_corrupt"):
                getattr(L, name).restype = ctypes.c_int
        L.ldt_debug_last_resize.argtypes = [vp]
        L.ldt_debug_last_resize.restype = ctypes.c_int
        if hasattr(L, "ldt_debug_last_resize_bands"):  # absent from an LDT_LIBRARY built before it
            L.ldt_debug_last_resize_bands.argtypes = [vp]
            L.ldt_debug_last_resize_bands.restype = ctypes.c_int
        if hasattr(L, "ldt_debug_last_idct"):  # absent from an LDT_LIBRARY built before the drafted decode
            L.ldt_debug_last_idct.argtypes = [vp]
            L.ldt_debug_last_idct.restype = ctypes.c_int
        if hasattr(L, "ldt_debug_resample_fills"):  # absent from an LDT_LIBRARY built before the cache
            L.ldt_debug_resample_fills.argtypes = [vp]
            L.ldt_debug_resample_fills.restype = i64
        L.ldt_register_host.argtypes = [vp, vp, sz]
        L.ldt_unregister_host.argtypes = [vp, vp]
        for name in ("ldt_set_option", "ldt_set_copy_stream", "ldt_set_output_size", "ldt_get_output_size",
                     "ldt_set_filter", "ldt_get_filter", "ldt_set_output_format", "ldt_get_output_format",
                     "ldt_set_crops", "ldt_set_windows", "ldt_image_sizes", "ldt_decode_batch", "ldt_decode_batch_large", "ldt_register_host",
                     "ldt_unregister_host",
                     "ldt_decode_batch_resident", "ldt_fetch_status", "ldt_fetch_status_ticket", "ldt_resize_raw", "ldt_stage_times", "ldt_host_times", "ldt_host_info",
                     "ldt_shard_ranges", "ldt_shard_fragments", "ldt_distributed_indices",
                     "ldt_debug_resample_coeffs",
                     "ldt_debug_counters"):
            getattr(L, name).restype = ctypes.c_int
        _lib = L
        return L


class Context:
    """One libldt context per (process, device) — ldt.h threading contract."""

    def __init__(self, device: int):
        self.lib = load_library()
        self.device = int(device)
        self.handle = self.lib.ldt_create(self.device, 0, 0)
        if not self.handle:
            raise LdtError(f"ldt_create(device={device}) failed (no HIP device?)")
        self.lock = threading.Lock()
        self._size = DEFAULT_SIZE  # what the library holds (ldt_set_output_size)
        self._filter = DEFAULT_INTERPOLATION  # likewise (ldt_set_filter)
        self._format = (DEFAULT_DTYPE, DEFAULT_MEMORY_FORMAT)  # likewise (ldt_set_output_format)

    def use_size(self, size) -> None:
        """Make ``size`` (a validated pair) the context's output size, with a
        library call only when it differs from the one in force. Call it with
        ``self.lock`` held, in the critical section of the decode call that
        relies on it: the device's shared context serves callers with
        different sizes. A ``ViewSizes`` (one size per view) is handed to the
        next decode call instead (ldt_set_view_sizes), which consumes it; the
        context's own size stays what it was."""
        if isinstance(size, ViewSizes):
            hw = (ctypes.c_int32 * (2 * len(size)))(*[x for p in size for x in p])
            self.check(self.lib.ldt_set_view_sizes(self.handle, hw, len(size)), "ldt_set_view_sizes")
            return
        if size != self._size:
            self.check(self.lib.ldt_set_output_size(self.handle, size[0], size[1]), "ldt_set_output_size")
            self._size = size

    def use_filter(self, interpolation) -> None:
        """Make ``interpolation`` (a name from ``check_interpolation``) the
        context's filter, as ``use_size`` does the size: with ``self.lock``
        held, in the critical section of the call that relies on it, and with
        a library call only when it differs from the one in force."""
        if interpolation != self._filter:
            self.check(self.lib.ldt_set_filter(self.handle, FILTERS[interpolation]), "ldt_set_filter")
            self._filter = interpolation

    def use_format(self, dtype, memory_format) -> None:
        """Make ``dtype`` / ``memory_format`` (names from ``check_dtype`` and
        ``check_memory_format``) the context's output format, as
        ``use_filter`` does the filter: with ``self.lock`` held, in the
        critical section of the call that relies on it, and with a library
        call only when it differs from the one in force."""
        if (dtype, memory_format) != self._format:
            self.check(self.lib.ldt_set_output_format(self.handle, DTYPES[dtype], LAYOUTS[memory_format]),
                       "ldt_set_output_format")
            self._format = (dtype, memory_format)

    def output_format(self):
        """(dtype, memory_format) names as the library reports them
        (ldt_get_output_format)."""
        d, m = ctypes.c_int(-1), ctypes.c_int(-1)
        self.check(self.lib.ldt_get_output_format(self.handle, ctypes.byref(d), ctypes.byref(m)),
                   "ldt_get_output_format")
        return ({v: k for k, v in DTYPES.items()}[d.value], {v: k for k, v in LAYOUTS.items()}[m.value])

    def filter(self) -> str:
        """The filter's name as the library reports it (ldt_get_filter)."""
        f = ctypes.c_int(-1)
        self.check(self.lib.ldt_get_filter(self.handle, ctypes.byref(f)), "ldt_get_filter")
        return {v: k for k, v in FILTERS.items()}[f.value]

    def use_crops(self, crops) -> None:
        """Hand the next decode / resize call of this context its crops (an
        array from ``check_crops``, or None for none). Call it with
        ``self.lock`` held, right before that call, which consumes them."""
        if crops is not None:
            # [n, 5], or [n, V, 5] image-major: n * V rows
            self.check(self.lib.ldt_set_crops(self.handle, crops.ctypes.data, crops.size // 5), "ldt_set_crops")

    def use_windows(self, windows) -> None:
        """Hand the next decode / resize call of this context its windows (an
        array from ``check_windows``, or None for none), as ``use_crops``
        does its crops: with ``self.lock`` held, right before that call."""
        if windows is not None:
            self.check(self.lib.ldt_set_windows(self.handle, windows.ctypes.data, windows.size // 4),
                       "ldt_set_windows")

    def use_views(self, views) -> None:
        """Hand the next decode call of this context its views (an int from
        ``check_views``, or None for a single-view call), as ``use_crops`` does
        its crops: with ``self.lock`` held, right before that call, which
        consumes the value. ``None`` makes no library call."""
        if views is not None:
            self.check(self.lib.ldt_set_views(self.handle, views), "ldt_set_views")

    def use_colors(self, colors) -> None:
        """Hand the next decode call of this context its colours (records from
        ``check_colors``, ``[n]`` or ``[n, V]`` image-major, or None for none),
        as ``use_crops`` does its crops: with ``self.lock`` held, right before
        that call, which consumes them. ``None`` makes no library call."""
        if colors is not None:
            self.check(self.lib.ldt_set_colors(self.handle, colors.ctypes.data, colors.size), "ldt_set_colors")

    def use_augments(self, augments) -> None:
        """Hand the next decode call of this context its augments (records from
        ``check_augments``, ``[n]`` or ``[n, V]`` image-major, or None for
        none), as ``use_colors`` does its colours: with ``self.lock`` held,
        right before that call, which consumes them. ``None`` makes no library
        call."""
        if augments is not None:
            self.check(self.lib.ldt_set_augments(self.handle, augments.ctypes.data, augments.size),
                       "ldt_set_augments")

    def use_mix(self, mixes) -> None:
        """Hand the next decode call of this context its mix: ``(records,
        num_classes, soft)`` with the records from ``check_mixes`` and ``soft``
        the address of the call's float32 ``[n, num_classes]`` soft-label
        buffer on the device (None with ``num_classes == 0``), or None for
        none, as ``use_augments`` does its augments: with ``self.lock`` held,
        right before that call, which consumes it. ``None`` makes no library
        call."""
        if mixes is not None:
            rows, num_classes, soft = mixes
            self.check(self.lib.ldt_set_mix(self.handle, rows.ctypes.data, rows.size, num_classes, soft),
                       "ldt_set_mix")

    def use_drafts(self, drafts) -> None:
        """Hand the next decode call of this context its draft scales (an int32
        ``[n]`` array from ``check_drafts``, or None for none), as
        ``use_crops`` does its crops: with ``self.lock`` held, right before
        that call, which consumes them. ``None`` makes no library call."""
        if drafts is not None:
            self.check(self.lib.ldt_set_draft(self.handle, drafts.ctypes.data, drafts.size), "ldt_set_draft")

    def arm(self, size, interpolation, dtype, memory_format, crops=None, windows=None, views=None, colors=None,
            augments=None, mixes=None, drafts=None) -> None:
        """Everything the next decode / resize call of this context relies on,
        in the one sequence of ``use_*`` calls there is: call it with
        ``self.lock`` held, right before that call. The arguments are validated
        values (``CallSpec.resolve`` in transforms.py; ``mixes``: the triple
        ``use_mix`` takes; ``drafts``: the scales ``use_drafts`` takes); ``None`` makes no
        library call, so what a caller parked with a ``use_*`` of its own is
        still served. If the library refuses one of them, everything pending
        is cleared before the ``LdtError`` goes on: the call is not going to be
        made, and what stayed parked would be consumed by the context's next
        call, which may be somebody else's."""
        sized = isinstance(size, ViewSizes)
        try:
            if not sized:
                self.use_size(size)
            self.use_filter(interpolation)
            self.use_format(dtype, memory_format)
            self.use_crops(crops)
            self.use_windows(windows)
            self.use_views(views)
            self.use_colors(colors)
            self.use_augments(augments)
            self.use_mix(mixes)
            self.use_drafts(drafts)
            if sized:
                # ldt.h has no call that clears pending view sizes, so they are
                # set last, after everything that can be refused
                self.use_size(size)
        except LdtError:
            for clear in (self.lib.ldt_set_crops, self.lib.ldt_set_windows, self.lib.ldt_set_colors,
                          self.lib.ldt_set_augments):
                clear(self.handle, None, 0)
            self.lib.ldt_set_mix(self.handle, None, 0, 0, None)
            if hasattr(self.lib, "ldt_set_draft"):
                self.lib.ldt_set_draft(self.handle, None, 0)
            self.lib.ldt_set_views(self.handle, 1)
            raise

    def output_size(self):
        """(out_h, out_w) as the library reports it (ldt_get_output_size)."""
        h, w = ctypes.c_int(0), ctypes.c_int(0)
        self.check(self.lib.ldt_get_output_size(self.handle, ctypes.byref(h), ctypes.byref(w)),
                   "ldt_get_output_size")
        return h.value, w.value

    def check(self, rc: int, what: str) -> None:
        if rc == LDT_OK:
            return
        msg = self.lib.ldt_last_error(self.handle).decode(errors="replace")
        raise LdtError(f"{what} failed (rc={rc}): {msg}")

    def set_option(self, opt: int, value: int) -> None:
        self.check(self.lib.ldt_set_option(self.handle, opt, int(value)), "ldt_set_option")

    def set_copy_stream(self, stream) -> None:
        """The stream (a torch.cuda.Stream, or None for the library's own)
        this context's host cells go to HBM on under LDT_OPT_COPY_MODE 0."""
        self.check(self.lib.ldt_set_copy_stream(self.handle, stream.cuda_stream if stream is not None else None),
                   "ldt_set_copy_stream")

    def stage_times(self, reset: bool = False):
        """{stage: (total_ms, launches)} from LDT_OPT_PROFILE events."""
        import numpy as np

        ms = np.zeros(len(STAGES), np.float64)
        cnt = np.zeros(len(STAGES), np.int64)
        self.check(self.lib.ldt_stage_times(self.handle, ms.ctypes.data, cnt.ctypes.data, int(reset)),
                   "ldt_stage_times")
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(STAGES)}

    def host_times(self, reset: bool = False):
        """({phase: total_us}, calls) from LDT_OPT_HOST_TIMING."""
        import numpy as np

        us = np.zeros(len(HOST_PHASES), np.float64)
        calls = ctypes.c_int64(0)
        self.check(self.lib.ldt_host_times(self.handle, us.ctypes.data, ctypes.byref(calls), int(reset)),
                   "ldt_host_times")
        return {k: float(us[i]) for i, k in enumerate(HOST_PHASES)}, int(calls.value)

    def debug_counters(self, stream=None):
        """The parallel Huffman decoder's 16 counters of the last batch
        (LDT_OPT_DEBUG_COUNTERS = 1; layout in ldt.h), as a list of ints."""
        import numpy as np

        out = np.zeros(16, np.int32)
        self.check(self.lib.ldt_debug_counters(self.handle, out.ctypes.data,
                                               stream.cuda_stream if stream is not None else None),
                   "ldt_debug_counters")
        return out.tolist()

    def sync_cache_stats(self) -> dict:
        """The device's sync cache statistics (ldt_sync_cache_stats; counted by
        decodes under OPT_SYNC_CACHE = 2), by name (SYNC_CACHE_STATS)."""
        import numpy as np

        out = np.zeros(8, np.int64)
        self.check(self.lib.ldt_sync_cache_stats(self.handle, out.ctypes.data), "ldt_sync_cache_stats")
        return dict(zip(SYNC_CACHE_STATS, out.tolist()))

    def sync_cache_clear(self) -> None:
        """Empty the device's sync cache (waits for the device)."""
        self.check(self.lib.ldt_sync_cache_clear(self.handle), "ldt_sync_cache_clear")

    def sync_cache_corrupt(self, mode: int) -> int:
        """Test hook (ldt_sync_cache_corrupt): entries changed."""
        rc = self.lib.ldt_sync_cache_corrupt(self.handle, int(mode))
        if rc < 0:
            self.check(rc, "ldt_sync_cache_corrupt")
        return rc

    def host_info(self) -> dict:
        """The host copy placement (ldt_host_info): copy threads and their
        CPUs, the GPU's NUMA node, the cgroup quota, local rank/world."""
        import json

        buf = ctypes.create_string_buffer(4096)
        self.check(self.lib.ldt_host_info(self.handle, buf, len(buf)), "ldt_host_info")
        return json.loads(buf.value.decode())

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                self.lib.ldt_destroy(h)
            except Exception:
                pass
            self.handle = None


_contexts: dict = {}
_ctx_lock = threading.Lock()


def get_context(device: int) -> Context:
    with _ctx_lock:
        ctx = _contexts.get(device)
        if ctx is None:
            ctx = Context(device)
            _contexts[device] = ctx
        return ctx


def version() -> str:
    return load_library().ldt_version().decode()
