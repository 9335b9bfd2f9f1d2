"""The call kinds of the sequence matrix (tests/test_call_sequences.py, tests/test_gpu_call_sequences.py).

A kind is one call of the library with fixed bytes: a name, the keywords of the entry point it goes through, the
``ldt_set_*`` setters that call arms on a fresh context, ``run(ctx, stream=None)``, which makes the call on ``ctx``
and returns host arrays, and ``reference()``, the same arrays from Pillow / the oracle without the library. Every
kind decodes the five cells of tests/test_gpu_pad.py unless its entry in `KINDS` says otherwise. The references are
the feature tests' own helpers (`test_gpu_pad._reference`, `test_gpu_native_sizes._pil`, `test_gpu_draft._pil_view`
and the colour, blur, augment and mix chains), called here, not restated.

A result (of ``run`` and of ``reference``) is a dict: ``images`` a list of arrays (one ``[n, 3, h, w]`` per view, or
one ``[3, h, w]`` per row of a native call; bfloat16 as its int16 bits), and where the call has them ``labels``,
``soft``, ``status`` ({row: LDT_IMG_*} of a failing kind) and ``rc``. A new per-call option adds a kind here.
"""
import functools

import numpy as np
import pyarrow as pa

NAN = float("nan")
N = 5
LABELS = np.arange(100, 100 + N, dtype=np.int64)
SMALL = (30, 33)  # a short last band, single stores
ARROW_KEYS = ("normalize", "size", "interpolation", "dtype", "memory_format", "views", "crops", "windows", "colors",
              "augments", "mixes", "drafts", "pad")  # CallSpec.make's order


@functools.lru_cache(maxsize=None)
def cells():
    """[(bytes, rgb)] of the five cells (tests/test_gpu_pad.py's): 4:2:0 48 x 64, 4:4:0 17 x 5, gray 77 x 91,
    progressive 64 x 80, 4:4:4 8 x 8."""
    import jpeg_recode as jr
    from conftest import read_golden
    from ldt_amd import synth
    from oracle import oracle

    data = [synth.encode(synth.field(48, 64, 201, 6.0)), {c.name: c for c in jr.layout_cells()}["440-17x5"].data,
            read_golden("jpeg/gray_77x91.jpg"), read_golden("jpeg/prog_64x80.jpg"),
            synth.encode(synth.field(8, 8, 205, 6.0), subsampling="4:4:4")]
    return tuple((d, oracle.decode_rgb(d)) for d in data)


@functools.lru_cache(maxsize=None)
def big_cells():
    from ldt_amd import synth
    from oracle import oracle

    data = [synth.encode(synth.field(96, 128, 310 + k, 6.0), subsampling="4:2:0") for k in range(9)]
    return tuple((d, oracle.decode_rgb(d)) for d in data)


def _scan_cut(data: bytes, scan: int) -> bytes:
    """``data`` cut in the middle of the entropy data of its ``scan``-th scan (1 = the first)."""
    at, seen = 2, 0
    while at < len(data):
        assert data[at] == 0xFF, at
        m, size = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        at += 2 + size
        if m != 0xDA:
            continue
        seen, end = seen + 1, at
        while not (data[end] == 0xFF and data[end + 1] != 0 and not 0xD0 <= data[end + 1] <= 0xD7):
            end += 1
        if seen == scan:
            return data[:at + (end - at) // 2]
        at = end
    raise AssertionError(f"no scan {scan}")


def _boxes(shapes):
    """A box of every cell (odd origin where it fits), every other row flipped: tests/test_gpu_pad.py's."""
    return np.array([[h > 8, w > 8, h - (h > 8), w - 2 * (w > 8), k & 1] for k, (h, w) in enumerate(shapes)], np.int32)


def _np(t):
    """A device or host tensor as a host array of its logical (NCHW) order; bfloat16 / float16 as int16 bits."""
    import torch

    t = t.detach().cpu().contiguous()
    return (t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t).numpy()


class Pending:
    """A call that was made: its device tensors, and ``host()``, which reads them (and waits for them)."""

    def __init__(self, ctx, images, labels=None, soft=None, status=None, ticket=None, n=0, rc=None, extra=None,
                 keep=None):
        self.ctx, self.images, self.labels, self.soft, self.status = ctx, images, labels, soft, status
        self.ticket, self.n, self.rc, self.extra, self.keep = ticket, n, rc, extra, keep

    def fetch_status(self):
        """A failing kind's row statuses through the ticket API (what a context under LDT_OPT_SYNC_STATUS = 0 has
        instead of the call's own wait): the device's statuses merged into those the host found. It waits for this
        call alone, and the context holds a call's status until two newer calls were made."""
        if self.ticket is None:
            return
        st = np.zeros(self.n, np.int32)
        for i, s in self.status.items():
            st[i] = s
        rc = self.ctx.lib.ldt_fetch_status_ticket(self.ctx.handle, self.ticket, st.ctypes.data, self.n)
        assert rc in (0, -4), (rc, self.ticket)  # LDT_OK, LDT_ERR_IMAGE
        self.status, self.ticket = {int(i): int(st[i]) for i in np.nonzero(st)[0]}, None

    def host(self):
        self.fetch_status()
        out = {"images": [a for t in self.images for a in ([_np(t)] if t.dim() < 5 else list(_np(t)))]}
        for name in ("labels", "soft"):
            if getattr(self, name) is not None:
                out[name] = _np(getattr(self, name))
        if self.status is not None:
            out["status"] = dict(self.status)
        if self.rc is not None:
            out["rc"] = self.rc
        out.update(self.extra or {})
        return out


class Kind:
    """``api``: "arrow" (decode_arrow), "native" (decode_native), "raw" (resize_raw) or "abi" (the refused call).
    ``kw``: the entry point's keywords. ``fails``: {row: status} the call must report, or None."""

    def __init__(self, name, api, kw, setters, state, batch=cells, fails=None, labels=LABELS):
        self.name, self.api, self.kw, self.setters, self.state = name, api, kw, frozenset(setters), state
        self.batch, self.fails, self.labels = batch, fails, labels

    def __repr__(self):
        return self.name

    @property
    def asynchronous(self):
        return self.api != "abi"

    def data(self):
        return [c[0] for c in self.batch()]

    # ---- the call ------------------------------------------------------------------------------------
    def launch(self, ctx, stream=None):
        import torch

        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            return getattr(self, "_launch_" + self.api)(ctx)

    def run(self, ctx, stream=None):
        return self.launch(ctx, stream).host()

    def _launch_arrow(self, ctx):
        import torch

        import ldt_amd

        arr, kw = pa.array(self.data(), pa.binary()), dict(self.kw)
        if self.fails is None:
            out, lbl = ldt_amd.decode_arrow(arr, self.labels, ctx=ctx, **kw)
            soft = kw.get("mixes") is not None
            return Pending(ctx, list(out) if isinstance(out, tuple) else [out], None if soft else lbl,
                           lbl if soft else None)
        # a failing kind: into the caller's buffers, which the exception leaves readable
        n = len(arr)
        out = torch.full((n, 3) + tuple(kw["size"]), 77.0, device="cuda")
        lbl = torch.full((n,), -777, dtype=torch.int64, device="cuda")
        rows = {}
        try:
            ldt_amd.decode_arrow(arr, self.labels, ctx=ctx, out=out, out_lbl=lbl, **kw)
        except ldt_amd.ImageDecodeError as e:
            rows = dict(e.rows)
        return Pending(ctx, [out], lbl, status=rows, ticket=ctx.lib.ldt_last_ticket(ctx.handle), n=n)

    def _launch_native(self, ctx):
        import ldt_amd

        imgs, lbl = ldt_amd.decode_native(self.data(), self.labels, ctx=ctx, **self.kw)
        return Pending(ctx, imgs, lbl)

    def _launch_raw(self, ctx):
        import torch

        import ldt_amd

        src = torch.from_numpy(raw_cells().copy()).cuda()
        return Pending(ctx, [ldt_amd.resize_raw(src, *RAW_HW, ctx=ctx, **self.kw)], keep=src)

    def _launch_abi(self, ctx):
        """tests/test_gpu_native_sizes.py's ``region-size`` refusal: the offsets give row 1 three elements more
        than its size has."""
        import torch

        import test_gpu_native_sizes as NS

        sizes, offsets = _refused_plan()
        flat = torch.full((int(offsets[-1]) + 8,), 0xFF, dtype=torch.uint8, device="cuda")
        rc, _, _ = NS._abi_call(ctx, self.data(), flat, offsets, sizes)
        return Pending(ctx, [], rc=rc, extra={"sentinel_untouched": bool(flat.cpu().numpy().min() == 0xFF)})

    # ---- the reference -------------------------------------------------------------------------------
    def reference(self):
        return getattr(self, "_reference_" + self.api)()

    def _reference_arrow(self):
        import torch

        import test_gpu_color as C
        import test_gpu_mix as M

        kw, batch = self.kw, self.batch()
        sizes = kw["size"] if isinstance(kw.get("size"), list) else [kw.get("size") or (224, 224)] * (kw.get("views") or 1)
        multi = isinstance(kw.get("size"), list) or kw.get("views") is not None
        dtype = {None: "float32", torch.bfloat16: "bfloat16", torch.uint8: "uint8"}[kw.get("dtype")]
        norm = C._norm_arg(kw.get("normalize"))
        images, fails = [], self.fails or {}
        for v, size in enumerate(sizes):
            rows = []
            for i, (data, rgb) in enumerate(batch):
                if i in fails:
                    rows.append(torch.zeros((3,) + tuple(size), dtype=C._td(dtype)))
                    continue
                pick = lambda a: None if a is None else (np.asarray(a)[i, v] if multi else np.asarray(a)[i])  # noqa: E731
                rows.append(self._row(i, data, rgb, tuple(size), pick(kw.get("crops")), pick(kw.get("windows")), dtype,
                                      norm))
            images.append(torch.stack(rows))
        out = {}
        labels = np.where([i in fails for i in range(len(batch))], -100, self.labels)
        if kw.get("mixes") is not None:
            assert len(images) == 1 and dtype == "float32" and not fails
            rows, nc = kw["mixes"]
            assert nc == M.NC
            images = [M._want(images[0], rows, dtype)]
            out["soft"] = _np(M._want_soft(self.labels, rows))
        else:
            out["labels"] = labels
        out["images"] = [_np(t) for t in images]
        if self.fails is not None:
            out["status"] = dict(fails)
        return out

    def _row(self, i, data, rgb, size, crop, window, dtype, norm):
        """One output image as a CPU tensor [3, h, w] of the call's dtype."""
        import torch

        import ldt_amd
        import test_gpu_affine_filter as AF
        import test_gpu_augment as G
        import test_gpu_blur as B
        import test_gpu_draft as D
        import test_gpu_pad as P
        from draft_ref import drafted_rgb

        kw = self.kw
        interp = kw.get("interpolation") or "bilinear"
        if kw.get("drafts") is not None:  # Pillow's own draft, crop, resize and crop
            assert dtype == "uint8"
            return torch.from_numpy(D._pil_view(drafted_rgb(data, int(kw["drafts"][i])), size, crop, window, interp))
        t, l, bh, bw, flip = (int(x) for x in crop) if crop is not None else (0, 0) + rgb.shape[:2] + (0,)
        window = window if window is not None else size + (0, 0)
        pad = kw.get("pad") or ldt_amd.Pad(0)  # (no overhang without a pad: np.pad by nothing)
        staged = kw.get("colors") is not None or kw.get("augments") is not None or dtype == "uint8"
        ref = P._reference(rgb[t:t + bh, l:l + bw], size, window, flip, pad, None if staged else norm, interp)
        assert not isinstance(ref, int), (self.name, i, ref)
        if not staged:
            return torch.from_numpy(ref).to(G.C._td(dtype))
        u8 = np.ascontiguousarray(np.rint(ref.astype(np.float64) * 255.0).astype(np.uint8).transpose(1, 2, 0))
        erase = None
        if kw.get("colors") is not None:
            u8 = B._pil_chain(u8, ([float(x) for x in np.asarray(kw["colors"])[i]] + [NAN])[:8])
        if kw.get("augments") is not None:
            rows, erase = AUGMENT_ROWS[i], AUGMENT_ERASE[i]
            for row in rows:
                u8 = AF._pil(u8, row)
        return G._expected(u8, None, erase, dtype, norm)

    def _reference_native(self):
        import test_gpu_native as NV
        import test_gpu_native_sizes as NS

        kw, images = self.kw, []
        for i, data in enumerate(self.data()):
            draft = 1 if kw.get("drafts") is None else int(kw["drafts"][i])
            box = None if kw.get("crops") is None else tuple(int(x) for x in kw["crops"][i])
            if kw.get("sizes") is not None:
                images.append(NS._pil(data, tuple(kw["sizes"][i]), kw.get("interpolation") or "bilinear", draft, box))
            else:
                images.append(NV._pil(data, draft, box))
        return {"images": images, "labels": self.labels.copy()}

    def _reference_raw(self):
        import test_gpu_pad as P

        import ldt_amd

        size = self.kw["size"]
        ref = [P._reference(c, size, size + (0, 0), 0, ldt_amd.Pad(0), self.kw.get("normalize")) for c in raw_cells()]
        return {"images": [np.stack(ref)]}

    def _reference_abi(self):
        return {"images": [], "rc": -1, "sentinel_untouched": True}  # LDT_ERR_ARG


RAW_HW = (61, 83)


@functools.lru_cache(maxsize=None)
def raw_cells():
    from ldt_amd import synth

    a = np.stack([synth.raw_hwc_one(*RAW_HW, 71 + k) for k in range(3)])
    a.setflags(write=False)
    return a


def _refused_plan():
    sizes = np.array([[9, 20], [17, 40]], np.int32)
    offsets = np.concatenate([[0], np.cumsum(3 * sizes[:, 0].astype(np.int64) * sizes[:, 1])])
    return sizes, offsets + np.array([0, 0, 3])


def _refused_cells():
    import test_gpu_native_sizes as NS

    return ((NS._cell("b", "420"), None), (NS._cell("a", "444"), None))


# (brightness, contrast, saturation, hue, order, gray, solarize, blur): saturation, brightness, hue, contrast
ORDER2031 = 2 + 4 * 0 + 16 * 3 + 64 * 1
COLOR_ROWS = np.array([[1.3, 0.8, 1.4, 0.1, ORDER2031, 0, 128, 2.0], [NAN, 1.2, NAN, -0.2, ORDER2031, 1, -1, 0.5],
                       [0.7, NAN, 0.3, NAN, ORDER2031, 0, 100, NAN], [1.1, 1.5, 1.9, 0.5, ORDER2031, 0, -1, 2.0],
                       [NAN, NAN, NAN, -0.5, ORDER2031, 1, 200, NAN]], np.float64)
AUGMENT_ERASE = np.array([[13, 1, 4, 8], [0, 0, 0, 0], [15, 4, 2, 3], [0, 0, 30, 33], [29, 30, 1, 3]])


def _augment_rows():
    """[n, 2, 11]: K = 2; a bicubic (rows 0, 2, 4) or a bilinear affine op beside a NEAREST one and the enhance ops."""
    import test_gpu_affine_filter as AF
    import test_gpu_augment as G
    from test_affine_filter_ops import matrix

    even = [AF._filt(2, matrix("rot30", *SMALL)), AF._plain(G._row(4, 1.6))]
    odd = [AF._plain(G._affine("Rotate", -20.0, SMALL, (7, 7, 7))), AF._filt(1, matrix("shearx", *SMALL))]
    return np.array([even, odd, even, odd, [AF._plain(G._row(9)), AF._filt(2, matrix("half", *SMALL))]], np.float64)


def _table():
    import torch

    import ldt_amd
    import test_gpu_mix as M
    import test_gpu_pad as P
    from ldt_amd import _lib

    shapes = [c[1].shape[:2] for c in cells()]
    wh = np.array([s[::-1] for s in shapes], np.int32)
    boxes = _boxes(shapes)
    two = np.stack([boxes, boxes ^ np.array([0, 0, 0, 0, 1], np.int32)], axis=1)  # view 1 mirrored
    center = ldt_amd.ResizeCenterCrop(36).sample(wh, None, SMALL)  # Resize(36) + CenterCrop((30, 33)), as an array
    overhang = np.array([[SMALL[0] - 5, SMALL[1] - 7, -2, -3]] * N, np.int32)  # all four sides
    cut = M._rows(N, box=(14, 2, 3, 5), cut=True)
    mixup = M._rows(N)
    global AUGMENT_ROWS
    AUGMENT_ROWS = _augment_rows()
    augments = _lib.check_augments(AUGMENT_ROWS, N, None, SMALL, AUGMENT_ERASE)
    size, u8 = "ldt_set_output_size", "ldt_set_output_format"
    K = Kind
    return [
        K("plain-224", "arrow", {}, (), "defaults: the fixed band kernel, the d_resamp cache"),
        K("plain-30x33", "arrow", {"size": SMALL}, (size,), "the generic band kernel, d_resamp_g"),
        K("plain-96x160", "arrow", {"size": (96, 160)}, (size,), "a second generic size: the have flags reset"),
        K("plain-299x299", "arrow", {"size": (299, 299)}, (size,), "the streaming kernel, two column tiles"),
        K("bicubic-30x33", "arrow", {"size": SMALL, "interpolation": "bicubic"}, (size, "ldt_set_filter"),
          "the sticky filter"),
        K("crops-flip", "arrow", {"size": SMALL, "crops": boxes}, (size, "ldt_set_crops"), "pending crops"),
        K("windows", "arrow", {"size": SMALL, "windows": center}, (size, "ldt_set_windows"), "pending windows"),
        K("windows-pad-reflect", "arrow", {"size": SMALL, "windows": overhang, "pad": ldt_amd.Pad(0, "reflect")},
          (size, "ldt_set_windows", "ldt_set_pad"), "the pending pad, an index map"),
        K("windows-pad-constant", "arrow", {"size": SMALL, "windows": overhang, "pad": ldt_amd.Pad(P.FILL)},
          (size, "ldt_set_windows", "ldt_set_pad"), "the pending pad, a fill colour"),
        K("views2-crops", "arrow", {"size": SMALL, "views": 2, "crops": two}, (size, "ldt_set_views", "ldt_set_crops"),
          "the view table, view-major output"),
        K("size-list", "arrow", {"size": [SMALL, (7, 5)], "crops": two}, ("ldt_set_views", "ldt_set_view_sizes", "ldt_set_crops"),
          "the view table with a size per view; 7 x 5 is under a band"),
        K("colour", "arrow", {"size": SMALL, "colors": COLOR_ROWS}, (size, "ldt_set_colors"),
          "d_colws and the colour entries; jitter in a non-default order, blur, solarize"),
        K("augment", "arrow", {"size": SMALL, "augments": augments, "normalize": True},
          (size, "ldt_set_augments", "ldt_set_affine_filters"), "d_colws / d_augws ping-pong, the stats, an erase box"),
        K("mix", "arrow", {"size": SMALL, "mixes": (cut, M.NC), "normalize": True}, (size, "ldt_set_mix"),
          "d_mix, the soft labels", labels=M.LABELS),
        K("colour+mix", "arrow", {"size": SMALL, "colors": COLOR_ROWS[:, :7], "mixes": (mixup, M.NC)},
          (size, "ldt_set_colors", "ldt_set_mix"), "the three-buffer ping-pong", labels=M.LABELS),
        K("draft-mixed", "arrow", {"size": SMALL, "drafts": np.array([2, 1, 4, 8, 2], np.int32), "dtype": torch.uint8},
          (size, u8, "ldt_set_draft"), "the scaled IDCT, last_idct_scaled"),
        K("bf16-nhwc-normalize", "arrow", {"size": SMALL, "dtype": torch.bfloat16, "memory_format": torch.channels_last,
                                           "normalize": True}, (size, u8), "the sticky output format"),
        K("uint8", "arrow", {"size": SMALL, "dtype": torch.uint8}, (size, u8), "the sticky output format"),
        K("native", "native", {}, (u8, "ldt_set_native"), "the native offsets, d_planes at each row's own size"),
        K("native-sizes-bicubic", "native",
          {"sizes": [SMALL, (7, 5), (33, 40), (16, 257), (9, 9)], "interpolation": "bicubic"},
          (u8, "ldt_set_filter", "ldt_set_native", "ldt_set_native_sizes"), "the ragged resize"),
        K("native-crops-drafts", "native",
          {"drafts": [2, 1, 1, 2, 1], "crops": [[1, 3, 20, 25, 1], [1, 1, 15, 3, 0], [3, 5, 61, 71, 1],
                                               [1, 1, 30, 37, 0], [0, 0, 8, 8, 1]]},
          (u8, "ldt_set_native", "ldt_set_crops", "ldt_set_draft"), "boxes in drafted coordinates"),
        K("big-first", "arrow", {"size": (64, 64)}, (size,), "every buffer larger than the others need",
          batch=big_cells, labels=np.arange(9, dtype=np.int64)),
        K("bad-rows", "arrow", {"size": SMALL}, (size,), "failed rows: statuses, zero rows",
          batch=lambda: _bad_rows(), fails={1: 1, 3: 3}),
        K("bad-progressive", "arrow", {"size": SMALL}, (size,), "coef_dirty: k_prog output without its k_idct",
          batch=lambda: _bad_progressive(), fails={0: 3}, labels=LABELS[:2]),
        K("refused", "abi", {}, (u8, "ldt_set_native", "ldt_set_native_sizes"), "take_pending on a refusal",
          batch=_refused_cells),
        K("raw", "raw", {"size": SMALL, "normalize": True}, (size,), "d_raw, resize_raw on the same caches"),
    ]


@functools.lru_cache(maxsize=None)
def _bad_rows():
    from conftest import read_golden

    c = cells()
    return (c[0], (read_golden("jpeg/bad_not_jpeg.bin"), None), c[2], (read_golden("jpeg/bad_truncated.bin"), None),
            c[4])


@functools.lru_cache(maxsize=None)
def _bad_progressive():
    c = cells()
    return ((_scan_cut(c[3][0], 2), None), c[3])


AUGMENT_ROWS = None
KINDS = _table()
BY_NAME = {k.name: k for k in KINDS}
EXEMPT = ("bad-rows", "bad-progressive", "refused")  # their refusal is the point


def diff(got, want, what):
    """Raise naming the first differing row and the count of differing bytes unless the results are the same bytes."""
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for key in sorted(want):
        if key != "images":
            g, w = got[key], want[key]
            same = np.array_equal(np.asarray(g).view(np.uint8), np.asarray(w).view(np.uint8)) \
                if isinstance(w, np.ndarray) else g == w
            assert same, f"{what}: {key} differs: {g!r}, expected {w!r}"
    assert len(got["images"]) == len(want["images"]), (what, len(got["images"]), len(want["images"]))
    for k, (g, w) in enumerate(zip(got["images"], want["images"])):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        ne = np.ascontiguousarray(g).view(np.uint8) != np.ascontiguousarray(w).view(np.uint8)
        if ne.any():
            row = k if g.ndim == 3 else int(np.nonzero(ne.reshape(g.shape[0], -1).any(axis=1))[0][0])
            raise AssertionError(f"{what}: image {k}: first differing row {row}, {int(ne.sum())} of {ne.size} "
                                 f"bytes differ")
