"""GPU tests of the drafted decode (ldt_set_draft, ``draft=`` / ``drafts=``):
the DCT-domain 1/2, 1/4 and 1/8 decode against Pillow itself, bit for bit:

    im.draft("RGB", req)  (the scale it picked asserted through the size),
    im.convert("RGB"), then Pillow's crop / resize / crop for the call's geometry.

Every case decodes ``torch.uint8`` where it can, so the bytes themselves are
compared; "identity" cases ask for the drafted size, which a bilinear resize
leaves untouched, so the planes (after upsampling and colour conversion) are
compared. tests/draft_ref.py says how Pillow is made to decode at a scale.

The draft changes nothing before the IDCT, so the cases do not consult the sync
cache: each decode runs through ``huff_paths.uncached`` with the cache switched
off (no counter moves), except the first layout case, which runs
``cold_then_warm`` (phase 1 and the rounds, then the hinted write pass) and
checks both results.
"""
import io

import numpy as np
import pyarrow as pa
import pytest

import huff_paths as hp
import jpeg_recode as jr
import test_gpu_augment as A
import test_gpu_color as C
import test_gpu_mix as M
from conftest import read_golden
from draft_ref import ceil_div, drafted_rgb

pytestmark = pytest.mark.gpu

SCALES = (2, 4, 8)
SMALL = (7, 5)


def _ctx():
    import torch

    from ldt_amd import _lib

    return _lib.get_context(torch.cuda.current_device()), _lib


def _save(arr, **kw) -> bytes:
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(arr)).save(b, format="JPEG", **kw)
    return b.getvalue()


def _field(h, w, seed):
    from ldt_amd import synth

    return synth.field(h, w, seed, 12.0)


@pytest.fixture(scope="module")
def layout_cells():
    """(name, data): 4:4:4, 4:2:2, 4:2:0 and grey from Pillow, 4:4:0, 4:1:1, 4:1:0 and 3x1 re-framed; each at
    67 x 93 (height x width) and at one of 1x1, 8x8, 17x9 and 130x34 (4:2:2 at 17 x 9: cdw == 2 at 1/4, the
    fancy upsampling's small-width exception)."""
    src = jr.layout_source()
    by_name = dict(jr.LAYOUTS)
    cells = []
    pil = (("444", "4:4:4", (1, 1)), ("422", "4:2:2", (9, 17)), ("420", "4:2:0", (34, 130)), ("gray", None, (8, 8)))
    for k, (name, sub, (h2, w2)) in enumerate(pil):
        for h, w in ((67, 93), (h2, w2)):
            a = _field(h, w, 300 + k)
            data = _save(a[:, :, 0], quality=90) if sub is None else _save(a, quality=90, subsampling=sub)
            cells.append((f"{name}-{h}x{w}", data))
    for lname, (h2, w2) in (("440", (9, 17)), ("411", (34, 130)), ("410", (8, 8)), ("3x1", (1, 1))):
        for h, w in ((67, 93), (h2, w2)):
            cells.append((f"{lname}-{h}x{w}", jr.reframe(src, by_name[lname], h, w)))
    return cells


_ref = {}


def _drafted(name, data, s):
    """Pillow's drafted RGB image of the cell at scale s, computed once."""
    if (name, s) not in _ref:
        _ref[name, s] = drafted_rgb(data, s)
    return _ref[name, s]


def _pil_view(im, size, crop=None, window=None, interp="bilinear"):
    """[3, h, w] uint8: Pillow's crop / resize / crop of the PIL image, mirrored when the box says so."""
    from PIL import Image

    flip = 0
    if crop is not None:
        top, left, bh, bw, flip = (int(v) for v in crop)
        im = im.crop((left, top, left + bw, top + bh))
    rh, rw, wt, wl = (int(v) for v in window) if window is not None else (size[0], size[1], 0, 0)
    im = im.resize((rw, rh), Image.BILINEAR if interp == "bilinear" else Image.BICUBIC)
    im = im.crop((wl, wt, wl + size[1], wt + size[0]))
    a = np.asarray(im, dtype=np.uint8)
    return np.ascontiguousarray((a[:, ::-1] if flip else a).transpose(2, 0, 1))


def _decode(cells, drafts, size, ctx=None, labels=None, **kw):
    """decode_arrow of the cells (uint8 unless the call names a dtype). Returns (image CPU numpy or tensor list,
    labels, failed rows); a failed batch's tensors are read all the same."""
    import torch

    import ldt_amd

    kw.setdefault("dtype", torch.uint8)
    n = len(cells)
    views = kw.get("views")
    shape = ((views, n) if views else (n,)) + (3,) + tuple(size)
    out = torch.full(shape, 99, dtype=kw["dtype"], device="cuda")
    if kw.get("memory_format") is torch.channels_last:
        out = out.to(memory_format=torch.channels_last)
    lbl = torch.full((n,), -777, dtype=torch.int64, device="cuda") if labels is not None else None
    failed = {}
    try:
        ldt_amd.decode_arrow(pa.array([d for _, d in cells], pa.binary()), labels, size=size, drafts=drafts, ctx=ctx,
                             out=out, out_lbl=lbl, **kw)
    except ldt_amd.ImageDecodeError as e:
        failed = dict(e.rows)
    torch.cuda.synchronize()
    return out.cpu(), (None if lbl is None else lbl.cpu().numpy()), failed


def _uncached(decode, what):
    run = hp.uncached(_ctx()[0], decode, what=what, cache=0)
    return run.out


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    assert d.max() == 0, f"{what}: {np.count_nonzero(d)} of {d.size} bytes differ, max abs {d.max()}"


# ---- layouts and scales ----------------------------------------------------------------------------

@pytest.mark.parametrize("s", SCALES)
def test_every_layout_small_output(layout_cells, s):
    """All sixteen cells in one batch at scale s, resized to 7 x 5."""
    n = len(layout_cells)
    drafts = np.full(n, s, np.int32)
    want = [_pil_view(_drafted(name, data, s), SMALL) for name, data in layout_cells]
    if s == 2:
        ctx = _ctx()[0]
        dups = hp.key_dups([d for _, d in layout_cells])
        runs = hp.cold_then_warm(ctx, lambda: _decode(layout_cells, drafts, SMALL), dups=dups, what=f"layouts 1/{s}")
        outs = [r.out for r in runs]
    else:
        outs = [_uncached(lambda: _decode(layout_cells, drafts, SMALL), f"layouts 1/{s}")]
    for path, (img, _, failed) in zip(("cold", "warm"), outs):
        assert not failed, (path, failed)
        for k, (name, _) in enumerate(layout_cells):
            _same(img[k].numpy(), want[k], f"{name} 1/{s} -> 7x5 ({path})")


@pytest.mark.parametrize("s", SCALES)
def test_every_layout_identity_size(layout_cells, s):
    """Each cell alone at its drafted size: the planes themselves."""
    for name, data in layout_cells:
        im = _drafted(name, data, s)
        size = (im.size[1], im.size[0])
        want = np.ascontiguousarray(np.asarray(im).transpose(2, 0, 1))
        img, _, failed = _uncached(lambda: _decode([(name, data)], np.array([s], np.int32), size), f"{name} 1/{s}")
        assert not failed, (name, s, failed)
        _same(img[0].numpy(), want, f"{name} 1/{s} identity {size}")


# ---- progressive, restarts -------------------------------------------------------------------------

@pytest.mark.parametrize("s", SCALES)
def test_progressive_sources_and_a_full_decode_after_them(s):
    import jpeg_progressive as jp

    cells = []
    for k, sub in enumerate(("4:4:4", "4:2:0", None)):
        a = _field(67, 93, 320 + k)
        cells.append((f"prog-{sub}", _save(a[:, :, 0], quality=90, progressive=True) if sub is None
                      else _save(a, quality=90, subsampling=sub, progressive=True)))
    sc = next(c for c in jp.script_cells() if c.name.startswith("deep-") and c.height >= 40)
    cells.append(("script-" + sc.name, sc.data))
    n = len(cells)
    img, _, failed = _uncached(lambda: _decode(cells, np.full(n, s, np.int32), SMALL), f"progressive 1/{s}")
    assert not failed, failed
    for k, (name, data) in enumerate(cells):
        _same(img[k].numpy(), _pil_view(_drafted(name, data, s), SMALL), f"{name} 1/{s}")
        im = _drafted(name, data, s)
        one, _, f1 = _uncached(lambda: _decode([cells[k]], np.array([s], np.int32), (im.size[1], im.size[0])),
                               f"{name} 1/{s} identity")
        assert not f1
        _same(one[0].numpy(), np.ascontiguousarray(np.asarray(im).transpose(2, 0, 1)), f"{name} 1/{s} identity")
    # another progressive file at full scale through the same context: pcoef was left all zero
    other = ("prog_64x80", read_golden("jpeg/prog_64x80.jpg"))
    full, _, f2 = _uncached(lambda: _decode([other], None, (64, 80)), "progressive after the drafts")
    assert not f2
    _same(full[0].numpy(), np.ascontiguousarray(np.asarray(drafted_rgb(other[1], 1)).transpose(2, 0, 1)),
          "full-scale progressive decode after drafted ones")


@pytest.mark.parametrize("s", SCALES)
def test_restart_intervals(s):
    from ldt_amd import synth

    cell = ("rst", synth.encode(_field(67, 93, 330), quality=90, restart_marker_rows=1))
    im = _drafted(cell[0], cell[1], s)
    img, _, failed = _uncached(lambda: _decode([cell], np.array([s], np.int32), (im.size[1], im.size[0])), f"rst 1/{s}")
    assert not failed
    _same(img[0].numpy(), np.ascontiguousarray(np.asarray(im).transpose(2, 0, 1)), f"restart intervals 1/{s}")


# ---- a mixed batch, stale workspace ----------------------------------------------------------------

def test_mixed_scales_with_a_truncated_cell(layout_cells):
    by = dict(layout_cells)
    names = ("420-67x93", "444-67x93", "422-67x93", "411-67x93", "gray-67x93")
    cells = [(nm, by[nm]) for nm in names]
    cells.insert(2, ("truncated", by["420-67x93"][:len(by["420-67x93"]) // 2]))
    drafts = np.array([1, 2, 4, 4, 8, 2], np.int32)
    labels = np.arange(10, 16, dtype=np.int64)
    img, lbl, failed = _uncached(lambda: _decode(cells, drafts, SMALL, labels=labels), "mixed scales")
    assert set(failed) == {2}, failed
    assert not img[2].numpy().any() and lbl[2] == -100
    for k, (name, data) in enumerate(cells):
        if k == 2:
            continue
        one, _, f1 = _uncached(lambda: _decode([cells[k]], drafts[k:k + 1], SMALL), f"{name} alone")
        assert not f1
        _same(img[k].numpy(), one[0].numpy(), f"mixed batch row {k} ({name}, 1/{drafts[k]}) against its single-row call")
        _same(img[k].numpy(), _pil_view(_drafted(name, data, int(drafts[k])), SMALL), f"mixed batch row {k} against Pillow")
        assert lbl[k] == labels[k]


def test_stale_workspace_does_not_reach_the_output():
    """An all-white batch at full scale, then drafted cells whose plane rows (blocks_w * s_c = 12, 6 and 3 bytes)
    are narrower than their stride, in the same context: the result equals a fresh context's and Pillow's."""
    import torch

    from ldt_amd import _lib

    white = [("white", _save(np.full((96, 128, 3), 255, np.uint8), quality=90, subsampling="4:4:4"))] * 4
    cells = [("stale-444-9x17", _save(_field(9, 17, 340), quality=90, subsampling="4:4:4")),
             ("stale-422-9x17", _save(_field(9, 17, 341), quality=90, subsampling="4:2:2")),
             ("stale-gray-9x17", _save(_field(9, 17, 342)[:, :, 0], quality=90))]
    ctx = _lib.Context(torch.cuda.current_device())
    for s in SCALES:
        w, _, f0 = _decode(white, None, (96, 128), ctx=ctx)
        assert not f0 and int(w.min()) >= 250
        size = (ceil_div(9, s), ceil_div(17, s))
        drafts = np.full(len(cells), s, np.int32)
        got, _, f1 = _decode(cells, drafts, size, ctx=ctx)
        fresh, _, f2 = _decode(cells, drafts, size, ctx=_lib.Context(torch.cuda.current_device()))
        assert not f1 and not f2
        _same(got.numpy(), fresh.numpy(), f"stale workspace 1/{s}")
        for k, (name, data) in enumerate(cells):
            _same(got[k].numpy(), np.ascontiguousarray(np.asarray(_drafted(name, data, s)).transpose(2, 0, 1)),
                  f"{name} 1/{s} after a white batch")


# ---- composition -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def photo():
    """Three files (4:2:0, 4:4:4, grey) of 150 x 200 with their drafts 2, 4, 2."""
    cells = [("p420", _save(_field(150, 200, 350), quality=90, subsampling="4:2:0")),
             ("p444", _save(_field(150, 200, 351), quality=90, subsampling="4:4:4")),
             ("pgray", _save(_field(150, 200, 352)[:, :, 0], quality=90))]
    return cells, np.array([2, 4, 2], np.int32)


def test_crop_boxes_in_drafted_coordinates_with_flip(photo):
    cells, drafts = photo
    crops = np.array([[3, 5, 60, 80, 1], [1, 2, 30, 40, 0], [10, 0, 65, 100, 1]], np.int32)  # inside 75x100, 38x50, 75x100
    img, _, failed = _uncached(lambda: _decode(cells, drafts, (20, 24), crops=crops), "crops")
    assert not failed
    for k, (name, data) in enumerate(cells):
        _same(img[k].numpy(), _pil_view(_drafted(name, data, int(drafts[k])), (20, 24), crop=crops[k]), f"crop {name}")


def test_window_resize_center_crop_and_the_draft_sampler(photo):
    import ldt_amd

    cells, _ = photo
    d = ldt_amd.Draft((64, 64))  # 150 x 200: k = min(200 // 64, 150 // 64) = 2
    win = ldt_amd.ResizeCenterCrop(64)
    img, _, failed = _uncached(lambda: _decode(cells, d, (56, 56), windows=win), "Draft + ResizeCenterCrop")
    assert not failed
    for k, (name, data) in enumerate(cells):
        im = _drafted(name, data, 2)
        assert im.size == (100, 75)
        w = win.sample(np.array([[100, 75]]), None, (56, 56))[0]
        _same(img[k].numpy(), _pil_view(im, (56, 56), window=w), f"window {name}")


def test_bicubic(photo):
    cells, drafts = photo
    img, _, failed = _uncached(lambda: _decode(cells, drafts, (21, 19), interpolation="bicubic"), "bicubic")
    assert not failed
    for k, (name, data) in enumerate(cells):
        _same(img[k].numpy(), _pil_view(_drafted(name, data, int(drafts[k])), (21, 19), interp="bicubic"), f"bicubic {name}")


def test_two_views_with_a_seeded_sampler(photo):
    import torch

    import ldt_amd

    cells, drafts = photo
    wh = np.array([[100, 75], [50, 38], [100, 75]], np.int32)  # the drafted sizes the sampler must be handed
    torch.manual_seed(11)
    boxes = ldt_amd.RandomResizedCropFlip().sample(wh, np.zeros(3, np.int32), views=2)
    torch.manual_seed(11)
    img, _, failed = _uncached(lambda: _decode(cells, drafts, (20, 24), crops=ldt_amd.RandomResizedCropFlip(), views=2),
                               "views=2")
    assert not failed
    for v in range(2):
        for k, (name, data) in enumerate(cells):
            _same(img[v, k].numpy(), _pil_view(_drafted(name, data, int(drafts[k])), (20, 24), crop=boxes[k, v]),
                  f"view {v} {name}")


def test_a_size_list(photo):
    import torch

    import ldt_amd

    cells, drafts = photo
    sizes = [(20, 24), (9, 7)]
    outs = _uncached(lambda: ldt_amd.decode_arrow(pa.array([d for _, d in cells], pa.binary()), size=sizes, drafts=drafts,
                                                  dtype=torch.uint8)[0], "size list")
    assert len(outs) == 2
    for v, size in enumerate(sizes):
        for k, (name, data) in enumerate(cells):
            _same(outs[v][0, k].cpu().numpy(), _pil_view(_drafted(name, data, int(drafts[k])), size), f"size {size} {name}")


def test_bf16_channels_last_normalize_equals_the_float32_result(photo):
    import torch

    cells, drafts = photo
    f32, _, f0 = _uncached(lambda: _decode(cells, drafts, (20, 24), dtype=torch.float32, normalize=True), "float32")
    b16, _, f1 = _uncached(lambda: _decode(cells, drafts, (20, 24), dtype=torch.bfloat16, normalize=True,
                                           memory_format=torch.channels_last), "bf16 channels_last")
    assert not f0 and not f1
    assert b16.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(b16.contiguous().view(torch.int16), f32.to(torch.bfloat16).contiguous().view(torch.int16))


def test_color_augment_and_mix_sit_behind_the_drafted_resize(photo):
    import torch

    cells, drafts = photo
    size, n = (20, 24), len(cells)
    u8 = [np.ascontiguousarray(_pil_view(_drafted(name, data, int(drafts[k])), size).transpose(1, 2, 0))
          for k, (name, data) in enumerate(cells)]
    rows = np.array([[1.3, 0.7, 1.9, -0.1, 0 + 4 * 1 + 16 * 2 + 64 * 3, 0, -1]] * n)
    img, _, failed = _uncached(lambda: _decode(cells, drafts, size, colors=rows), "color=")
    assert not failed
    for k in range(n):
        C._same(img[k], C._expected(u8[k], rows[k], "uint8"), f"color {cells[k][0]}")
    augs = np.array([[A._row(10), A._row(7, 100.0)]] * n)  # invert, then solarize
    img, _, failed = _uncached(lambda: _decode(cells, drafts, size, augments=augs), "augment=")
    assert not failed
    for k in range(n):
        C._same(img[k], A._expected(u8[k], augs[k], None, "uint8"), f"augment {cells[k][0]}")
    mix = M._rows(n, box=(2, 3, 5, 7))
    ref, _, f0 = _uncached(lambda: _decode(cells, drafts, size, dtype=torch.float32), "mix reference")
    img, _, failed = _uncached(lambda: _decode(cells, drafts, size, dtype=torch.float32, mixes=(mix, 0)), "mix=")
    assert not f0 and not failed
    for k in range(n):  # the reference itself is Pillow's byte / 255
        assert torch.equal(ref[k], torch.from_numpy(u8[k].transpose(2, 0, 1).astype(np.float32) / np.float32(255)))
    assert torch.equal(M._bits(img), M._bits(M._want(ref, mix, "float32")))


# ---- refusals, limits, launches --------------------------------------------------------------------

def test_refusals_and_limits(photo):
    import torch

    import ldt_amd
    from ldt_amd import _lib

    cells, drafts = photo
    # a box inside the file's image and outside the drafted one: its row alone
    crops = np.array([[0, 0, 75, 100, 0], [0, 0, 39, 50, 0], [0, 0, 75, 100, 0]], np.int32)  # row 1: 38 rows
    img, _, failed = _uncached(lambda: _decode(cells, drafts, SMALL, crops=crops), "bad crop")
    assert failed == {1: 6} and not img[1].numpy().any() and img[0].numpy().any()
    # 600 x 40 -> 7 x 5 reduces by 120 > 37: status 4 without a draft, served at 1/8 (75 x 5: by 15)
    wide = [("wide", _save(_field(40, 600, 360), quality=90))]
    _, _, f0 = _uncached(lambda: _decode(wide, None, SMALL), "too large")
    assert f0 == {0: 4}
    img, _, f1 = _uncached(lambda: _decode(wide, np.array([8], np.int32), SMALL), "too large, drafted")
    assert not f1
    _same(img[0].numpy(), _pil_view(_drafted("wide", wide[0][1], 8), SMALL), "600 x 40 at 1/8")
    # resize_raw takes no drafts; a draft parked on the context is refused by ldt_resize_raw and consumed
    raw = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(TypeError, match="drafts"):
        ldt_amd.resize_raw(raw, 8, 8, drafts=np.array([2], np.int32))
    ctx = _ctx()[0]
    with ctx.lock:
        ctx.use_drafts(_lib.check_drafts([2], 1))
    with pytest.raises(_lib.LdtError, match="draft"):
        ldt_amd.resize_raw(raw, 8, 8, normalize=None)
    assert ldt_amd.resize_raw(raw, 8, 8, normalize=None).shape == (1, 3, 224, 224)  # consumed: the next call is served
    # a bad scale: ValueError, nothing enqueued
    before = ctx.lib.ldt_last_ticket(ctx.handle)
    with pytest.raises(ValueError, match="not 1, 2, 4 or 8"):
        _decode(cells, np.array([2, 3, 2], np.int32), SMALL)
    with pytest.raises(ValueError, match="3 rows"):
        _decode(cells[:2], drafts, SMALL)
    assert ctx.lib.ldt_last_ticket(ctx.handle) == before
    # the C entry refuses the same and keeps nothing pending
    bad = np.array([2, 3, 2], np.int32)
    assert ctx.lib.ldt_set_draft(ctx.handle, bad.ctypes.data, 3) != 0
    img, _, failed = _decode(cells, None, (20, 24))  # a plain call: nothing was pending
    assert not failed
    for k, (name, data) in enumerate(cells):
        _same(img[k].numpy(), _pil_view(_drafted(name, data, 1), (20, 24)), f"plain call after the refusals: {name}")


def test_no_draft_and_all_ones_are_the_plain_call(photo):
    """draft=None and all scales 1 give the plain call's tensors, the library reports k_idct as the IDCT kernel
    of both (and k_idct_scaled for a drafted call), and LDT_OPT_PROFILE times each under the one IDCT entry."""
    import torch

    from ldt_amd import _lib

    cells, _ = photo
    ctx = _lib.Context(torch.cuda.current_device())
    ctx.set_option(_lib.OPT_PROFILE, 1)
    assert ctx.lib.ldt_debug_last_idct(ctx.handle) == -1
    plain, _, f0 = _decode(cells, None, (224, 224), ctx=ctx, dtype=torch.float32)
    assert ctx.lib.ldt_debug_last_idct(ctx.handle) == 0
    ones, _, f1 = _decode(cells, np.ones(3, np.int32), (224, 224), ctx=ctx, dtype=torch.float32)
    assert not f0 and not f1
    assert torch.equal(plain, ones)
    assert ctx.lib.ldt_debug_last_idct(ctx.handle) == 0
    for k, (name, data) in enumerate(cells):
        want = _pil_view(drafted_rgb(data, 1), (224, 224)).astype(np.float32) / np.float32(255)
        assert np.array_equal(plain[k].numpy(), want), name
    assert ctx.stage_times()["idct"][1] == 2  # two calls, one IDCT stage each
    _, _, f2 = _decode(cells, np.array([1, 2, 1], np.int32), (224, 224), ctx=ctx, dtype=torch.float32)
    assert not f2 and ctx.lib.ldt_debug_last_idct(ctx.handle) == 1
    assert ctx.stage_times()["idct"][1] == 3  # the scaled kernel under the same entry
    _, _, f3 = _decode(cells, None, (224, 224), ctx=ctx, dtype=torch.float32)
    assert not f3 and ctx.lib.ldt_debug_last_idct(ctx.handle) == 0
