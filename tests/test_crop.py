"""CPU tests of the per-image crop box and flip (RandomResizedCrop +
RandomHorizontalFlip inside the resize): what needs no GPU.

* The oracle pin: torchvision's ``F.resized_crop`` on a PIL image is
  ``img.crop(box).resize(size, BILINEAR)`` (+ ``transpose(FLIP_LEFT_RIGHT)``),
  and the expected tensors of tests/test_gpu_crop.py come from the oracle as
  ``resize_rgb(decode_rgb(cell)[top:top+bh, left:left+bw], oh, ow)``, mirrored
  when flipped. The two must agree bit for bit.
* ``image_sizes`` (ldt_image_sizes: the planner's marker walk) against
  ``oracle.jpeg_info``.
* ``check_crops``, the one validator of every ``crops=`` argument.
* ``RandomResizedCropFlip``: torchvision is not installed, so the sampler is
  held to the rule its docstring states, recomputed here.
* The planner with crops under AddressSanitizer + UBSan, through the
  stand-alone driver tests/fuzz/crop_plan_check.cpp (its own ``main``, run
  directly).
"""
import glob
import io
import math
import os
import pickle
import shutil
import struct
import subprocess

import numpy as np
import pyarrow as pa
import pytest

import jpeg_recode as jr
from conftest import GOLDEN, REPO, read_golden
from oracle import oracle


def _c4():
    """A 500 x 375 4:2:0 cell with restart rows (not a multiple of its 16 x 16 MCU)."""
    from ldt_amd import synth

    return synth.encode(synth.field(375, 500, 202, 6.0), quality=90, restart_marker_rows=1)


# ---- the oracle composition is Pillow's crop().resize() ---------------------------------

def _pin_cases():
    c4 = _c4()
    l411 = next(c for c in jr.layout_cells() if c.name == "411-33x40")
    gray = read_golden("jpeg/gray_77x91.jpg")
    prog = read_golden("jpeg/prog_64x80.jpg")
    # (name, cell, (top, left, height, width), (oh, ow), flip)
    return [
        ("odd-offsets", c4, (17, 33, 201, 311), (224, 224), 0),
        ("odd-offsets-flipped", c4, (101, 7, 99, 250), (30, 33), 1),
        ("last-pixel", c4, (374, 499, 1, 1), (7, 5), 0),
        ("right-strip", c4, (0, 491, 375, 9), (224, 224), 1),
        ("bottom-right", c4, (300, 401, 75, 99), (299, 299), 0),
        ("upscaled-2x3", c4, (120, 250, 3, 2), (224, 224), 1),
        ("411-odd", l411.data, (5, 3, 20, 30), (30, 33), 1),
        ("gray", gray, (1, 1, 60, 50), (224, 224), 1),
        ("progressive", prog, (13, 9, 40, 51), (7, 5), 0),
    ]


@pytest.mark.parametrize("case", _pin_cases(), ids=lambda c: c[0])
def test_oracle_composition_equals_pillow_crop_resize(case):
    from PIL import Image

    name, cell, (top, left, bh, bw), (oh, ow), flip = case
    im = Image.open(io.BytesIO(cell)).convert("RGB").crop((left, top, left + bw, top + bh))
    im = im.resize((ow, oh), Image.BILINEAR)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    pil = np.asarray(im, dtype=np.uint8)
    rgb = oracle.decode_rgb(cell)
    assert top + bh <= rgb.shape[0] and left + bw <= rgb.shape[1]
    got = oracle.resize_rgb(rgb[top:top + bh, left:left + bw], oh, ow)
    if flip:
        got = got[:, ::-1]
    assert got.shape == pil.shape == (oh, ow, 3)
    assert np.array_equal(got, pil), f"{name}: {np.count_nonzero(got != pil)} values differ"
    # and the tensor the GPU tests compare with: ToTensor of exactly those bytes
    t = oracle.raw_to_tensor(rgb[top:top + bh, left:left + bw], oh, ow)
    if flip:
        t = t[:, :, ::-1]
    assert np.array_equal(t, pil.transpose(2, 0, 1).astype(np.float32) / np.float32(255))


# ---- image_sizes ---------------------------------------------------------------------------

def test_image_sizes_equal_the_oracle():
    import ldt_amd

    cells = [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(GOLDEN, "jpeg", "*.jpg")))]
    assert len(cells) > 20
    cells += [c.data for c in jr.layout_cells()]
    cells += [read_golden("jpeg/prog_375x500_q90.jpg"), read_golden("jpeg/gray_77x91.jpg")]
    want = np.array([oracle.jpeg_info(c)[:2] for c in cells], np.int32)
    for typ in (pa.binary(), pa.large_binary()):
        wh, st = ldt_amd.image_sizes(pa.array(cells, typ))
        assert wh.dtype == np.int32 and st.dtype == np.int32 and wh.shape == (len(cells), 2)
        assert not st.any(), np.nonzero(st)
        assert np.array_equal(wh, want)
    wh, st = ldt_amd.image_sizes(cells)  # a plain list of bytes
    assert np.array_equal(wh, want) and not st.any()


def test_image_sizes_of_bad_rows_and_slices():
    import ldt_amd
    from ldt_amd import _lib

    good = read_golden("jpeg/odd_13x17.jpg")
    gw, gh, _ = oracle.jpeg_info(good)
    rows = [good, read_golden("jpeg/bad_not_jpeg.bin"), b"", None, read_golden("jpeg/bad_cmyk.bin"), good]
    for typ in (pa.binary(), pa.large_binary()):
        arr = pa.array(rows, typ)
        wh, st = ldt_amd.image_sizes(arr)
        assert st.tolist() == [0, _lib.IMG_NOT_JPEG, _lib.IMG_NOT_JPEG, _lib.IMG_NULL, _lib.IMG_UNSUPPORTED, 0]
        assert wh.tolist() == [[gw, gh], [0, 0], [0, 0], [0, 0], [0, 0], [gw, gh]]
        # a slice shares the buffers (offset > 0); the null row keeps its place
        wh2, st2 = ldt_amd.image_sizes(arr.slice(2, 4))
        assert st2.tolist() == st.tolist()[2:] and wh2.tolist() == wh.tolist()[2:]
    wh, st = ldt_amd.image_sizes(pa.array([], pa.binary()))
    assert wh.shape == (0, 2) and st.shape == (0,)
    with pytest.raises(TypeError):
        ldt_amd.image_sizes(pa.array([1, 2]))
    # a truncated cell has its header: the size is known, the decode reports the corruption
    wh, st = ldt_amd.image_sizes([read_golden("jpeg/bad_truncated.bin")])
    assert st.tolist() == [0] and wh[0].tolist() == list(oracle.jpeg_info(read_golden("jpeg/bad_truncated.bin"))[:2])


# ---- check_crops -----------------------------------------------------------------------------

def test_check_crops():
    import torch

    from ldt_amd import check_crops

    assert check_crops(None, 3) is None
    a = check_crops([[0, 0, 5, 6, 1], [1, 2, 3, 4, 0]], 2)
    assert a.dtype == np.int32 and a.shape == (2, 5) and a.flags["C_CONTIGUOUS"]
    assert a.tolist() == [[0, 0, 5, 6, 1], [1, 2, 3, 4, 0]]
    wide = np.arange(20, dtype=np.int64).reshape(2, 10)[:, ::2]  # not contiguous, int64
    assert check_crops(wide, 2).tolist() == wide.tolist() and check_crops(wide, 2).flags["C_CONTIGUOUS"]
    assert check_crops(torch.tensor([[0, 0, 1, 1, 0]]), 1).tolist() == [[0, 0, 1, 1, 0]]
    assert check_crops(np.zeros((0, 5), np.int32), 0).shape == (0, 5)
    for bad in ([[0, 0, 1, 1]], [0, 0, 1, 1, 0], np.zeros((1, 5, 1), np.int32), np.zeros((1, 6), np.int32)):
        with pytest.raises(ValueError):
            check_crops(bad, 1)
    with pytest.raises(ValueError):  # n does not match
        check_crops([[0, 0, 1, 1, 0]], 2)
    with pytest.raises(ValueError):
        check_crops(np.zeros((3, 5), np.int32), 2)
    for bad in (np.zeros((1, 5), np.float32), [[0.5, 0, 1, 1, 0]], np.zeros((1, 5), np.bool_), [["a"] * 5]):
        with pytest.raises(TypeError):
            check_crops(bad, 1)
    with pytest.raises(ValueError):
        check_crops(np.array([[0, 0, 1 << 31, 1, 0]], np.int64), 1)
    # negative values and flip 2 are the decode's to refuse (status 6), not the validator's
    assert check_crops([[-1, -2, 0, 0, 2]], 1).tolist() == [[-1, -2, 0, 0, 2]]


# ---- the sampler -------------------------------------------------------------------------------

def test_sampler_boxes_lie_inside_and_repeat():
    import torch

    from ldt_amd import RandomResizedCropFlip

    rng = np.random.default_rng(5)
    wh = np.stack([rng.integers(1, 801, 2000), rng.integers(1, 601, 2000)], axis=1).astype(np.int32)
    wh[0], wh[1], wh[2] = (1, 1), (800, 600), (800, 1)
    a = RandomResizedCropFlip(generator=torch.Generator().manual_seed(1234)).sample(wh)
    assert a.dtype == np.int32 and a.shape == (2000, 5)
    top, left, h, w, flip = a.T
    assert (top >= 0).all() and (left >= 0).all() and (h >= 1).all() and (w >= 1).all()
    assert (top + h <= wh[:, 1]).all() and (left + w <= wh[:, 0]).all()
    assert set(np.unique(flip)) == {0, 1}
    assert 800 < flip.sum() < 1200  # p = 0.5 over 2000 rows
    assert a[0, :4].tolist() == [0, 0, 1, 1]
    b = RandomResizedCropFlip(generator=torch.Generator().manual_seed(1234)).sample(wh)
    assert np.array_equal(a, b)
    c = RandomResizedCropFlip(generator=torch.Generator().manual_seed(1235)).sample(wh)
    assert not np.array_equal(a, c)
    assert not RandomResizedCropFlip(flip_p=0.0, generator=torch.Generator().manual_seed(1)).sample(wh)[:, 4].any()
    assert RandomResizedCropFlip(flip_p=1.0, generator=torch.Generator().manual_seed(1)).sample(wh)[:, 4].all()


def test_sampler_follows_the_stated_rule():
    """The draws recomputed here from the rule (uniform area, log-uniform
    aspect, randint top then left, rand flip) with the same seed."""
    import torch

    from ldt_amd import RandomResizedCropFlip

    scale, ratio, p = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0), 0.5
    wh = np.array([[500, 375], [64, 80], [33, 40], [1, 1], [8, 800], [800, 8], [13, 17]], np.int32)
    g = torch.Generator().manual_seed(77)
    want = []
    for W, H in wh.tolist():
        lr = torch.log(torch.tensor(ratio))
        box = None
        for _ in range(10):
            area = W * H * torch.empty(1).uniform_(scale[0], scale[1], generator=g).item()
            asp = torch.exp(torch.empty(1).uniform_(lr[0], lr[1], generator=g)).item()
            w, h = int(round(math.sqrt(area * asp))), int(round(math.sqrt(area / asp)))
            if 0 < w <= W and 0 < h <= H:
                top = torch.randint(0, H - h + 1, (1,), generator=g).item()
                left = torch.randint(0, W - w + 1, (1,), generator=g).item()
                box = [top, left, h, w]
                break
        if box is None:
            if W / H < ratio[0]:
                w, h = W, int(round(W / ratio[0]))
            elif W / H > ratio[1]:
                h, w = H, int(round(H * ratio[1]))
            else:
                w, h = W, H
            box = [(H - h) // 2, (W - w) // 2, h, w]
        want.append(box + [int(torch.rand(1, generator=g).item() < p)])
    got = RandomResizedCropFlip(scale, ratio, p, generator=torch.Generator().manual_seed(77)).sample(wh)
    assert got.tolist() == want
    assert got[3, :4].tolist() == [0, 0, 1, 1]


def test_sampler_centre_crop_fallback():
    """8 x 800 (W x H) cannot hold a box of ratio >= 3/4 and area >= 8% unless
    it is tiny: with scale (0.5, 1) every try fails (the narrowest box of area
    >= 3200 is sqrt(3200 * 3/4) = 49 wide) and the centre crop is what the
    rule gives: w = 8, h = round(8 / (3/4)) = 11, top = (800 - 11) // 2."""
    import torch

    from ldt_amd import RandomResizedCropFlip

    s = RandomResizedCropFlip(scale=(0.5, 1.0), generator=torch.Generator().manual_seed(3))
    a = s.sample(np.array([[8, 800], [800, 8], [1, 1]]))
    assert a[0, :4].tolist() == [(800 - 11) // 2, 0, 11, 8] == [394, 0, 11, 8]
    assert a[1, :4].tolist() == [0, (800 - 11) // 2, 8, 11]  # h = 8, w = round(8 * 4/3) = 11
    assert a[2, :4].tolist() == [0, 0, 1, 1]
    assert set(a[:, 4].tolist()) <= {0, 1}


def test_sampler_rng_state_unknown_rows_and_pickle():
    import torch

    from ldt_amd import RandomResizedCropFlip

    wh = np.array([[100, 80], [0, 0], [50, 60]], np.int32)
    torch.manual_seed(11)
    before = torch.get_rng_state()
    a = RandomResizedCropFlip().sample(wh)
    assert not torch.equal(before, torch.get_rng_state()), "the global RNG did not advance"
    torch.manual_seed(11)
    assert np.array_equal(RandomResizedCropFlip().sample(wh), a)  # the global seed decides
    before = torch.get_rng_state()
    g = torch.Generator().manual_seed(11)
    gstate = g.get_state()
    RandomResizedCropFlip(generator=g).sample(wh)
    assert torch.equal(before, torch.get_rng_state()), "a given generator must leave the global RNG alone"
    assert not torch.equal(gstate, g.get_state())
    # unknown sizes: (0, 0, 1, 1, 0), no draw (the rows around it get what they get without it)
    assert a[1].tolist() == [0, 0, 1, 1, 0]
    torch.manual_seed(11)
    assert np.array_equal(RandomResizedCropFlip().sample(wh[[0, 2]]), a[[0, 2]])
    torch.manual_seed(11)
    st = np.array([0, 3, 0], np.int32)
    b = RandomResizedCropFlip().sample(np.array([[100, 80], [40, 40], [50, 60]], np.int32), st)
    assert np.array_equal(b, a)
    s = pickle.loads(pickle.dumps(RandomResizedCropFlip(scale=(0.2, 0.9), ratio=(0.5, 2.0), flip_p=0.25)))
    assert (s.scale, s.ratio, s.flip_p, s.generator) == ((0.2, 0.9), (0.5, 2.0), 0.25, None)
    with pytest.raises(ValueError):
        RandomResizedCropFlip(flip_p=1.5)
    with pytest.raises(ValueError):
        RandomResizedCropFlip().sample(np.zeros((3,), np.int32))


def test_crop_arguments_default_to_none():
    """Every new argument is optional and named as documented."""
    import inspect

    import ldt_amd
    from ldt_amd import transforms as T

    for fn, name in ((T.decode_arrow, "crops"), (T.ResidentBatch.decode, "crops"), (T.resize_raw, "crops"),
                     (T.DecodePipeline.decode, "crops"), (T.collate_fn, "crop"), (T.make_collate_fn, "crop"),
                     (T.DecodePipeline.__init__, "crop"), (T.make_to_tensor_fn, "crop"), (T.DeviceBatch.__init__, "crop")):
        assert inspect.signature(fn).parameters[name].default is None, (fn, name)
    for name in ("RandomResizedCropFlip", "check_crops", "image_sizes"):
        assert hasattr(ldt_amd, name)
    fn = pickle.loads(pickle.dumps(ldt_amd.make_collate_fn(size=(64, 64), crop=ldt_amd.RandomResizedCropFlip())))
    assert isinstance(fn.crop, ldt_amd.RandomResizedCropFlip) and fn.size == (64, 64)


# ---- the planner with crops under sanitizers ----------------------------------------------------

def test_planner_with_crops_under_sanitizers(tmp_path):
    from ldt_amd import synth

    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "crop_plan_check")
    src = [os.path.join(REPO, "tests", "fuzz", "crop_plan_check.cpp"),
           os.path.join(REPO, "lance-distributed-training_amd", "csrc", "ldt_plan.cpp")]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", *src, "-o", exe], check=True)
    cells = [_c4(), synth.encode(synth.field(100, 150, 204, 6.0), subsampling="4:4:4"),
             read_golden("jpeg/gray_77x91.jpg"), read_golden("jpeg/prog_64x80.jpg"),
             synth.encode(synth.field(8, 8, 205, 6.0), subsampling="4:4:4")]
    inp = b"".join(struct.pack("<I", len(c)) + c for c in cells)
    r = subprocess.run([exe], input=inp, capture_output=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    out = r.stdout.decode()
    assert r.returncode == 0 and not r.stderr and "FAIL" not in out, (out[-4000:], r.stderr.decode(errors="replace")[-4000:])
    lines = out.splitlines()
    assert lines[-1] == "crop_plan_ok"
    sizes = [tuple(int(v) for v in x.split()[1:]) for x in lines if x.startswith("size ")]
    assert sizes == [oracle.jpeg_info(c)[:2] for c in cells]
