"""GPU tests of the source pad (``Pad(source=True)``): crop boxes beyond the decoded image. The reference is Pillow
alone (``convert("RGB")``, ``np.pad``, the box, ``resize``, the window, the mirror), compared as uint8 bytes."""
import io

import numpy as np
import pyarrow as pa
import pytest
import torch

import ldt_amd
from conftest import read_golden
from ldt_amd import synth

pytestmark = pytest.mark.gpu

MODES = ["constant", "edge", "reflect", "symmetric"]
FILTERS = ["bilinear", "bicubic"]
FILL = (122, 116, 104)  # CLIP's mean colour, LLaVA's fill


def padded_box(rgb, box, pad):
    """``np.pad(rgb, ..., pad.mode)`` cropped to ``box`` (top, left, h, w, ...)."""
    (t, l, h, w), (H, W) = box[:4], rgb.shape[:2]
    pt, pb, pl, pr = max(0, -t), max(0, t + h - H), max(0, -l), max(0, l + w - W)
    if pad.mode == "constant":
        P = np.stack([np.pad(rgb[..., c], ((pt, pb), (pl, pr)), constant_values=pad.fill[c]) for c in range(3)], -1)
    else:
        P = np.pad(rgb, ((pt, pb), (pl, pr), (0, 0)), mode=pad.mode)
    return np.ascontiguousarray(P[t + pt:t + pt + h, l + pl:l + pl + w])


def reference(rgb, box, size, pad, interp, window=None):
    """The call's uint8 HWC image of one row, by Pillow."""
    from PIL import Image

    rh, rw, wt, wl = window if window is not None else tuple(size) + (0, 0)
    R = np.asarray(Image.fromarray(padded_box(rgb, box, pad)).resize((rw, rh), getattr(Image, interp.upper())))
    R = R[wt:wt + size[0], wl:wl + size[1]]
    return R[:, ::-1] if box[4] else R


@pytest.fixture(scope="module")
def src():
    from PIL import Image

    data = {"odd": synth.encode(synth.field(37, 53, 4)), "folds": synth.encode(synth.field(5, 17, 5)),
            "col": synth.encode(synth.field(9, 1, 6)), "wide": synth.encode(synth.field(16, 64, 7)),
            "tall": synth.encode(synth.field(8, 16, 8)), "gray": read_golden("jpeg/gray_77x91.jpg"),
            "prog": read_golden("jpeg/prog_64x80.jpg"), "bad": read_golden("jpeg/bad_not_jpeg.bin"),
            "48x64": synth.encode(synth.field(48, 64, 9)), "64x48": synth.encode(synth.field(64, 48, 10))}
    return {k: (d, None if k == "bad" else np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))) for k, d in data.items()}


def _decode(src, names, crops, size, pad, interp, **kw):
    """uint8 HWC images [n, h, w, 3] (with views [V, n, h, w, 3]) of a decode_arrow call."""
    kw.setdefault("dtype", torch.uint8)
    out, _ = ldt_amd.decode_arrow(pa.array([src[k][0] for k in names], pa.binary()), size=size, pad=pad,
                                  crops=np.asarray(crops, np.int32), interpolation=interp, **kw)
    return out.movedim(-3, -1).cpu().numpy()


CASES = [  # (source, box, output size)
    ("odd", (-5, -7, 50, 70, 0), (30, 33)),      # overhang on all four sides of a 4:2:0 image odd both ways
    ("odd", (-5, -7, 50, 70, 1), (30, 33)),      # and flipped
    ("folds", (-40, -40, 96, 96, 0), (24, 24)),  # many reflections of 5 x 17
    ("col", (-3, -4, 15, 9, 0), (10, 6)),        # a single column: n == 1 under reflect
    ("odd", (-20, 60, 10, 10, 0), (5, 5)),       # wholly outside: all fill, or the corner pixel under edge
    ("wide", (0, 0, 16, 600, 0), (9, 300)),      # two tiles of 256 columns, the second reads no image column
    ("tall", (0, 0, 40, 16, 0), (20, 16)),       # bands of 8 rows, the third reads no image row
    ("gray", (-10, -12, 100, 110, 0), (30, 33)),
    ("prog", (-9, 30, 80, 70, 0), (30, 33)),
]


@pytest.mark.parametrize("interp", FILTERS)
@pytest.mark.parametrize("mode", MODES)
def test_boxes_beyond_the_image(src, mode, interp):
    pad = ldt_amd.Pad(FILL, mode, source=True)
    for name, box, size in CASES:
        got = _decode(src, [name], [box], size, pad, interp)[0]
        assert np.array_equal(got, reference(src[name][1], box, size, pad, interp)), (name, box, mode, interp)
    inside = [(3, 5, 20, 30, 1)]  # a box inside the image: the bytes of the same call without a pad
    assert np.array_equal(_decode(src, ["odd"], inside, (30, 33), pad, interp), _decode(src, ["odd"], inside, (30, 33), None, interp))


@pytest.mark.parametrize("mode", MODES)
def test_window_views_failed_rows_and_bad_boxes(src, mode):
    pad, rgb = ldt_amd.Pad(FILL, mode, source=True), src["odd"][1]
    boxes = [(-5, -7, 50, 70, 0), (20, -30, 40, 60, 1)]
    # a window inside res, as ResizeCenterCrop gives it
    win = (40, 44, 5, 6)
    got = _decode(src, ["odd"], boxes[:1], (30, 33), pad, "bicubic", windows=np.array([win], np.int32))[0]
    assert np.array_equal(got, reference(rgb, boxes[0], (30, 33), pad, "bicubic", win))
    # two views with different boxes, one decode
    got = _decode(src, ["odd", "gray"], [boxes, boxes], (30, 33), pad, "bilinear", views=2)
    for v, box in enumerate(boxes):
        for i, name in enumerate(["odd", "gray"]):
            assert np.array_equal(got[v, i], reference(src[name][1], box, (30, 33), pad, "bilinear")), (v, name)
    # a corrupt row between good ones stays zero; a box of height 0 and one 8193 wide fail alone
    names = ["odd", "bad", "odd", "odd", "odd"]
    crops = np.array([boxes[0], boxes[0], boxes[1], (0, 0, 0, 5, 0), (-1, -1, 5, 8193, 0)], np.int32)
    out = torch.full((5, 3, 30, 33), 77, dtype=torch.uint8, device="cuda")
    with pytest.raises(ldt_amd.ImageDecodeError) as e:
        ldt_amd.decode_arrow(pa.array([src[k][0] for k in names], pa.binary()), out=out, size=(30, 33), crops=crops,
                             pad=pad, dtype=torch.uint8)
    assert dict(e.value.rows) == {1: 1, 3: 6, 4: 6}
    got = out.movedim(-3, -1).cpu().numpy()
    assert not got[[1, 3, 4]].any()
    for i in (0, 2):
        assert np.array_equal(got[i], reference(rgb, crops[i], (30, 33), pad, "bilinear")), i


@pytest.mark.parametrize("fmt", ["f32", "bf16-cl"])
def test_formats_store_the_table(src, fmt):
    from oracle import oracle

    kw = {"f32": {"dtype": torch.float32},
          "bf16-cl": {"dtype": torch.bfloat16, "memory_format": torch.channels_last}}[fmt]
    pad, box, size = ldt_amd.Pad(FILL, source=True), (-20, -7, 50, 70, 1), (30, 33)
    out, _ = ldt_amd.decode_arrow(pa.array([src["odd"][0]], pa.binary()), size=size, crops=np.array([box], np.int32),
                                  pad=pad, normalize=True, **kw)
    ref = reference(src["odd"][1], box, size, pad, "bilinear")
    assert (ref[0] == FILL).all()  # rows of pure fill: each is the table's entry for the fill byte
    want = torch.from_numpy(oracle.raw_to_tensor(ref, *size, normalize=True)).to(kw["dtype"])  # an identity resize
    assert torch.equal(out[0].cpu(), want)


def test_the_llava_recipe(src):
    names, pad = ["48x64", "64x48"], ldt_amd.Pad(FILL, source=True)
    rb = pa.RecordBatch.from_arrays([pa.array([src[k][0] for k in names], pa.binary()), pa.array([0, 1], pa.int64())],
                                    names=["image", "label"])
    got = ldt_amd.decode_tensor_image(rb, crop=ldt_amd.ExpandToSquare(), pad=pad, size=(24, 24), interpolation="bicubic",
                                      dtype=torch.uint8)["image"].movedim(1, -1).cpu().numpy()
    for i, (k, box) in enumerate(zip(names, [(-8, 0, 64, 64, 0), (0, -8, 64, 64, 0)])):  # expand2square's canvases
        assert np.array_equal(got[i], reference(src[k][1], box, (24, 24), pad, "bicubic")), k
