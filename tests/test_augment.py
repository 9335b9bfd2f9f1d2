"""CPU tests of the Python side of ``augment=``: ``check_augments`` (shapes,
every refusal, records accepted again, the erase box rules) and the three
samplers (``TrivialAugmentWide``, ``RandAugment``, ``RandomErasing``): seeded
determinism, pickling, and draws equal to a literal transliteration of
torchvision's ``TrivialAugmentWide.forward``, ``RandAugment.forward``,
``_augmentation_space`` and ``RandomErasing.get_params`` kept below
(torchvision 0.20, ``transforms/autoaugment.py`` and ``transforms/
transforms.py``; torchvision itself is not a dependency). Needs no device.
"""
import math
import pickle

import numpy as np
import pytest
import torch

from ldt_amd import _lib
from ldt_amd import augment as A

NAN = float("nan")


def _row(op, *p, fill=(0, 0, 0)):
    return [float(op)] + [float(x) for x in p] + [NAN] * (6 - len(p)) + [float(x) for x in fill]


# ---- check_augments ----

def test_shapes_with_and_without_views():
    rows = np.full((3, 2, 10), NAN)
    rows[0, 1] = _row(9)
    rows[1] = [_row(4, 1.5), _row(6, 3)]
    rec = _lib.check_augments(rows, 3)
    assert rec.dtype == _lib.aug_dtype() and rec.shape == (3,) and rec.dtype.itemsize == 192
    assert rec["count"].tolist() == [1, 2, 0]
    assert rec["op"]["code"][0, 0] == 9 and rec["op"]["code"][1].tolist()[:2] == [4, 6]  # present ops keep their order
    assert rec["op"]["factor"][1, 0] == np.float32(1.5) and rec["op"]["param"][1, 1] == 3
    assert _lib.check_augments(rec, 3) is rec or np.array_equal(_lib.check_augments(rec, 3), rec)
    assert _lib.check_augments(None, 3) is None
    v = _lib.check_augments(np.broadcast_to(rows[:, None], (3, 2, 2, 10)), 3, views=2)
    assert v.shape == (3, 2) and v["count"].tolist() == [[1, 1], [2, 2], [0, 0]]
    assert np.array_equal(_lib.check_augments(v, 3, views=2), v)
    with pytest.raises(ValueError):
        _lib.check_augments(rows, 3, views=2)  # the 3-D form in a call with views
    with pytest.raises(ValueError):
        _lib.check_augments(rows, 4)  # rows for another batch
    with pytest.raises(ValueError):
        _lib.check_augments(np.full((3, 5, 10), NAN), 3)  # K above 4
    with pytest.raises(ValueError):
        _lib.check_augments(np.full((3, 2, 9), NAN), 3)
    with pytest.raises(ValueError):
        _lib.check_augments(rec, 3, views=2)  # records of the wrong shape
    with pytest.raises(TypeError):
        _lib.check_augments(np.zeros((3, 1, 10), bool), 3)
    # a size list implies its views
    s = _lib.check_augments(np.full((1, 2, 1, 10), NAN), 1, views=2, size=[(8, 8), (4, 4)])
    assert s.shape == (1, 2)
    with pytest.raises(ValueError):
        _lib.check_augments(np.full((1, 2, 1, 10), NAN), 1, views=2, size=[(8, 8)])


def test_affine_fixed_point_and_solarize_ceiling():
    m = (0.9, 0.3, -0.5, -0.3, 0.9, 0.75)
    rec = _lib.check_augments([[_row(1, *m, fill=(9, 8, 7)), _row(7, 246.5)]], 1, size=(20, 30))
    want = [math.floor(v * 65536 + 0.5) for v in (0.9, 0.3, -0.5 + 0.45 + 0.15, -0.3, 0.9, 0.75 - 0.15 + 0.45)]
    assert rec["op"]["a"][0, 0].tolist() == want == _lib.affine_fix(m)
    assert rec["op"]["fill"][0, 0].tolist() == [9, 8, 7]
    assert rec["op"]["param"][0, 1] == 247


@pytest.mark.parametrize("row", [
    _row(11), _row(-1), _row(2.5),  # no such op
    _row(2, -0.1), _row(3, NAN), _row(4, float("inf")), _row(5, 1e39),  # factors
    _row(6, 9), _row(6, 2.5), _row(6, -1),  # bits
    _row(7, 256.5), _row(7, -1), _row(7, NAN),  # threshold
    _row(1, 32768, 0.1, 0, 0.1, 1, 0), _row(1, 1, 0.1, NAN, 0.1, 1, 0),  # a coefficient out of range
    _row(1, 2, 0, 0, 0, 2, 0), _row(1, 1, 0, 0.5, 0, 1, 0), _row(1, 1, 0, 0, 0, 0.5, 0),  # pure scale, no shear
    _row(1, 1, 0.1, 0, 0.1, 1, 0, fill=(256, 0, 0)), _row(1, 1, 0.1, 0, 0.1, 1, 0, fill=(1.5, 0, 0)),
])
def test_refusals_by_name(row):
    with pytest.raises(ValueError, match="augments:"):
        _lib.check_augments([[row]], 1, size=(16, 16))


def test_affine_refusals_that_need_the_size():
    far = _row(1, 1, 0.5, 32000, 0.5, 1, 0)  # every coefficient is fine, a corner of 1024 x 1024 is not
    assert _lib.check_augments([[far]], 1)["count"][0] == 1  # left to the decode call
    assert _lib.check_augments([[far]], 1, size=(8, 8))["count"][0] == 1
    with pytest.raises(ValueError, match="corner"):
        _lib.check_augments([[far]], 1, size=(1024, 1024))
    # integer translations and flips are the one pure-scale family that passes
    for m in ((1, 0, -7, 0, 1, 3), (-1, 0, 16, 0, -1, 16), (1, 0, 0, 0, 1, 0)):
        assert _lib.check_augments([[_row(1, *m)]], 1, size=(16, 16))["count"][0] == 1


def test_erase_box_rules():
    boxes = np.array([[0, 0, 0, 0], [2, 3, 4, 5], [0, 0, 16, 16]])
    rec = _lib.check_augments(None, 3, size=(16, 16), erase=boxes)
    assert rec["count"].tolist() == [0, 0, 0] and rec["erase"].tolist() == boxes.tolist()
    both = _lib.check_augments(np.array([[_row(9)]] * 3), 3, size=(16, 16), erase=boxes)
    assert both["count"].tolist() == [1, 1, 1] and both["erase"].tolist() == boxes.tolist()
    again = _lib.check_augments(both, 3, size=(16, 16))
    assert np.array_equal(again, both)
    assert _lib.check_augments(None, 1, erase=[[9, 9, 0, 7]])["erase"].tolist() == [[0, 0, 0, 0]]  # height 0: none
    for bad in ([[-1, 0, 2, 2]], [[0, -1, 2, 2]], [[0, 0, 2, 0]], [[0, 0, -2, 2]], [[0, 0, 1.5, 2]], [[13, 0, 4, 4]],
                [[0, 13, 4, 4]]):
        with pytest.raises(ValueError, match="erase"):
            _lib.check_augments(None, 1, size=(16, 16), erase=bad)
    with pytest.raises(ValueError, match="erase"):
        _lib.check_augments(None, 2, size=(16, 16), erase=[[0, 0, 1, 1]])  # rows for another batch
    with pytest.raises(ValueError, match="erase"):
        _lib.check_augments(both, 3, size=(8, 8))  # records whose box leaves a smaller output
    v = _lib.check_augments(None, 1, views=2, size=[(16, 16), (4, 4)], erase=[[[0, 0, 16, 16], [1, 1, 3, 3]]])
    assert v.shape == (1, 2)
    with pytest.raises(ValueError, match="erase"):
        _lib.check_augments(None, 1, views=2, size=[(16, 16), (4, 4)], erase=[[[0, 0, 16, 16], [1, 1, 4, 3]]])


# ---- torchvision, transliterated (0.20): the reference of the samplers' draws ----

def _tv_space_wide(num_bins):
    return {
        "Identity": (torch.tensor(0.0), False),
        "ShearX": (torch.linspace(0.0, 0.99, num_bins), True),
        "ShearY": (torch.linspace(0.0, 0.99, num_bins), True),
        "TranslateX": (torch.linspace(0.0, 32.0, num_bins), True),
        "TranslateY": (torch.linspace(0.0, 32.0, num_bins), True),
        "Rotate": (torch.linspace(0.0, 135.0, num_bins), True),
        "Brightness": (torch.linspace(0.0, 0.99, num_bins), True),
        "Color": (torch.linspace(0.0, 0.99, num_bins), True),
        "Contrast": (torch.linspace(0.0, 0.99, num_bins), True),
        "Sharpness": (torch.linspace(0.0, 0.99, num_bins), True),
        "Posterize": (8 - (torch.arange(num_bins) / ((num_bins - 1) / 6)).round().int(), False),
        "Solarize": (torch.linspace(255.0, 0.0, num_bins), False),
        "AutoContrast": (torch.tensor(0.0), False),
        "Equalize": (torch.tensor(0.0), False),
    }


def _tv_space_rand(num_bins, image_size):
    return {
        "Identity": (torch.tensor(0.0), False),
        "ShearX": (torch.linspace(0.0, 0.3, num_bins), True),
        "ShearY": (torch.linspace(0.0, 0.3, num_bins), True),
        "TranslateX": (torch.linspace(0.0, 150.0 / 331.0 * image_size[1], num_bins), True),
        "TranslateY": (torch.linspace(0.0, 150.0 / 331.0 * image_size[0], num_bins), True),
        "Rotate": (torch.linspace(0.0, 30.0, num_bins), True),
        "Brightness": (torch.linspace(0.0, 0.9, num_bins), True),
        "Color": (torch.linspace(0.0, 0.9, num_bins), True),
        "Contrast": (torch.linspace(0.0, 0.9, num_bins), True),
        "Sharpness": (torch.linspace(0.0, 0.9, num_bins), True),
        "Posterize": (8 - (torch.arange(num_bins) / ((num_bins - 1) / 4)).round().int(), False),
        "Solarize": (torch.linspace(255.0, 0.0, num_bins), False),
        "AutoContrast": (torch.tensor(0.0), False),
        "Equalize": (torch.tensor(0.0), False),
    }


def _tv_trivial_forward(num_bins):
    """TrivialAugmentWide.forward up to _apply_op: (op_name, magnitude)."""
    op_meta = _tv_space_wide(num_bins)
    op_index = int(torch.randint(len(op_meta), (1,)).item())
    op_name = list(op_meta.keys())[op_index]
    magnitudes, signed = op_meta[op_name]
    magnitude = (
        float(magnitudes[torch.randint(len(magnitudes), (1,), dtype=torch.long)].item())
        if magnitudes.ndim > 0
        else 0.0
    )
    if signed and torch.randint(2, (1,)):
        magnitude *= -1.0
    return op_name, magnitude


def _tv_rand_forward(num_ops, magnitude_bin, num_bins, height, width):
    """RandAugment.forward up to _apply_op: [(op_name, magnitude)] * num_ops."""
    op_meta = _tv_space_rand(num_bins, (height, width))
    out = []
    for _ in range(num_ops):
        op_index = int(torch.randint(len(op_meta), (1,)).item())
        op_name = list(op_meta.keys())[op_index]
        magnitudes, signed = op_meta[op_name]
        magnitude = float(magnitudes[magnitude_bin].item()) if magnitudes.ndim > 0 else 0.0
        if signed and torch.randint(2, (1,)):
            magnitude *= -1.0
        out.append((op_name, magnitude))
    return out


def _tv_erasing(p, scale, ratio, img_h, img_w):
    """RandomErasing.forward + get_params with value=0: (i, j, h, w) or None."""
    if not torch.rand(1) < p:
        return None
    area = img_h * img_w
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        erase_area = area * torch.empty(1).uniform_(scale[0], scale[1]).item()
        aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
        h = int(round(math.sqrt(erase_area * aspect_ratio)))
        w = int(round(math.sqrt(erase_area / aspect_ratio)))
        if not (h < img_h and w < img_w):
            continue
        i = torch.randint(0, img_h - h + 1, size=(1,)).item()
        j = torch.randint(0, img_w - w + 1, size=(1,)).item()
        return i, j, h, w
    return None


def _tv_apply_op_row(op_name, magnitude, hw, fill=(0, 0, 0)):
    """_apply_op as a row of check_augments (F.affine's matrix through affine_matrix, which
    tests/test_augment_ops.py holds against Pillow)."""
    if op_name in ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate"):
        return _row(1, *A.affine_matrix(op_name, magnitude, hw), fill=fill)
    code = {"Brightness": 2, "Color": 3, "Contrast": 4, "Sharpness": 5}.get(op_name)
    if code:
        return _row(code, 1.0 + magnitude)
    if op_name == "Posterize":
        return _row(6, int(magnitude))
    if op_name == "Solarize":
        return _row(7, magnitude)
    return {"AutoContrast": _row(8), "Equalize": _row(9), "Identity": [NAN] * 10}[op_name]


def _records(rows, n, size, erase=None, views=None):
    return _lib.check_augments(np.array(rows, np.float64), n, views, size, erase)


# ---- the samplers ----

def test_trivial_augment_wide_equals_torchvision_order():
    n, size = 300, (224, 200)
    torch.manual_seed(31)
    got = A.TrivialAugmentWide(fill=(1, 2, 3)).sample(n, size)
    torch.manual_seed(31)
    rows = [[_tv_apply_op_row(*_tv_trivial_forward(31), size, (1, 2, 3))] for _ in range(n)]
    assert np.array_equal(got, _records(rows, n, size))


def test_rand_augment_and_erasing_equal_torchvision_order():
    n, size = 200, (96, 128)
    torch.manual_seed(8)
    got = A.RandAugment(num_ops=3, magnitude=9, erase=A.RandomErasing(p=0.6)).sample(n, size)
    torch.manual_seed(8)
    rows, boxes = [], []
    for _ in range(n):
        rows.append([_tv_apply_op_row(name, m, size) for name, m in _tv_rand_forward(3, 9, 31, *size)])
        boxes.append(_tv_erasing(0.6, (0.02, 0.33), (0.3, 3.3), *size) or (0, 0, 0, 0))
    want = _records(rows, n, size, np.array(boxes))
    assert np.array_equal(got, want)
    assert (want["erase"][:, 2] > 0).sum() > 60 and (want["count"] == 3).any() and (want["count"] < 3).any()
    # alone: RandomErasing as augment=
    torch.manual_seed(9)
    alone = A.RandomErasing(p=0.25).sample(50, size)
    torch.manual_seed(9)
    boxes = [_tv_erasing(0.25, (0.02, 0.33), (0.3, 3.3), *size) or (0, 0, 0, 0) for _ in range(50)]
    assert alone["erase"].tolist() == [list(b) for b in boxes] and not alone["count"].any()


def test_views_and_size_lists_draw_per_image_then_view():
    sizes = [(64, 48), (32, 32)]
    torch.manual_seed(4)
    got = A.RandAugment(erase=A.RandomErasing(p=1.0)).sample(5, sizes)
    torch.manual_seed(4)
    rows, boxes = [], []
    for _ in range(5):
        rows.append([]), boxes.append([])
        for hw in sizes:
            rows[-1].append([_tv_apply_op_row(name, m, hw) for name, m in _tv_rand_forward(2, 9, 31, *hw)])
            boxes[-1].append(_tv_erasing(1.0, (0.02, 0.33), (0.3, 3.3), *hw) or (0, 0, 0, 0))
    assert got.shape == (5, 2)
    assert np.array_equal(got, _records(rows, 5, sizes, np.array(boxes), views=2))
    assert A.TrivialAugmentWide().sample(3, (16, 16), views=2).shape == (3, 2)


def test_seeded_determinism_pickling_and_first_row():
    def gen(seed):
        g = torch.Generator()
        g.manual_seed(seed)
        return g

    for make in (lambda g: A.TrivialAugmentWide(generator=g, erase=A.RandomErasing(generator=g)),
                 lambda g: A.RandAugment(generator=g), lambda g: A.RandomErasing(p=0.9, generator=g)):
        a, b = make(gen(5)).sample(16, (64, 64)), make(gen(5)).sample(16, (64, 64))
        assert np.array_equal(a, b) and not np.array_equal(a, make(gen(6)).sample(16, (64, 64)))
        assert np.array_equal(make(gen(5)).sample(1, (64, 64)), a[:1])  # a single image: the batch's first row
        s = pickle.loads(pickle.dumps(make(None)))
        torch.manual_seed(3)
        x = s.sample(8, (64, 64))
        torch.manual_seed(3)
        assert np.array_equal(x, make(None).sample(8, (64, 64))) and repr(s) == repr(make(None))


def test_every_op_and_every_bin_occurs():
    """20 000 draws through the sampler itself: the records hold every op, and for every op exactly the
    values that its bins and signs give (the geometric ops by their fixed matrices)."""
    size = (224, 200)
    torch.manual_seed(1)
    rec = A.TrivialAugmentWide().sample(20000, size)
    assert (rec["count"] == 0).any()  # Identity
    op = rec["op"][:, 0][rec["count"] == 1]
    space = _tv_space_wide(31)

    def mags(name):
        m, signed = space[name]
        return [s * float(x) for x in m for s in ((1.0, -1.0) if signed else (1.0,))]

    assert set(np.unique(op["code"]).tolist()) == {1, 2, 3, 4, 5, 6, 7, 8, 9}
    # the five geometric ops: every bin and sign of each, as the matrix it becomes
    got = {tuple(a) for a in op["a"][op["code"] == 1].tolist()}
    per_op = {name: {tuple(_lib.affine_fix(A.affine_matrix(name, m, size))) for m in mags(name)}
              for name in ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")}
    assert got == set().union(*per_op.values())
    assert len(per_op["ShearX"]) == len(per_op["ShearY"]) == len(per_op["Rotate"]) == 61  # +-0 is one matrix
    assert len(per_op["TranslateX"]) == len(per_op["TranslateY"]) == 61  # int() of 0, 1.07, ..., 32: 31 values
    # the enhance ops: 61 factors each
    for code, name in ((2, "Brightness"), (3, "Color"), (4, "Contrast"), (5, "Sharpness")):
        want = {np.float32(1.0 + m) for m in mags(name)}
        assert set(op["factor"][op["code"] == code].tolist()) == {float(x) for x in want} and len(want) == 61, name
    assert set(op["param"][op["code"] == 6].tolist()) == {int(m) for m in mags("Posterize")} == {2, 3, 4, 5, 6, 7, 8}
    want = {math.ceil(m) for m in mags("Solarize")}
    assert set(op["param"][op["code"] == 7].tolist()) == want and len(want) == 31
    # RandAugment draws no bin: every op and both signs at its one magnitude
    torch.manual_seed(2)
    ra = A.RandAugment(num_ops=1).sample(5000, size)
    op = ra["op"][:, 0][ra["count"] == 1]
    assert set(np.unique(op["code"]).tolist()) == {1, 2, 3, 4, 5, 6, 7, 8, 9} and (ra["count"] == 0).any()
    assert len({tuple(a) for a in op["a"][op["code"] == 1].tolist()}) == 10  # five ops, two signs
    for code in (2, 3, 4, 5):
        assert len(set(op["factor"][op["code"] == code].tolist())) == 2


def test_constructor_refusals():
    with pytest.raises(ValueError):
        A.RandAugment(num_ops=5)
    with pytest.raises(ValueError):
        A.RandAugment(magnitude=31)
    with pytest.raises(ValueError):
        A.TrivialAugmentWide(interpolation="bilinear")
    with pytest.raises(ValueError):
        A.RandAugment(interpolation=2)
    A.TrivialAugmentWide(interpolation="nearest"), A.RandAugment(interpolation=0)
    with pytest.raises(ValueError):
        A.TrivialAugmentWide(fill=256)
    with pytest.raises(ValueError):
        A.RandomErasing(value=1)
    with pytest.raises(ValueError):
        A.RandomErasing(p=1.5)
    with pytest.raises(TypeError):
        A.TrivialAugmentWide(erase=0.25)
    with pytest.raises(ValueError):
        A.affine_matrix("Scale", 1.0, (8, 8))


def test_color_with_augment_is_refused_without_a_device():
    import ldt_amd
    from ldt_amd import transforms as T

    color, aug = ldt_amd.ColorJitterParams(), ldt_amd.TrivialAugmentWide()
    items = [{"image": b"not decoded", "label": 1}]
    with pytest.raises(ValueError, match="augment"):
        ldt_amd.make_collate_fn(color=color, augment=aug)
    with pytest.raises(ValueError, match="augment"):
        ldt_amd.collate_fn(items, color=color, augment=aug)
    with pytest.raises(ValueError, match="augment"):
        ldt_amd.collate_fn(items, color=np.array([[NAN, NAN, NAN, NAN, 228, 0, -1]]), augment=np.full((1, 1, 10), NAN))
    with pytest.raises(ValueError, match="augment"):
        T.DeviceBatch(T._pack_list([b"x"], [1]), None, None, color=color, augment=aug)
    with pytest.raises(ValueError, match="augment"):
        ldt_amd.DecodePipeline(color=color, augment=aug)
    with pytest.raises(ValueError, match="augment"):
        ldt_amd.make_to_tensor_fn(color=color, augment=aug)
    with pytest.raises(TypeError):
        T.resize_raw(np.zeros((1, 4, 4, 3), np.uint8), 4, 4, augments=aug)
