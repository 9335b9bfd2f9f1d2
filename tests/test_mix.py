"""CPU tests of ``mix=`` / ``mixes=``: ``check_mixes``' refusals by message, the
samplers MixUp / CutMix / MixChoice against torchvision's draw order
(transliterated here: torchvision is not a dependency), the spec every surface
carries, the draw order ending with the mix, ``Context.arm`` and the
``ValueError``s of a mix with views, a size list, uint8 or bad labels. Needs no
device."""
import math
import pickle

import numpy as np
import pyarrow as pa
import pytest
import torch

import ldt_amd
from ldt_amd import _lib
from ldt_amd import transforms as T

N = 4
CELLS = [b"cell-%d" % i for i in range(N)]  # never decoded
NC = 10


def _items():
    return [{"image": c, "label": i} for i, c in enumerate(CELLS)]


def _rb():
    return pa.RecordBatch.from_arrays([pa.array(CELLS, pa.binary()), pa.array(range(N), pa.int64())],
                                      ["image", "label"])


def _good():
    return np.array([[(i - 1) % N, 0.75, 0.25, 1, 2, 3, 4, 0.75, 0.25] for i in range(N)], np.float64)


# ---- check_mixes ----------------------------------------------------------------------------------

def test_check_mixes_builds_the_records():
    assert _lib.check_mixes(None, N) is None
    assert _lib.mix_dtype().itemsize == 40
    rows, nc = _lib.check_mixes((_good(), NC), N, (8, 8))
    assert nc == NC and rows.dtype == _lib.mix_dtype() and rows.shape == (N,) and rows.flags.c_contiguous
    assert rows["partner"].tolist() == [3, 0, 1, 2] and rows["box"].tolist() == [[1, 2, 3, 4]] * N
    lam = 0.123456789
    a = _good()
    a[:, 1], a[:, 2], a[:, 7], a[:, 8] = lam, 1.0 - lam, lam, 1.0 - lam
    rows, _ = _lib.check_mixes((a, 0), N)
    assert rows["w_self"][0] == np.float32(lam) and rows["w_partner"][0] == np.float32(1.0 - lam)
    assert rows["lw_partner"][0] == np.float32(1.0 - lam)
    again, _ = _lib.check_mixes((rows, 0), N, (8, 8))  # records pass through as they are
    assert again is rows or np.array_equal(again, rows)
    assert _lib.check_mixes((torch.from_numpy(_good()), NC), N)[0].dtype == _lib.mix_dtype()


def _edit(col, value, row=0):
    a = _good()
    a[row, col] = value
    return a


BAD = [
    ((_edit(0, N), NC), "partner is outside 0..3"),
    ((_edit(0, -1), NC), "partner is outside 0..3"),
    ((_edit(0, 0.5), NC), "must be integers"),
    ((_edit(5, np.nan), NC), "must be integers"),
    ((_edit(1, np.nan), NC), "w_self must be finite"),
    ((_edit(2, np.inf), NC), "w_partner must be finite"),
    ((_edit(2, 1e39), NC), "w_partner must be finite"),  # not finite as float32
    ((_edit(7, -np.inf), NC), "lw_self must be finite"),
    ((_edit(8, np.nan), NC), "lw_partner must be finite"),
    ((_edit(3, -1), NC), "a box needs top >= 0"),
    ((_edit(4, -1), NC), "a box needs top >= 0"),
    ((_edit(5, -3), NC), "a box needs top >= 0"),
    ((_edit(6, 0), NC), "a box needs top >= 0"),
    ((_edit(5, 8), NC), "leaves the 8 x 8 output image"),
    ((_edit(6, 7), NC), "leaves the 8 x 8 output image"),
    ((_good(), -1), "num_classes must be an integer in 0..1048576"),
    ((_good(), (1 << 20) + 1), "num_classes must be an integer"),
    ((_good(), 2.0), "num_classes must be an integer"),
    ((_good(), True), "num_classes must be an integer"),
    ((_good()[:3], NC), "mix for 3 rows, the batch has 4"),
    ((_good()[:, :8], NC), r"shape \[n, 9\]"),
    ((np.zeros(3, _lib.mix_dtype()), NC), r"shape \[4\] \(records\)"),
    (_good(), "a pair"),
    ((_good(), NC, 1), "a pair"),
]


@pytest.mark.parametrize("row", range(len(BAD)))
def test_check_mixes_refuses_by_message(row):
    mix, msg = BAD[row]
    with pytest.raises(ValueError, match=msg):
        _lib.check_mixes(mix, N, (8, 8))


def test_check_mixes_other_refusals():
    with pytest.raises(TypeError, match="must hold numbers"):
        _lib.check_mixes((np.array([["a"] * 9] * N), NC), N)
    with pytest.raises(ValueError, match="size list"):
        _lib.check_mixes((_good(), NC), N, _lib.check_view_sizes([(8, 8), (4, 4)]))
    assert _lib.check_mixes((_edit(5, 8), NC), N)[1] == NC  # without a size the decode call checks the box
    _lib.check_mix_labels(np.arange(NC), NC)
    _lib.check_mix_labels(np.array([99]), 0)  # images only: any label
    with pytest.raises(ValueError, match="row 2 has label 10, outside 0..9"):
        _lib.check_mix_labels(np.array([0, 9, 10, -1]), NC)
    with pytest.raises(ValueError, match="row 0 has label -1"):
        _lib.check_mix_labels(np.array([-1]), NC)


# ---- the samplers against torchvision's draws -----------------------------------------------------

def _tv_lam(alpha, g):
    return float(torch._sample_dirichlet(torch.tensor([[alpha, alpha]]), generator=g)[..., 0])


def _tv_mixup(alpha, g, H, W):
    lam = _tv_lam(alpha, g)
    return (np.float32(lam), np.float32(1.0 - lam), (0, 0, 0, 0), np.float32(lam), np.float32(1.0 - lam))


def _tv_cutmix(alpha, g, H, W):
    lam = _tv_lam(alpha, g)
    r_x = int(torch.randint(W, (1,), generator=g))
    r_y = int(torch.randint(H, (1,), generator=g))
    r = 0.5 * math.sqrt(1.0 - lam)
    r_w_half, r_h_half = int(r * W), int(r * H)
    x1, y1 = max(r_x - r_w_half, 0), max(r_y - r_h_half, 0)
    x2, y2 = min(r_x + r_w_half, W), min(r_y + r_h_half, H)
    lam_adj = float(1.0 - (x2 - x1) * (y2 - y1) / (W * H))
    box = (y1, x1, y2 - y1, x2 - x1) if (y2 - y1) > 0 and (x2 - x1) > 0 else (0, 0, 0, 0)
    return (np.float32(1.0), np.float32(0.0), box, np.float32(lam_adj), np.float32(1.0 - lam_adj))


def _tv_choice(p, g, H, W):
    idx = int(torch.multinomial(torch.tensor([q / sum(p) for q in p]), 1, generator=g))
    return _tv_mixup(0.2, g, H, W) if idx == 0 else _tv_cutmix(1.0, g, H, W)  # the chosen one's draws only


def _assert_rows(got, want, n, what):
    rows, nc = got
    assert nc == NC and rows.dtype == _lib.mix_dtype() and rows.shape == (n,), what
    assert rows["partner"].tolist() == [(i - 1) % n for i in range(n)], what
    for i in range(n):
        r = rows[i]
        assert (r["w_self"], r["w_partner"], tuple(r["box"].tolist()), r["lw_self"], r["lw_partner"]) == want, (what, i)
    assert _lib.check_mixes(got, n, None)[0] is not None


@pytest.mark.parametrize("size", [(1, 1), (7, 9), (224, 224)])
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_samplers_follow_torchvisions_draw_order(size, seed):
    H, W = size
    makers = {
        "mixup": (lambda g: ldt_amd.MixUp(0.2, num_classes=NC, generator=g), lambda g: _tv_mixup(0.2, g, H, W)),
        "cutmix": (lambda g: ldt_amd.CutMix(1.0, num_classes=NC, generator=g), lambda g: _tv_cutmix(1.0, g, H, W)),
        "choice": (lambda g: ldt_amd.MixChoice([ldt_amd.MixUp(0.2, num_classes=NC),
                                                ldt_amd.CutMix(1.0, num_classes=NC)], generator=g),
                   lambda g: _tv_choice([1.0, 1.0], g, H, W)),
        "choice_p": (lambda g: ldt_amd.MixChoice([ldt_amd.MixUp(0.2, num_classes=NC),
                                                  ldt_amd.CutMix(1.0, num_classes=NC)], p=[1, 3], generator=g),
                     lambda g: _tv_choice([1.0, 3.0], g, H, W)),
    }
    for name, (make, tv) in makers.items():
        # with a generator: three batches in a row from one stream of draws
        g, t = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
        s = make(g)
        for k in range(3):
            _assert_rows(s.sample(5, size), tv(t), 5, (name, "generator", k))
        # with the global RNG
        s = make(None)
        torch.manual_seed(seed)
        got = [s.sample(3, size) for _ in range(2)]
        torch.manual_seed(seed)
        for k in range(2):
            _assert_rows(got[k], tv(None), 3, (name, "global", k))


def test_mixup_lam_is_the_beta_distributions_draw():
    for alpha in (0.2, 0.8, 1.0):
        torch.manual_seed(7)
        want = float(torch.distributions.Beta(torch.tensor([alpha]), torch.tensor([alpha])).sample(()))
        torch.manual_seed(7)
        rows, _ = ldt_amd.MixUp(alpha, num_classes=NC).sample(2, (8, 8))
        assert rows["w_self"][0] == np.float32(want) and rows["lw_partner"][1] == np.float32(1.0 - want)


def test_sampler_arguments_and_pickle():
    for bad in (0, -1.0, float("nan"), "1", True):
        with pytest.raises(ValueError, match="alpha"):
            ldt_amd.MixUp(bad, num_classes=NC)
    with pytest.raises(ValueError, match="num_classes"):
        ldt_amd.CutMix(1.0)
    with pytest.raises(ValueError, match="num_classes"):
        ldt_amd.CutMix(1.0, num_classes=-1)
    with pytest.raises(ValueError, match="disagree on num_classes"):
        ldt_amd.MixChoice([ldt_amd.MixUp(num_classes=10), ldt_amd.CutMix(num_classes=11)])
    with pytest.raises(ValueError, match="p must hold"):
        ldt_amd.MixChoice([ldt_amd.MixUp(num_classes=10)], p=[1, 2])
    with pytest.raises(ValueError, match="non-empty list"):
        ldt_amd.MixChoice([])
    for s in (ldt_amd.MixUp(0.2, num_classes=NC), ldt_amd.CutMix(num_classes=NC),
              ldt_amd.MixChoice([ldt_amd.MixUp(0.2, num_classes=NC), ldt_amd.CutMix(num_classes=NC)], p=[1, 2])):
        back = pickle.loads(pickle.dumps(s))
        assert type(back) is type(s) and repr(back) == repr(s) and back.num_classes == NC
        torch.manual_seed(3)
        a = s.sample(3, (7, 9))
        torch.manual_seed(3)
        b = back.sample(3, (7, 9))
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]


# ---- the spec on every surface --------------------------------------------------------------------

def _same_mix(a, b):
    if hasattr(a, "sample"):
        return type(a) is type(b) and pickle.dumps(a) == pickle.dumps(b)
    return type(a) is type(b) is tuple and a[1] == b[1] and a[0].dtype == b[0].dtype and np.array_equal(a[0], b[0])


@pytest.mark.parametrize("mix", [ldt_amd.MixChoice([ldt_amd.MixUp(0.2, num_classes=NC),
                                                    ldt_amd.CutMix(num_classes=NC)]), (_good(), NC)],
                         ids=["sampler", "pair"])
def test_every_surface_carries_an_equal_picklable_mix(mix, monkeypatch):
    opts = dict(mix=mix, size=(8, 8), augment=ldt_amd.TrivialAugmentWide(erase=ldt_amd.RandomErasing()))
    monkeypatch.setattr(T, "_in_worker", lambda: True)
    want = T.CallSpec.make(**opts).check_arrays(N)
    assert T.CallSpec.__slots__[-1] == "mix"
    if not hasattr(mix, "sample"):
        assert want.mix[0].dtype == _lib.mix_dtype()  # checked for the batch: travels as records
    holders = {
        "DeviceBatch": T.DeviceBatch(T._pack_list(CELLS, list(range(N))), **opts),
        "make_collate_fn": T.make_collate_fn(**opts),
        "collate_fn": T.collate_fn(_items(), **opts),
        "decode_tensor_image": T.decode_tensor_image(_rb(), **opts),
        "make_collate_fn()()": T.make_collate_fn(**opts)(_items()),
    }
    for what, h in holders.items():
        spec = h._spec if what != "make_collate_fn" else h._spec.check_arrays(N)
        assert _same_mix(spec.mix, want.mix), what
        assert _same_mix(pickle.loads(pickle.dumps(h))._spec.check_arrays(N).mix, want.mix), what + " through pickle"
    assert _same_mix(holders["DeviceBatch"]._mix, want.mix)
    pipe = object.__new__(T.DecodePipeline)
    pipe._spec = T.CallSpec.make(size=(8, 8), mix=mix)
    assert pipe._spec.mix is mix and pipe._spec.override(interpolation="bicubic").mix is mix
    other = (_good(), 3)
    assert pipe._spec.override(mixes=other).mix is other


def test_the_mix_is_drawn_last():
    log = []

    class Rec:
        def __init__(self, name, value, **attrs):
            self.name, self.value = name, value
            self.__dict__.update(attrs)

        def sample(self, *a, **k):
            log.append(self.name)
            return self.value

    wh, status = np.full((N, 2), 50, np.int32), np.zeros(N, np.int32)
    crops = np.tile(np.array([0, 0, 9, 9, 0], np.int32), (N, 1))
    windows = np.tile(np.array([8, 8, 0, 0], np.int32), (N, 1))
    augs = _lib.check_augments(None, N, None, (8, 8), np.zeros((N, 4), np.int64))
    spec = T.CallSpec.make(size=(8, 8), crop=Rec("crop", crops), window=Rec("window", windows),
                           augment=Rec("augment", augs), mix=Rec("mix", (_good(), NC), num_classes=NC))
    got = spec.resolve(sizes=(wh, status), n=N)
    assert log == ["crop", "window", "augment", "mix"] and len(got) == 5
    assert got[4][0].dtype == _lib.mix_dtype() and got[4][1] == NC
    assert T.CallSpec.make(size=(8, 8)).resolve(sizes=(wh, status), n=N)[4] is None
    with pytest.raises(ValueError, match="leaves the 8 x 8"):
        T.CallSpec.make(size=(8, 8), mix=(_edit(5, 8), NC)).resolve(sizes=(wh, status), n=N)


# ---- arm ------------------------------------------------------------------------------------------

class _FakeLib:
    def __init__(self, refuse=None):
        self.calls, self.refuse = [], refuse

    def __getattr__(self, name):
        if not name.startswith("ldt_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name,) + args)
            if name == "ldt_last_error":
                return b"refused by the fake"
            return -1 if name == self.refuse else 0

        return fn


def _fake_context(refuse=None):
    import threading

    ctx = object.__new__(_lib.Context)
    ctx.lib, ctx.handle, ctx.device, ctx.lock = _FakeLib(refuse), 1234, 0, threading.Lock()
    ctx._size, ctx._filter, ctx._format = _lib.DEFAULT_SIZE, _lib.DEFAULT_INTERPOLATION, \
        (_lib.DEFAULT_DTYPE, _lib.DEFAULT_MEMORY_FORMAT)
    return ctx


def test_arm_makes_no_mix_call_for_none_and_disarms_it_with_the_others():
    ctx = _fake_context()
    ctx.arm((224, 224), "bilinear", "float32", "contiguous", mixes=None)
    assert ctx.lib.calls == []
    rows, nc = _lib.check_mixes((_good(), NC), N)
    ctx.arm((224, 224), "bilinear", "float32", "contiguous", mixes=(rows, nc, 0xBEEF))
    assert ctx.lib.calls == [("ldt_set_mix", 1234, rows.ctypes.data, N, NC, 0xBEEF)]
    # refused: everything pending is cleared, the mix too
    for refuse in ("ldt_set_mix", "ldt_set_augments"):
        ctx = _fake_context(refuse)
        augs = _lib.check_augments(None, N, None, (224, 224), np.zeros((N, 4), np.int64))
        with pytest.raises(_lib.LdtError, match="rc=-1"):
            ctx.arm((224, 224), "bilinear", "float32", "contiguous", augments=augs, mixes=(rows, nc, 0xBEEF))
        at = [c[0] for c in ctx.lib.calls].index(refuse)
        assert ("ldt_set_mix", 1234, None, 0, 0, None) in ctx.lib.calls[at + 1:]
        assert ("ldt_set_augments", 1234, None, 0) in ctx.lib.calls[at + 1:]
    assert "ldt_set_mix" in _lib.EXPORTED


# ---- ValueErrors on every surface ------------------------------------------------------------------

def _surfaces():
    rbatch = object.__new__(T.ResidentBatch)
    rbatch.n = N
    packed = T._pack_list(CELLS, list(range(N)))
    plural = {"crop": "crops", "window": "windows", "mix": "mixes"}

    def renamed(k):
        return {plural.get(name, name): v for name, v in k.items()}

    return {
        "decode_arrow": lambda **k: T.decode_arrow(pa.array(CELLS, pa.binary()), **renamed(k)),
        "decode_tensor_image": lambda **k: T.decode_tensor_image(_rb(), **k),
        "collate_fn": lambda **k: T.collate_fn(_items(), **k),
        "DeviceBatch": lambda **k: T.DeviceBatch(packed, **k),
        "ResidentBatch.decode": lambda **k: rbatch.decode(**renamed(k)),
        "make_collate_fn": lambda **k: T.make_collate_fn(**k),
        "DecodePipeline": lambda **k: T.DecodePipeline(**k),
        "make_to_tensor_fn": lambda **k: T.make_to_tensor_fn(**k),
    }


def test_a_mix_with_views_a_size_list_or_uint8_is_refused_on_every_surface():
    mix = ldt_amd.MixUp(0.2, num_classes=NC)
    for name, call in _surfaces().items():
        with pytest.raises(ValueError, match="mix= with views="):
            call(mix=mix, views=2)
        with pytest.raises(ValueError, match="mix= with views="):
            call(mix=mix, size=[(8, 8), (4, 4)])
        if name != "decode_arrow":  # its callers hand it arrays
            with pytest.raises(ValueError, match="mix= with views="):
                call(mix=mix, window=ldt_amd.ResizeFiveCrop(16), size=(8, 8))
        with pytest.raises(ValueError, match="mix= with dtype=torch.uint8"):
            call(mix=mix, dtype=torch.uint8)
        with pytest.raises(ValueError, match="a pair"):
            call(mix=_good())
    with pytest.raises(TypeError):
        T.resize_raw(np.zeros((1, 2, 2, 3), np.uint8), 2, 2, mix=mix)
    with pytest.raises(TypeError):
        T.resize_raw(np.zeros((1, 2, 2, 3), np.uint8), 2, 2, mixes=(_good(), NC))
    pipe = object.__new__(T.DecodePipeline)
    pipe._spec = T.CallSpec.make(views=2)
    with pytest.raises(ValueError, match="mix= with views="):
        pipe.decode(_rb(), mixes=mix)


def test_labels_outside_the_classes_are_refused_on_the_host(monkeypatch):
    monkeypatch.setattr(T, "_decoder", lambda device: 1 / 0)  # no device is asked for before the refusal
    mix = (_good(), 3)  # labels 0..3: row 3 is outside 0..2
    with pytest.raises(ValueError, match="row 3 has label 3, outside 0..2"):
        T.decode_tensor_image(_rb(), mix=mix)
    with pytest.raises(ValueError, match="row 3 has label 3, outside 0..2"):
        T.collate_fn(_items(), mix=mix)
    with pytest.raises(ValueError, match="row 3 has label 3, outside 0..2"):
        T.decode_arrow(pa.array(CELLS, pa.binary()), list(range(N)), mixes=mix)
    rbatch = object.__new__(T.ResidentBatch)
    rbatch.n, rbatch.labels, rbatch._sizes = N, np.arange(N, dtype=np.int64), None
    with pytest.raises(ValueError, match="row 3 has label 3, outside 0..2"):
        rbatch.decode(mixes=mix)
