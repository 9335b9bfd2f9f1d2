"""Host tests of the one record a call's options are gathered in
(``transforms.CallSpec``) and of the one arming point (``Context.arm``): every
decode surface builds an equal spec from the same options, through pickle too;
``resolve`` draws in the order boxes, windows, colours, augments, each sampler
once, and passes arrays through; a call with one bad option raises the same
exception on every surface that takes the option; and ``arm`` leaves nothing
pending in the library when one of its calls is refused. No device.
"""
import pickle

import numpy as np
import pyarrow as pa
import pytest
import torch

import ldt_amd
from ldt_amd import _lib
from ldt_amd import transforms as T

N = 4
CELLS = [b"a", b"bc", b"def", b"g"]
NAN = float("nan")
THREE = [(30, 33), (30, 33), (16, 16)]


def _items():
    return [{"image": c, "label": k} for k, c in enumerate(CELLS)]


def _rb():
    return pa.RecordBatch.from_arrays([pa.array(CELLS, pa.binary()), pa.array(range(N), pa.int64())],
                                      ["image", "label"])


# ---- equal specs on every surface ------------------------------------------------------------------

OPTION_SETS = {
    "defaults": {},
    "format": dict(size=(30, 33), interpolation="bicubic", dtype=torch.float16, memory_format=torch.channels_last),
    "views": dict(views=3, crop=np.tile(np.array([0, 0, 1, 1, 0], np.int32), (N, 3, 1))),
    "size_list": dict(size=THREE),
    "ten_crop": dict(window=ldt_amd.ResizeFiveCrop(40, ten=True), size=(30, 33)),
    "color": dict(color=ldt_amd.ColorJitterParams()),
    "augment": dict(augment=ldt_amd.TrivialAugmentWide(erase=ldt_amd.RandomErasing())),
}


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return type(a) is type(b) and a.dtype == b.dtype and np.array_equal(a, b)
    if hasattr(a, "sample"):  # a sampler: equal when it pickles to the same bytes
        return type(a) is type(b) and pickle.dumps(a) == pickle.dumps(b)
    return type(a) is type(b) and a == b


def _assert_equal_specs(a, b, what):
    assert isinstance(a, T.CallSpec) and isinstance(b, T.CallSpec), what
    for name in T.CallSpec.__slots__:
        assert _same(getattr(a, name), getattr(b, name)), (what, name, getattr(a, name), getattr(b, name))


@pytest.mark.parametrize("name", sorted(OPTION_SETS))
def test_every_surface_holds_an_equal_spec(name, monkeypatch):
    opts = OPTION_SETS[name]
    monkeypatch.setattr(T, "_in_worker", lambda: True)  # collate_fn / decode_tensor_image as in a DataLoader worker
    want = T.CallSpec.make(**opts).check_arrays(N)
    holders = {
        "DeviceBatch": T.DeviceBatch(T._pack_list(CELLS, list(range(N))), **opts),
        "make_collate_fn": T.make_collate_fn(**opts),
        "collate_fn": T.collate_fn(_items(), **opts),
        "decode_tensor_image": T.decode_tensor_image(_rb(), **opts),
        "make_collate_fn()()": T.make_collate_fn(**opts)(_items()),
    }
    for what, h in holders.items():
        assert what == "make_collate_fn" or isinstance(h, T.DeviceBatch), what
        _assert_equal_specs(h._spec, want, what)
        _assert_equal_specs(pickle.loads(pickle.dumps(h))._spec, want, what + " through pickle")
    # the attributes the surfaces always had read the spec
    b, fn = holders["DeviceBatch"], holders["make_collate_fn"]
    assert (b._size, b._views, b._interpolation, b._dtype, b._memory_format) == \
        (want.size, want.views, want.interpolation, want.dtype, want.memory_format) == \
        (fn.size, fn.views, fn.interpolation, fn.dtype, fn.memory_format)
    assert not hasattr(ldt_amd, "CallSpec")  # the surfaces' own: not exported


def test_override_serves_one_batch_and_keeps_the_views():
    spec = T.CallSpec.make(size=(30, 33), views=5, window=ldt_amd.ResizeFiveCrop(40), interpolation="bicubic")
    crops = np.zeros((N, 5, 5), np.int32)
    one = spec.override(crops=crops, interpolation="bilinear", normalize=True)
    assert one.crop is crops and one.interpolation == "bilinear" and one.normalize is True
    assert one.window is spec.window and one.views == 5 and spec.crop is None and spec.interpolation == "bicubic"
    plain = T.CallSpec.make(size=(30, 33))
    with pytest.raises(ValueError, match="the pipeline was built with views=None"):
        plain.override(windows=ldt_amd.ResizeFiveCrop(40))
    with pytest.raises(ValueError, match="uint8.*normalize"):
        T.CallSpec.make(dtype="uint8").override(normalize=True)


# ---- the draw order --------------------------------------------------------------------------------

class _Recorder:
    """A stand-in sampler: appends its name to the shared log and returns a valid array."""

    def __init__(self, name, log, value, **attrs):
        self.name, self.log, self.value = name, log, value
        self.__dict__.update(attrs)

    def sample(self, *a, **k):
        self.log.append(self.name)
        return self.value


def _color_rows():
    return np.tile(np.array([1.2, NAN, NAN, NAN, 228, 0, -1]), (N, 1))


def test_resolve_draws_boxes_windows_colours_augments_each_once():
    log = []
    wh, status = np.full((N, 2), 50, np.int32), np.zeros(N, np.int32)
    crops = np.tile(np.array([0, 0, 9, 9, 0], np.int32), (N, 1))
    windows = np.tile(np.array([30, 33, 0, 0], np.int32), (N, 1))
    augs = _lib.check_augments(None, N, None, (30, 33), np.zeros((N, 4), np.int64))
    spec = T.CallSpec.make(size=(30, 33), crop=_Recorder("crop", log, crops), window=_Recorder("window", log, windows),
                           color=_Recorder("color", log, _color_rows()))
    got = spec.resolve(sizes=(wh, status), n=N)
    assert log == ["crop", "window", "color"]
    assert got[0] is crops and got[1] is windows and got[2].dtype == _lib.color_dtype() and got[3] is None
    del log[:]
    spec = T.CallSpec.make(size=(30, 33), crop=_Recorder("crop", log, crops), window=_Recorder("window", log, windows),
                           augment=_Recorder("augment", log, augs))
    got = spec.resolve(sizes=(wh, status), n=N)
    assert log == ["crop", "window", "augment"] and got[2] is None and got[3].dtype == _lib.aug_dtype()
    # all four stand-ins at once (a spec that make() refuses: colours and augments do not compose): the order
    del log[:]
    spec = spec._replace(color=_Recorder("color", log, _color_rows()))
    with pytest.raises(ValueError, match="do not compose"):
        T.CallSpec.make(color=spec.color, augment=spec.augment)
    got = spec.resolve(sizes=(wh, status), n=N)
    assert log == ["crop", "window", "color", "augment"]
    assert got[0] is crops and got[1] is windows


def test_resolve_takes_the_boxes_of_a_ten_crop_window_and_passes_arrays_through():
    log = []
    wh, status = np.full((N, 2), 50, np.int32), np.zeros(N, np.int32)
    boxes = np.tile(np.array([0, 0, 50, 50, 0], np.int32), (N, 10, 1))
    windows = np.tile(np.array([30, 33, 0, 0], np.int32), (N, 10, 1))
    win = _Recorder("window", log, windows, views=10, ten=True)
    win.boxes = lambda wh_, st_: log.append("boxes") or boxes
    spec = T.CallSpec.make(size=(30, 33), window=win, color=_Recorder("color", log, np.tile(_color_rows()[:, None], (1, 10, 1))))
    assert spec.views == 10
    got = spec.resolve(sizes=(wh, status), n=N)
    assert log == ["boxes", "window", "color"] and got[0] is boxes and got[1] is windows
    # arrays: as they are, nothing drawn, no header walk (the cells here are no JPEGs)
    crops = np.tile(np.array([0, 0, 9, 9, 1], np.int32), (N, 1))
    plain = np.tile(np.array([30, 33, 0, 0], np.int32), (N, 1))
    got = T.CallSpec.make(size=(30, 33), crop=crops, window=plain).resolve(pa.array(CELLS, pa.binary()))
    assert got[0] is crops and got[1] is plain and got[2] is None and got[3] is None
    # a callable for the sizes is called only when a sampler wants them
    assert T.CallSpec.make(crop=crops).resolve(sizes=lambda: 1 / 0, n=N)[0] is crops


# ---- one bad option, every surface -----------------------------------------------------------------

def _surfaces():
    """name -> (call(**options), takes arrays). Options go by the spec's names."""
    rbatch = object.__new__(T.ResidentBatch)
    rbatch.n = N
    packed = T._pack_list(CELLS, list(range(N)))
    plural = {"crop": "crops", "window": "windows", "color": "colors", "augment": "augments"}

    def renamed(k):
        return {plural.get(name, name): v for name, v in k.items()}

    return {
        "decode_arrow": (lambda **k: T.decode_arrow(pa.array(CELLS, pa.binary()), **renamed(k)), True),
        "decode_tensor_image": (lambda **k: T.decode_tensor_image(_rb(), **k), True),
        "collate_fn": (lambda **k: T.collate_fn(_items(), **k), True),
        "DeviceBatch": (lambda **k: T.DeviceBatch(packed, **k), True),
        "ResidentBatch.decode": (lambda **k: rbatch.decode(**renamed(k)), True),
        "make_collate_fn": (lambda **k: T.make_collate_fn(**k), False),
        "DecodePipeline": (lambda **k: T.DecodePipeline(**k), False),
        "make_to_tensor_fn": (lambda **k: T.make_to_tensor_fn(**k), False),
    }


def _resize_raw(**k):
    return T.resize_raw(np.zeros((1, 2, 2, 3), np.uint8), 2, 2, **k)


CROPS_2D = np.tile(np.array([0, 0, 1, 1, 0], np.int32), (N, 1))
# (options, exception, message, surfaces: "all", "arrays" (those given a batch), and whether resize_raw takes them)
BAD = [
    (dict(size=224), (TypeError, ValueError), "pair", "all", True),
    (dict(size=(0, 5)), ValueError, "1..1024", "all", True),
    (dict(size=(2000, 5)), ValueError, "1..1024", "all", True),
    (dict(interpolation="lanczos"), ValueError, "lanczos", "all", True),
    (dict(interpolation=0), ValueError, "NEAREST", "all", True),
    (dict(dtype=torch.float64), ValueError, "float64", "all", True),
    (dict(dtype="fp8"), ValueError, "fp8", "all", True),
    (dict(memory_format=torch.preserve_format), ValueError, "preserve_format", "all", True),
    (dict(memory_format=3), ValueError, "memory_format=3", "all", True),
    (dict(dtype=torch.uint8, normalize=True), ValueError, "uint8.*normalize", "normalize", True),
    (dict(views=0), ValueError, "views", "all", False),
    (dict(views=17), ValueError, "views", "all", False),
    (dict(views=True), ValueError, "views", "all", False),
    (dict(views=1.0), ValueError, "views", "all", False),
    (dict(size=THREE, views=2), ValueError, "views", "all", False),
    (dict(size=[(8, 8), (0, 8)]), ValueError, "1..1024", "all", True),
    (dict(size=THREE, window=ldt_amd.ResizeFiveCrop(16)), ValueError, "one size", "samplers", False),
    (dict(window=ldt_amd.ResizeFiveCrop(64), views=2), ValueError, "views", "samplers", False),
    (dict(window=ldt_amd.ResizeFiveCrop(64, ten=True), crop=ldt_amd.RandomResizedCropFlip()), ValueError,
     "crop= must be None", "samplers", False),
    (dict(size=THREE, crop=CROPS_2D), ValueError, r"\[n, 3, 5\]", "arrays", False),
    (dict(color=_color_rows()[:, :6]), ValueError, "colors must have shape", "arrays", False),
    (dict(color=_color_rows()[:3]), ValueError, "colors for 3 rows", "arrays", False),
    (dict(views=2, color=_color_rows()), ValueError, "colors must have shape", "arrays", False),
    (dict(augment=np.full((N, 5, 10), NAN)), ValueError, "augments must have shape", "arrays", False),
    (dict(augment=np.full((N + 1, 1, 10), NAN)), ValueError, "augments for 5 rows", "arrays", False),
]


@pytest.mark.parametrize("row", range(len(BAD)))
def test_one_bad_option_raises_the_same_on_every_surface(row):
    opts, exc, msg, where, raw = BAD[row]
    for name, (call, arrays) in _surfaces().items():
        if where == "arrays" and not arrays:
            continue  # bound before any batch: an array is checked against each batch
        if where == "samplers" and name == "decode_arrow":
            continue  # decode_arrow's callers hand it arrays
        if where == "normalize" and name == "DecodePipeline":
            continue  # takes no normalize: DecodePipeline.decode does
        with pytest.raises(exc, match=msg):
            call(**opts)
    if raw:  # resize_raw normalizes by default
        with pytest.raises(exc, match=msg):
            _resize_raw(**{k: v for k, v in opts.items() if k != "normalize"})


def test_colours_and_augments_conflict_on_every_surface():
    color, aug = ldt_amd.ColorJitterParams(), ldt_amd.TrivialAugmentWide()
    arrays = dict(color=_color_rows(), augment=np.full((N, 1, 10), NAN))
    for name, (call, takes_arrays) in _surfaces().items():
        with pytest.raises(ValueError, match="do not compose"):
            call(color=color, augment=aug)
        if takes_arrays:
            with pytest.raises(ValueError, match="do not compose"):
                call(**arrays)


def test_a_batchs_own_augments_conflict_with_the_pipelines_color():
    pipe = object.__new__(T.DecodePipeline)
    pipe._spec = T.CallSpec.make(color=ldt_amd.ColorJitterParams())
    with pytest.raises(ValueError, match="do not compose"):
        pipe.decode(_rb(), augments=ldt_amd.TrivialAugmentWide())


def test_two_bad_options_are_reported_in_make_order():
    """size, then the filter, then the format, then the views, then colour + augment: on every surface."""
    color, aug = ldt_amd.ColorJitterParams(), ldt_amd.TrivialAugmentWide()
    for name, (call, _) in _surfaces().items():
        with pytest.raises((TypeError, ValueError), match="pair"):
            call(size=224, color=color, augment=aug)
        with pytest.raises(ValueError, match="lanczos"):
            call(interpolation="lanczos", dtype="fp8")
        with pytest.raises(ValueError, match="fp8"):
            call(dtype="fp8", views=0)
        with pytest.raises(ValueError, match="views"):
            call(views=0, color=color, augment=aug)


# ---- arm: nothing stays pending after a refusal ----------------------------------------------------

class _FakeLib:
    """Records every ldt_set_* call; ldt_set_colors refuses."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("ldt_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name,) + args)
            if name == "ldt_last_error":
                return b"refused by the fake"
            return -1 if name == "ldt_set_colors" else 0

        return fn


def _fake_context():
    import threading

    ctx = object.__new__(_lib.Context)
    ctx.lib, ctx.handle, ctx.device, ctx.lock = _FakeLib(), 1234, 0, threading.Lock()
    ctx._size, ctx._filter, ctx._format = _lib.DEFAULT_SIZE, _lib.DEFAULT_INTERPOLATION, \
        (_lib.DEFAULT_DTYPE, _lib.DEFAULT_MEMORY_FORMAT)
    return ctx


def test_arm_disarms_when_a_call_is_refused():
    ctx = _fake_context()
    crops = _lib.check_crops(np.tile(np.array([0, 0, 1, 1, 0]), (N, 3, 1)), N, 3)
    colors = _lib.check_colors(np.tile(_color_rows()[:, None], (1, 3, 1)), N, 3)
    with pytest.raises(_lib.LdtError, match="rc=-1"):
        ctx.arm(_lib.check_view_sizes(THREE), "bicubic", "float16", "channels_last", crops=crops, colors=colors)
    names = [c[0] for c in ctx.lib.calls]
    refused = names.index("ldt_set_colors")
    assert names[:refused] == ["ldt_set_filter", "ldt_set_output_format", "ldt_set_crops"]
    assert "ldt_set_view_sizes" not in names  # set last, after everything that can be refused: never reached
    after = ctx.lib.calls[refused + 1:]
    assert ("ldt_set_crops", 1234, None, 0) in after and ("ldt_set_views", 1234, 1) in after
    for name in ("ldt_set_windows", "ldt_set_colors", "ldt_set_augments"):
        assert (name, 1234, None, 0) in after


def test_arm_makes_no_call_for_none_and_sets_view_sizes_last():
    ctx = _fake_context()
    ctx.arm((224, 224), "bilinear", "float32", "contiguous")  # the context's settings already: no call at all
    assert ctx.lib.calls == []
    crops = _lib.check_crops(np.tile(np.array([0, 0, 1, 1, 0]), (N, 3, 1)), N, 3)
    ctx.arm(_lib.check_view_sizes(THREE), "bilinear", "float32", "contiguous", crops=crops, views=3)
    assert [c[0] for c in ctx.lib.calls] == ["ldt_set_crops", "ldt_set_views", "ldt_set_view_sizes"]
