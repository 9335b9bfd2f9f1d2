"""CPU side of the call-sequence matrix: the table of call kinds (tests/call_kinds.py) is well formed, every
``ldt_set_*`` setter of include/ldt.h is armed by some kind, and every kind's reference (Pillow / the oracle, never
the library) can be computed and has the call's shape and dtype. The GPU side is tests/test_gpu_call_sequences.py.
"""
import os
import re
import threading

import numpy as np
import pytest

import call_kinds as ck
from conftest import REPO

# the two setters that are no per-call or sticky output state: the option switchboard (LDT_OPT_*: which kernel or
# copy path a call takes, each with tests of its own) and the stream the host cells' DMA runs on
NOT_CALL_STATE = {"ldt_set_option", "ldt_set_copy_stream"}
NAMES = [k.name for k in ck.KINDS]


def test_the_table_names_every_kind_once():
    assert len(set(NAMES)) == len(NAMES) >= 25
    assert all(k.state for k in ck.KINDS)
    assert [k.name for k in ck.KINDS if not k.asynchronous] == ["refused"]
    assert {k.name for k in ck.KINDS if k.fails is not None} | {"refused"} == set(ck.EXEMPT)


@pytest.mark.parametrize("name", [n for n in NAMES if n not in ck.EXEMPT])
def test_keywords_pass_validation(name):
    from ldt_amd import transforms as T

    kind = ck.BY_NAME[name]
    n = len(kind.data())
    if kind.api == "native":
        plan = T._native_plan(kind.data(), kind.kw.get("crops"), kind.kw.get("drafts"), kind.kw.get("sizes"))
        assert len(plan[0]) == n and len(plan[4]) == n + 1
        return
    spec = T.CallSpec.make(*[kind.kw.get(key) for key in ck.ARROW_KEYS])
    if kind.api == "arrow":
        drawn = spec.check_arrays(n).resolve(kind.data(), n=n)
        for key, got in zip(("crops", "windows", "colors", "augments", "mixes"), drawn):
            assert (got is None) == (kind.kw.get(key) is None), (name, key)
        assert (drawn.drafts is None) == (kind.kw.get("drafts") is None)


class _Recorder:
    """A library whose every function returns LDT_OK and is remembered by name."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            return 0
        return call


def _armed(kind):
    """The ``ldt_set_*`` calls the kind's entry point makes on a fresh context: ``Context.arm`` itself, on a library
    that records, with what ``_decode_tail`` / ``decode_native`` / ``resize_raw`` hand it."""
    from ldt_amd import _lib
    from ldt_amd import transforms as T

    ctx = _lib.Context.__new__(_lib.Context)
    ctx.lib, ctx.handle, ctx.lock = _Recorder(), None, threading.Lock()
    ctx._size, ctx._filter, ctx._format = _lib.DEFAULT_SIZE, _lib.DEFAULT_INTERPOLATION, \
        (_lib.DEFAULT_DTYPE, _lib.DEFAULT_MEMORY_FORMAT)
    kw, n = kind.kw, len(kind.data())
    if kind.api == "native":
        dtype, mf = _lib.check_format("uint8", None, None)
        plan = T._native_plan(kind.data(), kw.get("crops"), kw.get("drafts"), kw.get("sizes"))
        interp = ctx._filter if kw.get("sizes") is None else _lib.check_interpolation(kw.get("interpolation"))
        ctx.arm(ctx._size, interp, dtype, mf, crops=plan[1], drafts=plan[2], native=plan[4],
                native_sizes=plan[5] if len(plan) > 5 else None)
    elif kind.api == "abi":  # what tests/test_gpu_native_sizes.py's _abi_call arms by hand
        sizes, offsets = ck._refused_plan()
        ctx.use_filter("bilinear")
        ctx.use_format("uint8", "contiguous")
        ctx.use_crops(None)
        ctx.use_native(offsets, sizes)
    else:
        spec = T.CallSpec.make(*[kw.get(key) for key in ck.ARROW_KEYS])
        drawn = spec.resolve(kind.data(), n=n)
        mixes = None if drawn[4] is None else (drawn[4][0], drawn[4][1], 1)
        ctx.arm(spec.size, spec.interpolation, spec.dtype, spec.memory_format, drawn[0], drawn[1], spec.views, drawn[2],
                drawn[3], mixes, drawn.drafts, pad=spec.pad)
    return {c for c in ctx.lib.calls if c.startswith("ldt_set_")}


@pytest.mark.parametrize("name", NAMES)
def test_a_kind_arms_the_setters_it_lists(name):
    kind = ck.BY_NAME[name]
    assert _armed(kind) == set(kind.setters), name


def test_every_setter_of_the_header_is_armed_by_some_kind():
    """A new feature's setter fails here until a kind of tests/call_kinds.py arms it."""
    with open(os.path.join(REPO, "include", "ldt.h")) as f:
        declared = set(re.findall(r"\bldt_set_\w+", f.read()))
    assert NOT_CALL_STATE <= declared and "ldt_set_crops" in declared
    armed = set().union(*[k.setters for k in ck.KINDS])
    assert armed <= declared, sorted(armed - declared)
    missing = declared - armed - NOT_CALL_STATE
    assert not missing, f"no call kind arms {sorted(missing)}: add one to tests/call_kinds.py"


_SHAPES = {"plain-224": [(5, 3, 224, 224)], "plain-96x160": [(5, 3, 96, 160)], "plain-299x299": [(5, 3, 299, 299)],
           "views2-crops": [(5, 3, 30, 33)] * 2, "size-list": [(5, 3, 30, 33), (5, 3, 7, 5)],
           "native": [(3, 48, 64), (3, 17, 5), (3, 77, 91), (3, 64, 80), (3, 8, 8)],
           "native-sizes-bicubic": [(3, 30, 33), (3, 7, 5), (3, 33, 40), (3, 16, 257), (3, 9, 9)],
           "native-crops-drafts": [(3, 20, 25), (3, 15, 3), (3, 61, 71), (3, 30, 37), (3, 8, 8)],
           "big-first": [(9, 3, 64, 64)], "bad-progressive": [(2, 3, 30, 33)], "refused": [], "raw": [(3, 3, 30, 33)]}
_DTYPES = {"draft-mixed": np.uint8, "uint8": np.uint8, "bf16-nhwc-normalize": np.int16, "native": np.uint8,
           "native-sizes-bicubic": np.uint8, "native-crops-drafts": np.uint8}


@pytest.mark.parametrize("name", NAMES)
def test_reference_has_the_calls_shape_and_dtype(name):
    kind = ck.BY_NAME[name]
    ref = kind.reference()
    assert [a.shape for a in ref["images"]] == _SHAPES.get(name, [(5, 3, 30, 33)])
    assert all(a.dtype == _DTYPES.get(name, np.float32) for a in ref["images"])
    n = len(kind.data())
    if kind.api in ("arrow", "native"):
        if "soft" in ref:
            assert ref["soft"].shape == (n, 11) and ref["soft"].dtype == np.float32 and "labels" not in ref
            assert np.allclose(ref["soft"].sum(axis=1), 1.0)
        else:
            assert ref["labels"].shape == (n,) and ref["labels"].dtype == np.int64
    if kind.fails is not None:
        assert ref["status"] == kind.fails
        for i in kind.fails:
            assert not ref["images"][0][i].any() and ref["labels"][i] == -100
        assert all(ref["images"][0][i].any() for i in range(n) if i not in kind.fails)
    ck.diff(kind.reference(), ref, name)  # the same bytes every time


def test_diff_names_the_row_and_counts_the_bytes():
    ref = ck.BY_NAME["plain-30x33"].reference()
    bad = dict(ref, images=[ref["images"][0].copy()])
    bad["images"][0][3, 1, 2, 5:7] += 1.0
    with pytest.raises(AssertionError, match=r"a after b: image 0: first differing row 3, \d+ of 59400 bytes differ"):
        ck.diff(bad, ref, "a after b")
    with pytest.raises(AssertionError, match="labels differs"):
        ck.diff(dict(ref, labels=ref["labels"] + 1), ref, "x")


def test_the_progressive_cell_is_cut_inside_its_second_scan():
    whole = ck.cells()[3][0]
    cut = ck._bad_progressive()[0][0]
    first, second = ck._scan_cut(whole, 1), ck._scan_cut(whole, 2)
    assert cut == second and whole.startswith(cut) and len(first) < len(cut) < len(whole)
    assert cut.count(b"\xff\xda") >= 2  # the second scan's header is in; its data ends early
