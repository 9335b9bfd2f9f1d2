"""GPU tests of the output-size parameter: every decode / resize entry point
at sizes other than 224 x 224, bit for bit against the oracle
(oracle.jpeg_to_tensor(data, oh, ow) / raw_to_tensor, which
tests/test_output_size.py pins to Pillow on the CPU); max abs <= 2/255 is
asserted first, as elsewhere.

One rule decides what a cell's expected result is at a size: a source that the
size reduces by more than 37 on an axis (ceil(W / out_w) or ceil(H / out_h):
the resize kernels' 75-tap bound, include/ldt.h LDT_IMG_TOO_LARGE) fails on
its own row with status 4, an all-zero image and label -100, and every other
cell of the batch is exact. At the small sizes of OUT ((1,1), (2,3), (7,5))
that is what the larger cells of the mixed batch must do; `_expected` applies
the rule, nothing is left out.
"""
import numpy as np
import pyarrow as pa
import pytest

import jpeg_recode as jr
from conftest import read_golden
from oracle import oracle

pytestmark = pytest.mark.gpu

TOL = 2.0 / 255.0
OUT = [(1, 1), (2, 3), (7, 5), (16, 16), (30, 33), (63, 65), (64, 64), (96, 128), (128, 96), (225, 223),
       (255, 257), (256, 256), (299, 299), (384, 384), (513, 100), (100, 513), (1024, 1024)]
ALONE = [(30, 33), (255, 257), (299, 299)]
PATHS = [(160, 160), (255, 257), (299, 299)]
SENTINEL = -12345.5
_ID = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


def _check(got, exp, what):
    diff = np.abs(got.astype(np.float64) - exp.astype(np.float64))
    assert diff.max() <= TOL, f"{what}: max abs {diff.max()} > 2/255 (mean {diff.mean()})"
    assert np.array_equal(got, exp), f"{what}: not bit-exact (max abs {diff.max()}, {np.count_nonzero(diff)} differ)"


@pytest.fixture(scope="module")
def mixed():
    """The mixed batch: (name, data) in a fixed order."""
    from ldt_amd import synth

    l440 = next(c for c in jr.layout_cells() if c.name == "440-17x5")
    return [
        ("420-48x64", synth.encode(synth.field(48, 64, 201, 6.0))),
        ("420-375x500", synth.encode(synth.field(375, 500, 202, 6.0), quality=90, restart_marker_rows=1)),
        ("420-512x512", synth.encode(synth.field(512, 512, 203, 6.0), quality=90)),
        ("444-100x150", synth.encode(synth.field(100, 150, 204, 6.0), subsampling="4:4:4")),
        ("gray-77x91", read_golden("jpeg/gray_77x91.jpg")),
        ("prog-64x80", read_golden("jpeg/prog_64x80.jpg")),
        ("440-17x5", l440.data),
        ("up-8x8", synth.encode(synth.field(8, 8, 205, 6.0), subsampling="4:4:4")),
    ]


_exp_cache = {}


def _expected(name, data, size, normalize=None):
    """The oracle's tensor, or None where the size reduces the source by more
    than 37 on an axis (the row must fail with LDT_IMG_TOO_LARGE)."""
    key = (name, size, bool(normalize))
    if key not in _exp_cache:
        w, h, _ = oracle.jpeg_info(data)
        if -(-w // size[1]) > 37 or -(-h // size[0]) > 37:
            _exp_cache[key] = None
        else:
            _exp_cache[key] = oracle.jpeg_to_tensor(data, size[0], size[1], normalize=normalize)
    return _exp_cache[key]


def _band_kernel_serves(cells, size):
    """Whether the default implementation runs the one-wave-per-band kernel
    for this batch: out_w <= 256 and no decodable source wider than 5 x out_w
    (11 horizontal taps); otherwise the streaming kernel."""
    ws = [oracle.jpeg_info(d)[0] for name, d in cells if _expected(name, d, size) is not None]
    return size[1] <= 256 and bool(ws) and max(-(-w // size[1]) for w in ws) <= 5


def _ctx():
    import torch

    from ldt_amd import _lib

    return _lib.get_context(torch.cuda.current_device()), _lib


def _decode_guarded(cells, size, guard=4096, normalize=None, **kw):
    """decode_arrow into the middle of a larger buffer full of a sentinel.
    Returns (images, labels, {failed row: status}); asserts the guards are
    untouched."""
    import torch

    import ldt_amd
    from ldt_amd import transforms as T

    n, (h, w) = len(cells), size
    cell = 3 * h * w
    flat = torch.full((guard + n * cell + guard,), SENTINEL, dtype=torch.float32, device="cuda")
    lflat = torch.full((n + 2,), -777, dtype=torch.int64, device="cuda")
    out = flat[guard:guard + n * cell].view(n, 3, h, w)
    labels = np.arange(100, 100 + n, dtype=np.int64)
    failed = {}
    try:
        T.decode_arrow(pa.array([d for _, d in cells], pa.binary()), labels, out=out, out_lbl=lflat[1:n + 1],
                       size=size, normalize=normalize, **kw)
    except ldt_amd.ImageDecodeError as e:
        failed = dict(e.rows)
    torch.cuda.synchronize()
    assert torch.all(flat[:guard] == SENTINEL).item(), f"{size}: wrote before the output"
    assert torch.all(flat[guard + n * cell:] == SENTINEL).item(), f"{size}: wrote past the output"
    assert int(lflat[0]) == -777 and int(lflat[n + 1]) == -777
    return out.cpu().numpy(), lflat[1:n + 1].cpu().numpy(), failed


def _check_batch(cells, size, img, lbl, failed, what, normalize=None, extra_failed=()):
    want_failed = {}
    for k, (name, data) in enumerate(cells):
        exp = None if k in extra_failed else _expected(name, data, size, normalize)
        if exp is None:
            want_failed[k] = extra_failed[k] if k in extra_failed else 4
            assert not img[k].any(), f"{what}: failed row {k} ({name}) is not all zero"
            assert img[k].shape == (3,) + tuple(size)
            assert lbl[k] == -100, f"{what}: failed row {k} label {lbl[k]}"
        else:
            _check(img[k], exp, f"{what}: {name} -> {size}")
            assert lbl[k] == 100 + k
    assert failed == want_failed, f"{what}: failed rows {failed}, expected {want_failed}"


# ---- parity over OUT, no write outside the output --------------------------------

@pytest.mark.parametrize("impl", [0, 2], ids=["band", "streaming"])
@pytest.mark.parametrize("size", OUT, ids=_ID)
def test_mixed_batch_parity_and_guards(mixed, size, impl):
    """The mixed batch at every size of OUT, decoded into the middle of a
    sentinel-filled buffer, through the default implementation and through
    the streaming kernel; then with one truncated cell in the batch: that row
    zeros [3, h, w] and label -100, neighbours exact, guards untouched. The
    band kernel takes a batch only while no source is wider than 5 x out_w, so
    at the narrow sizes the cells narrow enough are decoded again as a batch
    of their own (with a truncated cell that is narrow enough too), which that
    kernel must take."""
    ctx, _lib = _ctx()
    bad = ("truncated", read_golden("jpeg/bad_truncated.bin"))

    # a cell no wider than 64 px that ends halfway through its entropy-coded data
    d48 = mixed[0][1]
    sos = d48.rfind(b"\xff\xda")
    small_bad = ("truncated-48x64", d48[:sos + (len(d48) - sos) // 2])

    def with_bad(cells, what, bad=bad):
        cells = cells[:1] + [bad] + cells[1:]
        img, lbl, failed = _decode_guarded(cells, size)
        # truncated entropy data (3), unless the size already refuses its header's dimensions (4)
        bw, bh, _ = oracle.jpeg_info(bad[1])
        too_large = -(-bw // size[1]) > 37 or -(-bh // size[0]) > 37
        assert failed.get(1) == (4 if too_large else 3), failed
        _check_batch(cells, size, img, lbl, failed, what, extra_failed={1: failed[1]})
        return cells

    ctx.set_option(_lib.OPT_RESIZE_IMPL, impl)
    try:
        img, lbl, failed = _decode_guarded(mixed, size)
        _check_batch(mixed, size, img, lbl, failed, f"impl {impl}")
        took = ctx.lib.ldt_debug_last_resize(ctx.handle)
        assert (took > 0) == (impl == 0 and _band_kernel_serves(mixed, size)), f"{size} impl {impl}: path {took}"
        with_bad(mixed, f"impl {impl}, truncated cell")
        narrow = [(n, d) for n, d in mixed
                  if _expected(n, d, size) is not None and -(-oracle.jpeg_info(d)[0] // size[1]) <= 5]
        if impl == 0 and size[1] <= 256 and narrow and len(narrow) < len(mixed):
            # with a truncated cell that does not widen the batch, where one of the two is that narrow
            fits = [b for b in (bad, small_bad) if -(-oracle.jpeg_info(b[1])[0] // size[1]) <= 5]
            if fits:
                with_bad(narrow, "narrow cells, truncated cell", fits[0])
            else:
                img, lbl, failed = _decode_guarded(narrow, size)
                _check_batch(narrow, size, img, lbl, failed, "narrow cells")
            assert ctx.lib.ldt_debug_last_resize(ctx.handle) > 0, f"{size}: narrow batch off the band kernel"
    finally:
        ctx.set_option(_lib.OPT_RESIZE_IMPL, 0)


def test_unaligned_output_base(mixed):
    """An output that starts 4 bytes off 16-byte alignment, at a width that is
    a multiple of 4 and at one that is not: single-float stores only, guards
    untouched, in the streaming kernel (the mixed batch, with its 512-wide
    sources) and in the band kernel (the cells no wider than 5 x out_w)."""
    ctx, _ = _ctx()
    for size in [(30, 33), (64, 64)]:
        img, lbl, failed = _decode_guarded(mixed, size, guard=4097)
        _check_batch(mixed, size, img, lbl, failed, "guard 4097")
        assert ctx.lib.ldt_debug_last_resize(ctx.handle) == 0
        narrow = [(n, d) for n, d in mixed if -(-oracle.jpeg_info(d)[0] // size[1]) <= 5]
        assert 3 <= len(narrow) < len(mixed)
        img, lbl, failed = _decode_guarded(narrow, size, guard=4097)
        _check_batch(narrow, size, img, lbl, failed, "guard 4097, narrow cells")
        assert ctx.lib.ldt_debug_last_resize(ctx.handle) > 0


@pytest.mark.parametrize("size", ALONE, ids=_ID)
def test_each_cell_alone(mixed, size):
    import ldt_amd

    for name, data in mixed:
        rb = pa.RecordBatch.from_arrays([pa.array([data], pa.binary()), pa.array([5], pa.int64())],
                                        names=["image", "label"])
        out = ldt_amd.decode_tensor_image(rb, size=size)
        assert tuple(out["image"].shape) == (1, 3) + size and int(out["label"][0]) == 5
        _check(out["image"][0].cpu().numpy(), _expected(name, data, size), f"alone: {name} -> {size}")


def test_normalize_and_collate_at_other_sizes(mixed):
    import ldt_amd

    for size in [(96, 128), (299, 299)]:
        items = [{"image": d, "label": k} for k, (_, d) in enumerate(mixed)]
        out = ldt_amd.collate_fn(items, normalize=True, size=size)
        img = out["image"].cpu().numpy()
        assert out["label"].cpu().tolist() == list(range(len(mixed)))
        for k, (name, data) in enumerate(mixed):
            _check(img[k], _expected(name, data, size, normalize=True), f"collate normalize: {name} -> {size}")


# ---- kernel and option paths ------------------------------------------------------

@pytest.fixture(scope="module")
def path_cells(mixed):
    from ldt_amd import synth

    return mixed + [("tall-1300x200", synth.encode(synth.field(1300, 200, 206, 6.0), quality=85))]


@pytest.mark.parametrize("opt,value", [("RESIZE_IMPL", 1), ("RESIZE_IMPL", 2), ("RESIZE_IMPL", 3),
                                       ("RESIZE_WG_WAVES", 1), ("RESIZE_WG_WAVES", 2), ("RESIZE_WG_WAVES", 4)])
@pytest.mark.parametrize("size", PATHS, ids=_ID)
def test_option_paths(path_cells, size, opt, value):
    """Every resize implementation and workgroup shape, with a 1300-tall image
    (past the vertical table's limit at 224; its coefficients come from the
    table or the kernel depending on the size) in the batch."""
    ctx, _lib = _ctx()
    ctx.set_option(getattr(_lib, "OPT_" + opt), value)
    try:
        img, lbl, failed = _decode_guarded(path_cells, size)
        took = ctx.lib.ldt_debug_last_resize(ctx.handle)
    finally:
        ctx.set_option(getattr(_lib, "OPT_" + opt), 0)
    _check_batch(path_cells, size, img, lbl, failed, f"{opt}={value}")
    band = _band_kernel_serves(path_cells, size) and not (opt == "RESIZE_IMPL" and value == 2)
    assert (took > 0) == band, f"{size} {opt}={value}: resize path {took}"
    if band and opt == "RESIZE_WG_WAVES":
        assert took == value


def test_generic_kernel_at_224_equals_default(manifest):
    """LDT_OPT_RESIZE_IMPL 3 (the generic-width band kernel at 224 x 224) on
    the golden batch: equal to the default run and to the oracle."""
    import ldt_amd
    from ldt_amd import synth

    ents = [e for e in manifest["images"] if e["file"].endswith(".jpg")]
    cells = [read_golden(e["file"]) for e in ents]
    rb = synth.arrow_batch(cells, np.arange(len(cells)))
    ctx, _lib = _ctx()
    base = ldt_amd.decode_tensor_image(rb)["image"].cpu().numpy()
    ctx.set_option(_lib.OPT_RESIZE_IMPL, 3)
    try:
        gen = ldt_amd.decode_tensor_image(rb)["image"].cpu().numpy()
        assert ctx.lib.ldt_debug_last_resize(ctx.handle) > 0
    finally:
        ctx.set_option(_lib.OPT_RESIZE_IMPL, 0)
    assert np.array_equal(gen, base)
    for k, c in enumerate(cells):
        _check(gen[k], oracle.jpeg_to_tensor(c), f"golden {k}")


# ---- size changes on one context --------------------------------------------------

def test_size_changes_without_synchronisation(mixed):
    """224 -> 160 -> (96,128) -> 224 on the shared context with nothing
    waiting between the calls (LDT_OPT_SYNC_STATUS 0): every result exact, and
    ldt_get_output_size reads back what the last call set."""
    import torch

    from ldt_amd import transforms as T

    ctx, _lib = _ctx()
    cells = [c for c in mixed]
    arr = pa.array([d for _, d in cells], pa.binary())
    sizes = [(224, 224), (160, 160), (96, 128), (224, 224), (160, 160)]
    ctx.set_option(_lib.OPT_SYNC_STATUS, 0)
    try:
        outs = []
        for size in sizes:
            outs.append(T.decode_arrow(arr, size=size)[0])
            assert ctx.output_size() == size
        torch.cuda.synchronize()
    finally:
        ctx.set_option(_lib.OPT_SYNC_STATUS, 1)
    for size, out in zip(sizes, outs):
        img = out.cpu().numpy()
        assert img.shape == (len(cells), 3) + size
        for k, (name, data) in enumerate(cells):
            _check(img[k], _expected(name, data, size), f"sequence: {name} -> {size}")
    # None is the default size again
    assert tuple(T.decode_arrow(arr)[0].shape[2:]) == (224, 224) and ctx.output_size() == (224, 224)
    with pytest.raises(_lib.LdtError):
        ctx.check(ctx.lib.ldt_set_output_size(ctx.handle, 0, 5), "ldt_set_output_size")
    with pytest.raises(_lib.LdtError):
        ctx.check(ctx.lib.ldt_set_output_size(ctx.handle, 5, 1025), "ldt_set_output_size")
    assert ctx.output_size() == (224, 224)


def test_pipeline_with_a_size_beside_a_default_one(mixed):
    import ldt_amd

    cells = mixed[:4] + mixed[6:]
    rb = pa.RecordBatch.from_arrays([pa.array([d for _, d in cells], pa.binary()),
                                     pa.array(list(range(len(cells))), pa.int64())], names=["image", "label"])
    sized = ldt_amd.DecodePipeline(depth=3, size=(128, 128))
    plain = ldt_amd.DecodePipeline(depth=2)
    got = []
    for _ in range(4):
        got.append(((128, 128), sized.decode(rb)[0]))
        got.append(((224, 224), plain.decode(rb)[0]))
    sized.check()
    plain.check()
    for size, out in got:
        img = out.cpu().numpy()
        assert img.shape[2:] == size
        for k, (name, data) in enumerate(cells):
            _check(img[k], _expected(name, data, size), f"pipeline: {name} -> {size}")
    res = ldt_amd.ResidentBatch([d for _, d in cells], list(range(len(cells))))
    img, lbl = res.decode(size=(63, 65))
    for k, (name, data) in enumerate(cells):
        _check(img[k].cpu().numpy(), _expected(name, data, (63, 65)), f"resident: {name}")
    assert lbl.cpu().tolist() == list(range(len(cells)))


# ---- raw path -----------------------------------------------------------------------

@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("size", [(64, 64), (299, 299), (513, 100)], ids=_ID)
def test_resize_raw_sizes(size, normalize):
    import torch

    import ldt_amd
    from ldt_amd import synth

    for h, w in [(300, 200), (301, 517)]:
        raw = np.stack([synth.raw_hwc_one(h, w, 31 + k) for k in range(2)])
        out = ldt_amd.resize_raw(torch.from_numpy(raw).cuda(), h, w, normalize=normalize, size=size)
        assert tuple(out.shape) == (2, 3) + size
        img = out.cpu().numpy()
        for k in range(2):
            _check(img[k], oracle.raw_to_tensor(raw[k], size[0], size[1], normalize=normalize or None),
                   f"raw {h}x{w} -> {size} normalize={normalize}")
    # a reduction past 37 is an argument error here
    with pytest.raises(ldt_amd.LdtError):
        ldt_amd.resize_raw(torch.zeros((1, 16, 4000, 3), dtype=torch.uint8), 16, 4000, size=(64, 64))


# ---- loaders --------------------------------------------------------------------------

def _dataset(tmp_path, n, seed):
    import ldt_amd
    from ldt_amd import synth

    cells = [synth.encode(synth.field(96 + 16 * (i % 3), 128 - 8 * (i % 4), seed * 1000 + i, 6.0)) for i in range(n)]
    labels = (np.arange(n) * 7 + seed) % 101
    tbl = pa.table({"image": pa.array(cells, pa.binary()), "label": pa.array(labels, pa.int64())})
    return ldt_amd.write_dataset(tbl, str(tmp_path / f"ds{seed}"), max_rows_per_file=20), cells, labels


def test_stock_dataloader_workers_carry_the_size(tmp_path):
    from torch.utils.data import DataLoader

    import ldt_amd

    ds, cells, labels = _dataset(tmp_path, 40, seed=11)
    size = (128, 96)
    loader = DataLoader(ldt_amd.SafeLanceDataset(ds.uri), batch_size=16, num_workers=2,
                        collate_fn=ldt_amd.make_collate_fn(size=size), multiprocessing_context="spawn")
    seen = 0
    for k, batch in enumerate(loader):
        assert isinstance(batch, ldt_amd.transforms.DeviceBatch)
        rows = list(range(16 * k, min(16 * k + 16, 40)))
        img = batch["image"].cpu().numpy()
        assert img.shape == (len(rows), 3) + size
        assert batch["label"].cpu().tolist() == [int(labels[r]) for r in rows]
        for j, r in enumerate(rows):
            _check(img[j], oracle.jpeg_to_tensor(cells[r], *size), f"worker batch {k} row {r}")
        seen += len(rows)
    assert seen == 40


def test_lance_dataset_with_sized_to_tensor_fn(tmp_path):
    import ldt_amd

    ds, cells, labels = _dataset(tmp_path, 50, seed=12)
    size = (160, 160)
    fn = ldt_amd.make_to_tensor_fn(size=size, prefetch=2)
    lds = ldt_amd.LanceDataset(ds.uri, batch_size=16, to_tensor_fn=fn,
                               sampler=ldt_amd.ShardedBatchSampler(rank=0, world_size=1))
    seen = 0
    for k, batch in enumerate(lds):
        rows = list(range(16 * k, min(16 * k + 16, 50)))
        img = batch["image"].cpu().numpy()
        assert img.shape == (len(rows), 3) + size
        assert batch["label"].cpu().tolist() == [int(labels[r]) for r in rows]
        for j, r in enumerate(rows):
            _check(img[j], oracle.jpeg_to_tensor(cells[r], *size), f"lance batch {k} row {r}")
        seen += len(rows)
    assert seen == 50
    fn.check()


# ---- the reduction limit ---------------------------------------------------------------

def test_reduction_limit_fails_its_own_row(mixed):
    """A 4000-wide, 16-tall source at (64, 64): ceil(4000 / 64) = 63 > 37, so
    that row alone fails with LDT_IMG_TOO_LARGE; at 224 x 224 it decodes."""
    import ldt_amd
    from ldt_amd import synth

    wide = ("wide-16x4000", synth.encode(synth.field(16, 4000, 207, 6.0), quality=85))
    cells = [mixed[0], wide, mixed[3]]
    img, lbl, failed = _decode_guarded(cells, (64, 64))
    assert failed == {1: 4}
    _check_batch(cells, (64, 64), img, lbl, failed, "limit")
    rb = pa.RecordBatch.from_arrays([pa.array([wide[1]], pa.binary()), pa.array([1], pa.int64())],
                                    names=["image", "label"])
    out = ldt_amd.decode_tensor_image(rb)
    _check(out["image"][0].cpu().numpy(), oracle.jpeg_to_tensor(wide[1]), "wide at 224")
