"""The stress cells of tests/jpeg_recode.py, on the CPU: the re-coder is
lossless, the oracle agrees with Pillow on every cell, and every cell really
has the property it is there for (recomputed from its bytes). The GPU side is
tests/test_gpu_jpeg_stress.py; the device tables of the same cells are checked
on the host by tests/test_plan_fuzz.py.

The layout cells (every MCU layout the planner accepts) follow: Pillow must
read back from each the frame it is named for, and the oracle must equal
Pillow on it; their GPU side is tests/test_gpu_jpeg_layouts.py.

If a property below fails, change the cell's input image, not the threshold.
"""
import io

import numpy as np
import pytest

import jpeg_recode as jr
from oracle import oracle


def _pil_rgb(b: bytes) -> np.ndarray:
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))


@pytest.fixture(scope="module")
def cells():
    return jr.stress_cells()


def _tagged(cells, tag):
    out = [c for c in cells if tag in c.tags]
    assert out, tag
    return out


def test_recoded_files_decode_to_their_sources_pixels(cells):
    recoded = [c for c in cells if c.source is not None]
    assert len(recoded) >= 5 * 5 + 8 + 2
    for c in recoded:
        assert c.data != c.source
        assert np.array_equal(_pil_rgb(c.data), _pil_rgb(c.source)), c.name
        # the same symbols and extra bits, interval by interval
        assert jr.scan_symbols(c.data) == jr.scan_symbols(c.source), c.name


def test_oracle_equals_pillow_on_every_cell(cells):
    for c in cells:
        assert np.array_equal(oracle.decode_rgb(c.data), _pil_rgb(c.data)), c.name
        assert np.array_equal(oracle.jpeg_to_tensor(c.data), oracle.pil_image_to_tensor(c.data)), c.name


def test_recoder_rejects_tables_libjpeg_rejects():
    ok = ([0, 2] + [0] * 14, [1, 2])
    jr.validate_table(1, *ok)
    bad = {
        "all-ones code": (1, [0, 4] + [0] * 14, [1, 2, 3, 4]),
        "Kraft sum": (1, [3] + [0] * 15, [1, 2, 3]),
        "DC symbol 16": (0, [0, 2] + [0] * 14, [1, 16]),
        "count mismatch": (1, [0, 3] + [0] * 14, [1, 2]),
        "repeated symbol": (1, [0, 2] + [0] * 14, [1, 1]),
    }
    for what, (tc, counts, symbols) in bad.items():
        with pytest.raises(ValueError):
            jr.validate_table(tc, counts, symbols)
        pytest.raises(ValueError, jr.recode, jr.stress_cells()[0].source, lambda t, h: (counts, symbols))
    with pytest.raises(ValueError):  # a symbol of the image without a code
        jr.validate_table(1, *ok, histogram={3: 1})


def _ac(c):
    return [(th, counts) for tc, th, counts, _ in jr.dht_tables(c.data) if tc == 1]


def _dc(c):
    return [(th, counts) for tc, th, counts, _ in jr.dht_tables(c.data) if tc == 0]


def test_long_code_prefix_counts(cells):
    for c in _tagged(cells, "deep") + _tagged(cells, "edge9"):
        for th, counts in _ac(c):
            assert jr.long_prefixes(counts) > 8, (c.name, th)
    for c in _tagged(cells, "deep"):  # the long codes are the hot ones: the file grows
        assert len(c.data) > 1.15 * len(c.source), c.name
    for c in _tagged(cells, "edge8"):
        for th, counts in _ac(c):
            assert jr.long_prefixes(counts) == 8, (c.name, th)
    for c in _tagged(cells, "edge8") + _tagged(cells, "edge9"):
        for th, counts in _ac(c):
            assert jr.l2_widths(counts) == [1, 2, 3, 4, 5], (c.name, th)
        for th, counts in _dc(c):  # 16 codes of 12 bits: all eight chunks, both halves
            assert jr.long_prefixes(counts) == 8 and counts[11] == 16, (c.name, th)
    for c in _tagged(cells, "flat8"):
        for th, counts in _ac(c):
            assert counts[7] == sum(counts), (c.name, th)


def test_split_cells_carry_six_distinct_tables(cells):
    for c in _tagged(cells, "split"):
        tabs = jr.dht_tables(c.data)
        assert len(tabs) == 6 and len({(tc, tuple(counts), tuple(syms)) for tc, th, counts, syms in tabs}) == 6, c.name
        want = {0, 1, 3} if "sof1" in c.tags else {0, 1, 2}
        assert {th for tc, th, _, _ in tabs} == want, c.name
    sof1 = _tagged(cells, "sof1")
    assert all(jr.frame_info(c.data)[0] == 0xC1 for c in sof1)


def test_ones_cells_are_densely_stuffed(cells):
    for c in _tagged(cells, "ones"):
        assert jr.stuffing_share(c.data) >= 1 / 16, (c.name, jr.stuffing_share(c.data))
        assert jr.stuffing_share(c.source) < 0.01, c.name
    # the 16-bit codes of a runs cell start with 11 or more ones: an aligned byte of ones in
    # at least every other symbol (about 2.5 bytes each), and 16 ones in a row wherever the
    # most frequent code, 0xFFFE, follows a 1 bit on a byte boundary
    for c in _tagged(cells, "runs"):
        ecs = jr.scan_bytes(c.data)
        assert jr.stuffing_share(c.data) >= 1 / 8, (c.name, jr.stuffing_share(c.data))
        assert ecs.count(b"\xff\x00\xff\x00") >= len(ecs) // 1024, c.name
    big = _tagged(cells, "big")
    assert all(len(jr.scan_bytes(c.data)) > 2 * 16384 for c in big)  # more than one 16 KB destuff tile


def test_pillow_made_extremes(cells):
    for c in _tagged(cells, "large-symbols"):
        dc, ac = jr.max_sizes(c.data)
        assert ac == 10 and dc >= 10, (c.name, dc, ac)
    for c in _tagged(cells, "pq1"):
        assert jr.frame_info(c.data) == (0xC1, [1, 1]), c.name
    for c in _tagged(cells, "pq1-ac"):  # nonzero AC coefficients under quant values above 255
        assert jr.max_sizes(c.data)[1] >= 3, c.name
    for c in _tagged(cells, "one-symbol"):
        assert sorted(len(syms) for tc, th, counts, syms in jr.dht_tables(c.data))[:2] == [1, 1], c.name
    for c in _tagged(cells, "optimize"):  # not the Annex K tables
        assert all(len(syms) < 100 for tc, th, counts, syms in jr.dht_tables(c.data)), c.name
    for c in _tagged(cells, "q255"):
        q = [p for m, p in jr.parse(c.data)[0] if m == 0xDB]
        assert max(max(p[1:]) for p in q) == 255, c.name
    for c in _tagged(cells, "q1s"):
        q = [p for m, p in jr.parse(c.data)[0] if m == 0xDB]
        assert all(set(p[1:65]) == {1} for p in q), c.name
    ycc = _tagged(cells, "ycc")
    assert len(ycc) == 12
    for c in ycc:  # out of gamut: the RGB samples sit on a clamp (under 1 % of them in a field() image)
        rgb = _pil_rgb(c.data)
        assert ((rgb == 0) | (rgb == 255)).mean() > (0.5 if "corners" in c.name else 0.05), c.name
    assert _tagged(cells, "progressive") and jr.frame_info(_tagged(cells, "progressive")[0].data)[0] == 0xC2


# ---------------------------------------------------------------------------
# the layout cells: every MCU layout the planner accepts (jr.layout_cells)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def layouts():
    return jr.layout_cells()


def _open(b: bytes):
    from PIL import Image

    im = Image.open(io.BytesIO(b))
    im.load()
    return im


def test_reframer_reproduces_its_source():
    """4:4:4 factors at the source's size: the same blocks in the same order,
    so the same symbols (DC differences included) and the same pixels; with a
    restart interval the pixels stay and only the DC differences change."""
    src = jr.layout_source()
    same = jr.reframe(src, ((1, 1),) * 3, 96, 96)
    assert jr.scan_symbols(same) == jr.scan_symbols(src)
    assert np.array_equal(_pil_rgb(same), _pil_rgb(src))
    rst = jr.reframe(src, ((1, 1),) * 3, 96, 96, restart=5)
    assert len(jr.scan_symbols(rst)) == -(-144 // 5) and rst.count(b"\xff\xdd\x00\x04\x00\x05") == 1
    assert np.array_equal(_pil_rgb(rst), _pil_rgb(src))
    # a crop to whole blocks is the source's top-left corner
    assert np.array_equal(_pil_rgb(jr.reframe(src, ((1, 1),) * 3, 40, 56)), _pil_rgb(src)[:40, :56])


def test_layout_cells_are_what_they_claim(layouts):
    """Pillow opens and loads every cell (none is skipped) and reads from it
    exactly the ids, factors, size and mode the cell is named for."""
    names = {c.name for c in layouts}
    for lname, factors in jr.LAYOUTS:
        for h, w in jr.LAYOUT_SIZES:
            assert f"{lname}-{h}x{w}" in names
    assert {(1, 1), (2, 3), (17, 5), (33, 40), (64, 96)} <= set(jr.LAYOUT_SIZES)
    assert sorted({sum(h * v for h, v in f) for _, f in jr.LAYOUTS}) == [4, 5, 6, 7, 8, 9, 10]
    for c in layouts:
        im = _open(c.data)
        assert [tuple(l[:3]) for l in im.layer] == [(i, h, v) for i, (h, v) in zip(c.ids, c.factors)], c.name
        assert im.size == (c.width, c.height) and im.mode == "RGB", c.name
        assert c.height <= 64 and c.width <= 96, c.name
    tagged = lambda t: [c for c in layouts if t in c.tags]
    assert sorted({sum(h * v for h, v in c.factors) for c in tagged("restart")}) == [5, 7, 9, 10]
    for c in tagged("restart"):
        n = 1 if c.name.endswith("rst1") else 3
        assert c.data.count(b"\xff\xdd\x00\x04" + n.to_bytes(2, "big")) == 1, c.name
        assert len(jr._intervals(jr.parse(c.data)[1])) == -(-jr.mcu_counts(c.factors, c.height, c.width)[0] // n) > 1
    assert len(tagged("progressive")) == 2
    for c in tagged("progressive"):
        assert jr.frame_info(c.data)[0] == 0xC2 and c.factors == dict(jr.LAYOUTS)["440"], c.name
    assert len(tagged("colour")) >= 2 * 4 + 1


def test_colour_cells_take_the_colour_space_they_are_named_for(layouts):
    """jdapimin.c default_decompress_parms: Adobe transform 0, or ids 'R','G','B'
    without an APP segment, pass the components through; everything else is YCbCr."""
    by_name = {c.name: c for c in layouts}
    for l in ("420", "440"):
        through = _pil_rgb(by_name[f"{l}-adobe0"].data)
        ycc = _pil_rgb(by_name[f"{l}-adobe1"].data)
        assert not np.array_equal(through, ycc)
        assert np.array_equal(_pil_rgb(by_name[f"{l}-rgb-ids-no-app"].data), through)
        assert np.array_equal(_pil_rgb(by_name[f"{l}-rgb-ids-jfif"].data), ycc)
        assert by_name[f"{l}-adobe0"].rgb and not by_name[f"{l}-adobe1"].rgb
    for name in ("420-adobe2", "420-jfif-adobe0", "420-no-app"):
        assert np.array_equal(_pil_rgb(by_name[name].data), _pil_rgb(by_name["420-adobe1"].data)), name
    keep = by_name["pillow-keep-rgb"]
    assert keep.rgb and b"Adobe" in keep.data and b"JFIF" not in keep.data


def test_relabel_refuses_sizes_where_the_counts_differ():
    from PIL import Image

    from ldt_amd import synth

    assert jr.mcu_counts(((2, 1), (1, 1), (1, 1)), 64, 64) == jr.mcu_counts(dict(jr.LAYOUTS)["440"], 64, 64) == (32, [64, 32, 32])
    assert jr.mcu_counts(((2, 1), (1, 1), (1, 1)), 33, 40) == jr.mcu_counts(dict(jr.LAYOUTS)["440"], 33, 40) == (15, [25, 15, 15])
    p = jr._save(Image.fromarray(synth.field(40, 64, 1, 30.0)), subsampling="4:2:2", progressive=True)
    with pytest.raises(AssertionError):
        jr.relabel_422_as_440(p)


def test_refused_frames_and_the_reference(layouts):
    """The reference decodes 100 % of the accepted cells (asserted above, cell
    by cell) and rejects exactly the 12-block and the fractional frame; the
    subsampled-luma frame it decodes (a pinned divergence: LDT_IMG_UNSUPPORTED)."""
    refused = jr.refused_cells()
    assert [n for n, _, _ in refused] == ["12-blocks", "fractional", "subsampled-luma"]
    rejected = []
    for name, data, pillow_decodes in refused:
        try:
            _open(data)
        except Exception:
            rejected.append(name)
    assert rejected == ["12-blocks", "fractional"]
    assert [n for n, _, ok in refused if ok] == ["subsampled-luma"]


def test_oracle_equals_pillow_on_every_layout_cell(layouts):
    for c in layouts:
        assert np.array_equal(oracle.decode_rgb(c.data), _pil_rgb(c.data)), c.name
        assert np.array_equal(oracle.jpeg_to_tensor(c.data), oracle.pil_image_to_tensor(c.data)), c.name
        assert np.array_equal(oracle.jpeg_to_tensor(c.data, normalize=True),
                              oracle.pil_image_to_tensor(c.data, normalize=True)), c.name
