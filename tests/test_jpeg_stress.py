"""The stress cells of tests/jpeg_recode.py, on the CPU: the re-coder is
lossless, the oracle agrees with Pillow on every cell, and every cell really
has the property it is there for (recomputed from its bytes). The GPU side is
tests/test_gpu_jpeg_stress.py; the device tables of the same cells are checked
on the host by tests/test_plan_fuzz.py.

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
