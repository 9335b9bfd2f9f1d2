"""The script cells of tests/jpeg_progressive.py on the CPU: progressive files
under scan scripts Pillow never writes (band splits, Ah/Al ladders down from
3, per-component DC scans, DHT / DQT / DRI between scans, 64 scans, hostile
Huffman tables), checked four ways:

* the writer: Pillow's decode of every fully refined cell equals, byte for
  byte, Pillow's decode of the baseline file with the same coefficients (the
  same decoder and IDCT: no tolerance), with libjpeg's warnings as errors;
* the oracle: oracle.decode_rgb equals Pillow on every accepted cell;
* the planner (the sanitized host driver of tests/test_plan_fuzz.py): every
  ProgScan equals the script entry that wrote it, refused cells get their
  status on their own row, the latched quantisation tables reach the device
  plan;
* coverage: the paths the cells exist for are reached, asserted from the
  writer's record of what it emitted.

tests/test_gpu_progressive_scripts.py decodes the same cells on the GPU.
"""
import io
import warnings

import numpy as np
import pytest

import jpeg_progressive as jp
import jpeg_recode as jr
from oracle import oracle

# T.81 figure A.6: the natural (row-major) index of each zigzag position
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
          21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
          60, 61, 54, 47, 55, 62, 63]


def _pil(b: bytes, rgb=False):
    """Pillow's decode, with any warning (libjpeg's included) an error."""
    from PIL import Image

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(b))
        im.load()
        return np.asarray(im.convert("RGB") if rgb else im)


@pytest.fixture(scope="module")
def cells():
    return jp.script_cells()


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """The sanitized host planner driver of tests/test_plan_fuzz.py."""
    import test_plan_fuzz

    return test_plan_fuzz.build_planner(tmp_path_factory)


def _plan_batch(planner, data):
    import test_plan_fuzz

    return test_plan_fuzz._plan_batch(planner, data)


def test_cells_cover_the_layouts_and_sizes(cells):
    names = {c.name for c in cells}
    assert len(names) == len(cells) >= 30
    for script in ("deep", "bands"):
        assert {c.factors for c in cells if script in c.tags} >= {f for _, f in jp.LAYOUTS}
    assert {(c.height, c.width) for c in cells} >= set(jp.SIZES)
    assert {c.factors for c in cells if len(c.factors) == 3} == {f for _, f in jp.LAYOUTS}
    assert sum(1 for c in cells if c.height * c.width > 264 * 200) == 1  # eob-max is the only large cell
    for tag in ("spectral-only", "bands", "deep", "shuffled", "sixtyfour", "latch", "restarts", "partial", "tables",
                "gray", "eob-max", "dense"):
        assert any(tag in c.tags for c in cells), tag
    assert {s for c in cells if "tables" in c.tags for s in c.tags} >= set(jp.SHAPES)
    assert jp.script_cells() is cells and jp.script_cells()[0].data == cells[0].data  # deterministic


def test_baseline_writer_and_coefficient_reader_are_pinned_to_pillow():
    """coefs_from_444 and baseline() (the twin of the hand-made cells): a
    Pillow file's coefficients written again decode to the file's pixels, and
    under other factors to what jpeg_recode.reframe gives."""
    src = jr.layout_source()
    S = jp.coefs_from_444(src)
    assert np.array_equal(_pil(jp.baseline(S.coefs, S.qtables, jp.F444, 96, 96, tq=S.tq)), _pil(src))
    for factors, h, w in ((jp.F420, 40, 56), (jp.LAYOUTS[6][1], 33, 40)):
        mine = jp.baseline(S.coefs, S.qtables, factors, h, w, tq=S.tq, restart=3)
        assert np.array_equal(_pil(mine), _pil(jr.reframe(src, factors, h, w))), factors
    G = jp.Source(S.coefs[:1], S.qtables[:1], (0,))
    gray = _pil(jp.baseline(G.coefs, G.qtables, ((1, 1),), 96, 96, tq=(0,)))
    from PIL import Image

    luma = Image.open(io.BytesIO(src))
    luma.draft("L", luma.size)  # libjpeg decodes the Y plane alone
    assert luma.mode == "L" and np.array_equal(gray, np.asarray(luma))


def test_writer_equals_baseline_twin_under_pillow(cells):
    """Every accepted cell: Pillow opens it without a warning and decodes it
    to exactly the pixels of the baseline file with the same coefficients."""
    for c in cells:
        assert c.twin is not None, c.name
        got = _pil(c.data)
        assert got.shape[:2] == (c.height, c.width), c.name
        assert np.array_equal(got, _pil(c.twin)), c.name


def test_partial_twin_holds_what_the_scans_sent(cells):
    """`partial` stops early: its twin (test_writer_equals_baseline_twin_under_pillow)
    is the baseline file of the coefficients as the scans left them (chroma
    10-63 zero, luma 10-63 with bit 0 dropped toward zero), so Pillow applied
    no block smoothing to it; the file itself was written from the whole
    coefficients, which decode to other pixels."""
    c = next(c for c in cells if "partial" in c.tags)
    assert [e[1:5] for e in c.script if e[0] == 0][-1] == (10, 63, 0, 1)
    S = jp.coefs_from_444(jr.layout_source())
    assert not np.array_equal(_pil(c.data), _pil(jr.reframe(jr.layout_source(), c.factors, c.height, c.width)))
    assert any(np.any(np.abs(a[:, :, 10:]) == 1) for a in S.coefs)  # something was dropped


def test_oracle_equals_pillow(cells):
    for c in cells:
        assert np.array_equal(oracle.decode_rgb(c.data), _pil(c.data, rgb=True)), c.name


def test_refused_cells_under_pillow_and_the_oracle():
    """The progression libjpeg calls an error is refused by Pillow and by the
    oracle; the oracle refuses the two files libjpeg would decode differently
    from a plain decode (coefficient 5 unrefined: block smoothing) or that
    carry no DC for a component."""
    refused = {c.name: c for c in jp.refused_script_cells()}
    assert set(refused) == {"cb5-at-al1", "cr-without-dc", "sixtyfive", "ah-not-al-plus-1"}
    for name, c in refused.items():
        if "pillow-refuses" in c.tags:
            with pytest.raises(Exception):
                _pil(c.data)
        if name != "sixtyfive":
            with pytest.raises(oracle.OracleError):
                oracle.decode_rgb(c.data)
    assert len(refused["sixtyfive"].record["scans"]) == 65
    # 65 scans are a limit of the device decoder alone: the file itself is sound
    c = refused["sixtyfive"]
    assert np.array_equal(oracle.decode_rgb(c.data), _pil(c.data, rgb=True))
    assert np.array_equal(_pil(c.data), _pil(jr.reframe(jr.layout_source(), c.factors, c.height, c.width)))


def _mixed(cells):
    """The accepted cells with the refused ones between them: (data, {row: status})."""
    data = [c.data for c in cells]
    at = {}
    for k, c in zip((2, len(cells) // 3, len(cells) // 2 + 1, len(cells) + 2), jp.refused_script_cells()):
        data.insert(k, c.data)
        at[k] = c.status
    return data, at


def test_plan_equals_the_scripts(planner, cells):
    data, at = _mixed(cells)
    assert {v for v in at.values()} == {jp.UNSUPPORTED, jp.CORRUPT} and len(at) == 4
    want = [at.get(i, 0) for i in range(len(data))]
    assert planner(data) == want  # each cell alone
    plan = _plan_batch(planner, data)
    rows = plan["rows"]
    assert [r["status"] for r in rows] == want  # each refused cell on its own row
    ok = [i for i in range(len(data)) if i not in at]
    assert plan["prog_img"] == ok
    assert len(plan["pscans"]) == sum(len(c.record["scans"]) for c in cells)
    off = np.concatenate([[0], np.cumsum([len(d) for d in data])])
    for i, c in zip(ok, cells):
        r, scans = rows[i], c.record["scans"]
        assert (r["width"], r["height"], r["ncomp"]) == (c.width, c.height, len(c.factors)), c.name
        assert r["prog_count"] == len(scans) == sum(1 for e in c.script if e[0] != "DQT"), c.name
        got = plan["pscans"][r["prog_first"]:r["prog_first"] + r["prog_count"]]
        for k, (g, s) in enumerate(zip(got, scans)):
            ns = len(s["comps"])
            assert (g["ns"], tuple(g["comp"][:ns]), g["ss"], g["se"], g["ah"], g["al"], g["restart"]) == \
                   (ns, s["comps"], s["ss"], s["se"], s["ah"], s["al"], s["restart"]), (c.name, k)
            # a Huffman table exactly where the scan decodes symbols
            assert [t >= 0 for t in g["tab"][:ns]] == [s["kind"] != "dc-refine"] * ns, (c.name, k)
            assert off[i] < g["data_off"] and g["data_off"] + g["data_len"] < off[i + 1], (c.name, k)
    assert max(r["prog_count"] for r in rows) == 64


def test_latched_quant_tables_reach_the_plan(planner, cells):
    """The latch cell's device tables: luma's id 0 and the chroma table that
    id 1 held at Cb's first scan, not the table it held at the frame header
    and not the ones written after every component's first scan."""
    c = next(c for c in cells if "latch" in c.tags)
    S = jp.coefs_from_444(jr.layout_source())
    dqt = [e for e in c.script if e[0] == "DQT"]
    assert len(dqt) == 3 and dqt[0][2] == S.qtables[1] and dqt[1][2] == dqt[2][2] != S.qtables[1]
    first = {}
    for k, e in enumerate(c.script):
        if e[0] != "DQT":
            for comp in ((e[0],) if isinstance(e[0], int) else e[0]):
                first.setdefault(comp, k)
    assert first[0] < c.script.index(dqt[0]) < first[1] and max(first.values()) < c.script.index(dqt[1])
    plan = _plan_batch(planner, [cells[0].data, c.data])
    q = np.asarray(plan["qtabs"]).reshape(-1, 64)
    nat = lambda t: [t[ZIGZAG.index(n)] for n in range(64)]
    qt = plan["rows"][1]["qt"]
    assert list(q[qt[0]]) == nat(S.qtables[0])
    assert list(q[qt[1]]) == nat(S.qtables[1]) and list(q[qt[2]]) == nat(S.qtables[1])


def test_coverage(cells):
    """What the cells exist for, from the writer's record. These are
    conditions on the cells: if one fails, the cell has to change."""
    recs = [c.record for c in cells]
    chains = [n for r in recs for k, n in r["chains"].items() if k != "dc"]
    assert any(5 <= n < 60 for n in chains) and any(n >= 60 for n in chains)  # wave reuse in an AC chain
    assert max(r["eob_cat"] for r in recs) == 14
    big = next(c for c in cells if "eob-max" in c.tags).record
    assert [s["eob_cat"] for s in big["scans"] if s["ss"]] == [14, 14]  # AC first and refinement
    assert max(r["corr_stop"] for r in recs) > 32 and max(r["corr_eob"] for r in recs) > 32
    dense = next(c for c in cells if "dense" in c.tags).record
    assert dense["corr_stop"] > 32 and dense["corr_eob"] > 32 and dense["refine_zrl"] >= 1
    scans = [(c, s) for c in cells for s in c.record["scans"]]
    for kind in ("ac-first", "ac-refine", "dc-first"):
        assert any(s["kind"] == kind and s["max_len"] == 16 and s["top_code"] for _, s in scans), kind
    # EOBn symbols (n >= 1) on 16-bit codes, in a first scan and in a refinement
    for kind in ("ac-first", "ac-refine"):
        assert any(s["kind"] == kind and s["eob_len"] == 16 and s["eob_cat"] >= 1 for _, s in scans), kind
    # per-component DC refinement, no restarts, at least one whole 32-block chunk (the 32-bit read)
    assert any(s["kind"] == "dc-refine" and len(s["comps"]) == 1 and s["restart"] == 0 and s["units"] >= 32 and
               len(c.factors) == 3 for c, s in scans)
    # per-component DC scans that leave MCU-padding blocks untouched
    assert any(s["ss"] == 0 and len(s["comps"]) == 1 and len(c.factors) == 3 and
               s["units"] < jr.mcu_counts(c.factors, c.height, c.width)[0] * c.factors[s["comps"][0]][0] *
               c.factors[s["comps"][0]][1] for c, s in scans)
    rst = [s for c in cells if "restarts" in c.tags for s in c.record["scans"]]
    assert {s["restart"] for s in rst} == {0, 1, 3, 7, 33}
    assert any(a["restart"] != 0 and b["restart"] == 0 for a, b in zip(rst, rst[1:]))  # 0 after a non-zero one
    for kind in ("dc-first", "dc-refine", "ac-first", "ac-refine"):
        assert any(s["kind"] == kind and s["restarts"] > 0 for s in rst), kind
    assert any(s["kind"] == "dc-refine" and s["restart"] == 0 for s in rst)
    assert any(s["kind"] == "dc-refine" and s["restarts"] > 0 and len(s["comps"]) == 3 for s in rst)
    assert any(s["restart"] % 32 and s["restarts"] >= 2 and s["units"] > 64 for s in rst)  # not a chunk multiple
    # band edges: Ss == Se, a band that starts at 63, bands that end at 63
    bands = {(s["ss"], s["se"]) for _, s in scans}
    assert {(1, 1), (63, 63), (1, 63), (21, 62)} <= bands
    # refinement ladders from Al = 3, of a sub-band, and over two first scans at different Al
    assert {(3, 2), (2, 1), (1, 0)} <= {(s["ah"], s["al"]) for _, s in scans if s["ss"] == 0}
    assert {(3, 2), (2, 1), (1, 0)} <= {(s["ah"], s["al"]) for _, s in scans if s["ss"]}
    # every Huffman table id, and a scan without a DHT of its own
    assert {t for c, s in scans if "tables" in c.tags and s["kind"].startswith("ac") for t in s["th"]} == {0, 1, 2, 3}
    assert any(len(e) > 5 and e[5].get("dht") is False for c in cells if "tables" in c.tags for e in c.script)
