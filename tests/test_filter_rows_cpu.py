"""The filter probes (tests/filter_rows.py) judged on the CPU, without a device and without the code under test: the
restated constants are the sources', every class has probes on both sides (unless it is defined as passing all or no
rows), every edge the corpus plants is probed, and no wrong predicate of mutants() leaves every probe's expected answer
unchanged: test_filter_rows_gpu.py would notice each of them."""
import os
import re

import numpy as np
import pytest

import filter_rows as fr

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voitta_rag_amd", "csrc")
SIZES = [fr.N_SMALL, fr.N_BIG]


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.fixture(scope="module", params=SIZES)
def case(request):
    n = request.param
    h = fr.corpus(n)
    fr.delete(h, fr.dead_rows(n))
    return h, fr.probe_rows(n), fr.masks(h)


def test_restated_constants_are_the_sources():
    for name, where in (("kPlaneClasses", "filter.hip"), ("kQueryBlock", "engine_internal.h"), ("kFusedMaxK", "engine_internal.h"),
                        ("kMaxK", "engine_internal.h"), ("kInvMaxTerms", "engine_internal.h")):
        m = re.search(r"constexpr int %s = (\d+);" % name, _source(where))
        assert m, (name, where)
        assert int(m.group(1)) == getattr(fr, name), (name, where)
    m = re.search(r"bool prefilter_usable\([^)]*\) \{\s*return [^;]*e->n_rows >= (\d+);", _source("prefilter.hip"))
    assert m and int(m.group(1)) == fr.PREFILTER_MIN_ROWS
    m = re.search(r"nq > kQueryBlock && k <= kFusedMaxK && e->n_rows >= (\d+);", _source("batch.hip"))
    assert m and int(m.group(1)) == fr.BATCH_MIN_ROWS
    m = re.search(r"inv_grouped_fits\([^)]*\) \{\s*return nq >= (\d+) &&", _source("invert.hip"))
    assert m and int(m.group(1)) == fr.GROUPED_MIN_QUERIES
    # the planes: one ballot of a 64-lane wave into two words, grid.y in steps of kPlaneClasses
    planes = _source("filter.hip")
    assert "blockIdx.y * kPlaneClasses" in planes and "(n_cls + kPlaneClasses - 1) / kPlaneClasses" in planes
    with open(os.path.join(CSRC, "..", "..", "include", "voitta_engine.h")) as f:
        assert fr.ABSENT == -(2**63) and "#define VR_TS_ABSENT INT64_MIN" in f.read()
    # kMaxK bounds every k: the hybrid legs ask for 3 x limit
    assert "VR_CHECK(k >= 1 && k <= kMaxK," in _source("search.h") and "limit * 3 <= kMaxK" in _source("search.h")


def test_sizes_and_upserts():
    assert fr.N_SMALL < fr.PREFILTER_MIN_ROWS < fr.BATCH_MIN_ROWS < fr.N_BIG
    assert (fr.N_BIG % 32, fr.N_BIG % 64, fr.N_BIG % 256) == (5, 37, 37)
    for n, ups in fr.UPSERTS.items():
        assert sum(ups) == n > 1024 and len(ups) >= 3  # (the engine starts with room for 1,024 rows: it grows)
    assert len(fr.CLASSES) > 2 * fr.kPlaneClasses  # three grid.y steps
    assert set(fr.CLASS_COUNTS) >= {1, fr.kPlaneClasses - 1, fr.kPlaneClasses, fr.kPlaneClasses + 1, 2 * fr.kPlaneClasses,
                                    2 * fr.kPlaneClasses + 1, len(fr.CLASSES)}


def test_neighbours_differ(case):
    """rows i and i +- 1, 32, 64, 256 never share their whole pass pattern: a bit read one row, one word or one block off
    changes some class's answer wherever it happens"""
    h, _, _ = case
    m = fr.masks(dict(h, live=np.ones(h["n"], bool)))
    for s in (1, 32, 64, 256):
        same = (m[:, s:] == m[:, :-s]).all(axis=0)
        assert not same.any(), (s, np.flatnonzero(same)[:8])


def test_payload_columns(case):
    h, probes, _ = case
    n = h["n"]
    assert h["folder"].max() == fr.MAX_FOLDER and (h["folder"] == 0).sum() > 50 and (h["folder"] == fr.MAX_FOLDER).sum() > 50
    assert (h["folder"] == fr.ONE_FOLDER).sum() == 1 and h["live"][fr.ONE_ROW]
    last = np.flatnonzero(h["folder"] == fr.LAST_FOLDER)
    assert last.min() >= n // 32 * 32 and last.max() == n - 1 and 2 <= last.shape[0] < n - n // 32 * 32
    assert h["ifolder"].max() == 40
    for row, col, v in fr.edge_rows():
        other = "created" if col == "modified" else "modified"
        assert h[col][row] == v and h[other][row] == fr.IN_RANGE and h["live"][row] and row in probes
    assert {v for _, _, v in fr.edge_rows()} == {fr.LO - 1, fr.LO, fr.HI, fr.HI + 1, 0, fr.NEGATIVE, fr.INT64_MIN1, fr.INT64_MAX, fr.ABSENT}
    # every row's own term is its own; every row carries COMMON
    idx = h["idx"].reshape(n, -1)
    assert np.array_equal(idx[:, -1], fr.UNIQUE0 + np.arange(n)) and (idx[:, 0] == fr.COMMON).all()
    assert idx[:, 1:-1].max() < fr.UNIQUE0


def test_probes_cover_the_edges(case):
    h, probes, _ = case
    n = h["n"]
    p = set(probes.tolist())
    assert len(p) == probes.shape[0] >= 240 and set(range(131)) <= p and set(range(n - 70, n)) <= p
    for edge in (256, 512, n // 256 * 256, fr.PREFILTER_MIN_ROWS, fr.BATCH_MIN_ROWS):
        if edge < n:
            assert {edge - 1, edge} <= p, edge
    dead = probes[~h["live"][probes]]
    assert dead.shape[0] >= 20 and dead.min() < 131 and dead.max() >= n - 70      # tombstones among the first and last rows
    assert (~h["live"]).sum() > dead.shape[0]                                     # ... and between the probes
    assert h["live"][n - 1] and h["live"][0]
    assert set(np.flatnonzero(h["folder"] == fr.LAST_FOLDER).tolist()) <= p and fr.ONE_ROW in p
    for fid in (0, fr.MAX_FOLDER):
        assert (h["folder"][probes] == fid).sum() >= 10


def test_every_class_has_probes_on_both_sides(case):
    h, probes, m = case
    for c, spec in enumerate(fr.CLASSES):
        bits = m[c][probes]
        kind = fr.kind_of(spec)
        if kind == "none":
            assert not m[c].any(), c
        elif kind == "all":
            assert np.array_equal(m[c], h["live"]), c
            assert bits.any() and not bits.all(), c   # (the tombstoned probes fail)
        else:
            assert bits.sum() >= 1 and (~bits & h["live"][probes]).sum() >= 1, (c, int(bits.sum()))
    assert m[15].sum() == 1 and m[15][fr.ONE_ROW]
    assert m[16].any() and np.flatnonzero(m[16]).min() >= h["n"] // 32 * 32
    # the restated predicate is the one of test_batch_filters_gpu.py on the real filter objects
    for spec, f in zip(fr.CLASSES, fr.filters()):
        assert np.array_equal(fr.class_mask(spec, h), fr.class_mask(f, h))
        assert (f is None) == (spec is None) and (f is None or f.is_empty() == spec.is_empty())


def test_the_engine_sees_as_many_classes_as_the_prefix_names():
    """None and the empty filter are one class to the engine; every other pair of classes differs"""
    keys = [None if f is None else f.key() for f in fr.filters()]
    assert keys[0] is None and keys[-1] is None
    assert len(set(keys[:-1])) == len(keys) - 1
    for m in fr.CLASS_COUNTS:
        assert len(set(keys[:m])) == min(m, len(keys) - 1)


def test_no_mutant_survives(case):
    """every wrong predicate changes the expected answer of at least one probe under at least one class"""
    h, probes, m = case
    table = fr.mutants(h)
    assert len(table) == 13
    survivors = []
    for name, wrong in table.items():
        changed = (wrong[:, probes] != m[:, probes])
        print(f"n={h['n']} {name}: {int(changed.sum())} (probe, class) answers change, classes {np.flatnonzero(changed.any(axis=1)).tolist()}")
        if not changed.any():
            survivors.append(name)
    assert not survivors, survivors


def test_a_date_mutant_is_caught_at_its_edge_row(case):
    """the edge rows are what catches the date mutants: each changes the bit of the row planted for it"""
    h, _, m = case
    at = {(col, v): row for row, col, v in fr.edge_rows()}
    table = fr.mutants(h)
    assert table["> for >= at lo"][8][at[("modified", fr.LO)]] != m[8][at[("modified", fr.LO)]]
    assert table["< for <= at hi"][9][at[("modified", fr.HI)]] != m[9][at[("modified", fr.HI)]]
    assert table["> for >= at lo"][13][at[("created", fr.LO)]] != m[13][at[("created", fr.LO)]]
    assert table["absent passes a one-sided range"][9][at[("modified", fr.ABSENT)]] and not m[9][at[("modified", fr.ABSENT)]]
    assert table["absent passes a one-sided range"][19][at[("created", fr.ABSENT)]] and not m[19][at[("created", fr.ABSENT)]]
    assert table["created and modified swapped"][10][at[("created", fr.HI + 1)]] != m[10][at[("created", fr.HI + 1)]]
    assert m[18][at[("modified", 0)]] and not m[18][at[("modified", fr.NEGATIVE)]] and not m[18][at[("modified", fr.INT64_MIN1)]]
    assert m[19][at[("created", fr.INT64_MAX)]] and m[8][at[("modified", fr.INT64_MAX)]]


def test_helpers_keep_the_host_copy_in_step():
    h = fr.corpus(fr.N_SMALL)
    fr.delete(h, fr.dead_rows(fr.N_SMALL))
    keep = np.flatnonzero(h["live"])
    g = fr.take_rows(h, keep)
    assert g["n"] == keep.shape[0] and g["live"].all() and np.array_equal(g["folder"], h["folder"][keep])
    assert np.array_equal(g["idx"].reshape(g["n"], -1)[:, -1], fr.UNIQUE0 + keep)
    both = fr.append_rows(g, fr.take_rows(h, keep[:3]))
    assert both["n"] == g["n"] + 3 and both["off"][-1] == both["idx"].shape[0] and np.array_equal(both["x"][-3:], h["x"][keep[:3]])
    pairs = fr.sample_pairs(300, len(fr.CLASSES))
    assert len(set(pairs)) == len(pairs) >= 200
    # check_probe: the two statements
    mask = np.array([True, False, True, True])
    fr.check_probe(np.array([2, 0]), 2, mask, "ok")
    fr.check_probe(np.array([0, 2]), 1, mask, "ok")
    for rows, r in ((np.array([0, 2]), 2), (np.array([2, 1]), 2), (np.array([0, 1]), 1), (np.zeros(0, np.int64), 3)):
        with pytest.raises(AssertionError):
            fr.check_probe(rows, r, mask, "wrong")
