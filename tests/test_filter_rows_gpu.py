"""Every probed row's pass bit decides a winner, on each route that consumes a filter (voitta_rag_amd/csrc/filter.hip):
the corpora, classes and probes of tests/filter_rows.py on the device. The dense query of probe r is row r's own vector,
its sparse query the term only r carries plus one every row carries: under class c the probe is returned, and first, iff
the NumPy mask of c passes it, and every returned row passes. A seeded sample of (probe, class) pairs is held in full, rows
and score bits, against oracle.core. test_filter_rows_cpu.py proves without a device that a subtly wrong predicate (a bit
one row or one word off, a wrong edge of a date range, a neighbour's pass table, ...) changes some probe's answer.

Routes, and the counter of Engine.stats() that proves each:
  bytes   exact dense scan (N_SMALL: two_stage and batched stay), two-stage scan (N_BIG, one query: two_stage; int8 and
          f16 shadow), batched scan under one filter (N_BIG, 17 queries, int8: batched), score array + selection (k = 65)
  bytes   sparse: the inverted scan of one query, the per-query batch route (15 queries: sparse_grouped stays), the
          grouped scan with seed thresholds (17 queries: sparse_grouped), the forward scan (VR_SPARSE_INVERTED=0, and queries
          of 33 terms), the full scan of given weights, score array + selection (k = 65); both hybrid forms
  planes  batched dense scan with a filter per query (search_dense_multi, search_hybrid_batch_multi) with 1, 7, 8, 9, 16,
          17 and all classes in one batch (batched; with some 250 queries per class that counter alone would also rise
          on a class-by-class run over byte masks), and in batches whose classes hold 14 queries at most, where only the
          plane scan counts into `batched`; the class-grouped sparse scan in a child process whose 129 small upserts keep
          129 segments (VR_INV_REBUILD_FACTOR is read once per process), in such batches too (sparse_grouped)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import filter_rows as fr
from oracle import core as ocore
from oracle import fusion as ofus

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
K, K_BIG, LIMIT, WEIGHT = 10, fr.kFusedMaxK + 1, 5, 0.3
NQ_BATCH = fr.kQueryBlock + 1      # 17 queries: more than one dense block; at N_BIG the batched scan
NQ_PER_QUERY = fr.GROUPED_MIN_QUERIES - 1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class World:
    """an engine, its host copy, the probes and the classes' masks; the oracle's scores of the probes' queries"""

    def __init__(self, n, upserts=None):
        from voitta_rag_amd import Engine

        self.h = fr.corpus(n)
        self.e = Engine(fr.DIM)
        fr.upsert_all(self.e, self.h, upserts)
        dead = fr.dead_rows(n)
        self.e.delete_rows(dead)
        fr.delete(self.h, dead)
        self.specs = list(fr.CLASSES)
        self.flts = fr.filters()
        self.set_probes(fr.probe_rows(n))
        self.singles = {}

    def set_probes(self, probes, own_terms=None):
        self.probes = np.asarray(probes, np.int64)
        self.terms = self.h["idx"].reshape(self.h["n"], -1)[self.probes, -1] if own_terms is None else own_terms
        self.masks = fr.masks(self.h, self.specs)
        self._dense = self._sparse = None

    @property
    def n_probes(self):
        return self.probes.shape[0]

    def xq(self, pis):
        return np.ascontiguousarray(self.h["x"][self.probes[np.asarray(pis)]])

    def sq(self, pi, pad=0):
        return fr.sparse_query(int(self.terms[pi]) - fr.UNIQUE0, pad)

    def dense_scores(self, pi):
        if self._dense is None:
            qh = ocore.cosine_preprocess(self.xq(range(self.n_probes)))
            self._dense = ocore.dense_scores(qh, ocore.cosine_preprocess(self.h["x"]))
        return self._dense[pi]

    def sparse_scores(self, pi):
        if self._sparse is None:
            self._sparse = (ocore.SparseOracle.from_csr(self.h["off"], self.h["idx"], self.h["val"], self.h["live"]), {})
        oracle, memo = self._sparse
        if pi not in memo:
            memo[pi] = oracle.scores(*self.sq(pi))
        return memo[pi]

    def pairs(self, n_cls=None):
        n_cls = len(self.specs) if n_cls is None else n_cls
        return [(pi, ci) for ci in range(n_cls) for pi in range(self.n_probes)]

    def chunks(self, size):
        """the probes in calls of exactly `size` queries (the last one wraps around)"""
        n = self.n_probes
        return [[(a + j) % n for j in range(size)] for a in range(0, n, size)]

    def close(self):
        self.e.close()


def verify(w, got, kind, k, tag, sample=True):
    """got: {(probe index, class index): answer}. The probe statements for every pair; rows and score bits against the
    oracle for the sampled pairs among them. kind: dense | sparse | hybrid (k = the limit)."""
    for (pi, ci), ans in got.items():
        fr.check_probe(ans[0], int(w.probes[pi]), w.masks[ci], (tag, kind, "probe", int(w.probes[pi]), "class", ci))
    if not sample:
        return 0
    n = 0
    for pi, ci in fr.sample_pairs(w.n_probes, len(w.specs)):
        if (pi, ci) not in got:
            continue
        n += 1
        ans, mask, where = got[(pi, ci)], w.masks[ci].astype(np.uint8), (tag, kind, int(w.probes[pi]), ci)
        if kind == "hybrid":
            dr, ds = ocore.topk(w.dense_scores(pi), 3 * k, mask)
            sr, ss = ocore.topk(w.sparse_scores(pi), 3 * k, mask)
            want = ofus.hybrid_fuse(list(zip(dr.tolist(), ds.tolist())), list(zip(sr.tolist(), ss.tolist())), k, WEIGHT, "json")
            assert ans[0].tolist() == [r for r, _, _ in want] and ans[1].tolist() == [s for _, s, _ in want], where
            continue
        wr, ws = ocore.topk(w.dense_scores(pi) if kind == "dense" else w.sparse_scores(pi), k, mask)
        assert np.array_equal(ans[0], wr) and np.array_equal(_bits(ans[1]), _bits(ws)), (where, ans[0][:4], wr[:4])
    return n


def delta(e, before):
    after = e.stats()
    return {c: after[c] - before[c] for c in after}


@pytest.fixture(scope="module")
def small(gpu):
    w = World(fr.N_SMALL)
    yield w
    w.close()


@pytest.fixture(scope="module")
def big(gpu):
    w = World(fr.N_BIG)
    yield w
    w.close()


def single_dense(w, pi, ci):
    """search_dense with one query and its own filter, asked once per world"""
    key = ("dense", pi, ci)
    if key not in w.singles:
        w.singles[key] = w.e.search_dense(w.xq([pi]), K, w.flts[ci])[0]
    return w.singles[key]


def single_hybrid(w, pi, ci):
    key = ("hybrid", pi, ci)
    if key not in w.singles:
        w.singles[key] = w.e.search_hybrid(w.xq([pi])[0], *w.sq(pi), LIMIT, WEIGHT, flt=w.flts[ci])
    return w.singles[key]


def dense_in_calls(w, size, k=K):
    got = {}
    for ci, f in enumerate(w.flts):
        for chunk in w.chunks(size):
            for pi, ans in zip(chunk, w.e.search_dense(w.xq(chunk), k, f)):
                got[(pi, ci)] = ans
    return got


# ---- byte masks: one filter per call --------------------------------------------------------------------------------

def test_dense_exact_scan_one_query(small):
    w = small
    before = w.e.stats()
    got = {(pi, ci): single_dense(w, pi, ci) for pi, ci in w.pairs()}
    d = delta(w.e, before)
    assert d["two_stage"] == 0 and d["batched"] == 0
    assert verify(w, got, "dense", K, "exact, one query") >= 200


def test_dense_exact_scan_17_queries(small):
    w = small
    before = w.e.stats()
    got = dense_in_calls(w, NQ_BATCH)
    d = delta(w.e, before)
    assert d["two_stage"] == 0 and d["batched"] == 0
    assert len(got) == len(w.pairs()) and verify(w, got, "dense", K, "exact, 17 queries") >= 200


def _world_of(shadow, request, monkeypatch):
    if shadow == "int8":
        return request.getfixturevalue("big"), False
    monkeypatch.setenv("VR_PREFILTER", "f16")  # read when the engine is created
    return World(fr.N_BIG), True


@pytest.mark.parametrize("shadow", ["int8", "f16"])
def test_dense_two_stage_scan_one_query(gpu, shadow, request, monkeypatch):
    w, own = _world_of(shadow, request, monkeypatch)
    try:
        before = w.e.stats()
        got = {(pi, ci): w.e.search_dense(w.xq([pi]), K, w.flts[ci])[0] for pi, ci in w.pairs()}
        d = delta(w.e, before)
        assert d["two_stage"] == len(got) and d["fallback"] == 0 and d["batched"] == 0
        assert verify(w, got, "dense", K, f"two-stage {shadow}") >= 200
    finally:
        if own:
            w.close()


@pytest.mark.parametrize("shadow", ["int8", "f16"])
def test_dense_17_queries_under_one_filter(gpu, shadow, request, monkeypatch):
    """int8: the batched scan on the byte mask; f16 (no batched scan): a block of 16 on the exact scan and one two-stage query"""
    w, own = _world_of(shadow, request, monkeypatch)
    try:
        before = w.e.stats()
        got = dense_in_calls(w, NQ_BATCH)
        d = delta(w.e, before)
        calls = len(w.flts) * len(w.chunks(NQ_BATCH))
        if shadow == "int8":
            assert d["batched"] == NQ_BATCH * calls and d["batch_fallback"] == 0
        else:
            assert d["batched"] == 0 and d["two_stage"] == calls
        assert verify(w, got, "dense", K, f"17 queries {shadow}") >= 200
    finally:
        if own:
            w.close()


@pytest.mark.parametrize("size", ["small", "big"])
def test_score_array_and_selection_above_64(size, request):
    """k = 65: no fused list holds it; dense and sparse scores of every row under the byte mask, then topk_select"""
    w = request.getfixturevalue(size)
    before = w.e.stats()
    pairs = fr.sample_pairs(w.n_probes, len(w.specs))
    dense = {(pi, ci): w.e.search_dense(w.xq([pi]), K_BIG, w.flts[ci])[0] for pi, ci in pairs}
    sparse = {(pi, ci): w.e.search_sparse(*w.sq(pi), K_BIG, w.flts[ci]) for pi, ci in pairs}
    d = delta(w.e, before)
    assert d["two_stage"] == 0 and d["batched"] == 0 and d["sparse_grouped"] == 0
    assert verify(w, dense, "dense", K_BIG, "k = 65") >= 200 and verify(w, sparse, "sparse", K_BIG, "k = 65") >= 200
    # the largest k a search takes
    few = pairs[::10]
    dense = {(pi, ci): w.e.search_dense(w.xq([pi]), fr.kMaxK, w.flts[ci])[0] for pi, ci in few}
    sparse = {(pi, ci): w.e.search_sparse(*w.sq(pi), fr.kMaxK, w.flts[ci]) for pi, ci in few}
    assert verify(w, dense, "dense", fr.kMaxK, "k = 1024") >= 20 and verify(w, sparse, "sparse", fr.kMaxK, "k = 1024") >= 20


@pytest.mark.parametrize("size", ["small", "big"])
def test_sparse_one_query(size, request):
    """the inverted scan of one query (its terms' postings only)"""
    w = request.getfixturevalue(size)
    got = {(pi, ci): w.e.search_sparse(*w.sq(pi), K, w.flts[ci]) for pi, ci in w.pairs()}
    assert verify(w, got, "sparse", K, "inverted, one query") >= 200


@pytest.mark.parametrize("size", ["small", "big"])
def test_sparse_forward_scan(size, request, monkeypatch):
    """the forward scan: every query with the inverted index switched off (read per call), and queries of 33 distinct
    terms, which the inverted scans do not take, alone and inside a batch"""
    w = request.getfixturevalue(size)
    assert len(w.sq(0, fr.kInvMaxTerms - 1)[0]) == fr.kInvMaxTerms + 1
    long = {}
    before = w.e.stats()
    for ci, f in enumerate(w.flts):
        for chunk in w.chunks(NQ_BATCH):
            for pi, ans in zip(chunk, w.e.search_sparse_batch([w.sq(pi, fr.kInvMaxTerms - 1) for pi in chunk], K, f)):
                long[(pi, ci)] = ans
    assert delta(w.e, before)["sparse_grouped"] == 0   # (every query of these batches is served alone)
    assert verify(w, long, "sparse", K, "33 terms") >= 200
    monkeypatch.setenv("VR_SPARSE_INVERTED", "0")
    got = {(pi, ci): w.e.search_sparse(*w.sq(pi), K, w.flts[ci]) for pi, ci in w.pairs()}
    assert verify(w, got, "sparse", K, "forward, one query") >= 200


@pytest.mark.parametrize("size", ["small", "big"])
def test_sparse_batches_per_query_and_grouped(size, request):
    """15 queries: seed and pruned scan per query; 17 queries: the grouped scan with seed thresholds (the class-grouped scan
    of filtered batches needs 128 segments: test_class_grouped_sparse_scan_reads_the_planes)"""
    w = request.getfixturevalue(size)
    for nq, grouped in ((NQ_PER_QUERY, False), (NQ_BATCH, True)):
        got = {}
        before = w.e.stats()
        for ci, f in enumerate(w.flts):
            for chunk in w.chunks(nq):
                for pi, ans in zip(chunk, w.e.search_sparse_batch([w.sq(pi) for pi in chunk], K, f)):
                    got[(pi, ci)] = ans
        calls = len(w.flts) * len(w.chunks(nq))
        assert delta(w.e, before)["sparse_grouped"] == (nq * calls if grouped else 0)
        assert verify(w, got, "sparse", K, f"batches of {nq}") >= 200


@pytest.mark.parametrize("size", ["small", "big"])
def test_sparse_given_weights_take_the_full_scan(size, request):
    """weights_given: no seed and no grouped scan, every term's postings of every segment. The oracle has no entry for given
    weights; with weight 1000 on the probe's own term (values lie in [0.2, 2.2)) the probe statements hold as they are."""
    w = request.getfixturevalue(size)
    got = {}
    before = w.e.stats()
    for ci, f in enumerate(w.flts):
        for chunk in w.chunks(NQ_BATCH):
            qs = [(w.sq(pi)[0], np.array([1000.0, 1.0], np.float32)) for pi in chunk]
            for pi, ans in zip(chunk, w.e.search_sparse_batch(qs, K, f, weights_given=True)):
                got[(pi, ci)] = ans
    assert delta(w.e, before)["sparse_grouped"] == 0
    assert len(got) == len(w.pairs())
    verify(w, got, "sparse", K, "given weights", sample=False)


@pytest.mark.parametrize("size", ["small", "big"])
def test_hybrid_one_query(size, request):
    w = request.getfixturevalue(size)
    got = {(pi, ci): single_hybrid(w, pi, ci) for pi, ci in w.pairs()}
    assert verify(w, got, "hybrid", LIMIT, "hybrid, one query") >= 200


@pytest.mark.parametrize("size", ["small", "big"])
def test_hybrid_batch_under_one_filter(size, request):
    w = request.getfixturevalue(size)
    got = {}
    before = w.e.stats()
    for ci, f in enumerate(w.flts):
        for chunk in w.chunks(NQ_BATCH):
            for pi, ans in zip(chunk, w.e.search_hybrid_batch(w.xq(chunk), [w.sq(pi) for pi in chunk], LIMIT, WEIGHT, flt=f)):
                got[(pi, ci)] = ans
    d = delta(w.e, before)
    calls = len(w.flts) * len(w.chunks(NQ_BATCH))
    assert d["sparse_grouped"] == NQ_BATCH * calls and d["batched"] == (NQ_BATCH * calls if size == "big" else 0)
    assert verify(w, got, "hybrid", LIMIT, "hybrid batch") >= 200


# ---- bit planes: a filter per query -----------------------------------------------------------------------------------

def _same(a, b):
    return all(x.tolist() == y.tolist() for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("n_cls", fr.CLASS_COUNTS)
def test_dense_multi_reads_the_planes(big, n_cls):
    """all probes x the first n_cls classes in one batch: 8 classes fill one grid.y step of filter_planes_kernel, 9 start
    the second, 17 the third. Row i is the single call with query i's own filter, bit for bit."""
    w = big
    pairs = w.pairs(n_cls)
    q = w.xq([pi for pi, _ in pairs])
    before = w.e.stats()
    out = w.e.search_dense_multi(q, K, [w.flts[ci] for _, ci in pairs])
    d = delta(w.e, before)
    assert d["batched"] == len(pairs) and d["batch_fallback"] == 0
    got = dict(zip(pairs, out))
    for (pi, ci), ans in got.items():
        one = single_dense(w, pi, ci)
        assert np.array_equal(ans[0], one[0]) and np.array_equal(_bits(ans[1]), _bits(one[1])), (n_cls, int(w.probes[pi]), ci)
    n = verify(w, got, "dense", K, f"dense multi, {n_cls} classes")
    assert n >= 200 or n_cls < len(w.specs)


@pytest.mark.parametrize("n_cls", fr.CLASS_COUNTS)
def test_hybrid_multi_reads_the_planes(big, n_cls):
    """the dense legs share the batched scan and read the planes; at this size the sparse legs run class by class on
    byte masks (the grouped scan with seed thresholds)"""
    w = big
    pairs = w.pairs(n_cls)
    q = w.xq([pi for pi, _ in pairs])
    before = w.e.stats()
    out = w.e.search_hybrid_batch_multi(q, [w.sq(pi) for pi, _ in pairs], [LIMIT] * len(pairs), [WEIGHT] * len(pairs),
                                        [w.flts[ci] for _, ci in pairs])
    d = delta(w.e, before)
    assert d["batched"] == len(pairs) and d["batch_fallback"] == 0 and d["sparse_grouped"] == len(pairs)
    got = dict(zip(pairs, out))
    for (pi, ci), ans in got.items():
        assert _same(ans, single_hybrid(w, pi, ci)), (n_cls, int(w.probes[pi]), ci)
    n = verify(w, got, "hybrid", LIMIT, f"hybrid multi, {n_cls} classes")
    assert n >= 200 or n_cls < len(w.specs)


PER_CLASS = 7   # probes per class of a batch whose classes are too small for any route but the planes


def small_class_batches(w):
    """All (probe, class) pairs in batches of PER_CLASS probes x every class. No class of such a batch holds more than
    kQueryBlock queries (None and the empty filter are one class: 2 x PER_CLASS), so run class by class on byte masks none
    would reach the batched dense scan (more than kQueryBlock queries) or the grouped sparse scan (GROUPED_MIN_QUERIES):
    only a scan that takes the whole batch and tells the classes apart by their planes counts into `batched` and
    `sparse_grouped`."""
    keys = [None if f is None else f.key() for f in w.flts]
    out = []
    for a in range(0, w.n_probes, PER_CLASS):
        pairs = [(pi, ci) for ci in range(len(w.flts)) for pi in range(a, min(a + PER_CLASS, w.n_probes))]
        sizes = {}
        for _, ci in pairs:
            sizes[keys[ci]] = sizes.get(keys[ci], 0) + 1
        assert max(sizes.values()) <= fr.kQueryBlock and max(sizes.values()) < fr.GROUPED_MIN_QUERIES
        assert len(pairs) > fr.kQueryBlock
        out.append(pairs)
    return out


def test_only_the_planes_reach_the_batched_scan(big):
    """Batches whose classes hold 14 queries at most: had the filtered batch been run class by class on byte masks, no
    class would have reached the batched scan and `batched` would stay. The sparse legs of these batches (4 segments: no
    class-grouped scan) do run class by class, on the per-query kernels: `sparse_grouped` stays."""
    w = big
    dense, hybrid = {}, {}
    for pairs in small_class_batches(w):
        q, flts = w.xq([pi for pi, _ in pairs]), [w.flts[ci] for _, ci in pairs]
        before = w.e.stats()
        out = w.e.search_dense_multi(q, K, flts)
        d = delta(w.e, before)
        assert d["batched"] == len(pairs) and d["batch_fallback"] == 0
        dense.update(zip(pairs, out))
        before = w.e.stats()
        out = w.e.search_hybrid_batch_multi(q, [w.sq(pi) for pi, _ in pairs], [LIMIT] * len(pairs), [WEIGHT] * len(pairs), flts)
        d = delta(w.e, before)
        assert d["batched"] == len(pairs) and d["batch_fallback"] == 0 and d["sparse_grouped"] == 0
        hybrid.update(zip(pairs, out))
    assert len(dense) == len(hybrid) == len(w.pairs())
    for (pi, ci), ans in dense.items():
        one = single_dense(w, pi, ci)
        assert np.array_equal(ans[0], one[0]) and np.array_equal(_bits(ans[1]), _bits(one[1])), (int(w.probes[pi]), ci)
        assert _same(hybrid[(pi, ci)], single_hybrid(w, pi, ci)), (int(w.probes[pi]), ci)
    assert verify(w, dense, "dense", K, "small classes") >= 200 and verify(w, hybrid, "hybrid", LIMIT, "small classes") >= 200


SEGMENTS_UPSERTS = (128,) * 128 + (37,)   # 129 segments of the inverted index, as long as it is not rebuilt

_CHILD = r"""
import json, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import filter_rows as fr
import test_filter_rows_gpu as t
w = t.World(fr.N_BIG, t.SEGMENTS_UPSERTS)
got, total = {}, {"sparse_grouped": 0, "batched": 0, "sparse_group_redo": 0}
for pairs in t.small_class_batches(w):
    before = w.e.stats()
    out = w.e.search_hybrid_batch_multi(w.xq([pi for pi, _ in pairs]), [w.sq(pi) for pi, _ in pairs], [t.LIMIT] * len(pairs),
                                        [t.WEIGHT] * len(pairs), [w.flts[ci] for _, ci in pairs])
    d = t.delta(w.e, before)
    assert d["sparse_grouped"] == len(pairs) and d["batched"] == len(pairs), (len(pairs), d)
    for c in total:
        total[c] += d[c]
    got.update(zip(pairs, out))
n = t.verify(w, got, "hybrid", t.LIMIT, "class-grouped")
same = 0
for pi, ci in fr.sample_pairs(w.n_probes, len(w.specs)):
    assert t._same(got[(pi, ci)], t.single_hybrid(w, pi, ci)), (int(w.probes[pi]), ci)
    same += 1
print(json.dumps({"queries": len(got), "pairs": len(w.pairs()), "oracle": n, "single": same, "stats": total}))
w.close()
"""


def test_class_grouped_sparse_scan_reads_the_planes(gpu, tmp_path):
    """The sparse legs of a filtered batch share ONE grouped scan, whose groups read their class's plane, once the inverted
    index has 128 segments. 129 upserts of 128 rows give N_BIG rows that many as long as the index is not rebuilt; the
    rebuild factor is read once per process, so a fresh process with VR_INV_REBUILD_FACTOR set builds this engine and runs
    every (probe, class) pair there in the batches of small_class_batches: no class holds GROUPED_MIN_QUERIES queries, so
    had the batch fallen back to its classes' byte masks (an index rebuilt after all, fewer than 128 segments) the
    per-query kernels would have served it and `sparse_grouped` would stay; the child asserts per batch that it rises by
    the batch size. Checked there as well: the probe statements, the oracle sample, single calls."""
    env = dict(os.environ, VR_INV_REBUILD_FACTOR="1000")
    p = subprocess.run([sys.executable, "-c", _CHILD, HERE, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    print(r)
    assert r["queries"] == r["pairs"] and r["stats"]["sparse_grouped"] == r["queries"] and r["stats"]["batched"] == r["queries"]
    assert r["oracle"] >= 200 and r["single"] >= 200


# ---- state changes at N_SMALL ---------------------------------------------------------------------------------------

def _probe_check(w, tag):
    """every (probe, class) pair through the byte-mask dense and sparse batches and the filtered hybrid batch"""
    dense, sparse = dense_in_calls(w, NQ_BATCH), {}
    for ci, f in enumerate(w.flts):
        for chunk in w.chunks(NQ_BATCH):
            for pi, ans in zip(chunk, w.e.search_sparse_batch([w.sq(pi) for pi in chunk], K, f)):
                sparse[(pi, ci)] = ans
    pairs = w.pairs()
    out = w.e.search_hybrid_batch_multi(w.xq([pi for pi, _ in pairs]), [w.sq(pi) for pi, _ in pairs], [LIMIT] * len(pairs),
                                        [WEIGHT] * len(pairs), [w.flts[ci] for _, ci in pairs])
    assert len(dense) == len(sparse) == len(pairs)
    verify(w, dense, "dense", K, tag, sample=False)
    verify(w, sparse, "sparse", K, tag, sample=False)
    verify(w, dict(zip(pairs, out)), "hybrid", LIMIT, tag, sample=False)
    passing = w.masks[:, w.probes]
    assert passing.any(axis=1).sum() >= len(w.specs) - 4 and (~passing).any(axis=1).all(), tag  # (both sides are still probed)


def test_state_changes_keep_every_probe_right(gpu, tmp_path):
    from voitta_rag_amd import Engine, SearchFilter

    w = World(fr.N_SMALL)
    e2 = None
    try:
        _probe_check(w, "stored")
        more = fr.more_dead_rows(fr.N_SMALL)
        assert w.h["live"][more].all()
        w.e.delete_rows(more)
        fr.delete(w.h, more)
        w.set_probes(w.probes)
        _probe_check(w, "after further deletes")
        # compact: rows, masks and probes renumbered through the returned map
        remap = w.e.compact()
        keep = np.flatnonzero(w.h["live"])
        want = np.full(fr.N_SMALL, -1, np.int64)
        want[keep] = np.arange(keep.shape[0])
        assert np.array_equal(remap, want)
        alive = w.h["live"][w.probes]
        terms = w.terms[alive]
        w.h = fr.take_rows(w.h, keep)
        w.set_probes(remap[w.probes[alive]], terms)
        assert np.array_equal(w.h["idx"].reshape(w.h["n"], -1)[w.probes, -1], terms)
        # tombstone a few of the renumbered rows, so that the all-pass classes keep failing probes
        again = np.array([r for r in w.probes[2::9] if w.h["folder"][r] not in (fr.ONE_FOLDER, fr.LAST_FOLDER)])
        w.e.delete_rows(again)
        fr.delete(w.h, again)
        w.set_probes(w.probes, terms)
        _probe_check(w, "after compact")
        # save, load into a fresh engine
        path = str(tmp_path / "rows.vrindex")
        w.e.save(path)
        e2 = Engine(fr.DIM)
        e2.load(path)
        w.e.close()
        w.e = e2
        _probe_check(w, "after save and load")
        # an upsert that brings a folder id above the largest: the pass tables grow; filters from before and new ones
        g = fr.take_rows(fr.corpus(fr.N_SMALL, seed=99), np.arange(40))
        g["idx"] = g["idx"].copy()
        g["idx"].reshape(40, -1)[:, -1] += 100_000    # (their own terms stay their own)
        new_max = fr.MAX_FOLDER + 1001
        g["folder"][::3] = new_max
        n0 = w.h["n"]
        w.h = fr.append_rows(w.h, g)
        fr.upsert_all(w.e, w.h, (40,), first=n0)
        w.specs = w.specs + [fr.Spec(folder_filter=new_max), fr.Spec(include_folders=[new_max, fr.MAX_FOLDER]),
                             fr.Spec(exclude_folders=[new_max, 0]), fr.Spec(include_folders=[new_max + 1, 5])]
        old = w.flts
        w.flts = fr.filters(w.specs)
        w.flts[:len(old)] = old                        # the filter objects built before the upsert
        assert isinstance(w.flts[-1], SearchFilter)
        new_probes = np.arange(n0, n0 + 40)
        w.set_probes(np.concatenate([w.probes, new_probes]),
                     np.concatenate([terms, w.h["idx"].reshape(w.h["n"], -1)[new_probes, -1]]))
        assert w.masks[len(old)][new_probes].sum() == 14
        _probe_check(w, "after an upsert with a larger folder id")
    finally:
        w.close()
