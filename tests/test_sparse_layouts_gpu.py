"""Planted postings on every route of the inverted sparse index (voitta_rag_amd/csrc/invert.hip): the corpora and the
route model of tests/sparse_layouts.py, run on the device. Every answer is held bit for bit against oracle.core (rows,
f32 score bits, counts; ties to the lower row); where two routes serve the same batch they are held against each other;
the counters sparse_grouped, sparse_group_redo and sparse_group_candidates are asserted against the model wherever a
batch takes the grouped scan. test_sparse_layouts_cpu.py proves, without a GPU, that each case meets the condition it is
there for; profiles/sparse_layouts_checks.md lists the faults these cases catch."""
import numpy as np
import pytest

import sparse_layouts as sp
from oracle import core as ocore
from oracle import fusion as ofus
from search_layouts import gaussian

pytestmark = pytest.mark.gpu

DIM = 16
KS = (1, 3, 10, 30, 40, 41, 64)  # 3: a threshold among the first rows; 40 / 41: the sample's capacity at 1024-row segments
KS_LARGE = (10, 40, 41)          # the batches of 130 (the model of 130 riders costs CPU time per k)
FOLDER_TIE_OUT = sp.FOLDER_TIE_OUT


class Geo:
    """an engine of one geometry with its oracle, live rows and folders"""

    def __init__(self, name, corpus, upserts, deletes=True):
        from voitta_rag_amd import Engine

        self.name = name
        self.off, self.idx, self.val, self.plan = corpus
        n = self.plan["n"]
        self.x = gaussian(n, DIM, 7 + n)
        self.folder = self.plan.get("folder", np.zeros(n, np.int32)).copy()
        self.live = np.ones(n, bool)
        if deletes:
            self.live, self.dead, self.folder = sp.live_rows(self.off, self.idx, self.plan)
        self.e = Engine(DIM)
        at = 0
        for m in upserts:
            a, b = self.off[at], self.off[at + m]
            self.e.upsert(self.x[at:at + m], sparse=(self.off[at:at + m + 1] - a, self.idx[a:b], self.val[a:b]), folder_ids=self.folder[at:at + m])
            at += m
        if deletes:
            self.e.delete_rows(self.dead)
        self.oracle = ocore.SparseOracle.from_csr(self.off, self.idx, self.val, self.live)
        self._scores, self._prep = {}, {}

    def prepared(self, q, mask):
        """grouped_prepare of a query under a mask, computed once (the k of a test share it)"""
        key = (q[0].tobytes(), q[1].tobytes(), id(mask))
        if key not in self._prep:
            self._prep[key] = (mask, sp.grouped_prepare(self.scores(q), mask, self.plan["seg_base"], self.plan["seg_rows"]))
        return self._prep[key][1]

    def scores(self, q):
        key = (q[0].tobytes(), q[1].tobytes())
        if key not in self._scores:
            self._scores[key] = self.oracle.scores(q[0], q[1])
        return self._scores[key]

    def close(self):
        self.e.close()


def _geo(name):
    return Geo(name, sp.corpus_s(name), sp.GEOMETRIES[name])


@pytest.fixture(scope="module")
def s1024(gpu):
    g = _geo("s1024")
    yield g
    g.close()


@pytest.fixture(scope="module")
def s1021(gpu):
    g = _geo("s1021")
    yield g
    g.close()


@pytest.fixture(scope="module")
def s1row(gpu):
    g = _geo("s1row")
    yield g
    g.close()


@pytest.fixture(scope="module")
def p4096(gpu):
    g = Geo("p4096", sp.corpus_p(), sp.GEOMETRIES["p4096"], deletes=False)
    yield g
    g.close()


@pytest.fixture(scope="module")
def runs(gpu):
    g = Geo("runs", sp.corpus_r(), sp.R_UPSERTS, deletes=False)
    yield g
    g.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_oracle(g, qs, got, k, mask, tag):
    assert len(got) == len(qs)
    for i, q in enumerate(qs):
        if len(q[0]) == 0:
            assert len(got[i][0]) == 0, (tag, i)
            continue
        wr, ws = ocore.topk(g.scores(q), k, mask.astype(np.uint8))
        assert np.array_equal(got[i][0], wr), (tag, k, i, got[i][0][:8], wr[:8])
        assert np.array_equal(_bits(got[i][1]), _bits(ws)), (tag, k, i)


def _assert_same(a, b, tag):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(_bits(x[1]), _bits(y[1])), (tag, i)


def _flush(g):
    """sparse_group_candidates is added up when the NEXT batch starts: a one-term batch of the per-query route"""
    g.e.search_sparse_batch([sp.planted_queries()["absent"]], 1)


def _model_totals(g, qs, k, mask, sampled=True):
    """(queries the grouped scan is given up for, keys its selection ranks) of a batch, by the route model"""
    redo, gathered = [], 0
    for i, q in enumerate(qs):
        n_terms = np.unique(q[0]).shape[0]
        if n_terms == 0 or n_terms > sp.kInvMaxTerms:  # no terms: nothing offered; more than 32: served alone on the forward scan
            continue
        m = sp.grouped_model(None, mask, k, g.plan["seg_base"], g.plan["seg_rows"], sampled=sampled, prep=g.prepared(q, mask))
        gathered += m["gathered"]
        if m["redo"]:
            redo.append(i)
    return redo, gathered


def _grouped_batch(g, qs, k, flt, mask, tag):
    """one batch on the default route of a geometry-S engine (the sampled grouped scan), counters held against the model"""
    assert sp.pick_route(len(qs), g.plan["n_seg"]) == sp.ROUTE_GROUPED_SAMPLED
    redo, gathered = _model_totals(g, qs, k, mask)
    _flush(g)
    before = g.e.stats()
    got = g.e.search_sparse_batch(qs, k, flt)
    _flush(g)
    after = g.e.stats()
    delta = {c: after[c] - before[c] for c in ("sparse_grouped", "sparse_group_redo", "sparse_group_candidates")}
    print(f"{tag} k={k}: model redo={len(redo)} candidates={gathered}; observed {delta}")
    assert delta["sparse_grouped"] == len(qs), (tag, k)
    assert delta["sparse_group_redo"] == len(redo), (tag, k, redo)
    assert delta["sparse_group_candidates"] == gathered, (tag, k)
    _assert_oracle(g, qs, got, k, mask, tag)
    return got


# ---- geometry S: the sampled grouped scan ---------------------------------------------------------------------------

@pytest.mark.parametrize("geo,nq,shift,flood", [("s1024", 130, 0, True), ("s1024", 17, 1, False), ("s1021", 130, 1, True),
                                               ("s1021", 17, 0, False), ("s1row", 130, 0, False), ("s1row", 17, 1, True)])
def test_planted_batches_on_the_sampled_grouped_scan(geo, nq, shift, flood, request):
    """Winners the sample cannot see, the sample's capacity (k = 40 / 41 at 1024-row segments), terms of unsampled segments
    only (a region filled exactly, one key spilled, a spill area that overflows: that query and only the queries the model
    names are redone, no switch set), winners in the tail and in a one-row segment, a tie group with deleted members,
    mixed signs (a negative threshold, sums that cancel to +0.0, an all-negative query), queries of 24, 32 and 33 terms (two of
    32 share a group whose union is exactly 64), a
    term no row carries, no terms, a repeated term: planted at even and odd positions among riders."""
    g = request.getfixturevalue(geo)
    qs, at = sp.planted_batch(nq, shift, flood)
    for k in (KS if nq < 100 else KS_LARGE):
        got = _grouped_batch(g, qs, k, None, g.live, f"{geo}/nq{nq}/shift{shift}")
        if "cancel" in at and k == 41:  # the rows whose products cancel are hits with score +0.0, above the negative rows
            rows, scores = got[at["cancel"]]
            zero = _bits(scores) == 0  # (+0.0: 30 rows score above it, 30 below; an "untouched" row never shows)
            assert zero.sum() == 11 and np.isin(rows[zero], g.plan["cancel_rows"]).all() and (scores[:30] > 0).all()
        if "allneg" in at:
            assert (got[at["allneg"]][1] < 0).all() and len(got[at["allneg"]][0]) == min(k, 300)


def test_tie_group_of_70_with_deletes_and_a_filter(s1024):
    """70 equal scores across sampled and unsampled segments; two members deleted, a third filtered out: the lower rows win,
    at k = 10 (a threshold INSIDE the group: the key's row half decides) and k = 64 (no threshold)."""
    from voitta_rag_amd import SearchFilter

    g = s1024
    qs, at = sp.planted_batch(17, 0)
    flt = SearchFilter(exclude_folders=[FOLDER_TIE_OUT])
    mask = g.live & (g.folder != FOLDER_TIE_OUT)
    tie = g.plan["tie_rows"]
    alive = tie[mask[tie]]
    assert alive.shape[0] == sp.TIE_GROUP - 3
    for k in (10, 64):
        got = _grouped_batch(g, qs, k, flt, mask, "tie+filter")
        rows, scores = got[at["tie"]]
        assert np.array_equal(rows, alive[:k]) and np.unique(_bits(scores)).shape[0] == 1


@pytest.mark.parametrize("geo,nq", [("s1024", 130), ("s1021", 17), ("s1row", 60)])
def test_four_routes_agree_on_the_planted_batches(geo, nq, request, monkeypatch):
    """The same batch through the sampled grouped scan, the grouped scan with seed thresholds (VR_SPARSE_GROUP_SAMPLE=0),
    the per-query kernels (VR_SPARSE_GROUPED=0) and, in batches of fewer than 16, the per-query kernels again: identical
    rows and bits, and the oracle's."""
    g = request.getfixturevalue(geo)
    qs, _ = sp.planted_batch(nq, 1, flood=True)
    n_seg = g.plan["n_seg"]
    for k in (10, 64):
        want = g.e.search_sparse_batch(qs, k)
        _assert_oracle(g, qs, want, k, g.live, geo)
        monkeypatch.setenv("VR_SPARSE_GROUP_SAMPLE", "0")
        assert sp.pick_route(nq, n_seg, sample_env=False) == sp.ROUTE_GROUPED_SEED
        before = g.e.stats()["sparse_grouped"]
        seeded = g.e.search_sparse_batch(qs, k)
        assert g.e.stats()["sparse_grouped"] - before == nq
        monkeypatch.delenv("VR_SPARSE_GROUP_SAMPLE")
        monkeypatch.setenv("VR_SPARSE_GROUPED", "0")
        assert sp.pick_route(nq, n_seg, grouped_env=False) == sp.ROUTE_SEED_PRUNED
        before = g.e.stats()["sparse_grouped"]
        plain = g.e.search_sparse_batch(qs, k)
        assert g.e.stats()["sparse_grouped"] == before
        monkeypatch.delenv("VR_SPARSE_GROUPED")
        assert sp.pick_route(15, n_seg) == sp.ROUTE_SEED_PRUNED
        before = g.e.stats()["sparse_grouped"]
        small = [r for a in range(0, nq, 15) for r in g.e.search_sparse_batch(qs[a:a + 15], k)]
        assert g.e.stats()["sparse_grouped"] == before
        for other, tag in ((seeded, "seed thresholds"), (plain, "per query"), (small, "batches of 15")):
            _assert_same(want, other, (geo, k, tag))


@pytest.mark.parametrize("geo", ["s1024", "s1021"])
def test_class_planes_on_the_sampled_grouped_scan(geo, request):
    """Filtered batches (vr_search_hybrid_batch_multi) read a bit plane per class in the grouped scan: a class whose rows lie
    in unsampled segments only, one with fewer rows than the legs' k, one with none, one whose rows are segments' FIRST rows
    (on 1021-row segments: plane words that straddle), one that drops a member of the tie group. Expected: the oracle's legs
    fused as test_batch_hybrid_gpu.py fuses them, and search_hybrid per query."""
    from voitta_rag_amd import SearchFilter

    g = request.getfixturevalue(geo)
    nq, limit, w = 60, 10, 0.3
    sq, at = sp.planted_batch(nq, 0)
    sq[at["invisible"] + 2] = sp.planted_queries()["invisible"]
    fr = (np.array([sp.T_FIRSTROW], np.int32), np.ones(1, np.float32))
    classes = [(SearchFilter(include_folders=[1]), g.folder == 1), (SearchFilter(include_folders=[2]), g.folder == 2),
               (SearchFilter(include_folders=[]), np.zeros(g.plan["n"], bool)), (SearchFilter(include_folders=[4]), g.folder == 4),
               (SearchFilter(exclude_folders=[FOLDER_TIE_OUT]), g.folder != FOLDER_TIE_OUT)]
    cls = [i % 5 for i in range(nq)]
    cls[at["invisible"]], cls[at["invisible"] + 1], cls[at["invisible"] + 2] = 0, 1, 2
    cls[at["tie"]] = 4
    for i in range(nq):  # the first-row term under the first-row class (and under the others)
        if i % 8 == 7 and i not in at.values():
            sq[i], cls[i] = fr, (3 if i % 16 == 7 else 0)
    assert int(g.folder[g.plan["first_rows"][0]]) == 4 and (g.folder == 2).sum() == 5
    q = gaussian(nq, DIM, 99)
    xh = ocore.cosine_preprocess(g.x)
    dsc = ocore.dense_scores(ocore.cosine_preprocess(q), xh)
    assert sp.pick_route(nq, g.plan["n_seg"]) == sp.ROUTE_GROUPED_SAMPLED
    masks = [g.live & c[1] for c in classes]
    redo = [i for i in range(nq) if 0 < np.unique(sq[i][0]).shape[0] <= sp.kInvMaxTerms and
            sp.grouped_model(None, None, 3 * limit, g.plan["seg_base"], g.plan["seg_rows"], prep=g.prepared(sq[i], masks[cls[i]]))["redo"]]
    before = g.e.stats()
    got = g.e.search_hybrid_batch_multi(q, sq, [limit] * nq, [w] * nq, [classes[c][0] for c in cls])
    after = g.e.stats()
    print(f"{geo} class planes: model redo={redo}; observed sparse_group_redo +{after['sparse_group_redo'] - before['sparse_group_redo']}")
    assert after["sparse_grouped"] - before["sparse_grouped"] == nq  # (the redone queries run class by class, fewer than 16 each)
    assert after["sparse_group_redo"] - before["sparse_group_redo"] == len(redo)
    assert max(cls.count(c) for c in range(5)) < sp.GROUPED_MIN_QUERIES
    for i in range(nq):
        mask = masks[cls[i]].astype(np.uint8)
        dr, ds = ocore.topk(dsc[i], 3 * limit, mask)
        n_terms = np.unique(sq[i][0]).shape[0]
        if n_terms:
            sr, ss = ocore.topk(g.scores(sq[i]), 3 * limit, mask)
        else:
            sr, ss = np.zeros(0, np.int64), np.zeros(0, np.float32)
        want = ofus.hybrid_fuse(list(zip(dr.tolist(), ds.tolist())), list(zip(sr.tolist(), ss.tolist())), limit, w, "json")
        rows, scores, fd = got[i]
        assert rows.tolist() == [r for r, _, _ in want], (geo, i, cls[i])
        assert scores.tolist() == [s for _, s, _ in want], (geo, i, cls[i])
        if i in at.values() or i % 8 == 7:
            r1, s1, f1 = g.e.search_hybrid(q[i], sq[i][0], sq[i][1], limit, w, flt=classes[cls[i]][0])
            assert rows.tolist() == r1.tolist() and scores.tolist() == s1.tolist() and fd.tolist() == f1.tolist(), (geo, i)


# ---- geometry P: the per-query kernels --------------------------------------------------------------------------------

def _p_batch(nq):
    pq = sp.p_queries()
    qs = sp.riders(nq, sp.VOCAB, 500 + nq)
    at = {name: 2 * j + (j % 2) for j, name in enumerate(pq)}
    for name, i in at.items():
        qs[i] = pq[name]
    return qs, at


@pytest.mark.parametrize("nq,blocks", [(12, None), (12, "1"), (12, "2"), (17, None)])
def test_per_query_kernels_on_planted_segments(p4096, nq, blocks, monkeypatch):
    """Seed, pruned scan and the full scan of flagged shares (kSeedPruned: fewer than 16 queries, or VR_SPARSE_GROUPED=0) on
    5 full segments: a wave's table of partial sums overflows (winners passed on unfiltered and named by two essential
    terms), a wave buffers more than 448 candidates and flushes mid-segment (the ten best rows are scored twice), one block
    flags need_full (a huge weight in its segment) while the others prune, a seed that stops at kSeedRowsPerWave, a query
    whose terms are all essential, a query the seed finds nothing for, winners whose essential sums reach the threshold only
    with the non-essential terms' bound."""
    g = p4096
    qs, _ = _p_batch(nq)
    if blocks:
        monkeypatch.setenv("VR_SPARSE_BATCH_BLOCKS", blocks)
    if nq >= sp.GROUPED_MIN_QUERIES:
        monkeypatch.setenv("VR_SPARSE_GROUPED", "0")
    assert sp.pick_route(nq, g.plan["n_seg"], grouped_env=nq < sp.GROUPED_MIN_QUERIES) == sp.ROUTE_SEED_PRUNED
    before = g.e.stats()["sparse_grouped"]
    for k in (1, 10, 64):
        got = g.e.search_sparse_batch(qs, k)
        _assert_oracle(g, qs, got, k, g.live, ("p4096", nq, blocks))
        if k == 10:
            assert all(np.unique(r).shape[0] == r.shape[0] for r, _ in got)  # DISTINCT rows (a list that took a key twice repeats one)
    assert g.e.stats()["sparse_grouped"] == before


@pytest.mark.parametrize("blocks", ["1", "2"])
def test_survivor_cap_of_the_pruning_scan_without_a_seed(p4096, blocks, monkeypatch):
    """Given weights (route kFull: no seed, every t_frac = 1): inv_scan_segments prunes from its lists alone. One block walks
    all segments (or every second): its first segment fills wave 0's list, then the essential term marks 1023, 1024 and 1025
    rows of segment 2, all of which survive: the survivor buffer one under, at and one over kInvMaxSurvivors (over: the
    segment is added up in full after all). The oracle has no entry for given weights: the reference is the sum the forward
    scan defines, written out in f32 (ascending id: fl(fl(w_t v_t) + fl(w_b v_b))), and the forward scan itself
    (VR_SPARSE_INVERTED=0)."""
    g = p4096
    w_t, w_b = np.float32(1.0), np.float32(0.01)
    qs = [(np.array([t, sp.T_BALLAST], np.int32), np.array([w_t, w_b], np.float32)) for t in sp.T_SURV]
    rb, vb = sp.term_postings(g.off, g.idx, g.val, sp.T_BALLAST)
    ballast = np.zeros(g.plan["n"], np.float32)
    ballast[rb] = vb
    monkeypatch.setenv("VR_SPARSE_BATCH_BLOCKS", blocks)
    for k in (1, 10, 40):
        got = g.e.search_sparse_batch(qs, k, weights_given=True)
        monkeypatch.setenv("VR_SPARSE_INVERTED", "0")
        forward = g.e.search_sparse_batch(qs, k, weights_given=True)
        monkeypatch.delenv("VR_SPARSE_INVERTED")
        _assert_same(forward, got, ("forward scan", blocks, k))
        for (ids, _), (rows, scores) in zip(qs, got):
            rt, vt = sp.term_postings(g.off, g.idx, g.val, int(ids[0]))
            sc = (np.float32(0.0) + w_b * ballast).astype(np.float32)  # rows without the term: fl(w_b v_b)
            sc[rt] = (w_t * vt).astype(np.float32) + (w_b * ballast[rt]).astype(np.float32)
            wr, ws = ocore.topk(sc, k)
            assert np.array_equal(rows, wr) and np.array_equal(_bits(scores), _bits(ws)), (blocks, k, int(ids[0]))


def test_run_searches_at_every_segment_size(runs):
    """Segments of 1, 64, 65, 4096, 4097 and more than 64^3 postings; the segment's smallest and largest id, ids absent
    below, between and above; runs of 1, 64, 65, 256, 257 and 512 postings, the last one ending at the segment's last
    posting: through the single search (inv_wave_lower_bound), a small batch (the seed's and the pruned scan's walk, 4 x 64
    postings a round) and a batch of 17 or more (inv_wave_runs in the locate kernel)."""
    g = runs
    one = lambda *t: (np.array(t, np.int32), np.ones(len(t), np.float32))
    qs = [one(t) for t in sp.r_terms()]
    qs += [one(sp.R_COMMON0, t) for t, _ in sp.R_RUNS] + [one(100, 300, 900, 2000), one(50, 2000), one(2000, 2500)]
    assert len(qs) >= 17 and sp.pick_route(len(qs), g.plan["n_seg"]) == sp.ROUTE_GROUPED_SEED
    for k in (10, 64):
        for q in qs:
            rows, scores = g.e.search_sparse(q[0], q[1], k)
            wr, ws = ocore.topk(g.scores(q), k)
            assert np.array_equal(rows, wr) and np.array_equal(_bits(scores), _bits(ws)), ("single", k, q[0])
        before = g.e.stats()["sparse_grouped"]
        small = [r for a in range(0, len(qs), 13) for r in g.e.search_sparse_batch(qs[a:a + 13], k)]
        assert g.e.stats()["sparse_grouped"] == before
        _assert_oracle(g, qs, small, k, g.live, "runs, batches of 13")
        got = g.e.search_sparse_batch(qs, k)
        assert g.e.stats()["sparse_grouped"] - before == len(qs)
        _assert_oracle(g, qs, got, k, g.live, "runs, grouped")
