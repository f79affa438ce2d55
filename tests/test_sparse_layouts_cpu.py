"""The planted sparse layouts and their route model (tests/sparse_layouts.py), proven on the CPU from the oracle alone: the
mirrored constants are the sources', every geometry has the segments it is built for, and every case of the GPU matrix
(test_sparse_layouts_gpu.py) meets the condition it is there for: the route, the sample keys, the rows offered per segment,
spills and redos, and for the per-query route the seed, the blocks that prune and the 1 % margins of every inequality the
model relies on."""
import os
import re

import numpy as np
import pytest

import sparse_layouts as sp
from oracle import core as ocore

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voitta_rag_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_mirrored_constants_are_the_sources():
    for name, where in sp.CONSTANT_SOURCES.items():
        if name == "kInvSegRows":  # written as a shift
            assert "constexpr int kInvRowBits = 12;" in _source(where) and "constexpr int kInvSegRows = 1 << kInvRowBits;" in _source(where)
            assert sp.kInvSegRows == 1 << 12
            continue
        m = re.search(r"constexpr int %s = (\d+);" % name, _source(where))
        assert m, (name, where)
        assert int(m.group(1)) == getattr(sp, name), (name, where)
    inv, topk = _source("invert.hip"), _source("topk.hip")
    assert "constexpr int kGroup = 2;" in inv and sp.GROUP == 2
    assert ": 4096;" in inv and "std::min(4096, std::max(1, atoi(std::getenv(\"VR_SPARSE_GROUP_SPILL\"))))" in inv and sp.SPILL == 4096
    assert "return nq >= 16 && e->n_inv_seg <= 65535 &&" in inv and sp.GROUPED_MIN_QUERIES == 16
    assert "e->n_inv_seg >= 128 &&" in inv and sp.SAMPLED_MIN_SEGMENTS == 128
    assert "sampled ? static_cast<int>(n_seg / 16) : 1;" in inv and sp.SAMPLE_REGULAR == 16
    assert "(n_seg - kSampleTail + seg_stride - 1) / seg_stride + kSampleTail" in inv
    assert "std::max<int64_t>(kGrpCandCap, std::min<int64_t>(512, 8192 / std::max<int64_t>(n_seg, 1)))" in inv
    assert "e->n_inv_seg > 64 && e->n_inv_seg > rebuild_factor * ((e->inv_rows + kInvSegRows - 1) / kInvSegRows)" in inv
    assert ": 4;" in inv.split("VR_INV_REBUILD_FACTOR")[2].split("\n")[0]  # the rebuild factor's default
    assert "if (h_used >= kPrunedHash * 3 / 4) {" in inv and sp.PRUNED_TABLE_ROWS == 768
    assert "if (n_c + 64 > kPrunedCand) flush();" in inv and sp.PRUNED_FLUSH == 448
    assert "if (n > 0 && ess * 3.0f < all && ess < 0.15f) ne = n;" in inv
    assert "const float want = fmaxf(4.0f * k, 64.0f);" in inv
    assert "(select_regions_kernel<1024, 8>)" in topk and sp.SELECT_KEYS == 8192
    assert "if (n_spill > spill_cap || total > THREADS * ITEMS) {" in topk
    assert sp.SLICE_ROWS == 512 and "const int r0 = tid * 8;" in inv  # a wave's 64 threads x 8 rows
    assert [sp.region_cap(n) for n in (5, 16, 128, 129, 133, 250, 1000)] == [512, 512, 64, 63, 61, 32, 16]


def test_geometries_never_rebuild_and_sample_what_the_cases_need():
    for name, ups in sp.GEOMETRIES.items():
        assert sp.rebuilds(ups) == [], name
    # one row fewer and the 129th segment would have triggered the rebuild; small batches do from the 65th on
    assert sp.rebuilds([1024] * 127 + [1023, 1]) == [129] and sp.rebuilds([8] * 70)[0] == 65
    base, rows = sp.segment_table(sp.GEOMETRIES["s1024"])
    assert base.shape[0] == 128 and set(rows) == {1024} and base[-1] + rows[-1] == 131072
    assert sp.sampled_segments(128) == list(range(0, 128, 8)) + [124, 125, 126, 127]
    base, rows = sp.segment_table(sp.GEOMETRIES["s1021"])
    assert base.shape[0] == 133 and np.count_nonzero(base % 8) == 116 and np.count_nonzero(base % 32) == 128
    assert sp.sampled_segments(133) == list(range(0, 129, 8)) + [129, 130, 131, 132]  # 21: the regular sample ends next to the tail
    base, rows = sp.segment_table(sp.GEOMETRIES["s1row"])
    assert base.shape[0] == 129 and rows[-1] == 1 and sp.sampled_segments(129)[-4:] == [125, 126, 127, 128]
    base, rows = sp.segment_table(sp.GEOMETRIES["p4096"])
    assert rows.tolist() == [4096] * 5
    assert sp.segment_table([4097])[1].tolist() == [2049, 2048]  # equal parts
    # the sample's capacity: one key per 512-row slice of a sampled segment
    assert 20 * (1024 // sp.SLICE_ROWS) == 40 and 21 * 2 == 42


def test_routes():
    assert sp.pick_route(130, 128) == sp.pick_route(17, 133) == sp.pick_route(16, 129) == sp.ROUTE_GROUPED_SAMPLED
    assert sp.pick_route(15, 128) == sp.pick_route(130, 128, grouped_env=False) == sp.ROUTE_SEED_PRUNED
    assert sp.pick_route(130, 128, sample_env=False) == sp.pick_route(26, 6) == sp.pick_route(17, 127) == sp.ROUTE_GROUPED_SEED
    assert sp.pick_route(130, 128, allow_grouped=False) == sp.ROUTE_SEED_PRUNED  # the redo of overflowed queries
    assert sp.pick_route(3, 5, weights_given=True) == sp.pick_route(80, 7, weights_given=True) == sp.ROUTE_FULL
    assert sp.blocks_per_query(12, 5) == (5, 5) and sp.blocks_per_query(12, 5, 1) == (1, 1) and sp.blocks_per_query(130, 128) == (127, 16)


def test_the_edited_pruning_test_reaches_the_per_query_kernels():
    """tests/test_batch_hybrid_gpu.py, fixture `small`: upserts of 7000, 13, 8987 and 4000 rows are 2 + 1 + 3 + 1 = 7 segments;
    test_sparse_batch_pruning_keeps_the_exact_answer sends 80 queries with IDF weights."""
    ups = [7000, 13, 16000 - 7013, 4000]
    assert sp.rebuilds(ups) == [] and sp.segment_table(ups)[0].shape[0] == 7
    # as it was: the grouped scan with seed thresholds, which returns before pruned() and never reads the blocks switch
    assert sp.pick_route(80, 7) == sp.ROUTE_GROUPED_SEED
    # with VR_SPARSE_GROUPED=0: seed, sparse_inv_pruned_kernel<false>, sparse_inv_batch_kernel; one block per query walks
    # all 7 segments (two: 4 and 3 of them), so inv_scan_segments' lists fill and its pruned branch has a threshold
    assert sp.pick_route(80, 7, grouped_env=False) == sp.ROUTE_SEED_PRUNED
    assert sp.blocks_per_query(80, 7, 1) == (1, 1) and sp.blocks_per_query(80, 7, 2) == (2, 2)
    assert [len(sp.share_of_block(7, 2, b)) for b in range(2)] == [4, 3]
    inv = _source("invert.hip")
    grouped_seed = inv.split("case SparseRoute::kGroupedSeed:")[1].split("case SparseRoute::kSeedPruned:")[0]
    assert "if (done) return 0;" in grouped_seed and grouped_seed.index("if (done) return 0;") < grouped_seed.index("pruned()")


# ---- geometry S -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def s_models():
    out = {}
    for name in ("s1024", "s1021", "s1row"):
        off, idx, val, plan = sp.corpus_s(name)
        live, dead, folder = sp.live_rows(off, idx, plan)
        out[name] = (ocore.SparseOracle.from_csr(off, idx, val, live), plan, live, folder)
    return out


def _model(s_models, geo, name, k, mask=None):
    o, plan, live, _ = s_models[geo]
    q = sp.planted_queries()[name]
    return sp.grouped_model(o.scores(*q), live if mask is None else mask, k, plan["seg_base"], plan["seg_rows"])


def test_corpora_keep_their_chosen_document_frequencies(s_models):
    for geo, (o, plan, live, folder) in s_models.items():
        assert o.df[sp.T_ONLY64] == 64 and o.df[sp.T_ONLY65] == 65 and o.df[sp.T_FLOOD] == 49 * 150 and o.df[sp.T_TAIL] == 120
        assert o.df[sp.T_CANCEL_A] == o.df[sp.T_CANCEL_B] == 130       # equal idf: the products cancel to exactly +0.0
        assert o.df[sp.T_TIE] == 70 + 200 - 2 and sp.T_ABSENT not in o.df
        assert o.df[sp.T_LAST] == (1 if geo == "s1row" else 12)
        assert o.n_points == plan["n"] - 42 and (folder == 2).sum() == 5 and (folder == sp.FOLDER_TIE_OUT).sum() == 1


def test_winners_invisible_to_the_sample(s_models):
    """all 64 best rows sit in segments 1..7 (0 and 8 are sampled); the sample sees six weak rows per segment"""
    for geo, cap in (("s1024", 40), ("s1021", 42), ("s1row", 38)):
        o, plan, live, _ = s_models[geo]
        sc = o.scores(*sp.planted_queries()["invisible"])
        best, _ = ocore.topk(sc, 64, live.astype(np.uint8))
        seg = sp.segment_of(best, plan["seg_base"])
        assert set(seg) == set(range(1, 8)) and not set(seg) & set(sp.sampled_segments(plan["n_seg"])), geo
        m = _model(s_models, geo, "invisible", 10)
        assert m["sample_keys"] == cap and not m["redo"] and m["spilled"] == 0
        assert sp.key_score(m["threshold"]) < sc[best[63]]  # the threshold is a weak row's: every winner passes
        assert m["offered"][1:8].min() >= 4 and m["offered"][1:8].sum() >= 64 and m["gathered"] < 200


def test_sample_capacity_decides_whether_there_is_a_threshold(s_models):
    """40 keys at 1024-row segments: k = 40 has a threshold, k = 41 never; 42 at 133 x 1021; 38 where the one-row segment
    takes a tail slot. Without a threshold every touched row is offered."""
    hits = {"s1024": 832, "s1021": 862, "s1row": 832}
    for geo, full_until in (("s1024", 40), ("s1021", 42), ("s1row", 38)):
        for k in (1, 10, 30, 40, 41, 64):
            m = _model(s_models, geo, "invisible", k)
            assert (m["threshold"] != 0) == (k <= full_until), (geo, k)
            assert (m["gathered"] == hits[geo]) == (k > full_until), (geo, k)
    # the riders: at k = 41 most of them are redone on 1024-row segments, none on 1021-row segments (42 >= 41)
    for geo, redone in (("s1024", 90), ("s1021", 0)):
        o, plan, live, _ = s_models[geo]
        qs, at = sp.planted_batch(130, 0, flood=True)
        n = sum(sp.grouped_model(o.scores(*q), live, 41, plan["seg_base"], plan["seg_rows"])["redo"]
                for i, q in enumerate(qs) if 0 < np.unique(q[0]).shape[0] <= 32 and i != at["flood"])
        assert (n > redone) if redone else (n == 0), (geo, n)


def test_terms_of_unsampled_segments_fill_spill_and_overflow(s_models):
    m = _model(s_models, "s1024", "only64", 10)
    assert m["sample_keys"] == 0 and m["threshold"] == 0 and m["offered"].max() == 64 == sp.region_cap(128) and m["spilled"] == 0
    m = _model(s_models, "s1024", "only65", 10)
    assert m["offered"].max() == 65 and m["spilled"] == 1 and m["gathered"] == 65 and not m["redo"]
    assert _model(s_models, "s1021", "only64", 10)["spilled"] == 3 and _model(s_models, "s1row", "only65", 10)["spilled"] == 2
    for geo, spilled in (("s1024", 4214), ("s1021", 4361), ("s1row", 4263)):  # 49 segments x (150 - cap) keys > 4096
        m = _model(s_models, geo, "flood", 10)
        assert m["sample_keys"] == 0 and m["spilled"] == spilled > sp.SPILL and m["gathered"] <= sp.SELECT_KEYS and m["redo"]
    # at k = 10 the flood query is the ONLY query of its batch that is redone
    for geo in ("s1024", "s1row"):
        o, plan, live, _ = s_models[geo]
        qs, at = sp.planted_batch(130, 0, flood=True)
        redo = [i for i, q in enumerate(qs) if 0 < np.unique(q[0]).shape[0] <= 32 and
                sp.grouped_model(o.scores(*q), live, 10, plan["seg_base"], plan["seg_rows"])["redo"]]
        assert redo == [at["flood"]], geo


def test_tail_tie_and_sign_cases(s_models):
    for geo in ("s1024", "s1021", "s1row"):
        o, plan, live, _ = s_models[geo]
        n_seg = plan["n_seg"]
        sc = o.scores(*sp.planted_queries()["tail"])
        assert set(sp.segment_of(np.flatnonzero(sc > -np.inf), plan["seg_base"])) == {n_seg - 4, n_seg - 3, n_seg - 2}
        m = _model(s_models, geo, "tail", 1)
        assert m["sample_keys"] == 6 and m["gathered"] == 1  # the threshold is the best row itself
        sc = o.scores(*sp.planted_queries()["last"])
        assert set(sp.segment_of(np.flatnonzero(sc > -np.inf), plan["seg_base"])) == {n_seg - 1}
        # next to the tail: at k = 3 the threshold is the best row of the first tail segment, below the two rows of n_seg - 5
        sc = o.scores(*sp.planted_queries()["neartail"])
        best, _ = ocore.topk(sc, 3, live.astype(np.uint8))
        assert sp.segment_of(best, plan["seg_base"]).tolist() == [n_seg - 5, n_seg - 5, n_seg - 4] and len({b // 512 for b in best[:2] - plan["seg_base"][n_seg - 5]}) == 2
        m = _model(s_models, geo, "neartail", 3)
        assert m["sample_keys"] == (4 if geo == "s1021" else 2) and (m["threshold"] != 0) == (geo == "s1021")
        assert ((n_seg - 5) in sp.sampled_segments(n_seg)) == (geo == "s1021")
        # the tie group: 14 sample keys, all of them members; at k = 10 the threshold lies INSIDE the group
        tie = plan["tie_rows"]
        sc = o.scores(*sp.planted_queries()["tie"])
        assert np.unique(sc[tie]).shape[0] == 1 and (sc[tie[0]] > np.delete(sc, tie)).all()
        in_sampled = np.isin(sp.segment_of(tie, plan["seg_base"]), sp.sampled_segments(n_seg))
        assert in_sampled.sum() == 35 == (~in_sampled).sum()
        m = _model(s_models, geo, "tie", 10)
        assert m["sample_keys"] == 14 and sp.key_score(m["threshold"]) == sc[tie[0]] and m["gathered"] < 68
        assert _model(s_models, geo, "tie", 64)["threshold"] == 0
        # mixed signs: a negative threshold at k = 30, a threshold of exactly +0.0, an all-negative query without one
        m = _model(s_models, geo, "mixed", 30)
        assert sp.key_score(m["threshold"]) < 0 and m["threshold"] >> 32 < 0x80000000
        m = _model(s_models, geo, "cancel", 10)
        assert m["threshold"] >> 32 == 0x80000000  # +0.0
        sc = o.scores(*sp.planted_queries()["cancel"])
        zero = np.flatnonzero(sc == 0)
        assert np.array_equal(zero, plan["cancel_rows"]) and not np.signbit(sc[zero]).any()
        assert (sc > 0).sum() == 30 and ((sc < 0) & (sc > -np.inf)).sum() == 30  # k = 64 takes 30 positive rows, then 34 of the zeros
        sc = o.scores(*sp.planted_queries()["allneg"])
        assert (sc[sc > -np.inf] < 0).all() and (sc > -np.inf).sum() == 300
        assert _model(s_models, geo, "allneg", 10)["sample_keys"] == 0


def test_long_queries_fill_a_group_to_its_64_terms():
    """Groups hold two queries (kGroup = 2) of at most 32 terms, so a union never EXCEEDS kGrpMaxU = 64 and the host never
    has to close a group early; the edge that exists is a union of exactly 64, one run per lane of the scan block's wave 0
    and none to spare (`pre_of(64)`). group_queries mirrors inv_group_queries: in every batch of the GPU tests long32 and
    long32c (disjoint terms) share a group."""
    pq = sp.planted_queries()
    assert [np.unique(pq[n][0]).shape[0] for n in ("long24", "long32", "long33", "long32c", "long28b")] == [24, 32, 33, 32, 28]
    assert np.unique(pq["long33"][0]).shape[0] > sp.kInvMaxTerms  # served alone on the forward scan, inside the batch
    assert np.intersect1d(pq["long32"][0], pq["long32c"][0]).shape[0] == 0 and 2 * sp.kInvMaxTerms == sp.kGrpMaxU
    assert "static_cast<int>(members.size()) >= G || static_cast<int>(merged.size()) > kGrpMaxU" in _source("invert.hip")
    for nq, shift, flood in ((130, 0, True), (130, 1, True), (130, 0, False), (60, 1, True), (60, 0, False)):
        qs, at = sp.planted_batch(nq, shift, flood)
        groups = sp.group_queries(qs)
        assert ([at["long32"], at["long32c"]], 64) in groups and max(u for _, u in groups) == 64
        assert all(len(m) <= sp.GROUP for m, _ in groups) and at["long33"] not in [i for m, _ in groups for i in m]
    assert np.unique(pq["repeat"][0]).shape[0] == 2 and pq["none"][0].shape[0] == 0


def test_filter_classes(s_models):
    for geo in ("s1024", "s1021"):
        o, plan, live, folder = s_models[geo]
        seg = sp.segment_of(np.arange(plan["n"]), plan["seg_base"])
        samp = sp.sampled_segments(plan["n_seg"])
        assert not np.isin(seg[folder == 1], samp).any() and (folder == 1).sum() > 30000  # a class the sample cannot see
        assert (folder == 2).sum() == 5 < 30                                               # fewer rows than the legs' k
        first = plan["first_rows"]
        assert (folder[first] == 4).all() and np.isin(first, plan["seg_base"]).all()       # first rows of segments
        if geo == "s1021":
            assert np.count_nonzero(first % 32) == first.shape[0] and np.count_nonzero(first % 8) >= 25
        # under the unsampled-only class the invisible query has NO sample key: every passing row it touches is offered
        m = _model(s_models, geo, "invisible", 30, live & (folder == 1))
        assert m["sample_keys"] == 0 and not m["redo"]


# ---- geometry P -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def p_model():
    off, idx, val, plan = sp.corpus_p()
    return (off, idx, val), plan, ocore.SparseOracle.from_csr(off, idx, val)


def _pq(p_model, name, k=10, nq=12, blocks=None):
    csr, plan, o = p_model
    q = sp.p_queries()[name]
    return sp.per_query_model(csr, plan, o, q[0], q[1], k, nq, blocks)


def test_table_overflow_and_mixed_hand_over(p_model):
    csr, plan, o = p_model
    m = _pq(p_model, "table")
    order_ids = m["ids"][m["order"]].tolist()
    assert order_ids == [sp.T_C2, sp.T_EA, sp.T_EB]                      # ascending |weight|
    assert m["seed_ne"] == 2 and m["seed_scored"] == m["seed_named"] == 30  # the seed: T_EB's rows of segments 0 and 4
    assert m["margin"] >= sp.MARGIN and m["seed_margin"] >= sp.MARGIN
    # blocks 0, 1, 2, 4 prune with T_C2 non-essential; block 3 (the huge weight) flags need_full
    assert [(b[2], b[3]) for b in m["blocks"]] == [(1, True), (1, True), (1, True), (0, False), (1, True)]
    assert m["blocks"][3][1] == sp.HUGE and all(b[4] >= sp.MARGIN for b in m["blocks"])
    ess_share = m["frac"][m["order"]][1:].sum()
    assert ess_share < 0.15 / (1 + sp.MARGIN) and ess_share * 3 < m["frac"].sum() / (1 + sp.MARGIN)
    # segment 2: the essential terms name 900 rows > 768; T_EB's postings from the 320th on are passed on unfiltered
    runs = [np.count_nonzero(sp.segment_of(sp.term_postings(*csr, t)[0], plan["seg_base"]) == 2) for t in (sp.T_EA, sp.T_EB)]
    assert runs == [450, 450]
    tabled, direct, first = sp.pruned_wave_walk(runs)
    assert (tabled, direct, first) == (770, 130, [None, 320])
    rb = sp.term_postings(*csr, sp.T_EB)[0]
    rb = rb[sp.segment_of(rb, plan["seg_base"]) == 2]
    ra = sp.term_postings(*csr, sp.T_EA)[0]
    best, _ = ocore.topk(o.scores(*sp.p_queries()["table"]), 10)
    both = np.intersect1d(ra, rb)
    assert both.shape[0] == 4 and np.isin(both, best).all() and np.isin(both, rb[320:]).all()  # named by two terms, scored twice
    only_b = np.setdiff1d(best[sp.segment_of(best, plan["seg_base"]) == 2], both)
    assert only_b.shape[0] >= 2 and np.isin(only_b, rb[320:]).all() and not np.isin(only_b, ra).any()  # named after the table filled
    assert np.count_nonzero(sp.segment_of(best, plan["seg_base"]) == 3) >= 1  # winners in the need_full share as well


def test_buffer_flush(p_model):
    csr, plan, o = p_model
    m = _pq(p_model, "flush")
    assert m["seed_ne"] == 2 and m["margin"] >= sp.MARGIN
    assert [(b[2], b[3]) for b in m["blocks"]] == [(1, True), (1, True), (1, True), (0, False), (1, True)]
    # segment 1: every row the essential terms name reaches theta with room to spare, so the wave buffers 130 rows passed on
    # and 758 table rows: 888 > 448, it flushes mid-segment
    theta = m["theta"]
    sc = o.scores(*sp.p_queries()["flush"])
    ra, va = sp.term_postings(*csr, sp.T_FA)
    rb, vb = sp.term_postings(*csr, sp.T_FB)
    in1 = lambda r: sp.segment_of(r, plan["seg_base"]) == 1
    w = dict(zip(m["ids"].tolist(), m["w"].tolist()))
    assert (np.abs(w[sp.T_FA] * va[in1(ra)]).min() > theta * (1 + sp.MARGIN)) and (np.abs(w[sp.T_FB] * vb[in1(rb)]).min() > theta * (1 + sp.MARGIN))
    tabled, direct, first = sp.pruned_wave_walk([in1(ra).sum(), in1(rb).sum()])
    distinct = np.union1d(ra[in1(ra)], rb[in1(rb)][:first[1]]).shape[0]
    assert direct == 130 and distinct + direct > sp.PRUNED_FLUSH + 64
    best, _ = ocore.topk(sc, 10)
    assert np.isin(best, ra).all() and np.isin(best, rb[in1(rb)][first[1]:]).all()  # the ten best: both terms, scored twice


def test_seed_limits(p_model):
    csr, plan, o = p_model
    m = _pq(p_model, "seed_stops")
    # T_G names 1500 rows of segment 0, the seed wave that owns it stops after 1024 (+ nothing: the run is cut)
    assert m["seed_ne"] == 1 and m["seed_named"] == 1500 + 25 and m["seed_scored"] == sp.kSeedRowsPerWave + 25
    assert m["theta"] is not None and m["margin"] >= sp.MARGIN
    best, _ = ocore.topk(o.scores(*sp.p_queries()["seed_stops"]), 10)
    rg = sp.term_postings(*csr, sp.T_G)[0]
    assert np.isin(best, rg[sp.kSeedRowsPerWave:1500]).all()  # the winners are rows the seed never reached
    m = _pq(p_model, "all_essential")
    assert m["seed_ne"] == 0 and m["seed_margin"] >= sp.MARGIN and m["seed_scored"] == 16 and m["theta"] is not None
    assert all((b[2], b[3]) == (0, False) for b in m["blocks"]) and m["margin"] >= sp.MARGIN  # every term essential: need_full
    m = _pq(p_model, "no_seed")
    assert m["seed_ne"] == 0 and m["seed_scored"] == 0 and m["theta"] is None
    assert all((b[2], b[3]) == (0, False) for b in m["blocks"])  # no threshold: every share goes to the full scan
    # one block per query (VR_SPARSE_BATCH_BLOCKS=1): its vmax is the huge weight's, nothing prunes
    assert all(not b[3] for name in sp.p_queries() for b in _pq(p_model, name, blocks=1)["blocks"])


def test_the_non_essential_bound_decides(p_model):
    csr, plan, o = p_model
    m = _pq(p_model, "ne_bound")
    assert m["ids"][m["order"]].tolist() == [sp.T_C2, sp.T_N]
    # (the seed takes both terms: T_N alone is expected to name too few rows; each of its two waves stops T_C2's run at 1024
    # rows and still gives T_N one round, which holds its 12 seed rows)
    assert m["seed_ne"] == 0 and m["seed_scored"] == 2 * (sp.kSeedRowsPerWave + 12)
    assert m["margin"] >= sp.MARGIN and m["blocks"][2][2:4] == (1, True)
    sc = o.scores(*sp.p_queries()["ne_bound"])
    best, ws = ocore.topk(sc, 10)
    w_n = float(m["w"][m["ids"].tolist().index(sp.T_N)])
    assert m["theta"] == ws[9] == np.float32(w_n) * np.float32(5.0)       # the seed threshold is the final 10th score
    assert np.array_equal(np.sort(best[:6]), plan["lifted"])             # the lifted rows are the six best ...
    assert w_n * 4.9 * (1 + sp.MARGIN) < m["theta"]                        # ... their essential sums alone miss the threshold
    ne_ub = float(m["w"][m["ids"].tolist().index(sp.T_C2)]) * m["blocks"][2][1]
    assert w_n * 4.9 + ne_ub > m["theta"] * (1 + sp.MARGIN)                # ... and reach it with the non-essential bound


def test_survivor_cap_case(p_model):
    """Given weights 1.0 (the marking term) and 0.01 (the ballast), one block walking all segments: after segment 0 wave 0's
    list holds the 40 strong rows, so theta <= 6.01 for k <= 40; in segment 2 the ballast is non-essential and the marked
    rows' partial sums (>= 7.0) all reach theta: 1023, 1024 and 1025 survivors."""
    csr, plan, o = p_model
    vmax = sp.segment_vmax(*csr, plan["seg_base"])
    for t, marked in zip(sp.T_SURV, (1023, 1024, 1025)):
        r, v = sp.term_postings(*csr, t)
        seg = sp.segment_of(r, plan["seg_base"])
        assert (seg == 2).sum() == marked
        head = r[seg == 0]
        assert head.shape[0] == 40 and ((head - plan["seg_base"][0]) % 256 < 64).all() and np.unique(head % 256).shape[0] == 40
        theta_max = float(v[seg <= 1].max()) * 1.0 + 0.01 * 1.0
        assert 0.01 * float(vmax[2]) * (1 + sp.MARGIN) < v[seg == 0].min()     # the ballast is non-essential ...
        assert 1.01 * float(vmax[2]) > theta_max * (1 + sp.MARGIN)              # ... the marking term is not
        assert v[seg == 2].min() > theta_max * (1 + sp.MARGIN)                  # every marked row survives
        assert 1.0 * 1.5 < 2.0                                                  # ess * 1.5 < all with every t_frac = 1
    assert sp.pick_route(3, 5, weights_given=True) == sp.ROUTE_FULL


def test_run_search_corpus():
    off, idx, val, plan = sp.corpus_r()
    row_of = np.repeat(np.arange(plan["n"]), np.diff(off))
    counts = np.bincount(sp.segment_of(row_of, plan["seg_base"]))
    assert counts.tolist() == [1, 64, 65, 4096, 64 * 4096 + 1155, 4097] and counts[4] > 64 ** 3
    deep = idx[sp.segment_of(row_of, plan["seg_base"]) == 4]
    assert deep.min() == 900 and deep.max() == 2000
    for t, m in sp.R_RUNS:
        assert np.count_nonzero(deep == t) == m
    assert [m for _, m in sp.R_RUNS] == [1, 64, 65, 256, 257, 512]
    assert not np.isin(sp.R_ABSENT, idx).any() and min(sp.R_ABSENT) < idx.min() and max(sp.R_ABSENT) > idx.max()
    assert sp.seed_segments(6, 6) == {(0, 0): [0], (1, 0): [4]}  # the seed pass walks the deep segment
