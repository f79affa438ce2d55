"""No-GPU checks of MMR diversification: hand-worked known answers for the oracle (tests/mmr_oracle.py),
the ctypes declaration of vr_mmr_select against the header, argument errors before the engine is touched, and the
service wiring (VectorStoreService.search / search_many / search_requests with mmr_* arguments and settings) over an
engine whose arithmetic is the CPU oracle: pool sizes, relevance per path, order and score transport, the settings
fallback, mixed batches, and a stale answer that makes the search look again."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mmr_oracle as mo  # noqa: E402
from oracle import core as ocore  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- known answers ----------------------------------------------------------------------------------------------------
# Unit vectors in 3-D (exactly representable sims): a = e0, a2 = a (exact duplicate), b = e1, c = (e0 + e1)/|.|, d = e2
E0, E1, E2 = np.eye(3, dtype=np.float32)
C01 = (E0 + E1) / np.float32(np.sqrt(2.0))
ROWS = np.stack([E0, E0, E1, C01, E2]).astype(np.float32)  # positions 0..4: a, a2, b, c, d


def _sim():
    return mo.gram(ROWS)


def test_gram_is_the_dense_score():
    s = _sim()
    assert s[0, 1] == 1.0 and s[0, 2] == 0.0 and s[0, 4] == 0.0 and s[2, 4] == 0.0
    assert s[0, 3] == s[3, 0] == ocore.dense_scores(ROWS[:1], ROWS[3:4])[0, 0]
    assert np.array_equal(s, s.T)


def test_diversity_zero_is_the_prefix():
    rel = [0.9, 0.8, 0.7, 0.6, 0.5]
    assert mo.select(_sim(), rel, 0.0, 3) == [0, 1, 2]
    assert mo.select(_sim(), rel, 0.0, 5) == [0, 1, 2, 3, 4]


def test_diversity_one_ignores_relevance_after_the_first_pick():
    # step 1: (1 - 1) * rel = 0 for all -> position 0. Then -max sim: a2 has 1, c has 0.707, b and d 0 -> b (lower)
    # then vs {a, b}: a2 1, c 0.707, d 0 -> d; then c (0.707) before a2 (1)
    rel = [0.1, 0.9, 0.8, 0.7, 0.2]
    assert mo.select(_sim(), rel, 1.0, 5) == [0, 2, 4, 3, 1]


def test_half_diversity_skips_the_duplicate():
    # d = 0.5: step 1 picks a (0.45). Then 0.5 rel - 0.5 m: a2 0.425 - 0.5 = -0.075, b 0.4 - 0 = 0.4, c 0.35 - 0.354,
    # d 0.3 - 0 = 0.3 -> b; then m(c) = 0.707 still: c -0.004, a2 -0.075, d 0.3 -> d; then c, then a2
    rel = [0.9, 0.85, 0.8, 0.7, 0.6]
    assert mo.select(_sim(), rel, 0.5, 5) == [0, 2, 4, 3, 1]


def test_equal_relevance_and_duplicate_rows_tie_to_the_lower_position():
    rel = [0.5] * 5
    assert mo.select(_sim(), rel, 0.0, 5) == [0, 1, 2, 3, 4]
    # a and a2 are the same vector: equal similarity to everything; after a, with d = 0.3 b and d tie (0.35) -> b first
    assert mo.select(_sim(), rel, 0.3, 5) == [0, 2, 4, 3, 1]
    rel2 = [0.5, 0.5, 0.1, 0.1, 0.1]
    # the duplicate pair with equal relevance: position 0 first; a2 is then penalised by sim 1
    assert mo.select(_sim(), rel2, 0.5, 2) == [0, 2]


def test_limit_beyond_the_list():
    assert mo.select(_sim(), [0.9, 0.8, 0.7, 0.6, 0.5], 0.5, 50) == [0, 2, 4, 3, 1]
    assert mo.select(_sim(), [0.9, 0.8, 0.7, 0.6, 0.5], 0.5, 0) == []
    assert mo.select(np.zeros((0, 0), np.float32), [], 0.5, 3) == []


# ---- the C-ABI --------------------------------------------------------------------------------------------------------
def _header_params(name):
    src = open(os.path.join(ROOT, "include", "voitta_engine.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
    assert m, name
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


def test_ctypes_declaration_follows_the_header():
    from voitta_rag_amd import _lib

    lib = _lib.load_library()
    assert hasattr(lib, "vr_mmr_select")
    params = _header_params("vr_mmr_select")
    restype, argtypes = _lib.SIGNATURES["vr_mmr_select"]
    assert restype is C.c_int and len(argtypes) == len(params) == 11
    base = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}
    for p, a in zip(params, argtypes):
        if p.startswith("vr_engine"):
            assert a is C.c_void_p
            continue
        t = p.rsplit(" ", 1)[0].replace("const ", "").replace("*", "").strip()
        assert a == (C.POINTER(base[t]) if "*" in p else base[t]), (p, a)
    assert _lib.VR_STALE_GENERATION == 1
    hdr = open(os.path.join(ROOT, "include", "voitta_engine.h")).read()
    assert re.search(r"#define VR_STALE_GENERATION 1\b", hdr)


def test_null_engine_is_refused():
    from voitta_rag_amd import _lib

    lib = _lib.load_library()
    z = np.zeros(4, np.int64)
    assert lib.vr_mmr_select(None, 0, z.ctypes.data_as(C.POINTER(C.c_int64)), None, None, None, None, 0, 0, None,
                             None) < 0
    assert lib.vr_last_error().decode() == "null engine"


# ---- service wiring over the oracle engine ----------------------------------------------------------------------------
class MmrOracleEngine:
    """OracleEngine plus what the MMR paths call: generation, the filtered batches and mmr_select (the oracle's
    selection); records every mmr_select call, and answers `stale` of them as a renumbered index would."""

    def __new__(cls, dim):
        from oracle_engine import OracleEngine

        class _E(OracleEngine):
            def __init__(self, dim):
                super().__init__(dim)
                self.gen = 3
                self.calls = []
                self.stale = 0

            def generation(self):
                return self.gen

            def search_dense_multi(self, queries, k, filters, raw=False):
                q = np.asarray(queries, np.float32).reshape(-1, self.dim)
                rows = np.full((len(q), k), -1, np.int64)
                scores = np.zeros((len(q), k), np.float32)
                counts = np.zeros(len(q), np.int32)
                for i in range(len(q)):
                    r, s = self.search_dense(q[i:i + 1], k, filters[i])[0]
                    rows[i, : len(r)], scores[i, : len(r)], counts[i] = r, s, len(r)
                return rows, scores, counts

            def search_hybrid_batch_multi(self, queries, sparse_queries, limits, weights, filters, raw=False):
                n, k = len(limits), max(limits)
                rows = np.full((n, k), -1, np.int64)
                scores = np.zeros((n, k))
                fd = np.zeros((n, k), np.int32)
                counts = np.zeros(n, np.int32)
                for i in range(n):
                    r, s, f = self.search_hybrid(queries[i], sparse_queries[i][0], sparse_queries[i][1], limits[i],
                                                 weights[i], flt=filters[i])
                    rows[i, : len(r)], scores[i, : len(r)], fd[i, : len(r)], counts[i] = r, s, f, len(r)
                return rows, scores, fd, counts

            def mmr_select(self, rows_lists, relevance_lists, diversities, limits, generation):
                self.calls.append(([np.asarray(r).tolist() for r in rows_lists],
                                   [np.asarray(v, np.float64).tolist() for v in relevance_lists],
                                   list(diversities), list(limits), generation))
                if self.stale > 0 or generation != self.gen:
                    self.stale -= 1
                    return None
                return [np.asarray(mo.select_rows(self.x, r, v, d, lim), np.int32)
                        for r, v, d, lim in zip(rows_lists, relevance_lists, diversities, limits)]

        return _E(dim)


DIM = 16


@pytest.fixture
def store(monkeypatch):
    from voitta_rag_amd import config, store_registry
    from voitta_rag_amd.vector_store import ChunkMetadata, VectorStoreService

    for k in ("VOITTA_MMR_DIVERSITY", "VOITTA_MMR_CANDIDATES", "VOITTA_RERANK_MODEL"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("EMBEDDING_DIMENSION", str(DIM))
    config.get_settings.cache_clear()
    eng = MmrOracleEngine(DIM)
    store_registry.set_engine(eng)
    rng = np.random.default_rng(1)
    base = rng.standard_normal((12, DIM)).astype(np.float32)
    chunks, sparse = [], []
    for i in range(60):  # 12 topics, 5 near-copies each
        v = base[i % 12] + np.float32(0.05) * rng.standard_normal(DIM).astype(np.float32)
        meta = ChunkMetadata(file_path=f"f{i % 3}.md", folder_path=f"d{i % 2}", index_folder="ix", file_name="f",
                             chunk_index=i, total_chunks=60, start_char=0, end_char=1, indexed_at="t")
        chunks.append((f"chunk {i}", v.tolist(), meta))
        sparse.append(([int(i % 7), 10 + int(i % 5)], [1.0, 0.5]))
    vs = VectorStoreService()
    vs.store_chunks(chunks, sparse_vectors=sparse)
    yield vs, eng, base
    store_registry.set_engine(None)
    config.get_settings.cache_clear()


def _ids(res):
    return [c.id for c in res]


def test_search_without_mmr_is_unchanged_and_calls_nothing(store):
    vs, eng, base = store
    q = base[0].tolist()
    plain = vs.search(q, limit=5)
    assert eng.calls == []
    assert len(plain) == 5
    assert vs.search(q, limit=0, mmr_diversity=0.5) == [] and eng.calls == []


def test_dense_search_pool_relevance_and_order(store):
    from voitta_rag_amd.vector_store import _json_float

    vs, eng, base = store
    q = base[0].tolist()
    pool = vs.search(q, limit=20)
    got = vs.search(q, limit=5, mmr_diversity=0.5, mmr_candidates=20)
    rows, rels, divs, lims, gen = eng.calls[-1]
    assert len(rows[0]) == 20 and divs == [0.5] and lims == [5] and gen == eng.gen
    qh = ocore.cosine_preprocess(np.asarray([q], np.float32))
    want_rows, want_scores = ocore.topk(ocore.dense_scores(qh, eng.x)[0], 20, eng.live.astype(np.uint8))
    assert rows[0] == want_rows.tolist()
    assert rels[0] == [float(np.float32(s)) for s in want_scores]  # the f32 score widened
    pos = mo.select_rows(eng.x, want_rows, want_scores.astype(np.float64), 0.5, 5)
    assert _ids(got) == [_ids(pool)[i] for i in pos]
    assert [c.score for c in got] == [_json_float(want_scores[i]) for i in pos]  # the first stage's transport
    assert len({c.id for c in got}) == 5


def test_hybrid_search_relevance_is_the_fused_score(store):
    vs, eng, base = store
    q = base[1].tolist()
    sp = ([1, 11], [1.0, 1.0])
    pool = vs.search(q, limit=30, sparse_query=sp)
    got = vs.search(q, limit=6, sparse_query=sp, mmr_diversity=0.3, mmr_candidates=30)
    rows, rels, _, lims, _ = eng.calls[-1]
    assert len(rows[0]) == 30 and lims == [6]
    assert rels[0] == [c.score for c in pool]  # the fused f64 as transported
    pos = mo.select_rows(eng.x, rows[0], rels[0], 0.3, 6)
    assert [(c.id, c.score) for c in got] == [(pool[i].id, pool[i].score) for i in pos]


def test_settings_fallback_and_candidate_clamp(store, monkeypatch):
    from voitta_rag_amd import config

    vs, eng, base = store
    monkeypatch.setenv("VOITTA_MMR_DIVERSITY", "0.4")
    monkeypatch.setenv("VOITTA_MMR_CANDIDATES", "7")
    config.get_settings.cache_clear()
    vs.search(base[2].tolist(), limit=10)
    rows, _, divs, lims, _ = eng.calls[-1]
    assert divs == [0.4] and lims == [10] and len(rows[0]) == 10  # candidates clamped up to the limit
    vs.search(base[2].tolist(), limit=3)
    assert len(eng.calls[-1][0][0]) == 7
    vs.search(base[2].tolist(), limit=3, mmr_candidates=1000)
    assert len(eng.calls[-1][0][0]) == 60  # clamped to 341, the corpus holds 60
    monkeypatch.setenv("VOITTA_MMR_CANDIDATES", "50")
    config.get_settings.cache_clear()
    vs.search(base[2].tolist(), limit=3, mmr_diversity=0.9)
    assert eng.calls[-1][2] == [0.9] and len(eng.calls[-1][0][0]) == 50  # the argument wins over the setting
    with pytest.raises(ValueError):
        vs.search(base[2].tolist(), limit=3, mmr_diversity=1.5)


def test_diversity_zero_equals_the_plain_search(store):
    vs, eng, base = store
    for sp in (None, ([2, 12], [1.0, 0.5])):
        plain = vs.search(base[3].tolist(), limit=8, sparse_query=sp)
        got = vs.search(base[3].tolist(), limit=8, sparse_query=sp, mmr_diversity=0.0)
        assert [(c.id, c.score) for c in got] == [(c.id, c.score) for c in plain]


def test_search_requests_mixed_batch(store):
    vs, eng, base = store
    reqs = [dict(query_embedding=base[0].tolist(), limit=5),
            dict(query_embedding=base[1].tolist(), limit=4, mmr_diversity=0.5, mmr_candidates=25),
            dict(query_embedding=base[2].tolist(), limit=5, sparse_query=([3], [1.0]), folder_filter="d1"),
            dict(query_embedding=base[3].tolist(), limit=6, sparse_query=([4, 14], [1.0, 1.0]), mmr_diversity=0.7),
            dict(query_embedding=base[4].tolist(), limit=0, mmr_diversity=0.5)]
    plain = [vs.search(**{k: v for k, v in r.items()}) for r in reqs]
    n0 = len(eng.calls)
    got = vs.search_requests(reqs)
    assert len(eng.calls) == n0 + 1  # one call serves every MMR request
    rows, rels, divs, lims, _ = eng.calls[-1]
    assert divs == [0.5, 0.7] and lims == [4, 6] and [len(r) for r in rows] == [25, 50]
    for i in (0, 2, 4):  # requests without MMR keep their results
        assert [(c.id, c.score) for c in got[i]] == [(c.id, c.score) for c in plain[i]]
    for i in (1, 3):
        assert [(c.id, c.score) for c in got[i]] == [(c.id, c.score) for c in plain[i]]
    assert got[4] == []


def test_search_many_one_call(store):
    vs, eng, base = store
    q = base[:3]
    sq = [None, ([5], [1.0]), ([6, 16], [1.0, 1.0])]
    n0 = len(eng.calls)
    got = vs.search_many(q, limit=4, sparse_queries=sq, mmr_diversity=0.5, mmr_candidates=12)
    assert len(eng.calls) == n0 + 1
    for i in range(3):
        want = vs.search(q[i].tolist(), limit=4, sparse_query=sq[i], mmr_diversity=0.5, mmr_candidates=12)
        assert [(c.id, c.score) for c in got[i]] == [(c.id, c.score) for c in want]


def test_stale_answer_searches_again(store):
    vs, eng, base = store
    want = vs.search(base[5].tolist(), limit=5, mmr_diversity=0.5)
    eng.stale = 1
    n0 = len(eng.calls)
    got = vs.search(base[5].tolist(), limit=5, mmr_diversity=0.5)
    assert len(eng.calls) == n0 + 2  # the stale answer, then the first stage and the selection again
    assert [(c.id, c.score) for c in got] == [(c.id, c.score) for c in want]
    eng.stale = 1
    got = vs.search_requests([dict(query_embedding=base[5].tolist(), limit=5, mmr_diversity=0.5)])[0]
    assert [(c.id, c.score) for c in got] == [(c.id, c.score) for c in want]


def test_sharded_store_refuses_mmr_arguments():
    from voitta_rag_amd.sharded import ShardedVectorStore

    with pytest.raises(TypeError):
        ShardedVectorStore.search(object(), [0.0], limit=3, mmr_diversity=0.5)


def test_rrf_relevance_is_refused():
    from voitta_rag_amd.engine import VR_FUSION_RRF, Engine

    e = Engine.__new__(Engine)  # (no device needed: refused before the engine is called)
    with pytest.raises(ValueError, match="RRF"):
        e.mmr_select([[0]], [[1.0]], [0.5], [1], 0, fusion=VR_FUSION_RRF)


# ---- the reranked path over a stand-in cross-encoder ------------------------------------------------------------------
class _FakeReranker:
    """logits(questions, candidates) as the cross-encoder answers them, from the passage text alone (so that the batch's
    composition does not matter); records every call. Equal logits occur: the first stage's order must then decide."""

    def __init__(self):
        self.calls = []

    def logits(self, questions, candidates):
        self.calls.append((list(questions), [list(c) for c in candidates]))
        return [np.asarray([(int(t.split()[1]) * 7 % 13) * 0.375 - 2.0 for t in cands], np.float32) for cands in candidates]


class _Question(list):
    """A query vector that carries its question's text (what embed_query's result does)."""

    def __init__(self, vec, question):
        super().__init__(vec)
        self.question = question


@pytest.fixture
def reranked(store, monkeypatch):
    vs, eng, base = store
    rr = _FakeReranker()
    monkeypatch.setattr(vs, "_reranker", lambda: rr)
    return vs, eng, base, rr


def _pool(vs, eng, vec, n):
    rr = vs._reranker
    vs._reranker = lambda: None
    try:
        return vs.search(list(vec), limit=n)
    finally:
        vs._reranker = rr


def _rows_of(vs, chunks):
    return np.asarray([vs._col.row_of[c.id] for c in chunks], np.int64)


def test_reranked_search_without_mmr_is_unchanged(reranked):
    from voitta_rag_amd.vector_store import VectorStoreService

    vs, eng, base, rr = reranked
    pool = _pool(vs, eng, base[0], 50)  # VOITTA_RERANK_CANDIDATES: 50
    got = vs.search(_Question(base[0].tolist(), "q0"), limit=5)
    assert rr.calls[-1] == (["q0"], [[c.text for c in pool]]) and eng.calls == []
    want = VectorStoreService._rerank_order([pool], rr.logits(["q0"], [[c.text for c in pool]]), [5])[0]
    assert [(c.id, c.score) for c in got] == [(c.id, c.score) for c in want]


def test_reranked_search_with_mmr_selects_from_the_whole_reranked_pool(reranked):
    from voitta_rag_amd.reranker import sigmoid

    vs, eng, base, rr = reranked
    pool = _pool(vs, eng, base[1], 50)
    got = vs.search(_Question(base[1].tolist(), "q1"), limit=6, mmr_diversity=0.5, mmr_candidates=8)
    assert rr.calls[-1][1] == [[c.text for c in pool]]  # the rerank pool, not mmr_candidates, and every one rescored
    rows, rels, divs, lims, gen = eng.calls[-1]
    rel = sigmoid(rr.logits(["q1"], [[c.text for c in pool]])[0]).astype(np.float64)
    assert rows == [_rows_of(vs, pool).tolist()] and rels == [rel.tolist()] and divs == [0.5] and lims == [6]
    pos = mo.select_rows(eng.x, _rows_of(vs, pool), rel, 0.5, 6)
    assert [(c.id, c.score) for c in got] == [(pool[i].id, float(rel[i])) for i in pos]
    # d = 0: the reranked order itself
    plain = vs.search(_Question(base[1].tolist(), "q1"), limit=6)
    zero = vs.search(_Question(base[1].tolist(), "q1"), limit=6, mmr_diversity=0.0)
    assert [(c.id, c.score) for c in zero] == [(c.id, c.score) for c in plain]


def test_reranked_questions_mixed_batch(reranked, monkeypatch):
    from voitta_rag_amd.reranker import sigmoid
    from voitta_rag_amd.vector_store import VectorStoreService

    vs, eng, base, rr = reranked
    pools = {f"q{i}": _pool(vs, eng, base[i], 50) for i in range(3)}
    seen = []

    def first_stage(requests):
        seen.append(requests)
        return [pools[r["query"]][: r["limit"]] for r in requests]

    monkeypatch.setattr(vs, "_search_questions_first_stage", first_stage)
    reqs = [{"query": "q0", "limit": 5}, {"query": "q1", "limit": 4, "mmr_diversity": 0.6},
            {"query": "q2", "limit": 7, "folder_filter": None}]
    got = vs.search_questions(reqs)
    assert [r["limit"] for r in seen[-1]] == [50, 50, 50]
    assert all("mmr_diversity" not in r and "mmr_candidates" not in r for r in seen[-1])
    texts = [[c.text for c in pools[q]] for q in ("q0", "q1", "q2")]
    assert rr.calls[-1] == (["q0", "q1", "q2"], texts)  # one rerank call for every question
    logits = rr.logits(["q0", "q1", "q2"], texts)
    want = VectorStoreService._rerank_order([pools["q0"], pools["q2"]], [logits[0], logits[2]], [5, 7])
    assert [(c.id, c.score) for c in got[0]] == [(c.id, c.score) for c in want[0]]
    assert [(c.id, c.score) for c in got[2]] == [(c.id, c.score) for c in want[1]]
    rows, rels, divs, lims, _ = eng.calls[-1]
    rel = sigmoid(logits[1]).astype(np.float64)
    assert len(rows) == 1 and rels == [rel.tolist()] and divs == [0.6] and lims == [4]
    pos = mo.select_rows(eng.x, _rows_of(vs, pools["q1"]), rel, 0.6, 4)
    assert [(c.id, c.score) for c in got[1]] == [(pools["q1"][i].id, float(rel[i])) for i in pos]
    # without any MMR request: the reranked batch exactly as before (no selection call)
    n0 = len(eng.calls)
    got2 = vs.search_questions([{"query": "q0", "limit": 5}, {"query": "q2", "limit": 7}])
    assert len(eng.calls) == n0
    assert [[(c.id, c.score) for c in g] for g in got2] == [[(c.id, c.score) for c in w] for w in want]


def test_reranked_stale_answer_looks_again(reranked):
    vs, eng, base, rr = reranked
    want = vs.search(_Question(base[2].tolist(), "q2"), limit=5, mmr_diversity=0.5)
    eng.stale = 1
    n0 = len(eng.calls)
    got = vs.search(_Question(base[2].tolist(), "q2"), limit=5, mmr_diversity=0.5)
    assert len(eng.calls) == n0 + 2
    assert [(c.id, c.score) for c in got] == [(c.id, c.score) for c in want]


def test_reranked_pool_drops_candidates_deleted_since_the_first_stage(reranked, monkeypatch):
    from voitta_rag_amd.reranker import sigmoid

    vs, eng, base, rr = reranked
    pool = _pool(vs, eng, base[3], 50)
    gone = pool[1]
    real = rr.logits

    def logits_then_delete(questions, candidates):  # a delete lands between the rerank and the selection
        out = real(questions, candidates)
        with vs._col.lock:
            vs._col.row_of.pop(gone.id)
        return out

    monkeypatch.setattr(rr, "logits", logits_then_delete)
    got = vs.search(_Question(base[3].tolist(), "q3"), limit=6, mmr_diversity=0.5)
    keep = [c for c in pool if c.id != gone.id]
    rel = sigmoid(real(["q3"], [[c.text for c in keep]])[0]).astype(np.float64)
    assert eng.calls[-1][1] == [rel.tolist()]
    pos = mo.select_rows(eng.x, _rows_of(vs, keep), rel, 0.5, 6)
    assert [c.id for c in got] == [keep[i].id for i in pos] and gone.id not in {c.id for c in got}
