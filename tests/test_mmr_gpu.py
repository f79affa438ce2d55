"""MMR diversification on the GPU (vr_mmr_select, Engine.mmr_select and the mmr_* arguments of VectorStoreService):
positions and counts bit for bit against the NumPy oracle (tests/mmr_oracle.py) over list lengths around the 16-row tile,
both model widths, several diversities, duplicate rows and batches split into workspace slices; d = 0 leaves every search
as it was; the service paths (dense, hybrid, from text, batched, questions, reranked) equal the oracle's MMR over their
own first stage; the stale-generation answer and the argument errors."""
import ctypes as C

import numpy as np
import pytest

from oracle import core as ocore

import mmr_oracle as mo

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _device(gpu):
    """Every test here asks for the device the way the suite does (conftest's session fixture), before any engine opens it."""
    return gpu

LENGTHS = [1, 2, 15, 16, 17, 63, 100, 341, 1024]
DIVERSITIES = [0.0, 0.3, 0.5, 1.0]


def _corpus(n, dim, seed):
    """Random rows plus near-duplicate clusters (a base row and small perturbations of it) and exact duplicate rows."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    for c in range(min(20, (n - 40) // 50)):  # clusters of 8 near-copies
        base = x[c * 50]
        for j in range(1, 8):
            x[c * 50 + j] = base + np.float32(0.02) * rng.standard_normal(dim).astype(np.float32)
    x[n - 40: n - 20] = x[n - 20:]  # exact duplicates: rows n-40+i and n-20+i are the same vector
    return x


def _engine(x):
    from voitta_rag_amd import Engine

    e = Engine(x.shape[1])
    e.upsert(x)
    return e


def _lists(rng, n, lengths, cluster_rows=True):
    out = []
    for k in lengths:
        pool = rng.choice(n, size=k, replace=False)
        if cluster_rows and k >= 16:  # a cluster and a pair of exact duplicates inside the list
            pool[:8] = np.arange(8) + 50 * int(rng.integers(0, 20))
            pool[8:10] = [n - 40 + 3, n - 20 + 3]
            pool = np.unique(pool)
            rng.shuffle(pool)
            while pool.size < k:
                extra = rng.choice(n, size=k - pool.size, replace=False)
                pool = np.unique(np.concatenate([pool, extra]))
            pool = pool[:k]
        rel = np.sort(rng.random(k))[::-1].astype(np.float64)
        if k >= 4:
            rel[1] = rel[2]  # equal relevance: the position decides
        out.append((pool.astype(np.int64), rel))
    return out


def _check(e, stored, lists, divs, limits):
    got = e.mmr_select([r for r, _ in lists], [v for _, v in lists], divs, limits, e.generation())
    assert got is not None
    for (rows, rel), d, lim, g in zip(lists, divs, limits, got):
        want = mo.select_rows(stored, rows, rel, d, lim)
        assert g.tolist() == want, (len(rows), d, lim)


@pytest.mark.parametrize("dim", [384, 768])
def test_mmr_select_matches_oracle(dim):
    n = 3000
    x = _corpus(n, dim, dim)
    stored = ocore.cosine_preprocess(x)
    e = _engine(x)
    try:
        rng = np.random.default_rng(7 + dim)
        for d in DIVERSITIES:
            lists = _lists(rng, n, LENGTHS)
            limits = [min(k, 20) for k in LENGTHS[:-2]] + [341, 1024]
            _check(e, stored, lists, [d] * len(lists), limits)
        # one call holding lists of mixed lengths, limits and diversities (limit > K, limit 0 and empty lists among them)
        lengths = [17, 0, 100, 1, 63, 1024, 16, 5]
        lists = _lists(rng, n, lengths)
        divs = [0.5, 0.3, 1.0, 0.0, 0.7, 0.25, 0.5, 0.9]
        limits = [30, 4, 20, 3, 0, 50, 16, 5]
        _check(e, stored, lists, divs, limits)
    finally:
        e.close()


def test_mmr_select_workspace_slices(monkeypatch):
    """A batch above the workspace budget runs in slices; the answer is the same."""
    n, dim = 3000, 768
    x = _corpus(n, dim, 11)
    stored = ocore.cosine_preprocess(x)
    e = _engine(x)
    try:
        rng = np.random.default_rng(3)
        lengths = [50] * 40 + [1024, 341, 17]
        lists = _lists(rng, n, lengths)
        divs = list(rng.choice(DIVERSITIES, size=len(lists)))
        limits = [20] * len(lists)
        full = e.mmr_select([r for r, _ in lists], [v for _, v in lists], divs, limits, e.generation())
        monkeypatch.setenv("VR_MMR_WORKSPACE_MB", "1")  # (64 x 768 x 4 + 64^2 x 4 bytes per list of 50: four per slice)
        sliced = e.mmr_select([r for r, _ in lists], [v for _, v in lists], divs, limits, e.generation())
        assert [a.tolist() for a in sliced] == [a.tolist() for a in full]
        _check(e, stored, lists, divs, limits)
    finally:
        e.close()


def test_mmr_select_tombstoned_rows_and_duplicates():
    """Tombstoned rows keep their vectors until compaction: they may be candidates. Exact duplicate rows have equal
    similarities to everything; with equal relevance the lower position wins."""
    n, dim = 200, 384
    x = _corpus(n, dim, 5)
    stored = ocore.cosine_preprocess(x)
    e = _engine(x)
    try:
        e.delete_rows(np.arange(0, n, 3))
        rows = np.asarray([n - 20 + 3, n - 40 + 3, 0, 3, 50, 51, 7], np.int64)
        rel = np.asarray([0.9, 0.9, 0.8, 0.8, 0.7, 0.7, 0.1])
        for d in DIVERSITIES:
            got = e.mmr_select([rows], [rel], [d], [7], e.generation())[0]
            assert got.tolist() == mo.select_rows(stored, rows, rel, d, 7)
    finally:
        e.close()


def _raw(e, off, rows, rel, div, lim, gen, stride=None):
    from voitta_rag_amd import _lib

    lib = _lib.load_library()
    n = len(div)
    off = np.ascontiguousarray(off, np.int64)
    rows = np.ascontiguousarray(rows, np.int64)
    rel = np.ascontiguousarray(rel, np.float64)
    div = np.ascontiguousarray(div, np.float64)
    lim = np.ascontiguousarray(lim, np.int32)
    stride = int(stride if stride is not None else max(1, int(lim.max()) if n else 1))
    pos = np.full((max(n, 1), stride), -7, np.int32)
    cnt = np.full(max(n, 1), -7, np.int32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    rc = lib.vr_mmr_select(e.handle, n, p(off, C.c_int64), p(rows, C.c_int64), p(rel, C.c_double), p(div, C.c_double),
                           p(lim, C.c_int32), int(gen), stride, p(pos, C.c_int32), p(cnt, C.c_int32))
    return rc, pos, cnt, lib.vr_last_error().decode()


def test_mmr_select_stale_generation_writes_nothing():
    from voitta_rag_amd import _lib

    n, dim = 100, 384
    e = _engine(_corpus(n, dim, 9))
    try:
        g0 = e.generation()
        e.delete_rows([1, 2, 3])
        e.compact()
        assert e.generation() != g0
        rc, pos, cnt, _ = _raw(e, [0, 3], [0, 4, 5], [0.9, 0.5, 0.1], [0.5], [2], g0)
        assert rc == _lib.VR_STALE_GENERATION == 1
        assert (pos == -7).all() and (cnt == -7).all()
        assert e.mmr_select([[0, 4, 5]], [[0.9, 0.5, 0.1]], [0.5], [2], g0) is None
        rc, pos, cnt, _ = _raw(e, [0, 3], [0, 4, 5], [0.9, 0.5, 0.1], [0.5], [2], e.generation())
        assert rc == 0 and cnt[0] == 2
    finally:
        e.close()


def test_mmr_select_argument_errors():
    n, dim = 100, 384
    e = _engine(_corpus(n, dim, 13))
    g = e.generation()
    try:
        ok = ([0, 3], [0, 4, 5], [0.9, 0.5, 0.1], [0.5], [2])
        assert _raw(e, *ok, g)[0] == 0
        cases = {
            "list_off[0]": ([1, 3], [0, 4, 5], [0.9, 0.5, 0.1], [0.5], [2]),
            "decreases": ([0, 3, 2], [0, 4, 5], [0.9, 0.5, 0.1], [0.5, 0.5], [2, 2]),
            "diversity": ([0, 3], [0, 4, 5], [0.9, 0.5, 0.1], [1.5], [2]),
            "diversity -": ([0, 3], [0, 4, 5], [0.9, 0.5, 0.1], [-0.1], [2]),
            "out of range": ([0, 3], [0, 4, n], [0.9, 0.5, 0.1], [0.5], [2]),
            "negative row": ([0, 3], [0, -1, 5], [0.9, 0.5, 0.1], [0.5], [2]),
            "limit": ([0, 3], [0, 4, 5], [0.9, 0.5, 0.1], [0.5], [-1]),
            "too long": ([0, 1025], np.arange(1025) % n, np.ones(1025), [0.5], [2]),
        }
        for name, args in cases.items():
            rc, pos, cnt, msg = _raw(e, *args, g)
            assert rc < 0 and msg, name
            assert (cnt == -7).all(), name
        assert _raw(e, [0, 3], [0, 4, 5], [0.9, 0.5, 0.1], [0.5], [4], g, stride=2)[0] < 0  # stride below a limit
        assert _raw(e, [0], [], [], [], [], g)[0] == 0  # no lists: nothing to do
        rc, pos, cnt, _ = _raw(e, [0, 3], [0, 4, 5], [0.9, 0.5, 0.1], [0.5], [0], g)
        assert rc == 0 and cnt[0] == 0
    finally:
        e.close()


# ---- the services on the device engine --------------------------------------------------------------------------------
SDIM = 384


@pytest.fixture
def service(monkeypatch):
    """60 topics x 6 near-copies (one chunk re-indexed under several paths, overlapping chunks) plus 200 random rows."""
    from voitta_rag_amd import Engine, config, store_registry
    from voitta_rag_amd.vector_store import ChunkMetadata, VectorStoreService

    for k in ("VOITTA_MMR_DIVERSITY", "VOITTA_MMR_CANDIDATES", "VOITTA_RERANK_MODEL"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("EMBEDDING_DIMENSION", str(SDIM))
    config.get_settings.cache_clear()
    eng = Engine(SDIM)
    store_registry.set_engine(eng)
    rng = np.random.default_rng(21)
    topics = rng.standard_normal((60, SDIM)).astype(np.float32)
    vecs = [topics[t] + np.float32(0.03) * rng.standard_normal(SDIM).astype(np.float32) for t in range(60) for _ in range(6)]
    vecs += list(rng.standard_normal((200, SDIM)).astype(np.float32))
    chunks, sparse = [], []
    for i, v in enumerate(vecs):
        meta = ChunkMetadata(file_path=f"f{i % 5}.md", folder_path=f"d{i % 2}", index_folder="ix", file_name="f",
                             chunk_index=i, total_chunks=len(vecs), start_char=0, end_char=1, indexed_at="t")
        chunks.append((f"chunk {i}", v.tolist(), meta))
        sparse.append(([int(i % 11), 20 + int(i % 7)], [1.0, 0.5]))
    vs = VectorStoreService()
    vs.store_chunks(chunks, sparse_vectors=sparse)
    vs.flush()
    yield vs, eng, topics, np.stack(vecs)
    store_registry.set_engine(None)
    config.get_settings.cache_clear()
    eng.close()


def _stored_of(vs, eng, chunks):
    col = vs._col
    rows = np.asarray([col.row_of[c.id] for c in chunks], np.int64)
    return rows, eng.get_dense(rows)


def _expect(vs, eng, pool, rel, d, limit):
    rows, x = _stored_of(vs, eng, pool)
    return [pool[i] for i in mo.select(mo.gram(x), rel, d, limit)]


def test_service_diversity_zero_is_the_plain_search(service):
    vs, eng, topics, _ = service
    rng = np.random.default_rng(2)
    for t in range(4):
        q = (topics[t] + np.float32(0.1) * rng.standard_normal(SDIM).astype(np.float32)).tolist()
        for sp in (None, ([t, 20 + t], [1.0, 1.0])):
            plain = vs.search(q, limit=10, sparse_query=sp)
            got = vs.search(q, limit=10, sparse_query=sp, mmr_diversity=0.0)
            assert [(c.id, c.score) for c in got] == [(c.id, c.score) for c in plain]


def test_service_search_equals_oracle_over_its_first_stage(service):
    vs, eng, topics, _ = service
    q = (topics[3] + topics[4]).tolist()
    for sp in (None, ([3, 23], [1.0, 1.0])):
        for d in (0.3, 0.5, 1.0):
            pool = vs.search(q, limit=50, sparse_query=sp)
            rel = ([float(np.float32(c.score)) for c in pool] if sp is None else [c.score for c in pool])
            got = vs.search(q, limit=10, sparse_query=sp, mmr_diversity=d, mmr_candidates=50)
            want = _expect(vs, eng, pool, rel, d, 10)
            assert [(c.id, c.score) for c in got] == [(c.id, c.score) for c in want]


def test_service_requests_mixed_batch(service):
    vs, eng, topics, _ = service
    reqs = [dict(query_embedding=topics[0].tolist(), limit=5),
            dict(query_embedding=topics[1].tolist(), limit=8, mmr_diversity=0.5, mmr_candidates=40, folder_filter="d1"),
            dict(query_embedding=topics[2].tolist(), limit=5, sparse_query=([2], [1.0])),
            dict(query_embedding=topics[5].tolist(), limit=6, sparse_query=([5, 25], [1.0, 1.0]), mmr_diversity=0.7),
            dict(query_embedding=topics[6].tolist(), limit=0, mmr_diversity=0.5)]
    got = vs.search_requests(reqs)
    for r, g in zip(reqs, got):
        assert [(c.id, c.score) for c in g] == [(c.id, c.score) for c in vs.search(**r)]
    # the requests without MMR: the batch without any MMR request answers them the same
    plain = vs.search_requests([{k: v for k, v in r.items() if not k.startswith("mmr_")} for r in reqs])
    for j in (0, 2, 4):
        assert [(c.id, c.score) for c in got[j]] == [(c.id, c.score) for c in plain[j]]


def test_near_copies_are_diversified(service):
    """The plain top 10 of a topic's query holds its six near-copies; with d = 0.5 at most one of them. The pool holds
    more than ten mutually dissimilar relevant chunks (every topic's copies mix a shared component into the query)."""
    vs, eng, topics, _ = service
    mix = topics[0] * np.float32(1.5) + topics[1:12].sum(0) * np.float32(0.6)
    q = mix.tolist()
    copies = {c.id for c in vs.search(topics[0].tolist(), limit=6)}
    plain = vs.search(q, limit=10)
    assert len(copies & {c.id for c in plain}) >= 3
    got = vs.search(q, limit=10, mmr_diversity=0.5, mmr_candidates=80)
    assert len(copies & {c.id for c in got}) <= 1
    assert len(got) == 10
    pool = vs.search(q, limit=80)
    want = _expect(vs, eng, pool, [float(np.float32(c.score)) for c in pool], 0.5, 10)
    assert [c.id for c in got] == [c.id for c in want]


# ---- from text, search_questions and the reranked path (the native e5-shaped embedder, the synthetic cross-encoder) ------
from test_query_text_batch_gpu import WORDS, native, questions  # noqa: E402,F401  (fixture)
from test_rerank_gpu import reranked  # noqa: E402,F401  (fixture)


def _index_texts(vs, emb, sp, rng, n=150):
    """n chunks of vocabulary words; every fifth one is a near-copy of the one before (one word changed), as overlapping
    chunks and re-indexed files are."""
    from voitta_rag_amd.vector_store import ChunkMetadata

    texts = []
    for i in range(n):
        if i % 5 == 4:
            words = texts[-1].split()
            words[int(rng.integers(0, len(words)))] = str(rng.choice(WORDS))
            texts.append(" ".join(words))
        else:
            texts.append(" ".join(rng.choice(WORDS, size=int(rng.integers(4, 40)))))
    metas = [ChunkMetadata(file_path=f"docs/{i % 4}.md", folder_path="docs", index_folder="docs", file_name=f"{i % 4}.md",
                           chunk_index=i, total_chunks=n, start_char=i, end_char=i + 1, indexed_at="2026-01-01T00:00:00",
                           source_modified_at=1_700_000_000 + i) for i in range(n)]
    vs.store_chunks(list(zip(texts, emb.embed_texts(texts), metas)), sparse_vectors=sp.embed_texts(texts))
    vs.flush()


def _text_services():
    from voitta_rag_amd.embedding import get_embedding_service
    from voitta_rag_amd.sparse_embedding import get_sparse_embedding_service
    from voitta_rag_amd.vector_store import get_vector_store

    return get_embedding_service(), get_sparse_embedding_service(), get_vector_store()


def _mmr_of(vs, pool, rel, d, limit, score_of):
    """The oracle's MMR over a first stage's own output: [(id, score)]."""
    rows, x = _stored_of(vs, vs._engine, pool)
    return [(pool[i].id, score_of(i)) for i in mo.select(mo.gram(x), rel, d, limit)]


def _f32_rel(pool):
    return [float(np.float32(c.score)) for c in pool]  # (the f32 cosine: _json_float round-trips it)


def test_text_search_mmr(native):
    from voitta_rag_amd import deferred

    emb, sp, vs = _text_services()
    rng = np.random.default_rng(41)
    _index_texts(vs, emb, sp, rng)
    for q in questions(rng, 4):
        for hybrid in (False, True):
            def args():
                ref = emb.embed_query(q)
                assert isinstance(ref, deferred.QueryRef) and not ref.materialized  # (the one-call text path)
                return dict(query_embedding=ref, sparse_query=sp.embed_query(q) if hybrid else None)

            plain = vs.search(**args(), limit=8)
            zero = vs.search(**args(), limit=8, mmr_diversity=0.0)
            assert [(c.id, c.score) for c in zero] == [(c.id, c.score) for c in plain]
            pool = vs.search(**args(), limit=30)
            rel = [c.score for c in pool] if hybrid else _f32_rel(pool)
            for d in (0.3, 0.7):
                got = vs.search(**args(), limit=8, mmr_diversity=d, mmr_candidates=30)
                assert [(c.id, c.score) for c in got] == _mmr_of(vs, pool, rel, d, 8, lambda i: pool[i].score)


def test_search_questions_mixed_mmr(native):
    emb, sp, vs = _text_services()
    rng = np.random.default_rng(43)
    _index_texts(vs, emb, sp, rng)
    qs = questions(rng, 5)
    reqs = [{"query": qs[0], "limit": 6},
            {"query": qs[1], "limit": 5, "mmr_diversity": 0.5, "mmr_candidates": 30},
            {"query": qs[2], "limit": 4, "mmr_diversity": 0.0},
            {"query": qs[3], "limit": 7, "sparse_weight": 0.0, "mmr_diversity": 1.0, "mmr_candidates": 20},
            {"query": qs[4], "limit": 6, "folder_filter": "docs", "mmr_diversity": 0.3}]
    got = vs.search_questions(reqs)
    base = [{k: v for k, v in r.items() if not k.startswith("mmr_")} for r in reqs]
    plain = vs.search_questions(base)
    for j in (0, 2):  # no MMR, and d = 0: the plain answer
        assert [(c.id, c.score) for c in got[j]] == [(c.id, c.score) for c in plain[j]]
    for j, pool_n in ((1, 30), (3, 20), (4, 50)):  # the first stage at the pool size, in the same batch of questions
        first = vs.search_questions([dict(r, limit=pool_n) if i == j else r for i, r in enumerate(base)])[j]
        hybrid = len(sp.embed_query(qs[j])[0]) > 0
        rel = [c.score for c in first] if hybrid else _f32_rel(first)
        want = _mmr_of(vs, first, rel, reqs[j]["mmr_diversity"], reqs[j]["limit"], lambda i: first[i].score)
        assert [(c.id, c.score) for c in got[j]] == want, j


def test_reranked_mmr(reranked):
    from voitta_rag_amd.config import get_settings
    from voitta_rag_amd.reranker import get_reranker, sigmoid

    emb, sp, vs = _text_services()
    rng = np.random.default_rng(47)
    _index_texts(vs, emb, sp, rng, n=120)
    settings = get_settings()
    model = settings.rerank_model
    rr = get_reranker(vs._engine, model)
    qs = questions(rng, 3)

    def first_stage(call):
        settings.rerank_model = ""
        try:
            return call()
        finally:
            settings.rerank_model = model

    for q in qs:
        got = vs.search(emb.embed_query(q), limit=7, sparse_query=sp.embed_query(q), mmr_diversity=0.5)
        pool = first_stage(lambda: vs.search(emb.embed_query(q), limit=30, sparse_query=sp.embed_query(q)))  # 30: the rerank pool
        rel = sigmoid(rr.logits([q], [[c.text for c in pool]])[0]).astype(np.float64)
        assert [(c.id, c.score) for c in got] == _mmr_of(vs, pool, rel, 0.5, 7, lambda i: float(rel[i]))
        zero = vs.search(emb.embed_query(q), limit=7, sparse_query=sp.embed_query(q), mmr_diversity=0.0)
        plain = vs.search(emb.embed_query(q), limit=7, sparse_query=sp.embed_query(q))
        assert [(c.id, c.score) for c in zero] == [(c.id, c.score) for c in plain]
    # search_questions: one rerank call; the question without MMR is exactly _rerank's answer for the batch
    reqs = [{"query": qs[0], "limit": 7}, {"query": qs[1], "limit": 5, "mmr_diversity": 0.6}, {"query": qs[2], "limit": 6}]
    got = vs.search_questions(reqs)
    firsts = first_stage(lambda: vs.search_questions([{"query": q, "limit": 30} for q in qs]))
    plain = vs._rerank(rr, qs, firsts, [7, 5, 6])
    for j in (0, 2):
        assert [(c.id, c.score) for c in got[j]] == [(c.id, c.score) for c in plain[j]]
    logits = rr.logits(qs, [[c.text for c in f] for f in firsts])
    rel = sigmoid(logits[1]).astype(np.float64)
    assert [(c.id, c.score) for c in got[1]] == _mmr_of(vs, firsts[1], rel, 0.6, 5, lambda i: float(rel[i]))
