"""Parity of the HIP store/search path (through the C-ABI) against the CPU oracle, bit for bit:
stored vectors, dense scores, sparse scores, ranked row ids, fused scores.
Reference behaviour restated: src/voitta/services/vector_store.py:233-317 (store), :560-697
(search / hybrid), :462-530 (filters), :319-355 (delete)."""
import numpy as np
import pytest

from oracle import core as ocore
from oracle import fusion as ofus

pytestmark = pytest.mark.gpu


def _engine(dim, **kw):
    from voitta_rag_amd import Engine

    return Engine(dim, **kw)


def _corpus(rng, n, dim):
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x[::7] = ocore.cosine_preprocess(x[::7])  # already unit length -> stored untouched
    if n > 5:
        x[5] = 0.0  # zero vector -> stored untouched
    x[1::11] *= 37.5
    return x


def _sparse_rows(rng, n, vocab=500, lo=0, hi=40):
    rows = []
    for _ in range(n):
        m = int(rng.integers(lo, hi + 1))
        ids = rng.choice(vocab, size=m, replace=False).astype(np.int32) * 7919 + 13
        vals = rng.uniform(0.2, 2.2, size=m).astype(np.float32)
        rows.append((ids, vals))
    return rows


@pytest.mark.parametrize("dim,n", [(384, 3001), (768, 1000), (1024, 257), (16, 40)])
def test_store_and_dense_search_bit_exact(gpu, dim, n):
    rng = np.random.default_rng(dim + n)
    x = _corpus(rng, n, dim)
    e = _engine(dim)
    # several unaligned batches
    cuts = sorted({min(c, n) for c in (0, 1, 18, 100, n // 2, n)})
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert e.upsert(x[a:b]) == a
    assert e.count() == (n, n)
    want_x = ocore.cosine_preprocess(x)
    got_x = e.get_dense(np.arange(n))
    assert np.array_equal(got_x.view(np.uint32), want_x.view(np.uint32))

    q = rng.standard_normal((21, dim)).astype(np.float32)
    q[3] = x[17]  # exact duplicate of a stored row
    want_scores = ocore.dense_scores(ocore.cosine_preprocess(q), want_x)
    # 21 queries run as blocks of 16 and 5: more than 4 queries take the score array + select kernels at every k.
    # The first three alone take the fused scan + select for k <= 64 (the score array + select kernels above).
    for k in (1, 10, 30, 64, 70):
        got = e.search_dense(q, k)
        few = e.search_dense(q[:3], k)
        for i in range(q.shape[0]):
            wr, ws = ocore.topk(want_scores[i], k)
            assert np.array_equal(got[i][0], wr), (dim, n, k, i)
            assert np.array_equal(got[i][1].view(np.uint32), ws.view(np.uint32))
            if i < 3:
                assert np.array_equal(few[i][0], wr), (dim, n, k, i)
                assert np.array_equal(few[i][1].view(np.uint32), ws.view(np.uint32))
    e.close()


def test_ties_resolve_to_lower_row(gpu):
    dim = 64
    rng = np.random.default_rng(3)
    base = rng.standard_normal((50, dim)).astype(np.float32)
    x = np.concatenate([base, base[:20]])  # rows 50..69 duplicate rows 0..19
    e = _engine(dim)
    e.upsert(x)
    rows, scores = e.search_dense(base[7:8], 4)[0]
    assert rows[0] == 7 and rows[1] == 57 and scores[0] == scores[1]
    e.close()


def test_delete_filter_and_counts(gpu):
    dim, n = 128, 2000
    rng = np.random.default_rng(11)
    x = _corpus(rng, n, dim)
    folder = rng.integers(0, 9, size=n).astype(np.int32)
    ifolder = rng.integers(0, 4, size=n).astype(np.int32)
    from voitta_rag_amd import SearchFilter
    from voitta_rag_amd.engine import VR_TS_ABSENT

    modified = rng.integers(1_600_000_000, 1_700_000_000, size=n).astype(np.int64)
    modified[::5] = VR_TS_ABSENT
    created = rng.integers(1_500_000_000, 1_600_000_000, size=n).astype(np.int64)
    e = _engine(dim)
    e.upsert(x, folder_ids=folder, index_folder_ids=ifolder, created=created, modified=modified)
    dead = rng.choice(n, size=300, replace=False)
    e.delete_rows(np.concatenate([dead, dead[:10]]))  # duplicates ignored
    e.delete_rows(dead[:5])  # already dead ignored
    assert e.count() == (n, n - 300)
    live = np.ones(n, np.uint8)
    live[dead] = 0
    xh = ocore.cosine_preprocess(x)
    q = rng.standard_normal((3, dim)).astype(np.float32)
    sc = ocore.dense_scores(ocore.cosine_preprocess(q), xh)

    cases = [
        (SearchFilter(), live.astype(bool)),
        (SearchFilter(folder_filter=3), live.astype(bool) & (folder == 3)),
        (SearchFilter(include_folders=[1, 2, 8, 77]), live.astype(bool) & np.isin(folder, [1, 2, 8])),
        (SearchFilter(folder_filter=2, include_folders=[1, 2]), live.astype(bool) & (folder == 2)),
        (SearchFilter(folder_filter=2, include_folders=[1]), np.zeros(n, bool)),
        (SearchFilter(exclude_folders=[0, 4], exclude_index_folders=[1]),
         live.astype(bool) & ~np.isin(folder, [0, 4]) & (ifolder != 1)),
        (SearchFilter(date_start=1_650_000_000), live.astype(bool) & (modified != VR_TS_ABSENT) & (modified >= 1_650_000_000)),
        (SearchFilter(date_start=1_620_000_000, date_end=1_660_000_000),
         live.astype(bool) & (modified != VR_TS_ABSENT) & (modified >= 1_620_000_000) & (modified <= 1_660_000_000)),
        (SearchFilter(date_end=1_550_000_000, date_field="created"), live.astype(bool) & (created <= 1_550_000_000)),
        (SearchFilter(date_end=1_650_000_000, date_field="bogus"),
         live.astype(bool) & (modified != VR_TS_ABSENT) & (modified <= 1_650_000_000)),
    ]
    for flt, mask in cases:
        got = e.search_dense(q, 25, flt)
        for i in range(3):
            wr, ws = ocore.topk(sc[i], 25, mask.astype(np.uint8))
            assert np.array_equal(got[i][0], wr), flt
            assert np.array_equal(got[i][1], ws)
    e.close()


def test_sparse_and_hybrid_bit_exact(gpu):
    dim, n = 64, 1500
    rng = np.random.default_rng(5)
    x = _corpus(rng, n, dim)
    sp = _sparse_rows(rng, n)
    e = _engine(dim)
    cuts = [0, 70, 200, 1000, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        e.upsert(x[a:b], sparse=sp[a:b])
    xh = ocore.cosine_preprocess(x)
    df_want, n_points = ocore.document_frequencies(sp)
    some = np.array(sorted(df_want)[:50] + [999_999_999], np.int32)
    df_got, n_got = e.sparse_stats(some)
    assert n_got == n_points == n
    assert [int(v) for v in df_got] == [df_want.get(int(t), 0) for t in some]

    live = np.ones(n, bool)
    for round_ in range(2):
        for trial in range(12):
            m = int(rng.integers(1, 9))
            qi = (rng.choice(500, size=m, replace=False).astype(np.int32) * 7919 + 13)
            if trial == 0:
                qi[0] = 5  # a token no document has
            qv = np.ones(m, np.float32)
            want = ocore.sparse_scores(sp, qi, qv, live)
            for k in (10, 30, 100):
                wr, ws = ocore.topk(want, k, live.astype(np.uint8))
                gr, gs = e.search_sparse(qi, qv, k)
                assert np.array_equal(gr, wr), (round_, trial, k)
                assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
            # hybrid, reference defaults: limit 10, prefetch 30, sparse_weight 0.1
            q = rng.standard_normal(dim).astype(np.float32)
            dsc = ocore.dense_scores(ocore.cosine_preprocess(q[None]), xh)[0]
            for limit, w in ((10, 0.1), (20, 0.5), (3, 1.0), (5, 0.0)):
                dr, ds = ocore.topk(dsc, 3 * limit, live.astype(np.uint8))
                sr, ss = ocore.topk(want, 3 * limit, live.astype(np.uint8))
                fused = ofus.hybrid_fuse(list(zip(dr.tolist(), ds.tolist())), list(zip(sr.tolist(), ss.tolist())),
                                         limit, w, "json")
                rows, scores, fd = e.search_hybrid(q, qi, qv, limit, w)
                assert rows.tolist() == [r for r, _, _ in fused]
                assert scores.tolist() == [s for _, s, _ in fused]
                assert fd.astype(bool).tolist() == [f for _, _, f in fused]
                # the same two top-(3 limit) lists fused by reciprocal rank (VR_FUSION_RRF, north_star's mode;
                # the reference's note on it: vector_store.py:638-639)
                from voitta_rag_amd.engine import VR_FUSION_RRF

                rr = ofus.rrf_fuse(list(zip(dr.tolist(), ds.tolist())), list(zip(sr.tolist(), ss.tolist())), limit)
                rows, scores, fd = e.search_hybrid(q, qi, qv, limit, w, fusion=VR_FUSION_RRF)
                assert rows.tolist() == [r for r, _, _ in rr]
                assert scores.tolist() == [s for _, s, _ in rr]
                assert fd.astype(bool).tolist() == [f for _, _, f in rr]
        # second round: after deletes the document frequencies and N must follow
        dead = rng.choice(n, size=400, replace=False)
        e.delete_rows(dead)
        live[dead] = False
    e.close()


def test_rows_without_sparse_vectors_and_empty_engine(gpu):
    dim = 32
    rng = np.random.default_rng(9)
    e = _engine(dim)
    assert e.search_dense(np.ones((2, dim), np.float32), 5) == [] or all(len(r) == 0 for r, _ in e.search_dense(np.ones((2, dim), np.float32), 5))
    r, s = e.search_sparse([1, 2], [1.0, 1.0], 5)
    assert len(r) == 0
    x = _corpus(rng, 130, dim)
    sp = _sparse_rows(rng, 130, lo=0, hi=6)
    e.upsert(x[:65])  # no sparse vectors at all
    e.upsert(x[65:], sparse=sp[65:])
    rows_sp = [None] * 65 + sp[65:]
    qi = sp[70][0][:2] if len(sp[70][0]) >= 2 else np.array([13], np.int32)
    qv = np.ones(len(qi), np.float32)
    want = ocore.sparse_scores(rows_sp, qi, qv)
    wr, ws = ocore.topk(want, 10)
    gr, gs = e.search_sparse(qi, qv, 10)
    assert np.array_equal(gr, wr) and np.array_equal(gs, ws)
    assert (gr >= 65).all()
    # hybrid with an empty sparse query term list degrades to dense candidates only
    rows, scores, fd = e.search_hybrid(x[3], [], [], 5, 0.1)
    assert rows[0] == 3 and fd.all()
    e.close()


@pytest.mark.parametrize("shadow", ["int8", "f16"])
@pytest.mark.parametrize("dim,n", [(768, 20000), (384, 9000), (1024, 5000), (64, 6000), (96, 5000)])
def test_two_stage_dense_search_is_bit_identical(gpu, dim, n, shadow, monkeypatch):
    """Stores with dim % 32 == 0 and >= 4096 rows answer single-query dense searches through a
    reduced-precision shadow scan + exact re-score (prefilter.hip): int8 with a scale per row when
    dim % 64 == 0 (unless VR_PREFILTER=f16), f16 otherwise. Rows, scores and order must equal the
    oracle's — and therefore the one-stage scan's — bit for bit, with filters and tombstones in play."""
    from voitta_rag_amd import SearchFilter

    if shadow == "f16":
        monkeypatch.setenv("VR_PREFILTER", "f16")
    elif dim % 64:
        pytest.skip("the int8 shadow needs dim % 64 == 0; this dimension always takes the f16 one")
    rng = np.random.default_rng(dim * 7 + n)
    x = _corpus(rng, n, dim)
    x[100:140] = x[100] + rng.standard_normal((40, dim)).astype(np.float32) * 1e-3  # a tight cluster
    x[200] = x[300]  # exact duplicates -> exact score ties
    folder = rng.integers(0, 5, size=n).astype(np.int32)
    e = _engine(dim)
    e1 = _engine(dim, prefilter=False)
    for a in range(0, n, 3333):
        e.upsert(x[a:a + 3333], folder_ids=folder[a:a + 3333])
        e1.upsert(x[a:a + 3333], folder_ids=folder[a:a + 3333])
    xh = ocore.cosine_preprocess(x)
    q = rng.standard_normal((12, dim)).astype(np.float32)
    q[0] = x[100]       # lands in the cluster: many candidates
    q[1] = x[300]       # ties
    q[2] = 0.0          # zero query
    q[3] *= 1e-4
    live = np.ones(n, bool)
    for round_ in range(2):
        for i in range(q.shape[0]):
            sc = ocore.dense_scores(ocore.cosine_preprocess(q[i:i + 1]), xh)[0]
            for k, flt, mask in ((10, None, live), (30, None, live), (64, None, live),
                                 (10, SearchFilter(include_folders=[1, 3]), live & np.isin(folder, [1, 3]))):
                wr, ws = ocore.topk(sc, k, mask.astype(np.uint8))
                for eng in (e, e1):
                    gr, gs = eng.search_dense(q[i:i + 1], k, flt)[0]
                    assert np.array_equal(gr, wr), (dim, n, i, k, eng is e)
                    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
        dead = rng.choice(n, size=n // 5, replace=False)
        e.delete_rows(dead)
        e1.delete_rows(dead)
        live[dead] = False
    st = e.stats()
    assert st["two_stage"] >= 80 and e1.stats()["two_stage"] == 0
    print(f"dim {dim} n {n}: two-stage searches {st['two_stage']}, overflow fallbacks {st['fallback']}, "
          f"last candidate count {st['last_candidates']}")
    e.close()
    e1.close()


def test_two_stage_overflow_falls_back_to_exact_scan(gpu):
    """A corpus of near-duplicates cannot be separated by the shadow's bounds: every row is a candidate,
    the re-score budget (16384 tiles) overflows and the search must transparently redo the one-stage scan."""
    dim, n = 128, 300000
    rng = np.random.default_rng(1)
    base = rng.standard_normal(dim).astype(np.float32)
    x = (base[None, :] + rng.standard_normal((n, dim)).astype(np.float32) * 2e-4).astype(np.float32)
    e = _engine(dim)
    e.upsert(x)
    xh = ocore.cosine_preprocess(x)
    q = base + rng.standard_normal(dim).astype(np.float32) * 1e-4
    sc = ocore.dense_scores(ocore.cosine_preprocess(q[None]), xh)[0]
    wr, ws = ocore.topk(sc, 10)
    gr, gs = e.search_dense(q[None], 10)[0]
    assert np.array_equal(gr, wr) and np.array_equal(gs, ws)
    st = e.stats()
    assert st["two_stage"] == 1 and st["fallback"] == 1 and st["last_candidates"] > 16384 * 16
    e.close()


@pytest.mark.parametrize("shadow", ["int8", "f16"])
def test_two_stage_rescoring_by_tile_absorbs_a_tight_cluster(gpu, shadow, monkeypatch):
    """20,000 stored rows within 1e-3 of each other (what a random-init encoder produces, and what the int8
    bounds cannot separate) among random rows: tens of thousands of candidates, but they share 1,250
    tiles, so the query is answered by the two-stage path without a fallback — and bit-exactly."""
    if shadow == "f16":
        monkeypatch.setenv("VR_PREFILTER", "f16")
    dim, n = 256, 60000
    rng = np.random.default_rng(3)
    x = _corpus(rng, n, dim)
    base = rng.standard_normal(dim).astype(np.float32)
    x[30000:50000] = base[None, :] + rng.standard_normal((20000, dim)).astype(np.float32) * 1e-3
    e = _engine(dim)
    e.upsert(x)
    xh = ocore.cosine_preprocess(x)
    for q in (base + rng.standard_normal(dim).astype(np.float32) * 1e-3, x[7], x[31234]):
        sc = ocore.dense_scores(ocore.cosine_preprocess(q[None]), xh)[0]
        for k in (10, 64):
            wr, ws = ocore.topk(sc, k)
            gr, gs = e.search_dense(q[None], k)[0]
            assert np.array_equal(gr, wr) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
    st = e.stats()
    assert st["two_stage"] == 6 and st["fallback"] == 0
    if shadow == "int8":
        assert st["last_candidates"] > 4096  # the last query sits inside the cluster
    e.close()


# ---- batched dense search (csrc/batch.hip; BASELINE configs[4]: 1k batched queries) --------------------------

@pytest.mark.parametrize("dim,n,nq", [(384, 20000, 1000), (1024, 17000, 256), (768, 16500, 17), (128, 30011, 300)])
def test_batched_dense_search_is_bit_exact(gpu, dim, n, nq):
    """More than 16 queries in one call go through the int8 matrix-core GEMM + exact re-score; the answer must
    be the oracle's for every query: ranked rows and f32 score bits, with tombstones and a filter in play."""
    from voitta_rag_amd.engine import SearchFilter

    rng = np.random.default_rng(dim + nq)
    x = _corpus(rng, n, dim)
    x[100:140] = x[100] + 1e-3 * rng.standard_normal((40, dim)).astype(np.float32)  # a tight cluster
    x[200:205] = x[200]                                                               # exact duplicates: ties
    folders = rng.integers(0, 5, size=n).astype(np.int32)
    e = _engine(dim, initial_rows=n)
    e.upsert(x, folder_ids=folders)
    dead = rng.choice(n, size=n // 50, replace=False)
    e.delete_rows(dead)
    live = np.ones(n, np.uint8)
    live[dead] = 0
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    q[0] = x[100]
    q[1] = x[200] * 3.0
    q[2] = 0.0  # a zero query: every score 0, ranking by row id
    xh = ocore.cosine_preprocess(x)
    want = ocore.dense_scores(ocore.cosine_preprocess(q), xh)
    before = e.stats()
    for k, mask, flt in ((10, live, None), (30, live & (folders != 3).astype(np.uint8), SearchFilter(exclude_folders=[3]))):
        got = e.search_dense(q, k, flt)
        for i in range(nq):
            wr, ws = ocore.topk(want[i], k, mask)
            assert np.array_equal(got[i][0], wr), (dim, n, nq, k, i)
            assert np.array_equal(got[i][1].view(np.uint32), ws.view(np.uint32)), (dim, n, nq, k, i)
    after = e.stats()
    assert after["batched"] - before["batched"] == 2 * nq  # the batched path served them ...
    assert after["batch_fallback"] - before["batch_fallback"] <= 6  # ... alone but for the zero / cluster queries
    # the same queries one at a time (two-stage single-query path): identical
    for i in (0, 1, 3, nq - 1):
        r1, s1 = e.search_dense(q[i:i + 1], 10)[0]
        rb, sb = e.search_dense(q, 10)[i]
        assert np.array_equal(r1, rb) and np.array_equal(s1.view(np.uint32), sb.view(np.uint32))
    e.close()


def test_batched_search_overflow_falls_back_per_query(gpu):
    """A corpus of near-duplicates puts more rows inside a query's bound than its candidate budget: that query is
    redone by the exact scans, the others stay on the batched path, every answer is still the oracle's."""
    dim, n, nq = 256, 20000, 40
    rng = np.random.default_rng(77)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x[:6000] = x[0] + 2e-4 * rng.standard_normal((6000, dim)).astype(np.float32)
    e = _engine(dim, initial_rows=n)
    e.upsert(x)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    q[5] = x[0]
    q[6] = x[17] + 0.01 * rng.standard_normal(dim).astype(np.float32)
    want = ocore.dense_scores(ocore.cosine_preprocess(q), ocore.cosine_preprocess(x))
    got = e.search_dense(q, 10)
    for i in range(nq):
        wr, ws = ocore.topk(want[i], 10)
        assert np.array_equal(got[i][0], wr) and np.array_equal(got[i][1].view(np.uint32), ws.view(np.uint32)), i
    st = e.stats()
    assert st["batched"] == nq and 2 <= st["batch_fallback"] <= 10
    e.close()


def test_search_dense_keys_on_the_device(gpu):
    """vr_search_dense_keys: the packed ranking keys, on the host and written straight into a device tensor (what
    the sharded searcher hands to RCCL), decode to exactly search_dense's answer — single block and batched path."""
    import torch

    from voitta_rag_amd import Engine

    rng = np.random.default_rng(31)
    n, dim = 17000, 128
    x = rng.standard_normal((n, dim)).astype(np.float32)
    e = _engine(dim, initial_rows=n)
    e.upsert(x)
    e.delete_rows(np.arange(0, n, 9))
    for nq in (3, 50):
        q = rng.standard_normal((nq, dim)).astype(np.float32)
        want = e.search_dense(q, 12)
        host = e.search_dense_keys(q, 12)
        out = torch.zeros((nq, 12), dtype=torch.int64, device="cuda:0")
        e.search_dense_keys(torch.from_numpy(q).to("cuda:0"), 12, out=out)
        dev = out.cpu().numpy().view(np.uint64)
        assert np.array_equal(host, dev)
        rows, scores = Engine.decode_keys(host)
        for i in range(nq):
            assert np.array_equal(rows[i], want[i][0]) and np.array_equal(scores[i].view(np.uint32), want[i][1].view(np.uint32))
    # fewer results than k: empty slots are key 0 -> row -1
    small = _engine(dim)
    small.upsert(x[:5])
    rows, scores = Engine.decode_keys(small.search_dense_keys(x[:1], 8))
    assert (rows[0][:5] >= 0).all() and (rows[0][5:] == -1).all()
    small.close()
    e.close()


def _anisotropic(rng, n, dim, cos, common):
    """rows = common direction + noise: pairwise cosine ~cos, as sentence-embedding collections have"""
    u = rng.standard_normal((n, dim)).astype(np.float32)
    u -= (u @ common)[:, None] * common[None, :]
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (np.sqrt(cos) * common[None, :] + np.sqrt(1 - cos) * u).astype(np.float32)


@pytest.mark.parametrize("dim,n", [(768, 24000), (256, 40000)])
def test_two_stage_search_on_an_anisotropic_corpus(gpu, dim, n, monkeypatch):
    """VERDICT r1 item 8. Rows that share a common direction squeeze the scores together (sigma 0.011 instead of 0.036
    at D = 768) while the int8 bound stays as wide: ~6400 candidates per query at 1M rows and every batched query over
    its candidate budget. The shadow therefore holds residuals around the column mean (prefilter.hip "centred
    shadow"), re-centred whenever the collection has doubled. Whatever the centre, answers are the oracle's bit for
    bit — single queries, batched queries, across the re-centrings of a growing collection, deletes and a compaction
    — and the centred shadow needs several times fewer candidates than the uncentred one on the same data."""
    rng = np.random.default_rng(dim + n)
    common = rng.standard_normal(dim).astype(np.float32)
    common /= np.linalg.norm(common)
    x = _anisotropic(rng, n, dim, 0.7, common)
    q = _anisotropic(rng, 40, dim, 0.7, common)
    xh = ocore.cosine_preprocess(x)
    qh = ocore.cosine_preprocess(q)

    def run(centre):
        monkeypatch.setenv("VR_PREFILTER_CENTRE", "1" if centre else "0")
        e = _engine(dim)
        cands = []
        bounds = [0, 700, 1500, 5000, 11000, n]  # appends that cross the 1024-row start and three doublings
        for a, b in zip(bounds[:-1], bounds[1:]):
            e.upsert(x[a:b])
            if b >= 5000:  # (the two-stage path starts at 4096 rows)
                for i in range(4):
                    sc = ocore.dense_scores(qh[i:i + 1], xh[:b])[0]
                    wr, ws = ocore.topk(sc, 30)
                    gr, gs = e.search_dense(q[i:i + 1], 30)[0]
                    assert np.array_equal(gr, wr) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), (centre, b, i)
        live = np.ones(n, bool)
        for phase in range(3):
            sc_all = ocore.dense_scores(qh, xh)
            before = e.stats()
            for i in range(q.shape[0]):
                wr, ws = ocore.topk(sc_all[i], 10, live.astype(np.uint8))
                gr, gs = e.search_dense(q[i:i + 1], 10)[0]
                assert np.array_equal(gr if phase < 2 else remap_back[gr], wr), (centre, phase, i)
                assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
                cands.append(e.stats()["last_candidates"])
            after = e.stats()
            assert after["fallback"] == before["fallback"]
            if n >= 16384 and phase == 0:  # the batched path (needs >= 16384 rows): same answers
                batch = e.search_dense(q, 10)
                for i in range(q.shape[0]):
                    wr, ws = ocore.topk(sc_all[i], 10, live.astype(np.uint8))
                    assert np.array_equal(batch[i][0], wr) and np.array_equal(batch[i][1].view(np.uint32), ws.view(np.uint32))
                s2 = e.stats()
                assert s2["batched"] - after["batched"] == q.shape[0]
                if centre:
                    assert s2["batch_fallback"] == after["batch_fallback"]
            if phase == 0:
                dead = rng.choice(n, size=n // 4, replace=False)
                e.delete_rows(dead)
                live[dead] = False
            elif phase == 1:
                remap = e.compact()
                remap_back = np.flatnonzero(remap >= 0)[np.argsort(remap[remap >= 0])]  # new row -> old row
        e.close()
        return float(np.median(cands))

    centred, plain = run(True), run(False)
    print(f"anisotropic {n}x{dim}: median candidates {centred:.0f} centred, {plain:.0f} uncentred")
    assert centred * 2.5 < plain


def test_caller_supplied_sizes_the_reference_accepts(gpu):
    """`limit` is an MCP tool argument (mcp_server.py:376,474) and the reference accepts any value; so
    does this — 100 hybrid results (prefetch 300 per modality), 300 dense results, a sparse query of 400 distinct
    stems — bit-exact against the oracle, and the engine's caps (k <= 1024, 1024 query terms) fail with a message."""
    from voitta_rag_amd._lib import EngineError

    dim, n = 128, 6000
    rng = np.random.default_rng(77)
    x = _corpus(rng, n, dim)
    sp = _sparse_rows(rng, n)
    e = _engine(dim)
    e.upsert(x, sparse=sp)
    xh = ocore.cosine_preprocess(x)
    live = np.ones(n, bool)
    q = rng.standard_normal(dim).astype(np.float32)
    dsc = ocore.dense_scores(ocore.cosine_preprocess(q[None]), xh)[0]
    # dense, 300 results
    wr, ws = ocore.topk(dsc, 300, live.astype(np.uint8))
    gr, gs = e.search_dense(q[None], 300)[0]
    assert np.array_equal(gr, wr) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
    # hybrid, 100 results = two top-300 lists
    qi = (rng.choice(500, size=6, replace=False).astype(np.int32) * 7919 + 13)
    qv = np.ones(6, np.float32)
    ssc = ocore.sparse_scores(sp, qi, qv, live)
    dr, ds = ocore.topk(dsc, 300, live.astype(np.uint8))
    sr, ss = ocore.topk(ssc, 300, live.astype(np.uint8))
    fused = ofus.hybrid_fuse(list(zip(dr.tolist(), ds.tolist())), list(zip(sr.tolist(), ss.tolist())), 100, 0.1, "json")
    rows, scores, fd = e.search_hybrid(q, qi, qv, 100, 0.1)
    assert rows.tolist() == [r for r, _, _ in fused] and scores.tolist() == [s for _, s, _ in fused]
    # a sparse query of 400 distinct stems (a long pasted question)
    qi = (rng.choice(500, size=400, replace=False).astype(np.int32) * 7919 + 13)
    qv = np.ones(400, np.float32)
    ssc = ocore.sparse_scores(sp, qi, qv, live)
    wr, ws = ocore.topk(ssc, 50, live.astype(np.uint8))
    gr, gs = e.search_sparse(qi, qv, 50)
    assert np.array_equal(gr, wr) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
    # beyond the caps: a clear error, not a crash
    with pytest.raises(EngineError):
        e.search_dense(q[None], 1025)
    with pytest.raises(EngineError):
        e.search_hybrid(q, qi[:3], qv[:3], 342, 0.1)
    e.close()


def test_inverted_sparse_scan_equals_the_forward_scan(gpu, monkeypatch, tmp_path):
    """csrc/invert.hip (postings by term, what a query of <= 32 terms reads) against csrc/sparse.hip (every stored id)
    and the oracle: same rows, same f32 bits — across batches that cut segments at odd places, rows that list a term
    twice, deletes, filters, compaction and a save/load (the inverted index is derived data, rebuilt there)."""
    from voitta_rag_amd import SearchFilter

    dim, n = 16, 9000
    rng = np.random.default_rng(77)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    sp = _sparse_rows(rng, n, vocab=300, lo=0, hi=30)
    folder = rng.integers(0, 5, size=n).astype(np.int32)
    e = _engine(dim)
    cuts = [0, 1, 65, 2048, 2049, 4700, 8999, n]  # segments (<= 4096 rows) start afresh with every batch
    for a, b in zip(cuts[:-1], cuts[1:]):
        e.upsert(x[a:b], sparse=sp[a:b], folder_ids=folder[a:b])
    live = np.ones(n, bool)

    def check(engine, rows_sp, live_mask, folders, tag):
        for trial in range(10):
            m = int(rng.integers(1, 33)) if trial else 32
            qi = (rng.choice(300, size=m, replace=False).astype(np.int32) * 7919 + 13)
            qv = rng.uniform(0.5, 1.5, size=m).astype(np.float32)
            want = ocore.sparse_scores(rows_sp, qi, qv, live_mask)
            for flt, mask in ((None, live_mask), (SearchFilter(folder_filter=2), live_mask & (folders == 2))):
                for k in (1, 10, 64):
                    wr, ws = ocore.topk(want, k, mask.astype(np.uint8))
                    monkeypatch.setenv("VR_SPARSE_INVERTED", "1")
                    gr, gs = engine.search_sparse(qi, qv, k, flt)
                    monkeypatch.setenv("VR_SPARSE_INVERTED", "0")
                    fr, fs = engine.search_sparse(qi, qv, k, flt)
                    assert np.array_equal(gr, wr) and np.array_equal(fr, wr), (tag, trial, k)
                    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), (tag, trial, k)
                    assert np.array_equal(fs.view(np.uint32), ws.view(np.uint32)), (tag, trial, k)
        monkeypatch.setenv("VR_SPARSE_INVERTED", "1")

    check(e, sp, live, folder, "fresh")
    dead = rng.choice(n, size=2500, replace=False)
    e.delete_rows(dead)
    live[dead] = False
    check(e, sp, live, folder, "deleted")
    path = str(tmp_path / "inv.vrx")
    e.save(path)
    e2 = _engine(dim)
    e2.load(path)
    check(e2, sp, live, folder, "loaded")
    e2.close()
    remap = e.compact()
    keep = np.flatnonzero(remap >= 0)
    assert np.array_equal(remap[keep], np.arange(keep.size))
    sp_c = [sp[i] for i in keep]
    check(e, sp_c, np.ones(keep.size, bool), folder[keep], "compacted")
    more = _sparse_rows(rng, 100, vocab=300, lo=1, hi=30)
    e.upsert(x[:100], sparse=more, folder_ids=folder[:100])  # appends go on after a compaction
    check(e, sp_c + more, np.ones(keep.size + 100, bool), np.concatenate([folder[keep], folder[:100]]), "appended")
    e.close()

    # many small upserts: each is a segment of its own until there are four times as many as the rows need, then the
    # whole index is sorted into full segments again (twice on the way to 160 upserts)
    t = _engine(dim)
    for a in range(0, 800, 5):
        t.upsert(x[a:a + 5], sparse=sp[a:a + 5], folder_ids=folder[a:a + 5])
    check(t, sp[:800], np.ones(800, bool), folder[:800], "small upserts")
    t.close()

    # rows that list a term twice (caller-supplied vectors may; the oracle's statistics count such a term once, the
    # engine's once per entry, so here the engine is held against its own forward scan): both entries count, in row
    # order — the engine notices such rows and keeps the collection on the forward scan
    d = _engine(dim)
    rows = _sparse_rows(rng, 300, vocab=40, lo=2, hi=12)
    for r in range(0, 300, 3):
        ids, vals = rows[r]
        rows[r] = (np.concatenate([ids, ids[:2]]), np.concatenate([vals, np.array([1.375, 0.3], np.float32)]))
    d.upsert(x[:300], sparse=rows)
    for trial in range(8):
        qi = (rng.choice(40, size=5, replace=False).astype(np.int32) * 7919 + 13)
        qv = rng.uniform(0.5, 1.5, size=5).astype(np.float32)
        monkeypatch.setenv("VR_SPARSE_INVERTED", "1")
        gr, gs = d.search_sparse(qi, qv, 64)
        monkeypatch.setenv("VR_SPARSE_INVERTED", "0")
        fr, fs = d.search_sparse(qi, qv, 64)
        assert len(gr) > 0 and np.array_equal(gr, fr) and np.array_equal(gs.view(np.uint32), fs.view(np.uint32))
    # ... and a file of such rows is recognised when it is loaded (the index is rebuilt from the slices there)
    d.save(path)
    d2 = _engine(dim)
    d2.load(path)
    for trial in range(8):
        qi = (rng.choice(40, size=5, replace=False).astype(np.int32) * 7919 + 13)
        qv = rng.uniform(0.5, 1.5, size=5).astype(np.float32)
        monkeypatch.setenv("VR_SPARSE_INVERTED", "1")
        gr, gs = d2.search_sparse(qi, qv, 64)
        fr, fs = d.search_sparse(qi, qv, 64)
        assert len(gr) > 0 and np.array_equal(gr, fr) and np.array_equal(gs.view(np.uint32), fs.view(np.uint32))
    d2.close()
    monkeypatch.setenv("VR_SPARSE_INVERTED", "1")
    d.close()
