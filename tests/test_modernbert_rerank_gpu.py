"""ModernBERT cross-encoders on the GPU (vr_reranker_load with a VR_NORM_PRE description, rerank_head_ln_kernel):
logits against the transformers goldens and the f64 oracle at every precision and every pair length of the goldens,
the head alone on the encoder's own pooled rows, its 16-row block edges bit for bit, the reload and refusal rules, a
checkpoint directory through NativeCrossEncoder, and the VOITTA_RERANK_MODEL path of VectorStoreService."""
import os

import numpy as np
import pytest

import modernbert_oracle as mo
import modernbert_rerank_oracle as mro
from test_modernbert_rerank_cpu import GOLDEN, case

pytestmark = pytest.mark.gpu
# tests/test_rerank_gpu.py's bars: |logit - reference| for a head on the same encoder precisions
BAR = {"f32": 1e-4, "f16x3": 1e-4, "f16": 5e-2}


def _engine(shape, w, pooling, precision):
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    e = Engine(shape.hidden)
    enc.load_reranker(e, mro.desc_for(shape, pooling, precision), w)
    return e


_oracle = {}


def oracle_logits(path):
    """The f64 oracle's logits of a golden's pairs, computed once."""
    if path not in _oracle:
        g, shape, w, pooling = case(path)
        _oracle[path] = mro.logits(w, shape, g["ids"], g["offsets"], pooling)
    return _oracle[path]


@pytest.mark.parametrize("precision", list(BAR))
@pytest.mark.parametrize("path", GOLDEN, ids=os.path.basename)
def test_logits_match_golden_and_oracle(gpu, path, precision):
    g, shape, w, pooling = case(path)
    e = _engine(shape, w, pooling, precision)
    got = e.rerank(g["ids"], g["offsets"], None).astype(np.float64)
    again = e.rerank(g["ids"], g["offsets"], None).astype(np.float64)
    d_gold, d_oracle = np.abs(got - g["logits"]), np.abs(got - oracle_logits(path))
    print(f"{os.path.basename(path)} {precision}: max |d| vs transformers {d_gold.max():.3e}, vs f64 oracle "
          f"{d_oracle.max():.3e}; per pair length {dict(zip(np.diff(g['offsets']).tolist(), np.round(d_gold, 7).tolist()))}")
    assert np.array_equal(got, again)
    assert d_gold.max() <= BAR[precision] and d_oracle.max() <= BAR[precision]
    # every pair alone (another token count, another GEMM route, the staged windowed kernel below 384 tokens)
    off = g["offsets"]
    for i in range(len(off) - 1):
        one = e.rerank(g["ids"][off[i]:off[i + 1]], np.array([0, off[i + 1] - off[i]], np.int32), None)
        assert abs(float(one[0]) - g["logits"][i]) <= BAR[precision], (i, float(one[0]), g["logits"][i])
    e.close()


@pytest.mark.parametrize("path", GOLDEN, ids=os.path.basename)
def test_head_on_the_encoders_own_pooled_rows(gpu, path):
    """The body loaded as an embedder with the same pooling and no normalisation gives the rows the head reads (f32:
    one GEMM route, the same launches); the f64 head on exactly those rows is what the kernel must give, to f32
    rounding: H products per unit and H units per row of O(1) values at 2^-24 each, times the classifier's scale
    (<= 19) -- below 1e-4, the bar of the f32 head in tests/test_rerank_gpu.py."""
    from voitta_rag_amd import encoder as enc

    g, shape, w, pooling = case(path)
    e = _engine(shape, w, pooling, "f32")
    body = {k: v for k, v in w.items() if not k.startswith(("head.", "classifier."))}
    enc.load_encoder(e, mro.desc_for(shape, pooling, "f32"), body)
    rows = enc.encode(e, g["ids"], g["offsets"]).astype(np.float64)
    got = e.rerank(g["ids"], g["offsets"], None).astype(np.float64)
    d = np.abs(got - mro.head(w, rows, shape.eps)).max()
    print(f"{os.path.basename(path)}: head kernel vs f64 head on the same rows, max |d| {d:.3e}")
    assert d <= 1e-4
    e.close()


def test_head_block_edges_bit_for_bit(gpu):
    """n = 1, 15, 16, 17 and 33 pairs in one call: a pair's logit depends neither on n nor on its place in the batch.
    f32, every pair 24 tokens long: the body then takes the same kernels with the same per-row arithmetic whatever n
    is, so the rows the head reads are the same bits and any difference is the head's."""
    g, shape, w, pooling = case([p for p in GOLDEN if "mean_w64" in p][0])
    e = _engine(shape, w, pooling, "f32")
    rng = np.random.default_rng(12)
    S, N = 24, 33
    seqs = rng.integers(3, shape.vocab, size=(N, S)).astype(np.int32)
    seqs[:, 0], seqs[:, 9], seqs[:, -1] = 1, 2, 2

    def run(order):
        return e.rerank(seqs[order].reshape(-1), (np.arange(len(order) + 1) * S).astype(np.int32), None)

    full = run(np.arange(N))
    assert np.ptp(full) > 1.0  # the logits differ: equal bits below are no accident
    oracle = mro.logits(w, shape, seqs[:3].reshape(-1), (np.arange(4) * S).astype(np.int32), pooling)
    assert np.abs(full[:3] - oracle).max() <= BAR["f32"]
    for n in (1, 15, 16, 17, 33):
        assert np.array_equal(run(np.arange(n)), full[:n]), n
        tail = np.arange(N - n, N)
        assert np.array_equal(run(tail), full[tail]), n  # the same pairs at other places of other blocks
    perm = rng.permutation(N)
    assert np.array_equal(run(perm), full[perm])
    e.close()


def test_reload_refusals_and_the_embedder_beside_it(gpu):
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd._lib import EngineError

    g, shape, w, pooling = case(GOLDEN[0])
    e = Engine(128)
    emb_shape = mo.ModernShape(2, 128, 2, 256, window=8)
    enc.load_encoder(e, mo.desc_for(emb_shape, "mean", "f16"), mo.random_weights(emb_shape, 4))
    ids, off = g["ids"][: g["offsets"][4]], g["offsets"][:5]
    before = enc.encode(e, ids, off)
    enc.load_reranker(e, mro.desc_for(shape, pooling, "f16"), w)
    scores = e.rerank(g["ids"], g["offsets"], None)
    assert np.array_equal(enc.encode(e, ids, off), before)
    names, body = enc.modernbert_slots({k: v for k, v in w.items() if not k.startswith(("head.", "classifier."))},
                                       mro.desc_for(shape, pooling, "f16"))
    body.update(enc.modernbert_head(w, mro.desc_for(shape, pooling, "f16")))
    for desc, tensors, message in (
            (mro.desc_for(shape, pooling, "f16", normalize=True), names + enc.PRENORM_HEAD_NAMES, "without normalising"),
            (mro.desc_for(shape, pooling, "f16", type_vocab=2), names + enc.PRENORM_HEAD_NAMES, "one token type"),
            (mro.desc_for(shape, pooling, "f16"), names + enc.HEAD_NAMES[2:],
             f"expected {len(names) + 6} tensors, got {len(names) + 2}")):
        with pytest.raises(EngineError, match=message):
            enc._load(e, desc, dict(body, **{"embeddings.token_type_embeddings.weight": np.zeros((desc.type_vocab, 128), np.float32)}),
                      tensors, e._lib.vr_reranker_load)
        assert np.array_equal(e.rerank(g["ids"], g["offsets"], None), scores), message  # the loaded one stays
    with pytest.raises(EngineError, match="sequence 0 has 2000 tokens"):
        e.rerank(np.full(2000, 5, np.int32), np.array([0, 2000], np.int32), None)
    # a post-norm reranker replaces it, and the other way round
    import rerank_oracle as ro
    from oracle import bert as obert

    rshape = obert.BertShape(2, 128, 4, 256, vocab=200, max_pos=64)
    rw = ro.random_weights(rshape, 8)
    enc.load_reranker(e, enc.BertDesc(2, 128, 4, 256, vocab=200, max_pos=64, pooling="cls", normalize=False, precision="f32"), rw)
    rids = np.arange(3, 33, dtype=np.int32)
    want = ro.logits(rw, rshape, rids, np.array([0, 30], np.int32), np.array([11], np.int32))
    assert abs(float(e.rerank(rids, np.array([0, 30], np.int32), np.array([11], np.int32))[0]) - want[0]) <= BAR["f32"]
    enc.load_reranker(e, mro.desc_for(shape, pooling, "f16"), w)
    assert np.array_equal(e.rerank(g["ids"], g["offsets"], None), scores)
    assert np.array_equal(enc.encode(e, ids, off), before)
    e.close()


# ---- a checkpoint directory ------------------------------------------------------------------------------------------------
def _pairs(rng, words, n):
    a = [" ".join(rng.choice(words, size=int(rng.integers(1, 8)))) for _ in range(n)]
    b = [" ".join(rng.choice(words, size=int(rng.integers(0, 90)))) for _ in range(n)]
    return a, b


@pytest.mark.parametrize("pooling,biases", [("mean", False), ("cls", True)])
def test_native_cross_encoder_from_a_directory(gpu, tmp_path, monkeypatch, pooling, biases):
    pytest.importorskip("tokenizers")
    from modernbert_rerank_case import WORDS, reranker_checkpoint

    from voitta_rag_amd import Engine
    from voitta_rag_amd.bpe import BpeTokenizer
    from voitta_rag_amd.reranker import NativeCrossEncoder, sigmoid

    monkeypatch.setenv("VOITTA_RERANK_PRECISION", "f32")
    shape, w, tok = reranker_checkpoint(str(tmp_path / "rr"), pooling, biases, max_length=64)
    e = Engine(128)
    rr = NativeCrossEncoder.from_pretrained(str(tmp_path / "rr"), e)
    assert isinstance(rr.tokenizer, BpeTokenizer) and rr.max_length == 64  # (the native one: vr_rerank_text_bpe)
    assert (rr.desc.norm, rr.desc.pooling, rr.desc.normalize, rr.desc.window, rr.desc.type_vocab) == ("pre", pooling, False, 8, 1)
    rng = np.random.default_rng(5)
    a, b = _pairs(rng, WORDS, 20)
    a[3], b[3], b[4] = "", "", ""
    tok.enable_truncation(max_length=64, strategy="longest_first")
    encs = tok.encode_batch(list(zip(a, b)))
    assert max(len(x.ids) for x in encs) == 64 and min(len(x.ids) for x in encs) <= 6
    ids = np.concatenate([np.asarray(x.ids, np.int32) for x in encs])
    off = np.zeros(len(encs) + 1, np.int32)
    off[1:] = np.cumsum([len(x.ids) for x in encs])
    oracle = mro.logits(w, shape, ids, off, pooling)
    assert np.ptp(oracle) > 1.0  # (not all one value: the comparisons below mean something)
    got = rr.predict(list(zip(a, b)), activation=False)
    assert got.dtype == np.float32 and np.abs(got - oracle).max() <= BAR["f32"]
    assert np.array_equal(got, e.rerank(ids, off, None))  # the token form on the library's ids: the same call, the same bits
    assert np.abs(rr.predict(list(zip(a, b))) - sigmoid(oracle)).max() <= BAR["f32"]
    lists = rr.logits(["vector index", "kernel", "memory"], [b[:5], [], b[5:7]])
    assert [len(x) for x in lists] == [5, 0, 2]
    ranked = rr.rank(a[0], b, top_k=4)
    one = mro.logits(w, shape, *_ids(tok, [a[0]] * len(b), b), pooling)
    assert len(ranked) == 4 and all(x["score"] >= y["score"] for x, y in zip(ranked, ranked[1:]))
    for r in ranked:
        assert abs(r["score"] - sigmoid(one[r["corpus_id"]])) <= BAR["f32"]
    assert ranked[0]["score"] >= sigmoid(one.max()) - BAR["f32"]
    e.close()


def _ids(tok, a, b):
    encs = tok.encode_batch(list(zip(a, b)))
    off = np.zeros(len(encs) + 1, np.int32)
    off[1:] = np.cumsum([len(x.ids) for x in encs])
    return np.concatenate([np.asarray(x.ids, np.int32) for x in encs]), off


# ---- the service path --------------------------------------------------------------------------------------------------------
@pytest.fixture
def reranked(monkeypatch, tmp_path, gpu):
    pytest.importorskip("tokenizers")
    from modernbert_rerank_case import reranker_checkpoint
    from test_query_text_batch_gpu import checkpoint

    from voitta_rag_amd import config, embedding, sparse_embedding, store_registry, vector_store

    path = str(tmp_path / "e5-mini")
    checkpoint(path, 384, 12, "mean")
    rpath = str(tmp_path / "gte-reranker-mini")
    made = reranker_checkpoint(rpath, "mean", False)
    for k, v in (("EMBEDDING_MODEL", path), ("EMBEDDING_DIMENSION", "384"), ("VOITTA_ENCODER_PRECISION", "f16"),
                 ("VOITTA_RERANK_MODEL", rpath), ("VOITTA_RERANK_CANDIDATES", "30"), ("VOITTA_RERANK_PRECISION", "f16")):
        monkeypatch.setenv(k, v)

    def reset():
        config.get_settings.cache_clear()
        store_registry.reset()
        embedding._embedding_service = None
        sparse_embedding._sparse_embedding_service = None
        vector_store._vector_store = None

    reset()
    yield made
    reset()


def test_service_search_is_reranked(reranked):
    from test_query_text_batch_gpu import WORDS, questions

    from voitta_rag_amd.config import get_settings
    from voitta_rag_amd.embedding import get_embedding_service
    from voitta_rag_amd.reranker import get_reranker, sigmoid
    from voitta_rag_amd.sparse_embedding import get_sparse_embedding_service
    from voitta_rag_amd.vector_store import ChunkMetadata, VectorStoreService, get_vector_store

    shape, w, tok = reranked
    bar = BAR["f16"]
    rng = np.random.default_rng(8)
    emb, sp, vs = get_embedding_service(), get_sparse_embedding_service(), get_vector_store()
    texts = [" ".join(rng.choice(WORDS, size=int(rng.integers(3, 60)))) for _ in range(120)]
    metas = [ChunkMetadata(file_path="docs/a.md", folder_path="docs", index_folder="docs", file_name="a.md", chunk_index=i,
                           total_chunks=120, start_char=i, end_char=i + 1, indexed_at="2026-01-01T00:00:00",
                           source_modified_at=1_700_000_000 + i) for i in range(120)]
    vs.store_chunks(list(zip(texts, emb.embed_texts(texts), metas)), sparse_vectors=sp.embed_texts(texts))
    settings = get_settings()
    rr = get_reranker(vs._engine, settings.rerank_model)
    assert rr.desc.prenorm and rr.max_length == 128
    unranked_before = VectorStoreService.unreranked_searches
    qs = questions(rng, 4)
    per_question = []
    for q in qs:
        limit = 7
        got = vs.search(emb.embed_query(q), limit=limit, sparse_query=sp.embed_query(q))
        settings.rerank_model = ""  # the first stage alone: unreranked top-C
        first = vs.search(emb.embed_query(q), limit=30, sparse_query=sp.embed_query(q))
        settings.rerank_model = os.environ["VOITTA_RERANK_MODEL"]
        ids, off, _ = rr.tokenizer.encode_pairs([q] * len(first), [c.text for c in first])
        oracle = mro.logits(w, shape, ids, off.astype(np.int32), "mean")
        order = np.argsort(-oracle, kind="stable")[:limit]
        assert len(got) == min(limit, len(first)) and np.ptp(oracle) > 20 * bar
        for k, c in enumerate(got):
            i = [x.id for x in first].index(c.id)
            assert abs(c.score - sigmoid(oracle[i])) <= bar
            assert c.id == first[order[k]].id or abs(oracle[i] - oracle[order[k]]) <= 2 * bar
        per_question.append(got)
    assert VectorStoreService.unreranked_searches == unranked_before
    batch = vs.search_questions([{"query": q, "limit": 7} for q in qs])
    for got, want in zip(batch, per_question):
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a.id == b.id or abs(a.score - b.score) <= 2 * bar
