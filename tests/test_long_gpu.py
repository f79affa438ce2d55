"""Sequences of up to 8192 tokens on the GPU (VOITTA_MAX_SEQ_LENGTH): the long goldens of tests/golden/make_long_golden.py
at every precision — in f16 the lengths past the staged attention's LDS limit run attention_stream_kernel, at head
sizes 64 (mean pooling) and 32 (CLS pooling: the last layer computes query block 0 alone) — a long sequence alone and
beside short ones, learned position tables of 8192 rows (XLM-R embedder and cross-encoder), and EmbeddingService and the
one-call text path on a nomic directory with the cap raised to 2048."""
import glob
import os

import numpy as np
import pytest

from oracle import bert as obert

import rope_oracle as ro
import xlmr_oracle as xo
from test_encoder_gpu import TOL
from test_rerank_gpu import BAR

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "long_rope_*.npz")))
STAGED_KEYS = {64: 640, 32: 1280}  # the longest sequence attention_seq_kernel stages, by head size


def _case(path):
    g = np.load(path)
    L, H, nh, inter, vocab, max_pos, tv = (int(x) for x in g["shape"])
    shape = ro.RopeShape(L, H, nh, inter, vocab=vocab, max_pos=max_pos, type_vocab=tv, eps=float(g["eps"]),
                         theta=float(g["theta"]), act=str(g["act"]))
    return g, shape, str(g["pooling"]), ro.random_weights(shape, int(g["seed"]))


def _check(got, want, precision, what=""):
    cos_tol, abs_tol = TOL[precision]
    cos = (got * want).sum(1) / np.linalg.norm(got, axis=1) / np.linalg.norm(want, axis=1)
    worst, worst_abs = float(np.max(np.abs(1 - cos))), float(np.max(np.abs(got - want)))
    print(f"{what} {precision}: worst |1-cos| = {worst:.3e}, worst abs diff = {worst_abs:.3e}")
    assert worst < cos_tol, worst
    assert worst_abs < abs_tol, worst_abs


def _pack(seqs):
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs).astype(np.int32), off


def _engine(shape, pooling, precision, w):
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    e = Engine(shape.hidden)
    enc.load_encoder(e, ro.desc_for(shape, pooling, precision), w)
    return e


# ---- 1. golden parity ------------------------------------------------------------------------------------------------
def test_goldens_exist():
    assert [os.path.basename(p) for p in GOLDEN] == ["long_rope_d32.npz", "long_rope_d64.npz"]


@pytest.mark.parametrize("precision", list(TOL))
@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p))
def test_encoder_matches_the_long_golden(gpu, path, precision):
    """All sequences in one call (the 8192-token one sends every sequence of the call to the streaming kernel in f16),
    then each sequence too long to stage alone."""
    from voitta_rag_amd import encoder as enc

    g, shape, pooling, w = _case(path)
    assert shape.max_pos == 8192 and max(np.diff(g["offsets"])) == 8192
    e = _engine(shape, pooling, precision, w)
    name = os.path.basename(path)
    _check(enc.encode(e, g["ids"], g["offsets"]).astype(np.float64), g["want"], precision, f"{name}, one call")
    staged = STAGED_KEYS[shape.hidden // shape.heads]
    for i in range(len(g["offsets"]) - 1):
        a, b = int(g["offsets"][i]), int(g["offsets"][i + 1])
        if b - a > staged:
            one = enc.encode(e, g["ids"][a:b], np.array([0, b - a], np.int32)).astype(np.float64)
            _check(one, g["want"][i:i + 1], precision, f"{name}, {b - a} tokens alone")
    e.close()


# ---- 2. alone and in a batch -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16", "f32"])
@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p))
def test_a_long_sequence_alone_and_beside_short_ones(gpu, path, precision):
    """The 2049-token sequence of the golden alone, and in one call with sequences of 1, 17 and 64 tokens (which then
    leave the staged kernel for the streaming one in f16): within TOL of the oracle and of each other; f32 bit for bit."""
    from voitta_rag_amd import encoder as enc

    g, shape, pooling, w = _case(path)
    lens = np.diff(g["offsets"]).tolist()
    seq = lambda n: g["ids"][g["offsets"][lens.index(n)]:g["offsets"][lens.index(n) + 1]]  # noqa: E731
    extra = np.random.default_rng(5).integers(0, shape.vocab, size=64).astype(np.int32)
    seqs = [seq(1), seq(2049), seq(17), extra]
    want = np.concatenate([g["want"][[lens.index(1), lens.index(2049), lens.index(17)]],
                           ro.sentence_embeddings(w, shape, [extra], pooling)])
    e = _engine(shape, pooling, precision, w)
    together = enc.encode(e, *_pack(seqs))
    _check(together.astype(np.float64), want, precision, "1 + 2049 + 17 + 64 tokens in one call")
    alone = enc.encode(e, *_pack([seqs[1]]))
    _check(alone.astype(np.float64), want[1:2], precision, "2049 tokens alone")
    _check(alone.astype(np.float64), together[1:2].astype(np.float64), precision, "2049 tokens alone vs in the batch")
    if precision == "f32":
        assert np.array_equal(alone[0], together[1])
    e.close()


# ---- 3. learned position tables of 8192 rows ---------------------------------------------------------------------------
XLMR_SHAPE = obert.BertShape(1, 128, 2, 256, vocab=300, max_pos=8194, type_vocab=1, eps=1e-5)


def _xlmr_desc(precision, pooling="mean", normalize=True):
    from voitta_rag_amd import encoder as enc

    s = XLMR_SHAPE
    return enc.BertDesc(s.layers, s.hidden, s.heads, s.intermediate, vocab=s.vocab, max_pos=s.max_pos - xo.PAD - 1,
                        type_vocab=1, pooling=pooling, normalize=normalize, eps=s.eps, precision=precision)


@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_xlmr_embedder_with_8192_position_rows(gpu, precision):
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd.embedding import slice_positions

    w = xo.random_weights(XLMR_SHAPE, 51)
    rng = np.random.default_rng(52)
    seqs = [rng.integers(0, XLMR_SHAPE.vocab, size=n).astype(np.int32) for n in (656, 2049)]
    want = xo.embeddings(w, XLMR_SHAPE, seqs)
    e = Engine(XLMR_SHAPE.hidden)
    desc = _xlmr_desc(precision)
    assert desc.max_pos == 8192
    enc.load_encoder(e, desc, slice_positions(w, xo.PAD + 1))
    _check(enc.encode(e, *_pack(seqs)).astype(np.float64), want, precision, "XLM-R 656 + 2049 tokens")
    e.close()


@pytest.mark.parametrize("precision", list(BAR))
def test_xlmr_cross_encoder_scores_a_long_pair(gpu, precision):
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd.embedding import slice_positions
    from voitta_rag_amd.reranker import XLMR_HEAD

    w = xo.random_weights(XLMR_SHAPE, 53, head=True)
    rng = np.random.default_rng(54)
    # <s> question </s> </s> passage </s>: 700 tokens, and a short pair beside it
    pair = lambda nq, npass: np.concatenate([[0], rng.integers(4, 300, nq), [2, 2], rng.integers(4, 300, npass), [2]])  # noqa: E731
    ids, off = _pack([pair(20, 676).astype(np.int32), pair(5, 9).astype(np.int32)])
    assert off[1] == 700
    want = xo.logits(w, XLMR_SHAPE, ids, off)
    state = slice_positions(w, xo.PAD + 1)
    for head, name in XLMR_HEAD.items():
        state[head] = state.pop(name)
    e = Engine(XLMR_SHAPE.hidden)
    enc.load_reranker(e, _xlmr_desc(precision, "cls", False), state)
    got = e.rerank(ids, off, None).astype(np.float64)
    print(f"{precision}: max |logit - oracle| = {np.abs(got - want).max():.3e}")
    assert np.abs(got - want).max() <= BAR[precision]
    e.close()


# ---- 4. services ---------------------------------------------------------------------------------------------------------
def test_embedding_service_embeds_past_512_tokens_when_the_cap_is_raised(gpu, tmp_path, monkeypatch):
    """VOITTA_MAX_SEQ_LENGTH=2048 on a nomic directory that declares 2048 positions: a text of about 1500 tokens is
    embedded whole (vr_encode of its un-truncated ids, not of the first 512), and vr_query_text(_batch) of the same
    text answers with that embedding's search result."""
    pytest.importorskip("tokenizers")
    import test_query_text_batch_gpu as qt
    from test_rope_gpu import _hf_seqs, nomic_checkpoint

    from voitta_rag_amd import config, embedding, store_registry
    from voitta_rag_amd import encoder as enc

    path = str(tmp_path / "nomic-embed-text")
    _, _, vocab = nomic_checkpoint(path)
    for k, v in (("EMBEDDING_MODEL", path), ("EMBEDDING_DIMENSION", "384"), ("VOITTA_ENCODER_PRECISION", "f16"),
                 ("VOITTA_DEFERRED_INDEXING", "0"), ("VOITTA_MAX_SEQ_LENGTH", "2048")):
        monkeypatch.setenv(k, v)
    config.get_settings.cache_clear()
    store_registry.reset()
    embedding._embedding_service = None
    try:
        emb = embedding.get_embedding_service()
        model = emb.model
        assert model.max_seq_length == 2048 and model.desc.max_pos == 2048
        text = " ".join(["memory bandwidth of the wavefront"] * 300)
        ids = _hf_seqs(vocab, [text], 2048)[0]
        assert 1400 <= len(ids) <= 1600
        e = model.engine
        whole = enc.encode(e, *_pack([ids]))
        got = np.asarray(emb.embed_texts([text]), np.float32)
        assert np.array_equal(got, whole)
        first512 = enc.encode(e, *_pack([np.concatenate([ids[:511], ids[-1:]])]))  # what a cap of 512 embeds
        assert np.max(np.abs(whole - first512)) > 1e-3
        # the one-call text path: the same embedding, and its search result
        qt._store(e, model, np.random.default_rng(4))
        limits, weights = np.array([10], np.int32), np.array([0.1])
        res, qemb = e.query_text_batch(model.tokenizer, [text], [text], model.max_seq_length, limits, weights, [None],
                                       embeddings=True)
        assert np.array_equal(qemb, whole)
        want = qt.expected(e, qemb, [text], limits, weights, [None], 0)
        assert qt.same(res[0], want[0])
        one = e.query_text(model.tokenizer, text, text, model.max_seq_length, 10, 0.1, 0, None)
        assert qt.same(one, want[0])
    finally:
        store_registry.reset()
        config.get_settings.cache_clear()
        embedding._embedding_service = None


# ---- 5. the text calls' id buffers: sized by the texts' bytes, one retry with the tokenizer's own count -------------------
def test_text_calls_retry_when_the_ids_outnumber_the_bytes(gpu):
    """vr_query_text_batch and vr_rerank_text reserve one id per byte of text (+ the specials). A Unigram vocabulary
    without the prefixed piece of a word gives more: 'c' (one byte) is the lone Metaspace piece and an unknown, four ids
    with <s> and </s>. The call then asks the tokenizer again with the count it reported: the embeddings are vr_encode's
    and the logits vr_rerank's on the ids HF `tokenizers` gives."""
    tokenizers = pytest.importorskip("tokenizers")
    import json

    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd.embedding import slice_positions
    from voitta_rag_amd.reranker import XLMR_HEAD
    from voitta_rag_amd.unigram import UnigramTokenizer

    fixture = json.load(open(os.path.join(HERE, "golden", "xlmr_tokenizer.json"), encoding="utf-8"))
    spec = xo.tokenizer_spec(fixture, "ties")
    hf = tokenizers.Tokenizer.from_str(json.dumps(spec))
    hf.enable_truncation(max_length=64, strategy="longest_first")
    tok = UnigramTokenizer.from_tokenizer_json(spec, 64)
    texts = ["c", "c c", "b c"]
    seqs = [np.asarray(x.ids, np.int32) for x in hf.encode_batch(texts)]
    assert sum(len(s) for s in seqs) > sum(len(t.encode()) + 2 for t in texts)  # more ids than the first attempt reserves
    w = xo.random_weights(XLMR_SHAPE, 55, head=True)
    state = slice_positions(w, xo.PAD + 1)
    e = Engine(XLMR_SHAPE.hidden)
    enc.load_encoder(e, _xlmr_desc("f32"), {k: v for k, v in state.items() if not k.startswith("classifier.")})
    e.upsert(np.random.default_rng(56).standard_normal((40, XLMR_SHAPE.hidden)).astype(np.float32))
    n = len(texts)
    res, emb = e.query_text_batch(tok, texts, [None] * n, 64, np.full(n, 5, np.int32), np.zeros(n), [None] * n,
                                  embeddings=True)
    assert np.array_equal(emb, enc.encode(e, *_pack(seqs))) and all(len(r[0]) == 5 for r in res)
    one = e.query_text(tok, texts[0], None, 64, 5, 0.0, 0, None)
    assert np.array_equal(one[0], res[0][0]) and np.array_equal(one[1], res[0][1])
    # pairs: 'c' + 'c' is 2 + 2 ids and four specials against 1 + 1 bytes + 4
    pairs = [np.asarray(x.ids, np.int32) for x in hf.encode_batch([("c", "c"), ("c", "b c")])]
    assert sum(len(p) for p in pairs) > (1 + 1 + 4) + (1 + 3 + 4)
    for head, name in XLMR_HEAD.items():
        state[head] = state.pop(name)
    enc.load_reranker(e, _xlmr_desc("f32", "cls", False), state)
    got = e.rerank_text(tok, ["c"], [["c", "b c"]], 64)[0]
    assert np.array_equal(got, e.rerank(*_pack(pairs), None))
    e.close()


# ---- 6. a cap above what vr_query_text(_batch) accept: questions go through encode + search ------------------------------
def test_services_with_the_cap_at_8192_answer_questions_without_the_one_call_paths(gpu, tmp_path, monkeypatch):
    """VOITTA_MAX_SEQ_LENGTH=8192 on a nomic directory that declares 8192 positions: max_seq_length is 8192, above the
    4096 the one-call text paths take, so embed_query encodes at once (no QueryRef) and search_questions goes through
    embed_queries + search_requests. A question of more than 4096 tokens is embedded whole."""
    pytest.importorskip("tokenizers")
    import json

    import test_query_text_batch_gpu as qt
    from test_rope_gpu import _hf_seqs, nomic_checkpoint

    from voitta_rag_amd import config, deferred, embedding, sparse_embedding, store_registry, vector_store
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd.sparse_embedding import _query_vector
    from voitta_rag_amd.vector_store import ChunkMetadata

    path = str(tmp_path / "nomic-embed-text")
    _, _, vocab = nomic_checkpoint(path)
    cfg = json.load(open(os.path.join(path, "config.json")))
    cfg["max_position_embeddings"] = 8192  # rotary: no table depends on it
    json.dump(cfg, open(os.path.join(path, "config.json"), "w"))
    for k, v in (("EMBEDDING_MODEL", path), ("EMBEDDING_DIMENSION", "384"), ("VOITTA_ENCODER_PRECISION", "f16"),
                 ("VOITTA_DEFERRED_INDEXING", "1"), ("VOITTA_MAX_SEQ_LENGTH", "8192")):
        monkeypatch.setenv(k, v)

    def reset():
        config.get_settings.cache_clear()
        store_registry.reset()
        embedding._embedding_service = None
        sparse_embedding._sparse_embedding_service = None
        vector_store._vector_store = None

    reset()
    try:
        emb, sp, vs = (embedding.get_embedding_service(), sparse_embedding.get_sparse_embedding_service(),
                       vector_store.get_vector_store())
        model = emb.model
        assert model.max_seq_length == 8192 and model.desc.max_pos == 8192
        assert embedding.native_tokenizer(model.tokenizer) and not embedding.one_call_text_paths(model)
        rng = np.random.default_rng(7)
        texts = [" ".join(rng.choice(qt.WORDS, size=int(rng.integers(3, 30)))) for _ in range(60)]
        metas = [ChunkMetadata(file_path="d/a.md", folder_path="d", index_folder="d", file_name="a.md", chunk_index=i,
                               total_chunks=len(texts), start_char=0, end_char=1, indexed_at="t",
                               source_modified_at=1_700_000_000 + i) for i in range(len(texts))]
        vs.store_chunks(list(zip(texts, emb.embed_texts(texts), metas)), sparse_vectors=sp.embed_texts(texts))
        long_q = " ".join(["memory bandwidth of the wavefront"] * 900)
        q = emb.embed_query(long_q)
        assert not isinstance(q, deferred.QueryRef)
        ids = _hf_seqs(vocab, [long_q], 8192)[0]
        assert 4400 <= len(ids) <= 4600
        whole = enc.encode(model.engine, *_pack([ids]))
        assert np.array_equal(np.asarray(q, np.float32)[None], whole)
        cut = enc.encode(model.engine, *_pack([np.concatenate([ids[:4095], ids[-1:]])]))  # what max_len 4096 would embed
        assert np.max(np.abs(whole - cut)) > 1e-5
        reqs = [{"query": long_q, "limit": 5}, {"query": "vector search", "limit": 8, "sparse_weight": 1.0},
                {"query": "kernel memory", "limit": 3, "folder_filter": "d"}]
        got = vs.search_questions(reqs)
        vecs = emb.embed_queries([r["query"] for r in reqs])
        ref = vs.search_requests([dict({a: v for a, v in r.items() if a != "query"}, query_embedding=vecs[i],
                                       sparse_query=_query_vector(r["query"])) for i, r in enumerate(reqs)])
        for g, w_, r in zip(got, ref, reqs):
            assert len(g) == r["limit"] and [(c.id, c.score) for c in g] == [(c.id, c.score) for c in w_], r["query"][:30]
        one = vs.search(q, limit=5, sparse_query=sp.embed_query(long_q))
        assert len(one) == 5
    finally:
        reset()
