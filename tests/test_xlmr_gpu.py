"""XLM-RoBERTa embedders and rerankers on the GPU: the encoder against the transformers goldens at every precision (a
512-token sequence included, and a 250,002-row vocabulary read near its top), EmbeddingService on a synthetic
multilingual-e5 checkpoint directory, the one-call text paths with the native Unigram tokenizer bit for bit against
HF-tokenised ids through vr_encode and the _multi searches, the deferred indexing path against eager indexing, and the
XLM-R cross-encoder (vr_rerank with seg_b NULL, vr_rerank_text_unigram, the reranked service search)."""
import glob
import json
import os

import numpy as np
import pytest

from oracle import bert as obert

import xlmr_oracle as xo
from test_encoder_gpu import TOL
from test_rerank_gpu import BAR

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EMBED = sorted(p for p in glob.glob(os.path.join(HERE, "golden", "xlmr_*.npz")) if "rerank" not in p)
RERANK = os.path.join(HERE, "golden", "xlmr_rerank_tiny.npz")
TOKENIZER = json.load(open(os.path.join(HERE, "golden", "xlmr_tokenizer.json"), encoding="utf-8"))["tokenizer"]


def _case(path, head=False):
    g = np.load(path)
    L, H, nh, inter, vocab, max_pos, tv = (int(x) for x in g["shape"])
    shape = obert.BertShape(L, H, nh, inter, vocab=vocab, max_pos=max_pos, type_vocab=tv, eps=float(g["eps"]))
    return g, shape, xo.random_weights(shape, int(g["seed"]), head)


def _desc(shape, precision, pooling="mean", normalize=True):
    from voitta_rag_amd import encoder as enc

    return enc.BertDesc(shape.layers, shape.hidden, shape.heads, shape.intermediate, vocab=shape.vocab,
                        max_pos=shape.max_pos - xo.PAD - 1, type_vocab=shape.type_vocab, pooling=pooling,
                        normalize=normalize, eps=shape.eps, precision=precision)


def _check(got, want, precision):
    cos_tol, abs_tol = TOL[precision]
    cos = (got * want).sum(1) / np.linalg.norm(got, axis=1) / np.linalg.norm(want, axis=1)
    assert np.max(np.abs(1 - cos)) < cos_tol, np.max(np.abs(1 - cos))
    assert np.max(np.abs(got - want)) < abs_tol, np.max(np.abs(got - want))


def _hf():
    tokenizers = pytest.importorskip("tokenizers")
    return tokenizers.Tokenizer.from_str(json.dumps(TOKENIZER))


@pytest.mark.parametrize("precision", list(TOL))
@pytest.mark.parametrize("path", EMBED, ids=lambda p: os.path.basename(p))
def test_encoder_matches_transformers_golden(gpu, path, precision):
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd.embedding import slice_positions

    g, shape, w = _case(path)
    e = Engine(shape.hidden)
    enc.load_encoder(e, _desc(shape, precision), slice_positions(w, xo.PAD + 1))
    assert max(np.diff(g["offsets"])) == 512
    _check(enc.encode(e, g["ids"], g["offsets"]).astype(np.float64), g["want"], precision)
    # one at a time: the single-query paths (folded LayerNorm, cached graphs) read the same table, up to row 511
    for i in (0, len(g["offsets"]) - 2):
        a, b = g["offsets"][i], g["offsets"][i + 1]
        for _ in range(2):
            one = enc.encode(e, g["ids"][a:b], np.array([0, b - a], np.int32)).astype(np.float64)
            _check(one, g["want"][i:i + 1], precision)
    e.close()


def test_full_size_vocabulary_ids_near_the_top(gpu):
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd.embedding import slice_positions

    shape = obert.BertShape(1, 128, 2, 256, vocab=250_002, max_pos=514, type_vocab=1, eps=1e-5)
    w = xo.random_weights(shape, 77)
    rng = np.random.default_rng(1)
    seqs = [np.array([0, 250_001, 250_000, 2], np.int32), rng.integers(249_000, 250_002, 512).astype(np.int32),
            rng.integers(0, 250_002, 37).astype(np.int32)]
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    e = Engine(128)
    enc.load_encoder(e, _desc(shape, "f32"), slice_positions(w, xo.PAD + 1))
    _check(enc.encode(e, np.concatenate(seqs), off).astype(np.float64), xo.embeddings(w, shape, seqs), "f32")
    e.close()


# ---- the service paths ---------------------------------------------------------------------------------------------
def e5_checkpoint(d, seed=9, layers=2, hidden=384, heads=12):
    """A multilingual-e5-shaped sentence-transformers directory (XLM-R, mean pooling, Normalize) with the fixture's
    Unigram tokenizer.json and seeded weights (keys without a prefix, as sentence-transformers saves them)."""
    os.makedirs(os.path.join(d, "1_Pooling"), exist_ok=True)
    vocab = len(TOKENIZER["model"]["vocab"])
    shape = obert.BertShape(layers, hidden, heads, 4 * hidden, vocab=vocab, max_pos=514, type_vocab=1, eps=1e-5)
    json.dump({"architectures": ["XLMRobertaModel"], "model_type": "xlm-roberta", "hidden_size": hidden,
               "num_hidden_layers": layers, "num_attention_heads": heads, "intermediate_size": 4 * hidden,
               "vocab_size": vocab, "max_position_embeddings": 514, "type_vocab_size": 1, "layer_norm_eps": 1e-5,
               "hidden_act": "gelu", "pad_token_id": 1, "bos_token_id": 0, "eos_token_id": 2},
              open(os.path.join(d, "config.json"), "w"))
    json.dump([{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
               {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
               {"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}],
              open(os.path.join(d, "modules.json"), "w"))
    json.dump({"word_embedding_dimension": hidden, "pooling_mode_mean_tokens": True},
              open(os.path.join(d, "1_Pooling", "config.json"), "w"))
    json.dump({"max_seq_length": 512, "do_lower_case": False}, open(os.path.join(d, "sentence_bert_config.json"), "w"))
    json.dump(TOKENIZER, open(os.path.join(d, "tokenizer.json"), "w", encoding="utf-8"), ensure_ascii=False)
    w = xo.random_weights(shape, seed)
    from safetensors.numpy import save_file

    save_file(w, os.path.join(d, "model.safetensors"))
    return shape, w


def xlmr_reranker_checkpoint(d, seed=13):
    os.makedirs(d, exist_ok=True)
    vocab = len(TOKENIZER["model"]["vocab"])
    shape = obert.BertShape(2, 384, 12, 1536, vocab=vocab, max_pos=514, type_vocab=1, eps=1e-5)
    json.dump({"architectures": ["XLMRobertaForSequenceClassification"], "model_type": "xlm-roberta", "hidden_size": 384,
               "num_hidden_layers": 2, "num_attention_heads": 12, "intermediate_size": 1536, "vocab_size": vocab,
               "max_position_embeddings": 514, "type_vocab_size": 1, "layer_norm_eps": 1e-5, "hidden_act": "gelu",
               "pad_token_id": 1, "id2label": {"0": "LABEL_0"}}, open(os.path.join(d, "config.json"), "w"))
    json.dump({"model_max_length": 512}, open(os.path.join(d, "tokenizer_config.json"), "w"))
    json.dump(TOKENIZER, open(os.path.join(d, "tokenizer.json"), "w", encoding="utf-8"), ensure_ascii=False)
    w = xo.random_weights(shape, seed, head=True)
    from safetensors.numpy import save_file

    save_file({(k if k.startswith("classifier.") else "roberta." + k): v for k, v in w.items()},
              os.path.join(d, "model.safetensors"))
    return shape, w


@pytest.fixture
def services(monkeypatch, tmp_path, gpu):
    from voitta_rag_amd import config, embedding, sparse_embedding, store_registry, vector_store

    def make(name="multilingual-e5-small", precision="f32", rerank=None):
        path = str(tmp_path / name)
        shape, w = e5_checkpoint(path)
        monkeypatch.setenv("EMBEDDING_MODEL", path)
        monkeypatch.setenv("EMBEDDING_DIMENSION", "384")
        monkeypatch.setenv("VOITTA_ENCODER_PRECISION", precision)
        if rerank:
            monkeypatch.setenv("VOITTA_RERANK_MODEL", rerank)
            monkeypatch.setenv("VOITTA_RERANK_CANDIDATES", "30")
        config.get_settings.cache_clear()
        store_registry.reset()
        embedding._embedding_service = None
        sparse_embedding._sparse_embedding_service = None
        vector_store._vector_store = None
        return shape, w

    yield make
    store_registry.reset()
    config.get_settings.cache_clear()


def _hf_seqs(hf, texts, max_len=512):
    hf.enable_truncation(max_length=max_len, strategy="longest_first")
    return [np.asarray(e.ids, np.int32) for e in hf.encode_batch(list(texts))]


def test_embedding_service_on_a_multilingual_e5_directory(services, monkeypatch):
    from voitta_rag_amd import embedding
    from voitta_rag_amd.unigram import UnigramTokenizer

    monkeypatch.setenv("VOITTA_DEFERRED_INDEXING", "0")
    shape, w = services()
    hf = _hf()
    emb = embedding.get_embedding_service()
    assert isinstance(emb.model.tokenizer, UnigramTokenizer) and emb.model.max_seq_length == 512
    texts = ["Der schnelle braune Fuchs", "敏捷的棕色狐狸 <mask> 跳过", "빠른 갈색 여우", " ".join(["ｆｕｌｌ ﬁne"] * 400)]
    got = np.asarray(emb.embed_texts(texts), np.float64)
    _check(got, xo.embeddings(w, shape, _hf_seqs(hf, ["passage: " + t for t in texts])), "f32")
    q = np.asarray(emb.embed_query("Быстрая лиса?"), np.float64)[None]
    _check(q, xo.embeddings(w, shape, _hf_seqs(hf, ["query: Быстрая лиса?"])), "f32")


def test_one_call_paths_equal_hf_ids_through_encode_and_multi(gpu, tmp_path, monkeypatch):
    import test_query_text_batch_gpu as qt

    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    monkeypatch.setenv("VOITTA_ENCODER_PRECISION", "f16")
    path = str(tmp_path / "multilingual-e5-small")
    e5_checkpoint(path)
    e = Engine(384)
    model = qt._model(path, e)
    hf = _hf()
    rng = np.random.default_rng(4)
    qt._store(e, model, rng)
    for n in (1, 40, 700):
        texts, sparse, limits, weights, flt = qt.make_batch(rng, n)
        dense_texts = ["query: " + t + (" 中文 한국어" if i % 3 == 0 else "") for i, t in enumerate(texts)]
        seqs = _hf_seqs(hf, dense_texts, model.max_seq_length)
        off = np.zeros(n + 1, np.int32)
        off[1:] = np.cumsum([len(s) for s in seqs])
        want_emb = enc.encode(e, np.concatenate(seqs), off)
        for fusion in (0, 1):
            got, emb = e.query_text_batch(model.tokenizer, dense_texts, sparse, model.max_seq_length, limits, weights, flt,
                                          fusion=fusion, embeddings=True)
            assert np.array_equal(emb, want_emb), n
            want = qt.expected(e, emb, sparse, limits, weights, flt, fusion)
            assert all(qt.same(got[i], want[i]) for i in range(n)), (n, fusion)
        for i in range(min(n, 5)):
            one = e.query_text(model.tokenizer, dense_texts[i], sparse[i], model.max_seq_length, int(limits[i]),
                               float(weights[i]), 0, flt[i])
            assert qt.same(one, e.query_text_batch(model.tokenizer, [dense_texts[i]], [sparse[i]], model.max_seq_length,
                                                   [limits[i]], [weights[i]], [flt[i]])[0])
    e.close()


def test_deferred_indexing_and_query_take_the_native_paths(services, monkeypatch):
    from voitta_rag_amd import deferred, embedding, sparse_embedding, vector_store
    from voitta_rag_amd.vector_store import ChunkMetadata

    rng = np.random.default_rng(6)
    words = "Fuchs лиса 狐狸 여우 renard zorro αλεπού fox dog Hund собака 狗 개 chien perro".split()
    texts = [" ".join(rng.choice(words, size=int(rng.integers(2, 30)))) for _ in range(90)]
    stored = {}
    for defer in (True, False):
        services(f"multilingual-e5-small-{int(defer)}", precision="f16")
        monkeypatch.setenv("VOITTA_DEFERRED_INDEXING", "1" if defer else "0")
        emb, sp, vs = (embedding.get_embedding_service(), sparse_embedding.get_sparse_embedding_service(),
                       vector_store.get_vector_store())
        embeddings = emb.embed_texts(texts)
        assert isinstance(embeddings, deferred.DeferredEmbeddings) == defer
        metas = [ChunkMetadata(file_path="d/a.md", folder_path="d", index_folder="d", file_name="a.md", chunk_index=i,
                               total_chunks=len(texts), start_char=0, end_char=1, indexed_at="t",
                               source_modified_at=1_700_000_000 + i) for i in range(len(texts))]
        vs.store_chunks(list(zip(texts, embeddings, metas)), sparse_vectors=sp.embed_texts(texts))
        assert not defer or not embeddings.materialized  # the fused path took them
        q = emb.embed_query("лиса fox")
        assert isinstance(q, deferred.QueryRef) == defer  # the one-call vr_query_text path for a Unigram model
        got = vs.search(q, limit=8, sparse_query=sp.embed_query("лиса fox"))
        stored[defer] = (vs.client.get_dense(np.arange(len(texts))), [(c.metadata.chunk_index, c.score) for c in got])
    d1, d0 = stored[True][0], stored[False][0]
    # (batch composition picks the encoder's code path: f16-level rounding, as in test_services_gpu)
    assert np.max(np.abs(d1 - d0)) < 3e-4 and np.min((d1 * d0).sum(1)) > 1 - 1e-5
    assert [i for i, _ in stored[True][1]][:3] == [i for i, _ in stored[False][1]][:3]


@pytest.mark.parametrize("precision", list(BAR))
def test_xlmr_reranker_logits(gpu, precision):
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd.embedding import slice_positions
    from voitta_rag_amd.reranker import XLMR_HEAD

    g, shape, w = _case(RERANK, head=True)
    state = slice_positions(w, xo.PAD + 1)
    for head, name in XLMR_HEAD.items():
        state[head] = state.pop(name)
    e = Engine(shape.hidden)
    enc.load_reranker(e, _desc(shape, precision, "cls", False), state)
    got = e.rerank(g["ids"], g["offsets"], None).astype(np.float64)
    assert np.abs(got - g["want"]).max() <= BAR[precision]
    # a seg_b is ignored by a one-type model: the same bits
    seg = np.diff(g["offsets"]).astype(np.int32) // 2 + 1
    assert np.array_equal(e.rerank(g["ids"], g["offsets"], seg), got.astype(np.float32))
    # the text call with the native Unigram pair encoder: bit for bit what vr_rerank gives on HF's ids
    from voitta_rag_amd.unigram import UnigramTokenizer

    hf = _hf()
    tok = UnigramTokenizer.from_tokenizer_json(TOKENIZER, int(g["max_len"]))
    co = g["cand_off"]
    queries, passages = [str(q) for q in g["queries"]], [str(p) for p in g["passages"]]
    cands = [passages[co[i]:co[i + 1]] for i in range(len(queries))]
    text = np.concatenate(e.rerank_text(tok, queries, cands, int(g["max_len"])))
    hf.enable_truncation(max_length=int(g["max_len"]), strategy="longest_first")
    encs = hf.encode_batch([(q, p) for q, c in zip(queries, cands) for p in c])
    ids = np.concatenate([np.asarray(x.ids, np.int32) for x in encs])
    off = np.zeros(len(encs) + 1, np.int32)
    off[1:] = np.cumsum([len(x.ids) for x in encs])
    assert np.array_equal(ids, g["ids"]) and np.array_equal(off, g["offsets"])
    assert np.array_equal(text, e.rerank(ids, off, None))
    e.close()


def test_service_search_reranked_by_an_xlmr_cross_encoder(services, tmp_path, monkeypatch):
    from voitta_rag_amd import embedding, sparse_embedding, vector_store
    from voitta_rag_amd.config import get_settings
    from voitta_rag_amd.reranker import NativeCrossEncoder, get_reranker, sigmoid
    from voitta_rag_amd.unigram import UnigramTokenizer
    from voitta_rag_amd.vector_store import ChunkMetadata

    monkeypatch.setenv("VOITTA_DEFERRED_INDEXING", "0")
    monkeypatch.setenv("VOITTA_RERANK_PRECISION", "f32")
    rpath = str(tmp_path / "bge-reranker-mini")
    rshape, rw = xlmr_reranker_checkpoint(rpath)
    services(precision="f16", rerank=rpath)
    emb, sp, vs = embedding.get_embedding_service(), sparse_embedding.get_sparse_embedding_service(), vector_store.get_vector_store()
    rng = np.random.default_rng(2)
    words = "Fuchs лиса 狐狸 여우 renard zorro fox dog Hund собака chien perro brown quick".split()
    texts = [" ".join(rng.choice(words, size=int(rng.integers(2, 25)))) for _ in range(80)]
    metas = [ChunkMetadata(file_path="d/a.md", folder_path="d", index_folder="d", file_name="a.md", chunk_index=i,
                           total_chunks=80, start_char=0, end_char=1, indexed_at="t", source_modified_at=1_700_000_000 + i)
             for i in range(80)]
    vs.store_chunks(list(zip(texts, emb.embed_texts(texts), metas)), sparse_vectors=sp.embed_texts(texts))
    rr = get_reranker(vs._engine, get_settings().rerank_model)
    assert isinstance(rr, NativeCrossEncoder) and isinstance(rr.tokenizer, UnigramTokenizer) and rr.max_length == 512
    for q in ("quick brown лиса", "Hund 狐狸 zorro"):
        got = vs.search(emb.embed_query(q), limit=6, sparse_query=sp.embed_query(q))
        assert len(got) == 6
        ids, off, _ = rr.tokenizer.encode_pairs([q] * len(got), [c.text for c in got])
        oracle = sigmoid(xo.logits(rw, rshape, ids, off.astype(np.int32)))
        assert np.abs(np.array([c.score for c in got]) - oracle).max() <= BAR["f32"]
        assert all(a.score >= b.score for a, b in zip(got, got[1:]))


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_xlmr_reranker_at_512_tokens(gpu, precision):
    """Pairs truncated LongestFirst to exactly 512 tokens: the reranker reads position rows up to 513 of the
    checkpoint's table (row 511 of the sliced one), against the f64 oracle."""
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd.embedding import slice_positions
    from voitta_rag_amd.reranker import XLMR_HEAD
    from voitta_rag_amd.unigram import UnigramTokenizer

    _, shape, w = _case(RERANK, head=True)
    state = slice_positions(w, xo.PAD + 1)
    for head, name in XLMR_HEAD.items():
        state[head] = state.pop(name)
    e = Engine(shape.hidden)
    enc.load_reranker(e, _desc(shape, precision, "cls", False), state)
    tok = UnigramTokenizer.from_tokenizer_json(TOKENIZER, 512)
    long = " ".join(["Der schnelle braune Fuchs springt über den faulen Hund. 빠른 갈색 여우"] * 60)
    queries = ["Быстрая лиса", long]
    cands = [[long, "kurz"], [long, "short passage"]]
    got = np.concatenate(e.rerank_text(tok, queries, cands, 512)).astype(np.float64)
    ids, off, _ = tok.encode_pairs([q for q, c in zip(queries, cands) for _ in c], [p for c in cands for p in c])
    assert max(np.diff(off)) == 512 and (np.diff(off) == 512).sum() >= 2
    assert np.abs(got - xo.logits(w, shape, ids, off.astype(np.int32))).max() <= BAR[precision]
    e.close()
