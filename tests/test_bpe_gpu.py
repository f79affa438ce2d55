"""The native byte-level BPE tokenizer on the engine's text paths (vr_rerank_text_bpe, vr_query_text_bpe,
vr_query_text_batch_bpe) and through the services: each equals, bit for bit, the same call on the ids the HF
`tokenizers` library produces for the same texts."""
import json
import os

import numpy as np
import pytest

import bpe_case as bc
import modernbert_rerank_oracle as mro
import test_query_text_batch_gpu as qt

pytestmark = pytest.mark.gpu
N_ROWS = 200


def _hf_ids(hf, texts, max_len, pairs=None):
    hf.enable_truncation(max_length=max_len, strategy="longest_first")
    encs = hf.encode_batch(list(zip(texts, pairs)) if pairs is not None else list(texts))
    off = np.zeros(len(encs) + 1, np.int32)
    off[1:] = np.cumsum([len(e.ids) for e in encs])
    return np.concatenate([np.asarray(e.ids, np.int32) for e in encs]), off


def _texts(rng, n, lo=1, hi=12):
    pool = bc.random_texts(int(rng.integers(1 << 30)), 400)
    return [" ".join(pool[int(i)] for i in rng.integers(0, len(pool), size=int(rng.integers(lo, hi))))[:400] for _ in range(n)]


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_rerank_text_bpe_equals_rerank_on_the_librarys_ids(gpu, precision):
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd.bpe import BpeTokenizer
    import modernbert_oracle as mo

    g = bc.fixture()
    hf = bc.hf_tokenizer(g)
    tok = BpeTokenizer.from_tokenizer_json(g["tokenizer"], 48)
    shape = mo.ModernShape(3, 128, 2, 256, vocab=-(-hf.get_vocab_size() // 8) * 8, max_pos=512, window=8)
    w = mro.random_weights(shape, 9, False, 6.0)
    e = Engine(128)
    enc.load_reranker(e, mro.desc_for(shape, "mean", precision), w)
    rng = np.random.default_rng(2)
    queries = _texts(rng, 5, 1, 4) + [""]
    cands = [_texts(rng, k, 0, 14) for k in (7, 1, 0, 17, 3, 2)]
    cands[0][2], cands[5][0] = "", ""
    got = e.rerank_text(tok, queries, cands, 48)
    assert [len(x) for x in got] == [7, 1, 0, 17, 3, 2]
    a = [q for q, c in zip(queries, cands) for _ in c]
    ids, off = _hf_ids(hf, a, 48, [p for c in cands for p in c])
    assert int(np.diff(off).max()) == 48 and int(np.diff(off).min()) <= 8
    assert np.array_equal(np.concatenate(got), e.rerank(ids, off, None))
    assert np.ptp(np.concatenate(got)) > 0.5
    for max_len in (3, 5):  # nothing but the specials, and two ids of text
        ids, off = _hf_ids(hf, a, max_len, [p for c in cands for p in c])
        assert np.array_equal(np.concatenate(e.rerank_text(tok, queries, cands, max_len)), e.rerank(ids, off, None))
    e.close()


def _store(e, model, rng):
    """N_ROWS rows as test_query_text_batch_gpu stores them: embeddings of chunk texts, BM25 stems, folders, dates."""
    from voitta_rag_amd import bm25

    texts = [" ".join(rng.choice(qt.WORDS, size=int(rng.integers(3, 30)))) for _ in range(N_ROWS)]
    x = qt.encode_list(model, texts)
    off, stems = bm25.hashed_stems(texts)
    sp = []
    for i in range(N_ROWS):
        ids, cnt = np.unique(stems[off[i]: off[i + 1]], return_counts=True)
        sp.append((ids.astype(np.int32), (1.0 + np.log1p(cnt)).astype(np.float32)))
    folder = rng.integers(0, qt.N_FOLDERS, size=N_ROWS).astype(np.int32)
    created = rng.integers(0, 4000, size=N_ROWS).astype(np.int64)
    modified = rng.integers(0, 4000, size=N_ROWS).astype(np.int64)
    created[rng.random(N_ROWS) < 0.1] = qt.ABSENT
    e.upsert(x, sparse=sp, folder_ids=folder, created=created, modified=modified)
    e.delete_rows(rng.choice(N_ROWS, size=15, replace=False))


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_query_text_bpe_and_its_batch_bit_for_bit(gpu, tmp_path, monkeypatch, precision):
    from voitta_rag_amd import Engine, embedding
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd.bpe import BpeTokenizer
    from voitta_rag_amd.sparse_embedding import _query_vector

    # f32: every kernel of the forward pass computes a row from that row's sequence alone, in one order, so a question's
    # embedding has the same bits alone and in a batch, and row i of any batch is the single call. f16 picks its GEMM
    # kernel by the batch's token count (for every tokenizer alike): there the batch equals the separate steps on the
    # batch's own embeddings, and a batch of one equals the single call — what test_query_text_batch_gpu.py asserts for
    # WordPiece. In both, the single call equals tokenise (the library's ids), vr_encode, vr_search_hybrid.
    monkeypatch.setenv("VOITTA_ENCODER_PRECISION", precision)
    path = str(tmp_path / "modernbert-embed-mini")
    shape, w, hf = bc.embedder_checkpoint(path)
    e = Engine(128)
    model = qt._model(path, e)
    assert isinstance(model.tokenizer, BpeTokenizer) and embedding.one_call_text_paths(model) and model.max_seq_length == 64
    rng = np.random.default_rng(4)
    _store(e, model, rng)
    for n in (1, 16, 17):
        texts, sparse, limits, weights, flt = qt.make_batch(rng, n)
        dense_texts = [t + ("  it's é 中文 [MASK] x" if i % 3 == 0 else "") for i, t in enumerate(texts)]
        ids, off = _hf_ids(hf, dense_texts, model.max_seq_length)
        want_emb = enc.encode(e, ids, off)
        got, emb = e.query_text_batch(model.tokenizer, dense_texts, sparse, model.max_seq_length, limits, weights, flt,
                                      embeddings=True)
        assert np.array_equal(emb, want_emb), n
        want = qt.expected(e, emb, sparse, limits, weights, flt, 0)
        assert all(qt.same(got[i], want[i]) for i in range(n)), n  # the separate steps on the batch's embeddings
        for i in range(n):
            one = e.query_text(model.tokenizer, dense_texts[i], sparse[i], model.max_seq_length, int(limits[i]),
                               float(weights[i]), 0, flt[i])
            if precision == "f32":
                assert qt.same(one, got[i]), (n, i)  # row i of the batch is the single call
            alone = e.query_text_batch(model.tokenizer, [dense_texts[i]], [sparse[i]], model.max_seq_length, [limits[i]],
                                       [weights[i]], [flt[i]])[0]
            assert qt.same(one, alone), (n, i)  # a batch of one is the single call
            # ... and the single call is tokenise (the library's ids), vr_encode, vr_search_hybrid
            qi, qv = _query_vector(sparse[i]) if sparse[i] else ([], [])
            one_emb = enc.encode(e, ids[off[i]:off[i + 1]], np.array([0, off[i + 1] - off[i]], np.int32))[0]
            if len(qi):
                r, s, fd = e.search_hybrid(one_emb, np.array(qi, np.int32), np.array(qv, np.float32), int(limits[i]),
                                           float(weights[i]), 0, flt[i])
                assert one[3] and np.array_equal(one[0], r) and np.array_equal(one[1], s) and np.array_equal(one[2], fd), (n, i)
            else:
                assert not one[3]
    e.close()


# ---- services ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def services(monkeypatch, tmp_path, gpu):
    from voitta_rag_amd import config, embedding, sparse_embedding, store_registry, vector_store

    def reset():
        config.get_settings.cache_clear()
        store_registry.reset()
        embedding._embedding_service = None
        sparse_embedding._sparse_embedding_service = None
        vector_store._vector_store = None

    def make(name, native=True, precision="f16"):
        path = str(tmp_path / name)
        made = bc.embedder_checkpoint(path)
        if not native:  # dropout 0.0 never drops a merge, yet is outside the native pipeline: the library tokenises
            spec = json.load(open(os.path.join(path, "tokenizer.json")))
            spec["model"]["dropout"] = 0.0
            json.dump(spec, open(os.path.join(path, "tokenizer.json"), "w"))
        for k, v in (("EMBEDDING_MODEL", path), ("EMBEDDING_DIMENSION", "128"), ("VOITTA_ENCODER_PRECISION", precision)):
            monkeypatch.setenv(k, v)
        reset()
        return made

    yield make
    reset()


def _lists(results):
    return [[(c.metadata.chunk_index, c.score) for c in r] for r in results]


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_services_take_the_native_paths_with_the_librarys_results(services, monkeypatch, precision):
    """embed_query, search_questions and deferred indexing through the native tokenizer (one-call text paths, the fused
    indexing call) against the same services with the tokenizers library (several calls). f32: a row of the forward
    pass depends on its own sequence alone, so the stored vectors, every id and every score bit are equal. f16: the
    routes compose other batches and the encoder picks its GEMM kernel by the batch's token count, so the stored vectors
    agree to f16 rounding (3e-4, as in test_xlmr_gpu); the results are compared in f32 only."""
    from voitta_rag_amd import deferred, embedding, sparse_embedding, vector_store
    from voitta_rag_amd.vector_store import ChunkMetadata

    rng = np.random.default_rng(6)
    texts = [" ".join(rng.choice(qt.WORDS, size=int(rng.integers(2, 30)))) for _ in range(90)]
    questions = ["vector index", "hybrid fusion ranking", "memory bandwidth of a kernel", "it's a  tile [MASK] é"]
    seen = {}
    for native in (True, False):
        services(f"modernbert-{int(native)}", native, precision)
        monkeypatch.setenv("VOITTA_DEFERRED_INDEXING", "1")
        emb, sp, vs = (embedding.get_embedding_service(), sparse_embedding.get_sparse_embedding_service(),
                       vector_store.get_vector_store())
        assert embedding.native_tokenizer(emb.model.tokenizer) == native == embedding.one_call_text_paths(emb.model)
        embeddings = emb.embed_texts(texts)
        assert isinstance(embeddings, deferred.DeferredEmbeddings)  # (tokenised now, by whichever tokenizer)
        metas = [ChunkMetadata(file_path="d/a.md", folder_path="d", index_folder="d", file_name="a.md", chunk_index=i,
                               total_chunks=len(texts), start_char=0, end_char=1, indexed_at="t",
                               source_modified_at=1_700_000_000 + i) for i in range(len(texts))]
        vs.store_chunks(list(zip(texts, embeddings, metas)), sparse_vectors=sp.embed_texts(texts))
        assert not native or not embeddings.materialized  # the fused indexing call took them
        singles = []
        for t in questions:
            q = emb.embed_query(t)
            assert isinstance(q, deferred.QueryRef) == native  # the one-call vr_query_text_bpe path
            singles.append(vs.search(q, limit=8, sparse_query=sp.embed_query(t)))
        batch = vs.search_questions([{"query": t, "limit": 6} for t in questions])
        assert all(len(r) == 8 for r in singles) and all(len(r) == 6 for r in batch)
        seen[native] = (vs.client.get_dense(np.arange(len(texts))), _lists(singles), _lists(batch))
    d1, d0 = seen[True][0], seen[False][0]
    if precision == "f32":
        assert np.array_equal(d1, d0)
        assert seen[True][1] == seen[False][1]  # every id and every score, bit for bit
        assert seen[True][2] == seen[False][2]
    else:
        assert np.max(np.abs(d1 - d0)) < 3e-4 and np.min((d1 * d0).sum(1)) > 1 - 1e-5
