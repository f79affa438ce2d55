"""Rotary, gated-FFN encoders (model_type nomic_bert) on the GPU: the transformers goldens at every precision, one batch
per GEMM path against the f64 oracle with mean and CLS pooling, positions that restart per sequence, the longest
sequence and one token more, EmbeddingService / the one-call text paths / deferred indexing on a synthetic
nomic-shaped checkpoint directory in both tensor layouts, and the refusal of rotary or gated rerankers.

In f16 the skinny kernels (at most 256 rows) rotate and gate inside the projections' epilogues and the mid and
ping-pong kernels gate inside theirs; the same batches with VR_ENCODE_FUSE=0, in a fresh child process, run the separate
passes (rope_kernel, glu_kernel)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import bert as obert

import rope_oracle as ro
from test_encoder_gpu import TOL

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "rope_*.npz")))


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


def _engine(shape, pooling, precision, w, max_pos=None):
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    e = Engine(shape.hidden)
    enc.load_encoder(e, ro.desc_for(shape, pooling, precision, max_pos), w)
    return e


# ---- 1. goldens at every precision -----------------------------------------------------------------------------------
def test_goldens_exist():
    assert len(GOLDEN) == 3


@pytest.mark.parametrize("precision", list(TOL))
@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p))
def test_encoder_matches_transformers_golden(gpu, path, precision):
    from voitta_rag_amd import encoder as enc

    g, shape, pooling, w = _case(path)
    e = _engine(shape, pooling, precision, w)
    assert max(np.diff(g["offsets"])) == 512 and min(np.diff(g["offsets"])) == 1
    _check(enc.encode(e, g["ids"], g["offsets"]).astype(np.float64), g["want"], precision, os.path.basename(path))
    # the first and the last sequence alone, twice each: the single-query path, then its cached graph
    for i in (0, len(g["offsets"]) - 2):
        a, b = g["offsets"][i], g["offsets"][i + 1]
        for _ in range(2):
            one = enc.encode(e, g["ids"][a:b], np.array([0, b - a], np.int32)).astype(np.float64)
            _check(one, g["want"][i:i + 1], precision, f"sequence {i} alone")
    e.close()


# ---- 2. one batch per GEMM path ----------------------------------------------------------------------------------------
PATH_SHAPE = ro.RopeShape(2, 128, 2, 256, vocab=300, max_pos=512, act="silu")
# token counts: <= 64 (skinny, one block), 65..256 (skinny, several blocks), 300..1000 (the mid kernel), and more than
# 16384, where at H = 128 every projection has more than CUs / 4 ping-pong tiles (folded LayerNorm, f16 residual stream)
PATH_LENS = {
    "skinny1": [1, 2, 17, 31],
    "skinny4": [64, 65, 15, 16, 63],
    "mid": [129, 300, 1, 200, 77],
    "pingpong": [512, 511, 257, 300, 480, 333, 1, 64] * 7,
}


def path_batches():
    """The seeded weights and, per batch, its sequences (the ping-pong batch repeats its first eight)."""
    w = ro.random_weights(PATH_SHAPE, 21)
    rng = np.random.default_rng(22)
    batches = {}
    for name, lens in PATH_LENS.items():
        seqs = [rng.integers(0, PATH_SHAPE.vocab, size=n).astype(np.int32) for n in lens[:8]]
        batches[name] = (seqs * (len(lens) // len(seqs) + 1))[:len(lens)]
    return w, batches


@pytest.fixture(scope="module")
def path_refs():
    """Per batch: the sequences and the f64 oracle's embeddings for both poolings (computed once, shared, read-only)."""
    w, batches = path_batches()
    refs = {}
    hidden = {}  # the same lengths recur: one oracle pass per distinct sequence
    for name, seqs in batches.items():
        want = {"mean": [], "cls": []}
        for s in seqs:
            key = s.tobytes()
            if key not in hidden:
                hidden[key] = ro.encode_one(w, PATH_SHAPE, s)
            h = hidden[key]
            for pooling, e in (("mean", h.mean(axis=0)), ("cls", h[0])):
                want[pooling].append(e / np.linalg.norm(e))
        refs[name] = (seqs, {k: np.stack(v) for k, v in want.items()})
        for v in refs[name][1].values():
            v.setflags(write=False)
    return w, refs


def test_path_batches_have_the_sizes_that_pick_each_path():
    t = {k: sum(v) for k, v in PATH_LENS.items()}
    assert t["skinny1"] <= 64 and 65 <= t["skinny4"] <= 256 and 300 <= t["mid"] <= 1000 and t["pingpong"] > 16384


@pytest.mark.parametrize("pooling", ["mean", "cls"])
@pytest.mark.parametrize("precision", ["f16", "f32"])
@pytest.mark.parametrize("batch", list(PATH_LENS))
def test_every_gemm_path(gpu, path_refs, batch, precision, pooling):
    from voitta_rag_amd import encoder as enc

    w, refs = path_refs
    seqs, want = refs[batch]
    e = _engine(PATH_SHAPE, pooling, precision, w)
    ids, off = _pack(seqs)
    _check(enc.encode(e, ids, off).astype(np.float64), want[pooling], precision, f"{batch} {pooling}")
    e.close()


# ---- 3. fused equals unfused -------------------------------------------------------------------------------------------
def encode_path_batches(out_path=None):
    """Every batch of (2) at f16 and f32 with both poolings -> {"batch precision pooling": embeddings}; written to
    out_path when given (the child process of the test below)."""
    from voitta_rag_amd import encoder as enc

    w, batches = path_batches()
    out = {}
    for precision in ("f16", "f32"):
        for pooling in ("mean", "cls"):
            e = _engine(PATH_SHAPE, pooling, precision, w)
            for name, seqs in batches.items():
                out[f"{name} {precision} {pooling}"] = enc.encode(e, *_pack(seqs))
            e.close()
    if out_path:
        np.savez(out_path, **out)
    return out


def test_fused_equals_unfused(gpu, tmp_path):
    """VR_ENCODE_FUSE is read whenever a model is loaded; the unfused form is loaded and run in a fresh child process.
    f16: every batch takes a fused epilogue somewhere (the skinny kernels rotate and gate, the mid and ping-pong kernels
    gate), and the two forms differ by the f16 roundings the fused epilogues skip (Q and K once instead of twice, the
    gate's product once instead of three times): within TOL["f16"] of each other, and not equal. f32 never fuses:
    bit-identical."""
    out_path = str(tmp_path / "unfused.npz")
    env = dict(os.environ, VR_ENCODE_FUSE="0")
    code = f"import sys; sys.path[:0] = {[os.path.dirname(HERE), HERE]!r}; import test_rope_gpu as t; t.encode_path_batches({out_path!r})"
    subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=120)
    unfused = np.load(out_path)
    fused = encode_path_batches()
    assert sorted(unfused.files) == sorted(fused)
    differ = []
    for key, got in fused.items():
        if key.split()[1] == "f32":
            assert np.array_equal(got, unfused[key]), key
        else:
            _check(got.astype(np.float64), unfused[key].astype(np.float64), "f16", "fused vs unfused " + key)
            differ.append(not np.array_equal(got, unfused[key]))
    assert len(differ) == 8 and all(differ)  # every f16 batch really took another form


# ---- 4. positions restart per sequence; the table's last row; one token too many -----------------------------------------
@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_positions_restart_per_sequence(gpu, path_refs, precision):
    from voitta_rag_amd import encoder as enc

    w, _ = path_refs
    rng = np.random.default_rng(5)
    probe = rng.integers(0, PATH_SHAPE.vocab, size=40).astype(np.int32)
    long = rng.integers(0, PATH_SHAPE.vocab, size=512).astype(np.int32)
    others = [rng.integers(0, PATH_SHAPE.vocab, size=n).astype(np.int32) for n in (7, 130, 64)]
    e = _engine(PATH_SHAPE, "mean", precision, w)
    ids, off = _pack([probe] + others + [long, probe])
    got = enc.encode(e, ids, off).astype(np.float64)
    _check(got[-1:], got[:1], precision, "same sequence first and last")
    want = ro.sentence_embeddings(w, PATH_SHAPE, [probe, long], "mean")
    _check(got[[0, 4]], want, precision, "first and 512-token sequence vs oracle")  # (the 512th token reads table row 511)
    with pytest.raises(Exception, match="513 tokens"):
        enc.encode(e, np.zeros(513, np.int32), np.array([0, 513], np.int32))
    # the engine is intact after the refusal
    assert np.array_equal(enc.encode(e, ids, off).astype(np.float64), got)
    e.close()


def test_sequences_past_the_staged_attention_limit(gpu):
    """f16 attention stages a whole sequence's keys and values in LDS (attention_seq_kernel) while the longest sequence of
    the call fits a workgroup's LDS: 640 keys at head size 64. 656 tokens, the first multiple of 16 past that, go to the
    streaming kernel (attention_f16_kernel), and so does everything that shares the call; 640 tokens alone still stage.
    Each against the f64 oracle, and each sequence the same alone and in the batch, within TOL["f16"] (the two kernels
    accumulate in different orders: no equal bits across them)."""
    from voitta_rag_amd import encoder as enc

    shape = ro.RopeShape(1, 128, 2, 256, vocab=300, max_pos=1024, act="silu")
    w = ro.random_weights(shape, 31)
    rng = np.random.default_rng(32)
    seqs = [rng.integers(0, shape.vocab, size=n).astype(np.int32) for n in (656, 9, 640)]
    want = ro.sentence_embeddings(w, shape, seqs, "mean")
    e = _engine(shape, "mean", "f16", w)
    together = enc.encode(e, *_pack(seqs)).astype(np.float64)
    _check(together, want, "f16", "656 + 9 + 640 tokens in one call")
    for i in (0, 2):
        alone = enc.encode(e, *_pack([seqs[i]])).astype(np.float64)
        _check(alone, want[i:i + 1], "f16", f"{len(seqs[i])} tokens alone")
        _check(alone, together[i:i + 1], "f16", f"{len(seqs[i])} tokens alone vs in the batch")
    e.close()


def test_missing_biases_are_zeros_and_the_old_description_size_loads(gpu):
    """A plain BERT whose projection biases are absent (NULL slots) equals the same BERT with zero biases, bit for bit;
    and a description that ends at `precision` (the size before the rotary / gated fields) still loads."""
    import ctypes as C

    from voitta_rag_amd import Engine, _lib
    from voitta_rag_amd import encoder as enc

    shape = obert.BertShape(2, 128, 4, 256, vocab=200, max_pos=64)
    w = obert.random_weights(shape, 4)
    names = enc.tensor_names(shape.layers)
    zero = {k: (np.zeros_like(v) if k.endswith("bias") and "LayerNorm" not in k else v) for k, v in w.items()}
    desc = enc.BertDesc(2, 128, 4, 256, vocab=200, max_pos=64, pooling="mean", precision="f32")
    rng = np.random.default_rng(0)
    ids, off = _pack([rng.integers(0, 200, size=n).astype(np.int32) for n in (5, 33, 64)])
    e = Engine(128)
    enc.load_encoder(e, desc, zero)
    want = enc.encode(e, ids, off)
    keep = [np.ascontiguousarray(zero[n], np.float32) for n in names]
    for short in (False, True):
        ptrs = [None if (n.endswith("bias") and "LayerNorm" not in n and not short) else t.ctypes.data
                for n, t in zip(names, keep)]
        cdesc = desc.to_c()
        if short:
            cdesc.struct_size = _lib.VrBertDesc.position.offset
        arr = (C.c_void_p * len(ptrs))(*ptrs)
        _lib.check(e._lib.vr_encoder_load(e.handle, C.byref(cdesc), arr, len(ptrs), _lib.VR_MEM_HOST))
        assert np.array_equal(enc.encode(e, ids, off), want), short
    e.close()


# ---- 5. service level --------------------------------------------------------------------------------------------------
def nomic_checkpoint(d, layout="native", seed=9, layers=2, hidden=384, heads=6, max_seq=8192):
    """A nomic-embed-text-shaped sentence-transformers directory (nomic_bert in the native transformers config layout,
    mean pooling, Normalize) with the WordPiece fixture vocabulary and seeded weights under native or hub names."""
    import test_query_text_batch_gpu as qt

    os.makedirs(os.path.join(d, "1_Pooling"), exist_ok=True)
    vocab = qt._vocab()
    shape = ro.RopeShape(layers, hidden, heads, 4 * hidden, vocab=len(vocab), max_pos=2048, act="silu")
    json.dump({"architectures": ["NomicBertModel"], "model_type": "nomic_bert", "hidden_size": hidden,
               "num_hidden_layers": layers, "num_attention_heads": heads, "intermediate_size": 4 * hidden,
               "vocab_size": len(vocab), "max_position_embeddings": 2048, "type_vocab_size": 2, "layer_norm_eps": 1e-12,
               "hidden_act": "silu", "head_dim": hidden // heads,
               "rope_parameters": {"rope_type": "default", "rope_theta": 1000.0}}, open(os.path.join(d, "config.json"), "w"))
    json.dump([{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
               {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
               {"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}],
              open(os.path.join(d, "modules.json"), "w"))
    json.dump({"word_embedding_dimension": hidden, "pooling_mode_mean_tokens": True},
              open(os.path.join(d, "1_Pooling", "config.json"), "w"))
    json.dump({"max_seq_length": max_seq, "do_lower_case": True}, open(os.path.join(d, "sentence_bert_config.json"), "w"))
    open(os.path.join(d, "vocab.txt"), "w", encoding="utf-8").write("\n".join(vocab) + "\n")
    w = ro.random_weights(shape, seed)
    from safetensors.numpy import save_file

    save_file({k: np.ascontiguousarray(v) for k, v in (ro.hub_state(w, layers) if layout == "hub" else w).items()},
              os.path.join(d, "model.safetensors"))
    return shape, w, vocab


@pytest.fixture
def services(monkeypatch, tmp_path, gpu):
    from voitta_rag_amd import config, embedding, sparse_embedding, store_registry, vector_store

    def make(name="nomic-embed-text", precision="f32", layout="native", prefixes=None):
        path = str(tmp_path / name)
        made = nomic_checkpoint(path, layout)
        monkeypatch.setenv("EMBEDDING_MODEL", path)
        monkeypatch.setenv("EMBEDDING_DIMENSION", "384")
        monkeypatch.setenv("VOITTA_ENCODER_PRECISION", precision)
        for k, v in (prefixes or {}).items():
            monkeypatch.setenv(k, v)
        config.get_settings.cache_clear()
        store_registry.reset()
        embedding._embedding_service = None
        sparse_embedding._sparse_embedding_service = None
        vector_store._vector_store = None
        return made

    yield make
    store_registry.reset()
    config.get_settings.cache_clear()


def _hf_seqs(vocab, texts, max_len=512):
    pytest.importorskip("tokenizers")
    from voitta_rag_amd.embedding import build_wordpiece_tokenizer

    hf = build_wordpiece_tokenizer(vocab, True)
    hf.enable_truncation(max_length=max_len)
    return [np.asarray(e.ids, np.int32) for e in hf.encode_batch(list(texts))]


@pytest.mark.parametrize("layout,prefixes", [
    ("native", None), ("hub", {"VOITTA_EMBED_PASSAGE_PREFIX": "search_document: ", "VOITTA_EMBED_QUERY_PREFIX": "search_query: "})])
def test_embedding_service_on_a_nomic_directory(services, monkeypatch, layout, prefixes):
    from voitta_rag_amd import embedding
    from voitta_rag_amd.wordpiece import WordPieceTokenizer

    monkeypatch.setenv("VOITTA_DEFERRED_INDEXING", "0")
    shape, w, vocab = services(layout=layout, prefixes=prefixes)
    emb = embedding.get_embedding_service()
    assert isinstance(emb.model.tokenizer, WordPieceTokenizer)
    assert emb.model.max_seq_length == 512 and emb.model.desc.max_pos == 512  # 8192 declared, capped
    pp, qp = (prefixes or {}).get("VOITTA_EMBED_PASSAGE_PREFIX", ""), (prefixes or {}).get("VOITTA_EMBED_QUERY_PREFIX", "")
    texts = ["vector database index", "hybrid fusion ranking of sparse and dense retrieval", "kernel", " ".join(["memory bandwidth"] * 400)]
    seqs = _hf_seqs(vocab, [pp + t for t in texts])
    assert max(len(s) for s in seqs) == 512
    _check(np.asarray(emb.embed_texts(texts), np.float64), ro.sentence_embeddings(w, shape, seqs), "f32", "embed_texts")
    q = np.asarray(emb.embed_query("dense retrieval?"), np.float64)[None]
    _check(q, ro.sentence_embeddings(w, shape, _hf_seqs(vocab, [qp + "dense retrieval?"])), "f32", "embed_query")
    assert emb.query_texts(["a"]) == [qp + "a"]


def test_one_call_text_paths(gpu, tmp_path, monkeypatch):
    import test_query_text_batch_gpu as qt

    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    monkeypatch.setenv("VOITTA_ENCODER_PRECISION", "f16")
    path = str(tmp_path / "nomic-embed-text")
    _, _, vocab = nomic_checkpoint(path)
    e = Engine(384)
    model = qt._model(path, e)
    rng = np.random.default_rng(4)
    qt._store(e, model, rng)
    for n in (1, 40, 300):
        texts, sparse, limits, weights, flt = qt.make_batch(rng, n)
        dense_texts = ["search_query: " + t for t in texts]
        seqs = _hf_seqs(vocab, dense_texts, model.max_seq_length)
        ids, off = _pack(seqs)
        want_emb = enc.encode(e, ids, off)
        got, emb = e.query_text_batch(model.tokenizer, dense_texts, sparse, model.max_seq_length, limits, weights, flt,
                                      embeddings=True)
        assert np.array_equal(emb, want_emb), n  # the batch's embeddings are vr_encode's on the same ids
        want = qt.expected(e, emb, sparse, limits, weights, flt, 0)
        assert all(qt.same(got[i], want[i]) for i in range(n)), n
        for i in range(min(n, 5)):  # vr_query_text of question i, bit for bit a batch of one (the same encoder path)
            one = e.query_text(model.tokenizer, dense_texts[i], sparse[i], model.max_seq_length, int(limits[i]),
                               float(weights[i]), 0, flt[i])
            assert qt.same(one, e.query_text_batch(model.tokenizer, [dense_texts[i]], [sparse[i]], model.max_seq_length,
                                                   [limits[i]], [weights[i]], [flt[i]])[0])
    e.close()


def test_deferred_indexing_equals_eager(services, monkeypatch):
    from voitta_rag_amd import deferred, embedding, sparse_embedding, vector_store
    from voitta_rag_amd.vector_store import ChunkMetadata

    import test_query_text_batch_gpu as qt

    rng = np.random.default_rng(6)
    texts = [" ".join(rng.choice(qt.WORDS, size=int(rng.integers(2, 30)))) for _ in range(90)]
    stored = {}
    for defer in (True, False):
        services(f"nomic-embed-text-{int(defer)}", precision="f16")
        monkeypatch.setenv("VOITTA_DEFERRED_INDEXING", "1" if defer else "0")
        emb, sp, vs = (embedding.get_embedding_service(), sparse_embedding.get_sparse_embedding_service(),
                       vector_store.get_vector_store())
        embeddings = emb.embed_texts(texts)
        assert isinstance(embeddings, deferred.DeferredEmbeddings) == defer
        metas = [ChunkMetadata(file_path="d/a.md", folder_path="d", index_folder="d", file_name="a.md", chunk_index=i,
                               total_chunks=len(texts), start_char=0, end_char=1, indexed_at="t",
                               source_modified_at=1_700_000_000 + i) for i in range(len(texts))]
        vs.store_chunks(list(zip(texts, embeddings, metas)), sparse_vectors=sp.embed_texts(texts))
        assert not defer or not embeddings.materialized  # the fused write-behind took them
        q = emb.embed_query("vector search")
        assert isinstance(q, deferred.QueryRef) == defer
        got = vs.search(q, limit=8, sparse_query=sp.embed_query("vector search"))
        stored[defer] = (vs.client.get_dense(np.arange(len(texts))), [(c.metadata.chunk_index, c.score) for c in got])
    d1, d0 = stored[True][0], stored[False][0]
    # (batch composition picks the encoder's code path: f16-level rounding — the bounds of test_xlmr_gpu)
    assert np.max(np.abs(d1 - d0)) < 3e-4 and np.min((d1 * d0).sum(1)) > 1 - 1e-5
    assert [i for i, _ in stored[True][1]][:3] == [i for i, _ in stored[False][1]][:3]


# ---- 6. rotary or gated rerankers are refused ----------------------------------------------------------------------------
def test_rotary_or_gated_reranker_is_refused_and_the_loaded_one_stays(gpu):
    import rerank_oracle as rr

    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    shape = obert.BertShape(2, 128, 4, 256, vocab=200, max_pos=64)
    w = rr.random_weights(shape, 8)
    base = dict(vocab=200, max_pos=64, pooling="cls", normalize=False, precision="f32")
    e = Engine(128)
    enc.load_reranker(e, enc.BertDesc(2, 128, 4, 256, **base), w)
    rng = np.random.default_rng(1)
    ids, off = _pack([rng.integers(0, 200, size=n).astype(np.int32) for n in (9, 30)])
    seg = np.array([4, 11], np.int32)
    before = e.rerank(ids, off, seg)
    for extra in (dict(position="rotary", rope_theta=1000.0), dict(ffn="swiglu"), dict(ffn="geglu")):
        with pytest.raises(Exception, match="rotary positions or a gated FFN"):
            enc.load_reranker(e, enc.BertDesc(2, 128, 4, 256, **base, **extra), w)
        assert np.array_equal(e.rerank(ids, off, seg), before)
    e.close()
