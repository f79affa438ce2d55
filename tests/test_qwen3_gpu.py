"""Qwen3 decoder embedders on the GPU, through the C ABI against tests/qwen3_oracle.py at test_encoder_gpu.TOL: head size
128 in the three attention kernels (staged up to 320 keys, streamed beyond, the f32 kernel) with every query row an
output, an attention width that is not the hidden size on every GEMM route, the per-head Q/K norm fused with the
rotation (qk_norm_rope_kernel) — against the oracle, as a causality property and as batch invariance, bit for bit —
the refusals, and the services on a synthetic qwen3 checkpoint directory. Every test here fails without the feature
(BertDesc has no head_dim; through the C ABI: "vr_bert_desc size mismatch", "head size 128 unsupported")."""
import ctypes as C

import numpy as np
import pytest

import qwen3_oracle as qo
from test_encoder_gpu import TOL
from test_modernbert_gpu import PATH_LENS
from test_qwen3_cpu import GOLDENS, golden

pytestmark = pytest.mark.gpu
POOLINGS = ("last", "mean", "cls")
NAMES = [g[0] for g in GOLDENS]


def _check(got, want, precision, what=""):
    cos_tol, abs_tol = TOL[precision]
    assert np.isfinite(got).all(), what
    cos = (got * want).sum(1) / np.linalg.norm(got, axis=1) / np.linalg.norm(want, axis=1)
    worst, worst_abs = float(np.max(np.abs(1 - cos))), float(np.max(np.abs(got - want)))
    print(f"{what} {precision}: worst |1-cos| = {worst:.3e}, worst abs diff = {worst_abs:.3e}")
    assert worst < cos_tol, worst
    assert worst_abs < abs_tol, worst_abs


def _pack(seqs):
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs).astype(np.int32), off


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _engine(shape, pooling, precision, w, **over):
    """An engine with the model loaded through load_encoder (qwen3_slots: the NULL slots, the repeated K/V heads, the norms)."""
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    e = Engine(shape.hidden)
    enc.load_encoder(e, qo.desc_for(shape, pooling, precision, **over), w)
    return e


def _token_rows(e, seqs, positions=None):
    """vr_encode_spans rows of the single-token spans [t, t + 1), t in positions[i] (default: every token), of sequence i."""
    from voitta_rag_amd import encoder as enc

    positions = positions or [range(len(s)) for s in seqs]
    ids, off = _pack(seqs)
    span_off = np.zeros(len(seqs) + 1, np.int32)
    span_off[1:] = np.cumsum([len(p) for p in positions])
    tok = np.asarray([(t, t + 1) for p in positions for t in p], np.int32).reshape(-1, 2)
    return enc.encode_spans(e, ids, off, span_off, tok)


def _unit(rows):
    return rows / np.linalg.norm(rows, axis=-1, keepdims=True)


# ---- 1, 2. the goldens' shapes at every precision and pooling, causal and bidirectional ----------------------------------
@pytest.fixture(scope="module")
def golden_refs():
    """Per golden: shape, weights, sequences, the oracle's final hidden states per sequence, causal and bidirectional
    (once, read-only); the causal rows are pinned to transformers' own by test_qwen3_cpu."""
    out = {}
    for name in NAMES:
        shape, seed, seqs, _ = golden(name)
        w = qo.random_weights(shape, seed)
        hidden = {c: [qo.encode_one(w, shape, s, causal=bool(c)) for s in seqs] for c in (1, 0)}
        for states in hidden.values():
            for h in states:
                h.setflags(write=False)
        out[name] = (shape, w, seqs, hidden)
    return out


@pytest.mark.parametrize("pooling", POOLINGS)
@pytest.mark.parametrize("precision", list(TOL))
@pytest.mark.parametrize("name", NAMES)
def test_encoder_matches_the_oracle(gpu, golden_refs, name, precision, pooling):
    from voitta_rag_amd import encoder as enc

    shape, w, seqs, hidden = golden_refs[name]
    want = np.stack([qo.pool(h, pooling) for h in hidden[1]])
    e = _engine(shape, pooling, precision, w)
    _check(enc.encode(e, *_pack(seqs)).astype(np.float64), want, precision, f"{name} {pooling}")
    for i in (0, len(seqs) - 1):  # alone, twice: the second run replays the cached graph where one is cached
        runs = [enc.encode(e, *_pack(seqs[i:i + 1])) for _ in range(2)]
        _check(runs[0].astype(np.float64), want[i:i + 1], precision, f"{name} sequence {i} alone")
        assert np.array_equal(_bits(runs[0]), _bits(runs[1])), i
    e.close()


@pytest.mark.parametrize("precision", list(TOL))
@pytest.mark.parametrize("name", NAMES)
def test_causal_zero_is_the_same_body_run_bidirectionally(gpu, golden_refs, name, precision):
    from voitta_rag_amd import encoder as enc

    shape, w, seqs, hidden = golden_refs[name]
    for pooling in ("mean", "last"):
        want = np.stack([qo.pool(h, pooling) for h in hidden[0]])
        masked = np.stack([qo.pool(h, pooling) for h in hidden[1]])
        assert np.max(np.abs(want - masked)) > 50 * TOL[precision][1]  # the two models are far apart
        e = _engine(shape, pooling, precision, w, causal=0)
        _check(enc.encode(e, *_pack(seqs)).astype(np.float64), want, precision, f"{name} bidirectional {pooling}")
        e.close()


# ---- 3. every token a span: every query row of every attention kernel is an output ------------------------------------
ROW_SHAPE = qo.Qwen3Shape(1, 128, 2, 1, 256, 128)  # one layer, 2 heads of 128 over 1 KV head: A = 256
ROW_SEED = 31
STAGED = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 320]  # f16: attention_seq_kernel holds 320 keys of 128 ...
STREAMED = [321, 449]                                            # ... from 321 tokens on the streamed kernel runs


@pytest.fixture(scope="module")
def row_refs():
    """ROW_SHAPE's weights, one sequence per length, and the oracle's unit hidden states of every token, causal and
    bidirectional (once, read-only)."""
    w = qo.random_weights(ROW_SHAPE, ROW_SEED)
    rng = np.random.default_rng(ROW_SEED + 1)
    seqs = {n: rng.integers(0, ROW_SHAPE.vocab, size=n).astype(np.int32) for n in STAGED + STREAMED}
    rows = {(n, c): _unit(qo.encode_one(w, ROW_SHAPE, s, causal=bool(c))) for n, s in seqs.items() for c in (1, 0)}
    for r in rows.values():
        r.setflags(write=False)
    return w, seqs, rows


@pytest.mark.parametrize("causal", [1, 0])
@pytest.mark.parametrize("precision", list(TOL))
@pytest.mark.parametrize("lengths", [STAGED, STREAMED], ids=["staged", "streamed"])
def test_every_token_row_is_the_oracles_hidden_state(gpu, row_refs, lengths, precision, causal):
    """f16: the staged kernel at head size 128 up to its last length (320), the streamed one from 321; f32 and f16x3: the
    same lengths through attention_kernel<128> (f16x3: its split context rows, A wide)."""
    w, seqs, rows = row_refs
    e = _engine(ROW_SHAPE, "last", precision, w, causal=causal)
    got = _token_rows(e, [seqs[n] for n in lengths])
    want = np.concatenate([rows[(n, causal)] for n in lengths])
    assert got.shape == want.shape
    _check(got.astype(np.float64), want, precision, f"{lengths[0]}..{lengths[-1]} tokens, causal {causal}")
    e.close()


# ---- 4. causality as a property ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("n_tokens, cuts", [(200, (1, 16, 17, 64, 65, 128, 129)), (449, (129, 321))], ids=["staged", "streamed"])
def test_rows_do_not_move_when_later_tokens_change(gpu, row_refs, n_tokens, cuts, precision):
    """One sequence beside a short one: the tokens at positions >= n are replaced, length and batch kept. The rows of
    tokens t < n are bit-identical to the unperturbed run — masked logits are -inf, their P is exactly 0, the same tiles
    are skipped in both runs, and the Q/K norm of a token reads that token alone — and the row of token n differs."""
    w, seqs, _ = row_refs
    long_seq, short = seqs[n_tokens], seqs[17]
    e = _engine(ROW_SHAPE, "last", precision, w)
    base = _token_rows(e, [short, long_seq])
    rng = np.random.default_rng(8)
    for n in cuts:
        other = long_seq.copy()
        other[n:] = (other[n:] + rng.integers(1, ROW_SHAPE.vocab, size=n_tokens - n)) % ROW_SHAPE.vocab
        assert (other[n:] != long_seq[n:]).all() and np.array_equal(other[:n], long_seq[:n])
        rows = _token_rows(e, [short, other])
        keep = len(short) + n
        assert np.array_equal(_bits(rows[:keep]), _bits(base[:keep])), n
        assert not np.array_equal(rows[keep], base[keep]), n
    e.close()


# ---- 5. batch invariance of the Q/K norm pass ----------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("name", ["tiny_d128", "tiny_d64n"])
def test_a_sequences_rows_are_the_same_alone_and_in_a_batch_of_40(gpu, golden_refs, name, precision):
    """The 100-token golden sequence alone, and as sequence 17 of 40 (39 sequences of 2 .. 5 tokens around it): every
    token row bit-equal. Both calls have between 65 and 256 tokens, so their f16 products take one GEMM kernel and the
    comparison is about the passes between them: qk_norm_rope_kernel sums a head's squares in an order that depends on
    the head alone, at whatever row of whatever batch the token sits."""
    shape, w, seqs, _ = golden_refs[name]
    s = seqs[10]
    assert len(s) == 100
    rng = np.random.default_rng(5)
    crowd = [rng.integers(0, shape.vocab, size=int(n)).astype(np.int32) for n in rng.integers(2, 6, size=39)]
    batch = crowd[:17] + [s] + crowd[17:]
    assert len(batch) == 40 and 65 <= sum(len(b) for b in batch) <= 256
    e = _engine(shape, "last", precision, w)
    alone = _token_rows(e, [s])
    at = sum(len(b) for b in batch[:17])
    crowded = _token_rows(e, batch)[at:at + 100]
    assert np.array_equal(_bits(alone), _bits(crowded))
    e.close()


# ---- 6. one batch per GEMM route, and the real row geometry ------------------------------------------------------------
PATH_SHAPE = qo.Qwen3Shape(2, 256, 4, 2, 256, 128, vocab=300)  # tiny_d128b's rows: A = 512
PATH_SEED = 51


@pytest.fixture(scope="module")
def path_refs():
    """Per batch of test_modernbert_gpu.PATH_LENS: the sequences and the oracle's rows for two poolings (every distinct
    sequence computed once, shared, read-only)."""
    rng = np.random.default_rng(52)
    w = qo.random_weights(PATH_SHAPE, PATH_SEED)
    refs, hidden = {}, {}
    for name, lens in PATH_LENS.items():
        distinct = [rng.integers(0, PATH_SHAPE.vocab, size=n).astype(np.int32) for n in lens[:8]]
        seqs = (distinct * (len(lens) // len(distinct) + 1))[:len(lens)]
        for s in seqs:
            if s.tobytes() not in hidden:
                hidden[s.tobytes()] = qo.encode_one(w, PATH_SHAPE, s)
        want = {p: np.stack([qo.pool(hidden[s.tobytes()], p) for s in seqs]) for p in ("last", "mean")}
        for v in want.values():
            v.setflags(write=False)
        refs[name] = (seqs, want)
    return w, refs


@pytest.mark.parametrize("precision", list(TOL))
@pytest.mark.parametrize("batch", list(PATH_LENS))
def test_every_gemm_route(gpu, path_refs, batch, precision):
    """Q/K/V as N = 3 A, K = H and the output projection as N = H, K = A on the skinny, mid and ping-pong routes (and, with
    512-token sequences in the last batch, the streamed attention kernel inside a large batch)."""
    from voitta_rag_amd import encoder as enc

    w, refs = path_refs
    seqs, want = refs[batch]
    for pooling in ("last", "mean"):
        e = _engine(PATH_SHAPE, pooling, precision, w, max_pos=1024)
        _check(enc.encode(e, *_pack(seqs)).astype(np.float64), want[pooling], precision, f"{batch} {pooling}")
        e.close()


@pytest.mark.parametrize("precision", list(TOL))
def test_the_0_6b_bodys_row_geometry(gpu, precision):
    """One layer of the Qwen3-Embedding-0.6B rows: hidden 1024, 16 heads of 128 over 8 KV heads (A = 2048: q_proj 1024 ->
    2048, o_proj 2048 -> 1024), intermediate 3072. A 12-token question alone (f16: the folded-norm skinny route with the
    plain epilogue, then the norm pass) and 300 tokens (the staged kernel near its limit)."""
    from voitta_rag_amd import encoder as enc

    shape = qo.Qwen3Shape(1, 1024, 16, 8, 3072, 128, vocab=300)
    w = qo.random_weights(shape, 81)
    rng = np.random.default_rng(82)
    seqs = [rng.integers(0, shape.vocab, size=n).astype(np.int32) for n in (12, 300)]
    e = _engine(shape, "last", precision, w)
    want = qo.sentence_embeddings(w, shape, seqs, "last")
    _check(enc.encode(e, *_pack(seqs[:1])).astype(np.float64), want[:1], precision, "12 tokens alone")
    _check(enc.encode(e, *_pack(seqs[1:])).astype(np.float64), want[1:], precision, "300 tokens")
    e.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
REF_SHAPE = qo.Qwen3Shape(2, 128, 2, 1, 256, 128)
REFUSED = [
    (dict(head_dim=96), r"head_dim 96 must be 0 \(hidden / heads\), 32, 64 or 128"),
    (dict(head_dim=256), r"head_dim 256 must be 0 \(hidden / heads\), 32, 64 or 128"),
    (dict(qk_norm=2), r"qk_norm 2 must be 0 or 1"),
    (dict(heads=3, head_dim=32), r"heads 3 x head_dim 32 = 96: the attention width must be a multiple of 128 and at most 2048"),
    (dict(heads=17), r"heads 17 x head_dim 128 = 2176: the attention width must be a multiple of 128 and at most 2048"),
    (dict(head_dim=32, heads=2), r"heads 2 x head_dim 32 = 64: the attention width must be a multiple of 128"),
    (dict(norm="post", position="learned", ffn="gelu", causal=0), r"head_dim 128 needs norm VR_NORM_PRE_RMS_ROTARY \(norm 0\)"),
    (dict(norm="pre", ffn="geglu", causal=0), r"head_dim 128 needs norm VR_NORM_PRE_RMS_ROTARY \(norm 1\)"),
    (dict(norm="rms_pre", position="none", ffn="relu", causal=0, head_dim=0),
     r"qk_norm 1 needs norm VR_NORM_PRE_RMS_ROTARY \(norm 2\)"),
    (dict(head_dim=0, qk_norm=0, heads=1, causal=1), r"head size 128 unsupported \(32 or 64\)"),  # the old refusal, its old words
]


def _raw_load(e, desc, state, names, load_fn):
    """desc and the tensors across the C ABI as they are (encoder._load would refuse a description its tensors' shapes do
    not fit before the engine sees it; the engine refuses a description before it reads a tensor)."""
    from voitta_rag_amd import encoder as enc

    keep = [None if n is None else np.ascontiguousarray(state[n], np.float32) for n in names]
    arr = (C.c_void_p * len(keep))(*[None if t is None else t.ctypes.data for t in keep])
    cdesc = desc.to_c()
    enc.check(load_fn(e.handle, C.byref(cdesc), arr, len(keep), enc.VR_MEM_HOST))


def test_refusals_name_the_field_and_leave_the_encoder_answering(gpu, golden_refs):
    from voitta_rag_amd import _lib
    from voitta_rag_amd import encoder as enc

    shape, w, seqs, hidden = golden_refs["tiny_d128"]
    assert (shape.hidden, shape.heads, shape.head_dim) == (REF_SHAPE.hidden, REF_SHAPE.heads, REF_SHAPE.head_dim)
    ids, off = _pack(seqs[:8])
    e = _engine(shape, "last", "f32", w)
    before = enc.encode(e, ids, off)
    _check(before.astype(np.float64), np.stack([qo.pool(h, "last") for h in hidden[1][:8]]), "f32", "before")
    desc = qo.desc_for(shape, "last", "f32")
    names, state = enc.qwen3_slots(w, desc)
    import dataclasses

    for over, message in REFUSED:  # (a description is refused before the tensors are counted)
        bad = dataclasses.replace(desc, **over)
        with pytest.raises(Exception, match=message):
            _raw_load(e, bad, state, names, e._lib.vr_encoder_load)
        assert np.array_equal(enc.encode(e, ids, off), before), message
    # a reranker takes neither field; the embedder is untouched
    for over, message in ((dict(qk_norm=0), r"a reranker takes no head size of its own \(head_dim 128\)"),
                          (dict(head_dim=0), r"a reranker takes no query / key norms \(qk_norm 1\)")):
        bad = dataclasses.replace(desc, pooling="cls", normalize=False, causal=0, **over)
        with pytest.raises(Exception, match=message):
            _raw_load(e, bad, state, names + [names[5]] * 4, e._lib.vr_reranker_load)
        assert np.array_equal(enc.encode(e, ids, off), before)
    e.close()
    # a v2-sized description reads both fields as 0: the Qwen2-style body (no norms, head size hidden / heads) gives the
    # same bits as vr_bert_desc_v2 and as vr_bert_desc_v3 with head_dim 64 spelled out
    # (with q/k/v biases, which a description without either field reads through qwen2_slots)
    plain = qo.Qwen3Shape(2, 128, 2, 1, 256, 64, qk_norm=False, attention_bias=True)
    wp = qo.random_weights(plain, 7)
    want = qo.sentence_embeddings(wp, plain, seqs[:8], "last")
    rows = []
    for over, kind in ((dict(head_dim=0), _lib.VrBertDescV2), (dict(head_dim=64), _lib.VrBertDescV3)):
        d = qo.desc_for(plain, "last", "f32", **over)
        assert type(d.to_c()) is kind
        e = _engine(plain, "last", "f32", wp, **over)
        rows.append(enc.encode(e, ids, off))
        _check(rows[-1].astype(np.float64), want, "f32", kind.__name__)
        e.close()
    assert np.array_equal(_bits(rows[0]), _bits(rows[1]))


# ---- 8. services -----------------------------------------------------------------------------------------------------------
SERVICE_SEED = 91
WORDS = ("vector database index hybrid fusion ranking sparse dense retrieval kernel memory bandwidth decoder attention "
         "causal mask rotary position norm residual token chunk document search query score filter").split()


@pytest.fixture
def qwen(monkeypatch, tmp_path, gpu):
    import bpe_case as bc

    from voitta_rag_amd import config, embedding, sparse_embedding, store_registry, vector_store

    def reset():
        config.get_settings.cache_clear()
        store_registry.reset()
        embedding._embedding_service = None
        sparse_embedding._sparse_embedding_service = None
        vector_store._vector_store = None

    def make(name, deferred):
        path = str(tmp_path / name)
        hf = bc.hf_tokenizer(bc.fixture())
        shape = qo.Qwen3Shape(2, 128, 2, 1, 256, 128, vocab=-(-hf.get_vocab_size() // 8) * 8)
        w = qo.write_checkpoint(path, shape, SERVICE_SEED, max_seq=64)
        for k, v in (("EMBEDDING_MODEL", path), ("EMBEDDING_DIMENSION", "128"), ("VOITTA_ENCODER_PRECISION", "f32"),
                     ("VOITTA_DEFERRED_INDEXING", "1" if deferred else "0")):
            monkeypatch.setenv(k, v)
        reset()
        hf.enable_truncation(max_length=64)
        return shape, w, hf

    yield make
    reset()


def _metas(n):
    from voitta_rag_amd.vector_store import ChunkMetadata

    return [ChunkMetadata(file_path="d/a.md", folder_path="d", index_folder="d", file_name="a.md", chunk_index=i, total_chunks=n,
                          start_char=0, end_char=1, indexed_at="t", source_modified_at=1_700_000_000 + i) for i in range(n)]


def test_services_embed_store_and_answer_text_questions(qwen):
    from voitta_rag_amd import deferred, embedding, sparse_embedding, vector_store
    from voitta_rag_amd.bpe import BpeTokenizer
    from voitta_rag_amd.sparse_embedding import _query_vector

    rng = np.random.default_rng(3)
    texts = [" ".join(rng.choice(WORDS, size=int(n))) for n in (3, 40, 9, 1, 25, 12, 30, 7)] + [" ".join(["memory bandwidth"] * 60)]
    shape, w, hf = qwen("qwen3-tiny", deferred=False)
    emb, sp, vs = (embedding.get_embedding_service(), sparse_embedding.get_sparse_embedding_service(),
                   vector_store.get_vector_store())
    model = emb.model
    assert isinstance(model.tokenizer, BpeTokenizer) and embedding.one_call_text_paths(model)
    assert (model.desc.norm, model.desc.causal, model.desc.pooling, model.desc.head_dim, model.desc.qk_norm, model.max_seq_length) == \
        ("rms_pre_rotary", 1, "last", 128, 1, 64)
    seqs = [np.asarray(t.ids, np.int32) for t in hf.encode_batch(texts)]
    assert max(len(s) for s in seqs) == 64
    direct = np.asarray(emb.embed_texts(texts), np.float32)
    _check(direct.astype(np.float64), qo.sentence_embeddings(w, shape, seqs, "last"), "f32", "embed_texts")
    vs.store_chunks(list(zip(texts, direct.tolist(), _metas(len(texts)))), sparse_vectors=sp.embed_texts(texts))
    reqs = [{"query": texts[1], "limit": 3}, {"query": "causal mask?", "limit": 4, "sparse_weight": 1.0},
            {"query": texts[4], "limit": 2, "folder_filter": "d"}]
    got = vs.search_questions(reqs)
    vecs = emb.embed_queries([r["query"] for r in reqs])
    ref = vs.search_requests([dict({a: v for a, v in r.items() if a != "query"}, query_embedding=vecs[i],
                                   sparse_query=_query_vector(r["query"])) for i, r in enumerate(reqs)])
    for g, r_, r in zip(got, ref, reqs):
        assert len(g) == r["limit"] and [(c.id, c.score) for c in g] == [(c.id, c.score) for c in r_], r["query"][:30]
    assert got[0][0].metadata.chunk_index == 1 and got[2][0].metadata.chunk_index == 4
    # deferred indexing: the rows the fused indexing call stores are the direct ones, bit for bit
    qwen("qwen3-tiny", deferred=True)
    emb, sp, vs = (embedding.get_embedding_service(), sparse_embedding.get_sparse_embedding_service(),
                   vector_store.get_vector_store())
    later = emb.embed_texts(texts)
    assert isinstance(later, deferred.DeferredEmbeddings)
    vs.store_chunks(list(zip(texts, later, _metas(len(texts)))), sparse_vectors=sp.embed_texts(texts))
    assert not later.materialized  # the fused indexing call took them
    assert np.array_equal(_bits(vs.client.get_dense(np.arange(len(texts)))), _bits(direct))
