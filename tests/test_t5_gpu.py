"""T5 encoders (gtr-t5, sentence-t5) on the GPU, through the C ABI against tests/t5_oracle.py at test_encoder_gpu.TOL:
RMSNorm pre-norm layers (VR_NORM_PRE_RMS), the ReLU FFN (EPI_BIAS_RELU) on every GEMM route, the folded-RMSNorm question
route, the relative-position table on a model without positions in all three attention kernels and on sequences longer
than MPNet ever ran, the table's set / remove / zero equivalences, spans, the refusals, and the services on a synthetic
gtr-t5-style checkpoint directory. Every test here fails without VR_NORM_PRE_RMS ("unknown norm placement")."""
import os

import numpy as np
import pytest

import mpnet_oracle as mp
import t5_oracle as t5
from test_encoder_gpu import TOL
from test_modernbert_gpu import PATH_LENS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


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


def _engine(shape, pooling, precision, w, table="own", **over):
    """An engine with the model loaded through load_encoder (t5_slots: the NULL slots, the query fold). table: "own" (the
    checkpoint's, set by load_encoder), an array (carried by the description), None (removed after the load)."""
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    e = Engine(shape.hidden)
    carried = table if isinstance(table, np.ndarray) else None
    enc.load_encoder(e, t5.desc_for(shape, pooling, precision, attention_bias=carried, **over), w)
    if table is None:
        e.set_attention_bias(None)
    return e


# ---- 1. both goldens' shapes at every precision and pooling --------------------------------------------------------------
def _golden(name):
    z = np.load(os.path.join(HERE, "golden", f"t5_{name}.npz"))
    layers, hidden, heads, inter, vocab, buckets, max_distance = (int(v) for v in z["shape"])
    shape = t5.T5Shape(layers, hidden, heads, inter, vocab=vocab, eps=float(z["eps"]), buckets=buckets, max_distance=max_distance)
    off = z["offsets"]
    return shape, int(z["seed"]), [z["ids"][off[i]:off[i + 1]] for i in range(len(off) - 1)], str(z["pooling"]), z["want"]


@pytest.fixture(scope="module")
def golden_refs():
    """Per golden: shape, weights, sequences and the oracle's rows for both poolings (once, read-only); the recorded
    pooling's rows are transformers' own."""
    out = {}
    for name in ("tiny_d64", "tiny_d32"):
        shape, seed, seqs, pooling, recorded = _golden(name)
        w = t5.random_weights(shape, seed)
        want = {p: t5.sentence_embeddings(w, shape, seqs, p) for p in ("mean", "cls")}
        assert np.max(np.abs(want[pooling] - recorded)) < 1e-9
        for v in want.values():
            v.setflags(write=False)
        out[name] = (shape, w, seqs, want)
    return out


@pytest.mark.parametrize("pooling", ["mean", "cls"])
@pytest.mark.parametrize("precision", list(TOL))
@pytest.mark.parametrize("name", ["tiny_d64", "tiny_d32"])
def test_encoder_matches_the_oracle(gpu, golden_refs, name, precision, pooling):
    from voitta_rag_amd import encoder as enc

    shape, w, seqs, want = golden_refs[name]
    e = _engine(shape, pooling, precision, w)
    _check(enc.encode(e, *_pack(seqs)).astype(np.float64), want[pooling], precision, f"{name} {pooling}")
    for i in (0, len(seqs) - 1):  # alone, twice: the second run replays the cached graph where one is cached
        runs = [enc.encode(e, *_pack(seqs[i:i + 1])) for _ in range(2)]
        _check(runs[0].astype(np.float64), want[pooling][i:i + 1], precision, f"{name} sequence {i} alone")
        assert np.array_equal(_bits(runs[0]), _bits(runs[1])), i
    e.close()


# ---- 2. one batch per GEMM route ------------------------------------------------------------------------------------------
PATH_SHAPE = t5.T5Shape(3, 128, 2, 256)


@pytest.fixture(scope="module")
def path_refs():
    """Per batch of test_modernbert_gpu.PATH_LENS: the sequences, the oracle's rows for both poolings and its final
    hidden states per sequence (every distinct sequence computed once, shared, read-only)."""
    w = t5.random_weights(PATH_SHAPE, 51)
    rng = np.random.default_rng(52)
    refs, hidden = {}, {}
    for name, lens in PATH_LENS.items():
        distinct = [rng.integers(0, PATH_SHAPE.vocab, size=n).astype(np.int32) for n in lens[:8]]
        seqs = (distinct * (len(lens) // len(distinct) + 1))[:len(lens)]
        want = {"mean": [], "cls": []}
        states = []
        for s in seqs:
            key = s.tobytes()
            if key not in hidden:
                hidden[key] = t5.encode_one(w, PATH_SHAPE, s)
            states.append(hidden[key])
            for p in want:
                want[p].append(mp.pool(hidden[key], p))
        want = {p: np.stack(v) for p, v in want.items()}
        for v in want.values():
            v.setflags(write=False)
        refs[name] = (seqs, want, states)
    return w, refs


@pytest.mark.parametrize("pooling", ["mean", "cls"])
@pytest.mark.parametrize("precision", ["f16", "f32"])
@pytest.mark.parametrize("batch", list(PATH_LENS))
def test_every_gemm_route(gpu, path_refs, batch, precision, pooling):
    from voitta_rag_amd import encoder as enc

    w, refs = path_refs
    seqs, want, _ = refs[batch]
    e = _engine(PATH_SHAPE, pooling, precision, w)
    _check(enc.encode(e, *_pack(seqs)).astype(np.float64), want[pooling], precision, f"{batch} {pooling}")
    e.close()


# ---- 3. the folded-RMSNorm question route --------------------------------------------------------------------------------
FOLD_SHAPE = t5.T5Shape(2, 384, 6, 768)


@pytest.mark.parametrize("n", [1, 9, 16, 17])
def test_folded_norm_question_route(gpu, n):
    """H = 384 (6 heads of 64, d_ff 768), f16: at most 16 rows take gemm_f16_skinny_rms_kernel (the norm inside the
    projection), 17 the RMSNorm launches. Three runs, bit-identical: the later ones are the cached graph's."""
    from voitta_rag_amd import encoder as enc

    w = t5.random_weights(FOLD_SHAPE, 71)
    s = np.random.default_rng(72 + n).integers(0, FOLD_SHAPE.vocab, size=n).astype(np.int32)
    want = t5.sentence_embeddings(w, FOLD_SHAPE, [s], "mean")
    e = _engine(FOLD_SHAPE, "mean", "f16", w)
    runs = [enc.encode(e, *_pack([s])) for _ in range(3)]
    _check(runs[0].astype(np.float64), want, "f16", f"{n} rows")
    assert np.array_equal(_bits(runs[0]), _bits(runs[1])) and np.array_equal(_bits(runs[0]), _bits(runs[2]))
    e.close()


# ---- 4. attention edges with the table on long sequences -----------------------------------------------------------------
LONG_MODELS = {64: (t5.T5Shape(2, 128, 2, 256), 61), 32: (t5.T5Shape(2, 128, 4, 256), 62)}


@pytest.mark.parametrize("dh,n", [(64, 640), (64, 656), (64, 1100), (32, 1400)])
def test_staged_and_streamed_edges(gpu, dh, n):
    """As test_alibi_gpu.test_staged_and_streamed_edges, with the table: at d_h = 64 the staged kernel's LDS holds the
    keys, the values AND the head's 257-entry row, so 640 tokens no longer fit beside it and stream, as 656, 1100 and (at
    d_h = 32) 1400 do — lengths MPNet's 512 positions never reached. One sequence per call, f16, max_pos raised to
    2048; mean pooling and CLS. Most offsets lie past the table's radius: dropping the clamp's far entry (the oracle
    with the table cut to radius 64) moves the row by more than twice the tolerance, so the far keys' bias counts."""
    from voitta_rag_amd import encoder as enc

    shape, seed = LONG_MODELS[dh]
    assert shape.d_kv == dh
    w = t5.random_weights(shape, seed)
    s = np.random.default_rng(n).integers(0, shape.vocab, size=n).astype(np.int32)
    hidden = t5.encode_one(w, shape, s)
    short = t5.table_from_buckets(w[t5.BIAS_KEY], shape)[:, 64:-64]
    seen = float(np.max(np.abs(mp.pool(t5.encode_one(w, shape, s, short), "mean") - mp.pool(hidden, "mean"))))
    print(f"{n} tokens: a table clamped at 64 moves the mean embedding by {seen:.3e}")
    assert seen > 2 * TOL["f16"][1]
    for pooling in ("mean", "cls"):
        e = _engine(shape, pooling, "f16", w, max_pos=2048)
        _check(enc.encode(e, *_pack([s])).astype(np.float64), mp.pool(hidden, pooling)[None], "f16", f"{n} tokens {pooling}")
        e.close()


# ---- 5. equivalences ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_zero_table_removed_table_and_back(gpu, path_refs, precision):
    """A zero table gives the encoder without a table bit for bit; a removed table gives the engine that never had one
    (and the oracle without a bias); setting it again gives the first result."""
    from voitta_rag_amd import encoder as enc

    w, refs = path_refs
    seqs, want, _ = refs["skinny4"]
    ids, off = _pack(seqs)
    own = enc.t5_bias_table(w[t5.BIAS_KEY])
    never = _engine(PATH_SHAPE, "mean", precision, w, table=np.zeros((PATH_SHAPE.heads, 3), np.float32))
    never.set_attention_bias(None)
    bare = enc.encode(never, ids, off)
    _check(bare.astype(np.float64), t5.sentence_embeddings(w, PATH_SHAPE, seqs, "mean", table=None), precision, "no table")
    e = _engine(PATH_SHAPE, "mean", precision, w)
    first = enc.encode(e, ids, off)
    _check(first.astype(np.float64), want["mean"], precision, "own table")
    assert not np.array_equal(first, bare)
    e.set_attention_bias(np.zeros_like(own))
    assert np.array_equal(_bits(enc.encode(e, ids, off)), _bits(bare))
    e.set_attention_bias(None)
    assert np.array_equal(_bits(enc.encode(e, ids, off)), _bits(bare))
    e.set_attention_bias(own)
    assert np.array_equal(_bits(enc.encode(e, ids, off)), _bits(first))
    e.close()
    never.close()


@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_span_rows_are_the_oracles_span_means(gpu, path_refs, precision):
    from voitta_rag_amd import encoder as enc

    w, refs = path_refs
    seqs, _, states = refs["mid"]
    ids, off = _pack(seqs)
    rng = np.random.default_rng(5)
    spans, span_off = [], [0]
    for i, s in enumerate(seqs):
        cuts = sorted({0, len(s), *rng.integers(0, len(s) + 1, size=2).tolist()})
        spans += [(i, b, e_) for b, e_ in zip(cuts[:-1], cuts[1:])]
        span_off.append(len(spans))
    tok = np.asarray([(b, e_) for _, b, e_ in spans], np.int32)
    e = _engine(PATH_SHAPE, "mean", precision, w)
    got = enc.encode_spans(e, ids, off, np.asarray(span_off, np.int32), tok)
    want = np.stack([mp.pool(states[i][b:e_], "mean") for i, b, e_ in spans])
    _check(got.astype(np.float64), want, precision, f"{len(spans)} spans")
    # one span [0, len) per sequence: vr_encode's mean row, bit for bit
    whole = np.asarray([(0, len(s)) for s in seqs], np.int32)
    rows = enc.encode_spans(e, ids, off, np.arange(len(seqs) + 1, dtype=np.int32), whole)
    assert np.array_equal(_bits(rows), _bits(enc.encode(e, ids, off)))
    e.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_field_and_leave_the_encoder_answering(gpu, path_refs):
    from voitta_rag_amd import encoder as enc

    w, refs = path_refs
    seqs, want, _ = refs["skinny4"]
    ids, off = _pack(seqs)
    e = _engine(PATH_SHAPE, "mean", "f32", w)
    before = enc.encode(e, ids, off)
    _check(before.astype(np.float64), want["mean"], "f32", "before")
    names, state, _ = enc.t5_slots(w, t5.desc_for(PATH_SHAPE, "mean", "f32"))
    # (the description is refused before the tensors are counted: the 16-slot list serves the gated one too)
    for over, message in (
            (dict(position="rotary", rope_theta=10000.0), r"norm VR_NORM_PRE_RMS needs position VR_POS_NONE \(position 1\)"),
            (dict(position="learned"), r"norm VR_NORM_PRE_RMS needs position VR_POS_NONE \(position 0\)"),
            (dict(ffn="geglu"), r"norm VR_NORM_PRE_RMS needs ffn VR_FFN_RELU \(ffn 2\)"),
            (dict(ffn="gelu"), r"norm VR_NORM_PRE_RMS needs ffn VR_FFN_RELU \(ffn 0\)"),
            (dict(window=8, global_every=2), r"norm VR_NORM_PRE_RMS takes no window \(window 8\)"),
            (dict(type_vocab=2), r"norm VR_NORM_PRE_RMS needs type_vocab 1 \(type_vocab 2\)"),
            (dict(norm="post"), r"ffn VR_FFN_RELU needs norm VR_NORM_PRE_RMS \(norm 0\)"),
            (dict(norm="pre", position="rotary", rope_theta=10000.0), r"ffn VR_FFN_RELU needs norm VR_NORM_PRE_RMS \(norm 1\)")):
        with pytest.raises(Exception, match=message):
            enc._load(e, t5.desc_for(PATH_SHAPE, "mean", "f32", **over), state, names, e._lib.vr_encoder_load)
        assert np.array_equal(enc.encode(e, ids, off), before), message
    # slopes stay refused on this family; a table of the wrong head count and radius too
    with pytest.raises(Exception, match=r"an attention bias needs position VR_POS_LEARNED and norm VR_NORM_POST \(position 2, norm 2"):
        e.set_attention_slopes(np.array([0.5, 0.25], np.float32))
    with pytest.raises(Exception, match="bias table of 3 heads for an encoder of 2"):
        e.set_attention_bias(np.zeros((3, 257), np.float32))
    with pytest.raises(Exception, match="radius 513 must lie in 1..512"):
        e.set_attention_bias(np.zeros((2, 1027), np.float32))
    assert np.array_equal(enc.encode(e, ids, off), before)
    # a reranker never takes the new norm; the embedder is untouched
    with pytest.raises(Exception, match="a reranker with norm VR_NORM_PRE_RMS is not supported"):
        enc._load(e, t5.desc_for(PATH_SHAPE, "cls", "f32", normalize=False), state, names + [names[5]] * 4,
                  e._lib.vr_reranker_load)
    assert np.array_equal(enc.encode(e, ids, off), before)
    e.close()


# ---- 7. services -------------------------------------------------------------------------------------------------------------
SERVICE_SEED = 91


@pytest.fixture
def gtr(monkeypatch, tmp_path, gpu):
    from voitta_rag_amd import config, embedding, sparse_embedding, store_registry, vector_store

    def reset():
        config.get_settings.cache_clear()
        store_registry.reset()
        embedding._embedding_service = None
        sparse_embedding._sparse_embedding_service = None
        vector_store._vector_store = None

    def make(name, precision="f32", max_seq=128, **env):
        path = str(tmp_path / name)
        vocab = len(t5.tokenizer_fixture()["tokenizer"]["model"]["vocab"])
        shape = t5.T5Shape(2, 128, 2, 256, vocab=vocab)
        w = t5.write_checkpoint(path, shape, SERVICE_SEED, max_seq=max_seq, prefix="0.auto_model.")
        for k, v in dict({"EMBEDDING_MODEL": path, "EMBEDDING_DIMENSION": "128", "VOITTA_ENCODER_PRECISION": precision,
                          "VOITTA_DEFERRED_INDEXING": "0"}, **env).items():
            monkeypatch.setenv(k, v)
        reset()
        return shape, w

    yield make
    reset()


WORDS = ("vector database index hybrid fusion ranking sparse dense retrieval kernel memory bandwidth encoder attention "
         "relative position bias layer norm residual token chunk document search query score filter").split()


def test_services_embed_store_and_answer_text_questions(gtr):
    from voitta_rag_amd import embedding, sparse_embedding, vector_store
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd.unigram import UnigramTokenizer
    from voitta_rag_amd.vector_store import ChunkMetadata

    shape, w = gtr("gtr-t5-tiny")
    emb, sp, vs = (embedding.get_embedding_service(), sparse_embedding.get_sparse_embedding_service(),
                   vector_store.get_vector_store())
    model = emb.model
    assert isinstance(model.tokenizer, UnigramTokenizer) and embedding.one_call_text_paths(model)
    assert (model.desc.norm, model.desc.ffn, model.desc.position, model.max_seq_length) == ("rms_pre", "relu", "none", 128)
    assert model.desc.attention_bias.shape == (2, 257) and len(model.desc.head) == 1
    rng = np.random.default_rng(3)
    texts = [" ".join(rng.choice(WORDS, size=int(n))) for n in (3, 40, 9, 1, 25, 12)] + [" ".join(["memory bandwidth"] * 200)]
    ids, off = model.tokenize(texts)  # (the native ids are pinned to the tokenizers library's by test_t5_cpu)
    seqs = [ids[off[i]:off[i + 1]] for i in range(len(texts))]
    assert max(len(s) for s in seqs) == 128 and all(s[-1] == 1 for s in seqs)
    vectors = emb.embed_texts(texts)
    _check(np.asarray(vectors, np.float64), t5.head_embeddings(w, shape, seqs, SERVICE_SEED), "f32", "embed_texts")
    metas = [ChunkMetadata(file_path="d/a.md", folder_path="d", index_folder="d", file_name="a.md", chunk_index=i,
                           total_chunks=len(texts), start_char=0, end_char=1, indexed_at="t",
                           source_modified_at=1_700_000_000 + i) for i in range(len(texts))]
    vs.store_chunks(list(zip(texts, vectors, metas)), sparse_vectors=sp.embed_texts(texts))
    got = vs.search_questions([{"query": texts[1], "limit": 3}, {"query": texts[4], "limit": 2}])
    assert [len(g) for g in got] == [3, 2]
    assert got[0][0].metadata.chunk_index == 1 and got[1][0].metadata.chunk_index == 4
    # the text path's rows are vr_encode's of the same ids, bit for bit
    e = model.engine
    questions = [texts[1], "dense retrieval?", texts[6]]
    limits, weights = np.full(3, 5, np.int32), np.full(3, 0.1)
    _, qemb = e.query_text_batch(model.tokenizer, questions, questions, model.max_seq_length, limits, weights, [None] * 3,
                                 embeddings=True)
    qids, qoff = model.tokenize(questions)
    assert np.array_equal(_bits(qemb), _bits(enc.encode(e, qids, qoff)))


def test_late_chunking_with_the_cap_raised(gtr):
    """VOITTA_LATE_CHUNKING=1 and sequences of up to 2048 tokens: a long document is one sequence, and every chunk's row
    is the oracle's span mean through the Dense head — with a table whose clamp covers most of the document."""
    from test_late_chunking_gpu import document

    from voitta_rag_amd import embedding
    from voitta_rag_amd import late_chunking as lc
    from voitta_rag_amd.chunking import get_chunking_service

    shape, w = gtr("gtr-late", precision="f16", max_seq=2048, VOITTA_LATE_CHUNKING="1", VOITTA_MAX_SEQ_LENGTH="2048")
    emb = embedding.get_embedding_service()
    model = emb.model
    assert model.max_seq_length == 2048 and model.desc.max_pos == 2048
    doc = document(np.random.default_rng(15), 180)
    chunks = [str(c.text) for c in get_chunking_service().chunk_text(doc)]
    assert model.leading_specials == 0
    plan = lc.plan(doc, chunks, model.tokenize, 2048, 256, lead=0)
    assert plan.ids[0] != 1 and plan.ids[-1] == 1 and int(plan.span_tok[0, 0]) == 0  # no <s>: the first span starts at 0
    assert plan.n_seq == 1 and 1200 <= int(plan.offsets[-1]) <= 2048 and not plan.truncated.any()
    got = np.asarray(emb.embed_document(doc, chunks), np.float32)
    hidden = t5.encode_one(w, shape, plan.ids)
    dense = t5.dense_weight(shape, SERVICE_SEED).astype(np.float64)
    want = np.stack([hidden[b:e_].mean(axis=0) for b, e_ in plan.span_tok.tolist()]) @ dense.T
    want = want / np.linalg.norm(want, axis=1, keepdims=True)
    _check(got.astype(np.float64), want, "f16", f"{len(chunks)} chunks of a {int(plan.offsets[-1])}-token document")
