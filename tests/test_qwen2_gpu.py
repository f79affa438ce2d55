"""Qwen2 decoder embedders on the GPU, through the C ABI against tests/qwen2_oracle.py at test_encoder_gpu.TOL: the RMSNorm
pre-norm block with rotary positions and a SwiGLU (VR_NORM_PRE_RMS_ROTARY) on every GEMM route, the causal mask in all
three attention kernels at their tile edges — against the oracle and as a property (a token's row does not move when later
tokens change, bit for bit) — last-token pooling, grouped-query checkpoints through encoder.qwen2_slots, the refusals, and
the services on a synthetic qwen2 checkpoint directory. Every test here fails without the feature ("unknown norm
placement 3")."""
import os
import subprocess
import sys

import numpy as np
import pytest

import qwen2_oracle as qo
from test_encoder_gpu import TOL
from test_modernbert_gpu import PATH_LENS
from test_qwen2_cpu import golden

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
POOLINGS = ("last", "mean", "cls")


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
    """An engine with the model loaded through load_encoder (qwen2_slots: the NULL slots, the repeated K/V heads)."""
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    e = Engine(shape.hidden)
    enc.load_encoder(e, qo.desc_for(shape, pooling, precision, **over), w)
    return e


def _token_rows(e, seqs, positions):
    """vr_encode_spans rows of the single-token spans [t, t + 1), t in positions[i], of sequence i."""
    from voitta_rag_amd import encoder as enc

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
    (once, read-only); the causal rows are pinned to transformers' own by test_qwen2_cpu."""
    out = {}
    for name in ("tiny_d64", "tiny_d32"):
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
@pytest.mark.parametrize("name", ["tiny_d64", "tiny_d32"])
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
@pytest.mark.parametrize("name", ["tiny_d64", "tiny_d32"])
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


# ---- 3. causality as a property ------------------------------------------------------------------------------------------
CUTS = (1, 16, 17, 64, 65, 128, 129)


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("name", ["tiny_d64", "tiny_d32"])
def test_rows_do_not_move_when_later_tokens_change(gpu, golden_refs, name, precision):
    """One 200-token sequence (beside a short one): the tokens at positions >= n are replaced, length and batch kept. The
    rows of tokens t < n are bit-identical to the unperturbed run — masked logits are -inf, their P is exactly 0, the
    same tiles are skipped in both runs — and the row of token n differs. Nothing here rests on the oracle."""
    shape, w, seqs, _ = golden_refs[name]
    long_seq, short = seqs[-1], seqs[6]
    assert len(long_seq) == 200
    e = _engine(shape, "last", precision, w)
    every = [list(range(len(short))), list(range(200))]
    base = _token_rows(e, [short, long_seq], every)
    rng = np.random.default_rng(8)
    for n in CUTS:
        other = long_seq.copy()
        other[n:] = (other[n:] + rng.integers(1, shape.vocab, size=200 - n)) % shape.vocab
        assert (other[n:] != long_seq[n:]).all() and np.array_equal(other[:n], long_seq[:n])
        rows = _token_rows(e, [short, other], every)
        keep = len(short) + n
        assert np.array_equal(_bits(rows[:keep]), _bits(base[:keep])), n
        assert not np.array_equal(rows[keep], base[keep]), n
    e.close()


# ---- 4. single-token spans against the oracle's hidden states --------------------------------------------------------------
@pytest.mark.parametrize("precision", list(TOL))
@pytest.mark.parametrize("name", ["tiny_d64", "tiny_d32"])
def test_token_rows_are_the_oracles_hidden_states(gpu, golden_refs, name, precision):
    shape, w, seqs, hidden = golden_refs[name]
    at = [0, 15, 16, 63, 64, 127, 128, 199]
    e = _engine(shape, "last", precision, w)
    got = _token_rows(e, [seqs[6], seqs[-1]], [[0, len(seqs[6]) - 1], at])
    want = _unit(np.concatenate([hidden[1][6][[0, -1]], hidden[1][-1][at]]))
    _check(got.astype(np.float64), want, precision, f"{name} token rows")
    e.close()


# ---- 5. the streamed kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, n", [("tiny_d64", 705), ("tiny_d32", 1345)])
def test_streamed_sequences(gpu, golden_refs, name, n):
    """One sequence longer than a workgroup's LDS stages (from 641 tokens at head size 64, from 1281 at 32) beside a short
    one, f16: the last-token rows and single-token rows around the 128-query block edge, at 640 and at the end against
    the oracle, and the perturbation property of test_rows_do_not_move_when_later_tokens_change across block edges."""
    from voitta_rag_amd import encoder as enc

    shape, w, seqs, hidden = golden_refs[name]
    rng = np.random.default_rng(n)
    long_seq, short = rng.integers(0, shape.vocab, size=n).astype(np.int32), seqs[6]
    states = qo.encode_one(w, shape, long_seq)
    e = _engine(shape, "last", "f16", w, max_pos=2048)
    pooled = enc.encode(e, *_pack([short, long_seq]))
    _check(pooled.astype(np.float64), _unit(np.stack([hidden[1][6][-1], states[-1]])), "f16", f"{n} tokens, last-token rows")
    at = [127, 128, 129, 640, n - 1]
    got = _token_rows(e, [short, long_seq], [[0], at])[1:]
    _check(got.astype(np.float64), _unit(states[at]), "f16", f"{n} tokens, token rows")
    every = [[0], list(range(n))]
    base = _token_rows(e, [short, long_seq], every)[1:]
    for cut in (129, 641):
        other = long_seq.copy()
        other[cut:] = (other[cut:] + rng.integers(1, shape.vocab, size=n - cut)) % shape.vocab
        rows = _token_rows(e, [short, other], every)[1:]
        assert np.array_equal(_bits(rows[:cut]), _bits(base[:cut])), cut
        assert not np.array_equal(rows[cut], base[cut]), cut
    e.close()


# ---- 6. one batch per GEMM route -------------------------------------------------------------------------------------------
PATH_SHAPE = qo.Qwen2Shape(3, 128, 2, 1, 256, vocab=300)
PATH_SEED = 51


def path_batches():
    rng = np.random.default_rng(52)
    out = {}
    for name, lens in PATH_LENS.items():
        distinct = [rng.integers(0, PATH_SHAPE.vocab, size=n).astype(np.int32) for n in lens[:8]]
        out[name] = (distinct * (len(lens) // len(distinct) + 1))[:len(lens)]
    return qo.random_weights(PATH_SHAPE, PATH_SEED), out


@pytest.fixture(scope="module")
def path_refs():
    """Per batch of test_modernbert_gpu.PATH_LENS: the sequences and the oracle's rows for the three poolings (every
    distinct sequence computed once, shared, read-only)."""
    w, batches = path_batches()
    refs, hidden = {}, {}
    for name, seqs in batches.items():
        for s in seqs:
            if s.tobytes() not in hidden:
                hidden[s.tobytes()] = qo.encode_one(w, PATH_SHAPE, s)
        want = {p: np.stack([qo.pool(hidden[s.tobytes()], p) for s in seqs]) for p in POOLINGS}
        for v in want.values():
            v.setflags(write=False)
        refs[name] = (seqs, want)
    return w, refs


@pytest.mark.parametrize("precision", list(TOL))
@pytest.mark.parametrize("batch", list(PATH_LENS))
def test_every_gemm_route(gpu, path_refs, batch, precision):
    from voitta_rag_amd import encoder as enc

    w, refs = path_refs
    seqs, want = refs[batch]
    for pooling in ("last", "mean"):
        e = _engine(PATH_SHAPE, pooling, precision, w)
        _check(enc.encode(e, *_pack(seqs)).astype(np.float64), want[pooling], precision, f"{batch} {pooling}")
        e.close()


FOLD_SHAPE = qo.Qwen2Shape(2, 384, 6, 2, 768)


@pytest.mark.parametrize("n", [1, 9, 16, 17])
def test_folded_norm_question_route(gpu, n):
    """H = 384 (6 heads of 64 over 2 KV heads), f16: at most 16 rows take the skinny kernels with the RMSNorm inside the
    projection (gemm_f16_skinny_rms_rope_kernel for Q/K/V, the gate in the FFN-up epilogue), 17 the RMSNorm launches.
    Three runs, bit-identical: the later ones are the cached graph's."""
    from voitta_rag_amd import encoder as enc

    w = qo.random_weights(FOLD_SHAPE, 71)
    s = np.random.default_rng(72 + n).integers(0, FOLD_SHAPE.vocab, size=n).astype(np.int32)
    want = qo.sentence_embeddings(w, FOLD_SHAPE, [s], "last")
    e = _engine(FOLD_SHAPE, "last", "f16", w)
    runs = [enc.encode(e, *_pack([s])) for _ in range(3)]
    _check(runs[0].astype(np.float64), want, "f16", f"{n} rows")
    assert np.array_equal(_bits(runs[0]), _bits(runs[1])) and np.array_equal(_bits(runs[0]), _bits(runs[2]))
    e.close()


def encode_skinny_batches(out_path=None):
    """The batches whose f16 route fuses the rotation and the gate, and a folded-norm question, at both precisions."""
    from voitta_rag_amd import encoder as enc

    w, batches = path_batches()
    out = {}
    for precision in ("f16", "f32"):
        e = _engine(PATH_SHAPE, "last", precision, w)
        for name in ("skinny1", "skinny4", "mid"):
            out[f"{name} {precision}"] = enc.encode(e, *_pack(batches[name]))
        e.close()
    wf = qo.random_weights(FOLD_SHAPE, 71)
    e = _engine(FOLD_SHAPE, "last", "f16", wf)
    out["fold f16"] = enc.encode(e, *_pack([np.arange(9, dtype=np.int32)]))
    e.close()
    if out_path:
        np.savez(out_path, **out)
    return out


def test_unfused_passes_in_a_child_process(gpu, path_refs, tmp_path):
    """VR_ENCODE_FUSE is read when a model is loaded: the same batches, loaded once and run in a fresh child process
    with the rotation and the gate as passes of their own, against the same oracle rows. f32 never fuses:
    bit-identical to this process's run; the skinny f16 batches differ (one f16 rounding of Q, K and the gate's product
    more)."""
    out_path = str(tmp_path / "unfused.npz")
    code = (f"import sys; sys.path[:0] = {[os.path.dirname(HERE), HERE]!r}; import test_qwen2_gpu as t; "
            f"t.encode_skinny_batches({out_path!r})")
    subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, VR_ENCODE_FUSE="0"), timeout=120)
    unfused = np.load(out_path)
    fused = encode_skinny_batches()
    _, refs = path_refs
    fold_want = qo.sentence_embeddings(qo.random_weights(FOLD_SHAPE, 71), FOLD_SHAPE, [np.arange(9)], "last")
    assert sorted(unfused.files) == sorted(fused)
    for key, got in fused.items():
        batch, precision = key.split()
        want = fold_want if batch == "fold" else refs[batch][1]["last"]
        _check(unfused[key].astype(np.float64), want, precision, "unfused " + key)
        if precision == "f32":
            assert np.array_equal(got, unfused[key]), key
        elif batch != "mid":
            assert not np.array_equal(got, unfused[key]), key  # the child really ran another form


# ---- 7. the real row geometry, small ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_the_half_billion_bodys_row_geometry(gpu, precision):
    """One layer of the Qwen2-0.5B rows: hidden 896 (no multiple of 256: other norm and GEMM routes), 14 heads over 2 KV
    heads through qwen2_slots, intermediate 4864. 5, 64 and 70 tokens in one call, and the 5 alone (f16: the folded
    route at K = 896)."""
    from voitta_rag_amd import encoder as enc

    shape = qo.Qwen2Shape(1, 896, 14, 2, 4864, vocab=300)
    w = qo.random_weights(shape, 81)
    rng = np.random.default_rng(82)
    seqs = [rng.integers(0, shape.vocab, size=n).astype(np.int32) for n in (5, 64, 70)]
    e = _engine(shape, "last", precision, w)
    want = qo.sentence_embeddings(w, shape, seqs, "last")
    _check(enc.encode(e, *_pack(seqs)).astype(np.float64), want, precision, "5 + 64 + 70 tokens")
    _check(enc.encode(e, *_pack(seqs[:1])).astype(np.float64), want[:1], precision, "5 tokens alone")
    e.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------
REFUSED = [
    (dict(position="learned"), r"norm VR_NORM_PRE_RMS_ROTARY needs position VR_POS_ROTARY \(position 0\)"),
    (dict(position="none"), r"norm VR_NORM_PRE_RMS_ROTARY needs position VR_POS_ROTARY \(position 2\)"),
    (dict(ffn="gelu"), r"norm VR_NORM_PRE_RMS_ROTARY needs a gated ffn \(ffn 0\)"),
    (dict(ffn="relu"), r"norm VR_NORM_PRE_RMS_ROTARY needs a gated ffn \(ffn 3\)"),
    (dict(window=8, global_every=2), r"norm VR_NORM_PRE_RMS_ROTARY takes no window \(window 8\)"),
    (dict(type_vocab=2), r"norm VR_NORM_PRE_RMS_ROTARY needs type_vocab 1 \(type_vocab 2\)"),
    (dict(causal=2), r"causal 2 must be 0 or 1"),
    (dict(norm="post", position="learned", ffn="gelu"), r"causal 1 needs norm VR_NORM_PRE_RMS_ROTARY \(norm 0\)"),
    (dict(norm="pre", ffn="geglu"), r"causal 1 needs norm VR_NORM_PRE_RMS_ROTARY \(norm 1\)"),
    (dict(norm="rms_pre", position="none", ffn="relu"), r"causal 1 needs norm VR_NORM_PRE_RMS_ROTARY \(norm 2\)"),
]


def test_refusals_name_the_field_and_leave_the_encoder_answering(gpu, path_refs):
    from voitta_rag_amd import encoder as enc

    w, refs = path_refs
    seqs, want = refs["skinny4"]
    ids, off = _pack(seqs)
    e = _engine(PATH_SHAPE, "last", "f32", w)
    before = enc.encode(e, ids, off)
    _check(before.astype(np.float64), want["last"], "f32", "before")
    names, state = enc.qwen2_slots(w, qo.desc_for(PATH_SHAPE, "last", "f32"))
    # (a description is refused before the tensors are counted: the 18-slot list serves the 16-slot ones too)
    for over, message in REFUSED:
        with pytest.raises(Exception, match=message):
            enc._load(e, qo.desc_for(PATH_SHAPE, "last", "f32", **over), state, names, e._lib.vr_encoder_load)
        assert np.array_equal(enc.encode(e, ids, off), before), message
    # neither a bias table nor slopes under the new norm
    for call, arg in ((e.set_attention_bias, np.zeros((2, 257), np.float32)), (e.set_attention_slopes, np.array([0.5, 0.25], np.float32))):
        with pytest.raises(Exception, match=r"an attention bias needs position VR_POS_LEARNED and norm VR_NORM_POST \(position 1, norm 3\)"):
            call(arg)
        assert np.array_equal(enc.encode(e, ids, off), before)
    # a reranker never takes the new norm; the embedder is untouched
    with pytest.raises(Exception, match=r"a reranker with norm VR_NORM_PRE_RMS_ROTARY is not supported \(norm 3\)"):
        enc._load(e, qo.desc_for(PATH_SHAPE, "cls", "f32", normalize=False, causal=0), state, names + [names[5]] * 4,
                  e._lib.vr_reranker_load)
    assert np.array_equal(enc.encode(e, ids, off), before)
    e.close()


# ---- 9. services -----------------------------------------------------------------------------------------------------------
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
        shape = qo.Qwen2Shape(2, 128, 2, 1, 256, vocab=-(-hf.get_vocab_size() // 8) * 8)
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
    shape, w, hf = qwen("qwen2-tiny", deferred=False)
    emb, sp, vs = (embedding.get_embedding_service(), sparse_embedding.get_sparse_embedding_service(),
                   vector_store.get_vector_store())
    model = emb.model
    assert isinstance(model.tokenizer, BpeTokenizer) and embedding.one_call_text_paths(model)
    assert (model.desc.norm, model.desc.causal, model.desc.pooling, model.desc.ffn, model.max_seq_length) == \
        ("rms_pre_rotary", 1, "last", "swiglu", 64)
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
    qwen("qwen2-tiny", deferred=True)
    emb, sp, vs = (embedding.get_embedding_service(), sparse_embedding.get_sparse_embedding_service(),
                   vector_store.get_vector_store())
    later = emb.embed_texts(texts)
    assert isinstance(later, deferred.DeferredEmbeddings)
    vs.store_chunks(list(zip(texts, later, _metas(len(texts)))), sparse_vectors=sp.embed_texts(texts))
    assert not later.materialized  # the fused indexing call took them
    assert np.array_equal(_bits(vs.client.get_dense(np.arange(len(texts)))), _bits(direct))
