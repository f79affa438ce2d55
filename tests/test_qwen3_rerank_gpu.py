"""Decoder cross-encoders on the GPU (vr_reranker_load_decoder: gather_last_rows_kernel, the last layer's tail at
M = n_seq, rerank_head_rms_kernel): logits against the transformers goldens and the f64 oracle at every precision and
every pair length, the head on the embedder's own rows, the n_seq edges of the tail, batch invariance, the bidirectional
body, one layer of the 0.6B row geometry, the ABI's refusals and replacements, and a synthetic qwen3 directory through
NativeCrossEncoder and VectorStoreService. Every test here fails without the feature (the symbol does not exist)."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import qwen3_oracle as qo
import qwen3_rerank_oracle as ro
from test_qwen3_rerank_cpu import GOLDENS, LENGTHS, golden, golden_row_logits
from test_rerank_gpu import BAR  # the project's bars for reranker logits: f32 1e-4, f16x3 1e-4, f16 5e-2

pytestmark = pytest.mark.gpu


def _pack(seqs):
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs).astype(np.int32), off


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _engine(shape, w, precision, **over):
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    e = Engine(shape.hidden)
    enc.load_reranker(e, ro.desc_for(shape, precision, **over), w, yes_id=ro.YES_ID, no_id=ro.NO_ID)
    return e


def _case(name):
    shape, tied, seed, seqs, logits = golden(name)
    return shape, ro.random_weights(shape, seed, tied), seqs, logits


def _report(what, precision, d):
    print(f"{what} {precision}: worst |logit - reference| = {float(np.max(d)):.3e} (bar {BAR[precision]:.0e})")


# ---- 1. the goldens ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", list(BAR))
@pytest.mark.parametrize("name", GOLDENS)
def test_logits_match_golden_and_oracle(gpu, name, precision):
    shape, w, seqs, logits = _case(name)
    oracle = np.asarray([r[-1] for r in golden_row_logits(name)])
    e = _engine(shape, w, precision)
    ids, off = _pack(seqs)
    got = e.rerank(ids, off, None)
    again = e.rerank(ids, off, None)
    d_gold, d_oracle = np.abs(got - logits), np.abs(got - oracle)
    _report(f"{name} vs transformers", precision, d_gold)
    _report(f"{name} vs f64 oracle", precision, d_oracle)
    print("  per pair length:", dict(zip(LENGTHS, np.round(d_gold, 7).tolist())))
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(again))
    alone = np.asarray([float(e.rerank(*_pack([s]), None)[0]) for s in seqs])  # another T, another GEMM route, a cached graph
    _report(f"{name} every pair alone", precision, np.abs(alone - logits))
    assert d_gold.max() <= BAR[precision] and d_oracle.max() <= BAR[precision]
    assert np.abs(alone - logits).max() <= BAR[precision]
    e.close()


# ---- 2. the head on the embedder's own rows ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_head_on_the_embedders_own_rows(gpu, name):
    """The same body through vr_encoder_load (last pooling, no normalisation, f32) runs its whole last layer on T rows and
    gives the final-normed last rows; the f64 dot of exactly those rows with score.weight is what the tail and the head
    kernel must give, to f32 rounding of H products of O(1) values: below the f32 bar."""
    from voitta_rag_amd import encoder as enc

    shape, w, seqs, _ = _case(name)
    e = _engine(shape, w, "f32")
    enc.load_encoder(e, ro.desc_for(shape, "f32"), ro.body_weights(w))
    ids, off = _pack(seqs)
    rows = enc.encode(e, ids, off).astype(np.float64)
    row32 = enc.qwen3_rerank_head(w, ro.desc_for(shape, "f32"), ro.YES_ID, ro.NO_ID)[0].astype(np.float64)
    d = np.abs(e.rerank(ids, off, None) - rows @ row32)
    _report(f"{name} head kernel vs f64 dot of the embedder's rows", "f32", d)
    assert d.max() <= BAR["f32"]
    e.close()


# ---- 3. the n_seq edges of the tail -----------------------------------------------------------------------------------------
EDGE = "tiny_d128b"
N_SEQ = [1, 15, 16, 17, 40, 65, 130]


@pytest.fixture(scope="module")
def edge_refs():
    """130 pairs of 2 .. 5 tokens and 40 of one token over tiny_d128b's weights, with the oracle's logits (once, read-only)."""
    shape, w, seqs, logits = _case(EDGE)
    rng = np.random.default_rng(61)
    short = [rng.integers(0, shape.vocab, size=int(n)).astype(np.int32) for n in rng.integers(2, 6, size=130)]
    ones = [np.asarray([t], np.int32) for t in rng.integers(0, shape.vocab, size=40)]
    want = {k: np.asarray([ro.logit(w, shape, s) for s in v]) for k, v in (("short", short), ("ones", ones))}
    for v in want.values():
        v.setflags(write=False)
    return shape, w, short, ones, want, seqs, logits


@pytest.mark.parametrize("precision", list(BAR))
@pytest.mark.parametrize("n_seq", N_SEQ)
def test_tail_rows_at_the_gemm_edges(gpu, edge_refs, n_seq, precision):
    """The M = n_seq products of the tail: one row, the folded-norm limit (16), a skinny block (64) and a 128-row tile crossed."""
    shape, w, short, _, want, _, _ = edge_refs
    e = _engine(shape, w, precision)
    d = np.abs(e.rerank(*_pack(short[:n_seq]), None) - want["short"][:n_seq])
    _report(f"{n_seq} pairs of 2..5 tokens", precision, d)
    assert d.max() <= BAR[precision]
    e.close()


@pytest.mark.parametrize("precision", list(BAR))
def test_one_token_pairs_and_a_streamed_pair_among_short_ones(gpu, edge_refs, precision):
    """T = n_seq: the tail's matrices are as many rows as the pass itself (larger than the Q/K/V buffer). Then a 321-token
    golden pair (f16: the streamed attention kernel at head size 128) between short ones."""
    shape, w, short, ones, want, seqs, logits = edge_refs
    e = _engine(shape, w, precision)
    d = np.abs(e.rerank(*_pack(ones), None) - want["ones"])
    _report("40 one-token pairs", precision, d)
    assert d.max() <= BAR[precision]
    at = LENGTHS.index(321)
    batch = short[:5] + [seqs[at]] + short[5:9]
    ref = np.concatenate([want["short"][:5], [logits[at]], want["short"][5:9]])
    d = np.abs(e.rerank(*_pack(batch), None) - ref)
    _report("a 321-token pair among 9 short ones", precision, d)
    assert d.max() <= BAR[precision]
    e.close()


# ---- 4. batch invariance ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", list(BAR))
@pytest.mark.parametrize("name", GOLDENS)
def test_a_pairs_logit_alone_and_as_pair_17_of_40(gpu, name, precision):
    """f32: one GEMM kernel whose rows do not meet, a gather, a wave per row in the head — the same bits. f16 / f16x3: the
    M = 1 and M = 40 products of the tail may take other kernels, so the two are within the bar of the reference."""
    shape, w, seqs, logits = _case(name)
    at = LENGTHS.index(100)
    rng = np.random.default_rng(5)
    crowd = [rng.integers(0, shape.vocab, size=int(n)).astype(np.int32) for n in rng.integers(2, 6, size=39)]
    batch = crowd[:17] + [seqs[at]] + crowd[17:]
    e = _engine(shape, w, precision)
    alone = e.rerank(*_pack([seqs[at]]), None)[0]
    crowded = e.rerank(*_pack(batch), None)[17]
    print(f"{name} {precision}: alone {alone!r}, as pair 17 of 40 {crowded!r}, transformers {logits[at]!r}")
    if precision == "f32":
        assert np.array_equal(_bits(np.float32(alone)), _bits(np.float32(crowded)))
    assert abs(alone - logits[at]) <= BAR[precision] and abs(crowded - logits[at]) <= BAR[precision]
    e.close()


# ---- 5. causal = 0 ----------------------------------------------------------------------------------------------------------
_bidirectional = {}  # per golden: the oracle's bidirectional logits, computed once


@pytest.mark.parametrize("precision", list(BAR))
@pytest.mark.parametrize("name", GOLDENS)
def test_causal_zero_is_the_body_run_bidirectionally(gpu, name, precision):
    shape, w, seqs, logits = _case(name)
    seqs, logits = seqs[:13], logits[:13]  # up to 200 tokens
    if name not in _bidirectional:
        _bidirectional[name] = np.asarray([ro.logit(w, shape, s, causal=False) for s in seqs])
    want = _bidirectional[name]
    # the two models are apart: a route that ignored causal = 0 would miss most pairs by more than twice the widest bar
    assert (np.abs(want - logits) > 2 * BAR["f16"]).sum() >= len(seqs) // 2
    e = _engine(shape, w, precision, causal=0)
    d = np.abs(e.rerank(*_pack(seqs), None) - want)
    _report(f"{name} bidirectional", precision, d)
    assert d.max() <= BAR[precision]
    e.close()


# ---- 6. the real row geometry -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", list(BAR))
def test_one_layer_of_the_0_6b_rows(gpu, precision):
    """hidden 1024, 16 heads of 128 over 8 KV heads (A = 2048), intermediate 3072, tied embeddings: 3 pairs of about 40 tokens."""
    shape = qo.Qwen3Shape(1, 1024, 16, 8, 3072, 128, vocab=300)
    w = ro.random_weights(shape, 83, True)
    rng = np.random.default_rng(84)
    seqs = [rng.integers(0, shape.vocab, size=n).astype(np.int32) for n in (38, 40, 43)]
    want = np.asarray([ro.logit(w, shape, s) for s in seqs])
    e = _engine(shape, w, precision)
    d = np.abs(e.rerank(*_pack(seqs), None) - want)
    _report("0.6B rows, 3 pairs", precision, d)
    assert d.max() <= BAR[precision]
    e.close()


# ---- 7. the ABI ---------------------------------------------------------------------------------------------------------------
def _raw_load(e, desc, tensors, load_fn):
    """desc and the tensors across the C ABI as they are (None: NULL)."""
    from voitta_rag_amd import encoder as enc

    keep = [None if t is None else np.ascontiguousarray(t, np.float32) for t in tensors]
    arr = (C.c_void_p * len(keep))(*[None if t is None else t.ctypes.data for t in keep])
    cdesc = desc.to_c()
    enc.check(load_fn(e.handle, C.byref(cdesc), arr, len(keep), enc.VR_MEM_HOST))


def test_refusals_name_the_field_and_replacement_works_both_ways(gpu):
    import rerank_oracle as bro
    from oracle import bert as obert

    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd._lib import EngineError

    shape, w, seqs, logits = _case("tiny_d64n")
    desc = ro.desc_for(shape, "f32")
    names, body = enc.qwen3_slots(ro.body_weights(w), desc)
    head = enc.qwen3_rerank_head(w, desc, ro.YES_ID, ro.NO_ID)
    tensors = [None if n is None else body[n] for n in names] + [head]
    n = len(tensors)
    assert n == 5 + 20 * shape.layers + 1
    # a BERT cross-encoder is loaded and answers
    bshape = obert.BertShape(2, 128, 4, 256, vocab=200, max_pos=64)
    bw = bro.random_weights(bshape, 8)
    bdesc = enc.BertDesc(2, 128, 4, 256, vocab=200, max_pos=64, pooling="cls", normalize=False, precision="f32")
    e = Engine(128)
    enc.load_reranker(e, bdesc, bw)
    bids, boff, bseg = np.arange(3, 33, dtype=np.int32), np.array([0, 30], np.int32), np.array([11], np.int32)
    before = e.rerank(bids, boff, bseg)
    assert abs(float(before[0]) - bro.logits(bw, bshape, bids, boff, bseg)[0]) <= BAR["f32"]
    load = e._lib.vr_reranker_load_decoder
    rep = dataclasses.replace
    refused = [
        (bdesc, r"a decoder reranker needs norm VR_NORM_PRE_RMS_ROTARY \(norm 0\)"),
        (rep(desc, norm="pre", causal=0, head_dim=0, qk_norm=0), r"a decoder reranker needs norm VR_NORM_PRE_RMS_ROTARY \(norm 1\)"),
        (rep(desc, norm="rms_pre", position="none", ffn="relu", causal=0, head_dim=0, qk_norm=0),
         r"a decoder reranker needs norm VR_NORM_PRE_RMS_ROTARY \(norm 2\)"),
        (rep(desc, position="learned"), r"a decoder reranker needs position VR_POS_ROTARY \(position 0\)"),
        (rep(desc, ffn="gelu"), r"a decoder reranker needs a gated ffn \(ffn 0\)"),
        (rep(desc, pooling="mean"), r"a decoder reranker reads the last token's row \(pooling 0\)"),
        (rep(desc, pooling="cls"), r"a decoder reranker reads the last token's row \(pooling 1\)"),
        (rep(desc, normalize=True), r"a decoder reranker pools without normalising \(normalize 1\)"),
        (rep(desc, type_vocab=2), r"a decoder reranker has one token type \(type_vocab 2\)"),
        (rep(desc, qk_norm=2), r"qk_norm 2 must be 0 or 1"),
        (rep(desc, causal=2), r"causal 2 must be 0 or 1"),
        (rep(desc, head_dim=96), r"head_dim 96 must be 0 \(hidden / heads\), 32, 64 or 128"),
        (rep(desc, window=8), r"norm VR_NORM_PRE_RMS_ROTARY takes no window \(window 8\)"),
    ]
    for bad, message in refused:
        with pytest.raises(EngineError, match=message):
            _raw_load(e, bad, tensors, load)
        assert np.array_equal(_bits(e.rerank(bids, boff, bseg)), _bits(before)), message  # the loaded one stays, bit for bit
    for bad_tensors, message in ((tensors[:-1], f"expected {n} tensors, got {n - 1}"), (tensors + [head], f"expected {n} tensors, got {n + 1}"),
                                 (tensors[:-1] + [None], f"tensor {n - 1} is null"), ([None] + tensors[1:], "tensor 0 is null")):
        with pytest.raises(EngineError, match=message):
            _raw_load(e, desc, bad_tensors, load)
        assert np.array_equal(_bits(e.rerank(bids, boff, bseg)), _bits(before)), message
    # vr_reranker_load keeps its old words for the same description
    for bad, message in ((desc, r"a reranker takes no causal mask \(causal 1\)"),
                         (rep(desc, causal=0), r"a reranker takes no head size of its own \(head_dim 64\)"),
                         (rep(desc, causal=0, head_dim=0), r"a reranker takes no query / key norms \(qk_norm 1\)"),
                         (rep(desc, causal=0, qk_norm=0, head_dim=0), r"a reranker with norm VR_NORM_PRE_RMS_ROTARY is not supported "
                          r"\(norm 3\): decoder cross-encoders are not implemented")):
        with pytest.raises(EngineError, match=message):
            _raw_load(e, bad, tensors, e._lib.vr_reranker_load)
        assert np.array_equal(_bits(e.rerank(bids, boff, bseg)), _bits(before)), message
    # the decoder replaces the BERT reranker, and the other way round; seg_b is not needed (and ignored where given)
    _raw_load(e, desc, tensors, load)
    ids, off = _pack(seqs[:8])
    got = e.rerank(ids, off, None)
    assert np.abs(got - logits[:8]).max() <= BAR["f32"]
    assert np.array_equal(_bits(e.rerank(ids, off, np.ones(8, np.int32))), _bits(got))
    with pytest.raises(EngineError, match="sequence 0 has 2000 tokens"):
        e.rerank(np.full(2000, 5, np.int32), np.array([0, 2000], np.int32), None)
    enc.load_reranker(e, bdesc, bw)
    assert np.array_equal(_bits(e.rerank(bids, boff, bseg)), _bits(before))
    enc.load_reranker(e, desc, w, yes_id=ro.YES_ID, no_id=ro.NO_ID)
    assert np.array_equal(_bits(e.rerank(ids, off, None)), _bits(got))
    e.close()


# ---- 8. services --------------------------------------------------------------------------------------------------------------
def _service_tokenizer():
    pytest.importorskip("tokenizers")
    from test_query_text_batch_gpu import WORDS

    return ro.make_tokenizer(ro.template_words() + sorted(set(WORDS)))


def _service_shape(tok):
    return qo.Qwen3Shape(2, 128, 2, 1, 256, 128, vocab=-(-tok.get_vocab_size() // 8) * 8)


def _oracle_logits(w, shape, row, ids, off):
    return np.asarray([ro.row_logits(w, shape, ids[off[i]:off[i + 1]], row=row)[-1] for i in range(len(off) - 1)])


@pytest.mark.parametrize("arch, tied", [("Qwen3ForCausalLM", True), ("Qwen3ForCausalLM", False), ("Qwen3ForSequenceClassification", True)])
def test_native_cross_encoder_from_a_directory(gpu, tmp_path, monkeypatch, arch, tied):
    from test_query_text_batch_gpu import WORDS

    from voitta_rag_amd import Engine, config
    from voitta_rag_amd.reranker import DecoderPairTokenizer, NativeCrossEncoder, sigmoid

    monkeypatch.setenv("VOITTA_RERANK_PRECISION", "f32")
    monkeypatch.delenv("VOITTA_RERANK_INSTRUCTION", raising=False)
    config.get_settings.cache_clear()
    tok = _service_tokenizer()
    shape = _service_shape(tok)
    path = str(tmp_path / "rr")
    w, row = ro.write_checkpoint(path, shape, 93, tok, arch, tied)
    e = Engine(128)
    rr = NativeCrossEncoder.from_pretrained(path, e, max_length=96)
    assert isinstance(rr.tokenizer, DecoderPairTokenizer) and rr.max_length == 96
    assert (rr.desc.norm, rr.desc.pooling, rr.desc.normalize, rr.desc.causal, rr.desc.head_dim, rr.desc.qk_norm, rr.desc.max_pos) == \
        ("rms_pre_rotary", "last", False, 1, 128, 1, 512)
    rng = np.random.default_rng(5)
    a = [" ".join(rng.choice(WORDS, size=int(rng.integers(1, 8)))) for _ in range(20)]
    b = [" ".join(rng.choice(WORDS, size=int(rng.integers(0, 90)))) for _ in range(20)]
    encode = lambda t: tok.encode(t, add_special_tokens=False).ids  # noqa: E731
    want_ids = [ro.assemble(encode, q, d, 96) for q, d in zip(a, b)]
    assert max(len(s) for s in want_ids) == 96  # (some bodies are cut)
    ids, off = _pack([np.asarray(s, np.int32) for s in want_ids])
    oracle = _oracle_logits(w, shape, row, ids, off)
    assert np.ptp(oracle) > 1.0
    got = rr.predict(list(zip(a, b)), activation=False)
    print(f"{arch} tied {tied}: worst |logit - oracle| = {np.abs(got - oracle).max():.3e}")
    assert got.dtype == np.float32 and np.abs(got - oracle).max() <= BAR["f32"]
    assert np.array_equal(_bits(got), _bits(e.rerank(ids, off, None)))  # the restated prompt's ids: the same call, the same bits
    assert np.abs(rr.predict(list(zip(a, b))) - sigmoid(oracle)).max() <= BAR["f32"]  # sigmoid(logit) is the published score
    ranked = rr.rank(a[0], b, top_k=4)
    one = _oracle_logits(w, shape, row, *_pack([np.asarray(ro.assemble(encode, a[0], d, 96), np.int32) for d in b]))
    assert len(ranked) == 4 and all(x["score"] >= y["score"] for x, y in zip(ranked, ranked[1:]))
    for r in ranked:
        assert abs(r["score"] - sigmoid(one[r["corpus_id"]])) <= BAR["f32"]
    best = np.argsort(-one, kind="stable")
    for k, r in enumerate(ranked):  # the oracle's order wherever its logits are more than twice the bar apart
        assert r["corpus_id"] == best[k] or abs(one[r["corpus_id"]] - one[best[k]]) <= 2 * BAR["f32"]
    # another instruction is another prompt
    other = NativeCrossEncoder.from_pretrained(path, e, max_length=96, instruction="rank the chunk")
    want = [ro.assemble(encode, a[1], b[1], 96, "rank the chunk")]
    ids1, off1 = _pack([np.asarray(s, np.int32) for s in want])
    assert abs(float(other.predict([(a[1], b[1])], activation=False)[0]) - _oracle_logits(w, shape, row, ids1, off1)[0]) <= BAR["f32"]
    e.close()
    config.get_settings.cache_clear()


@pytest.fixture
def reranked(monkeypatch, tmp_path, gpu):
    from test_query_text_batch_gpu import checkpoint

    from voitta_rag_amd import config, embedding, sparse_embedding, store_registry, vector_store

    path = str(tmp_path / "e5-mini")
    checkpoint(path, 384, 12, "mean")
    rpath = str(tmp_path / "qwen3-reranker-mini")
    tok = _service_tokenizer()
    shape = _service_shape(tok)
    w, row = ro.write_checkpoint(rpath, shape, 94, tok, "Qwen3ForCausalLM", True)
    for k, v in (("EMBEDDING_MODEL", path), ("EMBEDDING_DIMENSION", "384"), ("VOITTA_ENCODER_PRECISION", "f16"),
                 ("VOITTA_RERANK_MODEL", rpath), ("VOITTA_RERANK_CANDIDATES", "30"), ("VOITTA_RERANK_PRECISION", "f32")):
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("VOITTA_RERANK_INSTRUCTION", raising=False)

    def reset():
        config.get_settings.cache_clear()
        store_registry.reset()
        embedding._embedding_service = None
        sparse_embedding._sparse_embedding_service = None
        vector_store._vector_store = None

    reset()
    yield shape, w, row, tok
    reset()


def test_service_search_is_reranked(reranked):
    from test_query_text_batch_gpu import WORDS, questions

    from voitta_rag_amd.config import get_settings
    from voitta_rag_amd.embedding import get_embedding_service
    from voitta_rag_amd.reranker import DecoderPairTokenizer, get_reranker, sigmoid
    from voitta_rag_amd.sparse_embedding import get_sparse_embedding_service
    from voitta_rag_amd.vector_store import ChunkMetadata, VectorStoreService, get_vector_store

    shape, w, row, tok = reranked
    # (the reranker in f32: the pairs share most of their prompt, so their logits lie within a unit or two of each other,
    # and only the f32 bar is small against their gaps — the order below is then the oracle's, candidate by candidate)
    bar = BAR["f32"]
    rng = np.random.default_rng(8)
    emb, sp, vs = get_embedding_service(), get_sparse_embedding_service(), get_vector_store()
    texts = [" ".join(rng.choice(WORDS, size=int(rng.integers(3, 60)))) for _ in range(120)]
    metas = [ChunkMetadata(file_path="docs/a.md", folder_path="docs", index_folder="docs", file_name="a.md", chunk_index=i,
                           total_chunks=120, start_char=i, end_char=i + 1, indexed_at="2026-01-01T00:00:00",
                           source_modified_at=1_700_000_000 + i) for i in range(120)]
    vs.store_chunks(list(zip(texts, emb.embed_texts(texts), metas)), sparse_vectors=sp.embed_texts(texts))
    settings = get_settings()
    rr = get_reranker(vs._engine, settings.rerank_model)
    assert isinstance(rr.tokenizer, DecoderPairTokenizer) and rr.desc.rms_rotary and rr.max_length == 512
    unranked_before = VectorStoreService.unreranked_searches
    qs = questions(rng, 4)
    encode = lambda t: tok.encode(t, add_special_tokens=False).ids  # noqa: E731
    per_question = []
    for q in qs:
        limit = 7
        got = vs.search(emb.embed_query(q), limit=limit, sparse_query=sp.embed_query(q))
        settings.rerank_model = ""  # the first stage alone: unreranked top-C
        first = vs.search(emb.embed_query(q), limit=30, sparse_query=sp.embed_query(q))
        settings.rerank_model = os.environ["VOITTA_RERANK_MODEL"]
        ids, off = _pack([np.asarray(ro.assemble(encode, q, c.text, 512), np.int32) for c in first])
        oracle = _oracle_logits(w, shape, row, ids, off)
        order = np.argsort(-oracle, kind="stable")[:limit]
        assert len(got) == min(limit, len(first)) and np.ptp(oracle) > 0.5  # thousands of bars: the order means something
        assert (np.diff(np.sort(oracle)) > 2 * bar).mean() > 0.9  # ... and nearly every neighbouring pair is decided
        for k, c in enumerate(got):
            i = [x.id for x in first].index(c.id)
            assert abs(c.score - sigmoid(oracle[i])) <= bar
            assert c.id == first[order[k]].id or abs(oracle[i] - oracle[order[k]]) <= 2 * bar
        per_question.append(got)
    assert VectorStoreService.unreranked_searches == unranked_before
    # search_questions: every question's candidates in ONE vr_rerank call
    calls = []
    kind = type(rr.engine)
    real = kind.rerank

    def counted(self, ids, offsets, seg_b):
        calls.append(len(offsets) - 1)
        return real(self, ids, offsets, seg_b)

    kind.rerank = counted
    try:
        batch = vs.search_questions([{"query": q, "limit": 7} for q in qs])
    finally:
        kind.rerank = real
    assert len(calls) == 1 and calls[0] > 30
    for got, want in zip(batch, per_question):
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a.id == b.id or abs(a.score - b.score) <= 2 * bar
