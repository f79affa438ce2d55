"""The post-pooling head on the GPU (vr_encoder_set_head: pool_kernel's column limit, embed_head_kernel) against the f64
oracle of tests/head_oracle.py, and through every path that carries an embedding.

Shapes: a tiny encoder (2 layers, H 128, 2 heads, I 256) and one wide one (1 layer, H 1024, 16 heads, I 128: 64 column
tiles, the most the kernel takes); sequences of 1, 2, 15, 16, 17, 64 and 129 tokens. The cases are head_oracle.CASES."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import head_oracle as ho
from oracle import bert as obert
from oracle import core as ocore
from test_encoder_gpu import TOL

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _pack(seqs):
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs).astype(np.int32), off


def _desc(shape, pooling, normalize, precision, **kw):
    from voitta_rag_amd import encoder as enc

    return enc.BertDesc(shape.layers, shape.hidden, shape.heads, shape.intermediate, vocab=shape.vocab, max_pos=shape.max_pos,
                        type_vocab=shape.type_vocab, pooling=pooling, normalize=normalize, eps=shape.eps, precision=precision, **kw)


def _engine(case, precision, w, head=True, normalize=None, dim=None):
    """An engine (a store of `dim` columns: the encoder's width unless given) with the case's encoder loaded; head: with
    the case's head (through the description), else headless."""
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    e = Engine(dim or case.shape.hidden)
    kw = dict(head=ho.stage_objects(ho.head_weights(case)), truncate_dim=case.truncate) if head else {}
    enc.load_encoder(e, _desc(case.shape, case.pooling, case.normalize if normalize is None else normalize, precision, **kw), w)
    return e


@functools.lru_cache(maxsize=None)
def _ref(name):
    """(weights, sequences, f64 embeddings) of a case, computed once for all tests."""
    case = ho.CASES[name]
    w = obert.random_weights(case.shape, case.seed)
    seqs = ho.sequences(case)
    want = ho.expected(case, w, seqs)
    want.setflags(write=False)
    return w, seqs, want


def _check(got, want, precision, what):
    """test_encoder_gpu's check, both rows divided by the oracle row's norm (nothing for a unit row)."""
    assert got.shape == want.shape, (got.shape, want.shape)
    norm = np.linalg.norm(want, axis=1, keepdims=True)
    got, want = got.astype(np.float64) / norm, want / norm
    cos = (got * want).sum(1) / np.linalg.norm(got, axis=1)
    worst, worst_abs = float(np.max(np.abs(1.0 - cos))), float(np.max(np.abs(got - want)))
    print(f"{what} {precision}: worst |1-cos| = {worst:.3e}, worst abs diff = {worst_abs:.3e}")
    cos_tol, abs_tol = TOL[precision]
    assert worst < cos_tol and worst_abs < abs_tol, what


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", [(n, p) for n in ho.CASES for p in ("f32", "f16")] + [("labse", "f16x3"), ("two", "f16x3")])
def test_head_against_the_f64_oracle(gpu, name, precision):
    from voitta_rag_amd import encoder as enc

    case = ho.CASES[name]
    w, seqs, want = _ref(name)
    e = _engine(case, precision, w)
    assert e.encoder_desc.out_dim == case.out_dim
    got = enc.encode(e, *_pack(seqs))
    e.close()
    _check(got, want, precision, name)


# ---- 2. the head alone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["labse", "distiluse"])
def test_head_alone_within_the_f32_dot_product_bound(gpu, name):
    """The head (normalisation off) on the GPU's own pooled rows p, element by element against the f64 head of p:
    |error| <= (K + 8) 2^-24 (|p| |W|^T + |b|) + 8 2^-24 — the standard bound of a K-term f32 dot product plus the bias
    add, with a few ulp for tanhf, whose value is at most 1 and whose slope is at most 1."""
    from voitta_rag_amd import encoder as enc

    case = ho.CASES[name]
    w, seqs, _ = _ref(name)
    (st,) = ho.head_weights(case)
    ids, off = _pack(seqs)
    plain = _engine(case, "f32", w, head=False, normalize=False)
    p = enc.encode(plain, ids, off).astype(np.float64)
    plain.close()
    e = _engine(case, "f32", w, normalize=False)
    got = enc.encode(e, ids, off).astype(np.float64)
    e.close()
    want = ho.apply_stages(p, [st])
    K = st["weight"].shape[1]
    u = 2.0 ** -24
    bound = (K + 8) * u * (np.abs(p) @ np.abs(st["weight"].astype(np.float64)).T + np.abs(st["bias"].astype(np.float64))) + 8 * u
    ratio = float(np.max(np.abs(got - want) / bound))
    print(f"{name}: worst |error| / bound = {ratio:.3f}, worst |error| = {np.max(np.abs(got - want)):.3e}")
    assert ratio <= 1.0


# ---- 3. truncation ---------------------------------------------------------------------------------------------------------
def _spans(seqs):
    """Two or three spans for every sequence but the second (which only gives context)."""
    span_off, tok = [0], []
    for i, s in enumerate(seqs):
        n = len(s)
        mine = [] if i == 1 else [(0, n), (n // 2, n), (0, max(1, n // 3))]
        tok += mine
        span_off.append(span_off[-1] + len(mine))
    return np.asarray(span_off, np.int32), np.asarray(tok, np.int32).reshape(-1, 2)


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_truncated_rows_are_the_leading_columns_bit_for_bit(gpu, precision):
    from voitta_rag_amd import encoder as enc

    case = ho.CASES["trunc"]
    w, seqs, _ = _ref("trunc")
    ids, off = _pack(seqs)
    span_off, span_tok = _spans(seqs)
    plain = _engine(case, precision, w, head=False)
    e = _engine(case, precision, w)
    for _ in range(3):  # (the third call of a shape is a graph replay)
        full, cut = enc.encode(plain, ids, off), enc.encode(e, ids, off)
        assert full.shape == (len(seqs), 128) and cut.shape == (len(seqs), 16)
        assert np.array_equal(_bits(cut), _bits(full[:, :16]))
        full, cut = enc.encode_spans(plain, ids, off, span_off, span_tok), enc.encode_spans(e, ids, off, span_off, span_tok)
        assert full.shape == (int(span_off[-1]), 128) and cut.shape == (int(span_off[-1]), 16)
        assert np.array_equal(_bits(cut), _bits(full[:, :16]))
    plain.close()
    e.close()


@functools.lru_cache(maxsize=None)
def _span_ref(name):
    """(span_off, span_tok, f64 rows) of a case's sequences cut by _spans: the span means (whatever the description's
    pooling says) through the head."""
    case = ho.CASES[name]
    w, seqs, _ = _ref(name)
    span_off, span_tok = _spans(seqs)
    rows = []
    for i, s in enumerate(seqs):
        h = obert.encode_one(w, case.shape, s)
        rows += [h[b:e_].sum(axis=0) / (e_ - b) for b, e_ in span_tok[span_off[i]:span_off[i + 1]].tolist()]
    want = ho.apply_head(np.stack(rows), ho.head_weights(case), case.normalize, case.truncate)
    want.setflags(write=False)
    return span_off, span_tok, want


@pytest.mark.parametrize("name", ["labse", "ln_trunc"])
def test_spans_go_through_the_head(gpu, name):
    """vr_encode_spans with a head that has stages."""
    from voitta_rag_amd import encoder as enc

    case = ho.CASES[name]
    w, seqs, _ = _ref(name)
    span_off, span_tok, want = _span_ref(name)
    e = _engine(case, "f32", w)
    got = enc.encode_spans(e, *_pack(seqs), span_off, span_tok)
    e.close()
    _check(got, want, "f32", name + " spans")


@pytest.mark.parametrize("name", ["labse", "ln_trunc", "trunc"])
def test_index_batch_spans_stores_the_head_rows(gpu, name):
    """vr_index_batch_spans with a head (the fused late-chunked indexing call: the span means go through the encoder's
    pooled scratch and the stages into the engine's batch buffer, at the store's width — 128, 32 and 16 columns here):
    the stored rows are the oracle's, normalised as the store does, and encode_spans' rows through the cosine
    preprocessing bit for bit (the relation test_late_chunking_gpu pins without a head). 18 rows: two blocks of the
    head kernel. A store of another width than the head's output is refused with the message worded as without one."""
    from voitta_rag_amd import encoder as enc

    case = ho.CASES[name]
    w, seqs, _ = _ref(name)
    span_off, span_tok, want = _span_ref(name)
    ids, off = _pack(seqs)
    n = int(span_off[-1])
    e = _engine(case, "f32", w, dim=case.out_dim)
    assert e.index_batch_spans(ids, off, span_off, span_tok) == 0 and e.count()[0] == n == 18
    rows = enc.encode_spans(e, ids, off, span_off, span_tok)
    assert rows.shape == (n, case.out_dim)
    stored = e.get_dense(np.arange(n))
    _check(stored, want / np.linalg.norm(want, axis=1, keepdims=True), "f32", name + " index_batch_spans rows")
    assert np.array_equal(_bits(stored), _bits(ocore.cosine_preprocess(rows)))
    assert e.index_batch_spans(ids, off, span_off, span_tok) == n  # appended behind them, from a replayed shape
    assert np.array_equal(_bits(e.get_dense(np.arange(n, 2 * n))), _bits(stored))
    e.close()
    if case.out_dim != case.shape.hidden:
        e = _engine(case, "f32", w)  # a store as wide as the encoder, not as its head
        with pytest.raises(Exception, match=f"encoder width {case.out_dim} != store dimension {case.shape.hidden}"):
            e.index_batch_spans(ids, off, span_off, span_tok)
        assert e.count()[0] == 0
        e.close()


# ---- 4. row independence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", [("labse", "f32"), ("two", "f32"), ("ln_trunc", "f32"), ("labse", "f16")])
def test_a_row_does_not_depend_on_its_batch(gpu, name, precision):
    """33 sequences (three blocks of the head kernel, the last with one live row) against the rows 0, 15, 16 and 32
    encoded alone: wherever the headless pooled rows agree in bits between the two runs, the head's rows agree too. A
    second and third run of every shape (the third replays a captured graph) repeat their bits.
    The f32 encoder is batch-invariant (test_encoder_gpu.py), so there all four rows must take part; the f16 body
    routes its products by the token count, so its pooled rows may differ between the runs before any head sees them."""
    from voitta_rag_amd import encoder as enc

    case = ho.CASES[name]
    w = _ref(name)[0]
    rng = np.random.default_rng(5)
    seqs = [rng.integers(0, case.shape.vocab, size=int(n)).astype(np.int32) for n in rng.integers(1, 24, size=33)]
    plain = _engine(case, precision, w, head=False, normalize=False)
    e = _engine(case, precision, w)

    def run(eng, batch):
        first = enc.encode(eng, *_pack(batch))
        for _ in range(2):
            assert np.array_equal(_bits(enc.encode(eng, *_pack(batch))), _bits(first))
        return first

    base, got = run(plain, seqs), run(e, seqs)
    agreed = 0
    for r in (0, 15, 16, 32):
        base_alone, alone = run(plain, [seqs[r]]), run(e, [seqs[r]])
        if np.array_equal(_bits(base_alone[0]), _bits(base[r])):
            agreed += 1
            assert np.array_equal(_bits(alone[0]), _bits(got[r])), r
    print(f"{name} {precision}: {agreed} of 4 headless rows agree in bits alone and in the batch")
    assert agreed == 4 or precision != "f32"
    plain.close()
    e.close()


# ---- 5. forward chunks -----------------------------------------------------------------------------------------------------
CHUNK_LENS = [9] * 20 + [17] * 21 + [128, 3, 5, 60] + [7] * 35  # at 256 tokens a chunk: 28, 16, 14, 1, 3, 36, ... rows


def encode_chunk_batch(out_path=None):
    """The f32 rows of one batch under each head case that has stages (and `trunc`), and the headless un-normalised
    pooled rows of the same encoders ("pooled ..."): run here, and in a child process whose VR_CHUNK_TOKENS cuts the
    batch into forward chunks."""
    from voitta_rag_amd import encoder as enc

    out = {}
    for name in ("labse", "two", "ln_trunc", "trunc"):
        case = ho.CASES[name]
        w = obert.random_weights(case.shape, case.seed)
        rng = np.random.default_rng(6)
        seqs = [rng.integers(0, case.shape.vocab, size=n).astype(np.int32) for n in CHUNK_LENS]
        for key, kw in ((name, {}), ("pooled " + name, dict(head=False, normalize=False))):
            e = _engine(case, "f32", w, **kw)
            out[key] = enc.encode(e, *_pack(seqs))
            e.close()
    if out_path:
        np.savez(out_path, **out)
    return out


def test_forward_chunks_in_a_child_process(gpu, tmp_path):
    """VR_CHUNK_TOKENS is read when the library is loaded: the same batch in a fresh child process that cuts it into
    forward chunks of at most 256 tokens — 9 to 36 rows each, so that the head kernel's blocks of 16 rows start
    elsewhere and end on other live counts — gives the uncut run's rows bit for bit, every one of them. The runs are
    f32: there the encoder in front of the head is itself indifferent to the cut (the headless pooled rows must confirm
    it for every row), and the head's arithmetic is f32 in every precision. An f16 body routes its products by the
    chunk's token count, so its pooled rows differ between the two runs before any head sees them: such a run would
    assert nothing about the head, and there is none."""
    out_path = str(tmp_path / "chunked.npz")
    env = dict(os.environ, VR_CHUNK_TOKENS="256")
    code = (f"import sys; sys.path[:0] = {[os.path.dirname(HERE), HERE]!r}; import test_head_gpu as t; "
            f"t.encode_chunk_batch({out_path!r})")
    subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=120)
    chunked = np.load(out_path)
    whole = encode_chunk_batch()
    assert sorted(chunked.files) == sorted(whole) and len(whole) == 8
    for key, got in whole.items():
        if key.startswith("pooled"):
            continue
        assert got.shape[0] == len(CHUNK_LENS)
        same = (_bits(chunked["pooled " + key]) == _bits(whole["pooled " + key])).all(axis=1)
        print(f"{key}: {int(same.sum())} of {len(same)} headless rows have the uncut run's bits")
        assert same.all(), key
        assert np.array_equal(_bits(chunked[key]), _bits(got)), key


# ---- 6. set, remove, set ---------------------------------------------------------------------------------------------------
def test_set_remove_set_and_reload(gpu):
    from voitta_rag_amd import encoder as enc

    case = ho.CASES["labse"]
    w, seqs, want = _ref("labse")
    ids, off = _pack(seqs[:3])  # (a small shape: its second call is captured into a graph)
    stages = ho.stage_objects(ho.head_weights(case))
    never = _engine(case, "f16", w, head=False)
    base = [enc.encode(never, ids, off) for _ in range(3)][-1]
    never.close()
    e = _engine(case, "f16", w, head=False)
    for _ in range(3):
        assert np.array_equal(_bits(enc.encode(e, ids, off)), _bits(base))
    e.set_encoder_head(stages)
    assert e.encoder_desc.out_dim == 128 and e.encoder_desc.head is not None
    with_head = enc.encode(e, ids, off)  # (a graph of this shape exists from before the change: it must not be replayed)
    _check(with_head, want[:3], "f16", "set")
    assert not np.array_equal(_bits(with_head), _bits(base))
    for _ in range(2):
        assert np.array_equal(_bits(enc.encode(e, ids, off)), _bits(with_head))
    e.set_encoder_head(None)
    assert e.encoder_desc.head is None and e.encoder_desc.out_dim == 128
    for _ in range(3):
        assert np.array_equal(_bits(enc.encode(e, ids, off)), _bits(base))
    e.set_encoder_head([], truncate_dim=32)
    assert enc.encode(e, ids, off).shape == (3, 32)
    e.set_encoder_head(stages, truncate_dim=64)
    cut = enc.encode(e, ids, off)
    assert cut.shape == (3, 64) and np.array_equal(_bits(cut), _bits(with_head[:, :64]))
    # vr_encoder_load resets the head
    enc.load_encoder(e, _desc(case.shape, case.pooling, case.normalize, "f16"), w)
    assert e.encoder_desc.out_dim == 128
    for _ in range(3):
        assert np.array_equal(_bits(enc.encode(e, ids, off)), _bits(base))
    e.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_encoder_as_it_was(gpu):
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd.encoder import HeadStage

    case = ho.CASES["labse"]
    w, seqs, _ = _ref("labse")
    ids, off = _pack(seqs)
    z = lambda *shape: np.zeros(shape, np.float32)  # noqa: E731
    bad = [
        ("multiples of 16", [HeadStage("dense", z(24, 128))], 0),                                   # a width of 24
        ("multiples of 16", [HeadStage("dense", z(1040, 128))], 0),                                 # a width of 1040
        ("stage 1 reads 64 columns", [HeadStage("dense", z(128, 128)), HeadStage("dense", z(32, 64))], 0),   # the chain
        ("stage 0 reads 64 columns, the encoder has 128", [HeadStage("dense", z(32, 64))], 0),      # not the encoder's width
        ("0..4 allowed", [HeadStage("dense", z(128, 128))] * 5, 0),                                 # five stages
        ("truncate_dim 144", [HeadStage("dense", z(128, 128))], 144),                               # above the last width
        ("truncate_dim 144", [], 144),
        ("truncate_dim 24", [], 24),
        ("eps", [HeadStage("layernorm", z(128), eps=0.0)], 0),
    ]
    for with_head in (False, True):
        e = _engine(case, "f32", w, head=with_head)
        before = enc.encode(e, ids, off)
        desc = e.encoder_desc
        for message, stages, keep in bad:
            with pytest.raises(Exception, match=message):
                e.set_encoder_head(stages, keep)
            assert e.encoder_desc is desc
            assert np.array_equal(_bits(enc.encode(e, ids, off)), _bits(before)), message
        # a LayerNorm that changes its width cannot be written as a HeadStage (one weight vector): through the C struct
        import ctypes as C

        from voitta_rag_amd import _lib

        g = z(128) + 1
        st = _lib.VrHeadStage(C.sizeof(_lib.VrHeadStage), _lib.VR_HEAD_LAYERNORM, 128, 64, 0, 1e-5, g.ctypes.data, None)
        assert e._lib.vr_encoder_set_head(e.handle, C.byref(st), 1, 0, _lib.VR_MEM_HOST) != 0
        assert b"LayerNorm keeps its width" in e._lib.vr_last_error()
        assert np.array_equal(_bits(enc.encode(e, ids, off)), _bits(before))
        e.close()
    e = Engine(128)
    with pytest.raises(Exception, match="no encoder loaded"):
        e.set_encoder_head([HeadStage("dense", z(128, 128))])
    e.close()


# ---- 9. DistilBERT ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f16x3", "f16"])
def test_distilbert_body_matches_transformers_golden(gpu, precision):
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    g = np.load(os.path.join(HERE, "golden", "distilbert_tiny.npz"))
    shape = ho.DISTIL_SHAPE
    _, state = ho.distilbert_weights(prefix="distilbert.")
    desc = _desc(shape, "mean", True, precision)
    e = Engine(shape.hidden)
    enc.load_encoder(e, desc, enc.distilbert_slots(state, desc))
    got = enc.encode(e, g["ids"], g["offsets"])
    e.close()
    _check(got, g["want"], precision, "distilbert vs transformers f64")


# ---- 8. through the services -----------------------------------------------------------------------------------------------
@pytest.fixture
def services(monkeypatch, tmp_path, gpu):
    from voitta_rag_amd import config, embedding, sparse_embedding, store_registry, vector_store

    import test_query_text_batch_gpu as qt

    def reset():
        config.get_settings.cache_clear()
        store_registry.reset()
        embedding._embedding_service = None
        sparse_embedding._sparse_embedding_service = None
        vector_store._vector_store = None

    def make(name, family, pooling, modules, dim, **env):
        path = str(tmp_path / name)
        vocab = qt._vocab()
        shape, w = ho.write_checkpoint(path, vocab, family, pooling, modules, max_seq=160)
        for k, v in dict({"EMBEDDING_MODEL": path, "EMBEDDING_DIMENSION": str(dim), "VOITTA_ENCODER_PRECISION": "f32"}, **env).items():
            monkeypatch.setenv(k, v)
        reset()
        return shape, w, vocab

    yield make
    reset()


def _metas(n):
    from voitta_rag_amd.vector_store import ChunkMetadata

    return [ChunkMetadata(file_path="d/a.md", folder_path="d", index_folder="d", file_name="a.md", chunk_index=i, total_chunks=n,
                          start_char=0, end_char=1, indexed_at="t", source_modified_at=1_700_000_000 + i) for i in range(n)]


def _ranking(want, q, k):
    """The oracle's k best chunks for question row q: cosine of the f64 rows (the store and the search normalise)."""
    unit = want / np.linalg.norm(want, axis=1, keepdims=True)
    return np.argsort(-(unit @ unit[q]), kind="stable")[:k].tolist()


def test_services_with_a_distiluse_like_checkpoint(services):
    """DistilBERT weights, mean pooling, 2_Dense 128 -> 64 tanh, a store of 64 columns: embed_texts (deferred: the rows
    are encoded inside vr_index_batch) -> store_chunks -> search (a question that is still text: vr_query_text),
    search_questions (vr_query_text_batch) and BulkIndexer, against the oracle's rows and ranking."""
    import test_query_text_batch_gpu as qt
    from test_rope_gpu import _hf_seqs

    from voitta_rag_amd import embedding, vector_store
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd.indexer import BulkIndexer, ParsedFile
    from voitta_rag_amd.wordpiece import WordPieceTokenizer

    dense = ho.head_weights(ho.CASES["distiluse"])
    shape, w, vocab = services("distiluse-tiny", "distilbert", "mean", dense, 64)
    emb, vs = embedding.get_embedding_service(), vector_store.get_vector_store()
    model = emb.model
    assert isinstance(model.tokenizer, WordPieceTokenizer) and embedding.one_call_text_paths(model)
    assert (model.desc.hidden, model.desc.out_dim, model.desc.type_vocab, model.desc.normalize) == (128, 64, 1, False)
    rng = np.random.default_rng(3)
    texts = [" ".join(rng.choice(qt.WORDS, size=int(n))) for n in (3, 40, 9, 150, 1, 25, 12, 60, 17, 33, 5, 80)]
    seqs = _hf_seqs(vocab, texts, max_len=160)
    want = ho.apply_head(obert.sentence_embeddings(w, shape, seqs, "mean", False), dense, False)
    unit = want / np.linalg.norm(want, axis=1, keepdims=True)
    assert model.encode([]).shape == (0, 64)
    vectors = emb.embed_texts(texts)
    vs.store_chunks(list(zip(texts, vectors, _metas(len(texts)))))
    _check(vs.client.get_dense(np.arange(len(texts))), unit, "f32", "stored rows")
    _check(np.asarray(emb.embed_texts(texts), np.float64), want, "f32", "embed_texts")
    for q in (1, 7):
        got = vs.search(emb.embed_query(texts[q]), limit=4)
        assert [g.metadata.chunk_index for g in got] == _ranking(want, q, 4)
    got = vs.search_questions([{"query": texts[3], "limit": 3}, {"query": texts[9], "limit": 2}])
    assert [[g.metadata.chunk_index for g in r] for r in got] == [_ranking(want, 3, 3), _ranking(want, 9, 2)]
    # BulkIndexer: one more file, its chunks' rows against the oracle
    doc = "\n\n".join(" ".join(rng.choice(qt.WORDS, size=int(n))) + "." for n in (30, 45, 28))
    counts = BulkIndexer().index_files(iter([ParsedFile(content=doc, file_path="docs/0.md", folder_path="docs",
                                                        index_folder="docs", file_name="0.md", source_modified_at=1_710_000_000)]))
    n_new = counts["docs/0.md"]
    from voitta_rag_amd.chunking import get_chunking_service

    chunks = [str(c.text) for c in get_chunking_service().chunk_text(doc)]
    assert n_new == len(chunks) >= 1
    cw = ho.apply_head(obert.sentence_embeddings(w, shape, _hf_seqs(vocab, chunks, max_len=160), "mean", False), dense, False)
    _check(vs.client.get_dense(np.arange(len(texts), len(texts) + n_new)), cw / np.linalg.norm(cw, axis=1, keepdims=True), "f32",
           "BulkIndexer rows")
    # the batched text path: its embeddings are vr_encode's, and row i is vr_query_text of question i, bit for bit
    e = model.engine
    qt._store(e, model, np.random.default_rng(4))
    questions = [texts[1], "dense retrieval?", texts[8]]
    limits, weights = np.full(3, 10, np.int32), np.full(3, 0.1)
    res, qemb = e.query_text_batch(model.tokenizer, questions, questions, model.max_seq_length, limits, weights, [None] * 3,
                                   embeddings=True)
    assert qemb.shape == (3, 64)
    assert np.array_equal(_bits(qemb), _bits(enc.encode(e, *_pack(_hf_seqs(vocab, questions, max_len=160)))))
    ref = qt.expected(e, qemb, questions, limits, weights, [None] * 3, 0)
    for i in range(3):
        one = e.query_text(model.tokenizer, questions[i], questions[i], model.max_seq_length, 10, 0.1, 0, None)
        assert qt.same(res[i], ref[i]) and qt.same(one, res[i]), i


def test_services_with_truncation_and_late_chunking(services):
    """VOITTA_EMBED_TRUNCATE_DIM=32 on a BERT directory (mean, Normalize), a store of 32 columns, late chunking on: every
    chunk's row is the leading 32 columns of the normalised mean over its span — from embed_document (vr_encode_spans)
    and from BulkIndexer (vr_index_batch_spans) — searches rank as the oracle does, and row i of the batched text path
    is vr_query_text of question i in bits."""
    import test_query_text_batch_gpu as qt
    from test_rope_gpu import _hf_seqs

    from voitta_rag_amd import embedding, vector_store
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd import late_chunking as lc
    from voitta_rag_amd.chunking import get_chunking_service
    from voitta_rag_amd.config import get_settings
    from voitta_rag_amd.indexer import BulkIndexer, ParsedFile

    shape, w, vocab = services("bert-matryoshka", "bert", "mean", ["Normalize"], 32, VOITTA_EMBED_TRUNCATE_DIM="32",
                               VOITTA_LATE_CHUNKING="1")
    emb, vs = embedding.get_embedding_service(), vector_store.get_vector_store()
    model = emb.model
    assert (model.desc.hidden, model.desc.out_dim, model.desc.truncate_dim, model.desc.head) == (128, 32, 32, None)
    rng = np.random.default_rng(8)

    def document():
        return "\n\n".join(" ".join(" ".join(rng.choice(qt.WORDS, size=int(rng.integers(5, 12)))) + "." for _ in range(3))
                           for _ in range(4))

    def late_rows(doc):
        """The document's chunks and the oracle's rows for them: the leading 32 columns of each span's normalised mean."""
        chunks = [c.text for c in get_chunking_service().chunk_texts([doc])[0]]
        assert len(chunks) >= 2 and all(type(t) is lc.LateChunkText for t in chunks)
        plan = lc.plan(doc, chunks, model.tokenize, model.max_seq_length, get_settings().late_chunking_context)
        h = [obert.encode_one(w, shape, plan.ids[a:b]) for a, b in zip(plan.offsets[:-1], plan.offsets[1:])]
        seq_of = np.repeat(np.arange(plan.n_seq), np.diff(plan.span_off))
        rows = np.stack([h[s][a:b].sum(axis=0) / (b - a) for s, (a, b) in zip(seq_of, plan.span_tok.tolist())])
        return chunks, ho.apply_head(rows, [], True, 32)

    doc = document()
    chunks, want = late_rows(doc)
    got = np.asarray(emb.embed_document(doc, [str(t) for t in chunks]), np.float64)
    assert got.shape == (len(chunks), 32)
    _check(got, want, "f32", "late-chunked truncated rows")
    # plain texts, stored and found
    texts = [" ".join(rng.choice(qt.WORDS, size=int(n))) for n in (3, 40, 9, 100, 1, 25, 12, 60)]
    tw = ho.apply_head(obert.sentence_embeddings(w, shape, _hf_seqs(vocab, texts, max_len=160), "mean", False), [], True, 32)
    vectors = emb.embed_texts(texts)
    vs.store_chunks(list(zip(texts, vectors, _metas(len(texts)))))
    _check(vs.client.get_dense(np.arange(len(texts))), tw / np.linalg.norm(tw, axis=1, keepdims=True), "f32", "stored rows")
    got = vs.search(emb.embed_query(texts[5]), limit=3)
    assert [g.metadata.chunk_index for g in got] == _ranking(tw, 5, 3)
    got = vs.search_questions([{"query": texts[3], "limit": 3}])
    assert [g.metadata.chunk_index for g in got[0]] == _ranking(tw, 3, 3)
    # BulkIndexer: two more files, cut and encoded in the context of their documents inside the fused indexing call
    docs = [document(), document()]
    counts = BulkIndexer().index_files(iter([ParsedFile(content=d, file_path=f"docs/{i}.md", folder_path="docs", index_folder="docs",
                                                        file_name=f"{i}.md", source_modified_at=1_710_000_000 + i)
                                             for i, d in enumerate(docs)]))
    made = [late_rows(d) for d in docs]
    assert counts == {f"docs/{i}.md": len(c) for i, (c, _) in enumerate(made)}
    bw = np.concatenate([r for _, r in made])
    stored = vs.client.get_dense(np.arange(len(texts), len(texts) + len(bw)))
    assert stored.shape == (len(bw), 32)
    _check(stored, bw / np.linalg.norm(bw, axis=1, keepdims=True), "f32", "BulkIndexer late-chunked truncated rows")
    # the batched text path at the truncated width: its embeddings are vr_encode's, and row i is vr_query_text of question i
    e = model.engine
    qt._store(e, model, np.random.default_rng(4))
    questions = [texts[1], "dense retrieval?", texts[6]]
    limits, weights = np.full(3, 10, np.int32), np.full(3, 0.1)
    res, qemb = e.query_text_batch(model.tokenizer, questions, questions, model.max_seq_length, limits, weights, [None] * 3,
                                   embeddings=True)
    assert qemb.shape == (3, 32)
    assert np.array_equal(_bits(qemb), _bits(enc.encode(e, *_pack(_hf_seqs(vocab, questions, max_len=160)))))
    ref = qt.expected(e, qemb, questions, limits, weights, [None] * 3, 0)
    for i in range(3):
        one = e.query_text(model.tokenizer, questions[i], questions[i], model.max_seq_length, 10, 0.1, 0, None)
        assert qt.same(res[i], ref[i]) and qt.same(one, res[i]), i
