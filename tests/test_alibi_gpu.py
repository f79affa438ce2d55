"""ALiBi encoders (jina-embeddings-v2) on the GPU: a model without positions whose attention logits lose
slope_h |key - query| in all three attention kernels. The f64 oracle at every precision for both head sizes and a
six-head (non-power-of-two) slope sequence; random slopes on one batch per GEMM route with both poolings, and once more
with VR_ENCODE_FUSE=0 in a fresh child process; the staged kernel at its largest, the first streamed length and beyond,
where the bias reaches past anything a table could say; position "none" against a zero position table, and slopes against
the table -m |offset|; setting and removing the slopes against engines that never knew the other state;
vr_encode_spans; the refusals; and the services on a jina-v2-shaped checkpoint directory."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import alibi_oracle as ao
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


def _engine(shape, pooling, precision, w, slopes=None, **over):
    """An engine with the model loaded; slopes: carried by the description, as a checkpoint directory's are."""
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    e = Engine(shape.hidden)
    enc.load_encoder(e, ao.desc_for(shape, pooling, precision, attention_slopes=slopes, **over), w)
    return e


def _random_slopes(heads, seed):
    """In (0, 1], independent: a head-order mix-up cannot hide behind a monotone sequence."""
    return (1.0 - np.random.default_rng(seed).random(heads)).astype(np.float32)


# ---- 1. the oracle at every precision ----------------------------------------------------------------------------------
MODELS = {"d64": ao.AlibiShape(2, 128, 2, 256), "d32": ao.AlibiShape(2, 128, 4, 256), "six": ao.AlibiShape(2, 384, 6, 256)}
LENS = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257, 512]


@pytest.fixture(scope="module")
def model_refs():
    """Per model: weights, the model's own slopes, the sequences and the oracle's mean-pooled rows (once, read-only)."""
    from voitta_rag_amd.encoder import alibi_slopes

    out = {}
    for i, (name, shape) in enumerate(MODELS.items()):
        w = ao.random_weights(shape, 21 + i)
        slopes = alibi_slopes(shape.heads)
        rng = np.random.default_rng(31 + i)
        seqs = [rng.integers(4, shape.vocab, size=n).astype(np.int32) for n in LENS]
        want = ao.sentence_embeddings(w, shape, seqs, slopes)
        want.setflags(write=False)
        out[name] = (shape, w, slopes, seqs, want)
    return out


@pytest.mark.parametrize("precision", list(TOL))
@pytest.mark.parametrize("name", list(MODELS))
def test_encoder_matches_the_oracle(gpu, model_refs, name, precision):
    from voitta_rag_amd import encoder as enc

    shape, w, slopes, seqs, want = model_refs[name]
    assert shape.heads != 6 or not np.allclose(slopes[4], slopes[3] / 4)  # six heads: not one geometric sequence
    e = _engine(shape, "mean", precision, w, slopes)
    _check(enc.encode(e, *_pack(seqs)).astype(np.float64), want, precision, name)
    # the first and the last sequence alone, twice each: the second run replays the cached graph where one is cached
    for i in (0, len(seqs) - 1):
        runs = [enc.encode(e, *_pack(seqs[i:i + 1])) for _ in range(2)]
        _check(runs[0].astype(np.float64), want[i:i + 1], precision, f"{name} sequence {i} alone")
        assert np.array_equal(_bits(runs[0]), _bits(runs[1])), i
    e.close()


# ---- 2. random slopes on one batch per GEMM route ------------------------------------------------------------------------
PATH_SHAPE = ao.AlibiShape(3, 128, 2, 256)
PATH_SLOPES = _random_slopes(PATH_SHAPE.heads, 50)


def path_batches():
    w = ao.random_weights(PATH_SHAPE, 51)
    rng = np.random.default_rng(52)
    batches = {}
    for name, lens in PATH_LENS.items():
        seqs = [rng.integers(4, PATH_SHAPE.vocab, size=n).astype(np.int32) for n in lens[:8]]
        batches[name] = (seqs * (len(lens) // len(seqs) + 1))[:len(lens)]
    return w, batches


@pytest.fixture(scope="module")
def path_refs():
    """Per batch: the sequences, the f64 oracle's embeddings for both poolings, and its final hidden states of each
    sequence (every distinct sequence computed once, shared, read-only)."""
    w, batches = path_batches()
    refs, hidden = {}, {}
    for name, seqs in batches.items():
        want = {"mean": [], "cls": []}
        for s in seqs:
            key = s.tobytes()
            if key not in hidden:
                hidden[key] = ao.encode_one(w, PATH_SHAPE, s, PATH_SLOPES)
                hidden[key].setflags(write=False)
            for pooling in want:
                want[pooling].append(ao.pool(hidden[key], pooling))
        refs[name] = (seqs, {k: np.stack(v) for k, v in want.items()}, [hidden[s.tobytes()] for s in seqs])
        for v in refs[name][1].values():
            v.setflags(write=False)
    return w, refs


@pytest.mark.parametrize("pooling", ["mean", "cls"])
@pytest.mark.parametrize("precision", ["f16", "f32"])
@pytest.mark.parametrize("batch", list(PATH_LENS))
def test_every_gemm_route(gpu, path_refs, batch, precision, pooling):
    """(cls in f16: the last layer runs the CLS tail, attention over the first query tile alone — with the bias.)"""
    from voitta_rag_amd import encoder as enc

    w, refs = path_refs
    seqs, want, _ = refs[batch]
    e = _engine(PATH_SHAPE, pooling, precision, w)
    e.set_attention_slopes(PATH_SLOPES)
    _check(enc.encode(e, *_pack(seqs)).astype(np.float64), want[pooling], precision, f"{batch} {pooling}")
    e.close()


def encode_path_batches(out_path=None):
    from voitta_rag_amd import encoder as enc

    w, batches = path_batches()
    out = {}
    for precision in ("f16", "f32"):
        for pooling in ("mean", "cls"):
            e = _engine(PATH_SHAPE, pooling, precision, w, PATH_SLOPES)
            for name, seqs in batches.items():
                out[f"{name} {precision} {pooling}"] = enc.encode(e, *_pack(seqs))
            e.close()
    if out_path:
        np.savez(out_path, **out)
    return out


def test_unfused_passes_in_a_child_process(gpu, path_refs, tmp_path):
    """VR_ENCODE_FUSE is read when a model is loaded: the same batches, loaded and run in a fresh child process with the
    gate as a pass of its own, against the same oracle rows."""
    out_path = str(tmp_path / "unfused.npz")
    env = dict(os.environ, VR_ENCODE_FUSE="0")
    code = (f"import sys; sys.path[:0] = {[os.path.dirname(HERE), HERE]!r}; import test_alibi_gpu as t; "
            f"t.encode_path_batches({out_path!r})")
    subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=120)
    unfused = np.load(out_path)
    _, refs = path_refs
    assert len(unfused.files) == 4 * len(PATH_LENS)
    for key in unfused.files:
        batch, precision, pooling = key.split()
        _check(unfused[key].astype(np.float64), refs[batch][1][pooling], precision, "unfused " + key)


# ---- 3. staged and streamed edges ----------------------------------------------------------------------------------------
# slopes small enough that keys more than 512 tokens away still carry weight (2^-8 * 1100 = 4.3 in the logit)
LONG_MODELS = {64: (ao.AlibiShape(2, 128, 2, 256), np.array([2.0 ** -8, 2.0 ** -10], np.float32), 61),
               32: (ao.AlibiShape(2, 128, 4, 256), np.array([2.0 ** -7, 2.0 ** -10, 2.0 ** -9, 2.0 ** -8], np.float32), 62)}


@pytest.mark.parametrize("dh,n", [(64, 640), (64, 656), (64, 1100), (32, 1400)])
def test_staged_and_streamed_edges(gpu, dh, n):
    """d_h = 64: 640 keys are the most the staged kernel holds, 160 KiB of LDS, which the slopes instantiation has to
    have been told (hipFuncSetAttribute); 656 tokens are the first streamed length (no byte of LDS goes to the slopes,
    so the edge is where it is without a bias); 1100 and, at d_h = 32, 1400 tokens stream. One sequence per call, f16,
    mean pooling (every query of the last layer) and CLS pooling (its tail: the first query tile alone).
    From 513 tokens on the bias reaches past a radius-512 table. The sequence starts and ends with a run of one token
    each, so that weight moved between near and far keys moves the context: the oracle with the distance saturated at
    512 puts the [CLS] row further from the oracle's than twice the tolerance — a kernel that saturated would fail."""
    from voitta_rag_amd import encoder as enc

    shape, slopes, seed = LONG_MODELS[dh]
    assert shape.hidden // shape.heads == dh
    w = ao.random_weights(shape, seed)
    s = np.random.default_rng(n).integers(4, shape.vocab, size=n).astype(np.int32)
    s[:n // 5], s[-(n // 5):] = 7, 9
    hidden = ao.encode_one(w, shape, s, slopes)
    saturated = ao.encode_one(w, shape, s, slopes, bias=ao.distance_bias(slopes, n, clamp=512))
    seen = float(np.max(np.abs(ao.pool(saturated, "cls") - ao.pool(hidden, "cls"))))
    print(f"{n} tokens: a bias saturated at 512 moves the [CLS] embedding by {seen:.3e}")
    assert seen > 2 * TOL["f16"][1]
    for pooling in ("mean", "cls"):
        e = _engine(shape, pooling, "f16", w, slopes)
        _check(enc.encode(e, *_pack([s])).astype(np.float64), ao.pool(hidden, pooling)[None], "f16", f"{n} tokens {pooling}")
        e.close()


# ---- 4. differential: no oracle ------------------------------------------------------------------------------------------
def _learned_twin(shape, pooling, precision, w, max_pos=513, table=None):
    """The same weights behind VR_POS_LEARNED with an all-zero position table (a GeGLU description with a position
    table is no checkpoint family's: its slots are jina_slots' with slot 1 filled in, loaded through the slot-level
    loader)."""
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    e = Engine(shape.hidden)
    desc = ao.desc_for(shape, pooling, precision, max_pos=max_pos, position="learned", attention_bias=table)
    zero = np.zeros((max_pos, shape.hidden), np.float32)
    if shape.ffn == "gelu":
        enc.load_encoder(e, desc, dict(w, **{"embeddings.position_embeddings.weight": zero}))
        return e
    names, state = enc.jina_slots(w, desc)
    names[1] = "embeddings.position_embeddings.weight"
    state[names[1]] = zero
    enc._load(e, desc, state, names, e._lib.vr_encoder_load)
    e.encoder_desc = desc
    if table is not None:
        e.set_attention_bias(table)
    return e


@pytest.mark.parametrize("precision", ["f16", "f32"])
@pytest.mark.parametrize("ffn", ["gelu", "geglu"])
def test_position_none_is_a_zero_position_table_bit_for_bit(gpu, ffn, precision):
    from voitta_rag_amd import encoder as enc

    shape = ao.AlibiShape(2, 128, 2, 256, ffn=ffn)
    w = ao.random_weights(shape, 71)
    rng = np.random.default_rng(72)
    batches = [[rng.integers(4, shape.vocab, size=n).astype(np.int32) for n in lens]
               for lens in ([5], PATH_LENS["skinny4"], PATH_LENS["mid"], LENS)]
    for pooling in ("mean", "cls"):
        none, learned = _engine(shape, pooling, precision, w, max_pos=513), _learned_twin(shape, pooling, precision, w)
        for seqs in batches:
            a, b = enc.encode(none, *_pack(seqs)), enc.encode(learned, *_pack(seqs))
            assert np.isfinite(a).all() and np.array_equal(_bits(a), _bits(b)), (pooling, len(seqs))
        none.close()
        learned.close()


@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_slopes_and_the_linear_table_meet_at_the_oracle(gpu, precision):
    """Sequences of at most 513 tokens never leave the radius-512 table -m_h |offset|. The two routes round differently
    (an fma on the distance; a table entry added), so both are held to the oracle, not to each other."""
    from voitta_rag_amd import encoder as enc

    shape = ao.AlibiShape(2, 128, 2, 256, ffn="gelu")
    w = ao.random_weights(shape, 73)
    slopes = _random_slopes(2, 74)
    rng = np.random.default_rng(75)
    seqs = [rng.integers(4, shape.vocab, size=n).astype(np.int32) for n in (1, 17, 64, 129, 300, 513)]
    want = ao.sentence_embeddings(w, shape, seqs, slopes)
    table = (-slopes.astype(np.float64)[:, None] * np.abs(np.arange(-512, 513))[None, :]).astype(np.float32)
    by_table = _learned_twin(shape, "mean", precision, w, table=table)
    by_slopes = _learned_twin(shape, "mean", precision, w)
    by_slopes.set_attention_slopes(slopes)
    got = {}
    for what, e in (("table", by_table), ("slopes", by_slopes)):
        got[what] = enc.encode(e, *_pack(seqs))
        _check(got[what].astype(np.float64), want, precision, what)
        e.close()
    print(f"slopes against table: max abs difference {float(np.max(np.abs(got['table'] - got['slopes']))):.3e}")


# ---- 5. set, remove, set -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_removed_slopes_are_the_engine_that_never_had_any_and_back(gpu, path_refs, precision):
    """One short sequence (its forward pass is captured and replayed as a graph) and one batch, each run twice in every
    state: a graph that survived a change would replay the other state's kernels."""
    from voitta_rag_amd import encoder as enc

    w, refs = path_refs
    one = _pack(refs["skinny1"][0][2:3])
    batch = _pack(refs["mid"][0])

    def runs(e):
        return [_bits(enc.encode(e, *x)) for x in (one, one, batch, batch)]

    never = _engine(PATH_SHAPE, "mean", precision, w)
    always = _engine(PATH_SHAPE, "mean", precision, w, PATH_SLOPES)
    plain, biased = runs(never), runs(always)
    assert not np.array_equal(plain[0], biased[0]) and not np.array_equal(plain[2], biased[2])
    e = _engine(PATH_SHAPE, "mean", precision, w, PATH_SLOPES)
    for state in (biased, plain, biased, plain):
        e.set_attention_slopes(PATH_SLOPES if state is biased else None)
        for got, want in zip(runs(e), state):
            assert np.array_equal(got, want)
    # vr_encoder_load resets them
    e.set_attention_slopes(PATH_SLOPES)
    enc.load_encoder(e, ao.desc_for(PATH_SHAPE, "mean", precision), w)
    for got, want in zip(runs(e), plain):
        assert np.array_equal(got, want)
    for x in (never, always, e):
        x.close()


# ---- 6. spans ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_span_rows_are_the_oracles_span_means(gpu, path_refs, precision):
    from voitta_rag_amd import encoder as enc

    w, refs = path_refs
    seqs, _, hidden = refs["mid"]
    spans = [[(0, 129), (120, 129), (7, 8)], [(0, 10), (5, 300), (150, 290)], [(0, 1)], [], [(70, 77), (0, 77)]]
    span_off = np.zeros(len(seqs) + 1, np.int32)
    span_off[1:] = np.cumsum([len(s) for s in spans])
    span_tok = np.array([p for s in spans for p in s], np.int32)
    want = np.stack([ao.pool(hidden[i][a:b], "mean") for i, s in enumerate(spans) for a, b in s])
    e = _engine(PATH_SHAPE, "cls", precision, w, PATH_SLOPES)  # (the description's pooling is ignored by a span call)
    ids, off = _pack(seqs)
    _check(enc.encode_spans(e, ids, off, span_off, span_tok).astype(np.float64), want, precision, "spans")
    e.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_loaded_encoder_unchanged(gpu, path_refs):
    import modernbert_oracle as mo
    import rope_oracle as ro

    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    w, refs = path_refs
    seqs, want, _ = refs["skinny4"]
    ids, off = _pack(seqs)
    e = _engine(PATH_SHAPE, "mean", "f32", w, PATH_SLOPES)
    before = enc.encode(e, ids, off)
    _check(before.astype(np.float64), want["mean"], "f32", "before")
    for slopes, message in ((np.array([0.5, 0.25, 0.125], np.float32), "3 attention slopes for an encoder of 2 heads"),
                            (np.array([0.5, -0.25], np.float32), "attention slope -0.25 of head 1 must be finite"),
                            (np.array([np.nan, 0.25], np.float32), "attention slope nan of head 0 must be finite"),
                            (np.array([0.5, np.inf], np.float32), "attention slope inf of head 1 must be finite")):
        with pytest.raises(Exception, match=message):
            e.set_attention_slopes(slopes)
        assert np.array_equal(enc.encode(e, ids, off), before), message
    with pytest.raises(ValueError, match="expected .heads."):
        e.set_attention_slopes(np.zeros((2, 2), np.float32))
    e.close()
    # slopes and a table never coexist: on a learned-position model either is accepted, the second one refused
    gelu = ao.AlibiShape(2, 128, 2, 256, ffn="gelu")
    wg = ao.random_weights(gelu, 81)
    table = np.random.default_rng(82).normal(size=(2, 17)).astype(np.float32)
    e = _learned_twin(gelu, "mean", "f32", wg)
    e.set_attention_slopes(PATH_SLOPES)
    before = enc.encode(e, ids, off)
    with pytest.raises(Exception, match="has attention slopes"):
        e.set_attention_bias(table)
    assert np.array_equal(enc.encode(e, ids, off), before)
    e.set_attention_slopes(None)
    e.set_attention_bias(table)
    before = enc.encode(e, ids, off)
    with pytest.raises(Exception, match="has an attention bias table"):
        e.set_attention_slopes(PATH_SLOPES)
    assert np.array_equal(enc.encode(e, ids, off), before)
    e.close()
    # a model without positions takes no table (that needs a position table's description, as before)
    e = _engine(PATH_SHAPE, "mean", "f32", w, PATH_SLOPES)
    before = enc.encode(e, ids, off)
    with pytest.raises(Exception, match="needs position VR_POS_LEARNED and norm VR_NORM_POST"):
        e.set_attention_bias(table)
    assert np.array_equal(enc.encode(e, ids, off), before)
    e.close()
    # a rotary description, and a pre-norm one: refused with the table's sentence, and they run as they did
    rope_shape = ro.RopeShape(2, 128, 2, 256, vocab=300, max_pos=512, act="gelu")
    modern_shape = mo.ModernShape(2, 128, 2, 256, vocab=300, max_pos=512, window=8)
    for desc, weights, stated in ((ro.desc_for(rope_shape, "mean", "f32"), ro.random_weights(rope_shape, 3), "position 1, norm 0"),
                                  (mo.desc_for(modern_shape, "mean", "f32"), mo.random_weights(modern_shape, 4), "position 1, norm 1")):
        e = Engine(128)
        enc.load_encoder(e, desc, weights)
        before = enc.encode(e, ids, off)
        with pytest.raises(Exception, match=r"an attention bias needs position VR_POS_LEARNED and norm VR_NORM_POST \(" + stated):
            e.set_attention_slopes(PATH_SLOPES)
        e.set_attention_slopes(None)  # nothing to remove: accepted
        assert np.array_equal(enc.encode(e, ids, off), before)
        e.close()
    e = Engine(128)
    for slopes in (PATH_SLOPES, None):
        with pytest.raises(Exception, match="no encoder loaded"):
            e.set_attention_slopes(slopes)
    e.close()
    # position "none" with norm "pre" (and with a window) at load: refused, the loaded encoder stays
    e = _engine(PATH_SHAPE, "mean", "f32", w, PATH_SLOPES)
    before = enc.encode(e, ids, off)
    names, state = enc.jina_slots(w, ao.desc_for(PATH_SHAPE, "mean", "f32"))
    for over, message in ((dict(norm="pre"), "position VR_POS_NONE needs norm VR_NORM_POST"),
                          (dict(window=8, global_every=2), "position VR_POS_NONE takes no window")):
        with pytest.raises(Exception, match=message):
            enc._load(e, ao.desc_for(PATH_SHAPE, "mean", "f32", **over), state, names, e._lib.vr_encoder_load)
        assert np.array_equal(enc.encode(e, ids, off), before), message
    e.close()


# ---- 8. services ---------------------------------------------------------------------------------------------------------
def jina_checkpoint(d, seed=91, extra=None):
    """A jina-embeddings-v2-shaped sentence-transformers directory: config.json (model_type bert, alibi, geglu), mean
    pooling, Normalize, the WordPiece fixture vocabulary, seeded weights under JinaBert's names with the `bert.` prefix
    and a pooler, as the published checkpoints carry."""
    import test_query_text_batch_gpu as qt
    from safetensors.numpy import save_file

    os.makedirs(os.path.join(d, "1_Pooling"), exist_ok=True)
    vocab = qt._vocab()
    shape = ao.AlibiShape(2, 128, 2, 256, vocab=len(vocab))
    json.dump({"architectures": ["JinaBertForMaskedLM"], "model_type": "bert", "position_embedding_type": "alibi",
               "feed_forward_type": "geglu", "hidden_act": "gelu", "hidden_size": 128, "num_hidden_layers": 2,
               "num_attention_heads": 2, "intermediate_size": 256, "vocab_size": len(vocab), "max_position_embeddings": 8192,
               "type_vocab_size": 2, "layer_norm_eps": shape.eps, "emb_pooler": "mean"}, open(os.path.join(d, "config.json"), "w"))
    json.dump([{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
               {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
               {"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}],
              open(os.path.join(d, "modules.json"), "w"))
    json.dump({"word_embedding_dimension": 128, "pooling_mode_mean_tokens": True},
              open(os.path.join(d, "1_Pooling", "config.json"), "w"))
    json.dump({"max_seq_length": 8192, "do_lower_case": True}, open(os.path.join(d, "sentence_bert_config.json"), "w"))
    open(os.path.join(d, "vocab.txt"), "w", encoding="utf-8").write("\n".join(vocab) + "\n")
    w = ao.random_weights(shape, seed)
    state = {"bert." + k: np.ascontiguousarray(v) for k, v in w.items()}
    state["bert.pooler.dense.weight"] = np.zeros((128, 128), np.float32)
    state["bert.pooler.dense.bias"] = np.zeros(128, np.float32)
    state.update(extra or {})
    save_file(state, os.path.join(d, "model.safetensors"))
    return shape, w, vocab


@pytest.fixture
def jina(monkeypatch, tmp_path, gpu):
    from voitta_rag_amd import config, embedding, sparse_embedding, store_registry, vector_store

    def reset():
        config.get_settings.cache_clear()
        store_registry.reset()
        embedding._embedding_service = None
        sparse_embedding._sparse_embedding_service = None
        vector_store._vector_store = None

    def make(name, precision="f32", extra=None, **env):
        path = str(tmp_path / name)
        made = jina_checkpoint(path, extra=extra)
        for k, v in dict({"EMBEDDING_MODEL": path, "EMBEDDING_DIMENSION": "128", "VOITTA_ENCODER_PRECISION": precision,
                          "VOITTA_DEFERRED_INDEXING": "0"}, **env).items():
            monkeypatch.setenv(k, v)
        reset()
        return made

    yield make
    reset()


def test_services_embed_store_and_answer_text_questions(jina):
    import test_query_text_batch_gpu as qt
    from test_rope_gpu import _hf_seqs

    from voitta_rag_amd import embedding, sparse_embedding, vector_store
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd.vector_store import ChunkMetadata
    from voitta_rag_amd.wordpiece import WordPieceTokenizer

    shape, w, vocab = jina("jina-embeddings-v2-tiny")
    emb, sp, vs = (embedding.get_embedding_service(), sparse_embedding.get_sparse_embedding_service(),
                   vector_store.get_vector_store())
    model = emb.model
    assert isinstance(model.tokenizer, WordPieceTokenizer) and embedding.one_call_text_paths(model)
    assert model.max_seq_length == 512 and model.desc.max_pos == 512  # 8192 declared, capped
    assert (model.desc.position, model.desc.ffn) == ("none", "geglu")
    assert np.array_equal(model.desc.attention_slopes, enc.alibi_slopes(2))
    rng = np.random.default_rng(3)
    texts = [" ".join(rng.choice(qt.WORDS, size=int(n))) for n in (3, 40, 9, 150, 1, 25, 12, 60)] + [" ".join(["memory bandwidth"] * 400)]
    seqs = _hf_seqs(vocab, texts)
    assert max(len(s) for s in seqs) == 512
    vectors = emb.embed_texts(texts)
    _check(np.asarray(vectors, np.float64), ao.sentence_embeddings(w, shape, seqs, enc.alibi_slopes(2)), "f32", "embed_texts")
    # search_questions through the vector store
    metas = [ChunkMetadata(file_path="d/a.md", folder_path="d", index_folder="d", file_name="a.md", chunk_index=i,
                           total_chunks=len(texts), start_char=0, end_char=1, indexed_at="t",
                           source_modified_at=1_700_000_000 + i) for i in range(len(texts))]
    vs.store_chunks(list(zip(texts, vectors, metas)), sparse_vectors=sp.embed_texts(texts))
    got = vs.search_questions([{"query": texts[1], "limit": 3}, {"query": texts[5], "limit": 2}])
    assert [len(g) for g in got] == [3, 2]
    assert got[0][0].metadata.chunk_index == 1 and got[1][0].metadata.chunk_index == 5
    # a question as text in one call: the rows of encode-then-search (rows put into the engine directly: after the
    # vector store's last write, whose row table they are no part of)
    e = model.engine
    qt._store(e, model, np.random.default_rng(4))
    questions = [texts[1], "dense retrieval?", texts[8]]
    limits, weights = np.full(3, 10, np.int32), np.full(3, 0.1)
    res, qemb = e.query_text_batch(model.tokenizer, questions, questions, model.max_seq_length, limits, weights, [None] * 3,
                                   embeddings=True)
    assert np.array_equal(qemb, enc.encode(e, *_pack(_hf_seqs(vocab, questions))))
    want = qt.expected(e, qemb, questions, limits, weights, [None] * 3, 0)
    assert all(qt.same(res[i], want[i]) for i in range(3))
    one = e.query_text(model.tokenizer, questions[0], questions[0], model.max_seq_length, 10, 0.1, 0, None)
    assert qt.same(one, want[0])


def test_late_chunking_with_the_cap_raised(jina):
    """VOITTA_LATE_CHUNKING=1 and sequences of up to 2048 tokens: a document of about 1500 tokens is one sequence, and
    every chunk's row is the oracle's mean over its span — with a bias that reaches across the whole document."""
    from test_late_chunking_gpu import document

    from voitta_rag_amd import embedding
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd import late_chunking as lc
    from voitta_rag_amd.chunking import get_chunking_service

    shape, w, _ = jina("jina-late", precision="f16", VOITTA_LATE_CHUNKING="1", VOITTA_MAX_SEQ_LENGTH="2048")
    emb = embedding.get_embedding_service()
    model = emb.model
    assert model.max_seq_length == 2048 and model.desc.max_pos == 2048
    doc = document(np.random.default_rng(15), 1100)
    chunks = [str(c.text) for c in get_chunking_service().chunk_text(doc)]
    plan = lc.plan(doc, chunks, model.tokenize, 2048, 256)
    assert plan.n_seq == 1 and 1000 <= int(plan.offsets[-1]) <= 2048 and not plan.truncated.any()
    got = np.asarray(emb.embed_document(doc, chunks), np.float32)
    hidden = ao.encode_one(w, shape, plan.ids, enc.alibi_slopes(2))
    want = np.stack([ao.pool(hidden[b:e], "mean") for b, e in plan.span_tok.tolist()])
    _check(got.astype(np.float64), want, "f16", f"{len(chunks)} chunks of a {int(plan.offsets[-1])}-token document")


def test_the_qk_layernorm_variant_is_refused_by_the_service(jina):
    from voitta_rag_amd import embedding

    jina("jina-embeddings-v2-base-code-tiny", extra={
        "bert.encoder.layer.0.attention.self.layer_norm_q.weight": np.ones(128, np.float32),
        "bert.encoder.layer.0.attention.self.layer_norm_q.bias": np.zeros(128, np.float32)})
    with pytest.raises(ValueError, match=r"layer_norm_q\.bias.*layer_norm_q\.weight.*LayerNorms on Q and K"):
        embedding.get_embedding_service().model
