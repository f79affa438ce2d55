"""MPNet encoders (model_type mpnet) on the GPU: the relative-position attention bias in all three attention kernels.
The transformers goldens at every precision (the batch, then the first and last sequence alone and again from the cached
graph); a synthetic radius-8 table of independent entries through Engine.set_attention_bias on one batch per GEMM route
with both poolings, and once more with VR_ENCODE_FUSE=0 in a fresh child process; the streamed kernel past what the
staged one holds, and the edge between them that the table's bytes move; setting and removing the bias against engines
that never knew the other state; vr_encode_spans; the refusals; and the services on a synthetic checkpoint directory with
the golden tokenizer.json."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mpnet_oracle as mp
from test_encoder_gpu import TOL
from test_modernbert_gpu import PATH_LENS
from test_mpnet_cpu import TOKENIZER, load_case, synthetic_table

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "mpnet_tiny_*.npz")))


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


def _engine(shape, pooling, precision, w, table="buckets", **over):
    """An engine with the model loaded. table: "buckets" — the model's own bias, as a checkpoint directory loads it (the
    description carries mpnet_bias_table's table); an array — that table; None — no bias."""
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    e = Engine(shape.hidden)
    desc = mp.desc_for(shape, pooling, precision, **over)
    state, own = enc.mpnet_slots(w, desc)
    desc.attention_bias = own if isinstance(table, str) else table
    enc.load_encoder(e, desc, state)
    return e


# ---- 1. goldens at every precision -----------------------------------------------------------------------------------
def test_goldens_exist():
    assert len(GOLDEN) == 2


@pytest.mark.parametrize("precision", list(TOL))
@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p))
def test_encoder_matches_transformers_golden(gpu, path, precision):
    from voitta_rag_amd import encoder as enc

    g, shape, pooling, seed, _, want = load_case(path)
    e = _engine(shape, pooling, precision, mp.random_weights(shape, seed))
    _check(enc.encode(e, g["ids"], g["offsets"]).astype(np.float64), want, precision, os.path.basename(path))
    # the first and the last sequence alone, twice each: the second run replays the cached graph where one is cached
    for i in (0, len(g["offsets"]) - 2):
        a, b = g["offsets"][i], g["offsets"][i + 1]
        runs = [enc.encode(e, g["ids"][a:b], np.array([0, b - a], np.int32)) for _ in range(2)]
        _check(runs[0].astype(np.float64), want[i:i + 1], precision, f"sequence {i} alone")
        assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)), i
    e.close()


# ---- 2. a synthetic table on one batch per GEMM route --------------------------------------------------------------------
PATH_SHAPE = mp.MpnetShape(3, 128, 2, 256)
PATH_TABLE = synthetic_table(PATH_SHAPE.heads)  # radius 8, independent N(0, 1) entries


def path_batches():
    w = mp.random_weights(PATH_SHAPE, 51)
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
                hidden[key] = mp.encode_one(w, PATH_SHAPE, s, PATH_TABLE)
                hidden[key].setflags(write=False)
            for pooling in want:
                want[pooling].append(mp.pool(hidden[key], pooling))
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
    e = _engine(PATH_SHAPE, pooling, precision, w, table=None)
    e.set_attention_bias(PATH_TABLE)
    _check(enc.encode(e, *_pack(seqs)).astype(np.float64), want[pooling], precision, f"{batch} {pooling}")
    e.close()


def encode_path_batches(out_path=None):
    from voitta_rag_amd import encoder as enc

    w, batches = path_batches()
    out = {}
    for precision in ("f16", "f32"):
        for pooling in ("mean", "cls"):
            e = _engine(PATH_SHAPE, pooling, precision, w, table=PATH_TABLE)
            for name, seqs in batches.items():
                out[f"{name} {precision} {pooling}"] = enc.encode(e, *_pack(seqs))
            e.close()
    if out_path:
        np.savez(out_path, **out)
    return out


def test_unfused_passes_in_a_child_process(gpu, path_refs, tmp_path):
    """VR_ENCODE_FUSE is read when a model is loaded: the same batches, loaded and run in a fresh child process with it
    off, against the same oracle rows."""
    out_path = str(tmp_path / "unfused.npz")
    env = dict(os.environ, VR_ENCODE_FUSE="0")
    code = (f"import sys; sys.path[:0] = {[os.path.dirname(HERE), HERE]!r}; import test_mpnet_gpu as t; "
            f"t.encode_path_batches({out_path!r})")
    subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=120)
    unfused = np.load(out_path)
    _, refs = path_refs
    assert len(unfused.files) == 4 * len(PATH_LENS)
    for key in unfused.files:
        batch, precision, pooling = key.split()
        _check(unfused[key].astype(np.float64), refs[batch][1][pooling], precision, "unfused " + key)


# ---- 3. the streamed kernel, and the edge the table's bytes move ---------------------------------------------------------
LONG_POSITIONS = 1538  # max_pos 1536


@pytest.fixture(scope="module")
def long_models():
    out = {}
    for dh, heads, seed in ((64, 2, 61), (32, 4, 62)):
        shape = mp.MpnetShape(2, 128, heads, 256, positions=LONG_POSITIONS)
        out[dh] = (shape, mp.random_weights(shape, seed))
    return out


@pytest.mark.parametrize("dh,n", [(64, 1100), (32, 1400)])
def test_streamed_kernel_with_the_models_bias(gpu, long_models, dh, n):
    """Past what the staged kernel holds (640 keys at d_h = 64, 1280 at 32): the keys stream in 64-row tiles, most of
    them a constant bias away from the query (|j - i| >= 128). One sequence, a call of its own, radius 128, f16."""
    from voitta_rag_amd import encoder as enc

    shape, w = long_models[dh]
    assert shape.hidden // shape.heads == dh and shape.max_pos == 1536
    s = np.random.default_rng(n).integers(4, shape.vocab, size=n).astype(np.int32)
    e = _engine(shape, "mean", "f16", w)
    _check(enc.encode(e, *_pack([s])).astype(np.float64), mp.sentence_embeddings(w, shape, [s]), "f16", f"{n} tokens")
    e.close()


def test_staged_kernel_at_its_largest_and_the_first_length_the_table_pushes_out(gpu, long_models):
    """d_h = 64: 640 staged keys fill the LDS a workgroup may have, so with the table's 1028 bytes behind them a
    625..640-token sequence streams (without a bias it stages), and 624 tokens are the most the biased staged kernel
    holds — above the 64 KiB default, the size hipFuncSetAttribute has to be told with the table counted."""
    from voitta_rag_amd import encoder as enc

    shape, w = long_models[64]
    rng = np.random.default_rng(9)
    e = _engine(shape, "mean", "f16", w)
    for n in (624, 640):
        s = rng.integers(4, shape.vocab, size=n).astype(np.int32)
        _check(enc.encode(e, *_pack([s])).astype(np.float64), mp.sentence_embeddings(w, shape, [s]), "f16", f"{n} tokens")
    e.close()


# ---- 4. setting and removing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_removed_bias_is_the_engine_that_never_had_one_and_back(gpu, path_refs, precision):
    """One short sequence (its forward pass is captured and replayed as a graph) and one batch, each run twice in every
    state: a graph that survived a change would replay the other state's kernels and table."""
    from voitta_rag_amd import encoder as enc

    w, refs = path_refs
    one = _pack(refs["skinny1"][0][2:3])
    batch = _pack(refs["mid"][0])

    def runs(e):
        return [enc.encode(e, *x).view(np.uint32) for x in (one, one, batch, batch)]

    never = _engine(PATH_SHAPE, "mean", precision, w, table=None)
    always = _engine(PATH_SHAPE, "mean", precision, w, table=PATH_TABLE)
    plain, biased = runs(never), runs(always)
    assert not np.array_equal(plain[0], biased[0]) and not np.array_equal(plain[2], biased[2])
    e = _engine(PATH_SHAPE, "mean", precision, w, table=PATH_TABLE)
    for state in (biased, plain, biased, plain):
        e.set_attention_bias(PATH_TABLE if state is biased else None)
        for got, want in zip(runs(e), state):
            assert np.array_equal(got, want)
    # vr_encoder_load resets it
    from voitta_rag_amd import encoder as enc2

    desc = mp.desc_for(PATH_SHAPE, "mean", precision)
    e.set_attention_bias(PATH_TABLE)
    enc2.load_encoder(e, desc, enc2.mpnet_slots(w, desc)[0])
    for got, want in zip(runs(e), plain):
        assert np.array_equal(got, want)
    for x in (never, always, e):
        x.close()


# ---- 5. spans ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_span_rows_are_the_oracles_span_means(gpu, path_refs, precision):
    from voitta_rag_amd import encoder as enc

    w, refs = path_refs
    seqs, _, hidden = refs["mid"]
    spans = [[(0, 129), (120, 129), (7, 8)], [(0, 10), (5, 300), (150, 290)], [(0, 1)], [], [(70, 77), (0, 77)]]
    span_off = np.zeros(len(seqs) + 1, np.int32)
    span_off[1:] = np.cumsum([len(s) for s in spans])
    span_tok = np.array([p for s in spans for p in s], np.int32)
    want = np.stack([mp.pool(hidden[i][a:b], "mean") for i, s in enumerate(spans) for a, b in s])
    e = _engine(PATH_SHAPE, "cls", precision, w, table=PATH_TABLE)  # (the description's pooling is ignored by a span call)
    ids, off = _pack(seqs)
    _check(enc.encode_spans(e, ids, off, span_off, span_tok).astype(np.float64), want, precision, "spans")
    e.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_loaded_encoder_unchanged(gpu, path_refs):
    import modernbert_oracle as mo
    import rope_oracle as ro

    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    w, refs = path_refs
    seqs, want, _ = refs["skinny4"]
    ids, off = _pack(seqs)
    e = _engine(PATH_SHAPE, "mean", "f32", w, table=PATH_TABLE)
    before = enc.encode(e, ids, off)
    _check(before.astype(np.float64), want["mean"], "f32", "before")
    rng = np.random.default_rng(1)
    for table, message in ((rng.normal(size=(3, 17)), "bias table of 3 heads for an encoder of 2"),
                           (rng.normal(size=(2, 1)), "radius 0 must lie in 1..512"),
                           (rng.normal(size=(2, 1027)), "radius 513 must lie in 1..512")):
        with pytest.raises(Exception, match=message):
            e.set_attention_bias(table.astype(np.float32))
        assert np.array_equal(enc.encode(e, ids, off), before), message
    with pytest.raises(ValueError, match="expected .heads, 2 . radius . 1."):
        e.set_attention_bias(np.zeros((2, 16), np.float32))
    e.set_attention_bias(np.zeros((2, 1025), np.float32))  # radius 512 is taken ...
    e.set_attention_bias(PATH_TABLE)
    assert np.array_equal(enc.encode(e, ids, off), before)  # ... and the table put back gives the same bits
    e.close()
    # a rotary description, and a pre-norm one: refused, and they run as they did
    rope_shape = ro.RopeShape(2, 128, 2, 256, vocab=300, max_pos=512, act="gelu")
    modern_shape = mo.ModernShape(2, 128, 2, 256, vocab=300, max_pos=512, window=8)
    for desc, weights in ((ro.desc_for(rope_shape, "mean", "f32"), ro.random_weights(rope_shape, 3)),
                          (mo.desc_for(modern_shape, "mean", "f32"), mo.random_weights(modern_shape, 4))):
        e = Engine(128)
        enc.load_encoder(e, desc, weights)
        before = enc.encode(e, ids, off)
        with pytest.raises(Exception, match="needs position VR_POS_LEARNED and norm VR_NORM_POST"):
            e.set_attention_bias(PATH_TABLE)
        e.set_attention_bias(None)  # nothing to remove: accepted
        assert np.array_equal(enc.encode(e, ids, off), before)
        e.close()
    e = Engine(128)
    for table in (PATH_TABLE, None):
        with pytest.raises(Exception, match="no encoder loaded"):
            e.set_attention_bias(table)
    e.close()


# ---- 7. services ---------------------------------------------------------------------------------------------------------
def mpnet_checkpoint(d, seed=71):
    """An MPNet-shaped sentence-transformers directory: config.json, mean pooling, Normalize, seeded weights under the
    `mpnet.`-less names sentence-transformers saves, and the golden tokenizer.json."""
    from safetensors.numpy import save_file

    os.makedirs(os.path.join(d, "1_Pooling"), exist_ok=True)
    spec = json.load(open(TOKENIZER, encoding="utf-8"))
    json.dump(spec, open(os.path.join(d, "tokenizer.json"), "w", encoding="utf-8"))
    vocab = -(-len(spec["model"]["vocab"]) // 8) * 8
    shape = mp.MpnetShape(3, 128, 2, 256, vocab=vocab)
    json.dump({"architectures": ["MPNetModel"], "model_type": "mpnet", "hidden_size": 128, "num_hidden_layers": 3,
               "num_attention_heads": 2, "intermediate_size": 256, "vocab_size": vocab, "max_position_embeddings": 514,
               "layer_norm_eps": shape.eps, "hidden_act": "gelu", "relative_attention_num_buckets": 32, "pad_token_id": 1,
               "bos_token_id": 0, "eos_token_id": 2}, open(os.path.join(d, "config.json"), "w"))
    json.dump([{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
               {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
               {"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}],
              open(os.path.join(d, "modules.json"), "w"))
    json.dump({"word_embedding_dimension": 128, "pooling_mode_mean_tokens": True},
              open(os.path.join(d, "1_Pooling", "config.json"), "w"))
    json.dump({"max_seq_length": 384}, open(os.path.join(d, "sentence_bert_config.json"), "w"))
    w = mp.random_weights(shape, seed)
    save_file({k: np.ascontiguousarray(v) for k, v in w.items()}, os.path.join(d, "model.safetensors"))
    return shape, w


def test_services_embed_store_and_answer_text_questions(gpu, tmp_path, monkeypatch):
    pytest.importorskip("tokenizers")
    from tokenizers import Tokenizer

    from voitta_rag_amd import config, embedding, sparse_embedding, store_registry, vector_store
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd.vector_store import ChunkMetadata

    path = str(tmp_path / "all-mpnet-tiny")
    shape, w = mpnet_checkpoint(path)
    for k, v in (("EMBEDDING_MODEL", path), ("EMBEDDING_DIMENSION", "128"), ("VOITTA_ENCODER_PRECISION", "f32")):
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
        assert embedding.native_tokenizer(model.tokenizer) and embedding.one_call_text_paths(model)
        assert model.tokenizer.specials == ("<s>", "</s>", "[UNK]")
        assert model.max_seq_length == 384 and model.desc.max_pos == 512 and model.desc.type_vocab == 1
        assert model.desc.attention_bias.shape == (2, 257)
        words = [t for t in json.load(open(TOKENIZER, encoding="utf-8"))["model"]["vocab"] if len(t) > 3 and t.isalpha()]
        rng = np.random.default_rng(3)
        texts = [" ".join(rng.choice(words, size=int(n))) for n in (3, 40, 9, 150, 1, 25, 12, 60)] + [" ".join(["memory bandwidth"] * 300)]
        hf = Tokenizer.from_file(TOKENIZER)
        hf.enable_truncation(max_length=384)
        seqs = [np.asarray(e.ids, np.int32) for e in hf.encode_batch(texts)]
        assert max(len(s) for s in seqs) == 384 and all(s[0] == 0 and s[-1] == 2 for s in seqs)
        ids, off = model.tokenize(texts)
        assert np.array_equal(ids, np.concatenate(seqs)) and np.array_equal(np.diff(off), [len(s) for s in seqs])
        vectors = emb.embed_texts(texts)
        assert np.array_equal(np.asarray(vectors, np.float32), enc.encode(model.engine, ids, off))  # tokenise-then-encode
        _check(np.asarray(vectors, np.float64), mp.sentence_embeddings(w, shape, seqs), "f32", "embed_texts")
        metas = [ChunkMetadata(file_path="d/a.md", folder_path="d", index_folder="d", file_name="a.md", chunk_index=i,
                               total_chunks=len(texts), start_char=0, end_char=1, indexed_at="t",
                               source_modified_at=1_700_000_000 + i) for i in range(len(texts))]
        vs.store_chunks(list(zip(texts, vectors, metas)), sparse_vectors=sp.embed_texts(texts))
        got = vs.search_questions([{"query": texts[1], "limit": 3}, {"query": texts[5], "limit": 2}])
        assert [len(g) for g in got] == [3, 2]
        assert got[0][0].metadata.chunk_index == 1 and got[1][0].metadata.chunk_index == 5
    finally:
        reset()
