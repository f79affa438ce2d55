"""Pre-norm, sliding-window encoders (model_type modernbert) on the GPU: the transformers goldens at every precision (the
batch, then the first and last sequence alone and again from the cached graph), one batch per GEMM route against the f64
oracle with both poolings, the same batches with VR_ENCODE_FUSE=0 in a fresh child process, window = 0 and
rope_theta_local = 0, vr_encode_spans, the refused descriptions, and the services on a synthetic checkpoint directory with
a byte-level BPE tokenizer.json.

The lengths of the goldens are the ones at which the windowed kernels can go wrong: the window's edge and one past it,
2w + 1 and 2w + 2, tile edges, 193 and 257 tokens (a block's later query tiles meet a key tile they see nothing of
before any they do see), and one token past what the staged kernel holds in LDS for each head size."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import modernbert_oracle as mo
from test_encoder_gpu import TOL
from test_modernbert_cpu import load_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "modernbert_*.npz")))


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


def _engine(shape, pooling, precision, w, **over):
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    e = Engine(shape.hidden)
    enc.load_encoder(e, mo.desc_for(shape, pooling, precision, **over), w)
    return e


# ---- 1. goldens at every precision -----------------------------------------------------------------------------------
def test_goldens_exist():
    assert len(GOLDEN) == 4


@pytest.mark.parametrize("precision", list(TOL))
@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p))
def test_encoder_matches_transformers_golden(gpu, path, precision):
    from voitta_rag_amd import encoder as enc

    g, shape, pooling, seed, _, want = load_case(path)
    e = _engine(shape, pooling, precision, mo.random_weights(shape, seed))
    _check(enc.encode(e, g["ids"], g["offsets"]).astype(np.float64), want, precision, os.path.basename(path))
    # the first and the last sequence alone, twice each: the second run replays the cached graph where one is cached
    for i in (0, len(g["offsets"]) - 2):
        a, b = g["offsets"][i], g["offsets"][i + 1]
        runs = [enc.encode(e, g["ids"][a:b], np.array([0, b - a], np.int32)) for _ in range(2)]
        _check(runs[0].astype(np.float64), want[i:i + 1], precision, f"sequence {i} alone")
        assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)), i
    e.close()


# ---- 2. one batch per GEMM route ---------------------------------------------------------------------------------------
PATH_SHAPE = mo.ModernShape(3, 128, 2, 256, vocab=300, max_pos=512, window=8)
# as test_rope_gpu.PATH_LENS: <= 64 tokens (skinny, one block), 65..256 (skinny, several blocks), 300..1000 (the mid
# kernel), more than 16384 (ping-pong)
PATH_LENS = {
    "skinny1": [1, 2, 17, 31],
    "skinny4": [64, 65, 15, 16, 63],
    "mid": [129, 300, 1, 200, 77],
    "pingpong": [512, 511, 257, 300, 480, 333, 1, 64] * 7,
}


def path_batches():
    w = mo.random_weights(PATH_SHAPE, 51)
    rng = np.random.default_rng(52)
    batches = {}
    for name, lens in PATH_LENS.items():
        seqs = [rng.integers(0, PATH_SHAPE.vocab, size=n).astype(np.int32) for n in lens[:8]]
        batches[name] = (seqs * (len(lens) // len(seqs) + 1))[:len(lens)]
    return w, batches


@pytest.fixture(scope="module")
def path_refs():
    """Per batch: the sequences, the f64 oracle's final hidden states of each distinct one, and its embeddings for both
    poolings (computed once, shared, read-only)."""
    w, batches = path_batches()
    refs, hidden = {}, {}
    for name, seqs in batches.items():
        want = {"mean": [], "cls": []}
        for s in seqs:
            key = s.tobytes()
            if key not in hidden:
                hidden[key] = mo.encode_one(w, PATH_SHAPE, s)
                hidden[key].setflags(write=False)
            for pooling in want:
                want[pooling].append(mo.pool(hidden[key], pooling))
        refs[name] = (seqs, {k: np.stack(v) for k, v in want.items()}, [hidden[s.tobytes()] for s in seqs])
        for v in refs[name][1].values():
            v.setflags(write=False)
    return w, refs


def test_path_batches_have_the_sizes_that_pick_each_route():
    t = {k: sum(v) for k, v in PATH_LENS.items()}
    assert t["skinny1"] <= 64 and 65 <= t["skinny4"] <= 256 and 300 <= t["mid"] <= 1000 and t["pingpong"] > 16384


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


def test_a_question_takes_the_folded_layernorm_projections(gpu):
    """At most 16 rows at H = 384 in f16: every projection computes its LayerNorm itself (launch_skinny_ln), which the
    H = 128 shapes above never reach. Alone, twice (the second run is the cached graph's), and 17 tokens, one past it."""
    from voitta_rag_amd import encoder as enc

    shape = mo.ModernShape(3, 384, 6, 768, vocab=300, max_pos=512, window=4)
    w = mo.random_weights(shape, 71)
    rng = np.random.default_rng(72)
    e = _engine(shape, "mean", "f16", w)
    for n in (1, 9, 16, 17):
        s = rng.integers(0, shape.vocab, size=n).astype(np.int32)
        runs = [enc.encode(e, *_pack([s])) for _ in range(3)]
        _check(runs[0].astype(np.float64), mo.sentence_embeddings(w, shape, [s]), "f16", f"{n} tokens")
        assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2]), n
    e.close()


def offset_logits_model(c):
    """The w = 8 route shape with every logit moved down by 2 c^2: in every head the 16 lowest-frequency rotary pairs of
    the query carry +c and of the key -c (a Wqkv bias; those weight rows are zero). Both bases are 160000, so a pair
    turns by at most 8 * 160000^-0.5 = 0.02 rad between a query and a key it sees in a windowed layer, and their term is
    -16 c^2 cos(<= 0.02) / sqrt(64) = -2 c^2 to 2e-4 for every such pair of positions."""
    shape = mo.ModernShape(3, 128, 2, 256, vocab=300, max_pos=512, window=8, theta_local=160000.0)
    w = mo.random_weights(shape, 81)
    H, dh = shape.hidden, shape.hidden // shape.heads
    for i in range(shape.layers):
        name = mo.layer_keys(i, shape.layers)["qkv_w"]
        bias = np.zeros(3 * H, np.float32)
        for head in range(shape.heads):
            f = np.arange(head * dh + dh // 2 - 16, head * dh + dh // 2)
            w[name][np.concatenate([f, H + f])] = 0.0
            bias[f], bias[H + f] = c, -c
        w[name[:-6] + "bias"] = bias
    return shape, w


@pytest.mark.parametrize("precision", list(TOL))
def test_logits_far_below_zero_keep_their_rows(gpu, precision):
    """A softmax does not care where its logits lie; a running maximum floored at 0 does. With w = 8, queries 73..79 of
    a staged sequence meet key tile 0..63 first and see nothing of it, as do queries 136.. of a streamed block against
    its first tile and every query past 72 in the f32 kernel: those rows need the maximum of the first tile they DO see.
    f32 and f16x3 (the f32 kernel): logits near -128, where exp underflows to 0 in f32. f16: logits near -32, where P is
    0 in f16 and exp is not in f32 (a row of zeros, not a NaN). The offset is smaller there because it costs accuracy
    in any f16-operand engine: the f64 oracle with nothing but the products' operands rounded to f16
    (encode_one(operand=f16_operand)) is 1.5e-4 max-abs from the exact one at c = 4 on the 512-token sequence below,
    4.4e-4 with the same -32 from one feature of 16, and 5e-5 without an offset; TOL["f16"] allows 5e-4. The bars are
    the table's in every precision."""
    from voitta_rag_amd import encoder as enc

    shape, w = offset_logits_model(4.0 if precision == "f16" else 8.0)
    rng = np.random.default_rng(82)
    seqs = [rng.integers(0, shape.vocab, size=n).astype(np.int32) for n in (129, 193)]
    long = [rng.integers(0, shape.vocab, size=512).astype(np.int32)]  # (from 384 tokens on the windowed layers stream)
    e = _engine(shape, "mean", precision, w)
    for batch, what in ((seqs, "129 + 193 tokens"), (long, "512 tokens")):
        _check(enc.encode(e, *_pack(batch)).astype(np.float64), mo.sentence_embeddings(w, shape, batch), precision,
               "offset logits, " + what)
    e.close()


# ---- 3. separate passes (VR_ENCODE_FUSE=0) -------------------------------------------------------------------------------
def encode_path_batches(out_path=None):
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


def test_unfused_passes_in_a_child_process(gpu, path_refs, tmp_path):
    """VR_ENCODE_FUSE is read when a model is loaded: the same batches, loaded and run in a fresh child process with
    the rotation and the gate as passes of their own, against the same oracle rows. f32 never fuses: bit-identical to
    this process's run; the skinny f16 batches differ (one f16 rounding of Q, K and the gate's product more)."""
    out_path = str(tmp_path / "unfused.npz")
    env = dict(os.environ, VR_ENCODE_FUSE="0")
    code = (f"import sys; sys.path[:0] = {[os.path.dirname(HERE), HERE]!r}; import test_modernbert_gpu as t; "
            f"t.encode_path_batches({out_path!r})")
    subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=120)
    unfused = np.load(out_path)
    fused = encode_path_batches()
    _, refs = path_refs
    assert sorted(unfused.files) == sorted(fused)
    for key, got in fused.items():
        batch, precision, pooling = key.split()
        _check(unfused[key].astype(np.float64), refs[batch][1][pooling], precision, "unfused " + key)
        if precision == "f32":
            assert np.array_equal(got, unfused[key]), key
        elif batch.startswith("skinny"):
            assert not np.array_equal(got, unfused[key]), key  # the child really ran another form


# ---- 4. window = 0, rope_theta_local = 0 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16", "f32"])
def test_no_window_is_the_all_global_model_and_no_local_theta_is_theta(gpu, path_refs, precision):
    from dataclasses import replace

    from voitta_rag_amd import encoder as enc

    w, refs = path_refs
    seqs = refs["mid"][0] + refs["skinny1"][0]
    ids, off = _pack(seqs)
    e = _engine(PATH_SHAPE, "mean", precision, w, window=0, global_every=0, rope_theta_local=0.0)
    want = mo.sentence_embeddings(w, replace(PATH_SHAPE, window=0), seqs, "mean")
    got = enc.encode(e, ids, off)
    _check(got.astype(np.float64), want, precision, "window 0")
    assert np.max(np.abs(want - np.concatenate([refs["mid"][1]["mean"], refs["skinny1"][1]["mean"]]))) > 1e-3  # another model
    e.close()
    same = replace(PATH_SHAPE, theta_local=PATH_SHAPE.theta)
    a = _engine(PATH_SHAPE, "mean", precision, w, rope_theta_local=0.0)
    b = _engine(same, "mean", precision, w)
    ga, gb = enc.encode(a, ids, off), enc.encode(b, ids, off)
    assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32))
    _check(ga.astype(np.float64), mo.sentence_embeddings(w, same, seqs, "mean"), precision, "rope_theta_local 0")
    a.close()
    b.close()


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
    want = np.stack([mo.pool(hidden[i][a:b], "mean") for i, s in enumerate(spans) for a, b in s])
    e = _engine(PATH_SHAPE, "cls", precision, w)  # (the description's pooling is ignored by a span call)
    ids, off = _pack(seqs)
    _check(enc.encode_spans(e, ids, off, span_off, span_tok).astype(np.float64), want, precision, "spans")
    e.close()


# ---- 6. refused descriptions ---------------------------------------------------------------------------------------------
def test_refused_descriptions_name_the_field_and_leave_the_loaded_encoder_working(gpu, path_refs):
    import rerank_oracle as rr
    from oracle import bert as obert

    from voitta_rag_amd import encoder as enc

    w, refs = path_refs
    seqs, want, _ = refs["skinny4"]
    ids, off = _pack(seqs)
    e = _engine(PATH_SHAPE, "mean", "f32", w)
    before = enc.encode(e, ids, off)
    _check(before.astype(np.float64), want["mean"], "f32", "before")
    bert_shape = obert.BertShape(3, 128, 2, 256, vocab=300, max_pos=512)
    bert_w = obert.random_weights(bert_shape, 2)
    base = dict(vocab=300, max_pos=512, pooling="mean", precision="f32")
    refused = [
        # pre-norm without rotary positions / without a gated FFN; a window without rotary positions
        (enc.BertDesc(3, 128, 2, 256, **base, norm="pre"), bert_w, "norm VR_NORM_PRE needs position VR_POS_ROTARY"),
        (enc.BertDesc(3, 128, 2, 256, **base, norm="pre", position="rotary", rope_theta=1e4), bert_w,
         "norm VR_NORM_PRE needs a gated ffn"),
        (enc.BertDesc(3, 128, 2, 256, **base, window=8, global_every=3), bert_w, "window 8 needs position VR_POS_ROTARY"),
    ]
    # a window in a post-norm rotary, gated model (the nomic family's tensors)
    import rope_oracle as ro

    rope_shape = ro.RopeShape(3, 128, 2, 256, vocab=300, max_pos=512, act="gelu")
    with pytest.raises(Exception, match="window 8 needs norm VR_NORM_PRE"):
        enc.load_encoder(e, mo.desc_for(PATH_SHAPE, "mean", "f32", norm="post", type_vocab=2), ro.random_weights(rope_shape, 3))
    assert np.array_equal(enc.encode(e, ids, off), before)
    for desc, weights, message in refused:
        names = enc.tensor_names(desc.layers)
        with pytest.raises(Exception, match=message):
            enc._load(e, desc, weights, names, e._lib.vr_encoder_load)
        assert np.array_equal(enc.encode(e, ids, off), before), message
    for over, message in ((dict(window=8, global_every=0), "global_every 0"), (dict(window=5000), "window 5000"),
                          (dict(rope_theta_local=-1.0), "rope_theta_local")):
        with pytest.raises(Exception, match=message):
            enc.load_encoder(e, mo.desc_for(PATH_SHAPE, "mean", "f32", **over), w)
        assert np.array_equal(enc.encode(e, ids, off), before), message
    # a reranker takes neither, and a loaded reranker stays as it is
    rshape = obert.BertShape(2, 128, 4, 256, vocab=200, max_pos=64)
    rw = rr.random_weights(rshape, 8)
    rbase = dict(vocab=200, max_pos=64, pooling="cls", normalize=False, precision="f32")
    enc.load_reranker(e, enc.BertDesc(2, 128, 4, 256, **rbase), rw)
    rng = np.random.default_rng(1)
    rids, roff = _pack([rng.integers(0, 200, size=n).astype(np.int32) for n in (9, 30)])
    seg = np.array([4, 11], np.int32)
    scores = e.rerank(rids, roff, seg)
    for extra in (dict(norm="pre"), dict(window=8, global_every=3)):
        with pytest.raises(Exception, match="a reranker with norm . or window . is not supported"):
            enc.load_reranker(e, enc.BertDesc(2, 128, 4, 256, **rbase, **extra), rw)
        assert np.array_equal(e.rerank(rids, roff, seg), scores)
    assert np.array_equal(enc.encode(e, ids, off), before)
    e.close()


# ---- 7. services ---------------------------------------------------------------------------------------------------------
WORDS = ("vector database index hybrid fusion ranking sparse dense retrieval kernel memory bandwidth wavefront encoder "
         "attention window rotary position layer norm residual gate token chunk document search query score filter").split()


def modernbert_checkpoint(d, layers=3, hidden=128, heads=2, inter=256, seed=61):
    """A ModernBERT-shaped sentence-transformers directory: config.json in transformers 5's spelling, mean pooling,
    Normalize, seeded weights, and a byte-level BPE tokenizer.json trained here on a few words."""
    from safetensors.numpy import save_file
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, processors, trainers

    os.makedirs(os.path.join(d, "1_Pooling"), exist_ok=True)
    tok = Tokenizer(models.BPE(unk_token=None))
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    trainer = trainers.BpeTrainer(vocab_size=400, special_tokens=["[PAD]", "[CLS]", "[SEP]"], show_progress=False,
                                  initial_alphabet=pre_tokenizers.ByteLevel.alphabet())
    rng = np.random.default_rng(seed)
    tok.train_from_iterator([" ".join(rng.choice(WORDS, size=12)) + "." for _ in range(200)], trainer)
    tok.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", special_tokens=[("[CLS]", 1), ("[SEP]", 2)])
    tok.save(os.path.join(d, "tokenizer.json"))
    vocab = -(-tok.get_vocab_size() // 8) * 8
    shape = mo.ModernShape(layers, hidden, heads, inter, vocab=vocab, max_pos=8192, window=8)
    json.dump({"architectures": ["ModernBertModel"], "model_type": "modernbert", "hidden_size": hidden,
               "num_hidden_layers": layers, "num_attention_heads": heads, "intermediate_size": inter, "vocab_size": vocab,
               "max_position_embeddings": 8192, "norm_eps": shape.eps, "hidden_activation": "gelu", "local_attention": 16,
               "global_attn_every_n_layers": 3,
               "layer_types": ["full_attention" if i % 3 == 0 else "sliding_attention" for i in range(layers)],
               "rope_parameters": {"full_attention": {"rope_type": "default", "rope_theta": shape.theta},
                                   "sliding_attention": {"rope_type": "default", "rope_theta": shape.theta_local}}},
              open(os.path.join(d, "config.json"), "w"))
    json.dump([{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
               {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
               {"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}],
              open(os.path.join(d, "modules.json"), "w"))
    json.dump({"word_embedding_dimension": hidden, "pooling_mode_mean_tokens": True},
              open(os.path.join(d, "1_Pooling", "config.json"), "w"))
    json.dump({"max_seq_length": 8192}, open(os.path.join(d, "sentence_bert_config.json"), "w"))
    w = mo.random_weights(shape, seed)
    save_file({"model." + k: np.ascontiguousarray(v) for k, v in w.items()}, os.path.join(d, "model.safetensors"))
    return shape, w, tok


@pytest.fixture
def services(monkeypatch, tmp_path, gpu):
    pytest.importorskip("tokenizers")
    from voitta_rag_amd import config, embedding, sparse_embedding, store_registry, vector_store

    def reset():
        config.get_settings.cache_clear()
        store_registry.reset()
        embedding._embedding_service = None
        sparse_embedding._sparse_embedding_service = None
        vector_store._vector_store = None

    def make(name, late=False, cap=512, precision="f32"):
        path = str(tmp_path / name)
        made = modernbert_checkpoint(path)
        for k, v in (("EMBEDDING_MODEL", path), ("EMBEDDING_DIMENSION", "128"), ("VOITTA_ENCODER_PRECISION", precision),
                     ("VOITTA_MAX_SEQ_LENGTH", str(cap)), ("VOITTA_LATE_CHUNKING", "1" if late else "0")):
            monkeypatch.setenv(k, v)
        reset()
        return made

    yield make
    reset()


def test_services_embed_store_and_find_with_a_bpe_tokenizer(services):
    from voitta_rag_amd import deferred, embedding, sparse_embedding, vector_store
    from voitta_rag_amd.vector_store import ChunkMetadata

    shape, w, tok = services("modernbert-embed")
    emb, sp, vs = (embedding.get_embedding_service(), sparse_embedding.get_sparse_embedding_service(),
                   vector_store.get_vector_store())
    model = emb.model
    assert not embedding.native_tokenizer(model.tokenizer) and not embedding.one_call_text_paths(model)
    assert model.max_seq_length == 512 and model.desc.max_pos == 512  # 8192 declared, capped
    assert (model.desc.norm, model.desc.window, model.desc.global_every) == ("pre", 8, 3)
    rng = np.random.default_rng(3)
    texts = [" ".join(rng.choice(WORDS, size=int(n))) for n in (3, 40, 9, 150, 1, 25, 12, 60)] + [" ".join(["memory bandwidth"] * 700)]
    tok.enable_truncation(max_length=512)
    seqs = [np.asarray(e.ids, np.int32) for e in tok.encode_batch(texts)]
    assert max(len(s) for s in seqs) == 512 and all(s[0] == 1 and s[-1] == 2 for s in seqs)
    vectors = emb.embed_texts(texts)
    _check(np.asarray(vectors, np.float64), mo.sentence_embeddings(w, shape, seqs), "f32", "embed_texts")
    q = emb.embed_query(texts[1])
    assert not isinstance(q, deferred.QueryRef)  # no one-call text path without a native tokenizer
    _check(np.asarray(q, np.float64)[None], mo.sentence_embeddings(w, shape, seqs[1:2]), "f32", "embed_query")
    metas = [ChunkMetadata(file_path="d/a.md", folder_path="d", index_folder="d", file_name="a.md", chunk_index=i,
                           total_chunks=len(texts), start_char=0, end_char=1, indexed_at="t",
                           source_modified_at=1_700_000_000 + i) for i in range(len(texts))]
    vs.store_chunks(list(zip(texts, vectors, metas)), sparse_vectors=sp.embed_texts(texts))
    got = vs.search(q, limit=3, sparse_query=sp.embed_query(texts[1]))
    assert len(got) == 3 and got[0].metadata.chunk_index == 1


def test_late_chunking_indexes_a_document_with_it(services):
    from voitta_rag_amd import embedding, vector_store
    from voitta_rag_amd import late_chunking as lc
    from voitta_rag_amd.chunking import get_chunking_service
    from voitta_rag_amd.indexer import BulkIndexer, ParsedFile

    shape, w, tok = services("modernbert-late", late=True, cap=2048)
    emb, vs, chunker = embedding.get_embedding_service(), vector_store.get_vector_store(), get_chunking_service()
    model = emb.model
    assert model.max_seq_length == 2048
    rng = np.random.default_rng(4)
    doc = "\n\n".join(" ".join(" ".join(rng.choice(WORDS, size=int(rng.integers(5, 14)))) + "." for _ in range(6))
                      for _ in range(10))
    chunks = [c.text for c in chunker.chunk_texts([doc])[0]]
    assert len(chunks) > 3 and all(type(t) is lc.LateChunkText for t in chunks)
    plan = lc.plan(doc, chunks, model.tokenize, 2048, 256)
    assert plan.n_seq == 1 and 300 < int(plan.offsets[-1]) <= 2048 and not plan.truncated.any()
    rows = np.asarray(emb.embed_document(doc, [str(t) for t in chunks]), np.float64)
    h = mo.encode_one(w, shape, plan.ids)
    want = np.stack([mo.pool(h[a:b], "mean") for a, b in plan.span_tok])
    _check(rows, want, "f32", "late-chunked rows")
    counts = BulkIndexer().index_files(iter([ParsedFile(content=doc, file_path="docs/0.md", folder_path="docs",
                                                        index_folder="docs", file_name="0.md",
                                                        source_modified_at=1_710_000_000)]))
    assert counts == {"docs/0.md": len(chunks)}
    stored = vs.client.get_dense(np.arange(len(chunks))).astype(np.float64)
    _check(stored, want, "f32", "stored late-chunked rows")
