"""ModernBERT cross-encoders, the parts that need no GPU: the f64 restatement of ModernBertForSequenceClassification
(tests/modernbert_rerank_oracle.py) against the transformers goldens, config.json reading and its refusals, the head's
tensors in their slots, and pair tokenisation through the tokenizers library."""
import glob
import json
import os

import numpy as np
import pytest

import modernbert_oracle as mo
import modernbert_rerank_oracle as mro

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "mbert_rerank_*.npz")))


def case(path):
    g = np.load(path)
    L, H, nh, inter, vocab, max_pos = (int(x) for x in g["shape"])
    shape = mo.ModernShape(L, H, nh, inter, vocab=vocab, max_pos=max_pos, eps=float(g["eps"]), theta=float(g["theta"]),
                           theta_local=float(g["theta_local"]), window=int(g["window"]), global_every=int(g["global_every"]))
    w = mro.random_weights(shape, int(g["seed"]), bool(g["biases"]), float(g["cls_scale"]), float(g["cls_bias"]))
    return g, shape, w, str(g["pooling"])


def test_the_goldens_cover_what_they_should():
    seen = {(str(g["pooling"]), bool(g["biases"]), int(g["window"])) for g in map(np.load, GOLDEN)}
    assert {p for p, _, _ in seen} == {"cls", "mean"} and {b for _, b, _ in seen} == {True, False}
    assert {w for _, _, w in seen} == {8, 64}
    for g in map(np.load, GOLDEN):
        assert list(np.diff(g["offsets"])) == [3, 16, 17, 129, 385, 705]
        assert g["logits"].min() <= -3 and g["logits"].max() >= 3
        assert int(g["window"]) == 8 or int(g["global_every"]) == 3


@pytest.mark.parametrize("path", GOLDEN, ids=os.path.basename)
def test_restated_head_equals_transformers(path):
    g, shape, w, pooling = case(path)
    assert ("head.dense.bias" in w) == ("head.norm.bias" in w) == bool(g["biases"])
    d = np.abs(mro.head(w, g["pooled"], shape.eps) - g["logits"]).max()
    print(f"{os.path.basename(path)}: head on transformers' pooled rows, max |d| {d:.3e}")
    assert d <= 1e-12


@pytest.mark.parametrize("path", GOLDEN, ids=os.path.basename)
def test_whole_oracle_against_transformers(path):
    """The oracle is f64 throughout with exact rotary tables; transformers' eager path rotates with f32 tables, rounds
    the rotated queries and keys' inputs and the softmax to f32 (modernbert_oracle's docstring). Those are relative
    roundings of 2^-24 = 6e-8 in values of order 1, on final-norm rows of order 1 that reach the logit through a head
    whose gain is the classifier's scale (at most 19 here): a few times 1e-7 on a logit is expected, and 1e-5 allows
    for 705 keys' worth of it without admitting any error in the model (the smallest structural mistake, one token's
    row or one bias, moves a logit by 1e-2 or more). The short pairs are enough: the rest is the GPU tier's."""
    g, shape, w, pooling = case(path)
    n = 4
    got = mro.logits(w, shape, g["ids"][: g["offsets"][n]], g["offsets"][: n + 1], pooling)
    d = np.abs(got - g["logits"][:n]).max()
    print(f"{os.path.basename(path)}: whole oracle, max |d| {d:.3e}")
    assert d <= 1e-5


# ---- config.json ---------------------------------------------------------------------------------------------------------
CFG = {"architectures": ["ModernBertForSequenceClassification"], "model_type": "modernbert", "hidden_size": 768,
       "num_hidden_layers": 22, "num_attention_heads": 12, "intermediate_size": 1152, "vocab_size": 50368,
       "max_position_embeddings": 8192, "norm_eps": 1e-5, "norm_bias": False, "hidden_activation": "gelu",
       "local_attention": 128, "global_attn_every_n_layers": 3, "global_rope_theta": 160000.0, "local_rope_theta": 10000.0,
       "classifier_pooling": "mean", "classifier_activation": "gelu", "classifier_bias": False,
       "id2label": {"0": "LABEL_0"}}


def _dir(tmp_path, cfg):
    d = tmp_path / "m"
    d.mkdir(exist_ok=True)
    json.dump(cfg, open(d / "config.json", "w"))
    return str(d)


def test_config_of_a_modernbert_cross_encoder_is_accepted(tmp_path):
    from voitta_rag_amd.reranker import read_cross_encoder_config

    cfg = read_cross_encoder_config(_dir(tmp_path, CFG))
    assert cfg["classifier_pooling"] == "mean"
    bare = {k: v for k, v in CFG.items() if k not in ("architectures", "classifier_pooling", "classifier_activation")}
    assert read_cross_encoder_config(_dir(tmp_path, bare))["model_type"] == "modernbert"  # the library's defaults
    # ... and the other families read as before
    bert = {"architectures": ["BertForSequenceClassification"], "model_type": "bert", "id2label": {"0": "LABEL_0"}}
    assert read_cross_encoder_config(_dir(tmp_path, bert))["model_type"] == "bert"
    with pytest.raises(ValueError, match="unsupported reranker"):
        read_cross_encoder_config(_dir(tmp_path, dict(bert, model_type="gpt2")))


@pytest.mark.parametrize("change,message", [
    ({"classifier_activation": "silu"}, "classifier_activation 'silu'"),
    ({"classifier_pooling": "max"}, "classifier_pooling 'max'"),
    ({"architectures": ["ModernBertForMaskedLM"]}, "ModernBertForSequenceClassification only"),
    ({"id2label": {"0": "a", "1": "b"}}, "2 labels"),
    ({"num_labels": 3}, "3 labels"),
])
def test_config_refusals(tmp_path, change, message):
    from voitta_rag_amd.reranker import read_cross_encoder_config

    with pytest.raises(ValueError, match=message):
        read_cross_encoder_config(_dir(tmp_path, dict(CFG, **change)))


# ---- the head's tensors ----------------------------------------------------------------------------------------------------
def test_head_tensors_land_in_their_slots():
    from voitta_rag_amd import encoder as enc

    shape = mo.ModernShape(3, 128, 2, 256, window=8)
    desc = mro.desc_for(shape, "mean", "f32")
    for biases in (True, False):
        w = mro.random_weights(shape, 5, biases, 3.0, 0.25)
        for prefix in ("", "model."):
            state = {(k if k.startswith(("head.", "classifier.")) else prefix + k): v for k, v in w.items()}
            head = enc.modernbert_head(state, desc)
            assert list(head) == enc.PRENORM_HEAD_NAMES
            for k in ("head.dense.weight", "head.norm.weight", "classifier.weight", "classifier.bias"):
                assert head[k] is w[k]
            for k in ("head.dense.bias", "head.norm.bias"):
                assert np.array_equal(head[k], w[k] if biases else np.zeros(128, np.float32))
            for name in enc.PRENORM_HEAD_NAMES:
                want = {"head.dense.weight": (128, 128), "classifier.weight": (1, 128), "classifier.bias": (1,)}.get(name, (128,))
                assert enc.expected_shape(desc, name) == want and tuple(head[name].shape) == want
    with pytest.raises(KeyError, match="classifier.weight"):
        enc.modernbert_head({k: v for k, v in w.items() if k != "classifier.weight"}, desc)


def test_load_reranker_hands_over_body_then_head(monkeypatch):
    """5 + 18 L body slots (modernbert_slots' names, NULL where the checkpoint has no bias) and the six head tensors."""
    from voitta_rag_amd import encoder as enc

    shape = mo.ModernShape(3, 128, 2, 256, window=8)
    seen = {}

    def fake_load(engine, desc, state, names, fn):
        seen.update(desc=desc, state=state, names=names, fn=fn)

    class Lib:
        vr_reranker_load = object()

    class Eng:
        _lib = Lib()

    monkeypatch.setattr(enc, "_load", fake_load)
    for pooling in ("cls", "mean"):
        w = mro.random_weights(shape, 5, False)
        e = Eng()
        enc.load_reranker(e, mro.desc_for(shape, pooling, "f16"), {"model." + k if not k.startswith(("head.", "classifier."))
                                                                   else k: v for k, v in w.items()})
        assert len(seen["names"]) == 5 + 18 * 3 + 6 and seen["names"][-6:] == enc.PRENORM_HEAD_NAMES
        assert seen["fn"] is Lib.vr_reranker_load and e.reranker_desc.pooling == pooling
        assert all(n is None or n in seen["state"] for n in seen["names"])
    with pytest.raises(ValueError, match="without normalising"):
        enc.load_reranker(Eng(), mro.desc_for(shape, "mean", "f16", normalize=True), w)
    # a post-norm description with mean pooling stays refused
    with pytest.raises(ValueError, match="CLS"):
        enc.load_reranker(Eng(), enc.BertDesc(2, 128, 2, 256, pooling="mean", normalize=False), {})


# ---- pair tokenisation through the library ---------------------------------------------------------------------------------
def test_library_pair_tokenizer_packs_pairs_and_truncates(tmp_path):
    pytest.importorskip("tokenizers")
    from modernbert_rerank_case import bpe_pair_tokenizer

    from voitta_rag_amd.reranker import LibraryPairTokenizer

    tok = bpe_pair_tokenizer()
    tok.save(str(tmp_path / "tokenizer.json"))
    lt = LibraryPairTokenizer.from_pretrained(str(tmp_path), 16)
    a = ["vector index", "", "hybrid " * 40]
    b = ["sparse dense retrieval kernel", "memory", "token " * 40]
    ids, off, seg = lt.encode_pairs(a, b)
    assert ids.dtype == np.int32 and off[0] == 0 and len(off) == 4 and int(off[-1]) == len(ids)
    tok.enable_truncation(max_length=16, strategy="longest_first")
    for i, e in enumerate(tok.encode_batch(list(zip(a, b)))):
        got = ids[off[i]:off[i + 1]]
        assert list(got) == e.ids and got[0] == 1 and got[-1] == 2 and len(got) <= 16
        assert got[seg[i] - 1] == 2  # B starts behind A's [SEP]
    assert int(off[3] - off[2]) == 16
    with pytest.raises(FileNotFoundError):
        LibraryPairTokenizer.from_pretrained(str(tmp_path / "nothing"), 16)


# ---- a checkpoint directory, up to the engine -----------------------------------------------------------------------------
def test_from_pretrained_reads_a_directory(tmp_path, monkeypatch):
    pytest.importorskip("tokenizers")
    from modernbert_rerank_case import reranker_checkpoint

    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd import reranker

    seen = {}
    monkeypatch.setattr(enc, "load_reranker", lambda engine, desc, state: seen.update(desc=desc, state=state))
    monkeypatch.setenv("VOITTA_RERANK_PRECISION", "f16x3")
    shape, w, tok = reranker_checkpoint(str(tmp_path / "rr"), "mean", True, max_length=96)
    rr = reranker.NativeCrossEncoder.from_pretrained(str(tmp_path / "rr"), engine=object())
    d = seen["desc"]
    assert (d.layers, d.hidden, d.heads, d.intermediate, d.vocab, d.type_vocab) == (3, 128, 2, 256, shape.vocab, 1)
    assert (d.norm, d.position, d.ffn, d.window, d.global_every, d.pooling, d.normalize) == ("pre", "rotary", "geglu", 8, 3,
                                                                                          "mean", False)
    assert (d.rope_theta, d.rope_theta_local, d.precision, d.max_pos) == (160000.0, 10000.0, "f16x3", 512)  # 8192, capped
    from voitta_rag_amd.bpe import BpeTokenizer

    assert isinstance(rr.tokenizer, BpeTokenizer) and rr.max_length == rr.tokenizer.max_length == 96
    ids, off, seg = rr.tokenizer.encode_pairs(["vector index"], ["sparse dense retrieval"])
    tok.no_truncation()
    assert ids.tolist() == tok.encode("vector index", "sparse dense retrieval").ids and ids[seg[0] - 1] == 2
    # a tokenizer.json outside the native pipeline: the library tokenises, the engine scores
    spec = json.load(open(tmp_path / "rr" / "tokenizer.json"))
    spec["pre_tokenizer"]["add_prefix_space"] = True
    json.dump(spec, open(tmp_path / "rr" / "tokenizer.json", "w"))
    lib = reranker.NativeCrossEncoder.from_pretrained(str(tmp_path / "rr"), engine=object())
    assert isinstance(lib.tokenizer, reranker.LibraryPairTokenizer) and lib.tokenizer.max_length == 96
    assert [x.size for x in lib.logits(["a", "b"], [[], []])] == [0, 0]
    names, body = enc.modernbert_slots({k: v for k, v in seen["state"].items() if not k.startswith(("head.", "classifier."))}, d)
    head = enc.modernbert_head(seen["state"], d)
    assert np.array_equal(np.asarray(head["head.norm.bias"]), w["head.norm.bias"])
    assert np.array_equal(np.asarray(body["layers.2.post_mlp_layernorm.bias"]), w["final_norm.bias"])
    assert reranker.NativeCrossEncoder.from_pretrained(str(tmp_path / "rr"), engine=object(), max_length=40).max_length == 40
