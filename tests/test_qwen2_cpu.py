"""Qwen2 decoder embedders without a GPU: tests/qwen2_oracle.py against transformers' recorded rows, the description across
the C ABI (VR_NORM_PRE_RMS_ROTARY, causal, VR_POOL_LAST), encoder.qwen2_slots (the slots, repeat_kv, the NULL biases) and
embedding.read_encoder_config on synthetic qwen2 directories with every refusal it has."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qwen2_oracle as qo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LENGTHS = [1, 2, 3, 15, 16, 17, 33, 63, 64, 65, 100, 127, 128, 129, 200]


def golden(name):
    z = np.load(os.path.join(HERE, "golden", f"qwen2_{name}.npz"))
    layers, hidden, heads, kv_heads, inter, vocab = (int(v) for v in z["shape"])
    shape = qo.Qwen2Shape(layers, hidden, heads, kv_heads, inter, vocab=vocab, theta=float(z["theta"]), eps=float(z["eps"]))
    off = z["offsets"]
    return shape, int(z["seed"]), [z["ids"][off[i]:off[i + 1]] for i in range(len(off) - 1)], {"last": z["last"], "mean": z["mean"]}


# ---- the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, heads, kv_heads", [("tiny_d64", 2, 1), ("tiny_d32", 4, 2)])
def test_oracle_matches_transformers_and_the_mask_is_live(name, heads, kv_heads):
    shape, seed, seqs, rows = golden(name)
    assert (shape.layers, shape.hidden, shape.heads, shape.kv_heads, shape.intermediate, shape.vocab, shape.theta, shape.eps) == \
        (2, 128, heads, kv_heads, 256, 200, 1e6, 1e-6)
    assert [len(s) for s in seqs] == LENGTHS
    w = qo.random_weights(shape, seed)
    for pooling in ("last", "mean"):
        worst = float(np.max(np.abs(qo.sentence_embeddings(w, shape, seqs, pooling) - rows[pooling])))
        print(f"{name} {pooling}: oracle - transformers = {worst:.2e}")
        assert worst < 1e-9
    # bidirectional rows are other rows: the flag is live (a 1-token sequence has nothing to mask)
    for pooling in ("last", "mean"):
        free = qo.sentence_embeddings(w, shape, seqs[1:], pooling, causal=False)
        assert np.min(np.max(np.abs(free - rows[pooling][1:]), axis=1)) > 1e-3
    one = qo.sentence_embeddings(w, shape, seqs[:1], "last", causal=False)
    assert np.max(np.abs(one - rows["last"][:1])) < 1e-9


def test_the_weights_have_biases_and_norm_weights_that_matter():
    w = qo.random_weights(qo.Qwen2Shape(2, 128, 4, 2, 256), 3)
    k = qo.layer_keys(1)
    assert w[k["k"]].shape == (64, 128) and w[k["kb"]].shape == (64,) and w[k["q"]].shape == (128, 128)
    for name in ("qb", "kb", "vb"):
        assert np.abs(w[k[name]]).min() > 0
    for name in (k["ln_a"], k["ln_m"], qo.FINAL_KEY):
        assert np.abs(w[name] - 1).max() > 0.05
    assert not any(n.endswith(("o_proj.bias", "mlp.up_proj.bias")) for n in w)


# ---- the description -------------------------------------------------------------------------------------------------------
def test_the_description_crosses_the_abi(tmp_path):
    """(fails without the feature: "unknown norm placement 'rms_pre_rotary'")"""
    from voitta_rag_amd import _lib
    from voitta_rag_amd import encoder as enc

    assert (_lib.VR_NORM_PRE_RMS_ROTARY, _lib.VR_POOL_LAST, _lib.VR_NORM_PRE_RMS) == (3, 2, 2)
    d = enc.BertDesc(2, 128, 2, 256, norm="rms_pre_rotary", causal=1, pooling="last", position="rotary", rope_theta=1e6,
                     ffn="swiglu", type_vocab=1)
    c = d.to_c()
    assert (c.norm, c.causal, c.pooling, c.position, c.ffn) == (3, 1, 2, _lib.VR_POS_ROTARY, _lib.VR_FFN_SWIGLU)
    # a causal description crosses as vr_bert_desc_v2 (vr_bert_desc and `causal` behind it), any other as vr_bert_desc
    assert type(c) is _lib.VrBertDescV2 and c.struct_size == C.sizeof(_lib.VrBertDescV2) == C.sizeof(_lib.VrBertDesc) + 4
    free = enc.BertDesc(2, 128, 2, 256, norm="rms_pre_rotary", position="rotary", rope_theta=1e6, ffn="swiglu", type_vocab=1).to_c()
    assert type(free) is _lib.VrBertDesc and free.struct_size == C.sizeof(_lib.VrBertDesc) and free.norm == 3
    assert d.rms_rotary and not d.rms and not d.prenorm and d.rotary and d.gated
    plain = enc.BertDesc(2, 128, 2, 256).to_c()
    assert (type(plain), plain.pooling, plain.norm) == (_lib.VrBertDesc, 0, 0)
    assert enc.BertDesc(2, 128, 2, 256, pooling="cls").to_c().pooling == 1
    with pytest.raises(ValueError, match="unknown pooling"):
        enc.BertDesc(2, 128, 2, 256, pooling="first").to_c()
    header = open(os.path.join(ROOT, "include", "voitta_engine.h")).read()
    assert "#define VR_NORM_PRE_RMS_ROTARY 3" in header and "#define VR_POOL_LAST 2" in header and "int32_t causal;" in header
    # sizeof of both structs and the new field's offset as gcc sees the header
    src, exe = tmp_path / "s.c", tmp_path / "s"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "voitta_engine.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu\\n",sizeof(vr_bert_desc),sizeof(vr_bert_desc_v2),'
                   'offsetof(vr_bert_desc_v2,causal),offsetof(vr_bert_desc_v2,base));return 0;}\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, size2, causal_at, base_at = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(_lib.VrBertDesc) and size2 == C.sizeof(_lib.VrBertDescV2)
    assert causal_at == _lib.VrBertDescV2.causal.offset == size and base_at == 0
    assert _lib.VrBertDesc._fields_[-1][0] == "rope_theta_local"  # vr_bert_desc itself did not grow
    assert _lib.VrBertDescV2.norm.offset == _lib.VrBertDesc.norm.offset  # the base's fields at their offsets


# ---- the state-dict mapping ------------------------------------------------------------------------------------------------
SLOT_SHAPE = qo.Qwen2Shape(2, 128, 4, 2, 256)  # 4 heads of 32 over 2 KV heads: g = 2


@pytest.mark.parametrize("prefix", ["", "model.", "0.auto_model."])
def test_state_dict_maps_onto_the_slots_and_kv_heads_repeat(prefix):
    from voitta_rag_amd import encoder as enc

    w = qo.random_weights(SLOT_SHAPE, 21)
    for i in range(2):  # distinguishable rows: row r of every K / V tensor holds r (+ 1000 for V)
        k = qo.layer_keys(i)
        w[k["k"]] = np.repeat(np.arange(64, dtype=np.float32)[:, None], 128, 1)
        w[k["v"]] = w[k["k"]] + 1000
        w[k["kb"]], w[k["vb"]] = np.arange(64, dtype=np.float32), np.arange(64, dtype=np.float32) + 1000
    state = {prefix + k: v for k, v in w.items()}
    state["lm_head.weight"] = w[qo.WORD_KEY]  # (ignored)
    desc = qo.desc_for(SLOT_SHAPE, "last", "f32")
    names, out = enc.qwen2_slots(state, desc)
    assert len(names) == 5 + 18 * 2
    assert names[1] is None and names[2] is None and names[4] is None  # no positions, no token types, no shift
    assert np.array_equal(out[names[0]], w[qo.WORD_KEY])
    assert np.array_equal(out[names[3]], w[qo.layer_keys(0)["ln_a"]])  # embeddings.LayerNorm = layers.0.input_layernorm
    # repeat_kv: query head h reads KV head h // 2 -> rows [0..32) [0..32) [32..64) [32..64)
    order = np.concatenate([np.arange(32), np.arange(32), np.arange(32, 64), np.arange(32, 64)]).astype(np.float32)
    for i in range(2):
        per, k = names[5 + 18 * i:5 + 18 * (i + 1)], qo.layer_keys(i)
        assert [j for j in range(18) if per[j] is None] == [7, 9, 11, 13, 15, 17]  # o_proj, norm shifts, the MLP: no bias
        assert np.array_equal(out[per[0]], w[k["q"]]) and np.array_equal(out[per[1]], w[k["qb"]])
        assert out[per[2]].shape == (128, 128) and np.array_equal(out[per[2]][:, 0], order) and np.array_equal(out[per[3]], order)
        assert np.array_equal(out[per[4]][:, 5], order + 1000) and np.array_equal(out[per[5]], order + 1000)
        for slot, short in ((6, "o"), (8, "ln_m"), (10, "up"), (12, "down"), (16, "gate")):
            assert np.array_equal(out[per[slot]], w[k[short]]), short
        nxt = w[qo.layer_keys(1)["ln_a"]] if i == 0 else w[qo.FINAL_KEY]
        assert np.array_equal(out[per[14]], nxt)  # layers.l+1.input_layernorm, `norm` for the last
    for n in names:
        if n is not None:
            assert tuple(out[n].shape) == enc.expected_shape(desc, n), n
    # the repeated heads are what HF's repeat_kv computes: the oracle with kv_heads = heads on the mapped weights
    full = qo.Qwen2Shape(2, 128, 4, 4, 256)
    w2 = qo.random_weights(SLOT_SHAPE, 22)
    _, mapped = enc.qwen2_slots(dict(w2), desc)
    as_full = dict(w2)
    for i in range(2):
        k = qo.layer_keys(i)
        for short in ("k", "kb", "v", "vb"):
            as_full[k[short]] = mapped[k[short]]
    s = np.arange(40) % SLOT_SHAPE.vocab
    assert np.array_equal(qo.encode_one(as_full, full, s), qo.encode_one(w2, SLOT_SHAPE, s))


def test_slots_refuse_leftovers_missing_tensors_and_odd_kv_rows():
    from voitta_rag_amd import encoder as enc

    w = qo.random_weights(SLOT_SHAPE, 21)
    desc = qo.desc_for(SLOT_SHAPE, "last", "f32")
    with pytest.raises(ValueError, match=r"unexpected tensors \['layers\.0\.self_attn\.q_norm\.weight'\]"):
        enc.qwen2_slots(dict(w, **{"layers.0.self_attn.q_norm.weight": np.ones(32, np.float32)}), desc)
    with pytest.raises(ValueError, match=r"unexpected tensors \['layers\.2\.mlp\.up_proj\.weight'\]"):
        enc.qwen2_slots(dict(w, **{"layers.2.mlp.up_proj.weight": w["layers.1.mlp.up_proj.weight"]}), desc)
    for gone in (qo.layer_keys(1)["down"], qo.FINAL_KEY, qo.layer_keys(0)["kb"]):
        with pytest.raises(KeyError, match=gone.replace(".", r"\.")):
            enc.qwen2_slots({k: v for k, v in w.items() if k != gone}, desc)
    with pytest.raises(ValueError, match="num_attention_heads 4 is not a multiple of num_key_value_heads 3"):
        enc.qwen2_slots(dict(w), desc, kv_heads=3)
    with pytest.raises(ValueError, match=r"has 64 rows, num_key_value_heads 1 of head size 32 imply 32"):
        enc.qwen2_slots(dict(w), desc, kv_heads=1)


def test_load_encoder_passes_null_slots_and_the_description():
    from voitta_rag_amd import encoder as enc

    w = qo.random_weights(SLOT_SHAPE, 21)
    calls = []

    class Lib:
        @staticmethod
        def vr_encoder_load(handle, desc, arr, n, mem):
            d = C.cast(desc, C.POINTER(enc._lib.VrBertDescV2)).contents
            assert d.struct_size == C.sizeof(enc._lib.VrBertDescV2)
            calls.append((n, d.position, d.ffn, d.norm, d.causal, d.pooling, [i for i in range(n) if arr[i] is None]))
            return 0

    class FakeEngine:
        handle, _lib = None, Lib

    enc.load_encoder(FakeEngine(), qo.desc_for(SLOT_SHAPE, "last", "f32"), w)
    null = [1, 2, 4] + [5 + 18 * l + j for l in range(2) for j in (7, 9, 11, 13, 15, 17)]
    assert calls == [(5 + 18 * 2, enc._lib.VR_POS_ROTARY, enc._lib.VR_FFN_SWIGLU, 3, 1, 2, null)]


# ---- the directory reader --------------------------------------------------------------------------------------------------
QWEN_05B = qo.Qwen2Shape(24, 896, 14, 2, 4864, vocab=151936)


@pytest.fixture
def settings(monkeypatch):
    """Environment for get_settings(), which caches: dropped on every change and when the test ends."""
    from voitta_rag_amd import config

    def setenv(**env):
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        config.get_settings.cache_clear()

    monkeypatch.delenv("VOITTA_ENCODER_PRECISION", raising=False)
    monkeypatch.delenv("VOITTA_MAX_SEQ_LENGTH", raising=False)
    config.get_settings.cache_clear()
    yield setenv
    config.get_settings.cache_clear()


def test_config_reader_describes_the_half_billion_body(tmp_path, settings):
    from voitta_rag_amd.embedding import read_encoder_config

    d = str(tmp_path / "qwen")
    qo.write_checkpoint(d, QWEN_05B, 5, max_seq=512, body=False)
    rc = read_encoder_config(d)
    desc = rc["desc"]
    assert (desc.layers, desc.hidden, desc.heads, desc.intermediate, desc.vocab) == (24, 896, 14, 4864, 151936)
    assert (desc.norm, desc.ffn, desc.position, desc.window, desc.type_vocab, desc.causal) == ("rms_pre_rotary", "swiglu", "rotary", 0, 1, 1)
    assert (desc.max_pos, rc["max_seq"], desc.eps, desc.rope_theta, desc.pooling, desc.normalize) == (512, 512, 1e-6, 1e6, "last", True)
    assert (rc["kv_heads"], desc.precision, desc.head) == (2, "f16", None)


@pytest.mark.parametrize("pooling", ["last", "mean", "cls"])
def test_pooling_comes_from_the_pooling_module(tmp_path, settings, pooling):
    from voitta_rag_amd.embedding import read_encoder_config

    d = str(tmp_path / "m")
    qo.write_checkpoint(d, qo.Qwen2Shape(2, 128, 2, 1, 256), 5, pooling=pooling, body=False)
    assert read_encoder_config(d)["desc"].pooling == pooling


def test_a_bare_config_is_causal_is_false_and_the_sequence_cap(tmp_path, settings):
    from voitta_rag_amd.embedding import read_encoder_config

    shape = qo.Qwen2Shape(2, 128, 2, 1, 256)
    bare = str(tmp_path / "bare")
    qo.write_checkpoint(bare, shape, 5, body=False, modules=False, max_seq=None, config=dict(max_position_embeddings=300))
    rc = read_encoder_config(bare)  # no modules.json: mean pooling, no Normalize, the config's own longest sequence
    assert (rc["desc"].pooling, rc["desc"].normalize, rc["desc"].causal, rc["max_seq"], rc["desc"].max_pos) == ("mean", False, 1, 300, 300)
    free = str(tmp_path / "free")
    qo.write_checkpoint(free, shape, 5, body=False, config=dict(is_causal=False))
    assert read_encoder_config(free)["desc"].causal == 0
    both = str(tmp_path / "both")
    qo.write_checkpoint(both, shape, 5, body=False, config=dict(is_causal=True, num_key_value_heads=None))
    rc = read_encoder_config(both)
    assert rc["desc"].causal == 1 and rc["kv_heads"] == 2  # no num_key_value_heads: multi-head attention
    long = str(tmp_path / "long")
    qo.write_checkpoint(long, shape, 5, body=False, max_seq=3000)  # min(max_seq_length, max_position_embeddings, cap)
    assert read_encoder_config(long)["max_seq"] == 512
    settings(VOITTA_MAX_SEQ_LENGTH=2048)
    assert read_encoder_config(long)["max_seq"] == 2048 and read_encoder_config(long)["desc"].max_pos == 2048
    settings(VOITTA_MAX_SEQ_LENGTH=4096)
    assert read_encoder_config(long)["max_seq"] == 3000
    short = str(tmp_path / "short")
    qo.write_checkpoint(short, shape, 5, body=False, max_seq=3000, config=dict(max_position_embeddings=1024))
    assert read_encoder_config(short)["max_seq"] == 1024
    theta5 = str(tmp_path / "theta5")  # transformers 5's spelling of the base
    qo.write_checkpoint(theta5, shape, 5, body=False, config=dict(rope_theta=None, rope_parameters={"rope_type": "default", "rope_theta": 5e5}))
    assert read_encoder_config(theta5)["desc"].rope_theta == 5e5


@pytest.mark.parametrize("over, message", [
    (dict(num_key_value_heads=3), "num_attention_heads 4 is not a multiple of num_key_value_heads 3"),
    (dict(head_dim=64), r"head_dim 64 differs from hidden_size / num_attention_heads = 128 / 4"),
    (dict(num_attention_heads=1, num_key_value_heads=1), r"head size 128 \(hidden_size 128 / num_attention_heads 1\)"),
    (dict(num_attention_heads=8, num_key_value_heads=2), r"head size 16 \(hidden_size 128 / num_attention_heads 8\)"),
    (dict(hidden_size=192, num_attention_heads=6, num_key_value_heads=2), "hidden_size 192 is not implemented"),
    (dict(hidden_size=1536, num_attention_heads=24, num_key_value_heads=2), "hidden_size 1536 is not implemented"),
    (dict(hidden_act="gelu"), "hidden_act 'gelu' is not implemented"),
    (dict(rope_scaling={"type": "yarn", "factor": 4.0}), "rope_scaling .*yarn.* is not implemented"),
    (dict(rope_parameters={"rope_type": "linear", "rope_theta": 1e6}), "rope_scaling 'linear' is not implemented"),
    (dict(use_sliding_window=True), "use_sliding_window true is not implemented"),
])
def test_config_reader_refusals(tmp_path, settings, over, message):
    from voitta_rag_amd.embedding import read_encoder_config

    d = str(tmp_path / "m")
    qo.write_checkpoint(d, qo.Qwen2Shape(2, 128, 4, 2, 256), 5, body=False, config=over)
    with pytest.raises(ValueError, match=message):
        read_encoder_config(d)


def test_unsupported_model_types_list_qwen2(tmp_path, settings):
    from voitta_rag_amd.embedding import read_encoder_config

    d = str(tmp_path / "m")
    qo.write_checkpoint(d, qo.Qwen2Shape(2, 128, 2, 1, 256), 5, body=False, config=dict(model_type="qwen3"))
    with pytest.raises(ValueError, match="unsupported model_type qwen3: BERT, DistilBERT, XLM-RoBERTa, MPNet, T5, nomic_bert and "
                                         "modernbert encoders only.*Qwen2"):
        read_encoder_config(d)


def test_the_fixture_tokenizer_runs_natively_and_qwens_own_pattern_goes_to_the_library(tmp_path, settings):
    import json

    from voitta_rag_amd.bpe import BpeTokenizer
    from voitta_rag_amd.embedding import NativeSentenceEncoder

    d = str(tmp_path / "m")
    qo.write_checkpoint(d, qo.Qwen2Shape(2, 128, 2, 1, 256), 5, body=False)
    cfg = json.load(open(os.path.join(d, "config.json")))
    assert isinstance(NativeSentenceEncoder._load_tokenizer(d, cfg), BpeTokenizer)
    spec = json.load(open(os.path.join(d, "tokenizer.json"), encoding="utf-8"))
    qwen_split = {"type": "Split", "behavior": "Isolated", "invert": False, "pattern": {
        "Regex": r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+"}}
    spec["pre_tokenizer"] = {"type": "Sequence", "pretokenizers": [
        qwen_split, {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": False, "use_regex": False}]}
    with pytest.raises((ValueError, KeyError, TypeError), match="pre_tokenizer"):
        BpeTokenizer.from_tokenizer_json(spec)
    json.dump(spec, open(os.path.join(d, "tokenizer.json"), "w", encoding="utf-8"))
    assert not isinstance(NativeSentenceEncoder._load_tokenizer(d, cfg), BpeTokenizer)  # the tokenizers library's object
