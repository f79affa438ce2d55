"""Qwen3 decoder embedders without a GPU: tests/qwen3_oracle.py against transformers' recorded rows, the logit condition
its Q/K gains are drawn for, vr_bert_desc_v3 across the C ABI (head_dim, qk_norm), encoder.qwen3_slots (the slots,
repeat_kv over heads of head_dim, the norm weights at 18 and 19) and embedding.read_encoder_config on synthetic qwen3
directories with every refusal it has."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qwen3_oracle as qo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LENGTHS = [1, 2, 3, 15, 16, 17, 33, 63, 64, 65, 100, 127, 128, 129, 200]
GOLDENS = [("tiny_d128", 128, 2, 1, 128), ("tiny_d128b", 256, 4, 2, 128), ("tiny_d64n", 128, 2, 1, 64)]


def golden(name):
    z = np.load(os.path.join(HERE, "golden", f"qwen3_{name}.npz"))
    layers, hidden, heads, kv_heads, inter, head_dim, qk_norm, vocab = (int(v) for v in z["shape"])
    shape = qo.Qwen3Shape(layers, hidden, heads, kv_heads, inter, head_dim, qk_norm=bool(qk_norm), vocab=vocab,
                          theta=float(z["theta"]), eps=float(z["eps"]))
    off = z["offsets"]
    return shape, int(z["seed"]), [z["ids"][off[i]:off[i + 1]] for i in range(len(off) - 1)], {"last": z["last"], "mean": z["mean"]}


# ---- the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, hidden, heads, kv_heads, head_dim", GOLDENS)
def test_oracle_matches_transformers_and_the_mask_is_live(name, hidden, heads, kv_heads, head_dim):
    shape, seed, seqs, rows = golden(name)
    assert (shape.layers, shape.hidden, shape.heads, shape.kv_heads, shape.intermediate, shape.head_dim, shape.qk_norm,
            shape.vocab, shape.theta, shape.eps) == (2, hidden, heads, kv_heads, 256, head_dim, True, 200, 1e6, 1e-6)
    assert [len(s) for s in seqs] == LENGTHS
    w = qo.random_weights(shape, seed)
    for pooling in ("last", "mean"):
        worst = float(np.max(np.abs(qo.sentence_embeddings(w, shape, seqs, pooling) - rows[pooling])))
        print(f"{name} {pooling}: oracle - transformers = {worst:.2e}")
        assert worst < 1e-9
    for pooling in ("last", "mean"):  # bidirectional rows are other rows (a 1-token sequence has nothing to mask)
        free = qo.sentence_embeddings(w, shape, seqs[1:], pooling, causal=False)
        assert np.min(np.max(np.abs(free - rows[pooling][1:]), axis=1)) > 1e-3
    # ... and so are rows without the Q/K norms, or with unit gains: both weights are live
    import dataclasses

    bare = qo.sentence_embeddings(w, dataclasses.replace(shape, qk_norm=False), seqs[3:], "last")
    assert np.min(np.max(np.abs(bare - rows["last"][3:]), axis=1)) > 1e-3
    unit = {k: (np.ones_like(v) if k.endswith(("q_norm.weight", "k_norm.weight")) else v) for k, v in w.items()}
    assert np.min(np.max(np.abs(qo.sentence_embeddings(unit, shape, seqs[3:], "last") - rows["last"][3:]), axis=1)) > 1e-4


@pytest.mark.parametrize("name", [g[0] for g in GOLDENS])
def test_the_gains_keep_the_logits_of_order_one(name):
    """The condition on the INPUTS: at most a quarter of the (layer, head, query) triples of the 200-token sequence put
    more than half their weight on one key — else a wrong key would hide behind a one-hot softmax — and the weights are
    not uniform either (the largest weight of a late query is well above 1 / keys)."""
    shape, seed, seqs, _ = golden(name)
    w = qo.random_weights(shape, seed)
    for n in range(2):
        k = qo.layer_keys(n)
        for g in (w[k["qn"]], w[k["kn"]]):
            assert g.shape == (shape.head_dim,) and np.abs(g - 1).max() > 0.05  # not one
    share = qo.peaked_share(w, shape, seqs[-1])
    probe = []
    qo.encode_one(w, shape, seqs[-1], probe=probe)
    top = float(np.median(np.stack(probe)[:, :, 100:].max(axis=-1)))
    print(f"{name}: peaked share {share:.3f}, median largest weight of queries 100.. {top:.3f}")
    assert share <= 0.25
    assert top > 3.0 / 200


# ---- the description -------------------------------------------------------------------------------------------------------
def test_the_description_crosses_the_abi(tmp_path):
    """(fails without the feature: BertDesc has no head_dim)"""
    from voitta_rag_amd import _lib
    from voitta_rag_amd import encoder as enc

    base = dict(norm="rms_pre_rotary", causal=1, pooling="last", position="rotary", rope_theta=1e6, ffn="swiglu", type_vocab=1)
    d = enc.BertDesc(2, 128, 2, 256, head_dim=128, qk_norm=1, **base)
    c = d.to_c()
    assert type(c) is _lib.VrBertDescV3 and c.struct_size == C.sizeof(_lib.VrBertDescV3) == C.sizeof(_lib.VrBertDescV2) + 8
    assert (c.norm, c.causal, c.head_dim, c.qk_norm, c.heads, c.hidden) == (3, 1, 128, 1, 2, 128)
    assert (d.head_size, d.attn_width, d.out_dim) == (128, 256, 128)  # the row stays `hidden` wide
    for kw in (dict(head_dim=64), dict(qk_norm=1)):  # either field alone is enough
        one = enc.BertDesc(2, 128, 2, 256, **kw, **base).to_c()
        assert type(one) is _lib.VrBertDescV3 and (one.head_dim, one.qk_norm) == (kw.get("head_dim", 0), kw.get("qk_norm", 0))
    free = enc.BertDesc(2, 128, 2, 256, head_dim=128, **dict(base, causal=0)).to_c()
    assert type(free) is _lib.VrBertDescV3 and free.causal == 0
    header = open(os.path.join(ROOT, "include", "voitta_engine.h")).read()
    assert "int32_t head_dim;" in header and "int32_t qk_norm;" in header and "vr_bert_desc_v3" in header
    # sizeof of all three structs and the new fields' offsets as gcc sees the header
    src, exe = tmp_path / "s.c", tmp_path / "s"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "voitta_engine.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu\\n",sizeof(vr_bert_desc),sizeof(vr_bert_desc_v2),'
                   'sizeof(vr_bert_desc_v3),offsetof(vr_bert_desc_v3,head_dim),offsetof(vr_bert_desc_v3,qk_norm),'
                   'offsetof(vr_bert_desc_v3,v2),offsetof(vr_bert_desc_v3,v2.causal));return 0;}\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    s1, s2, s3, hd_at, qn_at, v2_at, causal_at = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True,
                                                                                text=True).stdout.split())
    assert (s1, s2, s3) == (C.sizeof(_lib.VrBertDesc), C.sizeof(_lib.VrBertDescV2), C.sizeof(_lib.VrBertDescV3))
    assert hd_at == _lib.VrBertDescV3.head_dim.offset == s2 and qn_at == _lib.VrBertDescV3.qk_norm.offset == s2 + 4
    assert v2_at == 0 and causal_at == _lib.VrBertDescV3.causal.offset == s1
    assert _lib.VrBertDesc._fields_[-1][0] == "rope_theta_local" and _lib.VrBertDescV2._fields_ == [("causal", C.c_int32)]
    assert _lib.VrBertDescV3.norm.offset == _lib.VrBertDesc.norm.offset  # the base's fields at their offsets


def test_every_existing_family_crosses_as_the_bytes_it_always_was():
    from voitta_rag_amd import _lib
    from voitta_rag_amd import encoder as enc

    def old_bytes(d):  # to_c() as it was before head_dim and qk_norm existed: the fields in order, v2 only when causal
        c = _lib.VrBertDescV2() if d.causal else _lib.VrBertDesc()
        c.struct_size = C.sizeof(type(c))
        c.layers, c.hidden, c.heads, c.intermediate, c.vocab, c.max_pos, c.type_vocab = (
            d.layers, d.hidden, d.heads, d.intermediate, d.vocab, d.max_pos, d.type_vocab)
        c.pooling = {"mean": 0, "cls": 1, "last": 2}[d.pooling]
        c.normalize, c.eps = int(d.normalize), d.eps
        c.precision = {"f32": 0, "f16x3": 1, "f16": 2}[d.precision]
        c.position = {"learned": 0, "rotary": 1, "none": 2}[d.position]
        c.rope_theta, c.ffn = d.rope_theta, {"gelu": 0, "swiglu": 1, "geglu": 2, "relu": 3}[d.ffn]
        c.norm = {"post": 0, "pre": 1, "rms_pre": 2, "rms_pre_rotary": 3}[d.norm]
        c.window, c.global_every, c.rope_theta_local = d.window, d.global_every, d.rope_theta_local
        if d.causal:
            c.causal = 1
        return bytes(c)

    families = [
        enc.BertDesc(12, 768, 12, 3072, pooling="cls", precision="f16"),  # BERT / XLM-R / MPNet / DistilBERT
        enc.BertDesc(12, 768, 12, 3072, position="rotary", rope_theta=1000.0, ffn="swiglu", type_vocab=2),  # nomic
        enc.BertDesc(22, 768, 12, 1152, position="rotary", rope_theta=160000.0, ffn="geglu", norm="pre", window=64,
                     global_every=3, rope_theta_local=10000.0, type_vocab=1, eps=1e-5),  # ModernBERT
        enc.BertDesc(12, 768, 12, 3072, position="none", ffn="geglu", type_vocab=2),  # ALiBi
        enc.BertDesc(12, 768, 12, 3072, position="none", ffn="relu", norm="rms_pre", type_vocab=1, eps=1e-6),  # T5
        enc.BertDesc(24, 896, 14, 4864, position="rotary", rope_theta=1e6, ffn="swiglu", norm="rms_pre_rotary", causal=1,
                     pooling="last", type_vocab=1, eps=1e-6, precision="f16"),  # Qwen2
        enc.BertDesc(24, 896, 14, 4864, position="rotary", rope_theta=1e6, ffn="swiglu", norm="rms_pre_rotary", type_vocab=1),
    ]
    for d in families:
        c = d.to_c()
        assert type(c) is (_lib.VrBertDescV2 if d.causal else _lib.VrBertDesc)
        assert bytes(c) == old_bytes(d), d
        assert (d.head_size, d.attn_width) == (d.hidden // d.heads, d.hidden)


# ---- the state-dict mapping ------------------------------------------------------------------------------------------------
SLOT_SHAPE = qo.Qwen3Shape(2, 128, 4, 2, 256, 64)  # 4 heads of 64 over 2 KV heads: g = 2, A = 256


@pytest.mark.parametrize("prefix", ["", "model.", "0.auto_model."])
def test_state_dict_maps_onto_the_slots_and_kv_heads_repeat(prefix):
    from voitta_rag_amd import encoder as enc

    w = qo.random_weights(SLOT_SHAPE, 21)
    for i in range(2):  # distinguishable rows: row r of every K / V tensor holds r (+ 1000 for V)
        k = qo.layer_keys(i)
        w[k["k"]] = np.repeat(np.arange(128, dtype=np.float32)[:, None], 128, 1)
        w[k["v"]] = w[k["k"]] + 1000
    state = {prefix + k: v for k, v in w.items()}
    state["lm_head.weight"] = w[qo.WORD_KEY]  # (ignored)
    desc = qo.desc_for(SLOT_SHAPE, "last", "f32")
    names, out = enc.qwen3_slots(state, desc)
    assert len(names) == 5 + 20 * 2
    assert names[1] is None and names[2] is None and names[4] is None  # no positions, no token types, no shift
    assert np.array_equal(out[names[0]], w[qo.WORD_KEY])
    assert np.array_equal(out[names[3]], w[qo.layer_keys(0)["ln_a"]])  # embeddings.LayerNorm = layers.0.input_layernorm
    # repeat_kv over heads of 64: query head h reads KV head h // 2 -> rows [0..64) [0..64) [64..128) [64..128)
    order = np.concatenate([np.arange(64), np.arange(64), np.arange(64, 128), np.arange(64, 128)]).astype(np.float32)
    for i in range(2):
        per, k = names[5 + 20 * i:5 + 20 * (i + 1)], qo.layer_keys(i)
        # no attention biases (attention_bias false), o_proj, norm shifts, the MLP: no bias
        assert [j for j in range(20) if per[j] is None] == [1, 3, 5, 7, 9, 11, 13, 15, 17]
        assert np.array_equal(out[per[0]], w[k["q"]]) and out[per[0]].shape == (256, 128)
        assert out[per[2]].shape == (256, 128) and np.array_equal(out[per[2]][:, 0], order)
        assert out[per[4]].shape == (256, 128) and np.array_equal(out[per[4]][:, 5], order + 1000)
        assert out[per[6]].shape == (128, 256)
        for slot, short in ((6, "o"), (8, "ln_m"), (10, "up"), (12, "down"), (16, "gate"), (18, "qn"), (19, "kn")):
            assert np.array_equal(out[per[slot]], w[k[short]]), short
        assert per[18].endswith("self_attn.q_norm.weight") and per[19].endswith("self_attn.k_norm.weight")
        assert out[per[18]].shape == (64,) and not np.array_equal(out[per[18]], out[per[19]])
        nxt = w[qo.layer_keys(1)["ln_a"]] if i == 0 else w[qo.FINAL_KEY]
        assert np.array_equal(out[per[14]], nxt)  # layers.l+1.input_layernorm, `norm` for the last
    for n in names:
        if n is not None:
            assert tuple(out[n].shape) == enc.expected_shape(desc, n), n
    # the repeated heads are what HF's repeat_kv computes: the oracle with kv_heads = heads on the mapped weights
    import dataclasses

    full = dataclasses.replace(SLOT_SHAPE, kv_heads=4)
    w2 = qo.random_weights(SLOT_SHAPE, 22)
    _, mapped = enc.qwen3_slots(dict(w2), desc)
    as_full = dict(w2)
    for i in range(2):
        k = qo.layer_keys(i)
        for short in ("k", "v"):
            as_full[k[short]] = mapped[k[short]]
    s = np.arange(40) % SLOT_SHAPE.vocab
    assert np.array_equal(qo.encode_one(as_full, full, s), qo.encode_one(w2, SLOT_SHAPE, s))


def test_attention_biases_take_their_slots_where_the_checkpoint_has_them():
    import dataclasses

    from voitta_rag_amd import encoder as enc

    shape = dataclasses.replace(SLOT_SHAPE, attention_bias=True)
    w = qo.random_weights(shape, 4)
    names, out = enc.qwen3_slots(dict(w), qo.desc_for(shape, "last", "f32"))
    per, k = names[5:25], qo.layer_keys(0)
    assert [j for j in range(20) if per[j] is None] == [7, 9, 11, 13, 15, 17]
    assert np.array_equal(out[per[1]], w[k["qb"]]) and out[per[3]].shape == (256,) and out[per[5]].shape == (256,)
    assert np.array_equal(out[per[3]][:64], w[k["kb"]][:64]) and np.array_equal(out[per[3]][64:128], w[k["kb"]][:64])


def test_slots_refuse_leftovers_missing_tensors_and_odd_kv_rows():
    from voitta_rag_amd import encoder as enc

    w = qo.random_weights(SLOT_SHAPE, 21)
    desc = qo.desc_for(SLOT_SHAPE, "last", "f32")
    with pytest.raises(ValueError, match=r"not a Qwen3 state dict of 2 layers: unexpected tensors \['layers\.2\.mlp\.up_proj\.weight'\]"):
        enc.qwen3_slots(dict(w, **{"layers.2.mlp.up_proj.weight": w["layers.1.mlp.up_proj.weight"]}), desc)
    with pytest.raises(ValueError, match=r"unexpected tensors \['score\.weight'\]"):
        enc.qwen3_slots(dict(w, **{"score.weight": np.ones((1, 128), np.float32)}), desc)
    for gone in (qo.layer_keys(1)["down"], qo.FINAL_KEY, qo.layer_keys(0)["kn"], qo.layer_keys(1)["qn"]):
        with pytest.raises(KeyError, match=gone.replace(".", r"\.")):
            enc.qwen3_slots({k: v for k, v in w.items() if k != gone}, desc)
    with pytest.raises(ValueError, match="num_attention_heads 4 is not a multiple of num_key_value_heads 3"):
        enc.qwen3_slots(dict(w), desc, kv_heads=3)
    with pytest.raises(ValueError, match=r"has 128 rows, num_key_value_heads 1 of head size 64 imply 64"):
        enc.qwen3_slots(dict(w), desc, kv_heads=1)


def test_load_encoder_passes_null_slots_and_the_v3_description():
    from voitta_rag_amd import encoder as enc

    w = qo.random_weights(SLOT_SHAPE, 21)
    calls = []

    class Lib:
        @staticmethod
        def vr_encoder_load(handle, desc, arr, n, mem):
            d = C.cast(desc, C.POINTER(enc._lib.VrBertDescV3)).contents
            assert d.struct_size == C.sizeof(enc._lib.VrBertDescV3)
            calls.append((n, d.norm, d.causal, d.head_dim, d.qk_norm, d.pooling, [i for i in range(n) if arr[i] is None]))
            return 0

    class FakeEngine:
        handle, _lib = None, Lib

    enc.load_encoder(FakeEngine(), qo.desc_for(SLOT_SHAPE, "last", "f32"), w)
    null = [1, 2, 4] + [5 + 20 * l + j for l in range(2) for j in (1, 3, 5, 7, 9, 11, 13, 15, 17)]
    assert calls == [(5 + 20 * 2, 3, 1, 64, 1, 2, null)]
    bad = dict(w)
    bad[qo.layer_keys(0)["qn"]] = np.ones(128, np.float32)
    with pytest.raises(ValueError, match=r"q_norm\.weight' has shape \(128,\), the model description implies \(64,\)"):
        enc.load_encoder(FakeEngine(), qo.desc_for(SLOT_SHAPE, "last", "f32"), bad)


# ---- the directory reader --------------------------------------------------------------------------------------------------
QWEN3_06B = qo.Qwen3Shape(28, 1024, 16, 8, 3072, 128, vocab=151669)


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


def test_config_reader_describes_the_0_6b_body(tmp_path, settings):
    from voitta_rag_amd.embedding import read_encoder_config

    d = str(tmp_path / "qwen3")
    qo.write_checkpoint(d, QWEN3_06B, 5, max_seq=512, body=False)
    rc = read_encoder_config(d)
    desc = rc["desc"]
    assert (desc.layers, desc.hidden, desc.heads, desc.intermediate, desc.vocab) == (28, 1024, 16, 3072, 151669)
    assert (desc.head_dim, desc.qk_norm, desc.head_size, desc.attn_width, desc.out_dim) == (128, 1, 128, 2048, 1024)
    assert (desc.norm, desc.ffn, desc.position, desc.window, desc.type_vocab, desc.causal) == ("rms_pre_rotary", "swiglu", "rotary", 0, 1, 1)
    assert (desc.max_pos, rc["max_seq"], desc.eps, desc.rope_theta, desc.pooling, desc.normalize) == (512, 512, 1e-6, 1e6, "last", True)
    assert (rc["kv_heads"], rc["attention_bias"], desc.precision, desc.head) == (8, False, "f16", None)


def test_head_dim_defaults_and_the_other_fields(tmp_path, settings):
    from voitta_rag_amd.embedding import read_encoder_config

    shape = qo.Qwen3Shape(2, 128, 2, 1, 256, 64)
    d = str(tmp_path / "default")
    qo.write_checkpoint(d, shape, 5, body=False, config=dict(head_dim=None))
    desc = read_encoder_config(d)["desc"]
    assert (desc.head_dim, desc.qk_norm, desc.attn_width) == (64, 1, 128)  # hidden / heads
    for pooling in ("last", "mean", "cls"):
        p = str(tmp_path / pooling)
        qo.write_checkpoint(p, shape, 5, pooling=pooling, body=False)
        assert read_encoder_config(p)["desc"].pooling == pooling
    free = str(tmp_path / "free")
    qo.write_checkpoint(free, shape, 5, body=False, config=dict(is_causal=False, attention_bias=True, rms_norm_eps=1e-5))
    rc = read_encoder_config(free)
    assert (rc["desc"].causal, rc["attention_bias"], rc["desc"].eps) == (0, True, 1e-5)
    theta5 = str(tmp_path / "theta5")  # transformers 5's spelling of the base
    qo.write_checkpoint(theta5, shape, 5, body=False, config=dict(rope_theta=None, rope_parameters={"rope_type": "default", "rope_theta": 5e5}))
    assert read_encoder_config(theta5)["desc"].rope_theta == 5e5
    bare = str(tmp_path / "bare")
    qo.write_checkpoint(bare, shape, 5, body=False, modules=False, max_seq=None, config=dict(max_position_embeddings=300))
    rc = read_encoder_config(bare)
    assert (rc["desc"].pooling, rc["desc"].normalize, rc["max_seq"]) == ("mean", False, 300)


@pytest.mark.parametrize("over, message", [
    (dict(num_key_value_heads=3), "num_attention_heads 4 is not a multiple of num_key_value_heads 3"),
    (dict(head_dim=16), "head_dim 16 is not implemented: the attention kernels run head sizes 32, 64 and 128"),
    (dict(head_dim=256), "head_dim 256 is not implemented"),
    (dict(head_dim=96), "head_dim 96 is not implemented"),
    (dict(num_attention_heads=32, num_key_value_heads=8, head_dim=128), r"num_attention_heads 32 x head_dim 128 = 4096 is not implemented"),
    (dict(num_attention_heads=2, num_key_value_heads=1, head_dim=32), r"num_attention_heads 2 x head_dim 32 = 64 is not implemented"),
    (dict(hidden_size=192), "hidden_size 192 is not implemented"),
    (dict(hidden_size=2560), "hidden_size 2560 is not implemented"),
    (dict(hidden_act="gelu"), "hidden_act 'gelu' is not implemented"),
    (dict(rope_scaling={"type": "yarn", "factor": 4.0}), "rope_scaling .*yarn.* is not implemented"),
    (dict(rope_parameters={"rope_type": "linear", "rope_theta": 1e6}), "rope_scaling 'linear' is not implemented"),
    (dict(use_sliding_window=True), "use_sliding_window true is not implemented"),
])
def test_config_reader_refusals(tmp_path, settings, over, message):
    from voitta_rag_amd.embedding import read_encoder_config

    d = str(tmp_path / "m")
    qo.write_checkpoint(d, qo.Qwen3Shape(2, 128, 4, 2, 256, 64), 5, body=False, config=over)
    with pytest.raises(ValueError, match=message):
        read_encoder_config(d)


def test_unsupported_model_types_list_qwen3(tmp_path, settings):
    from voitta_rag_amd.embedding import read_encoder_config

    d = str(tmp_path / "m")
    qo.write_checkpoint(d, qo.Qwen3Shape(2, 128, 2, 1, 256, 64), 5, body=False, config=dict(model_type="qwen3_moe"))
    with pytest.raises(ValueError, match="unsupported model_type qwen3_moe: BERT, DistilBERT, XLM-RoBERTa, MPNet, T5, nomic_bert and "
                                         "modernbert encoders only.*Qwen2.*Qwen3"):
        read_encoder_config(d)


def test_a_qwen3_directory_of_another_familys_classes_is_refused(tmp_path, settings):
    """model_type qwen3 beside architectures that name no Qwen3 class: refused with the model-type message and the classes;
    Qwen3ForCausalLM (the published checkpoints' class) and a config without architectures load."""
    from voitta_rag_amd.embedding import read_encoder_config

    shape = qo.Qwen3Shape(2, 128, 2, 1, 256, 64)
    d = str(tmp_path / "other")
    qo.write_checkpoint(d, shape, 5, body=False, config=dict(architectures=["Qwen2Model"]))
    with pytest.raises(ValueError, match=r"unsupported model_type qwen3: .*Qwen3 decoder embedders \(the 0.6B body\); "
                                         r"architectures \['Qwen2Model'\] is not a Qwen3 model"):
        read_encoder_config(d)
    for i, archs in enumerate((["Qwen3ForCausalLM"], None, [])):
        ok = str(tmp_path / f"ok{i}")
        qo.write_checkpoint(ok, shape, 5, body=False, config=dict(architectures=archs))
        assert read_encoder_config(ok)["desc"].qk_norm == 1


def test_the_fixture_tokenizer_runs_natively_and_qwens_own_pattern_goes_to_the_library(tmp_path, settings):
    import json

    from voitta_rag_amd.bpe import BpeTokenizer
    from voitta_rag_amd.embedding import NativeSentenceEncoder

    d = str(tmp_path / "m")
    qo.write_checkpoint(d, qo.Qwen3Shape(2, 128, 2, 1, 256, 64), 5, body=False)
    cfg = json.load(open(os.path.join(d, "config.json")))
    assert isinstance(NativeSentenceEncoder._load_tokenizer(d, cfg), BpeTokenizer)
    spec = json.load(open(os.path.join(d, "tokenizer.json"), encoding="utf-8"))
    qwen_split = {"type": "Split", "behavior": "Isolated", "invert": False, "pattern": {
        "Regex": r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+"}}
    spec["pre_tokenizer"] = {"type": "Sequence", "pretokenizers": [
        qwen_split, {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": False, "use_regex": False}]}
    json.dump(spec, open(os.path.join(d, "tokenizer.json"), "w", encoding="utf-8"))
    tok = NativeSentenceEncoder._load_tokenizer(d, cfg)
    assert not isinstance(tok, BpeTokenizer)
