"""ALiBi encoders (jina-embeddings-v2: model_type bert, position_embedding_type alibi) without a GPU: the slope
sequence against transformers' BLOOM, the f64 oracle tied to oracles that transformers goldens pin (oracle.bert with a
zero position table; tests/mpnet_oracle.py with the table -m_h |offset|), the state-dict mapping into the slots of
vr_encoder_load, the config reader, and the description's new position."""
import json
import logging
import os

import numpy as np
import pytest

import alibi_oracle as ao
import mpnet_oracle as mp
from oracle import bert as obert

HEAD_COUNTS = list(range(1, 17)) + [24]


# ---- the slopes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", HEAD_COUNTS)
def test_slopes_are_blooms(heads):
    """build_alibi_tensor returns slopes[h] * position as [heads, 1, S] (f32): with one sequence of two tokens the entry
    at position 1 is the slope itself. f32 on both sides. BLOOM rounds the base to f32 (relative error <= 2^-24) and
    raises it to a power p <= heads with torch.pow in f32 (the base's error p times over, and pow's own rounding, taken
    as <= 2^-23); alibi_slopes rounds the f64 value once (<= 2^-24): relative difference <= (heads + 3) 2^-24."""
    torch = pytest.importorskip("torch")
    bloom = pytest.importorskip("transformers.models.bloom.modeling_bloom")
    from voitta_rag_amd.encoder import alibi_slopes

    want = bloom.build_alibi_tensor(torch.ones(1, 2), heads, torch.float32)[:, 0, 1].numpy()
    got = alibi_slopes(heads)
    assert got.dtype == np.float32 and got.shape == (heads,)
    worst = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)) / want.astype(np.float64)))
    print(f"{heads} heads: worst relative difference {worst:.2e}")
    assert worst <= (heads + 3) * 2.0 ** -24, worst
    assert np.all(got > 0) and np.all(got < 1)


def test_slopes_by_their_definition():
    from voitta_rag_amd.encoder import alibi_slopes

    assert np.allclose(alibi_slopes(8), [2.0 ** -(i + 1) for i in range(8)], rtol=1e-7, atol=0)
    assert np.allclose(alibi_slopes(4), [2.0 ** -(2 * (i + 1)) for i in range(4)], rtol=1e-7, atol=0)
    six = alibi_slopes(6)  # 4 heads' sequence, then every second of 8 heads'
    assert np.allclose(six, [2.0 ** -2, 2.0 ** -4, 2.0 ** -6, 2.0 ** -8, 2.0 ** -1, 2.0 ** -3], rtol=1e-7, atol=0)
    with pytest.raises(ValueError):
        alibi_slopes(0)


# ---- the oracle against oracles that transformers goldens pin -----------------------------------------------------------
def _seqs(vocab, lens, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(4, vocab, size=n).astype(np.int32) for n in lens]


def test_gelu_oracle_without_slopes_is_the_bert_oracle_with_a_zero_position_table():
    shape = ao.AlibiShape(2, 128, 4, 256, ffn="gelu", max_pos=64)
    w = ao.random_weights(shape, 5)
    bert_shape = obert.BertShape(2, 128, 4, 256, vocab=shape.vocab, max_pos=64, type_vocab=shape.type_vocab, eps=shape.eps)
    wb = dict(w)
    wb["embeddings.position_embeddings.weight"] = np.zeros((64, 128), np.float32)
    for s in _seqs(shape.vocab, (1, 7, 33, 64), 6):
        for slopes in (None, np.zeros(4)):
            got, want = ao.encode_one(w, shape, s, slopes), obert.encode_one(wb, bert_shape, s)
            assert np.max(np.abs(got - want)) < 1e-12


@pytest.mark.parametrize("heads", [2, 6])
def test_gelu_oracle_with_slopes_is_the_mpnet_oracle_with_the_linear_table(heads):
    """Sequences of at most 513 tokens never reach past the radius-512 table -m_h |offset|: sign (the bias falls with
    the distance), symmetry (|j - i|) and head order are those of an oracle pinned by transformers' MPNet goldens."""
    H = 64 * heads
    shape = ao.AlibiShape(2, H, heads, 256, ffn="gelu", type_vocab=1, eps=1e-5)
    w = ao.random_weights(shape, 7)
    slopes = np.random.default_rng(8).uniform(0.05, 1.0, heads)
    mshape = mp.MpnetShape(2, H, heads, 256, vocab=shape.vocab, positions=515, eps=shape.eps)
    wm = {}
    for k, v in w.items():
        for a, b in (("attention.self.query", "attention.attn.q"), ("attention.self.key", "attention.attn.k"),
                     ("attention.self.value", "attention.attn.v"), ("attention.output.dense", "attention.attn.o"),
                     ("attention.output.LayerNorm", "attention.LayerNorm")):
            k = k.replace(a, b)
        wm[k] = v
    # MPNet has no token types: fold row 0 into a position table that is otherwise zero
    wm["embeddings.position_embeddings.weight"] = np.tile(w["embeddings.token_type_embeddings.weight"][0], (515, 1))
    table = -slopes[:, None] * np.abs(np.arange(-512, 513))[None, :]
    for s in _seqs(shape.vocab, (1, 2, 65, 513), 9):
        got, want = ao.encode_one(w, shape, s, slopes), mp.encode_one(wm, mshape, s, table)
        assert np.max(np.abs(got - want)) < 1e-11
    s = _seqs(shape.vocab, (40,), 10)[0]
    assert np.max(np.abs(ao.encode_one(w, shape, s, slopes) - ao.encode_one(w, shape, s, slopes[::-1]))) > 1e-3  # head order matters
    assert np.max(np.abs(ao.encode_one(w, shape, s, slopes) - ao.encode_one(w, shape, s, None))) > 1e-3


# ---- the state-dict mapping ---------------------------------------------------------------------------------------------
SLOT_SHAPE = ao.AlibiShape(2, 128, 2, 256)


@pytest.mark.parametrize("prefix", ["", "bert.", "0.auto_model."])
def test_state_dict_maps_onto_the_gated_slots(prefix):
    from voitta_rag_amd import encoder as enc

    w = ao.random_weights(SLOT_SHAPE, 11)
    state = {prefix + k: v for k, v in w.items()}
    state[prefix + "pooler.dense.weight"] = np.zeros((128, 128), np.float32)
    state[prefix + "pooler.dense.bias"] = np.zeros(128, np.float32)
    state[prefix + "embeddings.position_ids"] = np.arange(8192)[None]
    state["cls.predictions.bias"] = np.zeros(300, np.float32)
    desc = ao.desc_for(SLOT_SHAPE, "mean", "f32")
    names, out = enc.jina_slots(state, desc)
    assert len(names) == 5 + 18 * 2 and names[1] is None
    inter = SLOT_SHAPE.intermediate
    for i in range(2):
        per = names[5 + 18 * i:5 + 18 * (i + 1)]
        k = ao.layer_keys(i)
        gated = w[k["gated_w"]]
        assert per[11] is None and per[17] is None  # both FFN-up bias slots NULL
        assert np.array_equal(out[per[16]], gated[:inter])  # GATE: the first I rows, what the activation is applied to
        assert np.array_equal(out[per[10]], gated[inter:])  # UP
        assert out[per[12]] is w[k["f_w"]] and out[per[13]] is w[k["f_b"]]
        assert out[per[14]] is w[k["ln2_g"]] and out[per[15]] is w[k["ln2_b"]]
        for slot, short in ((0, "q_w"), (1, "q_b"), (2, "k_w"), (3, "k_b"), (4, "v_w"), (5, "v_b"), (6, "o_w"), (7, "o_b"),
                            (8, "ln1_g"), (9, "ln1_b")):
            assert out[per[slot]] is w[k[short]]
    assert not any("pooler" in n for n in out)
    for n in names:
        if n is not None:
            assert tuple(out[n].shape) == enc.expected_shape(desc, n), n


def test_other_tensors_are_refused_by_name():
    from voitta_rag_amd import encoder as enc

    w = ao.random_weights(SLOT_SHAPE, 11)
    desc = ao.desc_for(SLOT_SHAPE, "mean", "f32")
    qk = dict(w)
    qk["encoder.layer.0.attention.self.layer_norm_q.weight"] = np.ones(128, np.float32)
    with pytest.raises(ValueError, match=r"encoder\.layer\.0\.attention\.self\.layer_norm_q\.weight"):
        enc.jina_slots(qk, desc)
    missing = {k: v for k, v in w.items() if not k.endswith("layer.1.mlp.wo.bias")}
    with pytest.raises(KeyError, match=r"encoder\.layer\.1\.mlp\.wo\.bias"):
        enc.jina_slots(missing, desc)
    wrong = dict(w)
    wrong["encoder.layer.0.mlp.gated_layers.weight"] = w["encoder.layer.0.mlp.gated_layers.weight"][:-1]
    with pytest.raises(ValueError, match="gated_layers"):
        enc.jina_slots(wrong, desc)


def test_load_encoder_sets_the_slopes_after_the_load():
    import ctypes as C

    from voitta_rag_amd import encoder as enc

    w = ao.random_weights(SLOT_SHAPE, 11)
    calls = []

    class Lib:
        @staticmethod
        def vr_encoder_load(handle, desc, arr, n, mem):
            d = C.cast(desc, C.POINTER(enc._lib.VrBertDesc)).contents
            calls.append(("load", n, d.position, d.ffn, arr[1], arr[5 + 11], arr[5 + 17]))
            return 0

    class FakeEngine:
        handle, _lib = None, Lib

        def set_attention_slopes(self, slopes):
            calls.append(("slopes", tuple(slopes.shape)))

    enc.load_encoder(FakeEngine(), ao.desc_for(SLOT_SHAPE, "mean", "f32", attention_slopes=enc.alibi_slopes(2)), w)
    assert calls == [("load", 5 + 18 * 2, enc._lib.VR_POS_NONE, enc._lib.VR_FFN_GEGLU, None, None, None), ("slopes", (2,))]
    del calls[:]
    enc.load_encoder(FakeEngine(), ao.desc_for(SLOT_SHAPE, "mean", "f32"), w)
    assert [c[0] for c in calls] == ["load"]
    # a GELU description without positions: a BERT state dict, the position slot NULL
    gelu = ao.AlibiShape(2, 128, 2, 256, ffn="gelu")
    del calls[:]
    enc.load_encoder(FakeEngine(), ao.desc_for(gelu, "mean", "f32"), ao.random_weights(gelu, 12))
    assert calls[0][:5] == ("load", 5 + 16 * 2, enc._lib.VR_POS_NONE, enc._lib.VR_FFN_GELU, None)


# ---- the description ----------------------------------------------------------------------------------------------------
def test_position_none_crosses_the_abi_as_vr_pos_none():
    from voitta_rag_amd import _lib
    from voitta_rag_amd import encoder as enc

    assert _lib.VR_POS_NONE == 2
    assert enc.BertDesc(2, 128, 2, 256, position="none").to_c().position == _lib.VR_POS_NONE
    a = enc.BertDesc(2, 128, 2, 256, position="none")
    b = enc.BertDesc(2, 128, 2, 256, position="none", attention_slopes=enc.alibi_slopes(2))
    assert a == b  # the slopes are no part of the comparison, as the bias table is not
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "voitta_engine.h")).read()
    assert "#define VR_POS_NONE    2" in header and "vr_encoder_set_attention_slopes" in header
    assert "vr_encoder_set_attention_slopes" in _lib.SIGNATURES
    from voitta_rag_amd import Engine

    assert callable(Engine.set_attention_slopes)


# ---- the config reader --------------------------------------------------------------------------------------------------
JINA_BASE = {"architectures": ["JinaBertForMaskedLM"], "model_type": "bert", "position_embedding_type": "alibi",
             "feed_forward_type": "geglu", "hidden_act": "gelu", "hidden_size": 768, "num_hidden_layers": 12,
             "num_attention_heads": 12, "intermediate_size": 3072, "vocab_size": 30528, "max_position_embeddings": 8192,
             "type_vocab_size": 2, "layer_norm_eps": 1e-12, "emb_pooler": "mean", "pad_token_id": 0}


def _dir(tmp_path, cfg, max_seq=None, pooling="mean", normalize=True):
    d = tmp_path / f"m{len(list(tmp_path.iterdir()))}"
    os.makedirs(d / "1_Pooling")
    json.dump(cfg, open(d / "config.json", "w"))
    mods = [{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
            {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"}]
    if normalize:
        mods.append({"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"})
    json.dump(mods, open(d / "modules.json", "w"))
    json.dump({"pooling_mode_cls_token": pooling == "cls", "pooling_mode_mean_tokens": pooling == "mean"},
              open(d / "1_Pooling" / "config.json", "w"))
    if max_seq:
        json.dump({"max_seq_length": max_seq}, open(d / "sentence_bert_config.json", "w"))
    return str(d)


@pytest.fixture
def cap(monkeypatch):
    from voitta_rag_amd import config

    def set_cap(value):
        if value is None:
            monkeypatch.delenv("VOITTA_MAX_SEQ_LENGTH", raising=False)
        else:
            monkeypatch.setenv("VOITTA_MAX_SEQ_LENGTH", str(value))
        config.get_settings.cache_clear()

    yield set_cap
    monkeypatch.delenv("VOITTA_MAX_SEQ_LENGTH", raising=False)
    config.get_settings.cache_clear()


def test_config_reader_describes_jina_v2_base(tmp_path, monkeypatch, cap, caplog):
    from voitta_rag_amd.embedding import read_encoder_config
    from voitta_rag_amd.encoder import alibi_slopes

    monkeypatch.delenv("VOITTA_ENCODER_PRECISION", raising=False)
    cap(None)
    with caplog.at_level(logging.WARNING, logger="voitta_rag_amd.embedding"):
        rc = read_encoder_config(_dir(tmp_path, JINA_BASE, max_seq=8192))
    assert "truncated to 512 tokens" in caplog.text and "VOITTA_MAX_SEQ_LENGTH" in caplog.text
    d = rc["desc"]
    assert (d.layers, d.hidden, d.heads, d.intermediate, d.vocab) == (12, 768, 12, 3072, 30528)
    assert (d.position, d.ffn, d.norm, d.window, d.precision) == ("none", "geglu", "post", 0, "f16")
    assert (d.max_pos, d.type_vocab, d.eps, d.pooling, d.normalize) == (512, 2, 1e-12, "mean", True)
    assert d.attention_bias is None and np.array_equal(d.attention_slopes, alibi_slopes(12))
    assert (rc["pos_start"], rc["max_seq"]) == (0, 512)
    cap(2048)  # the cap is honoured ...
    rc = read_encoder_config(_dir(tmp_path, JINA_BASE, max_seq=8192))
    assert (rc["max_seq"], rc["desc"].max_pos) == (2048, 2048)
    cap(8192)
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="voitta_rag_amd.embedding"):
        rc = read_encoder_config(_dir(tmp_path, JINA_BASE, max_seq=8192, pooling="cls", normalize=False))
    assert (rc["max_seq"], rc["desc"].max_pos, rc["desc"].pooling, rc["desc"].normalize) == (8192, 8192, "cls", False)
    assert "truncated" not in caplog.text
    rc = read_encoder_config(_dir(tmp_path, JINA_BASE, max_seq=1024))  # ... and so is max_seq_length below it
    assert rc["max_seq"] == 1024
    rc = read_encoder_config(_dir(tmp_path, dict(JINA_BASE, max_position_embeddings=4096, type_vocab_size=1), max_seq=8192))
    assert (rc["max_seq"], rc["desc"].type_vocab) == (4096, 1)
    small = dict(JINA_BASE, hidden_size=512, num_hidden_layers=4, num_attention_heads=8, intermediate_size=2048)
    assert np.array_equal(read_encoder_config(_dir(tmp_path, small))["desc"].attention_slopes, alibi_slopes(8))


def test_config_reader_refusals(tmp_path, cap):
    from voitta_rag_amd.embedding import read_encoder_config

    cap(None)
    with pytest.raises(ValueError, match="feed_forward_type 'original' is not implemented"):
        read_encoder_config(_dir(tmp_path, dict(JINA_BASE, feed_forward_type="original")))
    with pytest.raises(ValueError, match="hidden_act 'relu' is not implemented"):
        read_encoder_config(_dir(tmp_path, dict(JINA_BASE, hidden_act="relu")))
    # what is not an alibi model is refused as before
    with pytest.raises(ValueError, match="only exact-erf GELU and absolute position embeddings are implemented"):
        read_encoder_config(_dir(tmp_path, dict(JINA_BASE, position_embedding_type="relative_key")))
