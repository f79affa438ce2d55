"""T5 encoders (gtr-t5, sentence-t5) on the CPU: the oracle against transformers' goldens, the bias table against the
library's compute_bias, the loader on a synthetic gtr-t5-style directory, the description across the C ABI, and the
native Unigram tokenizer's "$A </s>" template against ids recorded from the tokenizers library."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import mpnet_oracle as mp
import t5_oracle as t5

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = {name: os.path.join(HERE, "golden", f"t5_{name}.npz") for name in ("tiny_d64", "tiny_d32")}


def _case(path):
    z = np.load(path)
    layers, hidden, heads, inter, vocab, buckets, max_distance = (int(v) for v in z["shape"])
    shape = t5.T5Shape(layers, hidden, heads, inter, vocab=vocab, eps=float(z["eps"]), buckets=buckets, max_distance=max_distance)
    off = z["offsets"]
    seqs = [z["ids"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    return shape, str(z["pooling"]), int(z["seed"]), seqs, z


@pytest.fixture(scope="module")
def cases():
    return {name: _case(path) for name, path in GOLDEN.items()}


# ---- goldens and oracle -------------------------------------------------------------------------------------------------
def test_goldens_hold_the_listed_cases(cases):
    shape, pooling, _, seqs, _ = cases["tiny_d64"]
    assert (shape.layers, shape.hidden, shape.heads, shape.intermediate, pooling) == (2, 128, 2, 256, "mean")
    shape32, pooling32, _, seqs32, _ = cases["tiny_d32"]
    assert (shape32.heads, shape32.d_kv, pooling32) == (4, 32, "cls")
    for s in (seqs, seqs32):
        lens = [len(x) for x in s]
        assert 1 in lens and max(lens) > 130 + shape.max_distance  # offsets pass the saturation point in both directions


def test_oracle_reproduces_transformers(cases):
    """`want` is T5EncoderModel in f64 throughout, everything f64 on both sides and the bias values the same f32
    numbers: 1e-9 max-abs on unit embeddings, the bound test_mpnet_cpu holds the MPNet oracle to. `want_lib` is the
    library exactly as it is, whose T5LayerNorm rounds every row's variance to f32 whatever the model's dtype: five
    norms in a row, each off by a relative 2^-24 rounding and an f32 mean of 128 squares (a few 2^-24 more), i.e. a
    relative error of a few 1e-7 per norm, mostly a common factor of the row that the final normalisation removes:
    1e-6 bounds what is left on unit embeddings (measured 1.8e-8 and 2.6e-8)."""
    for name, (shape, pooling, seed, seqs, z) in cases.items():
        got = t5.sentence_embeddings(t5.random_weights(shape, seed), shape, seqs, pooling)
        worst, worst_lib = float(np.max(np.abs(got - z["want"]))), float(np.max(np.abs(got - z["want_lib"])))
        print(f"{name}: oracle vs transformers max-abs {worst:.2e}; vs the library's f32 variances {worst_lib:.2e}")
        assert worst < 1e-9
        assert worst_lib < 1e-6


def test_goldens_see_a_dropped_bias_and_a_scaled_logit(cases):
    """What the engine could get wrong: no table, and the 1/sqrt(d_kv) T5 does not have (a query weight left unfolded)."""
    for name, (shape, pooling, seed, seqs, z) in cases.items():
        w = t5.random_weights(shape, seed)
        assert np.max(np.abs(t5.sentence_embeddings(w, shape, seqs, pooling, table=None) - z["want"])) > 1e-2
        scaled = dict(w)
        for i in range(shape.layers):
            scaled[t5.layer_keys(i)["q"]] = w[t5.layer_keys(i)["q"]] / np.float32(np.sqrt(shape.d_kv))
        assert np.max(np.abs(t5.sentence_embeddings(scaled, shape, seqs, pooling) - z["want"])) > 1e-2


def test_bias_table_is_the_librarys_bias_at_every_offset(cases):
    from voitta_rag_amd.encoder import t5_bias_table

    for name, (shape, _, seed, _, z) in cases.items():
        w = t5.random_weights(shape, seed)
        want = z["offset_bias"]  # [heads, 1201]: key - query = -600 .. 600
        assert want.shape == (shape.heads, 1201) and want.dtype == np.float32
        table = t5_bias_table(w[t5.BIAS_KEY], shape.buckets, shape.max_distance)
        R = shape.max_distance
        assert table.shape == (shape.heads, 2 * R + 1) and table.dtype == np.float32
        d = np.arange(-600, 601)
        assert np.array_equal(table[:, np.clip(d, -R, R) + R], want)  # bit for bit, the clamp included
        assert np.array_equal(t5.table_from_buckets(w[t5.BIAS_KEY], shape), table.astype(np.float64))


def test_bias_table_follows_the_configs_buckets_and_distance():
    from voitta_rag_amd.encoder import t5_bias_table

    rng = np.random.default_rng(3)
    for buckets, dist in ((32, 128), (16, 64), (32, 512), (8, 20)):
        wt = rng.normal(0, 1, (buckets, 3)).astype(np.float32)
        table = t5_bias_table(wt, buckets, dist)
        shape = t5.T5Shape(1, 192, 3, 256, buckets=buckets, max_distance=dist)
        assert table.shape == (3, 2 * dist + 1)
        assert np.array_equal(table.astype(np.float64), t5.table_from_buckets(wt, shape))
        far = mp.bucket(np.array([dist, dist + 1, 5 * dist, -dist, -dist - 1, -5 * dist]), buckets, dist)
        assert len(set(far[:3])) == 1 and len(set(far[3:])) == 1  # constant from |d| = max_distance on
    with pytest.raises(ValueError, match="relative_attention_num_buckets"):
        t5_bias_table(np.zeros((32, 2), np.float32), 16, 128)
    with pytest.raises(ValueError, match="radius of 1..512"):
        t5_bias_table(np.zeros((32, 2), np.float32), 32, 513)


# ---- the description ----------------------------------------------------------------------------------------------------
def test_rms_pre_relu_cross_the_abi():
    """(fails without the feature: "unknown norm placement 'rms_pre'")"""
    from voitta_rag_amd import _lib
    from voitta_rag_amd import encoder as enc

    assert (_lib.VR_NORM_PRE_RMS, _lib.VR_FFN_RELU) == (2, 3)
    d = enc.BertDesc(2, 128, 2, 256, norm="rms_pre", ffn="relu", position="none")
    c = d.to_c()
    assert (c.norm, c.ffn, c.position, c.window) == (_lib.VR_NORM_PRE_RMS, _lib.VR_FFN_RELU, _lib.VR_POS_NONE, 0)
    assert d.rms and not d.prenorm and not d.gated and not d.rotary
    assert not enc.BertDesc(2, 128, 2, 256).rms
    with pytest.raises(ValueError, match="unknown norm placement"):
        enc.BertDesc(2, 128, 2, 256, norm="rms").to_c()
    header = open(os.path.join(os.path.dirname(HERE), "include", "voitta_engine.h")).read()
    assert "#define VR_NORM_PRE_RMS 2" in header and "#define VR_FFN_RELU   3" in header
    assert "sqrt(d_h)" in header  # the missing logit scale is said there


# ---- the state-dict mapping ---------------------------------------------------------------------------------------------
SLOT_SHAPE = t5.T5Shape(2, 128, 4, 256)


@pytest.mark.parametrize("prefix", ["", "0.auto_model."])
def test_state_dict_maps_onto_the_slots(prefix):
    from voitta_rag_amd import encoder as enc

    w = t5.random_weights(SLOT_SHAPE, 11)
    state = {prefix + k: v for k, v in w.items()}
    state[prefix + "encoder.embed_tokens.weight"] = w[t5.WORD_KEY]
    desc = t5.desc_for(SLOT_SHAPE, "mean", "f32")
    names, out, table = enc.t5_slots(state, desc)
    assert len(names) == 5 + 16 * 2
    assert names[1] is None and names[2] is None and names[4] is None  # no positions, no token types, no shift
    assert np.array_equal(out[names[0]], w[t5.WORD_KEY])
    assert np.array_equal(out[names[3]], w[t5.layer_keys(0)["ln_a"]])  # embeddings.LayerNorm = block 0's attention norm
    for i in range(2):
        per, k = names[5 + 16 * i:5 + 16 * (i + 1)], t5.layer_keys(i)
        assert all(per[j] is None for j in range(1, 16, 2))  # every bias slot NULL
        # the fold: q.weight * sqrt(d_kv), one f32 rounding per weight at d_kv = 32
        assert np.array_equal(out[per[0]], (w[k["q"]] * np.sqrt(np.float32(32))).astype(np.float32))
        assert out[per[0]].dtype == np.float32
        for slot, short in ((2, "k"), (4, "v"), (6, "o"), (8, "ln_m"), (10, "wi"), (12, "wo")):
            assert np.array_equal(out[per[slot]], w[k[short]]), short
        nxt = w[t5.layer_keys(1)["ln_a"]] if i == 0 else w[t5.FINAL_KEY]
        assert np.array_equal(out[per[14]], nxt)  # block l + 1's attention norm, the final norm for the last
    for n in names:
        if n is not None:
            assert tuple(out[n].shape) == enc.expected_shape(desc, n), n
    assert np.array_equal(table, enc.t5_bias_table(w[t5.BIAS_KEY], 32, 128))


def test_the_fold_is_exactly_times_eight_at_head_size_64():
    from voitta_rag_amd import encoder as enc

    shape = t5.T5Shape(1, 128, 2, 256)
    w = t5.random_weights(shape, 12)
    names, out, _ = enc.t5_slots(dict(w), t5.desc_for(shape, "mean", "f32"))
    q = w[t5.layer_keys(0)["q"]]
    assert np.array_equal(out[names[5]], q * np.float32(8.0)) and np.array_equal(out[names[5]] / np.float32(8.0), q)


def test_missing_tensors_are_named():
    from voitta_rag_amd import encoder as enc

    w = t5.random_weights(SLOT_SHAPE, 11)
    desc = t5.desc_for(SLOT_SHAPE, "mean", "f32")
    for gone in (t5.layer_keys(1)["wo"], t5.FINAL_KEY, t5.BIAS_KEY):
        with pytest.raises(KeyError, match=gone.replace(".", r"\.")):
            enc.t5_slots({k: v for k, v in w.items() if k != gone}, desc)
    decoder_only = {"decoder." + k[len("encoder."):]: v for k, v in w.items() if k.startswith("encoder.")}
    decoder_only[t5.WORD_KEY] = w[t5.WORD_KEY]
    with pytest.raises(KeyError, match="no T5 encoder weights"):
        enc.t5_slots(decoder_only, desc)


def test_load_encoder_passes_null_slots_and_sets_the_table():
    from voitta_rag_amd import encoder as enc

    w = t5.random_weights(SLOT_SHAPE, 11)
    calls = []

    class Lib:
        @staticmethod
        def vr_encoder_load(handle, desc, arr, n, mem):
            d = C.cast(desc, C.POINTER(enc._lib.VrBertDesc)).contents
            calls.append(("load", n, d.position, d.ffn, d.norm, [i for i in range(n) if arr[i] is None]))
            return 0

    class FakeEngine:
        handle, _lib = None, Lib

        def set_attention_bias(self, table):
            calls.append(("bias", tuple(table.shape)))

    enc.load_encoder(FakeEngine(), t5.desc_for(SLOT_SHAPE, "mean", "f32"), w)
    null = [1, 2, 4] + [5 + 16 * l + j for l in range(2) for j in range(1, 16, 2)]
    assert calls == [("load", 5 + 16 * 2, enc._lib.VR_POS_NONE, enc._lib.VR_FFN_RELU, enc._lib.VR_NORM_PRE_RMS, null),
                     ("bias", (4, 257))]
    del calls[:]  # a table on the description wins over the checkpoint's
    enc.load_encoder(FakeEngine(), t5.desc_for(SLOT_SHAPE, "mean", "f32", attention_bias=np.zeros((4, 3), np.float32)), w)
    assert calls[1] == ("bias", (4, 3))
    del calls[:]  # ... and the checkpoint's is then not built (16 buckets: t5_slots' defaults would refuse it)
    w16 = dict(w, **{t5.BIAS_KEY: w[t5.BIAS_KEY][:16]})
    enc.load_encoder(FakeEngine(), t5.desc_for(SLOT_SHAPE, "mean", "f32", attention_bias=enc.t5_bias_table(w16[t5.BIAS_KEY], 16, 64)), w16)
    assert calls[1] == ("bias", (4, 129))


# ---- the directory reader -----------------------------------------------------------------------------------------------
def test_config_reader_describes_a_gtr_t5_directory(tmp_path, monkeypatch):
    from voitta_rag_amd.embedding import read_encoder_config

    monkeypatch.delenv("VOITTA_ENCODER_PRECISION", raising=False)
    shape = t5.T5Shape(12, 768, 12, 3072, vocab=32128)  # gtr-t5-base
    d = str(tmp_path / "gtr")
    t5.write_checkpoint(d, shape, 5, max_seq=512, body=False)
    rc = read_encoder_config(d)
    desc = rc["desc"]
    assert (desc.layers, desc.hidden, desc.heads, desc.intermediate, desc.vocab) == (12, 768, 12, 3072, 32128)
    assert (desc.norm, desc.ffn, desc.position, desc.window, desc.type_vocab) == ("rms_pre", "relu", "none", 0, 1)
    assert (desc.max_pos, rc["max_seq"], desc.eps, desc.pooling, desc.normalize) == (512, 512, 1e-6, "mean", True)
    assert (rc["buckets"], rc["max_distance"], desc.precision) == (32, 128, "f16")
    assert len(desc.head) == 1 and desc.head[0].kind == "dense" and desc.head[0].bias is None
    assert desc.head[0].activation == "identity" and desc.out_dim == 768
    assert np.array_equal(desc.head[0].weight, t5.dense_weight(shape, 5))


@pytest.fixture
def seq_cap_setting(monkeypatch):
    """Sets VOITTA_MAX_SEQ_LENGTH for get_settings(), which caches: dropped on every change and when the test ends."""
    from voitta_rag_amd import config

    def set_cap(value):
        monkeypatch.setenv("VOITTA_MAX_SEQ_LENGTH", str(value))
        config.get_settings.cache_clear()

    yield set_cap
    config.get_settings.cache_clear()


def test_max_seq_is_bounded_by_the_setting_alone(tmp_path, seq_cap_setting):
    from voitta_rag_amd.embedding import read_encoder_config

    shape = t5.T5Shape(2, 128, 2, 256)
    d = str(tmp_path / "long")
    t5.write_checkpoint(d, shape, 5, max_seq=3000, body=False)
    seq_cap_setting(2048)
    rc = read_encoder_config(d)
    assert rc["max_seq"] == 2048 and rc["desc"].max_pos == 2048  # no position table: nothing else bounds it
    seq_cap_setting(4096)
    assert read_encoder_config(d)["max_seq"] == 3000


@pytest.mark.parametrize("over, message", [
    (dict(feed_forward_proj="gated-gelu"), "gated-gelu"),
    (dict(feed_forward_proj="gated-silu"), "feed_forward_proj 'gated-silu'"),
    (dict(num_heads=3), r"num_heads \* d_kv = 3 \* 64 != d_model = 128"),
    (dict(num_heads=1, d_kv=128), "d_kv 128"),
    (dict(num_heads=8, d_kv=16), "d_kv 16"),
    (dict(relative_attention_max_distance=600), "relative_attention_max_distance 600 > 512"),
])
def test_config_reader_refusals(tmp_path, over, message):
    from voitta_rag_amd.embedding import read_encoder_config

    d = str(tmp_path / "m")
    t5.write_checkpoint(d, t5.T5Shape(2, 128, 2, 256), 5, body=False, config=over)
    with pytest.raises(ValueError, match=message):
        read_encoder_config(d)


def test_unsupported_model_types_list_t5(tmp_path):
    from voitta_rag_amd.embedding import read_encoder_config

    d = str(tmp_path / "m")
    t5.write_checkpoint(d, t5.T5Shape(2, 128, 2, 256), 5, body=False, config=dict(model_type="mt5"))
    with pytest.raises(ValueError, match="unsupported model_type mt5: .*T5"):
        read_encoder_config(d)


# ---- the tokenizer ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tok_fixture():
    return t5.tokenizer_fixture()


def test_golden_tokenizer_is_in_t5s_layout(tok_fixture):
    spec, cases = tok_fixture["tokenizer"], tok_fixture["cases"]
    vocab = [p for p, _ in spec["model"]["vocab"]]
    assert vocab[:3] == ["<pad>", "</s>", "<unk>"] and vocab[-2:] == ["<extra_id_1>", "<extra_id_0>"]
    assert spec["model"]["type"] == "Unigram" and spec["model"]["unk_id"] == 2
    assert spec["normalizer"]["type"] == "Precompiled" and spec["pre_tokenizer"]["type"] == "Metaspace"
    assert [list(i)[0] for i in spec["post_processor"]["single"]] == ["Sequence", "SpecialToken"]
    texts = {c["text"] for c in cases}
    assert "" in texts and "<extra_id_0>" in texts and any("ﬁ" in t for t in texts)
    assert sum(c["max_len"] == 12 for c in cases) >= 3


def test_native_tokenizer_gives_the_recorded_ids(tok_fixture):
    """(fails without the feature: the template $A </s> is refused)"""
    from voitta_rag_amd.unigram import UnigramTokenizer

    tok = UnigramTokenizer.from_tokenizer_json(tok_fixture["tokenizer"])
    assert tok.bos_id == -1
    for max_len in sorted({c["max_len"] for c in tok_fixture["cases"]}):
        tok.max_length = max_len
        group = [c for c in tok_fixture["cases"] if c["max_len"] == max_len]
        ids, off = tok.encode_batch([c["text"] for c in group])
        for i, c in enumerate(group):
            assert ids[off[i]:off[i + 1]].tolist() == c["ids"], (c["text"][:40], max_len)
            assert c["ids"][-1] == 1 and len(c["ids"]) <= max_len  # </s> survives the truncation
    tok.max_length = 512
    ids, off = tok.encode_batch([""])
    assert ids.tolist() == [1]


def test_encode_pairs_is_refused_and_the_xlmr_template_still_parses(tok_fixture):
    from voitta_rag_amd.unigram import UnigramTokenizer, parse_tokenizer_json

    tok = UnigramTokenizer.from_tokenizer_json(tok_fixture["tokenizer"])
    with pytest.raises(ValueError, match=r"\$A </s>"):
        tok.encode_pairs(["a"], ["b"])
    lib = tok._lib  # the C call refuses it too
    needed = C.c_int64()
    off = np.zeros(2, np.int64)
    a = (C.c_char_p * 1)(b"a")
    n1 = np.ones(1, np.int64)
    p64 = C.POINTER(C.c_int64)
    rc = lib.vr_unigram_encode_pairs(tok._h, a, n1.ctypes.data_as(p64), a, n1.ctypes.data_as(p64), 1, 16,
                                     off.ctypes.data_as(p64), None, None, 0, C.byref(needed))
    assert rc != 0 and b"$A </s>" in lib.vr_last_error()
    xlmr = json.load(open(os.path.join(HERE, "golden", "xlmr_tokenizer.json"), encoding="utf-8"))["tokenizer"]
    assert parse_tokenizer_json(xlmr)["bos_id"] == 0
    broken = json.loads(json.dumps(tok_fixture["tokenizer"]))
    broken["post_processor"]["single"] = broken["post_processor"]["single"][::-1]  # </s> $A
    with pytest.raises(ValueError, match="post-processor template"):
        parse_tokenizer_json(broken)


def test_a_t5_directory_gets_the_native_tokenizer(tmp_path):
    from voitta_rag_amd.embedding import NativeSentenceEncoder, native_tokenizer
    from voitta_rag_amd.unigram import UnigramTokenizer

    d = str(tmp_path / "m")
    t5.write_checkpoint(d, t5.T5Shape(2, 128, 2, 256), 5, body=False)
    tok = NativeSentenceEncoder._load_tokenizer(d, {"model_type": "t5"})
    assert isinstance(tok, UnigramTokenizer) and native_tokenizer(tok) and tok.bos_id == -1
