"""Pre-norm, sliding-window encoders (model_type modernbert) without a GPU: the f64 oracle against the transformers
goldens, config detection in both spellings and its refusals, the state-dict mapping into the slots of vr_encoder_load,
and the description's new fields."""
import glob
import json
import logging
import os

import numpy as np
import pytest

import modernbert_oracle as mo

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "modernbert_*.npz")))
SHORT = [p for p in GOLDEN if "tiny" in p]
LENS = {"modernbert_tiny_w8.npz": [1, 2, 8, 9, 10, 16, 17, 18, 63, 64, 65, 129, 193, 257, 512],
        "modernbert_tiny_w64.npz": [1, 64, 65, 66, 128, 129, 130, 193, 257, 512],
        "modernbert_long_d64.npz": [1, 641, 705, 1025, 2049, 8192],
        "modernbert_long_d32.npz": [1, 1281, 2049, 8192]}


def load_case(path):
    g = np.load(path)
    L, H, nh, inter, vocab, max_pos = (int(x) for x in g["shape"])
    shape = mo.ModernShape(L, H, nh, inter, vocab=vocab, max_pos=max_pos, eps=float(g["eps"]), theta=float(g["theta"]),
                           theta_local=float(g["theta_local"]), window=int(g["window"]), global_every=int(g["global_every"]))
    seqs = [g["ids"][g["offsets"][i]:g["offsets"][i + 1]] for i in range(len(g["offsets"]) - 1)]
    return g, shape, str(g["pooling"]), int(g["seed"]), seqs, g["want"]


def test_goldens_cover_the_listed_shapes_and_lengths():
    assert sorted(os.path.basename(p) for p in GOLDEN) == sorted(LENS)
    cases = {os.path.basename(p): load_case(p) for p in GOLDEN}
    for name, (g, shape, _, _, seqs, want) in cases.items():
        assert [len(s) for s in seqs] == LENS[name] and want.dtype == np.float64 and want.shape == (len(seqs), shape.hidden)
        assert all("weight" not in k for k in g.files)  # no weights are stored
        assert os.path.getsize(os.path.join(HERE, "golden", name)) < 300_000
        assert shape.global_every == 3 and (shape.theta, shape.theta_local) == (160000.0, 10000.0)
    s = cases["modernbert_tiny_w8.npz"]
    assert (s[1].layers, s[1].hidden, s[1].heads, s[1].intermediate, s[1].window, s[2]) == (4, 128, 2, 256, 8, "mean")
    assert [mo.is_global(s[1], i) for i in range(4)] == [True, False, False, True]
    s = cases["modernbert_tiny_w64.npz"]
    assert (s[1].layers, s[1].hidden, s[1].heads, s[1].intermediate, s[1].window, s[2]) == (3, 128, 4, 384, 64, "cls")
    s = cases["modernbert_long_d64.npz"]
    assert (s[1].layers, s[1].hidden // s[1].heads, s[1].window, s[1].max_pos) == (3, 64, 64, 8192)
    s = cases["modernbert_long_d32.npz"]
    assert (s[1].layers, s[1].hidden // s[1].heads, s[1].window, s[1].max_pos) == (3, 32, 64, 8192)


@pytest.mark.parametrize("path", SHORT, ids=lambda p: os.path.basename(p))
def test_oracle_reproduces_transformers(path):
    """With the f32 tables the golden recorded, and the two f32 roundings of transformers' eager path restated
    (modernbert_oracle's library_f32): 1e-9 max-abs on unit embeddings, test_rope_cpu's bound for the same comparison
    (measured 1.4e-16). The plain f64 oracle with exact tables, which the GPU tests compare against, differs from the
    library by those roundings: f32 tables (3e-5 rad at position 511), queries and keys rounded to f32 (2^-24 relative)
    and f32 probabilities (2^-24 relative), on unit embeddings whose entries are below 1 — held to 1e-7, ten times the
    3.4e-8 rope_oracle measured for its table alone (measured here: 1.3e-8 and 2.5e-9)."""
    g, shape, pooling, seed, seqs, want = load_case(path)
    half = shape.hidden // shape.heads // 2
    tables = ((g["rope_cos"], g["rope_sin"]), (g["rope_cos_local"], g["rope_sin_local"]))
    for (cos, sin), theta in zip(tables, (shape.theta, shape.theta_local)):
        assert cos.dtype == np.float32 and cos.shape == (512, half)
        exact = mo.rope_table(512, 2 * half, theta)
        assert np.abs(cos - exact[0]).max() < 1e-4 and np.abs(sin - exact[1]).max() < 1e-4  # it IS that table, in f32
    w = mo.random_weights(shape, seed)
    pinned = mo.sentence_embeddings(w, shape, seqs, pooling, True, tables=tables, library_f32=True)
    exact = mo.sentence_embeddings(w, shape, seqs, pooling, True)
    worst, worst_exact = float(np.max(np.abs(pinned - want))), float(np.max(np.abs(exact - want)))
    print(f"{os.path.basename(path)}: oracle vs transformers f64, max-abs {worst:.3e} pinned, {worst_exact:.3e} exact tables")
    assert worst < 1e-9
    assert worst_exact < 1e-7


def test_the_window_is_inclusive_on_both_sides():
    """Perturbing token 30 of a 64-token sequence changes rows 30 - w .. 30 + w of one windowed layer and no other."""
    for w_half in (8, 3):
        shape = mo.ModernShape(2, 128, 2, 256, window=w_half, global_every=2)  # layer 1 is the windowed one
        w = mo.random_weights(shape, 5)
        k0 = mo.layer_keys(0, 2)
        for name in (k0["qkv_w"], k0["o_w"], k0["wi_w"], k0["wo_w"]):
            w[name] = np.zeros_like(w[name])  # layer 0 passes its input through: what remains mixes tokens in layer 1 only
        rng = np.random.default_rng(1)
        a = rng.integers(0, shape.vocab, size=64)
        b = a.copy()
        b[30] = (b[30] + 1) % shape.vocab
        changed = np.flatnonzero(np.abs(mo.encode_one(w, shape, a) - mo.encode_one(w, shape, b)).max(axis=1) > 0)
        assert changed.tolist() == list(range(30 - w_half, 30 + w_half + 1))


# ---- config detection --------------------------------------------------------------------------------------------------
NEW = {"architectures": ["ModernBertModel"], "model_type": "modernbert", "hidden_size": 768, "num_hidden_layers": 22,
       "num_attention_heads": 12, "intermediate_size": 1152, "vocab_size": 50368, "max_position_embeddings": 8192,
       "norm_eps": 1e-5, "hidden_activation": "gelu", "local_attention": 128, "global_attn_every_n_layers": 3,
       "layer_types": ["full_attention" if i % 3 == 0 else "sliding_attention" for i in range(22)],
       "rope_parameters": {"full_attention": {"rope_type": "default", "rope_theta": 160000.0},
                           "sliding_attention": {"rope_type": "default", "rope_theta": 10000.0}}}
OLD = {k: v for k, v in NEW.items() if k not in ("rope_parameters", "layer_types")} | {"global_rope_theta": 160000.0,
                                                                                        "local_rope_theta": 10000.0}


def _dir(tmp_path, cfg, max_seq=None, pooling="mean"):
    d = tmp_path / f"m{len(list(tmp_path.iterdir()))}"
    (d / "1_Pooling").mkdir(parents=True)
    (d / "config.json").write_text(json.dumps(cfg))
    (d / "modules.json").write_text(json.dumps([
        {"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
        {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
        {"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}]))
    (d / "1_Pooling" / "config.json").write_text(json.dumps({"pooling_mode_cls_token": pooling == "cls",
                                                               "pooling_mode_mean_tokens": pooling == "mean"}))
    if max_seq is not None:
        (d / "sentence_bert_config.json").write_text(json.dumps({"max_seq_length": max_seq}))
    return str(d)


@pytest.mark.parametrize("cfg", [NEW, OLD], ids=["rope_parameters", "global_rope_theta"])
def test_both_config_spellings_give_the_same_description(tmp_path, cfg):
    from voitta_rag_amd import _lib
    from voitta_rag_amd.embedding import read_encoder_config

    rc = read_encoder_config(_dir(tmp_path, cfg, max_seq=256, pooling="cls"))
    d = rc["desc"]
    assert (d.layers, d.hidden, d.heads, d.intermediate, d.vocab, d.type_vocab) == (22, 768, 12, 1152, 50368, 1)
    assert (d.position, d.ffn, d.norm, d.pooling, d.normalize, d.eps) == ("rotary", "geglu", "pre", "cls", True, 1e-5)
    assert (d.rope_theta, d.rope_theta_local, d.window, d.global_every) == (160000.0, 10000.0, 64, 3)
    assert rc["max_seq"] == 256 and d.max_pos == 256 and rc["pos_start"] == 0 and d.prenorm
    c = d.to_c()
    assert (c.norm, c.window, c.global_every, c.rope_theta_local) == (_lib.VR_NORM_PRE, 64, 3, 10000.0)
    assert (c.position, c.ffn, c.rope_theta) == (_lib.VR_POS_ROTARY, _lib.VR_FFN_GEGLU, 160000.0)


def test_theta_defaults_other_thetas_and_all_global_models(tmp_path):
    from voitta_rag_amd.embedding import read_encoder_config

    bare = {k: v for k, v in OLD.items() if not k.endswith("rope_theta")}
    d = read_encoder_config(_dir(tmp_path, bare, max_seq=64))["desc"]
    assert (d.rope_theta, d.rope_theta_local) == (160000.0, 10000.0)
    d = read_encoder_config(_dir(tmp_path, dict(OLD, global_rope_theta=5e5, local_rope_theta=2e4, local_attention=16), 64))["desc"]
    assert (d.rope_theta, d.rope_theta_local, d.window) == (5e5, 2e4, 8)
    # an explicit null: transformers rotates the windowed layers with the global base then
    d = read_encoder_config(_dir(tmp_path, dict(OLD, global_rope_theta=5e5, local_rope_theta=None), 64))["desc"]
    assert (d.rope_theta, d.rope_theta_local) == (5e5, 5e5)
    d = read_encoder_config(_dir(tmp_path, dict(OLD, global_attn_every_n_layers=1), 64))["desc"]  # no windowed layer
    assert (d.window, d.global_every, d.rope_theta_local, d.norm) == (0, 0, 0.0, "pre")


def test_long_declared_sequences_are_capped_with_one_warning(tmp_path, caplog):
    from voitta_rag_amd.embedding import MAX_SEQ, read_encoder_config

    with caplog.at_level(logging.WARNING, logger="voitta_rag_amd.embedding"):
        rc = read_encoder_config(_dir(tmp_path, NEW, max_seq=8192))
    assert rc["max_seq"] == MAX_SEQ == 512 and rc["desc"].max_pos == 512
    warnings = [r for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warnings) == 1 and "8192" in warnings[0].getMessage() and "512" in warnings[0].getMessage()


@pytest.mark.parametrize("change,message", [
    ({"hidden_activation": "silu"}, "hidden_activation 'silu'"),
    ({"rope_parameters": {"full_attention": {"rope_type": "yarn", "rope_theta": 160000.0, "factor": 2.0},
                          "sliding_attention": {"rope_type": "default", "rope_theta": 10000.0}}}, "rope type 'yarn'"),
    ({"rope_parameters": {"full_attention": {"rope_type": "default", "rope_theta": 160000.0},
                          "sliding_attention": {"rope_type": "linear", "rope_theta": 10000.0, "factor": 2.0}}},
     "rope type 'linear'"),
    ({"layer_types": ["full_attention", "sliding_attention"] * 11}, "layer_types"),
    ({"head_dim": 32}, "head_dim 32"),
])
def test_modernbert_config_refusals(tmp_path, change, message):
    from voitta_rag_amd.embedding import read_encoder_config

    with pytest.raises(ValueError, match=message) as err:
        read_encoder_config(_dir(tmp_path, dict(NEW, **change), max_seq=128))
    assert "not implemented" in str(err.value)


def test_other_model_types_stay_refused_and_other_families_keep_zero_fields(tmp_path):
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd.embedding import read_encoder_config

    with pytest.raises(ValueError, match="unsupported model_type gpt2"):
        read_encoder_config(_dir(tmp_path, dict(NEW, model_type="gpt2")))
    d = enc.BertDesc(2, 128, 2, 256)
    c = d.to_c()
    assert (d.norm, d.window, d.global_every, d.rope_theta_local, d.prenorm) == ("post", 0, 0, 0.0, False)
    assert (c.norm, c.window, c.global_every, c.rope_theta_local) == (0, 0, 0, 0.0)
    with pytest.raises(ValueError, match="unknown norm placement"):
        enc.BertDesc(2, 128, 2, 256, norm="sandwich").to_c()


# ---- state-dict mapping ------------------------------------------------------------------------------------------------
def test_every_tensor_lands_in_its_slot():
    from voitta_rag_amd import encoder as enc

    shape = mo.ModernShape(3, 128, 2, 256, window=8)
    w = mo.random_weights(shape, 3)
    desc = mo.desc_for(shape, "mean", "f32")
    H, I = shape.hidden, shape.intermediate
    for prefix in ("", "model."):
        names, state = enc.modernbert_slots({prefix + k: v for k, v in w.items()}, desc)
        assert len(names) == 5 + 18 * shape.layers
        slot = lambda i: None if names[i] is None else state[names[i]]  # noqa: E731
        assert np.array_equal(slot(0), w["embeddings.tok_embeddings.weight"]) and slot(1) is None
        assert slot(2).shape == (1, H) and not slot(2).any()  # the token-type table these models lack
        assert np.array_equal(slot(3), w["embeddings.norm.weight"]) and slot(4).shape == (H,) and not slot(4).any()
        for l in range(shape.layers):
            k, at = mo.layer_keys(l, shape.layers), 5 + 18 * l
            for j in range(3):  # query, key, value: thirds of Wqkv; no biases
                assert np.array_equal(slot(at + 2 * j), w[k["qkv_w"]][j * H:(j + 1) * H]) and slot(at + 2 * j + 1) is None
            assert np.array_equal(slot(at + 6), w[k["o_w"]]) and slot(at + 7) is None
            assert np.array_equal(slot(at + 8), w[k["mlp_norm"]]) and not slot(at + 9).any()  # attention.output.LayerNorm
            assert np.array_equal(slot(at + 10), w[k["wi_w"]][I:]) and slot(at + 11) is None  # the UP projection
            assert np.array_equal(slot(at + 12), w[k["wo_w"]]) and slot(at + 13) is None
            follows = w[mo.layer_keys(l + 1, shape.layers)["attn_norm"]] if l + 1 < shape.layers else w["final_norm.weight"]
            assert np.array_equal(slot(at + 14), follows) and not slot(at + 15).any()  # output.LayerNorm
            assert np.array_equal(slot(at + 16), w[k["wi_w"]][:I]) and slot(at + 17) is None  # the GATE projection
            for i in range(at, at + 18):
                assert names[i] is None or tuple(slot(i).shape) == enc.expected_shape(desc, names[i]), names[i]
    assert not any(k.endswith("layers.0.attn_norm.weight") for k in w)  # layer 0 has no attention norm


def test_biases_are_mapped_where_the_checkpoint_has_them():
    from voitta_rag_amd import encoder as enc

    shape = mo.ModernShape(2, 128, 2, 256, window=8)
    w = mo.random_weights(shape, 4)
    rng = np.random.default_rng(0)
    H, I = shape.hidden, shape.intermediate
    extra = {"embeddings.norm.bias": H, "final_norm.bias": H, "layers.1.attn_norm.bias": H, "layers.0.mlp_norm.bias": H,
             "layers.0.attn.Wqkv.bias": 3 * H, "layers.0.attn.Wo.bias": H, "layers.0.mlp.Wi.bias": 2 * I, "layers.0.mlp.Wo.bias": H}
    w.update({k: rng.normal(0, 0.1, n).astype(np.float32) for k, n in extra.items()})
    names, state = enc.modernbert_slots(w, mo.desc_for(shape, "mean", "f32"))
    slot = lambda i: None if names[i] is None else state[names[i]]  # noqa: E731
    assert np.array_equal(slot(4), w["embeddings.norm.bias"])
    assert [np.array_equal(slot(5 + 2 * j + 1), w["layers.0.attn.Wqkv.bias"][j * H:(j + 1) * H]) for j in range(3)] == [True] * 3
    assert np.array_equal(slot(5 + 7), w["layers.0.attn.Wo.bias"]) and np.array_equal(slot(5 + 9), w["layers.0.mlp_norm.bias"])
    assert np.array_equal(slot(5 + 11), w["layers.0.mlp.Wi.bias"][I:]) and np.array_equal(slot(5 + 17), w["layers.0.mlp.Wi.bias"][:I])
    assert np.array_equal(slot(5 + 13), w["layers.0.mlp.Wo.bias"]) and np.array_equal(slot(5 + 15), w["layers.1.attn_norm.bias"])
    assert np.array_equal(slot(23 + 15), w["final_norm.bias"]) and slot(23 + 7) is None and not slot(23 + 9).any()
    with pytest.raises(ValueError, match="three|3 equal parts"):
        enc.modernbert_slots(dict(w, **{"layers.0.attn.Wqkv.weight": w["layers.0.attn.Wqkv.weight"][:-1]}),
                             mo.desc_for(shape, "mean", "f32"))


def test_the_ctypes_mirror_ends_with_the_new_fields():
    import ctypes as C

    from voitta_rag_amd import _lib

    fields = [n for n, _ in _lib.VrBertDesc._fields_]
    assert fields[-4:] == ["norm", "window", "global_every", "rope_theta_local"] and fields[-5] == "ffn"
    assert _lib.VrBertDesc.norm.offset == _lib.VrBertDesc.ffn.offset + 4 and C.sizeof(_lib.VrBertDesc) == 4 * len(fields)
    header = open(os.path.join(os.path.dirname(HERE), "include", "voitta_engine.h")).read()
    body = header[header.index("typedef struct vr_bert_desc {"):header.index("} vr_bert_desc;")]
    declared = [line.split(";")[0].split()[-1] for line in body.splitlines() if line.strip().startswith(("int32_t", "float"))]
    assert declared == fields
    assert "#define VR_NORM_POST 0" in header and "#define VR_NORM_PRE  1" in header
