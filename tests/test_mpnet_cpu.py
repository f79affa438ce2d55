"""MPNet encoders (model_type mpnet) without a GPU: the config reader and its refusals, the bucket table against the
library's recorded bias, the state-dict mapping into the slots of vr_encoder_load, the f64 oracle against the transformers
goldens, the proof that the goldens and the synthetic table of the GPU tests see the mistakes a kernel can make, the
native WordPiece with named specials against the tokenizers library's recorded ids, and the two new symbols."""
import glob
import json
import os
import re

import numpy as np
import pytest

import mpnet_oracle as mp
from test_encoder_gpu import TOL

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "mpnet_tiny_*.npz")))
LENS = [1, 2, 8, 9, 16, 17, 64, 65, 128, 129, 130, 193, 257, 512]
TOKENIZER = os.path.join(HERE, "golden", "mpnet_tokenizer.json")
TOKENIZER_CASES = os.path.join(HERE, "golden", "mpnet_tokenizer_cases.json")


def load_case(path):
    g = np.load(path)
    L, H, nh, inter, vocab, positions = (int(x) for x in g["shape"])
    shape = mp.MpnetShape(L, H, nh, inter, vocab=vocab, positions=positions, eps=float(g["eps"]))
    seqs = [g["ids"][g["offsets"][i]:g["offsets"][i + 1]] for i in range(len(g["offsets"]) - 1)]
    return g, shape, str(g["pooling"]), int(g["seed"]), seqs, g["want"]


@pytest.fixture(scope="module")
def cases():
    """Per golden: the case and the seeded weights (made once, shared, read-only)."""
    out = {}
    for path in GOLDEN:
        c = load_case(path)
        w = mp.random_weights(c[1], c[3])
        for v in w.values():
            v.setflags(write=False)
        out[os.path.basename(path)] = c + (w,)
    return out


# ---- the config reader ------------------------------------------------------------------------------------------------
BASE = {"architectures": ["MPNetModel"], "model_type": "mpnet", "hidden_size": 768, "num_hidden_layers": 12,
        "num_attention_heads": 12, "intermediate_size": 3072, "vocab_size": 30527, "max_position_embeddings": 514,
        "layer_norm_eps": 1e-5, "hidden_act": "gelu", "relative_attention_num_buckets": 32, "pad_token_id": 1}


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


def test_config_reader_describes_all_mpnet_base_v2(tmp_path, monkeypatch):
    from voitta_rag_amd.embedding import read_encoder_config

    monkeypatch.delenv("VOITTA_ENCODER_PRECISION", raising=False)
    rc = read_encoder_config(_dir(tmp_path, BASE, max_seq=384))
    d = rc["desc"]
    assert (d.layers, d.hidden, d.heads, d.intermediate, d.vocab) == (12, 768, 12, 3072, 30527)
    assert (d.max_pos, d.type_vocab, d.eps, d.pooling, d.normalize) == (512, 1, 1e-5, "mean", True)
    assert (d.position, d.ffn, d.norm, d.window, d.precision) == ("learned", "gelu", "post", 0, "f16")
    assert d.attention_bias is None  # (the table comes with the weights)
    assert (rc["pos_start"], rc["max_seq"]) == (2, 384)
    rc = read_encoder_config(_dir(tmp_path, BASE, pooling="cls", normalize=False))
    assert (rc["desc"].pooling, rc["desc"].normalize, rc["max_seq"]) == ("cls", False, 512)
    rc = read_encoder_config(_dir(tmp_path, BASE, max_seq=4096))  # never more than the position table holds
    assert rc["max_seq"] == 512


def test_config_reader_refusals(tmp_path):
    from voitta_rag_amd.embedding import read_encoder_config

    with pytest.raises(ValueError, match="hidden_act 'relu' is not implemented"):
        read_encoder_config(_dir(tmp_path, dict(BASE, hidden_act="relu")))
    with pytest.raises(ValueError, match="relative_attention_num_buckets 31 is not implemented"):
        read_encoder_config(_dir(tmp_path, dict(BASE, relative_attention_num_buckets=31)))
    for kind in ("gpt2", "roberta"):
        with pytest.raises(ValueError, match=f"unsupported model_type {kind}"):
            read_encoder_config(_dir(tmp_path, dict(BASE, model_type=kind)))


# ---- the bias table -----------------------------------------------------------------------------------------------------
def test_goldens_hold_the_listed_cases(cases):
    assert sorted(cases) == ["mpnet_tiny_d32.npz", "mpnet_tiny_d64.npz"]
    for name, (g, shape, pooling, _, seqs, want, _) in cases.items():
        assert [len(s) for s in seqs] == LENS and want.dtype == np.float64 and want.shape == (len(seqs), 128)
        assert sorted(g.files) == sorted(["ids", "offsets", "want", "seed", "pooling", "position_bias", "shape", "eps",
                                          "versions"])  # no weights are stored
        assert os.path.getsize(os.path.join(HERE, "golden", name)) < 100_000
        assert (shape.layers, shape.hidden, shape.intermediate, shape.vocab, shape.positions) == (2, 128, 256, 300, 514)
        assert g["position_bias"].shape == (shape.heads, 512, 512) and g["position_bias"].dtype == np.float32
        assert not (np.concatenate(seqs) == 1).any()  # the padding id would move the positions
    assert (cases["mpnet_tiny_d64.npz"][1].heads, cases["mpnet_tiny_d64.npz"][2]) == (2, "mean")
    assert (cases["mpnet_tiny_d32.npz"][1].heads, cases["mpnet_tiny_d32.npz"][2]) == (4, "cls")


def test_bias_table_is_the_librarys_bias_bit_for_bit(cases):
    """mpnet_bias_table (torch, operation for operation) and the oracle's NumPy restatement of the buckets, expanded by
    clamped offset, against compute_position_bias for every (i, j) below 512 and every head."""
    from voitta_rag_amd.encoder import mpnet_bias_table, mpnet_relative_position_bucket

    import torch

    d = np.arange(-600, 601)
    assert np.array_equal(mpnet_relative_position_bucket(torch.from_numpy(d)).numpy(), mp.bucket(d))
    for g, shape, _, _, _, _, w in cases.values():
        table = mpnet_bias_table(w[mp.BIAS_KEY])
        assert table.dtype == np.float32 and table.shape == (shape.heads, 257) and table.flags.c_contiguous
        want = g["position_bias"]
        assert np.array_equal(mp.offset_bias(table, 512).astype(np.float32).view(np.uint32), want.view(np.uint32))
        assert np.array_equal(mp.table_from_buckets(w[mp.BIAS_KEY]), table.astype(np.float64))
        assert np.array_equal(mpnet_bias_table(torch.from_numpy(w[mp.BIAS_KEY].copy())), table)
    with pytest.raises(ValueError, match="even bucket count"):
        mpnet_bias_table(np.zeros((31, 2), np.float32))
    with pytest.raises(ValueError, match="radius 64"):
        mpnet_bias_table(np.zeros((32, 2), np.float32), radius=64)


def test_buckets_split_by_sign_exact_below_8_logarithmic_to_128():
    b = mp.bucket
    assert [int(b(-n)) for n in range(9)] == [0, 1, 2, 3, 4, 5, 6, 7, 8]  # the key BEFORE the query: n = i - j > 0
    assert [int(b(n)) for n in range(1, 9)] == [17, 18, 19, 20, 21, 22, 23, 24]
    assert int(b(0)) == 0 and int(b(-11)) == 8 and int(b(-12)) == 9 and int(b(-16)) == 10
    assert int(b(-90)) == 14 and int(b(-91)) == 15 and int(b(-128)) == 15 and int(b(-5000)) == 15
    assert int(b(90)) == 30 and int(b(91)) == 31 and int(b(5000)) == 31
    assert mp.bucket(np.arange(-5000, 5001)).max() == 31


# ---- the slot mapping ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", ["", "mpnet.", "0.auto_model."])
def test_state_dict_maps_onto_the_bert_slots(cases, prefix):
    from voitta_rag_amd import encoder as enc

    _, shape, pooling, _, _, _, w = cases["mpnet_tiny_d32.npz"]
    desc = mp.desc_for(shape, pooling, "f32")
    state, table = enc.mpnet_slots({prefix + k: v for k, v in w.items()}, desc)
    names = enc.tensor_names(desc.layers)
    assert len(names) == 5 + 16 * shape.layers and sorted(state) == sorted(names)
    for n in names:
        assert tuple(state[n].shape) == enc.expected_shape(desc, n), n
    assert np.array_equal(table, enc.mpnet_bias_table(w[mp.BIAS_KEY]))
    tt = state["embeddings.token_type_embeddings.weight"]
    assert tt.shape == (1, shape.hidden) and not tt.any()
    assert np.array_equal(state["embeddings.position_embeddings.weight"], w[mp.EMB_KEYS["pos"]][2:])
    assert state["embeddings.position_embeddings.weight"].shape[0] == desc.max_pos == 512
    k, b = mp.layer_keys(1), "encoder.layer.1."
    for slot, key in (("attention.self.query.weight", "q_w"), ("attention.self.key.bias", "k_b"),
                      ("attention.self.value.weight", "v_w"), ("attention.output.dense.weight", "o_w"),
                      ("attention.output.LayerNorm.bias", "ln1_b"), ("intermediate.dense.weight", "i_w"),
                      ("output.dense.bias", "f_b"), ("output.LayerNorm.weight", "ln2_g")):
        assert state[b + slot] is w[k[key]], slot


def test_missing_or_ambiguous_tensors_are_named(cases):
    from voitta_rag_amd import encoder as enc

    _, shape, pooling, _, _, _, w = cases["mpnet_tiny_d64.npz"]
    desc = mp.desc_for(shape, pooling, "f32")
    for gone in ("encoder.relative_attention_bias.weight", "encoder.layer.1.attention.attn.o.bias",
                 "embeddings.position_embeddings.weight"):
        with pytest.raises(KeyError, match=re.escape(gone)):
            enc.mpnet_slots({k: v for k, v in w.items() if k != gone}, desc)
    twice = dict(w)
    twice["mpnet.encoder.layer.0.output.dense.weight"] = w["encoder.layer.0.output.dense.weight"]
    with pytest.raises(KeyError, match=r"encoder\.layer\.0\.output\.dense\.weight"):
        enc.mpnet_slots(twice, desc)


def test_load_encoder_sets_the_bias_after_the_load(cases):
    """load_encoder hands the 5 + 16 L tensors to vr_encoder_load and THEN the description's table to the engine; a
    description without one makes no such call."""
    import ctypes as C

    from voitta_rag_amd import encoder as enc

    _, shape, pooling, _, _, _, w = cases["mpnet_tiny_d64.npz"]
    calls = []

    class Lib:
        @staticmethod
        def vr_encoder_load(handle, desc, arr, n, mem):
            calls.append(("load", n, C.cast(desc, C.POINTER(enc._lib.VrBertDesc)).contents.type_vocab))
            return 0

    class FakeEngine:
        handle, _lib = None, Lib

        def set_attention_bias(self, table):
            calls.append(("bias", table.shape))

    desc = mp.desc_for(shape, pooling, "f32")
    state, desc.attention_bias = enc.mpnet_slots(w, desc)
    enc.load_encoder(FakeEngine(), desc, state)
    assert calls == [("load", 5 + 16 * shape.layers, 1), ("bias", (shape.heads, 257))]
    del calls[:]
    enc.load_encoder(FakeEngine(), mp.desc_for(shape, pooling, "f32"), state)
    assert calls == [("load", 5 + 16 * shape.layers, 1)]


# ---- the oracle and what the fixtures can see ---------------------------------------------------------------------------
def _miss(got, want):
    cos = (got * want).sum(1) / np.linalg.norm(got, axis=1) / np.linalg.norm(want, axis=1)
    return float(np.max(np.abs(1 - cos))), float(np.max(np.abs(got - want)))


def test_oracle_reproduces_transformers(cases):
    """Everything is f64 on both sides and the bias values are the same f32 numbers: 1e-9 max-abs on unit embeddings
    (measured 1.4e-16)."""
    for name, (_, shape, pooling, _, seqs, want, w) in cases.items():
        worst = _miss(mp.sentence_embeddings(w, shape, seqs, pooling), want)[1]
        print(f"{name}: oracle vs transformers f64, max-abs {worst:.3e}")
        assert worst < 1e-9


def test_goldens_see_a_dropped_a_mirrored_and_a_short_clamped_bias(cases):
    """The oracle re-run with each mistake a kernel can make must miss the golden by more than 100 x the f16 bar of
    test_encoder_gpu.TOL, taken on its |1 - cos| part (1e-5: the worst row's cosine is off by more than 1e-3).
    Measured |1 - cos| / max-abs, d64 then d32: dropped 8.3e-3 / 3.3e-2 and 1.8e-2 / 4.9e-2, mirrored 3.0e-2 / 7.2e-2
    and 9.0e-3 / 3.5e-2, clamp 1.4e-3 / 1.8e-2 and 1.2e-3 / 1.2e-2.
    The clamp: MPNet's buckets are constant from |j - i| = 91 on, not only from 128 (8 + 8 log(n / 8) / log 16 reaches
    15, the last bucket of a half, at n = 8 * 16^(7/8) = 90.5), so a clamp at 127 for 128 computes the same model and no
    seed or scale can tell them apart — asserted below. What the goldens can see is the clamp one short of where the
    table really saturates, 90 for 91; a clamp one short of the TABLE's radius is seen by the independent entries of the
    radius-8 table (test_synthetic_table_sees_a_clamp_one_short)."""
    bar = 100 * TOL["f16"][0]
    for name, (_, shape, pooling, _, seqs, want, w) in cases.items():
        for what, kw in (("dropped", dict(table=None)), ("mirrored", dict(mirrored=True)), ("clamp 90", dict(clamp=90))):
            cos, worst = _miss(mp.sentence_embeddings(w, shape, seqs, pooling, **kw), want)
            print(f"{name}: bias {what}: |1 - cos| {cos:.3e}, max-abs {worst:.3e}")
            assert cos > bar, (name, what)
        same = mp.sentence_embeddings(w, shape, seqs[-2:], pooling, clamp=127)
        assert np.array_equal(same, mp.sentence_embeddings(w, shape, seqs[-2:], pooling))
    assert np.array_equal(mp.bucket(np.array([-128, -127, -91, 91, 127, 128])), [15, 15, 15, 31, 31, 31])


def synthetic_table(heads: int, radius: int = 8, seed: int = 7) -> np.ndarray:
    """Independent N(0, 1) entries: unlike a bucket table, every offset up to the radius has a value of its own."""
    return np.random.default_rng(seed).normal(0, 1, (heads, 2 * radius + 1)).astype(np.float32)


def test_synthetic_table_sees_a_clamp_one_short():
    """The radius-8 table of the GPU tests against the same table clamped at 7 and mirrored, on a 17-token sequence (the
    shortest with an offset of 8 in more than one place): each more than 100 x the f16 bar away (measured 1.7e-3 and
    1.2e-3 in |1 - cos|, 2.1e-2 and 1.1e-2 max-abs)."""
    shape = mp.MpnetShape(3, 128, 2, 256)
    w = mp.random_weights(shape, 51)
    table = synthetic_table(shape.heads)
    seq = [np.random.default_rng(5).integers(4, shape.vocab, size=17)]
    want = mp.sentence_embeddings(w, shape, seq, "mean", table=table)
    for kw in (dict(clamp=7), dict(mirrored=True)):
        got = mp.sentence_embeddings(w, shape, seq, "mean", table=table, **kw)
        cos, worst = _miss(got, want)
        print(f"{kw}: |1 - cos| {cos:.3e}, max-abs {worst:.3e}")
        assert cos > 100 * TOL["f16"][0], kw


# ---- the tokenizer ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tok_cases():
    return json.load(open(TOKENIZER_CASES, encoding="utf-8"))


def _tokenizer_dir(tmp_path, spec=None):
    d = tmp_path / f"t{len(list(tmp_path.iterdir()))}"
    os.makedirs(d)
    json.dump(spec or json.load(open(TOKENIZER, encoding="utf-8")), open(d / "tokenizer.json", "w", encoding="utf-8"))
    return str(d)


def test_golden_tokenizer_is_in_mpnets_layout(tok_cases):
    spec = json.load(open(TOKENIZER, encoding="utf-8"))
    v = spec["model"]["vocab"]
    assert [v[t] for t in ("<s>", "<pad>", "</s>", "<unk>")] == [0, 1, 2, 3] and v["<mask>"] == len(v) - 1
    assert spec["model"]["type"] == "WordPiece" and spec["model"]["unk_token"] == "[UNK]"
    assert spec["post_processor"]["type"] == "RobertaProcessing"
    assert spec["post_processor"]["cls"] == ["<s>", 0] and spec["post_processor"]["sep"] == ["</s>", 2]
    assert len(tok_cases) >= 30 and os.path.getsize(TOKENIZER_CASES) < 100_000
    texts = [c["text"] for c in tok_cases]
    assert "" in texts and any("é" in t for t in texts) and any("中" in t for t in texts)
    assert any(c["max_len"] == 16 and len(c["ids"]) == 16 for c in tok_cases)
    assert any(c["max_len"] == 512 and len(c["ids"]) == 512 for c in tok_cases)


def test_native_tokenizer_gives_the_recorded_ids(tmp_path, tok_cases):
    from voitta_rag_amd.wordpiece import WordPieceTokenizer

    spec = json.load(open(TOKENIZER, encoding="utf-8"))
    unk = spec["model"]["vocab"]["[UNK]"]
    tok = WordPieceTokenizer.from_pretrained(_tokenizer_dir(tmp_path))
    assert tok.specials == ("<s>", "</s>", "[UNK]")
    seen_unk = False
    for max_len in (512, 16):
        part = [c for c in tok_cases if c["max_len"] == max_len]
        tok.max_length = max_len
        ids, off = tok.encode_batch([c["text"] for c in part])
        for i, c in enumerate(part):
            got = ids[off[i]:off[i + 1]].tolist()
            assert got == c["ids"], (c["text"][:40], max_len)
            assert got[0] == 0 and got[-1] == 2 and 3 not in got  # <s> ... </s>; <unk> is not the model's unknown token
            seen_unk |= unk in got
    assert seen_unk
    ids, off = tok.encode_batch(["zzzqqq unknownword"])
    assert ids.tolist() == [0, unk, unk, 2]
    tok.close()


def test_encode_pairs_is_refused_with_named_specials(tmp_path):
    import ctypes as C

    from voitta_rag_amd.wordpiece import WordPieceTokenizer

    tok = WordPieceTokenizer.from_pretrained(_tokenizer_dir(tmp_path))
    with pytest.raises(ValueError, match="encode_pairs on a tokenizer with the specials '<s>' / '</s>'"):
        tok.encode_pairs(["vector"], ["database"])
    # ... and by the library itself, for the engine's own callers (a reranker's text path)
    a, b = (C.c_char_p * 1)(b"vector"), (C.c_char_p * 1)(b"database")
    lens, off, ids, needed = (C.c_int64 * 1)(6), (C.c_int64 * 2)(), (C.c_int32 * 16)(), C.c_int64()
    lens_b = (C.c_int64 * 1)(8)
    rc = tok._lib.vr_wordpiece_encode_pairs(tok._h, a, lens, b, lens_b, 1, 16, off, ids, None, 16, C.byref(needed))
    assert rc == -1 and b"named specials" in tok._lib.vr_last_error()
    tok.close()


def test_template_processing_names_the_specials_too(tmp_path, tok_cases):
    from voitta_rag_amd.wordpiece import WordPieceTokenizer, wordpiece_specials

    spec = json.load(open(TOKENIZER, encoding="utf-8"))
    template = {"type": "TemplateProcessing",
                "single": [{"SpecialToken": {"id": "<s>", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}},
                           {"SpecialToken": {"id": "</s>", "type_id": 0}}],
                "pair": [], "special_tokens": {"<s>": {"id": "<s>", "ids": [0], "tokens": ["<s>"]},
                                               "</s>": {"id": "</s>", "ids": [2], "tokens": ["</s>"]}}}
    assert wordpiece_specials(dict(spec, post_processor=template)) == ("<s>", "</s>", "[UNK]")
    tok = WordPieceTokenizer.from_pretrained(_tokenizer_dir(tmp_path, dict(spec, post_processor=template)))
    c = next(c for c in tok_cases if "encoder" in c["text"])
    ids, _ = tok.encode_batch([c["text"]])
    assert ids.tolist() == c["ids"]
    tok.close()
    bad = json.loads(json.dumps(template))
    bad["single"] = bad["single"][:2]
    for post, message in ((bad, "template is not"), ({"type": "ByteLevel"}, "post_processor 'ByteLevel'"),
                          (dict(spec["post_processor"], cls=["<s>", 5]), "gives '<s>' id 5")):
        with pytest.raises(ValueError, match=message):
            wordpiece_specials(dict(spec, post_processor=post))


def test_encoder_takes_the_native_route_only_when_the_names_are_found(tmp_path):
    pytest.importorskip("tokenizers")
    from voitta_rag_amd.embedding import NativeSentenceEncoder, native_tokenizer

    spec = json.load(open(TOKENIZER, encoding="utf-8"))
    cfg = {"model_type": "mpnet"}
    tok = NativeSentenceEncoder._load_tokenizer(_tokenizer_dir(tmp_path), cfg)
    assert native_tokenizer(tok) and tok.specials == ("<s>", "</s>", "[UNK]")
    tok.close()
    # no post_processor, or one the native tokenizer does not produce: the tokenizers library, which wraps as the file says
    for post in (None, {"type": "ByteLevel", "add_prefix_space": True, "trim_offsets": True, "use_regex": True}):
        other = NativeSentenceEncoder._load_tokenizer(_tokenizer_dir(tmp_path, dict(spec, post_processor=post)), cfg)
        assert not native_tokenizer(other)
        assert other.encode("vector database").ids == [spec["model"]["vocab"]["vector"], spec["model"]["vocab"]["database"]]


def test_a_bert_tokenizer_json_yields_what_it_did(tmp_path):
    """[CLS] ... [SEP] through vr_wordpiece_create, with and without a post_processor in the file, equal to the
    tokenizers library's ids."""
    pytest.importorskip("tokenizers")
    from voitta_rag_amd.embedding import NativeSentenceEncoder, build_wordpiece_tokenizer, native_tokenizer
    from voitta_rag_amd.wordpiece import DEFAULT_SPECIALS

    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "vector", "data", "##base", "##s", "cafe", "!", "中"]
    hf = build_wordpiece_tokenizer(vocab)
    texts = ["Vector databases!", "café 中 unknown", ""]
    want = [e.ids for e in hf.encode_batch(texts)]
    spec = json.loads(hf.to_str())
    assert spec["post_processor"]["type"] == "TemplateProcessing"
    for s in (spec, dict(spec, post_processor=None)):
        tok = NativeSentenceEncoder._load_tokenizer(_tokenizer_dir(tmp_path, s), {"model_type": "bert"})
        assert native_tokenizer(tok) and tok.specials == DEFAULT_SPECIALS
        ids, off = tok.encode_batch(texts)
        assert [ids[off[i]:off[i + 1]].tolist() for i in range(len(texts))] == want
        assert want[0][0] == 2 and want[0][-1] == 3
        a_ids, a_off, seg = tok.encode_pairs(["vector"], ["data"])  # pairs stay available
        assert a_ids.tolist() == [2, 4, 3, 5, 3] and seg.tolist() == [3]
        tok.close()


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_header_library_and_signatures_list_both_new_symbols():
    import ctypes as C

    from voitta_rag_amd import _lib

    header = open(os.path.join(ROOT, "include", "voitta_engine.h"), encoding="utf-8").read()
    lib = _lib.load_library()
    for name in ("vr_encoder_set_attention_bias", "vr_wordpiece_create_specials"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["vr_encoder_set_attention_bias"][1]) == 5
    assert len(_lib.SIGNATURES["vr_wordpiece_create_specials"][1]) == 10
    # vr_bert_desc did not grow: the bias is not a field of it
    fields = [f[0] for f in _lib.VrBertDesc._fields_]
    assert fields[-4:] == ["norm", "window", "global_every", "rope_theta_local"]
    # no engine: refused, nothing dereferenced
    assert lib.vr_encoder_set_attention_bias(None, None, 0, 0, 0) != 0
