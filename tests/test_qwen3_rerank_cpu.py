"""Decoder cross-encoders (Qwen3-Reranker), no GPU: tests/qwen3_rerank_oracle.py against transformers' Qwen3ForCausalLM
(tests/golden/qwen3_rerank_*.npz) at 1e-9, the exposure of the goldens (a neighbouring row's logit is far from the
pair's own), the head row of every checkpoint form, the config reader and its refusals, the prompt assembly of
DecoderPairTokenizer against the oracle's pure-Python restatement, and the ctypes table against the header."""
import json
import os

import numpy as np
import pytest

import qwen3_oracle as qo
import qwen3_rerank_oracle as ro
from test_abi_cpu import header_symbols
from test_qwen3_cpu import settings  # noqa: F401  (fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = ["tiny_d128b", "tiny_d64n"]
LENGTHS = [1, 2, 15, 16, 17, 63, 64, 65, 100, 127, 128, 129, 200, 320, 321, 449]
F16_BAR = 5e-2  # tests/test_rerank_gpu.py's BAR["f16"]


def golden(name):
    """-> shape, tied, seed, sequences, transformers' logits"""
    z = np.load(os.path.join(HERE, "golden", f"qwen3_rerank_{name}.npz"))
    layers, hidden, heads, kv_heads, inter, head_dim, qk_norm, vocab, tied, yes, no = (int(v) for v in z["shape"])
    assert (yes, no) == (ro.YES_ID, ro.NO_ID)
    shape = qo.Qwen3Shape(layers, hidden, heads, kv_heads, inter, head_dim, qk_norm=bool(qk_norm), vocab=vocab,
                          theta=float(z["theta"]), eps=float(z["eps"]))
    off = z["offsets"]
    return shape, bool(tied), int(z["seed"]), [z["ids"][off[i]:off[i + 1]] for i in range(len(off) - 1)], z["logits"]


_rows = {}


def golden_row_logits(name):
    """The oracle's logit of EVERY token row of every golden pair (once, read-only); the model's is the last."""
    if name not in _rows:
        shape, tied, seed, seqs, _ = golden(name)
        w = ro.random_weights(shape, seed, tied)
        _rows[name] = [ro.row_logits(w, shape, s) for s in seqs]
        for r in _rows[name]:
            r.setflags(write=False)
    return _rows[name]


# ---- the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_matches_transformers(name):
    shape, tied, seed, seqs, logits = golden(name)
    assert [len(s) for s in seqs] == LENGTHS
    assert (tied, shape.hidden, shape.heads, shape.head_dim) == {"tiny_d128b": (True, 256, 4, 128), "tiny_d64n": (False, 128, 2, 64)}[name]
    mine = np.asarray([r[-1] for r in golden_row_logits(name)])
    assert np.max(np.abs(mine - logits)) < 1e-9
    assert logits.max() - logits.min() >= 20 * F16_BAR  # the logits spread: a constant answer cannot pass


@pytest.mark.parametrize("name", GOLDENS)
def test_a_neighbouring_row_gives_another_logit(name):
    """Exposure: the logit read off the penultimate token's row, or off the first row of the next sequence, is more than
    twice the f16 bar from the pair's own — a gather that is off by one row cannot pass the GPU tests."""
    rows = golden_row_logits(name)
    checked = 0
    for i, r in enumerate(rows):
        if len(r) < 2:
            continue
        assert abs(r[-2] - r[-1]) > 2 * F16_BAR, (i, r[-2], r[-1])
        checked += 1
        if i + 1 < len(rows):
            assert abs(rows[i + 1][0] - r[-1]) > 2 * F16_BAR, (i, rows[i + 1][0], r[-1])
            checked += 1
    assert checked == 2 * (len(LENGTHS) - 1) - 1


def test_the_score_is_the_softmax_at_yes():
    shape, tied, seed, seqs, _ = golden("tiny_d64n")
    w = ro.random_weights(shape, seed, tied)
    h = qo.encode_one(ro.body_weights(w), shape, seqs[4])[-1]
    two = np.asarray([w[ro.LM_HEAD_KEY][ro.NO_ID].astype(np.float64) @ h, w[ro.LM_HEAD_KEY][ro.YES_ID].astype(np.float64) @ h])
    p_yes = np.exp(two - two.max())[1] / np.exp(two - two.max()).sum()
    from voitta_rag_amd.reranker import sigmoid

    assert abs(p_yes - sigmoid(ro.logit(w, shape, seqs[4]))) < 1e-12


# ---- the head row ----------------------------------------------------------------------------------------------------------
def _desc(shape):
    return ro.desc_for(shape, "f32")


def test_head_row_of_tied_untied_and_seq_cls_checkpoints():
    from voitta_rag_amd import encoder as enc

    shape = qo.Qwen3Shape(1, 128, 2, 1, 256, 64)
    rng = np.random.default_rng(3)
    for tied in (True, False):
        w = {"model." + k: v for k, v in ro.random_weights(shape, 9, tied).items() if k != ro.LM_HEAD_KEY}
        if not tied:
            w["lm_head.weight"] = ro.random_weights(shape, 9, tied)[ro.LM_HEAD_KEY]
        W = w["model.embed_tokens.weight"] if tied else w["lm_head.weight"]
        row = enc.qwen3_rerank_head(w, _desc(shape), 5, 9)
        assert row.shape == (1, 128) and row.dtype == np.float32
        want = (W[5].astype(np.float64) - W[9].astype(np.float64)).astype(np.float32)  # f64, rounded once
        assert np.array_equal(row[0], want)
        for over, message in ((dict(yes_id=None, no_id=9), "the id of the token 'yes' is missing"),
                              (dict(yes_id=5, no_id=None), "the id of the token 'no' is missing"),
                              (dict(yes_id=5, no_id=shape.vocab), f"the id {shape.vocab} of the token 'no' is outside")):
            with pytest.raises(ValueError, match=message):
                enc.qwen3_rerank_head(w, _desc(shape), **over)
    score = rng.normal(size=(1, 128)).astype(np.float32)
    w = {"model." + k: v for k, v in qo.random_weights(shape, 9).items()}
    w["score.weight"] = score
    assert np.array_equal(enc.qwen3_rerank_head(w, _desc(shape)), score)  # as stored; no ids needed
    w["score.weight"] = np.zeros((2, 128), np.float32)
    with pytest.raises(ValueError, match=r"'score.weight' has shape \(2, 128\)"):
        enc.qwen3_rerank_head(w, _desc(shape))
    with pytest.raises(KeyError, match="'score.weight', 'lm_head.weight' or 'embed_tokens.weight' not found"):
        enc.qwen3_rerank_head({}, _desc(shape), 1, 2)


def test_load_reranker_passes_the_body_and_one_head_tensor():
    """load_reranker with a decoder description: qwen3_slots' tensors (NULL where the family has none), then score.weight,
    through vr_reranker_load_decoder — seen through a stand-in engine."""
    import ctypes as C

    from voitta_rag_amd import encoder as enc

    shape = qo.Qwen3Shape(2, 128, 2, 1, 256, 128)
    w = {"model." + k: v for k, v in ro.random_weights(shape, 4, True).items()}
    seen = {}

    class Lib:
        def vr_reranker_load_decoder(self, handle, desc, arr, n, mem):
            seen.update(n=n, ptrs=[arr[i] for i in range(n)], desc=desc._obj, mem=mem)
            seen["score"] = np.ctypeslib.as_array(C.cast(arr[n - 1], C.POINTER(C.c_float)), (128,)).copy()
            return 0

        def vr_reranker_load(self, *a):
            raise AssertionError("a decoder description must not go through vr_reranker_load")

    class Eng:
        handle = None
        _lib = Lib()

    e = Eng()
    enc.load_reranker(e, ro.desc_for(shape, "f16"), w, yes_id=ro.YES_ID, no_id=ro.NO_ID)
    assert seen["n"] == 5 + 20 * 2 + 1 and seen["ptrs"][-1] is not None and seen["ptrs"][1] is None
    assert np.array_equal(seen["score"], ro.score_row({qo.WORD_KEY: w["model.embed_tokens.weight"]}).astype(np.float32))
    assert (seen["desc"].pooling, seen["desc"].normalize, seen["desc"].head_dim, seen["desc"].qk_norm, seen["desc"].causal) == (2, 0, 128, 1, 1)
    assert e.reranker_desc.pooling == "last"
    for over, message in ((dict(pooling="mean"), "last token"), (dict(normalize=True), "without normalising")):
        with pytest.raises(ValueError, match=message):
            enc.load_reranker(e, ro.desc_for(shape, "f16", **over), w, yes_id=1, no_id=2)


# ---- config.json -----------------------------------------------------------------------------------------------------------
def _config_dir(tmp_path, **over):
    d = str(tmp_path / "rr")
    os.makedirs(d, exist_ok=True)
    cfg = qo.config_json(qo.Qwen3Shape(2, 128, 2, 1, 256, 128), architectures=["Qwen3ForCausalLM"])
    cfg.update(over)
    json.dump(cfg, open(os.path.join(d, "config.json"), "w"))
    return d


@pytest.mark.parametrize("over", [dict(), dict(architectures=["Qwen3ForSequenceClassification"], num_labels=1),
                                  dict(model_type="qwen2", architectures=["Qwen2ForCausalLM"]),
                                  dict(model_type="qwen2", architectures=["Qwen2ForSequenceClassification"], id2label={"0": "LABEL_0"})])
def test_config_reader_accepts_the_decoder_forms(tmp_path, over):
    from voitta_rag_amd.reranker import read_cross_encoder_config

    assert read_cross_encoder_config(_config_dir(tmp_path, **over))["model_type"] == over.get("model_type", "qwen3")


@pytest.mark.parametrize("over, message", [
    (dict(architectures=["Qwen3Model"]), r"unsupported reranker qwen3 / \['Qwen3Model'\]: Qwen3ForCausalLM .* or Qwen3ForSequenceClassification"),
    (dict(architectures=["Qwen2ForCausalLM"]), r"unsupported reranker qwen3 / \['Qwen2ForCausalLM'\]"),
    (dict(model_type="qwen2", architectures=["Qwen3ForCausalLM"]), r"unsupported reranker qwen2 / \['Qwen3ForCausalLM'\]"),
    (dict(architectures=[]), r"unsupported reranker qwen3 / \[\]"),
    (dict(architectures=["Qwen3ForSequenceClassification"], num_labels=2), "the reranker has 2 labels"),
    (dict(architectures=["Qwen3ForSequenceClassification"]), "the reranker has 2 labels"),  # (the library's default)
    (dict(architectures=["Qwen3ForSequenceClassification"], num_labels=3), "the reranker has 3 labels"),
])
def test_config_reader_refusals_by_name(tmp_path, over, message):
    from voitta_rag_amd.reranker import read_cross_encoder_config

    with pytest.raises(ValueError, match=message):
        read_cross_encoder_config(_config_dir(tmp_path, **over))


def test_the_bodys_limits_are_the_embedders(tmp_path, settings):  # noqa: F811
    """The 4B and 8B rerankers are refused by field, through embedding._read_qwen3_config: their 32 heads of 128 first,
    and a body of their hidden size with the 0.6B's heads by hidden_size."""
    from voitta_rag_amd.reranker import NativeCrossEncoder

    with pytest.raises(ValueError, match="num_attention_heads 32 x head_dim 128 = 4096 is not implemented"):
        NativeCrossEncoder.from_pretrained(_config_dir(tmp_path, hidden_size=2560, num_attention_heads=32), engine=object())
    with pytest.raises(ValueError, match="hidden_size 2560 is not implemented"):
        NativeCrossEncoder.from_pretrained(_config_dir(tmp_path, hidden_size=2560, num_attention_heads=16), engine=object())


# ---- the prompt ------------------------------------------------------------------------------------------------------------
WORDS = ("vector database index hybrid fusion ranking sparse dense retrieval kernel memory bandwidth decoder attention "
         "causal mask rotary position norm residual token chunk document search query score filter").split()


def _tokenizer():
    pytest.importorskip("tokenizers")
    return ro.make_tokenizer(ro.template_words() + WORDS)


def test_prompt_strings_are_the_published_ones():
    from voitta_rag_amd import reranker as rr

    assert (rr.DECODER_PREFIX, rr.DECODER_SUFFIX, rr.DEFAULT_INSTRUCTION) == (ro.PREFIX, ro.SUFFIX, ro.DEFAULT_INSTRUCTION)
    assert rr.decoder_body("i", "q", "d") == ro.body_text("i", "q", "d") == "<Instruct>: i\n<Query>: q\n<Document>: d"


def test_decoder_pair_tokenizer_equals_the_restatement(tmp_path):
    from tokenizers import Tokenizer

    from voitta_rag_amd.reranker import DecoderPairTokenizer

    tok = _tokenizer()
    tok.save(str(tmp_path / "tokenizer.json"))
    encode = lambda t: Tokenizer.from_file(str(tmp_path / "tokenizer.json")).encode(t, add_special_tokens=False).ids  # noqa: E731
    prefix, suffix = encode(ro.PREFIX), encode(ro.SUFFIX)
    for marker in ro.SPECIALS[:4]:  # the chat markers and the think tags are single tokens of the prompt
        assert tok.token_to_id(marker) in prefix + suffix
    assert suffix[-2:] == [tok.token_to_id("<think>"), tok.token_to_id("</think>")] and tok.token_to_id("[UNK]") not in prefix + suffix
    rng = np.random.default_rng(2)
    a = [" ".join(rng.choice(WORDS, size=int(n))) for n in (1, 4, 7, 2, 3)]
    b = [" ".join(rng.choice(WORDS, size=int(n))) for n in (0, 3, 60, 25, 11)]
    dt = DecoderPairTokenizer.from_pretrained(str(tmp_path), 512)
    assert dt.token_to_id("yes") is not None and dt.token_to_id("no") is not None and dt.token_to_id("maybe") is None
    for max_length, instruction in ((512, ro.DEFAULT_INSTRUCTION), (len(prefix) + len(suffix) + 30, ro.DEFAULT_INSTRUCTION),
                                    (len(prefix) + len(suffix) + 1, ro.DEFAULT_INSTRUCTION), (90, "rank index chunk")):
        dt.max_length = max_length
        dt.instruction = instruction
        ids, off, seg = dt.encode_pairs(a, b)
        assert seg is None and ids.dtype == np.int32 and off.dtype == np.int64 and off[0] == 0
        want = [ro.assemble(encode, q, d, max_length, instruction) for q, d in zip(a, b)]
        assert [ids[off[i]:off[i + 1]].tolist() for i in range(len(a))] == want
        assert max(len(s) for s in want) <= max_length
        if max_length < 512:  # the body is cut from the right, the suffix stays whole
            cut = [len(s) for s in want]
            assert max(cut) == max_length and all(s[-len(suffix):] == suffix and s[:len(prefix)] == prefix for s in want)
    body = encode(ro.body_text(ro.DEFAULT_INSTRUCTION, a[2], b[2]))
    dt.max_length, dt.instruction = len(prefix) + len(suffix) + 30, ro.DEFAULT_INSTRUCTION
    ids, off, _ = dt.encode_pairs(a[2:3], b[2:3])
    assert len(body) > 30 and ids.tolist() == prefix + body[:30] + suffix
    # nothing left for the body
    for bad in (len(prefix) + len(suffix), 3):
        with pytest.raises(ValueError, match=f"max_length {bad} leaves {bad - len(prefix) - len(suffix)} tokens for the body"):
            dt.max_length = bad
        with pytest.raises(ValueError, match=f"max_length {bad} leaves"):
            DecoderPairTokenizer.from_pretrained(str(tmp_path), bad)
        with pytest.raises(ValueError, match=f"max_length {bad} leaves"):
            ro.assemble(encode, "q", "d", bad)


def test_a_causal_lm_without_yes_or_no_is_refused_by_name(tmp_path, settings):  # noqa: F811
    from tokenizers import Tokenizer, models

    from voitta_rag_amd.reranker import NativeCrossEncoder

    d = _config_dir(tmp_path)
    for missing in ("yes", "no"):
        tok = Tokenizer(models.WordLevel({"[UNK]": 0, "a": 1}, unk_token="[UNK]"))
        tok.add_tokens([t for t in ro.SPECIALS if t != missing])
        tok.save(os.path.join(d, "tokenizer.json"))
        with pytest.raises(ValueError, match=f"has no token '{missing}'"):
            NativeCrossEncoder.from_pretrained(d, engine=object())


def test_the_instruction_setting(settings):  # noqa: F811
    from voitta_rag_amd.config import get_settings

    assert get_settings().rerank_instruction == ""
    settings(VOITTA_RERANK_INSTRUCTION="Rank code snippets")
    assert get_settings().rerank_instruction == "Rank code snippets"


# ---- the ABI table -----------------------------------------------------------------------------------------------------------
def test_the_ctypes_table_still_equals_the_header():
    from voitta_rag_amd import _lib

    names = header_symbols()
    assert "vr_reranker_load_decoder" in names and sorted(_lib.SIGNATURES) == names
    assert _lib.SIGNATURES["vr_reranker_load_decoder"] == _lib.SIGNATURES["vr_reranker_load"]
    assert hasattr(_lib.load_library(), "vr_reranker_load_decoder")
