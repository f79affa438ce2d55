"""No-GPU checks of cross-encoder reranking: the pair tokeniser (vr_wordpiece_encode_pairs) against the HF `tokenizers`
library itself (BERT pair template, LongestFirst truncation), the f64 oracle against the transformers golden logits,
the checkpoint refusals of reranker.read_config, and argument errors of vr_rerank / vr_rerank_text raised before the
engine is touched (a NULL engine: valid input reaches the engine check, bad input never does)."""
import ctypes as C
import glob
import json
import os

import numpy as np
import pytest

from oracle import bert as obert

import rerank_oracle as ro

tokenizers = pytest.importorskip("tokenizers")
from test_wordpiece_cpu import _hf, _random_text, _vocab  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "rerank_*.npz")))


def _hf_pairs(vocab, lowercase, max_len):
    from tokenizers import processors

    tok = _hf(vocab, lowercase, max_length=max_len)
    ids = {t: i for i, t in enumerate(vocab)}
    tok.post_processor = processors.TemplateProcessing(
        single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1",
        special_tokens=[("[CLS]", ids["[CLS]"]), ("[SEP]", ids["[SEP]"])])
    tok.enable_truncation(max_length=max_len, strategy="longest_first")
    return tok


@pytest.mark.parametrize("lowercase", [True, False])
def test_pair_ids_equal_hf_tokenizers(lowercase):
    from voitta_rag_amd.wordpiece import WordPieceTokenizer

    rng = np.random.default_rng(7 + int(lowercase))
    queries = [_random_text(rng, int(rng.integers(0, 60))) for _ in range(40)]
    passages = [_random_text(rng, int(rng.integers(0, 700))) for _ in range(400)]
    queries += ["", "hello world " * 300, "unbelievable tokenizers!"]
    passages += ["", "", "hello world " * 300, "a b c"]
    vocab = _vocab(rng, queries + passages, _hf(["[UNK]", "[CLS]", "[SEP]"], lowercase))
    a = [queries[int(rng.integers(len(queries)))] for _ in passages]
    a[-4:] = ["hello world " * 300, "", "", "hello world " * 300]  # one side alone over max_len, an empty side, both empty
    for max_len in (8, 16, 64, 512):
        hf = _hf_pairs(vocab, lowercase, max_len)
        ours = WordPieceTokenizer(vocab, lowercase, max_length=max_len)
        ids, off, seg = ours.encode_pairs(a, passages)
        want = hf.encode_batch(list(zip(a, passages)))
        bad = 0
        for i, enc in enumerate(want):
            got = ids[off[i]:off[i + 1]].tolist()
            if got != enc.ids or seg[i] != enc.type_ids.index(1):
                bad += 1
                if bad <= 3:
                    print(f"pair {i}: want {enc.ids} (B at {enc.type_ids.index(1)})\n  got {got} (B at {seg[i]})")
        assert bad == 0, f"{bad} of {len(want)} pairs differ (max_len {max_len})"
        assert (off[1:] - off[:-1]).max() <= max_len
        ours.close()


def test_pair_tokeniser_errors():
    from voitta_rag_amd._lib import EngineError
    from voitta_rag_amd.wordpiece import WordPieceTokenizer

    tok = WordPieceTokenizer(["[UNK]", "[CLS]", "[SEP]", "a"], max_length=2)
    with pytest.raises(EngineError, match="max_len 2"):
        tok.encode_pairs(["a"], ["a"])
    tok.max_length = 3
    ids, off, seg = tok.encode_pairs(["a"], ["a a"])
    assert ids.tolist() == [1, 2, 2] and seg.tolist() == [2]
    ids, off, seg = tok.encode_pairs([], [])
    assert ids.size == 0 and off.tolist() == [0] and seg.size == 0
    with pytest.raises(ValueError):
        tok.encode_pairs(["a"], [])


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_oracle_matches_golden(path):
    g = np.load(path)
    L, H, nh, inter, vocab, max_pos, tv = (int(x) for x in g["shape"])
    shape = obert.BertShape(L, H, nh, inter, vocab=vocab, max_pos=max_pos, type_vocab=tv, eps=float(g["eps"]))
    w = ro.random_weights(shape, int(g["seed"]), float(g["cls_scale"]), float(g["cls_bias"]))
    got = ro.logits(w, shape, g["ids"], g["offsets"], g["seg_b"])
    want = g["logits"]
    assert want.min() <= -3 and want.max() >= 3  # a bar means something only over a spread of logits
    assert np.abs(got - want).max() <= 1e-5, np.abs(got - want).max()


def test_golden_pairs_are_what_the_native_tokeniser_makes():
    from voitta_rag_amd.wordpiece import WordPieceTokenizer

    for path in GOLDEN:
        g = np.load(path)
        co = g["cand_off"]
        a = [str(q) for q, c in zip(g["queries"], np.diff(co)) for _ in range(c)]
        tok = WordPieceTokenizer([str(v) for v in g["vocab"]], max_length=int(g["max_len"]))
        ids, off, seg = tok.encode_pairs(a, [str(p) for p in g["passages"]])
        assert ids.tolist() == g["ids"].tolist() and off.tolist() == g["offsets"].tolist()
        assert seg.tolist() == g["seg_b"].tolist()


def _checkpoint(tmp_path, **cfg):
    base = {"architectures": ["BertForSequenceClassification"], "model_type": "bert", "num_hidden_layers": 1,
            "hidden_size": 128, "num_attention_heads": 2, "intermediate_size": 256, "vocab_size": 10,
            "max_position_embeddings": 32, "id2label": {"0": "LABEL_0"}}
    base.update(cfg)
    (tmp_path / "config.json").write_text(json.dumps(base))
    return str(tmp_path)


def test_read_config_refusals(tmp_path):
    from voitta_rag_amd.reranker import read_config

    assert read_config(_checkpoint(tmp_path))["hidden_size"] == 128
    with pytest.raises(ValueError, match="BertForSequenceClassification"):
        read_config(_checkpoint(tmp_path, architectures=["XLMRobertaForSequenceClassification"], model_type="xlm-roberta"))
    with pytest.raises(ValueError, match="BertForSequenceClassification"):
        read_config(_checkpoint(tmp_path, architectures=["BertModel"]))
    with pytest.raises(ValueError, match="2 labels"):
        read_config(_checkpoint(tmp_path, id2label={"0": "no", "1": "yes"}))
    with pytest.raises(ValueError, match="3 labels"):
        read_config(_checkpoint(tmp_path, num_labels=3))


def test_rerank_candidates_clamp():
    from voitta_rag_amd.reranker import rerank_candidates

    assert rerank_candidates(50, 10) == 50
    assert rerank_candidates(5, 10) == 10
    assert rerank_candidates(1000, 10) == 341


def test_library_exports_and_declares():
    from voitta_rag_amd import _lib

    lib = _lib.load_library()
    for name in ("vr_wordpiece_encode_pairs", "vr_reranker_load", "vr_rerank", "vr_rerank_text"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.vr_abi_version() == 1


def _err(lib):
    return lib.vr_last_error().decode()


def test_argument_errors_before_engine_work():
    from voitta_rag_amd import _lib

    lib = _lib.load_library()
    q = (C.c_char_p * 2)(b"question", b"other")
    ql = np.array([8, 5], np.int64)
    p = (C.c_char_p * 3)(b"p0", b"p1", b"p2")
    pl = np.array([2, 2, 2], np.int64)
    out = np.zeros(3, np.float32)
    i64 = C.POINTER(C.c_int64)

    def call(cand_off, max_len=32, qlens=ql, plens=pl, n=2, tok=1):
        co = np.asarray(cand_off, np.int64)
        return lib.vr_rerank_text(None, tok, n, q, qlens.ctypes.data_as(i64), co.ctypes.data_as(i64), p,
                                  plens.ctypes.data_as(i64), max_len, out.ctypes.data_as(C.POINTER(C.c_float)))

    assert call([0, 2, 3]) != 0 and _err(lib) == "null engine"  # valid input reaches the engine check
    assert call([0, 0, 0]) != 0 and _err(lib) == "null engine"  # questions without candidates are valid
    assert call([1, 2, 3]) != 0 and "cand_off[0]" in _err(lib)
    assert call([0, 2, 1]) != 0 and "decreases" in _err(lib)
    assert call([0, 2, 3], max_len=2) != 0 and "max_len" in _err(lib)
    assert call([0, 2, 3], qlens=np.array([8, -1], np.int64)) != 0 and "query 1" in _err(lib)
    assert call([0, 2, 3], plens=np.array([2, -2, 2], np.int64)) != 0 and "passage 1" in _err(lib)
    assert call([0, 2, 3], n=-1) != 0 and "bad arguments" in _err(lib)
    assert call([0, 2, 3], tok=None) != 0 and "bad arguments" in _err(lib)
    ids = np.zeros(4, np.int32)
    off = np.array([0, 4], np.int32)
    seg = np.array([2], np.int32)
    assert lib.vr_rerank(None, ids.ctypes.data, off.ctypes.data, seg.ctypes.data, 1, 0, out.ctypes.data, 0) != 0
    assert _err(lib) == "null engine"
    assert lib.vr_rerank(None, ids.ctypes.data, off.ctypes.data, None, 1, 0, out.ctypes.data, 0) != 0
    assert "bad arguments" in _err(lib)
    assert lib.vr_rerank(None, ids.ctypes.data, off.ctypes.data, seg.ctypes.data, 1, 7, out.ctypes.data, 0) != 0
    assert "bad mem" in _err(lib)
