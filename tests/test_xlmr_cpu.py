"""XLM-RoBERTa without a GPU: the f64 test oracle (oracle.bert on the sliced position table) against the transformers
goldens, the config reading of embedder and cross-encoder checkpoints (position slice, one token type, eps, max length,
the refusal above 512 tokens), and the C-ABI table of the new calls."""
import glob
import json
import os
import re

import numpy as np
import pytest

from oracle import bert as obert

import xlmr_oracle as xo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "xlmr_*.npz")))


def load_case(path):
    g = np.load(path)
    L, H, nh, inter, vocab, max_pos, tv = (int(x) for x in g["shape"])
    shape = obert.BertShape(L, H, nh, inter, vocab=vocab, max_pos=max_pos, type_vocab=tv, eps=float(g["eps"]))
    rerank = "rerank" in os.path.basename(path)
    return g, shape, xo.random_weights(shape, int(g["seed"]), rerank), rerank


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p))
def test_oracle_matches_transformers(path):
    g, shape, w, rerank = load_case(path)
    ids, off = g["ids"], g["offsets"]
    if rerank:
        got = xo.logits(w, shape, ids, off)
    else:
        got = xo.embeddings(w, shape, [ids[off[i]:off[i + 1]] for i in range(len(off) - 1)])
        assert max(np.diff(off)) == 512  # the longest sequence reads the last position row
    assert np.abs(got - g["want"]).max() < 1e-5


def _embedder(d, model_type="xlm-roberta", mpe=514, pad=1, max_seq=None, eps=1e-5):
    os.makedirs(os.path.join(d, "1_Pooling"), exist_ok=True)
    json.dump({"model_type": model_type, "hidden_size": 128, "num_hidden_layers": 1, "num_attention_heads": 2,
               "intermediate_size": 256, "vocab_size": 50, "max_position_embeddings": mpe, "type_vocab_size": 1,
               "layer_norm_eps": eps, "hidden_act": "gelu", "pad_token_id": pad}, open(os.path.join(d, "config.json"), "w"))
    json.dump([{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
               {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
               {"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}],
              open(os.path.join(d, "modules.json"), "w"))
    json.dump({"pooling_mode_mean_tokens": True}, open(os.path.join(d, "1_Pooling", "config.json"), "w"))
    if max_seq is not None:
        json.dump({"max_seq_length": max_seq}, open(os.path.join(d, "sentence_bert_config.json"), "w"))
    return d


def test_embedder_config(tmp_path):
    from voitta_rag_amd.embedding import read_encoder_config, slice_positions

    rc = read_encoder_config(_embedder(str(tmp_path / "a"), max_seq=512))
    d = rc["desc"]
    assert (rc["pos_start"], d.max_pos, d.type_vocab, rc["max_seq"], d.pooling, d.normalize) == (2, 512, 1, 512, "mean", True)
    assert abs(d.eps - 1e-5) < 1e-12
    assert read_encoder_config(_embedder(str(tmp_path / "b")))["max_seq"] == 512  # no sentence_bert_config.json
    assert read_encoder_config(_embedder(str(tmp_path / "c"), max_seq=128))["max_seq"] == 128
    assert read_encoder_config(_embedder(str(tmp_path / "d"), pad=0, mpe=513))["desc"].max_pos == 512
    with pytest.raises(ValueError, match="max_seq_length"):  # bge-m3-like: 8192 usable positions
        read_encoder_config(_embedder(str(tmp_path / "e"), mpe=8194, max_seq=8192))
    with pytest.raises(ValueError, match="max_seq_length"):
        read_encoder_config(_embedder(str(tmp_path / "f"), mpe=8194))
    assert read_encoder_config(_embedder(str(tmp_path / "g"), mpe=8194, max_seq=512))["max_seq"] == 512
    with pytest.raises(ValueError, match="model_type"):
        read_encoder_config(_embedder(str(tmp_path / "h"), model_type="roberta"))
    bert = read_encoder_config(_embedder(str(tmp_path / "i"), model_type="bert", mpe=512, max_seq=256, eps=1e-12))
    assert (bert["pos_start"], bert["desc"].max_pos, bert["max_seq"]) == (0, 512, 256)
    pos = np.arange(514 * 2, dtype=np.float32).reshape(514, 2)
    st = slice_positions({"roberta.embeddings.position_embeddings.weight": pos, "x": pos}, 2)
    assert np.array_equal(st["roberta.embeddings.position_embeddings.weight"], pos[2:]) and st["x"] is pos


def _reranker(d, archs=("XLMRobertaForSequenceClassification",), mpe=514, model_max=512):
    os.makedirs(d, exist_ok=True)
    json.dump({"architectures": list(archs), "model_type": "xlm-roberta", "hidden_size": 128, "num_hidden_layers": 1,
               "num_attention_heads": 2, "intermediate_size": 256, "vocab_size": 50, "max_position_embeddings": mpe,
               "type_vocab_size": 1, "layer_norm_eps": 1e-5, "pad_token_id": 1, "id2label": {"0": "LABEL_0"}},
              open(os.path.join(d, "config.json"), "w"))
    json.dump({"model_max_length": model_max}, open(os.path.join(d, "tokenizer_config.json"), "w"))
    return d


def test_reranker_config(tmp_path):
    from voitta_rag_amd.reranker import NativeCrossEncoder, read_config, read_cross_encoder_config

    assert read_cross_encoder_config(_reranker(str(tmp_path / "a")))["type_vocab_size"] == 1
    with pytest.raises(ValueError, match="BertForSequenceClassification"):
        read_config(str(tmp_path / "a"))  # the BERT reader is unchanged
    with pytest.raises(ValueError, match="XLMRobertaForSequenceClassification"):
        read_cross_encoder_config(_reranker(str(tmp_path / "b"), archs=["XLMRobertaModel"]))
    # bge-reranker-v2-m3-like: 8192 tokens; refused before any weight is read, naming the setting that lowers it
    with pytest.raises(ValueError, match="max_length"):
        NativeCrossEncoder.from_pretrained(_reranker(str(tmp_path / "c"), mpe=8194, model_max=8192))


def test_abi_table_lists_the_unigram_calls():
    from voitta_rag_amd import _lib

    header = open(os.path.join(ROOT, "include", "voitta_engine.h")).read()
    declared = set(re.findall(r"\b(vr_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    new = {"vr_unigram_create", "vr_unigram_destroy", "vr_unigram_encode", "vr_unigram_encode_pairs",
           "vr_query_text_unigram", "vr_query_text_batch_unigram", "vr_rerank_text_unigram"}
    assert new <= declared and new <= set(_lib.SIGNATURES)
    assert declared == set(_lib.SIGNATURES)
    lib = _lib.load_library()
    for name in new:
        assert hasattr(lib, name)


def test_native_unigram_only_for_xlmr_models(tmp_path):
    """An XLM-R model gets the native Unigram tokenizer; a BERT model whose tokenizer.json is a Unigram one
    (paraphrase-multilingual-MiniLM and the like) keeps the tokenizers library, as it did before."""
    tokenizers = pytest.importorskip("tokenizers")
    from voitta_rag_amd.embedding import NativeSentenceEncoder, native_tokenizer
    from voitta_rag_amd.unigram import UnigramTokenizer

    fixture = json.load(open(os.path.join(HERE, "golden", "xlmr_tokenizer.json"), encoding="utf-8"))
    (tmp_path / "tokenizer.json").write_text(json.dumps(xo.tokenizer_spec(fixture, "whitespace_metaspace")),
                                             encoding="utf-8")
    tok = NativeSentenceEncoder._load_tokenizer(str(tmp_path), {"model_type": "xlm-roberta"})
    assert isinstance(tok, UnigramTokenizer) and native_tokenizer(tok)
    tok = NativeSentenceEncoder._load_tokenizer(str(tmp_path), {"model_type": "bert"})
    assert isinstance(tok, tokenizers.Tokenizer) and not native_tokenizer(tok)
    # an XLM-R model whose tokenizer.json is outside the native shape: the library as well
    spec = xo.tokenizer_spec(fixture, "metaspace")
    spec["normalizer"] = {"type": "NFKC"}
    (tmp_path / "tokenizer.json").write_text(json.dumps(spec), encoding="utf-8")
    assert isinstance(NativeSentenceEncoder._load_tokenizer(str(tmp_path), {"model_type": "xlm-roberta"}),
                      tokenizers.Tokenizer)
