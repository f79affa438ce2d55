"""TEST INFRASTRUCTURE — what transformers' XLMRobertaModel / one-label XLMRobertaForSequenceClassification compute,
restated on top of oracle/bert.py (unchanged) [EXT, transformers' published behaviour]:
  positions  : token p of an unpadded sequence reads position row pad_token_id + 1 + p (XLM-R numbers positions from
               padding_idx + 1; pad_token_id = 1), so the encoder is oracle.bert on rows [2:] of the position table
  token type : one row (type_vocab_size = 1), every token reads it
  head       : logit = out_proj . tanh(dense h_<s> + b) + b_out (classifier.dense / classifier.out_proj)
Pinned against transformers itself by tests/golden/make_xlmr_golden.py -> tests/golden/xlmr_*.npz."""
from __future__ import annotations

import json
import math
from dataclasses import replace

import numpy as np

from oracle import bert as obert

PAD = 1  # pad_token_id of every XLM-R checkpoint
# a hand-made vocabulary with equal path scores: '▁ab' = '▁a' + 'b' = '▁' + 'ab' (-3); 'c' is missing (fused unknowns)
TIE_VOCAB = [["<s>", 0.0], ["<pad>", 0.0], ["</s>", 0.0], ["<unk>", 0.0], ["▁", -1.0], ["a", -1.0], ["b", -1.0],
             ["ab", -2.0], ["▁a", -2.0], ["▁ab", -3.0], ["ba", -2.0], ["▁b", -2.0], ["<mask>", 0.0]]
TOKENIZER_CASES = ["metaspace", "whitespace_metaspace", "no_charsmap", "ties"]


def tokenizer_spec(fixture: dict, case: str) -> dict:
    """The tokenizer.json of one case of tests/golden/xlmr_tokenizer.json, derived from the one stored there (the
    hub files' shape: Sequence[Precompiled, Replace(" {2,}", " ")], Metaspace):
      whitespace_metaspace  transformers 5's shape: Precompiled alone, Sequence[WhitespaceSplit, Metaspace]
      no_charsmap           Replace alone
      ties                  TIE_VOCAB as the Unigram vocabulary"""
    spec = json.loads(json.dumps(fixture["tokenizer"]))
    if case == "whitespace_metaspace":
        spec["normalizer"] = spec["normalizer"]["normalizers"][0]
        spec["pre_tokenizer"] = {"type": "Sequence", "pretokenizers": [{"type": "WhitespaceSplit"}, spec["pre_tokenizer"]]}
    elif case == "no_charsmap":
        spec["normalizer"]["normalizers"] = spec["normalizer"]["normalizers"][1:]
    elif case == "ties":
        spec["model"]["vocab"] = [list(v) for v in TIE_VOCAB]
        for at in spec["added_tokens"]:
            at["id"] = [v[0] for v in TIE_VOCAB].index(at["content"])
    else:
        assert case == "metaspace", case
    return spec


HEAD_KEYS = ["classifier.dense.weight", "classifier.dense.bias", "classifier.out_proj.weight", "classifier.out_proj.bias"]


def random_weights(shape: obert.BertShape, seed: int, head: bool = False) -> dict:
    """oracle.bert.random_weights (max_pos = max_position_embeddings, e.g. 514; type_vocab 1) plus, with head, a seeded
    classification head in XLMRobertaClassificationHead naming."""
    w = obert.random_weights(shape, seed)
    if head:
        rng = np.random.default_rng(seed + 500)
        H = shape.hidden
        w["classifier.dense.weight"] = rng.normal(0, 1.0 / math.sqrt(H), (H, H)).astype(np.float32)
        w["classifier.dense.bias"] = rng.normal(0, 0.1, H).astype(np.float32)
        w["classifier.out_proj.weight"] = (rng.normal(0, 4.0 / math.sqrt(H), (1, H))).astype(np.float32)
        w["classifier.out_proj.bias"] = np.array([0.25], np.float32)
    return w


def bert_view(w: dict, shape: obert.BertShape) -> tuple[dict, obert.BertShape]:
    """The same model as a BERT whose position p is XLM-R's position PAD + 1 + p."""
    v = dict(w)
    v[obert.EMB_KEYS["pos"]] = w[obert.EMB_KEYS["pos"]][PAD + 1:]
    return v, replace(shape, max_pos=shape.max_pos - PAD - 1)


def embeddings(w: dict, shape: obert.BertShape, seqs, pooling: str = "mean", normalize: bool = True) -> np.ndarray:
    v, s = bert_view(w, shape)
    return obert.sentence_embeddings(v, s, seqs, pooling, normalize, np.float64)


def logits(w: dict, shape: obert.BertShape, ids, offsets) -> np.ndarray:
    """One f64 logit per packed pair sequence."""
    v, s = bert_view(w, shape)
    n = len(offsets) - 1
    cls = np.stack([obert.encode_one(v, s, ids[offsets[i]:offsets[i + 1]])[0] for i in range(n)])
    W = lambda k: w[k].astype(np.float64)  # noqa: E731
    pooled = np.tanh(cls @ W("classifier.dense.weight").T + W("classifier.dense.bias"))
    return pooled @ W("classifier.out_proj.weight")[0] + W("classifier.out_proj.bias")[0]
