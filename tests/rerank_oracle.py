"""TEST INFRASTRUCTURE — f64 NumPy restatement of a one-label BertForSequenceClassification cross-encoder (what
sentence-transformers' CrossEncoder.predict computes before its sigmoid) [EXT, transformers' published behaviour]:
  embeddings : LayerNorm(word[id] + position[p] + token_type[t]), t = 0 for [CLS] A [SEP], 1 for B [SEP]
  encoder    : the layers of oracle/bert.py (each pair unpadded: padding never contributes)
  head       : pooled = tanh(Wp h_CLS + bp); logit = wc . pooled + bc
oracle/bert.py fixes the token type at 0, so the embedding step is restated here; the layers are the same arithmetic.
Pinned against transformers itself by tests/golden/make_rerank_golden.py -> tests/golden/rerank_*.npz."""
from __future__ import annotations

import math

import numpy as np

from oracle import bert as obert

HEAD_KEYS = ["pooler.dense.weight", "pooler.dense.bias", "classifier.weight", "classifier.bias"]


def random_weights(shape: obert.BertShape, seed: int, cls_scale: float = 1.0, cls_bias: float = 0.0) -> dict:
    """oracle.bert.random_weights plus a seeded pooler and classifier; the classifier row is scaled by cls_scale and its
    bias is cls_bias (the golden fixtures store both, chosen so that the logits spread over several units)."""
    w = obert.random_weights(shape, seed)
    rng = np.random.default_rng(seed + 500)
    H = shape.hidden
    w["pooler.dense.weight"] = rng.normal(0, 1.0 / math.sqrt(H), (H, H)).astype(np.float32)
    w["pooler.dense.bias"] = rng.normal(0, 0.1, H).astype(np.float32)
    w["classifier.weight"] = (rng.normal(0, 1.0 / math.sqrt(H), (1, H)) * cls_scale).astype(np.float32)
    w["classifier.bias"] = np.array([cls_bias], np.float32)
    return w


def last_hidden(w: dict, shape: obert.BertShape, ids, seg_b: int) -> np.ndarray:
    """last_hidden_state [S, H] of one unpadded pair sequence, in f64."""
    W = lambda k: w[k].astype(np.float64)  # noqa: E731
    ids = np.asarray(ids, dtype=np.int64)
    S, H, nh = len(ids), shape.hidden, shape.heads
    dh = H // nh
    types = (np.arange(S) >= seg_b).astype(np.int64)
    x = W(obert.EMB_KEYS["word"])[ids] + W(obert.EMB_KEYS["pos"])[:S] + W(obert.EMB_KEYS["type"])[types]
    x = obert._ln(x, W(obert.EMB_KEYS["ln_g"]), W(obert.EMB_KEYS["ln_b"]), shape.eps)
    for i in range(shape.layers):
        k = obert.layer_keys(i)
        q = (x @ W(k["q_w"]).T + W(k["q_b"])).reshape(S, nh, dh).transpose(1, 0, 2)
        kk = (x @ W(k["k_w"]).T + W(k["k_b"])).reshape(S, nh, dh).transpose(1, 0, 2)
        v = (x @ W(k["v_w"]).T + W(k["v_b"])).reshape(S, nh, dh).transpose(1, 0, 2)
        s = q @ kk.transpose(0, 2, 1) / math.sqrt(dh)
        s = s - s.max(axis=-1, keepdims=True)
        p = np.exp(s)
        p = p / p.sum(axis=-1, keepdims=True)
        ctx = (p @ v).transpose(1, 0, 2).reshape(S, H)
        x = obert._ln(ctx @ W(k["o_w"]).T + W(k["o_b"]) + x, W(k["ln1_g"]), W(k["ln1_b"]), shape.eps)
        h = obert._gelu(x @ W(k["i_w"]).T + W(k["i_b"]))
        x = obert._ln(h @ W(k["f_w"]).T + W(k["f_b"]) + x, W(k["ln2_g"]), W(k["ln2_b"]), shape.eps)
    return x


def head(w: dict, cls_rows: np.ndarray) -> np.ndarray:
    """[n, H] last-layer [CLS] rows -> n logits, f64."""
    W = lambda k: w[k].astype(np.float64)  # noqa: E731
    pooled = np.tanh(cls_rows @ W("pooler.dense.weight").T + W("pooler.dense.bias"))
    return pooled @ W("classifier.weight")[0] + W("classifier.bias")[0]


def logits(w: dict, shape: obert.BertShape, ids, offsets, seg_b) -> np.ndarray:
    """One f64 logit per packed pair sequence (ids / offsets / seg_b as vr_rerank takes them)."""
    n = len(offsets) - 1
    cls = np.stack([last_hidden(w, shape, ids[offsets[i]:offsets[i + 1]], int(seg_b[i]))[0] for i in range(n)]) if n else \
        np.zeros((0, shape.hidden))
    return head(w, cls)
