"""TEST INFRASTRUCTURE — NumPy f64 restatement of a one-label transformers ModernBertForSequenceClassification
[EXT, transformers' published behaviour], on top of modernbert_oracle's body:
  pooled : row 0 of final_norm(h) (classifier_pooling "cls") or the mean of its rows ("mean"); each pair unpadded
  head   : logit = wc . LayerNorm(gelu(Wd pooled + bd)) + bc — head.dense, the exact-erf GELU, head.norm (the body's
           norm_eps), classifier; bd (classifier_bias) and the LayerNorm shift (norm_bias) only where the checkpoint
           has them
Weights are seeded and never stored. With biases=True the checkpoint is one with classifier_bias and norm_bias set:
norm_bias is one switch for every LayerNorm of the model, so the body's norms get seeded shifts as well.
Pinned against transformers itself by tests/golden/make_modernbert_rerank_golden.py -> mbert_rerank_*.npz."""
from __future__ import annotations

import math

import numpy as np

from oracle import bert as obert

import modernbert_oracle as mo

HEAD_KEYS = ["head.dense.weight", "head.dense.bias", "head.norm.weight", "head.norm.bias", "classifier.weight",
             "classifier.bias"]


def random_weights(shape: mo.ModernShape, seed: int, biases: bool, cls_scale: float = 1.0, cls_bias: float = 0.0) -> dict:
    """modernbert_oracle.random_weights plus a seeded head; the classifier row is scaled by cls_scale and its bias is
    cls_bias (the goldens store both, chosen so that the logits spread over several units, as rerank_oracle does).
    biases: head.dense.bias, head.norm.bias and a shift for every LayerNorm of the body."""
    w = mo.random_weights(shape, seed)
    rng = np.random.default_rng(seed + 500)
    H = shape.hidden
    w["head.dense.weight"] = rng.normal(0, 1.0 / math.sqrt(H), (H, H)).astype(np.float32)
    dense_b = rng.normal(0, 0.1, H).astype(np.float32)
    w["head.norm.weight"] = (1.0 + rng.normal(0, 0.1, H)).astype(np.float32)
    norm_b = rng.normal(0, 0.1, H).astype(np.float32)
    w["classifier.weight"] = (rng.normal(0, 1.0 / math.sqrt(H), (1, H)) * cls_scale).astype(np.float32)
    w["classifier.bias"] = np.array([cls_bias], np.float32)
    if biases:
        w["head.dense.bias"], w["head.norm.bias"] = dense_b, norm_b
        for k in [k for k in w if k.endswith("norm.weight") and not k.startswith("head.")]:
            w[k[:-len("weight")] + "bias"] = rng.normal(0, 0.05, H).astype(np.float32)
    return w


def head(w: dict, pooled: np.ndarray, eps: float) -> np.ndarray:
    """[n, H] pooled final-norm rows -> n logits, f64."""
    W = lambda k: w[k].astype(np.float64)  # noqa: E731
    H = pooled.shape[-1]
    x = pooled @ W("head.dense.weight").T + (W("head.dense.bias") if "head.dense.bias" in w else 0.0)
    x = obert._ln(obert._gelu(x), W("head.norm.weight"), W("head.norm.bias") if "head.norm.bias" in w else np.zeros(H), eps)
    return x @ W("classifier.weight")[0] + W("classifier.bias")[0]


def pooled_rows(w: dict, shape: mo.ModernShape, ids, offsets, pooling: str) -> np.ndarray:
    """[n, H]: every packed pair's pooled final-norm row, f64 (exact rotary tables)."""
    n = len(offsets) - 1
    if n == 0:
        return np.zeros((0, shape.hidden))
    return np.stack([mo.pool(mo.encode_one(w, shape, ids[offsets[i]:offsets[i + 1]]), pooling, normalize=False)
                     for i in range(n)])


def logits(w: dict, shape: mo.ModernShape, ids, offsets, pooling: str) -> np.ndarray:
    """One f64 logit per packed pair sequence (ids / offsets as vr_rerank takes them; these models have no seg_b)."""
    return head(w, pooled_rows(w, shape, ids, offsets, pooling), shape.eps)


def desc_for(shape: mo.ModernShape, pooling: str, precision: str, **over):
    """The engine's description of the cross-encoder: modernbert_oracle.desc_for, not normalised."""
    return mo.desc_for(shape, pooling, precision, **dict(dict(normalize=False), **over))
