"""TEST INFRASTRUCTURE — NumPy f64 restatement of JinaBertModel (jina-embeddings-v2-small-en / -base-en: config.json
model_type bert, position_embedding_type alibi, feed_forward_type geglu) [EXT, the published model code's behaviour]:
a post-LayerNorm BERT with no position in its embeddings, a linear attention bias per head, and a gated FFN.
  embeddings : h = LayerNorm(word[id] + token_type[0])
  per layer  : s[h, i, j] = q_i . k_j / sqrt(d_h) - m_h |j - i|;  p = softmax_j(s);  h = LN(W_o (p v) + h)
               "geglu": g = W_gated h (no bias), rows [0, I) the gate and [I, 2I) the up projection;
                        h = LN(W_wo (gelu(gate) * up) + b_wo + h)
               "gelu" : h = LN(W_f gelu(W_i h + b_i) + b_f + h), BERT's block under BERT's names — so that this oracle
                        can be tied to oracle.bert and tests/mpnet_oracle.py, which transformers goldens pin
  result     : h, pooled (mean or first row) and L2-normalised
m_h: the ALiBi slopes (voitta_rag_amd.encoder.alibi_slopes for the model's own; any [heads] array here). JinaBert's
code is not part of transformers, so no golden of the published implementation exists; tests/test_alibi_cpu.py ties the
pieces to oracles that have one. Weights are seeded and never stored: oracle.bert's scales, the gate rows N(0, std) as
in tests/rope_oracle.py (whose docstring says why)."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from oracle import bert as obert


@dataclass
class AlibiShape:
    layers: int
    hidden: int
    heads: int
    intermediate: int
    vocab: int = 300
    max_pos: int = 8192  # max_position_embeddings: no table, the longest sequence alone
    type_vocab: int = 2
    eps: float = 1e-12
    ffn: str = "geglu"  # "geglu" (JinaBert) | "gelu" (BERT's block)


EMB_KEYS = {"word": "embeddings.word_embeddings.weight", "type": "embeddings.token_type_embeddings.weight",
            "ln_g": "embeddings.LayerNorm.weight", "ln_b": "embeddings.LayerNorm.bias"}


def layer_keys(i: int, ffn: str = "geglu") -> dict[str, str]:
    p = f"encoder.layer.{i}."
    k = {}
    for short, name in (("q", "attention.self.query"), ("k", "attention.self.key"), ("v", "attention.self.value"),
                        ("o", "attention.output.dense")):
        k[short + "_w"], k[short + "_b"] = p + name + ".weight", p + name + ".bias"
    k["ln1_g"], k["ln1_b"] = p + "attention.output.LayerNorm.weight", p + "attention.output.LayerNorm.bias"
    if ffn == "geglu":
        k["gated_w"] = p + "mlp.gated_layers.weight"
        k["f_w"], k["f_b"] = p + "mlp.wo.weight", p + "mlp.wo.bias"
        k["ln2_g"], k["ln2_b"] = p + "mlp.layernorm.weight", p + "mlp.layernorm.bias"
    else:
        k["i_w"], k["i_b"] = p + "intermediate.dense.weight", p + "intermediate.dense.bias"
        k["f_w"], k["f_b"] = p + "output.dense.weight", p + "output.dense.bias"
        k["ln2_g"], k["ln2_b"] = p + "output.LayerNorm.weight", p + "output.LayerNorm.bias"
    return k


def random_weights(shape: AlibiShape, seed: int, std: float = 0.02) -> dict[str, np.ndarray]:
    """Seeded weights under JinaBertModel's names (no prefix; "gelu": BertModel's, without a position table)."""
    rng = np.random.default_rng(seed)
    H, I = shape.hidden, shape.intermediate
    w = {EMB_KEYS["word"]: rng.normal(0, std, (shape.vocab, H)), EMB_KEYS["type"]: rng.normal(0, std, (shape.type_vocab, H)),
         EMB_KEYS["ln_g"]: 1.0 + rng.normal(0, 0.1, H), EMB_KEYS["ln_b"]: rng.normal(0, 0.1, H)}
    for i in range(shape.layers):
        k = layer_keys(i, shape.ffn)
        for n in "qkvo":
            w[k[n + "_w"]] = rng.normal(0, std * 2.5, (H, H))
            w[k[n + "_b"]] = rng.normal(0, 0.05, H)
        if shape.ffn == "geglu":
            w[k["gated_w"]] = np.concatenate([rng.normal(0, std, (I, H)), rng.normal(0, std * 2.5, (I, H))], axis=0)
        else:
            w[k["i_w"]], w[k["i_b"]] = rng.normal(0, std * 2.5, (I, H)), rng.normal(0, 0.05, I)
        w[k["f_w"]], w[k["f_b"]] = rng.normal(0, std * 2.5, (H, I)), rng.normal(0, 0.05, H)
        for n in ("ln1", "ln2"):
            w[k[n + "_g"]] = 1.0 + rng.normal(0, 0.1, H)
            w[k[n + "_b"]] = rng.normal(0, 0.1, H)
    return {k: v.astype(np.float32) for k, v in w.items()}


def distance_bias(slopes, S: int, clamp: int | None = None) -> np.ndarray:
    """[heads, S, S]: entry [h, i, j] = -slopes[h] |j - i|, f64. clamp: the distance saturated there — the mistake of a
    kernel that reads a table (for the proof that a test sees it)."""
    pos = np.arange(S, dtype=np.float64)
    d = np.abs(pos[None, :] - pos[:, None])
    if clamp is not None:
        d = np.minimum(d, clamp)
    return -np.asarray(slopes, np.float64)[:, None, None] * d[None]


def encode_one(w: dict, shape: AlibiShape, ids, slopes, bias=None, operand=None, hooks=None) -> np.ndarray:
    """last_hidden_state [S, H] of one unpadded sequence, f64. slopes: [heads], or None for no bias. bias: a ready
    [heads, S, S] array instead (distance_bias with a mistake built in). operand: as oracle.bert.encode_one's. hooks:
    deliberate mistakes of tests/encoder_family_rows_case.py, a dict of "glu" f(gate, up, layer) in place of
    gelu(gate) * up and "stale_residual" (the FFN's residual taken from before the attention block's LayerNorm); without
    it nothing changes."""
    hk = hooks or {}
    glu = hk["glu"] if "glu" in hk else (lambda gate, up, layer: obert._gelu(gate) * up)  # noqa: E731
    r = operand or (lambda a: a)  # noqa: E731
    product = lambda k: w[k].ndim == 2 and k.startswith("encoder.layer.")  # noqa: E731  (a projection matrix)
    W = lambda k: r(w[k].astype(np.float64)) if product(k) else w[k].astype(np.float64)  # noqa: E731
    ids = np.asarray(ids, dtype=np.int64)
    S, H, nh, I = len(ids), shape.hidden, shape.heads, shape.intermediate
    dh = H // nh
    if bias is None and slopes is not None:
        bias = distance_bias(slopes, S)
    x = obert._ln(W(EMB_KEYS["word"])[ids] + W(EMB_KEYS["type"])[0], W(EMB_KEYS["ln_g"]), W(EMB_KEYS["ln_b"]), shape.eps)
    for i in range(shape.layers):
        k = layer_keys(i, shape.ffn)
        xa = r(x)
        q, kk, v = (r((xa @ W(k[n + "_w"]).T + W(k[n + "_b"])).reshape(S, nh, dh).transpose(1, 0, 2)) for n in "qkv")
        s = q @ kk.transpose(0, 2, 1) / math.sqrt(dh)
        ctx = r(obert.attend(s, v, bias, operand).transpose(1, 0, 2).reshape(S, H))
        before = x
        x = obert._ln(ctx @ W(k["o_w"]).T + W(k["o_b"]) + x, W(k["ln1_g"]), W(k["ln1_b"]), shape.eps)
        if shape.ffn == "geglu":
            g = r(x) @ W(k["gated_w"]).T
            h = r(glu(g[:, :I], g[:, I:], i))
        else:
            h = r(obert._gelu(r(x) @ W(k["i_w"]).T + W(k["i_b"])))
        x = obert._ln(h @ W(k["f_w"]).T + W(k["f_b"]) + (before if hk.get("stale_residual") else x), W(k["ln2_g"]),
                      W(k["ln2_b"]), shape.eps)
    return x


def pool(h, pooling: str, normalize: bool = True):
    e = h[0] if pooling == "cls" else h.sum(axis=0) / max(float(len(h)), 1e-9)
    return e / max(float(np.sqrt((e * e).sum())), 1e-12) if normalize else e


def sentence_embeddings(w: dict, shape: AlibiShape, seqs, slopes, pooling: str = "mean") -> np.ndarray:
    return np.stack([pool(encode_one(w, shape, ids, slopes), pooling) for ids in seqs])


def desc_for(shape: AlibiShape, pooling: str, precision: str, max_pos: int | None = None, **over):
    """The engine's description of `shape`: no positions; the slopes are not part of it (attention_slopes=... in `over`
    makes load_encoder set them)."""
    from voitta_rag_amd import encoder as enc

    fields = dict(vocab=shape.vocab, max_pos=max_pos or shape.max_pos, type_vocab=shape.type_vocab, pooling=pooling,
                  normalize=True, eps=shape.eps, precision=precision, position="none", ffn=shape.ffn)
    fields.update(over)
    return enc.BertDesc(shape.layers, shape.hidden, shape.heads, shape.intermediate, **fields)
