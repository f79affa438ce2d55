"""TEST INFRASTRUCTURE — NumPy f64 restatement of transformers' NomicBertModel (model_type nomic_bert: a BERT with
rotary positions and a gated feed-forward block, no biases in its projections) [EXT, transformers' published behaviour]:
  embeddings : LayerNorm(word[id] + token_type[0]) — no position table
  per layer  : q, k, v = x W^T; q and k of every head rotated by the token's position p inside its sequence,
               rotate-half pairing: x[j] cos(p f_j) - x[j + d/2] sin(p f_j), x[j + d/2] cos(p f_j) + x[j] sin(p f_j),
               f_j = theta^(-2j/d_h), j < d_h/2; softmax(q k^T / sqrt(d_h)) v
               x = LayerNorm(ctx W_o^T + x)
               x = LayerNorm((act(x W_gate^T) * (x W_up^T)) W_down^T + x), act = SiLU ("silu") or exact-erf GELU ("gelu")
  pooling / normalize : as oracle.bert
transformers computes the cos/sin table in f32 whatever the model's dtype (f32 inv_freq: 3e-5 rad off at position
511; f32 cos / sin), and a table that differs from it in the last f32 bit of some entries already moves a 12-layer
embedding by 1e-8. The goldens of tests/golden/make_rope_golden.py therefore record the table transformers used
(rope_cos / rope_sin), and `table=(cos, sin)` makes the oracle use it in place of its own exact one: that is how the
oracle is pinned to 1e-9. Everywhere else (the GPU tests, whose engine builds its table in f64) the exact table is used.
Weights are seeded and never stored; tensors the family shares with BERT follow oracle.bert.random_weights' scales."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from oracle import bert as obert


@dataclass
class RopeShape:
    layers: int
    hidden: int
    heads: int
    intermediate: int
    vocab: int = 30528
    max_pos: int = 2048
    type_vocab: int = 2
    eps: float = 1e-12
    theta: float = 1000.0
    act: str = "silu"  # "silu" (SwiGLU) | "gelu" (GeGLU)


EMB_KEYS = {"word": "embeddings.word_embeddings.weight", "type": "embeddings.token_type_embeddings.weight",
            "ln_g": "embeddings.LayerNorm.weight", "ln_b": "embeddings.LayerNorm.bias"}


def layer_keys(i: int) -> dict[str, str]:
    p = f"layers.{i}."
    return {"q_w": p + "self_attn.q_proj.weight", "k_w": p + "self_attn.k_proj.weight", "v_w": p + "self_attn.v_proj.weight",
            "o_w": p + "self_attn.o_proj.weight", "ln1_g": p + "post_attention_layernorm.weight",
            "ln1_b": p + "post_attention_layernorm.bias", "gate_w": p + "mlp.gate_proj.weight",
            "up_w": p + "mlp.up_proj.weight", "down_w": p + "mlp.down_proj.weight",
            "ln2_g": p + "post_mlp_layernorm.weight", "ln2_b": p + "post_mlp_layernorm.bias"}


def random_weights(shape: RopeShape, seed: int, std: float = 0.02, gate_std: float | None = None) -> dict[str, np.ndarray]:
    """Seeded weights in the native NomicBertModel naming: matrices N(0, 2.5 std), LayerNorm gains 1 + N(0, 0.1) and
    shifts N(0, 0.1), embeddings N(0, std) — oracle.bert.random_weights' scales for every tensor the families share.
    The gate projection, which BERT does not have, is N(0, std). Why not 2.5 std as well: the block is bias-free and
    multiplicative, d(act(g) u) = act'(g) u dg + act(g) du, and with g = W_gate x of unit variance (2.5 std at H = 384)
    a perturbation of the hidden state grows ~1.3x per layer through LayerNorm(x + FFN(x)), ~24x over 12 layers (BERT's
    fixtures: ~1.03x per layer). Such a model measures its own instability: evaluated in f64 NumPy with nothing but the
    GEMM operands rounded to f16 once — what any f16-operand engine does at best — the 12-layer golden shape is already
    3e-5 .. 1e-4 off in |1 - cos|, ten times the bar the f16 precision is held to; with N(0, std) the growth is ~1.06x
    per layer and the same evaluation gives 1e-6 .. 2e-6, the BERT fixtures' level. Both figures are reproduced by
    tests/test_rope_cpu.py::test_gate_scale_of_the_fixture (gate_std selects the scale; encode_one(operand=...) is that
    evaluation)."""
    rng = np.random.default_rng(seed)
    H, I = shape.hidden, shape.intermediate
    w = {EMB_KEYS["word"]: rng.normal(0, std, (shape.vocab, H)), EMB_KEYS["type"]: rng.normal(0, std, (shape.type_vocab, H)),
         EMB_KEYS["ln_g"]: 1.0 + rng.normal(0, 0.1, H), EMB_KEYS["ln_b"]: rng.normal(0, 0.1, H)}
    for i in range(shape.layers):
        k = layer_keys(i)
        for n, shp in (("q", (H, H)), ("k", (H, H)), ("v", (H, H)), ("o", (H, H)), ("gate", (I, H)), ("up", (I, H)),
                       ("down", (H, I))):
            w[k[n + "_w"]] = rng.normal(0, (std if gate_std is None else gate_std) if n == "gate" else std * 2.5, shp)
        for n in ("ln1", "ln2"):
            w[k[n + "_g"]] = 1.0 + rng.normal(0, 0.1, H)
            w[k[n + "_b"]] = rng.normal(0, 0.1, H)
    return {k: v.astype(np.float32) for k, v in w.items()}


def hub_state(w: dict, layers: int) -> dict:
    """The same weights under the hub checkpoint's names, q/k/v fused into attn.Wqkv."""
    out = {EMB_KEYS["word"]: w[EMB_KEYS["word"]], EMB_KEYS["type"]: w[EMB_KEYS["type"]],
           "emb_ln.weight": w[EMB_KEYS["ln_g"]], "emb_ln.bias": w[EMB_KEYS["ln_b"]]}
    for i in range(layers):
        k, p = layer_keys(i), f"encoder.layers.{i}."
        out[p + "attn.Wqkv.weight"] = np.concatenate([w[k["q_w"]], w[k["k_w"]], w[k["v_w"]]], axis=0)
        out[p + "attn.out_proj.weight"] = w[k["o_w"]]
        out[p + "mlp.fc11.weight"], out[p + "mlp.fc12.weight"], out[p + "mlp.fc2.weight"] = w[k["up_w"]], w[k["gate_w"]], w[k["down_w"]]
        out[p + "norm1.weight"], out[p + "norm1.bias"] = w[k["ln1_g"]], w[k["ln1_b"]]
        out[p + "norm2.weight"], out[p + "norm2.bias"] = w[k["ln2_g"]], w[k["ln2_b"]]
    return out


def rope_table(S: int, dh: int, theta: float):
    """cos, sin [S, dh/2] of angle p * theta^(-2j/dh), f64."""
    j = np.arange(0, dh, 2)
    ang = np.arange(S, dtype=np.float64)[:, None] * (float(theta) ** (-j.astype(np.float64) / dh))[None, :]
    return np.cos(ang), np.sin(ang)


def _rotate(x, cos, sin):
    """x [heads, S, dh]: rotate-half pairing."""
    half = x.shape[-1] // 2
    a, b = x[..., :half], x[..., half:]
    return np.concatenate([a * cos - b * sin, b * cos + a * sin], axis=-1)


def _act(x, act: str):
    if act == "silu":
        return x / (1.0 + np.exp(-x))
    assert act == "gelu", act
    return obert._gelu(x)


def f16_operand(x):
    """x rounded to f16 once, as f64: what an f16-operand matrix product reads."""
    return np.asarray(x).astype(np.float16).astype(np.float64)


def encode_one(w: dict, shape: RopeShape, ids, table=None, operand=None, hooks=None) -> np.ndarray:
    """last_hidden_state [S, H] of one unpadded sequence, f64. table: (cos, sin) [>= S, d_h/2] to use instead of
    rope_table's. operand (e.g. f16_operand): applied to both operands of every matrix product (weights, hidden state,
    rotated q / k, v, context, gated activation) while everything else stays f64 — the best an engine whose products
    read f16 operands can do. hooks: deliberate mistakes of tests/encoder_family_rows_case.py, a dict of "rotate"
    f(x [heads, S, d_h], "q" | "k", layer) in place of the rotation, "glu" f(gate, up, layer) in place of
    act(gate) * up, and "stale_residual" (the FFN's residual taken from before the attention block's LayerNorm); without
    it nothing changes."""
    hk = hooks or {}
    rot = hk["rotate"] if "rotate" in hk else (lambda t, kind, layer: _rotate(t, cos, sin))  # noqa: E731
    glu = hk["glu"] if "glu" in hk else (lambda gate, up, layer: _act(gate, shape.act) * up)  # noqa: E731
    r = operand or (lambda v: v)  # noqa: E731
    W = lambda k: r(w[k].astype(np.float64))  # noqa: E731  (a projection matrix)
    P = lambda k: w[k].astype(np.float64)  # noqa: E731  (embeddings, LayerNorm parameters: no product reads them)
    ids = np.asarray(ids, dtype=np.int64)
    S, H, nh = len(ids), shape.hidden, shape.heads
    dh = H // nh
    cos, sin = rope_table(S, dh, shape.theta) if table is None else (np.asarray(table[0], np.float64)[:S],
                                                                      np.asarray(table[1], np.float64)[:S])
    x = obert._ln(P(EMB_KEYS["word"])[ids] + P(EMB_KEYS["type"])[0], P(EMB_KEYS["ln_g"]), P(EMB_KEYS["ln_b"]), shape.eps)
    for i in range(shape.layers):
        k = layer_keys(i)
        xa = r(x)
        q = r(rot((xa @ W(k["q_w"]).T).reshape(S, nh, dh).transpose(1, 0, 2), "q", i))
        kk = r(rot((xa @ W(k["k_w"]).T).reshape(S, nh, dh).transpose(1, 0, 2), "k", i))
        v = r((xa @ W(k["v_w"]).T).reshape(S, nh, dh).transpose(1, 0, 2))
        s = q @ kk.transpose(0, 2, 1) / math.sqrt(dh)
        s = s - s.max(axis=-1, keepdims=True)
        p = np.exp(s)
        p = p / p.sum(axis=-1, keepdims=True)
        ctx = r((p @ v).transpose(1, 0, 2).reshape(S, H))
        before = x
        x = obert._ln(ctx @ W(k["o_w"]).T + x, P(k["ln1_g"]), P(k["ln1_b"]), shape.eps)
        xa = r(x)
        h = r(glu(xa @ W(k["gate_w"]).T, xa @ W(k["up_w"]).T, i))
        x = obert._ln(h @ W(k["down_w"]).T + (before if hk.get("stale_residual") else x), P(k["ln2_g"]), P(k["ln2_b"]), shape.eps)
    return x


def sentence_embeddings(w: dict, shape: RopeShape, seqs, pooling: str = "mean", normalize: bool = True,
                        table=None) -> np.ndarray:
    out = np.zeros((len(seqs), shape.hidden), dtype=np.float64)
    for i, ids in enumerate(seqs):
        h = encode_one(w, shape, ids, table)
        e = h[0] if pooling == "cls" else h.sum(axis=0) / max(float(len(ids)), 1e-9)
        if normalize:
            e = e / max(float(np.sqrt((e * e).sum())), 1e-12)
        out[i] = e
    return out


def desc_for(shape: RopeShape, pooling: str, precision: str, max_pos: int | None = None):
    """The engine's description of `shape`."""
    from voitta_rag_amd import encoder as enc

    return enc.BertDesc(shape.layers, shape.hidden, shape.heads, shape.intermediate, vocab=shape.vocab,
                        max_pos=max_pos or shape.max_pos, type_vocab=shape.type_vocab, pooling=pooling, normalize=True,
                        eps=shape.eps, precision=precision, position="rotary", rope_theta=shape.theta,
                        ffn="swiglu" if shape.act == "silu" else "geglu")
