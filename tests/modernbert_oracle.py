"""TEST INFRASTRUCTURE — NumPy f64 restatement of transformers' ModernBertModel (model_type modernbert, eager attention)
[EXT, transformers' published behaviour]: a pre-norm encoder with rotary positions, GeGLU and alternating global and
sliding-window attention.
  embeddings : h = LayerNorm(tok[id]) — no position table, no token types
  per layer  : h = h + W_o attn(N_a(h)), N_a = layers.l.attn_norm, the identity in layer 0; q, k, v = rows of Wqkv in
               thirds; q and k rotated (rotate-half pairing, rope_oracle._rotate) with the base of the layer's kind;
               softmax(q k^T / sqrt(d_h)) v over the keys the layer sees: all of the sequence in a global layer
               (l % global_every == 0), keys j with |i - j| <= window in a windowed one
               h = h + W_mlp_o(gelu(a) * b), (a, b) = the first and second I rows of Wi N_m(h), N_m = layers.l.mlp_norm
  result     : final_norm(h); every norm a LayerNorm with the one norm_eps, biases only where the checkpoint has them
`window` is the engine's half-width: transformers' local_attention // 2. As in rope_oracle, transformers computes its
cos/sin tables in f32, and the goldens of tests/golden/make_modernbert_golden.py record them: tables=((cos, sin) of the
global layers, (cos, sin) of the windowed ones) makes the oracle rotate with those. This model's eager path rounds in
two more places whatever the model's dtype: apply_rotary_pos_emb rotates q.float() and k.float(), the query and key
rounded to f32, and eager_attention_forward takes the softmax with dtype=float32. library_f32=True restates both (the softmax
through torch's own f32 kernel, whose exp is not NumPy's to the last bit); that and the recorded tables pin the oracle
to the library at 1e-9. Everywhere else (the GPU tests) the oracle is plain f64 with exact tables: the model, not one
library's roundings of it.
Weights are seeded and never stored, at rope_oracle.random_weights' scales."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle import bert as obert
from rope_oracle import _rotate, f16_operand, rope_table  # noqa: F401  (f16_operand: for callers of encode_one)


@dataclass
class ModernShape:
    layers: int
    hidden: int
    heads: int
    intermediate: int
    vocab: int = 500
    max_pos: int = 512
    eps: float = 1e-5
    theta: float = 160000.0        # global layers
    theta_local: float = 10000.0   # windowed layers
    window: int = 64               # half-width; 0: every layer global
    global_every: int = 3


def is_global(shape: ModernShape, layer: int) -> bool:
    return shape.window == 0 or layer % shape.global_every == 0


def layer_keys(i: int, layers: int) -> dict[str, str]:
    p = f"layers.{i}."
    k = {"qkv_w": p + "attn.Wqkv.weight", "o_w": p + "attn.Wo.weight", "mlp_norm": p + "mlp_norm.weight",
         "wi_w": p + "mlp.Wi.weight", "wo_w": p + "mlp.Wo.weight"}
    if i > 0:
        k["attn_norm"] = p + "attn_norm.weight"
    return k


def random_weights(shape: ModernShape, seed: int, std: float = 0.02) -> dict[str, np.ndarray]:
    """Seeded weights under transformers' ModernBertModel names. Scales as rope_oracle.random_weights: matrices
    N(0, 2.5 std) with the gate half of Wi at N(0, std) (see there why), LayerNorm gains 1 + N(0, 0.1), embeddings
    N(0, std). No biases: the released checkpoints have none."""
    rng = np.random.default_rng(seed)
    H, I = shape.hidden, shape.intermediate
    w = {"embeddings.tok_embeddings.weight": rng.normal(0, std, (shape.vocab, H)),
         "embeddings.norm.weight": 1.0 + rng.normal(0, 0.1, H)}
    for i in range(shape.layers):
        k = layer_keys(i, shape.layers)
        if i > 0:
            w[k["attn_norm"]] = 1.0 + rng.normal(0, 0.1, H)
        w[k["qkv_w"]] = rng.normal(0, std * 2.5, (3 * H, H))
        w[k["o_w"]] = rng.normal(0, std * 2.5, (H, H))
        w[k["mlp_norm"]] = 1.0 + rng.normal(0, 0.1, H)
        w[k["wi_w"]] = np.concatenate([rng.normal(0, std, (I, H)), rng.normal(0, std * 2.5, (I, H))], axis=0)
        w[k["wo_w"]] = rng.normal(0, std * 2.5, (H, I))
    w["final_norm.weight"] = 1.0 + rng.normal(0, 0.1, H)
    return {k: v.astype(np.float32) for k, v in w.items()}


def _norm(x, w, name, eps):
    g = w[name].astype(np.float64)
    b = w[name[:-len("weight")] + "bias"].astype(np.float64) if name[:-len("weight")] + "bias" in w else np.zeros_like(g)
    return obert._ln(x, g, b, eps)


def _bias(w, name):
    return w[name].astype(np.float64) if name in w else 0.0


def _rotate_f32(x, cos, sin):
    """apply_rotary_pos_emb as transformers evaluates it: x.float() * cos + rotate_half(x.float()) * sin — the query or
    key rounded to f32, the products (with the model's-dtype copy of the f32 table) and their sum in f64."""
    return _rotate(x.astype(np.float32).astype(np.float64), cos, sin)


def _softmax_f32(s):
    import torch

    return torch.nn.functional.softmax(torch.from_numpy(s), dim=-1, dtype=torch.float32).double().numpy()


def encode_one(w: dict, shape: ModernShape, ids, tables=None, operand=None, library_f32: bool = False, bias=None,
               bias_layer: int | None = None, round_p: bool = False, hooks=None) -> np.ndarray:
    """last_hidden_state [S, H] of one unpadded sequence, f64. tables: ((cos, sin) global, (cos, sin) windowed), each
    [>= S, d_h/2], in place of the exact ones. operand: as rope_oracle.encode_one. library_f32: the rotation and the
    softmax rounded to f32 as transformers' eager path rounds them (see the module's docstring). bias: an additive
    [heads, S, S] array on the logits of layer bias_layer (None: of every layer), beside the window's mask (a deliberate
    mistake of tests/attention_case.py). round_p: with operand, the probabilities are rounded as well, as
    oracle.bert.attend rounds them. hooks: deliberate mistakes of tests/encoder_family_rows_case.py, a dict of "rotate"
    f(x [heads, S, d_h], "q" | "k", layer) in place of the rotation, "glu" f(gate, up, layer) in place of
    gelu(gate) * up, "stale_residual" (the FFN's residual taken from before the attention block) and "skip_final";
    without it nothing changes."""
    hk = hooks or {}
    glu = hk["glu"] if "glu" in hk else (lambda gate, up, layer: obert._gelu(gate) * up)  # noqa: E731
    r = operand or (lambda v: v)  # noqa: E731
    W = lambda k: r(w[k].astype(np.float64))  # noqa: E731
    ids = np.asarray(ids, dtype=np.int64)
    S, H, nh, I = len(ids), shape.hidden, shape.heads, shape.intermediate
    dh = H // nh
    if tables is None:
        tables = (rope_table(S, dh, shape.theta), rope_table(S, dh, shape.theta_local))
    tables = [(np.asarray(c, np.float64)[:S], np.asarray(s, np.float64)[:S]) for c, s in tables]
    pos = np.arange(S)
    outside = np.abs(pos[:, None] - pos[None, :]) > shape.window
    h = _norm(w["embeddings.tok_embeddings.weight"].astype(np.float64)[ids], w, "embeddings.norm.weight", shape.eps)
    for i in range(shape.layers):
        k = layer_keys(i, shape.layers)
        glob = is_global(shape, i)
        cos, sin = tables[0 if glob else 1]
        xa = r(_norm(h, w, k["attn_norm"], shape.eps) if i > 0 else h)
        qkv = xa @ W(k["qkv_w"]).T + _bias(w, k["qkv_w"][:-6] + "bias")
        q, kk, v = (qkv[:, j * H:(j + 1) * H].reshape(S, nh, dh).transpose(1, 0, 2) for j in range(3))
        rot = _rotate_f32 if library_f32 else _rotate
        if "rotate" in hk:
            q, kk, v = r(hk["rotate"](q, "q", i)), r(hk["rotate"](kk, "k", i)), r(v)
        else:
            q, kk, v = r(rot(q, cos, sin)), r(rot(kk, cos, sin)), r(v)
        s = q @ kk.transpose(0, 2, 1) * dh ** -0.5
        if not glob:
            s = np.where(outside[None], -np.inf, s)
        b = bias if bias is not None and bias_layer in (None, i) else None
        if library_f32:
            ctx = _softmax_f32(s) @ v
        elif b is not None or (round_p and operand is not None):
            ctx = obert.attend(s, v, b, operand if round_p else None)
        else:
            s = s - s.max(axis=-1, keepdims=True)
            p = np.exp(s)
            p = p / p.sum(axis=-1, keepdims=True)
            ctx = p @ v
        ctx = r(ctx.transpose(1, 0, 2).reshape(S, H))
        before = h
        h = h + ctx @ W(k["o_w"]).T + _bias(w, k["o_w"][:-6] + "bias")
        xm = r(_norm(h, w, k["mlp_norm"], shape.eps))
        ab = xm @ W(k["wi_w"]).T + _bias(w, k["wi_w"][:-6] + "bias")
        act = r(glu(ab[:, :I], ab[:, I:], i))
        h = (before if hk.get("stale_residual") else h) + act @ W(k["wo_w"]).T + _bias(w, k["wo_w"][:-6] + "bias")
    return h if hk.get("skip_final") else _norm(h, w, "final_norm.weight", shape.eps)


def pool(h, pooling: str, normalize: bool = True):
    e = h[0] if pooling == "cls" else h.sum(axis=0) / max(float(len(h)), 1e-9)
    return e / max(float(np.sqrt((e * e).sum())), 1e-12) if normalize else e


def sentence_embeddings(w: dict, shape: ModernShape, seqs, pooling: str = "mean", normalize: bool = True,
                        tables=None, library_f32: bool = False) -> np.ndarray:
    return np.stack([pool(encode_one(w, shape, ids, tables, library_f32=library_f32), pooling, normalize) for ids in seqs])


def desc_for(shape: ModernShape, pooling: str, precision: str, max_pos: int | None = None, **over):
    """The engine's description of `shape` (over: fields to replace, e.g. window=0)."""
    from voitta_rag_amd import encoder as enc

    windowed = shape.window > 0
    fields = dict(vocab=shape.vocab, max_pos=max_pos or shape.max_pos, type_vocab=1, pooling=pooling, normalize=True,
                  eps=shape.eps, precision=precision, position="rotary", rope_theta=shape.theta, ffn="geglu", norm="pre",
                  window=shape.window, global_every=shape.global_every if windowed else 0,
                  rope_theta_local=shape.theta_local if windowed else 0.0)
    fields.update(over)
    return enc.BertDesc(shape.layers, shape.hidden, shape.heads, shape.intermediate, **fields)
