"""TEST INFRASTRUCTURE — NumPy f64 restatement of transformers' Qwen2Model (model_type qwen2) [EXT, transformers'
published behaviour]: the decoder body the Qwen2.5-0.5B embedders run, with `causal` as an argument.
  embeddings : h = embed_tokens[id]                            (no norm, no position, no token type)
  rms(x, g)  : x / sqrt(mean(x^2) + eps) * g                   (Qwen2RMSNorm: no mean subtraction, no shift)
  rope(x, p) : x cos(p f) + rotate_half(x) sin(p f), f_i = theta^(-2i/d_h) repeated for both halves of the head,
               rotate_half(x) = (-x[d_h/2:], x[:d_h/2])        (the whole head is rotated)
  per layer  : a = rms(h, g_in);  q, k, v = W a + b  (biases on q, k, v only; k and v have kv_heads heads, each shared by
               heads / kv_heads consecutive query heads: repeat_kv)
               s[h, i, j] = rope(q)_i . rope(k)_j / sqrt(d_h), -inf where causal and j > i
               h = h + W_o (softmax_j(s) v);   h = h + W_down(silu(W_gate m) * W_up m), m = rms(h, g_post)
  result     : rms(h, g_norm) per token; pooled (last token, mean or first row) and L2-normalised
Weights are seeded and never stored: non-zero q/k/v biases and non-unit norm weights, so that every tensor matters.
tests/test_qwen2_cpu.py pins this file to transformers' own Qwen2Model (tests/golden/qwen2_tiny_*.npz) at 1e-9."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class Qwen2Shape:
    layers: int
    hidden: int
    heads: int
    kv_heads: int
    intermediate: int
    vocab: int = 200
    theta: float = 1e6
    eps: float = 1e-6

    @property
    def head_dim(self) -> int:
        return self.hidden // self.heads


WORD_KEY = "embed_tokens.weight"
FINAL_KEY = "norm.weight"


def layer_keys(i: int) -> dict[str, str]:
    p = f"layers.{i}."
    return {"q": p + "self_attn.q_proj.weight", "qb": p + "self_attn.q_proj.bias", "k": p + "self_attn.k_proj.weight",
            "kb": p + "self_attn.k_proj.bias", "v": p + "self_attn.v_proj.weight", "vb": p + "self_attn.v_proj.bias",
            "o": p + "self_attn.o_proj.weight", "gate": p + "mlp.gate_proj.weight", "up": p + "mlp.up_proj.weight",
            "down": p + "mlp.down_proj.weight", "ln_a": p + "input_layernorm.weight",
            "ln_m": p + "post_attention_layernorm.weight"}


def random_weights(shape: Qwen2Shape, seed: int) -> dict[str, np.ndarray]:
    """Seeded weights under transformers' Qwen2Model names (no prefix)."""
    rng = np.random.default_rng(seed)
    H, I, kv = shape.hidden, shape.intermediate, shape.kv_heads * shape.head_dim
    w = {WORD_KEY: rng.normal(0, 1.0, (shape.vocab, H)), FINAL_KEY: 1.0 + rng.normal(0, 0.1, H)}
    for i in range(shape.layers):
        k = layer_keys(i)
        # q and k entries of order one, so logits q.k / sqrt(d_h) of order one (as t5_oracle draws them): attention that
        # is neither uniform nor one-hot
        w[k["q"]] = rng.normal(0, H ** -0.5, (H, H))
        w[k["k"]] = rng.normal(0, H ** -0.5, (kv, H))
        w[k["v"]] = rng.normal(0, H ** -0.5, (kv, H))
        w[k["qb"]] = rng.normal(0, 0.3, H)
        w[k["kb"]] = rng.normal(0, 0.3, kv)
        w[k["vb"]] = rng.normal(0, 0.3, kv)
        w[k["o"]] = rng.normal(0, H ** -0.5, (H, H))
        w[k["gate"]] = rng.normal(0, H ** -0.5, (I, H))
        w[k["up"]] = rng.normal(0, H ** -0.5, (I, H))
        w[k["down"]] = rng.normal(0, I ** -0.5, (H, I))
        w[k["ln_a"]] = 1.0 + rng.normal(0, 0.1, H)
        w[k["ln_m"]] = 1.0 + rng.normal(0, 0.1, H)
    return {k: v.astype(np.float32) for k, v in w.items()}


def rms(x, g, eps):
    return x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + eps) * g


def rope(x, theta):
    """x [heads, S, d_h] rotated by positions 0 .. S - 1."""
    S, dh = x.shape[1], x.shape[2]
    f = theta ** (-np.arange(0, dh, 2, dtype=np.float64) / dh)
    a = np.arange(S, dtype=np.float64)[:, None] * np.concatenate([f, f])[None, :]
    rot = np.concatenate([-x[..., dh // 2:], x[..., :dh // 2]], axis=-1)
    return x * np.cos(a) + rot * np.sin(a)


def encode_one(w: dict, shape: Qwen2Shape, ids, causal: bool = True, bias=None, operand=None, hooks=None) -> np.ndarray:
    """The final-norm hidden states [S, H] of one unpadded sequence, f64. bias: an additive [heads, S, S] array on every
    layer's logits, beside the causal mask (a deliberate mistake of tests/attention_case.py). operand (e.g.
    rope_oracle.f16_operand): applied to both operands of every matrix product, the probabilities included (as
    oracle.bert.attend rounds them). hooks: deliberate mistakes of tests/encoder_family_rows_case.py, a dict of
    "rotate" f(x [heads, S, d_h], "q" | "k", layer) in place of rope, "glu" f(gate, up, layer) in place of
    silu(gate) * up, "rms" in place of rms, "kv_of" (the KV head of every query head), "stale_residual" (the FFN's
    residual taken from before the attention block) and "skip_final"; without it nothing changes."""
    from oracle.bert import attend

    hk = hooks or {}
    norm = hk.get("rms", rms)
    rot = hk["rotate"] if "rotate" in hk else (lambda x, kind, layer: rope(x, shape.theta))  # noqa: E731
    glu = hk["glu"] if "glu" in hk else (lambda gate, up, layer: gate / (1.0 + np.exp(-gate)) * up)  # noqa: E731
    r = operand or (lambda a: a)  # noqa: E731
    W = lambda k: r(w[k].astype(np.float64)) if k.endswith("_proj.weight") else w[k].astype(np.float64)  # noqa: E731
    ids = np.asarray(ids, dtype=np.int64)
    S, H, nh, nkv = len(ids), shape.hidden, shape.heads, shape.kv_heads
    dh, g = H // nh, nh // nkv
    masked = np.triu(np.ones((S, S), bool), 1) if causal else np.zeros((S, S), bool)
    h = W(WORD_KEY)[ids]
    for i in range(shape.layers):
        k = layer_keys(i)
        a = r(norm(h, W(k["ln_a"]), shape.eps))
        q = (a @ W(k["q"]).T + W(k["qb"])).reshape(S, nh, dh).transpose(1, 0, 2)
        kk = (a @ W(k["k"]).T + W(k["kb"])).reshape(S, nkv, dh).transpose(1, 0, 2)
        v = r((a @ W(k["v"]).T + W(k["vb"])).reshape(S, nkv, dh).transpose(1, 0, 2))
        if "kv_of" in hk:
            kk, v = kk[hk["kv_of"]], v[hk["kv_of"]]
        else:
            kk, v = np.repeat(kk, g, axis=0), np.repeat(v, g, axis=0)  # repeat_kv: query head j reads KV head j // g
        s = r(rot(q, "q", i)) @ r(rot(kk, "k", i)).transpose(0, 2, 1) / np.sqrt(dh)
        s = np.where(masked, -np.inf, s)
        before = h
        h = h + r(attend(s, v, bias, operand).transpose(1, 0, 2).reshape(S, H)) @ W(k["o"]).T
        m = r(norm(h, W(k["ln_m"]), shape.eps))
        gate = m @ W(k["gate"]).T
        h = (before if hk.get("stale_residual") else h) + r(glu(gate, m @ W(k["up"]).T, i)) @ W(k["down"]).T
    return h if hk.get("skip_final") else norm(h, W(FINAL_KEY), shape.eps)


def pool(hidden, pooling: str, normalize: bool = True):
    """[S, H] -> [H]: the last token's row, the mean, or the first row; then x / max(|x|, 1e-12)."""
    x = {"last": lambda: hidden[-1], "mean": lambda: hidden.mean(axis=0), "cls": lambda: hidden[0]}[pooling]()
    return x / max(np.sqrt((x * x).sum()), 1e-12) if normalize else x


def sentence_embeddings(w: dict, shape: Qwen2Shape, seqs, pooling: str = "last", causal: bool = True, normalize: bool = True):
    return np.stack([pool(encode_one(w, shape, ids, causal), pooling, normalize) for ids in seqs])


def desc_for(shape: Qwen2Shape, pooling: str, precision: str, max_pos: int = 512, causal: int = 1, **over):
    """The engine's description of `shape`."""
    from voitta_rag_amd import encoder as enc

    fields = dict(vocab=shape.vocab, max_pos=max_pos, type_vocab=1, pooling=pooling, normalize=True, eps=shape.eps,
                  precision=precision, position="rotary", rope_theta=shape.theta, ffn="swiglu", norm="rms_pre_rotary",
                  causal=causal)
    fields.update(over)
    return enc.BertDesc(shape.layers, shape.hidden, shape.heads, shape.intermediate, **fields)


# ---- a synthetic Qwen2 sentence-transformers directory -------------------------------------------------------------------
ST = "sentence_transformers.models."


def config_json(shape: Qwen2Shape, **over) -> dict:
    cfg = {"model_type": "qwen2", "architectures": ["Qwen2Model"], "hidden_size": shape.hidden,
           "num_attention_heads": shape.heads, "num_key_value_heads": shape.kv_heads, "intermediate_size": shape.intermediate,
           "num_hidden_layers": shape.layers, "vocab_size": shape.vocab, "rms_norm_eps": shape.eps, "rope_theta": shape.theta,
           "hidden_act": "silu", "max_position_embeddings": 32768, "use_sliding_window": False, "rope_scaling": None,
           "tie_word_embeddings": True}
    cfg.update(over)
    return cfg


def write_checkpoint(d: str, shape: Qwen2Shape, seed: int, pooling: str = "last", max_seq: int | None = 128,
                     body: bool = True, tokenizer: bool = True, prefix: str = "", config=None, modules: bool = True) -> dict:
    """config.json, modules.json (Transformer, Pooling, Normalize), 1_Pooling, sentence_bert_config.json (max_seq, or
    none), tokenizer.json (tests/golden/bpe_tokenizer.json's) and model.safetensors of a seeded Qwen2 body; returns its
    weights (qwen2_oracle names). modules=False: a bare config.json. body=False: no weights (the readers need none)."""
    import json
    import os

    from safetensors.numpy import save_file

    os.makedirs(d, exist_ok=True)
    json.dump(config_json(shape, **(config or {})), open(os.path.join(d, "config.json"), "w"))
    if modules:
        os.makedirs(os.path.join(d, "1_Pooling"), exist_ok=True)
        json.dump([{"idx": 0, "name": "0", "path": "", "type": ST + "Transformer"},
                   {"idx": 1, "name": "1", "path": "1_Pooling", "type": ST + "Pooling"},
                   {"idx": 2, "name": "2", "path": "2_Normalize", "type": ST + "Normalize"}],
                  open(os.path.join(d, "modules.json"), "w"))
        json.dump({"word_embedding_dimension": shape.hidden, "pooling_mode_cls_token": pooling == "cls",
                   "pooling_mode_mean_tokens": pooling == "mean", "pooling_mode_lasttoken": pooling == "last"},
                  open(os.path.join(d, "1_Pooling", "config.json"), "w"))
    if max_seq is not None:
        json.dump({"max_seq_length": max_seq, "do_lower_case": False}, open(os.path.join(d, "sentence_bert_config.json"), "w"))
    if tokenizer:
        here = os.path.dirname(os.path.abspath(__file__))
        spec = json.load(open(os.path.join(here, "golden", "bpe_tokenizer.json"), encoding="utf-8"))["tokenizer"]
        json.dump(spec, open(os.path.join(d, "tokenizer.json"), "w", encoding="utf-8"))
    w = random_weights(shape, seed)
    if body:
        save_file({prefix + k: np.ascontiguousarray(v) for k, v in w.items()}, os.path.join(d, "model.safetensors"))
    return w
