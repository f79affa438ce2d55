"""TEST INFRASTRUCTURE — NumPy f64 restatement of transformers' Qwen3Model (model_type qwen3) [EXT, transformers'
published behaviour]: tests/qwen2_oracle.py's body with a head size of its own and a per-head RMSNorm on Q and K.
  head_dim   : q_proj is [heads * head_dim, hidden], k_proj / v_proj [kv_heads * head_dim, hidden], o_proj
               [hidden, heads * head_dim]; the attention width A = heads * head_dim need not be hidden
  per layer  : a = rms(h, g_in);  q, k, v = W a (+ b where the shape has attention biases)
               q = rms_head(q, g_q), k = rms_head(k, g_k)      (over the head's head_dim values, the gains [head_dim]
                                                                shared by the heads; only where shape.qk_norm)
               s[h, i, j] = rope(q)_i . rope(k)_j / sqrt(head_dim), -inf where causal and j > i
               h = h + W_o (softmax_j(s) v);   h = h + W_down(silu(W_gate m) * W_up m), m = rms(h, g_post)
  result     : rms(h, g_norm) per token; pooled (last token, mean or first row) and L2-normalised
Weights are seeded and never stored. The Q/K gains are NOT one: they are drawn around GAIN (with a spread of a tenth), a
value chosen so that the logits stay of order one — behind the norm |q| = sqrt(head_dim) g whatever the weights, so the
logit of a query against a key is about g_q g_k sqrt(head_dim) cos(q, k), and a softmax that sits on one key would hide
a wrong key from every test. tests/test_qwen3_cpu.py asserts the condition on this file's own attention weights
(`probe`) and pins the file to transformers' Qwen3Model (tests/golden/qwen3_tiny_*.npz) at 1e-9."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from qwen2_oracle import ST, pool, rms, rope  # noqa: F401  (the same formulas; re-exported for the tests)

# the mean of the Q and K gains: logits of standard deviation about GAIN^2 sqrt(head_dim) |cos(q, k)|; with random
# projections of hidden 128 .. 256 the cosine is about head_dim^-1/2, so GAIN^2 is the logits' order
GAIN = 0.9


@dataclass
class Qwen3Shape:
    layers: int
    hidden: int
    heads: int
    kv_heads: int
    intermediate: int
    head_dim: int
    qk_norm: bool = True
    attention_bias: bool = False
    vocab: int = 200
    theta: float = 1e6
    eps: float = 1e-6

    @property
    def attn(self) -> int:
        return self.heads * self.head_dim


WORD_KEY = "embed_tokens.weight"
FINAL_KEY = "norm.weight"


def layer_keys(i: int) -> dict[str, str]:
    p = f"layers.{i}."
    return {"q": p + "self_attn.q_proj.weight", "qb": p + "self_attn.q_proj.bias", "k": p + "self_attn.k_proj.weight",
            "kb": p + "self_attn.k_proj.bias", "v": p + "self_attn.v_proj.weight", "vb": p + "self_attn.v_proj.bias",
            "o": p + "self_attn.o_proj.weight", "qn": p + "self_attn.q_norm.weight", "kn": p + "self_attn.k_norm.weight",
            "gate": p + "mlp.gate_proj.weight", "up": p + "mlp.up_proj.weight", "down": p + "mlp.down_proj.weight",
            "ln_a": p + "input_layernorm.weight", "ln_m": p + "post_attention_layernorm.weight"}


def random_weights(shape: Qwen3Shape, seed: int) -> dict[str, np.ndarray]:
    """Seeded weights under transformers' Qwen3Model names (no prefix)."""
    rng = np.random.default_rng(seed)
    H, I, A, kv, dh = shape.hidden, shape.intermediate, shape.attn, shape.kv_heads * shape.head_dim, shape.head_dim
    w = {WORD_KEY: rng.normal(0, 1.0, (shape.vocab, H)), FINAL_KEY: 1.0 + rng.normal(0, 0.1, H)}
    for i in range(shape.layers):
        k = layer_keys(i)
        w[k["q"]] = rng.normal(0, H ** -0.5, (A, H))
        w[k["k"]] = rng.normal(0, H ** -0.5, (kv, H))
        w[k["v"]] = rng.normal(0, H ** -0.5, (kv, H))
        if shape.attention_bias:
            w[k["qb"]] = rng.normal(0, 0.3, A)
            w[k["kb"]] = rng.normal(0, 0.3, kv)
            w[k["vb"]] = rng.normal(0, 0.3, kv)
        w[k["o"]] = rng.normal(0, A ** -0.5, (H, A))
        if shape.qk_norm:
            w[k["qn"]] = GAIN * (1.0 + rng.normal(0, 0.1, dh))
            w[k["kn"]] = GAIN * (1.0 + rng.normal(0, 0.1, dh))
        w[k["gate"]] = rng.normal(0, H ** -0.5, (I, H))
        w[k["up"]] = rng.normal(0, H ** -0.5, (I, H))
        w[k["down"]] = rng.normal(0, I ** -0.5, (H, I))
        w[k["ln_a"]] = 1.0 + rng.normal(0, 0.1, H)
        w[k["ln_m"]] = 1.0 + rng.normal(0, 0.1, H)
    return {k: v.astype(np.float32) for k, v in w.items()}


def encode_one(w: dict, shape: Qwen3Shape, ids, causal: bool = True, bias=None, operand=None, probe=None) -> np.ndarray:
    """The final-norm hidden states [S, H] of one unpadded sequence, f64. bias: an additive [heads, S, S] array on every
    layer's logits, beside the causal mask (a deliberate mistake of tests/attention_case.py, which passes causal=False
    and the complete array; [heads, S, S + n]: n zero keys behind the end, see oracle.bert.attend). operand (e.g.
    rope_oracle.f16_operand): applied to both operands of every matrix product, the probabilities included (as
    oracle.bert.attend rounds them). probe: a list that receives every layer's attention weights [heads, S, S]
    (unrounded, without the bias)."""
    from oracle.bert import attend

    r = operand or (lambda a: a)  # noqa: E731
    W = lambda k: r(w[k].astype(np.float64)) if k.endswith("_proj.weight") else w[k].astype(np.float64)  # noqa: E731
    ids = np.asarray(ids, dtype=np.int64)
    S, H, nh, nkv, dh = len(ids), shape.hidden, shape.heads, shape.kv_heads, shape.head_dim
    g = nh // nkv
    masked = np.triu(np.ones((S, S), bool), 1) if causal else np.zeros((S, S), bool)
    h = W(WORD_KEY)[ids]
    for i in range(shape.layers):
        k = layer_keys(i)
        a = r(rms(h, W(k["ln_a"]), shape.eps))
        q, kk, v = a @ W(k["q"]).T, a @ W(k["k"]).T, a @ W(k["v"]).T
        if shape.attention_bias:
            q, kk, v = q + W(k["qb"]), kk + W(k["kb"]), v + W(k["vb"])
        q = q.reshape(S, nh, dh).transpose(1, 0, 2)
        kk = kk.reshape(S, nkv, dh).transpose(1, 0, 2)
        v = r(v.reshape(S, nkv, dh).transpose(1, 0, 2))
        if shape.qk_norm:  # per head, over its head_dim values, ahead of the rotation
            q, kk = rms(q, W(k["qn"]), shape.eps), rms(kk, W(k["kn"]), shape.eps)
        kk, v = np.repeat(kk, g, axis=0), np.repeat(v, g, axis=0)  # repeat_kv: query head j reads KV head j // g
        s = r(rope(q, shape.theta)) @ r(rope(kk, shape.theta)).transpose(0, 2, 1) / np.sqrt(dh)
        s = np.where(masked, -np.inf, s)
        if probe is not None:
            e = np.exp(s - s.max(axis=-1, keepdims=True))
            probe.append(e / e.sum(axis=-1, keepdims=True))
        h = h + r(attend(s, v, bias, operand).transpose(1, 0, 2).reshape(S, nh * dh)) @ W(k["o"]).T
        m = r(rms(h, W(k["ln_m"]), shape.eps))
        gate = m @ W(k["gate"]).T
        h = h + r(gate / (1.0 + np.exp(-gate)) * (m @ W(k["up"]).T)) @ W(k["down"]).T
    return rms(h, W(FINAL_KEY), shape.eps)


def sentence_embeddings(w: dict, shape: Qwen3Shape, seqs, pooling: str = "last", causal: bool = True, normalize: bool = True):
    return np.stack([pool(encode_one(w, shape, ids, causal), pooling, normalize) for ids in seqs])


def peaked_share(w: dict, shape: Qwen3Shape, ids, causal: bool = True) -> float:
    """The share of (layer, head, query) triples of one sequence that put more than half their weight on one key (queries
    that see one key only — the first under a causal mask — are not counted: they have no choice)."""
    probe: list = []
    encode_one(w, shape, ids, causal, probe=probe)
    p = np.stack(probe)[:, :, 1:] if causal else np.stack(probe)
    return float((p.max(axis=-1) > 0.5).mean())


def desc_for(shape: Qwen3Shape, pooling: str, precision: str, max_pos: int = 512, causal: int = 1, **over):
    """The engine's description of `shape`."""
    from voitta_rag_amd import encoder as enc

    fields = dict(vocab=shape.vocab, max_pos=max_pos, type_vocab=1, pooling=pooling, normalize=True, eps=shape.eps,
                  precision=precision, position="rotary", rope_theta=shape.theta, ffn="swiglu", norm="rms_pre_rotary",
                  causal=causal, head_dim=shape.head_dim, qk_norm=int(shape.qk_norm))
    fields.update(over)
    return enc.BertDesc(shape.layers, shape.hidden, shape.heads, shape.intermediate, **fields)


# ---- a synthetic Qwen3 sentence-transformers directory -------------------------------------------------------------------
def config_json(shape: Qwen3Shape, **over) -> dict:
    cfg = {"model_type": "qwen3", "architectures": ["Qwen3Model"], "hidden_size": shape.hidden,
           "num_attention_heads": shape.heads, "num_key_value_heads": shape.kv_heads, "head_dim": shape.head_dim,
           "intermediate_size": shape.intermediate, "num_hidden_layers": shape.layers, "vocab_size": shape.vocab,
           "rms_norm_eps": shape.eps, "rope_theta": shape.theta, "hidden_act": "silu", "attention_bias": shape.attention_bias,
           "max_position_embeddings": 32768, "use_sliding_window": False, "rope_scaling": None, "tie_word_embeddings": True}
    cfg.update(over)
    return cfg


def write_checkpoint(d: str, shape: Qwen3Shape, seed: int, pooling: str = "last", max_seq: int | None = 128,
                     body: bool = True, tokenizer: bool = True, prefix: str = "", config=None, modules: bool = True) -> dict:
    """config.json, modules.json (Transformer, Pooling, Normalize), 1_Pooling, sentence_bert_config.json (max_seq, or
    none), tokenizer.json (tests/golden/bpe_tokenizer.json's) and model.safetensors of a seeded Qwen3 body; returns its
    weights (this file's names). modules=False: a bare config.json. body=False: no weights (the readers need none)."""
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
