"""TEST INFRASTRUCTURE — NumPy f64 restatement of transformers' T5EncoderModel (model_type t5, feed_forward_proj relu)
[EXT, transformers' published behaviour] on oracle.bert / mpnet_oracle pieces: pre-norm blocks with RMSNorm and a ReLU
FFN without biases, no position in the embeddings, and block 0's bucketed relative-position bias in every layer.
  embeddings : h = shared[id]                                  (no norm, no position, no token type)
  rms(x, g)  : x / sqrt(mean(x^2) + eps) * g                   (T5LayerNorm: no mean subtraction, no shift)
  per layer  : a = rms(h, g_a);  s[h, i, j] = q_i . k_j + table[h, clamp(j - i, -R, R) + R]   — NO 1/sqrt(d_kv)
               h = h + W_o (softmax_j(s) v);   h = h + W_wo relu(W_wi rms(h, g_m))
  result     : rms(h, g_final), pooled (mean or first row) and L2-normalised
The bias table is mpnet_oracle.table_from_buckets' form: T5's bidirectional _relative_position_bucket is the function
MPNet copied (mpnet_oracle.bucket restates it in NumPy with the library's f32 logarithm), with num_buckets and
max_distance from the config; the buckets are constant from |j - i| = max_distance on, so R = max_distance reproduces
compute_bias at any length (tests/test_t5_cpu.py pins the table to the library's recorded bias for offsets -600..600).
Weights are seeded and never stored. q is drawn at T5's own initialiser scale, (d_model * d_kv)^-0.5, so that the
UNSCALED logits are of order one; k at d_model^-0.5 as the library's; the rest at oracle.bert's scales; the bias table
N(0, 1) so that it matters."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import mpnet_oracle as mp

BUCKETS = 32
MAX_DISTANCE = 128


@dataclass
class T5Shape:
    layers: int
    hidden: int      # d_model
    heads: int       # num_heads; d_kv = hidden / heads
    intermediate: int  # d_ff
    vocab: int = 300
    eps: float = 1e-6
    buckets: int = BUCKETS
    max_distance: int = MAX_DISTANCE

    @property
    def d_kv(self) -> int:
        return self.hidden // self.heads


def layer_keys(i: int) -> dict[str, str]:
    p = f"encoder.block.{i}.layer."
    return {"q": p + "0.SelfAttention.q.weight", "k": p + "0.SelfAttention.k.weight", "v": p + "0.SelfAttention.v.weight",
            "o": p + "0.SelfAttention.o.weight", "ln_a": p + "0.layer_norm.weight",
            "wi": p + "1.DenseReluDense.wi.weight", "wo": p + "1.DenseReluDense.wo.weight", "ln_m": p + "1.layer_norm.weight"}


WORD_KEY = "shared.weight"
FINAL_KEY = "encoder.final_layer_norm.weight"
BIAS_KEY = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"


def random_weights(shape: T5Shape, seed: int, bias_std: float = 1.0) -> dict[str, np.ndarray]:
    """Seeded weights under transformers' T5EncoderModel names (no prefix; encoder.embed_tokens.weight is tied to
    shared.weight and not listed)."""
    rng = np.random.default_rng(seed)
    H, I, dkv = shape.hidden, shape.intermediate, shape.d_kv
    w = {WORD_KEY: rng.normal(0, 1.0, (shape.vocab, H)), FINAL_KEY: 1.0 + rng.normal(0, 0.1, H)}
    for i in range(shape.layers):
        k = layer_keys(i)
        w[k["q"]] = rng.normal(0, (H * dkv) ** -0.5, (H, H))  # T5's initialiser: unscaled logits of order one
        w[k["k"]] = rng.normal(0, H ** -0.5, (H, H))
        w[k["v"]] = rng.normal(0, H ** -0.5, (H, H))
        w[k["o"]] = rng.normal(0, H ** -0.5, (H, H))
        w[k["wi"]] = rng.normal(0, H ** -0.5, (I, H))
        w[k["wo"]] = rng.normal(0, I ** -0.5, (H, I))
        w[k["ln_a"]] = 1.0 + rng.normal(0, 0.1, H)
        w[k["ln_m"]] = 1.0 + rng.normal(0, 0.1, H)
    w[BIAS_KEY] = rng.normal(0, bias_std, (shape.buckets, shape.heads))
    return {k: v.astype(np.float32) for k, v in w.items()}


def table_from_buckets(weight, shape: T5Shape, radius: int | None = None) -> np.ndarray:
    """relative_attention_bias.weight [buckets, heads] -> the offset table [heads, 2 radius + 1], f64 (radius:
    max_distance)."""
    r = shape.max_distance if radius is None else radius
    d = np.arange(-r, r + 1)
    return np.asarray(weight, np.float64)[mp.bucket(d, shape.buckets, shape.max_distance)].T.copy()


def rms(x, g, eps):
    return x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + eps) * g


def encode_one(w: dict, shape: T5Shape, ids, table="buckets", operand=None, hooks=None) -> np.ndarray:
    """The final-norm hidden states [S, H] of one unpadded sequence, f64. table: an [heads, 2R + 1] offset table,
    "buckets" for the model's own, None for no bias. operand (e.g. rope_oracle.f16_operand): applied to both operands of
    every matrix product, the probabilities included (as oracle.bert.attend rounds them). hooks: deliberate mistakes of
    tests/encoder_family_rows_case.py, a dict of "act" f(x, layer) in place of relu, "rms" in place of rms,
    "stale_residual" (the FFN's residual taken from before the attention block) and "skip_final"; without it nothing
    changes."""
    hk = hooks or {}
    norm = hk.get("rms", rms)
    act = hk["act"] if "act" in hk else (lambda x, layer: np.maximum(x, 0.0))  # noqa: E731
    r = operand or (lambda a: a)  # noqa: E731
    product = lambda k: w[k].ndim == 2 and k != BIAS_KEY and k != WORD_KEY  # noqa: E731  (a projection matrix)
    W = lambda k: r(w[k].astype(np.float64)) if product(k) else w[k].astype(np.float64)  # noqa: E731
    ids = np.asarray(ids, dtype=np.int64)
    S, H, nh = len(ids), shape.hidden, shape.heads
    dh = H // nh
    bias = None
    if table is not None:
        bias = mp.offset_bias(table_from_buckets(w[BIAS_KEY], shape) if isinstance(table, str) else table, S)
    h = W(WORD_KEY)[ids]
    for i in range(shape.layers):
        k = layer_keys(i)
        a = r(norm(h, W(k["ln_a"]), shape.eps))
        q, kk, v = (r((a @ W(k[n]).T).reshape(S, nh, dh).transpose(1, 0, 2)) for n in "qkv")
        s = q @ kk.transpose(0, 2, 1)  # no 1/sqrt(d_kv)
        if bias is not None:
            s = s + bias
        s = s - s.max(axis=-1, keepdims=True)
        p = np.exp(s)
        p = p / p.sum(axis=-1, keepdims=True)
        before = h
        h = h + r((r(p) @ v).transpose(1, 0, 2).reshape(S, H)) @ W(k["o"]).T
        m = r(norm(h, W(k["ln_m"]), shape.eps))
        h = (before if hk.get("stale_residual") else h) + r(act(m @ W(k["wi"]).T, i)) @ W(k["wo"]).T
    return h if hk.get("skip_final") else norm(h, W(FINAL_KEY), shape.eps)


def sentence_embeddings(w: dict, shape: T5Shape, seqs, pooling: str = "mean", table="buckets", normalize: bool = True):
    return np.stack([mp.pool(encode_one(w, shape, ids, table), pooling, normalize) for ids in seqs])


def span_embeddings(w: dict, shape: T5Shape, seqs, spans, table="buckets") -> np.ndarray:
    """One row per (sequence index, begin, end): the normalised mean of that token range's final hidden states."""
    hidden = [encode_one(w, shape, ids, table) for ids in seqs]
    return np.stack([mp.pool(hidden[s][b:e], "mean") for s, b, e in spans])


def desc_for(shape: T5Shape, pooling: str, precision: str, max_pos: int = 512, **over):
    """The engine's description of `shape` (the bias table is not part of it)."""
    from voitta_rag_amd import encoder as enc

    fields = dict(vocab=shape.vocab, max_pos=max_pos, type_vocab=1, pooling=pooling, normalize=True, eps=shape.eps,
                  precision=precision, position="none", ffn="relu", norm="rms_pre")
    fields.update(over)
    return enc.BertDesc(shape.layers, shape.hidden, shape.heads, shape.intermediate, **fields)


# ---- a synthetic gtr-t5-style sentence-transformers directory ------------------------------------------------------------
ST = "sentence_transformers.models."


def tokenizer_fixture() -> dict:
    """tests/golden/t5_tokenizer.json: {"tokenizer": the tokenizer.json, "cases": [{text, max_len, ids}]}."""
    import json
    import os

    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "t5_tokenizer.json"),
                          encoding="utf-8"))


def config_json(shape: T5Shape, **over) -> dict:
    cfg = {"model_type": "t5", "architectures": ["T5EncoderModel"], "d_model": shape.hidden, "num_heads": shape.heads,
           "d_kv": shape.d_kv, "d_ff": shape.intermediate, "num_layers": shape.layers, "vocab_size": shape.vocab,
           "layer_norm_epsilon": shape.eps, "feed_forward_proj": "relu", "n_positions": 512,
           "relative_attention_num_buckets": shape.buckets, "relative_attention_max_distance": shape.max_distance,
           "is_encoder_decoder": False}
    cfg.update(over)
    return cfg


def dense_weight(shape: T5Shape, seed: int, out: int | None = None) -> np.ndarray:
    """The Dense module's weight [out, hidden] (no bias, identity), seeded."""
    return np.random.default_rng(seed + 500).normal(0, shape.hidden ** -0.5, (out or shape.hidden, shape.hidden)).astype(np.float32)


def write_checkpoint(d: str, shape: T5Shape, seed: int, pooling: str = "mean", max_seq: int = 128, body: bool = True,
                     tokenizer: bool = True, prefix: str = "", config=None) -> dict:
    """config.json, modules.json (Transformer, Pooling, Dense bias false Identity, Normalize), 1_Pooling, 2_Dense,
    sentence_bert_config.json, tokenizer.json (the fixture's) and model.safetensors of a seeded T5 encoder; returns its
    weights (t5_oracle names). body=False: no encoder weights (the readers need none)."""
    import json
    import os

    from safetensors.numpy import save_file

    os.makedirs(os.path.join(d, "1_Pooling"), exist_ok=True)
    os.makedirs(os.path.join(d, "2_Dense"), exist_ok=True)
    json.dump(config_json(shape, **(config or {})), open(os.path.join(d, "config.json"), "w"))
    json.dump([{"idx": 0, "name": "0", "path": "", "type": ST + "Transformer"},
               {"idx": 1, "name": "1", "path": "1_Pooling", "type": ST + "Pooling"},
               {"idx": 2, "name": "2", "path": "2_Dense", "type": ST + "Dense"},
               {"idx": 3, "name": "3", "path": "3_Normalize", "type": ST + "Normalize"}],
              open(os.path.join(d, "modules.json"), "w"))
    json.dump({"word_embedding_dimension": shape.hidden, "pooling_mode_cls_token": pooling == "cls",
               "pooling_mode_mean_tokens": pooling != "cls"}, open(os.path.join(d, "1_Pooling", "config.json"), "w"))
    json.dump({"in_features": shape.hidden, "out_features": shape.hidden, "bias": False,
               "activation_function": "torch.nn.modules.linear.Identity"}, open(os.path.join(d, "2_Dense", "config.json"), "w"))
    save_file({"linear.weight": dense_weight(shape, seed)}, os.path.join(d, "2_Dense", "model.safetensors"))
    json.dump({"max_seq_length": max_seq, "do_lower_case": False}, open(os.path.join(d, "sentence_bert_config.json"), "w"))
    if tokenizer:
        json.dump(tokenizer_fixture()["tokenizer"], open(os.path.join(d, "tokenizer.json"), "w", encoding="utf-8"))
    w = random_weights(shape, seed)
    if body:
        state = {prefix + k: np.ascontiguousarray(v) for k, v in w.items()}
        state[prefix + "encoder.embed_tokens.weight"] = state[prefix + WORD_KEY].copy()  # (the tied copy a T5EncoderModel saves)
        save_file(state, os.path.join(d, "model.safetensors"))
    return w


def head_embeddings(w: dict, shape: T5Shape, seqs, seed: int, pooling: str = "mean") -> np.ndarray:
    """The pipeline of write_checkpoint's directory: pooled (un-normalised) rows through the Dense, then normalised."""
    x = sentence_embeddings(w, shape, seqs, pooling, normalize=False) @ dense_weight(shape, seed).astype(np.float64).T
    return x / np.maximum(np.sqrt((x * x).sum(axis=-1, keepdims=True)), 1e-12)
