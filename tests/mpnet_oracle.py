"""TEST INFRASTRUCTURE — NumPy f64 restatement of transformers' MPNetModel (model_type mpnet) [EXT, transformers'
published behaviour] on oracle.bert's pieces: a post-LayerNorm BERT with exact-erf GELU and no token types whose
attention logits carry one additive relative-position bias shared by all layers.
  embeddings : h = LayerNorm(word[id] + pos[2 + t]) — positions start at row padding_idx + 1 = 2 (ids never hold the
               padding id 1 here: transformers gives such a token position 1 and does not count it)
  per layer  : s[h, i, j] = q_i . k_j / sqrt(d_h) + table[h, clamp(j - i, -R, R) + R];  p = softmax_j(s)
               h = LN(W_o (p v) + h);  h = LN(W_f gelu(W_i h) + h)
  result     : h, pooled (mean or first row) and L2-normalised
The bias is a general [heads, 2R + 1] table by clamped offset, the form the engine takes
(vr_encoder_set_attention_bias). MPNet's own table is table_from_buckets(): B[bucket(j - i), h] with T5-style buckets,
32 of them: split by the sign of i - j, exact below 8, logarithmic up to 128, saturated beyond — so R = 128 reproduces
the model at any length. bucket() restates transformers' relative_position_bucket separately, in NumPy; its logarithm is
taken in f32 as the library's is (tests/test_mpnet_cpu.py pins both to the library's recorded bias for every offset).
Weights are seeded and never stored: oracle.bert's scales, and the relative-bias table N(0, 1) so that the bias matters."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from oracle import bert as obert

POS_START = 2  # MPNetEmbeddings.padding_idx + 1
BUCKETS = 32
MAX_DISTANCE = 128


@dataclass
class MpnetShape:
    layers: int
    hidden: int
    heads: int
    intermediate: int
    vocab: int = 300
    positions: int = 514  # max_position_embeddings: rows of the table; sequences hold positions - 2 tokens
    eps: float = 1e-5

    @property
    def max_pos(self) -> int:
        return self.positions - POS_START


def layer_keys(i: int) -> dict[str, str]:
    p = f"encoder.layer.{i}."
    k = {}
    for short, name in (("q", "attention.attn.q"), ("k", "attention.attn.k"), ("v", "attention.attn.v"),
                        ("o", "attention.attn.o"), ("i", "intermediate.dense"), ("f", "output.dense")):
        k[short + "_w"], k[short + "_b"] = p + name + ".weight", p + name + ".bias"
    for short, name in (("ln1", "attention.LayerNorm"), ("ln2", "output.LayerNorm")):
        k[short + "_g"], k[short + "_b"] = p + name + ".weight", p + name + ".bias"
    return k


EMB_KEYS = {"word": "embeddings.word_embeddings.weight", "pos": "embeddings.position_embeddings.weight",
            "ln_g": "embeddings.LayerNorm.weight", "ln_b": "embeddings.LayerNorm.bias"}
BIAS_KEY = "encoder.relative_attention_bias.weight"


def random_weights(shape: MpnetShape, seed: int, std: float = 0.02, bias_std: float = 1.0) -> dict[str, np.ndarray]:
    """Seeded weights under transformers' MPNetModel names (no prefix), at oracle.bert.random_weights' scales; the
    relative-bias table [32, heads] is N(0, bias_std)."""
    rng = np.random.default_rng(seed)
    H, I = shape.hidden, shape.intermediate
    w = {EMB_KEYS["word"]: rng.normal(0, std, (shape.vocab, H)), EMB_KEYS["pos"]: rng.normal(0, std, (shape.positions, H)),
         EMB_KEYS["ln_g"]: 1.0 + rng.normal(0, 0.1, H), EMB_KEYS["ln_b"]: rng.normal(0, 0.1, H)}
    for i in range(shape.layers):
        k = layer_keys(i)
        for n, shp in (("q", (H, H)), ("k", (H, H)), ("v", (H, H)), ("o", (H, H)), ("i", (I, H)), ("f", (H, I))):
            w[k[n + "_w"]] = rng.normal(0, std * 2.5, shp)
            w[k[n + "_b"]] = rng.normal(0, 0.05, shp[0])
        for n in ("ln1", "ln2"):
            w[k[n + "_g"]] = 1.0 + rng.normal(0, 0.1, H)
            w[k[n + "_b"]] = rng.normal(0, 0.1, H)
    w[BIAS_KEY] = rng.normal(0, bias_std, (BUCKETS, shape.heads))
    return {k: v.astype(np.float32) for k, v in w.items()}


def bucket(relative_position, num_buckets: int = BUCKETS, max_distance: int = MAX_DISTANCE) -> np.ndarray:
    """transformers' MPNetEncoder.relative_position_bucket for relative_position = key - query (any int array)."""
    n = -np.asarray(relative_position, np.int64)
    half = num_buckets // 2
    ret = (n < 0).astype(np.int64) * half
    n = np.abs(n)
    max_exact = half // 2
    with np.errstate(divide="ignore"):
        # the library: log(n.float() / max_exact) / math.log(max_distance / max_exact) * (half - max_exact), all f32
        f = np.log(n.astype(np.float32) / np.float32(max_exact)) / np.float32(math.log(max_distance / max_exact))
        f = f * np.float32(half - max_exact)
    large = max_exact + np.where(n > 0, f, 0).astype(np.int64)  # (n = 0 is small: its -inf is never used)
    return ret + np.where(n < max_exact, n, np.minimum(large, half - 1))


def table_from_buckets(weight, radius: int = MAX_DISTANCE) -> np.ndarray:
    """relative_attention_bias.weight [32, heads] -> the offset table [heads, 2 radius + 1], f64."""
    d = np.arange(-radius, radius + 1)
    return np.asarray(weight, np.float64)[bucket(d)].T.copy()


def offset_bias(table, S: int, mirrored: bool = False, clamp: int | None = None) -> np.ndarray:
    """[heads, S, S]: entry [h, i, j] = table[h, clamp(j - i) + R]. mirrored / clamp: the two mistakes a kernel can make
    (i - j for j - i; the clamp one short), for the proof that the goldens see them."""
    table = np.asarray(table, np.float64)
    R = (table.shape[1] - 1) // 2
    c = R if clamp is None else clamp
    pos = np.arange(S)
    d = pos[None, :] - pos[:, None]  # key - query
    if mirrored:
        d = -d
    return table[:, np.clip(d, -c, c) + R]


def encode_one(w: dict, shape: MpnetShape, ids, table="buckets", bias=None, operand=None) -> np.ndarray:
    """last_hidden_state [S, H] of one unpadded sequence, f64. table: [heads, 2R + 1] offset table, "buckets" for the
    model's own (table_from_buckets of its relative_attention_bias), None for no bias. bias: a ready [heads, S, S]
    array instead (offset_bias with a mistake built in). operand: as oracle.bert.encode_one's."""
    r = operand or (lambda a: a)  # noqa: E731
    product = lambda k: w[k].ndim == 2 and k.startswith("encoder.layer.")  # noqa: E731  (a projection matrix)
    W = lambda k: r(w[k].astype(np.float64)) if product(k) else w[k].astype(np.float64)  # noqa: E731
    ids = np.asarray(ids, dtype=np.int64)
    S, H, nh = len(ids), shape.hidden, shape.heads
    dh = H // nh
    if bias is None and table is not None:
        bias = offset_bias(table_from_buckets(w[BIAS_KEY]) if isinstance(table, str) else table, S)
    x = W(EMB_KEYS["word"])[ids] + W(EMB_KEYS["pos"])[POS_START:POS_START + S]
    x = obert._ln(x, W(EMB_KEYS["ln_g"]), W(EMB_KEYS["ln_b"]), shape.eps)
    for i in range(shape.layers):
        k = layer_keys(i)
        xa = r(x)
        q, kk, v = (r((xa @ W(k[n + "_w"]).T + W(k[n + "_b"])).reshape(S, nh, dh).transpose(1, 0, 2)) for n in "qkv")
        s = q @ kk.transpose(0, 2, 1) / math.sqrt(dh)
        ctx = r(obert.attend(s, v, bias, operand).transpose(1, 0, 2).reshape(S, H))
        x = obert._ln(ctx @ W(k["o_w"]).T + W(k["o_b"]) + x, W(k["ln1_g"]), W(k["ln1_b"]), shape.eps)
        h = r(obert._gelu(r(x) @ W(k["i_w"]).T + W(k["i_b"])))
        x = obert._ln(h @ W(k["f_w"]).T + W(k["f_b"]) + x, W(k["ln2_g"]), W(k["ln2_b"]), shape.eps)
    return x


def pool(h, pooling: str, normalize: bool = True):
    e = h[0] if pooling == "cls" else h.sum(axis=0) / max(float(len(h)), 1e-9)
    return e / max(float(np.sqrt((e * e).sum())), 1e-12) if normalize else e


def sentence_embeddings(w: dict, shape: MpnetShape, seqs, pooling: str = "mean", table="buckets", **mistake) -> np.ndarray:
    """mistake: offset_bias's mirrored= / clamp= applied to the table (the proof that a fixture sees them)."""
    out = []
    for ids in seqs:
        bias = None
        if mistake:
            t = table_from_buckets(w[BIAS_KEY]) if isinstance(table, str) else table
            bias = offset_bias(t, len(ids), **mistake)
        out.append(pool(encode_one(w, shape, ids, table, bias), pooling))
    return np.stack(out)


def desc_for(shape: MpnetShape, pooling: str, precision: str, max_pos: int | None = None, **over):
    """The engine's description of `shape`: a BERT description with one token type (the bias is not part of it)."""
    from voitta_rag_amd import encoder as enc

    fields = dict(vocab=shape.vocab, max_pos=max_pos or shape.max_pos, type_vocab=1, pooling=pooling, normalize=True,
                  eps=shape.eps, precision=precision)
    fields.update(over)
    return enc.BertDesc(shape.layers, shape.hidden, shape.heads, shape.intermediate, **fields)
