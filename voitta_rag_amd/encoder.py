"""Host side of the dense encoder: hands BERT-family weights (held by PyTorch or NumPy) to
``vr_encoder_load`` in the order the C-ABI fixes, and drives ``vr_encode``.

Replaces the ``SentenceTransformer(model_name, device)`` object the reference lazily creates
(src/voitta/services/embedding.py:23-42) — model architecture facts come from the checkpoint's
``config.json`` / ``modules.json``; PyTorch is used only to read and hold the weights."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field, replace

import numpy as np

from . import _lib
from ._lib import VR_MEM_DEVICE, VR_MEM_HOST, VR_POOL_CLS, VR_POOL_LAST, VR_POOL_MEAN, check

EMB_SUFFIXES = [
    "embeddings.word_embeddings.weight",
    "embeddings.position_embeddings.weight",
    "embeddings.token_type_embeddings.weight",
    "embeddings.LayerNorm.weight",
    "embeddings.LayerNorm.bias",
]
LAYER_SUFFIXES = [
    "attention.self.query.weight", "attention.self.query.bias",
    "attention.self.key.weight", "attention.self.key.bias",
    "attention.self.value.weight", "attention.self.value.bias",
    "attention.output.dense.weight", "attention.output.dense.bias",
    "attention.output.LayerNorm.weight", "attention.output.LayerNorm.bias",
    "intermediate.dense.weight", "intermediate.dense.bias",
    "output.dense.weight", "output.dense.bias",
    "output.LayerNorm.weight", "output.LayerNorm.bias",
]

# A rotary, gated-FFN encoder (model_type nomic_bert) in the slot order of vr_encoder_load, named as the native
# transformers NomicBertModel names them. None = a slot the checkpoint has no tensor for (these models carry no
# biases in their projections and no position table): it crosses the ABI as NULL.
ROPE_EMB_SUFFIXES = [
    "embeddings.word_embeddings.weight", None, "embeddings.token_type_embeddings.weight",
    "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias",
]
ROPE_LAYER_SUFFIXES = [
    "self_attn.q_proj.weight", None, "self_attn.k_proj.weight", None, "self_attn.v_proj.weight", None,
    "self_attn.o_proj.weight", None,
    "post_attention_layernorm.weight", "post_attention_layernorm.bias",
    "mlp.up_proj.weight", None, "mlp.down_proj.weight", None,
    "post_mlp_layernorm.weight", "post_mlp_layernorm.bias",
    "mlp.gate_proj.weight", None,
]
# the hub checkpoint's names -> the native ones (transformers' conversion mapping for nomic_bert); attn.Wqkv is the
# q, k, v matrices stacked along dim 0
HUB_RENAMES = [("encoder.layers.", "layers."), ("emb_ln.", "embeddings.LayerNorm."), ("attn.out_proj.", "self_attn.o_proj."),
               ("mlp.fc11.", "mlp.up_proj."), ("mlp.fc12.", "mlp.gate_proj."), ("mlp.fc2.", "mlp.down_proj."),
               ("norm1.", "post_attention_layernorm."), ("norm2.", "post_mlp_layernorm.")]


@dataclass
class HeadStage:
    """One module behind pooling (vr_head_stage). kind "dense": y = act(weight @ x + bias), weight [out, in], bias [out]
    or None, activation "identity" | "tanh". kind "layernorm": y = (x - mean) / sqrt(var + eps) * weight + bias over
    the whole row, weight [width], bias [width] or None."""
    kind: str
    weight: object
    bias: object = None
    activation: str = "identity"
    eps: float = 1e-5

    @property
    def in_dim(self) -> int:
        return int(self.weight.shape[-1])

    @property
    def out_dim(self) -> int:
        return int(self.weight.shape[0])


@dataclass
class BertDesc:
    layers: int
    hidden: int
    heads: int
    intermediate: int
    vocab: int = 30522
    max_pos: int = 512
    type_vocab: int = 2
    pooling: str = "mean"  # "mean" | "cls" | "last" (the sequence's last token: decoder-style embedders)
    normalize: bool = True
    eps: float = 1e-12
    precision: str = "f32"  # "f32" (exact f32 MFMA) | "f16x3" (split-precision f16 MFMA, f32-class accuracy)
    # "learned" (a position table) | "rotary" (max_pos = length of the cos/sin table) | "none" (no position in the
    # embeddings or in Q and K: max_pos = the longest sequence; ALiBi models, whose position is in attention_slopes)
    position: str = "learned"
    rope_theta: float = 0.0
    # "gelu" | "swiglu" | "geglu" (down(act(gate(x)) * up(x)), act = SiLU / exact GELU) | "relu" (down(relu(up(x))): T5)
    ffn: str = "gelu"
    # "post" (x = LN(x + f(x))) | "pre" (x = x + f(LN(x)), a final LayerNorm: the ModernBERT family) | "rms_pre" (the
    # same with RMSNorm and no embedding norm in the stream: the T5 encoders; needs position "none" and ffn "relu") |
    # "rms_pre_rotary" (the Llama / Qwen2 block: RMSNorm pre-norm with rotary positions and a gated ffn)
    norm: str = "post"
    window: int = 0  # sliding-window attention: query i of a windowed layer sees key j iff |i - j| <= window; 0 = none
    global_every: int = 0  # window > 0: layer l attends globally iff l % global_every == 0
    rope_theta_local: float = 0.0  # the rotary base of the windowed layers; 0 = rope_theta
    causal: int = 0  # 1: query i sees key j iff j <= i (norm "rms_pre_rotary" only)
    # the head size when it is not hidden / heads (32, 64 or 128; 0 = hidden / heads): q/k/v are then [heads * head_dim,
    # hidden] and o_proj [hidden, heads * head_dim]; and whether every head of Q and K is RMS-normalised and scaled by
    # q_norm / k_norm [head_dim] before the rotation (two slots more per layer). Qwen3; norm "rms_pre_rotary" only
    head_dim: int = 0
    qk_norm: int = 0
    # additive attention bias by relative offset, f32 [heads, 2 * radius + 1] (MPNet: mpnet_bias_table, T5:
    # t5_bias_table); not a field of
    # vr_bert_desc: load_encoder hands it to vr_encoder_set_attention_bias once the model is loaded
    attention_bias: object = field(default=None, compare=False, repr=False)
    # linear attention bias, f32 [heads]: the logit of head h loses attention_slopes[h] * |key - query| (ALiBi:
    # alibi_slopes); like attention_bias not a field of vr_bert_desc: load_encoder hands it to
    # vr_encoder_set_attention_slopes once the model is loaded
    attention_slopes: object = field(default=None, compare=False, repr=False)
    # the post-pooling head: HeadStage objects in order (sentence-transformers' Dense / LayerNorm modules behind
    # Pooling) and the number of leading columns kept (SentenceTransformer(truncate_dim=...), 0 = all). Not fields of
    # vr_bert_desc either: load_encoder hands them to vr_encoder_set_head once the model is loaded
    head: object = field(default=None, compare=False, repr=False)
    truncate_dim: int = field(default=0, compare=False)

    @property
    def out_dim(self) -> int:
        """The width of an embedding row: truncate_dim, or the last head stage's output, or the model's."""
        if self.truncate_dim:
            return int(self.truncate_dim)
        return self.head[-1].out_dim if self.head else self.hidden

    @property
    def head_size(self) -> int:
        return int(self.head_dim) if self.head_dim else self.hidden // self.heads

    @property
    def attn_width(self) -> int:
        """The width of the query, key and value rows and of the context: heads * head size (hidden unless head_dim says otherwise)."""
        return self.heads * self.head_size

    @property
    def rotary(self) -> bool:
        return self.position == "rotary"

    @property
    def gated(self) -> bool:
        return self.ffn in ("swiglu", "geglu")

    @property
    def prenorm(self) -> bool:
        return self.norm == "pre"

    @property
    def rms(self) -> bool:
        return self.norm == "rms_pre"

    @property
    def rms_rotary(self) -> bool:
        return self.norm == "rms_pre_rotary"

    def to_c(self) -> _lib.VrBertDesc:
        # (a causal description crosses as vr_bert_desc_v2, one with a head_dim or Q/K norms as vr_bert_desc_v3, every
        # other one as the vr_bert_desc it always was)
        v3 = bool(self.head_dim or self.qk_norm)
        d = _lib.VrBertDescV3() if v3 else _lib.VrBertDescV2() if self.causal else _lib.VrBertDesc()
        d.struct_size = C.sizeof(type(d))
        d.layers, d.hidden, d.heads, d.intermediate = self.layers, self.hidden, self.heads, self.intermediate
        d.vocab, d.max_pos, d.type_vocab = self.vocab, self.max_pos, self.type_vocab
        poolings = {"mean": VR_POOL_MEAN, "cls": VR_POOL_CLS, "last": VR_POOL_LAST}
        if self.pooling not in poolings:
            raise ValueError(f"unknown pooling {self.pooling!r}")
        d.pooling = poolings[self.pooling]
        d.normalize = int(self.normalize)
        d.eps = self.eps
        codes = {"f32": _lib.VR_PRECISION_F32, "f16x3": _lib.VR_PRECISION_F16X3, "f16": _lib.VR_PRECISION_F16}
        if self.precision not in codes:
            raise ValueError(f"unknown encoder precision {self.precision!r}")
        d.precision = codes[self.precision]
        positions = {"learned": _lib.VR_POS_LEARNED, "rotary": _lib.VR_POS_ROTARY, "none": _lib.VR_POS_NONE}
        ffns = {"gelu": _lib.VR_FFN_GELU, "swiglu": _lib.VR_FFN_SWIGLU, "geglu": _lib.VR_FFN_GEGLU, "relu": _lib.VR_FFN_RELU}
        if self.position not in positions:
            raise ValueError(f"unknown position scheme {self.position!r}")
        if self.ffn not in ffns:
            raise ValueError(f"unknown ffn kind {self.ffn!r}")
        d.position, d.rope_theta, d.ffn = positions[self.position], float(self.rope_theta), ffns[self.ffn]
        norms = {"post": _lib.VR_NORM_POST, "pre": _lib.VR_NORM_PRE, "rms_pre": _lib.VR_NORM_PRE_RMS,
                 "rms_pre_rotary": _lib.VR_NORM_PRE_RMS_ROTARY}
        if self.norm not in norms:
            raise ValueError(f"unknown norm placement {self.norm!r}")
        d.norm, d.window, d.global_every = norms[self.norm], int(self.window), int(self.global_every)
        d.rope_theta_local = float(self.rope_theta_local)
        if self.causal:
            d.causal = int(self.causal)
        if v3:
            d.head_dim, d.qk_norm = int(self.head_dim), int(self.qk_norm)
        return d


def tensor_names(layers: int) -> list[str]:
    names = list(EMB_SUFFIXES)
    for i in range(layers):
        names += [f"encoder.layer.{i}.{s}" for s in LAYER_SUFFIXES]
    return names


def rope_tensor_names(layers: int) -> list:
    """The slots of a rotary, gated model (5 + 18 per layer) by native name; None = no tensor (NULL)."""
    names = list(ROPE_EMB_SUFFIXES)
    for i in range(layers):
        names += [None if s is None else f"layers.{i}.{s}" for s in ROPE_LAYER_SUFFIXES]
    return names


def names_for(desc: "BertDesc") -> list:
    """Tensor names by family: BERT / XLM-RoBERTa state-dict names, or the rotary gated family's (a pre-norm model's
    state is brought to those by modernbert_slots, which also knows which biases it has)."""
    if desc.rotary != desc.gated:
        raise ValueError("checkpoints are read for BERT-style (learned positions, GELU) and nomic-style (rotary, gated "
                         f"FFN) encoders; got position={desc.position!r} with ffn={desc.ffn!r}")
    return rope_tensor_names(desc.layers) if desc.rotary else tensor_names(desc.layers)


def native_rope_state(state: dict) -> dict:
    """A nomic-style state dict under its native names: hub-named entries (encoder.layers.N.attn.Wqkv, mlp.fc11, norm1,
    emb_ln, ...) are renamed and the fused Wqkv split in thirds along dim 0; native entries pass through."""
    out = {}
    for k, v in state.items():
        for old, new in HUB_RENAMES:
            k = k.replace(old, new)
        if ".attn.Wqkv." in k:
            if v.shape[0] % 3:
                raise ValueError(f"weight '{k}' has {v.shape[0]} rows, not three equal parts")
            n = v.shape[0] // 3
            for j, part in enumerate(("q_proj", "k_proj", "v_proj")):
                out[k.replace(".attn.Wqkv.", f".self_attn.{part}.")] = v[j * n:(j + 1) * n]
        else:
            out[k] = v
    return out


# A pre-norm encoder (model_type modernbert) in the slot order of vr_encoder_load. Every slot is named here — these
# checkpoints may carry biases (attention_bias, mlp_bias, norm_bias) — under the rotary family's native names, which
# modernbert_slots maps a ModernBertModel state dict to.
PRENORM_LAYER_SUFFIXES = [
    "self_attn.q_proj.weight", "self_attn.q_proj.bias", "self_attn.k_proj.weight", "self_attn.k_proj.bias",
    "self_attn.v_proj.weight", "self_attn.v_proj.bias", "self_attn.o_proj.weight", "self_attn.o_proj.bias",
    "post_attention_layernorm.weight", "post_attention_layernorm.bias",
    "mlp.up_proj.weight", "mlp.up_proj.bias", "mlp.down_proj.weight", "mlp.down_proj.bias",
    "post_mlp_layernorm.weight", "post_mlp_layernorm.bias",
    "mlp.gate_proj.weight", "mlp.gate_proj.bias",
]


def modernbert_slots(state: dict, desc: "BertDesc"):
    """A transformers ModernBertModel state dict (any key prefix) -> (slot names, state under those names).
    Under VR_NORM_PRE a LayerNorm slot holds the norm that follows the residual add it sits behind: layer l's
    post_attention_layernorm is layers.l.mlp_norm, its post_mlp_layernorm is layers.l+1.attn_norm — final_norm for the
    last layer — and layers.0 has no attn_norm (the embedding norm's rows go straight into its attention). attn.Wqkv is
    split in thirds (query, key, value); mlp.Wi in halves: rows [0, I) are what the activation is applied to (the GATE),
    rows [I, 2I) the UP projection. What these checkpoints lack is filled in here: zeros for an absent LayerNorm shift,
    a [1, H] zero table for the token types; an absent projection bias stays an empty (NULL) slot."""
    H, inter, L = desc.hidden, desc.intermediate, desc.layers

    def get(name, optional=False):
        hits = [k for k in state if k == name or k.endswith("." + name)]
        if not hits and optional:
            return None
        if len(hits) != 1:
            raise KeyError(f"weight '{name}' not found (or ambiguous) in state dict: {hits[:3]}")
        return state[hits[0]]

    def rows(t, name, parts):
        if t.shape[0] % parts:
            raise ValueError(f"weight '{name}' has {t.shape[0]} rows, not {parts} equal parts")
        n = t.shape[0] // parts
        return [t[j * n:(j + 1) * n] for j in range(parts)]

    zeros_h = np.zeros(H, np.float32)
    out = {"embeddings.word_embeddings.weight": get("embeddings.tok_embeddings.weight"),
           "embeddings.token_type_embeddings.weight": np.zeros((1, H), np.float32)}

    def norm(dst, src):
        out[dst + ".weight"] = get(src + ".weight")
        b = get(src + ".bias", optional=True)
        out[dst + ".bias"] = zeros_h if b is None else b

    norm("embeddings.LayerNorm", "embeddings.norm")
    for i in range(L):
        p = f"layers.{i}."
        for kind in ("weight", "bias"):
            t = get(p + "attn.Wqkv." + kind, optional=kind == "bias")
            if t is not None:
                for part, name in zip(rows(t, p + "attn.Wqkv." + kind, 3), ("q_proj", "k_proj", "v_proj")):
                    out[p + "self_attn." + name + "." + kind] = part
            t = get(p + "mlp.Wi." + kind, optional=kind == "bias")
            if t is not None:
                out[p + "mlp.gate_proj." + kind], out[p + "mlp.up_proj." + kind] = rows(t, p + "mlp.Wi." + kind, 2)
            for dst, src in (("self_attn.o_proj", "attn.Wo"), ("mlp.down_proj", "mlp.Wo")):
                t = get(p + src + "." + kind, optional=kind == "bias")
                if t is not None:
                    out[p + dst + "." + kind] = t
        norm(p + "post_attention_layernorm", p + "mlp_norm")
        norm(p + "post_mlp_layernorm", f"layers.{i + 1}.attn_norm" if i + 1 < L else "final_norm")
    names = ["embeddings.word_embeddings.weight", None, "embeddings.token_type_embeddings.weight",
             "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"]
    for i in range(L):
        names += [n if n in out else None for n in (f"layers.{i}.{s}" for s in PRENORM_LAYER_SUFFIXES)]
    return names, out


def mpnet_relative_position_bucket(relative_position, num_buckets: int = 32, max_distance: int = 128):
    """transformers' MPNetEncoder.relative_position_bucket, operation for operation (torch's f32 log decides the bucket
    at the logarithmic edges, so it is torch here too): relative_position = key - query, int64 tensor -> bucket."""
    import math

    import torch

    ret = 0
    n = -relative_position
    num_buckets //= 2
    ret += (n < 0).to(torch.long) * num_buckets
    n = torch.abs(n)
    max_exact = num_buckets // 2
    is_small = n < max_exact
    val_if_large = max_exact + (
        torch.log(n.float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)
    ).to(torch.long)
    val_if_large = torch.min(val_if_large, torch.full_like(val_if_large, num_buckets - 1))
    ret += torch.where(is_small, n, val_if_large)
    return ret


def mpnet_bias_table(weight, radius: int = 128) -> np.ndarray:
    """encoder.relative_attention_bias.weight [buckets, heads] -> float32 [heads, 2 * radius + 1], the table
    vr_encoder_set_attention_bias takes: entry [h, d + radius] is the bias of key - query = d. The buckets depend on
    key - query alone and saturate at |d| = 128, so radius 128 reproduces compute_position_bias at every length."""
    import torch

    if hasattr(weight, "detach"):
        weight = weight.detach().cpu().numpy()
    w = torch.from_numpy(np.array(weight, dtype=np.float32))
    if w.ndim != 2 or w.shape[0] % 2:
        raise ValueError(f"relative_attention_bias.weight of shape {tuple(w.shape)}: expected [an even bucket count, heads]")
    if radius < 128:
        raise ValueError(f"radius {radius}: the buckets saturate at a distance of 128 only")
    rel = torch.arange(-radius, radius + 1, dtype=torch.long)
    bucket = mpnet_relative_position_bucket(rel, num_buckets=int(w.shape[0]))
    return np.ascontiguousarray(w[bucket].T.numpy(), dtype=np.float32)


def mpnet_slots(state: dict, desc: "BertDesc", pos_start: int = 2):
    """A transformers MPNetModel state dict (with or without the `mpnet.` prefix) -> (state under the BERT names of
    tensor_names(), bias table). MPNet is a post-LayerNorm BERT without token types whose positions start at row
    padding_idx + 1 = 2: the token-type slot is a zero [1, H] row and the position table is taken from row pos_start.
    encoder.relative_attention_bias.weight, shared by all layers, becomes the offset table of mpnet_bias_table."""

    def get(name):
        hits = [k for k in state if k == name or k.endswith("." + name)]
        if len(hits) != 1:
            raise KeyError(f"weight '{name}' not found (or ambiguous) in state dict: {hits[:3]}")
        return state[hits[0]]

    out = {"embeddings.word_embeddings.weight": get("embeddings.word_embeddings.weight"),
           "embeddings.position_embeddings.weight": get("embeddings.position_embeddings.weight")[pos_start:],
           "embeddings.token_type_embeddings.weight": np.zeros((1, desc.hidden), np.float32),
           "embeddings.LayerNorm.weight": get("embeddings.LayerNorm.weight"),
           "embeddings.LayerNorm.bias": get("embeddings.LayerNorm.bias")}
    renames = [("attention.self.query", "attention.attn.q"), ("attention.self.key", "attention.attn.k"),
               ("attention.self.value", "attention.attn.v"), ("attention.output.dense", "attention.attn.o"),
               ("attention.output.LayerNorm", "attention.LayerNorm"), ("intermediate.dense", "intermediate.dense"),
               ("output.dense", "output.dense"), ("output.LayerNorm", "output.LayerNorm")]
    for i in range(desc.layers):
        for dst, src in renames:
            for kind in ("weight", "bias"):
                out[f"encoder.layer.{i}.{dst}.{kind}"] = get(f"encoder.layer.{i}.{src}.{kind}")
    return out, mpnet_bias_table(get("encoder.relative_attention_bias.weight"))


def t5_bias_table(weight, num_buckets: int = 32, max_distance: int = 128) -> np.ndarray:
    """encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight [num_buckets, heads] -> float32
    [heads, 2 * max_distance + 1], the table vr_encoder_set_attention_bias takes: entry [h, d + max_distance] is the bias
    of key - query = d. T5's bidirectional _relative_position_bucket is MPNet's function (MPNet took it from T5), its
    logarithm in f32 as the library's; the buckets are constant from |d| = max_distance on, so that radius reproduces
    compute_bias at every length."""
    import torch

    if hasattr(weight, "detach"):
        weight = weight.detach().cpu().numpy()
    w = torch.from_numpy(np.array(weight, dtype=np.float32))
    if w.ndim != 2 or w.shape[0] != num_buckets or num_buckets % 2:
        raise ValueError(f"relative_attention_bias.weight of shape {tuple(w.shape)}: expected [relative_attention_num_buckets "
                         f"= {num_buckets} (even), heads]")
    if not 1 <= max_distance <= 512:
        raise ValueError(f"relative_attention_max_distance {max_distance}: the engine's bias table has a radius of 1..512")
    rel = torch.arange(-max_distance, max_distance + 1, dtype=torch.long)
    bucket = mpnet_relative_position_bucket(rel, num_buckets=num_buckets, max_distance=max_distance)
    return np.ascontiguousarray(w[bucket].T.numpy(), dtype=np.float32)


def t5_slots(state: dict, desc: "BertDesc", num_buckets: int = 32, max_distance: int = 128, table: bool = True):
    """A transformers T5EncoderModel (or T5Model / T5ForConditionalGeneration: its encoder half) state dict, any key
    prefix -> (slot names, state under those names, bias table). The 16-slot layout under BERT's names with every bias,
    the position table and the token types absent (NULL). Under VR_NORM_PRE_RMS embeddings.LayerNorm holds block 0's
    attention norm, layer l's attention.output.LayerNorm its layer.1.layer_norm (in front of the FFN) and its
    output.LayerNorm block l + 1's layer.0.layer_norm, final_layer_norm for the last. T5's logits carry no
    1/sqrt(d_kv); the engine's do, so q.weight is multiplied by sqrt(d_kv) in f32 here (exactly x8 at d_kv = 64, one
    rounding per weight at 32). The table is t5_bias_table of block 0's relative_attention_bias (table=False: None, for
    a caller that has it already)."""

    def get(*names):
        hits = [k for k in state for name in names if k == name or k.endswith("." + name)]
        if names[0] == "shared.weight":  # (the tied embedding may be present under both names)
            hits = hits[:1]
        if len(hits) != 1:
            raise KeyError(f"weight '{names[0]}' not found (or ambiguous) in state dict: {hits[:3]}")
        t = state[hits[0]]
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    if not any(k == "encoder.block.0.layer.0.SelfAttention.q.weight" or k.endswith(".encoder.block.0.layer.0.SelfAttention.q.weight")
               for k in state):
        raise KeyError("weight 'encoder.block.0.layer.0.SelfAttention.q.weight' not found: the state dict holds no T5 "
                       "encoder weights")
    L, dkv = desc.layers, desc.hidden // desc.heads
    scale = np.sqrt(np.float32(dkv))
    out = {"embeddings.word_embeddings.weight": get("shared.weight", "encoder.embed_tokens.weight"),
           "embeddings.LayerNorm.weight": get("encoder.block.0.layer.0.layer_norm.weight")}
    names = ["embeddings.word_embeddings.weight", None, None, "embeddings.LayerNorm.weight", None]
    for i in range(L):
        src, dst = f"encoder.block.{i}.", f"encoder.layer.{i}."
        nxt = f"encoder.block.{i + 1}.layer.0.layer_norm.weight" if i + 1 < L else "encoder.final_layer_norm.weight"
        q = np.asarray(get(src + "layer.0.SelfAttention.q.weight"), np.float32)
        layer = [("attention.self.query.weight", (q * scale).astype(np.float32)),
                 ("attention.self.key.weight", get(src + "layer.0.SelfAttention.k.weight")),
                 ("attention.self.value.weight", get(src + "layer.0.SelfAttention.v.weight")),
                 ("attention.output.dense.weight", get(src + "layer.0.SelfAttention.o.weight")),
                 ("attention.output.LayerNorm.weight", get(src + "layer.1.layer_norm.weight")),
                 ("intermediate.dense.weight", get(src + "layer.1.DenseReluDense.wi.weight")),
                 ("output.dense.weight", get(src + "layer.1.DenseReluDense.wo.weight")),
                 ("output.LayerNorm.weight", get(nxt))]
        for name, t in layer:
            out[dst + name] = t
            names += [dst + name, None]
    bias = None
    if table:
        bias = t5_bias_table(get("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"), num_buckets,
                             max_distance)
    return names, out, bias


def qwen2_slots(state: dict, desc: "BertDesc", kv_heads: int | None = None, *, family: str = "Qwen2"):
    """A transformers Qwen2Model (or Qwen2ForCausalLM) state dict, any key prefix -> (slot names, state under those
    names): the 18-slot gated layout under the rotary family's native names, with no position table, no token types and
    no norm shifts (NULL), biases on q/k/v only. Under VR_NORM_PRE_RMS_ROTARY embeddings.LayerNorm holds
    layers.0.input_layernorm, layer l's post_attention_layernorm its own, and its post_mlp_layernorm
    layers.l+1.input_layernorm — `norm` for the last.
    Grouped-query attention is resolved here: k_proj and v_proj (weights and biases) of KV head j are repeated for the
    query heads j g .. j g + g - 1, g = heads / kv_heads (HF repeat_kv), so the engine sees `heads` full heads. kv_heads:
    num_key_value_heads, or None to read it off k_proj's rows. lm_head.* is ignored; any other tensor left over is
    refused by name."""
    used = set()

    def get(name, optional=False):
        hits = [k for k in state if k == name or k.endswith("." + name)]
        if not hits and optional:
            return None
        if len(hits) != 1:
            raise KeyError(f"weight '{name}' not found (or ambiguous) in state dict: {hits[:3]}")
        used.add(hits[0])
        t = state[hits[0]]
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    heads, L = desc.heads, desc.layers
    dh = desc.head_size
    qwen3 = family == "Qwen3"  # (q/k/v biases only where the checkpoint has them, and the two per-head norm weights)
    if kv_heads is None:
        rows = int(get("layers.0.self_attn.k_proj.weight").shape[0])
        if rows % dh:
            raise ValueError(f"weight 'layers.0.self_attn.k_proj.weight' has {rows} rows, not whole heads of {dh}")
        kv_heads = rows // dh
    if kv_heads < 1 or heads % kv_heads:
        raise ValueError(f"num_attention_heads {heads} is not a multiple of num_key_value_heads {kv_heads}")
    g = heads // kv_heads

    def repeat_kv(t, name):
        if t.shape[0] != kv_heads * dh:
            raise ValueError(f"weight '{name}' has {t.shape[0]} rows, num_key_value_heads {kv_heads} of head size {dh} "
                             f"imply {kv_heads * dh}")
        if g == 1:
            return t
        return np.ascontiguousarray(np.repeat(t.reshape(kv_heads, dh, *t.shape[1:]), g, axis=0).reshape(heads * dh, *t.shape[1:]))

    out = {"embeddings.word_embeddings.weight": get("embed_tokens.weight"),
           "embeddings.LayerNorm.weight": get("layers.0.input_layernorm.weight")}
    names = ["embeddings.word_embeddings.weight", None, None, "embeddings.LayerNorm.weight", None]
    for i in range(L):
        p = f"layers.{i}."
        for kind in ("weight", "bias"):
            optional = qwen3 and kind == "bias"
            t = get(p + "self_attn.q_proj." + kind, optional)
            if t is not None:
                out[p + "self_attn.q_proj." + kind] = t
            for part in ("k_proj", "v_proj"):
                name = p + "self_attn." + part + "." + kind
                t = get(name, optional)
                if t is not None:
                    out[name] = repeat_kv(t, name)
        out[p + "self_attn.o_proj.weight"] = get(p + "self_attn.o_proj.weight")
        for part in ("gate_proj", "up_proj", "down_proj"):
            out[p + "mlp." + part + ".weight"] = get(p + "mlp." + part + ".weight")
        out[p + "post_attention_layernorm.weight"] = get(p + "post_attention_layernorm.weight")
        out[p + "post_mlp_layernorm.weight"] = get(f"layers.{i + 1}.input_layernorm.weight" if i + 1 < L else "norm.weight")
        names += [n if n in out else None for n in (p + s for s in PRENORM_LAYER_SUFFIXES)]
        if desc.qk_norm:  # slots 18 and 19
            for part in QK_NORM_SUFFIXES:
                out[p + part] = get(p + part)
                names.append(p + part)
    extra = sorted(k for k in state if k not in used and "lm_head" not in k.split("."))
    if extra:
        raise ValueError(f"not a {family} state dict of {L} layers: unexpected tensors {extra[:4]}{' ...' if len(extra) > 4 else ''}")
    return names, out


QK_NORM_SUFFIXES = ["self_attn.q_norm.weight", "self_attn.k_norm.weight"]


def qwen3_slots(state: dict, desc: "BertDesc", kv_heads: int | None = None):
    """A transformers Qwen3Model (or Qwen3ForCausalLM) state dict, any key prefix -> (slot names, state under those
    names): qwen2_slots' layout with heads of desc.head_dim (q_proj is [heads * head_dim, hidden], o_proj its transpose
    shape, repeat_kv runs over KV heads of head_dim rows), q/k/v biases only where the checkpoint has them
    (attention_bias), and with desc.qk_norm two slots more per layer, 18: self_attn.q_norm.weight, 19:
    self_attn.k_norm.weight, [head_dim] each. lm_head.* is ignored; any other tensor left over is refused by name."""
    return qwen2_slots(state, desc, kv_heads, family="Qwen3")


def distilbert_slots(state: dict, desc: "BertDesc") -> dict:
    """A transformers DistilBertModel state dict (with or without the `distilbert.` prefix) -> the state under the BERT
    names of tensor_names(). DistilBERT is BERT's post-LayerNorm body without token types: the token-type slot is a zero
    [1, H] row, transformer.layer.N's attention.{q,k,v,out}_lin, sa_layer_norm, ffn.lin1 / lin2 and output_layer_norm
    are BERT's query / key / value / attention.output.dense, attention.output.LayerNorm, intermediate / output dense
    and output.LayerNorm."""

    def get(name):
        hits = [k for k in state if k == name or k.endswith("." + name)]
        if len(hits) != 1:
            raise KeyError(f"weight '{name}' not found (or ambiguous) in state dict: {hits[:3]}")
        return state[hits[0]]

    out = {"embeddings.word_embeddings.weight": get("embeddings.word_embeddings.weight"),
           "embeddings.position_embeddings.weight": get("embeddings.position_embeddings.weight"),
           "embeddings.token_type_embeddings.weight": np.zeros((1, desc.hidden), np.float32),
           "embeddings.LayerNorm.weight": get("embeddings.LayerNorm.weight"),
           "embeddings.LayerNorm.bias": get("embeddings.LayerNorm.bias")}
    renames = [("attention.self.query", "attention.q_lin"), ("attention.self.key", "attention.k_lin"),
               ("attention.self.value", "attention.v_lin"), ("attention.output.dense", "attention.out_lin"),
               ("attention.output.LayerNorm", "sa_layer_norm"), ("intermediate.dense", "ffn.lin1"),
               ("output.dense", "ffn.lin2"), ("output.LayerNorm", "output_layer_norm")]
    for i in range(desc.layers):
        for dst, src in renames:
            for kind in ("weight", "bias"):
                out[f"encoder.layer.{i}.{dst}.{kind}"] = get(f"transformer.layer.{i}.{src}.{kind}")
    return out


def alibi_slopes(heads: int) -> np.ndarray:
    """The standard ALiBi slope of every head, float32 [heads] (Press et al., as BLOOM's build_alibi_tensor and
    JinaBert compute them): for a power-of-two n the geometric sequence start^(i + 1), start = 2^(-8/n); otherwise
    the sequence of the largest power of two below n, followed by every second slope of the sequence for twice that."""
    if heads < 1:
        raise ValueError(f"alibi_slopes of {heads} heads")

    def power_of_two(n):
        start = 2.0 ** (-8.0 / n)
        return [start ** (i + 1) for i in range(n)]

    closest = 1 << (heads.bit_length() - 1)
    slopes = power_of_two(closest)
    if closest != heads:
        slopes += power_of_two(2 * closest)[0::2][:heads - closest]
    return np.asarray(slopes, dtype=np.float32)


# An ALiBi encoder (jina-embeddings-v2: model_type bert, position_embedding_type alibi) in the slot order of
# vr_encoder_load: a post-LayerNorm BERT body without a position table whose FFN is gated (GeGLU) and carries a bias
# on its down projection only. The names jina_slots files a JinaBert state dict under.
JINA_LAYER_SUFFIXES = [
    "attention.self.query.weight", "attention.self.query.bias",
    "attention.self.key.weight", "attention.self.key.bias",
    "attention.self.value.weight", "attention.self.value.bias",
    "attention.output.dense.weight", "attention.output.dense.bias",
    "attention.output.LayerNorm.weight", "attention.output.LayerNorm.bias",
    "mlp.up_proj.weight", None, "mlp.down_proj.weight", "mlp.down_proj.bias",
    "mlp.layernorm.weight", "mlp.layernorm.bias",
    "mlp.gate_proj.weight", None,
]


def jina_slots(state: dict, desc: "BertDesc"):
    """A JinaBertModel state dict (any key prefix) -> (slot names, state under those names): the 18-slot gated layout
    with no position table. mlp.gated_layers.weight is [2I, H] without a bias: rows [0, I) are what the activation is
    applied to (the GATE), rows [I, 2I) the UP projection; mlp.wo is the down projection and mlp.layernorm the output
    LayerNorm. pooler.*, cls.* and position_ids are ignored; ANY other tensor left over is refused by name — the
    -code, -de, -es and -zh checkpoints carry LayerNorms on Q and K (layer_norm_q / layer_norm_k), which is another
    model and must not load as this one."""
    used = set()

    def get(name):
        hits = [k for k in state if k == name or k.endswith("." + name)]
        if len(hits) != 1:
            raise KeyError(f"weight '{name}' not found (or ambiguous) in state dict: {hits[:3]}")
        used.add(hits[0])
        return state[hits[0]]

    out = {}
    for name in ("embeddings.word_embeddings.weight", "embeddings.token_type_embeddings.weight",
                 "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"):
        out[name] = get(name)
    inter = desc.intermediate
    for i in range(desc.layers):
        p = f"encoder.layer.{i}."
        for s in JINA_LAYER_SUFFIXES[:10]:
            out[p + s] = get(p + s)
        gated = get(p + "mlp.gated_layers.weight")
        if tuple(gated.shape) != (2 * inter, desc.hidden):
            raise ValueError(f"weight '{p}mlp.gated_layers.weight' has shape {tuple(gated.shape)}, the model description "
                             f"implies {(2 * inter, desc.hidden)}")
        out[p + "mlp.gate_proj.weight"], out[p + "mlp.up_proj.weight"] = gated[:inter], gated[inter:]
        out[p + "mlp.down_proj.weight"] = get(p + "mlp.wo.weight")
        out[p + "mlp.down_proj.bias"] = get(p + "mlp.wo.bias")
        out[p + "mlp.layernorm.weight"] = get(p + "mlp.layernorm.weight")
        out[p + "mlp.layernorm.bias"] = get(p + "mlp.layernorm.bias")

    def ignored(key):
        parts = key.split(".")
        return "pooler" in parts or "cls" in parts or parts[-1] == "position_ids"

    extra = sorted(k for k in state if k not in used and not ignored(k))
    if extra:
        raise ValueError(f"not a JinaBert (jina-embeddings-v2 -small-en / -base-en) state dict: unexpected tensors {extra[:4]}"
                         f"{' ...' if len(extra) > 4 else ''}; the variant with LayerNorms on Q and K (layer_norm_q / "
                         "layer_norm_k: the -code, -de, -es and -zh checkpoints) is not implemented")
    names = ["embeddings.word_embeddings.weight", None, "embeddings.token_type_embeddings.weight",
             "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"]
    for i in range(desc.layers):
        names += [None if s is None else f"encoder.layer.{i}.{s}" for s in JINA_LAYER_SUFFIXES]
    return names, out


# a BertForSequenceClassification's head, after the encoder's tensors (vr_reranker_load)
HEAD_NAMES = ["pooler.dense.weight", "pooler.dense.bias", "classifier.weight", "classifier.bias"]
# a ModernBertForSequenceClassification's: classifier(norm(gelu(dense(pooled row)))), six tensors
PRENORM_HEAD_NAMES = ["head.dense.weight", "head.dense.bias", "head.norm.weight", "head.norm.bias", "classifier.weight",
                      "classifier.bias"]


# a decoder cross-encoder's (vr_reranker_load_decoder): one row, no bias — Qwen3ForSequenceClassification's score.weight,
# or lm_head[yes] - lm_head[no] of a Qwen3ForCausalLM reranker (qwen3_rerank_head)
DECODER_HEAD_NAMES = ["score.weight"]


def qwen3_rerank_head(state: dict, desc: "BertDesc", yes_id: int | None = None, no_id: int | None = None) -> np.ndarray:
    """The head row of a decoder cross-encoder, [1, H] f32. A state dict with `score.weight` (a one-label
    Qwen3ForSequenceClassification / Qwen2ForSequenceClassification): that tensor as stored. Otherwise (Qwen3ForCausalLM /
    Qwen2ForCausalLM, Qwen3-Reranker's published form) W[yes_id] - W[no_id], W = lm_head.weight or, where the embeddings
    are tied and the checkpoint holds no lm_head, embed_tokens.weight: softmax over (W[no] . h, W[yes] . h) taken at
    "yes" is sigmoid((W[yes] - W[no]) . h). The difference is taken in f64 and rounded once."""

    def find(name):
        hits = [k for k in state if k == name or k.endswith("." + name)]
        if len(hits) > 1:
            raise KeyError(f"weight '{name}' is ambiguous in state dict: {hits[:3]}")
        if not hits:
            return None
        t = state[hits[0]]
        return t.detach().cpu().float().numpy() if hasattr(t, "detach") else np.asarray(t)

    score = find("score.weight")
    if score is not None:
        if tuple(score.shape) != (1, desc.hidden):
            raise ValueError(f"weight 'score.weight' has shape {tuple(score.shape)}: a one-label head is {(1, desc.hidden)}")
        return np.ascontiguousarray(score, np.float32)
    W = find("lm_head.weight")
    name = "lm_head.weight"
    if W is None:
        W, name = find("embed_tokens.weight"), "embed_tokens.weight"
    if W is None:
        raise KeyError("weight 'score.weight', 'lm_head.weight' or 'embed_tokens.weight' not found in state dict")
    if W.ndim != 2 or W.shape[1] != desc.hidden:
        raise ValueError(f"weight '{name}' has shape {tuple(W.shape)}, the model description implies (vocab, {desc.hidden})")
    for what, i in (("yes", yes_id), ("no", no_id)):
        if i is None:
            raise ValueError(f"the id of the token '{what}' is missing: a causal-LM reranker scores lm_head[yes] - lm_head[no]")
        if not 0 <= int(i) < W.shape[0]:
            raise ValueError(f"the id {int(i)} of the token '{what}' is outside the {W.shape[0]} rows of '{name}'")
    row = W[int(yes_id)].astype(np.float64) - W[int(no_id)].astype(np.float64)
    return np.ascontiguousarray(row.astype(np.float32)[None, :])


def modernbert_head(state: dict, desc: "BertDesc") -> dict:
    """The six head tensors of a ModernBertForSequenceClassification state dict (any key prefix) under
    PRENORM_HEAD_NAMES; zeros for an absent head.dense.bias (classifier_bias false) or head.norm.bias (norm_bias
    false), as modernbert_slots fills in an absent LayerNorm shift."""
    out = {}
    for name in PRENORM_HEAD_NAMES:
        hits = [k for k in state if k == name or k.endswith("." + name)]
        if len(hits) > 1:
            raise KeyError(f"weight '{name}' is ambiguous in state dict: {hits[:3]}")
        if hits:
            out[name] = state[hits[0]]
        elif name in ("head.dense.bias", "head.norm.bias"):
            out[name] = np.zeros(desc.hidden, np.float32)
        else:
            raise KeyError(f"weight '{name}' not found in state dict")
    return out


def expected_shape(desc: BertDesc, name: str) -> tuple:
    """Shape of a state-dict entry as the description implies it ([out, in] layout, as HF stores it)."""
    H, inter = desc.hidden, desc.intermediate
    if desc.head_dim or desc.qk_norm:  # (vr_bert_desc_v3: the attention width and the per-head norm weights)
        A = desc.attn_width
        if name.endswith(("self_attn.q_norm.weight", "self_attn.k_norm.weight")): return (desc.head_size,)
        if name.endswith(("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight")): return (A, H)
        if name.endswith(("self_attn.q_proj.bias", "self_attn.k_proj.bias", "self_attn.v_proj.bias")): return (A,)
        if name.endswith("self_attn.o_proj.weight"): return (H, A)
    if name == "classifier.weight" or name == "score.weight": return (1, H)
    if name == "classifier.bias": return (1,)
    if name.startswith("head.norm."): return (H,)
    if name.endswith("word_embeddings.weight"): return (desc.vocab, H)
    if name.endswith("position_embeddings.weight"): return (desc.max_pos, H)
    if name.endswith("token_type_embeddings.weight"): return (desc.type_vocab, H)
    if name.endswith("mlp.up_proj.weight") or name.endswith("mlp.gate_proj.weight"): return (inter, H)
    if name.endswith("mlp.up_proj.bias") or name.endswith("mlp.gate_proj.bias"): return (inter,)
    if name.endswith("mlp.down_proj.weight"): return (H, inter)
    if name.endswith("intermediate.dense.weight"): return (inter, H)
    if name.endswith("intermediate.dense.bias"): return (inter,)
    if name.endswith("output.dense.weight") and "attention" not in name: return (H, inter)
    if name.endswith(".weight") and "layernorm" not in name.lower(): return (H, H)
    return (H,)


def _find(state: dict, suffix: str):
    if suffix in state:
        return state[suffix]
    hits = [k for k in state if k.endswith("." + suffix)]
    if len(hits) != 1:
        raise KeyError(f"weight '{suffix}' not found (or ambiguous) in state dict: {hits[:3]}")
    return state[hits[0]]


def load_encoder(engine, desc: BertDesc, state: dict) -> None:
    """state: HF BertModel state dict (any key prefix), values NumPy arrays or torch tensors.
    Tensors on the engine's GPU are passed as device pointers, everything else as host memory.
    A description that carries an attention_bias table (MPNet, see mpnet_slots), attention_slopes (ALiBi) or a head /
    truncate_dim sets them once the model is loaded. position "none": a gated description reads a JinaBert state dict
    (jina_slots), a GELU one a BERT state dict without its position table."""
    if desc.prenorm:
        names, state = modernbert_slots(state, desc)
    elif desc.rms_rotary and (desc.head_dim or desc.qk_norm):  # (a Qwen3 state dict: a head size of its own, Q/K norms)
        names, state = qwen3_slots(state, desc)
    elif desc.rms_rotary:  # (a Qwen2 state dict; the K/V heads of grouped-query attention are repeated here)
        names, state = qwen2_slots(state, desc)
    elif desc.rms:  # (a T5 state dict; the description's attention_bias, else the checkpoint's table with T5's defaults)
        names, state, table = t5_slots(state, desc, table=desc.attention_bias is None)
        if table is not None:
            desc = replace(desc, attention_bias=table)
    elif desc.position == "none":
        if desc.gated:
            names, state = jina_slots(state, desc)
        else:
            names = [None if n == EMB_SUFFIXES[1] else n for n in tensor_names(desc.layers)]
    else:
        if desc.rotary or desc.gated:
            state = native_rope_state(state)
        names = names_for(desc)
    _load(engine, desc, state, names, engine._lib.vr_encoder_load)
    engine.encoder_desc = desc
    if desc.attention_bias is not None:
        engine.set_attention_bias(desc.attention_bias)
    if desc.attention_slopes is not None:
        engine.set_attention_slopes(desc.attention_slopes)
    if desc.head or desc.truncate_dim:
        engine.set_encoder_head(desc.head or [], desc.truncate_dim)


def load_reranker(engine, desc: BertDesc, state: dict, *, yes_id: int | None = None, no_id: int | None = None) -> None:
    """state: a one-label HF BertForSequenceClassification state dict (any key prefix), the encoder's tensors plus the
    pooler and the classifier. desc: CLS pooling, no normalisation. A pre-norm, rotary, gated description: a one-label
    ModernBertForSequenceClassification state dict (modernbert_slots' body, modernbert_head's head), pooling "cls" or
    "mean" (config.json's classifier_pooling), no normalisation. norm "rms_pre_rotary": a decoder cross-encoder
    (vr_reranker_load_decoder) — a Qwen3 / Qwen2 state dict, its body through qwen3_slots / qwen2_slots (grouped-query
    attention resolved here), pooling "last", no normalisation, and qwen3_rerank_head's row: score.weight, or
    lm_head[yes_id] - lm_head[no_id] of a causal-LM checkpoint."""
    if desc.rms_rotary:
        if desc.pooling != "last" or desc.normalize:
            raise ValueError("a decoder reranker reads the last token's row without normalising it")
        head = qwen3_rerank_head(state, desc, yes_id, no_id)
        body = {k: v for k, v in state.items() if "score" not in k.split(".")}
        slots = qwen3_slots if (desc.head_dim or desc.qk_norm) else qwen2_slots
        names, body = slots(body, desc)
        body[DECODER_HEAD_NAMES[0]] = head
        _load(engine, desc, body, names + DECODER_HEAD_NAMES, engine._lib.vr_reranker_load_decoder)
        engine.reranker_desc = desc
        return
    if desc.prenorm and desc.rotary and desc.gated:
        if desc.normalize:
            raise ValueError("a reranker pools without normalising")
        names, body = modernbert_slots({k: v for k, v in state.items() if ".head." not in "." + k
                                        and not k.endswith(("classifier.weight", "classifier.bias"))}, desc)
        body.update(modernbert_head(state, desc))
        _load(engine, desc, body, names + PRENORM_HEAD_NAMES, engine._lib.vr_reranker_load)
        engine.reranker_desc = desc
        return
    if desc.pooling != "cls" or desc.normalize:
        raise ValueError("a reranker pools the [CLS] row without normalising it")
    _load(engine, desc, state, tensor_names(desc.layers) + HEAD_NAMES, engine._lib.vr_reranker_load)
    engine.reranker_desc = desc


def _load(engine, desc: BertDesc, state: dict, names: list[str], load_fn) -> None:
    names, all_names = [n for n in names if n is not None], names
    tensors = [_find(state, n) for n in names]
    # raw pointers cross the C-ABI next: a checkpoint whose config.json disagrees with its weights (padded or
    # resized vocabulary, another max_position_embeddings, ...) must fail HERE, not read past a buffer there
    for name, t in zip(names, tensors):
        want = expected_shape(desc, name)
        if tuple(t.shape) != want:
            raise ValueError(f"weight '{name}' has shape {tuple(t.shape)}, the model description implies {want}")
    on_device = all(hasattr(t, "is_cuda") and t.is_cuda for t in tensors)
    keep, ptrs = [], []
    for t in tensors:
        if on_device:
            import torch

            t = t.detach().to(torch.float32).contiguous()
            ptrs.append(t.data_ptr())
        else:
            if hasattr(t, "detach"):
                t = t.detach().cpu().numpy()
            t = np.ascontiguousarray(t, dtype=np.float32)
            ptrs.append(t.ctypes.data)
        keep.append(t)
    if on_device:
        engine._follow(keep[0])
    it = iter(ptrs)
    ptrs = [None if n is None else next(it) for n in all_names]  # NULL where the family has no tensor for a slot
    arr = (C.c_void_p * len(ptrs))(*ptrs)
    cdesc = desc.to_c()
    check(load_fn(engine.handle, C.byref(cdesc), arr, len(ptrs), VR_MEM_DEVICE if on_device else VR_MEM_HOST))


def encode(engine, ids, offsets, out=None):
    """ids/offsets: NumPy int32 (host) or torch int32 tensors on the GPU. Returns an (n, W) f32
    NumPy array (W = the description's out_dim), or fills/returns ``out`` when a device tensor is given."""
    desc = engine.encoder_desc
    dev_in = hasattr(ids, "is_cuda") and ids.is_cuda
    if dev_in:
        engine._follow(ids)
        n = int(offsets.shape[0]) - 1
        ip, op_ = C.c_void_p(ids.data_ptr()), C.c_void_p(offsets.data_ptr())
        mem = VR_MEM_DEVICE
    else:
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        n = offsets.shape[0] - 1
        ip, op_ = C.c_void_p(ids.ctypes.data), C.c_void_p(offsets.ctypes.data)
        mem = VR_MEM_HOST
    if out is not None and hasattr(out, "is_cuda") and out.is_cuda:
        assert out.is_contiguous() and tuple(out.shape) == (n, desc.out_dim)
        engine._follow(out)
        check(engine._lib.vr_encode(engine.handle, ip, op_, n, mem, C.c_void_p(out.data_ptr()), VR_MEM_DEVICE))
        return out
    res = np.empty((n, desc.out_dim), np.float32)
    check(engine._lib.vr_encode(engine.handle, ip, op_, n, mem, C.c_void_p(res.ctypes.data), VR_MEM_HOST))
    return res


def encode_spans(engine, ids, offsets, span_off, span_tok, out=None):
    """``encode`` with one row per token span (late chunking): span_off (n_seq + 1) gives each sequence's range of
    spans, span_tok (n_spans, 2) their (begin, end) token positions inside that sequence. All four arrays NumPy int32
    (host) or torch int32 tensors on the GPU. Returns an (n_spans, out_dim) f32 NumPy array — the mean of each span's final
    hidden states, normalised as the description says — or fills/returns ``out`` when a device tensor is given."""
    desc = engine.encoder_desc
    dev_in = hasattr(ids, "is_cuda") and ids.is_cuda
    if dev_in:
        engine._follow(ids)
        arrays = [ids, offsets, span_off, span_tok.contiguous()]
        ptrs = [C.c_void_p(a.data_ptr()) for a in arrays]
        n_spans = int(span_off[-1].item()) if int(span_off.shape[0]) else 0
        mem = VR_MEM_DEVICE
    else:
        arrays = [np.ascontiguousarray(a, dtype=np.int32) for a in (ids, offsets, span_off, span_tok)]
        ptrs = [C.c_void_p(a.ctypes.data) for a in arrays]
        n_spans = int(arrays[2][-1]) if arrays[2].shape[0] else 0
        mem = VR_MEM_HOST
    n = int(arrays[1].shape[0]) - 1
    if int(arrays[2].shape[0]) != n + 1:
        raise ValueError(f"span_off has {int(arrays[2].shape[0])} entries for {n} sequences ({n + 1} expected)")
    if int(arrays[3].numel() if dev_in else arrays[3].size) < 2 * max(n_spans, 0):
        raise ValueError(f"span_tok holds fewer than the {n_spans} (begin, end) pairs span_off announces")
    ip, op_, sop, stp = ptrs
    if out is not None and hasattr(out, "is_cuda") and out.is_cuda:
        assert out.is_contiguous() and tuple(out.shape) == (max(n_spans, 0), desc.out_dim)
        engine._follow(out)
        check(engine._lib.vr_encode_spans(engine.handle, ip, op_, n, sop, stp, mem, C.c_void_p(out.data_ptr()),
                                          VR_MEM_DEVICE))
        return out
    res = np.empty((max(n_spans, 0), desc.out_dim), np.float32)
    check(engine._lib.vr_encode_spans(engine.handle, ip, op_, n, sop, stp, mem, C.c_void_p(res.ctypes.data), VR_MEM_HOST))
    return res


def encode_semantic(engine, ids, offsets, unit_off, unit_tok, *, buffer=1, break_permille=50, min_distance=0.0,
                    min_tokens=0, max_tokens=2**31 - 1):
    """Semantic chunking in one forward pass (vr_encode_semantic): the spans of ``encode_spans`` as UNITS —
    in order, never overlapping — of which the device joins neighbours into chunks and returns the chunks' late-chunked
    rows. Arrays as ``encode_spans`` takes them. Returns ``(rows, unit_start, gap_dist)``: (n_chunks, out_dim) f32 in chunk
    order, per unit an int32 1 where it begins a chunk, and per unit the f32 distance of the gap behind it (0 for a
    sequence's last unit) — the values the device decided on."""
    desc = engine.encoder_desc
    dev_in = hasattr(ids, "is_cuda") and ids.is_cuda
    if dev_in:
        engine._follow(ids)
        arrays = [ids, offsets, unit_off, unit_tok.contiguous()]
        ptrs = [C.c_void_p(a.data_ptr()) for a in arrays]
        n_units = int(unit_off[-1].item()) if int(unit_off.shape[0]) else 0
        mem = VR_MEM_DEVICE
    else:
        arrays = [np.ascontiguousarray(a, dtype=np.int32) for a in (ids, offsets, unit_off, unit_tok)]
        ptrs = [C.c_void_p(a.ctypes.data) for a in arrays]
        n_units = int(arrays[2][-1]) if arrays[2].shape[0] else 0
        mem = VR_MEM_HOST
    n = int(arrays[1].shape[0]) - 1
    if int(arrays[2].shape[0]) != n + 1:
        raise ValueError(f"unit_off has {int(arrays[2].shape[0])} entries for {n} sequences ({n + 1} expected)")
    if int(arrays[3].numel() if dev_in else arrays[3].size) < 2 * max(n_units, 0):
        raise ValueError(f"unit_tok holds fewer than the {n_units} (begin, end) pairs unit_off announces")
    params = _lib.VrSemanticParams(C.sizeof(_lib.VrSemanticParams), int(buffer), int(break_permille), int(min_tokens),
                                   int(max_tokens), float(min_distance))
    rows = np.empty((max(n_units, 0), desc.out_dim), np.float32)
    start = np.zeros(max(n_units, 0), np.int32)
    dist = np.zeros(max(n_units, 0), np.float32)
    n_chunks = C.c_int32(0)
    check(engine._lib.vr_encode_semantic(engine.handle, *ptrs[:2], n, *ptrs[2:], mem, C.byref(params),
                                         C.c_void_p(rows.ctypes.data), C.c_void_p(start.ctypes.data),
                                         C.c_void_p(dist.ctypes.data), C.byref(n_chunks), VR_MEM_HOST))
    return rows[:n_chunks.value].copy(), start, dist
