"""Drop-in for the reference's EmbeddingService (src/voitta/services/embedding.py): same class,
method names, e5 prefix rules, batch argument and return types (plain Python lists).

``SentenceTransformer(model_name, device)`` (embedding.py:40) is replaced by NativeSentenceEncoder:
the checkpoint directory is read the way sentence-transformers reads it (config.json, modules.json,
1_Pooling/config.json, sentence_bert_config.json, tokenizer.json / vocab.txt, model.safetensors),
PyTorch only loads and holds the weights, the HF ``tokenizers`` library (the one
sentence-transformers itself uses) produces WordPiece ids, and the forward pass runs in the HIP
engine (vr_encode). There is no CPU path: EMBEDDING_DEVICE=cpu raises."""
from __future__ import annotations

import json
import logging
import os

import numpy as np

from . import deferred as _deferred
from . import encoder as _enc
from . import late_chunking as _late
from . import semantic_chunking as _semantic
from .bpe import BpeTokenizer
from .config import MAX_SEQ_LENGTH_LIMIT, get_settings
from .store_registry import get_engine
from .unigram import UnigramTokenizer, is_unigram_pipeline
from .wordpiece import WordPieceTokenizer

logger = logging.getLogger(__name__)

# the default cap on a sequence's tokens; VOITTA_MAX_SEQ_LENGTH (1 ... 8192) sets another one, see seq_cap()
MAX_SEQ = 512
SEQ_CAP_VARIABLE = "VOITTA_MAX_SEQ_LENGTH"
TRUNCATE_VARIABLE = "VOITTA_EMBED_TRUNCATE_DIM"


def seq_cap() -> int:
    """The longest sequence a model may run: the VOITTA_MAX_SEQ_LENGTH setting, MAX_SEQ when it is unset."""
    return get_settings().max_seq_length


# vr_query_text(_batch) take a max_len of at most this (a question is not a document)
TEXT_PATH_MAX_LEN = 4096


def one_call_text_paths(model) -> bool:
    """Whether questions for `model` go through vr_query_text(_batch): a tokenizer of the engine, and a sequence cap those
    calls accept. Otherwise they are tokenised, encoded and searched in calls of their own, with the same result."""
    return native_tokenizer(model.tokenizer) and model.max_seq_length <= TEXT_PATH_MAX_LEN


def native_tokenizer(tok) -> bool:
    """A tokenizer of the engine itself (WordPiece, Unigram or byte-level BPE): the one-call text paths (vr_query_text(_batch), the
    deferred write-behind) take models with one; a tokenizers-library object goes through several calls instead."""
    return isinstance(tok, (WordPieceTokenizer, UnigramTokenizer, BpeTokenizer))


def read_encoder_config(path: str) -> dict:
    """config.json, modules.json and sentence_bert_config.json of a sentence-transformers directory -> the encoder
    description and how to load it: {"desc": BertDesc, "max_seq": int, "pos_start": first position-table row}.
    BERT: max_seq = min(max_seq_length, max_position_embeddings). XLM-RoBERTa (multilingual-e5 and the like): position
    p reads row pad_token_id + 1 + p, so the table is used from that row on (max_pos = max_position_embeddings -
    pad_token_id - 1); one token type; max_seq = min(max_seq_length, max_pos), refused above seq_cap().
    The description carries the modules behind Pooling as its head (read_head) and VOITTA_EMBED_TRUNCATE_DIM as its
    truncate_dim (apply_truncate_setting)."""
    cfg = json.load(open(os.path.join(path, "config.json")))
    rc = _read_family_config(path, cfg)
    rc["desc"].head = read_head(path, rc["desc"].hidden) or None
    apply_truncate_setting(rc["desc"])
    return rc


def apply_truncate_setting(desc) -> None:
    """VOITTA_EMBED_TRUNCATE_DIM (SentenceTransformer's truncate_dim) onto a description: the leading columns of the
    model's output — its head's, when it has one — are the embedding. Refused unless it is a multiple of 16 within that
    width, and unless EMBEDDING_DIMENSION, the width of the store, is the width that results."""
    settings = get_settings()
    keep = settings.embed_truncate_dim
    if not keep:
        return
    width = desc.out_dim
    if keep % 16 or not 16 <= keep <= width:
        raise ValueError(f"{TRUNCATE_VARIABLE}={keep}: accepted values are the multiples of 16 from 16 to the model's "
                         f"output width {width}")
    desc.truncate_dim = keep
    if settings.embedding_dimension != desc.out_dim:
        raise ValueError(f"EMBEDDING_DIMENSION={settings.embedding_dimension} but {TRUNCATE_VARIABLE}={keep} makes the "
                         f"embeddings {desc.out_dim} wide: set EMBEDDING_DIMENSION={desc.out_dim}")


def _read_family_config(path: str, cfg: dict) -> dict:
    kind = cfg.get("model_type", "bert")
    if kind == "nomic_bert":
        return _read_rope_config(path, cfg)
    if kind == "modernbert":
        return _read_modernbert_config(path, cfg)
    if kind == "mpnet":
        return _read_mpnet_config(path, cfg)
    if kind == "distilbert":
        return _read_distilbert_config(path, cfg)
    if kind == "t5":
        return _read_t5_config(path, cfg)
    if kind == "qwen2":
        return _read_qwen2_config(path, cfg)
    unsupported = (f"unsupported model_type {kind}: BERT, DistilBERT, XLM-RoBERTa, MPNet, T5, nomic_bert and "
                   "modernbert encoders only, and Qwen2 decoder embedders (the 0.5B body) and Qwen3 decoder "
                   "embedders (the 0.6B body)")
    if kind == "qwen3":
        # a directory that names its classes must name Qwen3 ones (Qwen3Model, Qwen3ForCausalLM): another family's
        # weights under this model_type have no q_norm / k_norm and would be refused tensor by tensor much later
        archs = [str(a) for a in cfg.get("architectures") or []]
        if archs and not any(a.startswith("Qwen3") for a in archs):
            raise ValueError(f"{unsupported}; architectures {archs} is not a Qwen3 model")
        return _read_qwen3_config(path, cfg)
    if kind not in ("bert", "xlm-roberta"):
        raise ValueError(unsupported)
    if kind == "bert" and cfg.get("position_embedding_type", "absolute") == "alibi":
        return _read_alibi_config(path, cfg)
    if cfg.get("hidden_act", "gelu") != "gelu" or cfg.get("position_embedding_type", "absolute") != "absolute":
        raise ValueError("only exact-erf GELU and absolute position embeddings are implemented")
    pos_start = int(cfg.get("pad_token_id", 1)) + 1 if kind == "xlm-roberta" else 0
    max_pos = int(cfg["max_position_embeddings"]) - pos_start
    pooling, normalize, max_seq = _read_modules(path, max_pos)
    max_seq = min(max_seq, max_pos)
    cap = seq_cap()
    if kind == "xlm-roberta" and max_seq > cap:
        raise ValueError(f"{path} uses sequences of up to {max_seq} tokens; the engine runs at most {cap}: set "
                         f"max_seq_length <= {cap} in its sentence_bert_config.json, or raise {SEQ_CAP_VARIABLE} "
                         f"(up to {MAX_SEQ_LENGTH_LIMIT})")
    desc = _enc.BertDesc(layers=cfg["num_hidden_layers"], hidden=cfg["hidden_size"],
                         heads=cfg["num_attention_heads"], intermediate=cfg["intermediate_size"],
                         vocab=cfg["vocab_size"], max_pos=max_pos,
                         type_vocab=cfg.get("type_vocab_size", 2), pooling=pooling, normalize=normalize,
                         eps=cfg.get("layer_norm_eps", 1e-12),
                         # f16 (default): f16 MFMA operands, f32 accumulate, |1 - cos| < 1e-6 vs f64
                         # (north_star allows 1e-4); f16x3: (hi, lo) f16 operands, three passes,
                         # |1 - cos| ~5e-8, 1.8x slower; f32: the f32-input MFMA, 5x slower
                         precision=os.environ.get("VOITTA_ENCODER_PRECISION", "f16"))
    return {"desc": desc, "max_seq": max_seq, "pos_start": pos_start, "config": cfg}


# modules.json types (sentence_transformers.models.*) by their last component
_HEAD_MODULES = ("Dense", "LayerNorm")
_SKIPPED_MODULES = ("Transformer", "Dropout")


def _module_kind(m: dict) -> str:
    return m.get("type", "").rsplit(".", 1)[-1]


def _read_modules(path: str, max_seq: int):
    """modules.json / sentence_bert_config.json of a sentence-transformers directory -> (pooling, normalize, max_seq).
    The Dense and LayerNorm modules behind Pooling are read_head's. Normalize is the pipeline's last step here
    (vr_encoder_set_head): one that is not the last module is refused. A module of any other type is ignored, with a
    warning that names it."""
    pooling, normalize = "mean", False
    mod_path = os.path.join(path, "modules.json")
    if os.path.exists(mod_path):
        mods = json.load(open(mod_path))
        for i, m in enumerate(mods):
            k = m.get("type", "")
            if k.endswith("Pooling"):
                pc = json.load(open(os.path.join(path, m["path"], "config.json")))
                if pc.get("pooling_mode_cls_token"):
                    pooling = "cls"
                elif pc.get("pooling_mode_lasttoken"):
                    pooling = "last"
                elif not pc.get("pooling_mode_mean_tokens", True):
                    raise ValueError("only CLS and mean pooling are implemented")
            elif k.endswith("Normalize"):
                if i != len(mods) - 1:
                    raise ValueError(f"{path}: module {i} is a Normalize followed by {_module_kind(mods[i + 1])}: "
                                     "normalisation is implemented as the last module only")
                normalize = True
            elif _module_kind(m) not in _HEAD_MODULES + _SKIPPED_MODULES:
                logger.warning("%s: module %d of type %s is not implemented and is ignored: the embeddings are those of "
                               "the pipeline without it", path, i, k or "(none)")
    sb = os.path.join(path, "sentence_bert_config.json")
    if os.path.exists(sb):
        max_seq = int(json.load(open(sb)).get("max_seq_length", max_seq))
    return pooling, normalize, max_seq


def read_head(path: str, hidden: int) -> list:
    """The Dense and LayerNorm modules that follow Pooling in modules.json -> encoder.HeadStage objects in order.
    sentence_transformers.models.Dense: <module path>/config.json holds in_features, out_features, bias and
    activation_function, a dotted torch class name (Tanh and Identity are implemented, anything else is refused by
    name); the weights are linear.weight / linear.bias in <module path>/model.safetensors or pytorch_model.bin.
    sentence_transformers.models.LayerNorm: config.json holds dimension; the weights are norm.weight / norm.bias, eps
    torch's default 1e-5. Dropout does nothing at inference. One of the two in front of Pooling (a per-token
    projection) is refused. The widths must chain from `hidden`."""
    mod_path = os.path.join(path, "modules.json")
    if not os.path.exists(mod_path):
        return []
    stages, pooled, width = [], False, hidden
    for i, m in enumerate(json.load(open(mod_path))):
        kind = _module_kind(m)
        if kind == "Pooling":
            pooled = True
        if kind not in _HEAD_MODULES:
            continue
        if not pooled:
            raise ValueError(f"{path}: module {i} ({m.get('type')}) stands in front of Pooling: per-token modules are not "
                             "implemented")
        mdir = os.path.join(path, m["path"])
        mc = json.load(open(os.path.join(mdir, "config.json")))
        weights = NativeSentenceEncoder._load_weights(mdir)

        def tensor(name, shape):
            if name not in weights:
                raise KeyError(f"weight '{name}' not found under {mdir}")
            t = weights[name]
            t = np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)
            if t.shape != shape:
                raise ValueError(f"weight '{name}' under {mdir} has shape {t.shape}, its config.json implies {shape}")
            return t

        if kind == "Dense":
            n_in, n_out = int(mc["in_features"]), int(mc["out_features"])
            act = mc.get("activation_function", "torch.nn.modules.activation.Tanh")
            acts = {"Tanh": "tanh", "Identity": "identity"}
            if act.rsplit(".", 1)[-1] not in acts:
                raise ValueError(f"{mdir}: activation_function {act} is not implemented (Tanh and Identity are)")
            stage = _enc.HeadStage("dense", tensor("linear.weight", (n_out, n_in)),
                                   tensor("linear.bias", (n_out,)) if mc.get("bias", True) else None,
                                   activation=acts[act.rsplit(".", 1)[-1]])
        else:
            n_in = n_out = int(mc["dimension"])
            stage = _enc.HeadStage("layernorm", tensor("norm.weight", (n_in,)), tensor("norm.bias", (n_in,)), eps=1e-5)
        if n_in != width:
            raise ValueError(f"{mdir}: the module reads {n_in} columns, the pipeline in front of it gives {width}")
        width = n_out
        stages.append(stage)
    return stages


def _read_distilbert_config(path: str, cfg: dict) -> dict:
    """model_type distilbert (distiluse-base-multilingual-cased, msmarco-distilbert-*): BERT's post-LayerNorm body with
    exact-erf GELU, learned positions and no token types, under its own config keys (dim, n_heads, n_layers,
    hidden_dim); LayerNorm eps is 1e-12 in the model's code. The position table is read from the checkpoint whatever
    sinusoidal_pos_embds says (a sinusoidal table is stored like a learned one). encoder.distilbert_slots maps the
    weights."""
    act = cfg.get("activation", "gelu")
    if act != "gelu":
        raise ValueError(f"activation {act!r} is not implemented: a distilbert FFN runs the exact-erf GELU")
    max_pos = int(cfg["max_position_embeddings"])
    pooling, normalize, max_seq = _read_modules(path, max_pos)
    max_seq = min(max_seq, max_pos)
    cap = seq_cap()
    if max_seq > cap:
        raise ValueError(f"{path} uses sequences of up to {max_seq} tokens; the engine runs at most {cap}: set "
                         f"max_seq_length <= {cap} in its sentence_bert_config.json, or raise {SEQ_CAP_VARIABLE} "
                         f"(up to {MAX_SEQ_LENGTH_LIMIT})")
    desc = _enc.BertDesc(layers=int(cfg["n_layers"]), hidden=int(cfg["dim"]), heads=int(cfg["n_heads"]),
                         intermediate=int(cfg["hidden_dim"]), vocab=int(cfg["vocab_size"]), max_pos=max_pos, type_vocab=1,
                         pooling=pooling, normalize=normalize, eps=1e-12,
                         precision=os.environ.get("VOITTA_ENCODER_PRECISION", "f16"))
    return {"desc": desc, "max_seq": max_seq, "pos_start": 0, "config": cfg}


def _read_t5_config(path: str, cfg: dict) -> dict:
    """model_type t5 (sentence-transformers' gtr-t5-base / -large, sentence-t5-base / -large: the encoder half of T5
    v1.0): pre-norm blocks with RMSNorm (T5LayerNorm), a ReLU FFN without biases, no position in the embeddings and
    block 0's bucketed relative-position bias in every layer's attention (encoder.t5_slots / t5_bias_table). There is
    no position table, so the longest sequence is min(max_seq_length, seq_cap()): VOITTA_MAX_SEQ_LENGTH alone bounds it.
    T5 v1.1 / flan (feed_forward_proj gated-gelu) is refused: its gate is the tanh-approximate GELU."""
    ffn = cfg.get("feed_forward_proj", "relu")
    if ffn == "gated-gelu":
        raise ValueError("feed_forward_proj 'gated-gelu' (T5 v1.1, flan-t5) is not implemented: its gate is the "
                         "tanh-approximate GELU; the ReLU FFN of T5 v1.0 (gtr-t5, sentence-t5) is")
    if ffn != "relu":
        raise ValueError(f"feed_forward_proj {ffn!r} is not implemented: a t5 encoder's FFN is wo(relu(wi(x)))")
    H, heads, dkv = int(cfg["d_model"]), int(cfg["num_heads"]), int(cfg["d_kv"])
    if heads * dkv != H:
        raise ValueError(f"num_heads * d_kv = {heads} * {dkv} != d_model = {H} is not implemented: the attention's inner "
                         "width must be the model's")
    if dkv not in (32, 64):
        raise ValueError(f"d_kv {dkv} is not implemented: the attention kernels run head sizes 32 and 64")
    buckets = int(cfg.get("relative_attention_num_buckets", 32))
    max_distance = int(cfg.get("relative_attention_max_distance", 128))
    if buckets % 2 or buckets < 4:
        raise ValueError(f"relative_attention_num_buckets {buckets} is not implemented: the buckets are split in two "
                         "halves by the sign of the offset")
    if not 1 <= max_distance <= 512:
        raise ValueError(f"relative_attention_max_distance {max_distance} > 512 is not implemented: the engine's bias "
                         "table has a radius of at most 512")
    cap = seq_cap()
    pooling, normalize, max_seq = _read_modules(path, int(cfg.get("n_positions", 512)))
    if max_seq > cap:
        logger.warning("%s declares sequences of up to %d tokens; the engine runs at most %d: longer texts are "
                       "truncated to %d tokens (%s raises the cap, up to %d)", path, max_seq, cap, cap, SEQ_CAP_VARIABLE,
                       MAX_SEQ_LENGTH_LIMIT)
        max_seq = cap
    desc = _enc.BertDesc(layers=int(cfg["num_layers"]), hidden=H, heads=heads, intermediate=int(cfg["d_ff"]),
                         vocab=int(cfg["vocab_size"]), max_pos=max_seq,  # no table: the longest accepted sequence
                         type_vocab=1, pooling=pooling, normalize=normalize,
                         eps=float(cfg.get("layer_norm_epsilon", 1e-6)),
                         precision=os.environ.get("VOITTA_ENCODER_PRECISION", "f16"), position="none", ffn="relu",
                         norm="rms_pre")
    return {"desc": desc, "max_seq": max_seq, "pos_start": 0, "config": cfg, "buckets": buckets,
            "max_distance": max_distance}


def _read_qwen2_config(path: str, cfg: dict) -> dict:
    """model_type qwen2 (jina-code-embeddings-0.5b, the KaLM-embedding-mini models and other Qwen2.5-0.5B fine-tunes): a
    decoder body used as an embedder — RMSNorm pre-norm blocks, rotary positions over the whole head, a SwiGLU FFN,
    biases on q/k/v only, causal self-attention (unless the directory says is_causal false) and grouped-query attention,
    which encoder.qwen2_slots resolves at load by repeating the K and V heads (HF repeat_kv). The row is pooled as
    1_Pooling says (pooling_mode_lasttoken for these models); a bare config.json pools the mean. The longest sequence is
    min(max_seq_length, max_position_embeddings, seq_cap())."""
    H, heads = int(cfg["hidden_size"]), int(cfg["num_attention_heads"])
    kv_heads = int(cfg.get("num_key_value_heads") or heads)
    if kv_heads < 1 or heads % kv_heads:
        raise ValueError(f"num_attention_heads {heads} is not a multiple of num_key_value_heads {kv_heads}")
    if heads < 1 or H % heads or cfg.get("head_dim") not in (None, H // heads):
        raise ValueError(f"head_dim {cfg.get('head_dim')} differs from hidden_size / num_attention_heads = {H} / {heads}: a "
                         "query width other than the hidden size is not implemented")
    if H // heads not in (32, 64):
        raise ValueError(f"head size {H // heads} (hidden_size {H} / num_attention_heads {heads}) is not implemented: the "
                         "attention kernels run head sizes 32 and 64")
    if H % 128 or H > 1024:
        raise ValueError(f"hidden_size {H} is not implemented: the engine runs multiples of 128 up to 1024 (the Qwen2-0.5B "
                         "body is 896)")
    act = cfg.get("hidden_act", "silu")
    if act != "silu":
        raise ValueError(f"hidden_act {act!r} is not implemented: a qwen2 FFN is down(silu(gate(x)) * up(x))")
    rp = cfg.get("rope_parameters") or {}
    rope_type = rp.get("rope_type", rp.get("type", "default"))
    if cfg.get("rope_scaling") is not None or rope_type != "default":
        raise ValueError(f"rope_scaling {cfg.get('rope_scaling') or rope_type!r} is not implemented: only the default rotary "
                         "embedding (no scaling)")
    if cfg.get("use_sliding_window", False):
        raise ValueError("use_sliding_window true is not implemented: a causal sliding window is not in the attention "
                         "kernels")
    declared = int(cfg.get("max_position_embeddings", 32768))
    pooling, normalize, max_seq = _read_modules(path, declared)
    max_seq = min(max_seq, declared)
    cap = seq_cap()
    if max_seq > cap:
        logger.warning("%s declares sequences of up to %d tokens; the engine runs at most %d: longer texts are "
                       "truncated to %d tokens (%s raises the cap, up to %d)", path, max_seq, cap, cap, SEQ_CAP_VARIABLE,
                       MAX_SEQ_LENGTH_LIMIT)
        max_seq = cap
    desc = _enc.BertDesc(layers=int(cfg["num_hidden_layers"]), hidden=H, heads=heads,
                         intermediate=int(cfg["intermediate_size"]), vocab=int(cfg["vocab_size"]),
                         max_pos=max_seq,  # rotary: the length of the cos/sin table
                         type_vocab=1, pooling=pooling, normalize=normalize, eps=float(cfg.get("rms_norm_eps", 1e-6)),
                         precision=os.environ.get("VOITTA_ENCODER_PRECISION", "f16"), position="rotary",
                         rope_theta=float(rp.get("rope_theta", cfg.get("rope_theta", 10000.0))), ffn="swiglu",
                         norm="rms_pre_rotary", causal=0 if cfg.get("is_causal", True) is False else 1)
    return {"desc": desc, "max_seq": max_seq, "pos_start": 0, "config": cfg, "kv_heads": kv_heads}


def _read_qwen3_config(path: str, cfg: dict) -> dict:
    """model_type qwen3 (Qwen3-Embedding-0.6B and its fine-tunes): the Qwen2 body with a head size of its own — head_dim,
    128 for the 0.6B body, so that q_proj is hidden -> heads * head_dim and o_proj the way back — and an RMSNorm over
    every head of the query and of the key ahead of the rotation (q_norm / k_norm, [head_dim], shared by the heads).
    attention_bias (false for these models) says whether q/k/v carry biases. Grouped-query attention is resolved at load
    (encoder.qwen3_slots), pooling, causality and the longest sequence are read as for qwen2."""
    H, heads = int(cfg["hidden_size"]), int(cfg["num_attention_heads"])
    kv_heads = int(cfg.get("num_key_value_heads") or heads)
    if heads < 1 or kv_heads < 1 or heads % kv_heads:
        raise ValueError(f"num_attention_heads {heads} is not a multiple of num_key_value_heads {kv_heads}")
    head_dim = int(cfg["head_dim"]) if cfg.get("head_dim") is not None else (H // heads if H % heads == 0 else 0)
    if head_dim not in (32, 64, 128):
        raise ValueError(f"head_dim {head_dim} is not implemented: the attention kernels run head sizes 32, 64 and 128")
    if heads * head_dim > 2048 or (heads * head_dim) % 128:
        raise ValueError(f"num_attention_heads {heads} x head_dim {head_dim} = {heads * head_dim} is not implemented: the "
                         "attention width must be a multiple of 128 and at most 2048")
    if H % 128 or H > 1024:
        raise ValueError(f"hidden_size {H} is not implemented: the engine runs multiples of 128 up to 1024 (the "
                         "Qwen3-Embedding-0.6B body is 1024)")
    act = cfg.get("hidden_act", "silu")
    if act != "silu":
        raise ValueError(f"hidden_act {act!r} is not implemented: a qwen3 FFN is down(silu(gate(x)) * up(x))")
    rp = cfg.get("rope_parameters") or {}
    rope_type = rp.get("rope_type", rp.get("type", "default"))
    if cfg.get("rope_scaling") is not None or rope_type != "default":
        raise ValueError(f"rope_scaling {cfg.get('rope_scaling') or rope_type!r} is not implemented: only the default rotary "
                         "embedding (no scaling)")
    if cfg.get("use_sliding_window", False):
        raise ValueError("use_sliding_window true is not implemented: a causal sliding window is not in the attention "
                         "kernels")
    declared = int(cfg.get("max_position_embeddings", 32768))
    pooling, normalize, max_seq = _read_modules(path, declared)
    max_seq = min(max_seq, declared)
    cap = seq_cap()
    if max_seq > cap:
        logger.warning("%s declares sequences of up to %d tokens; the engine runs at most %d: longer texts are "
                       "truncated to %d tokens (%s raises the cap, up to %d)", path, max_seq, cap, cap, SEQ_CAP_VARIABLE,
                       MAX_SEQ_LENGTH_LIMIT)
        max_seq = cap
    desc = _enc.BertDesc(layers=int(cfg["num_hidden_layers"]), hidden=H, heads=heads,
                         intermediate=int(cfg["intermediate_size"]), vocab=int(cfg["vocab_size"]),
                         max_pos=max_seq,  # rotary: the length of the cos/sin table
                         type_vocab=1, pooling=pooling, normalize=normalize, eps=float(cfg.get("rms_norm_eps", 1e-6)),
                         precision=os.environ.get("VOITTA_ENCODER_PRECISION", "f16"), position="rotary",
                         rope_theta=float(rp.get("rope_theta", cfg.get("rope_theta", 10000.0))), ffn="swiglu",
                         norm="rms_pre_rotary", causal=0 if cfg.get("is_causal", True) is False else 1,
                         head_dim=head_dim, qk_norm=1)
    return {"desc": desc, "max_seq": max_seq, "pos_start": 0, "config": cfg, "kv_heads": kv_heads,
            "attention_bias": bool(cfg.get("attention_bias", False))}


def _read_mpnet_config(path: str, cfg: dict) -> dict:
    """model_type mpnet (all-mpnet-base-v2, multi-qa-mpnet-*, paraphrase-mpnet-*): a post-LayerNorm BERT with exact-erf
    GELU, no token types, learned positions from row padding_idx + 1 = 2 on (as XLM-R's), and one relative-position
    attention bias shared by all layers — encoder.mpnet_slots turns its bucket table into the engine's offset table."""
    act = cfg.get("hidden_act", "gelu")
    if act != "gelu":
        raise ValueError(f"hidden_act {act!r} is not implemented: an mpnet FFN runs the exact-erf GELU")
    buckets = int(cfg.get("relative_attention_num_buckets", 32))
    if buckets % 2:
        raise ValueError(f"relative_attention_num_buckets {buckets} is not implemented: the buckets are split in two "
                         "halves by the sign of the offset")
    if buckets != 32:
        raise ValueError(f"relative_attention_num_buckets {buckets} is not implemented: transformers' MPNetEncoder computes "
                         "its buckets for 32 whatever this says, and so would not use such a table as it was trained")
    pos_start = 2  # MPNetEmbeddings.padding_idx + 1, fixed in the model's code
    max_pos = int(cfg["max_position_embeddings"]) - pos_start
    pooling, normalize, max_seq = _read_modules(path, max_pos)
    max_seq = min(max_seq, max_pos)
    cap = seq_cap()
    if max_seq > cap:
        raise ValueError(f"{path} uses sequences of up to {max_seq} tokens; the engine runs at most {cap}: set "
                         f"max_seq_length <= {cap} in its sentence_bert_config.json, or raise {SEQ_CAP_VARIABLE} "
                         f"(up to {MAX_SEQ_LENGTH_LIMIT})")
    desc = _enc.BertDesc(layers=cfg["num_hidden_layers"], hidden=cfg["hidden_size"], heads=cfg["num_attention_heads"],
                         intermediate=cfg["intermediate_size"], vocab=cfg["vocab_size"], max_pos=max_pos, type_vocab=1,
                         pooling=pooling, normalize=normalize, eps=cfg.get("layer_norm_eps", 1e-5),
                         precision=os.environ.get("VOITTA_ENCODER_PRECISION", "f16"))
    return {"desc": desc, "max_seq": max_seq, "pos_start": pos_start, "config": cfg}


def _read_alibi_config(path: str, cfg: dict) -> dict:
    """model_type bert with position_embedding_type alibi (jina-embeddings-v2-small-en / -base-en, JinaBert): a
    post-LayerNorm BERT without any position in its embeddings, a GeGLU FFN, and a linear attention bias of
    -slope_h |key - query| per head (encoder.alibi_slopes), which is what lets it run past its training length.
    Sequences are capped at seq_cap() (these checkpoints declare 8192): truncation is well defined without a table.
    The variant with LayerNorms on Q and K (-code, -de, -es, -zh) has the same config; encoder.jina_slots refuses its
    weights by name."""
    ffn = cfg.get("feed_forward_type", "original")
    if ffn != "geglu":
        raise ValueError(f"feed_forward_type {ffn!r} is not implemented: an alibi encoder's FFN is the gated 'geglu'")
    act = cfg.get("hidden_act", "gelu")
    if act != "gelu":
        raise ValueError(f"hidden_act {act!r} is not implemented: the gate of an alibi encoder's FFN is the exact-erf GELU")
    heads = int(cfg["num_attention_heads"])
    declared = int(cfg.get("max_position_embeddings", 8192))
    pooling, normalize, max_seq = _read_modules(path, declared)
    max_seq = min(max_seq, declared)
    cap = seq_cap()
    if max_seq > cap:
        logger.warning("%s declares sequences of up to %d tokens; the engine runs at most %d: longer texts are "
                       "truncated to %d tokens (%s raises the cap, up to %d)", path, max_seq, cap, cap, SEQ_CAP_VARIABLE,
                       MAX_SEQ_LENGTH_LIMIT)
        max_seq = cap
    desc = _enc.BertDesc(layers=cfg["num_hidden_layers"], hidden=cfg["hidden_size"], heads=heads,
                         intermediate=cfg["intermediate_size"], vocab=cfg["vocab_size"],
                         max_pos=max_seq,  # no table: the longest accepted sequence
                         type_vocab=cfg.get("type_vocab_size", 2), pooling=pooling, normalize=normalize,
                         eps=cfg.get("layer_norm_eps", 1e-12),
                         precision=os.environ.get("VOITTA_ENCODER_PRECISION", "f16"), position="none", ffn="geglu",
                         attention_slopes=_enc.alibi_slopes(heads))
    return {"desc": desc, "max_seq": max_seq, "pos_start": 0, "config": cfg}


def _read_rope_config(path: str, cfg: dict) -> dict:
    """model_type nomic_bert in the native transformers layout (NomicBertConfig's keys): a post-LayerNorm BERT with
    rotary positions over the whole head (rotate-half pairing) and a gated FFN without biases. Sequences are capped at
    seq_cap() (these checkpoints declare 2048-8192): truncation is well defined without a learned table."""
    if "hidden_size" not in cfg:
        raise ValueError(f"{path}: model_type nomic_bert without 'hidden_size' — the hub checkpoint's older config "
                         "spelling (n_embd, n_head, rotary_emb_base, ...) is not read; re-save the config in the "
                         "native transformers layout (NomicBertConfig)")
    H, heads = int(cfg["hidden_size"]), int(cfg["num_attention_heads"])
    rp = cfg.get("rope_parameters") or {}
    rope_type = rp.get("rope_type", rp.get("type", "default"))
    if rope_type != "default":
        raise ValueError(f"rope_type {rope_type!r}: only the default rotary embedding is implemented (no scaling)")
    if float(rp.get("partial_rotary_factor", cfg.get("rotary_emb_fraction", 1.0))) != 1.0:
        raise ValueError("partial rotary embeddings are not implemented: the whole head must be rotated")
    if cfg.get("rotary_emb_interleaved", False):
        raise ValueError("interleaved rotary embeddings are not implemented (rotate-half pairing only)")
    if cfg.get("head_dim") not in (None, H // heads):
        raise ValueError(f"head_dim {cfg['head_dim']} differs from hidden_size / num_attention_heads = {H // heads}")
    if cfg.get("prenorm", False):
        raise ValueError("pre-norm encoders are not implemented (post-LayerNorm residual blocks only)")
    act = cfg.get("hidden_act", "silu")
    if act not in ("silu", "gelu"):
        raise ValueError(f"hidden_act {act!r}: the gated FFN runs SiLU (SwiGLU) or exact-erf GELU (GeGLU)")
    declared = int(cfg.get("max_position_embeddings", 2048))
    pooling, normalize, max_seq = _read_modules(path, declared)
    max_seq = min(max_seq, declared)
    cap = seq_cap()
    if max_seq > cap:
        logger.warning("%s declares sequences of up to %d tokens; the engine runs at most %d: longer texts are "
                       "truncated to %d tokens (%s raises the cap, up to %d)", path, max_seq, cap, cap, SEQ_CAP_VARIABLE,
                       MAX_SEQ_LENGTH_LIMIT)
        max_seq = cap
    desc = _enc.BertDesc(layers=cfg["num_hidden_layers"], hidden=H, heads=heads, intermediate=cfg["intermediate_size"],
                         vocab=cfg["vocab_size"], max_pos=max_seq,  # rotary: the length of the cos/sin table
                         type_vocab=cfg.get("type_vocab_size", 2), pooling=pooling, normalize=normalize,
                         eps=cfg.get("layer_norm_eps", 1e-12),
                         precision=os.environ.get("VOITTA_ENCODER_PRECISION", "f16"), position="rotary",
                         rope_theta=float(rp.get("rope_theta", 1000.0)), ffn="swiglu" if act == "silu" else "geglu")
    return {"desc": desc, "max_seq": max_seq, "pos_start": 0, "config": cfg}


def _read_modernbert_config(path: str, cfg: dict) -> dict:
    """model_type modernbert (transformers' ModernBertConfig, in the spelling of transformers 5 — rope_parameters per
    attention kind, layer_types — or the older one — global_rope_theta / local_rope_theta): a pre-norm encoder with
    rotary positions, GeGLU, and sliding-window attention in every layer that is not a multiple of
    global_attn_every_n_layers. Query i of a windowed layer sees key j iff |i - j| <= local_attention // 2. Sequences
    are capped at seq_cap() as for nomic_bert."""
    H, heads, L = int(cfg["hidden_size"]), int(cfg["num_attention_heads"]), int(cfg["num_hidden_layers"])
    act = cfg.get("hidden_activation", "gelu")
    if act != "gelu":
        raise ValueError(f"hidden_activation {act!r} is not implemented: a modernbert gate is the exact-erf GELU (GeGLU)")
    if cfg.get("head_dim") not in (None, H // heads):
        raise ValueError(f"head_dim {cfg['head_dim']} differs from hidden_size / num_attention_heads = {H // heads}: "
                         "not implemented")
    rp = cfg.get("rope_parameters") or {}
    kinds = {"full_attention": ("global_rope_theta", 160000.0), "sliding_attention": ("local_rope_theta", 10000.0)}
    theta = {}
    for name, (old_key, default) in kinds.items():
        part = rp.get(name) or {}
        rope_type = part.get("rope_type", part.get("type", "default"))
        if rope_type != "default" or cfg.get("rope_scaling"):
            raise ValueError(f"rope type {rope_type!r} ({name}) is not implemented: only the default rotary embedding "
                             "(no rope scaling)")
        value = part.get("rope_theta", cfg.get(old_key, default))
        theta[name] = None if value is None else float(value)
    if theta["full_attention"] is None:
        raise ValueError("global_rope_theta null is not implemented: the global layers need a rotary base")
    if theta["sliding_attention"] is None:  # transformers: a null local_rope_theta means the global layers' base
        theta["sliding_attention"] = theta["full_attention"]
    every = int(cfg.get("global_attn_every_n_layers", 3))
    if every < 1:
        raise ValueError(f"global_attn_every_n_layers {every} must be >= 1")
    pattern = ["full_attention" if i % every == 0 else "sliding_attention" for i in range(L)]
    if cfg.get("layer_types") is not None and list(cfg["layer_types"]) != pattern:
        raise ValueError("layer_types that are not 'every global_attn_every_n_layers-th layer is full_attention' are "
                         f"not implemented (got {list(cfg['layer_types'])}, global_attn_every_n_layers = {every})")
    window = int(cfg.get("local_attention", 128)) // 2
    if not 0 <= window <= 4096:
        raise ValueError(f"local_attention {cfg.get('local_attention')}: the engine's window half-width is 0..4096")
    windowed = window > 0 and "sliding_attention" in pattern
    declared = int(cfg.get("max_position_embeddings", 8192))
    pooling, normalize, max_seq = _read_modules(path, declared)
    max_seq = min(max_seq, declared)
    cap = seq_cap()
    if max_seq > cap:
        logger.warning("%s declares sequences of up to %d tokens; the engine runs at most %d: longer texts are "
                       "truncated to %d tokens (%s raises the cap, up to %d)", path, max_seq, cap, cap, SEQ_CAP_VARIABLE,
                       MAX_SEQ_LENGTH_LIMIT)
        max_seq = cap
    desc = _enc.BertDesc(layers=L, hidden=H, heads=heads, intermediate=int(cfg["intermediate_size"]),
                         vocab=int(cfg["vocab_size"]), max_pos=max_seq, type_vocab=1, pooling=pooling, normalize=normalize,
                         eps=float(cfg.get("norm_eps", 1e-5)), precision=os.environ.get("VOITTA_ENCODER_PRECISION", "f16"),
                         position="rotary", rope_theta=theta["full_attention"], ffn="geglu", norm="pre",
                         window=window if windowed else 0, global_every=every if windowed else 0,
                         rope_theta_local=theta["sliding_attention"] if windowed else 0.0)
    return {"desc": desc, "max_seq": max_seq, "pos_start": 0, "config": cfg}


def slice_positions(state: dict, pos_start: int) -> dict:
    """The state dict with its position table from row pos_start on (XLM-R's rows for positions 0, 1, ...)."""
    if not pos_start:
        return state
    key = "embeddings.position_embeddings.weight"
    hits = [k for k in state if k == key or k.endswith("." + key)]
    if len(hits) != 1:
        raise KeyError(f"weight '{key}' not found (or ambiguous) in state dict: {hits[:3]}")
    out = dict(state)
    out[hits[0]] = state[hits[0]][pos_start:]
    return out


class NativeSentenceEncoder:
    """The object behind ``EmbeddingService.model``: ``encode(texts)`` like SentenceTransformer's."""

    def __init__(self, engine, desc: _enc.BertDesc, state: dict, tokenizer, max_seq_length: int):
        self.engine = engine
        self.tokenizer = tokenizer
        self.max_seq_length = min(max_seq_length, desc.max_pos)
        if native_tokenizer(tokenizer):
            tokenizer.max_length = self.max_seq_length
        else:
            self.tokenizer.no_padding()
            self.tokenizer.enable_truncation(max_length=self.max_seq_length)
        _enc.load_encoder(engine, desc, state)
        if get_settings().late_chunking and desc.pooling == "cls":
            logger.warning("VOITTA_LATE_CHUNKING=1 with a checkpoint that pools [CLS]: late-chunked vectors are means "
                           "over a chunk's tokens, which this model was not trained to produce; it runs all the same")

    @property
    def desc(self) -> _enc.BertDesc:
        """The loaded encoder's description as the engine holds it: Engine.set_encoder_head replaces it there, and the
        widths read from it here (empty results, deferred embeddings, the one-call text paths) follow."""
        return self.engine.encoder_desc

    @property
    def leading_specials(self) -> int:
        """The specials in front of a tokenised text: 1 (<s>, [CLS]) — 0 for a T5 tokenizer, whose template is $A </s>."""
        return 0 if getattr(self.tokenizer, "bos_id", 0) == -1 else 1

    # ---- loading ---------------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, path: str, engine=None) -> "NativeSentenceEncoder":
        if not os.path.isdir(path):
            raise FileNotFoundError(
                f"EMBEDDING_MODEL='{path}' is not a local checkpoint directory (hub names cannot be "
                "downloaded here: there is no network). Point it at a sentence-transformers / HF BERT directory.")
        rc = read_encoder_config(path)
        if rc["config"].get("model_type") == "mpnet":
            state, rc["desc"].attention_bias = _enc.mpnet_slots(cls._load_weights(path), rc["desc"], rc["pos_start"])
        elif rc["config"].get("model_type") == "distilbert":
            state = _enc.distilbert_slots(cls._load_weights(path), rc["desc"])
        elif rc["config"].get("model_type") == "t5":
            state = cls._load_weights(path)
            if not any(k.endswith("encoder.block.0.layer.0.SelfAttention.q.weight") for k in state):
                raise ValueError(f"{path}: model_type t5 (is_encoder_decoder {rc['config'].get('is_encoder_decoder')}) "
                                 "without encoder weights (encoder.block.*): only the encoder half is run")
            # (load_encoder's t5_slots maps the weights; the table needs the config's bucket count and distance)
            rc["desc"].attention_bias = _enc.t5_bias_table(
                _enc._find(state, "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"),
                rc["buckets"], rc["max_distance"])
        elif rc["config"].get("model_type") in ("qwen2", "qwen3"):
            state = cls._load_weights(path)  # (load_encoder's qwen2_slots / qwen3_slots maps the weights and repeats the K/V heads)
        else:
            state = slice_positions(cls._load_weights(path), rc["pos_start"])
        return cls(engine or get_engine(), rc["desc"], state, cls._load_tokenizer(path, rc["config"]), rc["max_seq"])

    @staticmethod
    def _load_weights(path: str) -> dict:
        st = os.path.join(path, "model.safetensors")
        if os.path.exists(st):
            from safetensors.torch import load_file

            return load_file(st)
        pt = os.path.join(path, "pytorch_model.bin")
        if os.path.exists(pt):
            import torch

            return torch.load(pt, map_location="cpu", weights_only=True)
        raise FileNotFoundError(f"no model.safetensors / pytorch_model.bin under {path}")

    @staticmethod
    def _load_tokenizer(path: str, cfg: dict):
        """The native WordPiece (csrc/wordpiece.cpp) for plain BERT tokenizers (an MPNet model's among them: the same
        pipeline wrapped in <s> ... </s>, the names read from tokenizer.json's post_processor), the native Unigram
        (csrc/unigram.cpp)
        for the XLM-R pipeline of an XLM-R model and the same pipeline with the template $A </s> of a T5 model, the
        native byte-level BPE (csrc/bpe.cpp) for a ModernBERT, Qwen2 or Qwen3 model's pipeline where it accepts it (Qwen's own
        pre-tokenizer pattern it refuses); anything else that a tokenizer.json may describe (a BERT model with a Unigram tokenizer.json among
        them, as before) goes through the HF `tokenizers` library."""
        tj = os.path.join(path, "tokenizer.json")
        if os.path.exists(tj) and cfg.get("model_type") in ("xlm-roberta", "t5"):
            spec = json.load(open(tj, encoding="utf-8"))
            if (spec.get("model") or {}).get("type") == "Unigram":
                if is_unigram_pipeline(spec):
                    return UnigramTokenizer.from_tokenizer_json(spec)
                logger.info("native Unigram not applicable; using the tokenizers library")
        if os.path.exists(tj) and cfg.get("model_type") in ("modernbert", "qwen2", "qwen3"):
            spec = json.load(open(tj, encoding="utf-8"))
            if (spec.get("model") or {}).get("type") == "BPE":
                try:
                    return BpeTokenizer.from_tokenizer_json(spec)
                except (ValueError, KeyError, TypeError) as e:
                    logger.info("native byte-level BPE not applicable (%s); using the tokenizers library", e)
        if os.path.exists(os.path.join(path, "vocab.txt")) or os.path.exists(tj):
            try:
                if os.path.exists(tj):
                    spec = json.load(open(tj, encoding="utf-8"))
                    plain = (spec["model"]["type"] == "WordPiece"
                             and (spec.get("normalizer") or {}).get("type") == "BertNormalizer"
                             and (spec.get("pre_tokenizer") or {}).get("type") == "BertPreTokenizer"
                             and spec["model"].get("continuing_subword_prefix", "##") == "##"
                             and spec["model"].get("max_input_chars_per_word", 100) == 100)
                    if not plain:
                        raise ValueError("not a plain BERT WordPiece pipeline")
                    # the wrapper is part of the pipeline: WordPieceTokenizer reads the specials' names from the
                    # post_processor and refuses one that is not <cls> $A <sep>. An MPNet model needs them found
                    # (<s> ... </s>): without a post_processor there the [CLS] ... [SEP] default would be wrong ids
                    if cfg.get("model_type") == "mpnet" and spec.get("post_processor") is None:
                        raise ValueError("an MPNet tokenizer.json without a post_processor names no specials")
                elif cfg.get("model_type") == "mpnet":
                    raise ValueError("an MPNet vocab.txt alone names no specials")
                return WordPieceTokenizer.from_pretrained(path)
            except (ValueError, KeyError) as e:
                logger.info("native WordPiece not applicable (%s); using the tokenizers library", e)
        from tokenizers import Tokenizer

        if os.path.exists(tj):
            return Tokenizer.from_file(tj)
        vocab = os.path.join(path, "vocab.txt")
        if not os.path.exists(vocab):
            raise FileNotFoundError(f"no tokenizer.json / vocab.txt under {path}")
        lower = True
        tc = os.path.join(path, "tokenizer_config.json")
        if os.path.exists(tc):
            lower = bool(json.load(open(tc)).get("do_lower_case", True))
        return build_wordpiece_tokenizer([l.rstrip("\n") for l in open(vocab, encoding="utf-8")], lower)

    # ---- SentenceTransformer.encode -------------------------------------------------------------
    def tokenize(self, texts: list[str]):
        if native_tokenizer(self.tokenizer):
            ids, off = self.tokenizer.encode_batch(list(texts))
            return ids, off.astype(np.int32)
        encs = self.tokenizer.encode_batch(list(texts))
        lens = [len(e.ids) for e in encs]
        off = np.zeros(len(texts) + 1, np.int32)
        off[1:] = np.cumsum(lens)
        ids = np.fromiter((t for e in encs for t in e.ids), dtype=np.int32, count=int(off[-1]))
        return ids, off

    def encode(self, sentences, batch_size: int = 32, convert_to_numpy: bool = True,
               show_progress_bar: bool = False, **_ignored):
        """str -> (D,) array, list[str] -> (n, D) array. batch_size shaped only the padding of the
        reference's batches; the packed GPU layout has none, so it is accepted and ignored."""
        single = isinstance(sentences, str)
        texts = [sentences] if single else list(sentences)
        if not texts:
            return np.zeros((0, self.desc.out_dim), np.float32)
        ids, off = self.tokenize(texts)
        out = _enc.encode(self.engine, ids, off)
        return out[0] if single else out

    # ---- late chunking -----------------------------------------------------------------------------
    def plan_documents(self, documents, prefix: str = "") -> _late.Plan:
        """The late-chunking plan (late_chunking.plan_many) of [(document, chunk_texts), ...] for this model: windows of
        max_seq_length tokens, VOITTA_LATE_CHUNKING_CONTEXT tokens of left context, ``prefix`` (the passage prefix) as
        ids in front of every window. A document that cannot be late-chunked goes the plain way inside the plan."""
        lead = self.leading_specials
        return _late.plan_many(documents, self.tokenize, self.max_seq_length, get_settings().late_chunking_context,
                               _late.prefix_ids_of(prefix, self.tokenize, lead), plain_text=lambda t: prefix + t,
                               pooling=self.desc.pooling, lead=lead)

    def encode_documents(self, documents, prefix: str = ""):
        """[(document, chunk_texts), ...] -> (total chunks, D): every chunk embedded in the context of its document,
        ONE engine call (vr_encode_spans) for all of them."""
        plan = self.plan_documents(documents, prefix)
        if plan.n_chunks == 0:
            return np.zeros((0, self.desc.out_dim), np.float32)
        return _enc.encode_spans(self.engine, plan.ids, plan.offsets, plan.span_off, plan.span_tok)

    def encode_document(self, document: str, chunk_texts, prefix: str = ""):
        """(n, D): the vectors of one document's chunks, each the mean of its own tokens' final hidden states after
        the whole document (or its window of it) went through the encoder."""
        return self.encode_documents([(document, chunk_texts)], prefix)


def build_wordpiece_tokenizer(vocab: list[str], lowercase: bool = True):
    """BertTokenizerFast equivalent from a vocab.txt: BertNormalizer + BertPreTokenizer + WordPiece
    ('##', 100-char word limit) + '[CLS] $A [SEP]' post-processing."""
    from tokenizers import Tokenizer, models, normalizers, pre_tokenizers, processors

    v = {t: i for i, t in enumerate(vocab)}
    tok = Tokenizer(models.WordPiece(v, unk_token="[UNK]", max_input_chars_per_word=100))
    tok.normalizer = normalizers.BertNormalizer(clean_text=True, handle_chinese_chars=True, strip_accents=None,
                                                lowercase=lowercase)
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    tok.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]",
                                                       special_tokens=[("[CLS]", v["[CLS]"]), ("[SEP]", v["[SEP]"])])
    return tok


class EmbeddingService:
    """Service for generating text embeddings on the GPU (reference: embedding.py:14-86)."""

    def __init__(self, model_name: str | None = None):
        settings = get_settings()
        self.model_name = model_name or settings.embedding_model
        self.dimension = settings.embedding_dimension  # taken from settings, not the model (embedding.py:20)
        self._model: NativeSentenceEncoder | None = None

    @property
    def model(self) -> NativeSentenceEncoder:
        """Lazy load the model (embedding.py:23-42)."""
        if self._model is None:
            settings = get_settings()
            logger.info(f"Loading embedding model: {self.model_name}")
            device_setting = settings.embedding_device.lower()
            if device_setting == "cpu":
                raise RuntimeError("EMBEDDING_DEVICE=cpu: the native embedding service has no CPU path "
                                   "(use the reference's sentence-transformers service instead)")
            self._model = NativeSentenceEncoder.from_pretrained(self.model_name)
            logger.info("Model loaded successfully on the MI355X engine")
        return self._model

    # Task prefixes. The reference knows the e5 rule only (model name contains "e5"); models that expect other
    # prefixes (nomic: "search_document: " / "search_query: ") are served by the opt-in VOITTA_EMBED_PASSAGE_PREFIX /
    # VOITTA_EMBED_QUERY_PREFIX, applied in front of the (possibly e5-prefixed) text. Empty by default: nothing changes.
    def _passage(self, text: str) -> str:
        if "e5" in self.model_name.lower():  # embedding.py:50-51, 65-66
            text = f"passage: {text}"
        prefix = get_settings().embed_passage_prefix
        return prefix + text if prefix else text

    def _query(self, text: str) -> str:
        if "e5" in self.model_name.lower():  # embedding.py:82-83
            text = f"query: {text}"
        prefix = get_settings().embed_query_prefix
        return prefix + text if prefix else text

    def embed_text(self, text: str) -> list[float]:
        text = self._passage(text)
        return self.model.encode(text, convert_to_numpy=True).tolist()

    def embed_document(self, document: str, chunk_texts: list[str]) -> list[list[float]]:
        """The vectors of one document's chunks, late-chunked: see NativeSentenceEncoder.encode_document."""
        return self.embed_documents([(document, chunk_texts)])

    def embed_documents(self, documents) -> list[list[float]]:
        """embed_document for [(document, chunk_texts), ...] in one engine call; the rows in chunk order."""
        return self.model.encode_documents(documents, self._passage("")).tolist()

    def chunk_and_embed_documents(self, texts: list[str], chunker=None) -> list:
        """Semantic chunking: per document ``(chunks, vectors)`` — its chunks (``chunking.Chunk``, the
        texts ``SemanticChunkText`` that carry the vectors) and their late-chunked rows (n, D) f32 — from ONE forward pass
        over all the documents (vr_encode_semantic): units by the native ``sentence`` strategy, boundaries where
        neighbouring units stop resembling each other, by the VOITTA_SEMANTIC_* settings. A document that cannot be
        planned (semantic_chunking.plan_units) is cut by ``chunker`` (default: the configured ChunkingService) and
        embedded the plain way."""
        from .chunking import Chunk, ChunkingService

        s = get_settings()
        texts = [t or "" for t in texts]
        if not texts:
            return []
        splitter = ChunkingService(chunk_size=s.semantic_unit_chars, strategy="sentence")
        splitter.chunk_overlap = 0  # (the constructor reads 0 as "the setting's")
        units = [[str(c.text) for c in own] for own in splitter.cut(texts)]
        model = self.model
        lead = model.leading_specials
        prefix = self._passage("")
        up = _semantic.plan_units(list(zip(texts, units)), model.tokenize, model.max_seq_length, s.late_chunking_context,
                                  _late.prefix_ids_of(prefix, model.tokenize, lead), lead)
        out: list = [None] * len(texts)
        if up.plan.n_chunks:
            p = up.plan
            rows, start, _ = _enc.encode_semantic(model.engine, p.ids, p.offsets, p.span_off, p.span_tok,
                                                  buffer=s.semantic_buffer, break_permille=s.semantic_break_permille,
                                                  min_distance=s.semantic_min_distance, min_tokens=s.semantic_min_tokens,
                                                  max_tokens=s.semantic_max_tokens)
            u0 = r0 = 0
            for k, where in zip(up.planned, up.where):
                own = start[u0:u0 + len(where)]
                pieces = _semantic.rebuild(texts[k], where, own)
                vectors = rows[r0:r0 + len(pieces)]
                wrapped = _semantic.wrap_chunks([t for t, _, _ in pieces], vectors)
                out[k] = ([Chunk(w, i, a, b) for i, (w, (_, a, b)) in enumerate(zip(wrapped, pieces))], vectors)
                u0, r0 = u0 + len(where), r0 + len(pieces)
            assert r0 == len(rows) and u0 == len(start)
        if up.plain:
            cutter = chunker or ChunkingService()
            for k, chunks in zip(up.plain, cutter.cut([texts[k] for k in up.plain])):
                plain = [str(c.text) for c in chunks]
                vectors = (model.encode([self._passage(t) for t in plain]) if plain
                           else np.zeros((0, model.desc.out_dim), np.float32))
                wrapped = _semantic.wrap_chunks(plain, vectors)
                out[k] = ([Chunk(w, c.index, c.start_char, c.end_char) for w, c in zip(wrapped, chunks)], vectors)
        return out

    def embed_texts(self, texts: list[str], batch_size: int = 32) -> list[list[float]]:
        if not texts:
            return []
        if get_settings().semantic_chunking:
            # chunk texts that ChunkingService returned under the flag (SemanticChunkText), whole documents of them in
            # order: their vectors came out of the pass that chose their boundaries and travel with them
            carried = _semantic.carried_vectors(texts)
            if carried is not None:
                return carried.tolist()
        if get_settings().late_chunking:
            # chunk texts that ChunkingService cut (LateChunkText), whole documents of them in order: embedded in the
            # context of their documents, plain floats at once (no deferred references in this mode)
            documents = _late.group_documents(texts)
            if documents is not None:
                return self.embed_documents(documents)
        texts = [self._passage(text) for text in texts]
        if _deferred.enabled():
            # tokenised now, encoded when somebody looks at a number — or, when the list goes to store_chunks
            # untouched, together with thousands of other chunks inside the engine (voitta_rag_amd/deferred.py)
            return _deferred.DeferredEmbeddings(self.model, *self.model.tokenize(list(texts)))
        embeddings = self.model.encode(texts, batch_size=batch_size, convert_to_numpy=True,
                                       show_progress_bar=len(texts) > 100)
        return embeddings.tolist()

    def embed_query(self, query: str) -> list[float]:
        question = query
        query = self._query(query)
        model = self.model
        if _deferred.enabled() and one_call_text_paths(model):
            out = _deferred.QueryRef(model, query)  # encoded when looked at — or inside the search call it goes to
        else:
            out = _deferred.QueryEmbedding(model.encode(query, convert_to_numpy=True))
        out.question = question  # the raw question, for a reranking search
        return out

    def query_texts(self, queries: list[str]) -> list[str]:
        """The questions as the encoder sees them: with the e5 ``query: `` prefix (and the opt-in query prefix), as
        embed_query applies them."""
        return [self._query(q) for q in queries]

    def embed_queries(self, queries: list[str]) -> list[list[float]]:
        """embed_query for many questions in ONE forward pass (the packed batch of vr_encode)."""
        if not queries:
            return []
        return self.model.encode(self.query_texts(queries), convert_to_numpy=True).tolist()


_embedding_service: EmbeddingService | None = None


def get_embedding_service() -> EmbeddingService:
    global _embedding_service
    if _embedding_service is None:
        _embedding_service = EmbeddingService()
    return _embedding_service
