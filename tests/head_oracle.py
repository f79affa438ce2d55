"""NumPy f64 oracle of the post-pooling head (vr_encoder_set_head) and the cases its tests share.

A head is what a sentence-transformers pipeline runs behind Pooling: Dense (y = act(W x + b), act identity or tanh) and
LayerNorm ((x - mean) / sqrt(var + eps) * g + b, biased variance) modules in order, then Normalize (x / max(|x|, 1e-12)
over the WHOLE last width) and SentenceTransformer(truncate_dim=...): the leading columns, not normalised again. It is
applied to UN-normalised pooled rows, which the existing oracles give with normalize=False.

Head weights are drawn W ~ N(0, 1 / in_dim), b ~ N(0, 0.1): a pooled row of these encoders has elements of order 1, so
the pre-activations are of order 1 as well — tanh works on its curved part and no case owes its accuracy to a vanishing
or a saturated output. tests/test_head_cpu.py::test_reference_arithmetic_clears_the_gpu_bar checks that f32 reference
arithmetic on these cases clears the bar the GPU tests use with a tenfold margin."""
import json
import os
from dataclasses import dataclass, field

import numpy as np

from oracle import bert as obert

LENS = [1, 2, 15, 16, 17, 64, 129]
TINY = obert.BertShape(2, 128, 2, 256, vocab=500, max_pos=160)
WIDE = obert.BertShape(1, 1024, 16, 128, vocab=300, max_pos=160)


@dataclass
class HeadCase:
    shape: obert.BertShape
    pooling: str
    normalize: bool
    # (kind, in_dim, out_dim, activation, bias)
    stages: list = field(default_factory=list)
    truncate: int = 0
    seed: int = 0

    @property
    def out_dim(self) -> int:
        if self.truncate:
            return self.truncate
        return self.stages[-1][2] if self.stages else self.shape.hidden


CASES = {
    "labse": HeadCase(TINY, "cls", True, [("dense", 128, 128, "tanh", True)], seed=11),
    "distiluse": HeadCase(TINY, "mean", False, [("dense", 128, 64, "tanh", True)], seed=12),
    # 48 columns: three 16-column tiles, so one of the kernel's four waves has none and the count is no multiple of 4
    "two": HeadCase(TINY, "mean", True, [("dense", 128, 256, "identity", False), ("dense", 256, 48, "identity", True)], seed=13),
    "ln_trunc": HeadCase(TINY, "mean", True, [("layernorm", 128, 128, "identity", True)], truncate=32, seed=14),
    "trunc": HeadCase(TINY, "mean", True, [], truncate=16, seed=15),
    "wide": HeadCase(WIDE, "mean", True, [("dense", 1024, 1024, "tanh", True), ("layernorm", 1024, 1024, "identity", True)],
                     seed=16),
}


def head_weights(case: HeadCase) -> list:
    """The case's stages with seeded f32 weights: dicts of kind, weight, bias (or None), activation, eps."""
    rng = np.random.default_rng(case.seed + 7000)
    out = []
    for kind, n_in, n_out, act, bias in case.stages:
        if kind == "dense":
            w = rng.normal(0.0, 1.0 / np.sqrt(n_in), (n_out, n_in))
            b = rng.normal(0.0, 0.1, n_out) if bias else None
        else:
            w = 1.0 + rng.normal(0.0, 0.1, n_in)
            b = rng.normal(0.0, 0.1, n_in) if bias else None
        out.append({"kind": kind, "weight": w.astype(np.float32), "bias": None if b is None else b.astype(np.float32),
                    "activation": act, "eps": 1e-5})
    return out


def sequences(case: HeadCase, lens=LENS) -> list:
    rng = np.random.default_rng(case.seed + 9000)
    return [rng.integers(0, case.shape.vocab, size=n).astype(np.int32) for n in lens]


def apply_stages(rows: np.ndarray, stages: list, dtype=np.float64) -> np.ndarray:
    x = np.asarray(rows, dtype=dtype)
    for st in stages:
        w = st["weight"].astype(dtype)
        b = None if st["bias"] is None else st["bias"].astype(dtype)
        if st["kind"] == "dense":
            x = x @ w.T
            if b is not None:
                x = x + b
            if st["activation"] == "tanh":
                x = np.tanh(x)
            elif st["activation"] != "identity":
                raise ValueError(st["activation"])
        elif st["kind"] == "layernorm":
            mu = x.mean(axis=-1, keepdims=True)
            var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
            x = (x - mu) / np.sqrt(var + dtype(st["eps"])) * w
            if b is not None:
                x = x + b
        else:
            raise ValueError(st["kind"])
    return x


def apply_head(rows: np.ndarray, stages: list, normalize: bool, truncate: int = 0, dtype=np.float64) -> np.ndarray:
    """stages, then x / max(|x|, 1e-12) over the whole width, then the leading `truncate` columns (0: all)."""
    x = apply_stages(rows, stages, dtype)
    if normalize:
        x = x / np.maximum(np.sqrt((x * x).sum(axis=-1, keepdims=True)), dtype(1e-12))
    return x[:, :truncate] if truncate else x


def expected(case: HeadCase, w: dict, seqs, stages=None) -> np.ndarray:
    """The f64 embeddings of `seqs`: the BERT oracle's un-normalised pooled rows through the case's head."""
    pooled = obert.sentence_embeddings(w, case.shape, seqs, case.pooling, False, np.float64)
    return apply_head(pooled, head_weights(case) if stages is None else stages, case.normalize, case.truncate)


def stage_objects(stages: list) -> list:
    from voitta_rag_amd.encoder import HeadStage

    return [HeadStage(s["kind"], s["weight"], s["bias"], s["activation"], s["eps"]) for s in stages]


# ---- DistilBERT: BERT's body without token types, under its own tensor names ---------------------------------------------
DISTIL_RENAMES = [("attention.self.query", "attention.q_lin"), ("attention.self.key", "attention.k_lin"),
                  ("attention.self.value", "attention.v_lin"), ("attention.output.dense", "attention.out_lin"),
                  ("attention.output.LayerNorm", "sa_layer_norm"), ("intermediate.dense", "ffn.lin1"),
                  ("output.dense", "ffn.lin2"), ("output.LayerNorm", "output_layer_norm")]
DISTIL_SHAPE = obert.BertShape(2, 128, 2, 256, vocab=500, max_pos=160, type_vocab=1)
DISTIL_SEED = 21


def distilbert_weights(shape: obert.BertShape = DISTIL_SHAPE, seed: int = DISTIL_SEED, prefix: str = ""):
    """(BERT-named weights with a zero token-type row, for the BERT oracle; the same tensors as a DistilBertModel state
    dict names them, each key behind `prefix`)."""
    w = obert.random_weights(shape, seed)
    w[obert.EMB_KEYS["type"]] = np.zeros((1, shape.hidden), np.float32)
    state = {prefix + k: w[k] for k in (obert.EMB_KEYS["word"], obert.EMB_KEYS["pos"], obert.EMB_KEYS["ln_g"],
                                        obert.EMB_KEYS["ln_b"])}
    for i in range(shape.layers):
        for bert, distil in DISTIL_RENAMES:
            for kind in ("weight", "bias"):
                state[f"{prefix}transformer.layer.{i}.{distil}.{kind}"] = w[f"encoder.layer.{i}.{bert}.{kind}"]
    return w, state


# ---- synthetic sentence-transformers directories ---------------------------------------------------------------------------
ST = "sentence_transformers.models."
ACT_CLASS = {"tanh": "torch.nn.modules.activation.Tanh", "identity": "torch.nn.modules.linear.Identity"}


def _save(tensors: dict, d: str, weight_format: str) -> None:
    if weight_format == "safetensors":
        from safetensors.numpy import save_file

        save_file({k: np.ascontiguousarray(v) for k, v in tensors.items()}, os.path.join(d, "model.safetensors"))
    else:
        import torch

        torch.save({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in tensors.items()}, os.path.join(d, "pytorch_model.bin"))


def write_checkpoint(d: str, vocab: list, family: str = "bert", pooling: str = "mean", modules=(), seed: int = 31,
                     weight_format: str = "safetensors", prefix: str = "", body: bool = True, max_seq: int = 128):
    """A sentence-transformers directory of a tiny encoder (2 layers, 128 wide, 2 heads, FFN 256; family "bert" or
    "distilbert") whose modules.json lists Transformer, Pooling and then `modules` in order: a stage dict of
    head_weights (a Dense or LayerNorm module directory with config.json and weights), or a type name behind
    sentence_transformers.models. ("Normalize", "Dropout", anything else) with an empty directory. Returns (shape,
    BERT-named weights for the BERT oracle). body=False: no encoder weights are written (the readers need none)."""
    os.makedirs(os.path.join(d, "1_Pooling"), exist_ok=True)
    shape = obert.BertShape(2, 128, 2, 256, vocab=len(vocab), max_pos=160, type_vocab=1 if family == "distilbert" else 2)
    if family == "distilbert":
        cfg = {"model_type": "distilbert", "dim": 128, "n_heads": 2, "n_layers": 2, "hidden_dim": 256, "activation": "gelu",
               "vocab_size": len(vocab), "max_position_embeddings": shape.max_pos, "sinusoidal_pos_embds": False}
        w, state = distilbert_weights(shape, seed, prefix)
    else:
        cfg = {"model_type": "bert", "hidden_size": 128, "num_hidden_layers": 2, "num_attention_heads": 2,
               "intermediate_size": 256, "vocab_size": len(vocab), "max_position_embeddings": shape.max_pos,
               "type_vocab_size": 2, "layer_norm_eps": 1e-12, "hidden_act": "gelu"}
        w = obert.random_weights(shape, seed)
        state = {prefix + k: v for k, v in w.items()}
    json.dump(cfg, open(os.path.join(d, "config.json"), "w"))
    mods = [{"idx": 0, "name": "0", "path": "", "type": ST + "Transformer"},
            {"idx": 1, "name": "1", "path": "1_Pooling", "type": ST + "Pooling"}]
    for m in modules:
        idx = len(mods)
        kind = m if isinstance(m, str) else {"dense": "Dense", "layernorm": "LayerNorm"}[m["kind"]]
        sub = f"{idx}_{kind}"
        os.makedirs(os.path.join(d, sub), exist_ok=True)
        mods.append({"idx": idx, "name": str(idx), "path": sub, "type": ST + kind})
        if isinstance(m, str):
            continue
        if m["kind"] == "dense":
            n_out, n_in = m["weight"].shape
            json.dump({"in_features": n_in, "out_features": n_out, "bias": m["bias"] is not None,
                       "activation_function": m.get("activation_class") or ACT_CLASS[m["activation"]]},
                      open(os.path.join(d, sub, "config.json"), "w"))
            tensors = {"linear.weight": m["weight"]}
            if m["bias"] is not None:
                tensors["linear.bias"] = m["bias"]
        else:
            json.dump({"dimension": int(m["weight"].shape[0])}, open(os.path.join(d, sub, "config.json"), "w"))
            tensors = {"norm.weight": m["weight"], "norm.bias": m["bias"]}
        _save(tensors, os.path.join(d, sub), weight_format)
    json.dump(mods, open(os.path.join(d, "modules.json"), "w"))
    json.dump({"word_embedding_dimension": 128, "pooling_mode_cls_token": pooling == "cls",
               "pooling_mode_mean_tokens": pooling != "cls"}, open(os.path.join(d, "1_Pooling", "config.json"), "w"))
    json.dump({"max_seq_length": max_seq, "do_lower_case": family != "distilbert"},
              open(os.path.join(d, "sentence_bert_config.json"), "w"))
    json.dump({"do_lower_case": family != "distilbert"}, open(os.path.join(d, "tokenizer_config.json"), "w"))
    open(os.path.join(d, "vocab.txt"), "w", encoding="utf-8").write("\n".join(vocab) + "\n")
    if body:
        _save(state, d, weight_format)
    return shape, w
