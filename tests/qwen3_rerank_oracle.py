"""TEST INFRASTRUCTURE — NumPy f64 restatement of Qwen3-Reranker's published scoring [EXT, the model card's text and
transformers' Qwen3ForCausalLM / Qwen3ForSequenceClassification], on top of tests/qwen3_oracle.py's body:
  ids     : prefix_ids + body_ids[:room] + suffix_ids, room = max_length - len(prefix_ids) - len(suffix_ids); prefix and
            suffix tokenised once without special tokens, the body "<Instruct>: .. <Query>: .. <Document>: .." on its own
            (`assemble`, pure Python over any text -> ids function)
  logit   : (W[yes] - W[no]) . h,  h = the final-normed hidden row of the pair's LAST token, W = lm_head.weight or, tied,
            embed_tokens.weight; the published score softmax((W[no] . h, W[yes] . h))[1] is sigmoid(logit)
Weights are seeded and never stored: qwen3_oracle.random_weights' body, with the "yes" and "no" rows of a tied embedding
(or the whole untied lm_head) drawn at HEAD_STD so that the logits are of the order real rerankers give (a few units)
instead of sqrt(2 H). tests/test_qwen3_rerank_cpu.py pins this file to transformers (tests/golden/qwen3_rerank_*.npz)
at 1e-9."""
from __future__ import annotations

import numpy as np

import qwen3_oracle as qo

PREFIX = ('<|im_start|>system\nJudge whether the Document meets the requirements based on the Query and the Instruct '
          'provided. Note that the answer can only be "yes" or "no".<|im_end|>\n<|im_start|>user\n')
SUFFIX = "<|im_end|>\n<|im_start|>assistant\n<think>\n\n</think>\n\n"
DEFAULT_INSTRUCTION = "Given a web search query, retrieve relevant passages that answer the query"

LM_HEAD_KEY = "lm_head.weight"
YES_ID, NO_ID = 7, 11  # the rows of the synthetic vocabulary that stand for "yes" and "no"


def body_text(instruction: str, query: str, document: str) -> str:
    return "<Instruct>: " + instruction + "\n<Query>: " + query + "\n<Document>: " + document


def assemble(encode, query: str, document: str, max_length: int, instruction: str = DEFAULT_INSTRUCTION) -> list[int]:
    """The ids of one pair. encode: text -> list of ids, without special tokens."""
    prefix, suffix = list(encode(PREFIX)), list(encode(SUFFIX))
    room = max_length - len(prefix) - len(suffix)
    if room < 1:
        raise ValueError(f"max_length {max_length} leaves {room} tokens for the body")
    return prefix + list(encode(body_text(instruction, query, document)))[:room] + suffix


def head_std(shape: qo.Qwen3Shape) -> float:
    """The standard deviation of the head's rows: (W[yes] - W[no]) . h then has one of about 3 (|h_i| is about 1)."""
    return 3.0 / np.sqrt(2.0 * shape.hidden)


def random_weights(shape: qo.Qwen3Shape, seed: int, tied: bool) -> dict[str, np.ndarray]:
    """qwen3_oracle.random_weights(shape, seed) with the head: tied, rows YES_ID and NO_ID of embed_tokens re-drawn at
    head_std; untied, an lm_head.weight [vocab, H] at head_std."""
    w = qo.random_weights(shape, seed)
    rng = np.random.default_rng(seed + 7000)
    if tied:
        w[qo.WORD_KEY] = w[qo.WORD_KEY].copy()
        w[qo.WORD_KEY][[YES_ID, NO_ID]] = rng.normal(0, head_std(shape), (2, shape.hidden)).astype(np.float32)
    else:
        w[LM_HEAD_KEY] = rng.normal(0, head_std(shape), (shape.vocab, shape.hidden)).astype(np.float32)
    return w


def score_row(w: dict, yes_id: int = YES_ID, no_id: int = NO_ID) -> np.ndarray:
    """W[yes] - W[no] in f64, [H]."""
    W = w[LM_HEAD_KEY] if LM_HEAD_KEY in w else w[qo.WORD_KEY]
    return W[yes_id].astype(np.float64) - W[no_id].astype(np.float64)


def body_weights(w: dict) -> dict:
    return {k: v for k, v in w.items() if k != LM_HEAD_KEY}


def row_logits(w: dict, shape: qo.Qwen3Shape, ids, causal: bool = True, row=None) -> np.ndarray:
    """The logit every token row of one pair would give, [S] f64 (the model's is the last); row: the head row, default
    score_row(w)."""
    return qo.encode_one(body_weights(w), shape, ids, causal) @ (score_row(w) if row is None else np.asarray(row, np.float64).ravel())


def logit(w: dict, shape: qo.Qwen3Shape, ids, causal: bool = True, row=None) -> float:
    return float(row_logits(w, shape, ids, causal, row)[-1])


def desc_for(shape: qo.Qwen3Shape, precision: str, max_pos: int = 512, causal: int = 1, **over):
    """The engine's description of `shape` as a decoder cross-encoder."""
    fields = dict(pooling="last", normalize=False)
    fields.update(over)
    return qo.desc_for(shape, fields.pop("pooling"), precision, max_pos=max_pos, causal=causal, **fields)


# ---- a synthetic Qwen3-Reranker directory ------------------------------------------------------------------------------------
SPECIALS = ["<|im_start|>", "<|im_end|>", "<think>", "</think>", "yes", "no"]


def make_tokenizer(words: list[str]):
    """A `tokenizers` WordLevel tokenizer over `words`, split on whitespace and punctuation, with the chat markers,
    <think>, </think>, yes and no as added tokens."""
    from tokenizers import Tokenizer, models, pre_tokenizers

    vocab = {"[UNK]": 0}
    for t in words:
        vocab.setdefault(t, len(vocab))
    tok = Tokenizer(models.WordLevel(vocab, unk_token="[UNK]"))
    tok.pre_tokenizer = pre_tokenizers.Sequence([pre_tokenizers.Whitespace()])
    tok.add_tokens(SPECIALS)
    return tok


def template_words() -> list[str]:
    import re

    text = PREFIX + SUFFIX + body_text(DEFAULT_INSTRUCTION, "", "")
    for s in SPECIALS[:4]:
        text = text.replace(s, " ")
    return sorted(set(re.findall(r"\w+|[^\w\s]+", text)))


def write_checkpoint(d: str, shape: qo.Qwen3Shape, seed: int, tok, arch: str = "Qwen3ForCausalLM", tied: bool = True,
                     config=None) -> tuple[dict, np.ndarray]:
    """config.json, tokenizer.json and model.safetensors of a seeded reranker; -> (body weights, the f64 head row).
    arch Qwen3ForCausalLM: the body under `model.`, lm_head.weight where untied, the "yes" / "no" rows at the tokenizer's
    ids. Qwen3ForSequenceClassification: score.weight [1, H] = the same row rounded to f32, num_labels 1."""
    import json
    import os

    from safetensors.numpy import save_file

    os.makedirs(d, exist_ok=True)
    yes, no = tok.token_to_id("yes"), tok.token_to_id("no")
    w = qo.random_weights(shape, seed)
    rng = np.random.default_rng(seed + 7000)
    W = w[qo.WORD_KEY].copy() if tied else rng.normal(0, head_std(shape), (shape.vocab, shape.hidden)).astype(np.float32)
    if tied:
        W[[yes, no]] = rng.normal(0, head_std(shape), (2, shape.hidden)).astype(np.float32)
        w[qo.WORD_KEY] = W
    row = W[yes].astype(np.float64) - W[no].astype(np.float64)
    cfg = qo.config_json(shape, architectures=[arch], tie_word_embeddings=tied, max_position_embeddings=512)
    out = {"model." + k: np.ascontiguousarray(v) for k, v in w.items()}
    if arch.endswith("ForSequenceClassification"):
        cfg["num_labels"] = 1
        out["score.weight"] = np.ascontiguousarray(row.astype(np.float32)[None, :])
        row = out["score.weight"][0].astype(np.float64)
    elif not tied:
        out[LM_HEAD_KEY] = W
    cfg.update(config or {})
    json.dump(cfg, open(os.path.join(d, "config.json"), "w"))
    tok.save(os.path.join(d, "tokenizer.json"))
    save_file(out, os.path.join(d, "model.safetensors"))
    return w, row
