"""Second-stage reranking: a BERT cross-encoder (``BertForSequenceClassification`` with one label, such as
cross-encoder/ms-marco-MiniLM-L-6-v2), an XLM-R one (``XLMRobertaForSequenceClassification``: BAAI/bge-reranker-base,
-large) or a ModernBERT one (``ModernBertForSequenceClassification``: Alibaba-NLP/gte-reranker-modernbert-base) that
reads a question and a passage together and scores the pair. It lives in
the engine beside the embedder (vr_reranker_load) and runs on the GPU: pair tokenisation on the host threads
(vr_wordpiece_encode_pairs / vr_unigram_encode_pairs), one forward pass and the classification head (vr_rerank / vr_rerank_text).
A ModernBERT checkpoint's byte-level BPE runs natively (vr_bpe_encode_pairs, vr_rerank_text_bpe); a tokenizer.json
outside that pipeline is tokenised by the HF `tokenizers` library (``LibraryPairTokenizer``) and scored by vr_rerank,
the same forward pass and head.
A decoder cross-encoder (Qwen3-Reranker-0.6B: ``Qwen3ForCausalLM`` scored by its "yes" logit against its "no" logit, or
a one-label ``Qwen3ForSequenceClassification`` / ``Qwen2ForSequenceClassification``) loads through
vr_reranker_load_decoder; ``DecoderPairTokenizer`` assembles its prompt (prefix + body + suffix) with the `tokenizers`
library and vr_rerank scores the ids. Its sigmoid(logit) IS the published score.

``NativeCrossEncoder`` answers what sentence-transformers' ``CrossEncoder`` does for one label: ``predict`` applies a
sigmoid (on the host, in f64) unless ``activation=False``; ``rank`` sorts the documents of one question."""
from __future__ import annotations

import dataclasses
import json
import logging
import os
import threading

import numpy as np

from . import encoder as _enc
from .bpe import BpeTokenizer
from .config import MAX_SEQ_LENGTH_LIMIT
from .embedding import (SEQ_CAP_VARIABLE, NativeSentenceEncoder, _read_modernbert_config, _read_qwen2_config,
                        _read_qwen3_config, seq_cap, slice_positions)
from .store_registry import get_engine
from .unigram import UnigramTokenizer
from .wordpiece import WordPieceTokenizer

logger = logging.getLogger(__name__)

# XLMRobertaClassificationHead -> the head tensors of vr_reranker_load (encoder.HEAD_NAMES order): out_proj(tanh(dense
# h_<s>)) is what the BERT pooler + classifier compute
XLMR_HEAD = {"pooler.dense.weight": "classifier.dense.weight", "pooler.dense.bias": "classifier.dense.bias",
             "classifier.weight": "classifier.out_proj.weight", "classifier.bias": "classifier.out_proj.bias"}


# Qwen3-Reranker's prompt, written from the model card's text: the ids of a pair are prefix + body + suffix
DECODER_PREFIX = ('<|im_start|>system\nJudge whether the Document meets the requirements based on the Query and the Instruct '
                  'provided. Note that the answer can only be "yes" or "no".<|im_end|>\n<|im_start|>user\n')
DECODER_SUFFIX = "<|im_end|>\n<|im_start|>assistant\n<think>\n\n</think>\n\n"
DEFAULT_INSTRUCTION = "Given a web search query, retrieve relevant passages that answer the query"
DECODER_ARCHS = {"qwen3": ("Qwen3ForCausalLM", "Qwen3ForSequenceClassification"),
                 "qwen2": ("Qwen2ForCausalLM", "Qwen2ForSequenceClassification")}


def decoder_body(instruction: str, query: str, document: str) -> str:
    return f"<Instruct>: {instruction}\n<Query>: {query}\n<Document>: {document}"


def sigmoid(x) -> np.ndarray:
    x = np.asarray(x, np.float64)
    return 1.0 / (1.0 + np.exp(-x))


def read_config(path: str) -> dict:
    """config.json of a one-label BERT cross-encoder; anything else is refused."""
    cfg = json.load(open(os.path.join(path, "config.json")))
    archs = cfg.get("architectures") or ["BertForSequenceClassification"]
    if cfg.get("model_type", "bert") != "bert" or archs != ["BertForSequenceClassification"]:
        raise ValueError(f"unsupported reranker {cfg.get('model_type')} / {archs}: BertForSequenceClassification only")
    return _check_head(cfg)


def read_cross_encoder_config(path: str) -> dict:
    """config.json of a one-label BERT (read_config), XLM-R (XLMRobertaForSequenceClassification) or ModernBERT
    (ModernBertForSequenceClassification) cross-encoder."""
    cfg = json.load(open(os.path.join(path, "config.json")))
    if cfg.get("model_type", "bert") in DECODER_ARCHS:  # a decoder cross-encoder: yes-minus-no of a causal LM, or one label
        kind = cfg["model_type"]
        causal_lm, seq_cls = DECODER_ARCHS[kind]
        archs = cfg.get("architectures") or []
        if archs not in ([causal_lm], [seq_cls]):
            raise ValueError(f"unsupported reranker {kind} / {archs}: {causal_lm} (scored by its yes and no logits) or "
                             f"{seq_cls} with one label only")
        if archs == [seq_cls]:
            labels = cfg.get("num_labels", len(cfg.get("id2label") or {0: "LABEL_0", 1: "LABEL_1"}))
            if labels != 1:
                raise ValueError(f"the reranker has {labels} labels: only one-label (relevance score) heads are implemented")
        return cfg
    if cfg.get("model_type", "bert") == "modernbert":
        archs = cfg.get("architectures") or ["ModernBertForSequenceClassification"]
        if archs != ["ModernBertForSequenceClassification"]:
            raise ValueError(f"unsupported reranker modernbert / {archs}: ModernBertForSequenceClassification only")
        labels = cfg.get("num_labels", len(cfg.get("id2label") or {0: "LABEL_0"}))
        if labels != 1:
            raise ValueError(f"the reranker has {labels} labels: only one-label (relevance score) heads are implemented")
        if cfg.get("classifier_activation", "gelu") != "gelu":
            raise ValueError(f"classifier_activation {cfg.get('classifier_activation')!r} is not implemented: the head's "
                             "activation is the exact-erf GELU")
        if cfg.get("classifier_pooling", "cls") not in ("cls", "mean"):
            raise ValueError(f"classifier_pooling {cfg.get('classifier_pooling')!r} is not implemented: cls or mean")
        return cfg
    if cfg.get("model_type", "bert") != "xlm-roberta":
        return read_config(path)
    archs = cfg.get("architectures") or ["XLMRobertaForSequenceClassification"]
    if archs != ["XLMRobertaForSequenceClassification"]:
        raise ValueError(f"unsupported reranker xlm-roberta / {archs}: XLMRobertaForSequenceClassification only")
    return _check_head(cfg)


def _check_head(cfg: dict) -> dict:
    labels = cfg.get("num_labels", len(cfg.get("id2label") or {0: "LABEL_0"}))
    if labels != 1:
        raise ValueError(f"the reranker has {labels} labels: only one-label (relevance score) heads are implemented")
    if cfg.get("hidden_act", "gelu") != "gelu" or cfg.get("position_embedding_type", "absolute") != "absolute":
        raise ValueError("only exact-erf GELU and absolute position embeddings are implemented")
    return cfg


class LibraryPairTokenizer:
    """Pair tokenisation by the HF `tokenizers` library, for a tokenizer.json the engine has no tokenizer for (a
    byte-level BPE outside bpe.parse_tokenizer_json's pipeline): encode_pairs as the native tokenizers answer it,
    LongestFirst truncation to max_length."""

    def __init__(self, tok, max_length: int):
        self._tok = tok
        self._tok.no_padding()
        self.max_length = int(max_length)

    @property
    def max_length(self) -> int:
        return self._max_length

    @max_length.setter
    def max_length(self, value: int) -> None:
        self._max_length = int(value)
        self._tok.enable_truncation(max_length=self._max_length, strategy="longest_first")

    @classmethod
    def from_pretrained(cls, path: str, max_length: int) -> "LibraryPairTokenizer":
        from tokenizers import Tokenizer

        tj = os.path.join(path, "tokenizer.json")
        if not os.path.exists(tj):
            raise FileNotFoundError(f"no tokenizer.json under {path}")
        return cls(Tokenizer.from_file(tj), max_length)

    def encode_pairs(self, a: list[str], b: list[str]):
        """-> (ids int32, offsets int64, seg_b int32): the packed pair sequences and the index of each B's first id."""
        encs = self._tok.encode_batch(list(zip(a, b)))
        off = np.zeros(len(encs) + 1, np.int64)
        off[1:] = np.cumsum([len(e.ids) for e in encs])
        ids = np.fromiter((t for e in encs for t in e.ids), dtype=np.int32, count=int(off[-1]))
        seg = np.array([next((i for i, s in enumerate(e.sequence_ids) if s == 1), len(e.ids) - 1) for e in encs], np.int32)
        return ids, off, seg


class DecoderPairTokenizer(LibraryPairTokenizer):
    """The prompt of a decoder cross-encoder (Qwen3-Reranker) through the HF `tokenizers` library: the prefix and the
    suffix are tokenised once, without special tokens; the body "<Instruct>: .. <Query>: .. <Document>: .." of every pair
    on its own, cut from the right to max_length - len(prefix) - len(suffix) tokens. encode_pairs answers as
    LibraryPairTokenizer's does, with no segment array: the model has one token type."""

    def __init__(self, tok, max_length: int, instruction: str = DEFAULT_INSTRUCTION):
        self._tok = tok
        self._tok.no_padding()
        self._tok.no_truncation()
        self.instruction = instruction or DEFAULT_INSTRUCTION
        self.prefix_ids = list(tok.encode(DECODER_PREFIX, add_special_tokens=False).ids)
        self.suffix_ids = list(tok.encode(DECODER_SUFFIX, add_special_tokens=False).ids)
        self.max_length = max_length

    @property
    def max_length(self) -> int:
        return self._max_length

    @max_length.setter
    def max_length(self, value: int) -> None:
        room = int(value) - len(self.prefix_ids) - len(self.suffix_ids)
        if room < 1:
            raise ValueError(f"max_length {int(value)} leaves {room} tokens for the body of a pair: the prompt's prefix and "
                             f"suffix take {len(self.prefix_ids)} + {len(self.suffix_ids)}")
        self._max_length = int(value)

    @classmethod
    def from_pretrained(cls, path: str, max_length: int, instruction: str = DEFAULT_INSTRUCTION) -> "DecoderPairTokenizer":
        from tokenizers import Tokenizer

        tj = os.path.join(path, "tokenizer.json")
        if not os.path.exists(tj):
            raise FileNotFoundError(f"no tokenizer.json under {path}")
        return cls(Tokenizer.from_file(tj), max_length, instruction)

    def token_to_id(self, token: str):
        return self._tok.token_to_id(token)

    def encode_pairs(self, a: list[str], b: list[str]):
        """-> (ids int32, offsets int64, None): prefix + body[:room] + suffix of every (query, document) pair."""
        room = self._max_length - len(self.prefix_ids) - len(self.suffix_ids)
        encs = self._tok.encode_batch([decoder_body(self.instruction, q, d) for q, d in zip(a, b)], add_special_tokens=False)
        seqs = [self.prefix_ids + list(e.ids)[:room] + self.suffix_ids for e in encs]
        off = np.zeros(len(seqs) + 1, np.int64)
        off[1:] = np.cumsum([len(s) for s in seqs])
        ids = np.fromiter((t for s in seqs for t in s), dtype=np.int32, count=int(off[-1]))
        return ids, off, None


class NativeCrossEncoder:
    def __init__(self, engine, desc: _enc.BertDesc, state: dict, tokenizer, max_length: int, **head):
        self.engine = engine
        self.desc = desc
        self.tokenizer = tokenizer
        self.max_length = min(int(max_length), desc.max_pos)
        tokenizer.max_length = self.max_length
        _enc.load_reranker(engine, desc, state, **head)

    @classmethod
    def from_pretrained(cls, path: str, engine=None, max_length: int | None = None,
                        instruction: str | None = None) -> "NativeCrossEncoder":
        if not os.path.isdir(path):
            raise FileNotFoundError(f"reranker '{path}' is not a local checkpoint directory")
        cfg = read_cross_encoder_config(path)
        if cfg.get("model_type", "bert") in DECODER_ARCHS:
            return cls._decoder(path, cfg, engine, max_length, instruction)
        if cfg.get("model_type", "bert") == "modernbert":
            return cls._modernbert(path, cfg, engine, max_length)
        xlmr = cfg.get("model_type", "bert") == "xlm-roberta"
        pos_start = int(cfg.get("pad_token_id", 1)) + 1 if xlmr else 0  # XLM-R: position p reads row pad + 1 + p
        max_pos = int(cfg["max_position_embeddings"]) - pos_start
        desc = _enc.BertDesc(layers=cfg["num_hidden_layers"], hidden=cfg["hidden_size"],
                             heads=cfg["num_attention_heads"], intermediate=cfg["intermediate_size"],
                             vocab=cfg["vocab_size"], max_pos=max_pos,
                             type_vocab=cfg.get("type_vocab_size", 2), pooling="cls", normalize=False,
                             eps=cfg.get("layer_norm_eps", 1e-12),
                             precision=os.environ.get("VOITTA_RERANK_PRECISION", "f16"))
        if max_length is None:
            max_length = max_pos
            tc = os.path.join(path, "tokenizer_config.json")
            if os.path.exists(tc):
                ml = json.load(open(tc)).get("model_max_length")
                if isinstance(ml, int) and ml > 0:
                    max_length = min(max_length, ml)
        cap = seq_cap()
        if xlmr and min(int(max_length), max_pos) > cap:
            raise ValueError(f"reranker {path} reads pairs of up to {min(int(max_length), max_pos)} tokens; the engine "
                             f"runs at most {cap}: pass max_length <= {cap}, or raise {SEQ_CAP_VARIABLE} (up to "
                             f"{MAX_SEQ_LENGTH_LIMIT})")
        state = NativeSentenceEncoder._load_weights(path)
        if not xlmr:
            return cls(engine or get_engine(), desc, state, WordPieceTokenizer.from_pretrained(path, max_length),
                       max_length)
        state = slice_positions(state, pos_start)
        for head, name in XLMR_HEAD.items():
            state[head] = state.pop(name)
        return cls(engine or get_engine(), desc, state, UnigramTokenizer.from_pretrained(path, max_length), max_length)

    @classmethod
    def _modernbert(cls, path: str, cfg: dict, engine, max_length: int | None) -> "NativeCrossEncoder":
        """A ModernBertForSequenceClassification directory: the body as the embedder reads it (_read_modernbert_config,
        sequences capped at seq_cap()), pooled as classifier_pooling says, not normalised."""
        rc = _read_modernbert_config(path, cfg)
        if max_length is None:
            max_length = rc["max_seq"]
            tc = os.path.join(path, "tokenizer_config.json")
            if os.path.exists(tc):
                ml = json.load(open(tc)).get("model_max_length")
                if isinstance(ml, int) and ml > 0:
                    max_length = min(max_length, ml)
        desc = dataclasses.replace(rc["desc"], pooling=cfg.get("classifier_pooling", "cls"), normalize=False,
                                   precision=os.environ.get("VOITTA_RERANK_PRECISION", "f16"))
        state = NativeSentenceEncoder._load_weights(path)
        max_length = min(int(max_length), desc.max_pos)
        try:
            tokenizer = BpeTokenizer.from_pretrained(path, max_length)
        except (ValueError, KeyError, TypeError) as e:
            logger.info("native byte-level BPE not applicable (%s); using the tokenizers library", e)
            tokenizer = LibraryPairTokenizer.from_pretrained(path, max_length)
        return cls(engine or get_engine(), desc, state, tokenizer, max_length)

    @classmethod
    def _decoder(cls, path: str, cfg: dict, engine, max_length: int | None, instruction: str | None) -> "NativeCrossEncoder":
        """A qwen3 / qwen2 reranker directory: the body as the embedder reads it (_read_qwen3_config / _read_qwen2_config),
        pooled at the last token, not normalised; the head row from score.weight or from the "yes" and "no" rows of
        lm_head; max_length = min(seq_cap(), max_position_embeddings, the tokenizer's model_max_length)."""
        from .config import get_settings

        rc = (_read_qwen3_config if cfg["model_type"] == "qwen3" else _read_qwen2_config)(path, cfg)
        desc = dataclasses.replace(rc["desc"], pooling="last", normalize=False,
                                   max_pos=min(seq_cap(), int(cfg.get("max_position_embeddings", 32768))),
                                   precision=os.environ.get("VOITTA_RERANK_PRECISION", "f16"))
        if max_length is None:
            max_length = desc.max_pos
            tc = os.path.join(path, "tokenizer_config.json")
            if os.path.exists(tc):
                ml = json.load(open(tc)).get("model_max_length")
                if isinstance(ml, int) and ml > 0:
                    max_length = min(max_length, ml)
        max_length = min(int(max_length), desc.max_pos)
        if instruction is None:
            instruction = get_settings().rerank_instruction
        tokenizer = DecoderPairTokenizer.from_pretrained(path, max_length, instruction or DEFAULT_INSTRUCTION)
        head = {}
        if (cfg.get("architectures") or [""])[0].endswith("ForCausalLM"):
            head = {"yes_id": tokenizer.token_to_id("yes"), "no_id": tokenizer.token_to_id("no")}
            for what, i in (("yes", head["yes_id"]), ("no", head["no_id"])):
                if i is None:
                    raise ValueError(f"the tokenizer of {path} has no token '{what}': a causal-LM reranker is scored by its "
                                     "'yes' logit against its 'no' logit")
        state = NativeSentenceEncoder._load_weights(path)
        return cls(engine or get_engine(), desc, state, tokenizer, max_length, **head)

    def logits(self, queries: list[str], candidates: list[list[str]]) -> list[np.ndarray]:
        """Raw logits of every (queries[q], candidates[q][j]) pair, one f32 array per question, in ONE engine call
        (a LibraryPairTokenizer: one tokenizers-library call, then one vr_rerank)."""
        if isinstance(self.tokenizer, LibraryPairTokenizer):
            a = [q for q, c in zip(queries, candidates) for _ in c]
            cand_off = np.zeros(len(queries) + 1, np.int64)
            cand_off[1:] = np.cumsum([len(c) for c in candidates])
            if not a:
                return [np.zeros(0, np.float32) for _ in queries]
            ids, off, _ = self.tokenizer.encode_pairs(a, [p for c in candidates for p in c])
            out = self.engine.rerank(ids, off.astype(np.int32), None)
            return [out[cand_off[i]:cand_off[i + 1]].copy() for i in range(len(queries))]
        return self.engine.rerank_text(self.tokenizer, queries, candidates, self.max_length)

    def predict(self, pairs, activation: bool = True) -> np.ndarray:
        """pairs: [(question, passage)] -> one score per pair: sigmoid(logit) in f64, or the f32 logit itself."""
        pairs = list(pairs)
        if not pairs:
            return np.zeros(0, np.float64 if activation else np.float32)
        # consecutive pairs of one question form one candidate list (the question is tokenised once)
        queries, cands = [], []
        for q, p in pairs:
            if not queries or queries[-1] != q:
                queries.append(q)
                cands.append([])
            cands[-1].append(p)
        out = np.concatenate(self.logits(queries, cands))
        return sigmoid(out) if activation else out

    def rank(self, query: str, documents: list[str], top_k: int | None = None) -> list[dict]:
        """[{"corpus_id", "score"}] of the documents, best first (stable for equal scores)."""
        if not documents:
            return []
        scores = sigmoid(self.logits([query], [list(documents)])[0])
        order = np.argsort(-scores, kind="stable")
        if top_k is not None:
            order = order[:top_k]
        return [{"corpus_id": int(i), "score": float(scores[i])} for i in order]


def rerank_candidates(settings_candidates: int, limit: int) -> int:
    """How many hybrid candidates a reranked search fetches: VOITTA_RERANK_CANDIDATES clamped to [limit, 341]
    (341 = the largest limit of a hybrid search, kMaxK / 3)."""
    return max(int(limit), min(int(settings_candidates), 341))




_loaded: dict = {}
_loaded_lock = threading.Lock()


def get_reranker(engine, path: str) -> NativeCrossEncoder:
    """The cross-encoder at `path`, loaded into `engine` once (its reranker slot holds one model)."""
    with _loaded_lock:
        key = id(engine)
        rr = _loaded.get(key)
        if rr is None or rr[0] != path or rr[1].engine is not engine:
            rr = (path, NativeCrossEncoder.from_pretrained(path, engine))
            _loaded[key] = rr
        return rr[1]
