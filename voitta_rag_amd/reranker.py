"""Second-stage reranking: a BERT cross-encoder (``BertForSequenceClassification`` with one label, such as
cross-encoder/ms-marco-MiniLM-L-6-v2) or an XLM-R one (``XLMRobertaForSequenceClassification``: BAAI/bge-reranker-base,
-large) that reads a question and a passage together and scores the pair. It lives in
the engine beside the embedder (vr_reranker_load) and runs on the GPU: pair tokenisation on the host threads
(vr_wordpiece_encode_pairs / vr_unigram_encode_pairs), one forward pass and the classification head (vr_rerank / vr_rerank_text).

``NativeCrossEncoder`` answers what sentence-transformers' ``CrossEncoder`` does for one label: ``predict`` applies a
sigmoid (on the host, in f64) unless ``activation=False``; ``rank`` sorts the documents of one question."""
from __future__ import annotations

import json
import os
import threading

import numpy as np

from . import encoder as _enc
from .config import MAX_SEQ_LENGTH_LIMIT
from .embedding import SEQ_CAP_VARIABLE, NativeSentenceEncoder, seq_cap, slice_positions
from .store_registry import get_engine
from .unigram import UnigramTokenizer
from .wordpiece import WordPieceTokenizer

# XLMRobertaClassificationHead -> the head tensors of vr_reranker_load (encoder.HEAD_NAMES order): out_proj(tanh(dense
# h_<s>)) is what the BERT pooler + classifier compute
XLMR_HEAD = {"pooler.dense.weight": "classifier.dense.weight", "pooler.dense.bias": "classifier.dense.bias",
             "classifier.weight": "classifier.out_proj.weight", "classifier.bias": "classifier.out_proj.bias"}


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
    """config.json of a one-label BERT (read_config) or XLM-R (XLMRobertaForSequenceClassification) cross-encoder."""
    cfg = json.load(open(os.path.join(path, "config.json")))
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


class NativeCrossEncoder:
    def __init__(self, engine, desc: _enc.BertDesc, state: dict, tokenizer, max_length: int):
        self.engine = engine
        self.desc = desc
        self.tokenizer = tokenizer
        self.max_length = min(int(max_length), desc.max_pos)
        tokenizer.max_length = self.max_length
        _enc.load_reranker(engine, desc, state)

    @classmethod
    def from_pretrained(cls, path: str, engine=None, max_length: int | None = None) -> "NativeCrossEncoder":
        if not os.path.isdir(path):
            raise FileNotFoundError(f"reranker '{path}' is not a local checkpoint directory")
        cfg = read_cross_encoder_config(path)
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

    def logits(self, queries: list[str], candidates: list[list[str]]) -> list[np.ndarray]:
        """Raw logits of every (queries[q], candidates[q][j]) pair, one f32 array per question, in ONE engine call."""
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
