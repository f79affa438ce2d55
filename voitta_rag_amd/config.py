"""Settings of the native services. Same environment variables and defaults as the reference's
``Settings`` for the hot path (src/voitta/config.py:28-44,72), plus the few the native engine adds
(SURVEY.md §5 "Config / flags"). EMBEDDING_MODEL must be a local checkpoint directory: there is no
network, so hub names cannot be resolved."""
from __future__ import annotations

import os
from functools import lru_cache


DEFAULT_MAX_SEQ_LENGTH = 512
MAX_SEQ_LENGTH_LIMIT = 8192  # the longest sequence the engine loads a model for (vr_encoder_load / vr_reranker_load)
DEFAULT_LATE_CHUNKING_CONTEXT = 256
DEFAULT_SEMANTIC_UNIT_CHARS = 200   # a sentence or two
DEFAULT_SEMANTIC_MIN_TOKENS = 32
DEFAULT_SEMANTIC_MAX_TOKENS = 256


class Settings:
    def __init__(self):
        self.qdrant_collection: str = os.getenv("QDRANT_COLLECTION", "voitta_documents")  # config.py:30
        self.embedding_model: str = os.getenv("EMBEDDING_MODEL", "intfloat/e5-base-v2")    # config.py:33
        self.embedding_dimension: int = int(os.getenv("EMBEDDING_DIMENSION", "768"))       # config.py:34
        self.embedding_device: str = os.getenv("EMBEDDING_DEVICE", "auto")                 # config.py:36
        self.chunk_size: int = int(os.getenv("CHUNK_SIZE", "512"))                         # config.py:39
        self.chunk_overlap: int = int(os.getenv("CHUNK_OVERLAP", "50"))                    # config.py:40
        self.chunking_strategy: str = os.getenv("CHUNKING_STRATEGY", "recursive")          # config.py:41
        self.sparse_weight: float = float(os.getenv("SPARSE_WEIGHT", "0.1"))               # config.py:44
        self.mcp_search_limit: int = int(os.getenv("MCP_SEARCH_LIMIT", "20"))              # config.py:72
        # native additions
        self.gpu: int = int(os.getenv("VOITTA_GPU", os.getenv("LOCAL_RANK", "0")))
        self.initial_rows: int = int(os.getenv("VOITTA_INITIAL_ROWS", "0"))
        # directory of the persisted index (VectorStoreService.save / load); loaded on first use when present
        self.index_dir: str = os.getenv("VOITTA_INDEX_DIR", "")
        # second-stage reranking (opt-in): a local cross-encoder checkpoint (one-label BERT, XLM-R or ModernBERT, or a
        # Qwen3-Reranker); a search fetches this many hybrid candidates (clamped to [limit, 341]), rescores them on the
        # GPU and returns the best `limit`
        self.rerank_model: str = os.getenv("VOITTA_RERANK_MODEL", "")
        self.rerank_candidates: int = int(os.getenv("VOITTA_RERANK_CANDIDATES", "50"))
        # the task instruction a decoder cross-encoder (Qwen3-Reranker) reads in front of every pair; empty = the
        # model card's default (reranker.DEFAULT_INSTRUCTION). Other rerankers ignore it
        self.rerank_instruction: str = os.getenv("VOITTA_RERANK_INSTRUCTION", "")
        # MMR diversification of search results (opt-in): unset = off; a value in [0, 1] is the diversity d of every
        # search. The first stage then fetches VOITTA_MMR_CANDIDATES (clamped to [limit, 341]) and MMR selects `limit`
        mmr = os.getenv("VOITTA_MMR_DIVERSITY", "")
        self.mmr_diversity: float | None = float(mmr) if mmr.strip() else None
        self.mmr_candidates: int = int(os.getenv("VOITTA_MMR_CANDIDATES", "50"))
        # task prefixes (opt-in, empty = none) put in front of every passage / query text before tokenisation, for models
        # that expect them and that the reference's e5 rule does not know (nomic: "search_document: " / "search_query: ")
        self.embed_passage_prefix: str = os.getenv("VOITTA_EMBED_PASSAGE_PREFIX", "")
        self.embed_query_prefix: str = os.getenv("VOITTA_EMBED_QUERY_PREFIX", "")
        # the leading columns of the model's output that are the embedding (opt-in; unset or empty = all of them):
        # SentenceTransformer's truncate_dim, for models trained so that a prefix of their vector still ranks well
        # (Matryoshka). A multiple of 16 within the model's width, checked when the model is read; EMBEDDING_DIMENSION
        # must then be this width
        trunc = os.getenv("VOITTA_EMBED_TRUNCATE_DIM", "").strip()
        self.embed_truncate_dim: int = int(trunc) if trunc else 0
        if trunc and (self.embed_truncate_dim < 16 or self.embed_truncate_dim % 16):
            raise ValueError(f"VOITTA_EMBED_TRUNCATE_DIM={trunc}: accepted values are the multiples of 16 from 16 to the "
                             "model's output width (unset = no truncation)")
        # the longest sequence, in tokens, that an embedder or reranker may run (opt-in above 512): a rotary checkpoint
        # that declares more is truncated to it, an XLM-R one is refused; past 640 tokens attention streams its keys
        self.max_seq_length: int = int(os.getenv("VOITTA_MAX_SEQ_LENGTH", str(DEFAULT_MAX_SEQ_LENGTH)))
        if not 1 <= self.max_seq_length <= MAX_SEQ_LENGTH_LIMIT:
            raise ValueError(f"VOITTA_MAX_SEQ_LENGTH={self.max_seq_length}: accepted values are 1 ... "
                             f"{MAX_SEQ_LENGTH_LIMIT} (default {DEFAULT_MAX_SEQ_LENGTH})")
        # late chunking (opt-in): a document goes through the encoder once, in windows of the model's max_seq_length,
        # and each stored chunk's dense vector is the mean of its own tokens' final hidden states. A follow-on window
        # of a document longer than the window starts this many tokens before its first chunk (left context)
        late = os.getenv("VOITTA_LATE_CHUNKING", "0").strip() or "0"
        if late not in ("0", "1"):
            raise ValueError(f"VOITTA_LATE_CHUNKING={late}: accepted values are 0 and 1 (default 0)")
        self.late_chunking: bool = late == "1"
        self.late_chunking_context: int = int(os.getenv("VOITTA_LATE_CHUNKING_CONTEXT",
                                                        str(min(DEFAULT_LATE_CHUNKING_CONTEXT, self.max_seq_length // 2))))
        if not 0 <= self.late_chunking_context <= self.max_seq_length // 2:
            raise ValueError(f"VOITTA_LATE_CHUNKING_CONTEXT={self.late_chunking_context}: accepted values are 0 ... "
                             f"{self.max_seq_length // 2} (half of VOITTA_MAX_SEQ_LENGTH={self.max_seq_length}; default "
                             f"{DEFAULT_LATE_CHUNKING_CONTEXT})")
        # semantic chunking (opt-in): a file is cut into sentence-sized units (the `sentence` strategy at
        # VOITTA_SEMANTIC_UNIT_CHARS characters), goes through the encoder once as late chunking sends it, and the device
        # breaks where neighbouring units stop resembling each other: at the break_permille/1000 largest distances of a
        # sequence that are at least min_distance, a chunk holding min_tokens ... max_tokens tokens (vr_encode_semantic).
        # The chunks come back with their late-chunked vectors. Defaults: the 95th percentile, one unit of buffer
        semantic = os.getenv("VOITTA_SEMANTIC_CHUNKING", "0").strip() or "0"
        if semantic not in ("0", "1"):
            raise ValueError(f"VOITTA_SEMANTIC_CHUNKING={semantic}: accepted values are 0 and 1 (default 0)")
        self.semantic_chunking: bool = semantic == "1"
        if self.semantic_chunking and self.late_chunking:
            raise ValueError("VOITTA_SEMANTIC_CHUNKING=1 together with VOITTA_LATE_CHUNKING=1: semantic chunks are "
                             "late-chunked already, set one of the two")

        def ranged(name: str, default: int, lo: int, hi: int, note: str = "") -> int:
            raw = os.getenv(name, str(default)).strip() or str(default)
            try:
                value = int(raw)
            except ValueError:
                value = lo - 1
            if not lo <= value <= hi:
                raise ValueError(f"{name}={raw}: accepted values are {lo} ... {hi}{note} (default {default})")
            return value

        self.semantic_unit_chars: int = ranged("VOITTA_SEMANTIC_UNIT_CHARS", DEFAULT_SEMANTIC_UNIT_CHARS, 16, 65536)
        self.semantic_buffer: int = ranged("VOITTA_SEMANTIC_BUFFER", 1, 0, 3)
        self.semantic_break_permille: int = ranged("VOITTA_SEMANTIC_BREAK_PERMILLE", 50, 0, 1000)
        self.semantic_max_tokens: int = ranged("VOITTA_SEMANTIC_MAX_TOKENS", min(DEFAULT_SEMANTIC_MAX_TOKENS, self.max_seq_length),
                                               1, self.max_seq_length, f" (VOITTA_MAX_SEQ_LENGTH={self.max_seq_length})")
        self.semantic_min_tokens: int = ranged("VOITTA_SEMANTIC_MIN_TOKENS", min(DEFAULT_SEMANTIC_MIN_TOKENS, self.semantic_max_tokens),
                                               0, self.semantic_max_tokens,
                                               f" (VOITTA_SEMANTIC_MAX_TOKENS={self.semantic_max_tokens})")
        raw = os.getenv("VOITTA_SEMANTIC_MIN_DISTANCE", "0").strip() or "0"
        try:
            self.semantic_min_distance: float = float(raw)
        except ValueError:
            self.semantic_min_distance = float("nan")
        if not 0.0 <= self.semantic_min_distance <= 2.0:
            raise ValueError(f"VOITTA_SEMANTIC_MIN_DISTANCE={raw}: accepted values are 0 ... 2, a cosine distance (default 0)")


@lru_cache
def get_settings() -> Settings:
    return Settings()
