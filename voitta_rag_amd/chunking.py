"""Drop-in for the reference's ``ChunkingService`` (src/voitta/services/chunking.py:9-246), the step
in front of the indexing path (services/indexing.py:380,515): same class, same
``Chunk`` fields, same constructor defaults (``x or settings.x``, so 0 falls back to the setting just
as it does there). The splitting runs in the native library (vr_chunk_texts, csrc/chunking.cpp), one
document per host thread; ``chunk_texts`` is the batched form the indexer uses to cut a whole folder
at once. Parity unpinned: see csrc/chunking.cpp. With VOITTA_LATE_CHUNKING=1 the chunk texts are
``LateChunkText``: plain strings that also carry their document, which is how ``embed_texts`` finds it. With
VOITTA_SEMANTIC_CHUNKING=1 the chunks are the encoder's (EmbeddingService.chunk_and_embed_documents) and their texts
``SemanticChunkText``: plain strings that also carry their vectors."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import late_chunking as _late
from ._lib import check, load_library
from .config import get_settings

_STRATEGY = {"recursive": 0, "sentence": 1, "fixed": 2}


@dataclass
class Chunk:
    """A chunk of text with its position (reference: chunking.py:9-16)."""

    text: str
    index: int
    start_char: int
    end_char: int


class ChunkingService:
    def __init__(self, chunk_size: int | None = None, chunk_overlap: int | None = None, strategy: str | None = None):
        settings = get_settings()
        self.chunk_size = chunk_size or settings.chunk_size            # chunking.py:29
        self.chunk_overlap = chunk_overlap or settings.chunk_overlap   # chunking.py:30
        self.strategy = strategy or settings.chunking_strategy         # chunking.py:31
        self._lib = load_library()

    def chunk_text(self, text: str) -> list[Chunk]:
        """chunking.py:33-45."""
        return self.chunk_texts([text])[0]

    def chunk_texts(self, texts: list[str]) -> list[list[Chunk]]:
        if get_settings().semantic_chunking:
            # semantic chunking (VOITTA_SEMANTIC_CHUNKING=1): the boundaries come from the encoder's forward pass, and so
            # do the chunks' vectors — the texts carry them (SemanticChunkText), which is how embed_texts finds them
            from .embedding import get_embedding_service

            return [chunks for chunks, _ in get_embedding_service().chunk_and_embed_documents(texts, chunker=self)]
        return self.cut(texts)

    def cut(self, texts: list[str]) -> list[list[Chunk]]:
        """The native chunker alone (vr_chunk_texts) at this service's size, overlap and strategy."""
        n = len(texts)
        if n == 0:
            return []
        raw = [(t or "").encode("utf-8", "surrogatepass") for t in texts]
        arr = (C.c_char_p * n)(*raw)
        lens = np.asarray([len(b) for b in raw], np.int64)
        handle = C.c_void_p()
        check(self._lib.vr_chunk_texts(arr, lens.ctypes.data_as(C.POINTER(C.c_int64)), n, int(self.chunk_size),
                                       int(self.chunk_overlap), _STRATEGY.get(self.strategy, 0), C.byref(handle)))
        try:
            count = C.c_int64()
            doc_off, span, text_off = (C.POINTER(C.c_int64)() for _ in range(3))
            blob = C.POINTER(C.c_char)()
            check(self._lib.vr_chunks_view(handle, C.byref(count), C.byref(doc_off), C.byref(span), C.byref(text_off),
                                           C.byref(blob)))
            m = count.value
            docs = np.ctypeslib.as_array(doc_off, (n + 1,)).copy()
            spans = np.ctypeslib.as_array(span, (2 * m,)).copy() if m else np.zeros(0, np.int64)
            offs = np.ctypeslib.as_array(text_off, (m + 1,)).copy()
            data = C.string_at(blob, int(offs[m])) if m else b""
        finally:
            self._lib.vr_chunks_free(handle)
        whole = data.decode("utf-8", "surrogatepass")
        offs, spans = offs.tolist(), spans.tolist()
        if len(whole) == len(data):  # pure ASCII: byte offsets are character offsets, slice the one decoded string
            texts_out = [whole[offs[i]:offs[i + 1]] for i in range(m)]
        else:
            texts_out = [data[offs[i]:offs[i + 1]].decode("utf-8", "surrogatepass") for i in range(m)]
        out: list[list[Chunk]] = []
        # late chunking (VOITTA_LATE_CHUNKING=1): a chunk text also knows its document, for embed_texts
        late = get_settings().late_chunking
        for d in range(n):
            lo, hi = int(docs[d]), int(docs[d + 1])
            own = _late.wrap_chunks(texts[d] or "", texts_out[lo:hi]) if late else texts_out[lo:hi]
            out.append([Chunk(own[i - lo], i - lo, spans[2 * i], spans[2 * i + 1]) for i in range(lo, hi)])
        return out


def get_chunking_service() -> ChunkingService:
    """chunking.py:244-246."""
    return ChunkingService()
