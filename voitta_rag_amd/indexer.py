"""Bulk front-end of the indexing path: parsed files in, stored rows out.

The reference indexes one file at a time (IndexingService._index_file_standard,
src/voitta/services/indexing.py:513-563): ``chunker.chunk_text`` → ``embedder.embed_texts`` →
``sparse_embedder.embed_texts`` → ``vector_store.store_chunks``, each step waiting for the one
before and N×D Python floats passing between them. ``BulkIndexer`` runs the same four steps for a
stream of files with the same stored result (same chunks, payload fields, vectors and scores), but

* cut into batches of ``batch_chunks`` chunks regardless of file boundaries (a 3-chunk file does not
  pay a GPU launch sequence of its own) — with VOITTA_LATE_CHUNKING=1, into batches of whole files until
  ``batch_chunks`` is reached: a file's chunks are token spans of the file's own sequences
  (late_chunking.plan_many, vr_index_batch_spans), so a batch never holds half a file; with
  VOITTA_SEMANTIC_CHUNKING=1 a group of whole files is chunked AND embedded by one forward pass
  (vr_encode_semantic) and stored with store_chunks,
* the host stages — chunking (vr_chunk_texts), WordPiece (vr_wordpiece_encode) and the BM25 tokeniser
  (vr_bm25_tokenize), all on every host thread — run on a producer thread for batch i+1 while
* point ids and payload dicts of batch i+1 are made there too (VectorStoreService.prepare_rows), and
* the GPU stages of batch i run as ONE engine call (vr_index_batch: encode → tf → append, nothing
  leaves HBM) on the caller's thread. ctypes drops the GIL inside both, so they overlap.

What the caller owns stays with the caller: parsing, content hashes, the SQL ``IndexedFile`` rows
(indexing.py:565-600). ``index_files`` returns the chunk count per file for that bookkeeping."""
from __future__ import annotations

import queue
import threading
from dataclasses import dataclass
from datetime import datetime, timezone
from typing import Iterable, Iterator

from . import bm25 as _bm25
from .config import get_settings
from .chunking import ChunkingService, get_chunking_service
from .embedding import EmbeddingService, get_embedding_service
from .vector_store import ChunkMetadata, VectorStoreService, get_vector_store


@dataclass
class ParsedFile:
    """What _index_file_standard holds once a file is parsed (indexing.py:486-512,537-552)."""

    content: str
    file_path: str
    folder_path: str
    index_folder: str
    file_name: str
    source_created_at: int | None = None
    source_modified_at: int | None = None
    allowed_users: list[str] | None = None
    source_url: str | None = None


@dataclass
class _Batch:
    texts: list[str]
    metadatas: list[ChunkMetadata]
    wp_ids: object
    wp_off: object
    bm_ids: object
    bm_off: object
    counts: dict[str, int]
    rows: tuple | None = None  # (point ids, payload dicts) made on the producer thread
    spans: tuple | None = None  # late chunking: (n_seq, span_off, span_tok), wp_ids / wp_off are document windows


class BulkIndexer:
    def __init__(self, chunker: ChunkingService | None = None, embedder: EmbeddingService | None = None,
                 vector_store: VectorStoreService | None = None, sparse: bool = True, batch_chunks: int = 4096,
                 files_per_cut: int = 64):
        self.chunker = chunker or get_chunking_service()
        self.embedder = embedder or get_embedding_service()
        self.vector_store = vector_store or get_vector_store()
        self.sparse = sparse
        self.batch_chunks = int(batch_chunks)
        self.files_per_cut = int(files_per_cut)
        # late chunking (VOITTA_LATE_CHUNKING=1): a batch is whole files, their contents kept beside the chunks
        self.late = get_settings().late_chunking
        # semantic chunking (VOITTA_SEMANTIC_CHUNKING=1): chunks and vectors come out of one pass per group of whole files
        self.semantic = get_settings().semantic_chunking

    @staticmethod
    def _metadata(f: ParsedFile, c, total: int, indexed_at: str) -> ChunkMetadata:
        return ChunkMetadata(
            file_path=f.file_path, folder_path=f.folder_path, index_folder=f.index_folder,
            file_name=f.file_name, chunk_index=c.index, total_chunks=total,
            start_char=c.start_char, end_char=c.end_char, indexed_at=indexed_at,
            source_created_at=f.source_created_at, source_modified_at=f.source_modified_at,
            allowed_users=f.allowed_users, source_url=f.source_url)

    # ---- semantic chunking: the chunks are only known after the forward pass -------------------------
    def _index_files_semantic(self, files: Iterable[ParsedFile]) -> dict[str, int]:
        """VOITTA_SEMANTIC_CHUNKING=1: per group of ``files_per_cut`` whole files ONE forward pass gives the chunks and
        their vectors (EmbeddingService.chunk_and_embed_documents); they are stored with store_chunks, the sparse
        vectors from the chunk texts as the per-file sequence makes them. The fused vr_index_batch cannot serve here:
        it needs the row count before the pass."""
        from .sparse_embedding import SparseEmbeddingService

        sparse_embedder = SparseEmbeddingService() if self.sparse else None
        done: dict[str, int] = {}

        def flush(group: list[ParsedFile]):
            indexed_at = datetime.now(timezone.utc).isoformat()
            rows = []
            results = self.embedder.chunk_and_embed_documents([f.content for f in group], chunker=self.chunker)
            for f, (chunks, vectors) in zip(group, results):
                done[f.file_path] = len(chunks)
                rows += [(str(c.text), v, self._metadata(f, c, len(chunks), indexed_at)) for c, v in zip(chunks, vectors)]
            if rows:
                sparse = sparse_embedder.embed_texts([r[0] for r in rows]) if sparse_embedder else None
                self.vector_store.store_chunks(rows, sparse)

        group: list[ParsedFile] = []
        for f in files:
            group.append(f)
            if len(group) >= self.files_per_cut:
                flush(group)
                group = []
        if group:
            flush(group)
        return done

    # ---- host stages (producer thread) -------------------------------------------------------------
    def _tokenise(self, texts: list[str], metadatas: list[ChunkMetadata], counts: dict[str, int],
                  documents: list | None = None) -> _Batch:
        model = self.embedder.model
        spans = None
        if documents is not None:  # [(content, its chunk texts)]: the texts of this batch, file by file
            plan = model.plan_documents(documents, self.embedder._passage(""))
            wp_ids, wp_off, spans = plan.ids, plan.offsets, plan.spans()
        else:
            encoder_texts = texts
            if "e5" in self.embedder.model_name.lower():  # embedding.py:65-66
                encoder_texts = [f"passage: {t}" for t in texts]
            wp_ids, wp_off = model.tokenize(encoder_texts)
        bm_ids = bm_off = None
        if self.sparse:
            bm_off, bm_ids = _bm25.hashed_stems(texts)  # BM25 sees the chunk text itself (indexing.py:529-530)
        rows = self.vector_store.prepare_rows(texts, metadatas) if hasattr(self.vector_store, "prepare_rows") else None
        return _Batch(texts, metadatas, wp_ids, wp_off, bm_ids, bm_off, counts, rows, spans)

    def _batches(self, files: Iterable[ParsedFile]) -> Iterator[_Batch]:
        texts: list[str] = []
        metadatas: list[ChunkMetadata] = []
        counts: dict[str, int] = {}
        pending: list[ParsedFile] = []
        documents: list = []  # late chunking: (content, chunk texts) of every file with chunks, in the order of `texts`

        def cut(group: list[ParsedFile]):
            indexed_at = datetime.now(timezone.utc).isoformat()  # indexing.py:538
            for f, chunks in zip(group, self.chunker.chunk_texts([f.content for f in group])):
                counts[f.file_path] = len(chunks)  # 0: empty content / no chunks (indexing.py:509-522)
                if self.late and chunks:
                    documents.append((f.content, [str(c.text) for c in chunks]))
                for c in chunks:
                    texts.append(str(c.text) if self.late else c.text)
                    metadatas.append(self._metadata(f, c, len(chunks), indexed_at))

        def drain(everything: bool):
            nonlocal texts, metadatas, counts, documents
            while len(texts) >= self.batch_chunks or (everything and texts):
                take = min(len(texts), self.batch_chunks)
                docs = None
                if self.late:  # files until batch_chunks is reached, never half a file: its chunks share its sequences
                    n_docs = take = 0
                    while n_docs < len(documents) and take < self.batch_chunks:
                        take += len(documents[n_docs][1])
                        n_docs += 1
                    docs, documents = documents[:n_docs], documents[n_docs:]
                last = take == len(texts)
                yield self._tokenise(texts[:take], metadatas[:take], counts if last else {}, docs)
                texts, metadatas = texts[take:], metadatas[take:]
                if last:
                    counts = {}

        for f in files:
            pending.append(f)
            if len(pending) >= self.files_per_cut:
                cut(pending)
                pending = []
                yield from drain(False)
        if pending:
            cut(pending)
        yield from drain(True)
        if counts:  # files that produced no chunk at all after the last batch
            yield _Batch([], [], None, None, None, None, counts, None)

    # ---- the pipeline --------------------------------------------------------------------------------
    def index_files(self, files: Iterable[ParsedFile]) -> dict[str, int]:
        """Index every file; returns {file_path: chunk_count} (0 = nothing to index, the reference's
        ``return False, 0`` cases at indexing.py:509-522). A file's count is reported with the batch that
        holds its last chunk."""
        self.embedder.model  # noqa: B018  load the encoder before the threads start
        if self.semantic:
            return self._index_files_semantic(files)
        q: queue.Queue = queue.Queue(maxsize=2)
        failure: list[BaseException] = []

        def produce():
            try:
                for batch in self._batches(files):
                    q.put(batch)
            except BaseException as exc:  # surfaced on the caller's thread
                failure.append(exc)
            finally:
                q.put(None)

        producer = threading.Thread(target=produce, name="voitta-tokenise", daemon=True)
        producer.start()
        done: dict[str, int] = {}
        try:
            while True:
                batch = q.get()
                if batch is None:
                    break
                if batch.texts:
                    if batch.spans is not None:
                        extra = {"rows": batch.rows} if batch.rows is not None else {}
                        self.vector_store.index_chunks(batch.texts, batch.metadatas, batch.wp_ids, batch.wp_off,
                                                       batch.bm_ids, batch.bm_off, spans=batch.spans, **extra)
                    elif batch.rows is not None:
                        self.vector_store.index_chunks(batch.texts, batch.metadatas, batch.wp_ids, batch.wp_off,
                                                       batch.bm_ids, batch.bm_off, rows=batch.rows)
                    else:
                        self.vector_store.index_chunks(batch.texts, batch.metadatas, batch.wp_ids, batch.wp_off,
                                                       batch.bm_ids, batch.bm_off)
                done.update(batch.counts)
        finally:
            while producer.is_alive():  # unblock a producer stuck on a full queue after an error here
                try:
                    q.get_nowait()
                except queue.Empty:
                    producer.join(0.01)
        if failure:
            raise failure[0]
        return done
