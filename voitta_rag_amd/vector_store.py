"""Drop-in for the reference's VectorStoreService (src/voitta/services/vector_store.py): same
dataclasses, method names, argument meaning, return types and error behaviour. The Qdrant server
behind ``self.client`` is replaced by the in-process engine: vectors, sparse rows and the numeric
filter columns live in HBM; the payload (text + metadata), the UUID <-> row map and the
folder-string dictionaries stay in this host table.

Error convention kept from the reference: store/search/delete/set_file_acl raise; the count_* /
get_* helpers swallow exceptions and return 0 / {} / [] / None (vector_store.py:727,773,812,865,
894,975,1014)."""
from __future__ import annotations

import contextlib
import dataclasses
import json
import logging
import os
import threading
import time
import uuid
from dataclasses import dataclass

import numpy as np

from . import deferred as _deferred
from .config import get_settings
from .engine import VR_TS_ABSENT, SearchFilter
from .sparse_embedding import SPARSE_VECTOR_NAME  # noqa: F401  (re-exported like the reference)
from .store_registry import collection, get_engine
from .store_registry import forget as forget_collection

logger = logging.getLogger(__name__)


@dataclass
class ChunkMetadata:
    """Metadata for a stored chunk (vector_store.py:18-41)."""

    file_path: str
    folder_path: str
    index_folder: str
    file_name: str
    chunk_index: int
    total_chunks: int
    start_char: int
    end_char: int
    indexed_at: str
    start_page: int | None = None
    end_page: int | None = None
    source_page_count: int | None = None
    source_created_at: int | None = None
    source_modified_at: int | None = None
    allowed_users: list[str] | None = None
    source_url: str | None = None


@dataclass
class StoredChunk:
    """A chunk stored in the vector database (vector_store.py:44-51)."""

    id: str
    text: str
    metadata: ChunkMetadata
    score: float | None = None


class _Collection:
    """Host half of one collection: payload rows and string dictionaries."""

    def __init__(self):
        # lock        guards the host table; held for table reads / writes only, NEVER across an engine call —
        #             so searches of several threads overlap in the engine (its search lanes)
        # write_lock  one mutator at a time (store, delete, compact, save); searches do not take it
        # version     bumped by every delete and compaction: a search maps its rows to payloads only if no such
        #             mutation finished in between, else it searches again (its answer then belongs to the later state)
        # generation  the engine generation (row numbering) the table corresponds to
        self.lock = threading.RLock()
        self.write_lock = threading.RLock()
        self.version = 0
        self.generation = 0
        self.ids: list[str | None] = []        # row -> point id (None once deleted)
        self.payload: list[dict | None] = []   # row -> payload dict
        self.row_of: dict[str, int] = {}
        self.rows_by_file: dict[str, list[int]] = {}
        self.folder_ids: dict[str, int] = {}
        self.index_folder_ids: dict[str, int] = {}
        # write-behind (voitta_rag_amd/deferred.py): stores whose rows are in the host table above but whose
        # vectors the engine has not computed yet, oldest first. Guarded by pending_cv; entries are appended
        # under write_lock (so queue order = row order) and consumed by ONE flusher thread.
        self.pending_cv = threading.Condition()
        self.pending: list[dict] = []
        self.pending_rows = 0
        self.flushing = False
        self.enq_seq = 0       # sequence number of the last store queued
        self.done_seq = 0      # ... of the last store the flusher has finished with (stored, or dropped after a failure)
        self.drain_target = 0  # the highest sequence number some caller is waiting for
        self.failed_files: set[str] = set()  # files whose queued rows a failed fused call took back (failed_file_paths)
        self.flusher: threading.Thread | None = None
        self.stopped = False
        self.deferred_error: BaseException | None = None
        self.recovering = False  # the flusher is taking the rows of a failed fused call back out of the host table

    def stop(self) -> None:
        """End the flusher thread; queued stores are dropped (the engine they were meant for is going away)."""
        with self.pending_cv:
            self.stopped = True
            self.pending, self.pending_rows = [], 0
            self.pending_cv.notify_all()
        t = self.flusher
        if t is not None and t is not threading.current_thread():
            t.join(timeout=60)

    def folder_id(self, name: str, create: bool) -> int:
        if name not in self.folder_ids:
            if not create:
                return -1  # never stored: matches no row
            self.folder_ids[name] = len(self.folder_ids)
        return self.folder_ids[name]

    def index_folder_id(self, name: str, create: bool) -> int:
        if name not in self.index_folder_ids:
            if not create:
                return -1
            self.index_folder_ids[name] = len(self.index_folder_ids)
        return self.index_folder_ids[name]

    def live_rows(self):
        return (r for r, p in enumerate(self.payload) if p is not None)


def _json_float(x) -> float:
    """The reference reads scores from Qdrant's REST/JSON replies: an f32 printed with the shortest
    round-tripping decimal, parsed by Python [EXT]."""
    return float(str(np.float32(x)))


class VectorStoreService:
    """Service for storing and retrieving document chunks in the native engine."""

    def __init__(self):
        settings = get_settings()
        self.collection_name = settings.qdrant_collection
        self.dimension = settings.embedding_dimension
        self._client = None
        self._has_sparse: bool = False

    # ---- the "client": engine + host table ------------------------------------------------------
    @property
    def client(self):
        """The engine behind the collection, for callers outside this class: rows whose store was deferred
        (voitta_rag_amd/deferred.py) are in it when this returns."""
        engine = self._engine
        self._drain(collection(self.collection_name, _Collection))
        return engine

    @property
    def _engine(self):
        if self._client is None:
            logger.info("Binding collection '%s' to the native engine", self.collection_name)
            self._client = get_engine()
            try:
                self._ensure_collection()
            except Exception:
                # a saved index that cannot be loaded: nothing half-bound may stay behind (the engine commits a
                # load only when its checksum held, the host table is installed last), so the next call retries
                # from scratch instead of finding a registered-but-empty collection
                self._client = None
                forget_collection(self.collection_name)
                raise
        return self._client

    def _ensure_collection(self) -> None:
        # The reference re-attaches to whatever the Qdrant volume holds (vector_store.py:75-115,
        # docker-compose.yml:8-9); here a saved index under VOITTA_INDEX_DIR is loaded once, when the
        # collection is first bound in this process and the engine is still empty.
        fresh = []

        def factory():
            fresh.append(True)
            return _Collection()

        col = collection(self.collection_name, factory)
        if fresh and hasattr(self._client, "generation"):
            col.generation = self._client.generation()
        index_dir = get_settings().index_dir
        if fresh and index_dir and self.has_saved(index_dir) and self._client.count()[0] == 0:
            self._load_into(col, index_dir)
        self._has_sparse = True  # every collection is created with the "bm25" sparse vector (:95-99,114)

    # ---- compaction -----------------------------------------------------------
    def compact(self, min_dead_fraction: float = 0.0) -> int:
        """Reclaim the rows of deleted points (delete_by_file on re-index, watcher deletes, orphan
        purge: indexing.py:281-288,696-721,886-901) — the role of Qdrant's background optimiser.
        Returns the number of rows dropped; does nothing below ``min_dead_fraction`` tombstones."""
        col = self._col
        with col.write_lock:
            self._drain(col)
            with col.lock:
                total = len(col.ids)
                dead = sum(1 for p in col.payload if p is None)
            if dead == 0 or dead < min_dead_fraction * total:
                return 0
            # the engine builds the compacted tables beside the live ones and swaps them in (searches keep running);
            # between that swap and the renumbering below a search sees a generation mismatch and waits (search())
            remap = self._engine.compact()
            with col.lock:
                ids, payload = [], []
                for pid, p in zip(col.ids, col.payload):
                    if p is not None:
                        ids.append(pid)
                        payload.append(p)
                col.ids, col.payload = ids, payload
                col.row_of = {pid: r for r, pid in enumerate(ids)}
                col.rows_by_file = {}
                for r, p in enumerate(payload):
                    col.rows_by_file.setdefault(p["file_path"], []).append(r)
                assert int((remap >= 0).sum()) == len(ids)
                col.generation = self._engine.generation()
                col.version += 1
            return dead

    # ---- persistence ---------------------------------------------------------
    # On disk a collection is ONE small pointer file, ``<name>.meta.json``, plus the two data files of the
    # generation it names: ``<name>.g<G>.vrindex`` (the device image, Engine.save) and
    # ``<name>.g<G>.payload.jsonl`` (a header line, then one JSON line per row: point id + payload, ``null``
    # for deleted rows). save() writes a NEW generation's data files completely (tmp, fsync, rename), and only
    # then replaces the pointer file (tmp, fsync, rename, directory fsync): the rename of the pointer is the
    # single commit point. A crash or a full disk before it leaves the previous generation untouched and
    # loadable; after it the previous generation's files are deleted. The pointer also records the size and a
    # digest of the index file's header (which holds the checksum of its content) and the payload header repeats
    # the generation, so a load can tell files that do not belong together.
    def _paths(self, directory: str, generation: int | None = None) -> tuple[str, str, str]:
        base = os.path.join(directory, self.collection_name)
        if generation is None:  # format 1 (one fixed name per file), still readable
            return base + ".vrindex", base + ".payload.jsonl", base + ".meta.json"
        return f"{base}.g{generation}.vrindex", f"{base}.g{generation}.payload.jsonl", base + ".meta.json"

    @staticmethod
    def _fsync_dir(directory: str) -> None:
        fd = os.open(directory, os.O_RDONLY)
        try:
            os.fsync(fd)
        finally:
            os.close(fd)

    @staticmethod
    def _write_durably(path: str, write) -> None:
        with open(path + ".tmp", "w", encoding="utf-8") as f:
            write(f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(path + ".tmp", path)

    @staticmethod
    def _index_digest(index_path: str) -> tuple[int, str]:
        import hashlib

        with open(index_path, "rb") as f:
            head = f.read(96)  # FileHeader of csrc/persist.hip: row counts + checksum of everything behind it
        return os.path.getsize(index_path), hashlib.sha256(head).hexdigest()

    def _read_meta(self, directory: str) -> dict | None:
        meta_path = self._paths(directory)[2]
        if not os.path.exists(meta_path):
            return None
        with open(meta_path, encoding="utf-8") as f:
            return json.load(f)

    def has_saved(self, directory: str) -> bool:
        return os.path.exists(self._paths(directory)[2])

    def save(self, directory: str | None = None) -> str:
        """Persist the collection (layout and crash behaviour: comment above). Returns the directory."""
        directory = directory or get_settings().index_dir
        if not directory:
            raise ValueError("no directory given and VOITTA_INDEX_DIR is not set")
        os.makedirs(directory, exist_ok=True)
        col = self._col
        with contextlib.ExitStack() as held:
            held.enter_context(col.write_lock)
            self._drain(col)  # (the flusher needs the table lock only to take rows back after a failure)
            held.enter_context(col.lock)
            try:
                previous = self._read_meta(directory)
            except (OSError, ValueError):
                previous = None  # an unreadable pointer names nothing worth keeping
            generation = int(previous.get("generation", 0)) + 1 if previous else 1
            index_path, payload_path, meta_path = self._paths(directory, generation)
            self._engine.save(index_path)  # tmp + fsync + rename inside vr_save
            index_bytes, index_digest = self._index_digest(index_path)

            def write_payload(f):
                f.write(json.dumps({"format": 2, "generation": generation, "rows": len(col.ids)}) + "\n")
                for pid, payload in zip(col.ids, col.payload):
                    f.write("null\n" if payload is None else json.dumps({"id": pid, "payload": payload}) + "\n")

            self._write_durably(payload_path, write_payload)
            meta = {"format": 2, "generation": generation, "dimension": self.dimension, "rows": len(col.ids),
                    "index_file": os.path.basename(index_path), "payload_file": os.path.basename(payload_path),
                    "index_bytes": index_bytes, "index_header_sha256": index_digest,
                    "folder_ids": col.folder_ids, "index_folder_ids": col.index_folder_ids}
            self._fsync_dir(directory)
            self._write_durably(meta_path, lambda f: json.dump(meta, f))  # <- the commit
            self._fsync_dir(directory)
            # the generation that was live before, and leftovers of saves that never committed
            keep = {os.path.basename(index_path), os.path.basename(payload_path), os.path.basename(meta_path)}
            prefix = self.collection_name + "."
            for name in os.listdir(directory):
                rest = name[len(prefix):] if name.startswith(prefix) else ""
                stale_generation = rest.startswith("g") and rest.split(".", 1)[0][1:].isdigit()
                legacy = rest in ("vrindex", "payload.jsonl")
                if name not in keep and (stale_generation or legacy or rest.endswith(".tmp")):
                    try:
                        os.remove(os.path.join(directory, name))
                    except OSError:
                        pass
        return directory

    def load(self, directory: str | None = None) -> int:
        """Restore a collection written by save() into the (empty) engine; returns the row count."""
        directory = directory or get_settings().index_dir
        if not directory:
            raise ValueError("no directory given and VOITTA_INDEX_DIR is not set")
        col = self._col
        if col.ids:
            raise RuntimeError("collection is not empty")
        return self._load_into(col, directory)

    def _load_into(self, col: _Collection, directory: str) -> int:
        """Fills ``col`` and the engine, or raises and leaves both empty (the engine commits a load only after
        its own checksum held; the host table is built aside and installed last)."""
        meta_path = self._paths(directory)[2]
        meta = self._read_meta(directory)
        if meta is None:
            raise FileNotFoundError(meta_path)
        fmt = meta.get("format")
        if fmt not in (1, 2) or meta.get("dimension") != self.dimension:
            raise ValueError(f"{meta_path}: format/dimension mismatch ({fmt}, {meta.get('dimension')})")
        if fmt == 1:
            index_path, payload_path, _ = self._paths(directory)
        else:
            index_path = os.path.join(directory, meta["index_file"])
            payload_path = os.path.join(directory, meta["payload_file"])
            for path in (index_path, payload_path):
                if not os.path.exists(path):
                    raise ValueError(f"{meta_path} names {os.path.basename(path)}, which is missing")
            if self._index_digest(index_path) != (meta["index_bytes"], meta["index_header_sha256"]):
                raise ValueError(f"{index_path} is not the index file generation {meta['generation']} was saved with")
        ids: list = []
        payloads: list = []
        row_of: dict = {}
        rows_by_file: dict = {}
        with open(payload_path, encoding="utf-8") as f:
            if fmt == 2:
                head = json.loads(f.readline() or "null")
                if not isinstance(head, dict) or head.get("generation") != meta["generation"] or head.get("rows") != meta["rows"]:
                    raise ValueError(f"{payload_path} does not belong to generation {meta['generation']}")
            for line in f:
                rec = json.loads(line)
                row = len(ids)
                if rec is None:
                    ids.append(None)
                    payloads.append(None)
                    continue
                ids.append(rec["id"])
                payloads.append(rec["payload"])
                row_of[rec["id"]] = row
                rows_by_file.setdefault(rec["payload"]["file_path"], []).append(row)
        if len(ids) != meta["rows"]:
            raise ValueError(f"{payload_path}: {len(ids)} rows, the pointer file says {meta['rows']} (truncated?)")
        with col.lock:
            self._client.load(index_path)
            n_rows, _ = self._client.count()
            if n_rows != len(ids):
                raise ValueError(f"{directory}: index holds {n_rows} rows, host table {len(ids)}")
            col.ids, col.payload, col.row_of, col.rows_by_file = ids, payloads, row_of, rows_by_file
            col.folder_ids = {k: int(v) for k, v in meta["folder_ids"].items()}
            col.index_folder_ids = {k: int(v) for k, v in meta["index_folder_ids"].items()}
            col.generation = self._client.generation() if hasattr(self._client, "generation") else 0
            col.version += 1
        logger.info("Loaded %d rows of collection '%s' from %s", len(col.ids), self.collection_name, directory)
        return len(col.ids)

    @property
    def _col(self) -> _Collection:
        self._engine  # noqa: B018  (lazy bind)
        return collection(self.collection_name, _Collection)

    # ---- helpers ----------------------------------------------------------------------------------
    @staticmethod
    def _payload_of(text: str, metadata: ChunkMetadata) -> dict:
        payload = {  # vector_store.py:259-288
            "text": text if type(text) is str else str(text),  # (a LateChunkText is stored as its characters alone)
            "file_path": metadata.file_path,
            "folder_path": metadata.folder_path,
            "index_folder": metadata.index_folder,
            "file_name": metadata.file_name,
            "chunk_index": metadata.chunk_index,
            "total_chunks": metadata.total_chunks,
            "start_char": metadata.start_char,
            "end_char": metadata.end_char,
            "indexed_at": metadata.indexed_at,
        }
        for key in ("start_page", "end_page", "source_page_count", "source_created_at", "source_modified_at",
                    "allowed_users", "source_url"):
            value = getattr(metadata, key)
            if value is not None:
                payload[key] = value
        return payload

    @staticmethod
    def _chunk_from(point_id: str, payload: dict, score) -> StoredChunk:
        return StoredChunk(  # _result_to_chunk, vector_store.py:532-558
            id=str(point_id),
            text=payload["text"],
            metadata=ChunkMetadata(
                file_path=payload["file_path"],
                folder_path=payload["folder_path"],
                index_folder=payload.get("index_folder", payload["folder_path"]),
                file_name=payload["file_name"],
                chunk_index=payload["chunk_index"],
                total_chunks=payload["total_chunks"],
                start_char=payload["start_char"],
                end_char=payload["end_char"],
                indexed_at=payload["indexed_at"],
                start_page=payload.get("start_page"),
                end_page=payload.get("end_page"),
                source_page_count=payload.get("source_page_count"),
                source_created_at=payload.get("source_created_at"),
                source_modified_at=payload.get("source_modified_at"),
                allowed_users=payload.get("allowed_users"),
                source_url=payload.get("source_url"),
            ),
            score=score,
        )

    def _delete_where(self, select) -> int:
        """Delete the live rows ``select(col)`` returns (evaluated under the table lock). Engine first — from then on
        no search returns the rows — then the host table; the version bump makes a search that straddled the two
        steps look again."""
        col = self._col
        with col.write_lock:
            with col.lock:
                rows = [r for r in select(col) if col.payload[r] is not None]
            if not rows:
                # nothing to delete — the common case: IndexingService deletes a file's chunks before it indexes the file,
                # every file, new ones included (indexing.py:281-288). Not waiting for queued rows here is what lets the
                # write-behind batch across files.
                return 0
            self._drain(col)  # the rows to delete may still be on their way into the engine
            with col.lock:   # (a failed flush takes rows back: select again)
                rows = [r for r in select(col) if col.payload[r] is not None]
            if not rows:
                return 0
            self._engine.delete_rows(np.asarray(rows, np.int64))
            with col.lock:
                for r in rows:
                    p = col.payload[r]
                    lst = col.rows_by_file.get(p["file_path"])
                    if lst is not None:
                        lst.remove(r)
                        if not lst:
                            del col.rows_by_file[p["file_path"]]
                    col.row_of.pop(col.ids[r], None)
                    col.payload[r] = None
                    col.ids[r] = None
                col.version += 1
            return len(rows)

    # ---- store ------------------------------------------------------------------------------------
    def store_chunks(self, chunks: list[tuple[str, list[float], ChunkMetadata]],
                     sparse_vectors: list[tuple[list[int], list[float]]] | None = None,
                     batch_size: int = 100) -> list[str]:
        """Store chunks with their embeddings; returns the generated point ids (vector_store.py:233-317).
        ``batch_size`` only bounded HTTP payloads in the reference; rows go to HBM in one append."""
        if not chunks:
            return []
        col = self._col
        n = len(chunks)
        if _deferred.enabled():
            taken = _deferred.take_deferred(chunks, sparse_vectors)
            if taken is not None and chunks[0][1].batch.encoder.engine is self._engine and chunks[0][1].batch.dim == self.dimension:
                if _deferred.write_behind():
                    return self._store_deferred(col, chunks, *taken)
                # the default: the embeddings were never looked at, so they never became Python floats — ONE fused
                # engine call (encode -> BM25 tf -> append) made HERE, failing here if it fails (the reference's
                # upsert raises inside store_chunks and the caller marks the file failed: indexing.py:558-590)
                wp_ids, wp_off, bm_ids, bm_off = taken
                return self.index_chunks([c[0] for c in chunks], [c[2] for c in chunks], np.asarray(wp_ids, np.int32),
                                         np.asarray(wp_off, np.int32), None if bm_off is None else np.asarray(bm_ids, np.int32),
                                         None if bm_off is None else np.asarray(bm_off, np.int64))
        dense = np.asarray([c[1] for c in chunks], dtype=np.float32).reshape(n, self.dimension)
        ids = [str(uuid.uuid4()) for _ in chunks]  # :256
        payloads = [self._payload_of(text, metadata) for text, _emb, metadata in chunks]
        sparse = None
        if sparse_vectors:
            # a chunk beyond len(sparse_vectors) is stored dense-only (:291,299-300): empty row here
            sparse = [sparse_vectors[i] if i < len(sparse_vectors) else ([], []) for i in range(n)]
        created = np.array([VR_TS_ABSENT if c[2].source_created_at is None else int(c[2].source_created_at)
                            for c in chunks], np.int64)
        modified = np.array([VR_TS_ABSENT if c[2].source_modified_at is None else int(c[2].source_modified_at)
                             for c in chunks], np.int64)
        with col.write_lock:
            self._drain(col)  # rows stored before these come before them in the engine too
            first = self._append_host_rows(col, ids, payloads)
            with col.lock:
                folder = np.array([col.folder_id(c[2].folder_path, True) for c in chunks], np.int32)
                ifolder = np.array([col.index_folder_id(c[2].index_folder, True) for c in chunks], np.int32)
            try:  # the host rows exist before the engine can return their row numbers; the engine call holds no table lock
                got = self._engine.upsert(dense, sparse=sparse, folder_ids=folder, index_folder_ids=ifolder,
                                         created=created, modified=modified)
                assert got == first, "host table and engine rows diverged"
            except BaseException:
                self._drop_host_rows(col, first, ids, payloads)
                raise
        logger.info(f"Stored {n} chunks in the native engine")
        return ids

    # ---- write-behind for embeddings that were never looked at (voitta_rag_amd/deferred.py) -----------
    _FLUSH_ROWS = int(os.environ.get("VOITTA_DEFERRED_ROWS", "4096"))        # a batch this large goes at once
    _FLUSH_LINGER_S = float(os.environ.get("VOITTA_DEFERRED_LINGER_MS", "20")) * 1e-3  # a smaller one waits this long for company
    _MAX_PENDING_ROWS = 16 * _FLUSH_ROWS                                      # the caller waits beyond this

    def _store_deferred(self, col: _Collection, chunks, wp_ids, wp_off, bm_ids, bm_off) -> list[str]:
        """store_chunks for chunks whose embeddings are still token ids: the host table gets its rows now, the
        engine gets them from the flusher thread (one vr_index_batch per few thousand chunks)."""
        n = len(chunks)
        ids = [str(uuid.uuid4()) for _ in chunks]  # vector_store.py:256
        payloads = [self._payload_of(text, metadata) for text, _emb, metadata in chunks]
        created = np.array([VR_TS_ABSENT if c[2].source_created_at is None else int(c[2].source_created_at)
                            for c in chunks], np.int64)
        modified = np.array([VR_TS_ABSENT if c[2].source_modified_at is None else int(c[2].source_modified_at)
                             for c in chunks], np.int64)
        with col.pending_cv:
            while col.pending_rows > self._MAX_PENDING_ROWS and not col.stopped and col.deferred_error is None:
                col.pending_cv.wait(0.05)
        with col.write_lock:
            # host rows and queue entry go in together under the queue's lock (order: write_lock, pending_cv, table
            # lock): a failing flush takes back exactly the rows of the entries it finds queued, and a store that
            # arrives while it does so waits
            with col.pending_cv:
                while col.recovering:
                    col.pending_cv.wait(0.05)
                err, col.deferred_error = col.deferred_error, None
                if err is not None:
                    raise RuntimeError("an earlier store_chunks could not be completed by the engine; its rows were dropped") from err
                if col.stopped:
                    raise RuntimeError("the collection was closed")
                first = self._append_host_rows(col, ids, payloads)
                with col.lock:
                    folder = np.array([col.folder_id(c[2].folder_path, True) for c in chunks], np.int32)
                    ifolder = np.array([col.index_folder_id(c[2].index_folder, True) for c in chunks], np.int32)
                col.enq_seq += 1
                entry = dict(engine=self._engine, first=first, n=n, ids=ids, payloads=payloads, t=time.monotonic(), seq=col.enq_seq,
                             wp_ids=np.asarray(wp_ids, np.int32), wp_off=np.asarray(wp_off, np.int64),
                             bm_ids=None if bm_off is None else np.asarray(bm_ids, np.int32),  # None: a dense-only store
                             bm_off=None if bm_off is None else np.asarray(bm_off, np.int64),
                             folder=folder, ifolder=ifolder, created=created, modified=modified)
                col.pending.append(entry)
                col.pending_rows += n
                if col.flusher is None or not col.flusher.is_alive():
                    col.flusher = threading.Thread(target=self._flush_loop, args=(col,), name="voitta-store-flusher", daemon=True)
                    col.flusher.start()
                if col.pending_rows >= self._FLUSH_ROWS:
                    col.pending_cv.notify_all()
        return ids

    @classmethod
    def _flush_loop(cls, col: _Collection) -> None:
        while True:
            with col.pending_cv:
                while not col.stopped:
                    if col.pending and (col.pending_rows >= cls._FLUSH_ROWS or col.pending[0]["seq"] <= col.drain_target
                                        or time.monotonic() - col.pending[0]["t"] >= cls._FLUSH_LINGER_S):
                        break
                    col.pending_cv.wait(cls._FLUSH_LINGER_S if col.pending else None)
                if col.stopped:
                    return
                batch, col.pending, col.pending_rows = col.pending, [], 0
                col.flushing = True
            try:
                cls._flush(col, batch)
            except BaseException as e:  # noqa: BLE001  (reported to the next caller, see _raise_deferred_error)
                logger.error("deferred store of %d chunks failed: %r", sum(b["n"] for b in batch), e)
                with col.pending_cv:
                    later, col.pending, col.pending_rows = col.pending, [], 0
                    col.deferred_error = e
                    col.recovering = True
                try:
                    for b in reversed(batch + later):  # rows that did not reach the engine: taken back, newest first
                        if not b.get("done"):
                            cls._drop_host_rows(col, b["first"], b["ids"], b["payloads"])
                            col.failed_files.update(p["file_path"] for p in b["payloads"])
                finally:
                    with col.pending_cv:
                        col.recovering = False
                        if later:
                            col.done_seq = max(col.done_seq, later[-1]["seq"])
                        col.pending_cv.notify_all()
            finally:
                with col.pending_cv:
                    col.flushing = False
                    col.done_seq = max(col.done_seq, batch[-1]["seq"])
                    col.pending_cv.notify_all()

    @staticmethod
    def _flush(col: _Collection, batch: list[dict]) -> None:
        """One fused engine call per run of consecutive stores of the same kind (with / without sparse vectors: points
        stored without one do not count towards the BM25 statistics, so the two kinds cannot share a call)."""
        engine = batch[0]["engine"]
        a = 0
        while a < len(batch):
            b = a + 1
            while b < len(batch) and (batch[b]["bm_off"] is None) == (batch[a]["bm_off"] is None):
                b += 1
            run = batch[a:b]
            cat = lambda key: run[0][key] if len(run) == 1 else np.concatenate([r[key] for r in run])  # noqa: E731,B023

            def offsets(key):
                if len(run) == 1:  # noqa: B023
                    return run[0][key]  # noqa: B023
                out, base = [run[0][key]], int(run[0][key][-1])  # noqa: B023
                for r in run[1:]:  # noqa: B023
                    out.append(r[key][1:] + base)
                    base += int(r[key][-1])
                return np.concatenate(out)

            sparse = run[0]["bm_off"] is not None
            got = engine.index_batch(cat("wp_ids"), offsets("wp_off").astype(np.int32),
                                     cat("bm_ids") if sparse else None, offsets("bm_off") if sparse else None,
                                     folder_ids=cat("folder"), index_folder_ids=cat("ifolder"),
                                     created=cat("created"), modified=cat("modified"))
            if got != run[0]["first"]:
                raise RuntimeError(f"host table and engine rows diverged ({run[0]['first']} vs {got})")
            for r in run:
                r["done"] = True
            a = b

    @staticmethod
    def _raise_deferred_error(col: _Collection) -> None:
        with col.pending_cv:
            err, col.deferred_error = col.deferred_error, None
        if err is not None:
            raise RuntimeError("an earlier store_chunks could not be completed by the engine; its rows were dropped") from err

    def _drain(self, col: _Collection, surface_errors: bool = True) -> None:
        """Returns when every store_chunks that returned BEFORE this call is in the engine (read-your-writes): the
        queue entries carry sequence numbers and the wait ends when the flusher has finished with the last one that
        was queued on entry — stores queued meanwhile by an indexing thread are not waited for.
        surface_errors=False (search): a failed background store is not this caller's error; it stays recorded for
        the next store_chunks / flush / delete."""
        if col.flusher is None:
            return
        with col.pending_cv:
            target = col.enq_seq
            if col.done_seq < target:
                col.drain_target = max(col.drain_target, target)
                col.pending_cv.notify_all()
                while col.done_seq < target and not col.stopped:
                    col.pending_cv.wait(0.5)
        if surface_errors:
            self._raise_deferred_error(col)

    def failed_file_paths(self, clear: bool = True) -> list[str]:
        """Write-behind only (VOITTA_DEFERRED_INDEXING=1): files whose rows a failed fused store took back out of the
        table after their store_chunks had returned. A caller that keeps its own bookkeeping (the reference commits an
        IndexedFile row per file, indexing.py:558-590) calls flush() and then this before it commits."""
        col = self._col
        with col.pending_cv:
            out = sorted(col.failed_files)
            if clear:
                col.failed_files.clear()
        return out

    def flush(self) -> None:
        """Wait until everything stored so far is searchable (it becomes so by itself within a few ms); raises if a
        queued store failed since the last call (see failed_file_paths)."""
        self._drain(self._col)

    @staticmethod
    def _append_host_rows(col: _Collection, ids: list[str], payloads: list[dict]) -> int:
        with col.lock:
            first = len(col.payload)
            col.ids.extend(ids)
            col.payload.extend(payloads)
            col.row_of.update(zip(ids, range(first, first + len(ids))))
            for i, payload in enumerate(payloads):
                col.rows_by_file.setdefault(payload["file_path"], []).append(first + i)
        return first

    @staticmethod
    def _drop_host_rows(col: _Collection, first: int, ids: list[str], payloads: list[dict]) -> None:
        """Undo _append_host_rows after a failed engine call (nothing else was appended: the write lock is held)."""
        with col.lock:
            del col.ids[first:]
            del col.payload[first:]
            for pid in ids:
                col.row_of.pop(pid, None)
            for i, payload in enumerate(payloads):
                lst = col.rows_by_file.get(payload["file_path"])
                if lst and first + i in lst:
                    lst.remove(first + i)
                    if not lst:
                        del col.rows_by_file[payload["file_path"]]

    @classmethod
    def prepare_rows(cls, texts: list[str], metadatas: list[ChunkMetadata]) -> tuple[list[str], list[dict]]:
        """Point ids and payload dicts of a batch — the pure part of the host table's work. BulkIndexer calls
        it on its producer thread, so that it runs beside the previous batch's GPU call instead of after it."""
        ids = [str(uuid.uuid4()) for _ in texts]  # vector_store.py:256
        return ids, [cls._payload_of(text, metadata) for text, metadata in zip(texts, metadatas)]

    def index_chunks(self, texts: list[str], metadatas: list[ChunkMetadata], wp_ids, wp_off,
                     bm_ids=None, bm_off=None, rows: tuple[list[str], list[dict]] | None = None,
                     spans: tuple | None = None) -> list[str]:
        """The fused form of the three calls of IndexingService._index_file_standard —
        ``embedder.embed_texts`` + ``sparse_embedder.embed_texts`` + ``store_chunks``
        (indexing.py:527-530,560) — for a caller that hands over token ids instead of vectors: WordPiece
        ids (``wp_ids`` / ``wp_off``, [CLS] … [SEP] per chunk) and hashed BM25 stems (``bm_ids`` /
        ``bm_off``, or None for a dense-only store). Encode, tf weighting and the append run in ONE engine
        call (vr_index_batch) and nothing leaves HBM; the stored rows, payloads and scores are those the
        three calls would have produced. Needs the encoder loaded into this store's engine.
        ``rows``: the result of ``prepare_rows`` for this batch, when the caller made it ahead of time.
        ``spans``: (n_seq, span_off, span_tok) of a late-chunking plan — ``wp_ids`` / ``wp_off`` then hold n_seq
        document windows, chunk r is token span r of them, and the call is vr_index_batch_spans."""
        n = len(texts)
        if n == 0:
            return []
        assert len(metadatas) == n
        ids, payloads = rows if rows is not None else self.prepare_rows(texts, metadatas)
        assert len(ids) == n and len(payloads) == n
        col = self._col
        created = np.array([VR_TS_ABSENT if m.source_created_at is None else int(m.source_created_at)
                            for m in metadatas], np.int64)
        modified = np.array([VR_TS_ABSENT if m.source_modified_at is None else int(m.source_modified_at)
                             for m in metadatas], np.int64)
        with col.write_lock:
            self._drain(col)
            first = self._append_host_rows(col, ids, payloads)
            with col.lock:
                folder = np.array([col.folder_id(m.folder_path, True) for m in metadatas], np.int32)
                ifolder = np.array([col.index_folder_id(m.index_folder, True) for m in metadatas], np.int32)
            try:
                if spans is not None:
                    n_seq, span_off, span_tok = spans
                    assert len(wp_off) == n_seq + 1 and len(span_off) == n_seq + 1 and int(span_off[-1]) == n
                    got = self._engine.index_batch_spans(wp_ids, wp_off, span_off, span_tok, bm_ids, bm_off,
                                                         folder_ids=folder, index_folder_ids=ifolder, created=created,
                                                         modified=modified)
                else:
                    got = self._engine.index_batch(wp_ids, wp_off, bm_ids, bm_off, folder_ids=folder,
                                                   index_folder_ids=ifolder, created=created, modified=modified)
                assert got == first, "host table and engine rows diverged"
            except BaseException:
                self._drop_host_rows(col, first, ids, payloads)
                raise
        return ids

    # ---- deletes / ACL ----------------------------------------------------------------------------
    def delete_by_file(self, file_path: str) -> int:
        count = self._delete_where(lambda col: list(col.rows_by_file.get(file_path, [])))
        if count > 0:
            logger.info(f"Deleted {count} chunks for file: {file_path}")
        return count

    def delete_by_folder(self, folder_path: str) -> int:
        count = self._delete_where(lambda col: [r for r in col.live_rows() if col.payload[r]["folder_path"] == folder_path])
        if count > 0:
            logger.info(f"Deleted {count} chunks for folder: {folder_path}")
        return count

    def delete_by_index_folder(self, index_folder: str) -> int:
        count = self._delete_where(lambda col: [r for r in col.live_rows() if col.payload[r].get("index_folder") == index_folder])
        if count > 0:
            logger.info(f"Deleted {count} chunks for index_folder: {index_folder}")
        return count

    def set_file_acl(self, file_path: str, allowed_users: list[str]) -> None:
        col = self._col
        with col.lock:
            for r in col.rows_by_file.get(file_path, []):
                col.payload[r]["allowed_users"] = allowed_users

    # ---- search -----------------------------------------------------------------------------------
    def _build_filter(self, folder_filter: str | None = None, include_folders: list[str] | None = None,
                      exclude_folders: list[str] | None = None, exclude_index_folders: list[str] | None = None,
                      date_start: int | None = None, date_end: int | None = None,
                      date_field: str | None = None) -> SearchFilter | None:
        """Integer form of the Qdrant filter the reference builds (vector_store.py:462-530)."""
        col = self._col
        flt = SearchFilter()
        if folder_filter:
            flt.folder_filter = col.folder_id(folder_filter, False)
        if include_folders:
            flt.include_folders = [col.folder_id(f, False) for f in include_folders]
        if exclude_folders:
            flt.exclude_folders = [i for i in (col.folder_id(f, False) for f in exclude_folders) if i >= 0]
        if exclude_index_folders:
            flt.exclude_index_folders = [i for i in (col.index_folder_id(f, False) for f in exclude_index_folders) if i >= 0]
        if date_start is not None or date_end is not None:
            flt.date_start, flt.date_end, flt.date_field = date_start, date_end, date_field
        return None if flt.is_empty() else flt

    # ---- second-stage reranking (VOITTA_RERANK_MODEL) -----------------------------------------------
    unreranked_searches = 0  # reranking searches answered without it: the question's text was not known

    def _reranker(self):
        path = get_settings().rerank_model
        if not path:
            return None
        from .reranker import get_reranker

        return get_reranker(self._engine, path)

    @staticmethod
    def _rerank(rr, questions: list[str], candidates: list[list[StoredChunk]], limits: list[int]) -> list[list[StoredChunk]]:
        """Every question's candidates rescored in ONE engine call (vr_rerank_text); the best `limit` of each, with
        score = sigmoid(logit), best first (equal scores keep the first stage's order)."""
        logits = rr.logits(questions, [[c.text for c in cands] for cands in candidates])
        return VectorStoreService._rerank_order(candidates, logits, limits)

    @staticmethod
    def _rerank_order(candidates: list[list[StoredChunk]], logits, limits: list[int]) -> list[list[StoredChunk]]:
        """The best `limit` of every list by its logits, score = sigmoid(logit) (equal scores keep the first stage's order)."""
        from .reranker import sigmoid

        out = []
        for cands, lg, limit in zip(candidates, logits, limits):
            scores = sigmoid(lg)
            order = np.argsort(-scores, kind="stable")[:limit]
            out.append([dataclasses.replace(cands[i], score=float(scores[i])) for i in order])
        return out

    # ---- MMR diversification (VOITTA_MMR_DIVERSITY) --------------------------------------------------------
    # The first stage (dense, hybrid, text, batched or reranked) fetches the candidate pool; ONE vr_mmr_select call then
    # picks `limit` of every list of the call, by maximal marginal relevance over the stored rows' similarities. Each
    # chunk keeps its first-stage score and transport, so the scores of an MMR result are not monotone.

    @staticmethod
    def _mmr_spec(limit: int, mmr_diversity, mmr_candidates) -> tuple[float, int] | None:
        """-> None (MMR off) or (diversity, candidates to fetch). None arguments fall back to the settings."""
        settings = get_settings()
        d = settings.mmr_diversity if mmr_diversity is None else mmr_diversity
        if d is None or int(limit) <= 0:
            return None
        d = float(d)
        if not 0.0 <= d <= 1.0:
            raise ValueError(f"mmr_diversity {d} not in [0, 1]")
        from .reranker import rerank_candidates

        c = settings.mmr_candidates if mmr_candidates is None else int(mmr_candidates)
        # d = 0 keeps the first stage's order, so its pool is the limit itself: a hybrid pool's min-max fusion depends on
        # the pool's size, and d = 0 answers exactly what the plain search does
        return d, (int(limit) if d == 0.0 else rerank_candidates(c, int(limit)))

    def _generation(self) -> int:
        return self._engine.generation() if hasattr(self._engine, "generation") else 0

    def _mmr_reorder(self, generation: int, rows: list, scores: list, rels: list, picks: list):
        """picks[j]: None (list j as it is) or (diversity, limit). Lists j with MMR are replaced by their selection, in
        place; False when the engine reports a renumbered index (the rows belong to another numbering)."""
        todo = [j for j, p in enumerate(picks) if p is not None]
        if not todo:
            return True
        pos = self._engine.mmr_select([rows[j] for j in todo], [rels[j] for j in todo], [picks[j][0] for j in todo],
                                      [picks[j][1] for j in todo], generation)
        if pos is None:
            return False
        for j, p in zip(todo, pos):
            rows[j] = np.asarray(rows[j], np.int64)[p]
            scores[j] = [scores[j][i] for i in p]
        return True

    def _mmr_rerank(self, rr, questions: list[str], candidates: list[list[StoredChunk]], limits: list[int],
                    specs: list) -> list[list[StoredChunk]]:
        """The reranked path with MMR: every candidate rescored (one vr_rerank_text call), then, for the lists with a spec,
        MMR over the whole pool with sigmoid(logit) as relevance; the others as _rerank returns them."""
        from .reranker import sigmoid

        logits = rr.logits(questions, [[c.text for c in cands] for cands in candidates])
        scored = [[dataclasses.replace(c, score=float(v)) for c, v in zip(cands, sigmoid(lg))]
                  for cands, lg in zip(candidates, logits)]
        plain = [j for j, spec in enumerate(specs) if spec is None]  # (the lists without MMR: exactly what _rerank returns)
        out: list = [[] for _ in specs]
        for j, res in zip(plain, self._rerank_order([candidates[j] for j in plain], [logits[j] for j in plain],
                                                    [limits[j] for j in plain])):
            out[j] = res
        todo = [j for j, spec in enumerate(specs) if spec is not None and scored[j]]
        if not todo:
            return out
        col = self._col

        def run(_):
            with col.lock:  # the candidates' rows in the numbering of the host table (deleted since: dropped)
                gen = col.generation
                kept = [[i for i, c in enumerate(scored[j]) if c.id in col.row_of] for j in todo]
                rows = [np.asarray([col.row_of[scored[j][i].id] for i in k], np.int64) for j, k in zip(todo, kept)]
            rels = [np.asarray([scored[j][i].score for i in k], np.float64) for j, k in zip(todo, kept)]
            picks = [(specs[j][0], limits[j]) for j in todo]
            if not self._mmr_reorder(gen, rows, kept, rels, picks):
                return None
            return np.zeros(0, np.int64), kept

        _, kept = self._consistent(col, run, lambda: None)
        for j, k in zip(todo, kept):
            out[j] = [scored[j][i] for i in k]
        return out

    def search(self, query_embedding: list[float], limit: int = 10, folder_filter: str | None = None,
               include_folders: list[str] | None = None, exclude_folders: list[str] | None = None,
               exclude_index_folders: list[str] | None = None,
               sparse_query: tuple[list[int], list[float]] | None = None, sparse_weight: float = 0.1,
               date_start: int | None = None, date_end: int | None = None,
               date_field: str | None = None, mmr_diversity: float | None = None,
               mmr_candidates: int | None = None) -> list[StoredChunk]:
        """Dense or hybrid retrieval with the reference's branch selection (vector_store.py:560-619). With
        VOITTA_RERANK_MODEL set: the top VOITTA_RERANK_CANDIDATES of that, reranked by the cross-encoder, the best
        `limit` returned. The question's text comes from the sparse query or from embed_query's result; a bare list
        of floats without either is answered unreranked (counted in ``unreranked_searches``).
        MMR (mmr_diversity, or VOITTA_MMR_DIVERSITY; None = the setting, unset = off): the first stage fetches
        mmr_candidates (VOITTA_MMR_CANDIDATES, clamped to [limit, 341]) — reranked, the rerank candidates, all of them
        rescored — and maximal marginal relevance picks `limit` of them. Every chunk keeps its first-stage
        score: an MMR result's scores are not monotone."""
        args = dict(folder_filter=folder_filter, include_folders=include_folders, exclude_folders=exclude_folders,
                    exclude_index_folders=exclude_index_folders, sparse_query=sparse_query, sparse_weight=sparse_weight,
                    date_start=date_start, date_end=date_end, date_field=date_field)
        spec = self._mmr_spec(limit, mmr_diversity, mmr_candidates)
        rr = self._reranker() if limit > 0 else None
        if rr is None:
            return self._search_mmr_or_plain(query_embedding, limit, spec, args)
        question = getattr(sparse_query, "text", None) if isinstance(sparse_query, _deferred.SparseQueryRef) else None
        if question is None:
            question = getattr(query_embedding, "question", None)
        if question is None:
            VectorStoreService.unreranked_searches += 1
            return self._search_mmr_or_plain(query_embedding, limit, spec, args)
        from .reranker import rerank_candidates

        cands = self._search_first_stage(query_embedding, rerank_candidates(get_settings().rerank_candidates, limit), **args)
        if spec is not None:
            return self._mmr_rerank(rr, [question], [cands], [limit], [spec])[0]
        return self._rerank(rr, [question], [cands], [limit])[0]

    def _search_mmr_or_plain(self, query_embedding, limit: int, spec, args: dict) -> list[StoredChunk]:
        if spec is None:
            return self._search_first_stage(query_embedding, limit, **args)
        return self._search_first_stage(query_embedding, spec[1], mmr=(spec[0], limit), **args)

    def _search_first_stage(self, query_embedding: list[float], limit: int = 10, folder_filter: str | None = None,
                            include_folders: list[str] | None = None, exclude_folders: list[str] | None = None,
                            exclude_index_folders: list[str] | None = None,
                            sparse_query: tuple[list[int], list[float]] | None = None, sparse_weight: float = 0.1,
                            date_start: int | None = None, date_end: int | None = None,
                            date_field: str | None = None, mmr: tuple[float, int] | None = None) -> list[StoredChunk]:
        """mmr: None, or (diversity, final limit): `limit` candidates are fetched and MMR picks the final limit of them."""
        if limit <= 0:
            return []  # Qdrant answers limit=0 with no points (a caller-supplied MCP argument, mcp_server.py:376,474)
        col = self._col
        self._drain(col, surface_errors=False)
        # a question that is still TEXT (embed_query / sparse embed_query results nobody looked at): one engine call
        # does the tokenising, the encode and the search (vr_query_text) — mcp_server.py:469-485 without the Python in between
        if (isinstance(query_embedding, _deferred.QueryRef) and not query_embedding.materialized
                and query_embedding.model.engine is self._engine and _deferred.embedding_width(query_embedding.model.desc) == self.dimension
                and (sparse_query is None or (isinstance(sparse_query, _deferred.SparseQueryRef) and not sparse_query.materialized))):
            model = query_embedding.model
            sparse_text = sparse_query.text if (sparse_query is not None and self._has_sparse) else None

            def run_text(search_filter):
                gen = self._generation()
                rows, scores, _fd, was_hybrid = self._engine.query_text(model.tokenizer, query_embedding.text, sparse_text,
                                                                        model.max_seq_length, limit, sparse_weight, flt=search_filter)
                out = [float(s) for s in scores] if was_hybrid else [_json_float(np.float32(s)) for s in scores]
                rel = np.asarray(scores, np.float64) if was_hybrid else np.asarray(scores, np.float32).astype(np.float64)
                return self._mmr_one(gen, rows, out, rel, mmr)

            rows, scores = self._search_consistent(col, run_text, folder_filter, include_folders, exclude_folders,
                                                   exclude_index_folders, date_start, date_end, date_field)
            return [self._chunk_from(pid, payload, s) for (pid, payload), s in zip(rows, scores) if payload is not None]
        q = self._query_array(query_embedding)
        hybrid = bool(sparse_query and self._has_sparse and sparse_query[0])

        def run(search_filter):
            gen = self._generation()
            if hybrid:
                rows, scores, _ = self._engine.search_hybrid(q, sparse_query[0], sparse_query[1], limit, sparse_weight,
                                                            flt=search_filter)
                return self._mmr_one(gen, rows, [float(s) for s in scores], np.asarray(scores, np.float64), mmr)
            rows, scores = self._engine.search_dense(q[None, :], limit, search_filter)[0]
            rel = np.asarray(scores, np.float32).astype(np.float64)
            return self._mmr_one(gen, rows, [_json_float(s) for s in scores], rel, mmr)

        rows, scores = self._search_consistent(col, run, folder_filter, include_folders, exclude_folders, exclude_index_folders,
                                               date_start, date_end, date_field)
        return [self._chunk_from(pid, payload, s) for (pid, payload), s in zip(rows, scores) if payload is not None]

    def _mmr_one(self, generation: int, rows, scores: list, rel, mmr):
        """(rows, scores) of one first-stage list, MMR-selected when mmr is (diversity, limit); None: look again."""
        if mmr is None:
            return rows, scores
        rows, scores = [rows], [scores]
        if not self._mmr_reorder(generation, rows, scores, [rel], [mmr]):
            return None
        return rows[0], scores[0]

    def _query_array(self, query_embedding) -> np.ndarray:
        """The (D,) f32 query of a search: embed_query's own array when the list was not edited since, else the list."""
        kept = getattr(query_embedding, "array", None) if isinstance(query_embedding, (_deferred.QueryEmbedding, _deferred.QueryRef)) else None
        if isinstance(query_embedding, _deferred.QueryRef):
            return kept.reshape(self.dimension)
        if (kept is not None and len(query_embedding) == kept.size == self.dimension
                and query_embedding[0] == float(kept[0]) and query_embedding[-1] == float(kept[-1])):  # (not edited since)
            return kept.reshape(self.dimension)  # (embed_query's own array; the list was not needed)
        return np.asarray(query_embedding, dtype=np.float32).reshape(self.dimension)

    _SEARCH_DEADLINE_S = float(os.environ.get("VOITTA_SEARCH_DEADLINE_S", "30"))

    def _search_consistent(self, col: _Collection, run, folder_filter, include_folders, exclude_folders, exclude_index_folders,
                           date_start, date_end, date_field):
        """``_consistent`` of one filter built from ``search``'s arguments."""
        return self._consistent(col, run, lambda: self._build_filter(folder_filter, include_folders, exclude_folders,
                                                                     exclude_index_folders, date_start=date_start,
                                                                     date_end=date_end, date_field=date_field))

    def _consistent(self, col: _Collection, run, build):
        """Runs ``run(build()) -> (rows, extra)`` against a consistent pair of engine state and host table and returns
        ([(point id, payload)] for the rows, extra). The engine call holds no Python lock (searches of several threads
        run side by side on the engine's lanes); a delete or a compaction that finished meanwhile (rows gone or
        renumbered) makes the search look again — its answer then belongs to the later state. While a compaction has
        swapped the engine's tables and the host table has not followed yet, the search WAITS (the old index is being
        freed: tens of milliseconds at millions of rows) — up to a deadline of seconds, after which it raises rather
        than return nothing or map rows through a table of another numbering."""
        deadline = time.monotonic() + self._SEARCH_DEADLINE_S
        has_generation = hasattr(self._engine, "generation")
        while True:
            with col.lock:  # (every filter ``build`` makes sees the same dictionaries)
                search_filter = build()
                version, generation = col.version, col.generation
            if has_generation and self._engine.generation() != generation:
                if time.monotonic() > deadline:
                    raise RuntimeError("search: the host table did not catch up with the engine's compaction "
                                       f"within {self._SEARCH_DEADLINE_S:.0f} s")
                time.sleep(0.0005)
                continue
            result = run(search_filter)
            if result is None:  # (an MMR step met a renumbered index: the first stage's rows are of no use)
                if time.monotonic() > deadline:
                    raise RuntimeError(f"search: the collection kept changing for {self._SEARCH_DEADLINE_S:.0f} s")
                continue
            rows, extra = result
            with col.lock:
                unchanged = col.version == version and (not has_generation
                                                        or self._engine.generation() == col.generation == generation)
                if unchanged:
                    flat = np.asarray(rows).reshape(-1).tolist()
                    return [(col.ids[r], col.payload[r]) if 0 <= r < len(col.payload) else (None, None) for r in flat], extra
            if time.monotonic() > deadline:
                raise RuntimeError(f"search: the collection kept changing for {self._SEARCH_DEADLINE_S:.0f} s")

    def search_many(self, query_embeddings, limit: int = 10, folder_filter: str | None = None,
                    include_folders: list[str] | None = None, exclude_folders: list[str] | None = None,
                    exclude_index_folders: list[str] | None = None, sparse_queries=None, sparse_weight: float = 0.1,
                    date_start: int | None = None, date_end: int | None = None,
                    date_field: str | None = None, mmr_diversity: float | None = None,
                    mmr_candidates: int | None = None) -> list[list[StoredChunk]]:
        """``search`` for MANY queries in one engine call (BASELINE configs[4]: 1k batched queries; the MCP search tool
        under load, mcp_server.py:469-485): query_embeddings is (nq, D), sparse_queries a list of (indices, values)
        per query or None. Result i is what ``search(query_embeddings[i], ..., sparse_query=sparse_queries[i])``
        returns — same branch selection per query (vector_store.py:560-619: hybrid only with sparse terms), same
        filters, same scores — but the dense legs share one batched scan, the sparse legs one launch over the inverted
        index, and the fusion of every query runs on the host threads (vr_search_hybrid_batch). MMR as in ``search``:
        every query fetches the candidate pool, one vr_mmr_select call serves them all."""
        q = np.ascontiguousarray(np.asarray(query_embeddings, dtype=np.float32).reshape(-1, self.dimension))
        nq = q.shape[0]
        if limit <= 0 or nq == 0:
            return [[] for _ in range(nq)]
        spec = self._mmr_spec(limit, mmr_diversity, mmr_candidates)
        fetch = limit if spec is None else spec[1]
        col = self._col
        self._drain(col, surface_errors=False)
        sq = list(sparse_queries) if sparse_queries is not None and self._has_sparse else [None] * nq
        assert len(sq) == nq
        sq = [s if s is not None and len(s[0]) > 0 else None for s in sq]
        any_hybrid = any(s is not None for s in sq)

        def run(search_filter):
            gen = self._generation()
            if any_hybrid:
                rows, scores, _fd, counts = self._engine.search_hybrid_batch(q, sq, fetch, sparse_weight, flt=search_filter, raw=True)
            else:
                rows, scores, counts = np.full((nq, fetch), -1, np.int64), np.zeros((nq, fetch)), np.zeros(nq, np.int32)
            # a query without sparse terms takes the dense-only branch (:612-617): `limit` results, raw cosine scores
            dense_only = [i for i in range(nq) if sq[i] is None]
            out_scores = [[float(s) for s in scores[i, : counts[i]]] for i in range(nq)]
            rels = [np.asarray(scores[i, : counts[i]], np.float64) for i in range(nq)]
            if dense_only:
                res = self._engine.search_dense(q[dense_only], fetch, search_filter)
                for i, (r, s) in zip(dense_only, res):
                    counts[i] = len(r)
                    rows[i, : len(r)] = r
                    rows[i, len(r):] = -1
                    out_scores[i] = [_json_float(v) for v in s]
                    rels[i] = np.asarray(s, np.float32).astype(np.float64)
            for i in range(nq):
                rows[i, counts[i]:] = -1
            if spec is not None:
                lists = [rows[i, : counts[i]] for i in range(nq)]
                if not self._mmr_reorder(gen, lists, out_scores, rels, [(spec[0], limit)] * nq):
                    return None
                rows = np.full((nq, limit), -1, np.int64)
                for i in range(nq):
                    counts[i] = len(lists[i])
                    rows[i, : counts[i]] = lists[i]
            return rows, (counts.copy(), out_scores)

        pairs, (counts, scores) = self._search_consistent(col, run, folder_filter, include_folders, exclude_folders,
                                                          exclude_index_folders, date_start, date_end, date_field)
        out = []
        for i in range(nq):
            base = i * limit
            out.append([self._chunk_from(pid, payload, s) for (pid, payload), s in zip(pairs[base: base + int(counts[i])], scores[i])
                        if payload is not None])
        return out

    _FILTER_ARGS = ("folder_filter", "include_folders", "exclude_folders", "exclude_index_folders", "date_start", "date_end",
                    "date_field")

    def search_requests(self, requests: list[dict]) -> list[list[StoredChunk]]:
        """Many independent ``search`` calls in one engine call each for the hybrid and the dense-only ones: requests[i]
        holds the keyword arguments of ``search`` and result i is ``search(**requests[i])`` — its own filter, limit and
        sparse weight, the same branch selection (hybrid only with sparse terms), ``limit <= 0 -> []`` and the same score
        transport. What concurrent MCP ``search`` calls of many users (mcp_server.py:374-485) can share: the dense legs
        scan the corpus once for all filters (vr_search_hybrid_batch_multi / vr_search_dense_multi). Every filter is built
        under one lock, so every request sees the same state of the collection. MMR per request (its keys
        ``mmr_diversity`` / ``mmr_candidates``, None = the settings): those requests fetch their candidate pool, one
        vr_mmr_select call serves them all; the others keep their results as without MMR."""
        n = len(requests)
        out: list[list[StoredChunk]] = [[] for _ in range(n)]
        live = [i for i in range(n) if int(requests[i].get("limit", 10)) > 0]
        if not live:
            return out
        col = self._col
        self._drain(col, surface_errors=False)
        q = np.stack([self._query_array(requests[i]["query_embedding"]) for i in live]).astype(np.float32, copy=False)
        finals = [int(requests[i].get("limit", 10)) for i in live]
        specs = [self._mmr_spec(finals[j], requests[i].get("mmr_diversity"), requests[i].get("mmr_candidates"))
                 for j, i in enumerate(live)]
        limits = [f if sp is None else sp[1] for f, sp in zip(finals, specs)]
        sparse = []
        for i in live:
            sp = requests[i].get("sparse_query")
            sparse.append((sp[0], sp[1]) if (sp and self._has_sparse and sp[0]) else None)
        hyb = [j for j in range(len(live)) if sparse[j] is not None]
        dns = [j for j in range(len(live)) if sparse[j] is None]

        def build():
            return [self._build_filter(**{a: requests[i].get(a) for a in self._FILTER_ARGS}) for i in live]

        def run(filters):
            gen = self._generation()
            rows, scores, rels = [None] * len(live), [None] * len(live), [None] * len(live)
            if hyb:
                r, s, _fd, c = self._engine.search_hybrid_batch_multi(
                    q[hyb], [sparse[j] for j in hyb], [limits[j] for j in hyb],
                    [float(requests[live[j]].get("sparse_weight", 0.1)) for j in hyb], [filters[j] for j in hyb], raw=True)
                for t, j in enumerate(hyb):
                    rows[j] = r[t, : c[t]]
                    scores[j] = [float(v) for v in s[t, : c[t]]]
                    rels[j] = np.asarray(s[t, : c[t]], np.float64)
            if dns:
                k = max(limits[j] for j in dns)  # (exact top-k lists: the first limit of k are the top limit)
                r, s, c = self._engine.search_dense_multi(q[dns], k, [filters[j] for j in dns], raw=True)
                for t, j in enumerate(dns):
                    m = min(int(c[t]), limits[j])
                    rows[j] = r[t, :m]
                    scores[j] = [_json_float(v) for v in s[t, :m]]
                    rels[j] = np.asarray(s[t, :m], np.float32).astype(np.float64)
            picks = [None if sp is None else (sp[0], f) for sp, f in zip(specs, finals)]
            if not self._mmr_reorder(gen, rows, scores, rels, picks):
                return None
            counts = [len(x) for x in rows]
            flat = np.concatenate([np.asarray(x, np.int64) for x in rows])
            return flat, (counts, scores)

        pairs, (counts, scores) = self._consistent(col, run, build)
        at = 0
        for j, i in enumerate(live):
            mine = pairs[at: at + counts[j]]
            at += counts[j]
            out[i] = [self._chunk_from(pid, payload, s) for (pid, payload), s in zip(mine, scores[j]) if payload is not None]
        return out

    def search_questions(self, requests: list[dict]) -> list[list[StoredChunk]]:
        """``search_requests`` for questions still as TEXT, in one engine call (vr_query_text_batch): requests[i] holds
        ``query`` (the raw question) and any keyword argument of ``search`` but the two vectors. Result i is what
        ``search_requests`` returns for it with ``query_embedding = embed_queries(queries)[i]`` and ``sparse_query`` =
        the sparse ``embed_query(query)``: one forward pass over all questions, whose embeddings stay on the device and
        feed the filtered batch searches. What an MCP server that gathers concurrent questions (mcp_server.py:469-485)
        sends. Every filter is built under one lock, as in ``search_requests``. With VOITTA_RERANK_MODEL set: each
        question's candidates as ``search`` fetches them, all reranked in one engine call (vr_rerank_text). MMR per
        request as in ``search_requests`` (after the rerank, over the whole reranked pool, when a reranker is set)."""
        rr = self._reranker()
        if rr is not None and requests:  # first stage at the candidate count, then one rerank call for all questions
            from .reranker import rerank_candidates

            c = get_settings().rerank_candidates
            first = self._search_questions_first_stage(
                [dict({a: v for a, v in r.items() if a not in ("mmr_diversity", "mmr_candidates")},
                      limit=rerank_candidates(c, int(r.get("limit", 10))) if int(r.get("limit", 10)) > 0 else 0)
                 for r in requests])
            limits = [int(r.get("limit", 10)) for r in requests]
            specs = [self._mmr_spec(lim, r.get("mmr_diversity"), r.get("mmr_candidates")) for r, lim in zip(requests, limits)]
            if any(sp is not None for sp in specs):
                return self._mmr_rerank(rr, [r["query"] for r in requests], first, limits, specs)
            return self._rerank(rr, [r["query"] for r in requests], first, limits)
        return self._search_questions_first_stage(requests)

    def _search_questions_first_stage(self, requests: list[dict]) -> list[list[StoredChunk]]:
        from .embedding import get_embedding_service, one_call_text_paths

        n = len(requests)
        out: list[list[StoredChunk]] = [[] for _ in range(n)]
        live = [i for i in range(n) if int(requests[i].get("limit", 10)) > 0]
        if not live:
            return out
        emb = get_embedding_service()
        model = emb.model
        queries = [requests[i]["query"] for i in live]
        if not (one_call_text_paths(model) and model.engine is self._engine
                and _deferred.embedding_width(model.desc) == self.dimension):
            # (an encoder outside this engine: the two services, then search_requests — the definition of the answer)
            from .sparse_embedding import _query_vector

            vecs = emb.embed_queries(queries)
            reqs = []
            for j, i in enumerate(live):
                r = {a: v for a, v in requests[i].items() if a != "query"}
                reqs.append(dict(r, query_embedding=vecs[j], sparse_query=_query_vector(queries[j])))
            res = self.search_requests(reqs)
            for j, i in enumerate(live):
                out[i] = res[j]
            return out
        col = self._col
        self._drain(col, surface_errors=False)
        texts = emb.query_texts(queries)
        sparse_texts = queries if self._has_sparse else None
        finals = [int(requests[i].get("limit", 10)) for i in live]
        specs = [self._mmr_spec(finals[j], requests[i].get("mmr_diversity"), requests[i].get("mmr_candidates"))
                 for j, i in enumerate(live)]
        limits = [f if sp is None else sp[1] for f, sp in zip(finals, specs)]
        weights = [float(requests[i].get("sparse_weight", 0.1)) for i in live]

        def build():
            return [self._build_filter(**{a: requests[i].get(a) for a in self._FILTER_ARGS}) for i in live]

        def run(filters):
            gen = self._generation()
            r, s, _fd, c, hyb = self._engine.query_text_batch(model.tokenizer, texts, sparse_texts, model.max_seq_length,
                                                              limits, weights, filters, raw=True)
            rows = [r[j, : c[j]] for j in range(len(live))]
            scores = [[float(v) for v in s[j, : c[j]]] if hyb[j] else [_json_float(np.float32(v)) for v in s[j, : c[j]]]
                      for j in range(len(live))]
            rels = [np.asarray(s[j, : c[j]], np.float64) if hyb[j] else np.asarray(s[j, : c[j]], np.float32).astype(np.float64)
                    for j in range(len(live))]
            picks = [None if sp is None else (sp[0], f) for sp, f in zip(specs, finals)]
            if not self._mmr_reorder(gen, rows, scores, rels, picks):
                return None
            counts = [len(x) for x in rows]
            flat = np.concatenate([np.asarray(x, np.int64) for x in rows])
            return flat, (counts, scores)

        pairs, (counts, scores) = self._consistent(col, run, build)
        at = 0
        for j, i in enumerate(live):
            mine = pairs[at: at + counts[j]]
            at += counts[j]
            out[i] = [self._chunk_from(pid, payload, s) for (pid, payload), s in zip(mine, scores[j]) if payload is not None]
        return out

    # ---- read helpers (payload only) ---------------------------------------------------------------
    def find_by_source_url(self, source_url: str) -> list[StoredChunk]:
        col = self._col
        with col.lock:
            chunks = [self._chunk_from(col.ids[r], col.payload[r], None) for r in col.live_rows()
                      if col.payload[r].get("source_url") == source_url]
        chunks.sort(key=lambda c: c.metadata.chunk_index)
        return chunks

    def get_file_paths_by_index_folder(self, index_folder: str) -> set[str]:
        col = self._col
        with col.lock:
            return {col.payload[r]["file_path"] for r in col.live_rows() if col.payload[r].get("index_folder") == index_folder}

    def get_collection_info(self) -> dict:
        try:
            n_rows, n_live = self.client.count()
            return {"name": self.collection_name, "vectors_count": n_live, "points_count": n_live, "status": "green"}
        except Exception as e:
            return {"error": str(e)}

    def count_by_file(self, file_path: str) -> int:
        try:
            col = self._col
            with col.lock:
                return len(col.rows_by_file.get(file_path, []))
        except Exception:
            return 0

    def count_chunks_for_files(self, file_paths: list[str]) -> dict[str, int]:
        if not file_paths:
            return {}
        try:
            col = self._col
            with col.lock:
                return {fp: len(col.rows_by_file[fp]) for fp in dict.fromkeys(file_paths) if col.rows_by_file.get(fp)}
        except Exception as e:
            logger.error(f"Error counting chunks for files: {e}")
            return {}

    @staticmethod
    def _in_folder(file_path: str, prefix: str) -> bool:
        return file_path.startswith(prefix) or (not prefix and "/" not in file_path)  # vector_store.py:805

    def count_chunks_for_folder(self, folder_path: str) -> tuple[int, int]:
        try:
            prefix = folder_path + "/" if folder_path else ""
            col = self._col
            with col.lock:
                counts = {fp: len(rows) for fp, rows in col.rows_by_file.items() if self._in_folder(fp, prefix)}
            return len(counts), sum(counts.values())
        except Exception as e:
            logger.error(f"Error counting chunks for folder {folder_path}: {e}")
            return 0, 0

    def get_folder_stats_batch(self, folder_paths: list[str]) -> dict[str, tuple[int, int]]:
        if not folder_paths:
            return {}
        try:
            col = self._col
            out = {}
            with col.lock:
                for fp in folder_paths:
                    prefix = fp + "/" if fp else ""
                    counts = [len(rows) for f, rows in col.rows_by_file.items() if self._in_folder(f, prefix)]
                    out[fp] = (len(counts), sum(counts))
            return out
        except Exception as e:
            logger.error(f"Error getting folder stats batch: {e}")
            return {fp: (0, 0) for fp in folder_paths}

    def get_stored_page_count(self, file_path: str) -> int | None:
        try:
            col = self._col
            with col.lock:
                rows = col.rows_by_file.get(file_path, [])
                if rows and col.payload[rows[0]].get("source_page_count"):
                    return col.payload[rows[0]]["source_page_count"]
            return None
        except Exception as e:
            logger.error(f"Error getting stored page count for {file_path}: {e}")
            return None

    def get_chunks_by_range(self, file_path: str, first_chunk: int, last_chunk: int) -> list[StoredChunk]:
        try:
            col = self._col
            with col.lock:
                chunks = [self._chunk_from(col.ids[r], col.payload[r], None) for r in col.rows_by_file.get(file_path, [])
                          if first_chunk <= col.payload[r]["chunk_index"] <= last_chunk]
            chunks.sort(key=lambda c: c.metadata.chunk_index)
            return chunks
        except Exception as e:
            logger.error(f"Error getting chunks by range for {file_path}: {e}")
            return []

    def get_file_chunk_counts(self, folder_prefix: str = "") -> dict[str, int]:
        try:
            col = self._col
            with col.lock:
                return {fp: len(rows) for fp, rows in col.rows_by_file.items()
                        if not folder_prefix or fp.startswith(folder_prefix)}
        except Exception as e:
            logger.error(f"Error getting file chunk counts: {e}")
            return {}

    def scan_file_stats(self) -> dict[str, dict]:
        """Per-file aggregate over every stored chunk: ``{file_path: {folder_path, index_folder,
        chunk_count, indexed_at}}`` — what the reference's ``scripts/sync_qdrant_stats.py:29-81``
        (``scan_qdrant``) collects by scrolling the whole collection, to re-seed the SQL bookkeeping from
        the index. ``indexed_at`` is that of the file's first stored chunk, as there."""
        col = self._col
        stats: dict[str, dict] = {}
        with col.lock:
            for row in col.live_rows():
                payload = col.payload[row]
                file_path = payload.get("file_path", "")
                entry = stats.get(file_path)
                if entry is None:
                    entry = stats[file_path] = {"folder_path": payload.get("folder_path", ""),
                                                "index_folder": payload.get("index_folder", ""),
                                                "chunk_count": 0, "indexed_at": payload.get("indexed_at")}
                entry["chunk_count"] += 1
        return stats


_vector_store: VectorStoreService | None = None


def get_vector_store() -> VectorStoreService:
    global _vector_store
    if _vector_store is None:
        _vector_store = VectorStoreService()
    return _vector_store
