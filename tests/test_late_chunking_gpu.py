"""Late chunking on the GPU: vr_encode_spans / span_pool_kernel and vr_index_batch_spans against the f64
oracles, then the services on a nomic-shaped checkpoint.

The expected value of a span row is ``encode_one(...)[begin:end].mean(0)`` in f64, normalised; the tolerances are the
project's own (test_encoder_gpu.TOL), which test_encoder_rows_gpu already holds single rows of the last layer to."""
import itertools
import uuid

import numpy as np
import pytest

import rope_oracle as ro
from oracle import bert as obert
from oracle import bm25 as obm
from oracle import core as ocore
from test_encoder_gpu import PRECISIONS, TOL

pytestmark = pytest.mark.gpu


# ---- models and oracle ---------------------------------------------------------------------------------------------------
class Model:
    def __init__(self, kind):
        self.kind = kind
        if kind == "bert":
            self.shape = obert.BertShape(2, 128, 2, 256, vocab=64, max_pos=512)
            self.w = obert.random_weights(self.shape, 31)
        else:  # head size 64 (2 heads) or 32 (4 heads)
            self.shape = ro.RopeShape(2, 128, 2 if kind == "rope64" else 4, 256, vocab=64, max_pos=2048)
            self.w = ro.random_weights(self.shape, 32)
        self.memo = {}

    def desc(self, pooling, precision):
        from voitta_rag_amd import encoder as enc

        s = self.shape
        if self.kind == "bert":
            return enc.BertDesc(s.layers, s.hidden, s.heads, s.intermediate, vocab=s.vocab, max_pos=s.max_pos,
                                pooling=pooling, normalize=True, eps=s.eps, precision=precision)
        return ro.desc_for(s, pooling, precision)

    def hidden(self, seq):
        """last_hidden_state of one sequence in f64, computed once."""
        key = np.asarray(seq, np.int32).tobytes()
        if key not in self.memo:
            self.memo[key] = (obert if self.kind == "bert" else ro).encode_one(self.w, self.shape, seq)
        return self.memo[key]

    def want(self, seqs, spans):
        """spans: per sequence a list of (begin, end) -> the f64 rows, in order."""
        rows = []
        for seq, own in zip(seqs, spans):
            for b, e in own:
                v = self.hidden(seq)[b:e].mean(0)
                rows.append(v / max(float(np.sqrt((v * v).sum())), 1e-12))
        return np.stack(rows)

    def engine(self, pooling, precision):
        from voitta_rag_amd import Engine
        from voitta_rag_amd import encoder as enc

        e = Engine(self.shape.hidden)
        enc.load_encoder(e, self.desc(pooling, precision), self.w)
        return e


@pytest.fixture(scope="module")
def models():
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = Model(kind)
        return made[kind]

    return get


def pack(seqs, spans=None):
    ids = np.concatenate(seqs).astype(np.int32)
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    if spans is None:
        return ids, off
    span_off = np.zeros(len(seqs) + 1, np.int32)
    span_off[1:] = np.cumsum([len(s) for s in spans])
    flat = [be for own in spans for be in own]
    return ids, off, span_off, np.asarray(flat, np.int32).reshape(len(flat), 2)


def check(got, want, precision, what):
    cos = (got * want).sum(1) / np.linalg.norm(got, axis=1) / np.linalg.norm(want, axis=1)
    worst, dabs = float(np.max(np.abs(1.0 - cos))), float(np.max(np.abs(got - want)))
    print(f"{what}: {len(got)} rows, worst |1-cos| = {worst:.3e}, worst abs diff = {dabs:.3e}")
    assert worst < TOL[precision][0] and dabs < TOL[precision][1]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


LENS = (1, 17, 65, 33, 129, 300)  # the 33-token sequence has no span: it only provides context


def span_set():
    rng = np.random.default_rng(7)
    seqs = [rng.integers(0, 64, size=n).astype(np.int32) for n in LENS]
    spans = []
    for n in LENS:
        own = [] if n == 33 else [(0, 1), (n - 1, n), (0, n)]
        if n >= 65:
            own += [(3, 40)]
        if n >= 129:
            own += [(20, 70), (60, 70), (3, 40)]  # overlapping; across the 64-key tile; (3, 40) a second time
        if n == 300:
            own += [(120, 135), (250, 300), (200, 260), (130, 131), (5, 9)]  # across the 128-query block; descending order
        spans.append(own)
    return seqs, spans


# ---- the span set ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pooling", ["mean", "cls"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["rope64", "rope32", "bert"])
def test_span_rows_against_the_oracle(gpu, models, kind, precision, pooling):
    """On the [CLS]-pooled description the rows are the same means: the [CLS]-only tail of the last layer is not taken."""
    from voitta_rag_amd import encoder as enc

    m = models(kind)
    seqs, spans = span_set()
    ids, off, span_off, span_tok = pack(seqs, spans)
    assert span_off[3] == span_off[4] and len(span_tok) == span_off[-1] == 29
    e = m.engine(pooling, precision)
    got = enc.encode_spans(e, ids, off, span_off, span_tok)
    e.close()
    assert got.shape == (29, 128)
    check(got, m.want(seqs, spans), precision, f"{kind} {precision} {pooling}")
    rows = {}
    for r, (s, be) in enumerate((s, be) for s, own in enumerate(spans) for be in own):
        if (s, be) in rows:  # the same span twice: the same bits
            assert np.array_equal(bits(got[r]), bits(got[rows[(s, be)]]))
        rows[(s, be)] = r
    assert len(rows) == 25  # (3, 40) twice on two sequences, and the one-token sequence's three spans are one


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("kind", ["rope64", "bert"])
def test_one_whole_span_per_sequence_is_encode_bit_for_bit(gpu, models, kind, precision):
    from voitta_rag_amd import encoder as enc

    m = models(kind)
    seqs, _ = span_set()
    ids, off, span_off, span_tok = pack(seqs, [[(0, len(s))] for s in seqs])
    e = m.engine("mean", precision)
    whole = enc.encode(e, ids, off)
    got = enc.encode_spans(e, ids, off, span_off, span_tok)
    again = e.encode_spans(ids, off, span_off, span_tok)  # (Engine's own method; the second call of a shape is captured)
    e.close()
    assert np.array_equal(bits(got), bits(whole)) and np.array_equal(bits(again), bits(whole))


def test_no_spans_and_no_sequences_write_nothing(gpu, models):
    from voitta_rag_amd import encoder as enc

    m = models("bert")
    seqs, _ = span_set()
    e = m.engine("mean", "f16")
    ids, off, span_off, span_tok = pack(seqs[:2], [[], []])
    assert enc.encode_spans(e, ids, off, span_off, span_tok).shape == (0, 128)
    assert enc.encode_spans(e, ids[:0], np.zeros(1, np.int32), np.zeros(1, np.int32), span_tok).shape == (0, 128)
    e.close()


# ---- the long route --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [("rope64", 700), ("rope32", 1300)])
def test_spans_on_the_streaming_attention_route(gpu, models, kind, n):
    """f16: 700 tokens at head size 64 pass the staged kernel's 640, 1300 at head size 32 its 1280."""
    from voitta_rag_amd import encoder as enc

    m = models(kind)
    edge = 640 if kind == "rope64" else 1280
    rng = np.random.default_rng(n)
    long, short = rng.integers(0, 64, size=n).astype(np.int32), rng.integers(0, 64, size=17).astype(np.int32)
    own = [(0, 1), (edge - 10, edge + 10), (n - 1, n), (0, n)]
    e = m.engine("mean", "f16")
    alone = enc.encode_spans(e, *pack([long], [own]))
    check(alone, m.want([long], [own]), "f16", f"{kind} f16 {n} tokens alone")
    pair = enc.encode_spans(e, *pack([short, long], [[(0, 17), (4, 9)], own]))
    e.close()
    check(pair, m.want([short, long], [[(0, 17), (4, 9)], own]), "f16", f"{kind} f16 {n} tokens beside 17")
    check(pair[2:], alone.astype(np.float64), "f16", f"{kind} f16 {n} tokens: beside 17 against alone")


# ---- the graph cache -------------------------------------------------------------------------------------------------------
def test_graph_cache_keeps_span_calls_and_plain_calls_apart(gpu, models):
    """One 65-token sequence (T <= 1024: its forward pass is captured the second time a shape is seen and replayed from
    then on). Three span lists of one count share a graph — eager, captured, replayed — and the span values are copied
    before every launch, so each call gives its own list's rows; another count and the plain call have graphs of their
    own. Every result carries the bits of the same call made first (eagerly) on a fresh engine."""
    from voitta_rag_amd import encoder as enc

    m = models("rope64")
    seq = np.random.default_rng(65).integers(0, 64, size=65).astype(np.int32)
    lists = [[(0, 65), (3, 40), (64, 65)], [(10, 20), (0, 1), (30, 65)], [(5, 6), (6, 7), (0, 64)], [(2, 50), (60, 65)]]
    ids, off = pack([seq])

    def fresh(call):
        e = m.engine("mean", "f16")
        out = call(e)
        e.close()
        return out

    want_plain = fresh(lambda e: enc.encode(e, ids, off))
    want_spans = [fresh(lambda e: enc.encode_spans(e, *pack([seq], [own]))) for own in lists]  # noqa: B023
    e = m.engine("mean", "f16")
    for round_ in range(2):  # (the second round replays every graph)
        for own, want in zip(lists, want_spans):
            got = enc.encode_spans(e, *pack([seq], [own]))
            assert np.array_equal(bits(got), bits(want)), (round_, own)
            check(got, m.want([seq], [own]), "f16", f"graph cache round {round_} {own}")
            assert np.array_equal(bits(enc.encode(e, ids, off)), bits(want_plain)), (round_, own)
    e.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_bad_spans_are_refused_and_leave_the_engine_usable(gpu, models):
    from voitta_rag_amd import EngineError
    from voitta_rag_amd import encoder as enc

    m = models("bert")
    seqs, _ = span_set()
    seqs = seqs[1:4]  # 17, 65, 33 tokens
    good = [[(0, 17)], [(3, 40), (0, 65)], [(1, 2)]]
    e = m.engine("mean", "f16")
    want = enc.encode_spans(e, *pack(seqs, good))

    def spans_with(seq, span, be):
        bad = [list(own) for own in good]
        bad[seq][span] = be
        return pack(seqs, bad)

    for seq, span, be, row in ((1, 0, (5, 5), 1),       # begin == end
                               (1, 1, (0, 66), 2),      # end > len
                               (0, 0, (-1, 4), 0),      # begin < 0
                               (2, 0, (40, 2), 3)):     # begin > end
        with pytest.raises(EngineError, match=rf"sequence {seq} span {row}\b"):
            enc.encode_spans(e, *spans_with(seq, span, be))
        assert np.array_equal(bits(enc.encode_spans(e, *pack(seqs, good))), bits(want))
    ids, off, span_off, span_tok = pack(seqs, good)
    with pytest.raises(EngineError, match=r"span_off decreases at sequence 1"):
        enc.encode_spans(e, ids, off, np.array([0, 3, 2, 4], np.int32), span_tok)
    with pytest.raises(EngineError, match=r"span_off must start at 0"):
        enc.encode_spans(e, ids, off, np.array([1, 1, 3, 4], np.int32), span_tok)
    assert np.array_equal(bits(enc.encode_spans(e, ids, off, span_off, span_tok)), bits(want))
    # index_batch_spans: n (here: the length of the payload columns) != span_off[n_seq]; a bad span; then a good call
    with pytest.raises(EngineError, match=r"5 rows announced, span_off holds 4 spans"):
        e.index_batch_spans(ids, off, span_off, span_tok, folder_ids=np.zeros(5, np.int32))
    with pytest.raises(EngineError, match=r"sequence 1 span 2\b"):
        e.index_batch_spans(*spans_with(1, 1, (0, 66)))
    assert e.count() == (0, 0)
    assert e.index_batch_spans(ids, off, span_off, span_tok) == 0 and e.count() == (4, 4)
    assert np.array_equal(bits(e.get_dense(np.arange(4))), bits(ocore.cosine_preprocess(want)))
    e.close()


# ---- the fused index call --------------------------------------------------------------------------------------------------
def test_index_batch_spans_stores_what_encode_spans_gives(gpu, models):
    """Three sequences, seven spans, BM25 ids. Dense rows: encode_spans' rows through the cosine preprocessing, bit for bit
    (the relation test_index_gpu pins between vr_index_batch and vr_encode). Sparse rows and payload columns: exactly as
    after index_batch with the same BM25 arrays."""
    from voitta_rag_amd import SearchFilter
    from voitta_rag_amd import encoder as enc

    m = models("rope64")
    rng = np.random.default_rng(3)
    seqs = [rng.integers(0, 64, size=n).astype(np.int32) for n in (40, 9, 120)]
    spans = [[(1, 20), (15, 39)], [(1, 8)], [(1, 30), (30, 60), (60, 119), (100, 119)]]
    texts = ["vector database index", "running kernels happily jumped", "chunk", "sparse dense hybrid fusion ranking",
             "memory bandwidth of the matrix kernel", "the of and", "document folder search engine vector"]
    streams = [obm.hashed_stems(t) for t in texts]
    bm_off = np.zeros(8, np.int64)
    bm_off[1:] = np.cumsum([len(s) for s in streams])
    bm_ids = np.array([t for s in streams for t in s], np.int32)
    cols = dict(folder_ids=np.array([0, 0, 1, 2, 2, 2, 1], np.int32), index_folder_ids=np.array([0, 0, 1, 1, 1, 1, 1], np.int32),
                created=np.arange(7, dtype=np.int64) + 1_700_000_000, modified=np.arange(7, dtype=np.int64) * 10 + 1_710_000_000)
    ids, off, span_off, span_tok = pack(seqs, spans)

    a = m.engine("mean", "f16")
    assert a.index_batch_spans(ids, off, span_off, span_tok, bm_ids, bm_off, **cols) == 0 and a.count() == (7, 7)
    rows = enc.encode_spans(a, ids, off, span_off, span_tok)
    check(rows, m.want(seqs, spans), "f16", "index_batch_spans rows")
    assert np.array_equal(bits(a.get_dense(np.arange(7))), bits(ocore.cosine_preprocess(rows)))
    assert a.index_batch_spans(ids, off, span_off, span_tok, bm_ids, bm_off, **cols) == 7  # appended behind them
    assert np.array_equal(bits(a.get_dense(np.arange(7, 14))), bits(ocore.cosine_preprocess(rows)))

    b = m.engine("mean", "f16")  # the plain call: seven sequences of their own, the same BM25 arrays and columns
    plain = [rng.integers(0, 64, size=12).astype(np.int32) for _ in range(7)]
    for _ in range(2):
        b.index_batch(*pack(plain), bm_ids, bm_off, **cols)
    filters = [None, SearchFilter(folder_filter=2), SearchFilter(include_folders=[0, 1]), SearchFilter(exclude_index_folders=[0]),
               SearchFilter(date_start=1_700_000_002, date_end=1_700_000_005, date_field="created"),
               SearchFilter(date_start=1_710_000_020, date_field="modified")]
    asked = 0
    for q in ("vector database", "running kernel", "fusion ranking of documents", "chunk"):
        qi, qv = obm.query_embed(q)
        for flt in filters:
            gr, gs = a.search_sparse(qi, qv, 10, flt)
            wr, ws = b.search_sparse(qi, qv, 10, flt)
            assert np.array_equal(gr, wr) and np.array_equal(gs, ws)
            asked += len(gr)
    assert asked > 40
    # the dense side sees the same payload columns: a filtered dense search returns rows of the filter only
    r, _ = a.search_dense(rows[3], 14, SearchFilter(folder_filter=2))[0]
    assert sorted(np.asarray(r).ravel().tolist()) == [3, 4, 5, 10, 11, 12]
    a.close()
    b.close()


# ---- services --------------------------------------------------------------------------------------------------------------
WORDS = ("vector database index retrieval query embedding sparse dense hybrid fusion ranking chunk document folder "
         "search engine kernel memory bandwidth wavefront matrix tile running jumped happily relational").split()


def document(rng, n_words):
    out, n = [], 0
    while n < n_words:
        sents = []
        for _ in range(int(rng.integers(2, 6))):
            k = int(rng.integers(4, 15))
            sents.append(" ".join(rng.choice(WORDS, size=k)) + rng.choice([".", "!", "?"]))
            n += k
        out.append(" ".join(sents))
    return "\n\n".join(out)


@pytest.fixture
def nomic(monkeypatch, tmp_path, gpu):
    from test_rope_gpu import nomic_checkpoint

    from voitta_rag_amd import config, embedding, sparse_embedding, store_registry, vector_store

    counter = [itertools.count()]
    monkeypatch.setattr(vector_store.uuid, "uuid4", lambda: uuid.UUID(int=next(counter[0])))  # point ids: run-independent

    def make(name, late, cap):
        counter[0] = itertools.count()
        path = str(tmp_path / name)
        made = nomic_checkpoint(path)
        for k, v in (("EMBEDDING_MODEL", path), ("EMBEDDING_DIMENSION", "384"), ("VOITTA_ENCODER_PRECISION", "f16"),
                     ("VOITTA_MAX_SEQ_LENGTH", str(cap)), ("VOITTA_LATE_CHUNKING", "1" if late else "0")):
            monkeypatch.setenv(k, v)
        config.get_settings.cache_clear()
        store_registry.reset()
        embedding._embedding_service = None
        sparse_embedding._sparse_embedding_service = None
        vector_store._vector_store = None
        from voitta_rag_amd.chunking import get_chunking_service
        from voitta_rag_amd.embedding import get_embedding_service
        from voitta_rag_amd.sparse_embedding import get_sparse_embedding_service
        from voitta_rag_amd.vector_store import get_vector_store

        return made, get_chunking_service(), get_embedding_service(), get_sparse_embedding_service(), get_vector_store()

    yield make
    store_registry.reset()
    config.get_settings.cache_clear()


def parsed(docs):
    from voitta_rag_amd.indexer import ParsedFile

    return [ParsedFile(content=d, file_path=f"docs/{i}.md", folder_path="docs", index_folder="docs", file_name=f"{i}.md",
                       source_modified_at=1_710_000_000 + i) for i, d in enumerate(docs)]


def stored(vs):
    col = vs._col
    return ([{k: v for k, v in p.items() if k != "indexed_at"} for p in col.payload], list(col.ids) if hasattr(col, "ids") else None,
            vs.client.get_dense(np.arange(len(col.payload))))


def test_services_embed_and_index_chunks_in_the_context_of_their_documents(nomic):
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd import late_chunking as lc
    from voitta_rag_amd.indexer import BulkIndexer
    from voitta_rag_amd.vector_store import ChunkMetadata

    rng = np.random.default_rng(15)
    docs = [document(rng, 1400), document(rng, 200)]
    # one chunk text placed in two documents (hand-cut chunk lists: the chunker's overlap tails would tell them apart)
    shared = "The hybrid fusion ranking of sparse and dense retrieval was raised to 32 in the next release."
    x, y, z = document(rng, 150), document(rng, 40), document(rng, 90)
    placed = [(x + "\n\n" + shared + "\n\n" + y, [x, shared, y]), (shared + "\n\n" + z, [shared, z])]

    def cos_of_shared(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return float(a @ b / np.sqrt((a @ a) * (b @ b)))

    # the setting on, sequences of up to 2048 tokens: BulkIndexer
    _, chunker, emb, sp, vs = nomic("late-bulk", True, 2048)
    model = emb.model
    assert model.max_seq_length == 2048
    chunks = [[c.text for c in cs] for cs in chunker.chunk_texts(docs)]
    assert all(type(t) is lc.LateChunkText for cs in chunks for t in cs) and len(chunks[0]) > 10
    plan = lc.plan(docs[0], chunks[0], model.tokenize, 2048, 256)
    assert plan.n_seq == 1 and 1400 <= int(plan.offsets[-1]) <= 2048 and not plan.truncated.any()
    one = emb.embed_document(docs[0], [str(t) for t in chunks[0]])
    assert type(one) is list and type(one[0][0]) is float
    direct = enc.encode_spans(model.engine, plan.ids, plan.offsets, plan.span_off, plan.span_tok)
    assert np.array_equal(bits(np.asarray(one, np.float32)), bits(direct))
    both = np.asarray(emb.embed_documents([(d, [str(t) for t in cs]) for d, cs in zip(docs, chunks)]), np.float32)
    rows_a, rows_b = emb.embed_document(*placed[0]), emb.embed_document(*placed[1])
    late_cos = cos_of_shared(rows_a[1], rows_b[0])
    print(f"one chunk text in two documents, late chunking on: |1 - cos| = {abs(1 - late_cos):.3e}")
    assert abs(1 - late_cos) > TOL["f16"][0]  # two vectors: further apart than the arithmetic's own error
    counts = BulkIndexer().index_files(iter(parsed(docs)))
    assert counts == {"docs/0.md": len(chunks[0]), "docs/1.md": len(chunks[1])}
    late_payloads, late_ids, late_dense = stored(vs)
    assert np.array_equal(bits(late_dense), bits(ocore.cosine_preprocess(both)))

    # the setting on: the per-file drop-in sequence chunk_text -> embed_texts -> store_chunks
    _, chunker, emb, sp, vs = nomic("late-drop-in", True, 2048)
    for f in parsed(docs):
        cs = chunker.chunk_text(f.content)
        texts = [c.text for c in cs]
        vectors = emb.embed_texts(texts)
        assert type(vectors) is list and type(vectors[0]) is list  # plain floats at once, no deferred references
        vs.store_chunks([(c.text, v, ChunkMetadata(
            file_path=f.file_path, folder_path=f.folder_path, index_folder=f.index_folder, file_name=f.file_name,
            chunk_index=c.index, total_chunks=len(cs), start_char=c.start_char, end_char=c.end_char, indexed_at="t",
            source_modified_at=f.source_modified_at)) for c, v in zip(cs, vectors)], sparse_vectors=sp.embed_texts(texts))
    drop_payloads, drop_ids, drop_dense = stored(vs)
    assert drop_payloads == late_payloads and drop_ids == late_ids and all(type(p["text"]) is str for p in drop_payloads)
    check(drop_dense, late_dense.astype(np.float64), "f16", "drop-in sequence against BulkIndexer")

    # the setting off: same texts, payloads and point ids; the shared chunk's two vectors are one
    _, chunker, emb, sp, vs = nomic("plain-bulk", False, 2048)
    assert all(type(c.text) is str for cs in chunker.chunk_texts(docs) for c in cs)
    assert BulkIndexer().index_files(iter(parsed(docs))) == counts
    plain_payloads, plain_ids, plain_dense = stored(vs)
    assert plain_payloads == late_payloads and plain_ids == late_ids
    off_cos = cos_of_shared(np.asarray(emb.embed_texts(placed[0][1]))[1], np.asarray(emb.embed_texts(placed[1][1]))[0])
    print(f"one chunk text in two documents, late chunking off: |1 - cos| = {abs(1 - off_cos):.3e}")
    assert abs(1 - off_cos) < TOL["f16"][0]
    worst = float(np.min((plain_dense * late_dense).sum(1)))
    print(f"stored rows, late chunking on against off: smallest cos = {worst:.6f}")
    assert 1 - worst > TOL["f16"][0]  # ... and late chunking did change the stored vectors


def test_a_document_longer_than_the_window_at_the_default_cap(nomic):
    """Cap 512: the ~1500-token document becomes as many sequences as the plan says, each at most 512 tokens, and every
    chunk's row is the oracle's mean over its span of its own window."""
    from voitta_rag_amd import late_chunking as lc

    rng = np.random.default_rng(16)
    doc = document(rng, 1400)
    (shape, w, _), chunker, emb, _, _ = nomic("late-512", True, 512)
    model = emb.model
    assert model.max_seq_length == 512
    chunks = [str(c.text) for c in chunker.chunk_text(doc)]
    plan = lc.plan(doc, chunks, model.tokenize, 512, 256)
    assert plan.n_seq >= 4 and int(np.diff(plan.offsets).max()) <= 512 and plan.n_chunks == len(chunks)
    assert np.all(np.diff(plan.span_off) >= 1) and not plan.truncated.any()
    same = model.plan_documents([(doc, chunks)])
    assert np.array_equal(same.ids, plan.ids) and np.array_equal(same.span_tok, plan.span_tok) and same.n_seq == plan.n_seq
    got = np.asarray(emb.embed_document(doc, chunks), np.float32)
    want = []
    for s in range(plan.n_seq):
        hidden = ro.encode_one(w, shape, plan.ids[plan.offsets[s]:plan.offsets[s + 1]])
        for b, e in plan.span_tok[plan.span_off[s]:plan.span_off[s + 1]].tolist():
            v = hidden[b:e].mean(0)
            want.append(v / np.sqrt((v * v).sum()))
    check(got, np.stack(want), "f16", f"{plan.n_seq} windows of a {int(plan.offsets[-1])}-token document")
