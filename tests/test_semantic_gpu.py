"""Semantic chunking on the GPU: vr_encode_semantic through the C ABI against tests/semantic_oracle.py.

Four relations hold every call here (``held``): the device's gap distances lie within 2 sqrt(H) TOL of the oracle's; its
unit_start IS the rule replayed in NumPy on its own f32 distances (no tolerance); its chunk count is the starts' sum; and
its rows are the oracle's chunk means taken at the device's starts, at TOL. On the fixtures, whose oracle margins
test_semantic_cpu.py asserts, the starts are the oracle's as well. Then the bit properties, ties, edges, refusals and
services. Every test fails without the feature: the library has no vr_encode_semantic."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import head_oracle as ho
import semantic_case as sc
import semantic_oracle as so
from test_encoder_gpu import PRECISIONS, TOL

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EVERY_GAP = so.Params(buffer=1, break_permille=1000, min_distance=0.0, min_tokens=0)
NO_BREAK = so.Params(buffer=1, break_permille=1000, min_distance=3.0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def held(m, seqs, units, p, precision, got, what, head=None):
    """The four relations of the module docstring for one call's result; returns the device's starts per sequence."""
    rows, start, dist = got
    ids, off, unit_off, unit_tok = sc.pack(seqs, units)
    assert start.shape == dist.shape == (unit_off[-1],) and rows.shape[0] == int(start.sum())
    assert np.array_equal(start, so.replay(dist, unit_off, unit_tok, p)), what  # the decisions, exactly
    bound, worst, want = sc.distance_bound(m.hidden_size, precision), 0.0, []
    for i, (seq, own) in enumerate(zip(seqs, units)):
        lo, hi = int(unit_off[i]), int(unit_off[i + 1])
        if hi == lo:
            continue
        S = so.unit_sums(m.hidden(seq), own)
        d = so.distances(S, p.buffer)
        assert dist[hi - 1] == 0.0
        if len(d):
            worst = max(worst, float(np.max(np.abs(dist[lo:hi - 1] - d))))
        want.append(so.chunk_means(S, [e - b for b, e in own], start[lo:hi]))
    print(f"{what} {precision}: worst |d - oracle| = {worst:.3e} (bound {bound:.3e})")
    assert worst <= bound, what
    if want:
        want = np.concatenate(want)
        want = so.normalized(want) if head is None else ho.apply_head(want, *head)
        norm = np.linalg.norm(want, axis=1, keepdims=True)  # (a truncated row is no unit row: test_head_gpu._check)
        g, w = rows.astype(np.float64) / norm, want / norm
        cos = (g * w).sum(1) / np.linalg.norm(g, axis=1)
        wc, wa = float(np.max(np.abs(1.0 - cos))), float(np.max(np.abs(g - w)))
        print(f"{what} {precision}: {len(rows)} chunk rows, worst |1-cos| = {wc:.3e}, worst abs diff = {wa:.3e}")
        assert wc < TOL[precision][0] and wa < TOL[precision][1], what
    return [start[int(unit_off[i]):int(unit_off[i + 1])] for i in range(len(seqs))]


def call(e, seqs, units, p):
    from voitta_rag_amd import encoder as enc

    return enc.encode_semantic(e, *sc.pack(seqs, units), **p.kwargs())


# ---- the fixtures ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture_run(name, precision):
    fx = sc.BY_NAME[name]
    e = fx.model.engine(precision)
    got = call(e, fx.seqs, fx.units, fx.params)
    e.close()
    return got


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(sc.BY_NAME))
def test_fixture_distances_decisions_and_rows(gpu, name, precision):
    """Every fixture at every precision: distances within the bound, decisions exactly the replayed rule, rows at TOL.
    H 128, 384 and 1024; a causal body; unowned tokens between units; min_tokens / max_tokens; buffer 0 and 1."""
    fx = sc.BY_NAME[name]
    held(fx.model, fx.seqs, fx.units, fx.params, precision, _fixture_run(name, precision), name)


@pytest.mark.parametrize("name,precision", [(f.name, p) for f in sc.FIXTURES for p in f.precisions])
def test_fixture_decisions_are_the_oracles(gpu, name, precision):
    fx = sc.BY_NAME[name]
    _, start, _ = _fixture_run(name, precision)
    want = np.concatenate([s for _, s, _ in fx.oracle()])
    assert np.array_equal(start, want), (name, precision)
    assert 1 < int(want.sum()) < len(want)  # (neither nothing nor everything: the fixture decides something)


# ---- bit properties --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", [None, "labse", "ln_trunc", "trunc"])
@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_every_gap_a_break_gives_encode_spans_bit_for_bit(gpu, precision, head):
    """break_permille 1000, min_tokens 0: every unit is a chunk, and its row the span's — also through a head with
    stages (the means go through enc->pooled and embed_head_kernel) and through a truncation."""
    from voitta_rag_amd import encoder as enc

    fx = sc.BY_NAME["bert128-b0-gaps"]
    m = fx.model
    kw, hd = {}, None
    if head:
        case = ho.CASES[head]
        st = ho.head_weights(case)
        kw, hd = dict(head=ho.stage_objects(st), truncate_dim=case.truncate), (st, True, case.truncate)
    e = m.engine(precision, **kw)
    got = call(e, fx.seqs, fx.units, EVERY_GAP)
    spans = enc.encode_spans(e, *fx.arrays())
    again = call(e, fx.seqs, fx.units, EVERY_GAP)
    e.close()
    assert got[1].all() and got[0].shape == spans.shape == (32, e.encoder_desc.out_dim)
    assert np.array_equal(bits(got[0]), bits(spans)) and np.array_equal(bits(again[0]), bits(spans))
    held(m, fx.seqs, fx.units, EVERY_GAP, precision, got, f"every gap, head {head}", hd)


@pytest.mark.parametrize("head", [None, "two", "ln_trunc"])
def test_chunks_of_several_units_through_a_head(gpu, head):
    """The fixture's own parameters (5 and 3 chunks of 21 and 11 units: rows of units that start nothing lie between
    the head's live rows) against the oracle's means through the f64 head."""
    fx = sc.BY_NAME["bert128-b0-gaps"]
    kw, hd = {}, None
    if head:
        case = ho.CASES[head]
        st = ho.head_weights(case)
        kw, hd = dict(head=ho.stage_objects(st), truncate_dim=case.truncate), (st, True, case.truncate)
    e = fx.model.engine("f32", **kw)
    got = call(e, fx.seqs, fx.units, fx.params)
    e.close()
    starts = held(fx.model, fx.seqs, fx.units, fx.params, "f32", got, f"head {head}", hd)
    assert [int(s.sum()) for s in starts] == [5, 3]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_whole_unit_and_no_break_is_encode_bit_for_bit(gpu, precision):
    """min_distance 3 (no distance reaches it) with one unit [0, len) per sequence on a mean-pooled model: vr_encode's
    rows. And with the fixture's units: one chunk per sequence."""
    from voitta_rag_amd import encoder as enc

    fx = sc.BY_NAME["bert128-b0"]
    whole = [[(0, len(s))] for s in fx.seqs]
    e = fx.model.engine(precision)
    rows, start, dist = call(e, fx.seqs, whole, NO_BREAK)
    plain = enc.encode(e, *fx.arrays()[:2])
    one = call(e, fx.seqs, fx.units, NO_BREAK)
    e.close()
    assert np.array_equal(bits(rows), bits(plain)) and start.tolist() == [1, 1, 1] and not dist.any()
    starts = held(fx.model, fx.seqs, fx.units, NO_BREAK, precision, one, "no break")
    assert [int(s.sum()) for s in starts] == [1, 1, 1]


def test_a_sequence_alone_and_inside_a_batch_has_the_same_bits(gpu):
    """f32: starts, distances and rows of every sequence of a fixture, alone and as a member of the batch."""
    fx = sc.BY_NAME["bert128-b0-tokens"]
    rows, start, dist = _fixture_run(fx.name, "f32")
    e = fx.model.engine("f32")
    r0 = u0 = 0
    for seq, own in zip(fx.seqs, fx.units):
        a_rows, a_start, a_dist = call(e, [seq], [own], fx.params)
        u1, r1 = u0 + len(own), r0 + len(a_rows)
        assert np.array_equal(a_start, start[u0:u1]) and np.array_equal(bits(a_dist), bits(dist[u0:u1]))
        assert np.array_equal(bits(a_rows), bits(rows[r0:r1]))
        u0, r0 = u1, r1
    e.close()
    assert r0 == len(rows) and u0 == len(start)


# ---- ties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("permille", [0, 50, 200, 1000])
def test_ties_break_at_the_lowest_gaps(gpu, precision, permille):
    """A last LayerNorm of zero weight and bias: every hidden row is zero, every d_r exactly 1 (0 / 1e-12 is 0). The
    lowest-index B gaps break — B = 0, 1, 4, 20 of 20 — and the rows are zeros."""
    m = sc.model("bertzero")
    ids, units, _ = sc.planted(21, 4, 0)
    p = so.Params(buffer=1, break_permille=permille)
    e = m.engine(precision)
    rows, start, dist = call(e, [ids], [units], p)
    e.close()
    B = so.break_budget(20, permille)
    assert B == {0: 0, 50: 1, 200: 4, 1000: 20}[permille]
    assert np.array_equal(dist, np.asarray([1.0] * 20 + [0.0], np.float32))
    assert start.tolist() == [1] * (B + 1) + [0] * (20 - B)
    assert rows.shape == (B + 1, 128) and not rows.any()


# ---- edges -----------------------------------------------------------------------------------------------------------------
def _one_token_units(rng, m, lead=1):
    """A sequence of `m` one-token units behind `lead` unowned tokens, and one unowned token behind them."""
    ids = np.concatenate([[1] * lead, rng.integers(3, 64, size=m), [2]]).astype(np.int32)
    return ids, [(lead + r, lead + r + 1) for r in range(m)]


@functools.lru_cache(maxsize=None)
def _unit_counts():
    rng = np.random.default_rng(2048)
    docs = [_one_token_units(rng, m) for m in (0, 1, 2, 3, 64, 65, 2048)]
    return [d[0] for d in docs], [d[1] for d in docs]


@pytest.mark.parametrize("precision,p", [("f32", so.Params(1, 50)), ("f16", so.Params(3, 300, 0.0, 3, 9)),
                                          ("f32", so.Params(0, 1000))])
def test_unit_counts_from_none_to_the_most(gpu, precision, p):
    """m = 0, 1, 2, 3, 64, 65 and 2048 one-token units in one call: B = 0, 0, 1, 1, 4, 4, 103 at 50 permille; the 2048
    fill unit_boundary_kernel's LDS; at permille 1000 all 2183 units are chunks (the row capacity)."""
    m = sc.model("bertlong")
    seqs, units = _unit_counts()
    e = m.engine(precision)
    got = call(e, seqs, units, p)
    e.close()
    starts = held(m, seqs, units, p, precision, got, f"unit counts {p}")
    assert [len(s) for s in starts] == [0, 1, 2, 3, 64, 65, 2048]
    if p.break_permille == 1000 and p.buffer == 0:
        assert got[1].all() and len(got[0]) == 2183


def test_more_buffer_than_units(gpu):
    """buffer 3 with m = 1, 2, 3, 4 (every C_r the sum of all units for m <= 4: every d_r is rounding away from 0), and
    buffer 0 beside it."""
    m = sc.model("bert128")
    docs = [sc.planted(k, 0, 10 + k) for k in (1, 2, 3, 4)]
    seqs, units = [d[0] for d in docs], [d[1] for d in docs]
    e = m.engine("f32")
    for p in (so.Params(3, 1000), so.Params(0, 1000), so.Params(3, 1000, min_distance=1e-3)):
        got = call(e, seqs, units, p)
        held(m, seqs, units, p, "f32", got, f"few units {p}")
        if p.buffer == 3:
            assert float(np.max(np.abs(got[2]))) < 1e-6
            if p.min_distance > 0:
                assert int(got[1].sum()) == 4
    e.close()


def test_the_streamed_attention_route_at_705_tokens(gpu):
    """f16, head size 64: 705 tokens pass the staged attention kernel's 640. Units of 5 tokens across that edge."""
    m = sc.model("rope64")
    rng = np.random.default_rng(705)
    long, short = rng.integers(0, 64, size=705).astype(np.int32), rng.integers(0, 64, size=17).astype(np.int32)
    units = [[(0, 9), (9, 17)], [(1 + 5 * r, 6 + 5 * r) for r in range(140)]]
    p = so.Params(1, 100, min_tokens=10, max_tokens=40)
    e = m.engine("f16")
    got = call(e, [short, long], units, p)
    e.close()
    starts = held(m, [short, long], units, p, "f16", got, "705 tokens")
    assert 18 <= int(starts[1].sum()) <= 70  # (at most 8 units a chunk, at least 2)


def run_chunked(out_path=None):
    """The f32 runs of two fixtures, as a dict of arrays (saved to out_path when given: the child process)."""
    out = {}
    for name in ("bert128-b0", "bert128-b0-gaps"):
        fx = sc.BY_NAME[name]
        for head in (None, "two"):
            kw = {}
            if head:
                case = ho.CASES[head]
                kw = dict(head=ho.stage_objects(ho.head_weights(case)), truncate_dim=case.truncate)
            e = fx.model.engine("f32", **kw)
            rows, start, dist = call(e, fx.seqs, fx.units, fx.params)
            e.close()
            out.update({f"{name} {head} rows": rows, f"{name} {head} start": start, f"{name} {head} dist": dist})
    if out_path:
        np.savez(out_path, **out)
    return out


def test_forward_chunks_share_the_running_chunk_counter(gpu, tmp_path):
    """VR_CHUNK_TOKENS is read when the library is loaded: the same calls in a child process that cuts every batch into
    forward chunks of one sequence each (<= 200 tokens). The chunk rows of a later forward chunk land behind the earlier
    ones' — the counter runs on — and every start, distance and row has the uncut run's bits (f32: the encoder is
    indifferent to the cut, test_head_gpu)."""
    out_path = str(tmp_path / "chunked.npz")
    env = dict(os.environ, VR_CHUNK_TOKENS="200")
    code = (f"import sys; sys.path[:0] = {[os.path.dirname(HERE), HERE]!r}; import test_semantic_gpu as t; "
            f"t.run_chunked({out_path!r})")
    subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=120)
    chunked, whole = np.load(out_path), run_chunked()
    assert sorted(chunked.files) == sorted(whole) and len(whole) == 12
    for key, got in whole.items():
        assert got.shape == chunked[key].shape and np.array_equal(bits(got), bits(chunked[key])), key
    assert len(whole["bert128-b0 None rows"]) == 15 and len(whole["bert128-b0-gaps two rows"]) == 8


def test_a_plain_call_after_a_semantic_one_finds_its_graph(gpu):
    """One 166-token sequence: vr_encode and vr_encode_spans are captured the second time their shape is seen. Semantic
    calls of the same shape in between are never captured and disturb neither: every result has its first call's bits."""
    from voitta_rag_amd import encoder as enc

    fx = sc.BY_NAME["bert128-b0"]
    seq, own = fx.seqs[0], fx.units[0]
    arrays = sc.pack([seq], [own])
    e = fx.model.engine("f16")
    first = (enc.encode(e, *arrays[:2]), enc.encode_spans(e, *arrays), call(e, [seq], [own], fx.params))
    for round_ in range(3):
        for p in (fx.params, EVERY_GAP):
            got = call(e, [seq], [own], p)
            if p is fx.params:
                assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, first[2])), round_
            assert np.array_equal(bits(enc.encode(e, *arrays[:2])), bits(first[0])), round_
            assert np.array_equal(bits(enc.encode_spans(e, *arrays)), bits(first[1])), round_
    e.close()
    held(fx.model, [seq], [own], fx.params, "f16", first[2], "between plain calls")


def test_no_units_and_no_sequences_write_nothing(gpu):
    fx = sc.BY_NAME["bert128-b0"]
    e = fx.model.engine("f16")
    rows, start, dist = call(e, fx.seqs[:2], [[], []], fx.params)
    assert rows.shape == (0, 128) and start.shape == dist.shape == (0,)
    rows, start, dist = e.encode_semantic(np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32),
                                          np.zeros((0, 2), np.int32))
    assert rows.shape == (0, 128) and start.shape == (0,)
    e.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_bad_units_and_parameters_are_refused_and_leave_the_engine_usable(gpu):
    from voitta_rag_amd import EngineError

    m = sc.model("bertlong")
    fx = sc.BY_NAME["bert128-b0-gaps"]
    seqs, good = fx.seqs, fx.units
    e = m.engine("f32")
    want = call(e, seqs, good, fx.params)

    def same():
        got = call(e, seqs, good, fx.params)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, want))

    def units_with(seq, unit, be):
        bad = [list(own) for own in good]
        bad[seq][unit] = be
        return bad

    b2, e2 = good[0][2]
    for seq, unit, be, row, why in ((0, 2, (b2, b2), 2, "empty or outside"),                     # empty
                                    (1, 10, (good[1][10][0], len(seqs[1]) + 1), 31, "empty or outside"),  # past the end
                                    (0, 0, (-1, 3), 0, "empty or outside"),
                                    (0, 2, (good[0][1][1] - 1, e2), 2, "never overlap"),          # overlaps unit 1
                                    (1, 4, good[1][2], 25, "never overlap")):                      # out of order
        with pytest.raises(EngineError, match=rf"sequence {seq} unit {row}\b.*{why}"):
            call(e, seqs, units_with(seq, unit, be), fx.params)
        same()
    rng = np.random.default_rng(9)
    ids, units = _one_token_units(rng, 2049)
    with pytest.raises(EngineError, match=r"sequence 1 has 2049 units \(at most 2048 allowed\)"):
        call(e, [seqs[0], ids], [good[0], units], fx.params)
    same()
    for field, value, msg in (("buffer", 4, "buffer 4 not in 0..3"), ("buffer", -1, "buffer -1 not in 0..3"),
                              ("break_permille", 1001, "break_permille 1001 not in 0..1000"),
                              ("break_permille", -1, "break_permille -1 not in 0..1000"),
                              ("min_tokens", -1, "min_tokens -1 is negative"), ("max_tokens", 0, "max_tokens 0 is below 1"),
                              ("min_distance", float("nan"), "min_distance is not a number")):
        with pytest.raises(EngineError, match=msg):
            e.encode_semantic(*sc.pack(seqs, good), **{**fx.params.kwargs(), field: value})
        same()
    with pytest.raises(EngineError, match="max_tokens 5 is below 1 or below min_tokens 6"):
        e.encode_semantic(*sc.pack(seqs, good), min_tokens=6, max_tokens=5)
    ids, off, unit_off, unit_tok = sc.pack(seqs, good)
    with pytest.raises(EngineError, match=r"unit_off decreases at sequence 1"):
        e.encode_semantic(ids, off, np.array([0, 32, 21], np.int32), unit_tok)
    with pytest.raises(EngineError, match=r"unit_off must start at 0"):
        e.encode_semantic(ids, off, np.array([1, 21, 32], np.int32), unit_tok)
    same()
    e.close()


# ---- services on a synthetic checkpoint directory ------------------------------------------------------------------------
SEMANTIC = {"VOITTA_SEMANTIC_UNIT_CHARS": "80", "VOITTA_SEMANTIC_BUFFER": "1", "VOITTA_SEMANTIC_BREAK_PERMILLE": "200",
            "VOITTA_SEMANTIC_MIN_TOKENS": "8", "VOITTA_SEMANTIC_MAX_TOKENS": "96"}


@pytest.fixture
def services(monkeypatch, tmp_path, gpu):
    """make(name, semantic, cap): fresh services (chunker, embedder, sparse embedder, vector store) on a nomic-shaped
    checkpoint directory, f16, sequences of up to `cap` tokens, VOITTA_SEMANTIC_CHUNKING as given."""
    import itertools
    import uuid

    from test_rope_gpu import nomic_checkpoint

    from voitta_rag_amd import config, embedding, sparse_embedding, store_registry, vector_store

    counter = [itertools.count()]
    monkeypatch.setattr(vector_store.uuid, "uuid4", lambda: uuid.UUID(int=next(counter[0])))  # point ids: run-independent

    def make(name, semantic, cap=512):
        counter[0] = itertools.count()
        path = str(tmp_path / name)
        nomic_checkpoint(path)
        env = {"EMBEDDING_MODEL": path, "EMBEDDING_DIMENSION": "384", "VOITTA_ENCODER_PRECISION": "f16",
               "VOITTA_MAX_SEQ_LENGTH": str(cap), "VOITTA_LATE_CHUNKING": "0"}
        for k, v in {**env, **SEMANTIC}.items():
            monkeypatch.setenv(k, v)
        if semantic:
            monkeypatch.setenv("VOITTA_SEMANTIC_CHUNKING", "1")
        else:
            monkeypatch.delenv("VOITTA_SEMANTIC_CHUNKING", raising=False)
        config.get_settings.cache_clear()
        store_registry.reset()
        embedding._embedding_service = None
        sparse_embedding._sparse_embedding_service = None
        vector_store._vector_store = None
        from voitta_rag_amd.chunking import get_chunking_service
        from voitta_rag_amd.embedding import get_embedding_service
        from voitta_rag_amd.sparse_embedding import get_sparse_embedding_service
        from voitta_rag_amd.vector_store import get_vector_store

        return get_chunking_service(), get_embedding_service(), get_sparse_embedding_service(), get_vector_store()

    yield make
    store_registry.reset()
    config.get_settings.cache_clear()


def _documents():
    from test_late_chunking_gpu import document

    rng = np.random.default_rng(26)
    return [document(rng, 300), document(rng, 1400), "", document(rng, 120), "One sentence alone."]


def _metadata(f, c, total):
    from voitta_rag_amd.vector_store import ChunkMetadata

    return ChunkMetadata(file_path=f.file_path, folder_path=f.folder_path, index_folder=f.index_folder, file_name=f.file_name,
                         chunk_index=c.index, total_chunks=total, start_char=c.start_char, end_char=c.end_char, indexed_at="t",
                         source_modified_at=f.source_modified_at)


def test_services_store_the_chunks_and_rows_of_one_forward_pass(services):
    """chunk_text -> embed_texts -> store_chunks, unmodified, stores exactly the texts and rows of
    chunk_and_embed_documents of the file; BulkIndexer those of chunk_and_embed_documents of its files. The 1400-word
    document goes through in windows of 512 tokens, and no chunk crosses one."""
    from oracle import core as ocore
    from test_late_chunking_gpu import parsed, stored
    from voitta_rag_amd import semantic_chunking as sem
    from voitta_rag_amd.indexer import BulkIndexer

    docs = _documents()
    files = parsed(docs)
    chunker, emb, sp, vs = services("semantic-drop-in", True)
    want_texts, want_rows = [], []
    for f in files:
        (chunks, vectors), = emb.chunk_and_embed_documents([f.content])
        assert vectors.shape == (len(chunks), 384) and [c.index for c in chunks] == list(range(len(chunks)))
        assert all(f.content[c.start_char:c.end_char] == c.text and type(c.text) is sem.SemanticChunkText for c in chunks)
        assert all(a.end_char <= b.start_char for a, b in zip(chunks, chunks[1:]))
        assert "".join("".join(c.text.split()) for c in chunks) == "".join(f.content.split())  # nothing lost or twice
        want_texts += [str(c.text) for c in chunks]
        want_rows.append(vectors)
        cs = chunker.chunk_text(f.content)
        texts = [c.text for c in cs]
        vectors = emb.embed_texts(texts)
        assert type(vectors) is list and (not vectors or type(vectors[0][0]) is float)
        if cs:
            vs.store_chunks([(c.text, v, _metadata(f, c, len(cs))) for c, v in zip(cs, vectors)],
                            sparse_vectors=sp.embed_texts(texts))
    n = [len(r) for r in want_rows]
    assert n[2] == 0 and n[4] == 1 and n[0] > 3 and n[1] > 12 and n[3] > 1
    payloads, ids, dense = stored(vs)
    assert [p["text"] for p in payloads] == want_texts and all(type(p["text"]) is str for p in payloads)
    assert np.array_equal(bits(dense), bits(ocore.cosine_preprocess(np.concatenate(want_rows))))
    # a re-ordered or partial list, or plain strings, are encoded plainly
    cs = chunker.chunk_text(docs[0])
    carried = np.asarray(emb.embed_texts([c.text for c in cs]), np.float32)
    plain = np.asarray(emb.embed_texts([str(c.text) for c in cs]), np.float32)
    assert carried.shape == plain.shape and not np.array_equal(bits(carried), bits(plain))
    for part in ([c.text for c in cs[:2]], [cs[1].text, cs[0].text], [c.text for c in cs] + ["more"]):
        assert np.array_equal(bits(np.asarray(emb.embed_texts(part), np.float32)),
                              bits(np.asarray(emb.embed_texts([str(t) for t in part]), np.float32)))

    chunker, emb, sp, vs = services("semantic-bulk", True)
    results = emb.chunk_and_embed_documents(docs)
    assert [len(c) for c, _ in results] == [len(v) for _, v in results]
    counts = BulkIndexer().index_files(iter(files))
    assert counts == {f.file_path: len(c) for f, (c, _) in zip(files, results)}
    b_payloads, b_ids, b_dense = stored(vs)
    assert [p["text"] for p in b_payloads] == [str(c.text) for cs, _ in results for c in cs]
    assert [(p["chunk_index"], p["start_char"], p["end_char"]) for p in b_payloads] == \
        [(c.index, c.start_char, c.end_char) for cs, _ in results for c in cs]
    assert np.array_equal(bits(b_dense), bits(ocore.cosine_preprocess(np.concatenate([v for _, v in results]))))
    # the sparse side: the chunk texts' BM25 vectors, as the drop-in sequence stores them
    if [p["text"] for p in b_payloads] == want_texts:
        assert b_ids == ids


def test_with_the_flag_unset_nothing_changes(services):
    """Chunks are the character counter's, their texts plain strings, and the stored rows the bits of a plain encode of
    the chunk texts — the fused indexing call's, as before."""
    from oracle import core as ocore
    from test_late_chunking_gpu import parsed, stored
    from voitta_rag_amd.indexer import BulkIndexer

    docs = _documents()
    chunker, emb, sp, vs = services("plain", False)
    chunks = chunker.chunk_texts(docs)
    assert all(type(c.text) is str for cs in chunks for c in cs)
    assert [[(c.text, c.index, c.start_char, c.end_char) for c in cs] for cs in chunks] == \
        [[(c.text, c.index, c.start_char, c.end_char) for c in cs] for cs in chunker.cut(docs)]
    texts = [c.text for cs in chunks for c in cs]
    counts = BulkIndexer().index_files(iter(parsed(docs)))
    assert list(counts.values()) == [len(cs) for cs in chunks]
    payloads, _, dense = stored(vs)
    assert [p["text"] for p in payloads] == texts
    assert np.array_equal(bits(dense), bits(ocore.cosine_preprocess(emb.model.encode(texts))))
