"""Questions as TEXT in one call (vr_query_text_batch, Engine.query_text_batch, VectorStoreService.search_questions):
one forward pass over all questions, whose embeddings stay on the device and feed the filtered batch searches. Row i
must be, bit for bit, what the separate steps give: vr_encode of the same tokenised list, then
vr_search_hybrid_batch_multi (questions with a stem) or vr_search_dense_multi (the others) on those embeddings — and, for
a batch of one, vr_query_text. The checkpoints are synthetic (seeded weights, synthetic vocab.txt)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import bert as obert

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ABSENT = -(2**63)
N_ROWS, N_FOLDERS = 3000, 12

WORDS = ("vector database index retrieval query embedding sparse dense hybrid fusion ranking chunk document folder "
         "search engine kernel memory bandwidth wavefront matrix tile running jumped happily relational the of and "
         "to in is it that was for on are as with they be at one have this from passage").split()
STOP = "the of and to in is it that was for on are as with they be at one have this from".split()

# (hidden, heads): head widths 32 and 64
WIDTHS = [(384, 12), (768, 12), (1024, 16)]
# questions per batch: <= 16 tokens, <= 256 tokens, the mid-size GEMM's range, and (at the FFN widths) the ping-pong one
BATCHES = (1, 12, 150, 1100)


def _vocab():
    v = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + list("abcdefghijklmnopqrstuvwxyz0123456789.,!?:;'-")
    v += ["##" + c for c in "abcdefghijklmnopqrstuvwxyz0123456789"]
    v += WORDS + ["##ing", "##ed", "##s", "##ly", "##tion"]
    return list(dict.fromkeys(v))


def checkpoint(d, hidden, heads, pooling, seed=5, max_seq=32):
    os.makedirs(os.path.join(d, "1_Pooling"), exist_ok=True)
    os.makedirs(os.path.join(d, "2_Normalize"), exist_ok=True)
    vocab = _vocab()
    shape = obert.BertShape(1, hidden, heads, 4 * hidden, vocab=len(vocab), max_pos=64)
    json.dump({"model_type": "bert", "hidden_size": hidden, "num_hidden_layers": 1, "num_attention_heads": heads,
               "intermediate_size": 4 * hidden, "vocab_size": len(vocab), "max_position_embeddings": 64,
               "type_vocab_size": 2, "layer_norm_eps": 1e-12, "hidden_act": "gelu"}, open(os.path.join(d, "config.json"), "w"))
    json.dump([{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
               {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
               {"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}],
              open(os.path.join(d, "modules.json"), "w"))
    json.dump({"word_embedding_dimension": hidden, "pooling_mode_cls_token": pooling == "cls",
               "pooling_mode_mean_tokens": pooling == "mean"}, open(os.path.join(d, "1_Pooling", "config.json"), "w"))
    json.dump({"max_seq_length": max_seq, "do_lower_case": True}, open(os.path.join(d, "sentence_bert_config.json"), "w"))
    open(os.path.join(d, "vocab.txt"), "w", encoding="utf-8").write("\n".join(vocab) + "\n")
    w = obert.random_weights(shape, seed)
    from safetensors.numpy import save_file

    save_file({("bert." + k): v for k, v in w.items()}, os.path.join(d, "model.safetensors"))
    return shape, w


def questions(rng, n):
    """Mixed questions: ordinary ones (some truncated at 32 tokens), stop words only (no stem survives)."""
    out = []
    for i in range(n):
        if i % 9 == 4:
            out.append(" ".join(rng.choice(STOP, size=int(rng.integers(1, 6)))))
        else:
            out.append(" ".join(rng.choice(WORDS, size=int(rng.integers(1, 40)))) + rng.choice(["", "?", " running"]))
    return out


def encode_list(model, texts):
    """vr_encode of the tokenised list (what embed_queries does)."""
    from voitta_rag_amd import encoder as enc

    ids, off = model.tokenize(texts)
    return enc.encode(model.engine, ids, off)


def _model(path, engine):
    from voitta_rag_amd.embedding import NativeSentenceEncoder

    return NativeSentenceEncoder.from_pretrained(path, engine=engine)


def _store(e, model, rng):
    """N_ROWS rows: the embeddings of chunk texts, their BM25 stems, 12 folders, both dates (some absent), deletes."""
    from voitta_rag_amd import bm25

    texts = [" ".join(rng.choice(WORDS, size=int(rng.integers(3, 30)))) for _ in range(N_ROWS)]
    x = encode_list(model, ["passage: " + t for t in texts])
    off, stems = bm25.hashed_stems(texts)
    sp = []
    for i in range(N_ROWS):
        ids, cnt = np.unique(stems[off[i]: off[i + 1]], return_counts=True)
        sp.append((ids.astype(np.int32), (1.0 + np.log1p(cnt)).astype(np.float32)))
    folder = rng.integers(0, N_FOLDERS, size=N_ROWS).astype(np.int32)
    created = rng.integers(0, 4000, size=N_ROWS).astype(np.int64)
    modified = rng.integers(0, 4000, size=N_ROWS).astype(np.int64)
    created[rng.random(N_ROWS) < 0.1] = ABSENT
    for a, b in ((0, 1700), (1700, N_ROWS)):
        e.upsert(x[a:b], sparse=sp[a:b], folder_ids=folder[a:b], created=created[a:b], modified=modified[a:b])
    e.delete_rows(rng.choice(N_ROWS, size=150, replace=False))


def filter_set():
    """Ten filter classes besides "none"."""
    from voitta_rag_amd import SearchFilter as F

    return [None, F(folder_filter=1), F(folder_filter=7), F(include_folders=[2, 5, 9]), F(exclude_folders=[0, 3]),
            F(date_start=1000), F(date_end=500, date_field="created"), F(date_start=100, date_end=2600, include_folders=[1, 4]),
            F(include_folders=[]), F(exclude_folders=list(range(1, N_FOLDERS))), F(folder_filter=9999)]


def make_batch(rng, n):
    texts = questions(rng, n)
    fs = filter_set()
    limits = rng.integers(1, 101, size=n).astype(np.int32)
    limits[rng.random(n) < 0.2] = 10
    weights = rng.choice([0.0, 0.1, 1.0], size=n)
    flt = [fs[int(rng.integers(0, len(fs)))] for _ in range(n)]
    sparse = [t if i % 13 != 6 else None for i, t in enumerate(texts)]  # some questions without a sparse text
    return texts, sparse, limits, weights, flt


def expected(e, emb, sparse, limits, weights, flt, fusion):
    """The separate steps on the same embeddings: the filtered hybrid batch for questions with a stem, the filtered
    dense batch (at the largest limit, trimmed) for the others."""
    from voitta_rag_amd.sparse_embedding import _query_vector

    n = len(limits)
    sq = [_query_vector(s) if s else ([], []) for s in sparse]
    hyb = [i for i in range(n) if len(sq[i][0]) > 0]
    dns = [i for i in range(n) if len(sq[i][0]) == 0]
    out = [None] * n
    if hyb:
        r, s, fd, c = e.search_hybrid_batch_multi(emb[hyb], [(np.array(sq[i][0], np.int32), np.array(sq[i][1], np.float32)) for i in hyb],
                                                  limits[hyb], weights[hyb], [flt[i] for i in hyb], fusion=fusion, raw=True)
        for t, i in enumerate(hyb):
            out[i] = (r[t, : c[t]], s[t, : c[t]], fd[t, : c[t]], True)
    if dns:
        k = int(max(limits[i] for i in dns))
        r, s, c = e.search_dense_multi(emb[dns], k, [flt[i] for i in dns], raw=True)
        for t, i in enumerate(dns):
            m = min(int(c[t]), int(limits[i]))
            out[i] = (r[t, :m], s[t, :m].astype(np.float64), np.ones(m, np.int32), False)
    return out


def same(a, b):
    return (len(a[0]) == len(b[0]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            and np.array_equal(a[2], b[2]) and a[3] == b[3])


@pytest.fixture
def engine(gpu):
    from voitta_rag_amd import Engine

    made = []

    def make(dim):
        e = Engine(dim)
        made.append(e)
        return e

    yield make
    for e in made:
        e.close()


@pytest.mark.parametrize("hidden,heads", WIDTHS)
def test_batch_equals_encode_then_filtered_batches(engine, tmp_path, monkeypatch, hidden, heads):
    monkeypatch.setenv("VOITTA_ENCODER_PRECISION", "f16")
    path = str(tmp_path / "m")
    checkpoint(path, hidden, heads, "mean")
    e = engine(hidden)
    model = _model(path, e)
    rng = np.random.default_rng(hidden)
    _store(e, model, rng)
    for n in BATCHES:
        texts, sparse, limits, weights, flt = make_batch(rng, n)
        dense_texts = ["query: " + t for t in texts]
        want_emb = encode_list(model, dense_texts)
        ids, off = model.tokenize(dense_texts)
        if n == BATCHES[-1]:
            assert int(off[-1]) > 16_000  # (the largest batch reaches the ping-pong kernel's range)
        for fusion in (0, 1):
            got, emb = e.query_text_batch(model.tokenizer._h, dense_texts, sparse, model.max_seq_length, limits, weights,
                                          flt, fusion=fusion, embeddings=True)
            assert np.array_equal(emb, want_emb), n
            want = expected(e, emb, sparse, limits, weights, flt, fusion)
            bad = [i for i in range(n) if not same(got[i], want[i])]
            assert not bad, (n, fusion, bad[:5])
            if n >= 12:
                assert any(g[3] for g in got) and not all(g[3] for g in got)


def test_batch_in_f16x3(engine, tmp_path, monkeypatch):
    monkeypatch.setenv("VOITTA_ENCODER_PRECISION", "f16x3")
    path = str(tmp_path / "m")
    checkpoint(path, 768, 12, "cls")
    e = engine(768)
    model = _model(path, e)
    rng = np.random.default_rng(11)
    _store(e, model, rng)
    for n in (5, 150):
        texts, sparse, limits, weights, flt = make_batch(rng, n)
        dense_texts = ["query: " + t for t in texts]
        got, emb = e.query_text_batch(model.tokenizer._h, dense_texts, sparse, model.max_seq_length, limits, weights, flt,
                                      embeddings=True)
        assert np.array_equal(emb, encode_list(model, dense_texts))
        want = expected(e, emb, sparse, limits, weights, flt, 0)
        assert all(same(got[i], want[i]) for i in range(n))


def test_batch_of_one_equals_query_text(engine, tmp_path, monkeypatch):
    from voitta_rag_amd import SearchFilter as F

    monkeypatch.setenv("VOITTA_ENCODER_PRECISION", "f16")
    path = str(tmp_path / "m")
    checkpoint(path, 384, 12, "mean")
    e = engine(384)
    model = _model(path, e)
    rng = np.random.default_rng(3)
    tok = model.tokenizer._h
    # an empty store first (both branches answer nothing), then the filled one
    for filled in (False, True):
        if filled:
            _store(e, model, rng)
        cases = [("vector search kernel", "vector search kernel", 10, 0.1, 0, None),
                 ("hybrid fusion ranking of the chunk", "hybrid fusion ranking of the chunk", 100, 1.0, 1, F(folder_filter=2)),
                 ("the of and", "the of and", 7, 0.1, 0, None),                       # stop words only: dense branch
                 ("matrix tile wavefront", None, 1, 0.0, 0, F(date_start=1000)),      # no sparse text: dense branch
                 ("matrix tile wavefront", "", 33, 0.1, 1, F(exclude_folders=[1, 2])),
                 ("memory bandwidth", "memory bandwidth", 341, 0.0, 1, F(include_folders=[]))]
        for dense, sparse, limit, w, fusion, f in cases:
            one = e.query_text(tok, "query: " + dense, sparse, model.max_seq_length, limit, w, fusion, f)
            got = e.query_text_batch(tok, ["query: " + dense], [sparse], model.max_seq_length, [limit], [w], [f], fusion=fusion)[0]
            assert same(got, one), (filled, dense, sparse)
            if filled and f is None:
                assert len(one[0]) > 0


_CHILD = r"""
import json, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import test_query_text_batch_gpu as t
from voitta_rag_amd import Engine
jobs = json.load(open(sys.argv[3]))
for job in jobs:
    e = Engine(job["hidden"])
    m = t._model(job["path"], e)
    np.save(job["out"], t.encode_list(m, job["texts"]))
    e.close()
print("ok")
"""


def test_mid_size_gemm_is_bit_identical_to_ping_pong(tmp_path, monkeypatch, gpu):
    """VR_GEMM_MID=0 in a fresh process: the same mid-range batches through the ping-pong kernel alone, for every width
    and for a mean- and a CLS-pooled model; the embeddings must not differ in a single bit."""
    from voitta_rag_amd import Engine

    monkeypatch.setenv("VOITTA_ENCODER_PRECISION", "f16")
    monkeypatch.delenv("VR_GEMM_MID", raising=False)
    rng = np.random.default_rng(17)
    jobs, mine = [], []
    for hidden, heads in WIDTHS:
        for pooling in ("mean", "cls"):
            path = str(tmp_path / f"m{hidden}{pooling}")
            checkpoint(path, hidden, heads, pooling, seed=hidden + len(pooling))
            for n in (40, 300):
                texts = ["query: " + q for q in questions(rng, n)]
                e = Engine(hidden)
                m = _model(path, e)
                ids, off = m.tokenize(texts)
                assert 256 < int(off[-1]) < 16_000
                mine.append(encode_list(m, texts))
                e.close()
                jobs.append({"hidden": hidden, "path": path, "texts": texts, "out": str(tmp_path / f"o{len(jobs)}.npy")})
    spec = tmp_path / "jobs.json"
    spec.write_text(json.dumps(jobs))
    env = dict(os.environ, VR_GEMM_MID="0", VOITTA_ENCODER_PRECISION="f16")
    p = subprocess.run([sys.executable, "-c", _CHILD, HERE, ROOT, str(spec)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    for job, a in zip(jobs, mine):
        b = np.load(job["out"])
        assert np.array_equal(a, b), (job["hidden"], job["path"])


def test_mid_range_batch_against_the_f64_oracle(engine, tmp_path, monkeypatch):
    """One mid-range batch (a few thousand tokens) within test_encoder_gpu.py's f16 tolerance of the f64 oracle."""
    monkeypatch.setenv("VOITTA_ENCODER_PRECISION", "f16")
    path = str(tmp_path / "m")
    shape, w = checkpoint(path, 768, 12, "mean")
    e = engine(768)
    model = _model(path, e)
    rng = np.random.default_rng(23)
    texts = ["query: " + q for q in questions(rng, 200)]
    got, emb = e.query_text_batch(model.tokenizer._h, texts, None, model.max_seq_length, 10, 0.1, [None] * 200,
                                  embeddings=True)
    ids, off = model.tokenize(texts)
    assert 256 < int(off[-1]) < 16_000
    seqs = [ids[off[i]: off[i + 1]] for i in range(len(texts))]
    want = obert.sentence_embeddings(w, shape, seqs, "mean", True, np.float64)
    cos = np.sum(emb.astype(np.float64) * want, axis=1) / (np.linalg.norm(emb, axis=1) * np.linalg.norm(want, axis=1))
    assert np.max(np.abs(1.0 - cos)) < 1e-5
    assert np.max(np.abs(emb - want)) < 5e-4


@pytest.fixture
def native(monkeypatch, tmp_path, gpu):
    from voitta_rag_amd import config, embedding, sparse_embedding, store_registry, vector_store

    path = str(tmp_path / "e5-mini")
    checkpoint(path, 384, 12, "mean")
    monkeypatch.setenv("EMBEDDING_MODEL", path)
    monkeypatch.setenv("EMBEDDING_DIMENSION", "384")
    monkeypatch.setenv("VOITTA_ENCODER_PRECISION", "f16")
    config.get_settings.cache_clear()
    store_registry.reset()
    embedding._embedding_service = None
    sparse_embedding._sparse_embedding_service = None
    vector_store._vector_store = None
    yield
    store_registry.reset()
    config.get_settings.cache_clear()


def test_search_questions_equals_search_requests(native):
    from voitta_rag_amd.embedding import get_embedding_service
    from voitta_rag_amd.sparse_embedding import _query_vector, get_sparse_embedding_service
    from voitta_rag_amd.vector_store import ChunkMetadata, get_vector_store

    rng = np.random.default_rng(5)
    emb, sp, vs = get_embedding_service(), get_sparse_embedding_service(), get_vector_store()
    assert "e5" in emb.model_name.lower()

    def index(fp, folder, n, when):
        texts = [" ".join(rng.choice(WORDS, size=int(rng.integers(3, 30)))) for _ in range(n)]
        metas = [ChunkMetadata(file_path=fp, folder_path=folder, index_folder=folder.split("/")[0], file_name=os.path.basename(fp),
                               chunk_index=i, total_chunks=n, start_char=i, end_char=i + 1, indexed_at="2026-01-01T00:00:00",
                               source_modified_at=when + i) for i in range(n)]
        vs.store_chunks(list(zip(texts, emb.embed_texts(texts), metas)), sparse_vectors=sp.embed_texts(texts))

    def requests(n):
        folders = [None, "docs", "notes", "docs/sub"]
        out = []
        for i, q in enumerate(questions(rng, n)):
            r = {"query": q, "limit": int(rng.choice([0, 1, 5, 10, 40])), "sparse_weight": float(rng.choice([0.0, 0.1, 1.0]))}
            f = folders[i % 4]
            if f:
                r["folder_filter"] = f
            if i % 5 == 2:
                r["date_start"], r["date_field"] = 1_700_000_020, "modified"
            if i % 7 == 3:
                r["exclude_folders"] = ["notes"]
            out.append(r)
        return out

    def check(reqs):
        got = vs.search_questions(reqs)
        vecs = emb.embed_queries([r["query"] for r in reqs])
        ref = vs.search_requests([dict({a: v for a, v in r.items() if a != "query"}, query_embedding=vecs[i],
                                       sparse_query=_query_vector(r["query"])) for i, r in enumerate(reqs)])
        assert len(got) == len(ref) == len(reqs)
        for g, w, r in zip(got, ref, reqs):
            assert [(c.id, c.score) for c in g] == [(c.id, c.score) for c in w], r
        assert any(len(g) for g in got)

    index("docs/a.md", "docs", 60, 1_700_000_000)
    index("notes/b.txt", "notes", 50, 1_700_000_010)
    check(requests(40))
    index("docs/sub/c.md", "docs/sub", 45, 1_700_000_030)  # writes between the calls
    vs.delete_by_file("notes/b.txt")
    check(requests(70))
    index("notes/d.txt", "notes", 30, 1_700_000_050)
    check(requests(1))
    assert vs.search_questions([]) == [] and vs.search_questions([{"query": "vector", "limit": 0}]) == [[]]
