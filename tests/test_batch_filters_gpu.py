"""Filtered batches (vr_search_dense_multi, vr_search_hybrid_batch_multi, VectorStoreService.search_requests): every
query of a batch carries its own filter, limit and sparse weight, and row i must be, bit for bit, what the single call
with query i's own arguments returns, and what the CPU oracle ranks. The caller that batches like this is the MCP search
tool under multi-user load (reference: mcp_server.py:374-485; the filter: vector_store.py:462-530)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import core as ocore
from oracle import fusion as ofus

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ABSENT = -(2**63)
N, DIM, VOCAB, N_FOLDERS, N_IFOLDERS = 20_000, 128, 600, 12, 4


def build_small(seed=2027):
    """20,000 rows x 128 (above the 16,384 rows the integer-GEMM dense batch needs) in several upsert batches, deletes,
    12 folders, 4 index folders, both timestamps with some absent. Returns the engine and the host copy."""
    from voitta_rag_amd import Engine

    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, DIM)).astype(np.float32)
    sp = []
    for _ in range(N):
        m = int(rng.integers(0, 30))
        ids = np.sort(rng.choice(VOCAB, size=m, replace=False)).astype(np.int32) * 7919 + 13
        sp.append((ids, rng.uniform(0.2, 2.2, size=m).astype(np.float32)))
    folder = rng.integers(0, N_FOLDERS, size=N).astype(np.int32)
    ifolder = rng.integers(0, N_IFOLDERS, size=N).astype(np.int32)
    created = rng.integers(0, 4000, size=N).astype(np.int64)
    modified = rng.integers(0, 4000, size=N).astype(np.int64)
    created[rng.random(N) < 0.1] = ABSENT
    modified[rng.random(N) < 0.15] = ABSENT
    e = Engine(DIM)
    for a, b in ((0, 7000), (7000, 7013), (7013, 16000), (16000, N)):
        e.upsert(x[a:b], sparse=sp[a:b], folder_ids=folder[a:b], index_folder_ids=ifolder[a:b], created=created[a:b],
                 modified=modified[a:b])
    dead = rng.choice(N, size=700, replace=False)
    e.delete_rows(dead)
    live = np.ones(N, bool)
    live[dead] = False
    return e, dict(x=x, sp=sp, folder=folder, ifolder=ifolder, created=created, modified=modified, live=live)


def classes(h):
    """About 40 distinct filters: none, folder_filter, include sets, both exclude kinds, date ranges on either field, one
    that passes no row, several that pass fewer rows than a query asks for."""
    from voitta_rag_amd import SearchFilter as F

    # a created day that few live rows carry: fewer rows than k
    days, counts = np.unique(h["created"][h["live"] & (h["created"] != ABSENT)], return_counts=True)
    rare = int(days[np.argmin(counts)])
    out = [None, F()]                                    # (an empty filter is no filter)
    out += [F(folder_filter=j) for j in range(N_FOLDERS)]
    out += [F(include_folders=[1, 4]), F(include_folders=[0, 2, 3, 7, 11]), F(include_folders=[5]),
            F(folder_filter=3, include_folders=[3, 4]), F(folder_filter=3, include_folders=[4])]  # (the last: no row)
    out += [F(exclude_folders=[0, 2]), F(exclude_folders=list(range(1, N_FOLDERS))), F(exclude_index_folders=[1]),
            F(exclude_index_folders=[0, 3], exclude_folders=[6]), F(include_folders=[2, 8], exclude_index_folders=[2])]
    out += [F(date_start=1000), F(date_end=500), F(date_start=100, date_end=2600, date_field="created"),
            F(date_start=3900, date_field="created"), F(date_start=rare, date_end=rare, date_field="created"),
            F(date_start=2000, date_end=2010), F(date_start=1000, date_end=3000, include_folders=[1, 2, 3]),
            F(date_end=3000, date_field="created", exclude_folders=[4])]
    out += [F(include_folders=[]),                       # an empty include set: nothing passes
            F(folder_filter=9999)]                       # an id no row carries
    out += [F(date_start=j * 300, date_end=j * 300 + 40, exclude_index_folders=[j % 4]) for j in range(4)]
    return out


def oracle_mask(f, h):
    m = h["live"].copy()
    if f is None or f.is_empty():
        return m
    if f.folder_filter is not None:
        m &= h["folder"] == f.folder_filter
    if f.include_folders is not None:
        m &= np.isin(h["folder"], f.include_folders)
    if f.exclude_folders:
        m &= ~np.isin(h["folder"], f.exclude_folders)
    if f.exclude_index_folders:
        m &= ~np.isin(h["ifolder"], f.exclude_index_folders)
    if f.date_start is not None or f.date_end is not None:
        ts = h["created"] if f.date_field == "created" else h["modified"]
        m &= ts != ABSENT
        if f.date_start is not None:
            m &= ts >= f.date_start
        if f.date_end is not None:
            m &= ts <= f.date_end
    return m


def make_batch(h, nq=300, seed=5, n_cls=None):
    rng = np.random.default_rng(seed)
    cls = classes(h)
    if n_cls is not None:
        cls = cls[:n_cls]
    q = rng.standard_normal((nq, DIM)).astype(np.float32)
    q[::11] = h["x"][rng.integers(0, N, size=len(q[::11]))]  # some queries sit on a stored row
    flt = [cls[i % len(cls)] for i in rng.permutation(nq)]
    limits = rng.integers(1, 22, size=nq).astype(np.int32)
    limits[rng.random(nq) < 0.08] = 40                   # 3 x 40 > 64: the per-query paths
    weights = rng.uniform(0.0, 1.0, size=nq)
    sq = []
    for i in range(nq):
        m = int(rng.integers(0, 10))
        if i % 13 == 5:
            m = 0                                        # no sparse terms
        if i % 17 == 3:
            m = 40                                       # more than the grouped scan takes
        ids = rng.choice(80 if i % 3 == 0 else VOCAB, size=m, replace=False).astype(np.int32) * 7919 + 13  # (shared terms)
        sq.append((ids, rng.uniform(0.5, 1.5, size=m).astype(np.float32)))
    return q, sq, limits, weights, flt


@pytest.fixture(scope="module")
def small(gpu):
    e, h = build_small()
    h["oracle"] = ocore.SparseOracle(h["sp"], h["live"].astype(np.uint8))
    h["xh"] = ocore.cosine_preprocess(h["x"])
    yield e, h
    e.close()


def _same(a, b):
    ra, sa, fa = a
    rb, sb, fb = b
    return ra.tolist() == rb.tolist() and sa.tolist() == sb.tolist() and fa.tolist() == fb.tolist()


@pytest.mark.parametrize("fusion", ["minmax", "rrf"])
def test_hybrid_multi_equals_single_calls_and_the_oracle(small, fusion):
    from voitta_rag_amd.engine import VR_FUSION_MINMAX, VR_FUSION_RRF

    e, h = small
    mode = VR_FUSION_MINMAX if fusion == "minmax" else VR_FUSION_RRF
    q, sq, limits, weights, flt = make_batch(h)
    before = e.stats()
    got = e.search_hybrid_batch_multi(q, sq, limits, weights, flt, fusion=mode)
    n_small = int((3 * limits <= 64).sum())
    assert e.stats()["batched"] - before["batched"] >= n_small       # the dense legs shared the bit-plane scan
    dsc = ocore.dense_scores(ocore.cosine_preprocess(q), h["xh"])
    n_empty = n_short = 0
    for i in range(len(q)):
        one = e.search_hybrid(q[i], sq[i][0], sq[i][1], int(limits[i]), float(weights[i]), fusion=mode, flt=flt[i])
        assert _same(got[i], one), (fusion, i, flt[i], int(limits[i]))
        k, limit, mask = 3 * int(limits[i]), int(limits[i]), oracle_mask(flt[i], h).astype(np.uint8)
        dr, ds = ocore.topk(dsc[i], k, mask)
        if len(sq[i][0]):
            sr, ss = ocore.topk(h["oracle"].scores(*sq[i]), k, mask)
        else:
            sr, ss = np.zeros(0, np.int64), np.zeros(0, np.float32)
        if fusion == "minmax":
            want = ofus.hybrid_fuse(list(zip(dr.tolist(), ds.tolist())), list(zip(sr.tolist(), ss.tolist())), limit,
                                    float(weights[i]), "json")
        else:
            want = ofus.rrf_fuse(list(zip(dr.tolist(), ds.tolist())), list(zip(sr.tolist(), ss.tolist())), limit)
        assert got[i][0].tolist() == [r for r, _, _ in want], (fusion, i)
        assert got[i][1].tolist() == [s for _, s, _ in want], (fusion, i)
        n_empty += int(mask.sum() == 0)
        n_short += int(0 < mask.sum() < k)
    assert n_empty > 0 and n_short > 0                   # the batch held a class that passes nothing and one below k


def test_dense_multi_equals_single_calls_and_the_oracle(small):
    e, h = small
    q, _sq, _limits, _w, flt = make_batch(h, seed=9)
    dsc = ocore.dense_scores(ocore.cosine_preprocess(q), h["xh"])
    for k in (10, 64, 100):
        got = e.search_dense_multi(q, k, flt)
        for i in range(len(q)):
            r1, s1 = e.search_dense(q[i:i + 1], k, flt[i])[0]
            assert np.array_equal(got[i][0], r1) and np.array_equal(got[i][1].view(np.uint32), s1.view(np.uint32)), (k, i)
            wr, ws = ocore.topk(dsc[i], k, oracle_mask(flt[i], h).astype(np.uint8))
            assert np.array_equal(got[i][0], wr) and np.array_equal(got[i][1].view(np.uint32), ws.view(np.uint32)), (k, i)


def test_one_class_is_the_unfiltered_batch(small):
    from voitta_rag_amd import SearchFilter

    e, h = small
    q, sq, _limits, _w, _flt = make_batch(h, seed=11, nq=200)
    for f in (None, SearchFilter(exclude_folders=[0, 2], date_start=500)):
        want = e.search_hybrid_batch(q, sq, 10, 0.3, flt=f, raw=True)
        got = e.search_hybrid_batch_multi(q, sq, [10] * len(q), [0.3] * len(q), [f] * len(q), raw=True)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        wd = e.search_dense(q, 30, f, raw=True)
        gd = e.search_dense_multi(q, 30, [f] * len(q), raw=True)
        for a, b in zip(gd, wd):
            assert np.array_equal(a, b)


_CHILD = r"""
import json, sys
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import test_batch_filters_gpu as t
e, h = t.build_small()
q, sq, limits, weights, flt = t.make_batch(h, seed=21, nq=400, n_cls=int(sys.argv[3]))
r, s, fd, c = e.search_hybrid_batch_multi(q, sq, limits, weights, flt, raw=True)
dr, ds, dc = e.search_dense_multi(q, 20, flt, raw=True)
np.savez(sys.argv[4], r=r, s=s, fd=fd, c=c, dr=dr, ds=ds, dc=dc)
print(json.dumps(e.stats()))
e.close()
"""


@pytest.mark.parametrize("n_cls", [5, 40])
def test_class_slices_give_the_same_answer(small, tmp_path, n_cls):
    """VR_CLASS_PLANE_MIB=0: one class per slice (one batched scan per class, or the byte-mask path for a class of
    few queries) in a fresh process; the answer must not change."""
    e, h = small
    q, sq, limits, weights, flt = make_batch(h, seed=21, nq=400, n_cls=n_cls)
    r, s, fd, c = e.search_hybrid_batch_multi(q, sq, limits, weights, flt, raw=True)
    dr, ds, dc = e.search_dense_multi(q, 20, flt, raw=True)
    out = tmp_path / "child.npz"
    env = dict(os.environ, VR_CLASS_PLANE_MIB="0")
    p = subprocess.run([sys.executable, "-c", _CHILD, HERE, ROOT, str(n_cls), str(out)], env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    stats = json.loads(p.stdout.strip().splitlines()[-1])
    assert stats["batched"] > 0
    z = np.load(out)
    for i in range(len(q)):
        n = int(c[i])
        assert int(z["c"][i]) == n
        assert np.array_equal(z["r"][i, :n], r[i, :n]) and np.array_equal(z["s"][i, :n], s[i, :n])
        assert np.array_equal(z["fd"][i, :n], fd[i, :n])
    assert np.array_equal(z["dr"], dr) and np.array_equal(z["ds"], ds) and np.array_equal(z["dc"], dc)


def test_filtered_batch_overflow_is_redone_by_class(gpu):
    """A query of a FILTERED batch over its dense candidate budget: the batched scan gives it up and the class loop
    redoes it on the byte mask of its class. The corpus of test_batched_search_overflow_falls_back_per_query (6,000
    near-duplicates of row 0) with folder = row % 3: each folder holds 2,000 of them, so a query on the cluster exceeds
    the budget of 1,024 under every filter here, whether or not the scan counts the rows its filter removes."""
    from voitta_rag_amd import Engine, SearchFilter
    from voitta_rag_amd.engine import VR_FUSION_MINMAX

    dim, n, nq, k = 256, 20000, 42, 10
    rng = np.random.default_rng(77)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x[:6000] = x[0] + 2e-4 * rng.standard_normal((6000, dim)).astype(np.float32)
    folder = (np.arange(n) % 3).astype(np.int32)
    filters = [None, SearchFilter(include_folders=[0, 1]), SearchFilter(exclude_folders=[0])]
    masks = [np.ones(n, np.uint8), (folder != 2).astype(np.uint8), (folder != 0).astype(np.uint8)]
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    q[3:6] = x[0]
    q[6:9] = x[17] + 0.01 * rng.standard_normal((3, dim)).astype(np.float32)
    flt = [filters[i % 3] for i in range(nq)]
    want = ocore.dense_scores(ocore.cosine_preprocess(q), ocore.cosine_preprocess(x))
    e = Engine(dim, initial_rows=n)
    try:
        e.upsert(x, folder_ids=folder)
        before = e.stats()
        got = e.search_dense_multi(q, k, flt)
        after = e.stats()
        print("batch_fallback:", after["batch_fallback"] - before["batch_fallback"])
        assert after["batched"] - before["batched"] == nq
        assert after["batch_fallback"] - before["batch_fallback"] >= 1
        for i in range(nq):
            wr, ws = ocore.topk(want[i], k, masks[i % 3])
            assert np.array_equal(got[i][0], wr) and np.array_equal(got[i][1].view(np.uint32), ws.view(np.uint32)), i
            r1, s1 = e.search_dense(q[i:i + 1], k, flt[i])[0]
            assert np.array_equal(got[i][0], r1) and np.array_equal(got[i][1].view(np.uint32), s1.view(np.uint32)), i
        # the same batch as hybrid queries without sparse terms: limits 3, so k = 9 per leg
        none = (np.zeros(0, np.int32), np.zeros(0, np.float32))
        fused = e.search_hybrid_batch_multi(q, [none] * nq, [3] * nq, [0.1] * nq, flt, fusion=VR_FUSION_MINMAX)
        for i in range(nq):
            assert _same(fused[i], e.search_hybrid(q[i], none[0], none[1], 3, 0.1, fusion=VR_FUSION_MINMAX, flt=flt[i])), i
    finally:
        e.close()


def test_search_requests_equals_search_per_request(monkeypatch, gpu):
    """VectorStoreService with string folders and dates: result i of search_requests is search(**requests[i])."""
    from voitta_rag_amd import config, store_registry, vector_store
    from voitta_rag_amd.vector_store import ChunkMetadata

    monkeypatch.setenv("EMBEDDING_DIMENSION", str(DIM))
    config.get_settings.cache_clear()
    store_registry.reset()
    vector_store._vector_store = None
    try:
        rng = np.random.default_rng(31)
        n = 18_000
        x = rng.standard_normal((n, DIM)).astype(np.float32)
        folders = [f"docs/team{j}" for j in range(8)] + ["docs/team1/sub", "notes"]
        metas, sparse = [], []
        for i in range(n):
            fo = folders[int(rng.integers(0, len(folders)))]
            metas.append(ChunkMetadata(file_path=f"{fo}/f{i % 97}.md", folder_path=fo, index_folder=fo.split("/")[0] + str(i % 3),
                                       file_name="f.md", chunk_index=i, total_chunks=n, start_char=0, end_char=1, indexed_at="t",
                                       source_created_at=None if i % 9 == 0 else 1_700_000_000 + int(rng.integers(0, 5000)),
                                       source_modified_at=None if i % 7 == 0 else 1_700_000_000 + int(rng.integers(0, 5000))))
            m = int(rng.integers(1, 12))
            sparse.append((sorted(rng.choice(500, size=m, replace=False).tolist()), rng.uniform(0.2, 2.0, size=m).tolist()))
        vs = vector_store.get_vector_store()
        vs.store_chunks([(f"t{i}", x[i].tolist(), metas[i]) for i in range(n)], sparse_vectors=sparse)
        vs.delete_by_file("docs/team2/f5.md")
        kinds = [{}, {"folder_filter": "docs/team1"}, {"include_folders": ["docs/team1", "docs/team1/sub", "nowhere"]},
                 {"exclude_folders": ["notes", "docs/team0"]}, {"exclude_index_folders": ["docs1", "unknown"]},
                 {"date_start": 1_700_001_000}, {"date_end": 1_700_002_000, "date_field": "created"},
                 {"folder_filter": "no/such/folder"}, {"include_folders": ["docs/team3"], "date_start": 1_700_004_990},
                 {"exclude_folders": ["docs/team4"], "date_start": 1_700_000_500, "date_end": 1_700_003_000}]
        reqs = []
        for i in range(120):
            r = dict(kinds[i % len(kinds)])
            r["query_embedding"] = rng.standard_normal(DIM).astype(np.float32).tolist()
            r["limit"] = [10, 3, 21, 0, 40, 1][i % 6]
            if i % 4 != 0:
                m = int(rng.integers(1, 6))
                r["sparse_query"] = (rng.choice(500, size=m, replace=False).tolist(), rng.uniform(0.5, 1.5, size=m).tolist())
                r["sparse_weight"] = float(rng.uniform(0.0, 1.0))
            elif i % 8 == 0:
                r["sparse_query"] = ([], [])             # no terms: the dense-only branch
            reqs.append(r)
        got = vs.search_requests(reqs)
        assert len(got) == len(reqs)
        key = lambda c: (c.id, c.score, c.text)  # noqa: E731
        n_nonempty = 0
        for r, g in zip(reqs, got):
            want = vs.search(**r)
            assert [key(c) for c in g] == [key(c) for c in want], {k: v for k, v in r.items() if k != "query_embedding"}
            n_nonempty += bool(want)
        assert n_nonempty > len(reqs) // 2
        assert vs.search_requests([]) == []
    finally:
        store_registry.reset()
        config.get_settings.cache_clear()
        vector_store._vector_store = None


def test_large_batch_of_64_classes(gpu, monkeypatch):
    """1M x 768 rows, 1000 hybrid queries over 64 classes of folder / date filters: 100 sampled queries against single
    calls. At this size the sparse legs take the class-grouped scan of the inverted index (groups of one class, each
    reading its class's plane); with its candidate buffers shrunk to force the redo, the answer must not change."""
    import torch

    from voitta_rag_amd import Engine, SearchFilter

    n, d, nnz = 1_000_000, 768, 24
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(99)
    rng = np.random.default_rng(99)
    e = Engine(d, initial_rows=n)
    try:
        folder = rng.integers(0, 2000, size=n).astype(np.int32)
        modified = rng.integers(0, 100_000, size=n).astype(np.int64)
        modified[rng.random(n) < 0.05] = ABSENT
        for a in range(0, n, 125_000):
            b = a + 125_000
            x = torch.randn((125_000, d), device=dev, generator=g)
            ids = (torch.rand((125_000, nnz), device=dev, generator=g) ** 2 * 20_000).to(torch.int32)
            ids, _ = torch.sort(ids, dim=1)
            ids = ids * 32 + torch.arange(nnz, device=dev, dtype=torch.int32)[None, :]
            off = (torch.arange(125_001, device=dev, dtype=torch.int64) * nnz).contiguous()
            val = torch.rand((125_000 * nnz,), device=dev, generator=g) + 0.5
            e.upsert(x.contiguous(), sparse=(off, ids.reshape(-1).contiguous(), val.contiguous()), folder_ids=folder[a:b],
                     modified=modified[a:b])
        e.delete_rows(rng.choice(n, size=5000, replace=False))
        cls = []
        for j in range(64):
            inc = rng.choice(2000, size=int(rng.integers(50, 600)), replace=False).tolist()
            if j % 4 == 0:
                cls.append(SearchFilter(include_folders=inc))
            elif j % 4 == 1:
                cls.append(SearchFilter(exclude_folders=inc))
            elif j % 4 == 2:
                cls.append(SearchFilter(include_folders=inc, date_start=20_000))
            else:
                cls.append(SearchFilter(date_start=int(rng.integers(0, 50_000)), date_end=int(rng.integers(50_000, 100_000))))
        cls[5] = SearchFilter(date_start=777, date_end=778)      # about 19 rows: fewer than the legs' k = 30
        cls[9] = SearchFilter(include_folders=[])                # no row
        nq = 1000
        q = rng.standard_normal((nq, d)).astype(np.float32)
        flt = [cls[i % 64] for i in range(nq)]
        limits = np.full(nq, 10, np.int32)
        limits[::7] = 5
        limits[3::50] = 40                                       # 3 x 40 > 64: the per-query paths
        weights = rng.uniform(0.0, 1.0, size=nq)
        sq = []
        for i in range(nq):
            m = int(rng.integers(0, 8)) if i % 97 else 40        # (40 terms: more than the grouped scan takes)
            t = np.sort(rng.choice(20_000, size=m, replace=False)).astype(np.int32)
            sq.append((t * 32 + rng.integers(0, nnz, size=m).astype(np.int32), rng.uniform(0.5, 1.5, size=m).astype(np.float32)))
        before = e.stats()
        got = e.search_hybrid_batch_multi(q, sq, limits, weights, flt)
        after = e.stats()
        small = int((limits <= 21).sum())
        assert after["batched"] - before["batched"] >= small
        assert after["sparse_grouped"] - before["sparse_grouped"] >= small
        sample = set(rng.choice(nq, size=100, replace=False).tolist()) | {5, 9, 3, 97}
        for i in sorted(sample):
            one = e.search_hybrid(q[i], sq[i][0], sq[i][1], int(limits[i]), float(weights[i]), flt=flt[i])
            assert _same(got[i], one), i
        assert len(got[9][0]) == 0
        monkeypatch.setenv("VR_SPARSE_GROUP_SPILL", "1")
        monkeypatch.setenv("VR_SPARSE_GROUP_CAP", "1")
        again = e.search_hybrid_batch_multi(q, sq, limits, weights, flt)
        assert e.stats()["sparse_group_redo"] > after["sparse_group_redo"]
        assert all(_same(a, b) for a, b in zip(again, got))
    finally:
        e.close()
