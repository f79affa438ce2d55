"""Dense search on planted layouts (tests/search_layouts.py): the winners of a query sit in one tile, in one wave's
tiles, in ascending or descending order of every wave's walk, in a few scan blocks, in the last partial tile, in a
group of exact ties that k cuts through — on every top-k route and on both sides of every route switch in the row
count. Every answer is compared bit for bit with oracle.core on the permuted corpus: ranked rows, f32 score bits, counts
when fewer than k rows survive, and row -1 in the key slots behind the count. The route a case is there for is proven
from the reference by the CPU model (asserted again here before the engine is touched) and by the stats() counters.
Each case prints one `LAYOUTS|` line (profiles/search_layouts_checks.md is made from them)."""
import json

import numpy as np
import pytest

import search_layouts as sl
from oracle import core as ocore

pytestmark = pytest.mark.gpu

COUNTERS = ("two_stage", "fallback", "batched", "batch_fallback")
TIE_G = sl.kListLen + 6  # copies of the best row: more than any fused k, so every k <= 65 cuts through the group


def _engine(dim, **kw):
    from voitta_rag_amd import Engine

    return Engine(dim, **kw)


def _delta(before, after):
    return {c: after[c] - before[c] for c in COUNTERS}


def _log(**kw):
    print("LAYOUTS| " + json.dumps(kw))


class Ref:
    """oracle answers for the queries q over the corpus x: one full sort per (query, mask), every k a prefix of it"""

    def __init__(self, x, q):
        self.q = np.ascontiguousarray(q, np.float32).reshape(-1, x.shape[1])
        self.sc = sl.reference_scores(x, self.q)
        self.cache = {}

    def want(self, i, k, mask=None, mask_id=None):
        key = (i, mask_id)
        if mask is None or mask_id is not None:
            if key not in self.cache:
                self.cache[key] = ocore.topk(self.sc[i], sl.kBatchCand, None if mask is None else mask.astype(np.uint8))
            rows, scores = self.cache[key]
            return rows[:k], scores[:k]
        return ocore.topk(self.sc[i], k, mask.astype(np.uint8))


def _check(e, ref, k, nq=None, flt=None, mask=None, mask_id=None, tag=None, keys=False):
    """search_dense (and, with keys, search_dense_keys) of the first nq queries of ref against the oracle"""
    from voitta_rag_amd import Engine

    q = ref.q if nq is None else ref.q[:nq]
    got = e.search_dense(q, k, flt)
    dec = Engine.decode_keys(e.search_dense_keys(q, k, flt)) if keys else None
    for i in range(q.shape[0]):
        wr, ws = ref.want(i, k, mask, mask_id)
        assert got[i][0].shape[0] == wr.shape[0], (tag, k, i, got[i][0].shape[0], wr.shape[0])
        assert np.array_equal(got[i][0], wr), (tag, k, i)
        assert np.array_equal(got[i][1].view(np.uint32), ws.view(np.uint32)), (tag, k, i)
        if keys:
            c = wr.shape[0]
            assert np.array_equal(dec[0][i][:c], wr) and (dec[0][i][c:] == -1).all(), (tag, k, i)
            assert np.array_equal(dec[1][i][:c].view(np.uint32), ws.view(np.uint32)), (tag, k, i)


def _corpora(base, q0):
    """(layout, corpus) for every layout that applies to a corpus of this size, planted for the query q0"""
    for layout in ("ascending", "descending", "one_tile", "one_wave"):
        yield layout, sl.plant(base, q0, layout)
    if base.shape[0] % sl.kTileRows:
        yield "tail", sl.plant(base, q0, "tail")
    yield "tie_group", sl.plant(base, q0, "tie_group", g=TIE_G)


def _expected(n, dim, prefilter, plans):
    """(two_stage, batched) movement of a list of (nq, k) searches, from the route conditions alone: more than 16
    queries of k <= 64 on an int8 shadow of dim % 128 == 0 and >= 16384 rows are batched; anything else runs in blocks
    of 16 queries, and a block of ONE query with k <= 64 takes the two-stage search from 4096 rows on."""
    shadow = prefilter and dim % 32 == 0
    two_stage = batched = 0
    for nq, k in plans:
        if shadow and dim % 128 == 0 and nq > sl.kQueryBlock and k <= sl.kFusedMaxK and n >= sl.BATCH_MIN_ROWS:
            batched += nq
        elif shadow and nq % sl.kQueryBlock == 1 and k <= sl.kFusedMaxK and n >= sl.PREFILTER_MIN_ROWS:
            two_stage += 1
    return two_stage, batched


def _run_layouts(route, base, q, planted, plans, prefilter=True, extra=()):
    """Every layout of _corpora (and `extra` ones) planted for q[planted], on an engine of its own: the searches of
    `plans` ((nq, k) pairs) against the oracle; then, for the tie group, two members deleted and a third filtered out."""
    from voitta_rag_amd import SearchFilter

    n, dim = base.shape
    for layout, x in list(_corpora(base, q[planted])) + [(name, sl.plant(base, q[planted], name, **geo)) for name, geo in extra]:
        ref = Ref(x, q)
        folder = np.zeros(n, np.int32)
        members = sl.tie_positions(n, TIE_G) if layout == "tie_group" else None
        if members is not None:
            folder[members[2]] = 7
        e = _engine(dim, prefilter=prefilter)
        e.upsert(x, folder_ids=folder)
        before = e.stats()
        for nq, k in plans:
            _check(e, ref, k, nq, tag=(route, n, layout, nq))
        d = _delta(before, e.stats())
        two_stage, batched = _expected(n, dim, prefilter, plans)
        # (a batched query over its budget is redone alone, by the two-stage search: counted there too)
        assert d["two_stage"] == two_stage + d["batch_fallback"], (route, n, layout, d)
        assert d["batched"] == batched, (route, n, layout, d)
        if n < 262144:  # fewer tiles than kMaxCandTiles: the re-score budget cannot overflow
            assert n // sl.kTileRows < sl.kMaxCandTiles and d["fallback"] == 0, (route, n, layout, d)
        _log(route=route, n=n, dim=dim, layout=layout, planted=planted, plans=plans, last_candidates=e.stats()["last_candidates"], **d)
        if members is not None:  # the survivors of the group still come back in row order
            e.delete_rows(members[[0, 4]])
            mask = np.ones(n, bool)
            mask[members[[0, 2, 4]]] = False
            for nq, k in plans:
                _check(e, ref, k, nq, SearchFilter(exclude_folders=[7]), mask, "tie", tag=(route, n, "tie_group-3", nq))
            got = e.search_dense(q[planted:planted + 1], plans[-1][1], SearchFilter(exclude_folders=[7]))[0]
            tied = got[0][got[1] == got[1][0]]
            want = np.sort(np.setdiff1d(np.flatnonzero(ref.sc[planted] == ref.sc[planted].max()), members[[0, 2, 4]]))
            assert tied.shape[0] >= 1 and np.array_equal(tied, want[:tied.shape[0]]), (route, n, tied)
        e.close()


# ---- merge_lists_kernel: fast path, cap, slow path ------------------------------------------------------------------

@pytest.mark.parametrize("shape", sl.MERGE_SHAPES)
def test_fused_merge_fast_and_slow_path(gpu, shape):
    """hot_blocks on the fused route: 65 lists and 512 lists, one query and the last of four. The CPU model says which
    path merge_lists_kernel takes ((k - 1)^2 + 1 keys at most: slow for k = 64 and 47, fast for k = 46 — the largest k
    that cannot leave the fast path — and for k = 32 and hot_blocks(8)); two more corpora gather exactly kGatherCap keys
    (still fast) and kGatherCap + 1 (slow)."""
    for name, x, q, planted, k, path in sl.merge_cases([shape]):
        ref = Ref(x, q)
        lists, gathered = sl.fused_merge_gather(ref.sc, None, k, planted, x.shape[0])
        assert sl.takes_slow_path(gathered) == (path == "slow"), (name, gathered)
        e = _engine(x.shape[1], prefilter=q.shape[0] > 1)  # one query: the one-stage engine; 2-4 queries: the default one
        e.upsert(x)
        _check(e, ref, k, tag=name, keys=True)
        d = _delta({c: 0 for c in COUNTERS}, e.stats())
        assert d["two_stage"] == 0 and d["batched"] == 0
        _log(route="fused-merge", case=name, k=k, planted=planted, n_lists=lists, gathered=gathered, path=path)
        e.close()


# ---- the route matrix -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [8320, 8192, 8064, sl.N_GRID_STRIDE, 8321, 8335, sl.N_ONE_WAVE])
def test_fused_one_query_layouts(gpu, n):
    """Engine(prefilter=False), one query, k <= 64: dense_scan_topk with 65, 64, 63 lists, 512 lists with grid-striding
    waves, n = 16 m + 1 / 16 m + 15 for the tail, and the size at which one wave walks four tiles (one_wave: all 64
    winners in ONE wave's list)."""
    base, q = sl.gaussian(n, 16, n), sl.gaussian(1, 16, n + 1)
    _run_layouts("fused-1q", base, q, 0, [(1, 1), (1, 10), (1, 64)], prefilter=False)


@pytest.mark.parametrize("n,dim", [(8320, 16), (8320, 32), (sl.N_GRID_STRIDE, 16), (sl.N_GRID_STRIDE, 32)])
def test_fused_few_queries_layouts(gpu, n, dim):
    """The default engine with 2 and 4 queries takes the fused scan at any size; the layout is planted for query 0 and
    again for the last query, the other queries ride along and are checked too."""
    base, q = sl.gaussian(n, dim, n + dim), sl.gaussian(4, dim, n + dim + 1)
    for planted, plans in ((0, [(2, 64), (4, 10), (4, 64)]), (1, [(2, 10), (2, 64)]), (3, [(4, 10), (4, 64)])):
        _run_layouts("fused-2..4q", base, q, planted, plans)


@pytest.mark.parametrize("n", [4095, 4096, 4097, 16385])
def test_select_layouts(gpu, n):
    """dense_scores + topk_select: 5 and 16 queries at any k, one query with k > 64; one segment, a second segment that
    holds one row, five segments."""
    base, q = sl.gaussian(n, 16, n), sl.gaussian(16, 16, n + 1)
    _run_layouts("select", base, q, 0, [(5, 1), (5, 64), (16, 1), (16, 64), (1, 65), (1, 1024)])


def test_select_three_levels(gpu):
    """n = 17 * 4096 + 1 and k = 1024: 18 segments leave 18,432 keys, two level-2 blocks, and a third level."""
    n = 17 * sl.kTopkSeg + 1
    assert -(-n // sl.kTopkSeg) * 1024 > sl.LEVEL2_KEYS
    base, q = sl.gaussian(n, 16, n), sl.gaussian(5, 16, n + 1)
    _run_layouts("select-3-levels", base, q, 0, [(1, 1024), (5, 64)], extra=[("packed_slabs", {"s": 8, "total": 1024})])


@pytest.mark.parametrize("n", [4095, 4096, 8320, sl.N_GRID_STRIDE])
@pytest.mark.parametrize("shadow", ["int8", "f16"])
def test_two_stage_layouts(gpu, shadow, n, monkeypatch):
    """The default engine, one query, k <= 64: the int8 shadow (dim 64) and the f16 one (dim 32, VR_PREFILTER=f16);
    two_stage moves exactly when n >= 4096, and the re-score budget never overflows."""
    dim = 64 if shadow == "int8" else 32
    if shadow == "f16":
        monkeypatch.setenv("VR_PREFILTER", "f16")
    base, q = sl.gaussian(n, dim, n + dim), sl.gaussian(1, dim, n + dim + 1)
    _run_layouts("two-stage-" + shadow, base, q, 0, [(1, 1), (1, 10), (1, 64)])


@pytest.mark.parametrize("n", [16383, 16384, 16385 + 16])
def test_batched_layouts(gpu, n):
    """dim 128, 17 queries and 130 (two query columns, the second almost empty), k = 10 and 64: the batched search serves
    them exactly when n >= 16384. batch_fallback is recorded, not asserted: the reference cannot decide it here."""
    base, q = sl.gaussian(n, sl.BATCH_DIM, n), sl.gaussian(130, sl.BATCH_DIM, n + 1)
    _run_layouts("batched", base, q, 0, [(17, 10), (17, 64), (130, 10), (130, 64)])


# ---- fewer than k survivors ---------------------------------------------------------------------------------------------

def _survivor_rows(n, k, where):
    if where == "tail":  # all inside the last, partial tile
        assert n % sl.kTileRows >= k
        return n - n % sl.kTileRows + np.arange(k)
    return np.linspace(3, n - 40, k).astype(np.int64)  # spread over the corpus


@pytest.mark.parametrize("route,dim,n,nq,prefilter", [
    ("fused", 16, 8335, 1, False), ("fused", 16, 8335, 3, True), ("select", 16, 4111, 5, True),
    ("two-stage-int8", 64, 4111, 1, True), ("two-stage-f16", 32, 4111, 1, True), ("batched", 128, 16399, 17, True)])
def test_fewer_than_k_survivors(gpu, route, dim, n, nq, prefilter, monkeypatch):
    """0, 1, k - 1 and k rows survive a folder filter, spread over the corpus and all inside the last partial tile; then
    the same counts produced by delete_rows. Counts, rows, score bits and the -1 rows behind the count are the oracle's."""
    from voitta_rag_amd import SearchFilter

    if route == "two-stage-f16":
        monkeypatch.setenv("VR_PREFILTER", "f16")
    k = 8
    x, q = sl.gaussian(n, dim, n + dim), sl.gaussian(nq, dim, n + dim + 1)
    ref = Ref(x, q)
    keep = {"spread": _survivor_rows(n, k, "spread"), "tail": _survivor_rows(n, k, "tail")}
    folder = np.zeros(n, np.int32)
    folder[keep["spread"]] = 100 + np.arange(k)
    folder[keep["tail"]] = 200 + np.arange(k)
    e = _engine(dim, prefilter=prefilter)
    e.upsert(x, folder_ids=folder)
    before = e.stats()
    for where, first in (("spread", 100), ("tail", 200)):
        for c in (0, 1, k - 1, k):
            ids = list(range(first, first + c)) or [999]
            mask = np.isin(folder, ids)
            assert mask.sum() == c
            _check(e, ref, k, flt=SearchFilter(include_folders=ids), mask=mask, tag=(route, where, c), keys=True)
    d = _delta(before, e.stats())
    two_stage, batched = _expected(n, dim, prefilter, [(nq, k)])
    assert (d["two_stage"], d["batched"], d["fallback"]) == (16 * two_stage, 16 * batched, 0), (route, d)
    e.close()
    for where in ("spread", "tail"):  # ... and by tombstones: k, k - 1, 1, 0 rows left
        e = _engine(dim, prefilter=prefilter)
        e.upsert(x)
        live = np.zeros(n, bool)
        live[keep[where]] = True
        e.delete_rows(np.flatnonzero(~live))
        for gone in ([], keep[where][-1:], keep[where][1:-1], keep[where][:1]):
            if len(gone):
                e.delete_rows(gone)
                live[gone] = False
            _check(e, ref, k, mask=live, tag=(route, where, "deleted", int(live.sum())), keys=True)
        assert live.sum() == 0 and e.count() == (n, 0)
        dd = _delta({c: 0 for c in COUNTERS}, e.stats())
        assert (dd["two_stage"], dd["batched"], dd["fallback"]) == (8 * two_stage, 8 * batched, 0), (route, dd)
        e.close()
    _log(route=route + "-survivors", n=n, dim=dim, nq=nq, k=k, **d)


# ---- the batched search's per-query overflow, by layout -----------------------------------------------------------------

@pytest.mark.parametrize("nq", [17, 130])
def test_batched_overflow_by_layout(gpu, nq):
    """packed_slabs(32): the whole top 4096 of the planted queries sits in 32 slabs, fewer than k = 64, so T_q collapses
    and the reference alone says that they exceed the candidate budget (batched_overflow_certain): batch_fallback rises
    by at least their number, the riders of the same call are answered exactly. The same with a filter that keeps one
    range of 4096 rows: every query overflows, batch_fallback rises by exactly nq."""
    from voitta_rag_amd import SearchFilter

    x, q = sl.packed_slabs_case(nq)
    n = x.shape[0]
    ref = Ref(x, q)
    certain = [sl.batched_overflow_certain(ref.sc[i], None, 64) for i in range(nq)]
    assert certain[:sl.BATCH_PLANTED] == [True] * sl.BATCH_PLANTED and sum(certain) == sl.BATCH_PLANTED
    assert not any(sl.batched_overflow_certain(ref.sc[i], None, 10) for i in range(nq))
    folder = np.zeros(n, np.int32)
    folder[2048:2048 + 4096] = 300  # 32 slabs
    folder[8192:8192 + 512] = 301   # 4 slabs, 512 rows: under the budget
    e = _engine(sl.BATCH_DIM)
    e.upsert(x, folder_ids=folder)
    log = {}
    for k, flt, mask, at_least, exactly in ((64, None, None, sum(certain), None), (10, None, None, 0, None),
                                            (64, 300, folder == 300, nq, nq), (10, 300, folder == 300, 0, None),
                                            (64, 301, folder == 301, 0, None)):
        if mask is not None:
            n_certain = sum(sl.batched_overflow_certain(ref.sc[i], mask, k) for i in range(nq))
            assert n_certain == (exactly or 0), (k, flt, n_certain)
        before = e.stats()
        _check(e, ref, k, flt=None if flt is None else SearchFilter(folder_filter=flt), mask=mask, mask_id=flt,
               tag=("overflow", k, flt), keys=flt == 301)
        d = _delta(before, e.stats())
        assert d["batched"] == nq * (2 if flt == 301 else 1) and d["fallback"] == 0, (k, flt, d)
        assert d["batch_fallback"] >= at_least, (k, flt, d)
        if exactly is not None:
            assert d["batch_fallback"] == exactly, (k, flt, d)
        log[f"k{k}_folder{flt}"] = d["batch_fallback"]
    _log(route="batched-overflow", n=n, dim=sl.BATCH_DIM, nq=nq, certain_k64=sum(certain), batch_fallback=log)
    e.close()


# ---- route switches in the row count --------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,sizes,prefilter,plans", [
    (64, (4095, 4096, 4097), True, [(1, 10), (3, 10), (5, 10), (1, 65)]),
    (16, (4095, 4096, 4097), False, [(1, 10), (1, 64), (5, 1)]),
    (128, (16383, 16384), True, [(17, 10), (1, 10), (4, 64)])])
def test_route_edges_in_the_row_count(gpu, dim, sizes, prefilter, plans):
    """4095 | 4096 (prefilter_usable), 4096 | 4097 (a second select segment of one row, a one-row last tile) and
    16383 | 16384 (batch_usable): the larger corpus is the smaller one plus one more upsert on the SAME engine, so the
    shadow corpus and the selection buffers grow across the switch; at every size the newest row is the best one."""
    n = sizes[-1]
    base, q = sl.gaussian(n, dim, n + dim), sl.gaussian(max(p[0] for p in plans), dim, n + dim + 1)
    x = sl.permute(base, sl.reference_ranking(base, q[0]), np.array([s - 1 for s in reversed(sizes)] + [0]))
    e = _engine(dim, prefilter=prefilter)
    have = 0
    for m in sizes:
        assert e.upsert(x[have:m]) == have
        have = m
        ref = Ref(x[:m], q)
        assert ref.want(0, 1)[0][0] == m - 1  # the row that crossed the edge wins
        before = e.stats()
        for nq, k in plans:
            _check(e, ref, k, nq, tag=("edge", dim, m, nq), keys=True)
        d = _delta(before, e.stats())
        two_stage, batched = _expected(m, dim, prefilter, plans)
        assert (d["two_stage"], d["batched"], d["fallback"]) == (2 * two_stage + d["batch_fallback"], 2 * batched, 0), (dim, m, d)
        _log(route="edge", n=m, dim=dim, plans=plans, **d)
    e.close()
