"""The planted search layouts and their route model (tests/search_layouts.py), proven on the CPU from the oracle alone:
the mirrored constants are the sources', plant() is a permutation that puts rank j at pos[j], and every case of the
GPU matrix (test_search_layouts_gpu.py) meets the route condition it is there for."""
import os
import re

import numpy as np
import pytest

import search_layouts as sl
from oracle import core as ocore

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voitta_rag_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_mirrored_constants_are_the_sources():
    for name, where in sl.CONSTANT_SOURCES.items():
        m = re.search(r"constexpr int %s = (\d+);" % name, _source(where))
        assert m, (name, where)
        assert int(m.group(1)) == getattr(sl, name), (name, where)
    assert re.search(r"constexpr int kScan16Waves = (\d+);", _source("prefilter.hip")).group(1) == str(sl.kScanWaves)
    assert f"e->n_rows >= {sl.PREFILTER_MIN_ROWS};" in _source("prefilter.hip")
    assert f"e->n_rows >= {sl.BATCH_MIN_ROWS};" in _source("batch.hip")
    assert "nq > kQueryBlock && k <= kFusedMaxK" in _source("batch.hip")
    assert "if (k <= kFusedMaxK && nq <= 4)" in _source("search.hip")
    topk = _source("topk.hip")
    assert "constexpr int T2 = 1024, I2 = 16;" in topk and sl.LEVEL2_KEYS == 1024 * 16
    assert "if (c <= kGatherCap) {" in topk  # the slow path starts ABOVE the cap
    assert "8 * wm + i" in _source("batch.hip") and sl.SLAB_ROWS == 8 * sl.kTileRows


def test_scan_geometry_of_the_matrix_sizes():
    assert [sl.scan_grid(n) for n in (8320, 8192, 8064, sl.N_GRID_STRIDE)] == [(520, 65), (512, 64), (504, 63), (4121, 512)]
    slot, visit = sl.row_slots(sl.N_GRID_STRIDE)
    assert slot[-1] == 4120 - 4096 and visit[-1] == 16  # the one-row last tile: second iteration of slot 24
    assert visit.max() == 31 and np.count_nonzero(visit >= 16) == 24 * 16 + 1
    # inside a tile the registers go first: rows 0, 4, 8, 12, then 1, 5, ...
    assert visit[:16].tolist() == [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15]


LAYOUTS = [("one_tile", {}), ("one_wave", {}), ("ascending", {}), ("descending", {}), ("tail", {}),
           ("hot_blocks", {"h": 64}), ("hot_blocks", {"h": 8, "k": 47}), ("hot_blocks", {"h": 64, "gathered": 2049}),
           ("packed_slabs", {"s": 32})]


@pytest.mark.parametrize("n", [4095, 8335, sl.N_GRID_STRIDE])
def test_plant_is_a_permutation_with_rank_j_at_pos_j(n):
    dim = 16
    x, q = sl.gaussian(n, dim, n), sl.gaussian(1, dim, n + 1)[0]
    order = sl.reference_ranking(x, q)
    for layout, geo in LAYOUTS:
        if (layout == "hot_blocks" and geo["h"] > sl.scan_grid(n)[1]) or (layout == "packed_slabs" and n < 48 * sl.SLAB_ROWS):
            continue
        y = sl.plant(x, q, layout, **geo)
        pos = sl.positions(layout, n, **geo)
        assert np.array_equal(y[np.lexsort(y.T)], x[np.lexsort(x.T)]), layout  # the same multiset of rows
        assert np.array_equal(y[pos].view(np.uint32), x[order[:pos.shape[0]]].view(np.uint32)), layout
        # the oracle on the permuted corpus finds rank j at pos[j] (by score: rows of equal score may swap ranks)
        sc = sl.reference_scores(y, q)[0]
        assert np.array_equal(sc[pos], ocore.topk(sc, pos.shape[0])[1]), layout


def test_layout_properties():
    n, dim = sl.N_GRID_STRIDE, 16
    x, q = sl.gaussian(n, dim, 5), sl.gaussian(1, dim, 6)[0]
    slot, visit = sl.row_slots(n)
    for layout, sign in (("ascending", 1), ("descending", -1)):
        sc = sl.reference_scores(sl.plant(x, q, layout), q)[0]
        keys = np.argsort(np.argsort(sl.make_keys(sc)))  # place of every row's key among all keys
        for s in (0, 3, 24, 25, 4095):  # two-tile waves, the one-row tile's wave, one-tile waves
            walk = np.flatnonzero(slot == s)
            walk = walk[np.argsort(visit[walk])]
            assert np.all(sign * np.diff(keys[walk]) > 0), (layout, s)
    pos = sl.positions("one_tile", n)
    assert len({p // 16 for p in pos[:16]}) == 1 and len({p // sl.BLOCK_ROWS for p in pos}) == 1
    pos = sl.positions("one_wave", n)
    assert set(slot[pos[:32]]) == {3} and set(slot[pos[32:]]) == {4}  # two tiles per wave at this size
    # four iterations for the first eight slots: all 64 ranks in ONE wave
    assert set(sl.row_slots(sl.N_ONE_WAVE)[0][sl.positions("one_wave", sl.N_ONE_WAVE)]) == {3}
    assert sl.positions("tail", 16 * 7 + 1).tolist() == [112, 0]
    assert sl.positions("tail", 16 * 7 + 15).tolist() == list(range(112, 127)) + [0]
    g = 70
    tp = sl.tie_positions(8320, g)
    assert len({p // 16 for p in tp[:6]}) == 1 and len({p // sl.BLOCK_ROWS for p in tp[5:]}) == g - 5  # one per block
    y = sl.plant(x, q, "tie_group", g=g)
    best = x[sl.reference_ranking(x, q)[0]]
    assert np.all(y[sl.tie_positions(n, g)] == best) and np.count_nonzero((y != x).any(1)) in (g - 1, g)


def test_route_model_on_hand_made_lists():
    # three blocks (384 rows), k = 3: every other row scores -1, so the thresholds can be read off
    n, k = 3 * sl.BLOCK_ROWS, 3
    sc = np.full(n, -1.0, np.float32)
    sc[[0, 1, 2]] = 9.0, 5.0, 4.0          # block 0
    sc[[128, 129, 130]] = 8.0, 3.0, 2.0    # block 1
    sc[[256, 257, 258]] = 1.0, 0.9, 0.8    # block 2
    # best k-th entry 4 (block 0), k-th largest head 1: the keys >= 4 are 9, 8, 5, 4
    assert sl.fused_merge_gather(sc, None, k, 0, n) == (3, 4)
    mask = np.ones(n, bool)
    mask[2] = False                        # block 0: 9, 5, -1 -> best k-th entry 2 (block 1): 9, 8, 5, 3, 2
    assert sl.fused_merge_gather(sc, mask, k, 0, n) == (3, 5)
    sc[256] = 8.5                          # heads 9, 8.5, 8: the k-th largest head takes over -> 9, 8.5, 8
    assert sl.fused_merge_gather(sc, mask, k, 0, n) == (3, 3)
    mask[:] = False
    mask[[0, 300]] = True                  # fewer than k lists hold a key: no threshold, both keys are gathered
    assert sl.fused_merge_gather(sc, mask, k, 0, n) == (3, 2)
    # ties: the lower row wins, as in the oracle; -0.0 sorts below +0.0 (the bits decide), -inf is no key
    keys = sl.make_keys(np.array([1.0, 1.0, -0.0, 0.0, -np.inf], np.float32))
    assert keys[0] > keys[1] > keys[3] > keys[2] > keys[4] == 0


MERGE_CASES = list(sl.merge_cases())


def test_merge_cases_take_the_path_they_are_there_for():
    bound = {k: (k - 1) ** 2 + 1 for _, k, _, _ in sl.MERGE_PATHS}
    seen = set()
    for name, x, q, planted, k, path in MERGE_CASES:
        sc = sl.reference_scores(x, q)
        lists, gathered = sl.fused_merge_gather(sc, None, k, planted, x.shape[0])
        assert lists == sl.scan_grid(x.shape[0])[1] and gathered <= bound[k], name
        assert sl.takes_slow_path(gathered) == (path == "slow"), (name, gathered)
        if "_g" in name:  # the cap itself and one key more
            assert gathered == int(name.rsplit("_g", 1)[1]), (name, gathered)
        seen.add((lists, path))
        for i in range(q.shape[0]):  # the riders are i.i.d. queries: a few keys each
            if i != planted:
                assert not sl.takes_slow_path(sl.fused_merge_gather(sc, None, k, i, x.shape[0])[1]), (name, i)
    assert seen == {(65, "slow"), (65, "fast"), (512, "slow"), (512, "fast")}
    # the bound is reached: hot_blocks is the worst case of the fast path's thresholds
    name, x, q, planted, k, _ = MERGE_CASES[0]
    assert sl.fused_merge_gather(sl.reference_scores(x, q), None, k, planted, x.shape[0])[1] == bound[k] == 3970
    # an i.i.d. corpus of the same size is nowhere near the slow path
    x = sl.gaussian(8320, 16, 1)
    assert sl.fused_merge_gather(sl.reference_scores(x, q[:1]), None, 64, 0, 8320)[1] < 1024


def test_fewer_lists_than_k_have_no_head_threshold():
    """8064 rows are 63 lists: with k = 64 there is no k-th largest head, only the best k-th entry bounds the gather.
    The layouts that deal the winners evenly over the blocks (ascending, descending) then take the slow path as well;
    the same layouts at 64 and 65 lists do not. (test_fused_one_query_layouts runs all of them.)"""
    for n, slow in ((8064, True), (8192, False), (8320, False)):
        base, q = sl.gaussian(n, 16, n), sl.gaussian(1, 16, n + 1)
        for layout in ("ascending", "descending"):
            sc = sl.reference_scores(sl.plant(base, q[0], layout), q)
            assert sl.takes_slow_path(sl.fused_merge_gather(sc, None, 64, 0, n)[1]) == slow, (n, layout)
            assert not sl.takes_slow_path(sl.fused_merge_gather(sc, None, 10, 0, n)[1])


def test_batched_overflow_bound():
    nq = 17
    x, q = sl.packed_slabs_case(nq)
    sc = sl.reference_scores(x, q)
    certain = [sl.batched_overflow_certain(sc[i], None, 64) for i in range(nq)]
    assert certain[:sl.BATCH_PLANTED] == [True] * sl.BATCH_PLANTED and not any(certain[sl.BATCH_PLANTED:])
    assert sl.batched_candidates_certain(sc[0], None, 64) >= 4096
    # the siblings on the other side: k = 10 finds its 10 slabs among the 32, an unplanted corpus at k = 64
    assert not any(sl.batched_overflow_certain(sc[i], None, 10) for i in range(nq))
    plain = sl.reference_scores(sl.gaussian(sl.BATCH_ROWS, sl.BATCH_DIM, 31), q)
    assert not any(sl.batched_overflow_certain(plain[i], None, 64) for i in range(nq))
    # a filter that keeps one range of 4096 rows (32 slabs < k = 64): every kept row is a candidate
    mask = np.zeros(sl.BATCH_ROWS, bool)
    mask[2048:2048 + 4096] = True
    assert all(sl.batched_candidates_certain(plain[i], mask, 64) == 4096 for i in range(nq))
    mask[:] = False
    mask[2048:2048 + 512] = True  # 4 slabs, 512 rows: under the budget, the reference cannot decide
    assert all(sl.batched_candidates_certain(plain[i], mask, 64) == 512 for i in range(nq))
    assert not sl.batched_overflow_certain(plain[0], mask, 64)
