"""MMR diversification (vr_mmr_select) on the bge-base shape: 1M synthetic rows x 768 with sparse vectors,
seeded. One JSON line per case:
  single dense / hybrid search, limit 20 from 50 and from 100 candidates: the first stage alone, then with MMR
  1000 dense-only search_requests with MMR: the two engine calls VectorStoreService.search_requests makes for them,
  the filtered batch at the candidate count (vr_search_dense_multi, 50 each), then ONE vr_mmr_select over the 1000 lists
  (the service's host work around them, payload lookups and score transport, is not timed)
Times are host wall-clock medians of whole engine calls (each returns its results to the host); the batch line's
gflops / gbs divide the Gram's FLOP and the gathered bytes by the whole call's time, a lower bound on the kernels' rates.
The per-kernel times of DESIGN §15 come from
  rocprofv3 --kernel-trace --stats -d OUT -o mmr -- python scripts/perf_mmr.py --reps 3
Usage: python scripts/perf_mmr.py [--rows N] [--reps R]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voitta_rag_amd import Engine  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--rows", type=int, default=1_000_000)
p.add_argument("--dim", type=int, default=768)
p.add_argument("--reps", type=int, default=30)
p.add_argument("--batch", type=int, default=1000)
a = p.parse_args()

rng = np.random.default_rng(31)
e = Engine(a.dim, initial_rows=a.rows)
step = 100_000
for s in range(0, a.rows, step):
    n = min(step, a.rows - s)
    x = rng.standard_normal((n, a.dim), dtype=np.float32)
    nnz = rng.integers(4, 16, size=n)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(nnz)
    idx = np.concatenate([np.sort(rng.choice(30000, size=int(k), replace=False)) for k in nnz]).astype(np.int32)
    val = rng.uniform(0.2, 2.0, size=int(off[-1])).astype(np.float32)
    e.upsert(x, sparse=(off, idx, val))
e.sync()
gen = e.generation()


def med(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def emit(**kw):
    print(json.dumps(kw), flush=True)


q = rng.standard_normal((a.batch, a.dim), dtype=np.float32)
qi = np.sort(rng.choice(30000, size=6, replace=False)).astype(np.int32)
qv = np.ones(6, np.float32)
for cands in (50, 100):
    r, s = e.search_dense(q[:1], cands)[0]
    rel = np.asarray(s, np.float32).astype(np.float64)
    t_first = med(lambda: e.search_dense(q[:1], cands), a.reps)
    t_mmr = med(lambda: e.mmr_select([r], [rel], [0.5], [20], gen), a.reps)
    t_both = med(lambda: e.mmr_select([e.search_dense(q[:1], cands)[0][0]], [rel], [0.5], [20], gen), a.reps)
    emit(case="dense", limit=20, candidates=cands, first_stage_ms=t_first, mmr_ms=t_mmr, with_mmr_ms=t_both)
    hr, hs, _ = e.search_hybrid(q[0], qi, qv, cands, 0.1)
    hrel = np.asarray(hs, np.float64)
    t_first = med(lambda: e.search_hybrid(q[0], qi, qv, cands, 0.1), a.reps)
    t_mmr = med(lambda: e.mmr_select([hr], [hrel], [0.5], [20], gen), a.reps)
    t_both = med(lambda: e.mmr_select([e.search_hybrid(q[0], qi, qv, cands, 0.1)[0]], [hrel], [0.5], [20], gen), a.reps)
    emit(case="hybrid", limit=20, candidates=cands, first_stage_ms=t_first, mmr_ms=t_mmr, with_mmr_ms=t_both)

filters = [None] * a.batch
br, bs, bc = e.search_dense_multi(q, 50, filters, raw=True)
rows = [br[i, : bc[i]] for i in range(a.batch)]
rels = [np.asarray(bs[i, : bc[i]], np.float32).astype(np.float64) for i in range(a.batch)]
reps = max(3, a.reps // 5)
t_first = med(lambda: e.search_dense_multi(q, 50, filters, raw=True), reps)
t_mmr = med(lambda: e.mmr_select(rows, rels, [0.5] * a.batch, [20] * a.batch, gen), reps)
# Gram work of the call: per list the tile pairs I <= J (16 x 16 x D fma each); the gathered rows K x D x 4 bytes
tiles = [(len(r) + 15) // 16 for r in rows]
flop = sum(t * (t + 1) // 2 for t in tiles) * 16 * 16 * a.dim * 2.0
gathered = sum(len(r) for r in rows) * a.dim * 4.0
emit(case="search_requests", queries=a.batch, limit=20, candidates=50, first_stage_ms=t_first, mmr_call_ms=t_mmr,
     gram_flop=flop, gathered_bytes=gathered, call_gflops_lower_bound=flop / t_mmr / 1e6, call_gbs_lower_bound=gathered / t_mmr / 1e6)
e.close()
