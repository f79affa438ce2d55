"""Filtered batches against the ways a server answers per-request filters without them:
python scripts/perf_filtered_batch.py [--rows N] [--queries Q] [--reps R] [--classes 1,8,64,1000] [--no-single]

bench.py's corpus (unit rows x 768, 40-term Zipf BM25 rows) with 2,000 folders; queries of 4-6 Zipf terms, hybrid
top-10. The queries of a batch fall into C classes, each an include_folders set of 200 random folders (the MCP search
tool's expanded active folders, mcp_server.py:419-452). Timed per class count C, after a warm-up call, with the engine
synchronised around every call:
  (a) one vr_search_hybrid_batch_multi call;
  (b) group by filter: one vr_search_hybrid_batch per class;
  (c) the queries one by one through vr_search_hybrid (C = max only, unless --no-single).
Also: today's unfiltered batch and the same batch under one filter (what (a) at C = 1 routes to). One JSON line per
measurement. Kernel times: run one class count under rocprofv3 --kernel-trace --stats with --reps 1."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from voitta_rag_amd import Engine, SearchFilter  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--rows", type=int, default=1_000_000)
p.add_argument("--queries", type=int, default=1000)
p.add_argument("--reps", type=int, default=5)
p.add_argument("--classes", default="1,8,64,1000")
p.add_argument("--folders", type=int, default=2000)
p.add_argument("--no-single", action="store_true", help="skip (c), the one-by-one calls")
args = p.parse_args()

dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev).manual_seed(1234)
dim, rows, nq = 768, args.rows, args.queries
rng = np.random.default_rng(7)
folder = rng.integers(0, args.folders, size=rows + 100_000).astype(np.int32)
e = Engine(dim, initial_rows=rows + 64)


class _WithFolders:
    """bench.populate's engine, with a folder id per row"""

    def __init__(self, engine):
        self.engine, self.at = engine, 0

    def upsert(self, x, sparse):
        n = int(x.shape[0])
        self.engine.upsert(x, sparse=sparse, folder_ids=folder[self.at:self.at + n])
        self.at += n


bench.populate(torch, gen, dev, _WithFolders(e), rows, dim)
qgen = torch.Generator(device=dev).manual_seed(99)
qs = torch.nn.functional.normalize(torch.randn((nq, dim), device=dev, generator=qgen), dim=1).cpu().numpy()
q_terms = bench.stem_hash(torch, bench.zipf_ids(qgen, torch, nq * 6, 30000, dev)).view(-1, 6).cpu().numpy()
q_nnz = np.random.default_rng(5).integers(4, 7, size=nq)
ones = np.ones(8, np.float32)
sq = [(q_terms[i, : q_nnz[i]], ones[: q_nnz[i]]) for i in range(nq)]
limits = np.full(nq, 10, np.int32)
weights = np.full(nq, 0.1)


def timed(name, fn, n=args.reps, **extra):
    fn()
    e.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    e.sync()
    ms = (time.perf_counter() - t0) / n * 1e3
    print(json.dumps({"case": name, "ms": round(ms, 3), **extra}), flush=True)
    return ms


timed("unfiltered batch (vr_search_hybrid_batch)", lambda: e.search_hybrid_batch(qs, sq, 10, 0.1, raw=True))
for c in [int(v) for v in args.classes.split(",")]:
    cls = [SearchFilter(include_folders=rng.choice(args.folders, size=200, replace=False).tolist()) for _ in range(c)]
    of = rng.permutation(nq) % c
    flt = [cls[j] for j in of]
    if c == 1:
        timed("one-filter batch (vr_search_hybrid_batch)", lambda: e.search_hybrid_batch(qs, sq, 10, 0.1, flt=cls[0], raw=True),
              classes=1)
    s0 = e.stats()
    timed("(a) vr_search_hybrid_batch_multi", lambda: e.search_hybrid_batch_multi(qs, sq, limits, weights, flt, raw=True),
          classes=c)
    s1 = e.stats()
    print(json.dumps({"classes": c, "batched_per_call": (s1["batched"] - s0["batched"]) / (args.reps + 1),
                      "batch_fallback": s1["batch_fallback"] - s0["batch_fallback"]}), flush=True)
    groups = [np.flatnonzero(of == j) for j in range(c)]

    def grouped():
        for j, idx in enumerate(groups):
            if len(idx):
                e.search_hybrid_batch(qs[idx], [sq[i] for i in idx], 10, 0.1, flt=cls[j], raw=True)

    timed("(b) one vr_search_hybrid_batch per class", grouped, n=max(1, min(args.reps, 3)), classes=c)
    if c == max(int(v) for v in args.classes.split(",")) and not args.no_single:
        timed("(c) single vr_search_hybrid calls",
              lambda: [e.search_hybrid(qs[i], sq[i][0], sq[i][1], 10, 0.1, flt=flt[i]) for i in range(nq)], n=1, classes=c)
e.close()
