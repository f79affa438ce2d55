"""A ModernBERT cross-encoder on the GPU (vr_rerank), the ModernBERT-base shape (L 22, H 768, 12 heads of 64, I 1152,
window 64 in two of every three layers, mean pooling as gte-reranker-modernbert-base):
python scripts/perf_modernbert_rerank.py [--reps R] [--precision f16] [--out profiles/modernbert_rerank_perf.jsonl]

Seeded weights and random ids: pairs of a 5-11 token question and a passage of about 110 tokens, as ids (the checkpoint's
byte-level BPE is the tokenizers library's work, not the engine's, and is not timed here). Timed after two warm-up calls
of the same shape, with a host clock around each synchronised call (vr_rerank returns with its logits on the host); one
JSON line per measurement, appended to --out:
  1 question x {20, 50, 100} candidates and 64 x 50 in one call: ms per call (median and minimum), pairs/s
  the head alone (rerank_head_ln_kernel) is inside those calls; its share: run under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import modernbert_oracle as mo  # noqa: E402
import modernbert_rerank_oracle as mro  # noqa: E402
from voitta_rag_amd import Engine  # noqa: E402
from voitta_rag_amd import encoder as enc  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=20)
p.add_argument("--precision", default="f16")
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "modernbert_rerank_perf.jsonl"))
args = p.parse_args()

CASES = [(1, 20), (1, 50), (1, 100), (64, 50)]
shape = mo.ModernShape(22, 768, 12, 1152, vocab=50368, max_pos=512, window=64, global_every=3)
w = mro.random_weights(shape, 5, False, 8.0)
e = Engine(768)
enc.load_reranker(e, mro.desc_for(shape, "mean", args.precision), w)
rng = np.random.default_rng(23)
out = open(args.out, "a")
for nq, nc in CASES:
    lens = np.concatenate([int(rng.integers(5, 12)) + rng.integers(100, 121, size=nc) + 3 for _ in range(nq)])
    off = np.zeros(len(lens) + 1, np.int32)
    off[1:] = np.cumsum(lens)
    ids = rng.integers(3, shape.vocab, size=int(off[-1])).astype(np.int32)
    e.rerank(ids, off, None)  # warm-up: workspace, graphs
    e.rerank(ids, off, None)
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        e.rerank(ids, off, None)
        ts.append(time.perf_counter() - t0)
    ms = 1e3 * float(np.median(ts))
    rec = {"what": "gpu vr_rerank, ModernBERT-base shape", "precision": args.precision, "queries": nq, "candidates": nc,
           "tokens": int(off[-1]), "ms_median": round(ms, 4), "ms_min": round(1e3 * min(ts), 4),
           "pairs_per_s": round(nq * nc / ms * 1e3, 1)}
    print(json.dumps(rec), flush=True)
    out.write(json.dumps(rec) + "\n")
out.close()
e.close()
