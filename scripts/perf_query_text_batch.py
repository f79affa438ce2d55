"""Questions as TEXT, N at a time, against the ways a server answers them without vr_query_text_batch:
python scripts/perf_query_text_batch.py [--rows N] [--sizes 1,16,64,256,1000] [--reps R] [--no-single] [--no-ab]

bench.py's corpus (unit rows x 768, 40-term Zipf BM25 rows) and its bge-base-shaped random encoder (f16) with a
synthetic WordPiece vocabulary; questions of 5-11 vocabulary words ("query: " prefixed on the dense side, about 14
tokens each), hybrid top-10, a filter class per question out of 8. Timed per batch size N, after a warm-up call, with
the engine synchronised around every call — one JSON line per measurement:
  (a) one vr_query_text_batch call;
  (b) N single vr_query_text calls (unless --no-single);
  (c) vr_encode, then vr_search_hybrid_batch_multi on the embeddings (two calls, the embeddings through the host);
  (d) the forward pass alone (vr_encode of the N questions), with the mid-size GEMM on, and — in a child process,
      VR_GEMM_MID=0 — off (unless --no-ab).
Kernel times: run one size under rocprofv3 --kernel-trace --stats with --reps 1 --no-single --no-ab."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from voitta_rag_amd import Engine, SearchFilter  # noqa: E402
from voitta_rag_amd import encoder as enc  # noqa: E402
from voitta_rag_amd.sparse_embedding import _query_vector  # noqa: E402
from voitta_rag_amd.wordpiece import WordPieceTokenizer  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--rows", type=int, default=1_000_000)
p.add_argument("--sizes", default="1,16,64,256,1000")
p.add_argument("--reps", type=int, default=5)
p.add_argument("--no-single", action="store_true", help="skip (b), the single calls")
p.add_argument("--no-ab", action="store_true", help="skip the forward pass with the mid-size GEMM off")
p.add_argument("--forward-only", action="store_true", help="(internal) the forward passes of (d) alone, no corpus")
args = p.parse_args()

M = bench.MODEL
dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev).manual_seed(1234)
rows = 0 if args.forward_only else args.rows
e = Engine(M["hidden"], initial_rows=rows + 4096)
state = bench.random_state(torch, gen, dev)
enc.load_encoder(e, enc.BertDesc(M["layers"], M["hidden"], M["heads"], M["intermediate"], vocab=M["vocab"], max_pos=M["max_pos"],
                                 pooling=M["pooling"], normalize=True, precision="f16"), state)
rng = np.random.default_rng(17)
vocab, words = bench.synthetic_vocab(rng, M["vocab"])
d = tempfile.mkdtemp(prefix="voitta-perf-")
open(os.path.join(d, "vocab.txt"), "w", encoding="utf-8").write("\n".join(vocab) + "\n")
tok = WordPieceTokenizer.from_pretrained(d)
warr = np.array(words)
sizes = [int(v) for v in args.sizes.split(",")]
pool = [" ".join(warr[rng.integers(0, len(warr), size=int(rng.integers(5, 12)))]) + "?" for _ in range(max(sizes))]
classes = [None] + [SearchFilter(folder_filter=j) for j in range(7)]


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


def forward(n, label):
    ids, off = tok.encode_batch(["query: " + q for q in pool[:n]])
    off = off.astype(np.int32)
    timed("(d) forward pass (vr_encode)", lambda: enc.encode(e, ids, off), n=max(args.reps, 5), questions=n,
          tokens=int(off[-1]), gemm_mid=label)


if args.forward_only:
    for n in sizes:
        forward(n, "off" if os.environ.get("VR_GEMM_MID") == "0" else "on")
    e.close()
    sys.exit(0)

folder = rng.integers(0, 8, size=rows + 100_000).astype(np.int32)


class _WithFolders:
    """bench.populate's engine, with a folder id per row"""

    def __init__(self, engine):
        self.engine, self.at = engine, 0

    def upsert(self, x, sparse):
        n = int(x.shape[0])
        self.engine.upsert(x, sparse=sparse, folder_ids=folder[self.at:self.at + n])
        self.at += n


bench.populate(torch, gen, dev, _WithFolders(e), rows, M["hidden"])
for n in sizes:
    qs = pool[:n]
    dense = ["query: " + q for q in qs]
    flt = [classes[i % len(classes)] for i in range(n)]
    limits = np.full(n, 10, np.int32)
    weights = np.full(n, 0.1)
    timed("(a) vr_query_text_batch", lambda: e.query_text_batch(tok._h, dense, qs, 512, limits, weights, flt, raw=True),
          questions=n)
    if not args.no_single:
        timed("(b) single vr_query_text calls", lambda: [e.query_text(tok._h, dense[i], qs[i], 512, 10, 0.1, flt=flt[i])
                                                         for i in range(n)], n=max(1, min(args.reps, 2)), questions=n)

    def two_calls():
        ids, off = tok.encode_batch(dense)
        emb = enc.encode(e, ids, off.astype(np.int32))
        sq = [_query_vector(q) for q in qs]
        sq = [(np.asarray(a, np.int32), np.asarray(b, np.float32)) for a, b in sq]
        return e.search_hybrid_batch_multi(emb, sq, limits, weights, flt, raw=True)

    timed("(c) vr_encode + vr_search_hybrid_batch_multi", two_calls, questions=n)
    forward(n, "on")
e.close()
if not args.no_ab:
    env = dict(os.environ, VR_GEMM_MID="0")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--forward-only", "--sizes", args.sizes, "--reps", str(args.reps)],
                   env=env, check=True, timeout=1200)
