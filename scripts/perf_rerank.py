"""Cross-encoder reranking on the GPU (vr_rerank_text), MiniLM-L6 / -L12 shapes (H 384, 12 heads of 32, I 1536):
python scripts/perf_rerank.py [--layers 6,12] [--reps R] [--precision f16] [--cpu-threads 16] [--no-cpu]

Seeded weights, a synthetic WordPiece vocabulary, questions of 5-11 words and passages of about 120 tokens (the chunk
length bench.py uses), max_len 512. Timed after a warm-up call of the same shape, with a host clock around each
synchronised call (vr_rerank_text returns with its logits on the host); one JSON line per measurement:
  1 question x {20, 50, 100} candidates, and 64 questions x 50 candidates in one call: ms per call, pairs/s, and the
  GEMM TFLOP/s computed from the shapes (24 H^2 L + 4 H I L per token ... see gemm_flop) over the call time;
  the CPU baseline (unless --no-cpu): torch BertForSequenceClassification on --cpu-threads threads, padded batch,
  for the single-question cases.
Kernel times: run under rocprofv3 --kernel-trace --stats with --reps 1 --no-cpu."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import rerank_oracle as ro  # noqa: E402
from oracle import bert as obert  # noqa: E402
from voitta_rag_amd import Engine  # noqa: E402
from voitta_rag_amd import encoder as enc  # noqa: E402
from voitta_rag_amd.wordpiece import WordPieceTokenizer  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--layers", default="6,12")
p.add_argument("--reps", type=int, default=20)
p.add_argument("--precision", default="f16")
p.add_argument("--cpu-threads", type=int, default=16)
p.add_argument("--no-cpu", action="store_true")
args = p.parse_args()

CASES = [(1, 20), (1, 50), (1, 100), (64, 50)]
rng = np.random.default_rng(23)
vocab, words = bench.synthetic_vocab(rng, 30522)
d = tempfile.mkdtemp(prefix="voitta-rerank-")
open(os.path.join(d, "vocab.txt"), "w", encoding="utf-8").write("\n".join(vocab) + "\n")
tok = WordPieceTokenizer.from_pretrained(d, max_length=512)
warr = np.array(words)


def text(n):
    return " ".join(warr[rng.integers(0, len(warr), size=n)])


def gemm_flop(T, n_pairs, H, I, L):
    """The GEMMs of the forward pass: Q/K/V over every token in every layer; output projection and FFN over every
    token except in the last layer, where only the n [CLS] rows need them; the head's pooler. 2 FLOP per MAC."""
    return 2.0 * (T * 3 * H * H * L + (T * (L - 1) + n_pairs) * (H * H + 2 * H * I) + n_pairs * H * H)


for L in (int(v) for v in args.layers.split(",")):
    shape = obert.BertShape(L, 384, 12, 1536, vocab=len(vocab), max_pos=512)
    w = ro.random_weights(shape, 5, 8.0)
    e = Engine(384)
    enc.load_reranker(e, enc.BertDesc(L, 384, 12, 1536, vocab=len(vocab), max_pos=512, pooling="cls", normalize=False,
                                      precision=args.precision), w)
    for nq, nc in CASES:
        queries = [text(int(rng.integers(5, 12))) + "?" for _ in range(nq)]
        cands = [[text(100) for _ in range(nc)] for _ in range(nq)]
        a = [q for q, c in zip(queries, cands) for _ in c]
        ids, off, seg = tok.encode_pairs(a, [x for c in cands for x in c])
        T = int(off[-1])
        e.rerank_text(tok._h, queries, cands, 512)  # warm-up: workspace, graphs
        e.rerank_text(tok._h, queries, cands, 512)
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            e.rerank_text(tok._h, queries, cands, 512)
            ts.append(time.perf_counter() - t0)
        ms = 1e3 * float(np.median(ts))
        n = nq * nc
        rec = {"what": "gpu rerank_text", "layers": L, "precision": args.precision, "queries": nq, "candidates": nc,
               "tokens": T, "ms_median": round(ms, 4), "ms_min": round(1e3 * min(ts), 4), "pairs_per_s": round(n / ms * 1e3, 1),
               "gemm_tflops": round(gemm_flop(T, n, 384, 1536, L) / (ms * 1e-3) / 1e12, 3)}
        print(json.dumps(rec), flush=True)
        if args.no_cpu or nq != 1:
            continue
        import torch
        import transformers

        torch.set_num_threads(args.cpu_threads)
        cfg = transformers.BertConfig(vocab_size=len(vocab), hidden_size=384, num_hidden_layers=L, num_attention_heads=12,
                                      intermediate_size=1536, max_position_embeddings=512, num_labels=1)
        m = transformers.BertForSequenceClassification(cfg).eval()
        m.load_state_dict({(k if k.startswith("classifier.") else "bert." + k): torch.from_numpy(v) for k, v in w.items()},
                          strict=False)
        S = int(np.max(np.diff(off)))
        bi = torch.zeros((n, S), dtype=torch.long)
        bm = torch.zeros((n, S), dtype=torch.long)
        bt = torch.zeros((n, S), dtype=torch.long)
        for i in range(n):
            k = int(off[i + 1] - off[i])
            bi[i, :k] = torch.from_numpy(ids[off[i]:off[i + 1]].astype(np.int64))
            bm[i, :k] = 1
            bt[i, int(seg[i]):k] = 1
        with torch.no_grad():
            m(input_ids=bi, attention_mask=bm, token_type_ids=bt)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                m(input_ids=bi, attention_mask=bm, token_type_ids=bt)
                ts.append(time.perf_counter() - t0)
        ms = 1e3 * float(np.median(ts))
        print(json.dumps({"what": f"cpu torch {args.cpu_threads} threads", "layers": L, "queries": nq, "candidates": nc,
                          "ms_median": round(ms, 2), "pairs_per_s": round(n / ms * 1e3, 1)}), flush=True)
    e.close()
