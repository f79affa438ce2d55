"""Leak check by arithmetic: create and close an engine 20 times in this process — per round one upsert, one search of
every kind (single, batched, filtered, filtered batch, sparse, grouped sparse batch, hybrid, hybrid batch), one
vr_query_text through a small random BERT and one compaction — and print the free device memory
(torch.cuda.mem_get_info) after every round. Flat from round 2 on = nothing the engine allocates outlives it.
Usage: python scripts/engine_leak_rounds.py TAG [ROUNDS]   (VOITTA_ENGINE_LIB selects another build of the library;
the last line is a JSON summary)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from oracle import bert as obert
from test_query_text_batch_gpu import WORDS, _vocab
from voitta_rag_amd import Engine, SearchFilter
from voitta_rag_amd import encoder as enc
from voitta_rag_amd.wordpiece import WordPieceTokenizer

tag = sys.argv[1]
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 20
N, D = 20000, 128
rng = np.random.default_rng(5)
vocab = _vocab()
tok = WordPieceTokenizer(vocab, max_length=32)
shape = obert.BertShape(2, D, 4, 256, vocab=len(vocab), max_pos=64)
w = obert.random_weights(shape, 5)
x = rng.standard_normal((N, D)).astype(np.float32)
idx = (np.sort(rng.integers(0, 600, (N, 8)), axis=1) + np.arange(8) * 600).astype(np.int32).reshape(-1)
off = np.arange(N + 1, dtype=np.int64) * 8
val = (rng.random(N * 8) + 0.25).astype(np.float32)
folder = rng.integers(0, 4, N).astype(np.int32)
q = rng.standard_normal((40, D)).astype(np.float32)
sq = [(np.sort(rng.choice(4800, size=5, replace=False)).astype(np.int32), np.ones(5, np.float32)) for _ in range(40)]
flt = SearchFilter(include_folders=[1, 2])
torch.cuda.init()
free = []
stats = None
for r in range(rounds):
    e = Engine(D)
    enc.load_encoder(e, enc.BertDesc(2, D, 4, 256, vocab=len(vocab), max_pos=64, pooling="mean", precision="f16"), w)
    e.upsert(x, sparse=(off, idx, val), folder_ids=folder)
    e.search_dense(q[:1], 10)
    e.search_dense(q[:1], 10, flt)
    e.search_dense(q[:3], 100)
    e.search_dense(q, 10)
    e.search_dense_multi(q, 10, [flt if i % 2 else None for i in range(40)])
    e.search_sparse(sq[0][0], sq[0][1], 30, flt)
    e.search_sparse(sq[0][0], sq[0][1], 100)
    e.search_sparse_batch(sq, 10)
    e.search_hybrid(q[0], sq[0][0], sq[0][1], 10, 0.1)
    e.search_hybrid_batch(q, sq, 10, 0.1)
    words = " ".join(rng.choice(WORDS, size=5))
    e.query_text(tok._h, "query: " + words, words, 32, 10, 0.1)
    e.delete_rows(np.arange(0, N, 3))
    e.compact()
    e.search_dense(q[:1], 10)
    stats = e.stats()
    e.close()
    torch.cuda.synchronize()
    free.append(int(torch.cuda.mem_get_info()[0]))
    print(f"{tag} round {r + 1}: free {free[-1]}", flush=True)
out = dict(tag=tag, free=free, after_round_2=free[1], after_last=free[-1], lost=free[1] - free[-1], stats=stats)
print(json.dumps({k: v for k, v in out.items() if k != "free"}))
