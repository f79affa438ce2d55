"""A Qwen3-Reranker-0.6B-shaped decoder cross-encoder, engine level only: what a reranking call costs, and what the
last-token tail (rerank_tail: the last layer's output projection, FFN and final norm on n_seq rows instead of T) saves.
python scripts/perf_qwen3_rerank.py [--reps R] [--rounds N] [--layers L] [--out profiles/qwen3_rerank_perf.jsonl]

28 x 1024, 16 heads of 128 over 8 KV heads, intermediate 3072, Q/K norms, vocabulary 151,669, tied embeddings, seeded
weights, f16, causal. Pairs as the published template makes them, by ASSUMED token counts (the real tokenizer is not
here): prefix 36, "<Instruct>: .." 22, "<Query>: " + 5..11, "<Document>: " + 100..120, suffix 10 — about 190 tokens a pair.
Cases: 1 question x 50 passages; 64 x 50 in one call. Ids, offsets and outputs on the device, a host clock around each
synchronised call, two warm-up calls per shape.
Comparator for the tail, on the SAME engine: the same body loaded as an embedder with last-token pooling and no
normalisation (vr_encoder_load), which runs its whole last layer on T rows and pools; the same ids. The two are run
interleaved, --rounds rounds of --reps calls each; per round the median of each and their ratio, then the spread of
the ratios. Beside it the arithmetic estimate: per token and layer the GEMMs are 2 H (3 A) + 2 A H (Q/K/V, output) +
2 H (2 I) + 2 I H (FFN) FLOP; the tail removes the output projection and the FFN of the last layer, all but n_seq / T
of them. One JSON line per measurement, also appended to --out."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voitta_rag_amd import Engine  # noqa: E402
from voitta_rag_amd import encoder as enc  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--reps", type=int, default=7)
p.add_argument("--rounds", type=int, default=3)
p.add_argument("--layers", type=int, default=28)
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "qwen3_rerank_perf.jsonl"))
args = p.parse_args()

dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(4322)
L, H, NH, NKV, DH, I, VOCAB = args.layers, 1024, 16, 8, 128, 3072, 151669
A = NH * DH
YES_ID, NO_ID = 9693, 2152  # any two rows: the head is their difference


def rand(*shape, std=0.02):
    return (torch.randn(shape, device=dev, generator=g) * std).cpu().numpy()


state = {"embed_tokens.weight": rand(VOCAB, H, std=1.0), "norm.weight": 1.0 + rand(H)}
for i in range(L):
    b = f"layers.{i}."
    state[b + "self_attn.q_proj.weight"] = rand(A, H, std=H ** -0.5)
    for n in ("k_proj", "v_proj"):
        state[b + f"self_attn.{n}.weight"] = rand(NKV * DH, H, std=H ** -0.5)
    state[b + "self_attn.q_norm.weight"], state[b + "self_attn.k_norm.weight"] = 0.9 + rand(DH), 0.9 + rand(DH)
    state[b + "self_attn.o_proj.weight"] = rand(H, A, std=A ** -0.5)
    state[b + "mlp.gate_proj.weight"], state[b + "mlp.up_proj.weight"] = rand(I, H, std=H ** -0.5), rand(I, H, std=H ** -0.5)
    state[b + "mlp.down_proj.weight"] = rand(H, I, std=I ** -0.5)
    state[b + "input_layernorm.weight"], state[b + "post_attention_layernorm.weight"] = 1.0 + rand(H), 1.0 + rand(H)
desc = enc.BertDesc(L, H, NH, I, vocab=VOCAB, max_pos=512, type_vocab=1, pooling="last", normalize=False, precision="f16",
                    eps=1e-6, position="rotary", rope_theta=1e6, ffn="swiglu", norm="rms_pre_rotary", causal=1, head_dim=DH,
                    qk_norm=1)
e = Engine(H)
enc.load_reranker(e, desc, state, yes_id=YES_ID, no_id=NO_ID)  # the reranker slot: the tail
enc.load_encoder(e, desc, state)                               # the embedder slot: the full last layer, then pooling
score = torch.from_numpy(enc.qwen3_rerank_head(state, desc, YES_ID, NO_ID)[0]).to(dev)
del state


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def rerank(ids, off, out):
    e._follow(ids)
    enc.check(e._lib.vr_rerank(e.handle, C.c_void_p(ids.data_ptr()), C.c_void_p(off.data_ptr()), None, int(off.shape[0]) - 1,
                               enc.VR_MEM_DEVICE, C.c_void_p(out.data_ptr()), enc.VR_MEM_DEVICE))


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        e.sync()
        t0 = time.perf_counter()
        fn()
        e.sync()
        ts.append(time.perf_counter() - t0)
    return 1e3 * np.asarray(ts)


rng = np.random.default_rng(29)
for nq, nc in ((1, 50), (64, 50)):
    lens = np.concatenate([36 + 22 + 2 + int(rng.integers(5, 12)) + 3 + rng.integers(100, 121, size=nc) + 10 for _ in range(nq)])
    off_h = np.zeros(len(lens) + 1, np.int32)
    off_h[1:] = np.cumsum(lens)
    T, n = int(off_h[-1]), len(lens)
    ids = torch.from_numpy(rng.integers(0, VOCAB, size=T).astype(np.int32)).to(dev)
    off = torch.from_numpy(off_h).to(dev)
    logits = torch.empty(n, dtype=torch.float32, device=dev)
    rows = torch.empty((n, H), dtype=torch.float32, device=dev)
    tail = lambda: rerank(ids, off, logits)  # noqa: E731
    full = lambda: enc.encode(e, ids, off, out=rows)  # noqa: E731
    for fn in (tail, full, tail, full):  # warm-up: workspaces, graphs
        fn()
    e.sync()
    # the two routes agree: the embedder's rows dotted with the head are the tail's logits (f16 body on both sides)
    worst = float((rows.double() @ score.double() - logits.double()).abs().max())
    per_tok = 2 * H * 3 * A + 2 * A * H + 2 * H * 2 * I + 2 * I * H
    removed = (2 * A * H + 2 * H * 2 * I + 2 * I * H) * (1 - n / T) / (per_tok * L)
    ratios, t_tail, t_full = [], [], []
    for r in range(args.rounds):
        a, b = timed(tail, args.reps), timed(full, args.reps)
        t_tail.append(float(np.median(a)))
        t_full.append(float(np.median(b)))
        ratios.append(t_tail[-1] / t_full[-1])
        emit(what="vr_rerank (last-token tail) against vr_encode of the same body with last pooling (full last layer), same engine, "
                  "same ids, interleaved", model=f"Qwen3-Reranker-0.6B shape ({L} layers), f16, seeded weights", round=r + 1,
             queries=nq, candidates=nc, pairs=n, tokens=T, reps=args.reps, tail_ms_median=round(t_tail[-1], 4),
             tail_ms_min=round(float(a.min()), 4), full_ms_median=round(t_full[-1], 4), full_ms_min=round(float(b.min()), 4),
             ratio_tail_over_full=round(ratios[-1], 5))
    emit(what="summary over the rounds; the estimate is GEMM FLOP removed over the call's GEMM FLOP (arithmetic, not measured)",
         queries=nq, candidates=nc, pairs=n, tokens=T, rounds=args.rounds,
         tail_ms=round(float(np.median(t_tail)), 4), full_ms=round(float(np.median(t_full)), 4),
         pairs_per_s=round(n / float(np.median(t_tail)) * 1e3, 1),
         ratio_tail_over_full=round(float(np.median(ratios)), 5), ratio_spread=round(max(ratios) - min(ratios), 5),
         estimated_gemm_share_removed=round(removed, 5),
         tail_ahead_by_more_than_the_spread=bool(1 - float(np.median(ratios)) > max(ratios) - min(ratios)),
         worst_logit_difference_between_the_routes=round(worst, 6))
e.close()
