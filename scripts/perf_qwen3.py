"""A Qwen3-Embedding-0.6B-shaped decoder embedder, engine level only: what head size 128 and the Q/K norm pass cost.
python scripts/perf_qwen3.py [--label NAME] [--reps R] [--out FILE] [--layers L] [--case SUBSTRING] [--only qwen3|qwen2]
(VOITTA_ENGINE_LIB selects the library)

Two models on ONE engine, one after the other, so both see the same box, clocks and neighbours, seeded weights, f16,
causal, last-token pooling, ids and outputs on the device:
  Qwen3-0.6B shape: 28 x 1024, 16 heads of 128 over 8 KV heads (attention width 2048), intermediate 3072, Q/K norms, no
                    attention biases, vocabulary 151,669 — loaded through encoder.qwen3_slots
  Qwen2-0.5B shape: 24 x 896, 14 heads of 64 over 2 KV heads, intermediate 4864, q/k/v biases, vocabulary 151,936 —
                    scripts/perf_qwen2.py's model, the yardstick beside every case
Cases: 2200 chunks of 96..140 tokens (~118: the bench's chunk lengths), 256 chunks of 384 tokens (head size 128: the
streamed kernel, from 321 tokens on), one 12-token question (the folded-RMSNorm skinny route, the cached graph's replay),
one sequence of 8192 tokens. Per case and model: two warm-up calls, then --reps synchronised calls (median, min, max),
then three profiled calls for the time of the attention launches alone (HIP events around each launch).
The attention launch's compulsory traffic is every token's Q, K and V read once and its context written once, f16:
8 A bytes per token and layer; `attention_hbm_share` is that over the launch's time as a share of 8 TB/s (the streamed
kernel re-reads K and V once per 128-query block, mostly from L2: its share of HBM traffic is not its share of time).
qk_norm_rope_kernel runs once per layer and call (`qk_norm_launches_per_call`); its time comes from a kernel trace of
this script (rocprofv3 --kernel-trace --stats -- python scripts/perf_qwen3.py --only qwen3 --case ... --reps 3): the
kernel's total time over its calls in the trace's kernel_stats.csv.
One JSON line per measurement, also appended to --out."""
import argparse
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
p.add_argument("--label", default="change")
p.add_argument("--reps", type=int, default=5)
p.add_argument("--layers", type=int, default=0, help="0: each model's own depth")
p.add_argument("--case", default="", help="only the cases whose name contains this")
p.add_argument("--only", default="", choices=["", "qwen3", "qwen2"])
p.add_argument("--out", default="profiles/qwen3_perf.jsonl")
args = p.parse_args()
assert args.reps >= 3

dev = torch.device("cuda", 0)
MAX_SEQ, HBM_BYTES_PER_S = 8192, 8.0e12
g = torch.Generator(device=dev).manual_seed(4321)


def rand(*shape, std=0.02):
    return (torch.randn(shape, device=dev, generator=g) * std).cpu().numpy()


def model(kind):
    """(name, hidden, attention width, layers, description, state dict under the library's names)"""
    if kind == "qwen3":
        L, H, NH, NKV, DH, I, vocab = args.layers or 28, 1024, 16, 8, 128, 3072, 151669
    else:
        L, H, NH, NKV, DH, I, vocab = args.layers or 24, 896, 14, 2, 64, 4864, 151936
    A = NH * DH
    state = {"embed_tokens.weight": rand(vocab, H, std=1.0), "norm.weight": 1.0 + rand(H)}
    for i in range(L):
        b = f"layers.{i}."
        state[b + "self_attn.q_proj.weight"] = rand(A, H, std=H ** -0.5)
        for n in ("k_proj", "v_proj"):
            state[b + f"self_attn.{n}.weight"] = rand(NKV * DH, H, std=H ** -0.5)
        if kind == "qwen3":
            state[b + "self_attn.q_norm.weight"], state[b + "self_attn.k_norm.weight"] = 0.9 + rand(DH), 0.9 + rand(DH)
        else:
            state[b + "self_attn.q_proj.bias"] = rand(A, std=0.3)
            for n in ("k_proj", "v_proj"):
                state[b + f"self_attn.{n}.bias"] = rand(NKV * DH, std=0.3)
        state[b + "self_attn.o_proj.weight"] = rand(H, A, std=A ** -0.5)
        state[b + "mlp.gate_proj.weight"], state[b + "mlp.up_proj.weight"] = rand(I, H, std=H ** -0.5), rand(I, H, std=H ** -0.5)
        state[b + "mlp.down_proj.weight"] = rand(H, I, std=I ** -0.5)
        state[b + "input_layernorm.weight"], state[b + "post_attention_layernorm.weight"] = 1.0 + rand(H), 1.0 + rand(H)
    extra = dict(head_dim=DH, qk_norm=1) if kind == "qwen3" else {}
    desc = enc.BertDesc(L, H, NH, I, vocab=vocab, max_pos=MAX_SEQ, type_vocab=1, pooling="last", precision="f16", eps=1e-6,
                        position="rotary", rope_theta=1e6, ffn="swiglu", norm="rms_pre_rotary", causal=1, **extra)
    name = f"Qwen3-0.6B shape ({L} layers), f16" if kind == "qwen3" else f"Qwen2-0.5B shape ({L} layers), f16"
    return name, H, A, L, vocab, desc, state


rng = np.random.default_rng(7)
CASES = [("2200 chunks of 96..140", rng.integers(96, 141, size=2200).tolist()), ("256 chunks of 384", [384] * 256),
         ("1 question of 12", [12]), ("1 x 8192", [8192])]
CASES = [c for c in CASES if args.case in c[0]]


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


results = {}
for kind in ("qwen3", "qwen2"):
    if args.only and kind != args.only:
        continue
    name, H, A, L, vocab, desc, state = model(kind)
    e = Engine(H)
    enc.load_encoder(e, desc, state)
    del state
    for case, lens in CASES:
        off_h = np.zeros(len(lens) + 1, np.int32)
        off_h[1:] = np.cumsum(lens)
        ids = torch.from_numpy(np.random.default_rng(11).integers(0, vocab, size=int(off_h[-1])).astype(np.int32)).to(dev)
        off, out = torch.from_numpy(off_h).to(dev), torch.empty((len(lens), H), dtype=torch.float32, device=dev)
        times = []
        for rep in range(args.reps + 2):
            e.sync()
            t0 = time.perf_counter()
            enc.encode(e, ids, off, out=out)
            e.sync()
            if rep >= 2:
                times.append(time.perf_counter() - t0)
        assert bool(torch.isfinite(out).all())
        e.profile(True)
        a0 = e.profile_read(Engine.PROF_ATTENTION)
        for _ in range(3):
            enc.encode(e, ids, off, out=out)
        e.sync()
        a1 = e.profile_read(Engine.PROF_ATTENTION)
        e.profile(False)
        t = np.array(times) * 1e3
        tokens, att_ms, launches = int(sum(lens)), (a1[0] - a0[0]) / 3, (a1[1] - a0[1]) // 3
        att_bytes = 8.0 * A * tokens * launches  # Q, K, V read and the context written once, f16, per launch
        results[kind, case] = (float(np.median(t)), att_ms)
        emit(build=args.label, model=name, case=case, sequences=len(lens), tokens=tokens, reps=args.reps,
             ms_median=round(float(np.median(t)), 3), ms_min=round(float(t.min()), 3), ms_max=round(float(t.max()), 3),
             sequences_per_s=round(len(lens) / float(np.median(t)) * 1e3, 1), attention_ms_per_call=round(att_ms, 3),
             attention_launches_per_call=launches, attention_bytes_per_call=int(att_bytes),
             attention_hbm_share=round(att_bytes / (att_ms * 1e-3) / HBM_BYTES_PER_S, 4),
             qk_norm_launches_per_call=L if kind == "qwen3" else 0)
    e.close()
if not args.only:
    for case, _ in CASES:
        a, b = results["qwen3", case], results["qwen2", case]
        emit(build=args.label, state="Qwen3-0.6B shape over Qwen2-0.5B shape", case=case, call_time=round(a[0] / b[0], 4),
             attention_time=round(a[1] / b[1], 4))
