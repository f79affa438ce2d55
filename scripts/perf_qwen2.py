"""A Qwen2-0.5B-shaped decoder embedder, engine level only: what the body costs, and what the causal mask saves.
python scripts/perf_qwen2.py [--label NAME] [--reps R] [--out FILE] [--layers L]   (VOITTA_ENGINE_LIB selects the library)

The model is the Qwen2-0.5B shape (24 x 896, 14 heads of 64 over 2 KV heads, intermediate 4864, RMSNorm pre-norm, rotary
positions with theta 1e6, SwiGLU, biases on q/k/v, vocabulary 151,936, last-token pooling, f16) with seeded weights under
Qwen2Model's names, loaded through encoder.qwen2_slots (the K/V heads repeated to 14); ids and outputs on the device.
ONE engine: the model is loaded with causal = 1, measured, loaded again with causal = 0 (the same weights, the same
buffers' sizes), measured, so both states see the same box, clocks and neighbours.
Cases: 2200 chunks of 96..140 tokens (~118: the bench's chunk lengths), one 12-token question (the folded-RMSNorm route at
K = 896, the cached graph's replay), 256 chunks of 384 tokens, one sequence of 8192 tokens (the streamed kernel). Per case
and state: two warm-up calls, then --reps synchronised calls (median, min, max), then three profiled calls for the time of
the attention launches alone (HIP events around each launch). Reported per case: causal over bidirectional, for the call
and for the attention launches.
Last: the Q/K/V product's width. The engine multiplies by [3H = 2688, 896] (K and V heads repeated); native grouped-query
attention would multiply by [H + 2 H_kv = 1152, 896]. Both are timed as plain f16 GEMMs (torch.matmul) over the 2200
chunks' tokens, times the 24 layers: what the follow-up can save per indexing call.
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
p.add_argument("--layers", type=int, default=24)
p.add_argument("--out", default="profiles/qwen2_perf.jsonl")
args = p.parse_args()
assert args.reps >= 3

dev = torch.device("cuda", 0)
L, H, NH, NKV, I, VOCAB, MAX_SEQ = args.layers, 896, 14, 2, 4864, 151936, 8192
DH = H // NH
g = torch.Generator(device=dev).manual_seed(4321)


def rand(*shape, std=0.02):
    return (torch.randn(shape, device=dev, generator=g) * std).cpu().numpy()


state = {"embed_tokens.weight": rand(VOCAB, H, std=1.0), "norm.weight": 1.0 + rand(H)}
for i in range(L):
    b = f"layers.{i}."
    state[b + "self_attn.q_proj.weight"], state[b + "self_attn.q_proj.bias"] = rand(H, H, std=H ** -0.5), rand(H, std=0.3)
    for n in ("k_proj", "v_proj"):
        state[b + f"self_attn.{n}.weight"], state[b + f"self_attn.{n}.bias"] = rand(NKV * DH, H, std=H ** -0.5), rand(NKV * DH, std=0.3)
    state[b + "self_attn.o_proj.weight"] = rand(H, H, std=H ** -0.5)
    state[b + "mlp.gate_proj.weight"], state[b + "mlp.up_proj.weight"] = rand(I, H, std=H ** -0.5), rand(I, H, std=H ** -0.5)
    state[b + "mlp.down_proj.weight"] = rand(H, I, std=I ** -0.5)
    state[b + "input_layernorm.weight"], state[b + "post_attention_layernorm.weight"] = 1.0 + rand(H), 1.0 + rand(H)


def describe(causal):
    return enc.BertDesc(L, H, NH, I, vocab=VOCAB, max_pos=MAX_SEQ, type_vocab=1, pooling="last", precision="f16", eps=1e-6,
                        position="rotary", rope_theta=1e6, ffn="swiglu", norm="rms_pre_rotary", causal=causal)


rng = np.random.default_rng(7)
CASES = [("2200 chunks of 96..140", rng.integers(96, 141, size=2200).tolist()), ("1 question of 12", [12]),
         ("256 chunks of 384", [384] * 256), ("1 x 8192", [8192])]
INPUTS = {}
for name, lens in CASES:
    off_h = np.zeros(len(lens) + 1, np.int32)
    off_h[1:] = np.cumsum(lens)
    INPUTS[name] = (torch.from_numpy(rng.integers(0, VOCAB, size=int(off_h[-1])).astype(np.int32)).to(dev),
                    torch.from_numpy(off_h).to(dev), torch.empty((len(lens), H), dtype=torch.float32, device=dev))
MODEL = f"Qwen2-0.5B shape ({L} layers), f16"


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


e = Engine(H)
results = {}
for causal in (1, 0):
    enc.load_encoder(e, describe(causal), state)
    for name, lens in CASES:
        ids, off, out = INPUTS[name]
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
        results[name, causal] = (float(np.median(t)), (a1[0] - a0[0]) / 3, out[:2].cpu().numpy())
        emit(build=args.label, model=MODEL, causal=causal, case=name, sequences=len(lens), tokens=int(sum(lens)), reps=args.reps,
             ms_median=round(float(np.median(t)), 3), ms_min=round(float(t.min()), 3), ms_max=round(float(t.max()), 3),
             sequences_per_s=round(len(lens) / float(np.median(t)) * 1e3, 1), attention_ms_per_call=round(results[name, causal][1], 3),
             attention_launches_per_call=(a1[1] - a0[1]) // 3)
e.close()
for name, _ in CASES:
    c, b = results[name, 1], results[name, 0]
    assert not np.array_equal(c[2], b[2])  # the two states are two models
    emit(build=args.label, model=MODEL, state="causal over bidirectional", case=name, call_time=round(c[0] / b[0], 4),
         attention_time=round(c[1] / b[1], 4))

# the Q/K/V product at the engine's width against the grouped-query width, as plain f16 GEMMs over the indexing call's tokens
T = int(sum(CASES[0][1]))
x = torch.randn((T, H), device=dev, dtype=torch.float16)
widths = {"3H (repeated K/V heads)": 3 * H, "H + 2 H_kv (grouped-query)": H + 2 * NKV * DH}
gemm_ms = {}
for what, n in widths.items():
    wt = torch.randn((n, H), device=dev, dtype=torch.float16)
    for _ in range(3):
        torch.matmul(x, wt.T)
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.reps + 2):
        t0 = time.perf_counter()
        for _ in range(L):
            torch.matmul(x, wt.T)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    gemm_ms[what] = float(np.median(ts))
    emit(build=args.label, model="plain f16 GEMM, torch.matmul", case=f"[{T}, {H}] x [{n}, {H}]^T, {L} products", width=what,
         ms_median=round(gemm_ms[what], 3))
wide, narrow = gemm_ms["3H (repeated K/V heads)"], gemm_ms["H + 2 H_kv (grouped-query)"]
emit(build=args.label, model="plain f16 GEMM, torch.matmul", state="grouped-query over repeated", time=round(narrow / wide, 4),
     ms_saved_per_indexing_call=round(wide - narrow, 3))
