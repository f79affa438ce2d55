"""A jina-embeddings-v2-base-shaped encoder, engine level only: what the linear (ALiBi) attention bias costs.
python scripts/perf_alibi.py [--label NAME] [--reps R] [--rounds N] [--out FILE]   (VOITTA_ENGINE_LIB selects the library)

The model is the jina-embeddings-v2-base-en shape (12 x 768, 12 heads, I = 3072, post-norm, GeGLU, no positions, two
token types, mean pooling, f16, sequences of up to 8192 tokens) with seeded weights under JinaBert's names and the
standard slopes (encoder.alibi_slopes(12)); ids and outputs on the device. ONE engine, ONE loaded model: the yardstick
is the same engine with set_attention_slopes(None), alternated with the biased state --rounds times in this process, so
both states see the same box, clocks and neighbours.
Cases: 2200 chunks of 96..140 tokens (the bench's chunk lengths; the staged attention kernel), 600 chunks of 384 tokens
(staged), one sequence of 8192 tokens (the streamed kernel) and one 12-token question (the cached graph's replay; time
per call). Per case, state and round: two warm-up calls, then --reps synchronised calls; then three calls under the
engine's own profiler for attention's time (12 launches per call). Reported per case and state: the median over all
rounds' calls, min and max, the per-launch attention time and which kernel it is, and biased over unbiased for both.
One JSON line per case and state, also appended to --out."""
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
p.add_argument("--rounds", type=int, default=3)
p.add_argument("--out", default="profiles/alibi_perf.jsonl")
args = p.parse_args()
assert args.reps >= 3 and args.rounds >= 2

dev = torch.device("cuda", 0)
L, H, NH, I, VOCAB, MAX_SEQ = 12, 768, 12, 3072, 30528, 8192
g = torch.Generator(device=dev).manual_seed(4321)


def rand(*shape, std=0.02):
    return (torch.randn(shape, device=dev, generator=g) * std).cpu().numpy()


state = {"embeddings.word_embeddings.weight": rand(VOCAB, H), "embeddings.token_type_embeddings.weight": rand(2, H),
         "embeddings.LayerNorm.weight": 1.0 + rand(H), "embeddings.LayerNorm.bias": rand(H)}
for i in range(L):
    q = f"encoder.layer.{i}."
    for n in ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense"):
        state[q + n + ".weight"], state[q + n + ".bias"] = rand(H, H), rand(H)
    state[q + "mlp.gated_layers.weight"] = rand(2 * I, H)
    state[q + "mlp.wo.weight"], state[q + "mlp.wo.bias"] = rand(H, I), rand(H)
    for n in ("attention.output.LayerNorm", "mlp.layernorm"):
        state[q + n + ".weight"], state[q + n + ".bias"] = 1.0 + rand(H), rand(H)
desc = enc.BertDesc(L, H, NH, I, vocab=VOCAB, max_pos=MAX_SEQ, type_vocab=2, pooling="mean", precision="f16", eps=1e-12,
                    position="none", ffn="geglu")
SLOPES = enc.alibi_slopes(NH)

rng = np.random.default_rng(7)
CASES = [("2200 chunks of 96..140", rng.integers(96, 141, size=2200).tolist(), "staged"),
         ("600 chunks of 384", [384] * 600, "staged"), ("1 sequence of 8192", [8192], "streamed"),
         ("1 question of 12", [12], "staged")]
INPUTS = {}
for name, lens, _ in CASES:
    off_h = np.zeros(len(lens) + 1, np.int32)
    off_h[1:] = np.cumsum(lens)
    INPUTS[name] = (torch.from_numpy(rng.integers(4, VOCAB, size=int(off_h[-1])).astype(np.int32)).to(dev),
                    torch.from_numpy(off_h).to(dev), torch.empty((len(lens), H), dtype=torch.float32, device=dev))


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


e = Engine(H)
enc.load_encoder(e, desc, state)
times = {(name, s): [] for name, _, _ in CASES for s in ("biased", "unbiased")}
attention = {k: [] for k in times}
outputs = {}
for rnd in range(args.rounds):
    for s in ("biased", "unbiased") if rnd % 2 == 0 else ("unbiased", "biased"):
        e.set_attention_slopes(SLOPES if s == "biased" else None)
        for name, _, _ in CASES:
            ids, off, out = INPUTS[name]
            for rep in range(args.reps + 2):
                e.sync()
                t0 = time.perf_counter()
                enc.encode(e, ids, off, out=out)
                e.sync()
                if rep >= 2:
                    times[name, s].append(time.perf_counter() - t0)
            assert bool(torch.isfinite(out).all())
            outputs[name, s] = out[:4].cpu().numpy()
            e.profile(True)
            a0 = e.profile_read(Engine.PROF_ATTENTION)
            for _ in range(3):
                enc.encode(e, ids, off, out=out)
            e.sync()
            a1 = e.profile_read(Engine.PROF_ATTENTION)
            e.profile(False)
            # one forward chunk, one attention launch per layer (a pass the profiler does not see launch by launch: nan)
            attention[name, s].append((a1[0] - a0[0]) / (3 * L) if a1[1] - a0[1] == 3 * L else float("nan"))
e.close()

for name, lens, kernel in CASES:
    assert not np.array_equal(outputs[name, "biased"], outputs[name, "unbiased"])  # the two states are two models
    med = {}
    for s in ("biased", "unbiased"):
        t = np.array(times[name, s]) * 1e3
        med[s] = (float(np.median(t)), float(np.median(attention[name, s])))
        emit(build=args.label, state=s, case=name, sequences=len(lens), tokens=int(sum(lens)), calls=len(t),
             ms_median=round(med[s][0], 3), ms_min=round(float(t.min()), 3), ms_max=round(float(t.max()), 3),
             sequences_per_s=round(len(lens) / med[s][0] * 1e3, 1), attention_kernel=kernel,
             attention_launch_ms=round(med[s][1], 4))
    emit(build=args.label, state="biased over unbiased", case=name, call_time=round(med["biased"][0] / med["unbiased"][0], 4),
         attention_kernel=kernel, attention_launch=round(med["biased"][1] / med["unbiased"][1], 4))
