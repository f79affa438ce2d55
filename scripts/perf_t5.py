"""A gtr-t5-base-shaped encoder, engine level only: what a T5 encoder costs, and what its bias table costs.
python scripts/perf_t5.py [--label NAME] [--reps R] [--rounds N] [--out FILE]   (VOITTA_ENGINE_LIB selects the library)

The model is the gtr-t5-base shape (12 x 768, 12 heads of 64, d_ff 3072, RMSNorm pre-norm, ReLU FFN without biases, no
positions, vocabulary 32128, mean pooling, f16) with seeded weights under T5EncoderModel's names, loaded through
encoder.t5_slots (the query fold, the NULL slots) with its own relative-position table (radius 128); ids and outputs on
the device. No Dense head: the head's cost is profiles/head_perf.jsonl's. ONE engine, ONE loaded model: the yardstick for
the table is the same engine with set_attention_bias(None), alternated with the biased state --rounds times in this
process, so both states see the same box, clocks and neighbours.
Cases: 2200 chunks of 96..140 tokens (~118: the bench's chunk lengths) and one 12-token question (the folded-RMSNorm
route, the cached graph's replay; time per call). Per case, state and round: two warm-up calls, then --reps synchronised
calls. Reported per case and state: the median over all rounds' calls, min and max, and biased over unbiased.
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
p.add_argument("--out", default="profiles/t5_perf.jsonl")
args = p.parse_args()
assert args.reps >= 3 and args.rounds >= 2

dev = torch.device("cuda", 0)
L, H, NH, I, VOCAB, MAX_SEQ = 12, 768, 12, 3072, 32128, 512
DKV = H // NH
g = torch.Generator(device=dev).manual_seed(4321)


def rand(*shape, std=0.02):
    return (torch.randn(shape, device=dev, generator=g) * std).cpu().numpy()


state = {"shared.weight": rand(VOCAB, H, std=1.0), "encoder.final_layer_norm.weight": 1.0 + rand(H)}
for i in range(L):
    b = f"encoder.block.{i}.layer."
    state[b + "0.SelfAttention.q.weight"] = rand(H, H, std=(H * DKV) ** -0.5)  # T5's initialiser: logits of order one
    for n in ("k", "v", "o"):
        state[b + f"0.SelfAttention.{n}.weight"] = rand(H, H, std=H ** -0.5)
    state[b + "1.DenseReluDense.wi.weight"] = rand(I, H, std=H ** -0.5)
    state[b + "1.DenseReluDense.wo.weight"] = rand(H, I, std=I ** -0.5)
    state[b + "0.layer_norm.weight"], state[b + "1.layer_norm.weight"] = 1.0 + rand(H), 1.0 + rand(H)
state["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"] = rand(32, NH, std=1.0)
desc = enc.BertDesc(L, H, NH, I, vocab=VOCAB, max_pos=MAX_SEQ, type_vocab=1, pooling="mean", precision="f16", eps=1e-6,
                    position="none", ffn="relu", norm="rms_pre")
TABLE = enc.t5_bias_table(state["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"])

rng = np.random.default_rng(7)
CASES = [("2200 chunks of 96..140", rng.integers(96, 141, size=2200).tolist()), ("1 question of 12", [12])]
INPUTS = {}
for name, lens in CASES:
    off_h = np.zeros(len(lens) + 1, np.int32)
    off_h[1:] = np.cumsum(lens)
    INPUTS[name] = (torch.from_numpy(rng.integers(0, VOCAB, size=int(off_h[-1])).astype(np.int32)).to(dev),
                    torch.from_numpy(off_h).to(dev), torch.empty((len(lens), H), dtype=torch.float32, device=dev))


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


e = Engine(H)
enc.load_encoder(e, desc, state)
times = {(name, s): [] for name, _ in CASES for s in ("biased", "unbiased")}
outputs = {}
for rnd in range(args.rounds):
    for s in ("biased", "unbiased") if rnd % 2 == 0 else ("unbiased", "biased"):
        e.set_attention_bias(TABLE if s == "biased" else None)
        for name, _ in CASES:
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
e.close()

for name, lens in CASES:
    assert not np.array_equal(outputs[name, "biased"], outputs[name, "unbiased"])  # the two states are two models
    med = {}
    for s in ("biased", "unbiased"):
        t = np.array(times[name, s]) * 1e3
        med[s] = float(np.median(t))
        emit(build=args.label, model="gtr-t5-base shape, f16", state=s, case=name, sequences=len(lens), tokens=int(sum(lens)),
             calls=len(t), ms_median=round(med[s], 3), ms_min=round(float(t.min()), 3), ms_max=round(float(t.max()), 3),
             sequences_per_s=round(len(lens) / med[s] * 1e3, 1))
    emit(build=args.label, model="gtr-t5-base shape, f16", state="biased over unbiased", case=name,
         call_time=round(med["biased"] / med["unbiased"], 4))
