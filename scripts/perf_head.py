"""A bge-base-shaped encoder, engine level only: what a post-pooling head (vr_encoder_set_head) costs, and what a narrower
store is worth to a query.
python scripts/perf_head.py [--label NAME] [--reps R] [--rounds N] [--rows N] [--out FILE]   (VOITTA_ENGINE_LIB selects the library)

The model is the bge-base-en-v1.5 shape (12 x 768, 12 heads, I = 3072, post-norm, GELU, CLS pooling, f16) with seeded
weights; ids and outputs on the device. ONE engine, ONE loaded model: the yardstick is the same engine with
set_encoder_head(None), alternated --rounds times in this process with each of two heads, so all states see the same
box, clocks and neighbours:
  dense     Dense 768 -> 768 tanh + bias, then the description's normalisation (a LaBSE-style head: one embed_head_kernel
            launch per forward chunk)
  truncate  no stages, truncate_dim 256 (pool_kernel stores fewer columns; no launch more)
Cases: 2200 chunks of 96..140 tokens (the bench's chunk lengths) and one 12-token question (the cached graph's replay;
time per call). Per case, state and round: two warm-up calls, then --reps synchronised calls. Reported per case and
state: the median over all rounds' calls, min and max, and each head over no head.
Then (--rows > 0) the hybrid top-10 query over --rows random rows at store widths 256 and 768: p50 and p99 of 200 calls.
The head launch's own time is not measured here: run this script under a kernel trace in a run of its own and read
embed_head_kernel's row. One JSON line per measurement, also appended to --out."""
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
p.add_argument("--rows", type=int, default=1_000_000)
p.add_argument("--out", default="profiles/head_perf.jsonl")
args = p.parse_args()
assert args.reps >= 3 and args.rounds >= 2

dev = torch.device("cuda", 0)
L, H, NH, I, VOCAB, MAX_SEQ = 12, 768, 12, 3072, 30522, 512
g = torch.Generator(device=dev).manual_seed(4321)


def rand(*shape, std=0.02):
    return (torch.randn(shape, device=dev, generator=g) * std).cpu().numpy()


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


state = {"embeddings.word_embeddings.weight": rand(VOCAB, H), "embeddings.position_embeddings.weight": rand(MAX_SEQ, H),
         "embeddings.token_type_embeddings.weight": rand(2, H), "embeddings.LayerNorm.weight": 1.0 + rand(H),
         "embeddings.LayerNorm.bias": rand(H)}
for i in range(L):
    q = f"encoder.layer.{i}."
    for n, shape in (("attention.self.query", (H, H)), ("attention.self.key", (H, H)), ("attention.self.value", (H, H)),
                     ("attention.output.dense", (H, H)), ("intermediate.dense", (I, H)), ("output.dense", (H, I))):
        state[q + n + ".weight"], state[q + n + ".bias"] = rand(*shape), rand(shape[0])
    for n in ("attention.output.LayerNorm", "output.LayerNorm"):
        state[q + n + ".weight"], state[q + n + ".bias"] = 1.0 + rand(H), rand(H)
desc = enc.BertDesc(L, H, NH, I, vocab=VOCAB, max_pos=MAX_SEQ, type_vocab=2, pooling="cls", precision="f16", eps=1e-12)
HEADS = {"none": (None, 0),
         "dense": ([enc.HeadStage("dense", rand(H, H, std=H ** -0.5), rand(H, std=0.1), activation="tanh")], 0),
         "truncate": ([], 256)}

rng = np.random.default_rng(7)
CASES = [("2200 chunks of 96..140", rng.integers(96, 141, size=2200).tolist()), ("1 question of 12", [12])]
INPUTS = {}
for name, lens in CASES:
    off_h = np.zeros(len(lens) + 1, np.int32)
    off_h[1:] = np.cumsum(lens)
    INPUTS[name] = (torch.from_numpy(rng.integers(4, VOCAB, size=int(off_h[-1])).astype(np.int32)).to(dev),
                    torch.from_numpy(off_h).to(dev), len(lens))

e = Engine(H)
enc.load_encoder(e, desc, state)
times = {(name, s): [] for name, _ in CASES for s in HEADS}
for rnd in range(args.rounds):
    order = list(HEADS) if rnd % 2 == 0 else list(HEADS)[::-1]
    for s in order:
        e.set_encoder_head(*HEADS[s])
        width = e.encoder_desc.out_dim
        for name, _ in CASES:
            ids, off, n = INPUTS[name]
            out = torch.empty((n, width), dtype=torch.float32, device=dev)
            for rep in range(args.reps + 2):
                e.sync()
                t0 = time.perf_counter()
                enc.encode(e, ids, off, out=out)
                e.sync()
                if rep >= 2:
                    times[name, s].append(time.perf_counter() - t0)
            assert bool(torch.isfinite(out).all())
e.close()

for name, lens in CASES:
    med = {}
    for s in HEADS:
        t = np.array(times[name, s]) * 1e3
        med[s] = float(np.median(t))
        emit(build=args.label, state=s, case=name, sequences=len(lens), tokens=int(sum(lens)), calls=len(t),
             ms_median=round(med[s], 4), ms_min=round(float(t.min()), 4), ms_max=round(float(t.max()), 4),
             sequences_per_s=round(len(lens) / med[s] * 1e3, 1))
    for s in ("dense", "truncate"):
        emit(build=args.label, state=s + " over none", case=name, call_time=round(med[s] / med["none"], 4))

# ---- what the store's width is worth: hybrid top-10 over --rows rows -----------------------------------------------------
if args.rows > 0:
    nnz_per = 40
    qi, qv = np.array([5, 1000, 20000, 150000, 77], np.int32), np.ones(5, np.float32)
    for dim in (768, 256):
        e = Engine(dim, initial_rows=args.rows)
        gs = torch.Generator(device=dev).manual_seed(1)
        for a in range(0, args.rows, 100_000):
            b = min(args.rows, a + 100_000)
            x = torch.nn.functional.normalize(torch.randn((b - a, 768), device=dev, generator=gs), dim=1)[:, :dim].contiguous()
            ids = (torch.rand((b - a, nnz_per), device=dev, generator=gs) ** 3 * 200_000).to(torch.int32)
            ids = torch.sort(ids, dim=1)[0] + torch.arange(nnz_per, device=dev, dtype=torch.int32)[None, :]
            off = (torch.arange(b - a + 1, device=dev, dtype=torch.int64) * nnz_per).contiguous()
            val = torch.rand(((b - a) * nnz_per,), device=dev, generator=gs) + 0.5
            e.upsert(x, sparse=(off, ids.reshape(-1).contiguous(), val.contiguous()))
        e.sync()
        qs = torch.nn.functional.normalize(torch.randn((201, 768), device=dev, generator=gs), dim=1)[:, :dim].cpu().numpy()
        ts = []
        for i in range(201):
            t0 = time.perf_counter()
            e.search_hybrid(qs[i], qi + i, qv, 10, 0.1)
            ts.append(time.perf_counter() - t0)
        ts = np.array(ts[1:]) * 1e3
        emit(build=args.label, case=f"hybrid top-10 over {args.rows} rows", store_width=dim, calls=len(ts),
             ms_p50=round(float(np.percentile(ts, 50)), 4), ms_p99=round(float(np.percentile(ts, 99)), 4))
        e.close()
