"""A ModernBERT-base-shaped encoder, engine level only:
python scripts/perf_modernbert.py [--label NAME] [--reps R] [--out FILE]      (VOITTA_ENGINE_LIB selects the library)

The model is the ModernBERT-base shape (22 x 768, 12 heads, I = 1152, pre-norm, GeGLU, window half-width 64, every third
layer global, bases 160000 / 10000, mean pooling, f16) with seeded weights and max_pos = 8192; ids and outputs on the
device. Three models of the same weights are loaded in turn, in one process:
  windowed        the description above: 8 global and 14 windowed layers
  global          window = 0: 22 global layers, whose attention launches are the kernels a post-norm model runs
  windowed/staged and windowed/streamed: the first again with VR_WINDOW_STREAM_FROM (read when a model is loaded) moved
                  so that the windowed layers of every stageable sequence take attention_seq_kernel, or
                  attention_stream_kernel — the routing decision, measured at 512 tokens
Cases: 2200 chunks of 96..140 tokens (the bench's chunk lengths; chunks/s), and one sequence of 512, 2048 and 8192
tokens (time per sequence). Per case and model: two warm-up calls, then --reps synchronised calls (median, min, max),
then three calls under the engine's own profiler for attention's time. Per-launch attention time: a global layer's is
the global model's attention time / 22; a windowed layer's is (the windowed model's - 8 global launches) / 14. One JSON
line per case and model, also appended to --out."""
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
p.add_argument("--reps", type=int, default=7)
p.add_argument("--out", default="profiles/modernbert_perf.jsonl")
args = p.parse_args()
assert args.reps >= 7

dev = torch.device("cuda", 0)
L, H, NH, I, VOCAB, W, EVERY = 22, 768, 12, 1152, 50368, 64, 3
N_GLOBAL = len(range(0, L, EVERY))
g = torch.Generator(device=dev).manual_seed(4321)


def describe(**over):
    fields = dict(vocab=VOCAB, max_pos=8192, type_vocab=1, pooling="mean", precision="f16", position="rotary",
                  rope_theta=160000.0, ffn="geglu", norm="pre", eps=1e-5, window=W, global_every=EVERY, rope_theta_local=10000.0)
    fields.update(over)
    return enc.BertDesc(L, H, NH, I, **fields)


state = {"embeddings.tok_embeddings.weight": torch.randn((VOCAB, H), device=dev, generator=g) * 0.02}
for name in ["embeddings.norm", "final_norm"] + [f"layers.{i}.{n}" for i in range(L) for n in ("attn_norm", "mlp_norm")]:
    if name != "layers.0.attn_norm":
        state[name + ".weight"] = 1.0 + torch.randn(H, device=dev, generator=g) * 0.02
for i in range(L):
    for n, shape in (("attn.Wqkv", (3 * H, H)), ("attn.Wo", (H, H)), ("mlp.Wi", (2 * I, H)), ("mlp.Wo", (H, I))):
        state[f"layers.{i}.{n}.weight"] = torch.randn(shape, device=dev, generator=g) * 0.02
state = {k: v.cpu().numpy() for k, v in state.items()}  # (the loader fills the absent slots with host arrays)

rng = np.random.default_rng(7)
chunks = rng.integers(96, 141, size=2200).tolist()
CASES = [("2200 chunks of 96..140", chunks)] + [(f"1 x {n}", [n]) for n in (512, 2048, 8192)]
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


def measure(model, desc, cases, stream_from=None):
    if stream_from is None:
        os.environ.pop("VR_WINDOW_STREAM_FROM", None)
    else:
        os.environ["VR_WINDOW_STREAM_FROM"] = str(stream_from)
    e = Engine(H)
    enc.load_encoder(e, desc, state)
    results = {}
    for name in cases:
        ids, off, out = INPUTS[name]
        n_seq, T = int(off.shape[0]) - 1, int(ids.shape[0])
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
        assert a1[1] - a0[1] == 3 * L, a1[1] - a0[1]  # one forward chunk, one attention launch per layer
        t = np.array(times) * 1e3
        results[name] = (float(np.median(t)), (a1[0] - a0[0]) / 3)
        emit(build=args.label, model=model, case=name, sequences=n_seq, tokens=T, reps=args.reps,
             ms_median=round(float(np.median(t)), 3), ms_min=round(float(t.min()), 3), ms_max=round(float(t.max()), 3),
             sequences_per_s=round(n_seq / float(np.median(t)) * 1e3, 1), attention_ms_per_call=round(results[name][1], 3))
    e.close()
    return results


names = [c for c, _ in CASES]
windowed = measure("windowed", describe(), names)
glob = measure("global", describe(window=0, global_every=0, rope_theta_local=0.0), names)
for name in names:
    per_global = glob[name][1] / L
    per_windowed = (windowed[name][1] - N_GLOBAL * per_global) / (L - N_GLOBAL)
    emit(build=args.label, model="per attention launch", case=name, global_layer_ms=round(per_global, 4),
         windowed_layer_ms=round(per_windowed, 4), global_over_windowed=round(per_global / per_windowed, 2))
short = ["2200 chunks of 96..140", "1 x 512"]
staged = measure("windowed/staged", describe(), short, stream_from=1 << 30)
streamed = measure("windowed/streamed", describe(), short, stream_from=1)
for name in short:
    per_global = glob[name][1] / L
    emit(build=args.label, model="routing of windowed layers", case=name,
         staged_layer_ms=round((staged[name][1] - N_GLOBAL * per_global) / (L - N_GLOBAL), 4),
         streamed_layer_ms=round((streamed[name][1] - N_GLOBAL * per_global) / (L - N_GLOBAL), 4),
         staged_call_ms=round(staged[name][0], 3), streamed_call_ms=round(streamed[name][0], 3))
