"""Long sequences through the encoder, engine level only, so that the same script measures any build of the library:
python scripts/perf_long.py [--label NAME] [--reps R] [--out FILE]      (VOITTA_ENGINE_LIB selects the library)

The model is the nomic-embed-text shape (12 x 768, 12 heads, I = 3072, rotary, SwiGLU, mean pooling, f16) with seeded
weights and max_pos = 8192. Cases, ids and outputs on the device:
  one sequence of 656, 1024, 2048, 4096 and 8192 tokens; 32 sequences of 2048 tokens;
  2200 chunks of 96..140 tokens, alone (every sequence stages: attention_seq_kernel) and with one 8192-token document
  added. The engine cuts a call into forward chunks of at most 262,144 tokens in sequence order, and 2200 chunks are
  260k tokens: that call runs as TWO forward chunks, the short sequences staged, the document streamed (24 attention
  launches per call), so it does not mix the two kinds.
  2100 of those chunks, alone and with the document FIRST: 256k tokens, one forward chunk, in which the one long
  sequence sends every sequence to the streaming kernel. The script asserts 12 attention launches per call there.
Per case: two warm-up calls, then --reps synchronised calls (median, min, max), then three calls under the engine's own
profiler (VR_PROF_ATTENTION) for attention's time, its share of the call and its TFLOP/s (4 H sum len^2 per layer).
To compare two builds, alternate them in one visit (parent, change, parent, change), each run a process of its own under
its own time limit, and compare the medians against the parent's own min..max. One JSON line per case, also appended to
--out."""
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
p.add_argument("--out", default=None)
args = p.parse_args()
assert args.reps >= 7

dev = torch.device("cuda", 0)
L, H, NH, I, VOCAB = 12, 768, 12, 3072, 30528
g = torch.Generator(device=dev).manual_seed(4321)
desc = enc.BertDesc(L, H, NH, I, vocab=VOCAB, max_pos=8192, pooling="mean", precision="f16", position="rotary",
                    rope_theta=1000.0, ffn="swiglu")
state = {}
for n in (n for n in enc.rope_tensor_names(L) if n is not None):
    t = torch.randn(enc.expected_shape(desc, n), device=dev, generator=g) * 0.02
    state[n] = t + 1.0 if n.lower().endswith("layernorm.weight") else t
e = Engine(H)
enc.load_encoder(e, desc, state)
del state
torch.cuda.empty_cache()

rng = np.random.default_rng(7)
chunks = rng.integers(96, 141, size=2200).tolist()
CASES = [(f"1 x {n}", [n]) for n in (656, 1024, 2048, 4096, 8192)]
CASES += [("32 x 2048", [2048] * 32), ("2200 chunks of 96..140", chunks),
          ("2200 chunks of 96..140 + 1 x 8192", chunks + [8192]), ("2100 chunks of 96..140", chunks[:2100]),
          ("1 x 8192 + 2100 chunks of 96..140, one forward chunk", [8192] + chunks[:2100])]
ONE_FORWARD_CHUNK = 262144  # tokens (kMaxChunkTokens of csrc/encoder.hip)


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


for name, lens in CASES:
    off_h = np.zeros(len(lens) + 1, np.int32)
    off_h[1:] = np.cumsum(lens)
    T = int(off_h[-1])
    ids = torch.from_numpy(rng.integers(0, VOCAB, size=T).astype(np.int32)).to(dev)
    off = torch.from_numpy(off_h).to(dev)
    out = torch.empty((len(lens), H), dtype=torch.float32, device=dev)
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
    e.sync()
    t0 = time.perf_counter()
    for _ in range(3):
        enc.encode(e, ids, off, out=out)
    e.sync()
    wall = time.perf_counter() - t0
    a1 = e.profile_read(Engine.PROF_ATTENTION)
    e.profile(False)
    att_ms, att_flop = (a1[0] - a0[0]) / 3, (a1[2] - a0[2]) / 3
    if "one forward chunk" in name:  # the case is about ONE attention launch per layer over both kinds of sequence
        assert T <= ONE_FORWARD_CHUNK and a1[1] - a0[1] == 3 * L, (T, a1[1] - a0[1])
    t = np.array(times) * 1e3
    emit(build=args.label, case=name, sequences=len(lens), tokens=T, reps=args.reps, ms_median=round(float(np.median(t)), 3),
         ms_min=round(float(t.min()), 3), ms_max=round(float(t.max()), 3), attention_ms=round(att_ms, 3),
         attention_share_of_profiled_call=round(att_ms / (wall / 3 * 1e3), 3),
         attention_tflops=round(att_flop / (att_ms * 1e-3) / 1e12, 1) if att_ms > 0 else None,
         attention_launches_per_call=(a1[1] - a0[1]) // 3)
e.close()
