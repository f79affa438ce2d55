"""What the boundary stage of semantic chunking costs: vr_encode_semantic against vr_encode_spans over the same sequences
with the units as spans (the span path is the code from before the feature, unchanged).
python scripts/perf_semantic.py [--layers L] [--repeats R] [--out profiles/semantic_perf.jsonl]

Model: the bge-base shape (12 x 768, 12 heads, FFN 3072), seeded random weights, f16, learned positions (8192 of them, so
that the long document is one sequence). Workloads, token ids seeded:
  chunks-2200   550 sequences of 474 tokens: 4 chunks' worth of ~118 tokens each, 2200 in all, in units of 22..26 tokens
  doc-8192      one sequence of 8192 tokens in units of 22..26 tokens
Both calls return host rows and drain the stream; the two are timed in turn, --repeats times after a warm-up of each, on
a host clock around the call. One JSON line per workload: the medians, their difference (the boundary stage: five short
launches per forward chunk and the copy of the chunk count) and the spread of each series."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

p = argparse.ArgumentParser()
p.add_argument("--layers", type=int, default=12)
p.add_argument("--repeats", type=int, default=12)
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "semantic_perf.jsonl"))
args = p.parse_args()

from voitta_rag_amd import Engine  # noqa: E402
from voitta_rag_amd import encoder as enc  # noqa: E402

H, NH, I, VOCAB, MAX_POS = 768, 12, 3072, 30522, 8192
rng = np.random.default_rng(0)
desc = enc.BertDesc(args.layers, H, NH, I, vocab=VOCAB, max_pos=MAX_POS, pooling="cls", precision="f16")
g = np.random.default_rng(4321)
weights = {}
for name in enc.tensor_names(args.layers):
    t = (g.standard_normal(enc.expected_shape(desc, name), dtype=np.float32) * 0.02).astype(np.float32)
    weights[name] = t + 1.0 if name.lower().endswith("layernorm.weight") else t
e = Engine(H)
enc.load_encoder(e, desc, weights)


def workload(n_seq, length):
    seqs, units = [], []
    for _ in range(n_seq):
        seqs.append(rng.integers(1000, VOCAB, size=length).astype(np.int32))
        own, t = [], 1
        while t < length - 1:
            n = min(int(rng.integers(22, 27)), length - 1 - t)
            own.append((t, t + n))
            t += n
        units.append(own)
    ids = np.concatenate(seqs)
    off = np.arange(n_seq + 1, dtype=np.int32) * length
    unit_off = np.zeros(n_seq + 1, np.int32)
    unit_off[1:] = np.cumsum([len(u) for u in units])
    return ids, off, unit_off, np.asarray([be for own in units for be in own], np.int32)


def timed(call):
    e.sync()
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


PARAMS = dict(buffer=1, break_permille=50, min_distance=0.0, min_tokens=32, max_tokens=256)
for label, n_seq, length in (("chunks-2200", 550, 474), ("doc-8192", 1, 8192)):
    arrays = workload(n_seq, length)
    calls = {"spans": lambda: enc.encode_spans(e, *arrays), "semantic": lambda: enc.encode_semantic(e, *arrays, **PARAMS)}  # noqa: B023
    ms = {k: [] for k in calls}
    for k, c in calls.items():
        timed(c)
        timed(c)
    for _ in range(args.repeats):
        for k, c in calls.items():
            dt, out = timed(c)
            ms[k].append(dt)
    rows, start, dist = calls["semantic"]()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    line = json.dumps(dict(workload=label, layers=args.layers, precision="f16", sequences=n_seq, tokens=int(arrays[1][-1]),
                           units=int(arrays[2][-1]), chunks=int(len(rows)), repeats=args.repeats,
                           spans_ms=round(med["spans"], 3), semantic_ms=round(med["semantic"], 3),
                           boundary_stage_ms=round(med["semantic"] - med["spans"], 3),
                           spans_ms_min_max=[round(min(ms["spans"]), 3), round(max(ms["spans"]), 3)],
                           semantic_ms_min_max=[round(min(ms["semantic"]), 3), round(max(ms["semantic"]), 3)]))
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
e.close()
