"""A rotary, gated-FFN encoder (nomic-embed-text-v1.5 shape) against the BERT shapes of the bench, in one process:
python scripts/perf_rope.py [--chunks N] [--reps R] [--rows N]

  (a) nomic-embed-text-v1.5 shape: 12 x 768, 12 heads, I = 3072, SwiGLU, rotary (theta 1000), mean pooling, f16, as
      shipped: products of at most 256 rows rotate and gate inside the skinny kernels' epilogues, larger ones run
      rope_kernel and glu_kernel as passes of their own.
  (b) the same weights loaded with VR_ENCODE_FUSE=0: the separate passes everywhere. (The indexing step is beyond 256
      rows, so (a) and (b) run the same kernels there; the question is where they differ.)
  (c) the bge-base BERT shape of bench.py (CLS pooling), and (c') the same BERT with mean pooling (e5-base), which
      pools like (a) and so runs the whole last layer on every token as (a) does.
Indexing: vr_encode of --chunks chunks with bench.py's length distribution, ids on the device. The variants ALTERNATE
inside every repetition (a, c, c', a, c, c', ...), after a warm-up of each; medians and the spread (min .. max) over
--reps repetitions. TFLOP/s is computed from shapes: per token and layer 2 (4 H^2 + 3 H I) for the gated model,
2 (4 H^2 + 2 H I) for BERT, plus 4 S H of attention per token (S = the token's sequence length); CLS pooling's
shortened last layer is counted as what it really runs.
Query path: a 12-token question through vr_query_text (tokenise + encode + hybrid top-10 over --rows rows), and the same
12 tokens through vr_encode alone, and 256 tokens (the largest batch the skinny kernels take).
Kernel launches per layer on the query path are COUNTED from a kernel trace, in runs of their own:
  rocprofv3 --kernel-trace --stats -d DIR -o q --output-format csv -- python scripts/perf_rope.py --trace-query a
  python scripts/perf_rope.py --count-launches DIR/q_kernel_stats.csv
--trace-query a|b|c loads that one model ((c) here is the mean-pooled BERT), turns the cached graphs off and encodes the
12-token question TRACE_REPS times; --count-launches adds up the calls of the forward pass's kernels in the stats file
and prints launches per forward pass and per layer (the per-pass kernels — embedding, positions, pooling — taken off).
One JSON line per measurement."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from voitta_rag_amd import Engine  # noqa: E402
from voitta_rag_amd import encoder as enc  # noqa: E402
from voitta_rag_amd.wordpiece import WordPieceTokenizer  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--chunks", type=int, default=2200)
p.add_argument("--reps", type=int, default=7)
p.add_argument("--rows", type=int, default=200_000)
p.add_argument("--trace-query", choices=["a", "b", "c"], default=None)
p.add_argument("--count-launches", metavar="STATS_CSV", default=None)
args = p.parse_args()
TRACE_REPS = 20
FORWARD_KERNELS = ("gemm_f16", "skinny_epilogue", "attention", "layernorm", "rope_kernel", "glu_kernel", "ln_finalize")
PER_PASS_KERNELS = ("embed_ln", "positions_kernel", "pool_kernel")

if args.count_launches:
    import csv

    per_layer, per_pass = {}, {}
    for row in csv.DictReader(open(args.count_launches)):
        name, calls = row["Name"], int(row["Calls"])
        for group, keys in ((per_layer, FORWARD_KERNELS), (per_pass, PER_PASS_KERNELS)):
            for k in keys:
                if k in name:
                    group[k] = group.get(k, 0) + calls
                    break
    total = sum(per_layer.values())
    print(json.dumps({"case": "kernel launches of the 12-token question, counted from the trace", "forward_passes": TRACE_REPS,
                      "layers": 12, "calls_in_the_layers": per_layer, "calls_per_pass_kernels": per_pass,
                      "launches_per_forward_pass": (total + sum(per_pass.values())) / TRACE_REPS,
                      "launches_per_layer": total / TRACE_REPS / 12}))
    sys.exit(0)
if args.trace_query:
    os.environ["VR_ENCODE_GRAPH"] = "0"  # every launch of every pass is its own kernel dispatch in the trace

dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev).manual_seed(1234)
rng = np.random.default_rng(3)
L, H, NH, I, VOCAB = 12, 768, 12, 3072, 30522


def out(**kw):
    print(json.dumps(kw), flush=True)


ROPE_SEED = 4321


def rope_state(fuse=True):
    g = torch.Generator(device=dev).manual_seed(ROPE_SEED)  # (a) and (b): the same weights
    os.environ["VR_ENCODE_FUSE"] = "1" if fuse else "0"     # read when the model is loaded
    names = [n for n in enc.rope_tensor_names(L) if n is not None]
    desc = enc.BertDesc(L, H, NH, I, vocab=VOCAB, max_pos=512, pooling="mean", precision="f16", position="rotary",
                        rope_theta=1000.0, ffn="swiglu")
    st = {}
    for n in names:
        t = torch.randn(enc.expected_shape(desc, n), device=dev, generator=g) * 0.02
        st[n] = t + 1.0 if n.lower().endswith("layernorm.weight") else t
    return desc, st


def bert_state(pooling):
    desc = enc.BertDesc(L, H, NH, I, vocab=VOCAB, max_pos=512, pooling=pooling, precision="f16")
    return desc, bench.random_state(torch, gen, dev, dict(layers=L, hidden=H, heads=NH, intermediate=I, vocab=VOCAB, max_pos=512))


VARIANTS = [("(a) nomic-embed-text-v1.5 shape, rotary + SwiGLU, fused skinny epilogues", lambda: rope_state(True), 3, "mean"),
            ("(b) the same, VR_ENCODE_FUSE=0: separate passes everywhere", lambda: rope_state(False), 3, "mean"),
            ("(c) bge-base shape, BERT, CLS pooling", lambda: bert_state("cls"), 2, "cls"),
            ("(c') e5-base shape, BERT, mean pooling", lambda: bert_state("mean"), 2, "mean")]

if args.trace_query:
    VARIANTS = [VARIANTS[{"a": 0, "b": 1, "c": 3}[args.trace_query]]]
engines = []
for label, make, ffn_mats, pooling in VARIANTS:
    e = Engine(H, initial_rows=args.rows + 4096)
    desc, st = make()
    enc.load_encoder(e, desc, st)
    os.environ.pop("VR_ENCODE_FUSE", None)
    del st
    engines.append(e)
torch.cuda.empty_cache()

if args.trace_query:
    bvocab, _ = bench.synthetic_vocab(rng, VOCAB)
    qids = np.concatenate([[101], rng.integers(1000, VOCAB, size=10), [102]]).astype(np.int32)
    for _ in range(TRACE_REPS):
        enc.encode(engines[0], qids, np.array([0, 12], np.int32))
    engines[0].sync()
    engines[0].close()
    sys.exit(0)

# ---- indexing -----------------------------------------------------------------------------------------------------------
ids, off, _, _, T = bench.make_batch(torch, gen, dev, args.chunks, 0)
lens = np.diff(off.cpu().numpy()).astype(np.float64)
outs = [torch.empty((args.chunks, H), dtype=torch.float32, device=dev) for _ in engines]


def flop(ffn_mats, pooling):
    per_tok_layer = 2.0 * (4 * H * H + ffn_mats * H * I)
    full = (L if pooling == "mean" else L - 1) * (T * per_tok_layer + 4.0 * H * float((lens * lens).sum()))
    if pooling == "cls":  # last layer: Q/K/V on every token, attention for one query block, the rest on one row per chunk
        full += T * 2.0 * 3 * H * H + 4.0 * H * float((np.minimum(lens, 64) * lens).sum())
        full += args.chunks * 2.0 * (H * H + ffn_mats * H * I)
    return full


times = [[] for _ in engines]
for rep in range(args.reps + 2):  # two warm-up rounds (workspace allocation, first-use costs)
    for k, e in enumerate(engines):
        e.sync()
        t0 = time.perf_counter()
        enc.encode(e, ids, off, out=outs[k])
        e.sync()
        if rep >= 2:
            times[k].append(time.perf_counter() - t0)
for k, (label, _, ffn_mats, pooling) in enumerate(VARIANTS):
    t = np.array(times[k])
    med = float(np.median(t))
    out(case="indexing: vr_encode", model=label, chunks=args.chunks, tokens=T, reps=args.reps, ms_median=round(med * 1e3, 3),
        ms_min=round(float(t.min()) * 1e3, 3), ms_max=round(float(t.max()) * 1e3, 3),
        chunks_per_s=round(args.chunks / med), encoder_tflops=round(flop(ffn_mats, pooling) / med / 1e12, 1))

# ---- the query path ---------------------------------------------------------------------------------------------------
bvocab, bwords = bench.synthetic_vocab(rng, VOCAB)
d = tempfile.mkdtemp(prefix="voitta-perf-")
open(os.path.join(d, "vocab.txt"), "w", encoding="utf-8").write("\n".join(bvocab) + "\n")
wp = WordPieceTokenizer.from_pretrained(d, 512)
question = None
for n_words in range(2, 12):
    for _ in range(200):
        q = " ".join(np.array(bwords)[rng.integers(0, len(bwords), size=n_words)]) + "?"
        if int(np.diff(wp.encode_batch([q])[1])[0]) == 12:
            question = q
            break
    if question:
        break
assert question is not None
qids, qoff = wp.encode_batch([question])
qoff = qoff.astype(np.int32)
for e in engines:
    bench.populate(torch, gen, dev, e, args.rows, H)
# the largest batch the skinny kernels take: 256 tokens, the first chunk and the head of the second
off_h, ids_h = off.cpu().numpy(), ids.cpu().numpy()
soff = np.array([0, off_h[1], 256], np.int32)
sids = np.ascontiguousarray(ids_h[:256])
qt = [[] for _ in engines]
qe = [[] for _ in engines]
qs = [[] for _ in engines]
for rep in range(args.reps * 4 + 3):  # (the third call of a shape replays its captured graph)
    for k, e in enumerate(engines):
        e.sync()
        t0 = time.perf_counter()
        e.query_text(wp, question, question, 512, 10)
        e.sync()
        t1 = time.perf_counter()
        enc.encode(e, qids, qoff)
        e.sync()
        t2 = time.perf_counter()
        enc.encode(e, sids, soff)
        e.sync()
        t3 = time.perf_counter()
        if rep >= 3:
            qt[k].append(t1 - t0)
            qe[k].append(t2 - t1)
            qs[k].append(t3 - t2)
for k, (label, _, ffn_mats, _) in enumerate(VARIANTS):
    a, b, c = np.array(qt[k]) * 1e3, np.array(qe[k]) * 1e3, np.array(qs[k]) * 1e3
    out(case="query: 12-token question", model=label, rows=args.rows, reps=len(a),
        query_text_ms_median=round(float(np.median(a)), 4), query_text_ms_min=round(float(a.min()), 4),
        query_text_ms_max=round(float(a.max()), 4), encode_ms_median=round(float(np.median(b)), 4),
        encode_ms_min=round(float(b.min()), 4), encode_ms_max=round(float(b.max()), 4),
        encode_256_tokens_ms_median=round(float(np.median(c)), 4), encode_256_tokens_ms_min=round(float(c.min()), 4),
        encode_256_tokens_ms_max=round(float(c.max()), 4))
for e in engines:
    e.close()
