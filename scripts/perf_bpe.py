"""The native byte-level BPE tokenizer and the text paths it opens for ModernBERT models:
python scripts/perf_bpe.py [--chunks 10000] [--rows 1000000] [--reps 20] [--out profiles/bpe_perf.jsonl]

One JSON line per measurement, printed and appended to --out. Seeded weights, the fixture tokenizer
(tests/golden/bpe_tokenizer.json: about 600 pieces, so a text makes more tokens than with a released vocabulary), host
clocks around synchronised calls:
  (a) --chunks chunks of 100 words tokenised by vr_bpe_encode on the host threads, and by HF tokenizers' encode_batch
  (b) the ModernBERT-base shape (L 22, H 768, I 1152, window 64, f16) over --rows rows: a question as text in one call
      (vr_query_text_bpe) against the several-call route a model without a native tokenizer takes (the library tokenises,
      vr_encode, vr_search_hybrid); 1000 questions in one vr_query_text_batch_bpe call
  (c) 1 question x 50 passages through the ModernBERT cross-encoder, as text (vr_rerank_text_bpe)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import bench  # noqa: E402
import bpe_case as bc  # noqa: E402
import modernbert_oracle as mo  # noqa: E402
import modernbert_rerank_oracle as mro  # noqa: E402
from make_xlmr_golden import SENTENCES  # noqa: E402
from voitta_rag_amd import Engine  # noqa: E402
from voitta_rag_amd import encoder as enc  # noqa: E402
from voitta_rag_amd.bpe import BpeTokenizer  # noqa: E402
from voitta_rag_amd.sparse_embedding import _query_vector  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--chunks", type=int, default=10_000)
p.add_argument("--rows", type=int, default=1_000_000)
p.add_argument("--reps", type=int, default=20)
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "bpe_perf.jsonl"))
args = p.parse_args()
rng = np.random.default_rng(11)
sink = open(args.out, "a")


def out(**kw):
    line = json.dumps(kw, ensure_ascii=False)
    print(line, flush=True)
    sink.write(line + "\n")
    sink.flush()


# ---- (a) tokenizer ---------------------------------------------------------------------------------------------------
g = bc.fixture()
words = " ".join(SENTENCES).split()
chunks = [" ".join(rng.choice(words, size=100)) for _ in range(args.chunks)]
tok = BpeTokenizer.from_tokenizer_json(g["tokenizer"], 512)
hf = bc.hf_tokenizer(g)
hf.enable_truncation(max_length=512, strategy="longest_first")
for name, fn in (("(a) native byte-level BPE (vr_bpe_encode)", lambda: tok.encode(chunks)),
                 ("(a) HF tokenizers encode_batch", lambda: hf.encode_batch(chunks))):
    fn()
    t0 = time.perf_counter()
    for _ in range(3):
        fn()
    ms = (time.perf_counter() - t0) / 3 * 1e3
    out(case=name, ms=round(ms, 2), chunks=args.chunks, chunks_per_s=round(args.chunks / ms * 1e3),
        pieces=len(g["tokenizer"]["model"]["vocab"]), host_threads=os.cpu_count() if "OMP_NUM_THREADS" not in os.environ
        else int(os.environ["OMP_NUM_THREADS"]))
ids, off = tok.encode(chunks)
assert [e.ids for e in hf.encode_batch(chunks[:200])] == [ids[off[i]:off[i + 1]].tolist() for i in range(200)]
out(case="(a) tokens per chunk", tokens=round(float(np.diff(off).mean()), 1))

# ---- (b) questions from text ----------------------------------------------------------------------------------------
dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev).manual_seed(1234)
vocab = -(-hf.get_vocab_size() // 8) * 8
shape = mo.ModernShape(22, 768, 12, 1152, vocab=vocab, max_pos=512, window=64, global_every=3)


def timed(e, name, fn, **kw):
    fn()
    fn()
    e.sync()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        fn()
    e.sync()
    out(case=name, ms=round((time.perf_counter() - t0) / args.reps * 1e3, 3), **kw)


e = Engine(768, initial_rows=args.rows + 4096)
enc.load_encoder(e, mo.desc_for(shape, "mean", "f16"), mo.random_weights(shape, 5))
bench.populate(torch, gen, dev, e, args.rows, 768)
qs = [" ".join(rng.choice(words, size=6)) + "?" for _ in range(1000)]
_, toff = tok.encode(qs)
tokens = round(float(np.diff(toff).mean()), 1)
label = "ModernBERT-base shape, byte-level BPE"
timed(e, "(b) vr_query_text_bpe, 1 question, one call", lambda: e.query_text(tok, qs[0], qs[0], 512, 10), model=label,
      tokens_per_question=tokens, rows=args.rows)


def several_calls():
    enc_ids = hf.encode(qs[0]).ids
    v = enc.encode(e, np.asarray(enc_ids, np.int32), np.array([0, len(enc_ids)], np.int32))[0]
    qi, qv = _query_vector(qs[0])
    return e.search_hybrid(v, np.asarray(qi, np.int32), np.asarray(qv, np.float32), 10, 0.1)


timed(e, "(b) the several-call route: library tokenise, vr_encode, vr_search_hybrid", several_calls, model=label,
      tokens_per_question=tokens, rows=args.rows)
n = len(qs)
timed(e, "(b) vr_query_text_batch_bpe, 1000 questions",
      lambda: e.query_text_batch(tok, qs, qs, 512, [10] * n, [0.1] * n, [None] * n, raw=True), model=label,
      tokens_per_question=tokens, rows=args.rows)
e.close()
del e
torch.cuda.empty_cache()

# ---- (c) reranking --------------------------------------------------------------------------------------------------
e = Engine(768)
enc.load_reranker(e, mro.desc_for(shape, "mean", "f16"), mro.random_weights(shape, 5, False, 8.0))
for target in (110,):
    n_words = 10
    while True:  # passages of about `target` tokens with this small vocabulary
        passages = [" ".join(rng.choice(words, size=n_words)) for _ in range(50)]
        _, poff, _ = tok.encode_pairs([qs[0]] * 50, passages)
        if float(np.diff(poff).mean()) >= target or n_words > 200:
            break
        n_words += 2
    timed(e, "(c) vr_rerank_text_bpe, 1 question x 50 passages", lambda: e.rerank_text(tok, [qs[0]], [passages], 512),
          model="ModernBERT-base shape cross-encoder", tokens_per_pair=round(float(np.diff(poff).mean()), 1))
e.close()
sink.close()
