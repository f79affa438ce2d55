"""XLM-R models against their BERT counterparts, and the native Unigram tokenizer against HF tokenizers:
python scripts/perf_xlmr.py [--rows N] [--reps R] [--chunks N]

  (a) tokenise --chunks multilingual chunks (~100 words each, 15 languages): vr_unigram_encode against HF tokenizers'
      encode_batch on the same tokenizer.json (tests/golden/xlmr_tokenizer.json: a 702-piece Unigram with a compiled
      charsmap), both on the host threads (VOITTA_HOST_THREADS / RAYON_NUM_THREADS, 16 by default); then again with
      the vocabulary padded to XLM-R's 250,002 pieces by synthetic ones, so the trie has a real vocabulary's size.
  (b) one question from text (vr_query_text) and 1000 questions (vr_query_text_batch), hybrid top-10 over --rows rows
      (bench.py's corpus), with a multilingual-e5-base-shaped encoder (12 x 768, 250,002-row vocabulary, one token
      type, Unigram) and with the BERT e5-base shape (30,522 rows, WordPiece); both f16, random weights. The
      BERT questions get as many words as give about the XLM-R questions' token count (both reported).
  (c) one question x 50 passages (vr_rerank_text(_unigram)) with a bge-reranker-base shape (12 x 768 XLM-R, f16)
      against the same shape as BERT.
One JSON line per measurement; the engine is synchronised around every timed call."""
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
from voitta_rag_amd.unigram import UnigramTokenizer  # noqa: E402
from voitta_rag_amd.wordpiece import WordPieceTokenizer  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--rows", type=int, default=1_000_000)
p.add_argument("--reps", type=int, default=20)
p.add_argument("--chunks", type=int, default=10_000)
args = p.parse_args()
os.environ.setdefault("RAYON_NUM_THREADS", "16")

SPEC = json.load(open(os.path.join(ROOT, "tests", "golden", "xlmr_tokenizer.json"), encoding="utf-8"))
UNI = SPEC["tokenizer"]
SENT = SPEC["texts"][49:]  # the fixture's sentences in 15 languages and its seeded multilingual lines
rng = np.random.default_rng(3)


def out(**kw):
    print(json.dumps(kw, ensure_ascii=False), flush=True)


# ---- (a) tokenizer ---------------------------------------------------------------------------------------------------
words = " ".join(SENT).split()
chunks = [" ".join(rng.choice(words, size=100)) for _ in range(args.chunks)]
uni = UnigramTokenizer.from_tokenizer_json(UNI, 512)
import tokenizers  # noqa: E402

hf = tokenizers.Tokenizer.from_str(json.dumps(UNI))
hf.enable_truncation(max_length=512, strategy="longest_first")
for name, fn in (("(a) native Unigram (vr_unigram_encode)", lambda: uni.encode_batch(chunks)),
                 ("(a) HF tokenizers encode_batch", lambda: hf.encode_batch(chunks))):
    fn()
    t0 = time.perf_counter()
    for _ in range(3):
        fn()
    ms = (time.perf_counter() - t0) / 3 * 1e3
    out(case=name, ms=round(ms, 2), chunks=args.chunks, chunks_per_s=round(args.chunks / ms * 1e3),
        pieces=len(UNI["model"]["vocab"]))
ids, off = uni.encode_batch(chunks)
assert [e.ids for e in hf.encode_batch(chunks[:200])] == [ids[off[i]:off[i + 1]].tolist() for i in range(200)]
# the same with a vocabulary of XLM-R's size (250,002 pieces): the fixture's pieces plus synthetic ones (substrings of the
# chunks' words, "▁"-prefixed or not, scored below every real piece), so the trie has a real vocabulary's breadth
big = json.loads(json.dumps(UNI))
have = {p for p, _ in big["model"]["vocab"]}
floor = min(sc for _, sc in big["model"]["vocab"])
alpha = sorted(set("".join(words)))
extra = []
while len(have) < 250_002:
    w = str(rng.choice(words))
    a = int(rng.integers(0, len(w)))
    piece = ("▁" if rng.random() < 0.5 else "") + w[a:a + int(rng.integers(2, 9))]
    if rng.random() < 0.3:
        piece += "".join(rng.choice(alpha, size=int(rng.integers(1, 4))))
    if piece not in have:
        have.add(piece)
        extra.append([piece, floor - 1.0 - float(rng.random())])
mask = big["model"]["vocab"].pop()  # <mask> stays last
big["model"]["vocab"] += extra + [mask]
for at in big["added_tokens"]:
    if at["content"] == "<mask>":
        at["id"] = len(big["model"]["vocab"]) - 1
uni_big = UnigramTokenizer.from_tokenizer_json(big, 512)
hf_big = tokenizers.Tokenizer.from_str(json.dumps(big))
hf_big.enable_truncation(max_length=512, strategy="longest_first")
n_pieces = len(big["model"]["vocab"])
for name, fn in (("(a) native Unigram (vr_unigram_encode)", lambda: uni_big.encode_batch(chunks)),
                 ("(a) HF tokenizers encode_batch", lambda: hf_big.encode_batch(chunks))):
    fn()
    t0 = time.perf_counter()
    for _ in range(3):
        fn()
    ms = (time.perf_counter() - t0) / 3 * 1e3
    out(case=name, ms=round(ms, 2), chunks=args.chunks, chunks_per_s=round(args.chunks / ms * 1e3), pieces=n_pieces)
ids, off = uni_big.encode_batch(chunks)
assert [e.ids for e in hf_big.encode_batch(chunks[:200])] == [ids[off[i]:off[i + 1]].tolist() for i in range(200)]

# ---- (b) questions from text ----------------------------------------------------------------------------------------
dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev).manual_seed(1234)
SHAPE = dict(layers=12, hidden=768, heads=12, intermediate=3072, max_pos=512, pooling="mean")


def load(e, vocab, xlmr, reranker=False):
    m = dict(SHAPE, vocab=vocab)
    st = bench.random_state(torch, gen, dev, m)
    desc = enc.BertDesc(12, 768, 12, 3072, vocab=vocab, max_pos=512, type_vocab=1 if xlmr else 2,
                        pooling="cls" if reranker else "mean", normalize=not reranker, eps=1e-5 if xlmr else 1e-12,
                        precision="f16")
    if xlmr:
        st["embeddings.token_type_embeddings.weight"] = st["embeddings.token_type_embeddings.weight"][:1].contiguous()
    if reranker:
        st.update({"pooler.dense.weight": torch.randn((768, 768), device=dev, generator=gen) * 0.03,
                   "pooler.dense.bias": torch.zeros(768, device=dev), "classifier.weight": torch.randn((1, 768), device=dev, generator=gen) * 0.03,
                   "classifier.bias": torch.zeros(1, device=dev)})
        enc.load_reranker(e, desc, st)
    else:
        enc.load_encoder(e, desc, st)


bvocab, bwords = bench.synthetic_vocab(rng, 30522)
d = tempfile.mkdtemp(prefix="voitta-perf-")
open(os.path.join(d, "vocab.txt"), "w", encoding="utf-8").write("\n".join(bvocab) + "\n")
wp = WordPieceTokenizer.from_pretrained(d, 512)
uq = [" ".join(rng.choice(words, size=6)) + "?" for _ in range(1000)]
u_tokens = float(np.diff(uni.encode_batch(["query: " + q for q in uq])[1]).mean())
for n_words in range(4, 40):  # BERT questions of about the same token count
    bq = [" ".join(np.array(bwords)[rng.integers(0, len(bwords), size=n_words)]) + "?" for _ in range(1000)]
    if float(np.diff(wp.encode_batch(["query: " + q for q in bq])[1]).mean()) >= u_tokens - 0.5:
        break


def timed(e, name, fn, **kw):
    fn()
    e.sync()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        fn()
    e.sync()
    out(case=name, ms=round((time.perf_counter() - t0) / args.reps * 1e3, 3), **kw)


for label, vocab, xlmr, tok, qs in (("multilingual-e5-base shape (XLM-R, Unigram)", 250_002, True, uni, uq),
                                    ("e5-base shape (BERT, WordPiece)", 30522, False, wp, bq)):
    e = Engine(768, initial_rows=args.rows + 4096)
    load(e, vocab, xlmr)
    bench.populate(torch, gen, dev, e, args.rows, 768)
    texts = ["query: " + q for q in qs]
    _, toff = tok.encode_batch(texts)
    tokens = float(np.diff(toff).mean())
    timed(e, "(b) vr_query_text, 1 question", lambda: e.query_text(tok, texts[0], qs[0], 512, 10), model=label,
          tokens_per_question=round(tokens, 1), rows=args.rows)
    n = len(texts)
    timed(e, "(b) vr_query_text_batch, 1000 questions",
          lambda: e.query_text_batch(tok, texts, qs, 512, [10] * n, [0.1] * n, [None] * n, raw=True), model=label,
          tokens_per_question=round(tokens, 1), rows=args.rows)
    e.close()
    del e
    torch.cuda.empty_cache()

# ---- (c) reranking --------------------------------------------------------------------------------------------------
passages = [" ".join(rng.choice(words, size=int(rng.integers(60, 120)))) for _ in range(50)]
bpass = [" ".join(np.array(bwords)[rng.integers(0, len(bwords), size=int(rng.integers(60, 120)))]) for _ in range(50)]
for label, vocab, xlmr, tok, q, ps in (("bge-reranker-base shape (XLM-R, Unigram)", 250_002, True, uni, uq[0], passages),
                                       ("the same shape as BERT (WordPiece)", 30522, False, wp, bq[0], bpass)):
    e = Engine(768)
    load(e, vocab, xlmr, reranker=True)
    ids, poff, _ = tok.encode_pairs([q] * 50, ps)
    timed(e, "(c) vr_rerank_text, 1 question x 50 passages", lambda: e.rerank_text(tok, [q], [ps], 512), model=label,
          tokens_per_pair=round(float(np.diff(poff).mean()), 1))
    e.close()
