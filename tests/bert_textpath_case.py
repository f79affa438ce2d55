"""TEST INFRASTRUCTURE — one seeded run of a BERT embedder and a BERT cross-encoder through the engine's text calls
(vr_query_text, vr_query_text_batch, vr_rerank_text with a WordPiece tokenizer). It uses only calls the engine had
before the Unigram tokenizer joined them, so tests/golden/make_bert_textpath_golden.py records it with the library of
that earlier engine (tests/golden/textpath_bert.npz) and tests/test_bert_textpath_gpu.py reruns it on this one:
the refactored text calls must give the same bits."""
from __future__ import annotations

import numpy as np

from oracle import bert as obert

N_ROWS = 2000
N_QUESTIONS = 12


def run() -> dict:
    import rerank_oracle as ro
    from test_query_text_batch_gpu import WORDS, _vocab

    from voitta_rag_amd import Engine, bm25
    from voitta_rag_amd import encoder as enc
    from voitta_rag_amd.wordpiece import WordPieceTokenizer

    rng = np.random.default_rng(2027)
    vocab = _vocab()
    tok = WordPieceTokenizer(vocab, max_length=32)
    out = {}
    # ---- the embedder and a store --------------------------------------------------------------------------------
    shape = obert.BertShape(2, 384, 12, 1536, vocab=len(vocab), max_pos=64)
    e = Engine(384)
    enc.load_encoder(e, enc.BertDesc(2, 384, 12, 1536, vocab=len(vocab), max_pos=64, pooling="mean", precision="f16"),
                     obert.random_weights(shape, 5))
    texts = [" ".join(rng.choice(WORDS, size=int(rng.integers(3, 30)))) for _ in range(N_ROWS)]
    ids, off = tok.encode_batch(["passage: " + t for t in texts])
    x = enc.encode(e, ids, off.astype(np.int32))
    soff, stems = bm25.hashed_stems(texts)
    sp = []
    for i in range(N_ROWS):
        u, cnt = np.unique(stems[soff[i]:soff[i + 1]], return_counts=True)
        sp.append((u.astype(np.int32), (1.0 + np.log1p(cnt)).astype(np.float32)))
    e.upsert(x, sparse=sp)
    questions = [" ".join(rng.choice(WORDS, size=int(rng.integers(2, 9)))) for _ in range(N_QUESTIONS)]
    questions[3] = "the of and"  # stop words only: the dense branch
    dense = ["query: " + q for q in questions]
    limits = rng.integers(1, 40, size=N_QUESTIONS).astype(np.int32)
    (rows, scores, fd, counts, hyb), emb = e.query_text_batch(tok._h, dense, questions, 32, limits, [0.1] * N_QUESTIONS,
                                                              [None] * N_QUESTIONS, raw=True, embeddings=True)
    keep = np.arange(rows.shape[1])[None, :] < counts[:, None]  # (entries past a question's count are unspecified)
    out.update(batch_rows=rows[keep], batch_scores=scores[keep], batch_from_dense=fd[keep], batch_counts=counts,
               batch_hybrid=hyb, batch_embeddings=emb)
    for i in range(3):
        r, s, f, h = e.query_text(tok._h, dense[i], questions[i], 32, 10, 0.1)
        out[f"single{i}_rows"], out[f"single{i}_scores"], out[f"single{i}_hybrid"] = r, s, np.array(h)
    e.close()
    # ---- a cross-encoder -----------------------------------------------------------------------------------------
    rshape = obert.BertShape(2, 384, 12, 1536, vocab=len(vocab), max_pos=128)
    e = Engine(384)
    enc.load_reranker(e, enc.BertDesc(2, 384, 12, 1536, vocab=len(vocab), max_pos=128, type_vocab=2, pooling="cls",
                                      normalize=False, precision="f16"), ro.random_weights(rshape, 31, 40.0))
    cands = [[texts[int(j)] for j in rng.integers(0, N_ROWS, size=n)] for n in (7, 0, 20)]
    out["rerank_logits"] = np.concatenate(e.rerank_text(tok._h, questions[:3], cands, 64))
    e.close()
    return out
