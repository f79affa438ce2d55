"""Late chunking through BulkIndexer against plain indexing, on one synthetic corpus:
python scripts/perf_late.py [--docs N] [--layers L] [--out profiles/late_chunking_perf.jsonl] [--models bge,nomic]
                              [--runs off,late-2048,late-8192] [--label NAME]

Models (seeded random weights, a synthetic 40k-word WordPiece vocabulary, f16):
  bge    bge-base-shaped BERT, 12 x 768, [CLS] pooling, 512 learned positions — its window is 512 whatever the cap;
  nomic  nomic-embed-text-shaped, 12 x 768, rotary, SwiGLU, mean pooling, 8192 positions (scripts/perf_long.py's model).
Corpus: --docs documents of about 500, 2000 and 8000 tokens in turn, chunked at 512 characters with overlap 50.
Runs, each a process of its own (the settings are read once per process), in this order and then once more in the same
order, so that every configuration is measured twice and drift shows:
  off        VOITTA_LATE_CHUNKING unset: the plain path, the behaviour before the setting existed
  late-2048  VOITTA_LATE_CHUNKING=1, VOITTA_MAX_SEQ_LENGTH=2048
  late-8192  VOITTA_LATE_CHUNKING=1, VOITTA_MAX_SEQ_LENGTH=8192
Per run: a warm-up pass over the first documents, one timed pass (chunks/s, encoder tokens/s, sequences), then one pass
under the engine's profiler (vr_profile: GEMM and attention milliseconds; it keeps small passes out of the graph cache, so
it is not the timed pass). One JSON line per run, appended to --out. `--runs off` is all a build from before the setting
existed can do: copied into such a tree, the script measures that build's plain path for comparison (--label names it)."""
import argparse
import json
import os
import pathlib
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

p = argparse.ArgumentParser()
p.add_argument("--docs", type=int, default=90)
p.add_argument("--layers", type=int, default=12)
p.add_argument("--out", default=os.path.join(ROOT, "profiles", "late_chunking_perf.jsonl"))
p.add_argument("--models", default="bge,nomic")
p.add_argument("--runs", default="off,late-2048,late-8192")
p.add_argument("--label", default="change")
p.add_argument("--child", default=None, help="internal: MODEL:RUN:CHECKPOINT, one run in this process")
args = p.parse_args()

H, NH, I = 768, 12, 3072
rng = np.random.default_rng(0)
letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))
words = sorted({"".join(rng.choice(letters, size=int(rng.integers(1, 7)))) for _ in range(40000)})
vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + list("abcdefghijklmnopqrstuvwxyz0123456789.,!?:;'-")
vocab = list(dict.fromkeys(vocab + ["##" + c for c in "abcdefghijklmnopqrstuvwxyz0123456789"] + words))
warr = np.array(words)


def document(n_words):
    out, n = [], 0
    while n < n_words:
        sents = []
        for _ in range(int(rng.integers(1, 5))):
            k = int(rng.integers(5, 25))
            sents.append(" ".join(rng.choice(warr, size=k)).capitalize() + ".")
            n += k
        out.append(" ".join(sents))
    return "\n\n".join(out)


def checkpoint(model, d):
    """A sentence-transformers directory of the model's shape with seeded weights."""
    from safetensors.numpy import save_file

    from voitta_rag_amd import encoder as enc

    (d / "1_Pooling").mkdir(parents=True)
    cfg = {"hidden_size": H, "num_hidden_layers": args.layers, "num_attention_heads": NH, "intermediate_size": I,
           "vocab_size": len(vocab), "type_vocab_size": 2, "layer_norm_eps": 1e-12}
    if model == "bge":
        cfg.update(model_type="bert", max_position_embeddings=512, hidden_act="gelu")
        desc = enc.BertDesc(args.layers, H, NH, I, vocab=len(vocab), max_pos=512, pooling="cls")
        names, prefix = enc.tensor_names(args.layers), "bert."
    else:
        cfg.update(model_type="nomic_bert", max_position_embeddings=8192, hidden_act="silu", head_dim=H // NH,
                   rope_parameters={"rope_type": "default", "rope_theta": 1000.0})
        desc = enc.BertDesc(args.layers, H, NH, I, vocab=len(vocab), max_pos=8192, pooling="mean", position="rotary",
                            rope_theta=1000.0, ffn="swiglu")
        names, prefix = [n for n in enc.rope_tensor_names(args.layers) if n is not None], ""
    g = np.random.default_rng(4321)
    state = {}
    for n in names:
        t = (g.standard_normal(enc.expected_shape(desc, n), dtype=np.float32) * 0.02).astype(np.float32)
        state[prefix + n] = t + 1.0 if n.lower().endswith(("layernorm.weight", "norm.weight")) else t
    save_file(state, str(d / "model.safetensors"))
    (d / "config.json").write_text(json.dumps(cfg))
    (d / "modules.json").write_text(json.dumps([
        {"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
        {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
        {"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}]))
    (d / "1_Pooling" / "config.json").write_text(json.dumps({
        "word_embedding_dimension": H, "pooling_mode_cls_token": model == "bge", "pooling_mode_mean_tokens": model != "bge"}))
    (d / "sentence_bert_config.json").write_text(json.dumps({"max_seq_length": 8192 if model != "bge" else 512,
                                                              "do_lower_case": True}))
    (d / "vocab.txt").write_text("\n".join(vocab) + "\n", encoding="utf-8")


def child(model, run, path):
    os.environ.update(EMBEDDING_MODEL=path, EMBEDDING_DIMENSION=str(H), VOITTA_ENCODER_PRECISION="f16")
    if run != "off":
        os.environ.update(VOITTA_LATE_CHUNKING="1", VOITTA_MAX_SEQ_LENGTH=run.split("-")[1])
    from voitta_rag_amd import Engine, config, embedding, sparse_embedding, store_registry, vector_store
    from voitta_rag_amd.indexer import BulkIndexer, ParsedFile

    # about 0.9 tokens per word... measured below: the sizes are in words, the report is in tokens
    files = [ParsedFile(document((450, 1800, 7200)[i % 3]), f"dir{i % 7}/f{i}.md", f"dir{i % 7}", f"dir{i % 7}", f"f{i}.md",
                        source_modified_at=1_700_000_000 + i) for i in range(args.docs)]

    def fresh():
        config.get_settings.cache_clear()
        store_registry.reset()
        embedding._embedding_service = sparse_embedding._sparse_embedding_service = vector_store._vector_store = None
        return embedding.get_embedding_service(), vector_store.get_vector_store()

    class Counting(BulkIndexer):  # the sequences and tokens the encoder sees, batch by batch
        seqs = tokens = 0

        def _tokenise(self, *a, **kw):
            b = super()._tokenise(*a, **kw)
            if b.wp_off is not None:
                Counting.seqs += len(b.wp_off) - 1
                Counting.tokens += int(b.wp_off[-1])
            return b

    emb, vs = fresh()  # (one model load per process: the three passes append to one store)
    BulkIndexer().index_files(files[:6])  # warm-up: workspaces, table growth
    Counting.seqs = Counting.tokens = 0
    vs.client.sync()
    t0 = time.perf_counter()
    counts = Counting().index_files(files)
    vs.client.sync()
    dt = time.perf_counter() - t0
    n = sum(counts.values())
    seqs, tokens = Counting.seqs, Counting.tokens
    eng = vs.client
    eng.profile(True)
    g0, a0 = eng.profile_read(Engine.PROF_GEMM), eng.profile_read(Engine.PROF_ATTENTION)
    BulkIndexer().index_files(files)
    eng.sync()
    g1, a1 = eng.profile_read(Engine.PROF_GEMM), eng.profile_read(Engine.PROF_ATTENTION)
    eng.profile(False)
    line = json.dumps(dict(build=args.label, model=model, run=run, layers=args.layers, window=emb.model.max_seq_length, documents=len(files),
                           chunks=n, sequences=seqs, encoder_tokens=tokens, seconds=round(dt, 3),
                           chunks_per_s=round(n / dt, 1), tokens_per_s=round(tokens / dt, 1),
                           gemm_ms=round(g1[0] - g0[0], 2), attention_ms=round(a1[0] - a0[0], 2),
                           attention_launches=a1[1] - a0[1]))
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if args.child:
    child(*args.child.split(":", 2))
    sys.exit(0)

with tempfile.TemporaryDirectory() as tmp:
    for model in args.models.split(","):
        path = pathlib.Path(tmp) / f"{model}-shaped"
        checkpoint(model, path)
        for _ in range(2):
            for run in args.runs.split(","):
                cmd = [sys.executable, os.path.abspath(__file__), "--docs", str(args.docs), "--layers", str(args.layers),
                       "--out", args.out, "--label", args.label, "--child", f"{model}:{run}:{path}"]
                subprocess.run(cmd, check=True, timeout=900)
