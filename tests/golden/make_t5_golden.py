"""Generates tests/golden/t5_tiny_*.npz and tests/golden/t5_tokenizer.json.

t5_tiny_d64 / t5_tiny_d32: seeded T5 encoders (tests/t5_oracle.py's weights) run through transformers.T5EncoderModel in
f64, then pooled and normalised as sentence-transformers does. Each sequence runs alone (batch of one, no padding).
T5LayerNorm takes its variance through `.to(torch.float32)` whatever the model's dtype (an upcast meant for half
precision, a DOWNcast of an f64 model), so the library run as it is carries f32 rounding in every norm: that run is
stored as want_lib. `want` is the same model with that one cast following the input's dtype (f64_norms(), which
restates T5LayerNorm.forward's three lines with the cast removed) — f64 throughout, the reference that can be held to
1e-9. The model weights are NOT stored: t5_oracle.random_weights regenerates them from the seed. Stored: ids, offsets, the expected
embeddings, the shape, seed, pooling, the library versions, and offset_bias [heads, 1201]: what the library's
compute_bias gives for key - query = -600 .. 600 (f32: entries of the f32 weight table).
The lengths include 1, the bucket edges (8, 9, 16, 17) and lengths past 130, so that offsets pass the saturation point
(128) in both directions.

t5_tokenizer.json: {"tokenizer": a small T5-shaped Unigram tokenizer.json, "cases": [...]}. The tokenizer is built with
the `tokenizers` library from the pieces and the precompiled charsmap of tests/golden/xlmr_tokenizer.json, re-ordered as
T5 has them (<pad> 0, </s> 1, <unk> 2, ..., <extra_id_1>, <extra_id_0> last), Precompiled + Metaspace, the template
"$A </s>". The cases are the ids the library gives for the texts at max_len 512 and for the truncated ones at max_len 12.
Run in the build container:  python tests/golden/make_t5_golden.py"""
import json
import os
import sys

import numpy as np
import torch
import transformers

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import mpnet_oracle as mp  # noqa: E402
import t5_oracle as t5  # noqa: E402

LENS = [1, 2, 8, 9, 16, 17, 65, 131, 200, 300]
CASES = {
    # name: (shape, pooling, seed)
    "tiny_d64": (t5.T5Shape(2, 128, 2, 256), "mean", 7),
    "tiny_d32": (t5.T5Shape(2, 128, 4, 256), "cls", 7),
}
TEXTS = [
    "", " ", "vector database", "Hybrid FUSION ranking!", "the encoder's attention bias, by relative position.",
    "café naïve résumé über", "fill <extra_id_0> in <extra_id_1>.", "<extra_id_0>", "a<extra_id_0>b", "ﬁlter ① ㎏ Ⅷ",
    "ｆｕｌｌ ｗｉｄｔｈ", "tokens\twith\nwhite\r\nspace", "double  spaces   here", "中文 search 日本", "zzzqqq unknownword",
    "🙂 emoji", "</s> in text", "memory bandwidth " * 40, "chunk " * 600,
]
TRUNCATED_LEN = 12


def hf_model(shape: t5.T5Shape, w: dict):
    cfg = transformers.T5Config(vocab_size=shape.vocab, d_model=shape.hidden, d_kv=shape.d_kv, d_ff=shape.intermediate,
                                num_layers=shape.layers, num_heads=shape.heads,
                                relative_attention_num_buckets=shape.buckets,
                                relative_attention_max_distance=shape.max_distance, dropout_rate=0.0,
                                layer_norm_epsilon=shape.eps, feed_forward_proj="relu", is_encoder_decoder=False,
                                use_cache=False)
    cfg._attn_implementation = "eager"
    model = transformers.T5EncoderModel(cfg)
    state = {k: torch.from_numpy(v) for k, v in w.items()}
    state["encoder.embed_tokens.weight"] = state[t5.WORD_KEY]
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected and not missing, (missing, unexpected)  # every tensor came from the seeded weights
    return model.double().eval()


class f64_norms:
    """Within the block, T5LayerNorm.forward is its own three lines without the `.to(torch.float32)` on the variance."""

    def __enter__(self):
        cls = transformers.models.t5.modeling_t5.T5LayerNorm
        self.cls, self.saved = cls, cls.forward

        def forward(norm, hidden_states):
            variance = hidden_states.pow(2).mean(-1, keepdim=True)
            hidden_states = hidden_states * torch.rsqrt(variance + norm.variance_epsilon)
            return norm.weight * hidden_states

        cls.forward = forward

    def __exit__(self, *exc):
        self.cls.forward = self.saved


def make_models():
    for name, (shape, pooling, seed) in CASES.items():
        w = t5.random_weights(shape, seed)
        model = hf_model(shape, w)
        rng = np.random.default_rng(seed + 1000)
        seqs = [rng.integers(0, shape.vocab, size=n).astype(np.int32) for n in LENS]
        want = np.zeros((len(seqs), shape.hidden), np.float64)
        want_lib = np.zeros_like(want)
        with torch.no_grad():
            for i, ids in enumerate(seqs):
                tokens = torch.from_numpy(ids.astype(np.int64))[None]
                want_lib[i] = mp.pool(model(input_ids=tokens).last_hidden_state[0].numpy(), pooling)
                with f64_norms():
                    want[i] = mp.pool(model(input_ids=tokens).last_hidden_state[0].numpy(), pooling)
            # compute_bias(query_length, key_length) -> [1, heads, q, k]; row 600 of 1201 positions sees offsets -600..600
            attn = model.encoder.block[0].layer[0].SelfAttention
            bias = attn.compute_bias(1201, 1201)[0, :, 600, :].double().numpy()
        assert np.array_equal(bias, bias.astype(np.float32))
        off = np.zeros(len(seqs) + 1, np.int32)
        off[1:] = np.cumsum(LENS)
        path = os.path.join(HERE, f"t5_{name}.npz")
        np.savez_compressed(
            path, ids=np.concatenate(seqs), offsets=off, want=want, want_lib=want_lib, seed=seed, pooling=pooling,
            offset_bias=bias.astype(np.float32),
            shape=np.array([shape.layers, shape.hidden, shape.heads, shape.intermediate, shape.vocab, shape.buckets,
                            shape.max_distance]),
            eps=shape.eps,
            versions=f"transformers {transformers.__version__}, torch {torch.__version__}, numpy {np.__version__}")
        got = t5.sentence_embeddings(w, shape, seqs, pooling)
        print(f"{name}: oracle vs transformers max-abs {np.max(np.abs(got - want)):.3e} "
              f"(the library's f32 variances: {np.max(np.abs(got - want_lib)):.3e})")
        wrong = t5.sentence_embeddings(w, shape, seqs, pooling, table=None)
        print(f"{name}: no bias max-abs {np.max(np.abs(wrong - want)):.3e}")
        print("wrote", path, os.path.getsize(path), "bytes")


def make_tokenizer():
    import tokenizers
    from tokenizers import Tokenizer, models, normalizers, pre_tokenizers, processors

    src = json.load(open(os.path.join(HERE, "xlmr_tokenizer.json"), encoding="utf-8"))["tokenizer"]
    norm = src["normalizer"]
    steps = norm["normalizers"] if norm.get("type") == "Sequence" else [norm]
    charsmap = next(s["precompiled_charsmap"] for s in steps if s.get("type") == "Precompiled")
    body = [(p, s) for p, s in src["model"]["vocab"] if p not in ("<s>", "<pad>", "</s>", "<unk>", "<mask>")]
    vocab = [("<pad>", 0.0), ("</s>", 0.0), ("<unk>", 0.0)] + body + [("<extra_id_1>", 0.0), ("<extra_id_0>", 0.0)]
    tok = Tokenizer(models.Unigram(vocab, unk_id=2, byte_fallback=False))
    import base64

    tok.normalizer = normalizers.Precompiled(base64.b64decode(charsmap))
    tok.pre_tokenizer = pre_tokenizers.Metaspace(replacement="▁", prepend_scheme="always")
    tok.post_processor = processors.TemplateProcessing(single="$A </s>", pair="$A </s> $B </s>",
                                                       special_tokens=[("</s>", 1)])
    tok.add_special_tokens([tokenizers.AddedToken(t, special=True, normalized=False)
                            for t in ("<pad>", "</s>", "<unk>", "<extra_id_1>", "<extra_id_0>")])
    spec = json.loads(tok.to_str())
    cases = []
    for max_len in (512, TRUNCATED_LEN):
        tok.enable_truncation(max_length=max_len)
        for text, e in zip(TEXTS, tok.encode_batch(TEXTS)):
            if max_len == 512 or len(e.ids) == max_len:
                cases.append({"text": text, "max_len": max_len, "ids": e.ids})
    n = len(vocab)
    assert sum(c["max_len"] == TRUNCATED_LEN for c in cases) >= 3 and any(len(c["ids"]) == 512 for c in cases)
    assert all(c["ids"][-1] == 1 for c in cases) and any(c["ids"] == [1] for c in cases)
    assert any(n - 1 in c["ids"] for c in cases) and any(2 in c["ids"] for c in cases)
    out = {"versions": f"tokenizers {tokenizers.__version__}", "tokenizer": spec, "cases": cases}
    path = os.path.join(HERE, "t5_tokenizer.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=True, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes;", len(cases), "cases,", n, "pieces")


if __name__ == "__main__":
    make_models()
    make_tokenizer()
