"""Generates tests/golden/mpnet_tiny_*.npz and tests/golden/mpnet_tokenizer.json.

mpnet_tiny_d64 / mpnet_tiny_d32: seeded MPNet encoders (tests/mpnet_oracle.py's weights) run through
transformers.MPNetModel in f64, then pooled and normalised as sentence-transformers does. Each sequence runs alone (batch
of one, no padding); no id is the padding id 1. The model weights are NOT stored: mpnet_oracle.random_weights regenerates
them from the seed. Stored: ids, offsets, the expected embeddings, the shape, seed, pooling, the library versions, and
position_bias [heads, 512, 512]: what the library's compute_position_bias gives for 512 positions (f32: the values are
entries of the f32 weight table).
The lengths are the ones at which a relative-offset bias can go wrong: the exact/logarithmic bucket edge (8, 9), tile
edges (16, 17, 64, 65), and the first offsets at and past +-128 (128, 129, 130), then 193, 257 and 512.

mpnet_tokenizer.json: a small WordPiece tokenizer.json in MPNet's layout, built with the `tokenizers` library: <s>,
<pad>, </s>, <unk> first, [UNK] as the model's unknown token, <mask> last, BertNormalizer, BertPreTokenizer and
RobertaProcessing. mpnet_tokenizer_cases.json beside it (the library refuses a tokenizer.json with a key it does not know)
holds the ids the library gives for a few dozen texts at max_len 512 and for the truncated ones at max_len 16.
Run in the build container:  python tests/golden/make_mpnet_golden.py"""
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

LENS = [1, 2, 8, 9, 16, 17, 64, 65, 128, 129, 130, 193, 257, 512]
CASES = {
    # name: (shape, pooling, seed)
    # (seeds at which each planted mistake of tests/test_mpnet_cpu.py moves a row by more than 100 x the f16 bar)
    "tiny_d64": (mp.MpnetShape(2, 128, 2, 256), "mean", 94),
    "tiny_d32": (mp.MpnetShape(2, 128, 4, 256), "cls", 94),
}

WORDS = ("vector database index hybrid fusion ranking sparse dense retrieval kernel memory bandwidth wavefront encoder "
         "attention relative position bucket bias layer norm residual token chunk document search query score filter "
         "the a of and to in is for on with cafe naive resume uber").split()
PIECES = ["##s", "##ing", "##ed", "##er", "##ly", "##a", "##b", "##c", "##e", "##n", "##t", "##x", "##1", "##2"]
CHARS = list("abcdefghijklmnopqrstuvwxyz0123456789") + list(".,!?-'\"()") + ["中", "文", "日", "本"]
TEXTS = [
    "", " ", "vector database", "Hybrid FUSION ranking!", "the encoder's attention bias, by relative position.",
    "café naïve résumé über", "CAFÉ Über", "中文 search 日本", "中中文文", "zzzqqq unknownword", "xylophone 12 21 3",
    "indexing chunked documents", "a-b (c) 'd' \"e\"", "tokens\twith\nwhite\r\nspace", "ﬁlter", "№ 5 ±", "🙂 emoji",
    "searches queries scores filters", "the the the", "dense. sparse? hybrid!", "layer norm residual",
    "a" * 101, "kernel" * 30, "scoréd", "İstanbul", "ǅ", "retrieval​bandwidth", "Ω mega", "é̀",
    "memory bandwidth " * 40, " ".join(WORDS), "chunk " * 600,
]
TRUNCATED_LEN = 16


def hf_model(shape: mp.MpnetShape, w: dict):
    cfg = transformers.MPNetConfig(vocab_size=shape.vocab, hidden_size=shape.hidden, num_hidden_layers=shape.layers,
                                   num_attention_heads=shape.heads, intermediate_size=shape.intermediate, hidden_act="gelu",
                                   max_position_embeddings=shape.positions, layer_norm_eps=shape.eps,
                                   relative_attention_num_buckets=mp.BUCKETS, hidden_dropout_prob=0.0,
                                   attention_probs_dropout_prob=0.0)
    cfg._attn_implementation = "eager"
    model = transformers.MPNetModel(cfg, add_pooling_layer=False)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    assert not unexpected and not missing, (missing, unexpected)  # every tensor came from the seeded weights
    return model.double().eval()


def make_models():
    for name, (shape, pooling, seed) in CASES.items():
        w = mp.random_weights(shape, seed)
        model = hf_model(shape, w)
        rng = np.random.default_rng(seed + 1000)
        seqs = [rng.integers(4, shape.vocab, size=n).astype(np.int32) for n in LENS]  # (never the padding id 1)
        want = np.zeros((len(seqs), shape.hidden), np.float64)
        with torch.no_grad():
            for i, ids in enumerate(seqs):
                h = model(input_ids=torch.from_numpy(ids.astype(np.int64))[None]).last_hidden_state[0].numpy()
                want[i] = mp.pool(h, pooling)
            bias = model.encoder.compute_position_bias(torch.zeros(1, 512, shape.hidden, dtype=torch.float64))[0].numpy()
        assert np.array_equal(bias, bias.astype(np.float32))
        off = np.zeros(len(seqs) + 1, np.int32)
        off[1:] = np.cumsum(LENS)
        path = os.path.join(HERE, f"mpnet_{name}.npz")
        np.savez_compressed(
            path, ids=np.concatenate(seqs), offsets=off, want=want, seed=seed, pooling=pooling,
            position_bias=bias.astype(np.float32),
            shape=np.array([shape.layers, shape.hidden, shape.heads, shape.intermediate, shape.vocab, shape.positions]),
            eps=shape.eps,
            versions=f"transformers {transformers.__version__}, torch {torch.__version__}, numpy {np.__version__}")
        got = mp.sentence_embeddings(w, shape, seqs, pooling)
        print(f"{name}: oracle vs transformers max-abs {np.max(np.abs(got - want)):.3e}")
        for what, kw in (("no bias", dict(table=None)), ("mirrored", dict(mirrored=True)), ("clamp 90", dict(clamp=90))):
            wrong = mp.sentence_embeddings(w, shape, seqs, pooling, **kw)
            print(f"{name}: {what} max-abs {np.max(np.abs(wrong - want)):.3e}")
        print("wrote", path, os.path.getsize(path), "bytes")


def make_tokenizer():
    from tokenizers import Tokenizer, models, normalizers, pre_tokenizers, processors

    vocab = list(dict.fromkeys(["<s>", "<pad>", "</s>", "<unk>", "[UNK]"] + CHARS + WORDS + PIECES + ["<mask>"]))
    assert len(set(vocab)) == len(vocab)
    v = {t: i for i, t in enumerate(vocab)}
    tok = Tokenizer(models.WordPiece(v, unk_token="[UNK]", max_input_chars_per_word=100))
    tok.normalizer = normalizers.BertNormalizer(clean_text=True, handle_chinese_chars=True, strip_accents=None, lowercase=True)
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    tok.post_processor = processors.RobertaProcessing(sep=("</s>", v["</s>"]), cls=("<s>", v["<s>"]))
    tok.add_special_tokens(["<s>", "<pad>", "</s>", "<unk>", "[UNK]", "<mask>"])
    spec = json.loads(tok.to_str())
    cases = []
    for max_len in (512, TRUNCATED_LEN):
        tok.enable_truncation(max_length=max_len)
        for text, e in zip(TEXTS, tok.encode_batch(TEXTS)):
            if max_len == 512 or len(e.ids) == max_len:
                cases.append({"text": text, "max_len": max_len, "ids": e.ids})
    assert sum(c["max_len"] == TRUNCATED_LEN for c in cases) >= 3 and any(len(c["ids"]) == 512 for c in cases)
    assert any(v["[UNK]"] in c["ids"] for c in cases)
    for name, what in (("mpnet_tokenizer.json", spec), ("mpnet_tokenizer_cases.json", cases)):
        path = os.path.join(HERE, name)
        with open(path, "w", encoding="utf-8") as f:
            json.dump(what, f, ensure_ascii=True, indent=None)
        print("wrote", path, os.path.getsize(path), "bytes")
    Tokenizer.from_file(os.path.join(HERE, "mpnet_tokenizer.json"))
    print(len(cases), "cases")


if __name__ == "__main__":
    make_models()
    make_tokenizer()
