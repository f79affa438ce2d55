"""Generates tests/golden/rerank_*.npz: seeded one-label cross-encoders run through
transformers.BertForSequenceClassification (torch CPU, f64 from the f32 weights, eager attention) on question / passage pairs tokenised by
the HF `tokenizers` library (BERT pair template, LongestFirst truncation), as a padded batch with the encoding's
attention_mask and token_type_ids. Run in the build container:
    python tests/golden/make_rerank_golden.py
The encoder weights are NOT stored: tests/rerank_oracle.random_weights regenerates them from the seed. The classifier
scale and bias are chosen here so that the logits span at least [-3, 3], and stored. Records the library versions."""
import os
import sys

import numpy as np
import tokenizers
import torch
import transformers

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import bert as obert  # noqa: E402
import rerank_oracle as ro  # noqa: E402

SYLLABLES = ["ka", "lo", "mi", "tre", "zu", "ban", "cor", "del", "fin", "gra", "hu", "jer", "qui", "vos", "ell", "ing",
             "ed", "on", "ar", "is", "um", "ex", "pre", "sta"]
CASES = {
    # name: (shape, seed, max_len, candidates per question, precision notes live in the GPU test)
    "tiny": (obert.BertShape(2, 128, 2, 512, max_pos=128), 21, 64, [7, 0, 3, 12]),
    "minilm": (obert.BertShape(6, 384, 12, 1536, max_pos=512), 22, 256, [10, 6, 16]),
}


def make_vocab():
    words = sorted({a + b for a in SYLLABLES for b in SYLLABLES})
    pieces = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [chr(c) for c in range(ord("a"), ord("z") + 1)]
    pieces += ["##" + chr(c) for c in range(ord("a"), ord("z") + 1)] + list(".,?!'-") + SYLLABLES
    pieces += ["##" + s for s in SYLLABLES] + words + ["é", "ü", "中", "文", "한"]
    return list(dict.fromkeys(pieces))


def text(rng, n_words):
    out = []
    for _ in range(n_words):
        r = rng.random()
        if r < 0.08:
            out.append(str(rng.choice(list(".,?!"))))
        elif r < 0.12:
            out.append(str(rng.choice(["Über", "café", "中文", "한국", "naïve"])))
        else:
            w = "".join(str(rng.choice(SYLLABLES)) for _ in range(int(rng.integers(1, 4))))
            out.append(w.capitalize() if rng.random() < 0.2 else w)
    return " ".join(out)


def hf_tokenizer(vocab, max_len):
    from tokenizers import Tokenizer, models, normalizers, pre_tokenizers, processors

    v = {t: i for i, t in enumerate(vocab)}
    tok = Tokenizer(models.WordPiece(v, unk_token="[UNK]", max_input_chars_per_word=100))
    tok.normalizer = normalizers.BertNormalizer(clean_text=True, handle_chinese_chars=True, strip_accents=None,
                                                lowercase=True)
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    tok.post_processor = processors.TemplateProcessing(
        single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1",
        special_tokens=[("[CLS]", v["[CLS]"]), ("[SEP]", v["[SEP]"])])
    tok.enable_truncation(max_length=max_len, strategy="longest_first")
    return tok


def hf_model(shape, w):
    cfg = transformers.BertConfig(
        vocab_size=shape.vocab, hidden_size=shape.hidden, num_hidden_layers=shape.layers,
        num_attention_heads=shape.heads, intermediate_size=shape.intermediate,
        max_position_embeddings=shape.max_pos, type_vocab_size=shape.type_vocab,
        layer_norm_eps=shape.eps, hidden_act="gelu", hidden_dropout_prob=0.0,
        attention_probs_dropout_prob=0.0, num_labels=1)
    cfg._attn_implementation = "eager"
    m = transformers.BertForSequenceClassification(cfg).eval()
    sd = m.state_dict()
    state = {}
    for k, v in w.items():
        key = k if k.startswith("classifier.") else "bert." + k
        assert key in sd and tuple(sd[key].shape) == v.shape, key
        state[key] = torch.from_numpy(v)
    missing = [k for k in sd if k not in state and "position_ids" not in k and "token_type_ids" not in k]
    assert not missing, missing
    m.load_state_dict(state, strict=False)
    return m.double()  # f64: the fixture is a reference for f32 and f16 engines alike


def run(m, encs):
    B, S = len(encs), max(len(e.ids) for e in encs)
    ids = torch.zeros((B, S), dtype=torch.long)
    mask = torch.zeros((B, S), dtype=torch.long)
    types = torch.zeros((B, S), dtype=torch.long)
    for i, e in enumerate(encs):
        n = len(e.ids)
        ids[i, :n] = torch.tensor(e.ids)
        mask[i, :n] = torch.tensor(e.attention_mask)
        types[i, :n] = torch.tensor(e.type_ids)
    with torch.no_grad():
        return m(input_ids=ids, attention_mask=mask, token_type_ids=types).logits[:, 0].double().numpy()


def main():
    vocab = make_vocab()
    for name, (shape, seed, max_len, counts) in CASES.items():
        shape.vocab = len(vocab)
        rng = np.random.default_rng(seed)
        queries = [text(rng, int(rng.integers(2, 12))) for _ in counts]
        queries[-1] = text(rng, max_len)  # one question alone longer than max_len
        passages = [text(rng, int(rng.integers(0, max_len))) for _ in range(sum(counts))]
        passages[0] = ""  # an empty passage
        a = [q for q, c in zip(queries, counts) for _ in range(c)]
        tok = hf_tokenizer(vocab, max_len)
        encs = tok.encode_batch(list(zip(a, passages)))
        base = run(hf_model(shape, ro.random_weights(shape, seed)), encs)
        spread = base.max() - base.min()
        cls_scale = float(np.float32(8.0 / spread))
        cls_bias = float(np.float32(-cls_scale * (base.max() + base.min()) / 2))
        w = ro.random_weights(shape, seed, cls_scale, cls_bias)
        logits = run(hf_model(shape, w), encs)
        assert logits.min() <= -3 and logits.max() >= 3, (logits.min(), logits.max())
        ids = np.concatenate([np.asarray(e.ids, np.int32) for e in encs])
        off = np.zeros(len(encs) + 1, np.int32)
        off[1:] = np.cumsum([len(e.ids) for e in encs])
        seg_b = np.array([e.type_ids.index(1) for e in encs], np.int32)
        cand_off = np.zeros(len(counts) + 1, np.int64)
        cand_off[1:] = np.cumsum(counts)
        np.savez_compressed(
            os.path.join(HERE, f"rerank_{name}.npz"),
            shape=np.array([shape.layers, shape.hidden, shape.heads, shape.intermediate, shape.vocab, shape.max_pos,
                            shape.type_vocab]),
            eps=np.array(shape.eps), seed=np.array(seed), cls_scale=np.array(cls_scale), cls_bias=np.array(cls_bias),
            max_len=np.array(max_len), vocab=np.array(vocab), queries=np.array(queries), passages=np.array(passages),
            cand_off=cand_off, ids=ids, offsets=off, seg_b=seg_b, logits=logits,
            versions=np.array(f"transformers {transformers.__version__}; tokenizers {tokenizers.__version__}; "
                              f"torch {torch.__version__}; numpy {np.__version__}"))
        print(name, len(encs), "pairs, logits", logits.min(), logits.max(), "scale", cls_scale)


if __name__ == "__main__":
    main()
