"""Generates tests/golden/bpe_tokenizer.json: a seeded byte-level BPE of about 600 pieces (tokenizers' BpeTrainer over
ByteLevel.alphabet(), trained on make_xlmr_golden.py's multilingual sentences and syllable corpus) with the ModernBERT
pipeline — NFC, ByteLevel(add_prefix_space=false, use_regex=true), TemplateProcessing [CLS] $A [SEP] / [CLS] $A [SEP] $B
[SEP] — five special tokens ([MASK] with lstrip) and three runs of spaces as normalized, non-special added tokens; and
the ids the HF `tokenizers` library gives for an adversarial list of texts and for pairs at several max_len.
Run in the build container:  python tests/golden/make_bpe_golden.py
Texts are stored as hex of their UTF-8 bytes (some are not valid UTF-8: the library saw them decoded with U+FFFD for
every malformed byte, which is what the engine's decoder does). Records the library versions."""
import json
import os
import sys

import numpy as np
import tokenizers
from tokenizers import AddedToken, Tokenizer, decoders, models, normalizers, pre_tokenizers, processors, trainers

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_xlmr_golden import corpus  # noqa: E402

SPECIALS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
MAX_LENS = [512, 16, 6, 3]


def train():
    tok = Tokenizer(models.BPE(unk_token=None))
    tok.normalizer = normalizers.NFC()
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
    tok.decoder = decoders.ByteLevel()
    specials = [AddedToken(s, special=True, normalized=False, lstrip=s == "[MASK]") for s in SPECIALS]
    trainer = trainers.BpeTrainer(vocab_size=600, special_tokens=specials, show_progress=False,
                                  initial_alphabet=sorted(pre_tokenizers.ByteLevel.alphabet()))
    tok.train_from_iterator(corpus(np.random.default_rng(17), 1500), trainer)
    tok.add_tokens([AddedToken(" " * n, normalized=True, special=False) for n in (2, 4, 8)])
    v = tok.get_vocab()
    tok.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B [SEP]",
                                                       special_tokens=[("[CLS]", v["[CLS]"]), ("[SEP]", v["[SEP]"])])
    return tok


def texts():
    t = ["I'll we've 'S it's they'Re don't 'd 'm x'll'", "The quick brown fox.", "a1b22 3.14 ①② ½x", "!!! ... ?! wow!!! (a) [b]",
         " !!!", "a !?", "é", "ạ̇ ḅ̇", "각 한글", "क़ क़",
         "敏捷的棕色狐狸 跳过了", "👩‍💻 ok 👍🏽", "x [SEP] y", "x[SEP]y", "a [MASK] b", "a   [MASK]b", "[CLS][MASK]",
         "", " ", "a b  c", "a\u0085b", "a　　b", "tab\tnew\nline\r\n end", "\t\t\ta", "a \n b",
         "Ünï cödé Ångström ǆ ﬁ", "Быстрая лиса", "게으른 개를", "w" * 5000, "ab" * 1200 + " end"]
    for n in range(1, 10):
        t += [" " * n + "lead", "trail" + " " * n, "in" + " " * n + "ner", "\n" * n + "x", "t" + "\t" * n]
    out = [s.encode("utf-8") for s in t]
    out += [b"bad \xff byte", b"\x80 start", b"cut \xc3", b"\xe2\x82 x", b"ok \xf0\x9f\x91 z"]
    return out


def main():
    tok = train()
    raw = texts()
    seen = [b.decode("utf-8", "replace") for b in raw]
    # one U+FFFD per malformed byte is the engine's rule; Python's decoder replaces a truncated sequence by one
    seen[-2], seen[-1] = "�� x", "ok ��� z"
    rng = np.random.default_rng(5)
    pa = [seen[int(i)] for i in rng.integers(0, len(seen) - 7, size=40)]
    pb = [seen[int(i)] for i in rng.integers(0, len(seen) - 7, size=40)]
    pa[0], pb[0], pa[1], pb[2] = "", "", "", ""
    rec = {"single": {}, "pairs": {}}
    for ml in MAX_LENS:
        tok.enable_truncation(max_length=ml, strategy="longest_first")
        rec["single"][str(ml)] = [e.ids for e in tok.encode_batch(seen)]
        encs = tok.encode_batch(list(zip(pa, pb)))
        rec["pairs"][str(ml)] = {"ids": [e.ids for e in encs],
                                 "seg_b": [next((i for i, s in enumerate(e.sequence_ids) if s == 1), len(e.ids) - 1) for e in encs]}
    tok.no_truncation()
    out = {"tokenizer": json.loads(tok.to_str()), "texts_hex": [b.hex() for b in raw],
           "pair_a_hex": [s.encode("utf-8").hex() for s in pa], "pair_b_hex": [s.encode("utf-8").hex() for s in pb],
           "expected": rec, "versions": f"tokenizers {tokenizers.__version__}, numpy {np.__version__}"}
    path = os.path.join(HERE, "bpe_tokenizer.json")
    json.dump(out, open(path, "w"), ensure_ascii=True, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes;", tok.get_vocab_size(), "tokens,", len(raw), "texts")


if __name__ == "__main__":
    main()
