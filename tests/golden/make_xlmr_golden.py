"""Generates the XLM-RoBERTa fixtures:
  tests/golden/xlmr_tokenizer.json  a seeded sentencepiece Unigram vocabulary (trained here on multilingual text) and a
                                    charsmap compiled from a small normalisation rule table, written as tokenizer.json
                                    file (the other pre-tokenizer shape, no charsmap and a hand-made vocabulary with
                                    equal-score ties are derived from it by xlmr_oracle.tokenizer_spec), with the ids HF
                                    tokenizers gives for adversarial texts and pairs in each case
  tests/golden/xlmr_*.npz           seeded encoders / a cross-encoder run through transformers.XLMRobertaModel
                                    (mean pooling, normalised) and XLMRobertaForSequenceClassification in f64 with eager
                                    attention, on ids from that tokenizer
Run in the build container:  python tests/golden/make_xlmr_golden.py
The model weights are NOT stored: tests/xlmr_oracle.py regenerates them from the seed (oracle.bert.random_weights with
514 positions and one token type). Records the library versions."""
import io
import json
import os
import sys
import tempfile

import numpy as np
import sentencepiece as spm
import tokenizers
import torch
import transformers
from sentencepiece import sentencepiece_model_pb2 as spm_pb
from tokenizers import Regex, Tokenizer, models, normalizers, pre_tokenizers, processors

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import xlmr_oracle as xo  # noqa: E402
from oracle import bert as obert  # noqa: E402

# normalisation rules (code points -> code points): fullwidth letters, ligatures, circled digits, e + U+0301,
# Hangul jamo -> syllable, NBSP / ideographic space -> space, ZWSP -> nothing
RULES = ([(f"{0xFF21 + i:X}", f"{0x41 + i:X}") for i in range(26)] + [(f"{0xFF41 + i:X}", f"{0x61 + i:X}") for i in range(26)]
         + [("FB01", "66 69"), ("FB02", "66 6C"), ("FB00", "66 66")]
         + [(f"{0x2460 + i:X}", f"{0x31 + i:X}") for i in range(9)]
         + [("65 301", "E9"), ("1100 1161", "AC00"), ("1102 1161", "B098"), ("A0", "20"), ("3000", "20"), ("200B", "")])

SENTENCES = [
    "The quick brown fox jumps over the lazy dog.", "Der schnelle braune Fuchs springt über den faulen Hund.",
    "Le renard brun rapide saute par-dessus le chien paresseux.", "El rápido zorro marrón salta sobre el perro perezoso.",
    "Быстрая коричневая лиса прыгает через ленивую собаку.", "Η γρήγορη καφέ αλεπού πηδάει πάνω από τον τεμπέλη σκύλο.",
    "敏捷的棕色狐狸跳过了懒狗。", "素早い茶色の狐がのろまな犬を飛び越える。", "빠른 갈색 여우가 게으른 개를 뛰어넘는다.",
    "तेज़ भूरी लोमड़ी आलसी कुत्ते के ऊपर कूदती है।", "الثعلب البني السريع يقفز فوق الكلب الكسول.",
    "Szybki brązowy lis przeskakuje nad leniwym psem.", "Hızlı kahverengi tilki tembel köpeğin üzerinden atlar.",
    "Con cáo nâu nhanh nhẹn nhảy qua con chó lười.", "Den snabba bruna räven hoppar över den lata hunden.",
]
SYLL = {"latin": ["ka", "lo", "mi", "tre", "zu", "ban", "cor", "del", "fin", "gra", "qui", "vos", "ing", "ed", "ar"],
        "cyr": ["ка", "ло", "ми", "тре", "зу", "бан", "кор"], "greek": ["κα", "λο", "μι", "τρε", "ζυ"],
        "han": list("的一是不了人我在有他这中大来上国个到说们为子和你地出道也时年"), "hangul": list("가나다라마바사아자차카타파하한국어"),
        "deva": ["क", "ख", "ग", "न", "म", "र", "स", "ति", "को", "में"]}


def corpus(rng, n=3000):
    out = list(SENTENCES) * 20
    for _ in range(n):
        script = str(rng.choice(list(SYLL)))
        words = []
        for _ in range(int(rng.integers(3, 12))):
            words.append("".join(str(rng.choice(SYLL[script])) for _ in range(int(rng.integers(1, 4)))))
        out.append(" ".join(words))
    return out


def train(rng):
    rules = "".join(f"{a}\t{b}\n" for a, b in RULES)
    with tempfile.TemporaryDirectory() as d:
        tsv = os.path.join(d, "rules.tsv")
        open(tsv, "w").write(rules)
        buf = io.BytesIO()
        spm.SentencePieceTrainer.train(sentence_iterator=iter(corpus(rng)), model_writer=buf, model_type="unigram",
                                       vocab_size=700, character_coverage=0.995, normalization_rule_tsv=tsv,
                                       byte_fallback=False, minloglevel=2, num_threads=1)
    proto = spm_pb.ModelProto()
    proto.ParseFromString(buf.getvalue())
    return proto


def xlmr_vocab(proto):  # transformers' XLMRobertaConverter.vocab
    return ([("<s>", 0.0), ("<pad>", 0.0), ("</s>", 0.0), ("<unk>", 0.0)]
            + [(p.piece, p.score) for p in proto.pieces[3:]] + [("<mask>", 0.0)])


def hf_tokenizer(vocab, charsmap, shape):
    tok = Tokenizer(models.Unigram(vocab, unk_id=3, byte_fallback=False))
    if shape == "metaspace":  # the hub files' shape: Precompiled + Replace, Metaspace
        steps = ([normalizers.Precompiled(charsmap)] if charsmap else []) + [normalizers.Replace(Regex(" {2,}"), " ")]
        tok.normalizer = normalizers.Sequence(steps)
        tok.pre_tokenizer = pre_tokenizers.Metaspace(replacement="▁", prepend_scheme="always")
    else:  # transformers 5's XLMRobertaTokenizer: Precompiled, Sequence[WhitespaceSplit, Metaspace]
        if charsmap:
            tok.normalizer = normalizers.Precompiled(charsmap)
        tok.pre_tokenizer = pre_tokenizers.Sequence([pre_tokenizers.WhitespaceSplit(),
                                                     pre_tokenizers.Metaspace(replacement="▁", prepend_scheme="always")])
    tok.post_processor = processors.TemplateProcessing(single="<s> $A </s>", pair="<s> $A </s> </s> $B </s>",
                                                       special_tokens=[("<s>", 0), ("</s>", 2)])
    tok.add_special_tokens([tokenizers.AddedToken(t, special=True, normalized=False) for t in ("<s>", "<pad>", "</s>", "<unk>")])
    tok.add_special_tokens([tokenizers.AddedToken("<mask>", special=True, normalized=False, lstrip=True)])
    return tok


ADVERSARIAL = [
    "", " ", "   ", "hello", " leading", "trailing  ", "many     spaces   inside", "tab\tand\nnewline\r\nend",
    "quick <s>brown", "a</s>b", "x <mask> y", "  <mask>", "<mask>", "<s><s></s>", "<pad> and <unk> literal",
    "<s", "mask>", "ｆｕｌｌｗｉｄｔｈ ＴＥＸＴ", "ﬁne ﬂow ﬀ", "①②③ circled", "café é", "가 나",
    "non breaking　space", "zero​width", "​first", "emoji 👩‍💻 family 👨‍👩‍👧 flag 🇫🇷🇩🇪",
    "🇫🇷🇫", "é́ ｅ́", "Ｅ́x", "中文 汉字 測試", "한국어 텍스트 각", "ⓐⓑ ㊀ ½ ™",
    "العربية نص", "हिन्दी पाठ", "ąęłńóśźż", "ÅÄÖ åäö", "x̀́̂̃y", "́start", "ab cd  ef",
    "😀😃😄 emoji only", "\U0001F469\U0001F3FD‍\U0001F52C", "mixed中文and한국어words", "123 4567 89.0",
    "Ω≈ç√∫˜µ≤≥÷", "▁literal meta▁space", "∆∆∆ ‰‰ ‱", "𝔘𝔫𝔦𝔠𝔬𝔡𝔢", "힣", "กิน",
]


def tokenizer_fixture(rng):
    proto = train(rng)
    charsmap = proto.normalizer_spec.precompiled_charsmap
    assert 200 < len(charsmap) < 4096, len(charsmap)
    vocab = xlmr_vocab(proto)
    texts = list(ADVERSARIAL) + [str(s) for s in rng.choice(SENTENCES, 10)] + corpus(rng, 30)[-30:]
    pairs = [(texts[int(i)], texts[int(j)]) for i, j in rng.integers(0, len(texts), (40, 2))]
    # one tokenizer.json is stored; xlmr_oracle.tokenizer_spec derives the other cases from it
    out = {"versions": f"tokenizers {tokenizers.__version__}; sentencepiece {spm.__version__}",
           "rules": RULES, "texts": texts, "pairs": pairs,
           "tie_texts": ["ab", "abab", " ab ba", "c", "cc ab", "abc cab", "bab ab", "ccc"],
           "tokenizer": json.loads(hf_tokenizer(vocab, charsmap, "metaspace").to_str()), "cases": {}}
    for name in xo.TOKENIZER_CASES:
        tok = Tokenizer.from_str(json.dumps(xo.tokenizer_spec(out, name)))
        case_texts = out["tie_texts"] if name == "ties" else texts
        case = {"single": {}, "pair": {}}
        for max_len in (512, 16, 6):
            tok.enable_truncation(max_length=max_len, strategy="longest_first")
            if max_len != 16:
                case["single"][str(max_len)] = [e.ids for e in tok.encode_batch(case_texts)]
            if max_len != 6:
                case["pair"][str(max_len)] = [e.ids for e in tok.encode_batch(pairs)]
        out["cases"][name] = case
    with open(os.path.join(HERE, "xlmr_tokenizer.json"), "w", encoding="utf-8") as f:
        json.dump(out, f, ensure_ascii=False, separators=(",", ":"))
    print("tokenizer: charsmap", len(charsmap), "bytes,", len(vocab), "pieces")
    return hf_tokenizer(vocab, charsmap, "metaspace"), len(vocab)


MODELS = {
    # name: (shape, seed, kind)
    "xlmr_tiny": (obert.BertShape(2, 128, 2, 512, max_pos=514, type_vocab=1, eps=1e-5), 41, "embed"),
    "xlmr_e5small": (obert.BertShape(12, 384, 12, 1536, max_pos=514, type_vocab=1, eps=1e-5), 42, "embed"),
    "xlmr_rerank_tiny": (obert.BertShape(2, 128, 2, 512, max_pos=514, type_vocab=1, eps=1e-5), 43, "rerank"),
}


def hf_config(shape, labels=None):
    cfg = transformers.XLMRobertaConfig(
        vocab_size=shape.vocab, hidden_size=shape.hidden, num_hidden_layers=shape.layers,
        num_attention_heads=shape.heads, intermediate_size=shape.intermediate, max_position_embeddings=shape.max_pos,
        type_vocab_size=shape.type_vocab, layer_norm_eps=shape.eps, hidden_act="gelu", hidden_dropout_prob=0.0,
        attention_probs_dropout_prob=0.0, pad_token_id=1, bos_token_id=0, eos_token_id=2,
        **({"num_labels": labels} if labels else {}))
    cfg._attn_implementation = "eager"
    return cfg


def load(m, w, prefix):
    sd = m.state_dict()
    state = {}
    for k, v in w.items():
        key = k if k.startswith("classifier.") else prefix + k
        assert key in sd and tuple(sd[key].shape) == v.shape, (key, v.shape)
        state[key] = torch.from_numpy(v)
    missing = [k for k in sd if k not in state and "position_ids" not in k and "token_type_ids" not in k
               and "pooler" not in k]
    assert not missing, missing
    m.load_state_dict(state, strict=False)
    return m.double()


def padded(seqs):
    B, S = len(seqs), max(len(s) for s in seqs)
    ids = torch.ones((B, S), dtype=torch.long)  # <pad> = 1
    mask = torch.zeros((B, S), dtype=torch.long)
    for i, s in enumerate(seqs):
        ids[i, :len(s)] = torch.tensor(s)
        mask[i, :len(s)] = 1
    return ids, mask


def model_fixtures(tok, n_vocab, rng):
    texts = [SENTENCES[0], SENTENCES[6], SENTENCES[8], "x <mask> y", "", " ".join(SENTENCES * 6)]
    for name, (shape, seed, kind) in MODELS.items():
        shape.vocab = n_vocab
        w = xo.random_weights(shape, seed, kind == "rerank")
        if kind == "embed":
            tok.enable_truncation(max_length=512, strategy="longest_first")
            seqs = [e.ids for e in tok.encode_batch(texts)]
            assert len(seqs[-1]) == 512 and all(1 not in s for s in seqs)
            m = load(transformers.XLMRobertaModel(hf_config(shape), add_pooling_layer=False).eval(), w, "")
            ids, mask = padded(seqs)
            with torch.no_grad():
                h = m(input_ids=ids, attention_mask=mask).last_hidden_state.double()
            mf = mask.unsqueeze(-1).double()
            emb = (h * mf).sum(1) / mf.sum(1).clamp(min=1e-9)
            want = torch.nn.functional.normalize(emb, p=2, dim=1).numpy()
            extra = dict(texts=np.array(texts))
        else:
            tok.enable_truncation(max_length=128, strategy="longest_first")
            queries = [SENTENCES[1], SENTENCES[7], " ".join(SENTENCES[:8])]
            counts = [5, 3, 4]
            passages = [str(s) for s in rng.choice(SENTENCES + ["", "<mask> tail"], sum(counts))]
            a = [q for q, c in zip(queries, counts) for _ in range(c)]
            seqs = [e.ids for e in tok.encode_batch(list(zip(a, passages)))]
            assert all(1 not in s for s in seqs)
            m = load(transformers.XLMRobertaForSequenceClassification(hf_config(shape, 1)).eval(), w, "roberta.")
            ids, mask = padded(seqs)
            with torch.no_grad():
                want = m(input_ids=ids, attention_mask=mask).logits[:, 0].double().numpy()
            cand_off = np.zeros(len(counts) + 1, np.int64)
            cand_off[1:] = np.cumsum(counts)
            extra = dict(queries=np.array(queries), passages=np.array(passages), cand_off=cand_off, max_len=np.array(128))
        off = np.zeros(len(seqs) + 1, np.int32)
        off[1:] = np.cumsum([len(s) for s in seqs])
        np.savez_compressed(
            os.path.join(HERE, f"{name}.npz"),
            shape=np.array([shape.layers, shape.hidden, shape.heads, shape.intermediate, shape.vocab, shape.max_pos,
                            shape.type_vocab]),
            eps=np.array(shape.eps), seed=np.array(seed), ids=np.concatenate([np.asarray(s, np.int32) for s in seqs]),
            offsets=off, want=want, **extra,
            versions=np.array(f"transformers {transformers.__version__}; tokenizers {tokenizers.__version__}; "
                              f"torch {torch.__version__}; numpy {np.__version__}"))
        print(name, len(seqs), "sequences, longest", max(len(s) for s in seqs))


def main():
    rng = np.random.default_rng(2026)
    tok, n_vocab = tokenizer_fixture(rng)
    model_fixtures(tok, n_vocab, rng)


if __name__ == "__main__":
    main()
