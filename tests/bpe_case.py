"""TEST INFRASTRUCTURE — what the byte-level BPE tests share: the fixture, and seeded random strings that mix scripts,
separators, apostrophes, combining marks, added tokens and white space, restricted to code points assigned in the
Unicode version the engine's tables were generated from (this interpreter's unicodedata)."""
import json
import os
import unicodedata as ud

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def fixture():
    return json.load(open(os.path.join(HERE, "golden", "bpe_tokenizer.json"), encoding="utf-8"))


def hf_tokenizer(g):
    from tokenizers import Tokenizer

    return Tokenizer.from_str(json.dumps(g["tokenizer"]))


POOLS = [
    list("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"), list("0123456789"), list(".,;:!?-_()[]{}\"'`~@#$%^&*+=/\\|<>"),
    [" ", " ", " ", " ", "\t", "\n", "\r", " ", "\u0085", "　", " ", " "],
    ["'s", "'t", "'re", "'ve", "'m", "'ll", "'d", "'S", "'T", "'x", "''"],
    list("äöüßéèêñçåøæœÄÖÜÉ"), list("абвгдежзиклмнопрстуфхцчшщъыьэюя"), list("αβγδεζηθικλμνξοπρστυφχψω"),
    list("的一是不了人我在有他这中大来上国个到说们为子和你地出道也时年"), list("가나다라마바사아자차카타파하한국어"),
    ["ᄀ", "ᅡ", "ᆨ", "ᄂ", "ᅵ", "ᆫ"], list("कखगनमरसतिकोमें") + ["क़", "क़"],
    ["́", "̀", "̣", "̇", "̈", "̧", "̨", "̛", "̈́", "ͅ", "ཱི", "ཱ"],
    ["[SEP]", "[MASK]", "[CLS]", "[PAD]", "[UNK]", "  ", "    ", "        ", "[", "]"],
    ["👍", "👩‍💻", "🏽", "‍", "​", "①", "½", "Ⅷ", "٣", "๓", "ǆ", "ﬁ", "Å", "Ω", "µ", "̈́"],
    ["ا", "ل", "ع", "ر", "ب", "َ", "ّ", "א", "ָ", "ּ"],
]


def random_text(rng) -> str:
    n = int(rng.integers(0, 40))
    weights = np.array([8, 3, 3, 6, 1, 2, 2, 1, 2, 2, 1, 1, 2, 1, 1, 1], np.float64)
    parts = []
    for _ in range(n):
        pool = POOLS[int(rng.choice(len(POOLS), p=weights / weights.sum()))]
        parts.append(str(pool[int(rng.integers(0, len(pool)))]) * (1 if rng.random() < 0.85 else int(rng.integers(2, 6))))
    s = "".join(parts)
    assert all(ud.category(c) != "Cn" for c in s)
    return s


def random_texts(seed: int, n: int) -> list[str]:
    rng = np.random.default_rng(seed)
    return [random_text(rng) for _ in range(n)]


def embedder_checkpoint(d, g=None, layers=3, seed=63):
    """A ModernBERT-shaped sentence-transformers directory (mean pooling, Normalize, seeded weights, H = 128) whose
    tokenizer.json is the fixture's byte-level BPE -> (shape, weights, the tokenizers-library tokenizer)."""
    from safetensors.numpy import save_file

    import modernbert_oracle as mo

    g = g or fixture()
    os.makedirs(os.path.join(d, "1_Pooling"), exist_ok=True)
    json.dump(g["tokenizer"], open(os.path.join(d, "tokenizer.json"), "w"))
    hf = hf_tokenizer(g)
    vocab = -(-hf.get_vocab_size() // 8) * 8
    shape = mo.ModernShape(layers, 128, 2, 256, vocab=vocab, max_pos=8192, window=8)
    json.dump({"architectures": ["ModernBertModel"], "model_type": "modernbert", "hidden_size": 128,
               "num_hidden_layers": layers, "num_attention_heads": 2, "intermediate_size": 256, "vocab_size": vocab,
               "max_position_embeddings": 8192, "norm_eps": shape.eps, "hidden_activation": "gelu", "local_attention": 16,
               "global_attn_every_n_layers": 3,
               "layer_types": ["full_attention" if i % 3 == 0 else "sliding_attention" for i in range(layers)],
               "rope_parameters": {"full_attention": {"rope_type": "default", "rope_theta": shape.theta},
                                   "sliding_attention": {"rope_type": "default", "rope_theta": shape.theta_local}}},
              open(os.path.join(d, "config.json"), "w"))
    json.dump([{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
               {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
               {"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}],
              open(os.path.join(d, "modules.json"), "w"))
    json.dump({"word_embedding_dimension": 128, "pooling_mode_mean_tokens": True},
              open(os.path.join(d, "1_Pooling", "config.json"), "w"))
    json.dump({"max_seq_length": 64}, open(os.path.join(d, "sentence_bert_config.json"), "w"))
    w = mo.random_weights(shape, seed)
    save_file({"model." + k: np.ascontiguousarray(v) for k, v in w.items()}, os.path.join(d, "model.safetensors"))
    return shape, w, hf
