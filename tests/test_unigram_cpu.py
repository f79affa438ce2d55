"""The native Unigram tokenizer (vr_unigram_*, csrc/unigram.cpp) against HF tokenizers, id for id: the recorded ids of
tests/golden/xlmr_tokenizer.json (both XLM-R pre-tokenizer shapes, no charsmap, equal-score ties; single texts and
LongestFirst pairs at several max_len), the live library where it is importable, and a model trained on the fly with
sentencepiece's full nmt_nfkc charsmap where sentencepiece is. Also the tokenizer.json shapes from_pretrained accepts
and refuses, and the C-ABI's argument checks."""
import json
import os
import random

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "xlmr_tokenizer.json"), encoding="utf-8"))
CASES = sorted(FIXTURE["cases"])


def _spec(case):
    import xlmr_oracle as xo

    return xo.tokenizer_spec(FIXTURE, case)


def _native(spec, max_len):
    from voitta_rag_amd.unigram import UnigramTokenizer

    return UnigramTokenizer.from_tokenizer_json(spec, max_len)


def _split(ids, off):
    return [ids[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("max_len", ["512", "6"])
def test_single_texts_match_recorded_hf_ids(case, max_len):
    c = FIXTURE["cases"][case]
    texts = FIXTURE["tie_texts"] if case == "ties" else FIXTURE["texts"]
    tok = _native(_spec(case), int(max_len))
    got = _split(*tok.encode_batch(texts))
    for text, g, w in zip(texts, got, c["single"][max_len]):
        assert g == w, (case, max_len, text)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("max_len", ["512", "16"])
def test_pairs_match_recorded_hf_ids(case, max_len):
    c = FIXTURE["cases"][case]
    pairs = FIXTURE["pairs"]
    tok = _native(_spec(case), int(max_len))
    ids, off, seg = tok.encode_pairs([a for a, _ in pairs], [b for _, b in pairs])
    got = _split(ids, off)
    for (a, b), g, w, s in zip(pairs, got, c["pair"][max_len], seg):
        assert g == w, (case, max_len, a, b)
        assert g[s - 2:s] == [2, 2] and g[0] == 0 and g[-1] == 2  # seg_b: the first id after "</s> </s>"


def test_live_hf_on_random_multilingual_text():
    tokenizers = pytest.importorskip("tokenizers")
    rng = random.Random(5)
    alphabet = (list("abcdefghij  ") + list("ａｂｃ①②ﬁ") + ["é", "가", " ", "　", "​"]
                + list("中文한국어кириллицаαβγ") + ["👩‍💻", "🇫🇷", "<s>", "</s>", " <mask>", "<unk>", "\t", "\n"])
    texts = ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, 40))) for _ in range(400)]
    for case in CASES:
        spec = _spec(case)
        hf = tokenizers.Tokenizer.from_str(json.dumps(spec))
        for max_len in (512, 9):
            hf.enable_truncation(max_length=max_len, strategy="longest_first")
            tok = _native(spec, max_len)
            want = [e.ids for e in hf.encode_batch(texts)]
            assert _split(*tok.encode_batch(texts)) == want, case
            pairs = list(zip(texts[::2], texts[1::2]))
            want = [e.ids for e in hf.encode_batch(pairs)]
            ids, off, _ = tok.encode_pairs([a for a, _ in pairs], [b for _, b in pairs])
            assert _split(ids, off) == want, case


def test_full_nmt_nfkc_charsmap_against_hf():
    """A model trained on the fly with sentencepiece's built-in nmt_nfkc rules (a charsmap of ~240 KB), through
    transformers' own XLM-R conversion shape, over a larger multilingual corpus."""
    spm = pytest.importorskip("sentencepiece")
    tokenizers = pytest.importorskip("tokenizers")
    import io

    from sentencepiece import sentencepiece_model_pb2 as spm_pb

    rng = random.Random(11)
    pool = [t for t in FIXTURE["texts"] if t.strip()]
    corpus = [" ".join(rng.choice(pool) for _ in range(3)) for _ in range(2000)]
    buf = io.BytesIO()
    spm.SentencePieceTrainer.train(sentence_iterator=iter(corpus), model_writer=buf, model_type="unigram",
                                   vocab_size=400, hard_vocab_limit=False, character_coverage=0.99, normalization_rule_name="nmt_nfkc",
                                   minloglevel=2, num_threads=1)
    proto = spm_pb.ModelProto()
    proto.ParseFromString(buf.getvalue())
    charsmap = proto.normalizer_spec.precompiled_charsmap
    assert len(charsmap) > 100_000
    vocab = ([("<s>", 0.0), ("<pad>", 0.0), ("</s>", 0.0), ("<unk>", 0.0)]
             + [(p.piece, p.score) for p in proto.pieces[3:]] + [("<mask>", 0.0)])
    base = _spec("metaspace")
    base["model"]["vocab"] = [list(v) for v in vocab]
    import base64

    for at in base["added_tokens"]:
        if at["content"] == "<mask>":
            at["id"] = len(vocab) - 1
    base["normalizer"]["normalizers"][0]["precompiled_charsmap"] = base64.b64encode(charsmap).decode()
    weird = "ǅǈ ﬃ ㎏ ㍱ Ⅻ ⑳ ｶﾞ ﾊﾟ ℌ ℍ ＡＢ ¼ ½ ² ³ ™ ℃ Å Ω K ﬀ ǆ ŉ ẛ ̈́ ᾳ ῲ ﹏ ︴ 〜 ～ ￡ ￦ ｟ ｠ ﾠ ᅠ"
    texts = corpus[:500] + [weird, weird.replace(" ", ""), "é́ ﬁ́", "ｶﾞｷﾞ"]
    for shape in ("metaspace", "whitespace_metaspace"):
        spec = json.loads(json.dumps(base))
        if shape == "whitespace_metaspace":
            spec["normalizer"] = spec["normalizer"]["normalizers"][0]
            spec["pre_tokenizer"] = {"type": "Sequence", "pretokenizers": [
                {"type": "WhitespaceSplit"}, {"type": "Metaspace", "replacement": "▁", "prepend_scheme": "always",
                                              "split": True}]}
        hf = tokenizers.Tokenizer.from_str(json.dumps(spec))
        hf.enable_truncation(max_length=512, strategy="longest_first")
        want = [e.ids for e in hf.encode_batch(texts)]
        assert _split(*_native(spec, 512).encode_batch(texts)) == want


def test_prepend_schemes_and_legacy_metaspace():
    tokenizers = pytest.importorskip("tokenizers")
    texts = ["hello world", "  two  spaces", "<s>after", "x <mask> y", "", "a\tb"]
    for shape in CASES[:2]:
        for pt in ({"type": "Metaspace", "replacement": "▁", "add_prefix_space": True},
                   {"type": "Metaspace", "replacement": "▁", "add_prefix_space": False},
                   {"type": "Metaspace", "replacement": "▁", "prepend_scheme": "first", "split": True},
                   {"type": "Metaspace", "replacement": "▁", "prepend_scheme": "never", "split": True}):
            spec = _spec(shape)
            if spec["pre_tokenizer"]["type"] == "Sequence":
                spec["pre_tokenizer"]["pretokenizers"][1] = pt
            else:
                spec["pre_tokenizer"] = pt
            if "add_prefix_space" in pt:  # what tokenizers 0.22 reads such a file as
                hf_spec = json.loads(json.dumps(spec).replace('"add_prefix_space": true', '"prepend_scheme": "always"')
                                     .replace('"add_prefix_space": false', '"prepend_scheme": "never"'))
            else:
                hf_spec = spec
            hf = tokenizers.Tokenizer.from_str(json.dumps(hf_spec))
            want = [e.ids for e in hf.encode_batch(texts)]
            assert _split(*_native(spec, 512).encode_batch(texts)) == want, (shape, pt)


def test_added_token_flags():
    tokenizers = pytest.importorskip("tokenizers")
    spec = _spec("metaspace")
    n = len(spec["model"]["vocab"])
    spec["model"]["vocab"] += [["[R]", 0.0], ["[W]", 0.0], ["[LR]", 0.0]]
    spec["added_tokens"] += [
        {"id": n, "content": "[R]", "single_word": False, "lstrip": False, "rstrip": True, "normalized": False, "special": True},
        {"id": n + 1, "content": "[W]", "single_word": True, "lstrip": False, "rstrip": False, "normalized": False, "special": True},
        {"id": n + 2, "content": "[LR]", "single_word": False, "lstrip": True, "rstrip": True, "normalized": False, "special": True}]
    hf = tokenizers.Tokenizer.from_str(json.dumps(spec))
    texts = ["a [R]  b", "x[W]y", "x [W] y", "[W]", "é[W]", "1[W]", "a  [LR]  b", "[R][R] [LR][LR]", "<mask>[R] <mask>",
             "中[W]文", "_[W]_", "-[W]-", "[W]_", "a\u0301[W]", "\u200d[W]", "‿[W]", "½[W]", "٣[W]"]
    want = [e.ids for e in hf.encode_batch(texts)]
    assert _split(*_native(spec, 512).encode_batch(texts)) == want


def test_malformed_utf8_becomes_replacement_character():
    from voitta_rag_amd._lib import load_library
    import ctypes as C

    tok = _native(_spec("metaspace"), 64)
    lib = load_library()
    raw = [b"ab\xffcd\xe4\xb8", b"\xc3"]
    arr = (C.c_char_p * 2)(*raw)
    lens = np.array([len(r) for r in raw], np.int64)
    off = np.zeros(3, np.int64)
    ids = np.zeros(64, np.int32)
    need = C.c_int64()
    assert lib.vr_unigram_encode(tok._h, arr, lens.ctypes.data_as(C.POINTER(C.c_int64)), 2, 64,
                                 off.ctypes.data_as(C.POINTER(C.c_int64)), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                 64, C.byref(need)) == 0
    want, _ = tok.encode_batch(["ab�cd�", "�"])
    assert ids[:need.value].tolist() == want.tolist()


def test_short_buffer_reports_needed():
    import ctypes as C

    from voitta_rag_amd._lib import load_library

    tok = _native(_spec("metaspace"), 64)
    lib = load_library()
    raw = [b"hello world", b"quick brown fox"]
    arr = (C.c_char_p * 2)(*raw)
    lens = np.array([len(r) for r in raw], np.int64)
    off = np.zeros(3, np.int64)
    ids = np.zeros(2, np.int32)
    need = C.c_int64()
    assert lib.vr_unigram_encode(tok._h, arr, lens.ctypes.data_as(C.POINTER(C.c_int64)), 2, 64,
                                 off.ctypes.data_as(C.POINTER(C.c_int64)), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                 2, C.byref(need)) == -2
    full, foff = tok.encode_batch([r.decode() for r in raw])
    assert need.value == full.size and off.tolist() == foff.tolist()


def test_from_pretrained_accepts_xlmr_shapes_and_refuses_others(tmp_path):
    from voitta_rag_amd.unigram import UnigramTokenizer, is_unigram_pipeline

    for case in CASES:
        d = tmp_path / case
        d.mkdir()
        (d / "tokenizer.json").write_text(json.dumps(_spec(case)), encoding="utf-8")
        assert UnigramTokenizer.from_pretrained(str(d), 128).max_length == 128
    base = _spec("metaspace")

    def variant(edit):
        spec = json.loads(json.dumps(base))
        edit(spec)
        return spec

    bad = [
        variant(lambda s: s["model"].update(type="BPE")),
        variant(lambda s: s["model"].update(byte_fallback=True)),
        variant(lambda s: s.update(normalizer={"type": "NFKC"})),
        variant(lambda s: s["normalizer"]["normalizers"].append({"type": "Lowercase"})),
        variant(lambda s: s["normalizer"]["normalizers"].insert(0, {"type": "Strip", "left": False, "right": True})),
        variant(lambda s: s["normalizer"]["normalizers"][1].update(content="▁")),
        variant(lambda s: s.update(pre_tokenizer={"type": "ByteLevel"})),
        variant(lambda s: s["pre_tokenizer"].update(split=False)),
        variant(lambda s: s.update(post_processor={"type": "BertProcessing", "sep": ["</s>", 2], "cls": ["<s>", 0]})),
        variant(lambda s: s["added_tokens"][0].update(normalized=True)),
    ]
    for spec in bad:
        assert not is_unigram_pipeline(spec)
    roberta = variant(lambda s: s.update(post_processor={"type": "RobertaProcessing", "sep": ["</s>", 2],
                                                         "cls": ["<s>", 0], "trim_offsets": True,
                                                         "add_prefix_space": True}))
    assert is_unigram_pipeline(roberta)
    assert is_unigram_pipeline(variant(lambda s: s.update(normalizer=None)))


def test_create_argument_checks():
    from voitta_rag_amd._lib import EngineError
    from voitta_rag_amd.unigram import UnigramTokenizer

    with pytest.raises(EngineError, match="unk / bos / eos"):
        UnigramTokenizer(["a", "b"], [0.0, -1.0], 5, 0, 1)
    with pytest.raises(EngineError, match="charsmap"):
        UnigramTokenizer(["a", "b"], [0.0, -1.0], 0, 0, 1, charsmap=b"\xff\xff\x00\x00xx")
    with pytest.raises(EngineError, match="pre-tokenizer"):
        UnigramTokenizer(["a", "b"], [0.0, -1.0], 0, 0, 1, pre_tokenizer=7)
    tok = UnigramTokenizer(["<s>", "</s>", "<unk>", "▁a"], [0.0, 0.0, 0.0, -1.0], 2, 0, 1, max_length=3)
    with pytest.raises(EngineError, match="max_len"):
        tok.encode_pairs(["a"], ["a"])
    tok.max_length = 2
    assert tok.encode_batch(["a a a"])[0].tolist() == [0, 1]


def test_short_texts_fill_their_sequences():
    """One-character texts: <s> ▁ x </s> is four ids for one input byte (Metaspace adds a piece no byte pays for)."""
    for case in CASES:
        tok = _native(_spec(case), 512)
        for texts in (["x", "y", "x"], ["a a a a a"] * 3, ["hello", "x"] * 5, ["ﬀ", "①"] * 40, ["é"] * 200, [""] * 7):
            ids, off = tok.encode_batch(texts)
            assert off[-1] == ids.size and np.all(np.diff(off) >= 2)
            assert all(ids[off[i]] == 0 and ids[off[i + 1] - 1] == 2 for i in range(len(texts)))
    tok = _native(_spec("metaspace"), 3)
    ids, off = tok.encode_batch(["x y z"] * 9)
    assert np.diff(off).tolist() == [3] * 9
