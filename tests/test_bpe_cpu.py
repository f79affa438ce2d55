"""The native byte-level BPE tokenizer (csrc/bpe.cpp, voitta_rag_amd/bpe.py) without a GPU: every id list the HF
`tokenizers` library recorded in tests/golden/bpe_tokenizer.json at every recorded max_len, a live comparison against the
installed library on seeded random strings, the short-buffer contract, the argument checks, from_pretrained and its
refusals, the model directory hooks, and the stand-alone sanitizer program."""
import copy
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import bpe_case as bc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def g():
    return bc.fixture()


@pytest.fixture(scope="module")
def tok(g):
    from voitta_rag_amd.bpe import BpeTokenizer

    return BpeTokenizer.from_tokenizer_json(g["tokenizer"])


def _rows(ids, off):
    return [ids[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]


def test_fixture_is_what_the_issue_lists(g):
    spec = g["tokenizer"]
    assert spec["normalizer"] == {"type": "NFC"} and spec["pre_tokenizer"]["type"] == "ByteLevel"
    assert 590 <= len(spec["model"]["vocab"]) <= 610 and os.path.getsize(os.path.join(HERE, "golden", "bpe_tokenizer.json")) < 100_000
    added = {a["content"]: a for a in spec["added_tokens"]}
    assert added["[MASK]"]["lstrip"] and not added["[SEP]"]["normalized"]
    assert all(added[" " * n]["normalized"] and not added[" " * n]["special"] for n in (2, 4, 8))
    assert sorted(g["expected"]["single"]) == sorted(g["expected"]["pairs"]) == ["16", "3", "512", "6"]
    texts = [bytes.fromhex(h) for h in g["texts_hex"]]
    assert b"" in texts and b"w" * 5000 in texts and any(b"\xff" in t for t in texts)


@pytest.mark.parametrize("max_len", [512, 16, 6, 3])
def test_recorded_ids(g, tok, max_len):
    tok.max_length = max_len
    texts = [bytes.fromhex(h) for h in g["texts_hex"]]
    assert _rows(*tok.encode(texts)) == g["expected"]["single"][str(max_len)]
    a, b = ([bytes.fromhex(h) for h in g[k]] for k in ("pair_a_hex", "pair_b_hex"))
    ids, off, seg = tok.encode_pairs(a, b)
    want = g["expected"]["pairs"][str(max_len)]
    assert _rows(ids, off) == want["ids"] and seg.tolist() == want["seg_b"]


def test_live_against_the_library(g, tok):
    pytest.importorskip("tokenizers")
    hf = bc.hf_tokenizer(g)
    texts = bc.random_texts(7, 3000)
    for max_len in (64, 9):
        tok.max_length = max_len
        hf.enable_truncation(max_length=max_len, strategy="longest_first")
        assert _rows(*tok.encode(texts)) == [e.ids for e in hf.encode_batch(texts)]
        a, b = texts[:1500], texts[1500:]
        encs = hf.encode_batch(list(zip(a, b)))
        ids, off, seg = tok.encode_pairs(a, b)
        assert _rows(ids, off) == [e.ids for e in encs]
        assert seg.tolist() == [next((i for i, s in enumerate(e.sequence_ids) if s == 1), len(e.ids) - 1) for e in encs]


def test_a_long_word_is_not_quadratic(tok):
    import time

    tok.max_length = 8192
    t0 = time.perf_counter()
    ids, off = tok.encode(["ab" * 100_000])
    assert time.perf_counter() - t0 < 5.0 and len(ids) == 8192


def test_short_buffer_contract_and_argument_checks(g, tok):
    from voitta_rag_amd._lib import EngineError, check

    lib = tok._lib
    tok.max_length = 16
    texts = [b"hello world", b"", b"a  b"]
    want_ids, want_off = tok.encode(texts)
    arr = (C.c_char_p * 3)(*texts)
    lens = np.array([len(t) for t in texts], np.int64)
    off = np.zeros(4, np.int64)
    needed = C.c_int64()
    p64, p32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    small = np.full(len(want_ids) - 1, -5, np.int32)
    rc = lib.vr_bpe_encode(tok._h, arr, lens.ctypes.data_as(p64), 3, 16, off.ctypes.data_as(p64), small.ctypes.data_as(p32),
                           len(small), C.byref(needed))
    assert rc == -2 and needed.value == len(want_ids) and off.tolist() == want_off.tolist() and (small == -5).all()
    rc = lib.vr_bpe_encode(tok._h, arr, lens.ctypes.data_as(p64), 3, 16, off.ctypes.data_as(p64), None, 0, C.byref(needed))
    assert rc == -2 and needed.value == len(want_ids)
    pids, poff, pseg = tok.encode_pairs(texts, texts[::-1])
    seg = np.zeros(3, np.int32)
    rc = lib.vr_bpe_encode_pairs(tok._h, arr, lens.ctypes.data_as(p64), arr, lens.ctypes.data_as(p64), 3, 16,
                                 off.ctypes.data_as(p64), None, seg.ctypes.data_as(p32), 0, C.byref(needed))
    assert rc == -2 and needed.value == sum(len(r) for r in _rows(*tok.encode_pairs(texts, texts)[:2]))
    for bad in (lambda: lib.vr_bpe_encode(tok._h, arr, lens.ctypes.data_as(p64), 3, 1, off.ctypes.data_as(p64), None, 0, C.byref(needed)),
                lambda: lib.vr_bpe_encode_pairs(tok._h, arr, lens.ctypes.data_as(p64), arr, lens.ctypes.data_as(p64), 3, 2,
                                                off.ctypes.data_as(p64), None, None, 0, C.byref(needed)),
                lambda: lib.vr_bpe_encode(None, arr, lens.ctypes.data_as(p64), 3, 16, off.ctypes.data_as(p64), None, 0, C.byref(needed)),
                lambda: lib.vr_bpe_encode(tok._h, None, None, 3, 16, off.ctypes.data_as(p64), None, 0, C.byref(needed))):
        with pytest.raises(EngineError):
            check(bad())
    from voitta_rag_amd.bpe import BpeTokenizer, parse_tokenizer_json

    args = parse_tokenizer_json(g["tokenizer"])
    for change, message in ((dict(cls_id=10_000), "cls / sep id"), (dict(unk_id=-3), "unk id"),
                            (dict(merges=[("zz", "qq")]), "merge 0"), (dict(added_flags=[64] * len(args["added"])), "unknown flags")):
        with pytest.raises(EngineError, match=message):
            BpeTokenizer(**dict(args, **change))


def test_from_pretrained_and_its_refusals(g, tmp_path):
    from voitta_rag_amd.bpe import BpeTokenizer

    def write(spec):
        json.dump(spec, open(tmp_path / "tokenizer.json", "w"))
        return str(tmp_path)

    t = BpeTokenizer.from_pretrained(write(g["tokenizer"]), max_length=32)
    assert t.max_length == 32 and t.vocab_size == len(g["tokenizer"]["model"]["vocab"]) + 3
    spec = g["tokenizer"]
    pair_only_single = copy.deepcopy(spec["post_processor"])
    pair_only_single["pair"] = [pair_only_single["pair"][1], pair_only_single["pair"][3]]
    for path, value, message in (
            (("model", "dropout"), 0.1, "model.dropout"), (("model", "ignore_merges"), True, "model.ignore_merges"),
            (("model", "byte_fallback"), True, "model.byte_fallback"),
            (("model", "continuing_subword_prefix"), "##", "model.continuing_subword_prefix"),
            (("model", "end_of_word_suffix"), "</w>", "model.end_of_word_suffix"),
            (("pre_tokenizer", "use_regex"), False, "pre_tokenizer.use_regex"),
            (("pre_tokenizer", "add_prefix_space"), True, "pre_tokenizer.add_prefix_space"),
            (("normalizer",), {"type": "NFKC"}, "normalizer 'NFKC'"),
            (("normalizer",), {"type": "Sequence", "normalizers": [{"type": "NFC"}, {"type": "Lowercase"}]}, "normalizer 'Sequence'"),
            (("pre_tokenizer",), {"type": "Sequence", "pretokenizers": []}, "pre_tokenizer 'Sequence'"),
            (("post_processor",), pair_only_single, "post_processor template"),
            (("post_processor",), {"type": "ByteLevel"}, "post_processor 'ByteLevel'"),
            (("model", "type"), "WordPiece", "model.type")):
        bad = copy.deepcopy(spec)
        node = bad
        for k in path[:-1]:
            node = node[k]
        node[path[-1]] = value
        with pytest.raises(ValueError, match=message):
            BpeTokenizer.from_pretrained(write(bad))
    none = copy.deepcopy(spec)
    none["normalizer"] = None  # no normaliser is part of the pipeline
    assert _rows(*BpeTokenizer.from_pretrained(write(none)).encode(["é"]))[0] != _rows(*t.encode(["é"]))[0]
    with pytest.raises(ValueError, match="no tokenizer.json"):
        BpeTokenizer.from_pretrained(str(tmp_path / "nothing"))


def test_a_modernbert_directory_gets_the_native_tokenizer(g, tmp_path):
    from voitta_rag_amd import embedding
    from voitta_rag_amd.bpe import BpeTokenizer
    from voitta_rag_amd.embedding import NativeSentenceEncoder

    json.dump(g["tokenizer"], open(tmp_path / "tokenizer.json", "w"))
    t = NativeSentenceEncoder._load_tokenizer(str(tmp_path), {"model_type": "modernbert"})
    assert isinstance(t, BpeTokenizer) and embedding.native_tokenizer(t)
    foreign = copy.deepcopy(g["tokenizer"])
    foreign["pre_tokenizer"]["add_prefix_space"] = True
    json.dump(foreign, open(tmp_path / "tokenizer.json", "w"))
    t = NativeSentenceEncoder._load_tokenizer(str(tmp_path), {"model_type": "modernbert"})
    assert not embedding.native_tokenizer(t)  # the library's object: the fallback


def test_sanitizer_program_builds_and_exits_clean(g, tmp_path):
    """csrc/tools/bpe_check.cpp with AddressSanitizer and UndefinedBehaviorSanitizer: a program of its own with the
    sanitizers' runtimes linked in statically, run as a child process in this process's environment as it is (the test
    preloads nothing and takes nothing away)."""
    from voitta_rag_amd.bpe import parse_tokenizer_json

    hx = lambda s: (s if isinstance(s, bytes) else s.encode("utf-8")).hex() or "-"  # noqa: E731
    a = parse_tokenizer_json(g["tokenizer"])
    lines = [f"P {a['unk_id']} {a['cls_id']} {a['sep_id']} {int(a['nfc'])}", f"V {len(a['vocab'])}"] + [hx(v) for v in a["vocab"]]
    lines += [f"M {len(a['merges'])}"] + [f"{hx(l)} {hx(r)}" for l, r in a["merges"]]
    lines += [f"A {len(a['added'])}"] + [f"{hx(c)} {i} {f}" for c, i, f in zip(a["added"], a["added_ids"], a["added_flags"])]
    single = [(ml, h, ids) for ml, rows in g["expected"]["single"].items() for h, ids in zip(g["texts_hex"], rows)]
    lines += [f"T {len(single)}"] + [f"{ml} {h or '-'} {len(ids)} " + " ".join(map(str, ids)) for ml, h, ids in single]
    pairs = [(ml, ha, hb, s, ids) for ml, rec in g["expected"]["pairs"].items()
             for ha, hb, s, ids in zip(g["pair_a_hex"], g["pair_b_hex"], rec["seg_b"], rec["ids"])]
    lines += [f"Q {len(pairs)}"] + [f"{ml} {ha or '-'} {hb or '-'} {s} {len(ids)} " + " ".join(map(str, ids))
                                    for ml, ha, hb, s, ids in pairs]
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    csrc = os.path.join(ROOT, "voitta_rag_amd", "csrc")
    exe = str(tmp_path / "bpe_check")
    srcs = [os.path.join(csrc, f) for f in ("tools/bpe_check.cpp", "bpe.cpp", "wordpiece.cpp", "unigram.cpp", "fusion.cpp",
                                            "host_stub.cpp")]
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                    "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I" + os.path.join(ROOT, "include"), "-I" + csrc, *srcs, "-o", exe, "-lpthread"], check=True,
                   capture_output=True)
    run = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    assert run.returncode == 0 and "bpe_check ok" in run.stdout and "ERROR" not in run.stderr, (run.stdout, run.stderr[-2000:])
