"""Sequences of up to 8192 tokens without a GPU: the long goldens (tests/golden/make_long_golden.py) and their pin to
transformers, the VOITTA_MAX_SEQ_LENGTH setting in the config readers of embedders and rerankers (raised, lowered, out of
range, and unset: the behaviour before the setting existed), and the native tokenizers at max_length = 8192."""
import glob
import json
import logging
import os

import numpy as np
import pytest

import rope_oracle as ro
from test_rope_cpu import NATIVE, _dir
from test_xlmr_cpu import _embedder, _reranker

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "long_rope_*.npz")))
LENS = {"long_rope_d64.npz": [1, 17, 641, 656, 705, 1025, 2049, 8192], "long_rope_d32.npz": [1, 17, 1281, 1296, 2049, 8192]}


def test_goldens_cover_the_listed_lengths_and_are_pinned_to_transformers():
    assert [os.path.basename(p) for p in GOLDEN] == sorted(LENS)
    for path in GOLDEN:
        g = np.load(path)
        name = os.path.basename(path)
        assert np.diff(g["offsets"]).tolist() == LENS[name] and g["want"].dtype == np.float64
        assert os.path.getsize(path) < 256 * 1024 and all("weight" not in k and "rope_" not in k for k in g.files)
        L, H, nh, inter, vocab, max_pos, tv = (int(x) for x in g["shape"])
        assert (L, H, vocab, max_pos) == (2, 128, 500, 8192)
        assert (nh, inter, str(g["act"]), str(g["pooling"])) == ((2, 256, "silu", "mean") if "d64" in name else (4, 384, "gelu", "cls"))
        # transformers in f64 against the oracle fed transformers' own table, per sequence, up to the recorded length
        pinned = np.diff(g["offsets"]) <= int(g["pinned_len"])
        print(f"{name}: pinned up to {int(g['pinned_len'])} tokens, worst pin {np.nanmax(g['pin']):.3e}, "
              f"worst table shift {np.nanmax(g['table_shift']):.3e}")
        assert int(g["pinned_len"]) >= 2049 and np.all(g["pin"][pinned] < 1e-9) and np.all(np.isnan(g["pin"][~pinned]))


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p))
def test_oracle_reproduces_the_short_end_of_the_goldens(path):
    """`want` is the oracle with its exact table: the sequences of at most 705 tokens, recomputed here, to 1e-12."""
    g = np.load(path)
    L, H, nh, inter, vocab, max_pos, tv = (int(x) for x in g["shape"])
    shape = ro.RopeShape(L, H, nh, inter, vocab=vocab, max_pos=max_pos, type_vocab=tv, eps=float(g["eps"]),
                         theta=float(g["theta"]), act=str(g["act"]))
    w = ro.random_weights(shape, int(g["seed"]))
    off = g["offsets"]
    pick = [i for i in range(len(off) - 1) if off[i + 1] - off[i] <= 705]
    assert len(pick) >= 2
    got = ro.sentence_embeddings(w, shape, [g["ids"][off[i]:off[i + 1]] for i in pick], str(g["pooling"]))
    assert np.max(np.abs(got - g["want"][pick])) < 1e-12


# ---- the setting -----------------------------------------------------------------------------------------------------------
@pytest.fixture
def cap(monkeypatch):
    from voitta_rag_amd import config

    def set_cap(value):
        if value is None:
            monkeypatch.delenv("VOITTA_MAX_SEQ_LENGTH", raising=False)
        else:
            monkeypatch.setenv("VOITTA_MAX_SEQ_LENGTH", str(value))
        config.get_settings.cache_clear()

    yield set_cap
    monkeypatch.delenv("VOITTA_MAX_SEQ_LENGTH", raising=False)
    config.get_settings.cache_clear()


def _warnings(caplog):
    return [r for r in caplog.records if r.levelno == logging.WARNING]


def test_a_rotary_checkpoint_runs_at_the_raised_cap(tmp_path, caplog, cap):
    from voitta_rag_amd.embedding import read_encoder_config

    long = dict(NATIVE, max_position_embeddings=8192)
    cap(8192)
    with caplog.at_level(logging.WARNING, logger="voitta_rag_amd.embedding"):
        rc = read_encoder_config(_dir(tmp_path, long, max_seq=8192))
    assert rc["max_seq"] == 8192 and rc["desc"].max_pos == 8192 and not _warnings(caplog)
    # min(max_seq_length, max_position_embeddings, cap)
    assert read_encoder_config(_dir(tmp_path, long, max_seq=4096))["max_seq"] == 4096
    assert read_encoder_config(_dir(tmp_path, NATIVE, max_seq=8192))["max_seq"] == 2048
    cap(2048)
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="voitta_rag_amd.embedding"):
        rc = read_encoder_config(_dir(tmp_path, long, max_seq=8192))
    assert rc["max_seq"] == 2048 and rc["desc"].max_pos == 2048
    w = _warnings(caplog)
    assert len(w) == 1 and "8192" in w[0].getMessage() and "2048" in w[0].getMessage()
    assert "VOITTA_MAX_SEQ_LENGTH" in w[0].getMessage()


def test_xlmr_checkpoints_with_8192_positions_load_at_the_raised_cap(tmp_path, cap):
    from voitta_rag_amd.embedding import read_encoder_config
    from voitta_rag_amd.reranker import NativeCrossEncoder

    cap(8192)
    rc = read_encoder_config(_embedder(str(tmp_path / "a"), mpe=8194, max_seq=8192))  # bge-m3-like
    assert (rc["max_seq"], rc["desc"].max_pos, rc["pos_start"]) == (8192, 8192, 2)
    assert read_encoder_config(_embedder(str(tmp_path / "b"), mpe=8194))["max_seq"] == 8192
    # the reranker's length check passes: the next thing it asks for is the weight file
    with pytest.raises(FileNotFoundError, match="model.safetensors"):
        NativeCrossEncoder.from_pretrained(_reranker(str(tmp_path / "c"), mpe=8194, model_max=8192))
    cap(2048)  # above the cap: refused as before, naming the real cap and the variable
    with pytest.raises(ValueError, match=r"at most 2048.*VOITTA_MAX_SEQ_LENGTH"):
        read_encoder_config(_embedder(str(tmp_path / "d"), mpe=8194, max_seq=8192))
    with pytest.raises(ValueError, match=r"at most 2048.*VOITTA_MAX_SEQ_LENGTH"):
        NativeCrossEncoder.from_pretrained(_reranker(str(tmp_path / "e"), mpe=8194, model_max=8192))
    assert read_encoder_config(_embedder(str(tmp_path / "f"), mpe=8194, max_seq=2048))["max_seq"] == 2048


@pytest.mark.parametrize("value", ["0", "8193", "-5"])
def test_values_outside_1_to_8192_are_refused_at_start(cap, value):
    from voitta_rag_amd import config

    cap(value)
    with pytest.raises(ValueError, match="VOITTA_MAX_SEQ_LENGTH"):
        config.get_settings()
    cap(1)
    assert config.get_settings().max_seq_length == 1
    cap(8192)
    assert config.get_settings().max_seq_length == 8192


def test_unset_the_cap_is_512_as_before(tmp_path, caplog, cap):
    from voitta_rag_amd import config
    from voitta_rag_amd.embedding import MAX_SEQ, read_encoder_config
    from voitta_rag_amd.reranker import NativeCrossEncoder

    cap(None)
    assert config.get_settings().max_seq_length == MAX_SEQ == 512
    with caplog.at_level(logging.WARNING, logger="voitta_rag_amd.embedding"):
        rc = read_encoder_config(_dir(tmp_path, dict(NATIVE, max_position_embeddings=8192), max_seq=8192))
    assert rc["max_seq"] == 512 and rc["desc"].max_pos == 512
    w = _warnings(caplog)
    assert len(w) == 1 and "8192" in w[0].getMessage() and "512" in w[0].getMessage()
    with pytest.raises(ValueError, match="max_seq_length"):
        read_encoder_config(_embedder(str(tmp_path / "e"), mpe=8194, max_seq=8192))
    assert read_encoder_config(_embedder(str(tmp_path / "g"), mpe=8194, max_seq=512))["max_seq"] == 512
    with pytest.raises(ValueError, match="max_length"):
        NativeCrossEncoder.from_pretrained(_reranker(str(tmp_path / "c"), mpe=8194, model_max=8192))


# ---- tokenizers at max_length = 8192 -------------------------------------------------------------------------------------
def test_wordpiece_truncates_20000_pieces_to_8192_ids_like_hf():
    pytest.importorskip("tokenizers")
    from voitta_rag_amd.embedding import build_wordpiece_tokenizer
    from voitta_rag_amd.wordpiece import WordPieceTokenizer

    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "vector", "search", "##ing", "kernel", "##s", "."]
    rng = np.random.default_rng(8)
    words = rng.choice(["vector", "searching", "kernels", "search", ".", "zzz"], size=15000)
    text = " ".join(words)  # 15000 words, ~20000 pieces
    hf = build_wordpiece_tokenizer(vocab, True)
    hf.enable_truncation(max_length=10**6)
    assert len(hf.encode(text).ids) >= 20000
    hf.enable_truncation(max_length=8192)
    want = [np.asarray(x.ids, np.int32) for x in hf.encode_batch([text, "vector search."])]
    ids, off = WordPieceTokenizer(vocab, max_length=8192).encode_batch([text, "vector search."])
    assert off.tolist() == [0, 8192, 8192 + len(want[1])] and ids[0] == 2 and ids[8191] == 3
    assert np.array_equal(ids[:8192], want[0]) and np.array_equal(ids[8192:], want[1])


def test_unigram_truncates_20000_pieces_to_8192_ids_like_hf():
    tokenizers = pytest.importorskip("tokenizers")
    import xlmr_oracle as xo

    from voitta_rag_amd.unigram import UnigramTokenizer

    fixture = json.load(open(os.path.join(HERE, "golden", "xlmr_tokenizer.json"), encoding="utf-8"))
    spec = xo.tokenizer_spec(fixture, "metaspace")
    pool = [t for t in fixture["texts"] if t.strip()]
    rng = np.random.default_rng(9)
    hf = tokenizers.Tokenizer.from_str(json.dumps(spec))
    text = " ".join(pool[int(i)] for i in rng.integers(0, len(pool), size=400))
    while len(hf.encode(text).ids) < 20000:
        text += " " + " ".join(pool[int(i)] for i in rng.integers(0, len(pool), size=400))
    hf.enable_truncation(max_length=8192, strategy="longest_first")
    want = [np.asarray(x.ids, np.int32) for x in hf.encode_batch([text, pool[0]])]
    ids, off = UnigramTokenizer.from_tokenizer_json(spec, 8192).encode_batch([text, pool[0]])
    assert off.tolist() == [0, 8192, 8192 + len(want[1])]
    assert np.array_equal(ids[:8192], want[0]) and np.array_equal(ids[8192:], want[1])
