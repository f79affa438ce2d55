"""The post-pooling head without a GPU: the NumPy oracle against torch's modules (tests/golden/head_*.npz), the
modules.json reader on synthetic sentence-transformers directories, VOITTA_EMBED_TRUNCATE_DIM, the DistilBERT config reader
and weight mapping (tests/golden/distilbert_tiny.npz), the ABI struct, and the check that f32 reference arithmetic on
every GPU case clears the GPU tests' bar tenfold."""
import ctypes as C
import glob
import logging
import os
import subprocess

import numpy as np
import pytest

import head_oracle as ho
from oracle import bert as obert

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]"] + [f"w{i}" for i in range(60)]


@pytest.fixture
def settings(monkeypatch):
    from voitta_rag_amd import config

    def set_env(**env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        config.get_settings.cache_clear()

    monkeypatch.delenv("VOITTA_EMBED_TRUNCATE_DIM", raising=False)
    config.get_settings.cache_clear()
    yield set_env
    monkeypatch.undo()
    config.get_settings.cache_clear()


def _stage(kind, n_in, n_out, act="identity", bias=True, seed=0):
    return ho.head_weights(ho.HeadCase(ho.TINY, "mean", False, [(kind, n_in, n_out, act, bias)], seed=seed))[0]


# ---- the oracle against torch.nn ---------------------------------------------------------------------------------------------
def test_goldens_hold_the_listed_cases():
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(HERE, "golden", "head_*.npz")))
    assert names == sorted(f"head_{n}.npz" for n in ho.CASES)


@pytest.mark.parametrize("name", list(ho.CASES))
def test_oracle_matches_torch_modules(name):
    case = ho.CASES[name]
    g = np.load(os.path.join(HERE, "golden", f"head_{name}.npz"))
    got = ho.apply_head(g["rows"], ho.head_weights(case), case.normalize, case.truncate)
    assert got.shape == g["want"].shape == (g["rows"].shape[0], case.out_dim)
    assert np.max(np.abs(got - g["want"])) < 1e-13


def test_reference_arithmetic_clears_the_gpu_bar():
    """The project's f32 restatement of the encoder (oracle/bert_torch.py) followed by the head in f32 NumPy, against
    the f64 oracle, on every case and sequence the GPU tests run: |1 - cos| and the largest component difference (both
    rows divided by the oracle row's norm) stay below a tenth of test_encoder_gpu's TOL["f32"]. So the bar is one that
    plain f32 arithmetic clears with room, and a GPU result outside it is the kernel's doing. The head weights are
    drawn W ~ N(0, 1 / in_dim) from the start (head_oracle's docstring), so no case needed its scale changed."""
    from test_encoder_gpu import TOL

    from oracle.bert_torch import TorchBert

    cos_tol, abs_tol = TOL["f32"]
    for name, case in ho.CASES.items():
        w = obert.random_weights(case.shape, case.seed)
        seqs = ho.sequences(case)
        stages = ho.head_weights(case)
        want = ho.expected(case, w, seqs, stages)
        pooled32 = TorchBert(w, case.shape, case.pooling, normalize=False).encode(seqs)
        got = ho.apply_head(pooled32, stages, case.normalize, case.truncate, dtype=np.float32).astype(np.float64)
        norm = np.linalg.norm(want, axis=1, keepdims=True)
        got, want = got / norm, want / norm
        cos = (got * want).sum(1) / np.linalg.norm(got, axis=1)
        worst_cos, worst_abs = float(np.max(np.abs(1.0 - cos))), float(np.max(np.abs(got - want)))
        print(f"{name}: f32 reference worst |1-cos| {worst_cos:.2e}, worst abs {worst_abs:.2e}")
        assert worst_cos < cos_tol / 10 and worst_abs < abs_tol / 10, name


# ---- modules.json ----------------------------------------------------------------------------------------------------------------
def test_labse_like_directory(tmp_path, settings):
    from voitta_rag_amd.embedding import read_encoder_config

    dense = _stage("dense", 128, 128, "tanh", seed=1)
    ho.write_checkpoint(str(tmp_path), VOCAB, "bert", "cls", [dense, "Normalize"], body=False)
    desc = read_encoder_config(str(tmp_path))["desc"]
    assert (desc.pooling, desc.normalize, desc.hidden, desc.out_dim, desc.truncate_dim) == ("cls", True, 128, 128, 0)
    (st,) = desc.head
    assert (st.kind, st.activation, st.in_dim, st.out_dim) == ("dense", "tanh", 128, 128)
    assert np.array_equal(st.weight, dense["weight"]) and np.array_equal(st.bias, dense["bias"])


@pytest.mark.parametrize("weight_format", ["safetensors", "bin"])
def test_distiluse_like_directory(tmp_path, settings, weight_format):
    from voitta_rag_amd.embedding import read_encoder_config

    dense = _stage("dense", 128, 64, "tanh", seed=2)
    ho.write_checkpoint(str(tmp_path), VOCAB, "distilbert", "mean", [dense], body=False, weight_format=weight_format)
    assert os.path.exists(tmp_path / "2_Dense" / ("model.safetensors" if weight_format == "safetensors" else "pytorch_model.bin"))
    rc = read_encoder_config(str(tmp_path))
    desc = rc["desc"]
    assert (desc.pooling, desc.normalize, desc.hidden, desc.out_dim, desc.type_vocab) == ("mean", False, 128, 64, 1)
    assert np.array_equal(desc.head[0].weight, dense["weight"]) and np.array_equal(desc.head[0].bias, dense["bias"])


def test_two_dense_a_dropout_and_a_layernorm(tmp_path, settings):
    from voitta_rag_amd.embedding import read_encoder_config

    a, b = _stage("dense", 128, 256, "identity", bias=False, seed=3), _stage("dense", 256, 48, "identity", seed=4)
    ln = _stage("layernorm", 48, 48, seed=5)
    ho.write_checkpoint(str(tmp_path), VOCAB, "bert", "mean", [a, "Dropout", b, ln, "Normalize"], body=False)
    desc = read_encoder_config(str(tmp_path))["desc"]
    assert [(s.kind, s.activation, s.in_dim, s.out_dim, s.bias is None) for s in desc.head] == [
        ("dense", "identity", 128, 256, True), ("dense", "identity", 256, 48, False), ("layernorm", "identity", 48, 48, False)]
    assert desc.head[2].eps == 1e-5 and np.array_equal(desc.head[2].weight, ln["weight"])
    assert desc.out_dim == 48 and desc.normalize


def test_reader_refusals_and_warnings(tmp_path, settings, caplog):
    from voitta_rag_amd.embedding import read_encoder_config

    relu = dict(_stage("dense", 128, 128, seed=6), activation_class="torch.nn.modules.activation.ReLU")
    ho.write_checkpoint(str(tmp_path / "relu"), VOCAB, modules=[relu], body=False)
    with pytest.raises(ValueError, match=r"activation_function torch\.nn\.modules\.activation\.ReLU is not implemented"):
        read_encoder_config(str(tmp_path / "relu"))
    ho.write_checkpoint(str(tmp_path / "norm"), VOCAB, modules=["Normalize", _stage("dense", 128, 128, seed=7)], body=False)
    with pytest.raises(ValueError, match="Normalize followed by Dense"):
        read_encoder_config(str(tmp_path / "norm"))
    ho.write_checkpoint(str(tmp_path / "chain"), VOCAB, modules=[_stage("dense", 64, 128, seed=8)], body=False)
    with pytest.raises(ValueError, match="reads 64 columns, the pipeline in front of it gives 128"):
        read_encoder_config(str(tmp_path / "chain"))
    ho.write_checkpoint(str(tmp_path / "odd"), VOCAB, modules=["CNN", "Normalize"], body=False)
    with caplog.at_level(logging.WARNING, logger="voitta_rag_amd.embedding"):
        desc = read_encoder_config(str(tmp_path / "odd"))["desc"]
    assert any("sentence_transformers.models.CNN" in r.getMessage() for r in caplog.records)
    assert desc.head is None and desc.normalize and desc.out_dim == 128
    # the refusal of other families stays, with DistilBERT in the list of the supported ones
    import json

    cfg = json.load(open(tmp_path / "odd" / "config.json"))
    json.dump(dict(cfg, model_type="gpt2"), open(tmp_path / "odd" / "config.json", "w"))
    with pytest.raises(ValueError, match="unsupported model_type gpt2: BERT, DistilBERT,"):
        read_encoder_config(str(tmp_path / "odd"))


# ---- VOITTA_EMBED_TRUNCATE_DIM ---------------------------------------------------------------------------------------------------
def test_truncate_setting(tmp_path, settings):
    from voitta_rag_amd import config
    from voitta_rag_amd.embedding import read_encoder_config

    ho.write_checkpoint(str(tmp_path / "plain"), VOCAB, modules=["Normalize"], body=False)
    ho.write_checkpoint(str(tmp_path / "dense"), VOCAB, modules=[_stage("dense", 128, 64, "tanh", seed=9)], body=False)
    settings(EMBEDDING_DIMENSION="128")
    assert read_encoder_config(str(tmp_path / "plain"))["desc"].truncate_dim == 0  # unset: off
    settings(VOITTA_EMBED_TRUNCATE_DIM="32", EMBEDDING_DIMENSION="32")
    desc = read_encoder_config(str(tmp_path / "plain"))["desc"]
    assert (desc.truncate_dim, desc.out_dim, desc.hidden) == (32, 32, 128)
    desc = read_encoder_config(str(tmp_path / "dense"))["desc"]
    assert (desc.truncate_dim, desc.out_dim, desc.head[0].out_dim) == (32, 32, 64)
    settings(VOITTA_EMBED_TRUNCATE_DIM="128", EMBEDDING_DIMENSION="128")
    assert read_encoder_config(str(tmp_path / "plain"))["desc"].out_dim == 128
    with pytest.raises(ValueError, match="VOITTA_EMBED_TRUNCATE_DIM=128: .*output width 64"):  # within the HEAD's width
        read_encoder_config(str(tmp_path / "dense"))
    settings(VOITTA_EMBED_TRUNCATE_DIM="144", EMBEDDING_DIMENSION="144")
    with pytest.raises(ValueError, match="VOITTA_EMBED_TRUNCATE_DIM=144: .*output width 128"):
        read_encoder_config(str(tmp_path / "plain"))
    settings(VOITTA_EMBED_TRUNCATE_DIM="64", EMBEDDING_DIMENSION="128")
    with pytest.raises(ValueError, match="EMBEDDING_DIMENSION=128 but VOITTA_EMBED_TRUNCATE_DIM=64 makes the embeddings 64 wide"):
        read_encoder_config(str(tmp_path / "plain"))
    for bad in ("24", "0", "-16", "8"):
        settings(VOITTA_EMBED_TRUNCATE_DIM=bad)
        with pytest.raises(ValueError, match=f"VOITTA_EMBED_TRUNCATE_DIM={bad}: accepted values are the multiples of 16"):
            config.get_settings()
    settings(VOITTA_EMBED_TRUNCATE_DIM="")
    assert config.get_settings().embed_truncate_dim == 0


def test_description_out_dim():
    from voitta_rag_amd.encoder import BertDesc, HeadStage

    d = BertDesc(2, 128, 2, 256)
    assert d.out_dim == 128
    d.head = [HeadStage("dense", np.zeros((64, 128), np.float32))]
    assert d.out_dim == 64 and d == BertDesc(2, 128, 2, 256)  # (not compared, as the attention bias is not)
    d.truncate_dim = 16
    assert d.out_dim == 16


# ---- DistilBERT --------------------------------------------------------------------------------------------------------------------
def test_distilbert_config_reader(tmp_path, settings):
    import json

    from voitta_rag_amd.embedding import read_encoder_config

    ho.write_checkpoint(str(tmp_path), VOCAB, "distilbert", "mean", [], body=False, max_seq=512)
    rc = read_encoder_config(str(tmp_path))
    d = rc["desc"]
    assert (d.layers, d.hidden, d.heads, d.intermediate, d.vocab, d.max_pos, d.type_vocab) == (2, 128, 2, 256, len(VOCAB), 160, 1)
    assert (d.eps, d.position, d.ffn, d.norm, rc["pos_start"], rc["max_seq"]) == (1e-12, "learned", "gelu", "post", 0, 160)
    cfg = json.load(open(tmp_path / "config.json"))
    json.dump(dict(cfg, sinusoidal_pos_embds=True), open(tmp_path / "config.json", "w"))
    assert read_encoder_config(str(tmp_path))["desc"] == d  # the table comes from the checkpoint either way
    json.dump(dict(cfg, activation="relu"), open(tmp_path / "config.json", "w"))
    with pytest.raises(ValueError, match="activation 'relu' is not implemented"):
        read_encoder_config(str(tmp_path))


@pytest.mark.parametrize("prefix", ["", "distilbert."])
def test_distilbert_slots(prefix):
    from voitta_rag_amd import encoder as enc

    shape = ho.DISTIL_SHAPE
    w, state = ho.distilbert_weights(prefix=prefix)
    desc = enc.BertDesc(shape.layers, shape.hidden, shape.heads, shape.intermediate, vocab=shape.vocab, max_pos=shape.max_pos,
                        type_vocab=1)
    out = enc.distilbert_slots(state, desc)
    assert sorted(out) == sorted(enc.tensor_names(shape.layers))
    for name in enc.tensor_names(shape.layers):
        assert np.array_equal(out[name], w[name]), name
        assert tuple(out[name].shape) == enc.expected_shape(desc, name), name
    missing = prefix + "transformer.layer.1.ffn.lin2.bias"
    with pytest.raises(KeyError, match=r"transformer\.layer\.1\.ffn\.lin2\.bias"):
        enc.distilbert_slots({k: v for k, v in state.items() if k != missing}, desc)


def test_distilbert_golden_is_the_bert_oracle_on_the_mapped_weights():
    g = np.load(os.path.join(HERE, "golden", "distilbert_tiny.npz"))
    w, _ = ho.distilbert_weights()
    seqs = [g["ids"][a:b] for a, b in zip(g["offsets"][:-1], g["offsets"][1:])]
    assert [len(s) for s in seqs] == ho.LENS and int(g["seed"]) == ho.DISTIL_SEED
    got = obert.sentence_embeddings(w, ho.DISTIL_SHAPE, seqs, "mean", True, np.float64)
    assert np.max(np.abs(got - g["want"])) < 1e-13


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_head_stage_layout_matches_header(tmp_path):
    """sizeof(vr_head_stage) and its pointers' offsets, as gcc sees the header, equal the ctypes mirror."""
    from voitta_rag_amd import _lib

    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "voitta_engine.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu\\n",sizeof(vr_head_stage),offsetof(vr_head_stage,eps),'
                   'offsetof(vr_head_stage,weight),offsetof(vr_head_stage,bias));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _lib.VrHeadStage
    assert sizes == [C.sizeof(S), S.eps.offset, S.weight.offset, S.bias.offset]
    assert "vr_encoder_set_head" in _lib.SIGNATURES
