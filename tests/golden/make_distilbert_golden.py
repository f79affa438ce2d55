"""Generates tests/golden/distilbert_tiny.npz: a seeded DistilBERT encoder (tests/head_oracle.py's distilbert_weights) run
through transformers.DistilBertModel in f64, each sequence alone (batch of one, no padding), then mean-pooled and
normalised as sentence-transformers does. The model weights are NOT stored: head_oracle.distilbert_weights regenerates
them from the seed. Stored: ids, offsets, the expected embeddings, the shape, seed and the library versions.
Run in the build container:  python tests/golden/make_distilbert_golden.py"""
import os
import sys

import numpy as np
import torch
import transformers

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import head_oracle as ho  # noqa: E402
from oracle import bert as obert  # noqa: E402

if __name__ == "__main__":
    shape, seed = ho.DISTIL_SHAPE, ho.DISTIL_SEED
    w, state = ho.distilbert_weights(shape, seed)
    cfg = transformers.DistilBertConfig(vocab_size=shape.vocab, max_position_embeddings=shape.max_pos, n_layers=shape.layers,
                                        n_heads=shape.heads, dim=shape.hidden, hidden_dim=shape.intermediate, dropout=0.0,
                                        attention_dropout=0.0, activation="gelu", sinusoidal_pos_embds=False)
    cfg._attn_implementation = "eager"
    model = transformers.DistilBertModel(cfg)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
    assert not unexpected and not [m for m in missing if "position_ids" not in m], (missing, unexpected)
    model = model.double().eval()
    rng = np.random.default_rng(seed + 1000)
    seqs = [rng.integers(1, shape.vocab, size=n).astype(np.int32) for n in ho.LENS]
    want = np.zeros((len(seqs), shape.hidden), np.float64)
    with torch.no_grad():
        for i, ids in enumerate(seqs):
            h = model(input_ids=torch.from_numpy(ids.astype(np.int64))[None]).last_hidden_state[0].numpy()
            e = h.sum(axis=0) / len(ids)
            want[i] = e / np.sqrt((e * e).sum())
    got = obert.sentence_embeddings(w, shape, seqs, "mean", True, np.float64)
    print(f"BERT oracle on the renamed weights vs transformers max-abs {np.max(np.abs(got - want)):.3e}")
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum(ho.LENS)
    path = os.path.join(HERE, "distilbert_tiny.npz")
    np.savez_compressed(path, ids=np.concatenate(seqs), offsets=off, want=want, seed=seed,
                        shape=np.array([shape.layers, shape.hidden, shape.heads, shape.intermediate, shape.vocab, shape.max_pos]),
                        versions=f"transformers {transformers.__version__}, torch {torch.__version__}, numpy {np.__version__}")
    print("wrote", path, os.path.getsize(path), "bytes")
