"""Generates tests/golden/long_rope_d64.npz and long_rope_d32.npz: seeded rotary, gated-FFN encoders (tests/rope_oracle.py's
weights, regenerated from the seed and never stored) on sequences of up to 8192 tokens, the lengths at which the f16
attention leaves the staged kernel for the streaming one and walks whole and partial 64-key tiles.
Run in the build container:  python tests/golden/make_long_golden.py

Stored: ids, offsets, the shape fields the other rope goldens store, and `want`: the f64 oracle's embeddings with the
EXACT cos/sin table, which is what the engine builds. transformers' own f32 table is not stored (at 8192 positions it is
megabytes, and its rounding grows with the position); instead the generator runs transformers' NomicBertModel in f64,
eager, one sequence at a time, and records two scalars per sequence:
  pin         : max-abs difference between transformers and the oracle fed transformers' own table (the oracle IS that
                model: ~1e-15; tests hold it below 1e-9, as for the other goldens)
  table_shift : max-abs difference between transformers and `want` (what the f32 table costs; informational)
`pinned_len` is the longest length the transformers run covered (every length, unless PIN_MAX_LEN lowers it for a
machine that cannot hold the 8192-token eager run; sequences past it record NaN)."""
import os
import sys

import numpy as np
import torch
import transformers

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import rope_oracle as ro  # noqa: E402
from make_rope_golden import hf_model  # noqa: E402

PIN_MAX_LEN = int(os.environ.get("PIN_MAX_LEN", "8192"))
CASES = {
    # name: (shape, pooling, seed, sequence lengths)
    # d_h = 64: 641 is the first length whose 16-padded key count does not stage, 656 sits just past the staged limit,
    # 705 = 11 whole tiles + 1 key, 1025 and 2049 are powers of two plus one, 8192 is the cap
    "d64": (ro.RopeShape(2, 128, 2, 256, vocab=500, max_pos=8192, act="silu"), "mean", 41,
            [1, 17, 641, 656, 705, 1025, 2049, 8192]),
    # d_h = 32 (staged up to 1280 keys), CLS pooling: the last layer computes query block 0 only
    "d32": (ro.RopeShape(2, 128, 4, 384, vocab=500, max_pos=8192, act="gelu", theta=10000.0), "cls", 42,
            [1, 17, 1281, 1296, 2049, 8192]),
}


def pooled(h, pooling):
    e = h[0] if pooling == "cls" else h.sum(axis=0) / float(len(h))
    return e / max(float(np.sqrt((e * e).sum())), 1e-12)


def main():
    for name, (shape, pooling, seed, lens) in CASES.items():
        w = ro.random_weights(shape, seed)
        model = hf_model(shape, w)
        rng = np.random.default_rng(seed + 1000)
        seqs = [rng.integers(0, shape.vocab, size=n).astype(np.int32) for n in lens]
        half = shape.hidden // shape.heads // 2
        with torch.no_grad():
            cos, sin = model.rotary_emb(torch.zeros(1, 1, dtype=torch.float32), torch.arange(max(lens))[None])
        table = cos[0, :, :half].numpy(), sin[0, :, :half].numpy()
        assert table[0].dtype == np.float32
        want = np.zeros((len(seqs), shape.hidden), np.float64)
        pin = np.full(len(seqs), np.nan)
        shift = np.full(len(seqs), np.nan)
        for i, ids in enumerate(seqs):
            want[i] = pooled(ro.encode_one(w, shape, ids), pooling)
            if len(ids) <= PIN_MAX_LEN:
                with torch.no_grad():
                    h = model(input_ids=torch.from_numpy(ids.astype(np.int64))[None]).last_hidden_state[0].numpy()
                hf = pooled(h, pooling)
                pin[i] = np.max(np.abs(hf - pooled(ro.encode_one(w, shape, ids, table=table), pooling)))
                shift[i] = np.max(np.abs(hf - want[i]))
            print(f"{name}: {len(ids):5d} tokens  pin {pin[i]:.3e}  table_shift {shift[i]:.3e}", flush=True)
        off = np.zeros(len(seqs) + 1, np.int32)
        off[1:] = np.cumsum(lens)
        path = os.path.join(HERE, f"long_rope_{name}.npz")
        np.savez_compressed(
            path, ids=np.concatenate(seqs), offsets=off, want=want, seed=seed, pooling=pooling, act=shape.act,
            theta=shape.theta, pin=pin, table_shift=shift, pinned_len=max(n for n in lens if n <= PIN_MAX_LEN),
            shape=np.array([shape.layers, shape.hidden, shape.heads, shape.intermediate, shape.vocab, shape.max_pos,
                            shape.type_vocab]), eps=shape.eps,
            versions=f"transformers {transformers.__version__}, torch {torch.__version__}, numpy {np.__version__}")
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
