"""Generates tests/golden/qwen3_tiny_d128.npz, qwen3_tiny_d128b.npz and qwen3_tiny_d64n.npz: the rows of transformers' own
Qwen3Model (f64, eager attention, the seeded weights of tests/qwen3_oracle.random_weights), every sequence run alone (no
padding), both the last-token and the mean row recorded, L2-normalised. As for Qwen2 (make_qwen2_golden.py) the library
computes three things in f32 whatever the model's dtype — the rotary angles, RMSNorm (the per-head Q/K norms are the
same class) and the softmax; library_rows lifts those casts. Only ids, offsets, the shape and the rows are stored; the
weights are re-drawn from the seed by whoever reads the file.

  python tests/golden/make_qwen3_golden.py

The lengths are the edges of the three attention kernels: the 16-query tile, the 64-key tile, the 64-query block of the
f32 kernel and the 128-query block of the streamed one.
  tiny_d128  : hidden 128, 2 heads of 128 over 1 KV head — the attention width 256 is not the hidden size
  tiny_d128b : hidden 256, 4 heads of 128 over 2 KV heads — width 512
  tiny_d64n  : hidden 128, 2 heads of 64 over 1 KV head with the Q/K norms — width = hidden, the norm without head size 128"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import qwen3_oracle as qo  # noqa: E402

LENGTHS = [1, 2, 3, 15, 16, 17, 33, 63, 64, 65, 100, 127, 128, 129, 200]
SHAPES = {"tiny_d128": (qo.Qwen3Shape(2, 128, 2, 1, 256, 128), 21), "tiny_d128b": (qo.Qwen3Shape(2, 256, 4, 2, 256, 128), 22),
          "tiny_d64n": (qo.Qwen3Shape(2, 128, 2, 1, 256, 64), 23)}


def library_rows(shape, seed, seqs):
    from transformers import Qwen3Config, Qwen3Model

    cfg = Qwen3Config(vocab_size=shape.vocab, hidden_size=shape.hidden, intermediate_size=shape.intermediate,
                      num_hidden_layers=shape.layers, num_attention_heads=shape.heads, num_key_value_heads=shape.kv_heads,
                      head_dim=shape.head_dim, hidden_act="silu", max_position_embeddings=512, rms_norm_eps=shape.eps,
                      rope_theta=shape.theta, attention_bias=shape.attention_bias, use_sliding_window=False,
                      attention_dropout=0.0, attn_implementation="eager")
    if getattr(cfg, "rope_parameters", None) is not None:  # (transformers 5 keeps the base there)
        cfg.rope_parameters["rope_theta"] = shape.theta
    model = Qwen3Model(cfg).to(torch.float64).eval()
    w = qo.random_weights(shape, seed)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v).to(torch.float64) for k, v in w.items()}, strict=False)
    assert not unexpected and all("rotary" in k or "inv_freq" in k for k in missing), (missing, unexpected)
    # f64 angles in place of the library's f32 ones: cos / sin of p * theta^(-2i/d_h), repeated for both halves of the head
    dh = shape.head_dim
    inv_freq = torch.tensor(shape.theta ** (-np.arange(0, dh, 2, dtype=np.float64) / dh), dtype=torch.float64)

    class Rotary64(torch.nn.Module):
        def forward(self, x, position_ids):
            a = position_ids[:, :, None].to(torch.float64) * torch.cat([inv_freq, inv_freq])[None, None, :]
            return a.cos(), a.sin()

    model.rotary_emb = Rotary64()
    # ... and RMSNorm (which casts the row to f32; q_norm and k_norm are instances of it) and the eager softmax
    # (dtype=torch.float32): the same two formulas without the casts, in place of the library's for this run.
    import transformers.models.qwen3.modeling_qwen3 as lib

    def rms64(self, x):
        return self.weight * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.variance_epsilon))

    def eager64(module, query, key, value, attention_mask, scaling, dropout=0.0, **kwargs):
        k = lib.repeat_kv(key, module.num_key_value_groups)
        v = lib.repeat_kv(value, module.num_key_value_groups)
        s = torch.matmul(query, k.transpose(2, 3)) * scaling
        if attention_mask is not None:
            s = s + attention_mask
        p = torch.nn.functional.softmax(s, dim=-1)
        return torch.matmul(p, v).transpose(1, 2).contiguous(), p

    lib.Qwen3RMSNorm.forward = rms64
    lib.eager_attention_forward = eager64
    rows = {"last": [], "mean": []}
    with torch.no_grad():
        for s in seqs:
            h = model(input_ids=torch.from_numpy(s.astype(np.int64))[None]).last_hidden_state[0].numpy()
            rows["last"].append(qo.pool(h, "last"))
            rows["mean"].append(qo.pool(h, "mean"))
    return {k: np.stack(v) for k, v in rows.items()}


def main():
    for name, (shape, seed) in SHAPES.items():
        rng = np.random.default_rng(seed + 100)
        seqs = [rng.integers(0, shape.vocab, size=n).astype(np.int32) for n in LENGTHS]
        rows = library_rows(shape, seed, seqs)
        off = np.zeros(len(seqs) + 1, np.int32)
        off[1:] = np.cumsum(LENGTHS)
        path = os.path.join(HERE, f"qwen3_{name}.npz")
        np.savez_compressed(path, ids=np.concatenate(seqs), offsets=off, seed=seed, theta=shape.theta, eps=shape.eps,
                            shape=np.asarray([shape.layers, shape.hidden, shape.heads, shape.kv_heads, shape.intermediate,
                                              shape.head_dim, int(shape.qk_norm), shape.vocab]),
                            last=rows["last"], mean=rows["mean"])
        w = qo.random_weights(shape, seed)
        mine = {p: qo.sentence_embeddings(w, shape, seqs, p) for p in ("last", "mean")}
        print(name, os.path.getsize(path), "bytes; oracle - library:",
              {p: float(np.max(np.abs(mine[p] - rows[p]))) for p in mine},
              "peaked share at 200 tokens:", qo.peaked_share(w, shape, seqs[-1]))


if __name__ == "__main__":
    main()
