"""Generates tests/golden/qwen3_rerank_tiny_d128b.npz and qwen3_rerank_tiny_d64n.npz: logits[last, yes] - logits[last, no]
of transformers' own Qwen3ForCausalLM (f64, eager attention, the seeded weights of tests/qwen3_rerank_oracle.random_weights),
every sequence run alone (no padding). The three f32 casts of the library — rotary angles, RMSNorm, the eager softmax —
are lifted exactly as make_qwen3_golden.py lifts them. Qwen3ForSequenceClassification with score.weight = W[yes] - W[no]
(one label, no padding token) must give the same numbers; the maker asserts it. Only ids, offsets, the shape, the seed
and the logits are stored; the weights are re-drawn from the seed by whoever reads the file.

  python tests/golden/make_qwen3_rerank_golden.py

  tiny_d128b : hidden 256, 4 heads of 128 over 2 KV heads (A = 512), tied embeddings: W = embed_tokens
  tiny_d64n  : hidden 128, 2 heads of 64, A = hidden, untied: W = lm_head
The lengths are make_qwen3_golden's attention edges, past the staged kernel's last length at head size 128 (320, 321, 449),
and the 100-token pair of the batch-invariance test. The seed of each shape is the first from its start value at which
the exposure property of tests/test_qwen3_rerank_cpu.py holds (a neighbouring row's logit is more than 0.1 away from the
pair's own for every pair), so that a gather that is off by one row cannot pass; the logits' spread is printed."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import qwen3_oracle as qo  # noqa: E402
import qwen3_rerank_oracle as ro  # noqa: E402

LENGTHS = [1, 2, 15, 16, 17, 63, 64, 65, 100, 127, 128, 129, 200, 320, 321, 449]
# name -> (shape, tied, first seed tried)
SHAPES = {"tiny_d128b": (qo.Qwen3Shape(2, 256, 4, 2, 256, 128), True, 122), "tiny_d64n": (qo.Qwen3Shape(2, 128, 2, 1, 256, 64), False, 123)}
EXPOSURE = 2 * 5e-2  # twice the f16 bar of tests/test_rerank_gpu.py


def lift_casts(model, shape):
    """f64 angles, RMSNorm and softmax in place of the library's f32 ones (make_qwen3_golden.library_rows)."""
    import transformers.models.qwen3.modeling_qwen3 as lib

    dh = shape.head_dim
    inv_freq = torch.tensor(shape.theta ** (-np.arange(0, dh, 2, dtype=np.float64) / dh), dtype=torch.float64)

    class Rotary64(torch.nn.Module):
        def forward(self, x, position_ids):
            a = position_ids[:, :, None].to(torch.float64) * torch.cat([inv_freq, inv_freq])[None, None, :]
            return a.cos(), a.sin()

    model.model.rotary_emb = Rotary64()

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


def config(shape, tied, **over):
    from transformers import Qwen3Config

    cfg = Qwen3Config(vocab_size=shape.vocab, hidden_size=shape.hidden, intermediate_size=shape.intermediate,
                      num_hidden_layers=shape.layers, num_attention_heads=shape.heads, num_key_value_heads=shape.kv_heads,
                      head_dim=shape.head_dim, hidden_act="silu", max_position_embeddings=512, rms_norm_eps=shape.eps,
                      rope_theta=shape.theta, attention_bias=shape.attention_bias, use_sliding_window=False,
                      attention_dropout=0.0, attn_implementation="eager", tie_word_embeddings=tied, **over)
    if getattr(cfg, "rope_parameters", None) is not None:  # (transformers 5 keeps the base there)
        cfg.rope_parameters["rope_theta"] = shape.theta
    return cfg


def library_logits(shape, tied, seed, seqs):
    from transformers import Qwen3ForCausalLM, Qwen3ForSequenceClassification

    w = ro.random_weights(shape, seed, tied)
    state = {"model." + k: torch.from_numpy(v).to(torch.float64) for k, v in ro.body_weights(w).items()}
    lm = Qwen3ForCausalLM(config(shape, tied)).to(torch.float64).eval()
    lm_state = dict(state)
    lm_state["lm_head.weight"] = torch.from_numpy(w[ro.LM_HEAD_KEY] if not tied else w[qo.WORD_KEY]).to(torch.float64)
    missing, unexpected = lm.load_state_dict(lm_state, strict=False)
    assert not unexpected and all("rotary" in k or "inv_freq" in k for k in missing), (missing, unexpected)
    if tied:
        assert lm.lm_head.weight.data_ptr() == lm.model.embed_tokens.weight.data_ptr() or \
            torch.equal(lm.lm_head.weight, lm.model.embed_tokens.weight)
    lift_casts(lm, shape)
    sc = Qwen3ForSequenceClassification(config(shape, tied, num_labels=1, pad_token_id=None)).to(torch.float64).eval()
    sc_state = dict(state)
    sc_state["score.weight"] = torch.from_numpy(ro.score_row(w))[None, :]
    missing, unexpected = sc.load_state_dict(sc_state, strict=False)
    assert not unexpected and all("rotary" in k or "inv_freq" in k for k in missing), (missing, unexpected)
    lift_casts(sc, shape)
    out, cls = [], []
    with torch.no_grad():
        for s in seqs:
            ids = torch.from_numpy(s.astype(np.int64))[None]
            lg = lm(input_ids=ids).logits[0, -1]
            out.append(float(lg[ro.YES_ID] - lg[ro.NO_ID]))
            cls.append(float(sc(input_ids=ids).logits[0, 0]))
    out, cls = np.asarray(out), np.asarray(cls)
    assert np.max(np.abs(out - cls)) < 1e-9, ("Qwen3ForSequenceClassification differs", np.max(np.abs(out - cls)))
    return out


def exposed(w, shape, seqs) -> bool:
    """Every pair's own logit is more than EXPOSURE away from its penultimate row's and from the next pair's first row's."""
    rows = [ro.row_logits(w, shape, s) for s in seqs]
    for i, r in enumerate(rows):
        near = ([r[-2]] if len(r) >= 2 else []) + ([rows[i + 1][0]] if i + 1 < len(rows) and len(r) >= 2 else [])
        if any(abs(v - r[-1]) <= EXPOSURE for v in near):
            return False
    return True


def main():
    for name, (shape, tied, seed) in SHAPES.items():
        while True:
            rng = np.random.default_rng(seed + 100)
            seqs = [rng.integers(0, shape.vocab, size=n).astype(np.int32) for n in LENGTHS]
            w = ro.random_weights(shape, seed, tied)
            if exposed(w, shape, seqs):
                break
            seed += 1
        logits = library_logits(shape, tied, seed, seqs)
        off = np.zeros(len(seqs) + 1, np.int32)
        off[1:] = np.cumsum(LENGTHS)
        path = os.path.join(HERE, f"qwen3_rerank_{name}.npz")
        np.savez_compressed(path, ids=np.concatenate(seqs), offsets=off, seed=seed, theta=shape.theta, eps=shape.eps,
                            shape=np.asarray([shape.layers, shape.hidden, shape.heads, shape.kv_heads, shape.intermediate,
                                              shape.head_dim, int(shape.qk_norm), shape.vocab, int(tied), ro.YES_ID, ro.NO_ID]),
                            logits=logits)
        mine = np.asarray([ro.logit(w, shape, s) for s in seqs])
        print(name, "seed", seed, os.path.getsize(path), "bytes; oracle - library:", float(np.max(np.abs(mine - logits))),
              "spread:", float(logits.max() - logits.min()), "logits:", np.round(logits, 3).tolist())


if __name__ == "__main__":
    main()
