"""Generates tests/golden/rope_*.npz: seeded rotary, gated-FFN encoders (tests/rope_oracle.py's weights) run through
transformers.NomicBertModel in f64 with eager attention, then pooled and normalised as sentence-transformers does.
Each sequence runs alone (batch of one, no padding).
Run in the build container:  python tests/golden/make_rope_golden.py
The model weights are NOT stored: rope_oracle.random_weights regenerates them from the seed. Stored: ids, offsets,
the expected embeddings, the shape, seed, theta, gate activation, pooling, the library versions, and the f32 cos/sin
table transformers rotated with (rope_cos / rope_sin [512, d_h/2]: it computes the table in f32 even for an f64 model,
and its last bits are the library's; see tests/rope_oracle.py)."""
import os
import sys

import numpy as np
import torch
import transformers

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import rope_oracle as ro  # noqa: E402

LENS = [1, 2, 15, 16, 17, 63, 64, 65, 129, 512]
CASES = {
    # name: (shape, pooling, seed, sequence lengths)
    "tiny_swiglu": (ro.RopeShape(2, 128, 2, 256, vocab=500, max_pos=512, act="silu"), "mean", 11, LENS),
    "tiny_geglu": (ro.RopeShape(2, 128, 4, 384, vocab=500, max_pos=512, act="gelu", theta=10000.0), "cls", 12, LENS),
    "nomic_like": (ro.RopeShape(12, 384, 6, 1536, vocab=1000, max_pos=512, act="silu"), "mean", 13, LENS),
}


def hf_model(shape: ro.RopeShape, w: dict):
    cfg = transformers.NomicBertConfig(
        vocab_size=shape.vocab, hidden_size=shape.hidden, num_hidden_layers=shape.layers,
        num_attention_heads=shape.heads, intermediate_size=shape.intermediate, hidden_act=shape.act,
        max_position_embeddings=shape.max_pos, type_vocab_size=shape.type_vocab, layer_norm_eps=shape.eps,
        rope_parameters={"rope_type": "default", "rope_theta": shape.theta})
    cfg._attn_implementation = "eager"
    model = transformers.NomicBertModel(cfg, add_pooling_layer=False) if "add_pooling_layer" in \
        transformers.NomicBertModel.__init__.__code__.co_varnames else transformers.NomicBertModel(cfg)
    state = {k: torch.from_numpy(v) for k, v in w.items()}
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected, unexpected
    assert all("pooler" in k for k in missing), missing  # every encoder tensor came from the seeded weights
    return model.double().eval()


def main():
    for name, (shape, pooling, seed, lens) in CASES.items():
        w = ro.random_weights(shape, seed)
        model = hf_model(shape, w)
        rng = np.random.default_rng(seed + 1000)
        seqs = [rng.integers(0, shape.vocab, size=n).astype(np.int32) for n in lens]
        want = np.zeros((len(seqs), shape.hidden), np.float64)
        with torch.no_grad():
            for i, ids in enumerate(seqs):
                h = model(input_ids=torch.from_numpy(ids.astype(np.int64))[None]).last_hidden_state[0].numpy()
                e = h[0] if pooling == "cls" else h.sum(axis=0) / max(float(len(ids)), 1e-9)
                want[i] = e / max(float(np.sqrt((e * e).sum())), 1e-12)
        off = np.zeros(len(seqs) + 1, np.int32)
        off[1:] = np.cumsum(lens)
        half = shape.hidden // shape.heads // 2
        with torch.no_grad():
            cos, sin = model.rotary_emb(torch.zeros(1, 1, dtype=torch.float32), torch.arange(max(lens))[None])
        cos, sin = cos[0, :, :half].numpy(), sin[0, :, :half].numpy()
        assert cos.dtype == np.float32
        path = os.path.join(HERE, f"rope_{name}.npz")
        np.savez_compressed(
            path, ids=np.concatenate(seqs), offsets=off, want=want, seed=seed, pooling=pooling, act=shape.act,
            theta=shape.theta, rope_cos=cos, rope_sin=sin, shape=np.array([shape.layers, shape.hidden, shape.heads, shape.intermediate, shape.vocab,
                                               shape.max_pos, shape.type_vocab]), eps=shape.eps,
            versions=f"transformers {transformers.__version__}, torch {torch.__version__}, numpy {np.__version__}")
        for what, table in (("transformers' f32 table", (cos, sin)), ("exact table", None)):
            got = ro.sentence_embeddings(w, shape, seqs, pooling, True, table=table)
            print(f"{name}: oracle with {what} vs transformers max-abs {np.max(np.abs(got - want)):.3e}")
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
