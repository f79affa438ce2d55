"""Generates tests/golden/modernbert_*.npz: seeded pre-norm, sliding-window encoders (tests/modernbert_oracle.py's
weights) run through transformers.ModernBertModel in f64 with eager attention, then pooled and normalised as
sentence-transformers does. Each sequence runs alone (batch of one, no padding).
Run in the build container:  python tests/golden/make_modernbert_golden.py
The model weights are NOT stored: modernbert_oracle.random_weights regenerates them from the seed. Stored: ids, offsets,
the expected embeddings, the shape, seed, both thetas, the window (the engine's half-width = local_attention // 2),
global_every, pooling, the library versions, and the f32 cos/sin tables of both layer kinds that transformers rotated
with (rope_cos / rope_sin: the global layers', rope_cos_local / rope_sin_local: the windowed layers', [rows, d_h/2]).
The tables hold the first 512 positions: all of a short case, and for the long cases (8192 positions of random-looking
f32: megabytes) as much as keeps the file the size of the others — the CPU tier pins the oracle on the short cases."""
import os
import sys

import numpy as np
import torch
import transformers

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import modernbert_oracle as mo  # noqa: E402

TABLE_ROWS = 512
CASES = {
    # name: (shape, pooling, seed, sequence lengths)
    "tiny_w8": (mo.ModernShape(4, 128, 2, 256, max_pos=512, window=8), "mean", 41,
                [1, 2, 8, 9, 10, 16, 17, 18, 63, 64, 65, 129, 193, 257, 512]),
    "tiny_w64": (mo.ModernShape(3, 128, 4, 384, max_pos=512, window=64), "cls", 42,
                 [1, 64, 65, 66, 128, 129, 130, 193, 257, 512]),
    "long_d64": (mo.ModernShape(3, 128, 2, 256, max_pos=8192, window=64), "mean", 43, [1, 641, 705, 1025, 2049, 8192]),
    "long_d32": (mo.ModernShape(3, 128, 4, 256, max_pos=8192, window=64), "mean", 44, [1, 1281, 2049, 8192]),
}


def hf_model(shape: mo.ModernShape, w: dict):
    cfg = transformers.ModernBertConfig(
        vocab_size=shape.vocab, hidden_size=shape.hidden, num_hidden_layers=shape.layers,
        num_attention_heads=shape.heads, intermediate_size=shape.intermediate, hidden_activation="gelu",
        max_position_embeddings=shape.max_pos, norm_eps=shape.eps, norm_bias=False, attention_bias=False, mlp_bias=False,
        local_attention=2 * shape.window, global_attn_every_n_layers=shape.global_every, pad_token_id=0, bos_token_id=1,
        eos_token_id=2, cls_token_id=1, sep_token_id=2,
        rope_parameters={"full_attention": {"rope_type": "default", "rope_theta": shape.theta},
                         "sliding_attention": {"rope_type": "default", "rope_theta": shape.theta_local}})
    cfg._attn_implementation = "eager"
    assert cfg.layer_types == ["full_attention" if mo.is_global(shape, i) else "sliding_attention"
                               for i in range(shape.layers)]
    model = transformers.ModernBertModel(cfg)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    assert not unexpected and not missing, (missing, unexpected)  # every tensor came from the seeded weights
    return model.double().eval()


def main():
    for name, (shape, pooling, seed, lens) in CASES.items():
        w = mo.random_weights(shape, seed)
        model = hf_model(shape, w)
        rng = np.random.default_rng(seed + 1000)
        seqs = [rng.integers(0, shape.vocab, size=n).astype(np.int32) for n in lens]
        want = np.zeros((len(seqs), shape.hidden), np.float64)
        with torch.no_grad():
            for i, ids in enumerate(seqs):
                h = model(input_ids=torch.from_numpy(ids.astype(np.int64))[None]).last_hidden_state[0].numpy()
                want[i] = mo.pool(h, pooling)
        off = np.zeros(len(seqs) + 1, np.int32)
        off[1:] = np.cumsum(lens)
        half = shape.hidden // shape.heads // 2
        tables = {}
        with torch.no_grad():
            for kind in ("full_attention", "sliding_attention"):
                cos, sin = model.rotary_emb(torch.zeros(1, 1, dtype=torch.float32), torch.arange(min(max(lens), TABLE_ROWS))[None],
                                            kind)
                tables[kind] = (cos[0, :, :half].numpy(), sin[0, :, :half].numpy())
                assert tables[kind][0].dtype == np.float32
        path = os.path.join(HERE, f"modernbert_{name}.npz")
        np.savez_compressed(
            path, ids=np.concatenate(seqs), offsets=off, want=want, seed=seed, pooling=pooling, theta=shape.theta,
            theta_local=shape.theta_local, window=shape.window, global_every=shape.global_every,
            rope_cos=tables["full_attention"][0], rope_sin=tables["full_attention"][1],
            rope_cos_local=tables["sliding_attention"][0], rope_sin_local=tables["sliding_attention"][1],
            shape=np.array([shape.layers, shape.hidden, shape.heads, shape.intermediate, shape.vocab, shape.max_pos]),
            eps=shape.eps,
            versions=f"transformers {transformers.__version__}, torch {torch.__version__}, numpy {np.__version__}")
        short = [s for s in seqs if len(s) <= TABLE_ROWS]
        rows = [i for i, s in enumerate(seqs) if len(s) <= TABLE_ROWS]
        recorded = (tables["full_attention"], tables["sliding_attention"])
        for what, tab, f32 in (("transformers' f32 tables and its f32 rotation and softmax", recorded, True),
                               ("transformers' f32 tables", recorded, False), ("exact tables", None, False)):
            got = mo.sentence_embeddings(w, shape, short, pooling, True, tables=tab, library_f32=f32)
            print(f"{name}: oracle with {what} vs transformers max-abs {np.max(np.abs(got - want[rows])):.3e}")
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
