"""Generates tests/golden/mbert_rerank_*.npz (not modernbert_*: the embedder tests take every file of that pattern
for an embedder golden): seeded one-label ModernBERT cross-encoders
(tests/modernbert_rerank_oracle.py's weights) run through transformers.ModernBertForSequenceClassification in f64 with
eager attention, each pair alone (batch of one, no padding, no attention mask: mean pooling is over the pair's tokens).
Run in the build container:  python tests/golden/make_modernbert_rerank_golden.py
The model weights are NOT stored: modernbert_rerank_oracle.random_weights regenerates them from the seed. Stored: ids,
offsets, the expected logits, the pooled final-norm rows that transformers fed its head (`pooled`: they pin the
restated head alone, free of the f32 roundings of the library's rotation and softmax), the shape, seed, pooling,
whether the checkpoint has biases, both thetas, the window (the engine's half-width), global_every, the classifier's
scale and bias (chosen here so that the logits span at least [-3, 3]) and the library versions.
Pairs are [CLS] A [SEP] B [SEP] of random ids, of 3 tokens (both sides empty), 16 and 17 (one query tile of the
attention kernels and its edge), 129, 385 (the windowed layers' streamed kernel starts at 384) and 705 (the global
layers stream beyond what they stage). The engine takes hidden sizes that are multiples of 128, so the head's H / 16
tiles always divide evenly among its four waves and no uneven case exists; the cases have H = 128 (two tiles per wave)
except one two-layer model at H = 256 (four), so that more than two tiles per wave are checked against a reference."""
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
import modernbert_rerank_oracle as mro  # noqa: E402

LENS = [3, 16, 17, 129, 385, 705]
CLS, SEP = 1, 2
CASES = {
    # name: (shape, pooling, head and norm biases, seed)
    "cls_w8": (mo.ModernShape(3, 128, 2, 256, max_pos=1024, window=8), "cls", True, 71),
    "mean_w8": (mo.ModernShape(3, 128, 2, 256, max_pos=1024, window=8), "mean", False, 72),
    "cls_w64": (mo.ModernShape(4, 128, 4, 384, max_pos=1024, window=64, global_every=3), "cls", False, 73),
    "mean_w64": (mo.ModernShape(4, 128, 4, 384, max_pos=1024, window=64, global_every=3), "mean", True, 74),
    # two layers at H = 256: four 16-unit tiles per wave of the head kernel, where the others have two
    "mean_h256": (mo.ModernShape(2, 256, 4, 256, max_pos=1024, window=8), "mean", True, 75),
}


def hf_model(shape: mo.ModernShape, w: dict, pooling: str, biases: bool):
    cfg = transformers.ModernBertConfig(
        vocab_size=shape.vocab, hidden_size=shape.hidden, num_hidden_layers=shape.layers,
        num_attention_heads=shape.heads, intermediate_size=shape.intermediate, hidden_activation="gelu",
        max_position_embeddings=shape.max_pos, norm_eps=shape.eps, norm_bias=biases, attention_bias=False, mlp_bias=False,
        local_attention=2 * shape.window, global_attn_every_n_layers=shape.global_every, pad_token_id=0, bos_token_id=1,
        eos_token_id=2, cls_token_id=1, sep_token_id=2, num_labels=1, classifier_pooling=pooling, classifier_bias=biases,
        classifier_activation="gelu", classifier_dropout=0.0,
        rope_parameters={"full_attention": {"rope_type": "default", "rope_theta": shape.theta},
                         "sliding_attention": {"rope_type": "default", "rope_theta": shape.theta_local}})
    cfg._attn_implementation = "eager"
    model = transformers.ModernBertForSequenceClassification(cfg)
    state = {(k if k.startswith(("head.", "classifier.")) else "model." + k): torch.from_numpy(v) for k, v in w.items()}
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected and not missing, (missing, unexpected)  # every tensor came from the seeded weights
    return model.double().eval()


def run(model, seqs):
    """(logits [n], pooled rows [n, H]) of every sequence alone."""
    rows = []
    hook = model.head.register_forward_hook(lambda _m, args, _out: rows.append(args[0][0].numpy().copy()))
    with torch.no_grad():
        out = np.array([float(model(input_ids=torch.from_numpy(ids.astype(np.int64))[None]).logits[0, 0]) for ids in seqs])
    hook.remove()
    return out, np.stack(rows)


def pairs(rng, vocab):
    seqs = []
    for n in LENS:
        a = int(rng.integers(0, n - 2)) if n > 3 else 0  # tokens of A; B has the rest
        ids = rng.integers(3, vocab, size=n).astype(np.int32)
        ids[0], ids[1 + a], ids[-1] = CLS, SEP, SEP
        seqs.append(ids)
    return seqs


def main():
    for name in sys.argv[1:] or list(CASES):  # (names on the command line: only those files)
        shape, pooling, biases, seed = CASES[name]
        rng = np.random.default_rng(seed + 1000)
        seqs = pairs(rng, shape.vocab)
        base, _ = run(hf_model(shape, mro.random_weights(shape, seed, biases), pooling, biases), seqs)
        spread = base.max() - base.min()
        cls_scale = float(np.float32(8.0 / spread))
        cls_bias = float(np.float32(-cls_scale * (base.max() + base.min()) / 2))
        w = mro.random_weights(shape, seed, biases, cls_scale, cls_bias)
        logits, pooled = run(hf_model(shape, w, pooling, biases), seqs)
        assert logits.min() <= -3 and logits.max() >= 3, (logits.min(), logits.max())
        off = np.zeros(len(seqs) + 1, np.int32)
        off[1:] = np.cumsum(LENS)
        ids = np.concatenate(seqs)
        path = os.path.join(HERE, f"mbert_rerank_{name}.npz")
        np.savez_compressed(
            path, ids=ids, offsets=off, logits=logits, pooled=pooled, seed=seed, pooling=pooling, biases=biases,
            theta=shape.theta, theta_local=shape.theta_local, window=shape.window, global_every=shape.global_every,
            cls_scale=cls_scale, cls_bias=cls_bias, eps=shape.eps,
            shape=np.array([shape.layers, shape.hidden, shape.heads, shape.intermediate, shape.vocab, shape.max_pos]),
            versions=f"transformers {transformers.__version__}, torch {torch.__version__}, numpy {np.__version__}")
        d_head = np.abs(mro.head(w, pooled, shape.eps) - logits).max()
        d_all = np.abs(mro.logits(w, shape, ids, off, pooling) - logits).max()
        print(f"{name}: logits {logits.min():.3f} .. {logits.max():.3f}, scale {cls_scale:.3f}; restated head on "
              f"transformers' pooled rows max-abs {d_head:.3e}; whole oracle (exact tables, f64 throughout) {d_all:.3e}")
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
