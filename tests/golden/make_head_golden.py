"""Generates tests/golden/head_*.npz: every case of tests/head_oracle.py's CASES with its head built from
torch.nn.Linear / Tanh / LayerNorm in f64 (then torch.nn.functional.normalize and the column cut, as sentence-transformers'
Normalize module and truncate_dim do them), applied to seeded rows of order 1. The head weights are NOT stored:
head_oracle.head_weights regenerates them from the case's seed. Stored: the input rows, the expected output, the library
versions. These files pin the NumPy oracle (head_oracle.apply_head) to torch's modules.
Run in the build container:  python tests/golden/make_head_golden.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import head_oracle as ho  # noqa: E402


def torch_head(stages):
    mods = []
    for st in stages:
        if st["kind"] == "dense":
            n_out, n_in = st["weight"].shape
            lin = torch.nn.Linear(n_in, n_out, bias=st["bias"] is not None, dtype=torch.float64)
            with torch.no_grad():
                lin.weight.copy_(torch.from_numpy(st["weight"].astype(np.float64)))
                if st["bias"] is not None:
                    lin.bias.copy_(torch.from_numpy(st["bias"].astype(np.float64)))
            mods += [lin, torch.nn.Tanh() if st["activation"] == "tanh" else torch.nn.Identity()]
        else:
            ln = torch.nn.LayerNorm(st["weight"].shape[0], eps=st["eps"], dtype=torch.float64)
            with torch.no_grad():
                ln.weight.copy_(torch.from_numpy(st["weight"].astype(np.float64)))
                ln.bias.copy_(torch.from_numpy(st["bias"].astype(np.float64)))
            mods.append(ln)
    return torch.nn.Sequential(*mods).eval()


if __name__ == "__main__":
    for name, case in ho.CASES.items():
        stages = ho.head_weights(case)
        rng = np.random.default_rng(case.seed + 5000)
        rows = rng.normal(0.0, 1.0, (4 if case.shape.hidden > 256 else 9, case.shape.hidden))
        with torch.no_grad():
            y = torch_head(stages)(torch.from_numpy(rows))
            if case.normalize:
                y = torch.nn.functional.normalize(y, p=2, dim=1)
            if case.truncate:
                y = y[..., :case.truncate]
        want = y.numpy()
        got = ho.apply_head(rows, stages, case.normalize, case.truncate)
        print(f"{name}: oracle vs torch max-abs {np.max(np.abs(got - want)):.3e}")
        path = os.path.join(HERE, f"head_{name}.npz")
        np.savez_compressed(path, rows=rows, want=want, versions=f"torch {torch.__version__}, numpy {np.__version__}")
        print("wrote", path, os.path.getsize(path), "bytes")
