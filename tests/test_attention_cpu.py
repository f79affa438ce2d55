"""The inputs of test_attention_gpu.py, checked on the CPU with the oracles alone: for every exposing model of
attention_case.py (attention_case.PAIRS: five states at head sizes 64 and 32, none and causal at 128), every length it is
used at and every catalogue mistake that applies there,
  (a) sensitivity: in each 16-query tile the mistake touches, at least one exposed row moves by more than
      2 x test_encoder_gpu.TOL[precision] — in the absolute deviation or in |1 - cos| — for all three precisions, so the GPU
      suite fails on a kernel that makes the mistake;
  (b) noise: the oracle run on f16 operands, the probabilities included, stays within TOL["f16"] / 2 of the f64 rows, so
      the GPU suite can pass on a kernel that makes none.
Both are conditions on the inputs (weights, ids, lengths), not measurements of the engine. The margin of every case is
printed: the factor by which the least moved touched tile exceeds 2 x TOL, and the noise as a fraction of TOL / 2.

The catalogue itself says where a mistake applies (attention_case.faults): where it changes a logit that can matter and
leaves every query a key; zero keys behind the end only where a kernel would admit at least PHANTOM_MIN of them."""
import numpy as np
import pytest

import attention_case as ac
from test_encoder_gpu import TOL

# the loosest bar of the three precisions decides "for all three precisions"
COS_BAR = 2 * max(t[0] for t in TOL.values())
ABS_BAR = 2 * max(t[1] for t in TOL.values())
NOISE_COS, NOISE_ABS = TOL["f16"][0] / 2, TOL["f16"][1] / 2


def all_cases(state, dh):
    """The union of the f16 and the f32 / f16x3 cases of a model, in order."""
    seen, out = set(), []
    for precision in ("f16", "f32"):
        for case in ac.cases(state, dh, precision):
            if case not in seen:
                seen.add(case)
                out.append(case)
    return out


def margin(m, S, param, bias, tiles):
    """The least, over the touched 16-query tiles, of the largest factor by which a row of the tile exceeds 2 x TOL."""
    moved = ac.unit(m.hidden(ac.sequence(S), param, bias=bias))
    dcos, dabs = ac.deviation(moved, m.rows(S, param))
    assert np.isfinite(moved).all()
    factor = np.maximum(dcos / COS_BAR, dabs / ABS_BAR)
    return min(float(factor[16 * t:16 * t + 16].max()) for t in tiles)


@pytest.mark.parametrize("state, dh", ac.PAIRS)
def test_every_mistake_shows_and_f16_noise_does_not(state, dh):
    m = ac.model(state, dh)
    failures = []
    for param, S in all_cases(state, dh):
        dcos, dabs = ac.deviation(ac.f16_rows(m, S, param), m.rows(S, param))
        noise = max(float(dcos.max()) / NOISE_COS, float(dabs.max()) / NOISE_ABS)
        line = f"{m.name} param {param} S {S}: f16 noise {noise:.2f} of TOL/2;"
        if not noise < 1.0:
            failures.append((param, S, "noise", noise))
        for name, bias, tiles in ac.faults(m, S, param):
            f = margin(m, S, param, bias, tiles)
            line += f" {name} {f:.1f}"
            if not f > 1.0:
                failures.append((param, S, name, f))
        print(line)
    assert not failures, failures
