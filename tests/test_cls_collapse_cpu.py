"""The inputs of test_cls_collapse_gpu.py, checked on the CPU with the oracles alone (cls_collapse_case.py):
  (a) the restatement of the collapsed last layer equals oracle.bert.sentence_embeddings in f64 to 1e-12 on the ladder;
  (b) sensitivity: every planted mistake moves the [CLS] embedding of every sequence it touches by more than
      2 x test_encoder_gpu.TOL["f16"], in the absolute deviation or in |1 - cos|, so the GPU suite fails on a kernel that
      makes it (cls_collapse_case.NOT_COVERED lists the pairs that arithmetic makes invisible);
  (c) noise: the restatement on f16 operands alone stays within half of TOL["f16"], so the GPU suite can pass on a kernel
      that makes none.
All three are conditions on the inputs, not measurements of the engine; every margin is printed."""
import numpy as np
import pytest

import cls_collapse_case as cc
from rope_oracle import f16_operand
from test_encoder_gpu import TOL

COS_BAR, ABS_BAR = 2 * TOL["f16"][0], 2 * TOL["f16"][1]
NOISE_COS, NOISE_ABS = TOL["f16"][0] / 2, TOL["f16"][1] / 2


@pytest.mark.parametrize("dh", cc.HEAD_SIZES)
def test_restatement_equals_the_oracle(dh):
    m = cc.model(dh)
    seqs = [cc.sequence(S) for S in cc.LADDER]
    want = m.oracle_rows(seqs)
    got = np.stack([m.cls_row(s) for s in seqs])
    worst = float(np.max(np.abs(got - want)))
    print(f"{m.name}: restatement against oracle.bert, worst abs diff {worst:.2e}")
    assert worst < 1e-12


@pytest.mark.parametrize("dh", cc.HEAD_SIZES)
def test_every_mistake_shows_and_f16_noise_does_not(dh):
    m = cc.model(dh)
    other = cc.pre_rows(m.w, m.shape, cc.sequence(40, 99))  # the sequence whose first key a wrong bound admits
    failures = []
    for S in cc.LADDER:
        seq = cc.sequence(S)
        right = m.cls_row(seq)
        dcos, dabs = cc.deviation(m.cls_row(seq, operand=f16_operand), right)
        noise = max(float(dcos) / NOISE_COS, float(dabs) / NOISE_ABS)
        line = f"{m.name} S {S}: f16 noise {noise:.2f} of TOL/2;"
        if not noise < 1.0:
            failures.append((S, "noise", noise))
        for name, (hooks, touches) in cc.MISTAKES.items():
            if not touches(S):
                continue
            wrong = m.cls_row(seq, phantom=other) if hooks == "phantom" else m.cls_row(seq, hooks=hooks)
            assert np.isfinite(wrong).all()
            dcos, dabs = cc.deviation(wrong, right)
            f = max(float(dcos) / COS_BAR, float(dabs) / ABS_BAR)
            covered = (name, S) not in cc.NOT_COVERED.get(dh, ())
            line += f" {name} {f:.1f}" + ("" if covered else " (NOT COVERED)")
            if covered and not f > 1.0:
                failures.append((S, name, round(f, 2)))
        print(line)
    assert not failures, failures
