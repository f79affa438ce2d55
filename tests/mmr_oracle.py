"""TEST INFRASTRUCTURE — NumPy restatement of the MMR selection of vr_mmr_select:
  sim(i, j) : the f32 dense score of stored row c_i against stored row c_j (oracle.core.dense_scores: the k-ordered
              fmaf chain of a search score, on the rows as stored, i.e. after the cosine preprocessing)
  step 1    : the largest (1 - d) * rel_i
  step t    : the largest (1 - d) * rel_i - d * (double) m_i over the unselected, m_i = the f32 max of sim(i, s) over
              the picks s so far
f64 arithmetic, one rounding per operation; ties go to the lower position (-0.0 == +0.0); min(limit, K) picks."""
from __future__ import annotations

import numpy as np

from oracle import core as ocore


def gram(x_hat: np.ndarray) -> np.ndarray:
    """K x K f32 similarities of stored (already preprocessed) rows."""
    x_hat = np.ascontiguousarray(x_hat, np.float32)
    if x_hat.shape[0] == 0:
        return np.zeros((0, 0), np.float32)
    return ocore.dense_scores(x_hat, x_hat)


def select(sim: np.ndarray, relevance, diversity: float, limit: int) -> list[int]:
    """Positions in selection order, given the K x K f32 similarities and the f64 relevance."""
    rel = np.asarray(relevance, np.float64)
    k = rel.size
    d = np.float64(diversity)
    keep = np.float64(1.0) - d
    a = keep * rel
    m = np.full(k, -np.inf, np.float32)
    open_ = np.ones(k, bool)
    out: list[int] = []
    for step in range(min(int(limit), k)):
        v = a if step == 0 else a - d * m.astype(np.float64)
        best = v[open_].max()
        pick = int(np.flatnonzero(open_ & (v == best))[0])  # (mmr desc, position asc)
        out.append(pick)
        open_[pick] = False
        m = np.maximum(m, sim[pick])
    return out


def select_rows(stored: np.ndarray, rows, relevance, diversity: float, limit: int) -> list[int]:
    """select() with the similarities of stored[rows] (stored: every row as the engine stores it)."""
    rows = np.asarray(rows, np.int64)
    return select(gram(stored[rows]), relevance, diversity, limit)
