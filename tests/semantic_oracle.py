"""The semantic chunking rule (vr_encode_semantic) in NumPy, step by step as include/voitta_engine.h states
it. Everything is per sequence. ``hidden`` is the f64 last_hidden_state [S, H] of an existing oracle (oracle.bert,
tests/qwen2_oracle.py, ...); ``units`` a list of (begin, end) token ranges, in order and never overlapping.

``decide`` takes the distances in ANY float dtype and compares them as they are: fed the device's own f32 ``gap_dist`` it
replays the device's decisions exactly (f32 compares, integer B) — no tolerance is involved."""
from dataclasses import dataclass

import numpy as np


@dataclass(frozen=True)
class Params:
    buffer: int = 1
    break_permille: int = 50
    min_distance: float = 0.0
    min_tokens: int = 0
    max_tokens: int = 2**31 - 1

    def kwargs(self) -> dict:
        return dict(buffer=self.buffer, break_permille=self.break_permille, min_distance=self.min_distance,
                    min_tokens=self.min_tokens, max_tokens=self.max_tokens)


def unit_sums(hidden: np.ndarray, units) -> np.ndarray:
    """S_r [m, H]: the sum of the unit's token rows."""
    return np.stack([hidden[b:e].sum(axis=0) for b, e in units]) if len(units) else np.zeros((0, hidden.shape[1]))


def combined(S: np.ndarray, buffer: int) -> np.ndarray:
    """C_r = sum of S_j over max(0, r - buffer) .. min(m - 1, r + buffer)."""
    m = len(S)
    return np.stack([S[max(0, r - buffer):min(m - 1, r + buffer) + 1].sum(axis=0) for r in range(m)]) if m else S


def distances(S: np.ndarray, buffer: int) -> np.ndarray:
    """d_r, r = 0 .. m - 2."""
    C = combined(S, buffer)
    d = np.zeros(max(len(S) - 1, 0))
    for r in range(len(d)):
        norms = np.sqrt((C[r] * C[r]).sum()) * np.sqrt((C[r + 1] * C[r + 1]).sum())
        d[r] = 1.0 - (C[r] * C[r + 1]).sum() / max(norms, 1e-12)
    return d


def break_budget(gaps: int, break_permille: int) -> int:
    """B = ceil(break_permille * gaps / 1000), in integers."""
    return (int(break_permille) * int(gaps) + 999) // 1000


def ranks(d: np.ndarray) -> np.ndarray:
    """rank(r): the gaps with a larger distance, or an equal one at a lower index."""
    r = np.arange(len(d))
    return ((d[None, :] > d[:, None]) | ((d[None, :] == d[:, None]) & (r[None, :] < r[:, None]))).sum(axis=1)


def candidates(d: np.ndarray, p: Params) -> np.ndarray:
    floor = d.dtype.type(p.min_distance) if len(d) else p.min_distance
    return (ranks(d) < break_budget(len(d), p.break_permille)) & (d >= floor)


def walk(cand: np.ndarray, n, p: Params) -> np.ndarray:
    """unit_start [m] from the candidate flags [m - 1] and the units' token counts."""
    m = len(n)
    start = np.zeros(m, np.int32)
    if m == 0:
        return start
    start[0] = 1
    acc = int(n[0])
    for r in range(m - 1):
        nxt = int(n[r + 1])
        close = (bool(cand[r]) and acc >= p.min_tokens) or acc + nxt > p.max_tokens
        start[r + 1] = int(close)
        acc = nxt if close else acc + nxt
    return start


def decide(d: np.ndarray, n, p: Params) -> np.ndarray:
    """unit_start of one sequence from its distances (m - 1 of them, compared in their own dtype) and token counts."""
    return walk(candidates(np.asarray(d), p), n, p)


def chunk_means(S: np.ndarray, n, start: np.ndarray) -> np.ndarray:
    """(sum of S_r over a chunk's units) / (sum of n_r), one row per chunk; un-normalised."""
    first = np.flatnonzero(start)
    last = np.append(first[1:], len(start))
    n = np.asarray(n, np.float64)
    return np.stack([S[a:b].sum(axis=0) / n[a:b].sum() for a, b in zip(first, last)]) if len(first) else S[:0]


def normalized(rows: np.ndarray) -> np.ndarray:
    return rows / np.maximum(np.sqrt((rows * rows).sum(axis=1, keepdims=True)), 1e-12)


def sequence(hidden: np.ndarray, units, p: Params):
    """One sequence through the whole rule: (d [m - 1] f64, unit_start [m], un-normalised chunk means)."""
    S = unit_sums(hidden, units)
    n = [e - b for b, e in units]
    d = distances(S, p.buffer)
    start = decide(d, n, p)
    return d, start, chunk_means(S, n, start)


def margins(d: np.ndarray, p: Params):
    """How far the candidate decisions of one sequence are from flipping: (the gap between the B-th and the (B + 1)-th
    largest distance — inf when B is 0 or every gap is inside the budget — and the least |d_r - min_distance| over the
    gaps inside the budget)."""
    B = break_budget(len(d), p.break_permille)
    order = np.sort(d)[::-1]
    rank_margin = float(order[B - 1] - order[B]) if 0 < B < len(d) else float("inf")
    inside = order[:B]
    floor_margin = float(np.min(np.abs(inside - p.min_distance))) if len(inside) else float("inf")
    return rank_margin, floor_margin


def replay(gap_dist: np.ndarray, unit_off, unit_tok, p: Params) -> np.ndarray:
    """unit_start of a whole call from the DEVICE's gap_dist (one f32 per unit, the last of a sequence unused)."""
    gap_dist = np.asarray(gap_dist)
    out = np.zeros(len(gap_dist), np.int32)
    for i in range(len(unit_off) - 1):
        lo, hi = int(unit_off[i]), int(unit_off[i + 1])
        if hi > lo:
            tok = np.asarray(unit_tok[lo:hi])
            out[lo:hi] = decide(gap_dist[lo:hi - 1], tok[:, 1] - tok[:, 0], p)
    return out
