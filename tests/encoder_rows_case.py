"""TEST INFRASTRUCTURE shared by test_encoder_rows_cpu.py and test_encoder_rows_gpu.py: batches in which EVERY row
of every GEMM output reaches a returned embedding, at the token counts where the f16 path changes kernel.

A pooled embedding hides rows: CLS pooling shows one row per sequence, mean pooling divides a wrong row by the
sequence length. A sequence of ONE token is its own [CLS] row and its own mean, so a batch of T one-token sequences
returns all T rows of the last layer, each fed by exactly one row of every GEMM before it. The batches cycle through
a few distinct sequences: the f64 oracle is computed for those only, and every repeat must also carry the same BITS
as the first occurrence, wherever its rows sit in a tile."""
import numpy as np

FIXED_EDGES = (16, 17, 64, 65, 128, 129, 255, 256, 257, 384, 385, 1024, 1025)
RAGGED_LENS = (1, 2, 17, 63, 64, 65, 127, 128, 129)


def mid_threshold(N, n_cu):
    """The last M for which launch_gemm_f16x3 sends a product with N output features to gemm_f16_mid_kernel:
    mid_usable asks 4 * ceil(M / GBM) * ceil(N / GBN) <= n_cu with GBM = GBN = 256 and n_cu rounded down to a
    multiple of 8."""
    return (n_cu // 8 * 8 // 4 // -(-N // 256)) * 256


def route_edges(H, I, n_cu):
    """Sorted token counts on both sides of every point where the f16 forward pass of a model of width H and FFN
    width I changes kernel or epilogue family on a device with n_cu compute units. Each number restates a constant
    of csrc/encoder.hip and has to follow it:
      16 / 17          skinny_ln_supported (M <= 16): fold_ln, gemm_f16_skinny_ln_kernel
      64 / 65          kSkinnyM = 64: one / two row blocks of the skinny kernels
      128 / 129        two / three row blocks; kMidM = 128 (one row panel of gemm_f16_mid_kernel, one row more)
      255 / 256 / 257  4 * kSkinnyM = 256: the last skinny M; mid_usable refuses M <= 256; fold_big and the f16
                       residual stream (res16) start at T > 256; GBM = 256 is the ping-pong kernel's row tile and
                       the f16x3 route's switch from the 128-row to the 256-row kernel (M >= GBM)
      384 / 385        a whole number of kMidM panels and one row more (3 and 4 panels: launch_mid pads the grid to
                       8 row panels, `panel >= tiles_m` retires the rest)
      1024 / 1025      8 panels exactly (no padding) and 9 (padded to 16); the last graph-replayed T and the first
                       that is not (forward_all: T <= 1024)
      thr / thr + 1    per N in (H, 3H, I), thr = mid_threshold(N, n_cu): the last M on gemm_f16_mid_kernel and the
                       first on gemm_f16_pp_kernel (mid_usable). thr is a multiple of GBM, so thr rows are whole
                       tiles of both kernels and thr + 1 leaves a one-row partial tile. (thr = 0, fewer than four CUs
                       per column tile: that product never takes the mid kernel and adds no edge.)"""
    edges = set(FIXED_EDGES)
    for N in (H, 3 * H, I):
        thr = mid_threshold(N, n_cu)
        if thr > 0:
            edges.update((thr, thr + 1))
    return sorted(edges)


class _AsIs(np.ndarray):
    """An array whose astype to its own dtype is itself. oracle.bert.encode_one casts every weight matrix once per
    sequence (w[k].astype(dtype)): a copy of 100 ms per sequence at H = 1024 when the weights are f64 already."""

    def astype(self, dtype, *args, **kwargs):
        return self if np.dtype(dtype) == self.dtype else np.asarray(self).astype(dtype, *args, **kwargs)


def f64_weights(w):
    """The weights cast to f64 once, for the f64 oracle; same arithmetic and bits as passing the f32 weights."""
    return {k: v.astype(np.float64).view(_AsIs) for k, v in w.items()}


def _distinct_ids(k, vocab, seed):
    return np.random.default_rng(seed).permutation(vocab)[:k].astype(np.int32)


def one_token_batch(T, k=23, vocab=64):
    """T one-token sequences cycling through k distinct ids. k = 23 is prime, so over a few tiles each id visits
    every row position of a 128- or 256-row tile."""
    ids = _distinct_ids(k, vocab, 101)
    which = np.arange(T) % k
    return [ids[j:j + 1] for j in which], which


def three_token_batch(n_seq, k=23, vocab=64):
    """n_seq three-token sequences cycling through k distinct ones. With CLS pooling n_seq * (4H + I) <= 3 n_seq * 3H
    holds for I = 4H, so the last layer runs its [CLS]-only tail on M = n_seq gathered rows (body: M = 3 n_seq)."""
    base = np.random.default_rng(102).integers(0, vocab, size=(k, 3)).astype(np.int32)
    which = np.arange(n_seq) % k
    return [base[j] for j in which], which


def ragged_batch(T, k=23, vocab=64):
    """Exactly T tokens of real attention: k distinct sequences, lengths cycling through RAGGED_LENS (both sides of
    the 64-key tile and of the 128-row panel), repeated in order while the next one still fits, then closed with one
    further distinct sequence (index k) of the exact remaining length, if any. Repeats of one sequence start at
    different offsets inside the 128- and 256-row tiles."""
    rng = np.random.default_rng(103)
    base = [rng.integers(0, vocab, size=RAGGED_LENS[j % len(RAGGED_LENS)]).astype(np.int32) for j in range(k)]
    closing = rng.integers(0, vocab, size=max(RAGGED_LENS)).astype(np.int32)
    seqs, which, total, i = [], [], 0, 0
    while total + len(base[i % k]) <= T:
        seqs.append(base[i % k])
        which.append(i % k)
        total += len(base[i % k])
        i += 1
    if total < T:
        seqs.append(closing[:T - total])
        which.append(k)
    return seqs, np.asarray(which)


def distinct_of(seqs, which):
    """The distinct sequences of a batch, densely renumbered: (distinct, which') with seqs[i] == distinct[which'[i]]."""
    _, first, dense = np.unique(which, return_index=True, return_inverse=True)
    return [seqs[i] for i in first], dense


def check_rows(got, want_distinct, which, precision):
    """(1) every row of `got` within TOL[precision] (cosine and absolute, unit-length rows) of the oracle row of the
    distinct sequence it repeats; (2) all rows that repeat one sequence bit-identical to the first of them.
    Returns (worst |1 - cos|, worst abs diff) over ALL rows."""
    from test_encoder_gpu import TOL

    got = np.ascontiguousarray(got, dtype=np.float32)
    which = np.asarray(which)
    want = np.asarray(want_distinct)[which]
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.all(np.isfinite(got))
    g64 = got.astype(np.float64)
    cos = (g64 * want).sum(1) / np.linalg.norm(g64, axis=1) / np.linalg.norm(want, axis=1)
    dcos = np.abs(1.0 - cos)
    dabs = np.abs(g64 - want).max(axis=1)
    cos_tol, abs_tol = TOL[precision]
    bad = np.flatnonzero(~((dcos < cos_tol) & (dabs < abs_tol)))
    assert bad.size == 0, (f"{bad.size} of {len(got)} rows outside TOL[{precision}]: rows {bad[:16].tolist()}, "
                           f"worst |1-cos| {dcos.max():.3e}, worst abs {dabs.max():.3e}")
    _, first = np.unique(which, return_index=True)
    first_of = np.empty(int(which.max()) + 1, np.int64)
    first_of[which[first]] = first
    bits = got.view(np.uint32)
    differ = np.flatnonzero((bits != bits[first_of[which]]).any(axis=1))
    assert differ.size == 0, (f"{differ.size} of {len(got)} rows differ in bits from the first row of the same "
                              f"sequence: rows {differ[:16].tolist()}")
    return float(dcos.max()), float(dabs.max())
