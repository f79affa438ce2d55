"""TEST INFRASTRUCTURE shared by test_search_layouts_cpu.py and test_search_layouts_gpu.py: corpora whose winners sit
where the selection kernels are least comfortable, and a CPU model of the routes those kernels then take.

Planting by permutation. The reference ranking of a corpus x for a query q is computed with oracle.core alone
(cosine_preprocess, dense_scores, topk over all n rows); the rows of x are then permuted so that the rank-j row sits at
a chosen position pos[j]. Scores, bounds and ties do not change, only WHERE the winners sit: all in one tile, all in
one wave's tiles, in ascending order of every wave's walk, in a few scan blocks, in the last partial tile. The expected
answer of a test is always recomputed by the oracle on the permuted corpus, never taken from the plan.

Route model. fused_merge_gather() restates, from reference scores alone, how the fused scan deals tiles to (block,
wave) lists and how many keys merge_lists_kernel's fast path gathers: more than kGatherCap sends it down the slow path
(the in-place tournament). batched_overflow_certain() says from the reference when a query of the batched search must
exceed its candidate budget. Every number below restates a constant of voitta_rag_amd/csrc and has to follow it
(test_search_layouts_cpu.py reads them back out of the sources):
  kTileRows   = 16     engine_internal.h  rows of one MFMA tile; a wave scans one tile per iteration
  kTopkSeg    = 4096   engine_internal.h  rows per block of topk_select's first level (select_from_scores_kernel)
  kQueryBlock = 16     engine_internal.h  queries per dense pass: 21 queries run as 16 + 5
  kScanBlocks = 512    engine_internal.h  grid cap of the fused scans: beyond 512 * 8 tiles the waves grid-stride
  kFusedMaxK  = 64     engine_internal.h  k <= 64 and nq <= 4 (search.hip, search_dense_block): fused scan + merge
  kBatchCand  = 1024   engine_internal.h  candidate rows per query of the batched search (batch.hip)
  kMaxCandTiles = 16384  engine_internal.h  candidate tiles of the two-stage re-score (prefilter.hip)
  kScanWaves  = 8      dense.hip          waves (= lists) per scan block; prefilter.hip's kScan16Waves is the same
  kListLen    = 64     topk_device.h      entries of a wave's / block's list
  kGatherCap  = 2048   topk.hip           keys merge_lists_kernel's fast path ranks in LDS
  kMergeMaxLists = 512 topk.hip           lists merge_lists_kernel takes (= kScanBlocks)
  PREFILTER_MIN_ROWS = 4096   prefilter.hip  prefilter_usable: `e->n_rows >= 4096`
  BATCH_MIN_ROWS     = 16384  batch.hip      batch_usable: `e->n_rows >= 16384` (and nq > kQueryBlock, dim % 128 == 0)
  LEVEL2_KEYS = 16384  topk.hip           topk_select: T2 * I2 = 1024 * 16 keys per block of the later levels
  SLAB_ROWS   = 128    batch.hip          rows whose best lower bound is one entry of T_q's selection (batch_scan_kernel:
                                          a wave's 8 tiles, rows rbi * 256 + wm * 128 ...)"""
import numpy as np

from oracle import core as ocore

kTileRows = 16
kTopkSeg = 4096
kQueryBlock = 16
kScanBlocks = 512
kFusedMaxK = 64
kBatchCand = 1024
kMaxCandTiles = 16384
kScanWaves = 8
kListLen = 64
kGatherCap = 2048
kMergeMaxLists = 512
PREFILTER_MIN_ROWS = 4096
BATCH_MIN_ROWS = 16384
LEVEL2_KEYS = 16384
SLAB_ROWS = 128

# where each mirrored `constexpr int kName = value` lives (relative to voitta_rag_amd/csrc)
CONSTANT_SOURCES = {
    "kTileRows": "engine_internal.h", "kTopkSeg": "engine_internal.h", "kQueryBlock": "engine_internal.h",
    "kScanBlocks": "engine_internal.h", "kFusedMaxK": "engine_internal.h", "kBatchCand": "engine_internal.h",
    "kMaxCandTiles": "engine_internal.h", "kScanWaves": "dense.hip", "kListLen": "topk_device.h",
    "kGatherCap": "topk.hip", "kMergeMaxLists": "topk.hip",
}

BLOCK_ROWS = kScanWaves * kTileRows  # rows a scan block reads per grid-stride iteration
N_GRID_STRIDE = 65536 + 16 * 8 * 3 + 1  # 4121 tiles on 512 blocks: slots 0..24 walk two tiles, the last tile holds one row

N_ONE_WAVE = 16 * (3 * 4096 + 8)  # 12,296 tiles: the first eight slots walk four tiles, 64 rows of one wave

# the order in which wave_offer inserts the rows of one tile for a query column: register by register (k0..k3), and
# within a register the lane groups g = 0..3 in ascending lane order; the row of (g, reg) is 4 g + reg
IN_TILE_ORDER = np.array([4 * g + reg for reg in range(4) for g in range(4)])


# ---- geometry of the fused scans (dense_scan_topk, prefilter_search) ------------------------------------------------

def scan_grid(n_rows):
    """(tiles, blocks) of the fused scans: blocks = min(ceil(tiles / kScanWaves), kScanBlocks), at least 1."""
    n_tiles = -(-n_rows // kTileRows)
    return n_tiles, max(1, min(-(-n_tiles // kScanWaves), kScanBlocks))


def row_slots(n_rows):
    """Per row: (slot, visit). slot = block * kScanWaves + wave of the list the row is offered to (tile t belongs to
    slot t % (blocks * kScanWaves): `tile = blockIdx.x * kScanWaves + wave; tile += gridDim.x * kScanWaves`); visit =
    the row's place in that wave's walk (iterations in tile order, IN_TILE_ORDER inside a tile)."""
    _, blocks = scan_grid(n_rows)
    rows = np.arange(n_rows)
    tile = rows // kTileRows
    stride = blocks * kScanWaves
    in_tile = np.empty(kTileRows, np.int64)
    in_tile[IN_TILE_ORDER] = np.arange(kTileRows)
    return tile % stride, (tile // stride) * kTileRows + in_tile[rows % kTileRows]


def row_blocks(n_rows):
    return row_slots(n_rows)[0] // kScanWaves


# ---- reference ranking and planting ---------------------------------------------------------------------------------

def reference_scores(x, q):
    """oracle scores of the queries q (nq x dim, or one vector) over the rows of x: nq x n"""
    q = np.asarray(q, np.float32).reshape(-1, x.shape[1])
    return ocore.dense_scores(ocore.cosine_preprocess(q), ocore.cosine_preprocess(x))


def reference_ranking(x, q):
    """rows of x from best to worst for the single query q, by the oracle (higher score, then lower row)"""
    rows, _ = ocore.topk(reference_scores(x, q)[0], x.shape[0])
    assert rows.shape[0] == x.shape[0], "a row without a finite score cannot be planted"
    return rows


def _default_tile(n_rows):
    _, blocks = scan_grid(n_rows)
    return (blocks // 2) * kScanWaves + 2


def positions(layout, n_rows, **geo):
    """pos[j] = the row where the rank-j row goes, for the leading ranks the layout cares about (every rank for
    ascending / descending). The positions are distinct."""
    n_tiles, blocks = scan_grid(n_rows)
    slot, visit = row_slots(n_rows)
    if layout == "one_tile":  # ranks 0..15 in one tile, 16..63 in the next three: four waves of one block
        t0 = geo.get("tile0", _default_tile(n_rows))
        assert t0 % kScanWaves <= kScanWaves - 4 and (t0 + 4) * kTileRows <= n_rows
        pos = t0 * kTileRows + np.arange(64)
    elif layout == "one_wave":  # ranks 0.. in the (full) tiles one wave walks, then the next wave of the same block
        count, s = geo.get("count", 64), geo.get("slot0", 3)
        stride, got = blocks * kScanWaves, []
        while len(got) < count:
            for t in range(s, n_tiles, stride):
                if (t + 1) * kTileRows <= n_rows:
                    got.extend(range(t * kTileRows, (t + 1) * kTileRows))
            s += 1
        pos = np.array(got[:count])
    elif layout == "ascending":  # every row beats all its wave saw before: each insert lands at 0 and shifts k - 1
        pos = np.lexsort((slot, -visit))
    elif layout == "descending":  # every row loses to all its wave saw before: the list fills once, then rejects
        pos = np.lexsort((slot, visit))
    elif layout == "hot_blocks":
        pos = _hot_blocks(n_rows, blocks, geo["h"], geo.get("k", kListLen), geo.get("gathered"))
    elif layout == "tail":  # the best rows are the last n % 16 rows, then row 0
        m = n_rows % kTileRows
        assert m > 0
        pos = np.concatenate([np.arange(n_rows - m, n_rows), [0]])
    elif layout == "packed_slabs":  # the top ranks fill s consecutive 128-row slabs, dealt round-robin
        s, total = geo["s"], geo.get("total", 4096)
        slab0, j = geo.get("slab0", 16), np.arange(total)
        assert total % s == 0 and total // s <= SLAB_ROWS and (slab0 + s) * SLAB_ROWS <= n_rows
        pos = (slab0 + j % s) * SLAB_ROWS + j // s
    else:
        raise ValueError(layout)
    pos = np.asarray(pos, np.int64)
    assert np.unique(pos).shape[0] == pos.shape[0] and pos.min() >= 0 and pos.max() < n_rows
    return pos


def _hot_blocks(n_rows, blocks, h, k, gathered=None):
    """h scan blocks each hold 64 rows (8 per wave) that outrank every row of every other block.

    What merge_lists_kernel then gathers is bounded by its two thresholds: with the k-th largest list head H and the
    best k-th list entry M it takes the keys >= max(H, M). Fewer than k lists can lie above H, and each list has at
    most k - 1 keys above M except the one that owns M, so the gather never exceeds (k - 1)^2 + 1 keys: the slow path
    (gathered > kGatherCap = 2048) exists for k >= 47 only. The layout reaches that bound: r = min(h, k) - 1 of the hot
    blocks share the first 64 r ranks round-robin (their lists' k-th entries are all about rank (k - 1) r, so
    r (k - 1) + 1 keys are gathered), the other hot blocks take the following ranks 64 at a time, so that the k-th
    largest head is no better than rank 64 r.

    gathered = G (k <= G <= (k - 1)^2 + 1, h >= k) makes the gather exactly G keys instead, for the cap itself: the
    r = k - 1 shared blocks are dealt t whole rounds and `rem` single keys with (r - 1) t + rem = G - k, then the first
    of them takes the next k - t ranks in one run. Its k-th entry M closes that run: the k keys of its list and t or
    t + 1 keys of every other list lie at or above M."""
    full = min(blocks, n_rows // BLOCK_ROWS)  # blocks whose first-iteration tiles are all full
    assert 2 <= h <= full and k >= 2
    ids = full - 1 - (np.arange(h) * full) // h  # evenly spread, the LAST full block first: with an odd number of
    # lists it is the one the tournament carries up unpaired, and here it holds rank 0
    r = min(h, k) - 1
    if gathered is not None:
        assert h >= k and k <= gathered <= r * r + 1 and r >= 2
        t, rem = divmod(gathered - k, r - 1)
        deal = [i for _ in range(t) for i in range(r)] + list(range(1, rem + 1)) + [0] * (k - t)
        room = np.full(h, kListLen)
        np.subtract.at(room, deal, 1)
        assert room.min() >= 0
        while room[:r].any():  # the rest of the shared blocks' 64 rows, round-robin, all below M
            deal += [i for i in range(r) if room[i] > 0]
            room[:r] -= room[:r] > 0
        deal = np.array(deal + [i for i in range(r, h) for _ in range(kListLen)])
        seen = np.zeros(h, np.int64)
        i = np.empty(deal.shape[0], np.int64)
        for at, b in enumerate(deal):
            i[at] = seen[b]
            seen[b] += 1
        return ids[deal] * BLOCK_ROWS + (i % kScanWaves) * kTileRows + i // kScanWaves
    j = np.arange(h * kListLen)
    shared = j < r * kListLen
    block = np.where(shared, ids[j % r], ids[np.minimum(r + (j - r * kListLen) // kListLen, h - 1)])
    i = np.where(shared, j // r, (j - r * kListLen) % kListLen)
    return block * BLOCK_ROWS + (i % kScanWaves) * kTileRows + i // kScanWaves


def tie_positions(n_rows, g, several=6):
    """g rows for exact copies of the best row: `several` inside one tile (lane groups and registers mixed), the others
    one per scan block, going round the blocks again (another wave, another row of the tile) when there are fewer
    blocks than copies."""
    _, blocks = scan_grid(n_rows)
    full = max(1, min(blocks, n_rows // BLOCK_ROWS))
    t0 = _default_tile(n_rows) if n_rows >= 8 * BLOCK_ROWS else 0
    pos = [t0 * kTileRows + r for r in (0, 1, 5, 6, 10, 15)[:min(several, g)]]
    c = 0
    while len(pos) < g:
        b, cycle = c % full, c // full
        c += 1
        if b == t0 // kScanWaves:
            continue
        pos.append(b * BLOCK_ROWS + ((3 * cycle + 1) % kScanWaves) * kTileRows + (7 + cycle) % kTileRows)
    pos = np.asarray(pos, np.int64)
    assert np.unique(pos).shape[0] == g and pos.max() < n_rows
    return pos


def permute(x, order, pos):
    """x with row order[j] moved to pos[j]; the rows the plan leaves out keep their relative order in the free places"""
    n = x.shape[0]
    out = np.empty_like(x)
    taken = np.zeros(n, bool)
    taken[pos] = True
    out[pos] = x[order[:pos.shape[0]]]
    out[~taken] = x[np.sort(order[pos.shape[0]:])]
    return out


def plant(x, q, layout, **geometry):
    """The corpus x with its rows permuted so that the rank-j row for query q sits at positions(layout)[j].
    layout "tie_group" is no permutation: g rows (geometry g) are overwritten with exact copies of the rank-0 row."""
    x = np.ascontiguousarray(x, np.float32)
    order = reference_ranking(x, q)
    if layout == "tie_group":
        out = x.copy()
        out[tie_positions(x.shape[0], geometry["g"], geometry.get("several", 6))] = x[order[0]]
        return out
    return permute(x, order, positions(layout, x.shape[0], **geometry))


# ---- route model ----------------------------------------------------------------------------------------------------

def make_keys(scores, mask=None):
    """topk_make_key: (order-preserving f32 bits << 32) | (0xFFFFFFFF - row); 0 for -inf and for masked rows"""
    s = np.ascontiguousarray(scores, np.float32)
    u = s.view(np.uint32)
    u = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint64)
    keys = (u << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(s.shape[0], dtype=np.uint64))
    keys[s == -np.inf] = 0
    if mask is not None:
        keys[~np.asarray(mask, bool)] = 0
    return keys


def block_lists(scores, mask, k, nq_index, n_rows):
    """[blocks][k] keys: what dense_scan_topk_kernel leaves in the first k entries of each block's list (the k best
    unmasked rows among the tiles the block walks), descending, zero padded"""
    sc = np.asarray(scores, np.float32)
    sc = sc[nq_index] if sc.ndim == 2 else sc
    keys = make_keys(sc[:n_rows], None if mask is None else np.asarray(mask)[:n_rows])
    _, blocks = scan_grid(n_rows)
    block = row_blocks(n_rows)
    o = np.lexsort((~keys, block))  # by block, then by key descending
    start = np.searchsorted(block[o], np.arange(blocks))
    rank = np.arange(n_rows) - start[block[o]]
    lists = np.zeros((blocks, k), np.uint64)
    keep = rank < k
    lists[block[o][keep], rank[keep]] = keys[o][keep]
    return lists


def fused_merge_gather(scores, mask, k, nq_index, n_rows):
    """(n_lists, gathered): the lists dense_scan_topk hands to merge_lists_kernel for query nq_index and the number of
    keys its fast path gathers: those >= max(best k-th list entry, k-th largest list head that is not 0).
    gathered > kGatherCap: the kernel takes the slow path."""
    lists = block_lists(scores, mask, k, nq_index, n_rows)
    heads = np.sort(lists[:, 0])[::-1]
    thr = lists[:, k - 1].max()
    if heads.shape[0] >= k and heads[k - 1] != 0:
        thr = max(thr, heads[k - 1])
    return lists.shape[0], int(np.count_nonzero((lists != 0) & (lists >= thr)))


def takes_slow_path(gathered):
    return gathered > kGatherCap


def batched_candidates_certain(scores, mask, k):
    """Rows that are certainly candidates of a batched query: the unmasked rows scoring at or above the best score of
    the k-th best 128-row slab (all unmasked rows when fewer than k slabs hold one). T_q is the k-th largest of the
    slabs' best LOWER bounds, each at most its slab's best score, so T_q is at most that score, and a row's upper
    bound is at least its score."""
    sc = np.asarray(scores, np.float32).copy()
    if mask is not None:
        sc[~np.asarray(mask, bool)] = -np.inf
    pad = -sc.shape[0] % SLAB_ROWS
    best = np.sort(np.concatenate([sc, np.full(pad, -np.inf, np.float32)]).reshape(-1, SLAB_ROWS).max(1))[::-1]
    bound = best[k - 1] if best.shape[0] >= k else -np.inf
    return int(np.count_nonzero((sc >= bound) & (sc > -np.inf)))


def batched_overflow_certain(scores, mask, k):
    return batched_candidates_certain(scores, mask, k) > kBatchCand


# ---- the shared case matrix -----------------------------------------------------------------------------------------

def gaussian(n, dim, seed):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


# merge_lists_kernel cases of the fused route: (h, k, expected path). (k - 1)^2 + 1 bounds the gather (_hot_blocks):
# k = 46 is the largest k that can never leave the fast path, k = 47 the smallest that can.
# The last two put exactly kGatherCap and kGatherCap + 1 keys in the gather: the cap itself must stay fast.
MERGE_PATHS = ((64, 64, None, "slow"), (64, 47, None, "slow"), (64, 46, None, "fast"), (64, 32, None, "fast"),
               (8, 64, None, "fast"), (64, 64, kGatherCap, "fast"), (64, 64, kGatherCap + 1, "slow"))
# (rows, dim, queries, planted query): 65 lists and 512 lists (grid-stride), one query and the last of four
MERGE_SHAPES = ((8320, 16, 1, 0), (8320, 32, 4, 3), (N_GRID_STRIDE, 16, 1, 0), (N_GRID_STRIDE, 16, 4, 3))


def merge_cases(shapes=MERGE_SHAPES):
    """(name, x, q, planted query, k, expected path) for every shape x path of the matrix; x is planted for q[planted]"""
    for n, dim, nq, planted in shapes:
        base, q = gaussian(n, dim, 1000 + n + dim), gaussian(nq, dim, 2000 + n + nq)
        for h, k, gathered, path in MERGE_PATHS:
            name = f"n{n}_d{dim}_nq{nq}_h{h}_k{k}" + (f"_g{gathered}" if gathered else "")
            yield name, plant(base, q[planted], "hot_blocks", h=h, k=k, gathered=gathered), q, planted, k, path


BATCH_DIM = 128
BATCH_ROWS = 16384 + 17  # 16 m + 1
BATCH_PLANTED = 3  # near-copies of one query at the head of a packed_slabs batch


def packed_slabs_case(nq):
    """(x, q): a corpus planted packed_slabs(32) for q[0]; q[1], q[2] are q[0] plus a little noise (their rankings
    share its head), the other queries are unrelated riders"""
    x, q = gaussian(BATCH_ROWS, BATCH_DIM, 31), gaussian(nq, BATCH_DIM, 32)
    q[1:BATCH_PLANTED] = q[0] + 0.02 * gaussian(BATCH_PLANTED - 1, BATCH_DIM, 33)
    return plant(x, q[0], "packed_slabs", s=32), q
