// The searches of libvoitta_engine.so (include/voitta_engine.h): search lanes, the dense, sparse and hybrid searches of
// one query, of a batch under one filter and of a batch with a filter per query, and the fusion of their lists. This
// file only sequences kernels on a lane's streams and moves small results back to the host; each step that several
// searches share (two-stage settle, batched round, auxiliary-stream fork, overflow read-back, decode and fuse) is
// written once.

#include "search.h"

#include <algorithm>
#include <thread>

#include "host_parallel.h"

namespace vr {

int check_engine(vr_engine* e) {
  VR_CHECK(e != nullptr, "null engine");
  VR_HIP(hipSetDevice(e->device));
  return 0;
}

// ---- ranking keys -> rows and scores --------------------------------------------------------------------------------

int64_t decode_keys(const uint64_t* keys, int k, int64_t* rows, float* scores) {
  int64_t n = 0;
  for (int i = 0; i < k; ++i) {
    uint64_t key = keys[i];
    if (key == 0) {
      rows[i] = -1;
      scores[i] = 0.0f;
      continue;
    }
    uint32_t hi = static_cast<uint32_t>(key >> 32);
    uint32_t u = (hi & 0x80000000u) ? (hi ^ 0x80000000u) : ~hi;
    float s;
    memcpy(&s, &u, 4);
    rows[i] = static_cast<int64_t>(0xFFFFFFFFu - static_cast<uint32_t>(key & 0xFFFFFFFFu));
    scores[i] = s;
    ++n;
  }
  return n;
}

// nq lists of k keys -> nq x k rows and scores, and (counts given) how many entries each list holds
static void decode_lists(const uint64_t* keys, int nq, int k, int64_t* rows, float* scores, int32_t* counts) {
  for (int i = 0; i < nq; ++i) {
    const int64_t c = decode_keys(keys + static_cast<size_t>(i) * k, k, rows + static_cast<int64_t>(i) * k,
                                  scores + static_cast<int64_t>(i) * k);
    if (counts) counts[i] = static_cast<int32_t>(c);
  }
}

// Two lists of k keys (sparse_keys null: no sparse list) decoded and fused into at most `limit` answers
static int fuse_one(const uint64_t* dense_keys, const uint64_t* sparse_keys, int k, int limit, double sparse_weight,
                    int32_t fusion, int64_t* out_rows, double* out_scores, int32_t* out_from_dense, int32_t* out_count) {
  int64_t d_rows[kMaxK], s_rows[kMaxK];
  float d_scores[kMaxK], s_scores[kMaxK];
  const int nd = static_cast<int>(decode_keys(dense_keys, k, d_rows, d_scores));
  const int ns = sparse_keys ? static_cast<int>(decode_keys(sparse_keys, k, s_rows, s_scores)) : 0;
  if (fusion == VR_FUSION_MINMAX)
    return fuse_minmax(d_rows, d_scores, nd, s_rows, s_scores, ns, limit, sparse_weight, 1, out_rows, out_scores,
                       out_from_dense, out_count);
  return fuse_rrf(d_rows, nd, s_rows, ns, limit, sparse_weight, out_rows, out_scores, out_from_dense, out_count);
}

// ---- search lanes and the writer protocol (see vr_engine::rw) -----------------------------------------------

// the index as the master holds it right now: pointers and counts only (call with rw held)
static void lane_view(vr_engine* L, const vr_engine* m) {
  static_cast<IndexTables&>(*L) = *m;
  static_cast<IndexTotals&>(*L) = *m;
  L->profiler = m->profiler;
}

static vr_engine* lane_create(vr_engine* m) {
  vr_engine* L = new vr_engine();
  L->master = m;
  L->device = m->device;
  L->dim = m->dim;
  L->kblocks = m->kblocks;
  L->prefilter = m->prefilter;
  L->prefilter8 = m->prefilter8;
  // The auxiliary stream (the sparse leg of a hybrid search, forked beside the dense scan) gets the highest stream
  // priority: streams of different priority never share a hardware queue. With equal priorities the runtime deals its
  // 4 hardware queues round-robin over ALL streams of the process, the two streams of a lane could land on one queue,
  // and the two legs then ran one after the other: hybrid p50 0.32 ms instead of 0.26 (scripts/perf_query_tail.py;
  // GPU_MAX_HW_QUEUES=8 in the environment had the same effect, but a library cannot rely on its host's environment).
  int prio_low = 0, prio_high = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);
  bool ok = hipStreamCreateWithFlags(&L->own_stream, hipStreamNonBlocking) == hipSuccess &&
            hipStreamCreateWithPriority(&L->aux_stream, hipStreamNonBlocking, prio_high) == hipSuccess &&
            hipEventCreateWithFlags(&L->ev_fork, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&L->ev_join, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&L->ev_input, hipEventDisableTiming) == hipSuccess &&
            hipHostMalloc(&L->pinned, kPinnedBytes, hipHostMallocMapped) == hipSuccess &&
            hipHostGetDevicePointer(&L->pinned_dev, L->pinned, 0) == hipSuccess;
  if (!ok) {
    set_error("creating a search lane failed");
    L->LaneResources::release();
    delete L;
    return nullptr;
  }
  L->stream = L->own_stream;
  L->pinned_bytes = kPinnedBytes;
  L->stat_last_candidates.store(-1);
  return L;
}

int SearchLane::acquire(bool device_input) {
  {
    std::unique_lock<std::mutex> g(m->lane_mu);
    while (m->lanes_free.empty() && static_cast<int>(m->lanes_all.size()) >= m->lanes_max) m->lane_cv.wait(g);
    if (!m->lanes_free.empty()) {
      L = m->lanes_free.back();
      m->lanes_free.pop_back();
    } else {
      L = lane_create(m);
      if (!L) return -1;
      m->lanes_all.push_back(L);
    }
  }
  while (m->writers_waiting.load(std::memory_order_acquire) > 0) std::this_thread::yield();
  lock = std::shared_lock<std::shared_mutex>(m->rw);
  lane_view(L, m);
  if (device_input) {
    if (hipEventRecord(L->ev_input, m->stream) != hipSuccess || hipStreamWaitEvent(L->stream, L->ev_input, 0) != hipSuccess) {
      set_error("ordering the search behind the caller's stream failed");
      return -1;
    }
  }
  return 0;
}

SearchLane::~SearchLane() {
  if (!L) return;
  L->drain_into(*m);
  if (lock.owns_lock()) lock.unlock();
  {
    std::lock_guard<std::mutex> g(m->lane_mu);
    m->lanes_free.push_back(L);
  }
  m->lane_cv.notify_one();
}

// A side leg on a lane's auxiliary stream. mark() records the point of the main stream the leg is ordered behind,
// enter() makes the auxiliary stream wait for it and points e->stream at it, so that everything queued through `e`
// goes there; the destructor points e->stream back on every path out. join() ends the leg and orders the main stream
// behind it; a caller that waits for the auxiliary stream itself leaves the scope without it.
namespace {
struct AuxScope {
  vr_engine* e;
  hipStream_t main_stream;
  explicit AuxScope(vr_engine* lane) : e(lane), main_stream(lane->stream) {}
  ~AuxScope() { e->stream = main_stream; }
  int mark() {
    VR_HIP(hipEventRecord(e->ev_fork, main_stream));
    return 0;
  }
  int enter() {
    VR_HIP(hipStreamWaitEvent(e->aux_stream, e->ev_fork, 0));
    e->stream = e->aux_stream;
    return 0;
  }
  int join() {
    e->stream = main_stream;
    VR_HIP(hipEventRecord(e->ev_join, e->aux_stream));
    VR_HIP(hipStreamWaitEvent(main_stream, e->ev_join, 0));
    return 0;
  }
};
}  // namespace

// ---- one block of queries ------------------------------------------------------------------------------------------

// A host query block goes into the pinned scratch and is read from there by query_image_kernel:
// no hipMemcpy on the latency path. Returns the pointer the kernels should read.
static const float* stage_query(vr_engine* e, const float* q, int nq, int mem) {
  if (mem == VR_MEM_DEVICE) return q;
  memcpy(pin_host<float>(e, kPinQuery), q, sizeof(float) * static_cast<size_t>(nq) * e->dim);
  return pin_dev<float>(e, kPinQuery);
}

// nq*k keys land in the pinned result area at kPinDenseKeys (readable after a stream sync).
// *two_stage is set when the f16 prefilter path ran: the caller must then sync and call dense_block_settle.
static int search_dense_block(vr_engine* e, const float* q_dev, int nq, int k, const uint8_t* mask,
                              bool allow_prefilter = true, bool* two_stage = nullptr) {
  if (two_stage) *two_stage = false;
  VR_TRY(dense_make_query_image(e, q_dev, nq));
  if (allow_prefilter && two_stage && prefilter_usable(e, nq, k)) {
    *two_stage = true;
    return prefilter_search(e, k, mask, pin_dev<uint64_t>(e, kPinDenseKeys), pin_dev<int32_t>(e, kPinCandCount));
  }
  // one or a few queries: scan and selection in one pass, results straight to pinned. A full
  // 16-query block offers 16x the candidates per tile; there the score array + select kernels win.
  if (k <= kFusedMaxK && nq <= 4)
    return dense_scan_topk(e, nq, k, mask, pin_dev<uint64_t>(e, kPinDenseKeys));
  const uint64_t* keys = nullptr;
  VR_TRY(dense_scores(e, nq, mask));
  VR_TRY(topk_select(e, e->scores.p, e->cap_rows, e->n_rows, nq, k, &keys));
  VR_HIP(hipMemcpyAsync(pin_host<uint64_t>(e, kPinDenseKeys), keys, sizeof(uint64_t) * static_cast<size_t>(nq) * k,
                        hipMemcpyDeviceToHost, e->stream));
  return 0;
}

// What follows the sync behind search_dense_block(.., true, &two_stage): the two-stage statistics, and when the
// candidate count at kPinCandCount is over the re-score budget (near-duplicate corpus) the one-stage exact scan of the
// same block and its sync.
static int dense_block_settle(vr_engine* e, const float* q_dev, int nb, int k, const uint8_t* mask, bool two_stage) {
  e->stat_two_stage += two_stage;
  if (!two_stage) return 0;
  const int32_t candidates = *pin_host<int32_t>(e, kPinCandCount);
  e->stat_last_candidates.store(candidates);
  if (candidates <= kMaxCandidates) return 0;
  ++e->stat_fallback;
  VR_TRY(search_dense_block(e, q_dev, nb, k, mask, false));
  VR_HIP(hipStreamSynchronize(e->stream));
  return 0;
}

// k keys land at kPinSparseKeys
static int search_sparse_block(vr_engine* e, const int32_t* q_idx, const float* q_val, int nnz, int k,
                               const uint8_t* mask, bool weights_given) {
  if (k <= kFusedMaxK)
    return sparse_scan_topk(e, q_idx, q_val, nnz, k, mask, weights_given, pin_dev<uint64_t>(e, kPinSparseKeys));
  const uint64_t* keys = nullptr;
  VR_TRY(sparse_scores(e, q_idx, q_val, nnz, mask, weights_given));
  VR_TRY(topk_select(e, e->sp_scores.p, e->cap_rows, e->n_rows, 1, k, &keys));
  VR_HIP(hipMemcpyAsync(pin_host<uint64_t>(e, kPinSparseKeys), keys, sizeof(uint64_t) * static_cast<size_t>(k),
                        hipMemcpyDeviceToHost, e->stream));
  return 0;
}

// Both legs of ONE hybrid query on the latency path (`e` is a search lane, n_rows > 0): the k dense keys end up in the
// pinned result area at kPinDenseKeys, the k sparse keys (when *have_sparse) at kPinSparseKeys; returns with the stream
// drained. The two legs share nothing but the mask: the (small, latency-bound) sparse leg is forked onto the auxiliary
// stream and runs under the dense scan. The k > kFusedMaxK sparse path borrows the dense leg's selection buffers and
// stays on the main stream.
static int hybrid_one_query(vr_engine* e, const float* q, int mem, const int32_t* q_idx, const float* q_val, int nnz, int k,
                            bool weights_given, const uint8_t* mask, bool* have_sparse_out) {
  const float* q_dev = stage_query(e, q, 1, mem);
  bool two_stage = false;
  const bool have_sparse = nnz > 0 && e->n_slices_dev > 0;
  *have_sparse_out = have_sparse;
  const bool fork = have_sparse && k <= kFusedMaxK;
  if (have_sparse) VR_CHECK(q_idx && q_val, "null sparse query");
  AuxScope aux(e);
  if (fork) VR_TRY(aux.mark());  // after the mask, before the dense leg
  VR_TRY(search_dense_block(e, q_dev, 1, k, mask, true, &two_stage));
  if (fork) {
    // queued after the dense leg (whose scan is already running by now), executed beside it
    VR_TRY(aux.enter());
    VR_TRY(search_sparse_block(e, q_idx, q_val, nnz, k, mask, weights_given));
    VR_TRY(aux.join());
  } else if (have_sparse) {
    VR_TRY(search_sparse_block(e, q_idx, q_val, nnz, k, mask, weights_given));
  }
  VR_HIP(hipStreamSynchronize(e->stream));
  return dense_block_settle(e, q_dev, 1, k, mask, two_stage);
}

int hybrid_one_fused(vr_engine* L, const float* q, int mem, const int32_t* q_idx, const float* q_val, int nnz, int limit,
                     double sparse_weight, int32_t fusion, const uint8_t* mask, int64_t* out_rows, double* out_scores,
                     int32_t* out_from_dense, int32_t* out_count) {
  const int k = limit * 3;  // prefetch_limit, vector_store.py:636
  bool have_sparse = false;
  VR_TRY(hybrid_one_query(L, q, mem, q_idx, q_val, nnz, k, false, mask, &have_sparse));
  return fuse_one(pin_host<uint64_t>(L, kPinDenseKeys), have_sparse ? pin_host<uint64_t>(L, kPinSparseKeys) : nullptr, k, limit,
                  sparse_weight, fusion, out_rows, out_scores, out_from_dense, out_count);
}

// ---- many dense queries under one filter ---------------------------------------------------------------------------

constexpr int kRound = 1024;  // queries per round of the batched dense search

// One round of the batched dense search (integer GEMM over the int8 shadow + exact re-score, batch.hip): nb <= kRound
// queries (host ones are staged in bq_stage) that pass the rows of `mask` or, with `planes`, query i those of plane
// cls[i] (a host array). Their nb x k keys are copied to keys_host and / or keys_dev. Returns with the stream drained,
// the batch statistics updated and the candidate counts in *cands: the keys of a query with more than kBatchCand are
// not valid, and the caller sends it through the exact scans.
static int batched_round(vr_engine* e, const float* q, int nb, int mem, int k, const uint8_t* mask, const uint32_t* planes,
                         int64_t plane_words, const int32_t* cls, uint64_t* keys_host, uint64_t* keys_dev,
                         std::vector<int32_t>* cands) {
  const size_t key_bytes = sizeof(uint64_t) * static_cast<size_t>(nb) * k;
  const float* q_dev = q;
  if (mem == VR_MEM_HOST) VR_TRY(e->bq_stage.grow(static_cast<int64_t>(nb) * e->dim, 0, e->stream));
  if (planes) VR_TRY(e->cls_of_q.grow(nb, 0, e->stream));
  if (mem == VR_MEM_HOST) {
    VR_HIP(hipMemcpyAsync(e->bq_stage.p, q, sizeof(float) * static_cast<size_t>(nb) * e->dim, hipMemcpyHostToDevice, e->stream));
    q_dev = e->bq_stage.p;
  }
  if (planes) VR_HIP(hipMemcpyAsync(e->cls_of_q.p, cls, sizeof(int32_t) * static_cast<size_t>(nb), hipMemcpyHostToDevice, e->stream));
  const uint64_t* round_keys = nullptr;
  const int32_t* cands_dev = nullptr;
  VR_TRY(batch_search(e, q_dev, nb, k, mask, &round_keys, &cands_dev, planes, planes ? e->cls_of_q.p : nullptr, plane_words));
  if (keys_host) VR_HIP(hipMemcpyAsync(keys_host, round_keys, key_bytes, hipMemcpyDeviceToHost, e->stream));
  if (keys_dev) VR_HIP(hipMemcpyAsync(keys_dev, round_keys, key_bytes, hipMemcpyDeviceToDevice, e->stream));
  cands->resize(static_cast<size_t>(nb));
  VR_HIP(hipMemcpyAsync(cands->data(), cands_dev, sizeof(int32_t) * static_cast<size_t>(nb), hipMemcpyDeviceToHost, e->stream));
  VR_HIP(hipStreamSynchronize(e->stream));  // (also: the caller's host queries and classes may be reused)
  e->stat_batched += nb;
  for (int32_t c : *cands) {
    e->stat_batch_cands += std::min<int32_t>(c, kBatchCand);
    e->stat_batch_fallback += c > kBatchCand;
  }
  return 0;
}

// Dense search of nq queries; the nq x k ranking keys ((order-preserving f32 score bits << 32) | ~row, descending,
// 0 = none) go to keys_host (host array) and/or keys_dev (device array). `e` is a search lane (SearchLane).
static int search_dense_keys_locked(vr_engine* e, const float* q, int nq, int mem, int k, const vr_filter* filter,
                                    uint64_t* keys_host, uint64_t* keys_dev, const uint8_t* mask_in = nullptr) {
  const size_t row_bytes = sizeof(uint64_t) * static_cast<size_t>(k);
  if (e->n_rows == 0) {
    if (keys_host) memset(keys_host, 0, row_bytes * static_cast<size_t>(nq));
    if (keys_dev) VR_HIP(hipMemsetAsync(keys_dev, 0, row_bytes * static_cast<size_t>(nq), e->stream));
    return 0;
  }
  const uint8_t* mask = mask_in;
  if (!mask) VR_TRY(filter_build_mask(e, filter, &mask));
  const uint64_t* pinned_keys = pin_host<uint64_t>(e, kPinDenseKeys);
  // one block of <= 16 queries through the one-/two-stage scans; its keys (in the pinned result area) go to slot `at`
  auto run_block = [&](const float* qsrc, int nb, int at) -> int {
    const float* q_dev = stage_query(e, qsrc, nb, mem);
    bool two_stage = false;
    VR_TRY(search_dense_block(e, q_dev, nb, k, mask, true, &two_stage));
    VR_HIP(hipStreamSynchronize(e->stream));
    VR_TRY(dense_block_settle(e, q_dev, nb, k, mask, two_stage));
    if (keys_host) memcpy(keys_host + static_cast<size_t>(at) * k, pinned_keys, row_bytes * static_cast<size_t>(nb));
    if (keys_dev) {
      VR_HIP(hipMemcpyAsync(keys_dev + static_cast<size_t>(at) * k, pinned_keys, row_bytes * static_cast<size_t>(nb),
                            hipMemcpyHostToDevice, e->stream));
      VR_HIP(hipStreamSynchronize(e->stream));  // the pinned area is reused by the next block
    }
    return 0;
  };
  if (batch_usable(e, nq, k)) {
    // many queries at once, a round at a time; a query over its candidate budget goes alone through the exact scans
    std::vector<int32_t> cands;
    for (int q0 = 0; q0 < nq; q0 += kRound) {
      const int nb = std::min(kRound, nq - q0);
      VR_TRY(batched_round(e, q + static_cast<int64_t>(q0) * e->dim, nb, mem, k, mask, nullptr, 0, nullptr,
                           keys_host ? keys_host + static_cast<size_t>(q0) * k : nullptr,
                           keys_dev ? keys_dev + static_cast<size_t>(q0) * k : nullptr, &cands));
      for (int i = 0; i < nb; ++i)
        if (cands[static_cast<size_t>(i)] > kBatchCand) VR_TRY(run_block(q + static_cast<int64_t>(q0 + i) * e->dim, 1, q0 + i));
    }
    return 0;
  }
  for (int q0 = 0; q0 < nq; q0 += kQueryBlock)
    VR_TRY(run_block(q + static_cast<int64_t>(q0) * e->dim, std::min(kQueryBlock, nq - q0), q0));
  return 0;
}

// ---- many sparse / hybrid queries per call (BASELINE configs[4]: 1k batched hybrid queries) ------------------------

// The sparse queries of a batch as the engine wants them: per query the terms in ascending id order, a repeated id
// keeping its first value (what sparse_run does for one query; Qdrant sorts sparse vectors by index [EXT]).
namespace {
struct SparseBatch {
  std::vector<int32_t> off;    // nq + 1: ranges of the queries the batch kernel serves (others: empty range)
  std::vector<int32_t> ids;
  std::vector<float> vals;
  std::vector<int32_t> alone;  // queries it cannot serve (more than kInvMaxTerms distinct terms): one by one
};
}  // namespace

static int prepare_sparse_batch(const int64_t* q_off, const int32_t* q_idx, const float* q_val, int nq, bool batchable,
                                SparseBatch* b) {
  b->off.assign(static_cast<size_t>(nq) + 1, 0);
  std::vector<std::pair<int32_t, float>> t;
  for (int i = 0; i < nq; ++i) {
    const int64_t lo = q_off[i], hi = q_off[i + 1];
    VR_CHECK(hi >= lo && hi - lo <= kMaxQueryTerms, "sparse query %d has %lld terms (0..%d supported)", i,
             static_cast<long long>(hi - lo), kMaxQueryTerms);
    t.clear();
    for (int64_t j = lo; j < hi; ++j) t.emplace_back(q_idx[j], q_val[j]);
    std::stable_sort(t.begin(), t.end(), [](const auto& a, const auto& c) { return a.first < c.first; });
    t.erase(std::unique(t.begin(), t.end(), [](const auto& a, const auto& c) { return a.first == c.first; }), t.end());
    if (!t.empty() && (!batchable || static_cast<int>(t.size()) > kInvMaxTerms)) {
      b->alone.push_back(i);
    } else {
      for (const auto& p : t) {
        b->ids.push_back(p.first);
        b->vals.push_back(p.second);
      }
    }
    b->off[static_cast<size_t>(i) + 1] = static_cast<int32_t>(b->ids.size());
  }
  return 0;
}

// Queues the batch kernel of the prepared queries on e->stream; the nq x k keys end up in e->sq_keys (device).
static int sparse_batch_launch(vr_engine* e, const SparseBatch& b, int nq, int k, bool weights_given, const uint8_t* mask,
                               bool allow_grouped = true, const ClassPlanes* classes = nullptr) {
  const int64_t nt = static_cast<int64_t>(b.ids.size());
  VR_TRY(e->sq_off.grow(nq + 1, 0, e->stream));
  VR_TRY(e->sq_ids.grow(std::max<int64_t>(nt, 1), 0, e->stream));
  VR_TRY(e->sq_val.grow(std::max<int64_t>(nt, 1), 0, e->stream));
  VR_TRY(e->sq_w.grow(std::max<int64_t>(2 * nt, 1), 0, e->stream));  // weights, then the terms' document-frequency shares
  VR_TRY(e->sq_keys.grow(static_cast<int64_t>(nq) * k, 0, e->stream));
  if (nt == 0 || e->n_rows == 0 || e->n_slices_dev == 0) {
    VR_HIP(hipMemsetAsync(e->sq_keys.p, 0, sizeof(uint64_t) * static_cast<size_t>(nq) * k, e->stream));
    return 0;
  }
  VR_HIP(hipMemcpyAsync(e->sq_off.p, b.off.data(), sizeof(int32_t) * (static_cast<size_t>(nq) + 1), hipMemcpyHostToDevice, e->stream));
  VR_HIP(hipMemcpyAsync(e->sq_ids.p, b.ids.data(), sizeof(int32_t) * static_cast<size_t>(nt), hipMemcpyHostToDevice, e->stream));
  VR_HIP(hipMemcpyAsync(e->sq_val.p, b.vals.data(), sizeof(float) * static_cast<size_t>(nt), hipMemcpyHostToDevice, e->stream));
  return inv_scan_topk_batch(e, e->sq_off.p, e->sq_ids.p, e->sq_val.p, e->sq_w.p, nq, static_cast<int>(nt), weights_given,
                             static_cast<float>(e->n_sparse_points), mask, k, e->sq_keys.p, b.off.data(), b.ids.data(),
                             allow_grouped, classes);
}

// After the stream of a sparse_batch_launch of n queries has been synchronised: the grouped scan gives up the queries
// whose candidate regions overflowed (invert.hip), and (*flagged)[i] != 0 for those. *flagged stays empty, and nothing
// is read from the device, when there are none. Runs on e->stream and waits for it.
static int read_overflowed(vr_engine* e, int n, std::vector<int32_t>* flagged) {
  if (*pin_host<int32_t>(e, kPinSparseOverflow) == 0 || !e->sq_overflow_q) return 0;
  flagged->resize(static_cast<size_t>(n));
  VR_HIP(hipMemcpyAsync(flagged->data(), e->sq_overflow_q, sizeof(int32_t) * static_cast<size_t>(n), hipMemcpyDeviceToHost, e->stream));
  VR_HIP(hipStreamSynchronize(e->stream));
  return 0;
}

// The overflowed queries of a batch (read_overflowed) are repeated on the per-query kernels, whose answer does not
// depend on any budget, and their rows of keys_host replaced. Runs on e->stream and waits for it.
static int sparse_batch_redo_if_overflowed(vr_engine* e, const SparseBatch& b, int nq, int k, bool weights_given,
                                           const uint8_t* mask, uint64_t* keys_host) {
  std::vector<int32_t> flagged;
  VR_TRY(read_overflowed(e, nq, &flagged));
  if (flagged.empty()) return 0;
  SparseBatch again;  // the same batch with the other queries' terms left out (an empty range: an empty list, at no cost)
  again.off.assign(static_cast<size_t>(nq) + 1, 0);
  int64_t n_again = 0;
  for (int i = 0; i < nq; ++i) {
    if (flagged[static_cast<size_t>(i)]) {
      again.ids.insert(again.ids.end(), b.ids.begin() + b.off[static_cast<size_t>(i)], b.ids.begin() + b.off[static_cast<size_t>(i) + 1]);
      again.vals.insert(again.vals.end(), b.vals.begin() + b.off[static_cast<size_t>(i)], b.vals.begin() + b.off[static_cast<size_t>(i) + 1]);
      ++n_again;
    }
    again.off[static_cast<size_t>(i) + 1] = static_cast<int32_t>(again.ids.size());
  }
  e->stat_sparse_group_redo.fetch_add(n_again);
  if (n_again == 0) return 0;
  VR_TRY(sparse_batch_launch(e, again, nq, k, weights_given, mask, false));
  std::vector<uint64_t> keys(static_cast<size_t>(nq) * k);
  VR_HIP(hipMemcpyAsync(keys.data(), e->sq_keys.p, sizeof(uint64_t) * keys.size(), hipMemcpyDeviceToHost, e->stream));
  VR_HIP(hipStreamSynchronize(e->stream));
  for (int i = 0; i < nq; ++i)
    if (flagged[static_cast<size_t>(i)])
      memcpy(keys_host + static_cast<size_t>(i) * k, keys.data() + static_cast<size_t>(i) * k, sizeof(uint64_t) * static_cast<size_t>(k));
  return 0;
}

// The queries the batch kernel could not take, one at a time through the single-query scans (e->stream); their keys
// replace row i of keys_host. q_off / q_idx / q_val: the caller's arrays.
static int sparse_batch_stragglers(vr_engine* e, const SparseBatch& b, const int64_t* q_off, const int32_t* q_idx,
                                   const float* q_val, int k, bool weights_given, const uint8_t* mask, uint64_t* keys_host) {
  for (int32_t i : b.alone) {
    const int nnz = static_cast<int>(q_off[i + 1] - q_off[i]);
    uint64_t* dst = keys_host + static_cast<size_t>(i) * k;
    if (e->n_rows == 0 || e->n_slices_dev == 0) {
      memset(dst, 0, sizeof(uint64_t) * static_cast<size_t>(k));
      continue;
    }
    VR_TRY(search_sparse_block(e, q_idx + q_off[i], q_val + q_off[i], nnz, k, mask, weights_given));
    VR_HIP(hipStreamSynchronize(e->stream));
    memcpy(dst, pin_host<uint64_t>(e, kPinSparseKeys), sizeof(uint64_t) * static_cast<size_t>(k));
  }
  return 0;
}

// nq sparse searches -> nq x k keys in keys_host. `e` is a search lane; everything runs on e->stream.
static int search_sparse_keys_locked(vr_engine* e, const int64_t* q_off, const int32_t* q_idx, const float* q_val, int nq,
                                     int k, bool weights_given, const uint8_t* mask, uint64_t* keys_host) {
  SparseBatch b;
  VR_TRY(prepare_sparse_batch(q_off, q_idx, q_val, nq, k <= kFusedMaxK && inv_usable(e, 1), &b));
  VR_TRY(sparse_batch_launch(e, b, nq, k, weights_given, mask));
  VR_HIP(hipMemcpyAsync(keys_host, e->sq_keys.p, sizeof(uint64_t) * static_cast<size_t>(nq) * k, hipMemcpyDeviceToHost, e->stream));
  VR_HIP(hipStreamSynchronize(e->stream));
  VR_TRY(sparse_batch_redo_if_overflowed(e, b, nq, k, weights_given, mask, keys_host));
  return sparse_batch_stragglers(e, b, q_off, q_idx, q_val, k, weights_given, mask, keys_host);
}

// Both legs of nq hybrid queries: nq x k dense keys and nq x k sparse keys (host arrays). The sparse batch is queued
// on the lane's auxiliary stream first and runs beside the dense batch (its kernels are small and latency-bound).
static int hybrid_keys_locked(vr_engine* e, const float* q, int nq, int mem, const int64_t* sq_off, const int32_t* sq_idx,
                              const float* sq_val, int k, bool weights_given, const vr_filter* filter, uint64_t* dense_host,
                              uint64_t* sparse_host) {
  const size_t bytes = sizeof(uint64_t) * static_cast<size_t>(nq) * k;
  if (e->n_rows == 0) {
    memset(dense_host, 0, bytes);
    memset(sparse_host, 0, bytes);
    return 0;
  }
  const uint8_t* mask = nullptr;
  VR_TRY(filter_build_mask(e, filter, &mask));
  if (nq == 1) {  // one query: the latency path (query in the pinned area / kernel arguments, both legs side by side)
    const int nnz = sq_off ? static_cast<int>(sq_off[1] - sq_off[0]) : 0;
    bool sparse_ran = false;
    VR_TRY(hybrid_one_query(e, q, mem, nnz ? sq_idx + sq_off[0] : nullptr, nnz ? sq_val + sq_off[0] : nullptr, nnz, k,
                            weights_given, mask, &sparse_ran));
    memcpy(dense_host, pin_host<uint64_t>(e, kPinDenseKeys), bytes);
    if (sparse_ran) memcpy(sparse_host, pin_host<uint64_t>(e, kPinSparseKeys), bytes);
    else memset(sparse_host, 0, bytes);
    return 0;
  }
  const bool have_sparse = sq_off != nullptr && sq_off[nq] > sq_off[0] && e->n_slices_dev > 0;
  SparseBatch b;
  if (have_sparse) {
    VR_TRY(check_sparse_csr(sq_off, sq_idx, sq_val, nq, false));
    VR_TRY(prepare_sparse_batch(sq_off, sq_idx, sq_val, nq, k <= kFusedMaxK && inv_usable(e, 1), &b));
    AuxScope aux(e);
    VR_TRY(aux.mark());  // after the mask
    VR_TRY(aux.enter());
    VR_TRY(sparse_batch_launch(e, b, nq, k, weights_given, mask));
    VR_CHECK(hipMemcpyAsync(sparse_host, e->sq_keys.p, bytes, hipMemcpyDeviceToHost, e->stream) == hipSuccess,
             "copying the sparse keys failed");
  } else {
    memset(sparse_host, 0, bytes);
  }
  VR_TRY(search_dense_keys_locked(e, q, nq, mem, k, filter, dense_host, nullptr, mask));
  if (have_sparse) {
    VR_HIP(hipStreamSynchronize(e->aux_stream));
    VR_TRY(sparse_batch_redo_if_overflowed(e, b, nq, k, weights_given, mask, sparse_host));
    VR_TRY(sparse_batch_stragglers(e, b, sq_off, sq_idx, sq_val, k, weights_given, mask, sparse_host));
  }
  return 0;
}

// ---- filtered batches: a filter, a limit and a sparse weight per query (vr_search_*_multi) -------------------------

int classify_queries(const vr_filter* filters, int n_filters, const int32_t* filter_of_query, int nq, QueryClasses* qc) {
  VR_CHECK(n_filters >= 0 && (n_filters == 0 || (filters && filter_of_query)), "bad filters");
  for (int j = 0; j < n_filters; ++j) {
    VR_CHECK(filters[j].struct_size == static_cast<int32_t>(sizeof(vr_filter)), "filters[%d]: vr_filter size mismatch", j);
    VR_CHECK(filters[j].n_must_folder_sets >= 0 && filters[j].n_must_folder_sets <= 2, "filters[%d]: at most 2 must-sets", j);
  }
  std::vector<int32_t> class_of(static_cast<size_t>(n_filters) + 1, -1);  // [n_filters]: no filter
  qc->of.assign(static_cast<size_t>(nq), 0);
  qc->filter.clear();
  for (int i = 0; i < nq; ++i) {
    const int32_t f = filter_of_query ? filter_of_query[i] : -1;
    VR_CHECK(f >= -1 && f < n_filters, "filter_of_query[%d] = %d not in -1..%d", i, f, n_filters - 1);
    int32_t& c = class_of[static_cast<size_t>(f < 0 ? n_filters : f)];
    if (c < 0) {
      c = static_cast<int32_t>(qc->filter.size());
      qc->filter.push_back(f < 0 ? nullptr : filters + f);
    }
    qc->of[static_cast<size_t>(i)] = c;
  }
  return 0;
}

// Bytes of class planes one batched scan may use (VR_CLASS_PLANE_MIB, default 256): a batch with more classes runs in
// slices of classes, one scan per slice.
static int64_t class_plane_budget() {
  static const int64_t mib = getenv("VR_CLASS_PLANE_MIB") ? std::max(0, atoi(getenv("VR_CLASS_PLANE_MIB"))) : 256;
  return mib << 20;
}

namespace {  // (to the end of MultiBatch::run)

// rows idx[0 .. n) of q (dim floats each) side by side in *out
static void gather_rows(const float* q, int dim, const int32_t* idx, int n, std::vector<float>* out) {
  out->resize(static_cast<size_t>(n) * dim);
  for (int j = 0; j < n; ++j)
    memcpy(out->data() + static_cast<size_t>(j) * dim, q + static_cast<int64_t>(idx[j]) * dim, sizeof(float) * dim);
}

// the sparse queries idx[0 .. n) of a CSR as a CSR of their own
struct GatheredCsr {
  std::vector<int64_t> off;
  std::vector<int32_t> ids;
  std::vector<float> vals;
};
static void gather_csr(const int64_t* off, const int32_t* ids, const float* vals, const int32_t* idx, int n, GatheredCsr* out) {
  out->off.assign(1, 0);
  out->ids.clear();
  out->vals.clear();
  for (int j = 0; j < n; ++j) {
    const int32_t i = idx[j];
    out->ids.insert(out->ids.end(), ids + off[i], ids + off[i + 1]);
    out->vals.insert(out->vals.end(), vals + off[i], vals + off[i + 1]);
    out->off.push_back(static_cast<int64_t>(out->ids.size()));
  }
}

// Both legs of a filtered batch. Query i asks for its ks[i] best keys under its class's filter; they go to row i of
// dense_host / sparse_host ([nq][kstride], zero padded; sparse_host null: dense only). q: nq x D. Three steps over this
// state: dense_batched, sparse_grouped, remainder. Every list is the exact top-k of the single call, so a list of the
// largest k of a group, cut to a query's own k, is that query's list.
struct MultiBatch {
  vr_engine* e;
  const float* q;  // host array (run() copies device queries back)
  int nq;
  const int32_t* ks;
  int kstride;
  const QueryClasses& qc;
  const int64_t* sq_off;
  const int32_t* sq_idx;
  const float* sq_val;
  uint64_t *dense_host, *sparse_host;
  std::vector<uint8_t> done{}, sparse_done{};  // per query: the leg has its keys
  std::vector<int32_t> order{};                // the queries of k <= kFusedMaxK, sorted by class
  int kb = 0;                                  // their largest k
  const uint32_t* all_planes = nullptr;        // e->cls_planes while it holds the planes of every class

  int n_cls() const { return static_cast<int>(qc.filter.size()); }
  int cls(int i) const { return qc.of[static_cast<size_t>(i)]; }
  void put(uint64_t* dst, int i, const uint64_t* src) const {
    memcpy(dst + static_cast<size_t>(i) * kstride, src, sizeof(uint64_t) * static_cast<size_t>(ks[i]));
  }
  int dense_batched();
  int sparse_grouped();
  int remainder();
  int run(int mem);
};

//   dense   the queries of k <= kFusedMaxK share the batched scan (batch.hip), which reads each query's class plane; the
//           queries sorted by class, so that a 128-query block column mostly sees one class. Classes go in slices whose
//           planes fit class_plane_budget(). A slice too small to batch, the larger k and the queries over their candidate
//           budget are left to remainder().
int MultiBatch::dense_batched() {
  if (!batch_usable(e, static_cast<int>(order.size()), kb)) return 0;
  const int64_t words = filter_plane_words(e);
  const int per_slice = static_cast<int>(std::min<int64_t>(n_cls(), std::max<int64_t>(1, class_plane_budget() / (4 * words))));
  std::vector<float> qs;
  std::vector<int32_t> slot;
  std::vector<uint64_t> keys;
  std::vector<int32_t> cands;
  size_t at = 0;
  for (int c0 = 0; c0 < n_cls() && at < order.size(); c0 += per_slice) {
    const int c1 = std::min(n_cls(), c0 + per_slice);
    size_t end = at;
    while (end < order.size() && cls(order[end]) < c1) ++end;
    const int ns = static_cast<int>(end - at);
    if (!batch_usable(e, ns, kb)) {  // (left to remainder())
      at = end;
      continue;
    }
    const uint32_t* planes = nullptr;
    VR_TRY(filter_build_planes(e, qc.filter.data() + c0, c1 - c0, &planes));
    all_planes = c0 == 0 && c1 == n_cls() ? planes : nullptr;
    for (int r0 = 0; r0 < ns; r0 += kRound) {
      const int nb = std::min(kRound, ns - r0);
      const int32_t* idx = order.data() + at + r0;
      gather_rows(q, e->dim, idx, nb, &qs);
      slot.resize(static_cast<size_t>(nb));
      for (int j = 0; j < nb; ++j) slot[static_cast<size_t>(j)] = cls(idx[j]) - c0;
      keys.resize(static_cast<size_t>(nb) * kb);
      VR_TRY(batched_round(e, qs.data(), nb, VR_MEM_HOST, kb, nullptr, planes, words, slot.data(), keys.data(), nullptr, &cands));
      for (int j = 0; j < nb; ++j) {
        if (cands[static_cast<size_t>(j)] > kBatchCand) continue;  // candidate budget exceeded: remainder() redoes it
        put(dense_host, idx[j], keys.data() + static_cast<size_t>(j) * kb);
        done[static_cast<size_t>(idx[j])] = 1;
      }
    }
    at = end;
  }
  return 0;
}

//   sparse  the queries of k <= kFusedMaxK as ONE grouped scan of the inverted index when it takes the batch (invert.hip:
//           groups hold queries of one class and read its plane); the rest — longer queries, the larger k, queries whose
//           candidates overflowed, batches the grouped scan does not take — are left to remainder().
int MultiBatch::sparse_grouped() {
  const int n = static_cast<int>(order.size());
  if (!(sparse_host && sq_off && e->n_slices_dev > 0 && n > 0 &&
        static_cast<int64_t>(n_cls()) * 4 * filter_plane_words(e) <= class_plane_budget() && inv_class_grouped_usable(e, n)))
    return 0;
  GatheredCsr g;
  gather_csr(sq_off, sq_idx, sq_val, order.data(), n, &g);
  std::vector<int32_t> cls_of;
  for (int32_t i : order) cls_of.push_back(cls(i));
  SparseBatch b;
  VR_TRY(prepare_sparse_batch(g.off.data(), g.ids.data(), g.vals.data(), n, true, &b));
  if (b.ids.empty()) return 0;
  const uint32_t* planes = all_planes;
  if (!planes) VR_TRY(filter_build_planes(e, qc.filter.data(), n_cls(), &planes));
  const ClassPlanes classes{planes, filter_plane_words(e), cls_of.data()};
  VR_TRY(sparse_batch_launch(e, b, n, kb, false, e->live.p, true, &classes));
  std::vector<uint64_t> keys(static_cast<size_t>(n) * kb);
  VR_HIP(hipMemcpyAsync(keys.data(), e->sq_keys.p, sizeof(uint64_t) * keys.size(), hipMemcpyDeviceToHost, e->stream));
  VR_HIP(hipStreamSynchronize(e->stream));
  std::vector<int32_t> flagged;  // (redone class by class in remainder())
  VR_TRY(read_overflowed(e, n, &flagged));
  flagged.resize(static_cast<size_t>(n), 0);
  std::vector<uint8_t> alone(static_cast<size_t>(n), 0);
  for (int32_t j : b.alone) alone[static_cast<size_t>(j)] = 1;
  for (int j = 0; j < n; ++j) {
    if (alone[static_cast<size_t>(j)] || flagged[static_cast<size_t>(j)]) {
      e->stat_sparse_group_redo += flagged[static_cast<size_t>(j)] != 0;
      continue;
    }
    put(sparse_host, order[static_cast<size_t>(j)], keys.data() + static_cast<size_t>(j) * kb);
    sparse_done[static_cast<size_t>(order[static_cast<size_t>(j)])] = 1;
  }
  return 0;
}

//   rest    class by class, what the batched scans left, on the byte mask of that class (filter_mask_kernel): the dense
//           queries through search_dense_keys_locked, the sparse ones as one batched sparse search
//           (search_sparse_keys_locked); in each class the queries of k <= kFusedMaxK, then the rest, each part at its
//           largest k.
int MultiBatch::remainder() {
  std::vector<std::vector<int32_t>> members(static_cast<size_t>(n_cls()));
  for (int i = 0; i < nq; ++i) members[static_cast<size_t>(cls(i))].push_back(i);
  const bool sparse_index = e->n_slices_dev > 0;
  std::vector<int32_t> part;
  int kq = 0;
  // the members of m on one side of kFusedMaxK whose leg is not done yet, and their largest k
  auto select_part = [&](const std::vector<int32_t>& m, bool big, const std::vector<uint8_t>& have) {
    part.clear();
    kq = 0;
    for (int32_t i : m)
      if ((ks[i] > kFusedMaxK) == big && !have[static_cast<size_t>(i)]) {
        part.push_back(i);
        kq = std::max(kq, ks[i]);
      }
    return static_cast<int>(part.size());
  };
  std::vector<float> qs;
  std::vector<uint64_t> keys;
  GatheredCsr g;
  for (int c = 0; c < n_cls(); ++c) {
    const std::vector<int32_t>& m = members[static_cast<size_t>(c)];
    bool dense_left = false, sparse_terms = false;
    for (int32_t i : m) {
      dense_left |= !done[static_cast<size_t>(i)];
      sparse_terms |= sparse_host && sq_off && sq_off[i + 1] > sq_off[i] && !sparse_done[static_cast<size_t>(i)];
    }
    if (!dense_left && !(sparse_terms && sparse_index)) continue;
    const uint8_t* mask = nullptr;
    VR_TRY(filter_build_mask(e, qc.filter[static_cast<size_t>(c)], &mask));
    for (int big = 0; big < 2; ++big) {
      if (const int n = select_part(m, big != 0, done)) {
        gather_rows(q, e->dim, part.data(), n, &qs);
        keys.resize(static_cast<size_t>(n) * kq);
        VR_TRY(search_dense_keys_locked(e, qs.data(), n, VR_MEM_HOST, kq, nullptr, keys.data(), nullptr, mask));
        for (int j = 0; j < n; ++j) put(dense_host, part[static_cast<size_t>(j)], keys.data() + static_cast<size_t>(j) * kq);
      }
      if (!sparse_terms || !sparse_index) continue;
      const int n = select_part(m, big != 0, sparse_done);
      gather_csr(sq_off, sq_idx, sq_val, part.data(), n, &g);
      if (g.ids.empty()) continue;
      keys.resize(static_cast<size_t>(n) * kq);
      VR_TRY(search_sparse_keys_locked(e, g.off.data(), g.ids.data(), g.vals.data(), n, kq, false, mask, keys.data()));
      for (int j = 0; j < n; ++j) put(sparse_host, part[static_cast<size_t>(j)], keys.data() + static_cast<size_t>(j) * kq);
    }
  }
  return 0;
}

// mem: where q is. Device queries are copied back once (the batch is gathered by class on the host).
int MultiBatch::run(int mem) {
  std::vector<float> copy;
  if (mem != VR_MEM_HOST) {
    copy.resize(static_cast<size_t>(nq) * e->dim);
    VR_HIP(hipMemcpyAsync(copy.data(), q, sizeof(float) * copy.size(), hipMemcpyDeviceToHost, e->stream));
    VR_HIP(hipStreamSynchronize(e->stream));
    q = copy.data();
  }
  const size_t bytes = sizeof(uint64_t) * static_cast<size_t>(nq) * kstride;
  memset(dense_host, 0, bytes);
  if (sparse_host) memset(sparse_host, 0, bytes);
  if (e->n_rows == 0) return 0;
  done.assign(static_cast<size_t>(nq), 0);
  sparse_done.assign(static_cast<size_t>(nq), 0);
  for (int i = 0; i < nq; ++i)
    if (ks[i] <= kFusedMaxK) {
      order.push_back(i);
      kb = std::max(kb, ks[i]);
    }
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t c) { return cls(a) < cls(c); });
  VR_TRY(dense_batched());
  VR_TRY(sparse_grouped());
  return remainder();
}

}  // namespace

// The dense leg of a filtered batch on lane L (vr_search_dense_multi after its checks): nq x k keys to keys_host.
int dense_multi_keys(vr_engine* L, const float* q, int nq, int mem, int k, const QueryClasses& qc, uint64_t* keys_host) {
  if (qc.filter.size() == 1)  // one class: vr_search_dense
    return search_dense_keys_locked(L, q, nq, mem, k, qc.filter[0], keys_host, nullptr);
  const std::vector<int32_t> ks(static_cast<size_t>(nq), k);
  return MultiBatch{L, q, nq, ks.data(), k, qc, nullptr, nullptr, nullptr, keys_host, nullptr}.run(mem);
}

// Both legs of a filtered hybrid batch on lane L (vr_search_hybrid_batch_multi after its checks): query i asks for
// 3 x limits[i] keys per leg; nq x kstride keys to dense / sparse.
int hybrid_multi_keys(vr_engine* L, const float* q, int nq, int mem, const int64_t* sq_off, const int32_t* sq_idx,
                      const float* sq_val, const int32_t* limits, const QueryClasses& qc, int kstride, uint64_t* dense,
                      uint64_t* sparse) {
  if (qc.filter.size() == 1)  // one class: vr_search_hybrid_batch's legs, at the largest k
    return hybrid_keys_locked(L, q, nq, mem, sq_off, sq_idx, sq_val, kstride, false, qc.filter[0], dense, sparse);
  std::vector<int32_t> ks(static_cast<size_t>(nq));
  for (int i = 0; i < nq; ++i) ks[static_cast<size_t>(i)] = 3 * limits[i];
  return MultiBatch{L, q, nq, ks.data(), kstride, qc, sq_off, sq_idx, sq_val, dense, sparse}.run(mem);
}

// Fusion of every query of a hybrid batch on the host threads, each with its own limit and weight
// (vector_store.py:659-697, once per query). Query i's answer goes to output row out_row[i] (out_row null: row i).
int fuse_multi(const uint64_t* dense, const uint64_t* sparse, int nq, int kstride, const int32_t* limits,
               const double* sparse_weights, int32_t fusion, const int32_t* out_row, int32_t out_stride, int64_t* out_rows,
               double* out_scores, int32_t* out_from_dense, int32_t* out_counts) {
  std::atomic<int> failed{0};
  parallel_for(nq, 8, [&](int64_t i) {
    const int64_t r = out_row ? out_row[i] : i;
    const int64_t at = r * out_stride;
    const int rc = fuse_one(dense + static_cast<size_t>(i) * kstride, sparse + static_cast<size_t>(i) * kstride, 3 * limits[i],
                            limits[i], sparse_weights[i], fusion, out_rows + at, out_scores + at,
                            out_from_dense ? out_from_dense + at : nullptr, out_counts + r);
    if (rc != 0) failed.store(1);
  });
  VR_CHECK(!failed.load(), "fusion failed");
  return 0;
}

}  // namespace vr

using namespace vr;

extern "C" {

int vr_search_dense(vr_engine* e, const float* q, int32_t nq, int mem, int32_t k,
                    const vr_filter* filter, int64_t* rows, float* scores, int32_t* counts) {
  VR_TRY(check_engine(e));
  VR_CHECK(q && rows && scores && nq >= 1, "bad arguments");
  VR_TRY(check_k(k));
  VR_TRY(check_mem(mem));
  SearchLane lane(e);
  VR_TRY(lane.acquire(mem == VR_MEM_DEVICE));
  std::vector<uint64_t> keys(static_cast<size_t>(nq) * k);
  VR_TRY(search_dense_keys_locked(lane.L, q, nq, mem, k, filter, keys.data(), nullptr));
  decode_lists(keys.data(), nq, k, rows, scores, counts);
  return 0;
}

int vr_search_dense_keys(vr_engine* e, const float* q, int32_t nq, int mem, int32_t k, const vr_filter* filter,
                         uint64_t* keys, int keys_mem) {
  VR_TRY(check_engine(e));
  VR_CHECK(q && keys && nq >= 1, "bad arguments");
  VR_TRY(check_k(k));
  VR_CHECK((mem == VR_MEM_HOST || mem == VR_MEM_DEVICE) && (keys_mem == VR_MEM_HOST || keys_mem == VR_MEM_DEVICE), "bad mem");
  SearchLane lane(e);
  VR_TRY(lane.acquire(true));  // (device output: ordered behind the caller's stream either way)
  VR_TRY(search_dense_keys_locked(lane.L, q, nq, mem, k, filter, keys_mem == VR_MEM_HOST ? keys : nullptr,
                                  keys_mem == VR_MEM_DEVICE ? keys : nullptr));
  if (keys_mem == VR_MEM_DEVICE) VR_HIP(hipStreamSynchronize(lane.L->stream));
  return 0;
}

int vr_search_sparse(vr_engine* e, const int32_t* q_idx, const float* q_val, int32_t nnz, int32_t k,
                     int32_t weights_given, const vr_filter* filter, int64_t* rows, float* scores,
                     int32_t* count) {
  VR_TRY(check_engine(e));
  VR_CHECK(rows && scores && count, "bad arguments");
  VR_TRY(check_k(k));
  SearchLane lane(e);
  VR_TRY(lane.acquire(false));
  e = lane.L;  // everything below runs on the lane: its stream, its scratch, its view of the index
  *count = 0;
  for (int i = 0; i < k; ++i) {
    rows[i] = -1;
    scores[i] = 0.0f;
  }
  if (e->n_rows == 0 || e->n_slices_dev == 0 || nnz <= 0) return 0;
  VR_CHECK(q_idx && q_val, "null sparse query");
  const uint8_t* mask = nullptr;
  VR_TRY(filter_build_mask(e, filter, &mask));
  const uint64_t* host_keys = pin_host<uint64_t>(e, kPinSparseKeys);
  VR_TRY(search_sparse_block(e, q_idx, q_val, nnz, k, mask, weights_given != 0));
  VR_HIP(hipStreamSynchronize(e->stream));
  *count = static_cast<int32_t>(decode_keys(host_keys, k, rows, scores));
  return 0;
}

int vr_search_hybrid(vr_engine* e, const float* q, int mem, const int32_t* q_idx, const float* q_val,
                     int32_t nnz, int32_t limit, double sparse_weight, int32_t fusion,
                     const vr_filter* filter, int64_t* out_rows, double* out_scores,
                     int32_t* out_from_dense, int32_t* out_count) {
  VR_TRY(check_engine(e));
  VR_CHECK(q && out_rows && out_scores && out_count, "bad arguments");
  VR_TRY(check_fusion_limit(limit, fusion));
  VR_TRY(check_mem(mem));
  SearchLane lane(e);
  VR_TRY(lane.acquire(mem == VR_MEM_DEVICE));
  e = lane.L;  // everything below runs on the lane: its stream, its scratch, its view of the index
  *out_count = 0;
  if (e->n_rows == 0) return 0;
  const uint8_t* mask = nullptr;
  VR_TRY(filter_build_mask(e, filter, &mask));
  return hybrid_one_fused(e, q, mem, q_idx, q_val, nnz, limit, sparse_weight, fusion, mask, out_rows, out_scores,
                          out_from_dense, out_count);
}

int vr_fuse_minmax(const int64_t* d_rows, const float* d_scores, int32_t nd, const int64_t* s_rows,
                   const float* s_scores, int32_t ns, int32_t limit, double sparse_weight,
                   int32_t json_scores, int64_t* out_rows, double* out_scores,
                   int32_t* out_from_dense, int32_t* out_count) {
  VR_CHECK(nd >= 0 && ns >= 0 && out_rows && out_scores && out_count, "bad arguments");
  return fuse_minmax(d_rows, d_scores, nd, s_rows, s_scores, ns, limit, sparse_weight, json_scores,
                     out_rows, out_scores, out_from_dense, out_count);
}

int vr_fuse_rrf(const int64_t* d_rows, int32_t nd, const int64_t* s_rows, int32_t ns, int32_t limit,
                int64_t* out_rows, double* out_scores, int32_t* out_from_dense, int32_t* out_count) {
  VR_CHECK(nd >= 0 && ns >= 0 && out_rows && out_scores && out_count, "bad arguments");
  return fuse_rrf(d_rows, nd, s_rows, ns, limit, 0.0, out_rows, out_scores, out_from_dense, out_count);
}

int vr_fuse_batch(const int64_t* d_rows, const float* d_scores, const int32_t* d_counts, const int64_t* s_rows,
                  const float* s_scores, const int32_t* s_counts, int32_t nq, int32_t k, int32_t limit, double sparse_weight,
                  int32_t fusion, int32_t json_scores, int64_t* out_rows, double* out_scores, int32_t* out_from_dense,
                  int32_t* out_counts) {
  return fuse_batch(d_rows, d_scores, d_counts, s_rows, s_scores, s_counts, nq, k, limit, sparse_weight, fusion, json_scores,
                    out_rows, out_scores, out_from_dense, out_counts);
}

int vr_search_dense_multi(vr_engine* e, const float* q, int32_t nq, int mem, int32_t k, const vr_filter* filters,
                          int32_t n_filters, const int32_t* filter_of_query, int64_t* rows, float* scores, int32_t* counts) {
  // (the arguments are checked before the engine is touched)
  VR_CHECK(q && rows && scores && nq >= 1, "bad arguments");
  VR_TRY(check_k(k));
  VR_TRY(check_mem(mem));
  QueryClasses qc;
  VR_TRY(classify_queries(filters, n_filters, filter_of_query, nq, &qc));
  VR_TRY(check_engine(e));
  std::vector<uint64_t> keys(static_cast<size_t>(nq) * k);
  {
    SearchLane lane(e);
    VR_TRY(lane.acquire(mem == VR_MEM_DEVICE));
    VR_TRY(dense_multi_keys(lane.L, q, nq, mem, k, qc, keys.data()));
  }
  decode_lists(keys.data(), nq, k, rows, scores, counts);
  return 0;
}

int vr_search_hybrid_batch_multi(vr_engine* e, const float* q, int32_t nq, int mem, const int64_t* sq_off,
                                 const int32_t* sq_idx, const float* sq_val, const int32_t* limits,
                                 const double* sparse_weights, int32_t fusion, const vr_filter* filters, int32_t n_filters,
                                 const int32_t* filter_of_query, int32_t out_stride, int64_t* out_rows, double* out_scores,
                                 int32_t* out_from_dense, int32_t* out_counts) {
  // (the arguments are checked before the engine is touched)
  VR_CHECK(q && limits && sparse_weights && out_rows && out_scores && out_counts && nq >= 1, "bad arguments");
  VR_TRY(check_fusion(fusion));
  VR_TRY(check_mem(mem));
  int max_limit = 0;
  VR_TRY(check_limits(limits, nq, out_stride, &max_limit));
  if (sq_off) VR_TRY(check_sparse_csr(sq_off, sq_idx, sq_val, nq));
  QueryClasses qc;
  VR_TRY(classify_queries(filters, n_filters, filter_of_query, nq, &qc));
  VR_TRY(check_engine(e));
  const int kstride = 3 * max_limit;  // prefetch_limit, vector_store.py:636, of the largest limit
  const size_t per = static_cast<size_t>(nq) * kstride;
  std::vector<uint64_t> dense(per), sparse(per);
  {
    SearchLane lane(e);
    VR_TRY(lane.acquire(mem == VR_MEM_DEVICE));
    VR_TRY(hybrid_multi_keys(lane.L, q, nq, mem, sq_off, sq_idx, sq_val, limits, qc, kstride, dense.data(), sparse.data()));
  }
  return fuse_multi(dense.data(), sparse.data(), nq, kstride, limits, sparse_weights, fusion, nullptr, out_stride, out_rows,
                    out_scores, out_from_dense, out_counts);
}

int vr_search_sparse_batch(vr_engine* e, const int64_t* q_off, const int32_t* q_idx, const float* q_val, int32_t nq,
                           int32_t k, int32_t weights_given, const vr_filter* filter, int64_t* rows, float* scores,
                           int32_t* counts) {
  VR_TRY(check_engine(e));
  VR_CHECK(q_off && rows && scores && nq >= 1, "bad arguments");
  VR_TRY(check_k(k));
  VR_TRY(check_sparse_csr(q_off, q_idx, q_val, nq, false));  // (the terms per query: prepare_sparse_batch, when it is reached)
  SearchLane lane(e);
  VR_TRY(lane.acquire(false));
  vr_engine* L = lane.L;
  std::vector<uint64_t> keys(static_cast<size_t>(nq) * k, 0ull);
  if (L->n_rows > 0 && L->n_slices_dev > 0) {
    const uint8_t* mask = nullptr;
    VR_TRY(filter_build_mask(L, filter, &mask));
    VR_TRY(search_sparse_keys_locked(L, q_off, q_idx, q_val, nq, k, weights_given != 0, mask, keys.data()));
  }
  decode_lists(keys.data(), nq, k, rows, scores, counts);
  return 0;
}

int vr_search_hybrid_keys(vr_engine* e, const float* q, int32_t nq, int mem, const int64_t* sq_off, const int32_t* sq_idx,
                          const float* sq_val, int32_t k, int32_t weights_given, const vr_filter* filter, uint64_t* keys,
                          int keys_mem) {
  VR_TRY(check_engine(e));
  VR_CHECK(q && keys && nq >= 1, "bad arguments");
  VR_TRY(check_k(k));
  VR_CHECK((mem == VR_MEM_HOST || mem == VR_MEM_DEVICE) && (keys_mem == VR_MEM_HOST || keys_mem == VR_MEM_DEVICE), "bad mem");
  SearchLane lane(e);
  VR_TRY(lane.acquire(true));
  vr_engine* L = lane.L;
  const size_t per = static_cast<size_t>(nq) * k;
  std::vector<uint64_t> dense(per), sparse(per);
  VR_TRY(hybrid_keys_locked(L, q, nq, mem, sq_off, sq_idx, sq_val, k, weights_given != 0, filter, dense.data(), sparse.data()));
  // [query][dense list, sparse list][k]
  std::vector<uint64_t> both;
  uint64_t* dst = keys;
  if (keys_mem == VR_MEM_DEVICE) {
    both.resize(2 * per);
    dst = both.data();
  }
  for (int i = 0; i < nq; ++i) {
    memcpy(dst + (2 * static_cast<size_t>(i)) * k, dense.data() + static_cast<size_t>(i) * k, sizeof(uint64_t) * k);
    memcpy(dst + (2 * static_cast<size_t>(i) + 1) * k, sparse.data() + static_cast<size_t>(i) * k, sizeof(uint64_t) * k);
  }
  if (keys_mem == VR_MEM_DEVICE) {
    VR_HIP(hipMemcpyAsync(keys, both.data(), sizeof(uint64_t) * 2 * per, hipMemcpyHostToDevice, L->stream));
    VR_HIP(hipStreamSynchronize(L->stream));
  }
  return 0;
}

int vr_search_hybrid_batch(vr_engine* e, const float* q, int32_t nq, int mem, const int64_t* sq_off, const int32_t* sq_idx,
                           const float* sq_val, int32_t limit, double sparse_weight, int32_t fusion, const vr_filter* filter,
                           int64_t* out_rows, double* out_scores, int32_t* out_from_dense, int32_t* out_counts) {
  VR_TRY(check_engine(e));
  VR_CHECK(q && out_rows && out_scores && out_counts && nq >= 1, "bad arguments");
  VR_TRY(check_fusion_limit(limit, fusion));
  VR_TRY(check_mem(mem));
  const int k = 3 * limit;  // prefetch_limit, vector_store.py:636
  const size_t per = static_cast<size_t>(nq) * k;
  std::vector<uint64_t> dense(per), sparse(per);
  {
    SearchLane lane(e);
    VR_TRY(lane.acquire(mem == VR_MEM_DEVICE));
    VR_TRY(hybrid_keys_locked(lane.L, q, nq, mem, sq_off, sq_idx, sq_val, k, false, filter, dense.data(), sparse.data()));
  }
  const std::vector<int32_t> limits(static_cast<size_t>(nq), limit);  // one limit and one weight for every query
  const std::vector<double> weights(static_cast<size_t>(nq), sparse_weight);
  return fuse_multi(dense.data(), sparse.data(), nq, k, limits.data(), weights.data(), fusion, nullptr, limit, out_rows,
                    out_scores, out_from_dense, out_counts);
}

}  // extern "C"
