// extern "C" surface of libvoitta_engine.so (include/voitta_engine.h): engine lifecycle, the
// store (upsert / delete / count / read-back) and the three searches. Every entry point cites
// the reference call it stands in for in the header; this file only sequences kernels on the
// engine's stream and moves small results back to the host.

#include "engine_internal.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <thread>

#include "host_parallel.h"

namespace vr {

static thread_local std::string g_last_error;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
}

__global__ void fill_i64_kernel(int64_t* p, int64_t v, int64_t n) {
  int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

int ensure_rows(vr_engine* e, int64_t need) {
  if (need <= e->cap_rows) return 0;
  int64_t ncap = e->cap_rows ? e->cap_rows : 1024;
  while (ncap < need) ncap *= 2;
  ncap = (ncap + 63) / 64 * 64;
  const int64_t keep_rows = e->n_rows;
  const int64_t keep_tiles = (keep_rows + kTileRows - 1) / kTileRows;
  VR_TRY(e->corpus.grow(ncap * e->dim, keep_tiles * kTileRows * e->dim, e->stream));
  if (e->prefilter) {
    const int per_u16 = e->prefilter8 ? 2 : 1;  // shadow elements per uint16 of storage
    VR_TRY(e->corpus16.grow(ncap * e->dim / per_u16, keep_tiles * kTileRows * e->dim / per_u16, e->stream));
    VR_TRY(e->row_err.grow(ncap, keep_tiles * kTileRows, e->stream));
    if (e->prefilter8) VR_TRY(e->row_scale.grow(ncap, keep_tiles * kTileRows, e->stream));
  }
  VR_TRY(e->live.grow(ncap, keep_rows, e->stream));
  VR_TRY(e->folder.grow(ncap, keep_rows, e->stream));
  VR_TRY(e->index_folder.grow(ncap, keep_rows, e->stream));
  VR_TRY(e->created.grow(ncap, keep_rows, e->stream));
  VR_TRY(e->modified.grow(ncap, keep_rows, e->stream));
  VR_TRY(e->row_slice.grow(ncap, keep_rows, e->stream));
  // DevArray rounds to powers of two; use the smallest capacity everywhere
  ncap = std::min({e->live.cap, e->folder.cap, e->index_folder.cap, e->created.cap,
                   e->modified.cap, e->row_slice.cap, e->corpus.cap / e->dim});
  ncap = ncap / 64 * 64;
  VR_HIP(hipMemsetAsync(e->live.p + keep_rows, 0, static_cast<size_t>(ncap - keep_rows), e->stream));
  e->cap_rows = ncap;
  return 0;
}

static int64_t decode_keys(const uint64_t* keys, int k, int64_t* rows, float* scores) {
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

static int check_engine(vr_engine* e) {
  VR_CHECK(e != nullptr, "null engine");
  VR_HIP(hipSetDevice(e->device));
  return 0;
}

// A host query block goes into the pinned scratch and is read from there by query_image_kernel:
// no hipMemcpy on the latency path. Returns the pointer the kernels should read.
static const float* stage_query(vr_engine* e, const float* q, int nq, int mem) {
  if (mem == VR_MEM_DEVICE) return q;
  memcpy(pin_host<float>(e, kPinQuery), q, sizeof(float) * static_cast<size_t>(nq) * e->dim);
  return pin_dev<float>(e, kPinQuery);
}

// nq*k keys land in the pinned result area at kPinDenseKeys (readable after a stream sync).
// *two_stage is set when the f16 prefilter path ran: the caller must then check the candidate
// count at kPinCandCount after the sync and, if it overflowed, call again with allow_prefilter=false.
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

// A search: takes a lane (waits for one when all are busy), the shared lock, and a fresh view of the index.
// device_input: the caller's buffers were produced on the stream bound to the master (vr_set_stream); the lane's
// stream is ordered behind it.
struct SearchLane {
  vr_engine* m;
  vr_engine* L = nullptr;
  std::shared_lock<std::shared_mutex> lock;
  explicit SearchLane(vr_engine* master) : m(master) {}
  int acquire(bool device_input) {
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
  ~SearchLane() {
    if (!L) return;
    L->drain_into(*m);
    if (lock.owns_lock()) lock.unlock();
    {
      std::lock_guard<std::mutex> g(m->lane_mu);
      m->lanes_free.push_back(L);
    }
    m->lane_cv.notify_one();
  }
};

}  // namespace vr

using namespace vr;

extern "C" {

int vr_abi_version(void) { return VR_ABI_VERSION; }

const char* vr_last_error(void) { return g_last_error.c_str(); }

int vr_engine_create(const vr_config* cfg, vr_engine** out) {
  VR_CHECK(cfg && out, "null argument");
  VR_CHECK(cfg->struct_size == static_cast<int32_t>(sizeof(vr_config)), "vr_config size mismatch");
  VR_CHECK(cfg->dim > 0 && cfg->dim % 16 == 0 && cfg->dim <= kMaxDim, "dim %d must be a multiple of 16 in 16..%d",
           cfg->dim, kMaxDim);
  int n_dev = 0;
  hipError_t err = hipGetDeviceCount(&n_dev);
  VR_CHECK(err == hipSuccess && n_dev > 0,
           "no HIP device available (%s): libvoitta_engine has no CPU fallback",
           err == hipSuccess ? "device count 0" : hipGetErrorString(err));
  VR_CHECK(cfg->device >= 0 && cfg->device < n_dev, "device %d out of range (0..%d)", cfg->device,
           n_dev - 1);
  hipDeviceProp_t prop;
  VR_HIP(hipGetDeviceProperties(&prop, cfg->device));
  VR_CHECK(strncmp(prop.gcnArchName, "gfx950", 6) == 0,
           "device %d is %s; this library carries gfx950 (MI355X) code objects only", cfg->device,
           prop.gcnArchName);
  VR_HIP(hipSetDevice(cfg->device));
  vr_engine* e = new vr_engine();
  e->device = cfg->device;
  e->dim = cfg->dim;
  e->kblocks = cfg->dim / kTileK;
  e->prefilter = (cfg->dim % 32 == 0) && !(cfg->flags & VR_ENGINE_NO_PREFILTER);
  {
    // shadow format of the two-stage search: int8 + row scale where the MFMA tiling allows, else f16;
    // VR_PREFILTER=f16 keeps the f16 shadow (tighter bounds: fewer re-scores on corpora of near-duplicates)
    const char* mode = getenv("VR_PREFILTER");
    e->prefilter8 = e->prefilter && cfg->dim % 64 == 0 && !(mode && strcmp(mode, "f16") == 0);
  }
  // a blocking stream: it orders itself against the legacy null stream, so device buffers
  // produced by a framework on its default stream are safe to hand in without extra events
  if (hipStreamCreateWithFlags(&e->own_stream, hipStreamDefault) != hipSuccess) {
    set_error("hipStreamCreate failed");
    delete e;
    return -1;
  }
  e->stream = e->own_stream;
  if (hipStreamCreateWithFlags(&e->aux_stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming) != hipSuccess) {
    set_error("creating the auxiliary stream failed");
    vr_engine_destroy(e);
    return -1;
  }
  if (hipHostMalloc(&e->pinned, kPinnedBytes, hipHostMallocMapped) != hipSuccess ||
      hipHostGetDevicePointer(&e->pinned_dev, e->pinned, 0) != hipSuccess) {
    set_error("hipHostMalloc (mapped) failed");
    e->pinned = nullptr;
    vr_engine_destroy(e);
    return -1;
  }
  e->pinned_bytes = kPinnedBytes;
  if (const char* lanes = getenv("VR_SEARCH_LANES")) e->lanes_max = std::min(16, std::max(1, atoi(lanes)));
  int64_t init = cfg->initial_rows > 0 ? cfg->initial_rows : 1024;
  if (ensure_rows(e, init) != 0) {
    vr_engine_destroy(e);
    return -1;
  }
  *out = e;
  return 0;
}

void vr_engine_destroy(vr_engine* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  encoder_release(e);
  prof_release(e);
  for (vr_engine* L : e->lanes_all) {  // (a lane holds views of the index, its own resources and scratch)
    if (L->own_stream) (void)hipStreamSynchronize(L->own_stream);
    L->LaneResources::release();
    delete L;
  }
  e->lanes_all.clear();
  e->lanes_free.clear();
  e->IndexTables::release();
  e->IndexTotals::release();
  for (float* p : e->query_rows_free) (void)hipFree(p);
  e->LaneResources::release();
  delete e;
}

int vr_sync(vr_engine* e) {
  VR_TRY(check_engine(e));
  VR_HIP(hipStreamSynchronize(e->stream));
  return 0;
}

void* vr_stream(vr_engine* e) { return e ? static_cast<void*>(e->stream) : nullptr; }

int vr_set_stream(vr_engine* e, void* stream) {
  VR_TRY(check_engine(e));
  std::lock_guard<std::mutex> writer(e->wmu);
  VR_HIP(hipStreamSynchronize(e->stream));
  e->stream = stream ? static_cast<hipStream_t>(stream) : e->own_stream;
  return 0;
}

int vr_encoder_load(vr_engine* e, const vr_bert_desc* desc, const void* const* tensors,
                    int32_t n_tensors, int mem) {
  VR_TRY(check_engine(e));
  VR_CHECK(desc && tensors, "null argument");
  VR_CHECK(mem == VR_MEM_HOST || mem == VR_MEM_DEVICE, "bad mem %d", mem);
  std::lock_guard<std::mutex> writer(e->wmu);
  return encoder_load(e, desc, tensors, n_tensors, mem);
}

int vr_encode(vr_engine* e, const int32_t* ids, const int32_t* offsets, int32_t n_seq, int mem,
              float* out, int out_mem) {
  VR_TRY(check_engine(e));
  VR_CHECK(n_seq >= 0 && (n_seq == 0 || (ids && offsets && out)), "bad arguments");
  VR_CHECK((mem == VR_MEM_HOST || mem == VR_MEM_DEVICE) && (out_mem == VR_MEM_HOST || out_mem == VR_MEM_DEVICE),
           "bad mem");
  std::lock_guard<std::mutex> writer(e->wmu);
  return encoder_encode(e, ids, offsets, n_seq, mem, out, out_mem);
}

int vr_reranker_load(vr_engine* e, const vr_bert_desc* desc, const void* const* tensors, int32_t n_tensors, int mem) {
  VR_TRY(check_engine(e));
  VR_CHECK(desc && tensors, "null argument");
  VR_CHECK(mem == VR_MEM_HOST || mem == VR_MEM_DEVICE, "bad mem %d", mem);
  std::lock_guard<std::mutex> writer(e->wmu);
  return reranker_load(e, desc, tensors, n_tensors, mem);
}

int vr_rerank(vr_engine* e, const int32_t* ids, const int32_t* offsets, const int32_t* seg_b, int32_t n_seq, int mem,
              float* out_logits, int out_mem) {
  VR_CHECK(n_seq >= 0 && (n_seq == 0 || (ids && offsets && out_logits)), "bad arguments");
  // A null seg_b is allowed for a reranker with one token type only; whether the loaded model has one is checked in
  // encoder_rerank, under the writers' mutex. This line runs BEFORE check_engine, so that a null engine with a null
  // seg_b still reports the argument error first, as vr_rerank always has (tests/test_rerank_cpu.py).
  VR_CHECK(n_seq == 0 || seg_b || e, "bad arguments");
  VR_CHECK((mem == VR_MEM_HOST || mem == VR_MEM_DEVICE) && (out_mem == VR_MEM_HOST || out_mem == VR_MEM_DEVICE),
           "bad mem");
  VR_TRY(check_engine(e));
  std::lock_guard<std::mutex> writer(e->wmu);
  return encoder_rerank(e, ids, offsets, seg_b, n_seq, mem, out_logits, out_mem);
}

}  // extern "C"

// vr_rerank_text and vr_rerank_text_unigram: one pipeline, whatever tokenises the pairs
static int rerank_text(vr_engine* e, const vr::Tokenizer* tokenizer, int32_t n_queries, const char* const* queries,
                       const int64_t* query_lens, const int64_t* cand_off, const char* const* passages,
                       const int64_t* passage_lens, int32_t max_len, float* out_logits) {
  VR_CHECK(n_queries >= 0 && (n_queries == 0 || (tokenizer && queries && query_lens && cand_off)), "bad arguments");
  VR_CHECK(max_len >= 3 && max_len <= 8192, "max_len %d", max_len);
  if (n_queries == 0) return check_engine(e);
  VR_CHECK(cand_off[0] == 0, "cand_off[0] = %lld, must be 0", static_cast<long long>(cand_off[0]));
  for (int q = 0; q < n_queries; ++q) {
    VR_CHECK(queries[q] && query_lens[q] >= 0, "query %d: null text or negative length", q);
    VR_CHECK(cand_off[q + 1] >= cand_off[q], "cand_off decreases at query %d", q);
  }
  const int64_t n = cand_off[n_queries];
  VR_CHECK(n <= INT32_MAX, "%lld pairs", static_cast<long long>(n));
  VR_CHECK(n == 0 || (passages && passage_lens && out_logits), "bad arguments");
  for (int64_t i = 0; i < n; ++i)
    VR_CHECK(passages[i] && passage_lens[i] >= 0, "passage %lld: null text or negative length", static_cast<long long>(i));
  VR_TRY(check_engine(e));
  if (n == 0) return 0;
  {
    std::lock_guard<std::mutex> writer(e->wmu);
    VR_CHECK(reranker_loaded(e), "no reranker loaded (vr_reranker_load)");
  }
  // host threads: the pairs' ids (each question tokenised once), then one forward pass over all of them
  std::vector<const char*> a(static_cast<size_t>(n));
  std::vector<int64_t> a_len(static_cast<size_t>(n));
  for (int q = 0; q < n_queries; ++q)
    for (int64_t i = cand_off[q]; i < cand_off[q + 1]; ++i) {
      a[static_cast<size_t>(i)] = queries[q];
      a_len[static_cast<size_t>(i)] = query_lens[q];
    }
  std::vector<int64_t> off(static_cast<size_t>(n) + 1);
  // room for the ids: a piece consumes at least a byte of text (n * max_len ids would be megabytes of zeros to write
  // at max_len = 8192); a normaliser that expands its input can need more, and then the tokenizer says how many
  size_t room = 0;
  for (int64_t i = 0; i < n; ++i)
    room += static_cast<size_t>(std::min<int64_t>(a_len[static_cast<size_t>(i)] + passage_lens[i] + 4, max_len));
  std::vector<int32_t> seg(static_cast<size_t>(n)), ids(room);
  int64_t needed = 0;
  int rc = tokenizer->encode_pairs(a.data(), a_len.data(), passages, passage_lens, n, max_len, off.data(), ids.data(),
                                   seg.data(), static_cast<int64_t>(ids.size()), &needed);
  if (rc == -2) {
    ids.resize(static_cast<size_t>(needed));
    rc = tokenizer->encode_pairs(a.data(), a_len.data(), passages, passage_lens, n, max_len, off.data(), ids.data(),
                                 seg.data(), static_cast<int64_t>(ids.size()), &needed);
    if (rc == 0) vr::set_error("%s", "");  // (the first attempt's "buffer holds ..." is not this call's error)
  }
  VR_TRY(rc);
  VR_CHECK(needed <= INT32_MAX, "%lld tokens", static_cast<long long>(needed));
  std::vector<int32_t> off32(static_cast<size_t>(n) + 1);
  for (int64_t i = 0; i <= n; ++i) off32[static_cast<size_t>(i)] = static_cast<int32_t>(off[static_cast<size_t>(i)]);
  std::lock_guard<std::mutex> writer(e->wmu);
  return encoder_rerank(e, ids.data(), off32.data(), seg.data(), static_cast<int>(n), VR_MEM_HOST, out_logits, VR_MEM_HOST);
}

extern "C" {

int vr_rerank_text(vr_engine* e, const vr_wordpiece* tokenizer, int32_t n_queries, const char* const* queries,
                   const int64_t* query_lens, const int64_t* cand_off, const char* const* passages,
                   const int64_t* passage_lens, int32_t max_len, float* out_logits) {
  return rerank_text(e, vr::as_tokenizer(tokenizer), n_queries, queries, query_lens, cand_off, passages, passage_lens,
                     max_len, out_logits);
}

int vr_rerank_text_unigram(vr_engine* e, const vr_unigram* tokenizer, int32_t n_queries, const char* const* queries,
                           const int64_t* query_lens, const int64_t* cand_off, const char* const* passages,
                           const int64_t* passage_lens, int32_t max_len, float* out_logits) {
  VR_CHECK(max_len >= 4, "max_len %d cannot hold <s> and three </s>", max_len);
  return rerank_text(e, vr::as_tokenizer(tokenizer), n_queries, queries, query_lens, cand_off, passages, passage_lens,
                     max_len, out_logits);
}

}  // extern "C"

// Body of vr_upsert, also the last stage of vr_index_batch. Caller holds e->wmu and the exclusive lock.
// sp_cnt_dev (device memory, mem == VR_MEM_DEVICE only): when given, the sparse rows are in the
// padded layout bm25_tf_kernel writes — row r = idx/val[sp_off[r] .. sp_off[r] + sp_cnt_dev[r]).
static int upsert_locked(vr_engine* e, int64_t n, int mem, const float* dense, const int64_t* sp_off,
                         const int32_t* sp_idx, const float* sp_val, const int32_t* sp_cnt_dev,
                         const int32_t* folder_id, const int32_t* index_folder_id,
                         const int64_t* created, const int64_t* modified, int64_t* out_first_row) {
  const int64_t first = e->n_rows;
  if (out_first_row) *out_first_row = first;
  if (n == 0) return 0;
  VR_CHECK(dense != nullptr, "null dense");
  VR_CHECK(first + n < (int64_t{1} << 32), "row id space exhausted");
  VR_TRY(ensure_rows(e, first + n));

  const float* x_dev = dense;
  if (mem == VR_MEM_HOST) {
    VR_TRY(e->stage_dense.grow(n * e->dim, 0, e->stream));
    VR_HIP(hipMemcpyAsync(e->stage_dense.p, dense, sizeof(float) * static_cast<size_t>(n * e->dim),
                          hipMemcpyHostToDevice, e->stream));
    x_dev = e->stage_dense.p;
  }
  VR_TRY(dense_store_rows(e, x_dev, n, first));
  // shadow of the rows just stored (no-op without prefilter); the int8 shadow is re-centred — all of it rebuilt —
  // whenever the collection has doubled since its centre was last computed
  e->n_rows = first + n;  // (prefilter_recentre works on [0, n_rows); the count is set again below)
  {
    // re-centre when the collection has doubled since a re-centring was last attempted (centre_checked_rows, not centre_rows:
    // with centring switched off or a non-finite centre the latter stays 0 and every upsert would rebuild the whole shadow)
    const int rc = (e->prefilter8 && first + n >= 1024 && first + n >= 2 * std::max(e->centre_rows, e->centre_checked_rows))
                       ? prefilter_recentre(e)
                       : prefilter_store_rows(e, n, first);
    e->n_rows = first;  // (also on failure: rows whose payload columns were never written must not become visible)
    if (rc != 0) return rc;
  }

  // payload columns are always host arrays (they come from Python metadata)
  if (folder_id) {
    for (int64_t i = 0; i < n; ++i) {
      VR_CHECK(folder_id[i] >= 0, "negative folder id");
      e->max_folder_id = std::max(e->max_folder_id, folder_id[i]);
    }
    VR_HIP(hipMemcpyAsync(e->folder.p + first, folder_id, sizeof(int32_t) * static_cast<size_t>(n),
                          hipMemcpyHostToDevice, e->stream));
  } else {
    e->max_folder_id = std::max(e->max_folder_id, 0);
    VR_HIP(hipMemsetAsync(e->folder.p + first, 0, sizeof(int32_t) * static_cast<size_t>(n), e->stream));
  }
  if (index_folder_id) {
    for (int64_t i = 0; i < n; ++i) {
      VR_CHECK(index_folder_id[i] >= 0, "negative index-folder id");
      e->max_index_folder_id = std::max(e->max_index_folder_id, index_folder_id[i]);
    }
    VR_HIP(hipMemcpyAsync(e->index_folder.p + first, index_folder_id,
                          sizeof(int32_t) * static_cast<size_t>(n), hipMemcpyHostToDevice, e->stream));
  } else {
    e->max_index_folder_id = std::max(e->max_index_folder_id, 0);
    VR_HIP(hipMemsetAsync(e->index_folder.p + first, 0, sizeof(int32_t) * static_cast<size_t>(n),
                          e->stream));
  }
  const unsigned fill_blocks = static_cast<unsigned>((n + 255) / 256);
  if (created)
    VR_HIP(hipMemcpyAsync(e->created.p + first, created, sizeof(int64_t) * static_cast<size_t>(n),
                          hipMemcpyHostToDevice, e->stream));
  else
    hipLaunchKernelGGL(fill_i64_kernel, dim3(fill_blocks), dim3(256), 0, e->stream,
                       e->created.p + first, static_cast<int64_t>(VR_TS_ABSENT), n);
  if (modified)
    VR_HIP(hipMemcpyAsync(e->modified.p + first, modified, sizeof(int64_t) * static_cast<size_t>(n),
                          hipMemcpyHostToDevice, e->stream));
  else
    hipLaunchKernelGGL(fill_i64_kernel, dim3(fill_blocks), dim3(256), 0, e->stream,
                       e->modified.p + first, static_cast<int64_t>(VR_TS_ABSENT), n);
  VR_HIP(hipMemsetAsync(e->live.p + first, 1, static_cast<size_t>(n), e->stream));
  VR_HIP(hipMemsetAsync(e->row_slice.p + first, 0xFF, sizeof(int32_t) * static_cast<size_t>(n),
                        e->stream));

  if (sp_off) {
    VR_CHECK(sp_idx && sp_val, "sparse offsets without indices/values");
    if (mem == VR_MEM_HOST) {
      const int64_t nnz = sp_off[n];
      VR_CHECK(sp_off[0] == 0 && nnz >= 0, "bad sparse offsets");
      // sort every row by token id (Qdrant sorts sparse vectors by index on ingestion [EXT])
      std::vector<int32_t> idx(sp_idx, sp_idx + nnz);
      std::vector<float> val(sp_val, sp_val + nnz);
      std::vector<std::pair<int32_t, float>> tmp;
      for (int64_t r = 0; r < n; ++r) {
        int64_t b = sp_off[r], en = sp_off[r + 1];
        VR_CHECK(en >= b, "sparse offsets must be non-decreasing");
        bool sorted = true;
        for (int64_t j = b + 1; j < en; ++j) sorted = sorted && idx[static_cast<size_t>(j - 1)] < idx[static_cast<size_t>(j)];
        for (int64_t j = b; j < en; ++j) VR_CHECK(idx[static_cast<size_t>(j)] >= 0, "negative token id");
        if (sorted) continue;
        tmp.clear();
        for (int64_t j = b; j < en; ++j) tmp.emplace_back(idx[static_cast<size_t>(j)], val[static_cast<size_t>(j)]);
        std::stable_sort(tmp.begin(), tmp.end(), [](const auto& a, const auto& c) { return a.first < c.first; });
        for (size_t j = 1; j < tmp.size(); ++j)
          if (tmp[j - 1].first == tmp[j].first) e->sp_has_dups = true;  // a term listed twice (invert.hip)
        for (int64_t j = b; j < en; ++j) {
          idx[static_cast<size_t>(j)] = tmp[static_cast<size_t>(j - b)].first;
          val[static_cast<size_t>(j)] = tmp[static_cast<size_t>(j - b)].second;
        }
      }
      VR_TRY(e->stage_off.grow(n + 1, 0, e->stream));
      VR_TRY(e->stage_idx.grow(std::max<int64_t>(nnz, 1), 0, e->stream));
      VR_TRY(e->stage_val.grow(std::max<int64_t>(nnz, 1), 0, e->stream));
      VR_HIP(hipMemcpyAsync(e->stage_off.p, sp_off, sizeof(int64_t) * static_cast<size_t>(n + 1),
                            hipMemcpyHostToDevice, e->stream));
      if (nnz > 0) {
        VR_HIP(hipMemcpyAsync(e->stage_idx.p, idx.data(), sizeof(int32_t) * static_cast<size_t>(nnz),
                              hipMemcpyHostToDevice, e->stream));
        VR_HIP(hipMemcpyAsync(e->stage_val.p, val.data(), sizeof(float) * static_cast<size_t>(nnz),
                              hipMemcpyHostToDevice, e->stream));
      }
      VR_HIP(hipStreamSynchronize(e->stream));  // idx/val vectors die at scope end
      std::vector<int32_t> cnt(static_cast<size_t>(n));
      for (int64_t r = 0; r < n; ++r) cnt[static_cast<size_t>(r)] = static_cast<int32_t>(sp_off[r + 1] - sp_off[r]);
      VR_TRY(sparse_append(e, n, first, cnt.data(), e->stage_off.p, nullptr, e->stage_idx.p, e->stage_val.p));
    } else if (sp_cnt_dev) {
      std::vector<int32_t> cnt(static_cast<size_t>(n));
      VR_HIP(hipMemcpyAsync(cnt.data(), sp_cnt_dev, sizeof(int32_t) * static_cast<size_t>(n),
                            hipMemcpyDeviceToHost, e->stream));
      VR_HIP(hipStreamSynchronize(e->stream));
      VR_TRY(sparse_append(e, n, first, cnt.data(), sp_off, sp_cnt_dev, sp_idx, sp_val));
    } else {
      std::vector<int64_t> off_host(static_cast<size_t>(n + 1));
      unsigned long long dups = 0;
      VR_TRY(inv_note_csr_dups(e, sp_off, sp_idx, n, &dups));
      VR_HIP(hipMemcpyAsync(off_host.data(), sp_off, sizeof(int64_t) * static_cast<size_t>(n + 1),
                            hipMemcpyDeviceToHost, e->stream));
      VR_HIP(hipStreamSynchronize(e->stream));
      if (dups) e->sp_has_dups = true;
      VR_CHECK(off_host[0] == 0, "sparse offsets must start at 0");
      std::vector<int32_t> cnt(static_cast<size_t>(n));
      for (int64_t r = 0; r < n; ++r) {
        VR_CHECK(off_host[static_cast<size_t>(r) + 1] >= off_host[static_cast<size_t>(r)], "sparse offsets must be non-decreasing");
        cnt[static_cast<size_t>(r)] = static_cast<int32_t>(off_host[static_cast<size_t>(r) + 1] - off_host[static_cast<size_t>(r)]);
      }
      VR_TRY(sparse_append(e, n, first, cnt.data(), sp_off, nullptr, sp_idx, sp_val));
    }
  }
  VR_HIP(hipGetLastError());
  // caller-owned host arrays must not be read after we return
  if (mem == VR_MEM_HOST || folder_id || index_folder_id || created || modified)
    VR_HIP(hipStreamSynchronize(e->stream));
  e->n_rows += n;
  e->n_live += n;
  return 0;
}

extern "C" {

int vr_upsert(vr_engine* e, int64_t n, int mem, const float* dense, const int64_t* sp_off,
              const int32_t* sp_idx, const float* sp_val, const int32_t* folder_id,
              const int32_t* index_folder_id, const int64_t* created, const int64_t* modified,
              int64_t* out_first_row) {
  VR_TRY(check_engine(e));
  VR_CHECK(n >= 0, "negative row count");
  VR_CHECK(mem == VR_MEM_HOST || mem == VR_MEM_DEVICE, "bad mem %d", mem);
  std::lock_guard<std::mutex> writer(e->wmu);
  PublishLock publish(e);  // (the append itself: a fraction of a millisecond per thousand rows)
  return upsert_locked(e, n, mem, dense, sp_off, sp_idx, sp_val, nullptr, folder_id, index_folder_id,
                       created, modified, out_first_row);
}

int vr_index_batch(vr_engine* e, int64_t n, int mem, const int32_t* wp_ids, const int32_t* wp_off,
                   const int32_t* bm_ids, const int64_t* bm_off, double k, double b, double avg_len,
                   const int32_t* folder_id, const int32_t* index_folder_id, const int64_t* created,
                   const int64_t* modified, int64_t* out_first_row) {
  VR_TRY(check_engine(e));
  VR_CHECK(n >= 0 && (n == 0 || (wp_ids && wp_off)), "bad arguments");
  VR_CHECK(mem == VR_MEM_HOST || mem == VR_MEM_DEVICE, "bad mem %d", mem);
  VR_CHECK((bm_ids == nullptr) == (bm_off == nullptr), "bm_ids and bm_off go together");
  std::lock_guard<std::mutex> writer(e->wmu);
  if (n == 0) {
    if (out_first_row) *out_first_row = e->n_rows;
    return 0;
  }
  // 1. sparse side first: it is microseconds of work and its per-document counts are the only
  //    thing the host has to wait for (slice widths); the long encode is queued behind it.
  const int64_t* bm_off_dev = nullptr;
  if (bm_off) {
    int64_t n_tokens = 0;
    const int32_t* bm_ids_dev = bm_ids;
    bm_off_dev = bm_off;
    if (mem == VR_MEM_HOST) {
      VR_CHECK(bm_off[0] == 0, "token offsets must start at 0");
      n_tokens = bm_off[n];
      VR_TRY(e->stage_off.grow(n + 1, 0, e->stream));
      VR_TRY(e->stage_idx.grow(std::max<int64_t>(n_tokens, 1), 0, e->stream));
      VR_HIP(hipMemcpyAsync(e->stage_off.p, bm_off, sizeof(int64_t) * static_cast<size_t>(n + 1),
                            hipMemcpyHostToDevice, e->stream));
      if (n_tokens > 0)
        VR_HIP(hipMemcpyAsync(e->stage_idx.p, bm_ids, sizeof(int32_t) * static_cast<size_t>(n_tokens),
                              hipMemcpyHostToDevice, e->stream));
      bm_off_dev = e->stage_off.p;
      bm_ids_dev = e->stage_idx.p;
    } else {
      VR_HIP(hipMemcpyAsync(&n_tokens, bm_off + n, sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
      VR_HIP(hipStreamSynchronize(e->stream));
    }
    const int64_t cap = std::max<int64_t>(n_tokens, 1);
    VR_TRY(e->bm_cnt.grow(n, 0, e->stream));
    VR_TRY(e->bm_idx.grow(cap, 0, e->stream));
    VR_TRY(e->bm_val.grow(cap, 0, e->stream));
    VR_TRY(bm25_tf(e, bm_off_dev, bm_ids_dev, n, n_tokens, k, b, avg_len, e->bm_cnt.p, e->bm_idx.p,
                   nullptr, e->bm_val.p));
  }
  // 2. dense encode into engine-owned rows
  VR_CHECK(encoder_hidden(e) == e->dim, "encoder width %d != store dimension %d", encoder_hidden(e), e->dim);
  VR_TRY(e->enc_out.grow(n * e->dim, 0, e->stream));
  VR_TRY(encoder_encode(e, wp_ids, wp_off, static_cast<int>(n), mem, e->enc_out.p, VR_MEM_DEVICE));
  // 3. store: the only part searches wait for (they ran beside the encode)
  PublishLock publish(e);
  return upsert_locked(e, n, VR_MEM_DEVICE, e->enc_out.p, bm_off_dev, bm_off ? e->bm_idx.p : nullptr,
                       bm_off ? e->bm_val.p : nullptr, bm_off ? e->bm_cnt.p : nullptr, folder_id,
                       index_folder_id, created, modified, out_first_row);
}

int vr_delete_rows(vr_engine* e, const int64_t* rows, int64_t n) {
  VR_TRY(check_engine(e));
  VR_CHECK(n >= 0 && (n == 0 || rows), "bad arguments");
  if (n == 0) return 0;
  std::lock_guard<std::mutex> writer(e->wmu);
  PublishLock publish(e);
  std::vector<int64_t> uniq(rows, rows + n);
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  const int64_t m = static_cast<int64_t>(uniq.size());
  VR_TRY(e->stage_i64a.grow(m, 0, e->stream));
  VR_HIP(hipMemcpyAsync(e->stage_i64a.p, uniq.data(), sizeof(int64_t) * static_cast<size_t>(m),
                        hipMemcpyHostToDevice, e->stream));
  int64_t deleted = 0, sparse_deleted = 0;
  VR_TRY(sparse_delete_rows(e, e->stage_i64a.p, m, &deleted, &sparse_deleted));
  e->n_live -= deleted;
  e->n_sparse_points -= sparse_deleted;
  return 0;
}

int vr_stats(vr_engine* e, int32_t which, int64_t* out) {
  VR_CHECK(e != nullptr && out != nullptr, "null argument");
  switch (which) {
    case VR_STAT_TWO_STAGE: *out = e->stat_two_stage.load(); break;
    case VR_STAT_FALLBACK: *out = e->stat_fallback.load(); break;
    case VR_STAT_LAST_CANDIDATES: *out = e->stat_last_candidates.load(); break;
    case VR_STAT_BATCHED: *out = e->stat_batched.load(); break;
    case VR_STAT_BATCH_FALLBACK: *out = e->stat_batch_fallback.load(); break;
    case VR_STAT_BATCH_CANDIDATES: *out = e->stat_batch_cands.load(); break;
    case VR_STAT_GENERATION: *out = e->generation.load(); break;
    case VR_STAT_SPARSE_GROUPED: *out = e->stat_sparse_grouped.load(); break;
    case VR_STAT_SPARSE_GROUP_REDO: *out = e->stat_sparse_group_redo.load(); break;
    case VR_STAT_SPARSE_GROUP_CANDIDATES: *out = e->stat_sparse_group_cands.load(); break;
    default: set_error("unknown statistic %d", which); return -1;
  }
  return 0;
}

int vr_count(vr_engine* e, int64_t* n_rows, int64_t* n_live) {
  VR_CHECK(e != nullptr, "null engine");
  std::shared_lock<std::shared_mutex> view(e->rw);
  if (n_rows) *n_rows = e->n_rows;
  if (n_live) *n_live = e->n_live;
  return 0;
}

int vr_get_dense(vr_engine* e, const int64_t* rows, int64_t n, float* out) {
  VR_TRY(check_engine(e));
  VR_CHECK(n >= 0 && (n == 0 || (rows && out)), "bad arguments");
  if (n == 0) return 0;
  std::lock_guard<std::mutex> writer(e->wmu);  // (the master's staging arrays)
  std::shared_lock<std::shared_mutex> view(e->rw);
  for (int64_t i = 0; i < n; ++i)
    VR_CHECK(rows[i] >= 0 && rows[i] < e->n_rows, "row %lld out of range", static_cast<long long>(rows[i]));
  VR_TRY(e->stage_i64a.grow(n, 0, e->stream));
  VR_TRY(e->stage_dense.grow(n * e->dim, 0, e->stream));
  VR_HIP(hipMemcpyAsync(e->stage_i64a.p, rows, sizeof(int64_t) * static_cast<size_t>(n),
                        hipMemcpyHostToDevice, e->stream));
  VR_TRY(dense_read_rows(e, e->stage_i64a.p, n, e->stage_dense.p));
  VR_HIP(hipMemcpyAsync(out, e->stage_dense.p, sizeof(float) * static_cast<size_t>(n * e->dim),
                        hipMemcpyDeviceToHost, e->stream));
  VR_HIP(hipStreamSynchronize(e->stream));
  return 0;
}

int vr_sparse_stats(vr_engine* e, const int32_t* ids, int32_t n, int32_t* out_df, int64_t* out_n_points) {
  VR_TRY(check_engine(e));
  std::lock_guard<std::mutex> writer(e->wmu);
  std::shared_lock<std::shared_mutex> view(e->rw);
  if (out_n_points) *out_n_points = e->n_sparse_points;
  if (n > 0) {
    VR_CHECK(ids && out_df, "null argument");
    if (e->df_cap == 0) {
      for (int i = 0; i < n; ++i) out_df[i] = 0;
    } else {
      VR_TRY(sparse_lookup_df(e, ids, n, out_df));
    }
  }
  return 0;
}

}  // extern "C"

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
  if (fork) VR_HIP(hipEventRecord(e->ev_fork, e->stream));  // after the mask, before the dense leg
  VR_TRY(search_dense_block(e, q_dev, 1, k, mask, true, &two_stage));
  if (fork) {
    // queued after the dense leg (whose scan is already running by now), executed beside it
    VR_HIP(hipStreamWaitEvent(e->aux_stream, e->ev_fork, 0));
    hipStream_t main_stream = e->stream;
    e->stream = e->aux_stream;
    const int rc = search_sparse_block(e, q_idx, q_val, nnz, k, mask, weights_given);
    e->stream = main_stream;
    if (rc != 0) return rc;
    VR_HIP(hipEventRecord(e->ev_join, e->aux_stream));
    VR_HIP(hipStreamWaitEvent(e->stream, e->ev_join, 0));
  } else if (have_sparse) {
    VR_TRY(search_sparse_block(e, q_idx, q_val, nnz, k, mask, weights_given));
  }
  VR_HIP(hipStreamSynchronize(e->stream));
  e->stat_two_stage += two_stage;
  if (two_stage) e->stat_last_candidates.store(*pin_host<int32_t>(e, kPinCandCount));
  if (two_stage && *pin_host<int32_t>(e, kPinCandCount) > kMaxCandidates) {
    ++e->stat_fallback;
    VR_TRY(search_dense_block(e, q_dev, 1, k, mask, false));  // candidate overflow: one-stage exact scan
    VR_HIP(hipStreamSynchronize(e->stream));
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
    e->stat_two_stage += two_stage;
    if (two_stage) e->stat_last_candidates.store(*pin_host<int32_t>(e, kPinCandCount));
    if (two_stage && *pin_host<int32_t>(e, kPinCandCount) > kMaxCandidates) {
      // more candidates than the re-score budget (near-duplicate corpus): one-stage exact scan
      ++e->stat_fallback;
      VR_TRY(search_dense_block(e, q_dev, nb, k, mask, false));
      VR_HIP(hipStreamSynchronize(e->stream));
    }
    if (keys_host) memcpy(keys_host + static_cast<size_t>(at) * k, pinned_keys, row_bytes * static_cast<size_t>(nb));
    if (keys_dev) {
      VR_HIP(hipMemcpyAsync(keys_dev + static_cast<size_t>(at) * k, pinned_keys, row_bytes * static_cast<size_t>(nb),
                            hipMemcpyHostToDevice, e->stream));
      VR_HIP(hipStreamSynchronize(e->stream));  // the pinned area is reused by the next block
    }
    return 0;
  };
  if (batch_usable(e, nq, k)) {
    // many queries at once: integer GEMM over the int8 shadow + exact re-score (batch.hip), 1024 queries per round
    constexpr int kRound = 1024;
    std::vector<int32_t> over(static_cast<size_t>(std::min(nq, kRound)));
    for (int q0 = 0; q0 < nq; q0 += kRound) {
      const int nb = std::min(kRound, nq - q0);
      const float* q_dev = q + static_cast<int64_t>(q0) * e->dim;
      if (mem == VR_MEM_HOST) {
        VR_TRY(e->bq_stage.grow(static_cast<int64_t>(nb) * e->dim, 0, e->stream));
        VR_HIP(hipMemcpyAsync(e->bq_stage.p, q_dev, sizeof(float) * static_cast<size_t>(nb) * e->dim, hipMemcpyHostToDevice,
                              e->stream));
        q_dev = e->bq_stage.p;
      }
      const uint64_t* round_keys = nullptr;
      const int32_t* over_dev = nullptr;
      VR_TRY(batch_search(e, q_dev, nb, k, mask, &round_keys, &over_dev));
      if (keys_host)
        VR_HIP(hipMemcpyAsync(keys_host + static_cast<size_t>(q0) * k, round_keys, row_bytes * static_cast<size_t>(nb),
                              hipMemcpyDeviceToHost, e->stream));
      if (keys_dev)
        VR_HIP(hipMemcpyAsync(keys_dev + static_cast<size_t>(q0) * k, round_keys, row_bytes * static_cast<size_t>(nb),
                              hipMemcpyDeviceToDevice, e->stream));
      VR_HIP(hipMemcpyAsync(over.data(), over_dev, sizeof(int32_t) * static_cast<size_t>(nb), hipMemcpyDeviceToHost, e->stream));
      VR_HIP(hipStreamSynchronize(e->stream));
      e->stat_batched += nb;
      for (int i = 0; i < nb; ++i) e->stat_batch_cands += std::min<int32_t>(over[static_cast<size_t>(i)], kBatchCand);
      for (int i = 0; i < nb; ++i)
        if (over[static_cast<size_t>(i)] > kBatchCand) {  // candidate budget exceeded: this query alone, through the exact scans
          ++e->stat_batch_fallback;
          VR_TRY(run_block(q + static_cast<int64_t>(q0 + i) * e->dim, 1, q0 + i));
        }
    }
    return 0;
  }
  for (int q0 = 0; q0 < nq; q0 += kQueryBlock)
    VR_TRY(run_block(q + static_cast<int64_t>(q0) * e->dim, std::min(kQueryBlock, nq - q0), q0));
  return 0;
}

extern "C" {

int vr_search_dense(vr_engine* e, const float* q, int32_t nq, int mem, int32_t k,
                    const vr_filter* filter, int64_t* rows, float* scores, int32_t* counts) {
  VR_TRY(check_engine(e));
  VR_CHECK(q && rows && scores && nq >= 1, "bad arguments");
  VR_CHECK(k >= 1 && k <= kMaxK, "k = %d not in 1..%d", k, kMaxK);
  VR_CHECK(mem == VR_MEM_HOST || mem == VR_MEM_DEVICE, "bad mem %d", mem);
  SearchLane lane(e);
  VR_TRY(lane.acquire(mem == VR_MEM_DEVICE));
  std::vector<uint64_t> keys(static_cast<size_t>(nq) * k);
  VR_TRY(search_dense_keys_locked(lane.L, q, nq, mem, k, filter, keys.data(), nullptr));
  for (int i = 0; i < nq; ++i) {
    const int64_t c = decode_keys(keys.data() + static_cast<size_t>(i) * k, k, rows + static_cast<int64_t>(i) * k,
                                  scores + static_cast<int64_t>(i) * k);
    if (counts) counts[i] = static_cast<int32_t>(c);
  }
  return 0;
}

int vr_search_dense_keys(vr_engine* e, const float* q, int32_t nq, int mem, int32_t k, const vr_filter* filter,
                         uint64_t* keys, int keys_mem) {
  VR_TRY(check_engine(e));
  VR_CHECK(q && keys && nq >= 1, "bad arguments");
  VR_CHECK(k >= 1 && k <= kMaxK, "k = %d not in 1..%d", k, kMaxK);
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
  VR_CHECK(k >= 1 && k <= kMaxK, "k = %d not in 1..%d", k, kMaxK);
  SearchLane lane(e);
  VR_TRY(lane.acquire(false));
  vr_engine* m = e;
  e = lane.L;  // everything below runs on the lane: its stream, its scratch, its view of the index
  (void)m;
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
  VR_CHECK(limit >= 1 && limit * 3 <= kMaxK, "limit = %d not in 1..%d", limit, kMaxK / 3);
  VR_CHECK(fusion == VR_FUSION_MINMAX || fusion == VR_FUSION_RRF, "unknown fusion %d", fusion);
  VR_CHECK(mem == VR_MEM_HOST || mem == VR_MEM_DEVICE, "bad mem %d", mem);
  SearchLane lane(e);
  VR_TRY(lane.acquire(mem == VR_MEM_DEVICE));
  e = lane.L;  // everything below runs on the lane: its stream, its scratch, its view of the index
  *out_count = 0;
  if (e->n_rows == 0) return 0;
  const int k = limit * 3;  // prefetch_limit, vector_store.py:636
  const uint8_t* mask = nullptr;
  VR_TRY(filter_build_mask(e, filter, &mask));
  bool have_sparse = false;
  VR_TRY(hybrid_one_query(e, q, mem, q_idx, q_val, nnz, k, false, mask, &have_sparse));
  int64_t d_rows[kMaxK], s_rows[kMaxK];
  float d_scores[kMaxK], s_scores[kMaxK];
  int nd = static_cast<int>(decode_keys(pin_host<uint64_t>(e, kPinDenseKeys), k, d_rows, d_scores));
  int ns = have_sparse ? static_cast<int>(decode_keys(pin_host<uint64_t>(e, kPinSparseKeys), k, s_rows, s_scores)) : 0;
  if (fusion == VR_FUSION_MINMAX)
    return fuse_minmax(d_rows, d_scores, nd, s_rows, s_scores, ns, limit, sparse_weight, 1, out_rows,
                       out_scores, out_from_dense, out_count);
  return fuse_rrf(d_rows, nd, s_rows, ns, limit, sparse_weight, out_rows, out_scores, out_from_dense,
                  out_count);
}

int vr_compact(vr_engine* e, int64_t* new_row_of_old, int64_t* n_rows_after) {
  VR_TRY(check_engine(e));
  std::lock_guard<std::mutex> writer(e->wmu);  // (engine_compact takes the exclusive lock itself, for the swap only)
  return engine_compact(e, new_row_of_old, n_rows_after);
}

int vr_save(vr_engine* e, const char* path) {
  VR_TRY(check_engine(e));
  VR_CHECK(path && *path, "null path");
  std::lock_guard<std::mutex> writer(e->wmu);
  std::shared_lock<std::shared_mutex> view(e->rw);
  return engine_save(e, path);
}

int vr_load(vr_engine* e, const char* path) {
  VR_TRY(check_engine(e));
  VR_CHECK(path && *path, "null path");
  std::lock_guard<std::mutex> writer(e->wmu);
  PublishLock publish(e);
  const int rc = engine_load(e, path);
  if (rc == 0) e->generation.fetch_add(1);
  return rc;
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

}  // extern "C"

// ---- many sparse / hybrid queries per call (BASELINE configs[4]: 1k batched hybrid queries) ------------------------

namespace {

// The sparse queries of a batch as the engine wants them: per query the terms in ascending id order, a repeated id
// keeping its first value (what sparse_run does for one query; Qdrant sorts sparse vectors by index [EXT]).
struct SparseBatch {
  std::vector<int32_t> off;    // nq + 1: ranges of the queries the batch kernel serves (others: empty range)
  std::vector<int32_t> ids;
  std::vector<float> vals;
  std::vector<int32_t> alone;  // queries it cannot serve (more than kInvMaxTerms distinct terms): one by one
};

int prepare_sparse_batch(const int64_t* q_off, const int32_t* q_idx, const float* q_val, int nq, bool batchable,
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
int sparse_batch_launch(vr_engine* e, const SparseBatch& b, int nq, int k, bool weights_given, const uint8_t* mask,
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

// After the stream of sparse_batch_launch has been synchronised: the grouped scan gives up the queries whose candidate
// regions overflowed (invert.hip) — those are repeated on the per-query kernels, whose answer does not depend on any
// budget, and their rows of keys_host replaced. Runs on e->stream and waits for it.
int sparse_batch_redo_if_overflowed(vr_engine* e, const SparseBatch& b, int nq, int k, bool weights_given, const uint8_t* mask,
                                    uint64_t* keys_host) {
  if (*pin_host<int32_t>(e, kPinSparseOverflow) == 0 || !e->sq_overflow_q) return 0;
  std::vector<int32_t> flagged(static_cast<size_t>(nq));
  VR_HIP(hipMemcpyAsync(flagged.data(), e->sq_overflow_q, sizeof(int32_t) * static_cast<size_t>(nq), hipMemcpyDeviceToHost, e->stream));
  VR_HIP(hipStreamSynchronize(e->stream));
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
int sparse_batch_stragglers(vr_engine* e, const SparseBatch& b, const int64_t* q_off, const int32_t* q_idx, const float* q_val,
                            int k, bool weights_given, const uint8_t* mask, uint64_t* keys_host) {
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
int search_sparse_keys_locked(vr_engine* e, const int64_t* q_off, const int32_t* q_idx, const float* q_val, int nq, int k,
                              bool weights_given, const uint8_t* mask, uint64_t* keys_host) {
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
int hybrid_keys_locked(vr_engine* e, const float* q, int nq, int mem, const int64_t* sq_off, const int32_t* sq_idx,
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
    VR_CHECK(sq_idx && sq_val, "null sparse queries");
    VR_TRY(prepare_sparse_batch(sq_off, sq_idx, sq_val, nq, k <= kFusedMaxK && inv_usable(e, 1), &b));
    VR_HIP(hipEventRecord(e->ev_fork, e->stream));  // after the mask
    VR_HIP(hipStreamWaitEvent(e->aux_stream, e->ev_fork, 0));
    hipStream_t main_stream = e->stream;
    e->stream = e->aux_stream;
    int rc = sparse_batch_launch(e, b, nq, k, weights_given, mask);
    if (rc == 0 && hipMemcpyAsync(sparse_host, e->sq_keys.p, bytes, hipMemcpyDeviceToHost, e->stream) != hipSuccess) {
      set_error("copying the sparse keys failed");
      rc = -1;
    }
    e->stream = main_stream;
    if (rc != 0) return rc;
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

// The classes of a filtered batch: the distinct entries of `filters` its queries name (and "no filter"), numbered in
// order of first appearance. Everything is validated here, before any device work.
struct QueryClasses {
  std::vector<int32_t> of;               // per query: its class
  std::vector<const vr_filter*> filter;  // per class: its filter (nullptr: none)
};

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
int64_t class_plane_budget() {
  static const int64_t mib = getenv("VR_CLASS_PLANE_MIB") ? std::max(0, atoi(getenv("VR_CLASS_PLANE_MIB"))) : 256;
  return mib << 20;
}

// Both legs of a filtered batch. Query i asks for its ks[i] best keys under its class's filter; they go to row i of
// dense_host / sparse_host ([nq][kstride], zero padded; sparse_host null: dense only). q: host array, nq x D.
//   dense   the queries of k <= kFusedMaxK share the batched scan (batch.hip), which reads each query's class plane; the
//           queries sorted by class, so that a 128-query block column mostly sees one class. Classes go in slices whose
//           planes fit class_plane_budget(). A slice too small to batch, the larger k and the queries over their candidate
//           budget run class by class on the byte mask of that class (filter_mask_kernel), through search_dense_keys_locked.
//   sparse  the queries of k <= kFusedMaxK as ONE grouped scan of the inverted index when it takes the batch (invert.hip:
//           groups hold queries of one class and read its plane); the rest — longer queries, the larger k, queries whose
//           candidates overflowed, batches the grouped scan does not take — class by class on the byte mask, each class's
//           queries as one batched sparse search (search_sparse_keys_locked).
// Every list is the exact top-k of the single call, so a list of the largest k of a group, cut to a query's own k, is
// that query's list.
int multi_keys_locked(vr_engine* e, const float* q, int nq, const int32_t* ks, int kstride, const QueryClasses& qc,
                      const int64_t* sq_off, const int32_t* sq_idx, const float* sq_val, uint64_t* dense_host,
                      uint64_t* sparse_host) {
  const size_t bytes = sizeof(uint64_t) * static_cast<size_t>(nq) * kstride;
  memset(dense_host, 0, bytes);
  if (sparse_host) memset(sparse_host, 0, bytes);
  if (e->n_rows == 0) return 0;
  const int n_cls = static_cast<int>(qc.filter.size());
  const int dim = e->dim;
  auto put = [&](uint64_t* dst, int i, const uint64_t* src) {
    memcpy(dst + static_cast<size_t>(i) * kstride, src, sizeof(uint64_t) * static_cast<size_t>(ks[i]));
  };
  std::vector<uint8_t> done(static_cast<size_t>(nq), 0);
  const uint32_t* all_planes = nullptr;  // e->cls_planes while it holds the planes of every class
  std::vector<int32_t> order;
  int kb = 0;
  for (int i = 0; i < nq; ++i)
    if (ks[i] <= kFusedMaxK) {
      order.push_back(i);
      kb = std::max(kb, ks[i]);
    }
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return qc.of[static_cast<size_t>(a)] < qc.of[static_cast<size_t>(b)]; });
  if (batch_usable(e, static_cast<int>(order.size()), kb)) {
    const int64_t words = filter_plane_words(e);
    const int per_slice = static_cast<int>(std::min<int64_t>(n_cls, std::max<int64_t>(1, class_plane_budget() / (4 * words))));
    constexpr int kRound = 1024;  // (as search_dense_keys_locked)
    std::vector<float> qs;
    std::vector<int32_t> cls, over;
    std::vector<uint64_t> keys;
    size_t at = 0;
    for (int c0 = 0; c0 < n_cls && at < order.size(); c0 += per_slice) {
      const int c1 = std::min(n_cls, c0 + per_slice);
      size_t end = at;
      while (end < order.size() && qc.of[static_cast<size_t>(order[end])] < c1) ++end;
      const int ns = static_cast<int>(end - at);
      if (!batch_usable(e, ns, kb)) {  // (left to the class loop below)
        at = end;
        continue;
      }
      const uint32_t* planes = nullptr;
      VR_TRY(filter_build_planes(e, qc.filter.data() + c0, c1 - c0, &planes));
      all_planes = c0 == 0 && c1 == n_cls ? planes : nullptr;
      for (int r0 = 0; r0 < ns; r0 += kRound) {
        const int nb = std::min(kRound, ns - r0);
        const int32_t* idx = order.data() + at + r0;
        qs.resize(static_cast<size_t>(nb) * dim);
        cls.resize(static_cast<size_t>(nb));
        for (int j = 0; j < nb; ++j) {
          memcpy(qs.data() + static_cast<size_t>(j) * dim, q + static_cast<int64_t>(idx[j]) * dim, sizeof(float) * dim);
          cls[static_cast<size_t>(j)] = qc.of[static_cast<size_t>(idx[j])] - c0;
        }
        VR_TRY(e->bq_stage.grow(static_cast<int64_t>(nb) * dim, 0, e->stream));
        VR_TRY(e->cls_of_q.grow(nb, 0, e->stream));
        VR_HIP(hipMemcpyAsync(e->bq_stage.p, qs.data(), sizeof(float) * qs.size(), hipMemcpyHostToDevice, e->stream));
        VR_HIP(hipMemcpyAsync(e->cls_of_q.p, cls.data(), sizeof(int32_t) * cls.size(), hipMemcpyHostToDevice, e->stream));
        const uint64_t* keys_dev = nullptr;
        const int32_t* over_dev = nullptr;
        VR_TRY(batch_search(e, e->bq_stage.p, nb, kb, nullptr, &keys_dev, &over_dev, planes, e->cls_of_q.p, words));
        keys.resize(static_cast<size_t>(nb) * kb);
        over.resize(static_cast<size_t>(nb));
        VR_HIP(hipMemcpyAsync(keys.data(), keys_dev, sizeof(uint64_t) * keys.size(), hipMemcpyDeviceToHost, e->stream));
        VR_HIP(hipMemcpyAsync(over.data(), over_dev, sizeof(int32_t) * over.size(), hipMemcpyDeviceToHost, e->stream));
        VR_HIP(hipStreamSynchronize(e->stream));  // (also: qs and cls may be reused)
        e->stat_batched += nb;
        for (int j = 0; j < nb; ++j) {
          e->stat_batch_cands += std::min<int32_t>(over[static_cast<size_t>(j)], kBatchCand);
          if (over[static_cast<size_t>(j)] > kBatchCand) {  // candidate budget exceeded: the class loop redoes it
            ++e->stat_batch_fallback;
            continue;
          }
          put(dense_host, idx[j], keys.data() + static_cast<size_t>(j) * kb);
          done[static_cast<size_t>(idx[j])] = 1;
        }
      }
      at = end;
    }
  }
  std::vector<uint8_t> sparse_done(static_cast<size_t>(nq), 0);
  if (sparse_host && sq_off && e->n_slices_dev > 0 && !order.empty() &&
      static_cast<int64_t>(n_cls) * 4 * filter_plane_words(e) <= class_plane_budget() &&
      inv_class_grouped_usable(e, static_cast<int>(order.size()))) {
    const int n = static_cast<int>(order.size());
    std::vector<int64_t> off(1, 0);
    std::vector<int32_t> ids, cls;
    std::vector<float> vals;
    for (int32_t i : order) {
      ids.insert(ids.end(), sq_idx + sq_off[i], sq_idx + sq_off[i + 1]);
      vals.insert(vals.end(), sq_val + sq_off[i], sq_val + sq_off[i + 1]);
      off.push_back(static_cast<int64_t>(ids.size()));
      cls.push_back(qc.of[static_cast<size_t>(i)]);
    }
    SparseBatch b;
    VR_TRY(prepare_sparse_batch(off.data(), ids.data(), vals.data(), n, true, &b));
    if (!b.ids.empty()) {
      const uint32_t* planes = all_planes;
      if (!planes) VR_TRY(filter_build_planes(e, qc.filter.data(), n_cls, &planes));
      const ClassPlanes classes{planes, filter_plane_words(e), cls.data()};
      VR_TRY(sparse_batch_launch(e, b, n, kb, false, e->live.p, true, &classes));
      std::vector<uint64_t> keys(static_cast<size_t>(n) * kb);
      std::vector<int32_t> flagged(static_cast<size_t>(n), 0);
      VR_HIP(hipMemcpyAsync(keys.data(), e->sq_keys.p, sizeof(uint64_t) * keys.size(), hipMemcpyDeviceToHost, e->stream));
      VR_HIP(hipStreamSynchronize(e->stream));
      if (*pin_host<int32_t>(e, kPinSparseOverflow) != 0 && e->sq_overflow_q) {  // (redone class by class below)
        VR_HIP(hipMemcpyAsync(flagged.data(), e->sq_overflow_q, sizeof(int32_t) * flagged.size(), hipMemcpyDeviceToHost, e->stream));
        VR_HIP(hipStreamSynchronize(e->stream));
      }
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
    }
  }
  // class by class: what the batched scans left
  std::vector<std::vector<int32_t>> members(static_cast<size_t>(n_cls));
  for (int i = 0; i < nq; ++i) members[static_cast<size_t>(qc.of[static_cast<size_t>(i)])].push_back(i);
  const bool sparse_index = e->n_slices_dev > 0;
  std::vector<int32_t> part;
  std::vector<float> qs;
  std::vector<uint64_t> keys;
  std::vector<int64_t> off;
  std::vector<int32_t> ids;
  std::vector<float> vals;
  for (int c = 0; c < n_cls; ++c) {
    const std::vector<int32_t>& m = members[static_cast<size_t>(c)];
    bool dense_left = false, sparse_terms = false;
    for (int32_t i : m) {
      dense_left |= !done[static_cast<size_t>(i)];
      sparse_terms |= sparse_host && sq_off && sq_off[i + 1] > sq_off[i] && !sparse_done[static_cast<size_t>(i)];
    }
    if (!dense_left && !(sparse_terms && sparse_index)) continue;
    const uint8_t* mask = nullptr;
    VR_TRY(filter_build_mask(e, qc.filter[static_cast<size_t>(c)], &mask));
    for (int big = 0; big < 2; ++big) {  // k <= kFusedMaxK, then the rest: each part at its largest k
      part.clear();
      int kq = 0;
      for (int32_t i : m)
        if ((ks[i] > kFusedMaxK) == (big != 0) && !done[static_cast<size_t>(i)]) {
          part.push_back(i);
          kq = std::max(kq, ks[i]);
        }
      if (!part.empty()) {
        const int n = static_cast<int>(part.size());
        qs.resize(static_cast<size_t>(n) * dim);
        for (int j = 0; j < n; ++j)
          memcpy(qs.data() + static_cast<size_t>(j) * dim, q + static_cast<int64_t>(part[static_cast<size_t>(j)]) * dim, sizeof(float) * dim);
        keys.resize(static_cast<size_t>(n) * kq);
        VR_TRY(search_dense_keys_locked(e, qs.data(), n, VR_MEM_HOST, kq, nullptr, keys.data(), nullptr, mask));
        for (int j = 0; j < n; ++j) put(dense_host, part[static_cast<size_t>(j)], keys.data() + static_cast<size_t>(j) * kq);
      }
      if (!sparse_terms || !sparse_index) continue;
      part.clear();
      kq = 0;
      off.assign(1, 0);
      ids.clear();
      vals.clear();
      for (int32_t i : m)
        if ((ks[i] > kFusedMaxK) == (big != 0) && !sparse_done[static_cast<size_t>(i)]) {
          part.push_back(i);
          kq = std::max(kq, ks[i]);
          ids.insert(ids.end(), sq_idx + sq_off[i], sq_idx + sq_off[i + 1]);
          vals.insert(vals.end(), sq_val + sq_off[i], sq_val + sq_off[i + 1]);
          off.push_back(static_cast<int64_t>(ids.size()));
        }
      if (ids.empty()) continue;
      const int n = static_cast<int>(part.size());
      keys.resize(static_cast<size_t>(n) * kq);
      VR_TRY(search_sparse_keys_locked(e, off.data(), ids.data(), vals.data(), n, kq, false, mask, keys.data()));
      for (int j = 0; j < n; ++j) put(sparse_host, part[static_cast<size_t>(j)], keys.data() + static_cast<size_t>(j) * kq);
    }
  }
  return 0;
}

// A batch's queries on the host: device queries are copied back once (the batch is gathered by class on the host).
int multi_host_queries(vr_engine* e, const float* q, int nq, int mem, std::vector<float>* copy, const float** out) {
  *out = q;
  if (mem == VR_MEM_HOST) return 0;
  copy->resize(static_cast<size_t>(nq) * e->dim);
  VR_HIP(hipMemcpyAsync(copy->data(), q, sizeof(float) * copy->size(), hipMemcpyDeviceToHost, e->stream));
  VR_HIP(hipStreamSynchronize(e->stream));
  *out = copy->data();
  return 0;
}

// The dense leg of a filtered batch on lane L (vr_search_dense_multi after its checks): nq x k keys to keys_host.
int dense_multi_keys(vr_engine* L, const float* q, int nq, int mem, int k, const QueryClasses& qc, uint64_t* keys_host) {
  if (qc.filter.size() == 1)  // one class: vr_search_dense
    return search_dense_keys_locked(L, q, nq, mem, k, qc.filter[0], keys_host, nullptr);
  std::vector<float> copy;
  const float* qh = nullptr;
  VR_TRY(multi_host_queries(L, q, nq, mem, &copy, &qh));
  const std::vector<int32_t> ks(static_cast<size_t>(nq), k);
  return multi_keys_locked(L, qh, nq, ks.data(), k, qc, nullptr, nullptr, nullptr, keys_host, nullptr);
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
  std::vector<float> copy;
  const float* qh = nullptr;
  VR_TRY(multi_host_queries(L, q, nq, mem, &copy, &qh));
  return multi_keys_locked(L, qh, nq, ks.data(), kstride, qc, sq_off, sq_idx, sq_val, dense, sparse);
}

// Fusion of every query of a filtered hybrid batch on the host threads, each with its own limit and weight
// (vector_store.py:659-697). Query i's answer goes to output row out_row[i] (out_row null: row i).
int fuse_multi(const uint64_t* dense, const uint64_t* sparse, int nq, int kstride, const int32_t* limits,
               const double* sparse_weights, int32_t fusion, const int32_t* out_row, int32_t out_stride, int64_t* out_rows,
               double* out_scores, int32_t* out_from_dense, int32_t* out_counts) {
  std::atomic<int> failed{0};
  parallel_for(nq, 8, [&](int64_t i) {
    const int k = 3 * limits[i], limit = limits[i];
    int64_t d_rows[kMaxK], s_rows[kMaxK];
    float d_scores[kMaxK], s_scores[kMaxK];
    const int nd = static_cast<int>(decode_keys(dense + static_cast<size_t>(i) * kstride, k, d_rows, d_scores));
    const int ns = static_cast<int>(decode_keys(sparse + static_cast<size_t>(i) * kstride, k, s_rows, s_scores));
    const int64_t r = out_row ? out_row[i] : i;
    const int64_t at = r * out_stride;
    int32_t* fd = out_from_dense ? out_from_dense + at : nullptr;
    const int rc = fusion == VR_FUSION_MINMAX
                       ? fuse_minmax(d_rows, d_scores, nd, s_rows, s_scores, ns, limit, sparse_weights[i], 1, out_rows + at,
                                     out_scores + at, fd, out_counts + r)
                       : fuse_rrf(d_rows, nd, s_rows, ns, limit, sparse_weights[i], out_rows + at, out_scores + at, fd,
                                  out_counts + r);
    if (rc != 0) failed.store(1);
  });
  VR_CHECK(!failed.load(), "fusion failed");
  return 0;
}

}  // namespace

extern "C" {

int vr_search_dense_multi(vr_engine* e, const float* q, int32_t nq, int mem, int32_t k, const vr_filter* filters,
                          int32_t n_filters, const int32_t* filter_of_query, int64_t* rows, float* scores, int32_t* counts) {
  // (the arguments are checked before the engine is touched)
  VR_CHECK(q && rows && scores && nq >= 1, "bad arguments");
  VR_CHECK(k >= 1 && k <= kMaxK, "k = %d not in 1..%d", k, kMaxK);
  VR_CHECK(mem == VR_MEM_HOST || mem == VR_MEM_DEVICE, "bad mem %d", mem);
  QueryClasses qc;
  VR_TRY(classify_queries(filters, n_filters, filter_of_query, nq, &qc));
  VR_TRY(check_engine(e));
  std::vector<uint64_t> keys(static_cast<size_t>(nq) * k);
  {
    SearchLane lane(e);
    VR_TRY(lane.acquire(mem == VR_MEM_DEVICE));
    VR_TRY(dense_multi_keys(lane.L, q, nq, mem, k, qc, keys.data()));
  }
  for (int i = 0; i < nq; ++i) {
    const int64_t c = decode_keys(keys.data() + static_cast<size_t>(i) * k, k, rows + static_cast<int64_t>(i) * k,
                                  scores + static_cast<int64_t>(i) * k);
    if (counts) counts[i] = static_cast<int32_t>(c);
  }
  return 0;
}

int vr_search_hybrid_batch_multi(vr_engine* e, const float* q, int32_t nq, int mem, const int64_t* sq_off,
                                 const int32_t* sq_idx, const float* sq_val, const int32_t* limits,
                                 const double* sparse_weights, int32_t fusion, const vr_filter* filters, int32_t n_filters,
                                 const int32_t* filter_of_query, int32_t out_stride, int64_t* out_rows, double* out_scores,
                                 int32_t* out_from_dense, int32_t* out_counts) {
  // (the arguments are checked before the engine is touched)
  VR_CHECK(q && limits && sparse_weights && out_rows && out_scores && out_counts && nq >= 1, "bad arguments");
  VR_CHECK(fusion == VR_FUSION_MINMAX || fusion == VR_FUSION_RRF, "unknown fusion %d", fusion);
  VR_CHECK(mem == VR_MEM_HOST || mem == VR_MEM_DEVICE, "bad mem %d", mem);
  int max_limit = 0;
  for (int i = 0; i < nq; ++i) {
    VR_CHECK(limits[i] >= 1 && limits[i] <= kMaxK / 3, "limits[%d] = %d not in 1..%d", i, limits[i], kMaxK / 3);
    max_limit = std::max(max_limit, limits[i]);
  }
  VR_CHECK(out_stride >= max_limit, "out_stride = %d is below the largest limit %d", out_stride, max_limit);
  if (sq_off) {
    VR_CHECK(sq_off[nq] == sq_off[0] || (sq_idx && sq_val), "null sparse queries");
    for (int i = 0; i < nq; ++i)
      VR_CHECK(sq_off[i + 1] >= sq_off[i] && sq_off[i + 1] - sq_off[i] <= kMaxQueryTerms,
               "sparse query %d has %lld terms (0..%d supported)", i, static_cast<long long>(sq_off[i + 1] - sq_off[i]), kMaxQueryTerms);
  }
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
  VR_CHECK(k >= 1 && k <= kMaxK, "k = %d not in 1..%d", k, kMaxK);
  VR_CHECK(q_off[nq] == q_off[0] || (q_idx && q_val), "null sparse queries");
  SearchLane lane(e);
  VR_TRY(lane.acquire(false));
  vr_engine* L = lane.L;
  std::vector<uint64_t> keys(static_cast<size_t>(nq) * k, 0ull);
  if (L->n_rows > 0 && L->n_slices_dev > 0) {
    const uint8_t* mask = nullptr;
    VR_TRY(filter_build_mask(L, filter, &mask));
    VR_TRY(search_sparse_keys_locked(L, q_off, q_idx, q_val, nq, k, weights_given != 0, mask, keys.data()));
  }
  for (int i = 0; i < nq; ++i) {
    const int64_t c = decode_keys(keys.data() + static_cast<size_t>(i) * k, k, rows + static_cast<int64_t>(i) * k,
                                  scores + static_cast<int64_t>(i) * k);
    if (counts) counts[i] = static_cast<int32_t>(c);
  }
  return 0;
}

int vr_search_hybrid_keys(vr_engine* e, const float* q, int32_t nq, int mem, const int64_t* sq_off, const int32_t* sq_idx,
                          const float* sq_val, int32_t k, int32_t weights_given, const vr_filter* filter, uint64_t* keys,
                          int keys_mem) {
  VR_TRY(check_engine(e));
  VR_CHECK(q && keys && nq >= 1, "bad arguments");
  VR_CHECK(k >= 1 && k <= kMaxK, "k = %d not in 1..%d", k, kMaxK);
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

int vr_fuse_batch(const int64_t* d_rows, const float* d_scores, const int32_t* d_counts, const int64_t* s_rows,
                  const float* s_scores, const int32_t* s_counts, int32_t nq, int32_t k, int32_t limit, double sparse_weight,
                  int32_t fusion, int32_t json_scores, int64_t* out_rows, double* out_scores, int32_t* out_from_dense,
                  int32_t* out_counts) {
  return fuse_batch(d_rows, d_scores, d_counts, s_rows, s_scores, s_counts, nq, k, limit, sparse_weight, fusion, json_scores,
                    out_rows, out_scores, out_from_dense, out_counts);
}

int vr_search_hybrid_batch(vr_engine* e, const float* q, int32_t nq, int mem, const int64_t* sq_off, const int32_t* sq_idx,
                           const float* sq_val, int32_t limit, double sparse_weight, int32_t fusion, const vr_filter* filter,
                           int64_t* out_rows, double* out_scores, int32_t* out_from_dense, int32_t* out_counts) {
  VR_TRY(check_engine(e));
  VR_CHECK(q && out_rows && out_scores && out_counts && nq >= 1, "bad arguments");
  VR_CHECK(limit >= 1 && limit * 3 <= kMaxK, "limit = %d not in 1..%d", limit, kMaxK / 3);
  VR_CHECK(fusion == VR_FUSION_MINMAX || fusion == VR_FUSION_RRF, "unknown fusion %d", fusion);
  VR_CHECK(mem == VR_MEM_HOST || mem == VR_MEM_DEVICE, "bad mem %d", mem);
  const int k = 3 * limit;  // prefetch_limit, vector_store.py:636
  const size_t per = static_cast<size_t>(nq) * k;
  std::vector<uint64_t> dense(per), sparse(per);
  {
    SearchLane lane(e);
    VR_TRY(lane.acquire(mem == VR_MEM_DEVICE));
    VR_TRY(hybrid_keys_locked(lane.L, q, nq, mem, sq_off, sq_idx, sq_val, k, false, filter, dense.data(), sparse.data()));
  }
  // fusion of every query on the host threads (vector_store.py:659-697, once per query)
  std::atomic<int> failed{0};
  parallel_for(nq, 8, [&](int64_t i) {
    int64_t d_rows[kMaxK], s_rows[kMaxK];
    float d_scores[kMaxK], s_scores[kMaxK];
    const int nd = static_cast<int>(decode_keys(dense.data() + static_cast<size_t>(i) * k, k, d_rows, d_scores));
    const int ns = static_cast<int>(decode_keys(sparse.data() + static_cast<size_t>(i) * k, k, s_rows, s_scores));
    int32_t* fd = out_from_dense ? out_from_dense + i * limit : nullptr;
    const int rc = fusion == VR_FUSION_MINMAX
                       ? fuse_minmax(d_rows, d_scores, nd, s_rows, s_scores, ns, limit, sparse_weight, 1, out_rows + i * limit,
                                     out_scores + i * limit, fd, out_counts + i)
                       : fuse_rrf(d_rows, nd, s_rows, ns, limit, sparse_weight, out_rows + i * limit, out_scores + i * limit,
                                  fd, out_counts + i);
    if (rc != 0) failed.store(1);
  });
  VR_CHECK(!failed.load(), "fusion failed");
  return 0;
}

int vr_merge_keys(vr_engine* e, const uint64_t* parts, int32_t n_parts, int32_t n_lists, int32_t k, int mem, int64_t* out_ids,
                  float* out_scores, int32_t* out_counts) {
  VR_TRY(check_engine(e));
  VR_CHECK(parts && out_ids && out_scores && n_parts >= 1 && n_lists >= 1 && k >= 1, "bad arguments");
  VR_CHECK(mem == VR_MEM_HOST || mem == VR_MEM_DEVICE, "bad mem %d", mem);
  SearchLane lane(e);
  VR_TRY(lane.acquire(mem == VR_MEM_DEVICE));
  vr_engine* L = lane.L;
  const int64_t total = static_cast<int64_t>(n_parts) * n_lists * k;
  const uint64_t* parts_dev = parts;
  if (mem == VR_MEM_HOST) {
    VR_TRY(L->mg_in.grow(total, 0, L->stream));
    VR_HIP(hipMemcpyAsync(L->mg_in.p, parts, sizeof(uint64_t) * static_cast<size_t>(total), hipMemcpyHostToDevice, L->stream));
    parts_dev = L->mg_in.p;
  }
  const int64_t per = static_cast<int64_t>(n_lists) * k;
  VR_TRY(L->mg_gid.grow(per, 0, L->stream));
  VR_TRY(L->mg_score.grow(per, 0, L->stream));
  VR_TRY(L->mg_cnt.grow(n_lists, 0, L->stream));
  VR_TRY(topk_merge_parts(L, parts_dev, n_parts, n_lists, k, L->mg_gid.p, L->mg_score.p, L->mg_cnt.p));
  VR_HIP(hipMemcpyAsync(out_ids, L->mg_gid.p, sizeof(int64_t) * static_cast<size_t>(per), hipMemcpyDeviceToHost, L->stream));
  VR_HIP(hipMemcpyAsync(out_scores, L->mg_score.p, sizeof(float) * static_cast<size_t>(per), hipMemcpyDeviceToHost, L->stream));
  std::vector<int32_t> cnt(static_cast<size_t>(n_lists));
  VR_HIP(hipMemcpyAsync(cnt.data(), L->mg_cnt.p, sizeof(int32_t) * static_cast<size_t>(n_lists), hipMemcpyDeviceToHost, L->stream));
  VR_HIP(hipStreamSynchronize(L->stream));
  if (out_counts) memcpy(out_counts, cnt.data(), sizeof(int32_t) * static_cast<size_t>(n_lists));
  return 0;
}

int vr_mmr_select(vr_engine* e, int32_t n_lists, const int64_t* list_off, const int64_t* rows, const double* relevance,
                  const double* diversity, const int32_t* limits, int64_t generation, int32_t out_stride, int32_t* out_pos,
                  int32_t* out_counts) {
  VR_TRY(check_engine(e));
  VR_CHECK(n_lists >= 0, "n_lists = %d", n_lists);
  if (n_lists == 0) return 0;
  VR_CHECK(list_off && diversity && limits && out_counts && out_stride >= 0, "bad arguments");
  VR_CHECK(list_off[0] == 0, "list_off[0] = %lld, must be 0", static_cast<long long>(list_off[0]));
  for (int32_t i = 0; i < n_lists; ++i) {
    const int64_t len = list_off[i + 1] - list_off[i];
    VR_CHECK(len >= 0, "list_off decreases at list %d", i);
    VR_CHECK(len <= kMaxK, "list %d holds %lld candidates, at most %d", i, static_cast<long long>(len), kMaxK);
    VR_CHECK(diversity[i] >= 0.0 && diversity[i] <= 1.0, "list %d: diversity %g not in [0, 1]", i, diversity[i]);
    VR_CHECK(limits[i] >= 0 && limits[i] <= out_stride, "list %d: limit %d not in [0, out_stride = %d]", i, limits[i],
             out_stride);
  }
  const int64_t n = list_off[n_lists];
  VR_CHECK(n == 0 || (rows && relevance), "bad arguments");
  VR_CHECK(out_pos || out_stride == 0, "bad arguments");
  for (int64_t j = 0; j < n; ++j)
    VR_CHECK(std::isfinite(relevance[j]), "relevance %lld is not finite", static_cast<long long>(j));
  SearchLane lane(e);
  VR_TRY(lane.acquire(false));
  if (e->generation.load() != generation) return VR_STALE_GENERATION;  // (under the shared lock: no renumbering now)
  vr_engine* L = lane.L;
  for (int64_t j = 0; j < n; ++j)
    VR_CHECK(rows[j] >= 0 && rows[j] < L->n_rows, "row %lld out of range [0, %lld)", static_cast<long long>(rows[j]),
             static_cast<long long>(L->n_rows));
  VR_TRY(mmr_select_run(L, n_lists, list_off, rows, relevance, diversity, limits, out_stride, out_pos));
  for (int32_t i = 0; i < n_lists; ++i)
    out_counts[i] = static_cast<int32_t>(std::min<int64_t>(limits[i], list_off[i + 1] - list_off[i]));
  return 0;
}

int vr_sparse_row_ids(vr_engine* e, const int64_t* rows, int64_t n, int32_t* out, int64_t cap, int mem, int32_t* stride,
                      int64_t* n_points) {
  VR_TRY(check_engine(e));
  VR_CHECK(stride != nullptr && n >= 0, "bad arguments");
  VR_CHECK(mem == VR_MEM_HOST || mem == VR_MEM_DEVICE, "bad mem %d", mem);
  std::lock_guard<std::mutex> writer(e->wmu);  // (the master's staging arrays)
  std::shared_lock<std::shared_mutex> view(e->rw);
  const int w = sparse_max_width(e);
  *stride = w;
  if (n_points) *n_points = 0;
  if (!out || n == 0 || w == 0) return 0;
  VR_CHECK(rows != nullptr, "null rows");
  const int64_t total = n * w;
  VR_CHECK(cap >= total, "room for %lld ids, %lld needed", static_cast<long long>(cap), static_cast<long long>(total));
  VR_TRY(e->stage_i64a.grow(n, 0, e->stream));
  VR_HIP(hipMemcpyAsync(e->stage_i64a.p, rows, sizeof(int64_t) * static_cast<size_t>(n), hipMemcpyHostToDevice, e->stream));
  int32_t* out_dev = out;
  if (mem == VR_MEM_HOST) {
    VR_TRY(e->stage_i32a.grow(total, 0, e->stream));
    out_dev = e->stage_i32a.p;
  }
  int64_t pts = 0;
  VR_TRY(sparse_row_ids(e, e->stage_i64a.p, n, w, out_dev, &pts));
  if (n_points) *n_points = pts;
  if (mem == VR_MEM_HOST) {
    VR_HIP(hipMemcpyAsync(out, out_dev, sizeof(int32_t) * static_cast<size_t>(total), hipMemcpyDeviceToHost, e->stream));
    VR_HIP(hipStreamSynchronize(e->stream));
  }
  return 0;
}

int vr_df_apply(vr_engine* e, const int32_t* ids, int64_t n_ids, int mem, int64_t n_points, int32_t sign) {
  VR_TRY(check_engine(e));
  VR_CHECK(n_ids >= 0 && (n_ids == 0 || ids) && (sign == 1 || sign == -1) && n_points >= 0, "bad arguments");
  VR_CHECK(mem == VR_MEM_HOST || mem == VR_MEM_DEVICE, "bad mem %d", mem);
  std::lock_guard<std::mutex> writer(e->wmu);
  PublishLock publish(e);  // (the table may be re-hashed; searches read it)
  const int32_t* ids_dev = ids;
  if (mem == VR_MEM_HOST && n_ids > 0) {
    VR_TRY(e->stage_i32a.grow(n_ids, 0, e->stream));
    VR_HIP(hipMemcpyAsync(e->stage_i32a.p, ids, sizeof(int32_t) * static_cast<size_t>(n_ids), hipMemcpyHostToDevice, e->stream));
    ids_dev = e->stage_i32a.p;
  }
  VR_TRY(sparse_df_apply(e, ids_dev, n_ids, sign));
  VR_HIP(hipStreamSynchronize(e->stream));
  e->n_sparse_points += sign * n_points;
  return 0;
}

}  // extern "C"

// ---- a question as TEXT, one call (the MCP search tool's three calls — embed_query, sparse embed_query,
// vector_store.search: mcp_server.py:469-485 — without the trips through Python between them) -----------------------

namespace {

// a device row for a query embedding in flight: from the engine's free list (released by vr_engine_destroy), or a new one
float* take_query_row(vr_engine* e) {
  {
    std::lock_guard<std::mutex> g(e->query_rows_mu);
    if (!e->query_rows_free.empty()) {
      float* p = e->query_rows_free.back();
      e->query_rows_free.pop_back();
      return p;
    }
  }
  float* p = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&p), sizeof(float) * kMaxDim) != hipSuccess) return nullptr;
  return p;
}

void give_query_row(vr_engine* e, float* p) {
  std::lock_guard<std::mutex> g(e->query_rows_mu);
  e->query_rows_free.push_back(p);
}

// token ids of n (prefixed) questions, packed: ids and n + 1 offsets as vr_encode takes them (host threads)
int question_wordpieces(const Tokenizer* tokenizer, const char* const* texts, const int64_t* lens, int n, int max_len,
                        std::vector<int32_t>* ids, std::vector<int32_t>* off32) {
  std::vector<int64_t> off(static_cast<size_t>(n) + 1, 0);
  // room for the ids: a piece consumes at least a byte of text (n * max_len ids would be megabytes of zeros to write
  // at max_len = 8192); a normaliser that expands its input can need more, and then the tokenizer says how many
  size_t room = 0;
  for (int i = 0; i < n; ++i) room += static_cast<size_t>(std::min<int64_t>(std::max<int64_t>(lens[i], 0) + 2, max_len));
  ids->resize(room);
  int64_t needed = 0;
  int rc = tokenizer->encode(texts, lens, n, max_len, off.data(), ids->data(), static_cast<int64_t>(ids->size()), &needed);
  if (rc == -2) {
    ids->resize(static_cast<size_t>(needed));
    rc = tokenizer->encode(texts, lens, n, max_len, off.data(), ids->data(), static_cast<int64_t>(ids->size()), &needed);
    if (rc == 0) vr::set_error("%s", "");  // (the first attempt's "buffer holds ..." is not this call's error)
  }
  VR_TRY(rc);
  VR_CHECK(needed <= INT32_MAX, "%lld tokens", static_cast<long long>(needed));
  ids->resize(static_cast<size_t>(needed));
  off32->resize(static_cast<size_t>(n) + 1);
  for (int i = 0; i <= n; ++i) (*off32)[static_cast<size_t>(i)] = static_cast<int32_t>(off[static_cast<size_t>(i)]);
  return 0;
}

// The hashed BM25 stems of n raw questions (Bm25.query_embed: the SET of them, every value 1.0 — SURVEY.md a7) as a
// CSR: per question ascending and distinct. A null text or length 0 has none. Host threads.
int question_stems(const char* const* texts, const int64_t* lens, int n, std::vector<int64_t>* off,
                   std::vector<int32_t>* stems) {
  static const char kEmpty[1] = {0};
  std::vector<const char*> t(static_cast<size_t>(n));
  std::vector<int64_t> l(static_cast<size_t>(n));
  int64_t cap = 0;
  for (int i = 0; i < n; ++i) {
    const bool some = texts && texts[i] && lens[i] > 0;
    t[static_cast<size_t>(i)] = some ? texts[i] : kEmpty;
    l[static_cast<size_t>(i)] = some ? lens[i] : 0;
    cap += l[static_cast<size_t>(i)] / 2 + 2;
  }
  off->assign(static_cast<size_t>(n) + 1, 0);
  stems->resize(static_cast<size_t>(cap));
  int64_t need = 0;
  int rc = vr_bm25_tokenize(t.data(), l.data(), n, off->data(), stems->data(), cap, &need);
  if (rc == -2) {
    stems->resize(static_cast<size_t>(need));
    rc = vr_bm25_tokenize(t.data(), l.data(), n, off->data(), stems->data(), need, &need);
  }
  VR_TRY(rc);
  // sort and deduplicate each question's range in place, then close the gaps
  std::vector<int64_t> kept(static_cast<size_t>(n));
  parallel_for(n, 64, [&](int64_t i) {
    int32_t* b = stems->data() + (*off)[static_cast<size_t>(i)];
    int32_t* e = stems->data() + (*off)[static_cast<size_t>(i) + 1];
    std::sort(b, e);
    kept[static_cast<size_t>(i)] = std::unique(b, e) - b;
  });
  int64_t at = 0;
  for (int i = 0; i < n; ++i) {
    VR_CHECK(kept[static_cast<size_t>(i)] <= kMaxQueryTerms, "query with %lld distinct terms",
             static_cast<long long>(kept[static_cast<size_t>(i)]));
    const int64_t from = (*off)[static_cast<size_t>(i)];
    if (at != from) memmove(stems->data() + at, stems->data() + from, sizeof(int32_t) * static_cast<size_t>(kept[static_cast<size_t>(i)]));
    (*off)[static_cast<size_t>(i)] = at;
    at += kept[static_cast<size_t>(i)];
  }
  (*off)[static_cast<size_t>(n)] = at;
  stems->resize(static_cast<size_t>(at));
  return 0;
}

// rows pick[0 .. n) of src (n_src x dim) side by side in dst (n x dim); device arrays
__global__ __launch_bounds__(256) void gather_query_rows_kernel(const float* __restrict__ src, const int32_t* __restrict__ pick,
                                                                int64_t n, int dim, float* __restrict__ dst) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n * dim) return;
  const int64_t r = i / dim;
  dst[i] = src[static_cast<int64_t>(pick[r]) * dim + (i - r * dim)];
}

// vr_query_text(_unigram): one pipeline, whatever tokenises the question
int query_text(vr_engine* e, const Tokenizer* tokenizer, const char* dense_text, int64_t dense_len,
               const char* sparse_text, int64_t sparse_len, int32_t max_len, int32_t limit, double sparse_weight,
               int32_t fusion, const vr_filter* filter, int64_t* out_rows, double* out_scores, int32_t* out_from_dense,
               int32_t* out_count, int32_t* out_hybrid) {
  VR_TRY(check_engine(e));
  VR_CHECK(tokenizer && dense_text && dense_len >= 0 && out_rows && out_scores && out_count, "bad arguments");
  VR_CHECK(limit >= 1 && limit * 3 <= kMaxK, "limit = %d not in 1..%d", limit, kMaxK / 3);
  VR_CHECK(fusion == VR_FUSION_MINMAX || fusion == VR_FUSION_RRF, "unknown fusion %d", fusion);
  VR_CHECK(max_len >= 2 && max_len <= 4096, "max_len %d", max_len);
  *out_count = 0;
  if (out_hybrid) *out_hybrid = 0;
  // 1. host: WordPiece ids of the (prefixed) query, hashed BM25 stems of the raw query (Bm25.query_embed: the SET of
  //    them, every value 1.0 — SURVEY.md a7)
  std::vector<int32_t> wp, off32;
  {
    const char* texts[1] = {dense_text};
    const int64_t lens[1] = {dense_len};
    VR_TRY(question_wordpieces(tokenizer, texts, lens, 1, max_len, &wp, &off32));
  }
  std::vector<int32_t> stems;
  {
    const char* texts[1] = {sparse_text};
    const int64_t lens[1] = {sparse_len};
    std::vector<int64_t> off;
    VR_TRY(question_stems(texts, lens, 1, &off, &stems));
  }
  // 2. the embedding, left in device memory (the encoder is shared with the writers: one forward pass at a time)
  VR_CHECK(encoder_hidden(e) == e->dim, "encoder width %d != store dimension %d", encoder_hidden(e), e->dim);
  float* q_dev = take_query_row(e);
  VR_CHECK(q_dev != nullptr, "no device memory for the query embedding");
  struct Giver {
    vr_engine* e;
    float* p;
    ~Giver() { give_query_row(e, p); }
  } giver{e, q_dev};
  const bool hybrid = !stems.empty();
  if (out_hybrid) *out_hybrid = hybrid ? 1 : 0;
  if (hybrid) {
    // 3a. hybrid: the lane is taken and the filter mask built BEFORE the forward pass (both used to follow it, in a
    //     second engine call; worth a hundredth of a millisecond), then the forward pass, then both legs on the lane. Lock order as
    //     everywhere: the writers' mutex (the encoder), then the shared lock of the lane — a writer takes the same mutex
    //     before it publishes.
    const int k = limit * 3;  // prefetch_limit, vector_store.py:636
    std::vector<float> ones(stems.size(), 1.0f);
    std::unique_lock<std::mutex> writer(e->wmu);
    SearchLane lane(e);
    VR_TRY(lane.acquire(false));
    vr_engine* L = lane.L;
    if (L->n_rows == 0) return 0;
    const uint8_t* mask = nullptr;
    VR_TRY(filter_build_mask(L, filter, &mask));
    const int nnz = static_cast<int>(stems.size());
    VR_TRY(encoder_encode(e, wp.data(), off32.data(), 1, VR_MEM_HOST, q_dev, VR_MEM_DEVICE));  // (returns with the stream drained)
    writer.unlock();
    bool have_sparse = false;
    VR_TRY(hybrid_one_query(L, q_dev, VR_MEM_DEVICE, stems.data(), ones.data(), nnz, k, false, mask, &have_sparse));
    int64_t d_rows[kMaxK], s_rows[kMaxK];
    float d_scores[kMaxK], s_scores[kMaxK];
    const int nd = static_cast<int>(decode_keys(pin_host<uint64_t>(L, kPinDenseKeys), k, d_rows, d_scores));
    const int ns = have_sparse ? static_cast<int>(decode_keys(pin_host<uint64_t>(L, kPinSparseKeys), k, s_rows, s_scores)) : 0;
    if (fusion == VR_FUSION_MINMAX)
      return fuse_minmax(d_rows, d_scores, nd, s_rows, s_scores, ns, limit, sparse_weight, 1, out_rows, out_scores, out_from_dense,
                         out_count);
    return fuse_rrf(d_rows, nd, s_rows, ns, limit, sparse_weight, out_rows, out_scores, out_from_dense, out_count);
  }
  {
    std::lock_guard<std::mutex> writer(e->wmu);
    VR_TRY(encoder_encode(e, wp.data(), off32.data(), 1, VR_MEM_HOST, q_dev, VR_MEM_DEVICE));  // (returns with the stream drained)
  }
  // no term survived the stop-word filter: the dense-only branch of VectorStoreService.search (vector_store.py:612-617)
  std::vector<float> sc(static_cast<size_t>(limit));
  int32_t c = 0;
  VR_TRY(vr_search_dense(e, q_dev, 1, VR_MEM_DEVICE, limit, filter, out_rows, sc.data(), &c));
  for (int i = 0; i < c; ++i) {
    out_scores[i] = static_cast<double>(sc[static_cast<size_t>(i)]);
    if (out_from_dense) out_from_dense[i] = 1;
  }
  *out_count = c;
  return 0;
}

// vr_query_text_batch(_unigram): one pipeline, whatever tokenises the questions
int query_text_batch(vr_engine* e, const Tokenizer* tokenizer, int32_t n, const char* const* dense_texts,
                     const int64_t* dense_lens, const char* const* sparse_texts, const int64_t* sparse_lens,
                     int32_t max_len, const int32_t* limits, const double* sparse_weights, int32_t fusion,
                     const vr_filter* filters, int32_t n_filters, const int32_t* filter_of_query, int32_t out_stride,
                     int64_t* out_rows, double* out_scores, int32_t* out_from_dense, int32_t* out_counts,
                     int32_t* out_hybrid, float* out_embeddings) {
  // (the arguments are checked before the engine is touched, as in the _multi calls)
  VR_CHECK(n >= 0, "bad arguments");
  if (n == 0) return 0;
  VR_CHECK(tokenizer && dense_texts && dense_lens && limits && sparse_weights && out_rows && out_scores && out_counts,
           "bad arguments");
  VR_CHECK(fusion == VR_FUSION_MINMAX || fusion == VR_FUSION_RRF, "unknown fusion %d", fusion);
  VR_CHECK(max_len >= 2 && max_len <= 4096, "max_len %d", max_len);
  int max_limit = 0;
  for (int i = 0; i < n; ++i) {
    VR_CHECK(dense_texts[i] && dense_lens[i] >= 0, "dense text %d: null or negative length", i);
    VR_CHECK(!sparse_texts || !sparse_texts[i] || (sparse_lens && sparse_lens[i] >= 0), "sparse text %d: no length", i);
    VR_CHECK(limits[i] >= 1 && limits[i] <= kMaxK / 3, "limits[%d] = %d not in 1..%d", i, limits[i], kMaxK / 3);
    max_limit = std::max(max_limit, limits[i]);
  }
  VR_CHECK(out_stride >= max_limit, "out_stride = %d is below the largest limit %d", out_stride, max_limit);
  {
    QueryClasses qc;
    VR_TRY(classify_queries(filters, n_filters, filter_of_query, n, &qc));
  }
  VR_TRY(check_engine(e));
  VR_CHECK(encoder_hidden(e) == e->dim, "encoder width %d != store dimension %d", encoder_hidden(e), e->dim);
  const int dim = e->dim;
  // 1. host: WordPiece ids of every (prefixed) question, the hashed stems of every raw one
  std::vector<int32_t> wp, off32;
  VR_TRY(question_wordpieces(tokenizer, dense_texts, dense_lens, n, max_len, &wp, &off32));
  std::vector<int64_t> st_off;
  std::vector<int32_t> stems;
  VR_TRY(question_stems(sparse_texts, sparse_lens, n, &st_off, &stems));
  // the questions with a stem take the hybrid branch, the others the dense one (vector_store.py:560-619); the hybrid
  // ones' stems again as a CSR in their order, values 1.0
  std::vector<int32_t> pick, h_lim, d_lim, h_fq, d_fq;
  std::vector<double> h_w;
  std::vector<int64_t> h_off(1, 0);
  std::vector<int32_t> h_ids;
  for (int i = 0; i < n; ++i) {
    const int64_t a = st_off[static_cast<size_t>(i)], b = st_off[static_cast<size_t>(i) + 1];
    if (out_hybrid) out_hybrid[i] = b > a ? 1 : 0;
    out_counts[i] = 0;
    if (b == a) continue;
    pick.push_back(i);
    h_ids.insert(h_ids.end(), stems.begin() + a, stems.begin() + b);
    h_off.push_back(static_cast<int64_t>(h_ids.size()));
  }
  const int nh = static_cast<int>(pick.size());
  for (int i = 0; i < n; ++i)
    if (st_off[static_cast<size_t>(i) + 1] == st_off[static_cast<size_t>(i)]) pick.push_back(i);
  const std::vector<float> ones(h_ids.size(), 1.0f);
  for (int j = 0; j < n; ++j) {
    const int i = pick[static_cast<size_t>(j)];
    (j < nh ? h_lim : d_lim).push_back(limits[i]);
    (j < nh ? h_fq : d_fq).push_back(filter_of_query ? filter_of_query[i] : -1);
    if (j < nh) h_w.push_back(sparse_weights[i]);
  }
  // 2. one forward pass over all n questions, the pooled rows left in device memory. Lock order as vr_query_text: the
  //    writers' mutex (the encoder), then the shared lock of a lane.
  std::unique_lock<std::mutex> writer(e->wmu);
  SearchLane lane(e);
  VR_TRY(lane.acquire(false));
  vr_engine* L = lane.L;
  VR_TRY(L->qt_emb.grow(static_cast<int64_t>(n) * dim, 0, L->stream));
  VR_TRY(encoder_encode(e, wp.data(), off32.data(), n, VR_MEM_HOST, L->qt_emb.p, VR_MEM_DEVICE));  // (stream drained)
  writer.unlock();
  if (out_embeddings)
    VR_HIP(hipMemcpyAsync(out_embeddings, L->qt_emb.p, sizeof(float) * static_cast<size_t>(n) * dim, hipMemcpyDeviceToHost,
                          L->stream));
  // the hybrid questions first, then the dense ones, gathered on the device (nothing to do when all are hybrid)
  const float* q = L->qt_emb.p;
  if (nh < n) {
    VR_TRY(L->qt_pick.grow(n, 0, L->stream));
    VR_TRY(L->qt_gather.grow(static_cast<int64_t>(n) * dim, 0, L->stream));
    VR_HIP(hipMemcpyAsync(L->qt_pick.p, pick.data(), sizeof(int32_t) * static_cast<size_t>(n), hipMemcpyHostToDevice, L->stream));
    const int64_t total = static_cast<int64_t>(n) * dim;
    hipLaunchKernelGGL(gather_query_rows_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, L->stream,
                       L->qt_emb.p, L->qt_pick.p, static_cast<int64_t>(n), dim, L->qt_gather.p);
    VR_HIP(hipGetLastError());
    q = L->qt_gather.p;
  }
  VR_HIP(hipStreamSynchronize(L->stream));
  // 3. the search legs in slices of questions (answers are per question: slicing changes no bits)
  constexpr int kSlice = 4096;
  std::vector<uint64_t> dense, sparse;
  for (int s0 = 0; s0 < nh; s0 += kSlice) {  // hybrid: the filtered hybrid batch, fused on the host threads
    const int ns = std::min(kSlice, nh - s0);
    QueryClasses qc;
    VR_TRY(classify_queries(filters, n_filters, h_fq.data() + s0, ns, &qc));
    int ml = 0;
    for (int j = 0; j < ns; ++j) ml = std::max(ml, h_lim[static_cast<size_t>(s0 + j)]);
    const int kstride = 3 * ml;
    dense.assign(static_cast<size_t>(ns) * kstride, 0);
    sparse.assign(static_cast<size_t>(ns) * kstride, 0);
    VR_TRY(hybrid_multi_keys(L, q + static_cast<int64_t>(s0) * dim, ns, VR_MEM_DEVICE, h_off.data() + s0, h_ids.data(),
                             ones.data(), h_lim.data() + s0, qc, kstride, dense.data(), sparse.data()));
    VR_TRY(fuse_multi(dense.data(), sparse.data(), ns, kstride, h_lim.data() + s0, h_w.data() + s0, fusion, pick.data() + s0,
                      out_stride, out_rows, out_scores, out_from_dense, out_counts));
  }
  const int nd = n - nh;
  for (int s0 = 0; s0 < nd; s0 += kSlice) {  // no stem: the filtered dense batch at the slice's largest limit, trimmed
    const int ns = std::min(kSlice, nd - s0);
    QueryClasses qc;
    VR_TRY(classify_queries(filters, n_filters, d_fq.data() + s0, ns, &qc));
    int k = 0;
    for (int j = 0; j < ns; ++j) k = std::max(k, d_lim[static_cast<size_t>(s0 + j)]);
    dense.assign(static_cast<size_t>(ns) * k, 0);
    VR_TRY(dense_multi_keys(L, q + static_cast<int64_t>(nh + s0) * dim, ns, VR_MEM_DEVICE, k, qc, dense.data()));
    parallel_for(ns, 64, [&](int64_t j) {
      const int i = pick[static_cast<size_t>(nh + s0 + j)], limit = d_lim[static_cast<size_t>(s0 + j)];
      int64_t rows[kMaxK];
      float sc[kMaxK];
      const int c = std::min(limit, static_cast<int>(decode_keys(dense.data() + static_cast<size_t>(j) * k, k, rows, sc)));
      const int64_t at = static_cast<int64_t>(i) * out_stride;
      for (int r = 0; r < c; ++r) {  // the cosines widened to f64 (vr_query_text's dense branch)
        out_rows[at + r] = rows[r];
        out_scores[at + r] = static_cast<double>(sc[r]);
        if (out_from_dense) out_from_dense[at + r] = 1;
      }
      out_counts[i] = c;
    });
  }
  if (out_embeddings) VR_HIP(hipStreamSynchronize(L->stream));
  return 0;
}

}  // namespace

extern "C" {

int vr_query_text(vr_engine* e, const vr_wordpiece* tokenizer, const char* dense_text, int64_t dense_len,
                  const char* sparse_text, int64_t sparse_len, int32_t max_len, int32_t limit, double sparse_weight,
                  int32_t fusion, const vr_filter* filter, int64_t* out_rows, double* out_scores, int32_t* out_from_dense,
                  int32_t* out_count, int32_t* out_hybrid) {
  return query_text(e, as_tokenizer(tokenizer), dense_text, dense_len, sparse_text, sparse_len, max_len, limit,
                    sparse_weight, fusion, filter, out_rows, out_scores, out_from_dense, out_count, out_hybrid);
}

int vr_query_text_unigram(vr_engine* e, const vr_unigram* tokenizer, const char* dense_text, int64_t dense_len,
                          const char* sparse_text, int64_t sparse_len, int32_t max_len, int32_t limit,
                          double sparse_weight, int32_t fusion, const vr_filter* filter, int64_t* out_rows,
                          double* out_scores, int32_t* out_from_dense, int32_t* out_count, int32_t* out_hybrid) {
  return query_text(e, as_tokenizer(tokenizer), dense_text, dense_len, sparse_text, sparse_len, max_len, limit,
                    sparse_weight, fusion, filter, out_rows, out_scores, out_from_dense, out_count, out_hybrid);
}

int vr_query_text_batch(vr_engine* e, const vr_wordpiece* tokenizer, int32_t n, const char* const* dense_texts,
                        const int64_t* dense_lens, const char* const* sparse_texts, const int64_t* sparse_lens,
                        int32_t max_len, const int32_t* limits, const double* sparse_weights, int32_t fusion,
                        const vr_filter* filters, int32_t n_filters, const int32_t* filter_of_query, int32_t out_stride,
                        int64_t* out_rows, double* out_scores, int32_t* out_from_dense, int32_t* out_counts,
                        int32_t* out_hybrid, float* out_embeddings) {
  return query_text_batch(e, as_tokenizer(tokenizer), n, dense_texts, dense_lens, sparse_texts, sparse_lens, max_len,
                          limits, sparse_weights, fusion, filters, n_filters, filter_of_query, out_stride, out_rows,
                          out_scores, out_from_dense, out_counts, out_hybrid, out_embeddings);
}

int vr_query_text_batch_unigram(vr_engine* e, const vr_unigram* tokenizer, int32_t n, const char* const* dense_texts,
                                const int64_t* dense_lens, const char* const* sparse_texts, const int64_t* sparse_lens,
                                int32_t max_len, const int32_t* limits, const double* sparse_weights, int32_t fusion,
                                const vr_filter* filters, int32_t n_filters, const int32_t* filter_of_query,
                                int32_t out_stride, int64_t* out_rows, double* out_scores, int32_t* out_from_dense,
                                int32_t* out_counts, int32_t* out_hybrid, float* out_embeddings) {
  return query_text_batch(e, as_tokenizer(tokenizer), n, dense_texts, dense_lens, sparse_texts, sparse_lens, max_len,
                          limits, sparse_weights, fusion, filters, n_filters, filter_of_query, out_stride, out_rows,
                          out_scores, out_from_dense, out_counts, out_hybrid, out_embeddings);
}

}  // extern "C"
