// extern "C" surface of libvoitta_engine.so (include/voitta_engine.h) outside the searches: engine lifecycle, the
// encoder and reranker entry points, the store (upsert / index / delete / count / read-back), persistence and the
// small helpers of the sharded and MMR paths. The searches are in search.hip, the text-question pipeline in
// query_text.hip. Every entry point cites the reference call it stands in for in the header; this file only
// sequences kernels on the engine's stream and moves small results back to the host.

#include "search.h"

#include <algorithm>
#include <climits>
#include <cmath>

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
  VR_TRY(check_mem(mem));
  std::lock_guard<std::mutex> writer(e->wmu);
  return encoder_load(e, desc, tensors, n_tensors, mem);
}

int vr_encoder_set_attention_bias(vr_engine* e, const float* table, int32_t heads, int32_t radius, int mem) {
  VR_TRY(check_engine(e));
  if (table) VR_TRY(check_mem(mem));
  std::lock_guard<std::mutex> writer(e->wmu);
  return encoder_set_attention_bias(e, table, heads, radius, mem);
}

int vr_encoder_set_attention_slopes(vr_engine* e, const float* slopes, int32_t heads, int mem) {
  VR_TRY(check_engine(e));
  if (slopes) VR_TRY(check_mem(mem));
  std::lock_guard<std::mutex> writer(e->wmu);
  return encoder_set_attention_slopes(e, slopes, heads, mem);
}

int vr_encoder_set_head(vr_engine* e, const vr_head_stage* stages, int32_t n_stages, int32_t truncate_dim, int mem) {
  VR_TRY(check_engine(e));
  if (stages) VR_TRY(check_mem(mem));
  std::lock_guard<std::mutex> writer(e->wmu);
  return encoder_set_head(e, stages, n_stages, truncate_dim, mem);
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

int vr_encode_spans(vr_engine* e, const int32_t* ids, const int32_t* offsets, int32_t n_seq, const int32_t* span_off,
                    const int32_t* span_tok, int mem, float* out, int out_mem) {
  VR_TRY(check_engine(e));
  if (n_seq <= 0) return 0;
  VR_CHECK(ids && offsets && span_off, "bad arguments");
  VR_CHECK((mem == VR_MEM_HOST || mem == VR_MEM_DEVICE) && (out_mem == VR_MEM_HOST || out_mem == VR_MEM_DEVICE),
           "bad mem");
  if (mem == VR_MEM_HOST) VR_CHECK(span_off[n_seq] <= 0 || (span_tok && out), "bad arguments");
  else VR_CHECK(span_tok && out, "bad arguments");
  std::lock_guard<std::mutex> writer(e->wmu);
  return encoder_encode_spans(e, ids, offsets, n_seq, span_off, span_tok, mem, -1, out, out_mem);
}

int vr_encode_semantic(vr_engine* e, const int32_t* ids, const int32_t* offsets, int32_t n_seq, const int32_t* unit_off,
                       const int32_t* unit_tok, int mem, const vr_semantic_params* params, float* out_rows,
                       int32_t* out_unit_start, float* out_gap_dist, int32_t* n_chunks, int out_mem) {
  VR_TRY(check_engine(e));
  VR_CHECK(n_chunks != nullptr, "null n_chunks");
  *n_chunks = 0;
  if (n_seq <= 0) return 0;
  VR_CHECK(ids && offsets && unit_off && params, "bad arguments");
  VR_CHECK((mem == VR_MEM_HOST || mem == VR_MEM_DEVICE) && (out_mem == VR_MEM_HOST || out_mem == VR_MEM_DEVICE),
           "bad mem");
  std::lock_guard<std::mutex> writer(e->wmu);
  return encoder_encode_semantic(e, ids, offsets, n_seq, unit_off, unit_tok, mem, params, out_rows, out_unit_start,
                                 out_gap_dist, n_chunks, out_mem);
}

int vr_reranker_load(vr_engine* e, const vr_bert_desc* desc, const void* const* tensors, int32_t n_tensors, int mem) {
  VR_TRY(check_engine(e));
  VR_CHECK(desc && tensors, "null argument");
  VR_TRY(check_mem(mem));
  std::lock_guard<std::mutex> writer(e->wmu);
  return reranker_load(e, desc, tensors, n_tensors, mem);
}

int vr_reranker_load_decoder(vr_engine* e, const vr_bert_desc* desc, const void* const* tensors, int32_t n_tensors, int mem) {
  VR_TRY(check_engine(e));
  VR_CHECK(desc && tensors, "null argument");
  VR_TRY(check_mem(mem));
  std::lock_guard<std::mutex> writer(e->wmu);
  return reranker_load_decoder(e, desc, tensors, n_tensors, mem);
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

int vr_rerank_text_bpe(vr_engine* e, const vr_bpe* tokenizer, int32_t n_queries, const char* const* queries,
                           const int64_t* query_lens, const int64_t* cand_off, const char* const* passages,
                           const int64_t* passage_lens, int32_t max_len, float* out_logits) {
  VR_CHECK(max_len >= 3, "max_len %d cannot hold the three special tokens of a pair", max_len);
  return rerank_text(e, vr::as_tokenizer(tokenizer), n_queries, queries, query_lens, cand_off, passages, passage_lens,
                     max_len, out_logits);
}

}  // extern "C"

// Body of vr_upsert, also the last stage of index_batch. Caller holds e->wmu and the exclusive lock.
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

// Body of vr_index_batch and vr_index_batch_spans: BM25 tf of the n rows, the forward pass of n_seq sequences into n
// engine-owned dense rows — one per sequence (span_off null, n_seq == n) or one per span — and the append.
static int index_batch(vr_engine* e, int64_t n, int mem, const int32_t* wp_ids, const int32_t* wp_off, int32_t n_seq,
                       const int32_t* span_off, const int32_t* span_tok, const int32_t* bm_ids, const int64_t* bm_off,
                       double k, double b, double avg_len, const int32_t* folder_id, const int32_t* index_folder_id,
                       const int64_t* created, const int64_t* modified, int64_t* out_first_row) {
  VR_TRY(check_mem(mem));
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
  VR_CHECK(encoder_out_dim(e) == e->dim, "encoder width %d != store dimension %d", encoder_out_dim(e), e->dim);
  VR_TRY(e->enc_out.grow(n * e->dim, 0, e->stream));
  if (span_off)
    VR_TRY(encoder_encode_spans(e, wp_ids, wp_off, n_seq, span_off, span_tok, mem, n, e->enc_out.p, VR_MEM_DEVICE));
  else
    VR_TRY(encoder_encode(e, wp_ids, wp_off, n_seq, mem, e->enc_out.p, VR_MEM_DEVICE));
  // 3. store: the only part searches wait for (they ran beside the encode)
  PublishLock publish(e);
  return upsert_locked(e, n, VR_MEM_DEVICE, e->enc_out.p, bm_off_dev, bm_off ? e->bm_idx.p : nullptr,
                       bm_off ? e->bm_val.p : nullptr, bm_off ? e->bm_cnt.p : nullptr, folder_id,
                       index_folder_id, created, modified, out_first_row);
}

extern "C" {

int vr_upsert(vr_engine* e, int64_t n, int mem, const float* dense, const int64_t* sp_off,
              const int32_t* sp_idx, const float* sp_val, const int32_t* folder_id,
              const int32_t* index_folder_id, const int64_t* created, const int64_t* modified,
              int64_t* out_first_row) {
  VR_TRY(check_engine(e));
  VR_CHECK(n >= 0, "negative row count");
  VR_TRY(check_mem(mem));
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
  VR_CHECK(n >= 0 && n <= INT32_MAX && (n == 0 || (wp_ids && wp_off)), "bad arguments");
  return index_batch(e, n, mem, wp_ids, wp_off, static_cast<int32_t>(n), nullptr, nullptr, bm_ids, bm_off, k, b, avg_len,
                     folder_id, index_folder_id, created, modified, out_first_row);
}

int vr_index_batch_spans(vr_engine* e, int64_t n, int mem, const int32_t* wp_ids, const int32_t* wp_off, int32_t n_seq,
                         const int32_t* span_off, const int32_t* span_tok, const int32_t* bm_ids, const int64_t* bm_off,
                         double k, double b, double avg_len, const int32_t* folder_id, const int32_t* index_folder_id,
                         const int64_t* created, const int64_t* modified, int64_t* out_first_row) {
  VR_TRY(check_engine(e));
  VR_CHECK(n >= 0 && n_seq >= 0 && span_off && (n == 0 || (n_seq > 0 && wp_ids && wp_off && span_tok)), "bad arguments");
  if (mem == VR_MEM_HOST)  // (device arrays: checked with the other span conditions, after the copy)
    VR_CHECK(span_off[n_seq] == n, "%lld rows announced, span_off holds %d spans", static_cast<long long>(n), span_off[n_seq]);
  return index_batch(e, n, mem, wp_ids, wp_off, n_seq, span_off, span_tok, bm_ids, bm_off, k, b, avg_len, folder_id,
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

extern "C" {

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

int vr_merge_keys(vr_engine* e, const uint64_t* parts, int32_t n_parts, int32_t n_lists, int32_t k, int mem, int64_t* out_ids,
                  float* out_scores, int32_t* out_counts) {
  VR_TRY(check_engine(e));
  VR_CHECK(parts && out_ids && out_scores && n_parts >= 1 && n_lists >= 1 && k >= 1, "bad arguments");
  VR_TRY(check_mem(mem));
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
  VR_TRY(check_mem(mem));
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
  VR_TRY(check_mem(mem));
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
