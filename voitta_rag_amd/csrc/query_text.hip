// A question as TEXT, one call (the MCP search tool's three calls — embed_query, sparse embed_query,
// vector_store.search: mcp_server.py:469-485 — without the trips through Python between them): vr_query_text,
// vr_query_text_batch and their Unigram twins. Tokenising on the host threads, one forward pass, then the searches
// of search.hip on a lane.

#include "search.h"

#include <algorithm>
#include <climits>

#include "host_parallel.h"

using namespace vr;

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
  VR_TRY(check_fusion_limit(limit, fusion));
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
  VR_CHECK(encoder_out_dim(e) == e->dim, "encoder width %d != store dimension %d", encoder_out_dim(e), e->dim);
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
    return hybrid_one_fused(L, q_dev, VR_MEM_DEVICE, stems.data(), ones.data(), nnz, limit, sparse_weight, fusion, mask, out_rows,
                            out_scores, out_from_dense, out_count);
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
  VR_TRY(check_fusion(fusion));
  VR_CHECK(max_len >= 2 && max_len <= 4096, "max_len %d", max_len);
  int max_limit = 0;
  for (int i = 0; i < n; ++i) {
    VR_CHECK(dense_texts[i] && dense_lens[i] >= 0, "dense text %d: null or negative length", i);
    VR_CHECK(!sparse_texts || !sparse_texts[i] || (sparse_lens && sparse_lens[i] >= 0), "sparse text %d: no length", i);
    VR_TRY(check_limit_at(limits, i, &max_limit));  // (in turn with the texts: the first bad entry is reported)
  }
  VR_TRY(check_out_stride(out_stride, max_limit));
  {
    QueryClasses qc;
    VR_TRY(classify_queries(filters, n_filters, filter_of_query, n, &qc));
  }
  VR_TRY(check_engine(e));
  VR_CHECK(encoder_out_dim(e) == e->dim, "encoder width %d != store dimension %d", encoder_out_dim(e), e->dim);
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

int vr_query_text_bpe(vr_engine* e, const vr_bpe* tokenizer, const char* dense_text, int64_t dense_len,
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

int vr_query_text_batch_bpe(vr_engine* e, const vr_bpe* tokenizer, int32_t n, const char* const* dense_texts,
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
