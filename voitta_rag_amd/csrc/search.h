// What api.hip and query_text.hip use of search.hip. Internal, like engine_internal.h.
#pragma once

#include "engine_internal.h"

namespace vr {

int check_engine(vr_engine* e);  // non-null, and its device made current

// Argument checks shared by the exports: each sets the error text and returns -1, or returns 0
inline int check_k(int k) {
  VR_CHECK(k >= 1 && k <= kMaxK, "k = %d not in 1..%d", k, kMaxK);
  return 0;
}
inline int check_mem(int mem) {
  VR_CHECK(mem == VR_MEM_HOST || mem == VR_MEM_DEVICE, "bad mem %d", mem);
  return 0;
}
inline int check_fusion(int32_t fusion) {
  VR_CHECK(fusion == VR_FUSION_MINMAX || fusion == VR_FUSION_RRF, "unknown fusion %d", fusion);
  return 0;
}
inline int check_fusion_limit(int limit, int32_t fusion) {  // the limit, then the fusion
  VR_CHECK(limit >= 1 && limit * 3 <= kMaxK, "limit = %d not in 1..%d", limit, kMaxK / 3);
  return check_fusion(fusion);
}
inline int check_limit_at(const int32_t* limits, int i, int* max_limit) {  // limits[i], and the running maximum
  VR_CHECK(limits[i] >= 1 && limits[i] <= kMaxK / 3, "limits[%d] = %d not in 1..%d", i, limits[i], kMaxK / 3);
  if (limits[i] > *max_limit) *max_limit = limits[i];
  return 0;
}
inline int check_out_stride(int32_t out_stride, int max_limit) {
  VR_CHECK(out_stride >= max_limit, "out_stride = %d is below the largest limit %d", out_stride, max_limit);
  return 0;
}
inline int check_limits(const int32_t* limits, int nq, int32_t out_stride, int* max_limit) {  // every limit, then the stride
  *max_limit = 0;
  for (int i = 0; i < nq; ++i) VR_TRY(check_limit_at(limits, i, max_limit));
  return check_out_stride(out_stride, *max_limit);
}
// the arrays of nq sparse queries and, with count_terms, the number of terms of each
inline int check_sparse_csr(const int64_t* off, const int32_t* idx, const float* val, int nq, bool count_terms = true) {
  VR_CHECK(off[nq] == off[0] || (idx && val), "null sparse queries");
  for (int i = 0; count_terms && i < nq; ++i)
    VR_CHECK(off[i + 1] >= off[i] && off[i + 1] - off[i] <= kMaxQueryTerms,
             "sparse query %d has %lld terms (0..%d supported)", i, static_cast<long long>(off[i + 1] - off[i]), kMaxQueryTerms);
  return 0;
}

// A search: takes a lane (waits for one when all are busy), the shared lock, and a fresh view of the index.
// device_input: the caller's buffers were produced on the stream bound to the master (vr_set_stream); the lane's
// stream is ordered behind it.
struct SearchLane {
  vr_engine* m;
  vr_engine* L = nullptr;
  std::shared_lock<std::shared_mutex> lock;
  explicit SearchLane(vr_engine* master) : m(master) {}
  int acquire(bool device_input);
  ~SearchLane();
};

// k ranking keys -> rows and scores (-1 / 0.0 where a key is 0); returns how many were set
int64_t decode_keys(const uint64_t* keys, int k, int64_t* rows, float* scores);

// The classes of a filtered batch: the distinct entries of `filters` its queries name (and "no filter"), numbered in
// order of first appearance. Everything is validated here, before any device work.
struct QueryClasses {
  std::vector<int32_t> of;               // per query: its class
  std::vector<const vr_filter*> filter;  // per class: its filter (nullptr: none)
};
int classify_queries(const vr_filter* filters, int n_filters, const int32_t* filter_of_query, int nq, QueryClasses* qc);

// Both legs of ONE hybrid query on lane L (hybrid_one_query) and the fusion of the two pinned lists; k = 3 x limit
int hybrid_one_fused(vr_engine* L, const float* q, int mem, const int32_t* q_idx, const float* q_val, int nnz, int limit,
                     double sparse_weight, int32_t fusion, const uint8_t* mask, int64_t* out_rows, double* out_scores,
                     int32_t* out_from_dense, int32_t* out_count);

// The legs of a filtered batch on lane L, and the fusion of a hybrid one (search.hip has the details)
int dense_multi_keys(vr_engine* L, const float* q, int nq, int mem, int k, const QueryClasses& qc, uint64_t* keys_host);
int hybrid_multi_keys(vr_engine* L, const float* q, int nq, int mem, const int64_t* sq_off, const int32_t* sq_idx,
                      const float* sq_val, const int32_t* limits, const QueryClasses& qc, int kstride, uint64_t* dense,
                      uint64_t* sparse);
int fuse_multi(const uint64_t* dense, const uint64_t* sparse, int nq, int kstride, const int32_t* limits,
               const double* sparse_weights, int32_t fusion, const int32_t* out_row, int32_t out_stride, int64_t* out_rows,
               double* out_scores, int32_t* out_from_dense, int32_t* out_counts);

}  // namespace vr
