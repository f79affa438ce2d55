// Search-time predicate over the numeric payload columns kept in HBM. Restates
// VectorStoreService._build_filter (reference: src/voitta/services/vector_store.py:462-530):
//   must     folder_path == folder_filter           (:476-482)
//   must     folder_path in include_folders         (:484-490)
//   must_not folder_path == each exclude_folders    (:492-499)
//   must_not index_folder == each exclude_index_folders (:501-508)
//   must     gte/lte range on source_modified_at (default) or source_created_at (:510-523);
//            a row lacking the field fails the range (SURVEY.md a14 [EXT]).
// Folder strings are dictionary ids (exact string equality in the reference == id equality),
// so the host folds the id lists into one pass/fail byte per dictionary id and the kernel is a
// single streaming pass: 1 + 4 + 4 (+ 8) bytes per row, HBM bound.

#include "engine_internal.h"

#include <algorithm>

namespace vr {

__global__ void filter_mask_kernel(const uint8_t* __restrict__ live,
                                   const int32_t* __restrict__ folder,
                                   const int32_t* __restrict__ index_folder,
                                   const int64_t* __restrict__ ts, const uint8_t* __restrict__ pass_f,
                                   const uint8_t* __restrict__ pass_if, int has_lo, int has_hi,
                                   int64_t lo, int64_t hi, int64_t n, uint8_t* __restrict__ mask) {
  int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool ok = live[i] != 0;
  if (pass_f) ok = ok && pass_f[folder[i]];
  if (pass_if) ok = ok && pass_if[index_folder[i]];
  if (has_lo | has_hi) {
    int64_t t = ts[i];
    ok = ok && t != VR_TS_ABSENT;
    if (has_lo) ok = ok && t >= lo;
    if (has_hi) ok = ok && t <= hi;
  }
  mask[i] = ok ? 1 : 0;
}

// The host half of a filter: one pass byte per dictionary id of folder_path (`pass_f`) and of index_folder (`pass_if`);
// an inactive condition leaves its table empty. Returns 1 when any condition is active.
static int filter_pass_tables(const vr_engine* e, const vr_filter* f, std::vector<uint8_t>* pass_f,
                              std::vector<uint8_t>* pass_if, bool* active) {
  pass_f->clear();
  pass_if->clear();
  *active = false;
  if (!f) return 0;
  VR_CHECK(f->struct_size == static_cast<int32_t>(sizeof(vr_filter)), "vr_filter size mismatch");
  const bool folder_active = f->n_must_folder_sets > 0 || f->n_not_folder > 0;
  const bool ifolder_active = f->n_not_index_folder > 0;
  const bool date_active = f->has_date_start || f->has_date_end;
  if (!folder_active && !ifolder_active && !date_active) return 0;
  if (e->n_rows == 0) return 0;
  VR_CHECK(f->n_must_folder_sets >= 0 && f->n_must_folder_sets <= 2, "at most 2 must-sets");
  *active = true;
  if (folder_active) {
    const int64_t nf = static_cast<int64_t>(e->max_folder_id) + 1;
    std::vector<uint8_t>& pass = *pass_f;
    pass.assign(static_cast<size_t>(nf), 1);
    for (int s = 0; s < f->n_must_folder_sets; ++s) {
      std::vector<uint8_t> in(static_cast<size_t>(nf), 0);
      for (int32_t j = f->must_folder_off[s]; j < f->must_folder_off[s + 1]; ++j) {
        int32_t id = f->must_folder_ids[j];
        if (id >= 0 && id < nf) in[static_cast<size_t>(id)] = 1;
      }
      for (int64_t i = 0; i < nf; ++i) pass[static_cast<size_t>(i)] &= in[static_cast<size_t>(i)];
    }
    for (int32_t j = 0; j < f->n_not_folder; ++j) {
      int32_t id = f->not_folder_ids[j];
      if (id >= 0 && id < nf) pass[static_cast<size_t>(id)] = 0;
    }
  }
  if (ifolder_active) {
    const int64_t nf = static_cast<int64_t>(e->max_index_folder_id) + 1;
    std::vector<uint8_t>& pass = *pass_if;
    pass.assign(static_cast<size_t>(nf), 1);
    for (int32_t j = 0; j < f->n_not_index_folder; ++j) {
      int32_t id = f->not_index_folder_ids[j];
      if (id >= 0 && id < nf) pass[static_cast<size_t>(id)] = 0;
    }
  }
  return 0;
}

int filter_build_mask(vr_engine* e, const vr_filter* f, const uint8_t** mask_out) {
  *mask_out = e->live.p;
  std::vector<uint8_t> pass_f, pass_if;
  bool active = false;
  VR_TRY(filter_pass_tables(e, f, &pass_f, &pass_if, &active));
  if (!active) return 0;
  const bool folder_active = f->n_must_folder_sets > 0 || f->n_not_folder > 0;
  const bool ifolder_active = f->n_not_index_folder > 0;

  const uint8_t* pf = nullptr;
  const uint8_t* pif = nullptr;
  if (folder_active) {
    const int64_t nf = static_cast<int64_t>(pass_f.size());
    VR_TRY(e->pass_folder.grow(nf, 0, e->stream));
    VR_HIP(hipMemcpyAsync(e->pass_folder.p, pass_f.data(), static_cast<size_t>(nf),
                          hipMemcpyHostToDevice, e->stream));
    VR_HIP(hipStreamSynchronize(e->stream));  // `pass_f` goes out of scope
    pf = e->pass_folder.p;
  }
  if (ifolder_active) {
    const int64_t nf = static_cast<int64_t>(pass_if.size());
    VR_TRY(e->pass_ifolder.grow(nf, 0, e->stream));
    VR_HIP(hipMemcpyAsync(e->pass_ifolder.p, pass_if.data(), static_cast<size_t>(nf),
                          hipMemcpyHostToDevice, e->stream));
    VR_HIP(hipStreamSynchronize(e->stream));
    pif = e->pass_ifolder.p;
  }
  VR_TRY(e->mask.grow(e->cap_rows, 0, e->stream));
  // rows past n_rows in the last 16-row tile must read as excluded
  {
    int64_t tail = e->cap_rows - e->n_rows;
    if (tail > 64) tail = 64;
    if (tail > 0)
      VR_HIP(hipMemsetAsync(e->mask.p + e->n_rows, 0, static_cast<size_t>(tail), e->stream));
  }
  const int64_t* ts = f->date_field == 1 ? e->created.p : e->modified.p;
  hipLaunchKernelGGL(filter_mask_kernel, dim3(static_cast<unsigned>((e->n_rows + 255) / 256)),
                     dim3(256), 0, e->stream, e->live.p, e->folder.p, e->index_folder.p, ts, pf, pif,
                     f->has_date_start, f->has_date_end, f->date_start, f->date_end, e->n_rows,
                     e->mask.p);
  VR_HIP(hipGetLastError());
  *mask_out = e->mask.p;
  return 0;
}

// ---- the classes of a filtered batch (vr_search_*_multi) as bit planes --------------------------------------------
// One pass over the payload columns evaluates up to kPlaneClasses classes per row (grid.y walks the rest): the
// predicate of filter_mask_kernel, term for term, per class, and a wave ballot turns the 64 answers of a wave into two
// words of the class's plane. The batched dense scan (batch.hip) then reads one word per 32 rows and query instead of a
// mask byte per row.
constexpr int kPlaneClasses = 8;

__global__ __launch_bounds__(256) void filter_planes_kernel(const uint8_t* __restrict__ live,
                                                            const int32_t* __restrict__ folder,
                                                            const int32_t* __restrict__ index_folder,
                                                            const int64_t* __restrict__ modified,
                                                            const int64_t* __restrict__ created,
                                                            const uint8_t* __restrict__ pass, const ClassDesc* __restrict__ cls,
                                                            int n_cls, int64_t n_rows, int64_t words,
                                                            uint32_t* __restrict__ planes) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;  // (the grid covers words x 32 rows exactly)
  const bool in = i < n_rows;
  const bool lv = in && live[i] != 0;
  const int32_t fo = in ? folder[i] : 0, ifo = in ? index_folder[i] : 0;
  const int64_t tm = in ? modified[i] : VR_TS_ABSENT, tc = in ? created[i] : VR_TS_ABSENT;
  const int c1 = min(n_cls, static_cast<int>(blockIdx.y + 1) * kPlaneClasses);
  for (int c = blockIdx.y * kPlaneClasses; c < c1; ++c) {
    const ClassDesc d = cls[c];
    bool ok = lv;
    if (d.pass_folder >= 0) ok = ok && pass[d.pass_folder + fo];
    if (d.pass_ifolder >= 0) ok = ok && pass[d.pass_ifolder + ifo];
    if (d.has_lo | d.has_hi) {
      const int64_t t = d.date_field == 1 ? tc : tm;
      ok = ok && t != VR_TS_ABSENT;
      if (d.has_lo) ok = ok && t >= d.lo;
      if (d.has_hi) ok = ok && t <= d.hi;
    }
    const unsigned long long b = __ballot(ok);
    if ((threadIdx.x & 63) == 0) {  // i % 64 == 0
      uint32_t* dst = planes + static_cast<int64_t>(c) * words + i / 32;
      dst[0] = static_cast<uint32_t>(b);
      dst[1] = static_cast<uint32_t>(b >> 32);
    }
  }
}

int64_t filter_plane_words(const vr_engine* e) {
  return (e->cap_rows + 255) / 256 * 8;
}

int filter_build_planes(vr_engine* e, const vr_filter* const* filters, int n_cls, const uint32_t** planes_out) {
  const int64_t words = filter_plane_words(e);
  std::vector<ClassDesc> desc(static_cast<size_t>(n_cls));
  std::vector<uint8_t> pass, pf, pif;
  for (int c = 0; c < n_cls; ++c) {
    const vr_filter* f = filters[c];
    bool active = false;
    VR_TRY(filter_pass_tables(e, f, &pf, &pif, &active));
    ClassDesc& d = desc[static_cast<size_t>(c)];
    d = ClassDesc{-1, -1, 0, 0, 0, 0, 0, 0};
    if (!active) continue;
    VR_CHECK(pass.size() + pf.size() + pif.size() < static_cast<size_t>(INT32_MAX), "pass tables of the batch too large");
    if (!pf.empty()) {
      d.pass_folder = static_cast<int32_t>(pass.size());
      pass.insert(pass.end(), pf.begin(), pf.end());
    }
    if (!pif.empty()) {
      d.pass_ifolder = static_cast<int32_t>(pass.size());
      pass.insert(pass.end(), pif.begin(), pif.end());
    }
    d.has_lo = f->has_date_start;
    d.has_hi = f->has_date_end;
    d.lo = f->date_start;
    d.hi = f->date_end;
    d.date_field = f->date_field == 1 ? 1 : 0;
  }
  VR_TRY(e->cls_planes.grow(static_cast<int64_t>(n_cls) * words, 0, e->stream));
  VR_TRY(e->cls_desc.grow(n_cls, 0, e->stream));
  VR_TRY(e->cls_pass.grow(std::max<int64_t>(1, static_cast<int64_t>(pass.size())), 0, e->stream));
  VR_HIP(hipMemcpyAsync(e->cls_desc.p, desc.data(), sizeof(ClassDesc) * desc.size(), hipMemcpyHostToDevice, e->stream));
  if (!pass.empty())
    VR_HIP(hipMemcpyAsync(e->cls_pass.p, pass.data(), pass.size(), hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(filter_planes_kernel, dim3(static_cast<unsigned>(words * 32 / 256), static_cast<unsigned>((n_cls + kPlaneClasses - 1) / kPlaneClasses)),
                     dim3(256), 0, e->stream, e->live.p, e->folder.p, e->index_folder.p, e->modified.p, e->created.p,
                     e->cls_pass.p, e->cls_desc.p, n_cls, e->n_rows, words, e->cls_planes.p);
  VR_HIP(hipGetLastError());
  VR_HIP(hipStreamSynchronize(e->stream));  // `desc` and `pass` go out of scope
  *planes_out = e->cls_planes.p;
  return 0;
}

}  // namespace vr
