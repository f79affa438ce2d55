// Maximal marginal relevance over candidate lists of stored rows (vr_mmr_select).
//
// Per list of K candidates (first-stage order, relevance rel_i in f64, diversity d):
//   sim(i, j) = the f32 dense score of stored row c_i against stored row c_j (the k-ordered fmaf chain of a search score)
//   step 1 picks the largest (1 - d) * rel_i, every later step the largest (1 - d) * rel_i - d * (double) m_i, where m_i is
//   the f32 maximum of sim(i, s) over the picks s so far; f64 operations rounded one at a time, ties to the lower position.
//
// Three kernels per slice of lists:
//   mmr_gather_kernel  the candidates' rows, copied from the tiled corpus into a workspace in the same MFMA-tiled layout
//                      (every list padded to whole 16-row tiles, zero rows behind its last candidate)
//   mmr_gram_kernel    per (list, tile column I) the 16 candidates of tile I as the query image in LDS, and tiles J >= I of
//                      the list swept with dense.hip's scan_tile: the Gram is bit for bit the search score, by construction.
//                      Tile pairs J < I are the mirror image (products commute inside an fma: sim is symmetric bit for bit)
//   mmr_select_kernel  one workgroup per list; a thread owns <= 4 candidates (m_i, rel_i in registers), every step is a
//                      block-wide argmax over (mmr desc, position asc), and the pick's Gram row updates every m_i
//
// Workspace per list: K_pad * D * 4 bytes of rows plus K_pad^2 * 4 of Gram (K_pad = K rounded up to 16). A batch whose
// lists need more than the budget (VR_MMR_WORKSPACE_MB, read at every call, default 256) runs in slices of lists, so the
// workspace never asks hipMalloc for more than about twice the budget, whatever the batch.

#include "engine_internal.h"
#include "dense_device.h"

#include <algorithm>
#include <climits>
#include <cstdlib>

namespace vr {

// One wave per 1-KiB block (workspace tile T, k block kb): lane p holds the float4 at p = tile_pos(g, r) of candidate
// 16 * t + r, read from that row's block of the corpus (the 64 bytes a row owns of a block are contiguous).
__global__ __launch_bounds__(256) void mmr_gather_kernel(const float4* __restrict__ corpus, const int64_t* __restrict__ rows,
                                                         const MmrList* __restrict__ lists,
                                                         const int32_t* __restrict__ tile_list, int kblocks,
                                                         int64_t n_blocks, float4* __restrict__ ws) {
  const int lane = threadIdx.x & 63;
  const int64_t blk = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (blk >= n_blocks) return;
  const int64_t T = blk / kblocks;
  const int kb = static_cast<int>(blk % kblocks);
  const MmrList L = lists[tile_list[T]];
  const int r = lane >> 2, g = lane & 3;  // lane == tile_pos(g, r)
  const int64_t c = (T - L.tile0) * kTileRows + r;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < L.k) {
    const int64_t row = rows[L.row_off + c];
    v = corpus[((row / kTileRows) * kblocks + kb) * 64 + tile_pos(g, static_cast<int>(row % kTileRows))];
  }
  ws[(T * kblocks + kb) * 64 + lane] = v;
}

// One block per (list, tile column I): the LDS image holds candidates 16 I .. 16 I + 15 as the B operand (lane g * 16 + r
// of k block kb = their floats 16 kb + 4 c + g, query_image_kernel's layout), the four waves sweep tiles J = I, I + 1, ...
__global__ __launch_bounds__(256) void mmr_gram_kernel(const float4* __restrict__ ws, const MmrList* __restrict__ lists,
                                                       const int2* __restrict__ pairs, int kblocks, float* __restrict__ gram) {
  extern __shared__ float4 img[];
  const int2 pr = pairs[blockIdx.x];
  const MmrList L = lists[pr.x];
  const int I = pr.y;
  const float4* tiles = ws + L.tile0 * kblocks * 64;
  for (int i = threadIdx.x; i < kblocks * 64; i += 256) {
    const int kb = i >> 6, l = i & 63;
    img[i] = tiles[(static_cast<int64_t>(I) * kblocks + kb) * 64 + tile_pos(l >> 4, l & 15)];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t kpad = static_cast<int64_t>(L.ntiles) * kTileRows;
  float* G = gram + L.gram_off;
  for (int J = I + wave; J < L.ntiles; J += 4) {
    const f32x4 acc = scan_tile(tiles + static_cast<int64_t>(J) * kblocks * 64 + tile_pos(lane >> 4, lane & 15), img, kblocks,
                                lane);
    // C/D map of the 16x16 MFMA: column (candidate of tile I) = lane & 15, rows (candidates of tile J) = 4 (lane >> 4) + reg
    const int64_t b = static_cast<int64_t>(I) * kTileRows + (lane & 15);
    const int64_t a0 = static_cast<int64_t>(J) * kTileRows + (lane >> 4) * 4;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      G[(a0 + reg) * kpad + b] = acc[reg];
      if (J != I) G[b * kpad + a0 + reg] = acc[reg];
    }
  }
}

__device__ __forceinline__ void mmr_better(double& v, int& p, double ov, int op) {
  if (ov > v || (ov == v && op < p)) {
    v = ov;
    p = op;
  }
}

// One workgroup per list. Candidate pos belongs to thread pos % (64 WAVES), slot pos / (64 WAVES).
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64) void mmr_select_kernel(const MmrList* __restrict__ lists,
                                                                const double* __restrict__ rel,
                                                                const float* __restrict__ gram, int32_t* __restrict__ out) {
  constexpr int kThreads = WAVES * 64;
  __shared__ double red_v[2][WAVES];
  __shared__ int red_p[2][WAVES];
  const MmrList L = lists[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double d = L.d;
  const double keep = __dsub_rn(1.0, d);
  const int64_t kpad = static_cast<int64_t>(L.ntiles) * kTileRows;
  const float* G = gram + L.gram_off;
  double a[4];
  float m[4];
  unsigned open = 0;  // bit s: slot s holds a candidate not picked yet
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int pos = tid + s * kThreads;
    a[s] = 0.0;
    m[s] = -__builtin_inff();
    if (pos < L.k) {
      a[s] = __dmul_rn(keep, rel[L.row_off + pos]);
      open |= 1u << s;
    }
  }
  for (int step = 0; step < L.count; ++step) {
    double bv = -__builtin_inf();
    int bp = INT_MAX;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (open & (1u << s)) {
        const double v = step == 0 ? a[s] : __dsub_rn(a[s], __dmul_rn(d, static_cast<double>(m[s])));
        mmr_better(bv, bp, v, tid + s * kThreads);
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mmr_better(bv, bp, __shfl_xor(bv, off), __shfl_xor(bp, off));
    if (WAVES > 1) {  // (buffers alternate by step: one barrier per step)
      if (lane == 0) {
        red_v[step & 1][wave] = bv;
        red_p[step & 1][wave] = bp;
      }
      __syncthreads();
      bv = red_v[step & 1][0];
      bp = red_p[step & 1][0];
#pragma unroll
      for (int w = 1; w < WAVES; ++w) mmr_better(bv, bp, red_v[step & 1][w], red_p[step & 1][w]);
    }
    const int pick = bp;
    if (tid == 0) out[L.out_off + step] = pick;
    if (step + 1 == L.count) break;
    const float* row = G + static_cast<int64_t>(pick) * kpad;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int pos = tid + s * kThreads;
      if (pos == pick) open &= ~(1u << s);
      if (open & (1u << s)) m[s] = fmaxf(m[s], row[pos]);
    }
  }
}

static int64_t mmr_budget_bytes() {
  const char* s = getenv("VR_MMR_WORKSPACE_MB");
  const long long mb = s && *s ? atoll(s) : 256;
  return std::min<long long>(std::max<long long>(mb, 1), 1ll << 20) << 20;  // [1 MiB, 1 TiB]: no overflow in the shift
}

int mmr_select_run(vr_engine* e, int32_t n_lists, const int64_t* list_off, const int64_t* rows, const double* relevance,
                   const double* diversity, const int32_t* limits, int32_t out_stride, int32_t* out_pos) {
  const int64_t budget = mmr_budget_bytes();
  const int64_t row_bytes = static_cast<int64_t>(e->kblocks) * 1024;  // one 16-row tile of the workspace
  std::vector<int32_t> todo;  // lists with at least one pick
  for (int32_t i = 0; i < n_lists; ++i)
    if (limits[i] > 0 && list_off[i + 1] > list_off[i]) todo.push_back(i);
  size_t at = 0;
  while (at < todo.size()) {
    // a slice: as many lists as the budget holds (always at least one)
    std::vector<MmrList> lists;
    std::vector<int32_t> tile_list;
    std::vector<int2> pairs;
    std::vector<int64_t> srows;
    std::vector<double> srel;
    int64_t bytes = 0, gram = 0, outs = 0, max_k = 0;
    const size_t first = at;
    for (; at < todo.size(); ++at) {
      const int32_t i = todo[at];
      const int64_t k = list_off[i + 1] - list_off[i];
      const int32_t nt = static_cast<int32_t>((k + kTileRows - 1) / kTileRows);
      const int64_t kpad = static_cast<int64_t>(nt) * kTileRows;
      const int64_t need = nt * row_bytes + kpad * kpad * 4;
      if (at > first && bytes + need > budget) break;
      MmrList L;
      L.row_off = static_cast<int64_t>(srows.size());
      L.tile0 = static_cast<int64_t>(tile_list.size());
      L.gram_off = gram;
      L.out_off = outs;
      L.d = diversity[i];
      L.k = static_cast<int32_t>(k);
      L.count = static_cast<int32_t>(std::min<int64_t>(limits[i], k));
      L.ntiles = nt;
      L.pad = 0;
      const int32_t li = static_cast<int32_t>(lists.size());
      for (int32_t t = 0; t < nt; ++t) {
        tile_list.push_back(li);
        pairs.push_back(make_int2(li, t));
      }
      srows.insert(srows.end(), rows + list_off[i], rows + list_off[i + 1]);
      srel.insert(srel.end(), relevance + list_off[i], relevance + list_off[i + 1]);
      gram += kpad * kpad;
      outs += L.count;
      bytes += need;
      max_k = std::max(max_k, k);
      lists.push_back(L);
    }
    const int64_t n_tiles = static_cast<int64_t>(tile_list.size());
    const int nl = static_cast<int>(lists.size());
    hipStream_t st = e->stream;
    VR_TRY(e->mmr_ws.grow(n_tiles * e->kblocks * 256, 0, st));
    VR_TRY(e->mmr_gram.grow(gram, 0, st));
    VR_TRY(e->mmr_rows.grow(static_cast<int64_t>(srows.size()), 0, st));
    VR_TRY(e->mmr_rel.grow(static_cast<int64_t>(srel.size()), 0, st));
    VR_TRY(e->mmr_lists.grow(nl, 0, st));
    VR_TRY(e->mmr_tiles.grow(n_tiles, 0, st));
    VR_TRY(e->mmr_pairs.grow(n_tiles, 0, st));
    VR_TRY(e->mmr_out.grow(std::max<int64_t>(outs, 1), 0, st));
    VR_HIP(hipMemcpyAsync(e->mmr_rows.p, srows.data(), sizeof(int64_t) * srows.size(), hipMemcpyHostToDevice, st));
    VR_HIP(hipMemcpyAsync(e->mmr_rel.p, srel.data(), sizeof(double) * srel.size(), hipMemcpyHostToDevice, st));
    VR_HIP(hipMemcpyAsync(e->mmr_lists.p, lists.data(), sizeof(MmrList) * lists.size(), hipMemcpyHostToDevice, st));
    VR_HIP(hipMemcpyAsync(e->mmr_tiles.p, tile_list.data(), sizeof(int32_t) * tile_list.size(), hipMemcpyHostToDevice, st));
    VR_HIP(hipMemcpyAsync(e->mmr_pairs.p, pairs.data(), sizeof(int2) * pairs.size(), hipMemcpyHostToDevice, st));
    const int64_t n_blocks = n_tiles * e->kblocks;
    hipLaunchKernelGGL(mmr_gather_kernel, dim3(static_cast<unsigned>((n_blocks + 3) / 4)), dim3(256), 0, st,
                       reinterpret_cast<const float4*>(e->corpus.p), e->mmr_rows.p, e->mmr_lists.p, e->mmr_tiles.p,
                       e->kblocks, n_blocks, reinterpret_cast<float4*>(e->mmr_ws.p));
    VR_HIP(hipGetLastError());
    const size_t lds = static_cast<size_t>(e->kblocks) * 1024;  // <= 64 KiB (dim <= kMaxDim)
    hipLaunchKernelGGL(mmr_gram_kernel, dim3(static_cast<unsigned>(n_tiles)), dim3(256), lds, st,
                       reinterpret_cast<const float4*>(e->mmr_ws.p), e->mmr_lists.p, e->mmr_pairs.p, e->kblocks,
                       e->mmr_gram.p);
    VR_HIP(hipGetLastError());
    // threads per list: 4 candidates each (max_k <= kMaxK = 1024 -> at most 4 waves)
    if (max_k <= 256)
      hipLaunchKernelGGL(mmr_select_kernel<1>, dim3(nl), dim3(64), 0, st, e->mmr_lists.p, e->mmr_rel.p, e->mmr_gram.p,
                         e->mmr_out.p);
    else if (max_k <= 512)
      hipLaunchKernelGGL(mmr_select_kernel<2>, dim3(nl), dim3(128), 0, st, e->mmr_lists.p, e->mmr_rel.p, e->mmr_gram.p,
                         e->mmr_out.p);
    else
      hipLaunchKernelGGL(mmr_select_kernel<4>, dim3(nl), dim3(256), 0, st, e->mmr_lists.p, e->mmr_rel.p, e->mmr_gram.p,
                         e->mmr_out.p);
    VR_HIP(hipGetLastError());
    std::vector<int32_t> picked(static_cast<size_t>(outs));
    if (outs > 0)
      VR_HIP(hipMemcpyAsync(picked.data(), e->mmr_out.p, sizeof(int32_t) * picked.size(), hipMemcpyDeviceToHost, st));
    VR_HIP(hipStreamSynchronize(st));
    for (int li = 0; li < nl; ++li) {
      const int32_t i = todo[first + static_cast<size_t>(li)];
      memcpy(out_pos + static_cast<int64_t>(i) * out_stride, picked.data() + lists[li].out_off,
             sizeof(int32_t) * static_cast<size_t>(lists[li].count));
    }
  }
  return 0;
}

}  // namespace vr
