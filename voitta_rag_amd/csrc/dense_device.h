// Device half of the dense scorer shared by the translation units that score MFMA-tiled rows (dense.hip, mmr.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace vr {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kScoreUnroll = 8;

// scores of one 16-row tile against the <=16 queries of the LDS image: D/4 back-to-back
// v_mfma_f32_16x16x4_f32 on one accumulator = the k-ordered f32 fma chain of every (row, query).
__device__ __forceinline__ f32x4 scan_tile(const float4* __restrict__ src,
                                           const float4* __restrict__ q_lds, int kblocks, int lane) {
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  int kb = 0;
  for (; kb + kScoreUnroll <= kblocks; kb += kScoreUnroll) {
    float4 a[kScoreUnroll];
#pragma unroll
    for (int u = 0; u < kScoreUnroll; ++u) a[u] = src[(kb + u) * 64];
#pragma unroll
    for (int u = 0; u < kScoreUnroll; ++u) {
      float4 b = q_lds[(kb + u) * 64 + lane];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].x, b.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].y, b.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].z, b.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u].w, b.w, acc, 0, 0, 0);
    }
  }
  for (; kb < kblocks; ++kb) {
    float4 a = src[kb * 64];
    float4 b = q_lds[kb * 64 + lane];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
  }
  return acc;
}

}  // namespace vr
