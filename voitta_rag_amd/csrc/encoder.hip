// Dense encode on the GPU: the BERT-family forward that SentenceTransformer.encode runs for the
// reference (call sites: src/voitta/services/embedding.py:40,53,68-73,85; SURVEY.md a4 [EXT]).
//
// Layout: sequences are PACKED — activations are [T, H] over the T real tokens of a batch, with
// an offsets array (cu) marking sequence boundaries. No padding rows exist, so no FLOP or byte is
// spent on them (sentence-transformers pads to the longest sequence of each 32-batch; padding
// never changes a result because masked logits underflow to exactly 0).
//
// Kernels (all f32; the matrix products run on the f32-input MFMA, which is an exact f32 fma
// chain, so the only differences from the torch-CPU reference are summation orders):
//   embed_ln_kernel   word+position+type gather, LayerNorm           HBM bound, 2*H*4 B/token
//   gemm_f32_kernel   C = A W^T + b (+GELU | +residual)              MFMA bound (v_mfma_f32_32x32x2_f32)
//                     128x128x32 block tile, 4 waves of 64x64, register-staged double-buffered LDS
//   attention_kernel  softmax(Q K^T / sqrt(d)) V per (sequence, head) MFMA (v_mfma_f32_16x16x4_f32),
//                     online softmax, keys streamed through LDS 64 at a time
//   layernorm_kernel  LayerNorm over H                               HBM bound
//   pool_kernel       mean / CLS / last-token pooling + L2 normalise HBM bound
//   rerank_head_kernel cross-encoder head on the pooled [CLS] rows   one f32 logit per pair (encoder_rerank)
//   rerank_head_ln_kernel the head of a pre-norm cross-encoder: dense, GELU, LayerNorm, classifier (encoder_rerank)
//   gather_last_rows_kernel, rerank_head_rms_kernel  a decoder cross-encoder (vr_reranker_load_decoder): the last token's
//                     context and residual rows into [n_seq, .] matrices behind the last layer's attention, and the final
//                     RMSNorm with the dot product against score.weight, one f32 logit per pair (rerank_tail)
//   embed_head_kernel the embedder's post-pooling head: Dense / LayerNorm stages, normalise, truncate (vr_encoder_set_head)
//   unit_sum_kernel, unit_gap_kernel, unit_boundary_kernel, chunk_base_kernel, chunk_row_kernel, chunk_gather_kernel
//                     semantic chunking (vr_encode_semantic): unit sums, gap distances, boundaries, chunk rows (launch_semantic)
//   rope_kernel       rotary positions, in place on Q and K            HBM bound (VR_POS_ROTARY models only)
//   glu_kernel        act(gate) * up of a gated FFN                    HBM bound (VR_FFN_SWIGLU / VR_FFN_GEGLU only)
//   embed_rms_kernel, rmsnorm_kernel, rmsnorm_f16_kernel  the embedding gather and the norms of an RMSNorm pre-norm
//                     model (VR_NORM_PRE_RMS, the T5 encoder: forward_chunk_rms); its ReLU FFN is EPI_BIAS_RELU of the GEMMs.
//                     T5's logits carry no 1/sqrt(d_h): launch_attention keeps its scale, the loader folds sqrt(d_h) into
//                     the query weights (include/voitta_engine.h)
//                     The same kernels serve VR_NORM_PRE_RMS_ROTARY (the Qwen2 block: forward_chunk_rms_rotary), with rope_kernel,
//                     glu_kernel and the causal state of the three attention kernels (kMaskCausal)
// Algorithmic FLOP per token = L * (24 H^2 + 4 S H), of which the GEMMs are
// 24 H^2 L: the dominant kernel of the indexing path.

#include "engine_internal.h"

#include <map>
#include <tuple>

#include <algorithm>
#include <cmath>

namespace vr {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;

struct SplitWeight {  // f16x3 mode: w * 2^s as (hi, lo) f16, [out][in]; unscale = 2^-s
  _Float16* hi = nullptr;
  _Float16* lo = nullptr;
  float unscale = 1.0f;
};

struct LayerWeights {
  float *wqkv, *bqkv, *wo, *bo, *ln1g, *ln1b, *w1, *b1, *w2, *b2, *ln2g, *ln2b;
  SplitWeight s_qkv, s_o, s_1, s_2;
  // f16 mode, LayerNorm folded into the consuming GEMM (see EPI_FOLD_*): weights scaled by the LayerNorm
  // gain in front of them, their column sums and the bias with the LayerNorm shift pushed through
  SplitWeight s_qkv_f{}, s_1_f{};  // s_qkv_f: layers >= 1 only (layer 0 reads the embedding LayerNorm's output)
  float *cs_qkv = nullptr, *c_qkv = nullptr, *cs_1 = nullptr, *c_1 = nullptr;
  // f16 mode, fused rotary / gate epilogues of the skinny kernels (EPI_ROPE_F16, EPI_*GLU_F16): the same matrices with
  // their output rows re-ordered so that the two values an epilogue combines are neighbours. s_qkv_p: inside every
  // head of the query and key thirds, row 2i = old row i and row 2i + 1 = old row i + d_h/2 (q.k is invariant under a
  // common permutation inside a head; the value third is untouched). s_1_p: row 2j = gate_j, row 2j + 1 = up_j.
  SplitWeight s_qkv_p{}, s_1_p{};
  float *bqkv_p = nullptr, *b1_p = nullptr;
  // ... and of EPI_FOLD_*GLU: the interleaved FFN-up matrix scaled by the LayerNorm gain in front of it, its column
  // sums and folded bias (what s_1_f, cs_1, c_1 are to the stacked matrix)
  SplitWeight s_1_fp{};
  float *cs_1_p = nullptr, *c_1_p = nullptr;
  // vr_bert_desc_v3.qk_norm: q_norm.weight / k_norm.weight, [head_dim] each, shared by the heads (qk_norm_rope_kernel)
  float *qn = nullptr, *kn = nullptr;
  // the last layer of a [CLS]-pooled f16 model (cls_attend_kernel): the key third of s_qkv_f transposed, [H (in)][H (out)]
  _Float16* wk_t = nullptr;
};

// vr_encoder_set_head: the stages embed_head_kernel runs on the pooled rows (device pointers; a null b: no bias / shift)
constexpr int kMaxHeadStages = 4;
struct HeadStage {
  int kind, in_dim, out_dim, act;
  float eps;
  const float *w, *b;
};
struct HeadParams {
  int n_stages;
  HeadStage st[kMaxHeadStages];
};

struct Encoder {
  vr_bert_desc d{};
  float *word = nullptr, *pos = nullptr, *type = nullptr, *lng = nullptr, *lnb = nullptr;
  std::vector<LayerWeights> layers;
  std::vector<float*> owned;  // every device allocation, for release
  // workspace for up to ws_tokens packed tokens
  int64_t ws_tokens = 0;
  float *x = nullptr, *qkv = nullptr, *ctx = nullptr, *tmp = nullptr, *ffn = nullptr;
  float* xs = nullptr;  // f16x3 / f16 mode: the hidden state as GEMM input ((hi, lo) or plain f16 rows)
  float* lnstat = nullptr;  // f16 mode: two arrays of per-row (mean, 1/sigma), see forward_chunk
  float* lnpart = nullptr;  // f16 mode: per (row, 64 columns) partial (sum, sum of squares) of the folded LayerNorms
  float* glu = nullptr;     // gated FFN: the [T, 2I] pre-activation (gate | up) of glu_kernel, f32 or plain f16 rows
  // rotary positions: (cos, sin) of position p for the pair q = head * d_h/2 + i of a head-major [H/2] row (the d_h/2
  // frequencies repeated for every head, so that an epilogue finds its entry from the column alone), max_pos rows
  float2* rope = nullptr;
  float2* rope_local = nullptr;  // ... of the windowed layers' base (vr_bert_desc.rope_theta_local); null: they use `rope`
  // vr_encoder_set_attention_bias: [heads, 2 bias_radius + 1] f32, logit += bias[h][clamp(key - query) + bias_radius]
  float* bias = nullptr;
  int bias_radius = 0;
  // vr_encoder_set_attention_slopes: [heads] f32, logit -= slopes[h] |key - query|; never set together with `bias`
  float* slopes = nullptr;
  // vr_encoder_set_head: the stages behind pooling (weights in `owned`) and the output width they and the truncation
  // leave; has_head false: out_dim == d.hidden and every launch is the headless one. `pooled`: the un-normalised pooled
  // rows of a call with stages, one H-wide row per output row — the size of what the caller holds for the result.
  bool has_head = false;
  HeadParams head{};
  int out_dim = 0;
  DevArray<float> pooled;
  int causal = 0;               // vr_bert_desc_v2.causal: 1 = the attention kernels' causal state (VR_NORM_PRE_RMS_ROTARY only)
  // vr_bert_desc_v3: the head size (head_dim, or hidden / heads), the attention width A = heads * dh of the [Q | K | V]
  // rows and of the context (== hidden for every family but Qwen3), and whether Q and K are RMS-normalised per head
  int dh = 0, attn = 0, qk_norm = 0;
  int window_stream_from = 0;   // windowed layers: sequences from this length on take attention_stream_kernel (build_encoder)
  float* posidx = nullptr;  // rotary: int32 position of every token inside its own sequence (positions_kernel)
  bool cls_collapse = true;  // the last layer attends from [CLS] on the hidden rows; VR_CLS_COLLAPSE=0 at load time: it projects K and V
  bool fuse = true;         // rotate / gate inside the skinny epilogues; VR_ENCODE_FUSE=0 at load time: separate passes
  DevArray<int32_t> ids, cu, seg;
  // a span call (encoder_encode_spans): the caller's (begin, end) pairs when they come from the host, and every span's
  // sequence index (built on the host from span_off; its host copy lives here until the upload has run)
  DevArray<int32_t> span_tok, span_seq;
  std::vector<int32_t> span_seq_host;
  // a semantic call (encoder_encode_semantic): unit_off on the device, the unit sums S_r [units, H], per unit its gap
  // distance, chunk-start flag and chunk index inside its sequence (-1: no start), per sequence its chunk count and
  // first chunk row, the running chunk counter, and (a head with stages) the head's rows before they are compacted
  DevArray<int32_t> sem_off, sem_start, sem_idx, sem_seq_chunks, sem_seq_base, sem_counter;
  DevArray<float> sem_sums, sem_dist, sem_rows;
  DevArray<float> out;
  // a cross-encoder (the reranker slot): pooler dense [H,H] + bias, classifier [1,H] + bias; the pooled [CLS] rows
  // (a pre-norm one, ModernBertForSequenceClassification: pool_w / pool_b are its head.dense, head_ln_g / head_ln_b its
  // head.norm, and the pooled rows are CLS or mean rows of the final norm; null head_ln_g: the tanh pooler head)
  float *pool_w = nullptr, *pool_b = nullptr, *cls_w = nullptr, *cls_b = nullptr;
  float *head_ln_g = nullptr, *head_ln_b = nullptr;
  DevArray<float> rows;
  // a decoder cross-encoder (vr_reranker_load_decoder): score.weight [H], and the [n_seq, *] matrices of the last layer's
  // tail (RerankRows), grown by encoder_rerank before the pass — never inside a capture — and dropped with the graphs
  float* score_w = nullptr;
  DevArray<float> tail_ws;
  DevArray<float> skinny_ws;  // K-slice partial sums of gemm_f16_skinny_kernel
  // hipGraphs of small forward passes (a query, a handful of sequences): ~135 launches of a few
  // microseconds of work each are launch-bound; replayed as one graph they are not
  // (a span call: its span buffers and span count as well — a whole-sequence call has null and 0 there. The span
  // VALUES are not part of the key: they are copied into the buffers before every launch, as the ids are.)
  struct GraphKey {
    int T, n_seq, max_len;
    const void *ids, *cu, *seg, *out;
    const void *span_tok = nullptr, *span_seq = nullptr;
    int n_spans = 0;
    const void* pooled = nullptr;  // a head with stages: the scratch the pool kernels write and embed_head_kernel reads
    bool operator<(const GraphKey& o) const {
      return std::tie(T, n_seq, max_len, ids, cu, seg, out, span_tok, span_seq, n_spans, pooled) <
             std::tie(o.T, o.n_seq, o.max_len, o.ids, o.cu, o.seg, o.out, o.span_tok, o.span_seq, o.n_spans, o.pooled);
    }
  };
  struct GraphEntry {
    int seen = 0;
    bool bad = false;
    hipGraphExec_t exec = nullptr;
  };
  std::map<GraphKey, GraphEntry> graphs;
};

// captured graphs hold raw workspace pointers: every reallocation of a buffer they touch drops them
static void invalidate_graphs(Encoder* enc) {
  for (auto& kv : enc->graphs)
    if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
  enc->graphs.clear();
}

// ---- elementwise / normalisation ---------------------------------------------------------------

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

constexpr int kMaxPairs = 8;  // H <= 1024: H/128 float2 per lane

// ---- split precision (f16x3) ---------------------------------------------------------------------
// A GEMM operand v is carried as two f16 numbers, hi = f16(v) and lo = f16(v - hi): together 22
// significant bits. The product a*w is then a_hi*w_hi + a_hi*w_lo + a_lo*w_hi (the dropped
// a_lo*w_lo term is < 2^-22 relative), three passes of the f16 MFMA whose products are exact in
// its f32 accumulator — f32-class accuracy at 16/3 of the f32-MFMA rate. Activations are O(1) so
// they are split unscaled (absolute granularity 2^-24, f16's subnormal spacing); values beyond
// f16's range are clamped. Weights are pre-scaled by a power of two per tensor (exact).
using half_t = _Float16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;

__device__ __forceinline__ void split_f16(float v, half_t& hi, half_t& lo) {
  v = fminf(fmaxf(v, -65504.0f), 65504.0f);
  hi = static_cast<half_t>(v);
  lo = static_cast<half_t>(v - static_cast<float>(hi));
}

struct half2_t {
  half_t x, y;
};

// GELU(x) = 0.5 x (1 + erf(x / sqrt 2)) for the f16x3 epilogues, where erff() made the epilogue VALU-bound
// (a third of the FFN-up tile time). Abramowitz-Stegun 7.1.26: erfc(z) = t (a1 + t (a2 + ... a5 t)) e^{-z^2},
// t = 1 / (1 + p z), |error| <= 1.5e-7 — the size of an f32 ulp of erf, and far inside what the (hi, lo)
// split of the result keeps. Negative x uses 0.5 x erfc(|x| / sqrt 2) directly, so the tail has no
// cancellation. 13 instructions (one v_rcp_f32, one v_exp_f32) against ~40 for erff.
__device__ __forceinline__ float gelu_fast(float x) {
  const float z = fabsf(x) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
  float p = fmaf(1.061405429f, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  const float q = p * t * __builtin_amdgcn_exp2f(-1.4426950408889634f * z * z);  // erfc(z)
  return x >= 0.0f ? x * fmaf(-0.5f, q, 1.0f) : 0.5f * x * q;
}

// two elements at a time on the packed-f32 VALU (v_pk_fma_f32 / v_pk_mul_f32): same operations in the
// same order as gelu_fast, so the same bits
using f32x2 = __attribute__((ext_vector_type(2))) float;
__device__ __forceinline__ f32x2 gelu_fast2(f32x2 x) {
  const f32x2 z = __builtin_elementwise_abs(x) * 0.70710678118654752440f;
  const f32x2 d = __builtin_elementwise_fma(f32x2{0.3275911f, 0.3275911f}, z, f32x2{1.0f, 1.0f});
  const f32x2 t = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
  f32x2 p = __builtin_elementwise_fma(f32x2{1.061405429f, 1.061405429f}, t, f32x2{-1.453152027f, -1.453152027f});
  p = __builtin_elementwise_fma(p, t, f32x2{1.421413741f, 1.421413741f});
  p = __builtin_elementwise_fma(p, t, f32x2{-0.284496736f, -0.284496736f});
  p = __builtin_elementwise_fma(p, t, f32x2{0.254829592f, 0.254829592f});
  const f32x2 a = (-1.4426950408889634f * z) * z;
  const f32x2 q = (p * t) * f32x2{__builtin_amdgcn_exp2f(a.x), __builtin_amdgcn_exp2f(a.y)};
  const f32x2 pos = x * __builtin_elementwise_fma(f32x2{-0.5f, -0.5f}, q, f32x2{1.0f, 1.0f});
  const f32x2 neg = (0.5f * x) * q;
  return f32x2{x.x >= 0.0f ? pos.x : neg.x, x.y >= 0.0f ? pos.y : neg.y};
}

// GELU of the single-pass f16 mode: its output is rounded to f16 (relative 4.9e-4), so the two
// quarter-rate transcendentals of gelu_fast (rcp, exp2: half of its issue cycles, and the GELU epilogue
// was 15 % of the FFN-up GEMM) buy nothing. erf(x / sqrt 2) = w Q(w^2) with w = clamp(x, +-3 sqrt 2), Q a
// degree-9 polynomial (near-minimax fit, |erf error| <= 3.3e-6 inside the clamp, 2.2e-5 beyond it):
// relative error of the result <= 1.4e-5 for x > 0, absolute <= 0.5 |x| 2.2e-5 for x < 0.
__device__ __forceinline__ f32x2 gelu_poly2(f32x2 x) {
  constexpr float kClamp = 4.242640495300293f;
  const f32x2 w = {__builtin_amdgcn_fmed3f(x.x, -kClamp, kClamp), __builtin_amdgcn_fmed3f(x.y, -kClamp, kClamp)};
  const f32x2 s = w * w;
  f32x2 q = __builtin_elementwise_fma(f32x2{-5.183208029e-12f, -5.183208029e-12f}, s, f32x2{5.512241219e-10f, 5.512241219e-10f});
  q = __builtin_elementwise_fma(q, s, f32x2{-2.635556129e-08f, -2.635556129e-08f});
  q = __builtin_elementwise_fma(q, s, f32x2{7.569865943e-07f, 7.569865943e-07f});
  q = __builtin_elementwise_fma(q, s, f32x2{-1.478758622e-05f, -1.478758622e-05f});
  q = __builtin_elementwise_fma(q, s, f32x2{2.114593954e-04f, 2.114593954e-04f});
  q = __builtin_elementwise_fma(q, s, f32x2{-2.317534527e-03f, -2.317534527e-03f});
  q = __builtin_elementwise_fma(q, s, f32x2{1.985279098e-02f, 1.985279098e-02f});
  q = __builtin_elementwise_fma(q, s, f32x2{-1.329084933e-01f, -1.329084933e-01f});
  q = __builtin_elementwise_fma(q, s, f32x2{7.978681326e-01f, 7.978681326e-01f});
  const f32x2 hx = 0.5f * x;
  return __builtin_elementwise_fma(hx, w * q, hx);
}

// Four pairs at once, step by step across the pairs: the same operations per element as gelu_poly2 (same bits), but a
// dependent v_pk_fma_f32 chain issues one instruction per ~2 issue slots (the compiler pads every step with s_nop 0 and keeps
// the source order of the four chains): written pair by pair the polynomial of a 16 x 8 epilogue piece was 4 x 11 dependent
// steps; interleaved, the four chains fill each other's slots.
__device__ __forceinline__ void gelu_poly2x4(f32x2 (&x)[4]) {
  constexpr float kClamp = 4.242640495300293f;
  constexpr float kC[10] = {-5.183208029e-12f, 5.512241219e-10f, -2.635556129e-08f, 7.569865943e-07f, -1.478758622e-05f,
                            2.114593954e-04f,  -2.317534527e-03f, 1.985279098e-02f,  -1.329084933e-01f, 7.978681326e-01f};
  f32x2 w[4], s[4], q[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = f32x2{__builtin_amdgcn_fmed3f(x[i].x, -kClamp, kClamp), __builtin_amdgcn_fmed3f(x[i].y, -kClamp, kClamp)};
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] = w[i] * w[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = __builtin_elementwise_fma(f32x2{kC[0], kC[0]}, s[i], f32x2{kC[1], kC[1]});
#pragma unroll
  for (int c = 2; c < 10; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = __builtin_elementwise_fma(q[i], s[i], f32x2{kC[c], kC[c]});
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 hx = 0.5f * x[i];
    x[i] = __builtin_elementwise_fma(hx, w[i] * q[i], hx);
  }
}

// Split (hi, lo) matrices live in ONE interleaved array: row r of a [rows][K] matrix is 2K halfs,
// element k's hi at  r*2K + (k/8)*16 + k%8  and its lo 8 halfs further. A 128-byte line then holds
// 32 consecutive k of BOTH halves of one row — exactly what a 32-deep GEMM K-tile needs of that row,
// so the GEMM's global->LDS loads consume every line they touch (with separate hi and lo arrays a
// 32-deep K-tile used 64 bytes of each line and the L1 fetched every line twice).
// Callers pass hi = base and lo = base + 8; split_at() turns a column into the offset inside a row.
__host__ __device__ __forceinline__ int split_at(int k) { return ((k >> 3) << 4) + (k & 7); }

// one element of a LayerNorm output, exactly as row_layernorm computes it (same operations, same order)
__device__ __forceinline__ float ln_apply(float v, float mean, float inv, float g, float b) {
  return (v - mean) * inv * g + b;
}

// one element of an RMSNorm output (T5LayerNorm: no mean, no shift), the one expression every kernel that norms so uses
__device__ __forceinline__ float rms_apply(float v, float inv, float g) { return v * inv * g; }

// LayerNorm of one row held as float2 pairs per lane (biased variance, eps inside the sqrt).
// out_hi/out_lo (optional): the same row split for the f16x3 GEMMs.
// RMS (VR_NORM_PRE_RMS): x * rsqrt(mean(x^2) + eps) * g instead — one sum of squares in the same fixed order, no mean
// pass, and b is never read (it may be null); stat gets (0, 1/rms). RMS = false is the code that never knew the flag.
template <bool RMS = false>
__device__ __forceinline__ void row_layernorm(float2 (&v)[kMaxPairs], int pairs, int H,
                                              const float* __restrict__ g,
                                              const float* __restrict__ b, float eps, int lane,
                                              float* __restrict__ out, half_t* __restrict__ out_hi = nullptr,
                                              half_t* __restrict__ out_lo = nullptr,
                                              float2* __restrict__ stat = nullptr) {
  if constexpr (RMS) {
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < kMaxPairs; ++i)
      if (i < pairs) q += v[i].x * v[i].x + v[i].y * v[i].y;
    const float inv = 1.0f / sqrtf(wave_sum(q) / static_cast<float>(H) + eps);
    if (stat && lane == 0) *stat = make_float2(0.0f, inv);
#pragma unroll
    for (int i = 0; i < kMaxPairs; ++i)
      if (i < pairs) {
        int e = (i * 64 + lane) * 2;
        float2 gg = *reinterpret_cast<const float2*>(g + e);
        float2 o;
        o.x = rms_apply(v[i].x, inv, gg.x);
        o.y = rms_apply(v[i].y, inv, gg.y);
        if (out) *reinterpret_cast<float2*>(out + e) = o;
        if (out_hi) {
          half2_t h, l;
          split_f16(o.x, h.x, l.x);
          split_f16(o.y, h.y, l.y);
          if (out_lo) {
            *reinterpret_cast<half2_t*>(out_hi + split_at(e)) = h;
            *reinterpret_cast<half2_t*>(out_lo + split_at(e)) = l;
          } else {
            *reinterpret_cast<half2_t*>(out_hi + e) = h;
          }
        }
      }
    return;
  }
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < kMaxPairs; ++i)
    if (i < pairs) s += v[i].x + v[i].y;
  const float mean = wave_sum(s) / static_cast<float>(H);
  float q = 0.0f;
#pragma unroll
  for (int i = 0; i < kMaxPairs; ++i)
    if (i < pairs) {
      float dx = v[i].x - mean, dy = v[i].y - mean;
      q += dx * dx + dy * dy;
    }
  const float var = wave_sum(q) / static_cast<float>(H);
  const float inv = 1.0f / sqrtf(var + eps);
  // stat (optional): the row's (mean, 1/sigma) — whoever holds the pre-LN row can then re-derive the
  // f32 output with ln_apply() instead of reading it back (see forward_chunk, f16 mode)
  if (stat && lane == 0) *stat = make_float2(mean, inv);
#pragma unroll
  for (int i = 0; i < kMaxPairs; ++i)
    if (i < pairs) {
      int e = (i * 64 + lane) * 2;
      float2 gg = *reinterpret_cast<const float2*>(g + e);
      float2 bb = *reinterpret_cast<const float2*>(b + e);
      float2 o;
      o.x = (v[i].x - mean) * inv * gg.x + bb.x;
      o.y = (v[i].y - mean) * inv * gg.y + bb.y;
      if (out) *reinterpret_cast<float2*>(out + e) = o;
      if (out_hi) {
        half2_t h, l;
        split_f16(o.x, h.x, l.x);
        split_f16(o.y, h.y, l.y);
        if (out_lo) {  // interleaved (hi, lo) row
          *reinterpret_cast<half2_t*>(out_hi + split_at(e)) = h;
          *reinterpret_cast<half2_t*>(out_lo + split_at(e)) = l;
        } else {       // plain f16 row (VR_PRECISION_F16)
          *reinterpret_cast<half2_t*>(out_hi + e) = h;
        }
      }
    }
}

// one wave per token: x[t] = LayerNorm(word[id] + pos[p] + type[0]); SEG (a cross-encoder's pairs): type[1] for the
// positions p >= seg_b[sequence], the segment-B tokens. POS = false (a rotary model): word + type only, no table is read.
// (The body of embed_ln_kernel and embed_ln_rotary_kernel: two kernels, so that the former keeps its signature.)
// RMS (VR_NORM_PRE_RMS): `pre`, the raw row, is the residual stream; the norm (block 0's attention norm) is row_layernorm<true>.
template <bool SEG, bool POS, bool RMS = false>
__device__ __forceinline__ void embed_ln_body(const int32_t* __restrict__ ids,
                                              const int32_t* __restrict__ cu, int n_seq,
                                              int tok_base, int T, int H, int vocab,
                                              const float* __restrict__ word,
                                              const float* __restrict__ pos,
                                              const float* __restrict__ type,
                                              const float* __restrict__ g,
                                              const float* __restrict__ b, float eps,
                                              float* __restrict__ x, half_t* __restrict__ x_hi,
                                              half_t* __restrict__ x_lo, float* __restrict__ pre,
                                              float2* __restrict__ stat, const int32_t* __restrict__ seg_b) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  // position = index inside the sequence: binary search of the offsets
  int lo = 0, hi = n_seq;
  const int tg = t + tok_base;
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    if (cu[mid] <= tg) lo = mid; else hi = mid;
  }
  const int p = tg - cu[lo];
  int id = ids[tg];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  if (SEG && p >= seg_b[lo]) type += H;
  const int pairs = H / 128;
  float2 v[kMaxPairs];
#pragma unroll
  for (int i = 0; i < kMaxPairs; ++i)
    if (i < pairs) {
      int e = (i * 64 + lane) * 2;
      float2 w = *reinterpret_cast<const float2*>(word + static_cast<int64_t>(id) * H + e);
      float2 tt = *reinterpret_cast<const float2*>(type + e);
      if constexpr (POS) {
        float2 pp = *reinterpret_cast<const float2*>(pos + static_cast<int64_t>(p) * H + e);
        v[i].x = w.x + pp.x + tt.x;
        v[i].y = w.y + pp.y + tt.y;
      } else {
        v[i].x = w.x + tt.x;
        v[i].y = w.y + tt.y;
      }
      if (pre) *reinterpret_cast<float2*>(pre + static_cast<int64_t>(t) * H + e) = v[i];  // the pre-LN row
    }
  const int64_t o = static_cast<int64_t>(t) * H;
  row_layernorm<RMS>(v, pairs, H, g, b, eps, lane, x ? x + o : nullptr, x_hi ? x_hi + (x_lo ? 2 : 1) * o : nullptr,
                     x_lo ? x_lo + 2 * o : nullptr, stat ? stat + t : nullptr);
}

template <bool SEG>
__global__ __launch_bounds__(256) void embed_ln_kernel(const int32_t* __restrict__ ids,
                                                       const int32_t* __restrict__ cu, int n_seq,
                                                       int tok_base, int T, int H, int vocab,
                                                       const float* __restrict__ word,
                                                       const float* __restrict__ pos,
                                                       const float* __restrict__ type,
                                                       const float* __restrict__ g,
                                                       const float* __restrict__ b, float eps,
                                                       float* __restrict__ x, half_t* __restrict__ x_hi,
                                                       half_t* __restrict__ x_lo, float* __restrict__ pre,
                                                       float2* __restrict__ stat, const int32_t* __restrict__ seg_b) {
  embed_ln_body<SEG, true>(ids, cu, n_seq, tok_base, T, H, vocab, word, pos, type, g, b, eps, x, x_hi, x_lo, pre, stat, seg_b);
}

// a rotary model, or one without positions (VR_POS_NONE): no position table (and no segment B: cross-encoders are neither)
__global__ __launch_bounds__(256) void embed_ln_rotary_kernel(const int32_t* __restrict__ ids,
                                                              const int32_t* __restrict__ cu, int n_seq,
                                                              int tok_base, int T, int H, int vocab,
                                                              const float* __restrict__ word,
                                                              const float* __restrict__ type,
                                                              const float* __restrict__ g,
                                                              const float* __restrict__ b, float eps,
                                                              float* __restrict__ x, half_t* __restrict__ x_hi,
                                                              half_t* __restrict__ x_lo, float* __restrict__ pre,
                                                              float2* __restrict__ stat) {
  embed_ln_body<false, false>(ids, cu, n_seq, tok_base, T, H, vocab, word, nullptr, type, g, b, eps, x, x_hi, x_lo, pre, stat,
                              nullptr);
}

// VR_NORM_PRE_RMS (T5): pre[t] = word[id] + type[0], the residual stream as it is; x / x_hi / x_lo = RMSNorm(pre[t]) by g,
// the rows block 0's Q/K/V projection reads
__global__ __launch_bounds__(256) void embed_rms_kernel(const int32_t* __restrict__ ids,
                                                        const int32_t* __restrict__ cu, int n_seq,
                                                        int tok_base, int T, int H, int vocab,
                                                        const float* __restrict__ word,
                                                        const float* __restrict__ type,
                                                        const float* __restrict__ g, float eps,
                                                        float* __restrict__ x, half_t* __restrict__ x_hi,
                                                        half_t* __restrict__ x_lo, float* __restrict__ pre) {
  embed_ln_body<false, false, true>(ids, cu, n_seq, tok_base, T, H, vocab, word, nullptr, type, g, nullptr, eps, x, x_hi, x_lo,
                                    pre, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ in, int T, int H,
                                                        const float* __restrict__ g,
                                                        const float* __restrict__ b, float eps,
                                                        float* __restrict__ out, half_t* __restrict__ out_hi,
                                                        half_t* __restrict__ out_lo, float2* __restrict__ stat) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const int pairs = H / 128;
  float2 v[kMaxPairs];
#pragma unroll
  for (int i = 0; i < kMaxPairs; ++i)
    if (i < pairs) v[i] = *reinterpret_cast<const float2*>(in + static_cast<int64_t>(t) * H + (i * 64 + lane) * 2);
  const int64_t o = static_cast<int64_t>(t) * H;
  row_layernorm(v, pairs, H, g, b, eps, lane, out ? out + o : nullptr, out_hi ? out_hi + (out_lo ? 2 : 1) * o : nullptr,
                out_lo ? out_lo + 2 * o : nullptr, stat ? stat + t : nullptr);
}

// the same launch with RMSNorm rows (VR_NORM_PRE_RMS): row_layernorm's RMS state. (A kernel beside layernorm_kernel, not
// a template state of it: that kernel keeps its name and its bytes.)
__global__ __launch_bounds__(256) void rmsnorm_kernel(const float* __restrict__ in, int T, int H,
                                                      const float* __restrict__ g, float eps,
                                                      float* __restrict__ out, half_t* __restrict__ out_hi,
                                                      half_t* __restrict__ out_lo) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const int pairs = H / 128;
  float2 v[kMaxPairs];
#pragma unroll
  for (int i = 0; i < kMaxPairs; ++i)
    if (i < pairs) v[i] = *reinterpret_cast<const float2*>(in + static_cast<int64_t>(t) * H + (i * 64 + lane) * 2);
  const int64_t o = static_cast<int64_t>(t) * H;
  row_layernorm<true>(v, pairs, H, g, nullptr, eps, lane, out ? out + o : nullptr,
                      out_hi ? out_hi + (out_lo ? 2 : 1) * o : nullptr, out_lo ? out_lo + 2 * o : nullptr, nullptr);
}

// f16-mode LayerNorm for H % 256 == 0: the row as float4 per lane (16-byte loads, 8-byte f16 stores —
// the generic kernel's 8-/4-byte accesses reached 4.6 TB/s on this 6-bytes-per-element pass). Writes the
// f16 row, the row's (mean, 1/sigma), and the f32 row only when `out` is given.
__global__ __launch_bounds__(256) void layernorm_f16_kernel(const float* __restrict__ in, int T, int H,
                                                            const float* __restrict__ g, const float* __restrict__ b,
                                                            float eps, float* __restrict__ out,
                                                            half_t* __restrict__ out_h, float2* __restrict__ stat) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const int quads = H / 256;  // <= 4
  const int64_t o = static_cast<int64_t>(t) * H;
  float4 v[4];
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < quads) {
      v[i] = *reinterpret_cast<const float4*>(in + o + (i * 64 + lane) * 4);
      s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
  const float mean = wave_sum(s) / static_cast<float>(H);
  float q = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < quads) {
      const float dx = v[i].x - mean, dy = v[i].y - mean, dz = v[i].z - mean, dw = v[i].w - mean;
      q += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
  const float var = wave_sum(q) / static_cast<float>(H);
  const float inv = 1.0f / sqrtf(var + eps);
  if (stat && lane == 0) stat[t] = make_float2(mean, inv);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < quads) {
      const int e = (i * 64 + lane) * 4;
      const float4 gg = *reinterpret_cast<const float4*>(g + e);
      const float4 bb = *reinterpret_cast<const float4*>(b + e);
      float4 r;
      r.x = ln_apply(v[i].x, mean, inv, gg.x, bb.x);
      r.y = ln_apply(v[i].y, mean, inv, gg.y, bb.y);
      r.z = ln_apply(v[i].z, mean, inv, gg.z, bb.z);
      r.w = ln_apply(v[i].w, mean, inv, gg.w, bb.w);
      if (out) *reinterpret_cast<float4*>(out + o + e) = r;
      half_t h[4], l[4];
      split_f16(r.x, h[0], l[0]);
      split_f16(r.y, h[1], l[1]);
      split_f16(r.z, h[2], l[2]);
      split_f16(r.w, h[3], l[3]);
      *reinterpret_cast<uint2*>(out_h + o + e) = *reinterpret_cast<const uint2*>(h);
    }
}

// layernorm_f16_kernel's RMSNorm twin (VR_NORM_PRE_RMS), the same loads and stores: one fixed-order sum of squares, no
// mean pass, no shift; the f16 row only. (A kernel of its own for the reason rmsnorm_kernel is one.)
__global__ __launch_bounds__(256) void rmsnorm_f16_kernel(const float* __restrict__ in, int T, int H,
                                                          const float* __restrict__ g, float eps,
                                                          half_t* __restrict__ out_h) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  const int quads = H / 256;  // <= 4
  const int64_t o = static_cast<int64_t>(t) * H;
  float4 v[4];
  float q = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < quads) {
      v[i] = *reinterpret_cast<const float4*>(in + o + (i * 64 + lane) * 4);
      q += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
    }
  const float inv = 1.0f / sqrtf(wave_sum(q) / static_cast<float>(H) + eps);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < quads) {
      const int e = (i * 64 + lane) * 4;
      const float4 gg = *reinterpret_cast<const float4*>(g + e);
      half_t h[4], l[4];
      split_f16(rms_apply(v[i].x, inv, gg.x), h[0], l[0]);
      split_f16(rms_apply(v[i].y, inv, gg.y), h[1], l[1]);
      split_f16(rms_apply(v[i].z, inv, gg.z), h[2], l[2]);
      split_f16(rms_apply(v[i].w, inv, gg.w), h[3], l[3]);
      *reinterpret_cast<uint2*>(out_h + o + e) = *reinterpret_cast<const uint2*>(h);
    }
}

// one block per sequence: mean (sum / max(count, 1e-9)), CLS or last-token pooling, then x / max(|x|, 1e-12) over all H columns.
// The leading ocols columns are stored, in rows of ostride floats (H and H without a head; a truncating head stores
// fewer, and what it stores are the bits it would have stored in full).
__global__ __launch_bounds__(256) void pool_kernel(const float* __restrict__ x,
                                                   const int32_t* __restrict__ cu, int seq0,
                                                   int tok_base, int H, int pooling, int normalize,
                                                   int compact, float* __restrict__ out, int ostride, int ocols) {
  __shared__ float red[4];
  const int seq = seq0 + blockIdx.x;
  // compact: x holds one row per sequence (its [CLS] row), see the last layer of forward_chunk
  const int t0 = compact ? static_cast<int>(blockIdx.x) : cu[seq] - tok_base;
  const int len = cu[seq + 1] - cu[seq];
  float vals[4];
  float ss = 0.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int c = threadIdx.x + 256 * j;
    float v = 0.0f;
    if (c < H && len > 0) {
      if (pooling == 1) {
        v = x[static_cast<int64_t>(t0) * H + c];
      } else if (pooling == 2) {  // VR_POOL_LAST: the sequence's last token (never compact: that is the CLS tail's)
        v = x[static_cast<int64_t>(t0 + len - 1) * H + c];
      } else {
        float acc = 0.0f;
        for (int t = 0; t < len; ++t) acc += x[static_cast<int64_t>(t0 + t) * H + c];
        v = acc / fmaxf(static_cast<float>(len), 1e-9f);
      }
    }
    vals[j] = v;
    ss += v * v;
  }
  ss = wave_sum(ss);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
  __syncthreads();
  const float norm = sqrtf(red[0] + red[1] + red[2] + red[3]);
  const float den = normalize ? fmaxf(norm, 1e-12f) : 1.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int c = threadIdx.x + 256 * j;
    if (c < ocols) out[static_cast<int64_t>(seq) * ostride + c] = vals[j] / den;
  }
}

// one block per span: the mean of the final hidden rows [begin, end) of the span's own sequence, summed in token order,
// then x / max(|x|, 1e-12) — pool_kernel's mean arithmetic over a token range, so a span [0, len) gives pool_kernel's
// bits. Block b serves span span0 + b; span_seq holds each span's sequence (no search here), span_tok its (begin, end).
// ostride / ocols: as pool_kernel's.
__global__ __launch_bounds__(256) void span_pool_kernel(const float* __restrict__ x, const int32_t* __restrict__ cu,
                                                        const int32_t* __restrict__ span_tok,
                                                        const int32_t* __restrict__ span_seq, int span0, int tok_base,
                                                        int H, int normalize, float* __restrict__ out, int ostride,
                                                        int ocols) {
  __shared__ float red[4];
  const int sp = span0 + blockIdx.x;
  const int begin = span_tok[2 * sp];
  const int len = span_tok[2 * sp + 1] - begin;
  const int t0 = cu[span_seq[sp]] - tok_base + begin;
  float vals[4];
  float ss = 0.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int c = threadIdx.x + 256 * j;
    float v = 0.0f;
    if (c < H && len > 0) {
      float acc = 0.0f;
      for (int t = 0; t < len; ++t) acc += x[static_cast<int64_t>(t0 + t) * H + c];
      v = acc / fmaxf(static_cast<float>(len), 1e-9f);
    }
    vals[j] = v;
    ss += v * v;
  }
  ss = wave_sum(ss);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
  __syncthreads();
  const float norm = sqrtf(red[0] + red[1] + red[2] + red[3]);
  const float den = normalize ? fmaxf(norm, 1e-12f) : 1.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int c = threadIdx.x + 256 * j;
    if (c < ocols) out[static_cast<int64_t>(sp) * ostride + c] = vals[j] / den;
  }
}

// ---- semantic chunking (vr_encode_semantic) --------------------------------------------------
// The stage between "unit sums" and "chunk rows" of a forward chunk, five launches in stream order; a unit is a span
// of vr_encode_spans (unit_tok, unit_seq as span_pool_kernel's), unit_off[seq] .. unit_off[seq + 1] a sequence's units.
// Every sum runs in one fixed order and nothing is decided by an atomic: same input, same bits, whatever the batch.
struct SemanticParams {
  int buffer, break_permille, min_tokens, max_tokens;
  float min_distance;
};
constexpr int kMaxSemUnits = 2048;  // units of one sequence: unit_boundary_kernel holds their distances in LDS

// one block per unit: S_r, span_pool_kernel's token-order sum without the divide, kept as [unit][H]
__global__ __launch_bounds__(256) void unit_sum_kernel(const float* __restrict__ x, const int32_t* __restrict__ cu,
                                                       const int32_t* __restrict__ unit_tok,
                                                       const int32_t* __restrict__ unit_seq, int unit0, int tok_base,
                                                       int H, float* __restrict__ sums) {
  const int u = unit0 + blockIdx.x;
  const int begin = unit_tok[2 * u];
  const int len = unit_tok[2 * u + 1] - begin;
  const int t0 = cu[unit_seq[u]] - tok_base + begin;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = threadIdx.x + 256 * j;
    if (c < H) {
      float acc = 0.0f;
      for (int t = 0; t < len; ++t) acc += x[static_cast<int64_t>(t0 + t) * H + c];
      sums[static_cast<int64_t>(u) * H + c] = acc;
    }
  }
}

// one block per unit r: the distance of the gap behind it, d_r = 1 - C_r . C_{r+1} / max(|C_r| |C_{r+1}|, 1e-12) with
// C_r the sum of S_j over the units j within `buffer` of r inside the sequence, in unit order; 0 for a sequence's last
// unit. The three sums over the columns: per thread over its columns, a xor butterfly in the wave, the four waves in order.
__global__ __launch_bounds__(256) void unit_gap_kernel(const float* __restrict__ sums, const int32_t* __restrict__ unit_off,
                                                       const int32_t* __restrict__ unit_seq, int unit0, int H, int buffer,
                                                       float* __restrict__ dist) {
  __shared__ float red[3][4];
  const int u = unit0 + blockIdx.x;
  const int seq = unit_seq[u];
  const int lo = unit_off[seq], hi = unit_off[seq + 1];
  if (u + 1 >= hi) {  // (the whole block: u is the block's)
    if (threadIdx.x == 0) dist[u] = 0.0f;
    return;
  }
  const int a0 = max(lo, u - buffer), a1 = min(hi - 1, u + buffer);
  const int b0 = max(lo, u + 1 - buffer), b1 = min(hi - 1, u + 1 + buffer);
  float dot = 0.0f, na = 0.0f, nb = 0.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = threadIdx.x + 256 * j;
    if (c < H) {
      float ca = 0.0f, cb = 0.0f;
      for (int v = a0; v <= a1; ++v) ca += sums[static_cast<int64_t>(v) * H + c];
      for (int v = b0; v <= b1; ++v) cb += sums[static_cast<int64_t>(v) * H + c];
      dot += ca * cb;
      na += ca * ca;
      nb += cb * cb;
    }
  }
  dot = wave_sum(dot);
  na = wave_sum(na);
  nb = wave_sum(nb);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = dot;
    red[1][threadIdx.x >> 6] = na;
    red[2][threadIdx.x >> 6] = nb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    dot = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    na = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    nb = red[2][0] + red[2][1] + red[2][2] + red[2][3];
    dist[u] = 1.0f - dot / fmaxf(sqrtf(na) * sqrtf(nb), 1e-12f);
  }
}

// one block per sequence: which of its m - 1 gaps are candidates, then the walk. rank(r) counts the gaps with a larger
// distance, or an equal one at a lower index (f32 compares on the stored values, all m - 1 of them from LDS); gap r is
// a candidate iff rank(r) < B = ceil(break_permille (m - 1) / 1000) and d_r >= min_distance. Lane 0 then walks the units
// left to right: start[u] = 1 and idx[u] = the chunk's index inside the sequence where a chunk begins, 0 and -1
// elsewhere; seq_chunks[seq] = the sequence's chunks.
__global__ __launch_bounds__(256) void unit_boundary_kernel(const float* __restrict__ dist, const int32_t* __restrict__ unit_off,
                                                            const int32_t* __restrict__ unit_tok, int seq0, SemanticParams p,
                                                            int32_t* __restrict__ start, int32_t* __restrict__ idx,
                                                            int32_t* __restrict__ seq_chunks) {
  __shared__ float d[kMaxSemUnits];
  __shared__ uint8_t cand[kMaxSemUnits];
  const int seq = seq0 + blockIdx.x;
  const int lo = unit_off[seq];
  const int m = min(unit_off[seq + 1] - lo, kMaxSemUnits);  // (the host refuses more: the bound of d[] stands in the kernel too)
  if (m <= 0) {
    if (threadIdx.x == 0) seq_chunks[seq] = 0;
    return;
  }
  const int gaps = m - 1;
  for (int r = threadIdx.x; r < gaps; r += 256) d[r] = dist[lo + r];
  __syncthreads();
  const int B = (p.break_permille * gaps + 999) / 1000;
  for (int r = threadIdx.x; r < gaps; r += 256) {
    const float dr = d[r];
    int rank = 0;
    for (int q = 0; q < gaps; ++q) {
      const float dq = d[q];
      rank += (dq > dr || (dq == dr && q < r)) ? 1 : 0;
    }
    cand[r] = (rank < B && dr >= p.min_distance) ? 1 : 0;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  int acc = unit_tok[2 * lo + 1] - unit_tok[2 * lo];
  int chunks = 1;
  start[lo] = 1;
  idx[lo] = 0;
  for (int r = 0; r < gaps; ++r) {
    const int u = lo + r + 1;
    const int n = unit_tok[2 * u + 1] - unit_tok[2 * u];
    const bool close = (cand[r] && acc >= p.min_tokens) || acc + n > p.max_tokens;
    start[u] = close ? 1 : 0;
    idx[u] = close ? chunks : -1;
    chunks += close ? 1 : 0;
    acc = close ? n : acc + n;
  }
  seq_chunks[seq] = chunks;
}

// one block: seq_base[seq] = the first chunk row of every sequence of the forward chunk — the running counter (chunks of
// the forward chunks before this one, in stream order) plus the chunk counts of the sequences before it — and the
// counter moved past them. Thread t adds up a contiguous slice of the sequences, lane 0 the 256 slices in order.
__global__ __launch_bounds__(256) void chunk_base_kernel(const int32_t* __restrict__ seq_chunks, int seq0, int n,
                                                         int32_t* __restrict__ seq_base, int32_t* __restrict__ counter) {
  __shared__ int part[256];
  const int per = (n + 255) / 256;
  const int b = min(n, static_cast<int>(threadIdx.x) * per), e = min(n, b + per);
  int s = 0;
  for (int i = b; i < e; ++i) s += seq_chunks[seq0 + i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = counter[0];
    for (int t = 0; t < 256; ++t) {
      const int v = part[t];
      part[t] = run;
      run += v;
    }
    counter[0] = run;
  }
  __syncthreads();
  int run = part[threadIdx.x];
  for (int i = b; i < e; ++i) {
    seq_base[seq0 + i] = run;
    run += seq_chunks[seq0 + i];
  }
}

// one block per unit, at work where a chunk starts: (the sum of S_r over the chunk's units, in unit order) / (their
// tokens), finished as span_pool_kernel finishes a span mean — the same operations, so a chunk of one unit has that
// span's bits. Row: the chunk's own (seq_base + idx) — or, by_unit, the starting unit's, with zeros in the rows of
// the other units: the rows embed_head_kernel then reads, a known number of them (chunk_gather_kernel compacts after).
__global__ __launch_bounds__(256) void chunk_row_kernel(const float* __restrict__ sums, const int32_t* __restrict__ unit_off,
                                                        const int32_t* __restrict__ unit_tok,
                                                        const int32_t* __restrict__ unit_seq,
                                                        const int32_t* __restrict__ start, const int32_t* __restrict__ idx,
                                                        const int32_t* __restrict__ seq_base, int unit0, int H,
                                                        int normalize, int by_unit, float* __restrict__ out, int ostride,
                                                        int ocols) {
  __shared__ float red[4];
  const int u = unit0 + blockIdx.x;
  if (!start[u]) {  // (the whole block)
    if (by_unit)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = threadIdx.x + 256 * j;
        if (c < ocols) out[static_cast<int64_t>(u) * ostride + c] = 0.0f;
      }
    return;
  }
  const int seq = unit_seq[u];
  const int hi = unit_off[seq + 1];
  int end = u + 1;
  while (end < hi && !start[end]) ++end;
  int len = 0;
  for (int v = u; v < end; ++v) len += unit_tok[2 * v + 1] - unit_tok[2 * v];
  const int row = by_unit ? u : seq_base[seq] + idx[u];
  float vals[4];
  float ss = 0.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int c = threadIdx.x + 256 * j;
    float v = 0.0f;
    if (c < H && len > 0) {
      float acc = 0.0f;
      for (int w = u; w < end; ++w) acc += sums[static_cast<int64_t>(w) * H + c];
      v = acc / fmaxf(static_cast<float>(len), 1e-9f);
    }
    vals[j] = v;
    ss += v * v;
  }
  ss = wave_sum(ss);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
  __syncthreads();
  const float norm = sqrtf(red[0] + red[1] + red[2] + red[3]);
  const float den = normalize ? fmaxf(norm, 1e-12f) : 1.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int c = threadIdx.x + 256 * j;
    if (c < ocols) out[static_cast<int64_t>(row) * ostride + c] = vals[j] / den;
  }
}

// one block per unit: the head's row of a unit that starts a chunk ([unit][W]) to the chunk's own row of out
__global__ __launch_bounds__(256) void chunk_gather_kernel(const float* __restrict__ rows, const int32_t* __restrict__ unit_seq,
                                                           const int32_t* __restrict__ start, const int32_t* __restrict__ idx,
                                                           const int32_t* __restrict__ seq_base, int unit0, int W,
                                                           float* __restrict__ out) {
  const int u = unit0 + blockIdx.x;
  if (!start[u]) return;
  const int64_t row = seq_base[unit_seq[u]] + idx[u];
  for (int c = threadIdx.x; c < W; c += 256) out[row * W + c] = rows[static_cast<int64_t>(u) * W + c];
}

// Cross-encoder head on n pooled [CLS] rows [n, H]: out[i] = wc . tanh(Wp h_i + bp) + bc, all f32. One block of 4 waves
// per 16 rows: each wave takes every 4th 16-unit column tile of the pooler, a v_mfma_f32_16x16x4_f32 tile with the 16
// rows as M and the tile's units as N (A and B read the same k permutation from float4 loads: lane quad q, step s holds
// k0 + 4q + s), so Wp is read once per 16 rows. The sum over units is in a fixed order — per lane over its tiles, a xor
// butterfly across the 16 lanes of a row group, then the four waves in order — with no atomics: same input, same bits.
__global__ __launch_bounds__(256) void rerank_head_kernel(const float* __restrict__ rows, int n, int H,
                                                          const float* __restrict__ wp, const float* __restrict__ bp,
                                                          const float* __restrict__ wc, const float* __restrict__ bc,
                                                          float* __restrict__ out) {
  __shared__ float red[4][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int p0 = blockIdx.x * 16;
  const bool live = p0 + r < n;
  const float* a_row = rows + static_cast<int64_t>(live ? p0 + r : p0) * H;
  float part[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int jt = wave; jt < H / 16; jt += 4) {
    const float* w_row = wp + static_cast<int64_t>(jt * 16 + r) * H;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k0 = 0; k0 < H; k0 += 16) {
      const float4 a = live ? *reinterpret_cast<const float4*>(a_row + k0 + 4 * q) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      const float4 b = *reinterpret_cast<const float4*>(w_row + k0 + 4 * q);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    }
    const int j = jt * 16 + r;  // D: column (unit) lane & 15, row (pair) 4 q + i
    const float bj = bp[j], cj = wc[j];
#pragma unroll
    for (int i = 0; i < 4; ++i) part[i] += tanhf(acc[i] + bj) * cj;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) part[i] += __shfl_xor(part[i], off);
  if (r == 0)
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave][4 * q + i] = part[i];
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 16 && p0 + t < n) out[p0 + t] = bc[0] + red[0][t] + red[1][t] + red[2][t] + red[3][t];
}

constexpr int kHeadTiles = 16;  // 16-unit tiles of the head's dense layer per wave: H / 64, H <= 1024

// The head of a pre-norm cross-encoder (ModernBertForSequenceClassification) on n pooled rows [n, H]:
// out[i] = wc . LN(gelu(Wd p_i + bd)) + bc, gelu the exact-erf one, LN over all H units with gain g, shift b and eps,
// all f32. The dense layer runs as rerank_head_kernel's does: one block of 4 waves per 16 rows, wave w takes the
// 16-unit tiles w, w + 4, ... on v_mfma_f32_16x16x4_f32, Wd read once per 16 rows. A row's H activations then sit in
// registers, 4 rows x H/64 tiles per lane, and three sums over them follow, each in the same fixed order — per lane over
// its tiles, a xor butterfly across the 16 lanes of a row group, then the four waves in order through LDS: the mean,
// the centred sum of squares (two passes: no cancellation), and the dot of the normalised units with wc. No atomics;
// a row's arithmetic never meets another row's, so its bits depend neither on n nor on its place among the 16.
__global__ __launch_bounds__(256) void rerank_head_ln_kernel(const float* __restrict__ rows, int n, int H,
                                                             const float* __restrict__ wd, const float* __restrict__ bd,
                                                             const float* __restrict__ g, const float* __restrict__ b,
                                                             float eps, const float* __restrict__ wc,
                                                             const float* __restrict__ bc, float* __restrict__ out) {
  __shared__ float red[3][4][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int p0 = blockIdx.x * 16;
  const bool live = p0 + r < n;
  const float* a_row = rows + static_cast<int64_t>(live ? p0 + r : p0) * H;
  const int tiles = H / 16;
  float act[kHeadTiles][4];
#pragma unroll
  for (int t = 0; t < kHeadTiles; ++t) {
    const int jt = wave + 4 * t;
#pragma unroll
    for (int i = 0; i < 4; ++i) act[t][i] = 0.0f;
    if (jt < tiles) {
      const float* w_row = wd + static_cast<int64_t>(jt * 16 + r) * H;
      f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int k0 = 0; k0 < H; k0 += 16) {
        const float4 a = live ? *reinterpret_cast<const float4*>(a_row + k0 + 4 * q) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float4 w = *reinterpret_cast<const float4*>(w_row + k0 + 4 * q);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w.w, acc, 0, 0, 0);
      }
      const float bj = bd[jt * 16 + r];  // D: column (unit) lane & 15, row (pair) 4 q + i
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = acc[i] + bj;
        act[t][i] = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
      }
    }
  }
  // the sum of part[i] over all H units of row 4 q + i, the same bits in every lane of the block that holds the row
  auto row_sums = [&](float (&part)[4], int slot) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) part[i] += __shfl_xor(part[i], off);
    if (r == 0)
#pragma unroll
      for (int i = 0; i < 4; ++i) red[slot][wave][4 * q + i] = part[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
      part[i] = red[slot][0][4 * q + i] + red[slot][1][4 * q + i] + red[slot][2][4 * q + i] + red[slot][3][4 * q + i];
  };
  const float inv_h = 1.0f / static_cast<float>(H);
  float mean[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int t = 0; t < kHeadTiles; ++t)  // (tiles past H / 16 hold zeros)
#pragma unroll
    for (int i = 0; i < 4; ++i) mean[i] += act[t][i];
  row_sums(mean, 0);
  float inv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int i = 0; i < 4; ++i) mean[i] *= inv_h;
#pragma unroll
  for (int t = 0; t < kHeadTiles; ++t)
    if (wave + 4 * t < tiles)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        act[t][i] -= mean[i];
        inv[i] += act[t][i] * act[t][i];
      }
  row_sums(inv, 1);
#pragma unroll
  for (int i = 0; i < 4; ++i) inv[i] = 1.0f / sqrtf(inv[i] * inv_h + eps);
  float part[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int t = 0; t < kHeadTiles; ++t) {
    const int jt = wave + 4 * t;
    if (jt < tiles) {
      const int j = jt * 16 + r;
      const float gj = g[j], sj = b[j], cj = wc[j];
#pragma unroll
      for (int i = 0; i < 4; ++i) part[i] += (act[t][i] * inv[i] * gj + sj) * cj;
    }
  }
  row_sums(part, 2);
  if (wave == 0 && r == 0)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (p0 + 4 * q + i < n) out[p0 + 4 * q + i] = bc[0] + part[i];
}

// The embedder's post-pooling head (vr_encoder_set_head) on n un-normalised pooled rows [n, W0], all f32: the stages of
// hp in order, then (normalize) x / max(|x|, 1e-12) over the whole last width, then the leading ocols columns into rows
// of ostride floats. One block of 4 waves per 16 rows. Between stages a row lives in registers in the MFMA's D layout:
// lane (r = lane & 15, q = lane >> 4) of wave w holds, for its 16-column tiles jt = w, w + 4, ... (slot t = jt / 4),
// column 16 jt + r of the rows 4 q + i; slots past the current width hold zeros.
//   Dense      the rows are handed over through LDS (abuf, [16][lda], lda = the widest Dense input + 4: the pad of one
//              b128 access keeps the 16 rows of an A read on different banks) and every wave runs its tiles as
//              rerank_head_kernel does — v_mfma_f32_16x16x4_f32, the 16 rows as M, A and W read with the same k
//              permutation — but k outermost: one A read serves all of a wave's tiles, their weight loads are in flight
//              together and the accumulators are independent. The weight is read once per 16 rows.
//   LayerNorm  two passes over the registers (mean, then the centred sum of squares: no cancellation).
// Every sum over a row's columns is in one fixed order — per lane over its tiles, a xor butterfly across the 16 lanes of
// a row group, then the four waves in order through LDS — with no atomics, and a row's arithmetic never meets another
// row's: its bits depend neither on n nor on its place among the 16.
__global__ __launch_bounds__(256) void embed_head_kernel(const float* __restrict__ rows, int n, int W0, HeadParams hp,
                                                         int normalize, int lda, float* __restrict__ out, int ostride,
                                                         int ocols) {
  extern __shared__ __attribute__((aligned(16))) float head_lds[];
  float* red = head_lds;        // [4][16]
  float* abuf = head_lds + 64;  // [16][lda]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int p0 = blockIdx.x * 16;
  f32x4 act[kHeadTiles];
  int W = W0;
#pragma unroll
  for (int t = 0; t < kHeadTiles; ++t) {
    const int col = (wave + 4 * t) * 16 + r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = p0 + 4 * q + i;
      act[t][i] = (col < W && row < n) ? rows[static_cast<int64_t>(row) * W0 + col] : 0.0f;
    }
  }
  // the sum of part[i] over all columns of row 4 q + i, the same bits in every lane of the block that holds the row
  auto row_sums = [&](f32x4& part) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) part[i] += __shfl_xor(part[i], off);
    if (r == 0)
#pragma unroll
      for (int i = 0; i < 4; ++i) red[wave * 16 + 4 * q + i] = part[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) part[i] = red[4 * q + i] + red[16 + 4 * q + i] + red[32 + 4 * q + i] + red[48 + 4 * q + i];
    __syncthreads();  // (red is written again by the next sum)
  };
  for (int s = 0; s < hp.n_stages; ++s) {
    const HeadStage st = hp.st[s];
    if (st.kind == VR_HEAD_DENSE) {
      const int K = st.in_dim, tiles = st.out_dim / 16;
#pragma unroll
      for (int t = 0; t < kHeadTiles; ++t) {
        const int col = (wave + 4 * t) * 16 + r;
        if (col < K)
#pragma unroll
          for (int i = 0; i < 4; ++i) abuf[(4 * q + i) * lda + col] = act[t][i];
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < kHeadTiles; ++t) act[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      const float* a_row = abuf + r * lda + 4 * q;
      const float* w_row = st.w + static_cast<int64_t>(wave * 16 + r) * K + 4 * q;  // slot t: 64 t rows further
      // (issuing four k-steps' weight loads ahead of their products changed nothing measurable: a block is bound by its
      // 16-row MFMA work and by one CU's share of the weight's bytes)
      for (int k0 = 0; k0 < K; k0 += 16) {
        const float4 a = *reinterpret_cast<const float4*>(a_row + k0);
        float4 w[kHeadTiles];
#pragma unroll
        for (int t = 0; t < kHeadTiles; ++t)
          if (wave + 4 * t < tiles) w[t] = *reinterpret_cast<const float4*>(w_row + static_cast<int64_t>(64 * t) * K + k0);
#pragma unroll
        for (int t = 0; t < kHeadTiles; ++t)
          if (wave + 4 * t < tiles) {
            act[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w[t].x, act[t], 0, 0, 0);
            act[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w[t].y, act[t], 0, 0, 0);
            act[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w[t].z, act[t], 0, 0, 0);
            act[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w[t].w, act[t], 0, 0, 0);
          }
      }
#pragma unroll
      for (int t = 0; t < kHeadTiles; ++t)
        if (wave + 4 * t < tiles) {  // D: column (unit) lane & 15, row 4 q + i
          const float bj = st.b ? st.b[(wave + 4 * t) * 16 + r] : 0.0f;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float v = act[t][i] + bj;
            act[t][i] = st.act == VR_ACT_TANH ? tanhf(v) : v;
          }
        }
      __syncthreads();  // (abuf is written again by the next Dense stage)
      W = st.out_dim;
    } else {
      const float inv_w = 1.0f / static_cast<float>(W);
      f32x4 mean = {0.0f, 0.0f, 0.0f, 0.0f}, inv = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int t = 0; t < kHeadTiles; ++t) mean += act[t];  // (slots past W hold zeros)
      row_sums(mean);
      mean *= inv_w;
#pragma unroll
      for (int t = 0; t < kHeadTiles; ++t)
        if ((wave + 4 * t) * 16 < W) {
          act[t] -= mean;
          inv += act[t] * act[t];
        }
      row_sums(inv);
#pragma unroll
      for (int i = 0; i < 4; ++i) inv[i] = 1.0f / sqrtf(inv[i] * inv_w + st.eps);
#pragma unroll
      for (int t = 0; t < kHeadTiles; ++t)
        if ((wave + 4 * t) * 16 < W) {
          const int col = (wave + 4 * t) * 16 + r;
          const float g = st.w[col], b = st.b ? st.b[col] : 0.0f;
#pragma unroll
          for (int i = 0; i < 4; ++i) act[t][i] = act[t][i] * inv[i] * g + b;
        }
    }
  }
  if (normalize) {
    f32x4 ss = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < kHeadTiles; ++t) ss += act[t] * act[t];
    row_sums(ss);
#pragma unroll
    for (int i = 0; i < 4; ++i) ss[i] = fmaxf(sqrtf(ss[i]), 1e-12f);
#pragma unroll
    for (int t = 0; t < kHeadTiles; ++t) act[t] /= ss;
  }
#pragma unroll
  for (int t = 0; t < kHeadTiles; ++t) {
    const int col = (wave + 4 * t) * 16 + r;
    if (col < ocols)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (p0 + 4 * q + i < n) out[static_cast<int64_t>(p0 + 4 * q + i) * ostride + col] = act[t][i];
  }
}

// embed_head_kernel's LDS: the four waves' partial sums, then 16 rows of the widest Dense input padded by one float4
static int head_lda(const HeadParams& hp) {
  int k = 0;
  for (int s = 0; s < hp.n_stages; ++s)
    if (hp.st[s].kind == VR_HEAD_DENSE) k = std::max(k, hp.st[s].in_dim);
  return k + 4;
}
static size_t head_lds_bytes(int lda) { return (64 + 16 * static_cast<size_t>(lda)) * sizeof(float); }
constexpr int kMaxHeadWidth = 1024;  // vr_encoder_set_head's widest stage: head_lds_bytes(kMaxHeadWidth + 4) is 65 KiB

// the width of an output row: the head's (vr_encoder_set_head), without one the model's
static int out_width(const Encoder* enc) { return enc->has_head ? enc->out_dim : enc->d.hidden; }

// dst[i] = src[first token of sequence seq0 + i]; rows of `row_f4` float4s (an f32 row of H floats and
// an interleaved (hi, lo) f16 row of 2H halfs have the same 4H bytes). One wave per row.
__global__ __launch_bounds__(256) void gather_first_rows_kernel(const float4* __restrict__ src,
                                                                const int32_t* __restrict__ cu, int seq0,
                                                                int tok_base, int n, int T, int row_f4,
                                                                float4* __restrict__ dst) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int t = min(cu[seq0 + i] - tok_base, T - 1);  // an empty sequence reads a neighbour's row; pooling ignores it
  for (int c = lane; c < row_f4; c += 64) dst[static_cast<int64_t>(i) * row_f4 + c] = src[static_cast<int64_t>(t) * row_f4 + c];
}

// The same for a decoder cross-encoder, which reads the LAST token of every pair (rerank_tail): the context row
// (`ctx_f4` float4s: f32, (hi, lo) or plain f16 rows, A wide) and the residual row (`x_f4` float4s, f32) of token
// cu[seq0 + i + 1] - 1, both in one launch. One wave per row.
__global__ __launch_bounds__(256) void gather_last_rows_kernel(const float4* __restrict__ ctx, const float4* __restrict__ x,
                                                               const int32_t* __restrict__ cu, int seq0, int tok_base, int n,
                                                               int T, int ctx_f4, int x_f4, float4* __restrict__ ctx_dst,
                                                               float4* __restrict__ x_dst) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int t = min(max(cu[seq0 + i + 1] - 1 - tok_base, 0), T - 1);  // (lengths are checked >= 1; never outside the pass)
  for (int c = lane; c < ctx_f4; c += 64) ctx_dst[static_cast<int64_t>(i) * ctx_f4 + c] = ctx[static_cast<int64_t>(t) * ctx_f4 + c];
  for (int c = lane; c < x_f4; c += 64) x_dst[static_cast<int64_t>(i) * x_f4 + c] = x[static_cast<int64_t>(t) * x_f4 + c];
}

// The head of a decoder cross-encoder on n residual rows [n, H]: out[i] = w . rms(x_i, g), the final RMSNorm and the dot
// product with score.weight in one launch, f32 whatever the model's precision. One wave per row, the row as float2
// pairs per lane (rmsnorm_kernel's layout and its sum of squares, so the normalised values are that kernel's bits);
// each lane sums its squares and then its products in index order, a fixed xor butterfly finishes both. No atomics, no
// LDS: a row's logit bits depend on that row alone, not on n or on the row's place in the launch.
__global__ __launch_bounds__(256) void rerank_head_rms_kernel(const float* __restrict__ x, int n, int H,
                                                              const float* __restrict__ g, float eps,
                                                              const float* __restrict__ w, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int pairs = H / 128;
  float2 v[kMaxPairs];
  float q = 0.0f;
#pragma unroll
  for (int k = 0; k < kMaxPairs; ++k)
    if (k < pairs) {
      v[k] = *reinterpret_cast<const float2*>(x + static_cast<int64_t>(i) * H + (k * 64 + lane) * 2);
      q += v[k].x * v[k].x + v[k].y * v[k].y;
    }
  const float inv = 1.0f / sqrtf(wave_sum(q) / static_cast<float>(H) + eps);
  float dot = 0.0f;
#pragma unroll
  for (int k = 0; k < kMaxPairs; ++k)
    if (k < pairs) {
      const int e = (k * 64 + lane) * 2;
      const float2 gg = *reinterpret_cast<const float2*>(g + e);
      const float2 ww = *reinterpret_cast<const float2*>(w + e);
      dot += rms_apply(v[k].x, inv, gg.x) * ww.x;
      dot += rms_apply(v[k].y, inv, gg.y) * ww.y;
    }
  dot = wave_sum(dot);
  if (lane == 0) out[i] = dot;
}

// dst[i] = LayerNorm output of the first token of sequence seq0 + i, re-derived from the pre-LN rows
// and their (mean, 1/sigma) — the f32 hidden state is not stored in f16 mode. One wave per row.
__global__ __launch_bounds__(256) void gather_first_rows_ln_kernel(const float* __restrict__ pre,
                                                                   const float2* __restrict__ stat,
                                                                   const float* __restrict__ g,
                                                                   const float* __restrict__ b,
                                                                   const int32_t* __restrict__ cu, int seq0,
                                                                   int tok_base, int n, int T, int H,
                                                                   float* __restrict__ dst) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int t = min(cu[seq0 + i] - tok_base, T - 1);
  const float2 st = stat[t];
  for (int c = lane; c < H; c += 64)
    dst[static_cast<int64_t>(i) * H + c] = ln_apply(pre[static_cast<int64_t>(t) * H + c], st.x, st.y, g[c], b[c]);
}

// the same from f16 pre-LN rows (f16 residual stream, see EPI_RLS_*)
__global__ __launch_bounds__(256) void gather_first_rows_ln16_kernel(const half_t* __restrict__ pre,
                                                                     const float2* __restrict__ stat,
                                                                     const float* __restrict__ g,
                                                                     const float* __restrict__ b,
                                                                     const int32_t* __restrict__ cu, int seq0,
                                                                     int tok_base, int n, int T, int H,
                                                                     float* __restrict__ dst,
                                                                     half_t* __restrict__ dst16) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int t = min(cu[seq0 + i] - tok_base, T - 1);
  const float2 st = stat[t];
  for (int c = lane; c < H; c += 64) {
    const float v = ln_apply(static_cast<float>(pre[static_cast<int64_t>(t) * H + c]), st.x, st.y, g[c], b[c]);
    dst[static_cast<int64_t>(i) * H + c] = v;
    // (or null) the same rows as a GEMM's f16 input: the [CLS] query projection of cls_attend_kernel's route
    if (dst16) dst16[static_cast<int64_t>(i) * H + c] = static_cast<half_t>(fminf(fmaxf(v, -65504.0f), 65504.0f));
  }
}

// ---- rotary positions and the gated FFN, as passes of their own ------------------------------------

// eight consecutive values of a row (16-byte aligned: every caller's column is a multiple of 8) as floats, and back
__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}
__device__ __forceinline__ void load8(const half_t* p, float (&v)[8]) {
  const f16x8 h = *reinterpret_cast<const f16x8*>(p);
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = static_cast<float>(h[k]);
}
__device__ __forceinline__ void store8(float* p, const float (&v)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ void store8(half_t* p, const float (&v)[8]) {
  f16x8 h;
#pragma unroll
  for (int k = 0; k < 8; ++k) h[k] = static_cast<half_t>(fminf(fmaxf(v[k], -65504.0f), 65504.0f));
  *reinterpret_cast<f16x8*>(p) = h;
}

// One wave per token, in place on the Q and K thirds of its [3H] row (T = float: the f32 / f16x3 modes, half_t: the
// f16 mode, whose rotated values are rounded to f16 a second time). Feature j < d_h/2 of a head pairs with j + d_h/2:
//   x[j] <- x[j] cos - x[j + d_h/2] sin,  x[j + d_h/2] <- x[j + d_h/2] cos + x[j] sin   (HF rotate_half)
// with (cos, sin) of (the token's position inside its own sequence, frequency j). The arithmetic is f32.
template <typename T>
__global__ __launch_bounds__(256) void rope_kernel(T* __restrict__ qkv, const int32_t* __restrict__ pos, int Tn, int H,
                                                   int dh, const float2* __restrict__ table) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= Tn) return;
  const int half = dh >> 1;          // 16 or 32
  const int groups = half >> 3;      // groups of 8 pairs per head
  const int per_third = (H / dh) * groups;
  T* row = qkv + static_cast<int64_t>(t) * 3 * H;
  const float2* cs_row = table + static_cast<int64_t>(pos[t]) * (H >> 1);  // (the first head's entries serve every head)
  for (int c = lane; c < 2 * per_third; c += 64) {  // a lane takes 8 pairs of one head of the query or the key
    const int third = c >= per_third ? 1 : 0;
    const int w = c - third * per_third;
    const int head = w / groups, i8 = (w - head * groups) << 3;
    T* at = row + third * H + head * dh + i8;
    float a[8], b[8], cs0[8], cs1[8];  // cs0 / cs1: (cos, sin) of pairs 0..3 / 4..7
    load8(at, a);
    load8(at + half, b);
    load8(reinterpret_cast<const float*>(cs_row + i8), cs0);
    load8(reinterpret_cast<const float*>(cs_row + i8 + 4), cs1);
    float ra[8], rb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float co = k < 4 ? cs0[2 * k] : cs1[2 * k - 8], si = k < 4 ? cs0[2 * k + 1] : cs1[2 * k - 7];
      ra[k] = a[k] * co - b[k] * si;
      rb[k] = b[k] * co + a[k] * si;
    }
    store8(at, ra);
    store8(at + half, rb);
  }
}

// The per-head RMSNorm of the query and the key (vr_bert_desc_v3.qk_norm, Qwen3) and the rotation behind it, in one
// pass: rope_kernel's walk (one wave per token, a lane takes 8 pairs of one head of the query or the key, `H` the
// width A of a third), with every value first scaled by rsqrt(mean_d(x^2) + eps) of its head and by the gain of its
// feature (gq for the query third, gk for the key third, [d_h] each, shared by the heads):
//   n[j] = x[j] r g[j];  x[j] <- n[j] cos - n[j + d_h/2] sin,  x[j + d_h/2] <- n[j + d_h/2] cos + n[j] sin
// A head's d_h values lie in d_h/16 neighbouring lanes (2, 4 or 8, aligned: c advances by 64 and the loop's bound is a
// multiple of d_h/16, so a group is active or idle as a whole). Each lane sums its 16 squares in index order, the
// group adds them with a butterfly of __shfl_xor (1, 2, 4): a fixed order that depends on the head alone, so a row's
// bits do not depend on the batch it travels in. Everything is f32; T = half_t rounds once, at the store.
template <typename T>
__global__ __launch_bounds__(256) void qk_norm_rope_kernel(T* __restrict__ qkv, const int32_t* __restrict__ pos, int Tn, int H,
                                                           int dh, const float2* __restrict__ table,
                                                           const float* __restrict__ gq, const float* __restrict__ gk,
                                                           float eps) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= Tn) return;
  const int half = dh >> 1;          // 16, 32 or 64
  const int groups = half >> 3;      // lanes per head: groups of 8 pairs
  const int per_third = (H / dh) * groups;
  const float inv_dh = 1.0f / static_cast<float>(dh);
  T* row = qkv + static_cast<int64_t>(t) * 3 * H;
  const float2* cs_row = table + static_cast<int64_t>(pos[t]) * (H >> 1);  // (the first head's entries serve every head)
  for (int c = lane; c < 2 * per_third; c += 64) {
    const int third = c >= per_third ? 1 : 0;
    const int w = c - third * per_third;
    const int head = w / groups, i8 = (w - head * groups) << 3;
    T* at = row + third * H + head * dh + i8;
    const float* gain = (third ? gk : gq) + i8;
    float a[8], b[8], ga[8], gb[8], cs0[8], cs1[8];  // cs0 / cs1: (cos, sin) of pairs 0..3 / 4..7
    load8(at, a);
    load8(at + half, b);
    load8(gain, ga);
    load8(gain + half, gb);
    load8(reinterpret_cast<const float*>(cs_row + i8), cs0);
    load8(reinterpret_cast<const float*>(cs_row + i8 + 4), cs1);
    float ss = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) ss = fmaf(a[k], a[k], ss);
#pragma unroll
    for (int k = 0; k < 8; ++k) ss = fmaf(b[k], b[k], ss);
    for (int o = 1; o < groups; o <<= 1) ss += __shfl_xor(ss, o);
    const float r = rsqrtf(ss * inv_dh + eps);
    float ra[8], rb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float co = k < 4 ? cs0[2 * k] : cs1[2 * k - 8], si = k < 4 ? cs0[2 * k + 1] : cs1[2 * k - 7];
      const float na = a[k] * r * ga[k], nb = b[k] * r * gb[k];
      ra[k] = na * co - nb * si;
      rb[k] = nb * co + na * si;
    }
    store8(at, ra);
    store8(at + half, rb);
  }
}

// pos[t] = index of token t inside its own sequence (binary search of the offsets), once per forward pass: the
// rotation of every layer reads it. Lengths are checked against max_pos before any launch, so pos < max_pos.
__global__ __launch_bounds__(256) void positions_kernel(const int32_t* __restrict__ cu, int n_seq, int tok_base, int Tn,
                                                        int32_t* __restrict__ pos) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Tn) return;
  int lo = 0, hi = n_seq;
  const int tg = t + tok_base;
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    if (cu[mid] <= tg) lo = mid; else hi = mid;
  }
  pos[t] = tg - cu[lo];
}

// dst row r = src row map(r), rows of K floats (K = 1: a bias). mode 0 (query / key / value stacked, H rows each):
// inside every head of the first two thirds, row 2i <- row i, row 2i + 1 <- row i + d_h/2; mode 1 ([gate; up], n rows
// each): row 2j <- gate row j, row 2j + 1 <- up row j.
__global__ void reorder_rows_kernel(const float* __restrict__ src, int64_t total, int K, int mode, int n, int dh,
                                    float* __restrict__ dst) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int r = static_cast<int>(i / K), k = static_cast<int>(i - static_cast<int64_t>(r) * K);
  int from = r;
  if (mode == 0) {
    if (r < 2 * n) {
      const int local = r % dh, base = r - local;
      from = base + (local >> 1) + ((local & 1) ? (dh >> 1) : 0);
    }
  } else {
    from = (r >> 1) + ((r & 1) ? n : 0);
  }
  dst[i] = src[static_cast<int64_t>(from) * K + k];
}

// SiLU as x / (1 + 2^(-x log2 e)) on the hardware exp2 and reciprocal (1 ulp each: f32-class, as gelu_fast); the
// exact-erf GELU through erff where the result stays f32, through gelu_fast (|erf error| <= 1.5e-7) where it is
// rounded to f16 or split into (hi, lo) — the choices the plain FFN's epilogues make
template <bool F32OUT>
__device__ __forceinline__ float glu_act(float g, int ffn) {
  if (ffn == VR_FFN_SWIGLU) return g * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * g));
  if (F32OUT) return 0.5f * g * (1.0f + erff(g * 0.70710678118654752440f));
  return gelu_fast(g);
}

// out[t][j] = act(pre[t][j]) * pre[t][I + j] for 8 consecutive j per thread. TIN: the pre-activation's type.
// OUT 0: f32 rows; 1: interleaved (hi, lo) f16 rows (split_at); 2: plain f16 rows.
template <typename TIN, int OUT>
__global__ __launch_bounds__(256) void glu_kernel(const TIN* __restrict__ pre, int64_t n8, int I, int ffn,
                                                  float* __restrict__ out, half_t* __restrict__ out_h) {
  const int64_t i8 = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i8 >= n8) return;
  const int per_row = I >> 3;
  const int64_t t = i8 / per_row;
  const int j = static_cast<int>(i8 - t * per_row) << 3;
  const TIN* gp = pre + t * 2 * I + j;
  float g[8], u[8], v[8];
  load8(gp, g);
  load8(gp + I, u);
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = glu_act<OUT == 0>(g[k], ffn) * u[k];
  if constexpr (OUT == 0) {
    store8(out + t * I + j, v);
  } else if constexpr (OUT == 2) {
    store8(out_h + t * I + j, v);
  } else {
    f16x8 h, l;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      half_t hk, lk;
      split_f16(v[k], hk, lk);
      h[k] = hk;
      l[k] = lk;
    }
    half_t* o = out_h + t * 2 * I + split_at(j);
    *reinterpret_cast<f16x8*>(o) = h;
    *reinterpret_cast<f16x8*>(o + 8) = l;
  }
}

// ---- GEMM: C[M,N] = A[M,K] W[N,K]^T + bias (+ GELU | + R) ---------------------------------------

constexpr int BM = 128, BN = 128, BK = 32;
constexpr int LDT = BK + 4;  // padded LDS row (floats); rows stay 16-byte aligned

// F16: plain f16 output; RESIDUAL_LN: the residual is LayerNorm(R) re-derived from the pre-LN rows R and
// their (mean, 1/sigma) — both in the 256-tile kernel only
enum { EPI_BIAS = 0, EPI_BIAS_GELU = 1, EPI_BIAS_RESIDUAL = 2, EPI_BIAS_F16 = 3, EPI_BIAS_RESIDUAL_LN = 4,
       // LayerNorm folded into the GEMMs of the large-batch f16 path (forward_chunk, `fold_big`):
       //   LN(x) W^T = inv (x (g o W)^T - mean colsum(g o W)) + W b  — the consumer reads f16 PRE-LN rows and its
       //   epilogue applies the row statistics (FOLD_*: bias = c, ln_g = colsum, ln_stat = (mean, 1/sigma));
       //   the producer (RESIDUAL_LN_STATS) also stores its output rows as f16 and per-(row, 64 columns)
       //   partial (sum, sum of squares), from which ln_finalize_kernel makes the statistics.
       EPI_FOLD_F16 = 5, EPI_FOLD_GELU = 6, EPI_BIAS_RESIDUAL_LN_STATS = 7,
       // ... with an f16 RESIDUAL STREAM (gemm_f16_pp_kernel only): the pre-LayerNorm rows exist as f16 only — the
       // array the next projection reads anyway — so the producer stores 2 bytes per element instead of 6 and
       // the residual read is 2 bytes instead of 4 (the statistics still come from the f32 sums before the
       // rounding). R32_O16: residual rows still f32 (layer 0: the embedding sum), f16 out; R16_O16: f16 in and
       // out, IN PLACE (every element is read and written by the same lane); R16_O32: f16 in, f32 + f16 out
       // (the last layer of a mean-pooled model: the final LayerNorm and the pooling read f32 rows).
       EPI_RLS_R32_O16 = 8, EPI_RLS_R16_O16 = 9, EPI_RLS_R16_O32 = 10,
       // the skinny kernels only (at most 256 rows; skinny_apply), over the re-ordered matrices of LayerWeights:
       // ROPE_F16: bias, then the (x, y) column pairs of the query and key thirds rotated by the row's position
       // (ln_stat = the cos/sin table, ln_g = the int32 positions), f16 out; *GLU_F16: bias, act(gate) * up of the
       // (gate, up) column pairs, N/2 f16 columns out
       EPI_ROPE_F16 = 11, EPI_SWIGLU_F16 = 12, EPI_GEGLU_F16 = 13,
       // the direct_epilogue kernels (mid, ping-pong) on the large-batch path: FOLD_F16's folded LayerNorm over the
       // gain-scaled INTERLEAVED matrix, then act(gate) * up of the lane's four (gate, up) column pairs, N/2 f16 columns out
       EPI_FOLD_SWIGLU = 14, EPI_FOLD_GEGLU = 15,
       // BIAS_GELU with max(x, 0) in the GELU's place (VR_FFN_RELU), in every kernel BIAS_GELU exists for, same output forms
       EPI_BIAS_RELU = 16 };

// Run-time epilogue id -> template argument: f(std::integral_constant<int, E>{}) for the E of the list that equals
// `epi`. Every launcher names the epilogues its kernel is instantiated for once, in its call of this; an id outside
// that list launches nothing and returns false, which the launcher reports as an error.
template <int... E, class F>
static bool with_epi(int epi, F&& f) {
  return ((epi == E && (f(std::integral_constant<int, E>{}), true)) || ...);
}

// Linear tile id -> (row panel, column panel), row panels taken kGroupM at a time with the column
// index slow inside a group. The ~32 blocks an XCD runs together then cover ~8 row panels x ~4
// column panels, so both operands' working set (~4 MB per sweep of K) fits the XCD's 4-MiB L2;
// with the plain column-fastest order all of W (7-9 MB) cycles through L2 for every row panel.
constexpr int kGroupM = 8;
__device__ __forceinline__ void grouped_tile(int id, int tiles_m, int tiles_n, int& tm, int& tn) {
  const int per_group = kGroupM * tiles_n;
  const int group = id / per_group;
  const int within = id - group * per_group;
  const int gm = min(kGroupM, tiles_m - group * kGroupM);
  tm = group * kGroupM + within % gm;
  tn = within / gm;
}

template <int EPI>
__global__ __launch_bounds__(256) void gemm_f32_kernel(const float* __restrict__ A,
                                                       const float* __restrict__ W,
                                                       const float* __restrict__ bias,
                                                       const float* __restrict__ R,
                                                       float* __restrict__ C, int M, int N, int K) {
  __shared__ float lds[2 * (BM + BN) * LDT];
  float* sA = lds;                 // [2][BM*LDT]
  float* sB = lds + 2 * BM * LDT;  // [2][BN*LDT]

  // XCD-aware tile order: blocks that share an XCD (blockIdx % 8) walk consecutive tiles of one
  // row panel, so the A panel and the W columns they re-read stay in that XCD's L2.
  const int tiles_n = N / BN;
  const int nwg = gridDim.x;
  const int bid = blockIdx.x;
  const int q8 = nwg / 8, r8 = nwg % 8, xcd = bid % 8;
  const int swz = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + bid / 8;
  int tm, tn;
  grouped_tile(swz, (M + BM - 1) / BM, tiles_n, tm, tn);
  const int bm = tm * BM;
  const int bn = tn * BN;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  // global -> register staging: thread covers rows (tid>>3) + 32p, 16 bytes at column (tid&7)*4
  const int lrow = tid >> 3;
  const int lcol = (tid & 7) * 4;
  // A rows past M are clamped to row M-1: they only feed C rows that are never stored.
  const float* w_g = W + static_cast<int64_t>(bn + lrow) * K + lcol;
  const int64_t rstep = static_cast<int64_t>(32) * K;
  const int last = M - 1;
  const float* a_g0 = A + static_cast<int64_t>(min(bm + lrow, last)) * K + lcol;
  const float* a_g1 = A + static_cast<int64_t>(min(bm + lrow + 32, last)) * K + lcol;
  const float* a_g2 = A + static_cast<int64_t>(min(bm + lrow + 64, last)) * K + lcol;
  const float* a_g3 = A + static_cast<int64_t>(min(bm + lrow + 96, last)) * K + lcol;
  float4 ra0, ra1, ra2, ra3, rw0, rw1, rw2, rw3;
#define VR_LOAD_TILE(k0)                                                                         \
  do {                                                                                           \
    ra0 = *reinterpret_cast<const float4*>(a_g0 + (k0));                                         \
    ra1 = *reinterpret_cast<const float4*>(a_g1 + (k0));                                         \
    ra2 = *reinterpret_cast<const float4*>(a_g2 + (k0));                                         \
    ra3 = *reinterpret_cast<const float4*>(a_g3 + (k0));                                         \
    rw0 = *reinterpret_cast<const float4*>(w_g + (k0));                                          \
    rw1 = *reinterpret_cast<const float4*>(w_g + rstep + (k0));                                  \
    rw2 = *reinterpret_cast<const float4*>(w_g + 2 * rstep + (k0));                              \
    rw3 = *reinterpret_cast<const float4*>(w_g + 3 * rstep + (k0));                              \
  } while (0)
#define VR_STORE_TILE(buf)                                                                       \
  do {                                                                                           \
    float* da = sA + (buf) * BM * LDT + lrow * LDT + lcol;                                       \
    float* db = sB + (buf) * BN * LDT + lrow * LDT + lcol;                                       \
    *reinterpret_cast<float4*>(da) = ra0;                                                        \
    *reinterpret_cast<float4*>(da + 32 * LDT) = ra1;                                             \
    *reinterpret_cast<float4*>(da + 64 * LDT) = ra2;                                             \
    *reinterpret_cast<float4*>(da + 96 * LDT) = ra3;                                             \
    *reinterpret_cast<float4*>(db) = rw0;                                                        \
    *reinterpret_cast<float4*>(db + 32 * LDT) = rw1;                                             \
    *reinterpret_cast<float4*>(db + 64 * LDT) = rw2;                                             \
    *reinterpret_cast<float4*>(db + 96 * LDT) = rw3;                                             \
  } while (0)

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  const int nk = K / BK;
  VR_LOAD_TILE(0);
  VR_STORE_TILE(0);
  __syncthreads();

  // MFMA operand addressing: lane l supplies row/col (l & 31) and k-slot (l >> 5); its float4
  // read at k offset kk + 4*(l>>5) feeds four MFMAs (component c covers k = kk + 4*(l>>5) + c;
  // A and B use the same map, so every product pairs equal k).
  const int frow = lane & 31;
  const int fk = 4 * (lane >> 5);
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) VR_LOAD_TILE((kt + 1) * BK);
    const float* a_base = sA + buf * BM * LDT + (wm * 64 + frow) * LDT + fk;
    const float* b_base = sB + buf * BN * LDT + (wn * 64 + frow) * LDT + fk;
#pragma unroll
    for (int kk = 0; kk < BK; kk += 8) {
      float4 a0 = *reinterpret_cast<const float4*>(a_base + kk);
      float4 a1 = *reinterpret_cast<const float4*>(a_base + 32 * LDT + kk);
      float4 b0 = *reinterpret_cast<const float4*>(b_base + kk);
      float4 b1 = *reinterpret_cast<const float4*>(b_base + 32 * LDT + kk);
      const float av[2][4] = {{a0.x, a0.y, a0.z, a0.w}, {a1.x, a1.y, a1.z, a1.w}};
      const float bv[2][4] = {{b0.x, b0.y, b0.z, b0.w}, {b1.x, b1.y, b1.z, b1.w}};
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][c], bv[j][c], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) VR_STORE_TILE(buf ^ 1);
    __syncthreads();
  }

#undef VR_LOAD_TILE
#undef VR_STORE_TILE

  // C/D map of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8*(reg >> 2) + 4*(lane >> 5)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = bn + wn * 64 + j * 32 + (lane & 31);
      const float bs = bias[col];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = bm + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < M) {
          float v = acc[i][j][r] + bs;
          if (EPI == EPI_BIAS_GELU) v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
          if (EPI == EPI_BIAS_RELU) v = fmaxf(v, 0.0f);
          if (EPI == EPI_BIAS_RESIDUAL) v += R[static_cast<int64_t>(row) * N + col];
          C[static_cast<int64_t>(row) * N + col] = v;
        }
      }
    }
}

static int launch_gemm(vr_engine* e, int epi, const float* A, const float* W, const float* bias,
                       const float* R, float* C, int M, int N, int K) {
  VR_CHECK(N % BN == 0 && K % BK == 0, "GEMM shape N=%d K=%d must be multiples of %d / %d", N, K, BN, BK);
  if (M <= 0) return 0;
  hipStream_t s = e->stream;
  const int grid = ((M + BM - 1) / BM) * (N / BN);
  prof_begin(e, VR_PROF_GEMM, 2.0 * M * static_cast<double>(N) * K);
  const bool known = with_epi<EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESIDUAL, EPI_BIAS_RELU>(epi, [&](auto E) {
    hipLaunchKernelGGL((gemm_f32_kernel<decltype(E)::value>), dim3(grid), dim3(256), 0, s, A, W, bias, R, C, M, N, K);
  });
  prof_end(e);
  VR_CHECK(known, "epilogue %d does not exist for the f32 GEMM (M=%d N=%d K=%d)", epi, M, N, K);
  VR_HIP(hipGetLastError());
  return 0;
}

// ---- GEMM, split precision: C = (A_hi + A_lo)(W_hi + W_lo)^T * unscale + bias ... ---------------------

constexpr int HBM_ = 128, HBN_ = 128, HBK_ = 64;  // block tile; 64 f16 along K = one 128-B line per row
constexpr int HLDT = HBK_ + 8;                     // padded LDS row: 72 halfs = 144 B (conflict-free b128 reads)

// Same 128x128 block / 64x64 wave decomposition as gemm_f32_kernel, on v_mfma_f32_32x32x16_f16:
// per 16-deep k-step a wave reads hi and lo fragments of 2 A tiles and 2 B tiles (8 ds_read_b128)
// and issues 2*2*3 MFMAs (hi*hi, hi*lo, lo*hi) into one f32 accumulator per tile.
// Staging moves whole 128-B lines (8 lanes x 16 B per row): the next K-tile is loaded into
// registers while the current one is multiplied out of the single 72-KiB LDS image (2 blocks/CU).
// EPI_BIAS: f32 out. EPI_BIAS_GELU / EPI_BIAS_RELU: split (hi, lo) out only. EPI_BIAS_RESIDUAL: + R, f32 out.
template <int EPI>
__global__ __launch_bounds__(256) void gemm_f16x3_kernel(
    const half_t* __restrict__ Ah, const half_t* __restrict__ Al, const half_t* __restrict__ Wh,
    const half_t* __restrict__ Wl, const float* __restrict__ bias, const float* __restrict__ R,
    float* __restrict__ C, half_t* __restrict__ Ch, half_t* __restrict__ Cl, int M, int N, int K,
    float unscale) {
  __shared__ half_t lds[4 * HBM_ * HLDT];  // [Ah, Al, Wh, Wl][128][HLDT] = 72 KiB
  const int tiles_n = N / HBN_;
  const int nwg = gridDim.x;
  const int bid = blockIdx.x;
  const int q8 = nwg / 8, r8 = nwg % 8, xcd = bid % 8;
  const int swz = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + bid / 8;
  int tm, tn;
  grouped_tile(swz, (M + HBM_ - 1) / HBM_, tiles_n, tm, tn);
  const int bm = tm * HBM_;
  const int bn = tn * HBN_;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  // staging: thread t moves the 16-B piece (t & 7) of rows (t >> 3) + 32p, p = 0..3, of each array
  const int lrow = tid >> 3;
  const int lcol = (tid & 7) * 8;
  const int last = M - 1;
  // (named registers, not arrays: arrays indexed inside macros ended up in scratch memory)
  // (interleaved (hi, lo) rows of 2K halfs, see split_at: 8 halfs of k sit 16 apart)
  const int64_t a_off0 = static_cast<int64_t>(min(bm + lrow, last)) * (2 * K) + 2 * lcol;
  const int64_t a_off1 = static_cast<int64_t>(min(bm + lrow + 32, last)) * (2 * K) + 2 * lcol;
  const int64_t a_off2 = static_cast<int64_t>(min(bm + lrow + 64, last)) * (2 * K) + 2 * lcol;
  const int64_t a_off3 = static_cast<int64_t>(min(bm + lrow + 96, last)) * (2 * K) + 2 * lcol;
  const int64_t w_off0 = static_cast<int64_t>(bn + lrow) * (2 * K) + 2 * lcol;
  const int64_t w_step = static_cast<int64_t>(32) * (2 * K);
  uint4 r_ah0, r_ah1, r_ah2, r_ah3, r_al0, r_al1, r_al2, r_al3;
  uint4 r_wh0, r_wh1, r_wh2, r_wh3, r_wl0, r_wl1, r_wl2, r_wl3;
#define VR_HLOAD1(P, k0)                                                              \
  r_ah##P = *reinterpret_cast<const uint4*>(Ah + a_off##P + 2 * (k0));                \
  r_al##P = *reinterpret_cast<const uint4*>(Al + a_off##P + 2 * (k0));                \
  r_wh##P = *reinterpret_cast<const uint4*>(Wh + w_off0 + P * w_step + 2 * (k0));     \
  r_wl##P = *reinterpret_cast<const uint4*>(Wl + w_off0 + P * w_step + 2 * (k0));
#define VR_HLOAD(k0) \
  do {               \
    VR_HLOAD1(0, k0) VR_HLOAD1(1, k0) VR_HLOAD1(2, k0) VR_HLOAD1(3, k0) \
  } while (0)
#define VR_HSTORE1(P)                                                                 \
  *reinterpret_cast<uint4*>(lds + (lrow + 32 * P) * HLDT + lcol) = r_ah##P;                          \
  *reinterpret_cast<uint4*>(lds + HBM_ * HLDT + (lrow + 32 * P) * HLDT + lcol) = r_al##P;            \
  *reinterpret_cast<uint4*>(lds + 2 * HBM_ * HLDT + (lrow + 32 * P) * HLDT + lcol) = r_wh##P;        \
  *reinterpret_cast<uint4*>(lds + 3 * HBM_ * HLDT + (lrow + 32 * P) * HLDT + lcol) = r_wl##P;
#define VR_HSTORE() \
  do {              \
    VR_HSTORE1(0) VR_HSTORE1(1) VR_HSTORE1(2) VR_HSTORE1(3) \
  } while (0)

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  const int nk = K / HBK_;
  VR_HLOAD(0);
  VR_HSTORE();
  __syncthreads();

  // 32x32x16 f16 operands: lane l supplies row/col (l & 31), k = 8*(l >> 5) + j, j = 0..7 (16 B)
  const int frow = lane & 31;
  const int fk = 8 * (lane >> 5);
  const half_t* pa = lds + (wm * 64 + frow) * HLDT + fk;
  const half_t* pw = lds + 2 * HBM_ * HLDT + (wn * 64 + frow) * HLDT + fk;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) VR_HLOAD((kt + 1) * HBK_);
#pragma unroll
    for (int kk = 0; kk < HBK_; kk += 16) {
      f16x8 ah[2], al[2], wh[2], wl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        ah[i] = *reinterpret_cast<const f16x8*>(pa + i * 32 * HLDT + kk);
        al[i] = *reinterpret_cast<const f16x8*>(pa + HBM_ * HLDT + i * 32 * HLDT + kk);
        wh[i] = *reinterpret_cast<const f16x8*>(pw + i * 32 * HLDT + kk);
        wl[i] = *reinterpret_cast<const f16x8*>(pw + HBM_ * HLDT + i * 32 * HLDT + kk);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], wh[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], wl[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], wh[j], acc[i][j], 0, 0, 0);
        }
    }
    __syncthreads();  // every wave is done reading this K-tile
    if (kt + 1 < nk) VR_HSTORE();
    __syncthreads();
  }
#undef VR_HLOAD
#undef VR_HLOAD1
#undef VR_HSTORE
#undef VR_HSTORE1

  // Epilogue through LDS (free now: the loop ended on a barrier). In the MFMA's C layout a lane
  // owns one column and 16 scattered rows, which gives 4-byte (or, split, 2-byte) stores — they
  // cost a quarter of the kernel. Each wave parks its 64x64 tile in its own LDS region and reads
  // it back by rows: 16 lanes x 16 B cover a 256-B row segment, bias / GELU / residual / split are
  // applied on float4s, and every global access is 16 B (8 B for the f16 halves).
  constexpr int SLD = 64 + 4;  // padded row of the staging tile (floats)
  float* stage = reinterpret_cast<float*>(lds) + wave * (64 * SLD);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        stage[(i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * SLD + j * 32 + (lane & 31)] = acc[i][j][r];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();  // the region is private to this wave: no block barrier needed
  const int c4 = (lane & 15) * 4;
  const int gcol = bn + wn * 64 + c4;
  const float4 b4 = *reinterpret_cast<const float4*>(bias + gcol);
#pragma unroll 4
  for (int it = 0; it < 16; ++it) {
    const int lr = it * 4 + (lane >> 4);
    const int grow = bm + wm * 64 + lr;
    float4 v = *reinterpret_cast<const float4*>(stage + lr * SLD + c4);
    if (grow >= M) continue;
    v.x = v.x * unscale + b4.x;
    v.y = v.y * unscale + b4.y;
    v.z = v.z * unscale + b4.z;
    v.w = v.w * unscale + b4.w;
    const int64_t o = static_cast<int64_t>(grow) * N + gcol;
    if (EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_RELU) {
      float g[4] = {v.x, v.y, v.z, v.w};
      half_t h[4], l[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        g[c] = EPI == EPI_BIAS_RELU ? fmaxf(g[c], 0.0f) : gelu_fast(g[c]);
        split_f16(g[c], h[c], l[c]);
      }
      const int64_t so = static_cast<int64_t>(grow) * (2 * N) + split_at(gcol);
      *reinterpret_cast<uint2*>(Ch + so) = *reinterpret_cast<const uint2*>(h);
      *reinterpret_cast<uint2*>(Cl + so) = *reinterpret_cast<const uint2*>(l);
    } else {
      if (EPI == EPI_BIAS_RESIDUAL) {
        const float4 r4 = *reinterpret_cast<const float4*>(R + o);
        v.x += r4.x;
        v.y += r4.y;
        v.z += r4.z;
        v.w += r4.w;
      }
      *reinterpret_cast<float4*>(C + o) = v;
    }
  }
}

// ---- the same product on a 256x256 block tile -----------------------------------------------------
//
// 8 waves as 2(M) x 4(N), wave tile 128x64 = 4x2 MFMA tiles: per 16-deep k-step a wave reads 12
// fragments (8 of A, 4 of W; hi and lo) for 24 MFMAs — half the LDS bytes per MFMA of the 128x128
// kernel above, whose LDS pipe was as busy as its matrix pipe. One block per CU (128 KiB of LDS):
// two 64-KiB stages [A, W][256 rows][128 B = 32 k of hi and lo], filled by global_load_lds_dwordx4 (no
// staging registers, no ds_write pass) for K-tile t+1 while K-tile t is multiplied; one barrier per
// K-tile. A direct-to-LDS load writes wave-uniform base + lane*16, so the image is unpadded; bank
// conflicts are avoided by an XOR swizzle applied on the SOURCE side: LDS chunk p of row r holds
// the row's 16-byte chunk p ^ ((r >> 1) & 7), and fragment reads use the same permutation (every
// lane group of a ds_read_b128 then covers all 64 banks once).

constexpr int GBM = 256, GBN = 256, GBK = 32;
constexpr int kStageHalfs = 4 * 256 * GBK;  // 64 KiB
constexpr int kGroupM256 = 4;

__device__ __forceinline__ void glds16(const half_t* src, half_t* lds_dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}

// PASSES = 3: split operands, interleaved (hi, lo) rows of 2K halfs (split_at), 32-deep K-tiles.
// PASSES = 1: plain f16 operands (VR_PRECISION_F16), rows of K halfs, 64-deep K-tiles. Either way a
// K-tile of one row is one 128-byte line, so staging, swizzle and LDS image are the same code.
template <int EPI, int PASSES>
__global__ __launch_bounds__(512) void gemm_f16x3_256_kernel(
    const half_t* __restrict__ Ah, const half_t* __restrict__ Al, const half_t* __restrict__ Wh,
    const half_t* __restrict__ Wl, const float* __restrict__ bias, const float* __restrict__ R,
    float* __restrict__ C, half_t* __restrict__ Ch, half_t* __restrict__ Cl, int M, int N, int K,
    float unscale, const float2* __restrict__ ln_stat, const float* __restrict__ ln_g,
    const float* __restrict__ ln_b) {
  __shared__ half_t lds[2 * kStageHalfs];  // the only LDS object of the kernel (a second one makes hipcc
                                           // drain the in-flight loads before every fragment read)
  // Persistent blocks: the grid is one block per CU and every block walks tiles g, g + G, g + 2G, ...
  // Inside a wave of G tiles the blocks that share an XCD (blockIdx % 8) take consecutive tiles, and
  // consecutive tiles are grouped kGroupM256 row panels at a time with the column index slow, so the
  // A panels and W columns an XCD re-reads stay in its L2.
  const int tiles_n = (N + GBN - 1) / GBN;  // N may end inside the last column tile (rows clamped, stores guarded)
  const int tiles_m = (M + GBM - 1) / GBM;
  const int total = tiles_m * tiles_n;
  const int G = gridDim.x;
  const int local = (G % 8 == 0) ? (static_cast<int>(blockIdx.x) % 8) * (G / 8) + static_cast<int>(blockIdx.x) / 8
                                 : static_cast<int>(blockIdx.x);
  auto coords = [&](int t, int& bm_, int& bn_) {
    const int per_group = kGroupM256 * tiles_n;
    const int group = t / per_group;
    const int within = t - group * per_group;
    const int gm = min(kGroupM256, tiles_m - group * kGroupM256);
    bm_ = (group * kGroupM256 + within % gm) * GBM;
    bn_ = (within / gm) * GBN;
  };
  int tile = local;
  if (tile >= total) return;  // block-uniform
  int bm, bn;
  coords(tile, bm, bn);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;

  // staging: a direct-to-LDS load moves 8 rows x 128 B (one line per row: 32 k of hi and lo, see
  // split_at). Wave w fills row groups w, w + 8, w + 16, w + 24 of the A image and of the W image;
  // lane -> row (lane >> 3) of the group, LDS chunk (lane & 7), source chunk (lane & 7) ^ ((row >> 1) & 7).
  const int srow = lane >> 3;
  const int schunk = ((lane & 7) ^ ((4 * (wave & 1) + (lane >> 4)) & 7)) * 8;
  const int r0 = wave * 8 + srow;  // + 64 j
  const int64_t K2 = (PASSES == 3 ? 2 : 1) * static_cast<int64_t>(K);  // halfs per operand row
  const half_t *g_a0, *g_a1, *g_a2, *g_a3, *g_w0, *g_w1, *g_w2, *g_w3;
  auto set_ptrs = [&](int bm_, int bn_) {
    g_a0 = Ah + static_cast<int64_t>(min(bm_ + r0, M - 1)) * K2 + schunk;
    g_a1 = Ah + static_cast<int64_t>(min(bm_ + r0 + 64, M - 1)) * K2 + schunk;
    g_a2 = Ah + static_cast<int64_t>(min(bm_ + r0 + 128, M - 1)) * K2 + schunk;
    g_a3 = Ah + static_cast<int64_t>(min(bm_ + r0 + 192, M - 1)) * K2 + schunk;
    g_w0 = Wh + static_cast<int64_t>(min(bn_ + r0, N - 1)) * K2 + schunk;
    g_w1 = Wh + static_cast<int64_t>(min(bn_ + r0 + 64, N - 1)) * K2 + schunk;
    g_w2 = Wh + static_cast<int64_t>(min(bn_ + r0 + 128, N - 1)) * K2 + schunk;
    g_w3 = Wh + static_cast<int64_t>(min(bn_ + r0 + 192, N - 1)) * K2 + schunk;
  };
  set_ptrs(bm, bn);
  half_t* l_dst = lds + wave * 8 * 64;  // rows of 64 halfs (128 B); the W image starts at 256 * 64
#define VR_GLDS_STAGE(buf, k0)                                          \
  do {                                                                  \
    half_t* d = l_dst + (buf) * kStageHalfs;                            \
    glds16(g_a0 + (k0), d);                                         \
    glds16(g_a1 + (k0), d + 64 * 64);                               \
    glds16(g_a2 + (k0), d + 128 * 64);                              \
    glds16(g_a3 + (k0), d + 192 * 64);                              \
    glds16(g_w0 + (k0), d + 256 * 64);                              \
    glds16(g_w1 + (k0), d + 256 * 64 + 64 * 64);                    \
    glds16(g_w2 + (k0), d + 256 * 64 + 128 * 64);                   \
    glds16(g_w3 + (k0), d + 256 * 64 + 192 * 64);                   \
  } while (0)

  f32x4 acc[8][4];

  // v_mfma_f32_16x16x32_f16 fragments: lane l supplies row (l & 15), k = 8*(l >> 4) + j of a 32-deep step
  // (the chip holds a higher clock on this shape than on 32x32x16 at the same work per cycle).
  // PASSES 3: k8-group g = l >> 4 of the 32-deep tile, hi = chunk 2g, lo = chunk 2g + 1.
  // PASSES 1: chunk 4*kk + (l >> 4) of the 64-deep tile.
  const int frow = lane & 15;
  const int fsw = (frow >> 1) & 7;
  const int fq = lane >> 4;
  const int pa = (wm * 128 + frow) * 64;
  const int pw = 256 * 64 + (wn * 64 + frow) * 64;

  constexpr int kTileHalfs = 64;               // halfs of one row per K-tile: 32 k x (hi, lo) or 64 k
  const int nk = K / (PASSES == 3 ? 32 : 64);
  int par = 0;  // stage buffer holding K-tile 0 of the current tile
  VR_GLDS_STAGE(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  while (true) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the next tile of this block: its first K-tile is loaded during this tile's LAST K-tile, so only the
  // first tile of a block pays a prologue, and this tile's stores drain under the next main loop
  const int next = tile + G;
  const bool has_next = next < total;
  int nbm = bm, nbn = bn;
  if (has_next) coords(next, nbm, nbn);
  for (int kt = 0; kt < nk; ++kt) {
    if (kt == nk - 1 && has_next) set_ptrs(nbm, nbn);
    const half_t* st = lds + ((par + kt) & 1) * kStageHalfs;
    // A direct-to-LDS load holds the issuing wave for ~100+ cycles. Eight of them in a row at the top
    // of the K-tile left the matrix pipe idle for a third of it; instead one load is issued after
    // every row of MFMA tiles, where the partner wave of the SIMD fills the gap.
    half_t* nd = l_dst + ((par + kt + 1) & 1) * kStageHalfs;
    const int nk0 = kt + 1 < nk ? (kt + 1) * kTileHalfs : 0;  // K-tile 0 of the next tile (or, at the very end, a harmless re-load)
    constexpr int kSteps = PASSES == 3 ? 1 : 2;  // 32-deep MFMA steps per K-tile
#pragma unroll
    for (int kk = 0; kk < kSteps; ++kk) {
      // the four weight fragments stay resident for the step; activation fragments are read one row
      // of tiles ahead of their MFMAs
      f16x8 wh[4], wl[4], ah[2], al[2];
      const int fh = PASSES == 3 ? ((2 * fq) ^ fsw) * 8 : ((4 * kk + fq) ^ fsw) * 8;
      const int fl = ((2 * fq + 1) ^ fsw) * 8;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        wh[j] = *reinterpret_cast<const f16x8*>(st + pw + j * 16 * 64 + fh);
        if (PASSES == 3) wl[j] = *reinterpret_cast<const f16x8*>(st + pw + j * 16 * 64 + fl);
      }
      ah[0] = *reinterpret_cast<const f16x8*>(st + pa + fh);
      if (PASSES == 3) al[0] = *reinterpret_cast<const f16x8*>(st + pa + fl);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (i + 1 < 8) {
          ah[(i + 1) & 1] = *reinterpret_cast<const f16x8*>(st + pa + (i + 1) * 16 * 64 + fh);
          if (PASSES == 3) al[(i + 1) & 1] = *reinterpret_cast<const f16x8*>(st + pa + (i + 1) * 16 * 64 + fl);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i & 1], wh[j], acc[i][j], 0, 0, 0);
          if (PASSES == 3) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i & 1], wl[j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i & 1], wh[j], acc[i][j], 0, 0, 0);
          }
        }
        if (kk == 0) {
          const int piece = i;  // compile-time after unrolling
          const half_t* src = piece == 0 ? g_a0 : piece == 1 ? g_a1 : piece == 2 ? g_a2 : piece == 3 ? g_a3
                            : piece == 4 ? g_w0 : piece == 5 ? g_w1 : piece == 6 ? g_w2 : g_w3;
          glds16(src + nk0, nd + (piece >> 2) * 256 * 64 + (piece & 3) * 64 * 64);
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the load where it was written, between the MFMA rows
        // (measured: dropping this barrier, or s_setprio(1) around the MFMA rows, changes nothing: +-0.5 %)
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces of K-tile kt+1 have landed
    __syncthreads();                                   // ... everybody's have, and K-tile kt is consumed
  }

  // Epilogue through LDS, 16 rows of the wave at a time (see gemm_f16x3_kernel): the wave parks 16x64
  // accumulators in its own region of the stage buffer that does NOT hold the next tile's first K-tile
  // and reads them back by rows for 16-byte accesses.
  // The residual rows of a tile are requested one tile AHEAD, all eight loads at once: read one by
  // one inside the store loop they cost eight exposed HBM latencies per tile.
  constexpr int SLD = 64 + 4;
  const int sbuf = ((par + nk) & 1) ^ 1;
  float* stage = reinterpret_cast<float*>(lds) + sbuf * (kStageHalfs / 2) + wave * (16 * SLD);
  const int c4 = (lane & 15) * 4;
  const int gcol = bn + wn * 64 + c4;
  const bool col_ok = gcol < N;  // N % 4 == 0: a lane's four columns are in or out together
  const float4 b4 = *reinterpret_cast<const float4*>(bias + (col_ok ? gcol : 0));
  constexpr bool kFold = EPI == EPI_FOLD_F16 || EPI == EPI_FOLD_GELU;
  constexpr bool kStats = EPI == EPI_BIAS_RESIDUAL_LN_STATS;
  constexpr bool kResidLN = EPI == EPI_BIAS_RESIDUAL_LN || kStats;
  constexpr bool kResidual = EPI == EPI_BIAS_RESIDUAL || kResidLN;
  // LayerNorm weight / bias of this lane's columns (residual re-derivation), or, folded consumers: the
  // column sums of the LayerNorm-scaled weight matrix
  float4 lg4 = make_float4(0.f, 0.f, 0.f, 0.f), lb4 = lg4;
  if (kResidLN || kFold) lg4 = *reinterpret_cast<const float4*>(ln_g + (col_ok ? gcol : 0));
  if (kResidLN) lb4 = *reinterpret_cast<const float4*>(ln_b + (col_ok ? gcol : 0));
  // The residual rows of a 16-row piece are requested one piece AHEAD, four loads at once (read one
  // by one inside the store loop they cost an exposed HBM latency each), with their (mean, 1/sigma)
  // when the residual is a LayerNorm output.
  float4 r4[2][4];
  float2 st4[2][4];
  auto fetch_residual = [&](int pc, float4 (&r)[4], float2 (&st)[4]) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int64_t rr = min(bm + wm * 128 + 16 * pc + (lane >> 4) + 4 * it, M - 1);
      if (kResidual) r[it] = *reinterpret_cast<const float4*>(R + rr * N + (col_ok ? gcol : 0));
      if (kResidLN || kFold) st[it] = ln_stat[rr];
    }
  };
  if (kResidual || kFold) fetch_residual(0, r4[0], st4[0]);
#pragma unroll
  for (int pc = 0; pc < 8; ++pc) {  // piece pc = rows 16 pc .. 16 pc + 15 of the wave's 128 = MFMA tile row pc
    const int row0 = bm + wm * 128 + 16 * pc + (lane >> 4);  // + 4 * it
    if ((kResidual || kFold) && pc + 1 < 8) fetch_residual(pc + 1, r4[(pc + 1) & 1], st4[(pc + 1) & 1]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        stage[(4 * (lane >> 4) + r) * SLD + j * 16 + (lane & 15)] = acc[pc][j][r];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    auto emit = [&](int it) {
      const int lr = it * 4 + (lane >> 4);
      const int grow = row0 + 4 * it;
      float4 v = *reinterpret_cast<const float4*>(stage + lr * SLD + c4);
      const bool ok = grow < M && col_ok;
      if (!kStats && !ok) return;  // (the statistics variant keeps every lane for its row sums)
      if (kFold) {  // inv (acc unscale - mean colsum) + c
        const float2 st = st4[pc & 1][it];
        v.x = fmaf(fmaf(v.x, unscale, -(st.x * lg4.x)), st.y, b4.x);
        v.y = fmaf(fmaf(v.y, unscale, -(st.x * lg4.y)), st.y, b4.y);
        v.z = fmaf(fmaf(v.z, unscale, -(st.x * lg4.z)), st.y, b4.z);
        v.w = fmaf(fmaf(v.w, unscale, -(st.x * lg4.w)), st.y, b4.w);
      } else {
        v.x = v.x * unscale + b4.x;
        v.y = v.y * unscale + b4.y;
        v.z = v.z * unscale + b4.z;
        v.w = v.w * unscale + b4.w;
      }
      const int64_t o = static_cast<int64_t>(grow) * N + gcol;
      if (EPI == EPI_BIAS_RELU) {  // (split_f16 saturates)
        const float g[4] = {fmaxf(v.x, 0.0f), fmaxf(v.y, 0.0f), fmaxf(v.z, 0.0f), fmaxf(v.w, 0.0f)};
        half_t h[4], l[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) split_f16(g[c], h[c], l[c]);
        if (PASSES == 3) {
          const int64_t so = static_cast<int64_t>(grow) * (2 * N) + split_at(gcol);
          *reinterpret_cast<uint2*>(Ch + so) = *reinterpret_cast<const uint2*>(h);
          *reinterpret_cast<uint2*>(Cl + so) = *reinterpret_cast<const uint2*>(l);
        } else {
          *reinterpret_cast<uint2*>(Ch + o) = *reinterpret_cast<const uint2*>(h);
        }
      } else if (EPI == EPI_BIAS_GELU || EPI == EPI_FOLD_GELU) {
        const f32x2 g01 = PASSES == 1 ? gelu_poly2(f32x2{v.x, v.y}) : gelu_fast2(f32x2{v.x, v.y});
        const f32x2 g23 = PASSES == 1 ? gelu_poly2(f32x2{v.z, v.w}) : gelu_fast2(f32x2{v.z, v.w});
        float g[4] = {g01.x, g01.y, g23.x, g23.y};
        half_t h[4], l[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) split_f16(g[c], h[c], l[c]);
        if (PASSES == 3) {
          const int64_t so = static_cast<int64_t>(grow) * (2 * N) + split_at(gcol);
          *reinterpret_cast<uint2*>(Ch + so) = *reinterpret_cast<const uint2*>(h);
          *reinterpret_cast<uint2*>(Cl + so) = *reinterpret_cast<const uint2*>(l);
        } else {
          *reinterpret_cast<uint2*>(Ch + o) = *reinterpret_cast<const uint2*>(h);  // plain f16 rows
        }
      } else if (EPI == EPI_BIAS_F16 || EPI == EPI_FOLD_F16) {  // Q, K, V for the f16 attention kernel
        half_t h[4] = {static_cast<half_t>(fminf(fmaxf(v.x, -65504.0f), 65504.0f)),
                       static_cast<half_t>(fminf(fmaxf(v.y, -65504.0f), 65504.0f)),
                       static_cast<half_t>(fminf(fmaxf(v.z, -65504.0f), 65504.0f)),
                       static_cast<half_t>(fminf(fmaxf(v.w, -65504.0f), 65504.0f))};
        *reinterpret_cast<uint2*>(Ch + o) = *reinterpret_cast<const uint2*>(h);
      } else {
        if (EPI == EPI_BIAS_RESIDUAL) {
          v.x += r4[pc & 1][it].x;
          v.y += r4[pc & 1][it].y;
          v.z += r4[pc & 1][it].z;
          v.w += r4[pc & 1][it].w;
        }
        if (kResidLN) {  // residual = LayerNorm(R row), exactly as the LN kernel would have stored it
          const float2 st = st4[pc & 1][it];
          v.x += ln_apply(r4[pc & 1][it].x, st.x, st.y, lg4.x, lb4.x);
          v.y += ln_apply(r4[pc & 1][it].y, st.x, st.y, lg4.y, lb4.y);
          v.z += ln_apply(r4[pc & 1][it].z, st.x, st.y, lg4.z, lb4.z);
          v.w += ln_apply(r4[pc & 1][it].w, st.x, st.y, lg4.w, lb4.w);
        }
        if (!kStats) {
          *reinterpret_cast<float4*>(C + o) = v;
        } else {
          // the pre-LayerNorm row also goes out as f16 (the next projection's operand), and this wave's 64
          // columns of it contribute a (sum, sum of squares) to the row's statistics
          float s1 = 0.0f, s2 = 0.0f;
          if (ok) {
            *reinterpret_cast<float4*>(C + o) = v;
            half_t h[4] = {static_cast<half_t>(fminf(fmaxf(v.x, -65504.0f), 65504.0f)),
                           static_cast<half_t>(fminf(fmaxf(v.y, -65504.0f), 65504.0f)),
                           static_cast<half_t>(fminf(fmaxf(v.z, -65504.0f), 65504.0f)),
                           static_cast<half_t>(fminf(fmaxf(v.w, -65504.0f), 65504.0f))};
            *reinterpret_cast<uint2*>(Ch + o) = *reinterpret_cast<const uint2*>(h);
            s1 = (v.x + v.y) + (v.z + v.w);
            s2 = (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
          }
#pragma unroll
          for (int off = 1; off < 16; off <<= 1) {  // the 16 lanes that share the row
            s1 += __shfl_xor(s1, off);
            s2 += __shfl_xor(s2, off);
          }
          const int seg = (bn + wn * 64) >> 6;
          if ((lane & 15) == 0 && grow < M && seg < (N >> 6))
            reinterpret_cast<float2*>(Cl)[static_cast<int64_t>(grow) * (N >> 6) + seg] = make_float2(s1, s2);
        }
      }
    };
#pragma unroll
    for (int it = 0; it < 4; ++it) emit(it);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();  // the rows are read before the next piece overwrites the region
  }
  if (!has_next) break;
  par = (par + nk) & 1;
  tile = next;
  bm = nbm;
  bn = nbn;
  __syncthreads();  // every wave has left the staging buffer before the next tile's loads land in it
  }  // tiles
#undef VR_GLDS_STAGE
}

// The epilogue of the f16 kernels whose MFMAs take the WEIGHT fragment as their A operand (gemm_f16_pp_kernel,
// gemm_f16_mid_kernel), straight from the accumulators of a wave's 128-token x 64-feature tile at token row
// `row0`, feature `col0`: acc[i][j][r] of lane (t = lane & 15, g = lane >> 4) is token row 16 i + t, feature 4 g + r of
// weight fragment j — four CONSECUTIVE features of one token — and the W image was staged with its rows permuted so
// that fragments 2p and 2p + 1 hold features 32 p + 8 g + {0..3} and {4..7}: a lane owns 8 consecutive features per
// fragment pair = one 16-byte f16 store (or two 16-byte f32 stores), 64 contiguous bytes per token and instruction
// across the four lane groups. No transpose through LDS (it cost 128 ds_write_b32 + 32 ds_read_b128 per wave and
// tile, about half of the f16-output epilogue) and no LDS use at all.
// FULL: the wave's tile lies inside the matrix, nothing is predicated. This is not about the compares: a store under
// `if (ok)` sits in its own basic block, the waits the compiler places for the loads that are in flight across it
// (bias, residual rows) are then merged over both paths into vmcnt(0) — and on gfx950 vmcnt counts STORES too, so every
// store waited for the one before it: one 1 KiB store in flight per wave, the epilogue latency-bound. In straight-line
// code the counts are exact and the stores stay in flight.

constexpr int kWaveStatHalfs = 128 * 4;  // 128 float2 per wave (direct_epilogue's row statistics), in halfs
constexpr int kTileConstHalfs = (3 * 256 * 4 + 256 * 8) / 2;  // a tile's bias / gain / shift vectors and row statistics

// Output rows are written once and read by the NEXT kernel, long after they have left the caches: non-temporal stores
// (they do not push the weight panels and activation rows the other tiles still need out of L2). Measured +2.7 % on the
// GEMMs and +2 % on the attention kernel that runs between them (profiles/r02_gemm_experiments.md §5).
template <typename T>
__device__ __forceinline__ void out_store(T* p, const T& v) {
  __builtin_nontemporal_store(v, p);
}

template <int EPI, bool FULL, bool XPOSE = false>
__device__ __forceinline__ void direct_epilogue(f32x4 (&acc)[8][4], int row0, int col0, int lane,
                                                const float* __restrict__ bias, const float* __restrict__ R,
                                                float* __restrict__ C, half_t* __restrict__ Ch, half_t* __restrict__ Cl,
                                                int M, int N, float unscale, const float2* __restrict__ ln_stat,
                                                const float* __restrict__ ln_g, const float* __restrict__ ln_b,
                                                float2* wave_stat, const float* tile_const = nullptr, int trow0 = 0,
                                                int tcol0 = 0, half_t* xpose = nullptr) {
  asm volatile("" : "+v"(lane));  // (lane-derived offsets are made per tile, not carried through the K loop)
  const int tok = lane & 15, fg = lane >> 4;
  const int fbase = col0 + 8 * fg;  // + 32 p (+ 4 q): this lane's features
  // FULL tiles address everything as (wave-uniform pointer) + (one 32-bit lane offset): the uniform part — row
  // 16 pc of the tile, column col0 + 32 p2 — lives in scalar registers, where per-lane 64-bit addresses of eight pieces
  // did not fit next to the accumulators. (A chunk's matrices stay below 4 GiB: kMaxChunkTokens.)
  const uint32_t loff = static_cast<uint32_t>(tok * N + 8 * fg);
  auto upiece = [&](auto* base, int pc, int col) { return base + (static_cast<int64_t>(row0 + 16 * pc) * N + col); };
  // XPOSE (gemm_f16_pp_kernel; xpose = 4 KiB of the stage buffer the finished K loop has left free, per wave): the f16 rows go out
  // through a lane exchange. Straight from the accumulators a store instruction has lane (tok, fg) write 16 bytes of token
  // `tok`: the four lanes of every quad address four different rows, and the store path takes one request per (quad, 64-byte
  // segment) — 64 per instruction; a lone block needs 4.5 us to get its 128 KiB tile out, 256 blocks together no longer
  // (scripts/probe_store_burst.hip, profiles/r03_experiments.md §5: the burst is bound per CU by requests, not by HBM).
  // With the 16 x 4 block of 16-byte pieces transposed — lane L gets token L >> 2, piece L & 3 — a quad writes 64 contiguous
  // bytes: 16 requests per instruction, the same bytes in 1.35 us. The exchange is one ds_write_b128 + one ds_read_b128 in
  // a 1-KiB slot only this wave touches (LDS executes a wave's instructions in order: no barrier, no wait in between);
  // 64-byte rows with piece p of token t at p ^ (t >> 2): both sides conflict-free. The store of a piece is issued one piece
  // later, so its LDS round trip runs under the next piece's arithmetic.
  const int xw = tok * 32 + ((fg ^ (tok >> 2)) & 3) * 8;                          // write side, halfs
  const int xtr = lane >> 2, xtc = lane & 3;
  const int xr = xtr * 32 + ((xtc ^ (xtr >> 2)) & 3) * 8;                         // read side
  const uint32_t xloff = static_cast<uint32_t>(xtr * N + 8 * xtc);
  f16x8 xh = {};
  int xpend_pc = -1, xpend_p2 = 0;  // (compile-time after unrolling)
  auto xflush = [&]() {
    if (FULL) {
      out_store(reinterpret_cast<f16x8*>(upiece(Ch, xpend_pc, col0 + 32 * xpend_p2) + xloff), xh);
    } else {
      const int grow2 = row0 + 16 * xpend_pc + xtr, c2 = col0 + 32 * xpend_p2 + 8 * xtc;
      if (grow2 < M && c2 < N) out_store(reinterpret_cast<f16x8*>(Ch + static_cast<int64_t>(grow2) * N + c2), xh);
    }
  };
  constexpr bool kGlu = EPI == EPI_FOLD_SWIGLU || EPI == EPI_FOLD_GEGLU;
  constexpr bool kFold = EPI == EPI_FOLD_F16 || EPI == EPI_FOLD_GELU || kGlu;
  constexpr bool kStats = EPI == EPI_BIAS_RESIDUAL_LN_STATS || EPI == EPI_RLS_R32_O16 || EPI == EPI_RLS_R16_O16 ||
                          EPI == EPI_RLS_R16_O32;
  constexpr bool kR16 = EPI == EPI_RLS_R16_O16 || EPI == EPI_RLS_R16_O32;   // residual rows are f16
  constexpr bool kNoOut32 = EPI == EPI_RLS_R32_O16 || EPI == EPI_RLS_R16_O16;  // pre-LN rows go out as f16 only
  constexpr bool kResidLN = EPI == EPI_BIAS_RESIDUAL_LN || kStats;
  constexpr bool kResidual = EPI == EPI_BIAS_RESIDUAL || kResidLN;
  constexpr bool kGelu = EPI == EPI_BIAS_GELU || EPI == EPI_FOLD_GELU;
  constexpr bool kRelu = EPI == EPI_BIAS_RELU;
  constexpr bool kHalfOut = kGelu || kRelu || EPI == EPI_BIAS_F16 || EPI == EPI_FOLD_F16 || kNoOut32;
  // fragment pair p2 (features fbase + 32 p2 .. + 7) outside, the eight 16-token pieces inside: the column
  // vectors (bias, LayerNorm gain / shift or column sums) of one pair stay in registers, not those of all four
  // fragments (which, with the residual rows in flight, did not fit next to the 128 accumulators)
  // kFold without residual rows (the QKV and FFN-up projections): the (mean, 1/sigma) of the wave's 128 rows are the
  // only per-row loads — all eight pieces' worth up front, for both fragment pairs (fetched piece by piece, one piece
  // ahead, each of the 16 pieces waited ~1 us for 8 bytes)
  // tile_const (FULL tiles of gemm_f16_pp_kernel): the tile's 256 bias / gain / shift values and its 256 rows' statistics
  // were fetched into LDS while the main loop ran — [bias 256][gain or column sums 256][shift 256][float2 stat 256];
  // trow0 / tcol0 = this wave's first row / column inside the tile
  const bool in_lds = FULL && tile_const != nullptr;
  const float2* lds_stat = reinterpret_cast<const float2*>(tile_const + 768) + trow0;
  constexpr bool kStatUpfront = kFold;
  float2 st8[kStatUpfront ? 8 : 1] = {};
  if (kStatUpfront && !in_lds) {
#pragma unroll
    for (int pc = 0; pc < 8; ++pc)
      st8[pc] = FULL ? (ln_stat + (row0 + 16 * pc))[static_cast<uint32_t>(tok)] : ln_stat[min(row0 + 16 * pc + tok, M - 1)];
  }
#pragma unroll
  for (int p2 = 0; p2 < 2; ++p2) {
    const int c0 = fbase + 32 * p2;
    const bool col_ok = FULL || c0 < N;  // N % 8 == 0: a lane's eight features are in or out together
    const int cs = col_ok ? c0 : 0;
    float4 b4[2], lg4[2] = {}, lb4[2] = {};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const uint32_t lc = static_cast<uint32_t>(8 * fg + 4 * q);
      const int uc = col0 + 32 * p2;
      if (in_lds) {
        const float* tc = tile_const + tcol0 + 32 * p2 + lc;
        b4[q] = *reinterpret_cast<const float4*>(tc);
        if (kResidLN || kFold) lg4[q] = *reinterpret_cast<const float4*>(tc + 256);
        if (kResidLN) lb4[q] = *reinterpret_cast<const float4*>(tc + 512);
        continue;
      }
      b4[q] = FULL ? *reinterpret_cast<const float4*>(bias + uc + lc) : *reinterpret_cast<const float4*>(bias + cs + 4 * q);
      if (kResidLN || kFold)
        lg4[q] = FULL ? *reinterpret_cast<const float4*>(ln_g + uc + lc) : *reinterpret_cast<const float4*>(ln_g + cs + 4 * q);
      if (kResidLN)
        lb4[q] = FULL ? *reinterpret_cast<const float4*>(ln_b + uc + lc) : *reinterpret_cast<const float4*>(ln_b + cs + 4 * q);
    }
    // residual rows (and row statistics) of a piece are requested TWO pieces ahead (one piece of arithmetic is ~600 cycles,
    // a global load 1-2 thousand: one ahead left every piece waiting)
    // (EPI_RLS_R16_O16 under gemm_f16_pp_kernel comes here for edge tiles only — whole tiles go to rls16_tile_epilogue — and
    // one piece ahead keeps this path inside the kernel's register budget)
    constexpr int kAhead = (!FULL && EPI == EPI_RLS_R16_O16) ? 1 : 2;
    float4 r4[kAhead + 1][2] = {};
    float2 st2[kAhead + 1] = {};
    auto fetch_residual = [&](int pc, float4 (&r)[2], float2& st) {
      if (FULL) {
        if (kResidual && kR16) {
          r[0] = *reinterpret_cast<const float4*>(upiece(reinterpret_cast<const half_t*>(R), pc, col0 + 32 * p2) + loff);
        } else if (kResidual) {
          r[0] = *reinterpret_cast<const float4*>(upiece(R, pc, col0 + 32 * p2) + loff);
          r[1] = *reinterpret_cast<const float4*>(upiece(R, pc, col0 + 32 * p2 + 4) + loff);
        }
        if (kResidLN || kFold) st = in_lds ? lds_stat[16 * pc + tok] : (ln_stat + (row0 + 16 * pc))[static_cast<uint32_t>(tok)];
        return;
      }
      const int64_t rr = min(row0 + 16 * pc + tok, M - 1);
      if (kResidual && kR16) {  // eight f16 residual values: carried in r[0]'s 16 bytes
        r[0] = *reinterpret_cast<const float4*>(reinterpret_cast<const half_t*>(R) + rr * N + cs);
      } else if (kResidual) {
        r[0] = *reinterpret_cast<const float4*>(R + rr * N + cs);
        r[1] = *reinterpret_cast<const float4*>(R + rr * N + cs + 4);
      }
      if (kResidLN || kFold) st = ln_stat[rr];
    };
    if ((kResidual || kFold) && !kStatUpfront) {
#pragma unroll
      for (int pc = 0; pc < kAhead; ++pc) fetch_residual(pc, r4[pc], st2[pc]);
    }
    // (tile constants in LDS: a piece's row statistics are read one piece ahead — every piece is a basic block of its own,
    // so a read at the point of use cannot be moved up by the compiler and each piece began with an exposed LDS round trip)
    float2 st_ahead = (kStatUpfront && in_lds) ? lds_stat[tok] : float2{};
#pragma unroll
    for (int pc = 0; pc < 8; ++pc) {  // piece pc = token rows 16 pc .. 16 pc + 15 of the wave's 128
      const int grow = row0 + 16 * pc + tok;
      if ((kResidual || kFold) && !kStatUpfront && pc + kAhead < 8)
        fetch_residual(pc + kAhead, r4[(pc + kAhead) % (kAhead + 1)], st2[(pc + kAhead) % (kAhead + 1)]);
      const bool ok = FULL || (grow < M && col_ok);
      const float2 st_lds = st_ahead;
      if (kStatUpfront && in_lds && pc + 1 < 8) {
        st_ahead = lds_stat[16 * (pc + 1) + tok];
        __builtin_amdgcn_sched_barrier(0);  // (left alone, the scheduler sinks the read to the end of the piece)
      }
      const float2 st = kStatUpfront ? (in_lds ? st_lds : st8[pc]) : st2[pc % (kAhead + 1)];
      float v[2][4];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const float bb[4] = {b4[q].x, b4[q].y, b4[q].z, b4[q].w};
        const float gg[4] = {lg4[q].x, lg4[q].y, lg4[q].z, lg4[q].w};
        const float lb[4] = {lb4[q].x, lb4[q].y, lb4[q].z, lb4[q].w};
        const float4 rq = r4[pc % (kAhead + 1)][kR16 ? 0 : q];
        float rr4[4] = {rq.x, rq.y, rq.z, rq.w};
        if (kR16) {
          const f16x8 rh = *reinterpret_cast<const f16x8*>(&rq);
#pragma unroll
          for (int r = 0; r < 4; ++r) rr4[r] = static_cast<float>(rh[4 * q + r]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float x = acc[pc][2 * p2 + q][r];
          if (kFold)  // inv (acc unscale - mean colsum) + c
            x = fmaf(fmaf(x, unscale, -(st.x * gg[r])), st.y, bb[r]);
          else
            x = x * unscale + bb[r];
          if (EPI == EPI_BIAS_RESIDUAL) x += rr4[r];
          if (kResidLN) x += ln_apply(rr4[r], st.x, st.y, gg[r], lb[r]);  // residual = LayerNorm(R row)
          v[q][r] = x;
        }
      }
      if (kGelu) {
        f32x2 g[4] = {f32x2{v[0][0], v[0][1]}, f32x2{v[0][2], v[0][3]}, f32x2{v[1][0], v[1][1]}, f32x2{v[1][2], v[1][3]}};
        gelu_poly2x4(g);
#pragma unroll
        for (int q = 0; q < 2; ++q)
          v[q][0] = g[2 * q].x, v[q][1] = g[2 * q].y, v[q][2] = g[2 * q + 1].x, v[q][3] = g[2 * q + 1].y;
      }
      if (kRelu) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int r = 0; r < 4; ++r) v[q][r] = fmaxf(v[q][r], 0.0f);
      }
      if (kGlu) {
        // the lane's eight columns are four (gate, up) pairs of the interleaved matrix: four f16 outputs at column c0 / 2
        // of a row of N / 2, one 8-byte store (the four lanes of a token write 32 contiguous bytes)
        constexpr int kFfn = EPI == EPI_FOLD_SWIGLU ? VR_FFN_SWIGLU : VR_FFN_GEGLU;
        half_t h4[4];
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int r = 0; r < 2; ++r)
            h4[2 * q + r] = static_cast<half_t>(fminf(fmaxf(glu_act<false>(v[q][2 * r], kFfn) * v[q][2 * r + 1], -65504.0f), 65504.0f));
        const int n2 = N >> 1;
        if (FULL)
          *reinterpret_cast<uint2*>((Ch + (static_cast<int64_t>(row0 + 16 * pc) * n2 + ((col0 + 32 * p2) >> 1))) +
                                    static_cast<uint32_t>(tok * n2 + 4 * fg)) = *reinterpret_cast<const uint2*>(h4);
        else if (ok)
          *reinterpret_cast<uint2*>(Ch + static_cast<int64_t>(grow) * n2 + (c0 >> 1)) = *reinterpret_cast<const uint2*>(h4);
      }
      if (kHalfOut || kStats) {  // f16 row: 8 consecutive features, one 16-byte store
        f16x8 h;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          h[r] = static_cast<half_t>(fminf(fmaxf(v[0][r], -65504.0f), 65504.0f));
          h[4 + r] = static_cast<half_t>(fminf(fmaxf(v[1][r], -65504.0f), 65504.0f));
        }
        if (XPOSE) {
          half_t* slot = xpose + ((8 * p2 + pc) & 3) * 512;
          *reinterpret_cast<f16x8*>(slot + xw) = h;
          asm volatile("" ::: "memory");
          if (xpend_pc >= 0) xflush();
          xh = *reinterpret_cast<const f16x8*>(slot + xr);
          asm volatile("" ::: "memory");
          xpend_pc = pc, xpend_p2 = p2;
        } else if (FULL)
          out_store(reinterpret_cast<f16x8*>(upiece(Ch, pc, col0 + 32 * p2) + loff), h);
        else if (ok)
          out_store(reinterpret_cast<f16x8*>(Ch + static_cast<int64_t>(grow) * N + c0), h);
      }
      if (kGlu) {
      } else if (!kHalfOut && FULL) {  // f32 row
        *reinterpret_cast<float4*>(upiece(C, pc, col0 + 32 * p2) + loff) = make_float4(v[0][0], v[0][1], v[0][2], v[0][3]);
        *reinterpret_cast<float4*>(upiece(C, pc, col0 + 32 * p2 + 4) + loff) = make_float4(v[1][0], v[1][1], v[1][2], v[1][3]);
      } else if (!kHalfOut && ok) {
        *reinterpret_cast<float4*>(C + static_cast<int64_t>(grow) * N + c0) = make_float4(v[0][0], v[0][1], v[0][2], v[0][3]);
        *reinterpret_cast<float4*>(C + static_cast<int64_t>(grow) * N + c0 + 4) = make_float4(v[1][0], v[1][1], v[1][2], v[1][3]);
      }
      if (kStats) {
        // this wave's 64 columns of every pre-LayerNorm row contribute a (sum, sum of squares) to the row's statistics:
        // 8 values per lane and fragment pair, the other 24 of the pair in the three other lane groups. The first
        // pair's sums wait in `wave_stat` (128 float2 of LDS that only this wave touches) for the second's — sixteen
        // registers per lane less than carrying them, which the branch-free form of this code did not have.
        float a1 = 0.0f, a2 = 0.0f;
        if (col_ok) {
          a1 = ((v[0][0] + v[0][1]) + (v[0][2] + v[0][3])) + ((v[1][0] + v[1][1]) + (v[1][2] + v[1][3]));
          a2 = ((v[0][0] * v[0][0] + v[0][1] * v[0][1]) + (v[0][2] * v[0][2] + v[0][3] * v[0][3])) +
               ((v[1][0] * v[1][0] + v[1][1] * v[1][1]) + (v[1][2] * v[1][2] + v[1][3] * v[1][3]));
        }
        a1 += __shfl_xor(a1, 16);
        a2 += __shfl_xor(a2, 16);
        a1 += __shfl_xor(a1, 32);
        a2 += __shfl_xor(a2, 32);
        if (p2 == 0) {
          if (fg == 0) wave_stat[16 * pc + tok] = make_float2(a1, a2);
        } else {
          const float2 first = wave_stat[16 * pc + tok];
          a1 += first.x;
          a2 += first.y;
          const int seg = col0 >> 6;
          if (FULL) {
            if (fg == 0)
              (reinterpret_cast<float2*>(Cl) + (static_cast<int64_t>(row0 + 16 * pc) * (N >> 6) + seg))[static_cast<uint32_t>(tok * (N >> 6))] =
                  make_float2(a1, a2);
          } else if (fg == 0 && grow < M && seg < (N >> 6)) {
            reinterpret_cast<float2*>(Cl)[static_cast<int64_t>(grow) * (N >> 6) + seg] = make_float2(a1, a2);
          }
        }
      }
      // Every piece stays a basic block of its own: in one long block the SLP vectoriser pairs up the arithmetic of
      // DIFFERENT pieces (v_pk_* over values of two pieces), all eight pieces are then in flight at once and a
      // thousand registers spill. The never-taken branch below (M is positive; the compiler cannot know) ends the
      // block without putting anything that counts in vmcnt on a side path, so the wait counts stay exact.
      if (FULL && M < 0) asm volatile("s_nop 0");
    }
  }
  if (XPOSE && (kHalfOut || kStats) && xpend_pc >= 0) xflush();
}


// Whole tiles of the f16-output projections without residual rows (QKV, FFN-up: four fifths of the bytes the GEMMs write),
// gemm_f16_pp_kernel only. Same arithmetic per element as direct_epilogue (same bits); what differs is the ORDER of things.
// In-kernel time stamps (profiles/r03_experiments.md) showed direct_epilogue's whole-tile path at 9-10k
// cycles per tile for the QKV variant with its arithmetic switched off as well as on, against 5.4k for the arithmetic
// alone: every 16-token piece ended in an LDS round trip (lane exchange in front of the store, see direct_epilogue) and
// began with one (row statistics) that nothing covered — one basic block per piece, lgkmcnt(0) at every block entry.
// Here four pieces form a batch: their statistics are read together, their f16 rows are written to four LDS slots as they
// are computed (no wait), then read back transposed together and stored — two exposed LDS round trips per batch of four
// instead of eight, and the next batch's statistics are requested before the read-back.
template <int EPI>
__device__ __forceinline__ void f16_tile_epilogue(f32x4 (&acc)[8][4], int row0, int col0, int lane, half_t* __restrict__ Ch,
                                                  int M, int N, float unscale, const float* tile_const, int trow0, int tcol0,
                                                  half_t* xpose) {
  constexpr bool kFold = EPI == EPI_FOLD_F16 || EPI == EPI_FOLD_GELU;
  constexpr bool kGelu = EPI == EPI_BIAS_GELU || EPI == EPI_FOLD_GELU;
  asm volatile("" : "+v"(lane));  // (the lane-derived offsets below are made per tile, not carried through the K loop)
  const int tok = lane & 15, fg = lane >> 4;
  const float2* lds_stat = reinterpret_cast<const float2*>(tile_const + 768) + trow0;
  const int xw = tok * 32 + ((fg ^ (tok >> 2)) & 3) * 8;  // lane exchange: see direct_epilogue (XPOSE)
  const int xtr = lane >> 2, xtc = lane & 3;
  const int xr = xtr * 32 + ((xtc ^ (xtr >> 2)) & 3) * 8;
  const uint32_t xloff = static_cast<uint32_t>(xtr * N + 8 * xtc);
  float2 st[4] = {};
  if (kFold) {
#pragma unroll
    for (int i = 0; i < 4; ++i) st[i] = lds_stat[16 * i + tok];
  }
#pragma unroll
  for (int p2 = 0; p2 < 2; ++p2) {
    float4 b4[2], lg4[2] = {};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const float* tc = tile_const + tcol0 + 32 * p2 + 8 * fg + 4 * q;
      b4[q] = *reinterpret_cast<const float4*>(tc);
      if (kFold) lg4[q] = *reinterpret_cast<const float4*>(tc + 256);
    }
#pragma unroll
    for (int hb = 0; hb < 2; ++hb) {
      float2 stc[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) stc[i] = st[i];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int pc = 4 * hb + i;
        // pairs of features on the packed-f32 instructions (element for element the operations of direct_epilogue)
        f32x2 g[4];  // pair 2 q + e: features 4 q + 2 e, + 1 of the lane's eight
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const f32x2 x = {acc[pc][2 * p2 + q][2 * e], acc[pc][2 * p2 + q][2 * e + 1]};
            const f32x2 bb = e == 0 ? f32x2{b4[q].x, b4[q].y} : f32x2{b4[q].z, b4[q].w};
            if (kFold) {
              const f32x2 gg = e == 0 ? f32x2{lg4[q].x, lg4[q].y} : f32x2{lg4[q].z, lg4[q].w};
              const f32x2 mean = {stc[i].x, stc[i].x}, inv = {stc[i].y, stc[i].y}, un = {unscale, unscale};
              g[2 * q + e] = __builtin_elementwise_fma(__builtin_elementwise_fma(x, un, -(mean * gg)), inv, bb);
            } else {
              g[2 * q + e] = x * unscale + bb;
            }
          }
        if (kGelu) gelu_poly2x4(g);
        if (EPI == EPI_BIAS_RELU) {
#pragma unroll
          for (int c = 0; c < 4; ++c) g[c] = f32x2{fmaxf(g[c].x, 0.0f), fmaxf(g[c].y, 0.0f)};
        }
        f16x8 h;
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            h[4 * q + 2 * e] = static_cast<half_t>(g[2 * q + e].x);  // (saturating: MODE.FP16_OVFL, set by the kernel)
            h[4 * q + 2 * e + 1] = static_cast<half_t>(g[2 * q + e].y);
          }
        *reinterpret_cast<f16x8*>(xpose + i * 512 + xw) = h;
        // (one basic block per piece, as in direct_epilogue: in one long block the SLP vectoriser pairs arithmetic of
        // different pieces and a thousand registers spill)
        if (M < 0) asm volatile("s_nop 0");
      }
      asm volatile("" ::: "memory");
      // the next batch's statistics are requested before this one's rows are read back
      const int nb = 2 * p2 + hb + 1;  // batches 0..3: (p2, hb); the statistics depend on hb only
      if (kFold && nb < 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) st[i] = lds_stat[16 * (4 * (nb & 1) + i) + tok];
      }
      f16x8 xh[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) xh[i] = *reinterpret_cast<const f16x8*>(xpose + i * 512 + xr);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        out_store(reinterpret_cast<f16x8*>(Ch + (static_cast<int64_t>(row0 + 16 * (4 * hb + i)) * N + col0 + 32 * p2) + xloff), xh[i]);
      asm volatile("" ::: "memory");
    }
  }
}

// Four values summed over the four 16-lane rows of a wave at once: afterwards the lanes of row r hold the total of value r,
// ((r0 + r1) + (r2 + r3)) — the bits of a += __shfl_xor(a, 16); a += __shfl_xor(a, 32) — in three lane swaps and three adds
// (v_permlane16_swap exchanges the odd rows of its first operand with the even rows of its second, v_permlane32_swap the
// upper half of the first with the lower half of the second: each swap + add halves two values at a time), on the vector
// ALU instead of eight ds_bpermute round trips through the LDS queue.
__device__ __forceinline__ float rows_sum4x4(float v0, float v1, float v2, float v3) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v0), __float_as_uint(v1), false, false);
  const unsigned a0 = a[0], a1 = a[1];
  const float s01 = __uint_as_float(a0) + __uint_as_float(a1);  // rows: v0 (r0 + r1), v1 (r0 + r1), v0 (r2 + r3), v1 (r2 + r3)
  const auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(v2), __float_as_uint(v3), false, false);
  const unsigned b0 = b[0], b1 = b[1];
  const float s23 = __uint_as_float(b0) + __uint_as_float(b1);
  const auto c = __builtin_amdgcn_permlane32_swap(__float_as_uint(s01), __float_as_uint(s23), false, false);
  const unsigned c0 = c[0], c1 = c[1];
  return __uint_as_float(c0) + __uint_as_float(c1);  // row r: value r, (r0 + r1) + (r2 + r3)
}

// Whole tiles of the two projections that add the residual stream (attention output, FFN-down; EPI_RLS_R16_O16: f16
// residual rows in, LayerNorm of them applied here, f16 pre-LayerNorm rows and per-row partial statistics out),
// gemm_f16_pp_kernel only. Same arithmetic per element and the same order of every sum as direct_epilogue (same bits).
// In the stamps direct_epilogue's predicated path took 25-27k cycles per tile for this variant — as long as the whole K loop
// of the attention-output projection — for ~6k cycles of arithmetic: sixteen 16-byte loads per wave whose quads address four
// different rows (64 requests per instruction, like the stores the lane exchange fixed), each waited for with the stores
// of the piece before it in the same queue, bias / gain / shift / row statistics from global memory, two ds_bpermute
// round trips per piece for the statistics. Here
//   * the residual rows arrive by direct-to-LDS loads — no registers, quad-contiguous requests (lane L: token L >> 2, piece
//     (L & 3) ^ f(token) of the 64-byte half row: the source-side form of the exchange layout), a batch of four pieces
//     AHEAD of the batch being computed, waited for with a counted vmcnt that leaves the previous batch's stores in flight;
//   * a piece reads its residual values out of its slot, and writes its f16 result rows into the same slot (LDS executes a
//     wave's instructions in order); four slots are read back transposed and stored, as in f16_tile_epilogue;
//   * the tile's constants and row statistics come from the LDS copy the K loop fetched; the sums over the four lane groups
//     are vector-ALU lane swaps (rows_sum4); the first fragment pair's sums wait in registers the dying accumulators free.
// xpose: 8 KiB per wave (two batches of four 1-KiB slots) in the stage buffer the K loop has left.
__device__ __forceinline__ void rls16_tile_epilogue(f32x4 (&acc)[8][4], int row0, int col0, int lane, const half_t* __restrict__ R16,
                                                    half_t* __restrict__ Ch, half_t* __restrict__ Cl, int M, int N, float unscale,
                                                    const float* tile_const, int trow0, int tcol0, half_t* xpose, half_t* xspare) {
  asm volatile("" : "+v"(lane));
  const int tok = lane & 15, fg = lane >> 4;
  const float2* lds_stat = reinterpret_cast<const float2*>(tile_const + 768) + trow0;
  const int xw = tok * 32 + ((fg ^ (tok >> 2)) & 3) * 8;
  const int xtr = lane >> 2, xtc = lane & 3;
  const int xr = xtr * 32 + ((xtc ^ (xtr >> 2)) & 3) * 8;
  const uint32_t xloff = static_cast<uint32_t>(xtr * N + 8 * xtc);
  // source of the direct-to-LDS loads: token xtr of the piece, 16-byte piece xtc ^ f(xtr) (it lands at position xtc)
  const uint32_t rloff = static_cast<uint32_t>(xtr * N + 8 * ((xtc ^ (xtr >> 2)) & 3));
  // Groups of two pieces, g = 0..7: fragment pair p2 = g >> 2, pieces 2 (g & 3), + 1. Five slot pairs (four in the stage
  // buffer the K loop has left, one in the LDS behind the tile constants) carry the group being computed and the four
  // behind it: a group's residual rows are requested FOUR groups (eight pieces of arithmetic) before they are read — with
  // batches of four pieces and one batch of lead every batch waited for memory (stamps: 17-19k cycles per tile against 9k of
  // vector instructions).
  auto pair_of_group = [&](int g) { return (g % 5) < 4 ? xpose + (g % 5) * 1024 : xspare; };
  auto request = [&](int g) {
    half_t* buf = pair_of_group(g);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      glds16(R16 + (static_cast<int64_t>(row0 + 16 * (2 * (g & 3) + i)) * N + col0 + 32 * (g >> 2)) + rloff, buf + i * 512);
  };
  float sk[4];  // the first fragment pair's sums, one register per group: lane row fg holds (a1, a2) of the group's first piece (fg = 0, 1) and of its second (fg = 2, 3)
#pragma unroll
  for (int g = 0; g < 5; ++g) request(g);
  float4 b4[2], lg4[2], lb4[2];
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    const int p2 = g >> 2;
    half_t* buf = pair_of_group(g);
    asm volatile("" ::: "memory");
    // operations younger than this group's two loads (the loads of the groups behind it, the stores of the groups before
    // it): what the counted wait leaves in flight
    // (a group of the first fragment pair issues two stores, one of the second three — its statistics; groups 0-2 are followed
    // by the two loads of the group five behind)
    if (g == 0) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");        // D1-D4
    else if (g == 1) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");  // D2-D4, S0, D5
    else if (g == 2) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");  // D3, D4, S0, D5, S1, D6
    else if (g <= 4) asm volatile("s_waitcnt vmcnt(14)" ::: "memory");  // g = 3: D4, (S, D) x 3; g = 4: (S, D) x 3, S3
    else if (g == 5) asm volatile("s_waitcnt vmcnt(13)" ::: "memory");  // S1, D6, S2, D7, S3, S4 (3)
    else if (g == 6) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");  // S2, D7, S3, S4 (3), S5 (3)
    else asm volatile("s_waitcnt vmcnt(11)" ::: "memory");              // S3, S4, S5, S6 (3 each but S3)
    if ((g & 3) == 0) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const float* tc = tile_const + tcol0 + 32 * p2 + 8 * fg + 4 * q;
        b4[q] = *reinterpret_cast<const float4*>(tc);
        lg4[q] = *reinterpret_cast<const float4*>(tc + 256);
        lb4[q] = *reinterpret_cast<const float4*>(tc + 512);
      }
    }
    float2 stc[2];
    f16x8 rh2[2];  // the group's residual values and row statistics, read together
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      stc[i] = lds_stat[16 * (2 * (g & 3) + i) + tok];
      rh2[i] = *reinterpret_cast<const f16x8*>(buf + i * 512 + xw);
    }
    asm volatile("" ::: "memory");
    float pa1[2], pa2[2];  // the two pieces' sums over this lane's eight features
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pc = 2 * (g & 3) + i;
      const f16x8 rh = rh2[i];
      // pairs of features on the packed-f32 instructions; element for element the operations (and their order) of
      // direct_epilogue: x = acc * unscale + bias; x += ((r - mean) * inv) * gain + shift
      // (stage by stage across the four pairs: a dependent chain of packed instructions issues every other slot)
      f32x2 g2[4], t[4];  // pair k = 2 q + e: features 4 q + 2 e, + 1 of the lane's eight
      const f32x2 mean = {stc[i].x, stc[i].x}, inv = {stc[i].y, stc[i].y};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        g2[k] = f32x2{acc[pc][2 * p2 + (k >> 1)][2 * (k & 1)], acc[pc][2 * p2 + (k >> 1)][2 * (k & 1) + 1]} * unscale;
        t[k] = f32x2{static_cast<float>(rh[4 * (k >> 1) + 2 * (k & 1)]), static_cast<float>(rh[4 * (k >> 1) + 2 * (k & 1) + 1])} - mean;
      }
      auto pair_of = [](const float4& c, int e) { return e == 0 ? f32x2{c.x, c.y} : f32x2{c.z, c.w}; };
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        g2[k] = g2[k] + pair_of(b4[k >> 1], k & 1);
        t[k] = t[k] * inv;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] = t[k] * pair_of(lg4[k >> 1], k & 1);
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] = t[k] + pair_of(lb4[k >> 1], k & 1);
#pragma unroll
      for (int k = 0; k < 4; ++k) g2[k] = g2[k] + t[k];
      f16x8 h;
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          h[4 * q + 2 * e] = static_cast<half_t>(g2[2 * q + e].x);  // (saturating: MODE.FP16_OVFL, set by the kernel)
          h[4 * q + 2 * e + 1] = static_cast<half_t>(g2[2 * q + e].y);
        }
      float v[2][4];
#pragma unroll
      for (int q = 0; q < 2; ++q) v[q][0] = g2[2 * q].x, v[q][1] = g2[2 * q].y, v[q][2] = g2[2 * q + 1].x, v[q][3] = g2[2 * q + 1].y;
      *reinterpret_cast<f16x8*>(buf + i * 512 + xw) = h;  // (behind the read of the same 16 bytes)
      pa1[i] = ((v[0][0] + v[0][1]) + (v[0][2] + v[0][3])) + ((v[1][0] + v[1][1]) + (v[1][2] + v[1][3]));
      pa2[i] = ((v[0][0] * v[0][0] + v[0][1] * v[0][1]) + (v[0][2] * v[0][2] + v[0][3] * v[0][3])) +
               ((v[1][0] * v[1][0] + v[1][1] * v[1][1]) + (v[1][2] * v[1][2] + v[1][3] * v[1][3]));
      if (M < 0) asm volatile("s_nop 0");  // (one basic block per piece: see direct_epilogue)
    }
    {
      // sums over the four lane groups, the group's four values at once: lane row 0 / 1 ends up with (sum, sum of squares)
      // of the first piece's token `tok`, row 2 / 3 with the second piece's
      float tot = rows_sum4x4(pa1[0], pa2[0], pa1[1], pa2[1]);
      if (p2 == 0) {
        sk[g & 3] = tot;
      } else {
        tot += sk[g & 3];
        const int pc = 2 * (g & 3) + (fg >> 1);
        (reinterpret_cast<float*>(Cl) + 2 * (static_cast<int64_t>(row0 + 16 * pc) * (N >> 6) + (col0 >> 6)))[static_cast<uint32_t>(2 * tok * (N >> 6) + (fg & 1))] = tot;
      }
    }
    asm volatile("" ::: "memory");
    f16x8 xh[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) xh[i] = *reinterpret_cast<const f16x8*>(buf + i * 512 + xr);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      out_store(reinterpret_cast<f16x8*>(Ch + (static_cast<int64_t>(row0 + 16 * (2 * (g & 3) + i)) * N + col0 + 32 * p2) + xloff), xh[i]);
    asm volatile("" ::: "memory");
    if (g + 5 < 8) request(g + 5);  // (into the slot pair this group has just read back)
  }
}

// ---- the 256x256 f16 product with a ping-pong main loop ----------------------------------------------
//
// Same tile, LDS image, swizzle, persistent tile walk and epilogues as gemm_f16x3_256_kernel<EPI, 1>; what
// changes is WHEN things happen inside a 64-deep K-tile. There every wave read fragments, multiplied and
// waited for the next K-tile's loads in step with its SIMD partner (one barrier and one vmcnt(0) per K-tile):
// while both read LDS or waited, the matrix pipe of the SIMD idled (64 % MFMA issue in the main loop). Here
//   * a K-tile is four PHASES, one 64x32 quadrant of the wave's 128x64 tile each (16 MFMAs over both 32-deep
//     steps): a READ segment (the phase's fragment reads + two direct-to-LDS loads of the next K-tile) and
//     an MFMA segment, each closed by a raw s_barrier;
//   * waves 4-7 (the second wave of every SIMD) run one segment behind waves 0-3, so at any time one wave of
//     a SIMD multiplies while its partner reads and loads: the partner's LDS latency, load issue and barrier
//     wait sit under 256 cycles of MFMAs instead of beside them;
//   * the next K-tile arrives in four half-tiles issued in the order they are needed (rows of quadrant
//     rows 0-63 of A, quadrant columns 0-31 of W, columns 32-63, rows 64-127), each waited for with a COUNTED
//     vmcnt two to three phases after its issue (never vmcnt(0) in the loop) — two half-tiles stay in flight
//     across every barrier. A wait sits in the READ segment of the phase BEFORE the one that reads the data, so
//     that every wave's wait and one more barrier lie between a load and any wave's read of it.
//   * the MFMAs take the WEIGHT fragment as their A operand, which leaves every lane with four consecutive
//     output features of one token: the epilogue stores straight from the accumulators (no LDS transpose).
// Accumulation order per output element is unchanged (k ascending), so the result is bit-identical to
// gemm_f16x3_256_kernel<EPI, 1>. Needs an even number of K-tiles (K % 128 == 0) and N % 8 == 0: every supported width.
template <int EPI>
__global__ __launch_bounds__(512) void gemm_f16_pp_kernel(
    const half_t* __restrict__ Ah, const half_t* __restrict__ Wh, const float* __restrict__ bias,
    const float* __restrict__ R, float* __restrict__ C, half_t* __restrict__ Ch, half_t* __restrict__ Cl, int M,
    int N, int K, float unscale, const float2* __restrict__ ln_stat, const float* __restrict__ ln_g,
    const float* __restrict__ ln_b, int stagger_sleeps, int group_m) {
  __shared__ half_t lds[2 * kStageHalfs + 8 * kWaveStatHalfs + kTileConstHalfs + 8 * 1024];  // the only LDS object (see gemm_f16x3_256_kernel)
  const int tiles_n = (N + GBN - 1) / GBN;
  const int tiles_m = (M + GBM - 1) / GBM;
  const int total = tiles_m * tiles_n;
  const int G = gridDim.x;
  const int local = (G % 8 == 0) ? (static_cast<int>(blockIdx.x) % 8) * (G / 8) + static_cast<int>(blockIdx.x) / 8
                                 : static_cast<int>(blockIdx.x);
  auto coords = [&](int t, int& bm_, int& bn_) {
    const int per_group = group_m * tiles_n;
    const int group = t / per_group;
    const int within = t - group * per_group;
    const int gm = min(group_m, tiles_m - group * group_m);
    bm_ = (group * group_m + within % gm) * GBM;
    bn_ = (within / gm) * GBN;
  };
  int tile = local;
  if (tile >= total) return;  // block-uniform
  // MODE.FP16_OVFL: f32 -> f16 conversions saturate at +-65504 instead of overflowing to infinity — for every finite input the
  // bits of clamp-then-convert (scripts/probe_fp16_ovfl.hip: 100,000 values, none differs; an infinite input stays infinite,
  // where the clamp makes it 65504), without the v_med3_f32 per element the whole-tile epilogues spent on the clamp
  asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 23, 1), 1");
  int bm, bn;
  coords(tile, bm, bn);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  float2* wave_stat = reinterpret_cast<float2*>(lds + 2 * kStageHalfs + wave * kWaveStatHalfs);
  // the epilogue's lane exchange (direct_epilogue: xpose) uses stage buffer 1: the K loop ends on it (nk is even), the next
  // tile's K-tile 0 is in buffer 0, and nothing loads into buffer 1 before the barrier that follows the epilogue
  half_t* xpose = lds + kStageHalfs + wave * 4096;  // 8 KiB per wave
  half_t* xspare = lds + 2 * kStageHalfs + 8 * kWaveStatHalfs + kTileConstHalfs + wave * 1024;  // + 2 KiB per wave (rls16_tile_epilogue)
  // the tile's epilogue constants (direct_epilogue: tile_const), fetched by waves 0-4 at the start of the tile's K loop —
  // one direct-to-LDS load each — so that the epilogue starts on LDS reads instead of three rounds of global-load latency
  half_t* tile_const_h = lds + 2 * kStageHalfs + 8 * kWaveStatHalfs;
  constexpr bool kUsesGain = EPI == EPI_FOLD_F16 || EPI == EPI_FOLD_GELU || EPI == EPI_FOLD_SWIGLU || EPI == EPI_FOLD_GEGLU ||
                             EPI == EPI_BIAS_RESIDUAL_LN ||
                             EPI == EPI_BIAS_RESIDUAL_LN_STATS || EPI == EPI_RLS_R32_O16 || EPI == EPI_RLS_R16_O16 ||
                             EPI == EPI_RLS_R16_O32;
  constexpr bool kUsesShift = kUsesGain && EPI != EPI_FOLD_F16 && EPI != EPI_FOLD_GELU && EPI != EPI_FOLD_SWIGLU &&
                              EPI != EPI_FOLD_GEGLU;
  // (the branch-free form of the epilogues that also read residual rows needs ~30 registers more than this kernel
  // has left beside its staging state; those keep the predicated form and their global loads)
  constexpr bool kBranchFree = EPI != EPI_BIAS_RESIDUAL_LN && EPI != EPI_BIAS_RESIDUAL_LN_STATS && EPI != EPI_RLS_R32_O16 &&
                               EPI != EPI_RLS_R16_O16 && EPI != EPI_RLS_R16_O32;
  constexpr bool kRlsTile = EPI == EPI_RLS_R16_O16;  // whole tiles: rls16_tile_epilogue
  auto issue_tile_consts = [&](int bm_, int bn_) {
    // edge tiles read them from global memory (predicated epilogue) — except a last column tile that ends on a 64-column
    // boundary (N = 384, 1152: the waves behind the edge have nothing to store, the others run the whole-tile epilogue)
    if (!(kBranchFree || kRlsTile) || bm_ + GBM > M || (bn_ + GBN > N && N % 64 != 0)) return;
    // (the lane offset is made opaque per call: left visible, the compiler keeps five per-lane 64-bit source addresses alive
    // across the whole kernel — ten registers the epilogue does not have)
    int l8 = lane * 8;  // 16 bytes per lane, in halfs
    asm volatile("" : "+v"(l8));
    const int c8 = min(2 * bn_ + l8, 2 * N - 8);  // (columns behind the edge re-read the last four: never used)
    if (wave == 0) glds16(reinterpret_cast<const half_t*>(bias) + c8, tile_const_h);
    if (wave == 1 && kUsesGain) glds16(reinterpret_cast<const half_t*>(ln_g) + c8, tile_const_h + 512);
    if (wave == 2 && kUsesShift) glds16(reinterpret_cast<const half_t*>(ln_b) + c8, tile_const_h + 1024);
    if (wave == 3 && kUsesGain) glds16(reinterpret_cast<const half_t*>(ln_stat + bm_) + l8, tile_const_h + 1536);
    if (wave == 4 && kUsesGain) glds16(reinterpret_cast<const half_t*>(ln_stat + bm_ + 128) + l8, tile_const_h + 2048);
  };
  // Phase diversity: every block's tile takes the same time, so without this all 256 CUs reach their
  // epilogues together — a burst of stores at the chip's store bandwidth with every matrix pipe idle,
  // followed by a main loop with the store path idle. Block `local` (of G) starts local / G of
  // `stagger_sleeps` x 64 cycles late, which spreads the epilogues over the tile period. The blocks with
  // the highest index — the ones that sleep longest — are also the ones that get one tile FEWER when the
  // tile count is not a multiple of G, so most of the delay falls into the last, partly filled round.
  for (int d = (static_cast<int64_t>(stagger_sleeps) * local) / G; d > 0; d -= 16) __builtin_amdgcn_s_sleep(16);

  // staging: one direct-to-LDS load moves 8 rows x 128 B; lane -> row (lane >> 3) of the 8, LDS chunk
  // (lane & 7), source chunk (lane & 7) ^ ((row >> 1) & 7). Wave w stages A rows 8w + {0, 128} (the rows
  // of quadrant rows 0-63 of both wave rows: "A lo"), 8w + {64, 192} ("A hi"), and W rows
  // 64 (w >> 2) + 8 (w & 3) + {0, 128} (quadrant columns 0-31 of all four wave columns: "W lo"), + {32, 160}
  // ("W hi"): every wave issues two loads per half-tile, so one vmcnt count serves all waves.
  // (the per-lane staging and fragment offsets are derived again after every epilogue — derive_lane_state — so that they
  // do not hold registers while the epilogue runs: it is the kernel's register peak)
  int schunk, ra, rwp, pa, pw, fk0, fk1;
  auto derive_lane_state = [&](int lane_) {
    const int srow = lane_ >> 3;
    schunk = ((lane_ & 7) ^ ((4 * (wave & 1) + (lane_ >> 4)) & 7)) * 8;
    ra = wave * 8 + srow;
    // image rows 64 (w >> 2) + 8 (w & 3) + srow (+ 0, 128, 32, 160): q = (w >> 1) & 1, r = 8 (w & 1) + srow of the
    // permutation above, i.e. weight row 64 (w >> 2) + 16 (w & 1) + 8 (srow >> 2) + 4 ((w >> 1) & 1) + (srow & 3)
    rwp = 64 * (wave >> 2) + 16 * (wave & 1) + 8 * (srow >> 2) + 4 * ((wave >> 1) & 1) + (srow & 3);
    // fragments (v_mfma_f32_16x16x32_f16): lane l supplies row (l & 15), k = 8 (l >> 4) + j of a 32-deep step;
    // step kk of the K-tile is chunk 4 kk + (l >> 4) of the row, stored at chunk ^ ((row >> 1) & 7)
    const int frow = lane_ & 15;
    const int fsw = (frow >> 1) & 7;
    const int fq = lane_ >> 4;
    pa = ((wave >> 2) * 128 + frow) * 64;
    pw = 256 * 64 + ((wave & 3) * 64 + frow) * 64;
    fk0 = (fq ^ fsw) * 8, fk1 = ((4 + fq) ^ fsw) * 8;
  };
  derive_lane_state(lane);
  const half_t *g_a0, *g_a1, *g_a2, *g_a3, *g_w0, *g_w1, *g_w2, *g_w3;
  auto set_ptrs = [&](int bm_, int bn_) {
    g_a0 = Ah + static_cast<int64_t>(min(bm_ + ra, M - 1)) * K + schunk;        // lo
    g_a1 = Ah + static_cast<int64_t>(min(bm_ + ra + 128, M - 1)) * K + schunk;  // lo
    g_a2 = Ah + static_cast<int64_t>(min(bm_ + ra + 64, M - 1)) * K + schunk;   // hi
    g_a3 = Ah + static_cast<int64_t>(min(bm_ + ra + 192, M - 1)) * K + schunk;  // hi
    // W rows are staged PERMUTED inside every block of 32: image row 32 P + 16 q + r holds weight row
    // 32 P + 8 (r >> 2) + 4 q + (r & 3) — see the epilogue: a lane then owns 8 consecutive output features
    g_w0 = Wh + static_cast<int64_t>(min(bn_ + rwp, N - 1)) * K + schunk;        // lo
    g_w1 = Wh + static_cast<int64_t>(min(bn_ + rwp + 128, N - 1)) * K + schunk;  // lo
    g_w2 = Wh + static_cast<int64_t>(min(bn_ + rwp + 32, N - 1)) * K + schunk;   // hi
    g_w3 = Wh + static_cast<int64_t>(min(bn_ + rwp + 160, N - 1)) * K + schunk;  // hi
  };
  set_ptrs(bm, bn);
  // wave-uniform LDS destinations (halfs, inside a stage buffer)
  const int da0 = wave * 8 * 64, da1 = da0 + 128 * 64, da2 = da0 + 64 * 64, da3 = da0 + 192 * 64;
  const int dw0 = 256 * 64 + (64 * (wave >> 2) + 8 * (wave & 3)) * 64, dw1 = dw0 + 128 * 64, dw2 = dw0 + 32 * 64,
            dw3 = dw0 + 160 * 64;

  f32x4 acc[8][4];

  const int nk = K / 64;  // even
#define VR_PP_BARRIER()                 \
  do {                                  \
    __builtin_amdgcn_sched_barrier(0);  \
    __builtin_amdgcn_s_barrier();       \
    __builtin_amdgcn_sched_barrier(0);  \
  } while (0)
#define VR_PP_VMCNT4() asm volatile("s_waitcnt vmcnt(4)" ::: "memory")
  // Epilogues that issue a known number of stores and no global loads (whole tiles of the branch-free f16-output variants:
  // constants and row statistics come from LDS): the last two half-tiles of the next tile's K-tile 0 (W hi, A hi, requested
  // in the last two phases of the K loop) are NOT waited for before the epilogue — their latency runs under its arithmetic —
  // but by counted waits in the first two phases of the next K loop that let exactly the younger operations (A hi where
  // it applies, the kEpiStores stores, the phase's own loads) stay in flight. Every other epilogue drains vmcnt first.
  constexpr bool kTileEpilogue = EPI == EPI_FOLD_F16 || EPI == EPI_FOLD_GELU || EPI == EPI_BIAS_F16 || EPI == EPI_BIAS_GELU ||
                                 EPI == EPI_BIAS_RELU;
  constexpr int kEpiStores = kTileEpilogue ? 16 : -1;
  bool counted_tail = false;  // block-uniform: the previous tile's epilogue left W hi / A hi to the counted waits
#define VR_PP_VMCNT_TAIL() asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kEpiStores > 0 ? kEpiStores + 4 : 0) : "memory")

  // prologue: K-tile 0 of the first tile, all eight pieces, into buffer 0
  glds16(g_a0, lds + da0);
  glds16(g_a1, lds + da1);
  glds16(g_w0, lds + dw0);
  glds16(g_w1, lds + dw1);
  glds16(g_w2, lds + dw2);
  glds16(g_w3, lds + dw3);
  glds16(g_a2, lds + da2);
  glds16(g_a3, lds + da3);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  VR_PP_BARRIER();
  if (wm == 1) VR_PP_BARRIER();  // waves 4-7 run one segment behind from here on

  while (true) {
    const int next = tile + G;
    const bool has_next = next < total;
    int nbm = bm, nbn = bn;

    // one K-tile out of stage buffer B; the next K-tile (or K-tile 0 of the next tile, or — at the very
    // end — a harmless re-load) goes into buffer B ^ 1
    // FIRST (a tile's K-tile 0): the first MFMA into each accumulator takes a zero C operand instead of the accumulator, so
    // the accumulators are never cleared (128 v_mov per wave and tile, all eight waves at once, nothing under them)
    auto ktile = [&](auto bsel, int kt, auto first_sel) {
      constexpr int B = decltype(bsel)::value;
      constexpr bool FIRST = decltype(first_sel)::value;
      const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
      const half_t* st = lds + B * kStageHalfs;
      half_t* nd = lds + (B ^ 1) * kStageHalfs;
      const bool lastk = kt == nk - 1;
      if (lastk && has_next) set_ptrs(nbm, nbn);
      const int koff = lastk ? 0 : (kt + 1) * 64;
      f16x8 af[4][2], bf[2][2];
      // ---- phase 0: quadrant rows 0-63 x columns 0-31 ------------------------------------------------
      if (kt == 0) issue_tile_consts(bm, bn);  // (older than every load the counted waits below reason about)
      glds16(g_a0 + koff, nd + da0);
      glds16(g_a1 + koff, nd + da1);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        bf[j][0] = *reinterpret_cast<const f16x8*>(st + pw + j * 16 * 64 + fk0);
        bf[j][1] = *reinterpret_cast<const f16x8*>(st + pw + j * 16 * 64 + fk1);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        af[i][0] = *reinterpret_cast<const f16x8*>(st + pa + i * 16 * 64 + fk0);
        af[i][1] = *reinterpret_cast<const f16x8*>(st + pa + i * 16 * 64 + fk1);
      }
      if (kt != 0) VR_PP_VMCNT4();  // W hi of this K-tile has landed (K-tile 0: waited for whole, or by the counted tail)
      else if (kEpiStores > 0 && counted_tail) VR_PP_VMCNT_TAIL();  // younger: A hi, the stores, this phase's two loads
      VR_PP_BARRIER();
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[j][kk], af[i][kk], (FIRST && kk == 0) ? zero4 : acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      VR_PP_BARRIER();
      // ---- phase 1: rows 0-63 x columns 32-63 ---------------------------------------------------------
      glds16(g_w0 + koff, nd + dw0);
      glds16(g_w1 + koff, nd + dw1);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        bf[j][0] = *reinterpret_cast<const f16x8*>(st + pw + (2 + j) * 16 * 64 + fk0);
        bf[j][1] = *reinterpret_cast<const f16x8*>(st + pw + (2 + j) * 16 * 64 + fk1);
      }
      if (kt != 0) VR_PP_VMCNT4();  // A hi of this K-tile has landed
      else if (kEpiStores > 0 && counted_tail) VR_PP_VMCNT_TAIL();  // younger: the stores, the loads of phases 0 and 1
      VR_PP_BARRIER();
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[j][kk], af[i][kk], (FIRST && kk == 0) ? zero4 : acc[i][2 + j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      VR_PP_BARRIER();
      // ---- phase 2: rows 64-127 x columns 32-63 -------------------------------------------------------
      glds16(g_w2 + koff, nd + dw2);
      glds16(g_w3 + koff, nd + dw3);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        af[i][0] = *reinterpret_cast<const f16x8*>(st + pa + (4 + i) * 16 * 64 + fk0);
        af[i][1] = *reinterpret_cast<const f16x8*>(st + pa + (4 + i) * 16 * 64 + fk1);
      }
      VR_PP_BARRIER();
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[4 + i][2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[j][kk], af[i][kk], (FIRST && kk == 0) ? zero4 : acc[4 + i][2 + j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      VR_PP_BARRIER();
      // ---- phase 3: rows 64-127 x columns 0-31 (W fragments read again: holding them costs 16 VGPRs) ----
      glds16(g_a2 + koff, nd + da2);
      glds16(g_a3 + koff, nd + da3);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        bf[j][0] = *reinterpret_cast<const f16x8*>(st + pw + j * 16 * 64 + fk0);
        bf[j][1] = *reinterpret_cast<const f16x8*>(st + pw + j * 16 * 64 + fk1);
      }
      VR_PP_VMCNT4();  // A lo and W lo of the next K-tile have landed; W hi and A hi stay in flight
      VR_PP_BARRIER();
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[4 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[j][kk], af[i][kk], (FIRST && kk == 0) ? zero4 : acc[4 + i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      VR_PP_BARRIER();
    };
    ktile(std::integral_constant<int, 0>{}, 0, std::true_type{});
    // (the next tile's coordinates — three integer divisions — are worked out here, under the K loop, not between the
    // epilogue and the first K-tile where every wave of the block would wait for them)
    if (has_next) coords(next, nbm, nbn);
    ktile(std::integral_constant<int, 1>{}, 1, std::false_type{});
#pragma clang loop unroll(disable)
    for (int kt = 2; kt < nk; kt += 2) {
      ktile(std::integral_constant<int, 0>{}, kt, std::false_type{});
      ktile(std::integral_constant<int, 1>{}, kt + 1, std::false_type{});
    }

    // waves 0-3 are a segment ahead: they wait here for waves 4-7's last MFMA segment, so that all eight waves
    // run the epilogue TOGETHER (one half after the other costs 13 %: each wave's epilogue is bound by the latency of
    // its own loads, and the two waves of a SIMD hide each other's — profiles/r02_gemm_experiments.md §4)
    if (wm == 0) VR_PP_BARRIER();
    // Epilogue, straight from the accumulators (direct_epilogue).
    // W hi / A hi of the next tile's K-tile 0 may still be in flight: waited for HERE, before this wave's
    // stores queue up behind them (vmcnt retires in order: a counted wait in the next main loop would otherwise
    // wait for the stores too).
    // whole tile, or a last column tile that ends on a 64-column boundary: every wave's 64 columns are in or out as a whole
    const bool whole_tile = bm + GBM <= M && (bn + GBN <= N || N % 64 == 0);  // block-uniform
    const bool no_columns = bn + wn * 64 >= N;                                // wave-uniform: nothing to store
    counted_tail = kEpiStores > 0 && whole_tile;
    if (!counted_tail) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (whole_tile && no_columns)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the counted waits of the next K loop assume this wave's stores)
    else if (kTileEpilogue && whole_tile)
      f16_tile_epilogue<EPI>(acc, bm + wm * 128, bn + wn * 64, lane, Ch, M, N, unscale, reinterpret_cast<const float*>(tile_const_h),
                             wm * 128, wn * 64, xpose);
    else if (kRlsTile && whole_tile)
      rls16_tile_epilogue(acc, bm + wm * 128, bn + wn * 64, lane, reinterpret_cast<const half_t*>(R), Ch, Cl, M, N, unscale,
                          reinterpret_cast<const float*>(tile_const_h), wm * 128, wn * 64, xpose, xspare);
    else if (kBranchFree && whole_tile)
      direct_epilogue<EPI, true, true>(acc, bm + wm * 128, bn + wn * 64, lane, bias, R, C, Ch, Cl, M, N, unscale, ln_stat, ln_g, ln_b, wave_stat,
                                 reinterpret_cast<const float*>(tile_const_h), wm * 128, wn * 64, xpose);
    else
      direct_epilogue<EPI, false, !kRlsTile>(acc, bm + wm * 128, bn + wn * 64, lane, bias, R, C, Ch, Cl, M, N, unscale, ln_stat, ln_g, ln_b, wave_stat,
                                  nullptr, 0, 0, xpose);
    if (!has_next) break;
    tile = next;
    bm = nbm;
    bn = nbn;
    // the eight staging pointers (16 registers) are dead through the epilogue: they are derived again here, from tile
    // coordinates the compiler cannot match with the ones the last K-tile used (else it keeps the old values alive)
    asm volatile("" : "+s"(bm), "+s"(bn));
    {
      int lane_again = lane;
      asm volatile("" : "+v"(lane_again));
      derive_lane_state(lane_again);
    }
    set_ptrs(bm, bn);
    VR_PP_BARRIER();
    if (wm == 1) VR_PP_BARRIER();  // waves 4-7 fall one segment behind again
  }  // tiles
#undef VR_PP_BARRIER
#undef VR_PP_VMCNT4
#undef VR_PP_VMCNT_TAIL
}

// ---- the f16 product for mid-size M: 128x128 tiles, three blocks per CU ------------------------------------
//
// gemm_f16_pp_kernel owns a CU alone (128 KiB of LDS, 8 waves) and walks 256x256 tiles: at 1.6k tokens and N = 768
// those number 7 x 3 = 21 for 256 CUs. Here (256 < M, a batch of questions or one file's chunks: mid_usable) a block
// is TWO waves on a 128-token x 128-feature tile with 48 KiB of stages, three blocks per CU: 13 x 6 = 78 tiles.
//   * K advances in steps of 32 through a ring of THREE stage buffers (A 128 x 32 + W 128 x 32 halfs = 16 KiB):
//     step s multiplies out of stage s % 3 while the loads of steps s + 1 and s + 2 are in flight — one
//     counted vmcnt(8) and one barrier per step (every wave issues 4 + 4 direct-to-LDS loads per step);
//   * rows are 64 bytes in LDS; 16-byte chunk c of row r sits at chunk c ^ ((r >> 1) & 3) (source-side swizzle of
//     the direct-to-LDS loads), which makes the ds_read_b128 fragment reads conflict-free;
//   * same wave tile (128 x 64), fragment roles, W row permutation and accumulation order (k ascending) as
//     gemm_f16_pp_kernel: the result is bit-identical to it, and the epilogue is the same code (direct_epilogue).
// One tile per block, no persistence: consecutive blocks of an XCD (blockIdx % 8) take the column tiles of one
// 128-row panel one after the other, so a panel of A is read from HBM once and then from that XCD's L2.
// (The same loop on 256x128 tiles, four waves and two blocks per CU, was tried as a replacement for the ping-pong
// kernel and lost, 750 against 930 TFLOP/s: profiles/r02_gemm_experiments.md)
constexpr int kMidM = 128, kMidN = 128, kMidK = 32;
constexpr int kMidStageHalfs = (kMidM + kMidN) * kMidK;

template <int EPI>
__global__ __launch_bounds__(128, 2) void gemm_f16_mid_kernel(
    const half_t* __restrict__ Ah, const half_t* __restrict__ Wh, const float* __restrict__ bias,
    const float* __restrict__ R, float* __restrict__ C, half_t* __restrict__ Ch, half_t* __restrict__ Cl, int M,
    int N, int K, float unscale, const float2* __restrict__ ln_stat, const float* __restrict__ ln_g,
    const float* __restrict__ ln_b) {
  constexpr int NW = 2;                            // waves: one row of two 128 x 64 wave tiles
  constexpr int TM = kMidM;                        // token rows of the block tile
  constexpr int kStage = kMidStageHalfs;
  constexpr int kLoadsW = 8 / NW;                  // W image loads per wave and step (A: always 4)
  __shared__ half_t lds[3 * kStage + NW * kWaveStatHalfs];  // the only LDS object (see gemm_f16x3_256_kernel)
  const int tiles_n = (N + kMidN - 1) / kMidN;
  const int tiles_m = (M + TM - 1) / TM;
  const int xcd = static_cast<int>(blockIdx.x) & 7, seq = static_cast<int>(blockIdx.x) >> 3;
  const int panel = (seq / tiles_n) * 8 + xcd;
  if (panel >= tiles_m) return;  // block-uniform (the grid is padded to a multiple of 8 panels)
  const int bm = panel * TM, bn = (seq % tiles_n) * kMidN;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  float2* wave_stat = reinterpret_cast<float2*>(lds + 3 * kStage + wave * kWaveStatHalfs);

  // staging: one direct-to-LDS load moves 16 rows x 64 B; lane -> row (lane >> 2) of the 16, LDS chunk (lane & 3),
  // source chunk (lane & 3) ^ ((row >> 1) & 3). Wave w stages A rows 16 (w + NW t) + .. (t = 0..3) and W image rows
  // 16 (w + NW t) + .. (t < 8 / NW); image row 32 P + 16 q + r holds weight row 32 P + 8 (r >> 2) + 4 q + (r & 3)
  // (direct_epilogue: a lane then owns 8 consecutive output features).
  const int srow = lane >> 2;
  const int schunk = ((lane & 3) ^ ((srow >> 1) & 3)) * 8;
  const half_t* g_a[4];
  const half_t* g_w[kLoadsW];
#pragma unroll
  for (int t = 0; t < 4; ++t)
    g_a[t] = Ah + static_cast<int64_t>(min(bm + 16 * (wave + NW * t) + srow, M - 1)) * K + schunk;
#pragma unroll
  for (int t = 0; t < kLoadsW; ++t) {
    const int img = 16 * (wave + NW * t);  // first image row of the instruction: P = img >> 5, q = (img >> 4) & 1
    const int wrow = (img & ~31) + 8 * (srow >> 2) + 4 * ((img >> 4) & 1) + (srow & 3);
    g_w[t] = Wh + static_cast<int64_t>(min(bn + wrow, N - 1)) * K + schunk;
  }
  const int da = wave * 16 * kMidK;               // + NW t * 16 * kMidK
  const int dw = TM * kMidK + wave * 16 * kMidK;    // + NW t * 16 * kMidK

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // fragments (v_mfma_f32_16x16x32_f16): lane l supplies row (l & 15), k = 8 (l >> 4) + j of the 32-deep step
  const int frow = lane & 15;
  const int fk = ((lane >> 4) ^ ((frow >> 1) & 3)) * 8;
  const int pa = (wm * 128 + frow) * kMidK + fk;
  const int pw = TM * kMidK + (wn * 64 + frow) * kMidK + fk;
  const int nk = K / kMidK;

#define VR_MID_BARRIER()                   \
  do {                                    \
    __builtin_amdgcn_sched_barrier(0);    \
    __builtin_amdgcn_s_barrier();         \
    __builtin_amdgcn_sched_barrier(0);    \
  } while (0)
  auto issue = [&](half_t* stage, int k0) {
#pragma unroll
    for (int t = 0; t < 4; ++t) glds16(g_a[t] + k0, stage + da + t * NW * 16 * kMidK);
#pragma unroll
    for (int t = 0; t < kLoadsW; ++t) glds16(g_w[t] + k0, stage + dw + t * NW * 16 * kMidK);
  };
  issue(lds, 0);
  if (nk > 1) issue(lds + kStage, kMidK);

  auto step = [&](auto bsel, int s) {
    constexpr int B = decltype(bsel)::value;
    const half_t* st = lds + B * kStage;
    half_t* nd = lds + ((B + 2) % 3) * kStage;
    // the loads of step s have landed (those of step s + 1, if any, stay in flight) ...
    if (s + 1 < nk) {
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // (4 + 4 loads per wave and step)
    } else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    VR_MID_BARRIER();  // ... every wave's; and every wave has finished with stage (s - 1) % 3 = (s + 2) % 3
    if (s + 2 < nk) issue(nd, (s + 2) * kMidK);
    f16x8 af[4], bf[4];  // token rows in two halves of 64: holding all eight fragments did not fit beside acc
#pragma unroll
    for (int j = 0; j < 4; ++j)
      bf[j] = *reinterpret_cast<const f16x8*>(st + pw + j * 16 * kMidK);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        af[i] = *reinterpret_cast<const f16x8*>(st + pa + (4 * h + i) * 16 * kMidK);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[4 * h + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[j], af[i], acc[4 * h + i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
  };
  int s = 0;
#pragma clang loop unroll(disable)
  for (; s + 3 <= nk; s += 3) {
    step(std::integral_constant<int, 0>{}, s);
    step(std::integral_constant<int, 1>{}, s + 1);
    step(std::integral_constant<int, 2>{}, s + 2);
  }
  if (s < nk) step(std::integral_constant<int, 0>{}, s);
  if (s + 1 < nk) step(std::integral_constant<int, 1>{}, s + 1);
#undef VR_MID_BARRIER
  // (EPI_RLS_R32_O16 — layer 0 only — holds two pieces of f32 residual rows: four registers too many without branches)
  if (EPI != EPI_RLS_R32_O16 && bm + TM <= M && bn + kMidN <= N)  // block-uniform
    direct_epilogue<EPI, true>(acc, bm + wm * 128, bn + wn * 64, lane, bias, R, C, Ch, Cl, M, N, unscale, ln_stat, ln_g, ln_b, wave_stat);
  else
    direct_epilogue<EPI, false>(acc, bm + wm * 128, bn + wn * 64, lane, bias, R, C, Ch, Cl, M, N, unscale, ln_stat, ln_g, ln_b, wave_stat);
}

// ---- skinny product for M <= 256 rows (one query, a handful of sequences) ---------------------------
//
// With a few rows the 256x256 kernel leaves the chip empty (N / 256 blocks, each walking all of K:
// 1.7 ms for a 12-token bge-base query). Here the work is cut along N (64 columns per block) AND along
// K (slices of kSkinnyK), so 50-200 blocks stream disjoint slabs of the weight matrix — the only real
// traffic — and write f32 partial sums; a second small kernel adds the slices and applies the
// epilogue. D[n][m] = sum_k W[n][k] A[m][k] on v_mfma_f32_16x16x32_f16: W rows are the MFMA rows, the
// activation rows (64 per block) its columns; both operands are 16-byte global loads (k contiguous).
// f16 mode only (plain f16 rows).
constexpr int kSkinnyM = 64;
// K slice per block: the largest of these that divides K (192 for 384 / 768 / 1536 / 3072, 256 for 1024 / 4096)
static int skinny_slice(int K) {
  for (int c : {192, 256, 128, 64, 32})
    if (K % c == 0) return c;
  return 0;
}

__global__ __launch_bounds__(256) void gemm_f16_skinny_kernel(const half_t* __restrict__ A, const half_t* __restrict__ W,
                                                              float* __restrict__ part, int M, int N, int K,
                                                              int kslice) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 64 + wave * 16;  // this wave's 16 output columns
  const int k0 = blockIdx.y * kslice;
  const int row = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.z * kSkinnyM;  // 64 activation rows per block
  if (n0 >= N) return;
  const half_t* wp = W + static_cast<int64_t>(min(n0 + row, N - 1)) * K + k0 + 8 * g;
  const half_t* ap[4];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) ap[mb] = A + static_cast<int64_t>(min(m0 + mb * 16 + row, M - 1)) * K + k0 + 8 * g;
  f32x4 acc[4];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) acc[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int mblocks = (min(M - m0, kSkinnyM) + 15) / 16;
  for (int k = 0; k < kslice; k += 32) {
    const f16x8 wf = *reinterpret_cast<const f16x8*>(wp + k);
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
      if (mb < mblocks) {
        const f16x8 af = *reinterpret_cast<const f16x8*>(ap[mb] + k);
        acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, af, acc[mb], 0, 0, 0);
      }
  }
  // C layout: column (lane & 15) = activation row m, rows 4g + r = output columns n0 + 4g + r
  float* dst = part + static_cast<int64_t>(blockIdx.y) * M * N;
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) {
    const int m = m0 + mb * 16 + row;
    if (mb < mblocks && m < M && n0 + 4 * g < N)
      *reinterpret_cast<float4*>(dst + static_cast<int64_t>(m) * N + n0 + 4 * g) =
          make_float4(acc[mb][0], acc[mb][1], acc[mb][2], acc[mb][3]);
  }
}

// the epilogue of the 256-tile kernel (same formulas) for the float4 of raw sums v at row m, column n
template <int EPI>
__device__ __forceinline__ void skinny_apply(float4 v, int m, int n, int N, float unscale,
                                             const float* __restrict__ bias, const float* __restrict__ R,
                                             const float2* __restrict__ ln_stat, const float* __restrict__ ln_g,
                                             const float* __restrict__ ln_b, float* __restrict__ C,
                                             half_t* __restrict__ Ch) {
  const int64_t o = static_cast<int64_t>(m) * N + n;
  const float4 b4 = *reinterpret_cast<const float4*>(bias + n);
  v.x = v.x * unscale + b4.x;
  v.y = v.y * unscale + b4.y;
  v.z = v.z * unscale + b4.z;
  v.w = v.w * unscale + b4.w;
  if (EPI == EPI_BIAS_GELU) {
    const f32x2 g01 = gelu_poly2(f32x2{v.x, v.y}), g23 = gelu_poly2(f32x2{v.z, v.w});  // f16 mode only
    v = make_float4(g01.x, g01.y, g23.x, g23.y);
  }
  if (EPI == EPI_BIAS_RELU) v = make_float4(fmaxf(v.x, 0.0f), fmaxf(v.y, 0.0f), fmaxf(v.z, 0.0f), fmaxf(v.w, 0.0f));
  if (EPI == EPI_SWIGLU_F16 || EPI == EPI_GEGLU_F16) {  // columns n .. n + 3 = gate_j, up_j, gate_j+1, up_j+1, j = n / 2
    constexpr int kFfn = EPI == EPI_SWIGLU_F16 ? VR_FFN_SWIGLU : VR_FFN_GEGLU;
    const float o0 = glu_act<false>(v.x, kFfn) * v.y, o1 = glu_act<false>(v.z, kFfn) * v.w;
    half_t h[2] = {static_cast<half_t>(fminf(fmaxf(o0, -65504.0f), 65504.0f)),
                   static_cast<half_t>(fminf(fmaxf(o1, -65504.0f), 65504.0f))};
    *reinterpret_cast<uint32_t*>(Ch + static_cast<int64_t>(m) * (N >> 1) + (n >> 1)) = *reinterpret_cast<const uint32_t*>(h);
    return;
  }
  if (EPI == EPI_ROPE_F16) {  // N = 3H; (v.x, v.y) and (v.z, v.w) are rotation partners in the query and key thirds
    const int H = N / 3;
    if (n < 2 * H) {
      const int c = n >= H ? n - H : n;
      const int p = reinterpret_cast<const int32_t*>(ln_g)[m];
      const float4 cs = *reinterpret_cast<const float4*>(ln_stat + static_cast<int64_t>(p) * (H >> 1) + (c >> 1));
      const float x0 = v.x, y0 = v.y, x1 = v.z, y1 = v.w;
      v.x = x0 * cs.x - y0 * cs.y;
      v.y = y0 * cs.x + x0 * cs.y;
      v.z = x1 * cs.z - y1 * cs.w;
      v.w = y1 * cs.z + x1 * cs.w;
    }
  }
  if (EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_RELU || EPI == EPI_BIAS_F16 || EPI == EPI_ROPE_F16) {
    half_t h[4] = {static_cast<half_t>(fminf(fmaxf(v.x, -65504.0f), 65504.0f)),
                   static_cast<half_t>(fminf(fmaxf(v.y, -65504.0f), 65504.0f)),
                   static_cast<half_t>(fminf(fmaxf(v.z, -65504.0f), 65504.0f)),
                   static_cast<half_t>(fminf(fmaxf(v.w, -65504.0f), 65504.0f))};
    *reinterpret_cast<uint2*>(Ch + o) = *reinterpret_cast<const uint2*>(h);
    return;
  }
  if (EPI == EPI_BIAS_RESIDUAL || EPI == EPI_BIAS_RESIDUAL_LN) {
    const float4 r = *reinterpret_cast<const float4*>(R + o);
    if (EPI == EPI_BIAS_RESIDUAL_LN) {
      const float2 st = ln_stat[m];
      const float4 lg = *reinterpret_cast<const float4*>(ln_g + n), lb = *reinterpret_cast<const float4*>(ln_b + n);
      v.x += ln_apply(r.x, st.x, st.y, lg.x, lb.x);
      v.y += ln_apply(r.y, st.x, st.y, lg.y, lb.y);
      v.z += ln_apply(r.z, st.x, st.y, lg.z, lb.z);
      v.w += ln_apply(r.w, st.x, st.y, lg.w, lb.w);
    } else {
      v.x += r.x;
      v.y += r.y;
      v.z += r.z;
      v.w += r.w;
    }
  }
  *reinterpret_cast<float4*>(C + o) = v;
}

// sum of the K slices + epilogue, one float4 per thread (second launch of the split-K skinny GEMM)
template <int EPI>
__global__ void skinny_epilogue_kernel(const float* __restrict__ part, int slices, int M, int N, float unscale,
                                       const float* __restrict__ bias, const float* __restrict__ R,
                                       const float2* __restrict__ ln_stat, const float* __restrict__ ln_g,
                                       const float* __restrict__ ln_b, float* __restrict__ C,
                                       half_t* __restrict__ Ch) {
  const int64_t i4 = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t total4 = static_cast<int64_t>(M) * N / 4;
  if (i4 >= total4) return;
  const int64_t o = i4 * 4;
  const int m = static_cast<int>(o / N), n = static_cast<int>(o % N);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < slices; ++s) {
    const float4 p = *reinterpret_cast<const float4*>(part + static_cast<int64_t>(s) * M * N + o);
    v.x += p.x;
    v.y += p.y;
    v.z += p.z;
    v.w += p.w;
  }
  skinny_apply<EPI>(v, m, n, N, unscale, bias, R, ln_stat, ln_g, ln_b, C, Ch);
}

// One launch per skinny GEMM when K % 128 == 0 (every width of the supported models): a block owns 16
// output columns and (up to) 64 activation rows; its NW = 8 (4 when K % 256 != 0) waves each take 1/NW of K
// — so the weight slab of the block (16 x K halfs) is streamed by all of them at once, in 1-3 memory round
// trips per wave — and meet in LDS, where the shares are summed in wave order and the epilogue is applied. N/16 blocks (48-192 for the base
// model) keep the weight stream wide without any cross-block reduction: a second launch costs ~4 us
// here and a device-scope fence per block costs more, an LDS barrier costs nothing.
template <int EPI, int UNR, int NW>
__global__ __launch_bounds__(NW * 64) void gemm_f16_skinny1_kernel(const half_t* __restrict__ A, const half_t* __restrict__ W,
                                                               int M, int N, int K, float unscale,
                                                               const float* __restrict__ bias,
                                                               const float* __restrict__ R,
                                                               const float2* __restrict__ ln_stat,
                                                               const float* __restrict__ ln_g,
                                                               const float* __restrict__ ln_b, float* __restrict__ C,
                                                               half_t* __restrict__ Ch) {
  __shared__ float red[NW][4][16][17];  // [wave][m block][output column][activation row (+1 pad)]
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 16;
  const int m0 = blockIdx.y * kSkinnyM;
  const int row = lane & 15, g = lane >> 4;
  const int kq = K / NW, k0 = wave * kq;  // this wave's share of K
  const half_t* wp = W + static_cast<int64_t>(n0 + row) * K + k0 + 8 * g;
  const half_t* ap[4];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) ap[mb] = A + static_cast<int64_t>(min(m0 + mb * 16 + row, M - 1)) * K + k0 + 8 * g;
  f32x4 acc[4];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) acc[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int mblocks = (min(M - m0, kSkinnyM) + 15) / 16;
  // UNR 32-deep steps at a time: all their loads are issued before the first MFMA (a dependent load per
  // step would expose one memory latency per step, and a query's forward pass is nothing but latency)
  for (int k = 0; k < kq; k += 32 * UNR) {
    f16x8 wf[UNR], af[UNR][4];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      wf[u] = *reinterpret_cast<const f16x8*>(wp + k + 32 * u);
#pragma unroll
      for (int mb = 0; mb < 4; ++mb)
        if (mb < mblocks) af[u][mb] = *reinterpret_cast<const f16x8*>(ap[mb] + k + 32 * u);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
      for (int mb = 0; mb < 4; ++mb)
        if (mb < mblocks) acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[u], af[u][mb], acc[mb], 0, 0, 0);
  }
  // C layout: column (lane & 15) = activation row, rows 4g + r = output columns n0 + 4g + r
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][mb][4 * g + r][row] = acc[mb][r];
  __syncthreads();
  if (threadIdx.x >= 256) return;
  const int ml = threadIdx.x >> 2, n4 = (threadIdx.x & 3) * 4;  // 64 rows x 4 float4 of columns
  const int m = m0 + ml;
  if (m >= M) return;
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float sum = red[0][ml >> 4][n4 + j][ml & 15];
#pragma unroll
    for (int w = 1; w < NW; ++w) sum += red[w][ml >> 4][n4 + j][ml & 15];  // fixed order
    v[j] = sum;
  }
  skinny_apply<EPI>(make_float4(v[0], v[1], v[2], v[3]), m, n0 + n4, N, unscale, bias, R, ln_stat, ln_g, ln_b, C, Ch);
}

// weights: w * scale -> (hi, lo); scale is a power of two chosen from max|w| of the tensor
__global__ void absmax_kernel(const float* __restrict__ w, int64_t n, unsigned int* __restrict__ out) {
  float m = 0.0f;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x)
    m = fmaxf(m, fabsf(w[i]));
  m = fmaxf(m, __shfl_xor(m, 32));
  m = fmaxf(m, __shfl_xor(m, 16));
  m = fmaxf(m, __shfl_xor(m, 8));
  m = fmaxf(m, __shfl_xor(m, 4));
  m = fmaxf(m, __shfl_xor(m, 2));
  m = fmaxf(m, __shfl_xor(m, 1));
  if ((threadIdx.x & 63) == 0) atomicMax(out, __float_as_uint(m));  // non-negative floats order as uints
}

__global__ void split_weights_kernel(const float* __restrict__ w, int64_t n, int K, float scale,
                                     half_t* __restrict__ hi, half_t* __restrict__ lo) {
  int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) {
    half_t h, l;
    split_f16(w[i] * scale, h, l);
    if (lo) {
      const int64_t o = (i / K) * (2 * K) + split_at(static_cast<int>(i % K));  // interleaved layout, see split_at
      hi[o] = h;
      lo[o] = l;
    } else {
      hi[i] = h;  // plain f16 rows (VR_PRECISION_F16)
    }
  }
}

// One product C = A W^T * unscale + bias (+ epilogue) as launch_gemm_f16x3 and the launchers behind it take it: a call
// site names the fields its epilogue uses, the rest stay null.
struct GemmArgs {
  const half_t *A = nullptr, *A_lo = nullptr;  // activation rows; passes = 3: interleaved (hi, lo) rows, A_lo = A + 8
  SplitWeight W{};                             // [N][K] weights (lo: passes = 3 only) and their 2^-s
  const float* bias = nullptr;
  const float* R = nullptr;                    // residual rows (EPI_RLS_R16_*: f16 rows behind this pointer)
  float* C = nullptr;                          // f32 output rows
  half_t *Ch = nullptr, *Cl = nullptr;         // f16 output rows (hi, lo); *_STATS / EPI_RLS_*: Cl = the rows' partial sums
  int M = 0, N = 0, K = 0;
  int passes = 3;                              // 3: (hi, lo) operands, three MFMA passes; 1: plain f16 rows
  const float2* ln_stat = nullptr;             // per row (mean, 1/sigma) of the LayerNorm an epilogue applies,
  const float *ln_g = nullptr, *ln_b = nullptr;  // its gain (EPI_FOLD_*: the column sums) and shift
  const float2* rope_tab = nullptr;            // EPI_ROPE_F16: the cos/sin table and the rows' positions
  const int32_t* rope_pos = nullptr;
};

// the kernels whose epilogue is direct_epilogue (gemm_f16_mid_kernel, gemm_f16_pp_kernel) exist for these
#define VR_DIRECT_EPIS                                                                                          \
  EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESIDUAL, EPI_BIAS_F16, EPI_BIAS_RESIDUAL_LN, EPI_FOLD_F16, EPI_FOLD_GELU,  \
      EPI_FOLD_SWIGLU, EPI_FOLD_GEGLU, EPI_BIAS_RESIDUAL_LN_STATS, EPI_RLS_R32_O16, EPI_RLS_R16_O16, EPI_RLS_R16_O32,     \
      EPI_BIAS_RELU

// (the launch_* below return false for an epilogue their kernel does not exist for: launch_gemm_f16x3 reports it)
template <int PASSES>
static bool launch_256(int epi, int grid, hipStream_t s, const GemmArgs& g) {
  auto launch = [&](auto E) {
    hipLaunchKernelGGL((gemm_f16x3_256_kernel<decltype(E)::value, PASSES>), dim3(grid), dim3(512), 0, s, g.A, g.A_lo, g.W.hi,
                       g.W.lo, g.bias, g.R, g.C, g.Ch, g.Cl, g.M, g.N, g.K, g.W.unscale, g.ln_stat, g.ln_g, g.ln_b);
  };
  if constexpr (PASSES == 1)  // the EPI_FOLD_* / *_STATS variants exist for plain f16 operands only
    return with_epi<EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESIDUAL, EPI_BIAS_F16, EPI_BIAS_RESIDUAL_LN, EPI_FOLD_F16,
                    EPI_FOLD_GELU, EPI_BIAS_RESIDUAL_LN_STATS, EPI_BIAS_RELU>(epi, launch);
  else
    return with_epi<EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESIDUAL, EPI_BIAS_F16, EPI_BIAS_RESIDUAL_LN, EPI_BIAS_RELU>(epi, launch);
}

// the ping-pong kernel serves the f16 mode when K is whole pairs of 64-deep K-tiles and a lane's 8 features are in
// or out of N together
static bool pp_usable(int N, int K) { return K % 128 == 0 && N % 8 == 0; }

// gemm_f16_mid_kernel (128x128 tiles) in place of the ping-pong kernel for 256 < M while the 256x256 tiles would fill
// at most a quarter of the CUs. Measured on an MI355X: at 21-48 ping-pong tiles (1k tokens,
// N = 768 / 2304 / 3072) it is 15-40 % faster; at 189 (16k tokens, N = 768) up to 35 % slower; the shapes between were
// not measured and stay with the ping-pong kernel. VR_GEMM_MID=0 turns it off (the bit-identity test's reference).
static bool mid_usable(int M, int N, int K, int n_cu) {
  static const bool mid_on = !(getenv("VR_GEMM_MID") && atoi(getenv("VR_GEMM_MID")) == 0);
  if (!mid_on || K % kMidK != 0 || N % 8 != 0 || M <= 256) return false;
  const int tiles_pp = ((M + GBM - 1) / GBM) * ((N + GBN - 1) / GBN);
  return 4 * tiles_pp <= n_cu;
}

// the kernels whose epilogue is direct_epilogue (all EPI_* variants, f16 residual stream included)
static bool direct_usable(int N, int K) { return pp_usable(N, K); }

static bool launch_mid(int epi, hipStream_t s, const GemmArgs& g) {
  const int tiles_m = (g.M + kMidM - 1) / kMidM, tiles_n = (g.N + kMidN - 1) / kMidN;
  const int grid = (tiles_m + 7) / 8 * 8 * tiles_n;
  return with_epi<VR_DIRECT_EPIS>(epi, [&](auto E) {
    hipLaunchKernelGGL((gemm_f16_mid_kernel<decltype(E)::value>), dim3(grid), dim3(128), 0, s, g.A, g.W.hi, g.bias, g.R, g.C,
                       g.Ch, g.Cl, g.M, g.N, g.K, g.W.unscale, g.ln_stat, g.ln_g, g.ln_b);
  });
}

static bool launch_pp(int epi, int grid, hipStream_t s, const GemmArgs& g) {
  return with_epi<VR_DIRECT_EPIS>(epi, [&](auto E) {  // (no start-time stagger; tile walk in groups of kGroupM256 row panels)
    hipLaunchKernelGGL((gemm_f16_pp_kernel<decltype(E)::value>), dim3(grid), dim3(512), 0, s, g.A, g.W.hi, g.bias, g.R, g.C,
                       g.Ch, g.Cl, g.M, g.N, g.K, g.W.unscale, g.ln_stat, g.ln_g, g.ln_b, 0, kGroupM256);
  });
}
#undef VR_DIRECT_EPIS

// The skinny GEMM of a handful of tokens (M <= 16) with the LayerNorm IN FRONT of it folded in: the
// activation operand is built from the pre-LayerNorm f32 rows instead of being read as f16 rows that a
// LayerNorm launch wrote a few microseconds earlier. Every block recomputes the (mean, 1/sigma) of the
// <= 16 rows (two passes over values it holds in registers, cross-wave sums in LDS in wave order, so every
// block gets the same bits), normalises its waves' shares of the columns and feeds the MFMA; block 0 also
// stores the statistics, which the residual epilogue of the NEXT projection needs (ln_apply re-derives
// the LayerNorm output from the pre-LN row). K = hidden size: each wave holds STEPS * 8 values per row.
// Two launches fewer per layer for a single query (7 -> 5): its forward pass is launch latency, not work.
// (gemm_f16_skinny_ln_body: shared by the kernel below and its rotary twin, which has two arguments more)
// RMS (VR_NORM_PRE_RMS, gemm_f16_skinny_rms_kernel): the folded norm is RMSNorm — the sum pass and its `part` reduction
// are gone, the one that is left sums the squares of the values themselves, ln_b is never read, stat_out gets (0, 1/rms).
template <int EPI, int STEPS, int NW, bool RMS = false>
__device__ __forceinline__ void gemm_f16_skinny_ln_body(
    const float* __restrict__ pre, const float* __restrict__ ln_g, const float* __restrict__ ln_b, float eps,
    float2* __restrict__ stat_out, const half_t* __restrict__ W, int M, int N, int K, float unscale,
    const float* __restrict__ bias, half_t* __restrict__ Ch, const float2* __restrict__ rope_tab,
    const int32_t* __restrict__ rope_pos) {
  __shared__ float red[NW][16][17];  // [wave][output column][activation row (+1 pad)]
  __shared__ float part[RMS ? 1 : 2][NW][16];  // row sums per wave: [pass][wave][row]
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 16;
  const int row = lane & 15, g = lane >> 4;
  const int kq = K / NW, k0 = wave * kq;
  const float* xp = pre + static_cast<int64_t>(min(row, M - 1)) * K + k0 + 8 * g;
  const half_t* wp = W + static_cast<int64_t>(n0 + row) * K + k0 + 8 * g;
  float x[STEPS][8];
  f16x8 wf[STEPS];
  float sum = 0.0f;
#pragma unroll
  for (int u = 0; u < STEPS; ++u) {
    wf[u] = *reinterpret_cast<const f16x8*>(wp + 32 * u);
    const float4 a = *reinterpret_cast<const float4*>(xp + 32 * u), c = *reinterpret_cast<const float4*>(xp + 32 * u + 4);
    x[u][0] = a.x, x[u][1] = a.y, x[u][2] = a.z, x[u][3] = a.w, x[u][4] = c.x, x[u][5] = c.y, x[u][6] = c.z, x[u][7] = c.w;
#pragma unroll
    for (int j = 0; j < 8; ++j) sum += x[u][j];
  }
  // a row's values of this wave sit in the four lanes row, row + 16, row + 32, row + 48
  float mean = 0.0f;  // (RMS: stays 0, and the squares below are the values' own)
  if constexpr (!RMS) {
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    if (g == 0) part[0][wave][row] = sum;
    __syncthreads();
    float total = part[0][0][row];
#pragma unroll
    for (int w = 1; w < NW; ++w) total += part[0][w][row];
    mean = total / static_cast<float>(K);
  }
  constexpr int kSq = RMS ? 0 : 1;  // the `part` plane of the squares
  float sq = 0.0f;
#pragma unroll
  for (int u = 0; u < STEPS; ++u)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = x[u][j] - mean;
      sq += d * d;
    }
  sq += __shfl_xor(sq, 16);
  sq += __shfl_xor(sq, 32);
  if (g == 0) part[kSq][wave][row] = sq;
  __syncthreads();
  float total_sq = part[kSq][0][row];
#pragma unroll
  for (int w = 1; w < NW; ++w) total_sq += part[kSq][w][row];
  const float inv = 1.0f / sqrtf(total_sq / static_cast<float>(K) + eps);
  if (blockIdx.x == 0 && wave == 0 && g == 0 && row < M) stat_out[row] = make_float2(mean, inv);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < STEPS; ++u) {
    const float4 g0 = *reinterpret_cast<const float4*>(ln_g + k0 + 8 * g + 32 * u), g1 = *reinterpret_cast<const float4*>(ln_g + k0 + 8 * g + 32 * u + 4);
    float4 b0 = {}, b1 = {};
    if constexpr (!RMS) {
      b0 = *reinterpret_cast<const float4*>(ln_b + k0 + 8 * g + 32 * u), b1 = *reinterpret_cast<const float4*>(ln_b + k0 + 8 * g + 32 * u + 4);
    }
    const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
    const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    f16x8 af;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      half_t h, l;
      // as layernorm_f16_kernel (RMS: rmsnorm_f16_kernel) rounds its output
      split_f16(RMS ? rms_apply(x[u][j], inv, gg[j]) : ln_apply(x[u][j], mean, inv, gg[j], bb[j]), h, l);
      af[j] = h;
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[u], af, acc, 0, 0, 0);
  }
  // C layout: column (lane & 15) = activation row, rows 4g + r = output columns n0 + 4g + r
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wave][4 * g + r][row] = acc[r];
  __syncthreads();
  if (threadIdx.x >= 64) return;
  const int m = threadIdx.x >> 2, n4 = (threadIdx.x & 3) * 4;  // 16 rows x 4 float4 of columns
  if (m >= M) return;
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float t = red[0][n4 + j][m];
#pragma unroll
    for (int w = 1; w < NW; ++w) t += red[w][n4 + j][m];  // fixed order
    v[j] = t;
  }
  skinny_apply<EPI>(make_float4(v[0], v[1], v[2], v[3]), m, n0 + n4, N, unscale, bias, nullptr, rope_tab,
                    reinterpret_cast<const float*>(rope_pos), nullptr, nullptr, Ch);
}

template <int EPI, int STEPS, int NW>
__global__ __launch_bounds__(NW * 64) void gemm_f16_skinny_ln_kernel(
    const float* __restrict__ pre, const float* __restrict__ ln_g, const float* __restrict__ ln_b, float eps,
    float2* __restrict__ stat_out, const half_t* __restrict__ W, int M, int N, int K, float unscale,
    const float* __restrict__ bias, half_t* __restrict__ Ch) {
  gemm_f16_skinny_ln_body<EPI, STEPS, NW>(pre, ln_g, ln_b, eps, stat_out, W, M, N, K, unscale, bias, Ch, nullptr, nullptr);
}

// VR_NORM_PRE_RMS: the folded norm is RMSNorm (no shift argument)
template <int EPI, int STEPS, int NW>
__global__ __launch_bounds__(NW * 64) void gemm_f16_skinny_rms_kernel(
    const float* __restrict__ pre, const float* __restrict__ ln_g, float eps, float2* __restrict__ stat_out,
    const half_t* __restrict__ W, int M, int N, int K, float unscale, const float* __restrict__ bias,
    half_t* __restrict__ Ch) {
  gemm_f16_skinny_ln_body<EPI, STEPS, NW, true>(pre, ln_g, nullptr, eps, stat_out, W, M, N, K, unscale, bias, Ch, nullptr, nullptr);
}

// EPI_ROPE_F16: the Q/K/V projection of a rotary model, with the cos/sin table and the rows' positions
template <int STEPS, int NW>
__global__ __launch_bounds__(NW * 64) void gemm_f16_skinny_ln_rope_kernel(
    const float* __restrict__ pre, const float* __restrict__ ln_g, const float* __restrict__ ln_b, float eps,
    float2* __restrict__ stat_out, const half_t* __restrict__ W, int M, int N, int K, float unscale,
    const float* __restrict__ bias, half_t* __restrict__ Ch, const float2* __restrict__ rope_tab,
    const int32_t* __restrict__ rope_pos) {
  gemm_f16_skinny_ln_body<EPI_ROPE_F16, STEPS, NW>(pre, ln_g, ln_b, eps, stat_out, W, M, N, K, unscale, bias, Ch, rope_tab, rope_pos);
}

// ... and its RMSNorm state (VR_NORM_PRE_RMS_ROTARY: the Q/K/V projection of a question to a Qwen2-style model)
template <int STEPS, int NW>
__global__ __launch_bounds__(NW * 64) void gemm_f16_skinny_rms_rope_kernel(
    const float* __restrict__ pre, const float* __restrict__ ln_g, float eps, float2* __restrict__ stat_out,
    const half_t* __restrict__ W, int M, int N, int K, float unscale, const float* __restrict__ bias,
    half_t* __restrict__ Ch, const float2* __restrict__ rope_tab, const int32_t* __restrict__ rope_pos) {
  gemm_f16_skinny_ln_body<EPI_ROPE_F16, STEPS, NW, true>(pre, ln_g, nullptr, eps, stat_out, W, M, N, K, unscale, bias, Ch, rope_tab,
                                                        rope_pos);
}

// K = hidden size H: 8 waves x 3 steps (768), 8 x 4 (1024), 4 x 3 (384); anything else keeps the LayerNorm launch
static bool skinny_ln_supported(int M, int N, int K) { return M <= 16 && N % 16 == 0 && (K == 768 || K == 1024 || K == 384); }
// forward_chunk_rms_rotary's: also 4 waves x 7 steps (896, the Qwen2-0.5B body). A test of its own, so that the routes
// of the families that came before do not move.
static bool skinny_rms_rotary_supported(int M, int N, int K) { return skinny_ln_supported(M, N, K) || (M <= 16 && N % 16 == 0 && K == 896); }

// `pre`: the pre-LayerNorm f32 rows, `stat_out`: where block 0 stores their statistics; of `g`: W, bias, Ch, M, N, K,
// ln_g / ln_b (the folded LayerNorm's gain and shift) and, for EPI_ROPE_F16, rope_tab / rope_pos
// rms: the folded norm is RMSNorm by ln_g (EPI_BIAS_F16, EPI_BIAS_RELU, EPI_ROPE_F16 and the two gates)
static int launch_skinny_ln(vr_engine* e, int epi, const float* pre, float eps, float2* stat_out, const GemmArgs& g,
                            bool rms = false) {
  hipStream_t s = e->stream;
  prof_begin(e, VR_PROF_GEMM, 2.0 * g.M * static_cast<double>(g.N) * g.K);
  const dim3 grid(static_cast<unsigned>(g.N / 16));
  auto rms_launch = [&](auto E) {
    auto launch = [&](auto ST, auto NWV) {
      constexpr int kE = decltype(E)::value, kSteps = decltype(ST)::value, kWaves = decltype(NWV)::value;
      if constexpr (kE == EPI_ROPE_F16)  // (a kernel of its own: two arguments more)
        hipLaunchKernelGGL((gemm_f16_skinny_rms_rope_kernel<kSteps, kWaves>), grid, dim3(kWaves * 64), 0, s, pre, g.ln_g, eps,
                           stat_out, g.W.hi, g.M, g.N, g.K, g.W.unscale, g.bias, g.Ch, g.rope_tab, g.rope_pos);
      else
        hipLaunchKernelGGL((gemm_f16_skinny_rms_kernel<kE, kSteps, kWaves>), grid, dim3(kWaves * 64), 0, s, pre, g.ln_g, eps,
                           stat_out, g.W.hi, g.M, g.N, g.K, g.W.unscale, g.bias, g.Ch);
    };
    if (g.K == 768) launch(std::integral_constant<int, 3>{}, std::integral_constant<int, 8>{});
    else if (g.K == 1024) launch(std::integral_constant<int, 4>{}, std::integral_constant<int, 8>{});
    else if (g.K == 896) launch(std::integral_constant<int, 7>{}, std::integral_constant<int, 4>{});
    else launch(std::integral_constant<int, 3>{}, std::integral_constant<int, 4>{});
  };
  const bool known = rms ? with_epi<EPI_BIAS_F16, EPI_BIAS_RELU, EPI_ROPE_F16, EPI_SWIGLU_F16, EPI_GEGLU_F16>(epi, rms_launch) :
                     with_epi<EPI_BIAS_F16, EPI_BIAS_GELU, EPI_ROPE_F16, EPI_SWIGLU_F16, EPI_GEGLU_F16>(epi, [&](auto E) {
    auto launch = [&](auto ST, auto NWV) {
      constexpr int kE = decltype(E)::value, kSteps = decltype(ST)::value, kWaves = decltype(NWV)::value;
      if constexpr (kE == EPI_ROPE_F16)  // (a kernel of its own: two arguments more)
        hipLaunchKernelGGL((gemm_f16_skinny_ln_rope_kernel<kSteps, kWaves>), grid, dim3(kWaves * 64), 0, s, pre, g.ln_g, g.ln_b,
                           eps, stat_out, g.W.hi, g.M, g.N, g.K, g.W.unscale, g.bias, g.Ch, g.rope_tab, g.rope_pos);
      else
        hipLaunchKernelGGL((gemm_f16_skinny_ln_kernel<kE, kSteps, kWaves>), grid, dim3(kWaves * 64), 0, s, pre, g.ln_g, g.ln_b,
                           eps, stat_out, g.W.hi, g.M, g.N, g.K, g.W.unscale, g.bias, g.Ch);
    };
    if (g.K == 768) launch(std::integral_constant<int, 3>{}, std::integral_constant<int, 8>{});
    else if (g.K == 1024) launch(std::integral_constant<int, 4>{}, std::integral_constant<int, 8>{});
    else launch(std::integral_constant<int, 3>{}, std::integral_constant<int, 4>{});
  });
  prof_end(e);
  VR_CHECK(known, "epilogue %d does not exist for the skinny GEMM with a folded LayerNorm (M=%d N=%d K=%d)", epi, g.M, g.N,
           g.K);
  VR_HIP(hipGetLastError());
  return 0;
}

// whether launch_gemm_f16x3 sends an f16-mode product of this shape to one of the skinny kernels (its two tests below)
static bool skinny_routed(int M, int N, int K) {
  const int sk_waves = K % 256 == 0 ? 8 : K % 128 == 0 ? 4 : 0;
  const int sk_steps = sk_waves ? K / (32 * sk_waves) : 0;
  const bool one_launch = sk_steps > 0 && (sk_steps % 6 == 0 || sk_steps % 4 == 0 || sk_steps % 3 == 0) && N % 16 == 0;
  return M <= 4 * kSkinnyM && (one_launch || (skinny_slice(K) > 0 && N % 64 == 0));
}

// the skinny kernels (skinny_apply) exist for these
#define VR_SKINNY_EPIS \
  EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESIDUAL, EPI_BIAS_F16, EPI_BIAS_RESIDUAL_LN, EPI_ROPE_F16, EPI_SWIGLU_F16, EPI_GEGLU_F16, \
      EPI_BIAS_RELU

// g.passes = 3: operands are interleaved (hi, lo) rows (A_lo = A + 8, W.lo = W.hi + 8); 1: plain f16 rows, A_lo / W.lo
// unused. enc: the model whose forward pass this is (its split-K scratch and graph cache)
static int launch_gemm_f16x3(vr_engine* e, Encoder* enc, int epi, const GemmArgs& g) {
  const int M = g.M, N = g.N, K = g.K, passes = g.passes;
  VR_CHECK(N % 4 == 0 && K % HBK_ == 0, "GEMM shape N=%d K=%d: N must be a multiple of 4, K of %d", N, K, HBK_);
  if (M <= 0) return 0;
  hipStream_t s = e->stream;
  // EPI_ROPE_F16 (skinny kernels only): their ln_stat / ln_g parameters carry the cos/sin table and the int32 positions
  // (skinny_apply casts the positions back) — the one place where the two meet
  const float2* k_stat = epi == EPI_ROPE_F16 ? g.rope_tab : g.ln_stat;
  const float* k_g = epi == EPI_ROPE_F16 ? reinterpret_cast<const float*>(g.rope_pos) : g.ln_g;
  bool known = false;  // whether the kernel this product goes to exists for `epi`
  prof_begin(e, VR_PROF_GEMM, 2.0 * M * static_cast<double>(N) * K);
  // one-launch skinny kernel: 8 waves per block when an eighth of K is whole 32-deep MFMA steps, else 4;
  // UNR = steps whose loads are issued together (the largest of 6, 4, 3 dividing the wave's step count)
  const int sk_waves = K % 256 == 0 ? 8 : K % 128 == 0 ? 4 : 0;
  const int sk_steps = sk_waves ? K / (32 * sk_waves) : 0;
  const int sk_unr = sk_steps == 0 ? 0 : sk_steps % 6 == 0 ? 6 : sk_steps % 4 == 0 ? 4 : sk_steps % 3 == 0 ? 3 : 0;
  if (passes == 1 && M <= 4 * kSkinnyM && sk_unr > 0 && N % 16 == 0) {
    const dim3 sg(static_cast<unsigned>(N / 16), static_cast<unsigned>((M + kSkinnyM - 1) / kSkinnyM));
    known = with_epi<VR_SKINNY_EPIS>(epi, [&](auto E) {
      auto launch = [&](auto U, auto W) {
        constexpr int kWaves = decltype(W)::value;
        hipLaunchKernelGGL((gemm_f16_skinny1_kernel<decltype(E)::value, decltype(U)::value, kWaves>), sg, dim3(kWaves * 64), 0, s,
                           g.A, g.W.hi, M, N, K, g.W.unscale, g.bias, g.R, k_stat, k_g, g.ln_b, g.C, g.Ch);
      };
      auto by_unr = [&](auto W) {
        if (sk_unr == 6) launch(std::integral_constant<int, 6>{}, W);
        else if (sk_unr == 4) launch(std::integral_constant<int, 4>{}, W);
        else launch(std::integral_constant<int, 3>{}, W);
      };
      if (sk_waves == 8) by_unr(std::integral_constant<int, 8>{});
      else by_unr(std::integral_constant<int, 4>{});
    });
  } else if (passes == 1 && M <= 4 * kSkinnyM && skinny_slice(K) > 0 && N % 64 == 0) {  // K % 128 != 0: split-K, two launches
    const int kslice = skinny_slice(K), slices = K / kslice;
    {
      const float* before = enc->skinny_ws.p;
      VR_TRY(enc->skinny_ws.grow(static_cast<int64_t>(slices) * M * N, 0, s));
      if (enc->skinny_ws.p != before) invalidate_graphs(enc);  // (never during a capture: a shape runs eagerly first)
    }
    hipLaunchKernelGGL(gemm_f16_skinny_kernel, dim3(static_cast<unsigned>(N / 64), static_cast<unsigned>(slices), static_cast<unsigned>((M + kSkinnyM - 1) / kSkinnyM)),
                       dim3(256), 0, s, g.A, g.W.hi, enc->skinny_ws.p, M, N, K, kslice);
    const unsigned eb = static_cast<unsigned>((static_cast<int64_t>(M) * N / 4 + 255) / 256);
    known = with_epi<VR_SKINNY_EPIS>(epi, [&](auto E) {
      hipLaunchKernelGGL((skinny_epilogue_kernel<decltype(E)::value>), dim3(eb), dim3(256), 0, s, enc->skinny_ws.p, slices, M, N,
                         g.W.unscale, g.bias, g.R, k_stat, k_g, g.ln_b, g.C, g.Ch);
    });
  } else if (passes == 1 || (N % GBN == 0 && K % GBK == 0 && M >= GBM)) {
    static int n_cu = 0;  // persistent grid: one block per CU (the kernel uses 128 KiB of the CU's LDS)
    if (n_cu == 0) {
      hipDeviceProp_t prop;
      VR_HIP(hipGetDeviceProperties(&prop, e->device));
      n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount / 8 * 8 : 256;
      if (n_cu == 0) n_cu = prop.multiProcessorCount;
    }
    const int tiles = ((M + GBM - 1) / GBM) * ((N + GBN - 1) / GBN);
    const int grid256 = std::min(tiles, n_cu);
    if (passes == 1 && mid_usable(M, N, K, n_cu))  // mid-size M: 128x128 tiles (gemm_f16_mid_kernel)
      known = launch_mid(epi, s, g);
    else if (passes == 1 && pp_usable(N, K))  // the ping-pong main loop (gemm_f16_pp_kernel)
      known = launch_pp(epi, grid256, s, g);
    else if (passes == 1)
      known = launch_256<1>(epi, grid256, s, g);
    else
      known = launch_256<3>(epi, grid256, s, g);
  } else {
    VR_CHECK(N % HBN_ == 0, "GEMM shape N=%d must be a multiple of %d", N, HBN_);
    const int grid = ((M + HBM_ - 1) / HBM_) * (N / HBN_);
    known = with_epi<EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESIDUAL, EPI_BIAS_RELU>(epi, [&](auto E) {
      hipLaunchKernelGGL((gemm_f16x3_kernel<decltype(E)::value>), dim3(grid), dim3(256), 0, s, g.A, g.A_lo, g.W.hi, g.W.lo, g.bias,
                         g.R, g.C, g.Ch, g.Cl, M, N, K, g.W.unscale);
    });
  }
  prof_end(e);
  VR_CHECK(known, "epilogue %d does not exist for the kernel of this product (M=%d N=%d K=%d passes=%d)", epi, M, N, K, passes);
  VR_HIP(hipGetLastError());
  return 0;
}
#undef VR_SKINNY_EPIS

// ---- attention -----------------------------------------------------------------------------------

// Sliding-window attention (vr_bert_desc.window = w > 0 on a windowed layer): query i sees key j of its own sequence iff
// |i - j| <= w. The three kernels below take `window` (0: none) and mask the logits outside it to -inf exactly as they
// mask keys behind the sequence's end. WIN, a template flag the host sets to window > 0, makes the argument a
// compile-time 0 for every other launch: those instantiate the code they ran before there was a window (with the
// bounds and the guard below as run-time values the staged kernel, 11 % of an indexing step, ran about 4 % slower in
// one A/B of the contract benchmark; those lines were not kept).
// One unsigned compare per logit: key - (q - w) <= 2w; without a window the bound is UINT_MAX and every key passes.
struct WindowMask {
  int lo;
  unsigned span;
  __device__ __forceinline__ WindowMask(int q, int window)
      : lo(window > 0 ? q - window : 0), span(window > 0 ? 2u * static_cast<unsigned>(window) : 0xffffffffu) {}
  __device__ __forceinline__ bool sees(int key) const { return static_cast<unsigned>(key - lo) <= span; }
  // the causal mask (kMaskCausal below) is the same compare: lo = 0, span = q is key <= q
  struct Causal {};
  __device__ __forceinline__ WindowMask(int q, Causal) : lo(0), span(static_cast<unsigned>(q)) {}
};
// With a window a query can meet a 64-key tile none of whose keys it sees — and that can be the FIRST tile it meets (the
// last queries of a block against the block's first key tile; query tiles are skipped per wave where the whole tile lies
// outside, but inside a tile that some query of the wave sees, others may see nothing). Its running maximum is then
// still -inf, and exp(s - m) = exp(-inf + inf) is NaN. The value the exponentials SUBTRACT is therefore 0 while the
// maximum is -inf: every p is exp(-inf) = 0, the rescale factor exp(-inf - 0) = 0 multiplies sums that are 0 anyway.
// Only the subtrahend is guarded: the running maximum a kernel keeps stays -inf (m = m_raw), so the first tile with a
// visible key rescales by exp(-inf - finite) = 0 and subtracts that tile's own maximum — a 0 stored back as the maximum
// would floor every later base at 0, and logits far below 0 (P rounds to f16 zero below about -17) would lose the row.
__device__ __forceinline__ float softmax_base(float m_raw) { return m_raw == -__builtin_inff() ? 0.0f : m_raw; }

// An additive bias by relative offset (vr_encoder_set_attention_bias): the logit of query i against key j of head h
// gains table[h][clamp(j - i, -radius, radius) + radius]. BIAS, a template flag the host sets like WIN, keeps every
// launch without a table on the code it ran before; a bias and a window never meet (a window needs pre-norm, the bias
// post-norm), so <WIN = false, BIAS = kBiasTable> is the one new instantiation of each kernel. A block works on one head: it
// stages that head's 2 radius + 1 floats in LDS once, ahead of a barrier it takes anyway (`mul`: log2(e) in the two f16
// kernels, whose softmax runs in the log2 domain, so that no logit pays a multiply for it). A lane then holds, per
// query, the row's origin radius - q and reads entry clamp(origin + key, 0, 2 radius): an add, a clamp and an LDS read
// per logit, in f32, ahead of the key-validity mask and the running maximum. Queries and keys behind the sequence's
// end index inside the row like any other (the clamp), and their logits are masked or never stored.
constexpr int kMaxBiasRadius = 512;
__device__ __forceinline__ void stage_bias(float* sB, const float* __restrict__ table, int head, int radius, float mul,
                                           int tid, int n_threads) {
  const int n = 2 * radius + 1;
  for (int i = tid; i < n; i += n_threads) sB[i] = table[static_cast<int64_t>(head) * n + i] * mul;
}
struct BiasRow {
  const float* row;
  int origin, last;
  __device__ __forceinline__ BiasRow(const float* sB, int q, int radius) : row(sB), origin(radius - q), last(2 * radius) {}
  __device__ __forceinline__ float at(int key) const { return row[min(max(origin + key, 0), last)]; }
};
// The two f16 kernels: a 64-key tile's logits of the 16-query tile at qt0 into the log2 domain, with their bias (lane
// (q, g) holds keys kt + 16 t + 4 g + r). A tile that lies `radius` keys or more to one side of every query of the
// tile — most tiles of a long sequence — has one bias for all its logits: one LDS read instead of sixteen
// (wave-uniform: qt0, kt and the radius are).
__device__ __forceinline__ void bias_tile(f32x4 (&st)[4], float scale2, const BiasRow& br, int kt, int g, int qt0) {
  const int radius = br.last >> 1;
  const bool after = kt - (qt0 + 15) >= radius, before = qt0 - (kt + 63) >= radius;
  if (after || before) {
    const float far = br.row[after ? br.last : 0];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) st[t][r] = fmaf(st[t][r], scale2, far);
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) st[t][r] = fmaf(st[t][r], scale2, br.at(kt + t * 16 + 4 * g + r));
  }
}

// A linear bias (vr_encoder_set_attention_slopes, ALiBi): the logit of query i against key j of head h loses
// slope[h] |j - i|, at any distance. The third state of BIAS; like the table it never meets a window, so
// <WIN = false, BIAS = kBiasSlopes> is one more instantiation of each kernel and the other two states compile to what
// they did. The kernels take the slopes where they take the table (`bias_table`: [heads] f32 then, `bias_radius`
// unused). Nothing is staged: a block works on one head, so the slope is one block-uniform value, and the bias is
// arithmetic on the key index. A lane's keys inside a 64-key tile are kt + 16 t + 4 g + r, so the tile costs one
// int -> float conversion, of kt + 4 g - q, and every logit a constant add on top of it.
// The f32 kernel keeps the distance exact (whole numbers below 2^24) and rounds once, in fmaf(|d|, -slope, s scale).
// The two f16 kernels, whose softmax VALU work bounds them, spend an add and an fma per logit (both packed, two logits
// an instruction) and the modulus where an unbiased tile spends one multiply: they carry the distance pre-multiplied
// by the slope (in the log2 domain, as the table is),
// d' = slope2 (kt + 4 g - q) + slope2 16 t + slope2 r with the six products block-uniform loop invariants (six
// registers; the sixteen of slope2 (16 t + r) took the streamed kernel from three waves per SIMD to two), and the
// logit is fmaf(s, scale2, -|d'|) (slope >= 0, so slope |d| = |slope d|; the sign is a source modifier of the packed
// fma, the modulus is not: one v_and_b32 per logit). Against the exact form that is three roundings more, each
// 2^-24 of a bias whose logit weighs 2^-bias: far below what the f16 rounding of P leaves. Applied ahead of the
// key-validity mask and the running maximum, for padded queries and in the CLS tail alike, exactly where the table is.
constexpr int kBiasNone = 0, kBiasTable = 1, kBiasSlopes = 2;
// A causal mask (vr_bert_desc_v2.causal, VR_NORM_PRE_RMS_ROTARY only: the decoder-style embedders): query i sees key j of
// its own sequence iff j <= i — an additive bias of 0 or -inf by relative offset, and the fourth state of BIAS_KIND. It
// meets neither a window nor a table nor slopes (build_encoder and the two setters refuse them under that norm), so
// <WIN = false, BIAS_KIND = kMaskCausal> is one more instantiation of each kernel, and the other states keep their names
// and their code. The mask is WindowMask's compare (lo = 0, span = q) beside the key-validity test. What it buys is the
// key loop's end: a 64-key tile that starts behind a query tile's (a block's) last query is never visited — half the
// tiles of a long sequence. The loop bounds are block-uniform where a barrier sits inside the loop (attention_kernel,
// attention_stream_kernel) and wave-uniform elsewhere. Every tile a query DOES meet starts at or before it (tiles start
// at multiples of 64, query tiles at multiples of 16, a streamed wave's pair of tiles at a multiple of 32, and the loops
// end at the tile that holds the diagonal), so it sees the tile's first key and its maximum is finite; the
// softmax_base guard is kept all the same, it costs one compare per tile and query.
constexpr int kMaskCausal = 3;
__device__ __forceinline__ void slope_tile(f32x4 (&st)[4], float scale2, float slope2, int kt, int g, int q) {
  const float d0 = slope2 * static_cast<float>(kt + 4 * g - q);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const float dt = d0 + slope2 * static_cast<float>(16 * t);
#pragma unroll
    for (int r = 0; r < 4; ++r) st[t][r] = fmaf(st[t][r], scale2, -fabsf(dt + slope2 * static_cast<float>(r)));
  }
}

// (attention_kernel<128, ...>: the bytes of its K and V tiles, dynamic LDS — see the kernel)
constexpr size_t kAttnF32Lds128 = 2 * 64 * (128 + 4) * sizeof(float);
// One block = 64 queries of one (sequence, head); wave w owns queries 16w..16w+15.
// S^T = K Q^T is computed with keys on the MFMA rows, so a lane (q = lane & 15, g = lane >> 4)
// ends up holding the logits of query q against keys 4g..4g+3 of each 16-key tile: exactly the B
// operand layout of the following O^T += V^T P^T product — no transpose, no LDS round trip for P.
template <int DH, bool WIN, int BIAS_KIND>
__global__ __launch_bounds__(256) void attention_kernel(const float* __restrict__ qkv,
                                                        const int32_t* __restrict__ cu, int seq0,
                                                        int tok_base, int H, int qblocks, float scale,
                                                        float* __restrict__ ctx, half_t* __restrict__ ctx_hi,
                                                        half_t* __restrict__ ctx_lo, int window_arg,
                                                        const float* __restrict__ bias_table, int bias_radius) {
  constexpr bool BIAS = BIAS_KIND == kBiasTable, SLOPES = BIAS_KIND == kBiasSlopes, CAUSAL = BIAS_KIND == kMaskCausal;
  static_assert(!(WIN && BIAS_KIND != kBiasNone), "a window needs pre-norm, a bias post-norm");
  const int window = WIN ? window_arg : 0;
  constexpr int LDK = DH + 4;
  constexpr int NS = DH / 16;  // 16-wide d blocks
  // (d_h = 128: two tiles of 64 x 132 floats are 67,584 bytes, above the 64 KiB a kernel may declare: that
  // instantiation alone takes them as dynamic LDS, kAttnF32Lds128 bytes that launch_attention asks for)
  float *sK, *sV;
  if constexpr (DH == 128) {
    extern __shared__ __attribute__((aligned(16))) float att_f32_lds[];
    sK = att_f32_lds;
    sV = att_f32_lds + 64 * LDK;
  } else {
    __shared__ float sK_tile[64 * LDK];
    __shared__ float sV_tile[64 * LDK];
    sK = sK_tile;
    sV = sV_tile;
  }
  const int seq = seq0 + blockIdx.x / qblocks;
  const int qb = blockIdx.x % qblocks;
  const int head = blockIdx.y;
  const int t0 = cu[seq] - tok_base;
  const int len = cu[seq + 1] - cu[seq];
  if (qb * 64 >= len) return;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int qi = lane & 15, g = lane >> 4;
  const int q_tok = qb * 64 + wave * 16 + qi;
  float* sB = nullptr;
  if constexpr (BIAS) {
    __shared__ float bias_lds[2 * kMaxBiasRadius + 1];
    sB = bias_lds;
    stage_bias(sB, bias_table, head, bias_radius, 1.0f, tid, 256);  // (read behind the key loop's first barriers)
  }
  const BiasRow br(sB, q_tok, BIAS ? bias_radius : 0);
  const float neg_slope = SLOPES ? -bias_table[head] : 0.0f;
  const bool q_valid = q_tok < len;
  const int64_t row3 = 3 * static_cast<int64_t>(H);

  float4 qf[NS];
  {
    const float* qp = qkv + (t0 + (q_valid ? q_tok : len - 1)) * row3 + head * DH + 4 * g;
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = *reinterpret_cast<const float4*>(qp + 16 * s);
  }
  f32x4 o[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) o[s] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -__builtin_inff();
  float l = 0.0f;
  const WindowMask wm = [&] {
    if constexpr (CAUSAL) return WindowMask(q_tok, WindowMask::Causal{});
    else return WindowMask(q_tok, window);
  }();

  // CAUSAL: the tiles up to the one that holds the block's 64 queries (block-uniform: barriers inside)
  const int kt_end = CAUSAL ? min(len, qb * 64 + 64) : len;
  for (int kt = 0; kt < kt_end; kt += 64) {
    __syncthreads();
    for (int idx = tid; idx < 64 * (DH / 4); idx += 256) {
      const int key = idx / (DH / 4), c4 = idx % (DH / 4);
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (kt + key < len) {
        const float* p = qkv + (t0 + kt + key) * row3 + H + head * DH + c4 * 4;
        kv = *reinterpret_cast<const float4*>(p);
        vv = *reinterpret_cast<const float4*>(p + H);
      }
      *reinterpret_cast<float4*>(sK + key * LDK + c4 * 4) = kv;
      *reinterpret_cast<float4*>(sV + key * LDK + c4 * 4) = vv;
    }
    __syncthreads();

    f32x4 st[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const float4 kf = *reinterpret_cast<const float4*>(sK + (t * 16 + qi) * LDK + 16 * s + 4 * g);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.x, qf[s].x, st[t], 0, 0, 0);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.y, qf[s].y, st[t], 0, 0, 0);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.z, qf[s].z, st[t], 0, 0, 0);
        st[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.w, qf[s].w, st[t], 0, 0, 0);
      }
    }
    float mx = -__builtin_inff();
    if constexpr (SLOPES) {  // (scaled and biased here; the loop below then takes the logits as they are)
      const float d0 = static_cast<float>(kt + 4 * g - q_tok);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) st[t][r] = fmaf(fabsf(d0 + static_cast<float>(16 * t + r)), neg_slope, st[t][r] * scale);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kt + t * 16 + 4 * g + r;
        const float v = key < len && wm.sees(key) ? (BIAS ? st[t][r] * scale + br.at(key) : SLOPES ? st[t][r] : st[t][r] * scale)
                                                  : -__builtin_inff();
        st[t][r] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_raw = fmaxf(m, mx);  // (no window: finite, key kt < len is always valid)
    const float m_new = WIN || CAUSAL ? softmax_base(m_raw) : m_raw;  // what the exponentials subtract; the maximum kept is m_raw
    const float alpha = expf(m - m_new);
    float psum = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = expf(st[t][r] - m_new);
        st[t][r] = p;
        psum += p;
      }
    l = l * alpha + psum;
    m = m_raw;
#pragma unroll
    for (int s = 0; s < NS; ++s) o[s] *= alpha;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* vrow = sV + (t * 16 + 4 * g + r) * LDK + qi;
#pragma unroll
        for (int s = 0; s < NS; ++s)
          o[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(vrow[16 * s], st[t][r], o[s], 0, 0, 0);
      }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (q_valid) {
    const float inv = 1.0f / l;
    const int64_t off = static_cast<int64_t>(t0 + q_tok) * H + head * DH + 4 * g;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      float4 v = make_float4(o[s][0] * inv, o[s][1] * inv, o[s][2] * inv, o[s][3] * inv);
      if (ctx_hi) {  // f16x3 mode: the only consumer is the output-projection GEMM
        half_t h[4], lo[4];
        split_f16(v.x, h[0], lo[0]);
        split_f16(v.y, h[1], lo[1]);
        split_f16(v.z, h[2], lo[2]);
        split_f16(v.w, h[3], lo[3]);
        if (ctx_lo) {
          const int64_t so = static_cast<int64_t>(t0 + q_tok) * (2 * H) + split_at(head * DH + 4 * g + 16 * s);
          *reinterpret_cast<uint2*>(ctx_hi + so) = *reinterpret_cast<const uint2*>(h);
          *reinterpret_cast<uint2*>(ctx_lo + so) = *reinterpret_cast<const uint2*>(lo);
        } else {  // plain f16 rows (VR_PRECISION_F16)
          *reinterpret_cast<uint2*>(ctx_hi + off + 16 * s) = *reinterpret_cast<const uint2*>(h);
        }
      } else {
        *reinterpret_cast<float4*>(ctx + off + 16 * s) = v;
      }
    }
  }
}

// The same attention on the f16 matrix pipe (VR_PRECISION_F16): Q (pre-scaled by 1/sqrt(d_h)), K, V and
// the probabilities P are rounded to f16, every product accumulates in f32, the softmax stays f32.
// v_mfma_f32_16x16x32_f16 has the C layout of the 16x16x4 instruction, so the structure above
// carries over: S^T = K Q^T leaves lane (q, g) with the logits of keys 16t + 4g + r — and the B
// operand of O^T += V^T P^T wants 8 k-slots per lane, so a 32-key step takes its slots in the order
// (g, tile parity, r): slot 8g + 4b + r = key 32u + 16b + 4g + r. 16 MFMAs of 16 cycles per 64 keys and
// 16-query tile against 128 of 32 cycles in the f32 kernel: the softmax's VALU work is what bounds it.
// Two kernels: attention_seq_kernel while a sequence's K and V fit a workgroup's LDS, attention_stream_kernel beyond.

// ---- attention, one block per (sequence, head) -------------------------------------------------------------
//
// A kernel that stages 64 keys at a time, once per 64-query block, pays four staging phases per (sequence, head) on the
// ~118-token chunks of the indexing path, each with its global-load latency exposed (the first f16 kernel did, and
// transposed its V tile through LDS by hand: it ran at half of what its 1.6 GB per launch cost at the HBM rate).
// Here the block stages the sequence's K and V rows ONCE, all loads of up to 128 keys in flight together, V stays
// row-major in LDS and its transposed MFMA operand comes out of ds_read_b64_tr_b16 (lane 4q + p of a 16-lane group
// addresses row q, columns 4p..4p+3 of a 4 x 16 block; lane i receives column i); the four waves then walk the
// sequence's 16-query tiles (wave w: tiles w, w + 4, ...) against keys already in LDS. Logits on the f16 MFMA, online
// softmax in the log2 domain over 64-key tiles, P as f16.
// `q_limit`: only queries below it are computed (the last layer of a CLS-pooled model needs token 0 only).
typedef short s16x4 __attribute__((ext_vector_type(4)));

template <int DH, int NW, bool WIN, int BIAS_KIND>
__global__ __launch_bounds__(NW * 64) void attention_seq_kernel(const half_t* __restrict__ qkv, const int32_t* __restrict__ cu,
                                                            int seq0, int tok_base, int H, float scale, int q_limit,
                                                            int lds_keys, half_t* __restrict__ ctx_h, int window_arg,
                                                            const float* __restrict__ bias_table, int bias_radius) {
  constexpr bool BIAS = BIAS_KIND == kBiasTable, SLOPES = BIAS_KIND == kBiasSlopes, CAUSAL = BIAS_KIND == kMaskCausal;
  static_assert(!(WIN && BIAS_KIND != kBiasNone), "a window needs pre-norm, a bias post-norm");
  const int window = WIN ? window_arg : 0;
  constexpr int LDK = DH;       // halfs per staged row: unpadded, 16-byte chunks XOR-swizzled by the row instead
  constexpr int CH = DH / 8;    // 16-byte chunks per row
  // chunk c of K row r sits at c ^ kswz(r): the 16 rows x one chunk of a ds_read_b128 fragment read then cover all 64
  // banks once; chunk c of V row r at c ^ vswz(r): the 8 rows x 32 bytes of a transposed read (per 32-lane half) do
  // d_h = 128: a row is 256 bytes, the whole bank row (bank = (a / 4) mod 64 for both reads), so every row starts at
  // bank 0 and the chunk position alone decides the banks: position p covers banks 4p .. 4p + 3.
  //  K: lane (qi, g) reads chunk 4u + g of row 16t + qi, and a ds_read_b128 is served in four 16-lane groups, lanes
  //  {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32: in each, qi takes all 16 values once, g one value on
  //  the eight lanes qi in {0-3, 12-15} and its neighbour g ^ 1 on the eight qi in {4-11}. kswz(r) = r & 15 puts the
  //  lane at position (4u + g) ^ qi: the first eight cover (4u + g) ^ {0-3, 12-15}, the others (4u + g) ^ 1 ^ {4-11} =
  //  (4u + g) ^ {4-11} (x ^ 1 maps {4-11} onto itself) — all 16 positions, every bank once.
  //  V: a transposed read is served per 32-lane half: 8 rows (4g + q, g in {0, 1} or {2, 3}: 0-7 or 8-15, behind a
  //  multiple of 16) x the chunk pair (2s, 2s + 1) of each, 32 bytes. The swizzle must keep a pair together (bit 0
  //  clear) and send the eight rows to eight different pairs: vswz(r) = (r & 7) << 1, pair s ^ (r & 7) — 8 x 32 bytes
  //  over 256, every bank once. It depends on (4g + q) & 7 alone, as tr_sw below assumes.
  //  The 16-byte stores are served in groups of 8 neighbouring lanes with bank = (a / 4) mod 32: the 8 chunks of one
  //  half row, which either swizzle sends to the 8 positions of one half row again (bit 3 of the swizzle picks the
  //  half, bits 0-2 permute inside it) — 128 bytes, 32 banks once.
  auto kswz = [](int r) { return DH == 128 ? r & 15 : DH == 64 ? (r >> 1) & 7 : (r >> 1) & 3; };
  auto vswz = [](int r) { return DH == 128 ? (r & 7) << 1 : DH == 64 ? ((r >> 1) & 3) << 1 : ((r >> 2) & 1) << 1; };
  constexpr int NS = DH / 16;   // 16-wide d blocks of the output
  constexpr int NKB = DH / 32;  // 32-deep MFMA steps over d
  extern __shared__ __attribute__((aligned(16))) half_t att_lds[];
  half_t* sK = att_lds;
  half_t* sV = att_lds + static_cast<size_t>(lds_keys) * LDK;
  // BIAS: the head's table behind V (the host adds its bytes to the launch's LDS; 4 lds_keys DH bytes in, 16-aligned)
  float* sB = BIAS ? reinterpret_cast<float*>(att_lds + static_cast<size_t>(2) * lds_keys * LDK) : nullptr;
  // heads fastest: the twelve 128-byte slices of a token's Q/K/V row are then fetched by blocks that run side by side —
  // one DRAM page opened once — instead of 2200 blocks apart (sequence-fastest order: 3.2 TB/s of 128-byte reads)
  const int n_heads = H / DH;
  const int seq = seq0 + static_cast<int>(blockIdx.x) / n_heads;
  const int head = static_cast<int>(blockIdx.x) % n_heads;
  const int t0 = cu[seq] - tok_base;
  const int len = cu[seq + 1] - cu[seq];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = lane & 15, g = lane >> 4;
  const int64_t row3 = 3 * static_cast<int64_t>(H);
  // keys are staged and multiplied in groups of 16 (one MFMA tile): a 140-token sequence costs 9 groups, not 3 x 4
  const int keys_pad = min((len + 15) & ~15, lds_keys);  // (len <= lds_keys: the host sizes the LDS by the longest sequence)

  const int q_end = min(len, q_limit);
  // Q rows go straight to registers; a wave's first tile is requested before the K/V loads, every further one while
  // the tile before it is computed
  auto load_q = [&](int qt, f16x8 (&q)[NKB]) {
    const int tok = min(qt * 16 + qi, len - 1);
    const half_t* qp = qkv + (t0 + tok) * row3 + head * DH + 8 * g;
#pragma unroll
    for (int u = 0; u < NKB; ++u) q[u] = *reinterpret_cast<const f16x8*>(qp + 32 * u);
  };
  f16x8 qf[NKB];
  if (wave * 16 < q_end) load_q(wave, qf);
  // stage K and V rows 0 .. keys_pad - 1 (zeros behind the sequence's end), up to 128 keys' loads in flight at once
  const int total = keys_pad * CH;
  constexpr int NT = NW * 64;
  constexpr int NST = 20 / NW;  // 16-byte loads of K and of V per thread and round: 160 keys of 64 dims in one round
  for (int base = 0; base < total; base += NST * NT) {
    uint4 kv[NST], vv[NST];
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int idx = base + i * NT + tid;
      const int key = idx / CH, c8 = idx % CH;
      kv[i] = vv[i] = make_uint4(0, 0, 0, 0);
      if (idx < total && key < len) {
        const half_t* p = qkv + (t0 + key) * row3 + H + head * DH + c8 * 8;
        kv[i] = *reinterpret_cast<const uint4*>(p);
        vv[i] = *reinterpret_cast<const uint4*>(p + H);
      }
    }
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int idx = base + i * NT + tid;
      const int key = idx / CH, c8 = idx % CH;
      if (idx < total) {
        *reinterpret_cast<uint4*>(sK + key * LDK + (c8 ^ kswz(key)) * 8) = kv[i];
        *reinterpret_cast<uint4*>(sV + key * LDK + (c8 ^ vswz(key)) * 8) = vv[i];
      }
    }
  }
  if constexpr (BIAS) stage_bias(sB, bias_table, head, bias_radius, 1.4426950408889634f, tid, NT);
  __syncthreads();

  const float scale2 = scale * 1.4426950408889634f;  // logits in the log2 domain: the softmax uses v_exp_f32 directly
  const float slope2 = SLOPES ? bias_table[head] * 1.4426950408889634f : 0.0f;  // (block-uniform)
  // transposed V reads: lane 4q + p of its 16-lane group -> row (key) q, columns 4p .. 4p + 3 of the block
  // (block rows are key0 + q with key0 a multiple of 4: the swizzle of the row depends on 4 g + q alone)
  const int tr_q = (lane & 15) >> 2, tr_p = lane & 3;
  const int tr_row = tr_q * LDK, tr_sw = vswz(4 * g + tr_q), tr_in = 4 * (tr_p & 1);
  const int k_sw = kswz(qi);  // rows kt + 16 t + qi
  for (int qt = wave; qt * 16 < q_end; qt += NW) {  // wave-uniform: EXEC stays full (the transposed reads need it)
    const int q_tok = qt * 16 + qi;
    const bool q_valid = q_tok < len;
    f16x8 qn[NKB];
    const bool more = (qt + NW) * 16 < q_end;
    if (more) load_q(qt + NW, qn);
    f32x4 o[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) o[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -__builtin_inff();
    float l = 0.0f;
    // a window: only the 64-key tiles that hold a key some query of this tile sees (wave-uniform bounds)
    // (CAUSAL: the tiles up to the one that holds this query tile, and inside it the 16-key groups up to the tile's own)
    const int kt0 = window > 0 ? max(0, qt * 16 - window) & ~63 : 0;
    const int kt1 = CAUSAL ? min(keys_pad, qt * 16 + 16) : window > 0 ? min(keys_pad, qt * 16 + 16 + window) : keys_pad;
    const WindowMask wm = [&] {
      if constexpr (CAUSAL) return WindowMask(q_tok, WindowMask::Causal{});
      else return WindowMask(q_tok, window);
    }();
    const BiasRow br(sB, q_tok, BIAS ? bias_radius : 0);
    for (int kt = kt0; kt < kt1; kt += 64) {
      const int nt = min(4, ((CAUSAL ? kt1 : keys_pad) - kt) >> 4);  // 16-key groups in this tile (block-uniform; CAUSAL: wave-uniform)
      f32x4 st[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (t < nt) {
#pragma unroll
          for (int u = 0; u < NKB; ++u) {
            const f16x8 kf = *reinterpret_cast<const f16x8*>(sK + (kt + t * 16 + qi) * LDK + ((4 * u + g) ^ k_sw) * 8);
            st[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[u], st[t], 0, 0, 0);
          }
        }
      }
      float mx = -__builtin_inff();
      // BIAS: scaled and biased ahead of both branches, which then take the logits as they are (a factor of 1)
      if constexpr (BIAS) bias_tile(st, scale2, br, kt, g, qt * 16);
      if constexpr (SLOPES) slope_tile(st, scale2, slope2, kt, g, q_tok);
      const float sc = BIAS || SLOPES ? 1.0f : scale2;
      // every key of the tile exists and every query of the tile sees all of them: no masks
      if (kt + 64 <= len && (!CAUSAL || kt + 63 <= qt * 16) &&
          (window <= 0 || (kt + 63 - qt * 16 <= window && qt * 16 + 15 - kt <= window))) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            st[t][r] *= sc;
            mx = fmaxf(mx, st[t][r]);
          }
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = kt + t * 16 + 4 * g + r;
            const float v = key < len && wm.sees(key) ? st[t][r] * sc : -__builtin_inff();
            st[t][r] = v;
            mx = fmaxf(mx, v);
          }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float m_raw = fmaxf(m, mx);  // (no window: finite, key kt < len is always valid)
      const float m_new = WIN || CAUSAL ? softmax_base(m_raw) : m_raw;  // what the exponentials subtract; the maximum kept is m_raw
      const float alpha = __builtin_amdgcn_exp2f(m - m_new);
      float psum = 0.0f;
      f16x8 pb[2];  // pb[u][j]: key kt + 32 u + 16 (j >> 2) + 4 g + (j & 3)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f(st[t][r] - m_new);
          psum += p;
          pb[t >> 1][(t & 1) * 4 + r] = static_cast<half_t>(p);
        }
      l = l * alpha + psum;
      m = m_raw;
#pragma unroll
      for (int s = 0; s < NS; ++s) o[s] *= alpha;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          // V^T fragment: d = 16 s + qi, k index 8 g + j <-> the key of pb[u][j]: two 4-key blocks, 16 keys apart
          // (a group behind the staged keys contributes nothing: its P values are zero, its V rows are not read)
          if (2 * u >= nt) continue;
          const half_t* vb = sV + (kt + 32 * u + 4 * g) * LDK + tr_row + ((2 * s + (tr_p >> 1)) ^ tr_sw) * 8 + tr_in;
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vb));
          s16x4 hi = s16x4{0, 0, 0, 0};
          if (2 * u + 1 < nt) hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vb + 16 * LDK));
          f16x8 vf;
          *reinterpret_cast<s16x4*>(&vf) = lo;
          *(reinterpret_cast<s16x4*>(&vf) + 1) = hi;
          o[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pb[u], o[s], 0, 0, 0);
        }
    }
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (q_valid) {
      const float inv = 1.0f / l;
      const int64_t off = static_cast<int64_t>(t0 + q_tok) * H + head * DH + 4 * g;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        half_t h[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = static_cast<half_t>(fminf(fmaxf(o[s][r] * inv, -65504.0f), 65504.0f));
        *reinterpret_cast<uint2*>(ctx_h + off + 16 * s) = *reinterpret_cast<const uint2*>(h);
      }
    }
    if (more) {
#pragma unroll
      for (int u = 0; u < NKB; ++u) qf[u] = qn[u];
    }
  }
}

// ---- attention, keys streamed through LDS: sequences too long to stage whole ---------------------------------
//
// attention_seq_kernel holds a sequence's K and V in LDS: 640 keys at d_h = 64. Past that the keys stream: one block =
// 128 queries of one (sequence, head), and the sequence's keys pass through LDS in 64-key tiles, K and V row-major with
// the swizzles of attention_seq_kernel (the same ds_read_b128 / ds_read_b64_tr_b16 fragments, a tile's rows taking the
// place of the sequence's). Each wave owns 32 queries as two 16-query tiles held in registers, so every K fragment and
// every transposed V fragment read from LDS feeds two MFMAs. The tiles are double-buffered: tile j + 1's rows are
// requested into registers before tile j's products (CH / NW 16-byte loads of K and of V per thread, all in flight
// together), written to the other buffer behind those products, and one barrier per tile hands it over. Rows behind
// the sequence's end are staged as zeros, their logits masked to -inf before the running maximum. Same arithmetic as
// attention_seq_kernel. Grid: heads fastest, then the 128-query blocks of a sequence (`qblocks` of them per sequence);
// `q_limit` as in attention_seq_kernel — the host launches query block 0 alone for it, and a wave whose queries all
// lie at or behind it stages and takes every barrier but skips the products.
template <int DH, int NW, bool WIN, int BIAS_KIND>
__global__ __launch_bounds__(NW * 64) void attention_stream_kernel(const half_t* __restrict__ qkv, const int32_t* __restrict__ cu,
                                                               int seq0, int tok_base, int H, int qblocks, float scale,
                                                               int q_limit, half_t* __restrict__ ctx_h, int window_arg,
                                                               const float* __restrict__ bias_table, int bias_radius) {
  constexpr bool BIAS = BIAS_KIND == kBiasTable, SLOPES = BIAS_KIND == kBiasSlopes, CAUSAL = BIAS_KIND == kMaskCausal;
  static_assert(!(WIN && BIAS_KIND != kBiasNone), "a window needs pre-norm, a bias post-norm");
  const int window = WIN ? window_arg : 0;
  static_assert(NW == 4 && (DH == 128 || DH == 64 || DH == 32), "one 16-byte piece of a 64-key tile per thread and CH / NW rounds");
  // (d_h = 128: the ring below is 4 x 64 x 128 halfs = 65,536 bytes, exactly the static limit; its two instantiations,
  // kBiasNone and kMaskCausal, put nothing else in LDS — a table would)
  static_assert(DH != 128 || BIAS_KIND == kBiasNone || BIAS_KIND == kMaskCausal, "head size 128 takes no table and no slopes");
  constexpr int LDK = DH;       // halfs per staged row: unpadded, 16-byte chunks XOR-swizzled by the row
  constexpr int CH = DH / 8;    // 16-byte chunks per row
  constexpr int NS = DH / 16;   // 16-wide d blocks of the output
  constexpr int NKB = DH / 32;  // 32-deep MFMA steps over d
  constexpr int NT = NW * 64;
  constexpr int NLD = 64 * CH / NT;  // 16-byte loads of K and of V per thread and tile
  constexpr int TILE = 64 * LDK;     // halfs of one K or V tile
  auto kswz = [](int r) { return DH == 128 ? r & 15 : DH == 64 ? (r >> 1) & 7 : (r >> 1) & 3; };
  auto vswz = [](int r) { return DH == 128 ? (r & 7) << 1 : DH == 64 ? ((r >> 1) & 3) << 1 : ((r >> 2) & 1) << 1; };
  __shared__ __attribute__((aligned(16))) half_t att_tiles[4 * TILE];  // buffer b: K at 2 b TILE, V at (2 b + 1) TILE
  const int n_heads = H / DH;
  const int head = static_cast<int>(blockIdx.x) % n_heads;
  const int sq = static_cast<int>(blockIdx.x) / n_heads;
  const int seq = seq0 + sq / qblocks;
  const int q0 = (sq % qblocks) * (NW * 32);
  const int t0 = cu[seq] - tok_base;
  const int len = cu[seq + 1] - cu[seq];
  if (q0 >= len) return;  // block-uniform, ahead of every barrier
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qi = lane & 15, g = lane >> 4;
  const int64_t row3 = 3 * static_cast<int64_t>(H);
  const int q_end = min(len, q_limit);
  const int qw = q0 + wave * 32;   // the wave's first query
  const bool active = qw < q_end;  // wave-uniform: EXEC stays full inside (the transposed reads need it)
  const bool two = qw + 16 < q_end;  // ... and so is this: the wave's second tile holds a query (not so in the CLS tail)

  f16x8 qf[2][NKB];
  if (active) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const half_t* qp = qkv + (t0 + min(qw + 16 * i + qi, len - 1)) * row3 + head * DH + 8 * g;
#pragma unroll
      for (int u = 0; u < NKB; ++u) qf[i][u] = *reinterpret_cast<const f16x8*>(qp + 32 * u);
    }
  }
  // a tile's rows: requested from a row inside the sequence whatever the key (no branch around a load), zeroed behind
  // the sequence's end when they are written. The registers of a request belong to one iteration of the key loop (a
  // pair carried around the loop is copied, and the copy waits for the loads ahead of the products).
  const half_t* kv_base = qkv + static_cast<int64_t>(t0) * row3 + H + head * DH;
  auto request = [&](int kt, uint4 (&kr)[NLD], uint4 (&vr)[NLD]) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = i * NT + tid;
      const half_t* p = kv_base + min(kt + idx / CH, len - 1) * row3 + (idx % CH) * 8;
      kr[i] = *reinterpret_cast<const uint4*>(p);
      vr[i] = *reinterpret_cast<const uint4*>(p + H);
    }
  };
  auto write = [&](int kt, const uint4 (&kr)[NLD], const uint4 (&vr)[NLD], half_t* sK, half_t* sV) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int idx = i * NT + tid;
      const int key = idx / CH, c8 = idx % CH;
      const bool behind = kt + key >= len;
      *reinterpret_cast<uint4*>(sK + key * LDK + (c8 ^ kswz(key)) * 8) = behind ? make_uint4(0, 0, 0, 0) : kr[i];
      *reinterpret_cast<uint4*>(sV + key * LDK + (c8 ^ vswz(key)) * 8) = behind ? make_uint4(0, 0, 0, 0) : vr[i];
    }
  };
  // a window: the block's 128 queries see keys q0 - w .. q0 + 127 + w only, so the key loop runs over the tiles that
  // hold those — 128 + 2 w keys and a tile's rounding, whatever the sequence's length (block-uniform bounds)
  const int kt0 = window > 0 ? max(0, q0 - window) & ~63 : 0;
  // (CAUSAL: the tiles up to the one that holds the block's last query, block-uniform as well)
  const int kt1 = CAUSAL ? min(len, q0 + NW * 32) : window > 0 ? min(len, q0 + NW * 32 + window) : len;
  {
    uint4 kr[NLD], vr[NLD];
    request(kt0, kr, vr);
    write(kt0, kr, vr, att_tiles, att_tiles + TILE);
  }
  float* sB = nullptr;
  if constexpr (BIAS) {
    __shared__ float bias_lds[2 * kMaxBiasRadius + 1];
    sB = bias_lds;
    stage_bias(sB, bias_table, head, bias_radius, 1.4426950408889634f, tid, NT);
  }
  __syncthreads();

  const float scale2 = scale * 1.4426950408889634f;  // logits in the log2 domain: the softmax uses v_exp_f32 directly
  const float slope2 = SLOPES ? bias_table[head] * 1.4426950408889634f : 0.0f;  // (block-uniform)
  // transposed V reads: lane 4q + p of its 16-lane group -> row (key) q, columns 4p .. 4p + 3 of the block
  const int tr_q = (lane & 15) >> 2, tr_p = lane & 3;
  const int tr_row = tr_q * LDK, tr_sw = vswz(4 * g + tr_q), tr_in = 4 * (tr_p & 1);
  const int k_sw = kswz(qi);  // rows 16 t + qi of the tile
  f32x4 o[2][NS];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int s = 0; s < NS; ++s) o[i][s] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m[2] = {-__builtin_inff(), -__builtin_inff()};
  float l[2] = {0.0f, 0.0f};
  const WindowMask wm[2] = {CAUSAL ? WindowMask(qw + qi, WindowMask::Causal{}) : WindowMask(qw + qi, window),
                            CAUSAL ? WindowMask(qw + 16 + qi, WindowMask::Causal{}) : WindowMask(qw + 16 + qi, window)};
  const BiasRow br[2] = {BiasRow(sB, qw + qi, BIAS ? bias_radius : 0), BiasRow(sB, qw + 16 + qi, BIAS ? bias_radius : 0)};
  int buf = 0;
  for (int kt = kt0; kt < kt1; kt += 64, buf ^= 1) {
    const bool more = kt + 64 < kt1;  // block-uniform
    uint4 kr[NLD], vr[NLD];
    if (more) request(kt + 64, kr, vr);
    // a tile none of the wave's 32 queries sees is skipped (wave-uniform; the wave still stages and takes the barrier)
    // (CAUSAL: a tile behind the wave's last query likewise)
    if (active && (!CAUSAL || kt <= qw + 31) && (window <= 0 || (kt <= qw + 31 + window && kt + 63 >= qw - window))) {
      const half_t* sK = att_tiles + 2 * buf * TILE;
      const half_t* sV = sK + TILE;
      f32x4 st[2][4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        st[0][t] = st[1][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < NKB; ++u) {
          const f16x8 kf = *reinterpret_cast<const f16x8*>(sK + (t * 16 + qi) * LDK + ((4 * u + g) ^ k_sw) * 8);
          st[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[0][u], st[0][t], 0, 0, 0);
          if (two) st[1][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[1][u], st[1][t], 0, 0, 0);
        }
      }
      f16x8 pb[2][2];  // pb[i][u][j]: key kt + 32 u + 16 (j >> 2) + 4 g + (j & 3)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (i == 1 && !two) break;
        float mx = -__builtin_inff();
        const int qt0 = qw + 16 * i;  // the tile's first query
        if constexpr (BIAS) bias_tile(st[i], scale2, br[i], kt, g, qt0);  // (as in attention_seq_kernel)
        if constexpr (SLOPES) slope_tile(st[i], scale2, slope2, kt, g, qt0 + qi);
        const float sc = BIAS || SLOPES ? 1.0f : scale2;
        // every key of the tile exists and every query of the tile sees all of them: no masks
        if (kt + 64 <= len && (!CAUSAL || kt + 63 <= qt0) &&
            (window <= 0 || (kt + 63 - qt0 <= window && qt0 + 15 - kt <= window))) {
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              st[i][t][r] *= sc;
              mx = fmaxf(mx, st[i][t][r]);
            }
        } else {
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int key = kt + t * 16 + 4 * g + r;
              const float v = key < len && wm[i].sees(key) ? st[i][t][r] * sc : -__builtin_inff();
              st[i][t][r] = v;
              mx = fmaxf(mx, v);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_raw = fmaxf(m[i], mx);  // (no window: finite, key kt < len is always valid)
        const float m_new = WIN || CAUSAL ? softmax_base(m_raw) : m_raw;  // what the exponentials subtract; the maximum kept is m_raw
        const float alpha = __builtin_amdgcn_exp2f(m[i] - m_new);
        float psum = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = __builtin_amdgcn_exp2f(st[i][t][r] - m_new);
            psum += p;
            pb[i][t >> 1][(t & 1) * 4 + r] = static_cast<half_t>(p);
          }
        l[i] = l[i] * alpha + psum;
        m[i] = m_raw;
#pragma unroll
        for (int s = 0; s < NS; ++s) o[i][s] *= alpha;
      }
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          // V^T fragment: d = 16 s + qi, k index 8 g + j <-> the key of pb[.][u][j]: two 4-key blocks, 16 keys apart
          const half_t* vb = sV + (32 * u + 4 * g) * LDK + tr_row + ((2 * s + (tr_p >> 1)) ^ tr_sw) * 8 + tr_in;
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vb));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vb + 16 * LDK));
          f16x8 vf;
          *reinterpret_cast<s16x4*>(&vf) = lo;
          *(reinterpret_cast<s16x4*>(&vf) + 1) = hi;
          o[0][s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pb[0][u], o[0][s], 0, 0, 0);
          if (two) o[1][s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pb[1][u], o[1][s], 0, 0, 0);
        }
    }
    if (more) write(kt + 64, kr, vr, att_tiles + 2 * (buf ^ 1) * TILE, att_tiles + (2 * (buf ^ 1) + 1) * TILE);
    __syncthreads();  // tile kt + 64 is in place, and nobody reads tile kt any more
  }
  if (!active) return;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    float li = l[i];
    li += __shfl_xor(li, 16);
    li += __shfl_xor(li, 32);
    const int q_tok = qw + 16 * i + qi;
    if (q_tok < len && (i == 0 || two)) {
      const float inv = 1.0f / li;
      const int64_t off = static_cast<int64_t>(t0 + q_tok) * H + head * DH + 4 * g;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        half_t h[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = static_cast<half_t>(fminf(fmaxf(o[i][s][r] * inv, -65504.0f), 65504.0f));
        *reinterpret_cast<uint2*>(ctx_h + off + 16 * s) = *reinterpret_cast<const uint2*>(h);
      }
    }
  }
}

// ---- the last layer of a [CLS]-pooled model, attended from the [CLS] rows alone ---------------------
//
// Behind the last layer's attention only the [CLS] rows are read (the cls_tail of forward_chunk), so that layer needs
// no query but the [CLS] one, and its keys and values only contracted with it. With the conventions of EPI_FOLD_F16,
// k_jc = inv_j (W'_k[c,:] . x_j - mean_j cs_k[c]) + c_k[c] over the f16 pre-LayerNorm rows x_j, for a head h
//   q_h . k_j = inv_j (u_h . x_j - mean_j alpha_h) + const,   u_h[d] = sum_{c in h} q_c W'_k[c,d],  alpha_h = sum_d u_h[d]
//   sum_j p_j v_j = W'_v,h z_h - cs_v gamma_h + c_v,          z_h = sum_j p_j inv_j x_j,  gamma_h = sum_j p_j inv_j mean_j
// (the constant is the same for every key and leaves the softmax; the weights p_j sum to 1, so c_v passes through).
// The K and V projections of the T rows become two H-wide dot products per (token, head): cls_head_gemm_kernel makes
// u from the [CLS] queries, cls_attend_kernel the logits, the softmax, z and gamma with one block per sequence, and
// cls_head_gemm_kernel again the context rows of the [CLS] tokens. u, p_j inv_j and z are rounded to f16 (the MFMA
// operands) where the ordinary route rounds the K and V rows; alpha and gamma are sums over those ROUNDED values —
// what the MFMAs really multiply by, as fold_vectors_kernel's column sums are — so the mean terms cancel exactly.
constexpr int kClsHeads = 16;  // heads per sequence: one 16-row MFMA operand (fewer: zero rows)
constexpr int kClsGroup = 16;  // keys per logit MFMA: a wave takes 16 keys of its sequence at a time
constexpr int kClsStep = 32;   // keys per context MFMA (its K dimension): the staged key count is padded to whole steps
using f16x4 = __attribute__((ext_vector_type(4))) _Float16;

// The LDS of cls_attend_kernel for hidden size H and lpad staged keys: the u rows, later the f16 weights (the larger of
// the two), the f32 logits and alpha. The launch is refused (the ordinary route runs) above the 64 KiB every kernel may have.
static size_t cls_attend_lds(int H, int lpad) {
  return static_cast<size_t>(kClsHeads) * (static_cast<size_t>(std::max(H, lpad)) + 8) * sizeof(half_t) +
         static_cast<size_t>(kClsHeads) * (static_cast<size_t>(lpad) + 4) * sizeof(float) + kClsHeads * sizeof(float);
}

// out[d][c] = in[c][d], H x H halfs: the last layer's gain-folded K weights with the contraction index of u contiguous
__global__ void transpose_f16_kernel(const half_t* __restrict__ in, int H, half_t* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= static_cast<int64_t>(H) * H) return;
  const int d = static_cast<int>(i / H), c = static_cast<int>(i % H);
  out[i] = in[static_cast<int64_t>(c) * H + d];
}

// Per head (blockIdx.z): out[m][n] = unscale * sum_k W[n][k] A[m][k], M rows, N columns, K deep, as
// gemm_f16_skinny_kernel computes it (W rows are the MFMA rows, 64 activation rows per block its columns, both
// operands 16-byte global loads). A head's operands start w_head / a_head / o_head halfs behind the previous head's;
// ldw / lda / ldo are the row strides. N % 16 == 0, K % 32 == 0.
// CTX = false: u — W the transposed K weights (row d, k = the head's 64 or 32 query columns), A the [CLS] queries.
// CTX = true: the context rows — W the head's V weights, A = z, and the epilogue adds - cs[col] gamma[m][head] + c[col].
template <bool CTX>
__global__ __launch_bounds__(256) void cls_head_gemm_kernel(const half_t* __restrict__ W, int ldw, int64_t w_head,
                                                            const half_t* __restrict__ A, int lda, int a_head, int M, int N,
                                                            int K, float unscale, const float* __restrict__ cs,
                                                            const float* __restrict__ c, const float* __restrict__ gamma,
                                                            half_t* __restrict__ out, int ldo, int o_head) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int head = blockIdx.z, nh = gridDim.z;
  const int n0 = blockIdx.x * 64 + wave * 16;  // this wave's 16 output columns
  const int row = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.y * 64;
  if (n0 >= N) return;
  const half_t* wp = W + head * w_head + static_cast<int64_t>(n0 + row) * ldw + 8 * g;
  const half_t* ap[4];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
    ap[mb] = A + static_cast<int64_t>(min(m0 + mb * 16 + row, M - 1)) * lda + static_cast<int64_t>(head) * a_head + 8 * g;
  f32x4 acc[4];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) acc[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int mblocks = (min(M - m0, 64) + 15) / 16;
  auto step = [&](int k) {
    const f16x8 wf = *reinterpret_cast<const f16x8*>(wp + k);
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
      if (mb < mblocks) {
        const f16x8 af = *reinterpret_cast<const f16x8*>(ap[mb] + k);
        acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, af, acc[mb], 0, 0, 0);
      }
  };
  int k = 0;
  for (; k + 64 <= K; k += 64) {  // (two steps' loads in flight)
    step(k);
    step(k + 32);
  }
  if (k < K) step(k);
  // C layout: column (lane & 15) = activation row m, rows 4g + r = output columns n0 + 4g + r
  const int n = n0 + 4 * g;
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) {
    const int m = m0 + mb * 16 + row;
    if (mb < mblocks && m < M) {
      half_t h[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[mb][r] * unscale;
        if (CTX) {
          const int col = head * N + n + r;
          v = (v - cs[col] * gamma[static_cast<int64_t>(m) * nh + head]) + c[col];
        }
        h[r] = static_cast<half_t>(fminf(fmaxf(v, -65504.0f), 65504.0f));
      }
      *reinterpret_cast<uint2*>(out + static_cast<int64_t>(m) * ldo + static_cast<int64_t>(head) * o_head + n) =
          *reinterpret_cast<const uint2*>(h);
    }
  }
}

// One block (4 waves) per sequence: the [CLS] query's attention over the sequence's own f16 pre-LayerNorm rows x_j
// (H wide, their (mean, 1/sigma) in stat), all heads at once as the 16 rows of one MFMA operand.
//   pass 1: logits s_hj = scale2 inv_j (u_h . x_j - mean_j alpha_h) (log2 domain), 16 keys per wave and MFMA chain, u from LDS
//   softmax per head in f32 over the sequence's len keys; w_hj = p_hj inv_j as f16 into LDS, gamma_h = sum_j w_hj mean_j
//   pass 2: z_h = sum_j w_hj x_j, the rows read a second time (from L2: a sequence's rows are at most a few hundred KB),
//           64 columns per wave and step — a lane loads 4 neighbouring columns of a key, one for each of 4 MFMA chains
// Every sum runs over the sequence's own rows in an order fixed by len alone, so a sequence's bits do not depend on
// its place in the batch. U, Z: [n_seq][nh][H] halfs; gamma: [n_seq][nh]. nh <= kClsHeads, H % 64 == 0,
// lpad = the batch's longest sequence rounded up to kClsStep; dynamic LDS: cls_attend_lds(H, lpad).
__global__ __launch_bounds__(256) void cls_attend_kernel(const half_t* __restrict__ x, const float2* __restrict__ stat,
                                                         const half_t* __restrict__ U, const int32_t* __restrict__ cu,
                                                         int seq0, int tok_base, int T, int H, int nh, float scale2, int lpad,
                                                         half_t* __restrict__ Z, float* __restrict__ gamma) {
  extern __shared__ __align__(16) unsigned char cls_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = lane & 15, g = lane >> 4;
  const int seq = blockIdx.x;
  const int us = H + 8;     // halfs per u row
  const int ps = lpad + 8;  // halfs per weight row
  const int ls = lpad + 4;  // floats per logit row
  half_t* sU = reinterpret_cast<half_t*>(cls_lds);
  half_t* sP = sU;  // the weights take the u rows' place once pass 1 is done
  float* sS = reinterpret_cast<float*>(cls_lds + static_cast<size_t>(kClsHeads) * (max(H, lpad) + 8) * sizeof(half_t));
  float* sA = sS + kClsHeads * ls;
  const int t0 = cu[seq0 + seq] - tok_base;
  const int len = min(min(cu[seq0 + seq + 1] - cu[seq0 + seq], T - t0), lpad);
  half_t* zrow = Z + static_cast<int64_t>(seq) * nh * H;
  if (len <= 0) {  // (block-uniform; read_offsets admits no empty sequence) zero rows, as pooling ignores them
    for (int i = tid; i < nh * H; i += 256) zrow[i] = static_cast<half_t>(0.0f);
    if (tid < nh) gamma[static_cast<int64_t>(seq) * nh + tid] = 0.0f;
    return;
  }
  // u rows into LDS (rows nh .. 15: zeros), then alpha_h = sum_d u_h[d] over the rounded values
  const int h8 = H >> 3;
  for (int i = tid; i < kClsHeads * h8; i += 256) {
    const int h = i / h8, c8 = i - h * h8;
    f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (h < nh) v = *reinterpret_cast<const f16x8*>(U + (static_cast<int64_t>(seq) * nh + h) * H + 8 * c8);
    *reinterpret_cast<f16x8*>(sU + h * us + 8 * c8) = v;
  }
  __syncthreads();
  for (int h = wave; h < kClsHeads; h += 4) {
    float a = 0.0f;
    for (int d = lane; d < H; d += 64) a += static_cast<float>(sU[h * us + d]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off);
    if (lane == 0) sA[h] = a;
  }
  __syncthreads();
  // pass 1
  const int groups = (len + kClsGroup - 1) / kClsGroup;
  for (int gi = wave; gi < groups; gi += 4) {
    const int tok = gi * kClsGroup + row;
    const int tc = min(tok, len - 1);  // (keys past the end: a valid row, its logit is not stored)
    const half_t* xp = x + static_cast<int64_t>(t0 + tc) * H + 8 * g;
    const half_t* up = sU + row * us + 8 * g;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < H; k += 64) {  // (H % 64 == 0: two steps' loads in flight)
      const f16x8 x0 = *reinterpret_cast<const f16x8*>(xp + k), x1 = *reinterpret_cast<const f16x8*>(xp + k + 32);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(up + k), x0, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(up + k + 32), x1, acc, 0, 0, 0);
    }
    // C layout: column (lane & 15) = key, rows 4g + r = heads
    const float2 st = stat[t0 + tc];
    if (tok < len) {
#pragma unroll
      for (int r = 0; r < 4; ++r) sS[(4 * g + r) * ls + tok] = scale2 * st.y * (acc[r] - st.x * sA[4 * g + r]);
    }
  }
  __syncthreads();
  // softmax, one wave per head; rows nh .. 15 and keys len .. lpad - 1: zero weights
  for (int h = wave; h < kClsHeads; h += 4) {
    if (h >= nh) {
      for (int j = lane; j < lpad; j += 64) sP[h * ps + j] = static_cast<half_t>(0.0f);
      continue;
    }
    float m = -INFINITY;
    for (int j = lane; j < len; j += 64) m = fmaxf(m, sS[h * ls + j]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    float sum = 0.0f;
    for (int j = lane; j < len; j += 64) sum += __builtin_amdgcn_exp2f(sS[h * ls + j] - m);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    const float inv_sum = 1.0f / sum;
    float gm = 0.0f;
    for (int j = lane; j < lpad; j += 64) {
      half_t wh = static_cast<half_t>(0.0f);
      if (j < len) {
        const float2 st = stat[t0 + j];
        wh = static_cast<half_t>(__builtin_amdgcn_exp2f(sS[h * ls + j] - m) * inv_sum * st.y);
        gm += static_cast<float>(wh) * st.x;
      }
      sP[h * ps + j] = wh;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) gm += __shfl_xor(gm, off);
    if (lane == 0) gamma[static_cast<int64_t>(seq) * nh + h] = gm;
  }
  __syncthreads();
  // pass 2: columns 64 dg + 4 row + q belong to chain q; its rows 4g + r are the columns 64 dg + 16 g + 4 r + q
  const half_t* pp = sP + row * ps + 8 * g;
  for (int dg = wave; dg < (H >> 6); dg += 4) {
    f32x4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    const half_t* xc = x + static_cast<int64_t>(t0) * H + 64 * dg + 4 * row;
    for (int j0 = 0; j0 < lpad; j0 += kClsStep) {
      f16x4 v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i)  // (keys past the end: a valid row times a zero weight)
        v[i] = *reinterpret_cast<const f16x4*>(xc + static_cast<int64_t>(min(j0 + 8 * g + i, len - 1)) * H);
      const f16x8 pf = *reinterpret_cast<const f16x8*>(pp + j0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f16x8 xf = {v[0][q], v[1][q], v[2][q], v[3][q], v[4][q], v[5][q], v[6][q], v[7][q]};
        acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xf, pf, acc[q], 0, 0, 0);
      }
    }
    // C layout: column (lane & 15) = head, this lane's 16 values = 16 consecutive columns from 64 dg + 16 g
    if (row < nh) {
      f16x8 o[2];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          o[(4 * r + q) >> 3][(4 * r + q) & 7] = static_cast<half_t>(fminf(fmaxf(acc[q][r], -65504.0f), 65504.0f));
      half_t* zp = zrow + static_cast<int64_t>(row) * H + 64 * dg + 16 * g;
      *reinterpret_cast<f16x8*>(zp) = o[0];
      *reinterpret_cast<f16x8*>(zp + 8) = o[1];
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------

static int dev_alloc_copy(vr_engine* e, Encoder* enc, const void* src, size_t n_floats, int mem, float** out) {
  float* p = nullptr;
  VR_HIP(hipMalloc(reinterpret_cast<void**>(&p), n_floats * sizeof(float)));
  enc->owned.push_back(p);
  if (src)
    VR_HIP(hipMemcpyAsync(p, src, n_floats * sizeof(float),
                          mem == VR_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, e->stream));
  *out = p;
  return 0;
}

// w (device, n floats) -> scaled (hi, lo) f16 pair; scale = 2^s puts max|w| into [1024, 2048)
// (mean, 1/sigma) of every row from the per-64-column partial sums of EPI_BIAS_RESIDUAL_LN_STATS
__global__ void ln_finalize_kernel(const float2* __restrict__ part, int T, int segs, int H, float eps,
                                   float2* __restrict__ stat) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  float s1 = 0.0f, s2 = 0.0f;
  for (int i = 0; i < segs; ++i) {  // fixed order
    const float2 p = part[static_cast<int64_t>(t) * segs + i];
    s1 += p.x;
    s2 += p.y;
  }
  const float mean = s1 / static_cast<float>(H);
  const float var = fmaxf(s2 / static_cast<float>(H) - mean * mean, 0.0f);
  stat[t] = make_float2(mean, 1.0f / sqrtf(var + eps));
}

// out[n][k] = w[n][k] * g[k]
__global__ void scale_cols_kernel(const float* __restrict__ w, const float* __restrict__ g, int64_t n, int K,
                                  float* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) out[i] = w[i] * g[i % K];
}

// one wave per output column n: colsum[n] = unscale * sum_k f16 weight[n][k] (the weights the MFMA really
// multiplies by), c[n] = bias[n] + sum_k w[n][k] b[k] (f32 weights, f64 accumulation)
__global__ __launch_bounds__(256) void fold_vectors_kernel(const half_t* __restrict__ wq, float unscale,
                                                           const float* __restrict__ w, const float* __restrict__ b,
                                                           const float* __restrict__ bias, int N, int K,
                                                           float* __restrict__ colsum, float* __restrict__ c) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  double sq = 0.0, sc = 0.0;
  for (int k = lane; k < K; k += 64) {
    sq += static_cast<double>(static_cast<float>(wq[static_cast<int64_t>(n) * K + k]));
    sc += static_cast<double>(w[static_cast<int64_t>(n) * K + k]) * static_cast<double>(b[k]);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    sq += __shfl_xor(sq, off);
    sc += __shfl_xor(sc, off);
  }
  if (lane == 0) {
    colsum[n] = static_cast<float>(sq * static_cast<double>(unscale));
    c[n] = static_cast<float>(static_cast<double>(bias[n]) + sc);
  }
}

static int make_split(vr_engine* e, Encoder* enc, const float* w_dev, size_t n, int K, bool plain, SplitWeight* out) {
  float* scratch = nullptr;
  VR_TRY(dev_alloc_copy(e, enc, nullptr, 1, 0, &scratch));
  VR_HIP(hipMemsetAsync(scratch, 0, sizeof(float), e->stream));
  const unsigned blocks = static_cast<unsigned>(std::min<size_t>(1024, (n + 255) / 256));
  hipLaunchKernelGGL(absmax_kernel, dim3(blocks), dim3(256), 0, e->stream, w_dev, static_cast<int64_t>(n),
                     reinterpret_cast<unsigned int*>(scratch));
  float m = 0.0f;
  VR_HIP(hipMemcpyAsync(&m, scratch, sizeof(float), hipMemcpyDeviceToHost, e->stream));
  VR_HIP(hipStreamSynchronize(e->stream));
  VR_CHECK(std::isfinite(m), "weight tensor holds a non-finite value");
  int s = 0;
  if (m > 0.0f) {
    int ex = 0;
    (void)std::frexp(m, &ex);  // m = f * 2^ex, f in [0.5, 1)
    s = 11 - ex;
  }
  const float scale = std::ldexp(1.0f, s);
  out->unscale = std::ldexp(1.0f, -s);
  float* both = nullptr;  // one interleaved array of 2n halfs (= n floats), see split_at; plain: n halfs
  VR_TRY(dev_alloc_copy(e, enc, nullptr, plain ? (n + 1) / 2 : n, 0, &both));
  out->hi = reinterpret_cast<_Float16*>(both);
  out->lo = plain ? nullptr : out->hi + 8;
  hipLaunchKernelGGL(split_weights_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, e->stream,
                     w_dev, static_cast<int64_t>(n), K, scale, out->hi, out->lo);
  VR_HIP(hipGetLastError());
  return 0;
}

static void free_encoder(void** slot) {
  Encoder* enc = static_cast<Encoder*>(*slot);
  if (!enc) return;
  for (float* p : enc->owned) (void)hipFree(p);
  enc->ids.release();
  enc->cu.release();
  enc->seg.release();
  enc->span_tok.release();
  enc->span_seq.release();
  for (DevArray<int32_t>* a : {&enc->sem_off, &enc->sem_start, &enc->sem_idx, &enc->sem_seq_chunks, &enc->sem_seq_base, &enc->sem_counter})
    a->release();
  for (DevArray<float>* a : {&enc->sem_sums, &enc->sem_dist, &enc->sem_rows}) a->release();
  enc->skinny_ws.release();
  invalidate_graphs(enc);
  enc->out.release();
  enc->rows.release();
  enc->tail_ws.release();
  enc->pooled.release();
  delete enc;
  *slot = nullptr;
}

void encoder_release(vr_engine* e) {
  free_encoder(&e->encoder);
  free_encoder(&e->reranker);
}

int encoder_hidden(vr_engine* e) {
  Encoder* enc = static_cast<Encoder*>(e->encoder);
  return enc ? enc->d.hidden : 0;
}

// The caller's description, zero-extended: a caller compiled against the header that ended at `precision` passes that
// shorter struct_size, and gets what it always got (learned positions, the plain GELU FFN).
// (vr_bert_desc_v2: the same description one field longer, `causal`; every shorter size reads it as 0)
// (vr_bert_desc_v3: two fields more, `head_dim` and `qk_norm`, read as 0 from every shorter size as well)
static int read_desc(const vr_bert_desc* src, vr_bert_desc* out, int32_t* causal = nullptr, int32_t* head_dim = nullptr,
                     int32_t* qk_norm = nullptr) {
  const int32_t short_size = static_cast<int32_t>(offsetof(vr_bert_desc, position));
  const int32_t post_size = static_cast<int32_t>(offsetof(vr_bert_desc, norm));  // ... or at `ffn`: post-norm, no window
  const bool v3 = src->struct_size == static_cast<int32_t>(sizeof(vr_bert_desc_v3));
  const bool v2 = v3 || src->struct_size == static_cast<int32_t>(sizeof(vr_bert_desc_v2));
  VR_CHECK(src->struct_size == static_cast<int32_t>(sizeof(vr_bert_desc)) || src->struct_size == short_size ||
               src->struct_size == post_size || v2,
           "vr_bert_desc size mismatch");
  *out = vr_bert_desc{};
  memcpy(out, src, v2 ? sizeof(vr_bert_desc) : static_cast<size_t>(src->struct_size));
  if (causal) *causal = v2 ? reinterpret_cast<const vr_bert_desc_v2*>(src)->causal : 0;
  if (head_dim) *head_dim = v3 ? reinterpret_cast<const vr_bert_desc_v3*>(src)->head_dim : 0;
  if (qk_norm) *qk_norm = v3 ? reinterpret_cast<const vr_bert_desc_v3*>(src)->qk_norm : 0;
  out->struct_size = static_cast<int32_t>(sizeof(vr_bert_desc));
  return 0;
}

// device array of n floats from src, or of zeros when src is null (an absent bias)
static int dev_alloc_copy_or_zero(vr_engine* e, Encoder* enc, const void* src, size_t n_floats, int mem, float** out) {
  VR_TRY(dev_alloc_copy(e, enc, src, n_floats, mem, out));
  if (!src) VR_HIP(hipMemsetAsync(*out, 0, n_floats * sizeof(float), e->stream));
  return 0;
}

// windowed layers take attention_stream_kernel from this many tokens on (the longest sequence of the pass), the staged
// kernel below: the measured crossover, see DESIGN.md §19
static const int kWindowStreamFrom = 384;

// a model from its 5 + 16 L (gated FFN: 5 + 18 L) tensors (vr_encoder_load's order) into *slot, replacing what is there
static int build_encoder(vr_engine* e, void** slot, const vr_bert_desc* d_in, const void* const* t, int n_tensors, int mem) {
  vr_bert_desc desc;
  int32_t causal = 0, head_dim = 0, qk_norm = 0;
  VR_TRY(read_desc(d_in, &desc, &causal, &head_dim, &qk_norm));
  const vr_bert_desc* d = &desc;
  const int H = d->hidden, I = d->intermediate, L = d->layers;
  VR_CHECK(d->position == VR_POS_LEARNED || d->position == VR_POS_ROTARY || d->position == VR_POS_NONE,
           "unknown position scheme %d", d->position);
  VR_CHECK(d->ffn == VR_FFN_GELU || d->ffn == VR_FFN_SWIGLU || d->ffn == VR_FFN_GEGLU || d->ffn == VR_FFN_RELU,
           "unknown ffn kind %d", d->ffn);
  const bool rotary = d->position == VR_POS_ROTARY, gated = d->ffn == VR_FFN_SWIGLU || d->ffn == VR_FFN_GEGLU;
  const int per_layer = (gated ? 18 : 16) + (qk_norm == 1 ? 2 : 0);  // (qk_norm: VR_NORM_PRE_RMS_ROTARY only, which is gated)
  VR_CHECK(!rotary || (std::isfinite(d->rope_theta) && d->rope_theta > 0.0f), "rope_theta %g must be positive",
           static_cast<double>(d->rope_theta));
  VR_CHECK(d->norm == VR_NORM_POST || d->norm == VR_NORM_PRE || d->norm == VR_NORM_PRE_RMS || d->norm == VR_NORM_PRE_RMS_ROTARY,
           "unknown norm placement %d", d->norm);
  const bool prenorm = d->norm == VR_NORM_PRE, rms = d->norm == VR_NORM_PRE_RMS, rms_rot = d->norm == VR_NORM_PRE_RMS_ROTARY;
  // (the Qwen2 form: one combination as well, and the only norm that takes the causal mask)
  VR_CHECK(!rms_rot || rotary, "norm VR_NORM_PRE_RMS_ROTARY needs position VR_POS_ROTARY (position %d)", d->position);
  VR_CHECK(!rms_rot || gated, "norm VR_NORM_PRE_RMS_ROTARY needs a gated ffn (ffn %d): VR_FFN_SWIGLU or VR_FFN_GEGLU", d->ffn);
  VR_CHECK(!rms_rot || d->window == 0, "norm VR_NORM_PRE_RMS_ROTARY takes no window (window %d): a causal sliding window is "
           "not implemented", d->window);
  VR_CHECK(!rms_rot || d->type_vocab == 1, "norm VR_NORM_PRE_RMS_ROTARY needs type_vocab 1 (type_vocab %d)", d->type_vocab);
  VR_CHECK(causal == 0 || causal == 1, "causal %d must be 0 or 1", causal);
  VR_CHECK(causal == 0 || rms_rot, "causal %d needs norm VR_NORM_PRE_RMS_ROTARY (norm %d): the causal mask exists in that "
           "loop only", causal, d->norm);
  // (vr_bert_desc_v3: a head size of its own and the Q/K norms, Qwen3's, in that loop only as well)
  VR_CHECK(head_dim == 0 || rms_rot, "head_dim %d needs norm VR_NORM_PRE_RMS_ROTARY (norm %d): a head size other than "
           "hidden / heads exists in that loop only", head_dim, d->norm);
  VR_CHECK(head_dim == 0 || head_dim == 32 || head_dim == 64 || head_dim == 128, "head_dim %d must be 0 (hidden / heads), 32, "
           "64 or 128", head_dim);
  VR_CHECK(qk_norm == 0 || qk_norm == 1, "qk_norm %d must be 0 or 1", qk_norm);
  VR_CHECK(qk_norm == 0 || rms_rot, "qk_norm %d needs norm VR_NORM_PRE_RMS_ROTARY (norm %d): the query / key norms exist in "
           "that loop only", qk_norm, d->norm);
  // (the T5 form: one combination, everything outside it refused by the field that leaves it)
  VR_CHECK(!rms || d->position == VR_POS_NONE, "norm VR_NORM_PRE_RMS needs position VR_POS_NONE (position %d): RMSNorm "
           "encoders with a position table or rotary positions are not implemented", d->position);
  VR_CHECK(!rms || d->ffn == VR_FFN_RELU, "norm VR_NORM_PRE_RMS needs ffn VR_FFN_RELU (ffn %d): RMSNorm encoders with a GELU "
           "or gated feed-forward block are not implemented", d->ffn);
  VR_CHECK(!rms || d->window == 0, "norm VR_NORM_PRE_RMS takes no window (window %d): sliding-window attention needs "
           "rotary positions", d->window);
  VR_CHECK(!rms || d->type_vocab == 1, "norm VR_NORM_PRE_RMS needs type_vocab 1 (type_vocab %d)", d->type_vocab);
  VR_CHECK(d->ffn != VR_FFN_RELU || rms, "ffn VR_FFN_RELU needs norm VR_NORM_PRE_RMS (norm %d): the ReLU feed-forward "
           "block exists in the RMSNorm pre-norm loop only", d->norm);
  // (a model without positions: refusals of its own, ahead of the ones that tell a table model what pre-norm needs)
  VR_CHECK(d->position != VR_POS_NONE || !prenorm, "position VR_POS_NONE needs norm VR_NORM_POST (norm %d): pre-norm encoders "
           "without positions are not implemented", d->norm);
  VR_CHECK(d->position != VR_POS_NONE || d->window == 0, "position VR_POS_NONE takes no window (window %d): sliding-window "
           "attention needs rotary positions", d->window);
  VR_CHECK(!prenorm || rotary, "norm VR_NORM_PRE needs position VR_POS_ROTARY (position %d): pre-norm encoders with a "
           "position table are not implemented", d->position);
  VR_CHECK(!prenorm || gated, "norm VR_NORM_PRE needs a gated ffn (ffn %d): pre-norm encoders with the plain GELU "
           "feed-forward block are not implemented", d->ffn);
  VR_CHECK(d->window >= 0 && d->window <= 4096, "window %d must lie in 0..4096", d->window);
  VR_CHECK(d->window == 0 || rotary, "window %d needs position VR_POS_ROTARY (position %d)", d->window, d->position);
  VR_CHECK(d->window == 0 || prenorm, "window %d needs norm VR_NORM_PRE (norm %d): sliding-window attention in a "
           "post-norm encoder is not implemented", d->window, d->norm);
  VR_CHECK(d->window == 0 || d->global_every >= 1, "global_every %d must be >= 1 when window is set", d->global_every);
  VR_CHECK(d->rope_theta_local == 0.0f || (rotary && std::isfinite(d->rope_theta_local) && d->rope_theta_local > 0.0f),
           "rope_theta_local %g must be positive (or 0: rope_theta) and needs position VR_POS_ROTARY",
           static_cast<double>(d->rope_theta_local));
  VR_CHECK(d->max_pos >= 1 && d->max_pos <= 8192, "max_pos %d must lie in 1..8192 (the longest sequence the engine runs)",
           d->max_pos);
  VR_CHECK(L >= 1 && H >= 128 && H % 128 == 0 && H <= 1024, "hidden %d must be a multiple of 128 in 128..1024", H);
  VR_CHECK(I % 128 == 0 && I % BK == 0, "intermediate %d must be a multiple of 128", I);
  if (head_dim == 0)
    VR_CHECK(d->heads >= 1 && H % d->heads == 0 && (H / d->heads == 32 || H / d->heads == 64),
             "head size %d unsupported (32 or 64)", d->heads ? H / d->heads : 0);
  VR_CHECK(d->heads >= 1, "heads %d must be >= 1", d->heads);
  // the attention width: the [Q | K | V] rows are 3 A wide, the context A (A == H unless head_dim says otherwise)
  const int dh = head_dim ? head_dim : H / d->heads;
  const int64_t A64 = static_cast<int64_t>(d->heads) * dh;
  VR_CHECK(A64 % 128 == 0 && A64 <= 2048, "heads %d x head_dim %d = %lld: the attention width must be a multiple of 128 and at "
           "most 2048", d->heads, dh, static_cast<long long>(A64));
  const int A = static_cast<int>(A64);
  VR_CHECK(n_tensors == 5 + per_layer * L, "expected %d tensors, got %d", 5 + per_layer * L, n_tensors);
  VR_CHECK(d->pooling == VR_POOL_MEAN || d->pooling == VR_POOL_CLS || d->pooling == VR_POOL_LAST,
           "pooling %d must be 0 (mean), 1 (cls) or 2 (last token)", d->pooling);
  VR_CHECK(d->precision == VR_PRECISION_F32 || d->precision == VR_PRECISION_F16X3 || d->precision == VR_PRECISION_F16,
           "unknown precision %d", d->precision);
  for (int i = 0; i < n_tensors; ++i) {
    const int in_layer = i < 5 ? -1 : (i - 5) % per_layer;  // null is allowed for a projection's bias, and for the
    const bool bias = in_layer == 1 || in_layer == 3 || in_layer == 5 || in_layer == 7 || in_layer == 11 ||  // unused table
                      in_layer == 13 || in_layer == 17;
    // (RMSNorm reads no shift, and its stream takes a missing token-type row as zeros)
    const bool rms_unused = (rms || rms_rot) && (i == 2 || i == 4 || in_layer == 9 || in_layer == 15);
    // (in_layer 18, 19: the Q/K norm weights, never null)
    VR_CHECK(t[i] != nullptr || bias || rms_unused || (i == 1 && d->position != VR_POS_LEARNED), "tensor %d is null", i);
  }
  int window_stream_from = kWindowStreamFrom;  // (checked here: nothing is replaced when it is refused)
  if (const char* from = getenv("VR_WINDOW_STREAM_FROM")) {
    char* end = nullptr;
    const long v = strtol(from, &end, 10);
    VR_CHECK(end != from && *end == '\0' && v >= 1 && v <= INT32_MAX, "VR_WINDOW_STREAM_FROM='%s' must be a whole number >= 1",
             from);
    window_stream_from = static_cast<int>(v);
  }
  free_encoder(slot);
  Encoder* enc = new Encoder();
  *slot = enc;
  enc->d = *d;
  enc->causal = causal;
  enc->dh = dh;
  enc->attn = A;
  enc->qk_norm = qk_norm;
  enc->fuse = !(getenv("VR_ENCODE_FUSE") && atoi(getenv("VR_ENCODE_FUSE")) == 0);
  // (the embedder alone: a cross-encoder's unnormalised logits keep the bits of the ordinary last layer, which
  // tests/golden/textpath_bert.npz pins)
  enc->cls_collapse = slot == &e->encoder && !(getenv("VR_CLS_COLLAPSE") && atoi(getenv("VR_CLS_COLLAPSE")) == 0);
  const size_t HH = static_cast<size_t>(A) * H;  // a projection's weights: [A, H] (query, key, value) or [H, A] (output)
  VR_TRY(dev_alloc_copy(e, enc, t[0], static_cast<size_t>(d->vocab) * H, mem, &enc->word));
  if (d->position == VR_POS_LEARNED) VR_TRY(dev_alloc_copy(e, enc, t[1], static_cast<size_t>(d->max_pos) * H, mem, &enc->pos));
  std::vector<float2> rope_host[2];  // (live until the synchronisation at the end: they are sources of async copies)
  auto rope_table = [&](float theta, std::vector<float2>& host, float2** out) -> int {
    // (cos, sin)(p * theta^(-2i/d_h)) in f64, stored as f32
    const int half = dh / 2, row = A / 2;  // a row repeats the d_h/2 frequencies for every head
    host.resize(static_cast<size_t>(d->max_pos) * row);
    for (int i = 0; i < half; ++i) {
      const double inv_freq = std::pow(static_cast<double>(theta), -2.0 * i / (2.0 * half));
      for (int p = 0; p < d->max_pos; ++p) {
        const double a = p * inv_freq;
        const float2 cs = make_float2(static_cast<float>(std::cos(a)), static_cast<float>(std::sin(a)));
        for (int h = 0; h < d->heads; ++h) host[static_cast<size_t>(p) * row + h * half + i] = cs;
      }
    }
    float* table = nullptr;
    VR_TRY(dev_alloc_copy(e, enc, host.data(), host.size() * 2, VR_MEM_HOST, &table));
    *out = reinterpret_cast<float2*>(table);
    return 0;
  };
  if (rotary) VR_TRY(rope_table(d->rope_theta, rope_host[0], &enc->rope));
  // the windowed layers' table: only where a layer is windowed and its base differs (bit for bit the same table else)
  if (rotary && d->window > 0 && d->rope_theta_local != 0.0f && d->rope_theta_local != d->rope_theta)
    VR_TRY(rope_table(d->rope_theta_local, rope_host[1], &enc->rope_local));
  // Windowed layers of sequences short enough to stage whole: the staged kernel visits 128 + 2 w keys per 128 queries
  // as well (it skips the key tiles outside a query tile's window) but runs one block per (sequence, head), the
  // streamed kernel one per 128 queries. Which is faster was measured at 512 tokens;
  // VR_WINDOW_STREAM_FROM, read when the model is loaded, moves the length from which the streamed kernel runs.
  enc->window_stream_from = window_stream_from;
  if (rms || rms_rot) VR_TRY(dev_alloc_copy_or_zero(e, enc, t[2], H, mem, &enc->type));
  else VR_TRY(dev_alloc_copy(e, enc, t[2], static_cast<size_t>(d->type_vocab) * H, mem, &enc->type));
  VR_TRY(dev_alloc_copy(e, enc, t[3], H, mem, &enc->lng));
  if (!rms && !rms_rot) VR_TRY(dev_alloc_copy(e, enc, t[4], H, mem, &enc->lnb));  // (RMSNorm: the shifts stay null, no kernel reads one)
  const hipMemcpyKind kind = mem == VR_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  for (int l = 0; l < L; ++l) {
    // q_w q_b k_w k_b v_w v_b o_w o_b ln1_g ln1_b i_w i_b f_w f_b ln2_g ln2_b (gated: + gate_w gate_b, i_* = up)
    const void* const* w = t + 5 + per_layer * l;
    const int N1 = gated ? 2 * I : I;  // rows of the FFN-up matrix: gated = the gate's I rows, then the up projection's
    LayerWeights lw{};
    VR_TRY(dev_alloc_copy(e, enc, nullptr, 3 * HH, mem, &lw.wqkv));
    VR_TRY(dev_alloc_copy(e, enc, nullptr, 3 * static_cast<size_t>(A), mem, &lw.bqkv));
    for (int p = 0; p < 3; ++p) {  // fused QKV projection: rows [0,A) = query, [A,2A) = key, [2A,3A) = value (A = H but for head_dim)
      VR_HIP(hipMemcpyAsync(lw.wqkv + p * HH, w[2 * p], HH * sizeof(float), kind, e->stream));
      if (w[2 * p + 1]) VR_HIP(hipMemcpyAsync(lw.bqkv + p * A, w[2 * p + 1], A * sizeof(float), kind, e->stream));
      else VR_HIP(hipMemsetAsync(lw.bqkv + p * A, 0, A * sizeof(float), e->stream));
    }
    if (qk_norm) {
      VR_TRY(dev_alloc_copy(e, enc, w[18], dh, mem, &lw.qn));
      VR_TRY(dev_alloc_copy(e, enc, w[19], dh, mem, &lw.kn));
    }
    VR_TRY(dev_alloc_copy(e, enc, w[6], HH, mem, &lw.wo));
    VR_TRY(dev_alloc_copy_or_zero(e, enc, w[7], H, mem, &lw.bo));
    VR_TRY(dev_alloc_copy(e, enc, w[8], H, mem, &lw.ln1g));
    if (!rms && !rms_rot) VR_TRY(dev_alloc_copy(e, enc, w[9], H, mem, &lw.ln1b));
    if (gated) {
      const size_t IH = static_cast<size_t>(I) * H;
      VR_TRY(dev_alloc_copy(e, enc, nullptr, 2 * IH, mem, &lw.w1));
      VR_TRY(dev_alloc_copy(e, enc, nullptr, 2 * static_cast<size_t>(I), mem, &lw.b1));
      for (int p = 0; p < 2; ++p) {  // p = 0: gate (slots 16, 17), 1: up (slots 10, 11)
        const void* pw = p == 0 ? w[16] : w[10];
        const void* pb = p == 0 ? w[17] : w[11];
        VR_HIP(hipMemcpyAsync(lw.w1 + p * IH, pw, IH * sizeof(float), kind, e->stream));
        if (pb) VR_HIP(hipMemcpyAsync(lw.b1 + p * I, pb, I * sizeof(float), kind, e->stream));
        else VR_HIP(hipMemsetAsync(lw.b1 + p * I, 0, I * sizeof(float), e->stream));
      }
    } else {
      VR_TRY(dev_alloc_copy(e, enc, w[10], static_cast<size_t>(I) * H, mem, &lw.w1));
      VR_TRY(dev_alloc_copy_or_zero(e, enc, w[11], I, mem, &lw.b1));
    }
    VR_TRY(dev_alloc_copy(e, enc, w[12], static_cast<size_t>(I) * H, mem, &lw.w2));
    VR_TRY(dev_alloc_copy_or_zero(e, enc, w[13], H, mem, &lw.b2));
    VR_TRY(dev_alloc_copy(e, enc, w[14], H, mem, &lw.ln2g));
    if (!rms && !rms_rot) VR_TRY(dev_alloc_copy(e, enc, w[15], H, mem, &lw.ln2b));
    if (d->precision != VR_PRECISION_F32) {
      const bool plain = d->precision == VR_PRECISION_F16;
      VR_TRY(make_split(e, enc, lw.wqkv, 3 * HH, H, plain, &lw.s_qkv));
      VR_TRY(make_split(e, enc, lw.wo, HH, A, plain, &lw.s_o));
      VR_TRY(make_split(e, enc, lw.w1, static_cast<size_t>(N1) * H, H, plain, &lw.s_1));
      VR_TRY(make_split(e, enc, lw.w2, static_cast<size_t>(I) * H, I, plain, &lw.s_2));
      if (plain && (rotary || gated) && enc->fuse) {  // the re-ordered matrices and biases of the fused epilogues
        auto reordered = [&](const float* w_dev, const float* b_dev, int rows, int mode, int n, SplitWeight* sw, float** bias) -> int {
          const size_t cnt = static_cast<size_t>(rows) * H;
          float* tmp = nullptr;
          VR_HIP(hipMalloc(reinterpret_cast<void**>(&tmp), cnt * sizeof(float)));
          hipLaunchKernelGGL(reorder_rows_kernel, dim3(static_cast<unsigned>((cnt + 255) / 256)), dim3(256), 0, e->stream, w_dev,
                             static_cast<int64_t>(cnt), H, mode, n, H / d->heads, tmp);
          int rc = make_split(e, enc, tmp, cnt, H, true, sw);
          if (rc == 0) rc = dev_alloc_copy(e, enc, nullptr, rows, 0, bias);
          if (rc == 0)
            hipLaunchKernelGGL(reorder_rows_kernel, dim3(static_cast<unsigned>((rows + 255) / 256)), dim3(256), 0, e->stream, b_dev,
                               static_cast<int64_t>(rows), 1, mode, n, H / d->heads, *bias);
          (void)hipStreamSynchronize(e->stream);
          (void)hipFree(tmp);
          return rc;
        };
        // (the rotating epilogues: not behind a Q/K norm, which needs a whole head first, nor at a width other than H)
        if (rotary && !qk_norm && A == H) VR_TRY(reordered(lw.wqkv, lw.bqkv, 3 * H, 0, H, &lw.s_qkv_p, &lw.bqkv_p));
        if (gated) VR_TRY(reordered(lw.w1, lw.b1, 2 * I, 1, I, &lw.s_1_p, &lw.b1_p));
      }
      if (plain && H % 64 == 0 && !prenorm && !rms && !rms_rot) {  // operands of the folded-LayerNorm GEMMs (the post-norm loop's)
        auto fold = [&](const float* w_dev, int N, const float* g, const float* b, const float* bias, SplitWeight* sw,
                        float** colsum, float** c) -> int {
          const size_t n = static_cast<size_t>(N) * H;
          float* scaled = nullptr;
          VR_HIP(hipMalloc(reinterpret_cast<void**>(&scaled), n * sizeof(float)));
          hipLaunchKernelGGL(scale_cols_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, e->stream, w_dev,
                             g, static_cast<int64_t>(n), H, scaled);
          int rc = make_split(e, enc, scaled, n, H, true, sw);
          if (rc == 0) rc = dev_alloc_copy(e, enc, nullptr, N, 0, colsum);
          if (rc == 0) rc = dev_alloc_copy(e, enc, nullptr, N, 0, c);
          if (rc == 0)
            hipLaunchKernelGGL(fold_vectors_kernel, dim3(static_cast<unsigned>((N + 3) / 4)), dim3(256), 0, e->stream, sw->hi,
                               sw->unscale, w_dev, b, bias, N, H, *colsum, *c);
          (void)hipStreamSynchronize(e->stream);
          (void)hipFree(scaled);
          return rc;
        };
        VR_TRY(fold(lw.w1, N1, lw.ln1g, lw.ln1b, lw.b1, &lw.s_1_f, &lw.cs_1, &lw.c_1));
        if (gated && lw.b1_p) {  // the same from the interleaved matrix (EPI_FOLD_*GLU)
          const size_t cnt = static_cast<size_t>(N1) * H;
          float* inter = nullptr;
          VR_HIP(hipMalloc(reinterpret_cast<void**>(&inter), cnt * sizeof(float)));
          hipLaunchKernelGGL(reorder_rows_kernel, dim3(static_cast<unsigned>((cnt + 255) / 256)), dim3(256), 0, e->stream, lw.w1,
                             static_cast<int64_t>(cnt), H, 1, I, H / d->heads, inter);
          const int rc = fold(inter, N1, lw.ln1g, lw.ln1b, lw.b1_p, &lw.s_1_fp, &lw.cs_1_p, &lw.c_1_p);  // (drains the stream)
          (void)hipFree(inter);
          VR_TRY(rc);
        }
        if (!enc->layers.empty()) {
          const LayerWeights& prev = enc->layers.back();
          VR_TRY(fold(lw.wqkv, 3 * H, prev.ln2g, prev.ln2b, lw.bqkv, &lw.s_qkv_f, &lw.cs_qkv, &lw.c_qkv));
          if (l + 1 == L && enc->cls_collapse && d->pooling == VR_POOL_CLS && A == H) {  // see cls_attend_kernel
            float* kt = nullptr;
            VR_TRY(dev_alloc_copy(e, enc, nullptr, HH / 2, 0, &kt));
            lw.wk_t = reinterpret_cast<_Float16*>(kt);
            hipLaunchKernelGGL(transpose_f16_kernel, dim3(static_cast<unsigned>((HH + 255) / 256)), dim3(256), 0, e->stream,
                               lw.s_qkv_f.hi + HH, H, lw.wk_t);
            VR_HIP(hipGetLastError());
          }
        }
      }
    }
    enc->layers.push_back(lw);
  }
  VR_HIP(hipStreamSynchronize(e->stream));  // host sources may be freed by the caller now
  return 0;
}

int encoder_load(vr_engine* e, const vr_bert_desc* d, const void* const* t, int n_tensors, int mem) {
  return build_encoder(e, &e->encoder, d, t, n_tensors, mem);
}

// The embedder's attention bias (vr_encoder_set_attention_bias). Every check runs before anything changes; the captured
// graphs hold the table's pointer and the kernels' instantiation, so they go as they do when the workspace moves.
int encoder_set_attention_bias(vr_engine* e, const float* table, int heads, int radius, int mem) {
  Encoder* enc = static_cast<Encoder*>(e->encoder);
  VR_CHECK(enc, "no encoder loaded");
  float* fresh = nullptr;
  if (table) {
    VR_CHECK((enc->d.position == VR_POS_LEARNED && enc->d.norm == VR_NORM_POST) ||
                 (enc->d.position == VR_POS_NONE && enc->d.norm == VR_NORM_PRE_RMS),  // (BERT / MPNet, or T5)
             "an attention bias needs position VR_POS_LEARNED and norm VR_NORM_POST (position %d, norm %d)", enc->d.position,
             enc->d.norm);
    VR_CHECK(heads == enc->d.heads, "bias table of %d heads for an encoder of %d", heads, enc->d.heads);
    VR_CHECK(!enc->slopes, "the encoder has attention slopes (vr_encoder_set_attention_slopes): remove them before a "
             "bias table is set");
    VR_CHECK(radius >= 1 && radius <= kMaxBiasRadius, "radius %d must lie in 1..%d", radius, kMaxBiasRadius);
    const size_t n = static_cast<size_t>(heads) * (2 * static_cast<size_t>(radius) + 1);
    VR_HIP(hipMalloc(reinterpret_cast<void**>(&fresh), n * sizeof(float)));
    hipError_t err = hipMemcpyAsync(fresh, table, n * sizeof(float),
                                    mem == VR_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);  // (the source may go; passes that read the old table are over)
    if (err != hipSuccess) {
      (void)hipFree(fresh);
      VR_HIP(err);
    }
  } else {
    VR_HIP(hipStreamSynchronize(e->stream));
  }
  invalidate_graphs(enc);
  if (enc->bias) {
    enc->owned.erase(std::remove(enc->owned.begin(), enc->owned.end(), enc->bias), enc->owned.end());
    (void)hipFree(enc->bias);
  }
  enc->bias = fresh;
  enc->bias_radius = fresh ? radius : 0;
  if (fresh) enc->owned.push_back(fresh);
  return 0;
}

// The embedder's linear attention bias (vr_encoder_set_attention_slopes), as encoder_set_attention_bias: every check
// runs before anything changes, and the captured graphs, which hold the pointer and the kernels' instantiation, go.
int encoder_set_attention_slopes(vr_engine* e, const float* slopes, int heads, int mem) {
  Encoder* enc = static_cast<Encoder*>(e->encoder);
  VR_CHECK(enc, "no encoder loaded");
  float* fresh = nullptr;
  if (slopes) {
    VR_CHECK((enc->d.position == VR_POS_LEARNED || enc->d.position == VR_POS_NONE) && enc->d.norm == VR_NORM_POST,
             "an attention bias needs position VR_POS_LEARNED and norm VR_NORM_POST (position %d, norm %d)", enc->d.position,
             enc->d.norm);
    VR_CHECK(heads == enc->d.heads, "%d attention slopes for an encoder of %d heads", heads, enc->d.heads);
    VR_CHECK(!enc->bias, "the encoder has an attention bias table (vr_encoder_set_attention_bias): remove it before "
             "slopes are set");
    std::vector<float> host(static_cast<size_t>(heads));
    if (mem == VR_MEM_HOST) {
      std::copy(slopes, slopes + heads, host.begin());
    } else {
      VR_HIP(hipMemcpyAsync(host.data(), slopes, host.size() * sizeof(float), hipMemcpyDeviceToHost, e->stream));
      VR_HIP(hipStreamSynchronize(e->stream));
    }
    for (int h = 0; h < heads; ++h)
      VR_CHECK(std::isfinite(host[h]) && host[h] >= 0.0f && host[h] <= 1e30f,
               "attention slope %g of head %d must be finite and lie in 0..1e30", static_cast<double>(host[h]), h);
    VR_HIP(hipMalloc(reinterpret_cast<void**>(&fresh), host.size() * sizeof(float)));
    hipError_t err = hipMemcpyAsync(fresh, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);  // (`host` may go; passes that read the old slopes are over)
    if (err != hipSuccess) {
      (void)hipFree(fresh);
      VR_HIP(err);
    }
  } else {
    VR_HIP(hipStreamSynchronize(e->stream));
  }
  invalidate_graphs(enc);
  if (enc->slopes) {
    enc->owned.erase(std::remove(enc->owned.begin(), enc->owned.end(), enc->slopes), enc->owned.end());
    (void)hipFree(enc->slopes);
  }
  enc->slopes = fresh;
  if (fresh) enc->owned.push_back(fresh);
  return 0;
}

// The embedder's post-pooling head (vr_encoder_set_head), as the two calls above: every check runs, and every weight is
// on the device, before anything changes; the captured graphs hold the weights' pointers and the launch list, so they go.
int encoder_set_head(vr_engine* e, const vr_head_stage* stages, int n_stages, int truncate_dim, int mem) {
  Encoder* enc = static_cast<Encoder*>(e->encoder);
  VR_CHECK(enc, "no encoder loaded");
  VR_CHECK(n_stages >= 0 && n_stages <= kMaxHeadStages, "%d head stages (0..%d allowed)", n_stages, kMaxHeadStages);
  VR_CHECK(n_stages == 0 || stages, "null stages");
  const bool remove = !stages && truncate_dim == 0;
  auto width_ok = [](int w) { return w >= 16 && w <= kMaxHeadWidth && w % 16 == 0; };
  int width = enc->d.hidden;
  VR_CHECK(remove || width_ok(width), "a head needs an encoder width that is a multiple of 16 in 16..1024 (%d)", width);
  for (int s = 0; s < n_stages; ++s) {
    const vr_head_stage& st = stages[s];
    VR_CHECK(st.struct_size == static_cast<int32_t>(sizeof(vr_head_stage)), "stage %d: vr_head_stage size mismatch", s);
    VR_CHECK(st.kind == VR_HEAD_DENSE || st.kind == VR_HEAD_LAYERNORM, "stage %d: unknown kind %d", s, st.kind);
    VR_CHECK(width_ok(st.in_dim) && width_ok(st.out_dim),
             "stage %d: widths %d -> %d must be multiples of 16 in 16..1024", s, st.in_dim, st.out_dim);
    VR_CHECK(st.in_dim == width, "stage %d reads %d columns, %s has %d", s, st.in_dim,
             s == 0 ? "the encoder" : "the stage before it", width);
    VR_CHECK(st.weight, "stage %d: null weight", s);
    if (st.kind == VR_HEAD_DENSE) {
      VR_CHECK(st.activation == VR_ACT_IDENTITY || st.activation == VR_ACT_TANH, "stage %d: unknown activation %d", s,
               st.activation);
    } else {
      VR_CHECK(st.in_dim == st.out_dim, "stage %d: a LayerNorm keeps its width (%d -> %d)", s, st.in_dim, st.out_dim);
      VR_CHECK(st.eps > 0.0f, "stage %d: LayerNorm eps %g must be positive", s, static_cast<double>(st.eps));
    }
    width = st.out_dim;
  }
  VR_CHECK(truncate_dim == 0 || (truncate_dim >= 16 && truncate_dim % 16 == 0 && truncate_dim <= width),
           "truncate_dim %d must be 0 or a multiple of 16 in 16..%d", truncate_dim, width);
  HeadParams hp{};
  std::vector<float*> fresh;
  auto upload = [&](const float* src, size_t n, const float** dst) -> hipError_t {
    float* p = nullptr;
    hipError_t err = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(float));
    if (err != hipSuccess) return err;
    fresh.push_back(p);
    *dst = p;
    return hipMemcpyAsync(p, src, n * sizeof(float), mem == VR_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice,
                          e->stream);
  };
  hipError_t err = hipSuccess;
  for (int s = 0; s < n_stages && err == hipSuccess; ++s) {
    const vr_head_stage& st = stages[s];
    HeadStage& h = hp.st[s];
    h = HeadStage{st.kind, st.in_dim, st.out_dim, st.activation, st.eps, nullptr, nullptr};
    const size_t nw = st.kind == VR_HEAD_DENSE ? static_cast<size_t>(st.in_dim) * st.out_dim : static_cast<size_t>(st.in_dim);
    err = upload(st.weight, nw, &h.w);
    if (err == hipSuccess && st.bias) err = upload(st.bias, static_cast<size_t>(st.out_dim), &h.b);
  }
  hp.n_stages = n_stages;
  // (the sources may go; passes that read the old head are over)
  if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
  // embed_head_kernel's LDS at the widest Dense is past the 64 KiB a launch gets unasked: allowed once, whatever this head is
  static const hipError_t lds_allowed =
      hipFuncSetAttribute(reinterpret_cast<const void*>(&embed_head_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          static_cast<int>(head_lds_bytes(kMaxHeadWidth + 4)));
  if (err == hipSuccess) err = lds_allowed;
  if (err != hipSuccess) {
    for (float* p : fresh) (void)hipFree(p);
    VR_HIP(err);
  }
  invalidate_graphs(enc);
  for (int s = 0; s < enc->head.n_stages; ++s)
    for (const float* old : {enc->head.st[s].w, enc->head.st[s].b})
      if (old) {
        enc->owned.erase(std::remove(enc->owned.begin(), enc->owned.end(), old), enc->owned.end());
        (void)hipFree(const_cast<float*>(old));
      }
  enc->head = hp;
  enc->has_head = !remove;
  enc->out_dim = truncate_dim ? truncate_dim : width;
  enc->owned.insert(enc->owned.end(), fresh.begin(), fresh.end());
  return 0;
}

int encoder_out_dim(vr_engine* e) {
  Encoder* enc = static_cast<Encoder*>(e->encoder);
  return enc ? out_width(enc) : 0;
}

int reranker_load(vr_engine* e, const vr_bert_desc* d_in, const void* const* t, int n_tensors, int mem) {
  vr_bert_desc desc;
  int32_t causal = 0, head_dim = 0, qk_norm = 0;
  VR_TRY(read_desc(d_in, &desc, &causal, &head_dim, &qk_norm));
  const vr_bert_desc* d = &desc;
  VR_CHECK(causal == 0, "a reranker takes no causal mask (causal %d)", causal);
  VR_CHECK(head_dim == 0, "a reranker takes no head size of its own (head_dim %d)", head_dim);
  VR_CHECK(qk_norm == 0, "a reranker takes no query / key norms (qk_norm %d)", qk_norm);
  // a pre-norm, rotary, gated description is a ModernBERT cross-encoder: its own head (6 tensors), CLS or mean pooling
  const bool modern = d->norm == VR_NORM_PRE && d->position == VR_POS_ROTARY && d->ffn != VR_FFN_GELU;
  VR_CHECK(d->norm != VR_NORM_PRE_RMS, "a reranker with norm VR_NORM_PRE_RMS is not supported (norm %d): T5 cross-encoders "
           "are not implemented", d->norm);
  VR_CHECK(d->norm != VR_NORM_PRE_RMS_ROTARY, "a reranker with norm VR_NORM_PRE_RMS_ROTARY is not supported (norm %d): decoder "
           "cross-encoders are not implemented", d->norm);
  if (!modern) {
    VR_CHECK(d->position == VR_POS_LEARNED && d->ffn == VR_FFN_GELU,
             "a reranker with rotary positions or a gated FFN is not supported (position %d, ffn %d): cross-encoders are "
             "BERT, XLM-RoBERTa or (pre-norm) ModernBERT models", d->position, d->ffn);
    VR_CHECK(d->norm == VR_NORM_POST && d->window == 0,
             "a reranker with norm %d or window %d is not supported: pre-norm and sliding-window cross-encoders need "
             "rotary positions and a gated FFN", d->norm, d->window);
    VR_CHECK(d->pooling == VR_POOL_CLS && d->normalize == 0, "a reranker pools the [CLS] row (pooling 1) without normalising");
  } else {
    VR_CHECK(d->pooling != VR_POOL_LAST, "a reranker pools the [CLS] row or the mean (pooling %d): last-token pooling is the "
             "embedder's", d->pooling);
    VR_CHECK(d->normalize == 0, "a reranker pools without normalising (normalize %d)", d->normalize);
    VR_CHECK(d->type_vocab == 1, "a pre-norm reranker has one token type (type_vocab %d)", d->type_vocab);
  }
  // two token types (BERT: segment B reads type row 1), or one (XLM-R: every token reads row 0, seg_b is not used)
  VR_CHECK(d->type_vocab >= 1, "a reranker needs a token type (type_vocab %d)", d->type_vocab);
  const int n_head = modern ? 6 : 4, per_layer = modern ? 18 : 16;
  VR_CHECK(d->layers >= 1 && n_tensors == 5 + per_layer * d->layers + n_head, "expected %d tensors, got %d",
           5 + per_layer * d->layers + n_head, n_tensors);
  for (int i = 0; i < n_head; ++i) VR_CHECK(t[n_tensors - n_head + i] != nullptr, "tensor %d is null", n_tensors - n_head + i);
  VR_TRY(build_encoder(e, &e->reranker, d, t, n_tensors - n_head, mem));
  Encoder* enc = static_cast<Encoder*>(e->reranker);
  const int H = d->hidden;
  const void* const* h = t + n_tensors - n_head;
  const int rc = [&]() -> int {
    // post-norm: pooler.dense w, b, classifier w, b. Pre-norm: head.dense w, b, head.norm w, b, classifier w, b
    VR_TRY(dev_alloc_copy(e, enc, h[0], static_cast<size_t>(H) * H, mem, &enc->pool_w));
    VR_TRY(dev_alloc_copy(e, enc, h[1], H, mem, &enc->pool_b));
    if (modern) {
      VR_TRY(dev_alloc_copy(e, enc, h[2], H, mem, &enc->head_ln_g));
      VR_TRY(dev_alloc_copy(e, enc, h[3], H, mem, &enc->head_ln_b));
    }
    VR_TRY(dev_alloc_copy(e, enc, h[n_head - 2], H, mem, &enc->cls_w));
    VR_TRY(dev_alloc_copy(e, enc, h[n_head - 1], 1, mem, &enc->cls_b));
    VR_HIP(hipStreamSynchronize(e->stream));
    return 0;
  }();
  if (rc != 0) free_encoder(&e->reranker);
  return rc;
}

// vr_reranker_load_decoder: the VR_NORM_PRE_RMS_ROTARY body as build_encoder takes it, pooled at the last token, and one
// head tensor, score.weight [1, H]. Every check — these and build_encoder's own — runs before the slot is touched.
int reranker_load_decoder(vr_engine* e, const vr_bert_desc* d_in, const void* const* t, int n_tensors, int mem) {
  vr_bert_desc desc;
  int32_t causal = 0, head_dim = 0, qk_norm = 0;
  VR_TRY(read_desc(d_in, &desc, &causal, &head_dim, &qk_norm));
  const vr_bert_desc* d = &desc;
  VR_CHECK(d->norm == VR_NORM_PRE_RMS_ROTARY, "a decoder reranker needs norm VR_NORM_PRE_RMS_ROTARY (norm %d): every other "
           "cross-encoder loads through vr_reranker_load", d->norm);
  VR_CHECK(d->position == VR_POS_ROTARY, "a decoder reranker needs position VR_POS_ROTARY (position %d)", d->position);
  VR_CHECK(d->ffn == VR_FFN_SWIGLU || d->ffn == VR_FFN_GEGLU, "a decoder reranker needs a gated ffn (ffn %d): VR_FFN_SWIGLU or "
           "VR_FFN_GEGLU", d->ffn);
  VR_CHECK(d->pooling == VR_POOL_LAST, "a decoder reranker reads the last token's row (pooling %d): VR_POOL_LAST", d->pooling);
  VR_CHECK(d->normalize == 0, "a decoder reranker pools without normalising (normalize %d)", d->normalize);
  VR_CHECK(d->type_vocab == 1, "a decoder reranker has one token type (type_vocab %d)", d->type_vocab);
  VR_CHECK(qk_norm == 0 || qk_norm == 1, "qk_norm %d must be 0 or 1", qk_norm);
  const int per_layer = qk_norm == 1 ? 20 : 18;
  VR_CHECK(d->layers >= 1 && n_tensors == 5 + per_layer * d->layers + 1, "expected %d tensors, got %d",
           5 + per_layer * d->layers + 1, n_tensors);
  VR_CHECK(t[n_tensors - 1] != nullptr, "tensor %d is null", n_tensors - 1);
  VR_TRY(build_encoder(e, &e->reranker, d_in, t, n_tensors - 1, mem));
  Encoder* enc = static_cast<Encoder*>(e->reranker);
  const int rc = [&]() -> int {
    VR_TRY(dev_alloc_copy(e, enc, t[n_tensors - 1], d->hidden, mem, &enc->score_w));
    VR_HIP(hipStreamSynchronize(e->stream));
    return 0;
  }();
  if (rc != 0) free_encoder(&e->reranker);
  return rc;
}

bool reranker_loaded(vr_engine* e) { return e->reranker != nullptr; }

static int ensure_workspace(vr_engine* e, Encoder* enc, int64_t tokens) {
  if (tokens <= enc->ws_tokens) return 0;
  // Headroom: batches of the same chunk count differ by a per cent or two in tokens, and a workspace that fits the
  // largest batch SO FAR exactly is freed and reallocated (gigabytes, with a device synchronisation) every time a
  // slightly longer one arrives — 200 ms per step at the bge-large shape. A sixteenth more, in whole 4096-token units.
  if (tokens > 4096) tokens = (tokens + tokens / 16 + 4095) / 4096 * 4096;
  VR_HIP(hipStreamSynchronize(e->stream));
  invalidate_graphs(enc);
  for (float** p : {&enc->x, &enc->qkv, &enc->ctx, &enc->tmp, &enc->ffn, &enc->xs, &enc->lnstat, &enc->lnpart, &enc->glu, &enc->posidx}) {
    if (*p) {
      enc->owned.erase(std::remove(enc->owned.begin(), enc->owned.end(), *p), enc->owned.end());
      (void)hipFree(*p);
      *p = nullptr;
    }
  }
  const size_t H = static_cast<size_t>(enc->d.hidden), I = static_cast<size_t>(enc->d.intermediate);
  const size_t A = static_cast<size_t>(enc->attn);  // the attention width: H for every family but Qwen3 (vr_bert_desc_v3.head_dim)
  const size_t T = static_cast<size_t>(tokens);
  VR_TRY(dev_alloc_copy(e, enc, nullptr, T * H, 0, &enc->x));
  VR_TRY(dev_alloc_copy(e, enc, nullptr, T * 3 * A, 0, &enc->qkv));
  // (the context, A wide — and in f32 mode the normalised rows a projection reads, H wide)
  VR_TRY(dev_alloc_copy(e, enc, nullptr, T * std::max(A, H), 0, &enc->ctx));
  VR_TRY(dev_alloc_copy(e, enc, nullptr, T * H, 0, &enc->tmp));
  VR_TRY(dev_alloc_copy(e, enc, nullptr, T * I, 0, &enc->ffn));
  if (enc->d.precision != VR_PRECISION_F32) VR_TRY(dev_alloc_copy(e, enc, nullptr, T * H, 0, &enc->xs));
  if (enc->d.precision == VR_PRECISION_F16) VR_TRY(dev_alloc_copy(e, enc, nullptr, T * 4, 0, &enc->lnstat));
  if (enc->d.precision == VR_PRECISION_F16) VR_TRY(dev_alloc_copy(e, enc, nullptr, T * ((H + 63) / 64) * 2, 0, &enc->lnpart));
  if (enc->d.position == VR_POS_ROTARY) VR_TRY(dev_alloc_copy(e, enc, nullptr, T, 0, &enc->posidx));
  // (enc->glu, the gated FFN's pre-activation, is allocated by forward_chunk when a pass is about to store one)
  enc->ws_tokens = tokens;
  return 0;
}

// One layer's attention over the Q/K/V rows in enc->qkv into enc->ctx, for sequences [seq0, seq0 + n_seq). tail: only the
// query block that holds token 0 of every sequence (the CLS tail of forward_chunk). window: 0, or the half-width of a
// windowed layer.
static int launch_attention(vr_engine* e, Encoder* enc, const int32_t* cu_dev, int seq0, int n_seq, int tok_base,
                            int max_len, bool tail, int window, double attn_flop) {
  const vr_bert_desc& d = enc->d;
  // (H: the width of a third of the Q/K/V row and of the context row — the attention width, the hidden size for
  // every family but Qwen3; dh: the head size, hidden / heads unless vr_bert_desc_v3.head_dim says otherwise)
  const int H = enc->attn, nh = d.heads, dh = enc->dh;
  hipStream_t s = e->stream;
  const bool split = d.precision != VR_PRECISION_F32;
  const bool plain = d.precision == VR_PRECISION_F16;
  half_t* ch = split ? reinterpret_cast<half_t*>(enc->ctx) : nullptr;
  half_t* cl = split && !plain ? ch + 8 : nullptr;
  const int qblocks = (max_len + 63) / 64;
  const float scale = 1.0f / sqrtf(static_cast<float>(dh));
  // the kernels' WIN and BIAS flags: a launch without a window or a bias instantiates the code that never knew one
  // (never both: vr_encoder_set_attention_bias / _slopes refuse VR_NORM_PRE, and only that norm has a window; the
  // table of a VR_NORM_PRE_RMS model, T5's, meets none). BIAS: none, the table, or the slopes, which travel in the table's argument (the radius is unused then)
  const float* bias = enc->bias ? enc->bias : enc->slopes;
  const bool table = enc->bias != nullptr;
  const int radius = enc->bias_radius;
  VR_CHECK(!(bias && window > 0), "an attention bias and a window %d cannot meet", window);
  // (the causal mask is BIAS_KIND's fourth state: its norm, VR_NORM_PRE_RMS_ROTARY, has no window and takes no bias)
  VR_CHECK(!(enc->causal && (bias || window > 0)), "a causal mask meets neither a bias nor a window %d", window);
  // head size 128 (vr_bert_desc_v3.head_dim: VR_NORM_PRE_RMS_ROTARY alone reaches it) exists in that norm's two states
  VR_CHECK(dh != 128 || !(bias || window > 0), "head size 128 meets neither a bias nor a window %d", window);
  auto plain_or_causal = [&](auto launch) {
    if (enc->causal) launch(std::integral_constant<int, kMaskCausal>{});
    else launch(std::integral_constant<int, kBiasNone>{});
  };
  auto windowed = [&](auto launch) {
    if (enc->causal) launch(std::false_type{}, std::integral_constant<int, kMaskCausal>{});
    else if (table) launch(std::false_type{}, std::integral_constant<int, kBiasTable>{});
    else if (bias) launch(std::false_type{}, std::integral_constant<int, kBiasSlopes>{});
    else if (window > 0) launch(std::true_type{}, std::integral_constant<int, kBiasNone>{});
    else launch(std::false_type{}, std::integral_constant<int, kBiasNone>{});
  };
  const int qb = tail ? 1 : qblocks;  // tail: only the query block that holds token 0 of every sequence
  dim3 agrid(static_cast<unsigned>(n_seq * qb), static_cast<unsigned>(nh));
  prof_begin(e, VR_PROF_ATTENTION, tail ? attn_flop / qblocks : attn_flop);
  // f16 mode: one block per (sequence, head) with the sequence's K/V staged once in dynamic LDS (attention_seq_kernel)
  // while the longest sequence's rows fit what a workgroup may have on this device; beyond that (max_pos admits up
  // to 8192 tokens) attention_stream_kernel, which streams the keys in 64-row tiles through static LDS
  const int lds_keys = (max_len + 15) & ~15;
  // (a bias table: the head's row behind the staged rows — the staged-or-streamed decision counts it; slopes add no byte)
  const size_t lds_bytes = static_cast<size_t>(2) * lds_keys * dh * sizeof(half_t) + (table ? (2 * radius + 1) * sizeof(float) : 0);
  static size_t lds_limit = 0;
  if (plain && lds_limit == 0) {
    hipDeviceProp_t prop;
    VR_HIP(hipGetDeviceProperties(&prop, e->device));
    lds_limit = std::max(prop.sharedMemPerBlock, prop.sharedMemPerBlockOptin);
  }
  // (a windowed layer: the streamed kernel from enc->window_stream_from tokens on, see build_encoder)
  if (plain && lds_bytes <= lds_limit && !(window > 0 && max_len >= enc->window_stream_from)) {
    static size_t lds_allowed[3] = {0, 0, 0};  // per instantiation: raised above the 64 KiB default when a sequence needs it
    const int which = dh == 64 ? 0 : dh == 32 ? 1 : 2;
    if (lds_bytes > 65536 && lds_bytes > lds_allowed[which]) {
      for (const void* f : {reinterpret_cast<const void*>(&attention_seq_kernel<128, 4, false, kBiasNone>),
                            reinterpret_cast<const void*>(&attention_seq_kernel<128, 4, false, kMaskCausal>)})
        if (dh == 128) VR_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds_bytes)));
      for (const void* f : {reinterpret_cast<const void*>(&attention_seq_kernel<64, 4, false, kBiasNone>),
                            reinterpret_cast<const void*>(&attention_seq_kernel<64, 4, true, kBiasNone>),
                            reinterpret_cast<const void*>(&attention_seq_kernel<64, 4, false, kBiasTable>),
                            reinterpret_cast<const void*>(&attention_seq_kernel<64, 4, false, kBiasSlopes>),
                            reinterpret_cast<const void*>(&attention_seq_kernel<64, 4, false, kMaskCausal>)})
        if (dh == 64) VR_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds_bytes)));
      for (const void* f : {reinterpret_cast<const void*>(&attention_seq_kernel<32, 4, false, kBiasNone>),
                            reinterpret_cast<const void*>(&attention_seq_kernel<32, 4, true, kBiasNone>),
                            reinterpret_cast<const void*>(&attention_seq_kernel<32, 4, false, kBiasTable>),
                            reinterpret_cast<const void*>(&attention_seq_kernel<32, 4, false, kBiasSlopes>),
                            reinterpret_cast<const void*>(&attention_seq_kernel<32, 4, false, kMaskCausal>)})
        if (dh == 32) VR_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds_bytes)));
      lds_allowed[which] = lds_bytes;
    }
    const dim3 sgrid(static_cast<unsigned>(n_seq) * static_cast<unsigned>(nh));
    const int q_limit = tail ? 16 : max_len;
    if (dh == 128)
      plain_or_causal([&](auto B) {
        hipLaunchKernelGGL((attention_seq_kernel<128, 4, false, decltype(B)::value>), sgrid, dim3(256), lds_bytes, s,
                           reinterpret_cast<const half_t*>(enc->qkv), cu_dev, seq0, tok_base, H, scale, q_limit, lds_keys, ch, 0, bias, radius);
      });
    else windowed([&](auto W, auto B) {
      constexpr bool kWin = decltype(W)::value;
      constexpr int kBias = decltype(B)::value;
      if (dh == 64)
        hipLaunchKernelGGL((attention_seq_kernel<64, 4, kWin, kBias>), sgrid, dim3(256), lds_bytes, s, reinterpret_cast<const half_t*>(enc->qkv),
                           cu_dev, seq0, tok_base, H, scale, q_limit, lds_keys, ch, window, bias, radius);
      else
        hipLaunchKernelGGL((attention_seq_kernel<32, 4, kWin, kBias>), sgrid, dim3(256), lds_bytes, s, reinterpret_cast<const half_t*>(enc->qkv),
                           cu_dev, seq0, tok_base, H, scale, q_limit, lds_keys, ch, window, bias, radius);
    });
  } else if (plain) {  // 128 queries per block
    const int qb128 = tail ? 1 : (max_len + 127) / 128;
    const dim3 sgrid(static_cast<unsigned>(n_seq) * static_cast<unsigned>(qb128) * static_cast<unsigned>(nh));
    const int q_limit = tail ? 16 : max_len;
    if (dh == 128)
      plain_or_causal([&](auto B) {
        hipLaunchKernelGGL((attention_stream_kernel<128, 4, false, decltype(B)::value>), sgrid, dim3(256), 0, s,
                           reinterpret_cast<const half_t*>(enc->qkv), cu_dev, seq0, tok_base, H, qb128, scale, q_limit, ch, 0, bias, radius);
      });
    else windowed([&](auto W, auto B) {
      constexpr bool kWin = decltype(W)::value;
      constexpr int kBias = decltype(B)::value;
      if (dh == 64)
        hipLaunchKernelGGL((attention_stream_kernel<64, 4, kWin, kBias>), sgrid, dim3(256), 0, s, reinterpret_cast<const half_t*>(enc->qkv),
                           cu_dev, seq0, tok_base, H, qb128, scale, q_limit, ch, window, bias, radius);
      else
        hipLaunchKernelGGL((attention_stream_kernel<32, 4, kWin, kBias>), sgrid, dim3(256), 0, s, reinterpret_cast<const half_t*>(enc->qkv),
                           cu_dev, seq0, tok_base, H, qb128, scale, q_limit, ch, window, bias, radius);
    });
  } else {
    if (dh == 128) {  // its two tiles as dynamic LDS, above the 64 KiB default: allowed once per instantiation
      static bool lds128_allowed = false;
      if (!lds128_allowed) {
        for (const void* f : {reinterpret_cast<const void*>(&attention_kernel<128, false, kBiasNone>),
                              reinterpret_cast<const void*>(&attention_kernel<128, false, kMaskCausal>)})
          VR_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kAttnF32Lds128)));
        lds128_allowed = true;
      }
      plain_or_causal([&](auto B) {
        hipLaunchKernelGGL((attention_kernel<128, false, decltype(B)::value>), agrid, dim3(256), kAttnF32Lds128, s, enc->qkv, cu_dev, seq0,
                           tok_base, H, qb, scale, enc->ctx, ch, cl, 0, bias, radius);
      });
    } else
    windowed([&](auto W, auto B) {
      constexpr bool kWin = decltype(W)::value;
      constexpr int kBias = decltype(B)::value;
      if (dh == 64)
        hipLaunchKernelGGL((attention_kernel<64, kWin, kBias>), agrid, dim3(256), 0, s, enc->qkv, cu_dev, seq0, tok_base, H, qb, scale,
                           enc->ctx, ch, cl, window, bias, radius);
      else
        hipLaunchKernelGGL((attention_kernel<32, kWin, kBias>), agrid, dim3(256), 0, s, enc->qkv, cu_dev, seq0, tok_base, H, qb, scale,
                           enc->ctx, ch, cl, window, bias, radius);
    });
  }
  prof_end(e);
  VR_HIP(hipGetLastError());
  return 0;
}

// The checked spans of a span call: span_off on the host (forward_all cuts the span range of a forward chunk from it),
// the (begin, end) pairs and the sequence index of every span on the device.
struct Spans {
  std::vector<int32_t> off;
  const int32_t* tok_dev = nullptr;
  const int32_t* seq_dev = nullptr;
  const struct Semantic* sem = nullptr;  // a semantic call: the spans are units, the rows are their chunks'
};

// What a semantic call (encoder_encode_semantic) adds to its units: the rule's parameters and the device arrays of
// launch_semantic — unit_off, the outputs per unit (dist, start) and the working arrays (Encoder::sem_*)
struct Semantic {
  SemanticParams p;
  const int32_t* off_dev;
  float *sums, *dist, *rows;
  int32_t *start, *idx, *seq_chunks, *seq_base, *counter;
};

// launch_pool's arm of a semantic call: the units of sequences [seq0, seq1) summed from x, their gap distances, the
// boundaries of every sequence, and the rows of the chunks that result at out_dev[counter ..], the counter running on
// through the forward chunks of the call. With stages the means go through enc->pooled and embed_head_kernel as a span
// call's do — one row per UNIT (the chunk count is the device's to know), the rows of chunk starts gathered after.
static void launch_semantic(vr_engine* e, Encoder* enc, const float* x, const int32_t* cu_dev, int seq0, int seq1, int tok_base,
                            float* out_dev, const Spans* sp) {
  const vr_bert_desc& d = enc->d;
  const Semantic& m = *sp->sem;
  const int H = d.hidden, W = out_width(enc);
  const bool staged = enc->head.n_stages > 0;
  const int unit0 = sp->off[static_cast<size_t>(seq0)];
  const int n_units = sp->off[static_cast<size_t>(seq1)] - unit0;
  if (n_units <= 0) return;
  const dim3 per_unit(static_cast<unsigned>(n_units)), block(256);
  hipStream_t s = e->stream;
  hipLaunchKernelGGL(unit_sum_kernel, per_unit, block, 0, s, x, cu_dev, sp->tok_dev, sp->seq_dev, unit0, tok_base, H, m.sums);
  hipLaunchKernelGGL(unit_gap_kernel, per_unit, block, 0, s, m.sums, m.off_dev, sp->seq_dev, unit0, H, m.p.buffer, m.dist);
  hipLaunchKernelGGL(unit_boundary_kernel, dim3(static_cast<unsigned>(seq1 - seq0)), block, 0, s, m.dist, m.off_dev, sp->tok_dev,
                     seq0, m.p, m.start, m.idx, m.seq_chunks);
  hipLaunchKernelGGL(chunk_base_kernel, dim3(1), block, 0, s, m.seq_chunks, seq0, seq1 - seq0, m.seq_base, m.counter);
  if (!staged) {
    hipLaunchKernelGGL(chunk_row_kernel, per_unit, block, 0, s, m.sums, m.off_dev, sp->tok_dev, sp->seq_dev, m.start, m.idx,
                       m.seq_base, unit0, H, d.normalize, 0, out_dev, W, W);
    return;
  }
  hipLaunchKernelGGL(chunk_row_kernel, per_unit, block, 0, s, m.sums, m.off_dev, sp->tok_dev, sp->seq_dev, m.start, m.idx,
                     m.seq_base, unit0, H, 0, 1, enc->pooled.p, H, H);
  hipLaunchKernelGGL(embed_head_kernel, dim3(static_cast<unsigned>((n_units + 15) / 16)), block, head_lds_bytes(head_lda(enc->head)),
                     s, enc->pooled.p + static_cast<int64_t>(unit0) * H, n_units, H, enc->head, d.normalize, head_lda(enc->head),
                     m.rows + static_cast<int64_t>(unit0) * W, W, W);
  hipLaunchKernelGGL(chunk_gather_kernel, per_unit, block, 0, s, m.rows, sp->seq_dev, m.start, m.idx, m.seq_base, unit0, W, out_dev);
}

// The last launches of a forward chunk: the rows of sequences [seq0, seq1) — or of their spans (sp) — pooled from x
// into out_dev, one row of out_width() floats each at its sequence's (span's) index. Without a head that is the pool
// kernel alone, as ever. A head without stages only narrows what the pool kernel stores. With stages the pool kernel
// leaves the un-normalised rows in enc->pooled (sized by the caller, same row indices) and embed_head_kernel finishes
// the chunk's rows, 16 per block counted from the chunk's first row. Spans that are the units of a semantic call
// (sp->sem) become the rows of their chunks instead: launch_semantic.
static void launch_pool(vr_engine* e, Encoder* enc, const float* x, const int32_t* cu_dev, int seq0, int seq1, int tok_base,
                        int compact, float* out_dev, const Spans* sp) {
  const vr_bert_desc& d = enc->d;
  const int H = d.hidden, W = out_width(enc);
  const bool staged = enc->head.n_stages > 0;
  float* dst = staged ? enc->pooled.p : out_dev;
  const int stride = staged ? H : W, cols = staged ? H : W, normalize = staged ? 0 : d.normalize;
  int row0 = seq0, n_rows = seq1 - seq0;
  if (sp && sp->sem) return launch_semantic(e, enc, x, cu_dev, seq0, seq1, tok_base, out_dev, sp);
  if (sp) {
    row0 = sp->off[static_cast<size_t>(seq0)];
    n_rows = sp->off[static_cast<size_t>(seq1)] - row0;
    if (n_rows <= 0) return;
    hipLaunchKernelGGL(span_pool_kernel, dim3(static_cast<unsigned>(n_rows)), dim3(256), 0, e->stream, x, cu_dev, sp->tok_dev,
                       sp->seq_dev, row0, tok_base, H, normalize, dst, stride, cols);
  } else {
    hipLaunchKernelGGL(pool_kernel, dim3(static_cast<unsigned>(n_rows)), dim3(256), 0, e->stream, x, cu_dev, seq0, tok_base, H,
                       d.pooling, normalize, compact, dst, stride, cols);
  }
  if (staged)
    hipLaunchKernelGGL(embed_head_kernel, dim3(static_cast<unsigned>((n_rows + 15) / 16)), dim3(256),
                       head_lds_bytes(head_lda(enc->head)), e->stream, enc->pooled.p + static_cast<int64_t>(row0) * H, n_rows, H,
                       enc->head, d.normalize, head_lda(enc->head), out_dev + static_cast<int64_t>(row0) * W, W, W);
}

// ---- the steps of a forward pass ---------------------------------------------------------------------------------------
// The four forward routines below are built from these: each step chooses its kernel by the model's precision in one
// place. They are host code that only picks a launch; none allocates but Pass::need_glu.

// One activation matrix as a product reads or writes it. f16x3 mode: every GEMM input also exists as interleaved
// (hi, lo) f16 rows (lo = hi + 8, see split_at); f16 mode: plain f16 rows and no lo half; f32 mode: both null, the rows
// are the f32 rows at f. The context and the FFN intermediate are ONLY needed split, so those reuse the f32 buffer.
struct Rows {
  float* f = nullptr;
  half_t *hi = nullptr, *lo = nullptr;
};

// What every step of one forward pass over T packed tokens needs: where it launches, the precision, and the workspace.
struct Pass {
  vr_engine* e;
  Encoder* enc;
  hipStream_t s;
  int T;
  unsigned row_blocks;  // of the kernels that take four rows per block
  bool split, plain;    // f16x3 or f16; f16
  int passes;
  bool rms;             // the pre-norm routines' N: RMSNorm (T5, Qwen) or LayerNorm (ModernBERT)
  int glu_epi;          // the gate of a fused FFN-up epilogue
  Rows ctx, ffn;        // the context and the activation, as the residual projections read them
  half_t *xh, *xl;      // the hidden (or normalised) rows as a product's input, in xs
  half_t* qkvh;         // f16 mode: the Q/K/V rows
  half_t* gluh;         // f16 mode: the [T, 2I] pre-activation of the unfused gate (f16x3, f32: enc->glu as it is)
  const int32_t* posidx;
  float2* stat;         // lnstat. (launch_skinny_ln stores the rows' statistics there; no pre-norm routine reads them)

  Pass(vr_engine* e_, Encoder* enc_, int T_)
      : e(e_), enc(enc_), s(e_->stream), T(T_), row_blocks(blocks4(T_)), split(enc_->d.precision != VR_PRECISION_F32),
        plain(enc_->d.precision == VR_PRECISION_F16), passes(plain ? 1 : 3),
        rms(enc_->d.norm == VR_NORM_PRE_RMS || enc_->d.norm == VR_NORM_PRE_RMS_ROTARY),
        glu_epi(enc_->d.ffn == VR_FFN_SWIGLU ? EPI_SWIGLU_F16 : EPI_GEGLU_F16), ctx(rows(enc_->ctx)), ffn(rows(enc_->ffn)),
        xh(rows(enc_->xs).hi), xl(rows(enc_->xs).lo), qkvh(reinterpret_cast<half_t*>(enc_->qkv)),
        gluh(reinterpret_cast<half_t*>(enc_->glu)), posidx(reinterpret_cast<const int32_t*>(enc_->posidx)),
        stat(reinterpret_cast<float2*>(enc_->lnstat)) {}

  static unsigned blocks4(int M) { return static_cast<unsigned>((M + 3) / 4); }
  // a buffer's rows by precision; f32: where the f32 rows are when they are not in the buffer itself
  Rows rows(float* buf, float* f32 = nullptr) const {
    half_t* hi = split ? reinterpret_cast<half_t*>(buf) : nullptr;
    return {f32 ? f32 : buf, hi, split && !plain ? hi + 8 : nullptr};
  }
  // a product's input in xs; f32 mode: the caller's f32 rows (the hidden state, or the rows a norm wrote into ctx)
  Rows x(float* f32) const { return {f32, xh, xl}; }

  // The [rows, 2I] pre-activation workspace of the unfused gate exists only once a pass really stores one. (Never
  // allocated during a graph capture: a shape runs eagerly first, and a reallocation of the workspace drops both this
  // buffer and the graphs.)
  int need_glu() {
    if (enc->glu) return 0;
    const size_t n = static_cast<size_t>(enc->ws_tokens), I = static_cast<size_t>(enc->d.intermediate);
    VR_TRY(dev_alloc_copy(e, enc, nullptr, plain ? n * I : n * 2 * I, 0, &enc->glu));
    gluh = reinterpret_cast<half_t*>(enc->glu);
    return 0;
  }
};

// out = a W^T + bias, M rows: plain f16 rows in f16 mode, f32 rows otherwise (`out` is the buffer in both cases)
static int project_bias(const Pass& p, const float* w32, const SplitWeight& W, const float* bias, int M, int N, int K, Rows a,
                        float* out) {
  if (p.plain)
    return launch_gemm_f16x3(p.e, p.enc, EPI_BIAS_F16, {.A = a.hi, .W = W, .bias = bias, .Ch = reinterpret_cast<half_t*>(out),
                                                        .M = M, .N = N, .K = K, .passes = 1});
  if (p.split)
    return launch_gemm_f16x3(p.e, p.enc, EPI_BIAS, {.A = a.hi, .A_lo = a.lo, .W = W, .bias = bias, .C = out, .M = M, .N = N,
                                                    .K = K, .passes = p.passes});
  return launch_gemm(p.e, EPI_BIAS, a.f, w32, bias, nullptr, out, M, N, K);
}

// C = R + a W^T + bias, f32 rows (f16x3 and f32 mode, and the pre-norm routines in every mode)
static int project_residual(const Pass& p, const float* w32, const SplitWeight& W, const float* bias, int M, int N, int K, Rows a,
                            const float* R, float* C) {
  if (p.split)
    return launch_gemm_f16x3(p.e, p.enc, EPI_BIAS_RESIDUAL, {.A = a.hi, .A_lo = a.lo, .W = W, .bias = bias, .R = R, .C = C, .M = M,
                                                             .N = N, .K = K, .passes = p.passes});
  return launch_gemm(p.e, EPI_BIAS_RESIDUAL, a.f, w32, bias, R, C, M, N, K);
}

// out = act(a W^T + bias), epi = EPI_BIAS_GELU or EPI_BIAS_RELU: the rows the FFN-down projection reads
static int project_act(const Pass& p, int epi, const float* w32, const SplitWeight& W, const float* bias, int M, int N, int K,
                       Rows a, Rows out) {
  if (p.split)
    return launch_gemm_f16x3(p.e, p.enc, epi, {.A = a.hi, .A_lo = a.lo, .W = W, .bias = bias, .Ch = out.hi, .Cl = out.lo, .M = M,
                                               .N = N, .K = K, .passes = p.passes});
  return launch_gemm(p.e, epi, a.f, w32, bias, nullptr, out.f, M, N, K);
}

// LayerNorm of M f32 rows -> out: the f32 rows and, where out has them, the f16 / (hi, lo) rows
static void layernorm_rows(const Pass& p, const float* in, int M, const float* g, const float* b, Rows out) {
  hipLaunchKernelGGL(layernorm_kernel, dim3(Pass::blocks4(M)), dim3(256), 0, p.s, in, M, p.enc->d.hidden, g, b, p.enc->d.eps,
                     out.f, out.hi, out.lo, static_cast<float2*>(nullptr));
}

// f16 mode: LayerNorm of the T rows -> the plain f16 rows in xs and, where the pointers are not null, the f32 rows and the
// rows' (mean, 1/sigma). (layernorm_f16_kernel and rmsnorm_f16_kernel exist for whole 256-column steps.)
static void layernorm_f16_rows(const Pass& p, const float* in, const float* g, const float* b, float* f32, float2* stat) {
  const int H = p.enc->d.hidden;
  if (H % 256 == 0)
    hipLaunchKernelGGL(layernorm_f16_kernel, dim3(p.row_blocks), dim3(256), 0, p.s, in, p.T, H, g, b, p.enc->d.eps, f32, p.xh, stat);
  else
    hipLaunchKernelGGL(layernorm_kernel, dim3(p.row_blocks), dim3(256), 0, p.s, in, p.T, H, g, b, p.enc->d.eps, f32, p.xh,
                       static_cast<half_t*>(nullptr), stat);
}

// The T rows of h normalised by (g, b) — by g alone under p.rms — as the next product's input: p.x(enc->ctx)
static void norm_rows(const Pass& p, const float* h, const float* g, const float* b) {
  const int H = p.enc->d.hidden;
  float* f32 = p.split ? nullptr : p.enc->ctx;
  if (!p.rms && p.plain)
    layernorm_f16_rows(p, h, g, b, nullptr, nullptr);
  else if (!p.rms)
    layernorm_rows(p, h, p.T, g, b, {f32, p.xh, p.xl});
  else if (p.plain && H % 256 == 0)
    hipLaunchKernelGGL(rmsnorm_f16_kernel, dim3(p.row_blocks), dim3(256), 0, p.s, h, p.T, H, g, p.enc->d.eps, p.xh);
  else
    hipLaunchKernelGGL(rmsnorm_kernel, dim3(p.row_blocks), dim3(256), 0, p.s, h, p.T, H, g, p.enc->d.eps, f32, p.xh, p.xl);
}

// The rotation as a pass of its own: in place on the Q and K parts (`width` columns each) of the T qkv rows
static void rotate_rows(const Pass& p, const float2* table, int width, int dh) {
  if (p.plain)
    hipLaunchKernelGGL(rope_kernel<half_t>, dim3(p.row_blocks), dim3(256), 0, p.s, p.qkvh, p.posidx, p.T, width, dh, table);
  else
    hipLaunchKernelGGL(rope_kernel<float>, dim3(p.row_blocks), dim3(256), 0, p.s, p.enc->qkv, p.posidx, p.T, width, dh, table);
}

// Qwen3: the per-head RMSNorm of Q and K by (qn, kn) and the rotation, one pass over the T qkv rows
static void qk_norm_rotate_rows(const Pass& p, const LayerWeights& w, int width, int dh) {
  if (p.plain)
    hipLaunchKernelGGL(qk_norm_rope_kernel<half_t>, dim3(p.row_blocks), dim3(256), 0, p.s, p.qkvh, p.posidx, p.T, width, dh,
                       p.enc->rope, w.qn, w.kn, p.enc->d.eps);
  else
    hipLaunchKernelGGL(qk_norm_rope_kernel<float>, dim3(p.row_blocks), dim3(256), 0, p.s, p.enc->qkv, p.posidx, p.T, width, dh,
                       p.enc->rope, w.qn, w.kn, p.enc->d.eps);
}

// The unfused gate: M rows of enc->glu -> the FFN-down input, f16 rows (f16), (hi, lo) rows (f16x3) or f32 rows of `out`
static void gate_rows(const Pass& p, int M, Rows out) {
  const int I = p.enc->d.intermediate, ffn = p.enc->d.ffn;
  const int64_t n8 = static_cast<int64_t>(M) * (I / 8);
  const dim3 grid(static_cast<unsigned>((n8 + 255) / 256));
  if (p.plain)
    hipLaunchKernelGGL((glu_kernel<half_t, 2>), grid, dim3(256), 0, p.s, p.gluh, n8, I, ffn, static_cast<float*>(nullptr), out.hi);
  else if (p.split)
    hipLaunchKernelGGL((glu_kernel<float, 1>), grid, dim3(256), 0, p.s, p.enc->glu, n8, I, ffn, static_cast<float*>(nullptr), out.hi);
  else
    hipLaunchKernelGGL((glu_kernel<float, 0>), grid, dim3(256), 0, p.s, p.enc->glu, n8, I, ffn, out.f, static_cast<half_t*>(nullptr));
}

// The gated FFN-up of M input rows -> out. fuse_glu (f16 mode, a product that goes to a skinny kernel): over the
// re-ordered matrix, the gate in the epilogue; otherwise the bias-only product into enc->glu, then the gate pass.
static int gated_up_rows(const Pass& p, const LayerWeights& w, bool fuse_glu, int M, Rows a, Rows out) {
  const int H = p.enc->d.hidden, N1 = 2 * p.enc->d.intermediate;
  if (fuse_glu)
    return launch_gemm_f16x3(p.e, p.enc, p.glu_epi, {.A = a.hi, .W = w.s_1_p, .bias = w.b1_p, .Ch = out.hi, .M = M, .N = N1, .K = H,
                                                     .passes = 1});
  VR_TRY(project_bias(p, w.w1, w.s_1, w.b1, M, N1, H, a, p.enc->glu));
  gate_rows(p, M, out);
  return 0;
}

// The gated FFN-up of N(h) by (g, b) -> p.ffn, pre-norm routines. fold_ln (a question): the norm runs inside the
// projection (launch_skinny_ln); otherwise as a launch of its own ahead of gated_up_rows.
static int gated_up_of_norm(const Pass& p, const LayerWeights& w, bool fold_ln, bool fuse_glu, const float* h, const float* g,
                            const float* b) {
  const int H = p.enc->d.hidden, N1 = 2 * p.enc->d.intermediate;
  const float eps = p.enc->d.eps;
  if (fold_ln && fuse_glu)
    return launch_skinny_ln(p.e, p.glu_epi, h, eps, p.stat,
                            {.W = w.s_1_p, .bias = w.b1_p, .Ch = p.ffn.hi, .M = p.T, .N = N1, .K = H, .ln_g = g, .ln_b = b}, p.rms);
  if (fold_ln) {
    VR_TRY(launch_skinny_ln(p.e, EPI_BIAS_F16, h, eps, p.stat,
                            {.W = w.s_1, .bias = w.b1, .Ch = p.gluh, .M = p.T, .N = N1, .K = H, .ln_g = g, .ln_b = b}, p.rms));
    gate_rows(p, p.T, p.ffn);
    return 0;
  }
  norm_rows(p, h, g, b);
  return gated_up_rows(p, w, fuse_glu, p.T, p.x(p.enc->ctx), p.ffn);
}

// Q, K, V (N columns) of N(h) by (g, b) -> the qkv rows, pre-norm routines; g null (layer 0): the embedding launch
// wrote the normalised rows, f32 mode at a32. fold_ln as above; fuse_rope (f16 mode, a skinny route): the rotation by
// `table` in the epilogue, over the re-ordered matrix — otherwise the caller rotates in a pass of its own.
static int project_qkv(const Pass& p, const LayerWeights& w, int N, bool fold_ln, bool fuse_rope, const float2* table,
                       const float* h, const float* g, const float* b, float* a32) {
  const int H = p.enc->d.hidden;
  if (fold_ln && g) {
    if (fuse_rope)
      return launch_skinny_ln(p.e, EPI_ROPE_F16, h, p.enc->d.eps, p.stat,
                              {.W = w.s_qkv_p, .bias = w.bqkv_p, .Ch = p.qkvh, .M = p.T, .N = N, .K = H, .ln_g = g, .ln_b = b,
                               .rope_tab = table, .rope_pos = p.posidx}, p.rms);
    return launch_skinny_ln(p.e, EPI_BIAS_F16, h, p.enc->d.eps, p.stat,
                            {.W = w.s_qkv, .bias = w.bqkv, .Ch = p.qkvh, .M = p.T, .N = N, .K = H, .ln_g = g, .ln_b = b}, p.rms);
  }
  if (g) norm_rows(p, h, g, b);
  if (fuse_rope)
    return launch_gemm_f16x3(p.e, p.enc, EPI_ROPE_F16, {.A = p.xh, .W = w.s_qkv_p, .bias = w.bqkv_p, .Ch = p.qkvh, .M = p.T, .N = N,
                                                        .K = H, .passes = 1, .rope_tab = table, .rope_pos = p.posidx});
  return project_bias(p, w.wqkv, w.s_qkv, w.bqkv, p.T, N, H, p.x(a32), p.enc->qkv);
}

// The forward pass of a pre-norm model (VR_NORM_PRE: rotary positions, a gated FFN, optionally alternating global and
// windowed attention — the ModernBERT family), forward_chunk's arguments:
//   h = LN_emb(word[id]);  per layer  h += W_o attn(N_a(h)),  h += W_down(act(gate(N_m(h))) * up(N_m(h)));  out = N_f(h)
// with N_a of layer 0 the identity, N_a of layer l > 0 in layer l - 1's output.LayerNorm slot, N_m in the layer's
// attention.output.LayerNorm slot and N_f in the last layer's output.LayerNorm slot (include/voitta_engine.h). The
// residual stream h is f32 and alternates between enc->x and enc->tmp: each projection back into it adds its residual
// in the epilogue (EPI_BIAS_RESIDUAL) and writes the other buffer. Every projection's input is a LayerNorm of h,
// written by a LayerNorm launch as the f16 / (hi, lo) / f32 rows the product reads — or, for a question (<= 16 rows in
// f16 mode), computed inside the projection from h itself (launch_skinny_ln: a folded LayerNorm IS a pre-norm
// projection), which keeps a question at the launch count of a post-norm rotary model. Rotation and gate run in the
// skinny epilogues where forward_chunk runs them there (VR_ENCODE_FUSE=0: passes of their own). None of the post-norm
// loop's LayerNorm folds apply: they exist to re-derive a LayerNorm output for the RESIDUAL, which here is h itself.
static int forward_chunk_prenorm(vr_engine* e, Encoder* enc, const int32_t* ids_dev, const int32_t* cu_dev, int n_seq_total,
                                 int seq0, int seq1, int tok_base, int T, int max_len, double attn_flop, float* out_dev,
                                 const Spans* sp) {
  const vr_bert_desc& d = enc->d;
  const int H = d.hidden, I = d.intermediate, dh = H / d.heads, N1 = 2 * I;
  // GEMM inputs, as in forward_chunk: the normalised rows in xs (f32 mode: in ctx, free until attention writes it and
  // again behind the output projection), the context in ctx, the gated activation in ffn
  Pass p(e, enc, T);
  const bool fuse = p.plain && enc->fuse;
  const bool fold_ln = p.plain && skinny_ln_supported(T, 3 * H, H) && I % 16 == 0;
  const bool fuse_rope = fuse && skinny_routed(T, 3 * H, H);
  const bool fuse_glu = fuse && skinny_routed(T, N1, H);
  if (!fuse_glu) VR_TRY(p.need_glu());
  hipLaunchKernelGGL(embed_ln_rotary_kernel, dim3(p.row_blocks), dim3(256), 0, p.s, ids_dev, cu_dev, n_seq_total, tok_base, T, H,
                     d.vocab, enc->word, enc->type, enc->lng, enc->lnb, d.eps, enc->x, p.xh, p.xl, static_cast<float*>(nullptr),
                     static_cast<float2*>(nullptr));
  hipLaunchKernelGGL(positions_kernel, dim3(static_cast<unsigned>((T + 255) / 256)), dim3(256), 0, p.s, cu_dev, n_seq_total,
                     tok_base, T, reinterpret_cast<int32_t*>(enc->posidx));
  float* h = enc->x;      // the residual stream
  float* other = enc->tmp;
  const int n_seq = seq1 - seq0;
  for (size_t li = 0; li < enc->layers.size(); ++li) {
    const LayerWeights& w = enc->layers[li];
    const LayerWeights* prev = li > 0 ? &enc->layers[li - 1] : nullptr;
    const bool global = d.window == 0 || li % static_cast<size_t>(d.global_every) == 0;
    const float2* table = !global && enc->rope_local ? enc->rope_local : enc->rope;
    // Q, K, V of N_a(h); layer 0 reads the embedding LayerNorm's rows as they are (f32 mode: h itself)
    VR_TRY(project_qkv(p, w, 3 * H, fold_ln, fuse_rope, table, h, prev ? prev->ln2g : nullptr, prev ? prev->ln2b : nullptr,
                       prev ? enc->ctx : h));
    if (!fuse_rope) rotate_rows(p, table, H, dh);  // with the table of the layer's kind
    // (the profiler's flop count of a windowed layer: at most 2 w + 1 keys per query, instead of the sequence's length)
    const double layer_flop = global ? attn_flop : std::min(attn_flop, 4.0 * H * T * (2.0 * d.window + 1.0));
    VR_TRY(launch_attention(e, enc, cu_dev, seq0, n_seq, tok_base, max_len, false, global ? 0 : d.window, layer_flop));
    // h' = h + W_o ctx
    VR_TRY(project_residual(p, w.wo, w.s_o, w.bo, T, H, H, p.ctx, h, other));
    std::swap(h, other);
    // the gated FFN of N_m(h)
    VR_TRY(gated_up_of_norm(p, w, fold_ln, fuse_glu, h, w.ln1g, w.ln1b));
    // h' = h + W_down act
    VR_TRY(project_residual(p, w.w2, w.s_2, w.b2, T, H, I, p.ffn, h, other));
    std::swap(h, other);
  }
  // the final norm writes the f32 rows pooling reads, into the buffer the stream is not in
  layernorm_rows(p, h, T, enc->layers.back().ln2g, enc->layers.back().ln2b, {other});
  launch_pool(e, enc, other, cu_dev, seq0, seq1, tok_base, 0, out_dev, sp);
  VR_HIP(hipGetLastError());
  return 0;
}

// The forward pass of an RMSNorm pre-norm model (VR_NORM_PRE_RMS: no positions, a ReLU FFN without a gate — the T5
// encoder), forward_chunk's arguments:
//   h = word[id];  per layer  h += W_o attn(N_a(h)),  h += W_down relu(W_up N_m(h));  out = N_f(h)
// forward_chunk_prenorm's loop with three differences: the embedding launch leaves the RAW row in the stream and writes
// N_a of layer 0 (the embeddings.LayerNorm slot) for the first projection; there is no rotation; and the FFN is one
// product with the ReLU in its epilogue (EPI_BIAS_RELU) on whichever GEMM route the shape takes. Every N is RMSNorm — a
// launch of its own, or for a question (<= 16 rows in f16 mode) folded into the projection that reads it
// (launch_skinny_ln, rms). The relative-position table reaches the attention kernels through launch_attention as
// MPNet's does; T5's missing 1/sqrt(d_h) is in the query weights (include/voitta_engine.h).
static int forward_chunk_rms(vr_engine* e, Encoder* enc, const int32_t* ids_dev, const int32_t* cu_dev, int n_seq_total,
                             int seq0, int seq1, int tok_base, int T, int max_len, double attn_flop, float* out_dev,
                             const Spans* sp) {
  const vr_bert_desc& d = enc->d;
  const int H = d.hidden, I = d.intermediate;
  // GEMM inputs as in forward_chunk_prenorm: the normalised rows in xs (f32 mode: in ctx), the context in ctx, the
  // activation in ffn
  Pass p(e, enc, T);
  const bool fold_ln = p.plain && skinny_ln_supported(T, 3 * H, H) && I % 16 == 0;
  hipLaunchKernelGGL(embed_rms_kernel, dim3(p.row_blocks), dim3(256), 0, p.s, ids_dev, cu_dev, n_seq_total, tok_base, T, H, d.vocab,
                     enc->word, enc->type, enc->lng, d.eps, p.split ? nullptr : enc->ctx, p.xh, p.xl, enc->x);
  float* h = enc->x;      // the residual stream
  float* other = enc->tmp;
  const int n_seq = seq1 - seq0;
  for (size_t li = 0; li < enc->layers.size(); ++li) {
    const LayerWeights& w = enc->layers[li];
    // Q, K, V of N_a(h); layer 0 reads the rows the embedding launch normalised
    VR_TRY(project_qkv(p, w, 3 * H, fold_ln, false, nullptr, h, li > 0 ? enc->layers[li - 1].ln2g : nullptr, nullptr, enc->ctx));
    VR_TRY(launch_attention(e, enc, cu_dev, seq0, n_seq, tok_base, max_len, false, 0, attn_flop));
    // h' = h + W_o ctx
    VR_TRY(project_residual(p, w.wo, w.s_o, w.bo, T, H, H, p.ctx, h, other));
    std::swap(h, other);
    // relu(W_up N_m(h))
    if (fold_ln) {
      VR_TRY(launch_skinny_ln(e, EPI_BIAS_RELU, h, d.eps, p.stat,
                              {.W = w.s_1, .bias = w.b1, .Ch = p.ffn.hi, .M = T, .N = I, .K = H, .ln_g = w.ln1g}, true));
    } else {
      norm_rows(p, h, w.ln1g, nullptr);
      VR_TRY(project_act(p, EPI_BIAS_RELU, w.w1, w.s_1, w.b1, T, I, H, p.x(enc->ctx), p.ffn));
    }
    // h' = h + W_down act
    VR_TRY(project_residual(p, w.w2, w.s_2, w.b2, T, H, I, p.ffn, h, other));
    std::swap(h, other);
  }
  // the final norm writes the f32 rows pooling reads, into the buffer the stream is not in
  hipLaunchKernelGGL(rmsnorm_kernel, dim3(p.row_blocks), dim3(256), 0, p.s, h, T, H, enc->layers.back().ln2g, d.eps, other,
                     static_cast<half_t*>(nullptr), static_cast<half_t*>(nullptr));
  launch_pool(e, enc, other, cu_dev, seq0, seq1, tok_base, 0, out_dev, sp);
  VR_HIP(hipGetLastError());
  return 0;
}

// A decoder cross-encoder's logit reads one row per pair, the last token's, so everything behind the LAST layer's
// attention runs on n_seq rows instead of T — cls_tail's idea for the pre-norm decoder block. The [n_seq, *] matrices live
// in enc->tail_ws (encoder_rerank sizes it: at one-token pairs they are larger than the qkv buffer cls_tail carves up).
struct RerankRows {
  float *x, *tmp, *xs, *ctx, *ffn;  // residual rows, the stream's other buffer, N(x) as a product reads it, context, activation
  static int64_t floats(const Encoder* enc, int64_t n) {
    return n * (3 * static_cast<int64_t>(enc->d.hidden) + enc->attn + enc->d.intermediate);
  }
  RerankRows(const Encoder* enc, int n_seq) {
    const int64_t n = n_seq, H = enc->d.hidden, A = enc->attn;
    x = enc->tail_ws.p;  // [n_seq, H] f32
    tmp = x + n * H;     // [n_seq, H] f32
    xs = tmp + n * H;    // [n_seq, H] f32, [n_seq, 2H] halfs (f16x3) or [n_seq, H] halfs (f16)
    ctx = xs + n * H;    // [n_seq, A] f32, [n_seq, 2A] halfs or [n_seq, A] halfs
    ffn = ctx + n * A;   // [n_seq, I] likewise
  }
};

// The rest of the last layer of a decoder cross-encoder on the last row of every pair, and the head (vr_reranker_load_decoder):
//   x = h_last + W_o ctx_last;  x = x + W_down(act(gate(N_m(x))) * up(N_m(x)));  logit = score . N_f(x)
// forward_chunk_rms_rotary's steps at M = n_seq: the norm as a launch of its own in every mode, the gate in the FFN-up
// epilogue where that routine fuses it (f16, a skinny product). h: the residual stream going into the last layer, whose
// attention has just written enc->ctx. Writes one logit per sequence at out_dev[seq0 ..].
static int rerank_tail(const Pass& p, const LayerWeights& w, const float* h, const int32_t* cu_dev, int seq0, int seq1,
                       int tok_base, float* out_dev) {
  Encoder* enc = p.enc;
  const vr_bert_desc& d = enc->d;
  const int T = p.T, H = d.hidden, I = d.intermediate, A = enc->attn, n_seq = seq1 - seq0;
  VR_CHECK(enc->tail_ws.cap >= RerankRows::floats(enc, n_seq), "the reranker's tail workspace holds %lld floats, %d pairs need "
           "%lld", static_cast<long long>(enc->tail_ws.cap), n_seq, static_cast<long long>(RerankRows::floats(enc, n_seq)));
  const RerankRows c(enc, n_seq);
  const dim3 gblocks(Pass::blocks4(n_seq));
  hipLaunchKernelGGL(gather_last_rows_kernel, gblocks, dim3(256), 0, p.s, reinterpret_cast<const float4*>(enc->ctx),
                     reinterpret_cast<const float4*>(h), cu_dev, seq0, tok_base, n_seq, T, p.plain ? A / 8 : A / 4, H / 4,
                     reinterpret_cast<float4*>(c.ctx), reinterpret_cast<float4*>(c.x));
  const Rows x = p.rows(c.xs), ctx = p.rows(c.ctx), ffn = p.rows(c.ffn);
  // x' = x + W_o ctx
  VR_TRY(project_residual(p, w.wo, w.s_o, w.bo, n_seq, H, A, ctx, c.x, c.tmp));
  // the gated FFN of N_m(x')
  if (p.plain && H % 256 == 0)
    hipLaunchKernelGGL(rmsnorm_f16_kernel, gblocks, dim3(256), 0, p.s, c.tmp, n_seq, H, w.ln1g, d.eps, x.hi);
  else
    hipLaunchKernelGGL(rmsnorm_kernel, gblocks, dim3(256), 0, p.s, c.tmp, n_seq, H, w.ln1g, d.eps, p.split ? nullptr : x.f, x.hi,
                       x.lo);
  VR_TRY(gated_up_rows(p, w, p.plain && enc->fuse && skinny_routed(n_seq, 2 * I, H), n_seq, x, ffn));
  // x'' = x' + W_down act
  VR_TRY(project_residual(p, w.w2, w.s_2, w.b2, n_seq, H, I, ffn, c.tmp, c.x));
  // the final norm and the dot product with score.weight, one wave per pair
  hipLaunchKernelGGL(rerank_head_rms_kernel, gblocks, dim3(256), 0, p.s, c.x, n_seq, H, w.ln2g, d.eps, enc->score_w,
                     out_dev + seq0);
  VR_HIP(hipGetLastError());
  return 0;
}

// The forward pass of an RMSNorm pre-norm model with rotary positions and a gated FFN (VR_NORM_PRE_RMS_ROTARY: the Llama /
// Qwen2 block, the decoder-style embedders), forward_chunk's arguments:
//   h = word[id];  per layer  h += W_o attn(rope(N_a(h))),  h += W_down(act(gate(N_m(h))) * up(N_m(h)));  out = N_f(h)
// forward_chunk_rms's stream (the embedding launch leaves the RAW row in it and writes N_a of layer 0; every N is RMSNorm,
// a launch of its own or, for a question of <= 16 rows in f16 mode, folded into the projection that reads it) with
// forward_chunk_prenorm's rotation and gate on every route those have: rope_kernel / glu_kernel as passes of their own in
// f32 and f16x3 (and under VR_ENCODE_FUSE=0), in f16 the gate inside the FFN-up epilogues and the rotation inside the
// Q/K/V epilogue of the skinny routes. The causal mask (vr_bert_desc_v2.causal) reaches the attention kernels through
// launch_attention; causal = 0 is the same body run bidirectionally.
static int forward_chunk_rms_rotary(vr_engine* e, Encoder* enc, const int32_t* ids_dev, const int32_t* cu_dev, int n_seq_total,
                                    int seq0, int seq1, int tok_base, int T, int max_len, double attn_flop, float* out_dev,
                                    const Spans* sp) {
  const vr_bert_desc& d = enc->d;
  // A: the attention width — the [Q | K | V] row is 3 A, the context A (A == H but for vr_bert_desc_v3.head_dim)
  const int H = d.hidden, I = d.intermediate, dh = enc->dh, A = enc->attn, N1 = 2 * I;
  const bool qk_norm = enc->qk_norm != 0;
  // GEMM inputs as in forward_chunk_prenorm: the normalised rows in xs (f32 mode: in ctx), the context in ctx, the gated
  // activation in ffn
  Pass p(e, enc, T);
  const bool fuse = p.plain && enc->fuse;
  const bool fold_ln = p.plain && skinny_rms_rotary_supported(T, 3 * A, H) && I % 16 == 0;
  // (the rotating Q/K/V epilogues: not behind a Q/K norm, which needs a whole head before the rotation — those models
  // take the plain epilogues and qk_norm_rope_kernel at every size — and, as they are, at A == H only)
  const bool fuse_rope = fuse && !qk_norm && A == H && skinny_routed(T, 3 * H, H);
  const bool fuse_glu = fuse && skinny_routed(T, N1, H);
  if (!fuse_glu) VR_TRY(p.need_glu());
  hipLaunchKernelGGL(embed_rms_kernel, dim3(p.row_blocks), dim3(256), 0, p.s, ids_dev, cu_dev, n_seq_total, tok_base, T, H, d.vocab,
                     enc->word, enc->type, enc->lng, d.eps, p.split ? nullptr : enc->ctx, p.xh, p.xl, enc->x);
  hipLaunchKernelGGL(positions_kernel, dim3(static_cast<unsigned>((T + 255) / 256)), dim3(256), 0, p.s, cu_dev, n_seq_total,
                     tok_base, T, reinterpret_cast<int32_t*>(enc->posidx));
  float* h = enc->x;      // the residual stream
  float* other = enc->tmp;
  const int n_seq = seq1 - seq0;
  // (a causal pass multiplies about half the logits)
  const double layer_flop = enc->causal ? 0.5 * attn_flop : attn_flop;
  for (size_t li = 0; li < enc->layers.size(); ++li) {
    const LayerWeights& w = enc->layers[li];
    // Q, K, V of N_a(h); layer 0 reads the rows the embedding launch normalised
    VR_TRY(project_qkv(p, w, 3 * A, fold_ln, fuse_rope, enc->rope, h, li > 0 ? enc->layers[li - 1].ln2g : nullptr, nullptr,
                       enc->ctx));
    if (qk_norm) qk_norm_rotate_rows(p, w, A, dh);
    else if (!fuse_rope) rotate_rows(p, enc->rope, A, dh);
    VR_TRY(launch_attention(e, enc, cu_dev, seq0, n_seq, tok_base, max_len, false, 0, layer_flop));
    // (a decoder cross-encoder, vr_reranker_load_decoder: the rest of its last layer on the pairs' last rows, and the head)
    if (enc->score_w && li + 1 == enc->layers.size()) return rerank_tail(p, w, h, cu_dev, seq0, seq1, tok_base, out_dev);
    // h' = h + W_o ctx
    VR_TRY(project_residual(p, w.wo, w.s_o, w.bo, T, H, A, p.ctx, h, other));
    std::swap(h, other);
    // the gated FFN of N_m(h)
    VR_TRY(gated_up_of_norm(p, w, fold_ln, fuse_glu, h, w.ln1g, nullptr));
    // h' = h + W_down act
    VR_TRY(project_residual(p, w.w2, w.s_2, w.b2, T, H, I, p.ffn, h, other));
    std::swap(h, other);
  }
  // the final norm writes the f32 rows pooling reads, into the buffer the stream is not in
  hipLaunchKernelGGL(rmsnorm_kernel, dim3(p.row_blocks), dim3(256), 0, p.s, h, T, H, enc->layers.back().ln2g, d.eps, other,
                     static_cast<half_t*>(nullptr), static_cast<half_t*>(nullptr));
  launch_pool(e, enc, other, cu_dev, seq0, seq1, tok_base, 0, out_dev, sp);
  VR_HIP(hipGetLastError());
  return 0;
}

// forward_chunk's hidden state in f16 mode: LayerNorm by (g, b) of the pre-LN rows `pre`, with the rows' (mean, 1/sigma)
struct Hidden {
  const float* pre;
  const float2* stat;
  const float* g;
  const float* b;
};

// CLS pooling reads one row per sequence, so everything after the LAST layer's attention is needed
// for those rows only: their context rows (and residual rows) are gathered into compact [n_seq, *]
// matrices carved out of the qkv buffer (free once attention has run), and the output projection,
// both LayerNorms and the FFN run on n_seq rows instead of T (cls_tail). Every row's arithmetic is unchanged
// (a GEMM row does not depend on its neighbours), so the embeddings are bit-identical; for
// bge-base this removes 10/12 of the last layer's GEMM work. The Q/K/V projection of all T rows
// (one GEMM) and the attention over them remain on this route; the large f16 batches of `collapse`
// (cls_collapse_attend) replace both, with a workspace behind the tail's.
struct ClsRows {
  float *x, *tmp, *xs, *ctx, *ffn;  // the tail's [n_seq, *] x, tmp, xs, ctx and ffn
  half_t *x16, *q16, *u16, *z16;    // collapse: f16 LN(x) of the [CLS] rows, their queries, u and z [n_seq, nh, H]
  float* gamma;                     // collapse: [n_seq, nh]
  int64_t floats;                   // all of it, from the start of the qkv buffer

  ClsRows(const Encoder* enc, int n_seq) {
    const int64_t n = n_seq, H = enc->d.hidden, I = enc->d.intermediate, nh = enc->d.heads;
    auto up4 = [](int64_t k) { return (k + 3) / 4 * 4; };  // (16-byte aligned pieces)
    x = enc->qkv;        // [n_seq, H] hidden state of the [CLS] rows
    tmp = x + n * H;     // [n_seq, H]
    xs = tmp + n * H;    // [n_seq, 2H] halfs (split) = n_seq*H floats
    ctx = xs + n * H;    // [n_seq, H] f32 or [n_seq, 2H] halfs
    ffn = ctx + n * H;   // [n_seq, I] f32 or [n_seq, 2I] halfs
    x16 = reinterpret_cast<half_t*>(ffn + up4(n * I));
    q16 = x16 + up4(n * H);
    u16 = q16 + up4(n * H);
    z16 = u16 + up4(n * nh * H);
    gamma = reinterpret_cast<float*>(z16 + up4(n * nh * H));
    floats = (gamma + n * nh) - enc->qkv;
  }
};

// `collapse`: the last layer of a [CLS]-pooled model attends from the [CLS] rows on the hidden rows themselves — no Q/K/V
// projection of the T rows, no attention launch over them: steps 1-4 of cls_attend_kernel's comment. Reads the f16
// pre-LayerNorm rows in xs with their statistics (forward_chunk's cur16 state); writes c.x and c.ctx, which cls_tail reads.
static int cls_collapse_attend(const Pass& p, const LayerWeights& w, const Hidden& cur, const ClsRows& c, const int32_t* cu_dev,
                               int seq0, int n_seq, int tok_base, int cls_lpad) {
  vr_engine* e = p.e;
  const int T = p.T, H = p.enc->d.hidden, nh = p.enc->d.heads, dh = H / nh;
  const unsigned mblocks = static_cast<unsigned>((n_seq + 63) / 64);
  hipLaunchKernelGGL(gather_first_rows_ln16_kernel, dim3(Pass::blocks4(n_seq)), dim3(256), 0, p.s, p.xh, cur.stat, cur.g, cur.b,
                     cu_dev, seq0, tok_base, n_seq, T, H, c.x, c.x16);
  VR_TRY(launch_gemm_f16x3(e, p.enc, EPI_BIAS_F16, {.A = c.x16, .W = w.s_qkv, .bias = w.bqkv, .Ch = c.q16, .M = n_seq, .N = H,
                                                    .K = H, .passes = 1}));
  const double head_flop = 2.0 * n_seq * static_cast<double>(H) * H;  // nh products of [n_seq, dh] x [dh, H]
  prof_begin(e, VR_PROF_GEMM, head_flop);
  hipLaunchKernelGGL((cls_head_gemm_kernel<false>), dim3(static_cast<unsigned>(H / 64), mblocks, static_cast<unsigned>(nh)),
                     dim3(256), 0, p.s, w.wk_t, H, static_cast<int64_t>(dh), c.q16, H, dh, n_seq, H, dh, w.s_qkv_f.unscale,
                     static_cast<const float*>(nullptr), static_cast<const float*>(nullptr),
                     static_cast<const float*>(nullptr), c.u16, nh * H, H);
  prof_end(e);
  // two passes over the T rows, 2 H multiply-adds per (token, head) each
  prof_begin(e, VR_PROF_ATTENTION, 4.0 * nh * static_cast<double>(H) * T);
  hipLaunchKernelGGL(cls_attend_kernel, dim3(static_cast<unsigned>(n_seq)), dim3(256), cls_attend_lds(H, cls_lpad), p.s, p.xh,
                     cur.stat, c.u16, cu_dev, seq0, tok_base, T, H, nh, 1.4426950408889634f / sqrtf(static_cast<float>(dh)),
                     cls_lpad, c.z16, c.gamma);
  prof_end(e);
  prof_begin(e, VR_PROF_GEMM, head_flop);
  hipLaunchKernelGGL((cls_head_gemm_kernel<true>), dim3(static_cast<unsigned>((dh + 63) / 64), mblocks, static_cast<unsigned>(nh)),
                     dim3(256), 0, p.s, w.s_qkv_f.hi + static_cast<int64_t>(2) * H * H, H, static_cast<int64_t>(dh) * H, c.z16,
                     nh * H, H, n_seq, dh, H, w.s_qkv_f.unscale, w.cs_qkv + 2 * H, w.c_qkv + 2 * H, c.gamma,
                     reinterpret_cast<half_t*>(c.ctx), H, dh);
  prof_end(e);
  return 0;
}

// The rest of the last layer of a [CLS]-pooled post-norm model, on the n_seq [CLS] rows only (ClsRows), and the pooling:
//   x = LN_1(x + W_o ctx);  x = LN_2(x + W_down act(W_up x))  — forward_chunk's f32 / f16x3 layer at M = n_seq, in every
// mode. `gathered` (collapse): c.x and c.ctx are written already; otherwise the context rows come from enc->ctx and the
// hidden rows from wherever the mode keeps them (f16: LayerNorm of the pre-LN rows — f32 ones, or with cur16 the f16 rows in xs).
static int cls_tail(const Pass& p, const LayerWeights& w, const ClsRows& c, bool gathered, const Hidden& cur, bool cur16,
                    const int32_t* cu_dev, int seq0, int seq1, int tok_base, float* out_dev) {
  Encoder* enc = p.enc;
  const vr_bert_desc& d = enc->d;
  const int T = p.T, H = d.hidden, I = d.intermediate, n_seq = seq1 - seq0;
  const dim3 gblocks(Pass::blocks4(n_seq));
  if (!gathered) {
    hipLaunchKernelGGL(gather_first_rows_kernel, gblocks, dim3(256), 0, p.s, reinterpret_cast<const float4*>(enc->ctx), cu_dev,
                       seq0, tok_base, n_seq, T, p.plain ? H / 8 : H / 4, reinterpret_cast<float4*>(c.ctx));
    if (p.plain && cur16)
      hipLaunchKernelGGL(gather_first_rows_ln16_kernel, gblocks, dim3(256), 0, p.s, p.xh, cur.stat, cur.g, cur.b, cu_dev, seq0,
                         tok_base, n_seq, T, H, c.x, static_cast<half_t*>(nullptr));
    else if (p.plain)
      hipLaunchKernelGGL(gather_first_rows_ln_kernel, gblocks, dim3(256), 0, p.s, cur.pre, cur.stat, cur.g, cur.b, cu_dev, seq0,
                         tok_base, n_seq, T, H, c.x);
    else
      hipLaunchKernelGGL(gather_first_rows_kernel, gblocks, dim3(256), 0, p.s, reinterpret_cast<const float4*>(enc->x), cu_dev,
                         seq0, tok_base, n_seq, T, H / 4, reinterpret_cast<float4*>(c.x));
  }
  const Rows x = p.rows(c.xs, c.x), ctx = p.rows(c.ctx), ffn = p.rows(c.ffn);
  VR_TRY(project_residual(p, w.wo, w.s_o, w.bo, n_seq, H, H, ctx, c.x, c.tmp));
  layernorm_rows(p, c.tmp, n_seq, w.ln1g, w.ln1b, x);
  if (d.ffn != VR_FFN_GELU)
    VR_TRY(gated_up_rows(p, w, p.plain && enc->fuse && skinny_routed(n_seq, 2 * I, H), n_seq, x, ffn));
  else
    VR_TRY(project_act(p, EPI_BIAS_GELU, w.w1, w.s_1, w.b1, n_seq, I, H, x, ffn));
  VR_TRY(project_residual(p, w.w2, w.s_2, w.b2, n_seq, H, I, ffn, c.x, c.tmp));
  layernorm_rows(p, c.tmp, n_seq, w.ln2g, w.ln2b, {c.x});
  launch_pool(p.e, enc, c.x, cu_dev, seq0, seq1, tok_base, 1, out_dev, nullptr);
  VR_HIP(hipGetLastError());
  return 0;
}

// forward of sequences [seq0, seq1) whose tokens are ids_dev[tok_base .. tok_base + T). sp (or null): pool the spans
// of these sequences, one row each at out_dev[span], instead of one row per sequence — the pass then runs as a
// mean-pooled model's does, whatever the description's pooling says.
static int forward_chunk(vr_engine* e, Encoder* enc, const int32_t* ids_dev, const int32_t* cu_dev,
                         const int32_t* seg_dev, int n_seq_total, int seq0, int seq1, int tok_base, int T, int max_len,
                         double attn_flop, float* out_dev, const Spans* sp = nullptr) {
  const vr_bert_desc& d = enc->d;
  if (d.norm == VR_NORM_PRE_RMS_ROTARY)  // the Qwen2 form
    return forward_chunk_rms_rotary(e, enc, ids_dev, cu_dev, n_seq_total, seq0, seq1, tok_base, T, max_len, attn_flop, out_dev, sp);
  if (d.norm == VR_NORM_PRE_RMS)  // the T5 form of the routine below
    return forward_chunk_rms(e, enc, ids_dev, cu_dev, n_seq_total, seq0, seq1, tok_base, T, max_len, attn_flop, out_dev, sp);
  if (d.norm == VR_NORM_PRE)  // a routine of its own: none of the LayerNorm folds below applies to it
    return forward_chunk_prenorm(e, enc, ids_dev, cu_dev, n_seq_total, seq0, seq1, tok_base, T, max_len, attn_flop, out_dev, sp);
  const int H = d.hidden, I = d.intermediate, nh = d.heads, dh = H / nh;
  // f16x3 mode: every GEMM input also exists as (hi, lo) f16. The split hidden state lives in xs;
  // the context and the FFN intermediate are ONLY needed split, so they reuse the f32 buffers.
  // f16 mode: the same, with plain f16 rows and no lo half (the lo pointers are null).
  Pass p(e, enc, T);
  hipStream_t s = p.s;
  const bool plain = p.plain;
  half_t *xh = p.xh, *xl = p.xl, *ch = p.ctx.hi, *fh = p.ffn.hi;
  // f16 mode does not store the f32 hidden state at all. A LayerNorm writes its f16 output (the next
  // GEMM's input) and the row's (mean, 1/sigma); the only other reader of the hidden state is the
  // residual add of the next projection's epilogue, which already reads 4 bytes per element — it
  // reads the PRE-LN row instead and re-derives the LayerNorm output (ln_apply: same operations,
  // same bits). That takes 4 of the 10 bytes per element out of every LayerNorm pass. The pre-LN
  // rows alternate between enc->tmp and enc->x; `cur` describes the current hidden state.
  float2* stat_a = p.stat;
  float2* stat_b = plain ? stat_a + T : nullptr;
  Hidden cur{enc->x, stat_b, enc->lng, enc->lnb};
  bool cur16 = false;  // f16 residual stream: the current pre-LN rows are the f16 rows in xh (cur.pre is stale)
  const float* final_x = enc->x;  // the f32 rows pooling reads
  const bool lnfuse = plain && !enc->layers.empty();  // (a model without layers pools the embedding LayerNorm's output)
  // a handful of tokens (one query): the two LayerNorm launches of a layer are folded into the projections
  // that consume them (gemm_f16_skinny_ln_kernel)
  const bool fold_ln = lnfuse && skinny_ln_supported(T, 3 * H, H) && I % 16 == 0;
  // large batches (the 256-tile GEMM): the LayerNorm passes disappear into the GEMMs on both sides of them —
  // the producing epilogue also stores f16 pre-LN rows and per-(row, 64 columns) partial sums, a tiny
  // kernel turns those into (mean, 1/sigma), and the consuming GEMM multiplies the pre-LN rows by the
  // gain-scaled weights and applies the statistics in its epilogue (EPI_FOLD_*).
  const bool fold_big = lnfuse && T > 4 * kSkinnyM && H % 64 == 0 && enc->layers[0].cs_1 != nullptr;
  // ... and with an f16 residual stream (EPI_RLS_*): the pre-LayerNorm rows live in xh only
  const bool res16 = fold_big && direct_usable(H, H) && direct_usable(H, I);
  float2* part = reinterpret_cast<float2*>(enc->lnpart);
  const int segs = H / 64;
  const unsigned fin_blocks = static_cast<unsigned>((T + 255) / 256);
  if (seg_dev)
    hipLaunchKernelGGL((embed_ln_kernel<true>), dim3(p.row_blocks), dim3(256), 0, s, ids_dev, cu_dev, n_seq_total,
                       tok_base, T, H, d.vocab, enc->word, enc->pos, enc->type, enc->lng, enc->lnb, d.eps,
                       lnfuse ? nullptr : enc->x, xh, xl, lnfuse ? enc->x : nullptr, lnfuse ? stat_b : nullptr, seg_dev);
  else if (d.position != VR_POS_LEARNED)  // rotary, or no positions at all: the body that reads no table
    hipLaunchKernelGGL(embed_ln_rotary_kernel, dim3(p.row_blocks), dim3(256), 0, s, ids_dev, cu_dev, n_seq_total,
                       tok_base, T, H, d.vocab, enc->word, enc->type, enc->lng, enc->lnb, d.eps, lnfuse ? nullptr : enc->x, xh, xl,
                       lnfuse ? enc->x : nullptr, lnfuse ? stat_b : nullptr);
  else
    hipLaunchKernelGGL((embed_ln_kernel<false>), dim3(p.row_blocks), dim3(256), 0, s, ids_dev, cu_dev, n_seq_total,
                       tok_base, T, H, d.vocab, enc->word, enc->pos, enc->type, enc->lng, enc->lnb, d.eps,
                       lnfuse ? nullptr : enc->x, xh, xl, lnfuse ? enc->x : nullptr, lnfuse ? stat_b : nullptr,
                       static_cast<const int32_t*>(nullptr));
  // Rotary positions and the gated FFN. UNFUSED: passes of their own behind the projections' existing epilogues —
  // rope_kernel in place on the Q and K thirds of the qkv rows (rotate_rows), and the FFN-up projection (N = 2I, bias
  // only) into enc->glu followed by glu_kernel (gate_rows), which writes the rows the FFN-down projection reads. FUSED
  // (f16 mode, products that launch_gemm_f16x3 / launch_skinny_ln send to a skinny kernel, i.e. at most 256 rows — a
  // question, a few chunks): the projection runs over the re-ordered matrix and its epilogue rotates / gates
  // (EPI_ROPE_F16, EPI_*GLU_F16), no further launch and no second f16 rounding. VR_ENCODE_FUSE=0 when the model is loaded
  // keeps the unfused form everywhere for that model (A/B runs in one process, tests); its cached graphs then hold that
  // form too.
  const bool rotary = d.position == VR_POS_ROTARY, gated = d.ffn != VR_FFN_GELU;
  const int N1 = gated ? 2 * I : I;
  const bool fuse_enabled = enc->fuse;
  const bool fuse_rope = rotary && plain && fuse_enabled && skinny_routed(T, 3 * H, H);
  auto fuse_glu = [&](int M) { return gated && plain && fuse_enabled && skinny_routed(M, N1, H); };
  // large batches: the gate in the epilogue of the folded-LayerNorm projection (mid / ping-pong kernel, EPI_FOLD_*GLU)
  const bool fuse_glu_big = gated && fuse_enabled && !fuse_glu(T) && fold_big && pp_usable(N1, H) &&
                            enc->layers[0].cs_1_p != nullptr;
  half_t* parth = reinterpret_cast<half_t*>(part);  // the folded LayerNorms' partial sums, in an epilogue's Cl slot
  if (rotary)
    hipLaunchKernelGGL(positions_kernel, dim3(static_cast<unsigned>((T + 255) / 256)), dim3(256), 0, s, cu_dev, n_seq_total,
                       tok_base, T, reinterpret_cast<int32_t*>(enc->posidx));
  // the last layer of a [CLS]-pooled model runs on the [CLS] rows only behind its attention (ClsRows, cls_tail)
  const int n_seq = seq1 - seq0;
  const bool cls_rows = !sp && d.pooling == VR_POOL_CLS && !enc->layers.empty() &&
                        static_cast<int64_t>(n_seq) * (4 * H + I) <= static_cast<int64_t>(T) * 3 * H;
  // the unfused gate's workspace: for an unfused FFN-up over the T rows, or over the CLS tail's n_seq rows
  if (gated && ((!fuse_glu(T) && !fuse_glu_big) || (cls_rows && !fuse_glu(n_seq)))) VR_TRY(p.need_glu());
  const ClsRows cls(enc, n_seq);
  // `collapse` (cls_collapse_attend) exists for the f16 residual stream of large batches (the hidden state is the f16
  // pre-LayerNorm rows in xh with their statistics), plain bidirectional attention of the hidden width (learned or no
  // positions, no bias, slopes, window, mask or Q/K norm), head size 32 or 64, at most kClsHeads heads, a longest
  // sequence whose logits and weights fit the 64 KiB of LDS beside the u rows (cls_attend_lds: 608 tokens at H = 768,
  // 480 at H = 1024), and T / n_seq large enough that its workspace fits the qkv buffer behind the tail's (no kernel
  // writes that buffer in the last layer then). Everything else, a cross-encoder (build_encoder) and every model loaded
  // under VR_CLS_COLLAPSE=0 keep the Q/K/V projection and the attention over the T rows.
  const int cls_lpad = (max_len + kClsStep - 1) / kClsStep * kClsStep;
  const bool collapse = cls_rows && enc->cls_collapse && plain && fold_big && res16 && enc->layers.size() > 1 &&
                        enc->layers.back().wk_t != nullptr && d.position != VR_POS_ROTARY && !enc->bias && !enc->slopes &&
                        !enc->causal && !enc->qk_norm && enc->attn == H && (dh == 32 || dh == 64) && nh <= kClsHeads &&
                        cls_attend_lds(H, cls_lpad) <= 65536 && cls.floats <= static_cast<int64_t>(T) * 3 * H;
  for (size_t li = 0; li < enc->layers.size(); ++li) {
    const LayerWeights& w = enc->layers[li];
    const bool tail = cls_rows && li + 1 == enc->layers.size();
    const bool fold_prev = fold_ln && li > 0;  // the previous layer's closing LayerNorm runs inside this projection
    if (tail && collapse)  // (cur16 holds: res16 and li > 0)
      VR_TRY(cls_collapse_attend(p, w, cur, cls, cu_dev, seq0, n_seq, tok_base, cls_lpad));
    else if (fold_prev && fuse_rope)  // ... and the rotation in its epilogue
      VR_TRY(launch_skinny_ln(e, EPI_ROPE_F16, cur.pre, d.eps, const_cast<float2*>(cur.stat),
                              {.W = w.s_qkv_p, .bias = w.bqkv_p, .Ch = p.qkvh, .M = T, .N = 3 * H, .K = H, .ln_g = cur.g,
                               .ln_b = cur.b, .rope_tab = enc->rope, .rope_pos = p.posidx}));
    else if (fold_prev)
      VR_TRY(launch_skinny_ln(e, EPI_BIAS_F16, cur.pre, d.eps, const_cast<float2*>(cur.stat),
                              {.W = w.s_qkv, .bias = w.bqkv, .Ch = p.qkvh, .M = T, .N = 3 * H, .K = H, .ln_g = cur.g, .ln_b = cur.b}));
    else if (fold_big && li > 0)  // xh holds the f16 PRE-LN rows the previous FFN-down epilogue stored
      VR_TRY(launch_gemm_f16x3(e, enc, EPI_FOLD_F16, {.A = xh, .W = w.s_qkv_f, .bias = w.c_qkv, .Ch = p.qkvh, .M = T, .N = 3 * H,
                                                      .K = H, .passes = 1, .ln_stat = cur.stat, .ln_g = w.cs_qkv}));
    else if (fuse_rope)
      VR_TRY(launch_gemm_f16x3(e, enc, EPI_ROPE_F16, {.A = xh, .W = w.s_qkv_p, .bias = w.bqkv_p, .Ch = p.qkvh, .M = T, .N = 3 * H,
                                                      .K = H, .passes = 1, .rope_tab = enc->rope, .rope_pos = p.posidx}));
    else  // (f16 mode: Q, K, V as plain f16 rows for the f16 attention kernels)
      VR_TRY(project_bias(p, w.wqkv, w.s_qkv, w.bqkv, T, 3 * H, H, p.x(enc->x), enc->qkv));
    if (!(tail && collapse)) {
      if (rotary && !fuse_rope) rotate_rows(p, enc->rope, H, dh);
      VR_TRY(launch_attention(e, enc, cu_dev, seq0, n_seq, tok_base, max_len, tail, 0, attn_flop));
    }
    if (tail) return cls_tail(p, w, cls, collapse, cur, cur16, cu_dev, seq0, seq1, tok_base, out_dev);
    if (plain) {
      // hidden state = LN(cur.pre): pre-LN rows alternate between the two buffers
      float* t1 = cur.pre == enc->x ? enc->tmp : enc->x;
      float2* s1 = cur.stat == stat_b ? stat_a : stat_b;
      const bool last = li + 1 == enc->layers.size();
      if (res16) {
        // f16 residual stream: residual rows are f32 only in layer 0 (the embedding sum), the pre-LN rows go out
        // as f16 into xh, in place where the residual came from there
        VR_TRY(launch_gemm_f16x3(e, enc, cur16 ? EPI_RLS_R16_O16 : EPI_RLS_R32_O16,
                                 {.A = ch, .W = w.s_o, .bias = w.bo, .R = cur16 ? reinterpret_cast<const float*>(xh) : cur.pre, .Ch = xh,
                                  .Cl = parth, .M = T, .N = H, .K = H, .passes = 1, .ln_stat = cur.stat, .ln_g = cur.g, .ln_b = cur.b}));
        hipLaunchKernelGGL(ln_finalize_kernel, dim3(fin_blocks), dim3(256), 0, s, part, T, segs, H, d.eps, s1);
      } else if (fold_big) {
        VR_TRY(launch_gemm_f16x3(e, enc, EPI_BIAS_RESIDUAL_LN_STATS,
                                 {.A = ch, .W = w.s_o, .bias = w.bo, .R = cur.pre, .C = t1, .Ch = xh, .Cl = parth, .M = T, .N = H, .K = H,
                                  .passes = 1, .ln_stat = cur.stat, .ln_g = cur.g, .ln_b = cur.b}));
        hipLaunchKernelGGL(ln_finalize_kernel, dim3(fin_blocks), dim3(256), 0, s, part, T, segs, H, d.eps, s1);
      } else
        VR_TRY(launch_gemm_f16x3(e, enc, EPI_BIAS_RESIDUAL_LN,
                                 {.A = ch, .W = w.s_o, .bias = w.bo, .R = cur.pre, .C = t1, .M = T, .N = H, .K = H, .passes = 1,
                                  .ln_stat = cur.stat, .ln_g = cur.g, .ln_b = cur.b}));
      // the attention-output LayerNorm: a launch of its own unless it runs inside the FFN-up projection below
      if (!fold_ln && !fold_big) layernorm_f16_rows(p, t1, w.ln1g, w.ln1b, nullptr, s1);
      const Hidden mid{t1, s1, w.ln1g, w.ln1b};
      float* t2 = const_cast<float*>(cur.pre);  // its last reader (the epilogue above) is done
      float2* s2 = const_cast<float2*>(cur.stat);
      half_t* up_out = gated ? p.gluh : fh;  // gated: the same projections with the bias-only f16 epilogues, then glu_kernel
      const bool fg = fuse_glu(T);      // ... or, fused, the gate in the projection's epilogue over the re-ordered matrix
      const bool fgb = fuse_glu_big;
      if (fg && fold_ln)
        VR_TRY(launch_skinny_ln(e, p.glu_epi, t1, d.eps, s1,
                                {.W = w.s_1_p, .bias = w.b1_p, .Ch = fh, .M = T, .N = N1, .K = H, .ln_g = w.ln1g, .ln_b = w.ln1b}));
      else if (fg)
        VR_TRY(gated_up_rows(p, w, true, T, p.x(nullptr), p.ffn));
      else if (fgb)
        VR_TRY(launch_gemm_f16x3(e, enc, d.ffn == VR_FFN_SWIGLU ? EPI_FOLD_SWIGLU : EPI_FOLD_GEGLU,
                                 {.A = xh, .W = w.s_1_fp, .bias = w.c_1_p, .Ch = fh, .M = T, .N = N1, .K = H, .passes = 1, .ln_stat = s1,
                                  .ln_g = w.cs_1_p}));
      else if (fold_ln)
        VR_TRY(launch_skinny_ln(e, gated ? EPI_BIAS_F16 : EPI_BIAS_GELU, t1, d.eps, s1,
                                {.W = w.s_1, .bias = w.b1, .Ch = up_out, .M = T, .N = N1, .K = H, .ln_g = w.ln1g, .ln_b = w.ln1b}));
      else if (fold_big)
        VR_TRY(launch_gemm_f16x3(e, enc, gated ? EPI_FOLD_F16 : EPI_FOLD_GELU,
                                 {.A = xh, .W = w.s_1_f, .bias = w.c_1, .Ch = up_out, .M = T, .N = N1, .K = H, .passes = 1, .ln_stat = s1,
                                  .ln_g = w.cs_1}));
      else
        VR_TRY(launch_gemm_f16x3(e, enc, gated ? EPI_BIAS_F16 : EPI_BIAS_GELU,
                                 {.A = xh, .W = w.s_1, .bias = w.b1, .Ch = up_out, .M = T, .N = N1, .K = H, .passes = 1}));
      if (gated && !fg && !fgb) gate_rows(p, T, p.ffn);
      if (res16)  // (the last layer of a mean-pooled model also writes f32 rows: the final LayerNorm reads them)
        VR_TRY(launch_gemm_f16x3(e, enc, last ? EPI_RLS_R16_O32 : EPI_RLS_R16_O16,
                                 {.A = fh, .W = w.s_2, .bias = w.b2, .R = reinterpret_cast<const float*>(xh), .C = last ? t2 : nullptr,
                                  .Ch = xh, .Cl = parth, .M = T, .N = H, .K = I, .passes = 1, .ln_stat = mid.stat, .ln_g = mid.g,
                                  .ln_b = mid.b}));
      else if (fold_big)
        VR_TRY(launch_gemm_f16x3(e, enc, EPI_BIAS_RESIDUAL_LN_STATS,
                                 {.A = fh, .W = w.s_2, .bias = w.b2, .R = mid.pre, .C = t2, .Ch = xh, .Cl = parth, .M = T, .N = H, .K = I,
                                  .passes = 1, .ln_stat = mid.stat, .ln_g = mid.g, .ln_b = mid.b}));
      else
        VR_TRY(launch_gemm_f16x3(e, enc, EPI_BIAS_RESIDUAL_LN,
                                 {.A = fh, .W = w.s_2, .bias = w.b2, .R = mid.pre, .C = t2, .M = T, .N = H, .K = I, .passes = 1,
                                  .ln_stat = mid.stat, .ln_g = mid.g, .ln_b = mid.b}));
      // The closing LayerNorm. Folded and not the last: inside the next layer's Q/K/V projection (fold_ln: all of it,
      // fold_big: but for its statistics). The last LayerNorm of the network is always a launch of its own and also
      // stores its f32 rows (into the free buffer): pooling reads them
      if (fold_big && !last)
        hipLaunchKernelGGL(ln_finalize_kernel, dim3(fin_blocks), dim3(256), 0, s, part, T, segs, H, d.eps, s2);
      else if (!fold_ln || last)
        layernorm_f16_rows(p, t2, w.ln2g, w.ln2b, last ? t1 : nullptr, s2);
      cur16 = res16;
      cur = Hidden{t2, s2, w.ln2g, w.ln2b};
      if (last) final_x = t1;
      continue;
    }
    // f16x3 and f32 mode: the hidden state is the f32 rows in enc->x (and their halves in xs)
    VR_TRY(project_residual(p, w.wo, w.s_o, w.bo, T, H, H, p.ctx, enc->x, enc->tmp));
    layernorm_rows(p, enc->tmp, T, w.ln1g, w.ln1b, p.x(enc->x));
    if (gated)
      VR_TRY(gated_up_rows(p, w, false, T, p.x(enc->x), p.ffn));
    else
      VR_TRY(project_act(p, EPI_BIAS_GELU, w.w1, w.s_1, w.b1, T, I, H, p.x(enc->x), p.ffn));
    VR_TRY(project_residual(p, w.w2, w.s_2, w.b2, T, H, I, p.ffn, enc->x, enc->tmp));
    layernorm_rows(p, enc->tmp, T, w.ln2g, w.ln2b, p.x(enc->x));
  }
  launch_pool(e, enc, final_x, cu_dev, seq0, seq1, tok_base, 0, out_dev, sp);
  VR_HIP(hipGetLastError());
  return 0;
}

// Tokens per forward pass. Large enough that the 768-wide GEMMs launch many full rounds of 256x256
// tiles (262144 tokens x 768 columns = 3072 tiles on 256 CUs: the partly filled last round is then
// a few per cent of the launch); activations for it are ~45 KB per token (11.8 GB of the 288).
// VR_CHUNK_TOKENS overrides it for experiments.
static const int64_t kMaxChunkTokens = getenv("VR_CHUNK_TOKENS") ? atoll(getenv("VR_CHUNK_TOKENS")) : 262144;

// The host copy of the offsets (needed to cut chunks), every length and segment start checked: before any work
// is queued when the arguments are in host memory. span_off (or null, n_seq + 1 entries in `mem`) is copied with them
// into *span_off_host; read_spans checks it.
static int read_offsets(vr_engine* e, Encoder* enc, const int32_t* offsets, const int32_t* seg_b, int n_seq, int mem,
                        std::vector<int32_t>* cu_host, const int32_t* span_off = nullptr,
                        std::vector<int32_t>* span_off_host = nullptr) {
  cu_host->resize(static_cast<size_t>(n_seq) + 1);
  std::vector<int32_t> seg_host(seg_b ? static_cast<size_t>(n_seq) : 0);
  if (span_off) span_off_host->resize(cu_host->size());
  if (mem == VR_MEM_HOST) {
    memcpy(cu_host->data(), offsets, sizeof(int32_t) * cu_host->size());
    if (seg_b) memcpy(seg_host.data(), seg_b, sizeof(int32_t) * seg_host.size());
    if (span_off) memcpy(span_off_host->data(), span_off, sizeof(int32_t) * cu_host->size());
  } else {
    VR_HIP(hipMemcpyAsync(cu_host->data(), offsets, sizeof(int32_t) * cu_host->size(), hipMemcpyDeviceToHost,
                          e->stream));
    if (span_off)
      VR_HIP(hipMemcpyAsync(span_off_host->data(), span_off, sizeof(int32_t) * cu_host->size(), hipMemcpyDeviceToHost,
                            e->stream));
    if (seg_b)
      VR_HIP(hipMemcpyAsync(seg_host.data(), seg_b, sizeof(int32_t) * seg_host.size(), hipMemcpyDeviceToHost, e->stream));
    VR_HIP(hipStreamSynchronize(e->stream));
  }
  VR_CHECK((*cu_host)[0] == 0, "offsets must start at 0");
  for (int i = 0; i < n_seq; ++i) {
    int len = (*cu_host)[static_cast<size_t>(i) + 1] - (*cu_host)[static_cast<size_t>(i)];
    VR_CHECK(len >= 1 && len <= enc->d.max_pos, "sequence %d has %d tokens (1..%d allowed)", i, len,
             enc->d.max_pos);
    VR_CHECK(!seg_b || (seg_host[static_cast<size_t>(i)] >= 1 && seg_host[static_cast<size_t>(i)] <= len),
             "sequence %d: seg_b %d not in 1..%d", i, seg_b ? seg_host[static_cast<size_t>(i)] : 0, len);
  }
  return 0;
}

// The forward pass of n_seq checked sequences (cu_host: their offsets), one pooled row each into out_dev (device).
// seg_b (or null): each sequence's first segment-B position. sp (or null): one row per span instead, see forward_chunk.
static int forward_all(vr_engine* e, Encoder* enc, const int32_t* ids, const int32_t* offsets, const int32_t* seg_b,
                       int n_seq, int mem, const std::vector<int32_t>& cu_host, float* out_dev,
                       const Spans* sp = nullptr) {
  const int H = enc->d.hidden;
  const int64_t T_all = cu_host[static_cast<size_t>(n_seq)];
  const int32_t* ids_dev = ids;
  const int32_t* cu_dev = offsets;
  const int32_t* seg_dev = seg_b;
  if (mem == VR_MEM_HOST) {
    VR_TRY(enc->ids.grow(T_all, 0, e->stream));
    VR_TRY(enc->cu.grow(n_seq + 1, 0, e->stream));
    VR_HIP(hipMemcpyAsync(enc->ids.p, ids, sizeof(int32_t) * static_cast<size_t>(T_all), hipMemcpyHostToDevice,
                          e->stream));
    VR_HIP(hipMemcpyAsync(enc->cu.p, offsets, sizeof(int32_t) * cu_host.size(), hipMemcpyHostToDevice,
                          e->stream));
    ids_dev = enc->ids.p;
    cu_dev = enc->cu.p;
    if (seg_b) {
      VR_TRY(enc->seg.grow(n_seq, 0, e->stream));
      VR_HIP(hipMemcpyAsync(enc->seg.p, seg_b, sizeof(int32_t) * static_cast<size_t>(n_seq), hipMemcpyHostToDevice,
                            e->stream));
      seg_dev = enc->seg.p;
    }
  }
  int seq0 = 0;
  while (seq0 < n_seq) {
    int seq1 = seq0;
    int max_len = 0;
    int64_t T = 0;
    double len2 = 0.0;
    while (seq1 < n_seq) {
      int len = cu_host[static_cast<size_t>(seq1) + 1] - cu_host[static_cast<size_t>(seq1)];
      if (seq1 > seq0 && T + len > kMaxChunkTokens) break;
      T += len;
      len2 += static_cast<double>(len) * len;
      max_len = std::max(max_len, len);
      ++seq1;
    }
    VR_TRY(ensure_workspace(e, enc, std::max<int64_t>(T, 1024)));
    // A small forward pass (one chunk, <= 1024 tokens) is launch-bound: the second time a shape is seen
    // it is captured into a hipGraph and replayed from then on. Only on the engine's own stream (a
    // caller's stream may be under capture itself) and with the HIP-event profiler off. Never a semantic call: its
    // parameters are launch arguments and its chunk counter is zeroed per call, neither of which the key knows.
    static const bool graphs_on = !(getenv("VR_ENCODE_GRAPH") && atoi(getenv("VR_ENCODE_GRAPH")) == 0);
    const bool graphable = graphs_on && seq0 == 0 && seq1 == n_seq && T <= 1024 && e->stream == e->own_stream &&
                           !prof_on(e) && !(sp && sp->sem);
    bool done = false;
    if (graphable) {
      if (enc->graphs.size() > 256) invalidate_graphs(enc);  // (shapes are few in practice; start over rather than track recency)
      Encoder::GraphEntry& g =
          enc->graphs[Encoder::GraphKey{static_cast<int>(T), n_seq, max_len, ids_dev, cu_dev, seg_dev, out_dev,
                                        sp ? sp->tok_dev : nullptr, sp ? sp->seq_dev : nullptr,
                                        sp ? sp->off[static_cast<size_t>(n_seq)] : 0,
                                        enc->head.n_stages > 0 ? enc->pooled.p : nullptr}];
      if (!g.exec && !g.bad && g.seen >= 1) {
        if (hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
          const int rc = forward_chunk(e, enc, ids_dev, cu_dev, seg_dev, n_seq, seq0, seq1, 0, static_cast<int>(T),
                                       max_len, 4.0 * H * len2, out_dev, sp);
          hipGraph_t graph = nullptr;
          const hipError_t end = hipStreamEndCapture(e->stream, &graph);
          if (rc != 0 || end != hipSuccess || !graph ||
              hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0) != hipSuccess) {
            g.exec = nullptr;
            g.bad = true;  // this shape runs eagerly from now on
          }
          if (graph) (void)hipGraphDestroy(graph);
          (void)hipGetLastError();
        } else {
          g.bad = true;
          (void)hipGetLastError();
        }
      }
      if (g.exec) {
        VR_HIP(hipGraphLaunch(g.exec, e->stream));
        done = true;
      }
      ++g.seen;
    }
    if (!done)
      VR_TRY(forward_chunk(e, enc, ids_dev, cu_dev, seg_dev, n_seq, seq0, seq1, cu_host[static_cast<size_t>(seq0)],
                           static_cast<int>(T), max_len, 4.0 * H * len2, out_dev, sp));
    seq0 = seq1;
  }
  return 0;
}

// n_floats results from out_dev to the caller's host `out` (out_mem == VR_MEM_HOST), or the stream drained while
// host inputs may still be read
static int finish(vr_engine* e, float* out, const float* out_dev, int64_t n_floats, int mem, int out_mem) {
  if (out_mem == VR_MEM_HOST) {
    VR_HIP(hipMemcpyAsync(out, out_dev, sizeof(float) * static_cast<size_t>(n_floats), hipMemcpyDeviceToHost, e->stream));
    VR_HIP(hipStreamSynchronize(e->stream));
  } else if (mem == VR_MEM_HOST) {
    VR_HIP(hipStreamSynchronize(e->stream));
  }
  return 0;
}

int encoder_encode(vr_engine* e, const int32_t* ids, const int32_t* offsets, int n_seq, int mem,
                   float* out, int out_mem) {
  Encoder* enc = static_cast<Encoder*>(e->encoder);
  VR_CHECK(enc != nullptr, "no encoder loaded (vr_encoder_load)");
  if (n_seq <= 0) return 0;
  const int W = out_width(enc);
  std::vector<int32_t> cu_host;
  VR_TRY(read_offsets(e, enc, offsets, nullptr, n_seq, mem, &cu_host));
  float* out_dev = out;
  if (out_mem == VR_MEM_HOST) {
    VR_TRY(enc->out.grow(static_cast<int64_t>(n_seq) * W, 0, e->stream));
    out_dev = enc->out.p;
  }
  if (enc->head.n_stages > 0) VR_TRY(enc->pooled.grow(static_cast<int64_t>(n_seq) * enc->d.hidden, 0, e->stream));
  VR_TRY(forward_all(e, enc, ids, offsets, nullptr, n_seq, mem, cu_host, out_dev));
  return finish(e, out, out_dev, static_cast<int64_t>(n_seq) * W, mem, out_mem);
}

// The spans of a span call, checked against the sequences (cu_host) — span_off monotone from 0 (sp->off holds its host
// copy already), every span non-empty and inside its sequence — and made ready for span_pool_kernel: sp->tok_dev is
// the caller's array or its staged copy, sp->seq_dev the sequence index of every span. n_expected >= 0: the span count
// the caller announced. Nothing is queued before the checks when the arrays are in host memory.
// units (a semantic call, the messages then say "unit"): a sequence's spans are also in order and never overlap, and
// there are at most kMaxSemUnits of them.
static int read_spans(vr_engine* e, Encoder* enc, const int32_t* span_tok, int n_seq, int mem,
                      const std::vector<int32_t>& cu_host, int64_t n_expected, Spans* sp, bool units = false) {
  const char* what = units ? "unit" : "span";
  VR_CHECK(sp->off[0] == 0, "%s_off must start at 0", what);
  for (int i = 0; i < n_seq; ++i) {
    VR_CHECK(sp->off[static_cast<size_t>(i) + 1] >= sp->off[static_cast<size_t>(i)],
             "%s_off decreases at sequence %d (%d %ss before it, %d after)", what, i, sp->off[static_cast<size_t>(i)], what,
             sp->off[static_cast<size_t>(i) + 1]);
    VR_CHECK(!units || sp->off[static_cast<size_t>(i) + 1] - sp->off[static_cast<size_t>(i)] <= kMaxSemUnits,
             "sequence %d has %d units (at most %d allowed)", i,
             sp->off[static_cast<size_t>(i) + 1] - sp->off[static_cast<size_t>(i)], kMaxSemUnits);
  }
  const int64_t n_spans = sp->off[static_cast<size_t>(n_seq)];
  VR_CHECK(n_expected < 0 || n_spans == n_expected, "%lld rows announced, span_off holds %lld spans",
           static_cast<long long>(n_expected), static_cast<long long>(n_spans));
  if (n_spans == 0) return 0;
  VR_CHECK(span_tok != nullptr, "null %s_tok", what);
  std::vector<int32_t> tok_copy;
  const int32_t* tok = span_tok;
  if (mem != VR_MEM_HOST) {
    tok_copy.resize(static_cast<size_t>(2 * n_spans));
    VR_HIP(hipMemcpyAsync(tok_copy.data(), span_tok, sizeof(int32_t) * tok_copy.size(), hipMemcpyDeviceToHost, e->stream));
    VR_HIP(hipStreamSynchronize(e->stream));
    tok = tok_copy.data();
  }
  enc->span_seq_host.resize(static_cast<size_t>(n_spans));
  for (int i = 0; i < n_seq; ++i) {
    const int len = cu_host[static_cast<size_t>(i) + 1] - cu_host[static_cast<size_t>(i)];
    for (int r = sp->off[static_cast<size_t>(i)]; r < sp->off[static_cast<size_t>(i) + 1]; ++r) {
      const int begin = tok[2 * static_cast<size_t>(r)], end = tok[2 * static_cast<size_t>(r) + 1];
      VR_CHECK(begin >= 0 && begin < end && end <= len, "sequence %d %s %d: [%d, %d) is empty or outside its %d tokens", i,
               what, r, begin, end, len);
      VR_CHECK(!units || r == sp->off[static_cast<size_t>(i)] || begin >= tok[2 * static_cast<size_t>(r) - 1],
               "sequence %d unit %d: [%d, %d) begins before the end of unit %d (%d): units are in order and never overlap",
               i, r, begin, end, r - 1, r > 0 ? tok[2 * static_cast<size_t>(r) - 1] : 0);
      enc->span_seq_host[static_cast<size_t>(r)] = i;
    }
  }
  VR_TRY(enc->span_seq.grow(n_spans, 0, e->stream));
  VR_HIP(hipMemcpyAsync(enc->span_seq.p, enc->span_seq_host.data(), sizeof(int32_t) * static_cast<size_t>(n_spans),
                        hipMemcpyHostToDevice, e->stream));
  sp->seq_dev = enc->span_seq.p;
  sp->tok_dev = span_tok;
  if (mem == VR_MEM_HOST) {
    VR_TRY(enc->span_tok.grow(2 * n_spans, 0, e->stream));
    VR_HIP(hipMemcpyAsync(enc->span_tok.p, span_tok, sizeof(int32_t) * static_cast<size_t>(2 * n_spans),
                          hipMemcpyHostToDevice, e->stream));
    sp->tok_dev = enc->span_tok.p;
  }
  return 0;
}

int encoder_encode_spans(vr_engine* e, const int32_t* ids, const int32_t* offsets, int n_seq, const int32_t* span_off,
                         const int32_t* span_tok, int mem, int64_t n_expected, float* out, int out_mem) {
  Encoder* enc = static_cast<Encoder*>(e->encoder);
  VR_CHECK(enc != nullptr, "no encoder loaded (vr_encoder_load)");
  if (n_seq <= 0) return 0;
  const int W = out_width(enc);
  std::vector<int32_t> cu_host;
  Spans sp;
  VR_TRY(read_offsets(e, enc, offsets, nullptr, n_seq, mem, &cu_host, span_off, &sp.off));
  VR_TRY(read_spans(e, enc, span_tok, n_seq, mem, cu_host, n_expected, &sp));
  const int64_t n_spans = sp.off[static_cast<size_t>(n_seq)];
  if (n_spans == 0) return 0;
  float* out_dev = out;
  if (out_mem == VR_MEM_HOST) {
    VR_TRY(enc->out.grow(n_spans * W, 0, e->stream));
    out_dev = enc->out.p;
  }
  if (enc->head.n_stages > 0) VR_TRY(enc->pooled.grow(n_spans * enc->d.hidden, 0, e->stream));
  VR_TRY(forward_all(e, enc, ids, offsets, nullptr, n_seq, mem, cu_host, out_dev, &sp));
  // (device arrays in and out: drain here, enc->span_seq_host must outlive its upload)
  if (mem != VR_MEM_HOST && out_mem != VR_MEM_HOST) VR_HIP(hipStreamSynchronize(e->stream));
  return finish(e, out, out_dev, n_spans * W, mem, out_mem);
}

int encoder_encode_semantic(vr_engine* e, const int32_t* ids, const int32_t* offsets, int n_seq, const int32_t* unit_off,
                            const int32_t* unit_tok, int mem, const vr_semantic_params* p, float* out_rows,
                            int32_t* out_unit_start, float* out_gap_dist, int32_t* n_chunks, int out_mem) {
  Encoder* enc = static_cast<Encoder*>(e->encoder);
  VR_CHECK(enc != nullptr, "no encoder loaded (vr_encoder_load)");
  *n_chunks = 0;
  if (n_seq <= 0) return 0;
  VR_CHECK(p->struct_size == static_cast<int32_t>(sizeof(vr_semantic_params)), "vr_semantic_params.struct_size is %d, %d expected",
           p->struct_size, static_cast<int>(sizeof(vr_semantic_params)));
  VR_CHECK(p->buffer >= 0 && p->buffer <= 3, "semantic buffer %d not in 0..3", p->buffer);
  VR_CHECK(p->break_permille >= 0 && p->break_permille <= 1000, "semantic break_permille %d not in 0..1000", p->break_permille);
  VR_CHECK(p->min_tokens >= 0, "semantic min_tokens %d is negative", p->min_tokens);
  VR_CHECK(p->max_tokens >= 1 && p->max_tokens >= p->min_tokens, "semantic max_tokens %d is below 1 or below min_tokens %d",
           p->max_tokens, p->min_tokens);
  VR_CHECK(p->min_distance == p->min_distance, "semantic min_distance is not a number");
  const int H = enc->d.hidden, W = out_width(enc);
  std::vector<int32_t> cu_host;
  Spans sp;
  VR_TRY(read_offsets(e, enc, offsets, nullptr, n_seq, mem, &cu_host, unit_off, &sp.off));
  VR_TRY(read_spans(e, enc, unit_tok, n_seq, mem, cu_host, -1, &sp, true));
  const int64_t n_units = sp.off[static_cast<size_t>(n_seq)];
  if (n_units == 0) return 0;
  VR_CHECK(out_rows && out_unit_start && out_gap_dist, "null output");
  const bool staged = enc->head.n_stages > 0;
  hipStream_t s = e->stream;
  VR_TRY(enc->sem_sums.grow(n_units * H, 0, s));
  VR_TRY(enc->sem_idx.grow(n_units, 0, s));
  VR_TRY(enc->sem_seq_chunks.grow(n_seq, 0, s));
  VR_TRY(enc->sem_seq_base.grow(n_seq, 0, s));
  VR_TRY(enc->sem_counter.grow(1, 0, s));
  if (staged) {
    VR_TRY(enc->pooled.grow(n_units * H, 0, s));
    VR_TRY(enc->sem_rows.grow(n_units * W, 0, s));
  }
  Semantic m{};
  m.p = SemanticParams{p->buffer, p->break_permille, p->min_tokens, p->max_tokens, p->min_distance};
  m.off_dev = unit_off;
  if (mem == VR_MEM_HOST) {
    VR_TRY(enc->sem_off.grow(n_seq + 1, 0, s));
    VR_HIP(hipMemcpyAsync(enc->sem_off.p, unit_off, sizeof(int32_t) * sp.off.size(), hipMemcpyHostToDevice, s));
    m.off_dev = enc->sem_off.p;
  }
  float* rows_dev = out_rows;
  m.start = out_unit_start;
  m.dist = out_gap_dist;
  if (out_mem == VR_MEM_HOST) {
    VR_TRY(enc->out.grow(n_units * W, 0, s));
    VR_TRY(enc->sem_start.grow(n_units, 0, s));
    VR_TRY(enc->sem_dist.grow(n_units, 0, s));
    rows_dev = enc->out.p;
    m.start = enc->sem_start.p;
    m.dist = enc->sem_dist.p;
  }
  m.sums = enc->sem_sums.p;
  m.rows = enc->sem_rows.p;
  m.idx = enc->sem_idx.p;
  m.seq_chunks = enc->sem_seq_chunks.p;
  m.seq_base = enc->sem_seq_base.p;
  m.counter = enc->sem_counter.p;
  sp.sem = &m;
  VR_HIP(hipMemsetAsync(m.counter, 0, sizeof(int32_t), s));
  VR_TRY(forward_all(e, enc, ids, offsets, nullptr, n_seq, mem, cu_host, rows_dev, &sp));
  // the chunk count decides how many rows there are to copy: the stream is drained here in every case
  VR_HIP(hipMemcpyAsync(n_chunks, m.counter, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  VR_HIP(hipStreamSynchronize(s));
  if (out_mem == VR_MEM_HOST) {
    VR_HIP(hipMemcpyAsync(out_rows, rows_dev, sizeof(float) * static_cast<size_t>(*n_chunks) * W, hipMemcpyDeviceToHost, s));
    VR_HIP(hipMemcpyAsync(out_unit_start, m.start, sizeof(int32_t) * static_cast<size_t>(n_units), hipMemcpyDeviceToHost, s));
    VR_HIP(hipMemcpyAsync(out_gap_dist, m.dist, sizeof(float) * static_cast<size_t>(n_units), hipMemcpyDeviceToHost, s));
    VR_HIP(hipStreamSynchronize(s));
  }
  return 0;
}

int encoder_rerank(vr_engine* e, const int32_t* ids, const int32_t* offsets, const int32_t* seg_b, int n_seq, int mem,
                   float* out, int out_mem) {
  Encoder* enc = static_cast<Encoder*>(e->reranker);
  VR_CHECK(enc != nullptr, "no reranker loaded (vr_reranker_load)");
  if (n_seq <= 0) return 0;
  if (enc->d.type_vocab == 1) seg_b = nullptr;  // one token type: the embed_ln_kernel<false> instantiation serves pairs
  else VR_CHECK(seg_b != nullptr, "seg_b is required for a reranker with %d token types", enc->d.type_vocab);
  const int H = enc->d.hidden;
  std::vector<int32_t> cu_host;
  VR_TRY(read_offsets(e, enc, offsets, seg_b, n_seq, mem, &cu_host));
  if (!enc->score_w) VR_TRY(enc->rows.grow(static_cast<int64_t>(n_seq) * H, 0, e->stream));
  float* out_dev = out;
  if (out_mem == VR_MEM_HOST) {
    VR_TRY(enc->out.grow(n_seq, 0, e->stream));
    out_dev = enc->out.p;
  }
  if (enc->score_w) {  // a decoder cross-encoder: the pass itself ends in the logits (rerank_tail)
    const float* before = enc->tail_ws.p;
    VR_TRY(enc->tail_ws.grow(RerankRows::floats(enc, n_seq), 0, e->stream));
    if (enc->tail_ws.p != before) invalidate_graphs(enc);  // (captured tails hold its pointers)
    VR_TRY(forward_all(e, enc, ids, offsets, nullptr, n_seq, mem, cu_host, out_dev));
    return finish(e, out, out_dev, n_seq, mem, out_mem);
  }
  VR_TRY(forward_all(e, enc, ids, offsets, seg_b, n_seq, mem, cu_host, enc->rows.p));
  const dim3 head_grid(static_cast<unsigned>((n_seq + 15) / 16));
  if (enc->head_ln_g)
    hipLaunchKernelGGL(rerank_head_ln_kernel, head_grid, dim3(256), 0, e->stream, enc->rows.p, n_seq, H, enc->pool_w,
                       enc->pool_b, enc->head_ln_g, enc->head_ln_b, enc->d.eps, enc->cls_w, enc->cls_b, out_dev);
  else
    hipLaunchKernelGGL(rerank_head_kernel, head_grid, dim3(256), 0, e->stream, enc->rows.p, n_seq, H, enc->pool_w,
                       enc->pool_b, enc->cls_w, enc->cls_b, out_dev);
  VR_HIP(hipGetLastError());
  return finish(e, out, out_dev, n_seq, mem, out_mem);
}

}  // namespace vr
