// Device code the row kernels over bf16 logits share (lia_score.hip, lia_sample.hip, lia_logprobs.hip): one LIA_ROW_THREADS workgroup
// per row, 8 consecutive tokens per thread.  Moved here word for word from the kernels that used to hold it, so that two kernels
// that must agree bit for bit -- lia_token_logprobs_kernel and lia_topn_logprobs_kernel on m, s and the log-probability; the sampler
// and the top-N selection on the order of a row -- run the same code.  lia_internal.h stays declarations only.
#pragma once
#include "lia_internal.h"

// ---- the scoring passes (lia_score.hip's header comment states them and their error bound) ------------------------------------
__device__ __forceinline__ void load_logits8(const bf16_t* __restrict__ row, int i, int vocab, bool vec, float f[8]) {
  if (vec) {                       // vec: vocab % 8 == 0, ld % 8 == 0 and a 16-byte aligned base; i < vocab
    const uint4 v = *(const uint4*)(row + i);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = bf2f((w[e >> 1] >> ((e & 1) * 16)) & 0xffff);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = i + e < vocab ? bf2f(row[i + e]) : -INFINITY;    // (-inf past the end: no maximum, no mass)
  }
}

// m = max_j l_j with the first index that holds it (0x7fffffff for an empty maximum), s = sum_j exp(l_j - m): the same bits in every
// thread.
struct RowMaxSum { float m, s; int bi; };

__device__ __forceinline__ RowMaxSum row_max_sum(const bf16_t* __restrict__ row, int vocab, int vec) {
  __shared__ float sv[LIA_ROW_WAVES];
  __shared__ int si[LIA_ROW_WAVES];
  __shared__ float ss[LIA_ROW_WAVES];
  const int tid = threadIdx.x, lane = tid & 63;

  // ---- pass 1: the maximum and its first index; indices ascend inside a lane, so a lane keeps the first of equal values ----
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = tid * 8; i < vocab; i += LIA_ROW_THREADS * 8) {
    float f[8];
    load_logits8(row, i, vocab, vec, f);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (i + e < vocab && (f[e] > best || (f[e] == best && i + e < bi))) { best = f[e]; bi = i + e; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  if (lane == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
  __syncthreads();
  best = sv[0]; bi = si[0];
#pragma unroll
  for (int w = 1; w < LIA_ROW_WAVES; ++w)
    if (sv[w] > best || (sv[w] == best && si[w] < bi)) { best = sv[w]; bi = si[w]; }
  const float m = best;              // the same bits in every thread

  // ---- pass 2: s = sum exp(l - m); the row comes from L2 ----
  float s = 0.f;
  for (int i = tid * 8; i < vocab; i += LIA_ROW_THREADS * 8) {
    float f[8];
    load_logits8(row, i, vocab, vec, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += expf(f[e] - m);
  }
  s = wave_sum(s);
  if (lane == 0) ss[tid >> 6] = s;
  __syncthreads();
  s = ss[lane & (LIA_ROW_WAVES - 1)];
#pragma unroll
  for (int o = LIA_ROW_WAVES / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);

  RowMaxSum r;
  r.m = m;
  r.s = s;
  r.bi = bi;
  return r;
}

// l_t - (m + log s) of token t, 0.0 for a t outside [0, vocab): the one expression both scoring kernels report
__device__ __forceinline__ float row_logprob(const bf16_t* __restrict__ row, int vocab, int64_t t, float m, float s) {
  return (t >= 0 && t < (int64_t)vocab) ? bf2f(row[t]) - (m + logf(s)) : 0.f;
}

// ---- the order of a row: the sampler's 16-bit key and its 12 + 4-bit histogram levels (lia_sample.hip's header comment) ----------
#define SMP_TILE (LIA_ROW_THREADS * 8)   // tokens per token-ordered tile: 8 consecutive tokens per thread
#define SMP_KEY_NEG_INF 0x007F           // key_of(bf16 -inf); keys below it are negative NaNs
#define SMP_KEY_POS_INF 0xFF80           // key_of(bf16 +inf)
#define SMP_BINS 4096

__device__ __forceinline__ int key_of(uint32_t h) { return (h & 0x8000u) ? (int)(~h & 0xFFFFu) : (int)(h | 0x8000u); }

// keys of tokens i .. i + 7 (-1 past the end of the row); the suppressed token's key is that of -inf.  MASKED
// (lia_ctx_set_token_mask): so is that of a token whose bit in the row's allowed-token mask is clear -- mrow: the mask row as bytes;
// i is a multiple of 8, so byte i >> 3 holds the bits of exactly these 8 tokens.  The passes need nothing else: membership, the
// histograms' bins and the weights are functions of the key.
template <int MASKED = 0>
__device__ __forceinline__ void load_keys8(const bf16_t* __restrict__ row, int i, int vocab, bool vec, int suppress, int k[8],
                                           const uint8_t* __restrict__ mrow = nullptr) {
  if (vec && i < vocab) {            // vec: vocab % 8 == 0 and 16-byte aligned rows
    const uint4 v = *(const uint4*)(row + i);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) k[e] = key_of((w[e >> 1] >> ((e & 1) * 16)) & 0xffffu);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) k[e] = i + e < vocab ? key_of(row[i + e]) : -1;
  }
  const unsigned d = (unsigned)(suppress - i);
  if (d < 8u) k[d] = SMP_KEY_NEG_INF;
  if constexpr (MASKED) {
    if (i < vocab) {
      const uint32_t allow = mrow[i >> 3];
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (k[e] >= 0 && !((allow >> e) & 1u)) k[e] = SMP_KEY_NEG_INF;
    }
  }
}

// exclusive prefix sum over the workgroup in thread order; *total (if not NULL): the sum of all, the same bits in every thread.
// red: LIA_ROW_WAVES T of LDS.
template <typename T> __device__ __forceinline__ T block_excl_scan(T v, T* red, T* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  T ex = __shfl_up(x, 1, 64);
  if (lane == 0) ex = 0;
  if (lane == 63) red[w] = x;
  __syncthreads();
  T pre = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < LIA_ROW_WAVES; ++i) {
    const T r = red[i];
    if (i < w) pre += r;
    tot += r;
  }
  __syncthreads();
  if (total) *total = tot;
  return pre + ex;
}

// The bin b of h[0 .. SMP_BINS) (bins in descending key order from the top) with  above(b) < thr <= above(b) + h[b],
// above(b) = the sum of the bins above b.  Thread t owns bins 4095 - 4t - j, j < 4.  Writes (bin, above) to *out_bin, *out_above.
template <typename T> __device__ __forceinline__ void find_boundary_bin(const T* h, T thr, T* red, int* out_bin, T* out_above) {
  const int t = threadIdx.x;
  if (t == 0) { *out_bin = 0; *out_above = 0; }     // (no bin qualifies only for a row without mass: no token is kept then)
  T v[4], s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) { v[j] = h[SMP_BINS - 1 - 4 * t - j]; s += v[j]; }
  T above = block_excl_scan<T>(s, red, (T*)nullptr);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (above < thr && thr <= above + v[j]) { *out_bin = SMP_BINS - 1 - 4 * t - j; *out_above = above; }
    above += v[j];
  }
  __syncthreads();
}
