// Sampled decoding: temperature -> top-k -> top-p -> one draw per row, over the bf16 logits lm_head wrote ("Sampled
// decoding").  One LIA_ROW_THREADS workgroup per row, in the shape of lia_argmax_kernel; nothing is sorted.
//
// tau > 0 makes s = fp32(l) / tau a non-decreasing function of l, and l is bf16, so a row's order is the order of a 16-bit key of
// its logits (key_of: sign-magnitude -> offset binary) and every per-token quantity -- s, the weight exp(s - m) -- is a function of
// the key.  The boundaries are found from histograms of keys, 4096 bins of the top 12 key bits then 16 bins of the low 4 inside the
// boundary bin (12 + 4 rather than 8 + 8: the top byte of a bf16 is its sign and exponent, and a row's logits fill only a few
// exponents -- the LDS atomics of 64 lanes would pile onto a handful of bins):
//   pass A  max key (m = s of it) and, with top-k on, counts per top-12 bin -> the bin holding the k-th largest key
//   pass B  (top-k) counts per low nibble inside that bin -> kappa_k, t_k = s(kappa_k)
//   pass C  (top-p) mass per top-12 bin over K1, in 2^-40 fixed point (u64 LDS atomics: exact integer sums, the same in every run)
//   pass D  (top-p) mass per low nibble inside the boundary bin -> kappa_p, v_p = s(kappa_p)
//   pass E  tiles of 8 tokens per thread in token order: block prefix sums of the kept weights, one carry per tile; then the tile
//           where the running sum passes u * W is walked again for the token.
// Membership is a key comparison: K = {key >= kappa_lo(t)}, kappa_lo(t) the smallest key whose s is >= t (a 16-step bisection by
// one thread).  That is s_i >= t exactly, also where two keys give the same s (-0 / +0, or an s that rounds to 0 or inf).  A token
// whose s is -inf (the suppressed one) carries no mass and is never kept.  Logits are finite or +-inf, not NaN.
#include "lia_row_passes.h"   // key_of, load_keys8, block_excl_scan, find_boundary_bin and the SMP_ key constants

#define SMP_MAX_TILES 256                // pass-E carries kept in LDS: vocab <= 256 * 8192 (lia_sample checks)
#define SMP_FIX 0x1p40f                  // fixed-point scale of the top-p masses (w <= 1, vocab <= 2^21: sums < 2^61)

__device__ __forceinline__ float score_of_key(int k, float tau) {
  const uint32_t h = (k & 0x8000) ? (uint32_t)(k & 0x7FFF) : (uint32_t)(~k & 0xFFFF);
  return bf2f((bf16_t)h) / tau;                // the IEEE fp32 division of the contract
}

// smallest key in (-inf, +inf] whose score is >= t (keys above SMP_KEY_NEG_INF: a -inf score is never kept)
__device__ int key_lower_bound(float t, float tau) {
  int lo = SMP_KEY_NEG_INF + 1, hi = SMP_KEY_POS_INF + 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (score_of_key(mid, tau) >= t) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// The row passes' LDS, shared by every kernel of this file (each is one row workgroup running the passes one after the other)
__shared__ uint64_t hist[SMP_BINS];            // pass A: uint32 counts (the first half), pass C: uint64 masses
__shared__ uint64_t nib[16];                   // passes B / D: the 16 low-nibble bins of the boundary bin
__shared__ uint64_t red64[LIA_ROW_WAVES];
__shared__ uint32_t red32[LIA_ROW_WAVES];
__shared__ float redf[LIA_ROW_WAVES];
__shared__ float carry_of[SMP_MAX_TILES + 1];  // pass E: running sum before tile j
__shared__ int sh_bin, sh_key[2], sh_pick;
__shared__ uint32_t sh_above32;
__shared__ uint64_t sh_above64;
__shared__ float sh_wd;                        // DRAFT: the draft token's kept weight

// What one row's draw leaves behind for the caller (the same values in every thread; the kernels use thread 0's): the id,
// lia_sample's four stats, and -- DRAFT only -- the kept weight exp(s - m) of the draft token (0 where it is not kept)
struct SmpRow { int pick; float t_k, v_p, nkept, W2, w_draft; };

// Passes A - D over one row by the whole LIA_ROW_THREADS workgroup: the row's kept set K2 = {key >= kap2} and the score m of its maximum
// (the weight of a kept token is exp(s - m)), the same values in every thread.  t_k / v_p: lia_sample's boundary stats.
struct SmpFilt { int kap2; float m, t_k, v_p; };

template <int MASKED = 0>
__device__ __forceinline__ SmpFilt filter_row(const bf16_t* __restrict__ row, int vocab, bool vec, float tau, int top_k, float top_p,
                                              int suppress, const uint8_t* __restrict__ mrow = nullptr) {
  uint32_t* cnt = (uint32_t*)hist;

  const int tid = threadIdx.x;
  const bool topk_on = top_k > 0 && top_k < vocab;
  const bool topp_on = top_p < 1.0f;

  // ---- pass A: the maximum key; with top-k on, counts per top-12 bin ----
  if (topk_on)
    for (int b = tid; b < SMP_BINS / 2; b += LIA_ROW_THREADS) hist[b] = 0;
  __syncthreads();
  int kmax = -1;
  for (int i = tid * 8; i < vocab; i += SMP_TILE) {
    int k[8];
    load_keys8<MASKED>(row, i, vocab, vec, suppress, k, mrow);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      kmax = max(kmax, k[e]);
      if (topk_on && k[e] >= 0) atomicAdd(&cnt[k[e] >> 4], 1u);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, __shfl_xor(kmax, o, 64));
  if ((tid & 63) == 0) red32[tid >> 6] = (uint32_t)kmax;
  __syncthreads();
  kmax = (int)red32[0];
#pragma unroll
  for (int w = 1; w < LIA_ROW_WAVES; ++w) kmax = max(kmax, (int)red32[w]);
  const float m = score_of_key(kmax, tau);
  __syncthreads();                   // (red32 is reused below)

  // ---- pass B: the k-th largest key ----
  int kap1 = SMP_KEY_NEG_INF + 1;    // K1 = {key >= kap1}
  float t_k = -INFINITY;
  if (topk_on) {
    find_boundary_bin<uint32_t>(cnt, (uint32_t)top_k, red32, &sh_bin, &sh_above32);
    const int bk = sh_bin;
    if (tid < 16) nib[tid] = 0;
    __syncthreads();
    for (int i = tid * 8; i < vocab; i += SMP_TILE) {
      int k[8];
      load_keys8<MASKED>(row, i, vocab, vec, suppress, k, mrow);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (k[e] >= 0 && (k[e] >> 4) == bk) atomicAdd((uint32_t*)&nib[k[e] & 15], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t above = sh_above32;
      int l = 15;
      for (; l > 0; --l) {
        const uint32_t c = *(const uint32_t*)&nib[l];
        if (above + c >= (uint32_t)top_k) break;
        above += c;
      }
      const int kk = (bk << 4) | l;
      sh_key[0] = key_lower_bound(score_of_key(kk, tau), tau);
      sh_key[1] = kk;
    }
    __syncthreads();
    kap1 = sh_key[0];
    t_k = score_of_key(sh_key[1], tau);
  }

  // ---- passes C and D: the top-p boundary over K1 ----
  int kap2 = kap1;                   // K2 = {key >= kap2}
  float v_p = -INFINITY;
  if (topp_on) {
    for (int b = tid; b < SMP_BINS; b += LIA_ROW_THREADS) hist[b] = 0;
    if (tid < 16) nib[tid] = 0;
    __syncthreads();
    for (int i = tid * 8; i < vocab; i += SMP_TILE) {
      int k[8];
      load_keys8<MASKED>(row, i, vocab, vec, suppress, k, mrow);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (k[e] >= kap1) {
          const uint64_t f = __float2ull_rn(expf(score_of_key(k[e], tau) - m) * SMP_FIX);
          if (f) atomicAdd((unsigned long long*)&hist[k[e] >> 4], (unsigned long long)f);
        }
    }
    __syncthreads();
    // W = the sum of every bin (the scan's total); the threshold p * W rounded up, so that A < p W <=> A < X for integers A
    uint64_t s4 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) s4 += hist[4 * tid + j];
    uint64_t W;
    (void)block_excl_scan<uint64_t>(s4, red64, &W);
    uint64_t X = (uint64_t)ceil((double)top_p * (double)W);
    if (X < 1) X = 1;
    find_boundary_bin<uint64_t>(hist, X, red64, &sh_bin, &sh_above64);
    const int bp = sh_bin;
    for (int i = tid * 8; i < vocab; i += SMP_TILE) {
      int k[8];
      load_keys8<MASKED>(row, i, vocab, vec, suppress, k, mrow);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (k[e] >= kap1 && (k[e] >> 4) == bp) {
          const uint64_t f = __float2ull_rn(expf(score_of_key(k[e], tau) - m) * SMP_FIX);
          if (f) atomicAdd((unsigned long long*)&nib[k[e] & 15], (unsigned long long)f);
        }
    }
    __syncthreads();
    if (tid == 0) {
      uint64_t above = sh_above64;
      int l = 15;
      for (; l > 0; --l) {
        if (above + nib[l] >= X) break;
        above += nib[l];
      }
      const int kp = (bp << 4) | l;
      sh_key[0] = key_lower_bound(score_of_key(kp, tau), tau);
      sh_key[1] = kp;
    }
    __syncthreads();
    kap2 = max(kap1, sh_key[0]);
    v_p = score_of_key(sh_key[1], tau);
  }

  SmpFilt f;
  f.kap2 = kap2;
  f.m = m;
  f.t_k = t_k;
  f.v_p = v_p;
  return f;
}

// Passes A - E over one row by the whole LIA_ROW_THREADS workgroup: the one function lia_sample_kernel and lia_verify_sample_kernel
// both draw with, so that a verify pass's token IS lia_sample's of the same logits and u.  u must be workgroup-uniform.  DRAFT: the
// thread that meets token `draft` in pass E also leaves its kept weight (no further pass over the row).
template <bool DRAFT, int MASKED = 0>
__device__ __forceinline__ SmpRow sample_row(const bf16_t* __restrict__ row, int vocab, bool vec, float tau, int top_k, float top_p,
                                             int suppress, float u, int draft, const uint8_t* __restrict__ mrow = nullptr) {
  const int tid = threadIdx.x;
  if (DRAFT && tid == 0) sh_wd = 0.f;              // (pass A's barrier orders it before the owner's store in pass E)
  const SmpFilt f = filter_row<MASKED>(row, vocab, vec, tau, top_k, top_p, suppress, mrow);
  const int kap2 = f.kap2;
  const float m = f.m, t_k = f.t_k, v_p = f.v_p;

  // ---- pass E: running sums of the kept weights in token order, one carry per tile ----
  const int ntiles = (vocab + SMP_TILE - 1) / SMP_TILE;
  float carry = 0.f;
  int nkept = 0, last = -1;
  for (int j = 0; j < ntiles; ++j) {
    const int i = j * SMP_TILE + tid * 8;
    int k[8];
    load_keys8<MASKED>(row, i, vocab, vec, suppress, k, mrow);
    float r = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (k[e] >= kap2) {
        const float w = expf(score_of_key(k[e], tau) - m);
        r += w; ++nkept; last = i + e;
        if (DRAFT && i + e == draft) sh_wd = w;
      }
    const float ex = block_excl_scan<float>(r, redf, (float*)nullptr);
    if (tid == LIA_ROW_THREADS - 1) {
      carry_of[j] = carry;
      redf[0] = ex + r;               // the tile's total as the walk below computes it at the tile's last token
    }
    __syncthreads();
    carry = carry + redf[0];
    __syncthreads();
  }
  if (tid == 0) carry_of[ntiles] = carry;
  // |K2| and the last kept token
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nkept += __shfl_xor(nkept, o, 64);
    last = max(last, __shfl_xor(last, o, 64));
  }
  if ((tid & 63) == 0) { red32[tid >> 6] = (uint32_t)nkept; red64[tid >> 6] = (uint64_t)(int64_t)last; }
  if (tid == 0) sh_pick = 0x7fffffff;
  __syncthreads();
  nkept = 0;
#pragma unroll
  for (int w = 0; w < LIA_ROW_WAVES; ++w) { nkept += (int)red32[w]; last = max(last, (int)(int64_t)red64[w]); }
  const float W2 = carry;
  const float thr = u * W2;
  int jc = -1;                        // the first tile whose running sum passes thr
  for (int j = 0; j < ntiles; ++j)
    if (carry_of[j + 1] > thr) { jc = j; break; }
  if (jc >= 0) {
    // walk tile jc again: the same sums in the same order, then the first kept token whose running sum passes thr
    const int i = jc * SMP_TILE + tid * 8;
    int k[8];
    load_keys8<MASKED>(row, i, vocab, vec, suppress, k, mrow);
    float wv[8], r = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      wv[e] = k[e] >= kap2 ? expf(score_of_key(k[e], tau) - m) : 0.f;
      r += wv[e];
    }
    const float ex = block_excl_scan<float>(r, redf, (float*)nullptr);
    const float c0 = carry_of[jc];
    float q = 0.f;
    int pick = 0x7fffffff, lastc = -1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      q += wv[e];
      if (k[e] >= kap2) {
        lastc = i + e;
        if (pick == 0x7fffffff && c0 + (ex + q) > thr) pick = i + e;
      }
    }
    if (pick != 0x7fffffff) atomicMin(&sh_pick, pick);
    // (the tile's total passed thr, so a kept token of it does; should rounding say otherwise, its last kept token)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lastc = max(lastc, __shfl_xor(lastc, o, 64));
    if ((tid & 63) == 0) red32[tid >> 6] = (uint32_t)lastc;
    __syncthreads();
    if (tid == 0 && sh_pick == 0x7fffffff) {
      int lc = -1;
      for (int w = 0; w < LIA_ROW_WAVES; ++w) lc = max(lc, (int)red32[w]);
      sh_pick = lc;
    }
    __syncthreads();
  }
  SmpRow res;
  int pick = jc >= 0 ? sh_pick : last;
  if (pick < 0 || pick >= vocab) pick = last >= 0 ? last : 0;
  res.pick = pick;
  res.t_k = t_k;
  res.v_p = v_p;
  res.nkept = (float)nkept;
  res.W2 = W2;
  res.w_draft = DRAFT ? sh_wd : 0.f;
  return res;
}

// MASKED (lia_ctx_set_token_mask): row r draws under the allowed-token bit row mask + r * ldm (ldm words; 0: one row for every row)
template <int MASKED>
__global__ __launch_bounds__(LIA_ROW_THREADS) void lia_sample_kernel(const bf16_t* __restrict__ logits, long ld, int vocab, int vec,
                                                                     float tau, int top_k, float top_p, int suppress,
                                                                     const float* __restrict__ uniforms, int64_t* __restrict__ out,
                                                                     float* __restrict__ stats, const uint32_t* __restrict__ mask, long ldm) {
  const uint8_t* mrow = MASKED ? (const uint8_t*)(mask + (long)blockIdx.x * ldm) : nullptr;
  const SmpRow r = sample_row<false, MASKED>(logits + (long)blockIdx.x * ld, vocab, vec, tau, top_k, top_p, suppress, uniforms[blockIdx.x], -1,
                                             mrow);
  if (threadIdx.x == 0) {
    out[blockIdx.x] = r.pick;
    if (stats) {
      float* so = stats + 4 * (long)blockIdx.x;
      so[0] = r.t_k;
      so[1] = r.v_p;
      so[2] = r.nkept;
      so[3] = r.W2;
    }
  }
}

// Speculative sampling ("Sampled verification"): lia_sample's draw behind every position of a draft block.  Chunk row
// r = r0 + blockIdx.x of the block is block row b = r / T at position t = r % T; `suppress` counts as -inf where t is below
// n_suppress_rows[b] (or n_suppress with a NULL table); the draw uses U[s, b] of the generation's table (ldu floats per step) at
// step s = step_rows[b] (or step0) + t -- and u = 0 without a read at s >= n_steps, a position that can never be kept.  The table
// entry is wave-uniform and goes through readfirstlane: the pass bounds that depend on it stay scalar.  p_draft (or NULL): the
// probability that this position's draw confirms the draft token block_ids[b, t + 1] -- its kept weight over the kept mass, 0 where
// it is not kept and at t = T - 1.  MASKED (lia_ctx_set_token_mask): the BLOCK row's mask row, mask + r * ldm words (a chunk boundary
// inside a block row changes r0, never r).
template <int MASKED>
__global__ __launch_bounds__(LIA_ROW_THREADS) void lia_verify_sample_kernel(const bf16_t* __restrict__ logits, long ld, int vocab, int vec,
                                                                            float tau, int top_k, float top_p, int suppress,
                                                                            int n_suppress, const int* __restrict__ n_suppress_rows,
                                                                            int T, int r0, const float* __restrict__ uniforms, long ldu,
                                                                            int n_steps, int step0, const int* __restrict__ step_rows,
                                                                            const int64_t* __restrict__ block_ids,
                                                                            int64_t* __restrict__ sampled, float* __restrict__ p_draft,
                                                                            const uint32_t* __restrict__ mask, long ldm) {
  const int r = r0 + (int)blockIdx.x;
  const int b = r / T, t = r % T;
  const int sup = t < (n_suppress_rows ? __builtin_amdgcn_readfirstlane(n_suppress_rows[b]) : n_suppress) ? suppress : -1;
  const long s = (long)(step_rows ? __builtin_amdgcn_readfirstlane(step_rows[b]) : step0) + t;
  float u = 0.f;
  if (s >= 0 && s < n_steps) u = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(uniforms[s * ldu + b])));
  int draft = -1;
  if (p_draft && t < T - 1) {
    const int64_t d = block_ids[(long)r + 1];
    draft = d >= 0 && d < (int64_t)vocab ? (int)d : -1;
  }
  const uint8_t* mrow = MASKED ? (const uint8_t*)(mask + (long)r * ldm) : nullptr;
  const SmpRow o = sample_row<true, MASKED>(logits + (long)blockIdx.x * ld, vocab, vec, tau, top_k, top_p, sup, u, draft, mrow);
  if (threadIdx.x == 0) {
    sampled[r] = o.pick;
    if (p_draft) p_draft[r] = o.w_draft > 0.f ? o.w_draft / o.W2 : 0.f;
  }
}

// ---- rejection verification ("Rejection verification") ------------------------------------------------------
// the probabilities of tokens i .. i + 7 under a filtered row: kept weight over kept mass, 0 for a token that is not kept (or past
// the end of the row)
__device__ __forceinline__ void load_probs8(const bf16_t* __restrict__ row, int i, int vocab, bool vec, int suppress, float tau, int kap2,
                                            float m, float W, float p[8]) {
  int k[8];
  load_keys8(row, i, vocab, vec, suppress, k);
#pragma unroll
  for (int e = 0; e < 8; ++e) p[e] = k[e] >= kap2 ? expf(score_of_key(k[e], tau) - m) / W : 0.f;
}

// Chunk row r = r0 + blockIdx.x is block row b = r / T at position t = r % T.  At t < T - 1 the draft token x = block_ids[b, t + 1]
// was drawn from Q_t, the filtered distribution of draft_logits[b, t, :] (the target's settings, the same suppress rule); P_t is that
// of this pass's logits row.  Passes A - D run on the target row, then on the draft row (the same LDS); one pass over both rows sums
// their kept weights (a fixed-order reduction: W_p, W_q); one more, in pass E's tiling, the running residual r_i = max(P_t(i) -
// Q_t(i), 0) in token order -- the thread that meets x leaves P_t(x) and Q_t(x) -- and the tile where the running sum passes
// U_res[s, b] * R is walked again for the token (else the last id with r_i > 0).  ok = (Q_t(x) > 0 and U_acc[s, b] * Q_t(x) < P_t(x))
// at step s = step0 + t; a position with s >= n_steps reads no table entry and is rejected.  R == 0 (P_t <= Q_t everywhere: P_t = Q_t)
// and t = T - 1 (the bonus token) take the plain draw of P_t with U_res[s, b]: sample_row, lia_sample's own function.
__global__ __launch_bounds__(LIA_ROW_THREADS) void lia_verify_reject_kernel(
    const bf16_t* __restrict__ logits, long ld, int vocab, int vec, const bf16_t* __restrict__ draft_logits, long ldd_row, long ldd_pos,
    int vecd, float tau, int top_k, float top_p, int suppress, int n_suppress, int T, int r0, const float* __restrict__ u_acc,
    const float* __restrict__ u_res, long ldu, int n_steps, int step0, const int64_t* __restrict__ block_ids, int64_t* __restrict__ token,
    int* __restrict__ ok, float* __restrict__ p_tok, float* __restrict__ q_tok, float* __restrict__ resid_mass) {
  __shared__ float sh_px, sh_qx;
  const int tid = threadIdx.x;
  const int r = r0 + (int)blockIdx.x;
  const int b = r / T, t = r % T;
  const int sup = t < n_suppress ? suppress : -1;
  const long s = (long)step0 + t;
  const bool inside = s >= 0 && s < n_steps;
  float ua = 0.f, ur = 0.f;
  if (inside) {
    ua = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(u_acc[s * ldu + b])));
    ur = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(u_res[s * ldu + b])));
  }
  const bf16_t* prow = logits + (long)blockIdx.x * ld;
  bool plain = t == T - 1;
  int pick = 0, accept = 0;
  float px = 0.f, qx = 0.f, R = 0.f;
  if (!plain) {
    const bf16_t* qrow = draft_logits + (long)b * ldd_row + (long)t * ldd_pos;
    const int64_t d = block_ids[(long)r + 1];
    const int x = d >= 0 && d < (int64_t)vocab ? (int)d : -1;
    if (tid == 0) { sh_px = 0.f; sh_qx = 0.f; }
    const SmpFilt fp = filter_row(prow, vocab, vec, tau, top_k, top_p, sup);
    __syncthreads();                      // (the draft row's passes reuse the LDS the target row's last reads came from)
    const SmpFilt fq = filter_row(qrow, vocab, vecd, tau, top_k, top_p, sup);
    // ---- the kept masses: per-thread sums in token order, then the waves in order ----
    float wp = 0.f, wq = 0.f;
    for (int i = tid * 8; i < vocab; i += SMP_TILE) {
      int kp[8], kq[8];
      load_keys8(prow, i, vocab, vec, sup, kp);
      load_keys8(qrow, i, vocab, vecd, sup, kq);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (kp[e] >= fp.kap2) wp += expf(score_of_key(kp[e], tau) - fp.m);
        if (kq[e] >= fq.kap2) wq += expf(score_of_key(kq[e], tau) - fq.m);
      }
    }
    float Wp, Wq;
    (void)block_excl_scan<float>(wp, redf, &Wp);
    (void)block_excl_scan<float>(wq, redf, &Wq);
    // ---- the running residual in token order, one carry per tile ----
    const int ntiles = (vocab + SMP_TILE - 1) / SMP_TILE;
    float carry = 0.f;
    int last = -1;
    for (int j = 0; j < ntiles; ++j) {
      const int i = j * SMP_TILE + tid * 8;
      float pv[8], qv[8], rs = 0.f;
      load_probs8(prow, i, vocab, vec, sup, tau, fp.kap2, fp.m, Wp, pv);
      load_probs8(qrow, i, vocab, vecd, sup, tau, fq.kap2, fq.m, Wq, qv);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float re = fmaxf(pv[e] - qv[e], 0.f);
        rs += re;
        if (re > 0.f) last = i + e;
        if (i + e == x) { sh_px = pv[e]; sh_qx = qv[e]; }
      }
      const float ex = block_excl_scan<float>(rs, redf, (float*)nullptr);
      if (tid == LIA_ROW_THREADS - 1) {
        carry_of[j] = carry;
        redf[0] = ex + rs;              // the tile's total as the walk below computes it at the tile's last token
      }
      __syncthreads();
      carry = carry + redf[0];
      __syncthreads();
    }
    if (tid == 0) carry_of[ntiles] = carry;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
    if ((tid & 63) == 0) red32[tid >> 6] = (uint32_t)last;
    if (tid == 0) sh_pick = 0x7fffffff;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < LIA_ROW_WAVES; ++w) last = max(last, (int)red32[w]);
    px = sh_px;
    qx = sh_qx;
    R = carry;
    accept = inside && qx > 0.f && ua * qx < px;
    const float thr = ur * R;
    int jc = -1;                        // the first tile whose running sum passes thr
    for (int j = 0; j < ntiles; ++j)
      if (carry_of[j + 1] > thr) { jc = j; break; }
    __syncthreads();                    // (red32 is reused below)
    if (jc >= 0) {
      // walk tile jc again: the same sums in the same order, then the first token with r_i > 0 whose running sum passes thr
      const int i = jc * SMP_TILE + tid * 8;
      float pv[8], qv[8], rv[8], rs = 0.f;
      load_probs8(prow, i, vocab, vec, sup, tau, fp.kap2, fp.m, Wp, pv);
      load_probs8(qrow, i, vocab, vecd, sup, tau, fq.kap2, fq.m, Wq, qv);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        rv[e] = fmaxf(pv[e] - qv[e], 0.f);
        rs += rv[e];
      }
      const float ex = block_excl_scan<float>(rs, redf, (float*)nullptr);
      const float c0 = carry_of[jc];
      float q = 0.f;
      int pk = 0x7fffffff, lastc = -1;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        q += rv[e];
        if (rv[e] > 0.f) {
          lastc = i + e;
          if (pk == 0x7fffffff && c0 + (ex + q) > thr) pk = i + e;
        }
      }
      if (pk != 0x7fffffff) atomicMin(&sh_pick, pk);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) lastc = max(lastc, __shfl_xor(lastc, o, 64));
      if ((tid & 63) == 0) red32[tid >> 6] = (uint32_t)lastc;
      __syncthreads();
      if (tid == 0 && sh_pick == 0x7fffffff) {
        int lc = -1;
        for (int w = 0; w < LIA_ROW_WAVES; ++w) lc = max(lc, (int)red32[w]);
        sh_pick = lc;
      }
      __syncthreads();
    }
    pick = jc >= 0 ? sh_pick : last;
    if (pick < 0 || pick >= vocab) pick = last >= 0 ? last : 0;
    plain = !(R > 0.f);
    __syncthreads();                    // (the plain draw below reuses every LDS word read above)
  }
  if (plain) pick = sample_row<false>(prow, vocab, vec, tau, top_k, top_p, sup, ur, -1).pick;
  if (tid == 0) {
    token[r] = pick;
    ok[r] = accept;
    if (p_tok) p_tok[r] = px;
    if (q_tok) q_tok[r] = qx;
    if (resid_mass) resid_mass[r] = R;
  }
}

// one workgroup: accepted[b] = the first position whose draft token was rejected (T - 1: none, or an inactive row), common = their
// minimum, next[b] = the draft token behind position `common` where row b accepted it, else the token the head computed there
__global__ __launch_bounds__(256) void lia_verify_reject_accept_kernel(const int64_t* __restrict__ block_ids, const int64_t* __restrict__ token,
                                                                       const int* __restrict__ ok, const int* __restrict__ active, int B, int T,
                                                                       int* __restrict__ accepted, int* __restrict__ common,
                                                                       int64_t* __restrict__ next) {
  __shared__ int smin[4];
  const int tid = threadIdx.x;
  int lo = T - 1;
  for (int b = tid; b < B; b += 256) {
    int a = T - 1;
    if (!active || active[b]) {
      a = 0;
      while (a < T - 1 && ok[(long)b * T + a]) ++a;
    }
    accepted[b] = a;
    lo = min(lo, a);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lo = min(lo, __shfl_xor(lo, o, 64));
  if ((tid & 63) == 0) smin[tid >> 6] = lo;
  __syncthreads();
  lo = min(min(smin[0], smin[1]), min(smin[2], smin[3]));
  if (tid == 0) common[0] = lo;
  // (each thread reads back the accepted[] entries it wrote itself)
  for (int b = tid; b < B; b += 256) next[b] = accepted[b] > lo ? block_ids[(long)b * T + lo + 1] : token[(long)b * T + lo];
}

extern "C" void lia_sample_launch(const bf16_t* logits, long ld, int B, int vocab, float tau, int top_k, float top_p, int suppress,
                                  const float* uniforms, int64_t* out, float* stats, hipStream_t st) {
  if (B <= 0) return;
  const int vec = (ld % 8 == 0) && (vocab % 8 == 0) && (((uintptr_t)logits & 15) == 0);
  hipLaunchKernelGGL(lia_sample_kernel<0>, dim3(B), dim3(LIA_ROW_THREADS), 0, st, logits, ld, vocab, vec, tau, top_k, top_p, suppress,
                     uniforms, out, stats, (const uint32_t*)nullptr, 0L);
}

// mask: device, row r at mask + r * ldm words (ldm >= ceil(vocab / 32), or 0: one row for every row)
extern "C" void lia_sample_masked_launch(const bf16_t* logits, long ld, int B, int vocab, float tau, int top_k, float top_p, int suppress,
                                         const float* uniforms, int64_t* out, float* stats, const uint32_t* mask, long ldm, hipStream_t st) {
  if (B <= 0) return;
  const int vec = (ld % 8 == 0) && (vocab % 8 == 0) && (((uintptr_t)logits & 15) == 0);
  hipLaunchKernelGGL(lia_sample_kernel<1>, dim3(B), dim3(LIA_ROW_THREADS), 0, st, logits, ld, vocab, vec, tau, top_k, top_p, suppress,
                     uniforms, out, stats, mask, ldm);
}

extern "C" void lia_verify_sample_launch(const bf16_t* logits, long ld, int n, int vocab, float tau, int top_k, float top_p, int suppress,
                                         int n_suppress, const int* n_suppress_rows, int T, int r0, const float* uniforms, long ldu,
                                         int n_steps, int step0, const int* step_rows, const int64_t* block_ids, int64_t* sampled,
                                         float* p_draft, hipStream_t st) {
  if (n <= 0) return;
  const int vec = (ld % 8 == 0) && (vocab % 8 == 0) && (((uintptr_t)logits & 15) == 0);
  hipLaunchKernelGGL(lia_verify_sample_kernel<0>, dim3(n), dim3(LIA_ROW_THREADS), 0, st, logits, ld, vocab, vec, tau, top_k, top_p, suppress,
                     n_suppress, n_suppress_rows, T, r0, uniforms, ldu, n_steps, step0, step_rows, block_ids, sampled, p_draft,
                     (const uint32_t*)nullptr, 0L);
}

// mask: device, block row r0 + i of the chunk at mask + (r0 + i) * ldm words (ldm >= ceil(vocab / 32), or 0: one row for every row)
extern "C" void lia_verify_sample_masked_launch(const bf16_t* logits, long ld, int n, int vocab, float tau, int top_k, float top_p,
                                                int suppress, int n_suppress, const int* n_suppress_rows, int T, int r0,
                                                const float* uniforms, long ldu, int n_steps, int step0, const int* step_rows,
                                                const int64_t* block_ids, int64_t* sampled, float* p_draft, const uint32_t* mask, long ldm,
                                                hipStream_t st) {
  if (n <= 0) return;
  const int vec = (ld % 8 == 0) && (vocab % 8 == 0) && (((uintptr_t)logits & 15) == 0);
  hipLaunchKernelGGL(lia_verify_sample_kernel<1>, dim3(n), dim3(LIA_ROW_THREADS), 0, st, logits, ld, vocab, vec, tau, top_k, top_p, suppress,
                     n_suppress, n_suppress_rows, T, r0, uniforms, ldu, n_steps, step0, step_rows, block_ids, sampled, p_draft, mask, ldm);
}

extern "C" void lia_verify_reject_launch(const bf16_t* logits, long ld, int n, int vocab, const bf16_t* draft_logits, long ldd_row,
                                         long ldd_pos, float tau, int top_k, float top_p, int suppress, int n_suppress, int T, int r0,
                                         const float* u_acc, const float* u_res, long ldu, int n_steps, int step0, const int64_t* block_ids,
                                         int64_t* token, int* ok, float* p_tok, float* q_tok, float* resid_mass, hipStream_t st) {
  if (n <= 0) return;
  const int vec = (ld % 8 == 0) && (vocab % 8 == 0) && (((uintptr_t)logits & 15) == 0);
  const int vecd = (ldd_row % 8 == 0) && (ldd_pos % 8 == 0) && (vocab % 8 == 0) && (((uintptr_t)draft_logits & 15) == 0);
  hipLaunchKernelGGL(lia_verify_reject_kernel, dim3(n), dim3(LIA_ROW_THREADS), 0, st, logits, ld, vocab, vec, draft_logits, ldd_row, ldd_pos,
                     vecd, tau, top_k, top_p, suppress, n_suppress, T, r0, u_acc, u_res, ldu, n_steps, step0, block_ids, token, ok, p_tok,
                     q_tok, resid_mass);
}

extern "C" void lia_verify_reject_accept_launch(const int64_t* block_ids, const int64_t* token, const int* ok, const int* active, int B, int T,
                                                int* accepted, int* common, int64_t* next, hipStream_t st) {
  if (B <= 0) return;
  hipLaunchKernelGGL(lia_verify_reject_accept_kernel, dim3(1), dim3(256), 0, st, block_ids, token, ok, active, B, T, accepted, common, next);
}
