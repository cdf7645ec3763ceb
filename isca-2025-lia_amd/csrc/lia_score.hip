// Scoring: per row of bf16 logits, log p(target) and the greedy token ("Scoring").  One LIA_ROW_THREADS workgroup per
// row, in the shape of lia_argmax_kernel: 16-byte loads of 8 logits, wave reduction by __shfl_xor, then the waves through LDS.
//
// Two passes over the row, both as fp32 of the bf16 logits:
//   pass 1  m = max_j l_j and the first index that holds it (lia_argmax_kernel's tie rule: the lowest index wins)
//   pass 2  s = sum_j exp(l_j - m): every lane adds its own terms in index order (LIA_SCORE_SERIAL(vocab) of them at most), then a
//           balanced tree over the LIA_ROW_THREADS lanes (6 shuffle levels inside a wave, 4 over the 16 wave totals)
//   logprobs[r] = l_target - (m + log s)
// The second pass finds the row (100 KB at vocab 50272, 256 KB at 128256) in L2, where the first pass left it: HBM is read once.
// An online (m, s) pair per lane reads the row once and rescales s at every new maximum: measured a third faster per launch
// (tools/score_row_bench.hip: 126 against 198 us for 4096 rows of 50272), 0.07 ms beside the 2 ms of GEMM that fill such a chunk, and
// not taken -- its extra roundings have no bound as short as the one above.
// exp is ocml's expf (about 1 ulp), log is logf.  -inf logits add exactly 0; a row of nothing but -inf has no distribution and
// gives NaN.  A target outside [0, vocab) -- -1 is the documented "no target" -- gives 0.0.  Logits are finite or +-inf, not NaN.
#include "lia_row_passes.h"   // load_logits8 and the two passes (row_max_sum), shared with lia_topn_logprobs_kernel

static_assert(LIA_ROW_THREADS == LIA_SCORE_ROW_THREADS, "lia_hip.h states the row kernel's lane count for the error bound of its tests");

__global__ __launch_bounds__(LIA_ROW_THREADS) void lia_token_logprobs_kernel(const bf16_t* __restrict__ logits, long ld, int vocab, int vec,
                                                                             const int64_t* __restrict__ targets,
                                                                             float* __restrict__ logprobs, int64_t* __restrict__ greedy) {
  const bf16_t* row = logits + (long)blockIdx.x * ld;
  const RowMaxSum p = row_max_sum(row, vocab, vec);
  if (threadIdx.x == 0) {
    greedy[blockIdx.x] = p.bi == 0x7fffffff ? 0 : p.bi;
    logprobs[blockIdx.x] = row_logprob(row, vocab, targets[blockIdx.x], p.m, p.s);
  }
}

extern "C" void lia_token_logprobs_launch(const bf16_t* logits, long ld, int M, int vocab, const int64_t* targets, float* logprobs,
                                          int64_t* greedy, hipStream_t st) {
  if (M <= 0) return;
  const int vec = (ld % 8 == 0) && (vocab % 8 == 0) && (((uintptr_t)logits & 15) == 0);
  hipLaunchKernelGGL(lia_token_logprobs_kernel, dim3(M), dim3(LIA_ROW_THREADS), 0, st, logits, ld, vocab, vec, targets, logprobs, greedy);
}

// ------------------------------------------------------------------------------------------------
// speculative verification (lia_lm_verify): the argmax of a chunk of block rows, then what the block's rows accept
// ------------------------------------------------------------------------------------------------
// lia_argmax_kernel's scan and tie rule over row r0 + blockIdx.x of the block; `suppress` counts as -inf where the row's block
// position (r0 + blockIdx.x) % T is below n_suppress -- or, with n_suppress_rows (int32 per block row b = (r0 + blockIdx.x) / T, or
// NULL), below n_suppress_rows[b].  MASKED (lia_ctx_set_token_mask): a token whose bit in the BLOCK row's mask row,
// mask + (r0 + blockIdx.x) * ldm words, is clear counts as -inf too; the lane's 8 tokens start at a multiple of 8, so one mask byte
// covers them on both load paths (bits at or beyond vocab are never looked at).
template <int MASKED>
__global__ __launch_bounds__(LIA_ROW_THREADS) void lia_verify_argmax_kernel(const bf16_t* __restrict__ logits, long ld, int vocab, int vec,
                                                                            int suppress, int n_suppress, int T, int r0,
                                                                            int64_t* __restrict__ greedy,
                                                                            const int* __restrict__ n_suppress_rows,
                                                                            const uint32_t* __restrict__ mask, long ldm) {
  __shared__ float sv[LIA_ROW_WAVES];
  __shared__ int si[LIA_ROW_WAVES];
  const int tid = threadIdx.x, lane = tid & 63;
  const bf16_t* row = logits + (long)blockIdx.x * ld;
  const uint8_t* mrow = MASKED ? (const uint8_t*)(mask + (long)(r0 + (int)blockIdx.x) * ldm) : nullptr;
  const int brow = (r0 + (int)blockIdx.x) / T;
  const int sup = (r0 + (int)blockIdx.x) % T < (n_suppress_rows ? n_suppress_rows[brow] : n_suppress) ? suppress : -1;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = tid * 8; i < vocab; i += LIA_ROW_THREADS * 8) {
    float f[8];
    load_logits8(row, i, vocab, vec, f);
    uint32_t allow = 0xffu;
    if constexpr (MASKED) allow = mrow[i >> 3];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = i + e == sup ? -INFINITY : f[e];
      if constexpr (MASKED) v = (allow >> e) & 1u ? v : -INFINITY;
      if (i + e < vocab && (v > best || (v == best && i + e < bi))) { best = v; bi = i + e; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  if (lane == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < LIA_ROW_WAVES; ++w)
      if (sv[w] > best || (sv[w] == best && si[w] < bi)) { best = sv[w]; bi = si[w]; }
    greedy[r0 + blockIdx.x] = bi == 0x7fffffff ? 0 : bi;
  }
}

// one workgroup: accepted[b] per row, their minimum, next[b] = greedy[b, common]
__global__ __launch_bounds__(256) void lia_verify_accept_kernel(const int64_t* __restrict__ block_ids, const int64_t* __restrict__ greedy,
                                                                const int* __restrict__ active, int B, int T, int* __restrict__ accepted,
                                                                int* __restrict__ common, int64_t* __restrict__ next) {
  __shared__ int smin[4];
  const int tid = threadIdx.x;
  int lo = T - 1;
  for (int b = tid; b < B; b += 256) {
    int a = T - 1;
    if (!active || active[b]) {
      a = 0;
      while (a < T - 1 && block_ids[(long)b * T + a + 1] == greedy[(long)b * T + a]) ++a;
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
  for (int b = tid; b < B; b += 256) next[b] = greedy[(long)b * T + lo];
}

extern "C" void lia_verify_argmax_rows_launch(const bf16_t* logits, long ld, int n, int vocab, int suppress, int n_suppress,
                                              const int* n_suppress_rows, int T, int r0, int64_t* greedy, hipStream_t st) {
  if (n <= 0) return;
  const int vec = (ld % 8 == 0) && (vocab % 8 == 0) && (((uintptr_t)logits & 15) == 0);
  hipLaunchKernelGGL(lia_verify_argmax_kernel<0>, dim3(n), dim3(LIA_ROW_THREADS), 0, st, logits, ld, vocab, vec, suppress, n_suppress, T, r0, greedy,
                     n_suppress_rows, (const uint32_t*)nullptr, 0L);
}

// mask: device, block row r0 + i of the chunk at mask + (r0 + i) * ldm words (ldm >= ceil(vocab / 32), or 0: one row for every row)
extern "C" void lia_verify_argmax_masked_launch(const bf16_t* logits, long ld, int n, int vocab, int suppress, int n_suppress,
                                                const int* n_suppress_rows, int T, int r0, int64_t* greedy, const uint32_t* mask, long ldm,
                                                hipStream_t st) {
  if (n <= 0) return;
  const int vec = (ld % 8 == 0) && (vocab % 8 == 0) && (((uintptr_t)logits & 15) == 0);
  hipLaunchKernelGGL(lia_verify_argmax_kernel<1>, dim3(n), dim3(LIA_ROW_THREADS), 0, st, logits, ld, vocab, vec, suppress, n_suppress, T, r0, greedy,
                     n_suppress_rows, mask, ldm);
}

extern "C" void lia_verify_argmax_launch(const bf16_t* logits, long ld, int n, int vocab, int suppress, int n_suppress, int T, int r0,
                                         int64_t* greedy, hipStream_t st) {
  lia_verify_argmax_rows_launch(logits, ld, n, vocab, suppress, n_suppress, nullptr, T, r0, greedy, st);
}

extern "C" void lia_verify_accept_launch(const int64_t* block_ids, const int64_t* greedy, const int* active, int B, int T, int* accepted,
                                         int* common, int64_t* next, hipStream_t st) {
  if (B <= 0) return;
  hipLaunchKernelGGL(lia_verify_accept_kernel, dim3(1), dim3(256), 0, st, block_ids, greedy, active, B, T, accepted, common, next);
}
