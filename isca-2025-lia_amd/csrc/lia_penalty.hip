// Repetition, presence and frequency penalties: the one piece of per-row decoding state that lives on the device.
//
// A row's state is its COUNT ROW, one uint16 word per token of the vocabulary:
//   bit 15     the token occurs in the prompt
//   bits 0..14 n, the number of times the token was generated in this generate() call, saturating at 32767
// lia_token_counts_kernel adds ids to the table (two words share a 32-bit location: 32-bit atomics on the containing word, the
// neighbouring word keeps its bits).  lia_penalty_kernel rewrites logits under the table, in fp32, every operation rounded on its own:
//   x = fp32(l);  if (c != 0) x = x < 0 ? x * theta : x / theta;  x = x - alpha_f * float(n);  x = x - (n > 0 ? alpha_p : 0);  bf16(x)
// (HF's RepetitionPenaltyLogitsProcessor on prompt and generated tokens, then OpenAI's / vLLM's frequency and presence penalties on
// the generated ones).  The result is rounded back to bf16 on purpose: the head kernels that read it order a row by its bf16 keys.
// +-inf stay +-inf (theta > 0); NaN logits and fp32-subnormal intermediates are not defined.
#include "lia_internal.h"

#define LIA_PEN_THREADS 256
#define LIA_PEN_TILE (LIA_PEN_THREADS * 8)   // columns per workgroup: 8 logits (one 16-byte load) per thread

__device__ __forceinline__ bf16_t lia_penalise(bf16_t l, uint32_t c, float theta, float alpha_p, float alpha_f) {
#pragma clang fp contract(off)   // (hipcc contracts a * b - c into an FMA by default: one rounding where the semantics name two)
  float x = bf2f(l);
  if (c != 0) x = x < 0.f ? x * theta : x / theta;
  const uint32_t n = c & 0x7fffu;
  const float f = alpha_f * (float)n;
  x = x - f;
  x = x - (n > 0 ? alpha_p : 0.f);
  return f2bf(x);
}

// Elementwise and memory-bound (2 + 2 bytes read, 2 written per token): a 2-D grid over (column tile, row).  VEC: 16-byte loads of 8
// logits and 8 count words and one 16-byte store per thread where a whole group of 8 lies inside the row -- the launcher grants it
// when the three bases are 16-byte aligned and the three pitches multiples of 8; the last vocab % 8 columns, and everything without
// VEC, go one element at a time.  out may be logits (in place): a thread reads its elements before it writes them, and no other
// thread touches them -- hence no __restrict__ on the two.
template <int VEC>
__global__ __launch_bounds__(LIA_PEN_THREADS) void lia_penalty_kernel(const bf16_t* logits, long ld, int M, int vocab,
                                                                      const uint16_t* __restrict__ counts, long ldc, float theta,
                                                                      float alpha_p, float alpha_f, bf16_t* out, long ldo) {
  const int i = ((int)blockIdx.x * LIA_PEN_THREADS + (int)threadIdx.x) * 8;
  if (i >= vocab) return;
  for (long r = blockIdx.y; r < M; r += gridDim.y) {        // (the grid's row dimension ends at 65535: more rows go round)
    const bf16_t* lrow = logits + r * ld;
    const uint16_t* crow = counts + r * ldc;
    bf16_t* orow = out + r * ldo;
    if (VEC && i + 8 <= vocab) {
      const uint4 lv = *(const uint4*)(lrow + i);
      const uint4 cv = *(const uint4*)(crow + i);
      const uint32_t lw[4] = {lv.x, lv.y, lv.z, lv.w}, cw[4] = {cv.x, cv.y, cv.z, cv.w};
      uint32_t o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16_t lo = lia_penalise((bf16_t)(lw[j] & 0xffff), cw[j] & 0xffff, theta, alpha_p, alpha_f);
        const bf16_t hi = lia_penalise((bf16_t)(lw[j] >> 16), cw[j] >> 16, theta, alpha_p, alpha_f);
        o[j] = (uint32_t)lo | ((uint32_t)hi << 16);
      }
      *(uint4*)(orow + i) = uint4{o[0], o[1], o[2], o[3]};
    } else {
      const int end = i + 8 < vocab ? i + 8 : vocab;
      for (int e = i; e < end; ++e) orow[e] = lia_penalise(lrow[e], crow[e], theta, alpha_p, alpha_f);
    }
  }
}

// logits [M, ld], counts [M, ldc], out [M, ldo]; ld, ldc, ldo >= vocab (the callers check); out == logits allowed
extern "C" void lia_penalty_launch(const bf16_t* logits, long ld, int M, int vocab, const uint16_t* counts, long ldc, float theta,
                                   float alpha_p, float alpha_f, bf16_t* out, long ldo, hipStream_t st) {
  if (M <= 0 || vocab <= 0) return;
  const bool vec = (((uintptr_t)logits | (uintptr_t)counts | (uintptr_t)out) & 15) == 0 && ld % 8 == 0 && ldc % 8 == 0 && ldo % 8 == 0;
  const dim3 grid((unsigned)((vocab + LIA_PEN_TILE - 1) / LIA_PEN_TILE), (unsigned)(M < 65535 ? M : 65535));
  if (vec)
    hipLaunchKernelGGL(lia_penalty_kernel<1>, grid, dim3(LIA_PEN_THREADS), 0, st, logits, ld, M, vocab, counts, ldc, theta, alpha_p, alpha_f, out, ldo);
  else
    hipLaunchKernelGGL(lia_penalty_kernel<0>, grid, dim3(LIA_PEN_THREADS), 0, st, logits, ld, M, vocab, counts, ldc, theta, alpha_p, alpha_f, out, ldo);
}

// One thread per id of ids [B, n] (pitch ldi).  Position t of row b is skipped when t < first[b] (first: int32 [B] or NULL -- left
// padding) or active[b] == 0 (active: int32 [B] or NULL -- finished rows); an id outside [0, vocab) is ignored.  generated = 0: bit 15
// of the token's word is set (atomicOr); generated = 1: its low 15 bits grow by one unless they hold 32767 (a compare-and-swap loop
// on the 32-bit location: the add can never carry into bit 15, and the other half of the location is written back as it was read
// in the same exchange).  The table base is 4-byte aligned and ldc even, so word (b, id) sits in half id & 1 of its location.
__global__ __launch_bounds__(256) void lia_token_counts_kernel(uint16_t* __restrict__ counts, long ldc, int vocab,
                                                               const int64_t* __restrict__ ids, long ldi, int n, long total,
                                                               const int* __restrict__ first, const int* __restrict__ active,
                                                               int generated) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const long b = g / n;
  const int t = (int)(g - b * n);
  if (first && t < first[b]) return;
  if (active && active[b] == 0) return;
  const int64_t id = ids[b * ldi + t];
  if (id < 0 || id >= vocab) return;
  const long word = b * ldc + id;
  uint32_t* p = (uint32_t*)counts + (word >> 1);
  const int shift = (int)(word & 1) * 16;
  if (!generated) {
    atomicOr(p, 0x8000u << shift);
    return;
  }
  uint32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
  while (true) {
    if (((old >> shift) & 0x7fffu) == 0x7fffu) return;       // saturated
    const uint32_t seen = atomicCAS(p, old, old + (1u << shift));
    if (seen == old) return;
    old = seen;
  }
}

// counts [rows >= B, ldc], ids [B, n] (pitch ldi >= n); the callers check the table (4-byte aligned, ldc even and >= vocab)
extern "C" void lia_token_counts_launch(uint16_t* counts, long ldc, int B, int vocab, const int64_t* ids, long ldi, int n, const int* first,
                                        const int* active, int generated, hipStream_t st) {
  const long total = (long)B * n;
  if (B <= 0 || n <= 0) return;
  hipLaunchKernelGGL(lia_token_counts_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, counts, ldc, vocab, ids, ldi, n, total,
                     first, active, generated);
}
