// Timing of the scoring row kernel (csrc/lia_score.hip) alone at M = 4096 rows of OPT's (50272) and Llama-3's (128256) vocabulary:
//   (a) lia_token_logprobs_kernel: max + first index, then sum exp(l - m) over the row the first pass left in L2;
//   (b) lia_argmax_kernel: one pass, no exp -- what reading the rows costs in this launch shape;
//   (c) an ONLINE variant kept in this file only: one pass, a running (m, s) pair per lane, rescaled at every new maximum.
// Bytes = M x vocab x 2 (the logits once); the rate is set against the 8 TB/s HBM peak DESIGN.md section 5 uses.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I isca-2025-lia_amd/csrc -I include tools/score_row_bench.hip -o tools/score_row_bench
//   tools/score_row_bench [reps]
// The cases run interleaved (a b c a b c ...), each launch bracketed by its own event pair; the median of `reps` is printed.
#include "../isca-2025-lia_amd/csrc/lia_score.hip"
#include "../isca-2025-lia_amd/csrc/lia_elementwise.hip"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

__global__ __launch_bounds__(LIA_ROW_THREADS) void online_logprobs_kernel(const bf16_t* __restrict__ logits, long ld, int vocab,
                                                                          const int64_t* __restrict__ targets, float* __restrict__ logprobs) {
  __shared__ float sm[LIA_ROW_WAVES], ss[LIA_ROW_WAVES];
  const int tid = threadIdx.x, lane = tid & 63;
  const bf16_t* row = logits + (long)blockIdx.x * ld;
  float m = -INFINITY, s = 0.f;
  for (int i = tid * 8; i < vocab; i += LIA_ROW_THREADS * 8) {      // (vocab % 8 == 0 here)
    float f[8];
    load_logits8(row, i, vocab, true, f);
    float vm = f[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) vm = fmaxf(vm, f[e]);
    if (vm > m) { s *= expf(m - vm); m = vm; }
#pragma unroll
    for (int e = 0; e < 8; ++e) s += expf(f[e] - m);
  }
  const float wm = wave_max(m);
  s = wave_sum(s * expf(m - wm));
  if (lane == 0) { sm[tid >> 6] = wm; ss[tid >> 6] = s; }
  __syncthreads();
  if (tid == 0) {
    float M = sm[0];
    for (int w = 1; w < LIA_ROW_WAVES; ++w) M = fmaxf(M, sm[w]);
    float S = 0.f;
    for (int w = 0; w < LIA_ROW_WAVES; ++w) S += ss[w] * expf(sm[w] - M);
    logprobs[blockIdx.x] = bf2f(row[targets[blockIdx.x]]) - (M + logf(S));
  }
}

static uint32_t rng_state = 12345;
static inline uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state; }
static inline bf16_t rnd_bf16(float scale) {
  float f = ((int)(rnd() >> 8) - (1 << 23)) * (scale / (1 << 23));
  uint32_t u; memcpy(&u, &f, 4);
  u += 0x7fff + ((u >> 16) & 1);
  return (bf16_t)(u >> 16);
}
static double median(std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

static void run_case(int M, int vocab, int reps) {
  const size_t n = (size_t)M * vocab;
  std::vector<bf16_t> h(n);
  for (auto& x : h) x = rnd_bf16(6.0f);
  std::vector<int64_t> ht(M);
  for (auto& t : ht) t = rnd() % (unsigned)vocab;
  bf16_t* lg; int64_t *tg, *gr, *am; float *lp, *lpo;
  CK(hipMalloc(&lg, n * 2)); CK(hipMalloc(&tg, M * 8)); CK(hipMalloc(&gr, M * 8)); CK(hipMalloc(&am, M * 8));
  CK(hipMalloc(&lp, M * 4)); CK(hipMalloc(&lpo, M * 4));
  CK(hipMemcpy(lg, h.data(), n * 2, hipMemcpyHostToDevice)); CK(hipMemcpy(tg, ht.data(), M * 8, hipMemcpyHostToDevice));
  hipStream_t st; CK(hipStreamCreate(&st));
  std::vector<hipEvent_t> ev(2 * 3 * (reps + 2));
  for (auto& e : ev) CK(hipEventCreate(&e));
  int ei = 0;
  for (int it = 0; it < reps + 2; ++it)
    for (int which = 0; which < 3; ++which) {
      CK(hipEventRecord(ev[ei++], st));
      if (which == 0) lia_token_logprobs_launch(lg, vocab, M, vocab, tg, lp, gr, st);
      else if (which == 1) lia_argmax_launch(lg, am, M, vocab, -1, st);
      else hipLaunchKernelGGL(online_logprobs_kernel, dim3(M), dim3(LIA_ROW_THREADS), 0, st, lg, (long)vocab, vocab, tg, lpo);
      CK(hipEventRecord(ev[ei++], st));
    }
  CK(hipStreamSynchronize(st));
  CK(hipGetLastError());
  std::vector<float> t[3];
  ei = 0;
  for (int it = 0; it < reps + 2; ++it)
    for (int which = 0; which < 3; ++which) {
      float ms = 0;
      CK(hipEventElapsedTime(&ms, ev[ei], ev[ei + 1]));
      ei += 2;
      if (it >= 2) t[which].push_back(1e3f * ms);
    }
  std::vector<float> a(M), c(M);
  std::vector<int64_t> g(M), g2(M);
  CK(hipMemcpy(a.data(), lp, M * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(c.data(), lpo, M * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(g.data(), gr, M * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(g2.data(), am, M * 8, hipMemcpyDeviceToHost));
  double dmax = 0;
  size_t gdiff = 0;
  for (int r = 0; r < M; ++r) { dmax = std::max(dmax, (double)fabsf(a[r] - c[r])); gdiff += g[r] != g2[r]; }
  const double bytes = 2.0 * n;
  const char* names[3] = {"(a) two-pass logprobs", "(b) argmax (one pass, no exp)", "(c) online one-pass logprobs"};
  for (int w = 0; w < 3; ++w) {
    const double us = median(t[w]);
    printf("M %d vocab %6d  %-32s %8.1f us  %6.2f TB/s of logits = %.2f of 8 TB/s\n", M, vocab, names[w], us, bytes / us / 1e6, bytes / us / 1e6 / 8.0);
  }
  printf("M %d vocab %6d  greedy ids differing from argmax: %zu;  max |two-pass - online| logprob %.3g\n", M, vocab, gdiff, dmax);
  for (auto& e : ev) CK(hipEventDestroy(e));
  CK(hipFree(lg)); CK(hipFree(tg)); CK(hipFree(gr)); CK(hipFree(am)); CK(hipFree(lp)); CK(hipFree(lpo));
  CK(hipStreamDestroy(st));
}

int main(int argc, char** argv) {
  const int reps = argc > 1 ? atoi(argv[1]) : 20;
  run_case(4096, 50272, reps);
  run_case(4096, 128256, reps);
  return 0;
}
