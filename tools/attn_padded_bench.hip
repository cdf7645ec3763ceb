// Timing of the left-padded attention kernels (csrc/lia_attention.hip, PADDED instantiations) at OPT-30B's attention shape
// (56 heads, d 128), against the unpadded kernels on the same inputs:
//   (a) the unpadded launcher;  (b) the padded launcher with every start 0 (must equal (a) bit for bit);
//   (c) the padded launcher with starts uniform in [0, T/2) -- "work" is the share of (a)'s q.k products left (prefill: causal
//       pairs of the row's T - s tokens; decode: keys S - s).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-honor-nans -I isca-2025-lia_amd/csrc -I include tools/attn_padded_bench.hip -o tools/attn_padded_bench
//   tools/attn_padded_bench [reps]
// The three cases run interleaved (a b c a b c ...), each launch bracketed by its own event pair; the median of `reps` is printed.
#include "../isca-2025-lia_amd/csrc/lia_attention.hip"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

static uint32_t rng_state = 12345;
static inline uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state; }
static inline bf16_t rnd_bf16(float scale) {
  float f = ((int)(rnd() >> 8) - (1 << 23)) * (scale / (1 << 23));
  uint32_t u; memcpy(&u, &f, 4);
  u += 0x7fff + ((u >> 16) & 1);
  return (bf16_t)(u >> 16);
}

static double median(std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

// T > 1: prefill over T tokens; T == 1: decode of one query per row over S keys (prompt of P tokens: starts < P / 2)
static void run_case(const char* name, int B, int T, int S, int P, int reps) {
  const int heads = 56, d = 128, H = heads * d, Bc = B;
  const size_t nq = (size_t)B * T * H, nkv = (size_t)S * Bc * H;
  std::vector<bf16_t> hq(nq), hk(nkv), hv(nkv);
  for (auto& x : hq) x = rnd_bf16(2.0f);
  for (auto& x : hk) x = rnd_bf16(2.0f);
  for (auto& x : hv) x = rnd_bf16(1.0f);
  std::vector<int> zero(B, 0), spread(B);
  double work_a = 0, work_c = 0;
  for (int b = 0; b < B; ++b) {
    spread[b] = (int)(rnd() % (unsigned)(P / 2));
    const double n = T > 1 ? (double)(T - spread[b]) : (double)(S - spread[b]);
    work_a += T > 1 ? (double)T * (T + 1) / 2 : (double)S;
    work_c += T > 1 ? n * (n + 1) / 2 : n;
  }
  bf16_t *q, *k, *v, *o[3];
  int *st0, *st1;
  CK(hipMalloc(&q, nq * 2)); CK(hipMalloc(&k, nkv * 2)); CK(hipMalloc(&v, nkv * 2));
  for (int i = 0; i < 3; ++i) { CK(hipMalloc(&o[i], nq * 2)); CK(hipMemset(o[i], 0xff, nq * 2)); }
  CK(hipMalloc(&st0, B * sizeof(int))); CK(hipMalloc(&st1, B * sizeof(int)));
  CK(hipMemcpy(q, hq.data(), nq * 2, hipMemcpyHostToDevice)); CK(hipMemcpy(k, hk.data(), nkv * 2, hipMemcpyHostToDevice));
  CK(hipMemcpy(v, hv.data(), nkv * 2, hipMemcpyHostToDevice));
  CK(hipMemcpy(st0, zero.data(), B * sizeof(int), hipMemcpyHostToDevice)); CK(hipMemcpy(st1, spread.data(), B * sizeof(int), hipMemcpyHostToDevice));
  hipStream_t st; CK(hipStreamCreate(&st));
  std::vector<hipEvent_t> ev(2 * 3 * (reps + 2));
  for (auto& e : ev) CK(hipEventCreate(&e));
  auto launch = [&](int which) {
    int rc;
    if (T > 1) rc = which == 0 ? lia_attn_prefill_launch(q, H, k, v, o[0], H, B, T, heads, heads, d, Bc, 0, 0, st)
                               : lia_attn_prefill_padded_launch(q, H, k, v, o[which], H, B, T, heads, heads, d, Bc, 0, 0, which == 1 ? st0 : st1, st);
    else rc = which == 0 ? lia_attn_decode_launch(q, H, k, v, o[0], H, B, S, heads, heads, d, Bc, 0, 0, st)
                         : lia_attn_decode_padded_launch(q, H, k, v, o[which], H, B, S, heads, heads, d, Bc, 0, 0, which == 1 ? st0 : st1, st);
    if (rc) { printf("launch rc %d\n", rc); exit(1); }
  };
  int ei = 0;
  for (int it = 0; it < reps + 2; ++it)
    for (int which = 0; which < 3; ++which) {
      CK(hipEventRecord(ev[ei++], st));
      launch(which);
      CK(hipEventRecord(ev[ei++], st));
    }
  CK(hipStreamSynchronize(st));
  std::vector<float> t[3];
  ei = 0;
  for (int it = 0; it < reps + 2; ++it)
    for (int which = 0; which < 3; ++which) {
      float ms = 0;
      CK(hipEventElapsedTime(&ms, ev[ei], ev[ei + 1]));
      ei += 2;
      if (it >= 2) t[which].push_back(1e3f * ms);
    }
  std::vector<bf16_t> r0(nq), r1(nq);
  CK(hipMemcpy(r0.data(), o[0], nq * 2, hipMemcpyDeviceToHost)); CK(hipMemcpy(r1.data(), o[1], nq * 2, hipMemcpyDeviceToHost));
  size_t diff = 0;
  for (size_t i = 0; i < nq; ++i) diff += r0[i] != r1[i];
  const double a = median(t[0]), b = median(t[1]), c = median(t[2]);
  printf("%-34s B %2d T %4d S %4d: (a) unpadded %8.1f us   (b) padded, starts 0 %8.1f us (%+.1f %%)   (c) padded, starts in [0, %d) "
         "%8.1f us (%.2f of a; work left %.2f)   (b) vs (a) differing outputs %zu%s\n",
         name, B, T, S, a, b, 100.0 * (b - a) / a, P / 2, c, c / a, work_c / work_a, diff, diff ? "   <-- MISMATCH" : "");
  for (auto& e : ev) CK(hipEventDestroy(e));
  CK(hipFree(q)); CK(hipFree(k)); CK(hipFree(v)); CK(hipFree(st0)); CK(hipFree(st1));
  for (int i = 0; i < 3; ++i) CK(hipFree(o[i]));
  CK(hipStreamDestroy(st));
}

int main(int argc, char** argv) {
  const int reps = argc > 1 ? atoi(argv[1]) : 30;
  run_case("OPT-30B prefill attention", 8, 256, 256, 256, reps);
  run_case("OPT-30B prefill attention", 8, 2016, 2016, 2016, reps > 10 ? 10 : reps);
  run_case("OPT-30B decode attention", 64, 1, 288, 256, reps);
  return 0;
}
