// Timing of the split-key decode attention (csrc/lia_attention.hip, lia_attn_decode_split_launch) beside the one-workgroup launch:
//   (a) lia_attn_decode_launch: one workgroup per (batch row, KV head) -- the kernel this change does not touch, so leg (a) of
//       this binary IS the parent's kernel; "refused" where its scores do not fit the LDS;
//   (b) lia_attn_decode_split_launch_chunk at C = 256 / 512 / 1024 keys per chunk (the multiples of the kernel's pass at this d):
//       scores, softmax, P.V and combine launches, one workgroup per (chunk, KV head, row).
// Shapes: OPT-30B's attention (56 / 56 heads, d 128) at B 1 / 4, S 288 / 1024 / 2047; Llama-3-8B's (32 / 8 heads, POST_SCALE) at
// B 1 / 4 / 16, S 1030 / 4096 / 8191; S 16384 for the split route alone; and, for the choice of C at the other head dims only, the
// Llama head layout at d 64 / 32 (B 1 / 4, S 4096 / 8191; C 256 is no multiple of the d 32 pass and is skipped there).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-honor-nans -I isca-2025-lia_amd/csrc -I include tools/attn_split_bench.hip -o tools/attn_split_bench
//   tools/attn_split_bench [reps]
// The legs run interleaved (a b256 b512 b1024 a ...), each launch bracketed by its own event pair; per leg the median and the
// 10th / 90th percentile of `reps` are printed, and the achieved K + V bytes per second at the median.  A decode step reads every
// layer's own cache once, so launch i reads copy i % n of the K / V (n copies, > 600 MB together): no leg finds the rows the
// previous launch left in the L2 / MALL.  Every (b) is compared with (a): for S <= C the outputs must be bit-identical.
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

static double pct(std::vector<float> v, double p) { std::sort(v.begin(), v.end()); return v[(size_t)(p * (v.size() - 1) + 0.5)]; }

static void run_case(const char* name, int B, int S, int heads, int kvh, int d, int post_scale, int reps) {
  const int H = heads * d, KD = kvh * d, Bc = B;
  const size_t nkv = (size_t)S * Bc * KD, nq = (size_t)B * H;
  const int copies = (int)std::min<size_t>(64, std::max<size_t>(2, (600u << 20) / (nkv * 4) + 1));
  std::vector<bf16_t> hk(nkv), hv(nkv), hq(nq);
  for (auto& x : hq) x = rnd_bf16(2.0f);
  for (auto& x : hk) x = rnd_bf16(2.0f);
  for (auto& x : hv) x = rnd_bf16(1.0f);
  const int chunks[3] = {256, 512, 1024};
  bf16_t *q, *k, *v, *o[4];
  CK(hipMalloc(&q, nq * 2)); CK(hipMalloc(&k, nkv * 2 * copies)); CK(hipMalloc(&v, nkv * 2 * copies));
  for (auto& p : o) { CK(hipMalloc(&p, nq * 2)); CK(hipMemset(p, 0xff, nq * 2)); }
  CK(hipMemcpy(q, hq.data(), nq * 2, hipMemcpyHostToDevice));
  for (int c = 0; c < copies; ++c) {
    CK(hipMemcpy(k + c * nkv, hk.data(), nkv * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(v + c * nkv, hv.data(), nkv * 2, hipMemcpyHostToDevice));
  }
  size_t sbytes = 0;
  for (int C : chunks) sbytes = std::max(sbytes, lia_attn_split_scratch_bytes_chunk(B, S, heads, kvh, d, C));
  void* scratch;
  CK(hipMalloc(&scratch, sbytes));
  hipStream_t st; CK(hipStreamCreate(&st));
  const bool one_wg = lia_attn_split_route(0, S, heads, kvh, d) != 2;
  bool leg[4] = {true, true, true, true};
  for (int w = 1; w < 4; ++w) leg[w] = lia_attn_split_scratch_bytes_chunk(B, S, heads, kvh, d, chunks[w - 1]) != 0;
  std::vector<hipEvent_t> ev(2 * 4 * (reps + 2));
  for (auto& e : ev) CK(hipEventCreate(&e));
  int n_launch = 0;
  auto launch = [&](int which) {
    const size_t at = (size_t)(n_launch++ % copies) * nkv;
    int rc = 0;
    if (which == 0) { if (one_wg) rc = lia_attn_decode_launch(q, H, k + at, v + at, o[0], H, B, S, heads, kvh, d, Bc, 0, post_scale, st); }
    else if (leg[which]) rc = lia_attn_decode_split_launch_chunk(q, H, k + at, v + at, o[which], H, B, S, heads, kvh, d, Bc, 0, post_scale, nullptr, chunks[which - 1], scratch, sbytes, st);
    if (rc) { printf("%s B %d S %d: launch %d rc %d\n", name, B, S, which, rc); exit(1); }
  };
  int ei = 0;
  for (int it = 0; it < reps + 2; ++it)
    for (int which = 0; which < 4; ++which) {
      CK(hipEventRecord(ev[ei++], st));
      launch(which);
      CK(hipEventRecord(ev[ei++], st));
    }
  CK(hipStreamSynchronize(st));
  std::vector<float> t[4];
  ei = 0;
  for (int it = 0; it < reps + 2; ++it)
    for (int which = 0; which < 4; ++which) {
      float ms = 0;
      CK(hipEventElapsedTime(&ms, ev[ei], ev[ei + 1]));
      ei += 2;
      if (it >= 2) t[which].push_back(1e3f * ms);
    }
  const double bytes = 2.0 * B * S * KD * 2;            // K and V once
  printf("%-10s d %3d B %2d S %5d heads %2d/%2d  %6.1f MB K+V, %d copies:", name, d, B, S, heads, kvh, bytes / 1e6, copies);
  std::vector<bf16_t> ra(nq), rb(nq);
  double am = 0;
  if (one_wg) {
    am = pct(t[0], 0.5);
    CK(hipMemcpy(ra.data(), o[0], nq * 2, hipMemcpyDeviceToHost));
    printf("  (a) one workgroup %7.1f us [%.1f, %.1f] %5.2f TB/s", am, pct(t[0], 0.1), pct(t[0], 0.9), bytes / am / 1e6);
  } else {
    printf("  (a) one workgroup: refused (LDS)");
  }
  for (int w = 1; w < 4; ++w) {
    if (!leg[w]) continue;
    const double bm = pct(t[w], 0.5);
    printf("   (b) C %4d %7.1f us [%.1f, %.1f] %5.2f TB/s", chunks[w - 1], bm, pct(t[w], 0.1), pct(t[w], 0.9), bytes / bm / 1e6);
    if (one_wg) {
      CK(hipMemcpy(rb.data(), o[w], nq * 2, hipMemcpyDeviceToHost));
      size_t diff = 0;
      for (size_t i = 0; i < nq; ++i) diff += ra[i] != rb[i];
      printf(" (b)/(a) %.2f, %zu of %zu outputs differ%s", bm / am, diff, nq, diff && S <= chunks[w - 1] ? "   <-- MISMATCH (one chunk)" : "");
    }
  }
  printf("\n");
  for (auto& e : ev) CK(hipEventDestroy(e));
  CK(hipFree(q)); CK(hipFree(k)); CK(hipFree(v)); CK(hipFree(scratch));
  for (auto& p : o) CK(hipFree(p));
  CK(hipStreamDestroy(st));
}

int main(int argc, char** argv) {
  const int reps = argc > 1 ? atoi(argv[1]) : 30;
  for (int B : {1, 4})
    for (int S : {288, 1024, 2047}) run_case("OPT-30B", B, S, 56, 56, 128, 0, reps);
  for (int B : {1, 4, 16})
    for (int S : {1030, 4096, 8191, 16384}) run_case("Llama-3-8B", B, S, 32, 8, 128, 1, reps);
  for (int d : {64, 32})
    for (int B : {1, 4})
      for (int S : {4096, 8191}) run_case("GQA 32/8", B, S, 32, 8, d, 1, reps);
  return 0;
}
