// Timing of the append attention kernels (csrc/lia_attention.hip, lia_attn_append_launch): a block of T queries at cache positions
// pos0 .. pos0 + T - 1 over S = pos0 + T cached keys, beside the two things a build without them has to do instead:
//   (a) lia_attn_append_launch over (pos0, T);
//   (b) lia_attn_prefill_launch over all S = pos0 + T tokens (the re-prefill; its rows pos0 .. must equal (a) bit for bit);
//   (c) T launches of lia_attn_decode_launch, query t over pos0 + t + 1 keys (the sum of the T launches is reported).
// Shapes: OPT-30B's attention (56 heads, d 128) B 64 pos0 256 T 2 / 17 / 128; Llama-3-8B's (32 / 8 heads, POST_SCALE) B 128 pos0 1024 T 33.
// "HBM" = the share of 8 TB/s that reading K and V once per sweep implies for (a): 2 sweeps x 2 B S H_kv d 2 bytes over the time.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-honor-nans -I isca-2025-lia_amd/csrc -I include tools/attn_append_bench.hip -o tools/attn_append_bench
//   tools/attn_append_bench [reps]           (kernel times: rocprofv3 --kernel-trace --stats -- tools/attn_append_bench 5, a run of its own)
// The three routes run interleaved (a b c a b c ...), each bracketed by its own event pair; the median of `reps` is printed.
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

static void run_case(const char* name, int B, int pos0, int T, int heads, int kvh, int post_scale, int reps) {
  const int d = 128, H = heads * d, KD = kvh * d, Bc = B, S = pos0 + T;
  const size_t nq = (size_t)B * S * H, nkv = (size_t)S * Bc * KD, nb = (size_t)B * T * H;
  std::vector<bf16_t> hq(nq), hk(nkv), hv(nkv), hqb(nb);
  for (auto& x : hq) x = rnd_bf16(2.0f);
  for (auto& x : hk) x = rnd_bf16(2.0f);
  for (auto& x : hv) x = rnd_bf16(1.0f);
  for (int b = 0; b < B; ++b)      // the block's q rows: rows pos0 .. of the full sequence
    memcpy(&hqb[(size_t)b * T * H], &hq[((size_t)b * S + pos0) * H], (size_t)T * H * 2);
  bf16_t *q, *qb, *k, *v, *o_full, *o_app, *o_dec;
  CK(hipMalloc(&q, nq * 2)); CK(hipMalloc(&qb, nb * 2)); CK(hipMalloc(&k, nkv * 2)); CK(hipMalloc(&v, nkv * 2));
  CK(hipMalloc(&o_full, nq * 2)); CK(hipMalloc(&o_app, nb * 2)); CK(hipMalloc(&o_dec, nb * 2));
  CK(hipMemset(o_full, 0xff, nq * 2)); CK(hipMemset(o_app, 0xff, nb * 2)); CK(hipMemset(o_dec, 0xff, nb * 2));
  CK(hipMemcpy(q, hq.data(), nq * 2, hipMemcpyHostToDevice)); CK(hipMemcpy(qb, hqb.data(), nb * 2, hipMemcpyHostToDevice));
  CK(hipMemcpy(k, hk.data(), nkv * 2, hipMemcpyHostToDevice)); CK(hipMemcpy(v, hv.data(), nkv * 2, hipMemcpyHostToDevice));
  hipStream_t st; CK(hipStreamCreate(&st));
  std::vector<hipEvent_t> ev(2 * 3 * (reps + 2));
  for (auto& e : ev) CK(hipEventCreate(&e));
  auto launch = [&](int which) {
    int rc = 0;
    if (which == 0) rc = lia_attn_append_launch(qb, H, k, v, o_app, H, B, T, pos0, heads, kvh, d, Bc, 0, post_scale, nullptr, st);
    else if (which == 1) rc = lia_attn_prefill_launch(q, H, k, v, o_full, H, B, S, heads, kvh, d, Bc, 0, post_scale, st);
    else
      for (int t = 0; t < T && !rc; ++t)
        rc = lia_attn_decode_launch(qb + (size_t)t * H, (long)T * H, k, v, o_dec + (size_t)t * H, (long)T * H, B, pos0 + t + 1, heads, kvh, d, Bc, 0, post_scale, st);
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
  std::vector<bf16_t> ra(nb), rf(nq);
  CK(hipMemcpy(ra.data(), o_app, nb * 2, hipMemcpyDeviceToHost)); CK(hipMemcpy(rf.data(), o_full, nq * 2, hipMemcpyDeviceToHost));
  size_t diff = 0;
  for (int b = 0; b < B; ++b)
    for (size_t i = 0; i < (size_t)T * H; ++i) diff += ra[(size_t)b * T * H + i] != rf[((size_t)b * S + pos0) * H + i];
  const double a = median(t[0]), p = median(t[1]), c = median(t[2]);
  const double sweep_bytes = 2.0 * B * S * KD * 2;            // K and V once
  printf("%-12s B %3d pos0 %4d T %3d heads %2d/%2d: (a) append %8.1f us   (b) prefill over %4d %8.1f us (%.2f x)   (c) %3d decode launches "
         "%8.1f us (%.2f x)   (a): %.0f MB per sweep, %.1f %% of 8 TB/s over two sweeps   (a) vs (b) differing outputs %zu%s\n",
         name, B, pos0, T, heads, kvh, a, S, p, p / a, T, c, c / a, sweep_bytes / 1e6, 100.0 * 2 * sweep_bytes / (a * 1e-6) / 8e12, diff,
         diff ? "   <-- MISMATCH" : "");
  for (auto& e : ev) CK(hipEventDestroy(e));
  CK(hipFree(q)); CK(hipFree(qb)); CK(hipFree(k)); CK(hipFree(v)); CK(hipFree(o_full)); CK(hipFree(o_app)); CK(hipFree(o_dec));
  CK(hipStreamDestroy(st));
}

int main(int argc, char** argv) {
  const int reps = argc > 1 ? atoi(argv[1]) : 20;
  for (int T : {2, 17, 128}) run_case("OPT-30B", 64, 256, T, 56, 56, 0, reps);
  run_case("Llama-3-8B", 128, 1024, 33, 32, 8, 1, reps);
  return 0;
}
