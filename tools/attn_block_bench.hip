// Timing of the block attention kernel (csrc/lia_attention.hip, lia_attn_block_launch) on the verification block of speculative
// decoding -- T = 2 .. 8 queries per row at cache positions pos0 .. pos0 + T - 1 -- beside the launches that serve it otherwise:
//   (a) lia_attn_block_launch over (pos0, T): the decode kernel for G * T query slots, K / V read once;
//   (b) lia_attn_append_launch over (pos0, T): the prefill tile form, 128-query blocks, two sweeps of K / V;
//   (c) ONE lia_attn_decode_launch over pos0 + T keys (what a single decode step costs at that length: the yardstick);
//   (d) T launches of lia_attn_decode_launch, query t over pos0 + t + 1 keys: (a)'s rows must equal them bit for bit.
// Shapes: OPT-30B's attention (56 / 56 heads, d 128) at B 1 / 4 / 64, pos0 288 / 2048, T 2 / 3 / 5 / 8; Llama-3-8B's (32 / 8 heads,
// POST_SCALE) at B 1 / 128, pos0 1024, T 2 / 4.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-honor-nans -I isca-2025-lia_amd/csrc -I include tools/attn_block_bench.hip -o tools/attn_block_bench
//   tools/attn_block_bench [reps]
// (a) (b) (c) run interleaved (a b c a b c ...), each bracketed by its own event pair; the median of `reps` is printed.
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
  const size_t nkv = (size_t)S * Bc * KD, nb = (size_t)B * T * H;
  std::vector<bf16_t> hk(nkv), hv(nkv), hqb(nb);
  for (auto& x : hqb) x = rnd_bf16(2.0f);
  for (auto& x : hk) x = rnd_bf16(2.0f);
  for (auto& x : hv) x = rnd_bf16(1.0f);
  bf16_t *qb, *k, *v, *o_blk, *o_app, *o_dec, *o_one;
  CK(hipMalloc(&qb, nb * 2)); CK(hipMalloc(&k, nkv * 2)); CK(hipMalloc(&v, nkv * 2));
  CK(hipMalloc(&o_blk, nb * 2)); CK(hipMalloc(&o_app, nb * 2)); CK(hipMalloc(&o_dec, nb * 2)); CK(hipMalloc(&o_one, nb * 2));
  CK(hipMemset(o_blk, 0xff, nb * 2)); CK(hipMemset(o_app, 0xff, nb * 2)); CK(hipMemset(o_dec, 0xff, nb * 2));
  CK(hipMemcpy(qb, hqb.data(), nb * 2, hipMemcpyHostToDevice));
  CK(hipMemcpy(k, hk.data(), nkv * 2, hipMemcpyHostToDevice)); CK(hipMemcpy(v, hv.data(), nkv * 2, hipMemcpyHostToDevice));
  hipStream_t st; CK(hipStreamCreate(&st));
  std::vector<hipEvent_t> ev(2 * 3 * (reps + 2));
  for (auto& e : ev) CK(hipEventCreate(&e));
  auto launch = [&](int which) {
    int rc = 0;
    if (which == 0) rc = lia_attn_block_launch(qb, H, k, v, o_blk, H, B, T, pos0, heads, kvh, d, Bc, 0, post_scale, nullptr, st);
    else if (which == 1) rc = lia_attn_append_launch(qb, H, k, v, o_app, H, B, T, pos0, heads, kvh, d, Bc, 0, post_scale, nullptr, st);
    else if (which == 2) rc = lia_attn_decode_launch(qb + (size_t)(T - 1) * H, (long)T * H, k, v, o_one, (long)T * H, B, S, heads, kvh, d, Bc, 0, post_scale, st);
    else
      for (int t = 0; t < T && !rc; ++t)
        rc = lia_attn_decode_launch(qb + (size_t)t * H, (long)T * H, k, v, o_dec + (size_t)t * H, (long)T * H, B, pos0 + t + 1, heads, kvh, d, Bc, 0, post_scale, st);
    if (rc) { printf("%s B %d pos0 %d T %d: launch %d rc %d\n", name, B, pos0, T, which, rc); exit(1); }
  };
  launch(3);
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
  std::vector<bf16_t> ra(nb), rd(nb);
  CK(hipMemcpy(ra.data(), o_blk, nb * 2, hipMemcpyDeviceToHost)); CK(hipMemcpy(rd.data(), o_dec, nb * 2, hipMemcpyDeviceToHost));
  size_t diff = 0;
  for (size_t i = 0; i < nb; ++i) diff += ra[i] != rd[i];
  const double a = median(t[0]), p = median(t[1]), c = median(t[2]);
  const double sweep_bytes = 2.0 * B * S * KD * 2;            // K and V once
  printf("%-11s B %3d pos0 %4d T %d heads %2d/%2d slots %2d: (a) block %7.1f us   (b) append %7.1f us (%.2f x)   (c) one decode launch %7.1f us "
         "(%.2f x)   (a): %.0f MB, %.1f %% of 8 TB/s   (a) vs T decode launches: differing outputs %zu%s\n",
         name, B, pos0, T, heads, kvh, heads / kvh * T, a, p, p / a, c, c / a, sweep_bytes / 1e6, 100.0 * sweep_bytes / (a * 1e-6) / 8e12, diff,
         diff ? "   <-- MISMATCH" : "");
  for (auto& e : ev) CK(hipEventDestroy(e));
  CK(hipFree(qb)); CK(hipFree(k)); CK(hipFree(v)); CK(hipFree(o_blk)); CK(hipFree(o_app)); CK(hipFree(o_dec)); CK(hipFree(o_one));
  CK(hipStreamDestroy(st));
}

int main(int argc, char** argv) {
  const int reps = argc > 1 ? atoi(argv[1]) : 20;
  for (int B : {1, 4, 64})
    for (int pos0 : {288, 2048})
      for (int T : {2, 3, 5, 8}) run_case("OPT-30B", B, pos0, T, 56, 56, 0, reps);
  for (int B : {1, 128})
    for (int T : {2, 4}) run_case("Llama-3-8B", B, 1024, T, 32, 8, 1, reps);
  return 0;
}
