// GPU attention for policies 0 / 3 (attentions.py:443-536), with every bf16 rounding point of the
// reference's op sequence kept:
//     q  = bf16(q * d^-0.5)            (:456)
//     s  = bf16(q . k)                 torch.bmm output (:499)
//     prefill: causal mask -> -inf     (:444-449, 500-509: fp32 add of -3.4028e38, clamp, cast to bf16)
//     p  = bf16(softmax(s))            fp32 inside (:512);  decode (T == 1): no mask
//     o  = bf16(p . v)                 torch.bmm output (:529)
// Because p is rounded AFTER normalisation by the full-row sum, a one-pass online softmax cannot
// reproduce it; the prefill kernel therefore makes two sweeps over the keys (statistics, then P.V).
// Attention is 0.3 % of the prefill flops at T = 256, so the second Q.K^T is
// irrelevant to the layer time while keeping bit-level agreement with the oracle.
//
// K and V are always read from the seq-major cache layout [S][Bc][h][d] (attentions.py:457-476) --
// the q|k|v GEMM epilogue has already scattered the fresh rows there -- so one kernel serves the
// resident layers (device cache) and the streamed prefill (staging slab that is then copied to the
// host cache).
#include <cstdlib>
#include "lia_internal.h"
#include <type_traits>

// ---------------------------------------------------------------------------------------------
// prefill: LDS-tiled, MFMA 32x32x16.  Workgroup = 4 waves = 128 query rows of one (batch, head);
// wave w owns query rows q0 + 32w .. +31.  Key tiles of 32 are staged in LDS and shared.
//   S^T = K . Qs^T   (A = K rows from LDS, B = Qs rows held in registers): the lane owns one query
//   column, so the softmax row statistics are in-lane + one cross-half shuffle.
//   O^T = V^T . P^T  (A = V^T from a transposed LDS image, B = the P^T accumulator registers re-used
//   directly as the next MFMA's operand, cdna_hip_programming.md section 3).
// ---------------------------------------------------------------------------------------------
// Left padding (PADDED = 1, every kernel below): served row b's tokens start at cache position kstart = starts[b]; its query i >= kstart
// sees keys kstart .. i.  That is the unpadded causal attention of a sequence of T - kstart tokens whose first sits at kstart, so the padded
// instantiations run the unpadded arithmetic on that shifted frame -- queries, keys and output rows offset by kstart, T - kstart tokens,
// key tiles aligned to kstart (every tile wholly before kstart is never visited, no key needs a lower mask) -- and write query rows
// 0 .. kstart - 1 as zeros without any K / V work.  A real row's result is bit for bit that of the same row unpadded.
// starts: per served row b (the caller passes its table + b0); PADDED = 0 never reads it
//
// Append (APPEND = 1): a block of Tq queries at cache positions pos0 .. pos0 + Tq - 1 over the keys kstart .. pos0 + Tq - 1 already in the
// cache.  The key frame starts at kstart as above, the query frame at pos0: query i of the block sits at frame position qoff + i,
// qoff = pos0 - kstart >= 0, and sees keys j <= qoff + i; q / out hold the block's rows only ([B][Tq], no pad query rows).  Key blocks
// stay aligned to kstart and a row's sums run over them in the same order with the same operations, and a block a row sees nothing of
// changes neither its maximum nor its sum nor its output (exp(-inf) = 0, P = 0) -- so a row's result is bit for bit that of the same
// row in a prefill over pos0 + Tq tokens.  APPEND = 0: qoff folds to 0 and Tq to the frame's T -- the code above, unchanged.
// One kernel template serves both: Pos0 is empty for the prefill (the kernel's parameters and code are then exactly those it had
// before the append block existed -- a wrapper around a shared body moved its SGPR allocation) and one int, pos0, for the append.
__device__ __forceinline__ int lia_pos0_of() { return 0; }
__device__ __forceinline__ int lia_pos0_of(int pos0) { return pos0; }
template <int D, int PADDED, typename... Pos0>
__global__ __launch_bounds__(256) void lia_attn_prefill_kernel(const bf16_t* __restrict__ q, long ldq, const bf16_t* __restrict__ kc,
                                                                const bf16_t* __restrict__ vc, bf16_t* __restrict__ out, long ldo, int Tp,
                                                                int heads, int kv_heads, int Bc, int b0, float scaling, int post_scale,
                                                                const int* __restrict__ starts, Pos0... pos0_arg) {
  constexpr int APPEND = sizeof...(Pos0);
  static_assert(APPEND <= 1, "Pos0: nothing (prefill) or pos0 (append)");
  const int pos0 = lia_pos0_of(pos0_arg...);
  constexpr int CH = D / 8;              // 16-byte chunks per K row
  constexpr int RPB = 16 / CH;           // K rows per 256-byte LDS bank row
  constexpr int KSTEPS = D / 16;         // MFMA k-steps over d for S^T
  constexpr int DB = D / 32;             // 32-row blocks of O^T
  constexpr int VT_STRIDE = 72;          // bytes per V^T row: 32 keys * 2 B + 8 pad (8-byte aligned)
  __shared__ __attribute__((aligned(16))) char k_lds[32 * D * 2];
  __shared__ __attribute__((aligned(16))) char vt_lds[D * VT_STRIDE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int hh = blockIdx.y, b = blockIdx.z;
  // Tp: the batch rows' pitch in q / out (tokens per row); T: the row's tokens from its start kstart on (the shifted frame, see above)
  const int kstart = PADDED ? __builtin_amdgcn_readfirstlane(starts[b]) : 0;   // (uniform: keeps the row start scalar)
  const int T = (APPEND ? pos0 + Tp : Tp) - kstart;               // keys of the frame
  const int Tq = APPEND ? Tp : T;                                // queries: the block's (append) or the frame's
  const int qoff = APPEND ? pos0 - kstart : 0;                   // frame position of query 0
  const int nqblk = (PADDED && !APPEND) ? (T + 127) / 128 : (int)gridDim.x;   // query blocks of the row
  if (PADDED && !APPEND) {
    // pad query rows of this workgroup's 128 (unshifted) rows: zeros
    for (int idx = tid; idx < 128 * (D / 4); idx += 256) {
      const int row = (int)blockIdx.x * 128 + idx / (D / 4);
      if (row < kstart) *(uint2*)(out + ((long)b * Tp + row) * ldo + (long)hh * D + 4 * (idx % (D / 4))) = uint2{0u, 0u};
    }
    if ((int)blockIdx.x >= nqblk) return;
  }
  // every other (batch row, head) takes its query blocks and its waves' row blocks in reverse order (r05, see the d = 128 kernel:
  // otherwise XCD gridDim.x - 1 and SIMD 3 collect all the long rows of the causal triangle); the results do not depend on it
  const int rev = (hh + b) & 1;
  const int q_wg = (rev ? nqblk - 1 - (int)blockIdx.x : (int)blockIdx.x) * 128;
  const int q_wave = q_wg + (rev ? 3 - wave : wave) * 32;
  // grouped-query attention (Llama family): query head hh reads K/V head hh / (heads / kv_heads); OPT: kv_heads == heads
  const int kh = hh / (heads / kv_heads);
  const long kv_row = (long)Bc * kv_heads * D;  // elements between consecutive sequence positions
  const bf16_t* kbase = kc + ((long)(b0 + b) * kv_heads + kh) * D + (long)kstart * kv_row;
  const bf16_t* vbase = vc + ((long)(b0 + b) * kv_heads + kh) * D + (long)kstart * kv_row;
  // OPT rounds q * d^-0.5 before the product (attentions.py:456); HF Llama rounds the product, then scales it
  // (eager_attention_forward: matmul(q, k^T) * scaling)
  const float qscale = post_scale ? 1.0f : scaling;

  // Qs fragments: B operand, lane holds Qs[q_wave + r][16 s + 8 h + j]
  bf16x8 qf[KSTEPS];
  {
    const int qrow = min(q_wave + r, Tq - 1);
    const bf16_t* qp = q + ((long)b * Tp + (APPEND ? 0 : kstart) + qrow) * ldq + (long)hh * D;
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
#ifdef P3X_NO_QLOAD
      uint4 v = uint4{(unsigned)lane, (unsigned)s, 0x3c003c00u, 0x3c003c00u};
#else
      uint4 v = *(const uint4*)(qp + 16 * s + 8 * h);
#endif
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      uint32_t o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = pack_bf16x2(bf2f(w[j] & 0xffff) * qscale, bf2f(w[j] >> 16) * qscale);
      qf[s] = __builtin_bit_cast(bf16x8, uint4{o[0], o[1], o[2], o[3]});
    }
  }

  const int n_tiles_wg = min((qoff + q_wg + 128 + 31) / 32, (T + 31) / 32);  // causal: keys <= last query of the WG
  const int my_row = q_wave + r;                                      // this lane's query within q / out ...
  const int my_q = qoff + my_row;                                     // ... and its frame position (column of S^T); prefill: the same

  auto stage_k = [&](int kt) {
    // 32 keys x D: thread -> (key = tid / CH', chunk); 256 threads move 4 KB per round
    constexpr int ROUNDS = (32 * CH + 255) / 256;
#pragma unroll
    for (int rr = 0; rr < ROUNDS; ++rr) {
      int idx = rr * 256 + tid;
      if (idx < 32 * CH) {
        int key = idx / CH, c = idx % CH;
        int gk = min(kt * 32 + key, T - 1);
        uint4 v = *(const uint4*)(kbase + (long)gk * kv_row + 8 * c);
        *(uint4*)(k_lds + key * (D * 2) + ((c ^ ((key / RPB) % CH)) << 4)) = v;
      }
    }
  };
  auto stage_vt = [&](int kt) {
    constexpr int ROUNDS = (32 * CH + 255) / 256;
#pragma unroll
    for (int rr = 0; rr < ROUNDS; ++rr) {
      int idx = rr * 256 + tid;
      if (idx < 32 * CH) {
        int key = idx / CH, c = idx % CH;
        int gk = min(kt * 32 + key, T - 1);
        uint4 v = *(const uint4*)(vbase + (long)gk * kv_row + 8 * c);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          *(bf16_t*)(vt_lds + (8 * c + 2 * j) * VT_STRIDE + key * 2) = (bf16_t)(w[j] & 0xffff);
          *(bf16_t*)(vt_lds + (8 * c + 2 * j + 1) * VT_STRIDE + key * 2) = (bf16_t)(w[j] >> 16);
        }
      }
    }
  };
  // S^T tile for key tile kt: lane gets S^T[key = kt*32 + (i&3) + 8*(i>>2) + 4h][query = my_q], rounded
  // to bf16 and causally masked
  auto scores = [&](int kt, f32x16& sacc) {
    sacc = f32x16{0};
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      uint4 kv = *(const uint4*)(k_lds + r * (D * 2) + (((2 * s + h) ^ ((r / RPB) % CH)) << 4));
      sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kv), qf[s], sacc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      int key = kt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
      float sv = rbf(sacc[i]);
      if (post_scale) sv = rbf(sv * scaling);
      sacc[i] = (key <= my_q && key < T) ? sv : -INFINITY;
    }
  };

  // ---- sweep 1: row max and sum of exp over all keys <= query ----
  float m = -INFINITY, l = 0.f;
  for (int kt = 0; kt < n_tiles_wg; ++kt) {
    __syncthreads();
    stage_k(kt);
    __syncthreads();
    if (kt * 32 <= qoff + q_wave + 31) {  // wave-uniform: tile not entirely above the diagonal
      f32x16 s;
      scores(kt, s);
      float tm = s[0];
#pragma unroll
      for (int i = 1; i < 16; ++i) tm = fmaxf(tm, s[i]);
      tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
      float mn = fmaxf(m, tm);
      if (mn > -INFINITY) {
        float ts = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) ts += __expf(s[i] - mn);
        ts += __shfl_xor(ts, 32, 64);
        l = l * __expf(m - mn) + ts;
        m = mn;
      }
    }
  }
  const float inv_l = 1.0f / l;

  // ---- sweep 2: P = bf16(exp(s - m) / l), O^T += V^T . P^T ----
  f32x16 oacc[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d) oacc[d] = f32x16{0};
  for (int kt = 0; kt < n_tiles_wg; ++kt) {
    __syncthreads();
    stage_k(kt);
    stage_vt(kt);
    __syncthreads();
    if (kt * 32 <= qoff + q_wave + 31) {
      f32x16 s;
      scores(kt, s);
      uint32_t pk[8];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        pk[i] = pack_bf16x2(__expf(s[2 * i] - m) / l, __expf(s[2 * i + 1] - m) / l);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8 pf = __builtin_bit_cast(bf16x8, uint4{pk[4 * ks], pk[4 * ks + 1], pk[4 * ks + 2], pk[4 * ks + 3]});
#pragma unroll
        for (int d = 0; d < DB; ++d) {
          const char* vrow = vt_lds + (32 * d + r) * VT_STRIDE + (16 * ks + 4 * h) * 2;
          uint2 lo = *(const uint2*)(vrow), hi = *(const uint2*)(vrow + 16);
          bf16x8 vf = __builtin_bit_cast(bf16x8, uint4{lo.x, lo.y, hi.x, hi.y});
          oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, oacc[d], 0, 0, 0);
        }
      }
    }
  }
  (void)inv_l;

  if (my_row < Tq) {
    bf16_t* op = out + ((long)b * Tp + (APPEND ? 0 : kstart) + my_row) * ldo + (long)hh * D;
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        uint2 o;
        o.x = pack_bf16x2(oacc[d][4 * g], oacc[d][4 * g + 1]);
        o.y = pack_bf16x2(oacc[d][4 * g + 2], oacc[d][4 * g + 3]);
        *(uint2*)(op + 32 * d + 8 * g + 4 * h) = o;
      }
  }
}


// ---------------------------------------------------------------------------------------------
// prefill, d = 128, third generation (r05).  The arithmetic -- every product, rounding, max / sum update and its order -- is that
// of lia_attn_prefill_kernel<128> and of the second generation (tools/attn_prefill_gen2.inc keeps that one;
// tools/attn_prefill_bench compares the two bit for bit on OPT-30B's, Llama-3-8B's and ragged shapes).  What changed is how the work
// is laid out, from per-wave cycle stamps and SQ counters of the second generation (LABNOTES.md r05: VALU 50 % busy, waves 40 % of
// their life in waits, SIMD 3 / XCD 7 holding every heavy piece of the causal triangle):
//   * K and V tiles (64 keys) go from global memory straight to LDS (global_load_lds, 16 B per lane, the images' chunk permutations
//     applied on the source address), double-buffered, ONE barrier per tile; the stage after sweep 1's last tile is sweep 2's first;
//   * a two-block tile runs as A: q.k chain of block 0 (fragments of block 1 fetched under it), B: chain of block 1 under the
//     softmax arithmetic of block 0, C: P.V of block 0 under the arithmetic of block 1, D: P.V of block 1 -- interleaved by hand
//     (sched_barrier between the pieces): hipcc otherwise serialises chain, arithmetic, chain, arithmetic;
//   * the arithmetic works on pairs (v_pk_add / v_pk_mul / v_pk_fma_f32, one v_cvt_pk_bf16_f32 per pair), masks are selects
//     (the second generation's `a || (b && c)` became a branch per element), POST_SCALE is a template parameter;
//   * every other (batch row, head) takes its query blocks and the four row blocks of a workgroup in reverse order.
// OPT-30B's B 64 x T 256 x 56 heads: 433 -> 333 us; Llama-3-8B's B 128 x T 1024 x 32 / 8 heads: 5.51 -> 3.23 ms.
// V^T operand: ds_read_b64_tr_b16 from the row-major image off(row, ch) = 256 row + 16 (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)))
// (lane 4q+p of a 16-lane group addresses row q, columns 4p..4p+3 of a 4-key x 16-dim block and receives one dim of the four keys).
// ---------------------------------------------------------------------------------------------
typedef short lia_v4s __attribute__((ext_vector_type(4)));
#define GL_AS1(p) ((const __attribute__((address_space(1))) void*)(p))
#define LDS_AS3(p) ((__attribute__((address_space(3))) void*)(p))

#define P3_KOFF(i) (((i) & 3) + 8 * ((i) >> 2))
typedef float f32x2 __attribute__((ext_vector_type(2)));

// one v_cvt_pk_bf16_f32 for the pair (compiler-visible: inline asm would hide the MFMA -> VALU read hazard from the hazard recognizer)
typedef __bf16 p3_bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t p3_cvt_pk(float a, float b) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, p3_bf16x2));
}
// two scores at the reference's rounding points: bf16 of q.k; with POST_SCALE the product by d^-0.5 and its rounding (values of rbf())
template <int POST_SCALE> __device__ __forceinline__ f32x2 p3_round2(float a, float b, float scaling) {
  uint32_t p = p3_cvt_pk(a, b);
  f32x2 r = {__uint_as_float(p << 16), __uint_as_float(p & 0xffff0000u)};
  if (POST_SCALE) {
    const f32x2 t = r * scaling;
    p = p3_cvt_pk(t.x, t.y);
    r = f32x2{__uint_as_float(p << 16), __uint_as_float(p & 0xffff0000u)};
  }
  return r;
}
// causal / length mask of elements 2 c, 2 c + 1 of the lane: key 32 kt + 4 h + P3_KOFF(i) is visible iff P3_KOFF(i) <= lim
__device__ __forceinline__ f32x2 p3_mask2(f32x2 r, int lim, int c) {
  return f32x2{(lim >= P3_KOFF(2 * c)) ? r.x : -INFINITY, (lim >= P3_KOFF(2 * c + 1)) ? r.y : -INFINITY};
}
// __expf(r - m) of a pair: the subtraction, the product by log2(e) and v_exp_f32, as __expf lowers it
__device__ __forceinline__ f32x2 p3_exp2(f32x2 r, float m) {
  const f32x2 t = (r - m) * 0x1.715476p+0f;
  return f32x2{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
}
// bf16(e / l) of a pair, packed: hoisted reciprocal + two residual corrections = the correctly rounded quotient (second generation)
__device__ __forceinline__ uint32_t p3_prob2(f32x2 r, float m, float l, float rl) {
  const f32x2 e = p3_exp2(r, m);
  const f32x2 nl = (f32x2)(-l), rr = (f32x2)rl;
  f32x2 q = e * rl;
  q = __builtin_elementwise_fma(__builtin_elementwise_fma(nl, q, e), rr, q);
  q = __builtin_elementwise_fma(__builtin_elementwise_fma(nl, q, e), rr, q);
  return p3_cvt_pk(q.x, q.y);
}

// r06: the same operations on TWO pairs at a time.  A pair's chain -- subtract, scale, exp, e * (1 / l) and the four residual
// fmas -- is ten dependent instructions, and behind every packed one hipcc must put an s_nop before its consumer: 75-99 s_nop
// per sweep-2 tile, each a 1.8 ns issue slot of the wave (tools/issue_model).  As 4-wide vector operations every stage
// legalises into two independent packed instructions side by side, so a stage's consumer is one instruction away and needs no
// s_nop: 79-85 -> 8-10 per tile (+11 vector instructions).  Same operations on the same values: bit-identical.  Sweep 2 only:
// in sweep 1 the 4-wide subtraction comes out as 32 single instructions instead of 16 packed ones and the gain is gone.
template <int POST_SCALE, int MASKED>
__device__ __forceinline__ f32x4 p3_round4(float a0, float a1, float a2, float a3, float scaling, int lim, int c) {
  uint32_t p0 = p3_cvt_pk(a0, a1), p1 = p3_cvt_pk(a2, a3);
  f32x4 r = {__uint_as_float(p0 << 16), __uint_as_float(p0 & 0xffff0000u), __uint_as_float(p1 << 16), __uint_as_float(p1 & 0xffff0000u)};
  if (POST_SCALE) {
    const f32x4 t = r * scaling;
    p0 = p3_cvt_pk(t.x, t.y);
    p1 = p3_cvt_pk(t.z, t.w);
    r = f32x4{__uint_as_float(p0 << 16), __uint_as_float(p0 & 0xffff0000u), __uint_as_float(p1 << 16), __uint_as_float(p1 & 0xffff0000u)};
  }
  if (MASKED) {      // pairs c and c + 1 (p3_mask2)
    r.x = (lim >= P3_KOFF(2 * c)) ? r.x : -INFINITY;
    r.y = (lim >= P3_KOFF(2 * c + 1)) ? r.y : -INFINITY;
    r.z = (lim >= P3_KOFF(2 * c + 2)) ? r.z : -INFINITY;
    r.w = (lim >= P3_KOFF(2 * c + 3)) ? r.w : -INFINITY;
  }
  return r;
}
__device__ __forceinline__ f32x4 p3_exp4(f32x4 r, float m) {
  const f32x4 t = (r - m) * 0x1.715476p+0f;
  return f32x4{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y), __builtin_amdgcn_exp2f(t.z), __builtin_amdgcn_exp2f(t.w)};
}
__device__ __forceinline__ uint2 p3_prob4(f32x4 r, float m, float l, float rl) {
  const f32x4 e = p3_exp4(r, m);
  const f32x4 nl = (f32x4)(-l), rr = (f32x4)rl;
  f32x4 q = e * rl;
  q = __builtin_elementwise_fma(__builtin_elementwise_fma(nl, q, e), rr, q);
  q = __builtin_elementwise_fma(__builtin_elementwise_fma(nl, q, e), rr, q);
  return uint2{p3_cvt_pk(q.x, q.y), p3_cvt_pk(q.z, q.w)};
}

// APPEND = 1: Tp queries at cache positions pos0 .. pos0 + Tp - 1 over the keys kstart .. pos0 + Tp - 1 (the frames of
// lia_attn_prefill_kernel: keys from kstart, queries from qoff = pos0 - kstart); q / out hold the block's rows only.  Staging, barriers,
// order, pairing and the output path are the prefill's.  The mirror pairing still balances: block bx visits ~(qoff + 128 (bx + 1)) / 64
// tiles -- a rectangle of qoff keys plus the triangle -- so cost(bx) + cost(nqb_all - 1 - bx) is the same for every pair.
template <int POST_SCALE, int PADDED, int APPEND>
__device__ __forceinline__ void lia_attn_prefill128_body(const bf16_t* __restrict__ q, long ldq, const bf16_t* __restrict__ kc,
                                                         const bf16_t* __restrict__ vc, bf16_t* __restrict__ out, long ldo, int Tp, int pos0,
                                                         int heads, int kv_heads, long kv_row, long kv_batch, int b0, float scaling,
                                                         int nqb, int n_groups, const int* __restrict__ starts) {
  constexpr int D = 128;
  __shared__ __attribute__((aligned(16))) char lds[2][2][64 * 256];   // [buffer][0 = K, 1 = V][key row of 256 bytes]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // r06: XCD-aware order (n_groups > 0).  The workgroups that read the same K / V -- every query block of the G query heads of one
  // (batch row, KV head) -- form a group of nqb * G members; group g runs on XCD g % 8 (workgroup ids are dealt round-robin over
  // the XCDs: id % 8), its members in consecutive slots of that XCD.  A K / V tile is then fetched into ONE L2 and found there by
  // the other members (and by the second sweep) instead of crossing the fabric once per XCD: the per-tile wait is an L2 hit, which
  // the one-tile-deep LDS-DMA prefetch covers; a miss (2-3 us under load) it does not (a tile's arithmetic is ~1.2 us).
  // OPT-30B T 2016: 1872 -> 1512 us per 8-row minibatch, bit-identical (tools/attn_prefill_bench, -DLIA_ATTN_LEGACY_GRID for r05's).
  // n_groups <= 0: r05's order -- consecutive ids = the query blocks of one head -- kept for launches whose groups do not spread
  // evenly over the 8 XCDs (the launcher decides).
  int bx, hh, b;
  if (n_groups > 0) {
    const int Gq = heads / kv_heads;
    const int nmem = nqb * Gq;
    const int slot = (int)(blockIdx.x >> 3);
    const int grp = (slot / nmem) * 8 + (int)(blockIdx.x & 7);
    if (grp >= n_groups) return;                      // (the grid is padded to a multiple of 8 groups)
    const int mem = slot % nmem;
    bx = mem % nqb;
    b = grp / kv_heads;
    hh = (grp % kv_heads) * Gq + mem / nqb;
  } else {
    bx = (int)(blockIdx.x % nqb);
    hh = (int)((blockIdx.x / nqb) % heads);
    b = (int)(blockIdx.x / ((unsigned)nqb * heads));
  }
  // every other (batch row, head) takes its query blocks -- and, below, the four row blocks of a workgroup -- in reverse order:
  // wave w of a workgroup goes to SIMD w, and late rows have more keys to visit, so without it SIMD 3 would get every heavy piece
  // and SIMD 0 every light one (with r05's grid: XCD 7 / XCD 0 as well)
  const int rev = (hh + b) & 1;
  // r06: a workgroup takes TWO query blocks of its head, block bx and its mirror image nqb_all - 1 - bx (the launcher passes
  // nqb = ceil(nqb_all / 2) then; nqb == nqb_all: one block per workgroup as before).  A light block and a heavy one: every
  // workgroup of a sequence costs the same (causal: 1 + ... keys), half as many workgroups are launched and drained -- the
  // launches alone were 75 us of the 313 us of OPT-30B's T = 256 launch (the kernel without loads, arithmetic and stores,
  // LABNOTES r06) -- and the second block's K / V tiles were just read by the first.
  // PADDED: the row's T - kstart tokens from its start kstart on form the sequence (the shifted frame of lia_attn_prefill_kernel); its
  // nqa query blocks are dealt to the first nqr workgroups of the row by the same pairing, Tp is the rows' pitch in q / out.
  // (With padding the pairs of one launch no longer cost the same: rows with later starts finish early.)
  const int kstart = PADDED ? __builtin_amdgcn_readfirstlane(starts[b]) : 0;   // (uniform: keeps the row start scalar)
  const int T = (APPEND ? pos0 + Tp : Tp) - kstart;               // keys of the frame
  const int Tq = APPEND ? Tp : T;                                // queries: the block's (append, no pad rows) or the frame's
  const int qoff = APPEND ? pos0 - kstart : 0;                   // frame position of query 0
  const int nqb_all = (Tp + 127) >> 7;
  const bool pairs = nqb != nqb_all;
  const int nqa = (PADDED && !APPEND) ? (T + 127) >> 7 : nqb_all;
  const int nqr = (PADDED && !APPEND) ? (pairs ? (nqa + 1) >> 1 : nqa) : nqb;
  if (PADDED && !APPEND) {
    // pad query rows of the (unshifted) blocks this workgroup is dealt -- bx and, with pairs, its mirror: zeros, no K / V work
    for (int k = 0; k < (pairs ? 2 : 1); ++k) {
      const int ob = k ? nqb_all - 1 - bx : bx;
      if (k && ob == bx) break;
      for (int idx = tid; idx < 128 * 16; idx += 256) {
        const int row = ob * 128 + (idx >> 4);
        if (row < kstart) *(uint4*)(out + ((long)b * Tp + row) * ldo + (long)hh * D + 8 * (idx & 15)) = uint4{0u, 0u, 0u, 0u};
      }
    }
    if (bx >= nqr) return;
  }
  const int npass = (pairs && nqa - 1 - bx != bx) ? 2 : 1;
  const int wsub = rev ? 3 - wave : wave;
  const int kh = hh / (heads / kv_heads);
  const bf16_t* kbase = kc + (long)(b0 + b) * kv_batch + (long)kh * D + (long)kstart * kv_row;
  const bf16_t* vbase = vc + (long)(b0 + b) * kv_batch + (long)kh * D + (long)kstart * kv_row;
  const float qscale = POST_SCALE ? 1.0f : scaling;

  // ---- staging by LDS-DMA: instruction j of wave w moves key rows 16 j + 4 w + (lane >> 4) of the tile, one 16-byte chunk per lane,
  // to consecutive LDS bytes (1 KB per instruction); the images' chunk permutations are applied on the SOURCE side:
  //   K: chunk c of row R sits in slot c ^ (R & 15);  V: in slot c ^ (((R & 3) << 2) | ((R >> 2) & 3))   (R & 15 = 4 w + (lane >> 4))
  // r06: the address of a row is a UNIFORM base (first row of the instruction's 16, scalar 64-bit arithmetic) plus a 32-bit
  // per-lane byte offset (row within the 16, clamped to the sequence's last row, + chunk): the global saddr form.  r05 computed
  // min(key, T - 1) * kv_row per lane in 64 bits -- ~36 of a tile's ~230 vector instructions in a VALU-bound loop (read in the ISA).
  const int srow = 4 * wave + (lane >> 4), sslot = lane & 15;
  // Second form (r06): ONE scalar base per tile (its first row) and the lane's row within the 64 clamped against one scalar limit,
  // min(srow + 16 j, T - 1 - 64 t) rows -- the per-instruction scalar arithmetic of the first form (a 64-bit product, two minima and
  // two adds, x 4) was 77-84 scalar instructions per tile, and scalar instructions cost 1.8 ns each WITHOUT overlapping between the
  // two waves of a SIMD (tools/issue_model): now 23-30.
  const unsigned kvrow_b = (unsigned)kv_row * 2u;                  // bytes per key row (the launcher checks 64 rows fit 32 bits)
  unsigned rowoff_b[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) rowoff_b[j] = (unsigned)(srow + 16 * j) * kvrow_b;
  const unsigned kch_b = 16u * (unsigned)(sslot ^ srow);
  const unsigned vch_b = 16u * (unsigned)(sslot ^ (((srow & 3) << 2) | ((srow >> 2) & 3)));
  // (measurement switches of tools/attn_prefill_bench, never defined in the library build: -DP3X_NO_LOADS leaves the K / V stages
  // out, -DP3X_NO_MATH the tiles' arithmetic, -DP3X_NO_WAIT the wait for a stage (wrong results) -- where a tile step's time goes, LABNOTES r06)
#ifdef P3X_NO_WAIT
#define P3X_WAIT() do {} while (0)
#else
#define P3X_WAIT() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#endif
#ifdef P3X_NO_LOADS
#define P3X_NJ 0
#else
#define P3X_NJ 4
#endif
#define P3_ISSUE(t, buf, WITH_V)                                                                                                   \
  do {                                                                                                                             \
    int t0_ = (t) * 64;                                                 /* uniform; <= T - 1: the tile holds a valid row */        \
    asm volatile("" : "+s"(t0_));   /* (opaque: or loop strength reduction turns the bases into per-lane 64-bit pointers) */       \
    const unsigned lim_ = (unsigned)min(T - 1 - t0_, 63) * kvrow_b;     /* min(t0 + row, T - 1) = t0 + min(row, T - 1 - t0) */     \
    const long base_ = (long)t0_ * (long)kvrow_b;                                                                                  \
    _Pragma("unroll") for (int j_ = 0; j_ < P3X_NJ; ++j_) {                                                                        \
      const unsigned ro_ = min(rowoff_b[j_], lim_);                                                                                \
      __builtin_amdgcn_global_load_lds(GL_AS1((const char*)kbase + base_ + (ro_ + kch_b)),                                        \
                                       LDS_AS3(&lds[buf][0][(16 * j_ + 4 * wave) * 256]), 16, 0, 0);                               \
      if (WITH_V)                                                                                                                  \
        __builtin_amdgcn_global_load_lds(GL_AS1((const char*)vbase + base_ + (ro_ + vch_b)),                                      \
                                         LDS_AS3(&lds[buf][1][(16 * j_ + 4 * wave) * 256]), 16, 0, 0);                             \
    }                                                                                                                              \
  } while (0)

  for (int pass = 0; pass < npass; ++pass) {
  // (the lane-derived LDS offsets below are the same in both passes; behind this opaque copy hipcc recomputes them per pass
  // instead of keeping ~20 more registers alive through both sweeps: as a plain loop the kernel needed 256 registers + scratch
  // and ran 19 % slower than without the loop)
  int lane_p_ = lane;
  asm volatile("" : "+v"(lane_p_));
  const int lane = lane_p_;
  const int r = lane & 31, h = lane >> 5;
  // (the blocks in reverse order for every other (batch row, head), as the waves: see `rev`)
  const int bxp = pairs ? (((pass ^ rev) & 1) ? nqa - 1 - bx : bx) : (rev ? nqr - 1 - bx : bx);
  const int q_wg = bxp * 128;
  const int q_wave = q_wg + wsub * 32;
  // (the first block's output staging lives in stage buffer 0, where the second block's first K tile goes)
  if (pass) __syncthreads();
  // r06: the first K tile is requested BEFORE the query rows -- the LDS-DMA needs no register, and the workgroup's two first
  // round trips to memory (q rows into registers, K tile 0 into LDS) then overlap instead of following each other (~1.5 us of a
  // ~16 us workgroup at T = 256: the prologue was ~5 us of it, LABNOTES r05)
  P3_ISSUE(0, 0, false);

  bf16x8 qf[8];
  {
    const int qrow = min(q_wave + r, Tq - 1);
    const bf16_t* qp = q + ((long)b * Tp + (APPEND ? 0 : kstart) + qrow) * ldq + (long)hh * D;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      uint4 v = *(const uint4*)(qp + 16 * s + 8 * h);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      uint32_t o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = pack_bf16x2(bf2f(w[j] & 0xffff) * qscale, bf2f(w[j] >> 16) * qscale);
      qf[s] = __builtin_bit_cast(bf16x8, uint4{o[0], o[1], o[2], o[3]});
    }
  }

  const int n32 = min((qoff + q_wg + 128 + 31) / 32, (T + 31) / 32);   // 32-key blocks the workgroup needs (causal)
  const int n64 = (n32 + 1) / 2;
  const int my_q = qoff + q_wave + r;                           // (frame position)
  const int nblk = min(qoff + q_wave + 31, T - 1) / 32 + 1;     // 32-key blocks THIS wave needs: 0 .. nblk - 1
  const int vis = min(my_q, T - 1) - 4 * h;                     // key 32 kt + 4 h + koff is visible iff koff <= vis - 32 kt

  // K^T fragment of 16-dim slice ss: key row 32 sb + r, chunk (2 ss + h) ^ (r & 15)
  int k_rd[8];
#pragma unroll
  for (int ss = 0; ss < 8; ++ss) k_rd[ss] = r * 256 + (((2 * ss + h) ^ (r & 15)) << 4);
  // V^T transposed read (ds_read_b64_tr_b16), as in the second generation
  const int tq = (lane & 15) >> 2, tp = lane & 3, g1 = (lane >> 4) & 1;
  int v_rd[2][4];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int key = 4 * h + 8 * u + tq;
      const int ch = 4 * d + 2 * g1 + (tp >> 1);
      v_rd[u][d] = 256 * key + 16 * (ch ^ (((key & 3) << 2) | ((key >> 2) & 3))) + 8 * (tp & 1);
    }

#define P3_KFRAGS(kf, kb, sb)                                                                                              \
  do { _Pragma("unroll") for (int ss_ = 0; ss_ < 8; ++ss_) kf[ss_] = *(const uint4*)((kb) + (sb) * 8192 + k_rd[ss_]); } while (0)
#define P3_QK(kf, sacc)                                                                                                    \
  do {                                                                                                                     \
    sacc = f32x16{0};                                                                                                      \
    _Pragma("unroll") for (int ss_ = 0; ss_ < 8; ++ss_)                                                                    \
      sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kf[ss_]), qf[ss_], sacc, 0, 0, 0);         \
  } while (0)

  // ---- sweep 1: row max and sum of exp over the visible keys ----
  // statistics of a block held as eight rounded pairs: the first generation's operations in its order (its `if (mn > -inf)` is
  // always taken: key 0 is visible to every query, so the running maximum is finite from block 0 on)
#define P3_STATS(rp)                                                                                                       \
  do {                                                                                                                     \
    float tm_ = fmaxf(rp[0].x, rp[0].y);                                                                                   \
    _Pragma("unroll") for (int c_ = 1; c_ < 8; ++c_) tm_ = fmaxf(tm_, fmaxf(rp[c_].x, rp[c_].y));                          \
    tm_ = fmaxf(tm_, __shfl_xor(tm_, 32, 64));                                                                             \
    const float mn_ = fmaxf(m, tm_);                                                                                       \
    float ts_ = 0.f;                                                                                                       \
    _Pragma("unroll") for (int c_ = 0; c_ < 8; ++c_) {                                                                     \
      const f32x2 e_ = p3_exp2(rp[c_], mn_);                                                                               \
      ts_ += e_.x;                                                                                                         \
      ts_ += e_.y;                                                                                                         \
    }                                                                                                                      \
    ts_ += __shfl_xor(ts_, 32, 64);                                                                                        \
    l = l * __expf(m - mn_) + ts_;                                                                                         \
    m = mn_;                                                                                                               \
  } while (0)
#define P3_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)
  // chain 0 of a two-block tile with the K^T fragments of block 1 fetched under it
#define P3_CHAIN0()                                                                                                        \
  P3_KFRAGS(kf0, kb, 0);                                                                                                   \
  _Pragma("unroll") for (int c = 0; c < 8; ++c) {                                                                          \
    s0 = P3_MFMA(__builtin_bit_cast(bf16x8, kf0[c]), qf[c], s0);                                                           \
    kf1[c] = *(const uint4*)(kb + 8192 + k_rd[c]);                                                                         \
    __builtin_amdgcn_sched_barrier(0);                                                                                     \
  }                                                                                                                        \
  __builtin_amdgcn_sched_barrier(0)
  // two visible blocks: chain 1 runs under the statistics of block 0 (never masked here) -- MFMAs 0..3 beside the rounding and the
  // maximum, 4..7 beside the sum of exp; then block 1, always through the mask (it may hold the diagonal or the end of the sequence)
#ifdef P3X_NO_MATH
#define P3X_MATH 0
#else
#define P3X_MATH 1
#endif
#define P3_S1_TILE2(MASK0, MASKED)                                                                                         \
  if (P3X_MATH) do {                                                                                                                     \
    uint4 kf0[8], kf1[8];                                                                                                  \
    f32x16 s0 = f32x16{0}, s1 = f32x16{0};                                                                                 \
    f32x2 rp[8];                                                                                                           \
    float tm = -INFINITY, mn = 0.f, ts = 0.f;                                                                              \
    P3_CHAIN0();                                                                                                           \
    _Pragma("unroll") for (int c = 0; c < 8; ++c) {                                                                        \
      s1 = P3_MFMA(__builtin_bit_cast(bf16x8, kf1[c]), qf[c], s1);                                                         \
      if (c < 4) {                                                                                                         \
        rp[2 * c] = p3_round2<POST_SCALE>(s0[4 * c], s0[4 * c + 1], scaling);                                              \
        rp[2 * c + 1] = p3_round2<POST_SCALE>(s0[4 * c + 2], s0[4 * c + 3], scaling);                                      \
        if (MASK0) {                                                                                                       \
          rp[2 * c] = p3_mask2(rp[2 * c], lim1 + 32, 2 * c);                                                               \
          rp[2 * c + 1] = p3_mask2(rp[2 * c + 1], lim1 + 32, 2 * c + 1);                                                   \
        }                                                                                                                  \
        tm = fmaxf(fmaxf(tm, fmaxf(rp[2 * c].x, rp[2 * c].y)), fmaxf(rp[2 * c + 1].x, rp[2 * c + 1].y));                   \
        if (c == 3) {                                                                                                      \
          tm = fmaxf(tm, __shfl_xor(tm, 32, 64));                                                                          \
          mn = fmaxf(m, tm);                                                                                               \
        }                                                                                                                  \
      } else {                                                                                                             \
        const f32x2 e0 = p3_exp2(rp[2 * (c - 4)], mn), e1 = p3_exp2(rp[2 * (c - 4) + 1], mn);                              \
        ts += e0.x; ts += e0.y; ts += e1.x; ts += e1.y;                                                                    \
      }                                                                                                                    \
      __builtin_amdgcn_sched_barrier(0);                                                                                   \
    }                                                                                                                      \
    ts += __shfl_xor(ts, 32, 64);                                                                                          \
    l = l * __expf(m - mn) + ts;                                                                                           \
    m = mn;                                                                                                                \
    _Pragma("unroll") for (int c = 0; c < 8; ++c) {                                                                        \
      rp[c] = p3_round2<POST_SCALE>(s1[2 * c], s1[2 * c + 1], scaling);                                                    \
      if (MASKED) rp[c] = p3_mask2(rp[c], lim1, c);                                                                        \
    }                                                                                                                      \
    P3_STATS(rp);                                                                                                          \
  } while (0)

  float m = -INFINITY, l = 0.f;
  // r06: both sweeps are FOUR loops instead of one loop with three cases.  A wave has two visible key blocks in tiles 0 .. nfull - 1
  // (nfull = nblk / 2), one in tile nfull when nblk is odd (the diagonal / the end of the sequence), none behind it -- but every
  // wave meets every barrier and issues its share of every stage; and in tiles 0 .. nfree - 1 the LAST key of the tile is visible
  // to the wave's FIRST query (64 t + 63 <= min(q_wave, T - 1)), so block 1's mask selects nothing there and is left out (two
  // v_cmp + two v_cndmask per pair: 12-14 % of a tile's vector instructions).  As ONE loop (`if (nb >= 2) ... else if (nb == 1)`)
  // hipcc also merged sweep 2's 64 accumulator registers at the latch: 64 v_mov out of the two-block body and 64 back on the
  // back-edge, 128 of ~400 vector instructions per iteration (found in the ISA).  Same operations on the same values in the same order.
  const int nfull = nblk >> 1;                                     // (<= n64: nblk <= n32 <= 2 n64)
  const int nfree = min((min(qoff + q_wave, T - 1) + 1) >> 6, nfull);
  // APPEND: the query frame is not aligned to the key blocks (qoff is any number), so the diagonal may cross BOTH blocks of a tile;
  // block 0 of tile t is wholly visible to the wave's first query while 2 t < (its position + 1) / 32 -- tiles 0 .. nb0 - 1 -- and the
  // one two-block tile behind them, if any, masks block 0 as well.  Prefill: q_wave is a multiple of 32, nb0 == nfull.
  const int nb0 = APPEND ? min((((min(qoff + q_wave, T - 1) + 1) >> 5) + 1) >> 1, nfull) : nfull;
#define P3_S1_STEP()                                                                                                       \
  P3X_WAIT();                                                                                                              \
  __syncthreads();                                                                                                         \
  /* (the stage after sweep 1's last tile is sweep 2's first: its K and V ride under this tile's arithmetic) */           \
  if (t + 1 < n64) P3_ISSUE(t + 1, (t + 1) & 1, false);                                                                    \
  else P3_ISSUE(0, n64 & 1, true);                                                                                         \
  const char* kb = &lds[t & 1][0][0];                                                                                      \
  const int lim1 = vis - 32 * (2 * t + 1)
  {
    int t = 0;
    for (; t < nfree; ++t) {
      P3_S1_STEP();
      P3_S1_TILE2(0, 0);
      (void)lim1;
    }
    for (; t < nb0; ++t) {
      P3_S1_STEP();
      P3_S1_TILE2(0, 1);
    }
    if (APPEND && t < nfull) {     // the diagonal in both blocks of a tile (at most one such tile)
      P3_S1_STEP();
      P3_S1_TILE2(1, 1);
      ++t;
    }
    if (t < n64) {
      P3_S1_STEP();
      if (nblk & 1) {
        uint4 kf0[8];
        f32x16 s0;
        f32x2 rp[8];
        P3_KFRAGS(kf0, kb, 0);
        P3_QK(kf0, s0);
#pragma unroll
        for (int c = 0; c < 8; ++c) rp[c] = p3_mask2(p3_round2<POST_SCALE>(s0[2 * c], s0[2 * c + 1], scaling), lim1 + 32, c);
        P3_STATS(rp);
      }
      ++t;
    }
    for (; t < n64; ++t) {
      P3_S1_STEP();
      (void)kb; (void)lim1;
    }
  }
#undef P3_S1_STEP

  // ---- sweep 2: P = bf16(exp(s - m) / l), O^T += V^T . P^T ----
  const float rl0 = __builtin_amdgcn_rcpf(l);
  const float rl = __builtin_fmaf(__builtin_fmaf(-l, rl0, 1.0f), rl0, rl0);
  f32x16 oacc[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) oacc[d] = f32x16{0};
  // V^T piece c = (ks = c >> 2, d = c & 3) of block sb: keys 32 sb + 16 ks + 4 h + (0..3) -> elements 0..3, the same + 8 -> elements
  // 4..7 (the k order of an accumulator tile used as an operand); dims 32 d ..
#define P3_VFRAG(dst, vb, sb, c)                                                                                            \
  do {                                                                                                                     \
    const char* vt_ = (vb) + (32 * (sb) + 16 * ((c) >> 2)) * 256;                                                          \
    lia_v4s lo_ = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) lia_v4s*)(vt_ + v_rd[0][(c) & 3])); \
    lia_v4s hi_ = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) lia_v4s*)(vt_ + v_rd[1][(c) & 3])); \
    dst = __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo_, hi_, 0, 1, 2, 3, 4, 5, 6, 7));                           \
  } while (0)
#define P3_PF(pk, c) __builtin_bit_cast(bf16x8, uint4{pk[4 * ((c) >> 2)], pk[4 * ((c) >> 2) + 1], pk[4 * ((c) >> 2) + 2], pk[4 * ((c) >> 2) + 3]})
  // two visible blocks: chain 1 under the softmax of block 0, P.V of block 0 under the softmax of block 1, then P.V of block 1; the
  // V^T pieces are fetched one phase ahead.  Every oacc[d] takes its four products in the order (block 0, ks 0), (0, 1), (1, 0), (1, 1).
#define P3_S2_TILE2(MASK0, MASKED)                                                                                         \
  if (P3X_MATH) do {                                                                                                                     \
    uint4 kf0[8], kf1[8];                                                                                                  \
    f32x16 s0 = f32x16{0}, s1 = f32x16{0};                                                                                 \
    uint32_t pk0[8], pk1[8];                                                                                               \
    bf16x8 vfa[8], vfb[8];                                                                                                 \
    P3_CHAIN0();                                                                                                           \
    _Pragma("unroll") for (int c2 = 0; c2 < 4; ++c2) {                                                                     \
      _Pragma("unroll") for (int c = 2 * c2; c < 2 * c2 + 2; ++c) {                                                        \
        s1 = P3_MFMA(__builtin_bit_cast(bf16x8, kf1[c]), qf[c], s1);                                                       \
        P3_VFRAG(vfa[c], vb, 0, c);                                                                                        \
      }                                                                                                                    \
      {                                                                                                                    \
        const uint2 p_ = p3_prob4(p3_round4<POST_SCALE, MASK0>(s0[4 * c2], s0[4 * c2 + 1], s0[4 * c2 + 2], s0[4 * c2 + 3], scaling, MASK0 ? lim1 + 32 : 0, MASK0 ? 2 * c2 : 0), m, l, rl); \
        pk0[2 * c2] = p_.x;                                                                                                \
        pk0[2 * c2 + 1] = p_.y;                                                                                            \
      }                                                                                                                    \
      __builtin_amdgcn_sched_barrier(0);                                                                                   \
    }                                                                                                                      \
    _Pragma("unroll") for (int c2 = 0; c2 < 4; ++c2) {                                                                     \
      _Pragma("unroll") for (int c = 2 * c2; c < 2 * c2 + 2; ++c) {                                                        \
        oacc[c & 3] = P3_MFMA(vfa[c], P3_PF(pk0, c), oacc[c & 3]);                                                         \
        P3_VFRAG(vfb[c], vb, 1, c);                                                                                        \
      }                                                                                                                    \
      {                                                                                                                    \
        const uint2 p_ = p3_prob4(p3_round4<POST_SCALE, MASKED>(s1[4 * c2], s1[4 * c2 + 1], s1[4 * c2 + 2], s1[4 * c2 + 3], scaling, lim1, 2 * c2), m, l, rl); \
        pk1[2 * c2] = p_.x;                                                                                                \
        pk1[2 * c2 + 1] = p_.y;                                                                                            \
      }                                                                                                                    \
      __builtin_amdgcn_sched_barrier(0);                                                                                   \
    }                                                                                                                      \
    _Pragma("unroll") for (int c = 0; c < 8; ++c) oacc[c & 3] = P3_MFMA(vfb[c], P3_PF(pk1, c), oacc[c & 3]);               \
  } while (0)

  // (four loops, as sweep 1)
#define P3_S2_STEP()                                                                                                       \
  P3X_WAIT();                                                                                                              \
  __syncthreads();                                                                                                         \
  if (t + 1 < n64) P3_ISSUE(t + 1, (n64 + t + 1) & 1, true);                                                               \
  const char* kb = &lds[(n64 + t) & 1][0][0];                                                                              \
  const char* vb = &lds[(n64 + t) & 1][1][0];                                                                              \
  const int lim1 = vis - 32 * (2 * t + 1)
  int t = 0;
  for (; t < nfree; ++t) {
    P3_S2_STEP();
    P3_S2_TILE2(0, 0);
    (void)lim1;
  }
  for (; t < nb0; ++t) {
    P3_S2_STEP();
    P3_S2_TILE2(0, 1);
  }
  if (APPEND && t < nfull) {
    P3_S2_STEP();
    P3_S2_TILE2(1, 1);
    ++t;
  }
  if (t < n64) {
    P3_S2_STEP();
    if (nblk & 1) {
      uint4 kf0[8];
      f32x16 s0;
      uint32_t pk0[8];
      bf16x8 vfa[8];
      P3_KFRAGS(kf0, kb, 0);
      P3_QK(kf0, s0);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        P3_VFRAG(vfa[c], vb, 0, c);
        pk0[c] = p3_prob2(p3_mask2(p3_round2<POST_SCALE>(s0[2 * c], s0[2 * c + 1], scaling), lim1 + 32, c), m, l, rl);
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) oacc[c & 3] = P3_MFMA(vfa[c], P3_PF(pk0, c), oacc[c & 3]);
    }
    (void)vb;
    ++t;
  }
  for (; t < n64; ++t) {
    P3_S2_STEP();
    (void)kb; (void)vb; (void)lim1;
  }
#undef P3_S2_STEP
#undef P3_S2_TILE2
#undef P3_S1_TILE2
#undef P3_CHAIN0
#undef P3_STATS
#undef P3_PF
#undef P3_MFMA
#undef P3_VFRAG
#undef P3_QK
#undef P3_KFRAGS
#undef P3_ISSUE

  // ---- output: through the LDS, so that a store instruction writes whole rows ----
  // A lane holds 4 consecutive dims of ONE query per accumulator register group: stored from the registers, an instruction
  // writes 16 bytes to each of 32 rows (r05: 16 such instructions per wave, 512 partial-line writes).  Measured with the stores
  // left out (-DP3X_NO_STORE): 66 of the 330 us of OPT-30B's T = 256 launch, 70 of Llama-3-8B's 901.  r06: each wave parks its
  // 32 rows x 256 bytes in its own 8 KB of stage buffer 0 -- free since the barrier of the last step: the last tile of sweep 2
  // lives in buffer (2 n64 - 1) & 1 = 1 and no stage was issued behind it -- 16-byte chunks XOR-swizzled by the row as the K
  // image, and reads them back row-major: 8 instructions of 4 rows x 256 contiguous bytes.  Wave-private, in order: no barrier.
  {
    char* ob = &lds[0][0][0] + wave * 8192;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        uint2 o;
        o.x = pack_bf16x2(oacc[d][4 * g], oacc[d][4 * g + 1]);
        o.y = pack_bf16x2(oacc[d][4 * g + 2], oacc[d][4 * g + 3]);
        *(uint2*)(ob + r * 256 + (((4 * d + g) ^ (r & 15)) << 4) + 8 * h) = o;
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const int orow = lane >> 4, oc = lane & 15;
#ifdef P3X_NO_STORE
    const bool st_on = scaling == 12345.f;
#else
    const bool st_on = true;
#endif
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int rr = 4 * i + orow;
      const uint4 v = *(const uint4*)(ob + rr * 256 + ((oc ^ (rr & 15)) << 4));
      if (q_wave + rr < Tq && st_on) *(uint4*)(out + ((long)b * Tp + (APPEND ? 0 : kstart) + q_wave + rr) * ldo + (long)hh * D + 8 * oc) = v;
    }
  }
  }   // pass
}

template <int POST_SCALE>
__global__ __launch_bounds__(256, 2) void lia_attn_prefill128_kernel(const bf16_t* __restrict__ q, long ldq, const bf16_t* __restrict__ kc,
                                                                  const bf16_t* __restrict__ vc, bf16_t* __restrict__ out, long ldo, int T,
                                                                  int heads, int kv_heads, long kv_row, long kv_batch, int b0, float scaling,
                                                                  int nqb, int n_groups) {
  lia_attn_prefill128_body<POST_SCALE, 0, 0>(q, ldq, kc, vc, out, ldo, T, 0, heads, kv_heads, kv_row, kv_batch, b0, scaling, nqb, n_groups, nullptr);
}
// starts: per served row b (the caller passes its table + b0)
template <int POST_SCALE>
__global__ __launch_bounds__(256, 2) void lia_attn_prefill128_padded_kernel(const bf16_t* __restrict__ q, long ldq, const bf16_t* __restrict__ kc,
                                                                         const bf16_t* __restrict__ vc, bf16_t* __restrict__ out, long ldo, int T,
                                                                         int heads, int kv_heads, long kv_row, long kv_batch, int b0, float scaling,
                                                                         int nqb, int n_groups, const int* __restrict__ starts) {
  lia_attn_prefill128_body<POST_SCALE, 1, 0>(q, ldq, kc, vc, out, ldo, T, 0, heads, kv_heads, kv_row, kv_batch, b0, scaling, nqb, n_groups, starts);
}
// the append block (APPEND = 1 of the body): Tq queries at pos0 .. pos0 + Tq - 1; PADDED reads the row starts, else starts is unused
template <int POST_SCALE, int PADDED>
__global__ __launch_bounds__(256, 2) void lia_attn_append128_kernel(const bf16_t* __restrict__ q, long ldq, const bf16_t* __restrict__ kc,
                                                                 const bf16_t* __restrict__ vc, bf16_t* __restrict__ out, long ldo, int Tq,
                                                                 int pos0, int heads, int kv_heads, long kv_row, long kv_batch, int b0,
                                                                 float scaling, int nqb, int n_groups, const int* __restrict__ starts) {
  lia_attn_prefill128_body<POST_SCALE, PADDED, 1>(q, ldq, kc, vc, out, ldo, Tq, pos0, heads, kv_heads, kv_row, kv_batch, b0, scaling, nqb, n_groups, starts);
}


// ---------------------------------------------------------------------------------------------
// decode (T == 1): one workgroup per (batch row, KV head); KV-bandwidth bound.  The G = heads / kv_heads query
// heads that share a KV head (grouped-query attention; G = 1 for OPT) are served together, so every K/V row is
// read from HBM once.  LPK = D/8 lanes share one key row (16 bytes each); scores are parked in LDS, then every
// thread accumulates its 8 output dims over its share of the keys and the shares are combined through LDS.
// ---------------------------------------------------------------------------------------------
// a 16-byte load of cache rows that are read once per step: non-temporal, so the stream does not push q, the scores' neighbours
// and the next kernel's operands out of L2 (tools/stream_bench: a once-read stream runs 6.7 TB/s with nt against 6.0 without)
__device__ __forceinline__ uint4 lia_ldg_stream(const bf16_t* p) {
  const u32x4 v = __builtin_nontemporal_load((const u32x4*)p);
  return uint4{v[0], v[1], v[2], v[3]};
}

template <int CTRL> __device__ __forceinline__ float dpp_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

// The softmax of a decode-shaped row, shared by the one-workgroup kernel and the split-key route (lia_attn_split_softmax_kernel) so
// that m, l and P are the same bits on both: e = exp(s - m) with the row maximum m; l summed by thread j % 256 over its keys in
// order, then over the wave, then over the four waves left to right; P = bf16(e / l).
//   load(j): the bf16-rounded score of key j;  store(j, e): where the caller keeps e (the split route recomputes it instead)
template <typename Load, typename Store>
__device__ __forceinline__ float lia_attn_exp_sum(int tid, int S, float m, Load load, Store store) {
  float ls = 0.f;
  for (int j = tid; j < S; j += 256) {
    float e = __expf(load(j) - m);
    store(j, e);
    ls += e;
  }
  return wave_sum(ls);
}
__device__ __forceinline__ float lia_attn_fold_waves(const float* w) { return w[0] + w[1] + w[2] + w[3]; }
__device__ __forceinline__ float lia_attn_prob(float e, float l) { return rbf(e / l); }

// PADDED: the row's keys are kstart .. Sp - 1 (kstart = starts[b] <= the query's position Sp - 1): the keys of a sequence of Sp - kstart
// tokens starting at kstart, as in the prefill kernels -- the key loop starts at kstart, no key below it is read.
// starts: per served row b (the caller passes its table + b0); PADDED = 0 never reads it
template <int D, int G, int PADDED>
__global__ __launch_bounds__(256) void lia_attn_decode_kernel(const bf16_t* __restrict__ q, long ldq, const bf16_t* __restrict__ kc,
                                                               const bf16_t* __restrict__ vc, bf16_t* __restrict__ out, long ldo, int Sp,
                                                               int heads, int kv_heads, int Bc, int b0, float scaling, int post_scale,
                                                               const int* __restrict__ starts) {
  constexpr int LPK = D / 8;          // lanes per key
  constexpr int KPP = 256 / LPK;      // keys per pass of the workgroup
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int kstart = PADDED ? __builtin_amdgcn_readfirstlane(starts[blockIdx.y]) : 0;   // (uniform: keeps the row start scalar)
  const int S = Sp - kstart;
  const int Spad = (S + 3) & ~3;
  float* sc = (float*)smem;                                   // [G][Spad] scores -> probabilities
  float* red = sc + (size_t)G * Spad;                         // [4 waves][G][D] partial outputs
  float* scratch = red + (size_t)4 * G * D;                   // [G][8]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kh = blockIdx.x, b = blockIdx.y;
  const long kv_row = (long)Bc * kv_heads * D;
  const bf16_t* kbase = kc + ((long)(b0 + b) * kv_heads + kh) * D + (long)kstart * kv_row;
  const bf16_t* vbase = vc + ((long)(b0 + b) * kv_heads + kh) * D + (long)kstart * kv_row;
  const float qscale = post_scale ? 1.0f : scaling;
  const int sub = tid % LPK, kslot = tid / LPK;

  // the (scaled, bf16-rounded) query slice of each head of the group as packed bf16 pairs: q . k runs on v_dot2c_f32_bf16,
  // two products per instruction and no unpacking of the key (the products of two bf16 are exact in fp32 either way; the
  // sum is rounded to bf16 right after): Llama-3-8B's grouped decode attention 119.6 -> 114.5 us per layer.  (Requesting
  // the next pass's rows before multiplying this pass's was tried too: 122 us -- four workgroups per CU already overlap.)
  typedef __attribute__((ext_vector_type(2))) __bf16 lia_bf16x2;
  uint32_t qp[G][4];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    uint4 v = *(const uint4*)(q + (long)b * ldq + (long)(kh * G + g) * D + 8 * sub);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) qp[g][j] = pack_bf16x2(bf2f(w[j] & 0xffff) * qscale, bf2f(w[j] >> 16) * qscale);
  }
  float lmax[G];
#pragma unroll
  for (int g = 0; g < G; ++g) lmax[g] = -INFINITY;
  constexpr int U = 8;   // key rows in flight per thread: KV reads are the whole cost, keep several 16-byte loads outstanding (4 -> 8: +2 % on Llama-3-8B decode)
  // One pass = U * KPP = 128 keys, every row of it requested before the first is used.  Full passes carry no bounds checks; the
  // last pass (S = prompt + 1 + step sits just behind a multiple of 128 for every usual prompt length: 1 ... 32 real keys) requests
  // only the rows that exist -- r03 clamped its other ~100 slots onto row S - 1, a hundred requests for one row per workgroup
  // (L2 hits, but 1/3 more requests at S = 257).  r04, OPT-30B decode: 83.3 -> 80.0 us.
  auto k_pass = [&](const int j0, auto tail) {
    constexpr bool TAIL = decltype(tail)::value;
    uint4 kv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * KPP + kslot;
      if constexpr (TAIL) {
        kv[u] = uint4{0u, 0u, 0u, 0u};
        if (j < S) kv[u] = lia_ldg_stream(kbase + (long)j * kv_row + 8 * sub);
      } else {
        kv[u] = lia_ldg_stream(kbase + (long)j * kv_row + 8 * sub);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * KPP + kslot;
      const uint32_t w[4] = {kv[u].x, kv[u].y, kv[u].z, kv[u].w};
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          a = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(lia_bf16x2, qp[g][e]), __builtin_bit_cast(lia_bf16x2, w[e]), a, false);
        if constexpr (LPK == 16) {
          // the 16 lanes of a key are one DPP row: the sum over them with row rotations / quad permutes as VALU operand
          // modifiers instead of four ds_bpermute_b32 per value (PMC, Llama-3-8B B 128: the LDS pipe was ~77 % busy with them).
          // Rotating by 8 and 4 instead of xor 8, 4 picks a partner that holds the same partial (same lane index mod 8 resp.
          // mod 4), so every lane still ends with ((p_l + p_l^8) + (p_l^4 + p_l^12)) + ...: the bits of the xor butterfly.
          a += dpp_f32<0x128>(a);     // row_ror:8
          a += dpp_f32<0x124>(a);     // row_ror:4
          a += dpp_f32<0x4E>(a);      // quad_perm:[2,3,0,1]  (xor 2)
          a += dpp_f32<0xB1>(a);      // quad_perm:[1,0,3,2]  (xor 1)
        } else {
#pragma unroll
          for (int o = LPK / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        }
        if (!TAIL || j < S) {
          float sv = rbf(a);
          if (post_scale) sv = rbf(sv * scaling);
          if (sub == 0) sc[g * Spad + j] = sv;
          lmax[g] = fmaxf(lmax[g], sv);
        }
      }
    }
  };
  const int s_full = S - S % (U * KPP);
  for (int j0 = 0; j0 < s_full; j0 += U * KPP) k_pass(j0, std::false_type{});
  if (s_full < S) k_pass(s_full, std::true_type{});
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float m = wave_max(lmax[g]);
    if (lane == 0) scratch[g * 8 + wave] = m;
  }
  __syncthreads();
  float mrow[G], lrow[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    mrow[g] = fmaxf(fmaxf(scratch[g * 8], scratch[g * 8 + 1]), fmaxf(scratch[g * 8 + 2], scratch[g * 8 + 3]));
    const float ls = lia_attn_exp_sum(tid, S, mrow[g], [&](int j) { return sc[g * Spad + j]; }, [&](int j, float e) { sc[g * Spad + j] = e; });
    if (lane == 0) scratch[g * 8 + 4 + wave] = ls;
  }
  __syncthreads();
#pragma unroll
  for (int g = 0; g < G; ++g) lrow[g] = lia_attn_fold_waves(scratch + g * 8 + 4);
  // probabilities once per (head, key) -- bf16(e / l), the reference's rounding point -- instead of once per lane of the
  // key in the P.V loop below (LPK lanes would each repeat the division)
#pragma unroll
  for (int g = 0; g < G; ++g)
    for (int j = tid; j < S; j += 256) sc[g * Spad + j] = lia_attn_prob(sc[g * Spad + j], lrow[g]);
  __syncthreads();

  float o[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int e = 0; e < 8; ++e) o[g][e] = 0.f;
  auto v_pass = [&](const int j0, auto tail) {
    constexpr bool TAIL = decltype(tail)::value;
    uint4 vv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if constexpr (TAIL) {
        vv[u] = uint4{0u, 0u, 0u, 0u};
        if (j0 + u * KPP < S) vv[u] = lia_ldg_stream(vbase + (long)(j0 + u * KPP) * kv_row + 8 * sub);
      } else {
        vv[u] = lia_ldg_stream(vbase + (long)(j0 + u * KPP) * kv_row + 8 * sub);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * KPP;
      if (!TAIL || j < S) {
        const uint32_t w[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float p = sc[g * Spad + j];
#pragma unroll
          for (int e = 0; e < 4; ++e) { o[g][2 * e] += p * bf2f(w[e] & 0xffff); o[g][2 * e + 1] += p * bf2f(w[e] >> 16); }
        }
      }
    }
  };
  for (int j0 = 0; j0 < s_full; j0 += U * KPP) v_pass(j0 + kslot, std::false_type{});
  if (s_full < S) v_pass(s_full + kslot, std::true_type{});
  // the key slots of one wave are folded with shuffles (a [KPP][G][D] LDS slab would cap the CU at three workgroups;
  // with [4][G][D] a B = 128, 8-kv-head launch is resident in one round), then the four waves through LDS
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = o[g][e];
#pragma unroll
      for (int off = LPK; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
      o[g][e] = v;
    }
  if (lane < LPK) {
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int e = 0; e < 8; ++e) red[((size_t)wave * G + g) * D + 8 * sub + e] = o[g][e];
  }
  __syncthreads();
  for (int idx = tid; idx < G * D; idx += 256) {
    const int g = idx / D, dd = idx - g * D;
    const float acc = (red[(size_t)g * D + dd] + red[((size_t)G + g) * D + dd]) +
                      (red[((size_t)2 * G + g) * D + dd] + red[((size_t)3 * G + g) * D + dd]);
    out[(long)b * ldo + (long)(kh * G + g) * D + dd] = f2bf(acc);
  }
}

// The d = 128 kernels' grid (prefill and append alike): nqb query-block slots per (row, head), the workgroup order, the grid size.
struct LiaGrid128 { long hd; int nqb, n_groups; unsigned nwg; };   // nwg == 0: the cache is beyond the 32-bit staging offsets
static LiaGrid128 grid128_of(int B, int T, int heads, int kv_heads, int Bc) {
  LiaGrid128 g{(long)kv_heads * 128, 0, B * kv_heads, 0};
  // (a token-major [B][T][h][d] K/V -- strides (hd, T hd) -- was measured: same time, so the cache layout stays)
#ifdef LIA_ATTN_NO_PAIRS
  g.nqb = (T + 127) / 128;
#else
  g.nqb = ((T + 127) / 128 + 1) / 2;        // two query blocks per workgroup: bx and its mirror image (see the kernel)
#endif
  // the staging addresses hold (row within a 64-key tile) x (bytes per key row) + chunk in 32 bits: 64 Bc hd 2 < 2^32, i.e. a
  // cache batch x hidden of < 3.3e7 elements per key row (OPT-175B at Bc = 2048 is 2.5e7)
  if ((long)Bc * g.hd * 2 * 64 + 256 >= (1L << 32)) return g;
  // the XCD-aware order when the groups spread evenly over the 8 XCDs (a multiple of 8, or so many that the remainder does not
  // matter); otherwise r05's order, which deals single workgroups round-robin (2 rows x 2 KV heads would use 4 XCDs of 8)
  bool xcd_order = (g.n_groups % 8 == 0) || g.n_groups >= 64;
#ifdef LIA_ATTN_LEGACY_GRID
  xcd_order = false;
#endif
  g.nwg = xcd_order ? (unsigned)(((g.n_groups + 7) / 8) * 8 * g.nqb * (heads / kv_heads)) : (unsigned)(g.nqb * heads * B);
  if (!xcd_order) g.n_groups = 0;
  return g;
}

// starts == nullptr: the unpadded kernels; otherwise their PADDED instantiations with the row starts starts[0 .. B - 1]
// (device memory, 0 <= starts[b] <= T - 1)
static int prefill_launch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B, int T,
                          int heads, int kv_heads, int d, int Bc, int b0, int post_scale, const int* starts, hipStream_t st) {
  if (B <= 0 || T <= 0) return 0;
  if (kv_heads <= 0 || heads % kv_heads) return -1;
  dim3 grid((T + 127) / 128, heads, B);
  const float scaling = 1.0f / sqrtf((float)d);
  switch (d) {
    case 128: {
      const LiaGrid128 g = grid128_of(B, T, heads, kv_heads, Bc);
      if (!g.nwg) return -1;
      if (starts) {
        if (post_scale) hipLaunchKernelGGL(lia_attn_prefill128_padded_kernel<1>, dim3(g.nwg), dim3(256), 0, st, q, ldq, kc, vc, out, ldo, T, heads, kv_heads, (long)Bc * g.hd, g.hd, b0, scaling, g.nqb, g.n_groups, starts);
        else hipLaunchKernelGGL(lia_attn_prefill128_padded_kernel<0>, dim3(g.nwg), dim3(256), 0, st, q, ldq, kc, vc, out, ldo, T, heads, kv_heads, (long)Bc * g.hd, g.hd, b0, scaling, g.nqb, g.n_groups, starts);
        break;
      }
      if (post_scale) hipLaunchKernelGGL(lia_attn_prefill128_kernel<1>, dim3(g.nwg), dim3(256), 0, st, q, ldq, kc, vc, out, ldo, T, heads, kv_heads, (long)Bc * g.hd, g.hd, b0, scaling, g.nqb, g.n_groups);
      else hipLaunchKernelGGL(lia_attn_prefill128_kernel<0>, dim3(g.nwg), dim3(256), 0, st, q, ldq, kc, vc, out, ldo, T, heads, kv_heads, (long)Bc * g.hd, g.hd, b0, scaling, g.nqb, g.n_groups);
      break;
    }
    case 64:
      if (starts) hipLaunchKernelGGL((lia_attn_prefill_kernel<64, 1>), grid, dim3(256), 0, st, q, ldq, kc, vc, out, ldo, T, heads, kv_heads, Bc, b0, scaling, post_scale, starts);
      else hipLaunchKernelGGL((lia_attn_prefill_kernel<64, 0>), grid, dim3(256), 0, st, q, ldq, kc, vc, out, ldo, T, heads, kv_heads, Bc, b0, scaling, post_scale, nullptr);
      break;
    case 32:
      if (starts) hipLaunchKernelGGL((lia_attn_prefill_kernel<32, 1>), grid, dim3(256), 0, st, q, ldq, kc, vc, out, ldo, T, heads, kv_heads, Bc, b0, scaling, post_scale, starts);
      else hipLaunchKernelGGL((lia_attn_prefill_kernel<32, 0>), grid, dim3(256), 0, st, q, ldq, kc, vc, out, ldo, T, heads, kv_heads, Bc, b0, scaling, post_scale, nullptr);
      break;
    default: return -1;
  }
  return 0;
}

extern "C" int lia_attn_prefill_launch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B, int T,
                                       int heads, int kv_heads, int d, int Bc, int b0, int post_scale, hipStream_t st) {
  return prefill_launch(q, ldq, kc, vc, out, ldo, B, T, heads, kv_heads, d, Bc, b0, post_scale, nullptr, st);
}

// left-padded rows (the reference's CPU branch with an HF padding mask, lia/modeling_opt.py:1133 + mha_fusion.py:532-566):
// served row b's query i >= starts[b] attends keys starts[b] .. i; rows i < starts[b] are zeros.  starts: device, B entries.
extern "C" int lia_attn_prefill_padded_launch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B,
                                              int T, int heads, int kv_heads, int d, int Bc, int b0, int post_scale, const int* starts, hipStream_t st) {
  if (!starts) return -1;
  return prefill_launch(q, ldq, kc, vc, out, ldo, B, T, heads, kv_heads, d, Bc, b0, post_scale, starts, st);
}

// A block of T queries at cache positions pos0 .. pos0 + T - 1 of every served row, over the keys starts[b] (or 0) .. pos0 + T - 1 that the
// cache already holds (the block's own K / V rows included).  q / out: [B][T][heads * d] with pitches ldq / ldo, the block's rows only.
// starts: device, B entries, each <= pos0 -- or NULL.  Row t of the result is bit for bit row pos0 + t of the prefill launch over
// pos0 + T tokens with the same q rows and cache (see lia_attn_prefill_kernel).  Grids, orders and the d = 128 limit are the prefill launcher's.
extern "C" int lia_attn_append_launch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B, int T,
                                      int pos0, int heads, int kv_heads, int d, int Bc, int b0, int post_scale, const int* starts,
                                      hipStream_t st) {
  if (B <= 0 || T <= 0) return 0;
  if (pos0 < 0 || kv_heads <= 0 || heads % kv_heads) return -1;
  dim3 grid((T + 127) / 128, heads, B);
  const float scaling = 1.0f / sqrtf((float)d);
  switch (d) {
    case 128: {
      const LiaGrid128 g = grid128_of(B, T, heads, kv_heads, Bc);
      if (!g.nwg) return -1;
#define LIA_APP128(PS, PD) hipLaunchKernelGGL((lia_attn_append128_kernel<PS, PD>), dim3(g.nwg), dim3(256), 0, st, q, ldq, kc, vc, out, ldo, T, pos0, heads, kv_heads, (long)Bc * g.hd, g.hd, b0, scaling, g.nqb, g.n_groups, starts)
      if (starts) { if (post_scale) LIA_APP128(1, 1); else LIA_APP128(0, 1); }
      else { if (post_scale) LIA_APP128(1, 0); else LIA_APP128(0, 0); }
#undef LIA_APP128
      break;
    }
    case 64:
      if (starts) hipLaunchKernelGGL((lia_attn_prefill_kernel<64, 1, int>), grid, dim3(256), 0, st, q, ldq, kc, vc, out, ldo, T, heads, kv_heads, Bc, b0, scaling, post_scale, starts, pos0);
      else hipLaunchKernelGGL((lia_attn_prefill_kernel<64, 0, int>), grid, dim3(256), 0, st, q, ldq, kc, vc, out, ldo, T, heads, kv_heads, Bc, b0, scaling, post_scale, (const int*)nullptr, pos0);
      break;
    case 32:
      if (starts) hipLaunchKernelGGL((lia_attn_prefill_kernel<32, 1, int>), grid, dim3(256), 0, st, q, ldq, kc, vc, out, ldo, T, heads, kv_heads, Bc, b0, scaling, post_scale, starts, pos0);
      else hipLaunchKernelGGL((lia_attn_prefill_kernel<32, 0, int>), grid, dim3(256), 0, st, q, ldq, kc, vc, out, ldo, T, heads, kv_heads, Bc, b0, scaling, post_scale, (const int*)nullptr, pos0);
      break;
    default: return -1;
  }
  return 0;
}

template <int D>
static int launch_decode(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B, int S, int heads,
                         int kv_heads, int Bc, int b0, float scaling, int post_scale, const int* starts, hipStream_t st) {
  const int G = heads / kv_heads;
  dim3 grid(kv_heads, B);
  const int Spad = (S + 3) & ~3;
  size_t lds = ((size_t)G * Spad + (size_t)4 * G * D + (size_t)G * 8) * sizeof(float);
  if (lds > 160 * 1024) return -1;
#define LIA_DEC(GV)                                                                                                            \
  if (starts) {                                                                                                                \
    static bool attr = false;                                                                                                  \
    if (!attr) { (void)hipFuncSetAttribute((const void*)lia_attn_decode_kernel<D, GV, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr = true; } \
    hipLaunchKernelGGL((lia_attn_decode_kernel<D, GV, 1>), grid, dim3(256), lds, st, q, ldq, kc, vc, out, ldo, S, heads, kv_heads, Bc, b0, scaling, post_scale, starts); \
  } else {                                                                                                                     \
    static bool attr = false;                                                                                                  \
    if (!attr) { (void)hipFuncSetAttribute((const void*)lia_attn_decode_kernel<D, GV, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr = true; } \
    hipLaunchKernelGGL((lia_attn_decode_kernel<D, GV, 0>), grid, dim3(256), lds, st, q, ldq, kc, vc, out, ldo, S, heads, kv_heads, Bc, b0, scaling, post_scale, nullptr); \
  }
  switch (G) {
    case 1: LIA_DEC(1) break;
    case 2: LIA_DEC(2) break;
    case 4: LIA_DEC(4) break;
    case 8: LIA_DEC(8) break;
    default: return -1;
  }
#undef LIA_DEC
  return 0;
}

static int decode_launch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B, int S, int heads,
                         int kv_heads, int d, int Bc, int b0, int post_scale, const int* starts, hipStream_t st) {
  if (B <= 0 || S <= 0) return 0;
  if (kv_heads <= 0 || heads % kv_heads) return -1;
  const float scaling = 1.0f / sqrtf((float)d);
  switch (d) {
    case 128: return launch_decode<128>(q, ldq, kc, vc, out, ldo, B, S, heads, kv_heads, Bc, b0, scaling, post_scale, starts, st);
    case 64: return launch_decode<64>(q, ldq, kc, vc, out, ldo, B, S, heads, kv_heads, Bc, b0, scaling, post_scale, starts, st);
    case 32: return launch_decode<32>(q, ldq, kc, vc, out, ldo, B, S, heads, kv_heads, Bc, b0, scaling, post_scale, starts, st);
    default: return -1;
  }
}

extern "C" int lia_attn_decode_launch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B, int S,
                                      int heads, int kv_heads, int d, int Bc, int b0, int post_scale, hipStream_t st) {
  return decode_launch(q, ldq, kc, vc, out, ldo, B, S, heads, kv_heads, d, Bc, b0, post_scale, nullptr, st);
}

// one query per served row at position S - 1 over keys starts[b] .. S - 1 (starts: device, B entries, each <= S - 1)
extern "C" int lia_attn_decode_padded_launch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B,
                                             int S, int heads, int kv_heads, int d, int Bc, int b0, int post_scale, const int* starts, hipStream_t st) {
  if (!starts) return -1;
  return decode_launch(q, ldq, kc, vc, out, ldo, B, S, heads, kv_heads, d, Bc, b0, post_scale, starts, st);
}

// ---------------------------------------------------------------------------------------------
// split-key decode (T == 1): the decode kernel's arithmetic with a row's keys cut into chunks of C keys, counted from the row's own
// first key, and one workgroup per (chunk, KV head, batch row) -- no LDS that grows with S, and a grid that fills the chip at small
// batches.  Four launches, every cross-workgroup dependency a kernel boundary (the per-XCD L2s are not coherent inside a launch):
//   scores   (chunks, kv_heads, B)  s = bf16(q . k) [bf16(. scaling)] with the decode kernel's key pass -> scratch, bf16
//                                   [row][head][Spad], and the chunk's maximum [row][head][chunk]
//   softmax  (heads, B)             m over the chunk maxima, l in the decode kernel's order (lia_attn_exp_sum), the scores rewritten
//                                   in place as P = bf16(exp(s - m) / l): 2 S bytes per head, served from L2
//   pv       (chunks, kv_heads, B)  the chunk's P staged in LDS, the decode kernel's V pass and folds -> fp32 partial
//                                   [chunk][row][head][D]
//   combine                         the partials added in chunk order, bf16 through ldo.  No floating-point atomics anywhere.
// Scores, m, l and P are bit for bit the one-workgroup kernel's; only the fp32 order of the P.V sum differs, and within a chunk the
// keys keep that kernel's thread assignment and fold order (C is a multiple of its pass of U * KPP keys), so a row of S <= C keys
// is the one-workgroup launch bit for bit.  A row's result depends on its own q, keys, S and C alone: not on B, b0, Bc or the other
// rows; a padded row (keys from kstart = starts[b]) is the unpadded launch of its shifted sequence.
// ---------------------------------------------------------------------------------------------
// C per head_dim: a multiple of the pass (128 / 256 / 512 keys at d = 128 / 64 / 32), the smallest candidate of tools/attn_split_bench's
// sweep over 256 / 512 / 1024 at every d: the route serves launches of few workgroups, where more chunks win up to S ~ 8k at B = 1
// (Llama-3-8B heads, B 1, S 4096: 33.9 / 39.2 / 53.2 us); a larger C wins by 5 - 15 % from B x S ~ 32k on (results/attn_split_bench.txt).
extern "C" int lia_attn_split_chunk(int d) {
  switch (d) {
    case 128: return 256;
    case 64: return 256;
    case 32: return 512;
    default: return 0;
  }
}

static int split_pass(int d) { return 8 * (256 / (d / 8)); }

struct LiaSplitPlan { int nch, Spad; size_t scores, cmax, part, total; };   // byte offsets into the scratch, each 256-aligned
static LiaSplitPlan split_plan(int B, int S, int heads, int d, int chunk) {
  LiaSplitPlan p;
  p.nch = (S + chunk - 1) / chunk;
  p.Spad = p.nch * chunk;
  size_t at = 0;
  auto take = [&](size_t bytes) { size_t o = at; at = align_up(at + bytes, 256); return o; };
  p.scores = take((size_t)B * heads * p.Spad * 2);
  p.cmax = take((size_t)B * heads * p.nch * 4);
  p.part = take((size_t)p.nch * B * heads * d * 4);
  p.total = at;
  return p;
}

static size_t split_scratch_bytes(int B, int S, int heads, int kv_heads, int d, int chunk) {
  if (B <= 0 || S <= 0 || heads <= 0 || kv_heads <= 0 || heads % kv_heads || !(d == 32 || d == 64 || d == 128)) return 0;
  if (chunk <= 0 || chunk % split_pass(d)) return 0;
  return split_plan(B, S, heads, d, chunk).total;
}

// pure host arithmetic: the scratch lia_attn_decode_split_launch needs for B rows of S keys (0: a shape it refuses)
extern "C" size_t lia_attn_split_scratch_bytes(int B, int S, int heads, int kv_heads, int d) {
  return split_scratch_bytes(B, S, heads, kv_heads, d, lia_attn_split_chunk(d));
}
extern "C" size_t lia_attn_split_scratch_bytes_chunk(int B, int S, int heads, int kv_heads, int d, int chunk) {
  return split_scratch_bytes(B, S, heads, kv_heads, d, chunk);
}

// sc: [B][heads][Spad] bf16 scores; cmax: [B][heads][nch].  C: keys per chunk
template <int D, int G, int PADDED>
__global__ __launch_bounds__(256) void lia_attn_split_scores_kernel(const bf16_t* __restrict__ q, long ldq, const bf16_t* __restrict__ kc,
                                                                     bf16_t* __restrict__ sc, float* __restrict__ cmax, int Sp, int heads,
                                                                     int kv_heads, int Bc, int b0, float scaling, int post_scale,
                                                                     const int* __restrict__ starts, int C, int nch, int Spad) {
  constexpr int LPK = D / 8;          // lanes per key
  constexpr int KPP = 256 / LPK;      // keys per pass of the workgroup
  constexpr int U = 8;
  __shared__ float wmax[G * 4];
  const int c = blockIdx.x, kh = blockIdx.y, b = blockIdx.z;
  const int kstart = PADDED ? __builtin_amdgcn_readfirstlane(starts[b]) : 0;
  const int c0 = c * C;
  if (c0 >= Sp - kstart) return;     // a padded row of fewer chunks than the longest row (uniform over the workgroup)
  const int S = min(C, Sp - kstart - c0);   // the keys of this chunk: c0 .. c0 + S - 1 of the row
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long kv_row = (long)Bc * kv_heads * D;
  const bf16_t* kbase = kc + ((long)(b0 + b) * kv_heads + kh) * D + (long)(kstart + c0) * kv_row;
  bf16_t* srow = sc + ((long)b * heads + (long)kh * G) * Spad + c0;
  const float qscale = post_scale ? 1.0f : scaling;
  const int sub = tid % LPK, kslot = tid / LPK;

  typedef __attribute__((ext_vector_type(2))) __bf16 lia_bf16x2;
  uint32_t qp[G][4];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    uint4 v = *(const uint4*)(q + (long)b * ldq + (long)(kh * G + g) * D + 8 * sub);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) qp[g][j] = pack_bf16x2(bf2f(w[j] & 0xffff) * qscale, bf2f(w[j] >> 16) * qscale);
  }
  float lmax[G];
#pragma unroll
  for (int g = 0; g < G; ++g) lmax[g] = -INFINITY;
  // the decode kernel's key pass (U * KPP keys, every row requested before the first is used; the tail requests only rows that exist)
  auto k_pass = [&](const int j0, auto tail) {
    constexpr bool TAIL = decltype(tail)::value;
    uint4 kv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * KPP + kslot;
      if constexpr (TAIL) {
        kv[u] = uint4{0u, 0u, 0u, 0u};
        if (j < S) kv[u] = lia_ldg_stream(kbase + (long)j * kv_row + 8 * sub);
      } else {
        kv[u] = lia_ldg_stream(kbase + (long)j * kv_row + 8 * sub);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * KPP + kslot;
      const uint32_t w[4] = {kv[u].x, kv[u].y, kv[u].z, kv[u].w};
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          a = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(lia_bf16x2, qp[g][e]), __builtin_bit_cast(lia_bf16x2, w[e]), a, false);
        if constexpr (LPK == 16) {
          a += dpp_f32<0x128>(a);     // row_ror:8   (the decode kernel's butterfly)
          a += dpp_f32<0x124>(a);     // row_ror:4
          a += dpp_f32<0x4E>(a);      // quad_perm:[2,3,0,1]  (xor 2)
          a += dpp_f32<0xB1>(a);      // quad_perm:[1,0,3,2]  (xor 1)
        } else {
#pragma unroll
          for (int o = LPK / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        }
        if (!TAIL || j < S) {
          float sv = rbf(a);
          if (post_scale) sv = rbf(sv * scaling);
          if (sub == 0) srow[(long)g * Spad + j] = f2bf(sv);   // (exact: sv is a bf16 value)
          lmax[g] = fmaxf(lmax[g], sv);
        }
      }
    }
  };
  const int s_full = S - S % (U * KPP);
  for (int j0 = 0; j0 < s_full; j0 += U * KPP) k_pass(j0, std::false_type{});
  if (s_full < S) k_pass(s_full, std::true_type{});
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float m = wave_max(lmax[g]);
    if (lane == 0) wmax[g * 4 + wave] = m;
  }
  __syncthreads();
  if (tid < G)
    cmax[((long)b * heads + (long)kh * G + tid) * nch + c] = fmaxf(fmaxf(wmax[tid * 4], wmax[tid * 4 + 1]), fmaxf(wmax[tid * 4 + 2], wmax[tid * 4 + 3]));
}

// one workgroup per (head, row): the head group's G rows are independent here, so each gets a workgroup of its own
template <int PADDED>
__global__ __launch_bounds__(256) void lia_attn_split_softmax_kernel(bf16_t* __restrict__ sc, const float* __restrict__ cmax, int Sp, int heads,
                                                                      const int* __restrict__ starts, int C, int nch, int Spad) {
  __shared__ float red[8];
  const int h = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kstart = PADDED ? __builtin_amdgcn_readfirstlane(starts[b]) : 0;
  const int S = Sp - kstart;
  const int n = (S + C - 1) / C;     // the row's own chunks
  bf16_t* s = sc + ((long)b * heads + h) * Spad;
  const float* cm = cmax + ((long)b * heads + h) * nch;
  float m = -INFINITY;
  for (int c = tid; c < n; c += 256) m = fmaxf(m, cm[c]);
  m = wave_max(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const float ls = lia_attn_exp_sum(tid, S, m, [&](int j) { return bf2f(s[j]); }, [](int, float) {});
  if (lane == 0) red[4 + wave] = ls;
  __syncthreads();
  const float l = lia_attn_fold_waves(red + 4);
  // (e is computed again rather than kept: the same operation on the same bits, and the scratch stays 2 bytes per score)
  for (int j = tid; j < S; j += 256) s[j] = f2bf(lia_attn_prob(__expf(bf2f(s[j]) - m), l));
}

// part: [nch][B][heads][D] fp32, part_stride = B * heads * D
template <int D, int G, int PADDED>
__global__ __launch_bounds__(256) void lia_attn_split_pv_kernel(const bf16_t* __restrict__ sc, const bf16_t* __restrict__ vc,
                                                                 float* __restrict__ part, int Sp, int heads, int kv_heads, int Bc, int b0,
                                                                 const int* __restrict__ starts, int C, int Spad, long part_stride) {
  constexpr int LPK = D / 8;
  constexpr int KPP = 256 / LPK;
  constexpr int U = 8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* p = (float*)smem;                    // [G][C] the chunk's probabilities
  float* red = p + (size_t)G * C;             // [4 waves][G][D] partial outputs
  const int c = blockIdx.x, kh = blockIdx.y, b = blockIdx.z;
  const int kstart = PADDED ? __builtin_amdgcn_readfirstlane(starts[b]) : 0;
  const int c0 = c * C;
  if (c0 >= Sp - kstart) return;
  const int S = min(C, Sp - kstart - c0);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long kv_row = (long)Bc * kv_heads * D;
  const bf16_t* vbase = vc + ((long)(b0 + b) * kv_heads + kh) * D + (long)(kstart + c0) * kv_row;
  const bf16_t* srow = sc + ((long)b * heads + (long)kh * G) * Spad + c0;
  const int sub = tid % LPK, kslot = tid / LPK;
#pragma unroll
  for (int g = 0; g < G; ++g)
    for (int j = tid; j < S; j += 256) p[g * C + j] = bf2f(srow[(long)g * Spad + j]);
  __syncthreads();

  float o[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int e = 0; e < 8; ++e) o[g][e] = 0.f;
  // the decode kernel's V pass and folds on the chunk
  auto v_pass = [&](const int j0, auto tail) {
    constexpr bool TAIL = decltype(tail)::value;
    uint4 vv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if constexpr (TAIL) {
        vv[u] = uint4{0u, 0u, 0u, 0u};
        if (j0 + u * KPP < S) vv[u] = lia_ldg_stream(vbase + (long)(j0 + u * KPP) * kv_row + 8 * sub);
      } else {
        vv[u] = lia_ldg_stream(vbase + (long)(j0 + u * KPP) * kv_row + 8 * sub);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * KPP;
      if (!TAIL || j < S) {
        const uint32_t w[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float pj = p[g * C + j];
#pragma unroll
          for (int e = 0; e < 4; ++e) { o[g][2 * e] += pj * bf2f(w[e] & 0xffff); o[g][2 * e + 1] += pj * bf2f(w[e] >> 16); }
        }
      }
    }
  };
  const int s_full = S - S % (U * KPP);
  for (int j0 = 0; j0 < s_full; j0 += U * KPP) v_pass(j0 + kslot, std::false_type{});
  if (s_full < S) v_pass(s_full + kslot, std::true_type{});
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = o[g][e];
#pragma unroll
      for (int off = LPK; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
      o[g][e] = v;
    }
  if (lane < LPK) {
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int e = 0; e < 8; ++e) red[((size_t)wave * G + g) * D + 8 * sub + e] = o[g][e];
  }
  __syncthreads();
  float* prow = part + (long)c * part_stride + ((long)b * heads + (long)kh * G) * D;
  for (int idx = tid; idx < G * D; idx += 256) {
    const int g = idx / D, dd = idx - g * D;
    prow[idx] = (red[(size_t)g * D + dd] + red[((size_t)G + g) * D + dd]) + (red[((size_t)2 * G + g) * D + dd] + red[((size_t)3 * G + g) * D + dd]);
  }
}

// hd = heads * D values per row; a thread per output value adds its partials in chunk order
template <int PADDED>
__global__ __launch_bounds__(256) void lia_attn_split_combine_kernel(const float* __restrict__ part, bf16_t* __restrict__ out, long ldo, int Sp,
                                                                      int hd, const int* __restrict__ starts, int C, long part_stride) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= part_stride) return;
  const int b = (int)(idx / hd);
  const int r = (int)(idx - (long)b * hd);
  const int kstart = PADDED ? starts[b] : 0;
  const int n = (Sp - kstart + C - 1) / C;
  float acc = part[idx];
  for (int c = 1; c < n; ++c) acc += part[(long)c * part_stride + idx];
  out[(long)b * ldo + r] = f2bf(acc);
}

template <int D>
static int launch_split(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B, int S, int heads,
                        int kv_heads, int Bc, int b0, float scaling, int post_scale, const int* starts, int C, char* scratch, hipStream_t st) {
  const int G = heads / kv_heads;
  const LiaSplitPlan p = split_plan(B, S, heads, D, C);
  bf16_t* sc = (bf16_t*)(scratch + p.scores);
  float* cmax = (float*)(scratch + p.cmax);
  float* part = (float*)(scratch + p.part);
  const long part_stride = (long)B * heads * D;
  const size_t lds = ((size_t)G * C + (size_t)4 * G * D) * sizeof(float);
  if (lds > 64 * 1024) return -1;
  const dim3 grid(p.nch, kv_heads, B);
#define LIA_SPLIT_PD(GV, PD)                                                                                                                       \
  hipLaunchKernelGGL((lia_attn_split_scores_kernel<D, GV, PD>), grid, dim3(256), 0, st, q, ldq, kc, sc, cmax, S, heads, kv_heads, Bc, b0, scaling, \
                     post_scale, starts, C, p.nch, p.Spad);                                                                                        \
  hipLaunchKernelGGL((lia_attn_split_softmax_kernel<PD>), dim3(heads, B), dim3(256), 0, st, sc, cmax, S, heads, starts, C, p.nch, p.Spad);         \
  hipLaunchKernelGGL((lia_attn_split_pv_kernel<D, GV, PD>), grid, dim3(256), lds, st, sc, vc, part, S, heads, kv_heads, Bc, b0, starts, C, p.Spad, \
                     part_stride);                                                                                                                 \
  hipLaunchKernelGGL((lia_attn_split_combine_kernel<PD>), dim3((unsigned)((part_stride + 255) / 256)), dim3(256), 0, st, part, out, ldo, S,        \
                     heads * D, starts, C, part_stride);
#define LIA_SPLIT(GV) if (starts) { LIA_SPLIT_PD(GV, 1) } else { LIA_SPLIT_PD(GV, 0) }
  switch (G) {
    case 1: LIA_SPLIT(1) break;
    case 2: LIA_SPLIT(2) break;
    case 4: LIA_SPLIT(4) break;
    case 8: LIA_SPLIT(8) break;
    default: return -1;
  }
#undef LIA_SPLIT
#undef LIA_SPLIT_PD
  return 0;
}

static int split_launch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B, int S, int heads,
                        int kv_heads, int d, int Bc, int b0, int post_scale, const int* starts, int chunk, void* scratch,
                        size_t scratch_bytes, hipStream_t st) {
  if (S < 1 || kv_heads <= 0 || heads <= 0 || heads % kv_heads) return -1;
  const int G = heads / kv_heads;
  if (!(G == 1 || G == 2 || G == 4 || G == 8)) return -1;
  if (B <= 0) return 0;
  const size_t need = split_scratch_bytes(B, S, heads, kv_heads, d, chunk);
  if (!need || !scratch || scratch_bytes < need || B > 65535 || kv_heads > 65535) return -1;
  const float scaling = 1.0f / sqrtf((float)d);
  switch (d) {
    case 128: return launch_split<128>(q, ldq, kc, vc, out, ldo, B, S, heads, kv_heads, Bc, b0, scaling, post_scale, starts, chunk, (char*)scratch, st);
    case 64: return launch_split<64>(q, ldq, kc, vc, out, ldo, B, S, heads, kv_heads, Bc, b0, scaling, post_scale, starts, chunk, (char*)scratch, st);
    case 32: return launch_split<32>(q, ldq, kc, vc, out, ldo, B, S, heads, kv_heads, Bc, b0, scaling, post_scale, starts, chunk, (char*)scratch, st);
    default: return -1;
  }
}

// lia_attn_decode_launch's arguments and meaning (starts: lia_attn_decode_padded_launch's, or NULL = unpadded) through the four
// launches above, for any S >= 1.  scratch: device memory of lia_attn_split_scratch_bytes(B, S, heads, kv_heads, d), owned by the
// call until the stream has passed it.  -1, nothing launched: d or heads / kv_heads not instantiated, scratch too small, S < 1.
extern "C" int lia_attn_decode_split_launch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B, int S,
                                            int heads, int kv_heads, int d, int Bc, int b0, int post_scale, const int* starts, void* scratch,
                                            size_t scratch_bytes, hipStream_t st) {
  return split_launch(q, ldq, kc, vc, out, ldo, B, S, heads, kv_heads, d, Bc, b0, post_scale, starts, lia_attn_split_chunk(d), scratch, scratch_bytes, st);
}
// the same with the chunk as an argument (a multiple of the pass; scratch of lia_attn_split_scratch_bytes_chunk): the bench's sweep
extern "C" int lia_attn_decode_split_launch_chunk(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B,
                                                  int S, int heads, int kv_heads, int d, int Bc, int b0, int post_scale, const int* starts,
                                                  int chunk, void* scratch, size_t scratch_bytes, hipStream_t st) {
  return split_launch(q, ldq, kc, vc, out, ldo, B, S, heads, kv_heads, d, Bc, b0, post_scale, starts, chunk, scratch, scratch_bytes, st);
}

// The route of a decode-shaped dispatch over S keys: 0 = the one-workgroup launch, 1 = split by LIA_OPT_SPLIT_DECODE (S > C),
// 2 = split because the one-workgroup launcher refuses the shape for LDS.  0 for shapes the split launch does not take either.
int lia_attn_split_route(int option, int S, int heads, int kv_heads, int d) {
  if (S < 1 || kv_heads <= 0 || heads <= 0 || heads % kv_heads || !(d == 32 || d == 64 || d == 128)) return 0;
  const int G = heads / kv_heads;
  if (!(G == 1 || G == 2 || G == 4 || G == 8)) return 0;
  const int Spad = (S + 3) & ~3;
  if (((size_t)G * Spad + (size_t)4 * G * d + (size_t)G * 8) * sizeof(float) > 160 * 1024) return 2;
  return option && S > lia_attn_split_chunk(d) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// block (2 <= T <= 16 queries per row behind pos0 > 0 cached positions: the verification block of speculative decoding).  The decode
// kernel, once, for the Q = G * T query slots of a (batch row, KV head): slot s = t * G + g is query t of head g of the group and
// sees keys 0 .. lim[s] - 1, lim[s] = pos0 + t + 1 - kstart.  Every K / V row is read once for all slots.  A slot keeps the decode
// kernel's assignment of keys to threads (key j: slot j % KPP of the workgroup; exp / sum: thread j % 256), its order of every sum
// and its rounding points, and only gains the limit -- so row t is bit for bit lia_attn_decode_kernel over S = pos0 + t + 1 keys with
// that query row (U, the rows in flight, batches the loads and is not part of any order).  Slots >= G * T (Q is the next
// instantiated size) have lim = 0: no key, no output.
// PADDED = 2, the ragged form (per-row acceptance of speculative decoding): row b holds lens[b] cached positions instead of pos0, and
// starts may be NULL (all zeros).  Both tables are read through readfirstlane -- a row's base length and start are wave-uniform --
// and everything below derives from S exactly as before, so row b is bit for bit the PADDED = 0 / 1 kernel of a B = 1 launch at
// pos0 = lens[b].  pos0 is then max(lens): it sized the LDS, and a table entry beyond it is clamped to it (never past the buffers).
// ---------------------------------------------------------------------------------------------
template <int D, int Q, int PADDED>
__global__ __launch_bounds__(256) void lia_attn_block_kernel(const bf16_t* __restrict__ q, long ldq, const bf16_t* __restrict__ kc,
                                                              const bf16_t* __restrict__ vc, bf16_t* __restrict__ out, long ldo, int T,
                                                              int pos0, int G, int kv_heads, int Bc, int b0, float scaling,
                                                              int post_scale, const int* __restrict__ starts,
                                                              const int* __restrict__ lens) {
  constexpr int LPK = D / 8;          // lanes per key
  constexpr int KPP = 256 / LPK;      // keys per pass of the workgroup
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int kstart, len;
  if constexpr (PADDED == 2) {
    kstart = starts ? __builtin_amdgcn_readfirstlane(starts[blockIdx.y]) : 0;
    len = min(__builtin_amdgcn_readfirstlane(lens[blockIdx.y]), pos0);
  } else {
    kstart = PADDED ? __builtin_amdgcn_readfirstlane(starts[blockIdx.y]) : 0;
    len = pos0;
  }
  const int S = len + T - kstart;           // the keys of the last query of the block
  const int Smin = S - T + 1;               // ... of the first: below it no slot needs a limit
  const int Spad = (S + 3) & ~3;
  float* sc = (float*)smem;                                   // [Q][Spad] scores -> probabilities
  float* red = sc + (size_t)Q * Spad;                         // [4 waves][Q][D] partial outputs
  float* scratch = red + (size_t)4 * Q * D;                   // [Q][8]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kh = blockIdx.x, b = blockIdx.y;
  const long kv_row = (long)Bc * kv_heads * D;
  const bf16_t* kbase = kc + ((long)(b0 + b) * kv_heads + kh) * D + (long)kstart * kv_row;
  const bf16_t* vbase = vc + ((long)(b0 + b) * kv_heads + kh) * D + (long)kstart * kv_row;
  const float qscale = post_scale ? 1.0f : scaling;
  const int sub = tid % LPK, kslot = tid / LPK;
  const int n_slots = G * T;

  typedef __attribute__((ext_vector_type(2))) __bf16 lia_bf16x2;
  int lim[Q];
  uint32_t qp[Q][4];
#pragma unroll
  for (int s = 0; s < Q; ++s) {
    const int t = s / G, g = s - t * G;
    lim[s] = s < n_slots ? Smin + t : 0;
    uint4 v = uint4{0u, 0u, 0u, 0u};
    if (s < n_slots) v = *(const uint4*)(q + ((long)b * T + t) * ldq + (long)(kh * G + g) * D + 8 * sub);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) qp[s][j] = pack_bf16x2(bf2f(w[j] & 0xffff) * qscale, bf2f(w[j] >> 16) * qscale);
  }
  float lmax[Q];
#pragma unroll
  for (int s = 0; s < Q; ++s) lmax[s] = -INFINITY;
  constexpr int U = Q > 8 ? 4 : 8;   // key rows in flight per thread (the decode kernel's 8 while the slots' registers allow it)
  // full passes end below Smin: every slot sees all of their keys, no checks; the passes behind carry the load bound and the limits
  auto k_pass = [&](const int j0, auto tail) {
    constexpr bool TAIL = decltype(tail)::value;
    uint4 kv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * KPP + kslot;
      if constexpr (TAIL) {
        kv[u] = uint4{0u, 0u, 0u, 0u};
        if (j < S) kv[u] = lia_ldg_stream(kbase + (long)j * kv_row + 8 * sub);
      } else {
        kv[u] = lia_ldg_stream(kbase + (long)j * kv_row + 8 * sub);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * KPP + kslot;
      const uint32_t w[4] = {kv[u].x, kv[u].y, kv[u].z, kv[u].w};
#pragma unroll
      for (int s = 0; s < Q; ++s) {
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          a = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(lia_bf16x2, qp[s][e]), __builtin_bit_cast(lia_bf16x2, w[e]), a, false);
        if constexpr (LPK == 16) {
          a += dpp_f32<0x128>(a);     // row_ror:8   (the decode kernel's butterfly)
          a += dpp_f32<0x124>(a);     // row_ror:4
          a += dpp_f32<0x4E>(a);      // quad_perm:[2,3,0,1]  (xor 2)
          a += dpp_f32<0xB1>(a);      // quad_perm:[1,0,3,2]  (xor 1)
        } else {
#pragma unroll
          for (int o = LPK / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        }
        if (!TAIL || j < lim[s]) {
          float sv = rbf(a);
          if (post_scale) sv = rbf(sv * scaling);
          if (sub == 0) sc[s * Spad + j] = sv;
          lmax[s] = fmaxf(lmax[s], sv);
        }
      }
    }
  };
  const int s_full = Smin - Smin % (U * KPP);
  for (int j0 = 0; j0 < s_full; j0 += U * KPP) k_pass(j0, std::false_type{});
  for (int j0 = s_full; j0 < S; j0 += U * KPP) k_pass(j0, std::true_type{});
#pragma unroll
  for (int s = 0; s < Q; ++s) {
    float m = wave_max(lmax[s]);
    if (lane == 0) scratch[s * 8 + wave] = m;
  }
  __syncthreads();
  float lrow[Q];
#pragma unroll
  for (int s = 0; s < Q; ++s) {
    const float mrow = fmaxf(fmaxf(scratch[s * 8], scratch[s * 8 + 1]), fmaxf(scratch[s * 8 + 2], scratch[s * 8 + 3]));
    float ls = 0.f;
    for (int j = tid; j < lim[s]; j += 256) {
      float e = __expf(sc[s * Spad + j] - mrow);
      sc[s * Spad + j] = e;
      ls += e;
    }
    ls = wave_sum(ls);
    if (lane == 0) scratch[s * 8 + 4 + wave] = ls;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < Q; ++s) lrow[s] = scratch[s * 8 + 4] + scratch[s * 8 + 5] + scratch[s * 8 + 6] + scratch[s * 8 + 7];
#pragma unroll
  for (int s = 0; s < Q; ++s)
    for (int j = tid; j < lim[s]; j += 256) sc[s * Spad + j] = rbf(sc[s * Spad + j] / lrow[s]);
  __syncthreads();

  float o[Q][8];
#pragma unroll
  for (int s = 0; s < Q; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) o[s][e] = 0.f;
  auto v_pass = [&](const int j0, auto tail) {
    constexpr bool TAIL = decltype(tail)::value;
    uint4 vv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if constexpr (TAIL) {
        vv[u] = uint4{0u, 0u, 0u, 0u};
        if (j0 + u * KPP < S) vv[u] = lia_ldg_stream(vbase + (long)(j0 + u * KPP) * kv_row + 8 * sub);
      } else {
        vv[u] = lia_ldg_stream(vbase + (long)(j0 + u * KPP) * kv_row + 8 * sub);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * KPP;
      const uint32_t w[4] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
#pragma unroll
      for (int s = 0; s < Q; ++s) {
        if (!TAIL || j < lim[s]) {
          const float p = sc[s * Spad + j];
#pragma unroll
          for (int e = 0; e < 4; ++e) { o[s][2 * e] += p * bf2f(w[e] & 0xffff); o[s][2 * e + 1] += p * bf2f(w[e] >> 16); }
        }
      }
    }
  };
  for (int j0 = 0; j0 < s_full; j0 += U * KPP) v_pass(j0 + kslot, std::false_type{});
  for (int j0 = s_full; j0 < S; j0 += U * KPP) v_pass(j0 + kslot, std::true_type{});
#pragma unroll
  for (int s = 0; s < Q; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = o[s][e];
#pragma unroll
      for (int off = LPK; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
      o[s][e] = v;
    }
  if (lane < LPK) {
#pragma unroll
    for (int s = 0; s < Q; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) red[((size_t)wave * Q + s) * D + 8 * sub + e] = o[s][e];
  }
  __syncthreads();
  for (int idx = tid; idx < n_slots * D; idx += 256) {
    const int s = idx / D, dd = idx - s * D;
    const int t = s / G, g = s - t * G;
    const float acc = (red[(size_t)s * D + dd] + red[((size_t)Q + s) * D + dd]) +
                      (red[((size_t)2 * Q + s) * D + dd] + red[((size_t)3 * Q + s) * D + dd]);
    out[((long)b * T + t) * ldo + (long)(kh * G + g) * D + dd] = f2bf(acc);
  }
}

// the instantiated slot counts: every G * T up to LIA_BLOCK_MAX_Q runs in the smallest of them that holds it
#define LIA_BLOCK_MAX_Q 16
static int block_q_of(int n_slots) {
  static const int qs[] = {2, 3, 4, 5, 6, 7, 8, 12, 16};
  for (int v : qs)
    if (n_slots <= v) return v;
  return 0;
}

// The one rule of what the block launches take (lia_attn_block_launch, lia_attn_block_ragged_launch, lia_attn_block_takes): T queries
// per row whose last one sees S keys at most (S = pos0 + T; ragged: pos0 = max(lens)).  -> the instantiated slot count and the LDS
// bytes, or 0: d other than 32 / 64 / 128, heads % kv_heads, T < 2 or S - T < 1, more than LIA_BLOCK_MAX_Q slots, or scores + partials
// beyond 160 KB of LDS.
static int block_shape(int heads, int kv_heads, int d, int T, long S, size_t* lds_out) {
  if (T < 2 || S - T < 1 || kv_heads <= 0 || heads <= 0 || heads % kv_heads) return 0;
  if (d != 32 && d != 64 && d != 128) return 0;
  if ((long)(heads / kv_heads) * T > LIA_BLOCK_MAX_Q) return 0;
  const int Qv = block_q_of((heads / kv_heads) * T);
  if (!Qv) return 0;
  const size_t Spad = (size_t)((S + 3) & ~3L);     // (a padded row holds fewer keys: the unpadded size bounds it)
  const size_t lds = ((size_t)Qv * Spad + (size_t)4 * Qv * d + (size_t)Qv * 8) * sizeof(float);
  if (lds > 160 * 1024) return 0;
  if (lds_out) *lds_out = lds;
  return Qv;
}

extern "C" int lia_attn_block_takes(int heads, int kv_heads, int head_dim, int T, int S) { return block_shape(heads, kv_heads, head_dim, T, S, nullptr) ? 1 : 0; }

template <int D>
static int launch_block(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B, int T, int pos0,
                        int heads, int kv_heads, int Bc, int b0, float scaling, int post_scale, const int* starts, const int* lens,
                        hipStream_t st) {
  const int G = heads / kv_heads;
  size_t lds = 0;
  const int Qv = block_shape(heads, kv_heads, D, T, (long)pos0 + T, &lds);
  if (!Qv) return -1;
  dim3 grid(kv_heads, B);
#define LIA_BLK_MODE(QV, MODE, STARTS, LENS)                                                                                   \
  {                                                                                                                            \
    static bool attr = false;                                                                                                  \
    if (!attr) { (void)hipFuncSetAttribute((const void*)lia_attn_block_kernel<D, QV, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); attr = true; } \
    hipLaunchKernelGGL((lia_attn_block_kernel<D, QV, MODE>), grid, dim3(256), lds, st, q, ldq, kc, vc, out, ldo, T, pos0, G, kv_heads, Bc, b0, scaling, post_scale, STARTS, LENS); \
  }
#define LIA_BLK(QV)                                                                                                            \
  if (lens) LIA_BLK_MODE(QV, 2, starts, lens)                                                                                  \
  else if (starts) LIA_BLK_MODE(QV, 1, starts, nullptr)                                                                        \
  else LIA_BLK_MODE(QV, 0, nullptr, nullptr)
  switch (Qv) {
    case 2: LIA_BLK(2) break;
    case 3: LIA_BLK(3) break;
    case 4: LIA_BLK(4) break;
    case 5: LIA_BLK(5) break;
    case 6: LIA_BLK(6) break;
    case 7: LIA_BLK(7) break;
    case 8: LIA_BLK(8) break;
    case 12: LIA_BLK(12) break;
    case 16: LIA_BLK(16) break;
    default: return -1;
  }
#undef LIA_BLK
#undef LIA_BLK_MODE
  return 0;
}

template <typename... A>
static int launch_block_d(int d, A... a) {
  switch (d) {
    case 128: return launch_block<128>(a...);
    case 64: return launch_block<64>(a...);
    default: return launch_block<32>(a...);
  }
}

// lia_attn_append_launch's arguments and meaning, for blocks of a few queries: row t of the result is bit for bit the decode launch
// (padded, with starts) over S = pos0 + t + 1 keys with that query row.  Returns -1, nothing launched, for a d other than 32 / 64 /
// 128, heads % kv_heads != 0, T < 2 or pos0 < 1, (heads / kv_heads) * T > LIA_BLOCK_MAX_Q, or scores + partials beyond 160 KB of LDS.
extern "C" int lia_attn_block_launch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B, int T,
                                     int pos0, int heads, int kv_heads, int d, int Bc, int b0, int post_scale, const int* starts,
                                     hipStream_t st) {
  if (!block_shape(heads, kv_heads, d, T, (long)pos0 + T, nullptr)) return -1;
  if (B <= 0) return 0;
  return launch_block_d(d, q, ldq, kc, vc, out, ldo, B, T, pos0, heads, kv_heads, Bc, b0, 1.0f / sqrtf((float)d), post_scale, starts, (const int*)nullptr, st);
}

// The ragged form: served row b holds lens[b] cached positions of its own (device, B entries, 1 <= lens[b] <= max_len; starts: device,
// B entries with starts[b] <= lens[b], or NULL = all zeros).  Row b is bit for bit lia_attn_block_launch with B = 1 on that row at
// pos0 = lens[b].  max_len = max(lens) sizes the LDS; the caller guarantees lens[b] + T <= the cache's positions.  The same refusals
// (at pos0 = max_len), plus a NULL lens: -1, nothing launched.
extern "C" int lia_attn_block_ragged_launch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B,
                                            int T, int max_len, int heads, int kv_heads, int d, int Bc, int b0, int post_scale,
                                            const int* starts, const int* lens, hipStream_t st) {
  if (!lens || !block_shape(heads, kv_heads, d, T, (long)max_len + T, nullptr)) return -1;
  if (B <= 0) return 0;
  return launch_block_d(d, q, ldq, kc, vc, out, ldo, B, T, max_len, heads, kv_heads, Bc, b0, 1.0f / sqrtf((float)d), post_scale, starts, lens, st);
}

// The attention launch of a call with T queries per row behind pos0 cached positions: see lia_internal.h for the rule.
int lia_attn_dispatch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B, int T, int pos0,
                      int heads, int kv_heads, int d, int Bc, int b0, int post_scale, const int* starts, int tail, hipStream_t st,
                      LiaAttnOpts* opts) {
  // LIA_OPT_BLOCK_ATTENTION: the decode-shaped block launch where it takes the shape (-1: nothing was launched), else the append launch
  if (T > 1 && pos0 > 0 && !tail && opts && opts->block_attention &&
      lia_attn_block_launch(q, ldq, kc, vc, out, ldo, B, T, pos0, heads, kv_heads, d, Bc, b0, post_scale, starts, st) == 0) {
    ++opts->block_launches;
    return 0;
  }
  if (T > 1 && pos0 > 0 && !tail) return lia_attn_append_launch(q, ldq, kc, vc, out, ldo, B, T, pos0, heads, kv_heads, d, Bc, b0, post_scale, starts, st);
  const LiaTail t = lia_tail(tail, B, T, ldq);
  // the split-key route: by LIA_OPT_SPLIT_DECODE, and always where the one-workgroup launcher would refuse for LDS -- when the caller
  // placed the scratch (a layer call does, behind its workspace layout); otherwise today's launch with today's arguments
  if ((T == 1 || tail) && opts && opts->split_scratch && lia_attn_split_route(opts->split_decode, pos0 + T, heads, kv_heads, d)) {
    if (lia_attn_decode_split_launch(q + t.off, t.ld, kc, vc, out, ldo, B, pos0 + T, heads, kv_heads, d, Bc, b0, post_scale, starts,
                                     opts->split_scratch, opts->split_scratch_bytes, st))
      return -1;
    ++opts->split_launches;
    return 0;
  }
  if (T == 1 || tail) return decode_launch(q + t.off, t.ld, kc, vc, out, ldo, B, pos0 + T, heads, kv_heads, d, Bc, b0, post_scale, starts, st);
  return prefill_launch(q, ldq, kc, vc, out, ldo, B, T, heads, kv_heads, d, Bc, b0, post_scale, starts, st);
}
