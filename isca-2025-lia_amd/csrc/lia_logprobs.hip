// Per-token log-probabilities with the top-N alternatives: per row of bf16 logits, log p(ids[r]) and the n_top
// tokens of largest logit with their log-probabilities, under the model's own distribution -- the fp32 log-softmax of the raw
// logits; no temperature, filter, suppressed token or token mask.  One LIA_ROW_THREADS workgroup per row; nothing is sorted but the
// at most LIA_LOGPROB_MAX_TOP survivors.
//
//   passes 1, 2  m and s = sum exp(l - m): row_max_sum, the very code of lia_token_logprobs_kernel, and the same final expression
//                l_t - (m + log s) for the chosen token and for every alternative -- bit for bit that kernel's value
//   pass A       counts per top-12-bit bin of the sampler's 16-bit key (key_of: the order of a bf16 row) -> the bin that holds the
//                n_top-th largest key, counting multiplicity
//   pass B       counts per low nibble inside that bin -> kappa, and n_above = |{key > kappa}| < n_top
//   pass C       tiles of 8 tokens per thread in token order: one block prefix sum per tile of (key > kappa, key == kappa) counts,
//                packed 16 + 16 bits (a tile holds 8192 tokens; the running counts over the tiles are two ints).  A token above kappa takes the slot of its rank among those; of the tokens AT kappa the first
//                n_top - n_above in id order take the slots behind.  Stops at the tile that completes both.
//   order        survivor j's place = |{i : (key_i, -id_i) > (key_j, -id_j)}|: key descending, ties by the lower id
// The histograms are integer LDS atomics (the same counts in every run); which slot a survivor lands in is a prefix sum, not an
// atomic: no result depends on the order in which lanes ran.  Logits are finite or +-inf, not NaN; a -inf logit has key
// SMP_KEY_NEG_INF, below every finite one, and log-probability -inf; a row of nothing but -inf gives NaN (as lia_score.hip).
#include "lia_row_passes.h"

static_assert(LIA_LOGPROB_MAX_TOP == 32, "the survivors are ordered by the first LIA_LOGPROB_MAX_TOP threads of the workgroup");
static_assert(SMP_TILE < (1 << 16), "pass C packs the two counts of ONE tile into 16 bits each; across tiles they are carried apart");

__global__ __launch_bounds__(LIA_ROW_THREADS) void lia_topn_logprobs_kernel(const bf16_t* __restrict__ logits, long ld, int vocab, int vec,
                                                                            const int64_t* __restrict__ ids, int n_top,
                                                                            float* __restrict__ chosen, int64_t* __restrict__ top_ids,
                                                                            float* __restrict__ top_logprobs) {
  __shared__ uint32_t cnt[SMP_BINS];
  __shared__ uint32_t nib[16];
  __shared__ uint32_t red32[LIA_ROW_WAVES];
  __shared__ int sh_bin, sh_kappa;
  __shared__ uint32_t sh_above;
  __shared__ int surv_key[LIA_LOGPROB_MAX_TOP], surv_id[LIA_LOGPROB_MAX_TOP];
  const int tid = threadIdx.x;
  const bf16_t* row = logits + (long)blockIdx.x * ld;

  const RowMaxSum p = row_max_sum(row, vocab, vec);
  if (tid == 0) chosen[blockIdx.x] = row_logprob(row, vocab, ids[blockIdx.x], p.m, p.s);
  if (n_top <= 0) return;

  // ---- pass A: counts per top-12 bin -> the bin of the n_top-th largest key ----
  for (int b = tid; b < SMP_BINS; b += LIA_ROW_THREADS) cnt[b] = 0;
  if (tid < 16) nib[tid] = 0;
  __syncthreads();
  for (int i = tid * 8; i < vocab; i += SMP_TILE) {
    int k[8];
    load_keys8(row, i, vocab, vec, -1, k);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (k[e] >= 0) atomicAdd(&cnt[k[e] >> 4], 1u);
  }
  __syncthreads();
  find_boundary_bin<uint32_t>(cnt, (uint32_t)n_top, red32, &sh_bin, &sh_above);    // (n_top <= vocab: a bin qualifies)
  const int bk = sh_bin;

  // ---- pass B: counts per low nibble inside it -> kappa ----
  for (int i = tid * 8; i < vocab; i += SMP_TILE) {
    int k[8];
    load_keys8(row, i, vocab, vec, -1, k);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (k[e] >= 0 && (k[e] >> 4) == bk) atomicAdd(&nib[k[e] & 15], 1u);
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t above = sh_above;
    int l = 15;
    for (; l > 0; --l) {
      if (above + nib[l] >= (uint32_t)n_top) break;
      above += nib[l];
    }
    sh_kappa = (bk << 4) | l;
    sh_above = above;
  }
  __syncthreads();
  const int kappa = sh_kappa;
  const int n_above = (int)sh_above;          // |{key > kappa}| < n_top
  const int need = n_top - n_above;           // of the tokens at kappa: the first `need` in id order

  // ---- pass C: the survivors' slots, by prefix sums in token order ----
  const int ntiles = (vocab + SMP_TILE - 1) / SMP_TILE;
  int above_seen = 0, at_seen = 0;            // tokens above kappa / at kappa before this tile (any vocab: never packed)
  for (int j = 0; j < ntiles; ++j) {
    const int i = j * SMP_TILE + tid * 8;
    int k[8];
    load_keys8(row, i, vocab, vec, -1, k);
    uint32_t c = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) c += (k[e] > kappa ? 1u : 0u) + (k[e] == kappa ? 0x10000u : 0u);
    uint32_t tot;
    const uint32_t ex = block_excl_scan<uint32_t>(c, red32, &tot);      // inside one tile either half is <= 8192
    int g = above_seen + (int)(ex & 0xffffu), q = at_seen + (int)(ex >> 16);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (k[e] > kappa) {
        if (g < n_above) { surv_key[g] = k[e]; surv_id[g] = i + e; }
        ++g;
      } else if (k[e] == kappa) {
        if (q < need) { surv_key[n_above + q] = k[e]; surv_id[n_above + q] = i + e; }
        ++q;
      }
    }
    above_seen += (int)(tot & 0xffffu);
    at_seen += (int)(tot >> 16);
    if (above_seen >= n_above && at_seen >= need) break;
  }
  __syncthreads();

  // ---- the order of the survivors: key descending, ties by the lower id ----
  if (tid < n_top) {
    const int kj = surv_key[tid], ij = surv_id[tid];
    int place = 0;
    for (int o = 0; o < n_top; ++o) {
      const int ko = surv_key[o], io = surv_id[o];
      place += (ko > kj || (ko == kj && io < ij)) ? 1 : 0;
    }
    const long at = (long)blockIdx.x * n_top + place;
    top_ids[at] = ij;
    top_logprobs[at] = row_logprob(row, vocab, ij, p.m, p.s);
  }
}

extern "C" void lia_topn_logprobs_launch(const bf16_t* logits, long ld, int M, int vocab, const int64_t* ids, int n_top, float* chosen,
                                         int64_t* top_ids, float* top_logprobs, hipStream_t st) {
  if (M <= 0) return;
  const int vec = (ld % 8 == 0) && (vocab % 8 == 0) && (((uintptr_t)logits & 15) == 0);
  hipLaunchKernelGGL(lia_topn_logprobs_kernel, dim3(M), dim3(LIA_ROW_THREADS), 0, st, logits, ld, vocab, vec, ids, n_top, chosen, top_ids,
                     top_logprobs);
}
