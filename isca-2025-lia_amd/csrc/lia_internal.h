// Everything that crosses a translation unit inside liblia_hip.so and is not part of the C ABI (include/lia_hip.h): the kernels'
// host launchers, the context, and the helpers the API files (lia_ctx / lia_ops / lia_layer / lia_stream .hip) share.  The file that
// defines one of these includes this header and so does every file that calls it: a signature that drifts is a compile error.
// (tests/launchers.py restates the launcher signatures for ctypes.)  Declarations only -- no __device__ code.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/lia_hip.h"

// ---- host-only part: what lia_host.cpp (g++, no HIP) defines or calls.  lia_pack10_bound is in lia_hip.h.
extern "C" void lia_set_error(const char* fmt, ...);
extern "C" void lia_host_parallel_memcpy(void* dst, const void* src, size_t bytes, int n_threads);

#ifdef __HIPCC__
#include <string.h>
#include <vector>

#include "lia_common.h"

// ---- kernels' host launchers (exported unmangled: the GPU tests and the benches in tools/ call them directly)
// lia_gemm.hip
extern "C" size_t lia_gemm_workspace_bytes(int M, int N);
extern "C" int lia_gemm_launch(const bf16_t* x, long ldx, const bf16_t* W, long ldw, int M, int N, int K, const LiaEpilogue* ep,
                               const LiaOutMap* om, float* workspace, size_t workspace_bytes, LiaGemmOpts* opts, int force_split,
                               hipStream_t st, hipEvent_t ev0, hipEvent_t ev1, int* regime, const LiaPost* post, int* post_done);
// lia_elementwise.hip
extern "C" void lia_layernorm_launch(const bf16_t* x, long ldx, const bf16_t* g, const bf16_t* b, bf16_t* y, long ldy, long rows, int H,
                                     float eps, hipStream_t st);
extern "C" void lia_embed_launch(const int64_t* ids, const bf16_t* tok, const bf16_t* pos, bf16_t* y, int B, int T, int past_len, int H,
                                 hipStream_t st);
extern "C" void lia_embed_padded_launch(const int64_t* ids, const bf16_t* tok, const bf16_t* pos, bf16_t* y, int B, int T, int past_len,
                                        int H, const int* starts, hipStream_t st);
extern "C" void lia_embed_ragged_launch(const int64_t* ids, const bf16_t* tok, const bf16_t* pos, bf16_t* y, int B, int T, int H,
                                        const int* lens, const int* starts, hipStream_t st);
extern "C" void lia_kv_scatter_ragged_launch(const bf16_t* ksrc, const bf16_t* vsrc, bf16_t* kc, bf16_t* vc, int B, int T, int H, int Bc,
                                             int b0, const int* lens, hipStream_t st);
extern "C" void lia_argmax_launch(const bf16_t* logits, int64_t* out, int B, int vocab, int suppress, hipStream_t st);
extern "C" void lia_blit_launch(void* dst, const void* src, size_t bytes, hipStream_t st);
// the MASKED instantiations (lia_ctx_set_token_mask): the launch above with the allowed-token bit rows -- row r of the call (the
// verify launches: block row r0 + r) reads mask + r * ldm words, ldm >= ceil(vocab / 32), or 0 for one row shared by every row
extern "C" void lia_argmax_masked_launch(const bf16_t* logits, int64_t* out, int B, int vocab, int suppress, const uint32_t* mask, long ldm,
                                         hipStream_t st);
extern "C" void lia_verify_argmax_masked_launch(const bf16_t* logits, long ld, int n, int vocab, int suppress, int n_suppress,
                                                const int* n_suppress_rows, int T, int r0, int64_t* greedy, const uint32_t* mask, long ldm,
                                                hipStream_t st);
extern "C" void lia_sample_masked_launch(const bf16_t* logits, long ld, int B, int vocab, float tau, int top_k, float top_p, int suppress,
                                         const float* uniforms, int64_t* out, float* stats, const uint32_t* mask, long ldm, hipStream_t st);
extern "C" void lia_verify_sample_masked_launch(const bf16_t* logits, long ld, int n, int vocab, float tau, int top_k, float top_p,
                                                int suppress, int n_suppress, const int* n_suppress_rows, int T, int r0,
                                                const float* uniforms, long ldu, int n_steps, int step0, const int* step_rows,
                                                const int64_t* block_ids, int64_t* sampled, float* p_draft, const uint32_t* mask, long ldm,
                                                hipStream_t st);
// lia_sample.hip, lia_score.hip
extern "C" void lia_sample_launch(const bf16_t* logits, long ld, int B, int vocab, float tau, int top_k, float top_p, int suppress,
                                  const float* uniforms, int64_t* out, float* stats, hipStream_t st);
extern "C" void lia_verify_sample_launch(const bf16_t* logits, long ld, int n, int vocab, float tau, int top_k, float top_p, int suppress,
                                         int n_suppress, const int* n_suppress_rows, int T, int r0, const float* uniforms, long ldu,
                                         int n_steps, int step0, const int* step_rows, const int64_t* block_ids, int64_t* sampled,
                                         float* p_draft, hipStream_t st);
extern "C" void lia_verify_reject_launch(const bf16_t* logits, long ld, int n, int vocab, const bf16_t* draft_logits, long ldd_row,
                                         long ldd_pos, float tau, int top_k, float top_p, int suppress, int n_suppress, int T, int r0,
                                         const float* u_acc, const float* u_res, long ldu, int n_steps, int step0, const int64_t* block_ids,
                                         int64_t* token, int* ok, float* p_tok, float* q_tok, float* resid_mass, hipStream_t st);
extern "C" void lia_verify_reject_accept_launch(const int64_t* block_ids, const int64_t* token, const int* ok, const int* active, int B, int T,
                                                int* accepted, int* common, int64_t* next, hipStream_t st);
extern "C" void lia_token_logprobs_launch(const bf16_t* logits, long ld, int M, int vocab, const int64_t* targets, float* logprobs,
                                          int64_t* greedy, hipStream_t st);
// lia_logprobs.hip: row r's chosen[r], top_ids / top_logprobs[r * n_top ..) of logits row r with ids[r]; n_top in [0, LIA_LOGPROB_MAX_TOP]
// and <= vocab (the callers check)
extern "C" void lia_topn_logprobs_launch(const bf16_t* logits, long ld, int M, int vocab, const int64_t* ids, int n_top, float* chosen,
                                         int64_t* top_ids, float* top_logprobs, hipStream_t st);
extern "C" void lia_verify_argmax_launch(const bf16_t* logits, long ld, int n, int vocab, int suppress, int n_suppress, int T, int r0,
                                         int64_t* greedy, hipStream_t st);
extern "C" void lia_verify_argmax_rows_launch(const bf16_t* logits, long ld, int n, int vocab, int suppress, int n_suppress,
                                              const int* n_suppress_rows, int T, int r0, int64_t* greedy, hipStream_t st);
extern "C" void lia_verify_accept_launch(const int64_t* block_ids, const int64_t* greedy, const int* active, int B, int T, int* accepted,
                                         int* common, int64_t* next, hipStream_t st);
// lia_penalty.hip: out [M, ldo] = logits [M, ld] penalised under counts [M, ldc] (out == logits allowed); ids [B, n] added to counts
// [B, ldc] -- generated = 0: the prompt bit, 1: the saturating count; first / active: int32 [B] or NULL.  The callers check the
// pitches (>= vocab; ldc even) and the table's 4-byte alignment
extern "C" void lia_penalty_launch(const bf16_t* logits, long ld, int M, int vocab, const uint16_t* counts, long ldc, float theta,
                                   float alpha_p, float alpha_f, bf16_t* out, long ldo, hipStream_t st);
extern "C" void lia_token_counts_launch(uint16_t* counts, long ldc, int B, int vocab, const int64_t* ids, long ldi, int n, const int* first,
                                        const int* active, int generated, hipStream_t st);
// lia_llama.hip
extern "C" void lia_rmsnorm_launch(const bf16_t* x, long ldx, const bf16_t* w, bf16_t* y, long ldy, long rows, int H, float eps,
                                   hipStream_t st);
extern "C" void lia_rope_launch(bf16_t* x, long row_stride, const bf16_t* cosb, const bf16_t* sinb, long rows, int heads, int d, int pos0,
                                int pos_mod, int pos_div, hipStream_t st);
extern "C" void lia_silu_mul_launch(const bf16_t* gu, bf16_t* out, long M, int F, int gu_block, hipStream_t st);
extern "C" void lia_embed_tokens_launch(const int64_t* ids, const bf16_t* tok, bf16_t* y, long rows, int H, hipStream_t st);
// lia_pack10.hip, lia_pack10a.hip
extern "C" void lia_packed_decode_launch(const char* src, bf16_t* dst, size_t n_values, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
extern "C" void lia_pack10a_decode_launch(const char* src, bf16_t* dst, size_t n_values, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
// lia_attention.hip.  The _padded ones return -1 for a NULL starts; the append one takes starts or NULL.
extern "C" int lia_attn_prefill_launch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B, int T,
                                       int heads, int kv_heads, int d, int Bc, int b0, int post_scale, hipStream_t st);
extern "C" int lia_attn_prefill_padded_launch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B,
                                              int T, int heads, int kv_heads, int d, int Bc, int b0, int post_scale, const int* starts,
                                              hipStream_t st);
extern "C" int lia_attn_append_launch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B, int T,
                                      int pos0, int heads, int kv_heads, int d, int Bc, int b0, int post_scale, const int* starts,
                                      hipStream_t st);
extern "C" int lia_attn_decode_launch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B, int S,
                                      int heads, int kv_heads, int d, int Bc, int b0, int post_scale, hipStream_t st);
extern "C" int lia_attn_decode_padded_launch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B,
                                             int S, int heads, int kv_heads, int d, int Bc, int b0, int post_scale, const int* starts,
                                             hipStream_t st);
// the append launch's arguments for a block of (heads / kv_heads) * T <= 16 query slots; -1 (nothing launched) for any other shape
extern "C" int lia_attn_block_launch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B, int T,
                                     int pos0, int heads, int kv_heads, int d, int Bc, int b0, int post_scale, const int* starts,
                                     hipStream_t st);
// the ragged form (per-row acceptance): row b at its own base length lens[b] <= max_len (device, B entries); starts or NULL; -1 as above
extern "C" int lia_attn_block_ragged_launch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B,
                                            int T, int max_len, int heads, int kv_heads, int d, int Bc, int b0, int post_scale,
                                            const int* starts, const int* lens, hipStream_t st);
// the split-key decode route (lia_attention.hip): lia_attn_decode_launch's arguments, starts or NULL, and the call's scratch of
// lia_attn_split_scratch_bytes; -1 (nothing launched): d or heads / kv_heads not instantiated, scratch too small, S < 1.
// lia_attn_split_chunk and lia_attn_split_scratch_bytes (include/lia_hip.h) are pure host arithmetic.
extern "C" int lia_attn_decode_split_launch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B, int S,
                                            int heads, int kv_heads, int d, int Bc, int b0, int post_scale, const int* starts, void* scratch,
                                            size_t scratch_bytes, hipStream_t st);
// ... with the chunk as an argument (a multiple of the kernel's pass), for tools/attn_split_bench's sweep
extern "C" size_t lia_attn_split_scratch_bytes_chunk(int B, int S, int heads, int kv_heads, int d, int chunk);
extern "C" int lia_attn_decode_split_launch_chunk(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B,
                                                  int S, int heads, int kv_heads, int d, int Bc, int b0, int post_scale, const int* starts,
                                                  int chunk, void* scratch, size_t scratch_bytes, hipStream_t st);

// ---- helpers shared by the API files: C++ linkage, kept out of the dynamic symbol table
#define LIA_HIDDEN __attribute__((visibility("hidden")))

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) {                                                                  \
      lia_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return _e == hipErrorOutOfMemory ? LIA_ERR_MEMORY : LIA_ERR_HIP;                      \
    }                                                                                        \
  } while (0)

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Rows behind the q | k | v projection of a layer call on B x T rows of pitch H: all of them, or (tail: the _last operators and the
// attention dispatch) the last position of each batch row -- row b*T + T-1, i.e. `off` values into the buffer at a pitch of `ld`.
struct LiaTail { long rows, off, ld; };
static inline LiaTail lia_tail(int tail, int B, int T, long H) {
  return tail ? LiaTail{(long)B, (long)(T - 1) * H, (long)T * H} : LiaTail{(long)B * T, 0, H};
}

// lia_attention.hip: the one place that picks the attention launch of a call with T queries per row behind pos0 cached positions
//   T > 1 && pos0 > 0 && !tail -> append;  T == 1 || tail -> decode over S = pos0 + T keys (tail: the last query of each row);
//   otherwise -> prefill;  starts != NULL: the padded instantiations.  Returns the launcher's 0 / -1.
//   opts (nullable = defaults), LIA_OPT_BLOCK_ATTENTION set: the append case goes to the block launch where that takes the shape
//   the decode case, when the caller placed split_scratch: the split-key launch where lia_attn_split_route says so
struct LiaAttnOpts {
  int block_attention;      // 0 (default): append launch; 1: lia_attn_block_launch first (the speculative verify pass sets it)
  long block_launches;      // LIA_CNT_BLOCK_ATTENTION
  int split_decode;         // LIA_OPT_SPLIT_DECODE: 0 (default): split only past the one-workgroup kernel's LDS bound; 1: whenever S > C
  long split_launches;      // LIA_CNT_SPLIT_DECODE
  void* split_scratch;      // the scratch of THIS call (a layer call places it behind its workspace layout), or NULL: never split
  size_t split_scratch_bytes;
};
// 0: the one-workgroup launch; 1: split by the option (S > lia_attn_split_chunk); 2: split because that launch refuses S for LDS
LIA_HIDDEN int lia_attn_split_route(int option, int S, int heads, int kv_heads, int d);
LIA_HIDDEN int lia_attn_dispatch(const bf16_t* q, long ldq, const bf16_t* kc, const bf16_t* vc, bf16_t* out, long ldo, int B, int T,
                                 int pos0, int heads, int kv_heads, int d, int Bc, int b0, int post_scale, const int* starts, int tail,
                                 hipStream_t st, LiaAttnOpts* opts = nullptr);

// ---- head modifiers: ambient state of the context that every head call (lm_head, sample, lm_score, lm_verify*) looks at.  Each is
// the CALLER's device memory -- only pointers are kept -- and row i of a call uses row i of each.  A NULL first member: not set, and
// a head launches what it launched without it.  lia_ctx_set_token_mask / _logprob_sink / _penalties (lia_ctx.hip) fill them;
// head_mods_resolve (lia_ops.hip) is the one place a head reads them.
struct LiaTokenMask {          // the MASKED kernel instantiations in place of the plain ones
  const uint32_t* table;
  long ld;                     // words between rows; 0: one row for every row
  int rows;
};
struct LiaSink {               // lia_topn_logprobs_kernel behind the head's own id kernel
  float* chosen;
  int64_t* top_ids;
  float* top;
  int n_top;
  long rows;
};
struct LiaPenalties {          // lm_head and sample: lia_penalty_kernel from their logits into the scratch, their id kernel on the scratch
  const uint16_t* counts;
  long ldc;
  int rows;
  float theta, presence, frequency;
  bf16_t* scratch;
  long lds;
};
struct LiaHeadMods { LiaTokenMask mask; LiaSink sink; LiaPenalties penalties; };

// ---- context (lia_ctx.hip)
struct lia_ctx {
  int device;
  hipStream_t compute;
  hipStream_t d2h;           // K/V delivery to the host cache (policy 0)
  char* ws;
  size_t ws_bytes;           // what a call may use: ws_alloc_bytes, or the kept part [0, keep) while the rest is lent (ctx_ws_lend)
  size_t ws_alloc_bytes;     // what lia_ctx_create allocated
  const void* ws_lent_to;    // the streamer whose wire cache holds the lent part; NULL: nothing is lent
  hipEvent_t slab_ready[2];  // recorded on compute when a K/V slab may be copied out
  hipEvent_t slab_done[2];   // recorded on d2h when the slab has been delivered
  bool slab_used[2];
  int slab_next;
  char* host_stage;          // pinned: q|k|v and attention output of the policy-2 round trip
  size_t host_stage_bytes;
  int host_threads;
  long last_rows, last_slab_rows;  // workspace layout of the previous layer call
  // live kernel timing for bench.py's roofline object (lia_prof_*)
  bool prof_on;
  std::vector<hipEvent_t>* prof_events;
  struct ProfRec { int regime; double bytes, flops; };
  std::vector<ProfRec>* prof_recs;
  size_t prof_cap;
  int prof_stride;      // every prof_stride-th GEMM launch is bracketed (an event pair costs ~2 x 6 us of stream idle)
  long prof_seen;
  long prof_host_attn_calls;
  double prof_host_attn_ms;
  LiaGemmOpts gemm_opts;     // per-context switches / counters of the GEMM launcher (lia_ctx_set_option, lia_ctx_get_counter)
  LiaAttnOpts attn_opts;     // ... of the attention dispatch
  std::vector<hipEvent_t>* deliver_events;   // lia_kv_deliver tickets (events on the d2h stream), recycled round-robin
  std::vector<char>* deliver_pending;
  hipEvent_t deliver_t0, deliver_t1;         // timing events on the d2h stream around one batch of deliveries (lia_kv_deliver_batch_ms)
  bool deliver_batch_open;
  // cross-layer chaining (lia_ctx_chain_next_norm): the combine of a layer call's last GEMM also normalises the output row with
  // the NEXT layer's first-norm weights into the workspace's norm buffer; the next call finds it there and skips its first norm
  const bf16_t *chain_g, *chain_b;
  bool chain_armed;                 // one-shot, consumed by the next layer call
  const void* normed_src;           // the y whose norm sits in normed_buf ...
  const void* normed_buf;
  long normed_rows;                 // ... for this many rows of this width
  int normed_h;
  // LIA_SERIALIZE=1 (debug): ONE stream for everything -- the K/V delivery stream IS the compute stream, and a streamer created
  // on this context copies and decodes on it too, so every event handshake is trivially ordered.  Results must not change; if
  // they do, a cross-stream ordering is missing (the role torch.cuda.synchronize() plays at lia/modeling_opt.py:1339,1528).
  bool serialized;
  char* hidden_tmp;           // a third hidden-state buffer for lia_decode_layers (a layer never writes the buffer it reads)
  size_t hidden_tmp_bytes;
  // left-padded batch (lia_ctx_set_key_starts): per cache batch row, the first cache position its queries attend; a host copy
  // (validation, the policy-2 host attention) and a device copy in a buffer of key_starts_cap entries that only grows
  std::vector<int>* key_starts;
  int* key_starts_dev;
  int key_starts_cap;
  int key_starts_n;           // 0: no table -- every layer call takes the unpadded route
  // ragged cache (lia_ctx_set_row_lens): per cache batch row, the positions it has cached; kept like the key starts.  While a table
  // is set, every lia_layer_forward is the ragged form (policy 3, T >= 2)
  std::vector<int>* row_lens;
  int* row_lens_dev;
  int row_lens_cap;
  int row_lens_n;             // 0: no table
  LiaHeadMods mods;           // what the head calls also look at: token mask, log-probability sink, penalties (above)
};

// the workspace is about to be reused: a norm the previous layer call chained into it is gone, and so is a pending hint
static inline void ws_invalidate(lia_ctx* ctx) { ctx->normed_src = nullptr; ctx->chain_armed = false; }

// Lending the workspace's tail to a streamer's wire cache (lia_stream_cache_configure).  Event-only, nothing is allocated.
//   lend: the context offers bytes [0, keep) from here on (keep a multiple of 256, < ws_alloc_bytes); `first_writer` -- the stream
//       that writes the lent part first -- is put behind everything queued on the compute stream and behind the K/V deliveries
//       still draining from the workspace's slabs.  LIA_ERR_INVALID when the workspace is lent already.
//   take_back: the compute stream's next launch runs behind `idle` (recorded by the borrower behind its last reader).
LIA_HIDDEN int ctx_ws_lend(lia_ctx* ctx, const void* borrower, size_t keep, hipStream_t first_writer, hipEvent_t scratch_event);
LIA_HIDDEN int ctx_ws_take_back(lia_ctx* ctx, const void* borrower, hipEvent_t idle);

// Chaining state of one layer call (lia_ctx_chain_next_norm).  take: consume the hint for THIS call's last GEMM (g / b: the next
// layer's first-norm weights, or NULL) and tell whether the previous call already left norm1(x) in `ln`; publish: after the last
// GEMM, when its combine did write the next layer's norm of y there.
struct LiaChain {
  const bf16_t *g, *b;
  bool have_norm1;
};
static inline LiaChain chain_take(lia_ctx* ctx, const void* x, const void* ln, long rows, int H) {
  LiaChain c{ctx->chain_armed ? ctx->chain_g : nullptr, ctx->chain_armed ? ctx->chain_b : nullptr,
             ctx->normed_src == x && ctx->normed_buf == ln && ctx->normed_rows == rows && ctx->normed_h == H};
  ws_invalidate(ctx);
  return c;
}
static inline void chain_publish(lia_ctx* ctx, const void* y, const void* ln, long rows, int H) {
  ctx->normed_src = y; ctx->normed_buf = ln; ctx->normed_rows = rows; ctx->normed_h = H;
}

// ---- sub-layer ops the layer operators build on (lia_ops.hip)
// the penalty settings and a count table (lia_ops.hip), worded once for the three entry points: true = refused, the error is set.
// vocab < 0: the pitch is checked for evenness only (lia_ctx_set_penalties does not know the vocabulary)
LIA_HIDDEN bool penalty_args_invalid(const char* who, float repetition, float presence, float frequency, const void* counts, long ldc,
                                     int vocab);
LIA_HIDDEN LiaOutMap plain_out(bf16_t* y, long ldy, int N);
LIA_HIDDEN int gemm_checked(lia_ctx* ctx, const bf16_t* x, long ldx, const bf16_t* w, int M, int N, int K, const LiaEpilogue& ep,
                            const LiaOutMap& om, float* ws, size_t ws_bytes, int split, hipStream_t st, const LiaPost* post = nullptr,
                            int* post_done = nullptr);
LIA_HIDDEN int qkv_project(lia_ctx* ctx, const bf16_t* x, const bf16_t* w, const bf16_t* bias, bf16_t* qout, bf16_t* kdst, bf16_t* vdst,
                           bool kv_cache_mode, int B, int T, int H, int cache_batch, int b0, int pos0, float* ws, size_t ws_bytes,
                           hipStream_t st);
#endif  // __HIPCC__
