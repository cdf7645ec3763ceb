/*
 * lia_hip.h -- C ABI of liblia_hip.so: the MI355X-native replacement for the GPU side and the
 * host-memory tiers of LIA's weight-offloaded cooperative decoder.
 *
 * Plain pointers and sizes only; no torch / HIP types in any signature (streams travel as void*,
 * which is a hipStream_t).  Every function returns 0 (LIA_OK) or a negative LIA_ERR_* code and never
 * throws; lia_last_error() gives the text.  The caller owns every buffer it passes in; the library
 * owns only its context, streams, events and workspace.  A context is re-entrant across contexts, not
 * thread-safe within one (the reference drives everything from one Python thread,
 * lia/modeling_opt.py:1208-1212).
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference tree;
 *   decoder.py    = intel_extension_for_pytorch/transformers/models/reference/modules/decoder.py
 *   attentions.py = intel_extension_for_pytorch/transformers/models/reference/modules/attentions.py
 *   modeling_opt.py = lia/modeling_opt.py).
 * INTEGRATION.md shows the ctypes stubs a reference maintainer would add.
 *
 * All activations / weights are bf16 (uint16 bit patterns).  Linear weights are ROW-MAJOR [N, K]
 * (the reference's TPP-blocked [N/16,K/64,32,16,2] wire format, _weight_prepack.py:19-63, is converted
 * once on the host by lia_tpp_unblock, not on every use as attentions.py:381-382 does).
 */
#ifndef LIA_HIP_H
#define LIA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIA_OK 0
#define LIA_ERR_INVALID (-1) /* bad shape / argument           -> Python ValueError  (attentions.py:503,516,532) */
#define LIA_ERR_MEMORY (-2)  /* allocation / pinning failed    -> Python MemoryError (modeling_opt.py:175)       */
#define LIA_ERR_HIP (-3)     /* HIP runtime error              -> Python RuntimeError                            */
#define LIA_ERR_MISSING (-4) /* a required tensor is NULL      -> Python AttributeError (modeling_opt.py:110,126) */

typedef uint16_t lia_bf16;
typedef struct lia_ctx lia_ctx;
typedef struct lia_streamer lia_streamer;

const char* lia_last_error(void);
const char* lia_version(void);

/* ---- context ----------------------------------------------------------------------------------
 * Replaces the per-forward stream/buffer setup of OPTDecoder.forward (modeling_opt.py:1178-1220).
 * workspace_bytes: device scratch for one layer call (see lia_layer_workspace_bytes). */
int lia_ctx_create(int device, size_t workspace_bytes, lia_ctx** out);
void lia_ctx_destroy(lia_ctx* ctx);
void* lia_ctx_compute_stream(lia_ctx* ctx); /* hipStream_t created by the context */
int lia_ctx_synchronize(lia_ctx* ctx);          /* compute AND K/V delivery streams */
int lia_ctx_synchronize_compute(lia_ctx* ctx);  /* the compute stream only (deferred K/V deliveries keep running) */
int lia_ctx_set_host_threads(lia_ctx* ctx, int n); /* OpenMP threads of the policy-2 host attention */
/* 1 when the context was created under LIA_SERIALIZE=1 (debug): the K/V delivery stream, and the copy / wire-decode streams of
 * every streamer created on it, ARE the compute stream, so no ordering depends on an event.  The reference serialises with
 * torch.cuda.synchronize() after every minibatch / layer (modeling_opt.py:1298,1339,1506,1528); a result that differs between
 * the two modes is a missing cross-stream dependency. */
int lia_ctx_serialized(lia_ctx* ctx);
/* Cross-layer chaining for decode (build-defined; the reference launches every LayerNorm as its own kernel, decoder.py:199-206).
 * One-shot promise about the NEXT lia_layer_forward / lia_llama_layer_forward call on this context: its output y will be the
 * input x of the call after it, unchanged, and that layer's first norm has weights g (and b; NULL for RMSNorm).  The layer then
 * normalises y inside the split-K combine of its last GEMM, and the following call (same x pointer, rows and width; anything
 * else falls back to the stand-alone norm kernel) skips its first norm.  g / b must be readable on the compute stream when the
 * hinted call is issued: chain resident layers, not a streamed layer whose copy may still be in flight. */
int lia_ctx_chain_next_norm(lia_ctx* ctx, const lia_bf16* g, const lia_bf16* b);

/* Live kernel timing for the benchmark's roofline report: while enabled, every GEMM main-kernel launch made
 * through this context is bracketed by HIP events on the stream it is launched on. */
typedef struct {
  long skinny_launches; double skinny_ms, skinny_bytes, skinny_flops; /* decode regime (M <= 256)  */
  long tiled_launches;  double tiled_ms, tiled_bytes, tiled_flops;    /* prefill regime            */
  double empty_bracket_ms; /* what an event pair around NOTHING reads on this stream: the bracket's own cost, measured at stop */
  long host_attention_calls; double host_attention_ms; /* policy-2 host attention (wall clock of lia_host_attention inside lia_layer_forward) */
} lia_prof_result;
int lia_prof_start(lia_ctx* ctx, int max_launches);
/* Bracket every stride-th GEMM launch only (default 1).  An event pair on the compute stream costs two ~6 us idle gaps, which is
 * the whole step's slack in the all-resident configurations; a stride co-prime to the launches per step samples every shape. */
int lia_prof_set_stride(lia_ctx* ctx, int stride);
int lia_prof_stop(lia_ctx* ctx, lia_prof_result* out); /* synchronises the compute stream */

/* ---- layer description and the 16-tensor weight set --------------------------------------------
 * Order fixed by create_buffer (modeling_opt.py:90-126) and consumed by index in decoder.py /
 * attentions.py:  0 ln1.w 1 ln1.b 2 q.w 3 q.b 4 k.w 5 k.b 6 v.w 7 v.b 8 out.w 9 out.b
 *                10 ln2.w 11 ln2.b 12 fc1.w 13 fc1.b 14 fc2.w 15 fc2.b                        */
typedef struct {
  int hidden; /* H */
  int heads;  /* h, head_dim = H / h in {32, 64, 128} */
  int ffn;    /* F */
  float ln_eps;
} lia_layer_desc;

/* Byte offsets of the 16 tensors inside one packed, 256-byte-aligned flat layer buffer -- the unit
 * the weight streamer moves (replaces 16 separate copy_ calls of load_layer, modeling_opt.py:270-293).
 * q.w|k.w|v.w and q.b|k.b|v.b are adjacent so the projection runs as one [3H,H] GEMM. */
int lia_layer_pack_offsets(const lia_layer_desc* d, size_t offsets[16], size_t* total_bytes);
size_t lia_layer_workspace_bytes(const lia_layer_desc* d, int max_rows /* B*T of one call */);

/* KV cache of one layer: seq-major [smax][batch][heads][head_dim] exactly like the reference's
 * past_key_value[1], [2] (attentions.py:462-476); the length is an explicit int instead of the shape of
 * a dummy tensor (attentions.py:464-470). */
typedef struct {
  lia_bf16* k;
  lia_bf16* v;
  int smax;
  int batch;     /* batch rows of the cache (row pitch) */
  int on_device; /* 1: k/v are device pointers (policy 3); 0: host pointers (policy 0 / 2)  */
} lia_kv;

/* ---- the operator boundary ----------------------------------------------------------------------
 * One decoder layer = decoder_layer(hidden, attention_mask=, past_key_value=, gpu_layer=, policy=,
 * max_new_tokens=) i.e. _IPEXDecoderLayerRef.forward -> OPTDecoderLayer_forward (decoder.py:172-335)
 * + _OPTAttention_forward (attentions.py:312-557).
 *
 *   policy 0 : everything on the GPU, K/V rows delivered to a HOST cache (prefill: rows [0,T) of batch
 *              rows [b0, b0+B) via the context's D2H stream; completion = lia_ctx_kv_store_wait)
 *   policy 3 : everything on the GPU, cache on the device (resident layers)
 *   policy 2 : LN + linears on the GPU, attention on the host over the host cache (decode, or a block of T > 1
 *              tokens appended at pos0 > 0: q, k, v of the B x T rows make the round trip)
 *   policy 1 : not a GPU policy -- LIA_ERR_INVALID (the all-CPU path lives in lia_host_*)
 *
 * weights[16]: DEVICE pointers (resident copy or a streamer slot).  x, y: device [B, T, H], may not
 * alias.  pos0 = tokens already in the cache; rows pos0..pos0+T-1 are written, 0..pos0+T-1 attended
 * (causal inside the new block).  b0 = first cache batch row served by this call (minibatch offset,
 * modeling_opt.py:1283-1339).  Asynchronous on `stream` except policy 2, which blocks the caller while
 * the host attends.
 * T > 1 at pos0 > 0 appends a block to a live cache (build-defined: a follow-up turn, a continuation to score): policy 3
 * scatters the block's K/V behind the cached rows and runs the append attention kernels (lia_attn_append_launch: query t at
 * position pos0 + t sees keys 0 .. pos0 + t) over the device cache; policy 0 pulls the pos0 cached rows of the served batch rows
 * into its slab -- (pos0 + T) x B rows, LIA_ERR_MEMORY before any launch when the workspace cannot hold them --, attends there
 * and delivers rows pos0 .. pos0 + T - 1 to the host cache (completion = lia_ctx_kv_store_wait). */
int lia_layer_forward(lia_ctx* ctx, const lia_layer_desc* d, int policy, const void* const weights[16],
                      const lia_bf16* x, lia_bf16* y, lia_kv* kv, int B, int T, int pos0, int b0, void* stream);
/* The LAST decoder layer of a prefill (build-defined; the reference computes every position of every layer, decoder.py:172-335):
 * only hidden[:, -1, :] of the last layer feeds the final LayerNorm and lm_head (models.py:424-431), but its K/V rows of EVERY
 * position feed the decode steps.  So: LN1 and the q | k | v projection on all B x T rows (cache written exactly as by
 * lia_layer_forward), then attention -- one query per row over the T keys --, out-proj, LN2, fc1 and fc2 on the last position
 * of each row only.  y_last: device [B, 1, H].  policy 0 or 3, T > 1, any pos0 (the last query attends the pos0 + T keys through the decode kernel).  Saves 9/12 of the layer's
 * GEMM flops. */
int lia_layer_forward_last(lia_ctx* ctx, const lia_layer_desc* d, int policy, const void* const weights[16],
                           const lia_bf16* x, lia_bf16* y_last, lia_kv* kv, int B, int T, int pos0, int b0, void* stream);
/* dst / src: device memory or pinned (mapped) host memory; bytes % 16 == 0; asynchronous on `stream`.  Kernel copy used for
 * the small activation hops of the cooperative policies (modeling_opt.py:320-355 load_activation / store_hidden). */
int lia_blit(void* dst, const void* src, size_t bytes, void* stream);
int lia_ctx_kv_store_wait(lia_ctx* ctx); /* host-blocks until every policy-0 K/V delivery has landed */
/* Deferred form of the policy-0 K/V delivery (store_cache, lia/modeling_opt.py:334-345): the prefill of a streamed layer writes
 * its K/V rows into a DEVICE holding cache (policy 3 arithmetic, `dev`: on_device = 1, same batch as `host`), and this call
 * enqueues the copy of rows [0, T) into the host cache behind everything already queued on the compute stream.  The scheduler
 * issues the deliveries after the prefill's last layer, so the 23 GB of K/V do not share the host link with the weight stream
 * of the prefill (H2D runs 8 % slower beside them); the first decode step waits per layer with lia_kv_deliver_wait(ticket)
 * right before that layer's host attention.  row_elems = heads * head_dim. */
int lia_kv_deliver(lia_ctx* ctx, const lia_kv* dev, lia_kv* host, int T, int row_elems, int* ticket);
int lia_kv_deliver_wait(lia_ctx* ctx, int ticket); /* host-blocks until that delivery has landed; frees the ticket */
/* device time (first copy's start -> last copy's end, on the delivery stream) of the deliveries issued since the last call; blocks
 * until they have landed.  What the reference's first-token latency contains and this build's does not (bench.py kv_delivery). */
int lia_kv_deliver_batch_ms(lia_ctx* ctx, double* ms);

/* ---- individual sub-layer ops (same kernels the layer call uses; exposed for parity tests) ------ */
/* F.layer_norm, decoder.py:107-119 */
int lia_layernorm(const lia_bf16* x, long ldx, const lia_bf16* g, const lia_bf16* b, lia_bf16* y, long ldy, long rows,
                  int H, float eps, void* stream);
/* torch.matmul(x, w.t()) + bias [relu] [residual + .], decoder.py:79-105,229,310; attentions.py:393-394,418.
 * y[M,N] row-major with leading dimension ldy.  bias / residual may be NULL.  split_k: 0 = heuristic.
 * Preconditions, else LIA_ERR_INVALID and nothing is launched: N % 16 == 0 and K % 64 == 0; ldx % 8 == 0 with x and w 16-byte
 * aligned (the kernels stage 16-byte row pieces); bias 8-byte aligned.  The skinny regime (M <= 256 and K % 128 == 0) stores
 * 4 columns at a time: ldy % 4 == 0 and ldr % 4 == 0, y and residual 8-byte aligned.  Every other shape runs the tiled kernels,
 * which store and read the residual 8 columns at a time: ldy % 8 == 0 and ldr % 8 == 0, y and residual 16-byte aligned. */
int lia_linear(lia_ctx* ctx, const lia_bf16* x, long ldx, const lia_bf16* w, const lia_bf16* bias,
               const lia_bf16* residual, long ldr, lia_bf16* y, long ldy, int M, int N, int K, int relu, int split_k,
               void* stream);
/* fused q|k|v projection: q -> qout [M,H]; k,v rows scattered into the seq-major cache slab
 * (attentions.py:393-394,418,457-458,475-476,490-491).  w = [3H,H], bias = [3H]. */
int lia_qkv_project(lia_ctx* ctx, const lia_bf16* x, const lia_bf16* w, const lia_bf16* bias, lia_bf16* qout,
                    lia_bf16* kcache, lia_bf16* vcache, int B, int T, int H, int cache_batch, int b0, int pos0,
                    void* stream);
/* GPU attention, attentions.py:443-536.  q [B,T,H] (ldq elements per token row); cache [S][cache_batch][h][d].
 * head_dim 32 / 64 / 128.  LIA_ERR_INVALID (by name in lia_last_error) for any other head_dim and, for a head_dim-128 prefill
 * (T > 1), for a cache whose key row -- cache_batch x heads x head_dim values -- exceeds 3.3e7 values (64 key rows = 4 GiB:
 * the kernel's 32-bit staging offsets; OPT-175B at a cache batch of 2048 is 2.5e7). */
int lia_attention(const lia_bf16* q, long ldq, const lia_bf16* kcache, const lia_bf16* vcache, lia_bf16* out, long ldo,
                  int B, int T, int S, int heads, int head_dim, int cache_batch, int b0, void* stream);
/* embed_tokens + embed_positions, modeling_opt.py:1108,357-378,1142 */
int lia_embed(const int64_t* ids, const lia_bf16* tok, const lia_bf16* pos, lia_bf16* y, int B, int T, int past_len, int H,
              void* stream);
/* ---- left-padded batches (generate(..., attention_mask=M), M = s_b zeros then ones per row) -------------------------------
 * The reference's CPU branch: positions from the mask (lia/modeling_opt.py:368-378), the 4-D additive causal + padding mask
 * (lia/modeling_opt.py:1133 -> mha_fusion.py:532-566).  A query at cache position i >= s_b attends keys s_b .. i; a query at a
 * pad position (i < s_b) gives a zero row.  Its GPU branch drops the mask (attentions.py:444-449, modeling_opt.py:1434,1469).
 * lia_ctx_set_key_starts: the table of s_b per cache batch row (host pointer, n_rows entries >= 0; NULL or 0 clears it).  The
 * context keeps a host copy and a device copy; lia_layer_forward, lia_layer_forward_last and lia_decode_layers then serve rows
 * b0 .. b0 + B - 1 through the padded attention (GPU policies and the policy-2 host attention); each s_b must be <= pos0 + T - 1,
 * and <= pos0 for a block of T > 1 tokens appended at pos0 > 0 (an appended block has no pad query rows).
 * Without a table they take the unpadded route, unchanged.
 * lia_embed_padded: position p - s_b + 2 for the token at cache position p = past_len + t >= s_b, position 1 at a pad position.
 * lia_attention_padded: lia_attention with the starts of the served rows.  starts: DEVICE pointers, B entries (row b <-> b0 + b). */
int lia_ctx_set_key_starts(lia_ctx* ctx, const int32_t* starts_host, int n_rows);
int lia_embed_padded(const int64_t* ids, const lia_bf16* tok, const lia_bf16* pos, lia_bf16* y, int B, int T, int past_len, int H,
                     const int32_t* starts_device, void* stream);
int lia_attention_padded(const lia_bf16* q, long ldq, const lia_bf16* kcache, const lia_bf16* vcache, lia_bf16* out, long ldo,
                         int B, int T, int S, int heads, int head_dim, int cache_batch, int b0, const int32_t* starts_device,
                         void* stream);
/* ---- ragged cache (build-defined; DESIGN.md 3.11 "row mode"): per-row acceptance of speculative decoding lets the rows' cache
 * lengths drift apart.  Serves OPT layers whose cache lives in HBM (policy 3), blocks of T >= 2 tokens.
 * lia_ctx_set_row_lens: the table of lens[b] >= 1 per cache batch row = the positions row b has cached (host pointer, n_rows
 * entries; NULL or 0 clears it), kept like the key starts: a host copy for validation, a device copy replaced only after the
 * compute stream has drained.  WHILE A TABLE IS SET every lia_layer_forward is the ragged form: it serves rows b0 .. b0 + B - 1 of the
 * table, block token t of row b sits at cache position lens[b] + t and attends keys starts[b] .. lens[b] + t (starts: the key-start
 * table, or zeros); pos0 must be >= every served lens[b] (pass max(lens)) and only sizes buffers.  The q | k | v GEMM writes K and V
 * into the workspace, a scatter kernel places row (b, t) in cache row (lens[b] + t) * batch + b0 + b, and the attention is the
 * ragged block launch -- row b bit for bit the block attention of a one-row call at pos0 = lens[b]; it counts in
 * LIA_CNT_BLOCK_ATTENTION whatever LIA_OPT_BLOCK_ATTENTION says.  LIA_ERR_INVALID, by name: a policy other than 3 or a host cache,
 * T == 1, lia_layer_forward_last, rows beyond the table, lens[b] outside 1 .. pos0, lens[b] + T > smax, starts[b] > lens[b], a
 * shape lia_attn_block_takes rejects.  lia_decode_layers (T == 1) is refused the same way.
 * lia_attn_block_takes: 1 when the block attention launches take T queries per row whose last one sees S keys (S = pos0 + T;
 * ragged: max(lens) + T) -- the launches' own rule: head_dim 32 / 64 / 128, heads % kv_heads == 0, T >= 2, S - T >= 1,
 * (heads / kv_heads) * T <= 16, scores and partial outputs within 160 KB of LDS.
 * lia_embed_ragged: lia_embed_padded's kernel with position lens[b] + t - starts[b] + 2 for block token t of row b.  lens, starts:
 * DEVICE pointers, B entries (row b <-> b0 + b); starts may be NULL (all zeros). */
int lia_ctx_set_row_lens(lia_ctx* ctx, const int32_t* lens_host, int n_rows);
int lia_attn_block_takes(int heads, int kv_heads, int head_dim, int T, int S);
int lia_embed_ragged(const int64_t* ids, const lia_bf16* tok, const lia_bf16* pos, lia_bf16* y, int B, int T, int H,
                     const int32_t* lens_device, const int32_t* starts_device, void* stream);
/* ---- allowed-token masks (build-defined; DESIGN.md "Constrained decoding"): restrict which tokens a row may emit -- HF's
 * prefix_allowed_tokens_fn / suppress_tokens / bad_words_ids, a grammar engine's packed bitmask.
 * A mask row is W = ceil(vocab / 32) int32 words in DEVICE memory; token i is allowed iff bit i & 31 of word i >> 5 is 1 (little
 * endian: tokens 8j .. 8j + 7 are byte j of the row -- xgrammar's layout); bits at or beyond vocab are ignored.  A token that is
 * not allowed COUNTS AS -inf, exactly as suppress_token does, and the two compose: in the greedy argmax (the first maximal index
 * among the rest) and in the sampler (no mass, never kept by top-k or top-p).  Every masked head call gives bit for bit what the
 * same call without a table gives on logits whose disallowed entries were overwritten with bf16 -inf.  The logits a head writes
 * (logits, logits_out) stay the raw ones.  A row that allows no token is the caller's to refuse; the kernels do not define it.
 * lia_ctx_set_token_mask: the table -- row r at mask_device + r * ldm_words, `rows` of them; ldm_words = 0: ONE row serves every row
 * of every call.  NULL or rows == 0 clears it.  The context keeps the POINTER only: the caller owns the memory and keeps it alive
 * and unchanged until the compute stream has passed the head call (nothing is copied, nothing synchronises).  WHILE A TABLE IS SET
 * lia_lm_head, lia_llama_lm_head, lia_sample, lia_lm_verify, lia_lm_verify_rows, lia_llama_lm_verify, lia_lm_verify_sample and
 * lia_llama_lm_verify_sample run the masked instantiations of their kernels and row i of the call reads table row i -- for the
 * verify heads i = b * T + t, whichever workspace chunk the row falls into.  Without a table every one of them is the unmasked call,
 * unchanged.  LIA_ERR_INVALID, by name: rows or ldm_words < 0 or a pointer that is not 4-byte aligned (here); at the head call an
 * ldm_words that is neither 0 nor >= ceil(vocab / 32), a call with more rows than the table (ldm_words != 0); lia_lm_verify_reject
 * and lia_llama_lm_verify_reject while a table is set (the drafter's Q would have to be masked the same way).  lia_token_logprobs and
 * the lm_score calls do not look at the table. */
int lia_ctx_set_token_mask(lia_ctx* ctx, const int32_t* mask_device, long ldm_words, int rows);
/* final LN on the last position + tied lm_head + greedy argmax: modeling_opt.py:1563, models.py:424-431,
 * greedy_search.py:367,395.  logits [B,vocab], next_ids [B] (device).  suppress_token >= 0: that token's score
 * counts as -inf (EOS while min_new_tokens is unmet, run_generation.py:173,179-182); -1: none.  Any B >= 1: rows are independent and
 * go through in chunks of 256 (the workspace need is that of min(B, 256) rows); row i reads row i of a token mask, a log-probability
 * sink and the penalties' tables, whichever chunk it falls into, and those are checked against the whole B before anything is launched. */
int lia_lm_head(lia_ctx* ctx, const lia_bf16* hidden, int B, int T, int H, const lia_bf16* lnw, const lia_bf16* lnb,
                const lia_bf16* emb, int vocab, float eps, int suppress_token, lia_bf16* logits, int64_t* next_ids,
                void* stream);

/* sampled decoding: HF's MinNewTokensLength -> Temperature -> TopK -> TopP -> multinomial, one draw per row of logits [B, ld]
 * (bf16, as lia_lm_head / lia_llama_lm_head write them; DESIGN.md "Sampled decoding").  Per row: s = fp32(l) / temperature
 * (s[suppress_token] = -inf); top_k > 0 and < vocab keeps every token with s >= the k-th largest s; top_p < 1 keeps, of those,
 * every token whose tokens of strictly larger s hold < top_p of the kept mass exp(s - max s); the result is the smallest kept id
 * whose running mass in id order exceeds uniforms[row] * the kept mass (the last kept id if rounding leaves none).  A token with
 * s = -inf is never kept.  uniforms: device, B floats in [0, 1); next_ids: device, B; stats: device, B x 4 floats or NULL --
 * per row t_k (-inf with top-k off), the top-p boundary s (-inf with top-p off), the kept count and the kept mass.
 * LIA_ERR_INVALID, by name: temperature <= 0 or not finite, top_k < 0, top_p not in (0, 1], B <= 0, vocab <= 0 or > 2^21,
 * ld < vocab, suppress_token not -1 or in [0, vocab), a NULL logits / uniforms / next_ids. */
int lia_sample(lia_ctx* ctx, const lia_bf16* logits, long ld, int B, int vocab, float temperature, int top_k, float top_p,
               int suppress_token, const float* uniforms, int64_t* next_ids, float* stats, void* stream);

/* ---- scoring (DESIGN.md "Scoring"): per-token log-probabilities instead of the last position's logits ---------------------
 * lia_token_logprobs: per row r of logits [M, ld] (bf16, device, ld >= vocab; columns >= vocab are never read), on the logits
 * read as fp32:  m = max_j l_j,  s = sum_j exp(l_j - m),  logprobs[r] = l_target - (m + log s)  with target = targets[r]
 * (int64, device; -1 = no target -> 0.0; any other value outside [0, vocab) is treated as -1: the ids live on the device, the
 * caller validates them against the vocabulary) and greedy_ids[r] = the first index holding m (lia_lm_head's tie rule).
 * logprobs: fp32 [M], greedy_ids: int64 [M], device.  -inf logits carry no mass.  One LIA_SCORE_ROW_THREADS workgroup per row;
 * a lane adds at most LIA_SCORE_SERIAL(vocab) terms of s before the balanced tree over the lanes.
 * LIA_ERR_INVALID, by name: a NULL logits / targets / logprobs / greedy_ids, M <= 0, vocab <= 0, ld < vocab. */
#define LIA_SCORE_ROW_THREADS 1024
#define LIA_SCORE_SERIAL(vocab) (8 * (((vocab) + 8 * LIA_SCORE_ROW_THREADS - 1) / (8 * LIA_SCORE_ROW_THREADS)))
int lia_token_logprobs(lia_ctx* ctx, const lia_bf16* logits, long ld, int M, int vocab, const int64_t* targets, float* logprobs,
                       int64_t* greedy_ids, void* stream);
/* lia_lm_score / lia_llama_lm_score: final LayerNorm / RMSNorm of EVERY row of hidden [M, ldh] (ldh >= H), the lm_head GEMM
 * (one bf16 rounding of the fp32 accumulator, as lia_lm_head rounds; never split over K, so a row's logits do not depend on the
 * workspace or on the rows beside it inside one GEMM kernel), then lia_token_logprobs.  Any M >= 1; vocab % 16 == 0, H % 64 == 0.
 * The [M, vocab] logits are never materialised as a whole.  CHUNK RULE: rows go through in chunks of
 *     c = min(M, LIA_SCORE_MAX_CHUNK, (workspace_bytes - 512) / (2 H + 2 vocab))   rows,
 * rounded down to a multiple of 256 when c < M: the context's workspace holds one chunk's normed rows [c, H] and its logits
 * [c, vocab], nothing else.  LIA_ERR_MEMORY (with a message, before anything is launched) when c < min(M, 256).
 * lia_lm_score_chunk_rows returns c (0: does not fit); lia_lm_score_workspace_bytes what the largest useful chunk needs. */
#define LIA_SCORE_MAX_CHUNK 4096
int lia_lm_score_chunk_rows(size_t workspace_bytes, int M, int H, int vocab);
size_t lia_lm_score_workspace_bytes(int M, int H, int vocab);
int lia_lm_score(lia_ctx* ctx, const lia_bf16* hidden, long ldh, int M, int H, const lia_bf16* lnw, const lia_bf16* lnb,
                 const lia_bf16* emb, int vocab, float eps, const int64_t* targets, float* logprobs, int64_t* greedy_ids,
                 void* stream);
int lia_llama_lm_score(lia_ctx* ctx, const lia_bf16* hidden, long ldh, int M, int H, const lia_bf16* normw, const lia_bf16* lm,
                       int vocab, float eps, const int64_t* targets, float* logprobs, int64_t* greedy_ids, void* stream);
/* ---- log-probabilities of emitted tokens with their top-N alternatives (build-defined) -------------------------
 * lia_topn_logprobs (the bare kernel): per row r of logits [M, ld] (bf16, device, ld >= vocab >= 1), under the MODEL'S OWN
 * distribution -- the fp32 log-softmax of the raw logits; no temperature, top-k / top-p, suppress_token or token mask:
 *   chosen[r]                = l[ids[r]] - (m + log s), bit for bit lia_token_logprobs' value for targets = ids (an id outside
 *                              [0, vocab) gives 0.0)
 *   top_ids[r, 0 .. n_top)   = the n_top tokens of largest logit, by logit descending, ties by the lower id; the order of a row is
 *                              that of the sampler's 16-bit key of the bf16 pattern (so +0.0 sorts above -0.0)
 *   top_logprobs[r, j]       = l_j - (m + log s) of top_ids[r, j], the same expression; a -inf logit gives -inf and is listed only
 *                              when fewer than n_top logits are finite
 * chosen: fp32 [M]; top_ids: int64 [M, n_top]; top_logprobs: fp32 [M, n_top]; ids: int64 [M]; all device, rows n_top apart.
 * n_top in [0, LIA_LOGPROB_MAX_TOP] and <= vocab; top_ids / top_logprobs may be NULL only with n_top = 0.  The selection is exact
 * (integer histograms of the key, prefix sums in id order) and the same in every run.  Logits are finite or +-inf, not NaN.
 * LIA_ERR_INVALID, by name: a NULL logits / ids / chosen, M <= 0, vocab <= 0, ld < vocab, n_top outside the range or > vocab, a
 * NULL top array with n_top > 0.
 * lia_ctx_set_logprob_sink: where the head calls leave these values.  The context keeps the POINTERS only: device memory the caller
 * owns and keeps alive until the compute stream has passed the head call (nothing is copied, nothing synchronises); `rows` rows.
 * chosen == NULL clears the sink.  WHILE A SINK IS SET lia_lm_head, lia_llama_lm_head, lia_sample, lia_lm_verify,
 * lia_lm_verify_rows, lia_llama_lm_verify, lia_lm_verify_sample and lia_llama_lm_verify_sample run the kernel behind their own id
 * kernel on the logits they have in hand, with ids = the head's own output for the row (the argmax, the draw, the greedy / sampled
 * id of each block position); row i of the call writes sink row i -- for the verify heads i = b * T + t, whichever workspace chunk
 * the row falls into.  lia_sample rewrites the rows lia_lm_head wrote, with the sampled id as chosen.  The heads' own outputs are
 * byte for byte those of the call without a sink; without a sink every head launches exactly what it launched before.
 * LIA_ERR_INVALID, by name, before anything is launched: n_top outside [0, LIA_LOGPROB_MAX_TOP], rows < 1 or a NULL top array
 * with n_top > 0 (here); at the head call n_top > vocab or a call with more rows than the sink; lia_lm_verify_reject,
 * lia_llama_lm_verify_reject, lia_lm_score and lia_llama_lm_score while a sink is set.  lia_token_logprobs and lia_topn_logprobs
 * do not look at the sink. */
#define LIA_LOGPROB_MAX_TOP 32
int lia_ctx_set_logprob_sink(lia_ctx* ctx, int n_top, float* chosen, int64_t* top_ids, float* top_logprobs, long rows);
int lia_topn_logprobs(lia_ctx* ctx, const lia_bf16* logits, long ld, int M, int vocab, const int64_t* ids, int n_top,
                      float* chosen, int64_t* top_ids, float* top_logprobs, void* stream);
/* ---- repetition, presence and frequency penalties (build-defined): the penalties that depend on a row's own token
 * history -- HF's repetition_penalty, OpenAI's / vLLM's presence_penalty and frequency_penalty.
 * A row's state is its COUNT ROW in DEVICE memory, one uint16 word per token: bit 15 = the token occurs in the prompt, bits 0..14 =
 * n, how often it was generated so far, saturating at 32767.  A table is `rows` count rows ldc words apart; its base is 4-byte
 * aligned and ldc even (two words share a 32-bit location, which the updates address atomically) and >= vocab.
 * With theta = repetition (> 0; 1: off), alpha_p = presence, alpha_f = frequency (0: off), token i of a row with word c and raw
 * bf16 logit l counts as, in fp32 and with every operation rounded on its own (no FMA, a correctly rounded division):
 *   x = fp32(l);  if (c != 0) x = x < 0 ? x * theta : x / theta;  n = c & 0x7fff;  x = x - alpha_f * float(n);
 *   x = x - (n > 0 ? alpha_p : 0);  bf16_round_to_nearest_even(x)
 * +-inf stay +-inf; NaN logits and fp32-subnormal intermediates are not defined.
 * lia_token_counts_add: ids [rows, n] (int64, device, ldi apart) are added to table rows 0 .. rows - 1.  generated = 0: bit 15 of the
 *   id's word is set; 1: its count grows by one (saturating).  first (int32 [rows], device, or NULL): positions t < first[b] of row b
 *   are skipped (left padding); active (int32 [rows], device, or NULL): a row with 0 is skipped (finished rows).  An id outside
 *   [0, vocab) is ignored; the same id several times in a row counts that often; no other word changes.
 * lia_apply_penalties: out [M, ldo] = the rows of logits [M, ld] rewritten with the values above under counts [M, ldc]; out ==
 *   logits (in place) is allowed.  16-byte loads and stores when the three bases are 16-byte aligned and ld, ldc, ldo multiples of 8.
 * lia_ctx_set_penalties: the context keeps the POINTERS only -- the table and a scratch of rows x lds bf16 values (lds >= vocab), both
 *   the caller's, alive and (the table) unchanged until the compute stream has passed the head call.  counts == NULL clears it.  WHILE
 *   IT IS SET lia_lm_head, lia_llama_lm_head and lia_sample run the penalty kernel from the logits they have in hand into the scratch
 *   and their id kernel -- the masked instantiation while a token mask is set too -- on the scratch; row i of the call reads table row
 *   i and writes scratch row i.  A penalised call gives, bit for bit, what the same call without penalties gives on logits rewritten
 *   with the values above.  The logits a head writes stay the raw ones, and a log-probability sink still reads the raw logits: the
 *   model's own distribution, with the penalised id as chosen.  Without it every head launches exactly what it launched before.
 * LIA_ERR_INVALID, by name, before anything is launched: repetition not finite or <= 0, presence or frequency not finite, an odd or
 * non-positive ldc, a table that is not 4-byte aligned, ldc < vocab, ld / ldo < vocab, generated outside {0, 1}, ldi < n, rows or M
 * < 1, a NULL scratch with a table; at the head call ldc < vocab, lds < vocab or a call with more rows than the table; every verify
 * head (lia_lm_verify, lia_lm_verify_rows, lia_lm_verify_sample, lia_lm_verify_reject and the lia_llama_ forms: each block position
 * would need its own counts) and lia_lm_score / lia_llama_lm_score while penalties are set. */
int lia_token_counts_add(lia_ctx* ctx, uint16_t* counts, long ldc, int rows, int vocab, const int64_t* ids, long ldi, int n,
                         const int32_t* first, const int32_t* active, int generated, void* stream);
int lia_apply_penalties(lia_ctx* ctx, const lia_bf16* logits, long ld, int M, int vocab, const uint16_t* counts, long ldc,
                        float repetition, float presence, float frequency, lia_bf16* out, long ldo, void* stream);
int lia_ctx_set_penalties(lia_ctx* ctx, const uint16_t* counts, long ldc, int rows, float repetition, float presence, float frequency,
                          lia_bf16* scratch, long lds);
/* ---- speculative verification: the greedy token behind every position of a draft block, and how much of the
 * draft it confirms.  hidden [B * T, ldh]: the last layer's output for the block [pending | d_1 .. d_{T-1}] of every row.
 * Final norm + lm_head GEMM per chunk exactly as lia_lm_score (same CHUNK RULE, same workspace, logits never materialised), then
 *   greedy[b, t]  = first index of the row's maximum (lia_lm_head's tie rule); suppress_token >= 0 counts as -inf at t < n_suppress
 *   accepted[b]   = the largest a <= T - 1 with block_ids[b, i + 1] == greedy[b, i] for all i < a; T - 1 where active[b] == 0
 *   common[0]     = min_b accepted[b]          next[b] = greedy[b, common]
 * block_ids: int64 [B, T]; active: int32 [B] or NULL (all active); greedy: int64 [B, T]; accepted, common: int32 [B], [1]; next:
 * int64 [B] -- all on the device.  LIA_ERR_INVALID, by name: a NULL tensor other than active, B <= 0, T < 2, n_suppress outside
 * [0, T], suppress_token not -1 or in [0, vocab), H % 64, vocab % 16, ldh < H or ldh % 8.  LIA_ERR_MEMORY as lia_lm_score. */
int lia_lm_verify(lia_ctx* ctx, const lia_bf16* hidden, long ldh, int B, int T, int H, const lia_bf16* lnw, const lia_bf16* lnb,
                  const lia_bf16* emb, int vocab, float eps, int suppress_token, int n_suppress, const int64_t* block_ids,
                  const int32_t* active, int64_t* greedy, int32_t* accepted, int32_t* common, int64_t* next, void* stream);
int lia_llama_lm_verify(lia_ctx* ctx, const lia_bf16* hidden, long ldh, int B, int T, int H, const lia_bf16* normw,
                        const lia_bf16* lm, int vocab, float eps, int suppress_token, int n_suppress, const int64_t* block_ids,
                        const int32_t* active, int64_t* greedy, int32_t* accepted, int32_t* common, int64_t* next, void* stream);
/* lia_lm_verify with a bound per row (build-defined, row mode): suppress_token counts as -inf at block positions t < n_suppress_rows[b]
 * (int32 [B], device, each in [0, T]; NULL is refused by name).  Everything else, common and next included, as lia_lm_verify. */
int lia_lm_verify_rows(lia_ctx* ctx, const lia_bf16* hidden, long ldh, int B, int T, int H, const lia_bf16* lnw, const lia_bf16* lnb,
                       const lia_bf16* emb, int vocab, float eps, int suppress_token, const int32_t* n_suppress_rows,
                       const int64_t* block_ids, const int32_t* active, int64_t* greedy, int32_t* accepted, int32_t* common,
                       int64_t* next, void* stream);
/* ---- sampled verification ("Sampled verification"): lia_lm_verify with lia_sample's draw in place of the argmax.
 * Plain sampled decoding emits  lia_sample(logits(prefix), U[step, row])  per step; a verify pass evaluates that same function behind
 * every position of the block.  Per chunk (lia_lm_score's CHUNK RULE and workspace), for block row b at position t:
 *   suppress_token counts as -inf where t < n_suppress_rows[b] (int32 [B], device) -- or, with a NULL n_suppress_rows, t < n_suppress
 *   s = (step_rows ? step_rows[b] : step0) + t        u = s < n_steps ? uniforms[s * ldu + b] : 0   (nothing is read past the table:
 *       such a position can never be kept)
 *   sampled[b, t] = lia_sample's id for these logits, settings and u -- the same device function, the same bits; no argmax runs
 *   p_draft[b, t] (fp32 [B, T], device, or NULL) = the probability that this draw confirms the draft token block_ids[b, t + 1]: its
 *       kept weight exp(s - max s) over the kept mass; 0 where that token is not kept (or no token id), and 0 at t = T - 1
 * then accepted / common / next exactly as lia_lm_verify computes them, on `sampled`.
 * logits_out (bf16 [B * T, vocab], device, or NULL): each chunk's logits are copied out on `stream` before the next chunk overwrites
 * them -- for tests and measurements; NULL in production.
 * lia_block_sampler: the settings and the generation's table U (device fp32 [n_steps, ldu], U[step, row]); step_rows: int32 [B],
 * device, or NULL (every row at step0).
 * LIA_ERR_INVALID, by name: every lia_lm_verify refusal; lia_sample's for temperature, top_k, top_p and vocab > 2^21; ldu < B,
 * n_steps < 1, step0 < 0, a NULL sampler, uniforms or sampled.  LIA_ERR_MEMORY as lia_lm_score. */
typedef struct {
  float temperature;
  int top_k;
  float top_p;
  const float* uniforms;
  long ldu;
  int n_steps;
  int step0;
  const int32_t* step_rows;
} lia_block_sampler;
int lia_lm_verify_sample(lia_ctx* ctx, const lia_bf16* hidden, long ldh, int B, int T, int H, const lia_bf16* lnw, const lia_bf16* lnb,
                         const lia_bf16* emb, int vocab, float eps, int suppress_token, int n_suppress, const int32_t* n_suppress_rows,
                         const lia_block_sampler* sampler, const int64_t* block_ids, const int32_t* active, int64_t* sampled,
                         int32_t* accepted, int32_t* common, int64_t* next, float* p_draft, lia_bf16* logits_out, void* stream);
int lia_llama_lm_verify_sample(lia_ctx* ctx, const lia_bf16* hidden, long ldh, int B, int T, int H, const lia_bf16* normw,
                               const lia_bf16* lm, int vocab, float eps, int suppress_token, int n_suppress,
                               const int32_t* n_suppress_rows, const lia_block_sampler* sampler, const int64_t* block_ids,
                               const int32_t* active, int64_t* sampled, int32_t* accepted, int32_t* common, int64_t* next,
                               float* p_draft, lia_bf16* logits_out, void* stream);

/* ---- rejection verification ("Rejection verification"): the verify head for a STOCHASTIC drafter -- the rule of
 * Leviathan et al.  The drafter drew the draft token x = block_ids[b, t + 1] from Q_t, lia_sample's filtered distribution of its own
 * bf16 logits draft_logits[b * ldd_row + t * ldd_pos + i] (t < T - 1) under the target's settings and the target's suppress rule;
 * P_t is the filtered distribution of this pass's logits behind block position t.  Per chunk (lia_lm_score's CHUNK RULE and
 * workspace), for block row b at position t, with s = step0 + t:
 *   p_tok[b, t] = P_t(x), q_tok[b, t] = Q_t(x): kept weight over kept mass, 0 where x is not kept; both 0 at t = T - 1
 *   ok[b, t]    = s < n_steps  and  q_tok > 0  and  u_acc[s * ldu + b] * q_tok < p_tok;   0 at t = T - 1.  A position with s >= n_steps
 *                 reads neither table (u = 0) and is rejected: its token lies beyond the generation's last step
 *   resid_mass[b, t] = R = sum_i r_i,  r_i = max(P_t(i) - Q_t(i), 0);  0 at t = T - 1
 *   token[b, t] = t < T - 1 and R > 0: the smallest id whose running residual mass in id order exceeds u_res[s * ldu + b] * R, else
 *                 the last id with r_i > 0 -- what the round emits if t is its first rejected position;
 *                 t = T - 1 (the bonus token) or R = 0 (P_t = Q_t): lia_sample's id for P_t's row and u_res[s * ldu + b] -- the same
 *                 device function, the same bits
 * then  accepted[b] = the first t with ok[b, t] = 0 (T - 1 where active[b] = 0),  common = min_b accepted[b],
 *       next[b] = accepted[b] > common ? block_ids[b, common + 1] : token[b, common]
 * (a row that accepted the draft token behind `common` keeps it: it is a valid sample).  The emitted tokens are an exact sample of the
 * target's filtered distribution but NOT the ids plain sampling would draw from the same seed.
 * p_tok / q_tok / resid_mass: fp32 [B, T], device, each or NULL.  logits_out as in lia_lm_verify_sample.  Common mode only.
 * LIA_ERR_INVALID, by name: lia_lm_verify_sample's refusals for the shapes, the suppress arguments and the settings; a NULL
 * rejector, draft_logits, u_acc, u_res, token or ok; ldd_row or ldd_pos < vocab; with vocab % 8 == 0 (rows read 16 bytes at a time) a
 * draft_logits that is not 16-byte aligned or a pitch that is no multiple of 8; a non-NULL n_suppress_rows.  LIA_ERR_MEMORY as
 * lia_lm_score. */
typedef struct {
  float temperature;
  int top_k;
  float top_p;
  const float* u_acc;           /* device fp32 [n_steps, ldu], [step, row] */
  const float* u_res;           /* the same shape */
  long ldu;
  int n_steps;
  int step0;
  const lia_bf16* draft_logits; /* device bf16, row b position t at b * ldd_row + t * ldd_pos */
  long ldd_row;
  long ldd_pos;
} lia_block_rejector;
int lia_lm_verify_reject(lia_ctx* ctx, const lia_bf16* hidden, long ldh, int B, int T, int H, const lia_bf16* lnw, const lia_bf16* lnb,
                         const lia_bf16* emb, int vocab, float eps, int suppress_token, int n_suppress, const int32_t* n_suppress_rows,
                         const lia_block_rejector* rejector, const int64_t* block_ids, const int32_t* active, int64_t* token, int32_t* ok,
                         int32_t* accepted, int32_t* common, int64_t* next, float* p_tok, float* q_tok, float* resid_mass,
                         lia_bf16* logits_out, void* stream);
int lia_llama_lm_verify_reject(lia_ctx* ctx, const lia_bf16* hidden, long ldh, int B, int T, int H, const lia_bf16* normw,
                               const lia_bf16* lm, int vocab, float eps, int suppress_token, int n_suppress,
                               const int32_t* n_suppress_rows, const lia_block_rejector* rejector, const int64_t* block_ids,
                               const int32_t* active, int64_t* token, int32_t* ok, int32_t* accepted, int32_t* common, int64_t* next,
                               float* p_tok, float* q_tok, float* resid_mass, lia_bf16* logits_out, void* stream);

/* ---- Llama-family layer (BASELINE.json config 4; build-defined: the reference's LlamaDecoderLayer_forward,
 * decoder.py:121-169, has no policy plumbing -- SURVEY.md quirk 3).  Arithmetic = HF transformers' eager bf16 Llama.
 * weights[9]: 0 input_norm.w  1 q.w [h*d,H]  2 k.w [kvh*d,H]  3 v.w  4 o.w [H,h*d]  5 post_norm.w  6 gate.w [F,H]
 * 7 up.w [F,H]  8 down.w [H,F]; q|k|v and gate|up adjacent in the packed layout.  KV cache on the device, seq-major
 * [smax][batch][kv_heads][head_dim], post-RoPE keys.  cos/sin: [max_pos][head_dim] bf16 tables.
 * gu_block: 0 = gate.w and up.w as they are; 32 (and weights[7] == weights[6] + F*H, ffn % 32 == 0) = the 2F rows of the
 * gate|up block are interleaved, 32 gate rows then the matching 32 up rows -- a 64-column tile of the projection then holds
 * both factors of 32 outputs and the prefill GEMM's epilogue writes silu(gate) * up itself. */
typedef struct {
  int hidden, heads, kv_heads, ffn;
  float rms_eps;
  int gu_block;
} lia_llama_desc;
int lia_llama_pack_offsets(const lia_llama_desc* d, size_t offsets[9], size_t* total_bytes);
size_t lia_llama_workspace_bytes(const lia_llama_desc* d, int max_rows);
int lia_llama_layer_forward(lia_ctx* ctx, const lia_llama_desc* d, const void* const weights[9], const lia_bf16* x, lia_bf16* y,
                            lia_kv* kv, const lia_bf16* cos_table, const lia_bf16* sin_table, int B, int T, int pos0, int b0,
                            void* stream);
/* the Llama counterpart of lia_layer_forward_last: the LAST layer of a prefill -- norm, q | k | v projection and RoPE on every row
 * (the cache holds every position), attention / o / MLP on the last position of each row; y_last: [B, 1, H]; T > 1, any pos0 */
int lia_llama_layer_forward_last(lia_ctx* ctx, const lia_llama_desc* d, const void* const weights[9], const lia_bf16* x,
                                 lia_bf16* y_last, lia_kv* kv, const lia_bf16* cos_table, const lia_bf16* sin_table, int B, int T,
                                 int pos0, int b0, void* stream);
int lia_llama_embed(const int64_t* ids, const lia_bf16* tok, lia_bf16* y, int B, int T, int H, void* stream);
/* lia_lm_head with the final RMSNorm and the untied lm_head of a Llama: any B >= 1, as there */
int lia_llama_lm_head(lia_ctx* ctx, const lia_bf16* hidden, int B, int T, int H, const lia_bf16* normw, const lia_bf16* lm,
                      int vocab, float eps, int suppress_token, lia_bf16* logits, int64_t* next_ids, void* stream);

/* ---- decode step over a run of HBM-resident layers (build-defined fast path of the per-layer loop) ---------------------
 * The reference runs its resident layers one torch op at a time (lia/modeling_opt.py:1246-1260 -> decoder.py:172-335,
 * attentions.py:393-529: ~10 launches per layer).  These two entry points run n_layers CONSECUTIVE resident layers of one decode
 * step (T == 1, KV cache in HBM = policy 3 arithmetic) in ONE library call: lia_layer_forward(policy 3) /
 * lia_llama_layer_forward layer by layer, every layer's closing norm chained into the next (lia_ctx_chain_next_norm), the
 * hidden state alternating between y and a context-owned buffer so that x is never written.  (r04 also offered a persistent
 * one-kernel-per-layer route behind a switch: bit-identical, measured 4-9 % slower per step, retired in r05 -- LABNOTES.md.)
 *   weights: n_layers x 16 (OPT) / n_layers x 9 (Llama) device pointers, layer-major;  kv: n_layers pointers to device caches
 *   x: [B, 1, H] input (never written);  y: [B, 1, H] result;  B <= cache batch, rows [0, B) of the caches are served */
int lia_decode_layers(lia_ctx* ctx, const lia_layer_desc* d, int n_layers, const void* const* weights, const lia_bf16* x,
                      lia_bf16* y, lia_kv* const* kv, int B, int pos0, void* stream);
int lia_llama_decode_layers(lia_ctx* ctx, const lia_llama_desc* d, int n_layers, const void* const* weights, const lia_bf16* x,
                            lia_bf16* y, lia_kv* const* kv, const lia_bf16* cos_table, const lia_bf16* sin_table, int B, int pos0,
                            void* stream);
/* Per-context options and counters.  The library keeps no process-wide setting: two contexts of one process may differ.
 *   LIA_OPT_FUSE_COMBINE (default 1): the split-K combine of a decode GEMM also runs the op behind it (LayerNorm / RMSNorm of the
 *     finished row, SiLU(gate) * up, RoPE); 0: every such op is a kernel of its own -- the same device functions on the same
 *     values, so the two routes agree bit for bit (tests/test_gpu_fused_combine.py).
 *   lia_ctx_get_counter(ctx, LIA_CNT_FUSED_COMBINE + kind), kind = 1 LayerNorm, 2 RMSNorm, 3 SiLU*up, 4 RoPE: fused combines
 *     launched through this context (tests assert the route was taken); -1 for an unknown key.
 *   LIA_OPT_BLOCK_ATTENTION (default 0): a block of T > 1 queries behind a non-empty cache takes the decode-shaped block
 *     attention kernel where (heads / kv_heads) * T <= 16 and its scores fit the LDS, the append kernels otherwise; row t is then
 *     bit for bit the decode attention over pos0 + t + 1 keys.  The speculative verify pass sets it around its layer calls, for
 *     the shapes where the kernel was measured faster (speculative.block_attention_pays).
 *   lia_ctx_get_counter(ctx, LIA_CNT_BLOCK_ATTENTION): block attention launches through this context.
 *   LIA_OPT_SPLIT_DECODE (default 0): 1 = a decode-shaped attention (one query per row: T == 1, or the _last operators) over
 *     S > lia_attn_split_chunk(head_dim) keys takes the split-key route -- the row's keys cut into chunks of that many keys, one
 *     workgroup per (chunk, KV head, row), fp32 partial outputs added in chunk order; scores, softmax and every rounding point are
 *     the one-workgroup kernel's, only the fp32 order of the P.V sum differs.  Whatever the option says, a layer call takes that
 *     route where the one-workgroup kernel cannot hold the row's scores in LDS (S beyond ~4.6k keys at 8 query heads per KV head,
 *     ~9.7k at 4, ~39k at 1), so a decode step has no limit on S.  The route's scratch, lia_attn_split_scratch_bytes(B, S, heads,
 *     kv_heads, head_dim) bytes, lies in the context's workspace behind the layer call's own layout (lia_layer_workspace_bytes /
 *     lia_llama_workspace_bytes of the call's rows): where it does not fit, a call sent there by the option alone takes the
 *     one-workgroup kernel, and a call beyond that kernel returns LIA_ERR_MEMORY, naming the bytes, before anything is launched.
 *   lia_ctx_get_counter(ctx, LIA_CNT_SPLIT_DECODE): split-key launches through this context. */
enum { LIA_OPT_FUSE_COMBINE = 1, LIA_OPT_BLOCK_ATTENTION = 2, LIA_OPT_SPLIT_DECODE = 3 };
enum { LIA_CNT_FUSED_COMBINE = 100, LIA_CNT_BLOCK_ATTENTION = 200, LIA_CNT_SPLIT_DECODE = 300 };
int lia_ctx_set_option(lia_ctx* ctx, int key, long value);
long lia_ctx_get_counter(lia_ctx* ctx, int key);
/* Pure host arithmetic (no GPU is touched).  lia_attn_split_chunk: the keys per chunk of the split-key route, one constant per
 * head_dim (32 / 64 / 128; 0 for any other).  lia_attn_split_scratch_bytes: the scratch of one split-key attention over B rows of
 * S keys, a multiple of 256: bf16 scores [B][heads][chunks * chunk], fp32 chunk maxima [B][heads][chunks] and fp32 partial outputs
 * [chunks][B][heads][head_dim], each rounded up to 256 bytes; 0 for a shape the route does not take. */
int lia_attn_split_chunk(int head_dim);
size_t lia_attn_split_scratch_bytes(int B, int S, int heads, int kv_heads, int head_dim);

/* ---- host side of the cooperative policies -------------------------------------------------------
 * Indirect-access-KV masked MHA, csrc/cpu/aten/kernels/MaskedMultiHeadAttentionKrnl.cpp:513-842: fp32
 * scores / softmax / weighted sum over a host cache, new K/V rows written in place.  q,k,v: [B,T,h*d]
 * host; cache [smax][cache_batch][h][d] host; rows pos0.. written, 0..pos0+T-1 attended. */
int lia_host_attention(const lia_bf16* q, const lia_bf16* k, const lia_bf16* v, lia_bf16* kcache, lia_bf16* vcache,
                       lia_bf16* out, int B, int T, int pos0, int heads, int head_dim, int cache_batch, int b0,
                       int n_threads);
/* the same over a left-padded batch (the reference's additive padding mask, mha_fusion.py:532-566): served row b attends keys
 * starts[b] .. pos0 + t, a query at a pad position gives a zero row.  starts: HOST, B entries, 0 <= starts[b] <= pos0 + T - 1. */
int lia_host_attention_padded(const lia_bf16* q, const lia_bf16* k, const lia_bf16* v, lia_bf16* kcache, lia_bf16* vcache,
                              lia_bf16* out, int B, int T, int pos0, int heads, int head_dim, int cache_batch, int b0,
                              int n_threads, const int32_t* starts);

/* policy 1, "compute everything on CPU" (modeling_opt.py:1168): the same layer entirely on the host cores.  The
 * reference routes it through IPEX (tpp_linear_bias/_relu/_add, TPPGEMMKrnl.h:89-176,671-765,858-951 + the masked
 * MHA kernel); here AVX-512(-BF16) code in the same library.  All pointers are HOST pointers; weights row-major. */
int lia_host_layer_forward(const lia_layer_desc* d, const void* const weights[16], const lia_bf16* x, lia_bf16* y,
                           lia_bf16* kcache, lia_bf16* vcache, int smax, int cache_batch, int B, int T, int pos0, int b0,
                           int n_threads);
/* The decode step of policy 1 over n_layers CONSECUTIVE layers (the reference's loop over decoder layers with every layer on the
 * CPU, modeling_opt.py:1545-1555) in one OpenMP region: weights = n_layers x 16 host pointers, kcaches / vcaches = n_layers host
 * caches; the hidden state ping-pongs between x and y (both are written).  B * T <= 256.  Returns 0 if the result is in x,
 * 1 if it is in y, a negative LIA_ERR_* code on error. */
int lia_host_layers_forward(const lia_layer_desc* d, int n_layers, const void* const* weights, lia_bf16* x, lia_bf16* y,
                            void* const* kcaches, void* const* vcaches, int smax, int cache_batch, int B, int T, int pos0,
                            int b0, int n_threads);
/* policy 1 over a left-padded batch (lia/modeling_opt.py:1133 + mha_fusion.py:532-566 on the CPU branch): the attention of
 * lia_host_attention_padded inside; starts: HOST, B entries for the served rows (no context here, so an explicit argument) */
int lia_host_layer_forward_padded(const lia_layer_desc* d, const void* const weights[16], const lia_bf16* x, lia_bf16* y,
                                  lia_bf16* kcache, lia_bf16* vcache, int smax, int cache_batch, int B, int T, int pos0, int b0,
                                  int n_threads, const int32_t* starts);
int lia_host_layers_forward_padded(const lia_layer_desc* d, int n_layers, const void* const* weights, lia_bf16* x, lia_bf16* y,
                                   void* const* kcaches, void* const* vcaches, int smax, int cache_batch, int B, int T, int pos0,
                                   int b0, int n_threads, const int32_t* starts);
int lia_host_layernorm(const lia_bf16* x, const lia_bf16* g, const lia_bf16* b, lia_bf16* y, long rows, int H, float eps,
                       int n_threads);
int lia_host_linear(const lia_bf16* x, const lia_bf16* w, const lia_bf16* bias, const lia_bf16* residual, lia_bf16* y, long M,
                    int N, int K, int relu, int n_threads);
int lia_host_has_avx512_bf16(void);
/* Per-thread scratch of the host kernels (fp32 C tiles of the linears, score rows of the attention) is refused above this many
 * bytes (0 = no limit, the default) in lia_host_* calls made BY THE CALLING THREAD from now on: the call that needed it returns
 * LIA_ERR_MEMORY -- as it does when the allocation itself fails in a worker thread -- instead of running the box out of memory.
 * Thread-local, like lia_last_error: callers on other threads are not affected. */
void lia_host_thread_scratch_limit(size_t bytes_per_thread);

/* ---- weight streamer ------------------------------------------------------------------------------
 * Replaces load_layer / layer_copy under torch.cuda.stream(load_weight_stream) + device-wide syncs
 * (modeling_opt.py:270-318,1287-1312,1508-1515): n_slots HBM slots, one pinned hipMemcpyAsync per packed
 * layer on a dedicated copy stream, event handshakes with the compute stream. */
int lia_stream_create(lia_ctx* ctx, int n_slots, size_t slot_bytes, lia_streamer** out);
void lia_stream_destroy(lia_streamer* s);
void* lia_stream_slot_ptr(lia_streamer* s, int slot);
/* enqueue host -> slot; first waits (on the copy stream) until the slot's last consumer released it.
 * pinned = 0 stages through the streamer's two pinned 64 MiB bounce buffers -- a team memcpy fills one while the copy engine drains
 * the other -- (the reference's cpu_buff path,
 * modeling_opt.py:1219-1220, 1289-1292). */
int lia_stream_prefetch(lia_streamer* s, int slot, const void* host_ptr, size_t bytes, int pinned);
/* the same in three steps, for callers that put work of their own (an RCCL broadcast of each chunk to the
 * data-parallel peers) between the host copy and the moment the slot is declared ready */
int lia_stream_begin(lia_streamer* s, int slot);
int lia_stream_copy_chunk(lia_streamer* s, int slot, size_t offset, const void* host_ptr, size_t bytes, int pinned);
int lia_stream_mark_ready(lia_streamer* s, int slot);
/* pack10: a lossless wire format for the streamed bf16 layers (lia_pack10.hip; build-defined: the reference ships raw bf16).  One
 * byte sign|mantissa per value + a three-level exponent code (2-bit level-1 planes for the three most frequent exponents of a
 * 65536-value region, a compacted 2-bit level 2 for the next three, a 4-bit level 3; two per-1024-value offset tables): 10.8 bits
 * per value for N(0,sigma) weights, against an exponent-entropy bound of 10.55.  The host keeps / ships the encoded bytes, a kernel
 * on a side stream rebuilds the exact bf16 layer in the slot.  n_values must be a multiple of 1024.  encode returns 0, or 1 when
 * the layer does not fit the format and must travel raw. */
size_t lia_pack10_bound(size_t n_values);
int lia_pack10_encode(const lia_bf16* src_device, size_t n_values, char* dst_device, size_t dst_capacity, size_t* out_bytes);
/* Host-side consistency check of an encoded buffer (`header_host`: all staged_bytes of it): the header (magic, version, value
 * count == the slot's, every offset inside `staged_bytes`, counts within their capacities), then the region and offset tables
 * and the escape records -- run when a packed layer is mapped from a checkpoint file or pinned, because the decode kernel takes
 * its loop bounds and offsets from the header and its stream positions from the tables.  0 = consistent, negative = the failed
 * check (LIA_P10_*). */
int lia_pack10_validate(const void* header_host, size_t staged_bytes, size_t n_values);
/* lia_pack10_validate's codes.  The checks beyond the header read the region tables, the two offset tables, the last block's
 * planes and level-2 codes and the escape records (O(n / 1024 + n_esc)), never beyond staged_bytes; they bound every address
 * the decode and patch kernels form, provided the decode reads from a staging buffer of lia_pack10_bound(n_values) bytes. */
#define LIA_P10_SHORT (-1)    /* NULL, or fewer than 256 staged bytes                                                      */
#define LIA_P10_FORMAT (-2)   /* magic / version                                                                           */
#define LIA_P10_COUNT (-3)    /* value count / region count differs from the slot's                                        */
#define LIA_P10_OFFSET (-4)   /* a section outside staged_bytes, overlapping the next or not 256-byte aligned; staged_bytes
                                 or a stream's read window beyond lia_pack10_bound(n_values)                               */
#define LIA_P10_CAPACITY (-5) /* a count beyond its capacity, or the overflow flag                                         */
#define LIA_P10_REGION (-6)   /* a region table with e3 outside 1..242 or a symbol twice                                   */
#define LIA_P10_TABLE (-7)    /* tab2 / tab3 not starting at 0, decreasing, stepping by more than 1024 (tab3 by more than
                                 tab2), far from n_l2 / n_l3, or the last block's counts disagree with its planes / codes  */
#define LIA_P10_ESCAPE (-8)   /* more escape records than level-3 codes, or a record index >= n_values                     */
/* Rebuild the raw bf16 values of an encoded buffer (device -> device), asynchronous on `stream` (NULL = the default
 * stream): the kernels the streamer runs, exposed for re-tiering a layer that the host holds in a packed format
 * (model placement, lia/modeling_opt.py:229-268) and for the round-trip tests.  format: the codec the buffer holds, LIA_WIRE_PACK10
 * or LIA_WIRE_PACK10A (lia_pack_codec reads it from a host copy's header); a call with another codec than the bytes hold decodes
 * garbage, one with any other value is refused.  A buffer that its codec's validator passed is decoded without a read outside
 * src_device when src_device holds lia_pack10_bound(n_values) bytes. */
int lia_pack_decode(const char* src_device, lia_bf16* dst_device, size_t n_values, int format, void* stream);
/* pack10a: the second codec of the pack10 wire family (lia_pack10a.hip): the same sign|mantissa byte plane, the exponents of every
 * 65536-value chunk coded by a 64-lane interleaved range-ANS coder (32-bit states, 16-bit words, one word stream per chunk) against
 * a 10-bit frequency table built per chunk over the exponents present in it -- 10.59 bits per value for N(0,sigma) weights.  Every
 * exponent has a code (no escape records).  Buffer: [header 256][directory: (chunks + 1) x {u32 first word, u32 first table
 * entry}][table entries u32: exponent | (f - 1) << 8][final states: chunks x 64 u32][sign|mantissa plane][u16 words].
 * "pack10" as a wire format names the family; the codec of a buffer is told by its header.
 * encode: as lia_pack10_encode (dst_capacity >= lia_pack10_bound(n_values)); returns 1 when the encoding would not fit
 * lia_pack10_bound(n_values), the size of every staging buffer, or is not smaller than max_bytes (0: no limit) -- the caller then
 * ships what it has (pack10 v2, or raw). */
#define LIA_WIRE_PACK10 10
#define LIA_WIRE_PACK10A 0x10a
int lia_pack10a_encode(const lia_bf16* src_device, size_t n_values, char* dst_device, size_t dst_capacity, size_t max_bytes, size_t* out_bytes);
/* Host-side consistency check, the counterpart of lia_pack10_validate (same arguments, same moment): header, sections inside
 * staged_bytes and lia_pack10_bound(n_values), word offsets starting at 0, never decreasing, ending at the stream's length, every
 * chunk's 1..256 frequencies summing to 1024.  O(chunks + table entries).  Returns 0 or LIA_P10_SHORT / _FORMAT / _COUNT / _OFFSET /
 * _TABLE (the directory) / LIA_P10A_FREQ (a frequency table). */
int lia_pack10a_validate(const void* header_host, size_t staged_bytes, size_t n_values);
#define LIA_P10A_FREQ (-9)    /* a chunk's frequencies do not sum to 1024, or its exponents do not ascend                    */
/* the codec of an encoded buffer from its first bytes on the host: LIA_WIRE_PACK10, LIA_WIRE_PACK10A, or 0 (neither) */
int lia_pack_codec(const void* header_host, size_t bytes);
/* format: LIA_WIRE_PACK10 | LIA_WIRE_PACK10A, the codec of the bytes shipped */
int lia_stream_prefetch_packed(lia_streamer* s, int slot, const void* host_ptr, size_t packed_bytes, size_t n_values, int format,
                               int pinned);
int lia_stream_copy_chunk_packed(lia_streamer* s, int slot, size_t offset, const void* host_ptr, size_t bytes, int pinned);
int lia_stream_decode_packed(lia_streamer* s, int slot, size_t n_values, int format);
void* lia_stream_staging_ptr(lia_streamer* s, int slot);
int lia_stream_wait(lia_streamer* s, int slot, void* compute_stream);    /* compute waits for the copy  */
int lia_stream_release(lia_streamer* s, int slot, void* compute_stream); /* slot reusable after this    */
/* bytes copied and copy-engine busy milliseconds since the last reset (hipEvent timing on the copy stream) */
int lia_stream_stats(lia_streamer* s, double* bytes, double* busy_ms, int reset);
/* the same totals without ever blocking: copies still in flight are left for a later call (used inside the token loop by the
 * online cooperative-split controller, which must not wait for the prefetched layers) */
int lia_stream_poll_stats(lia_streamer* s, double* bytes, double* busy_ms);
/* Live timing of the wire-format decode kernel (bench.py's roofline.dominant_kernel; the role rocprofv3's per-kernel average plays
 * in profiles/): launches, summed HIP-event milliseconds around the MAIN decode kernel on the decode stream, encoded bytes read and
 * bf16 bytes written by them since the last reset.  Waits for the decodes still in flight. */
int lia_stream_decode_stats(lia_streamer* s, long* launches, double* ms, double* bytes_in, double* bytes_out, int reset);
/* the same totals without blocking: decodes still in flight are left for a later call (counted into the window they finish in) --
 * what bench.py calls at the edge of its timed region, so that reading the counters does not drain the prefetched layers' decodes
 * right before the first timed step.  (busy_ms of lia_stream_stats includes the staging memcpy for PAGEABLE sources.) */
int lia_stream_poll_decode_stats(lia_streamer* s, long* launches, double* ms, double* bytes_in, double* bytes_out, int reset);
void* lia_stream_copy_stream(lia_streamer* s);
/* Decode mode (build-defined): a decode step is link-bound and its consumer needs a slot for a fraction of a layer's link time, so
 * keep_slots slots serve it and the others idle.  While the mode is on, slots keep_slots .. n_slots - 1 and their staging areas leave
 * the ring and hold layers in their WIRE format -- `capacity` entries, each with room for entry_bytes -- that the decode kernel
 * rebuilds in a kept slot every step without crossing the link again; the staging areas of the kept slots become landing buffers
 * that belong to no slot, so the link runs ahead by landing buffers while the slots cycle through the cached layers.  Nothing is
 * allocated or freed by a mode change, and every hand-over of memory is ordered by events on the copy and decode streams.
 *   capacity: entries that fit; 0 when n_slots <= keep_slots or no packed layer was ever staged (raw wire).
 *   enable: LIA_ERR_INVALID when the capacity is 0 or the mode is on.  Prefetches in flight into slots >= keep_slots are
 *       abandoned by it (their copies and decodes finish first); those into kept slots stay valid.
 *   land: H2D copy of an encoded layer into landing buffer `landing` (< keep_slots), behind the decode that last read it.
 *   decode_landed: landing buffer -> slot (< keep_slots) behind the copy and the slot's last release; the slot is then waited
 *       for and released with lia_stream_wait / lia_stream_release as ever.
 *   decode_cached: entry -> slot; the first call for an entry copies host_ptr into it first (counted by lia_stream_stats like
 *       any copy), later calls (same host_ptr and bytes) copy nothing.  Only layers that their validator passed belong here.
 *   disable: every entry is dropped, slots and staging areas return to the ring behind the mode's last decode.  The legacy packed
 *       entry points are refused while the mode is on; lia_stream_prefetch (a raw layer) works on the kept slots. */
int lia_stream_cache_capacity(lia_streamer* s, int keep_slots, size_t entry_bytes);
int lia_stream_cache_enable(lia_streamer* s, int keep_slots, size_t entry_bytes);
int lia_stream_cache_disable(lia_streamer* s);
int lia_stream_land(lia_streamer* s, int landing, const void* host_ptr, size_t packed_bytes, int pinned);
int lia_stream_decode_landed(lia_streamer* s, int landing, int slot, size_t n_values, int format);
int lia_stream_decode_cached(lia_streamer* s, int entry, int slot, const void* host_ptr, size_t packed_bytes, size_t n_values, int format,
                             int pinned);
/* Where the decode mode's entries lie: a pure host function (no device, no streamer), so that tests and the planner can ask it.
 * The pool has three regions, filled in this order up to LIA_CACHE_MAX_ENTRIES entries in all:
 *   slots:     the bytes of slots keep_slots .. n_slots - 1 of the slot allocation (n_slots x slot_bytes);
 *   staging:   the staging allocation (n_slots x staging_bytes) behind the keep_slots landing buffers.  landing_bytes == 0: a
 *              landing buffer is a whole staging area (the geometry before lia_stream_cache_configure); otherwise landing buffer b
 *              starts at b x landing_stride, landing_stride = landing_bytes + LIA_CACHE_READ_SLACK rounded up to 256;
 *   workspace: bytes [lend_offset, lend_offset + lend_bytes) of the context's workspace, lend_offset rounded up to 256 (the bytes
 *              lost to the rounding come off lend_bytes).  lend_bytes == 0: none.
 * Every entry starts on a multiple of 256 bytes of its allocation, keeps LIA_CACHE_READ_SLACK bytes behind entry_bytes and lies
 * inside one region.  offset[e] is entry e's byte offset from the start of ITS allocation (slots / staging / workspace); entries
 * 0 .. in_slots - 1 are in the slots, the next in_staging in the staging allocation, the next in_workspace in the workspace.
 * Returns LIA_OK -- with n_entries == 0 where the mode has nothing to offer: keep_slots < 1, keep_slots >= n_slots, no staging
 * allocation, entry_bytes == 0 -- or LIA_ERR_INVALID (*out zeroed) for a landing_stride larger than a staging area. */
#define LIA_CACHE_MAX_ENTRIES 64
#define LIA_CACHE_READ_SLACK 4096
typedef struct lia_cache_geometry {
  int n_entries, in_slots, in_staging, in_workspace;
  size_t entry_stride;      /* entry_bytes + LIA_CACHE_READ_SLACK rounded up to 256 */
  size_t landing_stride;    /* distance between two landing buffers in the staging allocation */
  size_t landing_capacity;  /* the largest encoded layer lia_stream_land takes */
  size_t offset[LIA_CACHE_MAX_ENTRIES];
  int in_extra;             /* the last in_extra entries lie in the streamer's extra allocation (lia_cache_geometry_plan_extra) */
} lia_cache_geometry;
int lia_cache_geometry_plan(int n_slots, size_t slot_bytes, size_t staging_bytes, int keep_slots, size_t entry_bytes, size_t landing_bytes,
                            size_t lend_offset, size_t lend_bytes, lia_cache_geometry* out);
/* The same with a fourth region behind the workspace entries: the whole of an allocation of extra_bytes (lia_stream_cache_extra),
 * offsets from its start.  extra_bytes == 0: lia_cache_geometry_plan, field for field. */
int lia_cache_geometry_plan_extra(int n_slots, size_t slot_bytes, size_t staging_bytes, int keep_slots, size_t entry_bytes,
                                  size_t landing_bytes, size_t lend_offset, size_t lend_bytes, size_t extra_bytes, lia_cache_geometry* out);
/* Opt-in geometry of the decode mode, refused while the mode is on and sticky until changed; all zero = the geometry above
 * without it, bit for bit.
 *   landing_bytes: the largest encoded layer that will be landed.  Landing buffers shrink from a whole staging area to this (+ read
 *       slack) and the rest of the staging allocation holds entries; lia_stream_land refuses a larger layer.
 *   lend_workspace != 0: while the mode is on, the context's workspace beyond its first workspace_keep_bytes (rounded up to 256)
 *       holds entries as well.  The context then offers only the kept part: lia_ctx_workspace_bytes returns it, every call that
 *       takes workspace (layer forwards, lm_head, score / verify / sample chunk loops, lia_gemm) sizes itself by it, and a call that
 *       needs more returns LIA_ERR_MEMORY without touching an entry.  Bytes [0, keep) are not written by the mode.
 * lia_stream_cache_enable lends and lia_stream_cache_disable takes back, by events alone: the pool's first copy runs behind
 * whatever the context's compute stream had queued and behind the K/V deliveries still draining from the workspace's slabs; the
 * compute stream's next launch runs behind the mode's last decode.  Calls that use the workspace must be on the context's compute
 * stream while a streamer of that context has this set.  lia_stream_cache_layout: the geometry lia_stream_cache_enable(s, keep_slots,
 * entry_bytes) would use now (its n_entries is lia_stream_cache_capacity); with the mode on, the one in use. */
int lia_stream_cache_configure(lia_streamer* s, size_t landing_bytes, int lend_workspace, size_t workspace_keep_bytes);
/* One more region of the decode mode, owned by the streamer: a device allocation of `bytes` -- what a model saves by holding its
 * HBM-resident layers in their wire format -- that holds entries behind the workspace's.  Allocated, resized (another size) or freed
 * (0) by this call alone, never by a mode change; refused while the mode is on; freed with the streamer. */
int lia_stream_cache_extra(lia_streamer* s, size_t bytes);
/* Decode a wire-format layer that already lies in device memory into `slot`, on the decode stream behind the slot's last release;
 * no copy.  The slot is then waited for and released like any other and the launch counts in lia_stream_decode_stats.  With the
 * decode mode on, slot < keep_slots; with it off, any slot of the ring (its next writer is ordered as by lia_stream_begin).
 * src_device must stay readable for packed_bytes + LIA_CACHE_READ_SLACK until the decode has run.  Refused: an unknown format,
 * n_values % 1024, n_values * 2 > slot_bytes. */
int lia_stream_decode_device(lia_streamer* s, int slot, const void* src_device, size_t packed_bytes, size_t n_values, int format);
int lia_stream_cache_layout(lia_streamer* s, int keep_slots, size_t entry_bytes, lia_cache_geometry* out);
/* the workspace a call on this context may use now: what lia_ctx_create allocated, or the kept part while the rest is lent */
size_t lia_ctx_workspace_bytes(lia_ctx* ctx);
/* the workspace itself (device memory, NULL for a context created without one): for tests and tools that inspect it */
void* lia_ctx_workspace_ptr(lia_ctx* ctx);

/* ---- host memory tiers ------------------------------------------------------------------------------
 * The four exports of the reference's libnuma shim, lia/cxl/numa_alloc.c:7,25,66,108 (same names, same
 * NULL-on-failure + stderr behaviour), with the interleave node set configurable instead of hard-coded
 * {2,3} (numa_alloc.c:80-81): lia_numa_set_interleave_nodes or env LIA_CXL_NODES="2,3". */
void* numa_alloc_node(size_t size, int node);
void* numa_alloc_interleave(size_t size);
void numa_free_node(void* memory, size_t size);
void check_memory_node(void* memory, int num);
int lia_numa_set_interleave_nodes(const int* nodes, int n);
int lia_numa_available(void);
/* make a host range DMA-able by the copy engine (hipHostRegister); the reference leaves CXL tensors
 * pageable (numa_alloc.py:49) so its copies degrade to staged synchronous ones */
int lia_numa_register(void* ptr, size_t size);
/* the same for a read-only mapping (PROT_READ, MAP_SHARED mmap of a checkpoint file): pinned without write intent, so the
 * page-cache pages are used in place */
int lia_numa_register_readonly(void* ptr, size_t size);
int lia_numa_unregister(void* ptr);
/* pinned host memory (Tensor.pin_memory(), modeling_opt.py:207-227) */
void* lia_host_alloc_pinned(size_t size);
void lia_host_free_pinned(void* p);

/* blocking copies between a host range and device memory (model placement, lia/modeling_opt.py:229-268) */
int lia_memcpy_h2d(void* dst_device, const void* src_host, size_t bytes);
int lia_memcpy_d2h(void* dst_host, const void* src_device, size_t bytes);

/* TPP-blocked [N/16,K/64,32,16,2] <-> row-major [N,K] on the host (_weight_prepack.py:19-63;
 * attentions.py:381-382) */
int lia_tpp_unblock(const lia_bf16* blocked, lia_bf16* plain, int N, int K);
int lia_tpp_block(const lia_bf16* plain, lia_bf16* blocked, int N, int K);

#ifdef __cplusplus
}
#endif
#endif /* LIA_HIP_H */
