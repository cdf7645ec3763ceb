// C ABI of liblia_hip.so (include/lia_hip.h), part 2: the sub-layer ops -- layernorm, linear, q | k | v projection, attention, embedding,
// lm_head, sampling, scoring.  No kernels here: see lia_internal.h for the launchers.
#include <algorithm>
#include <cmath>

#include "lia_internal.h"

// ------------------------------------------------------------------------------------------------
// sub-layer ops
// ------------------------------------------------------------------------------------------------
LiaOutMap plain_out(bf16_t* y, long ldy, int N) {
  LiaOutMap om;
  memset(&om, 0, sizeof(om));
  om.base[0] = y;
  om.ld[0] = ldy;
  om.seg_n = N;
  om.T = 1;
  return om;
}

extern "C" int lia_layernorm(const lia_bf16* x, long ldx, const lia_bf16* g, const lia_bf16* b, lia_bf16* y, long ldy,
                             long rows, int H, float eps, void* stream) {
  if (!x || !g || !b || !y) { lia_set_error("lia_layernorm: NULL tensor"); return LIA_ERR_MISSING; }
  if (rows < 0 || H <= 0 || H % 8) { lia_set_error("lia_layernorm: rows=%ld H=%d (H %% 8)", rows, H); return LIA_ERR_INVALID; }
  lia_layernorm_launch(x, ldx, g, b, y, ldy, rows, H, eps, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

int gemm_checked(lia_ctx* ctx, const bf16_t* x, long ldx, const bf16_t* w, int M, int N, int K, const LiaEpilogue& ep, const LiaOutMap& om,
                 float* ws, size_t ws_bytes, int split, hipStream_t st, const LiaPost* post, int* post_done) {
  if (N % 16 || K % 64) {
    lia_set_error("linear: N=%d must be a multiple of 16 and K=%d of 64", N, K);
    return LIA_ERR_INVALID;
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int regime = 0;
  const bool timed = ctx && ctx->prof_on && ctx->prof_recs->size() < ctx->prof_cap && (ctx->prof_seen++ % ctx->prof_stride) == 0;
  if (timed) {
    size_t i = ctx->prof_recs->size();
    e0 = (*ctx->prof_events)[2 * i];
    e1 = (*ctx->prof_events)[2 * i + 1];
  }
  int rc = lia_gemm_launch(x, ldx, w, (long)K, M, N, K, &ep, &om, ws, ws_bytes, ctx ? &ctx->gemm_opts : nullptr, split, st, e0, e1, &regime, post, post_done);
  if (timed && rc == 0 && regime != 0) {
    // algorithmic traffic of the op: the weight once, the activations in and out once
    double bytes = 2.0 * ((double)N * K + (double)M * K + (double)M * N);
    ctx->prof_recs->push_back({regime, bytes, 2.0 * M * (double)N * K});
  }
  if (rc) {
    lia_set_error("linear: unsupported shape or layout M=%d N=%d K=%d ldx=%ld ldy=%ld ldr=%ld (lia_hip.h, lia_linear: 16-byte x / w rows, "
                  "whole 8-byte stores, 16-byte ones unless M <= 256 and K %% 128 == 0)", M, N, K, ldx, om.ld[0], ep.residual ? ep.ldr : 0L);
    return LIA_ERR_INVALID;
  }
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

extern "C" int lia_linear(lia_ctx* ctx, const lia_bf16* x, long ldx, const lia_bf16* w, const lia_bf16* bias,
                          const lia_bf16* residual, long ldr, lia_bf16* y, long ldy, int M, int N, int K, int relu,
                          int split_k, void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  if (!x || !w || !y) { lia_set_error("lia_linear: NULL tensor"); return LIA_ERR_MISSING; }
  if (M < 0 || N <= 0 || K <= 0) { lia_set_error("lia_linear: M=%d N=%d K=%d", M, N, K); return LIA_ERR_INVALID; }
  LiaEpilogue ep{bias, residual, ldr, relu};
  LiaOutMap om = plain_out(y, ldy, N);
  size_t need = lia_gemm_workspace_bytes(M, N);          // split-K slabs: 8 for M <= 256, up to 4 for the tiled kernel below M = 2048
  size_t have = std::min(need, ctx->ws_bytes);
  ws_invalidate(ctx);
  return gemm_checked(ctx, x, ldx, w, M, N, K, ep, om, (float*)ctx->ws, have, split_k, (hipStream_t)stream);
}

int qkv_project(lia_ctx* ctx, const bf16_t* x, const bf16_t* w, const bf16_t* bias, bf16_t* qout, bf16_t* kdst, bf16_t* vdst,
                bool kv_cache_mode, int B, int T, int H, int cache_batch, int b0, int pos0, float* ws, size_t ws_bytes, hipStream_t st) {
  LiaEpilogue ep{bias, nullptr, 0, 0};
  LiaOutMap om;
  memset(&om, 0, sizeof(om));
  om.base[0] = qout; om.base[1] = kdst; om.base[2] = vdst;
  om.ld[0] = om.ld[1] = om.ld[2] = H;
  om.cache_mode[1] = om.cache_mode[2] = kv_cache_mode ? 1 : 0;
  om.seg_n = H; om.T = T; om.Bc = cache_batch; om.b0 = b0; om.pos0 = pos0;
  return gemm_checked(ctx, x, H, w, B * T, 3 * H, H, ep, om, ws, ws_bytes, 0, st);
}

extern "C" int lia_qkv_project(lia_ctx* ctx, const lia_bf16* x, const lia_bf16* w, const lia_bf16* bias, lia_bf16* qout,
                               lia_bf16* kcache, lia_bf16* vcache, int B, int T, int H, int cache_batch, int b0, int pos0,
                               void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  if (!x || !w || !qout || !kcache || !vcache) { lia_set_error("lia_qkv_project: NULL tensor"); return LIA_ERR_MISSING; }
  if (B <= 0 || T <= 0 || b0 < 0 || b0 + B > cache_batch || pos0 < 0) {
    lia_set_error("lia_qkv_project: B=%d T=%d cache_batch=%d b0=%d pos0=%d", B, T, cache_batch, b0, pos0);
    return LIA_ERR_INVALID;
  }
  size_t need = (size_t)B * T <= 256 ? (size_t)8 * B * T * 3 * H * 4 : 0;
  ws_invalidate(ctx);
  return qkv_project(ctx, x, w, bias, qout, kcache, vcache, true, B, T, H, cache_batch, b0, pos0, (float*)ctx->ws,
                     std::min(need, ctx->ws_bytes), (hipStream_t)stream);
}

extern "C" int lia_attention(const lia_bf16* q, long ldq, const lia_bf16* kcache, const lia_bf16* vcache, lia_bf16* out,
                             long ldo, int B, int T, int S, int heads, int head_dim, int cache_batch, int b0, void* stream) {
  if (!q || !kcache || !vcache || !out) { lia_set_error("lia_attention: NULL tensor"); return LIA_ERR_MISSING; }
  if (B <= 0 || T <= 0 || S < T || b0 < 0 || b0 + B > cache_batch) {
    lia_set_error("lia_attention: B=%d T=%d S=%d cache_batch=%d b0=%d", B, T, S, cache_batch, b0);
    return LIA_ERR_INVALID;
  }
  if (T > 1 && S != T) { lia_set_error("lia_attention: multi-token blocks only as a prefill (S == T), got S=%d T=%d", S, T); return LIA_ERR_INVALID; }
  if (lia_attn_dispatch(q, ldq, kcache, vcache, out, ldo, B, T, S - T, heads, heads, head_dim, cache_batch, b0, 0, nullptr, 0, (hipStream_t)stream)) {
    lia_set_error("lia_attention: head_dim %d unsupported (32/64/128), S=%d too long, or a cache of %d batch rows x %d values per key row beyond the d = 128 prefill kernel's 32-bit staging offsets (64 key rows < 4 GiB)",
                  head_dim, S, cache_batch, heads * head_dim);
    return LIA_ERR_INVALID;
  }
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

extern "C" int lia_embed(const int64_t* ids, const lia_bf16* tok, const lia_bf16* pos, lia_bf16* y, int B, int T,
                         int past_len, int H, void* stream) {
  if (!ids || !tok || !pos || !y) { lia_set_error("lia_embed: NULL tensor"); return LIA_ERR_MISSING; }
  if (B <= 0 || T <= 0 || past_len < 0 || H % 8) { lia_set_error("lia_embed: B=%d T=%d past=%d H=%d", B, T, past_len, H); return LIA_ERR_INVALID; }
  lia_embed_launch(ids, tok, pos, y, B, T, past_len, H, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

extern "C" int lia_embed_padded(const int64_t* ids, const lia_bf16* tok, const lia_bf16* pos, lia_bf16* y, int B, int T,
                                int past_len, int H, const int32_t* starts, void* stream) {
  if (!ids || !tok || !pos || !y || !starts) { lia_set_error("lia_embed_padded: NULL tensor"); return LIA_ERR_MISSING; }
  if (B <= 0 || T <= 0 || past_len < 0 || H % 8) { lia_set_error("lia_embed_padded: B=%d T=%d past=%d H=%d", B, T, past_len, H); return LIA_ERR_INVALID; }
  lia_embed_padded_launch(ids, tok, pos, y, B, T, past_len, H, starts, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

extern "C" int lia_embed_ragged(const int64_t* ids, const lia_bf16* tok, const lia_bf16* pos, lia_bf16* y, int B, int T, int H,
                                const int32_t* lens, const int32_t* starts, void* stream) {
  if (!ids || !tok || !pos || !y || !lens) { lia_set_error("lia_embed_ragged: NULL tensor"); return LIA_ERR_MISSING; }
  if (B <= 0 || T <= 0 || H % 8) { lia_set_error("lia_embed_ragged: B=%d T=%d H=%d", B, T, H); return LIA_ERR_INVALID; }
  lia_embed_ragged_launch(ids, tok, pos, y, B, T, H, lens, starts, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

extern "C" int lia_llama_embed(const int64_t* ids, const lia_bf16* tok, lia_bf16* y, int B, int T, int H, void* stream) {
  if (!ids || !tok || !y) return LIA_ERR_MISSING;
  if (B <= 0 || T <= 0 || H % 8) return LIA_ERR_INVALID;
  lia_embed_tokens_launch(ids, tok, y, (long)B * T, H, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

extern "C" int lia_attention_padded(const lia_bf16* q, long ldq, const lia_bf16* kcache, const lia_bf16* vcache, lia_bf16* out,
                                    long ldo, int B, int T, int S, int heads, int head_dim, int cache_batch, int b0,
                                    const int32_t* starts, void* stream) {
  if (!q || !kcache || !vcache || !out || !starts) { lia_set_error("lia_attention_padded: NULL tensor"); return LIA_ERR_MISSING; }
  if (B <= 0 || T <= 0 || S < T || b0 < 0 || b0 + B > cache_batch || (T > 1 && S != T)) {
    lia_set_error("lia_attention_padded: B=%d T=%d S=%d cache_batch=%d b0=%d (multi-token blocks only as a prefill, S == T)", B, T, S,
                  cache_batch, b0);
    return LIA_ERR_INVALID;
  }
  if (lia_attn_dispatch(q, ldq, kcache, vcache, out, ldo, B, T, S - T, heads, heads, head_dim, cache_batch, b0, 0, starts, 0, (hipStream_t)stream)) {
    lia_set_error("lia_attention_padded: head_dim %d unsupported (32/64/128), S=%d too long, or a cache of %d batch rows x %d values per key row beyond the d = 128 prefill kernel's 32-bit staging offsets",
                  head_dim, S, cache_batch, heads * head_dim);
    return LIA_ERR_INVALID;
  }
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

// ------------------------------------------------------------------------------------------------
// head modifiers (LiaHeadMods, lia_internal.h): the one path by which a head call sees the token mask, the log-probability sink and
// the penalties of its context
// ------------------------------------------------------------------------------------------------
// What a head does with each modifier WHEN IT IS SET: NULL -- takes it; a reason -- refuses the call, by name, with that reason;
// LIA_MOD_UNSEEN -- never looks at it.
struct LiaHeadTakes { const char *mask, *sink, *penalties; };
#define LIA_MOD_UNSEEN ""
#define LIA_NO_BLOCK_PENALTIES "every block position would need its own counts -- penalties are not applied under speculation"

static bool head_mod_refused(const char* who, bool set, const char* why, const char* what) {
  if (!set || !why || !*why) return false;
  lia_set_error("%s: %s: %s", who, what, why);
  return true;
}

// The modifiers of a head call on `rows` rows of `vocab` logits, checked against the call: *out holds what the head takes (a NULL
// first member: not set -- the launches without it); LIA_ERR_INVALID with the fault by name otherwise.  The one place that words
// these faults and orders them: what the head does not take (sink, penalties, mask), then the head's own arguments (args_invalid:
// true = refused, the error is set), then the fit of what it takes (mask, sink, penalties).  Nothing is launched before it returns.
template <typename ArgsInvalid>
static int head_mods_resolve(const char* who, const lia_ctx* ctx, const LiaHeadTakes& no, long rows, int vocab, LiaHeadMods* out,
                             ArgsInvalid args_invalid) {
  const LiaTokenMask& mk = ctx->mods.mask;
  const LiaSink& sk = ctx->mods.sink;
  const LiaPenalties& pn = ctx->mods.penalties;
  if (head_mod_refused(who, sk.chosen, no.sink, "a log-probability sink is set (lia_ctx_set_logprob_sink)")) return LIA_ERR_INVALID;
  if (head_mod_refused(who, pn.counts, no.penalties, "penalties are set (lia_ctx_set_penalties)")) return LIA_ERR_INVALID;
  if (head_mod_refused(who, mk.table, no.mask, "a token mask is set (lia_ctx_set_token_mask)")) return LIA_ERR_INVALID;
  if (args_invalid()) return LIA_ERR_INVALID;
  *out = LiaHeadMods{};
  if (mk.table && !no.mask) {
    const long W = ((long)vocab + 31) / 32;
    if (mk.ld != 0 && mk.ld < W) {
      lia_set_error("%s: the token mask has ldm=%ld words per row, vocab=%d needs ceil(vocab / 32) = %ld (or 0: one row for every row)", who,
                    mk.ld, vocab, W);
      return LIA_ERR_INVALID;
    }
    if (mk.ld != 0 && rows > mk.rows) {
      lia_set_error("%s: the call has %ld rows, the token mask table %d (lia_ctx_set_token_mask)", who, rows, mk.rows);
      return LIA_ERR_INVALID;
    }
    out->mask = mk;
  }
  if (sk.chosen && !no.sink) {
    if (sk.n_top > vocab) {
      lia_set_error("%s: the log-probability sink asks for n_top=%d alternatives, vocab=%d has fewer (lia_ctx_set_logprob_sink)", who,
                    sk.n_top, vocab);
      return LIA_ERR_INVALID;
    }
    if (rows > sk.rows) {
      lia_set_error("%s: the call has %ld rows, the log-probability sink %ld (lia_ctx_set_logprob_sink)", who, rows, sk.rows);
      return LIA_ERR_INVALID;
    }
    out->sink = sk;
  }
  if (pn.counts && !no.penalties) {
    if (pn.ldc < vocab) { lia_set_error("%s: the count table has ldc=%ld words per row, vocab=%d (lia_ctx_set_penalties)", who, pn.ldc, vocab); return LIA_ERR_INVALID; }
    if (pn.lds < vocab) { lia_set_error("%s: the penalty scratch has lds=%ld values per row, vocab=%d (lia_ctx_set_penalties)", who, pn.lds, vocab); return LIA_ERR_INVALID; }
    if (rows > pn.rows) { lia_set_error("%s: the call has %ld rows, the count table %d (lia_ctx_set_penalties)", who, rows, pn.rows); return LIA_ERR_INVALID; }
    out->penalties = pn;
  }
  return LIA_OK;
}
// ... for a head whose own arguments were checked in front of it
static int head_mods_resolve(const char* who, const lia_ctx* ctx, const LiaHeadTakes& no, long rows, int vocab, LiaHeadMods* out) {
  return head_mods_resolve(who, ctx, no, rows, vocab, out, [] { return false; });
}
// the mask and the penalties as a call on rows r0 .. sees them: each table from its row r0 on (the sink: sink_write takes r0)
static LiaHeadMods head_mods_at_row(LiaHeadMods m, long r0) {
  if (m.mask.table) m.mask.table += r0 * m.mask.ld;
  if (m.penalties.counts) { m.penalties.counts += r0 * m.penalties.ldc; m.penalties.scratch += r0 * m.penalties.lds; }
  return m;
}

// rows r0 .. r0 + n - 1 of the sink from the n logits rows in hand and the ids their head just wrote (ids: that of row r0)
static void sink_write(const LiaSink& sk, const bf16_t* logits, long ld, int n, int vocab, const int64_t* ids, long r0, hipStream_t st) {
  if (!sk.chosen) return;
  lia_topn_logprobs_launch(logits, ld, n, vocab, ids, sk.n_top, sk.chosen + r0, sk.n_top ? sk.top_ids + r0 * sk.n_top : nullptr,
                           sk.n_top ? sk.top + r0 * sk.n_top : nullptr, st);
}
// scratch rows 0 .. n - 1 = the n logits rows in hand, penalised under table rows 0 .. n - 1
static void penalties_write(const LiaPenalties& pn, const bf16_t* logits, long ld, int n, int vocab, hipStream_t st) {
  lia_penalty_launch(logits, ld, n, vocab, pn.counts, pn.ldc, pn.theta, pn.presence, pn.frequency, pn.scratch, pn.lds, st);
}
// the penalty settings and a count table, worded once for the three entry points (lia_internal.h)
bool penalty_args_invalid(const char* who, float repetition, float presence, float frequency, const void* counts, long ldc, int vocab) {
  if (!std::isfinite(repetition) || !(repetition > 0.f)) { lia_set_error("%s: repetition=%g must be finite and > 0 (1: off)", who, (double)repetition); return true; }
  if (!std::isfinite(presence)) { lia_set_error("%s: presence=%g must be finite (0: off)", who, (double)presence); return true; }
  if (!std::isfinite(frequency)) { lia_set_error("%s: frequency=%g must be finite (0: off)", who, (double)frequency); return true; }
  if ((uintptr_t)counts & 3) { lia_set_error("%s: counts=%p is not 4-byte aligned (two words share a 32-bit location)", who, counts); return true; }
  if (ldc % 2 || ldc <= 0) { lia_set_error("%s: ldc=%ld must be even and > 0 (two words share a 32-bit location)", who, ldc); return true; }
  if (vocab >= 0 && ldc < vocab) { lia_set_error("%s: ldc=%ld < vocab=%d", who, ldc, vocab); return true; }
  return false;
}

// Where a row of a verify block stands: block rows r0 .. of T positions each, `suppress` counting as -inf at positions < n_suppress
// (n_suppress_rows, device int32 [B] or NULL: one bound per row in its place).  NULL in the pick helpers: plain rows, as lm_head's.
struct LiaBlockPos { int n_suppress; const int* n_suppress_rows; int T, r0; };

// The greedy id of n logits rows `ld` apart, under the call's mask.  Plain rows `vocab` apart: the head's own argmax kernel (what
// penalties.py allocates for the penalised rows; 9.0 against 12.4 us at B 64 x 50272); plain rows at another pitch (a pitched penalty
// scratch): the verify heads' argmax launch, which takes a pitch -- the same scan and tie rule; T = 1, n_suppress = 1: `suppress`
// holds for every row, and block row i reads mask row i.  A verify block: that launch.
static void pick_argmax(const LiaTokenMask& mk, const bf16_t* logits, long ld, int n, int vocab, int suppress, const LiaBlockPos* blk,
                        int64_t* ids, hipStream_t st) {
  static const LiaBlockPos every_row{1, nullptr, 1, 0};
  if (!blk && ld == vocab) {
    if (mk.table) lia_argmax_masked_launch(logits, ids, n, vocab, suppress, mk.table, mk.ld, st);
    else lia_argmax_launch(logits, ids, n, vocab, suppress, st);
    return;
  }
  if (!blk) blk = &every_row;
  if (mk.table) lia_verify_argmax_masked_launch(logits, ld, n, vocab, suppress, blk->n_suppress, blk->n_suppress_rows, blk->T, blk->r0, ids, mk.table, mk.ld, st);
  else lia_verify_argmax_rows_launch(logits, ld, n, vocab, suppress, blk->n_suppress, blk->n_suppress_rows, blk->T, blk->r0, ids, st);
}

// norm_b == nullptr: RMSNorm (Llama), else LayerNorm.  Any B >= 1: the rows go through in chunks of LIA_HEAD_CHUNK -- rows are
// independent, so the results are those of one call -- and chunk b0 uses row b0 .. of the logits, the ids and every modifier.
#define LIA_HEAD_CHUNK 256    // the skinny GEMM regime's M (split-K slabs in the workspace)
static int lm_head_impl(const char* who, lia_ctx* ctx, const bf16_t* hidden, int B, int T, int H, const bf16_t* norm_w, const bf16_t* norm_b,
                        const bf16_t* emb, int vocab, float eps, int suppress_token, bf16_t* logits, int64_t* next_ids, hipStream_t st) {
  LiaHeadMods all;
  if (int rc = head_mods_resolve(who, ctx, LiaHeadTakes{}, B, vocab, &all)) return rc;
  if (ctx->ws_bytes < align_up((size_t)std::min(B, LIA_HEAD_CHUNK) * H * 2, 256)) { lia_set_error("%s: workspace too small", who); return LIA_ERR_MEMORY; }
  ws_invalidate(ctx);
  bf16_t* lno = (bf16_t*)ctx->ws;
  const LiaEpilogue ep{nullptr, nullptr, 0, 0};
  for (int b0 = 0; b0 < B; b0 += LIA_HEAD_CHUNK) {
    const int n = std::min(LIA_HEAD_CHUNK, B - b0);
    const size_t scratch = align_up((size_t)n * H * 2, 256);
    const size_t gemm_need = (size_t)8 * n * vocab * 4;
    const LiaHeadMods m = head_mods_at_row(all, b0);
    const bf16_t* x = hidden + (long)b0 * T * H;
    bf16_t* lg = logits + (long)b0 * vocab;
    // hidden[:, -1, :] -> final LN (lia/modeling_opt.py:1563 applies it to all positions; only the last one feeds
    // lm_head, models.py:424-431, and LN is row-wise, so the other rows are never needed)
    if (norm_b) lia_layernorm_launch(x + (long)(T - 1) * H, (long)T * H, norm_w, norm_b, lno, H, n, H, eps, st);
    else lia_rmsnorm_launch(x + (long)(T - 1) * H, (long)T * H, norm_w, lno, H, n, H, eps, st);
    const LiaOutMap om = plain_out(lg, vocab, vocab);
    if (int rc = gemm_checked(ctx, lno, H, emb, n, vocab, H, ep, om, (float*)(ctx->ws + scratch), std::min(ctx->ws_bytes - scratch, gemm_need), 0, st)) return rc;
    if (m.penalties.counts) {
      penalties_write(m.penalties, lg, vocab, n, vocab, st);
      pick_argmax(m.mask, m.penalties.scratch, m.penalties.lds, n, vocab, suppress_token, nullptr, next_ids + b0, st);
    } else {
      pick_argmax(m.mask, lg, vocab, n, vocab, suppress_token, nullptr, next_ids + b0, st);
    }
    sink_write(m.sink, lg, vocab, n, vocab, next_ids + b0, b0, st);
    HIP_TRY(hipGetLastError());
  }
  return LIA_OK;
}

extern "C" int lia_lm_head(lia_ctx* ctx, const lia_bf16* hidden, int B, int T, int H, const lia_bf16* lnw,
                           const lia_bf16* lnb, const lia_bf16* emb, int vocab, float eps, int suppress_token,
                           lia_bf16* logits, int64_t* next_ids, void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  if (!hidden || !lnw || !lnb || !emb || !logits || !next_ids) { lia_set_error("lia_lm_head: NULL tensor"); return LIA_ERR_MISSING; }
  if (B <= 0 || T <= 0 || vocab % 16) { lia_set_error("lia_lm_head: B=%d T=%d vocab=%d (%%16)", B, T, vocab); return LIA_ERR_INVALID; }
  return lm_head_impl("lia_lm_head", ctx, hidden, B, T, H, lnw, lnb, emb, vocab, eps, suppress_token, logits, next_ids, (hipStream_t)stream);
}

extern "C" int lia_llama_lm_head(lia_ctx* ctx, const lia_bf16* hidden, int B, int T, int H, const lia_bf16* normw, const lia_bf16* lm,
                                 int vocab, float eps, int suppress_token, lia_bf16* logits, int64_t* next_ids, void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  if (!hidden || !normw || !lm || !logits || !next_ids) { lia_set_error("lia_llama_lm_head: NULL tensor"); return LIA_ERR_MISSING; }
  if (B <= 0 || T <= 0 || vocab % 16) { lia_set_error("lia_llama_lm_head: B=%d T=%d vocab=%d", B, T, vocab); return LIA_ERR_INVALID; }
  return lm_head_impl("lia_llama_lm_head", ctx, hidden, B, T, H, normw, nullptr, lm, vocab, eps, suppress_token, logits, next_ids, (hipStream_t)stream);
}

// temperature -> top-k -> top-p -> one draw per row (lia_sample.hip).  Any B; the row is read a fixed number of times.
#define LIA_SAMPLE_MAX_VOCAB (256 * 8192)   // lia_sample.hip keeps one running sum per 8192-token tile in LDS
// the settings' refusals, worded once for lia_sample and the sampled verify heads
static bool sample_settings_invalid(const char* who, float temperature, int top_k, float top_p) {
  if (!(temperature > 0.f) || !std::isfinite(temperature)) { lia_set_error("%s: temperature=%g must be finite and > 0", who, (double)temperature); return true; }
  if (top_k < 0) { lia_set_error("%s: top_k=%d must be >= 0 (0: off)", who, top_k); return true; }
  if (!(top_p > 0.f && top_p <= 1.f)) { lia_set_error("%s: top_p=%g must be in (0, 1] (1: off)", who, (double)top_p); return true; }
  return false;
}

// A draw's settings and, for a verify block, where its uniforms come from: position t of block row b draws with
// uniforms[(step0 + t) * ldu + b] of an n_steps-row table (step_rows, device int32 [B] or NULL: a step origin per row)
struct LiaDraw { float tau; int top_k; float top_p; const float* uniforms; };
struct LiaBlockDraw { LiaBlockPos pos; long ldu; int n_steps, step0; const int* step_rows; const int64_t* block_ids; };

// The drawn id of n logits rows `ld` apart, under the call's mask.  Plain rows (blk == NULL): lia_sample's kernel, aux = stats or
// NULL; a verify block: the block draw, aux = p_draft or NULL.
static void pick_draw(const LiaTokenMask& mk, const bf16_t* logits, long ld, int n, int vocab, const LiaDraw& d, int suppress,
                      const LiaBlockDraw* blk, int64_t* ids, float* aux, hipStream_t st) {
  if (!blk) {
    if (mk.table) lia_sample_masked_launch(logits, ld, n, vocab, d.tau, d.top_k, d.top_p, suppress, d.uniforms, ids, aux, mk.table, mk.ld, st);
    else lia_sample_launch(logits, ld, n, vocab, d.tau, d.top_k, d.top_p, suppress, d.uniforms, ids, aux, st);
    return;
  }
  const LiaBlockPos& p = blk->pos;
  if (mk.table)
    lia_verify_sample_masked_launch(logits, ld, n, vocab, d.tau, d.top_k, d.top_p, suppress, p.n_suppress, p.n_suppress_rows, p.T, p.r0, d.uniforms,
                                    blk->ldu, blk->n_steps, blk->step0, blk->step_rows, blk->block_ids, ids, aux, mk.table, mk.ld, st);
  else
    lia_verify_sample_launch(logits, ld, n, vocab, d.tau, d.top_k, d.top_p, suppress, p.n_suppress, p.n_suppress_rows, p.T, p.r0, d.uniforms,
                             blk->ldu, blk->n_steps, blk->step0, blk->step_rows, blk->block_ids, ids, aux, st);
}

extern "C" int lia_sample(lia_ctx* ctx, const lia_bf16* logits, long ld, int B, int vocab, float temperature, int top_k, float top_p,
                          int suppress_token, const float* uniforms, int64_t* next_ids, float* stats, void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  if (!logits || !uniforms || !next_ids) {
    lia_set_error("lia_sample: NULL %s", !logits ? "logits" : !uniforms ? "uniforms" : "next_ids");
    return LIA_ERR_INVALID;
  }
  if (B <= 0) { lia_set_error("lia_sample: B=%d must be >= 1", B); return LIA_ERR_INVALID; }
  if (vocab <= 0 || vocab > LIA_SAMPLE_MAX_VOCAB) { lia_set_error("lia_sample: vocab=%d must be in [1, %d]", vocab, LIA_SAMPLE_MAX_VOCAB); return LIA_ERR_INVALID; }
  if (ld < vocab) { lia_set_error("lia_sample: ld=%ld < vocab=%d", ld, vocab); return LIA_ERR_INVALID; }
  if (sample_settings_invalid("lia_sample", temperature, top_k, top_p)) return LIA_ERR_INVALID;
  if (suppress_token < -1 || suppress_token >= vocab) { lia_set_error("lia_sample: suppress_token=%d must be -1 or in [0, vocab)", suppress_token); return LIA_ERR_INVALID; }
  LiaHeadMods m;
  if (int rc = head_mods_resolve("lia_sample", ctx, LiaHeadTakes{}, B, vocab, &m)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const LiaDraw draw{temperature, top_k, top_p, uniforms};
  if (m.penalties.counts) {
    penalties_write(m.penalties, logits, ld, B, vocab, st);
    pick_draw(m.mask, m.penalties.scratch, m.penalties.lds, B, vocab, draw, suppress_token, nullptr, next_ids, stats, st);
  } else {
    pick_draw(m.mask, logits, ld, B, vocab, draw, suppress_token, nullptr, next_ids, stats, st);
  }
  sink_write(m.sink, logits, ld, B, vocab, next_ids, 0, st);      // (the sink reads the model's own distribution)
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

// ------------------------------------------------------------------------------------------------
// penalties: the bare kernels (lia_penalty.hip); lia_ctx_set_penalties is in lia_ctx.hip
// ------------------------------------------------------------------------------------------------
extern "C" int lia_token_counts_add(lia_ctx* ctx, uint16_t* counts, long ldc, int rows, int vocab, const int64_t* ids, long ldi, int n,
                                    const int32_t* first, const int32_t* active, int generated, void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  if (!counts || !ids) { lia_set_error("lia_token_counts_add: NULL %s", !counts ? "counts" : "ids"); return LIA_ERR_INVALID; }
  if (rows <= 0) { lia_set_error("lia_token_counts_add: rows=%d must be >= 1", rows); return LIA_ERR_INVALID; }
  if (vocab <= 0) { lia_set_error("lia_token_counts_add: vocab=%d must be >= 1", vocab); return LIA_ERR_INVALID; }
  if (n < 0 || ldi < n) { lia_set_error("lia_token_counts_add: n=%d must be >= 0 and ldi=%ld >= n", n, ldi); return LIA_ERR_INVALID; }
  if (generated != 0 && generated != 1) { lia_set_error("lia_token_counts_add: generated=%d must be 0 (prompt) or 1 (generated)", generated); return LIA_ERR_INVALID; }
  if (penalty_args_invalid("lia_token_counts_add", 1.f, 0.f, 0.f, counts, ldc, vocab)) return LIA_ERR_INVALID;
  lia_token_counts_launch(counts, ldc, rows, vocab, ids, ldi, n, first, active, generated, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

extern "C" int lia_apply_penalties(lia_ctx* ctx, const lia_bf16* logits, long ld, int M, int vocab, const uint16_t* counts, long ldc,
                                   float repetition, float presence, float frequency, lia_bf16* out, long ldo, void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  if (!logits || !counts || !out) { lia_set_error("lia_apply_penalties: NULL %s", !logits ? "logits" : !counts ? "counts" : "out"); return LIA_ERR_INVALID; }
  if (M <= 0) { lia_set_error("lia_apply_penalties: M=%d must be >= 1", M); return LIA_ERR_INVALID; }
  if (vocab <= 0) { lia_set_error("lia_apply_penalties: vocab=%d must be >= 1", vocab); return LIA_ERR_INVALID; }
  if (ld < vocab) { lia_set_error("lia_apply_penalties: ld=%ld < vocab=%d", ld, vocab); return LIA_ERR_INVALID; }
  if (ldo < vocab) { lia_set_error("lia_apply_penalties: ldo=%ld < vocab=%d", ldo, vocab); return LIA_ERR_INVALID; }
  if (penalty_args_invalid("lia_apply_penalties", repetition, presence, frequency, counts, ldc, vocab)) return LIA_ERR_INVALID;
  lia_penalty_launch(logits, ld, M, vocab, counts, ldc, repetition, presence, frequency, out, ldo, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

// ------------------------------------------------------------------------------------------------
// scoring: log p(target) and the greedy token of every row (lia_score.hip; the chunk rule is stated in lia_hip.h)
// ------------------------------------------------------------------------------------------------
extern "C" int lia_token_logprobs(lia_ctx* ctx, const lia_bf16* logits, long ld, int M, int vocab, const int64_t* targets,
                                  float* logprobs, int64_t* greedy_ids, void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  if (!logits || !targets || !logprobs || !greedy_ids) {
    lia_set_error("lia_token_logprobs: NULL %s", !logits ? "logits" : !targets ? "targets" : !logprobs ? "logprobs" : "greedy_ids");
    return LIA_ERR_INVALID;
  }
  if (M <= 0) { lia_set_error("lia_token_logprobs: M=%d must be >= 1", M); return LIA_ERR_INVALID; }
  if (vocab <= 0) { lia_set_error("lia_token_logprobs: vocab=%d must be >= 1", vocab); return LIA_ERR_INVALID; }
  if (ld < vocab) { lia_set_error("lia_token_logprobs: ld=%ld < vocab=%d", ld, vocab); return LIA_ERR_INVALID; }
  lia_token_logprobs_launch(logits, ld, M, vocab, targets, logprobs, greedy_ids, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

extern "C" int lia_topn_logprobs(lia_ctx* ctx, const lia_bf16* logits, long ld, int M, int vocab, const int64_t* ids, int n_top,
                                 float* chosen, int64_t* top_ids, float* top_logprobs, void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  if (!logits || !ids || !chosen) {
    lia_set_error("lia_topn_logprobs: NULL %s", !logits ? "logits" : !ids ? "ids" : "chosen");
    return LIA_ERR_INVALID;
  }
  if (M <= 0) { lia_set_error("lia_topn_logprobs: M=%d must be >= 1", M); return LIA_ERR_INVALID; }
  if (vocab <= 0) { lia_set_error("lia_topn_logprobs: vocab=%d must be >= 1", vocab); return LIA_ERR_INVALID; }
  if (ld < vocab) { lia_set_error("lia_topn_logprobs: ld=%ld < vocab=%d", ld, vocab); return LIA_ERR_INVALID; }
  if (n_top < 0 || n_top > LIA_LOGPROB_MAX_TOP) { lia_set_error("lia_topn_logprobs: n_top=%d must be in [0, %d]", n_top, LIA_LOGPROB_MAX_TOP); return LIA_ERR_INVALID; }
  if (n_top > vocab) { lia_set_error("lia_topn_logprobs: n_top=%d alternatives, vocab=%d has fewer", n_top, vocab); return LIA_ERR_INVALID; }
  if (n_top > 0 && (!top_ids || !top_logprobs)) {
    lia_set_error("lia_topn_logprobs: NULL %s with n_top=%d (NULL only with n_top = 0)", !top_ids ? "top_ids" : "top_logprobs", n_top);
    return LIA_ERR_INVALID;
  }
  lia_topn_logprobs_launch(logits, ld, M, vocab, ids, n_top, chosen, top_ids, top_logprobs, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

extern "C" int lia_lm_score_chunk_rows(size_t workspace_bytes, int M, int H, int vocab) {
  if (M <= 0 || H <= 0 || vocab <= 0 || workspace_bytes < 512) return 0;
  const size_t per_row = 2 * (size_t)H + 2 * (size_t)vocab;
  size_t c = std::min({(size_t)M, (size_t)LIA_SCORE_MAX_CHUNK, (workspace_bytes - 512) / per_row});
  if (c < (size_t)M) c = c / 256 * 256;
  return c < (size_t)std::min(M, 256) ? 0 : (int)c;
}

extern "C" size_t lia_lm_score_workspace_bytes(int M, int H, int vocab) {
  if (M <= 0 || H <= 0 || vocab <= 0) return 0;
  return 512 + (size_t)std::min(M, LIA_SCORE_MAX_CHUNK) * (2 * (size_t)H + 2 * (size_t)vocab);
}

// Final norm + lm_head GEMM over EVERY row of hidden [M, ldh], one workspace chunk at a time (the CHUNK RULE of lia_hip.h): per
// chunk, per_chunk(logits [n, vocab], r0, n) consumes the bf16 logits of rows r0 .. r0 + n - 1 before the next chunk overwrites them.
// The one place that carves the workspace and words the refusals: lia_lm_score and lia_lm_verify cannot drift apart.
// norm_b == nullptr: RMSNorm (Llama), else LayerNorm
template <typename PerChunk>
static int lm_rows_chunked(const char* who, lia_ctx* ctx, const bf16_t* hidden, long ldh, int M, int H, const bf16_t* norm_w,
                           const bf16_t* norm_b, const bf16_t* emb, int vocab, float eps, hipStream_t st, PerChunk per_chunk) {
  if (M <= 0) { lia_set_error("%s: M=%d must be >= 1", who, M); return LIA_ERR_INVALID; }
  if (H <= 0 || H % 64 || vocab <= 0 || vocab % 16) { lia_set_error("%s: H=%d (%%64) vocab=%d (%%16)", who, H, vocab); return LIA_ERR_INVALID; }
  if (ldh < H || ldh % 8) { lia_set_error("%s: ldh=%ld must be >= H=%d and a multiple of 8", who, ldh, H); return LIA_ERR_INVALID; }
  const int c = lia_lm_score_chunk_rows(ctx->ws_bytes, M, H, vocab);
  if (c <= 0) {
    lia_set_error("%s: a workspace of %zu bytes holds no chunk of %d rows (normed rows [c, %d] + logits [c, %d] in bf16 need %zu)", who,
                  ctx->ws_bytes, std::min(M, 256), H, vocab, (size_t)512 + (size_t)std::min(M, 256) * (2 * (size_t)H + 2 * (size_t)vocab));
    return LIA_ERR_MEMORY;
  }
  ws_invalidate(ctx);
  bf16_t* lno = (bf16_t*)ctx->ws;
  bf16_t* logits = (bf16_t*)(ctx->ws + align_up((size_t)c * H * 2, 256));
  const LiaEpilogue ep{nullptr, nullptr, 0, 0};
  for (int r0 = 0; r0 < M; r0 += c) {
    const int n = std::min(c, M - r0);
    const bf16_t* x = hidden + (long)r0 * ldh;
    if (norm_b) lia_layernorm_launch(x, ldh, norm_w, norm_b, lno, H, n, H, eps, st);
    else lia_rmsnorm_launch(x, ldh, norm_w, lno, H, n, H, eps, st);
    const LiaOutMap om = plain_out(logits, vocab, vocab);
    const int rc = gemm_checked(ctx, lno, H, emb, n, vocab, H, ep, om, nullptr, 0, 0, st);    // no slabs: never split over K
    if (rc) return rc;
    per_chunk(logits, r0, n);
  }
  return LIA_OK;
}

static int lm_score_impl(const char* who, lia_ctx* ctx, const bf16_t* hidden, long ldh, int M, int H, const bf16_t* norm_w,
                         const bf16_t* norm_b, const bf16_t* emb, int vocab, float eps, const int64_t* targets, float* logprobs,
                         int64_t* greedy_ids, hipStream_t st) {
  LiaHeadMods none;
  if (int mrc = head_mods_resolve(who, ctx, LiaHeadTakes{LIA_MOD_UNSEEN, "the score heads report log-probabilities themselves and write no sink",
                                                         "the score heads report the model's own distribution and emit no token"}, M, vocab, &none))
    return mrc;
  const int rc = lm_rows_chunked(who, ctx, hidden, ldh, M, H, norm_w, norm_b, emb, vocab, eps, st, [&](const bf16_t* logits, int r0, int n) {
    lia_token_logprobs_launch(logits, vocab, n, vocab, targets + r0, logprobs + r0, greedy_ids + r0, st);
  });
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

extern "C" int lia_lm_score(lia_ctx* ctx, const lia_bf16* hidden, long ldh, int M, int H, const lia_bf16* lnw, const lia_bf16* lnb,
                            const lia_bf16* emb, int vocab, float eps, const int64_t* targets, float* logprobs, int64_t* greedy_ids,
                            void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  if (!hidden || !lnw || !lnb || !emb || !targets || !logprobs || !greedy_ids) { lia_set_error("lia_lm_score: NULL tensor"); return LIA_ERR_MISSING; }
  return lm_score_impl("lia_lm_score", ctx, hidden, ldh, M, H, lnw, lnb, emb, vocab, eps, targets, logprobs, greedy_ids, (hipStream_t)stream);
}

extern "C" int lia_llama_lm_score(lia_ctx* ctx, const lia_bf16* hidden, long ldh, int M, int H, const lia_bf16* normw,
                                  const lia_bf16* lm, int vocab, float eps, const int64_t* targets, float* logprobs,
                                  int64_t* greedy_ids, void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  if (!hidden || !normw || !lm || !targets || !logprobs || !greedy_ids) { lia_set_error("lia_llama_lm_score: NULL tensor"); return LIA_ERR_MISSING; }
  return lm_score_impl("lia_llama_lm_score", ctx, hidden, ldh, M, H, normw, nullptr, lm, vocab, eps, targets, logprobs, greedy_ids,
                       (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// speculative verification: lm_score's chunks (lm_rows_chunked) with a per-row id kernel behind them, then an acceptance kernel
// (lia_score.hip).  Three heads: the greedy one (argmax), the sampled one (lia_sample's draw behind every block position,
// lia_verify_sample_kernel) and the rejection one (the accept test and the residual draw of a stochastic drafter's block,
// lia_verify_reject_kernel, lia_sample.hip)
// ------------------------------------------------------------------------------------------------
// the block's shape and suppression, worded once for the three heads
static bool block_args_invalid(const char* who, int B, int T, int n_suppress, int suppress_token, int vocab) {
  if (B <= 0) { lia_set_error("%s: B=%d must be >= 1", who, B); return true; }
  if (T < 2) { lia_set_error("%s: T=%d must be >= 2 (the pending token and at least one draft token)", who, T); return true; }
  if ((long)B * T > 0x7fffffffL) { lia_set_error("%s: B=%d x T=%d rows", who, B, T); return true; }
  if (n_suppress < 0 || n_suppress > T) { lia_set_error("%s: n_suppress=%d must be in [0, T=%d]", who, n_suppress, T); return true; }
  if (suppress_token < -1 || (vocab > 0 && suppress_token >= vocab)) { lia_set_error("%s: suppress_token=%d must be -1 or in [0, vocab)", who, suppress_token); return true; }
  return false;
}
// a block draw's settings and uniform table, worded once for the sampled and the rejection head
static bool block_draw_invalid(const char* who, int B, int vocab, float temperature, int top_k, float top_p, long ldu, int n_steps, int step0) {
  if (vocab > LIA_SAMPLE_MAX_VOCAB) { lia_set_error("%s: vocab=%d must be in [1, %d]", who, vocab, LIA_SAMPLE_MAX_VOCAB); return true; }
  if (sample_settings_invalid(who, temperature, top_k, top_p)) return true;
  if (ldu < B) { lia_set_error("%s: ldu=%ld < B=%d", who, ldu, B); return true; }
  if (n_steps < 1) { lia_set_error("%s: n_steps=%d must be >= 1", who, n_steps); return true; }
  if (step0 < 0) { lia_set_error("%s: step0=%d must be >= 0", who, step0); return true; }
  return false;
}
// a chunk's logits into rows r0 .. of logits_out [B * T, vocab] (NULL: not asked for); *err keeps the first failure
static void logits_out_copy(bf16_t* logits_out, const bf16_t* logits, int r0, int n, int vocab, hipStream_t st, hipError_t* err) {
  if (logits_out && *err == hipSuccess)
    *err = hipMemcpyAsync(logits_out + (size_t)r0 * vocab, logits, (size_t)n * vocab * sizeof(bf16_t), hipMemcpyDeviceToDevice, st);
}

// the arguments every verify head needs (names: their names, in the order they are passed), refused by name
#define LIA_VERIFY_NULL(who, names, ...)                                                      \
  do {                                                                                        \
    const void* const ptrs[] = {__VA_ARGS__};                                                 \
    for (size_t i = 0; i < sizeof(ptrs) / sizeof(*ptrs); ++i)                                 \
      if (!ptrs[i]) { lia_set_error("%s: NULL %s", who, names[i]); return LIA_ERR_INVALID; }  \
  } while (0)
static const char* const GREEDY_ARGS[] = {"hidden", "norm weight", "lm_head weight", "block_ids", "greedy", "accepted", "common", "next"};
static const char* const SAMPLED_ARGS[] = {"hidden", "norm weight", "lm_head weight", "block_ids", "sampled", "accepted", "common", "next"};
static const char* const REJECT_ARGS[] = {"hidden", "norm weight", "lm_head weight", "block_ids", "token", "ok", "accepted", "common", "next"};

// norm_b == nullptr: RMSNorm (Llama), else LayerNorm
static int lm_verify_impl(const char* who, lia_ctx* ctx, const bf16_t* hidden, long ldh, int B, int T, int H, const bf16_t* norm_w,
                          const bf16_t* norm_b, const bf16_t* emb, int vocab, float eps, int suppress_token, int n_suppress,
                          const int64_t* block_ids, const int32_t* active, int64_t* greedy, int32_t* accepted, int32_t* common,
                          int64_t* next, hipStream_t st, const int32_t* n_suppress_rows = nullptr) {
  LiaHeadMods m;
  if (int mrc = head_mods_resolve(who, ctx, LiaHeadTakes{nullptr, nullptr, LIA_NO_BLOCK_PENALTIES}, (long)B * T, vocab, &m,
                                  [&] { return block_args_invalid(who, B, T, n_suppress, suppress_token, vocab); }))
    return mrc;
  const int rc = lm_rows_chunked(who, ctx, hidden, ldh, B * T, H, norm_w, norm_b, emb, vocab, eps, st, [&](const bf16_t* logits, int r0, int n) {
    const LiaBlockPos pos{n_suppress, n_suppress_rows, T, r0};
    pick_argmax(m.mask, logits, vocab, n, vocab, suppress_token, &pos, greedy, st);
    sink_write(m.sink, logits, vocab, n, vocab, greedy + r0, r0, st);
  });
  if (rc) return rc;
  lia_verify_accept_launch(block_ids, greedy, active, B, T, accepted, common, next, st);
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

extern "C" int lia_lm_verify(lia_ctx* ctx, const lia_bf16* hidden, long ldh, int B, int T, int H, const lia_bf16* lnw, const lia_bf16* lnb,
                             const lia_bf16* emb, int vocab, float eps, int suppress_token, int n_suppress, const int64_t* block_ids,
                             const int32_t* active, int64_t* greedy, int32_t* accepted, int32_t* common, int64_t* next, void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  LIA_VERIFY_NULL("lia_lm_verify", GREEDY_ARGS, hidden, lnw, emb, block_ids, greedy, accepted, common, next);
  if (!lnb) { lia_set_error("lia_lm_verify: NULL norm bias"); return LIA_ERR_INVALID; }
  return lm_verify_impl("lia_lm_verify", ctx, hidden, ldh, B, T, H, lnw, lnb, emb, vocab, eps, suppress_token, n_suppress, block_ids,
                        active, greedy, accepted, common, next, (hipStream_t)stream);
}

// lia_lm_verify with a bound per row: n_suppress_rows (device, int32 [B], each in [0, T] -- the caller's to guarantee; a larger entry
// suppresses at every block position, as T does) in place of the scalar
extern "C" int lia_lm_verify_rows(lia_ctx* ctx, const lia_bf16* hidden, long ldh, int B, int T, int H, const lia_bf16* lnw, const lia_bf16* lnb,
                                  const lia_bf16* emb, int vocab, float eps, int suppress_token, const int32_t* n_suppress_rows,
                                  const int64_t* block_ids, const int32_t* active, int64_t* greedy, int32_t* accepted, int32_t* common,
                                  int64_t* next, void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  LIA_VERIFY_NULL("lia_lm_verify_rows", GREEDY_ARGS, hidden, lnw, emb, block_ids, greedy, accepted, common, next);
  if (!lnb) { lia_set_error("lia_lm_verify_rows: NULL norm bias"); return LIA_ERR_INVALID; }
  if (!n_suppress_rows) { lia_set_error("lia_lm_verify_rows: NULL n_suppress_rows"); return LIA_ERR_INVALID; }
  return lm_verify_impl("lia_lm_verify_rows", ctx, hidden, ldh, B, T, H, lnw, lnb, emb, vocab, eps, suppress_token, 0, block_ids, active,
                        greedy, accepted, common, next, (hipStream_t)stream, n_suppress_rows);
}

extern "C" int lia_llama_lm_verify(lia_ctx* ctx, const lia_bf16* hidden, long ldh, int B, int T, int H, const lia_bf16* normw,
                                   const lia_bf16* lm, int vocab, float eps, int suppress_token, int n_suppress,
                                   const int64_t* block_ids, const int32_t* active, int64_t* greedy, int32_t* accepted,
                                   int32_t* common, int64_t* next, void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  LIA_VERIFY_NULL("lia_llama_lm_verify", GREEDY_ARGS, hidden, normw, lm, block_ids, greedy, accepted, common, next);
  return lm_verify_impl("lia_llama_lm_verify", ctx, hidden, ldh, B, T, H, normw, nullptr, lm, vocab, eps, suppress_token, n_suppress,
                        block_ids, active, greedy, accepted, common, next, (hipStream_t)stream);
}

// the sampled head.  norm_b == nullptr: RMSNorm (Llama), else LayerNorm
static int lm_verify_sample_impl(const char* who, lia_ctx* ctx, const bf16_t* hidden, long ldh, int B, int T, int H, const bf16_t* norm_w,
                                 const bf16_t* norm_b, const bf16_t* emb, int vocab, float eps, int suppress_token, int n_suppress,
                                 const int32_t* n_suppress_rows, const lia_block_sampler* smp, const int64_t* block_ids,
                                 const int32_t* active, int64_t* sampled, int32_t* accepted, int32_t* common, int64_t* next,
                                 float* p_draft, bf16_t* logits_out, hipStream_t st) {
  LiaHeadMods m;
  if (int mrc = head_mods_resolve(who, ctx, LiaHeadTakes{nullptr, nullptr, LIA_NO_BLOCK_PENALTIES}, (long)B * T, vocab, &m, [&] {
        if (!smp) { lia_set_error("%s: NULL sampler", who); return true; }
        if (!smp->uniforms) { lia_set_error("%s: NULL uniforms", who); return true; }
        return block_args_invalid(who, B, T, n_suppress, suppress_token, vocab) ||
               block_draw_invalid(who, B, vocab, smp->temperature, smp->top_k, smp->top_p, smp->ldu, smp->n_steps, smp->step0);
      }))
    return mrc;
  const LiaDraw draw{smp->temperature, smp->top_k, smp->top_p, smp->uniforms};
  hipError_t copy_err = hipSuccess;
  const int rc = lm_rows_chunked(who, ctx, hidden, ldh, B * T, H, norm_w, norm_b, emb, vocab, eps, st, [&](const bf16_t* logits, int r0, int n) {
    const LiaBlockDraw blk{{n_suppress, n_suppress_rows, T, r0}, smp->ldu, smp->n_steps, smp->step0, smp->step_rows, block_ids};
    pick_draw(m.mask, logits, vocab, n, vocab, draw, suppress_token, &blk, sampled, p_draft, st);
    sink_write(m.sink, logits, vocab, n, vocab, sampled + r0, r0, st);
    logits_out_copy(logits_out, logits, r0, n, vocab, st, &copy_err);
  });
  if (rc) return rc;
  HIP_TRY(copy_err);
  lia_verify_accept_launch(block_ids, sampled, active, B, T, accepted, common, next, st);
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

extern "C" int lia_lm_verify_sample(lia_ctx* ctx, const lia_bf16* hidden, long ldh, int B, int T, int H, const lia_bf16* lnw,
                                    const lia_bf16* lnb, const lia_bf16* emb, int vocab, float eps, int suppress_token, int n_suppress,
                                    const int32_t* n_suppress_rows, const lia_block_sampler* sampler, const int64_t* block_ids,
                                    const int32_t* active, int64_t* sampled, int32_t* accepted, int32_t* common, int64_t* next,
                                    float* p_draft, lia_bf16* logits_out, void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  LIA_VERIFY_NULL("lia_lm_verify_sample", SAMPLED_ARGS, hidden, lnw, emb, block_ids, sampled, accepted, common, next);
  if (!lnb) { lia_set_error("lia_lm_verify_sample: NULL norm bias"); return LIA_ERR_INVALID; }
  return lm_verify_sample_impl("lia_lm_verify_sample", ctx, hidden, ldh, B, T, H, lnw, lnb, emb, vocab, eps, suppress_token, n_suppress,
                               n_suppress_rows, sampler, block_ids, active, sampled, accepted, common, next, p_draft, logits_out,
                               (hipStream_t)stream);
}

extern "C" int lia_llama_lm_verify_sample(lia_ctx* ctx, const lia_bf16* hidden, long ldh, int B, int T, int H, const lia_bf16* normw,
                                          const lia_bf16* lm, int vocab, float eps, int suppress_token, int n_suppress,
                                          const int32_t* n_suppress_rows, const lia_block_sampler* sampler, const int64_t* block_ids,
                                          const int32_t* active, int64_t* sampled, int32_t* accepted, int32_t* common, int64_t* next,
                                          float* p_draft, lia_bf16* logits_out, void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  LIA_VERIFY_NULL("lia_llama_lm_verify_sample", SAMPLED_ARGS, hidden, normw, lm, block_ids, sampled, accepted, common, next);
  return lm_verify_sample_impl("lia_llama_lm_verify_sample", ctx, hidden, ldh, B, T, H, normw, nullptr, lm, vocab, eps, suppress_token,
                               n_suppress, n_suppress_rows, sampler, block_ids, active, sampled, accepted, common, next, p_draft,
                               logits_out, (hipStream_t)stream);
}

// the rejection head
static int lm_verify_reject_impl(const char* who, lia_ctx* ctx, const bf16_t* hidden, long ldh, int B, int T, int H, const bf16_t* norm_w,
                                 const bf16_t* norm_b, const bf16_t* emb, int vocab, float eps, int suppress_token, int n_suppress,
                                 const int32_t* n_suppress_rows, const lia_block_rejector* rej, const int64_t* block_ids,
                                 const int32_t* active, int64_t* token, int32_t* ok, int32_t* accepted, int32_t* common, int64_t* next,
                                 float* p_tok, float* q_tok, float* resid_mass, bf16_t* logits_out, hipStream_t st) {
  const LiaHeadTakes none{"rejection verification takes none -- the drafter's Q would have to be masked the same way",
                          "rejection verification writes none -- an accepted draft token is not this head's own output", LIA_NO_BLOCK_PENALTIES};
  LiaHeadMods m;
  if (int mrc = head_mods_resolve(who, ctx, none, (long)B * T, vocab, &m, [&] {
        if (!rej) { lia_set_error("%s: NULL rejector", who); return true; }
        if (!rej->draft_logits) { lia_set_error("%s: NULL draft_logits", who); return true; }
        if (!rej->u_acc) { lia_set_error("%s: NULL u_acc", who); return true; }
        if (!rej->u_res) { lia_set_error("%s: NULL u_res", who); return true; }
        if (n_suppress_rows) { lia_set_error("%s: n_suppress_rows must be NULL (rejection verification is common mode only)", who); return true; }
        if (block_args_invalid(who, B, T, n_suppress, suppress_token, vocab) ||
            block_draw_invalid(who, B, vocab, rej->temperature, rej->top_k, rej->top_p, rej->ldu, rej->n_steps, rej->step0))
          return true;
        if (rej->ldd_row < vocab) { lia_set_error("%s: ldd_row=%ld < vocab=%d", who, rej->ldd_row, vocab); return true; }
        if (rej->ldd_pos < vocab) { lia_set_error("%s: ldd_pos=%ld < vocab=%d", who, rej->ldd_pos, vocab); return true; }
        if (vocab % 8 == 0 && (((uintptr_t)rej->draft_logits & 15) || rej->ldd_row % 8 || rej->ldd_pos % 8)) {
          lia_set_error("%s: draft_logits=%p ldd_row=%ld ldd_pos=%ld: with vocab %% 8 == 0 the rows are read 16 bytes at a time -- a 16-byte "
                        "aligned pointer and pitches that are multiples of 8", who, (const void*)rej->draft_logits, rej->ldd_row, rej->ldd_pos);
          return true;
        }
        return false;
      }))
    return mrc;
  hipError_t copy_err = hipSuccess;
  const int rc = lm_rows_chunked(who, ctx, hidden, ldh, B * T, H, norm_w, norm_b, emb, vocab, eps, st, [&](const bf16_t* logits, int r0, int n) {
    lia_verify_reject_launch(logits, vocab, n, vocab, (const bf16_t*)rej->draft_logits, rej->ldd_row, rej->ldd_pos, rej->temperature, rej->top_k,
                             rej->top_p, suppress_token, n_suppress, T, r0, rej->u_acc, rej->u_res, rej->ldu, rej->n_steps, rej->step0,
                             block_ids, token, ok, p_tok, q_tok, resid_mass, st);
    logits_out_copy(logits_out, logits, r0, n, vocab, st, &copy_err);
  });
  if (rc) return rc;
  HIP_TRY(copy_err);
  lia_verify_reject_accept_launch(block_ids, token, ok, active, B, T, accepted, common, next, st);
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

extern "C" int lia_lm_verify_reject(lia_ctx* ctx, const lia_bf16* hidden, long ldh, int B, int T, int H, const lia_bf16* lnw,
                                    const lia_bf16* lnb, const lia_bf16* emb, int vocab, float eps, int suppress_token, int n_suppress,
                                    const int32_t* n_suppress_rows, const lia_block_rejector* rejector, const int64_t* block_ids,
                                    const int32_t* active, int64_t* token, int32_t* ok, int32_t* accepted, int32_t* common, int64_t* next,
                                    float* p_tok, float* q_tok, float* resid_mass, lia_bf16* logits_out, void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  LIA_VERIFY_NULL("lia_lm_verify_reject", REJECT_ARGS, hidden, lnw, emb, block_ids, token, ok, accepted, common, next);
  if (!lnb) { lia_set_error("lia_lm_verify_reject: NULL norm bias"); return LIA_ERR_INVALID; }
  return lm_verify_reject_impl("lia_lm_verify_reject", ctx, hidden, ldh, B, T, H, lnw, lnb, emb, vocab, eps, suppress_token, n_suppress,
                               n_suppress_rows, rejector, block_ids, active, token, ok, accepted, common, next, p_tok, q_tok, resid_mass,
                               logits_out, (hipStream_t)stream);
}

extern "C" int lia_llama_lm_verify_reject(lia_ctx* ctx, const lia_bf16* hidden, long ldh, int B, int T, int H, const lia_bf16* normw,
                                          const lia_bf16* lm, int vocab, float eps, int suppress_token, int n_suppress,
                                          const int32_t* n_suppress_rows, const lia_block_rejector* rejector, const int64_t* block_ids,
                                          const int32_t* active, int64_t* token, int32_t* ok, int32_t* accepted, int32_t* common,
                                          int64_t* next, float* p_tok, float* q_tok, float* resid_mass, lia_bf16* logits_out, void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  LIA_VERIFY_NULL("lia_llama_lm_verify_reject", REJECT_ARGS, hidden, normw, lm, block_ids, token, ok, accepted, common, next);
  return lm_verify_reject_impl("lia_llama_lm_verify_reject", ctx, hidden, ldh, B, T, H, normw, nullptr, lm, vocab, eps, suppress_token,
                               n_suppress, n_suppress_rows, rejector, block_ids, active, token, ok, accepted, common, next, p_tok, q_tok,
                               resid_mass, logits_out, (hipStream_t)stream);
}
