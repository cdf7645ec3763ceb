// C ABI of liblia_hip.so (include/lia_hip.h), part 3: layer descriptors, pack offsets, workspace layouts, the OPT and the Llama decoder-layer
// operators and the multi-layer decode runs.  No kernels here: see lia_internal.h for the launchers.
#include <algorithm>
#include <chrono>

#include "lia_internal.h"

// ------------------------------------------------------------------------------------------------
// packed layer layout / workspace sizing
// ------------------------------------------------------------------------------------------------
static int check_desc(const lia_layer_desc* d) {
  if (!d) return LIA_ERR_INVALID;
  if (d->hidden <= 0 || d->heads <= 0 || d->ffn <= 0 || d->hidden % d->heads) {
    lia_set_error("layer desc: hidden=%d heads=%d ffn=%d", d->hidden, d->heads, d->ffn);
    return LIA_ERR_INVALID;
  }
  int hd = d->hidden / d->heads;
  if (!(hd == 32 || hd == 64 || hd == 128) || d->hidden % 64 || d->ffn % 64) {
    lia_set_error("layer desc: head_dim %d must be 32/64/128 and hidden, ffn multiples of 64", hd);
    return LIA_ERR_INVALID;
  }
  return LIA_OK;
}

extern "C" int lia_layer_pack_offsets(const lia_layer_desc* d, size_t off[16], size_t* total) {
  int rc = check_desc(d);
  if (rc) return rc;
  const size_t H = d->hidden, F = d->ffn;
  size_t p = 0;
  auto put = [&](int idx, size_t elems, bool align) {
    if (align) p = align_up(p, 256);
    off[idx] = p;
    p += elems * 2;
  };
  // q.w | k.w | v.w contiguous = one [3H,H] operand; q.b | k.b | v.b contiguous = one [3H] bias
  put(2, H * H, true);  put(4, H * H, false);  put(6, H * H, false);
  put(3, H, true);      put(5, H, false);      put(7, H, false);
  put(8, H * H, true);  put(9, H, true);
  put(12, F * H, true); put(13, F, true);
  put(14, H * F, true); put(15, H, true);
  put(0, H, true);      put(1, H, true);
  put(10, H, true);     put(11, H, true);
  if (total) *total = align_up(p, 2048);   // 1024 bf16 values: the block size of the pack10 wire format
  return LIA_OK;
}

struct WsLayout {
  size_t ln, q, k, v, attn, h1, f1, slab[2], gemm, total;
  size_t gemm_bytes;
};

static WsLayout ws_layout(const lia_layer_desc* d, long rows, long slab_rows) {
  WsLayout w;
  const size_t H = d->hidden, F = d->ffn, R = (size_t)rows;
  size_t p = 0;
  auto take = [&](size_t bytes) { size_t o = p; p = align_up(p + bytes, 256); return o; };
  w.ln = take(R * H * 2);
  w.q = take(R * H * 2);   // q | k | v contiguous: the policy-2 round trip moves them in one copy
  w.k = take(R * H * 2);
  w.v = take(R * H * 2);
  w.attn = take(R * H * 2);
  w.h1 = take(R * H * 2);
  w.f1 = take(R * F * 2);
  w.slab[0] = take(2 * (size_t)slab_rows * H * 2);
  w.slab[1] = take(2 * (size_t)slab_rows * H * 2);
  // split-K slabs of the skinny regime (M <= 256).  Reserved for larger calls too, so that the size is monotonic in `rows`: a
  // context sized for a 292-row call must also serve a 256-row one (r01 sized 16 MB for 292 rows and then needed 82 MB for 256)
  w.gemm_bytes = (size_t)8 * std::min(R, (size_t)256) * std::max(3 * H, F) * 4;
  w.gemm = take(w.gemm_bytes);
  w.total = p;
  return w;
}

extern "C" size_t lia_layer_workspace_bytes(const lia_layer_desc* d, int max_rows) {
  if (check_desc(d) || max_rows <= 0) return 0;
  return ws_layout(d, max_rows, max_rows).total;
}

// ------------------------------------------------------------------------------------------------
// the decoder-layer operator
// ------------------------------------------------------------------------------------------------
static int ensure_host_stage(lia_ctx* c, size_t bytes) {
  if (c->host_stage_bytes >= bytes) return LIA_OK;
  if (c->host_stage) (void)hipHostFree(c->host_stage);
  c->host_stage = nullptr;
  c->host_stage_bytes = 0;
  HIP_TRY(hipHostMalloc((void**)&c->host_stage, bytes, hipHostMallocDefault));
  c->host_stage_bytes = bytes;
  return LIA_OK;
}

// The split-key route's scratch for the GPU attention of one layer call over S keys (decode_shaped: one query per row), placed behind
// the call's own workspace layout.  A call that does not take the route needs exactly the workspace it needed before; one sent there
// by LIA_OPT_SPLIT_DECODE alone falls back to the one-workgroup kernel when the scratch does not fit; one beyond that kernel's LDS
// bound is refused here, before anything is launched.
static int split_scratch_place(lia_ctx* ctx, const char* who, bool decode_shaped, int B, int S, int heads, int kv_heads, int hd, size_t layout) {
  LiaAttnOpts& o = ctx->attn_opts;
  o.split_scratch = nullptr;
  o.split_scratch_bytes = 0;
  const int route = decode_shaped ? lia_attn_split_route(o.split_decode, S, heads, kv_heads, hd) : 0;
  if (!route) return LIA_OK;
  const size_t need = lia_attn_split_scratch_bytes(B, S, heads, kv_heads, hd);
  if (layout + need > ctx->ws_bytes) {
    if (route == 1) return LIA_OK;
    lia_set_error("%s: workspace %zu < %zu + %zu bytes of split-key attention scratch (%d keys are beyond the one-workgroup decode kernel)",
                  who, ctx->ws_bytes, layout, need, S);
    return LIA_ERR_MEMORY;
  }
  o.split_scratch = ctx->ws + layout;
  o.split_scratch_bytes = need;
  return LIA_OK;
}

// tail = 1 (lia_layer_forward_last): LN1 and the q | k | v projection run on all B x T rows (the cache needs every K/V row), everything
// behind them -- attention, out-proj, LN2, fc1, fc2 -- only on the LAST position of each row; y is then [B, 1, H].
static int layer_forward_impl(lia_ctx* ctx, const lia_layer_desc* d, int policy, const void* const weights[16], const lia_bf16* x,
                              lia_bf16* y, lia_kv* kv, int B, int T, int pos0, int b0, void* stream, int tail) {
  if (!ctx) return LIA_ERR_INVALID;
  int rc = check_desc(d);
  if (rc) return rc;
  if (!weights || !x || !y || !kv || !kv->k || !kv->v) { lia_set_error("lia_layer_forward: NULL tensor"); return LIA_ERR_MISSING; }
  for (int i = 0; i < 16; ++i)
    if (!weights[i]) { lia_set_error("lia_layer_forward: weights[%d] is NULL", i); return LIA_ERR_MISSING; }
  if (policy != 0 && policy != 2 && policy != 3) {
    lia_set_error("lia_layer_forward: policy %d is not a GPU policy (0, 2, 3)", policy);
    return LIA_ERR_INVALID;
  }
  if (B <= 0 || T <= 0 || pos0 < 0 || b0 < 0 || b0 + B > kv->batch || pos0 + T > kv->smax) {
    lia_set_error("lia_layer_forward: B=%d T=%d pos0=%d b0=%d vs cache batch=%d smax=%d", B, T, pos0, b0, kv->batch, kv->smax);
    return LIA_ERR_INVALID;
  }
  if (tail && (policy == 2 || T < 2)) { lia_set_error("lia_layer_forward_last: a GPU-attention prefill (policy 0 / 3, T > 1) only"); return LIA_ERR_INVALID; }
  if ((policy == 3) != (kv->on_device != 0)) {
    lia_set_error("lia_layer_forward: policy %d needs a %s cache", policy, policy == 3 ? "device" : "host");
    return LIA_ERR_INVALID;
  }
  // left padding (lia_ctx_set_key_starts): the table's rows b0 .. b0 + B - 1 -- the generation's rows, whatever the layout of the
  // K / V destination below (the policy-0 slab has rows 0 .. B - 1 of its own)
  const int* kst_dev = nullptr;
  const int* kst_host = nullptr;
  if (ctx->key_starts_n) {
    if (b0 + B > ctx->key_starts_n) {
      lia_set_error("lia_layer_forward: rows %d..%d beyond the %d rows of the key-start table", b0, b0 + B - 1, ctx->key_starts_n);
      return LIA_ERR_INVALID;
    }
    kst_host = ctx->key_starts->data() + b0;
    kst_dev = ctx->key_starts_dev + b0;
    for (int b = 0; b < B; ++b)
      if (kst_host[b] > pos0 + T - 1) {
        lia_set_error("lia_layer_forward: row %d starts at %d, beyond its last position %d", b0 + b, kst_host[b], pos0 + T - 1);
        return LIA_ERR_INVALID;
      }
    // a block appended to a non-empty cache has no pad query rows: every row's sequence began at or before the block
    if (T > 1 && pos0 > 0)
      for (int b = 0; b < B; ++b)
        if (kst_host[b] > pos0) {
          lia_set_error("lia_layer_forward: row %d starts at %d, inside the block appended at %d", b0 + b, kst_host[b], pos0);
          return LIA_ERR_INVALID;
        }
  }
  // ragged cache (lia_ctx_set_row_lens): rows b0 .. b0 + B - 1 of the table are the rows' own base lengths; pos0 = max(lens) only
  // sizes buffers.  Policy 3 with T >= 2 only: K / V go to the plain workspace buffers and a scatter kernel places them, the
  // attention is the ragged block launch -- always, there is no append fallback behind per-row lengths
  const bool ragged = ctx->row_lens_n > 0;
  const int* lens_dev = nullptr;
  if (ragged) {
    if (policy != 3 || !kv->on_device) {
      lia_set_error("lia_layer_forward: row lengths are set (ragged cache), which serves policy 3 with the cache in HBM only; got policy %d with a %s cache",
                    policy, kv->on_device ? "device" : "host");
      return LIA_ERR_INVALID;
    }
    if (T < 2) { lia_set_error("lia_layer_forward: row lengths are set (ragged cache): a block of T >= 2 tokens only, got T=%d", T); return LIA_ERR_INVALID; }
    if (tail) { lia_set_error("lia_layer_forward_last: row lengths are set (ragged cache): the tail form is not served"); return LIA_ERR_INVALID; }
    if (b0 + B > ctx->row_lens_n) {
      lia_set_error("lia_layer_forward: rows %d..%d beyond the %d rows of the row-length table", b0, b0 + B - 1, ctx->row_lens_n);
      return LIA_ERR_INVALID;
    }
    const int* lens_host = ctx->row_lens->data() + b0;
    for (int b = 0; b < B; ++b) {
      if (lens_host[b] < 1 || lens_host[b] > pos0 || lens_host[b] + T > kv->smax) {
        lia_set_error("lia_layer_forward: row %d holds %d positions: outside 1 .. pos0 = %d (the largest row length), or its block of %d overruns the cache's %d",
                      b0 + b, lens_host[b], pos0, T, kv->smax);
        return LIA_ERR_INVALID;
      }
      if (kst_host && kst_host[b] > lens_host[b]) {
        lia_set_error("lia_layer_forward: row %d starts at %d, behind its %d cached positions", b0 + b, kst_host[b], lens_host[b]);
        return LIA_ERR_INVALID;
      }
    }
    if (!lia_attn_block_takes(d->heads, d->heads, d->hidden / d->heads, T, pos0 + T)) {
      lia_set_error("lia_layer_forward: row lengths are set (ragged cache), and the ragged block attention does not take %d heads x T=%d at %d keys "
                    "(at most 16 query slots per KV head, scores within 160 KB of LDS)", d->heads, T, pos0 + T);
      return LIA_ERR_INVALID;
    }
    lens_dev = ctx->row_lens_dev + b0;
  }
  const int H = d->hidden, F = d->ffn, hd = H / d->heads;
  const long M = (long)B * T;
  // policy 0 on a non-empty cache (a decode step, an appended block) parks the cached prefix and the call's rows, [pos0+T][B][H]
  // (K and V), in a slab
  const WsLayout w = ws_layout(d, M, policy == 0 ? (long)(pos0 + T) * B : M);
  if (w.total > ctx->ws_bytes) {
    lia_set_error("lia_layer_forward: workspace %zu < %zu needed for %ld rows", ctx->ws_bytes, w.total, M);
    return LIA_ERR_MEMORY;
  }
  rc = split_scratch_place(ctx, "lia_layer_forward", (T == 1 || tail) && policy != 2 && !ragged, B, pos0 + T, d->heads, d->heads, hd, w.total);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  {
    // a K/V delivery still draining from a slab of a DIFFERENT layout could overlap this call's buffers
    const long sr = policy == 0 ? (long)(pos0 + T) * B : M;
    if (ctx->last_rows != M || ctx->last_slab_rows != sr) {
      for (int i = 0; i < 2; ++i)
        if (ctx->slab_used[i]) HIP_TRY(hipStreamWaitEvent(st, ctx->slab_done[i], 0));
      ctx->last_rows = M;
      ctx->last_slab_rows = sr;
    }
  }
  char* ws = ctx->ws;
  bf16_t *ln = (bf16_t*)(ws + w.ln), *qb = (bf16_t*)(ws + w.q), *kb = (bf16_t*)(ws + w.k), *vb = (bf16_t*)(ws + w.v);
  bf16_t *ao = (bf16_t*)(ws + w.attn), *h1 = (bf16_t*)(ws + w.h1), *f1 = (bf16_t*)(ws + w.f1);
  float* gws = (float*)(ws + w.gemm);
  const bf16_t* const* W = (const bf16_t* const*)weights;
  const bool fused_qkv = (W[4] == W[2] + (size_t)H * H) && (W[6] == W[4] + (size_t)H * H) && (W[5] == W[3] + H) &&
                         (W[7] == W[5] + H);
  const float eps = d->ln_eps;
  const size_t S = (size_t)pos0 + T;
  // rows behind the projection: all of them, or the last position of each batch row (row b*T + T-1: stride T*H)
  const LiaTail tl = lia_tail(tail, B, T, H);
  const long Mt = tl.rows;
  // chaining state: a hint for THIS call's last GEMM, and whether the previous call already left LN1(x) in `ln`
  const LiaChain chain = chain_take(ctx, x, ln, M, H);

  // LN1 (decoder.py:199-206)
  if (!chain.have_norm1) lia_layernorm_launch(x, H, W[0], W[1], ln, H, M, H, eps, st);

  // destinations of the fresh K/V rows
  bf16_t *kdst, *vdst;
  int dst_batch, dst_b0, dst_pos0;
  bool cache_mode = true;
  int slab = -1;
  if (ragged) {   // plain [M,H] buffers; lia_kv_scatter_ragged_launch places the rows behind the projection
    kdst = kb; vdst = vb; dst_batch = B; dst_b0 = 0; dst_pos0 = 0; cache_mode = false;
  } else if (policy == 3) {
    kdst = kv->k; vdst = kv->v; dst_batch = kv->batch; dst_b0 = b0; dst_pos0 = pos0;
  } else if (policy == 0) {
    // device slab [S][B][h][d] shared by K then V; two slabs alternate so the previous delivery may still drain
    slab = ctx->slab_next; ctx->slab_next ^= 1;
    if (ctx->slab_used[slab]) HIP_TRY(hipStreamWaitEvent(st, ctx->slab_done[slab], 0));
    kdst = (bf16_t*)(ws + w.slab[slab]); vdst = kdst + S * B * H;
    dst_batch = B; dst_b0 = 0; dst_pos0 = pos0;
    if (pos0 > 0) {
      // intended semantics of the reference's decode policy 0 (modeling_opt.py:1379-1491; its own
      // implementation is not an oracle): bring the cached rows to the GPU, attend there
      const size_t width = (size_t)B * H * 2, pitch = (size_t)kv->batch * H * 2;
      HIP_TRY(hipMemcpy2DAsync(kdst, width, kv->k + (size_t)b0 * H, pitch, width, pos0, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpy2DAsync(vdst, width, kv->v + (size_t)b0 * H, pitch, width, pos0, hipMemcpyHostToDevice, st));
    }
  } else {  // policy 2: plain [M,H] buffers that travel to the host
    kdst = kb; vdst = vb; dst_batch = B; dst_b0 = 0; dst_pos0 = 0; cache_mode = false;
  }

  // q | k | v projection (attentions.py:393-394, 418)
  if (fused_qkv) {
    rc = qkv_project(ctx, ln, W[2], W[3], qb, kdst, vdst, cache_mode, B, T, H, dst_batch, dst_b0, dst_pos0, gws, w.gemm_bytes, st);
    if (rc) return rc;
  } else {
    for (int i = 0; i < 3; ++i) {
      LiaEpilogue ep{W[3 + 2 * i], nullptr, 0, 0};
      LiaOutMap om = plain_out(i == 0 ? qb : (i == 1 ? kdst : vdst), H, H);
      if (i > 0 && cache_mode) { om.cache_mode[0] = 1; om.T = T; om.Bc = dst_batch; om.b0 = dst_b0; om.pos0 = dst_pos0; }
      rc = gemm_checked(ctx, ln, H, W[2 + 2 * i], (int)M, H, H, ep, om, gws, w.gemm_bytes, 0, st);
      if (rc) return rc;
    }
  }

  if (ragged) {
    lia_kv_scatter_ragged_launch(kb, vb, kv->k, kv->v, B, T, H, kv->batch, b0, lens_dev, st);
    if (lia_attn_block_ragged_launch(qb, H, kv->k, kv->v, ao, H, B, T, pos0, d->heads, d->heads, hd, kv->batch, b0, 0, kst_dev, lens_dev, st)) {
      lia_set_error("ragged attention: unsupported head_dim %d / S %zu", hd, S);
      return LIA_ERR_INVALID;
    }
    ++ctx->attn_opts.block_launches;
  } else if (policy == 2) {
    // q, k, v -> host; host attention over the host cache; result back (attentions.py:421-440)
    const size_t one = (size_t)M * H * 2;
    rc = ensure_host_stage(ctx, 4 * one);
    if (rc) return rc;
    bf16_t* hq = (bf16_t*)ctx->host_stage;
    bf16_t *hk = hq + (size_t)M * H, *hv = hk + (size_t)M * H, *ha = hv + (size_t)M * H;
    // kernel blits over the mapped pinned buffer, not SDMA copies (see lia_blit_kernel)
    lia_blit_launch(hq, qb, one, st);
    lia_blit_launch(hk, kb, one, st);
    lia_blit_launch(hv, vb, one, st);
    HIP_TRY(hipStreamSynchronize(st));
    const auto ha_t0 = std::chrono::steady_clock::now();
    rc = kst_host ? lia_host_attention_padded(hq, hk, hv, kv->k, kv->v, ha, B, T, pos0, d->heads, hd, kv->batch, b0, ctx->host_threads, kst_host)
                  : lia_host_attention(hq, hk, hv, kv->k, kv->v, ha, B, T, pos0, d->heads, hd, kv->batch, b0, ctx->host_threads);
    if (rc) return rc;
    if (ctx->prof_on) {
      ctx->prof_host_attn_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ha_t0).count();
      ctx->prof_host_attn_calls++;
    }
    lia_blit_launch(ao, ha, one, st);
  } else {
    // GPU attention (attentions.py:443-536)
    // (tail: the last query of a causal block attends every key -- one decode-style query per row over the S rows just written)
    // (a block of T > 1 queries behind pos0 > 0 cached positions: the append kernels, query frame offset from the key frame)
    if (lia_attn_dispatch(qb, H, kdst, vdst, ao, H, B, T, pos0, d->heads, d->heads, hd, dst_batch, dst_b0, 0, kst_dev, tail, st, &ctx->attn_opts)) {
      lia_set_error("attention: unsupported head_dim %d / S %zu", hd, S);
      return LIA_ERR_INVALID;
    }
    if (policy == 0) {
      // deliver rows [pos0, pos0+T) of batch rows [b0, b0+B) to the host cache
      HIP_TRY(hipEventRecord(ctx->slab_ready[slab], st));
      HIP_TRY(hipStreamWaitEvent(ctx->d2h, ctx->slab_ready[slab], 0));
      const size_t width = (size_t)B * H * 2, pitch = (size_t)kv->batch * H * 2;
      lia_bf16* hk = kv->k + ((size_t)pos0 * kv->batch + b0) * H;
      lia_bf16* hv = kv->v + ((size_t)pos0 * kv->batch + b0) * H;
      // Always the strided 2-D path, even when width == pitch: the runtime serves it with a blit kernel, which
      // shares PCIe with the weight stream gracefully.  A linear copy would go to the SDMA queue behind the
      // 1.2 GB weight copies (measured: prefill 1057 ms -> 1335 ms with four slots).
      HIP_TRY(hipMemcpy2DAsync(hk, pitch, kdst + (size_t)pos0 * B * H, width, width, T, hipMemcpyDeviceToHost, ctx->d2h));
      HIP_TRY(hipMemcpy2DAsync(hv, pitch, vdst + (size_t)pos0 * B * H, width, width, T, hipMemcpyDeviceToHost, ctx->d2h));
      HIP_TRY(hipEventRecord(ctx->slab_done[slab], ctx->d2h));
      ctx->slab_used[slab] = true;
    }
  }

  // out-proj + bias, residual (decoder.py:225-229); LN2 (:268-276) rides in the split-K combine when there is one
  int ln2_done = 0;
  {
    LiaEpilogue ep{W[9], x + tl.off, tl.ld, 0};
    LiaOutMap om = plain_out(h1, H, H);
    LiaPost post{};
    post.kind = LIA_POST_LAYERNORM; post.g = W[10]; post.b = W[11]; post.eps = eps; post.out = ln; post.ldo = H;
    rc = gemm_checked(ctx, ao, H, W[8], (int)Mt, H, H, ep, om, gws, w.gemm_bytes, 0, st, &post, &ln2_done);
    if (rc) return rc;
  }
  // fc1 + relu (:282-285), fc2 + residual (:306-310)
  if (!ln2_done) lia_layernorm_launch(h1, H, W[10], W[11], ln, H, Mt, H, eps, st);
  {
    LiaEpilogue ep{W[13], nullptr, 0, 1};
    LiaOutMap om = plain_out(f1, F, F);
    rc = gemm_checked(ctx, ln, H, W[12], (int)Mt, F, H, ep, om, gws, w.gemm_bytes, 0, st);
    if (rc) return rc;
  }
  {
    LiaEpilogue ep{W[15], h1, H, 0};
    LiaOutMap om = plain_out(y, H, H);
    LiaPost post{};
    int chained = 0;
    if (chain.g && chain.b) { post.kind = LIA_POST_LAYERNORM; post.g = chain.g; post.b = chain.b; post.eps = eps; post.out = ln; post.ldo = H; }
    rc = gemm_checked(ctx, f1, F, W[14], (int)Mt, H, F, ep, om, gws, w.gemm_bytes, 0, st, post.kind ? &post : nullptr, &chained);
    if (rc) return rc;
    if (chained) chain_publish(ctx, y, ln, Mt, H);
  }
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

extern "C" int lia_layer_forward(lia_ctx* ctx, const lia_layer_desc* d, int policy, const void* const weights[16],
                                 const lia_bf16* x, lia_bf16* y, lia_kv* kv, int B, int T, int pos0, int b0, void* stream) {
  return layer_forward_impl(ctx, d, policy, weights, x, y, kv, B, T, pos0, b0, stream, 0);
}

extern "C" int lia_layer_forward_last(lia_ctx* ctx, const lia_layer_desc* d, int policy, const void* const weights[16],
                                      const lia_bf16* x, lia_bf16* y_last, lia_kv* kv, int B, int T, int pos0, int b0, void* stream) {
  return layer_forward_impl(ctx, d, policy, weights, x, y_last, kv, B, T, pos0, b0, stream, 1);
}

// ------------------------------------------------------------------------------------------------
// Llama-family layer (config 4, build-defined): RMSNorm, RoPE, grouped-query attention, SiLU-gated MLP
// ------------------------------------------------------------------------------------------------
static int check_llama_desc(const lia_llama_desc* d) {
  if (!d) return LIA_ERR_INVALID;
  if (d->hidden <= 0 || d->heads <= 0 || d->kv_heads <= 0 || d->ffn <= 0 || d->hidden % d->heads || d->heads % d->kv_heads) {
    lia_set_error("llama desc: hidden=%d heads=%d kv_heads=%d ffn=%d", d->hidden, d->heads, d->kv_heads, d->ffn);
    return LIA_ERR_INVALID;
  }
  int hd = d->hidden / d->heads;
  if (!(hd == 32 || hd == 64 || hd == 128) || d->hidden % 128 || d->ffn % 128 || (d->kv_heads * hd) % 16) {
    lia_set_error("llama desc: head_dim %d must be 32/64/128, hidden and ffn multiples of 128", hd);
    return LIA_ERR_INVALID;
  }
  if (d->gu_block != 0 && d->gu_block != LIA_GU_BLOCK) {
    lia_set_error("llama desc: gu_block %d (0 = gate.w | up.w as they are, %d = interleaved in blocks of %d rows)", d->gu_block, LIA_GU_BLOCK, LIA_GU_BLOCK);
    return LIA_ERR_INVALID;
  }
  return LIA_OK;
}

extern "C" int lia_llama_pack_offsets(const lia_llama_desc* d, size_t off[9], size_t* total) {
  int rc = check_llama_desc(d);
  if (rc) return rc;
  const size_t H = d->hidden, F = d->ffn, KD = (size_t)d->kv_heads * (H / d->heads);
  size_t p = 0;
  auto put = [&](int idx, size_t elems, bool align) { if (align) p = align_up(p, 256); off[idx] = p; p += elems * 2; };
  put(1, H * H, true);                            // q
  put(2, KD * H, true); put(3, KD * H, false);    // k | v adjacent: one [2*KD, H] GEMM
  put(4, H * H, true);                            // o
  put(6, F * H, true); put(7, F * H, false);      // gate | up adjacent: one [2F, H] GEMM
  put(8, H * F, true);                            // down
  put(0, H, true); put(5, H, true);               // the two RMSNorm weights
  if (total) *total = align_up(p, 2048);
  return LIA_OK;
}

struct LlamaWs { size_t ln, q, attn, h1, gu, act, gemm, gemm_bytes, total; };
static LlamaWs llama_ws(const lia_llama_desc* d, long rows) {
  LlamaWs w;
  const size_t H = d->hidden, F = d->ffn, R = (size_t)rows;
  size_t p = 0;
  auto take = [&](size_t bytes) { size_t o = p; p = align_up(p + bytes, 256); return o; };
  w.ln = take(R * H * 2); w.q = take(R * H * 2); w.attn = take(R * H * 2); w.h1 = take(R * H * 2);
  w.gu = take(R * 2 * F * 2); w.act = take(R * F * 2);
  w.gemm_bytes = (size_t)8 * std::min(R, (size_t)256) * 2 * F * 4;   // monotonic in rows, see ws_layout
  w.gemm = take(w.gemm_bytes);
  w.total = p;
  return w;
}

extern "C" size_t lia_llama_workspace_bytes(const lia_llama_desc* d, int max_rows) {
  if (check_llama_desc(d) || max_rows <= 0) return 0;
  return llama_ws(d, max_rows).total;
}

// tail = 1 (lia_llama_layer_forward_last): see layer_forward_impl -- norm, q | k | v projection and RoPE on every row, the rest on the
// last position of each row; y is [B, 1, H]
static int llama_layer_forward_impl(lia_ctx* ctx, const lia_llama_desc* d, const void* const weights[9], const lia_bf16* x,
                                    lia_bf16* y, lia_kv* kv, const lia_bf16* cos_table, const lia_bf16* sin_table, int B, int T,
                                    int pos0, int b0, void* stream, int tail) {
  if (!ctx) return LIA_ERR_INVALID;
  int rc = check_llama_desc(d);
  if (rc) return rc;
  if (!weights || !x || !y || !kv || !kv->k || !kv->v || !cos_table || !sin_table) { lia_set_error("lia_llama_layer_forward: NULL tensor"); return LIA_ERR_MISSING; }
  for (int i = 0; i < 9; ++i)
    if (!weights[i]) { lia_set_error("lia_llama_layer_forward: weights[%d] is NULL", i); return LIA_ERR_MISSING; }
  if (!kv->on_device) { lia_set_error("lia_llama_layer_forward: the KV cache must live on the device"); return LIA_ERR_INVALID; }
  if (B <= 0 || T <= 0 || pos0 < 0 || b0 < 0 || b0 + B > kv->batch || pos0 + T > kv->smax) {
    lia_set_error("lia_llama_layer_forward: B=%d T=%d pos0=%d b0=%d vs cache batch=%d smax=%d", B, T, pos0, b0, kv->batch, kv->smax);
    return LIA_ERR_INVALID;
  }
  if (tail && T < 2) { lia_set_error("lia_llama_layer_forward_last: a multi-token prefill only"); return LIA_ERR_INVALID; }
  const int H = d->hidden, F = d->ffn, hd = H / d->heads, KD = d->kv_heads * hd;
  const long M = (long)B * T;
  const LiaTail tl = lia_tail(tail, B, T, H);
  const long Mt = tl.rows;
  const LlamaWs w = llama_ws(d, M);
  if (w.total > ctx->ws_bytes) { lia_set_error("lia_llama_layer_forward: workspace %zu < %zu", ctx->ws_bytes, w.total); return LIA_ERR_MEMORY; }
  rc = split_scratch_place(ctx, "lia_llama_layer_forward", T == 1 || tail, B, pos0 + T, d->heads, d->kv_heads, hd, w.total);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  char* ws = ctx->ws;
  bf16_t *ln = (bf16_t*)(ws + w.ln), *qb = (bf16_t*)(ws + w.q), *ao = (bf16_t*)(ws + w.attn), *h1 = (bf16_t*)(ws + w.h1);
  bf16_t *gu = (bf16_t*)(ws + w.gu), *act = (bf16_t*)(ws + w.act);
  float* gws = (float*)(ws + w.gemm);
  const bf16_t* const* W = (const bf16_t* const*)weights;
  const LiaEpilogue none{nullptr, nullptr, 0, 0};
  // chaining state (see lia_layer_forward)
  const LiaChain chain = chain_take(ctx, x, ln, M, H);

  if (!chain.have_norm1) lia_rmsnorm_launch(x, H, W[0], ln, H, M, H, d->rms_eps, st);
  const bool fused_kv = W[3] == W[2] + (size_t)KD * H;
  const int G = d->heads / d->kv_heads;
  // q | k | v in ONE GEMM when the three weights are adjacent (they are in lia_llama_pack_offsets' layer buffer): the q columns
  // are G segments of the k / v width, the k and v segments scatter into the seq-major cache; in decode the rotation of the q and
  // k heads rides in the split-K combine
  const bool fused_qkv = fused_kv && W[2] == W[1] + (size_t)H * H && G + 2 <= LIA_OUT_SEGS;
  int rope_done = 0;
  if (fused_qkv) {
    LiaOutMap om;
    memset(&om, 0, sizeof(om));
    for (int j = 0; j < G; ++j) { om.base[j] = qb + (size_t)j * KD; om.ld[j] = H; }
    om.base[G] = kv->k; om.base[G + 1] = kv->v; om.ld[G] = om.ld[G + 1] = KD; om.cache_mode[G] = om.cache_mode[G + 1] = 1;
    om.seg_n = KD; om.T = T; om.Bc = kv->batch; om.b0 = b0; om.pos0 = pos0;
    LiaPost post{};
    post.kind = LIA_POST_ROPE; post.cos_t = cos_table; post.sin_t = sin_table; post.rot_heads = d->heads + d->kv_heads; post.hd = hd;
    post.pos0 = pos0; post.T = T;
    rc = gemm_checked(ctx, ln, H, W[1], (int)M, H + 2 * KD, H, none, om, gws, w.gemm_bytes, 0, st, &post, &rope_done);
    if (rc) return rc;
  } else {  // q projection
    LiaOutMap om = plain_out(qb, H, H);
    rc = gemm_checked(ctx, ln, H, W[1], (int)M, H, H, none, om, gws, w.gemm_bytes, 0, st);
    if (rc) return rc;
  }
  for (int part = 0; part < (fused_qkv ? 0 : (fused_kv ? 1 : 2)); ++part) {  // k | v projection, rows scattered into the seq-major cache
    LiaOutMap om;
    memset(&om, 0, sizeof(om));
    if (fused_kv) { om.base[0] = kv->k; om.base[1] = kv->v; om.cache_mode[0] = om.cache_mode[1] = 1; om.ld[0] = om.ld[1] = KD; }
    else { om.base[0] = part == 0 ? kv->k : kv->v; om.cache_mode[0] = 1; om.ld[0] = KD; }
    om.seg_n = KD; om.T = T; om.Bc = kv->batch; om.b0 = b0; om.pos0 = pos0;
    rc = gemm_checked(ctx, ln, H, fused_kv ? W[2] : W[2 + part], (int)M, fused_kv ? 2 * KD : KD, H, none, om, gws, w.gemm_bytes, 0, st);
    if (rc) return rc;
  }
  // RoPE on q (token rows b*T+t) and on the K rows just written (cache rows t*Bc + b); HF caches post-RoPE keys
  if (!rope_done) {
    lia_rope_launch(qb, H, cos_table, sin_table, M, d->heads, hd, pos0, T, 0, st);
    if (b0 == 0 && B == kv->batch) {
      lia_rope_launch(kv->k + (size_t)pos0 * kv->batch * KD, KD, cos_table, sin_table, (long)T * B, d->kv_heads, hd, pos0, 0, kv->batch, st);
    } else {
      for (int t = 0; t < T; ++t)  // minibatch slice of the cache rows: one launch per position
        lia_rope_launch(kv->k + ((size_t)(pos0 + t) * kv->batch + b0) * KD, KD, cos_table, sin_table, B, d->kv_heads, hd, pos0 + t, 0,
                        kv->batch + B, st);
    }
  }
  if (lia_attn_dispatch(qb, H, kv->k, kv->v, ao, H, B, T, pos0, d->heads, d->kv_heads, hd, kv->batch, b0, 1, nullptr, tail, st, &ctx->attn_opts)) {
    lia_set_error("llama attention: unsupported head_dim %d / S %d", hd, pos0 + T);
    return LIA_ERR_INVALID;
  }
  int norm2_done = 0, silu_done = 0;
  {  // o_proj + residual; the post-attention RMSNorm rides in the split-K combine when there is one
    LiaEpilogue ep{nullptr, x + tl.off, tl.ld, 0};
    LiaOutMap om = plain_out(h1, H, H);
    LiaPost post{};
    post.kind = LIA_POST_RMSNORM; post.g = W[5]; post.eps = d->rms_eps; post.out = ln; post.ldo = H;
    rc = gemm_checked(ctx, ao, H, W[4], (int)Mt, H, H, ep, om, gws, w.gemm_bytes, 0, st, &post, &norm2_done);
    if (rc) return rc;
  }
  if (!norm2_done) lia_rmsnorm_launch(h1, H, W[5], ln, H, Mt, H, d->rms_eps, st);
  const bool fused_gu = W[7] == W[6] + (size_t)F * H;
  if (fused_gu) {
    LiaOutMap om = plain_out(gu, 2 * F, 2 * F);
    LiaPost post{};
    post.kind = LIA_POST_SILU_MUL; post.out = act; post.ldo = F;     // act = silu(gate) * up straight from the combine / the tiled epilogue
    post.gu_block = d->gu_block;
    rc = gemm_checked(ctx, ln, H, W[6], (int)Mt, 2 * F, H, none, om, gws, w.gemm_bytes, 0, st, &post, &silu_done);
    if (rc) return rc;
  } else {
    for (int part = 0; part < 2; ++part) {
      LiaOutMap om = plain_out(gu + (size_t)part * F, 2 * F, F);
      rc = gemm_checked(ctx, ln, H, W[6 + part], (int)Mt, F, H, none, om, gws, w.gemm_bytes, 0, st);
      if (rc) return rc;
    }
  }
  if (!silu_done) lia_silu_mul_launch(gu, act, Mt, F, fused_gu ? d->gu_block : 0, st);
  {  // down_proj + residual (+ the next layer's input RMSNorm when the caller chained it)
    LiaEpilogue ep{nullptr, h1, H, 0};
    LiaOutMap om = plain_out(y, H, H);
    LiaPost post{};
    int chained = 0;
    if (chain.g) { post.kind = LIA_POST_RMSNORM; post.g = chain.g; post.eps = d->rms_eps; post.out = ln; post.ldo = H; }
    rc = gemm_checked(ctx, act, F, W[8], (int)Mt, H, F, ep, om, gws, w.gemm_bytes, 0, st, post.kind ? &post : nullptr, &chained);
    if (rc) return rc;
    if (chained) chain_publish(ctx, y, ln, Mt, H);
  }
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

extern "C" int lia_llama_layer_forward(lia_ctx* ctx, const lia_llama_desc* d, const void* const weights[9], const lia_bf16* x,
                                       lia_bf16* y, lia_kv* kv, const lia_bf16* cos_table, const lia_bf16* sin_table, int B, int T,
                                       int pos0, int b0, void* stream) {
  return llama_layer_forward_impl(ctx, d, weights, x, y, kv, cos_table, sin_table, B, T, pos0, b0, stream, 0);
}

extern "C" int lia_llama_layer_forward_last(lia_ctx* ctx, const lia_llama_desc* d, const void* const weights[9], const lia_bf16* x,
                                            lia_bf16* y_last, lia_kv* kv, const lia_bf16* cos_table, const lia_bf16* sin_table, int B,
                                            int T, int pos0, int b0, void* stream) {
  return llama_layer_forward_impl(ctx, d, weights, x, y_last, kv, cos_table, sin_table, B, T, pos0, b0, stream, 1);
}

// ------------------------------------------------------------------------------------------------
// decode step over a run of HBM-resident layers in one call, layer by layer through the per-op route, each layer's last combine
// also computing the next layer's first norm (lia_ctx_chain_next_norm).  (r04 also had a persistent per-layer "chain" kernel
// behind a switch here; bit-identical, measured 4-9 % slower per step -- a seam inside a launch costs what a kernel boundary
// costs -- and retired in r05: LABNOTES.md, git history.)
// ------------------------------------------------------------------------------------------------
static int hidden_tmp_buffer(lia_ctx* ctx, size_t bytes, bf16_t** out) {
  if (ctx->hidden_tmp_bytes < bytes) {
    HIP_TRY(hipStreamSynchronize(ctx->compute));
    if (ctx->hidden_tmp) (void)hipFree(ctx->hidden_tmp);
    ctx->hidden_tmp = nullptr; ctx->hidden_tmp_bytes = 0;
    HIP_TRY(hipMalloc((void**)&ctx->hidden_tmp, bytes));
    ctx->hidden_tmp_bytes = bytes;
  }
  *out = (bf16_t*)ctx->hidden_tmp;
  return LIA_OK;
}

// hidden state h_l (the input of layer l; h_n = the result): h_0 = x, never written; h_n = y; in between y and the context's
// third buffer alternate so that a layer never writes the buffer it reads
static inline bf16_t* hidden_of(int l, int n, const bf16_t* x, bf16_t* y, bf16_t* t) { return l == 0 ? (bf16_t*)x : (((n - l) & 1) ? t : y); }

// Both runs: the argument checks (`who` names the entry point, nw = weight slots per layer, extra_ok = its own pointers are non-NULL)
// and the loop over the hidden buffers.  layer(W, next, x_l, y_l, kv_l): chain the next layer's first norm (next = its weights, or
// NULL behind the last layer) and run one T == 1 layer call.
template <typename LayerCall>
static int decode_layers_run(const char* who, lia_ctx* ctx, int H, int n_layers, int nw, const void* const* weights, const lia_bf16* x, lia_bf16* y,
                             lia_kv* const* kv, bool extra_ok, int B, int pos0, LayerCall layer) {
  if (n_layers <= 0 || !weights || !x || !y || !kv || !extra_ok) { lia_set_error("%s: NULL argument", who); return LIA_ERR_MISSING; }
  for (int l = 0; l < n_layers; ++l) {
    if (!kv[l] || !kv[l]->k || !kv[l]->v) { lia_set_error("%s: kv[%d] is NULL", who, l); return LIA_ERR_MISSING; }
    if (!kv[l]->on_device || B <= 0 || B > kv[l]->batch || pos0 < 0 || pos0 + 1 > kv[l]->smax) {
      lia_set_error("%s: B=%d pos0=%d vs cache %d batch=%d smax=%d on_device=%d", who, B, pos0, l, kv[l]->batch, kv[l]->smax, kv[l]->on_device);
      return LIA_ERR_INVALID;
    }
    for (int i = 0; i < nw; ++i)
      if (!weights[l * nw + i]) { lia_set_error("%s: weights[%d][%d] is NULL", who, l, i); return LIA_ERR_MISSING; }
  }
  const int M = B;
  bf16_t* tmp = nullptr;
  int rc = hidden_tmp_buffer(ctx, (size_t)M * H * 2, &tmp);
  if (rc) return rc;
  const bf16_t* const* Wall = (const bf16_t* const*)weights;
  for (int l = 0; l < n_layers; ++l) {
    rc = layer(Wall + l * nw, l + 1 < n_layers ? Wall + (l + 1) * nw : nullptr, hidden_of(l, n_layers, x, y, tmp), hidden_of(l + 1, n_layers, x, y, tmp), kv[l]);
    if (rc) return rc;
  }
  return LIA_OK;
}

extern "C" int lia_llama_decode_layers(lia_ctx* ctx, const lia_llama_desc* d, int n_layers, const void* const* weights, const lia_bf16* x,
                                       lia_bf16* y, lia_kv* const* kv, const lia_bf16* cos_table, const lia_bf16* sin_table, int B, int pos0,
                                       void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  int rc = check_llama_desc(d);
  if (rc) return rc;
  return decode_layers_run("lia_llama_decode_layers", ctx, d->hidden, n_layers, 9, weights, x, y, kv, cos_table && sin_table, B, pos0,
                           [&](const bf16_t* const* W, const bf16_t* const* next, const bf16_t* xl, bf16_t* yl, lia_kv* kvl) {
                             if (next) lia_ctx_chain_next_norm(ctx, next[0], nullptr);
                             return llama_layer_forward_impl(ctx, d, (const void* const*)W, xl, yl, kvl, cos_table, sin_table, B, 1, pos0, 0, stream, 0);
                           });
}

// the OPT counterpart: policy 3 (everything on the GPU, KV cache in HBM) for n_layers consecutive resident layers, T == 1 --
// the loop over resident layers of OPTDecoder.forward (lia/modeling_opt.py:1246-1260) with decoder.py:172-335 /
// attentions.py:393-529 per layer
extern "C" int lia_decode_layers(lia_ctx* ctx, const lia_layer_desc* d, int n_layers, const void* const* weights, const lia_bf16* x,
                                 lia_bf16* y, lia_kv* const* kv, int B, int pos0, void* stream) {
  if (!ctx) return LIA_ERR_INVALID;
  int rc = check_desc(d);
  if (rc) return rc;
  return decode_layers_run("lia_decode_layers", ctx, d->hidden, n_layers, 16, weights, x, y, kv, true, B, pos0,
                           [&](const bf16_t* const* W, const bf16_t* const* next, const bf16_t* xl, bf16_t* yl, lia_kv* kvl) {
                             if (next) lia_ctx_chain_next_norm(ctx, next[0], next[1]);
                             return layer_forward_impl(ctx, d, 3, (const void* const*)W, xl, yl, kvl, B, 1, pos0, 0, stream, 0);
                           });
}
