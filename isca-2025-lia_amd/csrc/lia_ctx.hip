// C ABI of liblia_hip.so (include/lia_hip.h), part 1: errors, the context (create / destroy / sync, options, key starts), live kernel
// timing (lia_prof_*) and K/V delivery to the host cache (lia_kv_deliver*).  No kernels here: see lia_internal.h for the launchers.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include "lia_internal.h"

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

extern "C" void lia_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* lia_last_error(void) { return g_err; }
extern "C" const char* lia_version(void) { return "lia_hip 0.1 (gfx950)"; }

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
extern "C" int lia_ctx_chain_next_norm(lia_ctx* c, const lia_bf16* g, const lia_bf16* b) {
  if (!c || !g) return LIA_ERR_INVALID;
  c->chain_g = g;
  c->chain_b = b;
  c->chain_armed = true;
  return LIA_OK;
}

extern "C" int lia_ctx_create(int device, size_t workspace_bytes, lia_ctx** out) {
  if (!out) return LIA_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) {
    lia_set_error("lia_ctx_create: device %d not present (%d devices)", device, n);
    return LIA_ERR_INVALID;
  }
  HIP_TRY(hipSetDevice(device));
  lia_ctx* c = new lia_ctx();
  memset(c, 0, sizeof(*c));
  c->device = device;
  HIP_TRY(hipStreamCreateWithFlags(&c->compute, hipStreamNonBlocking));
  {
    const char* ser = getenv("LIA_SERIALIZE");
    c->serialized = ser && ser[0] == '1';
  }
  if (c->serialized) {
    c->d2h = c->compute;
  } else {
    // K/V delivery must not starve behind back-to-back GEMMs when it falls back to a blit kernel (strided case)
    int lo = 0, hi = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIP_TRY(hipStreamCreateWithPriority(&c->d2h, hipStreamNonBlocking, hi));
  }
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(hipEventCreateWithFlags(&c->slab_ready[i], hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->slab_done[i], hipEventDisableTiming));
  }
  c->ws_bytes = c->ws_alloc_bytes = workspace_bytes;
  if (workspace_bytes) HIP_TRY(hipMalloc((void**)&c->ws, workspace_bytes));
  c->gemm_opts.fuse_combine = 1;
  *out = c;
  return LIA_OK;
}

extern "C" void lia_ctx_destroy(lia_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->compute);
  (void)hipStreamSynchronize(c->d2h);
  for (int i = 0; i < 2; ++i) {
    (void)hipEventDestroy(c->slab_ready[i]);
    (void)hipEventDestroy(c->slab_done[i]);
  }
  if (c->ws) (void)hipFree(c->ws);
  if (c->hidden_tmp) (void)hipFree(c->hidden_tmp);
  if (c->key_starts_dev) (void)hipFree(c->key_starts_dev);
  delete c->key_starts;
  if (c->row_lens_dev) (void)hipFree(c->row_lens_dev);
  delete c->row_lens;
  if (c->host_stage) (void)hipHostFree(c->host_stage);
  if (c->deliver_t0) { (void)hipEventDestroy(c->deliver_t0); (void)hipEventDestroy(c->deliver_t1); }
  if (c->deliver_events) {
    for (hipEvent_t e : *c->deliver_events) (void)hipEventDestroy(e);
    delete c->deliver_events;
    delete c->deliver_pending;
  }
  if (c->prof_events) {
    for (hipEvent_t e : *c->prof_events) (void)hipEventDestroy(e);
    delete c->prof_events;
    delete c->prof_recs;
  }
  if (c->d2h != c->compute) (void)hipStreamDestroy(c->d2h);
  (void)hipStreamDestroy(c->compute);
  delete c;
}

extern "C" size_t lia_ctx_workspace_bytes(lia_ctx* c) { return c ? c->ws_bytes : 0; }
extern "C" void* lia_ctx_workspace_ptr(lia_ctx* c) { return c ? (void*)c->ws : nullptr; }

int ctx_ws_lend(lia_ctx* c, const void* borrower, size_t keep, hipStream_t first_writer, hipEvent_t scratch_event) {
  if (c->ws_lent_to || !c->ws || keep >= c->ws_alloc_bytes || (keep & 255)) {
    lia_set_error("workspace lend: keep=%zu of %zu bytes (%s)", keep, c->ws_alloc_bytes, c->ws_lent_to ? "lent already" : "nothing to lend");
    return LIA_ERR_INVALID;
  }
  if (first_writer != c->compute) {
    HIP_TRY(hipEventRecord(scratch_event, c->compute));
    HIP_TRY(hipStreamWaitEvent(first_writer, scratch_event, 0));
  }
  // a K/V delivery of the prefill may still read a slab, which lies beyond any decode step's keep
  for (int i = 0; i < 2; ++i)
    if (c->slab_used[i]) HIP_TRY(hipStreamWaitEvent(first_writer, c->slab_done[i], 0));
  // a norm the previous layer call chained into a buffer that is about to be lent is gone
  if (c->normed_buf && (const char*)c->normed_buf >= c->ws + keep) ws_invalidate(c);
  c->ws_bytes = keep;
  c->ws_lent_to = borrower;
  return LIA_OK;
}

int ctx_ws_take_back(lia_ctx* c, const void* borrower, hipEvent_t idle) {
  if (c->ws_lent_to != borrower) return LIA_OK;
  HIP_TRY(hipStreamWaitEvent(c->compute, idle, 0));
  c->ws_bytes = c->ws_alloc_bytes;
  c->ws_lent_to = nullptr;
  return LIA_OK;
}

extern "C" void* lia_ctx_compute_stream(lia_ctx* c) { return c ? (void*)c->compute : nullptr; }
extern "C" int lia_ctx_serialized(lia_ctx* c) { return c && c->serialized ? 1 : 0; }

// hipStreamSynchronize spins on this image (one CPU of the container's CFS quota for as long as the GPU works); a blocking event
// instead (the thread sleeps, +20-50 us to wake) was measured in r03: less throttling, no gain per step (LABNOTES.md) -- spinning stays.
static int ctx_wait(hipStream_t st) {
  HIP_TRY(hipStreamSynchronize(st));
  return LIA_OK;
}

extern "C" int lia_ctx_synchronize(lia_ctx* c) {
  if (!c) return LIA_ERR_INVALID;
  if (int rc = ctx_wait(c->compute)) return rc;
  return ctx_wait(c->d2h);
}

extern "C" int lia_ctx_synchronize_compute(lia_ctx* c) {
  if (!c) return LIA_ERR_INVALID;
  return ctx_wait(c->compute);
}

// Per-context options and counters (r05: the A/B switches used to be process-wide setters -- lia_gemm_set_* -- although the
// library promises that two contexts of one process are independent, include/lia_hip.h).
extern "C" int lia_ctx_set_key_starts(lia_ctx* c, const int32_t* starts, int n_rows) {
  if (!c || n_rows < 0) return LIA_ERR_INVALID;
  if (!starts || n_rows == 0) { c->key_starts_n = 0; return LIA_OK; }
  for (int b = 0; b < n_rows; ++b)
    if (starts[b] < 0) { lia_set_error("lia_ctx_set_key_starts: starts[%d] = %d < 0", b, starts[b]); return LIA_ERR_INVALID; }
  // launches queued earlier may still read the device table: let them finish before it is replaced or overwritten
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->compute));
  if (c->key_starts_cap < n_rows) {
    if (c->key_starts_dev) (void)hipFree(c->key_starts_dev);
    c->key_starts_dev = nullptr; c->key_starts_cap = 0; c->key_starts_n = 0;
    HIP_TRY(hipMalloc((void**)&c->key_starts_dev, (size_t)n_rows * sizeof(int)));
    c->key_starts_cap = n_rows;
  }
  if (!c->key_starts) c->key_starts = new std::vector<int>();
  c->key_starts->assign(starts, starts + n_rows);
  HIP_TRY(hipMemcpyAsync(c->key_starts_dev, c->key_starts->data(), (size_t)n_rows * sizeof(int), hipMemcpyHostToDevice, c->compute));
  HIP_TRY(hipStreamSynchronize(c->compute));
  c->key_starts_n = n_rows;
  return LIA_OK;
}

// the ragged cache's per-row lengths: lia_ctx_set_key_starts' discipline -- a host copy the layer calls validate against, a device
// copy that is replaced only after the compute stream has drained
extern "C" int lia_ctx_set_row_lens(lia_ctx* c, const int32_t* lens, int n_rows) {
  if (!c || n_rows < 0) return LIA_ERR_INVALID;
  if (!lens || n_rows == 0) { c->row_lens_n = 0; return LIA_OK; }
  for (int b = 0; b < n_rows; ++b)
    if (lens[b] < 1) { lia_set_error("lia_ctx_set_row_lens: lens[%d] = %d < 1 (a ragged block is appended behind a prefill)", b, lens[b]); return LIA_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->compute));
  if (c->row_lens_cap < n_rows) {
    if (c->row_lens_dev) (void)hipFree(c->row_lens_dev);
    c->row_lens_dev = nullptr; c->row_lens_cap = 0; c->row_lens_n = 0;
    HIP_TRY(hipMalloc((void**)&c->row_lens_dev, (size_t)n_rows * sizeof(int)));
    c->row_lens_cap = n_rows;
  }
  if (!c->row_lens) c->row_lens = new std::vector<int>();
  c->row_lens->assign(lens, lens + n_rows);
  HIP_TRY(hipMemcpyAsync(c->row_lens_dev, c->row_lens->data(), (size_t)n_rows * sizeof(int), hipMemcpyHostToDevice, c->compute));
  HIP_TRY(hipStreamSynchronize(c->compute));
  c->row_lens_n = n_rows;
  return LIA_OK;
}

// the allowed-token table of the head calls: the pointer only -- nothing is copied, nothing waits (the caller keeps the memory alive
// and unchanged until the compute stream has passed the head call that reads it)
extern "C" int lia_ctx_set_token_mask(lia_ctx* c, const int32_t* mask_device, long ldm_words, int rows) {
  if (!c) return LIA_ERR_INVALID;
  if (!mask_device || rows == 0) { c->mods.mask = LiaTokenMask{}; return LIA_OK; }
  if (rows < 0 || ldm_words < 0) { lia_set_error("lia_ctx_set_token_mask: rows=%d ldm=%ld must be >= 0", rows, ldm_words); return LIA_ERR_INVALID; }
  if ((uintptr_t)mask_device & 3) { lia_set_error("lia_ctx_set_token_mask: mask=%p is not 4-byte aligned", (const void*)mask_device); return LIA_ERR_INVALID; }
  c->mods.mask = LiaTokenMask{(const uint32_t*)mask_device, ldm_words, rows};
  return LIA_OK;
}

// the log-probability sink of the head calls: the pointers only, as the token mask -- nothing is copied, nothing waits
extern "C" int lia_ctx_set_logprob_sink(lia_ctx* c, int n_top, float* chosen, int64_t* top_ids, float* top_logprobs, long rows) {
  if (!c) return LIA_ERR_INVALID;
  if (!chosen) { c->mods.sink = LiaSink{}; return LIA_OK; }
  if (n_top < 0 || n_top > LIA_LOGPROB_MAX_TOP) {
    lia_set_error("lia_ctx_set_logprob_sink: n_top=%d must be in [0, %d]", n_top, LIA_LOGPROB_MAX_TOP);
    return LIA_ERR_INVALID;
  }
  if (rows < 1) { lia_set_error("lia_ctx_set_logprob_sink: rows=%ld must be >= 1", rows); return LIA_ERR_INVALID; }
  if (n_top > 0 && (!top_ids || !top_logprobs)) {
    lia_set_error("lia_ctx_set_logprob_sink: NULL %s with n_top=%d (NULL only with n_top = 0)", !top_ids ? "top_ids" : "top_logprobs", n_top);
    return LIA_ERR_INVALID;
  }
  c->mods.sink = LiaSink{chosen, top_ids, top_logprobs, n_top, rows};
  return LIA_OK;
}

// the penalties of the head calls: the pointers only, as the token mask -- the caller owns the count table and the scratch of
// rows x lds bf16 values, and keeps both alive until the compute stream has passed the head call.  The pitches are checked against
// the vocabulary where it is known, at the head call.
extern "C" int lia_ctx_set_penalties(lia_ctx* c, const uint16_t* counts, long ldc, int rows, float repetition, float presence,
                                     float frequency, lia_bf16* scratch, long lds) {
  if (!c) return LIA_ERR_INVALID;
  if (!counts) { c->mods.penalties = LiaPenalties{}; return LIA_OK; }
  if (penalty_args_invalid("lia_ctx_set_penalties", repetition, presence, frequency, counts, ldc, -1)) return LIA_ERR_INVALID;
  if (rows <= 0) { lia_set_error("lia_ctx_set_penalties: rows=%d must be >= 1", rows); return LIA_ERR_INVALID; }
  if (!scratch) { lia_set_error("lia_ctx_set_penalties: NULL scratch with a count table (rows x lds bf16 values, the caller's)"); return LIA_ERR_INVALID; }
  if (lds <= 0) { lia_set_error("lia_ctx_set_penalties: lds=%ld must be >= the vocabulary", lds); return LIA_ERR_INVALID; }
  c->mods.penalties = LiaPenalties{counts, ldc, rows, repetition, presence, frequency, (bf16_t*)scratch, lds};
  return LIA_OK;
}

extern "C" int lia_ctx_set_option(lia_ctx* c, int key, long value) {
  if (!c) return LIA_ERR_INVALID;
  switch (key) {
    case LIA_OPT_FUSE_COMBINE: c->gemm_opts.fuse_combine = value ? 1 : 0; return LIA_OK;
    case LIA_OPT_BLOCK_ATTENTION: c->attn_opts.block_attention = value ? 1 : 0; return LIA_OK;
    case LIA_OPT_SPLIT_DECODE: c->attn_opts.split_decode = value ? 1 : 0; return LIA_OK;
    default: lia_set_error("lia_ctx_set_option: unknown key %d", key); return LIA_ERR_INVALID;
  }
}
extern "C" long lia_ctx_get_counter(lia_ctx* c, int key) {
  if (!c) return -1;
  if (key > LIA_CNT_FUSED_COMBINE && key <= LIA_CNT_FUSED_COMBINE + 4) return c->gemm_opts.fused_combines[key - LIA_CNT_FUSED_COMBINE];
  if (key == LIA_CNT_BLOCK_ATTENTION) return c->attn_opts.block_launches;
  if (key == LIA_CNT_SPLIT_DECODE) return c->attn_opts.split_launches;
  return -1;
}

extern "C" int lia_ctx_set_host_threads(lia_ctx* c, int n) {
  if (!c || n < 0) return LIA_ERR_INVALID;
  c->host_threads = n;
  return LIA_OK;
}

extern "C" int lia_prof_start(lia_ctx* c, int max_launches) {
  if (!c || max_launches <= 0) return LIA_ERR_INVALID;
  if (!c->prof_events) { c->prof_events = new std::vector<hipEvent_t>(); c->prof_recs = new std::vector<lia_ctx::ProfRec>(); }
  while (c->prof_events->size() < (size_t)2 * max_launches) {
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    c->prof_events->push_back(e);
  }
  c->prof_recs->clear();
  c->prof_host_attn_calls = 0;
  c->prof_host_attn_ms = 0.0;
  c->prof_cap = max_launches;
  c->prof_seen = 0;
  if (c->prof_stride < 1) c->prof_stride = 1;
  c->prof_on = true;
  return LIA_OK;
}

extern "C" int lia_prof_set_stride(lia_ctx* c, int stride) {
  if (!c || stride < 1) return LIA_ERR_INVALID;
  c->prof_stride = stride;
  return LIA_OK;
}

extern "C" int lia_prof_stop(lia_ctx* c, lia_prof_result* out) {
  if (!c || !out || !c->prof_events) return LIA_ERR_INVALID;
  c->prof_on = false;
  memset(out, 0, sizeof(*out));
  out->host_attention_calls = c->prof_host_attn_calls;
  out->host_attention_ms = c->prof_host_attn_ms;
  HIP_TRY(hipStreamSynchronize(c->compute));
  for (size_t i = 0; i < c->prof_recs->size(); ++i) {
    float ms = 0.f;
    HIP_TRY(hipEventSynchronize((*c->prof_events)[2 * i + 1]));
    HIP_TRY(hipEventElapsedTime(&ms, (*c->prof_events)[2 * i], (*c->prof_events)[2 * i + 1]));
    const auto& r = (*c->prof_recs)[i];
    if (r.regime == 1) { out->skinny_launches++; out->skinny_ms += ms; out->skinny_bytes += r.bytes; out->skinny_flops += r.flops; }
    else { out->tiled_launches++; out->tiled_ms += ms; out->tiled_bytes += r.bytes; out->tiled_flops += r.flops; }
  }
  // calibrate the bracket: 32 empty event pairs on the same stream (rocprofv3's kernel durations carry no such term)
  if (c->prof_events->size() >= 2) {
    double sum = 0.0;
    const int reps = 32;
    for (int i = 0; i < reps; ++i) {
      HIP_TRY(hipEventRecord((*c->prof_events)[0], c->compute));
      HIP_TRY(hipEventRecord((*c->prof_events)[1], c->compute));
      HIP_TRY(hipEventSynchronize((*c->prof_events)[1]));
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, (*c->prof_events)[0], (*c->prof_events)[1]));
      sum += ms;
    }
    out->empty_bracket_ms = sum / reps;
  }
  return LIA_OK;
}

extern "C" int lia_ctx_kv_store_wait(lia_ctx* c) {
  if (!c) return LIA_ERR_INVALID;
  HIP_TRY(hipStreamSynchronize(c->d2h));
  return LIA_OK;
}

extern "C" int lia_kv_deliver(lia_ctx* c, const lia_kv* dev, lia_kv* host, int T, int row_elems, int* ticket) {
  if (!c || !dev || !host || !ticket) return LIA_ERR_INVALID;
  if (!dev->k || !dev->v || !host->k || !host->v) { lia_set_error("lia_kv_deliver: NULL cache"); return LIA_ERR_MISSING; }
  if (!dev->on_device || host->on_device || dev->batch != host->batch || T <= 0 || T > dev->smax || T > host->smax || row_elems <= 0) {
    lia_set_error("lia_kv_deliver: dev(on_device=%d batch=%d smax=%d) host(on_device=%d batch=%d smax=%d) T=%d", dev->on_device, dev->batch,
                  dev->smax, host->on_device, host->batch, host->smax, T);
    return LIA_ERR_INVALID;
  }
  if (!c->deliver_events) { c->deliver_events = new std::vector<hipEvent_t>(); c->deliver_pending = new std::vector<char>(); }
  // A ticket is freed by lia_kv_deliver_wait and by nothing else: recycling one whose copy merely happened to be complete
  // (r02) handed the same id to a later layer of the SAME prefill, and waiting for layer i then meant waiting for layer j > i.
  int id = -1;
  for (size_t i = 0; i < c->deliver_pending->size(); ++i)
    if (!(*c->deliver_pending)[i]) { id = (int)i; break; }
  if (id < 0) {
    hipEvent_t e;
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->deliver_events->push_back(e);
    c->deliver_pending->push_back(0);
    id = (int)c->deliver_events->size() - 1;
  }
  // behind the compute stream's work so far (the layer that filled the holding cache), on the K/V delivery stream
  HIP_TRY(hipEventRecord((*c->deliver_events)[id], c->compute));
  HIP_TRY(hipStreamWaitEvent(c->d2h, (*c->deliver_events)[id], 0));
  if (!c->deliver_t0) { HIP_TRY(hipEventCreate(&c->deliver_t0)); HIP_TRY(hipEventCreate(&c->deliver_t1)); }
  if (!c->deliver_batch_open) { HIP_TRY(hipEventRecord(c->deliver_t0, c->d2h)); c->deliver_batch_open = true; }
  // the strided 2-D form even though the rows are contiguous: the runtime serves it with a blit kernel, a linear copy would
  // queue on the SDMA engine behind the next step's weight copies (see the policy-0 delivery in lia_layer_forward)
  const size_t width = (size_t)dev->batch * row_elems * 2;
  HIP_TRY(hipMemcpy2DAsync(host->k, width, dev->k, width, width, T, hipMemcpyDeviceToHost, c->d2h));
  HIP_TRY(hipMemcpy2DAsync(host->v, width, dev->v, width, width, T, hipMemcpyDeviceToHost, c->d2h));
  HIP_TRY(hipEventRecord((*c->deliver_events)[id], c->d2h));
  HIP_TRY(hipEventRecord(c->deliver_t1, c->d2h));
  (*c->deliver_pending)[id] = 1;
  *ticket = id;
  return LIA_OK;
}

// Device time of the deliveries issued since the last call of this function (first copy's start to last copy's end on the K/V
// delivery stream); blocks until the last one has landed.  For the benchmark's prefill accounting.
extern "C" int lia_kv_deliver_batch_ms(lia_ctx* c, double* ms) {
  if (!c || !ms) return LIA_ERR_INVALID;
  *ms = 0.0;
  if (!c->deliver_batch_open) return LIA_OK;
  HIP_TRY(hipEventSynchronize(c->deliver_t1));
  float f = 0.f;
  HIP_TRY(hipEventElapsedTime(&f, c->deliver_t0, c->deliver_t1));
  *ms = f;
  c->deliver_batch_open = false;
  return LIA_OK;
}

extern "C" int lia_kv_deliver_wait(lia_ctx* c, int ticket) {
  if (!c || !c->deliver_events || ticket < 0 || ticket >= (int)c->deliver_events->size()) { lia_set_error("lia_kv_deliver_wait: ticket %d", ticket); return LIA_ERR_INVALID; }
  if (!(*c->deliver_pending)[ticket]) return LIA_OK;
  HIP_TRY(hipEventSynchronize((*c->deliver_events)[ticket]));
  (*c->deliver_pending)[ticket] = 0;
  return LIA_OK;
}
