// C ABI of liblia_hip.so (include/lia_hip.h), part 4: the weight streamer, lia_pack_decode, pinned / registered host memory, lia_blit and
// lia_memcpy_*.  No kernels here: see lia_internal.h for the launchers.
#include <algorithm>

#include "lia_internal.h"

// ------------------------------------------------------------------------------------------------
// weight streamer
// ------------------------------------------------------------------------------------------------
// the decode of one codec of the pack10 family (format: LIA_WIRE_PACK10 | LIA_WIRE_PACK10A, checked by the callers)
static void wire_decode_launch(int format, const char* src, bf16_t* dst, size_t n_values, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
  if (format == LIA_WIRE_PACK10A) lia_pack10a_decode_launch(src, dst, n_values, st, ev0, ev1);
  else lia_packed_decode_launch(src, dst, n_values, st, ev0, ev1);
}
static inline bool wire_format_known(int format) { return format == LIA_WIRE_PACK10 || format == LIA_WIRE_PACK10A; }

struct lia_streamer {
  lia_ctx* ctx;
  int n_slots;
  size_t slot_bytes;
  char* slots;
  char* staging;          // per-slot landing area of pack10-encoded layers (lazily allocated)
  size_t staging_bytes;
  hipStream_t decode;     // the wire-format decode kernels run here, ordered after the slot's copy by an event
  std::vector<hipEvent_t> landed;
  std::vector<char> decoded_on_side;
  // live timing of the wire-format decode kernel (lia_stream_decode_stats): one event pair per slot around the MAIN decode kernel
  std::vector<hipEvent_t> d0, d1;
  std::vector<char> decode_pending;
  std::vector<double> decode_in, decode_out;      // bytes of the pending launch: encoded layer read, bf16 layer written
  double dec_ms, dec_in, dec_out;
  long dec_launches;
  hipStream_t copy;
  std::vector<hipEvent_t> copied, released, t0, t1;
  std::vector<char> has_release, timing_pending, was_marked;
  std::vector<size_t> pending_bytes;
  // pageable sources (the reference's un-pinned numa_alloc tensors, a layer kept without --pin-weight) are staged through two pinned
  // bounce buffers of LIA_BOUNCE_BYTES: a team memcpy fills one while the copy engine drains the other (staged_copy)
  char* bounce[2];
  hipEvent_t bounce_done[2];
  int bounce_next;
  double bytes, busy_ms;
  // wire cache (lia_stream_cache_*, decode mode): while keep_slots != 0 a pool of geo.n_entries wire-format layers lies where
  // lia_cache_geometry_plan_extra put it -- the slots from keep_slots on, the staging allocation behind the keep_slots landing buffers
  // (which no longer belong to a slot), when configured the tail of the context's workspace, and the extra allocation
  int keep_slots;
  lia_cache_geometry geo;              // of the mode that is on (zeroed while it is off)
  // lia_stream_cache_configure: sticky, all zero = whole staging areas as landing buffers and no workspace entries
  size_t cfg_landing_bytes, cfg_keep_bytes;
  int cfg_lend;
  bool lent;                           // this mode holds the context's workspace tail
  char* extra;                         // lia_stream_cache_extra: a fourth region, owned by the streamer (NULL: none)
  size_t extra_bytes;
  hipEvent_t ws_fence;                 // on the compute stream when the workspace is lent
  std::vector<char> entry_filled;
  std::vector<const void*> entry_src;
  std::vector<size_t> entry_bytes;
  std::vector<hipEvent_t> drained;     // per landing buffer, on the decode stream: the decode that last read it has finished
  std::vector<char> has_drained;
  std::vector<size_t> landing_bytes;
  hipEvent_t cache_idle;               // on the decode stream when the mode ends: no decode reads an entry or a landing buffer any more
  // copy timing of the mode: its copies belong to no slot, so their event pairs come from a ring
  std::vector<hipEvent_t> r0, r1;
  std::vector<char> ring_pending;
  std::vector<size_t> ring_bytes;
  int ring_next;
};

constexpr int LIA_CACHE_TIMING_RING = 16;
// The decode kernels read a little past the bytes shipped: 16 bytes of stream padding for a consistent encoding, at most
// (1024 codes) / 2 + 8 bytes behind the level-3 stream whatever the planes hold once the validator passed the tables
// (lia_pack10_validate), 2 bytes behind pack10a's words.  Every entry, and every landing buffer sized by
// lia_stream_cache_configure, keeps LIA_CACHE_READ_SLACK (lia_hip.h) bytes of room behind its layer.

static void streamer_collect_decode(lia_streamer* s, int slot, bool wait) {
  if (s->decode_pending.empty() || !s->decode_pending[slot]) return;
  if (!wait && hipEventQuery(s->d1[slot]) != hipSuccess) return;
  if (hipEventSynchronize(s->d1[slot]) == hipSuccess) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s->d0[slot], s->d1[slot]) == hipSuccess) {
      s->dec_ms += ms; s->dec_in += s->decode_in[slot]; s->dec_out += s->decode_out[slot]; s->dec_launches++;
    }
  }
  s->decode_pending[slot] = 0;
}

static void streamer_collect(lia_streamer* s, int slot) {
  if (!s->timing_pending[slot]) return;
  if (hipEventSynchronize(s->t1[slot]) == hipSuccess) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s->t0[slot], s->t1[slot]) == hipSuccess) {
      s->busy_ms += ms;
      s->bytes += (double)s->pending_bytes[slot];
    }
  }
  s->timing_pending[slot] = 0;
}

// the same for record r of the decode mode's timing ring; wait = false: only if the copy has finished
static void streamer_collect_ring(lia_streamer* s, int r, bool wait) {
  if (!s->ring_pending[r]) return;
  if (!wait && hipEventQuery(s->r1[r]) != hipSuccess) return;
  if (hipEventSynchronize(s->r1[r]) == hipSuccess) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s->r0[r], s->r1[r]) == hipSuccess) {
      s->busy_ms += ms;
      s->bytes += (double)s->ring_bytes[r];
    }
  }
  s->ring_pending[r] = 0;
}

extern "C" int lia_stream_create(lia_ctx* ctx, int n_slots, size_t slot_bytes, lia_streamer** out) {
  if (!ctx || !out || n_slots < 1 || n_slots > 16 || slot_bytes == 0) { lia_set_error("lia_stream_create: n_slots=%d slot_bytes=%zu", n_slots, slot_bytes); return LIA_ERR_INVALID; }
  *out = nullptr;
  lia_streamer* s = new lia_streamer();
  s->ctx = ctx; s->n_slots = n_slots; s->slot_bytes = align_up(slot_bytes, 256);
  s->bounce[0] = s->bounce[1] = nullptr; s->bounce_done[0] = s->bounce_done[1] = nullptr; s->bounce_next = 0;
  s->bytes = 0; s->busy_ms = 0; s->slots = nullptr; s->staging = nullptr; s->staging_bytes = 0;
  s->dec_ms = s->dec_in = s->dec_out = 0; s->dec_launches = 0;
  s->keep_slots = 0; memset(&s->geo, 0, sizeof(s->geo)); s->cache_idle = nullptr; s->ring_next = 0;
  s->cfg_landing_bytes = s->cfg_keep_bytes = 0; s->cfg_lend = 0; s->lent = false; s->ws_fence = nullptr;
  s->extra = nullptr; s->extra_bytes = 0;
  HIP_TRY(hipMalloc((void**)&s->slots, s->slot_bytes * n_slots));
  if (ctx->serialized) s->copy = ctx->compute;
  else HIP_TRY(hipStreamCreateWithFlags(&s->copy, hipStreamNonBlocking));
  s->copied.resize(n_slots); s->released.resize(n_slots); s->t0.resize(n_slots); s->t1.resize(n_slots);
  s->has_release.assign(n_slots, 0); s->timing_pending.assign(n_slots, 0); s->pending_bytes.assign(n_slots, 0);
  s->was_marked.assign(n_slots, 0);
  for (int i = 0; i < n_slots; ++i) {
    HIP_TRY(hipEventCreateWithFlags(&s->copied[i], hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&s->released[i], hipEventDisableTiming));
    HIP_TRY(hipEventCreate(&s->t0[i]));
    HIP_TRY(hipEventCreate(&s->t1[i]));
  }
  *out = s;
  return LIA_OK;
}

extern "C" void lia_stream_destroy(lia_streamer* s) {
  if (!s) return;
  (void)lia_stream_cache_disable(s);     // (the context gets its workspace back)
  (void)hipStreamSynchronize(s->copy);
  for (int i = 0; i < s->n_slots; ++i) {
    (void)hipEventDestroy(s->copied[i]); (void)hipEventDestroy(s->released[i]);
    (void)hipEventDestroy(s->t0[i]); (void)hipEventDestroy(s->t1[i]);
  }
  for (int i = 0; i < 2; ++i) {
    if (s->bounce[i]) (void)hipHostFree(s->bounce[i]);
    if (s->bounce_done[i]) (void)hipEventDestroy(s->bounce_done[i]);
  }
  if (s->slots) (void)hipFree(s->slots);
  if (s->staging) {
    (void)hipStreamSynchronize(s->decode);
    for (hipEvent_t e : s->landed) (void)hipEventDestroy(e);
    for (hipEvent_t e : s->d0) (void)hipEventDestroy(e);
    for (hipEvent_t e : s->d1) (void)hipEventDestroy(e);
    for (hipEvent_t e : s->drained) (void)hipEventDestroy(e);
    for (hipEvent_t e : s->r0) (void)hipEventDestroy(e);
    for (hipEvent_t e : s->r1) (void)hipEventDestroy(e);
    if (s->cache_idle) (void)hipEventDestroy(s->cache_idle);
    if (s->ws_fence) (void)hipEventDestroy(s->ws_fence);
    if (s->decode != s->ctx->compute) (void)hipStreamDestroy(s->decode);
    (void)hipFree(s->staging);
  }
  if (s->extra) (void)hipFree(s->extra);
  if (s->copy != s->ctx->compute) (void)hipStreamDestroy(s->copy);
  delete s;
}

extern "C" void* lia_stream_slot_ptr(lia_streamer* s, int slot) {
  if (!s || slot < 0 || slot >= s->n_slots) return nullptr;
  return s->slots + (size_t)slot * s->slot_bytes;
}

extern "C" void* lia_stream_copy_stream(lia_streamer* s) { return s ? (void*)s->copy : nullptr; }

// prefetch = begin + copy_chunk(whole layer) + mark_ready.  The three-step form lets a data-parallel caller
// interleave RCCL broadcasts of the chunks (on streams ordered after the copy stream) before the slot is
// declared ready.
extern "C" int lia_stream_begin(lia_streamer* s, int slot) {
  if (!s || slot < 0 || slot >= s->n_slots) { lia_set_error("lia_stream_begin: slot=%d", slot); return LIA_ERR_INVALID; }
  if (s->keep_slots && slot >= s->keep_slots) { lia_set_error("lia_stream_begin: slot %d holds cached layers (decode mode keeps %d slots)", slot, s->keep_slots); return LIA_ERR_INVALID; }
  streamer_collect(s, slot);
  if (s->has_release[slot]) HIP_TRY(hipStreamWaitEvent(s->copy, s->released[slot], 0));
  // A prefetch the caller dropped (never waited for, never released) may still have its decode kernel running on the side
  // stream, reading this slot's staging area and writing the slot: the new copy must land behind it as well.
  if (s->was_marked[slot]) HIP_TRY(hipStreamWaitEvent(s->copy, s->copied[slot], 0));
  HIP_TRY(hipEventRecord(s->t0[slot], s->copy));
  s->pending_bytes[slot] = 0;
  return LIA_OK;
}

// Pageable source -> device through the two pinned bounce buffers (the reference's cpu_buff, modeling_opt.py:1219-1220, and what
// `copy_(non_blocking=True)` from its un-pinned numa_alloc tensors does inside torch).  r01-r04: one slot-sized bounce buffer, a
// single-threaded memcpy behind a stream synchronize -- 16.6 GB/s in the H2D microbenchmark twin where torch's own staging reaches
// 51.  Now 64 MiB pieces, a team memcpy (lia_host_parallel_memcpy, the context's host threads) into one buffer while the copy engine
// drains the other; the host thread waits only for the buffer it is about to overwrite.
constexpr size_t LIA_BOUNCE_BYTES = (size_t)64 << 20;
static int staged_copy(lia_streamer* s, char* dst_device, const void* host_ptr, size_t bytes) {
  for (int i = 0; i < 2; ++i)
    if (!s->bounce[i]) {
      HIP_TRY(hipHostMalloc((void**)&s->bounce[i], LIA_BOUNCE_BYTES, hipHostMallocDefault));
      HIP_TRY(hipEventCreateWithFlags(&s->bounce_done[i], hipEventDisableTiming));
      HIP_TRY(hipEventRecord(s->bounce_done[i], s->copy));
    }
  for (size_t off = 0; off < bytes; off += LIA_BOUNCE_BYTES) {
    const size_t n = std::min(LIA_BOUNCE_BYTES, bytes - off);
    const int b = s->bounce_next;
    s->bounce_next ^= 1;
    HIP_TRY(hipEventSynchronize(s->bounce_done[b]));                 // the DMA that last read this buffer has finished
    lia_host_parallel_memcpy(s->bounce[b], (const char*)host_ptr + off, n, s->ctx->host_threads);
    HIP_TRY(hipMemcpyAsync(dst_device + off, s->bounce[b], n, hipMemcpyHostToDevice, s->copy));
    HIP_TRY(hipEventRecord(s->bounce_done[b], s->copy));
  }
  return LIA_OK;
}

// one chunk into the slot's part of an area of `capacity` bytes per slot (the slots themselves, or the staging areas); checked by the callers
static int copy_chunk_to(lia_streamer* s, char* dst_base, size_t capacity, int slot, size_t offset, const void* host_ptr, size_t bytes, int pinned) {
  char* const dst = dst_base + (size_t)slot * capacity + offset;
  if (pinned) HIP_TRY(hipMemcpyAsync(dst, host_ptr, bytes, hipMemcpyHostToDevice, s->copy));
  else if (int rc = staged_copy(s, dst, host_ptr, bytes)) return rc;
  s->pending_bytes[slot] += bytes;
  return LIA_OK;
}

extern "C" int lia_stream_copy_chunk(lia_streamer* s, int slot, size_t offset, const void* host_ptr, size_t bytes, int pinned) {
  if (!s || slot < 0 || slot >= s->n_slots || !host_ptr || offset + bytes > s->slot_bytes) {
    lia_set_error("lia_stream_copy_chunk: slot=%d offset=%zu bytes=%zu (slot holds %zu)", slot, offset, bytes, s ? s->slot_bytes : 0);
    return LIA_ERR_INVALID;
  }
  return copy_chunk_to(s, s->slots, s->slot_bytes, slot, offset, host_ptr, bytes, pinned);
}

// packed path: the encoded layer lands in the slot's staging area, then a kernel on a side stream rebuilds the
// bf16 layer in the slot itself (lia_pack10.hip).  begin -> copy_chunk_packed* -> decode_packed -> mark_ready.
static int ensure_staging(lia_streamer* s) {
  if (s->staging) return LIA_OK;
  s->staging_bytes = lia_pack10_bound((s->slot_bytes / 2 + 1023) / 1024 * 1024);
  HIP_TRY(hipMalloc((void**)&s->staging, s->staging_bytes * s->n_slots));
  // The wire-format decode runs on a stream of its own, ordered by events, so the copy engine moves on to the next layer at once.
  // (r02-r04 could confine that stream to a few compute units with a CU mask: measured level or worse at every width -- k masked CUs
  // for 256 / k times as long cost the prefill GEMM the same CU-milliseconds -- and removed in r05; what did pay was making the
  // decode kernel itself cheaper, lia_pack10.hip.  LABNOTES.md r04 / r05.)
  if (s->ctx->serialized) s->decode = s->ctx->compute;
  else HIP_TRY(hipStreamCreateWithFlags(&s->decode, hipStreamNonBlocking));
  s->landed.resize(s->n_slots);
  s->decoded_on_side.assign(s->n_slots, 0);
  s->d0.resize(s->n_slots); s->d1.resize(s->n_slots);
  s->decode_pending.assign(s->n_slots, 0); s->decode_in.assign(s->n_slots, 0.0); s->decode_out.assign(s->n_slots, 0.0);
  for (int i = 0; i < s->n_slots; ++i) {
    HIP_TRY(hipEventCreateWithFlags(&s->landed[i], hipEventDisableTiming));
    HIP_TRY(hipEventCreate(&s->d0[i]));
    HIP_TRY(hipEventCreate(&s->d1[i]));
  }
  // everything the decode mode needs, so that turning it on or off allocates nothing
  s->drained.resize(s->n_slots);
  s->has_drained.assign(s->n_slots, 0); s->landing_bytes.assign(s->n_slots, 0);
  for (int i = 0; i < s->n_slots; ++i) HIP_TRY(hipEventCreateWithFlags(&s->drained[i], hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&s->cache_idle, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&s->ws_fence, hipEventDisableTiming));
  s->r0.resize(LIA_CACHE_TIMING_RING); s->r1.resize(LIA_CACHE_TIMING_RING);
  s->ring_pending.assign(LIA_CACHE_TIMING_RING, 0); s->ring_bytes.assign(LIA_CACHE_TIMING_RING, 0);
  for (int i = 0; i < LIA_CACHE_TIMING_RING; ++i) {
    HIP_TRY(hipEventCreate(&s->r0[i]));
    HIP_TRY(hipEventCreate(&s->r1[i]));
  }
  s->entry_filled.assign(LIA_CACHE_MAX_ENTRIES, 0); s->entry_src.assign(LIA_CACHE_MAX_ENTRIES, nullptr); s->entry_bytes.assign(LIA_CACHE_MAX_ENTRIES, 0);
  return LIA_OK;
}

extern "C" void* lia_stream_staging_ptr(lia_streamer* s, int slot) {
  if (!s || slot < 0 || slot >= s->n_slots || ensure_staging(s)) return nullptr;
  return s->staging + (size_t)slot * s->staging_bytes;
}

extern "C" int lia_stream_copy_chunk_packed(lia_streamer* s, int slot, size_t offset, const void* host_ptr, size_t bytes, int pinned) {
  if (!s || slot < 0 || slot >= s->n_slots || !host_ptr) return LIA_ERR_INVALID;
  if (s->keep_slots) { lia_set_error("lia_stream_copy_chunk_packed: the staging areas are landing buffers in decode mode (lia_stream_land)"); return LIA_ERR_INVALID; }
  int rc = ensure_staging(s);
  if (rc) return rc;
  if (offset + bytes > s->staging_bytes) { lia_set_error("lia_stream_copy_chunk_packed: %zu + %zu > staging %zu", offset, bytes, s->staging_bytes); return LIA_ERR_INVALID; }
  return copy_chunk_to(s, s->staging, s->staging_bytes, slot, offset, host_ptr, bytes, pinned);
}

// The decode kernel of one layer on the decode stream, src -> slot, inside the slot's timing bracket.  The bracket re-uses the
// slot's event pair: collect the previous launch first -- WITHOUT waiting (this runs inside the token loop).  The slot's previous
// decode finished long ago (its consumer released the slot); should it not have -- a dropped prefetch whose decode is still in
// flight -- this launch simply goes untimed.
static int launch_decode(lia_streamer* s, const char* src, int slot, size_t n_values, int format, double bytes_in) {
  streamer_collect_decode(s, slot, false);
  (void)hipGetLastError();                                             // hipErrorNotReady from the query is an answer, not an error
  const bool timed = !s->decode_pending[slot];
  wire_decode_launch(format, src, (bf16_t*)(s->slots + (size_t)slot * s->slot_bytes), n_values, s->decode, timed ? s->d0[slot] : nullptr,
                     timed ? s->d1[slot] : nullptr);
  HIP_TRY(hipGetLastError());
  if (timed) {
    s->decode_in[slot] = bytes_in;
    s->decode_out[slot] = 2.0 * (double)n_values;
    s->decode_pending[slot] = 1;
  }
  return LIA_OK;
}

extern "C" int lia_stream_decode_packed(lia_streamer* s, int slot, size_t n_values, int format) {
  if (!s || slot < 0 || slot >= s->n_slots || !s->staging || s->keep_slots || n_values * 2 > s->slot_bytes || !wire_format_known(format) || (n_values % 1024)) {
    lia_set_error("lia_stream_decode_packed: slot=%d n_values=%zu format=%d", slot, n_values, format);
    return LIA_ERR_INVALID;
  }
  // The decode runs on its own stream behind an event, so the copy engine moves on to the next layer at once.
  // It must not start before the slot's previous consumer released it: begin() made the COPY stream wait for that,
  // and `landed` is recorded on the copy stream after the copy, so the order is inherited.
  HIP_TRY(hipEventRecord(s->t1[slot], s->copy));                       // copy-engine busy time ends here
  HIP_TRY(hipEventRecord(s->landed[slot], s->copy));
  HIP_TRY(hipStreamWaitEvent(s->decode, s->landed[slot], 0));
  if (int rc = launch_decode(s, s->staging + (size_t)slot * s->staging_bytes, slot, n_values, format, (double)s->pending_bytes[slot])) return rc;
  s->decoded_on_side[slot] = 1;
  return LIA_OK;
}

extern "C" int lia_pack_decode(const char* src_device, lia_bf16* dst_device, size_t n_values, int format, void* stream) {
  if (!src_device || !dst_device) { lia_set_error("lia_pack_decode: NULL buffer"); return LIA_ERR_MISSING; }
  if (!wire_format_known(format) || (n_values % 1024)) {
    lia_set_error("lia_pack_decode: n_values=%zu format=%d", n_values, format);
    return LIA_ERR_INVALID;
  }
  wire_decode_launch(format, src_device, dst_device, n_values, (hipStream_t)stream, nullptr, nullptr);
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

extern "C" int lia_stream_prefetch_packed(lia_streamer* s, int slot, const void* host_ptr, size_t packed_bytes, size_t n_values, int format,
                                          int pinned) {
  int rc = lia_stream_begin(s, slot);
  if (rc) return rc;
  rc = lia_stream_copy_chunk_packed(s, slot, 0, host_ptr, packed_bytes, pinned);
  if (rc) return rc;
  rc = lia_stream_decode_packed(s, slot, n_values, format);
  if (rc) return rc;
  return lia_stream_mark_ready(s, slot);
}

extern "C" int lia_stream_mark_ready(lia_streamer* s, int slot) {
  if (!s || slot < 0 || slot >= s->n_slots) return LIA_ERR_INVALID;
  if (s->staging && s->decoded_on_side[slot]) {
    HIP_TRY(hipEventRecord(s->copied[slot], s->decode));              // ready = decoded
    s->decoded_on_side[slot] = 0;
  } else {
    HIP_TRY(hipEventRecord(s->t1[slot], s->copy));
    HIP_TRY(hipEventRecord(s->copied[slot], s->copy));
  }
  s->timing_pending[slot] = 1;
  s->was_marked[slot] = 1;
  return LIA_OK;
}

extern "C" int lia_stream_prefetch(lia_streamer* s, int slot, const void* host_ptr, size_t bytes, int pinned) {
  if (!s || slot < 0 || slot >= s->n_slots || !host_ptr || bytes > s->slot_bytes) {
    lia_set_error("lia_stream_prefetch: slot=%d bytes=%zu (slot holds %zu)", slot, bytes, s ? s->slot_bytes : 0);
    return LIA_ERR_INVALID;
  }
  int rc = lia_stream_begin(s, slot);
  if (rc) return rc;
  rc = lia_stream_copy_chunk(s, slot, 0, host_ptr, bytes, pinned);
  if (rc) return rc;
  return lia_stream_mark_ready(s, slot);
}

extern "C" int lia_stream_wait(lia_streamer* s, int slot, void* compute_stream) {
  if (!s || slot < 0 || slot >= s->n_slots) return LIA_ERR_INVALID;
  HIP_TRY(hipStreamWaitEvent((hipStream_t)compute_stream, s->copied[slot], 0));
  return LIA_OK;
}

extern "C" int lia_stream_release(lia_streamer* s, int slot, void* compute_stream) {
  if (!s || slot < 0 || slot >= s->n_slots) return LIA_ERR_INVALID;
  HIP_TRY(hipEventRecord(s->released[slot], (hipStream_t)compute_stream));
  s->has_release[slot] = 1;
  return LIA_OK;
}

// ------------------------------------------------------------------------------------------------
// decode mode: wire-format layers cached in the slots a decode step has no use for
// ------------------------------------------------------------------------------------------------
// A decode step is link-bound: its consumer holds a slot for 2-3 ms per layer, the link needs 14.5 ms per layer, so two slots and
// two landing buffers keep the link busy and the rest of the streamer's memory idles.  In decode mode that rest holds layers in
// their WIRE format; the decode kernel rebuilds such a layer in a slot every step and the layer never crosses the link again.
//   landing buffer b (< keep_slots): the staging area of slot b, cut loose from the slot.  lia_stream_land copies into it behind
//       drained[b], the decode that last read it; lia_stream_decode_landed decodes it into ANY kept slot behind landed[b] and the
//       slot's release, and records drained[b].
//   entry e: lia_stream_decode_cached fills it on first use (one H2D copy, counted like any copy) and decodes it into a kept slot.
// All copies stay on the copy stream and all decodes on the decode stream; nothing here waits on the host.
// the workspace bytes a mode turned on now would borrow: [*offset, *offset + bytes)
static size_t cache_lend_range(const lia_streamer* s, size_t* offset) {
  const lia_ctx* c = s->ctx;
  *offset = align_up(s->cfg_keep_bytes, 256);
  if (!s->cfg_lend || !c->ws || (c->ws_lent_to && c->ws_lent_to != s) || *offset >= c->ws_alloc_bytes) return 0;
  return c->ws_alloc_bytes - *offset;
}
static int cache_plan(const lia_streamer* s, int keep_slots, size_t entry_bytes, lia_cache_geometry* g) {
  size_t off = 0;
  const size_t lend = cache_lend_range(s, &off);
  return lia_cache_geometry_plan_extra(s->n_slots, s->slot_bytes, s->staging ? s->staging_bytes : 0, keep_slots, entry_bytes,
                                       s->cfg_landing_bytes, off, lend, s->extra ? s->extra_bytes : 0, g);
}
static char* cache_entry_ptr(lia_streamer* s, int e) {
  if (e < s->geo.in_slots) return s->slots + s->geo.offset[e];
  if (e < s->geo.in_slots + s->geo.in_staging) return s->staging + s->geo.offset[e];
  if (e < s->geo.n_entries - s->geo.in_extra) return s->ctx->ws + s->geo.offset[e];
  return s->extra + s->geo.offset[e];
}
static char* cache_landing_ptr(lia_streamer* s, int landing) { return s->staging + (size_t)landing * s->geo.landing_stride; }

extern "C" int lia_stream_cache_configure(lia_streamer* s, size_t landing_bytes, int lend_workspace, size_t workspace_keep_bytes) {
  if (!s) return LIA_ERR_INVALID;
  if (s->keep_slots) { lia_set_error("lia_stream_cache_configure: the mode is on"); return LIA_ERR_INVALID; }
  if (landing_bytes && s->staging && align_up(landing_bytes + LIA_CACHE_READ_SLACK, 256) > s->staging_bytes) {
    lia_set_error("lia_stream_cache_configure: a landing buffer of %zu bytes does not fit a staging area of %zu", landing_bytes, s->staging_bytes);
    return LIA_ERR_INVALID;
  }
  s->cfg_landing_bytes = landing_bytes;
  s->cfg_lend = lend_workspace ? 1 : 0;
  s->cfg_keep_bytes = lend_workspace ? workspace_keep_bytes : 0;
  return LIA_OK;
}

extern "C" int lia_stream_cache_extra(lia_streamer* s, size_t bytes) {
  if (!s) return LIA_ERR_INVALID;
  if (s->keep_slots) { lia_set_error("lia_stream_cache_extra: the mode is on"); return LIA_ERR_INVALID; }
  if (bytes == s->extra_bytes) return LIA_OK;
  if (s->extra) {
    // decodes of a mode that has ended may still read entries here
    if (s->staging) HIP_TRY(hipStreamSynchronize(s->decode));
    HIP_TRY(hipStreamSynchronize(s->copy));
    HIP_TRY(hipFree(s->extra));
    s->extra = nullptr; s->extra_bytes = 0;
  }
  if (bytes) {
    // a fresh allocation: its first writer, the copy stream, needs no fence
    if (hipMalloc((void**)&s->extra, bytes) != hipSuccess) {
      (void)hipGetLastError();
      s->extra = nullptr;
      lia_set_error("lia_stream_cache_extra: no device memory for %zu bytes", bytes);
      return LIA_ERR_MEMORY;
    }
    s->extra_bytes = bytes;
  }
  return LIA_OK;
}

extern "C" int lia_stream_cache_layout(lia_streamer* s, int keep_slots, size_t entry_bytes, lia_cache_geometry* out) {
  if (!s || !out) return LIA_ERR_INVALID;
  if (s->keep_slots) { *out = s->geo; return LIA_OK; }
  return cache_plan(s, keep_slots, entry_bytes, out);
}

extern "C" int lia_stream_cache_capacity(lia_streamer* s, int keep_slots, size_t entry_bytes) {
  if (!s) return 0;
  lia_cache_geometry g;
  return cache_plan(s, keep_slots, entry_bytes, &g) ? 0 : g.n_entries;
}

extern "C" int lia_stream_cache_enable(lia_streamer* s, int keep_slots, size_t entry_bytes) {
  if (!s) return LIA_ERR_INVALID;
  lia_cache_geometry g;
  const int bad = cache_plan(s, keep_slots, entry_bytes, &g);
  if (s->keep_slots || bad || g.n_entries == 0) {
    lia_set_error("lia_stream_cache_enable: keep_slots=%d entry_bytes=%zu on %d slots (%s)", keep_slots, entry_bytes, s->n_slots,
                  s->keep_slots ? "the mode is on" : bad ? "the configured landing buffers do not fit the staging areas" : "no room for an entry");
    return LIA_ERR_INVALID;
  }
  // the pool's first writer is the copy stream: behind the last consumers of the slots that leave the ring and behind their
  // prefetches' decodes (dropped ones included), which read the staging areas that leave with them
  for (int i = 0; i < s->n_slots; ++i) {
    if (i >= keep_slots && s->has_release[i]) HIP_TRY(hipStreamWaitEvent(s->copy, s->released[i], 0));
    // (a kept slot: its staging area becomes landing buffers and entries, still read by the decode of the slot's last legacy prefetch)
    if (s->was_marked[i]) HIP_TRY(hipStreamWaitEvent(s->copy, s->copied[i], 0));
    s->has_drained[i] = 0; s->landing_bytes[i] = 0;
  }
  // ... and, for the entries in the workspace, behind the compute stream's last use of it and the K/V deliveries draining from it
  if (g.in_workspace) {
    size_t keep = 0;
    (void)cache_lend_range(s, &keep);
    if (int rc = ctx_ws_lend(s->ctx, s, keep, s->copy, s->ws_fence)) return rc;
    s->lent = true;
  }
  s->keep_slots = keep_slots; s->geo = g;
  std::fill(s->entry_filled.begin(), s->entry_filled.end(), 0);
  return LIA_OK;
}

extern "C" int lia_stream_cache_disable(lia_streamer* s) {
  if (!s) return LIA_ERR_INVALID;
  if (!s->keep_slots) return LIA_OK;
  // Slots and staging areas return to the ring.  Their next writers are copies on the copy stream and decodes on the decode
  // stream: the latter run behind every decode of the mode by stream order, the former behind this event.
  HIP_TRY(hipEventRecord(s->cache_idle, s->decode));
  HIP_TRY(hipStreamWaitEvent(s->copy, s->cache_idle, 0));
  // the workspace returns to the context: its next user on the compute stream runs behind the decodes that read the entries there
  if (s->lent) {
    if (int rc = ctx_ws_take_back(s->ctx, s, s->cache_idle)) return rc;
    s->lent = false;
  }
  s->keep_slots = 0; memset(&s->geo, 0, sizeof(s->geo));
  std::fill(s->entry_filled.begin(), s->entry_filled.end(), 0);
  return LIA_OK;
}

// one timed copy of the mode on the copy stream (the caller has enqueued what it must wait for)
static int cache_copy(lia_streamer* s, char* dst, const void* host_ptr, size_t bytes, int pinned) {
  const int r = s->ring_next;
  s->ring_next = (r + 1) % LIA_CACHE_TIMING_RING;
  streamer_collect_ring(s, r, true);       // sixteen copies back: finished long ago
  HIP_TRY(hipEventRecord(s->r0[r], s->copy));
  if (pinned) HIP_TRY(hipMemcpyAsync(dst, host_ptr, bytes, hipMemcpyHostToDevice, s->copy));
  else if (int rc = staged_copy(s, dst, host_ptr, bytes)) return rc;
  HIP_TRY(hipEventRecord(s->r1[r], s->copy));
  s->ring_bytes[r] = bytes; s->ring_pending[r] = 1;
  return LIA_OK;
}

extern "C" int lia_stream_land(lia_streamer* s, int landing, const void* host_ptr, size_t packed_bytes, int pinned) {
  if (!s || !s->keep_slots || landing < 0 || landing >= s->keep_slots || !host_ptr || packed_bytes == 0 || packed_bytes > s->geo.landing_capacity) {
    lia_set_error("lia_stream_land: landing=%d bytes=%zu (decode mode %s, %d landing buffers of %zu)", landing, packed_bytes,
                  s && s->keep_slots ? "on" : "off", s ? s->keep_slots : 0, s ? s->geo.landing_capacity : 0);
    return LIA_ERR_INVALID;
  }
  if (s->has_drained[landing]) HIP_TRY(hipStreamWaitEvent(s->copy, s->drained[landing], 0));
  if (int rc = cache_copy(s, cache_landing_ptr(s, landing), host_ptr, packed_bytes, pinned)) return rc;
  HIP_TRY(hipEventRecord(s->landed[landing], s->copy));
  s->landing_bytes[landing] = packed_bytes;
  return LIA_OK;
}

// the decode stream takes over slot `slot`: behind its last consumer and behind whatever an abandoned prefetch still writes there
static int cache_claim_slot(lia_streamer* s, int slot) {
  if (s->has_release[slot]) HIP_TRY(hipStreamWaitEvent(s->decode, s->released[slot], 0));
  if (s->was_marked[slot]) HIP_TRY(hipStreamWaitEvent(s->decode, s->copied[slot], 0));
  return LIA_OK;
}
static int cache_slot_ready(lia_streamer* s, int slot) {
  HIP_TRY(hipEventRecord(s->copied[slot], s->decode));                  // ready = decoded, as in lia_stream_mark_ready
  s->was_marked[slot] = 1;
  return LIA_OK;
}

extern "C" int lia_stream_decode_landed(lia_streamer* s, int landing, int slot, size_t n_values, int format) {
  if (!s || !s->keep_slots || landing < 0 || landing >= s->keep_slots || slot < 0 || slot >= s->keep_slots || !s->landing_bytes[landing] ||
      n_values * 2 > s->slot_bytes || !wire_format_known(format) || (n_values % 1024)) {
    lia_set_error("lia_stream_decode_landed: landing=%d slot=%d n_values=%zu format=%d", landing, slot, n_values, format);
    return LIA_ERR_INVALID;
  }
  HIP_TRY(hipStreamWaitEvent(s->decode, s->landed[landing], 0));
  if (int rc = cache_claim_slot(s, slot)) return rc;
  if (int rc = launch_decode(s, cache_landing_ptr(s, landing), slot, n_values, format, (double)s->landing_bytes[landing])) return rc;
  HIP_TRY(hipEventRecord(s->drained[landing], s->decode));
  s->has_drained[landing] = 1; s->landing_bytes[landing] = 0;
  return cache_slot_ready(s, slot);
}

extern "C" int lia_stream_decode_cached(lia_streamer* s, int entry, int slot, const void* host_ptr, size_t packed_bytes, size_t n_values,
                                        int format, int pinned) {
  if (!s || !s->keep_slots || entry < 0 || entry >= s->geo.n_entries || slot < 0 || slot >= s->keep_slots || !host_ptr || packed_bytes == 0 ||
      packed_bytes + LIA_CACHE_READ_SLACK > s->geo.entry_stride || n_values * 2 > s->slot_bytes || !wire_format_known(format) || (n_values % 1024)) {
    lia_set_error("lia_stream_decode_cached: entry=%d slot=%d bytes=%zu n_values=%zu format=%d (%d entries, stride %zu)", entry, slot,
                  packed_bytes, n_values, format, s ? s->geo.n_entries : 0, s ? s->geo.entry_stride : 0);
    return LIA_ERR_INVALID;
  }
  char* const at = cache_entry_ptr(s, entry);
  if (!s->entry_filled[entry]) {
    // the one crossing of this layer.  (The event of a slot outside the ring serves: its wait is enqueued right here.)
    if (int rc = cache_copy(s, at, host_ptr, packed_bytes, pinned)) return rc;
    HIP_TRY(hipEventRecord(s->landed[s->keep_slots], s->copy));
    HIP_TRY(hipStreamWaitEvent(s->decode, s->landed[s->keep_slots], 0));
    s->entry_filled[entry] = 1; s->entry_src[entry] = host_ptr; s->entry_bytes[entry] = packed_bytes;
  } else if (s->entry_src[entry] != host_ptr || s->entry_bytes[entry] != packed_bytes) {
    // an entry is never refilled while decodes may still read it: the caller turns the mode off and on again
    lia_set_error("lia_stream_decode_cached: entry %d holds another layer", entry);
    return LIA_ERR_INVALID;
  }
  if (int rc = cache_claim_slot(s, slot)) return rc;
  if (int rc = launch_decode(s, at, slot, n_values, format, (double)packed_bytes)) return rc;
  return cache_slot_ready(s, slot);
}

// A wire-format layer that lies in device memory already (a resident layer the model holds packed): decode only.  Mode on or off,
// the decode stream is the slot's next writer, behind its last consumer and whatever was queued into it before.
extern "C" int lia_stream_decode_device(lia_streamer* s, int slot, const void* src_device, size_t packed_bytes, size_t n_values, int format) {
  if (!s || slot < 0 || slot >= s->n_slots || (s->keep_slots && slot >= s->keep_slots) || !src_device || packed_bytes == 0 ||
      n_values * 2 > s->slot_bytes || !wire_format_known(format) || (n_values % 1024)) {
    lia_set_error("lia_stream_decode_device: slot=%d bytes=%zu n_values=%zu format=%d (%d slots%s)", slot, packed_bytes, n_values, format,
                  s ? s->n_slots : 0, s && s->keep_slots ? ", decode mode on" : "");
    return LIA_ERR_INVALID;
  }
  if (int rc = ensure_staging(s)) return rc;            // the decode stream and its timing events live with the staging areas
  if (int rc = cache_claim_slot(s, slot)) return rc;
  if (int rc = launch_decode(s, (const char*)src_device, slot, n_values, format, (double)packed_bytes)) return rc;
  return cache_slot_ready(s, slot);
}

extern "C" int lia_stream_stats(lia_streamer* s, double* bytes, double* busy_ms, int reset) {
  if (!s) return LIA_ERR_INVALID;
  for (int i = 0; i < s->n_slots; ++i) streamer_collect(s, i);
  for (size_t r = 0; r < s->ring_pending.size(); ++r) streamer_collect_ring(s, (int)r, true);
  if (bytes) *bytes = s->bytes;
  if (busy_ms) *busy_ms = s->busy_ms;
  if (reset) { s->bytes = 0; s->busy_ms = 0; }
  return LIA_OK;
}

// Live timing of the wire-format decode kernel (the largest GPU consumer of a link-bound decode step; bench.py's
// roofline.dominant_kernel): HIP events on the decode stream around the main decode kernel of every packed layer since the last
// reset.  bytes_in = encoded bytes the kernel read, bytes_out = bf16 bytes it wrote (its algorithmic traffic: each once).
static int decode_stats(lia_streamer* s, bool wait, long* launches, double* ms, double* bytes_in, double* bytes_out, int reset) {
  if (!s) return LIA_ERR_INVALID;
  for (int i = 0; i < s->n_slots; ++i) streamer_collect_decode(s, i, wait);
  if (!wait) (void)hipGetLastError();   // hipErrorNotReady from the query is an answer, not an error
  if (launches) *launches = s->dec_launches;
  if (ms) *ms = s->dec_ms;
  if (bytes_in) *bytes_in = s->dec_in;
  if (bytes_out) *bytes_out = s->dec_out;
  if (reset) { s->dec_ms = s->dec_in = s->dec_out = 0; s->dec_launches = 0; }
  return LIA_OK;
}
extern "C" int lia_stream_decode_stats(lia_streamer* s, long* launches, double* ms, double* bytes_in, double* bytes_out, int reset) {
  return decode_stats(s, true, launches, ms, bytes_in, bytes_out, reset);
}
// The non-blocking form: only copies whose end event has already completed are counted (a queued copy stays pending and is
// counted by a later call).  For callers inside the token loop, which must never wait for the prefetched layers.
extern "C" int lia_stream_poll_decode_stats(lia_streamer* s, long* launches, double* ms, double* bytes_in, double* bytes_out, int reset) {
  return decode_stats(s, false, launches, ms, bytes_in, bytes_out, reset);
}

extern "C" int lia_stream_poll_stats(lia_streamer* s, double* bytes, double* busy_ms) {
  if (!s) return LIA_ERR_INVALID;
  for (int i = 0; i < s->n_slots; ++i)
    if (s->timing_pending[i] && hipEventQuery(s->t1[i]) == hipSuccess) streamer_collect(s, i);
  for (size_t r = 0; r < s->ring_pending.size(); ++r) streamer_collect_ring(s, (int)r, false);
  (void)hipGetLastError();   // hipErrorNotReady from the query is an answer, not an error
  if (bytes) *bytes = s->bytes;
  if (busy_ms) *busy_ms = s->busy_ms;
  return LIA_OK;
}

// ------------------------------------------------------------------------------------------------
// pinned / registered host memory
// ------------------------------------------------------------------------------------------------
extern "C" void* lia_host_alloc_pinned(size_t size) {
  void* p = nullptr;
  hipError_t e = hipHostMalloc(&p, size, hipHostMallocDefault);
  if (e != hipSuccess) {
    lia_set_error("hipHostMalloc(%zu) failed: %s", size, hipGetErrorString(e));
    return nullptr;
  }
  return p;
}
extern "C" void lia_host_free_pinned(void* p) { if (p) (void)hipHostFree(p); }

extern "C" int lia_memcpy_h2d(void* dst_device, const void* src_host, size_t bytes) {
  if (!dst_device || !src_host) return LIA_ERR_MISSING;
  HIP_TRY(hipMemcpy(dst_device, src_host, bytes, hipMemcpyHostToDevice));
  return LIA_OK;
}
// Small transfer between device memory and MAPPED pinned host memory by a kernel on `stream` (16-byte multiples):
// the copy engines belong to the weight stream, a hipMemcpy would queue behind a 0.8-1.2 GB layer copy.
extern "C" int lia_blit(void* dst, const void* src, size_t bytes, void* stream) {
  if (!dst || !src) return LIA_ERR_MISSING;
  if (bytes % 16) { lia_set_error("lia_blit: %zu bytes is not a multiple of 16", bytes); return LIA_ERR_INVALID; }
  lia_blit_launch(dst, src, bytes, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return LIA_OK;
}

extern "C" int lia_memcpy_d2h(void* dst_host, const void* src_device, size_t bytes) {
  if (!dst_host || !src_device) return LIA_ERR_MISSING;
  HIP_TRY(hipMemcpy(dst_host, src_device, bytes, hipMemcpyDeviceToHost));
  return LIA_OK;
}

extern "C" int lia_numa_register(void* ptr, size_t size) {
  if (!ptr || !size) return LIA_ERR_INVALID;
  hipError_t e = hipHostRegister(ptr, size, hipHostRegisterDefault);
  if (e != hipSuccess) {
    lia_set_error("hipHostRegister(%p, %zu) failed: %s", ptr, size, hipGetErrorString(e));
    return LIA_ERR_MEMORY;
  }
  return LIA_OK;
}
// Register a READ-ONLY mapping (a shared, PROT_READ mmap of a checkpoint file): the pages are pinned without write intent, so
// they stay the page-cache pages -- no private copy of the file appears in anonymous memory.
extern "C" int lia_numa_register_readonly(void* ptr, size_t size) {
  if (!ptr || !size) return LIA_ERR_INVALID;
  hipError_t e = hipHostRegister(ptr, size, hipHostRegisterReadOnly);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    lia_set_error("hipHostRegister(%p, %zu, read-only) failed: %s", ptr, size, hipGetErrorString(e));
    return LIA_ERR_MEMORY;
  }
  return LIA_OK;
}
extern "C" int lia_numa_unregister(void* ptr) {
  if (!ptr) return LIA_ERR_INVALID;
  HIP_TRY(hipHostUnregister(ptr));
  return LIA_OK;
}
