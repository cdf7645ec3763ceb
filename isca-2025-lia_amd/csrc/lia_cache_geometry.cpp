// lia_cache_geometry_plan / _plan_extra (include/lia_hip.h): where the wire cache's entries lie in the memory the streamer and the context own.
// Pure arithmetic on sizes -- no HIP, no other file of the library -- so the streamer, the planner and a host-only test program
// (tools/cache_geometry_sweep.cpp) share one answer.
#include <string.h>

#include "../../include/lia_hip.h"

static size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// entries of `stride` bytes from `begin` (rounded up to 256) while they end at or before `end`; at most `room` of them
static int fill_region(size_t begin, size_t end, size_t stride, int room, size_t* offset) {
  int n = 0;
  for (size_t at = up256(begin); n < room && at <= end && stride <= end - at; at += stride) offset[n++] = at;
  return n;
}

extern "C" int lia_cache_geometry_plan_extra(int n_slots, size_t slot_bytes, size_t staging_bytes, int keep_slots, size_t entry_bytes,
                                             size_t landing_bytes, size_t lend_offset, size_t lend_bytes, size_t extra_bytes,
                                             lia_cache_geometry* out) {
  if (!out) return LIA_ERR_INVALID;
  memset(out, 0, sizeof(*out));
  if (n_slots < 1 || keep_slots < 1 || keep_slots >= n_slots || slot_bytes == 0 || staging_bytes == 0 || entry_bytes == 0) return LIA_OK;
  // sizes beyond any device's memory: refuse before a sum below could wrap
  const size_t huge = (size_t)1 << 48;
  if (slot_bytes > huge || staging_bytes > huge || entry_bytes > huge || landing_bytes > huge || lend_offset > huge || lend_bytes > huge ||
      extra_bytes > huge || n_slots > 4096)
    return LIA_ERR_INVALID;
  const size_t landing_stride = landing_bytes ? up256(landing_bytes + LIA_CACHE_READ_SLACK) : staging_bytes;
  if (landing_stride > staging_bytes) return LIA_ERR_INVALID;
  out->entry_stride = up256(entry_bytes + LIA_CACHE_READ_SLACK);
  out->landing_stride = landing_stride;
  out->landing_capacity = landing_bytes ? landing_bytes : staging_bytes;
  int n = 0;
  out->in_slots = fill_region((size_t)keep_slots * slot_bytes, (size_t)n_slots * slot_bytes, out->entry_stride, LIA_CACHE_MAX_ENTRIES - n,
                              out->offset + n);
  n += out->in_slots;
  out->in_staging = fill_region((size_t)keep_slots * landing_stride, (size_t)n_slots * staging_bytes, out->entry_stride,
                                LIA_CACHE_MAX_ENTRIES - n, out->offset + n);
  n += out->in_staging;
  if (lend_bytes) out->in_workspace = fill_region(lend_offset, lend_offset + lend_bytes, out->entry_stride, LIA_CACHE_MAX_ENTRIES - n, out->offset + n);
  n += out->in_workspace;
  // the streamer's extra allocation (lia_stream_cache_extra), whole: offsets from its start
  if (extra_bytes) out->in_extra = fill_region(0, extra_bytes, out->entry_stride, LIA_CACHE_MAX_ENTRIES - n, out->offset + n);
  n += out->in_extra;
  out->n_entries = n;
  return LIA_OK;
}

extern "C" int lia_cache_geometry_plan(int n_slots, size_t slot_bytes, size_t staging_bytes, int keep_slots, size_t entry_bytes,
                                       size_t landing_bytes, size_t lend_offset, size_t lend_bytes, lia_cache_geometry* out) {
  return lia_cache_geometry_plan_extra(n_slots, slot_bytes, staging_bytes, keep_slots, entry_bytes, landing_bytes, lend_offset, lend_bytes, 0, out);
}
