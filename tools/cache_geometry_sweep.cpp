// Stand-alone sweep of lia_cache_geometry_plan (csrc/lia_cache_geometry.cpp) for a sanitizer build on the host:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/cache_geometry_sweep.cpp
//       isca-2025-lia_amd/csrc/lia_cache_geometry.cpp -o cache_geometry_sweep && ./cache_geometry_sweep
// No GPU and no other file of the library.  For every case: the entries are pairwise disjoint, inside their region, clear of the
// landing buffers and of the kept workspace, start on multiples of 256 and keep the read slack behind the layer.  Prints one line
// per case and exits 1 at the first violated property.  (tests/test_cache_geometry.py runs the same cases through the library.)
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "lia_hip.h"

struct Case {
  const char* name;
  int n_slots;
  size_t slot_bytes, staging_bytes;
  int keep_slots;
  size_t entry_bytes, landing_bytes, keep_bytes, workspace_bytes;   // workspace_bytes == 0: nothing lent
  int want_rc, want_slots, want_staging, want_workspace;             // want_* < 0: not pinned
};

#define FAIL(...) do { printf("FAILED %s: ", c.name); printf(__VA_ARGS__); printf("\n"); exit(1); } while (0)

static size_t up256(size_t v) { return (v + 255) / 256 * 256; }

static void check(const Case& c) {
  lia_cache_geometry g;
  const size_t lend_at = up256(c.keep_bytes);
  const size_t lend = c.workspace_bytes > lend_at ? c.workspace_bytes - lend_at : 0;
  // (the lent range starts at the keep as the caller states it: the function rounds it up and takes the difference off the range)
  const int rc = lia_cache_geometry_plan(c.n_slots, c.slot_bytes, c.staging_bytes, c.keep_slots, c.entry_bytes, c.landing_bytes, c.keep_bytes,
                                         lend ? c.workspace_bytes - c.keep_bytes : 0, &g);
  if (rc != c.want_rc) FAIL("rc %d, expected %d", rc, c.want_rc);
  if (rc != LIA_OK) {
    if (g.n_entries || g.entry_stride) FAIL("a refused geometry is not zeroed");
    printf("ok %-28s refused\n", c.name);
    return;
  }
  if (g.n_entries != g.in_slots + g.in_staging + g.in_workspace || g.n_entries < 0 || g.n_entries > LIA_CACHE_MAX_ENTRIES) FAIL("counts %d = %d + %d + %d", g.n_entries, g.in_slots, g.in_staging, g.in_workspace);
  if ((c.want_slots >= 0 && g.in_slots != c.want_slots) || (c.want_staging >= 0 && g.in_staging != c.want_staging) ||
      (c.want_workspace >= 0 && g.in_workspace != c.want_workspace))
    FAIL("%d + %d + %d entries, expected %d + %d + %d", g.in_slots, g.in_staging, g.in_workspace, c.want_slots, c.want_staging, c.want_workspace);
  if (g.n_entries && (g.entry_stride % 256 || g.entry_stride < c.entry_bytes + LIA_CACHE_READ_SLACK)) FAIL("stride %zu", g.entry_stride);
  // [begin, end) of every entry per allocation: 0 slots, 1 staging, 2 workspace
  struct Span { int region; size_t begin, end; };
  std::vector<Span> spans;
  for (int e = 0; e < g.n_entries; ++e) {
    const int region = e < g.in_slots ? 0 : e < g.in_slots + g.in_staging ? 1 : 2;
    const size_t at = g.offset[e], end = at + c.entry_bytes + LIA_CACHE_READ_SLACK;
    if (at % 256) FAIL("entry %d at %zu is not 256-aligned", e, at);
    size_t lo, hi;
    if (region == 0) { lo = (size_t)c.keep_slots * c.slot_bytes; hi = (size_t)c.n_slots * c.slot_bytes; }
    else if (region == 1) { lo = (size_t)c.keep_slots * g.landing_stride; hi = (size_t)c.n_slots * c.staging_bytes; }
    else { lo = c.keep_bytes; hi = c.workspace_bytes; }
    if (at < lo || end > hi) FAIL("entry %d [%zu, %zu) leaves region %d [%zu, %zu)", e, at, end, region, lo, hi);
    for (const Span& s : spans)
      if (s.region == region && at < s.end && s.begin < end) FAIL("entry %d overlaps [%zu, %zu)", e, s.begin, s.end);
    spans.push_back({region, at, end});
  }
  // the landing buffers: inside the staging allocation, apart from each other, with their slack when they were cut to size
  if (g.n_entries) {
    const size_t room = c.landing_bytes ? c.landing_bytes + LIA_CACHE_READ_SLACK : c.staging_bytes;
    if (g.landing_capacity != (c.landing_bytes ? c.landing_bytes : c.staging_bytes) || g.landing_stride < room || g.landing_stride > c.staging_bytes)
      FAIL("landing stride %zu capacity %zu", g.landing_stride, g.landing_capacity);
  }
  printf("ok %-28s %d + %d + %d entries, stride %zu, landing stride %zu\n", c.name, g.in_slots, g.in_staging, g.in_workspace, g.entry_stride,
         g.landing_stride);
}

int main() {
  // OPT-30B at batch 64: slot = the bf16 layer, staging = lia_pack10_bound of it, entry = the rANS-coded layer, workspace of a
  // 16384-row prefill, keep of a 64-row decode step
  const size_t slot = 1233311744, staging = 1392445440, entry = 815894255, ws = 3523215360, keep = 107675648;
  const Case cases[] = {
      {"headline", 4, slot, staging, 2, entry, entry, keep, ws, LIA_OK, 3, 4, 4},
      {"headline, not configured", 4, slot, staging, 2, entry, 0, 0, 0, LIA_OK, 3, 3, 0},
      {"headline, landing only", 4, slot, staging, 2, entry, entry, 0, 0, LIA_OK, 3, 4, 0},
      {"headline, lend only", 4, slot, staging, 2, entry, 0, keep, ws, LIA_OK, 3, 3, 4},
      {"three slots", 3, slot, staging, 2, entry, entry, keep, ws, LIA_OK, 1, 3, 4},
      {"keep not a multiple of 256", 4, 2 * 68608, 155000, 2, 91000, 91003, (1 << 20) + 3, 4 << 20, LIA_OK, -1, -1, -1},
      {"entry divides no region", 4, 1000192, 1130001, 2, 333333, 400001, 70001, 3000001, LIA_OK, -1, -1, -1},
      {"landing larger than staging", 4, slot, staging, 2, entry, staging, keep, ws, LIA_ERR_INVALID, 0, 0, 0},
      {"landing + slack > staging", 4, slot, staging, 2, entry, staging - 100, keep, ws, LIA_ERR_INVALID, 0, 0, 0},
      {"zero lend", 4, slot, staging, 2, entry, entry, ws, ws, LIA_OK, 3, 4, 0},
      {"keep beyond the workspace", 4, slot, staging, 2, entry, entry, ws + 5, ws, LIA_OK, 3, 4, 0},
      {"more than 64 entries", 4, (size_t)1 << 20, (size_t)1200000, 2, 40000, 41000, 4096, (size_t)64 << 20, LIA_OK, 47, 17, 0},
      {"64 reached in the workspace", 3, (size_t)1 << 20, (size_t)100000, 2, 40000, 41000, 4096, (size_t)64 << 20, LIA_OK, 23, 4, 37},
      {"64 entries in the slots", 16, (size_t)1 << 20, (size_t)1200000, 2, 40000, 0, 0, 0, LIA_OK, 64, 0, 0},
      {"two slots", 2, slot, staging, 2, entry, entry, keep, ws, LIA_OK, 0, 0, 0},
      {"no staging", 4, slot, 0, 2, entry, 0, keep, ws, LIA_OK, 0, 0, 0},
      {"entry larger than anything", 4, 4096, 8192, 2, 1 << 20, 0, 0, 1 << 19, LIA_OK, 0, 0, 0},
  };
  for (const Case& c : cases) check(c);
  printf("all cases hold\n");
  return 0;
}
