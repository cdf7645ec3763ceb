// Stand-alone sweep of lia_cache_geometry_plan_extra (csrc/lia_cache_geometry.cpp) for a sanitizer build on the host:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/cache_geometry_extra_sweep.cpp
//       isca-2025-lia_amd/csrc/lia_cache_geometry.cpp -o cache_geometry_extra_sweep && ./cache_geometry_extra_sweep
// No GPU and no other file of the library.  For every base case x every size of the extra region: without an extra region the
// answer is lia_cache_geometry_plan's, field for field; with one, the first three regions keep their entries (while the 64 are
// not reached), the extra entries are 256-aligned, pairwise disjoint, inside [0, extra_bytes) with the read slack behind the layer,
// and as many as fit.  Prints one line per case and exits 1 at the first violated property.
// (tests/test_cache_geometry_extra.py runs the same through the library; tools/cache_geometry_sweep.cpp sweeps the old function.)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "lia_hip.h"

struct Base {
  const char* name;
  int n_slots;
  size_t slot_bytes, staging_bytes;
  int keep_slots;
  size_t entry_bytes, landing_bytes, keep_bytes, workspace_bytes;
};

#define FAIL(...) do { printf("FAILED %s / %s: ", b.name, what); printf(__VA_ARGS__); printf("\n"); exit(1); } while (0)

static size_t up256(size_t v) { return (v + 255) / 256 * 256; }

static void check(const Base& b, const char* what, size_t extra_bytes, int want_extra) {
  lia_cache_geometry g0, g;
  const size_t lend_at = up256(b.keep_bytes);
  const size_t lend = b.workspace_bytes > lend_at ? b.workspace_bytes - b.keep_bytes : 0;
  const int rc0 = lia_cache_geometry_plan(b.n_slots, b.slot_bytes, b.staging_bytes, b.keep_slots, b.entry_bytes, b.landing_bytes, b.keep_bytes, lend, &g0);
  const int rc = lia_cache_geometry_plan_extra(b.n_slots, b.slot_bytes, b.staging_bytes, b.keep_slots, b.entry_bytes, b.landing_bytes,
                                               b.keep_bytes, lend, extra_bytes, &g);
  if (rc != rc0) FAIL("rc %d, without the region %d", rc, rc0);
  if (extra_bytes == 0 && memcmp(&g, &g0, sizeof(g))) FAIL("extra_bytes = 0 differs from lia_cache_geometry_plan");
  if (rc != LIA_OK) {
    if (g.n_entries || g.entry_stride || g.in_extra) FAIL("a refused geometry is not zeroed");
    printf("ok %-28s %-10s refused\n", b.name, what);
    return;
  }
  if (g.n_entries != g.in_slots + g.in_staging + g.in_workspace + g.in_extra || g.n_entries < 0 || g.n_entries > LIA_CACHE_MAX_ENTRIES)
    FAIL("counts %d = %d + %d + %d + %d", g.n_entries, g.in_slots, g.in_staging, g.in_workspace, g.in_extra);
  if (g.in_slots != g0.in_slots || g.in_staging != g0.in_staging || g.in_workspace != g0.in_workspace || g.entry_stride != g0.entry_stride ||
      g.landing_stride != g0.landing_stride || g.landing_capacity != g0.landing_capacity)
    FAIL("the first three regions moved");
  for (int e = 0; e < g0.n_entries; ++e)
    if (g.offset[e] != g0.offset[e]) FAIL("entry %d moved", e);
  // a geometry with nothing to offer (two slots, no staging) offers no extra entry either; else as many as fit, up to the 64
  int want = want_extra;
  if (g.entry_stride == 0) want = 0;
  if (want > LIA_CACHE_MAX_ENTRIES - g0.n_entries) want = LIA_CACHE_MAX_ENTRIES - g0.n_entries;
  if (g.in_extra != want) FAIL("%d extra entries, expected %d", g.in_extra, want);
  for (int k = 0; k < g.in_extra; ++k) {
    const size_t at = g.offset[g0.n_entries + k], end = at + b.entry_bytes + LIA_CACHE_READ_SLACK;
    if (at % 256) FAIL("extra entry %d at %zu is not 256-aligned", k, at);
    if (end > extra_bytes) FAIL("extra entry %d [%zu, %zu) leaves the region of %zu bytes", k, at, end, extra_bytes);
    if (k && at < g.offset[g0.n_entries + k - 1] + b.entry_bytes + LIA_CACHE_READ_SLACK) FAIL("extra entry %d overlaps entry %d", k, k - 1);
  }
  printf("ok %-28s %-10s %d + %d + %d + %d entries\n", b.name, what, g.in_slots, g.in_staging, g.in_workspace, g.in_extra);
}

int main() {
  // OPT-30B at batch 64 (tools/cache_geometry_sweep.cpp), and the layer size the headline run reports
  const size_t slot = 1233311744, staging = 1392445440, entry = 815894255, ws = 3523215360, keep = 107675648;
  const Base bases[] = {
      {"headline", 4, slot, staging, 2, entry, entry, keep, ws},
      {"headline, not configured", 4, slot, staging, 2, entry, 0, 0, 0},
      {"three slots", 3, slot, staging, 2, entry, entry, keep, ws},
      {"keep not a multiple of 256", 4, 2 * 68608, 155000, 2, 91000, 91003, (1 << 20) + 3, 4 << 20},
      {"entry divides no region", 4, 1000192, 1130001, 2, 333333, 400001, 70001, 3000001},
      {"landing larger than staging", 4, slot, staging, 2, entry, staging, keep, ws},
      {"more than 64 entries", 4, (size_t)1 << 20, (size_t)1200000, 2, 40000, 41000, 4096, (size_t)64 << 20},
      {"64 reached in the workspace", 3, (size_t)1 << 20, (size_t)100000, 2, 40000, 41000, 4096, (size_t)64 << 20},
      {"62 entries before the region", 16, (size_t)1 << 20, (size_t)1200000, 2, 496000, 0, 0, 0},
      {"two slots", 2, slot, staging, 2, entry, entry, keep, ws},
      {"no staging", 4, slot, 0, 2, entry, 0, keep, ws},
  };
  for (const Base& b : bases) {
    const size_t stride = up256(b.entry_bytes + LIA_CACHE_READ_SLACK);
    // (an entry takes its whole stride of the region, as in the other three)
    check(b, "none", 0, 0);
    check(b, "one short", stride - 1, 0);
    check(b, "one", stride, 1);
    check(b, "two short", 2 * stride - 1, 1);
    check(b, "two", 2 * stride, 2);
    check(b, "five", 5 * stride + 100, 5);
  }
  printf("all cases hold\n");
  return 0;
}
