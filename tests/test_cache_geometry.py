"""lia_cache_geometry_plan, the one place that says where the wire cache's entries lie (include/lia_hip.h), without a GPU.

Every case of the sweep asserts: the entries are pairwise disjoint, inside their region (the slots that leave the ring, the staging
allocation behind the landing buffers, the workspace behind the kept part), 256-aligned, with LIA_CACHE_READ_SLACK behind the layer,
and never more than LIA_CACHE_MAX_ENTRIES.  The headline's sizes give 3 + 4 + 4 entries; not configured, 3 + 3 + 0 as before.
tools/cache_geometry_sweep.cpp holds the same cases as a stand-alone program; the last test builds it with the address and
undefined-behaviour sanitizers (host code only, its own main) and runs it."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, -1
# OPT-30B at batch 64: the bf16 layer, lia_pack10_bound of it, the rANS-coded layer, the workspace of a 16384-row prefill and what
# a 64-row decode step keeps of it (OffloadScheduler._ensure's formula)
SLOT, STAGING, ENTRY, WS, KEEP = 1233311744, 1392445440, 815894255, 3523215360, 107675648
MB = 1 << 20

# name: (n_slots, slot, staging, keep_slots, entry, landing, keep, workspace (0: nothing lent), rc, entries per region or None)
CASES = {
    "headline": (4, SLOT, STAGING, 2, ENTRY, ENTRY, KEEP, WS, OK, (3, 4, 4)),
    "headline, not configured": (4, SLOT, STAGING, 2, ENTRY, 0, 0, 0, OK, (3, 3, 0)),
    "headline, landing only": (4, SLOT, STAGING, 2, ENTRY, ENTRY, 0, 0, OK, (3, 4, 0)),
    "headline, lend only": (4, SLOT, STAGING, 2, ENTRY, 0, KEEP, WS, OK, (3, 3, 4)),
    "three slots": (3, SLOT, STAGING, 2, ENTRY, ENTRY, KEEP, WS, OK, (1, 3, 4)),
    "keep not a multiple of 256": (4, 2 * 68608, 155000, 2, 91000, 91003, MB + 3, 4 * MB, OK, None),
    "entry divides no region": (4, 1000192, 1130001, 2, 333333, 400001, 70001, 3000001, OK, None),
    "landing larger than staging": (4, SLOT, STAGING, 2, ENTRY, STAGING, KEEP, WS, INVALID, None),
    "landing + slack > staging": (4, SLOT, STAGING, 2, ENTRY, STAGING - 100, KEEP, WS, INVALID, None),
    "zero lend": (4, SLOT, STAGING, 2, ENTRY, ENTRY, WS, WS, OK, (3, 4, 0)),
    "keep beyond the workspace": (4, SLOT, STAGING, 2, ENTRY, ENTRY, WS + 5, WS, OK, (3, 4, 0)),
    "more than 64 entries": (4, MB, 1200000, 2, 40000, 41000, 4096, 64 * MB, OK, (47, 17, 0)),
    "64 reached in the workspace": (3, MB, 100000, 2, 40000, 41000, 4096, 64 * MB, OK, (23, 4, 37)),
    "64 entries in the slots": (16, MB, 1200000, 2, 40000, 0, 0, 0, OK, (64, 0, 0)),
    "two slots": (2, SLOT, STAGING, 2, ENTRY, ENTRY, KEEP, WS, OK, (0, 0, 0)),
    "no staging": (4, SLOT, 0, 2, ENTRY, 0, KEEP, WS, OK, (0, 0, 0)),
    "entry larger than anything": (4, 4096, 8192, 2, MB, 0, 0, MB // 2, OK, (0, 0, 0)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_entries_stay_apart_and_inside_their_region(name):
    from lia_amd import _native as N
    n_slots, slot, staging, keep_slots, entry, landing, keep, ws, want_rc, want = CASES[name]
    slack = N.LIA_CACHE_READ_SLACK
    g = N.CacheGeometry()
    lend = ws - keep if ws > (keep + 255) // 256 * 256 else 0
    rc = N.lib().lia_cache_geometry_plan(n_slots, slot, staging, keep_slots, entry, landing, keep, lend, ctypes.byref(g))
    assert rc == want_rc
    if rc != OK:
        assert g.n_entries == 0 and g.entry_stride == 0
        return
    counts = (g.in_slots, g.in_staging, g.in_workspace)
    assert g.n_entries == sum(counts) and 0 <= g.n_entries <= N.LIA_CACHE_MAX_ENTRIES
    if want is not None:
        assert counts == want
    if not g.n_entries:
        return
    assert g.entry_stride % 256 == 0 and g.entry_stride >= entry + slack
    # the landing buffers: b x landing_stride, each with room for the largest landed layer (+ slack when cut to size)
    assert g.landing_capacity == (landing or staging)
    assert (landing + slack if landing else staging) <= g.landing_stride <= staging
    regions = [(keep_slots * slot, n_slots * slot), (keep_slots * g.landing_stride, n_slots * staging), (keep, ws)]
    spans = []
    for e in range(g.n_entries):
        region = 0 if e < g.in_slots else 1 if e < g.in_slots + g.in_staging else 2
        at, end = g.offset[e], g.offset[e] + entry + slack
        lo, hi = regions[region]
        assert at % 256 == 0, (e, at)
        assert lo <= at and end <= hi, f"entry {e} [{at}, {end}) leaves region {region} [{lo}, {hi})"
        assert all(r != region or end <= a or b <= at for r, a, b in spans), f"entry {e} overlaps another"
        spans.append((region, at, end))


def test_the_planner_counts_with_the_same_function():
    """Box(wire_cache=True) alone: the 3 + 3 of the measurements it is calibrated on; wire_cache_ws with the headline's batch and
    prompt: 3 + 4 + 4"""
    from lia_amd import planner
    from lia_amd.model import resolve_shape
    sh = resolve_shape("opt-30b")
    box = planner.Box(host_threads=16, host_mem_gb=280.0, wire_ratio=10.585 / 16, wire_cache=True)
    assert planner.wire_cache_layers(sh, box, 44) == 6 and planner.wire_cache_layers(sh, box, 44, B=64, T=256) == 6
    box.wire_cache_ws = True
    assert planner.wire_cache_layers(sh, box, 44) == 7                       # landing buffers cut to size; no workspace stated
    assert planner.wire_cache_layers(sh, box, 44, B=64, T=256) == 11
    assert planner.wire_cache_layers(sh, box, 9, B=64, T=256) == 9           # never more than stream
    off = planner.Box(host_threads=16, host_mem_gb=280.0, wire_ratio=10.585 / 16, wire_cache_ws=True)
    assert planner.wire_cache_layers(sh, off, 44, B=64, T=256) == 0          # not without the cache itself
    pre6, dec6, *_ = planner.estimate(sh, 64, 256, 32, 10, 2, planner.Box(host_threads=16, host_mem_gb=280.0, wire_ratio=10.585 / 16, wire_cache=True))
    pre11, dec11, *_ = planner.estimate(sh, 64, 256, 32, 10, 2, box)
    assert pre11 == pre6 and dec11 < dec6


def test_the_sweep_program_is_clean_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the library's host code; it must be here"
    exe = str(tmp_path / "cache_geometry_sweep")
    subprocess.run([cxx, "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "cache_geometry_sweep.cpp"),
                    os.path.join(ROOT, "isca-2025-lia_amd", "csrc", "lia_cache_geometry.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.splitlines()[-1] == "all cases hold" and "FAILED" not in out
    assert len([line for line in out.splitlines() if line.startswith("ok ")]) == len(CASES)
