"""lia_cache_geometry_plan_extra: the wire cache's geometry with a fourth region, the streamer's extra allocation (what a model
saves by holding its resident layers packed, lia_stream_cache_extra), without a GPU.

  * extra_bytes = 0 is lia_cache_geometry_plan, field for field, on every case of tests/test_cache_geometry.py's table;
  * regions of 0, 1 and 2 entries and one a byte short of an entry: the first three regions never move, the extra entries lie inside
    [0, extra_bytes), 256-aligned, apart, with the read slack behind the layer;
  * the headline's numbers give 3 + 4 + 4 + 2 = 13 entries, and the planner counts with the same function;
  * tools/cache_geometry_extra_sweep.cpp holds the sweep as a stand-alone program; the last test builds it with the address and
    undefined-behaviour sanitizers (host code only, its own main) and runs it."""
import ctypes
import os
import shutil
import subprocess

import pytest

from test_cache_geometry import CASES, OK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("n_entries", "in_slots", "in_staging", "in_workspace", "in_extra", "entry_stride", "landing_stride", "landing_capacity")


def plan(case, extra=None):
    from lia_amd import _native as N
    n_slots, slot, staging, keep_slots, entry, landing, keep, ws = case[:8]
    lend = ws - keep if ws > (keep + 255) // 256 * 256 else 0
    g = N.CacheGeometry()
    if extra is None:
        rc = N.lib().lia_cache_geometry_plan(n_slots, slot, staging, keep_slots, entry, landing, keep, lend, ctypes.byref(g))
    else:
        rc = N.lib().lia_cache_geometry_plan_extra(n_slots, slot, staging, keep_slots, entry, landing, keep, lend, extra, ctypes.byref(g))
    return rc, g


def fields(g):
    return tuple(getattr(g, f) for f in FIELDS) + tuple(g.offset)


@pytest.mark.parametrize("name", list(CASES))
def test_no_extra_region_is_the_old_function(name):
    rc0, g0 = plan(CASES[name])
    rc, g = plan(CASES[name], 0)
    assert rc == rc0 == CASES[name][8]
    assert fields(g) == fields(g0) and g.in_extra == 0
    assert bytes(g) == bytes(g0)


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("n_extra,short", [(0, 0), (1, 1), (1, 0), (2, 1), (2, 0)])
def test_extra_entries_lie_inside_their_region(name, n_extra, short):
    """a region of exactly n_extra strides, or (short) one byte less: n_extra - 1 entries"""
    from lia_amd import _native as N
    case = CASES[name]
    entry, slack = case[4], N.LIA_CACHE_READ_SLACK
    stride = (entry + slack + 255) // 256 * 256
    extra = n_extra * stride - short
    rc0, g0 = plan(case)
    rc, g = plan(case, extra)
    assert rc == rc0
    if rc != OK:
        assert g.n_entries == 0 and g.entry_stride == 0 and g.in_extra == 0
        return
    # the first three regions never move
    assert (g.in_slots, g.in_staging, g.in_workspace, g.entry_stride, g.landing_stride, g.landing_capacity) == \
           (g0.in_slots, g0.in_staging, g0.in_workspace, g0.entry_stride, g0.landing_stride, g0.landing_capacity)
    assert list(g.offset[:g0.n_entries]) == list(g0.offset[:g0.n_entries])
    # a geometry with nothing to offer (two slots, no staging) offers no extra entry either; never more than 64 in all
    want = (n_extra - short) if g0.entry_stride else 0
    want = max(0, min(want, N.LIA_CACHE_MAX_ENTRIES - g0.n_entries))
    assert g.in_extra == want and g.n_entries == g0.n_entries + want
    spans = []
    for e in range(g0.n_entries, g.n_entries):
        at, end = g.offset[e], g.offset[e] + entry + slack
        assert at % 256 == 0 and end <= extra, (e, at, end, extra)
        assert all(end <= a or b <= at for a, b in spans), f"extra entry {e} overlaps another"
        spans.append((at, end))


def test_the_headline_gains_two_entries():
    """OPT-30B, B 64, 256 in / 32 out, gpu% 10: four resident layers of 1 233 315 072 bytes held as 815 894 255 encoded bytes + 4096
    of read slack each; what they save holds two more entries: 3 + 4 + 4 + 2 = 13"""
    from lia_amd import _native as N
    from lia_amd.model import resolve_shape
    lib = N.lib()
    sh = resolve_shape("opt-30b")
    slot, entry = 1233315072, 815894255
    staging = lib.lia_pack10_bound((slot // 2 + 1023) // 1024 * 1024)
    desc = N.LayerDesc(sh.hidden, sh.heads, sh.ffn, 1e-5)
    lm_bytes = 2 * 256 * sh.hidden + 8 * 64 * sh.vocab * 4 + (1 << 20)                 # planner.wire_cache_layers, B = 64, T = 256
    ws = max(lib.lia_layer_workspace_bytes(ctypes.byref(desc), 64 * 256), lm_bytes)
    lend_at = (max(lib.lia_layer_workspace_bytes(ctypes.byref(desc), 64), lm_bytes) + 255) // 256 * 256
    extra = 4 * (slot - 815898351)
    g = N.CacheGeometry()
    assert lib.lia_cache_geometry_plan_extra(4, slot, staging, 2, entry, entry, lend_at, ws - lend_at, extra, ctypes.byref(g)) == OK
    assert (g.in_slots, g.in_staging, g.in_workspace, g.in_extra) == (3, 4, 4, 2) and g.n_entries == 13
    assert g.entry_stride == 815898368 and 2 * g.entry_stride <= extra < 3 * g.entry_stride
    # three residents save 1.5 entries, five 2.5
    for n_res, want in ((0, 0), (1, 0), (2, 1), (3, 1), (5, 2), (6, 3)):
        assert lib.lia_cache_geometry_plan_extra(4, slot, staging, 2, entry, entry, lend_at, ws - lend_at, n_res * (slot - 815898351), ctypes.byref(g)) == OK
        assert g.in_extra == want and g.n_entries == 11 + want


def test_the_planner_counts_the_extra_region():
    from lia_amd import planner
    from lia_amd.model import resolve_shape
    sh = resolve_shape("opt-30b")
    box = planner.Box(host_threads=16, host_mem_gb=280.0, wire_ratio=10.585 / 16, wire_cache=True, wire_cache_ws=True)
    assert not box.resident_packed
    assert planner.wire_cache_layers(sh, box, 44, B=64, T=256, n_res=4) == 11          # not without the switch
    pre11, dec11, hbm11, *_ = planner.estimate(sh, 64, 256, 32, 10, 2, box)
    box.resident_packed = True
    assert planner.wire_cache_layers(sh, box, 44, B=64, T=256) == 11                   # no resident layer stated
    assert planner.wire_cache_layers(sh, box, 44, B=64, T=256, n_res=4) == 13
    assert planner.wire_cache_layers(sh, box, 12, B=64, T=256, n_res=4) == 12          # never more than stream
    pre13, dec13, hbm13, *_ = planner.estimate(sh, 64, 256, 32, 10, 2, box)
    assert pre13 == pre11 and hbm13 == hbm11 and dec13 < dec11
    # two layers' copies less (14.5 ms each at the box's link rate), four resident decodes more
    assert 20.0 < dec11 - dec13 < 29.0


def test_the_sweep_program_is_clean_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the library's host code; it must be here"
    exe = str(tmp_path / "cache_geometry_extra_sweep")
    subprocess.run([cxx, "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "cache_geometry_extra_sweep.cpp"),
                    os.path.join(ROOT, "isca-2025-lia_amd", "csrc", "lia_cache_geometry.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert out.splitlines()[-1] == "all cases hold" and "FAILED" not in out
    assert len([line for line in out.splitlines() if line.startswith("ok ")]) == 11 * 6
