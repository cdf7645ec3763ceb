"""CPU tests of the host-side logic added around the hot path: NUMA pinning / cgroup guards (hostinfo), the slices of the
all-gather weight stream, the host-computed layer set of the cooperative split, the data-parallel stream mode switch."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "isca-2025-lia_amd"))


def test_pin_to_node_narrows_affinity_and_is_harmless_when_unknown():
    from lia_amd import hostinfo
    before = os.sched_getaffinity(0)
    try:
        cpus = hostinfo.node_cpus(0)
        if cpus:
            n = hostinfo.pin_to_node(0)
            assert n == len(before & cpus) and os.sched_getaffinity(0) == (before & cpus)
        assert hostinfo.pin_to_node(987) == 0                    # no such node: nothing changes, no exception
        assert hostinfo.node_cpus(987) is None
    finally:
        os.sched_setaffinity(0, before)
    assert hostinfo.gpu_numa_node(0) in (-1, 0, 1, 2, 3)        # -1 without a GPU


def test_cgroup_guards():
    from lia_amd import hostinfo
    m = hostinfo.cgroup_memory()
    assert set(m) == {"current", "peak", "max"}
    hostinfo.guard_host_allocation(1 << 20, "one MiB")           # always fits
    if m["max"] is not None:
        with pytest.raises(MemoryError):
            hostinfo.guard_host_allocation(m["max"], "the whole limit again")
    thr = hostinfo.cgroup_cpu_throttle()
    assert len(thr) == 2 and thr[0] >= 0 and thr[1] >= 0
    assert hostinfo.default_host_threads(8) >= 1 and hostinfo.default_host_threads(1) >= hostinfo.default_host_threads(8)


def test_minibatch_bounds_cover_every_row_once():
    """the ragged prefill split (scheduler.minibatch_bounds): the reference's own script lines that lia/modeling_opt.py:1178's
    int(bsz / num_minibatch) mishandles -- 1150 / 3 (cxl_offloading.sh:37), 1 / 2 (lia_offline.sh:27-29) -- and the property"""
    from lia_amd.scheduler import minibatch_bounds
    assert minibatch_bounds(1150, 3) == [(0, 383), (383, 383), (766, 384)]
    assert minibatch_bounds(1, 2) == [(0, 1)]
    assert minibatch_bounds(64, 2) == [(0, 32), (32, 32)] and minibatch_bounds(64, 1) == [(0, 64)]
    assert minibatch_bounds(1580, 4) == [(0, 395), (395, 395), (790, 395), (1185, 395)]
    for B in (1, 2, 3, 7, 64, 900, 1150):
        for mb in (1, 2, 3, 4, 8, 2000):
            b = minibatch_bounds(B, mb)
            assert len(b) == min(B, mb) and b[0][0] == 0 and sum(n for _, n in b) == B and all(n >= 1 for _, n in b)
            assert all(b[i][0] + b[i][1] == b[i + 1][0] for i in range(len(b) - 1))
            assert all(n == B // min(B, mb) for _, n in b[:-1])          # the reference's mini_bsz for every full minibatch


def test_allgather_slices_cover_the_wire_bytes():
    from lia_amd.model import LayerStore
    for total in (1, 255, 256, 832_000_123, 1_233_315_840):
        for world in (1, 2, 4, 8):
            sh = LayerStore.shard_bytes(total, world)
            assert sh % 256 == 0 and sh * world >= total and sh * (world - 1) < total + 256 * world
    # a raw OPT-30B packed layer (2048-aligned) splits exactly for 2 / 4 / 8 ranks: the slot has no room for padding
    assert all(LayerStore.shard_bytes(1_233_315_840, g) * g == 1_233_315_840 for g in (2, 4, 8))


def test_cpu_layer_set_properties():
    from lia_amd.scheduler import OffloadScheduler as S
    for n_gpu, L in ((4, 48), (0, 12), (3, 64), (9, 96)):
        for c in (0, 1, 5, 11, 16, 200):
            s = S.cpu_layer_set(n_gpu, L, c)
            assert len(s) == min(max(c, 0), L - n_gpu - 1)
            assert all(n_gpu < i < L for i in s)                 # never a resident layer, never the first streamed one
    s = sorted(S.cpu_layer_set(4, 48, 11))
    gaps = [b - a for a, b in zip(s, s[1:])]
    assert max(gaps) - min(gaps) <= 1                            # evenly spread


def test_dp_stream_mode_switch(monkeypatch):
    from lia_amd import dp
    monkeypatch.delenv("LIA_DP_STREAM", raising=False)
    assert dp.DataParallelGroup(None, 0, 2).mode == "broadcast"
    monkeypatch.setenv("LIA_DP_STREAM", "AllGather")
    assert dp.DataParallelGroup(None, 1, 2).mode == "allgather"
    monkeypatch.setenv("LIA_DP_STREAM", "ring")
    with pytest.raises(ValueError):
        dp.DataParallelGroup(None, 0, 2)


def test_rank_core_slices_do_not_overlap():
    from lia_amd import dp
    before = os.sched_getaffinity(0)
    try:
        seen = []
        for r in range(2):
            os.sched_setaffinity(0, before)
            g = dp.DataParallelGroup(None, r, 2, local_rank=r)
            n = g.pin_host_threads()
            cores = os.sched_getaffinity(0)
            assert n == len(cores) >= 1 and cores <= before
            seen.append(cores)
        if len(before) >= 4:
            assert not (seen[0] & seen[1])
    finally:
        os.sched_setaffinity(0, before)


class _FakeScheduler:
    """stands in for OffloadScheduler / LlamaScheduler in the greedy loop: next id = (last id + 1) mod vocab, EOS at a chosen step"""

    def __init__(self, vocab, eos_at=None):
        self.vocab, self.eos_at, self.calls, self.kw = vocab, eos_at, [], None

    def forward(self, ids, kv, max_new_tokens=None, suppress_token=-1, **lia):
        import torch
        self.calls.append((tuple(ids.shape), suppress_token))
        self.kw = lia
        nxt = (ids[:, -1] + 1) % self.vocab
        if self.eos_at is not None and len(self.calls) == self.eos_at and suppress_token < 0:
            nxt = torch.full_like(nxt, 2)
        return torch.zeros((ids.shape[0], self.vocab)), nxt


def _fake_model(sched, layers=4, max_pos=64):
    import types
    shape = types.SimpleNamespace(layers=layers, max_pos=max_pos, hidden=8, heads=2, head_dim=4)
    m = types.SimpleNamespace(shape=shape, family="llama", _lia_scheduler=sched)      # "llama": a KV state without host allocations
    return m


def test_greedy_loop_protocol_hooks_and_eos(monkeypatch):
    """generate(): latency_list has one entry per greedy iteration ([0] = the prefill), min_new_tokens suppresses EOS, the LIA
    kwargs reach forward() with the reference's defaults, step_hook(i) runs before iteration i and max_steps ends the loop
    early (what bench.py's bracket and warm-up are built on)."""
    import torch
    from lia_amd import generation, llama
    monkeypatch.setattr(llama, "LlamaKVState", lambda model, B, smax: object())
    ids = torch.tensor([[2, 5, 7], [2, 5, 7]])
    s = _FakeScheduler(50)
    seen = []
    out, lat = generation.generate(_fake_model(s), ids, max_new_tokens=6, min_new_tokens=6, token_latency=True, step_hook=seen.append,
                                   prefill_policy=0, decoding_policy=2, gpu_percentage=10, pin_weight=True)
    assert out.shape == (2, 9) and out[0].tolist() == [2, 5, 7, 8, 9, 10, 11, 12, 13] and len(lat) == 6 and seen == [0, 1, 2, 3, 4, 5]
    assert s.calls[0][0] == (2, 3) and all(c[0] == (2, 1) for c in s.calls[1:])            # prefill, then one token per step
    assert all(c[1] == 2 for c in s.calls)                                                   # EOS suppressed while min_new_tokens is unmet
    assert s.kw == dict(prefill_policy=0, decoding_policy=2, no_overlap=False, pin_weight=True, gpu_percentage=10, num_minibatch=1, enable_cxl=False)
    s = _FakeScheduler(50)
    out = generation.generate(_fake_model(s), ids, max_new_tokens=6, max_steps=3)
    assert out.shape == (2, 6) and len(s.calls) == 3
    assert s.kw["prefill_policy"] == 1 and s.kw["decoding_policy"] == 1 and s.kw["gpu_percentage"] == 0      # run.py defaults (IPEX baseline)
    s = _FakeScheduler(50, eos_at=2)                                                         # EOS at the second iteration ends the batch
    out = generation.generate(_fake_model(s), ids, max_new_tokens=6)
    assert out.shape == (2, 5) and out[0, -1] == 2
    with pytest.raises(ValueError):
        generation.generate(_fake_model(s), ids, max_new_tokens=6, num_beams=2)
    with pytest.raises(ValueError):
        generation.generate(_fake_model(s, max_pos=8), ids, max_new_tokens=6)


def test_planner_gpu_share_cap_and_model_shape_of_a_packed_directory(tmp_path):
    import json
    from lia_amd import packed_checkpoint as pc, planner, run_generation
    from lia_amd.model import resolve_shape
    shape = resolve_shape("opt-30b")
    box = planner.Box(host_threads=16, host_mem_gb=300.0)
    free = planner.plan(shape, 64, 256, 32, box)
    capped = planner.plan(shape, 64, 256, 32, box, max_gpu_percentage=10)
    assert free.gpu_percentage == 100 and capped.gpu_percentage <= 10 and capped.decode_tokens_per_s < free.decode_tokens_per_s
    d = tmp_path / "m"
    d.mkdir()
    assert not pc.is_packed_dir(str(d))
    json.dump({"format": pc.FORMAT, "family": "opt", "shape": {"name": "x", "hidden": 512, "heads": 4, "ffn": 2048, "layers": 3, "vocab": 100,
                                                                 "max_pos": 32}, "layers": []}, open(d / pc.MANIFEST, "w"))
    assert pc.is_packed_dir(str(d))
    args = run_generation.build_parser().parse_args(["-m", str(d)])
    sh = run_generation.model_shape(args)
    assert (sh.hidden, sh.heads, sh.ffn, sh.layers, sh.vocab, sh.max_pos) == (512, 4, 2048, 3, 100, 32)


def test_cap_torch_threads_only_lowers():
    """hostinfo.cap_torch_threads: torch's intra-op pool follows the cgroup quota / the caller's bound, never grows"""
    import torch
    from lia_amd import hostinfo
    before = torch.get_num_threads()
    try:
        assert hostinfo.cap_torch_threads(before + 7) == before           # a larger bound changes nothing
        got = hostinfo.cap_torch_threads(1)
        assert got == 1 and torch.get_num_threads() == 1
        assert hostinfo.cap_torch_threads(4) == 1                          # and it is never raised again
    finally:
        torch.set_num_threads(before)


def test_coop_controller_converges_on_a_synthetic_box():
    """the controller alone (no GPU work): step = max(link time of the streamed layers, host time) with 1 % noise"""
    import random
    from lia_amd.scheduler import CoopController, OffloadScheduler
    order = OffloadScheduler.cpu_layer_order(4, 48)
    assert len(order) == 43 and len(set(order)) == 43 and 4 not in order
    for k in (4, 8, 14):                                  # every prefix is spread: no two chosen layers adjacent while there is room
        assert min(b - a for a, b in zip(sorted(order[:k]), sorted(order[:k])[1:])) >= 2
    def box(c, host_ms=15.5):
        link, host = (44 - c) * 14.7, 110 + c * host_ms
        return max(link, host), link

    for start in (10, 14, 18, 22):
        random.seed(start)
        ctl = CoopController(order, start, start + 10)
        for _ in range(31):
            t, link = box(ctl.c)
            ms = t * (1 + random.uniform(-0.01, 0.01))
            ctl.observe(ms, min(1.0, link / ms))
        assert ctl.centre == 18 and ctl.report()["converged"], (start, ctl.report())  # argmin of max(link, host) for these rates
        assert ctl.converged_at <= 22, ctl.report()                                  # found inside one 32-token generation


def test_coop_controller_ignores_spikes_and_follows_the_box():
    """a shared box: every step has a 15 % chance of running 10 % long (another tenant on the host cores) -- the first version of
    the controller took such a step for the count's value and walked off the minimum (results/r03_final2_*).  Then the host
    slows down for good (15.5 -> 22 ms per host layer) and the controller has to find the new minimum by itself."""
    import random
    from lia_amd.scheduler import CoopController, OffloadScheduler
    order = OffloadScheduler.cpu_layer_order(4, 48)

    def step(c, host_ms):
        link, host = (44 - c) * 14.7, 110 + c * host_ms
        return max(link, host), link

    for seed in range(8):
        random.seed(100 + seed)
        ctl = CoopController(order, 15, 25)
        spent = []
        for i in range(120):
            t, link = step(ctl.c, 15.5)
            ms = t * (1 + random.uniform(-0.005, 0.005)) * (1.10 if random.random() < 0.15 else 1.0)
            spent.append(t)
            ctl.observe(ms, min(1.0, link / ms))
        assert step(ctl.centre, 15.5)[0] <= 1.025 * step(18, 15.5)[0], (seed, ctl.report())
        assert sum(spent[32:]) / len(spent[32:]) <= 1.03 * step(18, 15.5)[0], (seed, ctl.report())   # and it stays there: spikes move nothing
        for i in range(80):                                       # the box changes: best count is now 14 (441 vs 433 ... )
            t, link = step(ctl.c, 22.0)
            ctl.observe(t * (1 + random.uniform(-0.005, 0.005)), min(1.0, link / t))
        best = min(range(0, 26), key=lambda c: step(c, 22.0)[0])
        assert step(ctl.centre, 22.0)[0] <= 1.025 * step(best, 22.0)[0], (seed, best, ctl.report())
        assert ctl.searches >= 2


def test_coop_controller_on_a_bumpy_measured_landscape():
    """the step times of results/r03_final2 (fixed counts, one process each, on a noisy box: 17 host layers slower than 15 and
    19): whatever the bumps are, the search must end within 4 % of the best count and never below the seed's own time"""
    from lia_amd.scheduler import CoopController, OffloadScheduler
    order = OffloadScheduler.cpu_layer_order(4, 48)
    ms = {11: 500, 12: 474, 13: 456, 14: 444, 15: 432, 16: 440, 17: 461, 18: 430, 19: 417, 20: 428, 21: 446, 22: 470, 23: 490, 24: 505, 25: 520}
    ctl = CoopController(order, 15, 25)
    for _ in range(31):
        ctl.observe(ms[ctl.c], 1.0 if ctl.c < 19 else 0.9)
    assert ms[ctl.centre] <= 1.04 * min(ms.values()) and ms[ctl.centre] <= ms[15] and ctl.report()["converged"], ctl.report()


def test_coop_candidates_shrink_to_the_container(monkeypatch):
    """OPT-175B at gpu% = 5 in a 300 GiB container: the planner's count + 10 raw host copies do not fit; the candidate set is cut
    to a PREFIX of the nested order (still spread) before anything is placed, instead of a MemoryError halfway through"""
    from types import SimpleNamespace
    from lia_amd import hostinfo
    from lia_amd.scheduler import CoopController, OffloadScheduler
    GiB = 2**30
    L, n_gpu = 96, 4
    order = OffloadScheduler.cpu_layer_order(n_gpu, L)
    layers = [SimpleNamespace(nbytes=int(3.38 * GiB), stream_bytes=int(2.25 * GiB), packed=10, tier="cxl", raw_host_ptr=lambda: None) for _ in range(L)]
    me = SimpleNamespace(model=SimpleNamespace(layers=layers))
    monkeypatch.setattr(hostinfo, "cgroup_memory", lambda: {"current": int(244 * GiB), "peak": None, "max": int(300.1 * GiB)})
    ctl = CoopController(order, 40, 50)
    OffloadScheduler._fit_host_candidates(me, ctl, True)
    # 0.93 * 300.1 - 244 - 3.38 = 31.7 GiB of room, 1.13 GiB of growth per candidate (raw replaces packed in the tier)
    assert ctl.c_max == 28 and ctl.c == 28 and len(ctl.superset()) == 28 and ctl.superset() == frozenset(order[:28])
    ctl2 = CoopController(order, 10, 20)
    OffloadScheduler._fit_host_candidates(me, ctl2, True)
    assert ctl2.c_max == 20 and ctl2.c == 10                               # fits: untouched
    ctl3 = CoopController(order, 10, 20)
    OffloadScheduler._fit_host_candidates(me, ctl3, False)                 # pinned: raw + packed both stay, ceiling 0.85
    assert ctl3.c_max == int((0.85 * 300.1 - 244 - 3.38) // 3.38) == 2
    monkeypatch.setattr(hostinfo, "cgroup_memory", lambda: {"current": int(279 * GiB), "peak": None, "max": int(300.1 * GiB)})
    ctl0 = CoopController(order, 10, 20)
    with pytest.warns(RuntimeWarning, match="zero host-computed layers"):      # not even one copy fits: the plain streamed configuration
        OffloadScheduler._fit_host_candidates(me, ctl0, True)
    assert ctl0.c_max == 0 and ctl0.c == 0 and ctl0.host_set() == frozenset() and ctl0.superset() == frozenset()
    assert ctl0.observe(400.0, 1.0) == 0 and ctl0.observe(400.0, 1.0) == 0 and ctl0.observe(401.0, 1.0) == 0
    monkeypatch.setattr(hostinfo, "cgroup_memory", lambda: {"current": None, "peak": None, "max": None})
    ctl4 = CoopController(order, 40, 50)
    OffloadScheduler._fit_host_candidates(me, ctl4, True)                  # no cgroup limit readable: nothing to fit to
    assert ctl4.c_max == 50


def test_coop_controller_survives_restrict_at_any_point():
    """restrict() in the middle of a search (the raw copies of the upper candidates were lost on a re-placement): the search
    starts over from the clipped centre instead of comparing against a count that has no samples left"""
    import random
    from lia_amd.scheduler import CoopController, OffloadScheduler
    order = OffloadScheduler.cpu_layer_order(4, 48)

    def box(c):
        link, host = (44 - c) * 14.7, 110 + c * 15.5
        return max(link, host), link

    for seed in range(400):
        rnd = random.Random(seed)
        ctl = CoopController(order, rnd.randrange(8, 24), 30)
        for i in range(90):
            if rnd.random() < 0.08:
                ctl.restrict(rnd.randrange(0, 31))
            t, link = box(ctl.c)
            c = ctl.observe(t * (1 + rnd.uniform(-0.01, 0.01)), min(1.0, link / t))
            assert 0 <= c <= ctl.c_max and ctl.centre <= ctl.c_max
        rep = ctl.report()
        assert rep["host_layers"] <= rep["max_host_layers"]
    # a comparison against a centre whose samples are gone re-measures the centre first
    ctl = CoopController(order, 12, 22)
    for _ in range(4):
        t, link = box(ctl.c)
        ctl.observe(t, 1.0)
    assert ctl.c != ctl.centre
    ctl.samples.pop(ctl.centre)
    cand = ctl.c
    assert ctl.observe(box(cand)[0], 1.0) == cand                       # (the settle step after the move)
    assert ctl.observe(box(cand)[0], 1.0) == ctl.centre                 # the candidate's sample has nothing to be compared with yet
    ctl.observe(box(ctl.c)[0], 1.0)
    assert ctl.observe(box(ctl.c)[0], 1.0) == cand and ctl.value(ctl.centre) is not None   # centre measured: back to the candidate


def test_coop_controller_never_probes_upward_while_the_link_idles():
    """copy engine < 90 % busy = the host side is the bottleneck: counts above the centre are not tried (each such probe is a step
    at a slower count plus a cache move); and once a minimum has been bracketed the search moves by one count at a time"""
    from lia_amd.scheduler import CoopController, OffloadScheduler
    order = OffloadScheduler.cpu_layer_order(4, 48)
    ctl = CoopController(order, 20, 30)
    seen = []
    for _ in range(40):
        c = ctl.c
        seen.append(c)
        link, host = (44 - c) * 14.7, 110 + c * 15.5
        ctl.observe(max(link, host), min(1.0, link / max(link, host)) * 0.85)       # never above 0.85
    assert max(seen) == 20 and ctl.report()["converged"], (seen, ctl.report())
    # bracketed: after the first convergence every move is +-1
    ctl = CoopController(order, 12, 24)
    visited = []
    for i in range(200):
        c = ctl.c
        visited.append(c)
        host_ms = 15.5 if i < 60 else 22.0
        link, host = (44 - c) * 14.7, 110 + c * host_ms
        ctl.observe(max(link, host), min(1.0, link / max(link, host)))
        if ctl.bracketed and "first" not in locals():
            first = i
    after = visited[first + 1:]
    assert ctl.bracketed and all(abs(b - a) <= 2 for a, b in zip(after, after[1:])), (first, visited)   # centre-1 -> centre+1 is a jump of 2


def test_coop_store_seeds_the_next_process(tmp_path, monkeypatch):
    """the converged count is written next to the calibration (LIA_STATE_DIR) and the next controller for the same key starts ON
    it with +-1 probes: converged within a handful of steps"""
    from types import SimpleNamespace
    from lia_amd.scheduler import CoopController, CoopStore, OffloadScheduler
    monkeypatch.delenv("LIA_STATE_DIR", raising=False)
    assert CoopStore.path() is None and CoopStore.save("k", 1, 1.0) is False and CoopStore.load("k") is None    # nothing is kept unasked
    monkeypatch.setenv("LIA_STATE_DIR", str(tmp_path))
    assert CoopStore.load("k") is None and CoopStore.save(None, 3, 1.0) is False
    assert CoopStore.save("k", 18, 401.234) and CoopStore.load("k") == (18, 401.234)
    assert CoopStore.save("other", 3, 9.0) and CoopStore.load("k") == (18, 401.234) and CoopStore.load("other") == (3, 9.0)
    (tmp_path / CoopStore.FILE).write_text("{ not json")
    assert CoopStore.load("k") is None and CoopStore.save("k", 17, 400.0) and CoopStore.load("k") == (17, 400.0)   # a broken file is replaced

    def box(c):
        link, host = (44 - c) * 14.7, 110 + c * 15.5
        return max(link, host), link

    me = SimpleNamespace(model=SimpleNamespace(shape=SimpleNamespace(name="opt-x", hidden=7168, ffn=28672)), wire=10, host_threads=16,
                         _coop=None, _coop_key=None, cpu_layer_order=OffloadScheduler.cpu_layer_order)
    monkeypatch.setattr("lia_amd.planner.plan_cpu_layers", lambda *a, **k: (12, 0.0))
    ctl = OffloadScheduler._coop_controller(me, 4, 48, 64, 1, 32, 10, 3, None)
    assert ctl.c == 12 and not ctl.seeded
    n1 = 0
    while not ctl.report()["converged"]:
        t, link = box(ctl.c)
        ctl.observe(t, min(1.0, link / t))
        n1 += 1
    assert ctl.centre == 18 and CoopStore.load(ctl.store_key)[0] == 18
    me._coop = None                                                          # "the next process"
    ctl2 = OffloadScheduler._coop_controller(me, 4, 48, 64, 1, 32, 10, 3, None)
    assert ctl2.seeded and ctl2.c == 18 and ctl2.c_max == 28
    n2, seen = 0, []
    while not ctl2.report()["converged"]:
        seen.append(ctl2.c)
        t, link = box(ctl2.c)
        ctl2.observe(t, min(1.0, link / t))
        n2 += 1
    # starts ON the stored count; one stride-3 probe (a stored count that no longer fits is left quickly), then +-1
    assert ctl2.centre == 18 and n2 <= 12 and n2 < n1 and seen[0] == 18 and set(seen) <= {15, 17, 18, 19, 21}, (n1, n2, seen)
    # ... and a stored count that is WRONG for today's box (the optimum moved to 24) is left in strides, not one count at a time
    me._coop = None
    CoopStore.save(ctl2.store_key, 12, 400.0)

    def box24(c):
        link, host = (44 - c) * 14.7, 20 + c * 12.0
        return max(link, host), link

    ctl5 = OffloadScheduler._coop_controller(me, 4, 48, 64, 1, 32, 10, 3, None)
    assert ctl5.seeded and ctl5.c == 12
    n5 = 0
    while not ctl5.report()["converged"] and n5 < 80:
        t, link = box24(ctl5.c)
        ctl5.observe(t, min(1.0, link / t))
        n5 += 1
    best = min(range(0, ctl5.c_max + 1), key=lambda c: box24(c)[0])
    assert abs(ctl5.centre - best) <= 1 and n5 <= 30, (ctl5.centre, best, n5)
    CoopStore.save(ctl2.store_key, 18, 401.0)
    me._coop = None
    ctl3 = OffloadScheduler._coop_controller(me, 4, 48, 64, 1, 32, 10, 3, 9)   # an explicit start is taken as given
    assert ctl3.c == 9 and not ctl3.seeded
    me._coop = None
    ctl4 = OffloadScheduler._coop_controller(me, 4, 48, 32, 1, 32, 10, 3, None)  # another batch size: another key
    assert not ctl4.seeded and ctl4.c == 12
    me._coop = None
    ctl6 = OffloadScheduler._coop_controller(me, 4, 48, 64, 1024, 32, 10, 3, None)  # another prompt bucket: another key
    assert not ctl6.seeded
    me._coop = None
    ctl7 = OffloadScheduler._coop_controller(me, 4, 48, 64, 1, 128, 10, 3, None)   # more new tokens: another key
    assert not ctl7.seeded
    assert len({c.store_key for c in (ctl, ctl4, ctl6, ctl7)}) == 4


def test_bench_first_divergence_reports_step_and_gap():
    """bench.py's ids_check: legs are compared over their common length; the first divergent step and the top-2 logit gap there"""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("lia_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    T = 3
    a = torch.tensor([[1, 2, 3, 10, 11, 12, 13], [1, 2, 3, 10, 11, 12, 13]])
    b = torch.tensor([[1, 2, 3, 10, 11, 99], [1, 2, 3, 10, 11, 12]])            # shorter leg; row 0 parts at step 2
    logits = [torch.zeros((2, 8), dtype=torch.bfloat16) for _ in range(3)]
    logits[2][0, 5], logits[2][0, 6] = 8.0, 7.9375
    r = bench.first_divergence(a, b, T, logits)
    assert r["ids_equal"] is False and r["steps_compared"] == 3 and r["first_divergent_step"] == 2
    assert abs(r["top2_logit_gap_at_divergence"] - 0.0625) < 1e-6 and abs(r["bf16_quantum_at_top_logit"] - 0.0625) < 1e-9
    same = bench.first_divergence(a, a[:, :5], T)
    assert same == {"ids_equal": True, "steps_compared": 2, "first_divergent_step": None}


def test_bench_dump_outputs_dtypes_budget_and_sample(tmp_path):
    """bench.py --dump-outputs: integer outputs as float64, the rest as float32, every file within the budget; a larger output keeps a
    fixed, seeded sample of its rows (the same rows every run) and names them in <name>_rows.npy"""
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("lia_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    tokens = np.arange(4 * 9, dtype=np.int64).reshape(4, 9) + 50000
    logits = np.random.default_rng(1).standard_normal((4, 1000)).astype(np.float32)
    assert bench.dump_outputs(str(tmp_path / "all"), {"tokens": tokens, "logits": logits}) == {"tokens": [4, 9], "logits": [4, 1000]}
    t, lg = np.load(tmp_path / "all" / "tokens.npy"), np.load(tmp_path / "all" / "logits.npy")
    assert t.dtype == np.float64 and (t == tokens).all() and lg.dtype == np.float32 and (lg == logits).all()
    assert bench.DUMP_BUDGET_BYTES <= 64 * 2**20
    big = np.random.default_rng(2).standard_normal((64, 1000)).astype(np.float32)            # 256 kB against a 60 kB budget
    budget = 60_000
    shapes = [bench.dump_outputs(str(tmp_path / d), {"tokens": tokens, "logits": big}, budget=budget) for d in ("s1", "s2")]
    assert shapes[0] == shapes[1] and 1 <= shapes[0]["logits"][0] < 64 and shapes[0]["logits_rows"] == shapes[0]["logits"][:1]
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1")) <= budget + 3 * 128       # + the .npy headers
    rows = np.load(tmp_path / "s1" / "logits_rows.npy")
    assert rows.dtype == np.float64 and (np.diff(rows) > 0).all() and (rows == np.load(tmp_path / "s2" / "logits_rows.npy")).all()
    assert (np.load(tmp_path / "s1" / "logits.npy") == big[rows.astype(np.int64)]).all()


def test_bench_refuses_fewer_than_one_timed_step():
    """--steps is the number of timed decode steps and ms_per_step divides by it: 0 is refused before anything starts"""
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


def test_predicted_dp_table_names_what_binds_each_line():
    """planner.predict_dp (DESIGN.md section 6's table, bench.py's config.predicted): the broadcast stream is bound by the root's link at
    every N (throughput grows with the rows, the step does not move), the all-gather stream divides the link time by N until one
    xGMI ring or the host attention threads bind, and policy 0 / 2 pays the 16 / N host threads per rank."""
    from lia_amd import planner
    from lia_amd.model import resolve_shape
    sh = resolve_shape("opt-30b")
    box = planner.Box(host_threads=16, host_mem_gb=300.0)
    rows = planner.predict_dp_table(sh, 256, 32, 10, box)
    pick = lambda **kw: [r for r in rows if all(r[k] == v for k, v in kw.items())]          # noqa: E731
    assert len(rows) == 2 * (2 + 3 * 4)
    b33 = pick(scaling="weak", mode="broadcast", policies="3/3")
    assert [r["n_gpus"] for r in b33] == [1, 2, 4, 8] and len({r["ms_per_step"] for r in b33}) == 1 and all("link" in r["bound_by"] for r in b33)
    assert [round(r["tokens_per_s"] / b33[0]["tokens_per_s"]) for r in b33] == [1, 2, 4, 8]
    ag = pick(scaling="weak", mode="allgather", policies="3/3")
    assert ag[0]["ms_per_step"] < b33[0]["ms_per_step"] and ag[-1]["host_link_ms"] < ag[0]["host_link_ms"]
    assert "xGMI" in ag[-1]["bound_by"] and ag[-1]["ms_per_step_if_all_links"] < ag[-1]["ms_per_step"]
    h8 = pick(scaling="weak", n_gpus=8, mode="allgather", policies="0/2")[0]
    assert h8["host_attention_threads_per_rank"] == 2 and "host attention" in h8["bound_by"]
    strong = pick(scaling="strong", mode="broadcast", policies="3/3")
    assert [r["rows_per_gpu"] for r in strong] == [256, 128, 64, 32] and len({r["tokens_per_s"] for r in strong}) == 1   # link-bound: no gain from N


def test_placement_formats_per_policy_pair():
    """scheduler.placement_formats: which host copies a flag set keeps -- packed for the link, raw for the host cores"""
    from lia_amd.scheduler import placement_formats
    L, n_gpu = 48, 4
    streamed = frozenset(range(n_gpu, L))
    assert placement_formats(0, 2, 10, n_gpu, L, True, False) == (10, frozenset())                       # the headline: packed only
    assert placement_formats(0, 2, 10, n_gpu, L, True, False, {7, 9}) == (10, frozenset({7, 9}))          # + the cooperative split's candidates
    assert placement_formats(0, 1, 10, n_gpu, L, True, False) == (10, streamed)                            # README 0 / 1: both copies
    assert placement_formats(3, 1, 10, n_gpu, L, True, False)[1] == streamed
    assert placement_formats(0, 1, 10, n_gpu, L, True, True) == (0, frozenset())                           # the NUMA tier holds one (raw) copy
    assert placement_formats(0, 1, 10, n_gpu, L, False, False) == (0, frozenset())                         # unpinned: raw
    assert placement_formats(1, 1, 10, n_gpu, L, True, False) == (0, frozenset())                          # prefill on the host too: nothing streams
    assert placement_formats(0, 1, 0, n_gpu, L, True, False) == (0, frozenset())                           # --stream-format raw
    assert placement_formats(0, 1, 10, n_gpu, L, True, False, data_parallel=True) == (0, frozenset())
