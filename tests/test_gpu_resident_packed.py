"""HBM-resident layers held in the pack10 wire format (OffloadScheduler(resident_packed=), LIA_RESIDENT_PACKED;
LayerStore.to_device(packed=10), lia_stream_decode_device, lia_stream_cache_extra).

Through the C ABI, on one layer of hidden 128 / ffn 512:
  * lia_stream_decode_device leaves in the slot the bits lia_pack_decode gives, for both codecs, with the decode mode off (any slot)
    and on (a kept slot), copies nothing and counts its launches; it refuses an unknown format, a count that is no multiple of 1024
    or too large for a slot, and a slot outside the ring while the mode is on;
  * lia_stream_cache_extra adds entries behind the others (lia_stream_cache_layout), is refused while the mode is on, an entry
    there decodes to the same bits, and no mode change moves torch.cuda.mem_get_info().

Through generate(): the 12-layer model of tests/test_gpu_wire_cache_generate.py at gpu_percentage=25 -- three resident layers,
which save about 1.45 entries between them, so the extra region holds at least one (the test asks the geometry function with the
sizes the run had).  Packed residents only change where a resident layer's bits come from, so ids and last-step logits are
byte-identical to the run with resident_packed=False: policies 0 / 2 and 3 / 3, four and three slots, a second prompt, a
speculative run, a scoring pass, a generate behind it; a policy-1 call re-tiers the residents raw.  From the third step on exactly
the streamed layers without an entry cross the link; the capacity is not smaller and the free device memory not lower than with
raw residents."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEEP = 2
CFG = dict(hidden=128, heads=4, ffn=512, layers=12, vocab=512, max_pos=160)
B, T, NEW = 3, 96, 6
GPU_PCT, N_GPU = 25, 3
FORMATS = {"pack10": 10, "pack10a": 0x10A}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from lia_amd import _native as N, ops
    ctx = ops.Context(0, 1 << 20)
    yield torch, N, N.lib(), ctx
    ctx.close()


@pytest.fixture(scope="module")
def layer(gpu):
    """one layer of hidden 128 / ffn 512: codec -> (bf16 bits, device tensor of the encoding + read slack, pinned encoding, wire
    bytes, the bits lia_pack_decode gives); n values"""
    torch, N, L, ctx = gpu
    from lia_amd import ops
    _, layer_bytes = ops.pack_offsets(ops.make_desc(CFG["hidden"], CFG["heads"], CFG["ffn"]))
    n = layer_bytes // 2
    assert n % 1024 == 0
    w = (0.02 * torch.randn(n, generator=torch.Generator().manual_seed(77))).to(torch.bfloat16)
    bits = w.view(torch.int16).numpy().view(np.uint16).copy()
    src, out = w.cuda(), {}
    cap = L.lia_pack10_bound(n)
    for codec, fmt in FORMATS.items():
        enc = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        nb = ctypes.c_size_t(0)
        if codec == "pack10":
            rc = L.lia_pack10_encode(ctypes.c_void_p(src.data_ptr()), n, ctypes.c_void_p(enc.data_ptr()), cap, ctypes.byref(nb))
        else:
            rc = L.lia_pack10a_encode(ctypes.c_void_p(src.data_ptr()), n, ctypes.c_void_p(enc.data_ptr()), cap, 0, ctypes.byref(nb))
        torch.cuda.synchronize()
        assert rc == 0 and 0 < nb.value < 2 * n
        host = enc[:nb.value].cpu().pin_memory()
        validate = L.lia_pack10_validate if codec == "pack10" else L.lia_pack10a_validate
        assert validate(ctypes.c_void_p(host.data_ptr()), nb.value, n) == 0
        held = torch.zeros(nb.value + N.LIA_CACHE_READ_SLACK, dtype=torch.uint8, device="cuda")      # as LayerStore.to_device(packed=10) holds it
        held[:nb.value].copy_(enc[:nb.value])
        ref = torch.zeros(n, dtype=torch.int16, device="cuda")
        N.check(L.lia_pack_decode(ctypes.c_void_p(held.data_ptr()), ctypes.c_void_p(ref.data_ptr()), n, fmt, None), "lia_pack_decode")
        torch.cuda.synchronize()
        ref = ref.cpu().numpy().view(np.uint16).copy()
        assert np.array_equal(ref, bits)
        out[codec] = (bits, held, host, nb.value, ref)
    return out, n


def _slot_bits(gpu, h, slot, n):
    """the consumer: wait for the slot, read it back, release it"""
    torch, N, L, ctx = gpu
    stream = ctypes.c_void_p(ctx.stream)
    N.check(L.lia_stream_wait(h, slot, stream), "lia_stream_wait")
    ctx.synchronize()
    back = np.empty(n, np.uint16)
    N.check(L.lia_memcpy_d2h(back.ctypes.data, ctypes.c_void_p(L.lia_stream_slot_ptr(h, slot)), 2 * n), "lia_memcpy_d2h")
    N.check(L.lia_stream_release(h, slot, stream), "lia_stream_release")
    return back


def _counters(N, L, h):
    b, ms, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_long()
    N.check(L.lia_stream_stats(h, ctypes.byref(b), ctypes.byref(ms), 1), "lia_stream_stats")
    N.check(L.lia_stream_decode_stats(h, ctypes.byref(n), None, None, None, 1), "lia_stream_decode_stats")
    return int(b.value), n.value


@pytest.mark.parametrize("codec", list(FORMATS))
def test_decode_device_gives_the_bits_of_pack_decode(gpu, layer, codec):
    torch, N, L, ctx = gpu
    lay, n = layer
    bits, held, host, nb, ref = lay[codec]
    fmt, src = FORMATS[codec], ctypes.c_void_p(held.data_ptr())
    h = ctypes.c_void_p()
    N.check(L.lia_stream_create(ctx.handle, 4, 2 * n, ctypes.byref(h)), "lia_stream_create")
    try:
        # the mode off: any slot of the ring, twice into the same one (the second behind the first one's release)
        for slot in (3, 0, 3):
            N.check(L.lia_stream_decode_device(h, slot, src, nb, n, fmt), "lia_stream_decode_device")
            assert np.array_equal(_slot_bits(gpu, h, slot, n), ref), f"mode off, slot {slot}"
        assert _counters(N, L, h) == (0, 3)                                   # nothing copied, three launches
        # a legacy prefetch into a slot a device decode used, and back
        N.check(L.lia_stream_prefetch_packed(h, 3, ctypes.c_void_p(host.data_ptr()), nb, n, fmt, 1), "lia_stream_prefetch_packed")
        assert np.array_equal(_slot_bits(gpu, h, 3, n), ref)
        N.check(L.lia_stream_decode_device(h, 3, src, nb, n, fmt), "lia_stream_decode_device")
        assert np.array_equal(_slot_bits(gpu, h, 3, n), ref)
        assert _counters(N, L, h) == (nb, 2)
        # refusals
        assert L.lia_stream_decode_device(h, 0, src, nb, n, 11) != 0, "an unknown format"
        assert L.lia_stream_decode_device(h, 0, src, nb, n - 1, fmt) != 0, "n_values % 1024"
        assert L.lia_stream_decode_device(h, 0, src, nb, n + 1024, fmt) != 0, "n_values * 2 > slot_bytes"
        assert L.lia_stream_decode_device(h, 4, src, nb, n, fmt) != 0 and L.lia_stream_decode_device(h, 0, None, nb, n, fmt) != 0
        # the mode on: kept slots only
        assert L.lia_stream_cache_capacity(h, KEEP, nb) > 0
        N.check(L.lia_stream_cache_enable(h, KEEP, nb), "lia_stream_cache_enable")
        assert L.lia_stream_decode_device(h, KEEP, src, nb, n, fmt) != 0, "a slot that holds cached layers"
        for slot in (0, 1, 0):
            N.check(L.lia_stream_decode_device(h, slot, src, nb, n, fmt), "lia_stream_decode_device")
            assert np.array_equal(_slot_bits(gpu, h, slot, n), ref), f"mode on, slot {slot}"
        # beside a cached layer: entry 0 filled from the host, decoded into the other kept slot
        N.check(L.lia_stream_decode_cached(h, 0, 1, ctypes.c_void_p(host.data_ptr()), nb, n, fmt, 1), "lia_stream_decode_cached")
        N.check(L.lia_stream_decode_device(h, 0, src, nb, n, fmt), "lia_stream_decode_device")
        assert np.array_equal(_slot_bits(gpu, h, 1, n), ref) and np.array_equal(_slot_bits(gpu, h, 0, n), ref)
        assert _counters(N, L, h) == (nb, 5)
        N.check(L.lia_stream_cache_disable(h), "lia_stream_cache_disable")
        N.check(L.lia_stream_decode_device(h, 2, src, nb, n, fmt), "lia_stream_decode_device")
        assert np.array_equal(_slot_bits(gpu, h, 2, n), ref), "mode off again"
    finally:
        L.lia_stream_destroy(h)


def test_the_extra_region_holds_entries_and_no_mode_change_allocates(gpu, layer):
    torch, N, L, ctx = gpu
    lay, n = layer
    bits, held, host, nb, ref = lay["pack10a"]
    fmt = FORMATS["pack10a"]
    h = ctypes.c_void_p()
    N.check(L.lia_stream_create(ctx.handle, 4, 2 * n, ctypes.byref(h)), "lia_stream_create")
    try:
        N.check(L.lia_stream_decode_device(h, 0, ctypes.c_void_p(held.data_ptr()), nb, n, fmt), "lia_stream_decode_device")   # (staging areas: allocated)
        assert np.array_equal(_slot_bits(gpu, h, 0, n), ref) and _counters(N, L, h) == (0, 1)
        C0 = L.lia_stream_cache_capacity(h, KEEP, nb)
        stride = (nb + N.LIA_CACHE_READ_SLACK + 255) // 256 * 256
        assert C0 > 0
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        N.check(L.lia_stream_cache_extra(h, 2 * stride + 100), "lia_stream_cache_extra")
        free1 = torch.cuda.mem_get_info()[0]                                   # (an allocation this small may come out of a block the driver holds already)
        assert free1 <= free0
        g = N.CacheGeometry()
        N.check(L.lia_stream_cache_layout(h, KEEP, nb, ctypes.byref(g)), "lia_stream_cache_layout")
        assert g.in_extra == 2 and g.n_entries == C0 + 2 == L.lia_stream_cache_capacity(h, KEEP, nb)
        assert list(g.offset[C0:C0 + 2]) == [0, stride]
        for _ in range(2):
            N.check(L.lia_stream_cache_enable(h, KEEP, nb), "lia_stream_cache_enable")
            assert L.lia_stream_cache_extra(h, stride) != 0 and L.lia_stream_cache_extra(h, 0) != 0, "refused while the mode is on"
            # the last entry lies in the extra region: filled over the link once, decoded twice
            for slot in (0, 1):
                N.check(L.lia_stream_decode_cached(h, C0 + 1, slot, ctypes.c_void_p(host.data_ptr()), nb, n, fmt, 1), "lia_stream_decode_cached")
                assert np.array_equal(_slot_bits(gpu, h, slot, n), ref), "an entry in the extra region"
            assert _counters(N, L, h) == (nb, 2)
            N.check(L.lia_stream_cache_disable(h), "lia_stream_cache_disable")
            torch.cuda.synchronize()
            assert torch.cuda.mem_get_info()[0] == free1, "a mode change moved device memory"
        N.check(L.lia_stream_cache_extra(h, stride - 1), "lia_stream_cache_extra")            # a byte short of an entry
        assert L.lia_stream_cache_capacity(h, KEEP, nb) == C0
        N.check(L.lia_stream_cache_extra(h, 0), "lia_stream_cache_extra")
        torch.cuda.synchronize()
        assert L.lia_stream_cache_capacity(h, KEEP, nb) == C0 and free1 <= torch.cuda.mem_get_info()[0] <= free0
    finally:
        L.lia_stream_destroy(h)


# -- generate() ----------------------------------------------------------------------------------------
def _ids(seed, shape):
    return np.random.RandomState(seed).randint(3, CFG["vocab"], shape).astype(np.int64)


@pytest.fixture(scope="module")
def model(gpu):
    from lia_amd.model import LiaOPTModel, OPTShape
    shape = OPTShape("resident-packed", CFG["hidden"], CFG["heads"], CFG["ffn"], CFG["layers"], vocab=CFG["vocab"], max_pos=CFG["max_pos"])
    m = LiaOPTModel.random_init(shape, seed=11, n_gpu_layers=N_GPU)
    yield m
    if getattr(m, "_lia_scheduler", None) is not None:
        m._lia_scheduler.close()
    m.close()


def _scenario(model, resident_packed, policies, n_slots):
    import torch
    from lia_amd.generation import generate
    from lia_amd.scheduler import OffloadScheduler
    from lia_amd.scoring import score
    from lia_amd.speculative import ReplayDrafter
    if getattr(model, "_lia_scheduler", None) is not None:
        model._lia_scheduler.close()
    flags = dict(prefill_policy=policies[0], decoding_policy=policies[1], gpu_percentage=GPU_PCT, pin_weight=True)
    # Every scenario starts from the same placement, all layers on the host in the wire format, and an emptied allocator cache: its
    # first forward brings the residents to the device, raw or packed, into the same free memory.  (What the residents save is less
    # than one 2 MiB segment of torch's allocator here, so runs whose residents were allocated at different points of the process's
    # history would differ by where their tensors happened to land, not by what they hold.)
    model.place(0, True, False, 10)
    torch.cuda.empty_cache()
    sched = model._lia_scheduler = OffloadScheduler(model, wire="pack10", n_slots=n_slots, wire_cache=True, wire_cache_ws=True,
                                                    resident_packed=resident_packed)
    out, facts, per_step = {}, {}, []
    prompt, prompt2 = torch.from_numpy(_ids(1, (B, T))), torch.from_numpy(_ids(2, (B, T)))

    def hook(step):
        per_step.append(sched.stream_stats(reset=True)[0])            # bytes copied since the hook before
        if step == 2:
            facts["info"] = sched.wire_cache_info(regions=True)
            facts["launches"] = sched.decode_stats(reset=True)["launches"]
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            facts["free"] = torch.cuda.mem_get_info()[0]
        if step == 3:
            facts["launches_per_step"] = sched.decode_stats(reset=True)["launches"]

    try:
        ids, _, logits = generate(model, prompt, max_new_tokens=NEW, eos_token_id=None, return_logits=True, step_hook=hook, **flags)
        out["first"] = (ids.clone(), logits[-1].cpu())
        facts["per_step"] = list(per_step)
        facts["residents"] = [(st.tier, int(st.packed), int(st.codec), int(st.stream_bytes), int(st._dev.numel())) for st in model.layers[:N_GPU]]
        facts["nbytes"], facts["slot"] = int(model.layers[0].nbytes), int(model.layer_bytes)
        facts["wire"] = {i: int(model.layers[i].stream_bytes) for i in range(N_GPU, CFG["layers"])}
        facts["cfg"], facts["ws"] = sched.pipe._cfg, sched.ctx.workspace_alloc_bytes
        ids, _, logits = generate(model, prompt2, max_new_tokens=NEW, eos_token_id=None, return_logits=True, **flags)
        out["second"] = (ids.clone(), logits[-1].cpu())
        log = []
        ids = generate(model, prompt, max_new_tokens=NEW, eos_token_id=None, draft=ReplayDrafter(out["first"][0], corrupt=[None, [2, 1, 2]]),
                       draft_tokens=2, spec_log=log, **flags)
        out["speculative"] = (ids.clone(), torch.zeros(1))
        facts["rounds"], facts["on_after_speculative"] = len(log), sched.wire_cache_info()["on"]
        lp, greedy, _ = score(model, prompt2[:, :12], **flags)
        out["score"] = (greedy.clone(), lp)
        ids, _, logits = generate(model, prompt, max_new_tokens=NEW, eos_token_id=None, return_logits=True, **flags)
        out["back"] = (ids.clone(), logits[-1].cpu())
        facts["packed_before_policy_1"] = [int(st.packed) for st in model.layers[:N_GPU]]
        # policy 1: the resident prefix runs from raw pointers, the placement re-tiers the residents raw
        ids = generate(model, prompt[:, :16], max_new_tokens=3, eos_token_id=None, prefill_policy=1, decoding_policy=1, gpu_percentage=GPU_PCT,
                       pin_weight=True)
        out["policy 1"] = (ids.clone(), torch.zeros(1))
        facts["after_policy_1"] = [(st.tier, int(st.packed), int(st._dev.numel())) for st in model.layers[:N_GPU]]
        facts["extra_after_policy_1"] = sched.pipe._extra if sched.pipe is not None else 0
        ids, _, logits = generate(model, prompt, max_new_tokens=NEW, eos_token_id=None, return_logits=True, **flags)
        out["packed again"] = (ids.clone(), logits[-1].cpu())
    finally:
        sched.close()
        model._lia_scheduler = None
    return out, facts


@pytest.fixture(scope="module")
def runs(model):
    """(resident_packed, policies, n_slots) -> the scenario, once each; the run with raw residents first"""
    cache = {}

    def get(resident_packed, policies, n_slots):
        if not cache:
            # Two scenarios that are not compared, one of each kind.  The first ones of a process also load every code object and
            # fill the HIP runtime's own pools on the way: the first lia_stream_cache_extra of a process makes the runtime take one
            # 2 MiB block that it keeps when the region is freed and the streamer destroyed (every later scenario, with raw
            # residents too, finds 2 MiB less free: 308 327 481 344 against 308 329 578 496 bytes, measured twice), and what three
            # residents of this size save, 394 KB, is less than that block.  The footprint test compares runs with the same history.
            _scenario(model, False, (0, 2), 4)
            _scenario(model, True, (0, 2), 4)
        for rp in (False, True) if resident_packed else (False,):
            if (rp, policies, n_slots) not in cache:
                cache[(rp, policies, n_slots)] = _scenario(model, rp, policies, n_slots)
        return cache[(resident_packed, policies, n_slots)]
    return get


def _same(torch, got, ref, what):
    for name in ref:
        assert torch.equal(got[name][0], ref[name][0]), f"{name}: the ids differ {what}"
        a, b = got[name][1], ref[name][1]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), \
            f"{name}: the last step's logits differ {what}"


@pytest.mark.parametrize("policies,n_slots", [((0, 2), 4), ((3, 3), 4), ((0, 2), 3)])
def test_generate_is_the_same_with_packed_residents(gpu, model, runs, policies, n_slots):
    torch, N, lib, _ = gpu
    got, facts = runs(True, policies, n_slots)
    off, off_facts = runs(False, policies, n_slots)
    L, wire = CFG["layers"], facts["wire"]
    info, info0 = facts["info"], off_facts["info"]
    C, C0, regions = info["capacity"], info0["capacity"], info["regions"]
    print(f"\n{policies} {n_slots} slots: {info}; raw residents {info0}; bytes per step {facts['per_step']}; residents {facts['residents']}; "
          f"free {facts['free']} against {off_facts['free']}; decode launches per step {facts['launches_per_step']} against "
          f"{off_facts['launches_per_step']}")
    # the residents: packed, each in a tensor of exactly its encoding + the read slack; raw in the reference run
    for tier, packed, codec, stream_bytes, held in facts["residents"]:
        assert tier == "device" and packed == 10 and codec in (10, 0x10A) and held == stream_bytes + N.LIA_CACHE_READ_SLACK < facts["nbytes"]
    assert all(r[:2] == ("device", 0) and r[4] == facts["nbytes"] for r in off_facts["residents"])
    assert off_facts["wire"] == wire
    # they hold no entry and are never counted; the streamed layers bound are the first C
    assert info["on"] and info0["on"] and info0["regions"]["extra"] == 0
    assert info["layers"] == list(range(N_GPU, N_GPU + C)) and info["bytes"] == sum(wire[i] for i in info["layers"])
    assert C >= C0 and sum(regions.values()) >= C
    # the extra region: what the geometry function gives for the sizes this run had
    saved = sum(facts["nbytes"] - r[4] for r in facts["residents"])
    entry = max(wire[i] for i in info["layers"])
    g = N.CacheGeometry()
    staging = lib.lia_pack10_bound((facts["slot"] // 2 + 1023) // 1024 * 1024)
    landing, lend, keep = facts["cfg"]
    lend_at = (keep + 255) // 256 * 256
    assert lib.lia_cache_geometry_plan_extra(n_slots, facts["slot"], staging, KEEP, entry, landing, lend_at, facts["ws"] - lend_at if lend else 0,
                                             saved, ctypes.byref(g)) == 0
    assert regions == {"slots": g.in_slots, "staging": g.in_staging, "workspace": g.in_workspace, "extra": g.in_extra}
    if C < L - N_GPU:
        assert regions["extra"] >= 1 and C > C0, "three residents save more than one entry"
    # from the third step on exactly the streamed layers without an entry cross the link, and every layer is decoded once
    steady = sum(wire[i] for i in range(N_GPU + C, L))
    assert facts["per_step"][3:] == [steady] * (NEW - 3), (facts["per_step"], steady)
    assert off_facts["per_step"][3:] == [sum(wire[i] for i in range(N_GPU + C0, L))] * (NEW - 3)
    # (decode launches of one step, as lia_stream_decode_stats timed them: a launch into a slot whose last one is still in flight goes
    # uncounted, so these are upper bounds where the host runs ahead of the device)
    assert facts["launches_per_step"] <= L and off_facts["launches_per_step"] <= L - N_GPU
    assert facts["rounds"] >= 2 and facts["on_after_speculative"]
    # policy 1 re-tiered them raw (and the extra region went back); the next 0 / 2 call packed them again
    assert facts["packed_before_policy_1"] == [10] * N_GPU
    assert facts["after_policy_1"] == [("device", 0, facts["nbytes"])] * N_GPU and facts["extra_after_policy_1"] == 0
    _same(torch, got, off, "from the run with raw residents")
    _same(torch, {"back": got["back"], "packed again": got["packed again"]}, {"back": got["first"], "packed again": got["first"]},
          "between two generates of one scheduler")


def test_free_device_memory_is_not_lower_with_packed_residents(gpu, runs):
    """after torch.cuda.empty_cache(), torch.cuda.mem_get_info()[0] at the third decode step: what the residents save is the
    extra region, byte for byte, so the device holds no more than with raw residents.  Both runs start from the same placement and
    the same process history (_scenario, runs); measured 308 327 481 344 bytes free in both.  At the headline's sizes, where the
    saving is 1.67 GB, tools/free_hbm_at_first_step.py shows 265 149 218 816 bytes free against the 264 943 697 920 of raw residents."""
    _, facts = runs(True, (0, 2), 4)
    _, off_facts = runs(False, (0, 2), 4)
    print(f"\nfree at the third decode step: {facts['free']} with packed residents, {off_facts['free']} with raw ones "
          f"({facts['free'] - off_facts['free']:+d} bytes)")
    assert facts["free"] >= off_facts["free"], (facts["free"], off_facts["free"])
