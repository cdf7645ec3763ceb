"""The streamer's decode mode through the C ABI (lia_stream_cache_* / lia_stream_land / lia_stream_decode_landed /
lia_stream_decode_cached): wire-format layers cached in the slots that leave the ring.

  * every slot holds the raw bf16 bits of its layer exactly, on every step, in both codecs, for a layer that is no multiple of the
    rANS chunk and for one that is;
  * a cached layer crosses the link once: lia_stream_stats counts all 8 layers on the first step of a mode and exactly the 8 - C
    uncached ones afterwards (C from lia_stream_cache_capacity), lia_stream_decode_stats counts 8 launches on every step;
  * off -> a step over all slots -> on: contents stay exact and the first step refills;
  * two slots: capacity 0, the legacy path and its byte counts;
  * no mode change moves torch.cuda.mem_get_info()."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
KEEP = 2
LAYERS = 8
FORMATS = {"pack10": 10, "pack10a": 0x10A}
SIZES = {"67x1024": 67 * 1024, "4x65536": 4 * 65536}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from lia_amd import _native as N, ops
    ctx = ops.Context(0, 1 << 20)
    yield torch, N, N.lib(), ctx
    ctx.close()


@pytest.fixture(scope="module")
def layers(gpu):
    """(codec, size) -> [(bf16 bits, pinned encoded bytes, wire bytes)] x LAYERS, encoded once by the library's own encoders"""
    torch, N, L, ctx = gpu
    cache = {}

    def get(codec, size):
        if (codec, size) not in cache:
            n, out = SIZES[size], []
            gen = torch.Generator().manual_seed(1000 + n)
            for _ in range(LAYERS):
                w = (0.02 * torch.randn(n, generator=gen)).to(torch.bfloat16)
                src = w.cuda()
                cap = L.lia_pack10_bound(n)
                enc = torch.zeros(cap, dtype=torch.uint8, device="cuda")
                nb = ctypes.c_size_t(0)
                if codec == "pack10":
                    rc = L.lia_pack10_encode(ctypes.c_void_p(src.data_ptr()), n, ctypes.c_void_p(enc.data_ptr()), cap, ctypes.byref(nb))
                else:
                    rc = L.lia_pack10a_encode(ctypes.c_void_p(src.data_ptr()), n, ctypes.c_void_p(enc.data_ptr()), cap, 0, ctypes.byref(nb))
                torch.cuda.synchronize()
                assert rc == 0 and 0 < nb.value <= cap
                host = enc[:nb.value].cpu().pin_memory()
                validate = L.lia_pack10_validate if codec == "pack10" else L.lia_pack10a_validate
                assert validate(ctypes.c_void_p(host.data_ptr()), nb.value, n) == 0
                out.append((w.view(torch.int16).numpy().view(np.uint16).copy(), host, nb.value))
            cache[(codec, size)] = out
        return cache[(codec, size)]
    return get


class Streamer:
    def __init__(self, gpu, n_slots, n):
        self.torch, self.N, self.L, self.ctx = gpu
        self.n, self.n_slots = n, n_slots
        self.h = ctypes.c_void_p()
        self.N.check(self.L.lia_stream_create(self.ctx.handle, n_slots, 2 * n, ctypes.byref(self.h)), "lia_stream_create")
        self.stream = ctypes.c_void_p(self.ctx.stream)

    def close(self):
        self.L.lia_stream_destroy(self.h)

    def check_slot(self, slot, bits, what):
        """the consumer: wait for the slot, read it back, release it"""
        N, L = self.N, self.L
        N.check(L.lia_stream_wait(self.h, slot, self.stream), "lia_stream_wait")
        self.ctx.synchronize()
        back = np.empty(self.n, np.uint16)
        N.check(L.lia_memcpy_d2h(back.ctypes.data, ctypes.c_void_p(L.lia_stream_slot_ptr(self.h, slot)), 2 * self.n), "lia_memcpy_d2h")
        N.check(L.lia_stream_release(self.h, slot, self.stream), "lia_stream_release")
        assert np.array_equal(back, bits), f"{what}: {int((back != bits).sum())} of {self.n} values differ"

    def counters(self):
        """(wire bytes copied, decode launches) since the last call"""
        b, ms, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_long()
        self.N.check(self.L.lia_stream_stats(self.h, ctypes.byref(b), ctypes.byref(ms), 1), "lia_stream_stats")
        self.N.check(self.L.lia_stream_decode_stats(self.h, ctypes.byref(n), None, None, None, 1), "lia_stream_decode_stats")
        return int(b.value), n.value

    def legacy_step(self, lay, fmt, what):
        """every layer through lia_stream_prefetch_packed, one layer ahead, over all slots"""
        N, L, h = self.N, self.L, self.h

        def prefetch(i):
            N.check(L.lia_stream_prefetch_packed(h, i % self.n_slots, ctypes.c_void_p(lay[i][1].data_ptr()), lay[i][2], self.n, fmt, 1),
                    "lia_stream_prefetch_packed")
        prefetch(0)
        for i in range(LAYERS):
            if i + 1 < LAYERS and self.n_slots > 1:
                prefetch(i + 1)
            self.check_slot(i % self.n_slots, lay[i][0], f"{what} layer {i}")
            if i + 1 < LAYERS and self.n_slots == 1:
                prefetch(i + 1)

    def cached_step(self, lay, fmt, C, what):
        """decode mode: layers 0 .. C - 1 from their cache entries, the others through the two landing buffers with the link one
        layer ahead of the decodes; slots alternate"""
        N, L, h = self.N, self.L, self.h

        def land(i):
            if i < LAYERS:
                N.check(L.lia_stream_land(h, i % KEEP, ctypes.c_void_p(lay[i][1].data_ptr()), lay[i][2], 1), "lia_stream_land")
        land(C)
        land(C + 1)
        for i in range(LAYERS):
            slot = i % KEEP
            if i < C:
                N.check(L.lia_stream_decode_cached(h, i, slot, ctypes.c_void_p(lay[i][1].data_ptr()), lay[i][2], self.n, fmt, 1),
                        "lia_stream_decode_cached")
            else:
                N.check(L.lia_stream_decode_landed(h, i % KEEP, slot, self.n, fmt), "lia_stream_decode_landed")
                land(i + KEEP)             # into the buffer just read: the library orders the copy behind that decode
            self.check_slot(slot, lay[i][0], f"{what} layer {i}")


@pytest.mark.parametrize("n_slots", [4, 3])
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("codec", list(FORMATS))
def test_cached_layers_cross_the_link_once(gpu, layers, codec, size, n_slots):
    torch, N, L, ctx = gpu
    lay, fmt, n = layers(codec, size), FORMATS[codec], SIZES[size]
    wire = [nb for _, _, nb in lay]
    entry = max(wire)
    s = Streamer(gpu, n_slots, n)
    try:
        assert L.lia_stream_cache_capacity(s.h, KEEP, entry) == 0, "no staging yet (raw wire): nothing can be cached"
        assert L.lia_stream_cache_enable(s.h, KEEP, entry) != 0
        s.legacy_step(lay, fmt, "before the mode")                  # (allocates the staging areas, as a prefill does)
        assert s.counters() == (sum(wire), LAYERS)
        C = L.lia_stream_cache_capacity(s.h, KEEP, entry)
        assert 0 < C < LAYERS, C
        print(f"\n{codec} {size} n_slots={n_slots}: {entry} bytes per entry, capacity {C}")
        assert L.lia_stream_cache_capacity(s.h, n_slots, entry) == 0 and L.lia_stream_cache_capacity(s.h, KEEP, 0) == 0
        torch.cuda.synchronize()
        for cycle in range(2):
            # (read right around the call: the runtime's own pools may grow while copies and kernels are queued in between)
            mem = torch.cuda.mem_get_info()
            N.check(L.lia_stream_cache_enable(s.h, KEEP, entry), "lia_stream_cache_enable")
            assert torch.cuda.mem_get_info() == mem, "turning the mode on changed the free device memory"
            assert L.lia_stream_cache_enable(s.h, KEEP, entry) != 0                                       # it is on
            assert L.lia_stream_prefetch_packed(s.h, 0, ctypes.c_void_p(lay[0][1].data_ptr()), wire[0], n, fmt, 1) != 0
            assert L.lia_stream_decode_cached(s.h, C, 0, ctypes.c_void_p(lay[0][1].data_ptr()), wire[0], n, fmt, 1) != 0   # no such entry
            assert L.lia_stream_land(s.h, KEEP, ctypes.c_void_p(lay[0][1].data_ptr()), wire[0], 1) != 0         # no such landing buffer
            for step in range(3 if cycle == 0 else 2):
                s.cached_step(lay, fmt, C, f"cycle {cycle} step {step}")
                want = sum(wire) if step == 0 else sum(wire[C:])
                assert s.counters() == (want, LAYERS), (cycle, step)
            # an entry never changes its layer while the mode is on
            assert L.lia_stream_decode_cached(s.h, 0, 0, ctypes.c_void_p(lay[1][1].data_ptr()), wire[1], n, fmt, 1) != 0
            mem = torch.cuda.mem_get_info()
            N.check(L.lia_stream_cache_disable(s.h), "lia_stream_cache_disable")
            assert torch.cuda.mem_get_info() == mem, "turning the mode off changed the free device memory"
            assert L.lia_stream_land(s.h, 0, ctypes.c_void_p(lay[0][1].data_ptr()), wire[0], 1) != 0           # the mode is off
            s.legacy_step(lay, fmt, f"all slots after cycle {cycle}")
            assert s.counters() == (sum(wire), LAYERS)
    finally:
        s.close()


def test_two_slots_have_nothing_to_cache(gpu, layers):
    torch, N, L, ctx = gpu
    lay, fmt, n = layers("pack10a", "67x1024"), FORMATS["pack10a"], SIZES["67x1024"]
    wire = [nb for _, _, nb in lay]
    s = Streamer(gpu, 2, n)
    try:
        for step in range(2):
            s.legacy_step(lay, fmt, f"step {step}")
            assert s.counters() == (sum(wire), LAYERS)
            assert L.lia_stream_cache_capacity(s.h, KEEP, max(wire)) == 0
            assert L.lia_stream_cache_enable(s.h, KEEP, max(wire)) != 0
    finally:
        s.close()
