"""The wire cache with its opt-in geometry through the C ABI (lia_stream_cache_configure): landing buffers cut to size and the
context's idle workspace lent to the mode.  Shapes of tests/test_gpu_stream_cache.py with 16 layers, so that C < LAYERS still holds.

  * configured, the pool holds more entries than before, some of them in the workspace (lia_stream_cache_layout);
  * every slot holds the raw bf16 bits of its layer exactly on each of three steps, and again after off -> legacy step -> on;
  * lia_stream_stats counts all layers on a mode's first step and exactly the uncached ones afterwards;
  * a byte pattern written to the kept part [0, keep) of the workspace before the mode is intact after three steps of it;
  * while lent, the context offers the kept part: a layer forward inside it gives the bits it gave before the mode, one that needs
    more is refused with LIA_ERR_MEMORY and the next cached step is still exact;
  * after disable, a forward that uses the whole workspace gives the bits it gave before the mode;
  * no mode change moves torch.cuda.mem_get_info(); all-zero configuration restores the old capacity."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
KEEP = 2
LAYERS = 16
FORMATS = {"pack10": 10, "pack10a": 0x10A}
SIZES = {"67x1024": 67 * 1024, "4x65536": 4 * 65536}
WS_KEEP = (1 << 20) + 3                     # rounded up to 256 by the library
WS_KEEP_ROUNDED = (1 << 20) + 256
H, HEADS, FFN = 128, 4, 512                 # the layer whose forwards use the workspace


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from lia_amd import _native as N, ops
    return torch, N, N.lib(), ops


@pytest.fixture(scope="module")
def layers(gpu):
    """(codec, size) -> [(bf16 bits, pinned encoded bytes, wire bytes)] x LAYERS, encoded once by the library's own encoders"""
    torch, N, L, ops = gpu
    cache = {}

    def get(codec, size):
        if (codec, size) not in cache:
            n, out = SIZES[size], []
            gen = torch.Generator().manual_seed(2000 + n)
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


@pytest.fixture(scope="module")
def layer(gpu):
    """one random OPT layer (H = 128) on the device and its inputs: forward(ctx, rows) -> the output's bits"""
    torch, N, L, ops = gpu
    desc = ops.make_desc(H, HEADS, FFN)
    offs, total = ops.pack_offsets(desc)
    gen = torch.Generator().manual_seed(77)
    flat = (0.05 * torch.randn(total // 2, generator=gen)).to(torch.bfloat16).cuda()
    wptrs = ops.weight_ptr_array(flat.data_ptr(), offs)
    xs = {}

    def forward(ctx, rows):
        if rows not in xs:
            xs[rows] = torch.randn((rows, 1, H), generator=gen).to(torch.bfloat16).cuda()
        x = xs[rows]
        y = torch.empty_like(x)
        kc = torch.zeros((2, rows, HEADS, H // HEADS), dtype=torch.bfloat16, device="cuda")
        vc = torch.zeros_like(kc)
        kv = N.KV(kc.data_ptr(), vc.data_ptr(), 2, rows, 1)
        ctx.layer_forward(desc, 3, wptrs, x, y, kv, rows, 1, 0)
        ctx.synchronize()
        return y.view(torch.int16).cpu().numpy().copy()

    forward.keep = flat
    forward.need = lambda rows: ops.workspace_bytes(desc, rows)
    return forward


class Streamer:
    def __init__(self, gpu, ctx, n_slots, n):
        self.torch, self.N, self.L, _ = gpu
        self.ctx, self.n, self.n_slots = ctx, n, n_slots
        self.h = ctypes.c_void_p()
        self.N.check(self.L.lia_stream_create(ctx.handle, n_slots, 2 * n, ctypes.byref(self.h)), "lia_stream_create")
        self.stream = ctypes.c_void_p(ctx.stream)

    def close(self):
        self.L.lia_stream_destroy(self.h)

    def check_slot(self, slot, bits, what):
        N, L = self.N, self.L
        N.check(L.lia_stream_wait(self.h, slot, self.stream), "lia_stream_wait")
        self.ctx.synchronize()
        back = np.empty(self.n, np.uint16)
        N.check(L.lia_memcpy_d2h(back.ctypes.data, ctypes.c_void_p(L.lia_stream_slot_ptr(self.h, slot)), 2 * self.n), "lia_memcpy_d2h")
        N.check(L.lia_stream_release(self.h, slot, self.stream), "lia_stream_release")
        assert np.array_equal(back, bits), f"{what}: {int((back != bits).sum())} of {self.n} values differ"

    def counters(self):
        b, ms, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_long()
        self.N.check(self.L.lia_stream_stats(self.h, ctypes.byref(b), ctypes.byref(ms), 1), "lia_stream_stats")
        self.N.check(self.L.lia_stream_decode_stats(self.h, ctypes.byref(n), None, None, None, 1), "lia_stream_decode_stats")
        return int(b.value), n.value

    def legacy_step(self, lay, fmt, what):
        N, L, h = self.N, self.L, self.h

        def prefetch(i):
            N.check(L.lia_stream_prefetch_packed(h, i % self.n_slots, ctypes.c_void_p(lay[i][1].data_ptr()), lay[i][2], self.n, fmt, 1),
                    "lia_stream_prefetch_packed")
        prefetch(0)
        for i in range(LAYERS):
            if i + 1 < LAYERS:
                prefetch(i + 1)
            self.check_slot(i % self.n_slots, lay[i][0], f"{what} layer {i}")

    def cached_step(self, lay, fmt, C, what):
        """layers 0 .. C - 1 from their entries, the others through the two landing buffers, the link one layer ahead of the decodes"""
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
                land(i + KEEP)
            self.check_slot(slot, lay[i][0], f"{what} layer {i}")


@pytest.mark.parametrize("n_slots", [4, 3])
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("codec", list(FORMATS))
def test_configured_pool_holds_more_and_stays_exact(gpu, layers, layer, codec, size, n_slots):
    torch, N, L, ops = gpu
    lay, fmt, n = layers(codec, size), FORMATS[codec], SIZES[size]
    wire = [nb for _, _, nb in lay]
    entry = max(wire)
    # a workspace of a few MB: the kept part and room for three entries and a half behind it
    stride = (entry + N.LIA_CACHE_READ_SLACK + 255) // 256 * 256
    alloc = WS_KEEP_ROUNDED + 3 * stride + stride // 2
    rows_all = max(r for r in range(1, 512) if layer.need(r) <= alloc)          # the largest forward the whole workspace takes
    rows_kept = max(r for r in range(1, 512) if layer.need(r) <= WS_KEEP_ROUNDED)
    assert rows_kept < rows_all and layer.need(rows_all) > WS_KEEP_ROUNDED
    ctx = ops.Context(0, alloc)
    s = Streamer(gpu, ctx, n_slots, n)
    ws = L.lia_ctx_workspace_ptr(ctx.handle)
    try:
        s.legacy_step(lay, fmt, "before the mode")                  # (allocates the staging areas, as a prefill does)
        assert s.counters() == (sum(wire), LAYERS)
        C0 = L.lia_stream_cache_capacity(s.h, KEEP, entry)
        N.check(L.lia_stream_cache_configure(s.h, entry, 1, WS_KEEP), "lia_stream_cache_configure")
        C = L.lia_stream_cache_capacity(s.h, KEEP, entry)
        g = N.CacheGeometry()
        N.check(L.lia_stream_cache_layout(s.h, KEEP, entry, ctypes.byref(g)), "lia_stream_cache_layout")
        print(f"\n{codec} {size} n_slots={n_slots}: {entry} bytes per entry, capacity {C0} -> {C} = {g.in_slots} + {g.in_staging} + {g.in_workspace}")
        assert 0 < C0 < C < LAYERS and g.n_entries == C and g.in_workspace == 3 and g.landing_capacity == entry
        assert all(WS_KEEP_ROUNDED <= g.offset[e] and g.offset[e] + entry + N.LIA_CACHE_READ_SLACK <= alloc for e in range(C - 3, C))
        # a landing buffer larger than a staging area is refused and changes nothing
        assert L.lia_stream_cache_configure(s.h, L.lia_pack10_bound(n), 1, WS_KEEP) != 0
        assert L.lia_stream_cache_capacity(s.h, KEEP, entry) == C
        before_kept, before_all = layer(ctx, rows_kept), layer(ctx, rows_all)
        # (the comparisons below rest on this: the same forward twice gives the same bits, whatever the calls in between left behind)
        assert np.array_equal(layer(ctx, rows_kept), before_kept) and np.array_equal(layer(ctx, rows_all), before_all)
        pattern = np.random.RandomState(5).randint(0, 256, WS_KEEP_ROUNDED).astype(np.uint8)
        N.check(L.lia_memcpy_h2d(ctypes.c_void_p(ws), pattern.ctypes.data, pattern.size), "lia_memcpy_h2d")
        torch.cuda.synchronize()
        for cycle in range(2):
            assert ctx.workspace_bytes == alloc
            mem = torch.cuda.mem_get_info()
            N.check(L.lia_stream_cache_enable(s.h, KEEP, entry), "lia_stream_cache_enable")
            assert torch.cuda.mem_get_info() == mem, "turning the mode on changed the free device memory"
            assert ctx.workspace_bytes == WS_KEEP_ROUNDED
            assert L.lia_stream_cache_configure(s.h, 0, 0, 0) != 0                                         # the mode is on
            assert L.lia_stream_land(s.h, 0, ctypes.c_void_p(lay[0][1].data_ptr()), entry + 1, 1) != 0     # larger than a landing buffer
            assert L.lia_stream_decode_cached(s.h, C, 0, ctypes.c_void_p(lay[0][1].data_ptr()), wire[0], n, fmt, 1) != 0   # no such entry
            for step in range(3 if cycle == 0 else 2):
                s.cached_step(lay, fmt, C, f"cycle {cycle} step {step}")
                want = sum(wire) if step == 0 else sum(wire[C:])
                assert s.counters() == (want, LAYERS), (cycle, step)
            if cycle == 0:
                back = np.empty_like(pattern)
                N.check(L.lia_memcpy_d2h(back.ctypes.data, ctypes.c_void_p(ws), back.size), "lia_memcpy_d2h")
                assert np.array_equal(back, pattern), "the mode wrote into the kept part of the workspace"
            # the context offers the kept part: a forward inside it is what it was, one beyond it is refused and harms nothing
            assert np.array_equal(layer(ctx, rows_kept), before_kept)
            with pytest.raises(MemoryError):
                layer(ctx, rows_all)
            s.cached_step(lay, fmt, C, f"cycle {cycle} after the refused forward")
            assert s.counters() == (sum(wire[C:]), LAYERS)
            mem = torch.cuda.mem_get_info()
            N.check(L.lia_stream_cache_disable(s.h), "lia_stream_cache_disable")
            assert torch.cuda.mem_get_info() == mem, "turning the mode off changed the free device memory"
            assert ctx.workspace_bytes == alloc
            # the whole workspace is the context's again, behind the mode's last decode
            after_all = layer(ctx, rows_all)
            print(f"cycle {cycle}: {int((after_all != before_all).sum())} of {after_all.size} values of the {rows_all}-row forward differ; "
                  f"again: {int((layer(ctx, rows_all) != before_all).sum())}")
            assert np.array_equal(after_all, before_all)
            s.legacy_step(lay, fmt, f"all slots after cycle {cycle}")
            assert s.counters() == (sum(wire), LAYERS)
        # all zero: the geometry without the call
        N.check(L.lia_stream_cache_configure(s.h, 0, 0, 0), "lia_stream_cache_configure")
        assert L.lia_stream_cache_capacity(s.h, KEEP, entry) == C0
        N.check(L.lia_stream_cache_enable(s.h, KEEP, entry), "lia_stream_cache_enable")
        assert ctx.workspace_bytes == alloc                                                                # nothing lent
        s.cached_step(lay, fmt, C0, "not configured")
        assert s.counters() == (sum(wire), LAYERS)
        s.cached_step(lay, fmt, C0, "not configured, second step")
        assert s.counters() == (sum(wire[C0:]), LAYERS)
        # destroying the streamer with the mode on hands the workspace back
        N.check(L.lia_stream_cache_disable(s.h), "lia_stream_cache_disable")
        N.check(L.lia_stream_cache_configure(s.h, entry, 1, WS_KEEP), "lia_stream_cache_configure")
        N.check(L.lia_stream_cache_enable(s.h, KEEP, entry), "lia_stream_cache_enable")
        assert ctx.workspace_bytes == WS_KEEP_ROUNDED
    finally:
        s.close()
        assert ctx.workspace_bytes == alloc
        ctx.close()
