"""The wire cache's configuration (WeightPipeline.configure_cache, OffloadScheduler._set_wire_cache / _ensure) over a fake library,
without a GPU: landing buffers cut to size and the context's idle workspace lent to the mode.

  * the configure call precedes enable, with the largest encoded size over ALL packed streamed layers as landing size (enable still
    gets the maximum over the bound ones);
  * a keep that grows turns the mode off, configures and turns it on again: the entries refill once;
  * the scheduler disables the mode before it replaces a context whose workspace may be lent;
  * without the call, the log is the one tests/test_wire_cache_host.py expects: no configure, the first `capacity` layers bound."""
import types

import pytest

KEEP = 2


class FakeLib:
    """keeps what the library keeps: the mode, the sticky configuration, which entry is filled, landing buffers and slots in use;
    the capacity follows the configuration: base entries, + 1 with landing buffers cut to size, + ws_entries while a workspace is lent"""

    def __init__(self, base, ws_entries=4, staging=8000):
        self.base, self.ws_entries, self.staging = base, ws_entries, staging
        self.on, self.log, self.cfg = False, [], (0, 0, 0)
        self.filled, self.landing, self.slots = {}, {}, {}

    def lia_stream_create(self, ctx, n, bytes_, out):
        self.n_slots = n
        out._obj.value = 0x51                                   # (a handle, so that close() reaches lia_stream_destroy)
        return 0

    def lia_stream_slot_ptr(self, h, s):
        return 0x1000 * (s + 1)

    def lia_stream_destroy(self, h):
        self.on = False
        self.log.append(("destroy",))

    def _take_slot(self, slot):
        assert self.slots.get(slot) != "held", f"slot {slot} refilled while its layer is in use"
        assert not self.on or slot < KEEP, f"slot {slot} holds cached layers"
        self.slots[slot] = "queued"

    def lia_stream_prefetch(self, h, slot, ptr, n, pinned):
        self._take_slot(slot)
        self.log.append(("copy", ptr.value, "raw"))
        return 0

    def lia_stream_prefetch_packed(self, h, slot, ptr, nbytes, n_values, fmt, pinned):
        assert not self.on, "the legacy packed path while the mode is on"
        self._take_slot(slot)
        self.log.append(("copy", ptr.value, "legacy"))
        return 0

    def lia_stream_wait(self, h, slot, st):
        assert self.slots.get(slot) == "queued", (slot, self.slots)
        self.slots[slot] = "held"
        return 0

    def lia_stream_release(self, h, slot, st):
        assert self.slots.pop(slot) == "held"
        return 0

    def _capacity(self):
        landing, lend, keep = self.cfg
        return self.base + (1 if landing else 0) + (self.ws_entries if lend else 0)

    def lia_stream_cache_configure(self, h, landing, lend, keep):
        if self.on or (landing and landing + 4096 > self.staging):
            return -1
        self.cfg = (landing, lend, keep if lend else 0)
        self.log.append(("configure", landing, lend, keep))
        return 0

    def lia_last_error(self):
        return b"fake: refused"

    def lia_stream_cache_capacity(self, h, keep, entry_bytes):
        return self._capacity() if self.n_slots > keep and entry_bytes else 0

    def lia_stream_cache_enable(self, h, keep, entry_bytes):
        assert not self.on and keep == KEEP and self._capacity()
        for slot in [s for s in self.slots if s >= keep]:
            assert self.slots[slot] == "queued"
            del self.slots[slot]
        self.on, self.filled, self.landing = True, {}, {}
        self.log.append(("enable", entry_bytes))
        return 0

    def lia_stream_cache_disable(self, h):
        if self.on:
            self.log.append(("disable",))
        self.on, self.filled, self.landing = False, {}, {}
        return 0

    def lia_stream_land(self, h, b, ptr, nbytes, pinned):
        assert self.on and 0 <= b < KEEP and b not in self.landing, (b, self.landing)
        assert not self.cfg[0] or nbytes <= self.cfg[0], "a layer larger than the configured landing buffers was landed"
        self.landing[b] = ptr.value
        self.log.append(("copy", ptr.value, "land"))
        return 0

    def lia_stream_decode_landed(self, h, b, slot, n_values, fmt):
        assert self.on and b in self.landing
        self._take_slot(slot)
        self.log.append(("decode", self.landing.pop(b)))
        return 0

    def lia_stream_decode_cached(self, h, entry, slot, ptr, nbytes, n_values, fmt, pinned):
        assert self.on and 0 <= entry < self._capacity()
        self._take_slot(slot)
        if entry not in self.filled:
            self.filled[entry] = ptr.value
            self.log.append(("copy", ptr.value, "fill"))
        assert self.filled[entry] == ptr.value, "an entry changed its layer while the mode was on"
        self.log.append(("decode", ptr.value))
        return 0


class Store:
    nbytes, tier, codec = 2048, "pinned", 0x10A

    def __init__(self, idx, packed=10, stream_bytes=1400):
        # sizes rise with the layer index: the largest layer is the last one, which is landed, never bound
        self.idx, self.packed, self.stream_bytes = idx, packed, stream_bytes + idx

    def host_ptr(self):
        return 0x9000 + self.idx

    def is_dma_able(self):
        return True


class Ctx:
    handle, stream = 1, 2

    def __init__(self, device=0, workspace_bytes=0):
        self.workspace_alloc_bytes, self.closed = workspace_bytes, False

    def set_host_threads(self, n):
        pass

    def close(self):
        self.closed = True


def make(monkeypatch, n_slots, base, L=12, raw=(), **kw):
    from lia_amd import streaming, _native
    fake = FakeLib(base, **kw)
    monkeypatch.setattr(_native, "lib", lambda: fake)

    class Model:
        layer_bytes = 2048
        offsets = list(range(16))
        layers = [Store(i, packed=0 if i in raw else 10) for i in range(L)]

    return streaming, fake, streaming.WeightPipeline(Ctx(), Model(), n_slots)


def forward(streaming, pipe, first, L, mode=True, before=None):
    """one forward's calls on the pipeline, as OffloadScheduler._run_layers makes them"""
    if before is not None:
        before()
    pipe.set_decode_mode(list(range(first, L)) if mode else None)
    pipe.prefetch(first)
    for idx in range(first, L):
        pipe.acquire(idx)
        pipe.prefetch_ahead(idx, streaming.stream_order(idx, first, L, frozenset(), skip_now=mode))
        assert len(pipe.landed) + len(pipe.free_landing) == pipe.keep
        assert len(pipe.free_slots) + len(pipe.inflight) + len(pipe.held) == (pipe.keep or pipe.n_slots)
        pipe.release(idx)


def fills(fake):
    return [e[1] - 0x9000 for e in fake.log if e[0] == "copy" and e[2] == "fill"]


def test_configure_precedes_enable_and_sizes_landing_for_every_streamed_layer(monkeypatch):
    streaming, fake, pipe = make(monkeypatch, 4, 3, raw={5})
    first, L = 2, 12
    forward(streaming, pipe, first, L, mode=False)
    del fake.log[:]
    for _ in range(3):
        forward(streaming, pipe, first, L, before=lambda: pipe.configure_cache(True, 1000))
    sizes = {i: st.stream_bytes for i, st in enumerate(pipe.model.layers)}
    landing = max(sizes[i] for i in range(L) if i != 5)               # every packed layer that is streamed, bound or not; not the raw one
    bound = [2, 3, 4, 6, 7, 8, 9, 10]                                  # 3 + 1 + 4 entries, the first packed layers of the order
    kinds = [e[0] for e in fake.log if e[0] in ("configure", "enable", "disable")]
    assert kinds == ["configure", "enable"], kinds
    assert fake.log[0] == ("configure", landing, 1, 1000)
    assert fake.log[1] == ("enable", max(sizes[i] for i in bound)) and fake.log[1][1] < landing
    assert sorted(pipe.cache) == bound and fills(fake) == bound       # each filled once over three steps
    assert pipe.cache_info()["capacity"] == 8


def test_a_growing_keep_reconfigures_and_refills_once(monkeypatch):
    streaming, fake, pipe = make(monkeypatch, 4, 3)
    first, L = 2, 12
    for keep in (1000, 1000, 900, 5000, 5000):                         # (the scheduler never passes a smaller keep; the same one is a no-op)
        forward(streaming, pipe, first, L, before=lambda: pipe.configure_cache(True, max(keep, pipe._cfg[2])))
    kinds = [(e[0],) + ((e[3],) if e[0] == "configure" else ()) for e in fake.log if e[0] in ("configure", "enable", "disable")]
    assert kinds == [("configure", 1000), ("enable",), ("disable",), ("configure", 5000), ("enable",)], kinds
    bound = list(range(first, first + 8))
    assert fills(fake) == bound * 2                                    # the first mode's fill and exactly one refill
    assert pipe.keep and sorted(pipe.cache) == bound


def test_lend_off_and_oversized_landing_fall_back(monkeypatch):
    streaming, fake, pipe = make(monkeypatch, 4, 3)
    forward(streaming, pipe, 2, 12, before=lambda: pipe.configure_cache(False, 777))
    assert fake.log[0] == ("configure", max(st.stream_bytes for st in pipe.model.layers), 0, 0)     # no lend: no keep either
    assert pipe.cache_info()["capacity"] == 4
    # a layer whose encoding (+ slack) is larger than a staging area: whole areas as landing buffers, the lend stays
    streaming, fake, pipe = make(monkeypatch, 4, 3, staging=5000)
    forward(streaming, pipe, 2, 12, before=lambda: pipe.configure_cache(True, 64))
    forward(streaming, pipe, 2, 12, before=lambda: pipe.configure_cache(True, 64))
    assert [e for e in fake.log if e[0] in ("configure", "enable", "disable")] == [("configure", 0, 1, 64), ("enable", fake.log[1][1])]
    assert pipe.cache_info()["capacity"] == 7
    # two slots, or data parallel: nothing to configure
    streaming, fake, pipe = make(monkeypatch, 2, 3)
    assert not pipe.configure_cache(True, 64) and not fake.log


def test_without_the_call_nothing_changes(monkeypatch):
    streaming, fake, pipe = make(monkeypatch, 4, 5)
    first, L = 2, 12
    forward(streaming, pipe, first, L, mode=False)
    n_legacy = len(fake.log)
    assert all(e == ("copy", e[1], "legacy") for e in fake.log) and n_legacy == L - first + 3
    for _ in range(2):
        forward(streaming, pipe, first, L)
    assert not any(e[0] == "configure" for e in fake.log)
    assert fake.log[n_legacy] == ("enable", max(st.stream_bytes for st in pipe.model.layers[first:first + 5]))
    assert sorted(pipe.cache) == list(range(first, first + 5)) and fills(fake) == list(range(first, first + 5))
    assert [li for li, _ in pipe.landed] == [first + 5, first + 6]


def scheduler_stub(monkeypatch, streaming, fake):
    """an OffloadScheduler with everything _ensure and _set_wire_cache touch, over the fake library and a fake context"""
    from lia_amd import scheduler
    monkeypatch.setattr(scheduler.ops, "Context", Ctx)
    monkeypatch.setattr(scheduler.ops, "workspace_bytes", lambda desc, rows: rows * (1 << 20))
    monkeypatch.setattr(scheduler.torch.cuda, "empty_cache", lambda: None)
    monkeypatch.setattr(scheduler.hostinfo, "cap_torch_threads", lambda n: None)
    sched = scheduler.OffloadScheduler.__new__(scheduler.OffloadScheduler)
    model = types.SimpleNamespace(shape=types.SimpleNamespace(hidden=64, vocab=128, layers=12), desc=None, layer_bytes=2048, offsets=list(range(16)),
                                  layers=[Store(i) for i in range(12)])
    sched.model, sched.device, sched.dp, sched.n_slots = model, 0, None, 4
    sched.wire_cache, sched.wire_cache_ws, sched._ws_need, sched._cache_keep = True, True, 0, 0
    sched.ctx = sched.pipe = None
    sched.host_threads = 4
    sched.hidden = types.SimpleNamespace(get=lambda B, T: (None, None))
    sched._await_all_deliveries = lambda: fake.log.append(("await",))
    return scheduler, sched


def step(sched, streaming, B, T, is_prefill=False):
    """_prepare's and _run_layers' calls for one forward of B x T rows"""
    s = types.SimpleNamespace(coop=None, cpu_set=frozenset(), is_prefill=is_prefill, pos0=0 if is_prefill else 9, verify=not is_prefill and T > 1,
                              every_pos=False, B=B, T=T, n_gpu=2, L=12)
    sched._ensure(B * T, B, T, 2)
    sched._set_wire_cache(s)
    pipe = sched.pipe
    pipe.prefetch(2)
    for idx in range(2, 12):
        pipe.acquire(idx)
        pipe.prefetch_ahead(idx, streaming.stream_order(idx, 2, 12, frozenset(), skip_now=not is_prefill))
        pipe.release(idx)


def test_the_scheduler_keeps_what_its_decode_forwards_need(monkeypatch):
    streaming, fake, _ = make(monkeypatch, 4, 3)
    scheduler, sched = scheduler_stub(monkeypatch, streaming, fake)
    MB = 1 << 20
    lm = 2 * 256 * 64 + 8 * 4 * 128 * 4 + MB                          # _ensure's lm_head term for B = 4: larger than one row's MB
    step(sched, streaming, 4, 100, is_prefill=True)                    # 400 rows: a 400 MB workspace, the mode stays off
    assert sched.ctx.workspace_alloc_bytes == 400 * MB and not sched.pipe.keep
    assert not any(e[0] in ("configure", "enable") for e in fake.log)
    del fake.log[:]
    step(sched, streaming, 4, 1)                                       # a decode step of 4 rows keeps max(4 MB, lm)
    step(sched, streaming, 4, 1)
    landing = max(st.stream_bytes for st in sched.model.layers)
    assert [e for e in fake.log if e[0] in ("configure", "enable", "disable")] == [("configure", landing, 1, max(4 * MB, lm)), ("enable", fake.log[1][1])]
    assert sched.wire_cache_info()["capacity"] == 8
    del fake.log[:]
    step(sched, streaming, 4, 3)                                       # a verify block of 12 rows needs more: off, configure, on, one refill
    step(sched, streaming, 4, 1)                                       # ... and the keep never shrinks
    kinds = [e[:1] + (e[3:4] if e[0] == "configure" else ()) for e in fake.log if e[0] in ("configure", "enable", "disable")]
    assert kinds == [("disable",), ("configure", 12 * MB), ("enable",)], kinds
    assert fills(fake) == list(range(2, 10))
    del fake.log[:]
    step(sched, streaming, 4, 100, is_prefill=True)                    # the prefill gets everything back, the configuration stays
    assert [e[0] for e in fake.log if e[0] in ("configure", "enable", "disable")] == ["disable"]
    old_ctx = sched.ctx
    step(sched, streaming, 4, 1)
    assert sched.pipe.keep and not old_ctx.closed
    del fake.log[:]
    # a larger prefill replaces the context: the mode goes off BEFORE the streamer and the context are closed
    step(sched, streaming, 4, 120, is_prefill=True)
    order = [e[0] for e in fake.log if e[0] in ("disable", "await", "destroy")]
    assert order == ["disable", "destroy", "await"] and old_ctx.closed and sched.ctx is not old_ctx
    assert sched._cache_keep == 0                                      # the new context starts its own record
    # a workspace with less than WS_LEND_MIN_BYTES idle is not lent: landing buffers only
    del fake.log[:]
    sched.WS_LEND_MIN_BYTES = 500 * MB
    step(sched, streaming, 4, 1)
    assert [e for e in fake.log if e[0] == "configure"] == [("configure", landing, 0, 0)]
    assert sched.wire_cache_info(regions=False)["capacity"] == 4
    # LIA_WIRE_CACHE_WS=0 / wire_cache_ws=False: the pipeline is never configured
    streaming, fake, _ = make(monkeypatch, 4, 3)
    scheduler, sched = scheduler_stub(monkeypatch, streaming, fake)
    sched.wire_cache_ws = False
    step(sched, streaming, 4, 100, is_prefill=True)
    step(sched, streaming, 4, 1)
    assert sched.pipe.keep and not any(e[0] == "configure" for e in fake.log) and sched.wire_cache_info()["capacity"] == 3
