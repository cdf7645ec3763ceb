"""The decode mode's bookkeeping (WeightPipeline.set_decode_mode / _pump / _issue) over a fake library, without a GPU: the real
prefetch loop, driven the way a forward drives it (tests/test_dp_gloo.py::test_weight_pipeline_prefetch_ahead is the model).

The fake keeps what the library keeps -- which entry is filled, which landing buffer holds a copy that no decode has read, which
slot holds a decode that nobody released -- and refuses what the library would have to refuse."""
import pytest

KEEP = 2


class FakeLib:
    def __init__(self, capacity):
        self.capacity, self.on, self.log = capacity, False, []
        self.filled, self.landing, self.slots = {}, {}, {}      # entry -> host ptr; landing -> layer ptr; slot -> "queued" | "held"
        self.max_copies = 0

    # -- what every WeightPipeline needs
    def lia_stream_create(self, ctx, n, bytes_, out):
        self.n_slots = n
        return 0

    def lia_stream_slot_ptr(self, h, s):
        return 0x1000 * (s + 1)

    def lia_stream_destroy(self, h):
        self.log.append(("destroy",))

    def _take_slot(self, slot):
        # (a slot whose prefetch the caller abandoned is refilled while "queued": the library orders that by events)
        assert self.slots.get(slot) != "held", f"slot {slot} refilled while its layer is in use"
        assert not self.on or slot < KEEP, f"slot {slot} holds cached layers"
        self.slots[slot] = "queued"
        assert len(self.slots) <= (KEEP if self.on else self.n_slots), "more decodes in flight than slots"

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

    # -- the decode mode
    def lia_stream_cache_capacity(self, h, keep, entry_bytes):
        return self.capacity if self.n_slots > keep and entry_bytes else 0

    def lia_stream_cache_enable(self, h, keep, entry_bytes):
        assert not self.on and keep == KEEP and self.capacity
        for slot in [s for s in self.slots if s >= keep]:
            assert self.slots[slot] == "queued"               # abandoned by the caller; a held one would be a bug
            del self.slots[slot]
        self.on, self.filled, self.landing = True, {}, {}
        self.log.append(("enable", entry_bytes))
        return 0

    def lia_stream_cache_disable(self, h):
        self.on, self.filled, self.landing = False, {}, {}
        self.log.append(("disable",))
        return 0

    def lia_stream_land(self, h, b, ptr, nbytes, pinned):
        assert self.on and 0 <= b < KEEP and b not in self.landing, (b, self.landing)
        self.landing[b] = ptr.value
        self.max_copies = max(self.max_copies, len(self.landing))
        self.log.append(("copy", ptr.value, "land"))
        return 0

    def lia_stream_decode_landed(self, h, b, slot, n_values, fmt):
        assert self.on and b in self.landing
        self._take_slot(slot)
        self.log.append(("decode", self.landing.pop(b)))
        return 0

    def lia_stream_decode_cached(self, h, entry, slot, ptr, nbytes, n_values, fmt, pinned):
        assert self.on and 0 <= entry < self.capacity
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
        self.idx, self.packed, self.stream_bytes = idx, packed, stream_bytes + idx

    def host_ptr(self):
        return 0x9000 + self.idx

    def is_dma_able(self):
        return True


class Ctx:
    handle, stream = 1, 2


def make(monkeypatch, n_slots, capacity, L=12, raw=()):
    from lia_amd import streaming, _native
    fake = FakeLib(capacity)
    monkeypatch.setattr(_native, "lib", lambda: fake)

    class Model:
        layer_bytes = 2048
        offsets = list(range(16))
        layers = [Store(i, packed=0 if i in raw else 10) for i in range(L)]

    return streaming, fake, streaming.WeightPipeline(Ctx(), Model(), n_slots)


def forward(streaming, pipe, first, L, host=frozenset(), decode=True, mode=True):
    """one forward's calls on the pipeline, as OffloadScheduler._run_layers makes them"""
    if mode is not None:
        pipe.set_decode_mode([i for i in range(first, L) if i not in host] if mode else None)
    pipe.prefetch(first)
    for idx in range(first, L):
        if decode and idx in host:
            continue
        pipe.acquire(idx)
        pipe.prefetch_ahead(idx, streaming.stream_order(idx, first, L, host, skip_now=decode))
        assert len(pipe.landed) + len(pipe.free_landing) == pipe.keep
        assert len(set(pipe.free_slots)) == len(pipe.free_slots)
        assert len(pipe.free_slots) + len(pipe.inflight) + len(pipe.held) == (pipe.keep or pipe.n_slots)
        pipe.release(idx)


def copies(fake):
    """[(layer, "legacy" | "raw" | "land" | "fill")]: every H2D copy in the log"""
    return [(e[1] - 0x9000, e[2]) for e in fake.log if e[0] == "copy"]


@pytest.mark.parametrize("n_slots,capacity", [(4, 5), (3, 2), (4, 1)])
def test_cached_layers_are_copied_once(monkeypatch, n_slots, capacity):
    streaming, fake, pipe = make(monkeypatch, n_slots, capacity)
    first, L = 2, 12
    forward(streaming, pipe, first, L, decode=False, mode=False)          # a prefill: every slot, the legacy path
    assert [how for _, how in copies(fake)] == ["legacy"] * (L - first + n_slots - 1)
    del fake.log[:]
    steps = 3
    for _ in range(steps):
        forward(streaming, pipe, first, L)
    assert pipe.keep == KEEP and sorted(pipe.cache) == list(range(first, first + capacity))
    assert fake.log[0] == ("enable", max(st.stream_bytes for st in pipe.model.layers[first:first + capacity]))
    got = copies(fake)
    bound = set(range(first, first + capacity))
    for li in bound:
        assert [how for i, how in got if i == li] == ["fill"], f"cached layer {li} crossed the link {got}"
    for li in set(range(first, L)) - bound:
        n = len([1 for i, _ in got if i == li])
        assert steps <= n <= steps + 1, (li, n)              # (+ 1: queued for the step that never came)
    # every layer is decoded into a slot once per step, in the order the step needs them (the first step also consumed what
    # the prefill had left decoded in a kept slot); behind the last step the first layer of the next one is queued
    dec = [e[1] - 0x9000 for e in fake.log if e[0] == "decode"]
    assert dec[-1] == first and dec[-1 - 2 * (L - first):-1] == list(range(first, L)) * 2
    assert 0 < fake.max_copies <= KEEP
    # the link runs ahead by landing buffers: behind the last layer of a step both hold layers first + C, first + C + 1
    assert [li for li, _ in pipe.landed] == [first + capacity, first + capacity + 1]
    assert pipe.cache_info() == {"on": True, "capacity": capacity, "layers": list(range(first, first + capacity)),
                                 "bytes": sum(pipe.model.layers[i].stream_bytes for i in bound)}


def test_mode_off_drain_and_forget_return_every_resource(monkeypatch):
    streaming, fake, pipe = make(monkeypatch, 4, 5)
    monkeypatch.setattr(streaming.torch.cuda, "synchronize", lambda: None)
    first, L = 2, 12
    forward(streaming, pipe, first, L)                        # nothing staged in the real library: here the fake has room at once
    forward(streaming, pipe, first, L)
    assert pipe.keep and pipe.landed and pipe.inflight
    # a layer whose copy is queued and a layer whose decode is queued are given up: landing buffer and slot are free at once
    li, b = pipe.landed[0]
    assert pipe.forget(li) and b in pipe.free_landing and pipe.keep
    li, slot = pipe.inflight[0]
    assert li in pipe.cache                                   # (the wrapped first layer): the cache goes with it
    assert pipe.forget(li) and slot in pipe.free_slots and not pipe.keep and not pipe.cache and not pipe.landed
    assert sorted(pipe.free_slots) == [0, 1, 2, 3] and fake.log[-1] == ("disable",)
    # mode off before a prefill: what waits decoded in a kept slot is still good, the landed copies are not
    forward(streaming, pipe, first, L)
    queued = list(pipe.inflight)
    assert pipe.keep and pipe.landed and queued
    forward(streaming, pipe, first, L, decode=False, mode=False)
    assert not pipe.keep and not pipe.cache and not pipe.landed and not pipe.free_landing
    assert len(pipe.free_slots) + len(pipe.inflight) == 4 and len(pipe.inflight) == 3
    forward(streaming, pipe, first, L)
    assert pipe.keep
    pipe.drain()
    assert not pipe.keep and not pipe.cache and not pipe.landed and not pipe.inflight and sorted(pipe.free_slots) == [0, 1, 2, 3]
    assert not fake.on and not fake.landing
    # the next mode refills: a re-tiering has freed the host copies the entries were filled from
    del fake.log[:]
    fake.slots.clear()                                        # (drain's synchronize: nothing is queued any more)
    forward(streaming, pipe, first, L)
    assert [i for i, how in copies(fake) if how == "fill"] == list(range(first, first + 5))
    pipe.close()
    assert not pipe.keep and not pipe.cache


def test_host_set_and_raw_layers_are_never_bound(monkeypatch):
    streaming, fake, pipe = make(monkeypatch, 4, 3, raw={3})
    first, L, host = 2, 12, frozenset({4, 7})
    for _ in range(2):
        forward(streaming, pipe, first, L, host=host)
    assert sorted(pipe.cache) == [2, 5, 6]                     # not 3 (travels raw), not 4 (the host cores compute it)
    got = copies(fake)
    assert not [1 for i, _ in got if i in host]
    assert [how for i, how in got if i == 3] == ["raw", "raw"]
    # the host set changes: the binding follows at the next forward
    forward(streaming, pipe, first, L, host=frozenset({5}))
    assert sorted(pipe.cache) == [2, 4, 6]


def test_two_slots_and_data_parallel_stay_on_the_legacy_path(monkeypatch):
    streaming, fake, pipe = make(monkeypatch, 2, 5)
    for _ in range(2):
        forward(streaming, pipe, 2, 12)
    assert not pipe.keep and all(how == "legacy" for _, how in copies(fake))
    assert not any(e[0] == "enable" for e in fake.log)


def test_planner_subtracts_the_cached_layers():
    """OPT-30B headline (B 64, 256 / 32, gpu% 10, decode policy 2, rANS wire at 10.585 bits): 6 of the 44 streamed layers fit the
    two idle slots and staging areas; measured 554.2-555.8 ms per step with the cache, 638.6-640.2 without
    (results/wire_cache_ab_summary.txt).  A bare Box predicts without the cache, as the measurements it is calibrated on."""
    from lia_amd import planner
    from lia_amd.model import resolve_shape
    sh = resolve_shape("opt-30b")
    off = planner.Box(host_threads=16, host_mem_gb=280.0, wire_ratio=10.585 / 16)
    on = planner.Box(host_threads=16, host_mem_gb=280.0, wire_ratio=10.585 / 16, wire_cache=True)
    assert not planner.Box(host_threads=16, host_mem_gb=280.0).wire_cache
    assert planner.wire_cache_layers(sh, on, 44) == 6 and planner.wire_cache_layers(sh, off, 44) == 0
    assert planner.wire_cache_layers(sh, on, 4) == 4                                                   # never more than stream
    assert planner.wire_cache_layers(sh, planner.Box(host_threads=16, host_mem_gb=280.0, wire_ratio=1.0, wire_cache=True), 44) == 0   # raw wire
    pre_off, dec_off, *rest_off = planner.estimate(sh, 64, 256, 32, 10, 2, off)
    pre_on, dec_on, *rest_on = planner.estimate(sh, 64, 256, 32, 10, 2, on)
    assert abs(dec_on - 555.4) / 555.4 < 0.05 and abs(dec_off - 639.1) / 639.1 < 0.05
    assert pre_on == pre_off and rest_on == rest_off                                                   # a prefill has every slot; same memory
    # a cached layer is never cheaper than a resident one: the plan still keeps everything resident where it fits
    p = planner.plan(sh, 64, 256, 32, on)
    assert p.n_gpu_layers == sh.layers


def test_wire_cache_default_follows_the_environment(monkeypatch):
    from lia_amd import planner
    monkeypatch.delenv("LIA_WIRE_CACHE", raising=False)
    assert planner.wire_cache_default()
    monkeypatch.setenv("LIA_WIRE_CACHE", "0")
    assert not planner.wire_cache_default()
