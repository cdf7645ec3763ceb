"""Resident layers held packed (LayerStore.to_device(packed=10)) in the real WeightPipeline over a fake library, without a GPU:
the prefetch loop driven the way OffloadScheduler._run_layers drives it, with two or three packed device layers in front of the
streamed ones (tests/test_wire_cache_host.py is the model, and its fake library the base of this one).

The fake keeps what the library keeps and refuses what the library would refuse; a resident layer is decoded from device memory
(lia_stream_decode_device): it takes a slot like any decode and never a copy, a landing buffer or a cache entry."""
import pytest

from test_wire_cache_host import KEEP, Ctx, FakeLib, Store, copies

DEV = 0x7000


class ResidentFakeLib(FakeLib):
    def __init__(self, capacity, extra_entries=0):
        super().__init__(capacity)
        self.base, self.extra_entries, self.extra = capacity, extra_entries, 0

    def lia_stream_cache_extra(self, h, nbytes):
        assert not self.on, "the extra region changed while the mode was on"
        assert nbytes != self.extra, "a call that changes nothing"
        self.extra = nbytes
        self.capacity = self.base + (self.extra_entries if nbytes else 0)
        self.log.append(("extra", nbytes))
        return 0

    def lia_stream_decode_device(self, h, slot, ptr, nbytes, n_values, fmt):
        assert DEV <= ptr.value < DEV + 0x100 and nbytes and fmt == 0x10A
        self._take_slot(slot)
        self.log.append(("decode", ptr.value))
        return 0


class Resident:
    """a layer on the device: packed (its wire encoding, + read slack) or raw"""
    tier, codec = "device", 0x10A
    nbytes = 8192                                # raw bytes: a packed one saves 8192 - (1400 + idx + 4096)

    def __init__(self, idx, packed=10):
        self.idx, self.packed, self.stream_bytes = idx, packed, (1400 + idx) if packed else 8192
        if not packed:
            self.codec = 0

    def packed_device_ptr(self):
        assert self.packed
        return DEV + self.idx

    def host_ptr(self):
        raise RuntimeError("layer is on the device")

    def is_dma_able(self):
        raise AssertionError("a resident layer is never copied")


def make(monkeypatch, n_slots, capacity, n_res, L=12, raw_res=(), extra_entries=0, plain=False):
    from lia_amd import streaming, _native
    fake = ResidentFakeLib(capacity, extra_entries)
    monkeypatch.setattr(_native, "lib", lambda: fake)

    class Model:
        layer_bytes = 2048
        offsets = list(range(16))
        layers = [(Store(i) if plain else Resident(i, 0 if i in raw_res else 10)) if i < n_res else Store(i) for i in range(L)]

    return streaming, fake, streaming.WeightPipeline(Ctx(), Model(), n_slots)


def queued_residents(pipe):
    return [li for li, _ in pipe.inflight if pipe._resident(li) == 2]


def forward(streaming, pipe, first, L, decode=True, mode=True):
    """one forward's calls on the pipeline, as OffloadScheduler._run_layers makes them"""
    packed = frozenset(pipe.packed_residents())
    wrap_to = 0 if packed else first
    raw_res = (frozenset(range(first)) - packed) if packed else frozenset()
    if mode:
        pipe.configure_extra()                                  # (_set_wire_cache: inside configure_cache, or by itself)
    pipe.set_decode_mode(list(range(first, L)) if mode else None)
    if packed and not decode and not pipe.keep:
        pipe.trim_residents(min(packed))
    pipe.prefetch(min(packed) if packed else first)
    for idx in range(L):
        if idx < first and idx not in packed:
            continue                                            # a raw resident layer: computed from where it lies
        pipe.acquire(idx)
        pipe.prefetch_ahead(idx, streaming.stream_order(idx, wrap_to, L, raw_res, skip_now=decode))
        assert len(pipe.landed) + len(pipe.free_landing) == pipe.keep
        assert len(set(pipe.free_slots)) == len(pipe.free_slots)
        assert len(pipe.free_slots) + len(pipe.inflight) + len(pipe.held) == (pipe.keep or pipe.n_slots)
        if not decode:
            assert len(queued_residents(pipe)) <= 1, f"a prefill's slots went to resident layers {pipe.inflight}"
        pipe.release(idx)


def decodes(fake):
    """the layer of every decode in the log that names it (a legacy prefetch decodes without a log line of its own)"""
    return [e[1] - (DEV if e[1] < 0x9000 else 0x9000) for e in fake.log if e[0] == "decode"]


@pytest.mark.parametrize("n_slots,capacity,n_res", [(4, 5, 2), (4, 5, 3), (3, 2, 3), (4, 1, 2)])
def test_every_step_decodes_every_layer_once_and_residents_are_never_copied(monkeypatch, n_slots, capacity, n_res):
    streaming, fake, pipe = make(monkeypatch, n_slots, capacity, n_res)
    first, L = n_res, 12
    forward(streaming, pipe, first, L, decode=False, mode=False)          # a prefill: every slot, residents one at a time
    assert not [i for i, _ in copies(fake) if i < first]
    assert decodes(fake)[:n_res] == list(range(n_res))                     # each resident decoded when it was next
    del fake.log[:]
    steps = 3
    for _ in range(steps):
        forward(streaming, pipe, first, L)
    assert pipe.keep == KEEP and sorted(pipe.cache) == list(range(first, first + capacity))
    got = copies(fake)
    assert not [i for i, _ in got if i < first], "a resident layer crossed the link"
    bound = set(range(first, first + capacity))
    for li in bound:
        assert [how for i, how in got if i == li] == ["fill"], f"cached layer {li} crossed the link {got}"
    for li in set(range(first, L)) - bound:
        n = len([1 for i, _ in got if i == li])
        assert steps <= n <= steps + 1, (li, n)
    # every layer 0 .. L - 1 is decoded into a slot once per step, in order; behind the last step layer 0 of the next is queued
    dec = decodes(fake)
    assert dec[-1] == 0 and dec[-1 - 2 * L:-1] == list(range(L)) * 2
    assert 0 < fake.max_copies <= KEEP
    # the link still runs ahead by both landing buffers
    assert [li for li, _ in pipe.landed] == [first + capacity, first + capacity + 1]
    # residents hold no entry and are not counted
    assert pipe.cache_info() == {"on": True, "capacity": capacity, "layers": list(range(first, first + capacity)),
                                 "bytes": sum(pipe.model.layers[i].stream_bytes for i in bound)}


def test_the_first_decode_step_behind_a_prefill_and_the_next_prefill(monkeypatch):
    streaming, fake, pipe = make(monkeypatch, 4, 5, 3)
    first, L = 3, 12
    for _ in range(2):
        forward(streaming, pipe, first, L, decode=False, mode=False)
        assert not pipe.keep and len(queued_residents(pipe)) <= 1
        for _ in range(2):
            forward(streaming, pipe, first, L)
        assert pipe.keep and [li for li, _ in pipe.inflight] == [0]      # the wrap: layer 0 waits decoded in a kept slot
    dec = decodes(fake)
    assert dec[-1 - 2 * L:-1] == list(range(L)) * 2
    assert not [i for i, _ in copies(fake) if i < first]


def test_the_extra_region_follows_the_packed_residents(monkeypatch):
    """configure_extra: the bytes the packed residents save, asked of the library once; more entries while it stands; freed by
    drain (the layers are about to re-tier)"""
    streaming, fake, pipe = make(monkeypatch, 4, 3, 3, extra_entries=2)
    monkeypatch.setattr(streaming.torch.cuda, "synchronize", lambda: None)
    first, L = 3, 12
    saved = sum(8192 - (1400 + i + 4096) for i in range(3))
    for _ in range(3):
        forward(streaming, pipe, first, L)
    assert [e for e in fake.log if e[0] in ("extra", "enable", "disable")] == [("extra", saved), ("enable", fake.log[1][1])]
    assert pipe.cache_info()["capacity"] == 5 and pipe.cache_info()["layers"] == [3, 4, 5, 6, 7]
    pipe.drain()
    assert fake.log[-2:] == [("disable",), ("extra", 0)] and not fake.extra and not pipe.keep
    fake.slots.clear()
    # the residents became raw (policy 1): nothing to ask for, three entries, and no resident in the order
    for st in pipe.model.layers[:3]:
        st.packed, st.codec, st.stream_bytes = 0, 0, 8192
    del fake.log[:]
    for _ in range(2):
        forward(streaming, pipe, first, L)
    assert not any(e[0] == "extra" for e in fake.log) and pipe.cache_info()["capacity"] == 3
    assert min(decodes(fake)) == first


def test_a_layer_pack10_refused_stays_out_of_the_ring(monkeypatch):
    streaming, fake, pipe = make(monkeypatch, 4, 4, 3, raw_res={1})
    first, L = 3, 12
    forward(streaming, pipe, first, L, decode=False, mode=False)
    for _ in range(2):
        forward(streaming, pipe, first, L)
    dec = decodes(fake)
    want = [i for i in range(L) if i != 1]
    assert 1 not in dec and dec[-1] == 0 and dec[-1 - 2 * len(want):-1] == want * 2
    assert not [i for i, _ in copies(fake) if i < first]


def test_mode_off_drain_and_forget_return_every_resource(monkeypatch):
    streaming, fake, pipe = make(monkeypatch, 4, 5, 2)
    monkeypatch.setattr(streaming.torch.cuda, "synchronize", lambda: None)
    first, L = 2, 12
    forward(streaming, pipe, first, L)
    forward(streaming, pipe, first, L)
    assert pipe.keep and pipe.landed and [li for li, _ in pipe.inflight] == [0]
    # the queued resident is given up: its slot is free at once and the cache stays (it holds no entry)
    slot = pipe.inflight[0][1]
    assert pipe.forget(0) and slot in pipe.free_slots and pipe.keep and not pipe.inflight
    li, b = pipe.landed[0]
    assert pipe.forget(li) and b in pipe.free_landing and pipe.keep
    del fake.landing[b]                                        # (the library orders the next copy into it by events)
    forward(streaming, pipe, first, L)                         # layer 0 is decoded on demand
    assert pipe.keep and [li for li, _ in pipe.inflight] == [0]
    # mode off before a prefill: the resident decoded into a kept slot is still good, the landed copies are not
    forward(streaming, pipe, first, L, decode=False, mode=False)
    assert not pipe.keep and not pipe.cache and not pipe.landed and not pipe.free_landing
    assert len(pipe.free_slots) + len(pipe.inflight) == 4
    forward(streaming, pipe, first, L)
    assert pipe.keep
    pipe.drain()
    assert not pipe.keep and not pipe.cache and not pipe.landed and not pipe.inflight and sorted(pipe.free_slots) == [0, 1, 2, 3]
    assert not fake.on and not fake.landing and not fake.extra
    fake.slots.clear()
    del fake.log[:]
    forward(streaming, pipe, first, L)
    assert [i for i, how in copies(fake) if how == "fill"] == list(range(first, first + 5))
    pipe.close()
    assert not pipe.keep and not pipe.cache


@pytest.mark.parametrize("raw_in_front", [True, False])
def test_without_packed_residents_the_log_is_the_old_one(monkeypatch, raw_in_front):
    """raw resident layers (or, as in the existing tests, layers the pipeline never looks at) in front: not one call differs from
    the log of tests/test_wire_cache_host.py's scenario, and the new entry points are never reached"""
    logs = []
    for plain in (True, False):
        streaming, fake, pipe = make(monkeypatch, 4, 5, 2, raw_res={0, 1}, plain=plain or not raw_in_front)
        first, L = 2, 12
        forward(streaming, pipe, first, L, decode=False, mode=False)
        for _ in range(3):
            forward(streaming, pipe, first, L)
        logs.append(list(fake.log))
        assert [how for _, how in copies(fake)][:L - first + 3] == ["legacy"] * (L - first + 3)
        assert [li for li, _ in pipe.landed] == [first + 5, first + 6] and sorted(pipe.cache) == list(range(first, first + 5))
        assert not any(e[0] == "extra" for e in fake.log) and min(decodes(fake)) == first
    assert logs[0] == logs[1]
