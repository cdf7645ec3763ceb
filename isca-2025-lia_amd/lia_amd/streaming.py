"""What both schedulers (scheduler.OffloadScheduler, llama.LlamaScheduler) need to stream weights through HBM slots and to run
the resident layers: the slot pipeline over lia_stream_*, the order it prefetches in, the (B, T) hidden-state buffers and the
pointer tables of the one-call resident decode run."""
import ctypes

import torch

from . import _native as N
from . import ops
from .model import LayerStore

# (`.dp` is imported where a DataParallelGroup is in use, never at module level: it pulls in torch.distributed)


class WeightPipeline:
    """Slot bookkeeping over lia_stream_*: prefetch(layer) -> acquire(layer) -> release(layer).

    Decode mode (set_decode_mode, lia_stream_cache_*): KEEP_SLOTS slots stay in the ring, the memory of the others holds the first
    streamed layers of a step in their wire format, and a packed layer that is not cached passes two stages with a resource each:
    `landed` (its copy is queued into a landing buffer) and `inflight` (its decode is queued into a slot).  The link runs ahead by
    landing buffers while the slots cycle through the cached layers.  configure_cache (lia_stream_cache_configure) sizes the landing
    buffers for the layers that are landed and lends the mode the context's workspace beyond what its forwards need: more entries.

    Packed residents (LayerStore.to_device(packed=10): tier "device", packed): a resident layer held as its wire encoding goes
    through the same ring -- prefetch / _issue decode it from where it lies (lia_stream_decode_device), no copy, no landing buffer,
    no cache entry; it needs nothing but a slot.  What the model saves by holding them packed is the streamer's extra region
    (lia_stream_cache_extra, configure_extra): more entries at the same footprint."""

    KEEP_SLOTS = 2
    _extra = 0                      # bytes of the extra region asked of the library (configure_extra)

    def __init__(self, ctx, model, n_slots, dp_group=None):
        self.ctx, self.model, self.lib = ctx, model, N.lib()
        self.dp = dp_group
        h = ctypes.c_void_p()
        N.check(self.lib.lia_stream_create(ctx.handle, n_slots, model.layer_bytes, ctypes.byref(h)), "lia_stream_create")
        self.handle, self.n_slots = h, n_slots
        self.free_slots = list(range(n_slots))
        self.inflight = []          # [(layer_idx, slot)] in issue order, not yet acquired
        self.held = {}              # layer_idx -> slot (acquired, not yet released)
        self.keep = 0               # decode mode: the slots left in the ring (0 = the mode is off)
        self.cache = {}             # layer_idx -> cache entry, bound while the mode is on
        self.cache_filled = set()   # bound layers whose entry holds their bytes
        self.free_landing = []
        self.landed = []            # [(layer_idx, landing buffer)] in issue order: copy queued, decode not yet
        self._plan = None           # (order, bound layers, entry size) of the last cache_plan that found room
        self._cfg = (0, False, 0)   # (landing bytes, lend the workspace, workspace bytes kept) last asked of configure_cache
        self.slot_ptrs = [self.lib.lia_stream_slot_ptr(h, s) for s in range(n_slots)]
        self.ptr_arrays = [ops.weight_ptr_array(p, model.offsets) for p in self.slot_ptrs]
        if dp_group is not None:
            from .dp import RawDeviceBuffer
            self.slot_tensors = [RawDeviceBuffer(p, model.layer_bytes).tensor() for p in self.slot_ptrs]
            self.copy_stream = torch.cuda.ExternalStream(self.lib.lia_stream_copy_stream(h))
            self.staging_tensors = None
            # the root tells every rank which layers travel pack10-encoded and how many bytes each one ships
            # (gloo validation runs without a GPU -- tests/test_dp_gloo.py -- keep the table on the host)
            meta = torch.zeros((len(model.layers), 2), dtype=torch.int64, device="cuda" if torch.cuda.is_available() else "cpu")
            if dp_group.is_root:
                for i, st in enumerate(model.layers):
                    if getattr(st, "codec", 0) == 0x10A:      # LayerStore.CODEC_RANS
                        # the peers of a data-parallel group see no header: inside a group every packed layer travels as pack10 v2
                        if st.tier == "cxl":
                            st.to_cxl(st.want_fmt, v2_only=True)
                        else:
                            st.to_pinned(st.want_fmt, keep_raw=bool(getattr(st, "_raw_ptr", None)), v2_only=True)
                    if st.tier not in ("device", None):
                        meta[i, 0], meta[i, 1] = int(st.packed), int(st.stream_bytes)
            dp_group.dist.broadcast(meta, src=dp_group.root)
            self.layer_meta = meta.cpu().tolist()
            if dp_group.mode == "allgather" and dp_group.world > 1:
                for i, st in enumerate(model.layers):
                    if st.tier not in ("device", None, "remote") and [int(st.packed), int(st.stream_bytes)] != self.layer_meta[i]:
                        raise RuntimeError(f"layer {i}: this rank's wire encoding differs from the root's (allgather streaming needs "
                                           "identical weights and format on every rank)")

    def can_prefetch(self):
        return bool(self.free_slots)

    # -- resident layers -----------------------------------------------------------------------------
    def _resident(self, layer_idx):
        """0: streamed; 1: resident, raw (needs no slot, is never prefetched); 2: resident, held packed (decoded into a slot)"""
        st = self.model.layers[layer_idx]
        if getattr(st, "tier", None) != "device":
            return 0
        return 2 if st.packed else 1

    @property
    def _n_resident(self):
        """resident layers that appear in the prefetch order: all of them while one is held packed, else none"""
        layers = self.model.layers
        if not any(getattr(st, "tier", None) == "device" and st.packed for st in layers):
            return 0
        return sum(1 for st in layers if st.tier == "device")

    def packed_residents(self):
        return [i for i in range(len(self.model.layers)) if self._resident(i) == 2]

    def _decode_resident(self, layer_idx, slot):
        st = self.model.layers[layer_idx]
        N.check(self.lib.lia_stream_decode_device(self.handle, slot, ctypes.c_void_p(st.packed_device_ptr()), st.stream_bytes, st.nbytes // 2,
                                                  int(getattr(st, "codec", 0) or st.packed)), "lia_stream_decode_device")

    def trim_residents(self, first):
        """Before a prefill: of the packed residents a decode step's wrap has queued, only `first` keeps its slot -- a prefill's
        slots are the link's lead over the resident compute."""
        for li, _ in list(self.inflight):
            if li != first and self._resident(li) == 2:
                self.forget(li)

    # -- decode mode ---------------------------------------------------------------------------------
    def _cacheable(self, layer_idx):
        st = self.model.layers[layer_idx]
        return bool(st.packed) and st.tier not in ("device", None)

    def cache_plan(self, order):
        """the layers of `order` (streamed layers in the order a step computes them) that get a cache entry, and the entry size:
        the first C packed ones, C the most for which the library has room when an entry is sized for the largest of them"""
        if self.dp is not None or self.n_slots <= self.KEEP_SLOTS:
            return [], 0
        key = tuple(order)
        if self._plan is not None and self._plan[0] == key:      # (dropped with the cache: drain, before the layers re-tier)
            return self._plan[1:]
        cand = [i for i in order if self._cacheable(i)]
        for c in range(min(len(cand), 64), 0, -1):
            size = max(int(self.model.layers[i].stream_bytes) for i in cand[:c])
            if self.lib.lia_stream_cache_capacity(self.handle, self.KEEP_SLOTS, size) >= c:
                self._plan = (key, cand[:c], size)
                return cand[:c], size
        return [], 0

    def configure_extra(self):
        """The streamer's extra region = what the model saves by holding resident layers packed: sum of raw bytes - (encoded bytes
        + read slack).  Another size than the last one turns the mode off first (the region is part of its geometry); the library is
        called only for a positive sum, or to free a region that no packed resident stands for any more.  Returns whether it changed."""
        if self.dp is not None or self.n_slots <= self.KEEP_SLOTS:
            return False
        saved = sum(int(st.nbytes) - (int(st.stream_bytes) + N.LIA_CACHE_READ_SLACK) for st in self.model.layers if getattr(st, "tier", None) == "device" and st.packed)
        saved = max(saved, 0)
        if saved == self._extra:
            return False
        if self.keep:
            self.set_decode_mode(None)
        self._extra, self._plan = saved, None
        try:
            N.check(self.lib.lia_stream_cache_extra(self.handle, saved), "lia_stream_cache_extra")
        except MemoryError:
            pass                                  # no room on the device: the mode runs without the region
        return True

    def configure_cache(self, lend_workspace, keep_bytes=0):
        """Before set_decode_mode: landing buffers sized for the largest encoded layer this model streams (any of them may be landed,
        not only the ones behind the bound layers), and, lend_workspace, the context's workspace beyond its first keep_bytes as room
        for entries while the mode is on -- keep_bytes is what the forwards that run inside the mode need.  Another configuration
        than the last one turns the mode off first (the library refuses to change it underneath its entries): the next
        set_decode_mode binds and refills.  Returns whether the configuration changed."""
        if self.dp is not None or self.n_slots <= self.KEEP_SLOTS:
            return False
        extra = self.configure_extra()
        sizes = [int(self.model.layers[i].stream_bytes) for i in range(len(self.model.layers)) if self._cacheable(i)]
        cfg = (max(sizes, default=0), bool(lend_workspace), int(keep_bytes) if lend_workspace else 0)
        if cfg == self._cfg:
            return extra
        if self.keep:
            self.set_decode_mode(None)
        try:
            N.check(self.lib.lia_stream_cache_configure(self.handle, cfg[0], int(cfg[1]), cfg[2]), "lia_stream_cache_configure")
        except ValueError:
            # a layer that hardly compresses: its encoding plus the read slack is larger than a staging area -- whole areas then
            N.check(self.lib.lia_stream_cache_configure(self.handle, 0, int(cfg[1]), cfg[2]), "lia_stream_cache_configure")
        self._cfg, self._plan = cfg, None             # (what was asked for: the same request is a no-op whatever the library made of it)
        return True

    def set_decode_mode(self, order):
        """order: the streamed layers a decode step computes on the GPU, in order -> turn the mode on with the first of them bound
        to cache entries (no-op if it is on with these layers); None or nothing to cache: turn it off.  The caller switches between
        forwards, when no layer is held.  Returns whether the mode is on."""
        if order is None:
            self._plan = None
        bound, size = self.cache_plan(order) if order is not None else ([], 0)
        if self.keep and bound == sorted(self.cache, key=self.cache.get):
            return True
        if self.keep:
            N.check(self.lib.lia_stream_cache_disable(self.handle), "lia_stream_cache_disable")
            # decodes already queued into a kept slot stay good; a landed copy has no slot to be decoded into any more
            self.keep, self.cache, self.cache_filled, self.landed, self.free_landing = 0, {}, set(), [], []
            busy = {slot for _, slot in self.inflight} | set(self.held.values())
            self.free_slots = [s_ for s_ in self.free_slots if s_ not in busy] + \
                              [s_ for s_ in range(self.n_slots) if s_ not in busy and s_ not in self.free_slots]
        if not bound:
            return False
        if any(slot >= self.KEEP_SLOTS for slot in self.held.values()):
            raise RuntimeError("decode mode: a held layer sits in a slot that leaves the ring")
        # Prefetches queued into the slots that leave the ring are abandoned (lia_stream_cache_enable lets them finish first), and
        # so are those of the layers that get an entry: a slot holds the decoded layer, the entry wants its wire bytes, and every
        # entry is to be filled by the first step.  (Up to n_slots - 1 layers the prefill's tail had copied cross the link again:
        # once per generation.)
        self.inflight = [(li, slot) for li, slot in self.inflight if slot < self.KEEP_SLOTS and li not in bound]
        N.check(self.lib.lia_stream_cache_enable(self.handle, self.KEEP_SLOTS, size), "lia_stream_cache_enable")
        self.keep = self.KEEP_SLOTS
        busy = {slot for _, slot in self.inflight} | set(self.held.values())
        self.free_slots = [s_ for s_ in self.free_slots if s_ < self.keep and s_ not in busy]
        self.free_slots += [s_ for s_ in range(self.keep) if s_ not in busy and s_ not in self.free_slots]
        self.free_landing = list(range(self.keep))
        self.cache = {li: e for e, li in enumerate(bound)}
        return True

    def cache_info(self):
        return {"on": bool(self.keep), "capacity": len(self.cache), "layers": sorted(self.cache, key=self.cache.get),
                "bytes": sum(int(self.model.layers[i].stream_bytes) for i in self.cache_filled)}

    def cache_regions(self):
        """entries of the mode that is on per region: {"slots", "staging", "workspace", "extra"} (lia_stream_cache_layout)"""
        g = N.CacheGeometry()
        if self.keep:
            N.check(self.lib.lia_stream_cache_layout(self.handle, self.keep, 1, ctypes.byref(g)), "lia_stream_cache_layout")
        return {"slots": g.in_slots, "staging": g.in_staging, "workspace": g.in_workspace, "extra": g.in_extra}

    def _land(self, layer_idx):
        st = self.model.layers[layer_idx]
        b = self.free_landing.pop(0)
        N.check(self.lib.lia_stream_land(self.handle, b, ctypes.c_void_p(st.host_ptr()), st.stream_bytes, int(st.is_dma_able())), "lia_stream_land")
        self.landed.append((layer_idx, b))

    def _issue(self, layer_idx):
        """decode mode: queue whatever brings the layer into a free slot"""
        st = self.model.layers[layer_idx]
        slot = self.free_slots.pop(0)
        fmt = int(getattr(st, "codec", 0) or st.packed)
        if getattr(st, "tier", None) == "device":
            self._decode_resident(layer_idx, slot)
        elif layer_idx in self.cache:
            N.check(self.lib.lia_stream_decode_cached(self.handle, self.cache[layer_idx], slot, ctypes.c_void_p(st.host_ptr()), st.stream_bytes,
                                                      st.nbytes // 2, fmt, int(st.is_dma_able())), "lia_stream_decode_cached")
            self.cache_filled.add(layer_idx)
        elif st.packed:
            pos = next((j for j, (li, _) in enumerate(self.landed) if li == layer_idx), None)
            if pos is None:
                if not self.free_landing:                      # (out of order: give up the copy queued last)
                    self.free_landing.append(self.landed.pop()[1])
                self._land(layer_idx)
                pos = len(self.landed) - 1
            _, b = self.landed.pop(pos)
            N.check(self.lib.lia_stream_decode_landed(self.handle, b, slot, st.nbytes // 2, fmt), "lia_stream_decode_landed")
            self.free_landing.append(b)                        # (the next copy into it is ordered behind this decode by the library)
        else:
            N.check(self.lib.lia_stream_prefetch(self.handle, slot, ctypes.c_void_p(st.host_ptr()), st.nbytes, int(st.is_dma_able())),
                    "lia_stream_prefetch")
        self.inflight.append((layer_idx, slot))

    def _pump(self, idx, next_layer):
        """decode mode's prefetch_ahead: slots go to the layers behind idx strictly in the order they are needed; behind the first
        layer that finds none, packed layers without a cache entry still start their copies while a landing buffer is free."""
        in_order, n_res = True, self._n_resident
        for _, nxt in zip(range(len(self.cache) + 2 * self.keep + 2 + n_res), next_layer):
            if nxt == idx or not (self.free_slots or self.free_landing):
                break
            if nxt in self.held or any(li == nxt for li, _ in self.inflight):
                continue
            res = self._resident(nxt) if n_res else 0
            if res == 1:
                continue                                       # a raw resident layer: computed from where it lies
            if in_order and self.free_slots:
                self._issue(nxt)
                continue
            in_order = False
            if res or nxt in self.cache or not self.model.layers[nxt].packed or any(li == nxt for li, _ in self.landed):
                continue                                       # needs nothing but a slot
            if not self.free_landing:
                break
            self._land(nxt)

    def prefetch(self, layer_idx):
        if any(li == layer_idx for li, _ in self.inflight) or layer_idx in self.held:
            return
        if not self.can_prefetch():
            return
        if self.keep:
            self._issue(layer_idx)
            return
        st = self.model.layers[layer_idx]
        slot = self.free_slots.pop(0)
        if getattr(st, "tier", None) == "device":
            self._decode_resident(layer_idx, slot)
        elif self.dp is None and st.packed:
            N.check(self.lib.lia_stream_prefetch_packed(self.handle, slot, ctypes.c_void_p(st.host_ptr()), st.stream_bytes, st.nbytes // 2,
                                                        int(getattr(st, "codec", 0) or st.packed), int(st.is_dma_able())), "lia_stream_prefetch_packed")
        elif self.dp is None:
            N.check(self.lib.lia_stream_prefetch(self.handle, slot, ctypes.c_void_p(st.host_ptr()), st.nbytes, int(st.is_dma_able())),
                    "lia_stream_prefetch")
        elif self.dp.mode == "allgather" and self.dp.world > 1:        # (one rank: nothing to gather, the broadcast path serves)
            self._prefetch_allgather(st, slot, layer_idx)
        else:
            self._prefetch_broadcast(st, slot, layer_idx)
        self.inflight.append((layer_idx, slot))

    def _prefetch_broadcast(self, st, slot, layer_idx):
        """Root: host -> slot in chunks, each chunk RCCL-broadcast over xGMI as soon as it is enqueued, so chunk
        k travels to the peers while chunk k+1 is still arriving over PCIe.  Peers: receive into the same slot.
        Everything is ordered on the copy stream; the slot is declared ready after the last broadcast."""
        from .dp import RawDeviceBuffer, broadcast_chunked
        dp = self.dp
        packed, nbytes = self.layer_meta[layer_idx]
        N.check(self.lib.lia_stream_begin(self.handle, slot), "lia_stream_begin")
        if packed:
            target, copy_fn = self._staging()[slot][:nbytes], self.lib.lia_stream_copy_chunk_packed
        else:
            target, copy_fn = self.slot_tensors[slot][:self.model.layer_bytes], self.lib.lia_stream_copy_chunk
        before = None
        if dp.is_root:
            base, pinned = st.host_ptr(), int(st.is_dma_able())

            def before(off, n):
                N.check(copy_fn(self.handle, slot, off, ctypes.c_void_p(base + off), n, pinned), "lia_stream_copy_chunk")
        with torch.cuda.stream(self.copy_stream):
            works = broadcast_chunked(dp.dist, target, dp.root, dp.chunk_bytes, before_chunk=before)
            for w in works:
                w.wait()              # the copy stream waits for RCCL's stream; the host does not block
        if packed:
            N.check(self.lib.lia_stream_decode_packed(self.handle, slot, self.model.layer_bytes // 2, int(packed)), "lia_stream_decode_packed")
        N.check(self.lib.lia_stream_mark_ready(self.handle, slot), "lia_stream_mark_ready")

    def _staging(self):
        if self.staging_tensors is None:
            from .dp import RawDeviceBuffer
            cap = self.lib.lia_pack10_bound(self.model.layer_bytes // 2)
            self.staging_tensors = [RawDeviceBuffer(self.lib.lia_stream_staging_ptr(self.handle, s), cap).tensor()
                                    for s in range(self.n_slots)]
        return self.staging_tensors

    def _prefetch_allgather(self, st, slot, layer_idx):
        """Every rank copies ITS slice of the layer's wire bytes host -> device over its own link, then one all-gather on
        the copy stream assembles the layer in every rank's slot (or staging area, then the decode kernel)."""
        dp = self.dp
        packed, nbytes = self.layer_meta[layer_idx]
        G, r = dp.world, dp.rank
        sh = LayerStore.shard_bytes(nbytes, G)
        if st.shard is None or st.shard != (r, G, sh):
            raise ValueError(f"layer {layer_idx}: allgather streaming needs the host copy pinned as slice {r} of {G} "
                             "(LiaOPTModel.random_init(..., shard=(rank, world)))")
        N.check(self.lib.lia_stream_begin(self.handle, slot), "lia_stream_begin")
        if packed:
            full, copy_fn = self._staging()[slot], self.lib.lia_stream_copy_chunk_packed
        else:
            full, copy_fn = self.slot_tensors[slot], self.lib.lia_stream_copy_chunk
        if G * sh > full.numel():
            raise ValueError(f"layer {layer_idx}: {G} slices of {sh} bytes do not fit the {full.numel()}-byte slot")
        full = full[:G * sh]
        N.check(copy_fn(self.handle, slot, r * sh, ctypes.c_void_p(st.host_ptr()), sh, int(st.is_dma_able())), "lia_stream_copy_chunk")
        mine = full[r * sh:(r + 1) * sh]
        with torch.cuda.stream(self.copy_stream):
            if dp.dist.get_backend() == "nccl":
                dp.dist.all_gather_into_tensor(full, mine, async_op=True).wait()      # in place: `mine` is slice r of `full`
            else:
                parts = [torch.empty_like(mine) for _ in range(G)]                    # gloo (validation runs): out of place
                dp.dist.all_gather(parts, mine.clone())
                for g, p in enumerate(parts):
                    if g != r:
                        full[g * sh:(g + 1) * sh].copy_(p)
        if packed:
            N.check(self.lib.lia_stream_decode_packed(self.handle, slot, self.model.layer_bytes // 2, int(packed)), "lia_stream_decode_packed")
        N.check(self.lib.lia_stream_mark_ready(self.handle, slot), "lia_stream_mark_ready")

    def acquire(self, layer_idx):
        """Make the compute stream wait for the layer's copy; returns the 16 device pointers."""
        pos = next((j for j, (li, _) in enumerate(self.inflight) if li == layer_idx), None)
        if pos is None:
            # the layer was not prefetched (a prefill after a decode step with host-computed layers, a different gpu%):
            # load it on demand.  Queued copies of OTHER layers are kept -- the copy stream runs them in order and they
            # are acquired later in this forward; only when every slot is taken is the NEWEST of them given up
            # (lia_stream_begin orders the slot's next copy behind the dropped one's decode kernel).
            while not self.free_slots and self.inflight:
                _, s_drop = self.inflight.pop()
                self.free_slots.append(s_drop)
            if not self.free_slots:
                raise RuntimeError(f"no streamer slot free for layer {layer_idx}: {len(self.held)} layers are held")
            self.prefetch(layer_idx)
            pos = len(self.inflight) - 1
        li, slot = self.inflight.pop(pos)
        N.check(self.lib.lia_stream_wait(self.handle, slot, ctypes.c_void_p(self.ctx.stream)), "lia_stream_wait")
        self.held[layer_idx] = slot
        return self.ptr_arrays[slot]

    def release(self, layer_idx):
        slot = self.held.pop(layer_idx)
        N.check(self.lib.lia_stream_release(self.handle, slot, ctypes.c_void_p(self.ctx.stream)), "lia_stream_release")
        self.free_slots.append(slot)

    def prefetch_ahead(self, idx, next_layer):
        """Layer idx has just been acquired: fill every free slot with the layers that follow it (next_layer: an iterator,
        stream_order below), n_slots - 1 of them at most, until a slot is missing or the order comes back to idx.  The weight
        copies of the next streamed layer(s) overlap this layer's compute (:1305-1312, :1508-1515); behind the last layer the
        order wraps to the first streamed layer of the NEXT forward, so the copy engine keeps running across token steps."""
        if self.keep:
            self._pump(idx, next_layer)
            return
        n_res = self._n_resident
        if n_res:
            # Resident layers in the order (stream_order wraps to layer 0 while residents are held packed).  Outside the decode mode
            # the slots are the link's lead: a packed resident takes one ahead of time only as the very next layer, and never a
            # second one; the others are decoded when they are next -- they need nothing but a slot.
            ahead = sum(1 for li, _ in self.inflight if self._resident(li) == 2)
            for j, nxt in zip(range(self.n_slots - 1 + n_res), next_layer):
                if nxt == idx or not self.can_prefetch():
                    break
                res = self._resident(nxt)
                if res == 2 and j == 0 and not ahead:
                    self.prefetch(nxt)
                if not res:
                    self.prefetch(nxt)
            return
        for _, nxt in zip(range(self.n_slots - 1), next_layer):
            if nxt == idx or not self.can_prefetch():
                break
            self.prefetch(nxt)

    def forget(self, layer_idx):
        """Give up a queued copy of layer_idx (it will not be used: the layer's decode step moved to the host cores).  The slot is
        free again at once; lia_stream_begin orders its next copy behind the abandoned one.  A layer that is bound to a cache entry
        takes the whole cache with it: the next forward binds the layers that are then streamed."""
        if layer_idx in self.cache:
            self.set_decode_mode(None)
        for j, (li, b) in enumerate(self.landed):
            if li == layer_idx:
                self.landed.pop(j)
                self.free_landing.append(b)
                return True
        for j, (li, slot) in enumerate(self.inflight):
            if li == layer_idx:
                self.inflight.pop(j)
                self.free_slots.append(slot)
                return True
        return False

    def decode_stats(self, reset=False, block=True):
        """wire-format decode kernel since the last reset: {"launches", "ms", "bytes_in", "bytes_out"} (lia_stream_decode_stats);
        block=False: never waits for decodes in flight (lia_stream_poll_decode_stats) -- for the edge of a timed region"""
        n, ms, bi, bo = ctypes.c_long(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        fn = self.lib.lia_stream_decode_stats if block else self.lib.lia_stream_poll_decode_stats
        N.check(fn(self.handle, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(bi), ctypes.byref(bo), int(reset)))
        return {"launches": n.value, "ms": ms.value, "bytes_in": bi.value, "bytes_out": bo.value}

    def poll_stats(self):
        """(bytes, busy ms) of the copies that have COMPLETED so far -- never blocks (stats() waits for the queued copies)"""
        b, ms = ctypes.c_double(), ctypes.c_double()
        N.check(self.lib.lia_stream_poll_stats(self.handle, ctypes.byref(b), ctypes.byref(ms)))
        return b.value, ms.value

    def drain(self):
        """Forget every queued copy and every cached layer and wait for the copy engine: called before the model re-tiers its
        layers (the host copies the cache entries were filled from are about to be freed)."""
        self.set_decode_mode(None)
        for _, slot in self.inflight:
            self.free_slots.append(slot)
        self.inflight = []
        torch.cuda.synchronize()
        if self._extra:
            # the packed residents the extra region stands for may be about to become raw again: its bytes go back first
            self._extra, self._plan = 0, None
            N.check(self.lib.lia_stream_cache_extra(self.handle, 0), "lia_stream_cache_extra")

    def stats(self, reset=False):
        b, ms = ctypes.c_double(), ctypes.c_double()
        N.check(self.lib.lia_stream_stats(self.handle, ctypes.byref(b), ctypes.byref(ms), int(reset)))
        return b.value, ms.value

    def close(self):
        if self.handle:
            self.lib.lia_stream_destroy(self.handle)
            self.handle = None
        self.keep, self.cache, self.cache_filled, self.landed, self.free_landing = 0, {}, set(), [], []


def stream_order(idx, first, L, skip=frozenset(), skip_now=True):
    """The streamed layers behind idx in the order they will be needed, without end: idx + 1 ... L - 1, then first ... L - 1 of
    the next forward, and so on (first = 0 while resident layers are held packed: they take slots like streamed ones).  skip: the layers a decode step computes on the host cores, which need no slot; a prefill
    streams every layer (skip_now=False), so for it they are left out only behind the wrap, where the next forward is a
    decode step.  (skip never holds `first`: OffloadScheduler.cpu_layer_order.)"""
    i, skipping = idx, skip_now
    while True:
        i += 1
        if i >= L:
            i, skipping = first, True
        if not (skipping and i in skip):
            yield i


class HiddenPairs:
    """(B, T) -> two [B, T, hidden] bf16 device buffers (a layer reads one and writes the other), kept across forwards; all are
    dropped when a sixth shape arrives."""

    def __init__(self, hidden):
        self.hidden, self.pairs = hidden, {}

    def get(self, B, T):
        if (B, T) not in self.pairs:
            if len(self.pairs) > 4:
                self.pairs.clear()
            x = torch.empty((B, T, self.hidden), dtype=torch.bfloat16, device="cuda")
            self.pairs[(B, T)] = (x, torch.empty_like(x))
        return self.pairs[(B, T)]


class ResidentRun:
    """Device pointers of the HBM-resident layers: one array per layer (16 pointers for OPT, 9 for Llama: len(model.offsets)),
    built on first use, and the two tables lia_decode_layers / lia_llama_decode_layers take for the whole resident run of a
    decode step, rebuilt only when the run, the KV caches (serial, version) or the first layer's address changed."""

    def __init__(self, model):
        self.model, self.ptrs, self.key, self.arrays, self.tables = model, {}, None, None, None

    def layer(self, idx):
        if idx not in self.ptrs:
            self.ptrs[idx] = ops.weight_ptr_array(self.model.layers[idx].device_ptr(), self.model.offsets)
        return self.ptrs[idx]

    def decode_tables(self, n_gpu, kv_state):
        """(weight pointers [n_gpu x pointers per layer], KV struct pointers [n_gpu]), each cast to void*"""
        key = (n_gpu, kv_state.serial, kv_state.version, self.layer(0)[0])
        if self.key != key:
            ptrs = []
            for i in range(n_gpu):
                ptrs.extend(self.layer(i))
            self.arrays = ((ctypes.c_void_p * len(ptrs))(*ptrs), (ctypes.POINTER(N.KV) * n_gpu)(*[ctypes.pointer(kv_state.kv[i]) for i in range(n_gpu)]))
            self.tables = tuple(ctypes.cast(a, ctypes.c_void_p) for a in self.arrays)
            self.key = key
        return self.tables

    def replaced(self, pipe):
        """The model is about to re-tier its layers (another gpu%, wire format, host tier; policy 1 wants raw host copies):
        copies in flight read host buffers that are about to be freed, and the cached device pointers go stale."""
        if pipe is not None:
            pipe.drain()
        self.ptrs.clear()
        self.key = None
