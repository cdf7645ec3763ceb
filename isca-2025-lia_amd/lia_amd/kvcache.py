"""Where the KV caches of a generation live: exact-size pinned host blocks (PinnedPool) and the per-layer caches of an OPT
generation (KVState: HBM for resident layers, pinned host memory for streamed ones, both for the online split's candidates).
KV_SERIAL numbers every cache object of the process, LlamaKVState (llama.py) included."""
import ctypes
import itertools

import torch

from . import _native as N
from . import hostinfo


class PinnedPool:
    """Exact-size pinned host blocks with a per-size free list.  torch's pin_memory=True rounds every block up to a
    power of two (a 264 MB OPT-30B cache tensor takes 512 MB, 23 GB of host KV become 45 GB) -- on a box whose container
    limit decides which model fits, the caches are allocated here instead and recycled across generate() calls."""
    _free = {}

    @classmethod
    def acquire(cls, nbytes):
        lst = cls._free.get(nbytes)
        if lst:
            return lst.pop()
        hostinfo.guard_host_allocation(nbytes, "pinned host KV cache")
        ptr = N.lib().lia_host_alloc_pinned(nbytes)
        if not ptr:
            raise MemoryError("Fail to allocate pinned memory: " + N.lib().lia_last_error().decode())
        return ptr

    @classmethod
    def release(cls, ptr, nbytes):
        cls._free.setdefault(nbytes, []).append(ptr)

    @classmethod
    def idle_blocks(cls, nbytes):
        return len(cls._free.get(nbytes, ()))

    @classmethod
    def trim(cls):
        for lst in cls._free.values():
            for ptr in lst:
                N.lib().lia_host_free_pinned(ptr)
        cls._free.clear()

    @staticmethod
    def as_tensor(ptr, shape):
        n = 1
        for d in shape:
            n *= d
        buf = (ctypes.c_char * (2 * n)).from_address(ptr)
        return torch.frombuffer(buf, dtype=torch.int16).view(torch.bfloat16).view(*shape)


KV_SERIAL = itertools.count(1)       # KVState / LlamaKVState objects, numbered: id() values come back after a free


class KVState:
    """Per-layer KV caches of one generation: seq-major [Smax,B,h,d] (attentions.py:462-476), in HBM for
    resident layers and in pinned host memory for streamed ones (lia/modeling_opt.py:1270-1281)."""

    def __init__(self, model, n_gpu, B, smax, all_on_device=False, host_layers=(), dual_layers=()):
        """host_layers (with all_on_device): layers whose cache stays in pinned host memory all the same -- the layers the
        cooperative split computes on the host cores (scheduler.forward cpu_layers).  dual_layers (with all_on_device): the
        CANDIDATE host layers of the online split: a buffer in HBM and one in pinned host memory each, the cache living in one of
        them at a time (host_layers says where it starts) and moved by `move_cache` when the controller changes the host set."""
        sh = model.shape
        self.B, self.smax, self.len = B, smax, 0
        self.serial, self.version = next(KV_SERIAL), 0      # (serial, version) names one set of kv[] entries: cached pointer tables key on it
        self.pending = {}          # layer -> ticket of a deferred K/V delivery (scheduler.forward, lia_kv_deliver)
        self.all_on_device = all_on_device
        host_layers = frozenset(host_layers) if all_on_device else frozenset()
        dual_layers = frozenset(dual_layers) if all_on_device else frozenset()
        if all_on_device:
            n_gpu = sh.layers          # policy 3 for streamed layers too: every cache lives in HBM
        shape = (smax, B, sh.heads, sh.head_dim)
        nbytes = 2 * smax * B * sh.heads * sh.head_dim
        # what this generation must ALLOCATE: its host blocks minus the idle ones of the same size an earlier generation left in the
        # pool (r06: the check counted them twice -- a second generate() of a 168 GiB cache was refused on a box that holds it once)
        n_host_blocks = 2 * (sh.layers - n_gpu + len(host_layers | dual_layers))
        # (0.92 of what the container has left, not the planner's 0.85: the caches are the LAST large host allocation of a generation
        # -- the weights are placed by now -- and PinnedPool.acquire guards every block again at 0.93 of the limit; the reference's own
        # large-batch lines sit this close to their box's memory: cxl_offloading.sh:37, batch 1150 = 236 GiB of caches on a 300 GiB box)
        hostinfo.check_host_allocation(max(0, n_host_blocks - PinnedPool.idle_blocks(nbytes)) * nbytes, "host KV cache", safety=0.92)
        self.tensors, self.kv, self._pinned, self.dual = [], [], [], {}

        def device_pair():
            k = torch.empty(shape, dtype=torch.bfloat16, device="cuda")
            return k, torch.empty_like(k)

        def host_pair():
            pk, pv = PinnedPool.acquire(nbytes), PinnedPool.acquire(nbytes)
            self._pinned += [(pk, nbytes), (pv, nbytes)]
            return PinnedPool.as_tensor(pk, shape), PinnedPool.as_tensor(pv, shape)

        for i in range(sh.layers):
            on_dev = 1 if (i < n_gpu and i not in host_layers) else 0
            if i in dual_layers:
                self.dual[i] = {1: device_pair(), 0: host_pair()}
                k, v = self.dual[i][on_dev]
            else:
                k, v = device_pair() if on_dev else host_pair()
            self.tensors.append((k, v))
            self.kv.append(N.KV(k.data_ptr(), v.data_ptr(), smax, B, on_dev))

    def move_cache(self, lib, i, to_device):
        """The cache of dual layer i changes sides: rows [0, len) (contiguous in the seq-major layout) copied over the host link,
        `kv[i]` re-pointed.  Synchronous; the caller has synchronized the compute stream and awaited the layer's K/V delivery."""
        to_device = 1 if to_device else 0
        if i not in self.dual:
            raise ValueError(f"layer {i} has one KV cache only (KVState(dual_layers=...) names the layers that can change sides)")
        if self.kv[i].on_device == to_device:
            return 0
        nbytes = self.len * self.B * self.tensors[i][0].shape[2] * self.tensors[i][0].shape[3] * 2
        dst = self.dual[i][to_device]
        for s_t, d_t in zip(self.tensors[i], dst):
            if nbytes:
                fn = lib.lia_memcpy_h2d if to_device else lib.lia_memcpy_d2h
                N.check(fn(ctypes.c_void_p(d_t.data_ptr()), ctypes.c_void_p(s_t.data_ptr()), ctypes.c_size_t(nbytes)), "lia_memcpy (KV cache move)")
        self.tensors[i] = dst
        self.kv[i] = N.KV(dst[0].data_ptr(), dst[1].data_ptr(), self.smax, self.B, to_device)
        self.version += 1
        return 2 * nbytes

    def close(self):
        """Hand the pinned blocks back to the pool (the tensors over them must not be used afterwards)."""
        if self._pinned and torch.cuda.is_available():
            torch.cuda.synchronize()      # policy-0 K/V deliveries may still be landing in these blocks
        self.tensors, self.kv, self.dual = [], [], {}
        self.version += 1
        for ptr, nbytes in self._pinned:
            PinnedPool.release(ptr, nbytes)
        self._pinned = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
