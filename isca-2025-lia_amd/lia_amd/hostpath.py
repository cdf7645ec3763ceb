"""Decoder layers computed on the host cores (policy 1, and the cooperative split's host-computed decode layers): what the
offload scheduler keeps for them -- the pinned hidden-state pair, the OpenMP team, the pointer tables of the one-region decode
call, the wall clock spent in the library -- and the two calls into lia_host.cpp.  Weights are read in place from the layer's raw
bf16 host copy, K/V from the host cache; nothing crosses the link but the hidden state."""
import ctypes
import time

from . import _native as N
from . import hostinfo
from . import ops
from .kvcache import PinnedPool


class HostLayers:
    def __init__(self, model):
        self.model = model
        self.time = {"ms": 0.0, "calls": 0}     # wall clock inside lia_host_layer(s)_forward, and the layers it computed
        self.team = None                        # hostinfo.HostTeam, made by the first host-computed layer
        self.hidden = None                      # (pinned block, pinned block, bytes of each)
        self.tables = None                      # (key, weight pointers, K pointers, V pointers) of the last layers_forward

    def threads(self, host_threads, world=1):
        """the whole-layer host team (hostinfo.HostTeam): the attention team's count"""
        if self.team is None:
            self.team = hostinfo.HostTeam(host_threads or hostinfo.default_host_threads(world))
        return self.team.threads

    def report(self):
        return None if self.team is None else {"threads": self.team.threads}

    def hidden_pair(self, ctx, nbytes):
        """Two pinned hidden-state buffers for the host-computed layers, kept across steps; a larger request hands the old
        pair back to the pool first, release_hidden() hands back the last one."""
        if self.hidden is None or self.hidden[2] < nbytes:
            self.release_hidden(ctx)
            self.hidden = (PinnedPool.acquire(nbytes), PinnedPool.acquire(nbytes), nbytes)
        return self.hidden[:2]

    def release_hidden(self, ctx):
        if self.hidden is not None:
            ctx.synchronize()                 # a blit into / out of the pair may still be in flight
            PinnedPool.release(self.hidden[0], self.hidden[2])
            PinnedPool.release(self.hidden[1], self.hidden[2])
            self.hidden = None

    def _spent(self, t0, layers):
        self.time["ms"] += 1e3 * (time.time() - t0)
        self.time["calls"] += layers

    def layer_forward(self, raw, kv, hx, hy, B, T, pos0, threads, starts=None):
        """One layer (lia_host_layer_forward): hidden state at host address hx -> hy.  raw: the layer's raw bf16 host copy; kv:
        its _native.KV (host cache); starts: int32 [B] host array of a left-padded batch (row b's first real position) or None."""
        m, lib = self.model, N.lib()
        w = ops.weight_ptr_array(raw, m.offsets)
        args = (ctypes.byref(m.desc), ctypes.byref(w), ctypes.c_void_p(hx), ctypes.c_void_p(hy), ctypes.c_void_p(kv.k),
                ctypes.c_void_p(kv.v), kv.smax, kv.batch, B, T, pos0, 0, threads)
        t0 = time.time()
        if starts is None:
            rc = lib.lia_host_layer_forward(*args)
        else:
            rc = lib.lia_host_layer_forward_padded(*args, ctypes.c_void_p(starts.ctypes.data))
        self._spent(t0, 1)
        N.check(rc, "lia_host_layer_forward")

    def layers_forward(self, layers, raws, kv_state, hx, hy, B, T, pos0, threads, starts=None):
        """Every layer of `layers` (raws: their raw host copies) back to back in ONE OpenMP region (lia_host_layers_forward: a
        decode step, B * T <= 256); returns the address the result is at, hx or hy.  The pointer tables are rebuilt only when a
        layer's host copy or the caches moved."""
        m, lib, kv = self.model, N.lib(), kv_state.kv
        key = (tuple(raws), kv_state.serial, kv_state.version, tuple(kv[i].k for i in layers), tuple(kv[i].v for i in layers))
        if self.tables is None or self.tables[0] != key:
            wt = (ctypes.c_void_p * (16 * len(layers)))(*[raw + o for raw in raws for o in m.offsets])
            self.tables = (key, wt, (ctypes.c_void_p * len(layers))(*key[3]), (ctypes.c_void_p * len(layers))(*key[4]))
        _, wt, kt, vt = self.tables
        kv0 = kv[layers[0]]
        args = (ctypes.byref(m.desc), len(layers), wt, ctypes.c_void_p(hx), ctypes.c_void_p(hy), kt, vt, kv0.smax, kv0.batch, B, T,
                pos0, 0, threads)
        t0 = time.time()
        if starts is None:
            where = lib.lia_host_layers_forward(*args)
        else:
            where = lib.lia_host_layers_forward_padded(*args, ctypes.c_void_p(starts.ctypes.data))
        self._spent(t0, len(layers))
        N.check(min(where, 0), "lia_host_layers_forward")
        return hy if where == 1 else hx
