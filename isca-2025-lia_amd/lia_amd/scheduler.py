"""The offload scheduler: MI355X-native counterpart of OPTDecoder.forward (lia/modeling_opt.py:1021-1586).

Same policy table (lia/modeling_opt.py:1167-1176), same flag surface, different machinery:

  reference                                                   here
  ---------------------------------------------------------   ------------------------------------------------------
  16 copy_ per layer on load_weight_stream (:270-293)          ONE pinned hipMemcpyAsync of the packed layer on the
                                                               streamer's copy stream into an HBM slot
  torch.cuda.synchronize() after every minibatch/layer          hipEvent handshakes slot<->compute stream; the host only
  (:1298,1339,1346,1506,1528)                                   blocks for the policy-2 host attention round trip
  first streamed layer loaded synchronously at the start        prefetch runs ahead across token steps (after the last
  of every forward (:1287-1298, :1497-1506)                     layer it wraps to the first streamed layer), so the copy
                                                               engine never idles between forwards
  hidden states bounced through pinned host memory             the whole-batch hidden state stays in HBM (235 MB at
  (:1262-1267, load_activation/store_hidden :320-355)          B=64,T=256,H=7168; the GPU has 288 GB)
  GPU-side un-blocking of every streamed weight (G2)           none: host weights are row-major
  KV cache host tensors re-pinned per call (:1381-1387)        pinned once per generation
  embed / final LN / lm_head on the CPU                        on the GPU (weights resident), last position only

Weights of layers [0, n_gpu) are HBM-resident (policy 3, KV in HBM); layers [n_gpu, L) are streamed and
run the phase's policy: prefill 0 (minibatched, K/V delivered to the host cache) | decode 2 (GPU linears
+ host attention) | decode 0 (cached rows fetched to the GPU).  Policy 1 (all-CPU) is the IPEX baseline
and is not scheduled here.

This module holds the flag surface and OffloadScheduler.  What it drives lives beside it and is re-exported from here: the
slot pipeline and the caches shared with llama.LlamaScheduler (streaming.py), the host-computed layers (hostpath.py), the KV
caches and the pinned pool (kvcache.py), the cooperative split's controller (coop.py).
"""
import ctypes
import os
import time
import warnings
import weakref
from types import SimpleNamespace

import numpy as np
import torch

from . import _native as N
from . import hostinfo, ops, planner
from .coop import CoopController, CoopStore
from .hostpath import HostLayers
from .kvcache import KVState, PinnedPool
from .streaming import HiddenPairs, ResidentRun, WeightPipeline, stream_order

COOP_HEADROOM = 10                    # raw host copies kept beyond the planner's count: the room the online controller may search upward
DEFAULT_STREAM_FORMAT = "pack10"      # one default for OffloadScheduler, run_generation.py and bench.py


def default_stream_format():
    """Wire format of the pinned streamed layers when the caller names none: $LIA_STREAM_FORMAT, else pack10 -- a LOSSLESS encoding
    (the device decodes it back to the same bf16 bits, tests/test_gpu_ops.py), so the results are those of the reference's raw
    transfer; a layer whose values do not pack (encoding >= raw size, or too many out-of-window values) is pinned raw by itself
    (LayerStore._encode_packed).  `raw` = what the reference ships (Tensor.pin_memory of the bf16 tensors, modeling_opt.py:207-227)."""
    fmt = os.environ.get("LIA_STREAM_FORMAT", DEFAULT_STREAM_FORMAT).lower()
    if fmt not in ("raw", "pack10"):
        raise ValueError(f"LIA_STREAM_FORMAT={fmt!r}: expected raw or pack10")
    return fmt


def minibatch_bounds(B, num_minibatch):
    """[(first row, rows)] of the prefill minibatches: num_minibatch clamped to [1, B]; every minibatch has int(B / num_minibatch)
    rows (lia/modeling_opt.py:1178) except the last, which also takes the remainder the reference drops."""
    B, n = int(B), max(1, min(int(num_minibatch), int(B)))
    if B <= 0:
        return []
    mini = B // n
    return [(i * mini, mini) for i in range(n - 1)] + [((n - 1) * mini, B - (n - 1) * mini)]


def placement_formats(prefill_policy, decoding_policy, wire, n_gpu, L, pin_weight, enable_cxl, cpu_set=frozenset(), data_parallel=False):
    """(wire format of the streamed layers' host copy, layers that ALSO keep a raw bf16 host copy) for a flag set.  The host cores
    read raw bf16 in place (policy 1, the cooperative split's host layers); the link ships the lossless pack10 bytes.
      * neither phase on the host cores: packed, + raw copies for the cooperative split's candidates (cpu_set);
      * prefill 0 / decode 1 with pinned weights (the README example, llm/scripts/lia_offline.sh:13-19): r06 keeps BOTH -- the
        policy-0 prefill streams every layer once and is link-bound (54.3 GB raw: 950 ms; 36.6 GB packed: 650 ms), the decode
        steps read the raw copies.  +0.675 x the streamed bytes of pinned memory; a layer the container has no room to keep twice
        stays raw only (LayerStore.to_pinned);
      * prefill 1, the NUMA tier (one copy by definition), unpinned weights: raw."""
    if prefill_policy != 1 and decoding_policy != 1:
        return wire, frozenset(cpu_set)
    if wire and prefill_policy in (0, 3) and decoding_policy == 1 and pin_weight and not enable_cxl and not data_parallel:
        return wire, frozenset(range(n_gpu, L))
    return 0, frozenset(cpu_set)


def wire_format_code(fmt):
    """"raw" / "pack10" / 0 / 10 / False / True -> 0 | 10; anything else (pack11 / pack12 of builds before r05) is refused by name"""
    codes = {"raw": 0, "pack10": 10, False: 0, True: 10, 0: 0, 10: 10}
    if fmt not in codes:
        raise ValueError(f"wire format {fmt!r} is not supported by this build (raw or pack10): a model directory written with "
                         "--wire pack11 / pack12 by an earlier build must be rewritten (python -m lia_amd.packed_checkpoint ... --wire pack10)")
    return codes[fmt]


def check_verify_block(block_ids, kv_state):
    """every refusal of a scheduler's verify(), by name"""
    if block_ids.dim() != 2:
        raise ValueError(f"verify: block_ids must be [batch, T], got shape {tuple(block_ids.shape)}")
    T = block_ids.shape[1]
    if kv_state.len < 1:
        raise ValueError("verify: an empty cache (a draft block is verified behind the prompt's prefill)")
    if T < 2:
        raise ValueError(f"verify: a block of at least two tokens, the pending one and a draft (T={T})")
    if kv_state.len + T > kv_state.smax:
        raise ValueError(f"verify: the cache holds {kv_state.smax} positions, the context {kv_state.len} + the block {T} need {kv_state.len + T}")


def check_verify_rows(block_ids, kv_state, row_lens, flags, n_gpu, L):
    """every refusal of OffloadScheduler.verify_rows(), by name"""
    from . import speculative
    if block_ids.dim() != 2:
        raise ValueError(f"verify_rows: block_ids must be [batch, T], got shape {tuple(block_ids.shape)}")
    B, T = block_ids.shape
    why = speculative.row_flags_refusal(flags)
    if why is None and not (getattr(kv_state, "all_on_device", False) and all(kv_state.kv[i].on_device for i in range(L))):
        why = speculative.ROW_REFUSALS["flags"] + "; this cache has layers on the host"
    if why:
        raise ValueError("verify_rows: " + why)
    if T < 2:
        raise ValueError(f"verify_rows: a block of at least two tokens, the pending one and a draft (T={T})")
    if row_lens.shape != (B,) or (row_lens < 1).any():
        raise ValueError(f"verify_rows: row_lens must hold one cache length >= 1 per row ({B}), got {row_lens.tolist()}")
    if int(row_lens.max()) + T > kv_state.smax:
        raise ValueError(f"verify_rows: the cache holds {kv_state.smax} positions, the longest row {int(row_lens.max())} + the block {T} "
                         f"need {int(row_lens.max()) + T}")


def verify_head(ctx, head, hidden, ids_dev, act_dev, suppress_token, n_suppress=0, n_suppress_rows=None, sampler=None, rejector=None,
                return_logits=False):
    """the verify head of one pass, for every scheduler: rejection verification with a rejector, else the sampled head with a sampler,
    else the greedy one; n_suppress_rows (int32 [B], device: row mode) in place of n_suppress.  head: (norm tensors, head weight, eps,
    family prefix of the ops.Context methods -- "" or "llama_").  -> ops.VerifyResult"""
    norm, weight, eps, family = head
    if rejector is not None:
        return getattr(ctx, family + "lm_verify_reject")(hidden, *norm, weight, ids_dev, rejector, eps, suppress_token, n_suppress,
                                                         active=act_dev, return_logits=return_logits, return_probs=True)
    if sampler is not None:
        return getattr(ctx, family + "lm_verify_sample")(hidden, *norm, weight, ids_dev, sampler, eps, suppress_token, n_suppress,
                                                         n_suppress_rows=n_suppress_rows, active=act_dev, return_logits=return_logits,
                                                         return_p_draft=True)
    if n_suppress_rows is not None:
        return getattr(ctx, family + "lm_verify_rows")(hidden, *norm, weight, ids_dev, n_suppress_rows, eps, suppress_token, act_dev)
    return getattr(ctx, family + "lm_verify")(hidden, *norm, weight, ids_dev, eps, suppress_token, n_suppress, act_dev)


class HeadModifierHooks:
    """what generation.generate() asks of a scheduler about the head modifiers, shared by OffloadScheduler and LlamaScheduler: a table
    is passed per call -- forward(token_mask=, penalties=) / verify(token_mask=) set it on the library context around their head call
    (ops.Context.head_modifiers) -- and these clear the context when a generation ends, also after an exception."""

    supports_penalties = True         # forward(penalties=): generate()'s repetition / presence / frequency penalties

    def set_token_mask(self, mask):
        """None only: no allowed-token table on the library context -- every later head call is the unmasked one"""
        if mask is not None:
            raise ValueError("set_token_mask takes None only: a table is passed per call, forward(token_mask=) / verify(token_mask=)")
        if self.ctx is not None:
            self.ctx.set_token_mask(None)

    def set_penalties(self, table):
        """None only: no count table on the library context"""
        if table is not None:
            raise ValueError("set_penalties takes None only: the table is passed per call, forward(penalties=)")
        if self.ctx is not None:
            self.ctx.set_penalties(None)


class OffloadScheduler(HeadModifierHooks):
    """forward(input_ids, kv_state, **lia flags) -> (logits [B,vocab], next_ids [B]) on the device."""

    resident_packed = False     # (class-level: a scheduler built without __init__ holds its residents raw)

    def __init__(self, model, device=0, n_slots=None, dp_group=None, wire=None, wire_cache=None, wire_cache_ws=None, split_decode=None,
                 resident_packed=None):
        self.model, self.device, self.dp = model, device, dp_group
        # a decode step's GPU attention: "measured" = the split-key route where it was measured faster than the one-workgroup kernel
        # (ops.split_decode_pays), True = every step over more keys than one chunk (A/B runs, tests), False = never -- and always,
        # whatever this says, where the cache has outgrown the one-workgroup kernel.  LIA_SPLIT_DECODE=0|1|measured.
        self.split_decode = ops.split_decode_mode(os.environ.get("LIA_SPLIT_DECODE") if split_decode is None else split_decode,
                                                  "LIA_SPLIT_DECODE" if split_decode is None else "split_decode")
        self.n_slots = n_slots or 4
        # decode steps and small blocks keep the first streamed layers in HBM in their wire format, in the streamer slots such
        # forwards have no use for (WeightPipeline.set_decode_mode); LIA_WIRE_CACHE=0: every layer crosses the link every step
        self.wire_cache = (os.environ.get("LIA_WIRE_CACHE", "1") != "0") if wire_cache is None else bool(wire_cache)
        # ... and in the context's workspace beyond what such forwards need, which is sized for the prefill and idles during decode
        # (WeightPipeline.configure_cache); LIA_WIRE_CACHE_WS=0: slots and staging areas only, whole staging areas as landing buffers
        self.wire_cache_ws = (os.environ.get("LIA_WIRE_CACHE_WS", "1") != "0") if wire_cache_ws is None else bool(wire_cache_ws)
        # ... and the HBM-resident layers are held in that wire format too, decoded into a slot for every use like a cached layer: what
        # they save holds more entries at the same footprint (WeightPipeline.configure_extra).  Only where the wire cache applies
        # (_resident_format); LIA_RESIDENT_PACKED=0: raw residents, computed from where they lie
        self.resident_packed = (os.environ.get("LIA_RESIDENT_PACKED", "1") != "0") if resident_packed is None else bool(resident_packed)
        self._ws_need = 0           # workspace the forward being prepared needs (_ensure)
        self._cache_keep = 0        # the largest _ws_need of a forward that ran inside the decode mode on this context
        # wire format of the streamed layers: "pack10" (the lossless encoding of lia_pack10.hip) or "raw" bf16
        fmt = default_stream_format() if wire is None else wire
        self.wire = wire_format_code(fmt)
        self.ctx = None
        self.pipe = None
        self.hidden = HiddenPairs(model.shape.hidden)
        self.resident = ResidentRun(model)
        self.host = HostLayers(model)      # policy 1 and the cooperative split's host-computed layers
        self._key_starts = None     # (host int32 [B], device copy, context it was uploaded to) of a left-padded generation
        # a verify pass's attention: "measured" = the block kernel where it was measured faster than the append kernels
        # (speculative.block_attention_pays), True = wherever the launch takes the shape (A/B runs, tests), False = never
        self.block_attention = "measured"
        self.host_threads = None    # OpenMP team of the host attention / host layers; default = hostinfo.default_host_threads
        # policy-0 prefill: keep the fresh K/V of the streamed layers in HBM until the prefill's last layer has run and deliver
        # them to the host caches then (lia_kv_deliver), instead of beside the prefill's weight stream.  LIA_DEFER_KV=0: deliver at once.
        self.defer_kv = os.environ.get("LIA_DEFER_KV", "1") != "0"
        # the last layer of a prefill computes everything behind its q|k|v projection on the last position only (lia_layer_forward_last);
        # prefill_tail = False: every position, as the reference does (same ids, tests/test_gpu_round3.py)
        self.prefill_tail = True
        self._kv_hold = None        # ((B, T, first streamed layer), [(k, v, KV struct) per streamed layer])
        # every delivery ticket not yet waited for, whichever KVState it belongs to: ticket -> (weakref(KVState), layer).  The
        # holding caches are shared by all generations of this scheduler, so a new prefill may only write them once ALL of these
        # have landed (a generation that ended at its prefill, a second live KVState, a KVState reused with len reset)
        self._outstanding = {}
        self._coop = None           # CoopController of the cooperative split (cpu_layers=-1), kept across generations
        self._coop_key = None
        self.kv_moved_bytes = 0      # KV cache bytes moved between HBM and host by the online split (KVState.move_cache)
        self.kv_delivery = {"bytes": 0, "device_ms": None, "host_wait_ms": 0.0}   # of the last deferred delivery

    @property
    def host_layer_time(self):
        """wall clock inside lia_host_layer(s)_forward (policy 1 / host-computed layers); run_generation --profile reads and resets it"""
        return self.host.time

    @host_layer_time.setter
    def host_layer_time(self, value):
        self.host.time = value

    # -- resources -----------------------------------------------------------------------------------
    def _ensure(self, rows, B, T, n_gpu, score_rows=0, split_bytes=0):
        """Context workspace (sized by the largest layer call seen so far), streamer slots, hidden buffers.  score_rows: a scoring
        pass also needs room for one chunk of lm_score (its normed rows and bf16 logits, lia_lm_score_workspace_bytes).
        split_bytes: the split-key attention scratch of a forward that takes that route, behind the layer call's own layout."""
        sh = self.model.shape
        lm_bytes = 2 * 256 * sh.hidden + 8 * min(B, 256) * sh.vocab * 4 + (1 << 20)
        need = max(ops.workspace_bytes(self.model.desc, rows) + split_bytes, lm_bytes)
        if score_rows:
            need = max(need, N.lib().lia_lm_score_workspace_bytes(score_rows, sh.hidden, sh.vocab))
        self._ws_need = need
        if self.ctx is None or need > self.ctx.workspace_alloc_bytes:
            if self.pipe is not None:
                self.pipe.set_decode_mode(None)       # the wire cache hands the workspace's tail back before the context goes
                self.pipe.close()
                self.pipe = None
            if self.ctx is not None:
                self._await_all_deliveries()      # their tickets die with the context
                self.ctx.close()
            # (the library allocates with hipMalloc: blocks torch's caching allocator keeps from the model's placement -- the drawn
            # layers, the wire encoder's buffers -- are handed back first; at batch 1050 the planner's pick ran out of HBM here)
            torch.cuda.empty_cache()
            self.ctx = ops.Context(self.device, need)
            self._cache_keep = 0
            # the policy-2 host attention team: usable CPUs (affinity mask AND cgroup quota) split over the ranks, never
            # omp_get_max_threads() -- a team larger than the quota stalls every layer's round trip (hostinfo.py)
            if not self.host_threads:
                self.host_threads = hostinfo.default_host_threads(self.dp.world if self.dp else 1)
            self.ctx.set_host_threads(self.host_threads)
            hostinfo.cap_torch_threads(self.host_threads)     # torch's own CPU ops of the token loop obey the same bound
        if self.pipe is None and n_gpu < sh.layers:
            torch.cuda.empty_cache()
            self.pipe = WeightPipeline(self.ctx, self.model, self.n_slots, self.dp)
        return self.hidden.get(B, T)

    def _split_decode_plan(self, s, kv_state):
        """(LIA_OPT_SPLIT_DECODE around this forward's layers, bytes of split-key scratch its workspace needs).  Only a forward with
        a decode-shaped GPU attention has either: a decode step with resident layers or a GPU-attention policy (0 / 3), by the rule of
        self.split_decode; a prefill whose last layer attends, for its last position only, more keys than the one-workgroup kernel
        holds.  The scratch is sized for the cache's positions, not the step's, so that a generation sizes its workspace once."""
        sh = self.model.shape
        kvh = getattr(sh, "kv_heads", sh.heads)
        gpu_attn = s.n_gpu > 0 or (s.policy in (0, 3) and not s.on_host)
        if not gpu_attn:
            return 0, 0
        Bc = s.B if s.n_gpu > 0 else s.mini        # rows of the largest attention launch
        S = s.pos0 + s.T
        if s.is_prefill:
            tail = self.prefill_tail and not s.every_pos and s.T > 1
            forced = tail and ops.split_decode_forced(sh.head_dim, sh.heads, kvh, S)
            return 0, (ops.split_scratch_bytes(Bc, S, sh.heads, kvh, sh.head_dim) if forced else 0)
        opt, split = ops.split_decode_for(self.split_decode, sh.head_dim, sh.heads, kvh, Bc, S)
        return opt, (ops.split_scratch_bytes(Bc, max(S, kv_state.smax), sh.heads, kvh, sh.head_dim) if split else 0)

    def _hold_caches(self, B, T, n_gpu):
        """Device holding caches [T, B, h, d] x 2 for every streamed layer (20.7 GB for OPT-30B at B = 64, T = 256), or None when
        HBM has no room for them (the deliveries then run beside the prefill as in r01)."""
        sh = self.model.shape
        key = (B, T, n_gpu)
        if self._kv_hold is not None and self._kv_hold[0] == key:
            return self._kv_hold[1]
        self._kv_hold = None
        need = 2 * (sh.layers - n_gpu) * T * B * sh.hidden * 2
        free, _ = torch.cuda.mem_get_info()
        if need > 0.5 * free:
            return None
        out = []
        for _ in range(n_gpu, sh.layers):
            k = torch.empty((T, B, sh.heads, sh.head_dim), dtype=torch.bfloat16, device="cuda")
            v = torch.empty_like(k)
            out.append((k, v, N.KV(k.data_ptr(), v.data_ptr(), T, B, 1)))
        self._kv_hold = (key, out)
        return out

    def _await_kv(self, kv_state, idx=None):
        """block until the deferred K/V delivery of layer idx (None: of every layer) has reached the host cache"""
        pend = getattr(kv_state, "pending", None)
        if not pend:
            return
        t0 = time.time()
        for i in ([idx] if idx is not None else sorted(pend)):
            t = pend.pop(i, None)
            if t is not None:
                N.check(self.ctx.lib.lia_kv_deliver_wait(self.ctx.handle, t), "lia_kv_deliver_wait")
                self._outstanding.pop(t, None)
        self.kv_delivery["host_wait_ms"] += 1e3 * (time.time() - t0)
        if not pend and self.kv_delivery.get("_issued_at") is not None:
            self.kv_delivery.pop("_issued_at")
            ms = ctypes.c_double()
            N.check(self.ctx.lib.lia_kv_deliver_batch_ms(self.ctx.handle, ctypes.byref(ms)), "lia_kv_deliver_batch_ms")
            self.kv_delivery["device_ms"] = ms.value          # first copy's start -> last copy's end on the delivery stream

    def _await_all_deliveries(self):
        """every outstanding delivery of this scheduler, whichever generation issued it: their copies read the shared holding
        caches on the D2H stream, which the compute stream is about to overwrite"""
        for t, (ref, idx) in list(self._outstanding.items()):
            N.check(self.ctx.lib.lia_kv_deliver_wait(self.ctx.handle, t), "lia_kv_deliver_wait")
            owner = ref()
            if owner is not None and getattr(owner, "pending", None):
                owner.pending.pop(idx, None)
        if self._outstanding:
            ms = ctypes.c_double()
            N.check(self.ctx.lib.lia_kv_deliver_batch_ms(self.ctx.handle, ctypes.byref(ms)), "lia_kv_deliver_batch_ms")   # close the timing batch
            self.kv_delivery.pop("_issued_at", None)
        self._outstanding.clear()

    # -- one forward -----------------------------------------------------------------------------------
    # forward = _validate (shapes and flags -> a step record) -> _place (host set, cache sides, layer tiers) -> embed ->
    # _run_layers (resident run, streamed / host-computed layers; policy 1: _host_layers) -> lm_head -> sampler -> _deliver (K/V
    # to the host caches, synchronize, the new cache length, the cooperative controller's sample).  Each phase reads and extends
    # the step record `s`; none reaches back.
    def forward(self, input_ids, kv_state, prefill_policy=1, decoding_policy=1, no_overlap=False, pin_weight=False,
                gpu_percentage=0, num_minibatch=1, enable_cxl=False, max_new_tokens=None, suppress_token=-1, cpu_layers=0,
                cpu_layers_start=None, sampler=None, append_policy=None, token_mask=None, logprobs=None, penalties=None):
        """cpu_layers (build-defined): with decoding policy 2, that many of the streamed layers run
        their decode step entirely on the host cores (policy 1, weights read in place) instead of crossing the link --
        the cooperative split of the reference taken per layer.  Prefill is unaffected (policy 0 for every layer).
        cpu_layers=-1: the count is chosen ONLINE (CoopController) from the measured decode steps, starting at cpu_layers_start
        (default: planner.plan_cpu_layers for this shape and box defaults).
        sampler (sampling.Sampler, generate(do_sample=True)): the returned ids are its draw from the logits instead of their argmax.
        A multi-token call on a NON-EMPTY cache appends its block at positions kv_state.len .. (generate(past=)): it goes by the
        prefill policy like every multi-token call, or by append_policy = 2 where the caches live on the host -- q, k, v of the
        block travel to the host attention instead of the cached prefix to the GPU (the one multi-token policy 2).
        token_mask (int32 CUDA [B, W] or one broadcast row [1, W], constraints.Constraint): the allowed-token table of this call's
        head -- set on the context around lm_head and the sampler, cleared behind them (lia_ctx_set_token_mask).
        logprobs (ops.LogprobRequest): the head also leaves, per row, the log-probability of the id it returns (the argmax, or the
        sampler's draw) and the request's n_top alternatives in the request's device tensors [B] / [B, n_top] -- the sink is set
        around lm_head and the sampler only (lia_ctx_set_logprob_sink).
        penalties (penalties.Penalties): the head picks its ids from the logits penalised under the generation's count table -- the
        queued counts run and the table is set on the context in front of lm_head, cleared behind the sampler
        (lia_ctx_set_penalties); the returned logits stay raw."""
        s = self._validate(input_ids, kv_state, prefill_policy, decoding_policy, no_overlap, gpu_percentage, num_minibatch, append_policy)
        self._place(s, kv_state, pin_weight, enable_cxl, max_new_tokens, cpu_layers, cpu_layers_start)
        m, sh, ctx = self.model, self.model.shape, self.ctx
        ids_dev = input_ids.to("cuda", non_blocking=False).contiguous()
        ctx.embed_into(ids_dev, m.embed_tokens, m.embed_positions, s.x, s.pos0, starts=self._key_starts_for(s.B)[1])
        if s.split_opt:
            ctx.set_option(N.LIA_OPT_SPLIT_DECODE, 1)
        try:
            if s.on_host:
                self._await_kv(kv_state)
                hidden = self._host_layers(s.x, kv_state, s.n_gpu, s.B, s.T, s.pos0)  # resident prefix on the GPU, the rest on the CPU
            else:
                hidden = self._run_layers(s, kv_state)
        finally:
            if s.split_opt:
                ctx.set_option(N.LIA_OPT_SPLIT_DECODE, 0)
        with ctx.head_modifiers(token_mask, logprobs, (s.B,), penalties):
            logits, nxt = ctx.lm_head(hidden, m.final_ln_w, m.final_ln_b, m.embed_tokens, sh.ln_eps, suppress_token)
            if sampler is not None:
                nxt = sampler(ctx, logits, suppress_token)
        self._deliver(s, kv_state)
        return logits, nxt

    def score(self, input_ids, kv_state, targets, prefill_policy=1, decoding_policy=1, no_overlap=False, pin_weight=False,
              gpu_percentage=0, num_minibatch=1, enable_cxl=False, append_policy=None, **_decode_only):
        """One prefill-shaped pass over input_ids [B, T] (T > 1, an empty kv_state sized for T: the caches are scratch) that returns
        (logprobs float32 [B, T], greedy ids int64 [B, T]) on the device: entry [b, t] is log p(targets[b, t] | ids[b, :t + 1]) and
        the greedy token at position t (targets: int64 [B, T], -1 = none -> 0.0).  The phases are forward()'s, with the last layer
        computing EVERY position for this call and lm_score in place of lm_head.  A policy-0 pass keeps the streamed layers' K/V
        in the HBM holding caches and SKIPS their delivery to the host caches: nothing is outstanding when the call returns.
        Decode-only flags (decoding_policy, cpu_layers, ...) are accepted and have no effect beyond naming where the cache lives
        (policy 3 wants 3 for both, as in forward).
        On a NON-EMPTY cache the block is appended at positions kv_state.len .. and scored against the cached context (entry [b, t]
        conditions on the context and ids[b, :t + 1]); the cache must hold len + T positions.  kv_state.len does NOT advance: the
        block's K/V rows land behind len and are dead, so many continuations can be scored against one context.  A fixed cpu_layers
        of the generation that owns the cache is passed through so that the layers keep their placement."""
        B, T = input_ids.shape
        if T < 2:
            raise ValueError(f"score: a block of at least two tokens (T={T}, cache length {kv_state.len})")
        if kv_state.len + T > kv_state.smax:
            raise ValueError(f"score: the cache holds {kv_state.smax} positions, the context {kv_state.len} + the block {T} need {kv_state.len + T}")
        if tuple(targets.shape) != (B, T):
            raise ValueError(f"score: targets has shape {tuple(targets.shape)}, input_ids {(B, T)}")
        len0 = kv_state.len
        s = self._validate(input_ids, kv_state, prefill_policy, decoding_policy, no_overlap, gpu_percentage, num_minibatch, append_policy)
        s.every_pos = True
        cpu_layers = max(0, int(_decode_only.get("cpu_layers") or 0)) if len0 else 0
        self._place(s, kv_state, pin_weight, enable_cxl, None, cpu_layers, None)
        m, sh, ctx = self.model, self.model.shape, self.ctx
        ids_dev = input_ids.to("cuda", non_blocking=False).contiguous()
        tgt_dev = targets.to(device="cuda", dtype=torch.int64).contiguous()
        ctx.embed_into(ids_dev, m.embed_tokens, m.embed_positions, s.x, s.pos0, starts=self._key_starts_for(s.B)[1])
        if s.on_host:
            hidden = self._host_layers(s.x, kv_state, s.n_gpu, s.B, s.T, s.pos0)
        else:
            hidden = self._run_layers(s, kv_state)
        lp, greedy = ctx.lm_score(hidden, m.final_ln_w, m.final_ln_b, m.embed_tokens, tgt_dev, sh.ln_eps)
        self._deliver(s, kv_state)
        if len0:
            kv_state.len = len0               # (an appended block is scored, not kept)
        return lp.view(B, T), greedy.view(B, T)

    def verify(self, block_ids, kv_state, suppress_token=-1, n_suppress=0, active=None, prefill_policy=1, decoding_policy=1,
               no_overlap=False, pin_weight=False, gpu_percentage=0, num_minibatch=1, enable_cxl=False, append_policy=None,
               sampler=None, return_logits=False, rejector=None, token_mask=None, logprobs=None, **_decode_only):
        """Speculative verification: one pass of the weights over block_ids [B, T] = [pending | d_1 .. d_{T-1}]
        appended at kv_state.len on a NON-EMPTY cache.  forward()'s phases with the last layer on every position, lm_verify in
        place of lm_head and LIA_OPT_BLOCK_ATTENTION set around the layers; the K/V rows are delivered as in forward().  Returns
        ops.VerifyResult (device tensors) and the number `common` of draft tokens every active row accepts; the new cache length
        is pos0 + common + 1 -- the rows behind it are dead and are rewritten by the next round (nothing is outstanding into them:
        _deliver has synchronised both streams and awaited the policy-0 stores).  suppress_token counts as -inf at block positions
        < n_suppress; active (int32 / bool [B] or None): rows with 0 never limit common.  A fixed cpu_layers is passed through as
        in score().  sampler (sampling.SamplerBlock, sampled verification): the head is lm_verify_sample -- res.greedy holds the
        draws of U[step + t, b], res.p_draft the chance of each to confirm the draft; return_logits (with a sampler, for tests and
        measurements) also returns the block's logits.  rejector (sampling.RejectorBlock, rejection verification of a stochastic
        drafter's block): the head is lm_verify_reject -- res.greedy holds `token`, res.ok / p_tok / q_tok / resid_mass the accept
        test.  Everything else is the same pass.  token_mask (int32 CUDA [B, T, W] or one broadcast row): the allowed-token table of
        the verify head, row (b, t) for block position t of row b; set around the head call only.  Not with a rejector.
        logprobs (ops.LogprobRequest): the verify head also leaves, per block position, the log-probability of ITS id there
        (res.greedy[b, t]) and the n_top alternatives in the request's device tensors [B, T] / [B, T, n_top].  Not with a rejector."""
        from . import speculative
        check_verify_block(block_ids, kv_state)
        B, T = block_ids.shape
        pos0 = kv_state.len
        s = self._validate(block_ids, kv_state, prefill_policy, decoding_policy, no_overlap, gpu_percentage, num_minibatch, append_policy)
        s.every_pos = s.verify = True
        cpu_layers = max(0, int(_decode_only.get("cpu_layers") or 0))
        self._place(s, kv_state, pin_weight, enable_cxl, None, cpu_layers, None)
        m, sh, ctx = self.model, self.model.shape, self.ctx
        ids_dev = block_ids.to(device="cuda", dtype=torch.int64).contiguous()
        act_dev = None if active is None else torch.as_tensor(active).to(device="cuda", dtype=torch.int32).contiguous()
        ctx.set_option(N.LIA_OPT_BLOCK_ATTENTION, int(speculative.block_attention_for(self, sh, B, T, pos0)))
        try:
            ctx.embed_into(ids_dev, m.embed_tokens, m.embed_positions, s.x, s.pos0, starts=self._key_starts_for(s.B)[1])
            if s.on_host:
                self._await_kv(kv_state)
                hidden = self._host_layers(s.x, kv_state, s.n_gpu, s.B, s.T, s.pos0)
            else:
                hidden = self._run_layers(s, kv_state)
        finally:
            ctx.set_option(N.LIA_OPT_BLOCK_ATTENTION, 0)
        with ctx.head_modifiers(token_mask, logprobs, (B, T)):
            res = verify_head(ctx, self._head(), hidden, ids_dev, act_dev, suppress_token, n_suppress, sampler=sampler, rejector=rejector,
                              return_logits=return_logits)
        self._deliver(s, kv_state)
        common = int(res.common.item())
        kv_state.len = pos0 + common + 1
        return res, common

    def _head(self):
        """verify_head's description of this model's head: (norm tensors, head weight, eps, family prefix of the ops.Context methods)"""
        m = self.model
        return (m.final_ln_w, m.final_ln_b), m.embed_tokens, m.shape.ln_eps, ""

    def verify_rows(self, block_ids, kv_state, row_lens, suppress_token=-1, n_suppress_rows=None, active=None, prefill_policy=1,
                    decoding_policy=1, no_overlap=False, pin_weight=False, gpu_percentage=0, num_minibatch=1, enable_cxl=False,
                    sampler=None, return_logits=False, **_decode_only):
        """verify() on a ragged cache (DESIGN.md 3.11, row mode): row b of block_ids [B, T] is appended at ITS cache length
        row_lens[b] (int32 [B]; the caller owns it).  Policies 3 / 3 only -- every layer's cache in HBM.  verify()'s phases with the
        library's row-length table (lia_ctx_set_row_lens) set around the embedding and the layer calls and cleared in a finally:
        while it is set every layer call is the ragged form (per-row positions, K/V scatter, ragged block attention), with
        max(row_lens) as the scalar position that sizes buffers.  num_minibatch > 1 serves slices of the table as it does of the key
        starts.  suppress_token counts as -inf at block positions < n_suppress_rows[b] (int32 [B] or None: zeros).  Returns
        ops.VerifyResult (device tensors); kv_state.len is NOT advanced.  sampler (sampling.SamplerBlock of block_rows) /
        return_logits: as in verify()."""
        row_lens = np.ascontiguousarray(np.asarray(row_lens, dtype=np.int32))
        flags = dict(prefill_policy=prefill_policy, decoding_policy=decoding_policy, cpu_layers=int(_decode_only.get("cpu_layers") or 0))
        sh = self.model.shape
        check_verify_rows(block_ids, kv_state, row_lens, flags, int(sh.layers * gpu_percentage / 100), sh.layers)
        B, T = block_ids.shape
        len0 = kv_state.len
        kv_state.len = int(row_lens.max())                 # the scalar position of the ragged calls: it sizes buffers only
        try:
            s = self._validate(block_ids, kv_state, prefill_policy, decoding_policy, no_overlap, gpu_percentage, num_minibatch)
            s.every_pos = s.verify = True
            self._place(s, kv_state, pin_weight, enable_cxl, None, 0, None)
            m, ctx = self.model, self.ctx
            ids_dev = block_ids.to(device="cuda", dtype=torch.int64).contiguous()
            act_dev = None if active is None else torch.as_tensor(active).to(device="cuda", dtype=torch.int32).contiguous()
            nsup = np.zeros(B, np.int32) if n_suppress_rows is None else np.ascontiguousarray(np.asarray(n_suppress_rows, dtype=np.int32))
            if nsup.shape != (B,) or (nsup < 0).any() or (nsup > T).any():
                raise ValueError(f"verify_rows: n_suppress_rows must hold one count in [0, T={T}] per row, got {nsup.tolist()}")
            nsup_dev = torch.from_numpy(nsup).to("cuda")
            lens_dev = torch.from_numpy(row_lens).to("cuda")
            ctx.set_row_lens(row_lens)
            try:
                ctx.embed_ragged_into(ids_dev, m.embed_tokens, m.embed_positions, s.x, lens_dev, starts=self._key_starts_for(B)[1])
                hidden = self._run_layers(s, kv_state)
            finally:
                ctx.set_row_lens(None)
            res = verify_head(ctx, self._head(), hidden, ids_dev, act_dev, suppress_token, n_suppress_rows=nsup_dev, sampler=sampler,
                              return_logits=return_logits)
            self._deliver(s, kv_state)
        finally:
            kv_state.len = len0
        return res

    # -- left-padded batches (generation.generate(..., attention_mask=)) -----------------------------------------------------
    def set_key_starts(self, starts):
        """starts: int32 [B] (row b's first real cache position) for every forward until the next call, or None: the unpadded
        route.  The library context keeps its own table (lia_ctx_set_key_starts: every GPU layer call and the policy-2 host
        attention read rows b0 .. b0 + B - 1 of it); the embedding and the host-computed layers take it from here."""
        if starts is None:
            self._key_starts = None
            if self.ctx is not None:
                N.check(self.ctx.lib.lia_ctx_set_key_starts(self.ctx.handle, None, 0), "lia_ctx_set_key_starts")
            return
        host = np.ascontiguousarray(np.asarray(starts, dtype=np.int32))
        self._key_starts = (host, None, None)
        if self.ctx is not None:
            self._upload_key_starts()

    def _upload_key_starts(self):
        host = self._key_starts[0]
        N.check(self.ctx.lib.lia_ctx_set_key_starts(self.ctx.handle, ctypes.c_void_p(host.ctypes.data), host.shape[0]),
                "lia_ctx_set_key_starts")
        self._key_starts = (host, torch.from_numpy(host).to("cuda"), self.ctx.handle)

    def _key_starts_for(self, B):
        """(host int32 [B], device int32 [B]) of the current generation, or (None, None).  Called behind _place, which may have
        created a new library context (a larger workspace): the table is uploaded to the context that serves this forward."""
        ks = self._key_starts
        if ks is None:
            return None, None
        if ks[2] is None or ks[2] != self.ctx.handle:
            self._upload_key_starts()
            ks = self._key_starts
        if ks[0].shape[0] != B:
            raise ValueError(f"the key-start table has {ks[0].shape[0]} rows, the forward {B}")
        return ks[:2]

    def _validate(self, input_ids, kv_state, prefill_policy, decoding_policy, no_overlap, gpu_percentage, num_minibatch, append_policy=None):
        """shapes and flags of one forward -> the step record; raises on the combinations the path does not have"""
        sh = self.model.shape
        B, T = input_ids.shape
        L = sh.layers
        n_gpu = int(L * gpu_percentage / 100)                      # lia/modeling_opt.py:1182
        is_prefill = T != 1                                        # :1186-1188
        policy = prefill_policy if is_prefill else decoding_policy
        # a multi-token block behind a non-empty cache goes by the prefill policy, or by append_policy = 2 (host caches only)
        is_append = is_prefill and kv_state.len > 0
        if append_policy is not None and append_policy not in (prefill_policy, 2):
            raise ValueError(f"append_policy {append_policy}: None (the prefill policy, {prefill_policy}) or 2")
        if is_append and append_policy == 2 and n_gpu < L:
            if kv_state.all_on_device:
                raise ValueError("append_policy 2 computes the block's attention on the host cores: the KV cache must live on the host, "
                                 "this generation keeps it in HBM (policy 3)")
            policy = 2
        if n_gpu < L and policy not in (0, 1, 2, 3):
            raise ValueError(f"unsupported policy {policy} (prefill: 0, 1 or 3; decode: 0, 1, 2 or 3)")
        if n_gpu < L and (policy == 3) != bool(kv_state.all_on_device):
            raise ValueError("policy 3 on streamed layers (KV cache in HBM, SURVEY.md section 8 f-1) must be chosen for BOTH "
                             "phases: the cache of a generation lives either in HBM or on the host")
        if is_prefill and policy == 2 and n_gpu < L and not is_append:
            raise ValueError("prefill policy must be 0 on the GPU path (the reference has no prefill-2 branch)")
        # :1178 mini_bsz = int(bsz / num_minibatch), looped num_minibatch times: the reference leaves the rows behind the last full
        # minibatch unwritten when the division has a remainder and computes nothing at all for num_minibatch > bsz -- both happen in
        # its own scripts (cxl_offloading.sh:37 `--batch-size 1150 --num-minibatch 3`, lia_offline.sh:27-29 `--batch-size 1
        # --num-minibatch 2`).  Here: the intended semantics -- num_minibatch clamped to the batch, the last
        # minibatch takes the remainder (minibatch_bounds)
        minis = minibatch_bounds(B, num_minibatch) if (policy in (0, 3) and is_prefill) or policy == 0 else [(0, B)]
        mini = max(n for _, n in minis)
        return SimpleNamespace(B=B, T=T, L=L, n_gpu=n_gpu, is_prefill=is_prefill, policy=policy, prefill_policy=prefill_policy,
                               decoding_policy=decoding_policy, gpu_percentage=gpu_percentage, mini=mini, minis=minis, overlap=not no_overlap,
                               pos0=kv_state.len, coop=None, cpu_set=frozenset(), host_act=frozenset(), host_now=frozenset(),
                               t_fwd0=None, busy0=0.0, hold=None, x=None, y=None,
                               every_pos=False,                          # a scoring pass (score): no last-position-only last layer, no K/V delivery
                               verify=False,                             # a verify pass of speculative decoding (verify): every_pos, K/V delivered
                               on_host=(policy == 1 and n_gpu < L))      # policy 1: the streamed layers run on the host cores (_host_layers)

    def _place(self, s, kv_state, pin_weight, enable_cxl, max_new_tokens, cpu_layers, cpu_layers_start):
        """the host-computed layer set (fixed or the online controller's), the side every cache lives on, the layers' tiers
        (move_gpu_layer / pin_memory, idempotent), the hidden-state buffers and the holding caches of a deferred K/V delivery"""
        m = self.model
        n_gpu, L, B, T, is_prefill, decoding_policy = s.n_gpu, s.L, s.B, s.T, s.is_prefill, s.decoding_policy
        # The policy-1 host path reads the host copy directly, so the packed wire format is only used when neither phase runs on the CPU.
        coop = None
        if cpu_layers and cpu_layers < 0 and decoding_policy in (2, 3) and self.dp is None and n_gpu < L - 1:
            coop = self._coop_controller(n_gpu, L, B, T, max_new_tokens, s.gpu_percentage, decoding_policy, cpu_layers_start)
            self._fit_host_candidates(coop, enable_cxl and pin_weight)
            cpu_set = coop.superset()                                # layers that keep a raw host copy (and a host KV cache)
        else:
            cpu_set = self.cpu_layer_set(n_gpu, L, cpu_layers) if (cpu_layers and cpu_layers > 0 and decoding_policy in (2, 3) and self.dp is None) else frozenset()
        if cpu_set and decoding_policy == 3:
            # the host-computed layers need their cache on the host; with the online count a candidate's cache follows the host set
            need_host = coop.host_set() if coop is not None else cpu_set
            fixed = [i for i in need_host if i not in getattr(kv_state, "dual", {}) and kv_state.kv[i].on_device]
            if fixed:
                raise ValueError("cpu_layers with the KV cache in HBM: the host-computed layers need a host cache "
                                 "(KVState(..., all_on_device=True, host_layers=OffloadScheduler.cpu_layer_set(...)), "
                                 f"dual_layers=... for the online count); layers {fixed[:4]}")
            if is_prefill and kv_state.len == 0:
                for i in getattr(kv_state, "dual", {}):                  # an empty cache changes sides for free
                    kv_state.move_cache(N.lib(), i, to_device=(i not in need_host))
        shard = (self.dp.rank, self.dp.world) if (self.dp is not None and self.dp.world > 1 and self.dp.mode == "allgather") else None
        wire, raw_set = placement_formats(s.prefill_policy, decoding_policy, self.wire, n_gpu, L, pin_weight, enable_cxl, cpu_set, self.dp is not None)
        res_fmt = self._resident_format(s, wire, coop, cpu_set)
        if m.placed_for != m._place_key(n_gpu, pin_weight, enable_cxl, wire, raw_set, shard, res_fmt):
            # the flags changed since the last placement: the model re-tiers its layers (policy 1 wants raw host copies,
            # another gpu%, wire format or host tier).  Copies in flight read host buffers that are about to be freed and
            # the cached device pointers of the resident layers go stale.
            self.resident.replaced(self.pipe)
        m.place(n_gpu, pin_weight, enable_cxl, wire, raw_layers=raw_set, shard=shard, resident_packed=res_fmt)
        if coop is not None and is_prefill:
            coop.new_sequence()                                      # the first decode step is not a sample of the steady state
        s.coop, s.cpu_set = coop, cpu_set
        s.host_act = coop.host_set() if coop is not None else cpu_set   # the layers whose DECODE step runs on the host cores
        s.host_now = s.host_act if not is_prefill else frozenset()    # layers this forward computes on the host
        if coop is not None and not is_prefill:
            s.t_fwd0, s.busy0 = time.time(), (self.pipe.poll_stats()[1] if self.pipe else 0.0)
        rows = B * T if n_gpu > 0 else s.mini * T                  # resident layers take the whole batch
        if s.decoding_policy == 0 and n_gpu < L:
            # policy-0 DECODE parks the cached prefix in a slab.  (Until r06 the test was on the PHASE's policy, so every policy-0
            # prefill sized the workspace for batch x max positions rows: 60 GB of HBM at batch 1050 x 288 positions, which is
            # what ran the planner's batch-1050 pick out of memory; the reference's scripts never use decode policy 0.)
            rows = max(rows, s.mini * kv_state.smax)
        if is_prefill and s.policy == 0 and s.pos0 > 0 and n_gpu < L:
            # a policy-0 block appended to a non-empty cache parks the cached prefix and its own rows in the slab: mini (pos0 + T) rows
            # (a verify pass sizes the slab for the whole cache once: pos0 grows every round, and a larger workspace is a new context)
            rows = max(rows, s.mini * (kv_state.smax if s.verify else s.pos0 + T))
        s.split_opt, split_bytes = self._split_decode_plan(s, kv_state)
        s.x, s.y = self._ensure(rows, B, T, n_gpu, score_rows=B * T if s.every_pos else 0, split_bytes=split_bytes)
        if is_prefill and s.policy == 0 and n_gpu < L and self.defer_kv and s.pos0 == 0:
            self._await_all_deliveries()          # (host-blocking: afterwards nothing on the D2H stream reads the holding caches)
            s.hold = self._hold_caches(B, T, n_gpu)

    def _resident_format(self, s, wire, coop, cpu_set):
        """10 where this placement holds its resident layers as their pack10 wire encoding, else 0 (raw): where the wire cache itself
        applies -- the streamed layers travel as pack10, no data parallelism, no host-computed layers, a decode policy that streams (2,
        3 or 0), and there are both resident and streamed layers.  Every other placement re-tiers the residents raw: policy 1, whose
        resident prefix runs from raw pointers, the cooperative split, data parallelism."""
        if not (self.resident_packed and self.wire_cache) or wire != 10 or self.dp is not None or coop is not None or cpu_set:
            return 0
        if s.decoding_policy not in (2, 3, 0) or s.prefill_policy == 1 or not (0 < s.n_gpu < s.L) or self.n_slots <= WeightPipeline.KEEP_SLOTS:
            return 0
        return 10

    def _run_layers(self, s, kv_state):
        """the decoder layers of one forward on the GPU path: the resident run, then every streamed layer behind its weight copy
        (or on the host cores, for the cooperative split's host set); returns the hidden state that feeds lm_head"""
        m, sh, ctx, pipe = self.model, self.model.shape, self.ctx, self.pipe
        B, T, L, n_gpu, is_prefill, policy, mini, overlap, pos0, hold = s.B, s.T, s.L, s.n_gpu, s.is_prefill, s.policy, s.mini, s.overlap, s.pos0, s.hold
        host_act, host_now, x, y = s.host_act, s.host_now, s.x, s.y
        # resident layers held packed take slots like streamed ones: the order starts (and wraps) at layer 0
        packed = frozenset(pipe.packed_residents()) if (pipe is not None and n_gpu > 0) else frozenset()
        wrap_to = 0 if packed else n_gpu
        raw_res = frozenset(range(n_gpu)) - packed if packed else frozenset()     # (layers pack10 refused: they need no slot)
        if n_gpu < L:
            self._set_wire_cache(s)
        if packed and is_prefill and not pipe.keep:
            pipe.trim_residents(min(packed))
        if n_gpu < L and overlap:
            pipe.prefetch(min(packed) if packed else n_gpu)        # no-op if the previous step already wrapped to it
        # the prefill's last layer: only hidden[:, -1, :] feeds lm_head (models.py:424-431), its K/V of every position feed decode
        tail_last = self.prefill_tail and not s.every_pos and is_prefill and T > 1 and (policy in (0, 3) or n_gpu == L) and (L - 1) not in host_now
        xlast = None
        first = 0
        if not is_prefill and n_gpu > 0 and not packed:
            # decode: the resident run (whole batch, everything on the GPU incl. KV -- policy 3; :1246-1260) in ONE library call
            # (lia_decode_layers: the per-op route layer by layer, or with LIA_FUSED_DECODE=1 an attention launch and a
            # persistent chain launch per layer, lia_chain.hip)
            wt, kvt = self.resident.decode_tables(n_gpu, kv_state)
            N.check(ctx.lib.lia_decode_layers(ctx.handle, ctypes.byref(m.desc), n_gpu, wt, ctypes.c_void_p(x.data_ptr()),
                                              ctypes.c_void_p(y.data_ptr()), kvt, B, pos0, ctypes.c_void_p(ctx.stream)), "lia_decode_layers")
            x, y = y, x
            first = n_gpu
        for idx in range(first, L):
            if idx in packed:
                # resident layer held packed: decoded into a slot (no copy), then as below
                if not overlap:
                    pipe.prefetch(idx)
                wptrs = pipe.acquire(idx)
                if overlap:
                    pipe.prefetch_ahead(idx, stream_order(idx, wrap_to, L, host_act | raw_res, skip_now=not is_prefill))
                if tail_last and idx == L - 1:
                    xlast = torch.empty((B, 1, sh.hidden), dtype=torch.bfloat16, device="cuda")
                    ctx.layer_forward_last(m.desc, 3, wptrs, x, xlast, kv_state.kv[idx], B, T, pos0, 0)
                else:
                    ctx.layer_forward(m.desc, 3, wptrs, x, y, kv_state.kv[idx], B, T, pos0, 0)
                    x, y = y, x
                pipe.release(idx)
                if not overlap:
                    ctx.synchronize()
                continue
            if idx < n_gpu:
                # resident layer: whole batch, everything on the GPU incl. KV (policy 3; :1246-1260)
                if tail_last and idx == L - 1:
                    xlast = torch.empty((B, 1, sh.hidden), dtype=torch.bfloat16, device="cuda")
                    ctx.layer_forward_last(m.desc, 3, self.resident.layer(idx), x, xlast, kv_state.kv[idx], B, T, pos0, 0)
                    continue
                ctx.layer_forward(m.desc, 3, self.resident.layer(idx), x, y, kv_state.kv[idx], B, T, pos0, 0)
                x, y = y, x
                continue
            if hold is None:
                self._await_kv(kv_state, idx)                      # a deferred K/V delivery of an earlier prefill: the host cache must be complete
            if idx in host_now:
                x, y = self._host_decode_layer(idx, x, y, kv_state, B, T, pos0)
                continue
            if not overlap:
                pipe.prefetch(idx)
            wptrs = pipe.acquire(idx)
            if overlap:
                # (decode forwards skip the host-computed layers; a prefill streams them all and skips them behind the wrap)
                pipe.prefetch_ahead(idx, stream_order(idx, wrap_to, L, host_act | raw_res, skip_now=not is_prefill))
            if policy in (0, 3):
                # FlexGen-style minibatches (:1283-1365).  Policy 3 here = streamed weights with the cache kept in HBM
                # (build-defined; the reference reserves 3 for resident layers, :1175-1176)
                # a host-computed layer keeps its cache on the host: its prefill delivers K/V there (policy 0) even when the
                # other streamed layers keep theirs in HBM (policy 3)
                kvl = kv_state.kv[idx]
                pol = 0 if (policy == 3 and not kvl.on_device) else policy
                if pol == 0 and not is_prefill and policy == 3:
                    pol = 2            # a host layer of the split that the GPU computes this step: its cache lives on the host
                if hold is not None and pol == 0:
                    pol, kvl = 3, hold[idx - n_gpu][2]             # same arithmetic, rows land in the HBM holding cache
                if tail_last and idx == L - 1:
                    xlast = torch.empty((B, 1, sh.hidden), dtype=torch.bfloat16, device="cuda")
                for b0, nb in s.minis:
                    sl = slice(b0, b0 + nb)
                    if tail_last and idx == L - 1:
                        ctx.layer_forward_last(m.desc, pol, wptrs, x[sl], xlast[sl], kvl, nb, T, pos0, b0)
                    else:
                        ctx.layer_forward(m.desc, pol, wptrs, x[sl], y[sl], kvl, nb, T, pos0, b0)
            else:
                ctx.layer_forward(m.desc, 2, wptrs, x, y, kv_state.kv[idx], B, T, pos0, 0)   # :1493-1543
            pipe.release(idx)
            x, y = y, x
            if not overlap:
                ctx.synchronize()
        return x if xlast is None else xlast

    # The least idle workspace worth lending to the wire cache.  Lending ties the entries to the kept size: a forward that needs
    # more costs a refill of every entry, and a workspace this small (a prefill of a few hundred rows of a small model) holds no
    # layer of a model that is worth streaming.
    WS_LEND_MIN_BYTES = 64 << 20

    SKINNY_ROWS = 256       # B x T up to which a forward's GEMMs run in the skinny, weight-bandwidth-bound regime (lia_gemm.hip)

    def _set_wire_cache(self, s):
        """Decode mode of the streamer, decided per forward: on for decode steps and for blocks in the skinny GEMM regime (verify
        passes, short appends), which are link-bound like a decode step; off before a prefill, a scoring pass or any block in the
        tiled regime, which get every slot back.  Not with data parallelism, and not under the cooperative split (cpu_layers != 0),
        whose host set moves between steps."""
        pipe = self.pipe
        if not self.wire_cache or self.dp is not None or s.coop is not None or s.cpu_set:
            if pipe.keep:
                pipe.set_decode_mode(None)
            return
        # a decode step, or a block behind a non-empty cache that is kept: an append or a verify pass, not a scoring pass
        step = not s.is_prefill or (s.pos0 > 0 and (s.verify or not s.every_pos))
        if step and s.B * s.T <= self.SKINNY_ROWS:
            if self.wire_cache_ws:
                # the mode's forwards keep what _ensure's formula gives the largest of them, so every chunk size and split-K choice
                # is the one a whole workspace gives; a forward that needs more re-configures (off, on, one refill of the entries)
                self._cache_keep = max(self._cache_keep, self._ws_need)
                idle = self.ctx.workspace_alloc_bytes - self._cache_keep
                pipe.configure_cache(idle >= self.WS_LEND_MIN_BYTES, self._cache_keep)
            else:
                pipe.configure_extra()
            pipe.set_decode_mode(range(s.n_gpu, s.L))
        else:
            pipe.set_decode_mode(None)

    def wire_cache_info(self, regions=False):
        """{"enabled", "on", "capacity" (layers), "layers" (bound to an entry, in order), "bytes" (wire bytes held in HBM)};
        regions: also "workspace" (the context's idle workspace may hold entries) and "regions", the entries of the mode that is on
        in the idle slots, the staging allocation, the workspace and the streamer's extra region (what packed residents save):
        {"slots", "staging", "workspace", "extra"}.  Resident layers are never among "layers": they hold no entry."""
        info = self.pipe.cache_info() if self.pipe else {"on": False, "capacity": 0, "layers": [], "bytes": 0}
        info = dict(info, enabled=self.wire_cache)
        if regions:
            info.update(workspace=self.wire_cache_ws,
                        regions=self.pipe.cache_regions() if self.pipe else {"slots": 0, "staging": 0, "workspace": 0, "extra": 0})
        return info

    def _deliver(self, s, kv_state):
        """behind lm_head: the deferred K/V deliveries of a policy-0 prefill (tickets, awaited per layer by the first decode
        step), the synchronisation the policy needs, the new cache length, and the cooperative controller's sample of the step"""
        sh, ctx, pipe = self.model.shape, self.ctx, self.pipe
        B, T, L, n_gpu, hold = s.B, s.T, s.L, s.n_gpu, s.hold
        if s.on_host:
            ctx.synchronize()                     # policy 1: nothing was delivered, the host layers wrote their caches themselves
        elif hold is not None and s.every_pos:
            ctx.synchronize()                     # a scoring pass: the K/V in the holding caches were scratch, nothing is delivered
        elif hold is not None:
            # the deferred deliveries, in the order the first decode step will need them; tickets are awaited per layer there
            self._await_kv(kv_state)              # (a KVState reused for a second prefill: never drop a ticket unawaited)
            kv_state.pending = {}
            self.kv_delivery = {"bytes": 0, "device_ms": None, "host_wait_ms": 0.0, "_issued_at": time.time()}
            for idx in range(n_gpu, L):
                if kv_state.kv[idx].on_device:
                    continue
                t = ctypes.c_int()
                N.check(ctx.lib.lia_kv_deliver(ctx.handle, ctypes.byref(hold[idx - n_gpu][2]), ctypes.byref(kv_state.kv[idx]), T,
                                               sh.hidden, ctypes.byref(t)), "lia_kv_deliver")
                kv_state.pending[idx] = t.value
                self._outstanding[t.value] = (weakref.ref(kv_state), idx)
                self.kv_delivery["bytes"] += 2 * T * B * sh.hidden * 2
            N.check(ctx.lib.lia_ctx_synchronize_compute(ctx.handle), "lia_ctx_synchronize_compute")
        else:
            ctx.synchronize()
            if s.policy == 0 or (s.is_prefill and s.cpu_set):
                ctx.kv_store_wait()                                # host cache complete before the next step reads it
        kv_state.len = s.pos0 + T
        coop = s.coop
        if s.t_fwd0 is not None:
            step_ms = 1e3 * (time.time() - s.t_fwd0)
            busy = (self.pipe.poll_stats()[1] - s.busy0) / max(step_ms, 1e-6) if self.pipe else 0.0
            before = coop.host_set()
            coop.observe(step_ms, min(busy, 1.0))
            after = coop.host_set()
            for li in after - before:                             # newly host-computed: a queued copy of it will never be used
                pipe.forget(li)
            if s.decoding_policy == 3 and after != before:
                # KV in HBM: the cache of a layer that changes sides follows it (0.5 GB per layer at the headline shape, ~10 ms)
                for li in sorted(after ^ before):
                    self._await_kv(kv_state, li)
                    self.kv_moved_bytes += kv_state.move_cache(ctx.lib, li, to_device=(li not in after))

    def _coop_controller(self, n_gpu, L, B, T, max_new_tokens, gpu_percentage, decoding_policy, start):
        key = (n_gpu, L, B, decoding_policy)
        if self._coop is None or self._coop_key != key:
            seeded_ok = start is None            # an explicit start (tests, LIA_COOP_START) is taken as given
            if start is None:
                start, _ = planner.plan_cpu_layers(self.model.shape, B, T, max_new_tokens or 32, gpu_percentage,
                                                   planner.Box(host_threads=self.host_threads or hostinfo.default_host_threads(1),
                                                               wire_ratio={0: 1.0, 10: 0.675}[self.wire]),
                                                   kv_in_hbm=(decoding_policy == 3))
            order = self.cpu_layer_order(n_gpu, L)
            sh = self.model.shape
            # everything that moves the optimum is in the key: the prompt length in buckets of a power of two (the host attention and
            # the caches' size scale with it), the new tokens, which tier the streamed layers live in
            tiers = sorted({st.tier for st in getattr(self.model, "layers", [])[n_gpu:] if getattr(st, "tier", None) not in ("device", None)}) or ["-"]
            t_bucket = 1 << max(0, int(T) - 1).bit_length()
            store_key = "|".join(str(v) for v in (sh.name, sh.hidden, sh.ffn, L, n_gpu, B, f"T<={t_bucket}", f"new{max_new_tokens or 0}", decoding_policy,
                                                  self.wire, "+".join(tiers), self.host_threads or hostinfo.default_host_threads(1)))
            kept = CoopStore.load(store_key) if seeded_ok else None
            if kept is not None:
                start = max(0, min(kept[0], len(order)))
            self._coop = CoopController(order, start, min(len(order), int(start) + COOP_HEADROOM))
            self._coop.store_key = store_key
            if kept is not None:
                # a count this box converged on before for exactly this configuration: the search starts ON it, but still opens with
                # the stride-3 probe (one candidate, on the side the link points to) before the +-1 round -- a stored count that is
                # wrong for today's box is left in two moves, not walked away from one count at a time
                self._coop.seeded = True
            self._coop_key = key
        return self._coop

    def _fit_host_candidates(self, coop, in_numa_tier, extra_per_layer=0, trim_pool=False):
        """Shrink the controller's candidate set to the raw host copies the container has room for (OPT-175B at gpu% = 5 in a
        300 GiB container: the planner's count + 10 does not fit, and the per-allocation guard would refuse the placement halfway
        through, in layer-index order -- a clustered host set).  A candidate in the NUMA tier swaps its packed copy for the raw
        one (growth = the difference, guard ceiling 0.93); a pinned one keeps both (growth = the raw bytes, ceiling 0.85).
        extra_per_layer: what else a candidate will pin (its host KV buffer when the caches otherwise live in HBM)."""
        layers = self.model.layers
        need = [k for k, li in enumerate(coop.order[:coop.c_max]) if layers[li].raw_host_ptr() is None and layers[li].tier != "remote"]
        if not need:
            return                                   # (every decode step comes through here: nothing to read once the copies exist)
        if trim_pool:
            PinnedPool.trim()                        # idle cache blocks of earlier generations count against the room
        mem = hostinfo.cgroup_memory()
        if mem["max"] is None or mem["current"] is None:
            return
        st = layers[coop.order[need[0]]]
        grow = ((st.nbytes - (st.stream_bytes if st.packed else 0)) if in_numa_tier else st.nbytes) + int(extra_per_layer)
        room = (0.93 if in_numa_tier else 0.85) * mem["max"] - mem["current"] - st.nbytes          # (one layer of slack: the guard looks at the transient)
        fit = max(0, int(room // max(grow, 1)))
        if fit < len(need):
            new_max = need[fit]                      # candidates before the first one that does not fit
            if new_max <= 0:
                # cpu_layers = -1 asks for "as many as pay": with no room for even one raw copy that is zero host layers -- the plain
                # streamed configuration -- not an aborted generation (a fixed cpu_layers > 0 never comes through here; its
                # placement fails in the allocation guard, loudly)
                warnings.warn(f"cooperative split: no room for a raw host copy of one layer ({st.nbytes / 2**30:.2f} GiB) in this "
                              "container; running with zero host-computed layers", RuntimeWarning, stacklevel=2)
            coop.restrict(max(new_max, 0))

    def host_team_report(self):
        return self.host.report()

    def coop_report(self):
        return self._coop.report() if self._coop is not None else None

    @staticmethod
    def cpu_layer_order(n_gpu, L):
        """A fixed NESTED order of the streamed layers (never the first one, which the wrap-around prefetch targets) whose every
        prefix is spread over the layer range: the candidates sorted by the bit-reversal of their position (van der Corput), so the
        host set can grow or shrink by one layer without moving the others and never holds runs of neighbours while it is small
        enough not to.  (A greedy farthest-point order looks as even for the first m / 3 picks and then fills one end of the range
        with neighbours: eight host layers in a row leave the copy engine idle, 426 vs 404 ms per step at 17 layers -- r03 results.)"""
        cand = list(range(n_gpu + 1, L))
        bits = max(1, (len(cand) - 1).bit_length())
        rev = lambda i: int(format(i, f"0{bits}b")[::-1], 2)      # noqa: E731
        return [cand[i] for i in sorted(range(len(cand)), key=rev)]

    @staticmethod
    def cpu_layer_set(n_gpu, L, count):
        """`count` host-computed layers spread evenly over the streamed ones (never the first streamed layer, which the
        wrap-around prefetch targets): while the host works on one of them the copy engine fills the free slots."""
        n_str = L - n_gpu
        count = max(0, min(int(count), n_str - 1))
        if count == 0:
            return frozenset()
        return frozenset(n_gpu + 1 + int((j + 0.5) * (n_str - 1) / count) for j in range(count))

    def new_kv_state(self, B, T, max_new_tokens, prefill_policy=1, decoding_policy=1, gpu_percentage=0, pin_weight=False,
                     enable_cxl=False, cpu_layers=0, cpu_layers_start=None, **_other):
        """The KV caches of one generation under generate()'s LIA flags, sized [T + new, B, h, d] like modeling_opt.py:1277-1278:
        in HBM for every layer when both policies are 3, except the cooperative split's host-computed layers (_place)."""
        sh = self.model.shape
        L = sh.layers
        n_gpu = int(L * gpu_percentage / 100)
        on_dev = prefill_policy == 3 and decoding_policy == 3
        host_layers, dual_layers = (), ()
        if on_dev and cpu_layers > 0:
            host_layers = self.cpu_layer_set(n_gpu, L, cpu_layers)
        elif on_dev and cpu_layers < 0 and self.dp is None and n_gpu < L - 1:
            # online count: every CANDIDATE host layer has a cache buffer on both sides; the cache lives where the layer is computed
            coop = self._coop_controller(n_gpu, L, B, T, max_new_tokens, gpu_percentage, 3, cpu_layers_start)
            # (before the caches are pinned: a candidate costs its raw weight copy AND its host cache buffer; while copies are
            # missing, the pooled blocks of an earlier generation with the caches on the host go back first -- with them in HBM
            # only the candidates need one)
            self._fit_host_candidates(coop, bool(enable_cxl and pin_weight),
                                      extra_per_layer=2 * (T + max_new_tokens) * B * sh.hidden * 2, trim_pool=True)
            host_layers, dual_layers = coop.host_set(), coop.superset()
        return KVState(self.model, n_gpu, B, T + max_new_tokens, all_on_device=on_dev, host_layers=host_layers, dual_layers=dual_layers)

    def _host_decode_layer(self, idx, x, y, kv_state, B, T, pos0):
        """One decode step of layer idx on the host cores (policy 1 for this layer): hidden state GPU -> pinned host by a
        kernel blit, lia_host_layer_forward on the raw host copy of the weights and the host KV cache, result back."""
        ctx, lib = self.ctx, self.ctx.lib
        raw = self.model.layers[idx].raw_host_ptr()
        if raw is None:
            raise ValueError(f"layer {idx} is to run on the host but has no raw bf16 host copy")
        nbytes = B * T * self.model.shape.hidden * 2
        hx, hy = self.host.hidden_pair(ctx, nbytes)
        N.check(lib.lia_blit(ctypes.c_void_p(hx), ctypes.c_void_p(x.data_ptr()), nbytes, ctypes.c_void_p(ctx.stream)), "lia_blit")
        ctx.synchronize()
        self.host.layer_forward(raw, kv_state.kv[idx], hx, hy, B, T, pos0, self.host.threads(self.host_threads),
                                self._key_starts_for(B)[0])
        N.check(lib.lia_blit(ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(hy), nbytes, ctypes.c_void_p(ctx.stream)), "lia_blit")
        return y, x

    def _host_layers(self, x, kv_state, n_gpu, B, T, pos0):
        """Policy 1 ("compute everything on CPU", lia/modeling_opt.py:1168, branches :1367-1377 / :1545-1555): layers
        [0, n_gpu) still run on the GPU (policy 3), the hidden state then moves to pinned host memory ONCE
        (:1262-1267) and every remaining layer runs on the host cores (lia_host_layer_forward) straight from the
        host copy of its weights -- nothing is streamed."""
        m, sh, ctx, lib = self.model, self.model.shape, self.ctx, self.ctx.lib
        y = torch.empty_like(x)
        for idx in range(n_gpu):
            ctx.layer_forward(m.desc, 3, self.resident.layer(idx), x, y, kv_state.kv[idx], B, T, pos0, 0)
            x, y = y, x
        ctx.synchronize()
        nbytes = B * T * sh.hidden * 2
        hx, hy = self.host.hidden_pair(ctx, nbytes)
        N.check(lib.lia_memcpy_d2h(ctypes.c_void_p(hx), ctypes.c_void_p(x.data_ptr()), nbytes), "lia_memcpy_d2h")
        threads = self.host.threads(self.host_threads, self.dp.world if self.dp else 1)
        host = list(range(n_gpu, sh.layers))
        raws = [m.layers[idx].raw_host_ptr() for idx in host]
        if None in raws:
            raise ValueError("policy 1 needs the raw bf16 host copy, but the streamed layers were pinned in the pack10 wire "
                             "format only by an earlier call; reload the model or set LIA_STREAM_FORMAT=raw")
        starts = self._key_starts_for(B)[0]
        if host and B * T <= 256:
            # a decode step: every host layer in ONE OpenMP region
            hx = self.host.layers_forward(host, raws, kv_state, hx, hy, B, T, pos0, threads, starts)
        else:
            for idx, raw in zip(host, raws):
                self.host.layer_forward(raw, kv_state.kv[idx], hx, hy, B, T, pos0, threads, starts)
                hx, hy = hy, hx
        N.check(lib.lia_memcpy_h2d(ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(hx), nbytes), "lia_memcpy_h2d")
        return x

    def stream_stats(self, reset=False):
        return self.pipe.stats(reset) if self.pipe else (0.0, 0.0)

    def decode_stats(self, reset=False, block=True):
        return self.pipe.decode_stats(reset, block) if self.pipe else {"launches": 0, "ms": 0.0, "bytes_in": 0.0, "bytes_out": 0.0}

    def close(self):
        if self.pipe:
            self.pipe.close()
            self.pipe = None
        if self.ctx:
            self._await_all_deliveries()
            self.host.release_hidden(self.ctx)
            self.ctx.close()
            self.ctx = None
