"""Llama-family model + scheduler (BASELINE.json config 4: Llama-3-8B, gpu%=100, bs=128, in 1024 / out 128).

A build-defined extension: in the reference only OPT carries the LIA policies (LlamaDecoderLayer_forward takes no
`policy`, decoder.py:121-169; gpu_percentage=100 never copies activations back, lia/modeling_opt.py:1262-1267 --
SURVEY.md quirk 3).  Semantics chosen here: layers [0, n_gpu) are HBM-resident; the remaining ones stream their packed
weights through the same WeightPipeline; the KV cache of every layer lives in HBM (the host-attention policies are
OPT-only), i.e. every layer runs "policy 3" arithmetic.  Arithmetic = HF transformers' eager bf16 Llama.
"""
import ctypes
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _native as N
from . import hostinfo, ops
from .kvcache import KV_SERIAL
from .model import LayerStore
from .scheduler import HeadModifierHooks, check_verify_block, default_stream_format, minibatch_bounds, verify_head, wire_format_code
from .streaming import HiddenPairs, ResidentRun, WeightPipeline, stream_order

LLAMA_TENSORS = ("in_norm_w", "q_w", "k_w", "v_w", "o_w", "post_norm_w", "gate_w", "up_w", "down_w")


@dataclass(frozen=True)
class LlamaShape:
    name: str
    hidden: int
    heads: int
    kv_heads: int
    ffn: int
    layers: int
    vocab: int
    max_pos: int = 8192
    rope_theta: float = 500000.0
    rms_eps: float = 1e-5

    @property
    def head_dim(self):
        return self.hidden // self.heads


LLAMA_SHAPES = {s.name: s for s in (
    LlamaShape("llama-3-8b", 4096, 32, 8, 14336, 32, 128256),
    LlamaShape("llama-2-7b", 4096, 32, 32, 11008, 32, 32000, max_pos=4096, rope_theta=10000.0),
)}


def resolve_llama_shape(name):
    key = name.lower().split("/")[-1].replace("meta-", "")
    if key not in LLAMA_SHAPES:
        raise ValueError(f"unknown Llama shape {name!r}; known: {sorted(LLAMA_SHAPES)}")
    return LLAMA_SHAPES[key]


GU_BLOCK = 32      # lia_hip.h, lia_llama_desc.gu_block


def interleave_gate_up(gate, up, block=GU_BLOCK):
    """[F, H] gate.w and up.w -> the [2F, H] block of the layer buffer: `block` gate rows, the matching `block` up rows, ..."""
    F, H = gate.shape
    assert up.shape == (F, H) and F % block == 0
    return np.stack([gate.reshape(F // block, block, H), up.reshape(F // block, block, H)], axis=1).reshape(2 * F, H)


def rope_tables(max_pos, d, theta):
    """cos/sin [max_pos, d] in bf16, computed like LlamaRotaryEmbedding.forward: fp32 inv_freq, fp32 angles, cast."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, d, 2, dtype=torch.int64).float() / d))
    freqs = torch.outer(torch.arange(max_pos, dtype=torch.float32), inv_freq)
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().to(torch.bfloat16).cuda(), emb.sin().to(torch.bfloat16).cuda()


class LiaLlamaModel:
    family = "llama"

    def __init__(self, shape):
        self.shape = shape
        # gate.w / up.w live interleaved in the layer buffer, 32 gate rows then the matching 32 up rows (lia_hip.h, gu_block): a
        # 64-column tile of the gate|up projection then holds both factors of 32 outputs and the prefill GEMM's epilogue
        # writes silu(gate) * up itself.  The model is the same function of the same weights; only their order in memory differs.
        self.desc = N.LlamaDesc(shape.hidden, shape.heads, shape.kv_heads, shape.ffn, shape.rms_eps, GU_BLOCK)
        offs = (ctypes.c_size_t * 9)()
        total = ctypes.c_size_t()
        N.check(N.lib().lia_llama_pack_offsets(ctypes.byref(self.desc), ctypes.byref(offs), ctypes.byref(total)), "lia_llama_pack_offsets")
        self.offsets, self.layer_bytes = list(offs), total.value
        self.layers = [LayerStore(self.desc, self.offsets, self.layer_bytes) for _ in range(shape.layers)]
        self.embed_tokens = self.lm_head = self.final_norm_w = None
        self.placed_for = None

    def _pack_numpy(self, st, tensors):
        flat = np.zeros(self.layer_bytes, np.uint8)
        F, H = self.shape.ffn, self.shape.hidden
        gi, ui = LLAMA_TENSORS.index("gate_w"), LLAMA_TENSORS.index("up_w")
        assert self.offsets[ui] == self.offsets[gi] + F * H * 2, "gate.w and up.w must be adjacent in the layer buffer"
        for i, n in enumerate(LLAMA_TENSORS):
            if n == "up_w":
                continue                                   # written together with gate_w
            a = np.ascontiguousarray(tensors[n], dtype=np.uint16)
            if n == "gate_w":
                a = interleave_gate_up(a.reshape(F, H), np.ascontiguousarray(tensors["up_w"], dtype=np.uint16).reshape(F, H))
            a = a.reshape(-1).view(np.uint8)
            flat[self.offsets[i]: self.offsets[i] + a.size] = a
        st._free()
        st._np, st.tier = flat, "pageable"

    @classmethod
    def from_numpy(cls, shape, m):
        self = cls(shape)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(torch.bfloat16).cuda()  # noqa: E731
        self.embed_tokens, self.lm_head, self.final_norm_w = dev(m["embed_tokens"]), dev(m["lm_head"]), dev(m["final_norm_w"])
        for st, lw in zip(self.layers, m["layers"]):
            self._pack_numpy(st, lw)
        return self

    @classmethod
    def random_init(cls, shape, seed=0, n_gpu_layers=None, pin_weight=True, pack=0):
        """pack = 0 / 10: wire format of the pinned streamed layers (lia_pack10.hip), as for the OPT model"""
        self = cls(shape)
        n_gpu = shape.layers if n_gpu_layers is None else n_gpu_layers
        hostinfo.check_host_allocation((shape.layers - n_gpu) * self.layer_bytes, f"{shape.name}: streamed layers")
        g = torch.Generator(device="cuda")
        g.manual_seed(seed * 100003)
        H, F, KD = shape.hidden, shape.ffn, shape.kv_heads * shape.head_dim
        draw = lambda *s: (0.02 * torch.randn(*s, generator=g, device="cuda", dtype=torch.float32)).to(torch.bfloat16)  # noqa: E731
        self.embed_tokens, self.lm_head = draw(shape.vocab, H), draw(shape.vocab, H)
        self.final_norm_w = torch.ones(H, dtype=torch.bfloat16, device="cuda")
        dims = {"q_w": (H, H), "k_w": (KD, H), "v_w": (KD, H), "o_w": (H, H), "gate_w": (F, H), "up_w": (F, H), "down_w": (H, F)}
        for li, st in enumerate(self.layers):
            g.manual_seed(seed * 100003 + li + 1)
            flat = torch.zeros(self.layer_bytes // 2, dtype=torch.bfloat16, device="cuda")
            for i, n in enumerate(LLAMA_TENSORS):
                o = self.offsets[i] // 2
                if n in dims:
                    r, c = dims[n]
                    flat[o:o + r * c] = draw(r, c).reshape(-1)
                else:
                    flat[o:o + H] = 1.0
            st.set_from_device(flat.view(torch.uint8))
            if li >= n_gpu:
                st.to_pinned(pack)
        torch.cuda.synchronize()
        self.placed_for = (n_gpu, True, False, LayerStore._fmt_of(pack))
        return self

    def place(self, n_gpu_layers, pin_weight, enable_cxl, pack=0):
        """as LiaOPTModel.place: idempotent per flag set, re-places the layers when the flags change"""
        key = (n_gpu_layers, bool(pin_weight), bool(enable_cxl), LayerStore._fmt_of(pack))
        if self.placed_for == key:
            return
        for i, st in enumerate(self.layers):
            if i < n_gpu_layers:
                st.to_device()
        for i, st in enumerate(self.layers):
            if i < n_gpu_layers:
                continue
            if enable_cxl and pin_weight:
                st.to_cxl(pack)
            elif pin_weight:
                st.to_pinned(pack)
            elif st.tier == "device" or st.packed:
                st.to_pageable()
        torch.cuda.synchronize()
        self.placed_for = key

    def close(self):
        for st in self.layers:
            st.close()


class LlamaKVState:
    def __init__(self, model, B, smax):
        sh = model.shape
        self.B, self.smax, self.len = B, smax, 0
        self.serial, self.version = next(KV_SERIAL), 0
        self.tensors, self.kv = [], []
        for _ in range(sh.layers):
            k = torch.empty((smax, B, sh.kv_heads, sh.head_dim), dtype=torch.bfloat16, device="cuda")
            v = torch.empty_like(k)
            self.tensors.append((k, v))
            self.kv.append(N.KV(k.data_ptr(), v.data_ptr(), smax, B, 1))


class LlamaScheduler(HeadModifierHooks):
    """forward(ids, kv, gpu_percentage=..., num_minibatch=...) -> (logits, next ids) on the device."""

    def __init__(self, model, device=0, n_slots=4, pack=None, split_decode=None):
        self.model, self.device, self.n_slots = model, device, n_slots
        # a decode step's attention: OffloadScheduler.split_decode ("measured" / True / False; LIA_SPLIT_DECODE)
        self.split_decode = ops.split_decode_mode(os.environ.get("LIA_SPLIT_DECODE") if split_decode is None else split_decode,
                                                  "LIA_SPLIT_DECODE" if split_decode is None else "split_decode")
        fmt = default_stream_format() if pack is None else pack
        self.pack = wire_format_code(fmt)
        self.ctx = self.pipe = None
        self.hidden, self.resident, self.tables = HiddenPairs(model.shape.hidden), ResidentRun(model), None
        self.prefill_tail = True      # last layer of a prefill: last position only behind q|k|v (False: every position)
        self.block_attention = "measured"     # a verify pass's attention: OffloadScheduler.block_attention

    def _ensure(self, rows, B, T, n_gpu, smax, score_rows=0, split_bytes=0):
        """split_bytes: the split-key attention scratch of a forward that takes that route, behind the layer call's own layout"""
        sh, lib = self.model.shape, N.lib()
        lm_bytes = 2 * 256 * sh.hidden + 8 * min(B, 256) * sh.vocab * 4 + (1 << 20)
        need = max(lib.lia_llama_workspace_bytes(ctypes.byref(self.model.desc), rows) + split_bytes, lm_bytes)
        if score_rows:       # a scoring pass: room for one chunk of lia_llama_lm_score (normed rows + bf16 logits)
            need = max(need, lib.lia_lm_score_workspace_bytes(score_rows, sh.hidden, sh.vocab))
        if self.ctx is None or need > self.ctx.workspace_bytes:
            if self.pipe:
                self.pipe.close()
                self.pipe = None
            if self.ctx:
                self.ctx.close()
            self.ctx = ops.Context(self.device, need)
            hostinfo.cap_torch_threads()      # the token loop's CPU tensor ops: see hostinfo.cap_torch_threads
        if self.pipe is None and n_gpu < sh.layers:
            self.pipe = WeightPipeline(self.ctx, self.model, self.n_slots)
        if self.tables is None or self.tables[0].shape[0] < smax:
            self.tables = rope_tables(max(smax, 64), sh.head_dim, sh.rope_theta)
        return self.hidden.get(B, T)

    def forward(self, input_ids, kv_state, gpu_percentage=100, num_minibatch=1, pin_weight=True, enable_cxl=False,
                suppress_token=-1, sampler=None, token_mask=None, logprobs=None, penalties=None, **_ignored):
        """sampler (sampling.Sampler, generate(do_sample=True)): the returned ids are its draw from the logits instead of their argmax.
        token_mask (int32 CUDA [B, W] or one broadcast row, constraints.Constraint): the allowed-token table of this call's head,
        set on the context around lm_head and the sampler only (lia_ctx_set_token_mask).  logprobs (ops.LogprobRequest): as
        OffloadScheduler.forward -- the log-probability of every returned id and its n_top alternatives, in the request's tensors.
        penalties (penalties.Penalties): as OffloadScheduler.forward -- the ids come from the logits penalised under the
        generation's count table, set on the context around the head only."""
        m, sh = self.model, self.model.shape
        B, T = input_ids.shape
        x, xlast = self._layers(input_ids, kv_state, gpu_percentage, num_minibatch, pin_weight, enable_cxl)
        ctx = self.ctx
        with ctx.head_modifiers(token_mask, logprobs, (B,), penalties):
            # (xlast: the last layer already reduced the block to its last position)
            logits, nxt_ids = ctx.llama_lm_head(x if xlast is None else xlast, m.final_norm_w, m.lm_head, sh.rms_eps, suppress_token)
            if sampler is not None:
                nxt_ids = sampler(ctx, logits, suppress_token)
        ctx.synchronize()
        kv_state.len += T
        return logits, nxt_ids

    def score(self, input_ids, kv_state, targets, gpu_percentage=100, num_minibatch=1, pin_weight=True, enable_cxl=False, **_ignored):
        """One prefill-shaped pass over input_ids [B, T] (T > 1, an empty kv_state sized for T: scratch) -> (logprobs float32 [B, T],
        greedy ids int64 [B, T]) on the device: log p(targets[b, t] | ids[b, :t + 1]) (targets int64 [B, T], -1 = none -> 0.0) and the
        greedy token at t.  forward()'s prefill with the last layer on every position, then lia_llama_lm_score.
        On a NON-EMPTY cache the block is appended at kv_state.len .. and scored against the cached context; kv_state.len does not
        advance (the block's K/V rows behind len are dead), the cache must hold len + T positions."""
        m, sh = self.model, self.model.shape
        B, T = input_ids.shape
        if T < 2:
            raise ValueError(f"score: a block of at least two tokens (T={T}, cache length {kv_state.len})")
        if kv_state.len + T > kv_state.smax:
            raise ValueError(f"score: the cache holds {kv_state.smax} positions, the context {kv_state.len} + the block {T} need {kv_state.len + T}")
        len0 = kv_state.len
        if tuple(targets.shape) != (B, T):
            raise ValueError(f"score: targets has shape {tuple(targets.shape)}, input_ids {(B, T)}")
        x, _ = self._layers(input_ids, kv_state, gpu_percentage, num_minibatch, pin_weight, enable_cxl, every_pos=True)
        tgt_dev = targets.to(device="cuda", dtype=torch.int64).contiguous()
        lp, greedy = self.ctx.llama_lm_score(x, m.final_norm_w, m.lm_head, tgt_dev, sh.rms_eps)
        self.ctx.synchronize()
        kv_state.len = len0 + T if len0 == 0 else len0
        return lp.view(B, T), greedy.view(B, T)

    def verify(self, block_ids, kv_state, suppress_token=-1, n_suppress=0, active=None, gpu_percentage=100, num_minibatch=1,
               pin_weight=True, enable_cxl=False, sampler=None, return_logits=False, rejector=None, token_mask=None, logprobs=None,
               **_ignored):
        """Speculative verification: OffloadScheduler.verify for a Llama -- the block [pending | draft] appended at kv_state.len,
        every position through the last layer with the block attention kernel, lia_llama_lm_verify; -> (ops.VerifyResult, common),
        kv_state.len = pos0 + common + 1.  sampler / return_logits / rejector: sampled and rejection verification, as
        OffloadScheduler.verify.  token_mask (int32 CUDA [B, T, W] or one broadcast row): the verify head's allowed-token table.
        logprobs (ops.LogprobRequest): the head's own id of every block position with its log-probability and alternatives."""
        check_verify_block(block_ids, kv_state)
        m, sh = self.model, self.model.shape
        pos0 = kv_state.len
        try:
            x, _ = self._layers(block_ids, kv_state, gpu_percentage, num_minibatch, pin_weight, enable_cxl, every_pos=True,
                                block_attention=True)
        finally:
            if self.ctx is not None:
                self.ctx.set_option(N.LIA_OPT_BLOCK_ATTENTION, 0)
        ids_dev = block_ids.to(device="cuda", dtype=torch.int64).contiguous()
        act_dev = None if active is None else torch.as_tensor(active).to(device="cuda", dtype=torch.int32).contiguous()
        with self.ctx.head_modifiers(token_mask, logprobs, tuple(block_ids.shape)):
            res = verify_head(self.ctx, ((m.final_norm_w,), m.lm_head, sh.rms_eps, "llama_"), x, ids_dev, act_dev, suppress_token, n_suppress,
                              sampler=sampler, rejector=rejector, return_logits=return_logits)
        self.ctx.synchronize()
        common = int(res.common.item())
        kv_state.len = pos0 + common + 1
        return res, common

    def _layers(self, input_ids, kv_state, gpu_percentage, num_minibatch, pin_weight, enable_cxl, every_pos=False,
                block_attention=False):
        """embedding and every decoder layer of one forward -> (hidden [B, T, H], the last layer's [B, 1, H] output when it computed the
        last position only, else None).  every_pos (a scoring pass): the last layer computes every position."""
        m, sh = self.model, self.model.shape
        lib = N.lib()
        B, T = input_ids.shape
        L = sh.layers
        n_gpu = L if gpu_percentage >= 100 else int(L * gpu_percentage / 100)
        minis = minibatch_bounds(B, num_minibatch) if T > 1 else [(0, B)]      # ragged last minibatch, num_minibatch clamped to B
        mini = max(n for _, n in minis)
        if m.placed_for != (n_gpu, bool(pin_weight), bool(enable_cxl), LayerStore._fmt_of(self.pack)):
            self.resident.replaced(self.pipe)
        m.place(n_gpu, pin_weight, enable_cxl, self.pack)
        pos0 = kv_state.len
        # the split-key route of a decode-shaped attention (OffloadScheduler._split_decode_plan): a decode step by the rule of
        # self.split_decode, a prefill's last-position-only last layer where the one-workgroup kernel cannot hold its keys
        split_opt, split_bytes = 0, 0
        if T == 1:
            split_opt, split = ops.split_decode_for(self.split_decode, sh.head_dim, sh.heads, sh.kv_heads, mini, pos0 + 1)
            split_bytes = ops.split_scratch_bytes(mini, max(pos0 + 1, kv_state.smax), sh.heads, sh.kv_heads, sh.head_dim) if split else 0
        elif self.prefill_tail and not every_pos and ops.split_decode_forced(sh.head_dim, sh.heads, sh.kv_heads, pos0 + T):
            split_bytes = ops.split_scratch_bytes(mini, pos0 + T, sh.heads, sh.kv_heads, sh.head_dim)
        x, y = self._ensure(mini * T, B, T, n_gpu, kv_state.smax, score_rows=B * T if every_pos else 0, split_bytes=split_bytes)
        ctx, pipe = self.ctx, self.pipe
        st = ctypes.c_void_p(ctx.stream)
        if split_opt:
            ctx.set_option(N.LIA_OPT_SPLIT_DECODE, 1)
        try:
            return self._run_layers(input_ids, kv_state, x, y, n_gpu, minis, mini, every_pos, block_attention)
        finally:
            if split_opt:
                ctx.set_option(N.LIA_OPT_SPLIT_DECODE, 0)

    def _run_layers(self, input_ids, kv_state, x, y, n_gpu, minis, mini, every_pos, block_attention):
        """the embedding and the layer calls of _layers, on the context and buffers it prepared"""
        m, sh = self.model, self.model.shape
        lib = N.lib()
        B, T = input_ids.shape
        L = sh.layers
        ctx, pipe = self.ctx, self.pipe
        st = ctypes.c_void_p(ctx.stream)
        pos0 = kv_state.len
        cos, sin = self.tables
        if block_attention:          # (verify: set on the context that serves this call; the caller clears it)
            from . import speculative
            ctx.set_option(N.LIA_OPT_BLOCK_ATTENTION, int(speculative.block_attention_for(self, sh, B, T, pos0)))
        ids_dev = input_ids.to("cuda").contiguous()
        N.check(lib.lia_llama_embed(ctypes.c_void_p(ids_dev.data_ptr()), ctypes.c_void_p(m.embed_tokens.data_ptr()),
                                    ctypes.c_void_p(x.data_ptr()), B, T, sh.hidden, st), "lia_llama_embed")
        if n_gpu < L:
            pipe.prefetch(n_gpu)
        resident = self.resident.layer
        xlast = None
        first = 0
        if T == 1 and n_gpu > 0 and mini == B:
            # decode: the resident run in ONE library call (lia_llama_decode_layers: the per-op route layer by layer with the chained
            # norms, or with LIA_FUSED_DECODE=1 an attention launch and a persistent chain launch per layer, lia_chain.hip)
            wt, kvt = self.resident.decode_tables(n_gpu, kv_state)
            N.check(lib.lia_llama_decode_layers(ctx.handle, ctypes.byref(m.desc), n_gpu, wt, ctypes.c_void_p(x.data_ptr()),
                                                ctypes.c_void_p(y.data_ptr()), kvt, ctypes.c_void_p(cos.data_ptr()),
                                                ctypes.c_void_p(sin.data_ptr()), B, pos0, st), "lia_llama_decode_layers")
            x, y = y, x
            first = n_gpu
        for idx in range(first, L):
            if idx < n_gpu:
                w = resident(idx)
                if T == 1 and idx + 1 < n_gpu:
                    ctx.chain_next_norm(resident(idx + 1)[0])      # decode: the next layer's input RMSNorm rides in this layer's down-proj combine
            else:
                w = pipe.acquire(idx)
                pipe.prefetch_ahead(idx, stream_order(idx, n_gpu, L))
            tail = self.prefill_tail and not every_pos and T > 1 and idx == L - 1
            if tail:
                xlast = torch.empty((B, 1, sh.hidden), dtype=torch.bfloat16, device="cuda")
            fn = lib.lia_llama_layer_forward_last if tail else lib.lia_llama_layer_forward
            for b0, nb in minis:
                sl = slice(b0, b0 + nb)
                N.check(fn(ctx.handle, ctypes.byref(m.desc), ctypes.byref(w), ctypes.c_void_p(x[sl].data_ptr()),
                           ctypes.c_void_p((xlast if tail else y)[sl].data_ptr()), ctypes.byref(kv_state.kv[idx]),
                           ctypes.c_void_p(cos.data_ptr()), ctypes.c_void_p(sin.data_ptr()), nb, T, pos0, b0, st),
                        "lia_llama_layer_forward")
            if idx >= n_gpu:
                pipe.release(idx)
            x, y = y, x
        return x, xlast

    def stream_stats(self, reset=False):
        return self.pipe.stats(reset) if self.pipe else (0.0, 0.0)

    def close(self):
        if self.pipe:
            self.pipe.close()
            self.pipe = None
        if self.ctx:
            self.ctx.close()
            self.ctx = None
