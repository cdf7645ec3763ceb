"""torch-tensor front end of the C ABI: the GPU sub-layer ops of decoder.py / attentions.py.

torch provides device memory and stream handles only; all arithmetic happens in liblia_hip.so.
Every function takes contiguous bf16 CUDA tensors (int64 for ids) and launches on `stream`
(a raw hipStream_t as int; default = the context's compute stream).
"""
import collections
import contextlib
import ctypes

import torch

from . import _native as N

LAYER_TENSORS = (
    "ln1_w", "ln1_b", "q_w", "q_b", "k_w", "k_b", "v_w", "v_b",
    "out_w", "out_b", "ln2_w", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b",
)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _chk(t, dtype=torch.bfloat16):
    if t is None:
        return
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"expected a contiguous {dtype} CUDA tensor, got {t.dtype} {t.device} contiguous={t.is_contiguous()}")


def _chk_logits(logits, rows_name="M"):
    """logits [rows, vocab] as the bare head kernels take them (rows may be strided) -> (rows, vocab)"""
    if not logits.is_cuda or logits.dtype != torch.bfloat16 or logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError(f"logits: expected a [{rows_name}, vocab] bf16 CUDA tensor with unit column stride, got {logits.dtype} {logits.device} "
                         f"shape {tuple(logits.shape)} strides {logits.stride()}")
    return logits.shape


# lia_lm_verify's outputs, all on the device: greedy int64 [B, T], accepted int32 [B], common int32 [1], next int64 [B].  On the
# sampled route (lia_lm_verify_sample) `greedy` holds the SAMPLED ids, p_draft is float32 [B, T] and logits bf16 [B, T, vocab], each
# where it was asked for.
# On the rejection route (lia_lm_verify_reject) `greedy` holds `token` -- per position the residual draw, the bonus draw at T - 1 -- and
# ok is int32 [B, T], p_tok / q_tok / resid_mass float32 [B, T] where asked for.
VerifyResult = collections.namedtuple("VerifyResult", "greedy accepted common next logits p_draft ok p_tok q_tok resid_mass",
                                      defaults=(None,) * 6)


LOGPROB_MAX_TOP = 32       # LIA_LOGPROB_MAX_TOP (include/lia_hip.h)


class LogprobRequest:
    """forward(logprobs=) / verify(logprobs=): ask the head of that one call for the log-probability of every id it emits and the
    n_top most likely tokens beside it, under the model's own distribution (lia_ctx_set_logprob_sink).  After the call: chosen
    (float32 [rows...]), top_ids (int64 [rows..., n_top]) and top_logprobs (float32 [rows..., n_top]) on the device -- rows... is [B]
    behind forward, [B, T] behind verify."""

    def __init__(self, n_top):
        self.n_top = int(n_top)
        self.chosen = self.top_ids = self.top_logprobs = None

    def allocate(self, shape, device):
        shape = tuple(int(d) for d in shape)
        self.chosen = torch.empty(shape, dtype=torch.float32, device=device)
        self.top_ids = torch.empty(shape + (self.n_top,), dtype=torch.int64, device=device)
        self.top_logprobs = torch.empty(shape + (self.n_top,), dtype=torch.float32, device=device)
        return self


class Context:
    """lia_ctx: compute stream + D2H stream + per-layer workspace (include/lia_hip.h)."""

    def __init__(self, device=0, workspace_bytes=0):
        self.lib = N.lib()
        h = ctypes.c_void_p()
        N.check(self.lib.lia_ctx_create(device, workspace_bytes, ctypes.byref(h)), "lia_ctx_create")
        self.handle = h
        self.device = device
        self.workspace_alloc_bytes = workspace_bytes
        self.stream = self.lib.lia_ctx_compute_stream(h)
        self._token_mask = None          # (tensor [rows, W], ldm in words): the table lia_ctx_set_token_mask points at
        self._logprob_sink = None        # the LogprobRequest whose tensors lia_ctx_set_logprob_sink points at
        self._penalties = None           # (counts, scratch, repetition, presence, frequency): what lia_ctx_set_penalties points at

    @property
    def workspace_bytes(self):
        """what a call on this context may use now: the allocation, or its kept part while a streamer's wire cache holds the rest
        (lia_stream_cache_configure)"""
        return self.lib.lia_ctx_workspace_bytes(self.handle) if self.handle else 0

    def close(self):
        if self.handle:
            self.lib.lia_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        N.check(self.lib.lia_ctx_synchronize(self.handle), "lia_ctx_synchronize")

    def kv_store_wait(self):
        N.check(self.lib.lia_ctx_kv_store_wait(self.handle), "lia_ctx_kv_store_wait")

    def set_host_threads(self, n):
        N.check(self.lib.lia_ctx_set_host_threads(self.handle, n))

    def set_option(self, key, value):
        """lia_ctx_set_option: a switch of THIS context (N.LIA_OPT_*); other contexts of the process are not affected"""
        N.check(self.lib.lia_ctx_set_option(self.handle, key, value), "lia_ctx_set_option")

    def fused_combines(self, kind):
        """fused split-K combines of LIA_POST_* kind (1 LayerNorm, 2 RMSNorm, 3 SiLU*up, 4 RoPE) launched through this context"""
        return self.lib.lia_ctx_get_counter(self.handle, N.LIA_CNT_FUSED_COMBINE + kind)

    def block_attention_launches(self):
        """block attention launches through this context (N.LIA_OPT_BLOCK_ATTENTION set: the verify pass of speculative decoding)"""
        return self.lib.lia_ctx_get_counter(self.handle, N.LIA_CNT_BLOCK_ATTENTION)

    def split_decode_launches(self):
        """split-key decode attention launches through this context (N.LIA_OPT_SPLIT_DECODE set, or a cache beyond the one-workgroup
        decode kernel's LDS bound)"""
        return self.lib.lia_ctx_get_counter(self.handle, N.LIA_CNT_SPLIT_DECODE)

    def chain_next_norm(self, g_ptr, b_ptr=None):
        """lia_ctx_chain_next_norm: the next layer call also computes the first norm (weights g, b) of the layer after it."""
        N.check(self.lib.lia_ctx_chain_next_norm(self.handle, ctypes.c_void_p(g_ptr), ctypes.c_void_p(b_ptr) if b_ptr else None),
                "lia_ctx_chain_next_norm")

    def prof_start(self, max_launches=16384, stride=1):
        """HIP-event brackets around every stride-th GEMM launch from here on (lia_prof_start / lia_prof_set_stride)."""
        N.check(self.lib.lia_prof_set_stride(self.handle, stride), "lia_prof_set_stride")
        N.check(self.lib.lia_prof_start(self.handle, max_launches), "lia_prof_start")

    def prof_stop(self):
        r = N.ProfResult()
        N.check(self.lib.lia_prof_stop(self.handle, ctypes.byref(r)), "lia_prof_stop")
        return {k: getattr(r, k) for k, _ in r._fields_}

    def _st(self, stream):
        return ctypes.c_void_p(self.stream if stream is None else stream)

    # ---- sub-layer ops --------------------------------------------------------------------------
    def layernorm(self, x, g, b, eps=1e-5, stream=None):
        for t in (x, g, b):
            _chk(t)
        y = torch.empty_like(x)
        H = x.shape[-1]
        rows = x.numel() // H
        N.check(self.lib.lia_layernorm(_ptr(x), H, _ptr(g), _ptr(b), _ptr(y), H, rows, H, eps, self._st(stream)), "lia_layernorm")
        return y

    def linear(self, x, w, bias=None, residual=None, relu=False, split_k=0, stream=None):
        for t in (x, w, bias, residual):
            _chk(t)
        Nn, K = w.shape
        M = x.numel() // K
        y = torch.empty(x.shape[:-1] + (Nn,), dtype=torch.bfloat16, device=x.device)
        N.check(self.lib.lia_linear(self.handle, _ptr(x), K, _ptr(w), _ptr(bias), _ptr(residual), Nn, _ptr(y), Nn, M, Nn, K,
                                    int(relu), split_k, self._st(stream)), "lia_linear")
        return y

    def qkv_project(self, x, w, bias, kcache, vcache, b0, pos0, stream=None):
        for t in (x, w, bias, kcache, vcache):
            _chk(t)
        B, T, H = x.shape
        q = torch.empty_like(x)
        N.check(self.lib.lia_qkv_project(self.handle, _ptr(x), _ptr(w), _ptr(bias), _ptr(q), _ptr(kcache), _ptr(vcache), B, T, H,
                                         kcache.shape[1], b0, pos0, self._st(stream)), "lia_qkv_project")
        return q

    def attention(self, q, kcache, vcache, S, heads, b0=0, stream=None):
        for t in (q, kcache, vcache):
            _chk(t)
        B, T, H = q.shape
        out = torch.empty_like(q)
        N.check(self.lib.lia_attention(_ptr(q), H, _ptr(kcache), _ptr(vcache), _ptr(out), H, B, T, S, heads, H // heads,
                                       kcache.shape[1], b0, self._st(stream)), "lia_attention")
        return out

    def embed(self, ids, tok, pos, past_len, stream=None):
        _chk(ids, torch.int64)
        B, T = ids.shape
        y = torch.empty((B, T, tok.shape[1]), dtype=torch.bfloat16, device=tok.device)
        self.embed_into(ids, tok, pos, y, past_len, stream=stream)
        return y

    def embed_into(self, ids, tok, pos, y, past_len, starts=None, stream=None):
        """token + position embedding of ids [B, T] (int64, device) into y [B, T, H]; starts (int32 [B], device, or None): row b's
        first real position of a left-padded batch, whose positions then count from it."""
        _chk(tok)
        _chk(pos)
        B, T = ids.shape
        args = (_ptr(ids), _ptr(tok), _ptr(pos), _ptr(y), B, T, past_len, tok.shape[1])
        if starts is None:
            N.check(self.lib.lia_embed(*args, self._st(stream)), "lia_embed")
        else:
            N.check(self.lib.lia_embed_padded(*args, _ptr(starts), self._st(stream)), "lia_embed")

    def embed_ragged_into(self, ids, tok, pos, y, lens, starts=None, stream=None):
        """lia_embed_ragged: embed_into for a block on a ragged cache -- lens (int32 [B], device): row b's cached positions, block
        token t of row b takes the learned position lens[b] + t - starts[b] + 2 (starts: int32 [B], device, or None = zeros)."""
        _chk(tok)
        _chk(pos)
        _chk(lens, torch.int32)
        _chk(starts, torch.int32)
        B, T = ids.shape
        if lens.numel() != B or (starts is not None and starts.numel() != B):
            raise ValueError(f"lens / starts must have {B} entries, one per row of ids")
        N.check(self.lib.lia_embed_ragged(_ptr(ids), _ptr(tok), _ptr(pos), _ptr(y), B, T, tok.shape[1], _ptr(lens), _ptr(starts),
                                          self._st(stream)), "lia_embed_ragged")

    def set_row_lens(self, lens):
        """lia_ctx_set_row_lens: lens (int32 numpy [rows of the cache batch], or None to clear) -- while set, every layer call is the
        ragged form (policy 3, T >= 2) on rows b0 .. b0 + B - 1 of the table"""
        if lens is None:
            N.check(self.lib.lia_ctx_set_row_lens(self.handle, None, 0), "lia_ctx_set_row_lens")
        else:
            N.check(self.lib.lia_ctx_set_row_lens(self.handle, ctypes.c_void_p(lens.ctypes.data), lens.shape[0]), "lia_ctx_set_row_lens")

    def set_token_mask(self, mask):
        """lia_ctx_set_token_mask: mask (int32 CUDA tensor [..., W], W >= ceil(vocab / 32) words per row, rows contiguous; the leading
        dimensions are flattened -- [B, W] for lm_head / sample, [B, T, W] for the verify heads; or None to clear).  Token i of row r is
        allowed iff bit i & 31 of mask[r, i >> 5] is set; a token that is not counts as -inf in every head call on this context
        until the table is cleared.  ONE row ([W] or [1, W]) serves every row of every call (ldm = 0).  The library keeps the pointer
        only: this object keeps the tensor alive, the caller leaves it unchanged until the head call has run."""
        if mask is None:
            self._token_mask = None
            N.check(self.lib.lia_ctx_set_token_mask(self.handle, None, 0, 0), "lia_ctx_set_token_mask")
            return
        if not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.dtype != torch.int32 or mask.dim() < 1 or not mask.is_contiguous():
            raise ValueError("token mask: expected a contiguous int32 CUDA tensor [..., W], got "
                             + (f"{mask.dtype} {mask.device} shape {tuple(mask.shape)}" if isinstance(mask, torch.Tensor) else type(mask).__name__))
        m = mask.reshape(-1, mask.shape[-1])
        if m.numel() == 0:
            raise ValueError(f"token mask: an empty tensor of shape {tuple(mask.shape)}")
        torch.cuda.current_stream().synchronize()              # (the library's stream reads what torch's wrote)
        rows, W = m.shape
        ldm = 0 if rows == 1 else W                            # (one row: broadcast)
        N.check(self.lib.lia_ctx_set_token_mask(self.handle, _ptr(m), ldm, rows), "lia_ctx_set_token_mask")
        self._token_mask = m

    def token_mask_fits(self, vocab):
        """the table's rows hold ceil(vocab / 32) words (the library checks the pitch of a table, not the width of a broadcast row)"""
        m = self._token_mask
        if m is not None and m.shape[1] < (vocab + 31) // 32:
            raise ValueError(f"token mask: rows of {m.shape[1]} words, a vocabulary of {vocab} tokens needs {(vocab + 31) // 32}")

    def set_logprob_sink(self, req, shape=None):
        """lia_ctx_set_logprob_sink: req (LogprobRequest; its tensors are allocated here for a head call on `shape` = [B] or [B, T]
        rows, on the device) or None to clear.  While it is set every head call on this context also writes, per row, the
        log-probability of the id it emits and the n_top alternatives.  The library keeps the pointers only: this object keeps the
        request alive; its tensors are read once the compute stream has passed the head call."""
        if req is None:
            self._logprob_sink = None
            N.check(self.lib.lia_ctx_set_logprob_sink(self.handle, 0, None, None, None, 0), "lia_ctx_set_logprob_sink")
            return
        if not isinstance(req, LogprobRequest):
            raise ValueError(f"logprobs: expected an ops.LogprobRequest, got {type(req).__name__}")
        if not 0 <= req.n_top <= LOGPROB_MAX_TOP:
            raise ValueError(f"logprobs: n_top={req.n_top} must be in [0, {LOGPROB_MAX_TOP}]")
        req.allocate(shape, f"cuda:{self.device}")
        self._logprob_sink = req
        n = req.n_top
        N.check(self.lib.lia_ctx_set_logprob_sink(self.handle, n, _ptr(req.chosen), _ptr(req.top_ids) if n else None,
                                                  _ptr(req.top_logprobs) if n else None, req.chosen.numel()), "lia_ctx_set_logprob_sink")

    def topn_logprobs(self, logits, ids, n_top, stream=None):
        """lia_topn_logprobs (the bare kernel): per row of logits [M, vocab] (bf16, rows may be strided) the log-probability of ids[r]
        (int64 [M]) and the n_top tokens of largest logit with theirs, ordered by logit descending, ties by the lower id.  Returns
        (float32 [M], int64 [M, n_top], float32 [M, n_top]) on the device."""
        M, vocab = _chk_logits(logits)
        _chk(ids, torch.int64)
        if ids.numel() != M:
            raise ValueError(f"ids has {ids.numel()} entries, logits {M} rows")
        n = int(n_top)
        out = LogprobRequest(max(n, 0)).allocate((M,), logits.device)
        N.check(self.lib.lia_topn_logprobs(self.handle, _ptr(logits), logits.stride(0), M, vocab, _ptr(ids), n, _ptr(out.chosen),
                                           _ptr(out.top_ids) if n > 0 else None, _ptr(out.top_logprobs) if n > 0 else None,
                                           self._st(stream)), "lia_topn_logprobs")
        return out.chosen, out.top_ids, out.top_logprobs

    # ---- penalties (lia_penalty.hip) -----------------------------------------------------------------
    @staticmethod
    def _chk_counts(counts):
        if not isinstance(counts, torch.Tensor) or not counts.is_cuda or counts.dtype not in (torch.int16, torch.uint16) or counts.dim() != 2 \
                or counts.stride(1) != 1:
            raise ValueError("count table: expected a 16-bit integer CUDA tensor [rows, ldc] with unit column stride, got "
                             + (f"{counts.dtype} {counts.device} shape {tuple(counts.shape)}" if isinstance(counts, torch.Tensor)
                                else type(counts).__name__))

    def set_penalties(self, counts, repetition=1.0, presence=0.0, frequency=0.0, scratch=None, synchronize=True):
        """lia_ctx_set_penalties: counts (int16 / uint16 CUDA [rows, >= vocab]: bit 15 = in the prompt, bits 0..14 = times generated;
        or None to clear) and the settings.  While set, lm_head and sample pick their ids from the logits penalised under row i of
        the table (include/lia_hip.h); the logits they return stay raw.  scratch (bf16 CUDA [rows, >= vocab], allocated here when
        None) receives the penalised rows.  The library keeps the pointers only: this object keeps the tensors alive.  synchronize=False:
        the caller knows that torch's stream wrote nothing the head will read (a table kept by the library's own stream)."""
        if counts is None:
            self._penalties = None
            N.check(self.lib.lia_ctx_set_penalties(self.handle, None, 0, 0, 1.0, 0.0, 0.0, None, 0), "lia_ctx_set_penalties")
            return
        self._chk_counts(counts)
        if scratch is None:
            scratch = torch.empty(tuple(counts.shape), dtype=torch.bfloat16, device=counts.device)
        if not scratch.is_cuda or scratch.dtype != torch.bfloat16 or scratch.dim() != 2 or scratch.stride(1) != 1 \
                or scratch.shape[0] < counts.shape[0]:
            raise ValueError(f"penalty scratch: expected a bf16 CUDA tensor [>= {counts.shape[0]} rows, >= vocab] with unit column stride, got "
                             f"{scratch.dtype} {scratch.device} shape {tuple(scratch.shape)}")
        if synchronize:
            torch.cuda.current_stream().synchronize()          # (the library's stream reads what torch's wrote)
        N.check(self.lib.lia_ctx_set_penalties(self.handle, _ptr(counts), counts.stride(0), counts.shape[0], float(repetition), float(presence),
                                               float(frequency), _ptr(scratch), scratch.stride(0)), "lia_ctx_set_penalties")
        self._penalties = (counts, scratch, float(repetition), float(presence), float(frequency))

    @contextlib.contextmanager
    def head_modifiers(self, token_mask=None, logprobs=None, shape=None, penalties=None):
        """what a scheduler puts around one head call (and the sampler behind it): the allowed-token table (set_token_mask), the
        log-probability request for a head on `shape` rows (set_logprob_sink) and the generation's penalties (penalties.Penalties:
        its queued counts run, then its table is set) -- each where given, in that order -- and, however the block ends, none of
        them on the context afterwards: no later head call sees a modifier that was meant for this one."""
        try:
            if token_mask is not None:
                self.set_token_mask(token_mask)
            if logprobs is not None:
                self.set_logprob_sink(logprobs, shape)
            if penalties is not None:
                penalties.bind(self)
            yield self
        finally:
            if token_mask is not None:
                self.set_token_mask(None)
            if logprobs is not None:
                self.set_logprob_sink(None)
            if penalties is not None:
                self.set_penalties(None)

    def token_counts_add(self, counts, ids, generated, vocab=None, first=None, active=None, stream=None):
        """lia_token_counts_add: ids (int64 CUDA [B, n], unit column stride) are added to rows 0 .. B - 1 of counts -- generated False:
        the prompt bit, True: the saturating count.  first / active (int32 CUDA [B] or None): positions t < first[b] and rows with
        active[b] == 0 are skipped; ids outside [0, vocab) are ignored (vocab: the table's width when None)."""
        self._chk_counts(counts)
        if not ids.is_cuda or ids.dtype != torch.int64 or ids.dim() != 2 or (ids.shape[1] > 1 and ids.stride(1) != 1):
            raise ValueError(f"ids: expected an int64 CUDA tensor [B, n] with unit column stride, got {ids.dtype} {ids.device} "
                             f"shape {tuple(ids.shape)} strides {ids.stride()}")
        B, n = ids.shape
        if B > counts.shape[0]:
            raise ValueError(f"ids has {B} rows, the count table {counts.shape[0]}")
        for name, t in (("first", first), ("active", active)):
            _chk(t, torch.int32)
            if t is not None and t.numel() != B:
                raise ValueError(f"{name} has {t.numel()} entries, ids {B} rows")
        ldi = ids.stride(0) if B > 1 else max(n, 1)
        N.check(self.lib.lia_token_counts_add(self.handle, _ptr(counts), counts.stride(0), B, counts.shape[1] if vocab is None else int(vocab),
                                              _ptr(ids), ldi, n, _ptr(first), _ptr(active), int(bool(generated)), self._st(stream)),
                "lia_token_counts_add")

    def apply_penalties(self, logits, counts, repetition=1.0, presence=0.0, frequency=0.0, out=None, stream=None):
        """lia_apply_penalties (the bare kernel): the rows of logits [M, vocab] (bf16, rows may be strided) rewritten under counts
        [M, >= vocab] -> out (a new [M, vocab] tensor when None; `logits` itself: in place)."""
        self._chk_counts(counts)
        M, vocab = _chk_logits(logits)
        if counts.shape[0] < M:
            raise ValueError(f"logits has {M} rows, the count table {counts.shape[0]}")
        if out is None:
            out = torch.empty((M, vocab), dtype=torch.bfloat16, device=logits.device)
        elif not out.is_cuda or out.dtype != torch.bfloat16 or tuple(out.shape) != (M, vocab) or out.stride(1) != 1:
            raise ValueError(f"out: expected a [{M}, {vocab}] bf16 CUDA tensor with unit column stride, got {out.dtype} {out.device} "
                             f"shape {tuple(out.shape)} strides {out.stride()}")
        N.check(self.lib.lia_apply_penalties(self.handle, _ptr(logits), logits.stride(0), M, vocab, _ptr(counts), counts.stride(0),
                                             float(repetition), float(presence), float(frequency), _ptr(out), out.stride(0),
                                             self._st(stream)), "lia_apply_penalties")
        return out

    def _lm_head(self, name, norm, head, hidden, eps, suppress_token, stream):
        for t in (hidden,) + norm + (head,):
            _chk(t)
        B, T, H = hidden.shape
        vocab = head.shape[0]
        self.token_mask_fits(vocab)
        logits = torch.empty((B, vocab), dtype=torch.bfloat16, device=hidden.device)
        nxt = torch.empty((B,), dtype=torch.int64, device=hidden.device)
        N.check(getattr(self.lib, name)(self.handle, _ptr(hidden), B, T, H, *[_ptr(t) for t in norm], _ptr(head), vocab, eps, suppress_token,
                                        _ptr(logits), _ptr(nxt), self._st(stream)), name)
        return logits, nxt

    def lm_head(self, hidden, lnw, lnb, emb, eps=1e-5, suppress_token=-1, stream=None):
        """lia_lm_head: final LN + tied lm_head on the LAST position of hidden [B, T, H] + argmax (models.py:424-431,
        greedy_search.py:367) -> (logits bf16 [B, vocab], ids int64 [B]).  Any B: the library walks a batch beyond 256 rows (the
        reference's --batch-size 900 ... 1580 lines, llm/scripts/cxl_offloading.sh:13-39) in chunks of 256, and row i reads row i
        of a token mask, a log-probability sink and the penalties' tables in every chunk."""
        return self._lm_head("lia_lm_head", (lnw, lnb), emb, hidden, eps, suppress_token, stream)

    def llama_lm_head(self, hidden, normw, lm, eps=1e-5, suppress_token=-1, stream=None):
        """lia_llama_lm_head: lm_head with the final RMSNorm and the untied lm_head of a Llama"""
        return self._lm_head("lia_llama_lm_head", (normw,), lm, hidden, eps, suppress_token, stream)

    def sample(self, logits, temperature, top_k, top_p, uniforms, suppress_token=-1, stats=None, stream=None):
        """lia_sample: temperature -> top-k -> top-p -> one draw per row of logits [B, vocab] (bf16, rows may be strided) with
        uniforms [B] (float32, in [0, 1)).  Returns the ids (int64 [B]); stats (float32 [B, 4], optional) receives per row t_k, the
        top-p boundary, the kept count and the kept mass.  Any B: rows are independent."""
        B, vocab = _chk_logits(logits, "B")
        _chk(uniforms, torch.float32)
        self.token_mask_fits(vocab)
        if uniforms.numel() != B:
            raise ValueError(f"uniforms has {uniforms.numel()} entries, logits {B} rows")
        if stats is not None:
            _chk(stats, torch.float32)
            if tuple(stats.shape) != (B, 4):
                raise ValueError(f"stats must be [{B}, 4], got {tuple(stats.shape)}")
        nxt = torch.empty((B,), dtype=torch.int64, device=logits.device)
        N.check(self.lib.lia_sample(self.handle, _ptr(logits), logits.stride(0), B, vocab, float(temperature), int(top_k), float(top_p),
                                    int(suppress_token), _ptr(uniforms), _ptr(nxt), _ptr(stats), self._st(stream)), "lia_sample")
        return nxt

    def token_logprobs(self, logits, targets, stream=None):
        """lia_token_logprobs: per row of logits [M, vocab] (bf16, rows may be strided) the log-probability of targets[r] (int64
        [M], -1: none -> 0.0) under the row's softmax, and the row's greedy token (first maximal index).  Returns (float32 [M],
        int64 [M]) on the device."""
        M, vocab = _chk_logits(logits)
        _chk(targets, torch.int64)
        if targets.numel() != M:
            raise ValueError(f"targets has {targets.numel()} entries, logits {M} rows")
        lp = torch.empty((M,), dtype=torch.float32, device=logits.device)
        gr = torch.empty((M,), dtype=torch.int64, device=logits.device)
        N.check(self.lib.lia_token_logprobs(self.handle, _ptr(logits), logits.stride(0), M, vocab, _ptr(targets), _ptr(lp), _ptr(gr),
                                            self._st(stream)), "lia_token_logprobs")
        return lp, gr

    def _score_args(self, hidden, targets):
        _chk(hidden)
        _chk(targets, torch.int64)
        H = hidden.shape[-1]
        M = hidden.numel() // H
        if targets.numel() != M:
            raise ValueError(f"targets has {targets.numel()} entries, hidden {M} rows")
        lp = torch.empty((M,), dtype=torch.float32, device=hidden.device)
        gr = torch.empty((M,), dtype=torch.int64, device=hidden.device)
        return M, H, lp, gr

    def lm_score(self, hidden, lnw, lnb, emb, targets, eps=1e-5, stream=None):
        """lia_lm_score: final LN + tied lm_head on EVERY row of hidden [..., H], then token_logprobs against targets (int64, one per
        row); the logits exist one workspace chunk at a time (score_chunk_rows).  Returns (float32 [M], int64 [M]) on the device."""
        for t in (lnw, lnb, emb):
            _chk(t)
        M, H, lp, gr = self._score_args(hidden, targets)
        N.check(self.lib.lia_lm_score(self.handle, _ptr(hidden), H, M, H, _ptr(lnw), _ptr(lnb), _ptr(emb), emb.shape[0], eps,
                                      _ptr(targets), _ptr(lp), _ptr(gr), self._st(stream)), "lia_lm_score")
        return lp, gr

    def llama_lm_score(self, hidden, normw, lm, targets, eps=1e-5, stream=None):
        """lia_llama_lm_score: lm_score with the final RMSNorm and the untied lm_head of a Llama"""
        for t in (normw, lm):
            _chk(t)
        M, H, lp, gr = self._score_args(hidden, targets)
        N.check(self.lib.lia_llama_lm_score(self.handle, _ptr(hidden), H, M, H, _ptr(normw), _ptr(lm), lm.shape[0], eps,
                                            _ptr(targets), _ptr(lp), _ptr(gr), self._st(stream)), "lia_llama_lm_score")
        return lp, gr

    def _verify_args(self, hidden, block_ids, active):
        _chk(hidden)
        _chk(block_ids, torch.int64)
        if block_ids.dim() != 2:
            raise ValueError(f"block_ids must be [B, T], got shape {tuple(block_ids.shape)}")
        B, T = block_ids.shape
        H = hidden.shape[-1]
        if hidden.numel() != B * T * H:
            raise ValueError(f"hidden has {hidden.numel() // H} rows, block_ids {B} x {T}")
        if active is not None:
            _chk(active, torch.int32)
            if active.numel() != B:
                raise ValueError(f"active has {active.numel()} entries, block_ids {B} rows")
        dev = hidden.device
        out = VerifyResult(torch.empty((B, T), dtype=torch.int64, device=dev), torch.empty((B,), dtype=torch.int32, device=dev),
                           torch.empty((1,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int64, device=dev))
        return B, T, H, out

    def _verify(self, name, norm, head, hidden, block_ids, eps, suppress_token, n_suppress, active, stream):
        """n_suppress: the bound of every row, or (lia_lm_verify_rows) an int32 [B] device tensor of one bound per row"""
        for t in norm + (head,):
            _chk(t)
        per_row = isinstance(n_suppress, torch.Tensor)
        if per_row:
            _chk(n_suppress, torch.int32)
        B, T, H, out = self._verify_args(hidden, block_ids, active)
        if per_row and n_suppress.numel() != B:
            raise ValueError(f"n_suppress_rows has {n_suppress.numel()} entries, block_ids {B} rows")
        vocab = head.shape[0]
        self.token_mask_fits(vocab)
        N.check(getattr(self.lib, name)(self.handle, _ptr(hidden), H, B, T, H, *[_ptr(t) for t in norm], _ptr(head), vocab, eps,
                                        int(suppress_token), _ptr(n_suppress) if per_row else int(n_suppress), _ptr(block_ids), _ptr(active),
                                        _ptr(out.greedy), _ptr(out.accepted), _ptr(out.common), _ptr(out.next), self._st(stream)), name)
        return out

    def lm_verify(self, hidden, lnw, lnb, emb, block_ids, eps=1e-5, suppress_token=-1, n_suppress=0, active=None, stream=None):
        """lia_lm_verify: final LN + tied lm_head on every row of hidden [B, T, H] (lm_score's chunks), the greedy token of every
        block position (suppress_token counts as -inf at positions < n_suppress) and what block_ids [B, T] = [pending | draft]
        (int64, device) accepts of it; active (int32 [B], device, or None): rows with 0 never limit `common`.  -> VerifyResult."""
        return self._verify("lia_lm_verify", (lnw, lnb), emb, hidden, block_ids, eps, suppress_token, int(n_suppress), active, stream)

    def lm_verify_rows(self, hidden, lnw, lnb, emb, block_ids, n_suppress_rows, eps=1e-5, suppress_token=-1, active=None, stream=None):
        """lia_lm_verify_rows: lm_verify with one bound per row -- suppress_token counts as -inf at block positions
        t < n_suppress_rows[b] (int32 [B], device, each in [0, T])."""
        return self._verify("lia_lm_verify_rows", (lnw, lnb), emb, hidden, block_ids, eps, suppress_token, n_suppress_rows, active, stream)

    def llama_lm_verify(self, hidden, normw, lm, block_ids, eps=1e-5, suppress_token=-1, n_suppress=0, active=None, stream=None):
        """lia_llama_lm_verify: lm_verify with the final RMSNorm and the untied lm_head of a Llama"""
        return self._verify("lia_llama_lm_verify", (normw,), lm, hidden, block_ids, eps, suppress_token, int(n_suppress), active, stream)

    def _verify_sample(self, name, norm, head, hidden, block_ids, block, eps, suppress_token, n_suppress, n_suppress_rows, active,
                       return_logits, return_p_draft, stream):
        for t in norm + (head,):
            _chk(t)
        B, T, H, out = self._verify_args(hidden, block_ids, active)
        dev = hidden.device
        U = block.uniforms
        _chk(U, torch.float32)
        if U.dim() != 2:
            raise ValueError(f"uniforms must be the generation's [steps, rows] table, got shape {tuple(U.shape)}")
        if n_suppress_rows is not None:
            _chk(n_suppress_rows, torch.int32)
            if n_suppress_rows.numel() != B:
                raise ValueError(f"n_suppress_rows has {n_suppress_rows.numel()} entries, block_ids {B} rows")
        step_rows = block.step_rows
        if step_rows is not None:
            step_rows = torch.as_tensor(step_rows).to(device=dev, dtype=torch.int32).contiguous()
            if step_rows.numel() != B:
                raise ValueError(f"step_rows has {step_rows.numel()} entries, block_ids {B} rows")
            if U.is_cuda:
                torch.cuda.current_stream().synchronize()      # (the library's stream reads what torch's just copied)
            self._step_rows = step_rows                        # alive until the next call: the launch below is asynchronous
        args = N.BlockSampler(float(block.temperature), int(block.top_k), float(block.top_p), U.data_ptr(), U.stride(0), U.shape[0],
                              int(block.step0), None if step_rows is None else step_rows.data_ptr())
        vocab = head.shape[0]
        self.token_mask_fits(vocab)
        logits = torch.empty((B, T, vocab), dtype=torch.bfloat16, device=dev) if return_logits else None
        p_draft = torch.empty((B, T), dtype=torch.float32, device=dev) if return_p_draft else None
        N.check(getattr(self.lib, name)(self.handle, _ptr(hidden), H, B, T, H, *[_ptr(t) for t in norm], _ptr(head), vocab, eps,
                                        int(suppress_token), int(n_suppress), _ptr(n_suppress_rows), ctypes.byref(args), _ptr(block_ids),
                                        _ptr(active), _ptr(out.greedy), _ptr(out.accepted), _ptr(out.common), _ptr(out.next),
                                        _ptr(p_draft), _ptr(logits), self._st(stream)), name)
        return out._replace(logits=logits, p_draft=p_draft)

    def lm_verify_sample(self, hidden, lnw, lnb, emb, block_ids, block, eps=1e-5, suppress_token=-1, n_suppress=0, n_suppress_rows=None,
                         active=None, return_logits=False, return_p_draft=False, stream=None):
        """lia_lm_verify_sample: lm_verify with lia_sample's draw behind every block position in place of the argmax.  block
        (sampling.Sampler.block / block_rows): the settings, the generation's U table and the step origin -- position t of row b
        draws with U[step + t, b], 0 past the table.  n_suppress_rows (int32 [B], device) replaces n_suppress where given.
        -> VerifyResult with the sampled ids as `greedy`; logits / p_draft where asked for."""
        return self._verify_sample("lia_lm_verify_sample", (lnw, lnb), emb, hidden, block_ids, block, eps, suppress_token, n_suppress,
                                   n_suppress_rows, active, return_logits, return_p_draft, stream)

    def llama_lm_verify_sample(self, hidden, normw, lm, block_ids, block, eps=1e-5, suppress_token=-1, n_suppress=0, n_suppress_rows=None,
                               active=None, return_logits=False, return_p_draft=False, stream=None):
        """lia_llama_lm_verify_sample: lm_verify_sample with the final RMSNorm and the untied lm_head of a Llama"""
        return self._verify_sample("lia_llama_lm_verify_sample", (normw,), lm, hidden, block_ids, block, eps, suppress_token, n_suppress,
                                   n_suppress_rows, active, return_logits, return_p_draft, stream)

    def _verify_reject(self, name, norm, head, hidden, block_ids, rej, eps, suppress_token, n_suppress, active, return_logits,
                       return_probs, stream):
        for t in norm + (head,):
            _chk(t)
        B, T, H, out = self._verify_args(hidden, block_ids, active)
        dev = hidden.device
        vocab = head.shape[0]
        for U, what in ((rej.u_acc, "u_acc"), (rej.u_res, "u_res")):
            _chk(U, torch.float32)
            if U.dim() != 2 or tuple(U.shape) != tuple(rej.u_acc.shape):
                raise ValueError(f"{what} must be a [steps, rows] table of u_acc's shape, got shape {tuple(U.shape)}")
        dl = rej.draft_logits
        if dl is None:
            raise ValueError("the rejector carries no draft_logits: the drafter's logits of this round's k draft steps")
        if dl.dtype != torch.bfloat16 or not dl.is_cuda or dl.dim() != 3 or dl.stride(2) != 1:
            raise ValueError(f"draft_logits must be a bf16 CUDA tensor [B, k, vocab] with unit stride along the vocabulary, got {dl.dtype} "
                             f"{dl.device} shape {tuple(dl.shape)}")
        if tuple(dl.shape) != (B, T - 1, vocab):
            raise ValueError(f"draft_logits has shape {tuple(dl.shape)}, the block needs {(B, T - 1, vocab)}")
        torch.cuda.current_stream().synchronize()              # (the library's stream reads what torch's wrote: the drafter's logits)
        args = N.BlockRejector(float(rej.temperature), int(rej.top_k), float(rej.top_p), rej.u_acc.data_ptr(), rej.u_res.data_ptr(),
                               rej.u_acc.stride(0), rej.u_acc.shape[0], int(rej.step0), dl.data_ptr(), dl.stride(0), dl.stride(1))
        ok = torch.empty((B, T), dtype=torch.int32, device=dev)
        logits = torch.empty((B, T, vocab), dtype=torch.bfloat16, device=dev) if return_logits else None
        probs = [torch.empty((B, T), dtype=torch.float32, device=dev) if return_probs else None for _ in range(3)]
        N.check(getattr(self.lib, name)(self.handle, _ptr(hidden), H, B, T, H, *[_ptr(t) for t in norm], _ptr(head), vocab, eps,
                                        int(suppress_token), int(n_suppress), None, ctypes.byref(args), _ptr(block_ids), _ptr(active),
                                        _ptr(out.greedy), _ptr(ok), _ptr(out.accepted), _ptr(out.common), _ptr(out.next), _ptr(probs[0]),
                                        _ptr(probs[1]), _ptr(probs[2]), _ptr(logits), self._st(stream)), name)
        return out._replace(logits=logits, ok=ok, p_tok=probs[0], q_tok=probs[1], resid_mass=probs[2])

    def lm_verify_reject(self, hidden, lnw, lnb, emb, block_ids, rejector, eps=1e-5, suppress_token=-1, n_suppress=0, active=None,
                         return_logits=False, return_probs=False, stream=None):
        """lia_lm_verify_reject: the verify head for a stochastic drafter (accept x ~ Q with min(1, P(x) / Q(x)), else a draw of the
        residual).  rejector (sampling.RejectorBlock): the settings, the U_acc / U_res tables, the step origin and the drafter's
        logits [B, T - 1, vocab] behind block_ids[:, 1:].  -> VerifyResult with `token` as `greedy`, ok, and p_tok / q_tok /
        resid_mass / logits where asked for.  Common mode only."""
        return self._verify_reject("lia_lm_verify_reject", (lnw, lnb), emb, hidden, block_ids, rejector, eps, suppress_token, n_suppress,
                                   active, return_logits, return_probs, stream)

    def llama_lm_verify_reject(self, hidden, normw, lm, block_ids, rejector, eps=1e-5, suppress_token=-1, n_suppress=0, active=None,
                               return_logits=False, return_probs=False, stream=None):
        """lia_llama_lm_verify_reject: lm_verify_reject with the final RMSNorm and the untied lm_head of a Llama"""
        return self._verify_reject("lia_llama_lm_verify_reject", (normw,), lm, hidden, block_ids, rejector, eps, suppress_token, n_suppress,
                                   active, return_logits, return_probs, stream)

    def score_chunk_rows(self, M, H, vocab):
        """rows per chunk lm_score would use for M rows in this context's workspace (0: not even min(M, 256) rows fit)"""
        return self.lib.lia_lm_score_chunk_rows(self.workspace_bytes, M, H, vocab)

    # ---- the operator boundary ------------------------------------------------------------------
    def layer_forward(self, desc, policy, weight_ptrs, x, y, kv, B, T, pos0, b0=0, stream=None):
        """weight_ptrs: (c_void_p * 16) of device pointers; kv: _native.KV.  x, y: [B,T,H] device."""
        N.check(self.lib.lia_layer_forward(self.handle, ctypes.byref(desc), policy, ctypes.byref(weight_ptrs), _ptr(x), _ptr(y),
                                           ctypes.byref(kv), B, T, pos0, b0, self._st(stream)), "lia_layer_forward")


    def layer_forward_last(self, desc, policy, weight_ptrs, x, y_last, kv, B, T, pos0, b0=0, stream=None):
        """lia_layer_forward_last: the last layer of a prefill -- K/V of every position, the rest on the last position only;
        y_last: [B,1,H] device."""
        N.check(self.lib.lia_layer_forward_last(self.handle, ctypes.byref(desc), policy, ctypes.byref(weight_ptrs), _ptr(x), _ptr(y_last),
                                                ctypes.byref(kv), B, T, pos0, b0, self._st(stream)), "lia_layer_forward_last")


def block_attention_takes(heads, kv_heads, head_dim, T, S):
    """lia_attn_block_takes: whether the block attention launches (the ragged one included) take T queries per row whose last one
    sees S keys -- the launches' own rule, asked of the library"""
    return bool(N.lib().lia_attn_block_takes(int(heads), int(kv_heads), int(head_dim), int(T), int(S)))


def split_chunk(head_dim):
    """lia_attn_split_chunk: keys per chunk of the split-key decode attention (0: a head_dim it does not serve)"""
    return N.lib().lia_attn_split_chunk(int(head_dim))


def split_scratch_bytes(B, S, heads, kv_heads, head_dim):
    """lia_attn_split_scratch_bytes: the scratch of one split-key decode attention over B rows of S keys (0: a shape it refuses)"""
    return N.lib().lia_attn_split_scratch_bytes(int(B), int(S), int(heads), int(kv_heads), int(head_dim))


DECODE_LDS_BYTES = 160 * 1024       # what the one-workgroup decode kernel may use (lia_attention.hip, launch_decode)


def split_decode_forced(head_dim, heads, kv_heads, S):
    """whether a decode-shaped attention over S keys is beyond the one-workgroup kernel -- its launcher's own bound,
    (G Spad + 4 G d + 8 G) 4 bytes of LDS -- so that a layer call takes the split-key route whatever the option says"""
    G = heads // kv_heads
    return (G * ((S + 3) & ~3) + 4 * G * head_dim + 8 * G) * 4 > DECODE_LDS_BYTES


# Shape classes where tools/attn_split_bench measured the split-key route's median below the one-workgroup launch's by more than the
# run-to-run spread of the two legs (results/attn_split_bench.txt): (head_dim, heads / kv_heads, the most workgroups B * kv_heads of
# the one-workgroup launch, the fewest keys S).  A class nobody measured keeps the one-workgroup launch.
# Measured (MI355X, medians of 30 interleaved launches, split p90 below one-workgroup p10 in every listed class):
#   d 128, G 1 (OPT-30B heads), 56 workgroups, S 2047: 27.6 us against 35.2 (S 1024: 20.2 against 20.6, inside the spread -> not listed;
#     224 workgroups: the one-workgroup launch wins at every S)
#   d 128, G 4 (Llama-3-8B heads), 8 / 32 workgroups from S 1030 (25.4 / 26.0 us against 36.6 / 36.8), 128 workgroups from S 4096
#     (83.4 against 113.2; S 1030: 36.8 against 38.3, a 4 % margin -> not listed)
#   d 64 / 32, G 4, 8 / 32 workgroups from S 4096 (30.8 / 37.4 us against 103.0 / 103.4; 29.0 / 32.2 against 56.3 / 60.1)
SPLIT_DECODE_PAYS = (
    (128, 1, 56, 2047),
    (128, 4, 32, 1030),
    (128, 4, 128, 4096),
    (64, 4, 32, 4096),
    (32, 4, 32, 4096),
)
SPLIT_DECODE_MAX_WORKGROUPS = 255   # a launch of B * kv_heads >= 256 workgroups fills the chip by itself: never by the table


def split_decode_pays(head_dim, heads, kv_heads, B, S):
    """the "measured" rule of a scheduler's split_decode: the table above"""
    if kv_heads <= 0 or heads % kv_heads or B * kv_heads > SPLIT_DECODE_MAX_WORKGROUPS or S <= split_chunk(head_dim):
        return False
    G = heads // kv_heads
    return any(d == head_dim and g == G and B * kv_heads <= wgs and S >= s_min for d, g, wgs, s_min in SPLIT_DECODE_PAYS)


def split_decode_mode(value, what="split_decode"):
    """a scheduler's split_decode from an argument, $LIA_SPLIT_DECODE or --split-decode: True / False / "measured"; anything else is
    refused by name"""
    if value is None:
        return "measured"
    if isinstance(value, bool):
        return value
    modes = {"1": True, "on": True, "true": True, "0": False, "off": False, "false": False, "measured": "measured"}
    key = str(value).strip().lower()
    if key not in modes:
        raise ValueError(f"{what}={value!r}: one of 0 / off, 1 / on, measured")
    return modes[key]


def split_decode_for(mode, head_dim, heads, kv_heads, B, S):
    """(LIA_OPT_SPLIT_DECODE of one decode step, whether the step takes the split-key route and so needs its scratch): mode True =
    every step over more keys than one chunk, False = only beyond the one-workgroup kernel, "measured" = split_decode_pays"""
    if split_decode_forced(head_dim, heads, kv_heads, S):
        return 0, True
    on = split_decode_pays(head_dim, heads, kv_heads, B, S) if mode == "measured" else bool(mode) and S > split_chunk(head_dim)
    return int(on), bool(on)


def make_desc(hidden, heads, ffn, eps=1e-5):
    return N.LayerDesc(hidden, heads, ffn, eps)


def pack_offsets(desc):
    offs = (ctypes.c_size_t * 16)()
    total = ctypes.c_size_t()
    N.check(N.lib().lia_layer_pack_offsets(ctypes.byref(desc), ctypes.byref(offs), ctypes.byref(total)), "lia_layer_pack_offsets")
    return list(offs), total.value


def workspace_bytes(desc, max_rows):
    return N.lib().lia_layer_workspace_bytes(ctypes.byref(desc), max_rows)


def weight_ptr_array(base_ptr, offsets):
    """the device (or host) pointers of one layer's tensors: 16 for an OPT layer, 9 for a Llama layer"""
    return (ctypes.c_void_p * len(offsets))(*[base_ptr + o for o in offsets])
