"""Constrained decoding for generate(): restricting which tokens a row may emit ("Constrained decoding").

HF's spellings -- prefix_allowed_tokens_fn, suppress_tokens, begin_suppress_tokens, bad_words_ids (single-token entries) -- and a
grammar engine's packed bitmask (allowed_mask_fn) all become ONE thing on the device: a row of W = ceil(vocab / 32) int32 words per
batch row, token i allowed iff bit i & 31 of word i >> 5 is set (little endian, xgrammar's layout).  The head kernels count a token
whose bit is clear as -inf, exactly as they count suppress_token (lia_ctx_set_token_mask, include/lia_hip.h); the logits
return_logits=True hands back stay the raw ones.

The id lists are packed here, on the host, with numpy: a few hundred KB per step beside a decode step of hundreds of milliseconds.
Static lists are packed and uploaded once and served as one broadcast row; a callable is evaluated every step from the ids the
generation loop already holds.  A finished row (EOS bookkeeping) gets an all-ones row and its callable is not called.
"""
import numpy as np
import torch

DEVICE = "cuda"          # where the mask rows are uploaded (the head kernels read them there)

REFUSALS = {
    "both": "prefix_allowed_tokens_fn together with allowed_mask_fn is not supported: pass one callable (AND the two sets in it)",
    "bad_words": "bad_words_ids entries must be single-token lists: a multi-token bad word depends on the tokens before it, which "
                 "this build does not track",
    "row": "acceptance='row' together with a token constraint is not supported: the masks of a verify block are built for one "
           "step origin per batch",
    "rejection": "verify_rule='rejection' together with a token constraint is not supported: the drafter's distribution would have "
                 "to be masked the same way",
    "dp": "prefix_allowed_tokens_fn / allowed_mask_fn together with a data-parallel group is not supported: the callable would see "
          "one rank's rows under local row numbers (suppress_tokens, begin_suppress_tokens and bad_words_ids work: every rank "
          "packs the same row)",
    "cpu_layers": "prefix_allowed_tokens_fn / allowed_mask_fn together with cpu_layers=-1 (the online cooperative split) is not "
                  "supported: the controller times decode steps, a callable's host time would count as the step's",
}


def mask_words(vocab):
    """W: int32 words per mask row"""
    return (int(vocab) + 31) // 32


def _id_array(ids, vocab, what):
    """ids as a 1-D int64 array, every one inside [0, vocab) (ValueError names the first that is not)"""
    if isinstance(ids, torch.Tensor):
        ids = ids.detach().cpu().numpy()
    try:
        a = np.asarray(list(ids) if not isinstance(ids, np.ndarray) else ids)
    except TypeError:
        raise ValueError(f"{what} must be an iterable of token ids, got {type(ids).__name__}") from None
    if a.size == 0:
        return np.zeros(0, np.int64)
    if a.ndim != 1 or a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{what} must be a flat list of integer token ids, got an array of {a.dtype} with shape {a.shape}")
    a = a.astype(np.int64)
    bad = (a < 0) | (a >= vocab)
    if bad.any():
        raise ValueError(f"{what}: token id {int(a[bad][0])} is outside the vocabulary [0, {vocab})")
    return a


def pack_ids(ids, vocab):
    """the mask row (int32 [W]) that allows exactly `ids`: bit i & 31 of word i >> 5 per id i"""
    a = _id_array(ids, vocab, "token ids")
    words = np.zeros(mask_words(vocab), np.uint32)
    np.bitwise_or.at(words, a >> 5, np.uint32(1) << (a & 31).astype(np.uint32))
    return words.view(np.int32)


def full_row(vocab):
    """every token allowed, the bits at and beyond vocab clear"""
    W = mask_words(vocab)
    words = np.full(W, 0xFFFFFFFF, np.uint32)
    if vocab & 31:
        words[-1] = (np.uint32(1) << np.uint32(vocab & 31)) - np.uint32(1)
    return words.view(np.int32)


def _clear(row, ids):
    out = row.view(np.uint32).copy()
    np.bitwise_and.at(out, ids >> 5, ~(np.uint32(1) << (ids & 31).astype(np.uint32)))
    return out.view(np.int32)


class Constraint:
    """The token constraint of one generate() call.  The loops ask it for the mask of every forward:
        step_mask(step, ids, unfinished, suppress)               -> device int32 [1, W] (static lists: one broadcast row) or [B, W]
        block_mask(step0, ids, draft, unfinished, suppress, n)   -> device int32 [1, W] or [B, k + 1, W] of a verify pass: position t's
                                                                    row is built from ids + draft[:, :t] (the pending token is in ids)
    ids: int64 [B, n] on the CPU, the rows as HF would pass them (the prompt as given, pads included, plus what was generated; the
    whole conversation under past=); unfinished: [B], 0 / False = finished.  suppress: the token min_new_tokens suppresses at this
    step (or -1) -- only to refuse a row it would leave without any token.
    A row that allows no token is refused by name (row and step).  For a CUDA mask of allowed_mask_fn that check costs one device
    reduction and a synchronisation per step."""

    def __init__(self, vocab, prefix_allowed_tokens_fn=None, allowed_mask_fn=None, suppress_tokens=None, begin_suppress_tokens=None,
                 bad_words_ids=None):
        self.vocab, self.W = int(vocab), mask_words(vocab)
        if prefix_allowed_tokens_fn is not None and allowed_mask_fn is not None:
            raise ValueError(REFUSALS["both"])
        for name, fn in (("prefix_allowed_tokens_fn", prefix_allowed_tokens_fn), ("allowed_mask_fn", allowed_mask_fn)):
            if fn is not None and not callable(fn):
                raise ValueError(f"{name} must be callable, got {type(fn).__name__}")
        self.prefix_fn, self.mask_fn = prefix_allowed_tokens_fn, allowed_mask_fn
        sup = _id_array(suppress_tokens, vocab, "suppress_tokens") if suppress_tokens is not None else np.zeros(0, np.int64)
        beg = _id_array(begin_suppress_tokens, vocab, "begin_suppress_tokens") if begin_suppress_tokens is not None else np.zeros(0, np.int64)
        bad = []
        for w in (bad_words_ids if bad_words_ids is not None else ()):
            w = _id_array(w, vocab, "bad_words_ids")
            if w.size != 1:
                raise ValueError(REFUSALS["bad_words"] + f"; got an entry of {w.size} tokens")
            bad.append(int(w[0]))
        self.valid = full_row(vocab)
        self.static = _clear(self.valid, np.concatenate([sup, np.asarray(bad, np.int64)]))
        self.begin = _clear(self.static, beg)
        self.has_begin = beg.size > 0
        self._dev = {}                                  # uploaded rows: "static" / "begin" / "valid" -> device [1, W]
        self._checked = set()                           # (begin, suppress) pairs of the static rows already found non-empty
        self._check(self.static[None], 0, -1)

    @property
    def has_callable(self):
        return self.prefix_fn is not None or self.mask_fn is not None

    def check_context(self, sched, lia, draft=None, acceptance="common", verify_rule="draw"):
        """the refusals that depend on the rest of the call, by name (ValueError), before any forward"""
        if acceptance == "row":
            raise ValueError(REFUSALS["row"])
        if verify_rule == "rejection":
            raise ValueError(REFUSALS["rejection"])
        if self.has_callable:
            if getattr(sched, "dp", None) is not None:
                raise ValueError(REFUSALS["dp"])
            if lia.get("cpu_layers", 0) < 0:
                raise ValueError(REFUSALS["cpu_layers"])

    # -- host rows ---------------------------------------------------------------------------------
    def _check(self, rows, step, suppress, rows_of=None):
        """ValueError naming the first row of `rows` (int32 [n, W]) that allows no token, or only `suppress`"""
        live = rows.view(np.uint32) & self.valid.view(np.uint32)
        some = live.any(axis=1)
        if suppress is not None and 0 <= suppress < self.vocab:
            live = live.copy()
            live[:, suppress >> 5] &= ~(np.uint32(1) << np.uint32(suppress & 31))
        left = live.any(axis=1)
        self._refuse(some, left, step, suppress, rows_of)

    def _refuse(self, some, left, step, suppress, rows_of=None):
        if left.all():
            return
        i = int(np.flatnonzero(~left)[0])
        who = "every row (the static lists)" if rows_of is None else f"row {int(rows_of[i])}"
        if some[i]:
            raise ValueError(f"token constraint: {who} allows only the EOS token {suppress} at step {step}, which min_new_tokens suppresses there")
        raise ValueError(f"token constraint: {who} allows no token at step {step}")

    def _upload(self, key):
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(getattr(self, key)[None].copy()).to(DEVICE)
        return self._dev[key]

    def _rows(self, step, ids, unfinished, suppress):
        """the [B, W] rows of one step: a numpy array, a CUDA tensor (allowed_mask_fn returned one), or None (static lists only)"""
        base_key = "begin" if (step == 0 and self.has_begin) else "static"
        base = getattr(self, base_key)
        if not self.has_callable:
            if (base_key, suppress) not in self._checked:
                self._check(base[None], step, suppress)
                self._checked.add((base_key, suppress))
            return None
        B = int(ids.shape[0])
        unf = np.ones(B, bool) if unfinished is None else np.asarray(unfinished).astype(bool)
        live = np.flatnonzero(unf)
        if self.prefix_fn is not None:
            rows = np.tile(self.valid, (B, 1))
            for b in live:
                allowed = _id_array(self.prefix_fn(int(b), ids[b]), self.vocab, f"prefix_allowed_tokens_fn(row {int(b)}, step {step})")
                rows[b] = pack_ids(allowed, self.vocab) & base
            self._check(rows[live], step, suppress, rows_of=live)
            return rows
        m = self.mask_fn(ids)
        if not isinstance(m, torch.Tensor):
            m = torch.as_tensor(np.asarray(m))
        if m.dtype != torch.int32 or tuple(m.shape) != (B, self.W):
            raise ValueError(f"allowed_mask_fn must return an int32 tensor of shape [B, ceil(vocab / 32)] = {(B, self.W)}, got "
                             f"{m.dtype} {tuple(m.shape)} at step {step}")
        if not m.is_cuda:
            rows = m.numpy() & base
            rows[~unf] = self.valid
            self._check(rows[live], step, suppress, rows_of=live)
            return rows
        m = m & self._upload(base_key)
        if not unf.all():
            m[torch.from_numpy(~unf).to(m.device)] = self._upload("valid")[0]
        chk = m & self._upload("valid")
        some = (chk != 0).any(dim=1)
        if suppress is not None and 0 <= suppress < self.vocab:
            bit = int(np.array([1 << (suppress & 31)], np.uint32).view(np.int32)[0])      # (bit 31 is the int32 sign)
            chk = chk.clone()
            chk[:, suppress >> 5] &= ~bit
        left = (chk != 0).any(dim=1)
        both = torch.stack([some, left]).cpu().numpy()                    # (the one synchronisation of the step)
        self._refuse(both[0][live], both[1][live], step, suppress, rows_of=live)
        return m

    # -- what the loops call -----------------------------------------------------------------------
    def step_mask(self, step, ids, unfinished=None, suppress=-1):
        rows = self._rows(step, ids, unfinished, suppress)
        if rows is None:
            return self._upload("begin" if (step == 0 and self.has_begin) else "static")
        if isinstance(rows, np.ndarray):
            return torch.from_numpy(np.ascontiguousarray(rows)).to(DEVICE)
        return rows.contiguous()

    def block_mask(self, step0, ids, draft, unfinished=None, suppress=-1, n_suppress=0):
        """the masks of a verify pass over [pending | draft]: position t is generated step step0 + t behind ids + draft[:, :t], and
        `suppress` counts there iff t < n_suppress.  The drafter knows nothing of the constraint, so draft[:, t] may be a token
        position t's row forbids: the verify pass cannot accept it, no position behind it can be kept, and ids + draft[:, :t + 1] is
        a prefix the plain constrained run never reaches -- a trie or grammar callable answers it with an empty set or raises.  From
        there on the row is treated like a finished one: all-ones rows, no call, no empty-row refusal."""
        k = int(draft.shape[1])
        B = int(ids.shape[0])
        live = np.ones(B, bool) if unfinished is None else np.asarray(unfinished).astype(bool).copy()
        rows_b = np.arange(B)
        per = []
        for t in range(k + 1):
            row_ids = ids if t == 0 else torch.cat([ids, draft[:, :t]], dim=1)
            sup_t = suppress if t < n_suppress else -1
            rows = self._rows(step0 + t, row_ids, live, sup_t)
            per.append(rows)
            if rows is not None and t < k and live.any():
                tok = draft[:, t].numpy().astype(np.int64)
                inside = (tok >= 0) & (tok < self.vocab)
                word = np.where(inside, tok >> 5, 0)
                if isinstance(rows, np.ndarray):
                    words = rows.view(np.uint32)[rows_b, word]
                else:
                    words = rows[torch.from_numpy(rows_b).to(rows.device), torch.from_numpy(word).to(rows.device)].cpu().numpy().view(np.uint32)
                ok = inside & (((words >> (tok & 31).astype(np.uint32)) & 1) == 1)
                if sup_t is not None and sup_t >= 0:
                    ok &= tok != sup_t
                live &= ok
        if per[0] is None:                 # (a verify pass never holds generated step 0: the first forward is an ordinary one)
            return self._upload("static")
        if isinstance(per[0], np.ndarray):
            return torch.from_numpy(np.ascontiguousarray(np.stack(per, axis=1))).to(DEVICE)
        return torch.stack(per, dim=1).contiguous()
