"""generate(..., repetition_penalty=, presence_penalty=, frequency_penalty=): the penalties that depend on a row's own token history
(DESIGN.md 3.8c).

Per row the device holds a COUNT ROW of one uint16 word per token -- bit 15: the token occurs in the prompt, bits 0..14: how often it
was generated in this call (saturating at 32767).  With theta = repetition_penalty, alpha_p = presence_penalty and alpha_f =
frequency_penalty the heads pick their ids from

    x = fp32(l);  if word != 0: x = x * theta if x < 0 else x / theta;  x = x - alpha_f * n;  x = x - (alpha_p if n > 0 else 0);  bf16(x)

(HF's RepetitionPenaltyLogitsProcessor over prompt and generated tokens, OpenAI's / vLLM's two over the generated ones) -- in the
greedy argmax and in the sampler, in front of suppress_token, the token mask, the temperature and the filters.  The kernels are
lia_penalty.hip's; this module holds the settings' checks, the table and the bookkeeping of generation.py's loop.  Padded positions
of a left-padded prompt are not counted (HF penalises the pad token there).
"""
import math

import torch

DEVICE = "cuda"          # where the count table lives (the head kernels read it there)

NAMES = ("repetition_penalty", "presence_penalty", "frequency_penalty")
NEUTRAL = {"repetition_penalty": 1.0, "presence_penalty": 0.0, "frequency_penalty": 0.0}

REFUSALS = {
    "draft": "together with draft= is not supported yet: every block position of a verify pass would need its own counts",
    "dp": "together with a data-parallel group is not supported yet: the ranks' count tables are not kept in step",
}


def check_value(name, v):
    """the setting as a float, NEUTRAL[name] for None; ValueError names a bad one"""
    if v is None:
        return NEUTRAL[name]
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        raise ValueError(f"{name} must be a finite number, got {v!r}")
    if name == "repetition_penalty" and v <= 0:
        raise ValueError(f"repetition_penalty must be a finite number > 0 (1.0: off), got {v!r}")
    return float(v)


class Penalties:
    """the penalty settings of one generate() call and, between begin() and the end of the call, its count table"""

    def __init__(self, vocab, repetition_penalty=None, presence_penalty=None, frequency_penalty=None):
        self.vocab = None if vocab is None else int(vocab)       # (None: a model without one -- only check_context serves it)
        self.asked = dict(zip(NAMES, (repetition_penalty, presence_penalty, frequency_penalty)))
        self.repetition, self.presence, self.frequency = (check_value(k, v) for k, v in self.asked.items())
        self.counts = self.scratch = None
        self._pending = []
        self._torch_wrote = False       # torch's stream holds work the library's stream must see: the next bind() synchronises once

    @property
    def neutral(self):
        """nothing to apply: the call is the one without the keywords"""
        return (self.repetition, self.presence, self.frequency) == (1.0, 0.0, 0.0)

    def _first_set(self):
        for k in NAMES:
            if self.asked[k] is not None and float(self.asked[k]) != NEUTRAL[k]:
                return f"{k}={self.asked[k]!r}"

    def check_context(self, sched, draft=None):
        """the refusals that depend on the rest of the call, by name (ValueError), before any forward.  (The head of every route of
        this build runs on the GPU -- decoding policy 1 and cpu_layers move layers to the host cores, never the head -- so no
        route is refused for a host-side head.)"""
        if self.neutral:
            return
        if not getattr(sched, "supports_penalties", False):
            raise ValueError(f"{self._first_set()} is not supported: {type(sched).__name__} has no penalty route (a scheduler declares "
                             "supports_penalties and takes forward(penalties=))")
        if draft is not None:
            raise ValueError(f"{self._first_set()} {REFUSALS['draft']}")
        if getattr(sched, "dp", None) is not None:
            raise ValueError(f"{self._first_set()} {REFUSALS['dp']}")

    # -- the table -------------------------------------------------------------------------------------
    def begin(self, ids, starts=None):
        """ids int64 [B, T] (CPU): the prompt -- under past= the whole conversation so far; starts (int32 [B] or None): row b's first
        real position of a left-padded batch.  Allocates the zeroed table [B, ldc] and the scratch, and queues the prompt's count;
        the queue runs on the library's compute stream when the next head call binds the table."""
        ids = torch.as_tensor(ids, dtype=torch.int64)
        B = ids.shape[0]
        ldc = (self.vocab + 7) // 8 * 8           # rows 16-byte aligned: the penalty kernel's wide path
        self.counts = torch.zeros((B, ldc), dtype=torch.int16, device=DEVICE)
        self.scratch = torch.empty((B, ldc), dtype=torch.bfloat16, device=DEVICE)
        first = None if starts is None else torch.as_tensor(starts).to(device=DEVICE, dtype=torch.int32).contiguous()
        self._pending = [(ids.to(DEVICE).contiguous(), False, first, None)]
        self._torch_wrote = True        # (the zeroed table, the uploaded prompt)

    def advance(self, cur, unfinished=None):
        """cur (int64 [B] or [B, 1], on the device where the head left it): the token every row just emitted counts as generated;
        unfinished (int64 / int32 [B] of 0 / 1, or None = every row): a row that had finished before the step is skipped"""
        active = None if unfinished is None else torch.as_tensor(unfinished).to(device=DEVICE, dtype=torch.int32).contiguous()
        self._torch_wrote |= active is not None or not cur.is_cuda      # (an upload; the head's own ids were written by the library's stream)
        self._pending.append((cur.to(DEVICE).reshape(-1, 1), True, None, active))

    def bind(self, ctx):
        """in front of a head call on ctx: the queued counts, then the table on the context (ops.Context.set_penalties)"""
        if self.counts is None:
            raise ValueError("penalties: bind() before begin()")
        if self._torch_wrote and self.counts.is_cuda:
            torch.cuda.current_stream().synchronize()          # (the library's stream reads what torch's wrote: once, not per step)
        self._torch_wrote = False
        for ids, generated, first, active in self._pending:
            ctx.token_counts_add(self.counts, ids, generated, vocab=self.vocab, first=first, active=active)
        self._pending = []
        ctx.set_penalties(self.counts, self.repetition, self.presence, self.frequency, self.scratch, synchronize=False)
