"""generate(..., logprobs=N): the log-probability of every emitted token and its N most likely alternatives.

The distribution is the MODEL'S OWN -- the fp32 log-softmax of the raw bf16 logits a head has in hand; no temperature, top-k / top-p,
suppressed EOS or constraint is applied, so a token the processors forbid can appear among the alternatives and the emitted token's
own log-probability is reported whether or not it is one of them.  The head kernels write the values (lia_ctx_set_logprob_sink,
include/lia_hip.h) for the id they emit; this module holds the request's checks, the one host copy per step and the bookkeeping of
the loops in generation.py / speculative.py.
"""
import torch

from .ops import LOGPROB_MAX_TOP, LogprobRequest

REFUSALS = {
    "bool": "logprobs=True is not supported: name the number of alternatives, an int in [0, 32] (0: the emitted tokens' own "
            "log-probabilities only)",
    "int": f"logprobs must be None (off) or an int in [0, {LOGPROB_MAX_TOP}]",
    "vocab": "logprobs: more alternatives than the vocabulary has tokens",
    "row": "logprobs together with acceptance='row' is not supported yet: the rows keep different block positions per round",
    "rejection": "logprobs together with verify_rule='rejection' is not supported: an accepted draft token is the drafter's draw, not "
                 "the verify head's own output, and the rejection head writes no log-probabilities",
    "dp": "logprobs together with a data-parallel group is not supported yet: the ranks' rows are not gathered",
}


def check_request(logprobs, vocab, sched=None, draft=None, acceptance="common", verify_rule="draw"):
    """every refusal of generate(logprobs=), by name (ValueError), before any forward; -> N (int) or None (off)"""
    if logprobs is None:
        return None
    if isinstance(logprobs, bool):
        raise ValueError(REFUSALS["bool"] + f", got {logprobs!r}")
    if not isinstance(logprobs, int) or not 0 <= logprobs <= LOGPROB_MAX_TOP:
        raise ValueError(REFUSALS["int"] + f", got {logprobs!r}")
    if logprobs > vocab:
        raise ValueError(REFUSALS["vocab"] + f": logprobs={logprobs}, vocab={vocab}")
    if acceptance == "row":
        raise ValueError(REFUSALS["row"])
    if verify_rule == "rejection":
        raise ValueError(REFUSALS["rejection"])
    if getattr(sched, "dp", None) is not None:
        raise ValueError(REFUSALS["dp"])
    return logprobs


class TokenLogprobs:
    """token_logprobs float32 [B, n_new]: log p of the token at out[b, T + s]; top_ids int64 [B, n_new, N] / top_logprobs float32
    [B, n_new, N]: the N most likely tokens of that step by logit descending (ties by the lower id) and their log-probabilities.
    CPU tensors.  A step of a row that had already finished (the pad fill) holds 0.0 / -1 / -inf."""

    def __init__(self, token_logprobs, top_ids, top_logprobs):
        self.token_logprobs, self.top_ids, self.top_logprobs = token_logprobs, top_ids, top_logprobs

    def sequence_logprob(self):
        """float32 [B]: the sum over the generated tokens of every row"""
        return self.token_logprobs.sum(dim=1)


def fetch(ids_dev, req):
    """ONE device-to-host copy of a head's ids (int64 [...]) and the request's three tensors behind them -> (ids, chosen, top_ids,
    top_logprobs) on the CPU.  The four are packed as int32 words on the device, so that the step pays the one synchronising copy it
    paid for the ids alone."""
    n = req.n_top
    rows = ids_dev.numel()
    shape = tuple(ids_dev.shape)
    parts = [ids_dev.reshape(rows, 1).view(torch.int32), req.chosen.reshape(rows, 1).view(torch.int32)]
    if n:
        parts += [req.top_ids.reshape(rows, n).view(torch.int32), req.top_logprobs.reshape(rows, n).view(torch.int32)]
    host = torch.cat(parts, dim=1).cpu()
    ids = host[:, 0:2].contiguous().view(torch.int64).reshape(shape)
    chosen = host[:, 2:3].contiguous().view(torch.float32).reshape(shape)
    if n:
        top_ids = host[:, 3:3 + 2 * n].contiguous().view(torch.int64).reshape(shape + (n,))
        top_lp = host[:, 3 + 2 * n:].contiguous().view(torch.float32).reshape(shape + (n,))
    else:
        top_ids = torch.empty(shape + (0,), dtype=torch.int64)
        top_lp = torch.empty(shape + (0,), dtype=torch.float32)
    return ids, chosen, top_ids, top_lp


class Recorder:
    """the per-step bookkeeping of one generation: B rows, at most max_new_tokens steps, N alternatives"""

    def __init__(self, B, max_new_tokens, n_top):
        self.n_top = n_top
        self.lp = torch.zeros((B, max_new_tokens), dtype=torch.float32)
        self.ids = torch.full((B, max_new_tokens, n_top), -1, dtype=torch.int64)
        self.top = torch.full((B, max_new_tokens, n_top), float("-inf"), dtype=torch.float32)

    def request(self):
        return LogprobRequest(self.n_top)

    def record(self, step, unfinished, chosen, top_ids, top_lp):
        """step `step` of every row: the head's values where the row was still unfinished BEFORE the step (unfinished: int64 [B] of
        0 / 1, or None = every row), the fills where its token is the pad fill"""
        if unfinished is None:
            live = torch.ones(chosen.shape[0], dtype=torch.bool)
        else:
            live = unfinished.bool()
        self.lp[live, step] = chosen[live]
        self.ids[live, step] = top_ids[live]
        self.top[live, step] = top_lp[live]

    def result(self, n_steps):
        return TokenLogprobs(self.lp[:, :n_steps].clone(), self.ids[:, :n_steps].clone(), self.top[:, :n_steps].clone())
