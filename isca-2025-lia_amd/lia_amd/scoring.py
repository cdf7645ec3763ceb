"""Scoring: per-token log-likelihoods of whole sequences -- what the reference's accuracy harness computes with
F.log_softmax over the logits of every position (llm/single_instance/run_accuracy.py:412-495), here from one prefill-shaped pass
of the offload scheduler (OffloadScheduler.score / LlamaScheduler.score) under generate()'s LIA flags.

    logprobs, greedy, valid = score(model, input_ids, attention_mask=None, prefill_policy=0, gpu_percentage=10, ...)
    [(ll, is_greedy)] = loglikelihood(model, [(context_ids, continuation_ids), ...], batch_size=8, **lia_kwargs)
    ll = loglikelihood_rolling(model, token_ids, prefix_token, max_len=None, **lia_kwargs)

    logprobs, greedy = continuation_logprobs(model, state, cont_ids, append_policy=None)   # against a cached conversation

lm_eval itself is not a dependency; the two request kinds restate its meaning.
"""
import numpy as np
import torch

from .generation import LIA_KWARGS, LLAMA_PADDING_REFUSAL, _scheduler_of, left_padding_starts

PAD_TOKEN_ID = 1      # fills the left padding of an OPT batch (never attended, never a target)


def _lia_flags(kwargs):
    """generate()'s reading of the LIA kwargs (None -> the reference's defaults); decode-only extras pass through untouched"""
    kw = dict(kwargs)
    lia = {k: kw.pop(k, None) for k in LIA_KWARGS}
    lia = {"prefill_policy": 1 if lia["prefill_policy"] is None else lia["prefill_policy"],
           "decoding_policy": 1 if lia["decoding_policy"] is None else lia["decoding_policy"],
           "no_overlap": bool(lia["no_overlap"]), "pin_weight": bool(lia["pin_weight"]),
           "gpu_percentage": lia["gpu_percentage"] or 0, "num_minibatch": lia["num_minibatch"] or 1,
           "enable_cxl": bool(lia["enable_cxl"])}
    for k in ("cpu_layers", "cpu_layers_start", "max_new_tokens"):      # decode-only: accepted, no effect on a scoring pass
        kw.pop(k, None)
    if kw:
        raise TypeError(f"score() got unexpected keyword arguments {sorted(kw)}")
    return lia


def _is_llama(model):
    return getattr(model, "family", "opt") == "llama"


def score(model, input_ids, attention_mask=None, **lia_kwargs):
    """One scoring pass over input_ids [B, T] -> (logprobs float32 [B, T - 1], greedy bool [B, T - 1], valid bool [B, T - 1]), CPU:
        logprobs[b, t] = log p(ids[b, t + 1] | ids[b, :t + 1]),   greedy[b, t] = "ids[b, t + 1] is the greedy token there".
    attention_mask: a left-padded HF mask (OPT only); row b with s_b padding tokens has valid[b, t] = t >= s_b, and its invalid
    entries are 0.0 / False.  The LIA flags are generate()'s; decode-only ones are accepted and ignored."""
    lia = _lia_flags(lia_kwargs)
    ids = torch.as_tensor(input_ids, dtype=torch.int64).cpu()
    if ids.dim() != 2:
        raise ValueError("input_ids must be [batch, seq]")
    B, T = ids.shape
    if T < 2:
        raise ValueError(f"score() needs at least two tokens per row (T = {T}): the first token has no context to be predicted from")
    sh = model.shape
    if T > sh.max_pos:
        raise ValueError(f"sequence length {T} exceeds max positions {sh.max_pos}")
    if int(ids.min()) < 0 or int(ids.max()) >= sh.vocab:
        raise ValueError(f"input_ids outside the model's vocabulary of {sh.vocab} entries")
    starts = left_padding_starts(attention_mask, ids.shape)
    if starts is not None and _is_llama(model):
        raise ValueError(LLAMA_PADDING_REFUSAL)
    valid = torch.ones((B, T - 1), dtype=torch.bool)
    if starts is not None:
        valid = torch.arange(T - 1)[None, :] >= torch.from_numpy(starts.astype(np.int64))[:, None]
    targets = torch.full((B, T), -1, dtype=torch.int64)
    targets[:, :-1] = torch.where(valid, ids[:, 1:], torch.full_like(ids[:, 1:], -1))
    sched = _scheduler_of(model)

    def run():
        if _is_llama(model):
            from .llama import LlamaKVState
            kv = LlamaKVState(model, B, T)
        else:
            kv = sched.new_kv_state(B, T, 0, **lia)          # scratch: sized for T only
        return sched.score(ids, kv, targets, **lia)

    if starts is None:
        lp, gr = run()
    else:
        # the scheduler serves this pass with the row starts, cleared when it ends (as generate() does)
        sched.set_key_starts(starts)
        try:
            lp, gr = run()
        finally:
            sched.set_key_starts(None)
    lp = lp[:, :-1].to(torch.float32).cpu()
    gr = gr[:, :-1].cpu()
    logprobs = torch.where(valid, lp, torch.zeros_like(lp))
    greedy = (gr == ids[:, 1:]) & valid
    return logprobs, greedy, valid


def continuation_logprobs(model, state, cont_ids, append_policy=None):
    """cont_ids [B, Tc >= 1] scored against the cached conversation of `state` (generation.GenerationState) -> (logprobs float32
    [B, Tc], greedy bool [B, Tc]) on the CPU: logprobs[b, t] = log p(cont[b, t] | conversation, cont[b, :t]).  One appended block
    [pending | cont[:, :-1]] through the scheduler's score(): the first continuation token is scored from the pending token's
    position.  The state is not changed (its cache length stays; the block's K/V rows behind it are dead), so any number of
    continuations can be scored against one context.  The cache must have room for the block (generate(reserve_tokens=))."""
    from .generation import GenerationState
    if not isinstance(state, GenerationState):
        raise ValueError(f"state must be the GenerationState of generate(..., return_state=True), got {type(state).__name__}")
    cont = torch.as_tensor(cont_ids, dtype=torch.int64).cpu()
    if cont.dim() != 2 or cont.shape[0] != state.batch or cont.shape[1] < 1:
        raise ValueError(f"cont_ids must be [batch = {state.batch}, Tc >= 1], got {tuple(cont.shape)}")
    if int(cont.min()) < 0 or int(cont.max()) >= model.shape.vocab:
        raise ValueError(f"cont_ids outside the model's vocabulary of {model.shape.vocab} entries")
    B, Tc = cont.shape
    # (the schedulers score blocks of at least two tokens: a single continuation token takes itself along as an unscored input)
    block = torch.cat([state.pending[:, None], cont[:, :-1] if Tc > 1 else cont], dim=1)
    T = block.shape[1]
    if state.kv.len + T > state.kv.smax or state.kv.len + T > model.shape.max_pos:
        raise ValueError(f"the continuation needs {T} cache positions behind the {state.kv.len} cached ones, the cache has "
                         f"{state.room()} and the model {model.shape.max_pos} positions (give generate() a larger reserve_tokens)")
    targets = torch.full((B, T), -1, dtype=torch.int64)
    targets[:, :Tc] = cont
    sched = _scheduler_of(model)
    flags = dict(state.flags)
    if append_policy is not None:
        flags["append_policy"] = append_policy
    if state.starts is not None:
        sched.set_key_starts(state.starts)
    try:
        lp, gr = sched.score(block, state.kv, targets, **flags)
    finally:
        if state.starts is not None:
            sched.set_key_starts(None)
    return lp[:, :Tc].to(torch.float32).cpu(), gr[:, :Tc].cpu() == cont


def _max_len(model, max_len):
    max_len = int(model.shape.max_pos if max_len is None else max_len)
    if max_len < 2 or max_len > model.shape.max_pos:
        raise ValueError(f"max_len={max_len} must be in [2, max positions {model.shape.max_pos}]")
    return max_len


def _batches(lengths, batch_size, equal_length):
    """request indices grouped into batches: longest first (lm_eval's order, so the first batch is the largest one); equal_length:
    only rows of one length share a batch"""
    order = sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))
    out = []
    for i in order:
        if out and len(out[-1]) < batch_size and (not equal_length or lengths[out[-1][0]] == lengths[i]):
            out[-1].append(i)
        else:
            out.append([i])
    return out


def loglikelihood(model, pairs, batch_size=8, max_len=None, **lia_kwargs):
    """lm_eval's loglikelihood: pairs = [(context_ids, continuation_ids)] -> [(sum of the continuation tokens' log-probabilities,
    "every continuation token is the greedy one")] in request order.  The scored sequence is (context + continuation)[-max_len:]
    (max_len defaults to the model's max positions) and passes through score() whole.  lm_eval keeps max_len + 1 tokens and drops
    the last one as an input only; here a request truncated at the edge therefore has ONE TARGET FEWER: when the continuation alone
    has max_len tokens or more, its first kept token is the sequence's first token and is not scored.  OPT batches rows of
    different lengths by left padding; a Llama batches rows of equal length together."""
    if int(batch_size) < 1:
        raise ValueError(f"batch_size={batch_size} must be >= 1")
    max_len = _max_len(model, max_len)
    seqs, n_cont = [], []
    for i, (context, continuation) in enumerate(pairs):
        context, continuation = [int(t) for t in context], [int(t) for t in continuation]
        if not context or not continuation:
            raise ValueError(f"request {i}: context and continuation must each hold at least one token")
        seq = (context + continuation)[-max_len:]
        seqs.append(seq)
        n_cont.append(min(len(continuation), len(seq) - 1))
    results = [None] * len(seqs)
    llama = _is_llama(model)
    for batch in _batches([len(s) for s in seqs], int(batch_size), equal_length=llama):
        T = max(len(seqs[i]) for i in batch)
        ids = torch.full((len(batch), T), PAD_TOKEN_ID, dtype=torch.int64)
        mask = torch.zeros((len(batch), T), dtype=torch.int64)
        for r, i in enumerate(batch):
            ids[r, T - len(seqs[i]):] = torch.tensor(seqs[i], dtype=torch.int64)
            mask[r, T - len(seqs[i]):] = 1
        lp, gr, _ = score(model, ids, attention_mask=None if bool(mask.all()) else mask, **lia_kwargs)
        for r, i in enumerate(batch):
            n = n_cont[i]
            results[i] = (float(lp[r, T - 1 - n:].to(torch.float64).sum()), bool(gr[r, T - 1 - n:].all()))
    return results


def rolling_windows(token_ids, prefix_token, max_len):
    """lm_eval's get_rolling_token_windows(token_ids, prefix_token, max_len, context_len=1) + make_disjoint_window, restated:
    disjoint windows of at most max_len targets as (context, continuation) pairs.  The first is conditioned on prefix_token, a
    full later one on the last token of the window before it; a last window of n < max_len targets is, as in lm_eval, conditioned
    on the max_len + 1 - n tokens before it (the sequence is filled up to max_len + 1 tokens with context already scored)."""
    tokens = [int(t) for t in token_ids]
    if max_len < 1:
        raise ValueError(f"max_len={max_len} must be >= 1")
    out, done = [], 0
    while done < len(tokens):
        n = min(max_len, len(tokens) - done)
        end = done + n
        out.append(([int(prefix_token)] if done == 0 else tokens[end - max_len - 1:done], tokens[done:end]))
        done = end
    return out


def loglikelihood_rolling(model, token_ids, prefix_token, max_len=None, batch_size=1, **lia_kwargs):
    """lm_eval's loglikelihood_rolling: the log-likelihood of the whole token list, summed over rolling_windows of at most max_len
    targets (default: the model's max positions - 1: a window is at most max_len + 1 tokens, context included)."""
    max_len = int(model.shape.max_pos - 1 if max_len is None else max_len)
    if max_len < 1 or max_len + 1 > model.shape.max_pos:
        raise ValueError(f"max_len={max_len} must be in [1, max positions - 1 = {model.shape.max_pos - 1}]")
    windows = rolling_windows(token_ids, prefix_token, max_len)
    if not windows:
        raise ValueError("loglikelihood_rolling: no tokens")
    return float(sum(ll for ll, _ in loglikelihood(model, windows, batch_size=batch_size, max_len=max_len + 1, **lia_kwargs)))
