"""Speculative decoding: a drafter proposes k tokens per row, the target model verifies the block
[pending | proposal] in ONE pass of its weights (scheduler.verify) and keeps what its own greedy search would have produced.

The cache length stays one integer per batch: a round accepts `common` draft tokens on every row, the minimum over the active rows'
own counts, plus the target's token behind them.  That is exact -- the output is the greedy output -- and pays where one pass of the
weights is the cost of a token and the batch is small; at a large batch the minimum collapses towards 0.

    out = generate(model, ids, max_new_tokens=N, draft=ModelDrafter(small_model), draft_tokens=4, spec_log=log, **lia_flags)

A drafter is any object with  propose(ids [B, n] int64 CPU, k, suppress) -> int64 [B, k]:  its guess of the k tokens behind ids.
suppress = (token, n): the target will not produce `token` (EOS below min_new_tokens) as the first n of them; a drafter that ignores
it only loses acceptance.  An optional attribute `vocab` is checked against the target's.

Row mode, generate(..., acceptance="row") (speculative_search_rows): OPT targets whose KV cache lives in HBM on every layer
(policies 3 / 3) keep one cache length PER ROW -- row b appends accepted[b] + 1 tokens per round, whatever the other rows accept, and
the number of target passes is set by the slowest row's own acceptance.  The drafter then needs
propose_rows(rows: list of 1-D int64 CPU tensors, k, suppress_rows) -> int64 [B, k]  with suppress_rows = (token, [n per row]).

Sampled verification, generate(..., do_sample=True, sampled_verify=True, draft=...): the verify pass draws every block position with
the uniform the plain sampled loop would use there (U[generated so far + t, row]); a draft token is accepted iff it equals that
draw, and the emitted token is always the draw.  The ids are the same function of (logits, U) as plain sampled decoding's.

Rejection verification, generate(..., do_sample=True, sampled_verify=True, verify_rule="rejection", draft=ModelDrafter(m,
stochastic=True)): the drafter SAMPLES its own logits (U_draft), the verify pass accepts a draft token x with probability
min(1, P(x) / Q(x)) (U_acc) and emits a draw of norm(max(P - Q, 0)) at the first rejection (U_res) -- the rule of Leviathan et al.
The output is an exact sample of the target's filtered distribution, but NOT the ids plain sampling draws from the same seed.
"""
import time

import numpy as np
import torch

REFUSALS = {
    "do_sample": "draft together with do_sample=True is not supported: verification keeps the GREEDY token of every position "
                 "(sampled_verify=True verifies with the sampler's own draws instead)",
    "sampled_verify": "sampled_verify=True needs do_sample=True and draft=: it is speculative decoding whose verify pass draws every "
                      "position with the generation's own uniforms",
    "return_logits": "draft together with return_logits=True is not supported: a verify pass never materialises the logits",
    "dp": "draft together with a data-parallel group is not supported: the ranks would accept different counts",
    "cpu_layers": "draft together with cpu_layers=-1 (the online cooperative split) is not supported: the controller samples "
                  "single-token decode steps; name a fixed cpu_layers",
}


VERIFY_RULES = ("draw", "rejection")
REJECT_REFUSALS = {
    "rule": "verify_rule must be 'draw' (accept a draft token iff it equals the sampler's own draw) or 'rejection' (accept it with "
            "probability min(1, p / q), else draw from the residual)",
    "sampled_verify": "verify_rule='rejection' needs sampled_verify=True (with do_sample=True and draft=): it is a rule of sampled "
                      "verification",
    "stochastic": "verify_rule='rejection' needs a drafter that declares stochastic=True and keeps draft_logits: the rule divides by "
                  "the probability the drafter drew its token with",
    "coupled": "a drafter cannot be stochastic and coupled: a coupled drafter draws with the TARGET's uniforms (verify_rule='draw'), a "
               "stochastic one with uniforms of its own (verify_rule='rejection')",
    "row": "verify_rule='rejection' together with acceptance='row' is not supported: the row-mode drafter suppresses at the smallest n "
           "of the rows, so Q would not be what every row's token was drawn from",
}


def check_verify_rule(verify_rule, sampled_verify, draft, acceptance):
    """every refusal of generate(verify_rule=), by name (ValueError), before any forward"""
    if verify_rule not in VERIFY_RULES:
        raise ValueError(REJECT_REFUSALS["rule"] + f", got {verify_rule!r}")
    if getattr(draft, "stochastic", False) and getattr(draft, "coupled", False):
        raise ValueError(REJECT_REFUSALS["coupled"])
    if verify_rule != "rejection":
        return
    if not sampled_verify or draft is None:
        raise ValueError(REJECT_REFUSALS["sampled_verify"])
    if not getattr(draft, "stochastic", False):
        raise ValueError(REJECT_REFUSALS["stochastic"] + f", got {type(draft).__name__}")
    if acceptance == "row":
        raise ValueError(REJECT_REFUSALS["row"])


ACCEPTANCE = ("common", "row")
ROW_REFUSALS = {
    "llama": "acceptance='row' is not supported for Llama-family models: their RoPE positions are one per batch, not per row yet",
    "state": "acceptance='row' together with return_state=True or past= is not supported: a GenerationState has one cache length, "
             "row mode keeps one per row",
    "flags": "acceptance='row' needs the KV cache in HBM on every layer: prefill_policy=3 and decoding_policy=3 (any gpu_percentage)",
    "cpu_layers": "acceptance='row' together with cpu_layers is not supported: a host-computed layer keeps its cache on the host",
    "propose_rows": "acceptance='row' needs a drafter with propose_rows(rows, k, suppress_rows)",
    "llama_draft": "acceptance='row' with a Llama draft model is not supported: ModelDrafter.propose_rows re-prefills left padded, "
                   "which the Llama path does not have",
}


def check_acceptance(acceptance):
    if acceptance not in ACCEPTANCE:
        raise ValueError(f"acceptance must be 'common' or 'row', got {acceptance!r}")


def row_flags_refusal(lia):
    """the refusal (a ROW_REFUSALS text) of a flag set row mode does not serve, or None"""
    if lia.get("prefill_policy", 1) != 3 or lia.get("decoding_policy", 1) != 3:
        return ROW_REFUSALS["flags"] + f"; got {lia.get('prefill_policy', 1)} / {lia.get('decoding_policy', 1)}"
    if lia.get("cpu_layers", 0) != 0:
        return ROW_REFUSALS["cpu_layers"]
    return None


def largest_row_block(shape, T, max_new_tokens, k):
    """the largest draft_tokens <= k whose verify block (k + 1 queries, a cache of T + max_new_tokens + k positions) the ragged block
    attention takes (ops.block_attention_takes: the launch's own rule), or 0"""
    from . import ops
    kvh = getattr(shape, "kv_heads", shape.heads)
    for kk in range(k, 0, -1):
        if ops.block_attention_takes(shape.heads, kvh, shape.head_dim, kk + 1, T + max_new_tokens + kk):
            return kk
    return 0


def check_row_mode(model, draft, k, lia, T, max_new_tokens, past=None, return_state=False):
    """every refusal of generate(draft=, acceptance="row"), by name (ValueError), before any forward"""
    if getattr(model, "family", "opt") == "llama":
        raise ValueError(ROW_REFUSALS["llama"])
    if past is not None or return_state:
        raise ValueError(ROW_REFUSALS["state"])
    why = row_flags_refusal(lia)
    if why:
        raise ValueError(why)
    if not callable(getattr(draft, "propose_rows", None)):
        raise ValueError(ROW_REFUSALS["propose_rows"] + f", got {type(draft).__name__}")
    if isinstance(draft, ModelDrafter) and getattr(draft.model, "family", "opt") == "llama":
        raise ValueError(ROW_REFUSALS["llama_draft"])
    fit = largest_row_block(model.shape, T, max_new_tokens, k)
    if fit != k:
        raise ValueError(f"acceptance='row': the ragged block attention does not take a verify block of draft_tokens={k} + 1 queries on "
                         f"a cache of {T + max_new_tokens + k} positions ({model.shape.heads} heads of {model.shape.head_dim}); "
                         + (f"the largest draft_tokens that fits is {fit}" if fit else "no draft_tokens fits"))


def block_attention_pays(head_dim, heads, kv_heads, B, T, pos0):
    """Where the block attention launch beat the append launch by more than the ~20 % run-to-run spread of such short launches
    (results/attn_block_bench.txt, one MI355X) -- and nowhere else: a shape that was not measured keeps the append launch.
    Measured: d = 128 with G = heads / kv_heads = 1 (OPT-30B's 56 heads, B 1 / 4 / 64, pos0 288 / 2048, T 2 / 3 / 5 / 8) and G = 4
    (Llama-3-8B's 32 / 8, B 1 / 128, pos0 1024, T 2 / 4).  In work = (B x kv_heads workgroups) x keys:
        G 1: T 2 everywhere (1.4 - 2.1 x); T 3 from ~1e5 (1.3 - 1.8 x; 1.16 - 1.18 x below); T 4, 5 from ~4e6 (1.5 x at B 64, pos0 2048;
             0.8 - 1.2 x below; T 4 by its neighbours); T >= 6 nowhere (T 8: 0.4 - 0.8 x)
        G 4: T 2 and 4 (and 3 between them) from 512 workgroups (2.4 x / 1.3 x at B 128; 0.5 - 0.8 x at B 1)"""
    if head_dim != 128 or heads % kv_heads:
        return False
    G, wgs = heads // kv_heads, B * kv_heads
    work = wgs * (pos0 + T)
    if G == 1:
        return T == 2 or (T == 3 and work >= 100000) or (T in (4, 5) and work >= 4000000)
    if G == 4:
        return 2 <= T <= 4 and wgs >= 512
    return False


def block_attention_for(sched, shape, B, T, pos0):
    """LIA_OPT_BLOCK_ATTENTION of one verify pass: the scheduler's block_attention -- True / False, or "measured": the table above"""
    mode = getattr(sched, "block_attention", "measured")
    if mode == "measured":
        return block_attention_pays(shape.head_dim, shape.heads, getattr(shape, "kv_heads", shape.heads), B, T, pos0)
    return bool(mode)


def check_settings(model, sched, draft, draft_tokens, do_sample, return_logits, lia, sampled_verify=False):
    """every refusal of generate(draft=), by name (ValueError).  Sampling is opt-in: do_sample=True is served with
    sampled_verify=True only, and sampled_verify=True with do_sample=True only."""
    if sampled_verify and not do_sample:
        raise ValueError(REFUSALS["sampled_verify"])
    if do_sample and not sampled_verify:
        raise ValueError(REFUSALS["do_sample"])
    if return_logits:
        raise ValueError(REFUSALS["return_logits"])
    if getattr(sched, "dp", None) is not None:
        raise ValueError(REFUSALS["dp"])
    if lia.get("cpu_layers", 0) < 0:
        raise ValueError(REFUSALS["cpu_layers"])
    if isinstance(draft_tokens, bool) or not isinstance(draft_tokens, int) or draft_tokens < 1:
        raise ValueError(f"draft_tokens must be an int >= 1, got {draft_tokens!r}")
    if not callable(getattr(draft, "propose", None)):
        raise ValueError(f"draft must have propose(ids, k, suppress), got {type(draft).__name__}")
    vocab = getattr(draft, "vocab", None)
    if vocab is not None and vocab != model.shape.vocab:
        raise ValueError(f"the draft model has a vocabulary of {vocab} tokens, the target {model.shape.vocab}: their ids do not mean the same")


class ReplayDrafter:
    """Proposes a recorded continuation: ids [B, N] holds the prompt and what the target is known to generate behind it (its own
    earlier output, an oracle's).  corrupt (optional): per round r a list with, per row, the number a of leading proposal tokens
    left right -- token a of that row's proposal is made wrong (its lowest bit flipped), the tokens behind it are right again; an
    entry >= k, None, or a round past the end of the list leaves the row alone.  For tests and measurements: the acceptance of
    every round is scripted."""

    def __init__(self, ids, corrupt=None):
        self.ids = torch.as_tensor(ids, dtype=torch.int64).cpu()
        self.corrupt = list(corrupt) if corrupt is not None else []
        self.rounds = 0

    def script(self, r, B, k):
        """per row, the scripted number of right leading tokens of round r (k: all of them)"""
        row = self.corrupt[r] if r < len(self.corrupt) and self.corrupt[r] is not None else [None] * B
        return [k if a is None else min(int(a), k) for a in row]

    def propose(self, ids, k, suppress=(-1, 0)):
        B, n = ids.shape
        out = torch.zeros((B, k), dtype=torch.int64)
        have = max(0, min(k, self.ids.shape[1] - n))
        out[:, :have] = self.ids[:, n:n + have]
        for b, a in enumerate(self.script(self.rounds, B, k)):
            if a < k:
                out[b, a] ^= 1
        self.rounds += 1
        return out


    def propose_rows(self, rows, k, suppress_rows=(-1, None)):
        """propose() for rows of their own lengths (row mode): row b continues the recording behind its len(rows[b]) tokens; the
        script is the same, one entry per round"""
        B = len(rows)
        out = torch.zeros((B, k), dtype=torch.int64)
        for b, row in enumerate(rows):
            n = int(row.shape[0])
            have = max(0, min(k, self.ids.shape[1] - n))
            out[b, :have] = self.ids[b, n:n + have]
        for b, a in enumerate(self.script(self.rounds, B, k)):
            if a < k:
                out[b, a] ^= 1
        self.rounds += 1
        return out


class ModelDrafter:
    """A second, all-resident model (policy 3 / 3, gpu_percentage 100) with its own scheduler, context and cache.  Every round it
    feeds the tokens its cache lacks -- one, or two after a fully accepted round -- through the decode / append paths and runs
    k - 1 more decode steps whose argmax stays on the device.  Its cache length is rolled back to the common prefix of what it was
    fed and the ids it is given; it prefills again when that prefix is empty, the batch changed or the cache is too small (a new
    conversation, a new turn of past=).

    coupled=True (sampled verification only): the loops hand propose / propose_rows the round's sampling.SamplerBlock, and draft
    step i samples the drafter's own logits with the target's settings and the target's uniform of that position, U[g_b + i, b]
    (0 past the table) -- it guesses the target's DRAW, not its argmax, and is right wherever the two models' running masses put
    that uniform on the same token.  A drafter only ever changes how many positions a round keeps, never a token.

    stochastic=True (rejection verification only): the loop hands propose the round's sampling.RejectorBlock, and draft step i
    samples the drafter's own logits with the target's settings and a uniform of its own, U_draft[g + i, b]; step i suppresses iff
    i < n_sup, the rule the verify head applies to both models' rows.  The k steps' logits stay on the device as draft_logits
    (bf16 [B, k, vocab]): the Q the tokens were drawn from."""

    FLAGS = dict(prefill_policy=3, decoding_policy=3, gpu_percentage=100, pin_weight=True)

    def __init__(self, model, reserve=64, coupled=False, stochastic=False):
        from .generation import _scheduler_of
        if coupled and stochastic:
            raise ValueError(REJECT_REFUSALS["coupled"])
        self.model, self.sched, self.reserve, self.coupled = model, _scheduler_of(model), reserve, bool(coupled)
        self.stochastic = bool(stochastic)
        self.draft_logits = None
        self.vocab = model.shape.vocab
        self.kv = None
        self.fed = None          # int64 [B, kv.len]: the tokens whose K/V the cache holds
        self.prefills = self.rounds = 0

    def _new_cache(self, B, n, k):
        smax = min(n + k + self.reserve, self.model.shape.max_pos)
        if getattr(self.model, "family", "opt") == "llama":
            from .llama import LlamaKVState
            return LlamaKVState(self.model, B, smax)
        return self.sched.new_kv_state(B, n, smax - n, **self.FLAGS)

    def _step_kw(self, sampler, k):
        """the forward keywords of draft steps 0 .. k - 1: the coupled draws (gathered once per round), or none (the argmax)"""
        if not self.coupled or sampler is None:
            return [{}] * k
        return [{"sampler": s} for s in sampler.draft_steps(k)]

    def propose(self, ids, k, suppress=(-1, 0), sampler=None, rejector=None):
        ids = torch.as_tensor(ids, dtype=torch.int64).cpu()
        B, n = ids.shape
        tok, n_sup = suppress
        if n + k > self.model.shape.max_pos:
            raise ValueError(f"the draft model has max positions {self.model.shape.max_pos}, the round reaches {n + k}")
        keep = 0
        if self.kv is not None and self.fed is not None and self.fed.shape[0] == B and self.kv.smax >= n + k:
            m = min(self.fed.shape[1], n - 1)
            same = (self.fed[:, :m] == ids[:, :m]).all(dim=0).long()
            keep = int(same.cumprod(0).sum())
        if keep == 0:
            self.kv = self._new_cache(B, n, k)
            self.prefills += 1
        self.kv.len = keep
        cur = ids[:, keep:]
        dev, step_kw = [], self._step_kw(sampler, k)
        keep_logits = self.stochastic and rejector is not None
        if keep_logits:
            step_kw, kept = [{"sampler": smp} for smp in rejector.draft_steps(k)], []
        for i in range(k):
            sup = tok if i < n_sup else -1
            logits, nxt = self.sched.forward(cur, self.kv, max_new_tokens=k, suppress_token=sup, **step_kw[i], **self.FLAGS)
            dev.append(nxt)
            if keep_logits:
                kept.append(logits)
            cur = nxt.view(B, 1)
        out = torch.stack(dev, dim=1).cpu()
        self.draft_logits = torch.stack(kept, dim=1) if keep_logits else None
        self.fed = torch.cat([ids, out[:, :k - 1]], dim=1)
        self.rounds += 1
        return out


    def propose_rows(self, rows, k, suppress_rows=(-1, None), pad_token_id=1, sampler=None):
        """Row mode's baseline: every round is a fresh generation of its own -- the rows right-aligned (left padded to the longest),
        prefilled through the attention_mask machinery (the scheduler's key starts), then k - 1 decode steps.  No cache is kept
        between rounds.  suppress_rows = (token, [n per row]): `token` is suppressed at the steps below the SMALLEST n, so the
        drafter never suppresses where the target would not (a drafter that suppresses too little only loses acceptance)."""
        if getattr(self.model, "family", "opt") == "llama":
            raise ValueError(ROW_REFUSALS["llama_draft"])
        B = len(rows)
        lens = [int(r.shape[0]) for r in rows]
        n = max(lens)
        if n + k > self.model.shape.max_pos:
            raise ValueError(f"the draft model has max positions {self.model.shape.max_pos}, the round reaches {n + k}")
        ids = torch.full((B, n), pad_token_id, dtype=torch.int64)
        for b, r in enumerate(rows):
            ids[b, n - lens[b]:] = torch.as_tensor(r, dtype=torch.int64)
        starts = np.asarray([n - v for v in lens], dtype=np.int32)
        tok, n_rows = suppress_rows
        n_sup = min(n_rows) if n_rows is not None and len(n_rows) else 0
        kv = self.sched.new_kv_state(B, n, k, **self.FLAGS)
        self.kv = self.fed = None                      # (a later propose() of common mode starts from a fresh cache)
        self.sched.set_key_starts(starts if starts.any() else None)
        try:
            cur, dev, step_kw = ids, [], self._step_kw(sampler, k)
            for i in range(k):
                sup = tok if i < n_sup else -1
                _, nxt = self.sched.forward(cur, kv, max_new_tokens=k, suppress_token=sup, **step_kw[i], **self.FLAGS)
                dev.append(nxt)
                cur = nxt.view(B, 1)
            out = torch.stack(dev, dim=1).cpu()
        finally:
            self.sched.set_key_starts(None)
        self.prefills += 1
        self.rounds += 1
        return out


# Sampled verification reaches the schedulers and the drafters through keywords that exist only on that route: without a sampler
# the loops make exactly the calls they made before it existed.
def _first_kw(sampler):
    return {} if sampler is None else {"sampler": sampler.at(0)}


def _verify_kw(view):
    return {} if view is None else {"sampler": view}


def _draft_kw(draft, view):
    """the round's sampler view, for drafters that declare `coupled` only"""
    return {"sampler": view} if (view is not None and getattr(draft, "coupled", False)) else {}


def _reject_kw(view):
    return {} if view is None else {"rejector": view}


def speculative_search_rows(model, sched, input_ids, max_new_tokens, min_new_tokens, eos_token_id, pad_token_id, token_latency, lia,
                            draft, draft_tokens, spec_log=None, step_hook=None, max_steps=None, starts=None, sampler=None):
    """speculative_search with one cache length per row (acceptance="row").  Row b has generated g[b] tokens, caches T + g[b] - 1
    positions (its last token is pending), and appends greedy[b, :accepted[b] + 1] per round, cut behind its EOS token and at
    max_new_tokens.  A finished or full row is inactive: its block is pad tokens, its length stands still, it never holds another
    row back.  The output is _greedy_search's: finished rows padded with pad_token_id up to the length the greedy loop would have
    reached (the longest row's).  latency_list has one entry per target pass; spec_log receives (min over the active rows,
    accepted per row) per round.  sampler (the generation's sampling.Sampler, sampled verification): the first forward draws with
    U[0], a round's block position t of row b with U[g[b] + t, b]; the sampled ids stand where `greedy` stood."""
    k = draft_tokens
    ids = torch.as_tensor(input_ids, dtype=torch.int64).cpu()
    if ids.dim() != 2:
        raise ValueError("input_ids must be [batch, seq]")
    B, T = ids.shape
    check_row_mode(model, draft, k, lia, T, max_new_tokens)
    if T + max_new_tokens + k > model.shape.max_pos:
        raise ValueError(f"prompt {T} + max_new_tokens {max_new_tokens} + draft_tokens {k} exceeds max positions {model.shape.max_pos}")
    kv = sched.new_kv_state(B, T, max_new_tokens + k, **lia)
    limit = max_new_tokens if max_steps is None else min(max_new_tokens, max_steps)
    ids_buf = torch.full((B, T + max_new_tokens), pad_token_id, dtype=torch.int64)
    ids_buf[:, :T] = ids
    g = np.zeros(B, dtype=np.int64)                    # tokens generated per row
    unfinished = np.ones(B, dtype=bool)
    latency_list = []

    def append(b, token):
        ids_buf[b, T + g[b]] = token
        g[b] += 1
        if eos_token_id is not None and token == eos_token_id:
            unfinished[b] = False

    if step_hook is not None:
        step_hook(0)
    tic = time.time()
    suppress = eos_token_id if (eos_token_id is not None and 0 < min_new_tokens) else -1
    _, nxt = sched.forward(ids, kv, max_new_tokens=max_new_tokens, suppress_token=suppress, **_first_kw(sampler), **lia)
    for b, token in enumerate(nxt.cpu().tolist()):
        append(b, token)
    latency_list.append(time.time() - tic)
    rnd = 0
    while True:
        active = unfinished & (g < limit)
        if not active.any():
            break
        rnd += 1
        if step_hook is not None:
            step_hook(rnd)
        tic = time.time()
        row_lens = (T + g - 1).astype(np.int32)
        n_sup = np.clip(min_new_tokens - g, 0, k + 1).astype(np.int32) if eos_token_id is not None else np.zeros(B, np.int32)
        sup_tok = eos_token_id if n_sup.any() else -1
        rows = [ids_buf[b, :T + g[b]] for b in range(B)]
        view = None if sampler is None else sampler.block_rows(g)
        prop = torch.as_tensor(draft.propose_rows(rows, k, (sup_tok, np.minimum(n_sup, k).tolist()), **_draft_kw(draft, view)),
                               dtype=torch.int64).cpu()
        if tuple(prop.shape) != (B, k):
            raise ValueError(f"draft.propose_rows returned shape {tuple(prop.shape)}, expected {(B, k)}")
        block = torch.cat([torch.stack([r[-1] for r in rows])[:, None], prop], dim=1)
        block[torch.from_numpy(~active)] = pad_token_id                      # an inactive row is fed pad tokens
        res = sched.verify_rows(block, kv, row_lens, suppress_token=sup_tok, n_suppress_rows=n_sup,
                                active=torch.from_numpy(active.astype(np.int32)), **_verify_kw(view), **lia)
        greedy, acc = res.greedy.cpu(), res.accepted.cpu().tolist()
        if spec_log is not None:
            spec_log.append((min(a for a, on in zip(acc, active) if on), acc))
        for b in np.flatnonzero(active):
            for i in range(acc[b] + 1):
                append(b, int(greedy[b, i]))
                if not unfinished[b] or g[b] >= limit:
                    break
        latency_list.append(time.time() - tic)
    step = int(g.max())                                # where the greedy loop stops: every row finished, or the limit
    out = ids_buf[:, :T + step].clone() if step < max_new_tokens else ids_buf
    return (out, latency_list) if token_latency else out


def speculative_search(model, sched, input_ids, max_new_tokens, min_new_tokens, eos_token_id, pad_token_id, token_latency, lia,
                       draft, draft_tokens, spec_log=None, step_hook=None, max_steps=None, past=None, return_state=False,
                       reserve_tokens=0, starts=None, sampler=None, rejector=None, constraint=None, logprobs=None):
    """_greedy_search with a drafter: the ordinary prefill, then rounds of propose -> verify -> append.  The EOS / pad / unfinished
    bookkeeping is applied token by token as the greedy loop applies it; a finished row is inactive (it never limits `common`, its
    block is pad tokens, as the greedy loop feeds them); a round ends behind the token at which a row finishes, so the cache holds
    exactly what the greedy loop would have fed.  latency_list has one entry per target pass.
    sampler (the generation's sampling.Sampler, sampled verification): the first forward draws with U[0] as the plain sampled loop
    does, and a round that starts with g generated tokens draws block position t with U[g + t] -- the token at generated step s is
    lia_sample(logits(prefix), U[s]) on either loop; the sampled ids stand where `greedy` stood.
    rejector (the generation's sampling.Rejector, in place of sampler: rejection verification): the first forward draws with U[0]; a
    round hands the drafter and the verify pass the view of step origin g, gives the view the drafter's draft_logits, and emits the
    `common` draft tokens every active row accepted and then res.next -- per row its own accepted draft token or the head's token.
    constraint (constraints.Constraint; greedy and the draw rule): the first forward takes step 0's token mask, a verify pass one row
    per (row, position) -- position t's built from ids + draft[:t].  The drafter is not told: a proposal the mask forbids is simply
    not accepted, and the ids are those of the plain constrained run.
    logprobs (int N; greedy and the draw rule): the first forward and every verify pass take a logprobs.LogprobRequest; a round keeps
    the verify head's rows t = 0 .. common of every row -- the accepted draft tokens and the correction token, each the head's own
    id at its position -- for exactly the tokens it appends; a TokenLogprobs follows the other results."""
    from . import logprobs as token_logprobs
    from .generation import GenerationState, turn_positions
    if rejector is not None:
        sampler = None
    k = draft_tokens
    ids = torch.as_tensor(input_ids, dtype=torch.int64).cpu()
    if ids.dim() != 2:
        raise ValueError("input_ids must be [batch, seq]")
    first = ids
    if past is not None:
        first = torch.cat([past.pending[:, None], ids], dim=1)
        need = turn_positions(past.kv.len, ids.shape[1], max_new_tokens) + k
        if need > past.kv.smax:
            raise ValueError(f"the turn needs {need} cache positions with draft_tokens={k} (a verify block overhangs by {k}), the cache "
                             f"holds {past.kv.smax} (give the first turn a larger reserve_tokens)")
        if need + 1 > model.shape.max_pos:
            raise ValueError(f"the conversation would reach {need + 1} positions with draft_tokens={k}, the model has max positions {model.shape.max_pos}")
        ids = torch.cat([past.ids, ids], dim=1)
    B, T = ids.shape
    reserve = reserve_tokens if past is None else 0
    if past is None and T + max_new_tokens + reserve + k > model.shape.max_pos:
        raise ValueError(f"prompt {T} + max_new_tokens {max_new_tokens}" + (f" + reserve_tokens {reserve}" if reserve else "")
                         + f" + draft_tokens {k} exceeds max positions {model.shape.max_pos}")
    if past is not None:
        kv = past.kv
    elif getattr(model, "family", "opt") == "llama":
        from .llama import LlamaKVState
        kv = LlamaKVState(model, B, T + max_new_tokens + reserve + k)
    else:
        kv = sched.new_kv_state(B, T, max_new_tokens + reserve + k, **lia)
    unfinished = torch.ones(B, dtype=torch.int64)
    latency_list = []
    ids_buf = torch.empty((B, T + max_new_tokens), dtype=torch.int64)
    ids_buf[:, :T] = ids
    limit = max_new_tokens if max_steps is None else min(max_new_tokens, max_steps)
    state = {"step": 0, "unfinished": unfinished}
    recorder = None if logprobs is None else token_logprobs.Recorder(B, max_new_tokens, logprobs)

    def append(tokens, values=None):
        """one generated token per row, greedy_search.py:398-421; True when the generation is over.  values: the head's
        (chosen, top_ids, top_logprobs) of these tokens, recorded for the rows that were unfinished before them"""
        unf = state["unfinished"]
        if values is not None:
            recorder.record(state["step"], unf if eos_token_id is not None else None, *values)
        if eos_token_id is not None:
            tokens = tokens * unf + pad_token_id * (1 - unf)
        ids_buf[:, T + state["step"]] = tokens
        newly = False
        if eos_token_id is not None:
            nxt_unf = unf * (tokens != eos_token_id).long()
            newly = bool((nxt_unf != unf).any())
            state["unfinished"] = nxt_unf
        state["step"] += 1
        over = (eos_token_id is not None and int(state["unfinished"].max()) == 0) or state["step"] >= limit
        return over, newly

    # the prefill (or the turn's block): an ordinary forward
    if step_hook is not None:
        step_hook(0)
    tic = time.time()
    suppress = eos_token_id if (eos_token_id is not None and 0 < min_new_tokens) else -1
    first_mask = {} if constraint is None else {"token_mask": constraint.step_mask(0, ids, unfinished, suppress)}
    request = None if recorder is None else recorder.request()
    lp_kw = {} if request is None else {"logprobs": request}
    _, nxt = sched.forward(first, kv, max_new_tokens=max_new_tokens, suppress_token=suppress,
                           **_first_kw(sampler if rejector is None else rejector.sampler), **first_mask, **lp_kw, **lia)
    if recorder is None:
        over, _ = append(nxt.cpu())
    else:
        tokens, *values = token_logprobs.fetch(nxt, request)
        over, _ = append(tokens, values)
    latency_list.append(time.time() - tic)
    rnd = 0
    while not over:
        rnd += 1
        if step_hook is not None:
            step_hook(rnd)
        tic = time.time()
        g = state["step"]
        pos0 = kv.len
        n_sup = int(np.clip(min_new_tokens - g, 0, k + 1)) if eos_token_id is not None else 0
        sup_tok = eos_token_id if n_sup else -1
        active = state["unfinished"]
        view = None if sampler is None else sampler.block(g)
        rview = None if rejector is None else rejector.block(g)
        prop = torch.as_tensor(draft.propose(ids_buf[:, :T + g], k, (sup_tok, min(n_sup, k)), **_draft_kw(draft, view), **_reject_kw(rview)),
                               dtype=torch.int64).cpu()
        if tuple(prop.shape) != (B, k):
            raise ValueError(f"draft.propose returned shape {tuple(prop.shape)}, expected {(B, k)}")
        if eos_token_id is not None:
            prop = prop * active[:, None] + pad_token_id * (1 - active[:, None])      # a finished row is fed pad tokens
        block = torch.cat([ids_buf[:, T + g - 1:T + g], prop], dim=1)
        if rview is not None:
            rview.draft_logits = draft.draft_logits        # [B, k, vocab]: the Q behind prop (a finished row's is never looked at)
        mask_kw = {} if constraint is None else {"token_mask": constraint.block_mask(g, ids_buf[:, :T + g], prop, active, sup_tok, n_sup)}
        request = None if recorder is None else recorder.request()
        lp_kw = {} if request is None else {"logprobs": request}
        res, common = sched.verify(block, kv, suppress_token=sup_tok, n_suppress=n_sup, active=active.to(torch.int32), **_verify_kw(view),
                                   **_reject_kw(rview), **mask_kw, **lp_kw, **lia)
        values = None
        if recorder is not None:                           # (never with a rejector: generate() refuses the pair)
            greedy, *values = token_logprobs.fetch(res.greedy, request)
        elif rview is None:
            greedy = res.greedy.cpu()
        else:                                              # the accepted draft tokens, then each row's token behind them
            greedy = torch.cat([block[:, 1:common + 1], res.next.cpu()[:, None]], dim=1)
        if spec_log is not None:
            spec_log.append((common, res.accepted.cpu().tolist()))
        n_app = 0
        for i in range(common + 1):
            over, newly = append(greedy[:, i], None if values is None else [v[:, i] for v in values])
            n_app += 1
            if over or newly:
                break
        kv.len = pos0 + n_app          # the block's rows behind it are dead: the next round rewrites them
        latency_list.append(time.time() - tic)
    step = state["step"]
    out = ids_buf[:, :T + step].clone() if step < max_new_tokens else ids_buf
    res = (out, latency_list) if token_latency else (out,)
    if recorder is not None:
        res = res + (recorder.result(step),)
    if return_state:
        flags = past.flags if past is not None else {key: v for key, v in lia.items() if key != "append_policy"}
        res = res + (GenerationState(kv, out.clone(), starts, flags),)
    return res if len(res) > 1 else res[0]
