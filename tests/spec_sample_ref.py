"""NumPy restatement of sampled verification ("Sampled verification") on top of sample_ref.sample_ref: the contract
lia_lm_verify_sample is tested against.

For block row b at position t, on the verify pass's own logits [B, T, V]:
  suppress counts as -inf where t < n_suppress (a scalar, or one bound per row)
  s = steps[b] + t;  u = U[s, b] where s < len(U), else 0
  sampled[b, t] = sample_ref's id for (logits[b, t], settings, u)
  p_draft[b, t] = the kept weight of block_ids[b, t + 1] over the kept mass (0 if not kept, 0 at t = T - 1)
  accepted[b]   = the largest a <= T - 1 with block_ids[b, i + 1] == sampled[b, i] for all i < a; T - 1 where active[b] == 0
  common = min_b accepted[b];  next[b] = sampled[b, common]
"""
import collections

import numpy as np

from sample_ref import sample_ref

SpecRef = collections.namedtuple("SpecRef", "sampled accepted common next p_draft margin keep cum u")


def block_uniforms(U, steps, B, T):
    """u [B, T]: U[steps[b] + t, b], 0 past the table"""
    U = np.asarray(U, np.float32)
    steps = np.broadcast_to(np.asarray(steps, np.int64), (B,))
    s = steps[:, None] + np.arange(T)[None, :]
    inside = (s >= 0) & (s < U.shape[0])
    return np.where(inside, U[np.clip(s, 0, U.shape[0] - 1), np.arange(B)[:, None]], np.float32(0)).astype(np.float32)


def accept(block_ids, sampled, active=None):
    """(accepted [B], common, next [B]) of a block and the ids behind its positions"""
    block_ids, sampled = np.asarray(block_ids), np.asarray(sampled)
    B, T = block_ids.shape
    acc = np.zeros(B, np.int32)
    for b in range(B):
        a = T - 1
        if active is None or active[b]:
            a = 0
            while a < T - 1 and block_ids[b, a + 1] == sampled[b, a]:
                a += 1
        acc[b] = a
    common = int(acc.min())
    return acc, common, sampled[:, common].copy()


Draws = collections.namedtuple("Draws", "sampled margin keep cum u")


def sample_block(logits_f32, tau, top_k, top_p, U, steps, suppress=-1, n_suppress=0):
    """the draws behind every block position (the expensive part: it does not depend on block_ids) -> Draws"""
    logits_f32 = np.asarray(logits_f32, np.float32)
    B, T, V = logits_f32.shape
    u = block_uniforms(U, steps, B, T)
    n_sup = np.broadcast_to(np.asarray(n_suppress, np.int64), (B,))
    sampled = np.zeros((B, T), np.int64)
    margin = np.zeros((B, T))
    keep = np.zeros((B, T, V), bool)
    cum = np.zeros((B, T, V))
    for t in range(T):
        for sup_on in (False, True):                              # the rows with / without the suppressed token, each in one call
            rows = np.flatnonzero((t < n_sup) == sup_on)
            if rows.size == 0:
                continue
            ids, _, kp, mg, cm = sample_ref(logits_f32[rows, t], tau, top_k, top_p, u[rows, t], suppress if sup_on else -1)
            sampled[rows, t], margin[rows, t], keep[rows, t], cum[rows, t] = ids, mg, kp, cm
    return Draws(sampled, margin, keep, cum, u)


def spec_sample_ref(logits_f32, block_ids, tau, top_k, top_p, U, steps, suppress=-1, n_suppress=0, active=None, draws=None):
    """draws: a sample_block() result of the same logits and settings, to script block_ids from it without drawing twice"""
    d = draws if draws is not None else sample_block(logits_f32, tau, top_k, top_p, U, steps, suppress, n_suppress)
    block_ids = np.asarray(block_ids, np.int64)
    B, T = block_ids.shape
    V = d.keep.shape[2]
    p_draft = np.zeros((B, T), np.float64)
    rows = np.arange(B)
    for t in range(T - 1):
        tok = block_ids[:, t + 1]
        ok = (tok >= 0) & (tok < V)
        tk = np.where(ok, tok, 0)
        w = d.cum[rows, t, tk] - np.where(tk > 0, d.cum[rows, t, np.maximum(tk - 1, 0)], 0.0)        # the kept weight
        p_draft[:, t] = np.where(ok & d.keep[rows, t, tk], w / d.cum[:, t, -1], 0.0)
    acc, common, nxt = accept(block_ids, d.sampled, active)
    return SpecRef(d.sampled, acc, common, nxt, p_draft, d.margin, d.keep, d.cum, d.u)
