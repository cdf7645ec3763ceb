"""Float64 restatement of sampled decoding ("Sampled decoding"): the contract lia_sample is tested against.

Per row of bf16 logits l (given here as their exact fp32 values):
  s = fp32(l) / fp32(tau) (IEEE fp32), s[suppress] = -inf; a token with s = -inf is never kept
  top-k (0 < k < vocab): K1 = {s >= t_k}, t_k the k-th largest s counting multiplicity
  top-p (p < 1): w = exp(s - max s) over K1; keep i iff the mass of K1 tokens with a strictly larger s is < p * sum(w over K1)
  draw: the smallest kept id whose running mass in id order exceeds u * W2 (W2 = the kept mass), else the last kept id
All rows at once (numpy, sorted along the row).
"""
import numpy as np


def scores(logits_f32, tau, suppress=-1):
    s = (np.asarray(logits_f32, np.float32) / np.float32(tau)).astype(np.float32)
    if suppress >= 0:
        s[:, suppress] = -np.inf
    return s


def sample_ref(logits_f32, tau, top_k, top_p, u, suppress=-1):
    """ids [B], stats [B, 4] (t_k, top-p boundary s, |K2|, W2 -- -inf for a filter that is off), keep [B, V] bool, and the margins
    of each row: topp_margin (min over tie groups of |mass ahead - p W| / W, inf with top-p off), cum [B, V] (running kept mass)"""
    s = scores(logits_f32, tau, suppress)
    B, V = s.shape
    fin = s > -np.inf
    order = np.argsort(-s, axis=1, kind="stable")
    sd = np.take_along_axis(s, order, axis=1)                   # descending
    t_k = np.full(B, -np.inf, np.float32)
    if 0 < top_k < V:
        t_k = sd[:, top_k - 1].copy()
    k1 = fin & (s >= t_k[:, None])
    m = sd[:, 0].astype(np.float64)
    w = np.where(k1, np.exp(s.astype(np.float64) - m[:, None]), 0.0)
    v_p = np.full(B, -np.inf, np.float32)
    keep = k1
    margin = np.full(B, np.inf)
    if top_p < 1:
        wd = np.take_along_axis(w, order, axis=1)
        W = wd.sum(axis=1)
        excl = np.cumsum(wd, axis=1) - wd
        first = np.where(np.concatenate([np.ones((B, 1), bool), sd[:, 1:] != sd[:, :-1]], axis=1), np.arange(V)[None, :], 0)
        first = np.maximum.accumulate(first, axis=1)
        ahead = np.take_along_axis(excl, first, axis=1)         # mass of strictly larger s
        k1d = np.take_along_axis(k1, order, axis=1)
        kept_d = k1d & (ahead < top_p * W[:, None])
        last_kept = V - 1 - np.argmax(kept_d[:, ::-1], axis=1)
        v_p = sd[np.arange(B), last_kept].astype(np.float32)
        keep = k1 & (s >= v_p[:, None])
        gap = np.where(k1d & (first == np.arange(V)[None, :]), np.abs(ahead - top_p * W[:, None]) / W[:, None], np.inf)
        margin = gap.min(axis=1)
    wk = np.where(keep, w, 0.0)
    cum = np.cumsum(wk, axis=1)
    W2 = cum[:, -1]
    thr = np.asarray(u, np.float64) * W2
    hit = keep & (cum > thr[:, None])
    any_hit = hit.any(axis=1)
    last = V - 1 - np.argmax(keep[:, ::-1], axis=1)
    ids = np.where(any_hit, np.argmax(hit, axis=1), last)
    stats = np.stack([t_k.astype(np.float64), v_p.astype(np.float64), keep.sum(axis=1).astype(np.float64), W2], axis=1)
    return ids, stats, keep, margin, cum


def draw_acceptable(gid, keep, cum, u, tol=1e-5):
    """id gid is an acceptable draw of one row: kept, and u * W2 lies within tol * W2 of gid's interval of the running mass"""
    if gid < 0 or gid >= keep.shape[0] or not keep[gid]:
        return False
    W2 = cum[-1]
    thr = u * W2
    hi = cum[gid]
    lo = cum[gid - 1] if gid > 0 else 0.0
    return lo - tol * W2 <= thr < hi + tol * W2 or (thr >= W2 - tol * W2 and gid == np.flatnonzero(keep)[-1])
