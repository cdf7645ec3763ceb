"""Float64 restatement of rejection verification ("Rejection verification") on top of sample_ref.sample_ref: the
contract lia_lm_verify_reject and the rejection loop are tested against.

Per block row b with g generated tokens, block [pending | d_1 .. d_k], T = k + 1, step s = g + t:
  P_t = the filtered distribution (sample_ref's kept set, weights over the kept mass) of the target's logits behind position t,
  Q_t = the same pipeline on the drafter's logits of draft step t; the suppressed token counts as -inf in both where t < n_suppress
  x = d_{t+1};  ok[t] = Q_t(x) > 0 and U_acc[s] * Q_t(x) < P_t(x);  a position with s >= n_steps is rejected (u = 0, nothing read)
  r = max(P_t - Q_t, 0), R = sum r;  token[t] = R > 0: the smallest id whose running r in id order exceeds U_res[s] * R, else the last
  id with r > 0;  R == 0 or t == T - 1: sample_ref's draw of P_t with U_res[s]
  accepted[b] = the first t with ok[t] == 0 (T - 1 where inactive), common = min, next[b] = accepted[b] > common ? d_{common+1} :
  token[b, common]
"""
import collections

import numpy as np

from sample_ref import sample_ref

Filtered = collections.namedtuple("Filtered", "prob keep margin cum")
RejectRef = collections.namedtuple("RejectRef", "token ok p_tok q_tok resid r rcum plain margin u_acc u_res inside draws")


def filtered(logits_f32, tau, top_k, top_p, suppress=-1):
    """rows [N, V] -> Filtered: prob [N, V] float64 (0 outside the kept set), keep, the top-p margin per row, the running kept mass"""
    logits_f32 = np.asarray(logits_f32, np.float32)
    _, _, keep, margin, cum = sample_ref(logits_f32, tau, top_k, top_p, np.zeros(logits_f32.shape[0]), suppress)
    w = np.diff(cum, axis=1, prepend=0.0)
    return Filtered(np.where(keep, w / cum[:, -1:], 0.0), keep, margin, cum)


def plain_draw(f, u):
    """sample_ref's draw rule on a Filtered (one id per row)"""
    thr = np.asarray(u, np.float64) * f.cum[:, -1]
    hit = f.keep & (f.cum > thr[:, None])
    V = f.keep.shape[1]
    last = V - 1 - np.argmax(f.keep[:, ::-1], axis=1)
    return np.where(hit.any(axis=1), np.argmax(hit, axis=1), last)


def residual_draw(r, u):
    """(id, running residual mass) of one row: the smallest id with r > 0 whose running mass exceeds u * R, else the last id with
    r > 0; -1 where R == 0"""
    rc = np.cumsum(r)
    if not rc[-1] > 0:
        return -1, rc
    hit = (r > 0) & (rc > np.float64(u) * rc[-1])
    return int(np.argmax(hit)) if hit.any() else int(np.flatnonzero(r > 0)[-1]), rc


def table(U, step0, B, T):
    """(u [B, T], inside [B, T]): U[step0 + t, b], 0 past the table"""
    U = np.asarray(U, np.float32)
    s = step0 + np.arange(T)
    inside = np.broadcast_to(((s >= 0) & (s < U.shape[0]))[None, :], (B, T))
    u = U[np.clip(s, 0, U.shape[0] - 1)][:, :B].T
    return np.where(inside, u, np.float32(0)).astype(np.float32), inside


def positions(p_logits, q_logits, block_ids, tau, top_k, top_p, U_acc, U_res, step0, suppress=-1, n_suppress=0):
    """every block position of p_logits [B, T, V] / q_logits [B, T - 1, V] / block_ids [B, T] -> RejectRef.  margin [B, T]: the
    smaller top-p margin of the two rows; plain [B, T]: the token is P_t's plain draw (t = T - 1 or R == 0)"""
    p_logits, q_logits = np.asarray(p_logits, np.float32), np.asarray(q_logits, np.float32)
    block_ids = np.asarray(block_ids, np.int64)
    B, T, V = p_logits.shape
    ua, inside = table(U_acc, step0, B, T)
    ur, _ = table(U_res, step0, B, T)
    out = RejectRef(np.zeros((B, T), np.int64), np.zeros((B, T), np.int32), np.zeros((B, T)), np.zeros((B, T)), np.zeros((B, T)),
                    np.zeros((B, T, V)), np.zeros((B, T, V)), np.zeros((B, T), bool), np.zeros((B, T)), ua, ur, inside, [])
    rows = np.arange(B)
    for t in range(T):
        sup = suppress if t < n_suppress else -1
        fp = filtered(p_logits[:, t], tau, top_k, top_p, sup)
        out.draws.append(fp)
        plain = plain_draw(fp, ur[:, t])
        out.margin[:, t] = fp.margin
        if t == T - 1:
            out.token[:, t], out.plain[:, t] = plain, True
            continue
        fq = filtered(q_logits[:, t], tau, top_k, top_p, sup)
        out.margin[:, t] = np.minimum(fp.margin, fq.margin)
        x = block_ids[:, t + 1]
        valid = (x >= 0) & (x < V)
        xs = np.where(valid, x, 0)
        out.p_tok[:, t] = np.where(valid, fp.prob[rows, xs], 0.0)
        out.q_tok[:, t] = np.where(valid, fq.prob[rows, xs], 0.0)
        out.ok[:, t] = inside[:, t] & (out.q_tok[:, t] > 0) & (ua[:, t].astype(np.float64) * out.q_tok[:, t] < out.p_tok[:, t])
        r = np.maximum(fp.prob - fq.prob, 0.0)
        out.r[:, t] = r
        for b in range(B):
            tok, rc = residual_draw(r[b], ur[b, t])
            out.rcum[b, t], out.resid[b, t] = rc, rc[-1]
            out.plain[b, t] = tok < 0
            out.token[b, t] = plain[b] if tok < 0 else tok
    return out


def accept(block_ids, token, ok, active=None):
    """(accepted [B], common, next [B]) from the per-position outputs"""
    block_ids, token, ok = np.asarray(block_ids), np.asarray(token), np.asarray(ok)
    B, T = block_ids.shape
    acc = np.zeros(B, np.int32)
    for b in range(B):
        a = T - 1
        if active is None or active[b]:
            a = 0
            while a < T - 1 and ok[b, a]:
                a += 1
        acc[b] = a
    common = int(acc.min())
    nxt = np.where(acc > common, block_ids[:, min(common + 1, T - 1)], token[:, common])
    return acc, common, nxt


def emit(p_logits, q_logits, settings, u_draft, u_acc, u_res):
    """One row's round from its uniforms alone.  p_logits(prefix_tokens) -> the target's logits [V] behind the pending token and the
    draft tokens so far, q_logits(prefix_tokens) -> the drafter's; or arrays [T, V] / [k, V] for logits that do not depend on the
    tokens.  settings = (tau, top_k, top_p) or (tau, top_k, top_p, suppress, n_suppress).  u_draft / u_acc: [k], u_res: [k + 1].
    -> (emitted ids: the accepted draft tokens then the residual or bonus draw, the draft tokens, the number accepted)"""
    tau, top_k, top_p = settings[:3]
    suppress, n_suppress = settings[3:] if len(settings) > 3 else (-1, 0)
    k = len(u_draft)
    pl = p_logits if callable(p_logits) else (lambda toks: np.asarray(p_logits)[len(toks)])
    ql = q_logits if callable(q_logits) else (lambda toks: np.asarray(q_logits)[len(toks)])
    drafts, out = [], []
    for t in range(k + 1):
        sup = suppress if t < n_suppress else -1
        fp = filtered(np.asarray(pl(drafts), np.float32)[None], tau, top_k, top_p, sup)
        if t == k:
            out.append(int(plain_draw(fp, [u_res[t]])[0]))              # the bonus token
            break
        fq = filtered(np.asarray(ql(drafts), np.float32)[None], tau, top_k, top_p, sup)
        x = int(plain_draw(fq, [u_draft[t]])[0])                         # the drafter's draw from Q_t
        drafts.append(x)
        p_x, q_x = fp.prob[0, x], fq.prob[0, x]
        if q_x > 0 and np.float64(u_acc[t]) * q_x < p_x:
            out.append(x)
            continue
        tok, _ = residual_draw(np.maximum(fp.prob[0] - fq.prob[0], 0.0), u_res[t])
        out.append(int(plain_draw(fp, [u_res[t]])[0]) if tok < 0 else tok)
        break
    return out, drafts, len(out) - 1


def chi2_sf(x, df):
    """P(chi-square with df degrees of freedom > x): the regularised upper incomplete gamma function Q(df / 2, x / 2), by its series
    below a + 1 and Lentz's continued fraction above"""
    import math
    a, x = df / 2.0, x / 2.0
    if x <= 0:
        return 1.0
    lead = math.exp(-x + a * math.log(x) - math.lgamma(a))
    if x < a + 1:
        term = total = 1.0 / a
        n = a
        while abs(term) > abs(total) * 1e-16:
            n += 1
            term *= x / n
            total += term
        return 1.0 - lead * total
    tiny = 1e-300
    b = x + 1 - a
    c, d = 1 / tiny, 1 / b
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1 / d
        delta = d * c
        h *= delta
        if abs(delta - 1) < 1e-16:
            break
    return lead * h


def chi2_quantile(df, tail):
    """x with chi2_sf(x, df) == tail, by bisection"""
    lo, hi = 0.0, df + 100.0 * (df ** 0.5 + 10)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if chi2_sf(mid, df) > tail else (lo, mid)
    return 0.5 * (lo + hi)


def chi_square(tokens, prob, min_expected=5.0):
    """(statistic, degrees of freedom) of the counts of `tokens` against the distribution prob [V]; bins whose expectation is below
    min_expected are pooled into one (dropped where even the pool expects nothing)"""
    tokens, prob = np.asarray(tokens, np.int64), np.asarray(prob, np.float64)
    n = tokens.size
    counts = np.bincount(tokens, minlength=prob.size).astype(np.float64)
    exp = n * prob
    big = exp >= min_expected
    obs_b, exp_b = list(counts[big]), list(exp[big])
    if (~big).any() and exp[~big].sum() > 0:
        obs_b.append(counts[~big].sum())
        exp_b.append(exp[~big].sum())
    elif (~big).any():
        assert counts[~big].sum() == 0, "a token of probability 0 was emitted"
    obs_b, exp_b = np.asarray(obs_b), np.asarray(exp_b)
    return float(((obs_b - exp_b) ** 2 / exp_b).sum()), len(exp_b) - 1
