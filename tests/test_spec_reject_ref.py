"""The float64 reference of rejection verification (spec_reject_ref.py) is exact: for one draft token on a small vocabulary emit() is
piecewise constant on boxes of (u_draft, u_acc, u_res), so the distribution of its first emitted token is a finite sum of box volumes
-- which must be the target's filtered distribution P to rounding.  Box edges: Q's running mass (which token the drafter draws),
min(1, p / q) of that token (accepted below it), and -- in a rejected box only -- the residual's running mass.  Accepted boxes are
not split by residual intervals: with P = Q there is no residual at all and every box is an accepted one."""
import numpy as np
import pytest

import spec_reject_ref as R

V = 7


def _logits(seed, V=V, sigma=1.5):
    """bf16-representable fp32 logits"""
    x = (sigma * np.random.RandomState(seed).randn(V)).astype(np.float32)
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _intervals(edges):
    """[(lo, hi)] of the non-empty intervals between consecutive edges of a running mass normalised to [0, 1]"""
    e = np.concatenate([[0.0], np.asarray(edges, np.float64)])
    return [(lo, hi) for lo, hi in zip(e[:-1], e[1:]) if hi > lo]


def first_token_distribution(p, q, settings):
    """the distribution of emit()'s first token over uniform (u_draft, u_acc, u_res), by box midpoints weighted by volume"""
    tau, top_k, top_p = settings[:3]
    sup = settings[3] if len(settings) > 3 and settings[4] > 0 else -1
    fp = R.filtered(p[None], tau, top_k, top_p, sup)
    fq = R.filtered(q[None], tau, top_k, top_p, sup)
    P, Q = fp.prob[0], fq.prob[0]
    r = np.maximum(P - Q, 0.0)
    dist, volume = np.zeros(p.size), 0.0
    pl, ql = np.stack([p, p]), q[None]
    for lo_d, hi_d in _intervals(fq.cum[0] / fq.cum[0, -1]):
        ud = 0.5 * (lo_d + hi_d)
        d = int(R.plain_draw(fq, [ud])[0])
        a = min(1.0, P[d] / Q[d])
        boxes = [(0.0, a, 0.0, 1.0)] if a > 0 else []                         # accepted: one box, whatever u_res
        if a < 1:
            boxes += [(a, 1.0, lo, hi) for lo, hi in _intervals(np.cumsum(r) / r.sum())]
        for lo_a, hi_a, lo_r, hi_r in boxes:
            out, drafts, n_acc = R.emit(pl, ql, settings, [ud], [0.5 * (lo_a + hi_a)], [0.5 * (lo_r + hi_r), 0.5])
            assert drafts == [d] and n_acc == (1 if hi_a <= a else 0)
            vol = (hi_d - lo_d) * (hi_a - lo_a) * (hi_r - lo_r)
            dist[out[0]] += vol
            volume += vol
    return dist, volume, P, Q


def _disjoint():
    p = np.full(V, -8.0, np.float32)
    q = p.copy()
    p[[0, 2, 5]] = [1.0, 2.0, 1.5]
    q[[1, 3, 6]] = [2.0, 1.0, 1.5]
    return p, q, (1.0, 3, 1.0)


CASES = {
    "no filter": lambda: (_logits(1), _logits(2), (1.0, 0, 1.0)),
    "top-k 4": lambda: (_logits(3), _logits(4), (0.9, 4, 1.0)),
    "top-p 0.9": lambda: (_logits(5), _logits(6), (1.0, 0, 0.9)),
    "top-k 3 + top-p 0.9": lambda: (_logits(7), _logits(8), (1.2, 3, 0.9)),
    "one token kept in both (R = 0 or disjoint)": lambda: (_logits(9), _logits(9) + np.float32(0.5), (0.5, 0, 0.3)),
    "suppressed token": lambda: (_logits(11), _logits(12), (1.0, 0, 1.0, int(np.argmax(_logits(11))), 1)),
    "P = Q": lambda: (_logits(13), _logits(13), (0.8, 5, 0.95)),
    "disjoint kept sets": _disjoint,
}


@pytest.mark.parametrize("name", list(CASES))
def test_first_emitted_token_is_distributed_as_P(name):
    p, q, settings = CASES[name]()
    dist, volume, P, Q = first_token_distribution(p, q, settings)
    print(name, "max |dist - P| =", np.abs(dist - P).max(), "volume", volume, "accept", np.minimum(P, Q).sum())
    assert abs(volume - 1.0) <= 1e-12
    assert np.abs(dist - P).max() <= 1e-12
    if name == "P = Q":
        assert np.array_equal(P, Q)
    if name == "disjoint kept sets":
        assert np.minimum(P, Q).sum() == 0
    if name == "suppressed token":
        assert P[settings[3]] == 0 and Q[settings[3]] == 0 and dist[settings[3]] == 0


def test_R_zero_takes_the_plain_draw():
    p = _logits(21)
    for u in (0.0, 0.3, 0.999):
        # a rejected position with P = Q can only be a contract violation (a token Q gives no mass): the plain draw of P
        out, _, n = R.emit(np.stack([p, p]), p[None], (1.0, 3, 1.0), [0.2], [0.99999], [u, 0.5])
        assert n == 1                                                          # u_acc < 1 = p / q: accepted
        ref = R.positions(p[None, None].repeat(2, 1), p[None, None], [[0, int(np.argmin(p))]], 1.0, 3, 1.0, [[0.5]], [[u]], 0)
        assert ref.ok[0, 0] == 0 and ref.q_tok[0, 0] == 0 and ref.resid[0, 0] == 0 and ref.plain[0, 0]
        assert ref.token[0, 0] == R.plain_draw(R.filtered(p[None], 1.0, 3, 1.0), [u])[0]


def test_positions_agree_with_emit_and_accept():
    rs = np.random.RandomState(5)
    B, k, n = 4, 3, 6
    pl = np.stack([[_logits(100 + 10 * b + t) for t in range(k + 1)] for b in range(B)])
    ql = np.stack([[_logits(100 + 10 * b + t) + _logits(500 + 10 * b + t, sigma=0.5) for t in range(k)] for b in range(B)])
    ql = (ql.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    Ud, Ua, Ur = rs.rand(3, n, B).astype(np.float32)
    for g in (0, 2, 4):                                                        # g = 4: positions 2, 3 lie past the table
        s = np.clip(g + np.arange(k + 1), 0, n - 1)
        rows = [R.emit(pl[b], ql[b], (0.9, 5, 0.95), Ud[s[:k], b], Ua[s[:k], b], Ur[s, b]) for b in range(B)]
        block = np.array([[0] + d + [0] * (k - len(d)) for _, d, _ in rows])
        for b, (_, d, _) in enumerate(rows):                                   # the draft tokens behind a rejection: Q's draws too
            for t in range(len(d), k):
                block[b, t + 1] = R.plain_draw(R.filtered(ql[b, t][None], 0.9, 5, 0.95), [Ud[s[t], b]])[0]
        ref = R.positions(pl, ql, block, 0.9, 5, 0.95, Ua, Ur, g)
        acc, common, nxt = R.accept(block, ref.token, ref.ok)
        for b, (out, d, n_acc) in enumerate(rows):
            inside = n - g                                                     # positions with a table entry
            want = min(n_acc, inside) if n_acc >= inside else n_acc
            assert acc[b] == want, (g, b, acc[b], n_acc)
            if acc[b] == n_acc:
                assert ref.token[b, acc[b]] == out[-1]
            assert nxt[b] == (block[b, common + 1] if acc[b] > common else ref.token[b, common])
        assert (ref.ok[:, k] == 0).all() and (ref.ok[~ref.inside] == 0).all()


def test_chi_square_helpers():
    assert abs(R.chi2_quantile(41, 1e-6) - 99.1739375697) < 1e-6 and abs(R.chi2_quantile(3, 1e-6) - 30.6648497062) < 1e-6
    stat, df = R.chi_square(np.array([0, 0, 1, 1, 2, 2] * 5), np.array([1 / 3, 1 / 3, 1 / 3, 0.0]))
    assert stat == 0 and df == 2
