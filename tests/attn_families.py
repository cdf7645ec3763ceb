"""Attention inputs where kernels go wrong: an attention sink, scores in the hundreds, one-hot rows, a running maximum that moves
in every key tile, `exp` underflowing for most keys, p = 1 / n.  NumPy only, deterministic, no GPU.

Each family function returns bf16 bit patterns (q [B, T, heads * d], kc, vc [S + SLACK, Bc, kv_heads, d]) laid out as the kernel
tests lay them out: served rows b0 .. b0 + B - 1 of the Bc cache batch rows, T query rows per batch row at positions
S - T .. S - 1.  With `starts` (left padding) served row b's sequence begins at cache position starts[b]: the family is built on
the SHIFTED sequence (key i of the row sits at starts[b] + i), so a padded case is the unpadded case of S - starts[b] tokens.

Exact families: every q entry is 0 or +-2^k and every K entry a small integer, so every product and every partial sum of a score
is an integer multiple of one power of two below 2^24 of it -- exact in fp32 in ANY order, for both scalings (q * d^-0.5 of a
power of two rounds to the same bf16 however d^-0.5 was formed).  A legitimate difference of summation order then cannot move
a score by a bf16 quantum (e^0.5 of a probability at |s| ~ 100).  tests/test_attn_families.py checks these rules on the reference.

    exact    q in {0, +-1, +-2, +-4}, K integers in [-7, 7], V ~ N(0, 1): the baseline, |s| to ~40
    ramp     K row i = w * m_i, m_i a sawtooth 1 .. 100 that ends at 100 on the newest key, w the Walsh sign pattern of the key's period; q = a w of the
             query's own period, so keys of other periods score exactly 0 and the scores rise by ~4 .. 6 per key up to the
             newest: the maximum moves in every tile, the newest key holds ~0.98, |s| to 400 .. 566
    fall     K row i = u * max(100 - i, 1): the maximum is met by the first key, exp underflows from ~20 keys on
    sink     K row 0 = +63 u, every other row -u, q = a * u with a in {0, 1, 2, 4} (>= 8 non-zero per head), |V| in [2^-4, 8):
             gap >= 40, every row is one-hot in bf16 and the output IS the sink's V row
    uniform  every K row equal, every V row equal: p = bf16(1 / n) for n = 1 .. T
    hot      Gaussian data with q scaled by 8 (NOT exact): ordinary data at |s| ~ 100

Poison, where the kernels' contract says nothing is read: cache rows >= S and cache batch rows outside b0 .. b0 + B - 1 hold NaN
in K and V; pad positions 0 .. starts[b] - 1 hold a K row that would score above every real key of every query, and NaN in V.
Every operand a kernel is meant to read is finite, and so is every score.
"""
import numpy as np

import f64_ref as R

FAMILIES = ("exact", "ramp", "fall", "sink", "uniform", "hot")
EXACT_FAMILIES = ("exact", "ramp", "fall", "sink", "uniform")
NAN = 0x7fc0
SLACK = 3                   # cache rows behind S
PERIOD = 100                # ramp's sawtooth
SINK_C = 63                 # the sink key is +SINK_C u, the others -u
SINK_MIN_GAP = 40.0
PAD_BIG = 2.0 ** 15         # the pad K row's one entry (dimension 0, where every q is > 0 in sign-pattern terms)
RAMP_AMP = {32: 1.0, 64: 0.5, 128: 0.5}     # |q| entries of ramp / fall: sum |q| * d^-0.5 = 5.66, 4, 5.66 per step of m

# (mutant of f64_ref.attention, family) pairs the comparison rejects; tests/test_attn_families.py proves each on the reference
# and prints the margin of every (mutant, family), tests/test_gpu_attention_families.py turns each against the kernels' outputs.
# At d = 64 the scale 2^-3 is exact, so "round_qk=False" and "other scaling" ARE the right reference there: those pairs are
# taken at d 32 / 128.  With one query row (decode) a mask shifted by +1 shows no key there is.
MUTANTS = {
    "mask_shift=+1": dict(mask_shift=1),
    "mask_shift=-1": dict(mask_shift=-1),
    "round_p=False": dict(round_p=False),
    "round_qk=False": dict(round_qk=False),
    "other scaling": dict(other_scaling=True),
    "kh = hh % kv_heads": dict(kh_mod=True),
}
MUTANT_PAIRS = (("mask_shift=+1", "ramp"), ("mask_shift=-1", "ramp"), ("round_p=False", "exact"), ("round_qk=False", "hot"),
                ("other scaling", "hot"), ("kh = hh % kv_heads", "sink"))
DECODE_MUTANT_PAIRS = tuple(p for p in MUTANT_PAIRS if p[0] != "mask_shift=+1")


def _bf(x):
    return R.bits(R.rnd(x))


def _walsh(d):
    h = np.ones((1, 1))
    while h.shape[0] < d:
        h = np.block([[h, h], [h, -h]])
    return h                                            # rows orthogonal, column 0 all +1


def _rs(seed, fam, b):
    return np.random.RandomState([seed, FAMILIES.index(fam), b])


# ---- one served row: (q [Tq, heads, d], K [n, kv_heads, d], V [n, kv_heads, d], pad K row [kv_heads, d]) as float64 ------------
# n keys, the Tq queries at sequence positions n - Tq .. n - 1
def _pad_e0(kvh, d, sign=1.0):
    p = np.zeros((kvh, d))
    p[:, 0] = sign * PAD_BIG
    return p


def _q_exact(rs, Tq, heads, d):
    q = rs.choice(np.array([0.0, 1, -1, 2, -2, 4, -4]), size=(Tq, heads, d))
    q[..., 0] = 4.0                                     # the pad K row's dimension
    return q


def _row_exact(rs, n, Tq, heads, kvh, d):
    return (_q_exact(rs, Tq, heads, d), rs.randint(-7, 8, size=(n, kvh, d)).astype(np.float64), rs.standard_normal((n, kvh, d)),
            _pad_e0(kvh, d))


def _row_hot(rs, n, Tq, heads, kvh, d):
    q = 8 * 1.5 * rs.standard_normal((Tq, heads, d))
    q[..., 0] = np.abs(q[..., 0]) + 8.0
    return q, 1.5 * rs.standard_normal((n, kvh, d)), rs.standard_normal((n, kvh, d)), _pad_e0(kvh, d)


def _row_uniform(rs, n, Tq, heads, kvh, d):
    k0, v0 = rs.randint(-7, 8, size=(1, kvh, d)).astype(np.float64), rs.standard_normal((1, kvh, d))
    return _q_exact(rs, Tq, heads, d), np.repeat(k0, n, axis=0), np.repeat(v0, n, axis=0), _pad_e0(kvh, d)


def _row_sink(rs, n, Tq, heads, kvh, d):
    u = rs.choice(np.array([-1.0, 1.0]), size=(kvh, d))
    a = rs.choice(np.array([0.0, 0, 0, 1, 2, 4]), size=(Tq, heads, d))
    for t in range(Tq):                                 # at least 8 non-zero entries per head
        for h in range(heads):
            a[t, h, rs.permutation(d)[:8]] = rs.choice(np.array([1.0, 2, 4]), size=8)
    G = heads // kvh
    q = a * u[np.arange(heads) // G][None]
    k = np.repeat(-u[None], n, axis=0)
    k[0] = SINK_C * u
    v = rs.choice(np.array([-1.0, 1.0]), size=(n, kvh, d)) * 2.0 ** rs.uniform(-4, 3, size=(n, kvh, d))
    v = np.clip(np.abs(R.rnd(v)), 2.0 ** -4, 7.96875) * np.sign(v)
    return q, k, v, 4 * SINK_C * u


def _row_ramp(rs, n, Tq, heads, kvh, d):
    w = _walsh(d)
    G = heads // kvh
    i = np.arange(n) + (PERIOD - n % PERIOD) % PERIOD          # the sawtooth ends at its top on the newest key
    pat = (i[:, None] // PERIOD + 5 * np.arange(kvh)[None, :]) % d                      # [n, kvh]: pattern of key i, head kh
    k = w[pat] * (1 + i % PERIOD)[:, None, None]
    qpat = pat[n - Tq:][:, np.arange(heads) // G]                                       # [Tq, heads]
    return RAMP_AMP[d] * w[qpat], k, rs.standard_normal((n, kvh, d)), _pad_e0(kvh, d)


def _row_fall(rs, n, Tq, heads, kvh, d):
    u = rs.choice(np.array([-1.0, 1.0]), size=(kvh, d))
    G = heads // kvh
    k = u[None] * np.maximum(PERIOD - np.arange(n), 1)[:, None, None]
    q = np.repeat((RAMP_AMP[d] * u[np.arange(heads) // G])[None], Tq, axis=0)
    pad = np.zeros((kvh, d))
    pad[:, 0] = u[:, 0] * PAD_BIG
    return q, k, rs.standard_normal((n, kvh, d)), pad


_ROWS = dict(exact=_row_exact, ramp=_row_ramp, fall=_row_fall, sink=_row_sink, uniform=_row_uniform, hot=_row_hot)


def make(family, B, T, S, heads, kv_heads, d, post_scale, starts=None, Bc=None, b0=0, seed=0):
    """the case of `family`: (q, kc, vc) as bf16 bit patterns, poisoned as the module docstring says.  post_scale does not change
    the inputs (every family is exact under both scalings); it is taken so that a case is named by the launcher's arguments."""
    Bc = B + b0 if Bc is None else Bc
    st = np.zeros(B, np.int64) if starts is None else np.asarray(starts, np.int64)
    assert T <= S and (st <= S - 1).all() and (st >= 0).all() and b0 + B <= Bc
    q = np.full((B, T, heads, d), 0x3f80, np.uint16)                # pad query rows: 1.0 (their output rows are zeros)
    kc = np.full((S + SLACK, Bc, kv_heads, d), NAN, np.uint16)
    vc = np.full((S + SLACK, Bc, kv_heads, d), NAN, np.uint16)
    for b in range(B):
        s = int(st[b])
        n = S - s
        Tq = min(T, n)
        qb, kb, vb, pad = _ROWS[family](_rs(seed, family, b), n, Tq, heads, kv_heads, d)
        q[b, T - Tq:] = _bf(qb)
        kc[s:S, b0 + b] = _bf(kb)
        vc[s:S, b0 + b] = _bf(vb)
        kc[:s, b0 + b] = _bf(pad)[None]                             # (V at the pad positions stays NaN)
    return q.reshape(B, T, heads * d), kc, vc


def exact(B, T, S, heads, kv_heads, d, post_scale, **kw):
    return make("exact", B, T, S, heads, kv_heads, d, post_scale, **kw)


def ramp(B, T, S, heads, kv_heads, d, post_scale, **kw):
    return make("ramp", B, T, S, heads, kv_heads, d, post_scale, **kw)


def fall(B, T, S, heads, kv_heads, d, post_scale, **kw):
    return make("fall", B, T, S, heads, kv_heads, d, post_scale, **kw)


def sink(B, T, S, heads, kv_heads, d, post_scale, **kw):
    return make("sink", B, T, S, heads, kv_heads, d, post_scale, **kw)


def uniform(B, T, S, heads, kv_heads, d, post_scale, **kw):
    return make("uniform", B, T, S, heads, kv_heads, d, post_scale, **kw)


def hot(B, T, S, heads, kv_heads, d, post_scale, **kw):
    return make("hot", B, T, S, heads, kv_heads, d, post_scale, **kw)


# ---- what the tests ask of a case ----------------------------------------------------------------------------------------------
def real_rows(B, T, S, starts=None):
    """[B, T] bool: query rows at or behind their row's start (the others are pad rows: zeros in the output)"""
    st = np.zeros(B, np.int64) if starts is None else np.asarray(starts, np.int64)
    return (S - T + np.arange(T))[None, :] >= st[:, None]


def rows(q, kc, vc, S, starts=None, b0=0):
    """per served row b: (b, s, q rows [1, Tq, H] of the real queries, K, V [n + ..., 1, kv_heads, d] from the row's start on):
    the row's own unpadded case (S - s keys, batch row 0 of a cache of one)"""
    B, T, _ = q.shape
    st = np.zeros(B, np.int64) if starts is None else np.asarray(starts, np.int64)
    for b in range(B):
        s = int(st[b])
        Tq = min(T, S - s)
        yield b, s, q[b:b + 1, T - Tq:], kc[s:, b0 + b:b0 + b + 1], vc[s:, b0 + b:b0 + b + 1]


def reference(q, kc, vc, S, heads, kv_heads, post_scale, b0=0, starts=None, other_scaling=False, kh_mod=False, **mutant):
    """f64_ref.attention of the case; with `starts` each served row's own shifted sequence (the kernels' documented frame), pad
    query rows zeros.  other_scaling / kh_mod / the keywords of f64_ref.attention: the mutants of MUTANTS."""
    ps = (1 - post_scale) if other_scaling else post_scale
    if kh_mod:
        mutant["kv_head_of"] = lambda hh: hh % kv_heads
    if starts is None:
        return R.attention(q, kc, vc, S, heads, kv_heads, ps, b0=b0, **mutant)
    out = np.zeros(q.shape, np.uint16)
    for b, s, qb, kb, vb in rows(q, kc, vc, S, starts, b0):
        out[b, q.shape[1] - qb.shape[1]:] = R.attention(qb, kb, vb, S - s, heads, kv_heads, ps, **mutant)[0]
    return out


def sink_rows(q, vc, S, heads, kv_heads, b0=0, starts=None):
    """what a sink case's output must be, bit for bit: the V row of the first visible key under every head; pad rows zeros"""
    B, T, H = q.shape
    d = H // heads
    st = np.zeros(B, np.int64) if starts is None else np.asarray(starts, np.int64)
    kh = np.arange(heads) // (heads // kv_heads)
    out = np.zeros((B, T, heads, d), np.uint16)
    real = real_rows(B, T, S, st)
    for b in range(B):
        out[b, real[b]] = vc[st[b], b0 + b][kh][None]
    return out.reshape(B, T, H)


def scores64(q, kc, S, heads, kv_heads, post_scale, b0=0, starts=None):
    """the reference's rounded scores in float64, per served row: list of [heads, Tq, n] (all keys of the row, no causal mask)"""
    out = []
    for b, s, qb, kb, _ in rows(q, kc, kc, S, starts, b0):
        d = kb.shape[-1]
        G = heads // kv_heads
        qf = R.f64(qb[0]).reshape(-1, heads, d).transpose(1, 0, 2)
        kf = R.f64(kb[:S - s, 0]).transpose(1, 0, 2)[np.arange(heads) // G]
        if post_scale:
            out.append(R.rnd(R.rnd(qf @ kf.transpose(0, 2, 1)) * d ** -0.5))
        else:
            out.append(R.rnd(R.rnd(qf * d ** -0.5) @ kf.transpose(0, 2, 1)))
    return out


def order_slack(q, kc, vc, S, heads, kv_heads, post_scale, b0=0, starts=None):
    """`hot` only (the one family whose q . k is NOT exact in fp32): how far the output of a correct fp32 kernel may lie from
    reference() because of the ORDER of its q . k sum alone.  [B, T, H] float64, zero where no score is affected.

    The products of two bf16 are exact in fp32; a sum of d of them in any order lies within delta = d 2^-24 sum |q_i k_i| of the
    exact value, so the kernel's rounded score lies in [lo, hi] = the reference's rounding chain at acc -/+ delta (monotone), and
    so does the reference's.  Where lo != hi the fp32 sum sits next to a bf16 tie and either neighbour is a correct score: at
    |s| ~ 100 that is e^0.5 of a probability.  With eps = sum_j p_j (e^(hi_j - lo_j) - 1) over the visible keys, the softmax
    moves by at most 2 eps / (1 - eps) in l1, the output by at most eps / (1 - eps) (max_j v_j - min_j v_j) per dimension."""
    B, T, H = q.shape
    d, G = H // heads, heads // kv_heads
    scale = d ** -0.5
    out = np.zeros((B, T, heads, d))
    for b, s, qb, kb, vb in rows(q, kc, vc, S, starts, b0):
        n, Tq = S - s, qb.shape[1]
        pos = n - Tq + np.arange(Tq)
        vis = np.arange(n)[None, :] <= pos[:, None]
        for hh in range(heads):
            qf, kf, vf = R.f64(qb[0]).reshape(Tq, heads, d)[:, hh], R.f64(kb[:n, 0, hh // G]), R.f64(vb[:n, 0, hh // G])
            qs = qf if post_scale else R.rnd(qf * scale)
            acc, delta = qs @ kf.T, d * 2.0 ** -24 * (np.abs(qs) @ np.abs(kf).T)
            chain = (lambda a: R.rnd(R.rnd(a) * scale)) if post_scale else R.rnd
            lo, hi, sc = chain(acc - delta), chain(acc + delta), np.where(vis, chain(acc), -np.inf)
            e = np.exp(sc - sc.max(axis=1, keepdims=True))
            eps = ((e / e.sum(axis=1, keepdims=True)) * np.where(vis, np.expm1(hi - lo), 0.0)).sum(axis=1)
            spread = (np.maximum.accumulate(vf, axis=0) - np.minimum.accumulate(vf, axis=0))[pos]           # [Tq, d]
            out[b, T - Tq:, hh] = np.where(eps < 0.5, eps / (1 - np.minimum(eps, 0.5) + 1e-300), 1.0)[:, None] * spread
    return out.reshape(B, T, H)
