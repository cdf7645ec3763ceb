"""The attention input families of attn_families.py, on the CPU: the generator's rules (checked on the reference alone), that the
project's attention bounds can be met on them (an fp32 emulation of the kernels' two schemes), that the bounds reject every
reference mutant on a named family, and the host attention (lia_host_attention / _padded) against the oracle's CPU branch.
The GPU half is tests/test_gpu_attention_families.py."""
import numpy as np
import pytest

import attn_families as F
import f64_ref as R
import synth
from test_gpu_kernel_variants import ATTN_ATOL, ATTN_MIN_EXACT, ATTN_RTOL, verdict

ATTN = dict(min_exact=ATTN_MIN_EXACT, bound=(ATTN_ATOL, ATTN_RTOL))
LOG2E = np.float32(1.4426950408889634)


def family_verdict(family, got, ref, slack=None):
    """(ok, message) of the attention comparison.  Every family but `hot`: test_gpu_kernel_variants.verdict with the ATTN_* bounds.
    `hot` (q . k not exact in fp32): the same bit-identical fraction, and the same per-element bound -- one quantum of the largest
    output and ATTN_ATOL + ATTN_RTOL |ref| -- widened by attn_families.order_slack, what the order of a correct fp32 q . k sum
    alone can move the output by.  Why: a plain fp32 emulation summing q . k forward meets the float64 reference at 99.97-99.99 %
    bit-identical on hot, yet at (B 2, T 257, heads 8 / 2, d 64, post_scale 1) one of ~30 visible scores that round to the other
    bf16 neighbour carries weight and moves one row by 5.8 quanta -- in every summation order tried; the MI355X kernels return
    the emulation's figures to the digit (3.250 / 4.125 / 5.812 quanta on three prefill shapes).  The slack is zero on rows whose
    weighty scores are clear of a tie (median < 1e-15, mean 0.006-0.018)."""
    if family != "hot":
        return verdict(got, ref, **ATTN)
    a, b = R.f64(got), R.f64(ref)
    q = R.quantum(max(float(np.abs(b).max()), 2.0 ** -126))
    err = np.abs(a - b)
    err = np.where(np.isnan(err), np.inf, err)
    plain = np.minimum(q, ATTN_ATOL + ATTN_RTOL * np.abs(b))
    frac = float((got == ref).mean())
    over = err > plain
    worst = float((err / (plain + slack)).max())
    msg = (f"{100 * frac:.3f} % bit-identical, max |err| {float(err.max()):.3g} = {float(err.max()) / q:.3f} quanta of max |ref|, "
           f"{int(over.sum())} outputs beyond the plain bound, worst err / (bound + order slack) {worst:.3f}")
    return bool(frac >= ATTN_MIN_EXACT and worst <= 1.0), msg


def rb(x):
    """fp32 -> the nearest bf16 value, as fp32"""
    return synth.bf16_bits_to_f32(synth.f32_to_bf16_bits(np.asarray(x, np.float32)))


def f32(b):
    return synth.bf16_bits_to_f32(b)


# ---- 1. exactness --------------------------------------------------------------------------------------------------------------
ORDERS = ("forward", "reversed", "mfma16", "mfma32", "random")


def dot32(qv, kv, order):
    """q [Tq, d] . k [n, d]^T with every product and every sum formed in fp32, the d products taken in `order`"""
    d = qv.shape[1]
    idx = np.arange(d)
    if order == "reversed":
        idx = idx[::-1]
    elif order == "random":
        idx = np.random.RandomState(d).permutation(d)
    width = {"mfma16": 16, "mfma32": 32}.get(order, d)
    acc = np.zeros((qv.shape[0], kv.shape[0]), np.float32)
    for c0 in range(0, d, width):                    # an MFMA sums one k-slice, then adds it to the accumulator
        part = np.zeros_like(acc)
        for i in idx[c0:c0 + width]:
            part = part + qv[:, i, None] * kv[None, :, i]
        acc = acc + part
    return acc


def scores32(qv, kv, ps, order):
    d = qv.shape[1]
    scale = np.float32(float(d) ** -0.5)             # the launchers' float scaling
    if ps:
        return rb(rb(dot32(qv, kv, order)) * scale)
    return rb(dot32(rb(qv * scale), kv, order))


@pytest.mark.parametrize("ps", (0, 1))
@pytest.mark.parametrize("d", (32, 64, 128))
@pytest.mark.parametrize("family", F.EXACT_FAMILIES)
def test_scores_are_exact_in_fp32_in_any_order(family, d, ps):
    """Every exact family, d 32 / 64 / 128, both scalings, unpadded and with starts: the scores formed in fp32 in five orders of
    the d products equal the reference's float64 scores bit for bit after the reference's rounding points -- no score excluded."""
    B, T, heads, kvh = 3, 257, 2, 1
    for starts in (None, [0, 65, 200]):
        q, kc, vc = F.make(family, B, T, T, heads, kvh, d, ps, starts=starts, b0=1, Bc=B + 2)
        want = F.scores64(q, kc, T, heads, kvh, ps, b0=1, starts=starts)
        for (b, s, qb, kb, _), w in zip(F.rows(q, kc, vc, T, starts, 1), want):
            assert np.isfinite(w).all()
            for hh in range(heads):
                qv, kv = f32(qb[0]).reshape(-1, heads, d)[:, hh], f32(kb[:T - s, 0, hh // (heads // kvh)])
                for order in ORDERS:
                    got = scores32(qv, kv, ps, order)
                    bad = synth.f32_to_bf16_bits(got) != R.bits(w[hh])
                    assert not bad.any(), f"{family} d {d} ps {ps} row {b} head {hh} {order}: {bad.sum()} scores differ"


# ---- 2. the family conditions ----------------------------------------------------------------------------------------------------
CONDITION_SHAPES = [(2, 257, 257, 4, 2, 128, None), (2, 129, 129, 2, 2, 64, None), (3, 257, 257, 2, 1, 32, [0, 64, 255]),
                    (2, 1, 1037, 8, 2, 128, None), (3, 1, 1037, 2, 2, 64, [1, 128, 1036])]


def probabilities(q, kc, vc, S, heads, kvh, ps, b0, starts):
    """per served row: (scores [heads, Tq, n] with -inf above the diagonal, float64 softmax of them)"""
    for (b, s, qb, _, _), sc in zip(F.rows(q, kc, vc, S, starts, b0), F.scores64(q, kc, S, heads, kvh, ps, b0, starts)):
        n, Tq = S - s, qb.shape[1]
        vis = np.arange(n)[None, :] <= (n - Tq + np.arange(Tq))[:, None]
        sc = np.where(vis[None], sc, -np.inf)
        e = np.exp(sc - sc.max(axis=-1, keepdims=True))
        yield b, s, sc, e / e.sum(axis=-1, keepdims=True), vis


@pytest.mark.parametrize("ps", (0, 1))
@pytest.mark.parametrize("B,T,S,heads,kvh,d,starts", CONDITION_SHAPES)
@pytest.mark.parametrize("family", F.FAMILIES)
def test_family_conditions(family, B, T, S, heads, kvh, d, starts, ps):
    """What each family promises, on the reference: the poison sits where nothing is read and everything read is finite; pad K rows
    score above every real key; sink: >= 8 non-zero q entries per head and a gap >= 40 on EVERY row; ramp: the newest key holds
    >= 0.9 on >= 90 % of the rows with two or more keys; |s| reaches 300 (ramp, fall) / 50 (hot)."""
    b0, Bc = 1, B + 2
    q, kc, vc = F.make(family, B, T, S, heads, kvh, d, ps, starts=starts, b0=b0, Bc=Bc)
    st = np.zeros(B, int) if starts is None else np.asarray(starts)
    assert q.shape == (B, T, heads * d) and kc.shape == vc.shape == (S + F.SLACK, Bc, kvh, d)
    assert np.isfinite(R.f64(q)).all()
    for c in (kc, vc):
        assert (c[S:] == F.NAN).all() and (c[:, :b0] == F.NAN).all() and (c[:, b0 + B:] == F.NAN).all()
    for b in range(B):
        assert np.isfinite(R.f64(kc[:S, b0 + b])).all() and np.isfinite(R.f64(vc[st[b]:S, b0 + b])).all()
        assert (vc[:st[b], b0 + b] == F.NAN).all()
    top, newest, rows2 = 0.0, 0, 0
    scale = d ** -0.5
    for b, s, sc, p, vis in probabilities(q, kc, vc, S, heads, kvh, ps, b0, starts):
        seen = sc[np.isfinite(sc)]
        assert np.isfinite(sc.max(axis=-1)).all() and np.abs(seen).max() < 3.0e38
        top = max(top, float(np.abs(seen).max()))
        Tq = sc.shape[1]
        if s:                                        # the pad K row against every real query: above every real key's score
            qf = R.f64(q[b, T - Tq:]).reshape(Tq, heads, d).transpose(1, 0, 2)
            kp = R.f64(kc[0, b0 + b])[np.arange(heads) // (heads // kvh)][:, None, :]
            ps_ = R.rnd(R.rnd((qf * kp).sum(-1)) * scale) if ps else R.rnd((R.rnd(qf * scale) * kp).sum(-1))
            assert (ps_ > sc.max(axis=-1)).all(), f"{family}: a pad K row does not outscore the real keys of row {b}"
        if family == "sink":
            nz = (R.f64(q[b, T - Tq:]).reshape(Tq, heads, d) != 0).sum(-1)
            assert nz.min() >= 8
            last = np.where(vis[None] & (np.arange(sc.shape[2]) > 0)[None, None, :], sc, -np.inf).max(axis=-1)
            gap = sc[:, :, 0] - last                 # (inf where the sink is the only key)
            assert gap.min() >= F.SINK_MIN_GAP, f"sink gap {gap.min()} on row {b}"
        if family == "ramp":
            pos = sc.shape[2] - Tq + np.arange(Tq)
            pn = p[:, np.arange(Tq), pos]
            two = pos >= 1
            newest += int((pn[:, two] >= 0.9).sum())
            rows2 += int(two.sum()) * heads
    print(f"\n{family} d {d} ps {ps}: max |s| {top:.4g}" + (f", newest key >= 0.9 on {newest} of {rows2} rows" if rows2 else ""))
    if family == "ramp":
        assert newest >= 0.9 * rows2
    if family in ("ramp", "fall"):
        assert top >= 300
    if family == "hot":
        assert top >= 50


# ---- 3. sink rows are the sink's V row -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", (0, 1))
@pytest.mark.parametrize("B,T,S,heads,kvh,d,starts", CONDITION_SHAPES)
def test_sink_reference_is_the_sinks_v_row(B, T, S, heads, kvh, d, starts, ps):
    q, kc, vc = F.sink(B, T, S, heads, kvh, d, ps, starts=starts, b0=1, Bc=B + 2)
    ref = F.reference(q, kc, vc, S, heads, kvh, ps, b0=1, starts=starts)
    want = F.sink_rows(q, vc, S, heads, kvh, b0=1, starts=starts)
    assert (ref == want).all()
    a = np.abs(R.f64(want[F.real_rows(B, T, S, starts)]))
    assert a.min() >= 2.0 ** -4 and a.max() < 8


# ---- 4. the bounds are attainable ------------------------------------------------------------------------------------------------
def emulate(q, kc, vc, S, heads, kvh, ps, b0=0, starts=None, tile=64):
    """fp32 emulation of the kernels' schemes.  tile = 64 / 32: two sweeps over key tiles (online maximum and sum,
    l = l * exp2((m - mn) log2 e) + ts; then P = bf16(exp2((s - m) log2 e) / l), O += P . V in fp32), as the prefill kernels;
    tile = None: one pass with the scores stored, as the decode kernel.  A helper that shows the bound can be met, not a reference."""
    B, T, H = q.shape
    d, G = H // heads, heads // kvh
    scale = np.float32(float(d) ** -0.5)
    out = np.zeros((B, T, heads, d), np.uint16)
    for b, s, qb, kb, vb in F.rows(q, kc, vc, S, starts, b0):
        n, Tq = S - s, qb.shape[1]
        vis = np.arange(n)[None, :] <= (n - Tq + np.arange(Tq))[:, None]
        for hh in range(heads):
            qv, kv, vv = f32(qb[0]).reshape(Tq, heads, d)[:, hh], f32(kb[:n, 0, hh // G]), f32(vb[:n, 0, hh // G])
            sc = rb(rb(qv @ kv.T) * scale) if ps else rb(rb(qv * scale) @ kv.T)
            sc = np.where(vis, sc, np.float32(-np.inf))
            if tile is None:
                m = sc.max(axis=1, keepdims=True)
                e = np.exp2((sc - m) * LOG2E)
                o = rb(e / e.sum(axis=1, keepdims=True, dtype=np.float32)) @ vv
            else:
                m, l = np.full((Tq, 1), -np.inf, np.float32), np.zeros((Tq, 1), np.float32)
                for j0 in range(0, n, tile):
                    t = sc[:, j0:j0 + tile]
                    mn = np.maximum(m, t.max(axis=1, keepdims=True))
                    l = l * np.exp2((m - mn) * LOG2E) + np.exp2((t - mn) * LOG2E).sum(axis=1, keepdims=True, dtype=np.float32)
                    m = mn
                o = np.zeros((Tq, d), np.float32)
                for j0 in range(0, n, tile):
                    o = o + rb(np.exp2((sc[:, j0:j0 + tile] - m) * LOG2E) / l) @ vv[j0:j0 + tile]
            out[b, T - Tq:, hh] = synth.f32_to_bf16_bits(o)
    return out.reshape(B, T, H)


# one shape of each kernel class: (B, T, S, heads, kv_heads, d, starts, tile)
CLASS_SHAPES = {
    "prefill d 128": (2, 257, 257, 4, 2, 128, None, 64),
    "prefill generic": (2, 129, 129, 4, 2, 32, None, 32),
    "prefill padded": (3, 257, 257, 4, 2, 128, [1, 64, 255], 64),
    "decode": (3, 1, 1037, 8, 2, 128, None, None),
    "decode padded": (3, 1, 1037, 4, 2, 32, [0, 63, 1036], None),
}


def compare(what, got, ref, family, want_sink=None, slack=None):
    """the comparison the GPU tests use (test_gpu_attention_families.check_case restates it on the kernels' outputs)"""
    ok, msg = family_verdict(family, got, ref, slack)
    print(f"\n{what}: {msg}")
    assert not np.isnan(R.f64(got)).any(), f"{what}: NaN in the output"
    assert ok, f"{what}: {msg}"
    if want_sink is not None:
        assert (got == want_sink).all(), f"{what}: {(got != want_sink).sum()} outputs are not the sink's V row"


@pytest.mark.parametrize("ps", (0, 1))
@pytest.mark.parametrize("cls", list(CLASS_SHAPES))
@pytest.mark.parametrize("family", F.FAMILIES)
def test_bounds_are_attainable(family, cls, ps):
    """An fp32 emulation of the kernels' arithmetic passes the GPU tests' comparison against f64_ref.attention on every family
    and one shape of each kernel class; sink rows bit for bit.
    Measured: >= 99.98 % bit-identical, <= 0.25 quantum (lowest: hot on the generic prefill shape)."""
    B, T, S, heads, kvh, d, starts, tile = CLASS_SHAPES[cls]
    q, kc, vc = F.make(family, B, T, S, heads, kvh, d, ps, starts=starts, b0=1, Bc=B + 2)
    got = emulate(q, kc, vc, S, heads, kvh, ps, b0=1, starts=starts, tile=tile)
    ref = F.reference(q, kc, vc, S, heads, kvh, ps, b0=1, starts=starts)
    compare(f"emulation {cls} {family} ps {ps}", got, ref, family,
            F.sink_rows(q, vc, S, heads, kvh, 1, starts) if family == "sink" else None,
            F.order_slack(q, kc, vc, S, heads, kvh, ps, 1, starts) if family == "hot" else None)


def test_hot_needs_the_order_slack_and_no_more():
    """hot at (B 2, T 257, heads 8 / 2, d 64, post_scale 1): a plain fp32 emulation is 99.97 % bit-identical to the float64
    reference and still 5.8 quanta off on one row (a score next to a bf16 tie that carries weight) -- the plain comparison cannot
    be met there by an fp32 q . k -- and it is inside the comparison with attn_families.order_slack (that row at 0.14 of its widened bound);
    the slack itself stays small: zero for most rows, below one quantum of the largest output on average."""
    B, T, heads, kvh, d, ps = 2, 257, 8, 2, 64, 1
    q, kc, vc = F.hot(B, T, T, heads, kvh, d, ps, b0=1, Bc=B + 2)
    got, ref = emulate(q, kc, vc, T, heads, kvh, ps, b0=1, tile=None), F.reference(q, kc, vc, T, heads, kvh, ps, b0=1)
    slack = F.order_slack(q, kc, vc, T, heads, kvh, ps, 1)
    ok, msg = verdict(got, ref, **ATTN)
    print(f"\nplain: {msg}")
    assert not ok and float((got == ref).mean()) > 0.999
    ok, msg = family_verdict("hot", got, ref, slack)
    print(f"with the order slack: {msg}")
    assert ok
    assert np.median(slack) < 1e-9 and slack.mean() < R.quantum(np.abs(R.f64(ref)).max())


# ---- 5. the comparison rejects every mutant on a named family ---------------------------------------------------------------------
@pytest.mark.parametrize("cls", ("prefill d 128", "prefill generic", "prefill padded", "decode", "decode padded"))
def test_mutants_are_rejected_on_their_families(cls):
    """f64_ref.attention with one switch turned (mask off by one either way, P or q.k not rounded, the other scaling, the other
    head map) against an output that passes the right reference (the emulation's): every pair of attn_families.MUTANT_PAIRS is
    rejected by the GPU tests' comparison; the margin of every (mutant, family) is printed."""
    B, T, S, heads, kvh, d, starts, tile = CLASS_SHAPES[cls]
    ps = 1
    pairs = F.MUTANT_PAIRS if T > 1 else F.DECODE_MUTANT_PAIRS
    rejected = set()
    for family in F.FAMILIES:
        q, kc, vc = F.make(family, B, T, S, heads, kvh, d, ps, starts=starts, b0=1, Bc=B + 2)
        got = emulate(q, kc, vc, S, heads, kvh, ps, b0=1, starts=starts, tile=tile)
        slack = F.order_slack(q, kc, vc, S, heads, kvh, ps, 1, starts) if family == "hot" else None
        ok, msg = family_verdict(family, got, F.reference(q, kc, vc, S, heads, kvh, ps, b0=1, starts=starts), slack)
        assert ok, f"{cls} {family}: {msg}"
        for name, kw in F.MUTANTS.items():
            with np.errstate(invalid="ignore"):
                ok, msg = family_verdict(family, got, F.reference(q, kc, vc, S, heads, kvh, ps, b0=1, starts=starts, **kw), slack)
            print(f"\n{cls} {family} vs mutant '{name}': {'passes' if ok else 'REJECTED'}: {msg}")
            if not ok:
                rejected.add((name, family))
    assert set(pairs) <= rejected, f"{cls}: not rejected: {sorted(set(pairs) - rejected)}"
    assert {m for m, _ in F.MUTANT_PAIRS} == set(F.MUTANTS)


# ---- 7. the host attention against the oracle's CPU branch ------------------------------------------------------------------------
HOST_ATOL, HOST_RTOL, HOST_MIN_EXACT = 0.02, 0.016, 0.97
HOST_SHAPES = [(7, 0), (7, 5), (130, 0), (130, 5), (1, 64), (1, 1036), (1, 2047)]          # (T, pos0): prefill, decode S 65 / 1037 / 2048


def run_host(fn, q, k, v, kc, vc, T, pos0, heads, d, b0, threads, starts=None):
    from lia_amd import _native as N
    B, Bc = q.shape[0], kc.shape[1]
    out = np.full_like(q, F.NAN)
    kc, vc = kc.copy(), vc.copy()
    extra = () if starts is None else (np.ascontiguousarray(starts, np.int32).ctypes.data,)
    rc = getattr(N.lib(), fn)(q.ctypes.data, k.ctypes.data, v.ctypes.data, kc.ctypes.data, vc.ctypes.data, out.ctypes.data,
                              B, T, pos0, heads, d, Bc, b0, threads, *extra)
    assert rc == 0, N.lib().lia_last_error()
    return out, kc, vc


def host_inputs(q, kc, vc, pos0, S, b0):
    """the call's operands: the new K / V rows [B, T, H] (cache rows pos0 .. S - 1 of the served rows) and the cache with every
    row from pos0 on -- which the call itself appends -- poisoned"""
    B, T, H = q.shape
    k = np.ascontiguousarray(kc[pos0:S, b0:b0 + B].transpose(1, 0, 2, 3)).reshape(B, T, H)
    v = np.ascontiguousarray(vc[pos0:S, b0:b0 + B].transpose(1, 0, 2, 3)).reshape(B, T, H)
    kin, vin = kc.copy(), vc.copy()
    kin[pos0:], vin[pos0:] = F.NAN, F.NAN
    return k, v, kin, vin


def host_check(what, out, q, kc, vc, S, heads, starts, b0, oracle, family):
    B, T, H = q.shape
    ref = np.zeros_like(out)
    for b, s, qb, kb, vb in F.rows(q, kc, vc, S, starts, b0):
        ref[b, T - qb.shape[1]:] = oracle.attention(np.ascontiguousarray(qb), np.ascontiguousarray(kb), np.ascontiguousarray(vb),
                                                    S - s, heads, policy_gpu=False, causal=True)[0]
    real = F.real_rows(B, T, S, starts)
    assert (out[~real] == 0).all(), f"{what}: a pad query row is not exactly zero"
    a, r = R.f64(out[real]), R.f64(ref[real])
    assert not np.isnan(a).any(), f"{what}: NaN in the output"
    err = np.abs(a - r)
    frac = float((out[real] == ref[real]).mean())
    print(f"\n{what}: {100 * frac:.3f} % bit-identical, worst err - bound {float((err - HOST_ATOL - HOST_RTOL * np.abs(r)).max()):.4g}")
    assert (err <= HOST_ATOL + HOST_RTOL * np.abs(r)).all() and frac > HOST_MIN_EXACT, what
    if family == "sink":
        assert (out == F.sink_rows(q, vc, S, heads, heads, b0, starts)).all(), f"{what}: not the sink's V row"


@pytest.mark.parametrize("threads", (1, 16))
@pytest.mark.parametrize("d", (64, 128))
@pytest.mark.parametrize("T,pos0", HOST_SHAPES)
@pytest.mark.parametrize("family", F.FAMILIES)
def test_host_attention_on_the_families(oracle, family, T, pos0, d, threads):
    """lia_host_attention and lia_host_attention_padded against the oracle's CPU branch (fp32 scores and softmax, one rounding at
    the output: its rounding points are not the GPU's), prefill and decode up to S 2048, 1 and 16 threads, cache rows from pos0
    on and pad rows poisoned.  err <= 0.02 + 0.016 |ref| (test_host_attention_matches_oracle's bound with the project's relative
    term: these families put |ref| >= 4 on single V rows, where one bf16 quantum is 0.031), > 97 % bit-identical, sink rows bit
    for bit; each row of the padded call equals its own unpadded call bit for bit.
    Measured (AVX-512 host): >= 99.8 % bit-identical (hot, decode S 1037, d 128), every error below 0.016 |ref|."""
    B, heads, b0 = 4, 2, 2
    S = pos0 + T
    H = heads * d
    mid = 63 if T == 1 else pos0 + 2                     # decode: a start inside the cache; prefill: one behind pos0
    for starts in (None, np.array([0, min(1, S - 1), min(mid, S - 1), S - 1], np.int32)):
        q, kc, vc = F.make(family, B, T, S, heads, heads, d, 0, starts=starts, b0=b0, Bc=B + 3)
        k, v, kin, vin = host_inputs(q, kc, vc, pos0, S, b0)
        if starts is None:
            out, k2, v2 = run_host("lia_host_attention", q, k, v, kin, vin, T, pos0, heads, d, b0, threads)
        else:
            out, k2, v2 = run_host("lia_host_attention_padded", q, k, v, kin, vin, T, pos0, heads, d, b0, threads, starts)
        assert (k2[:S] == kc[:S]).all() and (v2[:S] == vc[:S]).all(), "the new rows were not appended in place"
        assert (k2[S:] == F.NAN).all() and (v2[S:] == F.NAN).all()
        what = f"host {family} T {T} pos0 {pos0} d {d} threads {threads} starts {None if starts is None else starts.tolist()}"
        host_check(what, out, q, kc, vc, S, heads, starts, b0, oracle, family)
        if starts is None:
            continue
        for b, s, qb, kb, vb in F.rows(q, kc, vc, S, starts, b0):          # row b alone, on its own shifted sequence
            Tq, p0 = qb.shape[1], max(pos0 - s, 0)
            qb, kb, vb = np.ascontiguousarray(qb), np.ascontiguousarray(kb), np.ascontiguousarray(vb)
            k1, v1, kin1, vin1 = host_inputs(qb, kb, vb, p0, S - s, 0)
            o1, _, _ = run_host("lia_host_attention", qb, k1, v1, kin1, vin1, Tq, p0, heads, d, 0, threads)
            assert (out[b, T - Tq:] == o1[0]).all(), f"{what}: row {b} differs from its unpadded run"
    assert H == q.shape[2]
