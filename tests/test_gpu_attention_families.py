"""-m gpu: every attention kernel the launchers dispatch to, on the input families of attn_families.py -- an attention sink, scores
in the hundreds, one-hot rows, a maximum that moves in every key tile, exp underflowing for most keys, p = 1 / n -- against
f64_ref.attention, with test_gpu_kernel_variants.py's comparison (ATTN_MIN_EXACT, one quantum, ATTN_ATOL / ATTN_RTOL) and
plumbing.  What the kernels must not read is NaN: cache rows behind S, cache batch rows that are not served, V at pad positions
(K there would outscore every real key), the pitch gap of q.  tests/test_attn_families.py is the CPU half: the families' rules,
that the bounds are attainable, and which (mutant, family) pairs the comparison rejects."""
import numpy as np
import pytest

import attn_families as F
import f64_ref as R
from test_attn_families import CLASS_SHAPES, family_verdict
from test_gpu_kernel_variants import (ATTN_ATOL, ATTN_MIN_EXACT, ATTN_QBLOCK, ATTN_RTOL, DECODE_G, SENTINEL, X_GAP, check, decode_s_max,
                                      gpu, host, pitched, prefill_variant, sentinel_buf)  # noqa: F401  (gpu: fixture)

pytestmark = pytest.mark.gpu

ATTN = dict(min_exact=ATTN_MIN_EXACT, bound=(ATTN_ATOL, ATTN_RTOL))
VARIANTS = ("128/r05", "128/xcd", "128/xcd-padded", "generic<32>", "generic<64>")
OUT_SLACK = 2                       # rows of `out` behind the last served row: they keep the sentinel
B0, BC_EXTRA = 1, 2                 # served rows b0 = 1 .. B of Bc = B + 2

# (B, T, heads, kv_heads, d) per variant and post_scale: T 129 / 257 / 641 are 2 / 3 / 6 query blocks of 128 (odd counts pair the
# middle block with itself), each with rows past the last full key tile; 128/xcd-padded needs >= 65 (batch row, KV head) groups
PREFILL_SHAPES = {
    "128/r05": {0: (1, 641, 8, 2, 128), 1: (3, 257, 6, 3, 128)},
    "128/xcd": {0: (4, 257, 16, 2, 128), 1: (2, 641, 4, 4, 128)},
    "128/xcd-padded": {0: (13, 129, 5, 5, 128), 1: (13, 129, 10, 5, 128)},
    "generic<32>": {0: (2, 257, 16, 2, 32), 1: (1, 641, 4, 2, 32)},
    "generic<64>": {0: (1, 641, 4, 4, 64), 1: (2, 257, 8, 2, 64)},
}
PREFILL_CASES = [(fam, v, ps) for fam in F.FAMILIES for v in VARIANTS for ps in (0, 1)]
# every group size at every d once more (the lists above hold G 1 / 2 / 4 / 8 only at some d), the families taken in turn
GROUP_CASES = [(F.FAMILIES[(3 * i + j) % len(F.FAMILIES)], (2, 129, 2 * G, 2, d), (i + j) % 2)
               for i, d in enumerate((32, 64, 128)) for j, G in enumerate(DECODE_G)]
# left padding: the starts of one batch mix 0, 1, 63, 64, 65, 127, 128 and T - 1 (more rows take them again)
PADDED_SHAPES = {
    "128/r05": {0: (9, 641, 2, 1, 128), 1: (9, 257, 4, 1, 128)},
    "128/xcd": {0: (8, 257, 4, 2, 128), 1: (8, 641, 2, 1, 128)},
    "128/xcd-padded": {0: (13, 129, 5, 5, 128), 1: (13, 129, 10, 5, 128)},
    "generic<32>": {0: (8, 257, 8, 1, 32), 1: (8, 129, 4, 2, 32)},
    "generic<64>": {0: (8, 129, 4, 4, 64), 1: (8, 257, 4, 2, 64)},
}
START_POOL = (0, 1, 63, 64, 65, 127, 128)
DECODE_S = (65, 1037)
DECODE_PADDED_B = len(START_POOL) + 1


def starts_for(B, n):
    """B starts over the pool's values below n - 1, and n - 1 itself"""
    pool = [s for s in START_POOL if s < n - 1] + [n - 1]
    return np.array([pool[b % len(pool)] for b in range(B)], np.int32)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def run_case(gpu, family, B, T, S, heads, kvh, d, ps, starts=None, shifted=False):
    """the family's case through the prefill (T > 1) or decode launcher, padded when `starts` is given: ldq / ldo > H with NaN /
    sentinel gaps, b0 = 1 of Bc = B + 2, NaN in every cache row that is not to be read.  -> (q, kc, vc, out [B, T, H]).
    shifted: every row of the padded prefill is launched once more alone, UNPADDED, on its own shifted sequence (pointers moved to
    the row's start) and must equal the padded launch's row bit for bit."""
    torch, launch = gpu
    Bc, H = B + BC_EXTRA, heads * d
    ldq, ldo = H + 16, H + 24
    q, kc, vc = F.make(family, B, T, S, heads, kvh, d, ps, starts=starts, b0=B0, Bc=Bc)
    qd = pitched(torch, dev(torch, q.reshape(B * T, H)), ldq, X_GAP)
    kd, vd = dev(torch, kc), dev(torch, vc)
    out = sentinel_buf(torch, (B * T + OUT_SLACK, ldo))
    name = "lia_attn_prefill" if T > 1 else "lia_attn_decode"
    n = T if T > 1 else S
    if starts is None:
        rc = launch(name + "_launch", qd, ldq, kd, vd, out, ldo, B, n, heads, kvh, d, Bc, B0, ps)
    else:
        st = torch.from_numpy(np.asarray(starts, np.int32)).cuda()
        rc = launch(name + "_padded_launch", qd, ldq, kd, vd, out, ldo, B, n, heads, kvh, d, Bc, B0, ps, st)
    assert rc == 0
    oh = host(out)
    assert (oh[:, H:] == SENTINEL).all(), "the launch wrote into the gap columns of out"
    assert (oh[B * T:] == SENTINEL).all(), "the launch wrote behind the last served row of out"
    assert (host(kd) == kc).all() and (host(vd) == vc).all(), "the launch changed the cache"
    got = oh[:B * T, :H].reshape(B, T, H)
    if shifted:
        kv_row = Bc * kvh * d
        for b, s in enumerate(starts):
            s = int(s)
            o1 = sentinel_buf(torch, (T - s + OUT_SLACK, ldo))
            rc = launch("lia_attn_prefill_launch", qd.data_ptr() + 2 * (b * T + s) * ldq, ldq, kd.data_ptr() + 2 * s * kv_row,
                        vd.data_ptr() + 2 * s * kv_row, o1, ldo, 1, T - s, heads, kvh, d, Bc, B0 + b, ps)
            assert rc == 0
            o1 = host(o1)
            assert (o1[T - s:] == SENTINEL).all() and (o1[:, H:] == SENTINEL).all()
            assert (o1[:T - s, :H] == got[b, s:]).all(), f"row {b} (start {s}) differs from its own unpadded launch"
    return q, kc, vc, got


def check_case(what, q, kc, vc, got, family, S, heads, kvh, ps, starts=None):
    """no NaN anywhere, pad query rows exact zeros, the real rows inside the file's attention comparison against
    f64_ref.attention, sink rows the sink's V row bit for bit"""
    B, T, _ = q.shape
    assert not np.isnan(R.f64(got)).any(), f"{what}: NaN in the output (a poisoned row was read)"
    real = F.real_rows(B, T, S, starts)
    assert (got[~real] == 0).all(), f"{what}: a pad query row is not exactly zero"
    ref = F.reference(q, kc, vc, S, heads, kvh, ps, b0=B0, starts=starts)
    if family == "hot":        # q . k is not exact in fp32 there: the same bounds + what the order of that sum alone can do (family_verdict)
        ok, msg = family_verdict(family, got[real], ref[real], F.order_slack(q, kc, vc, S, heads, kvh, ps, B0, starts)[real])
        print(f"\n{what}: {msg}")
        assert ok, f"{what}: {msg}"
    else:
        check(what, got[real], ref[real], **ATTN)
    if family == "sink":
        want = F.sink_rows(q, vc, S, heads, kvh, B0, starts)
        assert (got == want).all(), f"{what}: {(got != want).sum()} outputs are not the sink's V row"


@pytest.mark.parametrize("family,variant,ps", PREFILL_CASES)
def test_prefill_families(gpu, family, variant, ps):
    """lia_attn_prefill_launch: every family x every kernel variant x both scalings, T 129 / 257 / 641.
    Measured on the MI355X: the exact families >= 99.979 % bit-identical, max 0.5 quantum (128/xcd exact, post_scale 0); sink rows
    bit for bit; no kernel had to change.  hot: >= 99.967 % bit-identical, one row 3.250 / 4.125 / 5.812 quanta off (128/xcd and
    128/xcd-padded post_scale 0, generic<64> post_scale 1) where a weighty score's fp32 sum rounds to the other bf16 neighbour
    than float64's -- the figures of a plain fp32 emulation to the digit, inside the order slack (test_attn_families.family_verdict)."""
    B, T, heads, kvh, d = PREFILL_SHAPES[variant][ps]
    assert prefill_variant(B, T, kvh, d) == variant
    q, kc, vc, got = run_case(gpu, family, B, T, T, heads, kvh, d, ps)
    check_case(f"prefill {variant} {family} B {B} T {T} heads {heads}/{kvh} post {ps}", q, kc, vc, got, family, T, heads, kvh, ps)


@pytest.mark.parametrize("family,shape,ps", GROUP_CASES)
def test_prefill_families_every_group_size(gpu, family, shape, ps):
    """G 1 / 2 / 4 / 8 at every d, the families in turn.  Measured: >= 99.979 % bit-identical, max 0.5 quantum."""
    B, T, heads, kvh, d = shape
    q, kc, vc, got = run_case(gpu, family, B, T, T, heads, kvh, d, ps)
    check_case(f"prefill {family} heads {heads}/{kvh} d {d} post {ps}", q, kc, vc, got, family, T, heads, kvh, ps)


@pytest.mark.parametrize("family,variant,ps", PREFILL_CASES)
def test_padded_prefill_families(gpu, family, variant, ps):
    """lia_attn_prefill_padded_launch: the same, the starts of one batch mixing 0, 1, 63, 64, 65, 127, 128 and T - 1; K rows at the
    pad positions would outscore every real key and their V rows are NaN; pad query rows are zeros; every real row equals the same
    row of an unpadded launch on the shifted sequence bit for bit (the kernels' documented promise).
    Measured: >= 99.978 % bit-identical (generic<64> hot), max 0.5 quantum (128/r05 exact); every row equal to its own launch."""
    B, T, heads, kvh, d = PADDED_SHAPES[variant][ps]
    assert prefill_variant(B, T, kvh, d) == variant
    starts = starts_for(B, T)
    q, kc, vc, got = run_case(gpu, family, B, T, T, heads, kvh, d, ps, starts=starts, shifted=True)
    check_case(f"padded prefill {variant} {family} B {B} T {T} heads {heads}/{kvh} post {ps}", q, kc, vc, got, family, T, heads, kvh,
               ps, starts)


@pytest.mark.parametrize("S", DECODE_S)
@pytest.mark.parametrize("family", F.FAMILIES)
@pytest.mark.parametrize("ps", (0, 1))
@pytest.mark.parametrize("G", DECODE_G)
@pytest.mark.parametrize("D", (32, 64, 128))
def test_decode_families(gpu, D, G, ps, family, S):
    """lia_attn_decode_launch and lia_attn_decode_padded_launch: all twelve <D, G> x both scalings x every family at S 65 / 1037,
    the padded batch's starts mixing 0, 1, 63, 64 (65, 127, 128 at S 1037) and S - 1.
    Measured: unpadded >= 97.786 % bit-identical (<32, 4> post_scale 1 exact S 1037: 17 of 768 outputs, one probability next to a
    bf16 tie), max 0.5 quantum; padded >= 99.951 %, max 0.5 quantum."""
    kvh = 2
    q, kc, vc, got = run_case(gpu, family, 3, 1, S, G * kvh, kvh, D, ps)
    check_case(f"decode <{D}, {G}> post {ps} {family} S {S}", q, kc, vc, got, family, S, G * kvh, kvh, ps)
    starts = starts_for(DECODE_PADDED_B, S)
    q, kc, vc, got = run_case(gpu, family, len(starts), 1, S, G * kvh, kvh, D, ps, starts=starts)
    check_case(f"padded decode <{D}, {G}> post {ps} {family} S {S}", q, kc, vc, got, family, S, G * kvh, kvh, ps, starts)


@pytest.mark.parametrize("G", DECODE_G)
@pytest.mark.parametrize("D", (32, 64, 128))
def test_decode_ramp_at_the_lds_bound(gpu, D, G):
    """ramp at the largest S the decode launcher accepts at <D, G> (the scores fill the 160 KiB of LDS), unpadded and padded.
    Measured: inside the bounds at every <D, G> (S 4600 .. 40824)."""
    S = decode_s_max(D, G)
    q, kc, vc, got = run_case(gpu, "ramp", 2, 1, S, G, 1, D, 1)
    check_case(f"decode <{D}, {G}> ramp at the LDS bound S {S}", q, kc, vc, got, "ramp", S, G, 1, 1)
    starts = np.array([65, S - 1, 0], np.int32)
    q, kc, vc, got = run_case(gpu, "ramp", 3, 1, S, G, 1, D, 0, starts=starts)
    check_case(f"padded decode <{D}, {G}> ramp at the LDS bound S {S}", q, kc, vc, got, "ramp", S, G, 1, 0, starts)


def test_cases_reach_every_variant_and_family():
    """Every (variant, family, post_scale) is in both prefill lists with a shape that the launcher sends to that variant; 2, 3 and
    6 query blocks occur for the d 128 kernels and the generic one; every G at every d; every start of the pool in every padded
    batch.  Deleting a family or a variant from a list fails here."""
    want = {(f, v, ps) for f in ("exact", "ramp", "fall", "sink", "uniform", "hot")
            for v in ("128/r05", "128/xcd", "128/xcd-padded", "generic<32>", "generic<64>") for ps in (0, 1)}
    assert set(PREFILL_CASES) == want and set(F.FAMILIES) == {f for f, _, _ in want}
    for shapes, generic_blocks in ((PREFILL_SHAPES, {3, 6}), (PADDED_SHAPES, {2, 3})):
        assert set(shapes) == set(VARIANTS)
        blocks = {True: set(), False: set()}
        for v, by_ps in shapes.items():
            assert set(by_ps) == {0, 1}
            for B, T, heads, kvh, d in by_ps.values():
                assert prefill_variant(B, T, kvh, d) == v
                blocks[d == 128].add(-(-T // ATTN_QBLOCK))
        assert blocks[True] == {2, 3, 6} and blocks[False] == generic_blocks
    assert {(d, h // k) for _, (B, T, h, k, d), _ in GROUP_CASES} == {(d, G) for d in (32, 64, 128) for G in DECODE_G}
    assert {f for f, _, _ in GROUP_CASES} == set(F.FAMILIES)
    for by_ps in PADDED_SHAPES.values():
        for B, T, _, _, _ in by_ps.values():
            assert set(starts_for(B, T).tolist()) == set(START_POOL) | {T - 1}
    assert set(starts_for(DECODE_PADDED_B, 1037).tolist()) == set(START_POOL) | {1036}
    assert set(starts_for(DECODE_PADDED_B, 65).tolist()) == {0, 1, 63, 64}
    assert {m for m, _ in F.MUTANT_PAIRS} == set(F.MUTANTS) and {f for _, f in F.MUTANT_PAIRS} <= set(F.FAMILIES)


@pytest.mark.parametrize("cls", ("prefill d 128", "prefill generic", "decode", "prefill padded"))
def test_family_mutants_are_rejected(gpu, cls):
    """The kernel's output passes the comparison against the right reference and FAILS it against f64_ref.attention with one
    switch turned, for every (mutant, family) pair that tests/test_attn_families.py names: mask off by one either way (ramp), P
    not rounded (exact), q.k not rounded and the other scaling (hot), kh = hh % kv_heads (sink).
    Measured: the closest mutant is P not rounded on exact (77.4 - 77.9 % bit-identical against the 95 % asked); q.k not rounded
    and the other scaling on hot 72 - 76 %, 11 - 18 quanta; the others 0.1 - 50 % or infinite error."""
    B, T, S, heads, kvh, d, starts, _ = CLASS_SHAPES[cls]
    ps = 1
    pairs = F.MUTANT_PAIRS if T > 1 else F.DECODE_MUTANT_PAIRS
    for family in sorted({f for _, f in pairs}):
        q, kc, vc, got = run_case(gpu, family, B, T, S, heads, kvh, d, ps, starts=starts)
        real = F.real_rows(B, T, S, starts)
        slack = F.order_slack(q, kc, vc, S, heads, kvh, ps, B0, starts)[real] if family == "hot" else None
        ok, msg = family_verdict(family, got[real], F.reference(q, kc, vc, S, heads, kvh, ps, b0=B0, starts=starts)[real], slack)
        assert ok, f"{cls} {family}: the kernel fails the right reference: {msg}"
        for name in (m for m, f in pairs if f == family):
            with np.errstate(invalid="ignore"):
                ref = F.reference(q, kc, vc, S, heads, kvh, ps, b0=B0, starts=starts, **F.MUTANTS[name])
            ok, msg = family_verdict(family, got[real], ref[real], slack)
            print(f"\n{cls} {family} vs mutant '{name}': {msg}")
            assert not ok, f"{cls} {family}: the mutant '{name}' is not rejected: {msg}"
