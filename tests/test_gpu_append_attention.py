"""-m gpu: lia_attn_append_launch -- a block of T queries at cache positions pos0 .. pos0 + T - 1 over the keys the cache already
holds -- on every input family of attn_families.py, through every kernel the launcher can pick (d 32 / 64 / 128, the three d = 128
grid orders, G 1 / 2 / 4 / 8, both scalings), unpadded and with row starts, against f64_ref.attention with
test_gpu_attention_families.py's own comparison and plumbing; and the property the kernels are built on: the block's rows are bit
for bit rows pos0 .. pos0 + T - 1 of the prefill launch over pos0 + T tokens.

S = pos0 + T is what attn_families.make / reference take: T queries at positions S - T .. S - 1 over S keys."""
import numpy as np
import pytest

import attn_families as F
from test_gpu_attention_families import ATTN, B0, BC_EXTRA, OUT_SLACK, VARIANTS, check_case, dev  # noqa: F401
from test_gpu_kernel_variants import (DECODE_G, SENTINEL, X_GAP, gpu, host, pitched, prefill_variant,  # noqa: F401  (gpu: fixture)
                                      sentinel_buf)

pytestmark = pytest.mark.gpu

POS0 = (1, 63, 64, 65, 127, 128, 129, 1000)
TS = (1, 2, 17, 128, 129, 257)
PAIRS = [(p, t) for t in TS for p in POS0]
START_POOL = (0, 1, 63, 64)

# (B, heads, kv_heads, d) per variant and post_scale; the variant is the prefill launcher's rule on (B, kv_heads, d), which the append
# launcher shares: B * kv_heads a multiple of 8 -> 128/xcd, >= 64 otherwise -> 128/xcd-padded, else 128/r05
SHAPES = {
    "128/r05": {0: (1, 8, 2, 128), 1: (3, 6, 3, 128)},
    "128/xcd": {0: (4, 16, 2, 128), 1: (2, 4, 4, 128)},
    "128/xcd-padded": {0: (13, 5, 5, 128), 1: (13, 10, 5, 128)},
    "generic<32>": {0: (2, 16, 2, 32), 1: (3, 4, 2, 32)},
    "generic<64>": {0: (3, 4, 4, 64), 1: (2, 8, 2, 64)},
}
# every (family, variant, post_scale), the (pos0, T) pairs taken in turn: 60 cases over 48 pairs
CASES = [(fam, v, ps) + PAIRS[i % len(PAIRS)]
         for i, (fam, v, ps) in enumerate((fam, v, ps) for fam in F.FAMILIES for v in VARIANTS for ps in (0, 1))]
# every group size at every d, the families and the pairs in turn (another stride through the pairs)
GROUP_CASES = [(F.FAMILIES[(3 * i + j) % len(F.FAMILIES)], (2, 2 * G, 2, d), (i + j) % 2) + PAIRS[(7 * (4 * i + j) + 5) % len(PAIRS)]
               for i, d in enumerate((32, 64, 128)) for j, G in enumerate(DECODE_G)]


def starts_for(B, pos0):
    """B starts mixing 0, 1, 63, 64 (those below pos0) and pos0 itself: s_b <= pos0, a block has no pad query rows"""
    pool = [s for s in START_POOL if s < pos0] + [pos0]
    return np.array([pool[(b + 1) % len(pool)] for b in range(B)], np.int32)


def append(gpu, q, kc, vc, pos0, heads, kvh, d, ps, starts=None):
    """q [B, T, H], caches [.., Bc = B + 2, kvh, d] (bf16 bits) through lia_attn_append_launch, test_gpu_attention_families.run_case's
    plumbing: pitched q / out with NaN / sentinel gaps, served rows b0 = 1 .. B, the cache unchanged.  -> out [B, T, H]"""
    torch, launch = gpu
    B, T, H = q.shape
    Bc = kc.shape[1]
    assert Bc == B + BC_EXTRA
    ldq, ldo = H + 16, H + 24
    qd = pitched(torch, dev(torch, q.reshape(B * T, H)), ldq, X_GAP)
    kd, vd = dev(torch, kc), dev(torch, vc)
    out = sentinel_buf(torch, (B * T + OUT_SLACK, ldo))
    st = None if starts is None else torch.from_numpy(np.asarray(starts, np.int32)).cuda()
    rc = launch("lia_attn_append_launch", qd, ldq, kd, vd, out, ldo, B, T, pos0, heads, kvh, d, Bc, B0, ps, st)
    assert rc == 0
    oh = host(out)
    assert (oh[:, H:] == SENTINEL).all(), "the launch wrote into the gap columns of out"
    assert (oh[B * T:] == SENTINEL).all(), "the launch wrote behind the last served row of out"
    assert (host(kd) == kc).all() and (host(vd) == vc).all(), "the launch changed the cache"
    return oh[:B * T, :H].reshape(B, T, H)


def run_case(gpu, family, B, T, pos0, heads, kvh, d, ps, starts=None):
    S = pos0 + T
    q, kc, vc = F.make(family, B, T, S, heads, kvh, d, ps, starts=starts, b0=B0, Bc=B + BC_EXTRA)
    return q, kc, vc, append(gpu, q, kc, vc, pos0, heads, kvh, d, ps, starts)


@pytest.mark.parametrize("family,variant,ps,pos0,T", CASES)
def test_append_families(gpu, family, variant, ps, pos0, T):
    """every family x every kernel variant x both scalings, the (pos0, T) pairs in turn; NaN behind S, in the rows not served and in
    the pitch gaps.
    Measured on the MI355X (this test and the two below): >= 99.988 % bit-identical to float64, max 0.5 quantum; sink rows bit for bit."""
    B, heads, kvh, d = SHAPES[variant][ps]
    assert prefill_variant(B, T, kvh, d) == variant
    q, kc, vc, got = run_case(gpu, family, B, T, pos0, heads, kvh, d, ps)
    check_case(f"append {variant} {family} B {B} pos0 {pos0} T {T} heads {heads}/{kvh} post {ps}", q, kc, vc, got, family, pos0 + T,
               heads, kvh, ps)


@pytest.mark.parametrize("family,variant,ps,pos0,T", CASES)
def test_append_families_padded(gpu, family, variant, ps, pos0, T):
    """the same with row starts mixing 0, 1, 63, 64 and pos0: a K row that would outscore every real key and a NaN V row at every
    position before a row's start."""
    B, heads, kvh, d = SHAPES[variant][ps]
    starts = starts_for(B, pos0)
    q, kc, vc, got = run_case(gpu, family, B, T, pos0, heads, kvh, d, ps, starts=starts)
    check_case(f"padded append {variant} {family} B {B} pos0 {pos0} T {T} heads {heads}/{kvh} post {ps}", q, kc, vc, got, family,
               pos0 + T, heads, kvh, ps, starts)


@pytest.mark.parametrize("family,shape,ps,pos0,T", GROUP_CASES)
def test_append_every_group_size(gpu, family, shape, ps, pos0, T):
    """G 1 / 2 / 4 / 8 at every d, unpadded and padded"""
    B, heads, kvh, d = shape
    for starts in (None, starts_for(B, pos0)):
        q, kc, vc, got = run_case(gpu, family, B, T, pos0, heads, kvh, d, ps, starts=starts)
        check_case(f"append {family} heads {heads}/{kvh} d {d} post {ps} pos0 {pos0} T {T} starts {starts}", q, kc, vc, got, family,
                   pos0 + T, heads, kvh, ps, starts)


@pytest.mark.parametrize("family,variant,ps,pos0,T", CASES)
def test_append_is_the_prefill_rows_bit_for_bit(gpu, family, variant, ps, pos0, T):
    """Given the same q rows and cache, the append launch over (pos0, T) equals rows pos0 .. pos0 + T - 1 of the prefill launch over
    pos0 + T tokens bit for bit -- unpadded against lia_attn_prefill_launch, with starts against lia_attn_prefill_padded_launch.  No
    tolerance: key blocks are aligned to the row's start in both launches, a block a row sees nothing of adds exact zeros, and a row's
    sums run over the same blocks in the same order.  Measured: 0 differing outputs in every case."""
    torch, launch = gpu
    B, heads, kvh, d = SHAPES[variant][ps]
    S, H, Bc = pos0 + T, heads * d, B + BC_EXTRA
    ldq, ldo = H + 16, H + 24
    for starts in (None, starts_for(B, pos0)):
        q, kc, vc = F.make(family, B, S, S, heads, kvh, d, ps, starts=starts, b0=B0, Bc=Bc)
        qd = pitched(torch, dev(torch, q.reshape(B * S, H)), ldq, X_GAP)
        kd, vd = dev(torch, kc), dev(torch, vc)
        full = sentinel_buf(torch, (B * S + OUT_SLACK, ldo))
        if starts is None:
            rc = launch("lia_attn_prefill_launch", qd, ldq, kd, vd, full, ldo, B, S, heads, kvh, d, Bc, B0, ps)
        else:
            st = torch.from_numpy(starts).cuda()
            rc = launch("lia_attn_prefill_padded_launch", qd, ldq, kd, vd, full, ldo, B, S, heads, kvh, d, Bc, B0, ps, st)
        assert rc == 0
        want = host(full)[:B * S, :H].reshape(B, S, H)[:, pos0:]
        got = append(gpu, np.ascontiguousarray(q[:, pos0:]), kc, vc, pos0, heads, kvh, d, ps, starts)
        assert not np.isnan(F.R.f64(got)).any()
        assert (got == want).all(), (f"{variant} {family} post {ps} pos0 {pos0} T {T} starts {starts}: {(got != want).sum()} of {got.size} "
                                     f"outputs differ from the prefill launch's rows")


def test_launcher_refusals(gpu):
    """-1 where the prefill launcher returns it: an unsupported head_dim, heads not a multiple of kv_heads, and at d = 128 a cache
    whose 64 key rows reach 4 GiB (nothing is launched, so no cache of that size is needed)"""
    torch, launch = gpu
    z = torch.zeros(8, dtype=torch.int16, device="cuda")
    assert launch("lia_attn_append_launch", z, 48, z, z, z, 48, 1, 2, 3, 1, 1, 48, 1, 0, 0, None) == -1
    assert launch("lia_attn_append_launch", z, 128, z, z, z, 128, 1, 2, 3, 3, 2, 64, 1, 0, 0, None) == -1
    assert launch("lia_attn_append_launch", z, 128, z, z, z, 128, 1, 2, 3, 64, 64, 128, 4096, 0, 0, None) == -1


def test_cases_reach_every_variant_family_and_pair():
    """every (family, variant, post_scale) once, every (pos0, T) pair of the issue's lists at least once, every G at every d, every
    start of the pool in the padded batches"""
    assert {c[:3] for c in CASES} == {(f, v, ps) for f in F.FAMILIES for v in VARIANTS for ps in (0, 1)}
    assert {c[3:] for c in CASES} == set(PAIRS) and len(PAIRS) == len(POS0) * len(TS)
    for v, by_ps in SHAPES.items():
        for B, heads, kvh, d in by_ps.values():
            assert prefill_variant(B, 1, kvh, d) == v
    assert {(s[3], s[1] // s[2]) for _, s, _, _, _ in GROUP_CASES} == {(d, G) for d in (32, 64, 128) for G in DECODE_G}
    assert set(starts_for(13, 1000).tolist()) == {0, 1, 63, 64, 1000} and set(starts_for(3, 1).tolist()) == {0, 1}
    assert all((starts_for(B, p) <= p).all() for p in POS0 for B in (1, 2, 3, 13))
