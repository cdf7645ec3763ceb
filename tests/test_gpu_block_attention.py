"""-m gpu: lia_attn_block_launch -- the decode kernel for the G * T query slots of a verification block (T = 2 .. 16 queries per row at
cache positions pos0 .. pos0 + T - 1) -- on every input family of attn_families.py at every d, both scalings and every instantiated
slot count, unpadded and with row starts, against f64_ref.attention with test_gpu_attention_families.py's comparison and the append
test's plumbing; and the property the kernel is built on: row t is bit for bit the decode launch over pos0 + t + 1 keys.

pos0 is taken around the decode kernel's pass of P = 8 * (256 / (d / 8)) keys (128 / 256 / 512 at d = 128 / 64 / 32): a block then
straddles the boundary between the full passes and the checked ones, where a per-slot limit goes wrong."""
import ctypes

import numpy as np
import pytest

import attn_families as F
from launchers import SIGNATURES
from test_attn_families import emulate, family_verdict
from test_gpu_append_attention import starts_for
from test_gpu_attention_families import B0, BC_EXTRA, OUT_SLACK, check_case, dev
from test_gpu_kernel_variants import SENTINEL, X_GAP, gpu, host, pitched, sentinel_buf  # noqa: F401  (gpu: fixture)

# lia_attn_append_launch's argument list (lia_internal.h): q, ldq, kc, vc, out, ldo, B, T, pos0, heads, kv_heads, d, Bc, b0, post_scale,
# starts (or NULL), stream
BLOCK_SIGNATURE = (ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
                   + [ctypes.c_int] * 9 + [ctypes.c_void_p, ctypes.c_void_p])

BLOCK_Q = (2, 3, 4, 5, 6, 7, 8, 12, 16)             # the instantiated slot counts (lia_attention.hip, block_q_of)
BLOCK_MAX_Q = 16
BLOCK_LDS = 160 * 1024
# every (G, T) whose G * T is an instantiated slot count, and two that run in the next larger one (slots without a query)
GT = [(G, T) for G in (1, 2, 4, 8) for T in range(2, 17) if G * T in BLOCK_Q] + [(1, 9), (2, 7)]
PASS = {128: 128, 64: 256, 32: 512}


def pos0_list(d):
    P = PASS[d]
    return (1, P - 3, P - 1, P, P + 1, 2 * P - 2, 1000)


CASES = [(fam, d, ps) for fam in F.FAMILIES for d in (32, 64, 128) for ps in (0, 1)]


def shape_of(i, G):
    """(B <= 3, heads <= 8, kv_heads) of sub-case i"""
    kvh = 1 if G == 8 else 2
    return 1 + i % 3, G * kvh, kvh


@pytest.fixture
def block(gpu):
    torch, launch = gpu
    from lia_amd import _native as N
    fn = N.lib().lia_attn_block_launch
    fn.restype, fn.argtypes = BLOCK_SIGNATURE
    assert BLOCK_SIGNATURE == SIGNATURES["lia_attn_append_launch"], "the block launch takes the append launch's argument list"
    return torch, launch


def run_block(gpu, q, kc, vc, pos0, heads, kvh, d, ps, starts=None):
    """q [B, T, H], caches [.., Bc = B + 2, kvh, d] through lia_attn_block_launch with the append test's plumbing, then every row t
    through the decode launch over pos0 + t + 1 keys.  -> (out [B, T, H], decode rows [B, T, H])"""
    torch, launch = gpu
    B, T, H = q.shape
    Bc = kc.shape[1]
    assert Bc == B + BC_EXTRA
    ldq, ldo = H + 16, H + 24
    qd = pitched(torch, dev(torch, q.reshape(B * T, H)), ldq, X_GAP)
    kd, vd = dev(torch, kc), dev(torch, vc)
    out = sentinel_buf(torch, (B * T + OUT_SLACK, ldo))
    st = None if starts is None else torch.from_numpy(np.asarray(starts, np.int32)).cuda()
    rc = launch("lia_attn_block_launch", qd, ldq, kd, vd, out, ldo, B, T, pos0, heads, kvh, d, Bc, B0, ps, st)
    assert rc == 0
    oh = host(out)
    assert (oh[:, H:] == SENTINEL).all(), "the launch wrote into the gap columns of out"
    assert (oh[B * T:] == SENTINEL).all(), "the launch wrote behind the last served row of out"
    assert (host(kd) == kc).all() and (host(vd) == vc).all(), "the launch changed the cache"
    dec = np.zeros((B, T, H), np.uint16)
    for t in range(T):
        o1 = sentinel_buf(torch, (B + OUT_SLACK, ldo))
        qt = qd.data_ptr() + 2 * t * ldq                       # row b * T + t at a pitch of T * ldq
        if starts is None:
            rc = launch("lia_attn_decode_launch", qt, T * ldq, kd, vd, o1, ldo, B, pos0 + t + 1, heads, kvh, d, Bc, B0, ps)
        else:
            rc = launch("lia_attn_decode_padded_launch", qt, T * ldq, kd, vd, o1, ldo, B, pos0 + t + 1, heads, kvh, d, Bc, B0, ps, st)
        assert rc == 0
        dec[:, t] = host(o1)[:B, :H]
    return oh[:B * T, :H].reshape(B, T, H), dec


@pytest.mark.gpu
@pytest.mark.parametrize("family,d,ps", CASES)
def test_block_families_and_decode_rows_bit_for_bit(block, family, d, ps):
    """every family x d x scaling, and inside every (G, T): unpadded and padded, pos0 and the batch taken in turn; the float64
    comparison of the attention tests (no new tolerance) and 0 outputs differing from the decode launch's rows"""
    i0 = CASES.index((family, d, ps))
    for j, (G, T) in enumerate(GT):
        i = 5 * i0 + 3 * j
        B, heads, kvh = shape_of(i, G)
        pos0 = pos0_list(d)[i % 7]
        for starts in (None, starts_for(B, pos0)):
            S = pos0 + T
            q, kc, vc = F.make(family, B, T, S, heads, kvh, d, ps, starts=starts, b0=B0, Bc=B + BC_EXTRA)
            got, dec = run_block(block, q, kc, vc, pos0, heads, kvh, d, ps, starts)
            what = f"block {family} d {d} post {ps} G {G} T {T} B {B} pos0 {pos0} starts {None if starts is None else starts.tolist()}"
            check_case(what, q, kc, vc, got, family, S, heads, kvh, ps, starts)
            assert (got == dec).all(), f"{what}: {(got != dec).sum()} of {got.size} outputs differ from the decode launch's rows"


@pytest.mark.gpu
@pytest.mark.parametrize("d", (32, 64, 128))
def test_every_pos0_at_every_slot_count(block, d):
    """the turns above, made whole: every pos0 of the list at every d for the smallest, a middle and the largest slot count, G 1 and
    G 4, on ramp (the maximum sits on the newest key: a limit one short or one long moves every row)"""
    for pos0 in pos0_list(d):
        for G, T in ((1, 2), (1, 5), (1, 8), (4, 4)):
            B, heads, kvh = shape_of(pos0 + T, G)
            for starts in (None, starts_for(B, pos0)):
                q, kc, vc = F.make("ramp", B, T, pos0 + T, heads, kvh, d, 1, starts=starts, b0=B0, Bc=B + BC_EXTRA)
                got, dec = run_block(block, q, kc, vc, pos0, heads, kvh, d, 1, starts)
                check_case(f"block ramp d {d} G {G} T {T} pos0 {pos0}", q, kc, vc, got, "ramp", pos0 + T, heads, kvh, 1, starts)
                assert (got == dec).all(), f"d {d} G {G} T {T} pos0 {pos0} starts {starts}: {(got != dec).sum()} outputs differ from decode"


@pytest.mark.gpu
def test_refusals_launch_nothing(block):
    """-1 and `out` untouched: a head_dim other than 32 / 64 / 128, heads not a multiple of kv_heads, more slots than the largest
    instantiated count, scores beyond the LDS, a block of one query, an empty cache"""
    torch, launch = block
    z = torch.zeros(4096, dtype=torch.int16, device="cuda")
    out = sentinel_buf(torch, (64, 1024))
    need = lambda Q, S, d: 4 * (Q * ((S + 3) // 4 * 4) + 4 * Q * d + 8 * Q)
    assert need(16, 2400 + 4, 128) > BLOCK_LDS >= need(8, 2400 + 2, 128)
    for B, T, pos0, heads, kvh, d in ((1, 2, 3, 1, 1, 48), (1, 2, 3, 3, 2, 64), (1, BLOCK_MAX_Q + 1, 3, 1, 1, 64), (1, 3, 3, 8, 1, 64),
                                      (1, 4, 2400, 4, 1, 128), (1, 1, 5, 1, 1, 64), (1, 2, 0, 1, 1, 64)):
        assert launch("lia_attn_block_launch", z, 1024, z, z, out, 1024, B, T, pos0, heads, kvh, d, 1, 0, 0, None) == -1
        assert (host(out) == SENTINEL).all()


def test_the_comparison_rejects_a_limit_off_by_one():
    """CPU: on ramp a block's rows pass the comparison against the right reference and are rejected against a mask shifted by one
    key either way -- what a per-slot limit one short or one long would compute"""
    B, T, pos0, heads, kvh, d, ps = 2, 4, 255, 4, 2, 64, 1
    S = pos0 + T
    q, kc, vc = F.make("ramp", B, T, S, heads, kvh, d, ps, b0=1, Bc=B + 2)
    got = emulate(q, kc, vc, S, heads, kvh, ps, b0=1, tile=None)
    ok, msg = family_verdict("ramp", got, F.reference(q, kc, vc, S, heads, kvh, ps, b0=1))
    assert ok, msg
    for name in ("mask_shift=+1", "mask_shift=-1"):
        with np.errstate(invalid="ignore"):
            ok, msg = family_verdict("ramp", got, F.reference(q, kc, vc, S, heads, kvh, ps, b0=1, **F.MUTANTS[name]))
        assert not ok, f"{name} passes: {msg}"


def test_cases_reach_every_slot_count_and_pos0():
    assert {G * T for G, T in GT if G * T in BLOCK_Q} == set(BLOCK_Q)
    assert {(1, T) for T in range(2, 9)} | {(4, T) for T in (2, 3, 4)} <= set(GT)
    assert len(CASES) == len(F.FAMILIES) * 6
    for d in (32, 64, 128):
        seen = {pos0_list(d)[(5 * CASES.index(c) + 3 * j) % 7] for c in CASES if c[1] == d for j in range(len(GT))}
        assert seen == set(pos0_list(d))
    assert all(shape_of(i, G)[0] <= 3 and shape_of(i, G)[1] <= 8 for i in range(9) for G in (1, 2, 4, 8))
