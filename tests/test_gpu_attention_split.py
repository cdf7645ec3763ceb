"""-m gpu: the split-key decode attention (lia_attn_decode_split_launch: a row's keys cut into chunks of C = lia_attn_split_chunk(d)
keys over workgroups, four launches) through its launcher, with test_gpu_attention_families.run_case's plumbing -- ldq / ldo > H
with NaN and sentinel gaps, b0 = 1 of Bc = B + 2, NaN in every cache row and batch row that must not be read, the cache unchanged,
the sentinels intact -- and the scratch filled with NaN bits before every launch (a read of a word the launch did not write itself
poisons the output).  The shapes are the smallest at which the route can go wrong, derived from C at run time: one key, one key
either side of a chunk boundary, two and three chunks with a tail, and one key past the one-workgroup kernel's LDS bound.

What is pinned: the float64 comparison of check_case (unchanged), bit-identity with the one-workgroup launch for S <= C, of a padded
row with its own unpadded launch on the shifted pointers, and of a row with its own B = 1 launch at another b0 / Bc."""
import ctypes

import numpy as np
import pytest

import attn_families as F
from test_gpu_attention_families import B0, BC_EXTRA, OUT_SLACK, check_case, dev
from test_gpu_kernel_variants import (ATTN_ATOL, ATTN_MIN_EXACT, ATTN_RTOL, DECODE_G, SENTINEL, X_GAP, check, decode_s_max, gpu, host,  # noqa: F401
                                      pitched, sentinel_buf)

pytestmark = pytest.mark.gpu

ATTN = dict(min_exact=ATTN_MIN_EXACT, bound=(ATTN_ATOL, ATTN_RTOL))
vp, ci, cl, cz = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_size_t
# q, ldq, kc, vc, out, ldo, B, S, heads, kv_heads, d, Bc, b0, post_scale, starts (or NULL), scratch, scratch_bytes, stream
SPLIT_SIGNATURE = (ci, [vp, cl, vp, vp, vp, cl] + [ci] * 8 + [vp, vp, cz, vp])
DS = (32, 64, 128)
PASS = {128: 128, 64: 256, 32: 512}          # U * KPP keys: one pass of the decode kernel's workgroup
S_KINDS = ("1", "C-1", "C", "C+1", "2C", "2C+1", "3C+77")
KVH = 2
SCRATCH_FILL = 0xff                           # every scratch byte before a launch: bf16 0xffff and fp32 0xffffffff are NaN
FAMILY_CASES = [(D, G, ps, kind) for D in DS for G in DECODE_G for ps in (0, 1) for kind in S_KINDS]


def family_of(i):
    return F.FAMILIES[i % len(F.FAMILIES)]


@pytest.fixture(scope="module")
def split(gpu):
    from lia_amd import _native as N
    lib = N.lib()
    lib.lia_attn_decode_split_launch.restype, lib.lia_attn_decode_split_launch.argtypes = SPLIT_SIGNATURE
    chunk = {d: lib.lia_attn_split_chunk(d) for d in DS}
    assert all(chunk[d] > 0 and chunk[d] % PASS[d] == 0 for d in DS), chunk
    return lib, chunk


def s_of(kind, C):
    return {"1": 1, "C-1": C - 1, "C": C, "C+1": C + 1, "2C": 2 * C, "2C+1": 2 * C + 1, "3C+77": 3 * C + 77}[kind]


def starts_for(S, C):
    """the starts of one padded batch: 0, 1, C - 1, C, C + 1 where they lie below S - 1, and S - 1"""
    return np.array(sorted({s for s in (0, 1, C - 1, C, C + 1) if s < S - 1} | {S - 1}), np.int32)


def scratch_for(gpu, split, B, S, heads, kvh, d, short=0):
    torch, _ = gpu
    need = split[0].lia_attn_split_scratch_bytes(B, S, heads, kvh, d)
    assert need > 0 and need % 256 == 0
    return torch.full((need - short,), SCRATCH_FILL, dtype=torch.uint8, device="cuda"), need - short


def launch_split(gpu, split, qd, ldq, kd, vd, B, S, heads, kvh, d, Bc, b0, ps, starts=None, want_rc=0):
    """one split launch into a fresh sentinel buffer -> out [B, H] (uint16); qd / kd / vd: tensors or raw device addresses"""
    torch, launch = gpu
    H = heads * d
    ldo = H + 24
    out = sentinel_buf(torch, (B + OUT_SLACK, ldo))
    scratch, nbytes = scratch_for(gpu, split, B, S, heads, kvh, d)
    st = None if starts is None else torch.from_numpy(np.asarray(starts, np.int32)).cuda()
    rc = launch("lia_attn_decode_split_launch", qd, ldq, kd, vd, out, ldo, B, S, heads, kvh, d, Bc, b0, ps, st, scratch, nbytes)
    assert rc == want_rc
    oh = host(out)
    assert (oh[:, H:] == SENTINEL).all(), "the launch wrote into the gap columns of out"
    assert (oh[B:] == SENTINEL).all(), "the launch wrote behind the last served row of out"
    return oh[:B, :H]


def run_split(gpu, split, family, B, S, heads, kvh, d, ps, starts=None, shifted=False):
    """the family's decode case through the split launcher -> (q, kc, vc, out [B, 1, H], (qd, ldq, kd, vd, Bc)).  shifted: every row
    once more alone, UNPADDED, on its own shifted sequence (K / V pointers moved to the row's start), bit for bit the padded row"""
    torch, _ = gpu
    Bc, H = B + BC_EXTRA, heads * d
    ldq = H + 16
    q, kc, vc = F.make(family, B, 1, S, heads, kvh, d, ps, starts=starts, b0=B0, Bc=Bc)
    qd = pitched(torch, dev(torch, q.reshape(B, H)), ldq, X_GAP)
    kd, vd = dev(torch, kc), dev(torch, vc)
    got = launch_split(gpu, split, qd, ldq, kd, vd, B, S, heads, kvh, d, Bc, B0, ps, starts)
    assert (host(kd) == kc).all() and (host(vd) == vc).all(), "the launch changed the cache"
    if shifted:
        kv_row = Bc * kvh * d
        for b, s in enumerate(starts):
            s = int(s)
            o1 = launch_split(gpu, split, qd.data_ptr() + 2 * b * ldq, ldq, kd.data_ptr() + 2 * s * kv_row, vd.data_ptr() + 2 * s * kv_row,
                              1, S - s, heads, kvh, d, Bc, B0 + b, ps)
            assert (o1[0] == got[b]).all(), f"row {b} (start {s}) differs from its own unpadded launch"
    return q, kc, vc, got.reshape(B, 1, H), (qd, ldq, kd, vd, Bc)


def run_decode(gpu, handles, B, S, heads, kvh, d, ps, starts=None, want_rc=0):
    """the one-workgroup launch on the same device buffers -> out [B, H], or None where it refuses (nothing written)"""
    torch, launch = gpu
    qd, ldq, kd, vd, Bc = handles
    H = heads * d
    ldo = H + 24
    out = sentinel_buf(torch, (B + OUT_SLACK, ldo))
    if starts is None:
        rc = launch("lia_attn_decode_launch", qd, ldq, kd, vd, out, ldo, B, S, heads, kvh, d, Bc, B0, ps)
    else:
        rc = launch("lia_attn_decode_padded_launch", qd, ldq, kd, vd, out, ldo, B, S, heads, kvh, d, Bc, B0, ps,
                    torch.from_numpy(np.asarray(starts, np.int32)).cuda())
    assert rc == want_rc
    oh = host(out)
    if rc:
        assert (oh == SENTINEL).all(), "a refused launch wrote"
        return None
    assert (oh[:, H:] == SENTINEL).all() and (oh[B:] == SENTINEL).all()
    return oh[:B, :H]


@pytest.mark.parametrize("D,G,ps,kind", FAMILY_CASES)
def test_split_families(gpu, split, D, G, ps, kind):
    """every <D, G> x both scalings x S in 1, C - 1, C, C + 1, 2C, 2C + 1, 3C + 77, the families taken in turn, B = 3, kv_heads = 2,
    against attn_families.reference under check_case; then the padded form at the same S, the starts of one batch mixing 0, 1,
    C - 1, C, C + 1 and S - 1 (pad K rows would outscore every real key, their V rows are NaN), every row equal to its own unpadded
    launch on the shifted pointers bit for bit.
    Measured on the MI355X: unpadded >= 99.935 % bit-identical (<32, 8> post_scale 1 exact S 1025), padded >= 99.967 %, max 0.016
    quantum; every `hot` case 100 % bit-identical; sink rows bit for bit; every padded row equal to its own launch."""
    C = split[1][D]
    S = s_of(kind, C)
    family = family_of(FAMILY_CASES.index((D, G, ps, kind)))
    heads = G * KVH
    q, kc, vc, got, _ = run_split(gpu, split, family, 3, S, heads, KVH, D, ps)
    check_case(f"split <{D}, {G}> post {ps} {family} S {S}", q, kc, vc, got, family, S, heads, KVH, ps)
    starts = starts_for(S, C)
    q, kc, vc, got, _ = run_split(gpu, split, family, len(starts), S, heads, KVH, D, ps, starts=starts, shifted=True)
    check_case(f"padded split <{D}, {G}> post {ps} {family} S {S}", q, kc, vc, got, family, S, heads, KVH, ps, starts)


def test_family_cases_take_every_family_at_every_shape_class():
    """every family meets every S kind, every d and every G somewhere in the list (the stride of the enumeration is coprime to 6)"""
    seen = {(family_of(i), kind) for i, (_, _, _, kind) in enumerate(FAMILY_CASES)}
    assert seen == {(f, k) for f in F.FAMILIES for k in S_KINDS}
    assert {(family_of(i), D) for i, (D, _, _, _) in enumerate(FAMILY_CASES)} == {(f, D) for f in F.FAMILIES for D in DS}
    assert {(family_of(i), G) for i, (_, G, _, _) in enumerate(FAMILY_CASES)} == {(f, G) for f in F.FAMILIES for G in DECODE_G}


@pytest.mark.parametrize("ps", (0, 1))
@pytest.mark.parametrize("G", DECODE_G)
@pytest.mark.parametrize("D", DS)
def test_one_chunk_is_the_one_workgroup_launch(gpu, split, D, G, ps):
    """S <= C: the split launch equals lia_attn_decode_launch bit for bit -- same key-to-thread assignment and fold order inside the
    chunk, and a combine that adds nothing to one partial.  S = C (full passes only), C - 1 and 77 (a tail pass), `hot` and `exact`;
    and the padded launches of rows that keep at most C keys."""
    C = split[1][D]
    heads = G * KVH
    for family, S in (("hot", C), ("exact", C - 1), ("hot", 77)):
        q, kc, vc, got, h = run_split(gpu, split, family, 3, S, heads, KVH, D, ps)
        one = run_decode(gpu, h, 3, S, heads, KVH, D, ps)
        assert (got[:, 0] == one).all(), f"<{D}, {G}> post {ps} {family} S {S}: {(got[:, 0] != one).sum()} outputs differ"
    S = C + 40
    starts = np.array([40, 41, C, S - 1], np.int32)
    q, kc, vc, got, h = run_split(gpu, split, "hot", len(starts), S, heads, KVH, D, ps, starts=starts)
    one = run_decode(gpu, h, len(starts), S, heads, KVH, D, ps, starts=starts)
    assert (got[:, 0] == one).all(), f"padded <{D}, {G}> post {ps} S {S}: {(got[:, 0] != one).sum()} outputs differ"


@pytest.mark.parametrize("G", DECODE_G)
@pytest.mark.parametrize("D", DS)
def test_a_row_depends_on_nothing_but_itself(gpu, split, D, G):
    """S = 2C + 1: row b of a B = 3 launch equals the B = 1 launch of that row at b0 = 1 + b of the same cache, and the B = 1 launch
    at b0 = 0 of a cache that holds this row alone (Bc = 1), bit for bit"""
    torch, _ = gpu
    C = split[1][D]
    S, heads, ps = 2 * C + 1, G * KVH, G % 2
    q, kc, vc, got, (qd, ldq, kd, vd, Bc) = run_split(gpu, split, "hot", 3, S, heads, KVH, D, ps)
    for b in range(3):
        one = launch_split(gpu, split, qd.data_ptr() + 2 * b * ldq, ldq, kd, vd, 1, S, heads, KVH, D, Bc, B0 + b, ps)
        assert (one[0] == got[b, 0]).all(), f"row {b}: differs from its B = 1 launch at b0 = {B0 + b}"
        k1, v1 = dev(torch, kc[:, B0 + b:B0 + b + 1]), dev(torch, vc[:, B0 + b:B0 + b + 1])
        one = launch_split(gpu, split, qd.data_ptr() + 2 * b * ldq, ldq, k1, v1, 1, S, heads, KVH, D, 1, 0, ps)
        assert (one[0] == got[b, 0]).all(), f"row {b}: differs from its B = 1 launch on a cache of its own"


@pytest.mark.parametrize("G", DECODE_G)
@pytest.mark.parametrize("D", DS)
def test_ramp_past_the_lds_bound(gpu, split, D, G):
    """`ramp` one key past the largest S the one-workgroup launcher accepts at <D, G> (S 4601 .. 40825), B = 2 unpadded and B = 3
    padded (starts 65, S - 1, 0): lia_attn_decode_launch returns -1 and writes nothing, the split launch returns 0 and its output
    is inside check_case's comparison.
    Measured: all 24 cases 100 % bit-identical to the float64 reference's rounding."""
    S = decode_s_max(D, G) + 1
    q, kc, vc, got, h = run_split(gpu, split, "ramp", 2, S, G, 1, D, 1)
    assert run_decode(gpu, h, 2, S, G, 1, D, 1, want_rc=-1) is None
    check_case(f"split <{D}, {G}> ramp past the LDS bound S {S}", q, kc, vc, got, "ramp", S, G, 1, 1)
    starts = np.array([65, S - 1, 0], np.int32)
    q, kc, vc, got, h = run_split(gpu, split, "ramp", 3, S, G, 1, D, 0, starts=starts)
    assert run_decode(gpu, h, 3, S, G, 1, D, 0, starts=starts, want_rc=-1) is None
    check_case(f"padded split <{D}, {G}> ramp past the LDS bound S {S}", q, kc, vc, got, "ramp", S, G, 1, 0, starts)


@pytest.mark.parametrize("kind", ("1037", "2C+1"))
@pytest.mark.parametrize("G", DECODE_G)
@pytest.mark.parametrize("D", DS)
def test_split_against_the_one_workgroup_launch(gpu, split, D, G, kind):
    """S = 1037 and 2C + 1, the families in turn: the file's attention comparison with the one-workgroup launch's output in the
    reference's place -- the two differ in the fp32 order of the P.V sum only.
    Measured: 0 % of the outputs differ in all 24 cases (largest distance 0 quanta); on tools/attn_split_bench's random K / V 0 - 32
    of 4096 - 65536 outputs differ (<= 0.05 %, results/attn_split_bench.txt)."""
    C = split[1][D]
    S = 1037 if kind == "1037" else 2 * C + 1
    i = (DS.index(D) * len(DECODE_G) + DECODE_G.index(G)) * 2 + (kind != "1037")
    family, ps, heads = family_of(i), i % 2, G * KVH
    q, kc, vc, got, h = run_split(gpu, split, family, 3, S, heads, KVH, D, ps)
    one = run_decode(gpu, h, 3, S, heads, KVH, D, ps)
    check(f"split vs one workgroup <{D}, {G}> post {ps} {family} S {S}", got[:, 0], one, **ATTN)


def test_refusals(gpu, split):
    """scratch one byte short, G = 3, d = 96, S = 0: -1, and neither out nor the scratch is written"""
    torch, launch = gpu
    D, heads, kvh, B = 64, 4, 2, 2
    S = 2 * split[1][D] + 1
    Bc, H = B + BC_EXTRA, heads * D
    q, kc, vc = F.make("exact", B, 1, S, heads, kvh, D, 0, b0=B0, Bc=Bc)
    qd, kd, vd = dev(torch, q.reshape(B, H)), dev(torch, kc), dev(torch, vc)
    need = split[0].lia_attn_split_scratch_bytes(B, S, heads, kvh, D)
    for what, (hh, kk, dd, ss, nbytes) in {"scratch one byte short": (heads, kvh, D, S, need - 1), "G = 3": (6, 2, D, S, need),
                                           "d = 96": (heads, kvh, 96, S, need), "S = 0": (heads, kvh, D, 0, need)}.items():
        out = sentinel_buf(torch, (B, H))
        scratch = torch.full((need,), SCRATCH_FILL, dtype=torch.uint8, device="cuda")
        rc = launch("lia_attn_decode_split_launch", qd, H, kd, vd, out, H, B, ss, hh, kk, dd, Bc, B0, 0, None, scratch, nbytes)
        assert rc == -1, what
        assert (host(out) == SENTINEL).all() and bool((scratch == SCRATCH_FILL).all()), f"{what}: the refused launch wrote"
    out = sentinel_buf(torch, (B, H))
    scratch = torch.full((need,), SCRATCH_FILL, dtype=torch.uint8, device="cuda")
    assert launch("lia_attn_decode_split_launch", qd, H, kd, vd, out, H, B, S, heads, kvh, D, Bc, B0, 0, None, scratch, need) == 0
    assert not (host(out) == SENTINEL).all()
