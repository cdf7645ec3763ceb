"""-m gpu: every kernel the hot-path launchers dispatch to, called through its exported extern "C" launcher, against the float64
references of f64_ref.py (absolute bounds: never another GPU route).

The launchers pick a kernel from the shape.  The thresholds below restate those choices, with the launcher line they come from;
test_cases_reach_every_variant checks that the case lists reach each kernel, and the shapes on both sides of every threshold.

Bounds (f64_ref.quantum: one bf16 quantum at the largest |reference| output):
  norms, attention   no output further than one quantum of the largest, and a minimum bit-identical fraction; attention also
                     keeps test_gpu_ops.test_attention_prefill's 0.02 + 0.016 |ref| per element
  RoPE, argmax       bit-exact (RoPE's products of two bf16 are exact in fp32, its sum is rounded once)
  SiLU * up          at most 1 bf16 ulp per element (v_exp_f32 / v_rcp_f32 are 1-ulp approximations)
Each test's docstring records the margins measured on the MI355X.
"""
import ctypes

import numpy as np
import pytest

import f64_ref as R
import launchers

pytestmark = pytest.mark.gpu

# ---- dispatch thresholds of the launchers ---------------------------------------------------------------------------------
ROW_THREADS = 1024                  # LIA_ROW_THREADS, lia_common.h
ROW_NORM_MAX_ROWS = 1024            # rows <= this: one workgroup per row (lia_elementwise.hip:144, lia_llama.hip:100)
ROW_NORM_MAX_PIECES = 2 * ROW_THREADS   # ... while H / 8 <= this; row<1> up to ROW_THREADS pieces (lia_elementwise.hip:149-151)
LN_REG = (4, 8, 14, 24)             # reg<N> while ceil(H / 512) <= N, else the plain kernel (lia_elementwise.hip:156-161)
RMS_REG = (4, 8, 16)                # (lia_llama.hip:108-112)
ROPE_VEC_D, ROPE_VEC_STRIDE = 16, 8     # the vector kernel needs d % 16 == 0 and row_stride % 8 == 0 (lia_llama.hip:171)
SILU_MAX_BLOCKS = 4096              # grid of at most this many 256-thread blocks, grid-stride beyond (lia_llama.hip:205-207)
GU_BLOCK = 32                       # LIA_GU_BLOCK, lia_common.h
ATTN_QBLOCK = 128                   # query rows per block of the prefill kernels (lia_attention.hip:1055)
XCD_GROUPS = 8                      # B * kv_heads % 8 == 0 or >= 64: the XCD-aware order (lia_attention.hip:1040)
XCD_MANY_GROUPS = 64
DECODE_LDS = 160 * 1024             # decode's LDS need (G Spad + 4 G D + 8 G) floats must fit (lia_attention.hip:1136-1137)
DECODE_G = (1, 2, 4, 8)             # the instantiated group sizes (lia_attention.hip:1148-1154)
ARGMAX_VEC = 8                      # vocab % 8 == 0: 16-byte loads, else the scalar loop (lia_elementwise.hip:202)

# ---- bounds (see the module docstring; margins measured in the docstrings) --------------------------------------------------
NORM_MIN_EXACT = 0.995
NORM_OFFSET_MIN_EXACT = 0.98     # rows of mean 256: the fp32 mean itself is rounded (ulp 2^-15 of the spread)
ATTN_MIN_EXACT = 0.95
ATTN_ATOL, ATTN_RTOL = 0.02, 0.016  # test_gpu_ops.test_attention_prefill
SILU_MAX_ULP = 1

SENTINEL = 0x5a5a                   # fill of every output word a launch must not write
X_GAP = 0x7fc0                      # NaN in the pitch gap of an input: a read of it would poison the row


def norm_kernel(kind, rows, H):
    """the kernel lia_layernorm_launch / lia_rmsnorm_launch runs for (rows, H)"""
    if rows <= ROW_NORM_MAX_ROWS and H % 8 == 0 and H // 8 <= ROW_NORM_MAX_PIECES:
        return "row<1>" if H // 8 <= ROW_THREADS else "row<2>"
    nvl = -(-(H // 8) // 64)
    for n in (LN_REG if kind == "layernorm" else RMS_REG):
        if nvl <= n:
            return f"reg<{n}>"
    return "plain"


def prefill_variant(B, T, kvh, d):
    if d != 128:
        return f"generic<{d}>"
    g = B * kvh
    order = "xcd" if g % XCD_GROUPS == 0 else ("xcd-padded" if g >= XCD_MANY_GROUPS else "r05")
    return f"128/{order}"


def decode_s_max(D, G):
    """the largest S lia_attn_decode_launch accepts at <D, G>: Spad = S rounded up to 4 must keep the LDS need in bounds"""
    return ((DECODE_LDS // 4 - 4 * G * D - 8 * G) // G) & ~3


# ---- plumbing ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from lia_amd import _native as N, ops
    lib = launchers.bind(N.lib())
    ctx = ops.Context(0, 1 << 20)

    def launch(name, *args):
        torch.cuda.synchronize()            # torch filled the buffers on ITS stream; the kernel runs on the context's
        rc = getattr(lib, name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], ctypes.c_void_p(ctx.stream))
        ctx.synchronize()
        return rc

    yield torch, launch
    ctx.close()


def host(t):
    """a device int16 tensor of bf16 bits -> numpy uint16"""
    return t.cpu().numpy().view(np.uint16)


def dev_randn(torch, seed, shape, scale=1.0, mean=0.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (mean + scale * torch.randn(shape, generator=g, device="cuda")).to(torch.bfloat16).view(torch.int16)


def pitched(torch, vals, ld, fill):
    """rows of `vals` (int16 [rows, n]) in a buffer of row pitch ld, the gap columns set to `fill`"""
    buf = torch.full((vals.shape[0], ld), fill - 65536 if fill >= 32768 else fill, dtype=torch.int16, device="cuda")
    buf[:, :vals.shape[1]] = vals
    return buf


def sentinel_buf(torch, shape):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device="cuda")


def verdict(got, ref, min_exact=None, bound=None, max_ulp=None):
    """(ok, message): the per-op comparisons of this file, without asserting, so that the mutant test can use them too"""
    a, b = R.f64(got), R.f64(ref)
    top = float(np.abs(b[np.isfinite(b)]).max()) if np.isfinite(b).any() else 0.0
    q = R.quantum(max(top, 2.0 ** -126))
    err = np.abs(a - b)
    err = np.where(np.isnan(err), np.where(np.isnan(a) & np.isnan(b), 0.0, np.inf), err)
    worst = float(err.max()) if err.size else 0.0
    frac = float((got == ref).mean()) if got.size else 1.0
    ulp = int(R.ulp_distance(got, ref).max()) if got.size else 0
    msg = f"{100 * frac:.3f} % bit-identical, max |err| {worst:.3g} = {worst / q:.3f} quanta of max |ref| {top:.3g}, max {ulp} ulp"
    ok = True
    if max_ulp is not None:
        ok &= ulp <= max_ulp
    else:
        ok &= worst <= q
    if min_exact is not None:
        ok &= frac >= min_exact
    if bound is not None:
        ok &= bool((err <= bound[0] + bound[1] * np.abs(b)).all())
    return bool(ok), msg


def check(what, got, ref, **kw):
    ok, msg = verdict(got, ref, **kw)
    print(f"\n{what}: {msg}")
    assert ok, f"{what}: {msg} ({kw})"


# ---- norms -------------------------------------------------------------------------------------------------------------------
NORM_H = (768, 2048, 2056, 4096, 4104, 7168, 7176, 8192, 8200, 12288, 12296, 16384, 16392)
NORM_CASES = ([(rows, H, 1.0, 0.0) for rows in (1, ROW_NORM_MAX_ROWS, ROW_NORM_MAX_ROWS + 1) for H in NORM_H]
              + [(4097, H, 1.0, 0.0) for H in (768, 4104, 16392)]
              + [(1024, 4096, 1e-3, 0.0), (1025, 7168, 1e-3, 0.0), (1, 16392, 1e-3, 0.0), (1024, 8200, 300.0, 0.0),
                 (1025, 12296, 300.0, 0.0), (4097, 2048, 300.0, 0.0)])
LN_OFFSET_CASES = [(1, 768, 0.5, 256.0), (1024, 8192, 0.5, 256.0), (1025, 4104, 0.5, 256.0), (1025, 12296, 0.5, 256.0)]


def run_norm(gpu, kind, rows, H, scale, mean, seed=1):
    torch, launch = gpu
    ldx, ldy = H + 24, H + 40
    x = pitched(torch, dev_randn(torch, seed, (rows, H), scale, mean), ldx, X_GAP)
    w = dev_randn(torch, seed + 1, (H,), 0.3, 1.0)
    b = dev_randn(torch, seed + 2, (H,), 0.5)
    y = sentinel_buf(torch, (rows, ldy))
    if kind == "layernorm":
        launch("lia_layernorm_launch", x, ldx, w, b, y, ldy, rows, H, 1e-5)
    else:
        launch("lia_rmsnorm_launch", x, ldx, w, y, ldy, rows, H, 1e-5)
    yh = host(y)
    assert (yh[:, H:] == SENTINEL).all(), "the launch wrote into the gap columns of y"
    return host(x)[:, :H], host(w), host(b), yh[:, :H]


@pytest.mark.parametrize("rows,H,scale,mean", NORM_CASES + LN_OFFSET_CASES)
def test_layernorm_variants(gpu, rows, H, scale, mean):
    """lia_layernorm_launch (row<1>, row<2>, reg<4|8|14|24>, plain) against float64, rows pitched (ldx, ldy > H), N(mean, scale)
    inputs; mean 256 with spread 0.5 is what a one-pass variance would lose.
    Measured: >= 99.986 % bit-identical (mean-256 rows: >= 98.82 %, the fp32 mean's own rounding), max 0.5 quantum."""
    x, g, b, y = run_norm(gpu, "layernorm", rows, H, scale, mean)
    check(f"layernorm {norm_kernel('layernorm', rows, H)} {rows}x{H} N({mean}, {scale})", y, R.layernorm(x, g, b),
          min_exact=NORM_OFFSET_MIN_EXACT if mean else NORM_MIN_EXACT)


@pytest.mark.parametrize("rows,H,scale,mean", NORM_CASES)
def test_rmsnorm_variants(gpu, rows, H, scale, mean):
    """lia_rmsnorm_launch (row<1>, row<2>, reg<4|8|16>, plain) against float64, rows pitched, N(0, scale) inputs.
    Measured: >= 99.997 % bit-identical, max 0.5 quantum."""
    x, w, _, y = run_norm(gpu, "rmsnorm", rows, H, scale, mean)
    check(f"rmsnorm {norm_kernel('rmsnorm', rows, H)} {rows}x{H} N(0, {scale})", y, R.rmsnorm(x, w), min_exact=NORM_MIN_EXACT)


# ---- RoPE --------------------------------------------------------------------------------------------------------------------
ROPE_MAX_POS, ROPE_T, ROPE_B, ROPE_BC = 160, 37, 3, 5
ROPE_MAPS = ("q", "cache", "minibatch")
ROPE_CASES = ([(d, heads, m, 8) for d in (64, 128) for heads in (1, 8, 40) for m in ROPE_MAPS]          # vector kernel
              + [(8, 8, "q", 8), (24, 3, "cache", 8)]                                                   # scalar: d % 16 != 0
              + [(64, 8, m, 4) for m in ROPE_MAPS] + [(128, 1, "q", 2)])                                # scalar: stride % 8 != 0


def rope_map(m):
    """(rows, pos0, pos_mod, pos_div) of the three position maps lia_llama_layer_forward uses (lia_layer.hip, the RoPE launches):
    q rows b*T + t; cache rows t*Bc + b; one minibatch's rows of one cache position (pos_div = Bc + B)"""
    if m == "q":
        return ROPE_B * ROPE_T, ROPE_MAX_POS - ROPE_T, ROPE_T, 0
    if m == "cache":
        return ROPE_T * ROPE_BC, ROPE_MAX_POS - ROPE_T, 0, ROPE_BC
    return ROPE_B, ROPE_MAX_POS - 1, 0, ROPE_BC + ROPE_B


def run_rope(gpu, d, heads, m, pad, seed=3):
    from lia_amd.llama import rope_tables
    torch, launch = gpu
    rows, pos0, pos_mod, pos_div = rope_map(m)
    stride = heads * d + pad
    ct, st = (t.view(torch.int16) for t in rope_tables(ROPE_MAX_POS, d, 500000.0))
    cosb, sinb = host(ct), host(st)
    x = pitched(torch, dev_randn(torch, seed, (rows, heads * d), 2.0), stride, SENTINEL)
    x0 = host(x)
    launch("lia_rope_launch", x, stride, ct, st, rows, heads, d, pos0, pos_mod, pos_div)
    xh = host(x)
    assert (xh[:, heads * d:] == SENTINEL).all(), "the launch wrote into the gap columns"
    r = np.arange(rows)
    pos = pos0 + (r % pos_mod if pos_mod else r // pos_div)
    assert pos.max() == ROPE_MAX_POS - 1            # the last table row is read
    return x0[:, :heads * d], xh[:, :heads * d], cosb, sinb, pos


@pytest.mark.parametrize("d,heads,m,pad", ROPE_CASES)
def test_rope_variants(gpu, d, heads, m, pad):
    """lia_rope_launch (rope_vec_kernel, rope_kernel) at the three position maps up to the last table row: bit-exact.
    Measured: 100 % bit-identical."""
    x, got, cosb, sinb, pos = run_rope(gpu, d, heads, m, pad)
    kern = "vec" if d % ROPE_VEC_D == 0 and (heads * d + pad) % ROPE_VEC_STRIDE == 0 else "scalar"
    check(f"rope {kern} d {d} heads {heads} map {m}", got, R.rope(x, cosb, sinb, pos, heads), min_exact=1.0)


# ---- SiLU * up ---------------------------------------------------------------------------------------------------------------
SILU_CASES = [(1, 14336, 0, "normal"), (64, 14336, GU_BLOCK, "normal"), (7, 8 * 7, 0, "normal"), (3, 8 * 1793, 0, "normal"),
              (2048, 4096, 0, "normal"),          # M F / 8 = 4096 x 256 exactly: one element per thread
              (2049, 4096, GU_BLOCK, "normal"),   # just over: the grid-stride loop
              (2048, 14336, GU_BLOCK, "normal"), (256, 4096, GU_BLOCK, "span90"), (255, 8 * 37, 0, "span90")]


def run_silu(gpu, M, F, gu_block, dist, seed=5):
    torch, launch = gpu
    if dist == "span90":        # g across where exp2(-g log2 e) overflows and its reciprocal goes subnormal
        gen = torch.Generator(device="cuda").manual_seed(seed)
        gu = (180.0 * torch.rand((M, 2 * F), generator=gen, device="cuda") - 90.0).to(torch.bfloat16).view(torch.int16)
    else:
        gu = dev_randn(torch, seed, (M, 2 * F), 4.0)
    out = sentinel_buf(torch, (M, F))
    launch("lia_silu_mul_launch", gu, out, M, F, gu_block)
    return host(gu), host(out)


@pytest.mark.parametrize("M,F,gu_block,dist", SILU_CASES)
def test_silu_mul_variants(gpu, M, F, gu_block, dist):
    """lia_silu_mul_launch, both column layouts, one pass and grid-stride: at most 1 ulp from float64 per element.
    Measured (with lia_silu's accurate form): 100 % bit-identical, gates across +-90 included."""
    gu, got = run_silu(gpu, M, F, gu_block, dist)
    g, u = R.split_gate_up(gu, F, gu_block)
    ref = R.silu_mul(g, u)
    far = R.ulp_distance(got, ref) > SILU_MAX_ULP
    if far.any():
        print(f"\n{far.sum()} outputs more than {SILU_MAX_ULP} ulp away, gate in [{R.f64(g)[far].min()}, {R.f64(g)[far].max()}]")
    check(f"silu*up {M}x{F} block {gu_block} {dist}", got, ref, max_ulp=SILU_MAX_ULP)


def test_silu_rounding_of_every_bf16_gate(gpu):
    """Regression: bf16(silu(g)) for every finite bf16 gate (up = 1, so the output IS that rounding) equals float64's, bit for bit.
    The hardware exp2 / reciprocal form it replaced rounded g = 5.9375 to 5.9375 instead of 5.90625 (its silu, 5.92187444, is
    0.18 fp32 ulp below the neighbour of the bf16 tie), 2 ulp off after the product for 0.1 % of N(0, 4) gates, and returned 0
    for g <= -87.5, where silu(g) is a normal bf16 of ~1e-37."""
    torch, launch = gpu
    g = np.arange(65536, dtype=np.uint16)
    g = g[np.isfinite(R.f64(g))]
    F = -(-g.size // 8) * 8
    g = np.concatenate([g, np.zeros(F - g.size, np.uint16)])
    gu = np.concatenate([g, np.full(F, 0x3f80, np.uint16)])[None, :]         # [gate | up = 1.0]
    out = sentinel_buf(torch, (1, F))
    launch("lia_silu_mul_launch", torch.from_numpy(gu.view(np.int16)).cuda(), out, 1, F, 0)
    got, ref = host(out)[0], R.silu_mul(g, gu[0, F:])
    bad = got != ref
    assert not bad.any(), f"{bad.sum()} gates rounded differently, e.g. {list(zip(R.f64(g)[bad][:8], R.f64(got)[bad][:8], R.f64(ref)[bad][:8]))}"


# ---- attention ---------------------------------------------------------------------------------------------------------------
T_SWEEP = (2, 64, 65, 127, 128, 129, 256, 257, 385, 513, 641)     # query blocks of 128: 1 .. 6, odd counts pair the middle with itself
PREFILL_CASES = ([(1, T, 8, 2, 128, 1) for T in T_SWEEP]                                           # r05 order, G 4 (Llama)
                 + [(2, 257 if ps else 129, 2 * G, 2, d, ps) for d in (32, 64, 128) for G in DECODE_G for ps in (0, 1)]
                 + [(4, T, 8, 2, 128, 1) for T in (64, 385, 641)]                                  # XCD order, 8 groups
                 + [(13, 70, 5, 5, 128, 0), (13, 129, 10, 5, 128, 1), (65, 65, 8, 1, 128, 1)]       # 65 groups: padded XCD grid
                 + [(3, 200, 6, 3, 128, 0)]                                                         # 9 groups: r05 order
                 + [(1, T, 4, 2, 64, 1) for T in (2, 127, 128, 513)] + [(2, T, 2, 1, 32, 0) for T in (65, 385)])
KEY_SENTINEL, VAL_SENTINEL = 0x4280, 0x4580       # 64.0 and 4096.0: a read of a cache row outside the slice would show


def attn_buffers(torch, seed, B, T, S, heads, kvh, d, Bc, b0):
    H = heads * d
    q = pitched(torch, dev_randn(torch, seed, (B * T, H), 1.5), H + 16, X_GAP)
    kc = torch.full((S + 3, Bc, kvh, d), KEY_SENTINEL, dtype=torch.int16, device="cuda")
    vc = torch.full((S + 3, Bc, kvh, d), VAL_SENTINEL, dtype=torch.int16, device="cuda")
    kc[:S, b0:b0 + B] = dev_randn(torch, seed + 1, (S, B, kvh, d), 1.5)
    vc[:S, b0:b0 + B] = dev_randn(torch, seed + 2, (S, B, kvh, d))
    out = sentinel_buf(torch, (B * T, H + 24))
    return q, kc, vc, out


def run_attention(gpu, B, T, S, heads, kvh, d, ps, seed=7):
    """T > 1: the prefill launcher (S = T); T == 1: the decode launcher.  b0 = 1 of Bc = B + 2 cache batch rows."""
    torch, launch = gpu
    Bc, b0, H = B + 2, 1, heads * d
    q, kc, vc, out = attn_buffers(torch, seed, B, T, S, heads, kvh, d, Bc, b0)
    k0, v0 = host(kc), host(vc)
    if T > 1:
        rc = launch("lia_attn_prefill_launch", q, H + 16, kc, vc, out, H + 24, B, T, heads, kvh, d, Bc, b0, ps)
    else:
        rc = launch("lia_attn_decode_launch", q, H + 16, kc, vc, out, H + 24, B, S, heads, kvh, d, Bc, b0, ps)
    assert rc == 0
    oh = host(out)
    assert (oh[:, H:] == SENTINEL).all(), "the launch wrote into the gap columns of out"
    assert (host(kc) == k0).all() and (host(vc) == v0).all()
    qh = host(q)[:, :H].reshape(B, T, H)
    return qh, k0, v0, oh[:, :H].reshape(B, T, H), b0


def check_attention(what, got, ref, **kw):
    check(what, got, ref, min_exact=ATTN_MIN_EXACT, bound=(ATTN_ATOL, ATTN_RTOL), **kw)


@pytest.mark.parametrize("B,T,heads,kvh,d,ps", PREFILL_CASES)
def test_attention_prefill_variants(gpu, B, T, heads, kvh, d, ps):
    """lia_attn_prefill_launch: d 128 (r05 / XCD / padded XCD grid orders, paired mirror blocks, POST_SCALE 0 / 1) and the generic
    d 32 / 64 kernel, grouped heads G 1 .. 8, b0 > 0 of Bc > B, ldq / ldo > H, sentinel cache rows outside the slice.
    Measured: >= 99.94 % bit-identical, max 1.0 quantum (a one-ulp flip at |ref| ~3.9, padded XCD grid)."""
    q, kc, vc, got, b0 = run_attention(gpu, B, T, T, heads, kvh, d, ps)
    check_attention(f"prefill {prefill_variant(B, T, kvh, d)} B {B} T {T} heads {heads}/{kvh} d {d} post {ps}", got,
                    R.attention(q, kc, vc, T, heads, kvh, ps, b0=b0))


DECODE_S = (1, 2, 63, 64, 65, 1037)


@pytest.mark.parametrize("S", DECODE_S)
@pytest.mark.parametrize("ps", (0, 1))
@pytest.mark.parametrize("G", DECODE_G)
@pytest.mark.parametrize("D", (32, 64, 128))
def test_attention_decode_variants(gpu, D, G, ps, S):
    """lia_attn_decode_kernel<D, G> x post_scale, b0 > 0 of Bc > B, ldq / ldo > H.
    Measured: >= 96.875 % bit-identical (12 of 384 outputs at <32, 2> S 63), max 0.5 quantum."""
    kvh = 2
    q, kc, vc, got, b0 = run_attention(gpu, 3, 1, S, G * kvh, kvh, D, ps)
    check_attention(f"decode <{D}, {G}> post {ps} S {S}", got, R.attention(q, kc, vc, S, G * kvh, kvh, ps, b0=b0))


@pytest.mark.parametrize("G", DECODE_G)
@pytest.mark.parametrize("D", (32, 64, 128))
def test_attention_decode_lds_bound(gpu, D, G):
    """At the largest S whose scores fit the 160 KiB of LDS the decode result is right; one key more (the next Spad) is refused
    before any launch, and the output stays untouched.  Measured: 100 % bit-identical at the bound."""
    torch, launch = gpu
    S = decode_s_max(D, G)
    q, kc, vc, got, b0 = run_attention(gpu, 1, 1, S, G, 1, D, 1)
    check_attention(f"decode <{D}, {G}> at the LDS bound S {S}", got, R.attention(q, kc, vc, S, G, 1, 1, b0=b0))
    q, kc, vc, out = attn_buffers(torch, 11, 1, 1, S + 1, G, 1, D, 2, 1)
    assert launch("lia_attn_decode_launch", q, G * D + 16, kc, vc, out, G * D + 24, 1, S + 1, G, 1, D, 2, 1, 1) == -1
    assert (host(out) == SENTINEL).all()


@pytest.mark.parametrize("heads,kvh", [(3, 1), (6, 2), (16, 1), (32, 2), (5, 2)])
def test_attention_decode_refuses_other_groups(gpu, heads, kvh):
    """G not in {1, 2, 4, 8} (and heads not a multiple of kv_heads) is refused before any launch."""
    torch, launch = gpu
    q, kc, vc, out = attn_buffers(torch, 13, 2, 1, 9, heads, kvh, 64, 3, 1)
    assert launch("lia_attn_decode_launch", q, heads * 64 + 16, kc, vc, out, heads * 64 + 24, 2, 9, heads, kvh, 64, 3, 1, 1) == -1
    assert (host(out) == SENTINEL).all()


# ---- argmax ------------------------------------------------------------------------------------------------------------------
ARGMAX_CASES = [(1, 300), (7, 300), (8, 300), (50257, 300), (50272, 300), (128256, 64)]
TOP = 0x4280                        # 64.0: above every N(0, 1) logit


def argmax_rows(vocab, B, seed=17):
    """N(0, 1) logits with, by row: maximal ties in one lane, in two lanes of one wave (the higher index in the lower lane), in two
    waves (likewise), a unique maximum at index 0 / vocab - 1, and a row that is all -inf"""
    import synth
    rs = np.random.RandomState(seed)
    x = synth.f32_to_bf16_bits(rs.standard_normal((B, vocab)).astype(np.float32))
    vec = vocab % ARGMAX_VEC == 0
    per_lane, stride = (8, 8 * ROW_THREADS) if vec else (1, ROW_THREADS)    # elements per lane per step, step of the whole group
    ties = [(1, 6) if vec else (0, stride),                          # one lane: same 8-group / a later step
            (2, 2 + stride),
            (5 * per_lane + 3, stride + 2 * per_lane),               # lanes 5 and 2 (step 1) of wave 0
            (3 * 64 * per_lane, stride + 64 * per_lane),             # waves 3 and 1 (step 1)
            (0,), (vocab - 1,)]
    for r in range(B):
        kind = r % (len(ties) + 2)
        if kind < len(ties):
            for p in ties[kind]:
                x[r, p % vocab] = TOP
        elif kind == len(ties):
            x[r, :] = 0xff80
    return x


@pytest.mark.parametrize("vocab,B", ARGMAX_CASES)
def test_argmax_variants(gpu, vocab, B):
    """lia_argmax_launch, 16-byte and scalar paths: ties take the first index wherever the tied lanes are; an all -inf row gives 0;
    `suppress` equal to the unique maximum gives the runner-up.  Bit-exact."""
    torch, launch = gpu
    x = argmax_rows(vocab, B)
    xd = torch.from_numpy(x.view(np.int16)).cuda()
    out = torch.full((B,), -7, dtype=torch.int64, device="cuda")
    launch("lia_argmax_launch", xd, out, B, vocab, -1)
    assert (out.cpu().numpy() == R.argmax(x)).all()
    s = vocab // 2 + 1 if vocab > 1 else 0
    x[:, s] = 0x4300                                                  # 128.0: the unique maximum of every row ...
    xd = torch.from_numpy(x.view(np.int16)).cuda()
    launch("lia_argmax_launch", xd, out, B, vocab, s)                 # ... suppressed
    ref = R.argmax(x, suppress=s)
    assert (out.cpu().numpy() == ref).all()
    assert (ref != s).all() or vocab == 1


# ---- coverage and sensitivity ------------------------------------------------------------------------------------------------
def test_cases_reach_every_variant():
    """The case lists reach every kernel of every launcher, and the shapes on both sides of each threshold."""
    for kind, regs in (("layernorm", LN_REG), ("rmsnorm", RMS_REG)):
        got = {norm_kernel(kind, r, H) for r, H, _, _ in NORM_CASES}
        assert got == {"row<1>", "row<2>", "plain"} | {f"reg<{n}>" for n in regs}, (kind, got)
        for n in regs:                                                   # both sides of each reg<N> limit, H = 512 N
            assert {(1025, 512 * n), (1025, 512 * n + 8)} <= {(r, H) for r, H, _, _ in NORM_CASES}
    assert {(ROW_NORM_MAX_ROWS, 4096), (ROW_NORM_MAX_ROWS + 1, 4096), (1, 8 * ROW_THREADS), (1, 8 * ROW_THREADS + 8),
            (1, 16 * ROW_THREADS), (1, 16 * ROW_THREADS + 8)} <= {(r, H) for r, H, _, _ in NORM_CASES}
    assert {"vec", "scalar"} == {"vec" if d % ROPE_VEC_D == 0 and (h * d + p) % ROPE_VEC_STRIDE == 0 else "scalar"
                                 for d, h, _, p in ROPE_CASES}
    assert {m for _, _, m, _ in ROPE_CASES} == set(ROPE_MAPS)
    assert {gb for _, _, gb, _ in SILU_CASES} == {0, GU_BLOCK}
    n8 = [M * F // 8 for M, F, _, _ in SILU_CASES]
    assert SILU_MAX_BLOCKS * 256 in n8 and any(n > SILU_MAX_BLOCKS * 256 for n in n8)
    assert {prefill_variant(B, T, kvh, d) for B, T, _, kvh, d, _ in PREFILL_CASES} == {
        "128/r05", "128/xcd", "128/xcd-padded", "generic<32>", "generic<64>"}
    nqb = {-(-T // ATTN_QBLOCK) for B, T, _, _, d, _ in PREFILL_CASES if d == 128}
    assert nqb == {1, 2, 3, 4, 5, 6}
    assert {(d, h // k, ps) for _, _, h, k, d, ps in PREFILL_CASES} >= {(d, G, ps) for d in (32, 64, 128) for G in DECODE_G
                                                                         for ps in (0, 1)}
    assert {v % ARGMAX_VEC == 0 for v, _ in ARGMAX_CASES} == {True, False}
    assert decode_s_max(32, 1) == 40824 and decode_s_max(128, 8) == 4600


def test_reference_mutants_are_rejected(gpu):
    """Each kernel runs once; its output passes this file's comparison against the right reference and FAILS it against every
    subtly wrong one: the bounds above are tight enough to see such a bug.
    Measured: the closest mutants are decode's OPT scaling / unrounded q.k (11-12 % bit-identical, 7-8 quanta), the
    LayerNorm extra rounding (71 %) and RMSNorm's dropped rounding (74 %)."""
    torch, launch = gpu
    rejected = []

    def expect(what, got, ref, mutants, **kw):
        ok, msg = verdict(got, ref, **kw)
        assert ok, f"{what}: the kernel fails the right reference: {msg}"
        for name, m in mutants.items():
            ok, msg = verdict(got, m, **kw)
            print(f"\n{what} vs mutant '{name}': {msg}")
            assert not ok, f"{what}: the mutant '{name}' is not rejected: {msg}"
            rejected.append(f"{what}: {name}")

    attn = dict(min_exact=ATTN_MIN_EXACT, bound=(ATTN_ATOL, ATTN_RTOL))
    B, T, heads, kvh, d = 2, 257, 8, 2, 128
    q, kc, vc, got, b0 = run_attention(gpu, B, T, T, heads, kvh, d, 1)
    ref = lambda **m: R.attention(q, kc, vc, T, heads, kvh, m.pop("ps", 1), b0=b0, **m)  # noqa: E731
    expect("prefill <128> Llama", got, ref(), {
        "causal mask off by one": ref(mask_shift=1),
        "kh = hh % kv_heads": ref(kv_head_of=lambda hh: hh % kvh),
        "OPT scaling": ref(ps=0),
        "q.k not rounded": ref(round_qk=False)}, **attn)
    S = 1037
    q, kc, vc, got, b0 = run_attention(gpu, 3, 1, S, heads, kvh, d, 1)
    ref = lambda **m: R.attention(q, kc, vc, S, heads, kvh, m.pop("ps", 1), b0=b0, **m)  # noqa: E731
    expect("decode <128, 4> Llama", got, ref(), {
        "kh = hh % kv_heads": ref(kv_head_of=lambda hh: hh % kvh),
        "OPT scaling": ref(ps=0),
        "q.k not rounded": ref(round_qk=False)}, **attn)

    x, g, b, y = run_norm(gpu, "layernorm", 1025, 7168, 1.0, 0.0)
    expect("layernorm reg<14>", y, R.layernorm(x, g, b), {"extra rounding": R.layernorm(x, g, b, round_normalized=True)},
           min_exact=NORM_MIN_EXACT)
    x, w, _, y = run_norm(gpu, "rmsnorm", 1024, 4096, 1.0, 0.0)
    expect("rmsnorm row<1>", y, R.rmsnorm(x, w), {"inner rounding dropped": R.rmsnorm(x, w, round_inner=False)},
           min_exact=NORM_MIN_EXACT)

    x, got, cosb, sinb, pos = run_rope(gpu, 128, 8, "q", 8)
    expect("rope vec", got, R.rope(x, cosb, sinb, pos, 8), {
        "position + 1": R.rope(x, cosb, sinb, np.minimum(pos + 1, ROPE_MAX_POS - 1), 8),
        "products not rounded": R.rope(x, cosb, sinb, pos, 8, round_products=False)}, min_exact=1.0)

    M, F = 64, 4096
    gu, got = run_silu(gpu, M, F, GU_BLOCK, "normal")
    g, u = R.split_gate_up(gu, F, GU_BLOCK)
    expect("silu*up block 32", got, R.silu_mul(g, u), {"gate and up swapped in a block": R.silu_mul(u, g)}, max_ulp=SILU_MAX_ULP)

    x = argmax_rows(50272, 64)
    xd = torch.from_numpy(x.view(np.int16)).cuda()
    out = torch.zeros((64,), dtype=torch.int64, device="cuda")
    launch("lia_argmax_launch", xd, out, 64, 50272, -1)
    got = out.cpu().numpy()
    assert (got == R.argmax(x)).all() and (got != R.argmax(x, last_on_ties=True)).any()
    rejected.append("argmax: ties keep the last index")
    print("\nrejected:", *rejected, sep="\n  ")
