"""The float64 references of f64_ref.py against the oracle's restatements of the same ops (which tests/golden pins to the
reference and to HF), on seeded inputs.  The oracle computes in fp32, so the two may differ where an fp32 value lands next to
a bf16 rounding boundary: every output within one bf16 quantum of the op's largest output, at least 99 % bit-identical.
CPU only."""
import numpy as np
import pytest

import f64_ref as R
import synth


def rand_bits(seed, shape, scale=1.0, mean=0.0):
    rs = np.random.RandomState(seed)
    return synth.f32_to_bf16_bits((mean + scale * rs.standard_normal(shape)).astype(np.float32))


def agree(ref, orc, what):
    a, b = R.f64(ref), R.f64(orc)
    q = R.quantum(np.abs(b).max())
    err = np.abs(a - b).max()
    frac = float((ref == orc).mean())
    print(f"\n{what}: {100 * frac:.3f} % bit-identical, max |err| {err:.3g} = {err / q:.2f} quanta of max |oracle|")
    assert err <= q, f"{what}: max err {err:.4g} > one quantum {q:.3g}"
    assert frac >= 0.99, f"{what}: only {frac:.5f} bit-identical"


def test_rnd_is_round_to_nearest_even_from_float64():
    # ties to even at 1 + 2^-8 (down) and 1 + 3 * 2^-8 (up); just above a tie rounds up (an fp32 step would have lost 2^-40)
    x = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -40, -(1 + 2.0 ** -8 + 2.0 ** -40), 3.3962e38, 2.0 ** -134,
                  2.0 ** -133 * 1.5, 0.0, -0.0, np.inf, np.nan])
    y = R.rnd(x)
    assert y[0] == 1 and y[1] == 1 + 4 * 2.0 ** -8 and y[2] == 1 + 2.0 ** -7 and y[3] == -(1 + 2.0 ** -7)
    assert y[4] == np.inf and y[5] == 0 and y[6] == 2.0 ** -132 and np.signbit(y[8]) and y[9] == np.inf and np.isnan(y[10])
    b = rand_bits(1, (4096,), 3.0)
    assert (R.bits(R.rnd(R.f64(b))) == b).all() and (R.bits(R.f64(b)) == synth.f32_to_bf16_bits(R.f64(b).astype(np.float32))).all()
    assert R.ulp_distance(np.array([0x0000, 0x3f80, 0x3f80]), np.array([0x8000, 0x3f81, 0xbf80])).tolist() == [0, 1, 2 * 0x3f80]


@pytest.mark.parametrize("rows,H,scale,mean", [(64, 768, 1.0, 0.0), (7, 7168, 300.0, 0.0), (33, 2048, 1e-3, 0.0), (16, 4096, 0.5, 256.0)])
def test_layernorm_matches_oracle(oracle, rows, H, scale, mean):
    x = rand_bits(10, (rows, H), scale, mean)
    g, b = rand_bits(11, (H,), 0.5, 1.0), rand_bits(12, (H,), 0.5)
    agree(R.layernorm(x, g, b), oracle.layernorm(x, g, b), f"layernorm {rows}x{H} N({mean}, {scale})")


@pytest.mark.parametrize("rows,H,scale", [(64, 4096, 1.0), (5, 8200, 300.0), (40, 768, 1e-3)])
def test_rmsnorm_matches_oracle(oracle, rows, H, scale):
    x, w = rand_bits(20, (rows, H), scale), rand_bits(21, (H,), 0.3, 1.0)
    agree(R.rmsnorm(x, w), oracle.rmsnorm(x, w), f"rmsnorm {rows}x{H}")


@pytest.mark.parametrize("B,T,heads,d,pos0", [(2, 5, 4, 64, 3), (1, 9, 8, 128, 90), (3, 1, 2, 8, 99)])
def test_rope_matches_oracle(oracle, B, T, heads, d, pos0):
    cosb, sinb = oracle.rope_tables(100, d, 500000.0)
    x = rand_bits(30, (B, T, heads * d), 2.0)
    pos = np.tile(pos0 + np.arange(T), B)
    ref = R.rope(x.reshape(B * T, heads * d), cosb, sinb, pos, heads)
    orc = oracle.rope(x, cosb, sinb, heads, pos0).reshape(B * T, heads * d)
    agree(ref, orc, f"rope {B}x{T}x{heads}x{d}")
    assert (ref == orc).all()               # every product of two bf16 is exact in fp32: nothing to differ in


@pytest.mark.parametrize("M,F,gu_block", [(16, 4096, 0), (9, 1792, 32)])
def test_silu_mul_matches_oracle(oracle, M, F, gu_block):
    gu = rand_bits(40, (M, 2 * F), 4.0)
    g, u = R.split_gate_up(gu, F, gu_block)
    agree(R.silu_mul(g, u), oracle.silu_mul(np.ascontiguousarray(g), np.ascontiguousarray(u)), f"silu*up {M}x{F} block {gu_block}")


def _cache(seed, B, T, S, heads, d):
    q = rand_bits(seed, (B, T, heads * d), 1.5)
    return q, rand_bits(seed + 1, (S + 2, B, heads, d), 1.5), rand_bits(seed + 2, (S + 2, B, heads, d))


@pytest.mark.parametrize("B,T,S,heads,d", [(2, 40, 40, 2, 64), (1, 129, 129, 1, 128), (3, 1, 77, 4, 32), (2, 5, 21, 2, 128)])
def test_attention_opt_scaling_matches_oracle(oracle, B, T, S, heads, d):
    q, kc, vc = _cache(50, B, T, S, heads, d)
    agree(R.attention(q, kc, vc, S, heads, heads, post_scale=0), oracle.attention(q, kc, vc, S, heads, policy_gpu=True),
          f"attention (OPT) {B}x{T}/{S}x{heads}x{d}")


@pytest.mark.parametrize("B,T,S,heads,kvh,d", [(2, 33, 33, 8, 2, 128), (1, 64, 64, 4, 4, 64), (3, 1, 130, 8, 1, 32), (2, 7, 50, 4, 2, 128)])
def test_attention_llama_scaling_matches_oracle(oracle, B, T, S, heads, kvh, d):
    q = rand_bits(60, (B, T, heads * d), 1.5)
    kc, vc = rand_bits(61, (S + 2, B, kvh, d), 1.5), rand_bits(62, (S + 2, B, kvh, d))
    agree(R.attention(q, kc, vc, S, heads, kvh, post_scale=1), oracle.attention_gqa(q, kc, vc, S, heads, kvh),
          f"attention (Llama) {B}x{T}/{S}x{heads}/{kvh}x{d}")


@pytest.mark.parametrize("B,T,S,heads,kvh", [(2, 257, 257, 4, 2), (32, 1, 1037, 8, 2)])
@pytest.mark.parametrize("d", (32, 64, 128))
@pytest.mark.parametrize("family", ("exact", "ramp", "fall", "sink", "uniform", "hot"))
def test_attention_matches_oracle_on_the_families(oracle, family, d, B, T, S, heads, kvh):
    """the sink / ramp / one-hot / uniform inputs of attn_families.py (scores in the hundreds, exp underflowing for most keys):
    f64_ref.attention against the oracle's GPU-branch restatements, OPT scaling (kv_heads == heads) and Llama scaling (grouped)"""
    import attn_families as F
    q, kc, vc = F.make(family, B, T, S, heads, heads, d, 0)
    agree(R.attention(q, kc, vc, S, heads, heads, post_scale=0), oracle.attention(q, kc, vc, S, heads, policy_gpu=True, causal=True),
          f"attention (OPT) {family} {B}x{T}/{S}x{heads}x{d}")
    q, kc, vc = F.make(family, B, T, S, heads, kvh, d, 1)
    agree(R.attention(q, kc, vc, S, heads, kvh, post_scale=1), oracle.attention_gqa(q, kc, vc, S, heads, kvh),
          f"attention (Llama) {family} {B}x{T}/{S}x{heads}/{kvh}x{d}")


def test_argmax_takes_the_first_maximum_and_skips_the_suppressed_token():
    x = rand_bits(70, (4, 50), 1.0)
    x[1, [3, 17]] = x[1, 40] = synth.f32_to_bf16_bits(np.float32([9.0]))[0]
    x[2, :] = 0xff80                                                      # all -inf
    assert R.argmax(x)[1:3].tolist() == [3, 0] and R.argmax(x, last_on_ties=True)[1] == 40
    assert R.argmax(x, suppress=3)[1] == 17 and R.argmax(x, suppress=int(R.argmax(x)[0]))[0] != R.argmax(x)[0]


@pytest.mark.parametrize("M,N,K,has_bias,has_res,relu", [(37, 256, 768, True, False, False), (64, 96, 2048, True, True, False),
                                                         (5, 512, 4096, True, False, True), (130, 64, 320, False, True, False),
                                                         (16, 128, 1024, False, False, False), (9, 80, 4160, True, True, True)])
def test_linear_matches_oracle(oracle, M, N, K, has_bias, has_res, relu):
    """f64_ref.linear against the oracle's GPU-semantics linear (split_bias: bf16(acc) -> bf16(+ bias) -> relu -> bf16(res + .)),
    and the oracle's fp32 result inside the bracket [linear(acc - delta), linear(acc + delta)] the GPU tests use"""
    x, w = rand_bits(40, (M, K)), rand_bits(41, (N, K), K ** -0.5)
    b = rand_bits(42, (N,), 0.5) if has_bias else None
    r = rand_bits(43, (M, N)) if has_res else None
    orc = oracle.linear(x, w, b, r, relu, split_bias=True)
    agree(R.linear(x, w, b, r, relu), orc, f"linear {M}x{N}x{K} bias {has_bias} res {has_res} relu {relu}")
    acc, d = R.matmul(x, w), R.matmul_slack(x, w)
    lo, hi, o = R.f64(R.linear(x, w, b, r, relu, acc=acc - d)), R.f64(R.linear(x, w, b, r, relu, acc=acc + d)), R.f64(orc)
    assert ((lo <= o) & (o <= hi)).all()


def test_linear_rounding_points():
    """the chain's rounding points and its mutants on hand-made sums: ties to even at bf16(acc), at bf16(t + bias) and at
    bf16(residual + t); each mutant switch changes at least one of these outputs"""
    one = lambda v: R.bits(np.array([v], np.float64))
    x = R.bits(np.ones((1, 128)))
    w = R.bits(np.concatenate([np.full(64, 0.0), np.full(64, 4.0)])[None, :])     # x . w = 256, all of it in the last K chunk
    acc = np.array([[257.0]])                                    # a tie between 256 and 258: even -> 256
    assert R.f64(R.linear(x, w, acc=acc))[0, 0] == 256.0
    assert R.f64(R.linear(x, w, acc=acc, ties_away=True))[0, 0] == 258.0
    assert R.f64(R.linear(x, w, one(1.0), acc=acc))[0, 0] == 256.0            # bf16(256 + 1) = 256: the rounded sum came first
    assert R.f64(R.linear(x, w, one(1.0), acc=acc, round_acc=False))[0, 0] == 258.0   # bf16(257 + 1) = 258
    assert R.f64(R.linear(x, w, None, one(1.0), acc=acc))[0, 0] == 256.0
    assert R.f64(R.linear(x, w, None, one(1.0), acc=acc, round_before_residual=False))[0, 0] == 258.0
    assert R.f64(R.linear(x, w, None, None, True, acc=-acc))[0, 0] == 0.0
    assert R.f64(R.linear(x, w))[0, 0] == 256.0 and R.f64(R.linear(x, w, drop_last_k=True))[0, 0] == 0.0
    b2 = R.bits(np.array([1.0, 2.0]))
    assert R.f64(R.linear(x, np.concatenate([w, w]), b2, acc=np.array([[0.0, 0.0]]), bias_seg=1)).tolist() == [[2.0, 1.0]]
