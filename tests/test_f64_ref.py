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


def test_argmax_takes_the_first_maximum_and_skips_the_suppressed_token():
    x = rand_bits(70, (4, 50), 1.0)
    x[1, [3, 17]] = x[1, 40] = synth.f32_to_bf16_bits(np.float32([9.0]))[0]
    x[2, :] = 0xff80                                                      # all -inf
    assert R.argmax(x)[1:3].tolist() == [3, 0] and R.argmax(x, last_on_ties=True)[1] == 40
    assert R.argmax(x, suppress=3)[1] == 17 and R.argmax(x, suppress=int(R.argmax(x)[0]))[0] != R.argmax(x)[0]
