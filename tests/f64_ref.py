"""Plain float64 restatements of the hot-path ops, for the kernel-variant tests (test_gpu_kernel_variants.py) and pinned to
the oracle by test_f64_ref.py.

Tensors go in and come out as numpy uint16 arrays of bf16 bit patterns, like oracle/lia_oracle.py.  Inside, everything is
float64, and a value is rounded to bf16 (round-to-nearest-even, straight from the float64 value: no fp32 step) exactly where
the reference or HF transformers' eager bf16 model materialises a bf16 tensor.  Each function names its rounding points.

A few functions take keyword switches that only the sensitivity test (test_reference_mutants_are_rejected) turns: each one
makes the reference subtly wrong in one way a kernel could be.
"""
import numpy as np

ROWS_PER_CHUNK = 256        # norms work on this many rows at a time: a 4097 x 16392 input stays a few hundred MB in float64


def rnd(x, ties_away=False):
    """float64 -> the nearest bf16 value (ties to even), still as float64; subnormals, overflow to inf and NaN as bf16 has them.
    ties_away (a mutant): ties rounded away from zero."""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)                                  # |x| = m 2^e, 0.5 <= m < 1: 8 significant bits -> quantum 2^(e - 8)
    qe = np.maximum(e - 8, -133)                        # below 2^-126 the quantum stays 2^-133 (bf16 subnormals)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.ldexp(x, -qe)
        s = np.copysign(np.floor(np.abs(s) + 0.5), s) if ties_away else np.rint(s)
        y = np.ldexp(s, qe)
        y = np.where(np.abs(y) >= 2.0 ** 128, np.copysign(np.inf, x), y)
    return np.where(np.isfinite(x), y, x)


def f64(bits):
    """bf16 bit patterns -> float64 values"""
    b = np.ascontiguousarray(bits, dtype=np.uint16)
    with np.errstate(invalid="ignore"):                  # NaN patterns stay NaN
        return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bits(x):
    """float64 values that are bf16 values (the output of rnd) -> bit patterns"""
    return (np.ascontiguousarray(x, dtype=np.float64).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def quantum(x):
    """one bf16 quantum at magnitude |x| (x > 0)"""
    return 2.0 ** (np.floor(np.log2(x)) - 7)


def ulp_distance(a_bits, b_bits):
    """how many bf16 values lie between two bit patterns (0: identical; +0 and -0 are 0 apart)"""
    def ordered(b):
        b = np.ascontiguousarray(b, dtype=np.uint16).astype(np.int64)
        return np.where(b & 0x8000, -(b & 0x7fff), b)
    return np.abs(ordered(a_bits) - ordered(b_bits))


def layernorm(x, g, b, eps=1e-5, round_normalized=False):
    """F.layer_norm on bf16: mean and variance (two passes) and the affine in high precision, ONE rounding at the output:
        y = bf16((x - mean) / sqrt(var + eps) * g + b)
    round_normalized (a mutant): an extra rounding of the normalised value before the affine."""
    H = x.shape[-1]
    xr = np.ascontiguousarray(x).reshape(-1, H)
    gf, bf = f64(g), f64(b)
    out = np.empty(xr.shape, np.uint16)
    for r0 in range(0, xr.shape[0], ROWS_PER_CHUNK):
        xc = f64(xr[r0:r0 + ROWS_PER_CHUNK])
        c = xc - xc.mean(axis=1, keepdims=True)
        n = c / np.sqrt((c * c).mean(axis=1, keepdims=True) + eps)
        if round_normalized:
            n = rnd(n)
        out[r0:r0 + ROWS_PER_CHUNK] = bits(rnd(n * gf + bf))                       # the one rounding point
    return out.reshape(x.shape)


def rmsnorm(x, w, eps=1e-5, round_inner=True):
    """LlamaRMSNorm.forward: y = bf16(w * bf16(x * rsqrt(mean(x^2) + eps))), the statistic in high precision.
    round_inner=False (a mutant): the inner rounding dropped."""
    H = x.shape[-1]
    xr = np.ascontiguousarray(x).reshape(-1, H)
    wf = f64(w)
    out = np.empty(xr.shape, np.uint16)
    for r0 in range(0, xr.shape[0], ROWS_PER_CHUNK):
        xc = f64(xr[r0:r0 + ROWS_PER_CHUNK])
        n = xc / np.sqrt((xc * xc).mean(axis=1, keepdims=True) + eps)
        if round_inner:
            n = rnd(n)                                                              # rounding 1: hidden_states.to(bf16)
        out[r0:r0 + ROWS_PER_CHUNK] = bits(rnd(wf * n))                             # rounding 2: weight * .
    return out.reshape(x.shape)


def rope(x, cosb, sinb, pos, heads, round_products=True):
    """apply_rotary_pos_emb on rows of `heads` heads: x [rows, heads * d], pos [rows] (the table row of each row), cos / sin
    tables [max_pos, d].  rotate_half(x) = cat(-x2, x1);  out = bf16(bf16(x * cos) + bf16(rotate_half(x) * sin)).
    round_products=False (a mutant): the two products not rounded."""
    rows = x.shape[0]
    d = cosb.shape[1]
    xf = f64(x).reshape(rows, heads, d)
    c, s = f64(cosb)[pos][:, None, :], f64(sinb)[pos][:, None, :]
    half = d // 2
    rot = np.concatenate([-xf[..., half:], xf[..., :half]], axis=-1)
    r = rnd if round_products else (lambda v: v)
    return bits(rnd(r(xf * c) + r(rot * s))).reshape(rows, heads * d)        # roundings: x cos, rot sin, their sum


def matmul(x, w, drop_last_k=False):
    """x [M, K] . w [N, K]^T in float64 (bf16 bit patterns in).  drop_last_k (a mutant): the last K chunk of 64 left out."""
    K = w.shape[1]
    k = K - 64 if drop_last_k else K
    return f64(np.ascontiguousarray(x)[:, :k]) @ f64(np.ascontiguousarray(w)[:, :k]).T


def matmul_slack(x, w):
    """delta = K 2^-24 (|x| . |w|^T): how far any sequential fp32 accumulation of x . w^T can lie from the exact sum"""
    K = w.shape[1]
    return K * 2.0 ** -24 * (np.abs(f64(x)) @ np.abs(f64(w)).T)


def linear(x, w, bias=None, residual=None, relu=False, *, acc=None, round_acc=True, round_before_residual=True, ties_away=False,
           drop_last_k=False, bias_seg=None):
    """torch.matmul(x, w.t()) + bias [relu] [residual + .] with the reference's (and the GPU epilogue's) rounding points, each
    straight from float64:
        t = bf16(acc);  t = bf16(t + bias);  t = max(t, 0);  y = bf16(residual + t)
    acc: the float64 x . w^T (computed when None); passing acc -/+ delta evaluates the same chain there.  Every step is monotone
    non-decreasing in acc, so [linear(acc - delta), linear(acc + delta)] holds every result an accumulation within delta gives.
    Mutants: round_acc=False (no rounding after the matmul: the bias goes onto the unrounded sum), round_before_residual=False (the
    value before the residual add not rounded), ties_away (ties rounded away from zero at every rounding point), drop_last_k
    (the last K chunk of 64 left out of the sum), bias_seg=S (the bias of column n taken from column n + S: the neighbouring
    segment of an out-map with S columns per segment)."""
    a = matmul(x, w, drop_last_k) if acc is None else np.asarray(acc, dtype=np.float64)
    r = lambda v: rnd(v, ties_away)
    last = residual is not None and not round_before_residual         # the rounding in front of the residual add is skipped
    t = r(a) if round_acc and not (last and bias is None) else a
    if bias is not None:
        b = f64(bias)
        if bias_seg:
            b = np.roll(b, -bias_seg)
        t = t + b if last else r(t + b)
    if relu:
        t = np.maximum(t, 0.0)
    if residual is not None:
        t = r(f64(residual) + t)
    return bits(r(t))                                                               # (a no-op unless a mutant left t unrounded)


def split_gate_up(gu, F, gu_block):
    """gu [M, 2F] -> (gate [M, F], up [M, F]): gu_block 0: columns [gate | up]; 32: blocks of 32 gate | 32 up columns"""
    M = gu.shape[0]
    if gu_block:
        v = gu.reshape(M, F // gu_block, 2, gu_block)
        return v[:, :, 0, :].reshape(M, F), v[:, :, 1, :].reshape(M, F)
    return gu[:, :F], gu[:, F:2 * F]


def silu_mul_glu(gu, gu_block=32):
    """silu_mul of a gate | up projection's output gu [M, 2F] in the interleaved layout (blocks of gu_block gate | gu_block up
    columns, LIA_GU_BLOCK) or, gu_block 0, as [gate | up] halves"""
    g, u = split_gate_up(gu, gu.shape[1] // 2, gu_block)
    return silu_mul(g, u)


def silu_mul(g, u):
    """LlamaMLP act_fn(gate) * up: m = bf16(bf16(silu(g)) * u), silu(g) = g / (1 + exp(-g))"""
    gf = f64(g)
    with np.errstate(over="ignore"):
        s = rnd(gf / (1.0 + np.exp(-gf)))                                           # rounding 1: act_fn(gate) in bf16
    return bits(rnd(s * f64(u)))                                                    # rounding 2: . * up


def attention(q, kc, vc, S, heads, kv_heads, post_scale, b0=0, mask_shift=0, kv_head_of=None, round_qk=True, round_p=True):
    """Causal attention of T query rows per batch row at positions S - T .. S - 1 against cache rows 0 .. S - 1.

    q [B, T, heads * d]; kc / vc the seq-major cache [Smax, Bc, kv_heads, d], batch rows b0 .. b0 + B - 1 read.  Query head hh
    reads K / V head hh / (heads / kv_heads).  Rounding points:
        post_scale 0 (OPT, attentions.py:456, 499):   s = bf16(bf16(q * d^-0.5) . k)
        post_scale 1 (HF Llama eager):                s = bf16(bf16(q . k) * d^-0.5)
        causal mask: key j visible to query t iff j <= S - T + t, the others -inf
        p = bf16(softmax(s))      o = bf16(p . v)
    Mutants: mask_shift (the mask off by that many keys), kv_head_of (another head map: hh -> K / V head), round_qk=False (the
    rounding of the raw product dropped), round_p=False (P not rounded to bf16)."""
    B, T, HD = q.shape
    d = HD // heads
    G = heads // kv_heads
    hh = np.arange(heads)
    kh = hh // G if kv_head_of is None else kv_head_of(hh)
    qf = f64(q).reshape(B, T, heads, d).transpose(0, 2, 1, 3)                       # [B, h, T, d]
    kf = f64(kc[:S, b0:b0 + B]).transpose(1, 2, 0, 3)[:, kh]                        # [B, h, S, d]
    vf = f64(vc[:S, b0:b0 + B]).transpose(1, 2, 0, 3)[:, kh]
    scale = d ** -0.5
    r = rnd if round_qk else (lambda v: v)
    if post_scale:
        s = rnd(r(qf @ kf.transpose(0, 1, 3, 2)) * scale)
    else:
        s = r(rnd(qf * scale) @ kf.transpose(0, 1, 3, 2))
    visible = np.arange(S)[None, :] <= (S - T + np.arange(T) + mask_shift)[:, None]
    s = np.where(visible, s, -np.inf)
    e = np.exp(s - s.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True)
    if round_p:
        p = rnd(p)
    o = rnd(p @ vf)                                                                 # [B, h, T, d]
    return bits(o.transpose(0, 2, 1, 3).reshape(B, T, HD))


def argmax(logits, suppress=-1, last_on_ties=False):
    """greedy argmax over rows of bf16 logits [B, vocab]: the FIRST maximal index; the `suppress` token counts as -inf.
    last_on_ties (a mutant): the last maximal index."""
    f = f64(logits).reshape(-1, logits.shape[-1]).copy()
    if suppress >= 0:
        f[:, suppress] = -np.inf
    if last_on_ties:
        return f.shape[1] - 1 - np.argmax(f[:, ::-1], axis=1)
    return np.argmax(f, axis=1)
