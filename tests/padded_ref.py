"""float64 references for left-padded batches (generate(..., attention_mask=M), M = s_b zeros then ones per row).

attention(): f64_ref.attention's rounding points (bf16 of q * d^-0.5, of q . k, of softmax, of p . v) with a per-row lower key
bound: a query at cache position i >= s_b of row b sees keys s_b .. i, a masked key contributes exactly 0 (the reference's CPU
branch: exp(finfo.min - max) == 0, mha_fusion.py:532-566), a query at a pad position (i < s_b) gives a zero row.
host_attention(): the same visibility with the host kernel's single rounding (fp32 scores / softmax / sum, bf16 at the output).
positions(): HF's (cumsum(mask) * mask) - 1 + 2 of lia/modeling_opt.py:368-378, for a prefill or one decode position.
"""
import numpy as np

from f64_ref import bits, f64, rnd


def starts_of(mask):
    """[B, T] left-padded 0/1 mask -> the per-row starts s_b"""
    m = np.asarray(mask).astype(np.int64)
    return (m.shape[1] - m.sum(axis=1)).astype(np.int32)


def _visible(S, T, s):
    """[T, S] keys visible to the T queries at positions S - T .. S - 1 of a row starting at s; and [T] real-query flags"""
    pos = S - T + np.arange(T)
    j = np.arange(S)
    return (j[None, :] <= pos[:, None]) & (j[None, :] >= s), pos >= s


def attention(q, kc, vc, S, heads, kv_heads, post_scale, starts, b0=0):
    """q [B, T, heads * d] bf16 bits; kc / vc [Smax, Bc, kv_heads, d]; rows b0 .. b0 + B - 1; starts [B].  -> bf16 bits [B, T, H]"""
    B, T, HD = q.shape
    d = HD // heads
    kh = np.arange(heads) // (heads // kv_heads)
    qf = f64(q).reshape(B, T, heads, d).transpose(0, 2, 1, 3)
    kf = f64(kc[:S, b0:b0 + B]).transpose(1, 2, 0, 3)[:, kh]
    vf = f64(vc[:S, b0:b0 + B]).transpose(1, 2, 0, 3)[:, kh]
    scale = d ** -0.5
    out = np.zeros((B, heads, T, d))
    for b in range(B):
        vis, real = _visible(S, T, int(starts[b]))
        for h in range(heads):            # one head at a time: a T 2016 row stays a few arrays of T x S
            if post_scale:
                s = rnd(rnd(qf[b, h] @ kf[b, h].T) * scale)
            else:
                s = rnd(rnd(qf[b, h] * scale) @ kf[b, h].T)
            s = np.where(vis, s, -np.inf)[real]
            e = np.exp(s - s.max(axis=-1, keepdims=True))
            p = rnd(e / e.sum(axis=-1, keepdims=True))
            out[b, h][real] = rnd(p @ vf[b, h])
    return bits(out.transpose(0, 2, 1, 3).reshape(B, T, HD))


def host_attention(q, kc, vc, S, heads, starts, b0=0):
    """the host kernel's arithmetic in float64: scores q . k / sqrt(d) and softmax unrounded, one bf16 rounding of p . v"""
    B, T, HD = q.shape
    d = HD // heads
    qf = f64(q).reshape(B, T, heads, d).transpose(0, 2, 1, 3)
    kf = f64(kc[:S, b0:b0 + B]).transpose(1, 2, 0, 3)
    vf = f64(vc[:S, b0:b0 + B]).transpose(1, 2, 0, 3)
    out = np.zeros((B, heads, T, d))
    for b in range(B):
        vis, real = _visible(S, T, int(starts[b]))
        s = np.where(vis, (qf[b] @ kf[b].transpose(0, 2, 1)) * d ** -0.5, -np.inf)[:, real]
        e = np.exp(s - s.max(axis=-1, keepdims=True))
        out[b][:, real] = rnd((e / e.sum(axis=-1, keepdims=True)) @ vf[b])
    return bits(out.transpose(0, 2, 1, 3).reshape(B, T, HD))


def positions(mask, past_len=0, T=None):
    """learned-position indices of the tokens at cache positions past_len .. past_len + T - 1 (T defaults to the mask's width
    minus past_len): HF's (cumsum(mask) * mask) - 1 + 2 over the mask extended with ones for the generated tokens"""
    m = np.asarray(mask).astype(np.int64)
    W = m.shape[1]
    T = W - past_len if T is None else T
    ext = np.concatenate([m, np.ones((m.shape[0], max(0, past_len + T - W)), dtype=np.int64)], axis=1)
    p = np.cumsum(ext, axis=1) * ext - 1 + 2
    return p[:, past_len:past_len + T]
