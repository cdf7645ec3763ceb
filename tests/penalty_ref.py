"""NumPy restatement of the repetition / presence / frequency penalties (include/lia_hip.h, lia_ctx_set_penalties) for the penalty
tests: the formula in fp32, operation by operation, the bf16 rounding, and the count table's builder.

A count word: bit 15 = the token occurs in the prompt, bits 0..14 = n, how often it was generated (saturating at 32767).

    x = fp32(l);  if c != 0: x = x * theta if x < 0 else x / theta;  x = x - alpha_f * float(n);  x = x - (alpha_p if n > 0 else 0)

Every operation is one IEEE fp32 operation (NumPy's float32 arithmetic: no FMA, a correctly rounded division); the settings are the
fp32 values the C ABI receives."""
import numpy as np

PROMPT_BIT = 0x8000
COUNT_MAX = 0x7fff


def bf16_to_f32(u16):
    return (np.asarray(u16, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16(x):
    """round to nearest even; +-inf stay; NaN is not defined here"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def penalty_f32(x, counts, repetition=1.0, presence=0.0, frequency=0.0):
    """x: float32 [M, vocab]; counts: uint16 [M, >= vocab] -> the penalised fp32 values (before the bf16 rounding)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    c = np.asarray(counts)
    assert c.dtype.itemsize == 2 and c.shape[0] == x.shape[0] and c.shape[1] >= x.shape[1], "counts: 16-bit words, one per logit"
    c = c.view(np.uint16)[:, :x.shape[1]]
    theta, a_p, a_f = np.float32(repetition), np.float32(presence), np.float32(frequency)
    with np.errstate(all="ignore"):
        rep = np.where(x < 0, x * theta, x / theta).astype(np.float32)
        x = np.where(c != 0, rep, x).astype(np.float32)
        n = (c & COUNT_MAX)
        x = (x - (a_f * n.astype(np.float32)).astype(np.float32)).astype(np.float32)
        x = (x - np.where(n > 0, a_p, np.float32(0.0)).astype(np.float32)).astype(np.float32)
    return x


def penalty_ref(logits_u16, counts, repetition=1.0, presence=0.0, frequency=0.0):
    """logits_u16: uint16 bf16 patterns [M, vocab]; counts: uint16 [M, >= vocab] -> the penalised bf16 patterns, uint16 [M, vocab]"""
    return f32_to_bf16(penalty_f32(bf16_to_f32(logits_u16), counts, repetition, presence, frequency))


def first_argmax(u16, suppress=-1):
    """the greedy id of every row of bf16 patterns: the first index of the maximum (lia_argmax_kernel's tie rule)"""
    f = bf16_to_f32(u16).copy()
    if suppress >= 0:
        f[:, suppress] = -np.inf
    return f.argmax(axis=1)


def add_counts(table, ids, generated, vocab, first=None, active=None):
    """lia_token_counts_add on a uint16 table [B, ldc], in place: ids int64 [B, n]; positions t < first[b] and rows with active[b] == 0
    are skipped, ids outside [0, vocab) ignored.  Vectorised (np.add.at counts duplicates)."""
    ids = np.asarray(ids, dtype=np.int64)
    B, n = ids.shape
    keep = (ids >= 0) & (ids < vocab)
    if first is not None:
        keep &= np.arange(n)[None, :] >= np.asarray(first)[:, None]
    if active is not None:
        keep &= (np.asarray(active) != 0)[:, None]
    rows = np.broadcast_to(np.arange(B)[:, None], ids.shape)[keep]
    cols = ids[keep]
    if not generated:
        table[rows, cols] |= PROMPT_BIT
        return table
    add = np.zeros(table.shape, dtype=np.int64)
    np.add.at(add, (rows, cols), 1)
    n_new = np.minimum((table & COUNT_MAX).astype(np.int64) + add, COUNT_MAX).astype(np.uint16)
    table[:] = (table & PROMPT_BIT) | n_new
    return table


def build_counts(prompt, generated, vocab, ldc=None, starts=None):
    """the table of rows whose prompt is prompt[b, starts[b]:] and which generated `generated[b]` (a [B, n] array or a list of
    per-row id lists) -> uint16 [B, ldc]"""
    prompt = np.asarray(prompt, dtype=np.int64)
    B = prompt.shape[0]
    table = np.zeros((B, vocab if ldc is None else ldc), dtype=np.uint16)
    add_counts(table, prompt, False, vocab, first=starts)
    for b in range(B):
        g = np.asarray(generated[b], dtype=np.int64).reshape(1, -1) if len(generated) else np.zeros((1, 0), dtype=np.int64)
        if g.size:
            add_counts(table[b:b + 1], g, True, vocab)
    return table
