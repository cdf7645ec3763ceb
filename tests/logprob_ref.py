"""float64 NumPy reference of lia_topn_logprobs (include/lia_hip.h): per row of bf16 logits the log-probability of a chosen id and the
n_top tokens of largest logit with theirs, in the order of the sampler's 16-bit key -- logit descending, ties by the lower id."""
import numpy as np

import score_ref as SR


def key_of(bits):
    """the 16-bit order key of bf16 bit patterns (lia_row_passes.h, key_of): sign-magnitude -> offset binary"""
    h = np.asarray(bits, dtype=np.uint16).astype(np.int64)
    return np.where(h & 0x8000, ~h & 0xFFFF, h | 0x8000)


def topn_logprobs(logit_bits, ids, n_top):
    """bf16 logits [M, vocab] (bit patterns), ids [M], n_top <= vocab -> (chosen float64 [M] (0.0 for an id outside the row), top_ids
    int64 [M, n_top], top_logprobs float64 [M, n_top], m [M], log s [M])"""
    bits = np.asarray(logit_bits, dtype=np.uint16)
    M, vocab = bits.shape
    assert 0 <= n_top <= vocab
    x = SR.bf16_to_f64(bits)
    with np.errstate(invalid="ignore"):
        ls = SR.log_softmax(x)
    t = np.asarray(ids, dtype=np.int64)
    ok = (t >= 0) & (t < vocab)
    rows = np.arange(M)
    chosen = np.where(ok, ls[rows, np.where(ok, t, 0)], 0.0)
    keys = key_of(bits)
    tok = np.arange(vocab)
    top_ids = np.empty((M, n_top), np.int64)
    for r in range(M):
        top_ids[r] = np.lexsort((tok, -keys[r]))[:n_top]
    top_lp = np.take_along_axis(ls, top_ids, axis=1) if n_top else np.empty((M, 0))
    m = x.max(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        log_s = np.log(np.exp(x - m[:, None]).sum(axis=-1))
    return chosen, top_ids, top_lp, m, log_s
