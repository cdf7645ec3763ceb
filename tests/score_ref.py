"""NumPy references of the scoring path (float64): the row kernel's log-softmax / greedy token, its error bound, the target shift
and valid mask of scoring.score, lm_eval's rolling windows restated line by line, and loglikelihood over a table of log-probs."""
import numpy as np


def bf16_to_f64(bits):
    b = np.ascontiguousarray(bits, dtype=np.uint16)
    with np.errstate(invalid="ignore"):
        return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def log_softmax(logits):
    """float64 log-softmax over the last axis of float64 logits (-inf entries carry no mass)"""
    x = np.asarray(logits, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    with np.errstate(divide="ignore"):
        return x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))


def token_logprobs(logit_bits, targets):
    """bf16 logits [M, vocab] (bit patterns), targets [M] (-1: none) -> (logprob float64 [M] (0.0 without a target), greedy [M] =
    the first maximal index, m [M], log s [M])"""
    x = bf16_to_f64(logit_bits)
    t = np.asarray(targets, dtype=np.int64)
    ls = log_softmax(x)
    rows = np.arange(x.shape[0])
    ok = (t >= 0) & (t < x.shape[1])
    lp = np.where(ok, ls[rows, np.where(ok, t, 0)], 0.0)
    m = x.max(axis=-1)
    return lp, np.argmax(x, axis=-1).astype(np.int64), m, np.log(np.exp(x - m[:, None]).sum(axis=-1))


def row_kernel_bound(m, log_s, logprob, n_serial, n_threads):
    """|logprob error| allowed to a kernel that sums n_serial terms of s per lane before a tree over n_threads lanes, all in fp32:
    (n_serial + log2(n_threads) + 4) 2^-24 on log s (the additions' relative errors, + exp, + log) and 3 x 2^-24 relative for the
    roundings of log s, m + log s and l - (m + log s)."""
    u = 2.0 ** -24
    return (n_serial + np.log2(n_threads) + 4) * u + 3 * u * np.maximum(np.maximum(np.abs(m), np.abs(m + log_s)), np.abs(logprob))


def shift_targets(ids, starts=None):
    """ids [B, T], starts [B] or None -> (targets [B, T]: ids shifted left by one, -1 at pad positions and at T - 1; valid [B, T - 1])"""
    ids = np.asarray(ids, dtype=np.int64)
    B, T = ids.shape
    s = np.zeros(B, np.int64) if starts is None else np.asarray(starts, np.int64)
    valid = np.arange(T - 1)[None, :] >= s[:, None]
    tg = np.full((B, T), -1, np.int64)
    tg[:, :-1] = np.where(valid, ids[:, 1:], -1)
    return tg, valid


def lm_eval_rolling_windows(token_list, prefix_token, max_seq_len, context_len=1):
    """lm_eval.utils.get_rolling_token_windows followed by make_disjoint_window, restated statement by statement"""
    assert 1 <= context_len <= max_seq_len
    out = []
    if not token_list:
        return out
    pred_len = max_seq_len - context_len + 1
    predicted = 0
    first_seq_len = min(max_seq_len, len(token_list))
    out.append(([prefix_token] + token_list[:first_seq_len - 1], token_list[:first_seq_len]))
    predicted += first_seq_len
    while predicted < len(token_list):
        window_pred_len = min(len(token_list) - predicted, pred_len)
        window_end = predicted + window_pred_len
        out.append((token_list[window_end - max_seq_len - 1:window_end - 1], token_list[window_end - window_pred_len:window_end]))
        predicted += window_pred_len
    return [(a[:len(a) - (len(b) - 1)], b) for a, b in out]


def loglikelihood(logprob_of, greedy_of, pairs, max_len):
    """[(sum, all greedy)] for pairs scored as (context + continuation)[-max_len:] through a scorer of WHOLE sequences:
    logprob_of(seq) / greedy_of(seq) give one value per target position 1 .. len(seq) - 1"""
    out = []
    for c, k in pairs:
        seq = (list(c) + list(k))[-max_len:]
        n = min(len(k), len(seq) - 1)
        out.append((float(np.sum(logprob_of(seq)[len(seq) - 1 - n:])), bool(np.all(greedy_of(seq)[len(seq) - 1 - n:]))))
    return out
