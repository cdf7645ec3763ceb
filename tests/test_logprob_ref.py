"""The float64 reference of the top-N log-probability kernel (tests/logprob_ref.py) against a brute-force sort."""
import functools

import numpy as np

import logprob_ref as LR
import score_ref as SR
import synth


def _bits(x):
    return synth.f32_to_bf16_bits(np.asarray(x, np.float32))


def _brute(bits_row, n_top):
    """ids of one row by an explicit comparison sort: larger value first; +0.0 above -0.0; equal bit patterns by the lower id"""
    x = SR.bf16_to_f64(bits_row)

    def before(a, b):
        if x[a] != x[b]:
            return -1 if x[a] > x[b] else 1
        sa, sb = bits_row[a] >> 15, bits_row[b] >> 15          # (only +-0.0 compare equal with different bits)
        if sa != sb:
            return -1 if sa < sb else 1
        return -1 if a < b else 1
    return sorted(range(len(x)), key=functools.cmp_to_key(before))[:n_top]


def test_key_is_monotonic_in_the_value_over_every_non_nan_pattern():
    bits = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    x = SR.bf16_to_f64(bits)
    fin = ~np.isnan(x)
    k, v = LR.key_of(bits[fin]), x[fin]
    o = np.argsort(k, kind="stable")
    assert (np.diff(v[o]) >= 0).all()
    assert LR.key_of(np.array([0x0000], np.uint16))[0] > LR.key_of(np.array([0x8000], np.uint16))[0]       # +0.0 above -0.0
    assert LR.key_of(np.array([0xFF80], np.uint16))[0] == 0x007F                                           # -inf: the lowest non-NaN key


def test_reference_against_a_brute_force_sort():
    rs = np.random.RandomState(3)
    vocab = 97
    rows = [2.0 * rs.standard_normal(vocab),
            np.round(1.5 * rs.standard_normal(vocab)),                                   # many ties
            np.full(vocab, 0.75),                                                        # every logit equal
            np.where(rs.rand(vocab) < 0.5, -np.inf, rs.standard_normal(vocab)),          # runs of -inf
            np.where(np.arange(vocab) % 31 == 5, rs.standard_normal(vocab), -np.inf),    # 3 finite logits: fewer than N
            np.where(rs.rand(vocab) < 0.5, 0.0, -0.0)]                                   # +-0.0
    bits = _bits(np.stack(rows))
    ids = rs.randint(0, vocab, len(rows))
    ids[0] = -1
    for n in (0, 1, 5, 32, vocab):
        chosen, top_ids, top_lp, m, ls = LR.topn_logprobs(bits, ids, n)
        assert top_ids.shape == (len(rows), n) and top_lp.shape == (len(rows), n)
        full = SR.log_softmax(SR.bf16_to_f64(bits))
        for r in range(len(rows)):
            want = _brute(bits[r], n)
            assert top_ids[r].tolist() == want, (n, r)
            assert (top_lp[r] == full[r, want]).all()
        assert chosen[0] == 0.0
        assert (chosen[1:] == full[np.arange(1, len(rows)), ids[1:]]).all()
    chosen, top_ids, top_lp, _, _ = LR.topn_logprobs(bits, ids, 5)
    assert top_ids[2].tolist() == [0, 1, 2, 3, 4]                                        # all equal: ids 0 .. N - 1
    assert sorted(top_ids[4, :3].tolist()) == [5, 36, 67]
    assert np.isfinite(top_lp[4, :3]).all() and (top_lp[4, 3:] == -np.inf).all()
    assert top_ids[4, 3:].tolist() == [0, 1]                                             # the -inf tail: still in id order
    assert abs(np.exp(top_lp[2]).sum() - 5.0 / vocab) < 1e-12
