"""The penalties' NumPy restatement (penalty_ref.py) without a GPU: the repetition penalty against the installed transformers'
RepetitionPenaltyLogitsProcessor bit for bit, the presence / frequency terms against a float64 evaluation, the table builder
against a Python loop."""
import numpy as np
import pytest
import torch

from penalty_ref import COUNT_MAX, PROMPT_BIT, add_counts, bf16_to_f32, build_counts, f32_to_bf16, penalty_f32, penalty_ref


def _rows(seed, M, vocab):
    """bf16-valued fp32 rows with +-0, -inf and negative entries, and their patterns"""
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal((M, vocab)) * 4).astype(np.float32)
    x[:, 0], x[:, 1], x[:, 2], x[:, 3] = 0.0, -0.0, -np.inf, -1.0
    u = f32_to_bf16(x)
    return bf16_to_f32(u), u


@pytest.mark.parametrize("theta", [1.3, 0.8, 1.7, 2.0])
def test_repetition_against_hf_processor(theta):
    from transformers.generation import RepetitionPenaltyLogitsProcessor
    M, vocab = 6, 300
    x, _ = _rows(int(theta * 10), M, vocab)
    rs = np.random.RandomState(7)
    prev = rs.randint(0, vocab, size=(M, 40))
    prev[:, :4] = np.arange(4)                       # the +-0, -inf and -1 entries are among the penalised ones
    hf = RepetitionPenaltyLogitsProcessor(theta)(torch.from_numpy(prev), torch.from_numpy(x.copy())).numpy()
    # half of the history as prompt, half as generated: the repetition term sees their union (c != 0)
    table = build_counts(prev[:, :20], prev[:, 20:], vocab)
    mine = penalty_f32(x, table, theta, 0.0, 0.0)
    assert mine.dtype == np.float32
    assert (mine.view(np.uint32) == hf.view(np.uint32)).all()
    touched = np.zeros((M, vocab), dtype=bool)
    np.put_along_axis(touched, prev, True, axis=1)
    assert (mine.view(np.uint32)[~touched] == x.view(np.uint32)[~touched]).all()


@pytest.mark.parametrize("a_p,a_f", [(0.5, 0.0), (0.0, 0.25), (0.6, 0.3), (-0.5, -0.1)])
def test_presence_and_frequency_against_float64(a_p, a_f):
    M, vocab = 4, 257
    x, _ = _rows(3, M, vocab)
    rs = np.random.RandomState(11)
    table = np.zeros((M, vocab), dtype=np.uint16)
    table[:] = rs.choice(np.array([0, PROMPT_BIT, 1, PROMPT_BIT | 1, 5, 300, COUNT_MAX, 0xffff], dtype=np.uint16), size=(M, vocab))
    mine = penalty_f32(x, table, 1.0, a_p, a_f).astype(np.float64)
    n = (table & COUNT_MAX).astype(np.float64)
    exact = x.astype(np.float64) - float(np.float32(a_f)) * n - np.where(n > 0, float(np.float32(a_p)), 0.0)
    fin = np.isfinite(exact)
    assert (mine[~fin] == exact[~fin]).all()                        # -inf stays -inf
    # three fp32 roundings (product, two differences), each within half an ulp of a magnitude below |x| + |a_f| n + |a_p|
    scale = np.abs(x.astype(np.float64)) + abs(a_f) * n + abs(a_p)
    assert (np.abs(mine[fin] - exact[fin]) <= 3 * 2.0 ** -24 * scale[fin]).all()
    untouched = (table & COUNT_MAX) == 0
    assert (mine[untouched & fin] == x.astype(np.float64)[untouched & fin]).all()     # the prompt bit alone changes nothing here


def test_bf16_rounding_is_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.3895314e38, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert (f32_to_bf16(x) == want).all()
    rs = np.random.RandomState(5)
    y = (rs.standard_normal(4096) * 100).astype(np.float32)
    assert (f32_to_bf16(y) == torch.from_numpy(y).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)).all()
    assert (penalty_ref(f32_to_bf16(y)[None], np.zeros((1, 4096), np.uint16), 1.5, 0.5, 0.5) == f32_to_bf16(y)[None]).all()


def test_table_builder_against_a_loop():
    rs = np.random.RandomState(2)
    B, T, n, vocab, ldc = 5, 9, 14, 37, 40
    prompt = rs.randint(-1, vocab + 1, size=(B, T))              # -1 and vocab: ignored
    gen = rs.randint(0, 6, size=(B, n))                          # a small range: duplicates inside a row
    gen[0, :3] = (-1, vocab, vocab - 1)
    starts = np.array([0, 3, 8, 9, 1])
    table = build_counts(prompt, gen, vocab, ldc, starts)
    want = np.zeros((B, ldc), dtype=np.uint16)
    for b in range(B):
        for t in range(starts[b], T):
            if 0 <= prompt[b, t] < vocab:
                want[b, prompt[b, t]] |= PROMPT_BIT
        for t in range(n):
            if 0 <= gen[b, t] < vocab and (want[b, gen[b, t]] & COUNT_MAX) < COUNT_MAX:
                want[b, gen[b, t]] += 1
    assert (table == want).all() and (table[:, vocab:] == 0).all()
    # saturation, and the active rows of an update
    t2 = np.array([[32766, PROMPT_BIT | 32766, 7, 0]], dtype=np.uint16).repeat(2, axis=0)
    add_counts(t2, np.array([[0, 0, 0, 1, 1, 1, 2], [0, 1, 2, 3, 3, 3, 3]]), True, 4, active=np.array([1, 0]))
    assert t2[0].tolist() == [32767, PROMPT_BIT | 32767, 8, 0] and t2[1].tolist() == [32766, PROMPT_BIT | 32766, 7, 0]
