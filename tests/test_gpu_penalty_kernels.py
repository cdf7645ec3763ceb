"""-m gpu: lia_penalty_kernel and lia_token_counts_kernel through the C ABI (lia_apply_penalties, lia_token_counts_add,
include/lia_hip.h) against penalty_ref.py.  Every comparison is exact: the bf16 patterns byte for byte, the count words bit for bit."""
import ctypes

import numpy as np
import pytest

import penalty_ref as PR

pytestmark = pytest.mark.gpu

SETTINGS = [(1.3, 0.0, 0.0), (0.8, 0.0, 0.0), (1.0, 0.5, 0.0), (1.0, 0.0, 0.25), (1.7, 0.6, 0.3), (1.0, -0.5, -0.1)]
WORDS = np.array([0, 0x8000, 1, 0x8001, 0x7fff, 0xffff], dtype=np.uint16)
# (M, vocab, ld, ldc): the 16-byte path on OPT's and Llama-3's vocabularies, the scalar path with an odd ld, a row shorter than one
# 16-byte group, more rows than a head call holds at 64 columns (one column tile, the grid's row dimension), and more rows than that
# dimension of a grid can have (65535: the kernel's row loop goes round)
SHAPES = [(3, 50272, 50272, 50272), (1, 128256, 128256, 128256), (5, 1000, 1003, 1002), (2, 7, 8, 8), (257, 64, 64, 64),
          (65600, 16, 16, 16)]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    from lia_amd import ops
    c = ops.Context(0, 1 << 20)
    yield c
    c.close()


def _dev(torch, u16):
    return torch.from_numpy(np.ascontiguousarray(u16).view(np.int16)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint16)


def _logit_rows(M, vocab, seed):
    """bf16 patterns [M, vocab]: normal values with +-0, -inf, +inf, large magnitudes and exact ties planted in every row (of the first 300)"""
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal((M, vocab)) * 3).astype(np.float32)
    special = np.array([0.0, -0.0, -np.inf, np.inf, 3.0e38, -3.0e38, 1.0e30, -65280.0, 2.5, 2.5, -2.5, -2.5], dtype=np.float32)
    for r in range(min(M, 300)):
        at = rs.choice(vocab, size=min(vocab, len(special)), replace=False)
        x[r, at] = special[:len(at)]
    if vocab >= 64:
        x[:, -9:] = x[:, :9]                                # ties across the row, the last group of 8 included
    return PR.f32_to_bf16(x)


def _count_rows(M, vocab, ldc, seed):
    """every word of the issue's list next to every logit kind (random placement), small and mid counts between them; the padding
    columns at and beyond vocab hold garbage that must not matter"""
    rs = np.random.RandomState(seed)
    pool = np.concatenate([WORDS, WORDS, np.array([2, 5, 300, 0x8005, 0x812c], dtype=np.uint16)])
    c = rs.choice(pool, size=(M, ldc))
    c[:, vocab:] = 0xffff
    return c.astype(np.uint16)


@pytest.mark.parametrize("M,vocab,ld,ldc", SHAPES)
def test_apply_penalties_against_the_reference(ctx, M, vocab, ld, ldc):
    import torch
    from lia_amd import _native as N
    lg = _logit_rows(M, vocab, 17 + vocab)
    cnt = _count_rows(M, vocab, ldc, 29 + vocab)
    for w in WORDS:
        assert (cnt[:, :vocab] == w).any() or vocab < 8
    lg_pad = np.full((M, ld), 0x1234, dtype=np.uint16)
    lg_pad[:, :vocab] = lg
    cnt_dev = _dev(torch, cnt)
    ldo = ld + 8 if ld % 8 == 0 else ld - 2                 # another pitch: a multiple of 8 on the wide path, 1001 on the scalar one
    assert ldo >= vocab and ldo != ld
    st = ctypes.c_void_p(ctx.stream)
    for s in SETTINGS:
        want = PR.penalty_ref(lg, cnt, *s)
        # out of place, ldo != ld: the columns beyond vocab keep their bytes, the input is not touched
        src = _dev(torch, lg_pad)
        out = torch.full((M, ldo), 0x5a5a, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        N.check(ctx.lib.lia_apply_penalties(ctx.handle, _p(src), ld, M, vocab, _p(cnt_dev), ldc, *s, _p(out), ldo, st), "lia_apply_penalties")
        ctx.synchronize()
        got = _host(out)
        assert (got[:, :vocab] == want).all(), (s, np.argwhere(got[:, :vocab] != want)[:4])
        assert (got[:, vocab:] == 0x5a5a).all() and (_host(src) == lg_pad).all()
        # in place
        N.check(ctx.lib.lia_apply_penalties(ctx.handle, _p(src), ld, M, vocab, _p(cnt_dev), ldc, *s, _p(src), ld, st), "lia_apply_penalties")
        ctx.synchronize()
        got = _host(src)
        assert (got[:, :vocab] == want).all() and (got[:, vocab:] == 0x1234).all(), s
        assert (_host(cnt_dev) == cnt).all()
    # the properties the semantics name: a zero word changes nothing, +-inf stay, ties with equal words stay ties
    want = PR.penalty_ref(lg, cnt, 1.7, 0.6, 0.3)
    zero = cnt[:, :vocab] == 0
    assert (want[zero] == lg[zero]).all()
    inf = (lg & 0x7fff) == 0x7f80
    assert (want[inf] == lg[inf]).all()


def test_apply_penalties_wrapper_and_misaligned_bases(ctx):
    """ops.Context.apply_penalties on strided rows; a base that is only 2-byte aligned with pitches that are multiples of 8 takes
    the scalar path and gives the same bytes"""
    import torch
    M, vocab = 4, 264
    lg = _logit_rows(M, vocab, 3)
    cnt = _count_rows(M, vocab, vocab, 4)
    want = PR.penalty_ref(lg, cnt, 1.7, 0.6, 0.3)
    wide = torch.zeros((M, vocab + 24), dtype=torch.bfloat16, device="cuda")
    wide.view(torch.int16)[:, 8:8 + vocab] = _dev(torch, lg)
    torch.cuda.synchronize()
    for off in (8, 9):                                      # column offset 9: rows start 2 bytes past a 16-byte boundary
        wide.view(torch.int16)[:, off:off + vocab] = _dev(torch, lg)
        torch.cuda.synchronize()
        out = ctx.apply_penalties(wide[:, off:off + vocab], _dev(torch, cnt), 1.7, 0.6, 0.3)
        ctx.synchronize()
        assert (_host(out.view(torch.int16)) == want).all(), off
    neutral = ctx.apply_penalties(wide[:, 9:9 + vocab], _dev(torch, cnt), 1.0, 0.0, 0.0)
    ctx.synchronize()
    assert (_host(neutral.view(torch.int16)) == lg).all()      # theta 1, alpha 0: x / 1 - 0 - 0 is x for every word


@pytest.mark.parametrize("generated", [0, 1])
def test_token_counts_against_numpy(ctx, generated):
    """duplicates inside a row (also one id 300 times: every thread of a workgroup on one word), first skipping, inactive rows, ids
    at -1 and at vocab, even and odd neighbours -- on a table that already holds words of every kind"""
    import torch
    from lia_amd import _native as N
    B, n, vocab, ldc, ldi = 5, 300, 1000, 1002, 304
    rs = np.random.RandomState(5 + generated)
    ids = np.full((B, ldi), 7, dtype=np.int64)                          # (the pitch's tail is never read as an id of the row)
    ids[:, :n] = rs.randint(0, 40, size=(B, n))                         # a small range: duplicates, even and odd neighbours
    ids[0, :6] = (-1, vocab, vocab - 1, 0, vocab + 5, -7)
    ids[3, :n] = 501                                                    # one word, 300 times
    ids[4, :n] = rs.randint(0, vocab, size=n)
    first = np.array([0, 5, 299, 0, 17], dtype=np.int32)
    active = np.array([1, 1, 1, 1, 0], dtype=np.int32)
    table = rs.choice(np.array([0, 0x8000, 1, 0x8001, 40, 0x8028], dtype=np.uint16), size=(B, ldc)).astype(np.uint16)
    for use_first, use_active in ((False, False), (True, False), (False, True), (True, True)):
        dev = _dev(torch, table)
        ids_dev = torch.from_numpy(ids).cuda()
        f = torch.from_numpy(first).cuda() if use_first else None
        a = torch.from_numpy(active).cuda() if use_active else None
        torch.cuda.synchronize()
        N.check(ctx.lib.lia_token_counts_add(ctx.handle, _p(dev), ldc, B, vocab, _p(ids_dev), ldi, n, _p(f), _p(a), generated,
                                             ctypes.c_void_p(ctx.stream)), "lia_token_counts_add")
        ctx.synchronize()
        want = PR.add_counts(table.copy(), ids[:, :n], bool(generated), vocab, first if use_first else None, active if use_active else None)
        got = _host(dev)
        assert (got == want).all(), (use_first, use_active, np.argwhere(got != want)[:4])
        assert (got[:, vocab:] == table[:, vocab:]).all()
        if generated and not use_first:
            assert (got[3, 501] & 0x7fff) == (table[3, 501] & 0x7fff) + 300
        if use_active:
            assert (got[4] == table[4]).all()


def test_token_counts_saturate_and_keep_the_neighbour(ctx):
    """a word uploaded at 32766 that receives the same id three times ends at 32767; its neighbour in the same 32-bit location and its
    own bit 15 do not change -- for an even and an odd word, with and without the prompt bit; the wrapper's call"""
    import torch
    vocab = 16
    table = np.zeros((2, vocab), dtype=np.uint16)
    table[0, 4:8] = (32766, 0x1234, 0x8abc, 0x8000 | 32766)            # even word 4 next to 5; odd word 7 next to 6
    table[1, 4:8] = (0xffff, 32766, 32766, 0x7fff)
    ids = np.array([[4, 7, 4, 7, 4, 7], [5, 5, 5, 9, 4, 7]], dtype=np.int64)
    dev = _dev(torch, table)
    ctx.token_counts_add(dev, torch.from_numpy(ids).cuda(), True, vocab=vocab)
    ctx.synchronize()
    got = _host(dev)
    want = PR.add_counts(table.copy(), ids, True, vocab)
    assert (got == want).all()
    assert got[0, 4:8].tolist() == [32767, 0x1234, 0x8abc, 0x8000 | 32767]
    assert got[1, 4:8].tolist() == [0xffff, 32767, 32766, 0x7fff] and got[1, 9] == 1
    # the prompt bit on saturated and neighbouring words
    ctx.token_counts_add(dev, torch.from_numpy(ids).cuda(), False, vocab=vocab)
    ctx.synchronize()
    assert (_host(dev) == PR.add_counts(want.copy(), ids, False, vocab)).all()


def test_c_refusals_by_name(ctx):
    import torch
    from lia_amd import _native as N
    M, vocab = 2, 64
    lg = torch.zeros((M, vocab), dtype=torch.bfloat16, device="cuda")
    cnt = torch.zeros((M, vocab + 2), dtype=torch.int16, device="cuda")
    ids = torch.zeros((M, 4), dtype=torch.int64, device="cuda")
    err = lambda: ctx.lib.lia_last_error().decode()                     # noqa: E731
    st = ctypes.c_void_p(ctx.stream)
    inf, nan = float("inf"), float("nan")

    def apply(theta=1.2, a_p=0.0, a_f=0.0, logits=lg, ld=vocab, counts=cnt, ldc=vocab + 2, out=lg, ldo=vocab, M=M, V=vocab, off=0):
        c = None if counts is None else ctypes.c_void_p(counts.data_ptr() + off)
        return ctx.lib.lia_apply_penalties(ctx.handle, _p(logits), ld, M, V, c, ldc, theta, a_p, a_f, _p(out), ldo, st)

    for kw, text in ((dict(theta=0.0), "repetition=0 must be finite and > 0"), (dict(theta=-1.0), "repetition=-1"), (dict(theta=inf), "repetition=inf"),
                     (dict(theta=nan), "repetition=nan"), (dict(a_p=nan), "presence=nan must be finite"), (dict(a_p=-inf), "presence=-inf"),
                     (dict(a_f=inf), "frequency=inf must be finite"), (dict(ldc=vocab + 1), f"ldc={vocab + 1} must be even"),
                     (dict(ldc=vocab - 2), f"ldc={vocab - 2} < vocab={vocab}"), (dict(off=2), "is not 4-byte aligned"),
                     (dict(ld=vocab - 1), f"ld={vocab - 1} < vocab"), (dict(ldo=vocab - 8), f"ldo={vocab - 8} < vocab"),
                     (dict(M=0), "M=0 must be >= 1"), (dict(V=0), "vocab=0 must be >= 1"), (dict(logits=None), "NULL logits"),
                     (dict(counts=None), "NULL counts"), (dict(out=None), "NULL out")):
        assert apply(**kw) == N.LIA_ERR_INVALID, kw
        assert err().startswith("lia_apply_penalties: ") and text in err(), (kw, err())
    assert apply() == N.LIA_OK

    def add(counts=cnt, ldc=vocab + 2, rows=M, V=vocab, idt=ids, ldi=4, n=4, generated=1, off=0):
        c = None if counts is None else ctypes.c_void_p(counts.data_ptr() + off)
        return ctx.lib.lia_token_counts_add(ctx.handle, c, ldc, rows, V, _p(idt), ldi, n, None, None, generated, st)

    for kw, text in ((dict(ldc=vocab + 1), "must be even"), (dict(ldc=vocab - 2), f"ldc={vocab - 2} < vocab={vocab}"), (dict(off=2), "is not 4-byte aligned"),
                     (dict(rows=0), "rows=0 must be >= 1"), (dict(V=0), "vocab=0"), (dict(ldi=3), "ldi=3 >= n"), (dict(n=-1), "n=-1"),
                     (dict(generated=2), "generated=2 must be 0 (prompt) or 1 (generated)"), (dict(counts=None), "NULL counts"),
                     (dict(idt=None), "NULL ids")):
        assert add(**kw) == N.LIA_ERR_INVALID, kw
        assert err().startswith("lia_token_counts_add: ") and text in err(), (kw, err())
    assert add(n=0) == N.LIA_OK and add() == N.LIA_OK
    ctx.synchronize()

    scratch = torch.zeros((M, vocab), dtype=torch.bfloat16, device="cuda")

    def set_(theta=1.2, a_p=0.0, a_f=0.0, ldc=vocab + 2, rows=M, scr=scratch, lds=vocab, off=0):
        return ctx.lib.lia_ctx_set_penalties(ctx.handle, ctypes.c_void_p(cnt.data_ptr() + off), ldc, rows, theta, a_p, a_f, _p(scr), lds)

    try:
        for kw, text in ((dict(theta=0.0), "repetition=0"), (dict(theta=nan), "repetition=nan"), (dict(a_p=inf), "presence=inf"),
                         (dict(a_f=nan), "frequency=nan"), (dict(ldc=vocab + 1), "must be even"), (dict(off=2), "is not 4-byte aligned"),
                         (dict(rows=0), "rows=0"), (dict(scr=None), "NULL scratch with a count table"), (dict(lds=0), "lds=0")):
            assert set_(**kw) == N.LIA_ERR_INVALID, kw
            assert err().startswith("lia_ctx_set_penalties: ") and text in err(), (kw, err())
        # what only the head call can check: the pitches against the vocabulary, the rows against the table
        u = torch.rand(M, device="cuda")
        torch.cuda.synchronize()
        assert set_(ldc=vocab - 2) == N.LIA_OK
        with pytest.raises(ValueError, match=f"lia_sample: the count table has ldc={vocab - 2} words per row, vocab={vocab}"):
            ctx.sample(lg, 1.0, 0, 1.0, u)
        assert set_(lds=vocab - 8) == N.LIA_OK
        with pytest.raises(ValueError, match=f"lia_sample: the penalty scratch has lds={vocab - 8} values per row, vocab={vocab}"):
            ctx.sample(lg, 1.0, 0, 1.0, u)
        assert set_(rows=1) == N.LIA_OK
        with pytest.raises(ValueError, match="lia_sample: the call has 2 rows, the count table 1"):
            ctx.sample(lg, 1.0, 0, 1.0, u)
        assert set_() == N.LIA_OK
        ctx.sample(lg, 1.0, 0, 1.0, u)
        ctx.synchronize()
    finally:
        ctx.set_penalties(None)
    # the wrapper's own refusals
    for bad in (torch.zeros((M, vocab), dtype=torch.int32, device="cuda"), torch.zeros((M, vocab), dtype=torch.int16), [1, 2]):
        with pytest.raises(ValueError, match="count table: expected a 16-bit integer CUDA tensor"):
            ctx.set_penalties(bad)
    with pytest.raises(ValueError, match="penalty scratch: expected a bf16 CUDA tensor"):
        ctx.set_penalties(cnt, 1.2, scratch=torch.zeros((1, vocab), dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(ValueError, match="lia_ctx_set_penalties: repetition=0"):
        ctx.set_penalties(cnt, 0.0)
    assert ctx._penalties is None
