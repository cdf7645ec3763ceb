"""-m gpu: lia_lm_verify / lia_llama_lm_verify -- final norm + lm_head per chunk, the greedy token of every block position with the
suppress switch, and what a scripted draft block accepts of it -- against float64 and a NumPy restatement.

The hidden rows are chosen on the CPU: of a pool of random rows, those whose float64 logits (f64_ref norm + matmul) keep their
three largest values more than two bf16 quanta apart.  On such rows the argmax of correctly rounded bf16 logits IS the float64 argmax,
with the largest token suppressed too, so every comparison below is exact."""
import ctypes

import numpy as np
import pytest

import f64_ref as R
from test_gpu_kernel_variants import gpu  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

H, VOCAB, POOL = 256, 256, 6144
EPS = 1e-5
_POOLS = {}


def pool(family):
    """(hidden bits [n, H], norm w, norm b, emb bits, order [n, 3]: the three largest tokens of every kept row), computed once"""
    if family not in _POOLS:
        rs = np.random.RandomState(11 if family == "opt" else 12)
        hid = R.bits(R.rnd(1.5 * rs.randn(POOL, H)))
        emb = R.bits(R.rnd(0.05 * rs.randn(VOCAB, H)))
        nw = R.bits(R.rnd(1.0 + 0.1 * rs.randn(H)))
        nb = R.bits(R.rnd(0.05 * rs.randn(H)))
        normed = R.layernorm(hid, nw, nb, EPS) if family == "opt" else R.rmsnorm(hid, nw, EPS)
        logits = R.matmul(normed, emb)
        order = np.argsort(-logits, axis=1, kind="stable")[:, :4]
        top = np.take_along_axis(logits, order, axis=1)
        q = R.quantum(np.abs(top[:, 0]))
        keep = (top[:, 0] - top[:, 1] > 2 * q) & (top[:, 1] - top[:, 2] > 2 * q) & (top[:, 0] > 0)
        assert keep.sum() > POOL // 4
        _POOLS[family] = (hid[keep], nw, nb, emb, order[keep])
    return _POOLS[family]


def accept_ref(block, greedy, active):
    """the NumPy restatement: accepted [B], common, next [B]"""
    B, T = block.shape
    acc = np.full(B, T - 1, np.int32)
    for b in range(B):
        if active is None or active[b]:
            a = 0
            while a < T - 1 and block[b, a + 1] == greedy[b, a]:
                a += 1
            acc[b] = a
    common = int(acc.min())
    return acc, common, greedy[:, common].copy()


def scripted_block(greedy, wants, seed):
    """block_ids [B, T] that accepts wants[b] tokens on row b: matches up to there, one mismatch, then matches again"""
    B, T = greedy.shape
    blk = np.empty((B, T), np.int64)
    blk[:, 0] = np.random.RandomState(seed).randint(0, VOCAB, B)
    blk[:, 1:] = greedy[:, :T - 1]
    for b, a in enumerate(wants):
        if a < T - 1:
            blk[b, a + 1] ^= 1
    return blk


def build(family, B, T, n_suppress, seed):
    """rows for a [B, T] block, the suppressed token s and the expected greedy ids: s is the unsuppressed argmax of one row at every
    block position (suppressed below n_suppress, kept behind it)"""
    hid, nw, nb, emb, order = pool(family)
    rs = np.random.RandomState(seed)
    s = int(np.bincount(order[:, 0], minlength=VOCAB).argmax())
    with_s = np.flatnonzero(order[:, 0] == s)
    assert len(with_s) >= 1
    rows = rs.randint(0, hid.shape[0], (B, T))
    for t in range(T):
        rows[(t + seed) % B, t] = with_s[(t + seed) % len(with_s)]
    first, second = order[rows, 0], order[rows, 1]
    sup = np.arange(T)[None, :] < n_suppress
    greedy = np.where(sup & (first == s), second, first).astype(np.int64)
    return hid[rows.reshape(-1)], nw, nb, emb, s, greedy, first.astype(np.int64)


def dev(torch, bits, shape=None):
    t = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(torch.bfloat16)
    return t if shape is None else t.view(shape)


def run(torch, ctx, family, hidden, nw, nb, emb, block, s, n_suppress, active):
    hd, wd, bd, ed = dev(torch, hidden), dev(torch, nw), dev(torch, nb), dev(torch, emb)
    B, T = block.shape
    blk = torch.from_numpy(block).cuda()
    act = None if active is None else torch.from_numpy(np.asarray(active, np.int32)).cuda()
    torch.cuda.synchronize()
    if family == "opt":
        res = ctx.lm_verify(hd.view(B, T, H), wd, bd, ed, blk, EPS, s, n_suppress, act)
        _, gr = ctx.lm_score(hd, wd, bd, ed, torch.full((B * T,), -1, dtype=torch.int64, device="cuda"), EPS)
    else:
        res = ctx.llama_lm_verify(hd.view(B, T, H), wd, ed, blk, EPS, s, n_suppress, act)
        _, gr = ctx.llama_lm_score(hd, wd, ed, torch.full((B * T,), -1, dtype=torch.int64, device="cuda"), EPS)
    ctx.synchronize()
    return (res.greedy.cpu().numpy(), res.accepted.cpu().numpy(), int(res.common.cpu()[0]), res.next.cpu().numpy(),
            gr.cpu().numpy().reshape(B, T))


@pytest.mark.parametrize("family", ["opt", "llama"])
@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("T", [2, 5, 8])
def test_greedy_and_acceptance_exact(gpu, family, B, T):
    """greedy == the float64 argmax (with the suppressed positions) and, unsuppressed, lia_lm_score's greedy ids; accepted / common /
    next == the restatement, for blocks scripted to accept every count 0 .. T - 1 (a mismatch followed by matches), with inactive rows,
    n_suppress 0, 2 and T"""
    torch, _ = gpu
    from lia_amd import _native as N, ops
    ctx = ops.Context(0, N.lib().lia_lm_score_workspace_bytes(B * T, H, VOCAB))
    try:
        for n_suppress in (0, min(2, T), T):
            hidden, nw, nb, emb, s, greedy, first = build(family, B, T, n_suppress, 100 * B + T)
            if n_suppress:
                assert (greedy != first).any() and (greedy[:, :n_suppress] != s).all()
            if n_suppress < T:
                assert (greedy[:, n_suppress:] == s).any()            # the switch ends at n_suppress
            for shift in range(T):
                wants = [(b + shift) % T for b in range(B)]
                for active in (None, [(b + shift) % 3 != 0 for b in range(B)]):
                    block = scripted_block(greedy, wants, shift)
                    gr, acc, common, nxt, score_gr = run(torch, ctx, family, hidden, nw, nb, emb, block, s, n_suppress, active)
                    assert (gr == greedy).all(), (family, B, T, n_suppress, gr.tolist(), greedy.tolist())
                    assert (score_gr == first).all()
                    want_acc, want_common, want_next = accept_ref(block, greedy, active)
                    assert (acc == want_acc).all() and common == want_common and (nxt == want_next).all(), (acc.tolist(), want_acc.tolist())
                    live = [w for b, w in enumerate(wants) if active is None or active[b]]
                    assert common == (min(live) if live else T - 1)
    finally:
        ctx.close()


@pytest.mark.parametrize("family", ["opt", "llama"])
def test_a_block_the_chunk_rule_splits(gpu, family):
    """520 rows (104 x 5) in a workspace of 256-row chunks: three chunks, whose first rows sit at block positions 0, 1 and 2 -- the
    suppressed positions are those of the block, not of the chunk"""
    torch, _ = gpu
    from lia_amd import ops
    B, T, n_suppress = 104, 5, 2
    ctx = ops.Context(0, 512 + 256 * (2 * H + 2 * VOCAB) + 100)
    try:
        assert ctx.score_chunk_rows(B * T, H, VOCAB) == 256
        hidden, nw, nb, emb, s, greedy, first = build(family, B, T, n_suppress, 7)
        wants = [(3 * b) % T + (b % 2) for b in range(B)]
        wants = [min(w, T - 1) for w in wants]
        wants[17] = 1
        block = scripted_block(greedy, wants, 5)
        active = [b % 5 != 2 for b in range(B)]
        gr, acc, common, nxt, score_gr = run(torch, ctx, family, hidden, nw, nb, emb, block, s, n_suppress, active)
        assert (gr == greedy).all() and (score_gr == first).all()
        want_acc, want_common, want_next = accept_ref(block, greedy, active)
        assert (acc == want_acc).all() and common == want_common and (nxt == want_next).all()
    finally:
        ctx.close()


def test_argument_errors_by_name(gpu):
    torch, _ = gpu
    from lia_amd import _native as N, ops
    ctx = ops.Context(0, 1 << 20)
    try:
        hid = torch.zeros((6, 256), dtype=torch.bfloat16, device="cuda")
        w = torch.ones(256, dtype=torch.bfloat16, device="cuda")
        emb = torch.zeros((64, 256), dtype=torch.bfloat16, device="cuda")
        blk = torch.zeros((2, 3), dtype=torch.int64, device="cuda")
        gr = torch.zeros((2, 3), dtype=torch.int64, device="cuda")
        acc = torch.zeros(2, dtype=torch.int32, device="cuda")
        com = torch.zeros(1, dtype=torch.int32, device="cuda")
        nxt = torch.zeros(2, dtype=torch.int64, device="cuda")
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731

        def opt(hidden=hid, ldh=256, B=2, T=3, Hh=256, lnw=w, lnb=w, e=emb, vocab=64, sup=-1, n_sup=0, b=blk, g=gr, a=acc, c=com, n=nxt):
            return ctx.lib.lia_lm_verify(ctx.handle, p(hidden), ldh, B, T, Hh, p(lnw), p(lnb), p(e), vocab, 1e-5, sup, n_sup, p(b), None,
                                         p(g), p(a), p(c), p(n), None)

        def llama(hidden=hid, ldh=256, B=2, T=3, e=emb, sup=-1, n_sup=0, c=com):
            return ctx.lib.lia_llama_lm_verify(ctx.handle, p(hidden), ldh, B, T, 256, p(w), p(e), 64, 1e-5, sup, n_sup, p(blk), None,
                                               p(gr), p(acc), p(c), p(nxt), None)

        assert opt() == N.LIA_OK and llama() == N.LIA_OK
        ctx.synchronize()
        for kw, name in ((dict(hidden=None), "NULL hidden"), (dict(lnw=None), "NULL norm weight"), (dict(lnb=None), "NULL norm bias"),
                         (dict(e=None), "NULL lm_head weight"), (dict(b=None), "NULL block_ids"), (dict(g=None), "NULL greedy"),
                         (dict(a=None), "NULL accepted"), (dict(c=None), "NULL common"), (dict(n=None), "NULL next"),
                         (dict(B=0), "B=0"), (dict(T=1), "T=1"), (dict(n_sup=-1), "n_suppress=-1"), (dict(n_sup=4), "n_suppress=4"),
                         (dict(sup=64), "suppress_token=64"), (dict(sup=-2), "suppress_token=-2"), (dict(Hh=200), "H=200"),
                         (dict(vocab=40), "vocab=40"), (dict(ldh=128), "ldh=128"), (dict(ldh=260), "ldh=260")):
            assert opt(**kw) == N.LIA_ERR_INVALID, name
            err = ctx.lib.lia_last_error().decode()
            assert name in err and "lia_lm_verify" in err, (name, err)
        for kw, name in ((dict(hidden=None), "NULL hidden"), (dict(c=None), "NULL common"), (dict(T=1), "T=1"), (dict(n_sup=4), "n_suppress=4"),
                         (dict(sup=64), "suppress_token=64"), (dict(ldh=128), "ldh=128")):
            assert llama(**kw) == N.LIA_ERR_INVALID, name
            err = ctx.lib.lia_last_error().decode()
            assert name in err and "lia_llama_lm_verify" in err, (name, err)
        # a workspace that holds no 256-row chunk: a size check on the host, nothing is launched
        big_emb = torch.zeros((50272, 256), dtype=torch.bfloat16, device="cuda")
        big_hid = torch.zeros((100, 3, 256), dtype=torch.bfloat16, device="cuda")
        big_blk = torch.zeros((100, 3), dtype=torch.int64, device="cuda")
        with pytest.raises(MemoryError, match="lia_lm_verify: .* holds no chunk of 256 rows"):
            ctx.lm_verify(big_hid, w, w, big_emb, big_blk)
        with pytest.raises(ValueError, match="active has 3 entries"):
            ctx.lm_verify(hid.view(2, 3, 256), w, w, emb, blk, active=torch.zeros(3, dtype=torch.int32, device="cuda"))
    finally:
        ctx.close()
