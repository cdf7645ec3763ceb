"""-m gpu: lia_topn_logprobs_kernel and the log-probability sink of the head calls (lia_ctx_set_logprob_sink, include/lia_hip.h)
through the C ABI.

The ids are compared exactly with tests/logprob_ref.py; every value is compared BIT FOR BIT with lia_token_logprobs on the same
logits (the two kernels share their passes) and, against float64, within score_ref.row_kernel_bound -- the bound
tests/test_gpu_scoring.py applies to that kernel.  -inf compares exactly."""
import ctypes

import numpy as np
import pytest

import logprob_ref as LR
import score_ref as SR
import synth
from test_gpu_token_mask import EPS, H, _head_inputs, _lm_head, _p

pytestmark = pytest.mark.gpu

TILE = 8192                  # tokens per token-ordered tile of the row kernels: 1024 threads x 8


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    from lia_amd import ops
    c = ops.Context(0, 64 << 20)
    yield c
    c.close()


def _dev(torch, bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(torch.bfloat16)


def _i32(t):
    import torch
    return t.contiguous().view(torch.int32).cpu().numpy()


def tie_positions(vocab):
    """the ids of one tie group, those that exist in a row of `vocab` tokens: neighbours inside a lane's 8 tokens (3, 4), the next
    lane (11, 12), another wave (515, 520), and a run that begins 18 ids below the boundary of the first token tile and crosses it
    (below the middle of a row that has one tile only) -- so that the first 29 members in id order end behind the boundary"""
    edge = TILE if vocab > TILE else vocab // 2
    return sorted({p for p in [3, 4, 11, 12, 515, 520] + list(range(max(20, edge - 18), edge + 30)) if p < vocab})


def families(vocab, n_top, seed):
    """name -> one row of float32 logits: the row families of the kernel's contract"""
    rs = np.random.RandomState(seed)
    rows = {"random": 2.0 * rs.standard_normal(vocab), "all equal": np.full(vocab, 1.25)}
    # a tie group that straddles the n_top-th place: 3 distinct values above it, then more equal ones than places are left
    tie = -1.0 - np.abs(rs.standard_normal(vocab))
    pos = tie_positions(vocab)
    tie[pos] = 3.0
    free = [i for i in range(vocab) if i not in set(pos)]
    for j, i in enumerate(rs.permutation(free)[:3]):
        tie[i] = 4.0 + j
    rows["ties across the n-th place"] = tie
    last = 0.5 * rs.standard_normal(vocab)
    last[vocab - 1] = 9.0
    rows["maximum in the last element"] = last
    holes = np.full(vocab, -np.inf)
    keep = rs.permutation(vocab)[:3]
    holes[keep] = rs.standard_normal(len(keep))
    rows["fewer finite logits than N"] = holes
    runs = 2.0 * rs.standard_normal(vocab)
    runs[vocab // 4:vocab // 2] = -np.inf
    runs[rs.rand(vocab) < 0.3] = -np.inf
    runs[vocab - 1] = 0.25
    rows["runs of -inf"] = runs
    zeros = np.where(rs.rand(vocab) < 0.5, 0.0, -0.0) + np.where(rs.rand(vocab) < 0.3, -1.5, 0.0)
    rows["+-0.0"] = zeros
    return rows


def _layouts(torch, logits):
    """the rows in a 16-byte aligned pitch (the 16-byte loads when vocab % 8 == 0), in a pitch that is no multiple of 8, and behind a
    base offset by one element: (name, device view [M, vocab]); +inf stands in every gap, a read of it would show"""
    M, vocab = logits.shape
    out = []
    for name, gap, off in (("aligned", 24, 0), ("odd pitch", 3, 0), ("base + 1", 24, 1)):
        ld = vocab + gap
        buf = np.full(M * ld + 8, 0x7f80, np.uint16)
        for r in range(M):
            buf[off + r * ld:off + r * ld + vocab] = logits[r]
        d = _dev(torch, buf)
        out.append((name, d[off:off + M * ld].view(M, ld)[:, :vocab]))
    return out


def _check_rows(torch, ctx, view, logits, ids, n_top, tag):
    """one launch on `view` (device rows of `logits`) against the reference and against lia_token_logprobs"""
    from lia_amd import _native as N
    M, vocab = logits.shape
    ids_dev = torch.from_numpy(ids).cuda()
    torch.cuda.synchronize()
    chosen, top_ids, top_lp = ctx.topn_logprobs(view, ids_dev, n_top)
    same, _ = ctx.token_logprobs(view, ids_dev)
    ctx.synchronize()                                        # (torch's stream slices what the library's stream wrote)
    columns = [top_ids[:, j].contiguous() for j in range(n_top)]
    torch.cuda.synchronize()
    per_top = [ctx.token_logprobs(view, c)[0] for c in columns]
    ctx.synchronize()
    want_c, want_ids, want_lp, m, ls = LR.topn_logprobs(logits, ids, n_top)
    got_ids = top_ids.cpu().numpy()
    assert got_ids.shape == (M, n_top) and (got_ids == want_ids).all(), (tag, np.argwhere(got_ids != want_ids)[:4].tolist())
    # bit for bit lia_token_logprobs' values
    assert (_i32(chosen) == _i32(same)).all(), tag
    for j in range(n_top):
        assert (_i32(top_lp[:, j]) == _i32(per_top[j])).all(), (tag, j)
    # within the row kernel's bound of float64; -inf exactly; an id outside the row gives 0.0
    got_c = chosen.cpu().numpy().astype(np.float64)
    got_lp = top_lp.cpu().numpy().astype(np.float64)
    outside = (ids < 0) | (ids >= vocab)
    assert (got_c[outside] == 0.0).all() and (want_c[outside] == 0.0).all()
    worst = 0.0
    for got, want in [(got_c, want_c)] + [(got_lp[:, j], want_lp[:, j]) for j in range(n_top)]:
        inf = np.isneginf(want)
        assert (got[inf] == want[inf]).all(), tag
        fin = np.isfinite(want)
        bound = SR.row_kernel_bound(m, ls, want, N.score_serial_terms(vocab), N.SCORE_ROW_THREADS)
        err = np.abs(got[fin] - want[fin])
        assert (err <= bound[fin]).all(), (tag, err.max(), bound[fin].min())
        if fin.any():
            worst = max(worst, float(np.max(err / bound[fin])))
    return worst, got_ids, got_lp


@pytest.mark.parametrize("vocab", [1, 7, 8, 1000, TILE + 8, 50272])
def test_kernel_against_reference(ctx, vocab):
    """vocab 1, 7 (scalar loads), 8 (one 16-byte load), 1000, 8192 + 8 (a second token tile), 50272; N in 0, 1, 5, 32 and vocab where
    those fit; every row family in one launch per layout, and launches of M = 1 .. 5 rows."""
    import torch
    worst = 0.0
    for n_top in sorted({n for n in (0, 1, 5, 32, vocab if vocab <= 32 else 0) if n <= vocab}):
        fam = families(vocab, n_top, 11 * vocab + n_top)
        names = list(fam)
        logits = synth.f32_to_bf16_bits(np.stack([fam[k] for k in names]).astype(np.float32))
        M = logits.shape[0]
        rs = np.random.RandomState(vocab + n_top)
        ids = rs.randint(0, vocab, M).astype(np.int64)
        ids[0], ids[1] = -1, vocab                                       # no token, and one past the row
        ids[names.index("maximum in the last element")] = vocab - 1
        for lname, view in _layouts(torch, logits):
            w, got_ids, got_lp = _check_rows(torch, ctx, view, logits, ids, n_top, (vocab, n_top, lname))
            worst = max(worst, w)
            if n_top:
                assert got_ids[names.index("all equal")].tolist() == list(range(n_top))
                assert got_ids[names.index("maximum in the last element"), 0] == vocab - 1
                fin = np.isfinite(got_lp[names.index("fewer finite logits than N")])
                assert fin.sum() == min(3, vocab, n_top) and fin[:fin.sum()].all()
        if n_top in (5, vocab):
            aligned = _layouts(torch, logits)[0][1]
            for m_rows in range(1, 6):
                _check_rows(torch, ctx, aligned[:m_rows], logits[:m_rows], ids[:m_rows], n_top, (vocab, n_top, "M", m_rows))
    print(f"\ntop-N kernel vocab {vocab}: max |err| / bound {worst:.3f}")


@pytest.mark.parametrize("n_top", [5, 32])
def test_more_than_65535_tokens_at_the_boundary_key_before_the_last_one_above_it(ctx, n_top):
    """vocab 128256 (Llama-3-8B's), where a row can hold more than 2^16 tokens AT the boundary key in front of a token above it -- a
    count that 16 bits do not hold: every logit equal but a larger one in the last element (the answer is the last id, then ids
    0 .. N - 2); the same with the larger ones in the last three elements; 128000 leading -inf logits, then three finite ones near
    the end (the finite ones, then ids 0, 1, ... of the -inf run in id order); and a tie group of 70000 members below three larger
    logits in the last tile"""
    import torch
    vocab = 128256
    rs = np.random.RandomState(n_top)
    last = np.full(vocab, 1.25)
    last[vocab - 1] = 3.0
    last3 = np.full(vocab, -0.5)
    last3[vocab - 3:] = [2.0, 4.0, 3.0]
    holes = np.full(vocab, -np.inf)
    holes[[128000, 128100, vocab - 1]] = [0.5, 1.5, 1.0]
    group = -3.0 - np.abs(rs.standard_normal(vocab))
    group[:70000] = 2.0
    group[[vocab - 9, vocab - 700, vocab - 5000]] = [5.0, 6.0, 7.0]
    logits = synth.f32_to_bf16_bits(np.stack([last, last3, holes, group]).astype(np.float32))
    ids = np.array([0, vocab - 1, 128100, 69999], np.int64)
    _, got, got_lp = _check_rows(torch, ctx, _layouts(torch, logits)[0][1], logits, ids, n_top, (vocab, n_top, "2^16"))
    assert got[0].tolist() == [vocab - 1] + list(range(n_top - 1))
    assert got[1].tolist() == [vocab - 2, vocab - 1, vocab - 3] + list(range(n_top - 3))
    assert got[2].tolist() == [128100, vocab - 1, 128000] + list(range(n_top - 3)) and np.isneginf(got_lp[2, 3:]).all()
    assert got[3].tolist() == [vocab - 5000, vocab - 700, vocab - 9] + list(range(n_top - 3))


def test_the_tie_group_really_straddles_lanes_waves_and_tiles(ctx):
    """the tie family at vocab 8192 + 8, N = 5: three distinct logits above a group of equal ones at ids 3, 4 (one lane), 11 (the next
    lane), 515 (another wave), 8191 / 8192 (two tiles) ...; the two places left go to ids 3 and 4, and with N = 32 the group's
    members in id order across the tile boundary"""
    import torch
    vocab = TILE + 8
    for n_top, take in ((5, 2), (32, 29)):
        row = families(vocab, n_top, 5)["ties across the n-th place"]
        logits = synth.f32_to_bf16_bits(row[None, :].astype(np.float32))
        pos = tie_positions(vocab)
        assert {3, 4, 11, 515, TILE - 1, TILE} <= set(pos) and len(pos) > take
        torch.cuda.synchronize()
        _, top_ids, top_lp = ctx.topn_logprobs(_dev(torch, logits), torch.zeros(1, dtype=torch.int64, device="cuda"), n_top)
        ctx.synchronize()
        got = top_ids.cpu().numpy()[0]
        assert got[3:].tolist() == pos[:take], (n_top, got.tolist())
        assert (np.diff(top_lp.cpu().numpy()[0]) <= 0).all()
        if n_top == 32:
            assert TILE - 1 in got and TILE in got


def test_a_row_of_nothing_but_minus_inf_gives_nan(ctx):
    import torch
    logits = np.full((1, 64), 0xFF80, np.uint16)
    torch.cuda.synchronize()
    chosen, top_ids, top_lp = ctx.topn_logprobs(_dev(torch, logits), torch.zeros(1, dtype=torch.int64, device="cuda"), 3)
    same, _ = ctx.token_logprobs(_dev(torch, logits), torch.zeros(1, dtype=torch.int64, device="cuda"))
    ctx.synchronize()
    assert torch.isnan(chosen).all() and torch.isnan(same).all() and torch.isnan(top_lp).all()
    assert top_ids.cpu().tolist() == [[0, 1, 2]]


# ---- the heads -------------------------------------------------------------------------------------------------------------------
def _sink(torch, ctx, n_top, shape):
    from lia_amd import ops
    req = ops.LogprobRequest(n_top)
    ctx.set_logprob_sink(req, shape)
    req.chosen.fill_(7.0)                                    # stale values would show
    if n_top:
        req.top_ids.fill_(-5)
        req.top_logprobs.fill_(7.0)
    torch.cuda.synchronize()
    return req


def _same_bits(torch, a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _assert_sink_is_the_bare_kernel(torch, ctx, req, logits2d, ids, n_top):
    chosen, top_ids, top_lp = ctx.topn_logprobs(logits2d, ids.reshape(-1).contiguous(), n_top)
    ctx.synchronize()
    assert _same_bits(torch, req.chosen.reshape(-1), chosen)
    assert torch.equal(req.top_ids.reshape(-1, n_top), top_ids)
    assert _same_bits(torch, req.top_logprobs.reshape(-1, n_top), top_lp)


@pytest.mark.parametrize("family,B", [("opt", 3), ("opt", 300), ("llama", 3)])
def test_lm_head_and_sample_write_the_sink(ctx, family, B):
    """with a sink the ids and logits are byte for byte the call's without one; sink row i is the bare kernel on logits row i with the
    id the head returned; B 300 goes through ops.Context.lm_head's 256-row chunks (row 256 writes sink row 256); lia_sample rewrites
    the rows with the sampled id as chosen"""
    import torch
    V, n_top = 512, 5
    inp = _head_inputs(torch, family, B, V, 90 + B)
    raw_logits, raw_ids = _lm_head(torch, ctx, family, inp)
    sup = int(raw_ids[0])
    for suppress in (-1, sup):
        req = _sink(torch, ctx, n_top, (B,))
        try:
            logits, ids = _lm_head(torch, ctx, family, inp, suppress)
            assert torch.equal(logits, raw_logits)
            if suppress < 0:
                assert (ids == raw_ids).all()
            else:
                assert ids[0] != sup
            ids_dev = torch.from_numpy(ids).cuda()
            _assert_sink_is_the_bare_kernel(torch, ctx, req, logits, ids_dev, n_top)
            # the model's own distribution: the suppressed argmax still leads the alternatives
            assert (req.top_ids[:, 0].cpu().numpy() == raw_ids).all()
            # the sampler behind it: the same sink rows, chosen follows the sampled ids
            u = torch.rand(B, generator=torch.Generator(device="cpu").manual_seed(B)).cuda()
            torch.cuda.synchronize()
            before = req.chosen.clone()
            sampled = ctx.sample(logits, 1.3, 0, 1.0, u, suppress_token=suppress)
            ctx.synchronize()
            assert (sampled.cpu().numpy() != ids).any()
            _assert_sink_is_the_bare_kernel(torch, ctx, req, logits, sampled, n_top)
            assert not torch.equal(before, req.chosen)
        finally:
            ctx.set_logprob_sink(None)
        plain = ctx.sample(logits, 1.3, 0, 1.0, u, suppress_token=suppress)      # without a sink: the same draw
        ctx.synchronize()
        assert torch.equal(plain, sampled)
    _, again = _lm_head(torch, ctx, family, inp)
    assert (again == raw_ids).all()


def _verify(torch, ctx, family, inp, block, view=None, suppress=-1, n_suppress=0, return_logits=False):
    hidden, nw, nb, head = inp
    blk = torch.from_numpy(np.ascontiguousarray(block)).cuda()
    torch.cuda.synchronize()
    if view is None:
        res = (ctx.lm_verify(hidden, nw, nb, head, blk, EPS, suppress, n_suppress) if family == "opt" else
               ctx.llama_lm_verify(hidden, nw, head, blk, EPS, suppress, n_suppress))
    else:
        kw = dict(suppress_token=suppress, n_suppress=n_suppress, return_logits=return_logits, return_p_draft=True)
        res = (ctx.lm_verify_sample(hidden, nw, nb, head, blk, view, EPS, **kw) if family == "opt" else
               ctx.llama_lm_verify_sample(hidden, nw, head, blk, view, EPS, **kw))
    ctx.synchronize()
    return res


@pytest.mark.parametrize("family,B,T", [("opt", 3, 4), ("opt", 70, 5), ("llama", 3, 4)])
def test_verify_heads_write_the_sink(family, B, T):
    """lia_lm_verify / lia_llama_lm_verify and the sampled verify heads; B 70 x T 5 = 350 rows in a workspace of 256-row chunks -- the
    second chunk starts inside block row 51 and writes sink rows 256 ...  The heads' outputs are byte for byte those without a sink;
    chosen is bit for bit lia_lm_score's log-probability over the same hidden rows with targets = greedy (both go through the same
    chunks, so the logits are the same bits); the sampled head's sink rows are the bare kernel on logits_out with the sampled ids"""
    import torch
    from lia_amd import ops, sampling
    V, n_top = 512, 5
    ctx = ops.Context(0, 512 + 256 * (2 * H + 2 * V) + 100)
    try:
        if B * T > 256:
            assert ctx.score_chunk_rows(B * T, H, V) == 256
        inp = _head_inputs(torch, family, B, V, 31 + B, T=T)
        hidden, nw, nb, head = inp
        zeros = np.zeros((B, T), np.int64)
        free = _verify(torch, ctx, family, inp, zeros)
        g = free.greedy.cpu().numpy()
        block = np.concatenate([zeros[:, :1], g[:, :T - 1]], axis=1)
        for b in range(B):
            a = (b + 1) % T
            if a < T - 1:
                block[b, a + 1] ^= 1
        sup, n_sup = int(g[0, 0]), 2
        raw = _verify(torch, ctx, family, inp, block, suppress=sup, n_suppress=n_sup)
        req = _sink(torch, ctx, n_top, (B, T))
        try:
            res = _verify(torch, ctx, family, inp, block, suppress=sup, n_suppress=n_sup)
        finally:
            ctx.set_logprob_sink(None)
        for name in ("greedy", "accepted", "common", "next"):
            assert torch.equal(getattr(res, name), getattr(raw, name)), name
        assert res.greedy[0, 0] != sup
        torch.cuda.synchronize()
        tg = res.greedy.reshape(-1).contiguous()
        lp, gr = (ctx.lm_score(hidden, nw, nb, head, tg, EPS) if family == "opt" else ctx.llama_lm_score(hidden, nw, head, tg, EPS))
        ctx.synchronize()
        assert _same_bits(torch, req.chosen.reshape(-1), lp)
        # the alternatives are the raw row's: its unsuppressed argmax first -- the suppressed token at (0, 0)
        assert torch.equal(req.top_ids.reshape(-1, n_top)[:, 0], gr) and int(req.top_ids[0, 0, 0]) == sup
        assert (req.top_logprobs[..., 0] >= req.chosen).all()
        # the sampled head, with the block's logits returned
        U = torch.rand((T + 3, B), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
        view = sampling.Sampler(0.9, 20, 0.95, U).block(1)
        sraw = _verify(torch, ctx, family, inp, block, view, suppress=sup, n_suppress=n_sup, return_logits=True)
        req = _sink(torch, ctx, n_top, (B, T))
        try:
            sres = _verify(torch, ctx, family, inp, block, view, suppress=sup, n_suppress=n_sup, return_logits=True)
        finally:
            ctx.set_logprob_sink(None)
        for name in ("greedy", "accepted", "common", "next", "logits", "p_draft"):
            assert torch.equal(getattr(sres, name), getattr(sraw, name)), name
        big = ops.Context(0, 8 << 20)
        try:
            _assert_sink_is_the_bare_kernel(torch, big, req, sres.logits.view(B * T, V), sres.greedy, n_top)
        finally:
            big.close()
    finally:
        ctx.close()


def test_refusals_by_name(ctx):
    """LIA_ERR_INVALID with the call's name, before anything is launched"""
    import torch
    from lia_amd import _native as N, ops
    V, B, T = 256, 3, 2
    hidden, nw, nb, head = _head_inputs(torch, "opt", B, V, 1)
    hid2 = torch.zeros((B, T, H), dtype=torch.bfloat16, device="cuda")
    blk = torch.zeros((B, T), dtype=torch.int64, device="cuda")
    lg = torch.zeros((B, V), dtype=torch.bfloat16, device="cuda")
    ids = torch.zeros(B, dtype=torch.int64, device="cuda")
    ch = torch.zeros(8, dtype=torch.float32, device="cuda")
    ti = torch.zeros((8, 40), dtype=torch.int64, device="cuda")
    tl = torch.zeros((8, 40), dtype=torch.float32, device="cuda")
    err = lambda: ctx.lib.lia_last_error().decode()                     # noqa: E731
    sink = lambda n, rows, c=ch, a=ti, b=tl: ctx.lib.lia_ctx_set_logprob_sink(ctx.handle, n, _p(c), _p(a), _p(b), rows)      # noqa: E731
    bare = lambda n, vocab=V, a=ti, b=tl: ctx.lib.lia_topn_logprobs(ctx.handle, _p(lg), V, B, vocab, _p(ids), n, _p(ch), _p(a), _p(b), None)  # noqa: E731
    torch.cuda.synchronize()
    try:
        assert sink(33, 8) == N.LIA_ERR_INVALID and "lia_ctx_set_logprob_sink: n_top=33 must be in [0, 32]" in err()
        assert sink(-1, 8) == N.LIA_ERR_INVALID and "n_top=-1" in err()
        assert sink(2, 8, a=None) == N.LIA_ERR_INVALID and "NULL top_ids" in err()
        assert sink(2, 8, b=None) == N.LIA_ERR_INVALID and "NULL top_logprobs" in err()
        assert sink(0, 8, a=None, b=None) == N.LIA_OK
        assert bare(33) == N.LIA_ERR_INVALID and "lia_topn_logprobs: n_top=33 must be in [0, 32]" in err()
        assert bare(9, vocab=8) == N.LIA_ERR_INVALID and "lia_topn_logprobs: n_top=9 alternatives, vocab=8 has fewer" in err()
        assert bare(2, a=None) == N.LIA_ERR_INVALID and "NULL top_ids" in err()
        # n_top > vocab is known at the head call
        assert sink(20, 8) == N.LIA_OK
        small = torch.zeros((B, 16), dtype=torch.bfloat16, device="cuda")
        with pytest.raises(ValueError, match="lia_sample: the log-probability sink asks for n_top=20 alternatives, vocab=16 has fewer"):
            ctx.sample(small, 1.0, 0, 1.0, torch.rand(B).cuda())
        # too few sink rows
        assert sink(2, 2) == N.LIA_OK
        with pytest.raises(ValueError, match="lia_lm_head: the call has 3 rows, the log-probability sink 2"):
            ctx.lm_head(hidden, nw, nb, head, EPS)
        with pytest.raises(ValueError, match="lia_sample: the call has 3 rows, the log-probability sink 2"):
            ctx.sample(lg, 1.0, 0, 1.0, torch.rand(B).cuda())
        assert sink(2, 4) == N.LIA_OK
        with pytest.raises(ValueError, match="lia_lm_verify: the call has 6 rows, the log-probability sink 4"):
            ctx.lm_verify(hid2, nw, nb, head, blk, EPS)
        with pytest.raises(ValueError, match="lia_llama_lm_verify: the call has 6 rows, the log-probability sink 4"):
            ctx.llama_lm_verify(hid2, nw, head, blk, EPS)
        # the heads that take no sink
        assert sink(2, 8) == N.LIA_OK
        tg = torch.zeros(B * T, dtype=torch.int64, device="cuda")
        with pytest.raises(ValueError, match="lia_lm_score: a log-probability sink is set"):
            ctx.lm_score(hid2, nw, nb, head, tg, EPS)
        with pytest.raises(ValueError, match="lia_llama_lm_score: a log-probability sink is set"):
            ctx.llama_lm_score(hid2, nw, head, tg, EPS)
        out = [torch.zeros((B, T), dtype=torch.int64, device="cuda"), torch.zeros((B, T), dtype=torch.int32, device="cuda"),
               torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
               torch.zeros(B, dtype=torch.int64, device="cuda")]

        def reject(llama):
            norm = [_p(nw)] if llama else [_p(nw), _p(nb)]
            fn = ctx.lib.lia_llama_lm_verify_reject if llama else ctx.lib.lia_lm_verify_reject
            return fn(ctx.handle, _p(hid2), H, B, T, H, *norm, _p(head), V, EPS, -1, 0, None, None, _p(blk), None, *[_p(t) for t in out],
                      None, None, None, None, None)

        for llama, name in ((False, "lia_lm_verify_reject"), (True, "lia_llama_lm_verify_reject")):
            assert reject(llama) == N.LIA_ERR_INVALID
            assert f"{name}: a log-probability sink is set" in err(), err()
        # chosen == NULL clears it: the score head runs again
        assert ctx.lib.lia_ctx_set_logprob_sink(ctx.handle, 0, None, None, None, 0) == N.LIA_OK
        ctx.lm_score(hid2, nw, nb, head, tg, EPS)
        ctx.synchronize()
        # the wrapper's own
        with pytest.raises(ValueError, match="n_top=40 must be in"):
            ctx.set_logprob_sink(ops.LogprobRequest(40), (B,))
        with pytest.raises(ValueError, match="expected an ops.LogprobRequest"):
            ctx.set_logprob_sink(5, (B,))
    finally:
        ctx.set_logprob_sink(None)
