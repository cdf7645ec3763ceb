"""-m gpu: the allowed-token masks of the head kernels (lia_ctx_set_token_mask, include/lia_hip.h) through the C ABI.

Every comparison is exact.  The defining identity: a masked head call gives bit for bit what the same call without a table gives on
logits whose disallowed entries were overwritten with bf16 -inf; the greedy heads are also held against mask_ref's first argmax over
the allowed entries of the logits the call itself returned."""
import ctypes

import numpy as np
import pytest

import mask_ref as MR
from spec_sample_ref import accept, block_uniforms

pytestmark = pytest.mark.gpu

H, EPS = 128, 1e-5
SAMPLE_SETTINGS = [(0.7, k, p) for k in (0, 5, 50) for p in (1.0, 0.9)]
VOCABS = [250, 256, 257, 50272, 128256]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev_mask(torch, allowed):
    return torch.from_numpy(MR.pack(allowed)).cuda()


def _logits(torch, rows, vocab, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (2.0 * torch.randn(rows, vocab, generator=g)).to(torch.bfloat16).cuda()


def mask_kinds(lg_f32, seed):
    """name -> allowed bool [vocab] for one row of logits: the cases of the issue.  `suppress` (returned too) is a token the
    "random half" mask allows and that is the row's maximum among them: the mask and suppress_token must compose."""
    vocab = lg_f32.shape[0]
    rs = np.random.RandomState(seed)
    kinds = {"all ones": np.ones(vocab, bool)}
    for i in (0, 31, 32, vocab - 1):
        one = np.zeros(vocab, bool)
        one[i] = True
        kinds[f"only {i}"] = one
    no_win = np.ones(vocab, bool)
    no_win[int(np.argmax(lg_f32))] = False
    kinds["winner forbidden"] = no_win
    half = rs.rand(vocab) < 0.5
    half[int(np.argsort(-lg_f32)[3])] = True
    kinds["random half"] = half
    three = np.zeros(vocab, bool)
    three[rs.choice(vocab, 3, replace=False)] = True
    kinds["three allowed"] = three                       # fewer allowed tokens than top-k 5 / 50
    return kinds


def _batch(torch, vocab, base_rows, seed):
    """logits [R, vocab] (every base row once per mask kind), allowed [R, vocab], per-row kind names"""
    base = _logits(torch, base_rows, vocab, seed)
    bf = base.float().cpu().numpy()
    rows, allowed, names = [], [], []
    for r in range(base_rows):
        for name, a in mask_kinds(bf[r], seed + r).items():
            rows.append(r)
            allowed.append(a)
            names.append(name)
    lg = base[torch.tensor(rows).cuda()].contiguous()
    return lg, np.stack(allowed), names


@pytest.fixture(scope="module")
def lib():
    from lia_amd import _native as N
    return MR.bind(N.lib())


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    from lia_amd import ops
    c = ops.Context(0, 64 << 20)
    yield c
    c.close()


def _argmax(torch, lib, ctx, lg, suppress=-1, mask=None, ldm=0):
    out = torch.empty(lg.shape[0], dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    st = ctypes.c_void_p(ctx.stream)
    if mask is None:
        lib.lia_argmax_launch(_p(lg), _p(out), lg.shape[0], lg.shape[1], suppress, st)
    else:
        lib.lia_argmax_masked_launch(_p(lg), _p(out), lg.shape[0], lg.shape[1], suppress, _p(mask), ldm, st)
    ctx.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("vocab", VOCABS)
def test_argmax_kernel_vector_and_scalar_paths(lib, ctx, vocab):
    """lia_argmax_kernel<1> at vocab 250 / 257 (the scalar path, a last word of 26 / 1 live bits), 256, 50272 (1571 words), 128256:
    every mask kind on 3 rows in one launch and on 1 row, the broadcast row, the mask with a suppress_token it does not cover"""
    import torch
    lg, allowed, names = _batch(torch, vocab, 3, 40 + vocab)
    W = MR.words(vocab)
    mask = _dev_mask(torch, allowed)
    assert tuple(mask.shape) == (lg.shape[0], W)
    lf = lg.float().cpu().numpy()
    got = _argmax(torch, lib, ctx, lg, mask=mask, ldm=W)
    assert (got == MR.first_argmax(lf, allowed)).all(), [(n, g) for n, g in zip(names, got)]
    assert (got == _argmax(torch, lib, ctx, MR.substitute(torch, lg, allowed))).all()
    assert allowed[np.arange(len(got)), got].all()
    plain = _argmax(torch, lib, ctx, lg)
    ones = np.flatnonzero(np.array(names) == "all ones")
    assert (got[ones] == plain[ones]).all()
    assert (got[np.array(names) == "winner forbidden"] != plain[np.array(names) == "winner forbidden"]).all()
    # tail bits at and beyond vocab are ignored: the same rows with every tail bit set
    if vocab & 31:
        dirty = mask.clone()
        dirty[:, -1] |= int(np.array([0xFFFFFFFF << (vocab & 31) & 0xFFFFFFFF], np.uint32).view(np.int32)[0])
        assert (_argmax(torch, lib, ctx, lg, mask=dirty, ldm=W) == got).all()
    # a padded pitch (ldm > W), one row, and the broadcast row (ldm = 0) over all rows
    wide = torch.zeros((lg.shape[0], W + 3), dtype=torch.int32, device="cuda")
    wide[:, :W] = mask
    assert (_argmax(torch, lib, ctx, lg, mask=wide, ldm=W + 3) == got).all()
    half = names.index("random half")
    assert (_argmax(torch, lib, ctx, lg[half:half + 1].contiguous(), mask=mask[half:half + 1].contiguous(), ldm=W) == got[half:half + 1]).all()
    bro = np.broadcast_to(allowed[half], allowed.shape)
    got_b = _argmax(torch, lib, ctx, lg, mask=mask[half:half + 1].contiguous(), ldm=0)
    assert (got_b == MR.first_argmax(lf, bro)).all() and (got_b != got).any()
    # the mask together with a suppress_token it allows: the row's best allowed token
    sup = int(got[half])
    got_s = _argmax(torch, lib, ctx, lg, suppress=sup, mask=mask, ldm=W)
    assert (got_s == MR.first_argmax(lf, allowed, sup)).all() and got_s[half] != sup
    sub = MR.substitute(torch, lg, allowed)
    assert (got_s == _argmax(torch, lib, ctx, sub, suppress=sup)).all()


@pytest.mark.parametrize("vocab", VOCABS)
def test_sample_equals_the_unmasked_draw_on_substituted_logits(ctx, vocab):
    """lia_sample with a table == lia_sample without one on logits with -inf at the disallowed entries: ids and all four stats, bit
    for bit, tau 0.7 x top-k 0 / 5 / 50 x top-p 1 / 0.9 -- rows with one and three allowed tokens (fewer than top-k), the broadcast
    row, one row, and a suppress_token the mask allows"""
    import torch
    lg, allowed, names = _batch(torch, vocab, 3, 90 + vocab)
    R = lg.shape[0]
    mask = _dev_mask(torch, allowed)
    sub = MR.substitute(torch, lg, allowed)
    half = names.index("random half")
    u = torch.rand(R, generator=torch.Generator(device="cpu").manual_seed(vocab)).cuda()
    sup = int(MR.first_argmax(lg.float().cpu().numpy(), allowed)[half])

    def draw(logits, table, tau, k, p, suppress=-1, uu=u):
        stats = torch.full((logits.shape[0], 4), -7.0, device="cuda")
        ctx.set_token_mask(table)
        try:
            torch.cuda.synchronize()
            ids = ctx.sample(logits, tau, k, p, uu, suppress_token=suppress, stats=stats)
            ctx.synchronize()
        finally:
            ctx.set_token_mask(None)
        return ids.cpu().numpy(), stats.cpu().numpy()

    for tau, k, p in SAMPLE_SETTINGS:
        ids, st = draw(lg, mask, tau, k, p)
        want_ids, want_st = draw(sub, None, tau, k, p)
        assert (ids == want_ids).all() and (st.view(np.int32) == want_st.view(np.int32)).all(), (vocab, k, p)
        assert allowed[np.arange(R), ids].all()
        for i, n in enumerate(names):
            if n.startswith("only "):
                assert ids[i] == int(n[5:]) and st[i, 2] == 1.0
            if n == "three allowed":
                assert st[i, 2] <= 3.0
        # all ones == the call without a table on the raw logits
        ones = np.flatnonzero(np.array(names) == "all ones")
        raw_ids, raw_st = draw(lg, None, tau, k, p)
        assert (ids[ones] == raw_ids[ones]).all() and (st[ones].view(np.int32) == raw_st[ones].view(np.int32)).all()
        # the mask and a suppress_token it allows
        ids_s, st_s = draw(lg, mask, tau, k, p, suppress=sup)
        want_ids, want_st = draw(sub, None, tau, k, p, suppress=sup)
        assert (ids_s == want_ids).all() and (st_s.view(np.int32) == want_st.view(np.int32)).all()
        assert ids_s[half] != sup
        # the broadcast row and a one-row call
        bro = np.broadcast_to(allowed[half], allowed.shape)
        ids_b, st_b = draw(lg, mask[half:half + 1].contiguous(), tau, k, p)
        want_ids, want_st = draw(MR.substitute(torch, lg, bro), None, tau, k, p)
        assert (ids_b == want_ids).all() and (st_b.view(np.int32) == want_st.view(np.int32)).all()
        one_ids, one_st = draw(lg[half:half + 1].contiguous(), mask[half:half + 1].contiguous(), tau, k, p, uu=u[half:half + 1].contiguous())
        assert one_ids[0] == ids[half] and (one_st.view(np.int32) == st[half:half + 1].view(np.int32)).all()


def _head_inputs(torch, family, rows, V, seed, T=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                      # noqa: E731
    hidden = (1.5 * r(rows, T, H)).to(torch.bfloat16).cuda()
    nw = (1.0 + 0.1 * r(H)).to(torch.bfloat16).cuda()
    nb = (0.05 * r(H)).to(torch.bfloat16).cuda() if family == "opt" else None
    head = ((2.0 / H ** 0.5) * r(V, H)).to(torch.bfloat16).cuda()
    return hidden, nw, nb, head


def _lm_head(torch, ctx, family, inp, suppress=-1):
    hidden, nw, nb, head = inp
    B, T, _ = hidden.shape
    V = head.shape[0]
    torch.cuda.synchronize()
    if family == "opt":
        logits, nxt = ctx.lm_head(hidden, nw, nb, head, EPS, suppress)
    else:
        from lia_amd import _native as N
        logits = torch.empty((B, V), dtype=torch.bfloat16, device="cuda")
        nxt = torch.empty((B,), dtype=torch.int64, device="cuda")
        N.check(ctx.lib.lia_llama_lm_head(ctx.handle, _p(hidden), B, T, H, _p(nw), _p(head), V, EPS, suppress, _p(logits), _p(nxt),
                                          ctypes.c_void_p(ctx.stream)), "lia_llama_lm_head")
    ctx.synchronize()
    return logits, nxt.cpu().numpy()


@pytest.mark.parametrize("family", ["opt", "llama"])
@pytest.mark.parametrize("V", [256, 50272, 128256])
def test_lm_head_ids_and_untouched_logits(ctx, family, V):
    """lia_lm_head / lia_llama_lm_head: the logits buffer is the unmasked call's in every case; the id is mask_ref's first argmax over
    the allowed entries of those logits; an all-ones table is the unmasked call"""
    import torch
    for B in (1, 3):
        inp = _head_inputs(torch, family, B, V, 7 * V + B)
        raw_logits, raw_ids = _lm_head(torch, ctx, family, inp)
        lf = raw_logits.float().cpu().numpy()
        per_row = [mask_kinds(lf[b], 5 + b) for b in range(B)]
        sup = int(raw_ids[0])
        for name in per_row[0]:
            allowed = np.stack([per_row[b][name] for b in range(B)])
            for table, eff, suppress in ((_dev_mask(torch, allowed), allowed, -1),
                                         (_dev_mask(torch, allowed[:1]), np.broadcast_to(allowed[0], allowed.shape), -1),
                                         (_dev_mask(torch, allowed), allowed, sup)):
                if suppress >= 0 and not (eff & (np.arange(V)[None, :] != suppress)).any(axis=1).all():
                    continue                                   # (the mask allows only the suppressed token: the host's to refuse)
                ctx.set_token_mask(table)
                try:
                    logits, ids = _lm_head(torch, ctx, family, inp, suppress)
                finally:
                    ctx.set_token_mask(None)
                assert torch.equal(logits, raw_logits), (family, V, name)
                assert (ids == MR.first_argmax(lf, eff, suppress)).all(), (family, V, B, name, ids)
                if name == "all ones" and suppress < 0:
                    assert (ids == raw_ids).all()
        _, again = _lm_head(torch, ctx, family, inp)            # the table is gone: today's ids
        assert (again == raw_ids).all()


def test_257_rows_through_ops_lm_head_repoint_the_table_per_chunk(ctx):
    """ops.Context.lm_head serves 257 rows as 256 + 1: row 256 reads table row 256, and the table is pointed back at row 0 afterwards"""
    import torch
    B, V = 257, 256
    inp = _head_inputs(torch, "opt", B, V, 3)
    raw_logits, raw_ids = _lm_head(torch, ctx, "opt", inp)
    lf = raw_logits.float().cpu().numpy()
    allowed = np.random.RandomState(8).rand(B, V) < 0.5
    allowed[np.arange(B), raw_ids] = False                      # every row's unmasked winner is forbidden
    allowed[256] = False
    allowed[256, [5, 200]] = True
    ctx.set_token_mask(_dev_mask(torch, allowed))
    try:
        logits, ids = _lm_head(torch, ctx, "opt", inp)
        assert torch.equal(logits, raw_logits) and (ids == MR.first_argmax(lf, allowed)).all() and ids[256] in (5, 200)
        first3 = tuple(t[:3].contiguous() if t.dim() == 3 else t for t in inp)
        _, ids3 = _lm_head(torch, ctx, "opt", first3)           # rows 0 .. 2 of the table again
        assert (ids3 == ids[:3]).all()
        # one broadcast row over 257 rows: no re-pointing, every chunk reads it
        ctx.set_token_mask(_dev_mask(torch, allowed[256:257]))
        _, ids_b = _lm_head(torch, ctx, "opt", inp)
        assert set(ids_b.tolist()) <= {5, 200}
        ctx.set_token_mask(_dev_mask(torch, allowed[:100]))
        with pytest.raises(ValueError, match="257 rows, the token mask table 100"):
            ctx.lm_head(*inp, EPS)
    finally:
        ctx.set_token_mask(None)


def test_257_rows_through_the_raw_call(ctx):
    """lia_lm_head itself serves 257 rows (chunks of 256 inside the library): with a per-row table, what ops.Context.lm_head returns;
    with a 100-row table LIA_ERR_INVALID by name, the whole batch checked before anything is launched -- the ids keep their sentinel"""
    import torch
    from lia_amd import _native as N
    B, V = 257, 256
    inp = _head_inputs(torch, "opt", B, V, 3)
    hidden, nw, nb, head = inp
    _, raw_ids = _lm_head(torch, ctx, "opt", inp)
    allowed = np.random.RandomState(8).rand(B, V) < 0.5
    allowed[np.arange(B), raw_ids] = False                      # every row's unmasked winner is forbidden
    allowed[256] = False
    allowed[256, [5, 200]] = True

    def raw():
        logits = torch.full((B, V), 7.0, dtype=torch.bfloat16, device="cuda")
        nxt = torch.full((B,), -9, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        rc = ctx.lib.lia_lm_head(ctx.handle, _p(hidden), B, 1, H, _p(nw), _p(nb), _p(head), V, EPS, -1, _p(logits), _p(nxt),
                                 ctypes.c_void_p(ctx.stream))
        ctx.synchronize()
        return rc, logits, nxt.cpu().numpy()

    ctx.set_token_mask(_dev_mask(torch, allowed))
    try:
        want_logits, want_ids = _lm_head(torch, ctx, "opt", inp)
        rc, logits, ids = raw()
        assert rc == N.LIA_OK and torch.equal(logits, want_logits) and (ids == want_ids).all() and ids[256] in (5, 200)
        ctx.set_token_mask(_dev_mask(torch, allowed[:100]))
        rc, _, ids = raw()
        assert rc == N.LIA_ERR_INVALID
        assert "lia_lm_head: the call has 257 rows, the token mask table 100 (lia_ctx_set_token_mask)" in ctx.lib.lia_last_error().decode()
        assert (ids == -9).all()
    finally:
        ctx.set_token_mask(None)


def _verify_setup(torch, family, B, T, V, seed):
    inp = _head_inputs(torch, family, B, V, seed, T=T)
    allowed = np.random.RandomState(seed + 1).rand(B, T, V) < 0.5           # a different mask per (row, position)
    U = torch.rand((T + 3, B), device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed + 2))
    return inp, allowed, U


def _verify(torch, ctx, family, inp, block, table, view=None, suppress=-1, n_suppress=0, active=None, return_logits=False):
    hidden, nw, nb, head = inp
    blk = torch.from_numpy(np.ascontiguousarray(block)).cuda()
    act = None if active is None else torch.from_numpy(np.asarray(active, np.int32)).cuda()
    ctx.set_token_mask(table)
    try:
        torch.cuda.synchronize()
        if view is None:
            res = (ctx.lm_verify(hidden, nw, nb, head, blk, EPS, suppress, n_suppress, act) if family == "opt" else
                   ctx.llama_lm_verify(hidden, nw, head, blk, EPS, suppress, n_suppress, act))
        else:
            kw = dict(suppress_token=suppress, n_suppress=n_suppress, active=act, return_logits=return_logits, return_p_draft=True)
            res = (ctx.lm_verify_sample(hidden, nw, nb, head, blk, view, EPS, **kw) if family == "opt" else
                   ctx.llama_lm_verify_sample(hidden, nw, head, blk, view, EPS, **kw))
        ctx.synchronize()
    finally:
        ctx.set_token_mask(None)
    return res


@pytest.mark.parametrize("family", ["opt", "llama"])
def test_verify_heads_across_a_chunk_boundary(lib, family):
    """B 70 x T 5 = 350 rows in a workspace of 256-row chunks, a different mask per (row, position): chunk row 0 of the second chunk
    is block row 256 and reads table row 256.  greedy / accepted / common / next of lia_lm_verify and the sampled ids of
    lia_lm_verify_sample equal the unmasked kernels on the -inf-substituted logits of the same hidden; the greedy ids equal mask_ref
    on the logits lia_lm_verify_sample(return_logits=True) returns"""
    import torch
    from lia_amd import ops, sampling
    B, T, V = 70, 5, 512
    ctx = ops.Context(0, 512 + 256 * (2 * H + 2 * V) + 100)
    try:
        assert ctx.score_chunk_rows(B * T, H, V) == 256
        inp, allowed, U = _verify_setup(torch, family, B, T, V, 21)
        table = _dev_mask(torch, allowed)
        assert tuple(table.shape) == (B, T, MR.words(V))
        tau, k, p = 0.7, 5, 0.9
        view = sampling.Sampler(tau, k, p, U).block(2)
        zeros = np.zeros((B, T), np.int64)
        raw = _verify(torch, ctx, family, inp, zeros, None, view, return_logits=True)
        first = _verify(torch, ctx, family, inp, zeros, table, view, return_logits=True)
        assert torch.equal(first.logits, raw.logits)                        # the returned logits stay the raw ones
        lf = raw.logits.float().cpu().numpy().reshape(B * T, V)
        flat_allowed = allowed.reshape(B * T, V)
        n_sup = 2
        sup = int(MR.first_argmax(lf[:1], flat_allowed[:1])[0])             # row 0 position 0's masked winner: suppressed at t < 2
        sup_rows = np.where(np.tile(np.arange(T), B) < n_sup, sup, -1)
        want_greedy = MR.first_argmax(lf, flat_allowed, sup_rows).reshape(B, T)
        assert want_greedy[0, 0] != sup and flat_allowed[np.arange(B * T), want_greedy.reshape(-1)].all()
        assert (want_greedy != MR.first_argmax(lf, np.ones_like(flat_allowed)).reshape(B, T)).any()
        # a block scripted to accept (b + 1) % T tokens on row b
        block = np.concatenate([zeros[:, :1], want_greedy[:, :T - 1]], axis=1)
        for b in range(B):
            a = (b + 1) % T
            if a < T - 1:
                block[b, a + 1] ^= 1
        active = [int(b % 7 != 3) for b in range(B)]
        res = _verify(torch, ctx, family, inp, block, table, suppress=sup, n_suppress=n_sup, active=active)
        got = res.greedy.cpu().numpy()
        assert (got == want_greedy).all(), np.argwhere(got != want_greedy)[:5]
        acc, common, nxt = accept(block, got, active)
        assert (res.accepted.cpu().numpy() == acc).all() and int(res.common.cpu()[0]) == common and (res.next.cpu().numpy() == nxt).all()
        assert set(acc.tolist()) == set(range(T))
        # the unmasked kernels on the substituted logits: one launch over all 350 rows, then the acceptance kernel
        sub = MR.substitute(torch, raw.logits.view(B * T, V), flat_allowed)
        g2 = torch.empty((B, T), dtype=torch.int64, device="cuda")
        a2 = torch.empty(B, dtype=torch.int32, device="cuda")
        c2 = torch.empty(1, dtype=torch.int32, device="cuda")
        n2 = torch.empty(B, dtype=torch.int64, device="cuda")
        blk = torch.from_numpy(block).cuda()
        act = torch.from_numpy(np.asarray(active, np.int32)).cuda()
        torch.cuda.synchronize()
        st = ctypes.c_void_p(ctx.stream)
        lib.lia_verify_argmax_rows_launch(_p(sub), V, B * T, V, sup, n_sup, None, T, 0, _p(g2), st)
        lib.lia_verify_accept_launch(_p(blk), _p(g2), _p(act), B, T, _p(a2), _p(c2), _p(n2), st)
        ctx.synchronize()
        assert torch.equal(res.greedy, g2) and torch.equal(res.accepted, a2) and torch.equal(res.common, c2) and torch.equal(res.next, n2)
        # the masked launcher in one launch (no chunking) agrees with the chunked head
        g3 = torch.empty((B, T), dtype=torch.int64, device="cuda")
        lib.lia_verify_argmax_masked_launch(_p(raw.logits), V, B * T, V, sup, n_sup, None, T, 0, _p(g3), _p(table), MR.words(V), st)
        ctx.synchronize()
        assert torch.equal(g3, g2)
        # sampled verification: lia_sample without a table on the substituted rows, with the position's uniform and suppress switch
        u = torch.from_numpy(block_uniforms(U.cpu().numpy(), 2, B, T).reshape(-1)).cuda()
        plain = np.zeros(B * T, np.int64)
        for on in (False, True):
            rows = np.flatnonzero((sup_rows >= 0) == on)
            idx = torch.from_numpy(rows).cuda()
            lg_rows, u_rows = sub[idx].contiguous(), u[idx].contiguous()
            torch.cuda.synchronize()
            ids = ctx.sample(lg_rows, tau, k, p, u_rows, suppress_token=sup if on else -1)
            ctx.synchronize()
            plain[rows] = ids.cpu().numpy()
        sblock = np.concatenate([zeros[:, :1], plain.reshape(B, T)[:, :T - 1]], axis=1)
        for b in range(B):
            a = (b + 2) % T
            if a < T - 1:
                sblock[b, a + 1] ^= 1
        sres = _verify(torch, ctx, family, inp, sblock, table, view, suppress=sup, n_suppress=n_sup, active=active)
        sgot = sres.greedy.cpu().numpy()
        assert (sgot.reshape(-1) == plain).all(), np.flatnonzero(sgot.reshape(-1) != plain)[:5]
        assert flat_allowed[np.arange(B * T), sgot.reshape(-1)].all()
        acc, common, nxt = accept(sblock, sgot, active)
        assert (sres.accepted.cpu().numpy() == acc).all() and int(sres.common.cpu()[0]) == common and (sres.next.cpu().numpy() == nxt).all()
        # p_draft is the kept weight of the draft token under the MASKED distribution: 0 for a draft token the mask forbids
        pd = sres.p_draft.cpu().numpy()
        forbidden = ~np.take_along_axis(allowed[:, :T - 1], sblock[:, 1:, None], axis=2)[..., 0]
        assert forbidden.any() and (pd[:, :T - 1][forbidden] == 0).all()
        # an all-ones table and the broadcast row
        ones = _verify(torch, ctx, family, inp, sblock, _dev_mask(torch, np.ones((B, T, V), bool)), view, suppress=sup, n_suppress=n_sup)
        none = _verify(torch, ctx, family, inp, sblock, None, view, suppress=sup, n_suppress=n_sup)
        assert torch.equal(ones.greedy, none.greedy) and torch.equal(ones.p_draft, none.p_draft) and torch.equal(ones.next, none.next)
        bro = _verify(torch, ctx, family, inp, block, _dev_mask(torch, allowed[0, :1]), suppress=sup, n_suppress=n_sup)
        want_b = MR.first_argmax(lf, np.broadcast_to(allowed[0, 0], flat_allowed.shape), sup_rows).reshape(B, T)
        assert (bro.greedy.cpu().numpy() == want_b).all()
    finally:
        ctx.close()


@pytest.mark.parametrize("vocab", [250, 257, 256])
def test_verify_kernels_on_the_scalar_load_path(lib, ctx, vocab):
    """lia_verify_argmax_kernel<1> and lia_verify_sample_kernel<1> through their launchers at vocab 250 and 257 (rows that are not
    16-byte aligned: vec = 0, a last mask byte of 2 and 1 live bits) and 256: B 3 x T 4 rows launched as two chunks (r0 = 0 and 5, so the
    second chunk starts inside block row 1), equal to the unmasked launchers on the -inf-substituted logits and to mask_ref"""
    import torch
    B, T = 3, 4
    n, W = B * T, MR.words(vocab)
    lg = _logits(torch, n, vocab, 300 + vocab)
    lf = lg.float().cpu().numpy()
    rs = np.random.RandomState(vocab)
    allowed = rs.rand(n, vocab) < 0.5
    allowed[:, vocab - 1] = True                                         # the last live bit of the tail byte is in play
    allowed[3] = False
    allowed[3, [0, vocab - 1]] = True
    mask = _dev_mask(torch, allowed)
    sub = MR.substitute(torch, lg, allowed)
    sup, n_sup = int(MR.first_argmax(lf[:1], allowed[:1])[0]), 2
    sup_rows = np.where(np.tile(np.arange(T), B) < n_sup, sup, -1)
    U = torch.rand((T + 2, B), generator=torch.Generator(device="cpu").manual_seed(vocab)).cuda()
    blk = torch.from_numpy(rs.randint(0, vocab, (B, T)).astype(np.int64)).cuda()
    st = ctypes.c_void_p(ctx.stream)
    torch.cuda.synchronize()

    def run(masked):
        src = lg if masked else sub
        greedy = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        sampled = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        pd = torch.full((n,), -1.0, device="cuda")
        for r0, cnt in ((0, 5), (5, n - 5)):
            rows = src[r0:r0 + cnt]
            tail = (_p(mask), W) if masked else ()
            getattr(lib, "lia_verify_argmax_masked_launch" if masked else "lia_verify_argmax_rows_launch")(
                _p(rows), vocab, cnt, vocab, sup, n_sup, None, T, r0, _p(greedy), *tail, st)
            getattr(lib, "lia_verify_sample_masked_launch" if masked else "lia_verify_sample_launch")(
                _p(rows), vocab, cnt, vocab, 0.7, 5, 0.9, sup, n_sup, None, T, r0, _p(U), U.stride(0), U.shape[0], 1, None, _p(blk), _p(sampled),
                _p(pd), *tail, st)
        ctx.synchronize()
        return greedy.cpu().numpy(), sampled.cpu().numpy(), pd.cpu().numpy()

    g1, s1, p1 = run(True)
    g0, s0, p0 = run(False)
    assert (g1 == g0).all() and (s1 == s0).all() and (p1.view(np.int32) == p0.view(np.int32)).all()
    assert (g1 == MR.first_argmax(lf, allowed, sup_rows)).all()
    assert allowed[np.arange(n), s1].all() and allowed[np.arange(n), g1].all() and g1[0] != sup
    assert g1[3] in (0, vocab - 1) and s1[3] in (0, vocab - 1)


def test_refusals_by_name(ctx):
    """LIA_ERR_INVALID with the call's name: an ldm that is neither 0 nor >= ceil(vocab / 32), more rows than the table, the
    rejection heads while a table is set, bad arguments of lia_ctx_set_token_mask itself"""
    import torch
    from lia_amd import _native as N
    V, B, T = 256, 3, 2
    W = MR.words(V)
    inp = _head_inputs(torch, "opt", B, V, 1)
    hidden, nw, nb, head = inp
    lg = _logits(torch, B, V, 2)
    u = torch.rand(B).cuda()
    table = torch.full((4, W), -1, dtype=torch.int32, device="cuda")
    blk = torch.zeros((B, T), dtype=torch.int64, device="cuda")
    hid2 = torch.zeros((B, T, H), dtype=torch.bfloat16, device="cuda")
    err = lambda: ctx.lib.lia_last_error().decode()                     # noqa: E731
    set_raw = lambda ldm, rows, t=table: ctx.lib.lia_ctx_set_token_mask(ctx.handle, _p(t), ldm, rows)      # noqa: E731
    torch.cuda.synchronize()
    try:
        assert set_raw(-1, 4) == N.LIA_ERR_INVALID and "ldm=-1" in err()
        assert set_raw(W, -2) == N.LIA_ERR_INVALID and "rows=-2" in err()
        assert ctx.lib.lia_ctx_set_token_mask(ctx.handle, ctypes.c_void_p(table.data_ptr() + 2), W, 4) == N.LIA_ERR_INVALID and "aligned" in err()
        # ldm too small for the call's vocabulary
        assert set_raw(W - 1, 4) == N.LIA_OK
        with pytest.raises(ValueError, match=rf"lia_sample: the token mask has ldm={W - 1} words per row, vocab=256 needs ceil\(vocab / 32\) = {W}"):
            ctx.sample(lg, 1.0, 0, 1.0, u)
        with pytest.raises(ValueError, match=f"lia_lm_head: the token mask has ldm={W - 1}"):
            ctx.lm_head(hidden, nw, nb, head, EPS)
        with pytest.raises(ValueError, match=f"lia_lm_verify: the token mask has ldm={W - 1}"):
            ctx.lm_verify(hid2, nw, nb, head, blk, EPS)
        # more rows than the table
        assert set_raw(W, 2) == N.LIA_OK
        with pytest.raises(ValueError, match="lia_sample: the call has 3 rows, the token mask table 2"):
            ctx.sample(lg, 1.0, 0, 1.0, u)
        with pytest.raises(ValueError, match="lia_lm_head: the call has 3 rows, the token mask table 2"):
            ctx.lm_head(hidden, nw, nb, head, EPS)
        assert set_raw(W, 4) == N.LIA_OK
        with pytest.raises(ValueError, match="lia_lm_verify: the call has 6 rows, the token mask table 4"):
            ctx.lm_verify(hid2, nw, nb, head, blk, EPS)
        from lia_amd import sampling
        view = sampling.Sampler(1.0, 0, 1.0, torch.rand((4, B), device="cuda")).block(0)
        with pytest.raises(ValueError, match="lia_lm_verify_sample: the call has 6 rows, the token mask table 4"):
            ctx.lm_verify_sample(hid2, nw, nb, head, blk, view, EPS)
        with pytest.raises(ValueError, match="lia_llama_lm_verify: the call has 6 rows, the token mask table 4"):
            ctx.llama_lm_verify(hid2, nw, head, blk, EPS)
        # one row with ldm = 0 serves any call
        assert set_raw(0, 1) == N.LIA_OK
        ctx.sample(lg, 1.0, 0, 1.0, u)
        ctx.lm_verify(hid2, nw, nb, head, blk, EPS)
        ctx.synchronize()
        # the rejection heads refuse a table before anything else they would refuse
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
            assert f"{name}: a token mask is set" in err(), err()
        ctx.set_token_mask(None)
        for llama, name in ((False, "lia_lm_verify_reject"), (True, "lia_llama_lm_verify_reject")):
            assert reject(llama) == N.LIA_ERR_INVALID
            assert f"{name}: NULL rejector" in err(), err()
        # the wrapper's own refusals
        for bad, what in ((torch.zeros((3, W), dtype=torch.int64, device="cuda"), "int32"), (torch.zeros((3, W), dtype=torch.int32), "CUDA"),
                          (table[:, :4], "contiguous"), ([1, 2], "list")):
            with pytest.raises(ValueError, match="token mask: expected a contiguous int32 CUDA tensor"):
                ctx.set_token_mask(bad)
    finally:
        ctx.set_token_mask(None)
