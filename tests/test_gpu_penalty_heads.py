"""-m gpu: the head calls while penalties are set (lia_ctx_set_penalties, include/lia_hip.h) on a tiny H = 64, vocab = 1008 head.

Every comparison is exact.  The defining identity: a penalised head call gives bit for bit what the same call without penalties
gives on logits rewritten with penalty_ref's values; the logits a head returns stay the raw ones, and a log-probability sink still
describes the raw logits."""
import ctypes

import numpy as np
import pytest

import mask_ref as MR
import penalty_ref as PR

pytestmark = pytest.mark.gpu

H, V, EPS = 64, 1008, 1e-5
SETTINGS = (1.7, 0.6, 0.3)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    from lia_amd import ops
    c = ops.Context(0, 32 << 20)
    yield c
    c.close()


def _head_inputs(torch, family, rows, seed, T=1):
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


def _u16(t):
    import torch
    return (t if t.dtype == torch.int16 else t.view(torch.int16)).cpu().numpy().view(np.uint16)


def _table(rows, ldc, winners, seed):
    """count words of every kind over the row, the raw winner and its runners-up among the penalised tokens"""
    rs = np.random.RandomState(seed)
    pool = np.array([0, 0, 0, 0x8000, 1, 0x8001, 3, 0x7fff, 0xffff], dtype=np.uint16)
    t = rs.choice(pool, size=(rows, ldc)).astype(np.uint16)
    t[np.arange(rows), winners] = rs.choice(np.array([0x8000, 2, 0x8003], dtype=np.uint16), size=rows)
    return t


def _dev(torch, u16):
    return torch.from_numpy(np.ascontiguousarray(u16).view(np.int16)).cuda()


@pytest.mark.parametrize("family", ["opt", "llama"])
def test_lm_head_with_a_table(ctx, family):
    """B = 8: the logits are the call's without a table, byte for byte; the id is the first argmax of penalty_ref(those logits, table)
    -- with the table's pitch and the scratch's equal to vocab (the 16-byte path) and not (ldc = 1010: the scalar path; lds = 1016),
    and together with suppress_token; after clearing, the call is the plain one"""
    import torch
    B = 8
    inp = _head_inputs(torch, family, B, 11)
    raw_logits, raw_ids = _lm_head(torch, ctx, family, inp)
    lg = _u16(raw_logits)
    for ldc, lds in ((V, V), (V + 2, V + 8)):
        table = _table(B, ldc, raw_ids, 5 + ldc)
        want_rows = PR.penalty_ref(lg, table, *SETTINGS)
        want = PR.first_argmax(want_rows)
        assert (want != raw_ids).any()                       # (the table does change the winner of some row)
        scratch = torch.zeros((B, lds), dtype=torch.bfloat16, device="cuda")
        ctx.set_penalties(_dev(torch, table), *SETTINGS, scratch=scratch)
        try:
            logits, ids = _lm_head(torch, ctx, family, inp)
            assert torch.equal(logits, raw_logits)
            assert (ids == want).all(), (ids, want)
            assert (_u16(scratch)[:, :V] == want_rows).all()             # scratch row i holds the penalised row i
            sup = int(want[0])
            logits, ids = _lm_head(torch, ctx, family, inp, suppress=sup)
            assert torch.equal(logits, raw_logits)
            assert (ids == PR.first_argmax(want_rows, sup)).all() and ids[0] != sup
        finally:
            ctx.set_penalties(None)
        logits, ids = _lm_head(torch, ctx, family, inp)
        assert torch.equal(logits, raw_logits) and (ids == raw_ids).all()


def test_lm_head_chunks_beyond_256_rows(ctx):
    """B = 300 through Context.lm_head: the second chunk reads table rows 256 .. 299 and writes scratch rows 256 .. 299 -- rows whose
    words differ from those of rows 0 .. 43"""
    import torch
    B = 300
    inp = _head_inputs(torch, "opt", B, 13)
    raw_logits, raw_ids = _lm_head(torch, ctx, "opt", inp)
    lg = _u16(raw_logits)
    table = _table(B, V, raw_ids, 9)
    assert (table[256:] != table[:44]).any()
    want_rows = PR.penalty_ref(lg, table, *SETTINGS)
    want = PR.first_argmax(want_rows)
    wrong = PR.first_argmax(PR.penalty_ref(lg[256:], table[:44], *SETTINGS))
    assert (wrong != want[256:]).any()                       # (a chunk that read the table from row 0 would be caught)
    ctx.set_penalties(_dev(torch, table), *SETTINGS)
    try:
        logits, ids = _lm_head(torch, ctx, "opt", inp)
        assert torch.equal(logits, raw_logits) and (ids == want).all()
        assert (_u16(ctx._penalties[1])[:, :V] == want_rows).all()
        logits, ids = _lm_head(torch, ctx, "opt", (inp[0][:256].contiguous(),) + inp[1:])     # pointed back at row 0
        assert (ids == want[:256]).all()
        with pytest.raises(ValueError, match="the call has 301 rows, the count table 300"):
            ctx.lm_head(torch.zeros((301, 1, H), dtype=torch.bfloat16, device="cuda"), *inp[1:], EPS)
    finally:
        ctx.set_penalties(None)


def _draw(torch, ctx, logits, u, tau, k, p, suppress=-1):
    stats = torch.full((logits.shape[0], 4), -7.0, device="cuda")
    torch.cuda.synchronize()
    ids = ctx.sample(logits, tau, k, p, u, suppress_token=suppress, stats=stats)
    ctx.synchronize()
    return ids.cpu().numpy(), stats.cpu().numpy().view(np.int32)


@pytest.mark.parametrize("tau,k,p", [(0.7, 4, 0.9), (1.0, 0, 1.0)])
def test_sample_equals_the_plain_draw_on_rewritten_logits(ctx, tau, k, p):
    import torch
    B = 8
    g = torch.Generator(device="cpu").manual_seed(3)
    logits = (2.0 * torch.randn(B, V, generator=g)).to(torch.bfloat16).cuda()
    u = torch.rand(B, generator=g).cuda()
    lg = _u16(logits)
    table = _table(B, V, PR.first_argmax(lg), 21)
    rewritten = _dev(torch, PR.penalty_ref(lg, table, *SETTINGS)).view(torch.bfloat16)
    want_ids, want_st = _draw(torch, ctx, rewritten, u, tau, k, p)
    plain_ids, plain_st = _draw(torch, ctx, logits, u, tau, k, p)
    ctx.set_penalties(_dev(torch, table), *SETTINGS)
    try:
        ids, st = _draw(torch, ctx, logits, u, tau, k, p)
        assert (ids == want_ids).all() and (st == want_st).all()
        assert (_u16(logits) == lg).all()                                  # the caller's logits are not rewritten
        sup = int(want_ids[0])
        ids_s, st_s = _draw(torch, ctx, logits, u, tau, k, p, suppress=sup)
    finally:
        ctx.set_penalties(None)
    want_s = _draw(torch, ctx, rewritten, u, tau, k, p, suppress=sup)
    assert (ids_s == want_s[0]).all() and (st_s == want_s[1]).all() and ids_s[0] != sup
    assert (st != plain_st).any()                                          # (the penalties did move the distribution)
    again = _draw(torch, ctx, logits, u, tau, k, p)                        # after clearing: the plain call
    assert (again[0] == plain_ids).all() and (again[1] == plain_st).all()


def test_composition_with_a_token_mask(ctx):
    """mask and penalties together: the ids are the masked call's on the rewritten logits -- lm_head (OPT and Llama) against the
    first allowed argmax of the rewritten rows, sample against the masked draw on them; with the scratch rows vocab apart (lm_head's
    own masked argmax) and at another pitch (lds = 1016: the pitched masked launch, what a vocabulary that is no multiple of 8 takes)"""
    import torch
    B = 8
    rs = np.random.RandomState(2)
    for family in ("opt", "llama"):
        inp = _head_inputs(torch, family, B, 17)
        raw_logits, raw_ids = _lm_head(torch, ctx, family, inp)
        lg = _u16(raw_logits)
        table = _table(B, V, raw_ids, 31)
        rows = PR.penalty_ref(lg, table, *SETTINGS)
        allowed = rs.rand(B, V) < 0.5
        allowed[np.arange(B), PR.first_argmax(rows)] = False           # the penalised winner is forbidden: both must act
        allowed[:, 5] = True
        mask = torch.from_numpy(MR.pack(allowed)).cuda()
        want = MR.first_argmax(PR.bf16_to_f32(rows), allowed)
        assert (want != PR.first_argmax(rows)).all()
        u = torch.rand(B, generator=torch.Generator(device="cpu").manual_seed(4)).cuda()
        ctx.set_token_mask(mask)
        try:
            masked = _draw(torch, ctx, _dev(torch, rows).view(torch.bfloat16), u, 0.7, 4, 0.9)
            for lds in (V, V + 8):
                scratch = torch.zeros((B, lds), dtype=torch.bfloat16, device="cuda")
                ctx.set_penalties(_dev(torch, table), *SETTINGS, scratch=scratch)
                try:
                    logits, ids = _lm_head(torch, ctx, family, inp)
                    assert torch.equal(logits, raw_logits) and (ids == want).all(), lds
                    sup = int(want[0])
                    _, ids = _lm_head(torch, ctx, family, inp, suppress=sup)
                    assert (ids == MR.first_argmax(PR.bf16_to_f32(rows), allowed, sup)).all(), lds
                    got = _draw(torch, ctx, raw_logits, u, 0.7, 4, 0.9)
                finally:
                    ctx.set_penalties(None)
                assert (got[0] == masked[0]).all() and (got[1] == masked[1]).all(), lds
                assert allowed[np.arange(B), got[0]].all()
        finally:
            ctx.set_token_mask(None)


def test_composition_with_a_logprob_sink(ctx):
    """sink and penalties together: top_ids / top_logprobs are those of the call without penalties (the model's own distribution),
    chosen is the raw log-probability of the penalised id -- behind lm_head and behind sample"""
    import torch
    from lia_amd import ops
    B, n_top = 8, 3
    inp = _head_inputs(torch, "opt", B, 19)
    hidden, nw, nb, head = inp

    def head_call(sample):
        req = ops.LogprobRequest(n_top)
        ctx.set_logprob_sink(req, (B,))
        try:
            logits, ids = _lm_head(torch, ctx, "opt", inp)
            if sample:
                u = torch.rand(B, generator=torch.Generator(device="cpu").manual_seed(8)).cuda()
                ids = _draw(torch, ctx, logits, u, 0.7, 4, 0.9)[0]
        finally:
            ctx.set_logprob_sink(None)
        return logits, ids, req.chosen.cpu().numpy(), req.top_ids.cpu().numpy(), req.top_logprobs.cpu().numpy()

    for sample in (False, True):
        raw_logits, raw_ids, raw_chosen, raw_top_ids, raw_top = head_call(sample)
        table = _table(B, V, PR.first_argmax(_u16(raw_logits)), 41)
        ctx.set_penalties(_dev(torch, table), *SETTINGS)
        try:
            logits, ids, chosen, top_ids, top = head_call(sample)
        finally:
            ctx.set_penalties(None)
        assert torch.equal(logits, raw_logits)
        if not sample:
            assert (ids != raw_ids).any() and (chosen != raw_chosen).any()
        assert (top_ids == raw_top_ids).all() and (top.view(np.int32) == raw_top.view(np.int32)).all()
        own = ctx.topn_logprobs(raw_logits, torch.from_numpy(ids).cuda(), 0)[0]
        ctx.synchronize()
        assert (chosen.view(np.int32) == own.cpu().numpy().view(np.int32)).all()


def test_block_and_score_heads_refuse_by_name(ctx):
    import torch
    from lia_amd import _native as N
    from lia_amd import sampling
    B, T = 3, 2
    _, nw, nb, head = _head_inputs(torch, "opt", B, 23)
    hid2 = torch.zeros((B, T, H), dtype=torch.bfloat16, device="cuda")
    blk = torch.zeros((B, T), dtype=torch.int64, device="cuda")
    view = sampling.Sampler(1.0, 0, 1.0, torch.rand((4, B), device="cuda")).block(0)
    err = lambda: ctx.lib.lia_last_error().decode()                     # noqa: E731
    out = [torch.zeros((B, T), dtype=torch.int64, device="cuda"), torch.zeros((B, T), dtype=torch.int32, device="cuda"),
           torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
           torch.zeros(B, dtype=torch.int64, device="cuda")]

    def reject(llama):
        norm = [_p(nw)] if llama else [_p(nw), _p(nb)]
        fn = ctx.lib.lia_llama_lm_verify_reject if llama else ctx.lib.lia_lm_verify_reject
        return fn(ctx.handle, _p(hid2), H, B, T, H, *norm, _p(head), V, EPS, -1, 0, None, None, _p(blk), None, *[_p(t) for t in out],
                  None, None, None, None, None)

    calls = {
        "lia_lm_verify": lambda: ctx.lm_verify(hid2, nw, nb, head, blk, EPS),
        "lia_lm_verify_rows": lambda: ctx.lm_verify_rows(hid2, nw, nb, head, blk, torch.zeros(B, dtype=torch.int32, device="cuda"), EPS),
        "lia_llama_lm_verify": lambda: ctx.llama_lm_verify(hid2, nw, head, blk, EPS),
        "lia_lm_verify_sample": lambda: ctx.lm_verify_sample(hid2, nw, nb, head, blk, view, EPS),
        "lia_llama_lm_verify_sample": lambda: ctx.llama_lm_verify_sample(hid2, nw, head, blk, view, EPS),
        "lia_lm_score": lambda: ctx.lm_score(hid2, nw, nb, head, blk, EPS),
        "lia_llama_lm_score": lambda: ctx.llama_lm_score(hid2, nw, head, blk, EPS),
    }
    torch.cuda.synchronize()
    ctx.set_penalties(torch.zeros((B * T, V), dtype=torch.int16, device="cuda"), 1.2)
    try:
        for name, call in calls.items():
            with pytest.raises(ValueError, match=rf"{name}: penalties are set \(lia_ctx_set_penalties\)"):
                call()
        for llama, name in ((False, "lia_lm_verify_reject"), (True, "lia_llama_lm_verify_reject")):
            assert reject(llama) == N.LIA_ERR_INVALID
            assert f"{name}: penalties are set" in err(), err()
    finally:
        ctx.set_penalties(None)
    for call in calls.values():                                         # after clearing they run
        call()
    ctx.synchronize()
    for llama, name in ((False, "lia_lm_verify_reject"), (True, "lia_llama_lm_verify_reject")):
        assert reject(llama) == N.LIA_ERR_INVALID and f"{name}: NULL rejector" in err()
