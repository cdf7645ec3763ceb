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


def _llama_head_by_hand(torch, ctx, inp, mask, n_top, table, lds, bounds):
    """lia_llama_lm_head through the raw ABI, one call per (r0, n) of bounds, every modifier pointed at its row r0 by hand: mask
    (int32 [rows, W]; one row: broadcast), a sink of n_top alternatives, the count table (int16 [rows, ldc]) with a scratch of pitch lds.
    -> logits, ids, (chosen, top_ids, top_logprobs), scratch"""
    from lia_amd import _native as N
    hidden, nw, _, head = inp
    B, T, _ = hidden.shape
    lib, h = ctx.lib, ctx.handle
    at = lambda t, off: ctypes.c_void_p(t.data_ptr() + off)          # noqa: E731
    logits = torch.zeros((B, V), dtype=torch.bfloat16, device="cuda")
    nxt = torch.full((B,), -9, dtype=torch.int64, device="cuda")
    chosen = torch.zeros(B, dtype=torch.float32, device="cuda")
    top_ids = torch.full((B, n_top), -9, dtype=torch.int64, device="cuda")
    top = torch.zeros((B, n_top), dtype=torch.float32, device="cuda")
    scratch = torch.zeros((B, lds), dtype=torch.bfloat16, device="cuda")
    ldm = 0 if mask.shape[0] == 1 else mask.shape[1]
    ldc = table.shape[1]
    torch.cuda.synchronize()
    try:
        for r0, n in bounds:
            N.check(lib.lia_ctx_set_token_mask(h, at(mask, 4 * r0 * ldm), ldm, B - r0 if ldm else 1), "lia_ctx_set_token_mask")
            N.check(lib.lia_ctx_set_logprob_sink(h, n_top, at(chosen, 4 * r0), at(top_ids, 8 * r0 * n_top), at(top, 4 * r0 * n_top), B - r0),
                    "lia_ctx_set_logprob_sink")
            N.check(lib.lia_ctx_set_penalties(h, at(table, 2 * r0 * ldc), ldc, B - r0, *SETTINGS, at(scratch, 2 * r0 * lds), lds),
                    "lia_ctx_set_penalties")
            N.check(lib.lia_llama_lm_head(h, at(hidden, 2 * r0 * T * H), n, T, H, _p(nw), _p(head), V, EPS, -1, at(logits, 2 * r0 * V),
                                          at(nxt, 8 * r0), ctypes.c_void_p(ctx.stream)), "lia_llama_lm_head")
    finally:
        lib.lia_ctx_set_token_mask(h, None, 0, 0)
        lib.lia_ctx_set_logprob_sink(h, 0, None, None, None, 0)
        lib.lia_ctx_set_penalties(h, None, 0, 0, 1.0, 0.0, 0.0, None, 0)
    ctx.synchronize()
    return logits, nxt, (chosen, top_ids, top), scratch


@pytest.mark.parametrize("broadcast_mask", [False, True])
def test_llama_head_of_257_rows_offsets_every_modifier(ctx, broadcast_mask):
    """B = 257 through Context.llama_lm_head with a mask table, a sink (n_top = 3) and a count table all set: logits, ids, sink rows
    and scratch rows are bit for bit those of a 256-row call and a 1-row call made through the raw ABI with every table pointed at
    the call's first row by hand.  Row 256 differs from row 0 in its hidden row, its mask row and its count row, and its id is
    another under row 0's: a second chunk that read any table from row 0 would be caught.  Also with ONE broadcast mask row."""
    import torch
    from lia_amd import ops
    B, n_top = 257, 3
    inp = _head_inputs(torch, "llama", B, 29)
    hidden, nw, _, head = inp
    raw_logits, raw_ids = _lm_head(torch, ctx, "llama", inp)
    lg = _u16(raw_logits)
    table = _table(B, V, raw_ids, 15)
    rows = PR.penalty_ref(lg, table, *SETTINGS)
    allowed = np.random.RandomState(6).rand(B, V) < 0.5
    allowed[np.arange(B), PR.first_argmax(rows)] = False             # the penalised winner is forbidden: both must act
    allowed[:, 5] = True
    if broadcast_mask:
        allowed[:] = allowed[256]
    want = MR.first_argmax(PR.bf16_to_f32(rows), allowed)
    # row 256 under row 0's tables is another row: the hidden rows differ, and so does the id under row 0's mask / counts
    assert not torch.equal(hidden[256], hidden[0]) and (table[256] != table[0]).any()
    assert MR.first_argmax(PR.bf16_to_f32(PR.penalty_ref(lg[256:], table[:1], *SETTINGS)), allowed[256:])[0] != want[256]
    if not broadcast_mask:
        assert (allowed[256] != allowed[0]).any() and MR.first_argmax(PR.bf16_to_f32(rows[256:]), allowed[:1])[0] != want[256]
    mask = torch.from_numpy(MR.pack(allowed[256:] if broadcast_mask else allowed)).cuda()
    counts = _dev(torch, table)
    for lds in (V, V + 8):
        hand = _llama_head_by_hand(torch, ctx, inp, mask, n_top, counts, lds, ((0, 256), (256, 1)))
        req = ops.LogprobRequest(n_top)
        scratch = torch.zeros((B, lds), dtype=torch.bfloat16, device="cuda")
        torch.cuda.synchronize()
        ctx.set_token_mask(mask)
        ctx.set_logprob_sink(req, (B,))
        ctx.set_penalties(counts, *SETTINGS, scratch=scratch)
        try:
            logits, ids = ctx.llama_lm_head(hidden, nw, head, EPS)
            ctx.synchronize()
        finally:
            ctx.set_token_mask(None)
            ctx.set_logprob_sink(None)
            ctx.set_penalties(None)
        assert torch.equal(logits, hand[0]) and torch.equal(logits, raw_logits), lds
        assert torch.equal(ids, hand[1]) and (ids.cpu().numpy() == want).all(), lds
        for got, ref in zip((req.chosen, req.top_ids, req.top_logprobs), hand[2]):
            assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got,
                               ref.view(torch.int32) if ref.dtype == torch.float32 else ref), lds
        assert torch.equal(scratch.view(torch.int16), hand[3].view(torch.int16)) and (_u16(scratch)[:, :V] == rows).all(), lds


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


def test_the_first_fault_reported_keeps_its_place(ctx):
    """a call that is wrong in two ways reports what it always reported: a rejection head with penalties set AND a one-token block
    (T = 1) is refused for the penalties -- the modifiers a head does not take come before its own arguments"""
    import torch
    from lia_amd import _native as N
    B, T = 3, 1
    _, nw, nb, head = _head_inputs(torch, "opt", B, 23)
    hid = torch.zeros((B, T, H), dtype=torch.bfloat16, device="cuda")
    blk = torch.zeros((B, T), dtype=torch.int64, device="cuda")
    out = [torch.zeros((B, T), dtype=torch.int64, device="cuda"), torch.zeros((B, T), dtype=torch.int32, device="cuda"),
           torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
           torch.zeros(B, dtype=torch.int64, device="cuda")]
    torch.cuda.synchronize()
    ctx.set_penalties(torch.zeros((B * T, V), dtype=torch.int16, device="cuda"), 1.2)
    try:
        for name, norm in (("lia_lm_verify_reject", [_p(nw), _p(nb)]), ("lia_llama_lm_verify_reject", [_p(nw)])):
            rc = getattr(ctx.lib, name)(ctx.handle, _p(hid), H, B, T, H, *norm, _p(head), V, EPS, -1, 0, None, None, _p(blk), None,
                                        *[_p(t) for t in out], None, None, None, None, None)
            assert rc == N.LIA_ERR_INVALID
            assert ctx.lib.lia_last_error().decode() == (f"{name}: penalties are set (lia_ctx_set_penalties): every block position would need "
                                                         "its own counts -- penalties are not applied under speculation")
    finally:
        ctx.set_penalties(None)
