"""-m gpu: lia_lm_verify_sample / lia_llama_lm_verify_sample through the C ABI -- lia_sample's draw behind every position of a draft
block, against the NumPy restatement (spec_sample_ref.py) on the pass's OWN logits (logits_out), bit for bit against lia_sample on
those logits, and the acceptance against a host recomputation from the kernel's own ids."""
import ctypes

import numpy as np
import pytest

from sample_ref import draw_acceptable
from spec_sample_ref import accept, sample_block, spec_sample_ref

pytestmark = pytest.mark.gpu

H, EPS, TOL = 128, 1e-5, 1e-5
N_STEPS = 6
SETTINGS = [(1.0, 4, 1.0), (0.7, 0, 0.9), (1.3, 50, 0.9), (1.0, 0, 1.0)]
SHAPES = [(1, 2), (7, 5), (64, 8)]


def _inputs(torch, family, B, T, V, seed):
    """hidden [B, T, H], the final norm and an lm_head whose logits span about +-8 (sigma 2 over the vocabulary)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                      # noqa: E731
    hidden = (1.5 * r(B, T, H)).to(torch.bfloat16).cuda()
    nw = (1.0 + 0.1 * r(H)).to(torch.bfloat16).cuda()
    nb = (0.05 * r(H)).to(torch.bfloat16).cuda() if family == "opt" else None
    head = ((2.0 / H ** 0.5) * r(V, H)).to(torch.bfloat16).cuda()
    return hidden, nw, nb, head


def _block_view(torch, tau, k, p, U, step0=0, step_rows=None):
    from lia_amd import sampling
    s = sampling.Sampler(tau, k, p, U)
    return s.block(step0) if step_rows is None else s.block_rows(step_rows)


def _launch(torch, ctx, family, inp, block, view, suppress=-1, n_suppress=0, n_suppress_rows=None, active=None):
    hidden, nw, nb, head = inp
    blk = torch.from_numpy(np.ascontiguousarray(block)).cuda()
    nsr = None if n_suppress_rows is None else torch.from_numpy(np.asarray(n_suppress_rows, np.int32)).cuda()
    act = None if active is None else torch.from_numpy(np.asarray(active, np.int32)).cuda()
    torch.cuda.synchronize()
    kw = dict(suppress_token=suppress, n_suppress=n_suppress, n_suppress_rows=nsr, active=act, return_logits=True, return_p_draft=True)
    if family == "opt":
        res = ctx.lm_verify_sample(hidden, nw, nb, head, blk, view, EPS, **kw)
    else:
        res = ctx.llama_lm_verify_sample(hidden, nw, head, blk, view, EPS, **kw)
    ctx.synchronize()
    return res


def _scripted(draws, seed, V):
    """block_ids that accept (b + seed) % T tokens on row b: the draws up to there, then a token that is not the draw -- a random
    one, mostly outside the kept set, so that p_draft sees kept and unkept draft tokens"""
    B, T = draws.sampled.shape
    rs = np.random.RandomState(seed)
    blk = np.empty((B, T), np.int64)
    blk[:, 0] = rs.randint(0, V, B)
    blk[:, 1:] = draws.sampled[:, :T - 1]
    for b in range(B):
        a = (b + seed) % T
        if a < T - 1:
            wrong = int(rs.randint(0, V))
            blk[b, a + 1] = wrong if wrong != blk[b, a + 1] else wrong ^ 1
    return blk


def _check(torch, ctx, family, B, T, V, tau, k, p, variant, seed):
    inp = _inputs(torch, family, B, T, V, seed)
    gU = torch.Generator(device="cuda").manual_seed(seed + 1)
    U = torch.rand((N_STEPS, B + 3), device="cuda", generator=gU)           # ldu = B + 3 > B: the row is the column index
    rs = np.random.RandomState(seed + 2)
    if variant == 0:
        steps, view = N_STEPS - T // 2, _block_view(torch, tau, k, p, U, step0=N_STEPS - T // 2)
        n_sup, sup_kw, active = min(2, T), dict(n_suppress=min(2, T)), None
    else:
        steps = rs.randint(0, N_STEPS + 3, B)
        view = _block_view(torch, tau, k, p, U, step_rows=steps)
        n_sup = rs.randint(0, T + 1, B)
        sup_kw, active = dict(n_suppress_rows=n_sup), [int(b % 3 != 1) for b in range(B)]
    # a first pass for the logits: the suppressed token is row 0's maximum, the block is scripted from the reference's draws
    first = _launch(torch, ctx, family, inp, np.zeros((B, T), np.int64), view)
    lg = first.logits.float().cpu().numpy()
    suppress = int(np.argmax(lg[0, 0]))
    Uh = U.cpu().numpy()
    draws = sample_block(lg, tau, k, p, Uh, steps, suppress, n_sup)
    block = _scripted(draws, seed, V)
    res = _launch(torch, ctx, family, inp, block, view, suppress=suppress, active=active, **sup_kw)
    assert torch.equal(res.logits, first.logits)                            # the pass's logits do not depend on the block ids
    ref = spec_sample_ref(lg, block, tau, k, p, Uh, steps, suppress, n_sup, active, draws=draws)
    got = res.greedy.cpu().numpy()
    pd = res.p_draft.cpu().numpy().astype(np.float64)
    # (a) the ids against the reference, test_gpu_sampling's rule; (d) p_draft; (e) the table's edge
    skipped = 0
    step_of = np.broadcast_to(np.asarray(steps), (B,))[:, None] + np.arange(T)[None, :]
    past = 0
    for b in range(B):
        for t in range(T):
            if ref.margin[b, t] < TOL:
                skipped += 1
                continue
            print(f"row {b} pos {t}: id {got[b, t]} ref {ref.sampled[b, t]} p_draft {pd[b, t]:.6g} ref {ref.p_draft[b, t]:.6g} "
                  f"margin {ref.margin[b, t]:.3g}")
            assert got[b, t] == ref.sampled[b, t] or draw_acceptable(int(got[b, t]), ref.keep[b, t], ref.cum[b, t], float(ref.u[b, t]), TOL), \
                (b, t, got[b, t], ref.sampled[b, t])
            assert abs(pd[b, t] - ref.p_draft[b, t]) <= 2e-4, (b, t, pd[b, t], ref.p_draft[b, t])
            if t == T - 1 or not ref.keep[b, t, block[b, t + 1]]:
                assert pd[b, t] == 0.0
            if step_of[b, t] >= N_STEPS:
                past += 1
                assert ref.u[b, t] == 0 and got[b, t] == np.flatnonzero(ref.keep[b, t])[0]
    assert skipped * 8 <= B * T, (skipped, B * T)
    if B > 1:                                   # the cases reach past the table, and meet kept and unkept draft tokens
        assert past > 0 and (ref.p_draft > 0).any()
        if 0 < k < V or p < 1.0:                # (with neither top-k nor top-p every token is kept: only the suppressed one has weight 0)
            assert (ref.p_draft[:, :T - 1] == 0).any()
    assert (got[np.arange(T)[None, :] < np.broadcast_to(np.asarray(n_sup), (B,))[:, None]] != suppress).all()
    # (b) bit for bit lia_sample's ids on the same logits rows with the same u and suppress token: one device function
    flat = res.logits.view(B * T, V)
    u_flat = torch.from_numpy(ref.u.reshape(-1)).cuda()
    sup_on = (np.arange(T)[None, :] < np.broadcast_to(np.asarray(n_sup), (B,))[:, None]).reshape(-1)
    plain = np.zeros(B * T, np.int64)
    for on in (False, True):
        rows = np.flatnonzero(sup_on == on)
        if rows.size:
            idx = torch.from_numpy(rows).cuda()
            lg_rows, u_rows = flat[idx].contiguous(), u_flat[idx].contiguous()
            torch.cuda.synchronize()
            ids = ctx.sample(lg_rows, tau, k, p, u_rows, suppress_token=suppress if on else -1)
            ctx.synchronize()
            plain[rows] = ids.cpu().numpy()
    assert (plain.reshape(B, T) == got).all()
    # (c) accepted / common / next: the host recomputation from the kernel's own ids
    acc, common, nxt = accept(block, got, active)
    assert (res.accepted.cpu().numpy() == acc).all() and int(res.common.cpu()[0]) == common and (res.next.cpu().numpy() == nxt).all()
    if active is None:
        assert set(ref.accepted.tolist()) == {(b + seed) % T for b in range(B)}          # the script covers every count it can


CASES = [(V, B, T, si, variant) for V in (512, 50272) for B, T in SHAPES for si in range(len(SETTINGS)) for variant in (0, 1)]


@pytest.mark.parametrize("V,B,T,si,variant", CASES)
def test_ids_acceptance_and_p_draft(V, B, T, si, variant):
    """variant 0: step0 and a scalar n_suppress; 1: step_rows (steps 0 .. n_steps + 2), n_suppress per row, an active mask with zeros"""
    import torch
    from lia_amd import _native as N, ops
    ctx = ops.Context(0, N.lib().lia_lm_score_workspace_bytes(B * T, H, V))
    try:
        _check(torch, ctx, "opt", B, T, V, *SETTINGS[si], variant, seed=1000 * si + B + V)
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", [0, 1])
def test_llama_head_at_128256(variant):
    import torch
    from lia_amd import _native as N, ops
    B, T, V = 7, 5, 128256
    ctx = ops.Context(0, N.lib().lia_lm_score_workspace_bytes(B * T, H, V))
    try:
        _check(torch, ctx, "llama", B, T, V, *SETTINGS[2 - variant], variant, seed=77)
    finally:
        ctx.close()


@pytest.mark.parametrize("variant", [0, 1])
def test_a_chunk_boundary_inside_a_block_row(variant):
    """350 rows (70 x 5) in 256-row chunks: row 256 is block row 51 at position 1 -- block row, position, step and suppress bound are
    those of the block, not of the chunk"""
    import torch
    from lia_amd import ops
    B, T, V = 70, 5, 512
    ctx = ops.Context(0, 512 + 256 * (2 * H + 2 * V) + 100)
    try:
        assert ctx.score_chunk_rows(B * T, H, V) == 256
        _check(torch, ctx, "opt", B, T, V, *SETTINGS[variant], variant, seed=5)
    finally:
        ctx.close()


@pytest.mark.parametrize("V", [512, 50272])
def test_top_k_one_with_a_table_of_zeros_is_lm_verify(V):
    import torch
    from lia_amd import _native as N, ops
    B, T = 7, 5
    ctx = ops.Context(0, N.lib().lia_lm_score_workspace_bytes(B * T, H, V))
    try:
        inp = _inputs(torch, "opt", B, T, V, 3)
        hidden, nw, nb, head = inp
        view = _block_view(torch, 1.3, 1, 0.9, torch.zeros((N_STEPS, B), device="cuda"), step0=1)
        first = _launch(torch, ctx, "opt", inp, np.zeros((B, T), np.int64), view)
        suppress = int(first.greedy[0, 0])
        block = np.concatenate([np.zeros((B, 1), np.int64), first.greedy.cpu().numpy()[:, :T - 1]], axis=1)
        block[2, 3] ^= 1
        blk = torch.from_numpy(block).cuda()
        torch.cuda.synchronize()
        want = ctx.lm_verify(hidden, nw, nb, head, blk, EPS, suppress, 2)
        ctx.synchronize()
        res = _launch(torch, ctx, "opt", inp, block, view, suppress=suppress, n_suppress=2)
        assert torch.equal(res.greedy, want.greedy) and torch.equal(res.accepted, want.accepted)
        assert torch.equal(res.common, want.common) and torch.equal(res.next, want.next)
        assert (res.greedy[:, :2] != suppress).all() and int(res.accepted[2]) <= 2
    finally:
        ctx.close()


def test_argument_errors_by_name():
    import torch
    from lia_amd import _native as N, ops
    ctx = ops.Context(0, 1 << 20)
    try:
        hid = torch.zeros((6, 256), dtype=torch.bfloat16, device="cuda")
        w = torch.ones(256, dtype=torch.bfloat16, device="cuda")
        emb = torch.zeros((64, 256), dtype=torch.bfloat16, device="cuda")
        blk = torch.zeros((2, 3), dtype=torch.int64, device="cuda")
        smp = torch.zeros((2, 3), dtype=torch.int64, device="cuda")
        acc = torch.zeros(2, dtype=torch.int32, device="cuda")
        com = torch.zeros(1, dtype=torch.int32, device="cuda")
        nxt = torch.zeros(2, dtype=torch.int64, device="cuda")
        U = torch.zeros((4, 2), dtype=torch.float32, device="cuda")
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731

        def call(fn="lia_lm_verify_sample", hidden=hid, ldh=256, B=2, T=3, Hh=256, lnw=w, lnb=w, e=emb, vocab=64, sup=-1, n_sup=0, b=blk,
                 g=smp, a=acc, c=com, n=nxt, tau=1.0, k=0, pp=1.0, u=U, ldu=2, n_steps=4, step0=0, sampler=True):
            s = N.BlockSampler(tau, k, pp, None if u is None else u.data_ptr(), ldu, n_steps, step0, None)
            norm = (p(lnw), p(lnb)) if fn == "lia_lm_verify_sample" else (p(lnw),)
            return getattr(ctx.lib, fn)(ctx.handle, p(hidden), ldh, B, T, Hh, *norm, p(e), vocab, 1e-5, sup, n_sup, None,
                                        ctypes.byref(s) if sampler else None, p(b), None, p(g), p(a), p(c), p(n), None, None, None)

        assert call() == N.LIA_OK and call("lia_llama_lm_verify_sample") == N.LIA_OK
        ctx.synchronize()
        errors = ((dict(hidden=None), "NULL hidden"), (dict(lnw=None), "NULL norm weight"), (dict(e=None), "NULL lm_head weight"),
                  (dict(b=None), "NULL block_ids"), (dict(g=None), "NULL sampled"), (dict(a=None), "NULL accepted"),
                  (dict(c=None), "NULL common"), (dict(n=None), "NULL next"), (dict(u=None), "NULL uniforms"),
                  (dict(sampler=False), "NULL sampler"), (dict(B=0), "B=0"), (dict(T=1), "T=1"), (dict(n_sup=-1), "n_suppress=-1"),
                  (dict(n_sup=4), "n_suppress=4"), (dict(sup=64), "suppress_token=64"), (dict(sup=-2), "suppress_token=-2"),
                  (dict(Hh=200), "H=200"), (dict(vocab=40), "vocab=40"), (dict(ldh=128), "ldh=128"), (dict(ldh=260), "ldh=260"),
                  (dict(tau=0.0), "temperature=0"), (dict(tau=float("inf")), "temperature=inf"), (dict(tau=float("nan")), "temperature=nan"),
                  (dict(k=-1), "top_k=-1"), (dict(pp=0.0), "top_p=0"), (dict(pp=1.5), "top_p=1.5"), (dict(vocab=(1 << 21) + 16), "vocab=2097168"),
                  (dict(ldu=1), "ldu=1 < B=2"), (dict(n_steps=0), "n_steps=0"), (dict(step0=-1), "step0=-1"))
        for fn in ("lia_lm_verify_sample", "lia_llama_lm_verify_sample"):
            for kw, name in errors + (((dict(lnb=None), "NULL norm bias"),) if fn == "lia_lm_verify_sample" else ()):
                assert call(fn, **kw) == N.LIA_ERR_INVALID, (fn, name)
                err = ctx.lib.lia_last_error().decode()
                assert name in err and err.startswith(fn + ":"), (fn, name, err)
        big_emb = torch.zeros((50272, 256), dtype=torch.bfloat16, device="cuda")
        big_hid = torch.zeros((100, 3, 256), dtype=torch.bfloat16, device="cuda")
        big_blk = torch.zeros((100, 3), dtype=torch.int64, device="cuda")
        from lia_amd import sampling
        view = sampling.Sampler(1.0, 0, 1.0, torch.zeros((4, 100), device="cuda")).block(0)
        with pytest.raises(MemoryError, match="lia_lm_verify_sample: .* holds no chunk of 256 rows"):
            ctx.lm_verify_sample(big_hid, w, w, big_emb, big_blk, view)
    finally:
        ctx.close()
