"""-m gpu: lia_lm_verify_reject / lia_llama_lm_verify_reject through the C ABI -- the accept test and the residual draw of a stochastic
drafter's block -- against the float64 restatement (spec_reject_ref.py) on the pass's OWN logits (logits_out) and the drafter's
logits; the bonus token bit for bit against lia_sample; the acceptance against a host recomputation from the kernel's own ok /
token; and the distribution of the emitted token against P (chi-square) through the direct launcher."""
import ctypes

import numpy as np
import pytest

import spec_reject_ref as R
from sample_ref import draw_acceptable

pytestmark = pytest.mark.gpu

H, EPS, TOL = 128, 1e-5, 1e-5
N_STEPS = 6
SETTINGS = [(1.0, 0, 1.0), (0.9, 50, 1.0), (1.0, 0, 0.9), (0.8, 20, 0.95)]
SHAPES = [(3, 2), (5, 5), (2, 8)]
SIGMAS = (0.25, 1.0)


def _inputs(torch, family, B, T, V, seed):
    """hidden [B, T, H], the final norm and an lm_head whose logits span about +-8 (sigma 2 over the vocabulary)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                      # noqa: E731
    hidden = (1.5 * r(B, T, H)).to(torch.bfloat16).cuda()
    nw = (1.0 + 0.1 * r(H)).to(torch.bfloat16).cuda()
    nb = (0.05 * r(H)).to(torch.bfloat16).cuda() if family == "opt" else None
    head = ((2.0 / H ** 0.5) * r(V, H)).to(torch.bfloat16).cuda()
    return hidden, nw, nb, head


class _View:
    """what Context.lm_verify_reject reads of a sampling.RejectorBlock"""

    def __init__(self, settings, u_acc, u_res, step0, draft_logits):
        self.temperature, self.top_k, self.top_p = settings
        self.u_acc, self.u_res, self.step0, self.draft_logits = u_acc, u_res, step0, draft_logits


def _launch(torch, ctx, family, inp, block, view, suppress=-1, n_suppress=0, active=None):
    hidden, nw, nb, head = inp
    blk = torch.from_numpy(np.ascontiguousarray(block)).cuda()
    act = None if active is None else torch.from_numpy(np.asarray(active, np.int32)).cuda()
    torch.cuda.synchronize()
    kw = dict(suppress_token=suppress, n_suppress=n_suppress, active=act, return_logits=True, return_probs=True)
    if family == "opt":
        res = ctx.lm_verify_reject(hidden, nw, nb, head, blk, view, EPS, **kw)
    else:
        res = ctx.llama_lm_verify_reject(hidden, nw, head, blk, view, EPS, **kw)
    ctx.synchronize()
    return res


def _pass_logits(torch, ctx, family, inp, B, T):
    """the pass's logits [B, T, V] by the sampled verify head that exists already (the same chunks, the same GEMM)"""
    from lia_amd import sampling
    hidden, nw, nb, head = inp
    blk = torch.zeros((B, T), dtype=torch.int64, device="cuda")
    view = sampling.Sampler(1.0, 0, 1.0, torch.zeros((1, B), device="cuda")).block(0)
    torch.cuda.synchronize()
    if family == "opt":
        res = ctx.lm_verify_sample(hidden, nw, nb, head, blk, view, EPS, return_logits=True)
    else:
        res = ctx.llama_lm_verify_sample(hidden, nw, head, blk, view, EPS, return_logits=True)
    ctx.synchronize()
    return res.logits


def _draft(torch, ctx, logits, settings, sigma, U_draft, step0, suppress, n_sup, seed):
    """draft logits = the pass's logits + N(0, sigma^2) in bf16, and the draft tokens ctx.sample draws from them with U_draft[step0 + t]
    (0 past the table) and the verify head's suppress rule: the contract of the head"""
    B, T, V = logits.shape
    g = torch.Generator(device="cpu").manual_seed(seed + 7)
    noise = (sigma * torch.randn((B, T - 1, V), generator=g)).cuda()
    dl = (logits[:, :T - 1].float() + noise).to(torch.bfloat16).contiguous()
    ud, _ = R.table(U_draft.cpu().numpy(), step0, B, T - 1)
    drafts = np.zeros((B, T - 1), np.int64)
    for t in range(T - 1):
        rows, u = dl[:, t].contiguous(), torch.from_numpy(np.ascontiguousarray(ud[:, t])).cuda()
        torch.cuda.synchronize()
        ids = ctx.sample(rows, *settings, u, suppress_token=suppress if t < n_sup else -1)
        ctx.synchronize()
        drafts[:, t] = ids.cpu().numpy()
    return dl, drafts


def _prepare(torch, ctx, family, B, T, V, settings, sigma, seed):
    """the case's inputs and the reference on the pass's own logits -- nothing of the head under test"""
    tau, k, p = settings
    inp = _inputs(torch, family, B, T, V, seed)
    gU = torch.Generator(device="cuda").manual_seed(seed + 1)
    Ud, Ua, Ur = torch.rand((3, N_STEPS, B + 3), device="cuda", generator=gU)          # ldu = B + 3 > B: the row is the column index
    step0 = N_STEPS - (T + 1) // 2                                                      # the block's later positions lie past the table
    n_sup = min(2, T)
    logits = _pass_logits(torch, ctx, family, inp, B, T)
    lg = logits.float().cpu().numpy()
    suppress = int(np.argmax(lg[0, 0]))
    dl, drafts = _draft(torch, ctx, logits, settings, sigma, Ud, step0, suppress, n_sup, seed)
    block = np.concatenate([np.random.RandomState(seed).randint(0, V, (B, 1)), drafts], axis=1)
    view = _View(settings, Ua, Ur, step0, dl)
    ref = R.positions(lg, dl.float().cpu().numpy(), block, tau, k, p, Ua.cpu().numpy(), Ur.cpu().numpy(), step0, suppress, n_sup)
    return inp, logits, block, view, suppress, n_sup, ref


def reference_skips(ref):
    """the positions the checks below leave out: a kept-set margin below TOL, or (in front of the bonus position) R < 1e-3"""
    B, T = ref.margin.shape
    return int(sum(ref.margin[b, t] < TOL or (t < T - 1 and ref.resid[b, t] < 1e-3) for b in range(B) for t in range(T)))


def _check(torch, ctx, family, B, T, V, settings, sigma, seed, active=None):
    tau, k, p = settings
    inp, logits, block, view, suppress, n_sup, ref = _prepare(torch, ctx, family, B, T, V, settings, sigma, seed)
    assert reference_skips(ref) * 8 <= B * T, "the seed of this case was chosen so that the reference alone stays inside the cap"
    res = _launch(torch, ctx, family, inp, block, view, suppress=suppress, n_suppress=n_sup, active=active)
    assert torch.equal(res.logits, logits)
    tok, ok = res.greedy.cpu().numpy(), res.ok.cpu().numpy()
    pt, qt, rm = (x.cpu().numpy().astype(np.float64) for x in (res.p_tok, res.q_tok, res.resid_mass))
    skipped = compared_ok = past = 0
    for b in range(B):
        for t in range(T):
            print(f"row {b} pos {t}: token {tok[b, t]} ref {ref.token[b, t]} ok {ok[b, t]} ref {ref.ok[b, t]} p {pt[b, t]:.6g} ref {ref.p_tok[b, t]:.6g} "
                  f"q {qt[b, t]:.6g} ref {ref.q_tok[b, t]:.6g} R {rm[b, t]:.6g} ref {ref.resid[b, t]:.6g} margin {ref.margin[b, t]:.3g}")
            if t == T - 1:
                assert ok[b, t] == 0 and pt[b, t] == 0 and qt[b, t] == 0 and rm[b, t] == 0
            if ref.margin[b, t] < TOL:
                skipped += 1
                continue
            assert abs(pt[b, t] - ref.p_tok[b, t]) <= 2e-4 and abs(qt[b, t] - ref.q_tok[b, t]) <= 2e-4, (b, t)
            if not ref.inside[b, t]:
                past += 1
                assert ok[b, t] == 0, "a position past the table is rejected"
            elif t < T - 1:
                assert ref.q_tok[b, t] > 0, "the draft token was drawn from Q"
                if abs(float(ref.u_acc[b, t]) * ref.q_tok[b, t] - ref.p_tok[b, t]) >= TOL:
                    compared_ok += 1
                    assert ok[b, t] == ref.ok[b, t], (b, t)
            if t == T - 1:
                continue                                                  # (the bonus token: bit for bit below)
            if ref.resid[b, t] < 1e-3:
                skipped += 1
                continue
            assert abs(rm[b, t] - ref.resid[b, t]) <= 2e-4
            assert tok[b, t] == ref.token[b, t] or draw_acceptable(int(tok[b, t]), ref.r[b, t] > 0, ref.rcum[b, t], float(ref.u_res[b, t]),
                                                                     TOL / ref.resid[b, t]), (b, t, tok[b, t], ref.token[b, t])
    assert skipped * 8 <= B * T, (skipped, B * T)
    assert past > 0 and compared_ok > 0
    assert (tok[:, :n_sup] != suppress).all()
    # the bonus token: lia_sample's id of the same row and u, bit for bit
    u_last = torch.from_numpy(np.ascontiguousarray(ref.u_res[:, T - 1])).cuda()
    rows = res.logits[:, T - 1].contiguous()
    torch.cuda.synchronize()
    plain = ctx.sample(rows, tau, k, p, u_last, suppress_token=suppress if T - 1 < n_sup else -1)
    ctx.synchronize()
    assert (plain.cpu().numpy() == tok[:, T - 1]).all()
    # accepted / common / next: the host recomputation from the kernel's own ok and token
    acc, common, nxt = R.accept(block, tok, ok, active)
    assert (res.accepted.cpu().numpy() == acc).all() and int(res.common.cpu()[0]) == common and (res.next.cpu().numpy() == nxt).all()
    return acc, common


CASES = [(V, B, T, si) for V in (512, 50272) for B, T in SHAPES for si in range(len(SETTINGS))]
# Seeds: 1000 si + B + V, moved on by 100003 n where the REFERENCE alone, on the pass's logits of that seed, leaves out more than 1 / 8
# of the positions (a top-p boundary within 1e-5 of a tie group, frequent at vocab 50272) -- nothing of the head enters the choice.
SEED_STEPS = {(50272, 3, 2, 2): 1}


def case_seed(V, B, T, si):
    return 1000 * si + B + V + 100003 * SEED_STEPS.get((V, B, T, si), 0)


@pytest.mark.parametrize("V,B,T,si", CASES)
def test_accept_test_and_residual_draw(V, B, T, si):
    import torch
    from lia_amd import _native as N, ops
    ctx = ops.Context(0, N.lib().lia_lm_score_workspace_bytes(B * T, H, V))
    try:
        sigma = SIGMAS[(si + B) % 2]
        _check(torch, ctx, "opt", B, T, V, SETTINGS[si], sigma, seed=case_seed(V, B, T, si), active=[1, 0, 1, 1, 1][:B] if T == 5 else None)
    finally:
        ctx.close()


def test_llama_head_at_128256():
    import torch
    from lia_amd import _native as N, ops
    B, T, V = 3, 3, 128256
    ctx = ops.Context(0, N.lib().lia_lm_score_workspace_bytes(B * T, H, V))
    try:
        _check(torch, ctx, "llama", B, T, V, SETTINGS[3], 0.25, seed=77)
    finally:
        ctx.close()


def test_a_chunk_boundary_inside_a_block_row():
    """350 rows (70 x 5) in 256-row chunks: row 256 is block row 51 at position 1 -- block row, position, step, suppress bound and the
    drafter's row are those of the block, not of the chunk"""
    import torch
    from lia_amd import ops
    B, T, V = 70, 5, 512
    ctx = ops.Context(0, 512 + 256 * (2 * H + 2 * V) + 100)
    try:
        assert ctx.score_chunk_rows(B * T, H, V) == 256
        _check(torch, ctx, "opt", B, T, V, SETTINGS[1], 1.0, seed=5)
    finally:
        ctx.close()


def test_p_equals_q_is_accepted_and_draws_plainly():
    """the drafter's logits ARE the pass's: p = q for every token, every position inside the table is accepted, R = 0 and `token` is
    lia_sample's id with U_res"""
    import torch
    from lia_amd import _native as N, ops
    B, T, V, settings = 4, 3, 512, (0.9, 50, 0.95)
    ctx = ops.Context(0, N.lib().lia_lm_score_workspace_bytes(B * T, H, V))
    try:
        inp = _inputs(torch, "opt", B, T, V, 11)
        Ud, Ua, Ur = torch.rand((3, N_STEPS, B), device="cuda", generator=torch.Generator(device="cuda").manual_seed(12))
        logits = _pass_logits(torch, ctx, "opt", inp, B, T)
        dl, drafts = _draft(torch, ctx, logits, settings, 0.0, Ud, 0, -1, 0, 11)
        assert torch.equal(dl, logits[:, :T - 1])
        block = np.concatenate([np.zeros((B, 1), np.int64), drafts], axis=1)
        res = _launch(torch, ctx, "opt", inp, block, _View(settings, Ua, Ur, 0, dl))
        assert (res.ok.cpu().numpy()[:, :T - 1] == 1).all() and (res.resid_mass.cpu().numpy() == 0).all()
        assert torch.equal(res.p_tok, res.q_tok) and (res.p_tok[:, :T - 1] > 0).all()
        assert (res.accepted.cpu().numpy() == T - 1).all() and int(res.common[0]) == T - 1
        for t in range(T):
            rows, u = logits[:, t].contiguous(), Ur[t].contiguous()
            torch.cuda.synchronize()
            ids = ctx.sample(rows, *settings, u)
            ctx.synchronize()
            assert torch.equal(ids, res.greedy[:, t])
        assert torch.equal(res.next, res.greedy[:, T - 1])
    finally:
        ctx.close()


# ---- the distribution of the emitted token, through the direct launcher ----
DIST_V, DIST_ROWS, DIST_SETTINGS = 512, 4096, (1.0, 16, 1.0)


def dist_case(seed=2024):
    """(p_logits [V], q_logits [V], U_draft / U_acc / U_res [rows]) of the distribution test: bf16-representable fp32, host arrays"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    p = (2.0 * torch.randn(DIST_V, generator=g)).to(torch.bfloat16)
    q = (p.float() + 0.5 * torch.randn(DIST_V, generator=g)).to(torch.bfloat16)
    U = torch.rand((3, DIST_ROWS), generator=g)
    return p.float().numpy(), q.float().numpy(), U[0].numpy(), U[1].numpy(), U[2].numpy()


def dist_reference(case):
    """(emitted [rows], P [V]) of the NumPy reference on the case's uniforms"""
    p, q, ud, ua, ur = case
    fp, fq = R.filtered(p[None], *DIST_SETTINGS), R.filtered(q[None], *DIST_SETTINGS)
    n = ud.size
    drafts = R.plain_draw(R.Filtered(*(np.repeat(x, n, axis=0) for x in fq)), ud)
    block = np.stack([np.zeros(n, np.int64), drafts], axis=1)
    ref = R.positions(np.repeat(np.stack([p, p])[None], n, axis=0), np.repeat(q[None, None], n, axis=0), block, *DIST_SETTINGS, ua[None], ur[None], 0)
    return np.where(ref.ok[:, 0] == 1, drafts, ref.token[:, 0]), fp.prob[0], drafts, ref


def test_emitted_token_is_distributed_as_P():
    import torch
    from lia_amd import _native as N, ops
    case = dist_case()
    p, q, ud, ua, ur = case
    want, P, ref_drafts, ref = dist_reference(case)
    stat_ref, df_ref = R.chi_square(want, P)
    limit = R.chi2_quantile(df_ref, 1e-6)
    print(f"reference: chi-square {stat_ref:.2f} at {df_ref} degrees of freedom, limit {limit:.2f}; accepted {ref.ok[:, 0].mean():.3f}")
    assert stat_ref <= limit
    n, V = DIST_ROWS, DIST_V
    ctx = ops.Context(0, 1 << 20)
    try:
        lib = ctx.lib
        vp, ci, cl, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
        lib.lia_verify_reject_launch.restype = None
        lib.lia_verify_reject_launch.argtypes = [vp, cl, ci, ci, vp, cl, cl, cf, ci, cf, ci, ci, ci, ci, vp, vp, cl, ci, ci, vp, vp, vp, vp, vp, vp, vp]
        pl = torch.from_numpy(p).to(torch.bfloat16).cuda()
        logits = pl[None, None].expand(n, 2, V).contiguous()                                  # block row b: P behind both positions
        dl = torch.from_numpy(q).to(torch.bfloat16).cuda()[None, None].expand(n, 1, V).contiguous()
        Ud, Ua, Ur = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (ud, ua, ur))
        torch.cuda.synchronize()
        drafts = ctx.sample(dl.view(n, V), *DIST_SETTINGS, Ud)
        ctx.synchronize()
        assert (drafts.cpu().numpy() == ref_drafts).mean() > 0.99
        block = torch.stack([torch.zeros_like(drafts), drafts], dim=1).contiguous()
        token = torch.full((n, 2), -1, dtype=torch.int64, device="cuda")
        ok = torch.full((n, 2), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        # n_steps = 1, step0 = 0: position 0 reads U_acc[0, b] / U_res[0, b], the bonus position lies past the table
        lib.lia_verify_reject_launch(logits.data_ptr(), V, 2 * n, V, dl.data_ptr(), V, V, DIST_SETTINGS[0], DIST_SETTINGS[1], DIST_SETTINGS[2],
                                     -1, 0, 2, 0, Ua.data_ptr(), Ur.data_ptr(), n, 1, 0, block.data_ptr(), token.data_ptr(), ok.data_ptr(),
                                     None, None, None, None)
        torch.cuda.synchronize()
        okh, tokh = ok.cpu().numpy(), token.cpu().numpy()
        assert set(np.unique(okh[:, 0])) <= {0, 1} and (okh[:, 1] == 0).all()
        got = np.where(okh[:, 0] == 1, drafts.cpu().numpy(), tokh[:, 0])
        stat, df = R.chi_square(got, P)
        print(f"kernel: chi-square {stat:.2f} at {df} degrees of freedom; accepted {okh[:, 0].mean():.3f}; equal to the reference on "
              f"{(got == want).mean():.4f} of the rows")
        assert df == df_ref and stat <= limit
        assert (got == want).mean() > 0.99                       # the same function of the uniforms, up to near ties
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
        tok = torch.zeros((2, 3), dtype=torch.int64, device="cuda")
        okt = torch.zeros((2, 3), dtype=torch.int32, device="cuda")
        acc = torch.zeros(2, dtype=torch.int32, device="cuda")
        com = torch.zeros(1, dtype=torch.int32, device="cuda")
        nxt = torch.zeros(2, dtype=torch.int64, device="cuda")
        U = torch.zeros((4, 2), dtype=torch.float32, device="cuda")
        dlg = torch.zeros((2, 2, 72), dtype=torch.bfloat16, device="cuda")
        nsr = torch.zeros(2, dtype=torch.int32, device="cuda")
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731

        def call(fn="lia_lm_verify_reject", hidden=hid, ldh=256, B=2, T=3, Hh=256, lnw=w, lnb=w, e=emb, vocab=64, sup=-1, n_sup=0, b=blk,
                 g=tok, o=okt, a=acc, c=com, n=nxt, tau=1.0, k=0, pp=1.0, ua=U, ur=U, ldu=2, n_steps=4, step0=0, rej=True, dl=dlg, dl_off=0,
                 ldr=144, ldp=72, rows=None):
            s = N.BlockRejector(tau, k, pp, None if ua is None else ua.data_ptr(), None if ur is None else ur.data_ptr(), ldu, n_steps, step0,
                                None if dl is None else dl.data_ptr() + dl_off, ldr, ldp)
            norm = (p(lnw), p(lnb)) if fn == "lia_lm_verify_reject" else (p(lnw),)
            return getattr(ctx.lib, fn)(ctx.handle, p(hidden), ldh, B, T, Hh, *norm, p(e), vocab, 1e-5, sup, n_sup, p(rows),
                                        ctypes.byref(s) if rej else None, p(b), None, p(g), p(o), p(a), p(c), p(n), None, None, None, None, None)

        assert call() == N.LIA_OK and call("lia_llama_lm_verify_reject") == N.LIA_OK
        ctx.synchronize()
        errors = ((dict(hidden=None), "NULL hidden"), (dict(lnw=None), "NULL norm weight"), (dict(e=None), "NULL lm_head weight"),
                  (dict(b=None), "NULL block_ids"), (dict(g=None), "NULL token"), (dict(o=None), "NULL ok"), (dict(a=None), "NULL accepted"),
                  (dict(c=None), "NULL common"), (dict(n=None), "NULL next"), (dict(rej=False), "NULL rejector"),
                  (dict(dl=None), "NULL draft_logits"), (dict(ua=None), "NULL u_acc"), (dict(ur=None), "NULL u_res"),
                  (dict(ldp=56), "ldd_pos=56 < vocab=64"), (dict(ldr=56), "ldd_row=56 < vocab=64"), (dict(ldp=70), "ldd_pos=70"),
                  (dict(ldr=150), "ldd_row=150"), (dict(dl_off=2), "16-byte aligned"), (dict(rows=nsr), "n_suppress_rows must be NULL"),
                  (dict(B=0), "B=0"), (dict(T=1), "T=1"), (dict(n_sup=-1), "n_suppress=-1"), (dict(n_sup=4), "n_suppress=4"),
                  (dict(sup=64), "suppress_token=64"), (dict(sup=-2), "suppress_token=-2"), (dict(Hh=200), "H=200"),
                  (dict(ldh=128), "ldh=128"), (dict(tau=0.0), "temperature=0"), (dict(tau=float("nan")), "temperature=nan"),
                  (dict(k=-1), "top_k=-1"), (dict(pp=0.0), "top_p=0"), (dict(pp=1.5), "top_p=1.5"), (dict(vocab=(1 << 21) + 16), "vocab=2097168"),
                  (dict(ldu=1), "ldu=1 < B=2"), (dict(n_steps=0), "n_steps=0"), (dict(step0=-1), "step0=-1"))
        for fn in ("lia_lm_verify_reject", "lia_llama_lm_verify_reject"):
            for kw, name in errors + (((dict(lnb=None), "NULL norm bias"),) if fn == "lia_lm_verify_reject" else ()):
                assert call(fn, **kw) == N.LIA_ERR_INVALID, (fn, name)
                err = ctx.lib.lia_last_error().decode()
                assert name in err and err.startswith(fn + ":"), (fn, name, err)
        view = _View((1.0, 0, 1.0), U, U, 0, torch.zeros((2, 2, 60), dtype=torch.bfloat16, device="cuda"))
        with pytest.raises(ValueError, match="draft_logits has shape"):
            ctx.lm_verify_reject(hid.view(2, 3, 256), w, w, emb, blk, view)
    finally:
        ctx.close()
