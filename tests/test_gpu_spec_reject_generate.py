"""-m gpu: speculative sampled decoding with the rejection rule -- generate(do_sample=True, sampled_verify=True,
verify_rule="rejection", draft=ModelDrafter(other weights, stochastic=True)) -- on test_gpu_multiturn's tiny OPT (head dim 128, and a
4-head variant at 64) and a small Llama.

Every verify pass is RECORDED with its own logits and the drafter's logits and pinned against the float64 reference
(spec_reject_ref.positions) on exactly those: p_tok / q_tok, the accept decisions away from their boundary, the residual draws, the
acceptance as a host recomputation from the kernel's own ok / token, the drafter's tokens as draws of its own logits with U_draft,
and the output as exactly what the rounds kept.  No acceptance rate is asserted; the rates are printed."""
import numpy as np
import pytest

import spec_reject_ref as R
import synth
from sample_ref import draw_acceptable
from test_gpu_generate import cxl_nodes_of_this_box  # noqa: F401  (autouse fixture)
from test_gpu_multiturn import B, C, SEED, T0, W_STD, _close, _ids, _opt, choose_rows

pytestmark = pytest.mark.gpu

NEW, TOL = 10, 1e-5
SAMPLE = dict(do_sample=True, temperature=0.9, top_k=20, top_p=0.95)
POLICIES = [("3-3 100", dict(prefill_policy=3, decoding_policy=3, gpu_percentage=100)),
            ("0-2 25 pinned", dict(prefill_policy=0, decoding_policy=2, gpu_percentage=25, pin_weight=True)),
            ("1-1 0", dict(prefill_policy=1, decoding_policy=1, gpu_percentage=0))]


class Recorder:
    """wraps a scheduler's forward / verify: the rejection route is forced to return its logits, every pass is kept"""

    def __init__(self, sched):
        self.first, self.rounds = [], []
        fwd, ver = sched.forward, sched.verify

        def forward(ids, kv, **kw):
            logits, nxt = fwd(ids, kv, **kw)
            self.first.append((nxt.cpu().numpy(), kw["sampler"].u.cpu().numpy()))
            return logits, nxt

        def verify(block, kv, **kw):
            assert kw.get("rejector") is not None and kw.get("sampler") is None and "return_logits" not in kw
            res, common = ver(block, kv, **kw, return_logits=True)
            self.rounds.append((block.clone().numpy(), kw, res, common, kw["rejector"].draft_logits.float().cpu().numpy()))
            return res, common

        sched.forward, sched.verify = forward, verify


def tables(new, rows, seed):
    from lia_amd import sampling
    U = sampling.draw_uniforms(new, rows, seed).cpu().numpy()
    return (U,) + tuple(sampling.draw_reject_tables(new, rows, seed).cpu().numpy())


def check_rounds(rec, out, log, passes, tabs, t0, new=NEW, eos=None, pad=1, settings=SAMPLE):
    tau, k, p = settings["temperature"], settings["top_k"], settings["top_p"]
    U, Ud, Ua, Ur = tabs
    rows = out.shape[0]
    nxt, u = rec.first[0]
    assert (u == U[0]).all() and (out[:, t0] == nxt).all()
    g = 1
    unf = np.ones(rows, bool) if eos is None else nxt != eos
    assert passes == 1 + len(rec.rounds) and len(log) == len(rec.rounds) >= 1
    skipped = total = compared = accepted = 0
    sum_min = []
    for r, ((block, kw, res, common, dl), (lo, acc_log)) in enumerate(zip(rec.rounds, log)):
        view, T = kw["rejector"], block.shape[1]
        assert view.step0 == g and view.n_steps == new, (r, view.step0, g)
        active = np.asarray(kw["active"]).astype(bool)
        if eos is not None:
            assert active.tolist() == unf.tolist()
        sup, n_sup = kw.get("suppress_token", -1), kw.get("n_suppress", 0)
        ref = R.positions(res.logits.float().cpu().numpy(), dl, block, tau, k, p, Ua, Ur, g, sup, n_sup)
        tok, ok = res.greedy.cpu().numpy(), res.ok.cpu().numpy()
        pt, qt = res.p_tok.cpu().numpy().astype(np.float64), res.q_tok.cpu().numpy().astype(np.float64)
        ud, _ = R.table(Ud, g, rows, T - 1)
        for t in range(T - 1):                          # the contract: the draft tokens are draws of the drafter's own logits
            fq = R.filtered(dl[:, t], tau, k, p, sup if t < n_sup else -1)
            want = R.plain_draw(fq, ud[:, t])
            if t == 0:
                sum_min.append(np.minimum(ref.draws[0].prob, fq.prob).sum(axis=1)[active].mean())
            for b in np.flatnonzero(active):
                if fq.margin[b] >= TOL:
                    d = int(block[b, t + 1])
                    assert d == want[b] or draw_acceptable(d, fq.keep[b], fq.cum[b], float(ud[b, t]), TOL), ("draft", r, b, t, d, want[b])
        for b in np.flatnonzero(active):
            for t in range(T):
                total += 1
                if ref.margin[b, t] < TOL:
                    skipped += 1
                    continue
                assert abs(pt[b, t] - ref.p_tok[b, t]) <= 2e-4 and abs(qt[b, t] - ref.q_tok[b, t]) <= 2e-4, (r, b, t)
                if not ref.inside[b, t] or t == T - 1:
                    assert ok[b, t] == 0
                elif abs(float(ref.u_acc[b, t]) * ref.q_tok[b, t] - ref.p_tok[b, t]) >= TOL:
                    compared += 1
                    accepted += int(ok[b, t])
                    assert ok[b, t] == ref.ok[b, t], (r, b, t)
                if t == T - 1 or ref.plain[b, t]:
                    f = ref.draws[t]
                    assert tok[b, t] == ref.token[b, t] or draw_acceptable(int(tok[b, t]), f.keep[b], f.cum[b], float(ref.u_res[b, t]), TOL)
                elif ref.resid[b, t] < 1e-3:
                    skipped += 1
                else:
                    assert tok[b, t] == ref.token[b, t] or draw_acceptable(int(tok[b, t]), ref.r[b, t] > 0, ref.rcum[b, t], float(ref.u_res[b, t]),
                                                                             TOL / ref.resid[b, t]), (r, b, t, tok[b, t], ref.token[b, t])
        acc, com, nx = R.accept(block, tok, ok, active.astype(int))
        assert (res.accepted.cpu().numpy() == acc).all() and int(res.common.cpu()[0]) == com and (res.next.cpu().numpy() == nx).all()
        assert (lo, acc_log) == (com, acc.tolist()) and common == com
        for i in range(com + 1):                        # the output is exactly what the round kept
            kept = block[:, i + 1] if i < com else nx
            tokens = np.where(unf, kept, pad) if eos is not None else kept
            assert (out[:, t0 + g] == tokens).all(), (r, i)
            g += 1
            newly = eos is not None and bool((unf & (tokens == eos)).any())
            if eos is not None:
                unf &= tokens != eos
            if newly or not unf.any() or g >= new:
                break
    assert out.shape[1] == t0 + g and (g == new or not unf.any())
    assert skipped * 8 <= total, (skipped, total)
    first = [a >= 1 for (_, acc_log), (_, kw, _, _, _) in zip(log, rec.rounds) for a, on in zip(acc_log, np.asarray(kw["active"])) if on]
    print(f"\nrounds {len(log)}, first draft token accepted on {np.mean(first):.3f} of {len(first)} (round, active row) pairs, mean sum min(p, q) "
          f"{np.mean(sum_min):.3f}; accept decisions compared {compared} (accepted {accepted}), positions skipped {skipped} of {total}")
    return compared


def fresh(seed=SEED, heads=C["heads"]):
    from lia_amd.generation import _scheduler_of
    from lia_amd.model import LiaOPTModel, OPTShape
    m = synth.make_model(seed, C["vocab"], C["max_pos"], C["H"], C["F"], C["L"], W_STD)
    model = LiaOPTModel.from_numpy(OPTShape("reject", C["H"], heads, C["F"], C["L"], vocab=C["vocab"], max_pos=C["max_pos"]), m)
    _scheduler_of(model)
    return m, model


def run(model, prompt, draft, k, flags, seed, new=NEW, settings=SAMPLE, **kw):
    import torch
    from lia_amd.generation import generate
    rec, log = Recorder(model._lia_scheduler), []
    res = generate(model, torch.from_numpy(prompt), max_new_tokens=new, token_latency=True, draft=draft, draft_tokens=k, spec_log=log,
                   sampled_verify=True, verify_rule="rejection", sample_seed=seed, **{"eos_token_id": None, **settings, **flags, **kw})
    return res, log, rec


def recorded_case(flags, k, seed, heads=C["heads"], draft_seed=SEED + 1, **kw):
    from lia_amd.speculative import ModelDrafter
    prompt = _ids(1, (B, T0))
    _, model = fresh(heads=heads)
    _, dmodel = fresh(seed=draft_seed, heads=heads)
    try:
        (out, lat), log, rec = run(model, prompt, ModelDrafter(dmodel, stochastic=True), k, flags, seed, **kw)
        compared = check_rounds(rec, out.numpy(), log, len(lat), tables(NEW, B, seed), T0, eos=kw.get("eos_token_id"))
        return out.numpy(), log, rec, compared
    finally:
        _close(model)
        _close(dmodel)


@pytest.mark.parametrize("name,flags", POLICIES, ids=[n for n, _ in POLICIES])
@pytest.mark.parametrize("k", [1, 4])
def test_recorded_rounds(name, flags, k):
    _, _, _, compared = recorded_case(flags, k, 5)
    assert compared > 0


def test_recorded_rounds_head_dim_64():
    recorded_case(POLICIES[0][1], 3, 6, heads=4)


def test_recorded_rounds_llama():
    from lia_amd.llama import LiaLlamaModel, LlamaScheduler, LlamaShape
    from lia_amd.speculative import ModelDrafter
    H, heads, kvh, F, L, vocab, theta = 256, 4, 1, 512, 3, 256, 10000.0
    prompt = _ids(1, (B, T0))
    flags = dict(gpu_percentage=100, pin_weight=True)

    def llama(seed):
        m = synth.make_llama_model(seed, vocab, H, heads, kvh, F, L, 0.12)
        model = LiaLlamaModel.from_numpy(LlamaShape("t", H, heads, kvh, F, L, vocab, max_pos=64, rope_theta=theta), m)
        model._lia_scheduler = LlamaScheduler(model, pack="raw")
        return model

    model, dmodel = llama(3), llama(4)
    try:
        (out, lat), log, rec = run(model, prompt, ModelDrafter(dmodel, stochastic=True), 3, flags, 4)
        check_rounds(rec, out.numpy(), log, len(lat), tables(NEW, B, 4), T0)
    finally:
        _close(model)
        _close(dmodel)


def test_eos_min_new_tokens_and_pad():
    """a token the rows emit often is made EOS: never before min_new_tokens, only pad behind it, every round still pinned"""
    flags = POLICIES[1][1]
    free, _, _, _ = recorded_case(flags, 4, 9)
    vals, counts = np.unique(free[:, T0 + 4:], return_counts=True)
    eos = int(vals[np.argmax(counts)])
    out, log, rec, _ = recorded_case(flags, 4, 9, eos_token_id=eos, pad_token_id=1, min_new_tokens=4)
    gen = out[:, T0:]
    assert (gen[:, :4] != eos).all()
    print(f"\nEOS {eos} emitted on {int((gen == eos).any(axis=1).sum())} of {B} rows")
    for b in range(B):
        hit = np.flatnonzero(gen[b] == eos)
        if hit.size:
            assert (gen[b, hit[0] + 1:] == 1).all()
    assert rec.rounds[0][1]["suppress_token"] == eos


def test_a_drafter_with_the_targets_weights():
    """Q is P up to the rounding between a decode step and a verify pass: the accept decisions are those of the recorded p and q (the
    kernel's own), whatever their rate"""
    out, log, rec, compared = recorded_case(POLICIES[0][1], 4, 11, draft_seed=SEED)
    n = agree = 0
    for _, kw, res, _, _ in rec.rounds:
        view = kw["rejector"]
        T = res.ok.shape[1]
        ua, inside = R.table(view.u_acc.cpu().numpy(), view.step0, B, T)
        pt, qt, ok = res.p_tok.cpu().numpy().astype(np.float64), res.q_tok.cpu().numpy().astype(np.float64), res.ok.cpu().numpy()
        for b in range(B):
            for t in range(T - 1):
                if inside[b, t] and abs(ua[b, t] * qt[b, t] - pt[b, t]) >= TOL:
                    n += 1
                    assert ok[b, t] == int(qt[b, t] > 0 and ua[b, t] * qt[b, t] < pt[b, t])
                    agree += int(ok[b, t])
    print(f"\nthe target's own weights: {agree} of {n} compared accept decisions accepted")
    assert n > 0


def test_top_k_one_gives_the_greedy_ids(oracle):
    """on rows the oracle finds free of near-ties: the rejection rule at top_k = 1 is greedy decoding, whatever the drafter proposes"""
    import torch
    from lia_amd.generation import generate
    from lia_amd.speculative import ModelDrafter
    from test_gpu_speculative import pool_run
    flags = POLICIES[1][1]
    m, model = _opt()
    _, dmodel = fresh(seed=SEED + 1)
    try:
        prompt, pool = pool_run(oracle, m, flags)
        pick, _ = choose_rows(pool)
        prompt = prompt[pick]
        plain = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, **flags).numpy()
        for k in (1, 4):
            log = []
            got = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, draft=ModelDrafter(dmodel, stochastic=True),
                           draft_tokens=k, spec_log=log, do_sample=True, top_k=1, temperature=1.3, top_p=0.9, sample_seed=3,
                           sampled_verify=True, verify_rule="rejection", **flags).numpy()
            assert (got == plain).all(), (k, got.tolist(), plain.tolist())
            assert len(log) >= 1
    finally:
        _close(model)
        _close(dmodel)


def test_all_ones_mask_and_no_state_left_behind():
    import torch
    from lia_amd.generation import generate
    flags = POLICIES[1][1]
    prompt = _ids(1, (B, T0))
    base, _, _, _ = recorded_case(flags, 3, 13)
    masked, _, _, _ = recorded_case(flags, 3, 13, attention_mask=torch.ones((B, T0), dtype=torch.int64))
    assert (base == masked).all()
    _, model = fresh()
    _, dmodel = fresh(seed=SEED + 1)
    try:
        from lia_amd.speculative import ModelDrafter
        want = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, **flags).numpy()
        generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, draft=ModelDrafter(dmodel, stochastic=True), draft_tokens=3,
                 sampled_verify=True, verify_rule="rejection", sample_seed=13, **SAMPLE, **flags)
        again = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, **flags).numpy()
        assert (want == again).all()
    finally:
        _close(model)
        _close(dmodel)
