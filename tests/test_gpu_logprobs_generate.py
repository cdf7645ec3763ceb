"""-m gpu: generate(..., logprobs=N) end to end on the tiny OPT of test_gpu_padded.py and the tiny Llama of test_gpu_llama.py.

return_logits=True hands back the raw logits of every step, so every step's TokenLogprobs is held against tests/logprob_ref.py on
those very logits: ids exactly, values within score_ref.row_kernel_bound (the bound of the row kernel that computes them).  The ids,
the logits and the number of latency entries are those of the run without the keyword.  Speculative runs are held against what the
verify passes themselves report, never against the plain run's values (a verify pass and a decode step round differently); the
largest difference seen is printed."""
import os

import numpy as np
import pytest

import logprob_ref as LR
import score_ref as SR
import synth
import test_gpu_padded as TP

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW, NTOP = 4, 3


def _llama():
    from lia_amd.llama import LiaLlamaModel, LlamaShape
    z = np.load(os.path.join(GOLD, "llama_generate_h256.npz"))
    vocab, H, heads, kvh, F, L, _, _, _, seed = [int(v) for v in z["cfg"]]
    m = synth.make_llama_model(seed, vocab, H, heads, kvh, F, L, float(z["w_std"][0]))
    return LiaLlamaModel.from_numpy(LlamaShape("t", H, heads, kvh, F, L, vocab, max_pos=64, rope_theta=float(z["theta"][0])), m), vocab


def _close(model):
    if getattr(model, "_lia_scheduler", None) is not None:
        model._lia_scheduler.close()
    model.close()


def _bits(lg):
    import torch
    return lg.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def check_against_logits(lp, logits_list, new_ids, n_top, what, live=None):
    """step s of lp against the reference on logits_list[s] with the emitted ids new_ids[:, s]; live [B, steps] bool (or None):
    where a row had not finished before the step -- elsewhere the fills"""
    from lia_amd import _native as N
    worst = 0.0
    B = new_ids.shape[0]
    assert tuple(lp.token_logprobs.shape) == new_ids.shape and tuple(lp.top_ids.shape) == new_ids.shape + (n_top,)
    assert not lp.token_logprobs.is_cuda and not lp.top_ids.is_cuda and not lp.top_logprobs.is_cuda
    for s, lg in enumerate(logits_list):
        bits = _bits(lg)
        vocab = bits.shape[1]
        want_c, want_ids, want_lp, m, ls = LR.topn_logprobs(bits, new_ids[:, s], n_top)
        rows = np.ones(B, bool) if live is None else live[:, s]
        got_c = lp.token_logprobs[:, s].numpy().astype(np.float64)
        got_ids = lp.top_ids[:, s].numpy()
        got_lp = lp.top_logprobs[:, s].numpy().astype(np.float64)
        assert (got_ids[rows] == want_ids[rows]).all(), (what, s, got_ids.tolist(), want_ids.tolist())
        assert (got_c[~rows] == 0.0).all() and (got_ids[~rows] == -1).all() and np.isneginf(got_lp[~rows]).all(), (what, s)
        for got, want in [(got_c, want_c)] + [(got_lp[:, j], want_lp[:, j]) for j in range(n_top)]:
            bound = SR.row_kernel_bound(m, ls, want, N.score_serial_terms(vocab), N.SCORE_ROW_THREADS)
            err = np.abs(got[rows] - want[rows])
            assert (err <= bound[rows]).all(), (what, s, err.max(), bound[rows].min())
            if rows.any():
                worst = max(worst, float(np.max(err / bound[rows])))
    return worst


SAMPLE = dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9, sample_seed=11)
OPT_CASES = [("3/3 resident", False, True), ("3/3 resident", True, False), ("0/2", False, False), ("0/2", True, True), ("1/1", False, True),
             ("1/1", True, True), ("0/2 ragged minibatches", False, True), ("0/2 + cpu_layers", False, True)]


@pytest.mark.parametrize("pname,sampled,padded", OPT_CASES)
def test_opt_logprobs_equal_the_reference_on_the_returned_logits(pname, sampled, padded):
    """greedy and sampled, policy pairs 3/3, 0/2, 1/1, minibatches and cpu_layers, the left-padded batch and the unpadded one"""
    import torch
    from lia_amd.generation import generate
    kw = dict(TP.POLICIES[pname], pin_weight=True, max_new_tokens=NEW, eos_token_id=None, return_logits=True, **(SAMPLE if sampled else {}))
    ids, mask = TP._batch()
    if padded:
        kw["attention_mask"] = torch.from_numpy(mask)
    else:
        ids = ids[:, -3:]                                                    # (the columns every row holds real tokens in but one row's)
        ids = ids[[0, 2, 3]]
    T = ids.shape[1]
    _, model = TP._model("d64")
    try:
        out0, lat0, lg0 = generate(model, torch.from_numpy(ids), **kw)
        out, lat, lg, lp = generate(model, torch.from_numpy(ids), logprobs=NTOP, **kw)
        assert torch.equal(out, out0) and len(lat) == len(lat0) == NEW and all(torch.equal(a, b) for a, b in zip(lg, lg0))
        worst = check_against_logits(lp, lg, out[:, T:].numpy(), NTOP, pname)
        assert torch.equal(lp.sequence_logprob(), lp.token_logprobs.sum(dim=1))
        if not sampled:
            assert torch.equal(lp.top_ids[:, :, 0], out[:, T:])              # nothing suppressed: the argmax leads, with its own value
            assert torch.equal(lp.token_logprobs, lp.top_logprobs[:, :, 0])
        print(f"\n{pname} sampled={sampled} padded={padded}: max |err| / bound {worst:.3f}")
        assert model._lia_scheduler.ctx._logprob_sink is None
        again = generate(model, torch.from_numpy(ids), **kw)                  # the sink is gone: today's result
        assert torch.equal(again[0], out0) and len(again) == 3
    finally:
        _close(model)


@pytest.mark.parametrize("sampled", [False, True])
def test_llama_logprobs_equal_the_reference_on_the_returned_logits(sampled):
    import torch
    from lia_amd.generation import generate
    model, vocab = _llama()
    try:
        ids = np.random.RandomState(5).randint(3, vocab, (4, 7)).astype(np.int64)
        for flags in (dict(gpu_percentage=100, pin_weight=True), dict(gpu_percentage=34, num_minibatch=2, pin_weight=True)):
            kw = dict(flags, max_new_tokens=NEW, eos_token_id=None, return_logits=True, **(SAMPLE if sampled else {}))
            out0, _, lg0 = generate(model, torch.from_numpy(ids), **kw)
            out, lat, lg, lp = generate(model, torch.from_numpy(ids), logprobs=5, **kw)
            assert torch.equal(out, out0) and len(lat) == NEW and all(torch.equal(a, b) for a, b in zip(lg, lg0))
            worst = check_against_logits(lp, lg, out[:, 7:].numpy(), 5, f"llama {flags}")
            print(f"\nllama {flags} sampled={sampled}: max |err| / bound {worst:.3f}")
    finally:
        _close(model)


def test_eos_fills_and_the_state_of_a_second_turn():
    """an eos_token_id picked the way test_eos_in_a_padded_batch picks one: the finished row's later steps hold the fills; then two
    turns -- each returns its own tokens' values, with the state last"""
    import torch
    from lia_amd.generation import GenerationState, generate
    kw = dict(TP.POLICIES["0/2"], pin_weight=True)
    ids, mask = TP._batch()
    T, N_ = ids.shape[1], 6
    _, model = TP._model("d64")
    try:
        t_ids, t_mask = torch.from_numpy(ids), torch.from_numpy(mask)
        first = generate(model, t_ids, attention_mask=t_mask, max_new_tokens=N_, eos_token_id=None, **kw).numpy()
        gen = first[:, T:]
        pick = next((r, k, int(gen[r, k])) for k in range(1, N_ - 1) for r in range(gen.shape[0])
                    if gen[r, k] not in gen[r, :k] and gen[r, k] not in np.delete(gen, r, axis=0) and gen[r, k] != 1)
        r, k, tok = pick
        out, _, lg, lp = generate(model, t_ids, attention_mask=t_mask, max_new_tokens=N_, eos_token_id=tok, pad_token_id=1,
                                  return_logits=True, logprobs=NTOP, **kw)
        assert (out[r, T + k + 1:] == 1).all() and out[r, T + k] == tok
        live = np.ones((ids.shape[0], N_), bool)
        live[r, k + 1:] = False
        check_against_logits(lp, lg, out[:, T:].numpy(), NTOP, "eos", live)
        assert (lp.token_logprobs[r, k + 1:] == 0).all() and lp.token_logprobs[r, k] < 0
        # two turns
        res = generate(model, t_ids, attention_mask=t_mask, max_new_tokens=3, eos_token_id=None, return_logits=True, logprobs=NTOP,
                       return_state=True, reserve_tokens=8, **kw)
        assert len(res) == 5 and isinstance(res[4], GenerationState)
        check_against_logits(res[3], res[2], res[0][:, T:].numpy(), NTOP, "turn 1")
        follow = torch.from_numpy(np.random.RandomState(2).randint(3, TP.VOCAB, (ids.shape[0], 2)).astype(np.int64))
        res2 = generate(model, follow, past=res[4], max_new_tokens=3, eos_token_id=None, return_logits=True, logprobs=NTOP,
                        return_state=True, **kw)
        n0 = res[0].shape[1] + 2
        assert res2[0].shape[1] == n0 + 3 and res2[3].token_logprobs.shape == (ids.shape[0], 3)
        check_against_logits(res2[3], res2[2], res2[0][:, n0:].numpy(), NTOP, "turn 2")
    finally:
        _close(model)


def test_the_distribution_is_the_models_own_under_suppress_tokens():
    """suppress_tokens = every row's unconstrained first token: the run emits something else, yet the suppressed argmax leads
    top_ids and the emitted token's own log-probability is in token_logprobs"""
    import torch
    from lia_amd.generation import generate
    kw = dict(TP.POLICIES["3/3 resident"], pin_weight=True, max_new_tokens=NEW, eos_token_id=None, return_logits=True)
    ids, _ = TP._batch()
    ids = ids[[0, 3], -9:]
    T = ids.shape[1]
    _, model = TP._model("d64")
    try:
        free, _, _ = generate(model, torch.from_numpy(ids), **kw)
        banned = sorted(set(free[:, T].tolist()))
        out, _, lg, lp = generate(model, torch.from_numpy(ids), suppress_tokens=banned, logprobs=NTOP, **kw)
        assert not np.isin(out[:, T:].numpy(), banned).any()
        assert torch.equal(lp.top_ids[:, 0, 0], free[:, T])                  # the forbidden argmax is still the first alternative
        assert (lp.token_logprobs[:, 0] < lp.top_logprobs[:, 0, 0]).all()
        check_against_logits(lp, lg, out[:, T:].numpy(), NTOP, "suppress_tokens")
        for b in range(out.shape[0]):                                        # the emitted token's value, in the top N or not
            for s in range(NEW):
                hit = (lp.top_ids[b, s] == out[b, T + s]).nonzero()
                if len(hit):
                    assert lp.top_logprobs[b, s, int(hit[0])] == lp.token_logprobs[b, s]
    finally:
        _close(model)


@pytest.mark.parametrize("family,sampled", [("opt", False), ("opt", True), ("llama", False)])
def test_speculation_keeps_what_the_verify_passes_report(family, sampled):
    """ReplayDrafter with a script of mixed acceptance, the greedy verify head and sampled_verify with the draw rule: the ids are the
    plain run's; one entry per emitted token; round by round the kept values are rows 0 .. common of what that round's
    sched.verify(..., logprobs=) call reported"""
    import torch
    from lia_amd.generation import generate
    from lia_amd.speculative import ReplayDrafter
    n_new, k = 9, 3
    if family == "opt":
        _, model = TP._model("d64")
        flags = dict(TP.POLICIES["3/3 resident"], pin_weight=True)
        vocab = TP.VOCAB
    else:
        model, vocab = _llama()
        flags = dict(gpu_percentage=100, pin_weight=True)
    try:
        ids = torch.from_numpy(np.random.RandomState(9).randint(3, vocab, (3, 6)).astype(np.int64))
        T = ids.shape[1]
        kw = dict(flags, max_new_tokens=n_new, eos_token_id=None, **(dict(SAMPLE, top_k=2) if sampled else {}))
        plain, plain_lp = generate(model, ids, logprobs=NTOP, **kw)
        sched = model._lia_scheduler
        reports, ver, fwd = [], sched.verify, sched.forward

        def verify(block, kv, **vkw):
            res, common = ver(block, kv, **vkw)
            req = vkw["logprobs"]
            reports.append((common, req.chosen.cpu(), req.top_ids.cpu(), req.top_logprobs.cpu(), res.greedy.cpu()))
            return res, common

        def forward(cur, kv, **fkw):
            r = fwd(cur, kv, **fkw)
            req = fkw["logprobs"]
            reports.append((0, req.chosen.cpu()[:, None], req.top_ids.cpu()[:, None], req.top_logprobs.cpu()[:, None], r[1].cpu()[:, None]))
            return r

        sched.verify, sched.forward = verify, forward
        log = []
        try:
            out, lp = generate(model, ids, logprobs=NTOP, draft=ReplayDrafter(plain, [[3, 3, 3], [1, 3, 2], [0, 2, 3], [3, 3, 3]]),
                               draft_tokens=k, spec_log=log, **(dict(sampled_verify=True) if sampled else {}), **kw)
        finally:
            del sched.verify, sched.forward
        assert torch.equal(out, plain) and lp.token_logprobs.shape == (3, n_new) and lp.top_ids.shape == (3, n_new, NTOP)
        assert len({c for c, _ in log}) > 1 and len(reports) == len(log) + 1
        step = 0
        for common, chosen, top_ids, top_lp, emitted in reports:
            n = min(common + 1, n_new - step)
            assert torch.equal(out[:, T + step:T + step + n], emitted[:, :n])
            assert torch.equal(lp.token_logprobs[:, step:step + n], chosen[:, :n])
            assert torch.equal(lp.top_ids[:, step:step + n], top_ids[:, :n]) and torch.equal(lp.top_logprobs[:, step:step + n], top_lp[:, :n])
            step += n
        assert step == n_new
        diff = (lp.token_logprobs - plain_lp.token_logprobs).abs().max().item()
        print(f"\n{family} sampled={sampled}: largest |verify-pass logprob - decode-step logprob| over {3 * n_new} tokens: {diff:.4g}")
        assert model._lia_scheduler.ctx._logprob_sink is None
    finally:
        _close(model)
