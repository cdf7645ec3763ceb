"""-m gpu: generate(repetition_penalty= / presence_penalty= / frequency_penalty=) end to end on the tiny OPT and the tiny Llama of
test_gpu_constrained_generate.py, 8 rows x 8 prompt tokens x 12 new tokens.

Exact throughout.  return_logits=True hands back the RAW logits of every step, so a greedy id is checked against the first argmax of
penalty_ref(raw logits[t], the table rebuilt in NumPy from the row's own history), and a sampled id against lia_sample without a
table on those rewritten logits with the step's U[t, b].  The plain greedy run of these prompts repeats tokens inside its rows
(checked on the CPU oracle for seeds 5 .. 8 of both models), so a run that ignores the keywords fails both the per-step check and
the comparison with the plain run."""
import numpy as np
import pytest

import mask_ref as MR
import penalty_ref as PR
from test_gpu_constrained_generate import MODELS, _close

pytestmark = pytest.mark.gpu

B, T, NEW = 8, 8, 12
SETTINGS = [(1.8, 0.0, 0.0), (1.0, 1.0, 0.5)]


def _kw(s):
    return dict(repetition_penalty=s[0], presence_penalty=s[1], frequency_penalty=s[2])


def _gen(model, prompt, flags, new=NEW, eos=None, **kw):
    import torch
    from lia_amd.generation import generate
    return generate(model, torch.as_tensor(prompt), max_new_tokens=new, eos_token_id=eos, **flags, **kw)


def _u16(lg):
    import torch
    return lg.view(torch.int16).cpu().numpy().view(np.uint16)


def _rewritten(lgs, t, prompt, history, vocab, s, starts=None):
    """penalty_ref of step t's raw logits under the table of (prompt, what every row generated before step t)"""
    table = PR.build_counts(prompt, history[:, :t], vocab, starts=starts)
    return PR.penalty_ref(_u16(lgs[t]), table, *s)


def _check_greedy(out, lgs, prompt, vocab, s, starts=None, suppress=lambda t: -1, live=None, allowed=None, what=""):
    Tp = prompt.shape[1]
    gen = out[:, Tp:]
    for t in range(gen.shape[1]):
        rows = _rewritten(lgs, t, prompt, gen, vocab, s, starts)
        if allowed is None:
            want = PR.first_argmax(rows, suppress(t))
        else:
            want = MR.first_argmax(PR.bf16_to_f32(rows), allowed, suppress(t))
        ok = gen[:, t] == want
        if live is not None:
            ok = ok | ~live[:, t]
        assert ok.all(), (what, t, gen[:, t], want)


def _repeating_prompts(model, vocab, flags):
    """prompts whose PLAIN greedy run repeats a token inside some row (redrawn from the next seed, at most eight times), and that run"""
    for seed in range(5, 13):
        prompt = np.random.RandomState(seed).randint(3, vocab, (B, T)).astype(np.int64)
        plain, _, plain_lg = _gen(model, prompt, flags, return_logits=True)
        plain = plain.numpy()
        if any(len(set(r[T:].tolist())) < NEW for r in plain):
            return prompt, plain, plain_lg
    raise AssertionError("the plain greedy run repeated no token in eight draws of the prompts")


@pytest.mark.parametrize("family", ["opt", "llama"])
def test_greedy_and_sampled(family):
    import torch
    from lia_amd import ops, sampling
    model, vocab, flags = MODELS[family]()
    fresh, _, _ = MODELS[family]()
    try:
        prompt, plain, plain_lg = _repeating_prompts(model, vocab, flags)
        for s in SETTINGS:
            out, _, lgs = _gen(model, prompt, flags, return_logits=True, **_kw(s))
            out = out.numpy()
            assert out.shape == (B, T + NEW) and len(lgs) == NEW and (out[:, :T] == prompt).all()
            assert torch.equal(lgs[0], plain_lg[0])                         # step 0's raw logits do not know about the penalties
            _check_greedy(out, lgs, prompt, vocab, s, what=s)
            assert (out != plain).any(), s
        # sampled: tau 0.7, top-k 50, top-p 0.9
        s = (1.8, 0.5, 0.25)
        tau, k, p, sseed = 0.7, 50, 0.9, 11
        sout, _, slgs = _gen(model, prompt, flags, return_logits=True, do_sample=True, temperature=tau, top_k=k, top_p=p, sample_seed=sseed,
                             **_kw(s))
        sout = sout.numpy()
        U = sampling.draw_uniforms(NEW, B, sseed)
        ctx = ops.Context(0, 1 << 20)
        try:
            for t in range(NEW):
                rows = torch.from_numpy(_rewritten(slgs, t, prompt, sout[:, T:], vocab, s).view(np.int16)).cuda().view(torch.bfloat16)
                torch.cuda.synchronize()
                want = ctx.sample(rows, tau, k, p, U[t].contiguous())
                ctx.synchronize()
                assert (sout[:, T + t] == want.cpu().numpy()).all(), t
        finally:
            ctx.close()
        psout = _gen(model, prompt, flags, do_sample=True, temperature=tau, top_k=k, top_p=p, sample_seed=sseed).numpy()
        assert (sout != psout).any()
        # hygiene: a plain generate() afterwards is a fresh model's, byte for byte, and no table is left behind
        again = _gen(model, prompt, flags).numpy()
        ref = _gen(fresh, prompt, flags).numpy()
        assert again.tobytes() == ref.tobytes() == plain.tobytes()
        assert model._lia_scheduler.ctx._penalties is None
        # neutral values are the plain call
        assert _gen(model, prompt, flags, **_kw((1.0, 0.0, 0.0))).numpy().tobytes() == plain.tobytes()
    finally:
        _close(model)
        _close(fresh)


def test_left_padding_minibatches_eos_and_min_new_tokens():
    import torch
    model, vocab, flags = MODELS["opt"]()
    try:
        s = (1.8, 0.4, 0.2)
        prompt, plain, _ = _repeating_prompts(model, vocab, flags)
        # a left-padded batch: the pads are not counted.  Probe: the padded positions hold the very token the row emits first --
        # were they counted, that token's logit would be penalised at step 0
        starts = np.array([0, 3, 0, 5, 1, 0, 7, 2])
        mask = (np.arange(T)[None, :] >= starts[:, None]).astype(np.int64)
        padded = prompt.copy()
        padded[mask == 0] = 1
        a, _, a_lg = _gen(model, padded, flags, return_logits=True, attention_mask=torch.from_numpy(mask), **_kw(s))
        a = a.numpy()
        _check_greedy(a, a_lg, padded, vocab, s, starts=starts, what="padded")
        probe = padded.copy()
        for b in range(B):
            probe[b, :starts[b]] = a[b, T]
        b_, _, b_lg = _gen(model, probe, flags, return_logits=True, attention_mask=torch.from_numpy(mask), **_kw(s))
        assert (b_.numpy()[:, T:] == a[:, T:]).all() and torch.equal(b_lg[0], a_lg[0])
        # num_minibatch = 2
        mb = dict(flags, gpu_percentage=50, num_minibatch=2)
        out, _, lgs = _gen(model, prompt, mb, return_logits=True, **_kw(s))
        _check_greedy(out.numpy(), lgs, prompt, vocab, s, what="minibatch")
        base, _, base_lg = _gen(model, prompt, flags, return_logits=True, **_kw(s))
        base = base.numpy()
        assert (base != plain).any()
        # eos: a row finishes early, emits the pad fill from there on and its counts stop; the other rows go on
        gen = base[:, T:]
        r, k, tok = next((r, k, int(gen[r, k])) for k in range(2, NEW - 2) for r in range(B)
                         if gen[r, k] not in gen[r, :k] and gen[r, k] not in np.delete(gen, r, axis=0)[:, :k + 1] and gen[r, k] != 1)
        out, _, lgs = _gen(model, prompt, flags, eos=tok, return_logits=True, pad_token_id=1, **_kw(s))
        out = out.numpy()
        assert out[r, T + k] == tok and (out[r, T + k + 1:] == 1).all()
        live = np.ones((B, out.shape[1] - T), bool)
        for b in range(B):
            hit = np.flatnonzero(out[b, T:] == tok)
            if hit.size:
                live[b, hit[0] + 1:] = False
        _check_greedy(out, lgs, prompt, vocab, s, live=live, what="eos")
        assert live[:, -1].any()
        # min_new_tokens: EOS counts as -inf in front of the penalised argmax while fewer were generated
        out, _, lgs = _gen(model, prompt, flags, eos=tok, min_new_tokens=k + 2, return_logits=True, pad_token_id=1, **_kw(s))
        out = out.numpy()
        assert (out[:, T:T + k + 2] != tok).all() and (out[:, T:T + k] == base[:, T:T + k]).all()
        live = np.ones((B, out.shape[1] - T), bool)
        for b in range(B):
            hit = np.flatnonzero(out[b, T:] == tok)
            if hit.size:
                live[b, hit[0] + 1:] = False
        _check_greedy(out, lgs, prompt, vocab, s, suppress=lambda t: tok if t < k + 2 else -1, live=live, what="min_new_tokens")
    finally:
        _close(model)


@pytest.mark.parametrize("family", ["opt", "llama"])
def test_second_turn_counts_the_whole_conversation(family):
    """past=: the table's prompt bits are the whole conversation's tokens -- turn 1's prompt, what turn 1 generated, the follow-up --
    probed through the ids turn 2 emits; its generated counts start at zero"""
    import torch
    model, vocab, flags = MODELS[family]()
    try:
        s = (1.8, 0.0, 0.7)
        prompt, _, _ = _repeating_prompts(model, vocab, flags)
        out1, _, lg1, state = _gen(model, prompt, flags, new=4, return_logits=True, return_state=True, reserve_tokens=8, **_kw(s))
        _check_greedy(out1.numpy(), lg1, prompt, vocab, s, what="turn 1")
        follow = np.random.RandomState(2).randint(3, vocab, (B, 2)).astype(np.int64)
        out2, _, lg2, _ = _gen(model, follow, flags, new=5, return_logits=True, return_state=True, past=state, **_kw(s))
        out2 = out2.numpy()
        convo = np.concatenate([out1.numpy(), follow], axis=1)
        assert (out2[:, :convo.shape[1]] == convo).all() and out2.shape[1] == convo.shape[1] + 5
        _check_greedy(out2, lg2, convo, vocab, s, what="turn 2")
        # a table that knew the follow-up alone would have picked other ids from the same raw logits somewhere in the turn
        n0 = convo.shape[1]
        short = np.stack([PR.first_argmax(_rewritten(lg2, t, follow, out2[:, n0:], vocab, s)) for t in range(5)], axis=1)
        assert (short != out2[:, n0:]).any()
    finally:
        _close(model)


def test_with_suppress_tokens_and_logprobs():
    import torch
    from lia_amd import ops
    model, vocab, flags = MODELS["opt"]()
    try:
        s = (1.8, 0.4, 0.2)
        prompt, _, _ = _repeating_prompts(model, vocab, flags)
        base = _gen(model, prompt, flags, **_kw(s)).numpy()
        banned = sorted(set(base[:, T:T + 3].reshape(-1).tolist()))          # what the penalised run emits first
        allowed = np.ones((B, vocab), bool)
        allowed[:, banned] = False
        out, _, lgs, lp = _gen(model, prompt, flags, return_logits=True, suppress_tokens=banned, logprobs=3, **_kw(s))
        out = out.numpy()
        assert not np.isin(out[:, T:], banned).any() and (out != base).any()
        _check_greedy(out, lgs, prompt, vocab, s, allowed=allowed, what="suppress_tokens")
        ctx = ops.Context(0, 1 << 20)
        try:
            for t in range(NEW):
                torch.cuda.synchronize()
                chosen, top_ids, top = ctx.topn_logprobs(lgs[t], torch.from_numpy(out[:, T + t]).cuda(), 3)    # the RAW logits
                ctx.synchronize()
                assert (lp.top_ids[:, t] == top_ids.cpu()).all()
                assert (lp.top_logprobs[:, t].numpy().view(np.int32) == top.cpu().numpy().view(np.int32)).all()
                assert (lp.token_logprobs[:, t].numpy().view(np.int32) == chosen.cpu().numpy().view(np.int32)).all()
        finally:
            ctx.close()
    finally:
        _close(model)


def test_draft_and_data_parallel_refuse_by_name():
    model, vocab, flags = MODELS["opt"]()
    try:
        prompt = np.random.RandomState(5).randint(3, vocab, (B, T)).astype(np.int64)
        plain = _gen(model, prompt, flags).numpy()
        sched = model._lia_scheduler
        forwards, real_forward = [], sched.forward
        sched.forward = lambda *a, **kw: (forwards.append(1), real_forward(*a, **kw))[1]      # (counts the real scheduler's forwards)
        with pytest.raises(ValueError, match=r"repetition_penalty=1\.8 together with draft="):
            _gen(model, prompt, flags, draft=object(), repetition_penalty=1.8)
        sched.dp = object()
        try:
            with pytest.raises(ValueError, match=r"presence_penalty=0\.5 together with a data-parallel group"):
                _gen(model, prompt, flags, presence_penalty=0.5)
        finally:
            sched.dp = None
        assert forwards == [] and sched.ctx._penalties is None       # refused before any forward
        assert _gen(model, prompt, flags).numpy().tobytes() == plain.tobytes() and len(forwards) == NEW
    finally:
        _close(model)
