"""-m gpu: constrained decoding end to end -- generate(prefix_allowed_tokens_fn= / allowed_mask_fn= / suppress_tokens= /
begin_suppress_tokens=) on the tiny OPT of test_gpu_sampling.py and the tiny Llama of test_gpu_llama.py, 8 rows x 8 new tokens.

Exact throughout.  return_logits=True hands back the RAW logits of every step, so a greedy id is checked against mask_ref's first
argmax over the row's allowed entries of that step's logits, and a sampled id against lia_sample (no table) on those logits with -inf
at the disallowed entries and the step's U[t, b].  The unconstrained control -- the same prompts leave the sets -- is what fails
where the kwarg is silently ignored."""
import os

import numpy as np
import pytest

import mask_ref as MR
import synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B, T, NEW = 8, 8, 8
SEED = 2024                       # of the allowed sets; redrawn from SEED + 1, ... while the unconstrained control stays inside them
OPT_FLAGS = dict(prefill_policy=0, decoding_policy=2, gpu_percentage=34, pin_weight=True)
LLAMA_FLAGS = dict(gpu_percentage=100, pin_weight=True)


def _opt():
    from test_gpu_generate import _load, _model
    z, m, _, c = _load("generate_tiny")
    return _model(m, c), c["vocab"], OPT_FLAGS


def _llama():
    from lia_amd.llama import LiaLlamaModel, LlamaShape
    z = np.load(os.path.join(GOLD, "llama_generate_h256.npz"))
    vocab, H, heads, kvh, F, L, _, _, _, seed = [int(v) for v in z["cfg"]]
    m = synth.make_llama_model(seed, vocab, H, heads, kvh, F, L, float(z["w_std"][0]))
    return LiaLlamaModel.from_numpy(LlamaShape("t", H, heads, kvh, F, L, vocab, max_pos=64, rope_theta=float(z["theta"][0])), m), vocab, LLAMA_FLAGS


MODELS = {"opt": _opt, "llama": _llama}


def _close(model):
    if getattr(model, "_lia_scheduler", None) is not None:
        model._lia_scheduler.close()
    model.close()


def _prompts(vocab, rows=B, seed=5):
    return np.random.RandomState(seed).randint(3, vocab, (rows, T)).astype(np.int64)


def _sets(vocab, rows, seed):
    """allowed [rows, vocab] bool: every row its own random half of the vocabulary (never EOS 2 / pad 1), row 1 two tokens only"""
    rs = np.random.RandomState(seed)
    allowed = rs.rand(rows, vocab) < 0.5
    allowed[:, :3] = False
    allowed[1] = False
    allowed[1, rs.choice(np.arange(3, vocab), 2, replace=False)] = True
    return allowed


def _fn(allowed):
    lists = [np.flatnonzero(a).tolist() for a in allowed]
    return lambda b, row: lists[b]


def _gen(model, prompt, flags, **kw):
    import torch
    from lia_amd.generation import generate
    return generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, **flags, **kw)


def _f32(lg):
    return lg.float().cpu().numpy()


@pytest.mark.parametrize("family", ["opt", "llama"])
def test_greedy_and_sampled_with_prefix_allowed_tokens_fn(family):
    """every emitted id is in its row's set; every greedy id is mask_ref's on that step's returned (raw) logits; every sampled id is
    ctx.sample's on the -inf-substituted logits with U[t, b]; the unconstrained run of the same prompts leaves the sets (redrawn from
    the next seed while it does not); a later unconstrained generate() on the same scheduler is a fresh model's, byte for byte"""
    import torch
    from lia_amd import ops, sampling
    model, vocab, flags = MODELS[family]()
    fresh, _, _ = MODELS[family]()
    try:
        prompt = _prompts(vocab)
        plain, _, plain_lg = _gen(model, prompt, flags, return_logits=True)
        plain = plain.numpy()
        for seed in range(SEED, SEED + 8):
            allowed = _sets(vocab, B, seed)
            if (~allowed[np.arange(B)[:, None], plain[:, T:]]).any():
                break
        else:
            raise AssertionError("the unconstrained run stayed inside eight draws of the sets")
        rows = np.arange(B)
        # greedy
        out, _, lgs = _gen(model, prompt, flags, return_logits=True, prefix_allowed_tokens_fn=_fn(allowed))
        out = out.numpy()
        assert out.shape == (B, T + NEW) and len(lgs) == NEW and (out[:, :T] == prompt).all()
        assert torch.equal(lgs[0], plain_lg[0])                                   # step 0's raw logits do not know about the mask
        for t in range(NEW):
            assert allowed[rows, out[:, T + t]].all(), (t, out[:, T + t])
            assert (out[:, T + t] == MR.first_argmax(_f32(lgs[t]), allowed)).all(), t
        assert (out[:, T:] != plain[:, T:]).any()
        assert len(set(out[1, T:].tolist())) <= 2
        # sampled: tau 0.7, top-k 50 (row 1 has fewer allowed tokens than that), top-p 0.9
        tau, k, p, sseed = 0.7, 50, 0.9, 11
        sout, _, slgs = _gen(model, prompt, flags, return_logits=True, do_sample=True, temperature=tau, top_k=k, top_p=p, sample_seed=sseed,
                             prefix_allowed_tokens_fn=_fn(allowed))
        sout = sout.numpy()
        U = sampling.draw_uniforms(NEW, B, sseed)
        ctx = ops.Context(0, 1 << 20)
        try:
            for t in range(NEW):
                assert allowed[rows, sout[:, T + t]].all(), t
                sub = MR.substitute(torch, slgs[t], allowed)
                torch.cuda.synchronize()
                want = ctx.sample(sub, tau, k, p, U[t].contiguous())
                ctx.synchronize()
                assert (sout[:, T + t] == want.cpu().numpy()).all(), t
        finally:
            ctx.close()
        assert (sout[:, T:] != out[:, T:]).any()
        # hygiene: no table left behind
        again = _gen(model, prompt, flags).numpy()
        ref = _gen(fresh, prompt, flags).numpy()
        assert again.tobytes() == ref.tobytes() == plain.tobytes()
        assert model._lia_scheduler.ctx._token_mask is None
    finally:
        _close(model)
        _close(fresh)


@pytest.mark.parametrize("family", ["opt", "llama"])
def test_cuda_mask_fn_equals_the_prefix_fn(family):
    import torch
    model, vocab, flags = MODELS[family]()
    try:
        prompt = _prompts(vocab, seed=6)
        allowed = _sets(vocab, B, SEED + 20)
        dev = torch.from_numpy(MR.pack(allowed)).cuda()
        shapes = []

        def mask_fn(ids):
            shapes.append(tuple(ids.shape))
            return dev

        a = _gen(model, prompt, flags, prefix_allowed_tokens_fn=_fn(allowed)).numpy()
        b = _gen(model, prompt, flags, allowed_mask_fn=mask_fn).numpy()
        assert (a == b).all() and shapes == [(B, T + i) for i in range(NEW)]
        assert allowed[np.arange(B)[:, None], a[:, T:]].all()
        assert (dev.cpu().numpy() == MR.pack(allowed)).all()                     # the caller's tensor is not written
        # a drafter that knows nothing of the constraint (it replays the unconstrained run) under the CUDA mask: the forbidden
        # proposals are looked up in the device rows; the run ends and stays inside the sets
        from lia_amd.speculative import ReplayDrafter
        log = []
        c = _gen(model, prompt, flags, allowed_mask_fn=mask_fn, draft=ReplayDrafter(_gen(model, prompt, flags).numpy()), draft_tokens=3,
                 spec_log=log).numpy()
        assert allowed[np.arange(B)[:, None], c[:, T:]].all() and len(log) >= 1
        empty = dev.clone()
        empty[5] = 0
        with pytest.raises(ValueError, match="token constraint: row 5 allows no token at step 0"):
            _gen(model, prompt, flags, allowed_mask_fn=lambda ids: empty)
    finally:
        _close(model)


def test_static_lists_begin_suppress_and_eos_below_min_new_tokens_compose():
    """suppress_tokens bans the plain run's favourite tokens at every step, begin_suppress_tokens its first tokens at step 0 only, and
    the token made EOS is suppressed below min_new_tokens by the loop's own switch: each id is mask_ref's under all three"""
    import torch
    from lia_amd.generation import generate
    model, vocab, flags = _opt()
    try:
        prompt = _prompts(vocab, seed=7)
        plain = _gen(model, prompt, flags).numpy()
        firsts = sorted(set(plain[:, T].tolist()))
        vals, counts = np.unique(plain[:, T + 1:], return_counts=True)
        order = vals[np.argsort(-counts)]
        banned = [int(v) for v in order[:3]]
        eos = int(order[3])
        min_new = 5
        out, _, lgs = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, min_new_tokens=min_new, eos_token_id=eos, pad_token_id=1,
                               return_logits=True, suppress_tokens=banned, begin_suppress_tokens=firsts, **flags)
        out = out.numpy()
        static = np.ones((B, vocab), bool)
        static[:, banned] = False
        begin = static.copy()
        begin[:, firsts] = False
        unfinished = np.ones(B, bool)
        for t in range(len(lgs)):
            want = MR.first_argmax(_f32(lgs[t]), begin if t == 0 else static, eos if t < min_new else -1)
            got = out[:, T + t]
            assert (got[unfinished] == want[unfinished]).all() and (got[~unfinished] == 1).all(), t
            unfinished &= got != eos
        gen = out[:, T:]
        assert not np.isin(gen, banned).any() and not np.isin(gen[:, 0], firsts).any() and (gen[:, :min_new] != eos).all()
        assert np.isin(plain[:, T + 1:], banned).any()                            # the lists did change the run
    finally:
        _close(model)


def test_left_padded_batch_and_a_second_turn():
    import torch
    from lia_amd.generation import generate
    model, vocab, flags = _opt()
    try:
        prompt = _prompts(vocab, seed=8)
        mask = np.ones((B, T), np.int64)
        for b in range(B):
            mask[b, :b % 4] = 0
            prompt[b, :b % 4] = 1
        allowed = _sets(vocab, B, SEED + 30)
        seen = []

        def fn(b, row):
            seen.append((b, row.tolist()))
            return np.flatnonzero(allowed[b]).tolist()

        kw = dict(eos_token_id=None, prefix_allowed_tokens_fn=fn, **flags)
        out, _, lgs, state = generate(model, torch.from_numpy(prompt), max_new_tokens=4, attention_mask=torch.from_numpy(mask), return_logits=True,
                                      return_state=True, reserve_tokens=8, **kw)
        out = out.numpy()
        for t in range(4):
            assert (out[:, T + t] == MR.first_argmax(_f32(lgs[t]), allowed)).all(), t
        assert seen[:B] == [(b, prompt[b].tolist()) for b in range(B)]            # the prompt as given, pads included
        unpadded = generate(model, torch.from_numpy(prompt), max_new_tokens=4, **kw).numpy()
        assert (unpadded[:, T:] != out[:, T:]).any()                              # the padding was honoured, not ignored
        del seen[:]
        follow = _prompts(vocab, seed=9)[:, :3]
        allowed2 = _sets(vocab, B, SEED + 31)
        out2, _, lgs2, state2 = generate(model, torch.from_numpy(follow), max_new_tokens=3, past=state, return_logits=True, return_state=True,
                                         eos_token_id=None, prefix_allowed_tokens_fn=lambda b, row: (seen.append(len(row)), np.flatnonzero(allowed2[b]).tolist())[1],
                                         **flags)
        out2 = out2.numpy()
        n = T + 4 + 3
        assert out2.shape == (B, n + 3) and (out2[:, :T + 4] == out).all() and seen == [n] * B + [n + 1] * B + [n + 2] * B
        for t in range(3):
            assert (out2[:, n + t] == MR.first_argmax(_f32(lgs2[t]), allowed2)).all(), t
    finally:
        _close(model)


POOL = {"opt": 32, "llama": 192}          # candidate rows; the Llama's pool was enlarged from 32, where 3 rows survive (the gap stays)
QUANTA = 4


def _kept_rows(lgs, allowed):
    """rows whose top-2 gap among their allowed tokens exceeds QUANTA bf16 quanta of the step's largest logit at every step"""
    keep = np.ones(allowed.shape[0], bool)
    for lg in lgs:
        f = _f32(lg)
        quantum = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(f).max(-1), 1e-30))) - 7)          # parity_util's convention
        f = np.where(allowed, f, -np.inf)
        top2 = np.sort(f, -1)[:, -2:]
        keep &= (top2[:, 1] - top2[:, 0]) > QUANTA * quantum
    return keep


@pytest.mark.parametrize("family", ["opt", "llama"])
def test_speculation_replays_the_plain_constrained_run(family):
    """ReplayDrafter replays the plain constrained run at k = 4, with the greedy verify head and with sampled_verify (the draw rule;
    top_k = 1, where the draw is the row's best allowed token and the keep rule below is the rule that protects it): on every kept
    row the speculative ids are the plain constrained ids, and the block attention counter moved.  A verify pass and a decode step
    round differently, so a row is kept only if the top-2 gap among its allowed tokens exceeds 4 bf16 quanta of the largest logit at
    every compared step.  Survivors, measured on an MI355X: opt 11 of 32; llama 3 of the first 32 -- its vocabulary of 1024 leaves 512
    candidates per row over logits of a few quanta, so its pool is 192 rows, of which 18 survive; at least 8 are required."""
    import torch
    from lia_amd.generation import generate
    from lia_amd.speculative import ReplayDrafter
    model, vocab, flags = MODELS[family]()
    try:
        pool = POOL[family]
        prompt = _prompts(vocab, rows=pool, seed=12)
        allowed = _sets(vocab, pool, SEED + 40)
        fn = _fn(allowed)
        long_new = NEW + 5                                                        # the recording covers the last block's proposal too
        rec, _, lgs = generate(model, torch.from_numpy(prompt), max_new_tokens=long_new, eos_token_id=None, return_logits=True,
                               prefix_allowed_tokens_fn=fn, **flags)
        rec = rec.numpy()
        for t in range(long_new):                                                 # the plain constrained ids are pinned exactly
            assert (rec[:, T + t] == MR.first_argmax(_f32(lgs[t]), allowed)).all()
        keep = _kept_rows(lgs[:NEW], allowed)
        print(f"\n{family}: {int(keep.sum())} of {pool} rows survive the {QUANTA}-quanta rule")
        assert keep.sum() >= 8, f"{family}: only {int(keep.sum())} of {pool} rows survive"
        sched = model._lia_scheduler
        sched.block_attention = True
        inside = np.arange(pool)[:, None]
        for what, kw in (("greedy", {}), ("sampled_verify", dict(do_sample=True, sampled_verify=True, temperature=0.7, top_k=1, top_p=0.9,
                                                                   sample_seed=3))):
            ctx0, n0 = sched.ctx, sched.ctx.block_attention_launches()
            log = []
            out = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, draft=ReplayDrafter(rec), draft_tokens=4,
                           spec_log=log, prefix_allowed_tokens_fn=fn, **kw, **flags).numpy()
            assert (out[keep] == rec[keep, :T + NEW]).all(), (what, np.argwhere(out[keep] != rec[keep, :T + NEW])[:5])
            assert allowed[inside, out[:, T:]].all(), what
            n1 = sched.ctx.block_attention_launches()
            assert (n1 - n0 if sched.ctx is ctx0 else n1) > 0 and len(log) >= 1, what
            assert sched.ctx._token_mask is None
    finally:
        _close(model)


@pytest.mark.parametrize("family", ["opt", "llama"])
def test_sampled_verify_rounds_are_lia_sample_on_substituted_logits(family):
    """sampled_verify at tau 0.7, top-k 50, top-p 0.9 with a drafter that replays the plain sampled constrained run: every verify pass is
    recorded with its (raw) logits and its mask, and every sampled id of every round is lia_sample's (no table) on the round's logits
    with -inf at the disallowed entries and U[generated so far + t, row]; the output is what the rounds kept and stays in the sets"""
    import torch
    from spec_sample_ref import block_uniforms
    from lia_amd import ops, sampling
    from lia_amd.generation import generate
    from lia_amd.speculative import ReplayDrafter
    model, vocab, flags = MODELS[family]()
    try:
        prompt = _prompts(vocab, seed=13)
        allowed = _sets(vocab, B, SEED + 50)
        tau, k, p, sseed = 0.7, 50, 0.9, 17
        skw = dict(do_sample=True, temperature=tau, top_k=k, top_p=p, sample_seed=sseed, eos_token_id=None, prefix_allowed_tokens_fn=_fn(allowed),
                   max_new_tokens=NEW, **flags)
        plain = generate(model, torch.from_numpy(prompt), **skw).numpy()
        sched = model._lia_scheduler
        rounds, ver = [], sched.verify

        def verify(block, kv, **kw):
            res, common = ver(block, kv, **kw, return_logits=True)
            rounds.append((block.clone().numpy(), kw["token_mask"], kw["sampler"].step0, res, common))
            return res, common

        sched.verify = verify
        log = []
        try:
            out = generate(model, torch.from_numpy(prompt), draft=ReplayDrafter(plain), draft_tokens=4, spec_log=log, sampled_verify=True, **skw).numpy()
        finally:
            del sched.verify
        assert len(rounds) == len(log) >= 1 and allowed[np.arange(B)[:, None], out[:, T:]].all()
        U = sampling.draw_uniforms(NEW, B, sseed).cpu().numpy()
        ctx = ops.Context(0, 1 << 20)
        try:
            g = 1
            for block, mask, step0, res, common in rounds:
                Tb = block.shape[1]
                assert step0 == g and tuple(mask.shape) == (B, Tb, MR.words(vocab))
                al = MR.unpack(mask.cpu().numpy(), vocab).reshape(B * Tb, vocab)
                # position t's row is the callable's answer for ids + draft[:t]: the row's set, and every token behind a draft token
                # that the set forbids (nothing there can be kept; the callable is not asked about such a prefix)
                want_al = np.repeat(allowed, Tb, axis=0).reshape(B, Tb, vocab)
                for b in range(B):
                    bad = np.flatnonzero(~allowed[b, block[b, 1:]])
                    if bad.size:
                        want_al[b, bad[0] + 1:] = True
                assert (al == want_al.reshape(B * Tb, vocab)).all()
                sub = MR.substitute(torch, res.logits.view(B * Tb, vocab), al)
                u = torch.from_numpy(block_uniforms(U, step0, B, Tb).reshape(-1)).cuda()
                torch.cuda.synchronize()
                want = ctx.sample(sub, tau, k, p, u)
                ctx.synchronize()
                want = want.cpu().numpy().reshape(B, Tb)
                got = res.greedy.cpu().numpy()
                assert (got == want).all(), (g, np.argwhere(got != want)[:5])
                n_app = min(common + 1, NEW - g)
                assert (out[:, T + g:T + g + n_app] == got[:, :n_app]).all()
                g += n_app
            assert g == NEW
        finally:
            ctx.close()
        same = (out == plain).all(axis=1)
        print(f"\n{family}: sampled speculation equals plain sampling on {int(same.sum())} of {B} rows; commons {[c for c, _ in log]}")
    finally:
        _close(model)
