"""-m gpu: speculative SAMPLED decoding -- generate(do_sample=True, sampled_verify=True, draft=) -- on test_gpu_multiturn's tiny OPT and
a small Llama.

The logits of a verify pass and of a decode step differ in rounding, so plain and speculative sampled ids may part at a draw that
lies at a boundary of the running mass: no test here compares them, except at top_k = 1.  Instead every verify pass
is RECORDED with its logits (the schedulers' return_logits) and pinned against itself: the ids of every round are the reference's
draws from the round's own logits and U[generated so far + t, row], the acceptance is the host recomputation, the output is exactly
what the rounds kept, and spec_log says what the passes returned.

test_coupled_drafter prints its two measured shares (8 rows x 12 tokens, tau 1.0, top-k 4, k 4, seed 11, the target's own weights).
Measured on an MI355X: coupled 1.000 of 24 (round, active row) pairs (every round kept all k tokens, so 3 rounds finish the run; mean
p_draft of the first positions 0.333), uncoupled 0.352 of 88 (mean p_draft 0.417)."""
import numpy as np
import pytest

import synth
from sample_ref import draw_acceptable, sample_ref
from spec_sample_ref import accept, spec_sample_ref
from test_gpu_generate import cxl_nodes_of_this_box  # noqa: F401  (autouse fixture)
from test_gpu_multiturn import B, C, SEED, T0, W_STD, _close, _ids, _opt, choose_rows

pytestmark = pytest.mark.gpu

NEW, TOL = 12, 1e-5
KS = (1, 4, 7)
SAMPLE = dict(do_sample=True, temperature=1.0, top_k=4, top_p=0.9)
COMMON = [("3-3 100", dict(prefill_policy=3, decoding_policy=3, gpu_percentage=100), "raw"),
          ("0-2 25 pinned", dict(prefill_policy=0, decoding_policy=2, gpu_percentage=25, pin_weight=True), "raw"),
          ("0-2 25 pinned", dict(prefill_policy=0, decoding_policy=2, gpu_percentage=25, pin_weight=True), "pack10"),
          ("1-1 0", dict(prefill_policy=1, decoding_policy=1, gpu_percentage=0), "raw")]
ROW_FLAGS = dict(prefill_policy=3, decoding_policy=3, gpu_percentage=25, pin_weight=True)


def script(k, rounds=NEW, rows=B):
    """accept 0 .. k: round r leaves row b (b + r) % (k + 2) tokens right (k + 1: untouched)"""
    return [[(b + r) % (k + 2) for b in range(rows)] for r in range(rounds)]


class Recorder:
    """wraps a scheduler's forward / verify / verify_rows: the sampled route is forced to return its logits, every pass is kept"""

    def __init__(self, sched):
        self.first, self.rounds = [], []
        fwd, ver, rows = sched.forward, sched.verify, getattr(sched, "verify_rows", None)

        def forward(ids, kv, **kw):
            logits, nxt = fwd(ids, kv, **kw)
            self.first.append((logits.float().cpu().numpy(), nxt.cpu().numpy(), kw["sampler"].u.cpu().numpy(), kw.get("suppress_token", -1)))
            return logits, nxt

        def verify(block, kv, **kw):
            assert kw.get("sampler") is not None and "return_logits" not in kw
            res, common = ver(block, kv, **kw, return_logits=True)
            self.rounds.append((block.clone().numpy(), kw, res, common))
            return res, common

        def verify_rows(block, kv, row_lens, **kw):
            assert kw.get("sampler") is not None and "return_logits" not in kw
            res = rows(block, kv, row_lens, **kw, return_logits=True)
            self.rounds.append((block.clone().numpy(), kw, res, None))
            return res

        sched.forward, sched.verify = forward, verify
        if rows is not None:
            sched.verify_rows = verify_rows


def uniforms(new, rows, seed):
    from lia_amd import sampling
    return sampling.draw_uniforms(new, rows, seed).cpu().numpy()


def check_rounds(rec, out, log, passes, U, t0, new=NEW, row_mode=False, eos=None, pad=1, settings=SAMPLE):
    """check 1 of the module docstring.  out: the ids [B, t0 + new...]; t0: the positions in front of the first generated token"""
    tau, k, p = settings["temperature"], settings["top_k"], settings["top_p"]
    rows = out.shape[0]
    # the first forward draws with U[0]
    lg, nxt, u, sup = rec.first[0]
    assert (u == U[0]).all()
    ids, _, keep, margin, cum = sample_ref(lg, tau, k, p, u, sup)
    skipped, total = 0, rows
    for b in range(rows):
        if margin[b] < TOL:
            skipped += 1
        else:
            assert nxt[b] == ids[b] or draw_acceptable(int(nxt[b]), keep[b], cum[b], float(u[b]), TOL), ("first", b, nxt[b], ids[b])
    assert (out[:, t0] == nxt).all()
    g = np.ones(rows, np.int64)
    unf = np.ones(rows, bool) if eos is None else nxt != eos                  # the rows that have not drawn EOS
    assert passes == 1 + len(rec.rounds) and len(log) == len(rec.rounds) >= 1
    for r, ((block, kw, res, common), (lo, acc_log)) in enumerate(zip(rec.rounds, log)):
        view = kw["sampler"]
        T = block.shape[1]
        active = None if kw.get("active") is None else np.asarray(kw["active"]).astype(bool)
        # the rows that still generate are the active ones; the step origin is the number of tokens generated so far
        if row_mode or eos is not None:
            assert active.tolist() == (unf & (g < new)).tolist(), (r, active.tolist(), unf.tolist(), g.tolist())
        assert view.steps().numpy().tolist() == g.tolist(), (r, view.steps().tolist(), g.tolist())
        assert (view.step_rows is not None) == row_mode and view.n_steps == new
        n_sup = kw["n_suppress_rows"] if row_mode else kw.get("n_suppress", 0)
        got, pd = res.greedy.cpu().numpy(), res.p_draft.cpu().numpy()
        ref = spec_sample_ref(res.logits.float().cpu().numpy(), block, tau, k, p, U, g, kw.get("suppress_token", -1), n_sup,
                              None if active is None else active.astype(int))
        for b in range(rows):
            for t in range(T):
                total += 1
                if ref.margin[b, t] < TOL:
                    skipped += 1
                    continue
                assert got[b, t] == ref.sampled[b, t] or draw_acceptable(int(got[b, t]), ref.keep[b, t], ref.cum[b, t], float(ref.u[b, t]), TOL), \
                    (r, b, t, got[b, t], ref.sampled[b, t])
                assert abs(float(pd[b, t]) - ref.p_draft[b, t]) <= 2e-4
        acc, com, nx = accept(block, got, None if active is None else active.astype(int))
        assert (res.accepted.cpu().numpy() == acc).all() and int(res.common.cpu()[0]) == com and (res.next.cpu().numpy() == nx).all()
        # spec_log says what the pass returned
        if row_mode:
            assert acc_log == acc.tolist() and lo == min(a for a, on in zip(acc, active) if on)
        else:
            assert (lo, acc_log) == (com, acc.tolist()) and common == com
        # the output is exactly what the rounds kept: the loops' token-by-token bookkeeping, restated
        if row_mode:
            for b in np.flatnonzero(active):
                for i in range(acc[b] + 1):
                    assert out[b, t0 + g[b]] == got[b, i], (r, b, i)
                    g[b] += 1
                    if eos is not None and got[b, i] == eos:
                        unf[b] = False
                    if not unf[b] or g[b] >= new:
                        break
        else:
            for i in range(com + 1):
                tokens = np.where(unf, got[:, i], pad) if eos is not None else got[:, i]
                assert (out[:, t0 + g[0]] == tokens).all(), (r, i)
                g += 1
                newly = eos is not None and bool((unf & (tokens == eos)).any())
                if eos is not None:
                    unf &= tokens != eos
                if newly or not unf.any() or g[0] >= new:
                    break
    assert len(rec.rounds) == len(log)
    if row_mode:
        assert (~unf | (g == new)).all() and out.shape[1] == t0 + g.max()
        for b in range(rows):
            assert (out[b, t0 + g[b]:] == pad).all()
    else:
        assert out.shape[1] == t0 + g[0] and (g[0] == new or not unf.any())
    assert skipped * 8 <= total, (skipped, total)
    return skipped, total


def run(model, prompt, draft, k, flags, seed, new=NEW, settings=SAMPLE, **kw):
    import torch
    from lia_amd.generation import generate
    rec, log = Recorder(model._lia_scheduler), []
    res = generate(model, torch.from_numpy(prompt), max_new_tokens=new, token_latency=True, draft=draft, draft_tokens=k, spec_log=log,
                   sampled_verify=True, sample_seed=seed, **{"eos_token_id": None, **settings, **flags, **kw})
    return res, log, rec


def fresh(fmt="raw", monkeypatch=None):
    """the tiny OPT with a scheduler of its own (the Recorder patches it, so every case takes a new one)"""
    from lia_amd.generation import _scheduler_of
    if monkeypatch is not None:
        monkeypatch.setenv("LIA_STREAM_FORMAT", fmt)
    m, model = _opt()
    _scheduler_of(model)
    return m, model


def plain_sampled(model, prompt, flags, seed, new=NEW, **kw):
    import torch
    from lia_amd.generation import generate
    return generate(model, torch.from_numpy(prompt), max_new_tokens=new, sample_seed=seed, **{"eos_token_id": None, **SAMPLE, **flags, **kw}).numpy()


@pytest.mark.parametrize("name,flags,fmt", COMMON, ids=[f"{n} {f}" for n, _, f in COMMON])
def test_recorded_rounds_common(name, flags, fmt, monkeypatch):
    from lia_amd.speculative import ReplayDrafter
    prompt = _ids(1, (B, T0))
    _, model = fresh(fmt, monkeypatch)
    try:
        recording = plain_sampled(model, prompt, flags, 5)
    finally:
        _close(model)
    U = uniforms(NEW, B, 5)
    for k in KS:
        _, model = fresh(fmt, monkeypatch)
        try:
            (out, lat), log, rec = run(model, prompt, ReplayDrafter(recording, script(k)), k, flags, 5)
            check_rounds(rec, out.numpy(), log, len(lat), U, T0)
        finally:
            _close(model)


@pytest.mark.parametrize("k", KS)
def test_recorded_rounds_row_mode(k):
    from lia_amd.speculative import ReplayDrafter
    prompt = _ids(1, (B, T0))
    _, model = fresh()
    try:
        recording = plain_sampled(model, prompt, ROW_FLAGS, 6)
    finally:
        _close(model)
    _, model = fresh()
    try:
        (out, lat), log, rec = run(model, prompt, ReplayDrafter(recording, script(k)), k, ROW_FLAGS, 6, acceptance="row")
        check_rounds(rec, out.numpy(), log, len(lat), uniforms(NEW, B, 6), T0, row_mode=True)
        assert len({tuple(a) for _, a in log}) > 1 or k == 1
    finally:
        _close(model)


def test_recorded_rounds_llama():
    from lia_amd.llama import LiaLlamaModel, LlamaScheduler, LlamaShape
    from lia_amd.speculative import ReplayDrafter
    H, heads, kvh, F, L, vocab, theta = 256, 4, 1, 512, 3, 256, 10000.0
    m = synth.make_llama_model(3, vocab, H, heads, kvh, F, L, 0.12)
    prompt = _ids(1, (B, T0))
    flags = dict(gpu_percentage=100, pin_weight=True)

    def llama():
        model = LiaLlamaModel.from_numpy(LlamaShape("t", H, heads, kvh, F, L, vocab, max_pos=64, rope_theta=theta), m)
        model._lia_scheduler = LlamaScheduler(model, pack="raw")
        return model

    model = llama()
    try:
        recording = plain_sampled(model, prompt, flags, 4)
    finally:
        _close(model)
    model = llama()
    try:
        (out, lat), log, rec = run(model, prompt, ReplayDrafter(recording, script(3)), 3, flags, 4)
        check_rounds(rec, out.numpy(), log, len(lat), uniforms(NEW, B, 4), T0)
    finally:
        _close(model)


def test_eos_min_new_tokens_and_pad():
    """a token the rows draw often is made EOS: never before min_new_tokens, only pad behind it; every round still passes check 1,
    with the active rows, the step origins and the kept tokens replayed from the recorded passes and the EOS positions"""
    from lia_amd.speculative import ReplayDrafter
    flags = COMMON[1][1]
    prompt = _ids(1, (B, T0))
    _, model = fresh()
    try:
        free = plain_sampled(model, prompt, flags, 9)
        vals, counts = np.unique(free[:, T0:], return_counts=True)
        eos = int(vals[np.argmax(counts)])
        for mode, fl in (("common", flags), ("row", ROW_FLAGS)):
            _close(model)
            _, model = fresh()
            (out, lat), log, rec = run(model, prompt, ReplayDrafter(free, script(4)), 4, fl, 9, eos_token_id=eos, pad_token_id=1,
                                       min_new_tokens=4, acceptance=mode)
            gen = out.numpy()[:, T0:]
            assert (gen[:, :4] != eos).all(), (mode, eos, gen.tolist())
            print(f"\n{mode}: EOS {eos} drawn on {int((gen == eos).any(axis=1).sum())} of {B} rows")
            for b in range(B):
                hit = np.flatnonzero(gen[b] == eos)
                if hit.size:
                    assert (gen[b, hit[0] + 1:] == 1).all(), (mode, gen[b].tolist())
            assert len(lat) == 1 + len(rec.rounds) == 1 + len(log)
            check_rounds(rec, out.numpy(), log, len(lat), uniforms(NEW, B, 9), T0, row_mode=mode == "row", eos=eos)
            sup = [(kw.get("suppress_token"), kw.get("n_suppress", kw.get("n_suppress_rows"))) for _, kw, _, _ in rec.rounds]
            assert sup[0][0] == eos                           # the first round starts with one generated token: EOS is still suppressed
    finally:
        _close(model)


def test_top_k_one_is_the_greedy_speculative_run(oracle):
    """on rows the oracle finds free of near-ties: sampled verification at top_k = 1 == greedy speculation == plain greedy"""
    import torch
    from lia_amd.generation import generate
    from lia_amd.speculative import ReplayDrafter
    from test_gpu_speculative import pool_run, script as greedy_script
    flags = COMMON[1][1]
    m, model = fresh()
    try:
        prompt, pool = pool_run(oracle, m, flags)
        pick, turns = choose_rows(pool)
        prompt, recording = prompt[pick], turns[0][0]
        plain = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, **flags).numpy()
        for k in (1, 4):
            log_g, log_s = [], []
            greedy = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, draft=ReplayDrafter(recording, greedy_script(k)),
                              draft_tokens=k, spec_log=log_g, **flags).numpy()
            got = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, draft=ReplayDrafter(recording, greedy_script(k)),
                           draft_tokens=k, spec_log=log_s, do_sample=True, top_k=1, temperature=1.3, top_p=0.9, sample_seed=3,
                           sampled_verify=True, **flags).numpy()
            assert (got == greedy).all() and (got == plain).all(), (k, got.tolist(), plain.tolist())
            assert log_s == log_g and len(log_s) >= 1
    finally:
        _close(model)


def test_seeds_reproduce_and_differ():
    from lia_amd.speculative import ReplayDrafter
    flags = COMMON[0][1]
    prompt = _ids(1, (B, T0))
    outs = []
    for seed in (1, 1, 2):
        _, model = fresh()
        try:
            (out, _), _, _ = run(model, prompt, ReplayDrafter(np.zeros((B, T0), np.int64)), 3, flags, seed)
            outs.append(out.numpy())
        finally:
            _close(model)
    assert (outs[0] == outs[1]).all() and (outs[0] != outs[2]).any()


def test_a_past_turn():
    """turn 0 with a reserve, then a follow-up turn: [pending | follow-up] through an ordinary forward that draws with the turn's own
    U[0], the rounds behind it"""
    import torch
    from lia_amd.generation import generate
    from lia_amd.speculative import ReplayDrafter
    flags = COMMON[1][1]
    new, fu_n, k = (5, 6), 3, 3
    prompt, follow = _ids(1, (B, T0)), _ids(2, (B, fu_n))
    _, model = fresh()
    try:
        o1, st = generate(model, torch.from_numpy(prompt), max_new_tokens=new[0], eos_token_id=None, return_state=True, reserve_tokens=fu_n + new[1],
                          draft=ReplayDrafter(prompt), draft_tokens=k, sampled_verify=True, sample_seed=7, **SAMPLE, **flags)
        assert st.kv.len == o1.shape[1] - 1
        (o2, lat, st2), log, rec = run(model, follow, ReplayDrafter(prompt), k, flags, 8, new=new[1], past=st, return_state=True)
        n = T0 + new[0] + fu_n
        assert (o2.numpy()[:, :T0 + new[0]] == o1.numpy()).all() and (o2.numpy()[:, T0 + new[0]:n] == follow).all()
        check_rounds(rec, o2.numpy(), log, len(lat), uniforms(new[1], B, 8), n, new=new[1])
        assert st2.kv.len == o2.shape[1] - 1
    finally:
        _close(model)


def test_left_padded_batch():
    import torch
    from lia_amd.speculative import ReplayDrafter
    flags = COMMON[1][1]
    lengths = (9, 1, 5, 9, 3, 7, 2, 9)
    prompt, mask = np.full((B, T0), 1, np.int64), np.zeros((B, T0), np.int64)
    for b, n in enumerate(lengths):
        prompt[b, T0 - n:] = _ids(50 + b, (n,))
        mask[b, T0 - n:] = 1
    am = torch.from_numpy(mask)
    _, model = fresh()
    try:
        recording = plain_sampled(model, prompt, flags, 12, attention_mask=am)
        _close(model)
        _, model = fresh()
        (out, lat), log, rec = run(model, prompt, ReplayDrafter(recording, script(4)), 4, flags, 12, attention_mask=am)
        check_rounds(rec, out.numpy(), log, len(lat), uniforms(NEW, B, 12), T0)
    finally:
        _close(model)


def first_token_share(coupled, seed=11, k=4):
    """the share of (round, active row) pairs whose first draft token is accepted, with a ModelDrafter of the target's own weights"""
    from lia_amd.speculative import ModelDrafter
    flags = COMMON[0][1]
    settings = dict(do_sample=True, temperature=1.0, top_k=4, top_p=1.0)
    prompt = _ids(1, (B, T0))
    _, model = fresh()
    _, dmodel = _opt()
    try:
        (out, lat), log, rec = run(model, prompt, ModelDrafter(dmodel, coupled=coupled), k, flags, seed, settings=settings)
        check_rounds(rec, out.numpy(), log, len(lat), uniforms(NEW, B, seed), T0, settings=settings)
        pairs = [a >= 1 for _, acc in log for a in acc]                  # (no EOS: every row is active in every round)
        mean_p = float(np.mean([float(res.p_draft[:, 0].mean()) for _, _, res, _ in rec.rounds]))
        return sum(pairs) / len(pairs), len(pairs), mean_p
    finally:
        _close(model)
        _close(dmodel)


def test_coupled_drafter():
    """A drafter that draws with the target's uniforms proposes the target's draw wherever rounding does not move a boundary of the
    running mass across u; one that ignores U cannot exceed the mean top mass in expectation (0.428 for this model and setting on
    the CPU oracle).  0.7 is more than five binomial standard deviations from either.  The uncoupled share is reported, not asserted."""
    share, n, mean_p = first_token_share(True)
    plain_share, plain_n, plain_p = first_token_share(False)
    print(f"\ncoupled: first draft token accepted on {share:.3f} of {n} (round, active row) pairs, mean p_draft {mean_p:.3f}; "
          f"uncoupled: {plain_share:.3f} of {plain_n}, mean p_draft {plain_p:.3f}")
    assert share >= 0.7, (share, n)


def test_run_py_sampled_verify_end_to_end(tmp_path, capsys):
    """run.py -m <dir> --draft-model <dir of the same weights> --do-sample --sampled-verify --draft-coupled: it runs, the record of
    --result-json carries the speculative summary unchanged"""
    import json
    from lia_amd import run_generation
    from test_gpu_configs import _write_hf_checkpoint
    m = synth.make_model(SEED, C["vocab"], C["max_pos"], C["H"], C["F"], C["L"], W_STD)
    for name in ("target", "draft"):
        _write_hf_checkpoint(str(tmp_path / name), m, C, blocked=False)
    out_json = str(tmp_path / "res.json")
    res = run_generation.main(["--benchmark", "-m", str(tmp_path / "target"), "--draft-model", str(tmp_path / "draft"), "--draft-tokens", "3",
                               "--input-tokens", str(T0), "--max-new-tokens", str(NEW), "--batch-size", "2", "--token-latency",
                               "--num-iter", "2", "--num-warmup", "1", "--do-sample", "--temperature", "1.0", "--top-k", "4", "--sample-seed", "3",
                               "--sampled-verify", "--draft-coupled", "--prefill-policy", "0", "--decoding-policy", "2",
                               "--gpu-percentage", "50", "--pin-weight", "--result-json", out_json])
    text = capsys.readouterr().out
    sp = res["speculative"]
    assert sp["rounds"] >= 3 and sp["target_passes"] == sp["rounds"] and sp["decode_tokens_per_s"] > 0 and 0 <= sp["accepted_per_round"] <= 3
    assert "accepted draft tokens per round" in text
    rec = json.load(open(out_json))
    assert rec["status"] == "ok" and rec["result"]["speculative"]["rounds"] == sp["rounds"] and rec["sampling"]["do_sample"] is True
