"""-m gpu: speculative greedy decoding -- generate(draft=, draft_tokens=, spec_log=) -- on test_gpu_multiturn's model (vocab 256,
H 256, L 4) with its discipline: the batch is CHOSEN from a pool by the oracle alone so that no step of the continuation has a
near-tie, and every test asserts that at most one row in eight has one (none has).

Per case: the ids are the oracle's (parity_util.ids_equal_or_near_tie) AND plain generate()'s on the GPU; spec_log is the
ReplayDrafter's script round by round (a generate() that ignored draft= would leave it empty); and the block attention kernel ran
(LIA_CNT_BLOCK_ATTENTION > 0) wherever the block's attention runs on the GPU at all -- with prefill policy 1 and no resident layer
every layer of a multi-token call, attention included, runs on the host cores (scheduler._host_layers): the counter stays 0 there."""

import numpy as np
import pytest

import multiturn_ref as MR
import parity_util
import synth
from test_gpu_generate import FLAG_SETS, cxl_nodes_of_this_box  # noqa: F401  (cxl_nodes_of_this_box: autouse fixture)
from test_gpu_multiturn import B, C, FLAG_FMT, POOL, SEED, T0, W_STD, _assert_few_near_ties, _close, _ids, _opt, choose_rows

pytestmark = pytest.mark.gpu

NEW = 12
RECORD = NEW + 8                # the oracle's continuation is recorded past the run: the last block's proposal is covered too
KS = (1, 4, 7)


def script(k, rounds=NEW, rows=B):
    """per round the scripted right leading tokens per row: round r corrupts row r % rows at token (2 r + 1) % (k + 1) -- k there
    means untouched -- and row (r + 3) % rows one token later; every third round is left whole"""
    out = []
    for r in range(rounds):
        row = [None] * rows
        if r % 3 != 2:
            row[r % rows] = (2 * r + 1) % (k + 1)
            row[(r + 3) % rows] = min((2 * r + 2) % (k + 2), k)
        out.append(row)
    return out


def gpu_attention_runs(flags, L=C["L"]):
    """the block's attention runs on the GPU for some layer: a resident layer, or streamed layers under a prefill policy 0 / 3"""
    return int(L * flags.get("gpu_percentage", 0) / 100) > 0 or flags.get("prefill_policy", 1) != 1


def counter(model):
    """(the scheduler's library context, its block attention launches so far)"""
    ctx = model._lia_scheduler.ctx
    return ctx, ctx.block_attention_launches()


def launches_since(model, before):
    """block attention launches since counter(): a generation that moved to a larger workspace counts in a new context, from 0"""
    ctx, n = counter(model)
    return n - before[1] if ctx is before[0] else n


_ORACLE = {}


def pool_run(oracle, m, flags, append_policy=None):
    """(prompt pool, its oracle continuation, cut): computed once per placement (policies, gpu %), shared by the cases on it"""
    key = (flags.get("prefill_policy", 1), flags.get("decoding_policy", 1), flags.get("gpu_percentage", 0), append_policy)
    if key not in _ORACLE:
        prompt = _ids(1, (POOL, T0))
        _ORACLE[key] = (prompt, cut(oracle_run(oracle, m, prompt, flags, append_policy=append_policy)))
    return _ORACLE[key]


def cut(turns, new=NEW):
    """the continuation's ids whole (what a ReplayDrafter replays), its logits for the `new` steps of the run: the steps that are
    compared, and so the steps the chosen rows must be free of near-ties in"""
    ids, steps = turns[0]
    return [(ids, steps[:new])]


def oracle_run(oracle, m, prompt, flags, new=RECORD, append_policy=None):
    ref = MR.OptRef(oracle, m, C["heads"], prompt.shape[0], C["max_pos"], append_policy=append_policy,
                    **{k: v for k, v in flags.items() if k in ("prefill_policy", "decoding_policy", "gpu_percentage")})
    return MR.converse(ref, prompt, [], (new,))


def run_spec(model, prompt, recording, k, flags, corrupt=None, new=NEW, **kw):
    """-> (ids, spec_log, drafter, target passes)"""
    import torch
    from lia_amd.generation import generate
    from lia_amd.speculative import ReplayDrafter
    d, log = ReplayDrafter(recording, corrupt), []
    out, lat = generate(model, torch.from_numpy(prompt), max_new_tokens=new, eos_token_id=None, token_latency=True, draft=d, draft_tokens=k,
                        spec_log=log, **flags, **kw)
    return out.numpy(), log, d, len(lat)


def check_log(log, drafter, k, rows, passes=None, new=NEW, first_round=0):
    """the log against the drafter's script.  Round r starts with g generated tokens (1 behind the prefill, + common + 1 per round);
    its block position i holds generated token g + i.  The rows are free of near-ties over the `new` tokens of the run only, so a
    count is compared as far as it is decided by those: clipped at new - g, the block positions inside the run"""
    g = 1
    for r, (common, acc) in enumerate(log):
        want = drafter.script(first_round + r, rows, k) if hasattr(drafter, "script") else [k] * rows
        lim = new - g
        assert lim >= 1, (r, g, log)
        assert [min(a, lim) for a in acc] == [min(w, lim) for w in want], (k, r, g, acc, want)
        assert min(common, lim) == min(min(want), lim) and common == min(acc)
        g += common + 1
    assert g >= new > g - log[-1][0] - 1
    if passes is not None:
        assert passes == 1 + len(log) == 1 + drafter.rounds


@pytest.mark.parametrize("flags,fmt", FLAG_FMT, ids=lambda v: v if isinstance(v, str) else ("-".join(f"{k[:4]}{int(x)}" for k, x in v.items()) or "defaults"))
def test_every_flag_set(oracle, flags, fmt, monkeypatch):
    """prompt 9, 12 new tokens, k 1 / 4 / 7 on every flag set, raw and pack10: oracle ids, plain generate()'s ids, the scripted log,
    the block attention counter"""
    import torch
    from lia_amd.generation import generate
    monkeypatch.setenv("LIA_STREAM_FORMAT", fmt)
    m, model = _opt()
    try:
        prompt, pool = pool_run(oracle, m, flags)
        pick, turns = choose_rows(pool)
        prompt = prompt[pick]
        _assert_few_near_ties(f"{flags} {fmt}", turns, B)
        recording, steps = turns[0]
        plain = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, **flags).numpy()
        parity_util.ids_equal_or_near_tie(plain, recording[:, :T0 + NEW], steps, T0, what=f"plain {flags} {fmt}")
        # k = 1 by the measured rule ("measured": two slots take the block kernel at every size), then every k wherever the launch
        # takes the shape (True): 2, 5 and 8 slots through every flag set's minibatches, slabs and wire formats
        for mode, k in [("measured", KS[0])] + [(True, k) for k in KS]:
            model._lia_scheduler.block_attention = mode
            before = counter(model)
            got, log, d, passes = run_spec(model, prompt, recording, k, flags, script(k))
            parity_util.ids_equal_or_near_tie(got, recording[:, :T0 + NEW], steps, T0, what=f"k {k} {mode} {flags} {fmt}")
            assert (got == plain).all(), (k, mode, got.tolist(), plain.tolist())
            check_log(log, d, k, B, passes)
            n = launches_since(model, before)
            assert (n > 0) if gpu_attention_runs(flags) else (n == 0), (flags, k, mode, n)
    finally:
        _close(model)


@pytest.mark.parametrize("flags", [FLAG_SETS[7], FLAG_SETS[8]], ids=["1-1", "0-1"])
def test_batch_one_on_the_online_lines(oracle, flags):
    """B = 1 on the flag sets of the reference's online lines: every accepted token saves a whole pass"""
    import torch
    from lia_amd.generation import generate
    assert flags == {} or (flags["prefill_policy"], flags["decoding_policy"]) == (0, 1)
    m, model = _opt()
    try:
        prompt, pool = pool_run(oracle, m, flags)
        pick, turns = choose_rows(pool, 1)
        prompt = prompt[pick]
        assert len(MR.near_tie_rows(turns)) == 0
        recording, steps = turns[0]
        plain = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, **flags).numpy()
        got, log, d, passes = run_spec(model, prompt, recording, 4, flags, [[2], None, [0], None, None])
        parity_util.ids_equal_or_near_tie(got, recording[:, :T0 + NEW], steps, T0, what=f"B 1 {flags}")
        assert (got == plain).all()
        check_log(log, d, 4, 1, passes)
        assert [c for c, _ in log[:3]] == [2, 4, 0] and passes == 5           # 1 + 3 + 5 + 1 tokens, then the last two
    finally:
        _close(model)


@pytest.mark.parametrize("seed", ["the target's weights", "another seed"])
def test_model_drafter(oracle, seed):
    """ModelDrafter on a second all-resident model: with the target's own weights every round accepts k (its decode steps compute
    what the verify pass computes); with other weights the output is still the greedy output"""
    import torch
    from lia_amd.generation import generate
    from lia_amd.speculative import ModelDrafter
    flags = dict(prefill_policy=3, decoding_policy=3, gpu_percentage=100)
    m, model = _opt()
    _, dmodel = _opt() if seed == "the target's weights" else _opt(77)
    try:
        prompt, pool = pool_run(oracle, m, flags)
        pick, turns = choose_rows(pool)
        prompt = prompt[pick]
        _assert_few_near_ties(seed, turns, B)
        recording, steps = turns[0]
        plain = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, **flags).numpy()
        model._lia_scheduler.block_attention = True          # wherever the launch takes the shape, not only where it was measured to win
        for k in (2, 4):
            d, log = ModelDrafter(dmodel), []
            got, lat = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, token_latency=True, draft=d,
                                draft_tokens=k, spec_log=log, **flags)
            got = got.numpy()
            parity_util.ids_equal_or_near_tie(got, recording[:, :T0 + NEW], steps, T0, what=f"ModelDrafter {seed} k {k}")
            assert (got == plain).all() and len(lat) == 1 + len(log) == 1 + d.rounds and d.prefills == 1
            if seed == "the target's weights":
                check_log(log, d, k, B)
                assert len(log) == -(-(NEW - 1) // (k + 1))
            else:
                assert sum(c for c, _ in log) < k * len(log)
        assert model._lia_scheduler.ctx.block_attention_launches() > 0
    finally:
        _close(model)
        _close(dmodel)


def test_left_padded_batch(oracle):
    """rows of different prompt lengths, left padded, on the 0 / 2 line: every row equals its own unpadded generation through the
    oracle; the block attention kernel takes the row starts"""
    import torch
    from lia_amd.generation import generate
    flags = dict(prefill_policy=0, decoding_policy=2, gpu_percentage=25, pin_weight=True)
    lengths = (9, 1, 5, 9, 3, 7, 2, 9)
    prompt = np.full((B, T0), 1, np.int64)
    mask = np.zeros((B, T0), np.int64)
    m, model = _opt()
    try:
        recording, per_row = np.zeros((B, T0 + RECORD), np.int64), []
        for b, n in enumerate(lengths):
            cand = _ids(50 + b, (32, n))
            pick, t = choose_rows(cut(oracle_run(oracle, m, cand, flags)), 1)
            prompt[b, T0 - n:] = cand[pick[0]]
            mask[b, T0 - n:] = 1
            recording[b, :T0] = prompt[b]
            recording[b, T0:] = t[0][0][0, n:]
            per_row.append(t[0])
        merged = [(None, [np.concatenate([per_row[b][1][s_] for b in range(B)]) for s_ in range(NEW)])]
        _assert_few_near_ties("left padded", merged, B)
        am = torch.from_numpy(mask)
        plain = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, attention_mask=am, **flags).numpy()
        model._lia_scheduler.block_attention = True          # five slots on this small batch: not by the measured rule, so by force
        got, log, d, passes = run_spec(model, prompt, recording, 4, flags, script(4), attention_mask=am)
        assert (got == plain).all()
        for b, n in enumerate(lengths):
            ref_ids, steps = per_row[b]
            parity_util.ids_equal_or_near_tie(got[b:b + 1, T0 - n:], ref_ids[:, :n + NEW], steps, n, what=f"left padded row {b}")
        check_log(log, d, 4, B, passes)
        assert model._lia_scheduler.ctx.block_attention_launches() > 0
    finally:
        _close(model)


def test_append_policy_2(oracle):
    """append_policy = 2 on the 0 / 2 line: the verify blocks' attention runs on the host cores over the host caches (q, k, v travel,
    not the cached prefix); the resident layer still takes the block attention kernel"""
    import torch
    from lia_amd.generation import generate
    flags = dict(prefill_policy=0, decoding_policy=2, gpu_percentage=25, pin_weight=True)
    m, model = _opt()
    try:
        prompt, pool = pool_run(oracle, m, flags, append_policy=2)
        pick, turns = choose_rows(pool)
        prompt = prompt[pick]
        _assert_few_near_ties("append_policy 2", turns, B)
        recording, steps = turns[0]
        plain = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, **flags).numpy()
        model._lia_scheduler.block_attention = True
        got, log, d, passes = run_spec(model, prompt, recording, 4, flags, script(4), append_policy=2)
        parity_util.ids_equal_or_near_tie(got, recording[:, :T0 + NEW], steps, T0, what="append_policy 2")
        assert (got == plain).all()
        check_log(log, d, 4, B, passes)
        assert model._lia_scheduler.ctx.block_attention_launches() > 0
    finally:
        _close(model)


@pytest.mark.parametrize("pct,fmt", [(100, "pack10"), (34, "raw")], ids=["resident", "34 % streamed"])
def test_llama(oracle, pct, fmt):
    """a grouped-query Llama (4 / 1 heads, d 64: G = 4, so T <= 4 fits the 16 slots and k = 4 falls back to the append kernels)"""
    import torch
    from lia_amd.generation import generate
    from lia_amd.llama import LiaLlamaModel, LlamaScheduler, LlamaShape
    H, heads, kvh, F, L, vocab, theta = 256, 4, 1, 512, 3, 256, 10000.0
    m = synth.make_llama_model(3, vocab, H, heads, kvh, F, L, 0.12)
    prompt = _ids(1, (POOL, T0))
    model = LiaLlamaModel.from_numpy(LlamaShape("t", H, heads, kvh, F, L, vocab, max_pos=64, rope_theta=theta), m)
    flags = dict(gpu_percentage=pct, pin_weight=True)
    try:
        model._lia_scheduler = LlamaScheduler(model, pack=fmt)
        model._lia_scheduler.block_attention = True          # (by the measured rule a group of 4 wants >= 512 workgroups)
        ref = MR.LlamaRef(oracle, m, heads, kvh, theta, POOL, T0 + RECORD)
        pick, turns = choose_rows(cut(MR.converse(ref, prompt, [], (RECORD,))))
        prompt = prompt[pick]
        _assert_few_near_ties(f"llama {pct}", turns, B)
        recording, steps = turns[0]
        plain = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, **flags).numpy()
        for k, counted in ((3, True), (4, False)):
            before = counter(model)
            got, log, d, passes = run_spec(model, prompt, recording, k, flags, script(k))
            parity_util.ids_equal_or_near_tie(got, recording[:, :T0 + NEW], steps, T0, what=f"llama {pct} k {k}")
            assert (got == plain).all()
            check_log(log, d, k, B, passes)
            assert (launches_since(model, before) > 0) == counted
    finally:
        _close(model)


def test_llama_model_drafter(oracle):
    """a Llama drafting for a Llama (ModelDrafter's LlamaKVState / LlamaScheduler branch): with the target's own weights every round
    accepts k, and the drafter prefills once"""
    import torch
    from lia_amd.generation import generate
    from lia_amd.llama import LiaLlamaModel, LlamaShape
    from lia_amd.speculative import ModelDrafter
    H, heads, kvh, F, L, vocab, theta = 256, 4, 1, 512, 3, 256, 10000.0
    m = synth.make_llama_model(3, vocab, H, heads, kvh, F, L, 0.12)
    shape = LlamaShape("t", H, heads, kvh, F, L, vocab, max_pos=64, rope_theta=theta)
    model, dmodel = LiaLlamaModel.from_numpy(shape, m), LiaLlamaModel.from_numpy(shape, m)
    flags = dict(gpu_percentage=100, pin_weight=True)
    prompt = _ids(1, (POOL, T0))
    try:
        ref = MR.LlamaRef(oracle, m, heads, kvh, theta, POOL, T0 + RECORD)
        pick, turns = choose_rows(cut(MR.converse(ref, prompt, [], (RECORD,))))
        prompt = prompt[pick]
        _assert_few_near_ties("llama drafter", turns, B)
        recording, steps = turns[0]
        plain = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, **flags).numpy()
        d, log = ModelDrafter(dmodel), []
        got, lat = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, token_latency=True, draft=d, draft_tokens=3,
                            spec_log=log, **flags)
        parity_util.ids_equal_or_near_tie(got.numpy(), recording[:, :T0 + NEW], steps, T0, what="llama drafter")
        assert (got.numpy() == plain).all() and len(lat) == 1 + len(log) == 1 + d.rounds and d.prefills == 1
        check_log(log, d, 3, B)
        assert len(log) == -(-(NEW - 1) // 4)
    finally:
        _close(model)
        _close(dmodel)


def test_a_past_turn(oracle):
    """turn 0 with a drafter and a reserve, then a follow-up turn with one: [pending | follow-up] through an ordinary forward, the
    rounds behind it; both turns the oracle's conversation, the state consistent"""
    import torch
    from lia_amd.generation import generate
    from lia_amd.speculative import ReplayDrafter
    flags = dict(prefill_policy=0, decoding_policy=2, gpu_percentage=50, pin_weight=True, num_minibatch=2)
    new, fu_n, k = (5, 6), 3, 3
    prompt, follow = _ids(1, (POOL, T0)), _ids(2, (POOL, fu_n))
    m, model = _opt()
    try:
        ref = MR.OptRef(oracle, m, C["heads"], POOL, C["max_pos"],
                        **{kk: v for kk, v in flags.items() if kk in ("prefill_policy", "decoding_policy", "gpu_percentage")})
        pick, turns = choose_rows(MR.converse(ref, prompt, [follow], new))
        _assert_few_near_ties("past turn", turns, B)
        # (the recordings end with their turn: the proposals behind them are zeros, check_log compares what lies inside the turn)
        rec0, rec1 = turns[0][0], turns[1][0]
        log = []
        prompt, follow = prompt[pick], follow[pick]
        o1, st = generate(model, torch.from_numpy(prompt), max_new_tokens=new[0], eos_token_id=None, return_state=True,
                          reserve_tokens=fu_n + new[1], draft=ReplayDrafter(rec0, script(k)), draft_tokens=k, spec_log=log, **flags)
        parity_util.ids_equal_or_near_tie(o1.numpy(), turns[0][0], turns[0][1], T0, what="past turn 0")
        assert st.kv.len == o1.shape[1] - 1 and st.kv.smax == T0 + new[0] + fu_n + new[1] + k and len(log) >= 1
        n0 = len(log)
        d = ReplayDrafter(rec1, script(k))
        o2, st2 = generate(model, torch.from_numpy(follow), past=st, max_new_tokens=new[1], eos_token_id=None, return_state=True, draft=d,
                           draft_tokens=k, spec_log=log, **flags)
        n = T0 + new[0] + fu_n
        assert (o2.numpy()[:, :n] == turns[1][0][:, :n]).all()
        parity_util.ids_equal_or_near_tie(o2.numpy(), turns[1][0], turns[1][1], n, what="past turn 1")
        check_log(log[n0:], d, k, B, new=new[1])
        assert st2.kv.len == o2.shape[1] - 1
    finally:
        _close(model)


def test_run_py_draft_model_end_to_end(oracle, tmp_path, capsys):
    """run.py -m <dir> --draft-model <dir of the same weights> --draft-tokens 3: every iteration prints the oracle's continuation,
    every round accepts 3, the summary and --result-json carry the accepted tokens per round"""
    import json
    import torch
    from lia_amd import run_generation
    from test_gpu_configs import _write_hf_checkpoint
    m = synth.make_model(SEED, C["vocab"], C["max_pos"], C["H"], C["F"], C["L"], W_STD)
    for name in ("target", "draft"):
        _write_hf_checkpoint(str(tmp_path / name), m, C, blocked=False)
    flags = dict(prefill_policy=0, decoding_policy=2, gpu_percentage=50)
    cand, pool = pool_run(oracle, m, flags)
    # (run.py suppresses EOS for the whole run -- min_new_tokens = max_new_tokens -- the oracle's loop has no EOS handling: a row without one)
    ties = set(MR.near_tie_rows(pool).tolist())
    r = next(r for r in range(POOL) if r not in ties and (pool[0][0][r, T0:] != 2).all())
    prompt, recording = cand[r], pool[0][0][r:r + 1]
    orig = run_generation.synthetic_prompt
    run_generation.synthetic_prompt = lambda vocab_, n, batch, seed=0: torch.from_numpy(np.tile(prompt[None, :], (batch, 1)))
    out_json = str(tmp_path / "res.json")
    try:
        res = run_generation.main(["--benchmark", "-m", str(tmp_path / "target"), "--draft-model", str(tmp_path / "draft"), "--draft-tokens", "3",
                                   "--input-tokens", str(T0), "--max-new-tokens", str(NEW), "--batch-size", "2", "--token-latency",
                                   "--num-iter", "2", "--num-warmup", "1", "--greedy", "--prefill-policy", "0", "--decoding-policy", "2",
                                   "--gpu-percentage", "50", "--pin-weight", "--result-json", out_json])
    finally:
        run_generation.synthetic_prompt = orig
    text = capsys.readouterr().out
    assert text.count(str(recording[0, T0:T0 + NEW].tolist())) == 2, text[-3000:]
    sp = res["speculative"]
    assert sp["accepted_per_round"] == 3 and sp["rounds"] == 3 and sp["target_passes"] == 3 and sp["decode_tokens_per_s"] > 0
    assert "accepted draft tokens per round: 3.0" in text
    assert json.load(open(out_json))["result"]["speculative"]["accepted_per_round"] == 3
