"""-m gpu: per-row acceptance -- generate(draft=, acceptance="row") -- on test_gpu_speculative's model (vocab 256, H 256, L 4) with its
discipline: the batch is chosen from a pool by the oracle alone so that no compared step has a near-tie, and every test asserts that
at most one row in eight has one.

The KV cache lives in HBM on every layer (policies 3 / 3): all resident, and half the layers streamed raw and pack10.  A ReplayDrafter
script gives the rows DIFFERENT counts in the same round.  Per case: the ids are plain generate()'s on the GPU and the oracle's; the
log's per-row counts are the script's; the number of target passes is what a host-side replay of the script predicts for per-row
lengths -- and strictly smaller than what acceptance="common" needs on the same script, which is what shows that the rows advance
on their own; the block attention counter moved."""
import numpy as np
import pytest

import parity_util
from test_gpu_generate import cxl_nodes_of_this_box  # noqa: F401  (autouse fixture)
from test_gpu_multiturn import B, C, T0, _assert_few_near_ties, _close, _ids, _opt, choose_rows
from spec_rows_util import replay, script
from test_gpu_speculative import NEW, RECORD, counter, cut, launches_since, oracle_run, pool_run

pytestmark = pytest.mark.gpu

KS = (1, 4, 7)
FORMS = [("resident", dict(prefill_policy=3, decoding_policy=3, gpu_percentage=100, pin_weight=True), "raw"),
         ("50 % raw", dict(prefill_policy=3, decoding_policy=3, gpu_percentage=50, pin_weight=True), "raw"),
         ("50 % pack10", dict(prefill_policy=3, decoding_policy=3, gpu_percentage=50, pin_weight=True), "pack10")]


def check_row_log(log, drafter, k, rows, new=NEW):
    """the log against the script, row by row: row b starts round r with g[b] generated tokens; its count is compared as far as the
    `new` tokens of the run decide it (clipped at new - g[b], as test_gpu_speculative.check_log clips); a full row reports k"""
    g = [1] * rows
    for r, (lo, acc) in enumerate(log):
        want = drafter.script(r, rows, k)
        active = [v < new for v in g]
        assert any(active) and len(acc) == rows
        for b in range(rows):
            if active[b]:
                lim = new - g[b]
                assert min(acc[b], lim) == min(want[b], lim), (k, r, b, g, acc, want)
            else:
                assert acc[b] == k
        assert lo == min(a for a, on in zip(acc, active) if on)
        g = [v if v >= new else min(new, v + a + 1) for v, a in zip(g, acc)]
    assert min(g) >= new
    assert len({tuple(a) for _, a in log}) > 1 and any(len(set(a)) > 1 for _, a in log), "the rows never differed"


def run(model, prompt, recording, k, flags, scr, mode, new=NEW, **kw):
    import torch
    from lia_amd.generation import generate
    from lia_amd.speculative import ReplayDrafter
    d, log = ReplayDrafter(recording, scr), []
    out, lat = generate(model, torch.from_numpy(prompt), max_new_tokens=new, eos_token_id=None, token_latency=True, draft=d, draft_tokens=k,
                        spec_log=log, acceptance=mode, **flags, **kw)
    return out.numpy(), log, d, len(lat)


def chosen(oracle, m, flags, what, rows=B):
    prompt, pool = pool_run(oracle, m, flags)
    pick, turns = choose_rows(pool, rows)
    _assert_few_near_ties(what, turns, rows)
    return prompt[pick], turns[0][0], turns[0][1]


@pytest.mark.parametrize("name,flags,fmt", FORMS, ids=[f[0] for f in FORMS])
def test_rows_advance_on_their_own(oracle, name, flags, fmt, monkeypatch):
    import torch
    from lia_amd.generation import generate
    monkeypatch.setenv("LIA_STREAM_FORMAT", fmt)
    m, model = _opt()
    try:
        prompt, recording, steps = chosen(oracle, m, flags, f"rows {name}")
        plain = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, **flags).numpy()
        parity_util.ids_equal_or_near_tie(plain, recording[:, :T0 + NEW], steps, T0, what=f"plain {name}")
        for k in KS:
            scr = script(k)
            before = counter(model)
            got, log, d, passes = run(model, prompt, recording, k, flags, scr, "row")
            n_block = launches_since(model, before)
            parity_util.ids_equal_or_near_tie(got, recording[:, :T0 + NEW], steps, T0, what=f"row mode k {k} {name}")
            assert (got == plain).all(), (k, got.tolist(), plain.tolist())
            check_row_log(log, d, k, B)
            assert passes == 1 + len(log) == 1 + d.rounds == replay(scr, k, B, NEW, "row"), (k, passes, len(log))
            got_c, log_c, _, passes_c = run(model, prompt, recording, k, flags, scr, "common")
            assert (got_c == plain).all() and passes_c == replay(scr, k, B, NEW, "common")
            assert passes < passes_c, f"k {k}: row mode took {passes} target passes, common mode {passes_c}: the rows did not advance on their own"
            assert n_block >= C["L"] * (passes - 1), (k, n_block, passes)          # every layer of every verify pass
    finally:
        _close(model)


def test_minibatches(oracle, monkeypatch):
    """num_minibatch = 2: every streamed layer serves two slices of the row-length table"""
    import torch
    from lia_amd.generation import generate
    flags = dict(FORMS[1][1], num_minibatch=2)
    m, model = _opt()
    try:
        prompt, recording, steps = chosen(oracle, m, flags, "rows minibatches")
        plain = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, **flags).numpy()
        before = counter(model)
        got, log, d, passes = run(model, prompt, recording, 4, flags, script(4), "row")
        parity_util.ids_equal_or_near_tie(got, recording[:, :T0 + NEW], steps, T0, what="row mode minibatches")
        assert (got == plain).all()
        check_row_log(log, d, 4, B)
        assert passes == replay(script(4), 4, B, NEW, "row") < replay(script(4), 4, B, NEW, "common")
        # 2 resident layers serve the batch whole, 2 streamed layers in two slices
        assert launches_since(model, before) == (2 + 2 * 2) * (passes - 1)
    finally:
        _close(model)


def test_left_padded_batch(oracle):
    """mask starts 0, 2 and 5: every row equals plain padded generate() and its own unpadded generation through the oracle"""
    import torch
    from lia_amd.generation import generate
    flags = FORMS[1][1]
    lengths = (9, 7, 4, 9, 7, 4, 9, 7)
    prompt = np.full((B, T0), 1, np.int64)
    mask = np.zeros((B, T0), np.int64)
    m, model = _opt()
    try:
        recording, per_row = np.zeros((B, T0 + RECORD), np.int64), []
        for b, n in enumerate(lengths):
            cand = _ids(70 + b, (32, n))
            pick, t = choose_rows(cut(oracle_run(oracle, m, cand, flags)), 1)
            prompt[b, T0 - n:] = cand[pick[0]]
            mask[b, T0 - n:] = 1
            recording[b, :T0] = prompt[b]
            recording[b, T0:] = t[0][0][0, n:]
            per_row.append(t[0])
        merged = [(None, [np.concatenate([per_row[b][1][s_] for b in range(B)]) for s_ in range(NEW)])]
        _assert_few_near_ties("rows left padded", merged, B)
        am = torch.from_numpy(mask)
        plain = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, attention_mask=am, **flags).numpy()
        got, log, d, passes = run(model, prompt, recording, 4, flags, script(4), "row", attention_mask=am)
        assert (got == plain).all(), (got.tolist(), plain.tolist())
        for b, n in enumerate(lengths):
            ref_ids, steps = per_row[b]
            parity_util.ids_equal_or_near_tie(got[b:b + 1, T0 - n:], ref_ids[:, :n + NEW], steps, n, what=f"rows left padded row {b}")
        check_row_log(log, d, 4, B)
        assert passes == replay(script(4), 4, B, NEW, "row")
    finally:
        _close(model)


@pytest.mark.parametrize("side", ["min_new_tokens below the step", "min_new_tokens above the step"])
def test_eos(oracle, side):
    """eos_token_id = a token one row emits mid-run and no other row ever does: below min_new_tokens it is suppressed (per row and
    block position), from there on the row finishes and is padded; the output is plain generate()'s, pads and length included"""
    import torch
    from lia_amd.generation import generate
    from lia_amd.speculative import ReplayDrafter
    flags = FORMS[0][1]
    m, model = _opt()
    try:
        prompt, recording, steps = chosen(oracle, m, flags, "rows eos")
        gen = recording[:, T0:T0 + NEW]
        picks = [(s, r, int(gen[r, s])) for s in range(2, NEW - 2) for r in range(B)
                 if int(gen[r, s]) != 1 and (gen == gen[r, s]).sum() == 1]
        assert picks, f"no token emitted once by one row only: {gen.tolist()}"
        s, r, tok = picks[-1]                       # the latest such step: the least of the run lies behind a suppressed EOS
        min_new = s if side.endswith("below the step") else s + 2
        kw = dict(max_new_tokens=NEW, min_new_tokens=min_new, eos_token_id=tok, pad_token_id=1, **flags)
        plain = generate(model, torch.from_numpy(prompt), **kw).numpy()
        if min_new <= s:
            assert (plain[r, T0 + s + 1:] == 1).all() and plain[r, T0 + s] == tok and plain.shape[1] == T0 + NEW
        else:
            assert plain[r, T0 + s] != tok
        for k in (2, 5):
            log = []
            got = generate(model, torch.from_numpy(prompt), draft=ReplayDrafter(recording, script(k)), draft_tokens=k, spec_log=log,
                           acceptance="row", **kw).numpy()
            assert got.shape == plain.shape and (got == plain).all(), (side, k, got.tolist(), plain.tolist())
            assert len(log) >= 1
        # every row finishes: the run stops at the longest row's length, as the greedy loop does
        one = torch.from_numpy(prompt[r:r + 1])
        stop = generate(model, one, **{**kw, "min_new_tokens": 0}).numpy()
        got = generate(model, one, draft=ReplayDrafter(recording[r:r + 1]), draft_tokens=3, acceptance="row", **{**kw, "min_new_tokens": 0}).numpy()
        assert stop.shape[1] == T0 + s + 1 and got.shape == stop.shape and (got == stop).all()
    finally:
        _close(model)


@pytest.mark.parametrize("seed", ["the target's weights", "another seed"])
def test_model_drafter_rows(oracle, seed):
    """ModelDrafter.propose_rows (a fresh left-padded generation per round): with the target's own weights every row accepts k in
    every round; with other weights the rows drift apart and the output is still the greedy output"""
    import torch
    from lia_amd.generation import generate
    from lia_amd.speculative import ModelDrafter
    flags = FORMS[0][1]
    m, model = _opt()
    _, dmodel = _opt() if seed == "the target's weights" else _opt(77)
    try:
        prompt, recording, steps = chosen(oracle, m, flags, f"rows drafter {seed}")
        plain = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, **flags).numpy()
        for k in (2, 4):
            d, log = ModelDrafter(dmodel), []
            got, lat = generate(model, torch.from_numpy(prompt), max_new_tokens=NEW, eos_token_id=None, token_latency=True, draft=d,
                                draft_tokens=k, spec_log=log, acceptance="row", **flags)
            got = got.numpy()
            parity_util.ids_equal_or_near_tie(got, recording[:, :T0 + NEW], steps, T0, what=f"rows ModelDrafter {seed} k {k}")
            assert (got == plain).all() and len(lat) == 1 + len(log) == 1 + d.rounds
            if seed == "the target's weights":
                g = 1
                for lo, acc in log:
                    lim = NEW - g
                    assert [min(a, lim) for a in acc] == [min(k, lim)] * B, (k, g, acc)
                    g += k + 1
                assert len(lat) == 1 + -(-(NEW - 1) // (k + 1))
            else:
                assert sum(sum(a) for _, a in log) < k * B * len(log)
    finally:
        _close(model)
        _close(dmodel)
