"""Speculative greedy decoding against plain greedy decoding in the same run: what a verify pass of k + 1 tokens costs beside a decode
step, what a draft round of an opt-125m-shaped ModelDrafter costs, and the end-to-end tokens/s at a scripted acceptance.

    python tools/spec_ab.py --config opt30b-online-1-1 | opt30b-online-0-1 | opt30b-headline [--batch 1] [--prompt 256] [--new 32]
                            [--ks 1,2,4,7] [--draft opt-125m | none] [--append-policy 2]

Per k: a ReplayDrafter replays the run's own plain continuation with every row of every round scripted to accept 0, k // 2 and k
tokens, so tokens/s = B (common + 1) / verify pass is measured, not modelled.  A decode step and a verify pass round differently, and
a near-tie of a random-weight model then flips a token: the row leaves its recording and the replayed drafts are wrong from there on.
So the prompts are CHOSEN, as the tests choose theirs: --pool candidate rows are generated plain with their logits, and the B rows
whose smallest top-2 gap over all steps is largest are the run's batch (the gap is printed in bf16 quanta of the row's largest
logit).  Every line still reports whether its acceptance stayed on the script and how many rows differ from the plain run's ids:
only lines that stayed on it are figures of that acceptance.  The draft
round (k decode-shaped steps of the small model, all resident, its own context) is timed apart: a ReplayDrafter costs nothing, so
tokens/s with a real drafter of that acceptance is B (common + 1) / (verify + draft round).  Host clock around the passes (each ends
in a device synchronise); medians.

    python tools/spec_ab.py --config opt30b-kv-hbm --batch 64 --pool 0 --acceptance common,row [--reps 2] [--ks 1,4,7]

--acceptance common,row (KV cache in HBM on every layer, policies 3 / 3): per-row acceptance on a ragged cache beside the one-length
loop, in the same process, the two modes' generations taken in turn --reps times.  The ReplayDrafter draws every row's count
independently per round (uniform on 0 .. k, seeded), the same script for both modes.  Per k and mode: the verify pass (median, and
the min .. max of the generations' medians: the run-to-run spread), the passes, tokens/s; then the accepted counts per round, each
line marked on or off the script (off: some active row's count inside the run differs from its scripted one -- such a line is not
a figure of an acceptance rate).  The ModelDrafter's row-mode round (a fresh left-padded prefill + k - 1 steps) is timed at the end.

    python tools/spec_ab.py --config ... --sampled 1.0,4,1.0 [--coupled] [--acceptance common,row] [--draft opt-125m | none]

--sampled tau,k,p: sampled verification (generate(do_sample=True, sampled_verify=True)) in the same process as the plain sampled run
and the greedy verify, their generations taken in turn --reps times.  Per k and mode: the sampled verify pass beside the greedy
verify pass and a plain sampled decode step (medians, and the min .. max of the generations' medians), tokens/s, the accepted draft
tokens per round beside the mean p_draft of the same rounds' first positions (the expectation of a first token's acceptance), and how
many rows left the plain sampled ids, with the first step at which one did (a verify pass and a decode step round differently: such
rows are still exact samples of the verify pass's distribution).  The ReplayDrafter replays the plain SAMPLED run.  With --draft, a
ModelDrafter of that shape (random weights of its own: real checkpoints are not available here) drafts greedily and, with --coupled,
with the target's uniforms; each line is marked on or off what its drafter would be expected to give only by its p_draft column.
--verify-rule rejection adds, per k in common mode, a stochastic ModelDrafter verified with the rejection rule and one line with the
first-token acceptance of the three drafters side by side, next to the mean sum min(p, q) of the rejection rounds (1 - the head's
residual mass: the acceptance the rule reaches in expectation)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "isca-2025-lia_amd"))

CONFIGS = {     # the lia_online-shaped lines (batch 1, in 256 / out 32) at their gpu %, and the headline flags
    "opt30b-online-1-1": dict(model="opt-30b", flags=dict(prefill_policy=1, decoding_policy=1, gpu_percentage=64, pin_weight=True)),
    "opt30b-online-0-1": dict(model="opt-30b", flags=dict(prefill_policy=0, decoding_policy=1, gpu_percentage=58, pin_weight=True)),
    "opt30b-headline": dict(model="opt-30b", flags=dict(prefill_policy=0, decoding_policy=2, gpu_percentage=10, pin_weight=True)),
    "opt30b-kv-hbm": dict(model="opt-30b", flags=dict(prefill_policy=3, decoding_policy=3, gpu_percentage=10, pin_weight=True)),
    "opt1.3b-resident": dict(model="opt-1.3b", flags=dict(prefill_policy=3, decoding_policy=3, gpu_percentage=100, pin_weight=True)),
}


def build(name, flags):
    from lia_amd.model import LiaOPTModel, resolve_shape
    from lia_amd.scheduler import OffloadScheduler, placement_formats
    shape = resolve_shape(name)
    n_gpu = int(shape.layers * flags["gpu_percentage"] / 100)
    fmt, raw = placement_formats(flags["prefill_policy"], flags["decoding_policy"], 10, n_gpu, shape.layers, True, False, ())
    model = LiaOPTModel.random_init(shape, seed=0, n_gpu_layers=n_gpu, pin_weight=True, wire=fmt, raw_layers=raw)
    model._lia_scheduler = OffloadScheduler(model, wire="pack10")
    return shape, model


def rows_ab(a, model, prompt, rec, plain, step, ks, modes, kw, generate, ReplayDrafter):
    """common and row mode under one script of independent per-row counts, their generations taken in turn"""
    import numpy as np
    B = prompt.shape[0]
    for k in ks:
        rs = np.random.RandomState(k)
        scr = rs.randint(0, k + 1, size=(a.new + 1, B)).tolist()
        runs = {m: [] for m in modes}
        for rep in range(a.reps):
            for m in modes:
                d, log = ReplayDrafter(rec, scr), []
                t0 = time.time()
                out, slat = generate(model, prompt, max_new_tokens=a.new, draft=d, draft_tokens=k, spec_log=log, acceptance=m, **kw)
                runs[m].append((slat, log, out, time.time() - t0))
        for m in modes:
            meds = [statistics.median(sl[1:]) for sl, _, _, _ in runs[m]]
            every = [v for sl, _, _, _ in runs[m] for v in sl[1:]]
            slat, log, out, wall = runs[m][-1]
            differ = int((out != plain).any(dim=1).sum())
            print(f"  k {k} {m:6s}: verify pass {1e3 * statistics.median(every):8.2f} ms (generations' medians {1e3 * min(meds):.2f} .. {1e3 * max(meds):.2f}; "
                  f"{statistics.median(every) / step:5.2f} x a decode step), {len(slat) - 1:3d} passes, {B * (a.new - 1) / sum(slat[1:]):8.2f} tokens/s "
                  f"({step * (a.new - 1) / sum(slat[1:]):5.2f} x plain), wall {wall:6.2f} s, block attention launches "
                  f"{model._lia_scheduler.ctx.block_attention_launches()}, rows differing from plain {differ}", flush=True)
            g = [1] * B
            for r, (lo, acc) in enumerate(log):
                if m == "common":
                    lim = a.new - g[0]
                    on = [min(x, lim) for x in acc] == [min(x, lim) for x in scr[r]]
                    g = [v + lo + 1 for v in g]
                else:
                    on = all(v >= a.new or min(x, a.new - v) == min(w, a.new - v) for v, x, w in zip(g, acc, scr[r]))
                    g = [v if v >= a.new else min(a.new, v + x + 1) for v, x in zip(g, acc)]
                print(f"      round {r:2d} [{'on ' if on else 'OFF'} script] kept {lo if m == 'common' else 'per row'}, accepted per row {acc}", flush=True)


def sampled_ab(a, model, prompt, rec, step, ks, modes, kw, generate, ReplayDrafter, ModelDrafter):
    """--sampled: the plain sampled run, then per k and mode a greedy verify and a sampled verify generation taken in turn"""
    import torch
    tau, top_k, top_p = a.sampled.split(",")
    smp = dict(do_sample=True, temperature=float(tau), top_k=int(top_k), top_p=float(top_p), sample_seed=0)
    B = prompt.shape[0]
    sched = model._lia_scheduler
    generate(model, prompt, max_new_tokens=a.new, max_steps=2, **smp, **kw)
    runs = [generate(model, prompt, max_new_tokens=a.new, **smp, **kw) for _ in range(a.reps)]
    srec = runs[-1][0]
    meds = [statistics.median(lat[1:]) for _, lat in runs]
    sstep = statistics.median([v for _, lat in runs for v in lat[1:]])
    print(f"  plain sampled (tau {tau}, top-k {top_k}, top-p {top_p}): decode step {1e3 * sstep:8.2f} ms (generations' medians "
          f"{1e3 * min(meds):.2f} .. {1e3 * max(meds):.2f}; plain greedy {1e3 * step:.2f}), {B / sstep:8.2f} tokens/s", flush=True)
    seen = []                                          # the p_draft of every sampled verify pass
    ver, ver_rows = sched.verify, sched.verify_rows

    resid = []                                         # the residual mass behind the first position of every rejection verify pass

    def verify(*args, **k2):
        out = ver(*args, **k2)
        if k2.get("sampler") is not None:
            seen.append(out[0].p_draft)
        if k2.get("rejector") is not None:
            resid.append(float(out[0].resid_mass[:, 0].mean()))
        return out

    def verify_rows(*args, **k2):
        out = ver_rows(*args, **k2)
        if k2.get("sampler") is not None:
            seen.append(out.p_draft)
        return out
    sched.verify, sched.verify_rows = verify, verify_rows

    def line(what, k, m, gens, plain_ids):
        every = [v for sl, _, _, _ in gens for v in sl[1:]]
        gm = [statistics.median(sl[1:]) for sl, _, _, _ in gens]
        slat, log, out, pd = gens[-1]
        left = (out != plain_ids).any(dim=1)
        first = int((out != plain_ids).int().argmax(dim=1)[left].min()) - prompt.shape[1] if bool(left.any()) else None
        acc1 = [x >= 1 for _, acc in log for x in acc]
        print(f"  k {k} {m:6s} {what:22s}: verify pass {1e3 * statistics.median(every):8.2f} ms (generations' medians {1e3 * min(gm):.2f} .. "
              f"{1e3 * max(gm):.2f}; {statistics.median(every) / sstep:5.2f} x a sampled step), {len(slat) - 1:3d} passes, "
              f"{B * (a.new - 1) / sum(slat[1:]):8.2f} tokens/s ({sstep * (a.new - 1) / sum(slat[1:]):5.2f} x plain sampled), kept per round "
              f"{[lo for lo, _ in log]}" + (f", first draft token accepted {sum(acc1) / len(acc1):.3f} of {len(acc1)} (round, row) pairs, mean p_draft "
              f"{sum(pd) / len(pd):.3f}" if pd else "") + (f", rows that left the plain ids {int(left.sum())} of {B}"
              + (f" (first at step {first})" if first is not None else "")), flush=True)
        return sum(acc1) / max(len(acc1), 1)

    drafters = [("replay", lambda ids: ReplayDrafter(ids))]
    if a.draft != "none":
        _, dmodel = build(a.draft, ModelDrafter.FLAGS)
        drafters.append((a.draft + " greedy", lambda ids: ModelDrafter(dmodel)))
        if a.coupled:
            drafters.append((a.draft + " coupled", lambda ids: ModelDrafter(dmodel, coupled=True)))
    for k in ks:
        for m in modes:
            extra = {} if m == "common" else {"acceptance": "row"}
            shares = {}
            for name, make in drafters:
                greedy, sampled = [], []
                for rep_ in range(a.reps):
                    if name == "replay":               # the parent route: a greedy verify of the greedy recording, untouched code
                        log = []
                        out, slat = generate(model, prompt, max_new_tokens=a.new, draft=make(rec), draft_tokens=k, spec_log=log, **extra, **kw)
                        greedy.append((slat, log, out, []))
                    log = []
                    del seen[:]
                    out, slat = generate(model, prompt, max_new_tokens=a.new, draft=make(srec), draft_tokens=k, spec_log=log, sampled_verify=True,
                                         **extra, **smp, **kw)
                    sampled.append((slat, log, out, [float(p[:, 0].mean()) for p in seen]))
                if greedy:
                    line("greedy verify, " + name, k, m, greedy, rec[:, :prompt.shape[1] + a.new])
                shares[name.split()[-1]] = line("sampled verify, " + name, k, m, sampled, srec)
            if a.verify_rule == "rejection" and a.draft != "none" and m == "common":
                gens = []
                del resid[:]
                for rep_ in range(a.reps):
                    log = []
                    out, slat = generate(model, prompt, max_new_tokens=a.new, draft=ModelDrafter(dmodel, stochastic=True), draft_tokens=k, spec_log=log,
                                         sampled_verify=True, verify_rule="rejection", **smp, **kw)
                    gens.append((slat, log, out, []))
                shares["rejection"] = line("rejection, " + a.draft + " stochastic", k, m, gens, srec)
                print(f"  k {k} first draft token accepted: rejection {shares['rejection']:.3f} (mean sum min(p, q) of the same rounds' first positions "
                      f"{1 - sum(resid) / len(resid):.3f}), coupled {shares.get('coupled', float('nan')):.3f}, greedy drafter "
                      f"{shares.get('greedy', float('nan')):.3f}", flush=True)
    sched.verify, sched.verify_rows = ver, ver_rows
    if a.draft != "none":
        dmodel._lia_scheduler.close()
        dmodel.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True, choices=sorted(CONFIGS))
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--prompt", type=int, default=256)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--ks", type=str, default="1,2,4,7")
    ap.add_argument("--draft", type=str, default="opt-125m")
    ap.add_argument("--append-policy", type=int, default=None)
    ap.add_argument("--acceptance", type=str, default="common", help="common | row | common,row (row: policies 3 / 3 only)")
    ap.add_argument("--reps", type=int, default=2, help="with --acceptance common,row: generations per k and mode, taken in turn")
    ap.add_argument("--pool", type=int, default=16, help="candidate prompts the batch is chosen from (0: take the first --batch)")
    ap.add_argument("--sampled", type=str, default=None, help="tau,top_k,top_p: sampled verification beside plain sampling and the greedy verify")
    ap.add_argument("--coupled", action="store_true", help="with --sampled and --draft: also a ModelDrafter that draws with the target's uniforms")
    ap.add_argument("--verify-rule", type=str, default="draw", choices=["draw", "rejection"],
                    help="with --sampled and --draft: rejection = also a stochastic ModelDrafter verified with the rejection rule (common mode), "
                         "its first-token acceptance beside the coupled and the greedy drafter's and the mean sum min(p, q)")
    a = ap.parse_args()
    if a.coupled and not a.sampled:
        ap.error("--coupled needs --sampled")
    if a.verify_rule != "draw" and not a.sampled:
        ap.error("--verify-rule rejection needs --sampled")
    import torch
    from lia_amd.generation import generate
    from lia_amd.speculative import ModelDrafter, ReplayDrafter
    c = CONFIGS[a.config]
    flags, B, ks = c["flags"], a.batch, [int(v) for v in a.ks.split(",")]
    shape, model = build(c["model"], flags)
    g = torch.Generator().manual_seed(0)
    kw = dict(eos_token_id=None, token_latency=True, **flags)
    print(f"{a.config}: {c['model']} B {B}, in {a.prompt} / out {a.new}, {flags}, append_policy {a.append_policy}", flush=True)
    prompt = torch.randint(4, shape.vocab, (max(B, a.pool), a.prompt), generator=g)
    if a.pool > B:
        _, _, steps = generate(model, prompt, max_new_tokens=a.new + max(ks) + 1, return_logits=True, **kw)
        gaps = []
        for lg in steps:
            f = lg.float()
            top2 = f.topk(2, dim=-1).values
            q = torch.exp2(torch.floor(torch.log2(f.abs().amax(dim=-1).clamp_min(1e-30))) - 7)
            gaps.append(((top2[:, 0] - top2[:, 1]) / q).cpu())
        worst = torch.stack(gaps).amin(dim=0)
        pick = worst.argsort(descending=True)[:B]
        print(f"  rows {pick.tolist()} of {a.pool} candidates: smallest top-2 gap over {len(steps)} steps {[round(float(worst[i]), 1) for i in pick]} "
              f"bf16 quanta (pool median {float(worst.median()):.1f})", flush=True)
        prompt = prompt[pick]
        del steps
    prompt = prompt[:B].contiguous()
    generate(model, prompt, max_new_tokens=a.new + max(ks) + 1, max_steps=2, **kw)             # warm-up: placement, allocations
    rec, lat = generate(model, prompt, max_new_tokens=a.new + max(ks) + 1, **kw)                # the recording, and the plain figures
    plain = rec[:, :a.prompt + a.new]
    step = statistics.median(lat[1:])
    print(f"  plain greedy: prefill {1e3 * lat[0]:9.1f} ms, decode step {1e3 * step:8.2f} ms (median of {len(lat) - 1}), {B / step:8.2f} tokens/s", flush=True)
    modes = a.acceptance.split(",")
    if a.sampled:
        sampled_ab(a, model, prompt, rec, step, ks, modes, kw, generate, ReplayDrafter, ModelDrafter)
        model._lia_scheduler.close()
        model.close()
        return
    if modes != ["common"]:
        rows_ab(a, model, prompt, rec, plain, step, ks, modes, kw, generate, ReplayDrafter)
        if a.draft != "none":
            _, dmodel = build(a.draft, ModelDrafter.FLAGS)
            d = ModelDrafter(dmodel)
            for k in ks:
                rows = [rec[b, :a.prompt + 1 + (3 * b) % (a.new - 1)] for b in range(B)]        # lengths spread over the run
                times = []
                for r in range(4):
                    t0 = time.time()
                    d.propose_rows(rows, k, (-1, None))
                    times.append(time.time() - t0)
                print(f"  {a.draft} row-mode draft round (left-padded prefill of {max(len(r) for r in rows)} + {k - 1} steps), k {k}: "
                      f"{1e3 * statistics.median(times[1:]):8.2f} ms (median of 3, B {B})", flush=True)
            dmodel._lia_scheduler.close()
            dmodel.close()
        model._lia_scheduler.close()
        model.close()
        return
    for k in ks:
        for acc in sorted({0, k // 2, k}):
            d, log = ReplayDrafter(rec, [[acc] * B] * (a.new + 1)), []
            t0 = time.time()
            out, slat = generate(model, prompt, max_new_tokens=a.new, draft=d, draft_tokens=k, spec_log=log, append_policy=a.append_policy, **kw)
            wall = time.time() - t0
            vp = statistics.median(slat[1:])
            differ = int((out != plain).any(dim=1).sum())
            scripted = all(cm == acc for cm, _ in log[:-1]) and differ == 0
            print(f"  k {k} accept {acc}: verify pass {1e3 * vp:8.2f} ms ({vp / step:5.2f} x a decode step), {len(slat) - 1:3d} passes, "
                  f"{B * (a.new - 1) / sum(slat[1:]):8.2f} tokens/s ({step * (a.new - 1) / sum(slat[1:]):5.2f} x plain), wall {wall:6.2f} s, "
                  f"block attention launches {model._lia_scheduler.ctx.block_attention_launches()}, rows differing from plain {differ}"
                  f"{'' if scripted else '   (OFF THE SCRIPT, acceptance per round: ' + str([cm for cm, _ in log]) + ')'}", flush=True)
    if a.draft != "none":
        _, dmodel = build(a.draft, ModelDrafter.FLAGS)
        d = ModelDrafter(dmodel)
        for k in ks:
            ids = rec[:, :a.prompt + 1]
            out = d.propose(ids, k)                                   # its prefill (or its rollback to the prompt)
            p0, times = d.prefills, []
            for r in range(5):       # rounds behind a fully accepted one (its own proposal + one token): two tokens fed, then k - 1 steps
                ids = torch.cat([ids, out, rec[:, :1]], dim=1)
                t0 = time.time()
                out = d.propose(ids, k)
                times.append(time.time() - t0)
            assert d.prefills == p0, "the drafter prefilled again: its rollback did not find the common prefix"
            print(f"  {a.draft} draft round, k {k}: {1e3 * statistics.median(times[1:]):8.2f} ms (median of 4, B {B}, context {ids.shape[1]})", flush=True)
        dmodel._lia_scheduler.close()
        dmodel.close()
    model._lia_scheduler.close()
    model.close()


if __name__ == "__main__":
    main()
