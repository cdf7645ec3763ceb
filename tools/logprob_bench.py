"""Cost of a log-probability sink (lia_ctx_set_logprob_sink) in the head calls, at the two decode shapes of the project: OPT-30B
(B 64, vocab 50272, H 7168) and Llama-3-8B (B 128, vocab 128256, H 4096).  Per shape, without a sink and with one at N = 0 / 5 / 20,
alternating, `--rounds` times each:

    lia_lm_head / lia_llama_lm_head   final norm + lm_head GEMM + argmax (the greedy decode head), + the top-N kernel behind it
    lia_sample                        top_k 50, top_p 0.9 at tau 0.9, + the top-N kernel behind it
    the kernels alone                 lia_argmax_launch, lia_sample_launch and lia_topn_logprobs_launch (N = 0 / 5 / 20) on the logits the
                                      head wrote: what the sink adds next to the kernel it rides behind

Wall clock per call over `--reps` back-to-back calls that end in a synchronise.  Before anything is timed the sink's rows are checked
against lia_token_logprobs (bit for bit) and the head's ids against the call without a sink, at the timed size.

    python tools/logprob_bench.py
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/logprob_bench.py --reps 20 --rounds 1     # kernel times, a run of its own
"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "isca-2025-lia_amd"))

SHAPES = [("opt-30b", "opt", 64, 50272, 7168), ("llama-3-8b", "llama", 128, 128256, 4096)]
TOPS = (0, 5, 20)
vp, ci, cl, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float


def per_call_us(fn, ctx, reps):
    fn()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def alternate(label, fn, ctx, reps, rounds, sinks):
    """alternate `fn` without a sink and with each of `sinks` (name -> (request, shape) set on the context around the timed loop, or
    name -> callable timed in place of fn), `rounds` times each; print every figure and the medians"""
    runs = {"no sink": []}
    runs.update({k: [] for k in sinks})
    for _ in range(rounds):
        runs["no sink"].append(per_call_us(fn, ctx, reps))
        for k, v in sinks.items():
            if callable(v):
                runs[k].append(per_call_us(v, ctx, reps))
            else:
                ctx.set_logprob_sink(*v)
                try:
                    runs[k].append(per_call_us(fn, ctx, reps))
                finally:
                    ctx.set_logprob_sink(None)
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
    base = med["no sink"]
    cols = "  ".join(f"{k} {med[k]:8.1f} us" + ("" if k == "no sink" else f" ({med[k] - base:+7.1f})") for k in runs)
    print(f"{label:44s} {cols}   runs " + " / ".join(str([round(x, 1) for x in v]) for v in runs.values()), flush=True)


def main(reps, rounds):
    import torch
    from lia_amd import _native as N, ops
    lib = N.lib()
    lib.lia_argmax_launch.argtypes, lib.lia_argmax_launch.restype = [vp, vp, ci, ci, ci, vp], None
    lib.lia_sample_launch.argtypes, lib.lia_sample_launch.restype = [vp, cl, ci, ci, cf, ci, cf, ci, vp, vp, vp, vp], None
    lib.lia_topn_logprobs_launch.argtypes, lib.lia_topn_logprobs_launch.restype = [vp, cl, ci, ci, vp, ci, vp, vp, vp, vp], None
    p = lambda t: ctypes.c_void_p(t.data_ptr())                             # noqa: E731
    for name, family, B, V, H in SHAPES:
        ctx = ops.Context(0, 2 * 256 * H + 8 * B * V * 4 + (1 << 20))
        st = ctypes.c_void_p(ctx.stream)
        g = torch.Generator(device="cuda")
        g.manual_seed(0)
        hidden = (1.5 * torch.randn((B, 1, H), device="cuda", generator=g)).to(torch.bfloat16)
        nw = (1.0 + 0.1 * torch.randn(H, device="cuda", generator=g)).to(torch.bfloat16)
        nb = (0.05 * torch.randn(H, device="cuda", generator=g)).to(torch.bfloat16)
        head = ((2.0 / H ** 0.5) * torch.randn((V, H), device="cuda", generator=g)).to(torch.bfloat16)
        u = torch.rand(B, device="cuda", generator=g)
        logits = torch.empty((B, V), dtype=torch.bfloat16, device="cuda")
        nxt = torch.empty(B, dtype=torch.int64, device="cuda")
        drawn = torch.empty(B, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def lm_head():
            if family == "opt":
                N.check(lib.lia_lm_head(ctx.handle, p(hidden), B, 1, H, p(nw), p(nb), p(head), V, 1e-5, 2, p(logits), p(nxt), st), "lia_lm_head")
            else:
                N.check(lib.lia_llama_lm_head(ctx.handle, p(hidden), B, 1, H, p(nw), p(head), V, 1e-5, 2, p(logits), p(nxt), st), "lia_llama_lm_head")

        def sample():
            N.check(lib.lia_sample(ctx.handle, p(logits), V, B, V, 0.9, 50, 0.9, 2, p(u), p(drawn), None, st), "lia_sample")

        # what the tests pin, at the timed size, before any timing
        lm_head()
        ctx.synchronize()
        ids0, logits0 = nxt.clone(), logits.clone()
        req = ops.LogprobRequest(20)
        ctx.set_logprob_sink(req, (B,))
        lm_head()
        ctx.synchronize()
        assert torch.equal(nxt, ids0) and torch.equal(logits, logits0), f"{name}: the head's outputs changed under a sink"
        same, _ = ctx.token_logprobs(logits, nxt)
        ctx.synchronize()
        assert torch.equal(req.chosen.view(torch.int32), same.view(torch.int32)), f"{name}: chosen is not lia_token_logprobs' value"
        assert (req.top_logprobs[:, :-1] >= req.top_logprobs[:, 1:]).all() and (req.top_ids[:, 0] >= 0).all()
        sample()
        ctx.synchronize()
        same, _ = ctx.token_logprobs(logits, drawn)
        ctx.synchronize()
        assert torch.equal(req.chosen.view(torch.int32), same.view(torch.int32)), f"{name}: chosen does not follow the sampled ids"
        ctx.set_logprob_sink(None)
        print(f"{name}: B {B} vocab {V} H {H}; sink rows checked against lia_token_logprobs", flush=True)

        sinks = {f"N {n}": (ops.LogprobRequest(n), (B,)) for n in TOPS}
        alternate(f"{name} lm_head (norm + GEMM + argmax)", lm_head, ctx, reps, rounds, sinks)
        alternate(f"{name} lia_sample (top_k 50, top_p 0.9)", sample, ctx, reps, rounds, sinks)
        out = ops.LogprobRequest(20).allocate((B,), "cuda")
        torch.cuda.synchronize()
        kernels = {f"top-N kernel N {n}": (lambda n=n: lib.lia_topn_logprobs_launch(p(logits), V, B, V, p(nxt), n, p(out.chosen), p(out.top_ids),
                                                                                    p(out.top_logprobs), st)) for n in TOPS}
        kernels["sampler kernel"] = lambda: lib.lia_sample_launch(p(logits), V, B, V, 0.9, 50, 0.9, 2, p(u), p(drawn), None, st)
        alternate(f"{name} kernels alone (no sink = argmax)", lambda: lib.lia_argmax_launch(p(logits), p(nxt), B, V, 2, st), ctx, reps, rounds,
                  kernels)
        ctx.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    main(a.reps, a.rounds)
