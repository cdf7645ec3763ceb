"""Cost of the repetition / presence / frequency penalties (lia_penalty.hip, lia_ctx_set_penalties) at the two decode shapes of the
project: OPT-30B (B 64, vocab 50272, H 7168) and Llama-3-8B (B 128, vocab 128256, H 4096).  In one process, per shape:

    penalty kernel        lia_apply_penalties, logits -> scratch under a table; its traffic is 6 bytes per (row, token): 2 + 2 read, 2
                          written.  Back-to-back calls on the same buffers: the 19 / 98 MB working set is what the head's GEMM just
                          wrote, so a share of it is served from the caches, as in a decode step
    count update          lia_token_counts_add of one generated token per row (what a decode step adds)
    prompt count          lia_token_counts_add of T = 256 prompt tokens per row (once per generate())
    head calls            lia_lm_head / lia_llama_lm_head and that call followed by lia_sample (top_k 50, top_p 0.9, tau 0.9), without and
                          with a table, alternating, `--rounds` times each

Wall clock per call over `--reps` back-to-back calls that end in a synchronise.  Before anything is timed the penalised head's ids
are checked against the plain head on the rewritten logits, at the timed size.

    python tools/penalty_bench.py
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/penalty_bench.py --reps 20 --rounds 1     # kernel times, a run of its own
"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "isca-2025-lia_amd"))

SHAPES = [("opt-30b", "opt", 64, 50272, 7168), ("llama-3-8b", "llama", 128, 128256, 4096)]
SETTINGS = (1.2, 0.5, 0.25)
PROMPT_T = 256


def per_call_us(fn, ctx, reps):
    fn()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def median_of(fn, ctx, reps, rounds):
    runs = [per_call_us(fn, ctx, reps) for _ in range(rounds)]
    return sorted(runs)[len(runs) // 2], runs


def main(reps, rounds):
    import torch
    from lia_amd import _native as N, ops
    lib = N.lib()
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
        prompt = torch.randint(0, V, (B, PROMPT_T), device="cuda", generator=g)
        logits = torch.empty((B, V), dtype=torch.bfloat16, device="cuda")
        nxt = torch.empty(B, dtype=torch.int64, device="cuda")
        drawn = torch.empty(B, dtype=torch.int64, device="cuda")
        counts = torch.zeros((B, V), dtype=torch.int16, device="cuda")
        scratch = torch.empty((B, V), dtype=torch.bfloat16, device="cuda")
        torch.cuda.synchronize()

        def lm_head():
            if family == "opt":
                N.check(lib.lia_lm_head(ctx.handle, p(hidden), B, 1, H, p(nw), p(nb), p(head), V, 1e-5, 2, p(logits), p(nxt), st), "lia_lm_head")
            else:
                N.check(lib.lia_llama_lm_head(ctx.handle, p(hidden), B, 1, H, p(nw), p(head), V, 1e-5, 2, p(logits), p(nxt), st), "lia_llama_lm_head")

        def head_and_sample():
            lm_head()
            N.check(lib.lia_sample(ctx.handle, p(logits), V, B, V, 0.9, 50, 0.9, 2, p(u), p(drawn), None, st), "lia_sample")

        def kernel():
            N.check(lib.lia_apply_penalties(ctx.handle, p(logits), V, B, V, p(counts), V, *SETTINGS, p(scratch), V, st), "lia_apply_penalties")

        def step_update():
            N.check(lib.lia_token_counts_add(ctx.handle, p(counts), V, B, V, p(nxt), 1, 1, None, None, 1, st), "lia_token_counts_add")

        def prompt_count():
            N.check(lib.lia_token_counts_add(ctx.handle, p(counts), V, B, V, p(prompt), PROMPT_T, PROMPT_T, None, None, 0, st), "lia_token_counts_add")

        # a table a generation would hold: the prompt, and the plain head's own winner generated twice -- then what the tests pin
        prompt_count()
        lm_head()
        step_update()
        step_update()
        ctx.synchronize()
        ids0, logits0 = nxt.clone(), logits.clone()
        rewritten = ctx.apply_penalties(logits0, counts, *SETTINGS)
        ctx.synchronize()
        want = torch.empty(B, dtype=torch.int64, device="cuda")
        lib_argmax = lib.lia_argmax_launch
        lib_argmax.argtypes, lib_argmax.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], None
        torch.cuda.synchronize()
        lib_argmax(p(rewritten), p(want), B, V, 2, st)
        ctx.synchronize()
        ctx.set_penalties(counts, *SETTINGS, scratch=scratch)
        lm_head()
        ctx.synchronize()
        ctx.set_penalties(None)
        assert torch.equal(logits, logits0), f"{name}: the head's logits changed under penalties"
        assert torch.equal(nxt, want), f"{name}: the penalised ids are not the plain argmax of the rewritten logits"
        changed = int((nxt != ids0).sum())
        nxt.copy_(ids0)
        torch.cuda.synchronize()
        print(f"{name}: B {B} vocab {V} H {H}; penalised ids checked against the argmax of the rewritten logits ({changed} of {B} rows changed)",
              flush=True)

        med, runs = median_of(kernel, ctx, reps, rounds)
        mb = 6 * B * V / 1e6
        print(f"{name} penalty kernel            {med:8.1f} us   {mb:6.1f} MB -> {mb / med * 1e3:7.1f} GB/s   runs {[round(x, 1) for x in runs]}", flush=True)
        med, runs = median_of(step_update, ctx, reps, rounds)
        print(f"{name} count update (1 / row)    {med:8.1f} us   runs {[round(x, 1) for x in runs]}", flush=True)
        med, runs = median_of(prompt_count, ctx, reps, rounds)
        print(f"{name} prompt count (T {PROMPT_T})     {med:8.1f} us   runs {[round(x, 1) for x in runs]}", flush=True)
        for label, fn in (("lm_head (norm + GEMM + argmax)", lm_head), ("lm_head + lia_sample", head_and_sample)):
            plain, with_table = [], []
            for _ in range(rounds):
                plain.append(per_call_us(fn, ctx, reps))
                ctx.set_penalties(counts, *SETTINGS, scratch=scratch)
                try:
                    with_table.append(per_call_us(fn, ctx, reps))
                finally:
                    ctx.set_penalties(None)
            a, b = sorted(plain)[rounds // 2], sorted(with_table)[rounds // 2]
            print(f"{name} {label:32s} no table {a:8.1f} us   table {b:8.1f} us ({b - a:+7.1f})   runs {[round(x, 1) for x in plain]} / "
                  f"{[round(x, 1) for x in with_table]}", flush=True)
        ctx.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    main(a.reps, a.rounds)
