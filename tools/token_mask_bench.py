"""Cost of an allowed-token table (lia_ctx_set_token_mask) in the head calls, at the two decode shapes of the project: OPT-30B
(B 64, vocab 50272, H 7168) and Llama-3-8B (B 128, vocab 128256, H 4096).  Per shape, with a random-half mask per row and without a
table, alternating, `--rounds` times each:

    lia_lm_head / lia_llama_lm_head   final norm + lm_head GEMM + argmax (the greedy decode head)
    the argmax kernel alone           lia_argmax_launch against lia_argmax_masked_launch on the logits the head wrote
    lia_sample                        (top_k, top_p) = (50, 1), (0, 0.9), (50, 0.9) at tau 0.9

Wall clock per call over `--reps` back-to-back calls that end in a synchronise.  Before anything is timed the masked ids are checked
against the unmasked call on logits with -inf at the disallowed entries (the identity the tests pin) at the timed size.

    python tools/token_mask_bench.py
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/token_mask_bench.py --reps 20 --rounds 1     # kernel times, a run of its own
"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "isca-2025-lia_amd"))

SHAPES = [("opt-30b", "opt", 64, 50272, 7168), ("llama-3-8b", "llama", 128, 128256, 4096)]
SETTINGS = [(50, 1.0), (0, 0.9), (50, 0.9)]
vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long


def per_call_us(fn, ctx, reps):
    fn()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def ab(label, plain, masked, ctx, reps, rounds, table=None):
    """alternate the two, `rounds` times each; print every figure and the medians.  table: set on the context around the masked
    loop (outside the timed window), cleared behind it"""
    a, b = [], []
    for _ in range(rounds):
        a.append(per_call_us(plain, ctx, reps))
        if table is not None:
            ctx.set_token_mask(table)
        b.append(per_call_us(masked, ctx, reps))
        if table is not None:
            ctx.set_token_mask(None)
    ma, mb = sorted(a)[len(a) // 2], sorted(b)[len(b) // 2]
    print(f"{label:58s} no table {ma:8.1f} us  masked {mb:8.1f} us  ({100 * (mb / ma - 1):+5.1f} %)   runs {[round(v, 1) for v in a]} / "
          f"{[round(v, 1) for v in b]}", flush=True)


def main(reps, rounds):
    import torch
    from lia_amd import _native as N, ops
    lib = N.lib()
    lib.lia_argmax_launch.argtypes, lib.lia_argmax_launch.restype = [vp, vp, ci, ci, ci, vp], None
    lib.lia_argmax_masked_launch.argtypes, lib.lia_argmax_masked_launch.restype = [vp, vp, ci, ci, ci, vp, cl, vp], None
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
        W = (V + 31) // 32
        mask = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, W), device="cuda", generator=g, dtype=torch.int64).to(torch.int32)
        logits = torch.empty((B, V), dtype=torch.bfloat16, device="cuda")
        nxt = torch.empty(B, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def lm_head():
            if family == "opt":
                N.check(lib.lia_lm_head(ctx.handle, p(hidden), B, 1, H, p(nw), p(nb), p(head), V, 1e-5, 2, p(logits), p(nxt), st), "lia_lm_head")
            else:
                N.check(lib.lia_llama_lm_head(ctx.handle, p(hidden), B, 1, H, p(nw), p(head), V, 1e-5, 2, p(logits), p(nxt), st), "lia_llama_lm_head")

        # the identity at the timed size, before any timing
        lm_head()
        ctx.synchronize()
        bits = ((mask.view(B, W, 1) >> torch.arange(32, device="cuda").view(1, 1, 32)) & 1).bool().view(B, W * 32)[:, :V]
        sub = logits.clone()
        sub[~bits] = float("-inf")
        torch.cuda.synchronize()
        want = torch.empty_like(nxt)
        lib.lia_argmax_launch(p(sub), p(want), B, V, 2, st)
        ctx.set_token_mask(mask)
        lm_head()
        ctx.set_token_mask(None)
        ctx.synchronize()
        assert torch.equal(nxt, want), f"{name}: the masked head's ids are not the unmasked ids of the substituted logits"
        for k, pp in SETTINGS:
            ctx.set_token_mask(mask)
            got = ctx.sample(logits, 0.9, k, pp, u, suppress_token=2)
            ctx.set_token_mask(None)
            ref = ctx.sample(sub, 0.9, k, pp, u, suppress_token=2)
            ctx.synchronize()
            assert torch.equal(got, ref), f"{name}: masked lia_sample (top_k {k}, top_p {pp}) differs from the substituted draw"
        print(f"{name}: B {B} vocab {V} H {H}; mask {W * 4} bytes per row beside {2 * V} bytes of logits "
              f"({100 * W * 4 / (2 * V):.2f} %); identity checked", flush=True)

        ab(f"{name} lm_head (norm + GEMM + argmax)", lm_head, lm_head, ctx, reps, rounds, table=mask)
        ab(f"{name} argmax kernel alone", lambda: lib.lia_argmax_launch(p(logits), p(nxt), B, V, 2, st),
           lambda: lib.lia_argmax_masked_launch(p(logits), p(nxt), B, V, 2, p(mask), W, st), ctx, reps, rounds)
        for k, pp in SETTINGS:
            smp = lambda: ctx.sample(logits, 0.9, k, pp, u, suppress_token=2)      # noqa: E731
            ab(f"{name} lia_sample top_k {k:2d} top_p {pp:3.1f}", smp, smp, ctx, reps, rounds, table=mask)
        ctx.close()
        del head


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    main(a.reps, a.rounds)
