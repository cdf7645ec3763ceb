"""Cost of sampled decoding per decode step: lia_sample against the greedy argmax (lia_argmax_launch) on the same logits, at the two
decode shapes of the issue -- OPT-30B (B 64, vocab 50272) and Llama-3-8B (B 128, vocab 128256) -- for (top_k, top_p) in
(50, 1), (0, 0.9), (50, 0.9); then whole generate() decode steps, greedy and sampled, of an all-resident Llama-3-8B (random weights)
at B 128.

    python tools/sample_bench.py                       # wall-clock per call (synchronised loops)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/sample_bench.py --reps 20     # kernel times, in a run of its own
"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "isca-2025-lia_amd"))

SHAPES = [("opt-30b", 64, 50272), ("llama-3-8b", 128, 128256)]
SETTINGS = [(50, 1.0), (0, 0.9), (50, 0.9)]


def per_call_us(fn, ctx, reps):
    fn()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


def kernels(reps):
    import torch
    from lia_amd import _native as N, ops
    lib = N.lib()
    lib.lia_argmax_launch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.lia_argmax_launch.restype = None
    ctx = ops.Context(0, 0)
    for name, B, V in SHAPES:
        g = torch.Generator(device="cuda")
        g.manual_seed(0)
        lg = (torch.randn((B, V), device="cuda", generator=g) * 3).to(torch.bfloat16)
        u = torch.rand(B, device="cuda", generator=g)
        nxt = torch.empty(B, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        st = ctypes.c_void_p(ctx.stream)
        am = per_call_us(lambda: lib.lia_argmax_launch(ctypes.c_void_p(lg.data_ptr()), ctypes.c_void_p(nxt.data_ptr()), B, V, 2, st), ctx, reps)
        print(f"{name:11s} B {B:3d} vocab {V:6d}  argmax {am:7.1f} us/call", flush=True)
        for k, p in SETTINGS:
            us = per_call_us(lambda: ctx.sample(lg, 0.9, k, p, u, suppress_token=2), ctx, reps)
            print(f"{name:11s} B {B:3d} vocab {V:6d}  sample top_k {k:2d} top_p {p:3.1f}  {us:7.1f} us/call  ({us / am:4.2f} x argmax)",
                  flush=True)
    ctx.close()


def steps(new):
    """greedy and sampled generate() on an all-resident Llama-3-8B at B 128: mean decode-step wall clock"""
    import numpy as np
    import torch
    from lia_amd.generation import generate
    from lia_amd.llama import LLAMA_SHAPES, LiaLlamaModel
    model = LiaLlamaModel.random_init(LLAMA_SHAPES["llama-3-8b"], seed=0)
    ids = torch.from_numpy(np.random.RandomState(0).randint(3, 128256, (128, 32)))
    runs = [("greedy", {})] + [(f"sample top_k {k} top_p {p}", dict(do_sample=True, top_k=k, top_p=p, temperature=0.9, sample_seed=0))
                               for k, p in SETTINGS]
    for label, kw in runs * 2:                                     # two rounds: the first one warms up
        _, lat = generate(model, ids, max_new_tokens=new, min_new_tokens=new, token_latency=True, gpu_percentage=100, pin_weight=True, **kw)
        dec = 1e3 * float(np.mean(lat[1:]))
        if label == "greedy":
            base = dec
        print(f"generate llama-3-8b B 128 {label:28s} decode step {dec:7.3f} ms  (+{dec - base:6.3f} ms vs greedy)", flush=True)
    model._lia_scheduler.close()
    model.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--new", type=int, default=17)
    ap.add_argument("--no-steps", action="store_true")
    a = ap.parse_args()
    kernels(a.reps)
    if not a.no_steps:
        steps(a.new)
