"""Rejection verification, measured: the head's kernel against the sampled verify head's, and the acceptance of the
three drafters on one tiny target / drafter pair.

    python tools/spec_reject_bench.py [--reps 21] [--no-acceptance]

Kernels: lia_verify_reject_launch against lia_verify_sample_launch on the same bf16 logits (sigma 2.5; the draft logits are the
target's + N(0, 0.5^2)) at B 64, T 5, vocab 50272 and B 128, T 3, vocab 128256, tau 0.9 / top-k 50 / top-p 0.95: medians of --reps
launches taken in turn, timed with events on the stream.

Acceptance: the tests' tiny OPT shape (vocab 256, H 256, 4 layers, random weights) as the target, and as the drafter the same
weights with N(0, (noise * w_std)^2) added to every matrix (--noise 0: the target's own weights).  8 rows x 40 tokens, k 4.  Per
setting: the first draft token's acceptance under the rejection rule (a stochastic drafter), under sampled verification with a
coupled and with a greedy drafter, and the mean sum min(p, q) of the rejection rounds' first positions (1 - the head's residual
mass): what the rejection rule reaches in expectation."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "isca-2025-lia_amd"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

SHAPES = [("opt-30b", 64, 5, 50272), ("llama-3-8b", 128, 3, 128256)]
SETTINGS = (0.9, 50, 0.95)
LLAMA_STEP_MS = 7.86          # an all-resident Llama-3-8B decode step at B 128: a verify pass costs at least that


def kernels(reps):
    import torch
    from lia_amd import _native as N
    lib = N.lib()
    vp, ci, cl, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    lib.lia_verify_sample_launch.restype = lib.lia_verify_reject_launch.restype = None
    lib.lia_verify_sample_launch.argtypes = [vp, cl, ci, ci, cf, ci, cf, ci, ci, vp, ci, ci, vp, cl, ci, ci, vp, vp, vp, vp, vp]
    lib.lia_verify_reject_launch.argtypes = [vp, cl, ci, ci, vp, cl, cl, cf, ci, cf, ci, ci, ci, ci, vp, vp, cl, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    tau, k, p = SETTINGS
    for name, B, T, V in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        lg = (2.5 * torch.randn((B * T, V), device="cuda", generator=g)).to(torch.bfloat16)
        dl = (lg.view(B, T, V)[:, :T - 1].float() + 0.5 * torch.randn((B, T - 1, V), device="cuda", generator=g)).to(torch.bfloat16).contiguous()
        U = torch.rand((3, T, B), device="cuda", generator=g)
        blk = torch.randint(0, V, (B, T), device="cuda", generator=g)
        tok = torch.empty((B, T), dtype=torch.int64, device="cuda")
        ok = torch.empty((B, T), dtype=torch.int32, device="cuda")
        f = [torch.empty((B, T), dtype=torch.float32, device="cuda") for _ in range(3)]
        ptr = lambda t: t.data_ptr()                                 # noqa: E731

        def sample():
            lib.lia_verify_sample_launch(ptr(lg), V, B * T, V, tau, k, p, 2, 1, None, T, 0, ptr(U[0]), B, T, 0, None, ptr(blk), ptr(tok), ptr(f[0]), None)

        def reject():
            lib.lia_verify_reject_launch(ptr(lg), V, B * T, V, ptr(dl), (T - 1) * V, V, tau, k, p, 2, 1, T, 0, ptr(U[1]), ptr(U[2]), B, T, 0, ptr(blk),
                                         ptr(tok), ptr(ok), ptr(f[0]), ptr(f[1]), ptr(f[2]), None)

        times = {"sample": [], "reject": []}
        for i in range(reps + 2):
            for what, fn in (("sample", sample), ("reject", reject)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if i >= 2:                                           # the first two rounds warm up
                    times[what].append(1e3 * e0.elapsed_time(e1))
        s, r = statistics.median(times["sample"]), statistics.median(times["reject"])
        line = (f"{name:11s} B {B:3d} T {T} vocab {V:6d}: lia_verify_sample {s:7.1f} us, lia_verify_reject {r:7.1f} us ({r / s:4.2f} x; medians of {reps} "
                f"launches taken in turn; accepted {float(ok[:, :T - 1].float().mean()):.3f}, mean residual mass {float(f[2][:, :T - 1].mean()):.3f})")
        if name.startswith("llama"):
            line += f"; {100 * r / (1e3 * LLAMA_STEP_MS):.1f} % of an all-resident Llama-3-8B decode step of {LLAMA_STEP_MS} ms, the floor of a verify pass"
        print(line, flush=True)


def perturbed(m, noise, w_std, seed):
    """the model's matrices + N(0, (noise * w_std)^2), as bf16 bit patterns again"""
    import numpy as np
    import synth
    rs = np.random.RandomState(seed)

    def one(bits):
        if bits.ndim < 2 or noise == 0:
            return bits
        return synth.f32_to_bf16_bits((synth.bf16_bits_to_f32(bits) + noise * w_std * rs.standard_normal(bits.shape)).astype(np.float32))
    out = {k: one(v) for k, v in m.items() if k != "layers"}
    out["layers"] = [{k: one(v) for k, v in layer.items()} for layer in m["layers"]]
    return out


def acceptance(noises):
    import numpy as np
    import torch
    import synth
    from lia_amd.generation import generate, _scheduler_of
    from lia_amd.model import LiaOPTModel, OPTShape
    from lia_amd.speculative import ModelDrafter
    C, w_std, B, T0, new, k = dict(vocab=256, max_pos=64, H=256, heads=2, F=512, L=4), 0.12, 8, 9, 40, 4
    flags = dict(prefill_policy=3, decoding_policy=3, gpu_percentage=100)
    prompt = torch.from_numpy(np.random.RandomState(1).randint(3, C["vocab"], (B, T0)).astype(np.int64))
    m = synth.make_model(31, C["vocab"], C["max_pos"], C["H"], C["F"], C["L"], w_std)

    def load(weights):
        model = LiaOPTModel.from_numpy(OPTShape("tiny", C["H"], C["heads"], C["F"], C["L"], vocab=C["vocab"], max_pos=C["max_pos"]), weights)
        _scheduler_of(model)
        return model

    target = load(m)
    sched = target._lia_scheduler
    resid, ver = [], sched.verify

    def verify(*a, **kw):
        out = ver(*a, **kw)
        if kw.get("rejector") is not None:
            resid.append(float(out[0].resid_mass[:, 0].mean()))
        return out
    sched.verify = verify
    for noise in noises:
        dmodel = load(perturbed(m, noise, w_std, 7))
        for tau, top_k, top_p in ((1.0, 50, 1.0), (0.9, 50, 0.95), (1.0, 0, 0.9)):
            smp = dict(do_sample=True, temperature=tau, top_k=top_k, top_p=top_p, sample_seed=3, sampled_verify=True)
            shares = {}
            for what, drafter, extra in (("rejection", ModelDrafter(dmodel, stochastic=True), dict(verify_rule="rejection")),
                                         ("coupled", ModelDrafter(dmodel, coupled=True), {}), ("greedy drafter", ModelDrafter(dmodel), {})):
                log = []
                del resid[:]
                generate(target, prompt, max_new_tokens=new, eos_token_id=None, draft=drafter, draft_tokens=k, spec_log=log, **smp, **extra, **flags)
                first = [a >= 1 for _, acc in log for a in acc]
                shares[what] = (sum(first) / len(first), len(first), sum(c for c, _ in log) / len(log), 1 - sum(resid) / len(resid) if resid else None)
            r = shares["rejection"]
            print(f"tiny OPT, drafter = target + {noise:.2f} w_std noise, tau {tau} top-k {top_k} top-p {top_p}, k {k}: first draft token accepted -- "
                  f"rejection {r[0]:.3f} of {r[1]} (round, row) pairs (mean sum min(p, q) {r[3]:.3f}; kept per round {r[2]:.2f}), "
                  + ", ".join(f"{w} {shares[w][0]:.3f} of {shares[w][1]} (kept per round {shares[w][2]:.2f})" for w in ("coupled", "greedy drafter")),
                  flush=True)
        dmodel._lia_scheduler.close()
        dmodel.close()
    sched.close()
    target.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--noise", type=str, default="0,0.25,0.5,1.0", help="drafter weight noise in units of w_std, one pair per value")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-acceptance", action="store_true")
    a = ap.parse_args()
    if not a.no_kernels:
        kernels(a.reps)
    if not a.no_acceptance:
        acceptance([float(v) for v in a.noise.split(",")])
