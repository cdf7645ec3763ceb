"""A second turn through generate(past=state) against the only route a build without it has: a fresh generate() over the whole
conversation.  Turn 1 = a prompt of --prompt tokens + --first-new new tokens; turn 2 = --followup tokens + --new new tokens.

    python tools/multiturn_ab.py --config opt30b-resident | llama3-8b-resident | opt30b-headline [--reps 2]

Per route: the first forward (the appended block / the re-prefill of the whole conversation), the decode steps behind it, and the
turn's wall clock, each the median of --reps alternating repetitions (host clock around generate(), which ends in a device
synchronise).  opt30b-headline (prefill 0 / decode 2, gpu% 10, pack10) takes the appended block both ways: append_policy unset (policy
0: the cached prefix crosses the link into the slab) and append_policy=2 (q, k, v of the block go to the host attention)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "isca-2025-lia_amd"))

CONFIGS = {
    "opt30b-resident": dict(model="opt-30b", batch=64, flags=dict(prefill_policy=3, decoding_policy=3, gpu_percentage=100, pin_weight=True)),
    "llama3-8b-resident": dict(model="llama-3-8b", batch=128, flags=dict(gpu_percentage=100, pin_weight=True)),
    "opt30b-headline": dict(model="opt-30b", batch=64, flags=dict(prefill_policy=0, decoding_policy=2, gpu_percentage=10, pin_weight=True)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True, choices=sorted(CONFIGS))
    ap.add_argument("--prompt", type=int, default=256)
    ap.add_argument("--first-new", type=int, default=32)
    ap.add_argument("--followup", type=int, default=32)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    import torch
    from lia_amd.generation import generate
    c = CONFIGS[a.config]
    flags, B = c["flags"], c["batch"]
    if c["model"].startswith("llama"):
        from lia_amd.llama import LiaLlamaModel, LlamaScheduler, resolve_llama_shape
        shape = resolve_llama_shape(c["model"])
        model = LiaLlamaModel.random_init(shape, seed=0, n_gpu_layers=shape.layers)
        model._lia_scheduler = LlamaScheduler(model)
    else:
        from lia_amd.model import LiaOPTModel, resolve_shape
        from lia_amd.scheduler import OffloadScheduler
        shape = resolve_shape(c["model"])
        n_gpu = int(shape.layers * flags["gpu_percentage"] / 100)
        model = LiaOPTModel.random_init(shape, seed=0, n_gpu_layers=n_gpu, pin_weight=True, wire=10 if n_gpu < shape.layers else 0)
        model._lia_scheduler = OffloadScheduler(model, wire="pack10")
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(4, shape.vocab, (B, a.prompt), generator=g)
    follow = torch.randint(4, shape.vocab, (B, a.followup), generator=g)
    kw = dict(eos_token_id=None, token_latency=True, **flags)
    routes = [("past", None)] + ([("past, append_policy=2", 2)] if a.config == "opt30b-headline" else []) + [("fresh generate()", "fresh")]
    times = {name: [] for name, _ in routes}
    conv = None
    for rep in range(a.reps + 1):                       # repetition 0 warms every shape up and is dropped
        for name, how in routes:
            if how == "fresh":
                whole = torch.cat([conv, follow], dim=1)
                t0 = time.time()
                out, lat = generate(model, whole, max_new_tokens=a.new, **kw)
                wall = time.time() - t0
            else:
                conv, _, state = generate(model, prompt, max_new_tokens=a.first_new, return_state=True, reserve_tokens=a.followup + a.new, **kw)
                t0 = time.time()
                out, lat, state = generate(model, follow, past=state, max_new_tokens=a.new, return_state=True, append_policy=how, **kw)
                wall = time.time() - t0
                del state
            if rep:
                times[name].append((1e3 * lat[0], 1e3 * sum(lat[1:]), 1e3 * wall))
    pos0 = a.prompt + a.first_new - 1
    print(f"{a.config}: {c['model']} B {B}, turn 1 = {a.prompt} + {a.first_new} tokens (pos0 {pos0}), turn 2 = {a.followup} + {a.new} new, {flags}, "
          f"median of {a.reps}")
    base = None
    for name, _ in reversed(routes):
        first, dec, wall = (statistics.median(t[i] for t in times[name]) for i in range(3))
        base = wall if base is None else base
        print(f"  {name:26s} first forward {first:9.1f} ms   {a.new - 1} decode steps {dec:9.1f} ms   turn {wall:9.1f} ms   ({base / wall:.2f} x the fresh route)")
    model._lia_scheduler.close()
    model.close()


if __name__ == "__main__":
    main()
