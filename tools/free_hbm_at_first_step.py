"""Free device memory at the first decode step of the headline configuration (OPT-30B, B 64, 256 in, gpu% 10, prefill 0 / decode 2,
pack10 wire), as bench.py sets it up: one JSON line with torch.cuda.mem_get_info() at decode steps 1, 2 and 3 of the generate behind
the untimed shake-out, the wire cache's capacity and regions and the resident layers' tiers.

    python tools/free_hbm_at_first_step.py [--tree DIR] [--model opt-30b] [--batch-size 64] [--input-len 256] [--gpu-percentage 10]

--tree DIR: import lia_amd from another checkout (an A/B against the parent commit); LIA_RESIDENT_PACKED=0 / LIA_WIRE_CACHE=0 switch
as in any run."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--model", default="opt-30b")
ap.add_argument("--batch-size", type=int, default=64)
ap.add_argument("--input-len", type=int, default=256)
ap.add_argument("--gpu-percentage", type=int, default=10)
a = ap.parse_args()
sys.path.insert(0, os.path.join(a.tree, "isca-2025-lia_amd"))

import torch  # noqa: E402
from lia_amd.generation import generate  # noqa: E402
from lia_amd.model import LiaOPTModel, resolve_shape  # noqa: E402
from lia_amd.scheduler import OffloadScheduler  # noqa: E402

shape = resolve_shape(a.model)
n_gpu = int(shape.layers * a.gpu_percentage / 100)
model = LiaOPTModel.random_init(shape, seed=0, n_gpu_layers=n_gpu, pin_weight=True, wire=10)
sched = model._lia_scheduler = OffloadScheduler(model, wire=10)
row = torch.randint(4, shape.vocab, (a.input_len,), generator=torch.Generator().manual_seed(0), dtype=torch.int64)
ids = row[None, :].repeat(a.batch_size, 1)
flags = dict(prefill_policy=0, decoding_policy=2, pin_weight=True, gpu_percentage=a.gpu_percentage, num_minibatch=1)
kw = dict(do_sample=False, num_beams=1, max_new_tokens=32, min_new_tokens=32, **flags)
generate(model, ids, max_steps=3, **kw)
free = {}


def hook(step):
    if step >= 1:
        torch.cuda.synchronize()
        free[step] = torch.cuda.mem_get_info()[0]


generate(model, ids, max_steps=4, step_hook=hook, **kw)
info = sched.wire_cache_info(regions=True)
print(json.dumps({"tree": a.tree, "free_bytes": free, "total_bytes": torch.cuda.mem_get_info()[1], "capacity": info["capacity"],
                  "regions": info.get("regions"), "residents": [[st.tier, int(st.packed), int(st.stream_bytes)] for st in model.layers[:n_gpu]],
                  "torch_reserved": torch.cuda.memory_reserved(), "torch_allocated": torch.cuda.memory_allocated()}))
sched.close()
model.close()
