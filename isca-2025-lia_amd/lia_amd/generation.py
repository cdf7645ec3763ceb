"""generate() + the greedy loop: counterpart of GenerationMixin.generate with the LIA edits
(lia/generation_utils.py:1166-1170, 1542-1558) and IPEX's _greedy_search
(intel_extension_for_pytorch/transformers/generation/greedy_search.py:37-458).

Same call convention as the reference harness uses (llm/single_instance/run_generation.py:179-182,
319-320):

    out = generate(model, input_ids, do_sample=False, num_beams=1, max_new_tokens=N, min_new_tokens=N,
                   prefill_policy=, decoding_policy=, no_overlap=, pin_weight=, gpu_percentage=,
                   num_minibatch=, enable_cxl=, token_latency=True)
    ids, latency_list = out        # (ids only when token_latency is False)

latency_list[i] is the wall clock of greedy iteration i (prepare inputs -> forward -> lm_head -> argmax
-> append), exactly the quantity greedy_search.py:145,424 records: [0] is the prefill, [1:] the decode steps.
"""
import time

import numpy as np
import torch

from . import sampling
from .scheduler import OffloadScheduler

# Two imports stay inside the functions that need them: `.dp` pulls in torch.distributed, which a single-process generation
# never needs; `.llama` is looked up at call time because the CPU tests of the greedy loop replace llama.LlamaKVState.

LIA_KWARGS = ("prefill_policy", "decoding_policy", "no_overlap", "pin_weight", "gpu_percentage", "num_minibatch",
              "enable_cxl")


LLAMA_PADDING_REFUSAL = ("attention_mask with padding (zeros) is not supported for Llama-family models: their RoPE positions "
                         "are not per row yet; pass equal-length prompts")


def left_padding_starts(attention_mask, shape):
    """Validate a left-padded HF attention_mask of input_ids' shape [B, T] and return the per-row starts s_b (int32 [B]: row b
    is s_b zeros, then ones), or None when the mask is absent or all ones -- the unpadded route.  ValueError names the problem."""
    if attention_mask is None:
        return None
    m = attention_mask.detach().cpu().numpy() if isinstance(attention_mask, torch.Tensor) else np.asarray(attention_mask)
    if tuple(m.shape) != tuple(shape):
        raise ValueError(f"attention_mask has shape {tuple(m.shape)}, input_ids {tuple(shape)}: they must match")
    if m.dtype != np.bool_ and not np.isin(m, (0, 1)).all():
        raise ValueError("attention_mask values must be 0 or 1")
    m = m.astype(np.int32)
    if (m.sum(axis=1) == 0).any():
        raise ValueError(f"attention_mask rows {np.flatnonzero(m.sum(axis=1) == 0).tolist()} have no 1 (no token to attend)")
    if (np.diff(m, axis=1) < 0).any():
        raise ValueError("attention_mask must be left padded: a 1 before a 0 in rows "
                         f"{np.flatnonzero((np.diff(m, axis=1) < 0).any(axis=1)).tolist()} (right padding or holes)")
    starts = (m.shape[1] - m.sum(axis=1)).astype(np.int32)
    return None if not starts.any() else starts


def _scheduler_of(model):
    if getattr(model, "_lia_scheduler", None) is None:
        if getattr(model, "family", "opt") == "llama":
            from .llama import LlamaScheduler
            model._lia_scheduler = LlamaScheduler(model)
        else:
            model._lia_scheduler = OffloadScheduler(model)
    return model._lia_scheduler


def generate(model, input_ids, max_new_tokens=None, min_new_tokens=None, do_sample=False, num_beams=1,
             eos_token_id=2, pad_token_id=1, token_latency=False, return_logits=False, temperature=None, top_k=None, top_p=None,
             sample_seed=None, **model_kwargs):
    """do_sample=True: sampled decoding (sampling.py) with HF's temperature / top_k / top_p (defaults 1.0 / 50 / 1.0); U comes from a
    private generator seeded with sample_seed, else from the default CUDA generator.  do_sample=False ignores the three."""
    if num_beams != 1:
        raise ValueError(f"num_beams={num_beams}: beam search is not supported (greedy search and sampling carry the LIA kwargs; "
                         "beam paths are not plumbed in the reference either)")
    if max_new_tokens is None or max_new_tokens < 1:
        raise ValueError("max_new_tokens must be >= 1")
    sample = None
    if do_sample:
        sample = sampling.check_settings(temperature, top_k, top_p)
        sampling.check_unsupported(model_kwargs)
        if sample_seed is not None and (isinstance(sample_seed, bool) or not isinstance(sample_seed, int)):
            raise ValueError(f"sample_seed must be an int or None, got {sample_seed!r}")
        for k in sampling.UNSUPPORTED:
            model_kwargs.pop(k, None)
    # unknown kwargs are NOT rejected: the reference disables that check so its flags reach forward()
    # (lia/generation_utils.py:1166-1170)
    lia = {k: model_kwargs.pop(k, None) for k in LIA_KWARGS}
    attention_mask = model_kwargs.pop("attention_mask", None)
    lia = {"prefill_policy": 1 if lia["prefill_policy"] is None else lia["prefill_policy"],
           "decoding_policy": 1 if lia["decoding_policy"] is None else lia["decoding_policy"],
           "no_overlap": bool(lia["no_overlap"]), "pin_weight": bool(lia["pin_weight"]),
           "gpu_percentage": lia["gpu_percentage"] or 0, "num_minibatch": lia["num_minibatch"] or 1,
           "enable_cxl": bool(lia["enable_cxl"])}
    if model_kwargs.get("cpu_layers"):           # build-defined extension (scheduler.forward): host-computed decode layers
        lia["cpu_layers"] = int(model_kwargs.pop("cpu_layers"))          # -1: chosen online (scheduler.CoopController)
        if model_kwargs.get("cpu_layers_start") is not None:
            lia["cpu_layers_start"] = int(model_kwargs.pop("cpu_layers_start"))
    model_kwargs.pop("cpu_layers_start", None)
    # build-defined, for bench.py: step_hook(i) runs before greedy iteration i (barriers / profiler brackets around exactly the
    # timed steps); max_steps ends the loop early while the caches stay sized for max_new_tokens (a short warm-up call)
    hooks = {"step_hook": model_kwargs.pop("step_hook", None), "max_steps": model_kwargs.pop("max_steps", None)}
    min_new = min_new_tokens or 0
    ids = torch.as_tensor(input_ids, dtype=torch.int64).cpu()
    starts = left_padding_starts(attention_mask, ids.shape) if ids.dim() == 2 else None
    if starts is not None and getattr(model, "family", "opt") == "llama":
        raise ValueError(LLAMA_PADDING_REFUSAL)
    sched = _scheduler_of(model)
    if sample is not None and ids.dim() == 2:
        hooks["sampler"] = _sampler(sched, ids.shape[0], max_new_tokens, sample, sample_seed)
    if starts is None:
        return _greedy_search(model, ids, max_new_tokens, min_new, eos_token_id, pad_token_id, token_latency,
                              return_logits, lia, **hooks)
    # left-padded batch: the scheduler serves every forward of this generation with the row starts; cleared when it ends so
    # that a later unpadded generate() takes the unpadded route
    sched.set_key_starts(starts)
    try:
        return _greedy_search(model, ids, max_new_tokens, min_new, eos_token_id, pad_token_id, token_latency,
                              return_logits, lia, **hooks)
    finally:
        sched.set_key_starts(None)


def _sampler(sched, B, max_new_tokens, settings, sample_seed):
    """the generation's sampling.Sampler: U [max_new_tokens, B_global] drawn once, this process's columns of it.  Under data
    parallelism (the scheduler's DataParallelGroup, whose shard() recorded the global row count) every rank draws the same U --
    from sample_seed, else from a seed the root broadcasts -- and keeps the columns shard_rows gives it."""
    dpg = getattr(sched, "dp", None)
    n_rows = getattr(dpg, "n_rows", None) if dpg is not None else None
    if n_rows is None:
        lo, hi, n_rows = 0, B, B
    else:
        from .dp import shard_rows
        lo, hi = shard_rows(n_rows, dpg.rank, dpg.world)
        if hi - lo != B:
            raise ValueError(f"rank {dpg.rank} holds rows {lo}..{hi} of {n_rows} (DataParallelGroup.shard), generate() got {B}")
        if sample_seed is None:
            sample_seed = sampling.shared_seed(dpg)
    U = sampling.draw_uniforms(max_new_tokens, n_rows, sample_seed, device=sampling.DEVICE)
    U = U[:, lo:hi].contiguous()
    if U.is_cuda:
        torch.cuda.current_stream().synchronize()      # the library's compute stream reads U
    return sampling.Sampler(*settings, U)


def _greedy_search(model, input_ids, max_new_tokens, min_new_tokens, eos_token_id, pad_token_id, token_latency,
                   return_logits, lia, step_hook=None, max_steps=None, sampler=None):
    """the greedy loop of greedy_search.py; with a sampler, the next ids of every step are its draw (sampled decoding) and the
    EOS / pad bookkeeping is the same"""
    sched = _scheduler_of(model)
    ids = torch.as_tensor(input_ids, dtype=torch.int64).cpu()
    if ids.dim() != 2:
        raise ValueError("input_ids must be [batch, seq]")
    B, T = ids.shape
    if T + max_new_tokens > model.shape.max_pos:
        raise ValueError(f"prompt {T} + max_new_tokens {max_new_tokens} exceeds max positions {model.shape.max_pos}")
    if getattr(model, "family", "opt") == "llama":
        from .llama import LlamaKVState
        kv = LlamaKVState(model, B, T + max_new_tokens)
    else:
        kv = sched.new_kv_state(B, T, max_new_tokens, **lia)     # where each layer's cache lives: OffloadScheduler.new_kv_state
    unfinished = torch.ones(B, dtype=torch.int64)
    all_unfinished = True
    latency_list, logits_list = [], []
    # the ids grow in place (greedy_search.py:408 re-allocates [B, T + t] with torch.cat every step: 1 MB per step at
    # B 128 x T 1024, on the critical path between two decode steps)
    ids_buf = torch.empty((B, T + max_new_tokens), dtype=torch.int64)
    ids_buf[:, :T] = ids
    cur = ids
    step = 0
    while True:
        if step_hook is not None:
            step_hook(step)
        tic = time.time()
        # EOS is suppressed while fewer than min_new_tokens were generated (HF MinNewTokensLengthLogitsProcessor)
        suppress = eos_token_id if (eos_token_id is not None and step < min_new_tokens) else -1
        if sampler is None:
            logits, nxt = sched.forward(cur, kv, max_new_tokens=max_new_tokens, suppress_token=suppress, **lia)
        else:
            logits, nxt = sched.forward(cur, kv, max_new_tokens=max_new_tokens, suppress_token=suppress, sampler=sampler.at(step), **lia)
        next_tokens = nxt.cpu()
        same_as_device = eos_token_id is None or all_unfinished        # no row was replaced by the pad token below
        if eos_token_id is not None:
            next_tokens = next_tokens * unfinished + pad_token_id * (1 - unfinished)   # greedy_search.py:398-405
        ids_buf[:, T + step] = next_tokens                                             # :408
        if eos_token_id is not None:
            unfinished = unfinished * (next_tokens != eos_token_id).long()             # :415-421
            all_unfinished = bool(unfinished.min() == 1)
        # the next step's input: the argmax output where it already sits in HBM, unless the EOS bookkeeping changed a row
        cur = nxt.view(B, 1) if (same_as_device and nxt.is_cuda) else next_tokens[:, None]
        step += 1
        if return_logits:
            logits_list.append(logits.clone())
        latency_list.append(time.time() - tic)                                         # :424
        if (eos_token_id is not None and not all_unfinished and unfinished.max() == 0) or step >= max_new_tokens or \
                (max_steps is not None and step >= max_steps):
            break
    out = ids_buf[:, :T + step].clone() if step < max_new_tokens else ids_buf
    if return_logits:
        return out, latency_list, logits_list
    if token_latency:
        return out, latency_list
    return out
