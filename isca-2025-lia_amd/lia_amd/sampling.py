"""Sampled decoding for generate(do_sample=True): HF's MinNewTokensLength -> Temperature -> TopK -> TopP -> multinomial, drawn by
the lia_sample kernel (lia_sample.hip) from the logits lm_head wrote ("Sampled decoding").

The randomness of a generation is one block U = torch.rand(max_new_tokens, B_global) drawn when it starts; row r at step t uses
U[t, r].  A row's draw therefore depends only on its logits, the seed, its global row index and the step: minibatching, lm_head's
256-row chunks and data-parallel sharding cannot change any row's sample.
"""
import math

import torch

DEVICE = "cuda"          # where generate() draws U (the lia_sample kernel reads it there)

# HF's resolved defaults (GenerationConfig._get_default_generation_params)
DEFAULT_TEMPERATURE, DEFAULT_TOP_K, DEFAULT_TOP_P = 1.0, 50, 1.0

# HF sampling knobs this build does not implement, with the value that means "off"; generate(do_sample=True) refuses any other
UNSUPPORTED = {"repetition_penalty": 1.0, "min_p": None, "typical_p": 1.0, "epsilon_cutoff": 0.0, "eta_cutoff": 0.0,
               "no_repeat_ngram_size": 0, "num_return_sequences": 1}


def check_settings(temperature, top_k, top_p):
    """(temperature, top_k, top_p) with HF's defaults for None; ValueError names a bad one"""
    temperature = DEFAULT_TEMPERATURE if temperature is None else temperature
    top_k = DEFAULT_TOP_K if top_k is None else top_k
    top_p = DEFAULT_TOP_P if top_p is None else top_p
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not math.isfinite(temperature) or temperature <= 0:
        raise ValueError(f"temperature must be a finite number > 0, got {temperature!r}")
    if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 0:
        raise ValueError(f"top_k must be an int >= 0 (0: off), got {top_k!r}")
    if isinstance(top_p, bool) or not isinstance(top_p, (int, float)) or not (0 < top_p <= 1):
        raise ValueError(f"top_p must be in (0, 1] (1: off), got {top_p!r}")
    return float(temperature), int(top_k), float(top_p)


def check_unsupported(kwargs):
    """ValueError naming the first HF sampling knob of kwargs set to anything but its "off" value"""
    for name, off in UNSUPPORTED.items():
        v = kwargs.get(name)
        if v is None or v == off:
            continue
        raise ValueError(f"{name}={v!r} is not supported with do_sample=True (this build samples with temperature, top_k and "
                         "top_p only)")


def draw_uniforms(max_new_tokens, n_rows, sample_seed=None, device="cuda"):
    """U [max_new_tokens, n_rows] float32 in [0, 1): from a private generator seeded with sample_seed, else from the device's
    default generator (so that torch.manual_seed(s) before generate() reproduces a run, as with HF)"""
    if sample_seed is None:
        return torch.rand((max_new_tokens, n_rows), dtype=torch.float32, device=device)
    g = torch.Generator(device=device)
    g.manual_seed(sample_seed)
    return torch.rand((max_new_tokens, n_rows), dtype=torch.float32, device=device, generator=g)


def shared_seed(dp_group):
    """under data parallelism without a sample_seed: a seed drawn by the root from its default CUDA generator and broadcast,
    once per generate, so that every rank draws the same U"""
    dist = dp_group.dist
    device = "cuda" if dist.get_backend() == "nccl" else "cpu"
    t = torch.zeros(1, dtype=torch.int64, device=device)
    if dp_group.is_root:
        t.copy_(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device="cuda").to(device))
    dist.broadcast(t, src=dp_group.root)
    return int(t.item())


class Sampler:
    """What the schedulers' forward(sampler=) reads: the settings and this step's uniforms `u` (device float32 [B], the
    generation's rows).  `uniforms` is the generation's [max_new_tokens, B] block of this process's rows."""

    def __init__(self, temperature, top_k, top_p, uniforms):
        self.temperature, self.top_k, self.top_p = temperature, top_k, top_p
        self.uniforms = uniforms
        self.u = None

    def at(self, step):
        self.u = self.uniforms[step]
        return self

    def __call__(self, ctx, logits, suppress_token, stream=None):
        """the sampled ids (device int64 [B]) of logits [B, vocab] on ctx's compute stream"""
        return ctx.sample(logits, self.temperature, self.top_k, self.top_p, self.u, suppress_token=suppress_token, stream=stream)
