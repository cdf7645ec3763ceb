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
# (repetition_penalty is generate()'s own keyword: penalties.py)
UNSUPPORTED = {"min_p": None, "typical_p": 1.0, "epsilon_cutoff": 0.0, "eta_cutoff": 0.0,
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

    def at_rows(self, steps):
        """a Sampler of the same settings whose u[b] = U[steps[b], b], 0 where steps[b] is past the table: row b at ITS step (a
        coupled drafter's draft step, row mode).  self is not touched."""
        n, B = self.uniforms.shape
        steps = torch.as_tensor(steps, dtype=torch.int64).to(self.uniforms.device)
        if steps.dim() == 0:
            steps = steps.expand(B)
        u = self.uniforms[steps.clamp(0, n - 1), torch.arange(B, device=self.uniforms.device)]
        out = Sampler(self.temperature, self.top_k, self.top_p, self.uniforms)
        out.u = torch.where((steps >= 0) & (steps < n), u, torch.zeros_like(u)).contiguous()
        if out.u.is_cuda:
            torch.cuda.current_stream().synchronize()      # the library's compute stream reads u
        return out

    def block(self, step0):
        """what a sampled verify pass reads (speculative decoding): every row has generated step0 tokens, block
        position t of row b draws with U[step0 + t, b]"""
        return SamplerBlock(self, int(step0), None)

    def block_rows(self, steps):
        """block() with one origin per row (row mode): block position t of row b draws with U[steps[b] + t, b]"""
        return SamplerBlock(self, 0, torch.as_tensor(steps, dtype=torch.int32).contiguous())

    def __call__(self, ctx, logits, suppress_token, stream=None):
        """the sampled ids (device int64 [B]) of logits [B, vocab] on ctx's compute stream"""
        return ctx.sample(logits, self.temperature, self.top_k, self.top_p, self.u, suppress_token=suppress_token, stream=stream)


class SamplerBlock:
    """A view of a generation's Sampler for one verify round: the settings, the table (`uniforms` [n_steps, ldu]; row b is column
    b), and the step origin -- step0 for every row, or step_rows (int32 [B], CPU).  A position whose step is >= n_steps draws with
    u = 0 and reads nothing: it can never be kept."""

    def __init__(self, sampler, step0, step_rows):
        self.sampler, self.step0, self.step_rows = sampler, step0, step_rows
        self.temperature, self.top_k, self.top_p = sampler.temperature, sampler.top_k, sampler.top_p
        self.uniforms = sampler.uniforms
        self.n_steps, self.ldu = int(sampler.uniforms.shape[0]), int(sampler.uniforms.stride(0))

    def steps(self, t=0):
        """int64 [B]: the step of block position t per row"""
        B = self.uniforms.shape[1]
        base = torch.full((B,), self.step0, dtype=torch.int64) if self.step_rows is None else self.step_rows.to(torch.int64)
        return base + t

    def step(self, t):
        """the Sampler of block position t: what a coupled drafter's draft step t draws with"""
        return self.sampler.at_rows(self.steps(t))

    def draft_steps(self, k):
        """step(0) .. step(k - 1) from one gather and one synchronise: a coupled drafter's round"""
        U = self.uniforms
        n, B = U.shape
        s = (self.steps()[None, :] + torch.arange(k, dtype=torch.int64)[:, None]).to(U.device)
        u = U[s.clamp(0, n - 1), torch.arange(B, device=U.device)[None, :]]
        u = torch.where((s >= 0) & (s < n), u, torch.zeros_like(u)).contiguous()
        if u.is_cuda:
            torch.cuda.current_stream().synchronize()      # the library's compute stream reads u
        out = []
        for i in range(k):
            smp = Sampler(self.temperature, self.top_k, self.top_p, U)
            smp.u = u[i]
            out.append(smp)
        return out


def draw_reject_tables(max_new_tokens, n_rows, sample_seed=None, device="cuda"):
    """U_draft, U_acc, U_res of rejection verification, each [max_new_tokens, n_rows] float32 in [0, 1): from a SECOND private
    generator seeded from sample_seed, else from the device's default generator -- drawn after U either way, so U keeps the values
    plain sampling draws from the same seed"""
    shape = (3, max_new_tokens, n_rows)
    if sample_seed is None:
        return torch.rand(shape, dtype=torch.float32, device=device)
    g = torch.Generator(device=device)
    g.manual_seed((sample_seed + 0x5DEECE66D) % (1 << 63))
    return torch.rand(shape, dtype=torch.float32, device=device, generator=g)


class Rejector:
    """The randomness of a generation that verifies with the rejection rule (speculative.py): the generation's Sampler (U: the
    first token behind the prefill) and the three tables of the rounds."""

    def __init__(self, sampler, tables):
        self.sampler = sampler
        self.u_draft, self.u_acc, self.u_res = tables[0], tables[1], tables[2]

    def block(self, step0):
        """the view of a round that starts with step0 generated tokens: block position t is step step0 + t"""
        return RejectorBlock(self, int(step0))


class RejectorBlock:
    """What a rejection verify pass reads: the settings, U_acc / U_res ([n_steps, ldu], row b is column b), the step origin and --
    set by the loop between propose and verify -- draft_logits, the drafter's bf16 logits [B, k, vocab] of the round's draft steps.
    draft_steps(k): the Samplers a stochastic drafter draws step 0 .. k - 1 with, U_draft[step0 + i] (0 past the table)."""

    def __init__(self, rejector, step0):
        smp = rejector.sampler
        self.temperature, self.top_k, self.top_p = smp.temperature, smp.top_k, smp.top_p
        self.u_draft, self.u_acc, self.u_res = rejector.u_draft, rejector.u_acc, rejector.u_res
        self.step0 = step0
        self.n_steps = int(self.u_acc.shape[0])
        self.draft_logits = None

    def draft_steps(self, k):
        return Sampler(self.temperature, self.top_k, self.top_p, self.u_draft).block(self.step0).draft_steps(k)
