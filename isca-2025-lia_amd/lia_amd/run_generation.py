"""Benchmark harness: counterpart of llm/single_instance/run_generation.py (reference :60-117 flags,
:179-182 generate kwargs, :285 identical-row batch, :308-335 timing loop, :337-354 summary).

Differences forced by the environment: there is no network, so no HF checkpoint / tokenizer / prompt.json
(tools/env_setup.sh:221 downloads it) -- the prompt is `--input-tokens` synthetic token ids drawn with
seed 0 (row 0 = BOS), and weights are a seeded random init of the named OPT shape unless `-m` points at a
local HF checkpoint directory.  Everything else -- the protocol and the four summary lines -- is the
reference's.
"""
import argparse
import os
import time

import numpy as np
import torch

from .generation import generate
from .model import LiaOPTModel, resolve_shape
from .scheduler import default_stream_format


def add_model_args(p):
    """the model flags every harness shares (run_generation, run_accuracy)"""
    p.add_argument("-m", "--model-id", type=str, default="facebook/opt-30b", help="OPT shape name or local HF checkpoint dir")
    p.add_argument("--dtype", type=str, choices=["bfloat16"], default="bfloat16")


def add_lia_args(p):
    """the seven LIA flags, same names / types / defaults as run.py:195-215 and run_generation.py:111-117"""
    p.add_argument("--prefill-policy", default=1, type=int)
    p.add_argument("--decoding-policy", default=1, type=int)
    p.add_argument("--no-overlap", action="store_true")
    p.add_argument("--pin-weight", action="store_true")
    p.add_argument("--gpu-percentage", default=0, type=int)
    p.add_argument("--num-minibatch", default=1, type=int)
    p.add_argument("--enable-cxl", action="store_true")


def add_stream_format_arg(p):
    p.add_argument("--stream-format", default=None, choices=["raw", "pack10"],
                   help="wire format of the pinned streamed layers: a lossless packed format (default pack10, or $LIA_STREAM_FORMAT; same "
                        "results bit for bit, fewer bytes over the host link; layers that do not pack are pinned raw) or raw bf16 (what the "
                        "reference ships); a model directory in the build's packed format defaults to the format on disk")


def add_split_decode_arg(p):
    p.add_argument("--split-decode", default=None, choices=["measured", "on", "off"],
                   help="a decode step's GPU attention: the split-key route (a row's keys cut into chunks over many workgroups) where it "
                        "was measured faster (measured: the default, or $LIA_SPLIT_DECODE), at every step over more keys than one chunk "
                        "(on), or never (off); a cache beyond the one-workgroup kernel's LDS takes it whatever this says")


def add_init_args(p):
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--init", default="normal", choices=["normal", "uniform01", "trained-like"],
                   help="uniform01 = the reference's dummy-weight recipe (utils/opt-weight-gen.py:61-62)")


def lia_kwargs_of(args):
    """generate()'s / score()'s LIA kwargs of the command line"""
    return dict(prefill_policy=args.prefill_policy, decoding_policy=args.decoding_policy, no_overlap=args.no_overlap,
                pin_weight=args.pin_weight, gpu_percentage=args.gpu_percentage, num_minibatch=args.num_minibatch,
                enable_cxl=args.enable_cxl)


def attach_scheduler(model, stream_format, split_decode=None):
    """the scheduler generate() / score() drive, with the wire format and the --split-decode mode the command line names"""
    if getattr(model, "family", "opt") == "llama":
        from .llama import LlamaScheduler
        model._lia_scheduler = LlamaScheduler(model, pack=stream_format, split_decode=split_decode)
    else:
        from .scheduler import OffloadScheduler
        model._lia_scheduler = OffloadScheduler(model, wire=stream_format, split_decode=split_decode)
    return model._lia_scheduler


def build_parser():
    p = argparse.ArgumentParser("Generation script (bf16 path, MI355X)", add_help=True)
    add_model_args(p)
    p.add_argument("--input-tokens", default="32", type=str)
    p.add_argument("--max-new-tokens", default=32, type=int)
    p.add_argument("--greedy", action="store_true")
    p.add_argument("--ipex", action="store_true", help="accepted for command-line compatibility; no effect")
    p.add_argument("--benchmark", action="store_true")
    p.add_argument("--num-iter", default=100, type=int)
    p.add_argument("--num-warmup", default=10, type=int)
    p.add_argument("--batch-size", default=1, type=int)
    p.add_argument("--token-latency", action="store_true")
    p.add_argument("--prompt", default=None, type=str,
                   help="input prompt for self-defined if needed (run_generation.py:87); needs the tokenizer files in the -m directory")
    p.add_argument("--prompt-file", default=None, type=str,
                   help="a text file with one prompt per line: the batch is the prompts in file order, cycled to --batch-size, left "
                        "padded, with the matching attention_mask (needs the tokenizer files in the -m directory; not with --prompt)")
    p.add_argument("--followup", action="append", default=None, type=str,
                   help="with --prompt: a follow-up turn appended to the live KV cache of the conversation (generate(past=)); may be "
                        "given several times, one turn each.  Every turn generates --max-new-tokens and is printed; no benchmark loop")
    p.add_argument("--reserve-tokens", default=None, type=int,
                   help="with --followup: cache positions kept free behind the first turn for the later ones (default: what the "
                        "follow-ups and their new tokens need)")
    p.add_argument("--append-policy", default=None, type=int, choices=(0, 2, 3),
                   help="with --followup: 2 = a follow-up block's attention runs on the host cores (host caches only); default: the prefill policy")
    p.add_argument("--profile", action="store_true",
                   help="one profiled generate() before the timed loop (run_generation.py:103,290-307 runs torch.profiler over five "
                        "there); here the library's own HIP-event brackets: GEMM time / rates per phase, host attention, link traffic")
    add_lia_args(p)
    # build-specific
    add_stream_format_arg(p)
    add_split_decode_arg(p)
    p.add_argument("--auto-plan", action="store_true",
                   help="measure this box (lia_amd.planner.calibrate, a few seconds) and let the planner choose --gpu-percentage, "
                        "the policies and --cpu-layers instead of the hand-picked values of llm/scripts/lia_*.sh")
    p.add_argument("--plan-max-gpu-percentage", default=100, type=int,
                   help="--auto-plan what-if: the plan keeps at most this share of the layers resident (the others must stream)")
    p.add_argument("--plan-hbm-gb", default=0.0, type=float, help="--auto-plan what-if: plan as if the GPU had this much HBM")
    p.add_argument("--cpu-layers", default=0, type=int,
                   help="with --decoding-policy 2: this many streamed layers take their decode step on the host cores (policy 1 per layer); "
                        "-1 = chosen online from the measured decode steps (scheduler.CoopController), seeded by the planner")
    p.add_argument("--cpu-layers-start", default=None, type=int, help=argparse.SUPPRESS)
    p.add_argument("--cxl-nodes", default=None, type=str,
                   help="NUMA nodes of the --enable-cxl tier, e.g. 2,3 (the reference hard-codes {2, 3}, lia/cxl/numa_alloc.c:80-81; default: "
                        "$LIA_CXL_NODES, else {2, 3} where both exist, else this box's memory nodes other than the GPU's own)")
    p.add_argument("--result-json", default=None, type=str,
                   help="write one JSON record of the run to this path (tools/run_matrix.py): the summary numbers, the weight stream's "
                        "bytes / copy-engine time over the timed iterations, the library's per-launch brackets of the FIRST (warm-up) "
                        "iteration, the host-memory peak, the planner's pick for the same line; a run the box cannot hold (MemoryError) "
                        "is recorded with its reason instead of a traceback")
    p.add_argument("--do-sample", action="store_true",
                   help="sampled decoding (temperature -> top-k -> top-p -> multinomial, the lia_sample kernel) instead of greedy")
    p.add_argument("--temperature", default=0.9, type=float, help="with --do-sample (the reference harness passes 0.9)")
    p.add_argument("--top-k", default=50, type=int, help="with --do-sample; 0: off")
    p.add_argument("--top-p", default=1.0, type=float, help="with --do-sample; 1: off")
    p.add_argument("--sample-seed", default=0, type=int, help="with --do-sample: the seed of the generation's uniforms")
    p.add_argument("--draft-model", default=None, type=str,
                   help="speculative greedy decoding: an OPT / Llama shape name or checkpoint directory of the same vocabulary, kept all "
                        "resident (policies 3 / 3) beside the target; it proposes --draft-tokens tokens per round and one pass of the "
                        "target's weights verifies them (same ids as plain greedy; with --do-sample only together with --sampled-verify; "
                        "not with --cpu-layers -1)")
    p.add_argument("--draft-tokens", default=4, type=int, help="with --draft-model: draft tokens per round")
    p.add_argument("--acceptance", default="common", choices=["common", "row"],
                   help="with --draft-model: common = every row keeps the minimum over the rows per round; row = every row keeps what it "
                        "accepted itself on a ragged KV cache (OPT with --prefill-policy 3 --decoding-policy 3)")
    p.add_argument("--sampled-verify", action="store_true",
                   help="with --draft-model and --do-sample: speculative SAMPLED decoding -- the verify pass draws every block position "
                        "with the generation's own uniforms, a draft token is accepted iff it equals the draw (the ids are the same "
                        "function of the logits and --sample-seed as plain --do-sample)")
    p.add_argument("--draft-coupled", action="store_true",
                   help="with --sampled-verify: the draft model samples its own logits with the target's settings and uniforms (it guesses "
                        "the draw, not the argmax)")
    p.add_argument("--verify-rule", default="draw", choices=["draw", "rejection"],
                   help="with --sampled-verify: draw = accept a draft token iff it equals the sampler's own draw; rejection = the draft model "
                        "samples its own logits and a token is accepted with probability min(1, p / q), else a draw of the residual "
                        "(an exact sample, but not the ids of plain --do-sample; common acceptance only, not with --draft-coupled)")
    p.add_argument("--logprobs", default=None, type=int,
                   help="report every generated token's log-probability and its N most likely alternatives (generate(logprobs=N), "
                        "N in 0..32; the model's own distribution, before temperature / filters / constraints): printed per token "
                        "with --prompt, written to --result-json")
    p.add_argument("--repetition-penalty", default=None, type=float,
                   help="HF's repetition_penalty (> 0; 1.0: off): the logit of a token of the prompt or generated so far is divided by it "
                        "(a negative one multiplied), greedy and sampled (generate(repetition_penalty=); not with --draft-model)")
    p.add_argument("--presence-penalty", default=None, type=float,
                   help="OpenAI's / vLLM's presence_penalty (0: off): subtracted from the logit of every token generated so far")
    p.add_argument("--frequency-penalty", default=None, type=float,
                   help="OpenAI's / vLLM's frequency_penalty (0: off): subtracted once per time the token was generated so far")
    p.add_argument("--suppress-tokens", default=None, type=str,
                   help="constrained decoding: token ids no row may emit, e.g. 5,6,7 (generate(suppress_tokens=): they count as -inf in "
                        "the argmax and in the sampler)")
    p.add_argument("--allowed-tokens-file", default=None, type=str,
                   help="constrained decoding: ONE allow-list for every row and step -- a .npy of token ids, or text with one id per "
                        "line; every other token counts as -inf (not with --acceptance row or --verify-rule rejection)")
    add_init_args(p)
    return p


def format_logprobs(lp, new_ids, tokenizer=None, row=0):
    """--logprobs: one line per generated token of `row` -- the token, its log-probability under the model's own distribution, and
    the alternatives of that step (logprobs.TokenLogprobs; new_ids: the generated ids [B, n_new])"""
    name = (lambda t: repr(tokenizer.decode([t]))) if tokenizer is not None else str
    lines = []
    for s_, tok in enumerate(new_ids[row].tolist()):
        alts = ", ".join(f"{name(int(i))} {float(v):.4f}" for i, v in zip(lp.top_ids[row, s_].tolist(), lp.top_logprobs[row, s_].tolist())
                         if i >= 0)
        lines.append(f"  step {s_}: {name(tok)} logprob {float(lp.token_logprobs[row, s_]):.4f}" + (f" | top: {alts}" if alts else ""))
    lines.append(f"  sequence logprob {float(lp.sequence_logprob()[row]):.4f}")
    return lines


def constraint_kwargs(args, vocab):
    """generate()'s constraint kwargs of the command line: none without --suppress-tokens / --allowed-tokens-file.  The allow-list is
    turned into its complement, a suppress list: one static row, packed and uploaded once."""
    import numpy as np
    banned = set()
    if getattr(args, "suppress_tokens", None):
        try:
            banned |= {int(v) for v in args.suppress_tokens.split(",") if v.strip()}
        except ValueError:
            raise SystemExit(f"[ERROR] --suppress-tokens takes comma-separated token ids, got {args.suppress_tokens!r}") from None
    if getattr(args, "allowed_tokens_file", None):
        path = args.allowed_tokens_file
        try:
            ids = np.load(path) if path.endswith(".npy") else np.loadtxt(path, dtype=np.int64, ndmin=1)
        except (OSError, ValueError) as e:
            raise SystemExit(f"[ERROR] --allowed-tokens-file {path}: {e}") from None
        ids = np.asarray(ids).reshape(-1)
        if ids.size == 0 or not np.issubdtype(ids.dtype, np.integer):
            raise SystemExit(f"[ERROR] --allowed-tokens-file {path}: expected a non-empty list of integer token ids, got {ids.dtype} x {ids.size}")
        if ids.min() < 0 or ids.max() >= vocab:
            raise SystemExit(f"[ERROR] --allowed-tokens-file {path}: token id {int(ids.min() if ids.min() < 0 else ids.max())} is outside "
                             f"the vocabulary [0, {vocab})")
        banned |= set(range(vocab)) - set(ids.tolist())
    return {"suppress_tokens": sorted(banned)} if banned else {}


def penalty_kwargs(args):
    """generate()'s penalty kwargs of the command line: none without --repetition-penalty / --presence-penalty / --frequency-penalty"""
    names = ("repetition_penalty", "presence_penalty", "frequency_penalty")
    return {k: getattr(args, k) for k in names if getattr(args, k, None) is not None}


def check_spec_sample_flags(args):
    """--sampled-verify / --draft-coupled without what they modify: refused by name"""
    if args.sampled_verify and not (args.draft_model and args.do_sample):
        raise SystemExit("[ERROR] --sampled-verify needs --draft-model and --do-sample: it verifies the draft with the sampler's own draws")
    if args.draft_coupled and not args.sampled_verify:
        raise SystemExit("[ERROR] --draft-coupled needs --sampled-verify (with --draft-model and --do-sample): the draft model draws with "
                         "the target's uniforms, which only a sampled verify pass confirms")
    if getattr(args, "verify_rule", "draw") == "rejection":
        if not args.sampled_verify:
            raise SystemExit("[ERROR] --verify-rule rejection needs --sampled-verify (with --draft-model and --do-sample)")
        if args.draft_coupled:
            raise SystemExit("[ERROR] --verify-rule rejection together with --draft-coupled: the rejection rule's drafter draws with "
                             "uniforms of its own")
        if args.acceptance != "common":
            raise SystemExit("[ERROR] --verify-rule rejection together with --acceptance row is not supported")


def synthetic_prompt(vocab, n_tokens, batch, seed=0):
    g = torch.Generator().manual_seed(seed)
    row = torch.randint(4, vocab, (n_tokens,), generator=g, dtype=torch.int64)
    row[0] = 2
    return row[None, :].repeat(batch, 1)          # prompt = [prompt] * batch_size  (run_generation.py:285)


TOKENIZER_FILES = ("tokenizer.json", "tokenizer.model", "vocab.json", "tokenizer_config.json")


def choose_cxl_nodes(named=None):
    """The node set of the NUMA / CXL tier.  The reference hard-codes nodes {2, 3} of ITS machine (lia/cxl/numa_alloc.c:80-81); a box
    without them would fail every --enable-cxl line with "Fail to allocate CXL memory!".  Order: --cxl-nodes, $LIA_CXL_NODES (read by
    the library itself: None is returned), {2, 3} where both have memory, else the box's memory nodes other than GPU 0's own (all of
    them on a one- or two-node box)."""
    from . import hostinfo
    from .cxl.numa_alloc import set_cxl_nodes
    if named:
        nodes = [int(v) for v in named.split(",")]
    elif os.environ.get("LIA_CXL_NODES"):
        return None
    else:
        have = hostinfo.numa_nodes()
        if 2 in have and 3 in have:
            nodes = [2, 3]
        else:
            own = hostinfo.gpu_numa_node(0)
            nodes = [n for n in have if n != own] or have or [0]
            if len(have) <= 2:
                nodes = have or [0]
    set_cxl_nodes(nodes)
    return nodes


def load_tokenizer(model_id):
    """The tokenizer a local checkpoint directory ships (run_generation.py:167, `from_pretrained(args.model_id)`), or None: a shape
    name (no files offline) or a directory without tokenizer files."""
    if not os.path.isdir(model_id) or not any(os.path.exists(os.path.join(model_id, f)) for f in TOKENIZER_FILES):
        return None
    from transformers import AutoTokenizer
    return AutoTokenizer.from_pretrained(model_id, local_files_only=True)


def prompt_input_ids(args, vocab, tokenizer, out=print):
    """run_generation.py:262-285: `--prompt` goes through the checkpoint's tokenizer, every row of the batch is that prompt
    (`prompt = [prompt] * args.batch_size`), and its size is printed.  The reference otherwise draws the text from its prompt.json
    pool by --input-tokens; that file's texts are not reproduced here, so without --prompt the ids are the synthetic row of
    --input-tokens tokens as before."""
    if args.prompt is None:
        return synthetic_prompt(vocab, int(args.input_tokens), args.batch_size)
    if tokenizer is None:
        raise SystemExit("[ERROR] --prompt needs a tokenizer: point -m at a checkpoint directory that ships its tokenizer files "
                         f"({', '.join(TOKENIZER_FILES[:3])}); {args.model_id!r} has none")
    row = tokenizer(args.prompt, return_tensors="pt").input_ids.to(torch.int64)
    if row.numel() == 0 or int(row.max()) >= vocab or int(row.min()) < 0:
        raise SystemExit(f"[ERROR] the tokenizer produced ids outside the model's vocabulary of {vocab} entries")
    out("---- Prompt size:", int(row.shape[1]))
    return row.repeat(args.batch_size, 1)


def prompt_file_inputs(args, vocab, tokenizer, pad_token_id, out=print):
    """--prompt-file: one prompt per line (blank lines skipped), the batch = the prompts in file order cycled to --batch-size (as the
    reference repeats its one prompt), each tokenized alone and left padded to the longest with the tokenizer's pad token (the
    model's pad_token_id when the tokenizer has none).  Returns (input_ids int64 [B, T], attention_mask int64 [B, T])."""
    if tokenizer is None:
        raise SystemExit("[ERROR] --prompt-file needs a tokenizer: point -m at a checkpoint directory that ships its tokenizer files "
                         f"({', '.join(TOKENIZER_FILES[:3])}); {args.model_id!r} has none")
    with open(args.prompt_file, encoding="utf-8") as f:
        prompts = [line.rstrip("\n") for line in f if line.strip()]
    if not prompts:
        raise SystemExit(f"[ERROR] --prompt-file {args.prompt_file!r} holds no prompt")
    rows = []
    for text in prompts:
        r = tokenizer(text, return_tensors="pt").input_ids.to(torch.int64)[0]
        if r.numel() == 0 or int(r.max()) >= vocab or int(r.min()) < 0:
            raise SystemExit(f"[ERROR] the tokenizer produced ids outside the model's vocabulary of {vocab} entries for {text!r}")
        rows.append(r)
    pad = tokenizer.pad_token_id if tokenizer.pad_token_id is not None else pad_token_id
    B, T = args.batch_size, max(int(r.numel()) for r in rows)
    ids = torch.full((B, T), int(pad), dtype=torch.int64)
    mask = torch.zeros((B, T), dtype=torch.int64)
    for b in range(B):
        r = rows[b % len(rows)]
        ids[b, T - r.numel():] = r
        mask[b, T - r.numel():] = 1
    out("---- Prompt sizes:", [int(r.numel()) for r in rows])
    return ids, mask


def is_llama(args):
    """`-m` names a Llama: a HF directory whose config.json says so (run_generation.py:159-166 loads OPT and Llama through the same
    AutoModelForCausalLM call), or one of the known Llama shape names (random-init weights, like the OPT shape names)"""
    if os.path.isdir(args.model_id):
        from .checkpoint import is_llama_dir
        return is_llama_dir(args.model_id)
    try:
        resolve_shape(args.model_id)
        return False
    except ValueError:
        from .llama import resolve_llama_shape
        try:
            resolve_llama_shape(args.model_id)
            return True
        except ValueError:
            return False


def model_shape(args):
    """shape of the model `-m` names, without loading it (the planner needs it first)"""
    if is_llama(args):
        from .checkpoint import llama_shape_of
        from .llama import resolve_llama_shape
        return llama_shape_of(args.model_id) if os.path.isdir(args.model_id) else resolve_llama_shape(args.model_id)
    if os.path.isdir(args.model_id):
        import json
        from . import packed_checkpoint
        from .model import OPTShape
        if packed_checkpoint.is_packed_dir(args.model_id):
            sh = json.load(open(os.path.join(args.model_id, packed_checkpoint.MANIFEST)))["shape"]
            return OPTShape(sh["name"], sh["hidden"], sh["heads"], sh["ffn"], sh["layers"], vocab=sh["vocab"], max_pos=sh["max_pos"])
        cfg = json.load(open(os.path.join(args.model_id, "config.json")))
        return OPTShape(os.path.basename(args.model_id.rstrip("/")), cfg["hidden_size"], cfg["num_attention_heads"], cfg["ffn_dim"],
                        cfg["num_hidden_layers"], vocab=cfg["vocab_size"], max_pos=cfg["max_position_embeddings"])
    return resolve_shape(args.model_id)


def auto_plan(args, out=print):
    """--auto-plan: calibrate the box, plan, overwrite the LIA flags with the plan (f-3)."""
    from . import planner
    box = planner.calibrate(verbose=False)
    if args.plan_hbm_gb:                           # what-if: pretend the GPU is smaller
        box.hbm_gb = float(args.plan_hbm_gb)
    max_pct = int(args.plan_max_gpu_percentage)    # what-if / tests: cap the resident share
    fmt = args.stream_format or default_stream_format()
    box.wire_ratio = {"raw": 1.0, "pack10": 0.675}[fmt]
    box.wire_cache, box.wire_cache_ws, box.resident_packed = planner.wire_cache_default(), planner.wire_cache_ws_default(), planner.resident_packed_default()      # (Llama models stream nothing: every layer is resident)
    shape = model_shape(args)
    pl = planner.plan(shape, args.batch_size, int(args.input_tokens), args.max_new_tokens, box, max_gpu_percentage=max_pct)
    args.gpu_percentage, args.prefill_policy, args.decoding_policy = pl.gpu_percentage, pl.prefill_policy, pl.decoding_policy
    args.num_minibatch, args.pin_weight, args.stream_format = pl.num_minibatch, True, fmt
    coop_note = ""
    if pl.n_gpu_layers < shape.layers and pl.decoding_policy in (2, 3):
        # layers stream: the host cores take some of them (build-defined cooperative split).  The plan SEEDS the count; the
        # scheduler's online controller (cpu_layers = -1) moves it with the measured decode steps.  With room in HBM for every
        # layer's KV cache the other streamed layers attend on the GPU (policies 3/3): the host cores then run nothing but their
        # own layers (OPT-30B gpu% = 10 on MI355X: 190-205 against 165-185 tokens/s)
        B_, T_, new_ = args.batch_size, int(args.input_tokens), args.max_new_tokens
        c2, ms2 = planner.plan_cpu_layers(shape, B_, T_, new_, pl.gpu_percentage, box)
        c3, ms3 = planner.plan_cpu_layers(shape, B_, T_, new_, pl.gpu_percentage, box, kv_in_hbm=True)
        hbm3 = planner.estimate(shape, B_, T_, new_, pl.gpu_percentage, 3, box)[2]
        if c3 > 0 and ms3 < ms2 and hbm3 <= 0.92 * box.hbm_gb:
            args.prefill_policy, args.decoding_policy, args.cpu_layers_start, ms = 3, 3, c3, ms3
        else:
            args.prefill_policy, args.decoding_policy, args.cpu_layers_start, ms = 0, 2, c2, ms2
        args.cpu_layers = -1 if args.cpu_layers_start > 0 else 0
        if args.cpu_layers:
            coop_note = f"; cooperative split predicted {1e3 * B_ / ms:.1f} tokens/s at {args.cpu_layers_start} host layers"
    out(f"auto-plan: calibrated {box.calibrated}")
    out(f"auto-plan: gpu%={pl.gpu_percentage} ({pl.n_gpu_layers} resident layers) prefill policy {args.prefill_policy} decode policy "
        f"{args.decoding_policy} cpu-layers {'online from ' + str(args.cpu_layers_start) if args.cpu_layers < 0 else args.cpu_layers} wire {fmt}; predicted prefill {pl.prefill_ms:.0f} ms, "
        f"{pl.decode_tokens_per_s:.1f} tokens/s ({pl.note}){coop_note}")
    return pl


def load_model(args):
    if is_llama(args):
        # build-defined (the reference's LlamaDecoderLayer_forward carries no policy, decoder.py:121-169): layers [0, gpu%) resident,
        # the others stream through the same WeightPipeline, every layer's arithmetic and KV cache on the GPU
        from .llama import LiaLlamaModel
        shape = model_shape(args)
        n_gpu = shape.layers if args.gpu_percentage >= 100 else int(shape.layers * args.gpu_percentage / 100)
        fmt = {"raw": 0, "pack10": 10}[args.stream_format or default_stream_format()]
        if os.path.isdir(args.model_id):
            from .checkpoint import load_hf_llama
            return load_hf_llama(args.model_id, n_gpu_layers=n_gpu, pin_weight=True, wire=fmt)
        return LiaLlamaModel.random_init(shape, seed=args.seed, n_gpu_layers=n_gpu, pin_weight=True, pack=fmt)
    if os.path.isdir(args.model_id):
        from . import packed_checkpoint
        if packed_checkpoint.is_packed_dir(args.model_id):
            import json
            man = json.load(open(os.path.join(args.model_id, packed_checkpoint.MANIFEST)))
            shape_layers = man["shape"]["layers"]
            if args.stream_format is None:       # stream what is on disk, as it is
                wires = [e["wire"] for e in man["layers"]]
                args.stream_format = {0: "raw", 10: "pack10"}.get(max(set(wires), key=wires.count), "pack10")     # (load_packed refuses other formats by name)
            return packed_checkpoint.load_packed(args.model_id, n_gpu_layers=int(shape_layers * args.gpu_percentage / 100))
        # a HF directory: converted layer by layer, every layer straight to the tier the flags name (checkpoint.load_hf_opt)
        from .checkpoint import load_hf_opt
        from .scheduler import OffloadScheduler
        import json
        L_ = json.load(open(os.path.join(args.model_id, "config.json")))["num_hidden_layers"]
        n_gpu = int(L_ * args.gpu_percentage / 100)
        fmt = {"raw": 0, "pack10": 10}[args.stream_format or default_stream_format()]
        raw = OffloadScheduler.cpu_layer_set(n_gpu, L_, args.cpu_layers) if (args.cpu_layers and args.cpu_layers > 0 and args.decoding_policy in (2, 3)) else ()
        from .scheduler import placement_formats
        fmt, raw = placement_formats(args.prefill_policy, args.decoding_policy, fmt, n_gpu, L_, args.pin_weight, args.enable_cxl, raw)
        return load_hf_opt(args.model_id, n_gpu_layers=n_gpu, pin_weight=args.pin_weight, enable_cxl=args.enable_cxl, wire=fmt, raw_layers=raw)
    shape = resolve_shape(args.model_id)
    n_gpu = int(shape.layers * args.gpu_percentage / 100)
    fmt = {"raw": 0, "pack10": 10}[args.stream_format or default_stream_format()]
    from .scheduler import OffloadScheduler, placement_formats
    raw = OffloadScheduler.cpu_layer_set(n_gpu, shape.layers, args.cpu_layers) if (args.cpu_layers and args.cpu_layers > 0 and args.decoding_policy in (2, 3)) else ()
    # the host path reads a raw copy in place; a 0 / 1 line keeps the packed copy for the prefill's stream beside it (placement_formats)
    fmt, raw = placement_formats(args.prefill_policy, args.decoding_policy, fmt, n_gpu, shape.layers, args.pin_weight, args.enable_cxl, raw)
    return LiaOPTModel.random_init(shape, seed=args.seed, init=args.init, n_gpu_layers=n_gpu,
                                   pin_weight=args.pin_weight, enable_cxl=args.enable_cxl, wire=fmt, raw_layers=raw)


def load_draft(args):
    """--draft-model: the draft model, every layer resident, with a scheduler of its own -> speculative.ModelDrafter"""
    import copy
    from .speculative import ModelDrafter
    d = copy.copy(args)
    d.model_id, d.gpu_percentage, d.prefill_policy, d.decoding_policy = args.draft_model, 100, 3, 3
    d.pin_weight, d.enable_cxl, d.cpu_layers, d.stream_format = True, False, 0, args.stream_format
    model = load_model(d)
    attach_scheduler(model, d.stream_format or default_stream_format())
    return ModelDrafter(model, coupled=args.draft_coupled, stochastic=getattr(args, "verify_rule", "draw") == "rejection")


def summarize_speculation(spec_log, total_list, batch_size, out=print, acceptance="common"):
    """accepted draft tokens per round over the timed iterations, beside the latencies: -> the record of --result-json.
    acceptance="row": a row keeps its own count, so the tokens of a round are the mean over the rows (accepted_per_row_round; a full
    row reports draft_tokens, so this too is an upper bound) instead of the minimum."""
    commons = [c for c, _ in spec_log]
    rec = {"rounds": len(commons), "accepted_per_round": round(float(np.mean(commons)), 3) if commons else None,
           "accepted_histogram": {int(v): int(n) for v, n in zip(*np.unique(commons, return_counts=True))} if commons else {}}
    if acceptance == "row" and commons:
        rec.update(acceptance="row", accepted_per_row_round=round(float(np.mean([np.mean(a) for _, a in spec_log])), 3),
                   accepted_rows=[list(map(int, a)) for _, a in spec_log])
        out("Per-row acceptance: accepted draft tokens per row and round: %s" % rec["accepted_per_row_round"])
        commons = [float(np.mean(a)) for _, a in spec_log]
    out("Speculative rounds: %d, accepted draft tokens per round: %s (histogram %s)" % (rec["rounds"], rec["accepted_per_round"], rec["accepted_histogram"]))
    if total_list and commons:
        passes = sum(len(x) - 1 for x in total_list)
        secs = sum(sum(x[1:]) for x in total_list)
        tokens = sum(c + 1 for c in commons)
        rec.update(target_passes=passes, s_per_pass=secs / max(passes, 1),
                   decode_tokens_per_s=batch_size * tokens / max(secs, 1e-9))
        out("Average latency per target pass (draft included): %.3f sec; decode throughput by accepted tokens: %.2f tokens/s (an upper "
            "bound: the last round of an iteration may be cut)" % (rec["s_per_pass"], rec["decode_tokens_per_s"]))
    return rec


def summarize(total_time, num_iter, num_warmup, total_list, batch_size, out=print):
    """The reference's summary block (run_generation.py:337-354), verbatim formats; returns the numbers."""
    out("\n", "-" * 10, "Summary:", "-" * 10)
    latency = total_time / (num_iter - num_warmup)
    out("Inference latency: %.3f sec." % latency)
    res = {"inference_latency_s": latency}
    if total_list:
        from itertools import chain
        first_latency = float(np.mean([x[0] for x in total_list]))
        average_2n = sorted(chain(*[x[1:] for x in total_list]))
        average_2n_latency = float(np.mean(average_2n))
        p90_latency = average_2n[int(len(average_2n) * 0.9)]
        p99_latency = average_2n[int(len(average_2n) * 0.99)]
        out("First token average latency: %.3f sec." % first_latency)
        out("Average 2... latency: %.3f sec." % average_2n_latency)
        out("P90 2... latency: %.3f sec." % p90_latency)
        out("P99 2... latency: %.3f sec." % p99_latency)
        res.update(prefill_ms=1e3 * first_latency, decode_tokens_per_s=batch_size / average_2n_latency,
                   p90_s=p90_latency, p99_s=p99_latency)
    return res


def profile_once(model, input_ids, generate_kwargs, out=print, warm=True):
    """--profile (run_generation.py:290-307): one generate() with every GEMM launch bracketed by HIP events on its own stream
    (lia_prof_*), the host-attention wall clock and the weight stream's copy-engine time; prints the table and returns it.
    warm=False (--result-json): no untimed call in front -- the profiled generation IS the harness's first warm-up iteration."""
    sched = model._lia_scheduler
    if warm:
        generate(model, input_ids, **dict(generate_kwargs, max_steps=2))       # untimed: allocations, placement, page-in
    elif getattr(sched, "ctx", None) is None:
        generate(model, input_ids, **dict(generate_kwargs, max_steps=1))       # the library context (and its brackets) exists after the first forward
    st = {}

    def host_time(reset=True):
        ht = dict(getattr(sched, "host_layer_time", None) or {"ms": 0.0, "calls": 0})
        if reset and hasattr(sched, "host_layer_time"):
            sched.host_layer_time = {"ms": 0.0, "calls": 0}
        return ht

    def hook(step):
        if step == 0:
            sched.stream_stats(reset=True)
            host_time()
            sched.ctx.prof_start(65536)
        elif step == 1:
            st["prefill"], st["prefill_h2d"], st["prefill_host"] = sched.ctx.prof_stop(), sched.stream_stats(reset=True), host_time()
            sched.ctx.prof_start(65536)

    res = generate(model, input_ids, step_hook=hook, **dict(generate_kwargs, token_latency=True))
    lat = res[1]
    st["decode"], st["decode_h2d"], st["decode_host"] = sched.ctx.prof_stop(), sched.stream_stats(), host_time()
    if "prefill" not in st:          # a one-token generation: everything is the prefill
        st["prefill"], st["prefill_h2d"], st["decode"], st["decode_h2d"] = st["decode"], st["decode_h2d"], None, (0.0, 0.0)
        st["prefill_host"], st["decode_host"] = st["decode_host"], {"ms": 0.0, "calls": 0}
    rows = []
    for phase, wall in (("prefill", lat[0]), ("decode", sum(lat[1:]))):
        pr = st[phase]
        if pr is None:
            continue
        b, ms = st[phase + "_h2d"]
        for regime in ("tiled", "skinny"):
            n = pr[regime + "_launches"]
            if n:
                t = pr[regime + "_ms"]
                rows.append((phase, f"GEMM {regime} (M {'> 256' if regime == 'tiled' else '<= 256'})", n, t, f"{pr[regime + '_flops'] / t / 1e9:.1f} TFLOP/s",
                             f"{pr[regime + '_bytes'] / t / 1e6:.0f} GB/s"))
        if pr["host_attention_calls"]:
            rows.append((phase, "host attention (policy 2)", pr["host_attention_calls"], pr["host_attention_ms"], "", ""))
        hl = st.get(phase + "_host") or {}
        if hl.get("calls"):
            rows.append((phase, "host layers (policy 1: linears + attention on the host cores)", hl["calls"], hl["ms"], "", ""))
        if b:
            rows.append((phase, "weight stream H2D (copy engine busy)", "", ms, "", f"{b / max(ms, 1e-9) / 1e6:.1f} GB/s"))
        rows.append((phase, "wall clock", "", 1e3 * wall, "", ""))
    out("\n" + "-" * 10 + " Profile (one generate; HIP-event brackets per launch) " + "-" * 10)
    out("%-8s %-40s %8s %12s %16s %12s" % ("phase", "what", "calls", "ms", "compute", "memory"))
    for r in rows:
        out("%-8s %-40s %8s %12.3f %16s %12s" % r)
    profile_once.last = (res, rows)
    return rows


def _dominant(rows, phase):
    """the largest time share of a phase among the profiled resources (GEMM regimes, host attention, the link's copy engine)"""
    cand = [(r[3], r[1]) for r in rows if r[0] == phase and r[1] != "wall clock"]
    wall = next((r[3] for r in rows if r[0] == phase and r[1] == "wall clock"), None)
    if not cand or not wall:
        return None
    ms, what = max(cand)
    return {"what": what, "ms": round(ms, 2), "share_of_wall": round(ms / wall, 3)}


def plan_beside(args):
    """what lia_amd.planner would pick for this line's model / batch / lengths on this box (not applied): the reference hand-picks
    these per script line (llm/scripts/lia_offline.sh:13-29)"""
    if is_llama(args):
        return {"note": "lia_amd.planner models OPT layers and the LIA policies; a Llama runs every layer on the GPU (build-defined, SURVEY.md quirk 3)"}
    try:
        from . import planner
        box = planner.calibrate(verbose=False)
        fmt = args.stream_format or default_stream_format()
        box.wire_ratio = {"raw": 1.0, "pack10": 0.675}[fmt]
        box.wire_cache, box.wire_cache_ws, box.resident_packed = planner.wire_cache_default(), planner.wire_cache_ws_default(), planner.resident_packed_default()
        shape = model_shape(args)
        B, T, new = args.batch_size, int(args.input_tokens), args.max_new_tokens
        pl = planner.plan(shape, B, T, new, box)
        rec = {"gpu_percentage": pl.gpu_percentage, "prefill_policy": pl.prefill_policy, "decoding_policy": pl.decoding_policy,
               "predicted_prefill_ms": round(pl.prefill_ms, 1), "predicted_decode_tokens_per_s": round(pl.decode_tokens_per_s, 1),
               "hbm_gb": round(pl.hbm_gb, 1), "host_gb": round(pl.host_gb, 1), "note": pl.note, "calibrated": box.calibrated}
        if pl.n_gpu_layers < shape.layers:
            c2, ms2 = planner.plan_cpu_layers(shape, B, T, new, pl.gpu_percentage, box)
            c3, ms3 = planner.plan_cpu_layers(shape, B, T, new, pl.gpu_percentage, box, kv_in_hbm=True)
            rec["cooperative"] = {"kv_on_host": {"host_layers": c2, "predicted_tokens_per_s": round(1e3 * B / ms2, 1)},
                                  "kv_in_hbm": {"host_layers": c3, "predicted_tokens_per_s": round(1e3 * B / ms3, 1)}}
        try:          # the hand-picked flags through the same model, for the ratio
            pre, dec, hbm, host, _ = planner.estimate(shape, B, T, new, args.gpu_percentage, args.decoding_policy if args.decoding_policy in (2, 3) else 2, box)
            rec["hand_picked_estimate"] = {"prefill_ms": round(pre, 1), "decode_tokens_per_s": round(1e3 * B / dec, 1), "hbm_gb": round(hbm, 1),
                                           "host_gb": round(host, 1), "note": "decode estimated as policy 2" if args.decoding_policy not in (2, 3) else ""}
        except Exception as e:       # noqa: BLE001
            rec["hand_picked_estimate"] = {"error": str(e)}
        return rec
    except MemoryError as e:
        return {"error": f"no placement fits: {e}"}


def followup_ids(args, vocab, tokenizer):
    """--followup texts -> [int64 [B, T2]] through the checkpoint's tokenizer, every row the same text (as --prompt); no BOS / EOS
    of their own: a follow-up continues the conversation"""
    if args.prompt is None:
        raise SystemExit("[ERROR] --followup continues the conversation that --prompt starts: give --prompt")
    if tokenizer is None:
        raise SystemExit("[ERROR] --followup needs a tokenizer: point -m at a checkpoint directory that ships its tokenizer files "
                         f"({', '.join(TOKENIZER_FILES[:3])}); {args.model_id!r} has none")
    out = []
    for text in args.followup:
        row = tokenizer(text, return_tensors="pt", add_special_tokens=False).input_ids.to(torch.int64)
        if row.numel() and (int(row.max()) >= vocab or int(row.min()) < 0):
            raise SystemExit(f"[ERROR] the tokenizer produced ids outside the model's vocabulary of {vocab} entries")
        out.append(row.reshape(1, -1).repeat(args.batch_size, 1))
    return out


def reserve_for(args, followups):
    """--reserve-tokens, or what the follow-up turns need: their tokens and their new tokens"""
    if args.reserve_tokens is not None:
        return int(args.reserve_tokens)
    return sum(int(f.shape[1]) + int(args.max_new_tokens) for f in followups)


def run_conversation(model, input_ids, followups, generate_kwargs, args, tokenizer, out=print):
    """--prompt P --followup F ...: turn 0 generates from the prompt and keeps its state, every follow-up is appended to the live
    cache; each turn's new tokens (and text) are printed.  -> {"turns": [ids of the new tokens of row 0], "turn_s": [...]}"""
    kw = {k: v for k, v in generate_kwargs.items() if k not in ("token_latency", "attention_mask")}
    turns, secs = [], []
    state, seen = None, int(input_ids.shape[1])
    for i, block in enumerate([input_ids] + list(followups)):
        tic = time.time()
        if state is None:
            ids, state = generate(model, block, return_state=True, reserve_tokens=reserve_for(args, followups), **kw)
        else:
            ids, state = generate(model, block, past=state, return_state=True, append_policy=args.append_policy, **kw)
            seen += int(block.shape[1])
        secs.append(time.time() - tic)
        new = ids[0, seen:].tolist()
        seen = int(ids.shape[1])
        turns.append(new)
        if tokenizer is not None:
            out(f"turn {i}: {tokenizer.decode(new, skip_special_tokens=True)!r}")
        out(f"turn {i}: {new} in {secs[-1]:.6f} sec")
    return {"turns": turns, "turn_s": secs}


SAMPLE_FLAGS = ("do_sample", "temperature", "top_k", "top_p", "sample_seed")


def sampling_kwargs(args):
    """generate()'s sampling kwargs of the command line: none without --do-sample"""
    if not args.do_sample:
        return {}
    return dict(do_sample=True, temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, sample_seed=args.sample_seed)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not args.result_json:
        return _main(args)
    import json
    import resource
    from . import hostinfo
    rec = {"argv": list(argv) if argv is not None else None,
           "flags": {k: v for k, v in vars(args).items() if k != "result_json" and (args.do_sample or k not in SAMPLE_FLAGS)}}
    if args.do_sample:
        rec["sampling"] = {k: getattr(args, k) for k in SAMPLE_FLAGS}
    t0 = time.time()
    mem0 = hostinfo.cgroup_memory()["current"]
    rec["_mem_samples"] = []
    try:
        rec["result"] = _main(args, rec)
        rec["status"] = "ok"
    except MemoryError as e:
        rec["status"], rec["reason"] = "refused: memory", str(e)
        print("[refused]", e)
    except ValueError as e:
        rec["status"], rec["reason"] = "refused: flags", str(e)
        print("[refused]", e)
    rec["wall_s"] = round(time.time() - t0, 1)
    mem = hostinfo.cgroup_memory()
    samples = [v for v in rec.pop("_mem_samples", []) + [mem["current"]] if v is not None]
    rec["host_memory"] = {"container_gib_at_start": None if mem0 is None else round(mem0 / 2**30, 2),
                          "container_gib_peak_sampled": round(max(samples) / 2**30, 2) if samples else None,
                          "this_run_gib": round((max(samples) - mem0) / 2**30, 2) if (samples and mem0 is not None) else None,
                          "sampled": "memory.current of the container after the model load and after every iteration (pinned weights + host KV caches + page cache)",
                          "cgroup_limit_gib": None if mem["max"] is None else round(mem["max"] / 2**30, 1),
                          "process_max_rss_gib": round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2**20, 2)}
    os.makedirs(os.path.dirname(os.path.abspath(args.result_json)), exist_ok=True)
    with open(args.result_json, "w") as f:
        json.dump(rec, f, indent=1, default=str)
    return rec.get("result")


def _main(args, rec=None):
    print(args)
    check_spec_sample_flags(args)
    if args.prompt is not None and args.prompt_file is not None:
        raise SystemExit("[ERROR] --prompt and --prompt-file exclude each other: one prompt for every row, or one per line of the file")
    if not args.benchmark:
        print("note: only the --benchmark protocol exists here; running it")
    # the reference's launch line is `OMP_NUM_THREADS=40 numactl -m 0 -C 0-39 python run.py ...` (README.md:78): host compute
    # on the node that holds the pinned weights / KV caches.  Here: the NUMA node of GPU 0 (LIA_PIN_NODE overrides, -1 = off).
    import os
    from . import hostinfo
    import torch
    if torch.cuda.is_available():
        node = hostinfo.pin_node(0)
        if node >= 0 and hostinfo.pin_to_node(node):
            print(f"host threads pinned to NUMA node {node}")
    if args.enable_cxl:
        nodes = choose_cxl_nodes(args.cxl_nodes)
        if nodes is not None:
            print(f"--enable-cxl: the NUMA tier interleaves over nodes {nodes}")
            if rec is not None:
                rec["cxl_nodes"] = nodes
    if rec is not None and not args.auto_plan:
        rec["planner_pick"] = plan_beside(args)
    if args.auto_plan and is_llama(args):
        raise SystemExit("[ERROR] --auto-plan plans OPT layers and the LIA policies; a Llama has no policy to plan (pick --gpu-percentage)")
    if args.auto_plan:
        pl = auto_plan(args)
        if rec is not None:
            rec["auto_plan"] = {"gpu_percentage": args.gpu_percentage, "prefill_policy": args.prefill_policy, "decoding_policy": args.decoding_policy,
                                "cpu_layers": args.cpu_layers, "cpu_layers_start": args.cpu_layers_start,
                                "predicted_prefill_ms": round(pl.prefill_ms, 1), "predicted_decode_tokens_per_s": round(pl.decode_tokens_per_s, 1)}
    t_load = time.time()
    model = load_model(args)
    if rec is not None:
        rec["model_load_s"] = round(time.time() - t_load, 1)
        from . import hostinfo as _hi
        rec["_mem_samples"].append(_hi.cgroup_memory()["current"])
    if args.stream_format is None:
        args.stream_format = default_stream_format()
    attach_scheduler(model, args.stream_format, args.split_decode)                  # generate() drives this scheduler
    if getattr(model, "family", "opt") == "llama":
        print(f"note: {model.shape.name} is a Llama: --prefill-policy / --decoding-policy have no counterpart (decoder.py:121-169); "
              f"gpu% {args.gpu_percentage} of the layers resident, the others streamed, every layer computed on the GPU")
    generate_kwargs = dict(do_sample=False, num_beams=1, max_new_tokens=args.max_new_tokens, min_new_tokens=args.max_new_tokens,
                           token_latency=args.token_latency, **lia_kwargs_of(args))
    generate_kwargs.update(sampling_kwargs(args))
    if args.cpu_layers:
        generate_kwargs["cpu_layers"] = args.cpu_layers
        if args.cpu_layers < 0 and args.cpu_layers_start is not None:
            generate_kwargs["cpu_layers_start"] = args.cpu_layers_start
    generate_kwargs.update(constraint_kwargs(args, model.shape.vocab))
    generate_kwargs.update(penalty_kwargs(args))
    spec_log = None
    if args.draft_model:
        spec_log = []
        generate_kwargs.update(draft=load_draft(args), draft_tokens=args.draft_tokens, spec_log=spec_log)
        if args.acceptance != "common":
            generate_kwargs.update(acceptance=args.acceptance)
        if args.sampled_verify:
            generate_kwargs.update(sampled_verify=True)
            if args.verify_rule != "draw":
                generate_kwargs.update(verify_rule=args.verify_rule)
    if args.logprobs is not None:
        if args.followup:
            raise SystemExit("[ERROR] --logprobs with --followup is not supported on the command line (generate(past=, logprobs=) serves it)")
        if args.profile:
            raise SystemExit("[ERROR] --logprobs with --profile is not supported: the profiled generate() keeps its own result layout")
        generate_kwargs["logprobs"] = args.logprobs
    tokenizer = load_tokenizer(args.model_id)
    if args.prompt_file is not None:
        input_ids, generate_kwargs["attention_mask"] = prompt_file_inputs(args, model.shape.vocab, tokenizer,
                                                                          generate_kwargs.get("pad_token_id", 1))
    else:
        input_ids = prompt_input_ids(args, model.shape.vocab, tokenizer)
    if args.followup:
        if args.prompt_file is not None:
            raise SystemExit("[ERROR] --followup with --prompt-file is not supported: one conversation, every row the same (--prompt)")
        return run_conversation(model, input_ids, followup_ids(args, model.shape.vocab, tokenizer), generate_kwargs, args, tokenizer)
    if args.profile and spec_log is not None:
        raise SystemExit("[ERROR] --profile with --draft-model is not supported: the profile brackets a prefill and single-token decode steps")
    if args.profile:
        profile_once(model, input_ids, generate_kwargs)
    total_time, total_list = 0.0, []
    sched = model._lia_scheduler
    for i in range(args.num_iter):
        if rec is not None and i == args.num_warmup and hasattr(sched, "stream_stats"):
            sched.stream_stats(reset=True)                     # the weight stream's bytes / copy-engine time over the timed iterations
        tic = time.time()
        # (not with a drafter: the brackets describe a prefill and single-token decode steps, and the first verify pass may move
        # to a larger workspace -- a new library context -- between them)
        if rec is not None and spec_log is None and args.logprobs is None and i == 0 and args.num_warmup >= 1 and hasattr(sched, "coop_report"):
            profile_once(model, input_ids, generate_kwargs, warm=False)       # the first warm-up iteration, bracketed
            output = profile_once.last[0]
            if not args.token_latency:
                output = output[0]
            rows = profile_once.last[1]
            rec["profile_of_warmup_iteration"] = {"rows": [list(r) for r in rows], "dominant_prefill": _dominant(rows, "prefill"),
                                                  "dominant_decode": _dominant(rows, "decode")}
        else:
            output = generate(model, input_ids, **generate_kwargs)
        gen_ids = output[0] if (args.token_latency or args.logprobs is not None) else output
        token_lp = output[-1] if args.logprobs is not None else None
        toc = time.time()
        total_new_tokens = [int(o.shape[0] - i_.shape[0]) for i_, o in zip(input_ids, gen_ids)]
        if tokenizer is not None and args.prompt is not None:                 # run_generation.py:321-323
            print(tokenizer.batch_decode(gen_ids, skip_special_tokens=True)[:1], total_new_tokens[:4], flush=True)
        if tokenizer is not None and args.prompt_file is not None:           # every row: the rows hold different prompts
            for b, text in enumerate(tokenizer.batch_decode(gen_ids[:, input_ids.shape[1]:], skip_special_tokens=True)):
                print(f"row {b}: {text!r}", flush=True)
        print(gen_ids[0, input_ids.shape[1]:].tolist(), total_new_tokens[:4], flush=True)
        if token_lp is not None and args.prompt is not None:
            print("\n".join(format_logprobs(token_lp, gen_ids[:, input_ids.shape[1]:], tokenizer)), flush=True)
        print("Iteration: %d, Time: %.6f sec" % (i, toc - tic), flush=True)
        if rec is not None:
            from . import hostinfo as _hi
            rec["_mem_samples"].append(_hi.cgroup_memory()["current"])
        if spec_log is not None and i < args.num_warmup:
            del spec_log[:]                                        # the acceptance figures are those of the timed iterations
        if i >= args.num_warmup:
            total_time += toc - tic
            if args.token_latency:
                total_list.append(output[1])
    res = summarize(total_time, args.num_iter, args.num_warmup, total_list, args.batch_size)
    if rec is not None and hasattr(sched, "stream_stats"):
        b, ms = sched.stream_stats()
        n_t = max(1, args.num_iter - args.num_warmup)
        rec["weight_stream"] = {"bytes_per_timed_iteration": b / n_t, "copy_engine_busy_ms_per_timed_iteration": round(ms / n_t, 1),
                                "gbs_while_busy": round(b / max(ms, 1e-9) / 1e6, 2), "gbs_over_wall": round(b / max(total_time, 1e-9) / 1e9, 2),
                                "fraction_of_63_gbs_link_over_wall": round(b / max(total_time, 1e-9) / 63e9, 3),
                                "wire_format": ("pack10" if any(getattr(st, "packed", 0) for st in model.layers) else "raw"),
                                "wire_format_note": "the format of the host copies that streamed (a policy-1 / NUMA-tier / unpinned placement ships raw: scheduler.placement_formats)"}
    if args.logprobs is not None:                                  # the last iteration's arrays
        res["logprobs"] = {"n_top": args.logprobs, "token_logprobs": token_lp.token_logprobs.tolist(), "top_ids": token_lp.top_ids.tolist(),
                           "top_logprobs": token_lp.top_logprobs.tolist(), "sequence_logprob": token_lp.sequence_logprob().tolist()}
    if spec_log is not None:
        # (with a drafter a latency entry is a target pass of several tokens: "Average 2... latency" above is per pass)
        res["speculative"] = summarize_speculation(spec_log, total_list, args.batch_size, acceptance=args.acceptance)
    if "decode_tokens_per_s" in res:
        print("Decode throughput: %.2f tokens/s, prefill %.1f ms" % (res["decode_tokens_per_s"], res["prefill_ms"]))
    coop = getattr(model._lia_scheduler, "coop_report", lambda: None)()
    if coop:
        print("Cooperative split (online): %d host-computed decode layers, ms per step by count %s" % (coop["host_layers"], coop["ms_by_count"]))
    return res


if __name__ == "__main__":
    main()
