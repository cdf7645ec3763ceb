"""Accuracy harness: counterpart of llm/single_instance/run_accuracy.py (reference :384-495, the loglikelihood and
loglikelihood_rolling requests of its lm_eval adapter), on scoring.py.  No dataset is downloaded by anything: the texts or token
ids come from a local file.

    python run_accuracy.py -m DIR --tokens-file ids.npy  --prefill-policy 0 --gpu-percentage 10 --pin-weight
        -> word-free perplexity exp(-sum of the tokens' log-probabilities / number of tokens), rolling windows of --max-len targets
    python run_accuracy.py -m DIR --pairs-file pairs.jsonl --batch-size 8
        -> accuracy (the share of requests whose continuation is the greedy one throughout) and perplexity
           exp(-mean log-likelihood of a continuation), as the lambada task reports them

--tokens-file: a .npy of token ids, or a text file when the -m directory ships its tokenizer.  --pairs-file: JSON lines of
{"context": ..., "continuation": ...}, each either a list of ids or (with a tokenizer) a string.
"""
import argparse
import json
import math
import os
import sys
import time

os.environ.setdefault("OMP_WAIT_POLICY", "PASSIVE")      # as run.py: before the first libgomp load
os.environ.setdefault("GOMP_SPINCOUNT", "0")


def build_parser():
    from . import run_generation as rg
    p = argparse.ArgumentParser("Accuracy script (bf16 path, MI355X)", add_help=True)
    rg.add_model_args(p)
    rg.add_lia_args(p)
    rg.add_stream_format_arg(p)
    rg.add_init_args(p)
    p.add_argument("--batch-size", default=1, type=int, help="rows per scoring pass")
    p.add_argument("--tokens-file", default=None, type=str, help="a .npy of token ids, or a text file (needs the tokenizer files in the -m directory)")
    p.add_argument("--pairs-file", default=None, type=str, help='JSON lines of {"context": ids or text, "continuation": ids or text}')
    p.add_argument("--max-len", default=None, type=int,
                   help="--tokens-file: targets per rolling window (default: max positions - 1); --pairs-file: tokens kept of a request, from the right (default: max positions)")
    p.add_argument("--prefix-token", default=None, type=int,
                   help="--tokens-file: the token the first window is conditioned on (default: the tokenizer's BOS / EOS, else 2)")
    p.add_argument("--result-json", default=None, type=str, help="write one JSON record of the run to this path: flags, counts, the numbers")
    p.set_defaults(cpu_layers=0)
    return p


def check_args(args):
    """the argument errors, by name, before anything is loaded"""
    if (args.tokens_file is None) == (args.pairs_file is None):
        raise SystemExit("[ERROR] exactly one of --tokens-file and --pairs-file must be given")
    path = args.tokens_file or args.pairs_file
    if not os.path.isfile(path):
        raise SystemExit(f"[ERROR] {'--tokens-file' if args.tokens_file else '--pairs-file'} {path!r} does not exist")
    if args.batch_size < 1:
        raise SystemExit(f"[ERROR] --batch-size {args.batch_size} must be >= 1")
    if args.max_len is not None and args.max_len < (1 if args.tokens_file else 2):
        raise SystemExit(f"[ERROR] --max-len {args.max_len} must be >= {1 if args.tokens_file else 2}")


def _need_tokenizer(tokenizer, args, what):
    if tokenizer is None:
        from .run_generation import TOKENIZER_FILES
        raise SystemExit(f"[ERROR] {what} needs a tokenizer: point -m at a checkpoint directory that ships its tokenizer files "
                         f"({', '.join(TOKENIZER_FILES[:3])}); {args.model_id!r} has none")


def _check_ids(ids, vocab, what):
    if not ids or min(ids) < 0 or max(ids) >= vocab:
        raise SystemExit(f"[ERROR] {what}: empty, or ids outside the model's vocabulary of {vocab} entries")
    return ids


def read_tokens(args, vocab, tokenizer):
    """(token ids, prefix token) of --tokens-file"""
    import numpy as np
    prefix = args.prefix_token
    if args.tokens_file.endswith(".npy"):
        ids = [int(t) for t in np.load(args.tokens_file).reshape(-1)]
    else:
        _need_tokenizer(tokenizer, args, "a text --tokens-file")
        with open(args.tokens_file, encoding="utf-8") as f:
            ids = [int(t) for t in tokenizer(f.read(), add_special_tokens=False).input_ids]
    if prefix is None and tokenizer is not None:
        prefix = tokenizer.bos_token_id if tokenizer.bos_token_id is not None else tokenizer.eos_token_id
    prefix = 2 if prefix is None else int(prefix)
    _check_ids([prefix], vocab, "--prefix-token")
    return _check_ids(ids, vocab, "--tokens-file"), prefix


def read_pairs(args, vocab, tokenizer):
    """[(context ids, continuation ids)] of --pairs-file"""
    pairs = []
    with open(args.pairs_file, encoding="utf-8") as f:
        for n, line in enumerate(f, 1):
            if not line.strip():
                continue
            try:
                rec = json.loads(line)
                sides = [rec["context"], rec["continuation"]]
            except (ValueError, KeyError, TypeError):
                raise SystemExit(f'[ERROR] --pairs-file line {n}: expected a JSON object with "context" and "continuation"') from None
            for k, side in enumerate(sides):
                if isinstance(side, str):
                    _need_tokenizer(tokenizer, args, "a --pairs-file with text")
                    # the context as the tokenizer writes a prompt (its BOS included), the continuation bare
                    side = tokenizer(side, add_special_tokens=(k == 0)).input_ids
                sides[k] = _check_ids([int(t) for t in side], vocab, f"--pairs-file line {n}")
            pairs.append(tuple(sides))
    if not pairs:
        raise SystemExit(f"[ERROR] --pairs-file {args.pairs_file!r} holds no request")
    return pairs


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_args(args)
    print(args)
    from . import run_generation as rg
    from . import scoring
    model = rg.load_model(args)
    if args.stream_format is None:
        args.stream_format = rg.default_stream_format()
    rg.attach_scheduler(model, args.stream_format)
    tokenizer = rg.load_tokenizer(args.model_id)
    lia = rg.lia_kwargs_of(args)
    vocab = model.shape.vocab
    rec = {"flags": {k: v for k, v in vars(args).items() if k != "result_json"}}
    t0 = time.time()
    if args.tokens_file is not None:
        ids, prefix = read_tokens(args, vocab, tokenizer)
        ll = scoring.loglikelihood_rolling(model, ids, prefix, max_len=args.max_len, batch_size=args.batch_size, **lia)
        rec["counts"] = {"tokens": len(ids), "prefix_token": prefix,
                         "windows": len(scoring.rolling_windows(ids, prefix, args.max_len or model.shape.max_pos - 1))}
        rec["result"] = {"loglikelihood": ll, "perplexity": math.exp(-ll / len(ids))}
        print("tokens: %d  log-likelihood: %.4f  perplexity: %.4f" % (len(ids), ll, rec["result"]["perplexity"]))
    else:
        pairs = read_pairs(args, vocab, tokenizer)
        res = scoring.loglikelihood(model, pairs, batch_size=args.batch_size, max_len=args.max_len, **lia)
        acc = sum(1 for _, g in res if g) / len(res)
        mean_ll = sum(v for v, _ in res) / len(res)
        rec["counts"] = {"requests": len(res), "continuation_tokens": sum(len(c) for _, c in pairs)}
        rec["result"] = {"accuracy": acc, "perplexity": math.exp(-mean_ll), "mean_loglikelihood": mean_ll}
        print("requests: %d  accuracy: %.4f  perplexity: %.4f" % (len(res), acc, rec["result"]["perplexity"]))
    rec["wall_s"] = round(time.time() - t0, 2)
    if args.result_json:
        os.makedirs(os.path.dirname(os.path.abspath(args.result_json)), exist_ok=True)
        with open(args.result_json, "w") as f:
            json.dump(rec, f, indent=1, default=str)
    sched = getattr(model, "_lia_scheduler", None)
    if sched is not None:
        sched.close()
    model.close()
    return rec["result"]


if __name__ == "__main__":
    main(sys.argv[1:])
