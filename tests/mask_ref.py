"""NumPy restatement of the allowed-token masks (include/lia_hip.h, lia_ctx_set_token_mask) for the constrained-decoding tests:
the packed layout through np.packbits, the first argmax over the allowed entries, and the -inf substitution of the defining
identity -- a masked head call gives what the same call without a table gives on logits whose disallowed entries are bf16 -inf.
Also the ctypes signatures of the masked kernel launchers (isca-2025-lia_amd/csrc/lia_internal.h) that the kernel tests call."""
import ctypes

import numpy as np

vp, ci, cl, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float

# name -> (restype, argtypes); the trailing vp of each is the hipStream_t
LAUNCHERS = {
    "lia_argmax_launch": (None, [vp, vp, ci, ci, ci, vp]),
    "lia_argmax_masked_launch": (None, [vp, vp, ci, ci, ci, vp, cl, vp]),
    # logits, ld, n, vocab, suppress, n_suppress, n_suppress_rows, T, r0, greedy[, mask, ldm], stream
    "lia_verify_argmax_rows_launch": (None, [vp, cl, ci, ci, ci, ci, vp, ci, ci, vp, vp]),
    "lia_verify_argmax_masked_launch": (None, [vp, cl, ci, ci, ci, ci, vp, ci, ci, vp, vp, cl, vp]),
    "lia_verify_accept_launch": (None, [vp, vp, vp, ci, ci, vp, vp, vp, vp]),
    # logits, ld, n, vocab, tau, top_k, top_p, suppress, n_suppress, n_suppress_rows, T, r0, uniforms, ldu, n_steps, step0, step_rows,
    # block_ids, sampled, p_draft[, mask, ldm], stream
    "lia_verify_sample_launch": (None, [vp, cl, ci, ci, cf, ci, cf, ci, ci, vp, ci, ci, vp, cl, ci, ci, vp, vp, vp, vp, vp]),
    "lia_verify_sample_masked_launch": (None, [vp, cl, ci, ci, cf, ci, cf, ci, ci, vp, ci, ci, vp, cl, ci, ci, vp, vp, vp, vp, vp, cl, vp]),
}


def bind(lib):
    for name, (res, args) in LAUNCHERS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def words(vocab):
    return (vocab + 31) // 32


def pack(allowed):
    """allowed bool [..., vocab] -> int32 [..., W]: token i is bit i & 31 of word i >> 5 (little endian: tokens 8j .. 8j + 7 are byte j)"""
    allowed = np.asarray(allowed, bool)
    vocab = allowed.shape[-1]
    by = np.packbits(allowed, axis=-1, bitorder="little")
    pad = 4 * words(vocab) - by.shape[-1]
    if pad:
        by = np.concatenate([by, np.zeros(by.shape[:-1] + (pad,), np.uint8)], axis=-1)
    return np.ascontiguousarray(by).view("<i4")


def unpack(mask, vocab):
    """int32 [..., W] -> bool [..., vocab]; bits at and beyond vocab are dropped"""
    by = np.ascontiguousarray(np.asarray(mask, "<i4")).view(np.uint8)
    return np.unpackbits(by, axis=-1, bitorder="little")[..., :vocab].astype(bool)


def first_argmax(logits_f32, allowed, suppress=-1):
    """per row the first maximal index among the allowed entries; suppress: a token id (or -1) for every row, or one per row"""
    lg = np.array(logits_f32, np.float32, copy=True)
    lg[~np.asarray(allowed, bool)] = -np.inf
    sup = np.broadcast_to(np.asarray(suppress, np.int64), (lg.shape[0],))
    for r in np.flatnonzero(sup >= 0):
        lg[r, sup[r]] = -np.inf
    return np.argmax(lg, axis=-1).astype(np.int64)          # (np.argmax returns the first of equal maxima)


def substitute(torch, logits, allowed):
    """a copy of bf16 logits [n, vocab] (torch, any device) with bf16 -inf at the disallowed entries"""
    out = logits.clone()
    out[torch.from_numpy(~np.asarray(allowed, bool)).to(out.device)] = float("-inf")
    return out
