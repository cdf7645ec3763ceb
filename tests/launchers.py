"""The ctypes binding of the kernels' host launchers that the GPU tests call directly: the one place in tests/ that restates their
signatures.  Source: isca-2025-lia_amd/csrc/lia_internal.h (the launchers are extern "C"; the library itself checks every definition
and call against that header at compile time -- a change there is repeated here and nowhere else)."""
import ctypes

vp, ci, cl, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float

_ATTN = [vp, cl, vp, vp, vp, cl]            # q, ldq, kc, vc, out, ldo
_SHAPE = [ci] * 8                           # B, T (prefill) / S (decode), heads, kv_heads, d, Bc, b0, post_scale

# name -> (restype, argtypes); the trailing vp of each is the hipStream_t
SIGNATURES = {
    "lia_layernorm_launch": (None, [vp, cl, vp, vp, vp, cl, cl, ci, cf, vp]),
    "lia_rmsnorm_launch": (None, [vp, cl, vp, vp, cl, cl, ci, cf, vp]),
    "lia_rope_launch": (None, [vp, cl, vp, vp, cl, ci, ci, ci, ci, ci, vp]),
    "lia_silu_mul_launch": (None, [vp, vp, cl, ci, ci, vp]),
    "lia_argmax_launch": (None, [vp, vp, ci, ci, ci, vp]),
    "lia_attn_prefill_launch": (ci, _ATTN + _SHAPE + [vp]),
    "lia_attn_decode_launch": (ci, _ATTN + _SHAPE + [vp]),
    "lia_attn_prefill_padded_launch": (ci, _ATTN + _SHAPE + [vp, vp]),          # ..., starts, stream
    "lia_attn_decode_padded_launch": (ci, _ATTN + _SHAPE + [vp, vp]),
    "lia_attn_append_launch": (ci, _ATTN + [ci] * 9 + [vp, vp]),                # B, T, pos0, heads, ..., starts (or NULL), stream
}


def bind(lib):
    """set restype / argtypes of every launcher above on the loaded library; -> lib"""
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib
