"""ctypes signatures of the ragged-cache launchers and entry points (per-row acceptance of speculative decoding) that the GPU tests call
directly.  Source: isca-2025-lia_amd/csrc/lia_internal.h and include/lia_hip.h."""
import ctypes

vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long

_ATTN = [vp, cl, vp, vp, vp, cl]            # q, ldq, kc, vc, out, ldo

# name -> (restype, argtypes); the trailing vp of each is the hipStream_t
SIGNATURES = {
    # B, T, pos0, heads, kv_heads, d, Bc, b0, post_scale, starts (or NULL), stream
    "lia_attn_block_launch": (ci, _ATTN + [ci] * 9 + [vp, vp]),
    # B, T, max_len, heads, kv_heads, d, Bc, b0, post_scale, starts (or NULL), lens, stream
    "lia_attn_block_ragged_launch": (ci, _ATTN + [ci] * 9 + [vp, vp, vp]),
    # ksrc, vsrc, kc, vc, B, T, H, Bc, b0, lens, stream
    "lia_kv_scatter_ragged_launch": (None, [vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, vp]),
}


def bind(lib):
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib
