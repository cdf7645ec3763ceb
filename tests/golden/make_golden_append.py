#!/usr/bin/env python3
"""Golden vectors of a block appended to a live cache, by executing the reference's own CPU branch (needs the reference tree; the GPU
box never runs this, only the .npz it writes is read).  Same recipe as make_golden.py / make_golden_padded.py, whose helpers it
reuses: OPTDecoderLayer_forward(policy=1) (decoder.py:172: nn.LayerNorm, nn.Linear q/k/v, _IPEXScaleDotProductRef
mha_fusion.py:532-566, the fused linears) on a prefill of P tokens with the 4-D additive causal mask, then on a block of T tokens
with that call's past_key_value and the [B, 1, T, P + T] mask OPTDecoder.forward builds for a multi-token call with a past
(finfo.min where key j > P + query t).

Written: append_layer_h128.npz -- cfg [H, heads, F, B, P, T, seed], w_std, p1_prefill_hidden [B, P, H], p1_block_hidden [B, T, H],
p1_kcache / p1_vcache [P + T, B, h, d]."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402
import synth  # noqa: E402


def causal(T, P):
    """[1, 1, T, P + T] additive mask of T queries at positions P .. P + T - 1"""
    neg = torch.finfo(torch.bfloat16).min
    hidden = torch.arange(P + T)[None, :] > (P + torch.arange(T))[:, None]
    return torch.where(hidden, torch.tensor(neg, dtype=torch.bfloat16), torch.tensor(0.0, dtype=torch.bfloat16))[None, None]


def run_append_case(dec, att, mha, name, H, heads, F, B, P, T, seed, w_std):
    out = {"cfg": np.array([H, heads, F, B, P, T, seed], dtype=np.int64), "w_std": np.array([w_std], dtype=np.float64)}
    W = synth.make_layer(seed, H, F, w_std)
    x0 = G.bits_to_torch(synth.make_hidden(seed + 1, B, P, H, False))
    x1 = G.bits_to_torch(synth.make_hidden(seed + 2, B, T, H, False))
    with G.CudaToCpu(), torch.no_grad():
        layer1, _ = G.fake_layer(dec, att, mha, W, H, heads, 1)
        o = dec.OPTDecoderLayer_forward(layer1, x0.clone(), attention_mask=causal(P, 0).expand(B, -1, -1, -1).contiguous(),
                                        past_key_value=None, use_cache=True, policy=1, max_new_tokens=T)
        out["p1_prefill_hidden"] = G.torch_to_bits(o[0])
        o = dec.OPTDecoderLayer_forward(layer1, x1.clone(), attention_mask=causal(T, P).expand(B, -1, -1, -1).contiguous(),
                                        past_key_value=o[1], use_cache=True, policy=1, max_new_tokens=T)
        out["p1_block_hidden"] = G.torch_to_bits(o[0])
        out["p1_kcache"] = G.torch_to_bits(o[1][0].permute(2, 0, 1, 3))
        out["p1_vcache"] = G.torch_to_bits(o[1][1].permute(2, 0, 1, 3))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, {k: v.shape for k, v in out.items()})


def main():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    dec, att, mha = G.import_reference()
    run_append_case(dec, att, mha, "append_layer_h128", 128, 4, 512, 3, 7, 5, 43, 0.12)      # a 5-token block over a 7-token cache


if __name__ == "__main__":
    main()
