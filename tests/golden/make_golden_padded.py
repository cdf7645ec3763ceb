#!/usr/bin/env python3
"""Golden vectors of a LEFT-PADDED batch, by executing the reference's own CPU branch (needs the reference tree; the GPU box never
runs this, only the .npz it writes is read).  Same recipe as make_golden.py, whose helpers it reuses:

  * OPTLearnedPositionalEmbedding (lia/modeling_opt.py:357-378) on the padded 2-D mask, for the prefill and two decode steps
    (the mask extended by a one per generated token): the position INDICES (a weight table whose row r holds r);
  * OPTDecoderLayer_forward(policy=1) (decoder.py:172, its CPU branch: nn.LayerNorm, nn.Linear q/k/v, _IPEXScaleDotProductRef
    mha_fusion.py:532-566, the fused linears) on a prefill with the 4-D additive causal + padding mask OPTDecoder.forward builds
    (lia/modeling_opt.py:1133: finfo.min where key j > query i or column j is padding), then two decode steps whose [B,1,1,S+1]
    masks carry finfo.min at the pad columns.

Written: padded_layer_h128.npz -- cfg, w_std, starts, pos_prefill [B,T], pos_dec [new,B], p1_hidden [B,T,H] (the pad query rows
are the reference's uniform average over an all-masked row: not compared), p1_dec{s}_hidden, p1_kcache / p1_vcache [S,B,h,d].
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402
import synth  # noqa: E402


def reference_positional_embedding():
    spec = importlib.util.spec_from_file_location("transformers.models.opt.lia_ref_modeling_opt",
                                                  os.path.join(G.REF, "lia", "modeling_opt.py"))
    mod = importlib.util.module_from_spec(spec)
    mod.__package__ = "transformers.models.opt"
    na = types.ModuleType("transformers.models.opt.numa_alloc")
    na.numa_alloc_tensor = na.numa_free_tensor = None
    sys.modules["transformers.models.opt.numa_alloc"] = na
    spec.loader.exec_module(mod)
    return mod.OPTLearnedPositionalEmbedding


def run_padded_case(dec, att, mha, name, H, heads, F, starts, T, new, seed, w_std):
    B = len(starts)
    starts = np.asarray(starts, np.int64)
    mask2d = torch.from_numpy((np.arange(T)[None, :] >= starts[:, None]).astype(np.int64))
    out = {"cfg": np.array([H, heads, F, B, T, new, seed, 0], dtype=np.int64), "w_std": np.array([w_std], dtype=np.float64),
           "starts": starts.astype(np.int32)}
    PE = reference_positional_embedding()
    pe = PE(T + new + 2, 1)
    with torch.no_grad():
        pe.weight.copy_(torch.arange(T + new + 4, dtype=torch.float32)[:, None])
        out["pos_prefill"] = pe(mask2d, 0)[..., 0].long().numpy()
        dec_pos = []
        for s in range(new):
            m = torch.cat([mask2d, torch.ones(B, s + 1, dtype=torch.int64)], 1)
            dec_pos.append(pe(m, T + s)[:, 0, 0].long().numpy())
        out["pos_dec"] = np.stack(dec_pos)

    W = synth.make_layer(seed, H, F, w_std)
    x = G.bits_to_torch(synth.make_hidden(seed + 1, B, T, H, False))
    neg = torch.finfo(torch.bfloat16).min
    j = torch.arange(T)
    with G.CudaToCpu(), torch.no_grad():
        layer1, _ = G.fake_layer(dec, att, mha, W, H, heads, 1)
        hidden = (j[None, :] > j[:, None])[None] | (mask2d[:, None, :] == 0)          # [B, T(query), T(key)]
        cm = torch.where(hidden, torch.tensor(neg, dtype=torch.bfloat16), torch.tensor(0.0, dtype=torch.bfloat16))[:, None]
        o = dec.OPTDecoderLayer_forward(layer1, x.clone(), attention_mask=cm.contiguous(), past_key_value=None,
                                        use_cache=True, policy=1, max_new_tokens=new)
        out["p1_hidden"] = G.torch_to_bits(o[0])
        past = o[1]
        for s in range(new):
            xs = G.bits_to_torch(synth.make_hidden(seed + 100 + s, B, 1, H, False))
            cols = torch.cat([mask2d, torch.ones(B, s + 1, dtype=torch.int64)], 1)
            dm = torch.where(cols == 0, torch.tensor(neg, dtype=torch.bfloat16), torch.tensor(0.0, dtype=torch.bfloat16))[:, None, None]
            o = dec.OPTDecoderLayer_forward(layer1, xs, attention_mask=dm.contiguous(), past_key_value=past,
                                            use_cache=True, policy=1, max_new_tokens=new)
            out[f"p1_dec{s}_hidden"] = G.torch_to_bits(o[0])
            past = o[1]
        out["p1_kcache"] = G.torch_to_bits(past[0].permute(2, 0, 1, 3))
        out["p1_vcache"] = G.torch_to_bits(past[1].permute(2, 0, 1, 3))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("wrote", name, {k: v.shape for k, v in out.items()})


def main():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    dec, att, mha = G.import_reference()
    # name, H, heads, F, starts (one row unpadded, one with a single real token), T, new, seed, w_std
    run_padded_case(dec, att, mha, "padded_layer_h128", 128, 4, 512, [0, 3, 7, 1], 8, 2, 41, 0.12)
    run_padded_case(dec, att, mha, "padded_layer_h256_d64", 256, 4, 1024, [5, 0, 12], 13, 2, 42, 0.08)


if __name__ == "__main__":
    main()
