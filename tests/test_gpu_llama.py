"""-m gpu parity of the Llama-family layer (config 4, build-defined) through the C ABI: against the CPU oracle and the
HF-eager goldens (tests/golden/llama_*.npz); end-to-end greedy ids bit-exact, resident and streamed weights."""
import ctypes
import glob
import os

import numpy as np
import pytest

import launchers
import synth
from test_gpu_ops import assert_close, to_bits, to_dev

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LAYER_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "llama_layer_*.npz")))


@pytest.mark.parametrize("name", LAYER_CASES)
def test_llama_layer_forward(oracle, name):
    import torch
    from lia_amd import _native as N, ops
    from lia_amd.llama import LiaLlamaModel, LlamaShape, rope_tables
    z = np.load(os.path.join(GOLD, name + ".npz"))
    H, heads, kvh, F, B, T, new, seed = [int(v) for v in z["cfg"]]
    m = synth.make_llama_model(seed, 64, H, heads, kvh, F, 1, float(z["w_std"][0]))
    shape = LlamaShape("t", H, heads, kvh, F, 1, 64, max_pos=T + new + 4, rope_theta=float(z["theta"][0]))
    model = LiaLlamaModel.from_numpy(shape, m)
    model.place(1, True, False)
    d = H // heads
    lib = N.lib()
    ctx = ops.Context(0, max(lib.lia_llama_workspace_bytes(ctypes.byref(model.desc), B * T), 1 << 24))
    cos, sin = rope_tables(T + new + 4, d, shape.rope_theta)
    ocos, osin = oracle.rope_tables(T + new + 4, d, shape.rope_theta)
    assert (to_bits(cos) == ocos).all() and (to_bits(sin) == osin).all()
    kc = torch.zeros((T + new, B, kvh, d), dtype=torch.bfloat16, device="cuda")
    vc = torch.zeros_like(kc)
    kv = N.KV(kc.data_ptr(), vc.data_ptr(), T + new, B, 1)
    w = (ctypes.c_void_p * 9)(*[model.layers[0].device_ptr() + o for o in model.offsets])
    fin = lambda t: oracle.rmsnorm(to_bits(t), m["final_norm_w"])  # noqa: E731  (goldens include HF's final norm)

    def run(xbits, Tn, pos0):
        x = to_dev(torch, xbits)
        y = torch.empty_like(x)
        N.check(lib.lia_llama_layer_forward(ctx.handle, ctypes.byref(model.desc), ctypes.byref(w), ctypes.c_void_p(x.data_ptr()),
                                            ctypes.c_void_p(y.data_ptr()), ctypes.byref(kv), ctypes.c_void_p(cos.data_ptr()),
                                            ctypes.c_void_p(sin.data_ptr()), B, Tn, pos0, 0, ctypes.c_void_p(ctx.stream)))
        ctx.synchronize()
        return y

    y = run(synth.make_hidden(seed + 1, B, T, H), T, 0)
    assert_close(fin(y), z["prefill_hidden"], 0.07, 0.016, 0.75, "llama prefill vs HF")
    okc, ovc = np.zeros((T + new, B, kvh, d), np.uint16), np.zeros((T + new, B, kvh, d), np.uint16)
    oy = oracle.llama_layer_forward(m["layers"][0], synth.make_hidden(seed + 1, B, T, H), okc, ovc, ocos, osin, 0, heads, kvh)
    assert_close(to_bits(y), oy, 0.07, 0.016, 0.75, "llama prefill vs oracle")
    for s in range(new):
        ys = run(synth.make_hidden(seed + 100 + s, B, 1, H), 1, T + s)
        assert_close(fin(ys), z[f"dec{s}_hidden"], 0.07, 0.016, 0.7, f"llama decode {s} vs HF")
    assert_close(to_bits(kc), z["kcache"], 0.03, 0.008, 0.95, "post-RoPE K cache")
    assert_close(to_bits(vc), z["vcache"], 0.03, 0.008, 0.95, "V cache")
    ctx.close()
    model.close()


@pytest.mark.parametrize("fmt", ["raw", "pack10"])
@pytest.mark.parametrize("gpu_pct,mb", [(100, 1), (34, 1), (0, 2)])
def test_llama_generate_ids_match_hf(gpu_pct, mb, fmt, monkeypatch):
    import torch
    monkeypatch.setenv("LIA_STREAM_FORMAT", fmt)
    if fmt != "raw" and gpu_pct >= 100:
        pytest.skip("nothing is streamed")
    from lia_amd.generation import generate
    from lia_amd.llama import LiaLlamaModel, LlamaShape
    z = np.load(os.path.join(GOLD, "llama_generate_h256.npz"))
    vocab, H, heads, kvh, F, L, B, T, new, seed = [int(v) for v in z["cfg"]]
    m = synth.make_llama_model(seed, vocab, H, heads, kvh, F, L, float(z["w_std"][0]))
    ids = synth.make_prompt_ids(seed + 1, B, T, vocab)
    shape = LlamaShape("t", H, heads, kvh, F, L, vocab, max_pos=64, rope_theta=float(z["theta"][0]))
    model = LiaLlamaModel.from_numpy(shape, m)
    out, lat = generate(model, torch.from_numpy(ids), max_new_tokens=new, min_new_tokens=new, token_latency=True,
                        gpu_percentage=gpu_pct, num_minibatch=mb, pin_weight=True)
    assert (out.numpy() == z["ids_bf16"]).all(), (out[0, T:].tolist(), z["ids_bf16"][0, T:].tolist())
    if fmt != "raw":
        n_gpu = int(L * gpu_pct / 100)
        assert all(st.packed == 10 for st in model.layers[n_gpu:])      # the streamed layers really travel encoded
    model._lia_scheduler.close()
    model.close()


@pytest.mark.parametrize("B,S,kvh", [(3, 1, 2), (5, 127, 2), (2, 128, 1), (16, 129, 2), (128, 1037, 8), (7, 2050, 3)])
def test_grouped_decode_attention_d128(B, S, kvh, oracle):
    """lia_attn_decode_kernel<128, 4> (four query heads per K/V head, the DPP row sum of q.k) at sizes up to Llama-3-8B's decode
    step, against a plain fp32 restatement of HF's eager grouped attention at one query position."""
    import torch
    from lia_amd import _native as N, ops
    lib = launchers.bind(N.lib())
    ctx = ops.Context(0, 1 << 20)
    G, d = 4, 128
    heads = kvh * G
    g = torch.Generator(device="cuda").manual_seed(B * 977 + S)
    q = (1.5 * torch.randn((B, heads * d), generator=g, device="cuda")).to(torch.bfloat16)
    kc = (1.5 * torch.randn((S + 3, B, kvh, d), generator=g, device="cuda")).to(torch.bfloat16)
    vc = torch.randn((S + 3, B, kvh, d), generator=g, device="cuda").to(torch.bfloat16)
    out = torch.zeros_like(q)
    torch.cuda.synchronize()          # torch filled q / k / v / out on ITS stream; the kernel runs on the context's
    rc = lib.lia_attn_decode_launch(q.data_ptr(), heads * d, kc.data_ptr(), vc.data_ptr(), out.data_ptr(), heads * d, B, S, heads, kvh, d,
                                    B, 0, 1, ctypes.c_void_p(ctx.stream))
    assert rc == 0
    ctx.synchronize()
    # post_scale = 1 (Llama): scores = bf16(bf16(q.k) * d^-0.5), softmax in fp32 rounded to bf16, P.V rounded to bf16
    qf = q.float().view(B, kvh, G, d)
    kf, vf = kc[:S].float().permute(1, 2, 0, 3), vc[:S].float().permute(1, 2, 0, 3)          # [B, kvh, S, d]
    s = torch.einsum("bhgd,bhsd->bhgs", qf, kf).to(torch.bfloat16).float() * (d ** -0.5)
    p = torch.softmax(s.to(torch.bfloat16).float(), dim=-1).to(torch.bfloat16).float()
    ref = torch.einsum("bhgs,bhsd->bhgd", p, vf).reshape(B, heads * d)
    err = (out.float() - ref).abs()
    assert float(err.max()) <= 0.02 + 0.016 * float(ref.abs().max()), float(err.max())
    # ... and against oracle/'s restatement of the same attention (lia_oracle_attn_gqa), same rounding points: almost every output
    # bit-identical, none further than one bf16 quantum of the largest
    ob = oracle.attention_gqa(to_bits(q).reshape(B, 1, heads * d), to_bits(kc), to_bits(vc), S, heads, kvh)
    gb = to_bits(out).reshape(B, 1, heads * d)
    of, gf = synth.bf16_bits_to_f32(ob), synth.bf16_bits_to_f32(gb)
    quantum = 2.0 ** (np.floor(np.log2(np.abs(of).max())) - 7)
    assert np.abs(of - gf).max() <= quantum and (ob == gb).mean() >= 0.99, (float(np.abs(of - gf).max()), float((ob == gb).mean()))
    ctx.close()


@pytest.mark.parametrize("name", LAYER_CASES[:1])
def test_llama_layer_forward_last_equals_last_position(oracle, name):
    """lia_llama_layer_forward_last (the prefill's last layer: norm, q|k|v and RoPE on every row, the rest on the last position):
    caches bit-identical to the full call, last position's hidden state equal to rounding."""
    import torch
    from lia_amd import _native as N, ops
    from lia_amd.llama import LiaLlamaModel, LlamaShape, rope_tables
    z = np.load(os.path.join(GOLD, name + ".npz"))
    H, heads, kvh, F, B, T, new, seed = [int(v) for v in z["cfg"]]
    m = synth.make_llama_model(seed, 64, H, heads, kvh, F, 1, float(z["w_std"][0]))
    shape = LlamaShape("t", H, heads, kvh, F, 1, 64, max_pos=T + 4, rope_theta=float(z["theta"][0]))
    model = LiaLlamaModel.from_numpy(shape, m)
    model.place(1, True, False)
    d = H // heads
    lib = N.lib()
    ctx = ops.Context(0, max(lib.lia_llama_workspace_bytes(ctypes.byref(model.desc), B * T), 1 << 24))
    cos, sin = rope_tables(T + 4, d, shape.rope_theta)
    w = (ctypes.c_void_p * 9)(*[model.layers[0].device_ptr() + o for o in model.offsets])
    x = to_dev(torch, synth.make_hidden(seed + 1, B, T, H))
    outs = []
    for fn, shp in ((lib.lia_llama_layer_forward, (B, T, H)), (lib.lia_llama_layer_forward_last, (B, 1, H))):
        kc = torch.zeros((T, B, kvh, d), dtype=torch.bfloat16, device="cuda")
        vc = torch.zeros_like(kc)
        kv = N.KV(kc.data_ptr(), vc.data_ptr(), T, B, 1)
        y = torch.empty(shp, dtype=torch.bfloat16, device="cuda")
        N.check(fn(ctx.handle, ctypes.byref(model.desc), ctypes.byref(w), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()),
                   ctypes.byref(kv), ctypes.c_void_p(cos.data_ptr()), ctypes.c_void_p(sin.data_ptr()), B, T, 0, 0, ctypes.c_void_p(ctx.stream)))
        ctx.synchronize()
        outs.append((y, kc, vc))
    (yf, kf, vf), (yl, kl, vl) = outs
    assert torch.equal(kf.view(torch.int16), kl.view(torch.int16)) and torch.equal(vf.view(torch.int16), vl.view(torch.int16))
    assert_close(to_bits(yl)[:, 0], to_bits(yf)[:, -1], 0.07, 0.016, 0.75, "llama last-only vs full prefill")
    ctx.close()
    model.close()


def _write_hf_llama(path, m, cfg, shards=2):
    """synth.make_llama_model's dict as a HF LlamaForCausalLM directory: config.json + `shards` safetensors files"""
    import json
    import torch
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    json.dump(dict(architectures=["LlamaForCausalLM"], model_type="llama", hidden_size=cfg["H"], num_attention_heads=cfg["heads"],
                   num_key_value_heads=cfg["kvh"], intermediate_size=cfg["F"], num_hidden_layers=cfg["L"], vocab_size=cfg["vocab"],
                   max_position_embeddings=64, rope_theta=cfg["theta"], rms_norm_eps=1e-5, torch_dtype="bfloat16", tie_word_embeddings=False),
              open(os.path.join(path, "config.json"), "w"))
    t = lambda bits: torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16).clone()      # noqa: E731
    hf = {"in_norm_w": "input_layernorm", "q_w": "self_attn.q_proj", "k_w": "self_attn.k_proj", "v_w": "self_attn.v_proj", "o_w": "self_attn.o_proj",
          "post_norm_w": "post_attention_layernorm", "gate_w": "mlp.gate_proj", "up_w": "mlp.up_proj", "down_w": "mlp.down_proj"}
    parts = [{} for _ in range(shards)]
    parts[0].update({"model.embed_tokens.weight": t(m["embed_tokens"]), "model.norm.weight": t(m["final_norm_w"])})
    parts[-1]["lm_head.weight"] = t(m["lm_head"])
    for i, lw in enumerate(m["layers"]):
        for short, name in hf.items():
            parts[i * shards // len(m["layers"])][f"model.layers.{i}.{name}.weight"] = t(lw[short])
    for n, sd in enumerate(parts):
        save_file(sd, os.path.join(path, f"model-{n + 1:05d}-of-{shards:05d}.safetensors"))


@pytest.mark.parametrize("gpu_pct", [50, 100])
def test_llama_hf_directory_through_run_py(tmp_path, capsys, gpu_pct):
    """`python run.py --benchmark -m <HF Llama directory> ... --gpu-percentage 50 --pin-weight` (run_generation.py:159-166 loads OPT and
    Llama through the same AutoModelForCausalLM call): config.json names LlamaForCausalLM -> checkpoint.load_hf_llama converts it
    layer by layer (two safetensors shards), half the layers stream, the harness prints the HF golden continuation every iteration."""
    from lia_amd import run_generation
    z = np.load(os.path.join(GOLD, "llama_generate_h256.npz"))
    vocab, H, heads, kvh, F, L, B, T, new, seed = [int(v) for v in z["cfg"]]
    m = synth.make_llama_model(seed, vocab, H, heads, kvh, F, L, float(z["w_std"][0]))
    ck = str(tmp_path / "tiny-llama")
    _write_hf_llama(ck, m, dict(H=H, heads=heads, kvh=kvh, F=F, L=L, vocab=vocab, theta=float(z["theta"][0])))
    prompt = synth.make_prompt_ids(seed + 1, B, T, vocab)[0]
    orig = run_generation.synthetic_prompt
    run_generation.synthetic_prompt = lambda vocab_, n, batch, seed=0: __import__("torch").from_numpy(np.tile(prompt[None, :], (batch, 1)))
    try:
        res = run_generation.main(["--benchmark", "-m", ck, "--dtype", "bfloat16", "--ipex", "--input-tokens", str(T), "--max-new-tokens", str(new),
                                   "--batch-size", str(B), "--token-latency", "--num-iter", "2", "--num-warmup", "1", "--greedy",
                                   "--prefill-policy", "0", "--decoding-policy", "2", "--gpu-percentage", str(gpu_pct), "--num-minibatch", "2",
                                   "--pin-weight", "--stream-format", "pack10"])
    finally:
        run_generation.synthetic_prompt = orig
    text = capsys.readouterr().out
    assert "is a Llama" in text and res["prefill_ms"] > 0 and res["decode_tokens_per_s"] > 0
    assert text.count(str(z["ids_bf16"][0, T:].tolist())) == 2, text[-2000:]


def test_llama_shape_name_through_run_py(capsys):
    """`run.py -m meta-llama/Llama-3-8B` used to end in `ValueError: unknown OPT shape`: a known Llama shape name now
    resolves to a random-init model of that shape -- here a two-layer stand-in registered under a name, to keep the test small"""
    from lia_amd import llama, run_generation
    llama.LLAMA_SHAPES["llama-test-2l"] = llama.LlamaShape("llama-test-2l", 256, 4, 2, 512, 2, 512, max_pos=64, rope_theta=10000.0)
    try:
        res = run_generation.main(["--benchmark", "-m", "meta-llama/llama-test-2l", "--input-tokens", "8", "--max-new-tokens", "3", "--batch-size", "2",
                                   "--token-latency", "--num-iter", "2", "--num-warmup", "1", "--greedy", "--gpu-percentage", "50", "--pin-weight"])
    finally:
        del llama.LLAMA_SHAPES["llama-test-2l"]
    assert "is a Llama" in capsys.readouterr().out and res["decode_tokens_per_s"] > 0
