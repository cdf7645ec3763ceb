"""Left-padded batches on the host side (no GPU): generate()'s mask validation, the learned positions, the padded host attention
against tests/padded_ref.py, policy 1's padded layer, run_generation --prompt-file and DataParallelGroup.shard of a mask."""
import ctypes

import numpy as np
import pytest
import torch

import padded_ref as P
import synth
from lia_amd import _native as N
from lia_amd.generation import left_padding_starts


# ---- mask validation ---------------------------------------------------------------------------------------------------------
def test_left_padding_starts_accepts_left_padded_masks():
    m = torch.tensor([[0, 0, 1, 1], [1, 1, 1, 1], [0, 0, 0, 1]])
    assert left_padding_starts(m, (3, 4)).tolist() == [2, 0, 3]
    assert left_padding_starts(m.bool(), (3, 4)).dtype == np.int32
    assert left_padding_starts(np.array([[0, 1], [0, 1]]), (2, 2)).tolist() == [1, 1]
    assert left_padding_starts(None, (3, 4)) is None
    assert left_padding_starts(torch.ones(3, 4, dtype=torch.int64), (3, 4)) is None        # all ones: the unpadded route


@pytest.mark.parametrize("mask,shape,msg", [
    ([[1, 1, 1]], (1, 4), "shape"),
    ([[0, 2, 1]], (1, 3), "0 or 1"),
    ([[0.5, 1, 1]], (1, 3), "0 or 1"),
    ([[1, 1, 0]], (1, 3), "left padded"),
    ([[0, 1, 0, 1]], (1, 4), "left padded"),
    ([[0, 1, 1], [0, 0, 0]], (2, 3), "no 1"),
])
def test_left_padding_starts_refuses(mask, shape, msg):
    with pytest.raises(ValueError, match=msg):
        left_padding_starts(torch.tensor(mask), shape)


def test_generate_refuses_a_bad_mask_before_any_work():
    from lia_amd.generation import generate

    class Dummy:
        family = "opt"
    with pytest.raises(ValueError, match="left padded"):
        generate(Dummy(), torch.zeros((1, 3), dtype=torch.int64), max_new_tokens=1, attention_mask=torch.tensor([[1, 0, 1]]))

    class Llama:
        family = "llama"
    with pytest.raises(ValueError, match="Llama"):
        generate(Llama(), torch.zeros((1, 3), dtype=torch.int64), max_new_tokens=1, attention_mask=torch.tensor([[0, 1, 1]]))


# ---- positions ---------------------------------------------------------------------------------------------------------------
def test_positions_match_transformers_opt():
    from transformers.models.opt.modeling_opt import OPTLearnedPositionalEmbedding
    mask = torch.tensor([[0, 0, 0, 1, 1], [1, 1, 1, 1, 1], [0, 1, 1, 1, 1], [0, 0, 0, 0, 1]])
    emb = OPTLearnedPositionalEmbedding(16, 4)
    with torch.no_grad():
        emb.weight.copy_(torch.arange(18, dtype=torch.float32)[:, None].repeat(1, 4))
    try:
        hf = emb(mask, 0)
    except TypeError:
        hf = emb(mask)
    assert (hf[..., 0].long().numpy() == P.positions(mask.numpy())).all()
    starts = P.starts_of(mask.numpy())
    # the kernel's rule: position t - s_b + 2 at t >= s_b, 1 at a pad position; decode token at pos0: pos0 - s_b + 2
    t = np.arange(5)
    rule = np.where(t[None] >= starts[:, None], t[None] - starts[:, None] + 2, 1)
    assert (rule == P.positions(mask.numpy())).all()
    ext = torch.cat([mask, torch.ones((4, 3), dtype=torch.int64)], 1)
    try:
        hfd = emb(ext, 7)
    except TypeError:
        hfd = None
    dec = P.positions(mask.numpy(), past_len=7, T=1)
    assert (dec[:, 0] == 7 - starts + 2).all()
    if hfd is not None:
        assert (hfd[..., 0].long().numpy()[:, 0] == dec[:, 0]).all()


# ---- host attention ----------------------------------------------------------------------------------------------------------
def _host_case(B, T, pos0, starts, heads=2, d=64, seed=3):
    H = heads * d
    rs = np.random.RandomState(seed)
    q, k, v = (synth.f32_to_bf16_bits(rs.standard_normal((B, T, H)).astype(np.float32)) for _ in range(3))
    Bc, b0, smax = B + 3, 2, pos0 + T + 2
    kc = synth.f32_to_bf16_bits(rs.standard_normal((smax, Bc, heads, d)).astype(np.float32))
    vc = synth.f32_to_bf16_bits(rs.standard_normal((smax, Bc, heads, d)).astype(np.float32))
    # cache rows at pad positions hold large finite garbage: a kernel that read them would show
    for b, s in enumerate(starts):
        kc[:min(s, pos0), b0 + b] = synth.f32_to_bf16_bits(np.full((min(s, pos0), heads, d), 3.0e4, np.float32))
        vc[:min(s, pos0), b0 + b] = synth.f32_to_bf16_bits(np.full((min(s, pos0), heads, d), -2.0e4, np.float32))
        if s > pos0:
            k[b, :s - pos0] = synth.f32_to_bf16_bits(np.full((s - pos0, H), 3.0e4, np.float32))
            v[b, :s - pos0] = synth.f32_to_bf16_bits(np.full((s - pos0, H), -2.0e4, np.float32))
    return q, k, v, kc, vc, Bc, b0, heads, d


def _run_host(fn, q, k, v, kc, vc, B, T, pos0, heads, d, Bc, b0, *extra):
    out = np.full_like(q, 0x7fc0)
    kc, vc = kc.copy(), vc.copy()
    L = N.lib()
    rc = getattr(L, fn)(q.ctypes.data, k.ctypes.data, v.ctypes.data, kc.ctypes.data, vc.ctypes.data, out.ctypes.data,
                        B, T, pos0, heads, d, Bc, b0, 3, *extra)
    assert rc == 0, N.lib().lia_last_error()
    return out, kc, vc


@pytest.mark.parametrize("T", [1, 7, 64, 130])
@pytest.mark.parametrize("pos0", [0, 5])
def test_host_attention_padded_against_reference(T, pos0):
    B = 3
    S = pos0 + T
    starts = np.array([0, min(1, S - 1), S - 1], dtype=np.int32) if T > 1 else np.array([0, min(1, S - 1), S - 1], dtype=np.int32)
    q, k, v, kc, vc, Bc, b0, heads, d = _host_case(B, T, pos0, starts)
    out, kc2, vc2 = _run_host("lia_host_attention_padded", q, k, v, kc, vc, B, T, pos0, heads, d, Bc, b0, starts.ctypes.data)
    ref = P.host_attention(q, kc2, vc2, S, heads, starts, b0)
    pos = pos0 + np.arange(T)
    pad = pos[None, :] < starts[:, None]
    assert (out[pad] == 0).all(), "a pad query must give an exact zero row"
    real = ~pad
    a, b = synth.bf16_bits_to_f32(out[real]), synth.bf16_bits_to_f32(ref[real])
    assert np.isfinite(a).all()
    assert np.abs(a - b).max() <= 0.02 and (out[real] == ref[real]).mean() > 0.97
    # all-zero starts: bit-identical to the unpadded entry
    z = np.zeros(B, np.int32)
    o1, _, _ = _run_host("lia_host_attention_padded", q, k, v, kc, vc, B, T, pos0, heads, d, Bc, b0, z.ctypes.data)
    o0, _, _ = _run_host("lia_host_attention", q, k, v, kc, vc, B, T, pos0, heads, d, Bc, b0)
    assert (o1 == o0).all()


def test_host_attention_padded_refuses_a_start_behind_the_last_position():
    q, k, v, kc, vc, Bc, b0, heads, d = _host_case(2, 4, 0, [0, 0])
    bad = np.array([0, 4], np.int32)
    out = np.zeros_like(q)
    rc = N.lib().lia_host_attention_padded(q.ctypes.data, k.ctypes.data, v.ctypes.data, kc.ctypes.data, vc.ctypes.data,
                                           out.ctypes.data, 2, 4, 0, heads, d, Bc, b0, 2, bad.ctypes.data)
    assert rc != 0 and b"starts[1]" in N.lib().lia_last_error()


def test_host_layer_forward_padded_rows_equal_their_unpadded_run():
    """policy 1 (lia_host_layer_forward_padded): each real row of a left-padded batch equals the same row run alone and
    unpadded (the layer's linear parts are per row; the attention sees exactly the row's own keys), pad rows stay finite"""
    H, heads, F = 128, 2, 256
    rs = np.random.RandomState(11)
    m = synth.make_model(5, 64, 64, H, F, 1, 0.05)
    lw = m["layers"][0]
    desc = N.LayerDesc(H, heads, F, 1e-5)
    W = [np.ascontiguousarray(lw[k]) for k in synth.layer_shapes(H, F)]
    wp = (ctypes.c_void_p * 16)(*[w.ctypes.data for w in W])
    B, T = 3, 6
    starts = np.array([0, 2, 5], np.int32)
    x = synth.f32_to_bf16_bits(rs.standard_normal((B, T, H)).astype(np.float32))
    kc = np.zeros((T, B, heads, H // heads), np.uint16)
    vc = np.zeros_like(kc)
    y = np.zeros_like(x)
    L = N.lib()
    assert L.lia_host_layer_forward_padded(ctypes.byref(desc), ctypes.byref(wp), x.ctypes.data, y.ctypes.data, kc.ctypes.data,
                                           vc.ctypes.data, T, B, B, T, 0, 0, 2, starts.ctypes.data) == 0, L.lia_last_error()
    for b in range(B):
        s = int(starts[b])
        xb = np.ascontiguousarray(x[b:b + 1, s:])
        kb = np.zeros((T - s, 1, heads, H // heads), np.uint16)
        vb = np.zeros_like(kb)
        yb = np.zeros_like(xb)
        assert L.lia_host_layer_forward(ctypes.byref(desc), ctypes.byref(wp), xb.ctypes.data, yb.ctypes.data, kb.ctypes.data,
                                        vb.ctypes.data, T - s, 1, 1, T - s, 0, 0, 2) == 0
        assert (y[b, s:] == yb[0]).all(), f"row {b}"
        assert np.isfinite(synth.bf16_bits_to_f32(y[b, :s])).all()


# ---- --prompt-file -----------------------------------------------------------------------------------------------------------
def _tokenizer_dir(tmp_path, with_pad=True):
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast
    words = ["<pad>", "</s>", "<unk>", "the", "weights", "stay", "on", "host", "and", "stream", "layer", "by"]
    tok = Tokenizer(models.WordLevel({w: i for i, w in enumerate(words)}, unk_token="<unk>"))
    tok.pre_tokenizer = pre_tokenizers.Whitespace()
    d = tmp_path / ("ckpt" if with_pad else "ckpt_nopad")
    d.mkdir()
    kw = dict(pad_token="<pad>") if with_pad else {}
    PreTrainedTokenizerFast(tokenizer_object=tok, unk_token="<unk>", eos_token="</s>", **kw).save_pretrained(str(d))
    return d


def test_prompt_file_left_pads_and_cycles(tmp_path, capsys):
    from lia_amd import run_generation as rg
    d = _tokenizer_dir(tmp_path)
    pf = tmp_path / "prompts.txt"
    pf.write_text("the weights stay on host\nstream\n\nlayer by layer\n")
    args = rg.build_parser().parse_args(["-m", str(d), "--batch-size", "5", "--prompt-file", str(pf)])
    t = rg.load_tokenizer(str(d))
    ids, mask = rg.prompt_file_inputs(args, 64, t, 1)
    assert ids.shape == (5, 5) and mask.shape == (5, 5) and ids.dtype == torch.int64
    assert ids[0].tolist() == [3, 4, 5, 6, 7] and mask[0].tolist() == [1] * 5
    assert ids[1].tolist() == [0, 0, 0, 0, 9] and mask[1].tolist() == [0, 0, 0, 0, 1]          # the tokenizer's <pad> = 0
    assert ids[2].tolist() == [0, 0, 10, 11, 10] and mask[2].tolist() == [0, 0, 1, 1, 1]
    assert torch.equal(ids[3], ids[0]) and torch.equal(ids[4], ids[1])                          # cycled in file order
    assert left_padding_starts(mask, ids.shape).tolist() == [0, 4, 2, 0, 4]
    assert "Prompt sizes" in capsys.readouterr().out
    # no pad token in the tokenizer: the model's pad_token_id
    d2 = _tokenizer_dir(tmp_path, with_pad=False)
    ids2, mask2 = rg.prompt_file_inputs(rg.build_parser().parse_args(["-m", str(d2), "--batch-size", "2", "--prompt-file", str(pf)]),
                                        64, rg.load_tokenizer(str(d2)), 1)
    assert ids2[1].tolist() == [1, 1, 1, 1, 9] and torch.equal(mask2, mask[:2])
    with pytest.raises(SystemExit, match="tokenizer"):
        rg.prompt_file_inputs(args, 64, None, 1)


def test_prompt_file_and_prompt_exclude_each_other(tmp_path):
    from lia_amd import run_generation as rg
    pf = tmp_path / "p.txt"
    pf.write_text("the\n")
    args = rg.build_parser().parse_args(["-m", "facebook/opt-125m", "--prompt", "the", "--prompt-file", str(pf)])
    with pytest.raises(SystemExit, match="exclude"):
        rg._main(args)


# ---- data parallel -----------------------------------------------------------------------------------------------------------
def test_dp_shard_carries_the_mask_rows():
    from lia_amd.dp import DataParallelGroup, shard_rows
    ids = torch.arange(7 * 3).view(7, 3)
    mask = torch.ones(7, 3, dtype=torch.int64)
    mask[:, 0] = torch.tensor([0, 1, 0, 1, 0, 1, 0])
    for rank in range(3):
        g = DataParallelGroup.__new__(DataParallelGroup)
        g.rank, g.world = rank, 3
        i2, m2 = g.shard(ids, mask)
        lo, hi = shard_rows(7, rank, 3)
        assert torch.equal(i2, ids[lo:hi]) and torch.equal(m2, mask[lo:hi])
        assert torch.equal(g.shard(ids), ids[lo:hi])
    with pytest.raises(ValueError, match="rows"):
        g.shard(ids, mask[:3])


# ---- the reference's own CPU branch on a padded batch (tests/golden/make_golden_padded.py) ----------------------------------
PADDED_CASES = ("padded_layer_h128", "padded_layer_h256_d64")


def _close(a_bits, b_bits, atol, rtol, frac_exact=None):
    a, b = synth.bf16_bits_to_f32(a_bits), synth.bf16_bits_to_f32(b_bits)
    assert a.shape == b.shape
    err = np.abs(a - b)
    assert (err <= atol + rtol * np.abs(b)).all(), f"max err {err.max():.4g} at |ref| {np.abs(b).flat[err.argmax()]:.4g}"
    if frac_exact is not None:
        assert (a_bits == b_bits).mean() >= frac_exact, f"only {(a_bits == b_bits).mean():.3f} bit-identical"


@pytest.mark.parametrize("name", PADDED_CASES)
def test_positions_match_the_references_embedding(name):
    import os
    z = np.load(os.path.join(os.path.dirname(synth.__file__), name + ".npz"))
    H, heads, F, B, T, new, seed, _ = [int(v) for v in z["cfg"]]
    mask = (np.arange(T)[None, :] >= z["starts"][:, None]).astype(np.int64)
    assert (P.positions(mask) == z["pos_prefill"]).all()
    for s in range(new):
        assert (P.positions(mask, past_len=T + s, T=1)[:, 0] == z["pos_dec"][s]).all()
        assert (T + s - z["starts"] + 2 == z["pos_dec"][s]).all()          # the padded embedding kernel's rule


@pytest.mark.parametrize("name", PADDED_CASES)
def test_host_layer_forward_padded_matches_the_references_cpu_branch(name):
    """lia_host_layer_forward_padded (policy 1) against the reference's OPTDecoderLayer_forward(policy=1) with the HF 4-D causal +
    padding mask: the prefill's real rows, two decode steps, the cache it filled; the tolerances of the p1_* golden tests
    (tests/test_oracle_golden.py).  Pad query rows differ by design: zeros here, an average over an all-masked row there."""
    import os
    L = N.lib()
    if not L.lia_host_has_avx512_bf16():
        pytest.skip("host without AVX-512-BF16")
    z = np.load(os.path.join(os.path.dirname(synth.__file__), name + ".npz"))
    H, heads, F, B, T, new, seed, _ = [int(v) for v in z["cfg"]]
    starts = np.ascontiguousarray(z["starts"], dtype=np.int32)
    W = synth.make_layer(seed, H, F, float(z["w_std"][0]))
    desc = N.LayerDesc(H, heads, F, 1e-5)
    ws = [np.ascontiguousarray(W[n]) for n in synth.layer_shapes(H, F)]
    arr = (ctypes.c_void_p * 16)(*[w.ctypes.data for w in ws])
    kc = np.zeros((T + new, B, heads, H // heads), np.uint16)
    vc = np.zeros_like(kc)
    x = synth.make_hidden(seed + 1, B, T, H, False)
    y = np.zeros_like(x)
    assert L.lia_host_layer_forward_padded(ctypes.byref(desc), ctypes.byref(arr), x.ctypes.data, y.ctypes.data, kc.ctypes.data,
                                           vc.ctypes.data, T + new, B, B, T, 0, 0, 4, starts.ctypes.data) == 0, L.lia_last_error()
    real = np.arange(T)[None, :] >= starts[:, None]
    _close(y[real], z["p1_hidden"][real], atol=0.05, rtol=0.02)
    for s in range(new):
        xs = synth.make_hidden(seed + 100 + s, B, 1, H, False)
        ys = np.zeros_like(xs)
        assert L.lia_host_layer_forward_padded(ctypes.byref(desc), ctypes.byref(arr), xs.ctypes.data, ys.ctypes.data, kc.ctypes.data,
                                               vc.ctypes.data, T + new, B, B, 1, T + s, 0, 4, starts.ctypes.data) == 0
        _close(ys, z[f"p1_dec{s}_hidden"], atol=0.05, rtol=0.02)
    _close(kc, z["p1_kcache"], atol=0.02, rtol=0.008, frac_exact=0.97)
    _close(vc, z["p1_vcache"], atol=0.02, rtol=0.008, frac_exact=0.97)
