"""Left-padded batches on the MI355X: every padded kernel instantiation against tests/padded_ref.py, the padded embedding, and
generate(..., attention_mask=) on small OPTs (d 128: the tuned prefill kernel, d 64: the generic one) -- each row of a padded
batch against the oracle's run of that row ALONE and unpadded, and against the product's own B = 1 run of the row."""
import numpy as np
import pytest

import padded_ref as P
import synth
import test_gpu_kernel_variants as KV
from test_gpu_kernel_variants import gpu  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

GARBAGE_K, GARBAGE_V = 30000.0, -20000.0        # K / V rows at pad positions: large and finite, a read of one would show
START_POOL = (0, 1, 31, 32, 63, 64, 65, 127, 128, 129)


def _starts(B, n, seed):
    pool = [s for s in START_POOL if s <= n - 1] + [n - 1]
    rs = np.random.RandomState(seed)
    return np.array([pool[(seed + 3 * b) % len(pool)] if b < len(pool) else pool[rs.randint(len(pool))] for b in range(B)], np.int32)


def _bf16_fill(torch, v):
    return torch.tensor(v, dtype=torch.bfloat16).view(torch.int16).item()


def run_padded(gpu, B, T, S, heads, kvh, d, ps, starts, seed=7):
    torch, launch = gpu
    Bc, b0, H = B + 2, 1, heads * d
    q, kc, vc, out = KV.attn_buffers(torch, seed, B, T, S, heads, kvh, d, Bc, b0)
    for b, s in enumerate(starts):
        kc[:s, b0 + b] = _bf16_fill(torch, GARBAGE_K)
        vc[:s, b0 + b] = _bf16_fill(torch, GARBAGE_V)
    st = torch.from_numpy(np.asarray(starts, np.int32)).cuda()
    name = "lia_attn_prefill_padded_launch" if T > 1 else "lia_attn_decode_padded_launch"
    n = T if T > 1 else S
    assert launch(name, q, H + 16, kc, vc, out, H + 24, B, n, heads, kvh, d, Bc, b0, ps, st) == 0
    oh = KV.host(out)
    assert (oh[:, H:] == KV.SENTINEL).all(), "the launch wrote into the gap columns of out"
    qh = KV.host(q)[:, :H].reshape(B, T, H)
    return qh, KV.host(kc), KV.host(vc), oh[:, :H].reshape(B, T, H), b0, (q, kc, vc, out, st)


def check_padded(what, got, ref, starts, S, T):
    pos = S - T + np.arange(T)
    pad = pos[None, :] < np.asarray(starts)[:, None]
    assert (got[pad] == 0).all(), f"{what}: a pad query row is not exactly zero"
    KV.check_attention(what, got[~pad], ref[~pad])


PREFILL_CASES = [  # (B, T, heads, kv_heads, d, post_scale): d 128 r05 order (groups not a multiple of 8), XCD order, pairs, one block
    (3, 300, 4, 4, 128, 0), (2, 256, 4, 4, 128, 0), (4, 130, 2, 2, 128, 1), (2, 64, 4, 4, 128, 0), (3, 2, 2, 2, 128, 0),
    (3, 300, 4, 2, 128, 1),
    (2, 300, 4, 2, 64, 1), (3, 130, 2, 2, 64, 0), (2, 64, 2, 2, 32, 0), (3, 256, 2, 2, 32, 0), (2, 2, 2, 2, 64, 0),
    (1, 2016, 56, 56, 128, 0),                                                                  # OPT-30B width, T 2016
]


@pytest.mark.parametrize("B,T,heads,kvh,d,ps", PREFILL_CASES)
def test_padded_prefill_kernels(gpu, B, T, heads, kvh, d, ps):
    starts = _starts(B, T, seed=T + d) if B > 1 else np.array([129], np.int32)
    qh, k0, v0, got, b0, bufs = run_padded(gpu, B, T, T, heads, kvh, d, ps, starts)
    ref = P.attention(qh, k0, v0, T, heads, kvh, ps, starts, b0)
    check_padded(f"prefill B {B} T {T} heads {heads}/{kvh} d {d} ps {ps} starts {starts.tolist()}", got, ref, starts, T, T)
    # all-zero starts through the padded entry == the unpadded entry, bit for bit
    torch, launch = gpu
    q, kc, vc, out, st = bufs
    H = heads * d
    st.zero_()
    out.fill_(KV.SENTINEL)
    assert launch("lia_attn_prefill_padded_launch", q, H + 16, kc, vc, out, H + 24, B, T, heads, kvh, d, B + 2, b0, ps, st) == 0
    a = KV.host(out).copy()
    out.fill_(KV.SENTINEL)
    assert launch("lia_attn_prefill_launch", q, H + 16, kc, vc, out, H + 24, B, T, heads, kvh, d, B + 2, b0, ps) == 0
    assert (a == KV.host(out)).all()


DECODE_CASES = [(3, 1, 2, 2, 128), (3, 2, 4, 4, 64), (3, 65, 4, 1, 32), (3, 1037, 4, 4, 128), (2, 1037, 8, 1, 64), (3, 65, 2, 2, 128)]


@pytest.mark.parametrize("B,S,heads,kvh,d", DECODE_CASES)
def test_padded_decode_kernels(gpu, B, S, heads, kvh, d):
    starts = _starts(B, S, seed=S + d)
    qh, k0, v0, got, b0, bufs = run_padded(gpu, B, 1, S, heads, kvh, d, 0, starts)
    ref = P.attention(qh, k0, v0, S, heads, kvh, 0, starts, b0)
    check_padded(f"decode B {B} S {S} heads {heads}/{kvh} d {d} starts {starts.tolist()}", got, ref, starts, S, 1)
    torch, launch = gpu
    q, kc, vc, out, st = bufs
    H = heads * d
    st.zero_()
    out.fill_(KV.SENTINEL)
    assert launch("lia_attn_decode_padded_launch", q, H + 16, kc, vc, out, H + 24, B, S, heads, kvh, d, B + 2, b0, 0, st) == 0
    a = KV.host(out).copy()
    out.fill_(KV.SENTINEL)
    assert launch("lia_attn_decode_launch", q, H + 16, kc, vc, out, H + 24, B, S, heads, kvh, d, B + 2, b0, 0) == 0
    assert (a == KV.host(out)).all()


@pytest.mark.parametrize("past_len,T", [(0, 9), (12, 1)])
def test_padded_embedding_positions(gpu, past_len, T):
    torch, _ = gpu
    from lia_amd import _native as N
    L = N.lib()
    B, H, vocab = 4, 256, 50
    rs = np.random.RandomState(1)
    tok = synth.f32_to_bf16_bits((0.5 * rs.standard_normal((vocab, H))).astype(np.float32))
    pos = synth.f32_to_bf16_bits((0.5 * rs.standard_normal((64, H))).astype(np.float32))
    ids = rs.randint(0, vocab, (B, T)).astype(np.int64)
    starts = np.array([0, 1, 8, 5], np.int32)
    d = [torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda() for a in (ids, tok, pos)]
    y = torch.zeros((B, T, H), dtype=torch.int16, device="cuda")
    st = torch.from_numpy(starts).cuda()
    torch.cuda.synchronize()
    assert L.lia_embed_padded(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), y.data_ptr(), B, T, past_len, H, st.data_ptr(), None) == 0
    torch.cuda.synchronize()
    p = np.arange(past_len, past_len + T)[None, :] - starts[:, None]
    idx = np.where(p >= 0, p + 2, 1)
    mask = (np.arange(max(past_len + T, 9))[None, :] >= starts[:, None]).astype(np.int64)[:, :max(past_len + T, 9)]
    assert (idx == P.positions(mask, past_len, T)).all()
    want = synth.f32_to_bf16_bits(synth.bf16_bits_to_f32(tok[ids]) + synth.bf16_bits_to_f32(pos[idx]))
    assert (y.cpu().numpy().view(np.uint16) == want).all()
    y2 = torch.zeros_like(y)
    st.zero_()
    torch.cuda.synchronize()
    assert L.lia_embed_padded(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), y.data_ptr(), B, T, past_len, H, st.data_ptr(), None) == 0
    assert L.lia_embed(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), y2.data_ptr(), B, T, past_len, H, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(y, y2)


# ---- whole model --------------------------------------------------------------------------------------------------------------
MODELS = {"d128": dict(H=256, heads=2, F=512, L=4), "d64": dict(H=128, heads=2, F=256, L=4)}
VOCAB, MAX_POS, NEW = 256, 64, 4
LENGTHS = (9, 1, 5, 9, 3)                 # a row with one real token among them
POLICIES = {
    "3/3 resident": dict(prefill_policy=3, decoding_policy=3, gpu_percentage=100),
    "0/2": dict(prefill_policy=0, decoding_policy=2, gpu_percentage=25),
    "0/0": dict(prefill_policy=0, decoding_policy=0, gpu_percentage=25),
    "3/3 streamed": dict(prefill_policy=3, decoding_policy=3, gpu_percentage=25),
    "1/1": dict(prefill_policy=1, decoding_policy=1, gpu_percentage=25),
    "0/2 ragged minibatches": dict(prefill_policy=0, decoding_policy=2, gpu_percentage=25, num_minibatch=2),
    "0/2 + cpu_layers": dict(prefill_policy=0, decoding_policy=2, gpu_percentage=25, cpu_layers=1),
    "3/3 + online cpu_layers": dict(prefill_policy=3, decoding_policy=3, gpu_percentage=0, cpu_layers=-1, cpu_layers_start=2),
}
_CACHE = {}


def _model(name):
    from lia_amd.model import LiaOPTModel, OPTShape
    c = MODELS[name]
    w_std = float(np.load(synth.__file__.replace("synth.py", "generate_tiny.npz"))["w_std"][0])
    m = synth.make_model(31, VOCAB, MAX_POS, c["H"], c["F"], c["L"], w_std)
    model = LiaOPTModel.from_numpy(OPTShape("padded", c["H"], c["heads"], c["F"], c["L"], vocab=VOCAB, max_pos=MAX_POS), m)
    return m, model


def _batch():
    T = max(LENGTHS)
    rs = np.random.RandomState(5)
    ids = np.full((len(LENGTHS), T), 1, np.int64)
    mask = np.zeros((len(LENGTHS), T), np.int64)
    for b, n in enumerate(LENGTHS):
        ids[b, T - n:] = rs.randint(3, VOCAB, n)
        mask[b, T - n:] = 1
    return ids, mask


def _logits(lst):
    return [lg.view(__import__("torch").int16).cpu().numpy().view(np.uint16) for lg in lst]


def _logits_bound(got, ref_ids, lg, ref_lg, b, n, what, decode_within_one=0.95, first_within_one=0.95):
    """every step's logits of row b while it still follows the other run: within 4 quanta of the largest logit (the whole-model
    bound of test_gpu_wholemodel._check_logits), `within_one` of them within one quantum"""
    import parity_util
    for s in range(NEW):
        if not (got[0, n:n + s] == np.asarray(ref_ids)[0, n:n + s]).all():
            break
        parity_util.quantum_bound(lg[s][b:b + 1], ref_lg[s], f"{what}, step {s} logits", min_exact=0.0, max_quanta=4.0,
                                  within_one=first_within_one if s == 0 else decode_within_one)


@pytest.mark.parametrize("mname", list(MODELS))
@pytest.mark.parametrize("pname", list(POLICIES))
def test_generate_padded_rows_equal_their_own_unpadded_runs(mname, pname, oracle):
    import torch
    import parity_util
    from lia_amd.generation import generate
    kw = dict(POLICIES[pname], pin_weight=True)
    m, model = _model(mname)
    try:
        ids, mask = _batch()
        T = ids.shape[1]
        out, _, lg = generate(model, torch.from_numpy(ids), attention_mask=torch.from_numpy(mask), max_new_tokens=NEW,
                              min_new_tokens=NEW, return_logits=True, **kw)
        out, lg = out.numpy(), _logits(lg)
        opol = (kw["prefill_policy"], kw["decoding_policy"])
        for b, n in enumerate(LENGTHS):
            row = ids[b:b + 1, T - n:]
            ref_ids, _, ref_lg = oracle.generate(m, row, NEW, MODELS[mname]["heads"], opol[0], opol[1], kw["gpu_percentage"],
                                                     return_logits=True)
            got = np.concatenate([row, out[b:b + 1, T:]], axis=1)
            assert (out[b, T - n:T] == row[0]).all()
            parity_util.ids_equal_or_near_tie(got, ref_ids, ref_lg, n, what=f"{mname} {pname} row {b} vs oracle")
            # every step's logits while the row still follows the other run (the step's inputs are then the same tokens), within
            # the whole-model bound of test_gpu_wholemodel._check_logits: 4 quanta of the largest logit, 95 % within one quantum
            # (decode steps against the oracle: 88 % within one quantum.  One row's 256 logits of these small models after a decode
            # step spread to 2 quanta from the oracle's for the UNPADDED row 0 as much as for the padded ones -- the GPU decode's
            # rounding, not the padding; against the product's own unpadded run below they are nearly all bit-identical)
            _logits_bound(got, ref_ids, lg, ref_lg, b, n, f"{mname} {pname} row {b} vs oracle", decode_within_one=0.88)
            # the product's own B = 1 run of the row, unpadded
            o1, _, l1 = generate(model, torch.from_numpy(row), max_new_tokens=NEW, min_new_tokens=NEW, return_logits=True, **kw)
            l1 = _logits(l1)
            parity_util.ids_equal_or_near_tie(got, o1.numpy(), l1, n, what=f"{mname} {pname} row {b} vs B 1")
            # (a one-token prompt run alone is decode-sized: the cooperative split may compute it on the host cores, with the host
            # attention's rounding, where the padded batch's prefill runs on the GPU -- then the oracle's bound)
            coop = n == 1 and kw.get("cpu_layers")
            _logits_bound(got, o1.numpy(), lg, l1, b, n, f"{mname} {pname} row {b} vs B 1", decode_within_one=0.88 if coop else 0.95,
                          first_within_one=0.88 if coop else 0.95)
    finally:
        model._lia_scheduler.close() if getattr(model, "_lia_scheduler", None) else None
        model.close()


@pytest.mark.parametrize("pname", ["3/3 resident", "0/2"])
def test_all_ones_mask_and_a_later_unpadded_call_take_todays_route(pname):
    import torch
    from lia_amd.generation import generate
    kw = dict(POLICIES[pname], pin_weight=True, max_new_tokens=NEW, min_new_tokens=NEW, return_logits=True)
    ids, mask = _batch()
    t_ids = torch.from_numpy(ids)
    m, model = _model("d128")
    _, fresh = _model("d128")
    try:
        a, _, la = generate(model, t_ids, **kw)
        b, _, lb = generate(model, t_ids, attention_mask=torch.ones_like(t_ids), **kw)
        assert torch.equal(a, b) and all(torch.equal(x, y) for x, y in zip(la, lb))
        generate(model, t_ids, attention_mask=torch.from_numpy(mask), **kw)              # a padded generation ...
        c, _, lc = generate(model, t_ids, **kw)                                           # ... leaves no table behind
        d, _, ld = generate(fresh, t_ids, **kw)
        assert torch.equal(c, d) and all(torch.equal(x, y) for x, y in zip(lc, ld))
        assert torch.equal(a, c)
    finally:
        for mm in (model, fresh):
            if getattr(mm, "_lia_scheduler", None):
                mm._lia_scheduler.close()
            mm.close()


def test_eos_in_a_padded_batch():
    """the EOS / unfinished / early-stop branch of the greedy loop: a row that emits eos_token_id finishes, is then filled with
    pad_token_id, the other rows do not change, and a batch whose rows have all finished stops early"""
    import torch
    from lia_amd.generation import generate
    kw = dict(POLICIES["0/2"], pin_weight=True)
    ids, mask = _batch()
    T, N_ = ids.shape[1], 6
    m, model = _model("d64")
    try:
        t_ids, t_mask = torch.from_numpy(ids), torch.from_numpy(mask)
        first = generate(model, t_ids, attention_mask=t_mask, max_new_tokens=N_, eos_token_id=None, **kw).numpy()
        gen = first[:, T:]
        pick = None
        for k in range(1, N_ - 1):
            for r in range(gen.shape[0]):
                tok = int(gen[r, k])
                others = np.delete(gen, r, axis=0)
                if tok not in gen[r, :k] and tok not in others and tok != 1:
                    pick = (r, k, tok)
                    break
            if pick:
                break
        assert pick is not None, f"no token emitted by one row only: {gen.tolist()}"
        r, k, tok = pick
        out = generate(model, t_ids, attention_mask=t_mask, max_new_tokens=N_, eos_token_id=tok, pad_token_id=1, **kw).numpy()
        assert out.shape == first.shape                                         # the other rows are unfinished: no early stop
        assert (out[r, :T + k + 1] == first[r, :T + k + 1]).all() and (out[r, T + k + 1:] == 1).all()
        assert (np.delete(out, r, axis=0) == np.delete(first, r, axis=0)).all()
        # one row alone (still left padded): it finishes at step k and the loop stops there
        one = generate(model, t_ids[r:r + 1], attention_mask=t_mask[r:r + 1], max_new_tokens=N_, eos_token_id=None, **kw).numpy()
        k1 = [i for i in range(N_) if one[0, T + i] == tok]
        if k1:
            stop = generate(model, t_ids[r:r + 1], attention_mask=t_mask[r:r + 1], max_new_tokens=N_, eos_token_id=tok, **kw).numpy()
            assert stop.shape[1] == T + k1[0] + 1 and (stop[0] == one[0, :T + k1[0] + 1]).all()
        else:
            raise AssertionError(f"row {r} alone did not emit {tok}: {one.tolist()}")
    finally:
        if getattr(model, "_lia_scheduler", None):
            model._lia_scheduler.close()
        model.close()


# ---- HF transformers fp32 (the reference tests' model replacement check, tests/test_gpu_reference_tests.py) --------------------
HF_CFG = dict(model_type="opt", activation_function="relu", do_layer_norm_before=True, ffn_dim=8192, hidden_size=2048, init_std=0.02,
              max_position_embeddings=2048, num_attention_heads=16, num_hidden_layers=1, vocab_size=50272, word_embed_proj_dim=2048,
              bos_token_id=2, eos_token_id=2, pad_token_id=1, dropout=0.1, attention_dropout=0.0, activation_dropout=0.0, layerdrop=0.0,
              use_cache=True)


@pytest.fixture(scope="module")
def hf_models(tmp_path_factory):
    import json
    import os
    import torch
    import transformers
    from safetensors.torch import save_file
    from lia_amd.checkpoint import load_hf_opt
    torch.manual_seed(128)
    hf = transformers.OPTForCausalLM(transformers.OPTConfig(**HF_CFG)).eval()
    path = str(tmp_path_factory.mktemp("opt_padded") / "opt-fixture")
    os.makedirs(path)
    json.dump(dict(HF_CFG, torch_dtype="bfloat16"), open(os.path.join(path, "config.json"), "w"))
    sd = {k: v.detach().to(torch.bfloat16).contiguous() for k, v in hf.state_dict().items() if k != "lm_head.weight"}
    save_file(sd, os.path.join(path, "model.safetensors"))
    model = load_hf_opt(path)
    yield hf, model
    if getattr(model, "_lia_scheduler", None) is not None:
        model._lia_scheduler.close()
    model.close()


@pytest.mark.parametrize("flags", [dict(prefill_policy=3, decoding_policy=3, gpu_percentage=100, pin_weight=True),
                                   dict(prefill_policy=0, decoding_policy=2, gpu_percentage=0, pin_weight=True), dict()],
                         ids=["resident-3-3", "streamed-0-2", "host-1-1"])
def test_padded_batch_against_hf_fp32(hf_models, flags):
    """HF's fp32 OPTForCausalLM on the same left-padded batch and mask: each row's last-position logits within the reference
    tests' prec = 0.1, and the greedy ids equal on every step the fp32 model decides (top-2 gap > 4 bf16 quanta)"""
    import torch
    from lia_amd.generation import generate
    hf, model = hf_models
    lengths, T, new = (8, 1, 5), 8, 2
    rs = np.random.RandomState(9)
    ids = torch.ones((len(lengths), T), dtype=torch.long)
    mask = torch.zeros_like(ids)
    for b, n in enumerate(lengths):
        ids[b, T - n:] = torch.from_numpy(rs.randint(3, 50272, n))
        mask[b, T - n:] = 1
    out, _, logits = generate(model, ids, attention_mask=mask, max_new_tokens=new, min_new_tokens=new, return_logits=True, **flags)
    got = logits[0].float().cpu().numpy()
    with torch.no_grad():
        want = hf(input_ids=ids, attention_mask=mask).logits[:, -1].float().numpy()
    err = np.abs(got - want).max(axis=1)
    assert (err <= 0.1).all(), f"max |logit - HF fp32 logit| per row {err.tolist()} > prec 0.1 ({flags})"
    with torch.no_grad():
        cur, cm = ids, mask
        for s in range(new):
            lg = hf(input_ids=cur, attention_mask=cm).logits[:, -1].float()
            lg[:, 2] = -float("inf")                                # min_new_tokens: EOS suppressed
            for b in range(len(lengths)):
                quantum = 2.0 ** (np.floor(np.log2(max(float(lg[b].abs().max()), 1.0))) - 7)
                top = torch.topk(lg[b], 2).values
                if float(top[0] - top[1]) > 4 * quantum and (out[b, T:T + s] == cur[b, T:T + s]).all():
                    assert int(out[b, T + s]) == int(torch.argmax(lg[b])), (b, s, out.tolist())
            cur = torch.cat([cur, torch.argmax(lg, -1, keepdim=True)], 1)
            cm = torch.cat([cm, torch.ones_like(cm[:, :1])], 1)


def test_generate_refuses_bad_masks_by_name():
    import torch
    from lia_amd.generation import generate
    ids, mask = _batch()
    m, model = _model("d64")
    try:
        t = torch.from_numpy(ids)
        for bad, msg in ((torch.ones(2, 3), "shape"), (torch.from_numpy(mask) * 2, "0 or 1"),
                         (torch.from_numpy(mask[:, ::-1].copy()), "left padded"), (torch.zeros_like(t), "no 1")):
            with pytest.raises(ValueError, match=msg):
                generate(model, t, attention_mask=bad, max_new_tokens=2, prefill_policy=3, decoding_policy=3, gpu_percentage=100)
    finally:
        if getattr(model, "_lia_scheduler", None):
            model._lia_scheduler.close()
        model.close()
    # a Llama-family model refuses any padding by name (its RoPE positions are not per row); an all-ones mask still runs
    from lia_amd.llama import LiaLlamaModel, LlamaShape
    H, heads, kvh, F, vocab = 128, 4, 2, 256, 64
    lm = synth.make_llama_model(3, vocab, H, heads, kvh, F, 1, 0.05)
    llama = LiaLlamaModel.from_numpy(LlamaShape("t", H, heads, kvh, F, 1, vocab, max_pos=64, rope_theta=10000.0), lm)
    try:
        t = torch.from_numpy(np.array([[5, 6, 7], [8, 9, 10]], np.int64))
        with pytest.raises(ValueError, match="Llama"):
            generate(llama, t, attention_mask=torch.tensor([[0, 1, 1], [1, 1, 1]]), max_new_tokens=2, gpu_percentage=100)
        a = generate(llama, t, max_new_tokens=2, min_new_tokens=2, gpu_percentage=100)
        b = generate(llama, t, attention_mask=torch.ones_like(t), max_new_tokens=2, min_new_tokens=2, gpu_percentage=100)
        assert torch.equal(a, b)
    finally:
        if getattr(llama, "_lia_scheduler", None):
            llama._lia_scheduler.close()
        llama.close()
