"""Turn-by-turn reference of a multi-turn generation, composed from the oracle's own calls: embed / layer_forward / lm_head for
OPT, llama_layer_forward / the Llama lm_head for a Llama.  NumPy + the CPU oracle, no GPU.

A conversation is a prompt [B, T], follow-ups [B, T2_i] and new-token counts m_i.  Turn 0 prefills the prompt and decodes; turn i > 0
feeds the block [pending | follow-up i] -- pending = the last generated token, which no forward has consumed yet -- at position
`past` (the cached length), then decodes.  Per-layer policy of a forward, as the schedulers choose it: layers below n_gpu run
policy 3; the others the prefill policy for a multi-token forward on an empty cache, `append_policy` (default: the prefill policy)
for a multi-token forward on a non-empty one, the decoding policy for one token -- policy 1 there for the fixed host set of
cpu_layers.  Greedy, no EOS handling (the tests pass eos_token_id=None)."""
import numpy as np

import synth


class OptRef:
    def __init__(self, oracle, model, heads, B, smax, prefill_policy=1, decoding_policy=1, gpu_percentage=0, append_policy=None,
                 host_layers=(), **_other):
        self.o, self.m, self.heads, self.B = oracle, model, heads, B
        L = len(model["layers"])
        H = model["embed_tokens"].shape[1]
        self.n_gpu = int(L * gpu_percentage / 100)
        self.pp, self.dp = prefill_policy, decoding_policy
        self.ap = prefill_policy if append_policy is None else append_policy
        self.host = frozenset(host_layers)
        self.kcs = [np.zeros((smax, B, heads, H // heads), np.uint16) for _ in range(L)]
        self.vcs = [np.zeros((smax, B, heads, H // heads), np.uint16) for _ in range(L)]
        self.past = 0

    def _policy(self, li, T):
        if li < self.n_gpu:
            return 3
        if T == 1:
            return 1 if li in self.host else self.dp
        return self.pp if self.past == 0 else self.ap

    def hidden(self, cur, caches=None):
        """the last layer's output [B, T, H] of the block `cur` at position `past`; caches: (kcs, vcs) to write instead of the live ones"""
        kcs, vcs = caches or (self.kcs, self.vcs)
        hid = self.o.embed(cur, self.m["embed_tokens"], self.m["embed_positions"], self.past)
        for li, W in enumerate(self.m["layers"]):
            hid = self.o.layer_forward(self._policy(li, cur.shape[1]), W, hid, kcs[li], vcs[li], self.past, self.heads)
        return hid

    def logits_of(self, hid):
        """bf16 logits [rows, vocab] of every row of hid [.., H]"""
        H = hid.shape[-1]
        return self.o.lm_head(np.ascontiguousarray(hid.reshape(-1, 1, H)), self.m["final_ln_w"], self.m["final_ln_b"], self.m["embed_tokens"])[0]

    def forward(self, cur):
        hid = self.hidden(cur)
        logits, nxt = self.o.lm_head(hid, self.m["final_ln_w"], self.m["final_ln_b"], self.m["embed_tokens"])
        self.past += cur.shape[1]
        return logits, nxt

    def score_block(self, cur):
        """bf16 logits [B, T, vocab] of every position of the block appended at `past`, the caches and `past` left as they are"""
        copies = ([k.copy() for k in self.kcs], [v.copy() for v in self.vcs])
        hid = self.hidden(cur, copies)
        return self.logits_of(hid).reshape(cur.shape[0], cur.shape[1], -1)


class LlamaRef:
    def __init__(self, oracle, model, heads, kv_heads, theta, B, smax, eps=1e-5):
        self.o, self.m, self.heads, self.kvh, self.eps, self.B = oracle, model, heads, kv_heads, eps, B
        H = model["embed_tokens"].shape[1]
        d = H // heads
        self.cos, self.sin = oracle.rope_tables(smax, d, theta)
        L = len(model["layers"])
        self.kcs = [np.zeros((smax, B, kv_heads, d), np.uint16) for _ in range(L)]
        self.vcs = [np.zeros((smax, B, kv_heads, d), np.uint16) for _ in range(L)]
        self.past = 0

    def hidden(self, cur, caches=None):
        kcs, vcs = caches or (self.kcs, self.vcs)
        hid = np.ascontiguousarray(self.m["embed_tokens"][cur])
        for li, W in enumerate(self.m["layers"]):
            hid = self.o.llama_layer_forward(W, hid, kcs[li], vcs[li], self.cos, self.sin, self.past, self.heads, self.kvh, self.eps)
        return hid

    def _lm(self, hid, T):
        o = self.o
        rows, H, vocab = hid.shape[0], hid.shape[-1], self.m["lm_head"].shape[0]
        logits, nxt = np.empty((rows, vocab), np.uint16), np.empty((rows,), np.int64)
        o._llama_lib().lia_oracle_llama_lm_head(o._p(o._c(hid)), o._p(o._c(self.m["final_norm_w"])), o._p(o._c(self.m["lm_head"])),
                                                o._p(logits), o._p(nxt), rows, T, H, vocab, self.eps)
        return logits, nxt

    def logits_of(self, hid):
        return self._lm(np.ascontiguousarray(hid.reshape(-1, 1, hid.shape[-1])), 1)[0]

    def forward(self, cur):
        hid = self.hidden(cur)
        logits, nxt = self._lm(hid, cur.shape[1])
        self.past += cur.shape[1]
        return logits, nxt

    def score_block(self, cur):
        copies = ([k.copy() for k in self.kcs], [v.copy() for v in self.vcs])
        return self.logits_of(self.hidden(cur, copies)).reshape(cur.shape[0], cur.shape[1], -1)


def converse(ref, prompt, followups, new_tokens):
    """-> [(ids [B, n] of the whole conversation after turn i, [bf16 logits [B, vocab] of each of its steps])]"""
    ids = np.ascontiguousarray(prompt, dtype=np.int64)
    cur, out = ids, []
    for i, m_new in enumerate(new_tokens):
        if i > 0:
            fu = np.ascontiguousarray(followups[i - 1], dtype=np.int64).reshape(ids.shape[0], -1)
            cur = np.concatenate([ids[:, -1:], fu], axis=1)
            ids = np.concatenate([ids, fu], axis=1)
        steps = []
        for _ in range(m_new):
            logits, nxt = ref.forward(cur)
            steps.append(logits)
            ids = np.concatenate([ids, nxt[:, None]], axis=1)
            cur = nxt[:, None]
        out.append((ids.copy(), steps))
    return out


def near_tie_rows(turns):
    """rows whose oracle top-2 logit gap is within two bf16 quanta of the row's largest logit at ANY step of ANY turn -- the rows
    parity_util.ids_equal_or_near_tie would excuse from their divergent step on"""
    rows = None
    for _, steps in turns:
        for lg in steps:
            f = synth.bf16_bits_to_f32(lg)
            top2 = np.sort(f, -1)[:, -2:]
            q = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(f).max(-1), 1e-30))) - 7)
            tie = (top2[:, 1] - top2[:, 0]) <= 2 * q
            rows = tie if rows is None else rows | tie
    return np.flatnonzero(rows)
