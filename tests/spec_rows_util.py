"""What the row-mode tests of speculative decoding share: the ReplayDrafter script that gives the rows different counts in every round,
and the host-side replay that predicts the target passes a script needs.  NumPy-free, no GPU."""


def script(k, rounds=12, rows=8):
    """round r: row r % rows fully wrong, row (r + 1) % rows right to the end, the rest in between -- different counts in every round"""
    return [[0 if b == r % rows else (None if b == (r + 1) % rows else (r + 2 * b) % (k + 1)) for b in range(rows)] for r in range(rounds)]


def replay(scr, k, rows, new, mode):
    """target passes a script needs: 1 (the prefill) + the rounds until every row holds `new` tokens"""
    want = lambda r: [k if a is None else min(a, k) for a in (scr[r] if r < len(scr) and scr[r] is not None else [None] * rows)]
    g, r = [1] * rows, 0
    while min(g) < new:
        w = want(r)
        if mode == "common":
            g = [v + min(w) + 1 for v in g]
        else:
            g = [v if v >= new else min(new, v + a + 1) for v, a in zip(g, w)]
        r += 1
    return 1 + r
