"""The cooperative split's online choice of the number of host-computed decode layers (cpu_layers=-1): the pattern search over
measured decode steps (CoopController) and the file that carries a converged count to the next process (CoopStore).  Pure host logic."""
import fcntl
import json
import os


class CoopStore:
    """The converged host-layer count of a (model, batch, prompt bucket, new tokens, placement, host tier, wire format, host team)
    configuration, kept in a small JSON file -- ONLY where the user named a place for it (LIA_STATE_DIR; r04 wrote to
    ~/.cache/lia_amd unasked, so a benchmark's cooperative legs depended on whatever ran on the box before, and GPU tests wrote into
    the user's home: ADVICE r04).  The next process with the same key starts its search ON that count -- one stride-3 probe on the
    side the link points to, then +-1 -- instead of at the planner's estimate.  Best effort: without LIA_STATE_DIR, or with an
    unreadable / unwritable file, the search starts from the planner's seed and nothing is written."""

    FILE = "coop_counts.json"

    @staticmethod
    def path():
        d = os.environ.get("LIA_STATE_DIR")
        return os.path.join(d, CoopStore.FILE) if d else None

    @staticmethod
    def load(key):
        if key is None or CoopStore.path() is None:
            return None
        try:
            with open(CoopStore.path()) as f:
                e = json.load(f).get(key)
            return (int(e["count"]), float(e["ms"])) if e else None
        except (OSError, ValueError, KeyError, TypeError):
            return None

    @staticmethod
    def save(key, count, ms):
        if key is None or ms is None or CoopStore.path() is None:
            return False
        try:
            p = CoopStore.path()
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with open(p + ".lock", "w") as lk:        # read-modify-write under an exclusive lock: two processes keep each other's entries
                fcntl.flock(lk, fcntl.LOCK_EX)
                try:
                    with open(p) as f:
                        all_ = json.load(f)
                except (OSError, ValueError):
                    all_ = {}
                all_[key] = {"count": int(count), "ms": round(float(ms), 3)}
                tmp = f"{p}.{os.getpid()}.tmp"
                with open(tmp, "w") as f:
                    json.dump(all_, f, indent=1, sort_keys=True)
                os.replace(tmp, p)                    # whole-file swap: a reader never sees half a file
            return True
        except OSError:
            return False


class CoopController:
    """Online choice of the number of host-computed decode layers (`cpu_layers=-1`, build-defined cooperative split).

    r02 picked the count once from a 4-second calibration (planner.plan_cpu_layers) and landed 129 ... 177 tok/s depending on
    which socket the GPU hangs off.  Here the count follows the MEASURED decode steps: the host set of size c is the first c
    layers of a fixed nested order (`order`, every prefix spread over the streamed layers, raw host copies kept for the first
    c_max only).  A step is max(link time of the streamed layers, host + GPU time): roughly a V in c, but on a shared box the
    bottom is flat to ~1 % with +10 % spikes on single steps, and the first version (a +-1 hill climb on the last sample) walked
    away from the minimum on a spike and stalled two counts below it (results/r03_final2_*).  So this is a pattern search:
    measure the centre, then centre +- stride for stride 3, then 1 -- first on the side the copy engine's idle share points to (link
    >= 97 % busy: more host layers shorten the link time; less: the host is the bottleneck) -- moving the centre whenever a
    candidate beats it by > 0.5 % and carrying on in that direction, twice as far per move after two moves that paid (a seed far
    off; the planner's seed is usually 0-3 counts off, and strides 4 / 2 / 1 spent two steps at a count 40 % slower plus 2 GB of
    cache moves on the first probe: 3.2-3.9 % of a 31-step run in the synthetic box of tests/test_host_logic.py against 2.4-3.2 %); a count's value is the MINIMUM of its last `keep` samples
    (spikes only ever add time).  One settle step after every change (queued copies still reflect the old set).  Converged, it
    stays on the centre -- single slow steps move nothing -- and searches again (+-1 first) after `expire` steps or when six
    steps in a row run > 5 % above the value it converged on (the box changed); every `probe_every` steps it
    re-measures centre +- 1 (a spike on a candidate's single sample can end the search one or two counts off; the second look
    costs five steps at a neighbouring count and repairs that)."""

    STRIDES = (3, 1)
    UP_MIN_BUSY = 0.9             # below this copy-engine busy share no count ABOVE the centre is probed

    def __init__(self, order, start, c_max, expire=96, keep=3, probe_every=16):
        self.order, self.c_max = list(order), min(int(c_max), len(order))
        self.c = max(0, min(int(start), self.c_max))
        self.expire, self.keep, self.probe_every = expire, keep, probe_every
        self.samples = {}             # c -> [(step, ms), ...] the last `keep`
        self.busy_at = {}             # c -> copy-engine busy share of the last sampled step at c
        self.centre, self.stride_i, self.pending, self.direction, self.run = self.c, 0, None, 0, 0
        self.converged_at, self.converged_ms, self.c_conv, self.last_probe, self.probing, self.slow = None, None, None, 0, False, 0
        self.settle, self.step, self.moves, self.searches = 1, 0, 0, 1
        self.bracketed = False        # a minimum has been found once: from then on the search moves by +-1 only
        self.trace = []               # (step, c, ms, link busy share)
        self.store_key, self.seeded = None, False        # (CoopStore) where the converged count is kept across processes

    def host_set(self, c=None):
        return frozenset(self.order[:self.c if c is None else c])

    def superset(self):
        return frozenset(self.order[:self.c_max])

    def restrict(self, c_max):
        """fewer candidates than planned (the container has no room for more raw host copies)"""
        self.c_max = max(0, min(self.c_max, int(c_max)))
        clipped = self.c > self.c_max or self.centre > self.c_max
        self.c, self.centre = min(self.c, self.c_max), min(self.centre, self.c_max)
        self.samples = {k: v for k, v in self.samples.items() if k <= self.c_max}
        if self.pending:
            self.pending = [(c, d) for c, d in self.pending if c <= self.c_max]
        if clipped or self.centre not in self.samples:
            # the point the search stood on is gone (or was never measured): start over from the clipped centre -- a half-finished
            # comparison against a centre without samples would compare with None
            self.c = self.centre
            self.pending, self.direction, self.run, self.stride_i = None, 0, 0, (len(self.STRIDES) - 1 if self.bracketed else 0)
            self.converged_at, self.converged_ms, self.c_conv, self.probing, self.slow = None, None, None, False, 0
            self.settle = max(self.settle, 1)

    def new_sequence(self):
        """a new generation: its first decode step also waits for the prefill's K/V deliveries and loads layers on demand"""
        self.settle = max(self.settle, 1)

    def value(self, c):
        v = [ms for st, ms in self.samples.get(c, ()) if self.step - st <= self.expire]
        return min(v) if v else None

    def _go(self, c):
        if c != self.c:
            self.c, self.settle, self.moves = c, 1, self.moves + 1
        return self.c

    def _candidates(self, busy, again=False):
        s = self.STRIDES[self.stride_i]
        busy = self.busy_at.get(self.centre, busy)      # the copy engine's share AT THE CENTRE (the last step may have run at a candidate)
        side = (1, -1) if busy >= 0.97 else (-1, 1)
        if busy < self.UP_MIN_BUSY:
            side = (-1,)                # the link idles > 10 % of the step: the host side is the bottleneck, one more host layer cannot pay
        return [(self.centre + d * s, d) for d in side
                if 0 <= self.centre + d * s <= self.c_max and (again or self.value(self.centre + d * s) is None)]

    def observe(self, step_ms, busy_share):
        """one finished decode step at the current c -> the c of the next step"""
        self.step += 1
        self.trace.append((self.step, self.c, round(step_ms, 2), round(busy_share, 3)))
        if self.settle > 0:
            self.settle -= 1
            return self.c
        self.samples[self.c] = (self.samples.get(self.c, []) + [(self.step, step_ms)])[-self.keep:]
        self.busy_at[self.c] = busy_share
        if self.converged_at is not None and not self.probing:
            self.slow = self.slow + 1 if step_ms > 1.05 * self.converged_ms else 0
            if self.step - self.converged_at >= self.expire or self.slow >= 2 * self.keep:
                # search again around where we are, +-1 first (a move that pays carries on, twice as far after two): everything
                # measured before is stale.  (Six slow steps in a row, not three: a noise episode of 3-4 steps restarted the
                # search with a stride-3 probe 25 % off the optimum -- results/r03_final10_*.)
                self.samples = {self.c: self.samples[self.c][-1:]}
                self.centre, self.stride_i, self.pending, self.direction, self.run = self.c, len(self.STRIDES) - 1, None, 0, 0
                self.converged_at, self.searches, self.slow = None, self.searches + 1, 0
            elif self.step - self.last_probe >= self.probe_every:
                self.stride_i, self.probing = len(self.STRIDES) - 1, True
                self.pending = self._candidates(busy_share, again=True)
            else:
                return self.c
        if self.pending is None:                                  # the centre has just been measured: open this stride
            self.pending = self._candidates(busy_share)
        elif self.c != self.centre:                               # a candidate has just been measured
            if self.value(self.centre) is None:                   # the centre's samples expired / were dropped: measure it again first
                self.pending = [(self.c, self.direction)] + list(self.pending or [])
                self.direction = 0
                return self._go(self.centre)
            if self.value(self.c) < 0.995 * self.value(self.centre):
                d, s = self.direction, self.STRIDES[self.stride_i]
                self.centre, self.run = self.c, self.run + 1
                far = 2 if (self.run >= 2 and not self.bracketed) else 1
                nxt = self.centre + d * s * far                   # it paid: carry on the same way before looking back
                if d > 0 and busy_share < self.UP_MIN_BUSY:
                    nxt = self.centre
                nxt = max(0, min(self.c_max, nxt))
                self.pending = [(nxt, d)] if nxt != self.centre and self.value(nxt) is None else []
            else:
                self.run = 0
        while not self.pending:
            if self.stride_i + 1 >= len(self.STRIDES):
                if self.converged_at is None or self.centre != self.c_conv:
                    self.converged_at, self.converged_ms, self.c_conv = self.step, self.value(self.centre), self.centre
                    CoopStore.save(self.store_key, self.centre, self.converged_ms)
                self.last_probe, self.probing, self.bracketed = self.step, False, True
                return self._go(self.centre)
            self.stride_i, self.run = self.stride_i + 1, 0
            self.pending = self._candidates(busy_share)
        cand, self.direction = self.pending.pop(0)
        return self._go(cand)

    def report(self):
        return {"host_layers": self.c, "centre": self.centre, "converged": self.converged_at is not None, "max_host_layers": self.c_max,
                "seeded_from_store": self.seeded,
                "moves": self.moves, "searches": self.searches, "steps_observed": self.step,
                "ms_by_count": {str(k): round(self.value(k), 2) for k in sorted(self.samples) if self.value(k) is not None},
                "trace_tail": self.trace[-12:]}
