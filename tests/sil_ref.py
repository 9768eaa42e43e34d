"""Numpy restatement of the silence operator (the normative definition is the contract comment of ``sopro_sil_rows_f32`` in
include/sopro_hip.h).  ``squeeze`` is the one-shot form, written from the definition run by run; ``Stream`` is a causal chunk-by-chunk
model written from the streaming paragraph on its own (state = speech seen, run length, samples received, the retained hops);
``map_cuts`` / ``squeeze_cues`` restate the cue map.  tests/test_sil_host.py checks on the CPU that the two forms agree exactly;
tests/test_gpu_sil.py compares the kernels with them bit for bit.  Not imported by the package."""
import numpy as np

HOP = 240
TAB = (0.5 - 0.5 * np.cos(np.pi * (np.arange(HOP, dtype=np.float64) + 0.5) / HOP)).astype(np.float32)
TAB_R = TAB[::-1].copy()


def thr_of(floor_db):
    return np.float32(10.0 ** (float(floor_db) / 20.0))


def activity(x, thr):
    """bool per hop: max |x| over the hop >= thr (a NaN compares false)."""
    x = np.asarray(x, np.float32)
    L = len(x)
    nh = -(-L // HOP)
    pad = np.zeros(nh * HOP, np.float32)
    pad[:L] = x
    with np.errstate(invalid="ignore"):
        return (np.abs(pad).reshape(nh, HOP) >= np.float32(thr)).any(1)


def _runs(act):
    """[(j0, j1)] of the maximal stretches of inactive hops."""
    out, j, nh = [], 0, len(act)
    while j < nh:
        if act[j]:
            j += 1
            continue
        j0 = j
        while j < nh and not act[j]:
            j += 1
        out.append((j0, j))
    return out


def squeeze(x, thr, cap_h, b):
    """x [L] float32 -> (y, cuts [(source position, samples removed)])."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    L = len(x)
    if cap_h == 0:
        return x.copy(), []
    assert 1 <= b <= 16 and b + 1 <= cap_h <= 1000
    a = cap_h - b
    act = activity(x, thr)
    nh = len(act)
    if not act.any():
        return np.zeros(0, np.float32), ([(0, L)] if L else [])
    pieces, cuts, pos = [], [], 0  # pos: the source position up to which the output is made

    def hop(j):
        return x[j * HOP: (j + 1) * HOP]

    for j0, j1 in _runs(act):
        n = j1 - j0
        if j0 == 0:
            if n > b + 1:
                f = j1 - b - 1
                pieces.append(hop(f) * TAB)
                cuts.append((0, f * HOP))
                pos = (f + 1) * HOP
        elif j1 == nh:
            if n > a:
                f = j0 + a - 1
                pieces.append(x[pos: f * HOP])
                pieces.append(hop(f) * TAB_R)
                cuts.append(((j0 + a) * HOP, L - (j0 + a) * HOP))
                pos = L
        elif n > cap_h:
            p, q = j0 + a, j1 - b
            pieces.append(x[pos: (p - 1) * HOP])
            pieces.append(hop(p - 1) * TAB_R + hop(q - 1) * TAB)  # (three float32 operations, each rounded)
            cuts.append((p * HOP, (q - p) * HOP))
            pos = q * HOP
    pieces.append(x[pos:])
    return np.concatenate(pieces).astype(np.float32), cuts


class Stream:
    """The chunked form of one row: ``feed(chunk)`` -> (samples decided by this call, their cuts); ``flush()`` the rest."""

    def __init__(self, thr, cap_h, b):
        self.thr, self.cap_h, self.b = np.float32(thr), int(cap_h), int(b)
        self.a = self.cap_h - self.b
        self._fresh()

    def _fresh(self):
        self.seen = False
        self.run = 0          # inactive hops since the last active one (or since the start)
        self.hops = 0         # complete hops taken
        self.recv = 0
        self.part = np.zeros(0, np.float32)  # the incomplete hop
        self.held = None      # hop a - 1 of the current run
        self.ring = []        # the last b + 1 hops of the current run that were neither emitted nor held

    def _active(self, h):
        with np.errstate(invalid="ignore"):
            return bool((np.abs(h) >= self.thr).any())

    def _hop(self, h, out, cuts):
        j = self.hops  # this hop's index
        self.hops += 1
        b, a = self.b, self.a
        if self._active(h):
            n = self.run
            if not self.seen:
                if n <= b + 1:
                    out.extend(self.ring)
                else:
                    out.append(self.ring[0] * TAB)
                    out.extend(self.ring[1:])
                    cuts.append((0, (j - b - 1) * HOP))
                self.seen = True
            elif n >= a:
                if n <= self.cap_h:
                    out.append(self.held)
                    out.extend(self.ring)
                else:
                    out.append(self.held * TAB_R + self.ring[0] * TAB)
                    out.extend(self.ring[1:])
                    cuts.append(((j - n + a) * HOP, (n - self.cap_h) * HOP))
            out.append(h)
            self.run, self.held, self.ring = 0, None, []
            return
        r = self.run
        self.run += 1
        if self.seen and r < a - 1:
            out.append(h)
        elif self.seen and r == a - 1:
            self.held = h
        else:
            self.ring.append(h)
            del self.ring[: -(b + 1)]

    def feed(self, chunk, flush=False):
        if self.cap_h == 0:
            return np.asarray(chunk, np.float32).copy(), []
        buf = np.concatenate([self.part, np.asarray(chunk, np.float32)])
        self.recv += len(chunk)
        out, cuts = [], []
        k = len(buf) // HOP
        for i in range(k):
            self._hop(buf[i * HOP: (i + 1) * HOP], out, cuts)
        self.part = buf[k * HOP:]
        if flush:
            if len(self.part):
                self._hop(self.part, out, cuts)
            if not self.seen:
                if self.recv:
                    cuts.append((0, self.recv))
            elif self.run == self.a:
                out.append(self.held)
            elif self.run > self.a:
                out.append(self.held * TAB_R)
                at = (self.hops - self.run + self.a) * HOP
                cuts.append((at, self.recv - at))
            self._fresh()
        y = np.concatenate(out).astype(np.float32) if out else np.zeros(0, np.float32)
        return y, cuts

    def flush(self):
        return self.feed(np.zeros(0, np.float32), flush=True)


def stream_all(x, sizes, thr, cap_h, b):
    """x fed in chunks of ``sizes`` (cycled), then a flush -> (concatenated output, all cuts)."""
    st = Stream(thr, cap_h, b)
    ys, cuts, at, k = [], [], 0, 0
    while at < len(x):
        n = int(sizes[k % len(sizes)])
        y, c = st.feed(x[at: at + n])
        ys.append(y)
        cuts += c
        at += n
        k += 1
    y, c = st.flush()
    ys.append(y)
    cuts += c
    return np.concatenate(ys), cuts


def map_cuts(sample, cuts):
    """A sample position of the input -> its position in the output: a position inside a removed range maps to the cut's start."""
    s, off = int(sample), 0
    for pos, n in cuts:
        if s >= pos + n:
            off += n
        elif s > pos:
            return pos - off
        else:
            break
    return s - off


def squeeze_cues(cues, cuts):
    return [c._replace(start_sample=map_cuts(c.start_sample, cuts), end_sample=map_cuts(c.end_sample, cuts)) for c in cues]


def bursts(pattern, tail=0, amp=0.5, noise=1e-3, seed=0):
    """A signal from (kind, hops) pairs, kind 's' (a 220 Hz sine at ``amp`` plus noise: every hop of it is active at any floor below
    ``amp``) or 'g' (noise at ``noise``: inactive at any floor above ~5 ``noise``), and ``tail`` more samples of the last kind."""
    rng = np.random.default_rng(seed)
    n = sum(h for _k, h in pattern) * HOP + tail
    x = (rng.standard_normal(n) * noise).clip(-4 * noise, 4 * noise)
    t = np.arange(n)
    on = np.zeros(n, bool)
    at = 0
    for i, (k, h) in enumerate(pattern):
        m = h * HOP + (tail if i == len(pattern) - 1 else 0)
        on[at: at + m] = k == "s"
        at += m
    x = x + on * amp * np.sin(2 * np.pi * 220.0 * t / 24000.0 + 0.3)
    return x.astype(np.float32)


def designed_batch(plan_hops=4096):
    """The ragged batch of the tests: [(x, thr, cap_h, b)] - gaps at every boundary length of the definition, an identity row, an
    all-silent row, an empty row, two parameter sets more, and one row of more than ``plan_hops`` hops (what the plan kernel's
    workgroup takes per pass).  Rows 0 and 4 are the ones a stride of 1 mod 4 leaves 16-byte aligned."""
    S, G = "s", "g"
    thr, cap, b = np.float32(0.05), 4, 2  # a = 2
    rows = []
    # 0: leading b + 2 (cut), interior cap (kept) and cap + 1 (cut), a long one, trailing a + 1 (cut) ending in an inactive partial hop
    rows.append((bursts([(G, b + 2), (S, 3), (G, cap), (S, 2), (G, cap + 1), (S, 1), (G, 12), (S, 2), (G, 2)], tail=HOP + 100, seed=1), thr, cap, b))
    # 1: leading b + 1 (kept), a one-hop gap, a long gap, trailing a (kept), a whole number of hops
    rows.append((bursts([(G, b + 1), (S, 2), (G, 1), (S, 1), (G, 30), (S, 4), (G, cap - b)], seed=2), thr, cap, b))
    # 2: a = 1 (cap_h = b + 1) at another floor: interior cap and cap + 1, a trailing run of two hops (cut)
    rows.append((bursts([(S, 1), (G, 3), (S, 2), (G, 4), (S, 1), (G, 9), (S, 3), (G, 2)], seed=3), np.float32(0.1), 3, 2))
    # 3: about 30 k samples at the default-like (30, 3): gaps of 31 (cut) and 30 (kept), an active partial last hop; one sample at
    #    exactly the floor makes a silent hop active, a NaN does not
    x = bursts([(G, 10), (S, 5), (G, 31), (S, 7), (G, 30), (S, 6), (G, 34), (S, 1)], tail=77, seed=4)
    t3 = np.float32(0.02)
    x[(15 + 12) * HOP + 5] = -t3       # splits the 31-hop gap: 12 | active | 18
    x[(10 + 5 + 31 + 7 + 30 + 6 + 15) * HOP + 9] = np.nan  # inside the 34-hop gap, which is still cut
    rows.append((x, t3, 30, 3))
    # 4: the long row: more hops than one pass of the plan workgroup, gaps and bursts of many lengths across the word boundaries
    rng = np.random.default_rng(5)
    pat, hops, k = [(G, 7)], 7, 0
    while hops < plan_hops + 300:
        h = int(rng.integers(1, 9)) if k % 2 == 0 else int(rng.choice([1, 2, 5, 6, 7, 20, 63, 64, 65, 130]))
        pat.append((S if k % 2 == 0 else G, h))
        hops += h
        k += 1
    rows.append((bursts(pat, tail=17, seed=6), thr, 6, 2))
    # 5: identity, 6: all silent, 7: empty
    rows.append((bursts([(G, 5), (S, 2), (G, 9)], tail=3, seed=7), thr, 0, 1))
    rows.append((bursts([(G, 11)], tail=50, seed=8), thr, cap, b))
    rows.append((np.zeros(0, np.float32), thr, cap, b))
    return rows
