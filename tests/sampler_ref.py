"""Host reference of the sampler and the autoregressive driver state (csrc/ar_driver.hip: ar_init_kernel, ar_sample_kernel,
ar_admit_kernel), in plain numpy.  No GPU; torch only as the seeded generator of the fixtures' logits at the end of the file.

What is reproducible bit for bit is done in float32 exactly as the kernel does it: nan_to_num, the temperature division, the
repetition penalty (IEEE division and multiplication, one rounding each) and the next input cond[t + 1] + emb[tok] (one add).
Everything after that - ordering, softmax over the top kk, the cumulative mass, the top-p cut, the draw - is float64.

The uniform of a draw is not random from here: the generator is the published Philox4x32-10 (Salmon et al., "Parallel random
numbers: as easy as 1, 2, 3", SC'11) with counter (t, row_id, 0x5090, nonce) and key (seed low word, seed high word);
u = (word 0 >> 8) * 2^-24.  `philox4x32_10` is written from the paper and checked against its known-answer vectors in
tests/test_sampler_ref.py.

A draw is `draw(dist, u)`: the first kept entry j with u * kept < edge[j + 1].  `margin` is the distance from u * kept to the
nearest edge between two kept entries; a float32 evaluation may land on the other side of that edge when the margin is below its
rounding error (the bound M is derived in tests/test_gpu_sampler_edges.py), and on no other entry.

`decide` says what one row does in one frame without changing the state; `commit` applies it with the token that was actually
emitted (the reference's own, or a device's when the test follows the device through a chained run).  `step` is both."""
import numpy as np

RECENT = 64      # slots of the rolling token window; slot j = the token sampled j + 1 frames ago, -1 = none
WINDOW = 50      # slots the repetition penalty looks at
KMAX = 64        # largest top-k the sampling path serves; above it (or "no top-k" on a larger vocabulary) the arg-max
COUNTER_TAG = 0x5090
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter4, key2):
    """Philox4x32 with ten rounds.  counter4 / key2: unsigned 32-bit words (scalars or arrays that broadcast).  Returns four
    uint64 arrays holding the 32-bit output words."""
    c = [np.asarray(v, dtype=np.uint64) & _M32 for v in counter4]
    k = [np.asarray(v, dtype=np.uint64) & _M32 for v in key2]
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]       # 32 x 32 -> 64 bits: no overflow in uint64
        h0, l0, h1, l1 = p0 >> _S32, p0 & _M32, p1 >> _S32, p1 & _M32
        c = [h1 ^ c[1] ^ k[0], l1, h0 ^ c[3] ^ k[1], l0]
        k = [(k[0] + w0) & _M32, (k[1] + w1) & _M32]
    return tuple(c)


def uniform(seed, t, row_id, nonce):
    """The sampler's uniform in [0, 1): a multiple of 2^-24, exact in float32 and float64.  t / row_id / nonce may be arrays."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c0 = philox4x32_10((t, row_id, COUNTER_TAG, nonce), (seed & 0xFFFFFFFF, seed >> 32))[0]
    return (c0 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def window_ids(window, V1):
    """The token ids the repetition penalty applies to: slots 0 .. 49, entries in [0, V1), each once."""
    w = np.asarray(window, dtype=np.int64)[:WINDOW]
    return np.unique(w[(w >= 0) & (w < V1)])


def penalised(logits, window, temp, rep, V1):
    """nan_to_num -> temperature -> repetition penalty, in float32 and in that order (the first three steps of sample_token;
    oracle.penalised_logits with the history given as the 64-slot window)."""
    x = np.array(np.asarray(logits, dtype=np.float32)[:V1], dtype=np.float32, copy=True)
    x[np.isnan(x)] = np.float32(-1e9)
    x[x == np.inf] = np.float32(1e9)
    x[x == -np.inf] = np.float32(-1e9)
    temp, rep = np.float32(temp), np.float32(rep)
    if temp != 0 and temp != 1:
        x = x / temp
    if rep != 1:
        ids = window_ids(window, V1)
        v = x[ids]
        x[ids] = np.where(v < 0, v * rep, v / rep)
    return x


class Dist:
    """The sampling distribution of one frame.  order / p: the top kk tokens in rank order and their probabilities over the top kk;
    tokens: the kept prefix; edges: 0 and the cumulative mass behind every kept entry (edges[-1] = kept mass)."""
    __slots__ = ("order", "p", "kk", "tokens", "edges", "kept", "cut_margin")


def distribution(x32, top_p, top_k):
    """Top-k, renormalisation and the top-p cut of the penalised logits, in float64."""
    x = np.asarray(x32, dtype=np.float64)
    V1 = x.shape[0]
    kk = min(int(top_k), V1) if top_k > 0 else V1
    order = np.lexsort((np.arange(V1), -x))[:kk]      # value descending, then index ascending
    e = np.exp(x[order] - x[order[0]])
    p = e / e.sum()
    before = np.concatenate(([0.0], np.cumsum(p)[:-1]))
    top_p = float(top_p)
    keep = np.ones(kk, dtype=bool)
    d = Dist()
    d.cut_margin = float("inf")
    if top_p < 1.0:
        keep[1:] = ~(before[1:] > top_p)
        if kk > 1:
            d.cut_margin = float(np.abs(before[1:] - top_p).min())
    n = int(keep.sum())  # `before` grows with j, so the kept entries are a prefix
    assert keep[:n].all()
    d.order, d.p, d.kk = order, p, kk
    d.tokens = order[:n]
    d.edges = np.concatenate(([0.0], np.cumsum(p[:n])))
    d.kept = float(d.edges[-1])
    return d


def draw_many(dist, u):
    """Vector form of `draw`: arrays (token, margin, lower_neighbour, upper_neighbour) for an array of uniforms."""
    u = np.atleast_1d(np.asarray(u, dtype=np.float64))
    x = u * dist.kept
    n = dist.tokens.shape[0]
    j = np.minimum(np.searchsorted(dist.edges[1:], x, side="right"), n - 1)  # first j with x < edges[j + 1], else the last kept
    tok = dist.tokens[j]
    if n == 1:
        return tok, np.full(u.shape, np.inf), tok.copy(), tok.copy()
    inner = dist.edges[1:-1]                     # inner[i] separates kept entries i and i + 1
    i = np.clip(np.searchsorted(inner, x), 0, n - 2)
    i = np.where((i > 0) & (np.abs(x - inner[np.maximum(i - 1, 0)]) <= np.abs(x - inner[i])), i - 1, i)
    return tok, np.abs(x - inner[i]), dist.tokens[i], dist.tokens[i + 1]


def draw(dist, u):
    """(token, margin, lower_neighbour, upper_neighbour): the token the uniform u selects, the distance from u * kept to the nearest
    edge between two kept entries (inf when one entry is kept) and the two entries that edge separates."""
    tok, m, lo, hi = draw_many(dist, u)
    return int(tok[0]), float(m[0]), int(lo[0]), int(hi[0])


def repeated_window(window):
    """The anti-loop rule on the window: a tail of n in 3 .. 16 tokens that repeats the n before it (which needs 2n valid slots),
    or 9 equal newest tokens."""
    w = np.asarray(window, dtype=np.int64)
    for n in range(3, 17):
        if w[2 * n - 1] >= 0 and np.array_equal(w[:n], w[n:2 * n]):
            return True
    return bool(w[8] >= 0 and (w[:9] == w[0]).all())


def policy(window, prm, V1):
    """(recover, top_p, temp, kk, sampling) of one frame.  prm: the eight float32 parameters (top_p, temperature, anti_loop,
    recovery top_p, recovery temperature, repetition penalty, top_k, min_gen).  `sampling` is False - the token is the arg-max of
    the penalised logits, ties to the lower index - for top_p <= 0 and for kk > 64 (top_k above 64, or no top-k on more than 64
    logits)."""
    prm = np.asarray(prm, dtype=np.float32)
    recover = bool(prm[2] != 0) and repeated_window(window)
    top_p, temp = (prm[3], prm[4]) if recover else (prm[0], prm[1])
    top_k = int(prm[6])
    kk = min(top_k, V1) if top_k > 0 else V1
    return recover, float(top_p), float(temp), kk, bool(top_p > 0) and kk <= KMAX


class State:
    """The driver state of B rows as numpy arrays (the buffers of sopro_ar_state).  Classic mode: start is None.  Slot mode:
    start [B] (-1 = free), optional row_max [B] and row_params [B, 8].  Words nothing has written yet hold `junk`."""

    def __init__(self, B, D, Tar, max_steps, V, bos_row, cond, emb, params, *, seed=0, key=None, nonce=None, row_id=None,
                 slot=False, row_max=None, row_params=None, junk=0x0BADBEEF):
        i32 = lambda *s: np.full(s, junk, dtype=np.int32)  # noqa: E731
        self.B, self.D, self.Tar, self.max_steps, self.V, self.bos_row = B, D, Tar, max_steps, V, bos_row
        self.cond = np.asarray(cond, dtype=np.float32).reshape(B, Tar, D)
        self.emb = np.asarray(emb, dtype=np.float32)
        self.params = np.asarray(params, dtype=np.float32).copy()
        self.seed, self.key = int(seed), (None if key is None else np.asarray(key, dtype=np.uint32).copy())
        self.nonce = None if nonce is None else np.asarray(nonce, dtype=np.uint32).copy()
        self.row_id = None if row_id is None else np.asarray(row_id, dtype=np.int32).copy()
        self.row_max = None if row_max is None else np.asarray(row_max, dtype=np.int32).copy()
        self.row_params = None if row_params is None else np.asarray(row_params, dtype=np.float32).reshape(B, 8).copy()
        self.x_cur = np.full((B, D), 0.5, dtype=np.float32)
        self.hist, self.recent = i32(B, max_steps), i32(B, RECENT)
        self.first_eos, self.stop_t, self.row_step = i32(B), i32(B), i32(B)
        self.ctr = i32(2)                      # [step, n_stopped]
        self.start = i32(B) if slot else None

    @property
    def step(self):
        return int(self.ctr[0])

    @property
    def n_stopped(self):
        return int(self.ctr[1])

    def seed64(self):
        return self.seed if self.key is None else int(self.key[0]) | (int(self.key[1]) << 32)

    def row_prm(self, b):
        return self.row_params[b] if self.row_params is not None else self.params


def init(st):
    """sopro_ar_init: x_cur = cond[:, 0] + emb[bos_row], flags and windows reset, every slot free, counters zero.  hist stays."""
    st.x_cur[:] = st.cond[:, 0] + st.emb[st.bos_row][None]
    st.first_eos[:] = -1
    st.stop_t[:] = -1
    st.recent[:] = -1
    if st.start is not None:
        st.start[:] = -1
    st.row_step[:] = 0
    st.ctr[:] = 0


def admit(st, row):
    """sopro_ar_admit: (re)start `row` at the current global frame."""
    assert st.start is not None and 0 <= row < st.B
    st.x_cur[row] = st.cond[row, 0] + st.emb[st.bos_row]
    st.recent[row] = -1
    st.first_eos[row] = -1
    st.stop_t[row] = -1
    st.start[row] = st.ctr[0]


class Decision:
    """What row b does in one frame.  mode: 'done' (classic mode, the loop is over: nothing is written), 'idle' (a free slot or a
    row past its budget: row_step ticks, nothing else), 'greedy' or 'sample'.  tok: the reference's token; for a sampled frame u,
    dist, margin, lo, hi as in `draw` and `allowed(M)` the tokens a float32 evaluation may return."""
    __slots__ = ("b", "mode", "tg", "t", "tmax", "recover", "top_p", "temp", "kk", "x32", "tok", "u", "dist", "margin", "lo", "hi",
                 "min_gen")

    def allowed(self, M):
        if self.mode == "sample" and self.margin < M:
            return {self.lo, self.hi}
        return {self.tok}


_dist_cache = {}


def _distribution_cached(x32, top_p, top_k):
    key = (x32.tobytes(), float(top_p), int(top_k))
    d = _dist_cache.get(key)
    if d is None:
        if len(_dist_cache) >= 64:
            _dist_cache.clear()
        d = _dist_cache[key] = distribution(x32, top_p, top_k)
    return d


def decide(st, b, logits_row, u=None):
    """The decision of row b for this frame from the current state and its logits row ([>= V + 1] float32).  Changes nothing.
    u: the frame's uniform if the caller has computed it already (decide_frame does, for all rows at once)."""
    d = Decision()
    V1 = st.V + 1
    d.b, d.tg = b, int(st.row_step[b])
    slot = st.start is not None
    s0 = int(st.start[b]) if slot else 0
    d.t = d.tg - s0
    d.tmax = int(st.row_max[b]) if (slot and st.row_max is not None) else st.Tar
    d.tok = d.u = d.dist = d.x32 = None
    d.margin, d.lo, d.hi, d.recover = float("inf"), None, None, False
    if not slot and d.tg >= st.max_steps:
        d.mode = "done"
        return d
    if slot and (s0 < 0 or d.t >= min(d.tmax, st.max_steps)):
        d.mode = "idle"
        return d
    prm = st.row_prm(b)
    d.min_gen = int(prm[7])
    d.recover, d.top_p, d.temp, d.kk, sampling = policy(st.recent[b], prm, V1)
    d.x32 = penalised(logits_row, st.recent[b], d.temp, prm[5], V1)
    if not sampling:
        d.mode, d.tok = "greedy", int(np.argmax(d.x32))  # the first maximum: ties to the lower index
        return d
    d.mode = "sample"
    if u is None:
        rid = b if st.row_id is None else int(st.row_id[b])
        nonce = 0 if st.nonce is None else int(st.nonce[b])
        u = float(uniform(st.seed64(), d.t & 0xFFFFFFFF, rid & 0xFFFFFFFF, nonce))
    d.u = float(u)
    d.dist = _distribution_cached(d.x32, d.top_p, d.kk)
    d.tok, d.margin, d.lo, d.hi = draw(d.dist, d.u)
    return d


def commit(st, d, tok=None):
    """Apply decision d with the emitted token (default: the reference's own)."""
    b = d.b
    if d.mode == "done":
        return
    if d.mode != "idle":
        tok = d.tok if tok is None else int(tok)
        t = d.t
        if t + 1 < d.tmax:
            st.x_cur[b] = st.cond[b, t + 1] + st.emb[tok]
        st.recent[b, 1:] = st.recent[b, :-1].copy()
        st.recent[b, 0] = tok
        st.hist[b, t] = tok
        if tok == st.V:
            if st.first_eos[b] < 0:
                st.first_eos[b] = t
            if st.stop_t[b] < 0 and t + 1 >= d.min_gen:
                st.stop_t[b] = t
                st.ctr[1] += 1
    st.row_step[b] = d.tg + 1
    if b == 0:
        st.ctr[0] = d.tg + 1   # the global frame counter follows row 0, also while row 0 is a free slot


def step(st, b, logits_row):
    """One frame of row b: decide and commit the reference's own token."""
    d = decide(st, b, logits_row)
    commit(st, d)
    return d


def decide_frame(st, logits):
    """decide() for every row of one launch (logits [B, >= V + 1]); the uniforms of all rows come from one vector Philox call."""
    slot = st.start is not None
    tg = st.row_step.astype(np.int64)
    t = tg - (st.start.astype(np.int64) if slot else 0)
    rid = np.arange(st.B) if st.row_id is None else st.row_id.astype(np.int64)
    nonce = np.zeros(st.B, dtype=np.int64) if st.nonce is None else st.nonce.astype(np.int64)
    u = uniform(st.seed64(), t & 0xFFFFFFFF, rid & 0xFFFFFFFF, nonce)
    return [decide(st, b, logits[b], u=u[b]) for b in range(st.B)]


# --------------------------------------------------------------------------------------------------------------- the fixtures
# Shared by tests/test_sampler_ref.py (which asserts, on the CPU, every condition a fixture must meet) and
# tests/test_gpu_sampler_edges.py (which runs them on the device).
M = 2e-5            # ambiguity margin on cumulative probability; derived in the docstring of tests/test_gpu_sampler_edges.py
AMBIGUOUS_CAP = 0.01
SEED = 7
PARAM_SETS = [(0.9, 1.05, 50, 2.0), (0.6, 0.9, 50, 4.0), (1.0, 1.0, 8, 1.0), (0.97, 1.3, 64, 0.3), (0.9, 1.0, 50, -1.0)]


def randn(*shape, seed=0, scale=1.0):
    """torch's seeded normal generator (the logits of the parameter sets are those of tests/test_gpu_ops.py)."""
    import torch
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).numpy().astype(np.float32)


def params8(top_p, temp, anti=False, min_gen=12, rec_p=0.85, rec_t=1.2, rep=1.1, top_k=50):
    return np.asarray([top_p, temp, 1.0 if anti else 0.0, rec_p, rec_t, rep, float(top_k), float(min_gen)], dtype=np.float32)


def hist_window(hist):
    """A chronological token list as the 64-slot window."""
    w = np.full(RECENT, -1, dtype=np.int32)
    h = list(hist)[::-1][:RECENT]
    w[:len(h)] = h
    return w


def plateau_tokens(N, layout, V1=2049):
    if layout == "first":
        return np.arange(N)
    if layout == "stride16":
        return (np.arange(N) * 16 + 3) % V1   # every q row and every wave; entry 128 wraps to token 2
    if layout == "stride4":
        return np.arange(N) * 4 + 3           # sixteen threads of every wave per q row
    raise ValueError(layout)


def param_set_logits(scale, V1=2049):
    base = randn(V1, seed=310, scale=abs(scale))
    if scale < 0:
        base[:200] = (10.0 - 1e-3 * np.arange(200)).astype(np.float32)   # a crowded head: more than 128 candidates
    else:
        base[7] = base[11] = np.float32(float(base.max()) + 0.5)          # an exact tie at the head
    return base


def exact_draw_cases(golden_sampler):
    """name -> dict(V, B, frames, logits [V + 1] float32, top_p, temp, top_k, rep, window (None, or the 64 slots every frame
    starts from), chained, exact_cut (the cut sits ON an edge that float32 represents exactly: no cut margin to ask for),
    path ('fast' / 'lds' / None: the ranking path the fixture is built to take), kept (None or the expected kept tokens))."""
    cases = {}

    def add(name, logits, top_p, temp, top_k, *, V=2048, B=64, rep=1.0, window=None, chained=False, exact_cut=False, path=None,
            kept=None):
        logits = np.asarray(logits, dtype=np.float32)
        assert logits.shape == (V + 1,)
        cases[name] = dict(V=V, B=B, frames=32, logits=logits, top_p=top_p, temp=temp, top_k=top_k, rep=rep, window=window,
                           chained=chained, exact_cut=exact_cut, path=path, kept=kept)

    V1 = 2049
    for i, (top_p, temp, top_k, scale) in enumerate(PARAM_SETS):
        add(f"set{i}", param_set_logits(scale), top_p, temp, top_k, path="lds" if scale < 0 else "fast")
    for ci, (top_p, temp, top_k, _scale) in enumerate(golden_sampler["cases"].tolist()):
        add(f"golden{ci}", golden_sampler[f"logits{ci}"], top_p, temp, int(top_k), rep=1.1,
            window=hist_window(golden_sampler[f"hist{ci}"].tolist()))
    # the window is the sampler's own output: 2 048 different penalised distributions.  top_p = 1: among so many distributions
    # some entry's mass always lands within 10 M of any cut, and which ones depends on the tokens drawn; the cut has the cases
    # above (the golden ones with the penalty in force)
    add("chained", randn(V1, seed=340, scale=2.0), 1.0, 1.05, 50, rep=1.1, chained=True)
    # a tied plateau of exactly N top logits, the rest 20 below.  The bound reaches the plateau only where every wave has
    # ceil(kk / 4) threads on it: 'stride16' with top_k 16 and 'stride4' with top_k 50 give exactly N candidates (64: no second
    # slot; 65: the first lane + 64 slot; 128: the full register path; 129: the first size on the LDS path), 'first' (tokens
    # 0 .. N-1, all in wave 0 or waves 0 and 1) drops the other waves' bounds to the rest: all 2049 logits are candidates.
    for N in (64, 65, 128, 129):
        for layout, top_k in (("first", 50), ("stride16", 16), ("stride4", 50)):
            x = np.full(V1, -15.0, dtype=np.float32)
            toks = plateau_tokens(N, layout)
            x[toks] = 5.0
            add(f"plateau{N}_{layout}", x, 1.0, 1.0, top_k, kept=np.sort(toks)[:top_k],
                path="lds" if (layout == "first" or N > 128) else "fast")
    # the top 50 all in wave 0's threads: the other waves' bounds are low and the candidate superset is large
    x = randn(V1, seed=341, scale=1.0)
    own = np.asarray([q * 256 + l for q in range(8) for l in range(0, 64, 9)])[:50]
    x[own] = (8.0 - 0.05 * np.arange(50)).astype(np.float32)
    add("top50_in_one_wave", x, 0.85, 1.0, 50, path="fast")
    # (256 draws: the 1 % cap is two.  top_p = 0.95 puts three of these uniforms within M of an edge j / 50, 0.93 none)
    add("all_equal", np.full(V1, 1.25, dtype=np.float32), 0.93, 1.0, 50, B=8, path="lds", kept=np.arange(47))
    add("all_nan", np.full(V1, np.nan, dtype=np.float32), 1.0, 0.7, 50, B=8, path="lds", kept=np.arange(50))
    x = randn(V1, seed=342, scale=2.0)
    x[[100, 900]] = np.inf
    add("two_posinf", x, 0.9, 1.0, 50, kept=np.asarray([100, 900]))   # both 1e9: the lower index first, .5 each, the rest cut
    base = randn(V1, seed=343, scale=2.0)
    add("top_k_1", base, 0.9, 1.05, 1, kept=np.asarray([int(np.argmax(base))]))
    add("top_p_1e-6", base, 1e-6, 1.05, 50, kept=np.asarray([int(np.argmax(base))]))
    add("top_k_65", base, 0.9, 1.05, 65)
    add("top_k_0", base, 0.9, 1.05, 0)
    # the exact cut boundary: four equal top logits, all others at -1e9 -> before = .25, .5, .75 exactly, also in float32
    x = np.full(V1, -1e9, dtype=np.float32)
    x[[5, 300, 301, 2048]] = 3.0
    add("cut_at_half", x, 0.5, 1.0, 50, exact_cut=True, kept=np.asarray([5, 300, 301]))
    add("cut_below_half", x, float(np.nextafter(np.float32(0.5), np.float32(0))), 1.0, 50, exact_cut=True, kept=np.asarray([5, 300]))
    # small and ragged vocabularies
    add("V1000", randn(1001, seed=354, scale=2.0), 0.9, 1.05, 50, V=1000)   # (seed 344 puts an entry 7e-6 from the cut)
    add("V100", randn(101, seed=345, scale=2.0), 0.9, 1.05, 50, V=100)
    add("V20_top_k_50", randn(21, seed=346, scale=1.0), 0.97, 1.0, 50, V=20)
    return cases


def case_nonces(B, salt=0):
    return (np.arange(B, dtype=np.uint32) * np.uint32(7919) + np.uint32(13 + salt)).astype(np.uint32)


def case_state(c, D=72, salt=0, **kw):
    """The classic-mode State of an exact-draw case: distinct per-row nonces, key SEED, frames + 1 conditioning rows."""
    B, V, T = c["B"], c["V"], c["frames"] + 1
    st = State(B, D, T, T, V, V + 1, randn(B, T, D, seed=90), randn(V + 2, D, seed=91),
               params8(c["top_p"], c["temp"], rep=c["rep"], top_k=c["top_k"]), seed=SEED, nonce=case_nonces(B, salt), **kw)
    init(st)
    return st


def case_logits(c):
    return np.broadcast_to(c["logits"][None], (c["B"], c["V"] + 1))


def run_reference(c):
    """The case on the reference alone: (decisions of every frame, final state)."""
    st = case_state(c)
    lg = case_logits(c)
    out = []
    for _ in range(c["frames"]):
        if c["window"] is not None:
            st.recent[:] = c["window"][None]
        ds = decide_frame(st, lg)
        for d in ds:
            commit(st, d)
        out.append(ds)
    return out, st


def draw_stats(decisions):
    """(sampled draws, ambiguous draws (margin < M), smallest cut margin) over the frames of run_reference."""
    ds = [d for fr in decisions for d in fr if d.mode == "sample"]
    amb = sum(1 for d in ds if d.margin < M)
    cut = min((d.dist.cut_margin for d in ds), default=float("inf"))
    return len(ds), amb, cut


def assert_caps(decisions, what, exact_cut=False):
    """The two conditions every sampled fixture meets, from the reference alone: at most 1 % of its draws within M of an edge
    and every entry's mass ahead further than 10 M from the cut."""
    n, amb, cut = draw_stats(decisions)
    assert amb <= AMBIGUOUS_CAP * n, (what, amb, n)
    assert exact_cut or cut > 10 * M, (what, cut)
    return n, amb, cut


# ---- scripted fixtures (Philox words, classic bookkeeping, next-input widths, slot mode): a State that `begin` starts and a
# script of ("admit", row) and ("frame", logits [B, V + 1]) steps.  Every frame's rows share one logits row (but for the EOS
# overrides) and the repetition penalty is off, so a frame has one distribution per parameter set; the logits seeds were chosen
# on the CPU, frame by frame, as the first from their starting value that keeps every distribution 10 M clear of its cut.
def begin(fx):
    st = fx["state"]
    init(st)
    if fx.get("row_step"):
        st.row_step[:] = fx["row_step"]
        st.ctr[0] = fx["row_step"]
    return st


def run_script(fx):
    """The scripted fixture on the reference alone: the decisions of every frame."""
    st = begin(fx)
    out = []
    for op, arg in fx["script"]:
        if op == "admit":
            admit(st, arg)
        else:
            ds = decide_frame(st, arg)
            for d in ds:
                commit(st, d)
            out.append(ds)
    return out


def shared_logits(seed, B, V1, scale=2.0):
    return np.repeat(randn(V1, seed=seed, scale=scale)[None], B, axis=0)


PHILOX_RUNS = ("base", "t", "row_id", "nonce", "key_low", "key_high", "seed_by_value", "seed_by_value_same_key")


def philox_fixture(what):
    """Four frames of B = 64 on set0's logits with one word of the Philox counter or key changed against 'base'."""
    B, V, D, T = 64, 2048, 72, 4
    top_p, temp, top_k, scale = PARAM_SETS[0]
    kw = dict(key=[SEED, 0], nonce=case_nonces(B))
    row_step, max_steps = 0, 8
    if what == "t":
        row_step, max_steps = 1000, 1008
    elif what == "row_id":
        kw["row_id"] = 5000 + 3 * np.arange(B)
    elif what == "nonce":
        kw["nonce"] = case_nonces(B) ^ np.uint32(0x80000000)
    elif what == "key_low":
        kw["key"] = [0x89ABCDEF, 0]
    elif what == "key_high":
        kw["key"] = [SEED, 0x01234567]
    elif what == "seed_by_value":
        kw.update(key=None, seed=0x1122334455667788)
    elif what == "seed_by_value_same_key":
        kw.update(key=None, seed=SEED)
    else:
        assert what == "base"
    st = State(B, D, T, max_steps, V, V + 1, randn(B, T, D, seed=90), randn(V + 2, D, seed=91),
               params8(top_p, temp, rep=1.0, top_k=top_k), **kw)
    lg = np.repeat(param_set_logits(scale)[None], B, axis=0)
    return dict(state=st, script=[("frame", lg)] * 4, row_step=row_step)


CLASSIC_SEEDS = (600, 601, 602, 603, 604, 605, 606)


def classic_fixture(seeds=CLASSIC_SEEDS):
    """B = 37 sampled rows, D = 200, Tar = max_steps = 6, min_gen 3, seven launches.  Frames 1, 2 and 3: the EOS logit is 60, so
    p(EOS) = 1 - 1e-20 and it is the only kept entry."""
    B, V, D, T = 37, 2048, 200, 6
    st = State(B, D, T, T, V, V + 1, randn(B, T, D, seed=96), randn(V + 2, D, seed=97),
               params8(0.9, 1.05, min_gen=3, rep=1.0), key=[SEED, 0], nonce=case_nonces(B))
    script = []
    for f in range(T + 1):
        lg = shared_logits(seeds[f], B, V + 1)
        if f in (1, 2, 3):
            lg[:, V] = 60.0
        script.append(("frame", lg))
    return dict(state=st, script=script)


WIDTH_SEEDS = (610, 611, 612)


def next_input_fixture(D, seeds=WIDTH_SEEDS):
    B, V, T = 5, 2048, 4
    st = State(B, D, T, T, V, V + 1, randn(B, T, D, seed=98), randn(V + 2, D, seed=99), params8(0.9, 1.05, rep=1.0),
               key=[SEED, 0], nonce=case_nonces(B))
    return dict(state=st, script=[("frame", shared_logits(s, B, V + 1)) for s in seeds])


SLOT_SEEDS = (620, 621, 622, 823, 624, 625, 626, 627, 628, 629, 630)   # (623 puts an entry within 10 M of a cut)
SLOT_ADMITS = {0: (1, 2), 3: (3, 5), 7: (4, 1)}


def slot_fixture(seeds=SLOT_SEEDS):
    """Six slots, eleven global frames.  Slot 0 is never admitted; slots 1 and 2 are admitted at global frame 0, 3 and 5 at frame
    3, 4 at frame 7; slot 1 has a budget of 4 frames, draws EOS in its local frame 2 and is re-admitted at frame 7 (EOS again in
    local frame 2); slot 4 draws EOS in its local frame 0 with min_gen 1.  row_id is not the row index; slot 2 decodes greedily,
    slot 3 with top_k 8, slots 1 and 4 have their own min_gen."""
    B, V, D, T = 6, 2048, 200, 12
    prm = np.stack([params8(0.9, 1.05, rep=1.0), params8(0.9, 1.05, min_gen=2, rep=1.0), params8(0.0, 1.0, rep=1.0),
                    params8(0.95, 1.0, top_k=8, rep=1.0), params8(0.9, 1.05, min_gen=1, rep=1.0), params8(0.9, 1.05, rep=1.0)])
    st = State(B, D, T, T, V, V + 1, randn(B, T, D, seed=100), randn(V + 2, D, seed=101), params8(0.5, 0.5),
               key=[SEED, 0], nonce=[11, 22, 33, 44, 55, 66], row_id=[10, 3, 7, 0, 5, 2], slot=True,
               row_max=[12, 4, 12, 12, 12, 12], row_params=prm)
    script = []
    for g in range(len(seeds)):
        script += [("admit", row) for row in SLOT_ADMITS.get(g, ())]
        lg = shared_logits(seeds[g], B, V + 1)
        if g in (2, 9):
            lg[1, V] = 60.0
        if g == 7:
            lg[4, V] = 60.0
        script.append(("frame", lg))
    return dict(state=st, script=script)


# ---- anti-loop: one row per window, the nonce chosen so that the two policies give different tokens
def anti_loop_fixture():
    """dict(windows [B, 64], recover [B] bool, names, logits [2049], params (normal top_p 1.0, recovery top_p 0.0), nonce [B],
    normal_tok [B], recovery_tok [B]).  For every n in 3 .. 16: a window whose only repeat is a tail of length n; the same with
    one token changed; the same with only 2n - 1 valid slots; a repeat of length 17 only.  Then 9 equal newest tokens, 8 equal
    followed by another and 8 equal with nothing before them (both loops: six equal tokens are a repeated tail of 3), 5 equal (no
    loop), an empty window and a window of two tokens."""
    rows, rec, names = [], [], []

    def fillers(k, base):
        return np.arange(k, dtype=np.int32) * 3 + base

    for n in range(3, 17):
        tail = fillers(n, 100 + 40 * n)
        w = np.concatenate([tail, tail, fillers(RECENT - 2 * n, 1000 + 40 * n)]).astype(np.int32)
        rows.append(w.copy()); rec.append(True); names.append(f"n{n}_repeat")
        w2 = w.copy(); w2[n + n // 2] = 1999
        rows.append(w2); rec.append(False); names.append(f"n{n}_one_changed")
        w3 = w.copy(); w3[2 * n - 1:] = -1
        rows.append(w3); rec.append(False); names.append(f"n{n}_2n-1_valid")
        t17 = fillers(17, 100 + 40 * n)
        rows.append(np.concatenate([t17, t17, fillers(RECENT - 34, 1000 + 40 * n)]).astype(np.int32))
        rec.append(False); names.append(f"n{n}_repeat17_only")
    nine = np.concatenate([np.full(9, 77), fillers(RECENT - 9, 1000)]).astype(np.int32)
    rows.append(nine); rec.append(True); names.append("streak9")
    eight = nine.copy(); eight[8] = 78     # six equal tokens are already a repeated tail of 3: the streak rule never decides alone
    rows.append(eight); rec.append(True); names.append("streak8")
    only8 = np.full(RECENT, -1, dtype=np.int32); only8[:8] = 77
    rows.append(only8); rec.append(True); names.append("streak8_nothing_before")
    five = nine.copy(); five[5:9] = (78, 79, 80, 81)
    rows.append(five); rec.append(False); names.append("streak5")
    rows.append(np.full(RECENT, -1, dtype=np.int32)); rec.append(False); names.append("empty")
    two = np.full(RECENT, -1, dtype=np.int32); two[:2] = (5, 6)
    rows.append(two); rec.append(False); names.append("two_tokens")
    windows = np.stack(rows)
    B = len(rows)
    logits = randn(2049, seed=400, scale=0.01)
    prm = params8(1.0, 1.0, True, rec_p=0.0, rec_t=1.0, rep=1.1, top_k=50)
    prm_off = prm.copy(); prm_off[2] = 0.0
    nonce, normal, recovery = np.zeros(B, dtype=np.uint32), np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    for b in range(B):
        x = penalised(logits, windows[b], 1.0, prm[5], 2049)
        recovery[b] = int(np.argmax(x))
        dist = distribution(x, 1.0, 50)
        for k in range(1, 4096):   # ~1 in 50 draws is the arg-max, ~1 in 500 is ambiguous: the first nonce nearly always serves
            tok, margin, _lo, _hi = draw(dist, float(uniform(SEED, 0, b, k)))
            if tok != recovery[b] and margin >= 100 * M:
                nonce[b], normal[b] = k, tok
                break
        else:
            raise AssertionError("no nonce separates the two policies")
    return dict(windows=windows, recover=np.asarray(rec), names=names, logits=logits, params=prm, params_off=prm_off, nonce=nonce,
                normal_tok=normal, recovery_tok=recovery)
