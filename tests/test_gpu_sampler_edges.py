"""The sampler and the autoregressive driver state (csrc/ar_driver.hip: ar_init_kernel, ar_sample_kernel, ar_admit_kernel) against
the host reference of tests/sampler_ref.py: every draw exact, every buffer compared as a whole after every launch.

Rig.  All integer state (hist, recent, first_eos, stop_t, row_step, *step, *n_stopped, start, row_max, nonce, row_id, key) lives in
one device arena and all float state (x_cur, params, row_params) in another; every buffer has 64 canary words in front of it and 96
behind it (NaN for floats, 0x5A5A5A5A for integers); cond, emb and the logits have buffers of their own with the same guards.
Logits rows have ld > V + 1 and their slack and guard rows hold +inf and 1e30, so a read past V + 1 wins the arg-max.  Words the
reference has not written hold a junk pattern on both sides.  After a launch the arenas are read back and compared bit for bit
with the image the reference's state gives: the words a kernel owns and everything else alike.  cond, emb and the logits are
compared at the end of a run.

Exact draws.  The uniform of a draw is Philox4x32-10 of (t, row_id, 0x5090, nonce) under the key, which the reference computes too,
so the device token must be `draw(...)`'s token.  Where the draw's `margin` - the distance, on cumulative probability, from
u * kept to the nearest edge between two kept entries - is below M, it may be the entry on the other side of that edge, and
nothing else.  M from the kernel's arithmetic, U = 2^-24, kk <= 64, |x - xmax| <= 20 for everything that carries weight:
  * e_j = expf(x_j - xmax): the argument carries one rounding, U/2 |x_j - xmax| <= 10 U absolute = 10 U relative on e_j; expf is
    good to 1 ulp = 2 U relative; together 12 U;
  * S and `ahead` are float32 sums of at most 63 additions of positive terms (ahead: 32 sequential additions per wave and the
    three joining the waves' partials; S: a six-level tree): each at most 63 U/2 < 32 U relative on top of its terms' 12 U;
  * before_j = ahead_j / S and p_j = e_j / S, a division each (U/2): before_j within (44 + 44 + 1/2) U < 89 U relative, p_j within
    (12 + 44 + 1/2) U < 57 U; the edge before_j + p_j <= 1, one more addition: within 90 U absolute;
  * kept = the sum of the kept p_j, again at most 63 additions: 57 U + 32 U = 89 U relative; u is exact and the product u * kept one
    rounding: within 90 U absolute as kept <= 1.
The comparison u * kept < before_j + p_j can therefore differ from the exact one only where the exact sides are within 180 U =
1.07e-5 of each other (the error of S is common to both sides and cancels to first order, so this is generous; the issue's own
estimate is 150 U).  The issue's M = 2e-5 (335 U) is not below that and is used as it stands.  It is not fitted to the device's
output: profiles/sampler_edges.md records what the device did inside the margin.  The same figures bound the cut: an entry's
`before` is within 89 U of the exact one, so a kept set can differ only where |before_j - top_p| < 89 U; every case keeps
10 M = 2e-4 clear of that, except the two cases that put the cut ON before = 0.5, where e = 1, S = 4 and before = 0.25 j are exact
in float32 and the outcome is decided by the comparison alone.  At most 1 % of a case's draws may be inside the margin.  Both
conditions are properties of the reference alone and are asserted in tests/test_sampler_ref.py too.

Which test fails for which break of the kernel:
  * ranking with >= instead of > (keys are unique, so a candidate then counts itself: every rank moves up by one and every
    `ahead` gains the entry's own mass): every sampled case of test_exact_draws; ties ranked towards the higher index:
    [set0] .. [set3] (the exact tie at the head), [plateau*], [all_equal], [all_nan], [two_posinf], [cut_at_half];
  * dropping the `ahead` of the lane + 64 candidates: test_exact_draws[plateau128_stride16] and [plateau128_stride4], where kept
    entries of waves 2 and 3 are candidates 64 and above with kept entries ranked behind them (asserted on the CPU in
    test_register_path_cases_keep_entries_in_the_second_slot): their upper edge falls to p_j, they are never hit and the draw
    lands on a later entry;
  * `lane <= 50` in the penalty window: test_penalty_and_window (the rows with a token in slot 50 only);
  * `before >= top_p`: test_exact_draws[cut_at_half] (entry 2, token 301, must be drawn);
  * global instead of local t in the counter: test_slot_mode (rows admitted at frames 3 and 7);
  * writing hist for a free slot: test_slot_mode (row 0's hist row stays junk, bit for bit).

What the device did per case on an MI355X: profiles/sampler_edges.md (`pytest -s` prints the table after the last test)."""
import numpy as np
import pytest
import torch

import sampler_ref as R
from conftest import golden
from sopro_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M = R.M
ICAN = 0x5A5A5A5A
FCAN = int(np.asarray([np.nan], dtype=np.float32).view(np.int32)[0])
GUARD, SLACK = 64, 32
STATS = {}   # case -> dict(draws, ambiguous, neighbour, agree_margin)
CASES = R.exact_draw_cases(golden("sampler"))


class Arena:
    """Named buffers in one allocation, each with GUARD canary words in front and GUARD + SLACK behind.  Images are int32 bit
    patterns, so NaN canaries and junk compare like everything else."""

    def __init__(self, canary):
        self.canary, self.segs, self.size, self.dev = canary, {}, 0, None

    def add(self, name, n):
        self.size += GUARD
        self.segs[name] = (self.size, int(n))
        self.size += int(n) + GUARD + SLACK

    def image(self, arrays):
        img = np.full(self.size, self.canary, dtype=np.int64).astype(np.int32)
        for name, (off, n) in self.segs.items():
            a = np.ascontiguousarray(arrays[name]).reshape(-1)
            assert a.size == n and a.dtype.itemsize == 4, name
            img[off:off + n] = a.view(np.int32)
        return img

    def upload(self, arrays):
        img = torch.from_numpy(self.image(arrays))
        if self.dev is None:
            self.dev = img.to(DEV)
        else:
            self.dev.copy_(img)

    def ptr(self, name):
        return self.dev.data_ptr() + 4 * self.segs[name][0]

    def download(self):
        return self.dev.cpu().numpy()

    def compare(self, got, arrays, what):
        want = self.image(arrays)
        if np.array_equal(got, want):
            return
        i = int(np.nonzero(got != want)[0][0])
        where = "a guard or slack word"
        for name, (off, n) in self.segs.items():
            if off <= i < off + n:
                where = f"{name}[{i - off}]"
            elif off - GUARD <= i < off:
                where = f"the guard in front of {name}"
            elif off + n <= i < off + n + GUARD + SLACK:
                where = f"the slack behind {name} (+{i - off - n})"
        raise AssertionError(f"{what}: {where}: device 0x{int(got[i]) & 0xFFFFFFFF:08x}, reference 0x{int(want[i]) & 0xFFFFFFFF:08x} "
                             f"({int(np.count_nonzero(got != want))} words differ)")


class Rig:
    """Device image of a reference State.  The reference's arrays are the truth: `upload` sends them, `check` compares them."""

    def __init__(self, ref, ld=None):
        self.ref = ref
        B, D, V = ref.B, ref.D, ref.V
        self.ld = ld if ld is not None else V + 1 + 11
        self.ints, self.floats = Arena(ICAN), Arena(FCAN)
        for name, arr in self._int_arrays().items():
            self.ints.add(name, arr.size)
        for name, arr in self._float_arrays().items():
            self.floats.add(name, arr.size)
        self.ro = Arena(FCAN)          # read by the kernels only: compared at the end of a run
        self.ro.add("cond", ref.cond.size)
        self.ro.add("emb", ref.emb.size)
        self.upload()
        self.ro.upload({"cond": ref.cond, "emb": ref.emb})
        # logits: a guard row in front, B rows of ld words, a guard row and slack behind; everything but [b, :V + 1] is +inf / 1e30
        n = (B + 2) * self.ld + SLACK
        self.lg_fill = np.where(np.arange(n) % 2 == 0, np.float32(np.inf), np.float32(1e30)).astype(np.float32)
        self.lg_img, self.lg_dev = None, torch.empty(n, dtype=torch.float32, device=DEV)
        st = hip.ArState()
        ip, fp = self.ints.ptr, self.floats.ptr
        st.x_cur, st.cond, st.emb, st.hist = fp("x_cur"), self.ro.ptr("cond"), self.ro.ptr("emb"), ip("hist")
        st.step, st.n_stopped, st.row_step = ip("step"), ip("n_stopped"), ip("row_step")
        st.first_eos, st.stop_t, st.recent, st.params = ip("first_eos"), ip("stop_t"), ip("recent"), fp("params")
        st.seed, st.B, st.D, st.Tar, st.max_steps, st.V, st.bos_row = ref.seed, B, D, ref.Tar, ref.max_steps, V, ref.bos_row
        st.start = ip("start") if ref.start is not None else None
        st.row_max = ip("row_max") if ref.row_max is not None else None
        st.row_params = fp("row_params") if ref.row_params is not None else None
        st.nonce = ip("nonce") if ref.nonce is not None else None
        st.row_id = ip("row_id") if ref.row_id is not None else None
        st.key = ip("key") if ref.key is not None else None
        self.st = st

    def _int_arrays(self):
        r = self.ref
        a = {"hist": r.hist, "recent": r.recent, "first_eos": r.first_eos, "stop_t": r.stop_t, "row_step": r.row_step,
             "step": r.ctr[0:1], "n_stopped": r.ctr[1:2]}
        for name in ("start", "row_max", "nonce", "row_id", "key"):
            if getattr(r, name) is not None:
                a[name] = getattr(r, name)
        return a

    def _float_arrays(self):
        r = self.ref
        a = {"x_cur": r.x_cur, "params": r.params}
        if r.row_params is not None:
            a["row_params"] = r.row_params
        return a

    def upload(self):
        self.ints.upload(self._int_arrays())
        self.floats.upload(self._float_arrays())

    def check(self, what, ints=None):
        torch.cuda.synchronize()
        self.ints.compare(self.ints.download() if ints is None else ints, self._int_arrays(), what)
        self.floats.compare(self.floats.download(), self._float_arrays(), what)

    def check_inputs(self, what):
        self.ro.compare(self.ro.download(), {"cond": self.ref.cond, "emb": self.ref.emb}, what)
        if self.lg_img is not None:
            assert np.array_equal(self.lg_dev.cpu().numpy().view(np.int32), self.lg_img.view(np.int32)), f"{what}: the logits changed"

    def set_logits(self, rows):
        B, V1, ld = self.ref.B, self.ref.V + 1, self.ld
        img = self.lg_fill.copy()
        img[ld:(B + 1) * ld].reshape(B, ld)[:, :V1] = rows
        self.lg_img = img
        self.lg_dev.copy_(torch.from_numpy(img))
        self.rows = np.asarray(rows, dtype=np.float32)

    def init(self):
        hip.ar_init(self.st)
        R.init(self.ref)
        self.check("sopro_ar_init")

    def admit(self, row):
        hip.ar_admit(self.st, row)
        R.admit(self.ref, row)
        self.check(f"sopro_ar_admit({row})")

    def frame(self, what, stats=None):
        """One launch of the sampler on the current logits: every emitted token is the reference's (or, inside the margin, the
        entry across the nearest edge), the reference follows the device's token, then all state is compared."""
        ref = self.ref
        ds = R.decide_frame(ref, self.rows)
        hip.ar_sample(self.st, self.lg_dev[self.ld:], self.ld)
        torch.cuda.synchronize()
        ints = self.ints.download()
        off, n = self.ints.segs["hist"]
        hist = ints[off:off + n].reshape(ref.B, ref.max_steps)
        toks = np.full(ref.B, -1, dtype=np.int64)
        for d in ds:
            if d.mode in ("done", "idle"):
                R.commit(ref, d)
                continue
            tok = toks[d.b] = int(hist[d.b, d.t])
            assert tok in d.allowed(M), (f"{what}: row {d.b} frame {d.t} ({d.mode}): device token {tok}, reference {d.tok}, u {d.u}, "
                                         f"margin {d.margin:.3e}, the edge separates {d.lo} and {d.hi}")
            if stats is not None and d.mode == "sample":
                stats["draws"] += 1
                stats["ambiguous"] += int(d.margin < M)
                stats["neighbour"] += int(tok != d.tok)
                if tok == d.tok:
                    stats["agree_margin"] = min(stats["agree_margin"], d.margin)
                stats["cut_margin"] = min(stats["cut_margin"], d.dist.cut_margin)
            R.commit(ref, d, tok)
        self.check(what, ints)
        return ds, toks


def new_stats(name):
    STATS[name] = dict(draws=0, ambiguous=0, neighbour=0, agree_margin=float("inf"), cut_margin=float("inf"))
    return STATS[name]


def meets_caps(stats, exact_cut=False):
    """The conditions of every sampled fixture, on the run the device was judged by (tests/test_sampler_ref.py asserts them from
    the reference alone): at most 1 % of the draws within M of an edge, every cut further than 10 M from an entry's mass."""
    assert stats["ambiguous"] <= R.AMBIGUOUS_CAP * stats["draws"], stats
    assert exact_cut or stats["cut_margin"] > 10 * M, stats
    assert stats["neighbour"] <= stats["ambiguous"]


@pytest.fixture(scope="module", autouse=True)
def draw_table():
    """Prints what the tests that ran recorded, after the last of them (`pytest -s`): profiles/sampler_edges.md is written from it."""
    yield
    print(f"\nSAMPLER-EDGE M = {M:.1e}; per case: draws, inside the margin (share), of those the neighbouring entry, smallest margin "
          "at which device and reference agree, smallest cut margin")
    for name, s in STATS.items():
        share = s["ambiguous"] / max(s["draws"], 1)
        print(f"SAMPLER-EDGE {name}: {s['draws']} {s['ambiguous']} ({100 * share:.2f} %) {s['neighbour']} {s['agree_margin']:.3e} "
              f"{s['cut_margin']:.3e}")


def run_scripted(fx, what, stats, each=None):
    """A scripted fixture of sampler_ref on the device: admissions and frames in order, `each(g, ds, toks, ref)` after frame g."""
    rig = Rig(fx["state"])
    rig.init()
    if fx.get("row_step"):
        rig.ref.row_step[:] = fx["row_step"]
        rig.ref.ctr[0] = fx["row_step"]
        rig.upload()
    g, out = 0, []
    for op, arg in fx["script"]:
        if op == "admit":
            rig.admit(arg)
            assert rig.ref.start[arg] == g and (rig.ref.recent[arg] == -1).all()
            assert rig.ref.first_eos[arg] == -1 and rig.ref.stop_t[arg] == -1
            continue
        rig.set_logits(arg)
        ds, toks = rig.frame(f"{what} frame {g}", stats)
        if each is not None:
            each(g, ds, toks, rig.ref)
        rig.check_inputs(f"{what} frame {g}")
        out.append(toks)
        g += 1
    return rig.ref, np.stack(out)


# ------------------------------------------------------------------------------------------------------------- exact draws
@pytest.mark.parametrize("name", list(CASES))
def test_exact_draws(name):
    c = CASES[name]
    rig = Rig(R.case_state(c, key=[R.SEED, 0], junk=0x0BADBEEF))
    rig.init()
    rig.set_logits(R.case_logits(c))
    stats = new_stats(name)
    drawn = set()
    for f in range(c["frames"]):
        if c["window"] is not None:   # the same history for every frame
            rig.ref.recent[:] = c["window"][None]
            rig.upload()
        ds, toks = rig.frame(f"{name} frame {f}", stats)
        drawn |= set(toks.tolist())
        if c["kept"] is not None:
            assert ds[0].dist.tokens.tolist() == list(c["kept"])
    rig.check_inputs(name)
    greedy = name in ("top_k_65", "top_k_0")
    assert stats["draws"] == (0 if greedy else c["B"] * c["frames"])
    meets_caps(stats, c["exact_cut"])
    if greedy:
        assert drawn == {int(np.argmax(c["logits"]))}
    if c["kept"] is not None:
        assert drawn <= set(c["kept"].tolist())
        if c["B"] == 64:
            assert drawn == set(c["kept"].tolist()), "a kept entry is never drawn"
    if name == "cut_at_half":
        assert 301 in drawn       # before == top_p exactly: kept
    if name == "cut_below_half":
        assert 301 not in drawn   # before one float32 step above top_p: dropped
    assert int(rig.ref.ctr[0]) == c["frames"]


def test_philox_counter_and_key_words():
    """Each word of the counter (t, row_id, nonce) and each half of the key moves the draws, and moves them as the reference says;
    with `key` NULL the by-value seed is the key.  Every run is a case of its own for the 1 % cap."""
    toks = {}
    for what in R.PHILOX_RUNS:
        fx = R.philox_fixture(what)
        stats = new_stats(f"philox_{what}")
        ref, toks[what] = run_scripted(fx, f"philox {what}", stats)
        assert stats["draws"] == 256 and (ref.row_step == fx["row_step"] + 4).all()
        meets_caps(stats)
    for what in R.PHILOX_RUNS[1:-1]:
        assert np.mean(toks[what] != toks["base"]) > 0.5, what   # 35 kept tokens, the likeliest below 0.2: most draws move
    assert np.array_equal(toks["seed_by_value_same_key"], toks["base"])   # seed 7 by value == key (7, 0) in device memory


# ---------------------------------------------------------------------------------------------------- penalty and the window
def _penalty_rows(V, seed):
    """16 rows of (logits [V + 1], window [64]) whose arg-max depends on every rule of the penalty window."""
    V1 = V + 1
    rng = np.random.default_rng(seed)
    lg = R.randn(16, V1, seed=seed, scale=3.0)
    win = np.full((16, 64), -1, dtype=np.int32)
    m = float(np.abs(lg).max())
    A, Bt, EOS = 777 % V, 333 % V, V
    lg[:, Bt] = m
    lg[0, A] = m + 0.2; win[0, 49] = A                 # in slot 49: penalised below Bt
    lg[1, A] = m + 0.2; win[1, 50] = A                 # in slot 50 only: not penalised
    lg[2, EOS] = m + 0.2; win[2, 3] = EOS              # EOS in the window (q = 8, bit 8)
    lg[3, EOS] = m + 0.2; win[3, 60] = EOS             # EOS outside the last 50
    lg[4, A] = m + 0.2; win[4, [0, 2, 7, 7 + 8]] = A; win[4, 4] = Bt - 1   # duplicates and holes
    lg[5, A] = m + 0.2; win[5, :4] = (V1, V1 + 499, 4095, 2 * V1)          # entries >= V1 (a kernel that marked them would
    #                                                                         touch only padding registers: this row cannot tell)
    lg[6] -= 2 * m + 1.0                               # every logit negative: a penalised one is MULTIPLIED by rep
    lg[6, A] = lg[6, Bt] + 0.05; win[6, 10] = A
    lg[7] = -np.inf; lg[7, 0] = np.nan; win[7, 1] = 0  # NaN -> -1e9, penalised -> below the -inf entries: token 1
    lg[8] = np.nan; lg[8, 0] = -np.inf; win[8, 49] = 0
    lg[9, [5, 9]] = np.inf; win[9, 20] = 5             # two +inf, the lower index penalised
    for r in range(10, 16):                            # random windows over a near-tied head of 24 tokens
        head = rng.choice(V1, size=24, replace=False)
        lg[r, head] = m + 1.0 + 0.01 * rng.permutation(24)
        pool = np.concatenate([head, rng.integers(0, V1, size=24), [-1] * 8])
        win[r] = rng.choice(pool, size=64)
        win[r, 50:] = head[:14]                        # outside the last 50: no penalty
    return lg, win


@pytest.mark.parametrize("V", [2048, 1000])
@pytest.mark.parametrize("temp,rep", [(0.7, 1.1), (0.0, 1.1), (1.0, 1.1), (0.7, 1.0), (1.3, 2.0)])
def test_penalty_and_window(V, temp, rep):
    B, D, T = 16, 72, 3
    lg, win = _penalty_rows(V, 500 + V)
    ref = R.State(B, D, T, T, V, V + 1, R.randn(B, T, D, seed=92), R.randn(V + 2, D, seed=93),
                  R.params8(0.0, temp, rep=rep, min_gen=1))
    rig = Rig(ref)
    rig.init()
    ref.recent[:] = win
    rig.upload()
    rig.set_logits(lg)
    ds, toks = rig.frame(f"penalty V {V} temp {temp} rep {rep}")
    rig.frame("penalty, second frame on the shifted window")
    rig.check_inputs("penalty")
    A, Bt = 777 % V, 333 % V
    if rep != 1.0:   # what the rows were built to show, said once more without the reference
        assert toks[:10].tolist() == [Bt, A, Bt, V, Bt, A, Bt, 1, 1, 9]
    else:
        assert toks[:7].tolist() == [A, A, V, V, A, A, A] and toks[7:10].tolist() == [0, 0, 5]


# -------------------------------------------------------------------------------------------------------------- anti-loop
@pytest.mark.parametrize("anti", [True, False])
def test_anti_loop_every_tail_length(anti):
    """One row per window; the row's nonce makes the normal policy (top_p 1) draw another token than the recovery policy
    (top_p 0: the arg-max), so the token says which policy the kernel took."""
    f = R.anti_loop_fixture()
    B, V, D, T = len(f["names"]), 2048, 72, 2
    ref = R.State(B, D, T, T, V, V + 1, R.randn(B, T, D, seed=94), R.randn(V + 2, D, seed=95),
                  f["params"] if anti else f["params_off"], key=[R.SEED, 0], nonce=f["nonce"])
    rig = Rig(ref)
    rig.init()
    ref.recent[:] = f["windows"]
    rig.upload()
    rig.set_logits(np.broadcast_to(f["logits"][None], (B, V + 1)))
    ds, toks = rig.frame(f"anti-loop {'on' if anti else 'off'}", new_stats(f"anti_loop_{'on' if anti else 'off'}"))
    rig.check_inputs("anti-loop")
    for b, name in enumerate(f["names"]):
        rec = bool(f["recover"][b]) and anti
        assert ds[b].recover == rec and ds[b].margin >= M, name
        assert toks[b] == (f["recovery_tok"][b] if rec else f["normal_tok"][b]), (name, int(toks[b]))
        assert f["recovery_tok"][b] != f["normal_tok"][b]


# ------------------------------------------------------------------------------------------------------------ bookkeeping
def test_classic_bookkeeping_eos_min_gen_last_frame_and_the_end():
    """B = 37 sampled rows, D = 200 (sampler_ref.classic_fixture).  sopro_ar_init at D = 200; frame 1: every row draws EOS one
    frame before min_gen (first_eos only); frame 2: every row draws EOS again (stop_t, n_stopped == 37); frame 3: a third EOS
    changes nothing; frame 5 is the last of Tar (no next input); the launch after max_steps leaves every buffer as it is."""
    fx = R.classic_fixture()
    B, V, T = fx["state"].B, fx["state"].V, fx["state"].Tar
    stats = new_stats("classic_bookkeeping")

    def each(f, ds, toks, ref):
        if f in (1, 2, 3):
            assert (toks == V).all()
        if f == 1:
            assert (ref.first_eos == 1).all() and (ref.stop_t == -1).all() and ref.n_stopped == 0
        if f >= 2:
            assert (ref.first_eos == 1).all() and (ref.stop_t == 2).all() and ref.n_stopped == B
        if f == T - 1:
            assert all(d.mode == "sample" and d.t + 1 == d.tmax for d in ds)
        if f == T:
            assert all(d.mode == "done" for d in ds) and ref.step == T

    run_scripted(fx, "classic", stats, each)
    assert stats["draws"] == B * T
    meets_caps(stats)


@pytest.mark.parametrize("D", [512, 64, 1])
def test_next_input_at_other_widths(D):
    stats = new_stats(f"next_input_D{D}")
    run_scripted(R.next_input_fixture(D), f"D {D}", stats)
    assert stats["draws"] == 15
    meets_caps(stats)


def test_slot_mode():
    """sampler_ref.slot_fixture: six slots, sampled rows.  Slot 0 is never admitted (*step follows it all the same, its hist row
    stays junk); slots 1 and 2 are admitted at global frame 0, 3 and 5 at frame 3, 4 at frame 7; slot 1 has a budget of 4 frames,
    draws EOS in its local frame 2 and is re-admitted at frame 7.  row_id is not the row index; slot 2 decodes greedily, slot 3
    with top_k 8, slots 1 and 4 have their own min_gen."""
    fx = R.slot_fixture()
    stats = new_stats("slot_mode")
    other = {"t": 0, "id": 0}

    def each(g, ds, toks, ref):
        for d in ds:
            active = ref.start[d.b] >= 0 and g - ref.start[d.b] < ref.row_max[d.b]
            assert (d.mode != "idle") == bool(active) and d.tg == g, (g, d.b, d.mode)
            if d.mode == "sample":   # would the global frame, or the row index, have drawn something else?
                assert d.t == g - ref.start[d.b]
                other["t"] += R.draw(d.dist, float(R.uniform(R.SEED, g, ref.row_id[d.b], ref.nonce[d.b])))[0] != d.tok
                other["id"] += R.draw(d.dist, float(R.uniform(R.SEED, d.t, d.b, ref.nonce[d.b])))[0] != d.tok
        assert ref.step == g + 1 and (ref.row_step == g + 1).all()
        if g == 2:
            assert ref.first_eos[1] == 2 and ref.stop_t[1] == 2 and ref.n_stopped == 1
        if g == 6:
            assert ds[1].mode == "idle"   # past its budget since global frame 4

    ref, _toks = run_scripted(fx, "slot mode, global", stats, each)
    meets_caps(stats)
    assert other["t"] >= 10 and other["id"] >= 10, other
    assert ref.n_stopped == 3 and ref.first_eos.tolist()[1] == 2 and ref.stop_t[4] == 0
    assert (ref.hist[0] == 0x0BADBEEF).all()


def test_argument_checks():
    B, V, D, T = 2, 100, 8, 3
    ref = R.State(B, D, T, T, V, V + 1, R.randn(B, T, D, seed=1), R.randn(V + 2, D, seed=2), R.params8(0.0, 1.0), slot=True)
    rig = Rig(ref)
    rig.set_logits(R.randn(B, V + 1, seed=3))
    lg, st = rig.lg_dev[rig.ld:], rig.st

    def refused(fn, text):
        with pytest.raises(hip.SoproHipError, match=text) as e:
            fn()
        assert "(-2)" in str(e.value)

    st.V = 2049
    refused(lambda: hip.ar_sample(st, lg, 4096), "bad sizes")
    refused(lambda: hip.ar_init(st), "bad sizes")
    st.V, st.D = V, 513
    refused(lambda: hip.ar_sample(st, lg, rig.ld), "bad sizes")
    st.D = D
    refused(lambda: hip.ar_sample(st, lg, V), "bad logits")
    refused(lambda: hip.ar_admit(st, B), "row out of range")
    refused(lambda: hip.ar_admit(st, -1), "row out of range")
    start, st.start = st.start, None
    refused(lambda: hip.ar_admit(st, 0), "slot mode")
    st.start = start
    rig.check("refused calls launch nothing")
    rig.init()
    rig.frame("after the refused calls")
