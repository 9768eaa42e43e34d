"""CPU tests of tests/sampler_ref.py: the Philox transcription against the published known-answer vectors, the float64
distribution against the oracle's float32 one and against the recorded draws of the upstream sampler, the anti-loop rule against the
oracle's, and every condition the fixtures of tests/test_gpu_sampler_edges.py must meet - these are properties of the reference
alone, so they are asserted here as well as there."""
import numpy as np
import pytest
import torch

import sampler_ref as R
from conftest import golden
from oracle import sopro_oracle as O


def _words(c):
    return " ".join(f"{int(v):08x}" for v in c)


def test_philox_known_answer_vectors():
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    assert _words(R.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    f = 0xFFFFFFFF
    assert _words(R.philox4x32_10((f, f, f, f), (f, f))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _words(R.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_philox_vector_form_equals_the_scalar_form_and_uniform_is_a_24_bit_fraction():
    t, rid, nonce = np.arange(5), np.asarray([9, 1 << 31, 3, 0xFFFFFFFF, 5]), np.asarray([0, 1, 0xF0000001, 7, 8])
    seed = 0x0123456789ABCDEF
    u = R.uniform(seed, t, rid, nonce)
    for i in range(5):
        c0 = int(R.philox4x32_10((int(t[i]), int(rid[i]), 0x5090, int(nonce[i])), (seed & 0xFFFFFFFF, seed >> 32))[0])
        assert u[i] == (c0 >> 8) / 2.0 ** 24 and 0.0 <= u[i] < 1.0
        assert float(np.float32(u[i])) == u[i]


def _oracle_p(logits, hist, top_p, temp, top_k, rep):
    sp, si, forced = O.sampling_distribution(torch.from_numpy(np.asarray(logits)).float(), hist, top_p, temp, top_k=top_k,
                                             repetition_penalty=rep)
    assert forced is None
    p = torch.zeros(len(logits), dtype=torch.float64)
    p[si] = sp.double()
    return p.numpy()


def _ref_p(logits, window, top_p, temp, top_k, rep):
    V1 = len(logits)
    d = R.distribution(R.penalised(logits, window, temp, rep, V1), float(np.float32(top_p)), top_k)
    p = np.zeros(V1)
    p[d.tokens] = np.diff(d.edges) / d.kept
    return p, d


def _dist_cases():
    g = golden("sampler")
    cases = R.exact_draw_cases(g)
    out = [(f"set{i}", cases[f"set{i}"]["logits"], [], *R.PARAM_SETS[i][:3], 1.0) for i in range(5)]
    for ci, (top_p, temp, top_k, _s) in enumerate(g["cases"].tolist()):
        out.append((f"golden{ci}", g[f"logits{ci}"], g[f"hist{ci}"].tolist(), top_p, temp, int(top_k), 1.1))
    return g, out


def test_distribution_matches_the_oracle_to_float32_roundoff_with_the_same_kept_set():
    _g, cases = _dist_cases()
    for name, logits, hist, top_p, temp, top_k, rep in cases:
        want = _oracle_p(logits, hist, top_p, temp, top_k, rep)
        got, d = _ref_p(logits, R.hist_window(hist), top_p, temp, top_k, rep)
        assert set(np.nonzero(want)[0].tolist()) == set(d.tokens.tolist()), name
        # float32 softmax over 2049 terms, two renormalisations and a cumulative sum: a few 1e-7 relative
        assert np.abs(got - want).max() <= 2e-6, (name, float(np.abs(got - want).max()))
        assert np.array_equal(R.penalised(logits, R.hist_window(hist), temp, rep, len(logits)),
                              O.penalised_logits(torch.from_numpy(np.asarray(logits)).float(), hist, temp, rep).numpy()), name


def test_expected_frequencies_match_the_recorded_draws_of_the_upstream_sampler():
    """The two-sample rule of the device test (5 sigma of the difference + 0.003) with the reference's probabilities as a sample
    of unbounded size; nothing outside the kept set was ever drawn upstream."""
    g, cases = _dist_cases()
    n_ref = int(g["n_draws"])
    for name, logits, hist, top_p, temp, top_k, rep in cases[5:]:
        p, _d = _ref_p(logits, R.hist_window(hist), top_p, temp, top_k, rep)
        counts = g[f"counts{name[-1]}"].astype(np.float64)
        assert counts[p == 0].sum() == 0, name
        tol = 5.0 * np.sqrt(p * (1 - p) / n_ref) + 0.003
        assert ((np.abs(counts / n_ref - p) - tol).max()) <= 0.0, name


def test_policy_matches_the_oracle_rule_on_random_histories():
    rng = np.random.default_rng(5)
    seen = {True: 0, False: 0}
    for i in range(3000):
        L = int(rng.integers(0, 65))
        hist = rng.integers(0, int(rng.integers(1, 5)), size=L).tolist() if i % 3 else rng.integers(0, 2048, size=L).tolist()
        if i % 3 == 2 and L >= 8:   # plant a repeated tail of a random length (also 17 and more: no rule) in a random history
            n = int(rng.integers(1, 24))
            if 2 * n <= L:
                hist = rng.integers(0, 2048, size=L).tolist()
                hist[L - n:] = hist[L - 2 * n: L - n]
        streak9 = L >= 9 and len(set(hist[-9:])) == 1
        want = O.repeated_tail(hist, 16) or streak9
        w = R.hist_window(hist)
        assert R.repeated_window(w) == want, hist
        prm = R.params8(0.9, 1.05, True)
        rec, top_p, temp, kk, sampling = R.policy(w, prm, 2049)
        assert rec == want and sampling and kk == 50
        assert (top_p, temp) == ((float(prm[3]), float(prm[4])) if want else (float(prm[0]), float(prm[1])))
        prm[2] = 0.0
        assert R.policy(w, prm, 2049)[0] is False
        seen[want] += 1
    assert min(seen.values()) > 300, seen
    for top_p, top_k, V1, want in ((0.0, 50, 2049, False), (-1.0, 50, 2049, False), (0.9, 65, 2049, False), (0.9, 0, 2049, False),
                                   (0.9, 64, 2049, True), (0.9, 0, 21, True), (0.9, 65, 21, True)):
        assert R.policy(R.hist_window([]), R.params8(top_p, 1.0, top_k=top_k), V1)[4] is want


def test_draw_edges_margins_and_neighbours():
    d = R.distribution(np.log(np.asarray([0.5, 0.25, 0.125, 0.125])), 1.0, 4)
    assert d.tokens.tolist() == [0, 1, 2, 3] and np.allclose(d.edges, [0, .5, .75, .875, 1.0], atol=1e-15)
    assert R.draw(d, 0.49)[0] == 0 and R.draw(d, 0.5)[0] == 1 and R.draw(d, 0.999)[0] == 3
    tok, m, lo, hi = R.draw(d, 0.74)
    assert (tok, lo, hi) == (1, 1, 2) and abs(m - 0.01) < 1e-12
    tok, m, lo, hi = R.draw(d, 0.51)
    assert (tok, lo, hi) == (1, 0, 1) and abs(m - 0.01) < 1e-12
    d = R.distribution(np.log(np.asarray([0.5, 0.25, 0.125, 0.125])), 0.6, 4)   # before = 0, .5, .75, .875: entries 0, 1 stay
    assert d.tokens.tolist() == [0, 1] and abs(d.kept - 0.75) < 1e-15 and abs(d.cut_margin - 0.1) < 1e-12
    assert R.draw(d, 0.999)[0] == 1 and R.draw(d, 0.6)[0] == 0 and R.draw(d, 0.7)[0] == 1
    d = R.distribution(np.asarray([1.0, 3.0, 3.0, 0.0]), 1e-6, 3)
    assert d.tokens.tolist() == [1] and R.draw(d, 0.99) == (1, float("inf"), 1, 1)


def test_penalised_window_rules():
    x = np.asarray([2.0, -2.0, 4.0, np.nan, np.inf, -np.inf, 1.0, 3.0], dtype=np.float32)
    w = np.full(64, -1, dtype=np.int32)
    w[49], w[50], w[3], w[4], w[5], w[6] = 0, 2, 1, 1, 7, 99     # slot 50 does not count, token 1 twice, 99 >= V1
    got = R.penalised(x, w, 0.5, 2.0, 8)
    assert got.tolist() == [2.0, -8.0, 8.0, -2e9, 2e9, -2e9, 2.0, 3.0]
    assert R.penalised(x, w, 0.0, 1.0, 8).tolist()[:3] == [2.0, -2.0, 4.0]


# ------------------------------------------------------------------------------------------------ the fixtures' own conditions
def candidates(x32, kk, threads=256):
    """The candidate tokens the kernel's top-k bound keeps, in the order the kernel numbers them.  A restatement of the bound
    for choosing and checking fixtures that take a given ranking path - kept here, out of the reference, because it describes the
    kernel's method and not the sampler's result; nothing judges device output with it.  Thread i % 256 owns logit i; every wave
    of 64 threads takes the ceil(kk / 4)-th largest of its threads' maxima (threads without a logit count as the lowest value);
    the bound is the smallest of the four; every logit >= the bound is a candidate, numbered wave by wave, inside a wave by q row
    (token // 256), then lane.  At most 128 candidates are ranked in registers (64 .. 127 in the lanes' second slot), more
    through LDS."""
    x = np.asarray(x32, dtype=np.float32)
    pad = np.full((-len(x)) % threads, -np.inf, dtype=np.float32)
    tmax = np.concatenate([x, pad]).reshape(-1, threads).max(axis=0)
    n = (kk + 3) // 4
    thr = min(np.sort(tmax[w * 64:(w + 1) * 64])[::-1][n - 1] for w in range(threads // 64))
    tok = np.nonzero(x >= thr)[0]
    return tok[np.lexsort((tok % 64, tok // threads, (tok % threads) // 64))]


def candidate_count(x32, kk):
    return len(candidates(x32, kk))


@pytest.fixture(scope="module")
def cases():
    return R.exact_draw_cases(golden("sampler"))


def test_every_exact_draw_case_meets_its_caps(cases):
    """Per case: at most 1 % of the draws within M of an edge, the top-p cut further than 10 M from every entry's mass (except
    where the cut is placed ON an edge that float32 represents exactly), the expected kept set, the ranking path."""
    for name, c in cases.items():
        ds, st = R.run_reference(c)
        n, amb, cut = R.draw_stats(ds)
        greedy = name in ("top_k_65", "top_k_0")
        assert n == (0 if greedy else c["B"] * c["frames"]), name
        assert amb <= R.AMBIGUOUS_CAP * max(n, 1), (name, amb, n)
        if not c["exact_cut"]:
            assert cut > 10 * R.M, (name, cut)
        toks = {d.tok for fr in ds for d in fr}
        if c["kept"] is not None:
            d0 = ds[0][0].dist
            assert d0.tokens.tolist() == list(c["kept"]), name
            assert toks <= set(c["kept"].tolist()), name
            if c["B"] == 64:   # 2 048 draws reach every kept entry of these cases (256 draws of 1 / 50 each need not)
                assert toks == set(c["kept"].tolist()), (name, "a kept entry is never drawn")
            if name.startswith("plateau") or name.startswith("all_"):
                assert np.abs(np.diff(d0.edges) / d0.kept - 1.0 / len(c["kept"])).max() < 1e-12, name
        if greedy:
            assert toks == {int(np.argmax(c["logits"]))}
        if c["path"] is not None and not c["chained"]:
            win = c["window"] if c["window"] is not None else np.full(64, -1)
            C = candidate_count(R.penalised(c["logits"], win, c["temp"], c["rep"], c["V"] + 1), min(c["top_k"], c["V"] + 1))
            assert (C <= 128) == (c["path"] == "fast"), (name, C)
            if name.startswith("plateau") and not name.endswith("first"):
                assert C == int(name[7:].split("_")[0]), (name, C)
        if name == "cut_at_half":
            assert 301 in toks
        if name == "cut_below_half":
            assert 301 not in toks
        assert (st.hist[:, :c["frames"]] >= 0).all() and int(st.ctr[0]) == c["frames"]


def test_the_one_wave_case_has_a_large_superset(cases):
    c = cases["top50_in_one_wave"]
    assert candidate_count(R.penalised(c["logits"], np.full(64, -1), c["temp"], 1.0, 2049), 50) > 100


def test_register_path_cases_keep_entries_in_the_second_slot(cases):
    """A kernel that loses the mass ahead of the candidates 64 .. 127 is caught only where such a candidate is a kept entry with
    kept entries ranked behind it: these cases have them."""
    second = {}
    for name, c in cases.items():
        if c["path"] != "fast" or c["window"] is not None:
            continue
        x = R.penalised(c["logits"], np.full(64, -1), c["temp"], c["rep"], c["V"] + 1)
        cand = candidates(x, min(c["top_k"], c["V"] + 1)).tolist()
        kept = R.distribution(x, float(np.float32(c["top_p"])), c["top_k"]).tokens.tolist()
        second[name] = sum(1 for r, tok in enumerate(kept) if 0 < r < len(kept) - 1 and cand.index(tok) >= 64)
    for name in ("plateau128_stride16", "plateau128_stride4"):
        assert second[name] >= 4, second
    assert second["plateau64_stride16"] == 0 and second["plateau64_stride4"] == 0


def test_anti_loop_fixture_separates_the_two_policies():
    f = R.anti_loop_fixture()
    assert len(f["names"]) == 14 * 4 + 6 <= 64
    assert (f["normal_tok"] != f["recovery_tok"]).all()
    for b, name in enumerate(f["names"]):
        assert R.repeated_window(f["windows"][b]) == bool(f["recover"][b]), name
        hist = [int(v) for v in f["windows"][b][::-1] if v >= 0]
        assert (O.repeated_tail(hist, 16) or (len(hist) >= 9 and len(set(hist[-9:])) == 1)) == bool(f["recover"][b]), name
        for prm, want in ((f["params"], f["recovery_tok"][b] if f["recover"][b] else f["normal_tok"][b]),
                          (f["params_off"], f["normal_tok"][b])):
            st = R.State(1, 8, 2, 2, 2048, 2049, np.zeros((1, 2, 8)), np.zeros((2050, 8)), prm, seed=R.SEED, nonce=[f["nonce"][b]],
                         row_id=[b])
            R.init(st)
            st.recent[0] = f["windows"][b]
            d = R.decide(st, 0, f["logits"])
            assert d.tok == want and d.recover == (bool(f["recover"][b]) and prm[2] != 0), name
            assert d.mode == ("greedy" if d.recover else "sample") and d.margin >= R.M


def test_scripted_fixtures_meet_the_caps():
    """The Philox-word runs (each a case of its own), the classic bookkeeping run, the next-input widths and the slot-mode run:
    at most 1 % of the draws within M of an edge, every cut 10 M clear, and the events each script is built around."""
    toks = {}
    for what in R.PHILOX_RUNS:
        fx = R.philox_fixture(what)
        ds = R.run_script(fx)
        assert R.assert_caps(ds, what)[0] == 256 and all(d.t == fx["row_step"] + f for f, fr in enumerate(ds) for d in fr)
        toks[what] = np.asarray([[d.tok for d in fr] for fr in ds])
    for what in R.PHILOX_RUNS[1:-1]:
        assert np.mean(toks[what] != toks["base"]) > 0.5, what
    assert np.array_equal(toks["seed_by_value_same_key"], toks["base"])

    fx = R.classic_fixture()
    ds, st = R.run_script(fx), fx["state"]
    assert R.assert_caps(ds, "classic")[0] == 37 * 6
    assert all(d.tok == st.V for f in (1, 2, 3) for d in ds[f]) and all(d.mode == "done" for d in ds[6])
    assert (st.first_eos == 1).all() and (st.stop_t == 2).all() and st.n_stopped == 37 and st.step == 6

    for D in (512, 64, 1):
        assert R.assert_caps(R.run_script(R.next_input_fixture(D)), f"D {D}")[0] == 15

    fx = R.slot_fixture()
    ds, st = R.run_script(fx), fx["state"]
    R.assert_caps(ds, "slot mode")
    other_t = other_id = 0
    for g, fr in enumerate(ds):
        for d in fr:
            if d.mode == "sample":   # the global frame, or the row index, in the counter would draw another token
                other_t += R.draw(d.dist, float(R.uniform(R.SEED, g, st.row_id[d.b], st.nonce[d.b])))[0] != d.tok
                other_id += R.draw(d.dist, float(R.uniform(R.SEED, d.t, d.b, st.nonce[d.b])))[0] != d.tok
    assert other_t >= 10 and other_id >= 10, (other_t, other_id)
    assert [d.mode for d in ds[6]] == ["idle", "idle", "greedy", "sample", "idle", "sample"]
    assert st.start.tolist() == [-1, 7, 0, 3, 7, 3] and st.n_stopped == 3 and st.stop_t[4] == 0 and st.first_eos[1] == 2
    assert (st.hist[0] == 0x0BADBEEF).all() and st.step == 11


def test_step_bookkeeping_classic_and_slot_mode():
    """The driver rules on a toy vocabulary (V = 4, EOS = 4), greedy so that the logits name the token."""
    V, D, T = 4, 3, 5
    cond, emb = R.randn(2, T, D, seed=1), R.randn(V + 2, D, seed=2)

    def lg(*toks):
        x = np.zeros((len(toks), V + 1), dtype=np.float32)
        x[np.arange(len(toks)), toks] = 9.0
        return x

    st = R.State(2, D, T, T, V, V + 1, cond, emb, R.params8(0.0, 1.0, min_gen=3, rep=1.0))
    R.init(st)
    assert np.array_equal(st.x_cur, cond[:, 0] + emb[V + 1]) and st.step == 0 and (st.recent == -1).all()
    for t, toks in enumerate([(1, 4), (4, 2), (4, 4), (4, 0), (3, 3)]):
        for b in range(2):
            d = R.step(st, b, lg(*toks)[b])
            assert d.tok == toks[b] and d.t == t
        if t + 1 < T:
            assert np.array_equal(st.x_cur, cond[:, t + 1] + emb[list(toks)])
    assert st.first_eos.tolist() == [1, 0] and st.stop_t.tolist() == [2, 2] and st.n_stopped == 2 and st.step == 5
    assert st.recent[0, :6].tolist() == [3, 4, 4, 4, 1, -1] and st.hist[1].tolist() == [4, 2, 4, 0, 3]
    x_last = st.x_cur.copy()
    assert R.step(st, 0, lg(0, 0)[0]).mode == "done" and st.step == 5 and np.array_equal(st.x_cur, x_last)
    # slot mode: row 0 free, row 1 admitted at global frame 2 with a budget of 2 frames
    st = R.State(2, D, T, T, V, V + 1, cond, emb, R.params8(0.0, 1.0, rep=1.0), slot=True, row_max=[T, 2])
    R.init(st)
    assert st.start.tolist() == [-1, -1]
    for _ in range(2):
        assert [R.step(st, b, lg(1, 1)[b]).mode for b in range(2)] == ["idle", "idle"]
    assert st.step == 2 and st.row_step.tolist() == [2, 2]
    R.admit(st, 1)
    assert st.start.tolist() == [-1, 2]
    hist0 = st.hist.copy()
    modes = [[R.step(st, b, lg(2, 3)[b]).mode for b in range(2)] for _ in range(3)]
    assert modes == [["idle", "greedy"], ["idle", "greedy"], ["idle", "idle"]]
    assert st.hist[1, :2].tolist() == [3, 3] and np.array_equal(st.hist[0], hist0[0]) and st.step == 5
    assert np.array_equal(st.x_cur[1], cond[1, 1] + emb[3])   # local frame 1 is the last of the budget: no next input
