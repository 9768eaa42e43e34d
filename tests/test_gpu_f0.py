"""Pitch tracking on the GPU: ``hip.f0_track`` and ``hip.f0_paths`` against the numpy restatement (tests/f0_ref.py), and the engine
seam (``pitch_track`` / ``voice_pitch``).

The front end is floating point: the device's v is compared with the float64 restatement under a measured bar.  Everything after v
is integer, so candidates, path and ``nvoiced`` are compared for equality with the restatement run on the device's own v and e bits;
the output step is compared bit for bit with the restatement's fp32 form and under a measured bar with its float64 form.  The bars
are 4 x the largest deviation measured on an MI355X (profiles/f0_check.md), below 2^-12 = a quarter of a cost quantum."""
import wave

import numpy as np
import pytest
import torch

import f0_ref as R

pytestmark = pytest.mark.gpu

TOL_V = 4 * 1.452e-6      # |v - v64|: 4 x the largest deviation measured over the designed rows (profiles/f0_check.md)
TOL_E = 4 * 1.243e-7      # |e - e64| / e64 likewise
TOL_F0 = 4 * 9.264e-8     # |f0 - f0_64| / f0_64 on the same v bits likewise
TOL_ST = 4 * 2.980e-8     # |strength - strength_64| likewise
PAD = 7.5e3      # what stands after a row's length in the input: it must reach no result
CANARY = -3.25   # what stands in f0 / strength before the call: it must survive past a row's frames
K_LAST = R.K - 1


def _pp(params: dict):
    from sopro_amd import PitchParams

    return PitchParams(**params)


class Got:
    """One row's results as numpy: f0, strength [F]; nvoiced; v [F, 401], e [F], cands [F, 4]."""

    def __init__(self, f0, st, nv, v, e, cands):
        self.f0, self.st, self.nv, self.v, self.e, self.cands = f0, st, nv, v, e, cands


def _run(rows, offset=1, width_extra=3, stream=None):
    """The rows in one call: a row stride that is odd and a first sample that is not 16-byte aligned, PAD after each row's length,
    CANARY in f0 / strength -> per row a ``Got``, and whether everything past a row's frames is as it was."""
    from sopro_amd import hip

    lens = [len(r.x) for r in rows]
    width = max(max(lens), 1) + width_extra
    width += 1 - width % 2  # odd
    wav = np.full(len(rows) * width + offset, PAD, np.float32)
    for b, r in enumerate(rows):
        wav[offset + b * width: offset + b * width + lens[b]] = r.x
    dwav = torch.from_numpy(wav).cuda()[offset:].view(len(rows), width)
    frames = [R.frames(n) for n in lens]
    fcap = max(frames)
    f0 = torch.full((len(rows), fcap + 5), CANARY, dtype=torch.float32, device="cuda:0")
    st = torch.full((len(rows), fcap + 5), CANARY, dtype=torch.float32, device="cuda:0")
    call = lambda: hip.f0_track(dwav, lens, [_pp(r.params) for r in rows], debug=True, f0=f0, strength=st)  # noqa: E731
    if stream is None:
        res = call()
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            res = call()
        stream.synchronize()
    torch.cuda.synchronize()
    hz, _sg, nv, fr, dv, de, dc = res
    assert fr == frames and tuple(hz.shape) == (len(rows), fcap) and tuple(dv.shape) == (len(rows), fcap, R.NV)
    f0h, sth, nvh, dvh, deh, dch = f0.cpu().numpy(), st.cpu().numpy(), nv.cpu().numpy(), dv.cpu().numpy(), de.cpu().numpy(), dc.cpu().numpy()
    intact = True
    for b, F in enumerate(frames):
        intact = intact and bool((f0h[b, F:] == CANARY).all() and (sth[b, F:] == CANARY).all())
        intact = intact and not dvh[b, F:].any() and not deh[b, F:].any() and not dch[b, F:].any()  # (fresh debug buffers are zero)
    return [Got(f0h[b, :F].copy(), sth[b, :F].copy(), int(nvh[b]), dvh[b, :F].copy(), deh[b, :F].copy(), dch[b, :F].copy()) for b, F in enumerate(frames)], intact


@pytest.fixture(scope="module")
def batch_run():
    """The designed rows through one multi-row call (shared by the tests below)."""
    rows = R.designed_rows()
    got, intact = _run(rows)
    return rows, {r.name: g for r, g in zip(rows, got)}, intact


def _same(a: Got, b: Got) -> bool:
    return all(np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
               for x, y in ((a.f0, b.f0), (a.st, b.st), (a.v, b.v), (a.e, b.e), (a.cands, b.cands))) and a.nv == b.nv


def _chosen_lags(g: Got) -> np.ndarray:
    """The lag of every frame from f0 and the kept lags: candidates lie at least 2 apart and f0 = 24000 / (lag + off), |off| <= 0.5."""
    tau = np.zeros(len(g.f0), np.int64)
    for f in np.nonzero(g.f0 > 0)[0]:
        kept = g.cands[f][g.cands[f] > 0]
        t = 24000.0 / float(g.f0[f])
        k = int(np.argmin(np.abs(kept - t)))
        assert abs(float(kept[k]) - t) <= 0.5 + 1e-3, (f, kept, t)
        tau[f] = kept[k]
    return tau


# ---- the front end ----
def test_v_and_e_against_the_float64_restatement(batch_run):
    rows, got, intact = batch_run
    assert intact, "the call wrote past a row's frames"
    worst_v = worst_e = 0.0
    for row in rows:
        v64, e64, _ = R.reference(row)
        g = got[row.name]
        assert g.v.shape == v64.shape and g.e.shape == e64.shape
        if not len(e64):
            continue
        dv = float(np.abs(g.v.astype(np.float64) - v64).max())
        de = float((np.abs(g.e.astype(np.float64) - e64) / np.maximum(e64, 1e-300)).max()) if e64.max() > 0 else float(np.abs(g.e).max())
        print(f"{row.name:24s} n={len(row.x):6d} F={len(e64):3d} max|dv| {dv:.3e} max|de|/e {de:.3e} max v {v64.max():.3f}")
        worst_v, worst_e = max(worst_v, dv), max(worst_e, de)
    print(f"largest |dv| {worst_v:.3e} (bar {TOL_V:.3e}; a quarter of a cost quantum is {2.0 ** -12:.3e}), largest |de|/e {worst_e:.3e} (bar {TOL_E:.3e})")
    assert TOL_V <= 2.0 ** -12
    assert worst_v <= TOL_V and worst_e <= TOL_E


def test_candidates_path_and_nvoiced_are_the_restatements_on_the_devices_bits(batch_run):
    rows, got, _ = batch_run
    for row in rows:
        g = got[row.name]
        tr = R.paths(g.v, g.e, **row.params)
        assert np.array_equal(g.cands, tr.cands), row.name
        assert np.array_equal(_chosen_lags(g), tr.tau), row.name
        assert np.array_equal(g.f0 > 0, tr.state > 0) and np.array_equal(g.st > 0, (tr.state > 0) & (tr.strength > 0)), row.name
        assert g.nv == tr.nvoiced, row.name


def test_f0_and_strength_against_the_same_run(batch_run):
    rows, got, _ = batch_run
    worst_f = worst_s = 0.0
    for row in rows:
        g = got[row.name]
        t64, t32 = R.paths(g.v, g.e, **row.params), R.paths(g.v, g.e, dtype=np.float32, **row.params)
        assert np.array_equal(g.f0.view(np.int32), t32.f0.view(np.int32)) and np.array_equal(g.st.view(np.int32), t32.strength.view(np.int32)), row.name
        vo = t64.state > 0
        if vo.any():
            worst_f = max(worst_f, float(np.abs(g.f0[vo] / t64.f0[vo] - 1.0).max()))
            worst_s = max(worst_s, float(np.abs(g.st[vo] - t64.strength[vo]).max()))
        assert not g.f0[~vo].any() and not g.st[~vo].any()
    print(f"largest |f0 / f0_64 - 1| {worst_f:.3e} (bar {TOL_F0:.3e}), largest |strength - strength_64| {worst_s:.3e} (bar {TOL_ST:.3e})")
    assert worst_f <= TOL_F0 and worst_s <= TOL_ST


def test_planted_tones_through_the_operator(batch_run):
    rows, got, _ = batch_run
    for row in rows:
        if row.hz is None:
            continue
        g = got[row.name]
        rel = np.abs(g.f0 / row.hz - 1.0)
        print(f"{row.name}: voiced {g.nv} of {len(g.f0)}, largest relative error {rel.max():.3g}")
        assert len(g.f0) == 31 and g.nv == 31 and rel.max() <= 1e-3, row.name
    assert got["noise"].nv == 0 and got["zeros"].nv == 0 and got["voice_1e-3"].nv == 0 and got["voice_1e-3_floor-100"].nv == 31
    assert [len(got[f"n{n}"].f0) for n in (0, R.SPAN - 1, R.SPAN, R.SPAN + R.H)] == [0, 0, 1, 2]


# ---- the path operator on designed matrices ----
def _paths_on_device(cases):
    """[(v [F, 401], e [F], params)] as one ragged batch through hip.f0_paths -> per case (f0, strength, cands) as numpy."""
    from sopro_amd import hip

    frames = [len(c[1]) for c in cases]
    fcap = max(frames)
    v = np.zeros((len(cases), fcap, R.NV), np.float32)
    e = np.zeros((len(cases), fcap), np.float32)
    for b, (cv, ce, _p) in enumerate(cases):
        v[b, : frames[b]], e[b, : frames[b]] = cv, ce
    f0, st, dc = hip.f0_paths(torch.from_numpy(v).cuda(), torch.from_numpy(e).cuda(), frames, [_pp(c[2]) for c in cases])
    torch.cuda.synchronize()
    f0, st, dc = f0.cpu().numpy(), st.cpu().numpy(), dc.cpu().numpy()
    for b, F in enumerate(frames):
        assert not f0[b, F:].any() and not st[b, F:].any() and not dc[b, F:].any()  # nothing past a row's frames
    return [(f0[b, :F], st[b, :F], dc[b, :F]) for b, F in enumerate(frames)]


def _assert_equal_to_restatement(got, v, e, params, what):
    f0, st, dc = got
    tr = R.paths(v, e, dtype=np.float32, **params)
    assert np.array_equal(dc, tr.cands), what
    assert np.array_equal(f0.view(np.int32), tr.f0.view(np.int32)), what
    assert np.array_equal(st.view(np.int32), tr.strength.view(np.int32)), what
    return tr


def test_paths_planted_cases():
    cases = R.planted_cases()
    got = _paths_on_device([(v, e, p) for _n, v, e, p, _x in cases])
    for (name, v, e, p, expect), g in zip(cases, got):
        tr = _assert_equal_to_restatement(g, v, e, p, name)
        assert [int(t) for t in tr.tau] == expect, name
        assert [int(round(24000.0 / h)) if h > 0 else 0 for h in g[0]] == expect, name


def test_paths_ragged_random_batch_with_ties():
    """Frame counts around the path kernel's chunk of 64 frames and one long row; every third row holds small integers / 1024, so
    that equal totals are common and the tie rules decide."""
    cases = []
    for i, F in enumerate((1, 2, 63, 64, 65, 2600)):
        v, e = R.random_v(F, seed=100 + i, integers=i % 3 == 2)
        cases.append((v, e, dict(jump_cost=(96, 0, 7)[i % 3], octave_cost=(24, 0, 24)[i % 3])))
    got = _paths_on_device(cases)
    for i, ((v, e, p), g) in enumerate(zip(cases, got)):
        tr = _assert_equal_to_restatement(g, v, e, p, f"row {i}")
        assert (tr.cands[:, K_LAST] > 0).any() and 0 < tr.nvoiced, i  # the case has full candidate sets and a voiced stretch
    assert (R.paths(*cases[5][:2], **cases[5][2]).state == 0).any()



# ---- invariances ----
def test_a_row_alone_equals_the_row_in_a_batch_of_70(batch_run):
    rows, got, _ = batch_run
    by = {r.name: r for r in rows}
    pick = ["tone97.3", "glide", "voice_x20", "n1120", "noise", "n0", "voice_1e-3_floor-100"]
    big = [by[pick[i % len(pick)]] for i in range(70)]  # two launch groups: 64 + 6
    res, intact = _run(big, offset=3, width_extra=8)
    assert intact
    for row, g in zip(big, res):
        assert _same(g, got[row.name]), row.name
    for name in pick[:4]:
        (alone,), ok = _run([by[name]], offset=0, width_extra=0)
        assert ok and _same(alone, got[name]), name


def test_two_calls_and_a_side_stream_give_the_same_bits(batch_run):
    rows, got, _ = batch_run
    again, ok1 = _run(rows)
    side, ok2 = _run(rows, stream=torch.cuda.Stream())
    assert ok1 and ok2
    for row, a, s in zip(rows, again, side):
        assert _same(a, got[row.name]) and _same(s, got[row.name]), row.name


def test_no_frames_launches_nothing_that_writes():
    from sopro_amd import hip

    x = torch.full((2, R.SPAN), PAD, dtype=torch.float32, device="cuda:0")
    f0, st, nv, frames = hip.f0_track(x, [0, R.SPAN - 1])
    torch.cuda.synchronize()
    assert frames == [0, 0] and tuple(f0.shape) == (2, 0) and nv.tolist() == [0, 0]


# ---- the engine ----
@pytest.fixture(scope="module")
def tone_wav(tmp_path_factory):
    """0.5 s of the 120 Hz eight-harmonic tone at 24 kHz as a PCM16 file."""
    x = R.harmonics(12000, 120.0, seed=9)
    path = str(tmp_path_factory.mktemp("f0") / "tone120.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(1), f.setsampwidth(2), f.setframerate(R.SR)
        f.writeframes(np.round(x * 32767).astype("<i2").tobytes())
    return path


def test_pitch_track_accepts_the_three_forms(tts):
    from sopro_amd import PitchParams, PitchTrack

    x = R.harmonics(R.N_ROW, 220.0, seed=220).astype(np.float32)
    a = tts.pitch_track(torch.from_numpy(x))                             # [N] on the host
    b = tts.pitch_track(torch.from_numpy(x).cuda().reshape(1, 1, -1))    # [1, 1, N] on the device: what synthesize returns
    padded = np.full((2, R.N_ROW + 7), PAD, np.float32)
    padded[0, : R.N_ROW], padded[1, : R.SPAN] = x, x[: R.SPAN]
    c = tts.pitch_track(padded, lens=[R.N_ROW, R.SPAN])
    assert isinstance(a, PitchTrack) and isinstance(c, list) and [len(t) for t in c] == [31, 1] and len(a) == len(b) == 31
    assert a.f0.is_cuda and a.centres.tolist() == [f * 240 + 560 for f in range(31)]
    for other in (b, c[0]):
        assert torch.equal(a.f0, other.f0) and torch.equal(a.strength, other.strength)
    assert torch.equal(c[1].f0, a.f0[:1])
    assert a.voiced_fraction == 1.0 and abs(a.median_hz / 220.0 - 1.0) <= 1e-3
    assert a.span(0, 560 + 240) == (pytest.approx(float(a.f0[0])), 1.0)
    assert abs(a.semitones_to(110.0) + 12.0) < 0.02
    none = tts.pitch_track(x, params=PitchParams(unvoiced_cost=0, switch_cost=4096, threshold=0.01))
    assert none.median_hz is None and none.voiced_fraction == 0.0


def test_voice_pitch_and_the_shift_it_gives(tts, tone_wav):
    vp = tts.voice_pitch(ref_audio_path=tone_wav)
    print(f"voice_pitch: frames {len(vp)} median {vp.median_hz:.3f} Hz voiced {vp.voiced_fraction:.3f}")
    assert len(vp) > 20 and abs(vp.median_hz / 120.0 - 1.0) <= 1e-3
    # exactly the waveform the encoder would see
    x = tts.codec.reference_waveform(tone_wav, crop_seconds=12.0)
    assert torch.equal(tts.pitch_track(x).f0, vp.f0)
    short = tts.voice_pitch(ref_audio_path=tone_wav, ref_seconds=0.16)  # two codec frames: 3840 samples
    assert len(short) == R.frames(3840)
    shift = vp.semitones_to(110.0)
    assert abs(shift - 12.0 * np.log2(110.0 / 120.0)) < 0.02
    ref = tts.prepare_reference(ref_tokens_tq=torch.from_numpy(np.random.default_rng(7).integers(0, 2048, size=(24, 32))))
    tts.tokenizer.table["hello there"] = [1 + (ord(ch) % 500) for ch in "hello there"]
    wav = tts.synthesize("hello there", ref=ref, max_frames=6, seed=3, pitch=shift)
    assert wav.dim() == 3 and wav.shape[-1] > 0
    trk = tts.pitch_track(wav)
    assert len(trk) == R.frames(int(wav.shape[-1]))
