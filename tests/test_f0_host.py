"""Pitch tracking without a GPU: the numpy restatement against planted material (tones, a missing fundamental, noise, silence, the
level gate), the integer path on planted matrices and its tie rules, the frame count at the edges, ``PitchTrack`` on hand-made arrays,
the ``PitchParams`` ranges, and the size function and the refusals of the C entry points, which come before any launch."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import f0_ref as R


# ---- the restatement on planted material ----
@pytest.mark.parametrize("row", [r for r in R.designed_rows() if r.hz is not None], ids=lambda r: r.name)
def test_planted_frequency_is_recovered_in_every_frame(row):
    """Eight-harmonic tones and harmonics 2-4 of 120 Hz without the fundamental: 1e-3 relative leaves the definition room (the
    parabola's own error is below 2e-4 on these) and still catches an octave error or a neighbouring lag."""
    tr = R.reference(row)[2]
    rel = np.abs(tr.f0 / row.hz - 1.0)
    print(f"{row.name}: frames {len(tr.f0)} voiced {tr.nvoiced} largest relative error {rel.max():.3g}")
    assert len(tr.f0) == 31 and tr.nvoiced == 31 and rel.max() <= 1e-3


def test_noise_and_silence_are_unvoiced():
    by = {r.name: r for r in R.designed_rows()}
    for name in ("noise", "zeros"):
        tr = R.reference(by[name])[2]
        assert len(tr.f0) == 31 and tr.nvoiced == 0 and not tr.f0.any() and not tr.strength.any()
    v = R.reference(by["zeros"])[0]
    assert np.array_equal(v, np.ones_like(v))  # c = 0 everywhere: v is 1 by definition


def test_level_gate():
    by = {r.name: r for r in R.designed_rows()}
    quiet, open_ = R.reference(by["voice_1e-3"])[2], R.reference(by["voice_1e-3_floor-100"])[2]
    assert quiet.nvoiced == 0 and not quiet.cands.any()
    assert open_.nvoiced == 31
    assert float(R.gate_of(-50.0)) == float(np.float32(720e-5)) and float(R.gate_of(0.0)) == 720.0


def test_glide_and_vibrato_are_voiced_throughout():
    by = {r.name: r for r in R.designed_rows()}
    tr = R.reference(by["glide"])[2]
    assert tr.nvoiced == 31 and np.all(np.diff(tr.f0) > 0)
    assert R.track(R.voice(R.SPAN + 100 * R.H).astype(np.float32)).nvoiced == 101


# ---- the path on planted matrices ----
@pytest.mark.parametrize("case", R.planted_cases(), ids=lambda c: c[0])
def test_planted_path_cases(case):
    _name, v, e, params, expect = case
    tr = R.paths(v, e, **params)
    assert [int(t) for t in tr.tau] == expect
    assert tr.nvoiced == sum(1 for t in expect if t)


def _ints_v(n_frames, dips):
    """v of multiples of 1 / 1024: 1.0 but for (frame, lag, cost) dips."""
    v = np.ones((n_frames, R.NV), np.float32)
    for f, t, c in dips:
        v[f, t] = c / 1024.0
    return v


def test_tie_rules():
    e3 = np.ones(3, np.float32)
    free = dict(octave_cost=0, jump_cost=0)
    # two candidates of one cost in every frame: the smaller state (the shorter lag) at the last frame and at every predecessor
    v = _ints_v(3, [(f, t, 40) for f in range(3) for t in (100, 200)])
    assert [int(t) for t in R.paths(v, e3, **free).tau] == [100, 100, 100]
    # a voiced candidate that costs what the unvoiced state costs: the unvoiced state is state 0 and wins
    v = _ints_v(3, [(f, 100, 150) for f in range(3)])
    assert [int(t) for t in R.paths(v, e3, switch_cost=0, **free).tau] == [0, 0, 0]
    assert [int(t) for t in R.paths(v, e3, switch_cost=0, unvoiced_cost=151, **free).tau] == [100, 100, 100]
    # the last frame prefers lag 200 by one unit; its two predecessors cost the same: the smaller predecessor
    v = _ints_v(3, [(0, 100, 40), (0, 200, 40), (1, 100, 40), (1, 200, 40), (2, 100, 41), (2, 200, 40)])
    assert [int(t) for t in R.paths(v, e3, **free).tau] == [100, 100, 200]
    # five equal dips: the K kept are the four shortest lags (the key is (q, lag)), numbered by ascending lag
    v = _ints_v(1, [(0, t, 40) for t in (60, 90, 120, 150, 180)])
    tr = R.paths(v, np.ones(1, np.float32), octave_cost=0)
    assert [int(t) for t in tr.cands[0]] == [60, 90, 120, 150] and int(tr.tau[0]) == 60
    # a cheaper dip at a longer lag displaces the longest of the equal ones, and the order stays by lag
    v[0, 300] = 39 / 1024.0
    tr = R.paths(v, np.ones(1, np.float32), octave_cost=0)
    assert [int(t) for t in tr.cands[0]] == [60, 90, 120, 300] and int(tr.tau[0]) == 300
    # a plateau: v[t] < v[t - 1] and v[t] <= v[t + 1] makes its first lag the candidate, and only that
    v = _ints_v(1, [(0, 100, 40), (0, 101, 40)])
    assert [int(t) for t in R.paths(v, np.ones(1, np.float32)).cands[0]] == [100, 0, 0, 0]
    # the threshold is strict, and the ends of the lag range are no candidates
    v = _ints_v(1, [(0, 100, 512), (0, R.TMIN - 1, 10), (0, R.TMAX, 10)])
    assert not R.paths(v, np.ones(1, np.float32)).cands.any()
    v = _ints_v(1, [(0, R.TMIN, 10), (0, R.TMAX - 1, 10)])
    assert [int(t) for t in R.paths(v, np.ones(1, np.float32)).cands[0]] == [R.TMIN, R.TMAX - 1, 0, 0]


def test_lag_table_is_far_from_its_rounding_boundaries():
    t = np.arange(1, R.NV, dtype=np.float64)
    y = 256.0 * np.log2(t)
    assert np.abs(y - np.floor(y) - 0.5).min() > 8e-4 and R.L[1] == 0 and R.L[R.TMAX] == 2213 and len(R.L) == 401


def test_frame_count_at_the_edges():
    from sopro_amd import f0 as F0

    want = {0: 0, R.SPAN - 1: 0, R.SPAN: 1, R.SPAN + R.H - 1: 1, R.SPAN + R.H: 2}
    for n, F in want.items():
        assert R.frames(n) == F == F0.frames_of(n)
        v, e = R.front(np.zeros(n, np.float32))
        assert v.shape == (F, R.NV) and e.shape == (F,)
    assert (F0.H, F0.W, F0.TMIN, F0.TMAX, F0.SPAN, F0.K, F0.CENTRE) == (R.H, R.W, R.TMIN, R.TMAX, R.SPAN, R.K, R.CENTRE) == (240, 720, 48, 400, 1120, 4, 560)


# ---- PitchTrack ----
def test_pitch_track_on_hand_made_arrays():
    import sopro_amd
    from sopro_amd.f0 import PitchTrack

    assert sopro_amd.PitchTrack is PitchTrack and {"PitchTrack", "PitchParams"} <= set(sopro_amd.__all__)
    hz = torch.tensor([0.0, 100.0, 110.0, 0.0, 130.0, 200.0], dtype=torch.float32)
    trk = PitchTrack(hz, torch.where(hz > 0, 0.9, 0.0))
    assert len(trk) == 6 and trk.centres.tolist() == [560 + 240 * f for f in range(6)]
    assert trk.median_hz == 120.0 and trk.voiced_fraction == pytest.approx(4 / 6)
    assert trk.span(0, 560) == (None, 0.0)                      # no centre in [0, 560)
    assert trk.span(0, 561) == (None, 0.0)                      # frame 0 alone, unvoiced
    assert trk.span(560, 1041) == (105.0, pytest.approx(2 / 3))  # frames 0, 1, 2
    assert trk.span(801, 1040) == (None, 0.0)                   # between two centres: an empty span
    assert trk.span(800, 801) == (100.0, 1.0)
    assert trk.span(1520, 10 ** 9) == (165.0, 1.0) and trk.span(-5000, 10 ** 9) == (120.0, pytest.approx(4 / 6))
    assert trk.span(5000, 100) == (None, 0.0)
    assert trk.semitones_to(240.0) == pytest.approx(12.0) and trk.semitones_to(120.0) == 0.0
    with pytest.raises(ValueError):
        trk.semitones_to(0.0)
    silent = PitchTrack(torch.zeros(3), torch.zeros(3))
    assert silent.median_hz is None and silent.voiced_fraction == 0.0
    with pytest.raises(ValueError, match="no voiced frame"):
        silent.semitones_to(110.0)
    empty = PitchTrack(torch.zeros(0), torch.zeros(0))
    assert empty.median_hz is None and empty.voiced_fraction == 0.0 and empty.span(0, 1000) == (None, 0.0)
    with pytest.raises(ValueError):
        PitchTrack(torch.zeros(3), torch.zeros(4))


# ---- parameters ----
def test_pitch_params_defaults_and_ranges():
    import sopro_amd
    from sopro_amd.f0 import PitchParams, check_params, per_row

    assert sopro_amd.PitchParams is PitchParams
    p = PitchParams()
    assert (p.threshold, p.floor_db, p.octave_cost, p.jump_cost, p.switch_cost, p.unvoiced_cost) == (0.5, -50.0, 24, 96, 160, 150)
    assert dict(zip(("threshold", "floor_db", "octave_cost", "jump_cost", "switch_cost", "unvoiced_cost"), p.as_floats())) == R.DEFAULTS
    assert PitchParams(1.0, 0.0, 1024, 4096, 4096, 1024).jump_cost == 4096 and PitchParams(1e-3, -100, 0, 0, 0, 0).unvoiced_cost == 0
    assert isinstance(PitchParams(jump_cost=3.0).jump_cost, int)
    with pytest.raises(Exception):
        p.threshold = 0.3  # frozen
    for kw in (dict(threshold=0.0), dict(threshold=1.01), dict(threshold=-0.5), dict(floor_db=-100.5), dict(floor_db=0.1), dict(octave_cost=-1),
               dict(octave_cost=1025), dict(unvoiced_cost=1025), dict(unvoiced_cost=-1), dict(jump_cost=4097), dict(jump_cost=-1), dict(switch_cost=4097),
               dict(switch_cost=2.5), dict(octave_cost=0.5), dict(threshold=math.nan), dict(floor_db=math.inf), dict(jump_cost=math.nan),
               dict(threshold="low"), dict(switch_cost=None), dict(octave_cost=True)):
        with pytest.raises(ValueError):
            PitchParams(**kw)
    assert check_params(None) == PitchParams() and check_params(p) is p
    with pytest.raises(TypeError):
        check_params(0.5)
    q = PitchParams(threshold=0.3)
    assert per_row(None, 2) == [p, p] and per_row(q, 3) == [q, q, q] and per_row([q, None], 2) == [q, p]
    with pytest.raises(ValueError):
        per_row([q], 2)
    with pytest.raises(TypeError):
        per_row("pp", 2)


def test_constants_match_the_header():
    import os
    import re

    from conftest import ROOT
    from sopro_amd import f0 as F0
    from sopro_amd import hip

    src = open(os.path.join(ROOT, "include", "sopro_hip.h")).read()
    val = {k: int(v) for k, v in re.findall(r"#define SOPRO_F0_([A-Z_]+) ([0-9]+)", src)}
    assert (val["H"], val["W"], val["TMIN"], val["TMAX"], val["SPAN"], val["K"], val["PARAMS"]) == (R.H, R.W, R.TMIN, R.TMAX, R.SPAN, R.K, 6)
    assert (val["H"], val["W"], val["TMIN"], val["TMAX"], val["SPAN"], val["K"], val["PARAMS"]) == (hip.F0_H, hip.F0_W, hip.F0_TMIN, hip.F0_TMAX, hip.F0_SPAN, hip.F0_K, hip.F0_PARAMS)
    assert (val["COST_MAX"], val["JUMP_MAX"]) == (F0.COST_MAX, F0.JUMP_MAX) == (1024, 4096)
    assert {"sopro_f0_workspace_bytes", "sopro_f0_rows_f32", "sopro_f0_paths"} <= set(hip.SYMBOLS) and isinstance(hip.f0_calls, int)


def test_entry_points_exist_and_no_existing_one_grew_a_keyword():
    import inspect

    from sopro_amd import SoproTTS

    assert list(inspect.signature(SoproTTS.pitch_track).parameters) == ["self", "wav", "lens", "params"]
    assert list(inspect.signature(SoproTTS.voice_pitch).parameters) == ["self", "ref_audio_path", "denoise", "crop", "ref_seconds", "params"]
    for name in ("synthesize", "synthesize_timed", "synthesize_batch", "stream", "prepare_reference"):
        assert "params" not in inspect.signature(getattr(SoproTTS, name)).parameters


def test_waveform_forms_are_told_apart_on_the_argument_path():
    from sopro_amd.f0 import as_rows

    x = np.arange(10, dtype=np.float32)
    for form in (x, x.reshape(1, 10), x.reshape(1, 1, 10), torch.from_numpy(x).double()):
        rows, lens, batched = as_rows(form, None, "cpu")
        assert tuple(rows.shape) == (1, 10) and rows.dtype == torch.float32 and lens == [10] and not batched
    rows, lens, batched = as_rows(np.zeros((3, 10), np.float32), [10, 0, 4], "cpu")
    assert tuple(rows.shape) == (3, 10) and lens == [10, 0, 4] and batched
    for bad, ln in ((np.zeros((3, 10), np.float32), None), (np.zeros((3, 10), np.float32), [10, 10]), (np.zeros((3, 10), np.float32), [10, 11, 0]),
                    (np.zeros(10, np.float32), [10])):
        with pytest.raises(ValueError):
            as_rows(bad, ln, "cpu")
    with pytest.raises(TypeError):
        as_rows(np.zeros(10, np.int16), None, "cpu")


# ---- the library on the CPU ----
def test_workspace_size_is_monotone():
    from sopro_amd import hip

    lib = hip.load()
    assert lib.sopro_f0_workspace_bytes(0, 100) == -1 and lib.sopro_f0_workspace_bytes(1, -1) == -1 and lib.sopro_f0_workspace_bytes(1, (1 << 24) + 1) == -1
    assert lib.sopro_f0_workspace_bytes(1, 0) == lib.sopro_f0_workspace_bytes(1, R.SPAN - 1) == 4
    assert lib.sopro_f0_workspace_bytes(1, R.SPAN) == (17 + 1) * 4 and lib.sopro_f0_workspace_bytes(3, R.SPAN + R.H) == (3 * 2 * 17 + 1) * 4
    caps = [0, 1, R.SPAN - 1, R.SPAN, R.SPAN + 1, R.SPAN + R.H - 1, R.SPAN + R.H, 48000, 384000, 1 << 24]
    for rows in (1, 2, 70, 65535):
        sizes = [lib.sopro_f0_workspace_bytes(rows, c) for c in caps]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
        assert lib.sopro_f0_workspace_bytes(rows, 384000) <= lib.sopro_f0_workspace_bytes(rows + 1, 384000)
    # v for the whole batch is never held: a frame costs 17 words, not 401
    assert lib.sopro_f0_workspace_bytes(32, 384000) < 32 * R.frames(384000) * 18 * 4


def test_c_entries_refuse_bad_arguments_without_a_device():
    """Every check of sopro_f0_rows_f32 and sopro_f0_paths comes before the first launch, so the refusals can be seen without a GPU."""
    from sopro_amd import hip

    lib = hip.load()
    n = 5000
    good = (0.5, -50.0, 24.0, 96.0, 160.0, 150.0)
    lens, par = (C.c_int32 * 1)(n), (C.c_float * 6)(*good)
    fake = 1 << 12  # (never dereferenced: the call is refused first)
    need = lib.sopro_f0_workspace_bytes(1, n)

    def call(lens_=lens, par_=par, ws=fake, wsb=need, rows=1, nvoiced=fake, wav=fake, f0=fake):
        return lib.sopro_f0_rows_f32(wav, n, lens_, par_, rows, f0, fake, 100, nvoiced, None, None, None, ws, wsb, None)

    assert call(wsb=need - 1) == -2 and b"ws_bytes" in lib.sopro_last_error()
    assert call(ws=None) == -2 and call(lens_=None) == -2 and call(par_=None) == -2 and call(nvoiced=None) == -2
    assert call(wav=None) == -2 and call(f0=None) == -2 and call(ws=fake + 2) == -2 and call(wav=fake + 2) == -2
    assert call(rows=0) == -2 and call(rows=65536) == -2
    assert call(lens_=(C.c_int32 * 1)(-1)) == -2 and call(lens_=(C.c_int32 * 1)((1 << 24) + 1)) == -2
    bad_values = ((0, (0.0, 1.5, -0.1, math.nan), b"threshold"), (1, (-100.5, 0.5, math.nan), b"floor_db"), (2, (-1.0, 1025.0, 0.5, math.nan), b"octave_cost"),
                  (3, (-1.0, 4097.0, 2.5, math.nan), b"jump_cost"), (4, (-1.0, 4097.0, 2.5, math.nan), b"switch_cost"),
                  (5, (-1.0, 1025.0, 0.5, math.nan), b"unvoiced_cost"))
    for i, vals, word in bad_values:
        for bad in vals:
            p = list(good)
            p[i] = bad
            assert call(par_=(C.c_float * 6)(*p)) == -2, (i, bad)
            assert word in lib.sopro_last_error(), (i, bad, lib.sopro_last_error())
    lens2, par2 = (C.c_int32 * 2)(n, 10), (C.c_float * 12)(*(good + good))
    need2 = lib.sopro_f0_workspace_bytes(2, n)
    F = R.frames(n)
    assert lib.sopro_f0_rows_f32(fake, n - 1, lens2, par2, 2, fake, fake, F, fake, None, None, None, fake, need2, None) == -2  # rows would overlap
    assert b"stride" in lib.sopro_last_error()
    assert lib.sopro_f0_rows_f32(fake, n, lens2, par2, 2, fake, fake, F - 1, fake, None, None, None, fake, need2, None) == -2
    assert b"stride" in lib.sopro_last_error()
    # the path entry
    fr = (C.c_int32 * 1)(9)
    needp = lib.sopro_f0_workspace_bytes(1, R.SPAN + 8 * R.H)

    def paths(v=fake, e=fake, fr_=fr, par_=par, rows=1, fcap=9, ws=fake, wsb=needp):
        return lib.sopro_f0_paths(v, e, fr_, par_, rows, fcap, fake, fake, 9, None, ws, wsb, None)

    assert paths(wsb=needp - 1) == -2 and b"ws_bytes" in lib.sopro_last_error()
    assert paths(v=None) == -2 and paths(e=None) == -2 and paths(fr_=None) == -2 and paths(par_=None) == -2 and paths(ws=None) == -2
    assert paths(rows=0) == -2 and paths(fcap=-1) == -2 and paths(fcap=8) == -2 and paths(fr_=(C.c_int32 * 1)(-1)) == -2
    assert paths(par_=(C.c_float * 6)(0.5, -50.0, 24.0, 96.0, 5000.0, 150.0)) == -2 and b"switch_cost" in lib.sopro_last_error()
    fr2 = (C.c_int32 * 2)(9, 3)
    assert lib.sopro_f0_paths(fake, fake, fr2, par2, 2, 9, fake, fake, 8, None, fake, lib.sopro_f0_workspace_bytes(2, R.SPAN + 8 * R.H), None) == -2
    assert b"out_stride" in lib.sopro_last_error()
