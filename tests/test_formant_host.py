"""Formant control without a GPU: the numpy restatement (tests/formant_ref.py) against its own definition - reconstruction, a synthetic
vowel whose envelope and pitch are measured before and after - and the host side of ``formant=``: validation, per-row values, the
chain's order, the refusal wording and the cues."""
import numpy as np
import pytest

import formant_ref as R
import pitch_ref as PR
from sopro_amd import effects as E
from sopro_amd import hip

BIN_HZ = R.SR / R.N  # 46.875
# The allowed error of an envelope peak, in Hz.  Measured with the restatement on the vowel below: the peak of L sits 59.8 Hz from
# 2^(4/12) times its place after formant=+4 at pitch 0, and 16.1 Hz from its place after pitch -4 with formant=0 (the harmonics
# sample the envelope every 120 Hz, and L follows the spectral tilt as well as the resonances).  One bin is 46.9 Hz, the floor of
# this figure; 1.25 x the larger measurement is used.
PEAK_TOL_HZ = 75.0
assert PEAK_TOL_HZ >= BIN_HZ


@pytest.mark.parametrize("n", [1, 127, 128, 129, 513, 5000])
def test_unit_gain_reconstructs_the_row(n):
    x = np.random.default_rng(n).standard_normal(n)
    y = R.warp(x, 1.0)
    assert y.shape == x.shape and float(np.abs(y - x).max()) <= 8 * np.finfo(np.float64).eps * max(1.0, float(np.abs(x).max()))
    assert R.warp(np.zeros(0), 0.8).shape == (0,)
    z = R.warp(np.zeros(n), R.inv_of(4.0))
    assert z.shape == (n,) and not z.any()  # an all-zero frame has a flat envelope: zeros out


def test_the_vowel_s_envelope_moves_and_its_pitch_stays():
    """120 Hz harmonics under resonances at 700 and 1200 Hz.  The 32 liftered coefficients cannot tell resonances 500 Hz apart (the
    finest term of L has a period of 512 / 31 bins, 774 Hz): L has one maximum between them, and that maximum is what is followed."""
    v = R.vowel(R.SR)
    lag = R.pitch_lag(v)
    assert lag == 200
    base = R.envelope_peaks(v)
    assert len(base) == 1 and R.RES[0] < base[0] < R.RES[1]
    ratio = 2.0 ** (4.0 / 12.0)
    up = R.formant(v, 4.0)
    peaks = R.envelope_peaks(up)
    print("formant=+4: peak", peaks, "expected", [p * ratio for p in base])
    assert len(peaks) == 1 and abs(peaks[0] - base[0] * ratio) <= PEAK_TOL_HZ
    assert abs(peaks[0] - base[0]) > 2 * PEAK_TOL_HZ  # (it did move)
    assert R.pitch_lag(up) == lag
    # pitch -4 moves everything; formant=0 puts the envelope back and leaves the pitch where the shift took it
    low = PR.shift(v.astype(np.float32), -4.0).astype(np.float64)
    moved = R.envelope_peaks(low)
    assert len(moved) == 1 and abs(moved[0] - base[0] / ratio) <= PEAK_TOL_HZ
    back = R.formant(low, 0.0, -4.0)
    peaks = R.envelope_peaks(back)
    print("pitch=-4, formant=0: peak", peaks, "expected", base)
    assert len(peaks) == 1 and abs(peaks[0] - base[0]) <= PEAK_TOL_HZ
    assert abs(R.pitch_lag(back) - lag * ratio) <= 1 and R.pitch_lag(back) == R.pitch_lag(low)


def test_the_gain_is_clamped_and_the_parameter_is_one_fp32_value():
    assert R.inv_of(None) == 1.0 and R.inv_of(-3.0, -3.0) == 1.0
    for f, p in ((4.0, 0.0), (0.0, -3.0), (12.0, 0.0), (-7.5, 2.0)):
        inv = R.inv_of(f, p)
        assert inv == float(np.float32(inv)) == hip.formant_inv(f, p) and abs(inv - 2.0 ** (-(f - p) / 12.0)) <= 2.0 ** -24 * inv
    assert hip.formant_inv(12.0, 0.0) == 0.5 and hip.formant_inv(-12.0, 0.0) == 2.0 and hip.formant_inv(0.0, 12.0) == 2.0
    # a line spectrum on silence asks for more than 18 dB between its peaks and its floor: the output stays bounded by the clamp
    x = 0.5 * np.sin(2 * np.pi * 3000.0 * np.arange(4000) / R.SR)
    y = R.formant(x, 12.0)
    assert np.isfinite(y).all() and float(np.abs(y).max()) <= 0.5 * np.exp(R.GAIN_MAX) * 1.01


def test_validation():
    assert (hip.FM_N, hip.FM_H, hip.FM_Q, hip.FM_STATE) == (R.N, R.H, R.Q, 896) and hip.ABI_VERSION == 43
    assert {"sopro_formant_workspace_bytes", "sopro_formant_state_bytes", "sopro_formant_chunk_out_cap", "sopro_formant_rows_f32"} <= set(hip.SYMBOLS)
    assert isinstance(hip.formant_calls, int)
    for bad in (dict(formant=12.5), dict(formant=-12.01), dict(formant=float("nan")), dict(formant="high"), dict(formant=3.0, pitch=-10.0),
                dict(formant=-6.0, pitch=7.0), dict(formant=0.0, pitch=13.0)):
        with pytest.raises(ValueError):
            E.Effects.of(**bad)
    assert E.Effects.of().plain and E.Effects.of(formant=None, pitch=0.0).plain
    assert E.Effects.of(formant=0.0).plain                       # formant equal to pitch: sigma = 1
    fx = E.Effects.of(pitch=-3.0, formant=-3.0)
    assert fx.inv == 1.0 and not fx.plain and fx.inc != hip.PITCH_ONE  # (the pitch stage still has work; the warp has none)
    assert E.Effects.of(formant=1e-9).plain                      # rounds to 1 as fp32: nothing to launch
    fx = E.Effects.of(pitch=-3.0, formant=0.0)
    assert not fx.plain and fx.inv == R.inv_of(0.0, -3.0) and fx.inv < 1.0
    assert E.Effects.of(formant=2.0).inv == R.inv_of(2.0) and not E.Effects.of(formant=2.0).plain
    # positional construction of the four earlier fields keeps its meaning
    old = E.Effects(1.25, -2.0, None, None)
    assert (old.speed, old.pitch, old.silence, old.watermark, old.formant) == (1.25, -2.0, None, None, None) and old.inv == 1.0
    assert E.Effects(1.0, 0.0, None, None, 5.0).formant == 5.0
    lib = hip.load()
    assert lib.sopro_formant_workspace_bytes(2, 1000) == 2 * (8 + 3) * 512 * 4 and lib.sopro_formant_workspace_bytes(1, 0) == 0
    assert lib.sopro_formant_workspace_bytes(0, 10) == -1 and lib.sopro_formant_workspace_bytes(1, (1 << 24) + 1) == -1
    assert lib.sopro_formant_state_bytes(3) == 3 * 2 * 896 * 4 and lib.sopro_formant_chunk_out_cap(100) == 612
    assert lib.sopro_formant_rows_f32(None, 0, None, None, 1, None, None, 0, 0, None, 0, 0, None, None, 0, None) == -2
    assert b"lens, inv" in lib.sopro_last_error()


def test_per_row_values():
    fxs = E.per_row(1.0, [0.0, -3.0, 2.0, 0.0], None, None, 4, [None, 0.0, 2.0, 4.0])
    assert [fx.inv for fx in fxs] == [1.0, R.inv_of(0.0, -3.0), 1.0, R.inv_of(4.0)]
    assert [fx.plain for fx in fxs] == [True, False, False, False]
    assert [fx.inv for fx in E.per_row(1.0, 0.0, None, None, 3, 2.0)] == [R.inv_of(2.0)] * 3
    assert all(fx.plain for fx in E.per_row(1.0, 0.0, None, None, 2))  # the keyword left out: as before
    with pytest.raises(ValueError):
        E.per_row(1.0, 0.0, None, None, 3, [1.0, 2.0])
    with pytest.raises(ValueError):
        E.per_row(1.0, [0.0, 8.0], None, None, 2, [0.0, -6.0])


def test_refuse_and_cues():
    E.refuse("x")
    E.refuse("x", formant=None)
    E.refuse("x", formant=0.0)
    with pytest.raises(NotImplementedError, match=r"x has no formant control \(formant=2\.0\)"):
        E.refuse("x", formant=2.0)
    with pytest.raises(NotImplementedError, match="pitch control"):  # (the pitch is refused first, as before)
        E.refuse("x", pitch=-3.0, formant=-3.0)
    with pytest.raises(ValueError):
        E.refuse("x", formant=13.0)
    from sopro_amd import align as A

    words = [A.WordCue("a", 0, 1, 0, 1920), A.WordCue("b", 2, 3, 1920, 5760)]
    assert E.map_cues(words, E.Effects.of(formant=3.0)) == words  # no sample moves
    with_pitch = E.map_cues(words, E.Effects.of(pitch=-3.0))
    assert E.map_cues(words, E.Effects.of(pitch=-3.0, formant=0.0)) == with_pitch and with_pitch != words


class _Stage:
    def __init__(self, name, *a, **k):
        self.name = name


def test_the_chain_places_the_stage_third(monkeypatch):
    from sopro_amd.silence import Silence
    from sopro_amd.watermark import Watermark

    for cls in ("TimeStretchState", "PitchShiftState", "FormantState", "SilenceState", "WatermarkState"):
        monkeypatch.setattr(hip, cls, lambda *a, _n=cls, **k: _Stage(_n, *a, **k))
    fx = E.Effects.of(1.25, -3.0, Silence(), Watermark(key=5), 0.0)
    assert [s.name for s in E.Chain.of(fx, "cuda:0").stages] == ["TimeStretchState", "PitchShiftState", "FormantState", "SilenceState", "WatermarkState"]
    assert [s.name for s in E.Chain.of(E.Effects.of(formant=2.0), "cuda:0").stages] == ["FormantState"]
    assert [s.name for s in E.Chain.of(E.Effects.of(pitch=-3.0, formant=-3.0), "cuda:0").stages] == ["TimeStretchState", "PitchShiftState"]
    assert E.Chain.of(E.Effects.of(formant=0.0), "cuda:0").stages == []
