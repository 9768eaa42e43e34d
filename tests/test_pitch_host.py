"""Pitch, host side: the numpy restatement of the resampler (tests/pitch_ref.py) does what a band-limited resampler should (its
bank is normalised and symmetric, in-band tones come out at the new frequency to 5e-4 of their amplitude, what would alias is
removed), the chain of stretch and resampler has the properties a pitch shift of speech needs (length, pitch, level, no clicks), the
chunked form equals the one-shot form exactly, the helpers of ``sopro_amd.hip`` agree with the restatement and with the library, and
``pitch`` is a keyword-only parameter with default 0.0 on every public entry point.  The kernel itself is compared with the
restatement in tests/test_gpu_pitch.py."""
import inspect

import numpy as np
import pytest

import pitch_ref as PR
import tsm_ref as T
from sopro_amd import hip

AMP = 0.5
EDGE = 128  # the zero extension rings at the ends: the interior is the output without 128 samples at each end


def _rho(inc):
    return inc / 4294967296.0


def _db(v):
    return 20.0 * np.log10(max(float(v), 1e-30))


# ------------------------------------------------------------------------------------------ the bank
def test_bank_is_normalised_symmetric_and_shared():
    ulp = 2.0 ** -24
    for pitch in (0.0, -12.0, 3.0, 7.0, 12.0):
        inc = PR.inc_of(pitch)
        b = PR.bank(inc)
        assert b.shape == (257, 64) and b.dtype == np.float32
        sums = b.astype(np.float64).sum(axis=1)
        print(f"pitch {pitch}: max |row sum - 1| = {np.abs(sums - 1).max():.3e}")
        assert np.abs(sums - 1.0).max() <= 64 * ulp * 0.5           # every tap is rounded once, |tap| < 1
        assert np.abs(b[::-1, ::-1] - b).max() <= 2 * ulp            # t(256 - p, 63 - j) = -t(p, j)
        assert b[256, 0] == 0.0 and b[0, 63] == 0.0                  # |t| = 32: the window's end
        assert np.abs(b[256, 1:] - b[0, :-1]).max() <= 2 * ulp       # phase 1.0 is phase 0.0 one tap on
        assert np.array_equal(hip.pitch_bank_host(inc), b)
    assert PR.bank(PR.inc_of(-12.0)) is PR.bank(PR.ONE) and PR.bank(PR.inc_of(-0.01)) is PR.bank(PR.ONE)
    assert np.array_equal(hip.pitch_bank_host(1 << 31), hip.pitch_bank_host(1 << 32))
    assert not np.array_equal(PR.bank(PR.inc_of(12.0)), PR.bank(PR.ONE))


# ------------------------------------------------------------------------------------------ the resampler alone, analytic sines
@pytest.mark.parametrize("pitch", (-12.0, -5.0, 4.0, 7.0, 12.0))
def test_resampler_against_analytic_sines(pitch):
    inc = PR.inc_of(pitch)
    rho = _rho(inc)
    n_in = 2 * PR.SR
    t_out = np.arange(PR.out_len(n_in, inc), dtype=np.float64) * rho / PR.SR     # output n reads the input at n * rho
    limit = (0.5 * min(1.0, 1.0 / rho) - 0.0685) * PR.SR
    tones = [hz for hz in (200.0, 3000.0, 8000.0) if hz < limit]
    assert tones
    for hz in tones:
        y = PR.resample(PR.sine(hz, amp=AMP), inc)
        assert len(y) == len(t_out)
        err = float(np.abs(y.astype(np.float64) - AMP * np.sin(2 * np.pi * hz * t_out))[EDGE:-EDGE].max()) / AMP
        print(f"pitch {pitch}: {hz} Hz in band, max |y - ideal| / amplitude = {err:.3e}")
        assert err <= 5e-4, (pitch, hz, err)
    if rho > 1.0:
        nyq_new, nyq_old = 0.5 * PR.SR / rho, 0.5 * PR.SR
        for hz, bar in ((0.5 * (nyq_new + nyq_old), -70.0), (nyq_new + 1.0, -60.0)):
            y = PR.resample(PR.sine(hz, amp=AMP), inc)
            level = _db(np.abs(y[EDGE:-EDGE]).max() / AMP)
            print(f"pitch {pitch}: {hz:.1f} Hz would alias, comes out at {level:.1f} dB")
            assert level <= bar, (pitch, hz, level)


# ------------------------------------------------------------------------------------------ the chain on harmonic signals
@pytest.mark.parametrize("f0", (90.0, 120.0, 220.0))
def test_chain_keeps_length_and_level_and_moves_the_pitch(f0):
    x = T.harmonic(f0)
    L = len(x)
    rms_x, step_x = float(np.sqrt((x.astype(np.float64) ** 2).mean())), float(np.abs(np.diff(x)).max())
    ran = 0
    for pitch in (-12, -7, -3, -1, 1, 3, 7, 12):
        rho = _rho(PR.inc_of(pitch))
        for speed in (1.0, 0.8, 1.25):
            if not 0.5 <= speed / rho <= 2.0:
                with pytest.raises(ValueError):
                    PR.steps_of(speed, pitch)
                continue
            y = PR.chain(x, speed, pitch)
            ran += 1
            assert np.isfinite(y).all()
            dlen = abs(len(y) - L / speed)
            inner = y[EDGE:-EDGE].astype(np.float64)
            bins = abs(T.peak_hz(y) - f0 * rho) / (T.SR / len(y))
            rms = float(np.sqrt((inner ** 2).mean())) / rms_x
            smooth = float(np.abs(np.diff(inner)).max()) / (rho * step_x)
            print(f"f0 {f0} pitch {pitch:+d} speed {speed}: len off by {dlen:.2f}, peak off by {bins:.2f} bins, rms ratio {rms:.4f}, "
                  f"max|diff| ratio {smooth:.4f}")
            assert dlen <= 3.0, (pitch, speed, dlen)
            assert bins <= 1.5, (pitch, speed, bins)
            assert abs(rms - 1.0) <= 0.01, (pitch, speed, rms)
            assert smooth <= 1.25, (pitch, speed, smooth)
    assert ran >= 16


def test_chain_at_pitch_zero_is_the_stretch_and_at_matching_speed_the_resampler():
    x = T.harmonic(120.0, seconds=0.5)
    assert np.array_equal(PR.chain(x, 1.0, 0.0), x)
    assert np.array_equal(PR.chain(x, 1.3, 0.0), T.tsm(x, 1.3))
    assert PR.steps_of(2.0, 12.0) == (480 << 16, 1 << 33) and PR.steps_of(0.5, -12.0) == (480 << 16, 1 << 31)
    assert np.array_equal(PR.chain(x, 2.0, 12.0), PR.resample(x, 1 << 33))  # speed == rho: the stretch is skipped


# ------------------------------------------------------------------------------------------ chunked == one-shot
@pytest.mark.parametrize("pitch", (-12.0, -3.3, 5.0, 12.0))
def test_chunked_feed_equals_one_shot(pitch):
    rng = np.random.default_rng(3)
    inc = PR.inc_of(pitch)
    x = np.concatenate([T.glide(100.0, 180.0, 30000), np.zeros(3000, np.float32), T.noise_with_silence(0.5, seed=4, head=0, tail=2000),
                        T.harmonic(220.0, seconds=0.6)])
    want = PR.resample(x, inc)
    assert len(want) == PR.out_len(len(x), inc)
    for sizes in ([479], [1920], [int(v) for v in rng.integers(1, 6001, size=37)], [len(x)]):
        y, tail = PR.resample_chunked(x, inc, sizes)
        assert np.array_equal(y, want), sizes[:3]
        assert tail < 64, (sizes[:3], tail)                  # the bound derived in include/sopro_hip.h (SOPRO_PITCH_TAIL = 128)
    short = x[28000:37000]
    y, tail = PR.resample_chunked(short, inc, [1])
    assert np.array_equal(y, PR.resample(short, inc)) and tail < 64, tail


def test_short_rows_and_the_identity():
    base = T.harmonic(150.0)
    for n in (0, 1, 31, 32, 33, 63, 64, 65):
        x = base[100: 100 + n]
        for pitch in (-12.0, -3.3, 0.0, 0.01, 5.0, 12.0):
            inc = PR.inc_of(pitch)
            y = PR.resample(x, inc)
            assert y.dtype == np.float32 and len(y) == PR.out_len(n, inc) == hip.pitch_out_len(n, inc)
            for sizes in ([1], [7, 30], [100]):
                yc, tail = PR.resample_chunked(x, inc, sizes)
                assert np.array_equal(yc, y) and tail < 64, (n, pitch, sizes)
        assert np.array_equal(PR.resample(x, PR.ONE), x)      # inc == 2^32: a copy, the bank is not read
    x = T.noise_with_silence(0.3, seed=2, head=100, tail=100)
    assert np.array_equal(PR.resample(x, PR.ONE), x) and np.array_equal(PR.resample_chunked(x, PR.ONE, [500, 3])[0], x)
    assert not np.array_equal(PR.resample(x, PR.ONE + 1)[:7000], x[:7000])   # (one step off the identity is the filter, not a copy)
    assert not PR.resample(np.zeros(5000, np.float32), PR.inc_of(7.0)).any()


# ------------------------------------------------------------------------------------------ helpers
def test_increment_step_and_length_helpers():
    assert hip.pitch_inc(0.0) == 1 << 32 == hip.PITCH_ONE and hip.pitch_inc(12) == 1 << 33 and hip.pitch_inc(-12.0) == 1 << 31
    for bad in (12.01, -12.5, float("nan"), float("inf"), "high", None, [1.0]):
        with pytest.raises(ValueError):
            hip.pitch_inc(bad)
    with pytest.raises(ValueError):
        PR.inc_of(13.0)
    pitches = np.linspace(-12.0, 12.0, 241)
    incs = [hip.pitch_inc(v) for v in pitches]
    assert incs == [PR.inc_of(v) for v in pitches] and all(b > a for a, b in zip(incs, incs[1:]))
    assert hip.pitch_incs(3.0, 2) == [hip.pitch_inc(3.0)] * 2 and hip.pitch_incs([-12, 0, 12], 3) == [1 << 31, 1 << 32, 1 << 33]
    with pytest.raises(ValueError):
        hip.pitch_incs([1.0, 2.0], 3)
    for L in (0, 1, 31, 1920, 72000, 768000):
        lens = [hip.pitch_out_len(L, s) for s in incs]
        assert lens == [PR.out_len(L, s) for s in incs] and all(b <= a for a, b in zip(lens, lens[1:]))
        assert hip.pitch_out_len(L, 1 << 32) == L and hip.pitch_out_len(L, 1 << 31) == 2 * L and hip.pitch_out_len(L, 1 << 33) == L // 2
    for bad in ((10, 1), (-1, 1 << 32), (10, (1 << 33) + 1)):
        with pytest.raises(ValueError):
            hip.pitch_out_len(*bad)
    # the pair: the stretch runs at speed / rho
    for speed in (0.5, 0.8, 1.0, 1.25, 2.0):
        assert hip.prosody_step(speed, 0.0) == (hip.tsm_step(speed), 1 << 32)
        for pitch in (-12.0, -7.0, -1.0, 0.01, 3.0, 12.0):
            rho = _rho(PR.inc_of(pitch))
            if 0.5 <= speed / rho <= 2.0:
                step, inc = hip.prosody_step(speed, pitch)
                assert (step, inc) == PR.steps_of(speed, pitch)
                assert abs(step / (480 * 65536) - speed / rho) <= 1e-7
            else:
                with pytest.raises(ValueError) as e:
                    hip.prosody_step(speed, pitch)
                assert "speed" in str(e.value) and "pitch" in str(e.value)
    assert hip.prosody_steps([1.0, 2.0], [0.0, 12.0], 2) == [(480 << 16, 1 << 32), (480 << 16, 1 << 33)]
    assert hip.prosody_steps(1.25, [0.0, 3.0], 2) == [hip.prosody_step(1.25, 0.0), hip.prosody_step(1.25, 3.0)]
    assert hip.is_plain(hip.prosody_steps(1.0, 0.0, 3)) and not hip.is_plain(hip.prosody_steps(1.0, [0.0, 0.01, 0.0], 3))
    for bad in ((2.5, 0.0), (1.0, 13.0), (2.0, -12.0), (0.5, 12.0), (float("nan"), 0.0), (1.0, "up")):
        with pytest.raises(ValueError):
            hip.prosody_step(*bad)
    with pytest.raises(ValueError):
        hip.prosody_steps(1.0, [0.0, 1.0], 3)


def test_cue_mapping():
    from sopro_amd import align as A

    cues = [A.WordCue("a", 0, 1, 0, 1920), A.WordCue("b", 2, 3, 1920, 28800)]
    for pitch in (-12.0, -3.3, 5.0, 12.0):
        inc = hip.pitch_inc(pitch)
        got = A.shift_cues(cues, inc)
        assert [(c.start_sample, c.end_sample) for c in got] == [(PR.shift_sample(c.start_sample, inc), PR.shift_sample(c.end_sample, inc)) for c in cues]
        assert [(c.text, c.char_start, c.char_end) for c in got] == [(c.text, c.char_start, c.char_end) for c in cues]
        assert A.map_pitch(28800, inc) == hip.pitch_out_len(28800, inc)   # the waveform's end maps to the new length
    assert A.shift_cues(cues, 1 << 32) == cues


def test_library_helpers_agree_with_the_host_arithmetic():
    lib = hip.load()
    for name in ("sopro_pitch_out_len", "sopro_pitch_chunk_out_cap", "sopro_pitch_state_bytes", "sopro_pitch_rows_f32"):
        assert name in hip.SYMBOLS
    for L in (0, 1, 31, 72000, 768000):
        for v in (-12.0, -3.3, 0.0, 5.0, 12.0):
            inc = hip.pitch_inc(v)
            assert lib.sopro_pitch_out_len(L, inc) == hip.pitch_out_len(L, inc) == PR.out_len(L, inc)
    assert lib.sopro_pitch_out_len(100, 1) == -1 and lib.sopro_pitch_out_len(-1, 1 << 32) == -1 and lib.sopro_pitch_out_len(100, (1 << 33) + 1) == -1
    assert lib.sopro_pitch_state_bytes(0) == 0 and lib.sopro_pitch_state_bytes(2) == 2 * lib.sopro_pitch_state_bytes(1) >= 2 * (3 * 8 + 128 * 4)
    for n in (0, 1, 1920, 11520):
        assert lib.sopro_pitch_chunk_out_cap(n) >= 2 * (n + 64) + 2
    assert lib.sopro_pitch_chunk_out_cap(-1) == -1
    assert lib.sopro_pitch_rows_f32(None, 0, None, 0, None, None, None, 1, 1, None, 1, None, 0, 0, None, None) == -2
    assert b"non-NULL" in lib.sopro_last_error()
    assert hip.PITCH_TILE == 2048 and hip.ABI_VERSION == 43


def test_pitch_is_keyword_only_with_default_zero_everywhere():
    from sopro_amd import longform, streaming
    from sopro_amd.serving import SynthesisService
    from sopro_amd.tts import SoproTTS

    fns = [SoproTTS.synthesize, SoproTTS.synthesize_batch, SoproTTS.synthesize_timed, SoproTTS.stream, SoproTTS.synthesize_long,
           SoproTTS.stream_long, streaming.SoproTTSStreamer.stream, streaming.stream, longform.synthesize_long, longform.stream_long,
           SynthesisService.submit, SynthesisService.submit_long]
    for fn in fns:
        p = inspect.signature(fn).parameters.get("pitch")
        assert p is not None, f"{fn.__qualname__} has no pitch parameter"
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 0.0, fn.__qualname__
    # out of scope, but never silently ignored
    for fn in (SoproTTS.stream_batch, streaming.stream_batch, SynthesisService.submit_stream):
        p = inspect.signature(fn).parameters.get("pitch")
        assert p is not None and p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 0.0, fn.__qualname__
