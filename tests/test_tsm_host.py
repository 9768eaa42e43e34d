"""Speaking rate, host side: the numpy restatement of the operator (tests/tsm_ref.py) has the properties a time stretch of speech
needs (identity at 1.0, exact length, pitch kept, no splice clicks, level kept), its chunked form equals its one-shot form
exactly, the step / length helpers of ``sopro_amd.hip`` agree with it and with the library, and ``speed`` is a keyword-only
parameter with default 1.0 on every public entry point.  The kernel itself is compared with the restatement in
tests/test_gpu_tsm.py."""
import inspect

import numpy as np
import pytest

import tsm_ref as T
from sopro_amd import hip

SPEEDS = (0.5, 0.75, 0.9, 1.1, 1.25, 1.5, 2.0)
F0S = (90.0, 120.0, 220.0)


def test_speed_one_is_the_identity():
    for x in (T.harmonic(120.0), T.noise_with_silence(), T.harmonic(90.0)[:1000], T.harmonic(90.0)[:479], np.zeros(0, np.float32)):
        y, d = T.tsm(x, 1.0, True)
        assert y.dtype == np.float32 and np.array_equal(y, x) and not d.any()


@pytest.mark.parametrize("f0", F0S)
def test_harmonic_signals_keep_length_pitch_smoothness_and_level(f0):
    x = T.harmonic(f0)
    L = len(x)
    rms_x, step_x = float(np.sqrt((x.astype(np.float64) ** 2).mean())), float(np.abs(np.diff(x)).max())
    for s in SPEEDS:
        y = T.tsm(x, s)
        assert len(y) == (L * 480 * 65536) // T.step_of(s)
        assert np.isfinite(y).all()
        pk = T.peak_hz(y)
        smooth = float(np.abs(np.diff(y)).max()) / step_x
        rms = float(np.sqrt((y.astype(np.float64) ** 2).mean())) / rms_x
        print(f"f0 {f0} speed {s}: len {len(y)} peak {pk:.2f} Hz, max|diff| ratio {smooth:.4f}, rms ratio {rms:.4f}")
        assert abs(pk - f0) <= T.SR / len(y), (s, pk)        # within one bin: the pitch is kept
        assert smooth <= 1.01, (s, smooth)                   # no clicks at the splices
        assert abs(rms - 1.0) <= 0.01, (s, rms)              # the level is kept
    assert len(T.tsm(x, 1.1)) == 65454


def test_noise_with_silent_head_and_tail():
    x = T.noise_with_silence()
    for s in (0.8, 1.3):
        y = T.tsm(x, s)
        assert len(y) == T.out_len(len(x), T.step_of(s)) and np.isfinite(y).all()
        print("noise", s, "rms ratio", float(np.sqrt((y ** 2).mean()) / np.sqrt((x ** 2).mean())))  # (0.95 - 0.96: a record, not a bar)
    assert len(T.tsm(x, 1.3)) == 36923


def test_wherever_the_search_lands_on_the_template_the_output_is_a_copy():
    x = T.harmonic(120.0, seconds=1.0)
    y, d = T.tsm(x, 0.75, True)
    step, p_prev, copies = T.step_of(0.75), 0, 0
    for k in range(1, len(d)):
        p = ((k * step) >> 16) + int(d[k])
        if p == p_prev + T.HS and (k + 1) * T.HS <= len(y) and p + T.HS <= len(x):
            assert np.array_equal(y[k * T.HS: (k + 1) * T.HS], x[p: p + T.HS])
            copies += 1
        p_prev = p
    assert copies > 0


@pytest.mark.parametrize("speed", (0.5, 0.9, 1.3, 2.0))
def test_chunked_feed_equals_one_shot(speed):
    rng = np.random.default_rng(3)
    x = np.concatenate([T.glide(100.0, 180.0, 30000), np.zeros(3000, np.float32), T.noise_with_silence(0.5, seed=4, head=0, tail=2000),
                        T.harmonic(220.0, seconds=0.6)])
    want, wd = T.tsm(x, speed, True)
    for sizes in ([479], [1920], [11520], [int(v) for v in rng.integers(1, 6000, size=37)], [len(x)]):
        y, d, tail = T.tsm_chunked(x, speed, sizes)
        assert np.array_equal(y, want) and np.array_equal(d, wd), sizes[:3]
        assert tail < 1920, (sizes[:3], tail)                # what is kept between calls: the bound derived in include/sopro_hip.h
    short = x[:9000]
    y, d, tail = T.tsm_chunked(short, speed, [1])
    want, wd = T.tsm(short, speed, True)
    assert np.array_equal(y, want) and np.array_equal(d, wd)
    assert tail < 1920, tail                                 # the bound derived in include/sopro_hip.h (SOPRO_TSM_TAIL = 2048)


def test_short_and_empty_rows():
    for n in (0, 1, 100, 479, 480, 481, 1199, 1200):
        x = T.harmonic(150.0)[:n]
        for s in (0.5, 1.0, 1.7, 2.0):
            y, d = T.tsm(x, s, True)
            assert len(y) == T.out_len(n, T.step_of(s)) and len(d) == -(-len(y) // T.HS)
            yc, dc, _ = T.tsm_chunked(x, s, [7, 300])
            assert np.array_equal(yc, y) and np.array_equal(dc, d)
    assert len(T.tsm(np.zeros(0, np.float32), 0.5)) == 0
    z = T.tsm(np.zeros(5000, np.float32), 1.5, True)
    assert not z[0].any() and not z[1].any()                  # silence: d = 0 everywhere


def test_step_and_length_helpers():
    assert hip.tsm_step(1.0) == 480 << 16 and hip.tsm_step(0.5) == 480 << 15 and hip.tsm_step(2.0) == 480 << 17
    for bad in (0.49, 2.01, 0.0, -1.0, float("nan"), float("inf"), "fast", None):
        with pytest.raises(ValueError):
            hip.tsm_step(bad)
    with pytest.raises(ValueError):
        T.step_of(2.5)
    speeds = np.linspace(0.5, 2.0, 301)
    steps = [hip.tsm_step(v) for v in speeds]
    assert steps == [T.step_of(v) for v in speeds] and all(b > a for a, b in zip(steps, steps[1:]))
    for L in (0, 1, 479, 1920, 72000, 768000):
        lens = [hip.tsm_out_len(L, s) for s in steps]
        assert lens == [T.out_len(L, s) for s in steps]
        assert all(b <= a for a, b in zip(lens, lens[1:]))      # monotone: faster is never longer
        assert hip.tsm_out_len(L, 480 << 16) == L
    assert hip.tsm_out_len(0, hip.tsm_step(0.5)) == 0 and hip.tsm_blocks(0) == 0
    assert hip.tsm_out_len(72000, hip.tsm_step(1.1)) == 65454 and hip.tsm_out_len(48000, hip.tsm_step(1.3)) == 36923
    assert [hip.tsm_blocks(m) for m in (1, 480, 481)] == [1, 1, 2]
    assert hip.tsm_steps(1.25, 3) == [hip.tsm_step(1.25)] * 3 and hip.tsm_steps([0.5, 2.0], 2) == [480 << 15, 480 << 17]
    with pytest.raises(ValueError):
        hip.tsm_steps([1.0, 1.0], 3)
    with pytest.raises(ValueError):
        hip.tsm_out_len(10, 1)


def test_library_helpers_agree_with_the_host_arithmetic():
    lib = hip.load()
    for L in (0, 1, 479, 72000, 768000):
        for v in (0.5, 0.77, 1.0, 1.3, 2.0):
            s = hip.tsm_step(v)
            assert lib.sopro_tsm_out_len(L, s) == hip.tsm_out_len(L, s)
            assert lib.sopro_tsm_blocks(hip.tsm_out_len(L, s)) == hip.tsm_blocks(hip.tsm_out_len(L, s))
    assert lib.sopro_tsm_out_len(100, 1) == -1 and lib.sopro_tsm_out_len(-1, 480 << 16) == -1
    assert lib.sopro_tsm_state_bytes(0) == 0 and lib.sopro_tsm_state_bytes(2) == 2 * lib.sopro_tsm_state_bytes(1) > 2 * 2 * 1920 * 4
    # one chunked call never yields more than the bound: blocks are at least 240 input samples apart
    assert lib.sopro_tsm_chunk_out_cap(0) >= (1920 // 240 + 2) * 480 and lib.sopro_tsm_chunk_out_cap(11520) >= (11520 + 1920) // 240 * 480
    assert lib.sopro_tsm_rows_f32(None, 0, None, 0, None, 1, None, 1, None, None, 0, 0, None, None, 0, None) == -2
    assert b"non-NULL" in lib.sopro_last_error()
    assert hip.ABI_VERSION == 43


def test_speed_is_keyword_only_with_default_one_everywhere():
    from sopro_amd import longform, streaming
    from sopro_amd.serving import SynthesisService
    from sopro_amd.tts import SoproTTS

    fns = [SoproTTS.synthesize, SoproTTS.synthesize_batch, SoproTTS.stream, SoproTTS.synthesize_long, SoproTTS.stream_long,
           streaming.SoproTTSStreamer.stream, streaming.stream, longform.synthesize_long, longform.stream_long,
           SynthesisService.submit, SynthesisService.submit_long]
    for fn in fns:
        p = inspect.signature(fn).parameters.get("speed")
        assert p is not None, f"{fn.__qualname__} has no speed parameter"
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 1.0, fn.__qualname__
    # out of scope, but never silently ignored
    for fn in (SoproTTS.stream_batch, streaming.stream_batch, SynthesisService.submit_stream):
        p = inspect.signature(fn).parameters.get("speed")
        assert p is not None and p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 1.0, fn.__qualname__
