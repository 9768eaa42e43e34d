"""Reference denoising without a GPU: the numpy restatement against its own definition (perfect reconstruction, ranges, an
objective SNR gain on synthetic material), the ``Denoise`` parameters, and the refusals of the entry points on the argument path."""
import math

import numpy as np
import pytest
import torch

import denoise_ref as R


# ---- the restatement ----
def test_zero_attenuation_reproduces_the_input():
    """g_min = 1 forces G = 1 everywhere: what is left is analysis, synthesis and overlap-add, and w^2 sums to 2 over four frames."""
    rng = np.random.default_rng(3)
    for n in (1, 129, 3001):
        x = rng.standard_normal(n)
        y = R.denoise(x, atten_db=0.0)
        assert y.shape == x.shape
        assert float(np.abs(y - x).max()) <= 1e-12


def test_window_is_power_complementary():
    w2 = R.window() ** 2
    assert float(np.abs(w2.reshape(4, R.H).sum(axis=0) - 2.0).max()) < 1e-14


def test_zeros_in_zeros_out():
    p = R.denoise_parts(np.zeros(1000))
    assert np.array_equal(p.y, np.zeros(1000)) and p.input_db == pytest.approx(-200.0) and p.removed_db == pytest.approx(0.0)


@pytest.mark.parametrize("row", R.designed_batch(), ids=lambda r: r.name)
def test_gain_range_and_length(row):
    p64, p32 = R.reference(row)
    g_min = 10.0 ** (-row.atten_db / 20.0)
    assert p64.y.shape == row.x.shape and p32.y.shape == row.x.shape
    assert p64.G.shape == (R.n_frames(len(row.x)), R.BINS)
    assert float(p64.G.min()) >= g_min and float(p64.G.max()) <= 1.0
    assert bool(np.isfinite(p64.y).all()) and bool(np.isfinite(p32.y).all())


def test_designed_batch_covers_the_lengths():
    lens = [len(r.x) for r in R.designed_batch()]
    for n in (1, 2, 127, 128, 129, 511, 512, 513, 94 * 128, 95 * 128 + 1, 189 * 128 + 5):
        assert n in lens
    names = {r.name for r in R.designed_batch()}
    assert {"voice_white", "voice_pink", "voice_zero_run", "all_zero", "scale20"} <= names


def test_float32_run_stays_close_to_float64():
    """The definition is well conditioned, which is why the GPU bar (8 x this deviation) is honest.  Bound: 8 fp32 ulps of the row's
    peak (8 x 2^-24 = 4.8e-7).  A sample passes 18 butterfly stages on its way through the two transforms and four overlap-adds; as a
    random walk of half-ulp roundings that is sqrt(22) / 2 = 2.3 ulps, and the gain (a ratio below 1) adds no more than its own
    rounding, so 8 leaves a factor 3 for the worst sample of a row."""
    for row in R.designed_batch():
        p64, p32 = R.reference(row)
        peak = float(np.abs(row.x).max())
        if peak > 0:
            assert float(np.abs(p32.y - p64.y).max()) <= 8 * 2.0 ** -24 * peak, row.name


def test_minimum_window_is_centred_and_clipped():
    x = R.designed_batch()[10].x  # 189 * 128 + 5 samples: the full span
    p = R.denoise_parts(x)
    F = p.S.shape[0]
    for f in (0, 93, 94, 95, F - 95, F - 1):
        lo, hi = max(0, f - R.SPAN), min(F - 1, f + R.SPAN)
        assert np.array_equal(p.M[f], p.S[lo: hi + 1].min(axis=0))


def test_snr_gain_white():
    s, x = R.noisy_voice(4.0, "white", snr=10.0, seed=1)
    assert R.snr_db(s, x) == pytest.approx(10.0, abs=1e-9)
    out = R.snr_db(s, R.denoise(x))
    print(f"white noise: 10.0 dB in, {out:.2f} dB out")
    assert out >= 15.0


def test_snr_gain_pink():
    s, x = R.noisy_voice(4.0, "pink", snr=10.0, seed=2)
    out = R.snr_db(s, R.denoise(x))
    print(f"1/f noise: 10.0 dB in, {out:.2f} dB out")
    assert out >= 13.0


# ---- parameters ----
def test_denoise_defaults_and_ranges():
    import sopro_amd
    from sopro_amd.denoise import Denoise

    assert sopro_amd.Denoise is Denoise
    d = Denoise()
    assert (d.atten_db, d.bias) == (15.0, 3.0) == (R.ATTEN_DEFAULT, R.BIAS_DEFAULT)
    assert Denoise(0, 1).atten_db == 0.0 and Denoise(40, 8).bias == 8.0
    with pytest.raises(Exception):
        d.bias = 2.0  # frozen
    for kw in (dict(atten_db=-0.1), dict(atten_db=40.5), dict(bias=0.99), dict(bias=8.01), dict(atten_db=math.nan), dict(bias=math.inf),
               dict(atten_db="loud"), dict(bias=None), dict(atten_db=True)):
        with pytest.raises(ValueError):
            Denoise(**kw)


def test_per_row_and_check():
    from sopro_amd.denoise import Denoise, check_denoise, per_row

    d = Denoise(20.0, 2.0)
    assert per_row(d, 3) == [d, d, d] and per_row(None, 2) == [None, None]
    assert per_row([d, None, Denoise()], 3) == [d, None, Denoise()]
    with pytest.raises(ValueError):
        per_row([d], 2)
    with pytest.raises(TypeError):
        per_row([d, 15.0], 2)
    with pytest.raises(TypeError):
        per_row("dd", 2)
    assert check_denoise(None) is None and check_denoise(d) is d
    with pytest.raises(TypeError):
        check_denoise(15.0)


def test_constants_match_the_header():
    import os
    import re

    from conftest import ROOT
    from sopro_amd import denoise as D
    from sopro_amd import hip

    src = open(os.path.join(ROOT, "include", "sopro_hip.h")).read()
    val = {k: v.rstrip("f") for k, v in re.findall(r"#define SOPRO_DN_([A-Z_]+) ([0-9.e+-]+f?)", src)}
    assert (int(val["N"]), int(val["H"]), int(val["BINS"]), int(val["SPAN"])) == (R.N, R.H, R.BINS, R.SPAN) == (hip.DN_N, hip.DN_H, hip.DN_BINS, hip.DN_SPAN)
    assert (float(val["BETA"]), float(val["ALPHA"]), float(val["FLOOR"])) == (R.BETA, R.ALPHA, R.FLOOR)
    assert (float(val["ATTEN_MIN"]), float(val["ATTEN_MAX"]), float(val["ATTEN_DEFAULT"])) == (D.ATTEN_MIN, D.ATTEN_MAX, D.ATTEN_DEFAULT)
    assert (float(val["BIAS_MIN"]), float(val["BIAS_MAX"]), float(val["BIAS_DEFAULT"])) == (D.BIAS_MIN, D.BIAS_MAX, D.BIAS_DEFAULT)


def test_c_entry_refuses_bad_arguments_without_a_device():
    """Every check of sopro_denoise_rows_f32 comes before its first launch, so the refusals can be seen without a GPU."""
    import ctypes as C

    from sopro_amd import hip

    lib = hip.load()
    assert lib.sopro_denoise_workspace_bytes(0, 100) == -1 and lib.sopro_denoise_workspace_bytes(1, -1) == -1
    assert lib.sopro_denoise_workspace_bytes(1, (1 << 24) + 1) == -1
    assert lib.sopro_denoise_workspace_bytes(2, 1000) == 2 * (8 + 3) * (2 * 257 + 2 * 257 + 2) * 4
    lens, good = (C.c_int32 * 1)(1000), (C.c_float * 2)(15.0, 3.0)
    fake = 1 << 12  # (never dereferenced: the call is refused first)
    need = lib.sopro_denoise_workspace_bytes(1, 1000)
    call = lambda lens_, par, ws, wsb, rows=1: lib.sopro_denoise_rows_f32(fake, 1000, lens_, par, rows, fake, 1000, None, ws, wsb, None)  # noqa: E731
    assert call(lens, good, fake, need - 1) == -2 and b"ws_bytes" in lib.sopro_last_error()
    assert call(lens, good, None, need) == -2
    assert call(None, good, fake, need) == -2 and call(lens, None, fake, need) == -2
    for bad in ((41.0, 3.0), (-1.0, 3.0), (15.0, 0.5), (15.0, 9.0), (math.nan, 3.0), (15.0, math.nan)):
        assert call(lens, (C.c_float * 2)(*bad), fake, need) == -2, bad
        assert b"atten_db" in lib.sopro_last_error() or b"bias" in lib.sopro_last_error()
    assert call((C.c_int32 * 1)(-1), good, fake, need) == -2
    assert call(lens, good, fake, need, rows=0) == -2
    lens2, par2 = (C.c_int32 * 2)(1000, 10), (C.c_float * 4)(15.0, 3.0, 0.0, 0.0)
    assert lib.sopro_denoise_rows_f32(fake, 999, lens2, par2, 2, fake, 1000, None, fake, 2 * need, None) == -2  # rows would overlap
    assert lib.sopro_denoise_rows_f32(fake, 1000, lens2, par2, 2, fake, 999, None, fake, 2 * need, None) == -2
    assert b"stride" in lib.sopro_last_error()


# ---- the entry points refuse denoise= where there is no waveform (argument path: no engine, no device) ----
class _Tok:
    vocab_size = 512

    def encode(self, text):
        return [1, 2, 3]


def _bare_tts():
    """A facade without an engine: whatever touches the model, the codec or the device fails loudly with AttributeError."""
    from sopro_amd import SoproTTS
    from sopro_amd.config import SoproTTSConfig

    return SoproTTS(None, SoproTTSConfig(), _Tok(), None, "cpu")


def test_entry_points_refuse_denoise_without_a_waveform():
    from sopro_amd import Denoise

    tts, d = _bare_tts(), Denoise()
    toks = torch.zeros(4, 32, dtype=torch.long)
    ref = object()  # (stands for a PreparedReference: it is never looked into)
    for name in ("encode_reference", "encode_speaker", "prepare_reference"):
        with pytest.raises(ValueError, match="denoise="):
            getattr(tts, name)(ref_tokens_tq=toks, denoise=d)
    for name in ("synthesize", "synthesize_timed", "stream", "stream_timed", "synthesize_long", "stream_long"):
        fn = getattr(tts, name)
        with pytest.raises(ValueError, match="denoise="):
            fn("hello there", ref_tokens_tq=toks, denoise=d)
        with pytest.raises(ValueError, match="denoise="):
            fn("hello there", ref=ref, denoise=d)
    with pytest.raises(TypeError):
        tts.prepare_reference(ref_audio_path="x.wav", denoise=15.0)
    with pytest.raises(TypeError):
        tts.prepare_reference(ref_audio_path="x.wav", denoise=d, report={})


def test_entry_points_take_the_keywords():
    import inspect

    from sopro_amd import SoproTTS, longform, streaming
    from sopro_amd.codec import MimiCodec

    for fn in (SoproTTS.encode_reference, SoproTTS.encode_speaker, SoproTTS.prepare_reference, SoproTTS.synthesize, SoproTTS.synthesize_timed,
               streaming.SoproTTSStreamer.stream, streaming.SoproTTSStreamer.stream_timed, longform.synthesize_long, longform.stream_long,
               MimiCodec.encode_file, MimiCodec.reference_waveform):
        ps = inspect.signature(fn).parameters
        for k in ("denoise", "report"):
            assert ps[k].kind is inspect.Parameter.KEYWORD_ONLY and ps[k].default is None, (fn.__qualname__, k)
