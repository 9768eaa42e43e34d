"""Reference crop selection without a GPU: the numpy restatement against its own definition (a tie is the centre crop, a dense window
is found, a clipped one avoided), the condition that lets the GPU test demand equality (every designed row keeps its blocks away
from the threshold, and its fp32 run picks what its float64 run picks), the ``SpeechCrop`` parameters, and the refusals of the C
entry and of the entry points on the argument path."""
import math

import numpy as np
import pytest
import torch

import crop_ref as R


# ---- the restatement ----
def test_a_row_without_preference_gets_the_centre_crop():
    from sopro_amd import audio

    rng = np.random.default_rng(5)
    for n in (1921, 2554, 5000, 7777):
        for x in (np.zeros(n, np.float32), (0.25 * np.sin(2 * np.pi * 1000.0 * np.arange(n) / R.SR)).astype(np.float32),
                  (0.1 * rng.standard_normal(n)).astype(np.float32)):  # white noise: a constant level, so nothing clears the margin
            p = R.crop_parts(x, R.W0)
            assert p.start == (n - R.W0) // 2 and p.report.row_active == 0
            assert np.array_equal(R.crop(x, R.W0), audio.center_crop_audio(torch.from_numpy(x), R.W0).numpy())


def test_short_rows_come_back_whole():
    for n in (0, 1, 239, 240, 1919, 1920):
        x = R.voice(n).astype(np.float32)
        p = R.crop_parts(x, R.W0)
        assert (p.start, p.out_len, p.o, p.F) == (0, n, 0, n // R.H) and np.array_equal(R.crop(x, R.W0), x)


def test_the_grid_is_anchored_on_the_centre_crop():
    for n in range(R.W0 + 1, R.W0 + 3 * R.H + 2, 7):
        lng, sc, o, F, Wb, kc = R.grid(n, R.W0)
        assert lng and o + kc * R.H == sc and 0 <= kc <= F - Wb and o + F * R.H <= n < o + (F + 1) * R.H + R.H


def test_a_dense_window_is_found_and_a_clipped_one_avoided():
    by = {r.name: r for r in R.designed_batch()}
    late, early = R.reference(by["late"])[0], R.reference(by["early"])[0]
    assert late.report.active == 8 and late.report.centre_active == 0 and late.start > (len(by["late"].x) - R.W0) // 2 > early.start
    clipped, free = R.reference(by["clipped_densest"])[0], R.reference(by["clipped_weight0"])[0]
    assert free.report.clipped == 1 and free.report.active == 8
    assert clipped.report.clipped == 0 and clipped.report.active == 7 and clipped.start != free.start
    two = R.reference(by["two_sided_tie"])[0]
    assert two.score[0] == two.score[12] == two.score.max() and two.k == 0 and two.kc == 6


@pytest.mark.parametrize("row", R.designed_batch(), ids=lambda r: r.name)
def test_designed_row_is_decided_and_decided_alike_in_fp32(row):
    """A condition on the rows, not a measurement of a library: no block within 1e-3 of the threshold (the device's e[f] is within
    240 x 2^-24 = 1.4e-5 of the exact sum and its threshold within a few ulps more), the fp32 run picks the float64 run's start with
    the same flags, and the start is the one the design worked out by hand."""
    p64, p32 = R.reference(row)
    print(f"{row.name}: n {len(row.x)} F {p64.F} start {p64.start} margin {R.margin(row):.3g}")
    assert R.margin(row) >= 1e-3
    assert p32.start == p64.start and np.array_equal(p32.a, p64.a) and np.array_equal(p32.c, p64.c) and p32.report[:7] == p64.report[:7]
    assert row.start is None or p64.start == row.start
    assert p64.out_len == min(len(row.x), row.W)


def test_designed_batch_covers_the_cases():
    rows = {r.name: r for r in R.designed_batch()}
    W, H = R.W0, R.H
    assert {len(r.x) for r in rows.values()} >= {0, 100, W, W + 1, W + H - 1, W + H, W + 2 * H - 1, W + 2 * H}
    assert [len(R.reference(rows[k])[0].score) for k in ("nW+1", "nW+H-1", "nW+H", "nW+2H-1", "nW+2H")] == [1, 1, 1, 2, 3]
    assert R.reference(rows["tone_tie"])[0].o != 0 and rows["W=H_F3"].W == H and R.reference(rows["W=H_F3"])[0].F < R.SMOOTH
    assert R.reference(rows["zero_gap"])[0].e.min() == 0.0 and R.reference(rows["blocks2600"])[0].F == 2600
    assert rows["clipped_weight0"].clip_weight == 0 and np.array_equal(rows["clipped_weight0"].x, rows["clipped_densest"].x)


# ---- parameters ----
def test_speech_crop_defaults_and_ranges():
    import sopro_amd
    from sopro_amd.crop import CropReport, SpeechCrop

    assert sopro_amd.SpeechCrop is SpeechCrop and sopro_amd.CropReport is CropReport
    c = SpeechCrop()
    assert (c.range_db, c.margin_db, c.clip_level, c.clip_weight) == (30.0, 10.0, 0.999, 4) == (R.RANGE_DEFAULT, R.MARGIN_DEFAULT, R.LEVEL_DEFAULT, R.WEIGHT_DEFAULT)
    assert SpeechCrop(6, 0, 8, 0).clip_weight == 0 and SpeechCrop(80, 40, 1e-3, 64.0).clip_weight == 64 and isinstance(SpeechCrop(clip_weight=3.0).clip_weight, int)
    with pytest.raises(Exception):
        c.range_db = 20.0  # frozen
    for kw in (dict(range_db=5.9), dict(range_db=80.1), dict(margin_db=-0.1), dict(margin_db=40.5), dict(clip_level=0.0), dict(clip_level=8.01),
               dict(clip_weight=-1), dict(clip_weight=65), dict(clip_weight=2.5), dict(range_db=math.nan), dict(margin_db=math.inf),
               dict(clip_level="loud"), dict(clip_weight=None), dict(range_db=True)):
        with pytest.raises(ValueError):
            SpeechCrop(**kw)
    assert CropReport._fields == R.Report._fields


def test_per_row_and_check():
    from sopro_amd.crop import SpeechCrop, check_crop, per_row, refuse_without_window

    c = SpeechCrop(20.0, 5.0)
    assert per_row(c, 3) == [c, c, c] and per_row(None, 2) == [None, None]
    assert per_row([c, None, SpeechCrop()], 3) == [c, None, SpeechCrop()]
    with pytest.raises(ValueError):
        per_row([c], 2)
    with pytest.raises(TypeError):
        per_row([c, 30.0], 2)
    with pytest.raises(TypeError):
        per_row("cc", 2)
    assert check_crop(None) is None and check_crop(c) is c
    with pytest.raises(TypeError):
        check_crop(30.0)
    refuse_without_window(None, "x", 0.0), refuse_without_window(c, "x", 1.0)
    for s in (0.0, -1.0, None):
        with pytest.raises(ValueError, match="crop="):
            refuse_without_window(c, "x", s)


def test_constants_match_the_header():
    import os
    import re

    from conftest import ROOT
    from sopro_amd import crop as CR
    from sopro_amd import hip

    src = open(os.path.join(ROOT, "include", "sopro_hip.h")).read()
    val = {k: v.rstrip("f") for k, v in re.findall(r"#define SOPRO_CROP_([A-Z_]+) ([0-9.e+-]+f?)", src)}
    assert (int(val["H"]), int(val["SMOOTH"]), int(val["REPORT_WORDS"])) == (R.H, R.SMOOTH, len(R.Report._fields)) == (hip.CROP_H, hip.CROP_SMOOTH, hip.CROP_REPORT_WORDS)
    assert (float(val["RANGE_MIN"]), float(val["RANGE_MAX"]), float(val["RANGE_DEFAULT"])) == (CR.RANGE_MIN, CR.RANGE_MAX, CR.RANGE_DEFAULT)
    assert (float(val["MARGIN_MIN"]), float(val["MARGIN_MAX"]), float(val["MARGIN_DEFAULT"])) == (CR.MARGIN_MIN, CR.MARGIN_MAX, CR.MARGIN_DEFAULT)
    assert (float(val["LEVEL_MAX"]), float(val["LEVEL_DEFAULT"])) == (CR.LEVEL_MAX, CR.LEVEL_DEFAULT)
    assert (int(val["WEIGHT_MAX"]), int(val["WEIGHT_DEFAULT"])) == (CR.WEIGHT_MAX, CR.WEIGHT_DEFAULT)
    assert hip.ABI_VERSION == 43 and {"sopro_crop_workspace_bytes", "sopro_crop_rows_f32"} <= set(hip.SYMBOLS) and isinstance(hip.crop_calls, int)


def test_c_entry_refuses_bad_arguments_without_a_device():
    """Every check of sopro_crop_rows_f32 comes before its first launch, so the refusals can be seen without a GPU."""
    import ctypes as C

    from sopro_amd import hip

    lib = hip.load()
    assert lib.sopro_crop_workspace_bytes(0, 100) == -1 and lib.sopro_crop_workspace_bytes(1, -1) == -1
    assert lib.sopro_crop_workspace_bytes(1, (1 << 24) + 1) == -1
    assert lib.sopro_crop_workspace_bytes(2, 1000) == 2 * (3 * 4 + 1) * 4 and lib.sopro_crop_workspace_bytes(1, 0) == 4
    n = 5000
    lens, good = (C.c_int32 * 1)(n), (C.c_float * 4)(30.0, 10.0, 0.999, 4.0)
    fake = 1 << 12  # (never dereferenced: the call is refused first)
    need = lib.sopro_crop_workspace_bytes(1, n)

    def call(lens_=lens, par=good, ws=fake, wsb=need, rows=1, win=1920, starts=fake):
        return lib.sopro_crop_rows_f32(fake, n, lens_, par, rows, win, fake, n, starts, None, None, ws, wsb, None)

    assert call(wsb=need - 1) == -2 and b"ws_bytes" in lib.sopro_last_error()
    assert call(ws=None) == -2 and call(lens_=None) == -2 and call(par=None) == -2 and call(starts=None) == -2
    for win in (0, -240, 239, 1921, 100):
        assert call(win=win) == -2 and b"win" in lib.sopro_last_error(), win
    for bad, word in (((5.0, 10.0, 0.999, 4.0), b"range_db"), ((81.0, 10.0, 0.999, 4.0), b"range_db"), ((30.0, -1.0, 0.999, 4.0), b"margin_db"),
                      ((30.0, 41.0, 0.999, 4.0), b"margin_db"), ((30.0, 10.0, -0.5, 4.0), b"clip_level"), ((30.0, 10.0, 8.5, 4.0), b"clip_level"),
                      ((30.0, 10.0, 0.999, 65.0), b"clip_weight"), ((30.0, 10.0, 0.999, 2.5), b"clip_weight"), ((30.0, 10.0, 0.999, -1.0), b"clip_weight"),
                      ((math.nan, 10.0, 0.999, 4.0), b"range_db"), ((30.0, math.nan, 0.999, 4.0), b"margin_db"),
                      ((30.0, 10.0, math.nan, 4.0), b"clip_level"), ((30.0, 10.0, 0.999, math.nan), b"clip_weight")):
        assert call(par=(C.c_float * 4)(*bad)) == -2, bad
        assert word in lib.sopro_last_error(), (bad, lib.sopro_last_error())
    assert call(lens_=(C.c_int32 * 1)(-1)) == -2 and call(lens_=(C.c_int32 * 1)((1 << 24) + 1)) == -2
    assert call(rows=0) == -2 and call(rows=65536) == -2
    lens2, par2 = (C.c_int32 * 2)(n, 10), (C.c_float * 8)(30.0, 10.0, 0.999, 4.0, 0.0, 0.0, 0.0, 0.0)
    need2 = lib.sopro_crop_workspace_bytes(2, n)
    assert lib.sopro_crop_rows_f32(fake, n - 1, lens2, par2, 2, 1920, fake, 1920, fake, None, None, fake, need2, None) == -2  # rows would overlap
    assert b"stride" in lib.sopro_last_error()
    assert lib.sopro_crop_rows_f32(fake, n, lens2, par2, 2, 1920, fake, 1919, fake, None, None, fake, need2, None) == -2
    assert b"stride" in lib.sopro_last_error()


# ---- the entry points refuse crop= where there is no waveform or no window (argument path: no engine, no device) ----
class _Tok:
    vocab_size = 512

    def encode(self, text):
        return [1, 2, 3]


def _bare_tts():
    """A facade without an engine: whatever touches the model, the codec or the device fails loudly with AttributeError."""
    from sopro_amd import SoproTTS
    from sopro_amd.config import SoproTTSConfig

    return SoproTTS(None, SoproTTSConfig(), _Tok(), None, "cpu")


def test_entry_points_refuse_crop_without_a_waveform_or_a_window():
    from sopro_amd import SpeechCrop

    tts, c = _bare_tts(), SpeechCrop()
    toks = torch.zeros(4, 32, dtype=torch.long)
    ref = object()  # (stands for a PreparedReference: it is never looked into)
    for name in ("encode_reference", "encode_speaker", "prepare_reference"):
        with pytest.raises(ValueError, match="crop="):
            getattr(tts, name)(ref_tokens_tq=toks, crop=c)
        for s in (0.0, -1.0):
            with pytest.raises(ValueError, match="crop="):
                getattr(tts, name)(ref_audio_path="x.wav", ref_seconds=s, crop=c)
    for name in ("synthesize", "synthesize_timed", "stream", "stream_timed", "synthesize_long", "stream_long"):
        fn = getattr(tts, name)
        with pytest.raises(ValueError, match="crop="):
            fn("hello there", ref_tokens_tq=toks, crop=c)
        with pytest.raises(ValueError, match="crop="):
            fn("hello there", ref=ref, crop=c)
    with pytest.raises(TypeError):
        tts.prepare_reference(ref_audio_path="x.wav", crop=12.0)


def test_entry_points_take_the_keyword():
    import inspect

    from sopro_amd import SoproTTS, longform, streaming
    from sopro_amd.codec import MimiCodec

    for fn in (SoproTTS.encode_reference, SoproTTS.encode_speaker, SoproTTS.prepare_reference, SoproTTS.synthesize, SoproTTS.synthesize_timed,
               streaming.SoproTTSStreamer.stream, streaming.SoproTTSStreamer.stream_timed, longform.synthesize_long, longform.stream_long,
               MimiCodec.encode_file, MimiCodec.reference_waveform):
        p = inspect.signature(fn).parameters["crop"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn.__qualname__
