"""Watermark, host side: the numpy restatement (tests/wm_ref.py) has the carrier statistics a spread-spectrum mark needs, the
embedder keeps length and silence and stays inside alpha * g(n), the chunked form equals the one-shot form exactly, the detector
finds the mark - tag and offset exact - on the speech-like signals of tests/tsm_ref.py after PCM16, cropping, gain and mild noise,
and finds nothing on unmarked clips or with another key; the host tables of ``sopro_amd.watermark`` equal the restatement; and
``watermark`` is a keyword-only parameter with default None on every public entry point.  The kernels are compared with the
restatement in tests/test_gpu_wm.py.

Scores measured with this file (min of the two lanes' z; tag 173 and the offsets 0 / 5191 / 5191 recovered in every case):
    signal                        clean   PCM16 + crop + gain   + noise at -40 dB of peak
    harmonic(120) 3 s              43.0        42.9                 42.4
    harmonic(220, 1 s)             42.5        41.9                 40.3
    glide + gap + noise burst      14.5        13.6                 12.4
    low-passed random walk 3 s     42.4        42.3                 40.9
Unmarked clips and marked clips read with key ^ 1 reach at most 5.5 in max(z_0, z_1): not present.  Known weak case, not asserted:
a white-noise host (noise_with_silence(2.0, seed=1)) scores 7.0 at -30 dB and 3.7 at -36 dB."""
import functools
import inspect

import numpy as np
import pytest

import tsm_ref as T
import wm_ref as W
from sopro_amd import hip
from sopro_amd import watermark as wm

KEY, TAG = 0x0123456789ABCDEF, 173


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def glide_noise():
    return np.concatenate([T.glide(100, 180, 30000), np.zeros(3000, np.float32), T.noise_with_silence(0.5, seed=4, head=0, tail=2000)])


SIGNALS = {
    "harmonic120": lambda: T.harmonic(120),
    "harmonic220_1s": lambda: T.harmonic(220, 1.0),
    "glide_noise": glide_noise,
    "random_walk": W.pinkish,
}


@functools.lru_cache(maxsize=None)
def _signal(name):
    x = SIGNALS[name]()
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _marked(name):
    y = W.embed(_signal(name), KEY, TAG)
    y.setflags(write=False)
    return y


# ------------------------------------------------------------------------------------------ carrier
def test_carrier_values_balance_and_key_separation():
    car = W.carrier(KEY, TAG)
    assert car.dtype == np.int8 and car.shape == (W.P,) and set(np.unique(car)) <= {-2, 0, 2}
    tpl = W.templates(KEY)
    assert tpl.dtype == np.int8 and tpl.shape == (2, W.P) and set(np.unique(tpl)) <= {-2, 0, 2}
    c0, c1 = W.lanes(KEY)
    assert np.array_equal(c0[0::2], c0[1::2]) and set(np.unique(c0)) == {-1, 1}  # two samples per chip
    for c in (c0, c1):
        print("lane sum", int(c.astype(np.int64).sum()))
        assert abs(int(c.astype(np.int64).sum())) <= 4 * np.sqrt(W.NC)
    assert np.array_equal(car, c0 + np.roll(c1, W.SHIFT * TAG))
    assert 256 * W.SHIFT == W.P and np.array_equal(W.carrier(KEY, 0), c0 + c1)
    for bit in (0, 1, 31, 32, 63):
        for a, b in zip(W.lanes(KEY), W.lanes(KEY ^ (1 << bit))):
            rho = float(np.dot(a.astype(np.float64), b.astype(np.float64))) / W.P
            print(f"bit {bit}: normalised correlation {rho:+.4f}")
            assert abs(rho) < 0.08
    rho = float(np.dot(c0.astype(np.float64), c1.astype(np.float64))) / W.P  # the two lanes of one key
    assert abs(rho) < 0.08


def test_host_tables_equal_the_restatement():
    for key, tag in ((KEY, TAG), (0, 0), ((1 << 64) - 1, 255), (0x9E3779B97F4A7C15, 1)):
        assert np.array_equal(wm.carrier_host(key, tag), W.carrier(key, tag))
        assert np.array_equal(wm.templates_host(key), W.templates(key))
        assert np.array_equal(wm.lanes_host(key), np.stack(W.lanes(key)))
    for db in (-48.0, -30.0, -18.0, -33.3):
        assert np.float32(wm.Watermark(1, 0, db).alpha) == W.alpha_of(db)
    assert (wm.HS, wm.P, wm.CH, wm.SHIFT, wm.NC) == (W.HS, W.P, W.CH, W.SHIFT, W.NC) == (480, 8192, 2, 32, 4096)
    assert wm.THRESHOLD == W.THRESHOLD == 6.0
    r = W.detect(_marked("harmonic220_1s"), KEY)
    assert wm.result_of(r.offset, (r.offset + W.SHIFT * TAG) % W.P, r.z_sync, r.z_tag) == wm.WatermarkResult(*r)
    assert wm.result_of(0, 0, 0.0, 0.0) == wm.WatermarkResult(False, 0.0, 0, 0, 0.0, 0.0)


# ------------------------------------------------------------------------------------------ embedder
@pytest.mark.parametrize("name", sorted(SIGNALS))
def test_embed_keeps_length_and_stays_inside_the_envelope(name):
    x, y = _signal(name), _marked(name)
    g = W.envelope(x)
    assert len(y) == len(x) and y.dtype == np.float32
    alpha = float(W.alpha_of(-30.0))
    slack = np.abs(x).astype(np.float64) * 2.0 ** -23  # the one rounding of the final sum
    assert np.all(np.abs(y.astype(np.float64) - x) <= alpha * g.astype(np.float64) * (1 + 2.0 ** -22) + slack)
    assert np.all(g >= np.abs(x))  # the envelope covers the signal: the mark is at most alpha of the local peak
    assert np.any(y != x)


def test_embed_silence_short_rows_and_rows_without_a_mark():
    for L in (0, 1, 479, 480, 481, 5000):
        assert not W.embed(np.zeros(L, np.float32), KEY, TAG).any()
    x = _signal("glide_noise")[:5000].copy()
    x[0] = -0.0
    assert np.array_equal(_bits(W.embed(x, None)), _bits(x))  # bit for bit, the sign of a zero included
    y, _ = W.embed_chunked(x, [700], None)
    assert np.array_equal(_bits(y), _bits(x))
    for L in (1, 479, 481):
        y = W.embed(x[2000: 2000 + L], KEY, TAG, -18.0)
        assert len(y) == L and np.abs(y - x[2000: 2000 + L]).max() <= float(W.alpha_of(-18.0)) * np.abs(x[2000: 2000 + L]).max() * 1.001


@pytest.mark.parametrize("sizes", ([1], [479], [1920], "random"))
def test_chunked_embed_equals_one_shot(sizes):
    x = _signal("glide_noise")
    if sizes == [1]:
        x = x[28000:33000]  # (sample by sample: 5000 samples across the glide's end and the gap)
        want = W.embed(x, KEY, TAG)
    else:
        want = _marked("glide_noise")
    if sizes == "random":
        sizes = [int(v) for v in np.random.default_rng(5).integers(1, 6001, 37)]
    got, longest = W.embed_chunked(x, sizes, KEY, TAG)
    print(f"sizes {sizes[:4]}...: longest retained tail {longest}")
    assert np.array_equal(_bits(got), _bits(want))
    assert longest <= 1440


# ------------------------------------------------------------------------------------------ detector
@pytest.mark.parametrize("name", sorted(SIGNALS))
def test_detection_after_pcm16_crop_gain_and_noise(name):
    y = _marked(name)
    deg = W.degrade(y)
    cases = (("clean", y, 0), ("pcm16+crop+gain", deg, 5191), ("+noise -40 dB", W.add_noise(deg), 5191))
    for what, clip, offset in cases:
        r = W.detect(clip, KEY)
        print(f"{name} {what}: score {r.score:.1f} (sync {r.z_sync:.1f}, tag lane {r.z_tag:.1f}) tag {r.tag} offset {r.offset}")
        assert r.present
        assert r.tag == TAG
        assert r.offset == offset
        assert r.score >= 10.0


@pytest.mark.parametrize("name", sorted(SIGNALS))
def test_unmarked_and_wrong_key_are_not_present(name):
    un = W.detect(_signal(name), KEY)
    wk = W.detect(_marked(name), KEY ^ 1)
    print(f"{name}: unmarked max z {max(un.z_sync, un.z_tag):.2f}, key ^ 1 max z {max(wk.z_sync, wk.z_tag):.2f}")
    assert not un.present and not wk.present
    assert not W.detect(W.degrade(_signal(name)), KEY).present


def test_detector_edges_and_the_known_weak_case():
    assert W.detect(np.zeros(0, np.float32), KEY) == W.Result(False, 0.0, 0, 0, 0.0, 0.0)
    assert W.detect(np.zeros(30000, np.float32), KEY) == W.Result(False, 0.0, 0, 0, 0.0, 0.0)
    x = T.noise_with_silence(2.0, seed=1)  # a white-noise host: recorded, not asserted
    for db in (-30.0, -36.0):
        print(f"white noise host at {db} dB: score {W.detect(W.embed(x, KEY, TAG, db), KEY).score:.1f}")
    # every tag comes back from its rotation (clean clip, a few tags)
    base = _signal("harmonic220_1s")
    for tag in (0, 1, 128, 255):
        r = W.detect(W.embed(base, KEY, tag), KEY)
        assert r.present and r.tag == tag


# ------------------------------------------------------------------------------------------ interface
def test_watermark_validation():
    m = wm.Watermark(KEY, TAG)
    assert (m.key, m.tag, m.strength_db) == (KEY, TAG, -30.0)
    with pytest.raises(Exception):
        m.tag = 3  # frozen
    assert wm.Watermark(0).tag == 0 and wm.Watermark((1 << 64) - 1, 255, -18).strength_db == -18.0
    for bad in (dict(key=-1), dict(key=1 << 64), dict(key=1.5), dict(key="a"), dict(key=True), dict(key=1, tag=256), dict(key=1, tag=-1),
                dict(key=1, tag=2.0), dict(key=1, strength_db=-17.9), dict(key=1, strength_db=-48.1), dict(key=1, strength_db=float("nan")),
                dict(key=1, strength_db="loud")):
        with pytest.raises(ValueError):
            wm.Watermark(**bad)
    with pytest.raises(TypeError):
        wm.check_mark(KEY)
    with pytest.raises(TypeError):
        wm.per_row([m, 7], 2)
    with pytest.raises(ValueError):
        wm.per_row([m, None], 3)
    assert wm.per_row(m, 3) == [m, m, m] and wm.per_row(None, 2) == [None, None] and wm.per_row([m, None], 2) == [m, None]
    import sopro_amd

    assert sopro_amd.Watermark is wm.Watermark


def test_watermark_is_keyword_only_with_default_none_everywhere():
    from sopro_amd import longform, streaming
    from sopro_amd.serving import SynthesisService
    from sopro_amd.tts import SoproTTS

    fns = [SoproTTS.synthesize, SoproTTS.synthesize_batch, SoproTTS.synthesize_timed, SoproTTS.stream, SoproTTS.synthesize_long,
           SoproTTS.stream_long, streaming.SoproTTSStreamer.stream, streaming.stream, longform.synthesize_long, longform.stream_long,
           SynthesisService.submit, SynthesisService.submit_long,
           # out of scope, but never silently ignored
           SoproTTS.stream_batch, streaming.stream_batch, SynthesisService.submit_stream]
    for fn in fns:
        p = inspect.signature(fn).parameters.get("watermark")
        assert p is not None, f"{fn.__qualname__} has no watermark parameter"
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn.__qualname__
    assert callable(SoproTTS.detect_watermark)


def test_refusing_paths_raise_before_anything_runs():
    from sopro_amd import effects, streaming
    from sopro_amd.serving import SynthesisService
    from sopro_amd.tts import SoproTTS

    m = wm.Watermark(KEY, TAG)
    effects.refuse("x", watermark=None)
    with pytest.raises(NotImplementedError):
        effects.refuse("stream_batch", watermark=m)
    with pytest.raises(NotImplementedError):
        next(iter(streaming.stream_batch(None, ["a"], [None], watermark=m)))
    with pytest.raises(NotImplementedError):
        SoproTTS.stream_batch(object.__new__(SoproTTS), ["a"], [None], watermark=m)
    svc = object.__new__(SynthesisService)
    svc._closed, svc.engine = False, None
    with pytest.raises(NotImplementedError):
        svc.submit_stream("a", None, watermark=m)
    svc.engine = object()  # (continuous mode: refused before the engine is touched)
    with pytest.raises(NotImplementedError):
        svc.submit("a", None, watermark=m)
    with pytest.raises(TypeError):
        SoproTTS.synthesize(object.__new__(SoproTTS), "a", watermark=KEY)


def test_library_helpers_and_argument_checks():
    lib = hip.load()
    for name in ("sopro_wm_state_bytes", "sopro_wm_chunk_out_cap", "sopro_wm_fold_ws_bytes", "sopro_wm_embed_rows_f32", "sopro_wm_fold_rows_f32",
                 "sopro_wm_corr_rows_f32", "sopro_wm_peak_rows_f32"):
        assert name in hip.SYMBOLS
    assert lib.sopro_wm_state_bytes(0) == 0 and lib.sopro_wm_state_bytes(2) == 2 * lib.sopro_wm_state_bytes(1) >= 2 * (3 * 8 + 1536 * 4)
    for n in (0, 1, 1920, 11520):
        assert lib.sopro_wm_chunk_out_cap(n) >= n + 1440
    assert lib.sopro_wm_chunk_out_cap(-1) == -1
    assert lib.sopro_wm_fold_ws_bytes(3, 72000) >= 3 * 4 * (72000 // 480 + 2) and lib.sopro_wm_fold_ws_bytes(0, 10) == -1
    assert lib.sopro_wm_embed_rows_f32(None, 0, None, 0, None, None, 0, None, 1, None, 1, None, None, 0, 0, None, None) == -2
    assert b"non-NULL" in lib.sopro_last_error()
    assert lib.sopro_wm_corr_rows_f32(None, None, 1, None, 1, None, None) == -2
    assert lib.sopro_wm_peak_rows_f32(None, 1, None, None) == -2
    assert (hip.WM_HS, hip.WM_P, hip.WM_TAIL) == (480, 8192, 1536) and hip.WM_TILE % hip.WM_HS == 0 and hip.ABI_VERSION == 43
    assert hip.wm_calls() == 0  # nothing here launched anything
