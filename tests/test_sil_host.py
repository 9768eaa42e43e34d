"""Silence control on the CPU: the numpy restatement (tests/sil_ref.py) against hand-computed cases at every boundary of the
definition, its chunked model against its one-shot form, the cue map, ``Silence`` validation, the refusing paths and the argument
checks of the C entry points.  The device side is tests/test_gpu_sil.py."""
import inspect

import numpy as np
import pytest

import sil_ref as R
from sopro_amd import align as A
from sopro_amd import hip
from sopro_amd import silence as S

HOP = R.HOP
THR = np.float32(0.5)
TAB = R.TAB


def _sig(pattern, tail=0, tail_active=False):
    """Hops from a string: 'S' an active hop (0.75 at one sample of it), 'g' an inactive one; every sample is distinct, so a result
    says where each of its samples came from.  ``tail`` more samples form a partial last hop."""
    n = len(pattern) * HOP + tail
    x = (np.arange(n, dtype=np.float64) * 1e-6 + 1e-3).astype(np.float32)
    for j, c in enumerate(pattern):
        if c == "S":
            x[j * HOP + (7 * j) % HOP] = -0.75 if j % 2 else 0.75
    if tail and tail_active:
        x[len(pattern) * HOP + tail - 1] = 0.75
    return x


def _hop(x, j):
    return x[j * HOP: (j + 1) * HOP]


def _fin(h):
    return h * TAB


def _fout(h):
    return h * TAB[::-1]


def _check(x, cap_h, b, want, cuts):
    y, c = R.squeeze(x, THR, cap_h, b)
    want = np.concatenate(want).astype(np.float32) if want else np.zeros(0, np.float32)
    assert c == cuts
    assert y.dtype == np.float32 and len(y) == len(want) and np.array_equal(y.view(np.int32), want.view(np.int32))
    assert len(y) == len(x) - sum(n for _p, n in c)


# ------------------------------------------------------------------------------------------ the definition, by hand (cap_h 4, b 2, a 2)
def test_leading_run_at_its_boundary():
    x = _sig("gggS")                      # n = b + 1: unchanged
    _check(x, 4, 2, [x], [])
    x = _sig("ggggSS")                    # n = b + 2: hop 0 goes, hop 1 fades in, hops 2 and 3 stay whole
    _check(x, 4, 2, [_fin(_hop(x, 1)), x[2 * HOP:]], [(0, HOP)])
    x = _sig("g" * 9 + "S")               # a long one: hops 0 .. 5 go, hop 6 fades in
    _check(x, 4, 2, [_fin(_hop(x, 6)), x[7 * HOP:]], [(0, 6 * HOP)])


def test_interior_run_at_its_boundary():
    x = _sig("SggggS")                    # n = cap_h: unchanged
    _check(x, 4, 2, [x], [])
    x = _sig("SgggggS")                   # n = cap_h + 1: j0 1, j1 6, p 3, q 4: hop 1 stays, hop 2 crossfades into hop 3, hops 4, 5 stay
    cross = _fout(_hop(x, 2)) + _fin(_hop(x, 3))
    _check(x, 4, 2, [x[: 2 * HOP], cross, x[4 * HOP:]], [(3 * HOP, HOP)])
    x = _sig("SS" + "g" * 11 + "S")       # j0 2, j1 13, p 4, q 11: hop 3 crossfades into hop 10
    cross = _fout(_hop(x, 3)) + _fin(_hop(x, 10))
    _check(x, 4, 2, [x[: 3 * HOP], cross, x[11 * HOP:]], [(4 * HOP, 7 * HOP)])
    y, _c = R.squeeze(x, THR, 4, 2)
    assert len(y) == (2 + 4 + 1) * HOP    # the run is exactly cap_h hops long


def test_trailing_run_at_its_boundary():
    x = _sig("Sgg")                       # n = a: unchanged
    _check(x, 4, 2, [x], [])
    x = _sig("Sggg")                      # n = a + 1: hop 1 stays, hop 2 fades out, hop 3 goes
    _check(x, 4, 2, [x[: 2 * HOP], _fout(_hop(x, 2))], [(3 * HOP, HOP)])
    x = _sig("Sg", tail=10)               # an inactive partial last hop counts: n = 2 = a, unchanged, the partial hop included
    _check(x, 4, 2, [x], [])
    x = _sig("Sgg", tail=10)              # n = 3: hop 2 fades out, hop 3's ten samples go
    _check(x, 4, 2, [x[: 2 * HOP], _fout(_hop(x, 2))], [(3 * HOP, 10)])
    x = _sig("Sggggg", tail=10, tail_active=True)  # an active partial last hop ends an interior run and is copied
    cross = _fout(_hop(x, 2)) + _fin(_hop(x, 3))
    _check(x, 4, 2, [x[: 2 * HOP], cross, x[4 * HOP:]], [(3 * HOP, HOP)])


def test_a_equal_to_one():
    x = _sig("SggggS")                    # cap_h 3, b 2: j0 1, j1 5, p 2, q 3: no whole hop stays in front, hop 1 crossfades into hop 2
    cross = _fout(_hop(x, 1)) + _fin(_hop(x, 2))
    _check(x, 3, 2, [x[:HOP], cross, x[3 * HOP:]], [(2 * HOP, HOP)])
    x = _sig("SgggS")                     # n = cap_h: unchanged
    _check(x, 3, 2, [x], [])
    x = _sig("Sgg")                       # trailing n = 2 > a: hop 1 fades out
    _check(x, 3, 2, [x[:HOP], _fout(_hop(x, 1))], [(2 * HOP, HOP)])
    x = _sig("Sg")                        # trailing n = a
    _check(x, 3, 2, [x], [])


def test_rows_without_sound_short_rows_the_floor_itself_and_nan():
    x = _sig("ggggg", tail=30)
    _check(x, 4, 2, [], [(0, len(x))])    # no active hop: empty
    _check(np.zeros(0, np.float32), 4, 2, [], [])
    x = _sig("", tail=100)
    _check(x, 4, 2, [], [(0, 100)])       # L < HOP, silent
    x = _sig("", tail=100, tail_active=True)
    _check(x, 4, 2, [x], [])              # L < HOP, active
    x = _sig("Sgg")
    _check(x, 0, 1, [x], [])              # cap_h == 0: the identity
    x = _sig("gggggS")
    x[2 * HOP + 5] = -THR                 # |x| == thr exactly: active, so the leading run is hops 0, 1 only
    _check(x, 4, 2, [x], [])
    x[2 * HOP + 5] = np.nextafter(THR, np.float32(0))
    _check(x, 4, 2, [_fin(_hop(x, 2)), x[3 * HOP:]], [(0, 2 * HOP)])
    x[2 * HOP + 5] = np.nan               # a NaN compares false: the hop stays inactive, the NaN is copied (and faded) like any sample
    y, c = R.squeeze(x, THR, 4, 2)
    assert c == [(0, 2 * HOP)] and len(y) == 4 * HOP and np.isnan(y[5]) and int(np.isnan(y).sum()) == 1


# ------------------------------------------------------------------------------------------ the two forms
def _random_signal(rng):
    L = int(rng.integers(0, 12000))
    x = np.zeros(L, np.float32)
    at, on = 0, bool(rng.integers(2))
    while at < L:
        n = int(rng.integers(1, 2500))
        x[at: at + n] = (rng.standard_normal(min(n, L - at)) * (1.0 if on else 0.001)).astype(np.float32)
        at += n
        on = not on
    return x


def test_chunked_model_equals_one_shot_on_random_signals_and_chunkings():
    rng = np.random.default_rng(0)
    kinds = set()
    for t in range(150):
        b = int(rng.integers(1, 5))
        cap_h = int(rng.integers(b + 1, b + 6))
        x = _random_signal(rng)
        y, c = R.squeeze(x, 0.05, cap_h, b)
        assert len(y) == len(x) - sum(n for _p, n in c)
        assert all(p % HOP == 0 for p, _n in c) and all(c[k][0] + c[k][1] < c[k + 1][0] for k in range(len(c) - 1))
        kinds |= {"lead" if p == 0 else ("trail" if p + n == len(x) else "mid") for p, n in c}
        sizes = [1] if (t % 50 == 0 and len(x) < 3000) else rng.integers(1, 3000, size=7).tolist()
        y2, c2 = R.stream_all(x, sizes, 0.05, cap_h, b)
        assert c2 == c and np.array_equal(y2.view(np.int32), y.view(np.int32)), t
    assert kinds == {"lead", "mid", "trail"}
    # a stream after its flush is a fresh stream; the identity passes chunks through
    st = R.Stream(0.05, 4, 2)
    x = _random_signal(rng)
    for _ in range(2):
        got = [st.feed(x[:1000])[0], st.feed(x[1000:])[0], st.flush()[0]]
        assert np.array_equal(np.concatenate(got), R.squeeze(x, 0.05, 4, 2)[0])
    assert np.array_equal(R.Stream(0.05, 0, 1).feed(x)[0], x)


def test_the_designed_batch_holds_what_the_device_test_needs():
    rows = R.designed_batch(hip.SIL_PLAN_WORDS * 64)
    assert len(rows) == 8 and len(rows[4][0]) > hip.SIL_PLAN_WORDS * 64 * HOP
    x, thr, cap_h, b = rows[3]
    assert int(np.isnan(x).sum()) == 1 and int((np.abs(x) == thr).sum()) == 1
    y, cuts = R.squeeze(x, thr, cap_h, b)
    assert [n for _p, n in cuts] == [6 * HOP, 4 * HOP]  # the sample at the floor splits the 31-hop gap, the NaN does not split the 34-hop one
    y2, c2 = R.stream_all(x, [4999, 1, 239, 241], thr, cap_h, b)
    assert c2 == cuts and np.array_equal(y2.view(np.int32), y.view(np.int32))


# ------------------------------------------------------------------------------------------ cues
def test_map_cuts_and_squeeze_cues():
    cuts = [(0, 480), (2400, 720), (7200, 100)]
    want = {0: 0, 100: 0, 479: 0, 480: 0, 481: 1, 2399: 1919, 2400: 1920, 2401: 1920, 3119: 1920, 3120: 1920, 3121: 1921,
            7200: 6000, 7250: 6000, 7300: 6000}
    for s, m in want.items():
        assert A.map_cuts(s, cuts) == m == R.map_cuts(s, cuts), s
    assert A.map_cuts(5, []) == 5
    prev = -1
    for s in range(0, 7301, 7):  # monotone, and exact outside the cuts
        m = A.map_cuts(s, cuts)
        assert m >= prev and m == R.map_cuts(s, cuts)
        prev = m
    cues = [A.WordCue("a", 0, 1, 100, 2500), A.WordCue("b", 2, 3, 2500, 7300)]
    got = A.squeeze_cues(cues, cuts)
    assert got == [A.WordCue("a", 0, 1, 0, 1920), A.WordCue("b", 2, 3, 1920, 6000)] == R.squeeze_cues(cues, cuts)
    # the map of a real result: every kept stretch keeps its samples
    x = _sig("ggggSSgggggggSgggg", tail=5)
    y, c = R.squeeze(x, THR, 4, 2)
    for s in (4 * HOP, 5 * HOP + 17, 13 * HOP + 3):
        assert y[A.map_cuts(s, c)] == x[s]
    assert A.map_cuts(len(x), c) == len(y)


# ------------------------------------------------------------------------------------------ interface
def test_silence_validation():
    s = S.Silence()
    assert (s.max_pause_ms, s.onset_ms, s.floor_db, s.floor) == (300.0, 30.0, -40.0, None)
    assert (s.cap_hops, s.onset_hops) == (30, 3) and s.thr == float(np.float32(10.0 ** (-40.0 / 20.0))) == float(np.float32(0.01))
    with pytest.raises(Exception):
        s.onset_ms = 3  # frozen
    assert S.Silence(floor=0.25, floor_db=-90.0).thr == 0.25                 # floor overrides floor_db
    assert S.Silence(floor=0.1).thr == float(np.float32(0.1))
    assert S.Silence(max_pause_ms=20, onset_ms=10).cap_hops == 2 and S.Silence(max_pause_ms=10000, onset_ms=160).onset_hops == 16
    assert S.Silence(max_pause_ms=44, onset_ms=26).cap_hops == 4 and S.Silence(max_pause_ms=44, onset_ms=26).onset_hops == 3
    for bad in (dict(onset_ms=0), dict(onset_ms=4), dict(onset_ms=170), dict(max_pause_ms=30, onset_ms=30), dict(max_pause_ms=10010),
                dict(max_pause_ms=-5), dict(max_pause_ms=float("nan")), dict(onset_ms=float("inf")), dict(floor_db=float("nan")),
                dict(floor=0.0), dict(floor=-0.1), dict(floor=float("inf")), dict(floor=1e-60), dict(floor_db=-2000.0), dict(floor_db=9000.0),
                dict(floor="low"), dict(max_pause_ms="long"), dict(onset_ms=True)):
        with pytest.raises(ValueError):
            S.Silence(**bad)
    with pytest.raises(TypeError):
        S.check_silence(0.01)
    with pytest.raises(TypeError):
        S.per_row([s, 7], 2)
    with pytest.raises(ValueError):
        S.per_row([s, None], 3)
    assert S.per_row(s, 3) == [s, s, s] and S.per_row(None, 2) == [None, None] and S.per_row([s, None], 2) == [s, None]
    import sopro_amd

    assert sopro_amd.Silence is S.Silence and "Silence" in sopro_amd.__all__


def test_silence_is_keyword_only_with_default_none_everywhere():
    from sopro_amd import longform, streaming
    from sopro_amd.serving import SynthesisService
    from sopro_amd.tts import PaddedBatch, SoproTTS

    fns = [SoproTTS.synthesize, SoproTTS.synthesize_batch, SoproTTS.synthesize_timed, SoproTTS.stream, SoproTTS.synthesize_long,
           SoproTTS.stream_long, streaming.SoproTTSStreamer.stream, streaming.stream, longform.synthesize_long, longform.stream_long,
           SynthesisService.submit, SynthesisService.submit_long,
           # out of scope, but never silently ignored
           SoproTTS.stream_batch, streaming.stream_batch, SynthesisService.submit_stream]
    for fn in fns:
        p = inspect.signature(fn).parameters.get("silence")
        assert p is not None, f"{fn.__qualname__} has no silence parameter"
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn.__qualname__
    assert PaddedBatch._fields == ("wav", "lens", "tokens", "frames", "cuts") and PaddedBatch(1, 2, 3).cuts is None


def test_refusing_paths_raise_before_anything_runs():
    from sopro_amd import effects, streaming
    from sopro_amd.serving import SynthesisService
    from sopro_amd.tts import SoproTTS

    s = S.Silence()
    effects.refuse("x", silence=None)
    with pytest.raises(NotImplementedError):
        effects.refuse("stream_batch", silence=s)
    with pytest.raises(NotImplementedError):
        next(iter(streaming.stream_batch(None, ["a"], [None], silence=s)))
    with pytest.raises(NotImplementedError):
        SoproTTS.stream_batch(object.__new__(SoproTTS), ["a"], [None], silence=s)
    svc = object.__new__(SynthesisService)
    svc._closed, svc.engine = False, None
    with pytest.raises(NotImplementedError):
        svc.submit_stream("a", None, silence=s)
    svc.engine = object()  # (continuous mode: refused before the engine is touched)
    with pytest.raises(NotImplementedError):
        svc.submit("a", None, silence=s)
    with pytest.raises(TypeError):
        SoproTTS.synthesize(object.__new__(SoproTTS), "a", silence=0.01)
    with pytest.raises(TypeError):
        SoproTTS.stream_long(object.__new__(SoproTTS), "a", silence="quiet")
    with pytest.raises(TypeError):
        svc.submit_long("a", None, silence=3)


def test_library_helpers_and_argument_checks():
    lib = hip.load()
    calls = hip.sil_calls
    for name in ("sopro_sil_state_bytes", "sopro_sil_chunk_out_cap", "sopro_sil_ws_bytes", "sopro_sil_rows_f32"):
        assert name in hip.SYMBOLS
    assert (hip.SIL_HOP, hip.SIL_TAIL, hip.SIL_TILE, hip.SIL_PLAN_WORDS) == (240, 4608, 2048, 64) and hip.ABI_VERSION == 43
    assert hip.SIL_TAIL >= 18 * 240 + 239                                # the held hop, a ring of b + 1 <= 17, the incomplete hop
    assert lib.sopro_sil_state_bytes(0) == 0 and lib.sopro_sil_state_bytes(2) == 2 * lib.sopro_sil_state_bytes(1) >= 2 * (6 * 8 + 4608 * 4)
    for n in (0, 1, 1920, 11520):
        assert lib.sopro_sil_chunk_out_cap(n) == n + hip.SIL_TAIL
    assert lib.sopro_sil_chunk_out_cap(-1) == -1
    assert lib.sopro_sil_ws_bytes(0, 10) == -1 and lib.sopro_sil_ws_bytes(1, -1) == -1
    one, many = lib.sopro_sil_ws_bytes(1, 384000), lib.sopro_sil_ws_bytes(32, 384000)
    assert many == 32 * one and one % 8 == 0 and one >= 8 * (1600 // 64 + 1) and lib.sopro_sil_ws_bytes(1, 0) > 0
    assert lib.sopro_sil_rows_f32(None, 0, None, 0, None, None, None, 1, None, 1, None, None, None, 0, 0, None, None, 0, None, None) == -2
    assert b"non-NULL" in lib.sopro_last_error()
    import ctypes as C

    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    args = lambda **k: [k.get("inp", None), 0, p, k.get("in_cap", 0), p, p, p, k.get("rows", 1), k.get("state", None), k.get("flush", 1), p, p,  # noqa: E731
                        k.get("out", None), 0, k.get("out_cap", 0), p, k.get("cuts", None), k.get("cuts_cap", 0), p, None]
    for bad, msg in ((dict(rows=0), b"rows"), (dict(rows=70000), b"rows"), (dict(in_cap=5), b"in must be non-NULL"), (dict(in_cap=-1), b"in_cap"),
                     (dict(in_cap=(1 << 30) + 1, inp=p), b"in_cap"), (dict(out_cap=8), b"out must be non-NULL"), (dict(cuts_cap=4), b"cuts must be non-NULL"),
                     (dict(flush=0), b"flush must be set"), (dict(state=p + 4), b"8-byte aligned"), (dict(out=p + 2, out_cap=1), b"4-byte aligned")):
        assert lib.sopro_sil_rows_f32(*args(**bad)) == -2, bad
        assert msg in lib.sopro_last_error(), (bad, lib.sopro_last_error())
    assert hip.sil_calls == calls  # nothing here launched anything
    with pytest.raises(ValueError):
        hip.SilenceState(0, None, "cuda:0")
