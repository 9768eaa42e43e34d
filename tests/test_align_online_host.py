"""Streaming word timestamps without a device: the restatement of the online path operator (tests/align_online_ref.py) against the
offline one (tests/align_ref.py), its invariants on random ragged rows, ``StreamCues`` against ``word_cues``, and the argument
checks of ``sopro_align_online_f32`` / ``hip.align_online`` / ``SoproTTS.stream_timed`` that need no GPU.

Two things the online operator does NOT promise, measured here and printed (DESIGN.md "Word timestamps" quotes them): on flat or
random maps its path differs from the offline one in most rows, and a row whose text is nearly as long as its audio often ends with
status 2 (the best end it could see at some commit was too far left to finish the text afterwards)."""
import ctypes as C

import numpy as np
import pytest
import torch

import align_online_ref as O
import align_ref as R
from sopro_amd import align as A
from sopro_amd import hip

SCHEDULES = [(1, 0), (6, 8), (7, 3), (16, 20)]


def _log_uniform(rng, T, S):
    return np.log(rng.uniform(1e-4, 1.0, size=(T, S))).astype(np.float32)


def _ties(rng, T, S):
    return (-rng.integers(0, 2, size=(T, S))).astype(np.float32)  # small integers: exact in fp32, so equal totals are real ties


def _bits(v):
    return np.float32(v).tobytes()


# ------------------------------------------------------------------------------------------ the restatement's properties
@pytest.mark.parametrize("T,S", [(60, 40), (63, 63), (40, 1), (63, 7)])
@pytest.mark.parametrize("make", [_log_uniform, _ties])
def test_one_window_over_the_whole_row_is_the_offline_operator(T, S, make):
    sc = make(np.random.default_rng(T * 100 + S), T, S)
    want_path, _bounds, want_total, status = R.dp(sc)
    assert status == 0
    for chunk, lag in [(63, 63), (63, 0), (64, 100)]:  # one final step: the lag plays no part
        row = O.run(sc, chunk, lag)
        assert row.path == want_path and _bits(row.base) == _bits(want_total) and row.state() == (T - 1, S - 1, 0, S - 1)
    # the same row in steps of one frame at a lag that covers it: nothing is committed before the final step
    row = O.Online(S, 63)
    for t1 in range(1, T):
        assert row.step(sc, t1, False) == [] and row.c == -1
    row.step(sc, T, True)
    assert row.path == want_path and _bits(row.base) == _bits(want_total)


def _ragged_rows(n=200, seed=11):
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        T = int(rng.integers(1, 121))
        S = int(rng.integers(1, T + 6)) if i % 4 else int(rng.integers(max(1, T - 3), T + 1))  # every fourth row: S near T
        rows.append((_ties if i % 3 == 0 else _log_uniform)(rng, T, S))
    return rows


@pytest.mark.parametrize("chunk,lag", SCHEDULES)
def test_committed_prefixes_are_never_revised(chunk, lag):
    n_diff = n_st2 = n_cmp = 0
    for sc in _ragged_rows():
        T, S = sc.shape
        row = O.Online(S, lag)
        seen = []
        for t1, final in O.schedule(T, chunk, stream=True):
            c0, base0 = row.c, row.base
            new = row.step(sc, t1, final)
            assert row.path[: len(seen)] == seen and row.path[len(seen):] == new      # what was committed stays
            assert row.c == len(row.path) - 1 and (row.c == c0 or row.c >= c0 + 1)
            if not final:
                assert row.c <= max(t1 - 1 - lag, -1) and (new == [] or row.c == t1 - 1 - lag)
            if new == []:
                assert _bits(row.base) == _bits(base0)
            seen = list(row.path)
        path = row.path
        assert len(path) == T and path[0] == 0 and all(0 <= b - a <= 1 for a, b in zip(path, path[1:]))
        assert row.p == path[-1] and row.e == path[-1] and row.status in (0, 2)
        if not (lag == 0 and T % chunk == 0):  # (else the final step found every frame committed and did nothing: status is the last step's)
            assert (row.status == 0) == (path[-1] == S - 1)
        assert _bits(row.base) == _bits(R.path_total(sc, path))                        # the fold is the path's own total
        n_st2 += path[-1] != S - 1
        if T >= S:
            n_cmp += 1
            n_diff += path != R.dp(sc)[0]
        else:
            assert path[-1] < S - 1                                                      # (the offline operator spreads such a row)
        tf = A.path_token_frames(path, S)
        assert tf == O.token_frames(path, S)
        assert all(tf[s] == (T, T) for s in range(path[-1] + 1, S))
    print(f"chunk {chunk}, lag {lag}: path differs from the offline one in {n_diff} of {n_cmp} rows with T >= S; the text not finished (status 2) in {n_st2} of 200")
    assert n_diff > 0 and n_st2 > 0  # (both documented effects occur in this population)


@pytest.mark.parametrize("S", [40, 300])
def test_planted_alignments_are_recovered_at_every_schedule(S):
    rng = np.random.default_rng(300 + S)
    dur = rng.integers(1, 6, size=S)
    want = np.repeat(np.arange(S), dur)
    T = len(want)
    sc = np.full((T, S), -4.0, np.float32)
    sc[np.arange(T), want] = 0.0
    sc = (sc - rng.uniform(0.0, 0.99, size=(T, S))).astype(np.float32)  # on the path > -1, off it < -4
    for chunk, lag in SCHEDULES + [(6, 0), (16, 47)]:
        row = O.run(sc, chunk, lag)
        assert row.path == want.tolist() and row.status == 0, (chunk, lag)
        assert _bits(row.base) == _bits(R.path_total(sc, row.path))
    if T <= 63:
        assert R.dp(sc)[0] == want.tolist()


def test_windows_past_63_frames_are_outside_the_operator():
    sc = np.zeros((70, 3), np.float32)
    row = O.Online(3, 0)
    row.step(sc, 63, False)
    assert row.c == 62
    with pytest.raises(ValueError, match="64 frames"):
        O.Online(3, 0).step(sc, 64, False)
    with pytest.raises(ValueError, match="64 frames"):
        O.Online(3, 70).step(sc, 64, True)


# ------------------------------------------------------------------------------------------ StreamCues
TEXT = "  Hi, unbelievable world ! bye"
SPANS = [(0, 0),                       # BOS: empty span
         (2, 4), (4, 5),               # "Hi" ","
         (5, 8), (8, 14), (14, 18),    # " un" "believ" "able"
         (18, 19),                     # " ": a token of blanks only belongs to no word
         (19, 24),                     # "world"; "!" has no token
         (26, 30),                     # " bye"
         (30, 30)]                     # EOS


def _splits(rng, T):
    cuts = sorted(set(int(v) for v in rng.integers(0, T + 1, size=int(rng.integers(0, 6)))))
    return [0] + cuts + [T]


@pytest.mark.parametrize("reach", [len(SPANS) - 1, 7, 4, 0])
def test_stream_cues_concatenate_to_word_cues(reach):
    """``reach``: the last position the path gets to (below the last one: a status-2 tail)."""
    rng = np.random.default_rng(reach)
    for trial in range(20):
        dur = rng.integers(1, 5, size=reach + 1)
        path = np.repeat(np.arange(reach + 1), dur).tolist()
        T = len(path)
        want = A.word_cues(TEXT, SPANS, A.path_token_frames(path, len(SPANS)), hop=10)
        assert [c.text for c in want] == ["Hi,", "unbelievable", "world", "!", "bye"]
        edges = _splits(rng, T)
        sc = A.StreamCues(TEXT, SPANS, hop=10)
        got, per_step = [], []
        for a, b in zip(edges, edges[1:]):
            per_step.append(sc.feed(path[a:b]))
            got += per_step[-1]
            # a word is only reported once the committed position has passed its last token
            assert all(c.end_sample <= b * 10 for c in per_step[-1])
        got += sc.feed([], final=True)
        assert got == want, (reach, edges)
        with pytest.raises(ValueError):
            sc.feed([])
    if reach == 4:  # the tail: "unbelievable" ends with the audio, the words behind it are empty cues there
        assert [(c.start_sample, c.end_sample) for c in want[2:]] == [(T * 10, T * 10)] * 3 and want[1].end_sample == T * 10


def test_stream_cues_edge_cases():
    assert A.StreamCues("", [(0, 0)]).feed([0, 0], final=True) == []
    sc = A.StreamCues("a b", [(1, 2), (2, 3)], hop=10)  # "a" has no token: it is reported at once, at 0
    assert sc.feed([]) == [A.WordCue("a", 0, 1, 0, 0)]
    assert sc.feed([0, 0, 0, 1]) == [] and sc.feed([], final=True) == [A.WordCue("b", 2, 3, 30, 40)]
    with pytest.raises(ValueError, match="steps from"):
        A.StreamCues("a b", [(0, 1), (2, 3)]).feed([0, 2])
    with pytest.raises(ValueError, match="steps from"):
        A.StreamCues("a b", [(0, 1), (2, 3)]).feed([1])
    assert A.path_token_frames([], 3) == [(0, 0)] * 3
    chunk = A.TimedChunk(None, [], False)
    assert chunk.alignment is None and chunk._fields == ("wav", "words", "final", "alignment")


# ------------------------------------------------------------------------------------------ library, wrapper, public entry
def test_the_online_entry_is_there_and_checks_its_arguments():
    assert "sopro_align_online_f32" in hip.SYMBOLS and callable(hip.align_online) and isinstance(hip.align_calls, int)
    lib = hip.load()
    assert lib.sopro_abi_version() == hip.ABI_VERSION
    assert (hip.ALIGN_STATE_WORDS, hip.ALIGN_WINDOW_MAX, A.ONLINE_WINDOW_MAX) == (5, 63, 63)
    buf = (C.c_int32 * 64)()
    p = C.addressof(buf)  # (never dereferenced: every call below is refused before a launch)
    fn = lib.sopro_align_online_f32
    assert fn(None, 8, 0, None, None, None, 1, 8, 8, 0, None, None, 8, None) == -2 and b"non-NULL" in lib.sopro_last_error()
    for missing in range(6):
        ptrs = [p] * 6
        ptrs[missing] = None
        sc, t1, sl, fl, st, pa = ptrs
        assert fn(sc, 8, 0, t1, sl, fl, 1, 8, 8, 0, st, pa, 8, None) == -2 and b"non-NULL" in lib.sopro_last_error()
    assert fn(p, 8, 0, p, p, p, 1, 8, 8, -1, p, p, 8, None) == -2 and b"lag" in lib.sopro_last_error()
    assert fn(p, 4096, 0, p, p, p, 1, 8, 2049, 0, p, p, 8, None) == -2 and b"2048" in lib.sopro_last_error()
    assert fn(p, 7, 0, p, p, p, 1, 8, 8, 0, p, p, 8, None) == -2 and b"ld >= S_cap" in lib.sopro_last_error()
    assert fn(p, 8, 0, p, p, p, 1, 8, 8, 0, p, p, 7, None) == -2 and b"path_ld" in lib.sopro_last_error()
    assert fn(p, 8, 63, p, p, p, 2, 8, 8, 0, p, p, 8, None) == -2 and b"bstride" in lib.sopro_last_error()
    assert fn(p, 8, 0, p, p, p, 0, 8, 8, 0, p, p, 8, None) == -2
    calls = hip.align_calls
    cpu = torch.zeros(1, 4, 3)
    with pytest.raises(hip.SoproHipError, match="lag"):
        hip.align_online(cpu, [4], [3], [1], -1, torch.zeros(1, 5, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int32))
    with pytest.raises(hip.SoproHipError, match="not on a HIP device"):
        hip.align_online(cpu, [4], [3], [1], 0, torch.zeros(1, 5, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int32))
    assert hip.align_calls == calls
    st = hip.align_online_state(3, "cpu")
    assert st.dtype == torch.int32 and st.tolist() == [[-1, -1, 0, 0, 0]] * 3


def test_stream_timed_refuses_before_anything_runs():
    from sopro_amd import Silence, SoproTTS, TimedChunk

    assert TimedChunk is A.TimedChunk
    nobody = object()  # (no engine: whatever touched it would raise AttributeError)
    with pytest.raises(NotImplementedError, match="stream_timed has no silence control"):
        SoproTTS.stream_timed(nobody, "a b", silence=Silence())
    with pytest.raises(ValueError, match="lag_frames \\+ chunk_frames = 64"):
        SoproTTS.stream_timed(nobody, "a b", lag_frames=58, chunk_frames=6)
    with pytest.raises(ValueError, match="lag_frames \\+ chunk_frames = 64"):
        SoproTTS.stream_timed(nobody, "a b", lag_frames=0, chunk_frames=64)
    with pytest.raises(ValueError, match="lag_frames must be >= 0"):
        SoproTTS.stream_timed(nobody, "a b", lag_frames=-1)
    with pytest.raises(ValueError):
        SoproTTS.stream_timed(nobody, "a b", speed=9.0)
    A.check_align_window(57, 6)
    with pytest.raises(AttributeError):  # past the checks, the engine is needed
        SoproTTS.stream_timed(nobody, "a b", lag_frames=57, chunk_frames=6)
    # the refusals of the paths without timing now name the streaming entry too, and behave as before
    with pytest.raises(NotImplementedError, match="no word timing.*stream_timed\\(\\)"):
        A.refuse_timing({"word_cues": True}, "stream_batch")
