"""Word timestamps, host side: from a frame-to-token path (``replay.align_batch`` / ``replay.AlignStream``) to word cues in samples.

Pure Python, importable without a device.  The device half (attention maps of the AR generator's text cross-attention, the best
monotonic path through them) is ``sopro_amd/replay.py``, defined in DESIGN.md "Word timestamps" and include/sopro_hip.h.

    Alignment   what the engine knows about one utterance, in frames
    token_spans character range of every token id ``encode_text`` returns (BOS / EOS: empty)
    word_cues   tokens -> words -> sample ranges
    StreamCues  the same for a path that arrives in committed pieces (``SoproTTS.stream_timed`` -> ``TimedChunk``)
    map_speed   a sample position before the speaking-rate stretch -> after it
    map_pitch   a sample position before the pitch resampler -> after it
"""
from __future__ import annotations

import bisect
import math
from dataclasses import dataclass, field
from typing import Any, List, NamedTuple, Optional, Sequence, Tuple

HOP = 1920                      # samples per codec frame (24 kHz / 12.5 frames per second)
TSM_HS, TSM_R = 480, 240        # the stretch's output hop and search radius (hip.TSM_HS / hip.TSM_R; kept here so that this module
                                # imports without the kernel library)


@dataclass
class Alignment:
    """One utterance's alignment, in frames, before any stretch.  ``path[t]``: the text position frame t belongs to;
    ``token_frames[s]``: (first frame, last frame + 1) of text position s; ``total``: the path's log score; ``confidence`` =
    exp(total / T), the geometric mean of the mean attention probability along the path (1 / S for flat maps); ``status`` 0: the
    path is the best monotonic one, 1: no monotonic path exists (fewer frames than text positions, or none) and the frames were
    spread evenly, 2 (``stream_timed`` only): the online path ended before the last text position - the positions above
    ``path[-1]`` have the empty range (T, T); ``total`` is then the score of the path as committed."""

    path: List[int]
    token_frames: List[Tuple[int, int]]
    total: float
    confidence: float = field(default=-1.0)
    status: int = 0

    def __post_init__(self):
        if self.confidence < 0.0:
            n = len(self.path)
            self.confidence = math.exp(self.total / n) if (n > 0 and self.status == 0) else 0.0


class WordCue(NamedTuple):
    text: str
    char_start: int
    char_end: int
    start_sample: int
    end_sample: int


class LongWordCue(NamedTuple):
    """A word of ``synthesize_long``: character offsets are relative to segment ``segment``'s text, samples to the joined waveform."""
    text: str
    char_start: int
    char_end: int
    start_sample: int
    end_sample: int
    segment: int


class TimedResult(NamedTuple):
    wav: Any                    # [1, 1, N] on the device, what ``synthesize`` returns for the same seed
    words: List[WordCue]
    alignment: Alignment


def token_spans(tokenizer: Any, text: str) -> List[Tuple[int, int]]:
    """Character span (start, end) in ``text`` of every id ``tokenizer.encode(text)`` returns.  Sources, in this order: the
    tokenizer's own ``encode_with_offsets(text) -> (ids, spans)``; a Hugging Face fast tokenizer under ``tokenizer.tok``
    (``offset_mapping``; the BOS / EOS ids the wrapper adds get empty spans).  A tokenizer offering neither cannot be timed
    automatically: pass ``token_spans=`` to the timed entry point."""
    fn = getattr(tokenizer, "encode_with_offsets", None)
    if fn is not None:
        _ids, spans = fn(text)
        return [(int(a), int(b)) for a, b in spans]
    tok = getattr(tokenizer, "tok", None)
    if tok is not None and getattr(tok, "is_fast", False):
        enc = tok(text, add_special_tokens=False, return_offsets_mapping=True)
        spans = [(int(a), int(b)) for a, b in enc["offset_mapping"]]
        if getattr(tokenizer, "bos_id", None) is not None and getattr(tokenizer, "eos_id", None) is not None:
            spans = [(0, 0)] + spans + [(len(text), len(text))]
        return spans
    raise TypeError("this tokenizer gives no character offsets (no encode_with_offsets, no fast Hugging Face tokenizer): "
                    "pass token_spans=[(start, end), ...], one span per id of encode_text(text)")


def words_of(text: str) -> List[Tuple[int, int]]:
    """Maximal runs of non-whitespace characters as (start, end)."""
    out, start = [], None
    for i, ch in enumerate(text):
        if ch.isspace():
            if start is not None:
                out.append((start, i))
                start = None
        elif start is None:
            start = i
    if start is not None:
        out.append((start, len(text)))
    return out


def word_cues(text: str, spans: Sequence[Tuple[int, int]], token_frames: Sequence[Tuple[int, int]], hop: int = HOP) -> List[WordCue]:
    """One cue per word of ``text``.  A token belongs to the word that contains the first non-blank character of its span; tokens
    with empty (or all-blank) spans belong to no word - their frames are leading / trailing silence.  A word runs from the first
    frame of its first token to the end frame of its last token, times ``hop``; a word with no token gets a zero-length cue at the
    previous word's end (0 for the first word)."""
    if len(spans) != len(token_frames):
        raise ValueError(f"one span per token: {len(spans)} spans, {len(token_frames)} tokens")
    words = words_of(text)
    first: List[Optional[int]] = [None] * len(words)
    last: List[Optional[int]] = [None] * len(words)
    starts = [a for a, _b in words]
    for s in range(len(spans)):
        a, b = int(spans[s][0]), min(int(spans[s][1]), len(text))
        c = max(a, 0)
        while c < b and text[c].isspace():
            c += 1
        if c >= b:
            continue
        wi = bisect.bisect_right(starts, c) - 1  # (c is not blank, so it lies inside the word that starts at or before it)
        if first[wi] is None:
            first[wi] = s
        last[wi] = s
    cues: List[WordCue] = []
    prev_end = 0
    for k, (a, b) in enumerate(words):
        if first[k] is None:
            st = en = prev_end
        else:
            st, en = int(token_frames[first[k]][0]) * hop, int(token_frames[last[k]][1]) * hop
        cues.append(WordCue(text[a:b], a, b, st, en))
        prev_end = en
    return cues


class TimedChunk(NamedTuple):
    """One item of ``SoproTTS.stream_timed``: ``wav`` [1, n] on the device (n may be 0), the ``WordCue`` of every word this step
    closed (samples on the timeline of the concatenated ``wav`` fields), and on the last item ``final=True`` with the utterance's
    ``Alignment``."""
    wav: Any
    words: List[WordCue]
    final: bool
    alignment: Optional[Alignment] = None


ONLINE_WINDOW_MAX = 63          # frames one step of the online aligner can walk (hip.ALIGN_WINDOW_MAX; kept here like TSM_HS)


def check_align_window(lag_frames: int, chunk_frames: int) -> None:
    """A stream that steps by ``chunk_frames`` at lag ``lag_frames`` hands the online aligner windows of up to their sum."""
    lag, cf = int(lag_frames), int(chunk_frames)
    if lag < 0 or cf < 1:
        raise ValueError(f"lag_frames must be >= 0 and chunk_frames >= 1, got {lag} and {cf}")
    if lag + cf > ONLINE_WINDOW_MAX:
        raise ValueError(f"lag_frames + chunk_frames = {lag + cf}: the online aligner walks at most {ONLINE_WINDOW_MAX} uncommitted "
                         "frames per step")


def path_token_frames(path: Sequence[int], n_tokens: int) -> List[Tuple[int, int]]:
    """(first frame, last frame + 1) per text position of a monotone frame-to-position path (steps of 0 or +1 from position 0);
    positions the path never reached (an online alignment that ended with status 2) get the empty range (T, T)."""
    T = len(path)
    out: List[Tuple[int, int]] = [(T, T)] * int(n_tokens)
    t = 0
    while t < T:
        s, a = int(path[t]), t
        while t < T and int(path[t]) == s:
            t += 1
        if 0 <= s < n_tokens:
            out[s] = (a, t)
    return out


def _word_tokens(text: str, spans: Sequence[Tuple[int, int]]):
    """(words, first token, last token) by the membership rule of ``word_cues``."""
    words = words_of(text)
    first: List[Optional[int]] = [None] * len(words)
    last: List[Optional[int]] = [None] * len(words)
    starts = [a for a, _b in words]
    for s in range(len(spans)):
        a, b = int(spans[s][0]), min(int(spans[s][1]), len(text))
        c = max(a, 0)
        while c < b and text[c].isspace():
            c += 1
        if c >= b:
            continue
        wi = bisect.bisect_right(starts, c) - 1
        if first[wi] is None:
            first[wi] = s
        last[wi] = s
    return words, first, last


class StreamCues:
    """``word_cues`` for a path that arrives in committed pieces (``hip.align_online`` never revises what it committed).  ``feed``
    takes the next slice of the path and returns the cues of the words it closed, in text order: a token closes when the committed
    position passes it, or at the final step; a word closes with its last token; a word without tokens follows the word before it
    at once, as a zero-length cue.  After the final step the concatenated cues equal ``word_cues(text, spans,
    path_token_frames(whole path, len(spans)))``."""

    def __init__(self, text: str, spans: Sequence[Tuple[int, int]], hop: int = HOP):
        self.text, self.hop = text, int(hop)
        self.n_tokens = len(spans)
        self.words, self.first, self.last = _word_tokens(text, spans)
        self.frames: List[Optional[Tuple[int, int]]] = [None] * self.n_tokens  # closed tokens only
        self.T = 0            # committed frames
        self.pos = -1         # position of the last committed frame
        self.start = 0        # first frame of position ``pos``
        self.closed = 0       # tokens [0, closed) are closed
        self.next_word = 0
        self.prev_end = 0
        self.done = False

    def feed(self, path_slice: Sequence[int], final: bool = False) -> List[WordCue]:
        if self.done:
            raise ValueError("StreamCues: fed after the final step")
        for v in path_slice:
            s = int(v)
            if s != self.pos:
                if not (s == self.pos + 1 and 0 <= s < self.n_tokens):
                    raise ValueError(f"StreamCues: frame {self.T} steps from position {self.pos} to {s}")
                if self.pos >= 0:
                    self.frames[self.pos] = (self.start, self.T)
                self.pos, self.start = s, self.T
                self.closed = s
            self.T += 1
        if final:
            if self.pos >= 0:
                self.frames[self.pos] = (self.start, self.T)
            for s in range(self.pos + 1, self.n_tokens):
                self.frames[s] = (self.T, self.T)
            self.closed = self.n_tokens
            self.done = True
        out: List[WordCue] = []
        while self.next_word < len(self.words):
            k = self.next_word
            a, b = self.words[k]
            if self.first[k] is None:
                st = en = self.prev_end
            elif self.last[k] < self.closed:
                st, en = self.frames[self.first[k]][0] * self.hop, self.frames[self.last[k]][1] * self.hop
            else:
                break
            out.append(WordCue(self.text[a:b], a, b, st, en))
            self.prev_end = en
            self.next_word += 1
        return out


def map_speed(sample: int, step: int) -> int:
    """A sample position of the unstretched waveform -> its position after ``hip.time_stretch`` at ``step = hip.tsm_step(speed)``:
    (sample * HS * 65536) // step, the arithmetic of ``hip.tsm_out_len``.  Exact for the waveform's length; inside it the stretch
    places every 480-sample block within its search radius of the nominal position, so a cue is accurate to +-240 samples
    (``TSM_R``, 10 ms) by the operator's definition."""
    return (int(sample) * TSM_HS * 65536) // int(step)


def stretch_cues(cues: Sequence[WordCue], step: int) -> List[WordCue]:
    return [c._replace(start_sample=map_speed(c.start_sample, step), end_sample=map_speed(c.end_sample, step)) for c in cues]


def map_pitch(sample: int, inc: int) -> int:
    """A sample position before the pitch resampler -> after ``hip.pitch_shift`` at ``inc = hip.pitch_inc(semitones)``:
    (sample << 32) // inc, the arithmetic of ``hip.pitch_out_len``.  The resampler's filter is symmetric about the read position
    n * inc / 2^32 of output n (no delay), so the map is exact up to the floor: less than one sample."""
    return (int(sample) << 32) // int(inc)


def shift_cues(cues: Sequence[WordCue], inc: int) -> List[WordCue]:
    """Cues of the waveform that went into the pitch resampler -> cues of what came out.  After ``stretch_cues(cues, step')`` (the
    public ``pitch=``: stretch, then resample) a cue keeps the stretch's accuracy, +-240 samples of the stretched waveform, which the
    resampler divides by rho = inc / 2^32 like every other distance: +-240 / rho samples (+-10 ms / rho; at most +-480 samples at -12
    semitones), plus the floor's one sample."""
    return [c._replace(start_sample=map_pitch(c.start_sample, inc), end_sample=map_pitch(c.end_sample, inc)) for c in cues]


def map_cuts(sample: int, cuts: Sequence[Tuple[int, int]]) -> int:
    """A sample position before the silence operator -> after it, by the operator's own cut table (``hip.silence_squeeze``: (source
    position, samples removed) in order).  Exact: a position at or past the end of a removed range moves up by what was removed
    before it, a position inside a removed range maps to the cut's start."""
    s, off = int(sample), 0
    for pos, n in cuts:
        if s >= pos + n:
            off += n
        elif s > pos:
            return int(pos) - off
        else:
            break
    return s - off


def squeeze_cues(cues: Sequence[WordCue], cuts: Sequence[Tuple[int, int]]) -> List[WordCue]:
    """Cues of the waveform that went into the silence operator -> cues of what came out (after ``stretch_cues`` / ``shift_cues``:
    the operator runs last before the watermark)."""
    return [c._replace(start_sample=map_cuts(c.start_sample, cuts), end_sample=map_cuts(c.end_sample, cuts)) for c in cues]


def long_cue(cue: WordCue, segment: int, off: int, edge_start: int, edge_end: int) -> LongWordCue:
    """A segment's cue in the joined waveform: ``off + (sample - edge_start)``, the sample clamped to the kept range
    [edge_start, edge_end] of the segment first (what the join trimmed away holds no word)."""
    def m(v: int) -> int:
        return int(off) + (min(max(int(v), int(edge_start)), int(edge_end)) - int(edge_start))

    return LongWordCue(cue.text, cue.char_start, cue.char_end, m(cue.start_sample), m(cue.end_sample), int(segment))


TIMING_KEYWORDS = ("alignment", "align_heads", "word_cues", "token_spans")


def refuse_timing(kwargs, what: str) -> None:
    """The streaming and serving paths have no word timing: a timing keyword there is an error, never ignored; timing
    keywords that pass (None / False) are dropped from ``kwargs``."""
    asked = [k for k in TIMING_KEYWORDS if kwargs.get(k) not in (None, False)]
    if asked:
        raise NotImplementedError(f"{what} has no word timing ({', '.join(asked)}): use stream_timed(), synthesize_timed(), "
                                  "synthesize_batch(alignment=[...]) or synthesize_long(word_cues=True)")
    for k in TIMING_KEYWORDS:
        kwargs.pop(k, None)
