"""Long-form synthesis: split a text into utterance-sized segments, synthesise them as the rows of ordinary batches, and join the
rows on the device into one waveform.

The model speaks one utterance of at most ~32 s (400 frames; the reference says so in its README) and every entry point
inherits that limit.  The sentences of one text are independent utterances with the same voice - the shape ``synthesize_batch``
was built for - so a paragraph, an article or a chapter costs about one batched pass per ``max_rows`` sentences.  What lies
between the decoder's padded batch and one continuous waveform (finding where each row's speech starts and ends, laying the
kept parts end to end with pauses, fading the cuts) is ``hip.join_segments`` (csrc/join.hip; contract in include/sopro_hip.h).
No reference counterpart.

Host side, pure Python (importable without a device): ``split_text``, ``pause_samples``, ``group_plan``.
Engine side: ``synthesize_long`` / ``stream_long`` (``SoproTTS`` methods of the same names call them).

Out of scope: merging short sentences, prosody carried across segments (the model has no such input), loudness levelling,
overlap-add crossfades (the join is overlap-free on purpose: streamed pieces concatenate to the offline result bit for bit) and
text normalisation (numbers, symbols: the reference leaves it to the caller too).
"""
from __future__ import annotations

import re
from typing import Any, Dict, Iterator, List, NamedTuple, Optional, Sequence, Tuple, Union

SAMPLE_RATE = 24000
JOIN_HOP = 240  # 10 ms: the hop of the join's peak envelope

BOUNDARIES = ("paragraph", "sentence", "clause", "space", "hard", "end")
DEFAULT_PAUSES_MS: Dict[str, float] = {"paragraph": 600.0, "sentence": 250.0, "clause": 120.0, "space": 60.0, "hard": 0.0, "end": 0.0}
# a full stop after one of these tokens does not end a sentence (case-sensitive, as written)
ABBREVIATIONS = frozenset(("Mr.", "Mrs.", "Ms.", "Dr.", "Prof.", "St.", "vs.", "etc.", "e.g.", "i.e.", "No.", "Jr.", "Sr.", "Mt.", "cf."))

_PARAGRAPH = re.compile(r"\n(?:[^\S\n]*\n)+")
_STOP = re.compile(r"[.!?…]+[\"'”’»)\]}]*(?= |$)")
_OPENERS = "\"'“‘«([{"
_INITIALS = re.compile(r"(?:[A-Z]\.)+$")
_CLAUSE_MARKS = ";:,—"


class Segment(NamedTuple):
    text: str
    boundary: str  # what follows the segment: one of BOUNDARIES ("end": the last segment only)


def _sentences(par: str) -> List[str]:
    """Sentences of one whitespace-normalised paragraph (joined by single blanks they give the paragraph back)."""
    out, start = [], 0
    for m in _STOP.finditer(par):
        if m.end() >= len(par):
            break
        tok = par[par.rfind(" ", 0, m.start()) + 1: m.end()].lstrip(_OPENERS)
        if tok in ABBREVIATIONS or _INITIALS.match(tok):  # "Dr. Who", "J. R. R. Tolkien", "the U.S. fleet"
            continue
        out.append(par[start: m.end()])
        start = m.end() + 1
    out.append(par[start:])
    return out


def _cut(sentence: str, max_chars: int) -> List[Tuple[str, str]]:
    """A sentence longer than ``max_chars`` as (piece, boundary after it) with the last boundary left open (None)."""
    out: List[Tuple[str, Any]] = []
    s = sentence
    while len(s) > max_chars:
        # the last clause mark at or below the limit; it counts when a blank follows it ("3,000" and "12:30" stay whole)
        p = next((i for i in range(max_chars - 1, -1, -1) if s[i] in _CLAUSE_MARKS and s[i + 1] == " "), -1)
        if p >= 0:
            out.append((s[: p + 1], "clause"))
            s = s[p + 2:]
            continue
        p = s.rfind(" ", 0, max_chars + 1)
        if p > 0:
            out.append((s[:p], "space"))
            s = s[p + 1:]
            continue
        out.append((s[:max_chars], "hard"))  # one word longer than the limit
        s = s[max_chars:]
    out.append((s, None))
    return out


def split_text(text: str, *, max_chars: int = 280) -> List[Segment]:
    """Text -> segments of at most ``max_chars`` characters, each with the kind of boundary that follows it.

    - Whitespace runs collapse to one blank; a blank line (two or more newlines, blanks allowed between them) is a paragraph
      boundary, remembered before collapsing.
    - A sentence ends after one or more of ``. ! ? …`` plus any closing quotes / brackets directly after them, when a blank or
      the end of the text follows - but not after a token of ``ABBREVIATIONS``, nor after initials (``J.``, ``U.S.``).  A number
      such as ``3.14`` holds no blank and so never splits.
    - A sentence longer than ``max_chars`` is cut at the last of ``; : , —`` (followed by a blank) at or below the limit
      ("clause"), else at the last blank ("space"), else after exactly ``max_chars`` characters ("hard"); repeated on the rest.
    - Short sentences are NOT merged (out of scope: every sentence is a row of a batch, and rows are cheap).

    ``" ".join(s.text for s in segments)`` is the whitespace-normalised text, except that a "hard" cut joins with ``""``; no
    segment is empty; ``split_text("")`` and whitespace-only text give ``[]``."""
    max_chars = int(max_chars)
    if max_chars < 1:
        raise ValueError("max_chars must be at least 1")
    text = text.replace("\r\n", "\n").replace("\r", "\n")
    pars = [" ".join(p.split()) for p in _PARAGRAPH.split(text)]
    pars = [p for p in pars if p]
    segs: List[Segment] = []
    for pi, par in enumerate(pars):
        sents = _sentences(par)
        for si, sent in enumerate(sents):
            after = "sentence" if si + 1 < len(sents) else ("paragraph" if pi + 1 < len(pars) else "end")
            for piece, b in _cut(sent, max_chars):
                segs.append(Segment(piece, after if b is None else b))
    return segs


def pause_samples(boundary: str, pauses_ms: Optional[Dict[str, float]] = None) -> int:
    """Samples of silence (24 kHz) after a segment that ends in ``boundary``.  ``pauses_ms`` overrides ``DEFAULT_PAUSES_MS`` per
    kind; the defaults are presentation choices with no counterpart in the reference."""
    if boundary not in BOUNDARIES:
        raise ValueError(f"unknown boundary {boundary!r}")
    ms = DEFAULT_PAUSES_MS[boundary] if pauses_ms is None or boundary not in pauses_ms else float(pauses_ms[boundary])
    if ms < 0:
        raise ValueError("a pause cannot be negative")
    return int(round(ms * SAMPLE_RATE / 1000.0))


def scaled_pause(samples: int, speed: float = 1.0) -> int:
    """A pause at a speaking rate: int(round(samples / speed)) (``speed`` 1.0: unchanged)."""
    return int(samples) if float(speed) == 1.0 else int(round(int(samples) / float(speed)))


def group_plan(n: int, plan: Union[str, Sequence[int]] = "throughput", max_rows: int = 32) -> List[int]:
    """How many consecutive segments go into each ``synthesize_batch`` call.  "throughput": ``max_rows`` per group, the remainder
    last.  "latency": 1, 2, 4, ... doubling up to ``max_rows``, then ``max_rows``, the remainder last (the first audio of a stream
    waits for one short batch-of-one pass only).  A list of ints is taken as given (it must sum to ``n``)."""
    n, max_rows = int(n), int(max_rows)
    if n < 0 or max_rows < 1:
        raise ValueError("n >= 0 and max_rows >= 1")
    if not isinstance(plan, str):
        groups = [int(g) for g in plan]
        if any(g < 1 for g in groups) or sum(groups) != n:
            raise ValueError(f"a group plan must list positive sizes that sum to {n}, got {groups}")
        return groups
    if plan not in ("throughput", "latency"):
        raise ValueError("plan must be 'throughput', 'latency' or a list of group sizes")
    groups, size = [], (1 if plan == "latency" else max_rows)
    while n > 0:
        g = min(size, n)
        groups.append(g)
        n -= g
        size = min(2 * size, max_rows)
    return groups


# ------------------------------------------------------------------------------------------ engine side
class LongformPart(NamedTuple):
    """One segment as ``synthesize_batch`` returned it (``keep_parts=True``)."""
    wav: Any     # [1, 1, n] untrimmed waveform on the device
    tokens: Any  # [T, Q] int64 codec tokens on the device


class LongformResult(NamedTuple):
    wav: Any                                   # [1, 1, N] on the device, 24 kHz
    segments: List[Tuple[str, int, int]]       # (text, start sample, end sample) in ``wav``: caption / cue timing
    groups: List[int]                          # the group plan used
    parts: Optional[List[LongformPart]] = None  # keep_parts=True
    edges: Optional[List[Tuple[int, int]]] = None  # keep_parts=True: (start, end) the join kept of every part
    words: Optional[List[Any]] = None          # word_cues=True: align.LongWordCue per word, samples in ``wav`` (accurate to one frame)
    voice: Optional[List[Any]] = None          # voice_match=True: one voicematch.VoiceMatch per entry of ``segments``


def join_params(trim_db: Optional[float], keep_ms: float, fade_ms: float) -> Dict[str, Any]:
    """The join's parameters from the public ones: rel = fl32(10 ** (trim_db / 20)), keep = round(keep_ms * 24 / hop) hops,
    fade_len = round(fade_ms * 24) samples, hop = 240; ``trim_db=None``: no trimming."""
    import numpy as np

    rel = float(np.float32(10.0 ** (float(trim_db) / 20.0))) if trim_db is not None else 0.0
    return dict(hop=JOIN_HOP, rel=rel, keep=int(round(float(keep_ms) * 24.0 / JOIN_HOP)), fade_len=int(round(float(fade_ms) * 24.0)),
                trim=trim_db is not None)


class _Group(NamedTuple):
    first: int      # index of the group's first segment in the whole text
    piece: Any      # [n] joined waveform of the group, its trailing pause included
    edges: Any      # host int32 [g, 2]
    offs: Any       # host int64 [g + 1]
    batch: Any      # tts.PaddedBatch
    align: Any = None  # word_cues: one align.Alignment per row


def _groups(tts, segs: List[Segment], groups: List[int], *, ref, max_frames, top_p, temperature, anti_loop, style_strength, min_gen_frames,
            seed, pauses_ms, join_kw, fx, word_cues=False, align_heads=None) -> Iterator[_Group]:
    """Run the groups in order: one ``synthesize_batch`` and one ``hip.join_segments`` each, straight from the decoder's padded
    batch.  Segment k of the text draws with nonce (seed + k) & 0xFFFFFFFF and row id 0 - the sampler stream
    ``synthesize(segment_k, ref=ref, seed=seed + k)`` uses; without a seed every segment takes a fresh nonce.  ``fx``: every row's
    ``effects.Effects``; the batch comes back with them applied (rows in parallel, before the join: trimming, fades and cue times then
    refer to the audio as it is heard, and the squeeze never sees the pauses the join adds) and the pauses shrink or grow with
    ``fx.speed`` only."""
    from . import hip

    n = len(segs)
    nonces = [(int(seed) + k) & 0xFFFFFFFF if seed is not None else tts.model.next_nonce(None) for k in range(n)]
    gaps = [scaled_pause(pause_samples(s.boundary, pauses_ms), fx.speed) for s in segs]
    gaps[-1] = 0  # nothing follows the last segment
    k0 = 0
    for g in groups:
        sink = [] if word_cues else None  # (None: the pass launches nothing for timing)
        batch = tts.synthesize_batch([s.text for s in segs[k0: k0 + g]], [ref] * g, max_frames=max_frames, top_p=top_p, temperature=temperature,
                                     anti_loop=anti_loop, style_strength=style_strength, min_gen_frames=min_gen_frames, seed=seed,
                                     nonces=nonces[k0: k0 + g], row_ids=[0] * g, padded=True, alignment=sink,
                                     align_heads=align_heads, effects=[fx] * g)
        piece, edges, offs = hip.join_segments(batch.wav, batch.lens, gaps[k0: k0 + g], **join_kw)
        yield _Group(k0, piece, edges, offs, batch, sink)
        k0 += g


def _setup(tts, text, ref, ref_audio_path, ref_tokens_tq, ref_seconds, max_chars, plan, max_rows, denoise=None, report=None, crop=None):
    from .crop import refuse_without_waveform as crop_refuse_without_waveform
    from .denoise import refuse_without_waveform

    refuse_without_waveform(denoise, "long-form synthesis", ref=ref, ref_tokens_tq=ref_tokens_tq)
    crop_refuse_without_waveform(crop, "long-form synthesis", ref=ref, ref_tokens_tq=ref_tokens_tq)
    segs = split_text(text, max_chars=max_chars)
    groups = group_plan(len(segs), plan, max_rows)
    if segs and ref is None:  # the voice is prepared once for the whole text
        ref = tts.prepare_reference(ref_audio_path=ref_audio_path, ref_tokens_tq=ref_tokens_tq, ref_seconds=ref_seconds, denoise=denoise,
                                    report=report, crop=crop)
    return segs, groups, ref


def synthesize_long(tts, text: str, *, ref=None, ref_audio_path: Optional[str] = None, ref_tokens_tq=None, ref_seconds: Optional[float] = None,
                    max_frames: int = 400, top_p: float = 0.9, temperature: float = 1.05, anti_loop: bool = True,
                    style_strength: Optional[float] = None, min_gen_frames: Optional[int] = None, seed: Optional[int] = None,
                    max_chars: int = 280, pauses_ms: Optional[Dict[str, float]] = None, trim_db: Optional[float] = -40.0, keep_ms: float = 30.0,
                    fade_ms: float = 5.0, plan: Union[str, Sequence[int]] = "throughput", max_rows: int = 32,
                    keep_parts: bool = False, speed: float = 1.0, word_cues: bool = False, token_spans=None, align_heads=None,
                    pitch: float = 0.0, watermark=None, silence=None, denoise=None, report: Optional[list] = None, crop=None,
                    formant: Optional[float] = None, voice_match: bool = False) -> LongformResult:
    """A text of any length -> one waveform (see ``SoproTTS.synthesize_long``).  ``voice_match=True`` fills ``voice``: one
    ``VoiceMatch`` per segment, the speaker vector of the segment's generated tokens (each group's ``PaddedBatch.tokens`` over its
    ``frames``) against the voice's ``sv_ref`` (``SoproTTS.voice_similarity``; three launches per group).  ``word_cues=True`` fills ``words``: one
    ``align.LongWordCue`` per word, character offsets relative to its segment's text, samples in the joined waveform
    (``offs[k] + (cue - edge_start)`` with the cue clamped to the range the join kept of segment k, after ``effects.map_cues`` has
    taken it through its row's rate, pitch and cut table).  ``token_spans``: a callable text -> [(start, end)] per token id for
    tokenizers that give no character offsets; ``align_heads``: the (layer, head) pairs to average.  ``watermark``: the batches get no
    mark (parts stay unmarked); the joined waveform is marked in one launch, so the carrier's phase runs on across the segments and no
    cue moves.  ``formant``: every row is warped in its batch, like ``pitch``.  ``denoise``, ``crop``, ``report``: the input side, forwarded to ``prepare_reference`` (refused with ``ref`` or ``ref_tokens_tq``)."""
    import dataclasses

    import torch

    from . import align as A
    from . import effects

    fx = effects.Effects.of(speed, pitch, silence, watermark, formant)  # (a bad value is refused before anything runs)
    rows = dataclasses.replace(fx, watermark=None)
    if token_spans is not None and not callable(token_spans):
        raise TypeError("synthesize_long(token_spans=...) wants a callable: segment text -> [(start, end)] per token id")
    spans_of = token_spans if token_spans is not None else (lambda t: A.token_spans(tts.tokenizer, t))
    segs, groups, ref = _setup(tts, text, ref, ref_audio_path, ref_tokens_tq, ref_seconds, max_chars, plan, max_rows, denoise, report, crop)
    if not segs:
        return LongformResult(torch.zeros(1, 1, 0, device=tts.device), [], [], [] if keep_parts else None, [] if keep_parts else None,
                              [] if word_cues else None, [] if voice_match else None)
    if word_cues:
        spans_of(segs[0].text)  # (a tokenizer without character offsets is refused before any segment runs)
    pieces, cues, parts, all_edges, base = [], [], [], [], 0
    words = [] if word_cues else None
    voice = [] if voice_match else None
    for grp in _groups(tts, segs, groups, ref=ref, max_frames=max_frames, top_p=top_p, temperature=temperature, anti_loop=anti_loop,
                       style_strength=style_strength, min_gen_frames=min_gen_frames, seed=seed, pauses_ms=pauses_ms,
                       join_kw=join_params(trim_db, keep_ms, fade_ms), fx=rows, word_cues=word_cues, align_heads=align_heads):
        pieces.append(grp.piece)
        offs, edges = grp.offs.tolist(), grp.edges.tolist()
        if voice_match:
            voice.extend(tts.voice_similarity(ref=ref, tokens=grp.batch.tokens, lens=grp.batch.frames))
        for i, (s, e) in enumerate(edges):
            cues.append((segs[grp.first + i].text, base + offs[i], base + offs[i] + (e - s)))
            if word_cues:
                seg_text = segs[grp.first + i].text
                wc = A.word_cues(seg_text, spans_of(seg_text), grp.align[i].token_frames)
                wc = effects.map_cues(wc, rows, grp.batch.cuts[i] if grp.batch.cuts is not None else None)
                words.extend(A.long_cue(c, grp.first + i, base + offs[i], s, e) for c in wc)
            if keep_parts:
                n = grp.batch.lens[i]
                parts.append(LongformPart(grp.batch.wav[i, :n].reshape(1, 1, -1), grp.batch.tokens[i, : grp.batch.frames[i]]))
                all_edges.append((s, e))
        base += offs[-1]
    wav = (pieces[0] if len(pieces) == 1 else torch.cat(pieces)).reshape(1, 1, -1)
    if fx.watermark is not None:
        wav = effects.apply(wav.reshape(1, -1), [int(wav.shape[-1])], [effects.Effects(watermark=fx.watermark)])[0].reshape(1, 1, -1)
    return LongformResult(wav, cues, groups, parts if keep_parts else None, all_edges if keep_parts else None, words, voice)


def stream_long(tts, text: str, *, ref=None, ref_audio_path: Optional[str] = None, ref_tokens_tq=None, ref_seconds: Optional[float] = None,
                max_frames: int = 400, top_p: float = 0.9, temperature: float = 1.05, anti_loop: bool = True,
                style_strength: Optional[float] = None, min_gen_frames: Optional[int] = None, seed: Optional[int] = None,
                max_chars: int = 280, pauses_ms: Optional[Dict[str, float]] = None, trim_db: Optional[float] = -40.0, keep_ms: float = 30.0,
                fade_ms: float = 5.0, plan: Union[str, Sequence[int]] = "latency", max_rows: int = 32, speed: float = 1.0,
                pitch: float = 0.0, watermark=None, silence=None, denoise=None, report: Optional[list] = None, crop=None,
                formant: Optional[float] = None) -> Iterator[Any]:
    """The same text as a generator of joined pieces, one [1, n] tensor per group of the plan (see ``SoproTTS.stream_long``).
    ``watermark``: every piece goes through one mark-only ``effects.Chain`` (what is ready of it is yielded, nothing when that is empty)
    and a last piece carries the flush.  ``silence``: every group's batch is squeezed before its join, as in ``synthesize_long``.
    ``denoise``, ``crop``, ``report``: the input side, forwarded to ``prepare_reference``."""
    import dataclasses

    from .effects import Chain, Effects

    fx = Effects.of(speed, pitch, silence, watermark, formant)
    segs, groups, ref = _setup(tts, text, ref, ref_audio_path, ref_tokens_tq, ref_seconds, max_chars, plan, max_rows, denoise, report, crop)
    if not segs:
        return
    mark = Chain.of(Effects(watermark=fx.watermark), tts.device)
    for grp in _groups(tts, segs, groups, ref=ref, max_frames=max_frames, top_p=top_p, temperature=temperature, anti_loop=anti_loop,
                       style_strength=style_strength, min_gen_frames=min_gen_frames, seed=seed, pauses_ms=pauses_ms,
                       join_kw=join_params(trim_db, keep_ms, fade_ms), fx=dataclasses.replace(fx, watermark=None)):
        piece = mark.feed(grp.piece.reshape(1, -1))
        if piece is not None:
            yield piece
    piece = mark.flush()
    if piece is not None:
        yield piece
