"""Chunked streaming synthesis (reference: src/sopro/streaming.py:12-152).

AR tokens are produced ``chunk_frames`` at a time by replaying the recorded per-frame hipGraph;
every chunk the NAR refiner is re-run on a left-context window of ``rf_nar`` frames and the new
frames go through the streaming Mimi decoder.  Same chunking policy, same stop rule (first EOS,
regardless of ``min_gen_frames``: streaming.py:114-115) and same yielded shapes ``[1, n*1920]``.
"""
from __future__ import annotations

from dataclasses import dataclass
import contextlib
import time
from typing import Callable, Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .codec import MimiDecodeState, MimiStreamBatchState, MimiStreamDecoder
from .model import PreparedReference


@dataclass
class StreamConfig:
    chunk_frames: int = 16
    nar_context_frames: Optional[int] = None
    cache_trim: str = "none"  # MimiStreamDecoder policy: "none" = transformers 5.x behaviour, "legacy" = 4.57.6 (quirk Q6)


class SoproTTSStreamer:
    def __init__(self, tts, cfg: Optional[StreamConfig] = None):
        self.tts = tts
        self.cfg = cfg or StreamConfig()
        self.mimi_stream = MimiStreamDecoder(tts.codec, trim=self.cfg.cache_trim)

    @torch.inference_mode()
    def stream(self, text: str, *, ref_audio_path: Optional[str] = None, ref_tokens_tq: Optional[torch.Tensor] = None,
               ref: Optional[PreparedReference] = None, max_frames: int = 400, top_p: float = 0.9,
               temperature: float = 1.05, anti_loop: bool = True, style_strength: Optional[float] = None,
               ref_seconds: Optional[float] = None, chunk_frames: Optional[int] = None,
               nar_context_frames: Optional[int] = None, min_gen_frames: Optional[int] = None,
               text_ids: Optional[torch.Tensor] = None, seed: Optional[int] = None, speed: float = 1.0,
               pitch: float = 0.0, watermark=None, silence=None, denoise=None, report: Optional[list] = None, crop=None,
               formant: Optional[float] = None) -> Iterator[torch.Tensor]:
        """``speed``, ``pitch``, ``formant``, ``silence``, ``watermark`` (new): every decoded chunk goes through an ``effects.Chain`` and what is
        ready of it is yielded as [1, n] (a step that completes nothing yields nothing); a flush after the last chunk yields the rest.
        The concatenation is ``effects.apply`` of the plain stream's concatenation, bit for bit (``sopro_amd.effects``).
        ``denoise``, ``crop``, ``report``: the input side, forwarded to ``prepare_reference``."""
        from .effects import Chain, Effects

        tts = self.tts
        chain = Chain.of(Effects.of(speed, pitch, silence, watermark, formant), tts.device)

        model = tts.model
        ids = text_ids if text_ids is not None else tts.encode_text(text)
        if ref is None:
            ref = tts.prepare_reference(ref_audio_path=ref_audio_path, ref_tokens_tq=ref_tokens_tq, ref_seconds=ref_seconds, denoise=denoise,
                                        report=report, crop=crop)
        prep = model.prepare_conditioning(
            ids, ref, max_frames=max_frames,
            style_strength=float(style_strength if style_strength is not None else tts.cfg.style_strength))
        cf = int(chunk_frames if chunk_frames is not None else self.cfg.chunk_frames)
        nar_ctx = nar_context_frames if nar_context_frames is not None else self.cfg.nar_context_frames
        if nar_ctx is None:
            nar_ctx = int(model.rf_nar())
        nar_ctx = int(nar_ctx)

        hist: List[int] = []
        emitted = 0
        state = MimiDecodeState()

        def refine_and_emit(end: int) -> Optional[torch.Tensor]:
            nonlocal emitted, state
            if end <= emitted:
                return None
            ws = max(0, emitted - nar_ctx)
            cond_win = prep["cond_ar"][:, ws:end, :]
            tok_a = torch.as_tensor(hist[ws:end], dtype=torch.long).unsqueeze(0)
            toks = model.nar_refine(cond_win, tok_a).squeeze(0)
            wav, state = self.mimi_stream.decode_step(toks[emitted - ws:, :], state)
            emitted = end
            return wav if wav.numel() > 0 else None

        for _t, tok, is_eos in model.ar_stream(prep, max_frames=max_frames, top_p=top_p, temperature=temperature,
                                               anti_loop=anti_loop, min_gen_frames=min_gen_frames, lookahead=cf, seed=seed):
            if is_eos:
                break
            hist.append(int(tok))
            if len(hist) % cf == 0:
                wav = chain.feed(refine_and_emit(len(hist)))
                if wav is not None:
                    yield wav
        if emitted < len(hist):
            wav = chain.feed(refine_and_emit(len(hist)))
            if wav is not None:
                yield wav
        wav = chain.flush()
        if wav is not None:
            yield wav


    @torch.inference_mode()
    def stream_timed(self, text: str, spans, *, lag_frames: int = 8, align_heads=None, ref_audio_path: Optional[str] = None,
                     ref_tokens_tq: Optional[torch.Tensor] = None, ref: Optional[PreparedReference] = None, max_frames: int = 400,
                     top_p: float = 0.9, temperature: float = 1.05, anti_loop: bool = True, style_strength: Optional[float] = None,
                     ref_seconds: Optional[float] = None, chunk_frames: Optional[int] = None, nar_context_frames: Optional[int] = None,
                     min_gen_frames: Optional[int] = None, text_ids: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                     speed: float = 1.0, pitch: float = 0.0, watermark=None, denoise=None, report: Optional[list] = None, crop=None,
                     formant: Optional[float] = None):
        """``stream`` with word cues (``SoproTTS.stream_timed``): the same sampler draws, chunks and effects chain, and after every
        chunk's decode one step of ``replay.AlignStream`` on the frames generated so far.  Yields ``align.TimedChunk``; the words of an
        item are those the step closed, mapped through ``speed`` / ``pitch`` like ``synthesize_timed``'s.  The aligner steps at every
        multiple of ``chunk_frames`` (not final: whether the utterance ends there is only known a frame later) and once more, final,
        when the generator stops.  The loop is ``stream``'s, written out again rather than shared, so that ``stream`` runs the code
        it ran before this method existed (``silence`` is not a keyword here: its cut table does not exist chunk by chunk)."""
        from . import align as A
        from .effects import Chain, Effects, map_cues

        tts = self.tts
        fx = Effects.of(speed, pitch, None, watermark, formant)
        chain = Chain.of(fx, tts.device)
        model = tts.model
        ids = text_ids if text_ids is not None else tts.encode_text(text)
        if len(spans) != int(ids.numel()):
            raise ValueError(f"token_spans: {len(spans)} spans for {int(ids.numel())} token ids")
        if ref is None:
            ref = tts.prepare_reference(ref_audio_path=ref_audio_path, ref_tokens_tq=ref_tokens_tq, ref_seconds=ref_seconds, denoise=denoise,
                                        report=report, crop=crop)
        prep = model.prepare_conditioning(
            ids, ref, max_frames=max_frames,
            style_strength=float(style_strength if style_strength is not None else tts.cfg.style_strength))
        cf = int(chunk_frames if chunk_frames is not None else self.cfg.chunk_frames)
        nar_ctx = nar_context_frames if nar_context_frames is not None else self.cfg.nar_context_frames
        if nar_ctx is None:
            nar_ctx = int(model.rf_nar())
        nar_ctx = int(nar_ctx)
        al = model.align_stream(prep, max_frames=max_frames, lag_frames=lag_frames, chunk_frames=cf, heads=align_heads)
        cues = A.StreamCues(text, spans, hop=int(tts.codec.mc.frame_samples))

        hist: List[int] = []
        emitted = 0
        state = MimiDecodeState()
        empty = torch.zeros(1, 0, device=tts.device)

        def refine_and_emit(end: int) -> Optional[torch.Tensor]:
            nonlocal emitted, state
            if end <= emitted:
                return None
            ws = max(0, emitted - nar_ctx)
            cond_win = prep["cond_ar"][:, ws:end, :]
            tok_a = torch.as_tensor(hist[ws:end], dtype=torch.long).unsqueeze(0)
            toks = model.nar_refine(cond_win, tok_a).squeeze(0)
            wav, state = self.mimi_stream.decode_step(toks[emitted - ws:, :], state)
            emitted = end
            return wav if wav.numel() > 0 else None

        for _t, tok, is_eos in model.ar_stream(prep, max_frames=max_frames, top_p=top_p, temperature=temperature,
                                               anti_loop=anti_loop, min_gen_frames=min_gen_frames, lookahead=cf, seed=seed):
            if is_eos:
                break
            hist.append(int(tok))
            if len(hist) % cf == 0:
                wav = chain.feed(refine_and_emit(len(hist)))
                words = map_cues(cues.feed(al.step(hist, len(hist), False)), fx)
                if wav is not None or words:
                    yield A.TimedChunk(wav if wav is not None else empty, words, False)
        if emitted < len(hist):
            wav = chain.feed(refine_and_emit(len(hist)))
            if wav is not None:
                yield A.TimedChunk(wav, [], False)
        words = map_cues(cues.feed(al.step(hist, len(hist), True), final=True), fx)
        wav = chain.flush()
        # (not the device's word: a final step that finds every frame committed - lag 0, the end on a chunk boundary - changes nothing)
        status = 0 if (al.path and al.path[-1] == len(spans) - 1) else 2
        alignment = A.Alignment(path=list(al.path), token_frames=A.path_token_frames(al.path, len(spans)), total=float(al.base), status=status)
        yield A.TimedChunk(wav if wav is not None else empty, words, True, alignment)


@torch.inference_mode()
def stream_timed(tts, text: str, *, lag_frames: int = 8, token_spans=None, align_heads=None, chunk_frames: int = 6, cache_trim: str = "none",
                 speed: float = 1.0, pitch: float = 0.0, watermark=None, silence=None, formant: Optional[float] = None, **kwargs):
    """New: ``stream`` with word cues as they are committed -> an iterator of ``align.TimedChunk`` (see
    SoproTTSStreamer.stream_timed).  Everything that can be refused is refused here, before anything runs: ``silence=`` (its cut table
    does not exist chunk by chunk), ``lag_frames + chunk_frames > 63`` (the online aligner's window), bad effect values, a bad head
    selection, spans that do not match the text's ids."""
    from . import align as A
    from .crop import refuse_without_waveform as crop_refuse_without_waveform
    from .denoise import refuse_without_waveform
    from .effects import Effects, refuse

    refuse("stream_timed", silence=silence)
    refuse_without_waveform(kwargs.get("denoise"), "stream_timed", ref=kwargs.get("ref"), ref_tokens_tq=kwargs.get("ref_tokens_tq"))
    crop_refuse_without_waveform(kwargs.get("crop"), "stream_timed", ref=kwargs.get("ref"), ref_tokens_tq=kwargs.get("ref_tokens_tq"))
    A.check_align_window(lag_frames, chunk_frames)
    Effects.of(speed, pitch, None, watermark, formant)
    tts.model._align_heads(align_heads)
    spans = token_spans(text) if callable(token_spans) else (list(token_spans) if token_spans is not None else A.token_spans(tts.tokenizer, text))
    streamer = SoproTTSStreamer(tts, StreamConfig(chunk_frames=chunk_frames, cache_trim=cache_trim))
    return streamer.stream_timed(text, spans, lag_frames=lag_frames, align_heads=align_heads, chunk_frames=chunk_frames, speed=speed,
                                 pitch=pitch, watermark=watermark, formant=formant, **kwargs)


@torch.inference_mode()
def stream(tts, text: str, *, ref_audio_path: Optional[str] = None, ref_tokens_tq: Optional[torch.Tensor] = None,
           ref: Optional[PreparedReference] = None, chunk_frames: int = 6, cache_trim: str = "none", speed: float = 1.0,
           pitch: float = 0.0, watermark=None, silence=None, formant: Optional[float] = None, **kwargs) -> Iterator[torch.Tensor]:
    """reference: src/sopro/streaming.py:133-152 (``cache_trim``, ``speed``, ``pitch``, ``formant``, ``watermark`` and ``silence`` are new: see
    MimiStreamDecoder, SoproTTSStreamer.stream)"""
    from .crop import refuse_without_waveform as crop_refuse_without_waveform
    from .denoise import refuse_without_waveform
    from .effects import Effects

    Effects.of(speed, pitch, silence, watermark, formant)  # (a bad value is refused here, not at the first chunk)
    refuse_without_waveform(kwargs.get("denoise"), "stream", ref=ref, ref_tokens_tq=ref_tokens_tq)
    crop_refuse_without_waveform(kwargs.get("crop"), "stream", ref=ref, ref_tokens_tq=ref_tokens_tq)
    streamer = SoproTTSStreamer(tts, StreamConfig(chunk_frames=chunk_frames, cache_trim=cache_trim))
    return streamer.stream(text, ref_audio_path=ref_audio_path, ref_tokens_tq=ref_tokens_tq, ref=ref,
                           chunk_frames=chunk_frames, speed=speed, pitch=pitch, watermark=watermark, silence=silence, formant=formant, **kwargs)


# ---------------------------------------------------------------------------------------------------------------------------------
# Batched streaming: B utterances in lockstep (same chunk_frames / max_frames / sampling / style / cache policy; own text, voice, seed
# and end).  Every step advances the batched AR run by one chunk, refines all emitting rows at once over the shared left-context window
# and decodes them in one call of the batched stream decoder.  Per row, the chunks are exactly what ``stream()`` yields for that row.

def step_plan(t0: int, t1: int, lens: Sequence[Optional[int]], nar_ctx: int) -> Tuple[int, List[Optional[int]]]:
    """One lockstep step over AR frames [t0, t1) for the live rows (every one has emitted frames [0, t0) so far).  ``lens[b]``: the
    row's final history length (its first EOS frame, or max_frames + 1) once known, None while it runs past t1.
    -> (ws, ends): the refinement window starts at ws = max(0, t0 - nar_ctx) for all rows; row b emits frames [t0, ends[b]) with
    ends[b] = min(t1, lens[b]), or nothing (None) when that is empty - the reference's ``refine_and_emit(end)`` with
    ``end <= frames_emitted`` (src/sopro/streaming.py:81-104)."""
    ws = max(0, int(t0) - int(nar_ctx))
    ends: List[Optional[int]] = []
    for L in lens:
        e = int(t1) if L is None else min(int(t1), int(L))
        ends.append(e if e > t0 else None)
    return ws, ends


def stream_schedule(lens: Sequence[int], chunk_frames: int, nar_ctx: int, n_frames: int) -> List[Dict[str, object]]:
    """The whole lockstep schedule for rows whose final history lengths ``lens`` (first EOS frame, else ``n_frames`` =
    max_frames + 1) are given up front: a list of steps {"t0", "t1", "ws", "ends": one entry per row (None: no chunk)}.  Rows leave
    after the step whose window reaches their length; steps in which no row emits are left out.  (The host loop learns the lengths
    step by step from the tokens; a length equal to t1 it learns one step later, which changes no chunk.)"""
    cf = int(chunk_frames)
    if cf < 1:
        raise ValueError("chunk_frames must be >= 1")
    B = len(lens)
    live = list(range(B))
    steps: List[Dict[str, object]] = []
    t0 = 0
    while live and t0 < n_frames:
        t1 = min(t0 + cf, int(n_frames))
        known = [int(lens[b]) if int(lens[b]) <= t1 else None for b in live]
        ws, ends_live = step_plan(t0, t1, known, nar_ctx)
        ends: List[Optional[int]] = [None] * B
        for b, e in zip(live, ends_live):
            ends[b] = e
        if any(e is not None for e in ends):
            steps.append({"t0": t0, "t1": t1, "ws": ws, "ends": ends})
        live = [b for b, k in zip(live, known) if k is None]
        t0 = t1
    return steps


@torch.inference_mode()
def stream_batch(tts, texts: Sequence[str], refs: Sequence, *, chunk_frames: int = 6, max_frames: int = 400, top_p: float = 0.9,
                 temperature: float = 1.05, anti_loop: bool = True, style_strength: Optional[float] = None,
                 min_gen_frames: Optional[int] = None, seeds: Optional[Sequence[Optional[int]]] = None, cache_trim: str = "none",
                 nar_context_frames: Optional[int] = None, text_ids: Optional[Sequence[torch.Tensor]] = None,
                 phase_locks: Optional[tuple] = None, timings: Optional[Dict[str, float]] = None,
                 alive: Optional[Callable[[int], bool]] = None, speed: float = 1.0,
                 pitch: float = 0.0, watermark=None, silence=None, formant: Optional[float] = None) -> Iterator[List[Optional[torch.Tensor]]]:
    """B utterances streamed in lockstep.  Yields, per step, a list of B entries: a [1, n * 1920] chunk or None.  Row b's non-None
    chunks are what ``stream(texts[b], ref=refs[b], seed=seeds[b], ...)`` yields: same chunk sizes, same stop rule (first EOS).
    ``seeds``: one per row (None: a fresh take for that row).  ``phase_locks`` = (AR lock, bulk lock): held around the AR advance and
    around refinement + decode of every step (a serving lane shares its device with whole-utterance batches).  ``timings``: seconds
    of host wall time accumulated under "ar", "refine", "decode".  ``alive(b)`` (a server): False once row b's consumer has gone - the
    row then leaves the batch at the next step as if it had ended there.  ``speed``: only 1.0, ``pitch``: only 0.0,
    ``formant``: only None or ``pitch``, ``watermark``, ``silence``: only None (batched streams have none of the five effects)."""
    from .effects import refuse

    refuse("stream_batch", speed=speed, pitch=pitch, watermark=watermark, silence=silence, formant=formant)
    model = tts.model
    B = len(texts)
    if B == 0 or len(refs) != B:
        raise ValueError("need one reference per text")
    cf = int(chunk_frames)
    if cf < 1:
        raise ValueError("chunk_frames must be >= 1")
    locks = tuple(phase_locks) if phase_locks is not None else ()
    ar_lock = locks[0] if len(locks) > 0 else contextlib.nullcontext()
    bulk_lock = locks[1] if len(locks) > 1 else contextlib.nullcontext()
    ids = list(text_ids) if text_ids is not None else [tts.encode_text(t) for t in texts]
    ss = float(style_strength if style_strength is not None else tts.cfg.style_strength)
    nar_ctx = int(nar_context_frames if nar_context_frames is not None else model.rf_nar())
    if seeds is not None and len(seeds) != B:
        raise ValueError("one seed per row")
    # row b draws what a single-row run with nonce next_nonce(seed_b) draws: its own nonce, row index 0
    nonces = [model.next_nonce(seeds[b] if seeds is not None else None) for b in range(B)]
    tm = timings if timings is not None else {}
    for k in ("ar", "refine", "decode"):
        tm.setdefault(k, 0.0)
    prep = model.prepare_conditioning_batch(ids, list(refs), max_frames=max_frames, style_strength=ss)
    run = model.ar_prepare(prep, top_p=top_p, temperature=temperature, anti_loop=anti_loop, min_gen_frames=min_gen_frames,
                           nonces=nonces, row_ids=[0] * B)
    Tar = int(max_frames) + 1
    eos = int(model.V)
    dec = MimiStreamDecoder(tts.codec, trim=cache_trim)
    state: Optional[MimiStreamBatchState] = None
    hist = np.zeros((B, Tar), dtype=np.int64)
    lens: List[Optional[int]] = [None] * B
    live = list(range(B))  # rows that have not ended
    dec_rows: List[int] = []  # rows in the decoder state's order (those that emitted in its last call)
    cond = prep["cond_ar"]
    try:
        t0 = 0
        t_ar = time.perf_counter()
        with ar_lock:
            run.advance(min(cf, Tar))
        while live and t0 < Tar:
            t1 = min(t0 + cf, Tar)
            if alive is not None:
                for b in live:
                    if lens[b] is None and not alive(b):
                        lens[b] = t0  # (emits nothing more: leaves with this step)
            with ar_lock:
                hist[:, t0:t1] = run.tokens_host_batch(t0, t1)
                for b in live:
                    if lens[b] is None:
                        hit = np.nonzero(hist[b, t0:t1] == eos)[0]
                        if hit.size:
                            lens[b] = t0 + int(hit[0])
                        elif t1 == Tar:
                            lens[b] = Tar
                still = [b for b in live if lens[b] is None]
                if still and t1 < Tar:  # the next chunk's frames are generated while this one is refined and decoded
                    run.advance(min(cf, Tar - t1))
            tm["ar"] += time.perf_counter() - t_ar
            ws, ends_live = step_plan(t0, t1, [lens[b] for b in live], nar_ctx)
            ends = {b: e for b, e in zip(live, ends_live) if e is not None}
            if ends:
                em = sorted(ends)
                e_max = max(ends.values())
                with bulk_lock:
                    t_r = time.perf_counter()
                    idx = torch.tensor(em, device=cond.device)
                    cond_win = cond.index_select(0, idx)[:, ws:e_max, :]
                    tok_a = torch.from_numpy(hist[em, ws:e_max])
                    toks = model.nar_refine(cond_win, tok_a, lens=[ends[b] - ws for b in em])
                    t_d = time.perf_counter()
                    tm["refine"] += t_d - t_r
                    pos = {b: j for j, b in enumerate(em)}
                    rows = dec_rows if state is not None else em
                    chunks = [toks[pos[b], t0 - ws:ends[b] - ws, :] if b in ends else None for b in rows]
                    wavs, state = dec.decode_step_batch(chunks, state)
                    tm["decode"] += time.perf_counter() - t_d
                out: List[Optional[torch.Tensor]] = [None] * B
                for b, w in zip(rows, wavs):
                    if w is not None and w.numel() > 0:
                        out[b] = w
                dec_rows = [b for b in rows if b in ends]
                yield out
            live = [b for b in live if lens[b] is None]
            t0 = t1
            t_ar = time.perf_counter()
    finally:
        run.done = True  # also when the consumer abandons the generator: the plan is free again
