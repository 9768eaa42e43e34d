"""Batched admission in front of the engine (the serving loop's engine side).

The reference's demo server serialises requests behind one global lock (demo/server.py:56, 224, 241): one utterance on
the device at a time.  Here concurrent callers ``submit`` requests; a scheduler groups compatible ones (same sampling
parameters and frame budget: those are per-launch constants of the AR graph) into batches of up to ``max_batch`` rows,
waiting at most ``max_wait_ms`` for a batch to fill, and the batches flow through the lanes of a
``PipelinedSynthesizer`` (generation of one batch overlaps refinement / decoding of others).  Text lengths, reference
voices and end-of-speech times may differ inside a batch.  Transport (HTTP, framing into responses) stays outside:
``sopro_amd.wire`` has the byte formats.
"""
from __future__ import annotations

import atexit
import queue
import threading
import time
from concurrent.futures import Future
from dataclasses import dataclass
from typing import Any, Dict, Iterator, List, Optional, Tuple

import torch

from .model import PreparedReference


@dataclass
class _Request:
    text_ids: torch.Tensor
    ref: PreparedReference
    key: Tuple
    future: Future
    t_submit: float
    stream: Optional["_StreamSink"] = None  # submit_stream: where the lane puts this row's chunks
    seed: Optional[int] = None
    fx: Any = None  # submit: this request's effects.Effects (formant included) - applied after decoding, one per row, so no part of the batching key
    silence: Any = None  # the silence control of this request: applied after rate and pitch, one per row


class _StreamSink:
    """The blocking iterator ``submit_stream`` returns: an unbounded queue the lane fills (a slow or absent reader never holds up the
    batch), ended by a sentinel or an exception.  A consumer that closes it or drops it makes its row leave the batch."""

    _END = object()

    def __init__(self):
        self.q: "queue.Queue[Any]" = queue.Queue()
        self.cancelled = threading.Event()
        self._done = False

    def put(self, item) -> None:
        if not self.cancelled.is_set():
            self.q.put(item)

    def __iter__(self) -> "Iterator[torch.Tensor]":
        return self

    def __next__(self) -> torch.Tensor:
        if self._done:
            raise StopIteration
        item = self.q.get()
        if item is self._END:
            self._done = True
            raise StopIteration
        if isinstance(item, BaseException):
            self._done = True
            raise item
        return item

    def close(self) -> None:
        self._done = True
        self.cancelled.set()

    def __del__(self):
        self.cancelled.set()


class SynthesisService:
    def __init__(self, tts, *, max_batch: int = 32, max_wait_ms: float = 4.0, lanes: int = 4, ar_cus: int = 64, ar_parts: int = 2,
                 ar_shared: bool = True, mode: str = "batch", **continuous_kw):
        """``mode="batch"``: requests with equal parameters are grouped into batches for the lanes of a PipelinedSynthesizer.
        ``mode="continuous"``: frame-level admission (``ContinuousSynthesizer``; extra keywords go to it): parameters, frame
        budgets and end-of-speech times may all differ between neighbouring slots."""
        from .pipeline import PipelinedSynthesizer

        self.tts = tts
        self._closed = False
        self.stats = {"requests": 0, "batches": 0, "rows": 0, "stream_batches": 0}
        self.engine = None
        if mode == "continuous":
            from .continuous import ContinuousSynthesizer

            kw = dict(slots=max_batch, ar_cus=ar_cus, generators=max(1, ar_parts))
            kw.update(continuous_kw)
            self.engine = ContinuousSynthesizer(tts, **kw)
            self.engine.start()
            self.pipe, self._threads = None, []
            return
        if mode != "batch":
            raise ValueError("mode must be 'batch' or 'continuous'")
        self.max_batch, self.max_wait = int(max_batch), float(max_wait_ms) * 1e-3
        self.pipe = PipelinedSynthesizer(tts, lanes=lanes, ar_cus=ar_cus, ar_parts=ar_parts, ar_shared=ar_shared) if lanes > 1 else None
        self._lanes = self.pipe.lanes if self.pipe is not None else [tts]
        self._inbox: "queue.Queue[Optional[_Request]]" = queue.Queue()
        self._batches: "queue.Queue[Optional[List[_Request]]]" = queue.Queue(maxsize=2 * len(self._lanes))
        self._threads = [threading.Thread(target=self._schedule, name="sopro-sched", daemon=True)]
        for i, lane in enumerate(self._lanes):
            self._threads.append(threading.Thread(target=self._work, args=(lane, i), name=f"sopro-lane{i}", daemon=True))
        for t in self._threads:
            t.start()
        atexit.register(self.close)  # worker threads must not be inside the HIP runtime when the interpreter tears it down

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------ client side
    def submit(self, text: str, ref: PreparedReference, *, max_frames: int = 400, top_p: float = 0.9, temperature: float = 1.05,
               anti_loop: bool = True, style_strength: Optional[float] = None, min_gen_frames: Optional[int] = None,
               text_ids: Optional[torch.Tensor] = None, speed: float = 1.0, pitch: float = 0.0, watermark=None, silence=None,
               formant: Optional[float] = None, **timing) -> "Future[torch.Tensor]":
        """Queue one utterance; the future resolves to the waveform ``[1, 1, N]`` on the device (``synthesize``'s result).
        ``speed``, ``pitch``, ``formant``, ``silence``, ``watermark`` (``sopro_amd.effects``; ``mode="batch"`` only): this request's own.  They are
        applied to the decoded batch, one setting per row, so requests (and tenants) that differ in them share a batch.  The service
        has no word timing in either mode: a timing keyword (``alignment``, ``word_cues``, ...) raises."""
        from . import effects
        from .align import refuse_timing

        refuse_timing(timing, f"SynthesisService(mode={'continuous' if self.engine is not None else 'batch'!r})")
        if timing:
            raise TypeError(f"submit() got unexpected keyword arguments {sorted(timing)}")
        if self._closed:
            raise RuntimeError("service is closed")
        fx = effects.Effects.of(speed, pitch, silence, watermark, formant)
        if self.engine is not None:
            effects.refuse("SynthesisService(mode='continuous')", speed=speed, pitch=pitch, watermark=watermark, silence=silence, formant=formant)
            self.stats["requests"] += 1
            return self.engine.submit(text=text, text_ids=text_ids, ref=ref, max_frames=max_frames, top_p=top_p, temperature=temperature,
                                      anti_loop=anti_loop, style_strength=style_strength, min_gen_frames=min_gen_frames)
        ids = text_ids if text_ids is not None else self.tts.encode_text(text)
        if int(ids.numel()) == 0:
            raise ValueError("empty text")
        ss = float(style_strength if style_strength is not None else self.tts.cfg.style_strength)
        key = (int(max_frames), float(top_p), float(temperature), bool(anti_loop), ss, min_gen_frames)
        fut: Future = Future()
        self._inbox.put(_Request(ids, ref, key, fut, time.perf_counter(), fx=fx))
        return fut

    def submit_stream(self, text: str, ref: PreparedReference, *, max_frames: int = 400, top_p: float = 0.9, temperature: float = 1.05,
                      anti_loop: bool = True, style_strength: Optional[float] = None, min_gen_frames: Optional[int] = None,
                      text_ids: Optional[torch.Tensor] = None, chunk_frames: int = 6, cache_trim: str = "none",
                      nar_context_frames: Optional[int] = None, seed: Optional[int] = None, speed: float = 1.0,
                      pitch: float = 0.0, watermark=None, silence=None, formant: Optional[float] = None) -> Iterator[torch.Tensor]:
        """Queue one streamed utterance -> a blocking iterator over its [1, n * 1920] chunks (``stream``'s chunks).  Streams with equal
        parameters are grouped into batches of up to ``max_batch`` rows (within ``max_wait_ms``) and each batch runs as one
        ``stream_batch`` on a lane, sharing the device with whole-utterance batches (AR lock per chunk, bulk lock for refinement and
        decoding).  Closing or dropping the iterator drops the row from its batch.  Batched streams have none of the five effects:
        ``speed`` other than 1.0, ``pitch`` other than 0.0, a ``formant`` other than None or ``pitch``, ``watermark`` or ``silence`` other than
        None raises."""
        from .effects import refuse

        if self._closed:
            raise RuntimeError("service is closed")
        refuse("submit_stream", speed=speed, pitch=pitch, watermark=watermark, silence=silence, formant=formant)
        if self.engine is not None:
            raise RuntimeError("submit_stream is not available in mode='continuous' (frame-level admission has no streaming path); "
                               "use mode='batch'")
        ids = text_ids if text_ids is not None else self.tts.encode_text(text)
        if int(ids.numel()) == 0:
            raise ValueError("empty text")
        if cache_trim not in ("none", "legacy"):
            raise ValueError("cache_trim must be 'none' or 'legacy'")
        ss = float(style_strength if style_strength is not None else self.tts.cfg.style_strength)
        key = ("stream", int(max_frames), float(top_p), float(temperature), bool(anti_loop), ss, min_gen_frames, int(chunk_frames), cache_trim,
               nar_context_frames)
        sink = _StreamSink()
        self._inbox.put(_Request(ids, ref, key, Future(), time.perf_counter(), stream=sink, seed=seed))
        return sink

    def submit_long(self, text: str, ref: PreparedReference, *, max_frames: int = 400, top_p: float = 0.9, temperature: float = 1.05,
                    anti_loop: bool = True, style_strength: Optional[float] = None, min_gen_frames: Optional[int] = None,
                    max_chars: int = 280, pauses_ms: Optional[Dict[str, float]] = None, trim_db: Optional[float] = -40.0,
                    keep_ms: float = 30.0, fade_ms: float = 5.0, keep_parts: bool = False, speed: float = 1.0,
                    pitch: float = 0.0, watermark=None, silence=None, formant: Optional[float] = None) -> "Future":
        """Queue a text of any length -> a future of ``longform.LongformResult`` (``SoproTTS.synthesize_long``'s result).  The text is
        split here and every segment goes through ``submit``, so the scheduler batches the segments with whatever else is queued;
        a small waiter thread gathers the segment futures in order, stacks them into one padded tensor and joins them on the
        device (``hip.join_segments``).  The sampler draws as ``submit`` draws (a fresh take per segment: no seed, no group plan).
        ``speed``, ``pitch``, ``formant``, ``silence``: every segment is submitted with them (applied in its batch, before the join); the pauses are
        divided by ``speed`` only.  ``watermark``: the segments are submitted unmarked and the joined waveform is marked, as in
        ``SoproTTS.synthesize_long``."""
        from . import effects, hip
        from .longform import LongformPart, LongformResult, join_params, pause_samples, scaled_pause, split_text

        fx = effects.Effects.of(speed, pitch, silence, watermark, formant)
        mark = effects.Effects(watermark=fx.watermark)

        if self._closed:
            raise RuntimeError("service is closed")
        if self.engine is not None:
            raise RuntimeError("submit_long is not available in mode='continuous'; use mode='batch'")
        segs = split_text(text, max_chars=max_chars)
        gaps = [scaled_pause(pause_samples(s.boundary, pauses_ms), speed) for s in segs]
        join_kw = join_params(trim_db, keep_ms, fade_ms)
        futs = [self.submit(s.text, ref, max_frames=max_frames, top_p=top_p, temperature=temperature, anti_loop=anti_loop,
                            style_strength=style_strength, min_gen_frames=min_gen_frames, speed=speed, pitch=pitch, silence=silence,
                            formant=formant) for s in segs]
        done: Future = Future()
        dev = self.tts.device

        def gather() -> None:
            try:
                if not segs:
                    done.set_result(LongformResult(torch.zeros(1, 1, 0, device=dev), [], [], [] if keep_parts else None, [] if keep_parts else None))
                    return
                gaps[-1] = 0
                wavs = [f.result().reshape(-1) for f in futs]
                lens = [int(w.numel()) for w in wavs]
                with torch.cuda.device(dev):
                    # the lanes synchronise their streams before a future resolves: the rows are complete when they are read here
                    rows = torch.zeros(len(wavs), max(1, max(lens)), device=dev)
                    for k, w in enumerate(wavs):
                        rows[k, : lens[k]] = w
                    out, edges, offs = hip.join_segments(rows, lens, gaps, **join_kw)
                    if not mark.plain and out.numel() > 0:
                        out = effects.apply(out.reshape(1, -1), [int(out.numel())], [mark])[0].reshape(-1)
                        torch.cuda.current_stream(dev).synchronize()  # (the future's reader may be on another stream)
                o, e = offs.tolist(), edges.tolist()
                cues = [(segs[k].text, o[k], o[k] + e[k][1] - e[k][0]) for k in range(len(segs))]
                parts = [LongformPart(w.reshape(1, 1, -1), None) for w in wavs] if keep_parts else None
                done.set_result(LongformResult(out.reshape(1, 1, -1), cues, [len(segs)], parts, [tuple(x) for x in e] if keep_parts else None))
            except BaseException as exc:  # noqa: BLE001
                done.set_exception(exc)

        threading.Thread(target=gather, name="sopro-long", daemon=True).start()
        return done

    def synthesize(self, text: str, ref: PreparedReference, **kw) -> torch.Tensor:
        return self.submit(text, ref, **kw).result()

    def close(self) -> None:
        if self._closed:
            return
        self._closed = True
        atexit.unregister(self.close)
        if self.engine is not None:
            self.engine.close()
            return
        self._inbox.put(None)
        for t in self._threads:
            t.join()
        if self.pipe is not None:
            self.pipe.close()

    # ------------------------------------------------------------------ scheduler: group compatible requests
    def _schedule(self) -> None:
        pending: Dict[Tuple, List[_Request]] = {}
        stop = False
        while not stop or pending:
            deadline = min((rs[0].t_submit + self.max_wait for rs in pending.values()), default=None)
            timeout = None if deadline is None else max(0.0, deadline - time.perf_counter())
            try:
                r = self._inbox.get(timeout=timeout) if not stop else None
                if r is None and not stop:
                    stop = True
                elif r is not None:
                    pending.setdefault(r.key, []).append(r)
                    while True:  # drain whatever else is already queued
                        try:
                            r2 = self._inbox.get_nowait()
                        except queue.Empty:
                            break
                        if r2 is None:
                            stop = True
                        else:
                            pending.setdefault(r2.key, []).append(r2)
            except queue.Empty:
                pass
            now = time.perf_counter()
            for key in list(pending):
                rs = pending[key]
                while len(rs) >= self.max_batch:
                    self._batches.put(rs[: self.max_batch])
                    del rs[: self.max_batch]
                if rs and (stop or now >= rs[0].t_submit + self.max_wait):
                    self._batches.put(list(rs))
                    rs.clear()
                if not rs:
                    del pending[key]
        for _ in self._lanes:
            self._batches.put(None)

    # ------------------------------------------------------------------ lanes: run batches
    def _work(self, lane, idx: int) -> None:
        locks = (self.pipe.ar_locks[idx % self.pipe.ar_parts], self.pipe.bulk_lock) if self.pipe is not None else None
        with torch.cuda.stream(lane.model.stream):
            while True:
                batch = self._batches.get()
                if batch is None:
                    return
                if batch[0].stream is not None:
                    self._run_stream_batch(lane, batch, locks)
                    continue
                mf, top_p, temp, anti, ss, mg = batch[0].key
                try:
                    out = lane.synthesize_batch([""] * len(batch), [r.ref for r in batch], max_frames=mf, top_p=top_p, temperature=temp,
                                                anti_loop=anti, style_strength=ss, min_gen_frames=mg, text_ids=[r.text_ids for r in batch],
                                                phase_locks=locks, effects=[r.fx for r in batch])
                    self.stats["requests"] += len(batch)
                    self.stats["batches"] += 1
                    self.stats["rows"] += len(batch)
                    for r, w in zip(batch, out):
                        r.future.set_result(w)
                except BaseException as e:  # noqa: BLE001
                    for r in batch:
                        if not r.future.done():
                            r.future.set_exception(e)

    def _run_stream_batch(self, lane, batch: List[_Request], locks) -> None:
        _tag, mf, top_p, temp, anti, ss, mg, cf, trim, nar_ctx = batch[0].key
        sinks = [r.stream for r in batch]
        try:
            it = lane.stream_batch([""] * len(batch), [r.ref for r in batch], chunk_frames=cf, max_frames=mf, top_p=top_p, temperature=temp,
                                   anti_loop=anti, style_strength=ss, min_gen_frames=mg, seeds=[r.seed for r in batch], cache_trim=trim,
                                   nar_context_frames=nar_ctx, text_ids=[r.text_ids for r in batch], phase_locks=locks,
                                   alive=lambda b: not sinks[b].cancelled.is_set())
            self.stats["stream_batches"] += 1
            self.stats["requests"] += len(batch)
            self.stats["rows"] += len(batch)
            for step in it:
                for sink, c in zip(sinks, step):
                    if c is not None:
                        sink.put(c)
            for sink in sinks:
                sink.put(_StreamSink._END)
        except BaseException as e:  # noqa: BLE001
            for sink in sinks:
                sink.put(e)
