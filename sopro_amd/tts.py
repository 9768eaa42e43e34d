"""``SoproTTS``: the drop-in public facade (reference: src/sopro/model.py:404-583).

Same constructor / method signatures and error behaviour as the reference class, so existing call
sites (``README.md:69-120``, ``src/sopro/cli.py``, ``demo/server.py:224,241``) keep working; the body
of every method runs on the MI355X engine (``sopro_amd.model`` / ``sopro_amd.codec``).  Additions
that the reference does not have: ``synthesize_batch``, ``stream_batch``, ``from_weights``, the long-form entry points
``synthesize_long`` / ``stream_long`` (text of any length: split, batched, joined on the device; ``sopro_amd.longform``) and
``synthesize_timed`` (word timestamps; ``sopro_amd.align``).
"""
from __future__ import annotations

import os
from typing import Any, Dict, Iterator, List, NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from .codec import MimiCodec
from .config import DEFAULT_MIMI_ID, TARGET_SR, MimiDecoderConfig, SoproTTSConfig
from .model import PreparedReference, SoproTTSModel
from .weights import load_cfg_from_safetensors, load_safetensors


class PaddedBatch(NamedTuple):
    """``synthesize_batch(..., padded=True)``: the decoder's batch where it is."""
    wav: torch.Tensor      # [B, T * 1920] fp32; row b is valid for lens[b] samples
    lens: List[int]        # samples
    tokens: torch.Tensor   # [B, T, Q] int64; row b is valid for frames[b] frames
    frames: Optional[List[int]] = None  # frames per row (lens[b] / 1920 unless a speaking rate stretched ``wav``)
    cuts: Optional[List[list]] = None   # with ``silence=``: per row the (source position, samples removed) pairs (``align.map_cuts``)


class SoproTTS:
    def __init__(self, model: SoproTTSModel, cfg: SoproTTSConfig, tokenizer: Any, codec: MimiCodec, device: str):
        self.model = model
        self.cfg = cfg
        self.tokenizer = tokenizer
        self.codec = codec
        self.device = torch.device(device)

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_pretrained(cls, repo_id: str, *, revision: Optional[str] = None, cache_dir: Optional[str] = None,
                        token: Optional[str] = None, device: Optional[str] = None, precision: str = "f32") -> "SoproTTS":
        """reference: src/sopro/model.py:419-451.  ``repo_id`` may also be a local directory holding
        ``model.safetensors`` (+ tokenizer files) and, for the codec, ``mimi/model.safetensors``.  ``precision`` (new):
        "f32" reproduces the fp32 reference; "bf16" runs the NAR / Mimi contractions with bf16 operands."""
        device = device or "cuda"
        if os.path.isdir(repo_id):
            local_dir = repo_id
        else:
            from huggingface_hub import snapshot_download  # reference: src/sopro/hub.py:15-27

            local_dir = snapshot_download(repo_id=repo_id, revision=revision, cache_dir=cache_dir, token=token)
        model_path = os.path.join(local_dir, "model.safetensors")
        if not os.path.exists(model_path):
            raise FileNotFoundError(f"Expected {model_path} in repo snapshot.")
        cfg = load_cfg_from_safetensors(model_path)
        weights = load_safetensors(model_path)
        tokenizer = _load_tokenizer(local_dir)
        mimi_dir = os.path.join(local_dir, "mimi")
        if os.path.exists(os.path.join(mimi_dir, "model.safetensors")):
            mimi_weights = load_safetensors(os.path.join(mimi_dir, "model.safetensors"))
        else:
            from huggingface_hub import snapshot_download

            mdir = snapshot_download(repo_id=DEFAULT_MIMI_ID, cache_dir=cache_dir, token=token)
            mimi_weights = load_safetensors(os.path.join(mdir, "model.safetensors"))
        return cls.from_weights(cfg, weights, mimi_weights, tokenizer, device=device, precision=precision)

    @classmethod
    def from_weights(cls, cfg: SoproTTSConfig, weights: Dict[str, np.ndarray], mimi_weights: Dict[str, np.ndarray],
                     tokenizer: Any, *, device: str = "cuda", seed: int = 0, use_graph: bool = True,
                     precision: str = "f32") -> "SoproTTS":
        """Build from in-memory checkpoints (reference ``state_dict`` names; HF Mimi names)."""
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        model = SoproTTSModel(cfg, weights, str(dev), seed=seed, use_graph=use_graph, precision=precision)
        codec = MimiCodec(mimi_weights, MimiDecoderConfig(num_quantizers=int(cfg.num_codebooks)), str(dev), precision=precision)
        return cls(model, cfg, tokenizer, codec, str(dev))

    # ------------------------------------------------------------------ reference API
    def encode_text(self, text: str) -> torch.Tensor:
        ids = self.tokenizer.encode(text)  # reference: src/sopro/model.py:453-455
        return torch.tensor(ids, dtype=torch.long)

    @torch.inference_mode()
    def encode_speaker(self, *, ref_audio_path: Optional[str] = None, ref_tokens_tq: Optional[torch.Tensor] = None,
                       ref_seconds: Optional[float] = None, denoise=None, report: Optional[list] = None, crop=None) -> torch.Tensor:
        """reference: src/sopro/model.py:457-475 -> the voice's speaker vector [sv_student_dim] (Token2SV over the cropped
        reference tokens; the same vector ``prepare_reference`` stores as ``sv_ref``).  ``denoise``, ``report``, ``crop``: as in
        ``encode_reference``."""
        ref = self.encode_reference(ref_audio_path=ref_audio_path, ref_tokens_tq=ref_tokens_tq, ref_seconds=ref_seconds, denoise=denoise,
                                    report=report, crop=crop)
        ref_btq = ref.unsqueeze(0)
        lengths = torch.tensor([int(ref_btq.size(1))], dtype=torch.long)
        return self.model.token2sv(ref_btq, lengths=lengths).squeeze(0).detach()

    @torch.inference_mode()
    def encode_reference(self, *, ref_audio_path: Optional[str] = None, ref_tokens_tq: Optional[torch.Tensor] = None,
                         ref_seconds: Optional[float] = None, denoise=None, report: Optional[list] = None, crop=None) -> torch.Tensor:
        """reference: src/sopro/model.py:477-514 (token path only; audio -> tokens needs the Mimi encoder).  ``denoise`` (new; a
        ``sopro_amd.Denoise``): the reference waveform goes through the stationary-noise suppressor before it is cropped and encoded
        (``MimiCodec.reference_waveform``); ``report``: a list used as a sink, it receives one ``DenoiseReport``.  With
        ``ref_tokens_tq`` there is no waveform: ``denoise`` other than None is refused.  ``crop`` (new; a ``sopro_amd.SpeechCrop``): the
        ``ref_seconds`` that are encoded are the window with the most speech and the least clipping (``hip.speech_crop``) instead of
        the centre crop, and ``report`` receives a ``CropReport`` (after the ``DenoiseReport``, if both are asked for); refused with
        ``ref_tokens_tq`` and with ``ref_seconds <= 0`` (no window to select)."""
        from . import crop as CR
        from . import denoise as D

        D.report_sink(report)
        D.refuse_without_waveform(denoise, "encode_reference", ref_tokens_tq=ref_tokens_tq)
        CR.refuse_without_waveform(crop, "encode_reference", ref_tokens_tq=ref_tokens_tq)
        if ref_tokens_tq is None and ref_audio_path is None:  # model.py:486-493
            raise RuntimeError("SoproTTS requires a reference. Provide ref_audio_path=... or ref_tokens_tq=...")
        if ref_tokens_tq is not None and ref_audio_path is not None:
            raise RuntimeError("Provide only one of ref_audio_path or ref_tokens_tq (not both).")
        if ref_seconds is None:
            ref_seconds = 12.0  # model.py:495-496
        CR.refuse_without_window(crop, "encode_reference", ref_seconds)
        if ref_tokens_tq is None:
            return self.codec.encode_file(ref_audio_path, crop_seconds=ref_seconds if ref_seconds > 0 else None, denoise=denoise, report=report, crop=crop)
        ref = ref_tokens_tq.long()
        if ref_seconds and ref_seconds > 0:
            fps = float(self.cfg.mimi_fps)
            win = max(1, int(round(ref_seconds * fps)))
            T = int(ref.shape[0])
            if T > win:  # center crop, reference: src/sopro/sampling.py:8-13
                s = (T - win) // 2
                ref = ref[s: s + win]
        return ref

    @torch.inference_mode()
    def prepare_reference(self, *, ref_audio_path: Optional[str] = None, ref_tokens_tq: Optional[torch.Tensor] = None,
                          ref_seconds: Optional[float] = None, denoise=None, report: Optional[list] = None, crop=None) -> PreparedReference:
        """reference: src/sopro/model.py:516-529.  ``denoise``, ``report``, ``crop`` (new): as in ``encode_reference``."""
        ref = self.encode_reference(ref_audio_path=ref_audio_path, ref_tokens_tq=ref_tokens_tq, ref_seconds=ref_seconds, denoise=denoise,
                                    report=report, crop=crop)
        return self.model.prepare_reference(ref)

    @torch.inference_mode()
    def synthesize(self, text: str, *, ref: Optional[PreparedReference] = None, ref_audio_path: Optional[str] = None,
                   ref_tokens_tq: Optional[torch.Tensor] = None, max_frames: int = 400, top_p: float = 0.9,
                   temperature: float = 1.05, anti_loop: bool = True, style_strength: Optional[float] = None,
                   ref_seconds: Optional[float] = None, min_gen_frames: Optional[int] = None,
                   seed: Optional[int] = None, speed: float = 1.0, pitch: float = 0.0, watermark=None,
                   silence=None, denoise=None, report: Optional[list] = None, crop=None, formant: Optional[float] = None,
                   similarity: Optional[list] = None) -> torch.Tensor:
        """reference: src/sopro/model.py:531-575 -> waveform [1, 1, N] on ``self.device``.  ``seed`` (new) pins the sampler's
        draws: the same seed, text and voice give the same audio; without it every call is a new take (the reference
        draws from torch's global generator; its CLI seeds that once, src/sopro/cli.py:72-75).  ``speed``, ``pitch``, ``formant``,
        ``silence``, ``watermark`` (new): applied to the decoded waveform, see ``sopro_amd.effects``; at their defaults nothing is launched.
        ``denoise``, ``report`` (new): the input side, forwarded to ``prepare_reference``; with ``ref`` or ``ref_tokens_tq`` there is
        no waveform to clean and ``denoise`` other than None is refused.  ``crop`` (new): which ``ref_seconds`` of the recording are
        encoded, forwarded likewise and refused likewise.  ``similarity`` (new): a sink like ``report`` - a list passed in receives
        one ``VoiceMatch``, the generated tokens' speaker vector against ``ref.sv_ref`` (see ``synthesize_batch``); ``None``: nothing
        is launched."""
        from . import crop as CR
        from . import denoise as D
        from . import effects
        from . import voicematch as VM

        VM.sink_of(similarity, "synthesize")
        fx = effects.Effects.of(speed, pitch, silence, watermark, formant)
        D.refuse_without_waveform(denoise, "synthesize", ref=ref, ref_tokens_tq=ref_tokens_tq)
        CR.refuse_without_waveform(crop, "synthesize", ref=ref, ref_tokens_tq=ref_tokens_tq)
        text_ids = self.encode_text(text)
        if ref is None:
            ref = self.prepare_reference(ref_audio_path=ref_audio_path, ref_tokens_tq=ref_tokens_tq, ref_seconds=ref_seconds, denoise=denoise,
                                         report=report, crop=crop)
        tokens = self.model.generate_tokens(
            text_ids, ref, max_frames=max_frames, top_p=top_p, temperature=temperature, anti_loop=anti_loop,
            style_strength=float(style_strength if style_strength is not None else self.cfg.style_strength),
            min_gen_frames=min_gen_frames, seed=seed)
        wav = self.codec.decode_full(tokens)
        if similarity is not None:
            with self.model.on_stream(bulk=True):
                similarity[:] = self._voice_matches(tokens.unsqueeze(0), [int(tokens.shape[0])], [ref])
        if wav.numel() == 0:
            return wav
        return effects.apply(wav.reshape(1, -1), [int(wav.shape[-1])], [fx])[0].reshape(1, 1, -1)

    @torch.inference_mode()
    def synthesize_batch(self, texts: Sequence[str], refs: Sequence[PreparedReference], *, max_frames: int = 400,
                         top_p: float = 0.9, temperature: float = 1.05, anti_loop: bool = True,
                         style_strength: Optional[float] = None, min_gen_frames: Optional[int] = None,
                         timings: Optional[Dict[str, float]] = None, text_ids: Optional[Sequence[torch.Tensor]] = None,
                         phase_locks: Optional[tuple] = None, seed: Optional[int] = None, nonces: Optional[Sequence[int]] = None,
                         row_ids: Optional[Sequence[int]] = None, padded: bool = False,
                         speed: Union[float, Sequence[float]] = 1.0, alignment: Optional[list] = None,
                         align_heads=None, pitch: Union[float, Sequence[float]] = 0.0,
                         watermark=None, silence=None, effects=None, formant=None,
                         similarity: Optional[list] = None) -> Union[List[torch.Tensor], "PaddedBatch"]:
        """New: B utterances in one pass (batched AR graph, NAR and Mimi decode) -> list of [1, 1, N_b].
        ``nonces`` / ``row_ids``: per-utterance sampler stream of a scheduler that coalesces requests (see model._ARRun).
        ``padded`` (opt-in, the long-form join's input): return the decoder's batch as it is instead of per-row slices - a
        ``PaddedBatch`` of ``wav`` [B, T * 1920], ``lens`` (valid samples per row) and ``tokens`` [B, T, Q] (a copy: the engine's
        own token matrix is overwritten by the next pass); the list above is ``[wav[b, :lens[b]].reshape(1, 1, -1)]``.
        ``speed``, ``pitch``, ``formant``, ``silence``, ``watermark``: one value or one per row each (None entries allowed in the last three), see
        ``sopro_amd.effects``; the decoder's padded batch goes through the chain on the bulk stream before it is sliced, so
        ``PaddedBatch.wav`` / ``lens`` are the finished rows and ``cuts`` their cut tables (None without ``silence``), while ``tokens``
        and ``frames`` stay what the model produced.
        ``alignment``: a sink like ``timings`` - a list passed in is filled with one ``align.Alignment`` per row (frame -> text
        position path, frame range per position, confidence; in frames, before any stretch) by a post-pass on the bulk stream
        (``model.align_batch``: the AR stack replayed over the generated tokens, ``hip.align_scores`` / ``hip.align_paths``);
        ``align_heads``: the (layer, head) pairs whose attention is averaged (default all 12).  ``None``: nothing is launched.
        ``effects`` (internal): the rows' ``effects.Effects`` as they are, instead of the five keywords.
        ``similarity``: a sink as well - a list passed in is filled with one ``VoiceMatch`` per row: the cosine between the speaker
        vector of the row's generated tokens ([frames, Q], over the row's own length; ``model.speaker_vectors``, every row as its own
        unpadded utterance) and that row's ``ref.sv_ref``, queued on the bulk stream behind the decoder (three launches for the
        batch, fp32 in both precision modes); a row without frames gives ``VoiceMatch(0.0, 0)``.  It reads tokens only: the
        waveforms are the same bits with and without it.  ``None``: nothing is launched and nothing is allocated.  What cosine
        means "same speaker" is for the caller to calibrate (``sopro_amd.voicematch``)."""
        import contextlib
        import time

        from . import effects as E
        from . import voicematch as VM

        VM.sink_of(similarity, "synthesize_batch")

        ids = list(text_ids) if text_ids is not None else [self.encode_text(t) for t in texts]
        # (a bad value is refused before anything runs)
        fxs = list(effects) if effects is not None else E.per_row(speed, pitch, silence, watermark, len(ids), formant)
        if len(fxs) != len(ids):
            raise ValueError(f"effects: one per row ({len(ids)}), got {len(fxs)}")
        if alignment is not None:
            self.model._align_heads(align_heads)  # (a bad selection is refused before anything runs)
        locks = tuple(phase_locks) if phase_locks is not None else ()
        ar_lock = locks[0] if len(locks) > 0 else contextlib.nullcontext()
        bulk_lock = locks[1] if len(locks) > 1 else contextlib.nullcontext()
        cond_gate = locks[2] if len(locks) > 2 else contextlib.nullcontext()  # (a pipeline: conditioning phases take turns in job order)
        ss = float(style_strength if style_strength is not None else self.cfg.style_strength)
        from .model import _PhaseTimer

        # Every phase runs with ITS stream as the current one: stray torch ops (slices, clamps, allocations) are then queued where
        # the phase's kernels are, and no phase ever waits on a stream another engine of a pipeline may be generating on.
        self.model.prep_stream.wait_stream(torch.cuda.current_stream(self.device))  # the caller's inputs
        # conditioning needs no generation slot: it overlaps with whatever the other engines are doing
        with cond_gate, torch.cuda.stream(self.model.prep_stream):
            ev = _PhaseTimer(self.model.prep_stream, timings)
            # the stages of a pass hand their results over IN PLACE (round 5): conditioning writes into the AR plan's buffer, the
            # refinement reads that buffer and the plan's token history, the decoder reads the refinement's token matrix and writes
            # into the tensor this call returns - no copy, fill or cast of the runtime's runs between the library's launch sequences
            plan = self.model.plan_for(ids, max_frames)
            prep = self.model.phase_cond(ids, refs, max_frames=max_frames, style_strength=ss, plan=plan)
            # the AR phase's own preparation (plan buffers, folded text operands) belongs here too: the generation slot then
            # only replays frames (it sat idle for 2-3.5 ms per phase while this ran inside it)
            run = self.model.ar_prepare(prep, top_p=top_p, temperature=temperature, anti_loop=anti_loop, min_gen_frames=min_gen_frames,
                                        seed=seed, nonces=nonces, row_ids=row_ids)
            ev.mark("cond")
        with ar_lock, torch.cuda.stream(self.model.stream):  # latency-bound phase: AR graph replay (a pipeline picks the stream with the lock)
            ev = _PhaseTimer(self.model.stream, timings)
            if timings is not None:
                timings["_ar_t0"] = time.perf_counter()
            state = self.model.phase_ar(ids, refs, max_frames=max_frames, top_p=top_p, temperature=temperature, anti_loop=anti_loop,
                                        style_strength=ss, min_gen_frames=min_gen_frames, ev=ev, prep=prep, seed=seed, run=run)
            if timings is not None:
                timings["_ar_t1"] = time.perf_counter()
        # (the AR phase ends with its token history on the host side of a stream sync: the next phase needs no stream wait)
        with bulk_lock, torch.cuda.stream(self.model.bulk_stream):  # throughput-bound phase: NAR refinement + Mimi decode
            t0 = time.perf_counter()
            if timings is not None:
                timings["_bulk_t0"] = t0
            # refinement and decoding are queued back to back on the one stream (no host round trip between them: the partition
            # does not idle while the host wakes up and issues the decoder); with phase timings on, the host syncs in between
            same = self.codec.stream is self.model.bulk_stream or self.codec.stream.cuda_stream == self.model.bulk_stream.cuda_stream
            fused = same
            evs = None
            if fused and timings is not None:  # phase times from device events (a host sync between the phases is what fusing removes)
                evs = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                evs[0].record(self.model.bulk_stream)
            full = self.model.phase_nar(state, full=True, sync=not fused, raw=fused)  # [B, Tn, Q]
            if evs is not None:
                evs[1].record(self.model.bulk_stream)
            t1 = time.perf_counter()
            lens = [int(n) for n in state["lens"]]
            B, Tn = int(full.shape[0]), int(full.shape[1])
            if max(lens) == 0:
                if alignment is not None:
                    alignment[:] = self.model.align_batch(state["prep"], state, heads=align_heads)
                if similarity is not None:
                    similarity[:] = VM.matches([0.0] * B, [0] * B)
                if padded:
                    return PaddedBatch(torch.zeros(B, 0, device=self.device), [0] * B, torch.zeros(B, 0, self.model.Q, dtype=torch.long, device=self.device), [0] * B)
                return [torch.zeros(1, 1, 0, device=self.device) for _ in range(B)]
            # The padded batch goes to the decoder as it is: the decoder is causal, so the (valid, meaningless) codes a row holds
            # past its own length never reach the samples that are returned.
            codes = full
            wav = self.codec.decode_batch(codes)  # causal decoder: padding frames never reach earlier samples
            if fused and self.model.nar_guard(redo=True):  # (decode_batch has synchronised the stream: the pass's range word is in)
                wav = self.codec.decode_batch(codes)  # the refinement was repeated on the six-pass operands: decode its tokens
            if timings is not None:
                if evs is not None:
                    evs[2].record(self.model.bulk_stream)
                    evs[2].synchronize()
                    timings["nar"] = timings.get("nar", 0.0) + evs[0].elapsed_time(evs[1]) * 1e-3
                    timings["mimi"] = timings.get("mimi", 0.0) + evs[1].elapsed_time(evs[2]) * 1e-3
                else:
                    timings["nar"] = timings.get("nar", 0.0) + (t1 - t0)
                    timings["mimi"] = timings.get("mimi", 0.0) + (time.perf_counter() - t1)
                timings["_bulk_t1"] = time.perf_counter()
            if alignment is not None:  # (queued behind the decoder on the bulk stream)
                alignment[:] = self.model.align_batch(state["prep"], state, heads=align_heads)
            if similarity is not None:  # (likewise; the tokens are the engine's own matrix, read before the next pass writes it)
                similarity[:] = self._voice_matches(codes, lens, refs)
            hop = int(self.codec.mc.frame_samples)
            wav, n_samples, cuts = E.apply(wav, [n * hop for n in lens], fxs)
            toks = None
            if padded:  # (the engine's own token matrix: copied before the next pass overwrites it, complete before any stream reads it)
                toks = codes.long()
            if padded or not all(fx.plain for fx in fxs):
                self.model.bulk_stream.synchronize()
        if padded:
            return PaddedBatch(wav, n_samples, toks, lens, cuts)
        return [wav[b, : n_samples[b]].reshape(1, 1, -1) for b in range(B)]

    @torch.inference_mode()
    def synthesize_timed(self, text: str, *, ref: Optional[PreparedReference] = None, ref_audio_path: Optional[str] = None,
                         ref_tokens_tq: Optional[torch.Tensor] = None, token_spans=None, align_heads=None, max_frames: int = 400,
                         top_p: float = 0.9, temperature: float = 1.05, anti_loop: bool = True, style_strength: Optional[float] = None,
                         ref_seconds: Optional[float] = None, min_gen_frames: Optional[int] = None, seed: Optional[int] = None,
                         speed: float = 1.0, pitch: float = 0.0, watermark=None, silence=None, denoise=None, report: Optional[list] = None, crop=None,
                         formant: Optional[float] = None):
        """New: ``synthesize`` with word timestamps -> ``align.TimedResult(wav, words, alignment)``.  ``wav`` is what ``synthesize``
        returns for the same arguments (same sampler stream, same launches: bit-identical for the same ``seed``); ``words`` holds one
        ``align.WordCue`` (text, character range, sample range in ``wav``) per whitespace-separated word; ``alignment`` the frame-level
        ``align.Alignment`` with its ``confidence``.  Cues are whole frames (1920 samples) and follow the audio through ``speed``,
        ``pitch`` and ``silence`` (``effects.map_cues`` has their accuracy); ``formant`` and the mark move no sample, so they move no cue.
        ``token_spans``: the character span
        of every id of ``encode_text(text)`` (a list, or a callable text -> list) for tokenizers without character offsets;
        ``align_heads``: the (layer, head) pairs to average, picked with tools/align_probe.py (default all 12).  ``denoise``,
        ``report``, ``crop``: as in ``synthesize``."""
        from . import align as A
        from . import crop as CR
        from . import denoise as D
        from . import effects

        fx = effects.Effects.of(speed, pitch, silence, watermark, formant)
        D.refuse_without_waveform(denoise, "synthesize_timed", ref=ref, ref_tokens_tq=ref_tokens_tq)
        CR.refuse_without_waveform(crop, "synthesize_timed", ref=ref, ref_tokens_tq=ref_tokens_tq)
        text_ids = self.encode_text(text)
        spans = token_spans(text) if callable(token_spans) else (list(token_spans) if token_spans is not None else A.token_spans(self.tokenizer, text))
        if len(spans) != int(text_ids.numel()):
            raise ValueError(f"token_spans: {len(spans)} spans for {int(text_ids.numel())} token ids")
        if ref is None:
            ref = self.prepare_reference(ref_audio_path=ref_audio_path, ref_tokens_tq=ref_tokens_tq, ref_seconds=ref_seconds, denoise=denoise,
                                         report=report, crop=crop)
        sink: list = []
        tokens = self.model.generate_tokens_batch(
            [text_ids], [ref], max_frames=max_frames, top_p=top_p, temperature=temperature, anti_loop=anti_loop,
            style_strength=float(style_strength if style_strength is not None else self.cfg.style_strength),
            min_gen_frames=min_gen_frames, seed=seed, alignment=sink, align_heads=align_heads)[0]
        wav = self.codec.decode_full(tokens)
        words = A.word_cues(text, spans, sink[0].token_frames, hop=int(self.codec.mc.frame_samples))
        if wav.numel() > 0:
            out, _, cuts = effects.apply(wav.reshape(1, -1), [int(wav.shape[-1])], [fx])
            wav = out.reshape(1, 1, -1)
            words = effects.map_cues(words, fx, cuts[0] if cuts is not None else None)
        return A.TimedResult(wav, words, sink[0])

    def clone_lane(self) -> "SoproTTS":
        """Another engine over the same device weights (own streams / scratch), for pipelining batches."""
        return SoproTTS(self.model.clone_lane(), self.cfg, self.tokenizer, self.codec.clone_lane(), str(self.device))

    def stream(self, text: str, *, speed: float = 1.0, pitch: float = 0.0, watermark=None, silence=None, formant: Optional[float] = None,
               **kwargs) -> Iterator[torch.Tensor]:
        """reference: src/sopro/model.py:577-580.  ``speed``, ``pitch``, ``formant``, ``silence``, ``watermark`` (new): every decoded chunk goes
        through the chunked chain of ``sopro_amd.effects`` and what is ready is yielded as [1, n] (with a watermark a chunk comes out
        up to 1440 samples short and the rest follows); the concatenation is ``synthesize``'s chain over the plain stream's
        concatenation, bit for bit (see streaming.SoproTTSStreamer.stream).  ``denoise=``, ``report=`` (keywords of
        ``prepare_reference``) clean the reference waveform, ``crop=`` selects its window; with ``ref`` or ``ref_tokens_tq`` ``denoise``
        and ``crop`` are refused here."""
        from .align import refuse_timing
        from .streaming import stream

        refuse_timing(kwargs, "stream")
        return stream(self, text, speed=speed, pitch=pitch, watermark=watermark, silence=silence, formant=formant, **kwargs)

    def stream_timed(self, text: str, *, lag_frames: int = 8, token_spans=None, align_heads=None, speed: float = 1.0, pitch: float = 0.0,
                     watermark=None, silence=None, chunk_frames: int = 6, formant: Optional[float] = None, **kwargs):
        """New: ``stream`` with word timestamps as the audio is generated -> an iterator of ``align.TimedChunk(wav, words, final,
        alignment)``.  The ``wav`` fields ([1, n], n may be 0) concatenate to what ``stream`` yields for the same arguments and
        ``seed``, bit for bit; ``words`` holds an ``align.WordCue`` for every word the step closed, in text order, samples on the
        timeline of the concatenated output (through ``speed`` and ``pitch`` with ``synthesize_timed``'s accuracy; ``formant`` and the
        mark move no cue).  A cue is final when it is yielded: the online aligner (``hip.align_online``) commits a frame once ``lag_frames``
        later frames are in (default 8, 640 ms: a guess until a trained checkpoint is probed with tools/align_probe.py) and never
        revises it, so a word is reported about ``lag_frames`` frames after its last frame was generated.  The last item has
        ``final=True``, the remaining words and the ``align.Alignment`` (``status`` 2: the audio ended before the path reached the last
        text position; the words left over get empty cues at the end).  ``token_spans`` / ``align_heads``: as in ``synthesize_timed``.
        ``silence=`` is refused, and so is ``lag_frames + chunk_frames > 63``; other keywords are ``stream``'s (``denoise=``,
        ``crop=`` and ``report=`` among them)."""
        from .streaming import stream_timed

        return stream_timed(self, text, lag_frames=lag_frames, token_spans=token_spans, align_heads=align_heads, speed=speed, pitch=pitch,
                            watermark=watermark, silence=silence, chunk_frames=chunk_frames, formant=formant, **kwargs)

    def stream_batch(self, texts: Sequence[str], refs: Sequence[PreparedReference], *, chunk_frames: int = 6, max_frames: int = 400,
                     top_p: float = 0.9, temperature: float = 1.05, anti_loop: bool = True, style_strength: Optional[float] = None,
                     min_gen_frames: Optional[int] = None, seeds: Optional[Sequence[Optional[int]]] = None, cache_trim: str = "none",
                     nar_context_frames: Optional[int] = None, text_ids: Optional[Sequence[torch.Tensor]] = None,
                     speed: float = 1.0, pitch: float = 0.0, watermark=None, silence=None, formant: Optional[float] = None,
                     **kwargs) -> Iterator[List[Optional[torch.Tensor]]]:
        """New: B streams in lockstep (one batched AR run, refinement and stream decode per chunk).  Yields per step a list of B
        entries, a [1, n * 1920] chunk or None; row b's chunks are what ``stream`` yields for it (see streaming.stream_batch).
        None of the five effects is available here (``speed`` other than 1.0, ``pitch`` other than 0.0, a ``formant`` other than None
        or ``pitch``, ``watermark`` or ``silence`` other than None raises): use ``stream`` or ``synthesize_batch``."""
        from . import effects
        from .align import refuse_timing
        from .streaming import stream_batch

        refuse_timing(kwargs, "stream_batch")
        effects.refuse("stream_batch", speed=speed, pitch=pitch, watermark=watermark, silence=silence, formant=formant)
        return stream_batch(self, texts, refs, chunk_frames=chunk_frames, max_frames=max_frames, top_p=top_p, temperature=temperature,
                            anti_loop=anti_loop, style_strength=style_strength, min_gen_frames=min_gen_frames, seeds=seeds,
                            cache_trim=cache_trim, nar_context_frames=nar_context_frames, text_ids=text_ids, speed=speed, pitch=pitch,
                            **kwargs)

    def synthesize_long(self, text: str, *, speed: float = 1.0, pitch: float = 0.0, watermark=None, silence=None,
                        formant: Optional[float] = None, **kwargs):
        """New: a text of any length (a paragraph, an article, a chapter) -> ``LongformResult``: ``wav`` [1, 1, N] on the device and
        ``segments`` [(text, start sample, end sample)] in it.  The text is cut into sentences (``longform.split_text``,
        ``max_chars``), the voice is prepared once, groups of up to ``max_rows`` segments (``plan``: "throughput", "latency" or a
        list of group sizes) run through ``synthesize_batch``, and each group's padded decoder batch is joined on the device
        (``hip.join_segments``): silence below ``trim_db`` of a segment's peak is trimmed to ``keep_ms`` around the speech
        (``trim_db=None``: nothing is trimmed), pauses follow the kind of boundary (``pauses_ms``), cuts get ``fade_ms`` raised-cosine
        fades.  ``max_frames`` and the sampling parameters are per segment, as in ``synthesize``; segment k draws as
        ``synthesize(segment_k, ref=ref, seed=seed + k)`` does.  ``keep_parts=True`` also returns every segment's untrimmed
        waveform and tokens (``parts``) and the kept range (``edges``).  ``word_cues=True`` also fills ``words`` (one
        ``align.LongWordCue`` per word, samples in the joined waveform).  ``speed``, ``pitch``, ``formant``, ``silence`` (``sopro_amd.effects``): every group's padded batch goes through them
        before the join, so ``parts`` are the finished rows, cue times refer to the audio as it is heard and the pauses the join puts
        between sentences are untouched by the squeeze; the pauses are divided by ``speed`` and not touched by ``pitch``.
        ``watermark``: the batches run unmarked and the joined waveform is marked in one launch, so the carrier's phase is continuous
        across the segments (``parts`` stay unmarked).  ``voice_match=True`` also fills ``voice``: one ``VoiceMatch`` per entry of
        ``segments`` (the segment's generated tokens against the voice's ``sv_ref``, see ``voice_similarity``).  Full parameter list:
        ``longform.synthesize_long`` (``denoise=``, ``crop=`` and ``report=`` among them: the input side, as in ``synthesize``)."""
        from .longform import synthesize_long

        return synthesize_long(self, text, speed=speed, pitch=pitch, watermark=watermark, silence=silence, formant=formant, **kwargs)

    def stream_long(self, text: str, *, speed: float = 1.0, pitch: float = 0.0, watermark=None, silence=None, formant: Optional[float] = None,
                    **kwargs) -> Iterator[torch.Tensor]:
        """New: ``synthesize_long`` as a generator: runs group g of the plan ("latency" by default: 1, 2, 4, ... segments), joins it,
        yields the joined piece [1, n] (its trailing pause included), then runs group g + 1.  The join has no overlap between
        segments, so the pieces concatenate to ``synthesize_long(..., plan="latency").wav`` bit for bit (at any ``speed``, ``pitch`` and
        ``formant``).
        ``watermark``: the pieces go through one chunked mark (a piece comes out up to 1440 samples short, the rest follows,
        and a last piece carries the flush); they concatenate to ``synthesize_long(..., plan="latency", watermark=...).wav`` bit for bit.
        ``silence``: every group's batch is squeezed before its join, as in ``synthesize_long``."""
        from .align import refuse_timing
        from .crop import refuse_without_waveform as crop_refuse_without_waveform
        from .denoise import refuse_without_waveform
        from .effects import Effects
        from .longform import stream_long

        refuse_timing(kwargs, "stream_long")
        Effects.of(speed, pitch, silence, watermark, formant)  # (refused here, not at the first piece)
        refuse_without_waveform(kwargs.get("denoise"), "stream_long", ref=kwargs.get("ref"), ref_tokens_tq=kwargs.get("ref_tokens_tq"))
        crop_refuse_without_waveform(kwargs.get("crop"), "stream_long", ref=kwargs.get("ref"), ref_tokens_tq=kwargs.get("ref_tokens_tq"))
        return stream_long(self, text, speed=speed, pitch=pitch, watermark=watermark, silence=silence, formant=formant, **kwargs)

    def detect_watermark(self, wav, key: int):
        """New: does ``wav`` carry the mark of ``key``?  -> ``watermark.WatermarkResult(present, score, tag, offset, z_sync, z_tag)``,
        or a list of them for a list of clips (``watermark.detect`` on this engine's device)."""
        from .watermark import detect

        return detect(wav, key, device=self.device)

    @torch.inference_mode()
    def pitch_track(self, wav, *, lens=None, params=None):
        """New: the pitch of a waveform -> ``f0.PitchTrack`` (``f0`` in Hz per 10 ms frame with 0.0 = unvoiced, ``strength``,
        ``centres``, ``median_hz``, ``voiced_fraction``, ``span``, ``semitones_to``).  ``wav``: [N] / [1, N] / [1, 1, N] on any device
        (what ``synthesize`` returns), read as 24 kHz, the codec's rate and the only one supported; or a padded [rows, cap] with
        ``lens=[...]`` -> a list of ``PitchTrack``, one per row.  ``params``: a ``sopro_amd.PitchParams`` (None: the defaults), or one
        per row.  Runs on the bulk stream (``hip.f0_track``: the YIN difference, the candidate pick and an integer Viterbi path in
        HIP) and synchronises it, so the track is ready when the call returns.  An offline analysis: it changes no audio."""
        from . import f0 as F0
        from . import hip

        rows, lens_h, batched = F0.as_rows(wav, lens, self.device)
        ps = F0.per_row(params, len(lens_h), "params")
        if not lens_h:
            return []
        with self.model.on_stream(bulk=True):
            hz, st, _nv, frames = hip.f0_track(rows, lens_h, ps)
        self.model.bulk_stream.synchronize()
        tracks = [F0.PitchTrack(hz[b, :n], st[b, :n]) for b, n in enumerate(frames)]
        return tracks if batched else tracks[0]

    @torch.inference_mode()
    def voice_pitch(self, *, ref_audio_path: str, denoise=None, crop=None, ref_seconds: Optional[float] = None, params=None):
        """New: the pitch of a reference voice -> the ``f0.PitchTrack`` of exactly the waveform the encoder would see for the same
        arguments of ``prepare_reference`` (``MimiCodec.reference_waveform``: load, energy trim, resample, ``denoise``, the crop to
        ``ref_seconds``, 12 s by default, at the centre or by ``crop``).  ``vp.semitones_to(110.0)`` is the ``pitch=`` that brings the
        voice's median to 110 Hz."""
        from . import crop as CR

        if ref_seconds is None:
            ref_seconds = 12.0
        CR.refuse_without_window(crop, "voice_pitch", ref_seconds)
        x = self.codec.reference_waveform(ref_audio_path, crop_seconds=ref_seconds if ref_seconds > 0 else None, denoise=denoise, crop=crop)
        return self.pitch_track(x, params=params)

    # ------------------------------------------------------------------ voice similarity (sopro_amd.voicematch)
    def _voice_matches(self, tokens_btq: torch.Tensor, lens: Sequence[int], refs: Sequence[PreparedReference]) -> list:
        """One ``VoiceMatch`` per row of a padded token batch against one reference per row, on the CURRENT stream (three launches
        and one copy of B floats to the host, which waits for them)."""
        from . import hip
        from . import voicematch as VM

        lens = [int(n) for n in lens]
        if len(refs) != len(lens):
            raise ValueError(f"one reference per row ({len(lens)}), got {len(refs)}")
        if int(tokens_btq.shape[1]) == 0 or max(lens) == 0:
            return VM.matches([0.0] * len(lens), [0] * len(lens))
        sv = self.model.speaker_vectors(tokens_btq, lens)
        if all(r is refs[0] for r in refs):
            ref_m = refs[0].sv_ref.to(self.device, torch.float32).reshape(1, -1).expand(len(lens), -1).contiguous()
        else:
            ref_m = torch.cat([r.sv_ref.to(self.device, torch.float32).reshape(1, -1) for r in refs], dim=0).contiguous()
        return VM.matches(hip.spk_cosine(sv, ref_m).tolist(), lens)

    def _voice_rows(self, what: str, wav, tokens, lens):
        """``wav=`` (one 24 kHz clip, encoded by ``codec.encode_waveform``) or ``tokens=`` (+ ``lens=``) -> (tokens [B, T, Q], lens on
        the host, batched)."""
        from . import voicematch as VM

        if (wav is None) == (tokens is None):
            raise ValueError(f"{what} wants wav=... or tokens=... (one of them)")
        if tokens is not None:
            return VM.token_rows(tokens, lens, self.model.Q)
        if lens is not None:
            raise ValueError(f"{what}: lens= goes with tokens=")
        if not isinstance(wav, torch.Tensor) or not wav.is_floating_point() or wav.numel() == 0 or wav.numel() != int(wav.shape[-1]):
            raise ValueError(f"{what}: wav must be one floating-point clip [N], [1, N] or [1, 1, N] with N >= 1 (24 kHz)")
        codes = self.codec.encode_waveform(wav.reshape(-1))
        return codes.unsqueeze(0), [int(codes.shape[0])], False

    @torch.inference_mode()
    def speaker_vectors(self, *, tokens: Optional[torch.Tensor] = None, lens=None, wav: Optional[torch.Tensor] = None) -> torch.Tensor:
        """New: unit speaker vectors -> fp32 [B, sv_student_dim] on the device (a row without frames: zeros).  ``tokens``: codec tokens
        [T, Q] or a padded batch [B, T, Q] with ``lens`` (valid frames per row; default T); or ``wav``: one 24 kHz clip ([N] / [1, N] /
        [1, 1, N], what ``synthesize`` returns), encoded by the Mimi encoder first.  Every row is the model's Token2SV of its own
        frames as an unpadded utterance - what ``encode_speaker`` gives for them one voice at a time - in two launches for the whole
        batch on the bulk stream, which is synchronised before the call returns.  fp32 in both precision modes."""
        t, lens_h, _ = self._voice_rows("speaker_vectors", wav, tokens, lens)
        with self.model.on_stream(bulk=True):
            sv = self.model.speaker_vectors(t, lens_h)
        self.model.bulk_stream.synchronize()
        return sv

    @torch.inference_mode()
    def voice_similarity(self, *, ref, wav: Optional[torch.Tensor] = None, tokens: Optional[torch.Tensor] = None, lens=None):
        """New: did this take keep the voice?  -> ``VoiceMatch(cosine, frames)``: the cosine between the clip's speaker vector and
        ``ref.sv_ref``.  The clip is ``wav`` (one 24 kHz clip, encoded first) or ``tokens`` [T, Q]; a padded batch ``tokens`` [B, T, Q]
        with ``lens`` gives a list, one ``VoiceMatch`` per row, against ``ref`` (one ``PreparedReference`` for every row, or a
        sequence with one per row).  Runs on the bulk stream and waits for the result.  There is no threshold here: what cosine
        means "same speaker" depends on the checkpoint (``sopro_amd.voicematch``)."""
        t, lens_h, batched = self._voice_rows("voice_similarity", wav, tokens, lens)
        refs = list(ref) if isinstance(ref, (list, tuple)) else [ref] * len(lens_h)
        if not all(isinstance(r, PreparedReference) for r in refs):
            raise TypeError("voice_similarity(ref=...) wants a PreparedReference (or one per row)")
        with self.model.on_stream(bulk=True):
            out = self._voice_matches(t, lens_h, refs)
        return out if batched else out[0]

    @torch.inference_mode()
    def identify_voice(self, *, voices, wav: Optional[torch.Tensor] = None, tokens: Optional[torch.Tensor] = None, top: int = 5) -> list:
        """New: which of my stored voices is this clip?  -> the ``top`` best ``VoiceHit(index, name, cosine)``, best first (equal
        cosines: the lower index first).  ``voices``: a ``VoiceBank`` (build it once and keep it) or a sequence of
        ``PreparedReference``; the clip is ``wav`` (one 24 kHz clip) or ``tokens`` [T, Q].  One Token2SV pass and one bank cosine
        launch on the bulk stream; the ranking is done on the host.  No threshold: the best hit of a clip whose voice is not in the
        bank is still a hit."""
        from . import hip
        from . import voicematch as VM

        top = VM.check_top(top)
        bank = VM.as_bank(voices)
        t, lens_h, batched = self._voice_rows("identify_voice", wav, tokens, None)
        if batched:
            raise ValueError("identify_voice: one clip at a time (tokens [T, Q])")
        if bank.dim != int(self.cfg.sv_student_dim):
            raise ValueError(f"identify_voice: the bank's vectors have {bank.dim} elements, this model's {int(self.cfg.sv_student_dim)}")
        if lens_h[0] == 0:
            raise ValueError("identify_voice: the clip has no frames")
        with self.model.on_stream(bulk=True):
            sv = self.model.speaker_vectors(t, lens_h)
            cos = hip.spk_cosine(sv, bank.on(self.device), bank=True)[0].tolist()
        return VM.rank(cos, bank.names, top)

    def save_wav(self, path: str, wav: torch.Tensor) -> None:
        """reference: src/sopro/model.py:582-583 (16-bit PCM via the stdlib; soundfile is not required)."""
        import wave

        x = wav.detach().reshape(-1).float().clamp(-1.0, 1.0).cpu().numpy()
        pcm = (x * 32767.0).astype("<i2")
        with wave.open(path, "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(TARGET_SR)
            f.writeframes(pcm.tobytes())


def _load_tokenizer(local_dir: str):
    """reference: src/sopro/tokenizer.py:15-38 (HF AutoTokenizer + BOS/EOS)."""
    from transformers import AutoTokenizer

    class TextTokenizer:
        def __init__(self, d: str):
            self.tok = AutoTokenizer.from_pretrained(d, use_fast=True)
            if self.tok.pad_token_id is None:
                self.tok.add_special_tokens({"pad_token": "<|pad|>"})
            self.bos_id = int(self.tok.bos_token_id) if self.tok.bos_token_id is not None else None
            self.eos_id = int(self.tok.eos_token_id) if self.tok.eos_token_id is not None else None
            self.vocab_size = int(self.tok.vocab_size + len(self.tok.get_added_vocab()))

        def encode(self, text: str) -> List[int]:
            ids = self.tok.encode(text, add_special_tokens=False)
            if self.bos_id is not None and self.eos_id is not None:
                ids = [self.bos_id] + ids + [self.eos_id]
            return ids

    return TextTokenizer(local_dir)
