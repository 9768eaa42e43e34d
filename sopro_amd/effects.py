"""Post-decode effects: what ``speed=``, ``pitch=``, ``formant=``, ``silence=`` and ``watermark=`` do to a decoded waveform, and in
which order.

Every public entry point takes the five keywords; this module is the only place that knows what they mean together.

``speed``: speaking rate in [0.5, 2.0] (> 1: faster, shorter), pitch-preserving (``hip.time_stretch``, WSOLA).  ``pitch``: semitones in
[-12, 12]: every frequency is multiplied by rho = 2^(pitch / 12) and the duration stays what ``speed`` makes it: the stretch runs at
``speed / rho``, which must lie in [0.5, 2.0] too (``hip.prosody_step``), and a band-limited resampler then reads rho times as fast
(``hip.pitch_shift``).  ``formant``: semitones, where the spectral envelope sits relative to the decoded voice's; None (the default)
leaves it where ``pitch`` took it, 0.0 next to a ``pitch`` keeps the timbre, a value at ``pitch`` 0.0 makes the voice sound smaller
(> 0) or larger (< 0) at the same pitch.  The envelope is warped by sigma = 2^((formant - pitch) / 12), which must lie in [0.5, 2.0]
(``hip.formant_inv``, ``hip.formant_shift``); no sample moves.  ``silence``: a ``sopro_amd.Silence``: pauses longer than its cap are squeezed, the silent
lead-in and the tail are trimmed (``hip.silence_squeeze``).  ``watermark``: a ``sopro_amd.Watermark`` (key, tag, strength) added to the
waveform (``hip.wm_embed``; ``sopro_amd.watermark`` says what the mark survives).

The order is stretch -> resample -> warp -> squeeze -> mark.  The warp follows the resampler because it undoes what the resampler did
to the envelope, and precedes the squeeze so that the squeeze sees the levels that are heard.  The squeeze comes after rate and pitch
because its times are heard time, and before the mark because the mark does not survive interior cuts; the mark is last because it survives neither a stretch nor a
resample.  A keyword at its identity (1.0, 0.0, None or equal to ``pitch``, None, None) launches nothing, and a row at its identity inside a batch whose other
rows have work comes back bit for bit.  Chunked, every stage holds back what it cannot decide yet (the stretch whole 480-sample
blocks, the resampler the outputs whose taps are not in, the warp the 128-sample hops whose last frame is not in, the squeeze a pause until sound resumes - the silent lead-in never comes
out -, the mark up to 1440 samples whose envelope is not final) and a flush after the last chunk brings the rest: the concatenation
of a ``Chain``'s outputs is ``apply`` of the concatenated input, bit for bit, whatever the chunking.  Word cues follow the audio
through ``map_cues``: +-240 samples through the stretch (its search radius), +-240 / rho after the resampler, exact through the
squeeze (the operator's own cut table); the warp and the mark move no sample.

To add an effect: a field and its check in ``Effects``, a stage in ``apply`` and in ``Chain.of``, its wording in ``refuse``, and a
line in ``map_cues`` if it moves samples (the formant warp moves none, so it has no line there).  New fields go after the existing
ones, so that positional construction keeps its meaning.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, List, Optional, Sequence, Tuple

from . import hip
from .silence import Silence, check_silence
from .silence import per_row as _silences
from .watermark import Watermark, check_mark
from .watermark import per_row as _marks

STEP_ONE = hip.TSM_HS << 16  # the stretch's step at rate 1: nothing to do


@dataclass(frozen=True)
class Effects:
    """The five keywords of one row as given, validated, with the stretch's step, the resampler's increment and the warp's 1 / sigma
    they come to."""
    speed: Any = 1.0
    pitch: Any = 0.0
    silence: Optional[Silence] = None
    watermark: Optional[Watermark] = None
    formant: Any = None
    step: int = field(init=False)
    inc: int = field(init=False)
    inv: float = field(init=False)

    def __post_init__(self):
        step, inc = hip.prosody_step(self.speed, self.pitch)
        inv = hip.formant_inv(self.formant, self.pitch)
        check_silence(self.silence)
        check_mark(self.watermark)
        object.__setattr__(self, "step", step)
        object.__setattr__(self, "inc", inc)
        object.__setattr__(self, "inv", inv)

    @classmethod
    def of(cls, speed=1.0, pitch=0.0, silence=None, watermark=None, formant=None) -> "Effects":
        """``ValueError`` for a rate, a pitch, a formant or a pair of them out of range, ``TypeError`` for a ``silence`` or ``watermark`` of
        another type."""
        return cls(speed, pitch, silence, watermark, formant)

    @property
    def plain(self) -> bool:
        """No stage has anything to do."""
        return (self.step == STEP_ONE and self.inc == hip.PITCH_ONE and self.inv == hip.FORMANT_ONE and self.silence is None
                and self.watermark is None)


def per_row(speed, pitch, silence, watermark, rows: int, formant=None) -> List[Effects]:
    """One ``Effects`` per row of a batch from one value or one per row of each keyword (None entries allowed in the last three)."""
    return [Effects(*v) for v in zip(hip._per_row(speed, rows, "speed"), hip._per_row(pitch, rows, "pitch"), _silences(silence, rows),
                                     _marks(watermark, rows), hip._per_row(formant, rows, "formant"))]


def apply(wav, lens, fxs: Sequence[Effects]) -> Tuple[Any, List[int], Optional[List[list]]]:
    """The chain on a padded batch, on the current stream: ``wav`` fp32 [rows, >= max(lens)] on the device, ``lens`` valid samples per
    row, one ``Effects`` per row -> (wav, lens, cuts); ``cuts``: per row the (source position, samples removed) pairs of the squeeze,
    None when no row asked for one.  A stage at its identity for every row is not called; nothing here synchronises, and an all-plain
    batch comes back as it is."""
    cuts = None
    if any(fx.step != STEP_ONE or fx.inc != hip.PITCH_ONE for fx in fxs):
        wav, lens = hip.apply_prosody(wav, lens, [(fx.step, fx.inc) for fx in fxs])
    if any(fx.inv != hip.FORMANT_ONE for fx in fxs) and max(lens, default=0) > 0:
        wav = hip.formant_shift(wav, lens, [fx.inv for fx in fxs])
    if any(fx.silence is not None for fx in fxs):
        wav, lens, cuts = hip.silence_squeeze(wav, lens, [fx.silence for fx in fxs])
    if any(fx.watermark is not None for fx in fxs) and max(lens, default=0) > 0:  # (a squeeze may have left nothing to mark)
        wav = hip.wm_embed(wav, lens, [fx.watermark for fx in fxs])
    return wav, lens, cuts


class Chain:
    """The chain on one row that arrives in chunks: an ordered list of stages, each with ``feed(wav, flush=...) -> (out, lens)`` (the
    interface of ``hip.TimeStretchState``, ``PitchShiftState``, ``FormantState``, ``SilenceState`` and ``WatermarkState``)."""

    def __init__(self, stages: Sequence[Any]):
        self.stages = list(stages)

    @classmethod
    def of(cls, fx: Effects, device) -> "Chain":
        """The stages of ``fx`` that have work, in order."""
        stages: List[Any] = []
        if fx.step != STEP_ONE:
            stages.append(hip.TimeStretchState(1, None, device, steps=[fx.step]))
        if fx.inc != hip.PITCH_ONE:
            stages.append(hip.PitchShiftState(1, None, device, incs=[fx.inc]))
        if fx.inv != hip.FORMANT_ONE:
            stages.append(hip.FormantState(1, [fx.inv], device))
        if fx.silence is not None:
            stages.append(hip.SilenceState(1, fx.silence, device))
        if fx.watermark is not None:
            stages.append(hip.WatermarkState(1, fx.watermark, device))
        return cls(stages)

    def _run(self, wav, last: bool):
        for st in self.stages:
            if wav is None and not last:  # (a stage that yields nothing ends the step)
                break
            out, n = st.feed(wav, flush=last)
            wav = out[:, : n[0]] if n[0] > 0 else None
        return wav

    def feed(self, chunk):
        """A chunk [1, n] -> what the chain has ready of it, [1, m], or None.  None or an empty chunk launches nothing; a chain without
        stages hands the chunk back as it is."""
        if not self.stages:
            return chunk
        return self._run(chunk, False) if chunk is not None and chunk.numel() > 0 else None

    def flush(self):
        """After the last chunk: every stage is flushed in order, and what a stage's flush yields goes into the next stage's."""
        return self._run(None, True)


def map_cues(words, fx: Effects, cuts=None):
    """Word cues of the decoded row -> cues of what ``apply`` / a ``Chain`` made of it (``cuts``: the row's cut table, None without a
    squeeze)."""
    from . import align as A

    if fx.step != STEP_ONE:
        words = A.stretch_cues(words, fx.step)
    if fx.inc != hip.PITCH_ONE:
        words = A.shift_cues(words, fx.inc)
    if cuts is not None:
        words = A.squeeze_cues(words, cuts)
    return words


def refuse(what: str, *, speed=1.0, pitch=0.0, watermark=None, silence=None, formant=None) -> None:
    """The lockstep / frame-level paths have none of the five: anything off its identity is an error there, never ignored."""
    use = "use stream(), synthesize_batch() or SynthesisService.submit() in mode='batch'"
    if hip.tsm_step(speed) != STEP_ONE:
        raise NotImplementedError(f"{what} has no speaking-rate control (speed={speed!r}): {use}")
    if hip.pitch_inc(pitch) != hip.PITCH_ONE:
        raise NotImplementedError(f"{what} has no pitch control (pitch={pitch!r}): {use}")
    if hip.formant_inv(formant, pitch) != hip.FORMANT_ONE:
        raise NotImplementedError(f"{what} has no formant control (formant={formant!r}): {use}")
    if watermark is not None:
        raise NotImplementedError(f"{what} has no watermark (watermark={watermark!r}): {use}")
    if silence is not None:
        raise NotImplementedError(f"{what} has no silence control (silence={silence!r}): {use}")
