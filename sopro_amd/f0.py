"""Pitch tracking: what the fundamental frequency of a voice is, frame by frame (definition: include/sopro_hip.h "pitch tracking",
DESIGN.md "Pitch tracking"; numpy restatement: tests/f0_ref.py).

``PitchParams(threshold, floor_db, octave_cost, jump_cost, switch_cost, unvoiced_cost)`` is what ``params=`` of
``SoproTTS.pitch_track`` / ``SoproTTS.voice_pitch`` takes; ``PitchTrack`` is what they return.  One value per 10 ms frame over a 30 ms
window: YIN's normalised difference, up to four candidate lags per frame with integer costs, an integer Viterbi path with an unvoiced
state, a parabolic refinement.  The defaults were chosen on synthetic material with the numpy prototype; they are not tuned on real
speech.  The tracker is offline (it sees the whole row) and works at the codec rate, 24 kHz, only.

The hot path is the HIP kernels of ``csrc/f0.hip`` behind ``hip.f0_track``."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

SR = 24000
H, W, TMIN, TMAX, K = 240, 720, 48, 400, 4
SPAN = W + TMAX
CENTRE = SPAN // 2
COST_MAX, JUMP_MAX = 1024, 4096
THRESHOLD_DEFAULT, FLOOR_DEFAULT = 0.5, -50.0
OCTAVE_DEFAULT, JUMP_DEFAULT, SWITCH_DEFAULT, UNVOICED_DEFAULT = 24, 96, 160, 150


def frames_of(n: int) -> int:
    """Frames of a row of ``n`` samples."""
    n = int(n)
    return 0 if n < SPAN else (n - SPAN) // H + 1


def _number(name: str, v) -> float:
    if isinstance(v, bool):
        raise ValueError(f"PitchParams.{name} must be a number, got {v!r}")
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"PitchParams.{name} must be a number, got {v!r}") from None
    if not math.isfinite(f):
        raise ValueError(f"PitchParams.{name} must be finite, got {v!r}")
    return f


@dataclass(frozen=True)
class PitchParams:
    """``threshold``: a dip of the normalised difference below it is a candidate, (0, 1]; ``floor_db``: a frame whose mean power is
    not above it (dB re 1.0) has no candidate, -100 .. 0; ``octave_cost``: what a candidate an octave below the shortest lag costs
    more, an integer in 0 .. 1024 (1024 = one whole unit of the difference); ``jump_cost``: what an octave between consecutive frames
    costs, 0 .. 4096; ``switch_cost``: what a change between voiced and unvoiced costs, 0 .. 4096; ``unvoiced_cost``: what an
    unvoiced frame costs, 0 .. 1024."""
    threshold: float = THRESHOLD_DEFAULT
    floor_db: float = FLOOR_DEFAULT
    octave_cost: int = OCTAVE_DEFAULT
    jump_cost: int = JUMP_DEFAULT
    switch_cost: int = SWITCH_DEFAULT
    unvoiced_cost: int = UNVOICED_DEFAULT

    def __post_init__(self):
        for name in ("threshold", "floor_db"):
            object.__setattr__(self, name, _number(name, getattr(self, name)))
        for name, hi in (("octave_cost", COST_MAX), ("jump_cost", JUMP_MAX), ("switch_cost", JUMP_MAX), ("unvoiced_cost", COST_MAX)):
            w = _number(name, getattr(self, name))
            if w != int(w):
                raise ValueError(f"PitchParams.{name} must be an integer, got {getattr(self, name)!r}")
            if not 0 <= int(w) <= hi:
                raise ValueError(f"PitchParams.{name} must lie in [0, {hi}], got {getattr(self, name)!r}")
            object.__setattr__(self, name, int(w))
        if not 0.0 < self.threshold <= 1.0:
            raise ValueError(f"PitchParams.threshold must lie in (0, 1], got {self.threshold!r}")
        if not -100.0 <= self.floor_db <= 0.0:
            raise ValueError(f"PitchParams.floor_db must lie in [-100, 0] dB, got {self.floor_db!r}")

    def as_floats(self) -> Tuple[float, ...]:
        """The six values in the order the C entry points take them."""
        return (self.threshold, self.floor_db, float(self.octave_cost), float(self.jump_cost), float(self.switch_cost), float(self.unvoiced_cost))


def check_params(p, what: str = "params") -> PitchParams:
    """None means the defaults."""
    if p is None:
        return PitchParams()
    if not isinstance(p, PitchParams):
        raise TypeError(f"{what} must be a sopro_amd.PitchParams or None, got {type(p).__name__}")
    return p


def per_row(ps, rows: int, what: str = "params") -> List[PitchParams]:
    """One ``PitchParams`` per row from one ``PitchParams`` / None or a sequence of them."""
    if ps is None or isinstance(ps, PitchParams):
        return [check_params(ps, what)] * int(rows)
    if isinstance(ps, (str, bytes)) or not hasattr(ps, "__len__"):
        raise TypeError(f"{what} must be a sopro_amd.PitchParams, None or one of them per row, got {type(ps).__name__}")
    vals = [check_params(p, what) for p in ps]
    if len(vals) != int(rows):
        raise ValueError(f"{what}: one value or one per row ({rows}), got {len(vals)}")
    return vals


class PitchTrack:
    """The pitch of one row.  ``f0`` fp32 [F] in Hz, 0.0 = unvoiced, one value per 10 ms frame, and ``strength`` fp32 [F] (1 - the
    normalised difference at the chosen lag, 0.0 unvoiced) stay where the operator wrote them; ``centres`` [F] is the sample a frame
    describes, f * 240 + 560.  The summaries (``median_hz``, ``voiced_fraction``, ``span``) copy the F values to the host once."""

    def __init__(self, f0: torch.Tensor, strength: torch.Tensor):
        if f0.dim() != 1 or tuple(strength.shape) != tuple(f0.shape):
            raise ValueError(f"PitchTrack wants f0 [F] and strength [F], got {tuple(f0.shape)} and {tuple(strength.shape)}")
        self.f0, self.strength = f0, strength
        self._host: Optional[np.ndarray] = None

    def __len__(self) -> int:
        return int(self.f0.shape[0])

    @property
    def centres(self) -> torch.Tensor:
        return torch.arange(len(self), device=self.f0.device) * H + CENTRE

    def _f0_host(self) -> np.ndarray:
        if self._host is None:
            self._host = self.f0.detach().to("cpu", torch.float64).numpy()
        return self._host

    @staticmethod
    def _summary(hz: np.ndarray) -> Tuple[Optional[float], float]:
        voiced = hz[hz > 0]
        return (float(np.median(voiced)) if voiced.size else None, float(voiced.size) / hz.size if hz.size else 0.0)

    @property
    def median_hz(self) -> Optional[float]:
        """The median of the voiced frames; None if there is none."""
        return self._summary(self._f0_host())[0]

    @property
    def voiced_fraction(self) -> float:
        return self._summary(self._f0_host())[1]

    def span(self, a: int, b: int) -> Tuple[Optional[float], float]:
        """(median_hz or None, voiced_fraction) of the frames whose centre lies in [a, b): a ``WordCue``'s samples give a word's pitch."""
        lo = max(0, -(-(int(a) - CENTRE) // H))
        hi = min(len(self), max(lo, -(-(int(b) - CENTRE) // H)))
        return self._summary(self._f0_host()[lo:hi])

    def semitones_to(self, hz: float) -> float:
        """12 log2(hz / median_hz): what ``pitch=`` must be to bring this voice to ``hz``."""
        hz = float(hz)
        if not (math.isfinite(hz) and hz > 0):
            raise ValueError(f"semitones_to wants a positive frequency, got {hz!r}")
        m = self.median_hz
        if m is None:
            raise ValueError("semitones_to: the track has no voiced frame, so there is no pitch to move")
        return 12.0 * math.log2(hz / m)

    def __repr__(self) -> str:
        m = self.median_hz
        return f"PitchTrack(frames={len(self)}, median_hz={'None' if m is None else format(m, '.2f')}, voiced_fraction={self.voiced_fraction:.3f})"


def as_rows(wav, lens, device) -> Tuple[torch.Tensor, List[int], bool]:
    """What ``pitch_track`` accepts -> (fp32 [rows, cap] on ``device``, lens, batched): a waveform [N] / [1, N] / [1, 1, N] (numpy or
    tensor, any device) without ``lens``, or a padded [rows, cap] with one length per row."""
    t = torch.as_tensor(wav)
    if not t.is_floating_point():
        raise TypeError(f"pitch_track wants a floating-point waveform, got {t.dtype}")
    if lens is None:
        if t.dim() > 1 and any(int(s) != 1 for s in t.shape[:-1]):
            raise ValueError(f"pitch_track: a waveform [N] / [1, 1, N], or a padded [rows, cap] with lens=, got {tuple(t.shape)}")
        t = t.reshape(1, -1)
        return t.to(device, torch.float32), [int(t.shape[1])], False
    lens_h = [int(v) for v in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
    if t.dim() != 2 or int(t.shape[0]) != len(lens_h):
        raise ValueError(f"pitch_track: with lens= the waveforms are a padded [rows, cap] with one length per row, got {tuple(t.shape)} and {len(lens_h)}")
    if lens_h and (min(lens_h) < 0 or max(lens_h) > int(t.shape[1])):
        raise ValueError("pitch_track: lens must lie in [0, cap]")
    return t.to(device, torch.float32), lens_h, True
