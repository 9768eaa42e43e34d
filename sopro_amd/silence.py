"""Silence control: how much of a take is dead air (definition: include/sopro_hip.h "silence control", DESIGN.md "Silence control";
numpy restatement: tests/sil_ref.py).

``Silence(max_pause_ms, onset_ms, floor_db, floor)`` is what the public ``silence=`` keyword takes: no pause longer than
``max_pause_ms`` is left in, the take starts ``onset_ms`` before its first sound and ends ``max_pause_ms - onset_ms`` after its last.
Sound is anything whose 10 ms hop reaches the floor, an absolute amplitude (``floor_db`` re full scale 1.0, or ``floor`` as a
linear amplitude); a peak-relative floor is not offered, because a streamed take cannot know its own peak and one definition serves
both forms.  The operator runs after rate and pitch, so the times are heard time, and before the watermark.

The device sees only integers and a threshold; the hot path is the HIP kernels of ``csrc/sil.hip`` behind ``hip.silence_squeeze``
and ``hip.SilenceState``."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

HOP = 240
HOP_MS = 10.0
B_MAX, CAP_MAX = 16, 1000


def _number(name: str, v) -> float:
    if isinstance(v, bool):
        raise ValueError(f"Silence.{name} must be a number, got {v!r}")
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"Silence.{name} must be a number, got {v!r}") from None
    if not math.isfinite(f):
        raise ValueError(f"Silence.{name} must be finite, got {v!r}")
    return f


@dataclass(frozen=True)
class Silence:
    """``max_pause_ms``: the longest pause left in (and, less ``onset_ms``, the tail kept after the last sound); ``onset_ms``: what is
    kept before a sound resumes; both are rounded to 10 ms hops, ``1 <= onset <= 16`` hops and ``onset + 1 <= max_pause <= 1000``
    hops.  ``floor_db``: the level below which a hop is silent, dB re 1.0; ``floor``: the same as a linear amplitude (overrides
    ``floor_db``)."""
    max_pause_ms: float = 300.0
    onset_ms: float = 30.0
    floor_db: float = -40.0
    floor: Optional[float] = None

    def __post_init__(self):
        for name in ("max_pause_ms", "onset_ms", "floor_db"):
            object.__setattr__(self, name, _number(name, getattr(self, name)))
        if self.floor is not None:
            object.__setattr__(self, "floor", _number("floor", self.floor))
        b, cap = self.onset_hops, self.cap_hops
        if not 1 <= b <= B_MAX:
            raise ValueError(f"Silence.onset_ms must round to 1 .. {B_MAX} hops of {HOP_MS:g} ms, got {self.onset_ms!r}")
        if not b + 1 <= cap <= CAP_MAX:
            raise ValueError(f"Silence.max_pause_ms must round to onset + 1 .. {CAP_MAX} hops of {HOP_MS:g} ms, got {self.max_pause_ms!r} "
                             f"(onset {b} hops)")
        t = self.thr
        if not (t > 0.0 and math.isfinite(t)):
            raise ValueError(f"Silence: the floor must be a positive fp32 amplitude, got floor_db={self.floor_db!r}, floor={self.floor!r}")

    @property
    def cap_hops(self) -> int:
        return int(round(self.max_pause_ms / HOP_MS))

    @property
    def onset_hops(self) -> int:
        return int(round(self.onset_ms / HOP_MS))

    @property
    def thr(self) -> float:
        """fl32(floor), or fl32(10^(floor_db / 20)) from float64: all the device sees of a floor."""
        try:
            v = self.floor if self.floor is not None else 10.0 ** (self.floor_db / 20.0)
        except OverflowError:
            v = math.inf
        with np.errstate(over="ignore"):
            return float(np.float32(v))


def check_silence(sil, what: str = "silence") -> Optional[Silence]:
    if sil is not None and not isinstance(sil, Silence):
        raise TypeError(f"{what} must be a sopro_amd.Silence or None, got {type(sil).__name__}")
    return sil


def per_row(sils, rows: int, what: str = "silence") -> List[Optional[Silence]]:
    """One ``Silence`` (or None) per row from one ``Silence`` / None or a sequence of them."""
    if sils is None or isinstance(sils, Silence):
        return [sils] * int(rows)
    if isinstance(sils, (str, bytes)) or not hasattr(sils, "__len__"):
        raise TypeError(f"{what} must be a sopro_amd.Silence, None or one of them per row, got {type(sils).__name__}")
    vals = [check_silence(s, what) for s in sils]
    if len(vals) != int(rows):
        raise ValueError(f"{what}: one value or one per row ({rows}), got {len(vals)}")
    return vals
