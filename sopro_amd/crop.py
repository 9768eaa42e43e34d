"""Reference crop selection: which ``ref_seconds`` of a recording the voice is cloned from (definition: include/sopro_hip.h
"reference crop selection", DESIGN.md "Reference crop selection"; numpy restatement: tests/crop_ref.py).

``SpeechCrop(range_db, margin_db, clip_level, clip_weight)`` is what the public ``crop=`` keyword takes.  A 10 ms block counts as
speech when its energy is within ``range_db`` of the loudest block and ``margin_db`` above the 50 ms-smoothed floor; a block with a
sample at or above ``clip_level`` is clipped and costs ``clip_weight`` speech blocks.  The window with the largest score replaces the
centre crop; on a tie the window nearest the centre wins, so a recording the search has no preference on gets the centre crop
itself.  All four defaults and the 50 ms smoothing are choices, not measurements on real recordings.

The step acts on the input side only: load -> energy trim -> resample -> denoise -> crop -> encode
(``MimiCodec.reference_waveform``).  With ``ref_tokens_tq=`` or ``ref=`` there is no waveform, and ``crop=`` is refused; so it is
with no window (``ref_seconds <= 0``).  The hot path is the HIP kernels of ``csrc/crop.hip`` behind ``hip.speech_crop``."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, NamedTuple, Optional

RANGE_MIN, RANGE_MAX, RANGE_DEFAULT = 6.0, 80.0, 30.0
MARGIN_MIN, MARGIN_MAX, MARGIN_DEFAULT = 0.0, 40.0, 10.0
LEVEL_MAX, LEVEL_DEFAULT = 8.0, 0.999
WEIGHT_MAX, WEIGHT_DEFAULT = 64, 4


def _number(name: str, v) -> float:
    if isinstance(v, bool):
        raise ValueError(f"SpeechCrop.{name} must be a number, got {v!r}")
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"SpeechCrop.{name} must be a number, got {v!r}") from None
    if not math.isfinite(f):
        raise ValueError(f"SpeechCrop.{name} must be finite, got {v!r}")
    return f


@dataclass(frozen=True)
class SpeechCrop:
    """``range_db``: how far below the loudest block a block still counts as speech, 6 .. 80 dB; ``margin_db``: how far above the
    smoothed floor it must lie, 0 .. 40 dB; ``clip_level``: the amplitude from which a sample counts as clipped, (0, 8];
    ``clip_weight``: the speech blocks a clipped block costs, an integer in 0 .. 64 (0: clipping is ignored)."""
    range_db: float = RANGE_DEFAULT
    margin_db: float = MARGIN_DEFAULT
    clip_level: float = LEVEL_DEFAULT
    clip_weight: int = WEIGHT_DEFAULT

    def __post_init__(self):
        for name in ("range_db", "margin_db", "clip_level"):
            object.__setattr__(self, name, _number(name, getattr(self, name)))
        w = _number("clip_weight", self.clip_weight)
        if w != int(w):
            raise ValueError(f"SpeechCrop.clip_weight must be an integer, got {self.clip_weight!r}")
        object.__setattr__(self, "clip_weight", int(w))
        if not RANGE_MIN <= self.range_db <= RANGE_MAX:
            raise ValueError(f"SpeechCrop.range_db must lie in [{RANGE_MIN:g}, {RANGE_MAX:g}] dB, got {self.range_db!r}")
        if not MARGIN_MIN <= self.margin_db <= MARGIN_MAX:
            raise ValueError(f"SpeechCrop.margin_db must lie in [{MARGIN_MIN:g}, {MARGIN_MAX:g}] dB, got {self.margin_db!r}")
        if not 0.0 < self.clip_level <= LEVEL_MAX:
            raise ValueError(f"SpeechCrop.clip_level must lie in (0, {LEVEL_MAX:g}], got {self.clip_level!r}")
        if not 0 <= self.clip_weight <= WEIGHT_MAX:
            raise ValueError(f"SpeechCrop.clip_weight must lie in [0, {WEIGHT_MAX}], got {self.clip_weight!r}")


class CropReport(NamedTuple):
    """What the search saw on a row: ``start`` the first sample of the chosen window, ``active`` / ``clipped`` its speech and clipped
    blocks (10 ms each), ``centre_active`` / ``centre_clipped`` the same for the centre crop it replaces, ``row_active`` the speech
    blocks of the whole row, ``blocks`` the blocks of the row, ``level_db`` the chosen window's mean power (dB re 1.0)."""
    start: int
    active: int
    clipped: int
    centre_active: int
    centre_clipped: int
    row_active: int
    blocks: int
    level_db: float


def check_crop(cr, what: str = "crop") -> Optional[SpeechCrop]:
    if cr is not None and not isinstance(cr, SpeechCrop):
        raise TypeError(f"{what} must be a sopro_amd.SpeechCrop or None, got {type(cr).__name__}")
    return cr


def per_row(crs, rows: int, what: str = "crop") -> List[Optional[SpeechCrop]]:
    """One ``SpeechCrop`` (or None) per row from one ``SpeechCrop`` / None or a sequence of them."""
    if crs is None or isinstance(crs, SpeechCrop):
        return [crs] * int(rows)
    if isinstance(crs, (str, bytes)) or not hasattr(crs, "__len__"):
        raise TypeError(f"{what} must be a sopro_amd.SpeechCrop, None or one of them per row, got {type(crs).__name__}")
    vals = [check_crop(c, what) for c in crs]
    if len(vals) != int(rows):
        raise ValueError(f"{what}: one value or one per row ({rows}), got {len(vals)}")
    return vals


def refuse_without_waveform(cr, what: str, **given) -> None:
    """``crop=`` needs a waveform: with reference tokens or a prepared reference (the keywords of ``given`` that are not None)
    there is none, and the request is refused instead of ignored."""
    if check_crop(cr) is None:
        return
    have = [k for k, v in given.items() if v is not None]
    if have:
        raise ValueError(f"{what}: crop= acts on a reference waveform (ref_audio_path=); with {have[0]}= there is none")


def refuse_without_window(cr, what: str, seconds) -> None:
    """``crop=`` selects a window of ``seconds``: with none (``ref_seconds <= 0``: the whole clip is encoded) there is nothing to
    select, and the request is refused instead of ignored."""
    if check_crop(cr) is not None and (seconds is None or not seconds > 0):
        raise ValueError(f"{what}: crop= selects a window of ref_seconds; with ref_seconds <= 0 (the whole clip) there is none")
