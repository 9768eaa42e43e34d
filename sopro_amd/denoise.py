"""Reference denoising: a stationary-noise suppressor on the waveform a voice is cloned from (definition: include/sopro_hip.h
"reference denoising", DESIGN.md "Reference denoising"; numpy restatement: tests/denoise_ref.py).

``Denoise(atten_db, bias)`` is what the public ``denoise=`` keyword takes.  ``atten_db`` is the most a bin is ever turned down
(the floor of the Wiener gain), ``bias`` the factor between the tracked minimum of the smoothed periodogram and the noise power
it stands for.  Both defaults are choices, not measurements on real recordings: on white noise the tracked minimum is 0.21 of the
mean power, so an unbiased floor would be 4.7; 3.0 sits below that and errs towards keeping speech.

The step acts on the input side only: load -> energy trim -> resample -> denoise -> centre crop -> encode
(``MimiCodec.reference_waveform``).  With ``ref_tokens_tq=`` or ``ref=`` there is no waveform, and ``denoise=`` is refused.  The hot
path is the HIP kernels of ``csrc/denoise.hip`` behind ``hip.denoise``."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, NamedTuple, Optional

ATTEN_MIN, ATTEN_MAX, ATTEN_DEFAULT = 0.0, 40.0, 15.0
BIAS_MIN, BIAS_MAX, BIAS_DEFAULT = 1.0, 8.0, 3.0


def _number(name: str, v) -> float:
    if isinstance(v, bool):
        raise ValueError(f"Denoise.{name} must be a number, got {v!r}")
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"Denoise.{name} must be a number, got {v!r}") from None
    if not math.isfinite(f):
        raise ValueError(f"Denoise.{name} must be finite, got {v!r}")
    return f


@dataclass(frozen=True)
class Denoise:
    """``atten_db``: the largest attenuation of a bin, 0 .. 40 dB (0: the row comes back as it went in, to rounding);
    ``bias``: noise power over tracked minimum, 1 .. 8."""
    atten_db: float = ATTEN_DEFAULT
    bias: float = BIAS_DEFAULT

    def __post_init__(self):
        for name in ("atten_db", "bias"):
            object.__setattr__(self, name, _number(name, getattr(self, name)))
        if not ATTEN_MIN <= self.atten_db <= ATTEN_MAX:
            raise ValueError(f"Denoise.atten_db must lie in [{ATTEN_MIN:g}, {ATTEN_MAX:g}] dB, got {self.atten_db!r}")
        if not BIAS_MIN <= self.bias <= BIAS_MAX:
            raise ValueError(f"Denoise.bias must lie in [{BIAS_MIN:g}, {BIAS_MAX:g}], got {self.bias!r}")


class DenoiseReport(NamedTuple):
    """What a denoised row was and what left it: ``input_db`` the row's mean power (dB re 1.0), ``removed_db`` the energy of
    (input - output) over the input's energy (dB, below 0)."""
    input_db: float
    removed_db: float


def check_denoise(dn, what: str = "denoise") -> Optional[Denoise]:
    if dn is not None and not isinstance(dn, Denoise):
        raise TypeError(f"{what} must be a sopro_amd.Denoise or None, got {type(dn).__name__}")
    return dn


def per_row(dns, rows: int, what: str = "denoise") -> List[Optional[Denoise]]:
    """One ``Denoise`` (or None) per row from one ``Denoise`` / None or a sequence of them."""
    if dns is None or isinstance(dns, Denoise):
        return [dns] * int(rows)
    if isinstance(dns, (str, bytes)) or not hasattr(dns, "__len__"):
        raise TypeError(f"{what} must be a sopro_amd.Denoise, None or one of them per row, got {type(dns).__name__}")
    vals = [check_denoise(d, what) for d in dns]
    if len(vals) != int(rows):
        raise ValueError(f"{what}: one value or one per row ({rows}), got {len(vals)}")
    return vals


def refuse_without_waveform(dn, what: str, **given) -> None:
    """``denoise=`` needs a waveform: with reference tokens or a prepared reference (the keywords of ``given`` that are not None)
    there is none, and the request is refused instead of ignored."""
    if check_denoise(dn) is None:
        return
    have = [k for k, v in given.items() if v is not None]
    if have:
        raise ValueError(f"{what}: denoise= acts on a reference waveform (ref_audio_path=); with {have[0]}= there is none")


def report_sink(report) -> None:
    if report is not None and not isinstance(report, list):
        raise TypeError(f"report must be a list (it receives the DenoiseReport, then the CropReport, of what was asked for) or None, got {type(report).__name__}")
