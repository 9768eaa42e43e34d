"""Voice similarity: did a take keep the voice, and which stored voice is a clip?

The instrument is the model's own ``Token2SV`` (reference: src/sopro/nn/speaker.py:37-61), the module that makes ``sv_ref``: codec
tokens -> a unit speaker vector.  ``hip.spk_embed_rows`` computes it for every row of a padded batch in two launches, each row
exactly as its own unpadded utterance (the form ``prepare_reference`` stores), and ``hip.spk_cosine`` compares the vectors pair by
pair or against a bank of voices.  This module holds the public value types, the argument checks and the host-side ranking;
``SoproTTS.speaker_vectors`` / ``voice_similarity`` / ``identify_voice`` and the ``similarity=`` sink of ``synthesize`` /
``synthesize_batch`` are built on it.

No thresholds: what cosine means "the same speaker" depends on the checkpoint, and this project ships none, so nothing here
turns a cosine into a yes or a no.  Calibrate on recordings of your own voices.

Out of scope: the streaming entry points (``stream*``), ``SynthesisService``, choosing between takes or retrying one, and any
guarantee about the bf16 mode's tokens (the similarity path itself is fp32 in both modes).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, List, Optional, Sequence

import torch


@dataclass(frozen=True)
class VoiceMatch:
    """How close a clip's voice is to a reference: ``cosine`` of the two speaker vectors (in [-1, 1]; 0.0 for a clip without
    frames) over the clip's ``frames`` codec frames (12.5 per second)."""

    cosine: float
    frames: int

    def __post_init__(self):
        if isinstance(self.frames, bool) or not isinstance(self.frames, int) or self.frames < 0:
            raise ValueError(f"VoiceMatch.frames must be an integer >= 0, got {self.frames!r}")
        if isinstance(self.cosine, bool) or not isinstance(self.cosine, (int, float)) or not math.isfinite(self.cosine):
            raise ValueError(f"VoiceMatch.cosine must be a finite number, got {self.cosine!r}")


@dataclass(frozen=True)
class VoiceHit:
    """One entry of ``identify_voice``'s ranking: the voice's ``index`` in the bank, its ``name`` (None for an unnamed bank) and the
    ``cosine`` of the clip's speaker vector with it."""

    index: int
    name: Optional[str]
    cosine: float


class VoiceBank:
    """A set of stored voices as one [N, sv_dim] fp32 matrix, built once and compared against in one launch.  ``voices``: a sequence
    of ``PreparedReference`` (their ``sv_ref``), a sequence of speaker vectors ([sv_dim] or [1, sv_dim] each), or one [N, sv_dim]
    tensor.  ``names``: one string per voice (optional; ``VoiceHit.name`` is None without them).  The matrix lives where the
    vectors live; ``on(device)`` gives it on the engine's device."""

    def __init__(self, voices: Any, names: Optional[Sequence[str]] = None):
        if isinstance(voices, torch.Tensor):
            if voices.dim() != 2:
                raise ValueError(f"VoiceBank: a tensor of voices must be [N, sv_dim], got {tuple(voices.shape)}")
            rows = [voices[i] for i in range(int(voices.shape[0]))]
        elif isinstance(voices, (list, tuple)):
            rows = [getattr(v, "sv_ref", v) for v in voices]
        else:
            raise TypeError("VoiceBank wants a sequence of PreparedReference, a sequence of speaker vectors or one [N, sv_dim] tensor")
        if not rows:
            raise ValueError("VoiceBank: at least one voice")
        vecs = []
        for i, v in enumerate(rows):
            if not isinstance(v, torch.Tensor) or not v.is_floating_point() or v.numel() == 0 or v.numel() != int(v.shape[-1]):
                raise ValueError(f"VoiceBank: voice {i} is not a speaker vector ([sv_dim] or [1, sv_dim] floating point)")
            vecs.append(v.detach().reshape(-1))
        if len({int(v.numel()) for v in vecs}) != 1 or len({v.device for v in vecs}) != 1:
            raise ValueError("VoiceBank: the speaker vectors must have one width and live on one device")
        if names is not None:
            names = list(names)
            if len(names) != len(vecs) or not all(isinstance(n, str) for n in names):
                raise ValueError(f"VoiceBank: names must be one string per voice ({len(vecs)})")
        self.names: Optional[List[str]] = names
        self.vectors = torch.stack(vecs).to(torch.float32).contiguous()
        self._on = {}

    def __len__(self) -> int:
        return int(self.vectors.shape[0])

    @property
    def dim(self) -> int:
        return int(self.vectors.shape[1])

    def on(self, device) -> torch.Tensor:
        """The matrix on ``device`` (copied once per device)."""
        device = torch.device(device)
        if self.vectors.device == device:
            return self.vectors
        t = self._on.get(device)
        if t is None:
            t = self._on[device] = self.vectors.to(device)
        return t


def sink_of(sink: Any, what: str) -> None:
    """``similarity=`` is a sink like ``alignment=`` and ``report=``: None, or a list that receives the results."""
    if sink is not None and not isinstance(sink, list):
        raise TypeError(f"{what}(similarity=...) wants a list to fill with one VoiceMatch per row (or None), got {type(sink).__name__}")


def as_bank(voices: Any) -> VoiceBank:
    return voices if isinstance(voices, VoiceBank) else VoiceBank(voices)


def check_top(top: Any) -> int:
    if isinstance(top, bool) or not isinstance(top, int) or top < 1:
        raise ValueError(f"top must be an integer >= 1, got {top!r}")
    return top


def rank(cosines: Sequence[float], names: Optional[Sequence[str]] = None, top: int = 5) -> List[VoiceHit]:
    """The ``top`` best voices, best first.  The sort is stable: equal cosines keep the bank's order (the lower index wins)."""
    top = check_top(top)
    cs = [float(c) for c in cosines]
    if names is not None and len(names) != len(cs):
        raise ValueError("rank: one name per cosine")
    order = sorted(range(len(cs)), key=lambda i: -cs[i])
    return [VoiceHit(i, names[i] if names is not None else None, cs[i]) for i in order[:top]]


def matches(cosines: Sequence[float], frames: Sequence[int]) -> List[VoiceMatch]:
    """One ``VoiceMatch`` per row; a row without frames has no voice: (0.0, 0)."""
    return [VoiceMatch(float(c) if int(n) > 0 else 0.0, int(n)) for c, n in zip(cosines, frames)]


def token_rows(tokens: Any, lens: Any, Q: int):
    """``tokens`` [T, Q] (one clip) or [B, T, Q] (a padded batch; ``lens`` valid frames per row, default T) of integer codes ->
    (tokens [B, T, Q], lens on the host, batched)."""
    if not isinstance(tokens, torch.Tensor) or tokens.is_floating_point() or tokens.dim() not in (2, 3) or int(tokens.shape[-1]) != int(Q):
        raise ValueError(f"tokens must be integer codes [T, {Q}] or [B, T, {Q}]")
    batched = tokens.dim() == 3
    t = tokens if batched else tokens.unsqueeze(0)
    B, T = int(t.shape[0]), int(t.shape[1])
    if lens is None:
        lens_h = [T] * B
    else:
        lens_h = [int(v) for v in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
        if not batched and len(lens_h) != 1:
            raise ValueError("lens: one clip has one length")
    if len(lens_h) != B or any(n < 0 or n > T for n in lens_h):
        raise ValueError(f"lens must hold one length in [0, {T}] per row ({B}), got {lens_h}")
    return t, lens_h, batched
