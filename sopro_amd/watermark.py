"""Audio watermark: a keyed, tagged spread-spectrum mark added to the waveform as the engine's last step, and its detector
(definition: include/sopro_hip.h "watermark", DESIGN.md "Watermark"; numpy restatement: tests/wm_ref.py).

``Watermark(key, tag, strength_db)`` is what the public ``watermark=`` keyword takes: ``key`` (64 bits) names the deployment,
``tag`` (8 bits) a tenant of it, ``strength_db`` the level of the mark below the local peak of the audio.  ``detect(wav, key)``
answers whether a clip carries the mark of ``key``, with which tag and at which offset into the 8192-sample carrier period.

What the mark is and is not: it survives cropping, gain, 16-bit quantisation and mild additive noise, and needs a second or two of
speech-like audio (white noise is a weak host); it does NOT survive a later change of speed or pitch, resampling or a lossy codec.
It is a provenance aid, not cryptography: whoever holds the key can remove or forge it.  Its audibility at -30 dB of the local peak
has not been judged by ear on real speech.

The host makes every table (the device evaluates no hash and no transcendental function); the hot paths are the HIP kernels of
``csrc/wm.hip`` behind ``hip.wm_embed``, ``hip.WatermarkState`` and ``hip.wm_detect_rows``."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Union

import numpy as np

HS, P, CH, SHIFT, TAGS = 480, 8192, 2, 32, 256
NC = P // CH
STRENGTH_MIN, STRENGTH_MAX = -48.0, -18.0
THRESHOLD = 6.0  # one lane exceeds it by chance with probability about 8192 Q(6) = 8e-6; both are required
_M32 = 0xFFFFFFFF


@dataclass(frozen=True)
class Watermark:
    """``key`` in [0, 2^64), ``tag`` in [0, 256), ``strength_db`` in [-48, -18] (the mark's level below the local peak)."""
    key: int
    tag: int = 0
    strength_db: float = -30.0

    def __post_init__(self):
        for name, hi in (("key", 1 << 64), ("tag", TAGS)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < hi:
                raise ValueError(f"Watermark.{name} must be an integer in [0, {hi}), got {v!r}")
            object.__setattr__(self, name, int(v))
        try:
            s = float(self.strength_db)
        except (TypeError, ValueError):
            raise ValueError(f"Watermark.strength_db must be a number in [{STRENGTH_MIN}, {STRENGTH_MAX}], got {self.strength_db!r}") from None
        if not (STRENGTH_MIN <= s <= STRENGTH_MAX):  # (NaN fails both comparisons)
            raise ValueError(f"Watermark.strength_db must lie in [{STRENGTH_MIN}, {STRENGTH_MAX}], got {self.strength_db!r}")
        object.__setattr__(self, "strength_db", s)

    @property
    def alpha(self) -> float:
        """fl32(10^(strength_db / 20)): all the device sees of a strength."""
        return float(np.float32(10.0 ** (self.strength_db / 20.0)))


class WatermarkResult(NamedTuple):
    present: bool   # score >= 6
    score: float    # min(z_sync, z_tag)
    tag: int        # meaningful when present
    offset: int     # position of the clip's first sample in the carrier period, as -crop mod 8192
    z_sync: float
    z_tag: float


def check_mark(mark, what: str = "watermark") -> Optional[Watermark]:
    if mark is not None and not isinstance(mark, Watermark):
        raise TypeError(f"{what} must be a sopro_amd.Watermark or None, got {type(mark).__name__}")
    return mark


def per_row(marks, rows: int, what: str = "watermark") -> List[Optional[Watermark]]:
    """One mark (or None) per row from one ``Watermark`` / None or a sequence of them."""
    if marks is None or isinstance(marks, Watermark):
        return [marks] * int(rows)
    if isinstance(marks, (str, bytes)) or not hasattr(marks, "__len__"):
        raise TypeError(f"{what} must be a sopro_amd.Watermark, None or one of them per row, got {type(marks).__name__}")
    vals = [check_mark(m, what) for m in marks]
    if len(vals) != int(rows):
        raise ValueError(f"{what}: one value or one per row ({rows}), got {len(vals)}")
    return vals


def _key(key) -> int:
    if isinstance(key, bool) or not isinstance(key, (int, np.integer)) or not 0 <= int(key) < 1 << 64:
        raise ValueError(f"key must be an integer in [0, 2^64), got {key!r}")
    return int(key)


def _fmix(h):
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(_M32)
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(_M32)
    return h ^ (h >> np.uint64(16))


def lanes_host(key: int) -> np.ndarray:
    """int8 [2, P]: the chip sequences c_0 (sync) and c_1 (tag) of a key, values +-1, two samples per chip."""
    key = _key(key)
    lo, hi = np.uint64(key & _M32), np.uint64(key >> 32)
    i = np.arange(NC, dtype=np.uint64)
    first = _fmix((i * np.uint64(0x9E3779B1) + lo) & np.uint64(_M32))
    out = np.empty((2, P), np.int8)
    for lane in (0, 1):
        h = _fmix(first ^ hi ^ np.uint64((lane * 0x7F4A7C15) & _M32))
        out[lane] = np.repeat(np.where((h >> np.uint64(31)) & np.uint64(1), -1, 1).astype(np.int8), CH)
    return out


def carrier_host(key: int, tag: int) -> np.ndarray:
    """int8 [P]: car[n] = c_0[n] + c_1[(n - SHIFT * tag) mod P], values in {-2, 0, 2}."""
    if isinstance(tag, bool) or not 0 <= int(tag) < TAGS:
        raise ValueError(f"tag must lie in [0, {TAGS}), got {tag!r}")
    c = lanes_host(key)
    return (c[0] + np.roll(c[1], SHIFT * int(tag))).astype(np.int8)


def templates_host(key: int) -> np.ndarray:
    """int8 [2, P]: d_l[n] = c_l[n] - c_l[(n - 1) mod P], the detector's templates (the whitening is a first difference)."""
    c = lanes_host(key)
    return (c - np.roll(c, 1, axis=1)).astype(np.int8)


_tables: dict = {}  # ("car", key, tag, device) / ("tpl", key, device) -> the table on the device; a tuple of such keys -> their stack


def _cached(key, make):
    t = _tables.get(key)
    if t is None:
        if len(_tables) > 256:  # (a service with many tenants: the tables are cheap to make again)
            _tables.clear()
        t = _tables[key] = make()
    return t


def carrier_tables(marks: Sequence[Optional[Watermark]], device):
    """The carrier tables a batch needs, int8 [n_cars, P] on the device, and every row's index into them (-1: no mark)."""
    import torch

    keys: List[tuple] = []
    idx = []
    for m in marks:
        if m is None:
            idx.append(-1)
            continue
        k = (m.key, m.tag)
        if k not in keys:
            keys.append(k)
        idx.append(keys.index(k))
    dev = str(device)
    one = [_cached(("car", k[0], k[1], dev), lambda k=k: torch.from_numpy(carrier_host(*k)).to(device)) for k in keys]
    if len(one) == 1:
        return one[0].unsqueeze(0), idx
    return _cached((tuple(keys), "car", dev), lambda: torch.stack(one)), idx


def template_tables(keys_per_row: Sequence[int], device):
    """The templates a batch of clips needs, int8 [n_keys, 2, P] on the device, and every row's index into them."""
    import torch

    keys: List[int] = []
    idx = []
    for k in keys_per_row:
        k = _key(k)
        if k not in keys:
            keys.append(k)
        idx.append(keys.index(k))
    dev = str(device)
    one = [_cached(("tpl", k, dev), lambda k=k: torch.from_numpy(templates_host(k)).to(device)) for k in keys]
    if len(one) == 1:
        return one[0].unsqueeze(0), idx
    return _cached((tuple(keys), "tpl", dev), lambda: torch.stack(one)), idx


def result_of(o0: int, o1: int, z0: float, z1: float, empty: bool = False) -> WatermarkResult:
    """Step 5 of the definition, on the host."""
    if empty:
        return WatermarkResult(False, 0.0, 0, 0, 0.0, 0.0)
    tag = ((((int(o1) - int(o0)) % P) + SHIFT // 2) // SHIFT) % TAGS
    score = min(float(z0), float(z1))
    return WatermarkResult(bool(score >= THRESHOLD), score, tag, int(o0), float(z0), float(z1))


def detect(wav, key: int, *, lens=None, device=None) -> Union[WatermarkResult, List[WatermarkResult]]:
    """Does ``wav`` carry the mark of ``key``?  ``wav``: a clip [N] or [1, 1, N] (one result), a list of such clips (a list of
    results), or padded rows [B, N] with ``lens`` (a list); torch tensors or numpy arrays, 24 kHz mono.  The clips are moved to
    ``device`` (default: where the first tensor lives, else the current HIP device) and run through ``hip.wm_detect_rows`` as one
    padded batch: fold, two 8192 x 8192 circular correlations per clip, peak statistics - four launches and one small host copy."""
    import torch

    from . import hip

    key = _key(key)
    single = False
    if isinstance(wav, (list, tuple)):
        clips = [torch.as_tensor(w).reshape(-1) for w in wav]
    else:
        t = torch.as_tensor(wav)
        if lens is not None:
            if t.dim() != 2:
                raise ValueError("detect(wav, key, lens=...) wants padded rows [B, N]")
            clips = None
        else:
            if t.dim() == 2 and int(t.shape[0]) != 1:
                raise ValueError("detect: padded rows [B, N] need lens=")
            clips, single = [t.reshape(-1)], True
    if device is None:
        src = t if clips is None else (clips[0] if clips else None)
        device = src.device if src is not None and src.device.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if clips is None:
        rows = t.to(device=device, dtype=torch.float32)
        lens_h = [int(v) for v in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
    else:
        if not clips:
            return []
        lens_h = [int(c.numel()) for c in clips]
        rows = torch.zeros(len(clips), max(1, max(lens_h)), dtype=torch.float32, device=device)
        for b, c in enumerate(clips):
            rows[b, : lens_h[b]] = c.to(device=device, dtype=torch.float32)
    res = hip.wm_detect_rows(rows, lens_h, [key] * len(lens_h))
    return res[0] if single else res
