"""numpy restatement of the formant control's envelope warp (definition: include/sopro_hip.h "formant control", DESIGN.md "Formants"):
sqrt-Hann STFT at 512 / 128, the low-quefrency cepstral envelope L(x) as a function of a real bin position, the gain
L(k / sigma) - L(k), overlap-add.  float64 throughout; the only fp32 value is 1 / sigma, which is what the device sees.

Also the synthetic vowel and the envelope measurements the host and GPU tests share."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

N, H, BINS, Q = 512, 128, 257, 32
EPS = 1e-12
GAIN_MAX = 18.0 * np.log(10.0) / 20.0
SR = 24000


def inv_of(formant, pitch=0.0) -> float:
    """1 / sigma, sigma = 2^((formant - pitch) / 12), in float64 and rounded once to fp32; ``formant=None`` is sigma = 1."""
    if formant is None:
        return 1.0
    return float(np.float32(2.0 ** (-(float(formant) - float(pitch)) / 12.0)))


def window() -> np.ndarray:
    i = np.arange(N, dtype=np.float64)
    return np.sqrt(0.5 * (1.0 - np.cos(2.0 * np.pi * i / N)))


def n_frames(n: int) -> int:
    return -(-int(n) // H) + 3


def frames_of(x) -> np.ndarray:
    """[F, N]: the row behind N - H zeros, zero-extended, cut into frames and windowed."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = int(x.shape[0])
    F = n_frames(n)
    xp = np.zeros(F * H + N - H)
    xp[N - H: N - H + n] = x
    return xp[np.arange(F)[:, None] * H + np.arange(N)[None, :]] * window()


def overlap_add(yf: np.ndarray, n: int) -> np.ndarray:
    """Synthesis window, scale 1/2, frames added in ascending f (the order is part of the definition); samples N - H .. N - H + n."""
    yf = yf * window() * 0.5
    y = np.zeros(yf.shape[0] * H + N - H)
    for f in range(yf.shape[0]):
        y[f * H: f * H + N] += yf[f]
    return y[N - H: N - H + n]


def cepstrum(X: np.ndarray) -> np.ndarray:
    """[F, Q]: the liftered coefficients a_q = l_q c_q (doubled for q >= 1) of the spectra X [F, 257], so that L(x) = sum_q a_q cos(2 pi q x / N)."""
    m = 0.5 * np.log(X.real * X.real + X.imag * X.imag + EPS)
    m = np.concatenate([m, m[:, -2:0:-1]], axis=1)  # even extension to N bins
    q = np.arange(Q, dtype=np.float64)
    c = m @ np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64)[:, None] * q[None, :] / N) / N
    lift = 0.5 * (1.0 + np.cos(np.pi * q / Q))
    return c * lift * np.where(q > 0, 2.0, 1.0)


def envelope_at(a: np.ndarray, x) -> np.ndarray:
    """L at the real bin positions x [P] from the coefficients a [F, Q] -> [F, P]: evaluated, never interpolated."""
    x = np.asarray(x, dtype=np.float64)
    return a @ np.cos(2.0 * np.pi * np.arange(Q, dtype=np.float64)[:, None] * x[None, :] / N)


def warp(x, inv: float) -> np.ndarray:
    """The operator on one row: x [n] -> y [n] float64, ``inv`` the fp32 value of 1 / sigma."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = int(x.shape[0])
    if n == 0:
        return x.copy()
    inv = float(np.float32(inv))
    X = np.fft.rfft(frames_of(x), axis=1)
    a = cepstrum(X)
    k = np.arange(BINS, dtype=np.float64)
    g = envelope_at(a, np.minimum(k * inv, N / 2)) - envelope_at(a, k)
    g = np.clip(g, -GAIN_MAX, GAIN_MAX)
    return overlap_add(np.fft.irfft(X * np.exp(g), n=N, axis=1), n)


def formant(x, formant_st, pitch=0.0) -> np.ndarray:
    """``warp`` with the public parameters: the envelope ends ``formant_st`` semitones from where it was before a shift by ``pitch``."""
    return warp(x, inv_of(formant_st, pitch))


# ---- synthetic material and measurements ----
F0, RES = 120.0, (700.0, 1200.0)


def vowel(n: int, f0: float = F0, res: Tuple[float, ...] = RES, bw: float = 90.0, peak: float = 0.5, sr: int = SR) -> np.ndarray:
    """A harmonic source at ``f0`` under an envelope with resonances at ``res`` (two-pole shapes of bandwidth ``bw``), float64."""
    t = np.arange(n) / sr
    s = np.zeros(n)
    for h in range(1, int(0.45 * sr / f0)):
        f = h * f0
        amp = sum(1.0 / np.sqrt(1.0 + ((f - r) / bw) ** 2) for r in res) + 0.02
        s += amp * np.sin(2.0 * np.pi * f * t + 0.7 * h * h)
    return peak * s / np.abs(s).max()


def envelope_peaks(x, lo_hz: float = 300.0, hi_hz: float = 2500.0, sr: int = SR) -> List[float]:
    """The local maxima, in Hz, of the operator's own envelope L of a row (its interior frames averaged), on a 1/32-bin grid."""
    X = np.fft.rfft(frames_of(x), axis=1)[4:-4]
    a = cepstrum(X).mean(axis=0, keepdims=True)
    grid = np.arange(lo_hz * N / sr, hi_hz * N / sr, 1.0 / 32.0)
    L = envelope_at(a, grid)[0]
    i = np.nonzero((L[1:-1] > L[:-2]) & (L[1:-1] >= L[2:]))[0] + 1
    return [float(grid[j] * sr / N) for j in i]


def pitch_lag(x, lo_hz: float = 60.0, hi_hz: float = 400.0, sr: int = SR) -> int:
    """The lag of the autocorrelation's maximum between sr / hi_hz and sr / lo_hz samples."""
    x = np.asarray(x, dtype=np.float64)
    r = np.fft.irfft(np.abs(np.fft.rfft(x, 2 * len(x))) ** 2)
    lo, hi = int(sr / hi_hz), int(sr / lo_hz)
    return lo + int(np.argmax(r[lo:hi]))
