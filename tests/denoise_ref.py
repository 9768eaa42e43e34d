"""numpy restatement of the reference denoiser (definition: include/sopro_hip.h "reference denoising", DESIGN.md "Reference
denoising"): STFT, minimum-statistics noise floor, decision-directed Wiener gain, overlap-add.  float64 by default; ``dtype=np.float32``
runs every step in fp32, which is what the GPU tests take their bar from (the restatement's own rounding, never the library's).

Also the designed inputs the host and GPU tests share (``designed_batch``) and the synthetic voice they are built from."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

N, H, BINS, SPAN = 512, 128, 257, 94
BETA, ALPHA, FLOOR = 0.7, 0.98, 1e-20
ATTEN_DEFAULT, BIAS_DEFAULT = 15.0, 3.0
SR = 24000


def window(dtype=np.float64) -> np.ndarray:
    i = np.arange(N, dtype=np.float64)
    return np.sqrt(0.5 * (1.0 - np.cos(2.0 * np.pi * i / N))).astype(dtype)


def n_frames(n: int) -> int:
    return -(-int(n) // H) + 3


class Parts(NamedTuple):
    y: np.ndarray      # [n]
    X: np.ndarray      # [F, 257] complex
    S: np.ndarray      # [F, 257]
    M: np.ndarray
    G: np.ndarray
    input_db: float
    removed_db: float


def denoise_parts(x, atten_db: float = ATTEN_DEFAULT, bias: float = BIAS_DEFAULT, dtype=np.float64) -> Parts:
    dt = np.dtype(dtype).type
    cdt = np.complex64 if dt is np.float32 else np.complex128
    x = np.asarray(x, dtype=dt).reshape(-1)
    n = int(x.shape[0])
    if n == 0:
        z = np.zeros((0, BINS), dt)
        return Parts(x.copy(), z.astype(cdt), z, z, z, float(10.0 * np.log10(1e-20)), 0.0)
    w = window(dt)
    F = n_frames(n)
    xp = np.zeros(F * H + N - H, dt)
    xp[N - H: N - H + n] = x
    frames = xp[np.arange(F)[:, None] * H + np.arange(N)[None, :]] * w
    X = np.fft.rfft(frames, axis=1).astype(cdt)
    P = (X.real * X.real + X.imag * X.imag).astype(dt)
    beta, alpha = dt(BETA), dt(ALPHA)
    S = np.empty_like(P)
    S[0] = P[0]
    for f in range(1, F):
        S[f] = beta * S[f - 1] + (dt(1) - beta) * P[f]
    M = np.empty_like(S)
    for f in range(F):
        M[f] = S[max(0, f - SPAN): min(F, f + SPAN + 1)].min(axis=0)
    noise = np.maximum(dt(bias) * M, dt(FLOOR))
    gamma = P / noise
    g_min = dt(10.0 ** (-float(atten_db) / 20.0))
    G = np.empty_like(P)
    inst = np.maximum(gamma - dt(1), dt(0))
    xi = inst[0]
    G[0] = np.maximum(xi / (dt(1) + xi), g_min)
    for f in range(1, F):
        xi = alpha * G[f - 1] * G[f - 1] * gamma[f - 1] + (dt(1) - alpha) * inst[f]
        G[f] = np.maximum(xi / (dt(1) + xi), g_min)
    yf = np.fft.irfft((G * X).astype(cdt), n=N, axis=1).astype(dt) * w * dt(0.5)
    y = np.zeros_like(xp)
    for f in range(F):  # ascending f: the order of the additions is part of the definition
        y[f * H: f * H + N] += yf[f]
    out = y[N - H: N - H + n]
    x64, d64 = x.astype(np.float64), x.astype(np.float64) - out.astype(np.float64)
    ex, ed = float((x64 * x64).sum()), float((d64 * d64).sum())
    return Parts(out, X, S, M, G, float(10.0 * np.log10(ex / n + 1e-20)), float(10.0 * np.log10((ed + 1e-20) / (ex + 1e-20))))


def denoise(x, atten_db: float = ATTEN_DEFAULT, bias: float = BIAS_DEFAULT, dtype=np.float64) -> np.ndarray:
    return denoise_parts(x, atten_db, bias, dtype).y


# ---- synthetic material ----
def voice(n: int, sr: int = SR) -> np.ndarray:
    """24 harmonics of 120 Hz with a slow vibrato under a 300 ms on / 200 ms off envelope, peak 0.3."""
    t = np.arange(n) / sr
    s = np.zeros(n)
    for h in range(1, 25):
        s += np.sin(2 * np.pi * 120 * h * t * (1 + 0.02 * np.sin(2 * np.pi * 0.7 * t))) / h
    env = ((t % 0.5) < 0.3).astype(np.float64)
    k = np.hanning(481)
    env = np.convolve(env, k / k.sum(), "same")
    s *= env
    return 0.3 * s / np.abs(s).max()


def noise(n: int, kind: str, rng) -> np.ndarray:
    v = rng.standard_normal(n)
    if kind == "pink":  # 1/f power
        V = np.fft.rfft(v)
        V[1:] /= np.sqrt(np.arange(1, len(V)))
        V[0] = 0
        v = np.fft.irfft(V, n)
    return v


def at_snr(s: np.ndarray, v: np.ndarray, snr_db: float) -> np.ndarray:
    """``s`` plus ``v`` scaled so that the mix has ``snr_db``."""
    return s + v * np.sqrt((s * s).sum() / (v * v).sum() / 10.0 ** (snr_db / 10.0))


def snr_db(clean: np.ndarray, y: np.ndarray) -> float:
    return float(10.0 * np.log10((clean * clean).sum() / ((y - clean) ** 2).sum()))


def noisy_voice(seconds: float, kind: str = "white", snr: float = 10.0, seed: int = 1, sr: int = SR):
    """(clean, noisy) float64."""
    n = int(round(seconds * sr))
    s = voice(n, sr)
    return s, at_snr(s, noise(n, kind, np.random.default_rng(seed)), snr)


class Row(NamedTuple):
    name: str
    x: np.ndarray               # float32
    atten_db: float
    bias: float


_BATCH: Optional[list] = None


def designed_batch() -> list:
    """The rows every operator test runs (built once): the lengths around a hop and a frame, the lengths at the edge and the full
    span of the minimum window, the voice under white and 1/f noise, a run of exact zeros, an all-zero row, a row at 20 x scale."""
    global _BATCH
    if _BATCH is not None:
        return _BATCH
    rng = np.random.default_rng(20)
    rows = []
    for n in (1, 2, 127, 128, 129, 511, 512, 513):
        rows.append(Row(f"len{n}", (0.1 * rng.standard_normal(n)).astype(np.float32), ATTEN_DEFAULT, BIAS_DEFAULT))
    for n in (SPAN * H, (SPAN + 1) * H + 1, (2 * SPAN + 1) * H + 5):
        s = voice(n)
        rows.append(Row(f"len{n}", at_snr(s, noise(n, "white", rng), 10.0).astype(np.float32), ATTEN_DEFAULT, BIAS_DEFAULT))
    s, white = noisy_voice(2.0, "white", seed=21)
    _, pink = noisy_voice(2.0, "pink", seed=22)
    rows.append(Row("voice_white", white.astype(np.float32), ATTEN_DEFAULT, BIAS_DEFAULT))
    rows.append(Row("voice_pink", pink.astype(np.float32), 25.0, 2.0))
    gap = white.astype(np.float32).copy()
    gap[20000:26000] = 0.0
    rows.append(Row("voice_zero_run", gap, ATTEN_DEFAULT, BIAS_DEFAULT))
    rows.append(Row("all_zero", np.zeros(3000, np.float32), ATTEN_DEFAULT, BIAS_DEFAULT))
    rows.append(Row("scale20", (20.0 * white[:24000]).astype(np.float32), 40.0, 8.0))
    _BATCH = rows
    return rows


_REF: dict = {}


def reference(row: Row):
    """(float64 parts, float32 parts) of a designed row, computed once and shared."""
    if row.name not in _REF:
        _REF[row.name] = (denoise_parts(row.x, row.atten_db, row.bias), denoise_parts(row.x, row.atten_db, row.bias, np.float32))
    return _REF[row.name]


def bar(row: Row) -> float:
    """What the device may deviate from the float64 run on this row: 8 x the restatement's own float32 deviation, and at least one
    fp32 ulp of the row's peak."""
    p64, p32 = reference(row)
    dev = float(np.abs(p32.y.astype(np.float64) - p64.y).max()) if len(p64.y) else 0.0
    peak = float(np.abs(row.x).max()) if len(row.x) else 0.0
    return max(8.0 * dev, float(np.spacing(np.float32(peak))))
