"""numpy restatement of the pitch tracker (definition: include/sopro_hip.h "pitch tracking", DESIGN.md "Pitch tracking"): the YIN
difference and its cumulative-mean normalisation over 30 ms windows every 10 ms, up to four integer-cost candidates per frame, an
integer Viterbi path with an unvoiced state, a parabolic refinement of the chosen lag.  float64 by default; ``dtype=np.float32``
computes steps 1-2 in fp32 (numpy's summation order, not the device's).  ``paths`` runs steps 3-5 from a given v and e, which is how
the GPU test checks everything after the floating-point front end exactly: on the device's own bits.

Also the designed inputs the host and GPU tests share and the synthetic material they are built from."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from crop_ref import voice

SR = 24000
H, W, TMIN, TMAX, K = 240, 720, 48, 400, 4
SPAN = W + TMAX
NV = TMAX + 1  # values of v per frame, v[0] = 1 is never used
CENTRE = SPAN // 2
L = np.concatenate([[0], np.rint(256.0 * np.log2(np.arange(1, NV, dtype=np.float64)))]).astype(np.int64)
DEFAULTS = dict(threshold=0.5, floor_db=-50.0, octave_cost=24, jump_cost=96, switch_cost=160, unvoiced_cost=150)


def frames(n: int) -> int:
    return 0 if n < SPAN else (n - SPAN) // H + 1


def gate_of(floor_db: float) -> np.float32:
    """W 10^(floor_db / 10), floor_db as fp32, the product in double, rounded once to fp32."""
    return np.float32(float(W) * 10.0 ** (float(np.float32(floor_db)) / 10.0))


def front(x, dtype=np.float64):
    """Steps 1-2: (v [F, 401], e [F]) of one row."""
    dt = np.dtype(dtype).type
    x = np.asarray(x, dtype=np.float32).reshape(-1).astype(dt)  # the samples are fp32 in every run
    F = frames(len(x))
    v, e = np.ones((F, NV), dt), np.zeros(F, dt)
    if F == 0:
        return v, e
    idx = np.arange(F)[:, None] * H + np.arange(W)[None, :]
    a = x[idx]
    e[:] = (a * a).sum(axis=1, dtype=dt)
    d = np.zeros((F, NV), dt)
    for tau in range(1, NV):
        t = a - x[idx + tau]
        d[:, tau] = (t * t).sum(axis=1, dtype=dt)
    c = np.cumsum(d[:, 1:], axis=1, dtype=dt)
    tau = np.arange(1, NV).astype(dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        v[:, 1:] = np.where(c == 0, dt(1), d[:, 1:] * tau / c)
    return v, e


class Track(NamedTuple):
    cands: np.ndarray     # [F, 4] lags by ascending lag, 0 = none
    q: np.ndarray         # [F, 4] their integer costs
    state: np.ndarray     # [F] 0 = unvoiced, k = candidate k - 1
    tau: np.ndarray       # [F] chosen lag, 0 = unvoiced
    f0: np.ndarray        # [F] float64
    strength: np.ndarray  # [F] float64
    nvoiced: int


def candidates(v, e, threshold=0.5, floor_db=-50.0, octave_cost=24, **_):
    """Step 3 of every frame: (lags [F, 4] ascending with 0 = none, costs [F, 4])."""
    v = np.asarray(v).astype(np.float64)  # exact from fp32 bits
    F = v.shape[0]
    cands, qs = np.zeros((F, K), np.int64), np.zeros((F, K), np.int64)
    if F == 0:
        return cands, qs
    thr, gate = float(np.float32(threshold)), gate_of(floor_db)
    t = np.arange(TMIN, TMAX)
    ok = (v[:, t] < v[:, t - 1]) & (v[:, t] <= v[:, t + 1]) & (v[:, t] < thr) & (np.asarray(e).astype(np.float64) > float(gate))[:, None]
    q = np.minimum(1023, np.floor(1024.0 * v[:, t])).astype(np.int64) + ((int(octave_cost) * (L[t] - L[TMIN])) >> 8)[None, :]
    for f in np.nonzero(ok.any(axis=1))[0]:
        got = sorted((int(q[f, i]), int(t[i])) for i in np.nonzero(ok[f])[0])[:K]
        for k, (qq, tt) in enumerate(sorted(got, key=lambda p: p[1])):
            cands[f, k], qs[f, k] = tt, qq
    return cands, qs


def viterbi(cands, qs, jump_cost=96, switch_cost=160, unvoiced_cost=150, **_):
    """Step 4: the state of every frame (0 = unvoiced, k = candidate k - 1), python integers throughout."""
    F = cands.shape[0]
    state = np.zeros(F, np.int64)
    if F == 0:
        return state
    back = np.zeros((F, K + 1), np.int64)
    prev_tot, prev_tau = None, None
    for f in range(F):
        taus = [0] + [int(c) for c in cands[f]]
        cost = [int(unvoiced_cost)] + [int(c) for c in qs[f]]
        tot = [None] * (K + 1)
        for s in range(K + 1):
            if s > 0 and taus[s] == 0:
                continue
            if prev_tot is None:
                tot[s] = cost[s]
                continue
            best, arg = None, 0
            for p in range(K + 1):
                if prev_tot[p] is None:
                    continue
                if s == 0 and p == 0:
                    tr = 0
                elif s == 0 or p == 0:
                    tr = int(switch_cost)
                else:
                    tr = (int(jump_cost) * abs(int(L[taus[s]]) - int(L[prev_tau[p]]))) >> 8
                if best is None or prev_tot[p] + tr < best:
                    best, arg = prev_tot[p] + tr, p
            tot[s], back[f, s] = best + cost[s], arg
        prev_tot, prev_tau = tot, taus
    s = min((t, i) for i, t in enumerate(prev_tot) if t is not None)[1]
    for f in range(F - 1, -1, -1):
        state[f] = s
        s = int(back[f, s])
    return state


def refine(v, cands, state, dtype=np.float64):
    """Step 5: (tau [F], f0 [F], strength [F]) from the chosen states, in float64 or, with ``dtype=np.float32``, in the device's
    arithmetic (every operation rounded to fp32, den = (a - 2 b) + c; 2 b and the halving are exact, so this is what a fused form
    gives too)."""
    dt = np.dtype(dtype).type
    v = np.asarray(v).astype(dt)
    F = v.shape[0]
    tau, f0, st = np.zeros(F, np.int64), np.zeros(F, dt), np.zeros(F, dt)
    for f in np.nonzero(state)[0]:
        t = int(cands[f, state[f] - 1])
        a, b, c = v[f, t - 1], v[f, t], v[f, t + 1]
        den = (a - dt(2.0) * b) + c
        off = min(dt(0.5), max(dt(-0.5), dt(0.5) * (a - c) / den)) if den > 0 else dt(0.0)
        tau[f], f0[f], st[f] = t, dt(SR) / (dt(t) + off), dt(1.0) - min(dt(1.0), b)
    return tau, f0, st


def paths(v, e, dtype=np.float64, **params) -> Track:
    """Steps 3-5 from a given v [F, 401] and e [F] (any float type: taken as the exact values they hold); ``dtype`` is the output
    step's arithmetic."""
    p = dict(DEFAULTS, **params)
    cands, qs = candidates(v, e, **p)
    state = viterbi(cands, qs, **p)
    tau, f0, st = refine(v, cands, state, dtype)
    return Track(cands, qs, state, tau, f0, st, int((state > 0).sum()))


def track(x, dtype=np.float64, **params) -> Track:
    v, e = front(x, dtype)
    return paths(v, e, **params)


# ---- material ----
TONES = (62.0, 70.0, 97.3, 120.0, 220.0, 311.0, 440.0, 495.0)
N_ROW = SPAN + 30 * H  # the longest designed row: 31 frames


def harmonics(n: int, hz, orders=range(1, 9), noise: float = 1e-3, seed: int = 1, peak: float = 0.3) -> np.ndarray:
    """Harmonics ``orders`` of ``hz`` (a number, or the instantaneous frequency per sample) at amplitude 1 / order, peak 0.3, plus
    white noise (float64)."""
    ph = 2.0 * np.pi * np.cumsum(np.broadcast_to(np.asarray(hz, np.float64), (n,))) / SR
    s = np.zeros(n)
    for h in orders:
        s += np.sin(h * ph) / h
    s *= peak / np.abs(s).max()
    return s + noise * np.random.default_rng(seed).standard_normal(n)


def glide_hz(n: int, lo: float = 100.0, hi: float = 200.0) -> np.ndarray:
    return lo * (hi / lo) ** (np.arange(n) / max(1, n - 1))


class Row(NamedTuple):
    name: str
    x: np.ndarray              # float32
    hz: Optional[float] = None  # the planted frequency (None: the row's only check is equality with the restatement)
    params: dict = {}


_ROWS: Optional[list] = None


def designed_rows() -> list:
    """The rows every operator test runs (built once): the eight tones, the missing fundamental, the glide, noise, zeros, the vibrato
    voice at 1e-3 and 20 x scale, and the lengths 0, SPAN - 1, SPAN and SPAN + H around the first and second frame."""
    global _ROWS
    if _ROWS is None:
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
        rows = [Row(f"tone{hz:g}", f32(harmonics(N_ROW, hz, seed=int(hz))), hz) for hz in TONES]
        rows.append(Row("missing_fundamental", f32(harmonics(N_ROW, 120.0, orders=(2, 3, 4), seed=3)), 120.0))
        rows.append(Row("glide", f32(harmonics(N_ROW, glide_hz(N_ROW), seed=4))))
        rows.append(Row("noise", f32(0.1 * np.random.default_rng(5).standard_normal(N_ROW))))
        rows.append(Row("zeros", np.zeros(N_ROW, np.float32)))
        rows.append(Row("voice_1e-3", f32(1e-3 * voice(N_ROW))))
        rows.append(Row("voice_1e-3_floor-100", f32(1e-3 * voice(N_ROW)), None, dict(floor_db=-100.0)))
        rows.append(Row("voice_x20", f32(20.0 * voice(N_ROW))))
        for n in (0, SPAN - 1, SPAN, SPAN + H):
            rows.append(Row(f"n{n}", f32(voice(n))))
        _ROWS = rows
    return _ROWS


_REF: dict = {}


def reference(row: Row):
    """(v float64, e float64, Track) of a designed row, computed once and shared."""
    if row.name not in _REF:
        v, e = front(row.x)
        _REF[row.name] = (v, e, paths(v, e, **row.params))
    return _REF[row.name]


# ---- planted v matrices for the path operator ----
def planted_v(n_frames: int = 9, lags=(100, 200), cost: int = 40) -> np.ndarray:
    """v [n_frames, 401] fp32: 1.0 everywhere but a dip of ``cost`` / 1024 at every lag of ``lags``."""
    v = np.ones((n_frames, NV), np.float32)
    for t in lags:
        v[:, t] = cost / 1024.0
    return v


def planted_cases():
    """The three planted path cases as (name, v, e, params, expected chosen lags per frame).  At the default octave cost
    the lag 100 costs 40 + 25 and the lag 200 costs 40 + 49, so the shorter lag is the cheaper one unless a frame says otherwise."""
    e = np.ones(9, np.float32)
    a = planted_v()
    a[4, 200] = 5 / 1024.0
    b = planted_v()
    b[4] = 1.0
    c = np.ones((9, NV), np.float32)
    c[4, 100] = 40 / 1024.0
    base: dict = {}
    stay, visit = [100] * 9, [100] * 4 + [200] + [100] * 4
    return [("cheaper_octave_jump96", a, e, dict(base), stay), ("cheaper_octave_jump0", a, e, dict(base, jump_cost=0), visit),
            ("gap", b, e, dict(base), [100] * 4 + [0] + [100] * 4),
            ("lone", c, e, dict(base), [0] * 9), ("lone_switch0", c, e, dict(base, switch_cost=0), [0] * 4 + [100] + [0] * 4)]


def random_v(n_frames: int, seed: int, integers: bool) -> tuple:
    """A v matrix with many candidates per frame: uniform values, or multiples of 1 / 1024 from a small set (real ties); every
    seventh frame is below the gate."""
    rng = np.random.default_rng(seed)
    if integers:
        v = (rng.integers(1, 6, size=(n_frames, NV)) * 100 / 1024.0).astype(np.float32)
    else:
        v = rng.uniform(0.0, 1.2, size=(n_frames, NV)).astype(np.float32)
    e = np.where(np.arange(n_frames) % 7 == 6, 0.0, 1.0).astype(np.float32)
    return v, e
