"""numpy restatement of the reference crop selection (definition: include/sopro_hip.h "reference crop selection", DESIGN.md
"Reference crop selection"): a grid of 10 ms blocks anchored on the centre crop, per-block energy and clip flag, a threshold from the
row's loudest block and its 50 ms-smoothed floor, an integer score per candidate window, the pick with its tie rules.  float64 by
default; ``dtype=np.float32`` computes the energies and the threshold in fp32, which is what the host test uses to show that the
designed rows leave the decision no room (``margin``), so that the GPU test can demand equality.

Also the designed inputs the host and GPU tests share (``designed_batch``) and the synthetic material they are built from."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

H, SMOOTH = 240, 5
RANGE_DEFAULT, MARGIN_DEFAULT, LEVEL_DEFAULT, WEIGHT_DEFAULT = 30.0, 10.0, 0.999, 4
SR = 24000
W0 = 1920  # the window of the designed batch: one Mimi frame, 8 blocks


class Report(NamedTuple):
    start: int
    active: int
    clipped: int
    centre_active: int
    centre_clipped: int
    row_active: int
    blocks: int
    level_db: float


class Parts(NamedTuple):
    start: int
    out_len: int
    o: int
    F: int
    e: np.ndarray        # [F]
    c: np.ndarray        # [F] 0 / 1
    a: np.ndarray        # [F] 0 / 1
    thr: float
    score: np.ndarray    # [candidates], int64
    k: int
    kc: int
    report: Report


def grid(n: int, W: int):
    """(long, s_c, o, F, Wb, k_c) of a row of n samples under a window of W."""
    if n <= W:
        F = n // H
        return False, 0, 0, F, F, 0
    sc = (n - W) // 2
    o = sc % H
    return True, sc, o, (n - o) // H, W // H, (sc - o) // H


def crop_parts(x, W: int, range_db: float = RANGE_DEFAULT, margin_db: float = MARGIN_DEFAULT, clip_level: float = LEVEL_DEFAULT,
               clip_weight: int = WEIGHT_DEFAULT, dtype=np.float64) -> Parts:
    assert W >= H and W % H == 0
    dt = np.dtype(dtype).type
    x = np.asarray(x, dtype=np.float32).reshape(-1)  # the samples are fp32 in every run
    n = int(x.shape[0])
    lng, sc, o, F, Wb, kc = grid(n, W)
    if F == 0:
        z = np.zeros(0, np.int64)
        return Parts(0, n, 0, 0, np.zeros(0, dt), z, z, 0.0, np.zeros(1, np.int64), 0, 0, Report(0, 0, 0, 0, 0, 0, 0, float(10.0 * np.log10(1e-20))))
    blk = x[o: o + F * H].reshape(F, H)
    e = (blk.astype(dt) ** 2).sum(axis=1, dtype=dt)
    c = (np.abs(blk) >= np.float32(clip_level)).any(axis=1).astype(np.int64)
    emax = e.max()
    if F >= SMOOTH:
        s5 = e[: F - SMOOTH + 1].copy()
        for u in range(1, SMOOTH):  # ascending, as the definition writes the sum
            s5 = s5 + e[u: F - SMOOTH + 1 + u]
        emin = (s5 / dt(SMOOTH)).min()
    else:
        emin = e.min()
    thr = max(emax * dt(10.0 ** (-float(range_db) / 10.0)), emin * dt(10.0 ** (float(margin_db) / 10.0)))
    a = (e > thr).astype(np.int64)
    pre = np.concatenate([[0], np.cumsum(a - int(clip_weight) * c)])
    score = pre[Wb:] - pre[: F - Wb + 1]
    ks = np.arange(F - Wb + 1)
    k = int(min(ks, key=lambda q: (-int(score[q]), abs(int(q) - kc), int(q))))
    start = o + k * H if lng else 0
    lvl = float(10.0 * np.log10(float(e[k: k + Wb].astype(np.float64).sum()) / W + 1e-20))
    rep = Report(start, int(a[k: k + Wb].sum()), int(c[k: k + Wb].sum()), int(a[kc: kc + Wb].sum()), int(c[kc: kc + Wb].sum()), int(a.sum()), F, lvl)
    return Parts(start, min(n, W), o, F, e, c, a, float(thr), score, k, kc, rep)


def crop(x, W: int, **kw) -> np.ndarray:
    p = crop_parts(x, W, **kw)
    return np.asarray(x, np.float32).reshape(-1)[p.start: p.start + p.out_len]


# ---- synthetic material ----
def voice(n: int, sr: int = SR, f0: float = 120.0) -> np.ndarray:
    """Eight harmonics of ``f0`` with a slow vibrato, peak 0.3 (float64)."""
    if n == 0:
        return np.zeros(0)
    t = np.arange(n) / sr
    s = np.zeros(n)
    for h in range(1, 9):
        s += np.sin(2 * np.pi * f0 * h * t * (1 + 0.02 * np.sin(2 * np.pi * 0.7 * t))) / h
    peak = np.abs(s).max()
    return 0.3 * s / peak if peak > 0 else s


def clip_of(n: int, spans, seed: int, noise: float = 1e-4, sr: int = SR) -> np.ndarray:
    """``n`` samples of faint white noise with the voice switched on (hard edges) over the sample ranges ``spans``."""
    x = noise * np.random.default_rng(seed).standard_normal(n)
    v = voice(n, sr)
    for lo, hi in spans:
        x[lo:hi] += v[lo:hi]
    return x


def on_blocks(n: int, W: int, runs, seed: int, **kw) -> np.ndarray:
    """``clip_of`` with the voice on over runs of whole blocks [(first block, end block)] of the row's own grid."""
    o = grid(n, W)[2]
    return clip_of(n, [(o + a * H, o + b * H) for a, b in runs], seed, **kw)


class Row(NamedTuple):
    name: str
    x: np.ndarray               # float32
    W: int
    range_db: float = RANGE_DEFAULT
    margin_db: float = MARGIN_DEFAULT
    clip_level: float = LEVEL_DEFAULT
    clip_weight: int = WEIGHT_DEFAULT
    start: Optional[int] = None  # the start the design expects, worked out by hand (None: whatever the restatement says)

    @property
    def params(self):
        return dict(range_db=self.range_db, margin_db=self.margin_db, clip_level=self.clip_level, clip_weight=self.clip_weight)


_BATCH: Optional[list] = None


def designed_batch() -> list:
    """The rows every operator test runs (built once), W = 1920 (8 blocks) unless a row says otherwise: the smallest rows at which
    each part can go wrong.  The lengths 0, below a block, W, W + 1, W + H - 1, W + H (one candidate each), W + 2H - 1 (two
    candidates) and W + 2H (by the definition o = 0 and F = 10, so three candidates); a constant tone whose grid offset is not 0 (no
    preference: the centre start, not a multiple of H); a symmetric two-sided tie (the smaller k); speech late and early; a clipped
    sample in the densest window, and the same row with clip_weight = 0; an all-zero row; a row with a gap of exact zeros (Emin =
    0); a W = H call with F < 5; the late row at 1e-3 and at 20 x scale; a row of 2600 blocks."""
    global _BATCH
    if _BATCH is not None:
        return _BATCH
    f32 = lambda v: np.asarray(v, np.float32)  # noqa: E731
    W = W0
    rows = [Row("n0", np.zeros(0, np.float32), W, start=0),
            Row("n100", f32(voice(100)), W, start=0),
            Row("nW", f32(voice(W)), W, start=0),
            Row("nW+1", f32(voice(W + 1)), W, start=0),
            Row("nW+H-1", f32(voice(W + H - 1)), W, start=(H - 1) // 2),
            Row("nW+H", f32(voice(W + H)), W, start=H // 2),
            # s_c = 239 = o, F = 9, k in {0, 1}, k_c = 0: the voice is on over blocks 1 .. 8, so k = 1
            Row("nW+2H-1", f32(on_blocks(W + 2 * H - 1, W, [(1, 9)], 1)), W, margin_db=0.0, start=239 + H),
            # s_c = 240, o = 0, F = 10, k in {0, 1, 2}, k_c = 1: the voice is on over blocks 2 .. 9, so k = 2
            Row("nW+2H", f32(on_blocks(W + 2 * H, W, [(2, 10)], 2)), W, margin_db=0.0, start=2 * H)]
    # a 1 kHz tone, ten periods per block: every block has the same energy, none is active; n - W = 634: s_c = 317, o = 77
    n = W + 634
    rows.append(Row("tone_tie", f32(0.25 * np.sin(2 * np.pi * 1000.0 * np.arange(n) / SR)), W, start=317))
    # F = 20 blocks from o = 50, k = 0 .. 12, k_c = 6: on over blocks 0 .. 6 and 13 .. 19; k = 0 and k = 12 both score 7
    n = W + 12 * H + 100
    rows.append(Row("two_sided_tie", f32(on_blocks(n, W, [(0, 7), (13, 20)], 3)), W, start=50))
    # F = 28 from o = 0, k = 0 .. 20, k_c = 10: on over the last / the first 10 blocks; the nearest full window wins
    n = W + 20 * H
    late = f32(on_blocks(n, W, [(18, 28)], 4))
    rows.append(Row("late", late, W, start=18 * H))
    rows.append(Row("early", f32(on_blocks(n, W, [(0, 10)], 5)), W, start=2 * H))
    # F = 24 from o = 0, k = 0 .. 16, k_c = 8: on over blocks 2 .. 9 (k = 2 scores 8) and 15 .. 21 (k = 14 and 15 score 7); one
    # sample of block 5 at full scale charges clip_weight = 4 to every window over it: k = 14 (nearer the centre than 15)
    n = W + 16 * H
    x = on_blocks(n, W, [(2, 10), (15, 22)], 6)
    x[5 * H + 100] = 1.0
    rows.append(Row("clipped_densest", f32(x), W, start=14 * H))
    rows.append(Row("clipped_weight0", f32(x), W, clip_weight=0, start=2 * H))
    rows.append(Row("all_zero", np.zeros(5000, np.float32), W, start=(5000 - W) // 2))
    # the early row with exact zeros over blocks 12 .. 19: Emin = 0, the range term alone sets the threshold
    x = on_blocks(W + 20 * H, W, [(0, 10)], 7)
    x[12 * H: 20 * H] = 0.0
    rows.append(Row("zero_gap", f32(x), W, start=2 * H))
    # W = H: n = 990, s_c = 375, o = 135, F = 3 (below the smoothing length: Emin = min e), k = 0 .. 2, k_c = 1; on over block 2
    rows.append(Row("W=H_F3", f32(on_blocks(990, H, [(2, 3)], 8)), H, start=135 + 2 * H))
    rows.append(Row("late_1e-3", f32(1e-3 * late.astype(np.float64)), W, start=18 * H))
    rows.append(Row("late_x20", f32(20.0 * late.astype(np.float64)), W, clip_level=8.0, start=18 * H))
    # 2600 blocks from o = 57: voiced stretches of 3, 5 and 6 blocks, one of 8 blocks at 2001 .. 2008 whose block 2004 clips, and one
    # of 7 at 700 .. 706: k = 699 and 700 score 7, and 700 is the nearer to k_c = 1296
    n = W + 2592 * H + 114
    x = on_blocks(n, W, [(100, 103), (700, 707), (1290, 1295), (2001, 2009), (2500, 2506)], 9)
    x[57 + 2004 * H + 7] = -1.0
    rows.append(Row("blocks2600", f32(x), W, start=57 + 700 * H))
    _BATCH = rows
    return rows


_REF: dict = {}


def reference(row: Row):
    """(float64 parts, float32 parts) of a designed row, computed once and shared."""
    if row.name not in _REF:
        _REF[row.name] = (crop_parts(row.x, row.W, **row.params), crop_parts(row.x, row.W, dtype=np.float32, **row.params))
    return _REF[row.name]


def margin(row: Row) -> float:
    """The smallest |e[f] / thr - 1| of the row in float64: how far the nearest block is from changing sides.  A row without a block,
    or with thr = 0 (every e is then exactly 0 in every precision, and 0 > 0 is false), has nothing that could."""
    p = reference(row)[0]
    if p.F == 0 or p.thr == 0.0:
        return float("inf")
    return float(np.abs(p.e / p.thr - 1.0).min())
