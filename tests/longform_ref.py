"""Numpy restatement of the long-form join's contract (include/sopro_hip.h, "long-form join"): the yardstick the GPU tests compare
``hip.join_segments`` with, bit for bit.  Written from the definition, sample by sample where that is affordable and with plain
numpy reductions otherwise; it shares no code with sopro_amd/.  tests/test_longform_host.py checks it against hand-computed cases."""
import numpy as np


def fade_table(fade_len):
    m = np.arange(int(fade_len), dtype=np.float64)
    return (0.5 - 0.5 * np.cos(np.pi * (m + 0.5) / fade_len)).astype(np.float32) if fade_len > 0 else np.zeros(0, np.float32)


def row_edges(x, L, *, hop=240, rel=0.01, keep=3, trim=True):
    """(start, end) of one row; ``x``: the row's samples (only x[:L] is looked at)."""
    L = int(L)
    if not trim:
        return 0, L
    if L == 0:
        return 0, 0
    a = np.abs(np.asarray(x[:L], dtype=np.float32))
    peak = np.float32(a.max())
    if peak == 0:
        return 0, 0
    thr = np.float32(np.float32(rel) * peak)  # one fp32 multiply
    n_hops = -(-L // hop)
    active = [j for j in range(n_hops) if np.float32(a[j * hop: min((j + 1) * hop, L)].max()) >= thr]
    first, last = active[0], active[-1]
    return max(0, (first - keep) * hop), min(L, (last + 1 + keep) * hop)


def join(wav, lens, gaps, *, hop=240, rel=0.01, keep=3, fade_len=120, trim=True):
    """wav [n_seg, >= max(lens)] float32 -> (out float32 [total], edges int [n_seg, 2], offs int64 [n_seg + 1])."""
    wav = np.asarray(wav, dtype=np.float32)
    n_seg = len(lens)
    edges = np.zeros((n_seg, 2), dtype=np.int64)
    for k in range(n_seg):
        edges[k] = row_edges(wav[k], lens[k], hop=hop, rel=rel, keep=keep, trim=trim)
    offs = np.zeros(n_seg + 1, dtype=np.int64)
    for k in range(n_seg):
        n_k = int(edges[k, 1] - edges[k, 0])
        offs[k + 1] = offs[k] + (n_k + int(gaps[k]) if n_k > 0 else 0)
    tab = fade_table(fade_len)
    out = np.zeros(int(offs[n_seg]), dtype=np.float32)
    for k in range(n_seg):
        s, e = int(edges[k, 0]), int(edges[k, 1])
        n_k = e - s
        if n_k <= 0:
            continue
        F = min(int(fade_len), n_k // 2)
        g = np.ones(n_k, dtype=np.float32)
        for i in range(F):
            g[i] = tab[i]
            g[n_k - 1 - i] = tab[i]  # i' = n_k - 1 - i >= n_k - F takes tab[n_k - 1 - i'] = tab[i]
        out[offs[k]: offs[k] + n_k] = wav[k, s:e] * g  # float32 * float32 -> one rounding per sample
    return out, edges, offs


DESIGNED_STRIDE = 50 * 1920 + 64
DESIGNED_LENS = [96000, 0, 100, 71047, 95999, 5000, 3840]
DESIGNED_GAPS = [6000, 6000, 2880, 6000, 0, 6000, 0]
# hand-derived from the layout below with hop 240, rel 0.01, keep 3 (any noise seed gives these integers, up to the negligible chance
# that a whole 240-sample hop of unit noise stays below 1 % of the peak)
DESIGNED_EDGES = [[11280, 79920], [0, 0], [0, 100], [0, 71047], [95040, 95999], [0, 0], [960, 2880]]
DESIGNED_TOTAL = 157546


def designed_batch(seed=0):
    """The operator test's batch: 7 rows of stride 50 * 1920 + 64.  Row 0: unit-peak noise between samples 12000 and 79200 over a
    -60 dB floor; row 1 empty; row 2 shorter than a hop; row 3 noise throughout; row 4 a single 0.5 click at sample 95998; row 5
    all zero; row 6 ones at 1900 .. 1949.  Every sample past a row's length is 777.0."""
    rng = np.random.default_rng(seed)
    wav = np.zeros((7, DESIGNED_STRIDE), dtype=np.float32)

    def unit_noise(n):
        v = rng.standard_normal(n).astype(np.float32)
        return (v / np.abs(v).max()).astype(np.float32)

    wav[0, :96000] = np.float32(1e-3) * unit_noise(96000)
    wav[0, 12000:79200] = unit_noise(79200 - 12000)
    wav[2, :100] = unit_noise(100)
    wav[3, :71047] = unit_noise(71047)
    wav[4, 95998] = 0.5
    wav[6, 1900:1950] = 1.0
    for k, L in enumerate(DESIGNED_LENS):
        wav[k, L:] = 777.0
    return wav, list(DESIGNED_LENS), list(DESIGNED_GAPS)
