"""Numpy restatement of the audio watermark (the normative definition is the contract comment of ``sopro_wm_embed_rows_f32`` and
its neighbours in include/sopro_hip.h).  ``carrier`` / ``templates`` are the host tables, ``embed`` the one-shot embedder,
``Stream`` its chunked form written from the streaming paragraph of the definition on its own, ``detect`` the detector with
float64 sums.  tests/test_wm_host.py checks on the CPU that the pieces agree and that the mark is found where it should be;
tests/test_gpu_wm.py compares the kernels with them.  Not imported by the package."""
from collections import namedtuple

import numpy as np

from tsm_ref import HS, TAB

P, CH, SHIFT, TAGS = 8192, 2, 32, 256
NC = P // CH
THRESHOLD = 6.0
MASK = 0xFFFFFFFF

Result = namedtuple("Result", "present score tag offset z_sync z_tag")


def _fmix(h):
    """The 32-bit finaliser on a uint64 array that holds 32-bit values."""
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(MASK)
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(MASK)
    return h ^ (h >> np.uint64(16))


def lanes(key):
    """c_0, c_1: int8 [P] each, values +-1."""
    key = int(key)
    if not 0 <= key < 1 << 64:
        raise ValueError("key in [0, 2^64)")
    lo, hi = np.uint64(key & MASK), np.uint64(key >> 32)
    i = np.arange(NC, dtype=np.uint64)
    out = []
    for lane in (0, 1):
        h = _fmix((i * np.uint64(0x9E3779B1) + lo) & np.uint64(MASK))
        h = _fmix(h ^ hi ^ np.uint64((lane * 0x7F4A7C15) & MASK))
        s = np.where((h >> np.uint64(31)) & np.uint64(1), -1, 1).astype(np.int8)
        out.append(np.repeat(s, CH))
    return out[0], out[1]


def carrier(key, tag):
    """int8 [P]: c_0[n] + c_1[(n - SHIFT * tag) mod P]."""
    tag = int(tag)
    if not 0 <= tag < TAGS:
        raise ValueError("tag in [0, 256)")
    c0, c1 = lanes(key)
    return (c0 + np.roll(c1, SHIFT * tag)).astype(np.int8)


def templates(key):
    """int8 [2, P]: d_l[n] = c_l[n] - c_l[(n - 1) mod P]."""
    c0, c1 = lanes(key)
    return np.stack([c0 - np.roll(c0, 1), c1 - np.roll(c1, 1)]).astype(np.int8)


def alpha_of(strength_db):
    return np.float32(10.0 ** (float(strength_db) / 20.0))


def envelope(x):
    """g [L] float32 of a row (zero-extended)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    L = len(x)
    if L == 0:
        return np.zeros(0, np.float32)
    K = -(-L // HS)
    pad = np.zeros((K + 1) * HS, np.float32)
    pad[:L] = np.abs(x)
    b = pad.reshape(K + 1, HS).max(1)                       # b_j = max |x| over block j
    e = np.maximum(np.concatenate([[np.float32(0)], b]), np.concatenate([b, [np.float32(0)]])).astype(np.float32)  # e_k, k = 0 .. K + 1
    n = np.arange(L)
    k, r = n // HS, n % HS
    return (e[k] + TAB[r] * (e[k + 1] - e[k])).astype(np.float32)  # three float32 operations, each rounded


def _mark(x, g, alpha, car, n0):
    cf = np.float32(0.5) * car[(n0 + np.arange(len(x))) % P].astype(np.float32)
    return (x + (np.float32(alpha) * g) * cf).astype(np.float32)


def embed(x, key, tag=0, strength_db=-30.0):
    """x [L] float32 -> y [L]; ``key=None``: a copy."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if key is None:
        return x.copy()
    return _mark(x, envelope(x), alpha_of(strength_db), carrier(key, tag), 0)


class Stream:
    """The chunked form: ``feed(chunk)`` returns the samples of the blocks that became computable, ``flush()`` the rest."""

    def __init__(self, key, tag=0, strength_db=-30.0):
        self.car = carrier(key, tag) if key is not None else None
        self.alpha = alpha_of(strength_db)
        self.k = 0                          # next block; k * HS samples were emitted
        self.received = 0
        self.base = 0                       # absolute position of tail[0]
        self.tail = np.zeros(0, np.float32)
        self.max_tail = 0

    def _x(self, s, n):  # absolute positions [s, s + n); zero below 0 and past what was received
        out = np.zeros(n, np.float32)
        a, b = max(s, 0), min(s + n, self.received)
        if b > a:
            assert a >= self.base, "the retained tail was cut too short"
            out[a - s: b - s] = self.tail[a - self.base: b - self.base]
        return out

    def _block(self, k, cut=HS):
        x = self._x(k * HS, HS)
        if self.car is None:
            return x[:cut]
        e0 = np.float32(np.abs(self._x((k - 1) * HS, 2 * HS)).max())
        e1 = np.float32(np.abs(self._x(k * HS, 2 * HS)).max())
        g = (e0 + TAB * (e1 - e0)).astype(np.float32)
        return _mark(x, g, self.alpha, self.car, k * HS)[:cut]

    def feed(self, chunk):
        chunk = np.ascontiguousarray(chunk, dtype=np.float32)
        self.tail = np.concatenate([self.tail, chunk])
        self.received += len(chunk)
        ys = []
        while self.received >= (self.k + 2) * HS:
            ys.append(self._block(self.k))
            self.k += 1
        nb = min(max(self.base, (self.k - 1) * HS), self.received)
        self.tail = self.tail[nb - self.base:]
        self.base = nb
        self.max_tail = max(self.max_tail, len(self.tail))
        return np.concatenate(ys) if ys else np.zeros(0, np.float32)

    def flush(self):
        L = self.received
        ys = []
        while self.k * HS < L:
            ys.append(self._block(self.k, cut=min(HS, L - self.k * HS)))
            self.k += 1
        self.k = self.received = self.base = 0  # a fresh row
        self.tail = np.zeros(0, np.float32)
        return np.concatenate(ys) if ys else np.zeros(0, np.float32)


def embed_chunked(x, sizes, key, tag=0, strength_db=-30.0):
    """Feed x in chunks of the given sizes (cycled), flush -> (y, longest retained tail)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    st = Stream(key, tag, strength_db)
    ys, i, j, longest = [], 0, 0, 0
    while i < len(x):
        n = int(sizes[j % len(sizes)])
        j += 1
        ys.append(st.feed(x[i: i + n]))
        longest = max(longest, st.max_tail)
        i += n
    ys.append(st.flush())
    return np.concatenate(ys), longest


# ---------------------------------------------------------------------------------------------- detector
def whiten(y):
    """u [L] float32 (steps 1 of the detector) and pk."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    L = len(y)
    if L == 0:
        return np.zeros(0, np.float32), np.float32(0)
    w = y.copy()
    w[1:] = y[1:] - y[:-1]
    g = envelope(y)
    pk = np.float32(np.abs(y).max())
    ok = g > np.float32(1e-3) * pk
    u = np.zeros(L, np.float32)
    u[ok] = w[ok] / g[ok]
    return u, pk


def fold(u, dtype=np.float64):
    """f [P]: the sum over m of u[r + m P] (float64 unless asked otherwise) and the sum of |u| alongside."""
    L = len(u)
    pad = np.zeros(-(-max(L, 1) // P) * P, dtype)
    pad[:L] = u
    rows = pad.reshape(-1, P)
    return rows.sum(0), np.abs(rows).sum(0)


def correlate(f, d):
    """R [P] float64: R[o] = sum_n f[(n + o) mod P] d[n], by FFT (float64: far below the fp32 bounds of the tests)."""
    F = np.fft.rfft(np.asarray(f, np.float64))
    D = np.fft.rfft(np.asarray(d, np.float64))
    return np.fft.irfft(F * np.conj(D), P)


def correlate_at(f, d, offsets):
    """The same sum, term by term in float64, at a few offsets -> (R, sum of |terms|)."""
    f = np.asarray(f, np.float64)
    d = np.asarray(d, np.float64)
    n = np.arange(P)
    R = np.array([np.sum(f[(n + o) % P] * d) for o in offsets])
    A = np.array([np.sum(np.abs(f[(n + o) % P] * d)) for o in offsets])
    return R, A


def peak(R):
    """(o, z) of one lane."""
    o = int(np.argmax(R))
    sd = float(np.std(R))
    return o, (float((R[o] - np.mean(R)) / sd) if sd > 0 else 0.0)


def detect(y, key, details=False):
    """y [L] float32 -> Result (and, with ``details``, a dict of the intermediate u, f, R)."""
    u, pk = whiten(y)
    f, fa = fold(u)
    d = templates(key)
    R = np.stack([correlate(f, d[0]), correlate(f, d[1])])
    if len(u) == 0 or not pk > 0:
        res = Result(False, 0.0, 0, 0, 0.0, 0.0)
    else:
        (o0, z0), (o1, z1) = peak(R[0]), peak(R[1])
        tag = ((((o1 - o0) % P) + SHIFT // 2) // SHIFT) % TAGS
        score = min(z0, z1)
        res = Result(bool(score >= THRESHOLD), score, tag, o0, z0, z1)
    return (res, dict(u=u, f=f, fa=fa, R=R, d=d, pk=pk)) if details else res


# ---------------------------------------------------------------------------------------------- what a clip goes through
def pcm16(y):
    """16-bit quantisation and back."""
    q = np.rint(np.clip(np.asarray(y, np.float32), -1.0, 1.0) * np.float32(32767.0)).astype(np.int16)
    return (q.astype(np.float32) / np.float32(32768.0)).astype(np.float32)


def crop(y, a=3001, b=-1777):
    return np.ascontiguousarray(y[a:b])


def degrade(y, gain=0.37):
    """PCM16, crop [3001:-1777], gain: the middle column of the detection table."""
    return (crop(pcm16(y)) * np.float32(gain)).astype(np.float32)


def add_noise(y, db=-40.0, seed=11):
    """White noise whose standard deviation is ``db`` below the clip's peak."""
    y = np.asarray(y, np.float32)
    sd = float(np.abs(y).max()) * 10.0 ** (db / 20.0)
    return (y + np.random.default_rng(seed).standard_normal(len(y)).astype(np.float32) * np.float32(sd)).astype(np.float32)


def pinkish(seconds=3.0, seed=3, amp=0.3):
    """A low-passed random walk: leaky integration of white noise (pole 0.995), smoothed over 4 samples, peak ``amp``."""
    n = int(seconds * 24000)
    w = np.random.default_rng(seed).standard_normal(n)
    x = np.zeros(n)
    acc = 0.0
    for i in range(n):
        acc = 0.995 * acc + w[i]
        x[i] = acc
    x = np.convolve(x, np.ones(4) / 4.0, mode="same")
    return (x * (amp / np.abs(x).max())).astype(np.float32)
