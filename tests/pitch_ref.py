"""Numpy restatement of the pitch resampler (the normative definition is the contract comment of ``sopro_pitch_rows_f32`` in
include/sopro_hip.h).  ``resample`` is the one-shot form, ``Stream`` the chunked form written from the chunked paragraph of the
definition on its own (state = next output index, samples received, retained tail), ``chain`` the public ``pitch=`` / ``speed=``
pair: the stretch of tests/tsm_ref.py at ``step'`` followed by the resampler.  tests/test_pitch_host.py checks on the CPU that the
two forms agree exactly and that the operator does what a pitch shift should; tests/test_gpu_pitch.py compares the kernel with them
bit for bit.  Not imported by the package."""
import numpy as np

import tsm_ref as T

NT, P, HALF = 64, 256, 32
ONE = 1 << 32
INC_MIN, INC_MAX = 1 << 31, 1 << 33
SR = 24000
BETA = 7.0
FC_MARGIN = 0.034
IDENTITY_STEP = T.HS << 16


def inc_of(semitones):
    v = float(semitones)
    if not (-12.0 <= v <= 12.0):  # (NaN fails both comparisons)
        raise ValueError(f"pitch must lie in [-12, 12] semitones, got {semitones!r}")
    return min(INC_MAX, max(INC_MIN, int(round(2.0 ** (v / 12.0) * 4294967296.0))))


def out_len(L, inc):
    return (int(L) << 32) // int(inc)


def steps_of(speed, pitch):
    """(step', inc): the stretch's step and the resampler's increment of a (speed, pitch) pair"""
    step, inc = T.step_of(speed), inc_of(pitch)
    sp = int(round(float(speed) * T.HS * 65536 * 4294967296.0 / inc))
    if not (T.HS << 15) <= sp <= (T.HS << 17):
        raise ValueError(f"speed={speed!r} with pitch={pitch!r}: speed / 2^(pitch / 12) must lie in [0.5, 2]")
    if inc == ONE:
        assert sp == step
    return sp, inc


_banks = {}


def bank(inc):
    """float32 [P + 1, NT]: the windowed-sinc rows of an increment, each normalised to sum 1 in float64"""
    key = max(int(inc), ONE)  # every inc <= 2^32 has the bank of 2^32
    b = _banks.get(key)
    if b is None:
        fc = 0.5 * min(1.0, ONE / key) - FC_MARGIN
        p = np.arange(P + 1, dtype=np.float64)[:, None]
        j = np.arange(NT, dtype=np.float64)[None, :]
        t = j - (HALF - 1) - p / P
        u = 1.0 - (t / HALF) ** 2
        w = np.where(u > 0.0, np.i0(BETA * np.sqrt(np.maximum(u, 0.0))) / np.i0(BETA), 0.0)
        g = 2.0 * fc * np.sinc(2.0 * fc * t) * w
        g = g / g.sum(axis=1, keepdims=True)
        b = _banks[key] = g.astype(np.float32)
    return b


def _samples(xp, base, n0, n1, inc):
    """y[n0 .. n1) from xp, where xp[k] = x[base + k] holds every sample the outputs read (zeros where the row has none)"""
    n = np.arange(n0, n1, dtype=np.uint64)
    if inc == ONE:
        return xp[(n.astype(np.int64) - base)].astype(np.float32)
    pos = n * np.uint64(inc)
    i = (pos >> np.uint64(32)).astype(np.int64)
    fr = (pos & np.uint64(0xFFFFFFFF)).astype(np.int64)
    p = fr >> 24
    f = (fr & 0xFFFFFF).astype(np.float32) * np.float32(2.0 ** -24)
    b = bank(inc)
    acc = np.zeros(len(n), np.float32)
    for j in range(NT):
        h0, h1 = b[p, j], b[p + 1, j]
        c = h0 + f * (h1 - h0)                            # three float32 operations, each rounded
        acc = acc + c * xp[i - (HALF - 1) + j - base]     # two more
    return acc


def resample(x, inc):
    """x [L] float32 -> y [M], M = (L << 32) // inc."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    inc = int(inc)
    assert INC_MIN <= inc <= INC_MAX
    L = len(x)
    M = out_len(L, inc)
    if M == 0:
        return np.zeros(0, np.float32)
    xp = np.concatenate([np.zeros(HALF - 1, np.float32), x, np.zeros(HALF + 2, np.float32)])  # x[-31 .. L + 34)
    return _samples(xp, -(HALF - 1), 0, M, inc)


def shift(x, pitch):
    return resample(x, inc_of(pitch))


def chain(x, speed=1.0, pitch=0.0):
    """What ``synthesize(speed=, pitch=)`` does to the decoded waveform x: the stretch at step', then the resampler at inc; a stage
    at its identity is skipped."""
    sp, inc = steps_of(speed, pitch)
    y = np.ascontiguousarray(x, dtype=np.float32)
    if sp != IDENTITY_STEP:
        v = sp / (T.HS * 65536)
        assert T.step_of(v) == sp  # (tsm_ref takes a rate: this one gives back the step exactly)
        y = T.tsm(y, v)
    if inc != ONE:
        y = resample(y, inc)
    return y


def shift_sample(sample, inc):
    return (int(sample) << 32) // int(inc)


class Stream:
    """The chunked form: ``feed(chunk)`` returns the outputs that became computable, ``flush()`` the rest."""

    def __init__(self, inc):
        self.inc = int(inc)
        self.n = 0                          # next output index
        self.received = 0
        self.base = 0                       # absolute position of tail[0]
        self.tail = np.zeros(0, np.float32)
        self.max_tail = 0

    def _i(self, n):
        return (n * self.inc) >> 32

    def _run(self, n1):
        n0, self.n = self.n, max(self.n, n1)
        if self.n == n0:
            return np.zeros(0, np.float32)
        lo = self._i(n0) - (HALF - 1)
        hi = self._i(self.n - 1) + HALF + 1
        assert lo >= self.base or lo < 0, "the retained tail was cut too short"
        xp = np.zeros(hi - lo, np.float32)  # xp[k] = x[lo + k], zero outside [base, received)
        a, b = max(lo, self.base), min(hi, self.received)
        if b > a:
            xp[a - lo: b - lo] = self.tail[a - self.base: b - self.base]
        return _samples(xp, lo, n0, self.n, self.inc)

    def feed(self, chunk):
        chunk = np.ascontiguousarray(chunk, dtype=np.float32)
        self.tail = np.concatenate([self.tail, chunk])
        self.received += len(chunk)
        n1 = self.n
        while self._i(n1) + HALF < self.received:  # (the definition's rule, one output at a time)
            n1 += 1
        y = self._run(n1)
        nb = min(max(self.base, self._i(self.n) - (HALF - 1)), self.received)
        self.tail = self.tail[nb - self.base:]
        self.base = nb
        self.max_tail = max(self.max_tail, len(self.tail))
        return y

    def flush(self):
        return self._run(out_len(self.received, self.inc))


def resample_chunked(x, inc, sizes):
    """Feed x in chunks of the given sizes (cycled), flush -> (y, longest retained tail)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    st = Stream(inc)
    ys, i, j = [], 0, 0
    while i < len(x):
        n = int(sizes[j % len(sizes)])
        j += 1
        ys.append(st.feed(x[i: i + n]))
        i += n
    ys.append(st.flush())
    return np.concatenate(ys), st.max_tail


def sine(hz, seconds=2.0, amp=0.5):
    return (amp * np.sin(2 * np.pi * hz * np.arange(int(seconds * SR)) / SR)).astype(np.float32)
