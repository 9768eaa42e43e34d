"""Numpy restatement of the speaking-rate operator (WSOLA; the normative definition is the contract comment of ``sopro_tsm_rows_f32``
in include/sopro_hip.h).  ``tsm`` is the one-shot form, ``Stream`` the chunked form written from the streaming paragraph of the
definition on its own (state = block index, last position, samples received, retained tail); tests/test_tsm_host.py checks on the
CPU that the two agree exactly and that the operator does what a time stretch should; tests/test_gpu_tsm.py compares the kernel
with them bit for bit.  Not imported by the package."""
import numpy as np

W, HS, R = 960, 480, 240
SR = 24000
TAB = (0.5 - 0.5 * np.cos(np.pi * (np.arange(HS, dtype=np.float64) + 0.5) / HS)).astype(np.float32)


def step_of(speed):
    v = float(speed)
    if not (0.5 <= v <= 2.0):
        raise ValueError(f"speed must lie in [0.5, 2.0], got {speed!r}")
    return int(round(v * HS * 65536))


def out_len(L, step):
    return (int(L) * HS * 65536) // int(step)


def _at(x, s, n):
    """x[s : s + n], zero-extended past the end"""
    out = np.zeros(n, np.float32)
    if s < len(x):
        seg = x[s: s + n]
        out[: len(seg)] = seg
    return out


def _search(reg, tm, lo):
    """d of least ssd between the template and the windows of the region (reg[0] is x[a + lo]); ties: smaller |d|, then d > 0"""
    m = max(float(np.abs(reg).max()), float(np.abs(tm).max()))
    if not m > 0:
        return 0
    inv = np.float32(127.0) / np.float32(m)
    qr = np.rint(reg * inv).astype(np.int32)
    qt = np.rint(tm * inv).astype(np.int32)
    win = np.lib.stride_tricks.sliding_window_view(qr, W)  # [R - lo + 1, W]
    ssd = ((win - qt[None, :]) ** 2).sum(1)
    ds = np.arange(lo, R + 1)
    key = ssd.astype(np.int64) * 4096 + np.abs(ds) * 2 + (ds < 0)
    return int(ds[int(key.argmin())])


def _mix(A, B):
    return A + TAB * (B - A)  # three float32 operations, each rounded


def tsm(x, speed, want_deltas=False):
    """x [L] float32 -> y [M] (and the chosen offsets d_k [K])."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    L, step = len(x), step_of(speed)
    M = out_len(L, step)
    K = -(-M // HS)
    y = np.zeros(K * HS, np.float32)
    deltas = np.zeros(K, np.int32)
    p_prev = 0
    for k in range(K):
        if k == 0:
            y[:HS] = _at(x, 0, HS)
            continue
        a = (k * step) >> 16
        t = p_prev + HS
        lo = max(-R, -a)
        d = _search(_at(x, a + lo, W + R - lo), _at(x, t, W), lo)
        deltas[k] = d
        p = a + d
        y[k * HS: (k + 1) * HS] = _mix(_at(x, t, HS), _at(x, p, HS))
        p_prev = p
    return (y[:M], deltas) if want_deltas else y[:M]


class Stream:
    """The chunked form: ``feed(chunk)`` returns the samples (and offsets) of the blocks that became computable, ``flush()`` the rest."""

    def __init__(self, speed):
        self.step = step_of(speed)
        self.k = 0
        self.p_prev = 0
        self.received = 0
        self.base = 0                       # absolute position of tail[0]
        self.tail = np.zeros(0, np.float32)
        self.max_tail = 0

    def _x(self, s, n):  # absolute positions; zero past what was received
        assert s >= self.base, "the retained tail was cut too short"
        return _at(self.tail, s - self.base, n)

    def _block(self, k, cut=None):
        if k == 0:
            y, d, p = self._x(0, HS), 0, 0
        else:
            a = (k * self.step) >> 16
            t = self.p_prev + HS
            lo = max(-R, -a)
            d = _search(self._x(a + lo, W + R - lo), self._x(t, W), lo)
            p = a + d
            y = _mix(self._x(t, HS), self._x(p, HS))
        self.p_prev = p
        return (y if cut is None else y[:cut]), d

    def _need(self, k):
        if k == 0:  # whole: all of x[0 : HS) is in, and the output is at least HS long whatever follows
            return max(HS, -(-self.step // 65536))
        a = (k * self.step) >> 16
        return max(self.p_prev + HS, a + R) + W

    def _trim(self):
        if self.k > 0:
            a = (self.k * self.step) >> 16
            nb = max(self.base, min(self.p_prev + HS, a - R))
            nb = min(nb, self.received)
            self.tail = self.tail[nb - self.base:]
            self.base = nb
        self.max_tail = max(self.max_tail, len(self.tail))

    def feed(self, chunk):
        chunk = np.ascontiguousarray(chunk, dtype=np.float32)
        self.tail = np.concatenate([self.tail, chunk])
        self.received += len(chunk)
        ys, ds = [], []
        while self.received >= self._need(self.k):
            y, d = self._block(self.k)
            ys.append(y)
            ds.append(d)
            self.k += 1
        self._trim()
        return (np.concatenate(ys) if ys else np.zeros(0, np.float32)), ds

    def flush(self):
        M = out_len(self.received, self.step)
        K = -(-M // HS)
        ys, ds = [], []
        while self.k < K:
            y, d = self._block(self.k, cut=min(HS, M - self.k * HS))
            ys.append(y)
            ds.append(d)
            self.k += 1
        return (np.concatenate(ys) if ys else np.zeros(0, np.float32)), ds


def tsm_chunked(x, speed, sizes):
    """Feed x in chunks of the given sizes (cycled), flush -> (y, deltas, longest retained tail)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    st = Stream(speed)
    ys, ds, i, j = [], [], 0, 0
    while i < len(x):
        n = int(sizes[j % len(sizes)])
        j += 1
        y, d = st.feed(x[i: i + n])
        i += n
        ys.append(y)
        ds += d
    y, d = st.flush()
    ys.append(y)
    ds += d
    return np.concatenate(ys), np.asarray(ds, np.int32), st.max_tail


# ---------------------------------------------------------------------------------------------- signals
def harmonic(f0, seconds=3.0, amp=0.3, harmonics=5):
    t = np.arange(int(seconds * SR)) / SR
    return (sum(np.sin(2 * np.pi * f0 * h * t) / h for h in range(1, harmonics + 1)) * amp).astype(np.float32)


def glide(f_a, f_b, n, amp=0.3, harmonics=4):
    """harmonic tone whose fundamental moves linearly from f_a to f_b over n samples"""
    f = np.linspace(f_a, f_b, n)
    ph = 2 * np.pi * np.cumsum(f) / SR
    return (sum(np.sin(h * ph) / h for h in range(1, harmonics + 1)) * amp).astype(np.float32)


def noise_with_silence(seconds=2.0, seed=0, head=5000, tail=7000, amp=0.1):
    x = (np.random.default_rng(seed).standard_normal(int(seconds * SR)) * amp).astype(np.float32)
    x[:head] = 0
    if tail:
        x[-tail:] = 0
    return x


def peak_hz(y):
    n = len(y)
    sp = np.abs(np.fft.rfft(y * np.hanning(n)))
    return float(np.argmax(sp)) * SR / n
