"""CPU restatement of the online path operator (DESIGN.md "Word timestamps", include/sopro_hip.h ``sopro_align_online_f32``): the
yardstick ``hip.align_online`` and ``SoproTTS.stream_timed`` are compared with.  Written from the definition in numpy fp32, one
frame at a time over the full width of the text (no band, no wave); it shares no code with sopro_amd/.

One row has S >= 1 text positions and fp32 scores score[t][s].  Frames arrive in steps; the lag is L >= 0 frames.  Per-row state:
c, the last committed frame (initially -1); p, the position of frame c (initially -1: a virtual position left of 0); base, the fp32
score of the committed path (initially 0); status.  A step is step(t1, final) with frames [0, t1) scored; a = c + 1, n = t1 - a:

  1. n <= 0: nothing.  Not final and t1 - 1 - L < a: nothing.
  2. the virtual previous row E has E[p] = base and -inf everywhere else;
  3. D[t][s] = score[t][s] + max(D[t-1][s], D[t-1][s-1]) for t = a .. t1 - 1 with D[a-1] = E: one fp32 add per cell; the cell came
     from s - 1 only when the left value is strictly greater (p = -1 makes frame 0 land on position 0 without a special case);
  4. the end e: S - 1 with status 0 when the step is final and D[t1-1][S-1] is finite; else the lowest s that maximises D[t1-1][s],
     with status 2 when final (the text was not finished: positions above e get empty ranges at T), 0 otherwise;
  5. backtrack from (t1 - 1, e);
  6. commit frames a .. u, u = t1 - 1 when final, else t1 - 1 - L: path[a..u] is final, base += score[t][path[t]] in frame order,
     c = u, p = path[u].

A window of more than 63 frames is outside the operator (the device form holds one band position per lane): ``step`` raises.
"""
import numpy as np

WINDOW_MAX = 63


class Online:
    """One row's state and committed path."""

    def __init__(self, S, lag):
        self.S, self.lag = int(S), int(lag)
        self.c, self.p, self.status, self.e = -1, -1, 0, 0
        self.base = np.float32(0.0)
        self.path = []  # committed frames only

    def state(self):
        return (self.c, self.p, self.status, self.e)

    def step(self, score, t1, final):
        """``score``: [>= t1, >= S] fp32, frames [0, t1) valid -> the newly committed path slice (a list, maybe empty)."""
        sc = np.asarray(score, dtype=np.float32)
        S, L = self.S, self.lag
        a = self.c + 1
        n = int(t1) - a
        if n <= 0 or S <= 0:
            return []
        if not final and t1 - 1 - L < a:
            return []
        if n > WINDOW_MAX:
            raise ValueError(f"a window of {n} frames (at most {WINDOW_MAX})")
        ninf = np.float32(-np.inf)
        # positions -1 .. S-1 live at index s + 1, so that the virtual position -1 needs no special case
        prev = np.full(S + 1, ninf, dtype=np.float32)
        prev[self.p + 1] = self.base
        back = np.zeros((n, S + 1), dtype=bool)
        for k in range(n):
            row = np.concatenate([np.array([ninf], np.float32), sc[a + k, :S]])  # (position -1 never scores)
            left = np.concatenate([np.array([ninf], np.float32), prev[:-1]])
            take = left > prev  # strictly: ties stay
            back[k] = take
            cur = (row + np.where(take, left, prev)).astype(np.float32)  # one fp32 add per cell
            cur[0] = ninf
            prev = cur
        D = prev[1:]
        if final and np.isfinite(D[S - 1]):
            e, status = S - 1, 0
        else:
            e, status = int(np.argmax(D)), (2 if final else 0)  # (numpy's arg-max is the lowest index among equals)
        pos = [0] * n
        s = e
        for k in range(n - 1, -1, -1):
            pos[k] = s
            s -= int(back[k, s + 1])
        assert s == self.p
        u = (t1 - 1) if final else (t1 - 1 - L)
        new = pos[: u - a + 1]
        for k, s in enumerate(new):
            self.base = np.float32(self.base + sc[a + k, s])
        self.path += new
        self.c, self.p, self.status, self.e = u, new[-1], status, e
        return new


def schedule(T, chunk, stream=False):
    """The steps of a row of T frames that arrive ``chunk`` at a time: [(t1, final)], the last one final (T == 0: one empty final
    step).  ``stream``: the schedule of a generator that learns of the end one frame late - when T is a multiple of ``chunk`` the
    step at T is not final, and a final step with the same T follows."""
    out, t = [], 0
    while t + chunk < T or (stream and t + chunk == T):
        t += chunk
        out.append((t, False))
    out.append((T, True))
    return out


def run(score, chunk, lag, S=None, stream=False):
    """A whole row through ``schedule`` -> the ``Online`` after its final step."""
    sc = np.asarray(score, dtype=np.float32)
    T = int(sc.shape[0])
    row = Online(sc.shape[1] if S is None else S, lag)
    for t1, final in schedule(T, chunk, stream):
        row.step(sc, t1, final)
    return row


def token_frames(path, S, T=None):
    """(first frame, last frame + 1) per text position of a committed path; a position without frames gets an empty range where the
    next position with frames starts (``T`` past the last one)."""
    T = len(path) if T is None else int(T)
    out, t = [], 0
    for s in range(S):
        while t < len(path) and path[t] < s:
            t += 1
        a = t
        while t < len(path) and path[t] == s:
            t += 1
        out.append((a, t) if (a < len(path) and t > a) else ((a, a) if a < len(path) else (T, T)))
    return out
