"""CPU restatement of the word-timestamp contract (DESIGN.md "Word timestamps", include/sopro_hip.h "word timestamps"): the yardstick
the GPU tests compare ``hip.align_scores`` / ``hip.align_paths`` / ``SoproTTSModel.align_batch`` (sopro_amd/replay.py) with.  Written from the definition;
it shares no code with sopro_amd/.  The recurrence and the backtrack are numpy fp32, one frame at a time; the teacher-forced replay is plain
torch in a dtype of the caller's choice (float32: the contract; float64: the error model the tests derive their tolerances from).
tests/test_align_host.py checks ``dp`` against brute-force enumeration and ``replay`` against the oracle's own blocks."""
import itertools
import math

import numpy as np
import torch
import torch.nn.functional as F

FLOOR = 1e-9
DH = 96


# ------------------------------------------------------------------------------------------ the path
def fallback(T, S):
    """Rows without a monotonic path (T < S, T == 0 or S == 0): frames spread evenly."""
    path = [(t * S) // T for t in range(T)] if S > 0 else [0] * T
    bounds = []
    for s in range(S):
        f = (s * T + S - 1) // S if T > 0 else 0
        hit = 1 if (T > 0 and f < T and (f * S) // T == s) else 0
        bounds.append((f, f + hit))
    return path, bounds, np.float32(0.0), 1


def dp(score):
    """score [T, S] -> (path [T], bounds [S] of (first frame, last frame + 1), total fp32, status)."""
    sc = np.asarray(score, dtype=np.float32)
    T, S = (int(v) for v in sc.shape) if sc.ndim == 2 else (0, 0)
    if T < S or T == 0 or S == 0:
        return fallback(T, S)
    ninf = np.float32(-np.inf)
    D = np.full((T, S), ninf, dtype=np.float32)
    back = np.zeros((T, S), dtype=bool)
    D[0, 0] = sc[0, 0]
    for t in range(1, T):  # (the cells of a frame do not depend on each other: one numpy row operation per frame, fp32 throughout)
        stay = D[t - 1]
        left = np.concatenate([np.array([ninf], np.float32), D[t - 1, :-1]])
        take = left > stay  # strictly: ties stay
        back[t] = take
        D[t] = sc[t] + np.where(take, left, stay)  # one fp32 add per cell
    path = [0] * T
    s = S - 1
    for t in range(T - 1, 0, -1):
        path[t] = s
        s -= int(back[t, s])
    path[0] = s
    bounds = [[None, None] for _ in range(S)]
    for t in range(T):
        if t == 0 or path[t - 1] != path[t]:
            bounds[path[t]][0] = t
        if t == T - 1 or path[t + 1] != path[t]:
            bounds[path[t]][1] = t + 1
    return path, [tuple(b) for b in bounds], D[T - 1, S - 1], 0


def monotone_paths(T, S):
    """Every path with path[0] = 0, path[T-1] = S-1 and steps of 0 or 1 (T >= S >= 1)."""
    for ups in itertools.combinations(range(1, T), S - 1):
        path, s, up = [], 0, set(ups)
        for t in range(T):
            s += 1 if t in up else 0
            path.append(s)
        yield path


def path_total(score, path):
    """The path's score as the recurrence adds it up: frame by frame, in fp32."""
    sc = np.asarray(score, dtype=np.float32)
    acc = sc[0, path[0]]
    for t in range(1, len(path)):
        acc = np.float32(sc[t, path[t]] + acc)
    return acc


def brute(score):
    """(best total, every path that reaches it) by enumeration."""
    sc = np.asarray(score, dtype=np.float32)
    T, S = sc.shape
    best, who = None, []
    for p in monotone_paths(T, S):
        v = path_total(sc, p)
        if best is None or v > best:
            best, who = v, [p]
        elif v == best:
            who.append(p)
    return best, who


# ------------------------------------------------------------------------------------------ the scores
def head_probs(q, k, dtype=torch.float32):
    """q [T, H * 96], k [S, H * 96] -> P [H, T, S] = softmax over s of q_t,h . k_s,h / sqrt(96)."""
    T, S = q.shape[0], k.shape[0]
    H = q.shape[1] // DH
    qh = q.to(dtype).view(T, H, DH).transpose(0, 1)
    kh = k.to(dtype).view(S, H, DH).transpose(0, 1)
    return torch.softmax(torch.matmul(qh, kh.transpose(1, 2)) / math.sqrt(DH), dim=-1)


def mean_probs(qk, heads=None, dtype=torch.float32):
    """qk: {layer: (q [T, D], k [S, D])} -> A [T, S], the mean of P over the selected (layer, head) pairs (default: all)."""
    sel = [(l, h) for l in sorted(qk) for h in range(qk[l][0].shape[1] // DH)] if heads is None else [(int(l), int(h)) for l, h in heads]
    P = {l: head_probs(qk[l][0], qk[l][1], dtype) for l in sorted({l for l, _h in sel})}
    A = None
    for l, h in sel:
        A = P[l][h] / len(sel) if A is None else A + P[l][h] / len(sel)
    return A


def log_scores(A):
    return torch.log(torch.clamp(A, min=FLOOR))


def scores_layer(q, k, head_mask, weight, dtype=torch.float32):
    """One launch's contribution: sum over the heads in ``head_mask`` of weight * P_h -> [T, S]."""
    P = head_probs(q, k, dtype)
    out = torch.zeros(q.shape[0], k.shape[0], dtype=dtype)
    for h in range(P.shape[0]):
        if (head_mask >> h) & 1:
            out = out + weight * P[h]
    return out


# ------------------------------------------------------------------------------------------ the teacher-forced replay
def _rms(x, wt, eps=1e-6):
    return x * torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + eps) * wt


def _block(x, w, p, dil):
    """Full-sequence causal SSM block on x [1, T, D] (GLU projection, causal depthwise conv, residual, feed-forward, residual)."""
    y = F.linear(_rms(x, w[p + ".norm.weight"]), w[p + ".glu.pro.weight"], w[p + ".glu.pro.bias"])
    a, b = y.chunk(2, dim=-1)
    h = a * torch.sigmoid(b)
    wt = w[p + ".dw.dw.weight"]
    k = int(wt.shape[-1])
    h = F.conv1d(F.pad(h.transpose(1, 2), ((k - 1) * dil, 0)), wt, w[p + ".dw.dw.bias"], dilation=dil, groups=wt.shape[0]).transpose(1, 2)
    x = x + h
    f = F.linear(_rms(x, w[p + ".ff.0.weight"]), w[p + ".ff.1.weight"], w[p + ".ff.1.bias"])
    f = F.linear(F.gelu(f), w[p + ".ff.3.weight"], w[p + ".ff.3.bias"])
    return x + f


def replay(w, cfg, cond_td, tokens_t, txt_sd, dtype=torch.float32, hidden=None):
    """The AR stack teacher-forced over T frames -> {layer: (q [T, D], k [S, D])} for the cross-attention layers.
    cond_td [>= T, D] conditioning rows, tokens_t [T] codebook-0 tokens, txt_sd [S, D] encoded text.  ``hidden``: a list that
    receives the stream after every block (+ attention), for the cross-check against the oracle."""
    w = {k: v.to(dtype) for k, v in w.items() if k.startswith(("ar.", "cb_embed."))}
    T = int(len(tokens_t))
    E = w["cb_embed.emb.weight"]
    prev = torch.tensor([int(cfg.bos_row)] + [int(v) for v in tokens_t[: T - 1]], dtype=torch.long)
    x = (cond_td[:T].to(dtype) + E[prev]).unsqueeze(0)
    txt = txt_sd.to(dtype).unsqueeze(0)
    out = {}
    for i, dil in enumerate(cfg.ar_dilations):
        x = _block(x, w, f"ar.blocks.{i}", int(dil))
        if i in cfg.ar_xattn_layers:
            p = f"ar.x_attns.{i}"
            kvn = _rms(txt, w[p + ".nkv.weight"])
            k, v = F.linear(kvn, w[p + ".k_proj.weight"]), F.linear(kvn, w[p + ".v_proj.weight"])
            q = F.linear(_rms(x, w[p + ".nq.weight"]), w[p + ".q_proj.weight"])
            out[i] = (q[0], k[0])
            P = head_probs(q[0], k[0], dtype)                                   # [H, T, S]
            H = P.shape[0]
            a = torch.matmul(P, v[0].view(-1, H, DH).transpose(0, 1))           # [H, T, dh]
            a = a.transpose(0, 1).reshape(1, T, H * DH)
            x = x + torch.tanh(w[p + ".gate"]) * F.linear(a, w[p + ".out_proj.weight"])
        if hidden is not None:
            hidden.append(x[0])
    return out


def utterance_scores(w, cfg, cond_td, tokens_t, txt_sd, heads=None, dtype=torch.float32):
    """-> (score [T, S] = log(max(A, 1e-9)), A [T, S]) of one utterance."""
    A = mean_probs(replay(w, cfg, cond_td, tokens_t, txt_sd, dtype), heads, dtype)
    return log_scores(A), A
