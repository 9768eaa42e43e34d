"""Float64 restatement of the UNPADDED Token2SV and of the speaker-vector cosine, in numpy: where the expected values of
tests/test_spk_host.py and tests/test_gpu_spk.py come from (never from the code under test).

Token2SV, reference src/sopro/nn/speaker.py:37-61 with ``lengths == T`` (how src/sopro/model.py:158-159 makes ``sv_ref``):
  * codebook mix, speaker.py:48-54 (``_get_mixed_embedding`` 33-35): x[t] = sum_q softmax(cb_weights)[q] emb[q V + tok[t, q]];
  * two ``DepthwiseConv1d(d, 7, causal=False)`` + GELU (speaker.py:23-29; src/sopro/nn/blocks.py:63-74: three zeros on each side
    of the T frames in front of EACH conv - the second conv's padding is zeros, not GELU of a conv over padding);
  * ``AttentiveStatsPool`` (blocks.py:174-188): logit = attn.2(tanh(attn.0(h))), softmax over time, mu = sum a h,
    std = sqrt(clamp_min(sum a (h - mu)^2, 1e-6));
  * ``proj`` and ``F.normalize(eps=1e-6)`` (speaker.py:60-61).
Weights: the reference's ``state_dict`` names (what ``sopro_amd.weights.synth_sopro_weights`` returns), any float dtype.
"""
import math

import numpy as np

_erf = np.vectorize(math.erf, otypes=[np.float64])


def gelu(x):
    """torch.nn.GELU() (the erf form)"""
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def dwconv7(x, weight, bias):
    """blocks.py:63-74, non-causal, kernel 7, dilation 1: x [T, C], weight [C, 1, 7], bias [C] -> [T, C]"""
    T, C = x.shape
    xp = np.zeros((T + 6, C), np.float64)
    xp[3: 3 + T] = x
    y = np.zeros((T, C), np.float64)
    for j in range(7):
        y += xp[j: j + T] * weight[:, 0, j][None, :]
    return y + bias[None, :]


def token2sv(tok_tq, w, V, stages=False):
    """tok_tq integer [T, Q], T >= 1 -> sv float64 [sv_student_dim]; ``stages=True``: (sv, h [T, SD], logit [T])."""
    f = lambda k: np.asarray(w["token2sv." + k], np.float64)  # noqa: E731
    tok = np.asarray(tok_tq).astype(np.int64)
    T, Q = tok.shape
    assert T >= 1
    emb = f("emb.weight")
    cbw = f("cb_weights")
    cw = np.exp(cbw - cbw.max())
    cw /= cw.sum()
    x = np.zeros((T, emb.shape[1]), np.float64)
    for q in range(Q):
        x += cw[q] * emb[q * int(V) + tok[:, q]]
    h = gelu(dwconv7(x, f("enc.0.dw.weight"), f("enc.0.dw.bias")))
    h = gelu(dwconv7(h, f("enc.3.dw.weight"), f("enc.3.dw.bias")))
    a1 = np.tanh(h @ f("pool.attn.0.weight").T + f("pool.attn.0.bias"))
    logit = a1 @ f("pool.attn.2.weight")[0] + f("pool.attn.2.bias")[0]
    a = np.exp(logit - logit.max())
    a /= a.sum()
    mu = (a[:, None] * h).sum(0)
    var = (a[:, None] * (h - mu[None, :]) ** 2).sum(0)
    std = np.sqrt(np.maximum(var, 1e-6))
    e = f("proj.weight") @ np.concatenate([mu, std]) + f("proj.bias")
    sv = e / max(float(np.sqrt((e * e).sum())), 1e-6)
    return (sv, h, logit) if stages else sv


def variance_clamped(tok_tq, w, V):
    """How many channels of the pooled variance sit on the 1e-6 clamp (T = 1: all of them)."""
    _, h, logit = token2sv(tok_tq, w, V, stages=True)
    a = np.exp(logit - logit.max())
    a /= a.sum()
    mu = (a[:, None] * h).sum(0)
    return int(((a[:, None] * (h - mu[None, :]) ** 2).sum(0) < 1e-6).sum())


def cosine(a, b):
    """pairwise: a [n, d], b [n, d] -> [n]; a . b / max(|a| |b|, 1e-12)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.maximum(np.sqrt((a * a).sum(-1)) * np.sqrt((b * b).sum(-1)), 1e-12)
    return (a * b).sum(-1) / den


def cosine_bank(a, b):
    """a [na, d] against every b [nb, d] -> [na, nb]"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.maximum(np.sqrt((a * a).sum(-1))[:, None] * np.sqrt((b * b).sum(-1))[None, :], 1e-12)
    return (a @ b.T) / den


def designed_rows(tile):
    """Row lengths of the GPU test and what each is there for (``tile`` = hip.SPK_TILE_FRAMES)."""
    TF = int(tile)
    return [
        (1, "one frame: both convs see padding only around it; the variance clamp"),
        (2, "shorter than a conv radius"),
        (3, "exactly one radius"),
        (4, "radius + 1"),
        (6, "two radii: the first frame's h still sees the end"),
        (7, "one conv kernel"),
        (TF - 1, "one part-filled tile"),
        (TF, "exactly one tile: no frame beyond it"),
        (TF + 1, "a second tile of one frame: its halo is almost all of its input"),
        (TF + 3, "the end falls one radius into tile 2: h1's zero rule at the end inside tile 1's halo"),
        (TF + 5, "inside the 6-frame halo of tile 1"),
        (TF + 6, "exactly the halo"),
        (TF + 7, "one past the halo"),
        (2 * TF, "two whole tiles"),
        (2 * TF + 1, "three tiles"),
        (150, "the default reference crop (12 s)"),
        (400, "max_frames: many tiles, several passes of the pooling loops"),
        (0, "no frames: a zero vector, nothing read"),
    ]
