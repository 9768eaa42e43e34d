"""float64 reference of the fused SEANet decoder kernels at their ABI (include/sopro_hip.h: sopro_seanet_res128_*, _up128_*, _tail_*,
_uptail_*), with the per-element tolerance of every owned output word.

``res128`` / ``up128`` / ``tail`` / ``uptail`` take what the entry points take - flat caller buffers with segment strides and
element offsets, the packed matrices (w1 tap-major [32][3*64] / [64][3*128], w2, wf [3][64], pack_convtr1d's W [256][256] and bias
[256]), ``passes`` and the row type (the dtype of the input buffer: fp32 or bf16) - as CPU tensors, and write into COPIES of the
caller's output buffers, so every word the operation does not own keeps whatever the caller put there (canaries).  They know
samples, channels and segments; they do not know that the kernels work in tiles.

Operand models.  passes = 3 on fp32 rows: float64 on the fp32 operands as given.  passes = 1, and bf16 rows: the float64 product of
the bf16-rounded operands - the weights, the activated input ELU(h), the activated intermediate ELU(y), and on bf16 rows the input
and the output are rounded to bf16 (round to nearest even) where the kernels round them; the skip operand is the raw row (fp32, or
the widened bf16); the last 64 -> 1 convolution is always fp32 arithmetic on the unrounded ELU(h').  The causal padding is the
operation's, not the buffer's: samples before 0 contribute zero to every convolution of the residual blocks and of the last layer -
ELU(h') at samples -2, -1 is zero whatever b1 and b2 are - and the two rows in front of an h segment are never read here.  The
transposed convolution is defined on buffer rows (out[t] = bias + W [x[t] | x[t+1]], row 0 = the caller's zero row), so its row 0 IS
read.

Tolerances (U = 2^-24; the rules of tests/test_gpu_gemm_edges.py and csrc/common.h, computed from the reference alone).
  contraction, three passes, against the exact product:        2^-15 (|a| |W|^T) + U |bias|
  contraction, one pass, against the product of the rounded:   K U (|a| |W|^T) + U |bias|     (an fp32 accumulation of K terms)
  eluf_ on a value v:   2e-7 + 2 U |v| where v <= 1e-6, and on small positive v as far as exp(v) - 1 - v <= 2e-7 (v < 6.4e-4):
                        eluf_ is med3(v, __expf(v) - 1, 0), and csrc/common.h states that the computed exp(v) - 1 can fall below a
                        small positive v by the exponential's round-off (<= ~2e-7), the result then being it instead of v.  Above
                        that eluf_ is the identity; an exact 0 gives an exact 0 (med3(0, 1 - 1, 0)).  (The rule of
                        tests/test_gpu_gemm_edges.py, identity above 1e-6, is too short for a bare ELU(h + b) with zero weights:
                        first run, res128 three passes, all-zero weights: 28 x that tolerance.)
  every fp32 sum of an epilogue (K-half sum, + bias, + skip):  U times the magnitude it rounds
  bf16-row output: 2^-8 |ref|;   last layer: an fma chain, 192 U sum |wf| |ELU(h')| + U |wav|
The error of a stage is carried into the next by |W| of the next contraction (ELU has Lipschitz constant 1; the skip addition
carries it as it is).  Where a one-pass kernel rounds a staged value to bf16, the kernel's value a' lies within its carried error
d of the reference's a: if d is below a quarter of the bf16 spacing at a, a' rounds to bf16(a) or - only where a lies within d of a
rounding boundary - to its neighbour: exactly those elements are charged one bf16 step times |w| (gemm_ref.bf16_flip_charge).
Where d is larger than that (values near 0 behind an ELU or a long contraction) the staged number may be several steps off; it is
the rounding of a number within d of a, so it lies within d + spacing(|a| + d) of bf16(a): those elements are charged that times
|w|.  That is a bound on the value, so their NUMBER needs no cap for soundness (behind the K = 256 one-pass contraction of the
fused level the K U rule alone is a fifth of the spacing at |h| = 0.3, so there they are many); what is capped is what they cost:
no such element is charged more than WIDE_CAP = 9 times the error it carries (derived at WIDE_CAP below), which the CPU suite
asserts element by element on a grid and in sum on every one-pass case, together with the soundness of the charge by sampling.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, Optional

import torch

import gemm_ref as G

U = 2.0 ** -24
BF16 = torch.bfloat16


@dataclass
class SRef:
    out: G.Out                 # the output buffer's copy with the reference written into it, and the owned positions
    tol: torch.Tensor          # [rows, n] tolerance of every owned word (same shape as out.ref)
    stages: Dict[str, torch.Tensor] = field(default_factory=dict)   # intermediates, for the CPU suite
    wide: int = 0              # staged elements whose carried error exceeded a quarter of their bf16 spacing
    staged: int = 0            # staged elements that carried an error at all
    wide_charge: float = 0.0   # what the wide elements were charged, summed, and
    wide_d: float = 0.0        # their carried errors, summed: the cap is wide_charge <= WIDE_CAP * wide_d


class _Count:
    def __init__(self):
        self.wide = 0
        self.staged = 0
        self.wide_charge = 0.0
        self.wide_d = 0.0


# A wide element has d > spacing(a) / 4.  Its charge is max(one step, d + spacing(|a| + d)): one step = spacing(a) < 4 d; for
# d <= |a|, spacing(|a| + d) <= 2 spacing(a) < 8 d; for d > |a|, spacing(|a| + d) <= 2^-7 * 2 d.  So no wide element is charged more
# than 9 times the error it carries - what the three-pass forms charge for carrying it at all.
WIDE_CAP = 9.0


# ------------------------------------------------------------------------------------------------ pieces
def spacing_bf16(x: torch.Tensor) -> torch.Tensor:
    """Distance between neighbouring bf16 numbers at |x| (0 at 0)."""
    r = G.bf16_round(x.abs())
    _, e = torch.frexp(r)
    return torch.where(r > 0, torch.ldexp(torch.ones_like(r), e - 8), torch.zeros_like(r))


def stage_charge(a: torch.Tensor, d: torch.Tensor, cnt: Optional[_Count] = None) -> torch.Tensor:
    """Bound of |bf16(a') - bf16(a)| over |a' - a| <= d (see the module docstring)."""
    one = G.bf16_flip_charge(a, d)
    wide = d > spacing_bf16(a) / 4
    if cnt is not None:
        cnt.wide += int(wide.sum())
        cnt.staged += int((d > 0).sum())
    charge = torch.where(wide, torch.maximum(one, d + spacing_bf16(a.abs() + d)), one)
    if cnt is not None:
        cnt.wide_charge += float(charge[wide].sum())
        cnt.wide_d += float(d[wide].sum())
    return charge


def elu_stage(v: torch.Tensor, dv):
    """(ELU(v), error of the kernel's eluf_ on its own value, which lies within dv of v)."""
    dv = dv if torch.is_tensor(dv) else torch.full_like(v, float(dv))
    exact0 = (v == 0) & (dv == 0)
    lo = v - dv                                            # the smallest value the kernel may hold
    inexact = (lo <= 1e-6) | (torch.expm1(lo.clamp_min(0.0)) - lo <= 2e-7)
    own = torch.where(inexact & ~exact0, 2e-7 + 2 * U * v.abs(), torch.zeros_like(v))
    return G.elu64(v), dv + own


def win3(e: torch.Tensor) -> torch.Tensor:
    """[B, T, C] -> [B, T, 3 C]: tap j of sample t is sample t - 2 + j, zero before sample 0 (the k = 3 causal convolution)."""
    B, T, Cc = e.shape
    p = torch.cat([torch.zeros(B, 2, Cc, dtype=e.dtype), e], dim=1)
    return torch.cat([p[:, 0:T], p[:, 1:T + 1], p[:, 2:T + 2]], dim=2)


def contract(name: str, A: torch.Tensor, dA: Optional[torch.Tensor], W: torch.Tensor, bias: torch.Tensor, one_pass: bool,
             hook: Optional[Callable] = None, cnt: Optional[_Count] = None):
    """A [..., K] the staged operand before its operand rounding, dA its carried error (None: the kernel holds the same number).
    -> (pre-activation, tolerance, magnitude |a| |W|^T + |bias|).  ``hook(name, a, w)`` may replace the operand the PRODUCT is
    formed from (the CPU suite's broken kernels); magnitudes and tolerances always come from the unbroken operand."""
    K = A.shape[-1]
    b = bias.double().reshape(-1)
    if one_pass:
        w, a = G.bf16_round(W.double()), G.bf16_round(A)
        rel = K * U
        extra = stage_charge(A, dA, cnt) @ w.abs().t() if dA is not None else 0.0
    else:
        w, a = W.double(), A
        rel = 2.0 ** -15
        extra = (1.0 + rel) * (dA @ w.abs().t()) if dA is not None else 0.0
    used = hook(name, a, w) if hook is not None else a
    pm = a.abs() @ w.abs().t()
    return used @ w.t() + b, rel * pm + U * b.abs() + extra, pm + b.abs()


def _rows(buf: torch.Tensor, B: int, R: int, Cc: int, seg: int, off: int, first: int):
    """Rows first .. first + R - 1 (of Cc elements) of every segment: (float64 [B, R, Cc], element index [B, R, Cc])."""
    idx = (off + torch.arange(B, dtype=torch.int64)[:, None, None] * seg
           + (first + torch.arange(R, dtype=torch.int64))[None, :, None] * Cc + torch.arange(Cc, dtype=torch.int64)[None, None, :])
    return buf.reshape(-1)[idx].double(), idx


def _emit(name: str, buf: torch.Tensor, idx: torch.Tensor, vals: torch.Tensor) -> G.Out:
    out = buf.detach().cpu().clone()
    kind = "bf16" if out.dtype == BF16 else "f32"
    idx2, v2 = idx.reshape(-1, idx.shape[-1]), vals.reshape(-1, vals.shape[-1])
    out.reshape(-1)[idx2] = v2.float().to(out.dtype)
    return G.Out(name, kind, "raw", out, idx2, v2)


# ------------------------------------------------------------------------------------------------ the four operations
def res128(h, w1, b1, w2, b2, out, *, B, T, h_seg_stride, out_seg_stride, h_off=0, out_off=0, passes=3, hook=None) -> SRef:
    """out = ELU(h + c2(ELU(c1(ELU(h))))) on [B][2 + T][128] segments; rows 0, 1 of an out segment are not written."""
    hb = h.dtype == BF16
    one, cnt = hb or passes == 1, _Count()
    rows, _ = _rows(h, B, T, 128, h_seg_stride, h_off, 2)
    e, de = elu_stage(rows, 0.0)
    ypre, ty, my = contract("res.c1", win3(e), win3(de), w1, b1, one, hook, cnt)
    ty = ty + 2 * U * my                                  # the K-half sum and the bias addition
    y, dy = elu_stage(ypre, ty)
    zpre, tz, mz = contract("res.c2", y, dy, w2, b2, one, hook, cnt)
    opre = rows + zpre
    o, to = elu_stage(opre, tz + 2 * U * (rows.abs() + mz))  # skip + accumulator, + bias
    if hb:
        to = to + 2.0 ** -8 * o.abs()
    _, oidx = _rows(out, B, T, 128, out_seg_stride, out_off, 2)
    return SRef(_emit("out", out, oidx, o), to.reshape(-1, 128), dict(e=e, ypre=ypre, y=y, opre=opre), cnt.wide, cnt.staged, cnt.wide_charge, cnt.wide_d)


def _up_core(x, w, bias, B, T, seg, off, one, hook):
    X, _ = _rows(x, B, T + 1, 128, seg, off, 0)
    A = torch.cat([X[:, :T], X[:, 1:]], dim=2)            # [x[t-1] | x[t]] in samples = buffer rows t, t + 1
    pre, tol, mag = contract("up", A, None, w, bias, one, hook)
    return pre, tol + U * mag                             # accumulator + bias


def up128(x, w, bias, out, *, B, T, x_seg_stride, out_seg_stride, x_off=0, out_off=0, passes=3, hook=None) -> SRef:
    """out[b][t][0..255] = bias + W [x[b][t] | x[b][t+1]] (buffer rows; row 0 of a segment is the caller's zero row)."""
    xb = x.dtype == BF16
    pre, tol = _up_core(x, w, bias, B, T, x_seg_stride, x_off, xb or passes == 1, hook)
    if xb:
        tol = tol + 2.0 ** -8 * pre.abs()
    _, oidx = _rows(out, B, T, 256, out_seg_stride, out_off, 0)
    return SRef(_emit("out", out, oidx, pre), tol.reshape(-1, 256), dict(pre=pre))


def _tail_core(rows, drows, w1, b1, w2, b2, wf, bf, one, hook, cnt):
    """rows [B, S, 64] raw h (drows: its carried error, 0 for caller data) -> (wav [B, S], tolerance, stages)."""
    e, de = elu_stage(rows, drows)
    ypre, ty, my = contract("tail.c1", win3(e), win3(de), w1, b1, one, hook, cnt)
    ty = ty + U * my                                      # + bias
    y, dy = elu_stage(ypre, ty)
    zpre, tz, mz = contract("tail.c2", y, dy, w2, b2, one, hook, cnt)
    hp = rows + zpre
    g, dg = elu_stage(hp, tz + drows + 2 * U * (rows.abs() + mz))
    wfv = wf.double().reshape(192)                        # [3][64]: tap-major like win3
    wav = win3(g) @ wfv + float(bf)
    mw = win3(g.abs()) @ wfv.abs()
    tol = win3(dg) @ wfv.abs() + 192 * U * mw + U * (abs(float(bf)) + wav.abs())
    return wav, tol, dict(e=e, ypre=ypre, y=y, hp=hp, g=g)


def _wav_index(B, S, seg, off):
    return off + torch.arange(B, dtype=torch.int64)[:, None] * seg + torch.arange(S, dtype=torch.int64)[None, :]


def tail(h, w1, b1, w2, b2, wf, bf, wav, *, B, T, h_seg_stride, wav_seg_stride, h_off=0, wav_off=0, passes=3, hook=None) -> SRef:
    """wav = last layer(ELU(h + c2(ELU(c1(ELU(h)))))) on h [B][2 + T][64]; wav [B][T] fp32."""
    one, cnt = h.dtype == BF16 or passes == 1, _Count()
    rows, _ = _rows(h, B, T, 64, h_seg_stride, h_off, 2)
    v, tol, st = _tail_core(rows, torch.zeros_like(rows), w1, b1, w2, b2, wf, bf, one, hook, cnt)
    return SRef(_emit("wav", wav, _wav_index(B, T, wav_seg_stride, wav_off), v), tol, st, cnt.wide, cnt.staged, cnt.wide_charge, cnt.wide_d)


def uptail(x, wu, bu, w1, b1, w2, b2, wf, bf, wav, *, B, T, x_seg_stride, wav_seg_stride, x_off=0, wav_off=0, passes=3, hook=None) -> SRef:
    """The transposed convolution (h stays fp32, never rounded) followed by the tail on its 4 T samples; wav [B][4 T] fp32."""
    one, cnt = x.dtype == BF16 or passes == 1, _Count()
    pre, tup = _up_core(x, wu, bu, B, T, x_seg_stride, x_off, one, hook)
    rows, drows = pre.reshape(B, 4 * T, 64), tup.reshape(B, 4 * T, 64)   # column phase * 64 + channel -> sample 4 t + phase
    v, tol, st = _tail_core(rows, drows, w1, b1, w2, b2, wf, bf, one, hook, cnt)
    st["h"] = rows
    return SRef(_emit("wav", wav, _wav_index(B, 4 * T, wav_seg_stride, wav_off), v), tol, st, cnt.wide, cnt.staged, cnt.wide_charge, cnt.wide_d)


# ------------------------------------------------------------------------------------------------ cases (shared by the CPU and GPU suites)
NAN = float("nan")
SENTINEL = 7.25                     # res128: what the caller left in the two front rows of every out segment
CH = {"res128": 128, "tail": 64, "up128": 128, "uptail": 128}
SUBSTEPS = {"res128": {"c1": 24, "c2": 4}, "tail": {"c1": 12, "c2": 2}, "up128": {"up": 16}, "uptail": {"up": 16, "c1": 12, "c2": 2}}
SPECIALS = ("zero", "tiny", "big", "bias1", "w0")
TINY = (1e-8, -1e-8, 1e-6, -1e-6, -1e-3, -20.0, -100.0)


def _band(w: torch.Tensor, s: int) -> torch.Tensor:
    o = torch.zeros_like(w)
    o[:, 16 * s:16 * s + 16] = w[:, 16 * s:16 * s + 16]
    return o


def _thin_behind(w, op, banded: str, s: int, seed: int) -> None:
    """wav sums every column of the contractions in front of it, and the fused level's first contraction feeds its error budget
    into the block behind it: in the banded families of the tail and the fused level every contraction but the one under test
    (and the dense first convolution in front of a banded second) keeps ONE live term per output - w2: column (row + s) % 32 of
    every row; wf: one tap of one channel; wu in front of a banded block: column (row + 16 s + seed) % 256 - so the fragment under
    test reaches wav unsummed."""
    if "wf" not in w:
        return
    if banded != "c2":
        n = torch.arange(64)
        thin = torch.zeros_like(w["w2"])
        live = w["w2"][n, (n + s) % 32]
        thin[n, (n + s) % 32] = torch.where(live < 0, live - 0.17, live + 0.17)   # (never a term so small that the path through it vanishes)
        w["w2"] = thin
    thin = torch.zeros_like(w["wf"])
    j, c = s % 3, (5 * s + 3 * seed + 1) % 64
    thin[j, c] = 1.0 + w["wf"][j, c]
    w["wf"] = thin
    if "wu" in w and banded != "up":
        n = torch.arange(256)
        thin = torch.zeros_like(w["wu"])
        k = (n + 16 * s + seed) % 256
        thin[n, k] = 10.0 * w["wu"][n, k]
        w["wu"] = thin


def make_case(op: str, B: int, T: int, *, bf16: bool = False, seed: int = 0, band=None, live=None, special=None, slack: int = 3, lead: int = 1):
    """One valid problem with slack in every stride and NaN canaries everywhere the operation owns nothing.
    band = (contraction, substep): that contraction's weights live in one 16-wide K substep only; live = (tile, position): one live
    input row per `tile` rows, all others zero; special: one of SPECIALS.  -> dict(op, B, T, bufs, kw, w)"""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * T + 31 * B + len(op))
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale  # noqa: E731
    Cc, dt = CH[op], (BF16 if bf16 else torch.float32)
    w = {}
    if op == "res128":
        w.update(w1=rn(64, 384, scale=0.05), b1=rn(64, scale=0.1), w2=rn(128, 64, scale=0.12), b2=rn(128, scale=0.1))
    if op in ("up128", "uptail"):
        w.update(wu=rn(256, 256, scale=0.06), bu=rn(64, scale=0.1).repeat(4))
    if op in ("tail", "uptail"):
        w.update(w1=rn(32, 192, scale=0.07), b1=rn(32, scale=0.1), w2=rn(64, 32, scale=0.17), b2=rn(64, scale=0.1), wf=rn(3, 64, scale=0.07))
        w["bf"] = 0.03
    x = rn(B, T, Cc)
    if band is not None:
        key = {"c1": "w1", "c2": "w2", "up": "wu"}[band[0]]
        w[key] = _band(w[key], band[1] % SUBSTEPS[op][band[0]])
        _thin_behind(w, op, band[0], band[1], seed)
    if live is not None:
        keep = (torch.arange(T) % live[0]) == (live[1] % live[0])
        x = x * keep[None, :, None]
        _thin_behind(w, op, "c1", live[1], seed)
    if special == "zero":
        x[:, ::3] = 0.0
        x[:, :, 5::7] = 0.0
    elif special == "tiny":
        x = torch.tensor(TINY)[torch.randint(0, len(TINY), (B, T, Cc), generator=g)]
    elif special == "big":
        x = 1e3 * (1.0 + 0.1 * x)
    elif special == "bias1":
        for k in ("b1", "b2"):
            if k in w:
                w[k] = rn(*w[k].shape)
    elif special == "w0":
        for k in ("w1", "w2", "wu"):
            if k in w:
                w[k] = torch.zeros_like(w[k])
    # ---- buffers: [guard | B segments | guard]; rows the operation owns hold data, its zero rows 0, everything else NaN
    front = 2 if op in ("res128", "tail") else 1
    rows_in = front + T + slack
    seg_in, off_in = rows_in * Cc, lead * Cc
    xin = torch.full((off_in + B * seg_in + Cc,), NAN)
    body = torch.full((B, rows_in, Cc), NAN)
    body[:, :front] = 0.0
    body[:, front:front + T] = x
    xin[off_in:off_in + B * seg_in] = body.reshape(-1)
    bufs, kw = {"in": xin.to(dt)}, {}
    if op == "res128":
        ob = torch.full((B, rows_in, Cc), NAN)
        ob[:, :2] = SENTINEL
        o = torch.full((off_in + B * seg_in + Cc,), NAN)
        o[off_in:off_in + B * seg_in] = ob.reshape(-1)
        bufs["out"] = o.to(dt)
        kw = dict(h_seg_stride=seg_in, out_seg_stride=seg_in, h_off=off_in, out_off=off_in)
    elif op == "up128":
        seg_o = T * 256 + 8 * slack
        bufs["out"] = torch.full((256 + B * seg_o + 256,), NAN).to(dt)
        kw = dict(x_seg_stride=seg_in, out_seg_stride=seg_o, x_off=off_in, out_off=256)
    else:
        S = T if op == "tail" else 4 * T
        seg_o = S + 3 * slack
        bufs["out"] = torch.full((3 + B * seg_o + 9,), NAN)
        kw = dict(wav_seg_stride=seg_o, wav_off=3)
        kw.update(dict(h_seg_stride=seg_in, h_off=off_in) if op == "tail" else dict(x_seg_stride=seg_in, x_off=off_in))
    return dict(op=op, B=B, T=T, bf16=bf16, bufs=bufs, kw=kw, w=w, x=x)


def run_ref(case, passes: int = 3, hook=None) -> SRef:
    op, w, b, kw = case["op"], case["w"], case["bufs"], dict(case["kw"], B=case["B"], T=case["T"], passes=passes, hook=hook)
    if op == "res128":
        return res128(b["in"], w["w1"], w["b1"], w["w2"], w["b2"], b["out"], **kw)
    if op == "up128":
        return up128(b["in"], w["wu"], w["bu"], b["out"], **kw)
    if op == "tail":
        return tail(b["in"], w["w1"], w["b1"], w["w2"], w["b2"], w["wf"], w["bf"], b["out"], **kw)
    return uptail(b["in"], w["wu"], w["bu"], w["w1"], w["b1"], w["w2"], w["b2"], w["wf"], w["bf"], b["out"], **kw)


def compare(ref: SRef, got: torch.Tensor):
    """-> (worst error / tolerance over the owned words, number of other words that changed).  NaN-safe: a NaN in an owned word is inf."""
    o = ref.out
    err = (o.values(got) - o.ref).abs()
    ratio = torch.where(torch.isfinite(err), err / ref.tol.reshape(err.shape).clamp_min(1e-300), torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    other = ~o.owned()
    changed = int((o.bits(got)[other] != o.bits(o.buf)[other]).sum())
    return float(ratio.max()), changed
