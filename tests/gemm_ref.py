"""float64 reference of the tiled-contraction ABI (sopro_gemm_args + sopro_gemm_split_ext, include/sopro_hip.h).

``gemm_ref`` takes what ``sopro_amd.hip.gemm`` takes - flat buffers, leading dimensions, segment strides, element offsets,
rows_per_seg, prologue / epilogue, scale, pro_vec, the packed GLU pairing, the rotary tables, LayerNorm statistics, the
fused-RMSNorm eps, c_mode 0-8 and the three A formats - as CPU tensors, and writes into COPIES of the caller's output
buffers, so every word the operation does not own keeps whatever the caller put there (canaries).  It knows rows,
columns and segments; it does not know that the kernels work in tiles.

Formats: "split form" = every aligned group of 32 channels (128 bytes as fp32) holds [32 hi bf16 | 32 lo bf16]; bf16 rows are
torch.bfloat16 buffers whose offsets / strides count elements.  All rounding to bf16 is round-to-nearest-even (torch's cast).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional

import torch

PRO_NONE, PRO_ELU, PRO_ADDVEC = 0, 1, 2
EPI_NONE, EPI_GELU, EPI_GLU, EPI_RES, EPI_TANH, EPI_ROPE = 0, 1, 2, 3, 4, 6

_INT_VIEW = {"f32": torch.int32, "pairs": torch.int32, "stats": torch.int32, "bf16": torch.int16, "split": torch.int16}


# ------------------------------------------------------------------------------------------------ number formats
def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """Round to the nearest bf16 (ties to even), returned as float64."""
    return x.float().to(torch.bfloat16).double()


def split_pieces(x: torch.Tensor):
    """fp32 values -> (hi, lo) bf16 tensors with hi = bf16(x), lo = bf16(x - hi)."""
    x = x.float()
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi, lo


def to_split_form(x: torch.Tensor) -> torch.Tensor:
    """fp32 rows [..., C] (C % 32 == 0) -> the fp32-typed tensor of the same shape whose bytes are the split form."""
    sh = x.shape
    hi, lo = split_pieces(x.reshape(-1, sh[-1] // 32, 32))
    return torch.cat([hi, lo], dim=-1).contiguous().view(torch.float32).reshape(sh)


def from_split_form(words: torch.Tensor) -> torch.Tensor:
    """The inverse: fp32-typed split-form rows [..., C] -> float64 values hi + lo."""
    sh = words.shape
    h = words.contiguous().view(torch.bfloat16).reshape(-1, sh[-1] // 32, 2, 32).double()
    return (h[:, :, 0] + h[:, :, 1]).reshape(sh)


# ------------------------------------------------------------------------------------------------ addressing
def row_starts(M: int, rows_per_seg: int, ld: int, seg_stride: int, off: int) -> torch.Tensor:
    """Element index of the first column of every row: off + (m / rps) * seg_stride + (m % rps) * ld (seg stride 0 = dense)."""
    m = torch.arange(M, dtype=torch.int64)
    seg = m // rows_per_seg
    ss = seg_stride if seg_stride else rows_per_seg * ld
    return off + seg * ss + (m - seg * rows_per_seg) * ld


def _cols(starts: torch.Tensor, n: int) -> torch.Tensor:
    return starts[:, None] + torch.arange(n, dtype=torch.int64)[None, :]


def _split_index(starts: torch.Tensor, n: int):
    """16-bit positions of the hi / lo halves of columns 0..n-1 of split-form rows (starts in fp32 words)."""
    c = torch.arange(n, dtype=torch.int64)[None, :]
    hi = starts[:, None] * 2 + (c >> 5) * 64 + (c & 31)
    return hi, hi + 32


def gather_rows(buf: torch.Tensor, starts: torch.Tensor, n: int, kind: str = "f32") -> torch.Tensor:
    """Rows of a flat buffer as float64 [M, n]; kind: f32 | bf16 | split."""
    flat = buf.reshape(-1)
    if kind == "split":
        h = flat.view(torch.bfloat16)
        hi, lo = _split_index(starts, n)
        return h[hi].double() + h[lo].double()
    return flat[_cols(starts, n)].double()


@dataclass
class Out:
    """One output stream of a call: ``buf`` is the copy of the caller's buffer with the reference written into it, ``idx`` (and
    ``idx_lo`` for the split form) the positions the operation owns in units of ``view`` elements, ``ref`` the float64 values
    [M, n] that were encoded there (before the rounding of the format)."""
    name: str   # "C" | "C2" | "ln_stats_out"
    kind: str   # f32 | bf16 | split | pairs | stats
    role: str   # raw | act | argmax | stats
    buf: torch.Tensor
    idx: torch.Tensor
    ref: torch.Tensor
    idx_lo: Optional[torch.Tensor] = None

    @property
    def view(self):
        return _INT_VIEW[self.kind]

    def bits(self, buf: torch.Tensor) -> torch.Tensor:
        return buf.detach().cpu().reshape(-1).view(self.view)

    def owned(self) -> torch.Tensor:
        m = torch.zeros(self.bits(self.buf).numel(), dtype=torch.bool)
        m[self.idx.reshape(-1)] = True
        if self.idx_lo is not None:
            m[self.idx_lo.reshape(-1)] = True
        return m

    def values(self, buf: torch.Tensor) -> torch.Tensor:
        """What a buffer (the reference's or the kernel's) holds at the owned positions, as float64 [M, n]."""
        flat = buf.detach().cpu().reshape(-1)
        if self.kind == "split":
            h = flat.view(torch.bfloat16)
            return h[self.idx].double() + h[self.idx_lo].double()
        if self.kind == "bf16":
            return flat[self.idx].double()
        return flat.view(torch.float32)[self.idx].double()


@dataclass
class Ref:
    pre: torch.Tensor    # [M, N] float64 pre-activation: pro(A) W^T + bias (row-scaled for the fused RMSNorm)
    mag: torch.Tensor    # [M, N] |pro(A)| |W|^T + |bias|: what the operand-precision bound multiplies
    out: torch.Tensor    # [M, n_out] float64 value of the epilogue
    a_eff: torch.Tensor  # [M, K] the staged operand pro(A) (after the operand rounding of the one-pass form)
    w_eff: torch.Tensor  # [N, K]
    outs: List[Out] = field(default_factory=list)
    res: Optional[torch.Tensor] = None       # EPI_RES: the skip operand's values [M, N]
    scale: Optional[torch.Tensor] = None     # EPI_RES: the per-column scale [N] (ones when absent)
    rope_cs: Optional[tuple] = None          # EPI_ROPE: (cos, sin, partner pre-activation index) for the bound
    a_pre: Optional[torch.Tensor] = None     # [M, K] pro(A) in float64 before the operand rounding of the one-pass form
    ln_terms: Optional[torch.Tensor] = None  # fused LayerNorm: |a rstd| + |mean rstd| per element [M, K]

    def __getitem__(self, name: str) -> Out:
        return [o for o in self.outs if o.name == name][0]


def bf16_flip_charge(x: torch.Tensor, eps: torch.Tensor) -> torch.Tensor:
    """[M, K]: one bf16 ulp of x where x lies within ``eps`` of a bf16 rounding boundary (a value that is off x by at most eps may
    round to the other neighbour: its rounded image then differs by at most that ulp beyond eps), 0 elsewhere."""
    r = bf16_round(x)
    _, e = torch.frexp(r)
    ulp = torch.ldexp(torch.ones_like(r), e - 8)
    toward_zero = (x.abs() < r.abs()) & (torch.frexp(r)[0].abs() == 0.5)  # below a power of two the spacing halves
    half = torch.where(toward_zero, ulp / 4, ulp / 2)
    # (what gets rounded is an fp32 number: where there is an error at all, half an fp32 ulp more - it can land ON the boundary)
    eps = torch.where(eps > 0, eps + 2.0 ** -24 * x.abs(), eps)
    return torch.where(half - (x - r).abs() <= eps, ulp, torch.zeros_like(ulp))


# ------------------------------------------------------------------------------------------------ elementary functions
def elu64(x):
    return torch.where(x > 0, x, torch.expm1(torch.clamp(x, max=0.0)))


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _write(kind: str, name: str, role: str, buf: torch.Tensor, starts: torch.Tensor, vals: torch.Tensor) -> Out:
    """Encode float64 values [M, n] into a copy of ``buf`` at rows ``starts``."""
    out = buf.detach().cpu().clone()
    flat = out.reshape(-1)
    n = vals.shape[1]
    if kind == "split":
        hi, lo = split_pieces(vals.float())
        ih, il = _split_index(starts, n)
        h = flat.view(torch.bfloat16)
        h[ih] = hi
        h[il] = lo
        return Out(name, kind, role, out, ih, vals, il)
    idx = _cols(starts, n)
    flat[idx] = vals.float().to(flat.dtype) if kind == "bf16" else vals.float()
    return Out(name, kind, role, out, idx, vals)


def ln_from_pairs(pairs: torch.Tensor, K: int):
    """(mean, sum of squared deviations) per 64 columns [M, K / 64, 2] -> (mean, variance) per row, Chan's combination."""
    p = pairs.double()
    mean = p[..., 0].mean(dim=1)
    m2 = (p[..., 1] + 64.0 * (p[..., 0] - mean[:, None]) ** 2).sum(dim=1)
    return mean, m2 / K


def row_stats64(x: torch.Tensor) -> torch.Tensor:
    """[M, C] -> [M, C / 64, 2] (mean, sum of squared deviations from it) per 64-column group."""
    g = x.double().reshape(x.shape[0], -1, 64)
    mu = g.mean(dim=2)
    return torch.stack([mu, ((g - mu[..., None]) ** 2).sum(dim=2)], dim=2)


# ------------------------------------------------------------------------------------------------ the reference
def gemm_ref(A: torch.Tensor, W: torch.Tensor, Cout: Optional[torch.Tensor], *, M: int, N: int, K: int, lda: Optional[int] = None,
             ldc: Optional[int] = None, bias: Optional[torch.Tensor] = None, epilogue: int = EPI_NONE, prologue: int = PRO_NONE,
             R: Optional[torch.Tensor] = None, ldr: Optional[int] = None, scale: Optional[torch.Tensor] = None,
             pro_vec: Optional[torch.Tensor] = None, rows_per_seg: Optional[int] = None, a_seg_stride: int = 0, c_seg_stride: int = 0,
             r_seg_stride: int = 0, a_off: int = 0, c_off: int = 0, r_off: int = 0, a_split: bool = False, c_mode: int = 0,
             C2: Optional[torch.Tensor] = None, ldc2: Optional[int] = None, c2_seg_stride: int = 0, c2_off: int = 0, rms_eps: float = 0.0,
             rope: Optional[tuple] = None, ln_stats: Optional[torch.Tensor] = None, ln_eps: float = 0.0,
             ln_stats_out: Optional[torch.Tensor] = None, round_operands: bool = False) -> Ref:
    """``W`` is the logical [N, K] fp32 matrix (for EPI_GLU in the packed [32 value | 32 gate] row order the kernels read).
    ``round_operands``: the one-pass form - both operands rounded to bf16 before the float64 product."""
    n_out = N // 2 if epilogue == EPI_GLU else N
    rps = M if rows_per_seg is None else rows_per_seg
    lda = K if lda is None else lda
    ldc = n_out if ldc is None else ldc
    ldr = n_out if ldr is None else ldr
    a16 = A.dtype == torch.bfloat16
    c16 = c_mode in (6, 7, 8)
    # ---- the staged operand
    a_st = row_starts(M, rps, lda, a_seg_stride, a_off)
    a = gather_rows(A, a_st, K, "split" if a_split else "f32")
    w = W.double()[:N, :K]
    if round_operands:
        w = bf16_round(w)
    rs = None
    if prologue == PRO_ELU:
        a = elu64(a)
    elif prologue == PRO_ADDVEC:
        a = a + pro_vec.double().reshape(-1)[:K][None, :]
    if ln_stats is not None:
        mean, var = ln_from_pairs(ln_stats.reshape(-1)[: M * (K // 64) * 2].reshape(M, K // 64, 2), K)
        rstd = 1.0 / torch.sqrt(var[:, None] + ln_eps)
        ln_terms = (a.abs() + mean.abs()[:, None]) * rstd  # |a rstd| + |mean rstd|: what an fp32 evaluation of the next line rounds
        a = (a - mean[:, None]) * rstd
    else:
        ln_terms = None
    if rms_eps > 0.0:
        rs = 1.0 / torch.sqrt((a * a).mean(dim=1) + rms_eps)  # of the raw row; the staged operand is the raw row
    a_pre = a
    if round_operands and not a16:
        a = bf16_round(a)
    b = bias.double().reshape(-1)[:N] if bias is not None else torch.zeros(N, dtype=torch.float64)
    prod, pmag = a @ w.t(), a.abs() @ w.abs().t()
    if rs is not None:
        prod, pmag = prod * rs[:, None], pmag * rs[:, None]
    pre, mag = prod + b, pmag + b.abs()
    ref = Ref(pre=pre, mag=mag, out=pre, a_eff=a, w_eff=w, a_pre=a_pre, ln_terms=ln_terms)
    # ---- epilogue
    if epilogue == EPI_GELU:
        out = gelu64(pre)
    elif epilogue == EPI_TANH:
        out = torch.tanh(pre)
    elif epilogue == EPI_GLU:
        g = pre.reshape(M, N // 64, 2, 32)
        out = (g[:, :, 0] * torch.sigmoid(g[:, :, 1])).reshape(M, n_out)
    elif epilogue == EPI_RES:
        r_st = row_starts(M, rps, ldr, r_seg_stride, r_off)
        ref.res = gather_rows(R, r_st, N, "f32")
        ref.scale = scale.double().reshape(-1)[:N] if scale is not None else torch.ones(N, dtype=torch.float64)
        out = ref.res + ref.scale[None, :] * pre
    elif epilogue == EPI_ROPE:
        cos_t, sin_t, rcols, dh, pos0, rrps = rope
        half = dh // 2
        pos = pos0 + torch.arange(M, dtype=torch.int64) % rrps
        col = torch.arange(rcols, dtype=torch.int64)
        e = col % dh
        low = e < half
        partner = torch.where(low, col + half, col - half)
        c = cos_t.double().reshape(-1, half)[pos][:, e % half]
        s = sin_t.double().reshape(-1, half)[pos][:, e % half]
        sgn = torch.where(low, -1.0, 1.0).double()[None, :]
        out = pre.clone()
        out[:, :rcols] = pre[:, :rcols] * c + sgn * pre[:, partner] * s
        ref.rope_cs = (c, s, partner)
    else:
        out = pre
    ref.out = out
    act = elu64(out)
    # ---- output streams
    c_st = row_starts(M, rps, ldc, c_seg_stride, c_off)
    ldc2_given = ldc2
    ldc2 = n_out if ldc2 is None else ldc2
    c2_st = row_starts(M, rps, ldc2, c2_seg_stride, c2_off) if C2 is not None and c_mode != 5 else None
    if c_mode == 0:
        ref.outs.append(_write("f32", "C", "raw", Cout, c_st, out))
    elif c_mode == 1:
        ref.outs.append(_write("split", "C", "act", Cout, c_st, act))
    elif c_mode == 2:
        ref.outs.append(_write("f32", "C", "raw", Cout, c_st, out))
        ref.outs.append(_write("split", "C2", "act", C2, c2_st, act))
    elif c_mode == 3:
        ref.outs.append(_write("f32", "C", "act", Cout, c_st, act))
    elif c_mode == 4:
        ref.outs.append(_write("f32", "C", "raw", Cout, c_st, out))
        ref.outs.append(_write("f32", "C2", "act", C2, c2_st, act))
    elif c_mode == 5:  # (max, column) per row and 64-column group, first maximum; rows are m * ldc2 pairs apart, no segments
        G = -(-N // 64)
        ldp = G if ldc2_given is None else ldc2_given
        pad = torch.full((M, G * 64), -float("inf"), dtype=torch.float64)
        pad[:, :N] = out
        grp = pad.reshape(M, G, 64)
        best, arg = grp.max(dim=2)
        arg = torch.argmax((grp == best[..., None]).to(torch.int8), dim=2) + 64 * torch.arange(G)[None, :]
        buf = C2.detach().cpu().clone()
        flat = buf.reshape(-1)
        base = c2_off + (torch.arange(M, dtype=torch.int64)[:, None] * ldp + torch.arange(G, dtype=torch.int64)[None, :]) * 2
        flat[base] = best.float()
        flat.view(torch.int32)[base + 1] = arg.to(torch.int32)
        ref.outs.append(Out("C2", "pairs", "argmax", buf, torch.stack([base, base + 1], dim=2).reshape(M, 2 * G),
                            torch.stack([best, arg.double()], dim=2).reshape(M, 2 * G)))
    elif c_mode == 6:
        ref.outs.append(_write("bf16", "C", "raw", Cout, c_st, out))
    elif c_mode == 7:
        ref.outs.append(_write("bf16", "C", "act", Cout, c_st, act))
    elif c_mode == 8:
        ref.outs.append(_write("bf16", "C", "raw", Cout, c_st, out))
        ref.outs.append(_write("bf16", "C2", "act", C2, c2_st, act))
    else:
        raise ValueError(f"c_mode {c_mode}")
    if c16 and epilogue == EPI_RES and R.dtype != torch.bfloat16:
        raise ValueError("bf16 rows take a bf16 skip operand")
    if ln_stats_out is not None:  # statistics of the stream as it was written (fp32 values)
        st = row_stats64(out.float())
        buf = ln_stats_out.detach().cpu().clone()
        idx = torch.arange(M * (N // 64) * 2, dtype=torch.int64).reshape(M, (N // 64) * 2)
        buf.reshape(-1)[idx] = st.reshape(M, -1).float()
        ref.outs.append(Out("ln_stats_out", "stats", "stats", buf, idx, st.reshape(M, -1)))
    return ref
