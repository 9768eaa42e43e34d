"""float64 reference of the AR-step contraction ABI (sopro_skinny_args, include/sopro_hip.h) and of its two weight packers.

``skinny_ref`` takes what ``sopro_skinny_f32`` takes - flat buffers, ldx / ldw / ldy / ldr, xp_stride, y_part_stride, the aux operand
set with its strides and flags, ring, dw_w, dw_b, step, ring_len, ring_bcap, dil, ksize, ring_format - as CPU tensors, and writes
into COPIES of the caller's Y, aux_Y and ring, so every word the call does not own keeps whatever the caller put there (canaries):
the `Out` idea of tests/gemm_ref.py.  It knows rows, columns, K-slices and ring slots; it does not know tiles, waves, mt or nt, and
the weights are always the logical row-major [N, ldw] matrix (``pack_skinny_ref`` is the separate reference of the fragment order).

The one thing it does in fp32 is the header's "fixed order": Xin = ((X + Xp0) + Xp1) + Xp2, so that the staged value is reproduced
bit for bit - for the norm statistic and for the bf16 operand rounding of w_layout 2 alike.  Everything after that is float64.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

import gemm_ref as G
from gemm_ref import bf16_flip_charge, bf16_round, gelu64  # noqa: F401  (re-exported for the tests)

EPI_NONE, EPI_GELU, EPI_GLU, EPI_RES, EPI_TANH, EPI_GLU_DW = 0, 1, 2, 3, 4, 5
KS = 384        # K slice
MAXTAPS = 13


@dataclass
class Stream(G.Out):
    """One value stream of a call (``G.Out``: copy of the buffer, owned positions, float64 values) with what its bound needs."""
    target: str = "Y"                       # the caller's buffer it lives in: Y | aux_Y | ring
    pre: Optional[torch.Tensor] = None      # float64 pre-activation rs * sum + bias of this stream (this slice alone for a K-slice)
    pmag: Optional[torch.Tensor] = None     # rs * |Xin| |W|^T over the K range of this stream
    bmag: Optional[torch.Tensor] = None     # |bias| where this stream carries the bias, else 0  [N]
    epi: int = EPI_NONE                     # the effective epilogue of this stream (NONE for the raw K-slices)
    normed: bool = False
    res: Optional[torch.Tensor] = None
    scale: Optional[torch.Tensor] = None
    nslices: int = 1                        # K-slices accumulated into this stream by one workgroup


@dataclass
class SkinnyRef:
    xin: torch.Tensor                        # [B, K] fp32: the staged rows, bit for bit
    rs: Optional[torch.Tensor]               # [B] float64 row scale (None without rms_norm)
    outs: List[Stream] = field(default_factory=list)
    bufs: Dict[str, torch.Tensor] = field(default_factory=dict)   # target -> the copy with every stream written
    glu: Optional[dict] = None               # GLU tail: v, g, h, taps [B, D, 13], tapw [D, 13], dw_b, y, slot

    def __getitem__(self, name: str) -> Stream:
        return [o for o in self.outs if o.name == name][0]

    def owned(self, target: str) -> torch.Tensor:
        m = None
        for o in self.outs:
            if o.target == target:
                m = o.owned() if m is None else (m | o.owned())
        return m


def stage(X, Xp, *, B, K, ldx, np_=0, xp_stride=0) -> torch.Tensor:
    """Xin [B, K] in fp32: ((X + Xp0) + Xp1) + Xp2, every sum rounded to fp32 in that order."""
    idx = torch.arange(B, dtype=torch.int64)[:, None] * ldx + torch.arange(K, dtype=torch.int64)[None, :]
    x = X.reshape(-1).float()[idx]
    for s in range(np_):
        x = x + Xp.reshape(-1).float()[s * xp_stride + idx]
    return x


def skinny_mag(A: torch.Tensor, Wm: torch.Tensor, bias: Optional[torch.Tensor] = None):
    """|A| |W|^T + |bias| [B, N] and its per-slice parts (the bias is in the total only): what the operand-precision bound multiplies."""
    a, w = A.double().abs(), Wm.double().abs()
    parts = [a[:, k0:k0 + KS] @ w[:, k0:k0 + KS].t() for k0 in range(0, a.shape[1], KS)]
    total = sum(parts)
    if bias is not None:
        total = total + bias.double().abs()[None, :]
    return total, parts


def _put(bufs, target, kind, name, pos, vals, **kw) -> Stream:
    flat = bufs[target].reshape(-1)
    flat[pos] = vals.float().to(flat.dtype) if kind == "bf16" else vals.float()
    return Stream(name, kind, "raw", bufs[target], pos, vals, target=target, **kw)


def _logical(Wbuf, ldw, N, K):
    idx = torch.arange(N, dtype=torch.int64)[:, None] * ldw + torch.arange(K, dtype=torch.int64)[None, :]
    return Wbuf.reshape(-1).float()[idx]


def _plain(ref, target, prefix, A, rs, Wm, bias, R, scale, *, B, N, K, ld, ldr, yps, epi, split):
    """One operand set of the plain form: the unsplit stream, or one stream per K-slice."""
    rows = torch.arange(B, dtype=torch.int64)[:, None]
    cols = torch.arange(N, dtype=torch.int64)[None, :]
    b = bias.double().reshape(-1)[:N] if bias is not None else torch.zeros(N, dtype=torch.float64)
    r = R.reshape(-1).double()[rows * ldr + cols] if epi == EPI_RES else None   # read before anything is written (R may be Y)
    sc = scale.double().reshape(-1)[:N] if scale is not None else torch.ones(N, dtype=torch.float64)
    rsc = rs[:, None] if rs is not None else 1.0
    parts = [A[:, k0:k0 + KS] @ Wm[:, k0:k0 + KS].t() for k0 in range(0, K, KS)]
    mags = [A[:, k0:k0 + KS].abs() @ Wm[:, k0:k0 + KS].abs().t() for k0 in range(0, K, KS)]
    if not split:
        pre = rsc * sum(parts) + b
        out = {EPI_GELU: G.gelu64, EPI_TANH: torch.tanh}.get(epi, lambda v: v)(pre)
        if epi == EPI_RES:
            out = r + sc[None, :] * pre
        ref.outs.append(_put(ref.bufs, target, "f32", prefix, rows * ld + cols, out, pre=pre, pmag=rsc * sum(mags), bmag=b.abs(), epi=epi,
                             normed=rs is not None, res=r, scale=sc if epi == EPI_RES else None, nslices=K // KS))
        return
    # K-split: slice s at s * yps; slice 0 carries bias + residual under EPI_RES, every other word is the raw partial sum
    # (EPI_NONE with a bias and any scale are refused by the entry point: no slice would carry them as the header's formula says)
    for s, (p, m) in enumerate(zip(parts, mags)):
        first = s == 0 and epi == EPI_RES
        pre = p + b if first else p
        out = r + pre if first else pre
        ref.outs.append(_put(ref.bufs, target, "f32", f"{prefix}{s}", s * yps + rows * ld + cols, out, pre=pre, pmag=m,
                             bmag=b.abs() if first else torch.zeros_like(b), epi=EPI_RES if first else EPI_NONE, res=r if first else None,
                             scale=torch.ones_like(b) if first else None))


def skinny_ref(X, W, Y, *, B, N, K, ldx=None, ldw=None, ldy=None, bias=None, epilogue=EPI_NONE, R=None, ldr=None, scale=None,
               Xp=None, np_=0, xp_stride=0, ksplit=0, y_part_stride=0, rms_norm=False, eps=1e-6, w_layout=0,
               aux_W=None, aux_tiles=0, aux_bias=None, aux_R=None, aux_Y=None, aux_ldy=None, aux_ldr=None, aux_y_part_stride=0,
               aux_flags=0, ring=None, dw_w=None, dw_b=None, step=0, ring_len=0, ring_bcap=0, dil=1, ksize=1, ring_format=0) -> SkinnyRef:
    """``W`` / ``aux_W``: the logical fp32 matrices as flat row-major buffers ([N, ldw]; aux: [16 * aux_tiles, K] dense), whatever
    w_layout says about the image the kernel reads; w_layout 2 rounds both operands to bf16.  ``step``: the frame index (an int)."""
    glu = epilogue == EPI_GLU_DW
    n_out = N // 2 if glu else N
    ldx = K if ldx is None else ldx
    ldw = K if ldw is None else ldw
    ldy = n_out if ldy is None else ldy
    ldr = n_out if ldr is None else ldr
    xin = stage(X, Xp, B=B, K=K, ldx=ldx, np_=np_, xp_stride=xp_stride)
    x64 = xin.double()
    rs = 1.0 / torch.sqrt((x64 * x64).mean(dim=1) + float(np.float32(eps))) if rms_norm else None
    A = bf16_round(xin) if w_layout == 2 else x64
    rnd = bf16_round if w_layout == 2 else (lambda t: t.double())
    Wm = rnd(_logical(W, ldw, N, K))
    ref = SkinnyRef(xin=xin, rs=rs)
    ref.bufs["Y"] = Y.detach().cpu().clone()
    split = bool(ksplit) and K > KS
    if not glu:
        if aux_tiles:  # copied before the main set is written: aux_R may be any buffer
            ref.bufs["aux_Y"] = aux_Y.detach().cpu().clone()
        _plain(ref, "Y", "Y", A, rs, Wm, bias, R, scale, B=B, N=N, K=K, ld=ldy, ldr=ldr, yps=y_part_stride, epi=epilogue, split=split)
        if aux_tiles:
            Na = 16 * aux_tiles
            _plain(ref, "aux_Y", "aux", A, None if (aux_flags & 1) else rs, rnd(_logical(aux_W, K, Na, K)), aux_bias, aux_R, None,
                   B=B, N=Na, K=K, ld=Na if aux_ldy is None else aux_ldy, ldr=Na if aux_ldr is None else aux_ldr,
                   yps=aux_y_part_stride, epi=EPI_NONE if (aux_flags & 2) else epilogue, split=split)
        return ref
    # ---- GLU tail: h = v * sigmoid(g); y = taps over the ring as it was + the newest tap (unrounded h); Y = Xin + y; ring[t % L] = h
    D, L = N // 2, ring_len
    b = bias.double().reshape(-1)[:N] if bias is not None else torch.zeros(N, dtype=torch.float64)
    pre = rs[:, None] * (A @ Wm.t()) + b
    pmag = rs[:, None] * (A.abs() @ Wm.abs().t())
    v, g = pre[:, :D], pre[:, D:]
    h = v * torch.sigmoid(g)
    ring0 = ring.detach().cpu().clone()
    ref.bufs["ring"] = ring0.clone()
    rflat = ring0.reshape(-1).double()
    rows = torch.arange(B, dtype=torch.int64)[:, None]
    cols = torch.arange(D, dtype=torch.int64)[None, :]
    wt = dw_w.double().reshape(-1)[: ksize * D].reshape(ksize, D)
    taps = torch.zeros(B, D, MAXTAPS, dtype=torch.float64)
    tapw = torch.zeros(D, MAXTAPS, dtype=torch.float64)
    for j in range(ksize - 1):  # tap j is frame t - (ksize - 1 - j) * dil, slot (t + 1 + j * dil) mod L
        slot = (step + 1 + j * dil) % L
        taps[:, :, j] = rflat[(slot * ring_bcap + rows) * D + cols]
        tapw[:, j] = wt[j]
    taps[:, :, MAXTAPS - 1], tapw[:, MAXTAPS - 1] = h, wt[ksize - 1]
    dwb = dw_b.double().reshape(-1)[:D]
    y = (taps * tapw[None]).sum(dim=2) + dwb
    out = x64[:, :D] + y
    slot = step % L
    kw = dict(pre=pre, pmag=pmag, bmag=b.abs(), epi=EPI_GLU_DW, normed=True)
    ref.outs.append(_put(ref.bufs, "Y", "f32", "Y", rows * ldy + cols, out, **kw))
    ref.outs.append(_put(ref.bufs, "ring", "bf16" if ring_format == 1 else "f32", "ring", (slot * ring_bcap + rows) * D + cols, h, **kw))
    ref.glu = dict(v=v, g=g, h=h, taps=taps, tapw=tapw, dw_b=dwb, y=y, slot=slot)
    return ref


# ------------------------------------------------------------------------------------------------ the packers
def skinny_packed_floats(N: int, K: int, glu: bool) -> int:
    tiles = (N // 2 + 7) // 8 if glu else (N + 15) // 16
    return tiles * (K // 32) * 512


def pack_skinny_ref(W: torch.Tensor, ldw: int, N: int, K: int, glu: bool, bf16: bool) -> torch.Tensor:
    """The exact packed image by the header's fragment-order formula: fp32 [tile][K/32][2][64 lanes][4], or bf16
    [tile][K/32][64 lanes][8] (torch's round-to-nearest-even cast).  Lane (i = lane & 15, g = lane >> 4) of tile t holds
    k = 32 * chunk + 8 * g + 4 * half .. + 3 of row t * 16 + i, or for glu of the value row t * 8 + (i & 7) (i < 8) / the gate row
    N / 2 + t * 8 + (i & 7).  Rows past N are zero."""
    D = N // 2
    tiles = (D + 7) // 8 if glu else (N + 15) // 16
    lane = torch.arange(64, dtype=torch.int64)
    i, g = lane & 15, lane >> 4
    t = torch.arange(tiles, dtype=torch.int64)[:, None]
    if glu:
        n = t * 8 + (i & 7)[None, :]
        ok = n < D
        row = torch.where(i[None, :] < 8, n, D + n)
    else:
        row = t * 16 + i[None, :]
        ok = row < N
    row = torch.where(ok, row, torch.zeros_like(row))
    chunk = torch.arange(K // 32, dtype=torch.int64)
    flat = W.reshape(-1).float()
    if bf16:
        k = chunk[:, None, None] * 32 + g[None, :, None] * 8 + torch.arange(8)[None, None, :]                    # [chunk, lane, 8]
        v = flat[row[:, None, :, None] * ldw + k[None]]                                                          # [tile, chunk, lane, 8]
        return torch.where(ok[:, None, :, None], v, torch.zeros_like(v)).to(torch.bfloat16).reshape(-1)
    k = chunk[:, None, None, None] * 32 + g[None, None, :, None] * 8 + torch.arange(2)[None, :, None, None] * 4 + torch.arange(4)[None, None, None, :]
    v = flat[row[:, None, None, :, None] * ldw + k[None]]                                                        # [tile, chunk, 2, lane, 4]
    return torch.where(ok[:, None, None, :, None], v, torch.zeros_like(v)).reshape(-1)
