"""Attention kernels (MI355X) against the plain formula in float64: masked scores, softmax, weighted sum; a row that sees no key is
zeros.  Five kernels: the fp32 VALU kernel and the single-query decode kernel (csrc/attention.hip), the exact fp32 MFMA kernel and
the split-bf16 MFMA kernel (csrc/attention_mfma.hip), and the one-launch xattn_step block.  tests/test_gpu_ops.py feeds them randn
Q and K (scores ~ N(0,1)), where the online-softmax rescale factor stays near 1; here the keys carry a gain profile so that the
running maximum moves by more than 2^8 from one key tile to the next, kv_index / k_bstride == 0 are run at op level, rows without a
visible key are checked to be exactly zero, and the tile edges are swept.

Limits.  Exact kernels: max(limit of test_gpu_ops.py for that kernel, 4 x the error of the SAME formula evaluated in float32 on the
CPU) - the factor 4 covers another summation order, nothing else.  Split-bf16 kernel: 4 x the error of a CPU model of its operands
(Q * scale * log2 e, K and V as hi + lo bf16 pieces, or one piece; everything else in float64), relative to the output peak; the
flat family keeps the 3e-5 / 2e-2 of test_gpu_ops.py.  The figures below are printed by the tests (`pytest -s`, lines "ATTN ...").

Measured on an MI355X against float64 ("cpu32" = the float32 CPU formula, "model3" / "model1" = the split model with two / one
bf16 pieces); inputs are seeded, so the cpu32 / model columns and the rise counts reproduce exactly:

Causal window, H=2 dh=64 N=160 (B=2).  rises: rises > 8 between 32-key / 64-key tiles.  cpu32, valu, mfma: max abs error; model,
split: of the output peak; limit = max(2e-5, 4 x cpu32), limit3 / limit1 = 4 x model (flat: 3e-5 / 2e-2).
  window family      rises    max|s|  cpu32    limit    valu     mfma   | model3  limit3  split3 | model1  limit1  split1
  97     flat          0/0       5.0  9.3e-07  2.0e-05  7.2e-07  1.2e-06 | 4.8e-06 3.0e-05 4.8e-06 | 3.3e-03 2.0e-02 3.1e-03
  97     ramp_up     337/237    38.4  9.2e-06  3.7e-05  9.2e-06  9.3e-06 | 3.0e-05 1.2e-04 2.7e-05 | 1.5e-02 6.0e-02 1.5e-02
  97     ramp_down    78/28     43.8  7.3e-06  2.9e-05  7.3e-06  7.9e-06 | 2.9e-05 1.2e-04 3.9e-05 | 2.5e-02 9.8e-02 2.5e-02
  97     step_last   116/116    36.0  6.3e-06  2.5e-05  6.2e-06  6.0e-06 | 2.2e-05 8.9e-05 4.0e-05 | 1.1e-02 4.4e-02 1.1e-02
  97     step_first    3/0      41.1  6.3e-06  2.5e-05  6.4e-06  7.0e-06 | 2.6e-05 1.0e-04 4.4e-05 | 2.2e-02 8.9e-02 2.2e-02
  97     spike       131/131   112.4  2.4e-06  2.0e-05  2.9e-06  1.9e-06 | 4.4e-05 1.7e-04 4.5e-05 | 1.7e-02 6.8e-02 1.7e-02
  250    flat          0/0       5.0  6.5e-07  2.0e-05  6.9e-07  1.2e-06 | 4.8e-06 3.0e-05 4.8e-06 | 3.3e-03 2.0e-02 3.1e-03
  250    ramp_up     352/234    38.4  9.1e-06  3.6e-05  9.2e-06  9.2e-06 | 3.0e-05 1.2e-04 2.7e-05 | 1.5e-02 6.0e-02 1.5e-02
  250    ramp_down    38/1      46.0  7.3e-06  2.9e-05  7.7e-06  7.9e-06 | 3.4e-05 1.4e-04 3.9e-05 | 2.5e-02 1.0e-01 2.5e-02
  250    step_last   116/116    36.0  6.3e-06  2.5e-05  6.2e-06  6.0e-06 | 2.2e-05 8.9e-05 4.0e-05 | 1.1e-02 4.4e-02 1.1e-02
  250    step_first    0/0      41.1  6.6e-06  2.6e-05  6.7e-06  8.3e-06 | 3.2e-05 1.3e-04 4.4e-05 | 2.2e-02 8.9e-02 2.2e-02
  250    spike       130/129   112.4  2.9e-06  2.0e-05  2.9e-06  1.7e-06 | 4.2e-05 1.7e-04 4.3e-05 | 1.9e-02 7.5e-02 1.9e-02

Dense with klens, Tq=40 Tk=160 (B=3, H=2); limit = max(2e-5, 4 x cpu32).
  dh   family      rises    max|s|  cpu32    limit    mfma     valu
  64   flat          0/0       4.2  5.0e-07  2.0e-05  3.3e-07  3.7e-07
  64   ramp_up     276/212    42.3  7.4e-06  3.0e-05  7.9e-06  7.4e-06
  64   ramp_down    18/0      50.4  7.6e-06  3.0e-05  8.2e-06  7.5e-06
  64   step_last   113/112    36.8  6.1e-06  2.4e-05  7.3e-06  6.0e-06
  64   step_first    0/0      42.3  5.0e-06  2.0e-05  5.5e-06  4.2e-06
  64   spike       108/106   106.8  4.7e-06  2.0e-05  3.8e-06  4.2e-06
  96   flat          0/0       4.1  5.3e-07  2.0e-05  4.4e-07  6.1e-07
  96   ramp_up     289/201    38.7  9.5e-06  3.8e-05  9.4e-06  9.4e-06
  96   ramp_down    34/1      40.4  1.2e-05  4.9e-05  1.6e-05  1.2e-05
  96   step_last   107/107    34.8  1.2e-05  4.6e-05  9.0e-06  1.1e-05
  96   step_first    0/0      37.8  9.6e-06  3.8e-05  7.5e-06  9.4e-06
  96   spike       105/104   153.2  2.8e-06  2.0e-05  3.5e-06  2.7e-06
  192  flat          0/0       4.3  6.5e-07  2.0e-05  7.6e-07  8.0e-07
  192  ramp_up     271/196    36.9  1.7e-05  6.7e-05  1.6e-05  1.6e-05
  192  ramp_down    21/0      42.6  1.7e-05  6.8e-05  1.7e-05  1.7e-05
  192  step_last   114/113    34.6  1.1e-05  4.3e-05  8.7e-06  1.1e-05
  192  step_first    0/0      42.6  1.2e-05  4.7e-05  1.2e-05  1.2e-05
  192  spike       115/115   138.4  8.0e-06  3.2e-05  6.6e-06  8.5e-06

Decode, S=160 (B=8, H=4), 64-key tiles; limit = max(2e-5, 4 x cpu32).
  dh   family      rises/falls  max|s|  cpu32    limit    decode
  64   flat          0/0           3.7  2.7e-07  2.0e-05  1.5e-07
  64   ramp_up      32/8          36.9  8.9e-06  3.6e-05  1.9e-06
  64   ramp_down     0/49         35.3  4.0e-06  2.0e-05  2.1e-06
  64   step_last    22/1          32.5  8.6e-06  3.4e-05  2.0e-06
  64   step_first    0/32         35.6  4.4e-06  2.0e-05  2.3e-06
  64   spike         9/6          84.5  1.3e-06  2.0e-05  4.8e-07
  96   flat          0/0           3.6  2.7e-07  2.0e-05  1.7e-07
  96   ramp_up      26/7          34.4  6.4e-06  2.5e-05  2.0e-06
  96   ramp_down     0/52         37.3  3.8e-06  2.0e-05  1.6e-06
  96   step_last    20/4          34.5  5.8e-06  2.3e-05  2.8e-06
  96   step_first    0/32         35.9  6.2e-06  2.5e-05  2.6e-06
  96   spike        13/11         80.8  1.3e-06  2.0e-05  8.0e-07

xattn_step, S=160 (B=5, H=4, three partial sums), 64-key tiles, every head's partial output.  The limit is 5.0e-05 throughout:
4 x cpu32 stays below it (the residual slice, peak 7.3, sets the round-off).  gpu: folded fp32 / folded bf16 / unfolded fp32 / unfolded bf16.
  family      rises/falls  max|s|  cpu32 (worst form)  gpu
  flat          0/0           3.8  5.7e-07             4.9e-07 / 5.7e-07 / 4.9e-07 / 4.9e-07
  ramp_up      12/4          27.7  6.2e-07             5.8e-07 / 4.2e-07 / 5.7e-07 / 5.3e-07
  ramp_down     0/27         41.0  1.0e-06             5.3e-07 / 6.1e-07 / 5.3e-07 / 5.2e-07
  step_last    10/0          25.8  8.2e-07             5.5e-07 / 5.7e-07 / 5.5e-07 / 5.2e-07
  step_first    0/20         35.1  1.1e-06             6.6e-07 / 5.5e-07 / 6.6e-07 / 5.8e-07
  spike         9/7          92.7  5.1e-07             4.9e-07 / 5.1e-07 / 4.9e-07 / 5.1e-07

xattn_step: the gain multiplies the projected key rows (the block's RMSNorm of the context rows would cancel a gain put on the
context itself), and the family test runs at three times the softmax scale (the synthetic checkpoint's scores have a spread of 0.4).

Guard against easy inputs: for every non-flat family "at least one rise > 8 (log2) between consecutive visible key tiles" is asserted
on the CPU (32-key tiles for the MFMA kernels, 64-key tiles for the others) wherever the profile can produce one.  It cannot where
every query's first visible tile already holds the loud keys: the step on the first 32 keys with window 250 or dense keys (a rise
needs a query whose window cuts into the first tile: window 97 has 3), and both descending profiles with 64-key tiles that start
at key 0.  There the mirror image is asserted - a fall of more than 8, weights underflowing against a reference that stays put.
The counts are printed ("ATTN moves ...")."""
import itertools
import math
import random

import numpy as np
import pytest
import torch

from conftest import golden
from oracle import sopro_oracle as O
from sopro_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOG2E = 1.4426950408889634
FAMILIES = ["flat", "ramp_up", "ramp_down", "step_last", "step_first", "spike"]
SENTINEL = -12345.0


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def dev(t):
    return t.to(DEV).contiguous()


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def err_of(a, b):
    return float((a.detach().double().cpu() - b.double()).abs().max())


def close(a, b, atol, what=""):
    err = err_of(a, b)
    assert err <= atol, f"{what}: max abs err {err:.3e} > {atol:.1e}"


def gain(family, n):
    g = torch.ones(n)
    if family == "ramp_up":
        g = torch.linspace(0.2, 12.0, n)
    elif family == "ramp_down":
        g = torch.linspace(12.0, 0.2, n)
    elif family == "step_last":
        g[-32:] = 10.0
    elif family == "step_first":
        g[:32] = 10.0
    elif family == "spike":
        g[n // 2] = 40.0
    else:
        assert family == "flat"
    return g


# ------------------------------------------------------------------------------------------ references
def visible(B, Tq, Tk, klens=None, causal=False, window=0, q_pos0=0, k_pos0=0):
    """[B, Tq, Tk] bool: key tk < klens[b], and (causal) q_abs - window < k_abs <= q_abs."""
    vis = torch.ones(B, Tq, Tk, dtype=torch.bool)
    if klens is not None:
        vis &= (torch.arange(Tk)[None, None, :] < torch.as_tensor(klens)[:, None, None])
    if causal:
        qa, ka = q_pos0 + torch.arange(Tq)[:, None], k_pos0 + torch.arange(Tk)[None, :]
        vis &= ((ka <= qa) & (ka > qa - window))[None]
    return vis


def masked_softmax(s, vis):
    """softmax over the last axis of the visible entries; an all-masked row is zeros."""
    s = s.masked_fill(~vis, -math.inf)
    m = s.max(-1, keepdim=True).values
    p = torch.exp(s - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    l = p.sum(-1, keepdim=True)
    return p / torch.where(l > 0, l, torch.ones_like(l))


def attn_formula(q, k, v, H, vis, dtype=torch.float64, scale=None, scores=False):
    """q [B, Tq, H*dh], k / v [B, Tk, H*dh], vis [B, Tq, Tk] -> [B, Tq, H*dh] in ``dtype`` (the whole formula, not just the sums)."""
    dh = q.shape[-1] // H
    qh, kh, vh = (O._heads(t.to(dtype), H) for t in (q, k, v))
    s = torch.matmul(qh, kh.transpose(-1, -2)) * (dh ** -0.5 if scale is None else scale)
    if scores:
        return s.masked_fill(~vis[:, None], -math.inf)
    return O._unheads(torch.matmul(masked_softmax(s, vis[:, None]), vh))


def _pieces(x, passes):
    hi = x.to(torch.bfloat16).float()
    if passes == 1:
        return hi.double()
    return hi.double() + (x - hi).to(torch.bfloat16).double()


def split_model(q, k, v, H, vis, passes):
    """The split-bf16 kernel's operands, the rest exact: Q * (scale * log2 e) (fp32 product, as the kernel forms it), K and V
    rounded to hi + lo bf16 pieces (one piece for passes == 1); softmax in base 2 and both products in float64."""
    dh = q.shape[-1] // H
    qs = q * torch.tensor(dh ** -0.5, dtype=torch.float32) * torch.tensor(1.44269504088896340736, dtype=torch.float32)
    qh, kh, vh = (O._heads(_pieces(t, passes), H) for t in (qs, k, v))
    s = torch.matmul(qh, kh.transpose(-1, -2)) * math.log(2.0)
    return O._unheads(torch.matmul(masked_softmax(s, vis[:, None]), vh))


def tile_moves(s, tile):
    """s [..., Tk] float64 scores with -inf where masked -> (rises, falls): how often, over all queries, the maximum of a visible
    tile of ``tile`` keys (tiles start at multiples of ``tile``, as in every kernel) lies more than 8 above / below the maximum
    of the previous visible tile in the log2 domain."""
    s = s * LOG2E
    Tk = s.shape[-1]
    nt = (Tk + tile - 1) // tile
    s = torch.nn.functional.pad(s, (0, nt * tile - Tk), value=-math.inf)
    tm = s.reshape(*s.shape[:-1], nt, tile).max(-1).values
    prev = torch.full(tm.shape[:-1], -math.inf, dtype=tm.dtype)
    rises = falls = 0
    for t in range(nt):
        cur = tm[..., t]
        both = torch.isfinite(cur) & torch.isfinite(prev)
        rises += int((both & (cur > prev + 8)).sum())
        falls += int((both & (cur < prev - 8)).sum())
        prev = torch.where(torch.isfinite(cur), cur, prev)
    return rises, falls


DESCENDING = ("ramp_down", "step_first")


def assert_moves(family, s, tile, what, rise_possible=True):
    """The guard against inputs that silently degrade to the easy case: at least one rise of more than 8 (log2) between consecutive
    visible tiles; where the profile cannot give one (see the module docstring), at least one fall of more than 8."""
    rises, falls = tile_moves(s, tile)
    print(f"ATTN moves {what} {family} tile={tile}: rises>8 {rises}, falls>8 {falls}, max|score| {float(s[torch.isfinite(s)].abs().max()):.1f}")
    if family == "flat":
        return
    if not rise_possible:
        assert family in DESCENDING
        assert falls >= 1, f"{what}/{family}: the inputs degraded to the easy case (no fall > 8 between {tile}-key tiles)"
    else:
        assert rises >= 1, f"{what}/{family}: the inputs degraded to the easy case (no rise > 8 between {tile}-key tiles)"


def exact_limit(base, q_args, ref, what):
    """max(the limit test_gpu_ops.py uses, 4 x the float32 CPU formula's own error against float64)."""
    e32 = err_of(q_args, ref)
    lim = max(base, 4.0 * e32)
    print(f"ATTN cpu32 {what}: {e32:.2e} -> limit {lim:.2e}")
    return lim


def report(what, out, ref, lim, rel=False):
    e = err_of(out, ref) / (float(ref.abs().max()) if rel else 1.0)
    print(f"ATTN gpu {what}: {e:.2e} (limit {lim:.2e})")
    assert torch.isfinite(out).all(), what
    assert e <= lim, f"{what}: {e:.3e} > {lim:.3e}"


# ------------------------------------------------------------------------------------------ launchers
def run_attn(q, k, v, H, *, klens=None, causal=False, window=0, q_pos0=0, k_pos0=0, valu=False, split=0, kv_index=None, kshare=False,
             decode=False):
    """q [B, Tq, D], k / v [Bk, Tk, D] on the CPU -> O [B, Tq, D] on the device, started from NaN.  ``valu``: Q sits one float past
    a 16-byte boundary, which the MFMA entry does not take: the fp32 VALU kernel runs.  ``kshare``: k_bstride = v_bstride = 0."""
    B, Tq, D = q.shape
    Tk = k.shape[1]
    qd = torch.empty(B * Tq * D + 4, device=DEV)
    q_off = 1 if valu else 0
    qd[q_off:q_off + B * Tq * D] = dev(q).reshape(-1)
    out = torch.full((B, Tq, D), float("nan"), device=DEV)
    hip.attention(qd, dev(k), dev(v), out, B=B, H=H, dh=D // H, Tq=Tq, Tk=Tk, ldq=D, ldk=D, ldv=D, ldo=D, q_bstride=Tq * D,
                  k_bstride=0 if kshare else Tk * D, v_bstride=0 if kshare else Tk * D, o_bstride=Tq * D,
                  klens=None if klens is None else i32(klens), causal=causal, window=window, q_pos0=q_pos0, k_pos0=k_pos0, q_off=q_off,
                  kv_index=None if kv_index is None else i32(kv_index), split_passes=split, decode=decode)
    return out


def assert_zero_rows(out, vis, H, what):
    """Rows (b, tq) that see no key are exactly zero in every head; everything is finite."""
    assert torch.isfinite(out).all(), what
    dead = ~vis.any(-1)
    assert bool(dead.any()), f"{what}: the case has no row without a key"
    assert float(out.cpu()[dead].abs().max()) == 0.0, f"{what}: a row that sees no key is not exactly zero"


# ================================================================================ A. inputs that move the running maximum
@pytest.mark.parametrize("window", [97, 250])
@pytest.mark.parametrize("family", FAMILIES)
def test_window_kernels_when_the_running_maximum_moves(family, window):
    """Causal window attention, H=2, dh=64, N=160: VALU, exact MFMA and split-bf16 (3 passes, 1 pass) kernels on gain-profiled keys."""
    B, H, dh, N = 2, 2, 64, 160
    D = H * dh
    q, k, v = rnd(B, N, D, seed=903), rnd(B, N, D, seed=904) * gain(family, N)[None, :, None], rnd(B, N, D, seed=905)
    vis = visible(B, N, N, causal=True, window=window)
    s = attn_formula(q, k, v, H, vis, scores=True)
    assert_moves(family, s, 32, f"window{window}/mfma", rise_possible=not (family == "step_first" and window == 250))
    assert_moves(family, s, 64, f"window{window}/valu", rise_possible=family not in DESCENDING)
    ref = attn_formula(q, k, v, H, vis)
    lim = exact_limit(2e-5, attn_formula(q, k, v, H, vis, dtype=torch.float32), ref, f"window{window} {family}")
    kw = dict(causal=True, window=window)
    report(f"window{window} {family} valu", run_attn(q, k, v, H, valu=True, **kw), ref, lim)
    report(f"window{window} {family} mfma", run_attn(q, k, v, H, **kw), ref, lim)
    peak = float(ref.abs().max())
    for passes, flat_lim in ((3, 3e-5), (1, 2e-2)):
        em = err_of(split_model(q, k, v, H, vis, passes), ref) / peak
        slim = flat_lim if family == "flat" else 4.0 * em
        print(f"ATTN model window{window} {family} split{passes}: {em:.2e} of peak {peak:.2f} -> limit {slim:.2e}")
        report(f"window{window} {family} split{passes}", run_attn(q, k, v, H, split=passes, **kw), ref, slim, rel=True)


@pytest.mark.parametrize("dh", [64, 96, 192])
@pytest.mark.parametrize("family", FAMILIES)
def test_dense_kernels_when_the_running_maximum_moves(family, dh):
    """Dense attention with per-row key counts, Tq=40, Tk=160: exact MFMA kernel and the VALU kernel."""
    B, H, Tq, Tk = 3, 2, 40, 160
    D = H * dh
    klens = [Tk, 97, 130]
    q, k, v = rnd(B, Tq, D, seed=910), rnd(B, Tk, D, seed=911) * gain(family, Tk)[None, :, None], rnd(B, Tk, D, seed=912)
    vis = visible(B, Tq, Tk, klens)
    s = attn_formula(q, k, v, H, vis, scores=True)
    assert_moves(family, s, 32, f"dense{dh}/mfma", rise_possible=family != "step_first")
    assert_moves(family, s, 64, f"dense{dh}/valu", rise_possible=family not in DESCENDING)
    ref = attn_formula(q, k, v, H, vis)
    lim = exact_limit(2e-5, attn_formula(q, k, v, H, vis, dtype=torch.float32), ref, f"dense{dh} {family}")
    report(f"dense{dh} {family} mfma", run_attn(q, k, v, H, klens=klens), ref, lim)
    report(f"dense{dh} {family} valu", run_attn(q, k, v, H, klens=klens, valu=True), ref, lim)


@pytest.mark.parametrize("dh", [64, 96])
@pytest.mark.parametrize("family", FAMILIES)
def test_decode_kernel_when_the_running_maximum_moves(family, dh):
    B, H, S = 8, 4, 160
    D = H * dh
    klens = [S, S, 129, S, 97, S, 65, S]
    q, k, v = rnd(B, 1, D, seed=920), rnd(B, S, D, seed=921) * gain(family, S)[None, :, None], rnd(B, S, D, seed=922)
    vis = visible(B, 1, S, klens)
    assert_moves(family, attn_formula(q, k, v, H, vis, scores=True), 64, f"decode{dh}", rise_possible=family not in DESCENDING)
    ref = attn_formula(q, k, v, H, vis)
    lim = exact_limit(2e-5, attn_formula(q, k, v, H, vis, dtype=torch.float32), ref, f"decode{dh} {family}")
    report(f"decode{dh} {family}", run_attn(q, k, v, H, klens=klens, decode=True), ref, lim)


# ---- xattn_step
XP = "ar.x_attns.3"


def xattn_operands(w, B, S, np_, klens, family="flat", seed=930):
    """Operands of the block as test_gpu_ops.py builds them (folded in float64, then rounded once): the partial-sum input, folded
    K' / V', unfolded K, the raw query in four slices.  The gain multiplies the projected key rows."""
    H, D = 4, 384
    dh = D // H
    S_cap = ((S + 63) // 64) * 64
    parts = torch.stack([rnd(B, D, seed=seed + i) for i in range(np_ + 1)])
    ctx = rnd(B, S, D, seed=seed + 10)
    k, v = O.xattn_kv(ctx, w, XP, H)
    k = k * gain(family, S)[None, None, :, None]
    Wq, Wo, nq = w[XP + ".q_proj.weight"].double(), w[XP + ".out_proj.weight"].double(), w[XP + ".nq.weight"].double()
    Kp, Vp, Ku = torch.zeros(B, H, S_cap, D), torch.zeros(B, H, S_cap, D), torch.zeros(B, S_cap, D)
    for h in range(H):
        Kp[:, h, :S] = ((k[:, h].double() @ Wq[h * dh:(h + 1) * dh]) * nq).float()
        Vp[:, h, :S] = (v[:, h].double() @ Wo[:, h * dh:(h + 1) * dh].t()).float()
        Ku[:, :S, h * dh:(h + 1) * dh] = k[:, h]
    x = parts.double().sum(0)
    q_raw = (x @ (Wq * nq[None, :]).t()).float()
    cuts = torch.rand(3, B, D, generator=torch.Generator().manual_seed(3))
    qparts = torch.stack([q_raw * cuts[0], q_raw * (1 - cuts[0]) * cuts[1], q_raw * (1 - cuts[0]) * (1 - cuts[1]) * cuts[2],
                          q_raw * (1 - cuts[0]) * (1 - cuts[1]) * (1 - cuts[2])])
    kw = dict(B=B, H=H, D=D, S_cap=S_cap, gate=float(torch.tanh(w[XP + ".gate"])), scale=dh ** -0.5, eps=1e-6, np_=np_, xp_stride=B * D,
              y_part_stride=B * D)
    return parts, Kp, Vp, Ku, qparts, kw


def xattn_formula(parts, Kp, Vp, klens, kw, dtype=torch.float64, Ku=None, qparts=None, scores=False):
    """include/sopro_hip.h: Y[h][b] = (h == 0 ? Xin[b] : 0) + gate * sum_k softmax_k(<RMSNorm(Xin[b]), Kp[b,h,k]> * scale) Vp[b,h,k];
    unfolded keys: the score is <rstd * sum_s Qp[s][b, head h], K[b, k, head h]>.  -> Y [H, B, D] in ``dtype``."""
    B, H, D, S_cap = kw["B"], kw["H"], kw["D"], kw["S_cap"]
    xin = parts[0].to(dtype)
    for s_ in range(1, parts.shape[0]):
        xin = xin + parts[s_].to(dtype)
    rstd = torch.rsqrt(xin.pow(2).mean(-1, keepdim=True) + kw["eps"])
    if Ku is None:
        s = torch.einsum("bd,bhkd->bhk", xin * rstd, Kp.to(dtype))
    else:
        qr = qparts[0].to(dtype)
        for s_ in range(1, qparts.shape[0]):
            qr = qr + qparts[s_].to(dtype)
        s = torch.einsum("bhe,bkhe->bhk", (qr * rstd).view(B, H, D // H), Ku.to(dtype).view(B, S_cap, H, D // H))
    s = s * kw["scale"]
    vis = (torch.arange(S_cap)[None, :] < torch.as_tensor(klens)[:, None])[:, None, :].expand(B, H, S_cap)
    if scores:
        return s.masked_fill(~vis, -math.inf)
    y = kw["gate"] * torch.einsum("bhk,bhkd->hbd", masked_softmax(s, vis), Vp.to(dtype))
    y[0] += xin
    return y


def run_xattn(parts, Kp, Vp, klens, kw, Ku=None, qparts=None, bf16=False):
    B, H, D = kw["B"], kw["H"], kw["D"]
    Pd = dev(parts)
    Y = torch.full((H, B, D), float("nan"), device=DEV)
    cast = (lambda t: dev(t).to(torch.bfloat16)) if bf16 else dev
    extra = {} if Ku is None else dict(Qp=dev(qparts), nqp=qparts.shape[0], qp_stride=B * D)
    hip.xattn_step(Pd[0], Y, None, cast(Kp if Ku is None else Ku), cast(Vp), i32(klens), Xp=Pd[1:] if kw["np_"] else None, **extra, **kw)
    return Y


def bf16_values(t):
    return t.to(torch.bfloat16).float()


@pytest.mark.parametrize("family", FAMILIES)
def test_xattn_step_when_the_running_maximum_moves(family, w):
    """S=160 (three 64-key tiles): folded and unfolded keys, fp32 and bf16 storage; every head's partial output against float64.
    The bf16-stored forms are exact kernels on the bf16 values, so their reference is the formula on those values."""
    B, S = 5, 160
    klens = [S, 129, 65, S, 97]
    parts, Kp, Vp, Ku, qparts, kw = xattn_operands(w, B, S, 3, klens, family)
    kw["scale"] *= 3.0  # the synthetic checkpoint's scores have a spread of 0.4: three times the softmax scale makes them unit-scale
    for unfolded in (False, True):
        for bf16 in (False, True):
            what = f"xattn {'unfolded' if unfolded else 'folded'} {'bf16' if bf16 else 'fp32'}"
            K_, V_, U_ = (bf16_values(t) for t in (Kp, Vp, Ku)) if bf16 else (Kp, Vp, Ku)
            fa = dict(Ku=U_, qparts=qparts) if unfolded else {}
            assert_moves(family, xattn_formula(parts, K_, V_, klens, kw, scores=True, **fa), 64, what, rise_possible=family not in DESCENDING)
            ref = xattn_formula(parts, K_, V_, klens, kw, **fa)
            lim = exact_limit(5e-5, xattn_formula(parts, K_, V_, klens, kw, dtype=torch.float32, **fa), ref, f"{what} {family}")
            report(f"{what} {family}", run_xattn(parts, Kp, Vp, klens, kw, bf16=bf16, **({"Ku": Ku, "qparts": qparts} if unfolded else {})), ref, lim)


# ================================================================================ B. kv_index
KV_INDEX = [1, 0, 1, 1, 0]


def _kv_case(H, dh, Tq, Tk, seed):
    D = H * dh
    return rnd(5, Tq, D, seed=seed), rnd(2, Tk, D, seed=seed + 1), rnd(2, Tk, D, seed=seed + 2)


@pytest.mark.parametrize("H,dh,Tq,Tk", [(4, 96, 7, 70), (4, 96, 40, 70), (2, 192, 40, 70), (2, 192, 7, 33)])
def test_kv_index_dense_equals_gathered_blocks(H, dh, Tq, Tk):
    """Rows that share a voice read one K/V block; klens stay per ROW.  Bit-equal to a call on explicitly gathered K/V.
    Tq = 7 runs the VALU kernel, Tq = 40 the dense MFMA kernel."""
    q, k, v = _kv_case(H, dh, Tq, Tk, 940)
    klens = [Tk, Tk - 1, max(1, Tk // 3), 33, 1]
    got = run_attn(q, k, v, H, klens=klens, kv_index=KV_INDEX)
    want = run_attn(q, k[KV_INDEX], v[KV_INDEX], H, klens=klens)
    assert torch.equal(got, want)
    close(got, attn_formula(q, k[KV_INDEX], v[KV_INDEX], H, visible(5, Tq, Tk, klens)), 2e-5, "kv_index, dense")


@pytest.mark.parametrize("split", [0, 3, 1])
def test_kv_index_causal_window_equals_gathered_blocks(split):
    H, dh, N = 2, 64, 40
    q, k, v = _kv_case(H, dh, N, N, 945)
    klens = [N, N - 1, 13, 33, 1]
    kw = dict(klens=klens, causal=True, window=17, split=split)
    got = run_attn(q, k, v, H, kv_index=KV_INDEX, **kw)
    want = run_attn(q, k[KV_INDEX], v[KV_INDEX], H, **kw)
    assert torch.equal(got, want)
    vis = visible(5, N, N, klens, True, 17)
    ref = attn_formula(q, k[KV_INDEX], v[KV_INDEX], H, vis)
    if split:
        assert err_of(got, ref) / float(ref.abs().max()) < (3e-5 if split == 3 else 2e-2)
    else:
        close(got, ref, 2e-5, "kv_index, causal window")
    assert_zero_rows(got, vis, H, "kv_index, causal window with short rows")


@pytest.mark.parametrize("H,dh,Tq,causal,split", [(4, 96, 7, False, 0), (2, 192, 40, False, 0), (2, 64, 40, True, 0), (2, 64, 40, True, 3)])
def test_one_shared_block_with_zero_batch_stride(H, dh, Tq, causal, split):
    """One voice for the whole batch: k_bstride = v_bstride = 0, no kv_index."""
    B, Tk = 5, 40
    q, k, v = rnd(B, Tq, H * dh, seed=950), rnd(1, Tk, H * dh, seed=951), rnd(1, Tk, H * dh, seed=952)
    klens = [Tk, Tk - 1, 13, 33, 1]
    kw = dict(klens=klens, causal=causal, window=250 if causal else 0, q_pos0=Tk - Tq if causal else 0, split=split)
    got = run_attn(q, k, v, H, kshare=True, **kw)
    ke, ve = k.expand(B, -1, -1).contiguous(), v.expand(B, -1, -1).contiguous()
    assert torch.equal(got, run_attn(q, ke, ve, H, **kw))
    vis = visible(B, Tq, Tk, klens, causal, 250, Tk - Tq if causal else 0)
    ref = attn_formula(q, ke, ve, H, vis)
    if split:
        assert err_of(got, ref) / float(ref.abs().max()) < 3e-5
    else:
        close(got, ref, 2e-5, "shared block")


def test_decode_rejects_kv_index():
    q, k, v = _kv_case(4, 96, 1, 19, 955)
    out = torch.full((5, 1, 384), 7.0, device=DEV)
    with pytest.raises(hip.SoproHipError, match="kv_index"):
        hip.attention(dev(q), dev(k), dev(v), out, B=5, H=4, dh=96, Tq=1, Tk=19, ldq=384, ldk=384, ldv=384, ldo=384, q_bstride=384,
                      k_bstride=19 * 384, v_bstride=19 * 384, o_bstride=384, kv_index=i32(KV_INDEX), decode=True)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched


# ================================================================================ C. rows that see nothing
@pytest.mark.parametrize("kernel,H,dh,Tq,Tk", [("valu", 4, 96, 7, 70), ("valu", 2, 64, 40, 70), ("mfma", 2, 64, 40, 70), ("mfma", 4, 96, 40, 70),
                                               ("mfma", 2, 192, 33, 33), ("decode", 4, 96, 1, 70), ("decode", 4, 64, 1, 130)])
def test_rows_with_zero_keys_are_zero_dense(kernel, H, dh, Tq, Tk):
    B = 4
    klens = [Tk, 0, 33, 0]
    q, k, v = rnd(B, Tq, H * dh, seed=960), rnd(B, Tk, H * dh, seed=961), rnd(B, Tk, H * dh, seed=962)
    got = run_attn(q, k, v, H, klens=klens, valu=kernel == "valu", decode=kernel == "decode")
    vis = visible(B, Tq, Tk, klens)
    assert_zero_rows(got, vis, H, kernel)
    close(got, attn_formula(q, k, v, H, vis), 2e-5, f"{kernel}: rows next to the empty ones")


# (N, Tk, window, q_pos0, k_pos0): window 4 far into a stream whose keys start 6 positions AFTER the first query; a whole
# 32-query tile (and part of the next) in front of the first key; keys cached so long ago that only the first queries reach them
NO_KEY_CASES = [(40, 40, 4, 1000, 1006), (80, 80, 250, 1000, 1035), (80, 50, 20, 1000, 940), (129, 64, 33, 45, 77)]


@pytest.mark.parametrize("kernel", ["valu", "mfma", "split3", "split1"])
@pytest.mark.parametrize("N,Tk,window,q_pos0,k_pos0", NO_KEY_CASES)
def test_causal_rows_outside_every_window_are_zero(kernel, N, Tk, window, q_pos0, k_pos0):
    B, H, dh = 2, 2, 64
    klens = [Tk, 0] if N == 40 else [Tk, max(1, Tk - 7)]
    q, k, v = rnd(B, N, H * dh, seed=965), rnd(B, Tk, H * dh, seed=966), rnd(B, Tk, H * dh, seed=967)
    kw = dict(klens=klens, causal=True, window=window, q_pos0=q_pos0, k_pos0=k_pos0)
    got = run_attn(q, k, v, H, valu=kernel == "valu", split=int(kernel[5:]) if kernel.startswith("split") else 0, **kw)
    vis = visible(B, N, Tk, klens, True, window, q_pos0, k_pos0)
    assert bool(vis.any()), "the case must keep rows that do see keys"
    assert_zero_rows(got, vis, H, kernel)
    ref = attn_formula(q, k, v, H, vis)
    if kernel.startswith("split"):
        assert err_of(got, ref) / float(ref.abs().max()) < (3e-5 if kernel == "split3" else 2e-2)
    else:
        close(got, ref, 2e-5, f"{kernel}: rows next to the empty ones")


@pytest.mark.parametrize("unfolded,bf16", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("S,np_", [(19, 0), (130, 3)])
def test_xattn_step_row_without_keys_passes_its_input_through(S, np_, unfolded, bf16, w):
    """klens[b] == 0: Y[0][b] = Xin[b] (the input plus the partials, in slice order) and Y[h > 0][b] = 0, exactly."""
    B = 5
    klens = [S, 0, max(1, S // 2), 0, S - 3]
    parts, Kp, Vp, Ku, qparts, kw = xattn_operands(w, B, S, np_, klens)
    Y = run_xattn(parts, Kp, Vp, klens, kw, bf16=bf16, **({"Ku": Ku, "qparts": qparts} if unfolded else {})).cpu()
    assert torch.isfinite(Y).all()
    xin = parts[0].clone()
    for s_ in range(1, np_ + 1):
        xin += parts[s_]
    for b in (1, 3):
        assert torch.equal(Y[0, b], xin[b]), f"row {b} without keys: the residual slice is not the input"
        assert float(Y[1:, b].abs().max()) == 0.0
    K_, V_, U_ = (bf16_values(t) for t in (Kp, Vp, Ku)) if bf16 else (Kp, Vp, Ku)
    close(Y, xattn_formula(parts, K_, V_, klens, kw, **({"Ku": U_, "qparts": qparts} if unfolded else {})), 5e-5, "rows next to the empty ones")


def xattn_golden_operands(B, S, np_):
    """Operands for the bit-identity fixtures: small integers (a 64-bit integer mix of the element index) over a power of two,
    so that every host produces the same bits: no BLAS, no transcendental and no library generator in their making."""
    H, D = 4, 384
    S_cap = ((S + 63) // 64) * 64

    def draw(salt, *shape, den):
        h = (np.arange(int(np.prod(shape)), dtype=np.uint64) + np.uint64(1000003 * salt + S)) * np.uint64(0x9E3779B97F4A7C15)
        h ^= h >> np.uint64(29)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(32)
        v = (h % np.uint64(513)).astype(np.int64) - 256
        return torch.from_numpy((v.astype(np.float32) / np.float32(den)).reshape(shape))

    parts = draw(1, np_ + 1, B, D, den=128.0)
    Kp, Vp, Ku = draw(2, B, H, S_cap, D, den=128.0), draw(3, B, H, S_cap, D, den=256.0), draw(4, B, S_cap, D, den=128.0)
    qparts = draw(5, 4, B, D, den=256.0)
    kw = dict(B=B, H=H, D=D, S_cap=S_cap, gate=0.75, scale=96 ** -0.5, eps=1e-6, np_=np_, xp_stride=B * D, y_part_stride=B * D)
    return parts, Kp, Vp, Ku, qparts, kw


XATTN_GOLDEN_CASES = [(5, 19, 0), (5, 64, 3), (5, 130, 3), (8, 130, 3)]


def xattn_golden_outputs():
    """Every form of the block on the cases of test_gpu_ops.py's xattn_step tests (B=5; S, partial sums = (19, 0), (64, 3), (130, 3);
    its klens) plus the B=8 case that takes the non-temporal bf16 variant -> {name: Y [H, B, D]}."""
    out = {}
    for B, S, np_ in XATTN_GOLDEN_CASES:
        klens = ([S, 1, max(1, S // 2), S, max(1, S - 3)] * 2)[:B]
        parts, Kp, Vp, Ku, qparts, kw = xattn_golden_operands(B, S, np_)
        for unfolded in (False, True):
            for bf16 in (False, True):
                Y = run_xattn(parts, Kp, Vp, klens, kw, bf16=bf16, **({"Ku": Ku, "qparts": qparts} if unfolded else {}))
                out[f"B{B}_S{S}_{'u' if unfolded else 'f'}_{'bf16' if bf16 else 'fp32'}"] = Y.cpu().numpy()
    return out


def test_xattn_step_outputs_with_keys_are_bit_identical_to_the_recorded_ones():
    """The klens == 0 handling must not move any other output by a bit: tests/golden/xattn_step_bits.npz holds what the kernel
    wrote before that change (all four forms, both load variants)."""
    want = golden("xattn_step_bits")
    got = xattn_golden_outputs()
    assert sorted(got) == sorted(want.files)
    for name, y in got.items():
        assert np.isfinite(y).all(), name
        assert np.array_equal(y.view(np.uint32), want[name].view(np.uint32)), f"{name}: xattn_step output changed"


# ================================================================================ D. mask and path combinations
@pytest.mark.parametrize("kernel", ["valu", "mfma", "split3"])
def test_causal_window_with_per_row_key_counts(kernel):
    B, H, dh, N, past, win = 4, 2, 64, 70, 10, 40
    Tk = N + past
    klens = [1, 31, 33, Tk]
    q, k, v = rnd(B, N, H * dh, seed=970), rnd(B, Tk, H * dh, seed=971), rnd(B, Tk, H * dh, seed=972)
    kw = dict(klens=klens, causal=True, window=win, q_pos0=past)
    got = run_attn(q, k, v, H, valu=kernel == "valu", split=3 if kernel == "split3" else 0, **kw)
    vis = visible(B, N, Tk, klens, True, win, past)
    ref = attn_formula(q, k, v, H, vis)
    assert_zero_rows(got, vis, H, kernel)  # late queries of the short rows have their whole window past klens[b]
    if kernel == "split3":
        assert err_of(got, ref) / float(ref.abs().max()) < 3e-5
    else:
        close(got, ref, 2e-5, f"causal + klens, {kernel}")


@pytest.mark.parametrize("dh,Tq", [(96, 16), (96, 40), (192, 16), (192, 40)])
def test_causal_wide_heads_run_the_valu_kernel(dh, Tq):
    B, H, past, win = 2, 2, 30, 25
    Tk = Tq + past
    q, k, v = rnd(B, Tq, H * dh, seed=975), rnd(B, Tk, H * dh, seed=976), rnd(B, Tk, H * dh, seed=977)
    got = run_attn(q, k, v, H, causal=True, window=win, q_pos0=past)
    close(got, attn_formula(q, k, v, H, visible(B, Tq, Tk, None, True, win, past)), 2e-5, "causal, wide heads")


@pytest.mark.parametrize("split", [0, 3])
@pytest.mark.parametrize("N,win,past", [(16, 250, 300), (95, 40, 1000), (33, 64, 45)])
def test_cached_keys_with_a_batch(N, win, past, split):
    """The batched streaming decoder's shape: past > 0 and B = 3."""
    B, H, dh = 3, 8, 64
    Tk = N + min(past, win - 1)
    q, k, v = rnd(B, N, H * dh, seed=980), rnd(B, Tk, H * dh, seed=981), rnd(B, Tk, H * dh, seed=982)
    kw = dict(causal=True, window=win, q_pos0=past, k_pos0=past + N - Tk)
    got = run_attn(q, k, v, H, split=split, **kw)
    ref = attn_formula(q, k, v, H, visible(B, N, Tk, None, True, win, past, past + N - Tk))
    if split:
        assert err_of(got, ref) / float(ref.abs().max()) < 3e-5
    else:
        close(got, ref, 2e-5, "cached keys, B = 3")


@pytest.mark.parametrize("case", ["dh96", "tq15", "o_unaligned"])
def test_split_entry_hands_other_shapes_to_the_exact_kernel(case):
    B, H, dh, N = 2, 2, (96 if case == "dh96" else 64), (15 if case == "tq15" else 40)
    D = H * dh
    o_off = 1 if case == "o_unaligned" else 0
    q, k, v = dev(rnd(B, N, D, seed=985)), dev(rnd(B, N, D, seed=986)), dev(rnd(B, N, D, seed=987))
    outs = []
    for passes in (3, 1, 0):
        out = torch.full((B * N * D + 4,), float("nan"), device=DEV)
        hip.attention(q, k, v, out, B=B, H=H, dh=dh, Tq=N, Tk=N, ldq=D, ldk=D, ldv=D, ldo=D, q_bstride=N * D, k_bstride=N * D, v_bstride=N * D,
                      o_bstride=N * D, causal=True, window=17, o_off=o_off, split_passes=passes)
        outs.append(out[o_off:o_off + B * N * D].view(B, N, D))
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[2])
    close(outs[2], attn_formula(q.cpu(), k.cpu(), v.cpu(), H, visible(B, N, N, None, True, 17)), 2e-5, case)


@pytest.mark.parametrize("S", [1, 63, 64, 65, 129])
def test_decode_with_64_wide_heads(S):
    B, H, dh = 5, 4, 64
    klens = [S, 1, max(1, S // 2), S, max(1, S - 3)]
    q, k, v = rnd(B, 1, H * dh, seed=990), rnd(B, S, H * dh, seed=991), rnd(B, S, H * dh, seed=992)
    got = run_attn(q, k, v, H, klens=klens, decode=True)
    close(got, attn_formula(q, k, v, H, visible(B, 1, S, klens)), 2e-5, "decode, dh = 64")


@pytest.mark.parametrize("unfolded", [False, True])
def test_xattn_step_bf16_storage_large_enough_for_the_streaming_loads(unfolded, w):
    """B=8, S=130 (S_cap=192): 8*4*192*384 bf16 operands x 2 > 8 MiB, the non-temporal bf16 variant.  Against the same bf16 values
    held in fp32 (as test_gpu_ops.py does for the cached variant) and against float64."""
    B, S = 8, 130
    assert B * 4 * 192 * 384 * 4 > (8 << 20)
    klens = [S, 1, S // 2, S, S - 3, 64, 65, 129]
    parts, Kp, Vp, Ku, qparts, kw = xattn_operands(w, B, S, 3, klens)
    fa = {"Ku": Ku, "qparts": qparts} if unfolded else {}
    Y16 = run_xattn(parts, Kp, Vp, klens, kw, bf16=True, **fa)
    K_, V_, U_ = (bf16_values(t) for t in (Kp, Vp, Ku))
    fb = {"Ku": U_, "qparts": qparts} if unfolded else {}
    Y32 = run_xattn(parts, K_, V_, klens, kw, **fb)
    close(Y16.sum(0), Y32.sum(0).cpu(), 2e-5, "bf16-stored operands vs the same values in fp32")
    close(Y16, xattn_formula(parts, K_, V_, klens, kw, **fb), 5e-5, "bf16-stored operands vs float64")


# ================================================================================ E. edge sweep
TQS, KLENS, WINDOWS, OFFSETS = [16, 31, 32, 33, 127, 128, 129], [1, 31, 32, 33, 63, 64, 65], [1, 2, 31, 32, 33, 64], [0, 1, 31, 45]


def causal_sweep_cases():
    """Subset rule: all 7 x 7 x 6 x 4 x 4 = 4704 (Tq, klen, window, q offset, k offset) combinations in itertools.product order,
    150 of them drawn with random.Random(20).sample, kept in product order.  Every value of every axis occurs (asserted)."""
    allc = list(itertools.product(TQS, KLENS, WINDOWS, OFFSETS, OFFSETS))
    picked = sorted(random.Random(20).sample(range(len(allc)), 150))
    cases = [allc[i] for i in picked]
    for axis, values in enumerate((TQS, KLENS, WINDOWS, OFFSETS, OFFSETS)):
        assert {c[axis] for c in cases} == set(values)
    return cases


@pytest.mark.parametrize("kernel", ["valu", "mfma", "split3"])
def test_edge_sweep_causal_window(kernel):
    """H=1, B=2, dh=64.  64 cached keys in front of the Tq new ones; the queries start q_off after the cache, the keys are numbered
    from k_off; row 0 has klen keys (so most of its queries see nothing), row 1 all of them."""
    B, H, dh = 2, 1, 64
    Q, K, V = rnd(B, 129, dh, seed=1001), rnd(B, 193, dh, seed=1002), rnd(B, 193, dh, seed=1003)
    worst = 0.0
    for Tq, klen, win, qo, ko in causal_sweep_cases():
        Tk = Tq + 64
        q, k, v = Q[:, :Tq].contiguous(), K[:, :Tk].contiguous(), V[:, :Tk].contiguous()
        kw = dict(klens=[klen, Tk], causal=True, window=win, q_pos0=64 + qo, k_pos0=ko)
        got = run_attn(q, k, v, H, valu=kernel == "valu", split=3 if kernel == "split3" else 0, **kw)
        vis = visible(B, Tq, Tk, [klen, Tk], True, win, 64 + qo, ko)
        ref = attn_formula(q, k, v, H, vis)
        what = f"{kernel} Tq={Tq} klen={klen} window={win} q_off={qo} k_off={ko}"
        assert torch.isfinite(got).all(), what
        dead = ~vis.any(-1)
        if bool(dead.any()):
            assert float(got.cpu()[dead].abs().max()) == 0.0, what
        e = err_of(got, ref) / (max(float(ref.abs().max()), 1e-30) if kernel == "split3" else 1.0)
        worst = max(worst, e)
        assert e <= (3e-5 if kernel == "split3" else 2e-5), f"{what}: {e:.3e}"
    print(f"ATTN sweep causal {kernel}: worst {worst:.2e}")


@pytest.mark.parametrize("kernel", ["valu", "mfma"])
def test_edge_sweep_dense(kernel):
    """All 7 x 7 (Tq, klen) pairs at each head width, Tk = 65: 147 cases, none dropped."""
    B, H = 2, 1
    for dh in (64, 96, 192):
        Q, K, V = rnd(B, 129, dh, seed=1011), rnd(B, 65, dh, seed=1012), rnd(B, 65, dh, seed=1013)
        for Tq, klen in itertools.product(TQS, KLENS):
            q = Q[:, :Tq].contiguous()
            got = run_attn(q, K, V, H, klens=[klen, 65], valu=kernel == "valu")
            close(got, attn_formula(q, K, V, H, visible(B, Tq, 65, [klen, 65])), 2e-5, f"{kernel} dh={dh} Tq={Tq} klen={klen}")


def test_edge_sweep_decode():
    """Every klen at both head widths, with S = klen (the last tile ends the buffer) and S = 65."""
    B, H = 2, 1
    for dh in (64, 96):
        Q, K, V = rnd(B, 1, dh, seed=1021), rnd(B, 65, dh, seed=1022), rnd(B, 65, dh, seed=1023)
        for klen in KLENS:
            for S in sorted({klen, 65}):
                k, v = K[:, :S].contiguous(), V[:, :S].contiguous()
                got = run_attn(Q, k, v, H, klens=[klen, S], decode=True)
                close(got, attn_formula(Q, k, v, H, visible(B, 1, S, [klen, S])), 2e-5, f"decode dh={dh} klen={klen} S={S}")


def test_edge_sweep_xattn_step(w):
    """Every klen in each of the four forms (S_cap = 128)."""
    B, S = 2, 65
    parts, Kp, Vp, Ku, qparts, kw = xattn_operands(w, B, S, 1, [S, S])
    Kb, Vb, Ub = (bf16_values(t) for t in (Kp, Vp, Ku))
    for klen in KLENS:
        klens = [klen, S]
        for unfolded in (False, True):
            for bf16 in (False, True):
                K_, V_, U_ = (Kb, Vb, Ub) if bf16 else (Kp, Vp, Ku)
                Y = run_xattn(parts, Kp, Vp, klens, kw, bf16=bf16, **({"Ku": Ku, "qparts": qparts} if unfolded else {}))
                ref = xattn_formula(parts, K_, V_, klens, kw, **({"Ku": U_, "qparts": qparts} if unfolded else {}))
                close(Y, ref, 5e-5, f"xattn_step klen={klen} unfolded={unfolded} bf16={bf16}")


# ================================================================================ F. output discipline
@pytest.mark.parametrize("kernel,H,dh,causal", [("mfma", 2, 64, True), ("split3", 2, 64, True), ("split1", 2, 64, True), ("valu", 2, 96, True),
                                                ("mfma_dense", 2, 96, False), ("mfma_dense", 1, 192, False)])
@pytest.mark.parametrize("Tq", [33, 129])
def test_outputs_stay_inside_their_rows_and_repeat_bit_for_bit(kernel, H, dh, causal, Tq):
    """Q, K, V read from fused [q|k|v] rows (ld = 3 D); O written at a column offset into wider rows (ldo = D + 64) between
    sentinel guard rows: no sentinel moves, every element of the output window is written, two runs agree bit for bit."""
    B, D, G = 2, H * dh, 3
    ldo, col0 = D + 64, 32
    qkv = rnd(B, Tq, 3 * D, seed=1030)
    qkvd = dev(qkv)
    rows = B * Tq + 2 * G
    inside = torch.zeros(rows, ldo, dtype=torch.bool)
    inside[G:G + B * Tq, col0:col0 + D] = True
    inside = inside.to(DEV)
    outs = []
    for _ in range(2):
        buf = torch.full((rows, ldo), SENTINEL, device=DEV)
        buf[inside] = float("nan")
        hip.attention(qkvd, qkvd, qkvd, buf, B=B, H=H, dh=dh, Tq=Tq, Tk=Tq, ldq=3 * D, ldk=3 * D, ldv=3 * D, ldo=ldo, q_bstride=Tq * 3 * D,
                      k_bstride=Tq * 3 * D, v_bstride=Tq * 3 * D, o_bstride=Tq * ldo, causal=causal, window=40 if causal else 0, k_off=D,
                      v_off=2 * D, o_off=G * ldo + col0, split_passes=int(kernel[5:]) if kernel.startswith("split") else 0)
        assert bool((buf[~inside] == SENTINEL).all()), f"{kernel}: wrote outside the output window"
        assert not bool(torch.isnan(buf[inside]).any()), f"{kernel}: left part of the output window unwritten"
        outs.append(buf)
    assert torch.equal(outs[0], outs[1])
    got = outs[0][G:G + B * Tq, col0:col0 + D].reshape(B, Tq, D)
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    ref = attn_formula(q, k, v, H, visible(B, Tq, Tq, None, causal, 40))
    if kernel.startswith("split"):
        assert err_of(got, ref) / float(ref.abs().max()) < (3e-5 if kernel == "split3" else 2e-2)
    else:
        close(got, ref, 2e-5, kernel)


def test_decode_and_xattn_step_repeat_bit_for_bit_between_guards(w):
    B, H, dh, S = 5, 4, 96, 130
    D = H * dh
    q, k, v = rnd(B, 1, D, seed=1040), rnd(B, S, D, seed=1041), rnd(B, S, D, seed=1042)
    klens = [S, 1, 65, 64, S - 3]
    outs = []
    for _ in range(2):
        buf = torch.full((B + 2, D), SENTINEL, device=DEV)
        buf[1:B + 1] = float("nan")
        hip.attention(dev(q), dev(k), dev(v), buf, B=B, H=H, dh=dh, Tq=1, Tk=S, ldq=D, ldk=D, ldv=D, ldo=D, q_bstride=D, k_bstride=S * D,
                      v_bstride=S * D, o_bstride=D, klens=i32(klens), o_off=D, decode=True)
        assert bool((buf[0] == SENTINEL).all()) and bool((buf[B + 1] == SENTINEL).all()) and not bool(torch.isnan(buf).any())
        outs.append(buf)
    assert torch.equal(outs[0], outs[1])
    parts, Kp, Vp, Ku, qparts, kw = xattn_operands(w, B, S, 3, klens)
    ys = [run_xattn(parts, Kp, Vp, klens, kw, Ku=Ku, qparts=qparts) for _ in range(2)]
    assert torch.equal(ys[0], ys[1]) and torch.isfinite(ys[0]).all()
