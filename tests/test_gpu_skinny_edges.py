"""Edge rows and columns, strides, K-slices, partial-sum input, the RMSNorm row scale, the GLU tail's ring arithmetic, aux tiles and
the two weight packers of the AR-step contraction (sopro_skinny_f32, csrc/skinny_f32.hip) against the float64 reference of
tests/skinny_ref.py.

Every case has slack in every stride and NaN canaries in all output slack, in guard rows in front of and behind Y, aux_Y, every
partial slice and the ring, in the X / Xp / W row slack, behind bias, scale, dw_w and dw_b, and in the R slack.  Ring rows
B .. ring_bcap-1 are NaN (the kernel clamps its reads to row B-1, so they must stay NaN); ring rows < B are FINITE in every slot,
because the dead taps (ksize < 13) multiply real ring words by a zero weight and a NaN there would poison a correct kernel.  After
a launch the WHOLE buffer is compared with the reference's copy: owned words are held to tolerance, all others bit for bit.

Tolerances (derived, never fitted to a kernel's output; U = 2^-24; the rules are those of tests/test_gpu_gemm_edges.py).
Pre-activation, fp32 weights: c * U * (rs |Xin| |W|^T) + U |bias| with c = 384 = the K-slice (an fma chain; a wave's chain is 96
long and the cross-wave sum of four partials lies inside it); where ONE workgroup walks n slices (ksplit = 0, K = 384 n) a wave's
chain is 96 n long plus the three cross-wave sums, so c = max(384, 96 n + 3) (387 at K = 1536: the term the K-slice rule lacks).
bf16 weights: the same on the magnitudes of the bf16-rounded operands against the float64 product of the rounded operands.  No flip
charge for the operands: Xin = ((X + Xp0) + Xp1) + Xp2 is reproduced in fp32 bit for bit, so both sides round the same number.
RMSNorm row scale: (384 * 2^-25 + 4 U) * (rs |Xin| |W|^T + |bias|) more.  A K-slice is judged alone against its own 384-wide
float64 partial sum (slice 0 with bias + residual under RES).  Through the epilogue by its Lipschitz constant - GELU 1.13, tanh 1,
RES |scale| (plus U |scale * pre| for the product) - plus U |out| for the result; erff's GELU, tanhf and the precise sigmoid are
library functions without a stated figure: 4 x the error of torch's fp32 CPU evaluation against float64 on the case's own
pre-activations.  GLU tail: delta_h = sigmoid(g) delta_v + |v| delta_g / 4 + (sigmoid allowance) |v| + U |h|;
delta_y = |w_new| delta_h + 14 U (sum_j |w_j| |tap_j| + |dw_b|) (thirteen fmas and one add); Y: U |Y| more for Xin + y.  The
written ring slot: within delta_h (fp32 ring); bf16 ring: bf16(h_ref) exactly, or the neighbouring bf16 value only where h_ref lies
within delta_h of a rounding boundary (gemm_ref.bf16_flip_charge) - stated for every size of delta_h: another value than
bf16(h_ref) must be the bf16 rounding of some number within delta_h of h_ref, which below the spacing is that neighbour and nothing
else, and where h = v sigmoid(g) is so near 0 that delta_h exceeds the spacing (first run: one word, |h| = 8.9e-7, delta_h = 8.5e-5,
two steps off) may lie further; the words that may use the allowance are capped per case at ten
times 2 delta_h / (bf16 spacing) averaged over the case - a figure of the reference alone, asserted on the CPU.  Chained frames:
the older taps are the device's own h (each within its delta_h of the reference's), so delta_y = sum_j |w_j| delta_h(tap j) + the
same 14 U term.  Bit-equality claims (mt x nt, row-major against packed weights, repeated launches, ksplit = 1 at K = 384, main
and aux tiles against launches of their own) are exact.

Worst error / tolerance per group and the measured libm errors on an MI355X: profiles/skinny_edges.md (every comparison feeds
`WORST`; `pytest -s` prints the table last).
"""
import ctypes as C

import pytest
import torch

import gemm_ref as G
import skinny_ref as S
from sopro_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
U = 2.0 ** -24
NONE, GELU, RES, TANH, GLU_DW = S.EPI_NONE, S.EPI_GELU, S.EPI_RES, S.EPI_TANH, S.EPI_GLU_DW
LAYOUTS = ("row", "packed", "bf16")
WORST = {}   # group -> (error / tolerance, what)
LIBM = {}    # function -> largest measured fp32-vs-float64 error of torch's CPU evaluation (x 4 = the allowance)
NEIGH = {"words": 0, "flagged": 0, "used": 0, "worst_share_of_cap": 0.0}   # bf16 ring: neighbour allowance bookkeeping
COUNT = {"streams": 0}
D = 384


def up(x, a):
    return -(-x // a) * a


def gen(seed):
    return torch.Generator().manual_seed(seed)


def nanbuf(n, dtype=torch.float32):
    return torch.full((n,), NAN, dtype=dtype)


# ------------------------------------------------------------------------------------------------ operands
_w = {}


def weight(N, K, wseed=0):
    key = (N, K, wseed)
    if key not in _w:
        _w[key] = {"W": torch.randn(N, K, generator=gen(1000 + wseed + 7 * N + 13 * K)) * K ** -0.5}
    return _w[key]


def w_operand(N, K, wseed, layout, glu=False):
    """Device image of the weight in the layout, made once per module: (tensor, ldw)."""
    e, key = weight(N, K, wseed), (layout, glu)
    if key not in e:
        if layout == "row":
            ldw = K + 4
            buf = nanbuf(N * ldw)
            buf[torch.arange(N)[:, None] * ldw + torch.arange(K)[None, :]] = e["W"]
            e[key] = buf.to(DEV)
        else:
            e[key] = hip.pack_skinny_w(e["W"].to(DEV), glu=glu, bf16=layout == "bf16").data
    return e[key]


def rows_buf(vals, ld, lead, tail, dtype=torch.float32):
    Bn, n = vals.shape
    buf = nanbuf(lead + Bn * ld + tail, dtype)
    buf[lead + torch.arange(Bn)[:, None] * ld + torch.arange(n)[None, :]] = vals.to(dtype)
    return buf


def make(B, N, K, *, layout="row", epi=NONE, scale=False, inplace=False, bias=True, np_=0, rms=False, eps=1e-6, ksplit=0, aux=None,
         glu=None, seed=0, wseed=0, special=False, cancel=False, apart=False, odd=True):
    """One valid problem with slack everywhere.  aux: dict(tiles, flags, bias); glu: dict(ksize, dil, step, extra, bf16, zero).
    `full`: name -> (flat CPU buffer, elements in front of the operand); `p`: the scalar arguments."""
    g = gen(seed * 7919 + B * 31 + N * 17 + K)
    isglu = glu is not None
    n_out = N // 2 if isglu else N
    p = dict(B=B, N=N, K=K, epilogue=GLU_DW if isglu else epi, np_=np_, rms_norm=bool(rms), eps=eps, ksplit=ksplit,
             w_layout=LAYOUTS.index(layout))
    full = {}
    # ---- X (+ Xp: the product's layout is one buffer of four slices, X = slice 0)
    ldx = K + 8
    parts = torch.randn(4 if np_ else 1, B, K, generator=g)
    if cancel:  # large parts that cancel to small rows: the fixed order and the norm statistic matter
        parts[1:] *= 50.0
        parts[3] = -(parts[1] + parts[2]) + 0.01 * torch.randn(B, K, generator=g)
    if special:  # a zero row, a 1e-12 row and a 1e12 row beside ordinary ones
        for r, f in ((0, 0.0), (1, 1e-12), (2, 1e12)):
            if r < B:
                parts[:, r] *= f
    xps = up(B * ldx + 12, 4)
    lead_x = ldx
    if np_ and apart:
        full["X"] = (rows_buf(parts[0], ldx, lead_x, ldx), lead_x)
        xp = nanbuf(lead_x + 3 * xps + ldx)
        for s in range(3):
            xp[lead_x + s * xps + torch.arange(B)[:, None] * ldx + torch.arange(K)[None, :]] = parts[s + 1]
        full["Xp"] = (xp, lead_x)
    else:
        xb = nanbuf(lead_x + parts.shape[0] * xps + ldx)
        for s in range(parts.shape[0]):
            xb[lead_x + s * xps + torch.arange(B)[:, None] * ldx + torch.arange(K)[None, :]] = parts[s]
        full["X"] = (xb, lead_x)
    p.update(ldx=ldx, xp_stride=xps if np_ else 0)
    p["ldw"] = K + 4 if layout == "row" else K
    # ---- bias / scale
    if bias:
        full["bias"] = (torch.cat([torch.randn(N, generator=g), nanbuf(5)]), 0)
    if scale:
        full["scale"] = (torch.cat([torch.randn(N, generator=g), nanbuf(5)]), 0)
    # ---- Y / R
    nsl = K // 384 if (ksplit and K > 384) else 1
    ldy = n_out + (3 if odd else 4)
    yps = B * ldy + 11
    lead_y = 2 * ldy + 1
    ybuf = nanbuf(lead_y + (nsl - 1) * yps + B * ldy + 2 * ldy)
    p.update(ldy=ldy, y_part_stride=yps if nsl > 1 else 0)
    if epi == RES and not isglu:
        Rv = torch.randn(B, N, generator=g)
        if inplace:
            ybuf[lead_y + torch.arange(B)[:, None] * ldy + torch.arange(N)[None, :]] = Rv
            p["ldr"] = ldy
        else:
            ldr = N + 6
            full["R"] = (rows_buf(Rv, ldr, 3, ldr), 3)
            p["ldr"] = ldr
    full["Y"] = (ybuf, lead_y)
    # ---- aux set
    if aux:
        Na = 16 * aux["tiles"]
        aepi = NONE if aux["flags"] & 2 else epi
        ldya, ldra = Na + 7, Na + 2
        ypa = B * ldya + 5
        full["aux_Y"] = (nanbuf(2 * ldya + (nsl - 1) * ypa + B * ldya + 2 * ldya), 2 * ldya)
        if aux.get("bias", True):
            full["aux_bias"] = (torch.cat([torch.randn(Na, generator=g), nanbuf(3)]), 0)
        if aepi == RES:
            full["aux_R"] = (rows_buf(torch.randn(B, Na, generator=g), ldra, 5, ldra), 5)
        p.update(aux_tiles=aux["tiles"], aux_flags=aux["flags"], aux_ldy=ldya, aux_ldr=ldra, aux_y_part_stride=ypa if nsl > 1 else 0)
    # ---- GLU tail
    if isglu:
        ks, dil, bcap = glu["ksize"], glu["dil"], B + glu.get("extra", 0)
        L = (ks - 1) * dil + 1
        rdt = torch.bfloat16 if glu.get("bf16") else torch.float32
        ring = torch.zeros(L, bcap, D) if glu.get("zero") else torch.randn(L, bcap, D, generator=g)
        ring[:, B:] = NAN
        lead_r = 2 * D
        full["ring"] = (torch.cat([nanbuf(lead_r, rdt), ring.reshape(-1).to(rdt), nanbuf(2 * D, rdt)]), lead_r)
        full["dw_w"] = (torch.cat([torch.randn(ks * D, generator=g), nanbuf(7)]), 0)
        full["dw_b"] = (torch.cat([torch.randn(D, generator=g), nanbuf(7)]), 0)
        p.update(ring_len=L, ring_bcap=bcap, dil=dil, ksize=ks, ring_format=1 if glu.get("bf16") else 0, step=glu["step"])
    return dict(p=p, full=full, layout=layout, wseed=wseed, inplace=inplace, aux_wseed=wseed + 50)


def view(case, name, extra=0):
    if name not in case["full"]:
        return None
    buf, lead = case["full"][name]
    return buf[lead + extra:]


def reference(case):
    p = dict(case["p"])
    N, K = p["N"], p["K"]
    kw = {k: p[k] for k in ("B", "N", "K", "ldx", "ldy", "epilogue", "np_", "xp_stride", "ksplit", "y_part_stride", "rms_norm", "eps", "w_layout")}
    kw["ldr"] = p.get("ldr")
    Y = view(case, "Y")
    R = Y if case["inplace"] else view(case, "R")
    Xp = view(case, "Xp") if "Xp" in case["full"] else (view(case, "X", p["xp_stride"]) if p["np_"] else None)
    if p.get("aux_tiles"):
        kw.update(aux_W=weight(16 * p["aux_tiles"], K, case["aux_wseed"])["W"], aux_tiles=p["aux_tiles"], aux_flags=p["aux_flags"],
                  aux_bias=view(case, "aux_bias"), aux_R=view(case, "aux_R"), aux_Y=view(case, "aux_Y"), aux_ldy=p["aux_ldy"],
                  aux_ldr=p["aux_ldr"], aux_y_part_stride=p["aux_y_part_stride"])
    if p["epilogue"] == GLU_DW:
        kw.update(ring=view(case, "ring"), dw_w=view(case, "dw_w"), dw_b=view(case, "dw_b"),
                  **{k: p[k] for k in ("step", "ring_len", "ring_bcap", "dil", "ksize", "ring_format")})
    return S.skinny_ref(view(case, "X"), weight(N, K, case["wseed"])["W"], Y, bias=view(case, "bias"), R=R, scale=view(case, "scale"), Xp=Xp, **kw)


def launch(case, mt=1, nt=1, tweak=None, dev=None):
    """Every operand to the device, sopro_skinny_args filled directly, the launch, the output buffers back.  -> (rc, buffers)"""
    p = case["p"]
    d = dev if dev is not None else {k: v[0].to(DEV) for k, v in case["full"].items()}

    def at(name, extra=0):
        if name not in d:
            return None
        return d[name].data_ptr() + (case["full"][name][1] + extra) * d[name].element_size()

    isglu = p["epilogue"] == GLU_DW
    a = hip.SkinnyArgs()
    a.X, a.ldx = at("X"), p["ldx"]
    a.W, a.ldw = w_operand(p["N"], p["K"], case["wseed"], case["layout"], glu=isglu).data_ptr(), p["ldw"]
    a.bias, a.scale = at("bias"), at("scale")
    a.Y, a.ldy = at("Y"), p["ldy"]
    a.R, a.ldr = (at("Y") if case["inplace"] else at("R")), p.get("ldr", 0)
    if p["np_"]:
        a.Xp = at("Xp") if "Xp" in d else at("X", p["xp_stride"])
    a.xp_stride, a.y_part_stride, a.eps = p["xp_stride"], p["y_part_stride"], p["eps"]
    a.B, a.N, a.K, a.epilogue = p["B"], p["N"], p["K"], p["epilogue"]
    a.np, a.ksplit, a.rms_norm, a.w_layout = p["np_"], p["ksplit"], int(p["rms_norm"]), p["w_layout"]
    a.mt, a.nt = mt, nt
    if p.get("aux_tiles"):
        a.aux_W = w_operand(16 * p["aux_tiles"], p["K"], case["aux_wseed"], case["layout"]).data_ptr()
        a.aux_bias, a.aux_R, a.aux_Y = at("aux_bias"), at("aux_R"), at("aux_Y")
        a.aux_ldy, a.aux_ldr, a.aux_y_part_stride = p["aux_ldy"], p["aux_ldr"], p["aux_y_part_stride"]
        a.aux_tiles, a.aux_flags = p["aux_tiles"], p["aux_flags"]
    if isglu:
        step = torch.full((1,), p["step"], dtype=torch.int32, device=DEV)
        a.ring, a.dw_w, a.dw_b, a.step = at("ring"), at("dw_w"), at("dw_b"), step.data_ptr()
        a.ring_len, a.ring_bcap, a.dil, a.ksize, a.ring_format = p["ring_len"], p["ring_bcap"], p["dil"], p["ksize"], p["ring_format"]
    if tweak is not None:
        tweak(a)
    rc = hip.load().sopro_skinny_f32(C.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, {k: d[k].cpu() for k in ("Y", "aux_Y", "ring") if k in d}


# ------------------------------------------------------------------------------------------------ tolerances
def libm4(name, f32, f64, x):
    """4 x the error of torch's fp32 CPU evaluation against float64 on these arguments (the allowance for another libm), taken
    per ROW [B, 1]: a 1e12 row beside ordinary ones must not lend them its allowance.  `LIBM` records the rows below 1e3 only."""
    e = (f32(x.float()).double() - f64(x)).abs().amax(dim=1, keepdim=True)
    small = x.abs().amax(dim=1) < 1e3
    if bool(small.any()):
        LIBM[name] = max(LIBM.get(name, 0.0), float(e[small].max()))
    return 4.0 * e


def pre_bound(o):
    c = max(384, 96 * o.nslices + 3)
    d = c * U * o.pmag + U * o.bmag[None, :]
    if o.normed:
        d = d + (384 * 2.0 ** -25 + 4 * U) * (o.pmag + o.bmag[None, :])
    return d


def bounds(ref):
    """stream name -> tolerance tensor (module docstring)."""
    tol = {}
    if ref.glu is not None:
        o, q = ref["Y"], ref.glu
        d = pre_bound(o)
        v, gt, h = q["v"], q["g"], q["h"]
        sg = torch.sigmoid(gt)
        dh = sg * d[:, :D] + v.abs() * d[:, D:] / 4 + v.abs() * libm4("expf sigmoid", torch.sigmoid, torch.sigmoid, gt) + U * h.abs()
        dy = q["tapw"][:, -1].abs()[None, :] * dh + 14 * U * ((q["taps"].abs() * q["tapw"].abs()[None]).sum(dim=2) + q["dw_b"].abs()[None, :])
        tol["Y"] = dy + U * o.ref.abs()
        tol["ring"] = dh
        return tol
    for o in ref.outs:
        d = pre_bound(o)
        if o.epi == GELU:
            e = 1.13 * d + libm4("erff gelu", torch.nn.functional.gelu, G.gelu64, o.pre)
        elif o.epi == TANH:
            e = d + libm4("tanhf", torch.tanh, torch.tanh, o.pre)
        elif o.epi == RES:
            e = o.scale.abs()[None, :] * d + U * (o.scale[None, :] * o.pre).abs()
        else:
            e = d
        tol[o.name] = e + U * o.ref.abs()
    return tol


def bf16_ulp(x):
    _, e = torch.frexp(G.bf16_round(x))
    return torch.ldexp(torch.ones_like(x), e - 8)


def note(group, worst, what):
    COUNT["streams"] += 1
    if worst > WORST.get(group, (0.0, ""))[0]:
        WORST[group] = (worst, what)


def check(case, ref, got, group, what):
    """Canaries bit for bit (guards in front included), nothing owned left NaN, every value stream inside its bound."""
    tol = bounds(ref)
    for target, rbuf in ref.bufs.items():
        full, lead = case["full"][target]
        iv = torch.int16 if full.dtype == torch.bfloat16 else torch.int32
        g = got[target]
        assert torch.equal(g[:lead].view(iv), full[:lead].view(iv)), f"{group} {what}: {target}: the guard in front was written"
        gb, rb, own = g[lead:].view(iv), rbuf.view(iv), ref.owned(target)
        assert torch.equal(gb[~own], rb[~own]), f"{group} {what}: {target}: words outside the output were written ({int((gb[~own] != rb[~own]).sum())})"
    for o in ref.outs:
        val = o.values(got[o.target][case["full"][o.target][1]:])
        assert bool(torch.isfinite(val).all()), f"{group} {what}: {o.name}: {int((~torch.isfinite(val)).sum())} owned values are not finite"
        t = tol[o.name]
        if o.kind == "bf16":  # the written ring slot: bf16(h_ref), or its neighbour only next to a rounding boundary
            want = G.bf16_round(o.ref)
            charge = G.bf16_flip_charge(o.ref, t)
            flagged = charge > 0
            cap = 10.0 * float((2 * t / bf16_ulp(o.ref)).mean()) * val.numel()
            assert int(flagged.sum()) <= cap, f"{group} {what}: {int(flagged.sum())} ring words sit at a rounding boundary, cap {cap:.1f}"
            used = val != want
            NEIGH["words"] += val.numel()
            NEIGH["flagged"] += int(flagged.sum())
            NEIGH["used"] += int(used.sum())
            NEIGH["worst_share_of_cap"] = max(NEIGH["worst_share_of_cap"], int(flagged.sum()) / cap)
            # another value than bf16(h_ref) must be the rounding of SOME number within delta_h of h_ref: h_ref lies within delta_h of
            # the interval that rounds to it.  Where delta_h is below the spacing that is the neighbour at a flagged boundary and
            # nothing else; where |h| is so small that delta_h exceeds the spacing (h = v sigmoid(g) with v near 0) it may be further.
            m, e = torch.frexp(val)
            half = torch.ldexp(torch.ones_like(val), e - 9)
            half = torch.where((o.ref.abs() < val.abs()) & (m.abs() == 0.5), half / 2, half)   # below a power of two the spacing halves
            half = torch.where(val == 0, torch.zeros_like(half), half)
            reach = (val - o.ref).abs() <= half + t + U * o.ref.abs()
            bad = used & ~(reach & flagged)
            assert not bool(bad.any()), f"{group} {what}: ring: {int(bad.sum())} words are not bf16(h) (nor its neighbour at a boundary)"
            note(group + " bf16 ring", float(used.sum()) / max(1.0, float(flagged.sum())), f"{what} (neighbours used / allowed)")
            continue
        ratio = (val - o.ref).abs() / t.clamp_min(1e-300)  # (a zero row without a bias: the bound is 0 and the result exact)
        worst = float(ratio.max())
        note(group, worst, f"{what} {o.name}")
        print(f"SKINNY-EDGE {group} {what} {o.name}: worst error / tolerance {worst:.3f}")
        assert worst <= 1.0, f"{group} {what}: {o.name}: error / tolerance {worst:.3f} at {tuple(int(i) for i in (ratio == ratio.max()).nonzero()[0])}"


def whole(case, group, what, **kw):
    ref = reference(case)
    rc, got = launch(case, **kw)
    assert rc == 0, f"{group} {what}: refused ({rc}): {hip.load().sopro_last_error().decode()}"
    check(case, ref, got, group, what)
    return ref, got


def same_bits(a, b, what):
    for k in a:
        iv = torch.int16 if a[k].dtype == torch.bfloat16 else torch.int32
        x, y = a[k].view(iv), b[k].view(iv)
        assert torch.equal(x, y), f"{what}: {k} differs in {int((x != y).sum())} words"


def same_owned(ca, ra, ga, cb, rb, gb, pairs, what):
    """The owned values of two launches with different buffers: equal bit for bit.  pairs: (stream of a, stream of b)."""
    for na, nb in pairs:
        oa, ob = ra[na], rb[nb]
        va = oa.values(ga[oa.target][ca["full"][oa.target][1]:])
        vb = ob.values(gb[ob.target][cb["full"][ob.target][1]:])
        assert torch.equal(va, vb), f"{what}: {na} / {nb} differ at {int((va != vb).sum())} elements"


# ------------------------------------------------------------------------------------------------ 1. plain form, rows and columns
BS = (1, 15, 16, 17, 31, 32, 33, 48, 49)
NS = (1, 15, 16, 17, 31, 33, 48, 49)
CROSS = sorted({(b, 33) for b in BS} | {(17, n) for n in NS} | {(1, 1), (49, 49), (33, 15), (31, 31), (16, 16), (48, 48), (49, 97)})
EPIS = {"none": dict(), "gelu": dict(epi=GELU), "tanh": dict(epi=TANH), "res": dict(epi=RES), "res_scale": dict(epi=RES, scale=True),
        "res_inplace": dict(epi=RES, inplace=True), "res_scale_inplace": dict(epi=RES, scale=True, inplace=True)}


@pytest.mark.parametrize("B,N", CROSS)
def test_plain_form_rows_columns_epilogues_and_layouts(B, N):
    for li, layout in enumerate(LAYOUTS):
        for ei, (name, kw) in enumerate(EPIS.items()):
            case = make(B, N, 384, layout=layout, seed=ei, odd=(ei + li) % 2 == 0, **kw)
            whole(case, "1 plain", f"{layout} {name} {B}x{N}")


def test_plain_form_without_a_bias():
    for layout in LAYOUTS:
        whole(make(17, 33, 384, layout=layout, bias=False), "1 plain", f"{layout} no bias")
        whole(make(17, 33, 384, layout=layout, bias=False, epi=RES, scale=True), "1 plain", f"{layout} no bias, res")


# ------------------------------------------------------------------------------------------------ 2. K-slices
@pytest.mark.parametrize("K", [768, 1152, 1536])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_k_slices_in_one_workgroup_and_over_the_grid(K, layout):
    for B, N in ((17, 33), (33, 49), (1, 97), (49, 16)):
        for name, kw in (("none", dict()), ("gelu", dict(epi=GELU)), ("tanh", dict(epi=TANH)), ("res_scale", dict(epi=RES, scale=True)), ("res_inplace", dict(epi=RES, inplace=True))):
            whole(make(B, N, K, layout=layout, **kw), "2 K-slices", f"{layout} ksplit 0 {name} {B}x{N}x{K}")
        for name, kw in (("none", dict(bias=False)), ("res", dict(epi=RES)), ("res_inplace", dict(epi=RES, inplace=True)), ("res no bias", dict(epi=RES, bias=False))):
            ref, _ = whole(make(B, N, K, layout=layout, ksplit=1, **kw), "2 K-slices", f"{layout} ksplit 1 {name} {B}x{N}x{K}")
            assert len(ref.outs) == K // 384


@pytest.mark.parametrize("layout", LAYOUTS)
def test_ksplit_at_one_slice_is_the_unsplit_launch(layout):
    for kw in (dict(), dict(epi=GELU), dict(epi=RES, scale=True), dict(rms=True, np_=3)):
        c0, c1 = make(33, 49, 384, layout=layout, **kw), make(33, 49, 384, layout=layout, ksplit=1, **kw)
        _, g0 = whole(c0, "2 K-slices", f"{layout} K 384 ksplit 0")
        _, g1 = whole(c1, "2 K-slices", f"{layout} K 384 ksplit 1")
        same_bits(g0, g1, f"ksplit 1 at K = 384 ({layout})")


# ------------------------------------------------------------------------------------------------ 3. partial-sum input
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rms", [False, True])
def test_partial_sum_input(layout, rms):
    for B, N in ((1, 17), (17, 33), (33, 31), (49, 97)):
        for ci, kw in enumerate((dict(), dict(cancel=True), dict(apart=True), dict(cancel=True, epi=GELU))):
            whole(make(B, N, 384, layout=layout, np_=3, rms=rms, seed=ci, **kw), "3 partial sums", f"{layout} rms {rms} {B}x{N} {kw}")
        if not rms:
            for ksplit in (0, 1):
                whole(make(B, N, 1536, layout=layout, np_=3, ksplit=ksplit, epi=RES, cancel=ksplit == 1), "3 partial sums", f"{layout} K 1536 ksplit {ksplit} {B}x{N}")


# ------------------------------------------------------------------------------------------------ 4. RMSNorm row scale
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("eps", [1e-6, 1e-5])
def test_rmsnorm_row_scale_on_zero_tiny_and_huge_rows(layout, eps):
    for B, N in ((3, 17), (17, 33), (33, 49)):
        for name, kw in EPIS.items():
            ref, _ = whole(make(B, N, 384, layout=layout, rms=True, eps=eps, special=True, **kw), "4 row scale", f"{layout} eps {eps} {name} {B}x{N}")
        assert abs(float(ref.rs[0]) * float(torch.tensor(eps, dtype=torch.float32)) ** 0.5 - 1.0) < 1e-6  # the zero row: rs = rsqrt(eps)
        # without a bias the 1e-12 row's output is its row scale times O(1e-12) and nothing else: eps itself is on trial (beside a
        # bias of O(1) a wrong eps would hide in U |bias|, and on ordinary rows 1e-5 against 1e-6 moves rs by 4.5e-6 < 384 U)
        for kw in (dict(), dict(epi=GELU)):
            whole(make(B, N, 384, layout=layout, rms=True, eps=eps, special=True, bias=False, **kw), "4 row scale", f"{layout} eps {eps} no bias {B}x{N}")
        whole(make(B, N, 384, layout=layout, rms=True, eps=eps, special=True, np_=3), "4 row scale", f"{layout} eps {eps} np 3 {B}x{N}")
    if layout != "row":
        for flags in range(4):
            whole(make(33, 32, 384, layout=layout, rms=True, eps=eps, special=True, epi=GELU, aux=dict(tiles=2, flags=flags)),
                  "4 row scale", f"{layout} eps {eps} aux flags {flags}")


# ------------------------------------------------------------------------------------------------ 5. GLU tail and ring
KD = ((13, 1), (13, 2), (13, 4), (13, 8), (12, 3), (7, 5), (3, 2), (2, 1), (1, 1), (1, 3))
GB = (1, 15, 17, 33)


def steps_of(L):
    return (0, 1, max(L - 2, 0), L - 1, L, L + 1, 2 * L - 1, 1_000_003)


@pytest.mark.parametrize("ksize,dil", KD)
@pytest.mark.parametrize("ring", ["f32", "bf16"])
def test_glu_tail_one_frame_at_a_time(ksize, dil, ring):
    """Each frame is judged alone: the reference is given the ring as it was before the launch.  (1, 3): ksize 1 ignores dil.)"""
    L = (ksize - 1) * dil + 1
    ki = KD.index((ksize, dil))
    for i, step in enumerate(steps_of(L)):
        B, extra, np_ = GB[(i + ki) % 4], (0, 3)[(i // 2 + ki) % 2], (0, 3)[(i + ki // 2) % 2]
        layout = "bf16" if ring == "bf16" else LAYOUTS[(i + ki) % 3]
        case = make(B, 768, 384, layout=layout, rms=True, np_=np_, seed=i, cancel=np_ == 3 and i % 4 == 1,
                    glu=dict(ksize=ksize, dil=dil, step=step, extra=extra, bf16=ring == "bf16"))
        whole(case, "5 GLU tail", f"{layout} ring {ring} ksize {ksize} dil {dil} step {step} B {B} bcap +{extra} np {np_}")


@pytest.mark.parametrize("B", GB)
def test_glu_tail_every_batch_size_capacity_and_input_form(B):
    for extra in (0, 3):
        for np_ in (0, 3):
            for ring, layout in (("f32", "row"), ("f32", "packed"), ("f32", "bf16"), ("bf16", "bf16")):
                case = make(B, 768, 384, layout=layout, rms=True, np_=np_, glu=dict(ksize=7, dil=5, step=61, extra=extra, bf16=ring == "bf16"))
                whole(case, "5 GLU tail", f"{layout} ring {ring} B {B} bcap +{extra} np {np_}")


@pytest.mark.parametrize("ksize,dil", [(13, 1), (3, 2), (7, 5)])
def test_glu_tail_chained_frames_through_two_wraps(ksize, dil):
    """From a zero ring, 3 L + 2 frames; `step` is written by the test each frame.  Y of every frame against the float64 dilated
    causal convolution of the whole h sequence: the check of the slot arithmetic through two wraps."""
    B, L = 17, (ksize - 1) * dil + 1
    T = 3 * L + 2
    case = make(B, 768, 384, layout="packed", rms=True, glu=dict(ksize=ksize, dil=dil, step=0, extra=3, zero=True))
    p, full = case["p"], case["full"]
    dev = {k: v[0].to(DEV) for k, v in full.items()}
    xs = torch.randn(T, B, 384, generator=gen(ksize * 100 + dil))
    lead, ldx = full["X"][1], p["ldx"]
    xi = lead + torch.arange(B)[:, None] * ldx + torch.arange(384)[None, :]
    hs, dhs, worst = [], [], 0.0
    wt = view(case, "dw_w")[: ksize * D].double().reshape(ksize, D)
    dwb = view(case, "dw_b")[:D].double()
    zero_ring = full["ring"][0].clone()
    for t in range(T):
        full["X"][0][xi] = xs[t]
        dev["X"].copy_(full["X"][0])
        p["step"] = t
        full["ring"] = (zero_ring, full["ring"][1])   # the reference of one frame only supplies h and its bound
        ref = reference(case)
        hs.append(ref.glu["h"])
        dhs.append(bounds(ref)["ring"])
        rc, got = launch(case, dev=dev)
        assert rc == 0
        y, dy = dwb[None, :].repeat(B, 1), torch.zeros(B, D, dtype=torch.float64)
        mag = dwb.abs()[None, :].repeat(B, 1)
        for j in range(ksize):
            tt = t - (ksize - 1 - j) * dil
            if tt >= 0:
                y += wt[j] * hs[tt]
                mag += wt[j].abs() * hs[tt].abs()
                dy += wt[j].abs() * dhs[tt]
        want = xs[t].double() + y
        tol = dy + 14 * U * mag + U * want.abs()
        o = ref["Y"]
        val = o.values(got["Y"][full["Y"][1]:])
        ratio = float(((val - want).abs() / tol).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"chained ksize {ksize} dil {dil}: frame {t}: error / tolerance {ratio:.3f}"
    note("5 GLU chained", worst, f"ksize {ksize} dil {dil}, {T} frames")
    # the ring at the end: slot s holds h of the last frame written there, rows >= B and the guards are still NaN
    ring = got["ring"][full["ring"][1]:][: L * p["ring_bcap"] * D].reshape(L, p["ring_bcap"], D)
    assert bool(torch.isnan(ring[:, B:]).all()) and bool(torch.isnan(got["ring"][: full["ring"][1]]).all()) and bool(torch.isnan(got["ring"][-2 * D:]).all())
    for s in range(L):
        t = max(tt for tt in range(T) if tt % L == s)
        assert bool(((ring[s, :B].double() - hs[t]).abs() <= dhs[t]).all()), f"ring slot {s}"


# ------------------------------------------------------------------------------------------------ 6. bit-equalities
SHAPES = ((1, 1), (1, 2), (2, 1), (2, 2))


def _edge_cases():
    out = []
    for B, N in ((17, 17), (31, 33), (33, 49), (49, 97), (1, 15)):
        out.append((f"plain {B}x{N}", dict(B=B, N=N, K=384, epi=GELU, rms=True)))
        out.append((f"K-slices {B}x{N}", dict(B=B, N=N, K=1536, epi=RES, ksplit=1)))
        out.append((f"walk {B}x{N}", dict(B=B, N=N, K=1152, epi=RES, scale=True)))
        out.append((f"np 3 {B}x{N}", dict(B=B, N=N, K=384, np_=3, rms=True, cancel=True)))
    for B in (1, 17, 31, 33):
        out.append((f"glu B {B}", dict(B=B, N=768, K=384, rms=True, np_=3, glu=dict(ksize=12, dil=3, step=40, extra=3))))
    return out


@pytest.mark.parametrize("what,kw", _edge_cases(), ids=[w for w, _ in _edge_cases()])
def test_workgroup_shapes_layouts_and_repeats_are_bit_identical(what, kw):
    base = None
    for layout in LAYOUTS:
        case = make(layout=layout, **kw)
        ref = reference(case)
        first = None
        for mt, nt in SHAPES:
            rc, got = launch(case, mt=mt, nt=nt)
            assert rc == 0
            if first is None:
                first = got
                check(case, ref, got, "6 bit-equal", f"{what} {layout}")
                for _ in range(2):  # three launches of one case
                    same_bits(first, launch(case)[1], f"{what} {layout}: repeated launch")
            else:
                same_bits(first, got, f"{what} {layout}: {mt} x {nt} against 1 x 1")
        if layout == "row":
            base = (case, ref, first)
        elif layout == "packed":  # the same function as row-major weights (other strides of W only)
            names = [(o.name, o.name) for o in ref.outs]
            same_owned(base[0], base[1], base[2], case, ref, first, names, f"{what}: row-major against packed weights")
        if layout == "bf16" and "glu" in kw:  # and the bf16 ring under every workgroup shape
            c16 = make(layout=layout, **dict(kw, glu=dict(kw["glu"], bf16=True)))
            g0 = launch(c16)[1]
            check(c16, reference(c16), g0, "6 bit-equal", f"{what} bf16 ring")
            for mt, nt in SHAPES[1:]:
                same_bits(g0, launch(c16, mt=mt, nt=nt)[1], f"{what} bf16 ring: {mt} x {nt} against 1 x 1")


# ------------------------------------------------------------------------------------------------ 7. aux tiles
def _own_launch(case, ref, got):
    """The aux set as a launch of its own: W = aux_W, N = 16 * aux_tiles, the effective epilogue / row scale."""
    p = case["p"]
    flags, Na = p["aux_flags"], 16 * p["aux_tiles"]
    epi = NONE if flags & 2 else p["epilogue"]
    own = make(p["B"], Na, p["K"], layout=case["layout"], epi=epi, bias="aux_bias" in case["full"], np_=p["np_"], ksplit=p["ksplit"],
               rms=p["rms_norm"] and not flags & 1, eps=p["eps"], wseed=case["aux_wseed"])
    own["full"]["X"] = case["full"]["X"]
    if "aux_bias" in case["full"]:
        own["full"]["bias"] = case["full"]["aux_bias"]
    if epi == RES:
        own["full"]["R"], own["p"]["ldr"] = case["full"]["aux_R"], p["aux_ldr"]
    r2, g2 = whole(own, "7 aux tiles", f"aux set alone flags {flags}")
    names = [(o.name, o.name.replace("aux", "Y")) for o in ref.outs if o.target == "aux_Y"]
    same_owned(case, ref, got, own, r2, g2, names, "aux tiles against a launch of their own")


@pytest.mark.parametrize("N", [32, 96])
@pytest.mark.parametrize("tiles", [2, 4])
@pytest.mark.parametrize("layout", ["packed", "bf16"])
def test_aux_tiles_ff1_and_ff2_forms(N, tiles, layout):
    for flags in range(4):
        for B in (17, 33):
            # FF1 form: norm + GELU on the main tiles; the aux tiles raw (flags 3), or with the row scale / GELU of the launch
            case = make(B, N, 384, layout=layout, rms=True, epi=GELU, aux=dict(tiles=tiles, flags=flags, bias=flags != 3))
            ref, got = whole(case, "7 aux tiles", f"{layout} FF1 {B}x{N} tiles {tiles} flags {flags}")
            plain = make(B, N, 384, layout=layout, rms=True, epi=GELU)
            rp, gp = whole(plain, "7 aux tiles", f"{layout} FF1 {B}x{N} without aux")
            same_bits({"Y": got["Y"]}, {"Y": gp["Y"]}, "main tiles with and without aux tiles")
            _own_launch(case, ref, got)
            for mt, nt in SHAPES[1:]:
                same_bits(got, launch(case, mt=mt, nt=nt)[1], f"aux FF1 {mt} x {nt} against 1 x 1")
            # FF2 form: K-slices with aux_R, aux_bias and aux_y_part_stride (flags bit 1: raw slices, no bias, no residual)
            case = make(B, N, 1536, layout=layout, epi=RES, ksplit=1, aux=dict(tiles=tiles, flags=flags, bias=not flags & 2))
            ref, got = whole(case, "7 aux tiles", f"{layout} FF2 {B}x{N} tiles {tiles} flags {flags}")
            gp = whole(make(B, N, 1536, layout=layout, epi=RES, ksplit=1), "7 aux tiles", f"{layout} FF2 {B}x{N} without aux")[1]
            same_bits({"Y": got["Y"]}, {"Y": gp["Y"]}, "main K-slices with and without aux tiles")
            _own_launch(case, ref, got)
            for mt, nt in SHAPES[1:]:
                same_bits(got, launch(case, mt=mt, nt=nt)[1], f"aux FF2 {mt} x {nt} against 1 x 1")


# ------------------------------------------------------------------------------------------------ 8. packers
@pytest.mark.parametrize("K", [32, 64, 384])
@pytest.mark.parametrize("N,glu", [(1, 0), (15, 0), (16, 0), (17, 0), (33, 0), (8, 1), (16, 1), (18, 1), (40, 1)])
def test_packers_word_for_word(N, K, glu):
    lib, st = hip.load(), torch.cuda.current_stream().cuda_stream
    ldw = K + 8
    W = torch.randn(N, K, generator=gen(N * 1000 + K + glu))
    Wb = nanbuf(N * ldw + 4)
    Wb[torch.arange(N)[:, None] * ldw + torch.arange(K)[None, :]] = W
    n = int(lib.sopro_skinny_packed_floats(N, K, glu))
    assert n == S.skinny_packed_floats(N, K, bool(glu))
    Wd = Wb.to(DEV)
    out = nanbuf(n + 64).to(DEV)
    assert lib.sopro_pack_skinny_w(Wd.data_ptr(), ldw, N, K, glu, out.data_ptr(), st) == 0
    out16 = torch.full((n // 2 + 32,), -7, dtype=torch.int32, device=DEV)
    assert lib.sopro_pack_skinny_w_bf16(Wd.data_ptr(), ldw, N, K, glu, out16.data_ptr(), st) == 0
    torch.cuda.synchronize()
    want = torch.cat([S.pack_skinny_ref(Wb, ldw, N, K, bool(glu), False), nanbuf(64)])
    assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32))
    want16 = torch.cat([S.pack_skinny_ref(Wb, ldw, N, K, bool(glu), True).view(torch.int16), torch.full((32,), -7, dtype=torch.int32).view(torch.int16)])
    assert torch.equal(out16.cpu().view(torch.int16), want16)


# ------------------------------------------------------------------------------------------------ 9. refusals
def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _glu_case(**g):
    return make(17, 768, 384, layout=g.pop("layout", "packed"), rms=True, glu=dict(dict(ksize=7, dil=5, step=3, extra=3), **g))


REFUSALS = [
    ("K not a multiple of 384", lambda: make(17, 33, 768), _set(K=400)),
    ("rms_norm with K = 768", lambda: make(17, 33, 768), _set(rms_norm=1)),
    ("EPI_GLU", lambda: make(17, 34, 384), _set(epilogue=S.EPI_GLU)),
    ("np = 1", lambda: make(17, 33, 384, np_=3), _set(np=1)),
    ("np = 3 without Xp", lambda: make(17, 33, 384, np_=3), _set(Xp=None)),
    ("ksplit = 2", lambda: make(17, 33, 768, ksplit=1, bias=False), _set(ksplit=2)),
    ("K-split with GELU", lambda: make(17, 33, 768, ksplit=1, bias=False), _set(epilogue=GELU)),
    ("K-split with TANH", lambda: make(17, 33, 768, ksplit=1, bias=False), _set(epilogue=TANH)),
    ("mt = 3", lambda: make(17, 33, 384), _set(mt=3)),
    ("nt = 3", lambda: make(17, 33, 384), _set(nt=3)),
    ("GLU tail: wrong ring_len", lambda: _glu_case(), _set(ring_len=32)),
    ("GLU tail: ksize 14", lambda: _glu_case(), _set(ksize=14, ring_len=66)),
    ("GLU tail: ring_bcap < B", lambda: _glu_case(), _set(ring_bcap=16)),
    ("GLU tail: no rms_norm", lambda: _glu_case(), _set(rms_norm=0)),
    ("GLU tail: ring_format 1 on fp32 weights", lambda: _glu_case(), _set(ring_format=1)),
    ("odd aux_tiles", lambda: make(17, 32, 384, layout="packed", aux=dict(tiles=2, flags=3)), _set(aux_tiles=1)),
    ("aux on row-major weights", lambda: make(17, 32, 384, layout="packed", aux=dict(tiles=2, flags=3)), _set(w_layout=0)),
    ("aux with N % 32 != 0", lambda: make(17, 48, 384, layout="packed", aux=dict(tiles=2, flags=3)), None),
    ("X off 16 bytes", lambda: make(17, 33, 384), lambda a: setattr(a, "X", a.X + 4)),
    ("ldx % 4 != 0", lambda: make(17, 33, 384), _set(ldx=394)),
    # the contract holes closed with this file (include/sopro_hip.h): what the K-slices would not sum to
    ("K-split with scale", lambda: make(17, 33, 768, epi=RES, scale=True), _set(ksplit=1, y_part_stride=17 * 36 + 11)),
    ("K-split, EPI_NONE with a bias", lambda: make(17, 33, 768), _set(ksplit=1, y_part_stride=17 * 36 + 11)),
    ("K-split, aux epilogue NONE with aux_bias", lambda: make(17, 32, 768, layout="packed", epi=RES, ksplit=1, aux=dict(tiles=2, flags=2, bias=True)), None),
    ("aux tiles with scale", lambda: make(17, 32, 384, layout="packed", epi=RES, scale=True, aux=dict(tiles=4, flags=0)), None),
]


@pytest.mark.parametrize("what,mk,tweak", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_every_output_alone(what, mk, tweak):
    case = mk()
    rc, got = launch(case, tweak=tweak)
    assert rc != 0, f"{what}: accepted"
    assert hip.load().sopro_last_error()
    same_bits(got, {k: case["full"][k][0] for k in got}, f"{what}: refused, but written")


def test_packers_refuse():
    lib, st = hip.load(), torch.cuda.current_stream().cuda_stream
    W, out = torch.randn(34 * 72, generator=gen(1)).to(DEV), nanbuf(4096).to(DEV)
    for name in ("sopro_pack_skinny_w", "sopro_pack_skinny_w_bf16"):
        fn = getattr(lib, name)
        assert fn(W.data_ptr(), 72, 16, 48, 0, out.data_ptr(), st) != 0      # K % 32
        assert fn(W.data_ptr(), 64, 17, 64, 1, out.data_ptr(), st) != 0      # odd GLU N
        assert fn(W.data_ptr(), 60, 16, 64, 0, out.data_ptr(), st) != 0      # ldw < K
    assert lib.sopro_skinny_packed_floats(16, 48, 0) == 0 and lib.sopro_skinny_packed_floats(17, 64, 1) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def test_glu_tail_with_one_tap_ignores_the_dilation():
    """ksize 1: the ring is one slot.  The twelve dead taps still read ring words; with dil > 1 their slot arithmetic (one
    subtraction of ring_len per step) would walk them out of the ring - behind it lie NaN guards here, which a zero weight does
    not stop.  The entry point runs the one-slot ring with dil 1."""
    for ring, layout in (("f32", "row"), ("f32", "packed"), ("bf16", "bf16")):
        for dil in (2, 3, 8):
            for step in (0, 1, 7):
                whole(make(17, 768, 384, layout=layout, rms=True, glu=dict(ksize=1, dil=dil, step=step, extra=3, bf16=ring == "bf16")),
                      "5 GLU tail", f"{layout} ring {ring} ksize 1 dil {dil} step {step}")


# ------------------------------------------------------------------------------------------------ 10. seeded sweep
SWEEP_SEED = 20261


def _draw(rng, i):
    pick = lambda xs: xs[int(torch.randint(len(xs), (1,), generator=rng))]  # noqa: E731
    form = pick(("plain", "plain", "kslices", "np3", "glu", "aux"))
    layout = pick(LAYOUTS)
    B = pick(BS + (2, 7, 40))
    mt, nt = pick(SHAPES)
    if form == "glu":
        ks, dil = pick(KD)
        L = (ks - 1) * dil + 1
        bf = layout == "bf16" and pick((0, 1)) == 1
        kw = dict(B=min(B, 33), N=768, K=384, layout=layout, rms=True, np_=pick((0, 3)),
                  glu=dict(ksize=ks, dil=dil, step=pick(steps_of(L) + (5, 77, 2 ** 31 - 1)), extra=pick((0, 3)), bf16=bf))
    elif form == "aux":
        layout = pick(LAYOUTS[1:])
        ff2 = pick((0, 1))
        flags = pick((0, 1, 2, 3))
        kw = dict(B=B, N=pick((32, 64, 96)), layout=layout, aux=dict(tiles=pick((2, 4)), flags=flags, bias=not (flags & 2) or not ff2))
        kw.update(dict(K=pick((768, 1536)), epi=RES, ksplit=1) if ff2 else dict(K=384, rms=True, epi=pick((NONE, GELU, TANH, RES))))
    else:
        N = pick(NS + (2, 64, 97))
        K = 384 if form != "kslices" else pick((768, 1152, 1536))
        ksplit = pick((0, 1)) if K > 384 or form == "np3" else 0
        split = ksplit and K > 384
        ename = pick(("none", "res", "res_inplace") if split else tuple(EPIS))
        kw = dict(B=B, N=N, K=K, layout=layout, ksplit=ksplit, np_=3 if form == "np3" else pick((0, 0, 3)), **EPIS[ename])
        kw["bias"] = False if (split and ename == "none") else pick((True, True, False))
        kw["rms"] = K == 384 and pick((0, 1)) == 1
        kw["cancel"] = kw["np_"] == 3 and pick((0, 1)) == 1
        kw["special"] = kw["rms"] and pick((0, 0, 1)) == 1
        kw["eps"] = pick((1e-6, 1e-5))
    return dict(kw, seed=i, odd=pick((True, False))), mt, nt


def test_seeded_sweep():
    rng = gen(SWEEP_SEED)
    for i in range(150):
        kw, mt, nt = _draw(rng, i)
        what = f"seed {SWEEP_SEED} draw {i}: {mt} x {nt} " + " ".join(f"{k}={v}" for k, v in kw.items())
        whole(make(**kw), "10 sweep", what, mt=mt, nt=nt)


# ------------------------------------------------------------------------------------------------ the table
def test_zz_print_the_worst_ratios():
    print("\nSKINNY-EDGE value streams compared:", COUNT["streams"])
    for grp in sorted(WORST, key=lambda s: (int(s.split()[0]), s)):
        print(f"SKINNY-EDGE WORST {grp}: {WORST[grp][0]:.3f}  ({WORST[grp][1]})")
    for k, v in sorted(LIBM.items()):
        print(f"SKINNY-EDGE LIBM {k}: {v:.3e} (allowance 4 x)")
    print(f"SKINNY-EDGE bf16 ring: {NEIGH['words']} words written, {NEIGH['flagged']} within delta_h of a rounding boundary, "
          f"{NEIGH['used']} hold the neighbour; largest flagged count / cap {NEIGH['worst_share_of_cap']:.3f}")
