"""Edge tiles, strides, segments, K tails, tile walks and split-K of the tiled contractions against the float64 reference of
tests/gemm_ref.py: sopro_gemm_f32, sopro_gemm_bf16x3 / x6 / x1, sopro_gemm_f16x3 and the long-K form sopro_gemm_bf16x3_8p.

Every case has slack in every stride, NaN canaries in the output and residual buffers (-7 words in the arg-max pairs), guard rows
in front of the first and behind the last row, and NaN in the A-row slack and behind pro_vec / scale.  After a launch the WHOLE
buffer is compared with the reference's copy: words the operation does not own must be bit for bit what they were.

Tolerances (derived, never fitted to a kernel's output).  Pre-activation: delta = rel * (|pro(A)| |W|^T + |bias|) + 1e-6 with
rel = 2^-15 (bf16x3, long-K), 2^-21 (bf16x6), 2^-19 (f16x3) - `_split_bound` of tests/test_gpu_ops.py - and K * 2^-24 for
sopro_gemm_f32 (an fma chain of length K) and for bf16x1 against the product of the bf16-rounded operands.  Added where they apply:
the error eps_k of the kernel's fp32 evaluation of a staged element times |w_nk|, summed over k - eps_k = 2e-7 + 2 * 2^-24 |a| for
the ELU prologue on a <= 1e-6 (eluf_, csrc/common.h; on larger a it is the identity: 0) and 16 * 2^-24 (|a rstd| + |mean rstd|) for
the fused LayerNorm; PRO_ADDVEC adds nothing (the fp32 sum is the rounding of the exact sum).  For bf16x1 behind ELU / LayerNorm,
in addition one bf16 ulp of a_k times |w_nk| for exactly those k whose float64 value lies within eps_k of a bf16 rounding boundary
(gemm_ref.bf16_flip_charge): every other element is staged as the same bf16 number as the reference's.  (K 2^-25 + 4 * 2^-24) * mag
for the fused RMSNorm's row scale.  Through the epilogue by its Lipschitz constant: GELU 1.13, tanh / ELU 1, RES |scale|,
GLU sigmoid(g) delta_v + |v| delta_g / 4, ROPE |c| delta + |s| delta_partner; plus the function's own error - 4.7e-7 (gelu_fast) and
3 * 2^-23 relative (sigmoid_fast) as csrc/common.h states them, 2e-7 for eluf_, and for the library functions without a stated
figure (erff, tanhf, the precise sigmoid) 4 x the error of torch's fp32 CPU evaluation against float64 on the case's own
pre-activations - plus one rounding of every fp32 product / sum of the epilogue and of the result (2^-24 each), 2^-17 |ref| for a
split-form output and 2^-8 |ref| for bf16 rows.  Bit-equality claims (tile shapes, group_m, the long-K form, repeated launches,
vector against scalar stores, ksplit = 1) are exact.

Worst error / tolerance per group on an MI355X (first run, profiles/gemm_edges.md; every comparison feeds `WORST`, `pytest -s`
prints it):
    1 epilogues 0.996 (bf16x1 128-row tile, bf16 rows, RES) 2 segments 0.993 (bf16x1, bf16 rows, RES)
    3 K tail 0.991 (bf16x1, bf16 rows in and out, K = 4)    4 tile walk 0.295 (bf16x6, 9 x 5 tiles)
    5 split-K 0.200 (bf16x6, ksplit 1, K = 160)             6 special outputs 0.924 (bf16x1, ln_stats consumer, GELU)
    7 long-K form 0.215 (255 x 512 x 32, c_mode 2)          9 sweep 0.996 (bf16x1, bf16 rows, RES)
(group 8 compares nothing numerically).  The ratios at 0.99 are bf16-row outputs: half an ulp of a value at the low end of its
binade is 2^-8 of it, which is the whole bf16 term of the bound.  Measured fp32-libm errors behind the 4 x allowances: erff GELU
1.26e-6, expf sigmoid 9.2e-8, tanhf 5.4e-8.
"""
import ctypes as C
import math
from contextlib import contextmanager

import pytest
import torch

import gemm_ref as G
from sopro_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
U = 2.0 ** -24
NONE, GELU, GLU, RES, TANH, ROPE = G.EPI_NONE, G.EPI_GELU, G.EPI_GLU, G.EPI_RES, G.EPI_TANH, G.EPI_ROPE
P_NONE, P_ELU, P_ADD = G.PRO_NONE, G.PRO_ELU, G.PRO_ADDVEC
REL = {"x3": 2.0 ** -15, "8p": 2.0 ** -15, "x6": 2.0 ** -21, "f16": 2.0 ** -19}
TILES = {"f32": (0, 1, 2, 3, 4, 5), "x3": (0, 1, 2, 4, 5, 7), "x6": (0, 1, 4, 5), "f16": (0, 1, 4, 5), "x1": (0,), "8p": (0,)}
# ("every tile shape" below = every entry of TILES: bf16x1 and the long-K form have no override; bf16x1's second tile, 128 x 128, is
# chosen by shape alone and has its own test, test_one_pass_128_tile_is_reached_by_shape)
FAST = ("x3", "x1", "f16", "8p")  # gelu_fast / sigmoid_fast in the epilogue
WORST = {}   # group -> (error / tolerance, what)
LIBM = {}    # function -> largest measured fp32-vs-float64 error of torch's CPU evaluation (x 4 = the allowance)


def up(x, a):
    return -(-x // a) * a


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ operands
_weights = {}


def weight(entry, N, K, wseed=0, zero_tail=False, ints=False):
    """[N, K] weight on the CPU and as the entry point's operand; packed once per (entry, N, K, ...) for the module."""
    key = (entry if entry != "8p" else "x3", N, K, wseed, zero_tail, ints)
    if key not in _weights:
        g = gen(1000 + wseed + 7 * N + 13 * K)
        W = torch.randint(-2, 3, (N, K), generator=g).float() if ints else torch.randn(N, K, generator=g) * K ** -0.5
        if zero_tail:
            W[:, K - 4:] = 0.0
        Wd = W.to(DEV)
        op = {"f32": lambda: Wd, "x3": lambda: hip.pack_w_bf16x3(Wd, rows=K % 32 == 0), "x6": lambda: hip.pack_w_bf16x6(Wd),
              "x1": lambda: hip.pack_w_bf16x1(Wd), "f16": lambda: hip.pack_w_f16x3(Wd)}[key[0]]()
        _weights[key] = (W, op)
    return _weights[key]


def make(entry, M, N, K, *, epi=NONE, pro=P_NONE, c_mode=0, rps=None, lda=None, sa=4, sc=4, sr=8, s2=12, pads=(8, 12, 20, 24),
         c_mis=0, r_mis=0, scale=False, inplace=False, a_fmt=0, rope=None, ln=False, rms=False, ln_out=False, seed=0, wseed=0,
         big_tail=False, ints=False, bias=True, dense_seg=False):
    """One valid problem with slack everywhere.  sa / sc / sr / s2: extra elements per row of A / C / R / C2; pads: extra elements
    per segment; c_mis / r_mis: added to the C / R offsets (break the 16-byte alignment where the entry point takes that)."""
    g = gen(seed * 7919 + M * 31 + N * 17 + K)
    n_out = N // 2 if epi == GLU else N
    rps = M if rps is None else rps
    nseg = -(-M // rps)
    c16 = c_mode in (6, 7, 8)
    W, Wop = weight(entry, N, K, wseed, zero_tail=big_tail, ints=ints)
    kw = dict(M=M, N=N, K=K, epilogue=epi, prologue=pro, c_mode=c_mode, rows_per_seg=rps)
    # ---- A
    ua = 32 if a_fmt == 1 else 4
    lda = up(K + sa, ua) if lda is None else lda
    a_seg = 0 if dense_seg else up((rps - 1) * lda + K + pads[0], ua)
    a_off = up(lda, 32)
    An = a_off + nseg * (a_seg or rps * lda) + up(K, 32) + lda
    vals = torch.randint(-3, 4, (M, K), generator=g).float() if ints else torch.randn(M, K, generator=g)
    if big_tail:
        vals[::3, K - 4:] = 1e30
    if ln:
        vals = vals * 1.5 + 2.0  # a row mean that is not small against the deviations
    st = G.row_starts(M, rps, lda, a_seg, a_off)
    idx = st[:, None] + torch.arange(K)[None, :]
    if a_fmt == 1:
        A = torch.full((An,), NAN)
        A.view(torch.int32)[idx] = G.to_split_form(vals).view(torch.int32)
    elif a_fmt == 2:
        A = torch.full((An,), NAN, dtype=torch.bfloat16)
        A[idx] = vals.to(torch.bfloat16)
    else:
        A = torch.full((An,), NAN)
        A[idx] = vals
    kw.update(lda=lda, a_seg_stride=a_seg, a_off=a_off, a_split=a_fmt == 1)
    # ---- C / C2 / R
    cdt = torch.bfloat16 if c16 else torch.float32
    alc = 32 if c_mode == 1 else (4 if (c_mode in (3, 6, 7, 8) or epi == ROPE or ln_out) else 1)
    ldc = up(n_out + sc, alc)
    c_seg = 0 if dense_seg else up(rps * ldc + pads[1], alc)
    c_off = up(ldc, 32) + c_mis
    Cb = torch.full((c_off + nseg * (c_seg or rps * ldc) + ldc + 8,), NAN, dtype=cdt)
    kw.update(ldc=ldc, c_seg_stride=c_seg, c_off=c_off)
    C2 = None
    if c_mode in (2, 4, 8):
        al2 = 32 if c_mode == 2 else 4
        ldc2 = up(n_out + s2, al2)
        c2_seg = 0 if dense_seg else up(rps * ldc2 + pads[3], al2)
        c2_off = up(ldc2, 32)
        C2 = torch.full((c2_off + nseg * (c2_seg or rps * ldc2) + ldc2,), NAN, dtype=cdt)
        kw.update(ldc2=ldc2, c2_seg_stride=c2_seg, c2_off=c2_off)
    elif c_mode == 5:
        ldc2 = -(-N // 64) + 1
        C2 = torch.empty(4 + M * ldc2 * 2 + 6)
        C2.view(torch.int32).fill_(-7)
        kw.update(ldc2=ldc2, c2_off=4)
        Cb = None
    R = None
    if epi == RES:
        if inplace:
            R = Cb
            Cb.reshape(-1)[G.row_starts(M, rps, ldc, c_seg, c_off)[:, None] + torch.arange(N)[None, :]] = torch.randn(M, N, generator=g).to(cdt)
            kw.update(ldr=ldc, r_seg_stride=c_seg, r_off=c_off)
        else:
            alr = 4 if (c16 or ln_out) else 1
            ldr = up(N + sr, alr)
            r_seg = 0 if dense_seg else up(rps * ldr + pads[2], alr)
            r_off = up(ldr, 32) + r_mis
            R = torch.full((r_off + nseg * (r_seg or rps * ldr) + ldr + 8,), NAN, dtype=cdt)
            R[G.row_starts(M, rps, ldr, r_seg, r_off)[:, None] + torch.arange(N)[None, :]] = torch.randn(M, N, generator=g).to(cdt)
            kw.update(ldr=ldr, r_seg_stride=r_seg, r_off=r_off)
        if scale:
            kw["scale"] = torch.cat([torch.randn(N, generator=g), torch.full((5,), NAN)])
    if bias:
        kw["bias"] = torch.randint(-3, 4, (N,), generator=g).float() if ints else torch.randn(N, generator=g)
    if pro == P_ADD:
        kw["pro_vec"] = torch.cat([torch.randn(K, generator=g), torch.full((4,), NAN)])
    if rms:
        kw["rms_eps"] = 1e-6
    if ln:
        kw.update(ln_stats=G.row_stats64(vals).float().reshape(-1), ln_eps=1e-5)
    if ln_out:
        kw["ln_stats_out"] = torch.full((M * (N // 64) * 2 + 6,), NAN)
    if rope is not None:  # (columns, head dim, first position, rows per utterance)
        rcols, dh, pos0, rrps = rope
        ang = torch.rand(pos0 + min(M, rrps), dh // 2, generator=g) * 6.28
        kw["rope"] = (torch.cos(ang), torch.sin(ang), rcols, dh, pos0, rrps)
    return dict(entry=entry, A=A, W=W, Wop=Wop, C=Cb, C2=C2, R=R, inplace=inplace, kw=kw)


def reference(case):
    kw = dict(case["kw"])
    return G.gemm_ref(case["A"], case["W"], case["C"], R=case["R"], C2=case["C2"], round_operands=case["entry"] == "x1", **kw)


def run(case, **extra):
    """The launch: every operand to the device, hip.gemm, the output buffers back."""
    d = lambda t: None if t is None else t.to(DEV)
    kw = {k: (d(v) if isinstance(v, torch.Tensor) else v) for k, v in case["kw"].items()}
    if "rope" in kw:
        r = kw["rope"]
        kw["rope"] = (d(r[0]), d(r[1])) + tuple(r[2:])
    Cd, C2d = d(case["C"]), d(case["C2"])
    Rd = Cd if case["inplace"] else d(case["R"])
    if case["entry"] == "8p":
        extra = dict(extra, long_k=True)
    elif case["entry"] == "x3":
        extra = dict(dict(long_k=False), **extra)
    hip.gemm(d(case["A"]), case["Wop"], Cd, R=Rd, C2=C2d, **kw, **extra)
    torch.cuda.synchronize()
    got = {"C": None if Cd is None else Cd.cpu(), "C2": None if C2d is None else C2d.cpu()}
    if kw.get("ln_stats_out") is not None:
        got["ln_stats_out"] = kw["ln_stats_out"].cpu()
    return got


@contextmanager
def tile(entry, cfg):
    lib = hip.load()
    fn = lib.sopro_gemm_set_tile_override if entry == "f32" else lib.sopro_gemm_bf16_set_tile_override
    fn(int(cfg))
    try:
        yield
    finally:
        fn(0)


# ------------------------------------------------------------------------------------------------ tolerances
def libm4(name, f32, f64, x):
    """4 x the error of torch's fp32 CPU evaluation against float64 on these arguments (the allowance for another libm)."""
    e = float((f32(x.float()).double() - f64(x)).abs().max()) if x.numel() else 0.0
    LIBM[name] = max(LIBM.get(name, 0.0), e)
    return 4.0 * e


def bounds(case, ref):
    """name -> tolerance tensor of every value stream of the call (module docstring)."""
    entry, kw = case["entry"], case["kw"]
    K, N, epi, pro = kw["K"], kw["N"], kw["epilogue"], kw["prologue"]
    fast = entry in FAST
    d = (K * U if entry in ("f32", "x1") else REL[entry]) * ref.mag + 1e-6
    # the staged operand as the kernel's fp32 arithmetic evaluates it: absolute error per element (None: exact - no prologue, or
    # ADDVEC, whose fp32 sum is the rounding of the exact sum the reference forms)
    stage = None
    if pro == P_ELU:  # eluf_ is the identity on v > 0 (csrc/common.h: but for v < 6e-8); else exp(v) - 1 within 2e-7
        stage = torch.where(ref.a_pre <= 1e-6, 2e-7 + 2 * U * ref.a_pre.abs(), torch.zeros_like(ref.a_pre))
    elif ref.ln_terms is not None:  # mean and rstd from K / 64 pairs, rsqrt, one fused multiply-add: 16 roundings of the two terms
        stage = 16 * U * ref.ln_terms
    if stage is not None:
        d = d + stage @ ref.w_eff.abs().t()
        if entry == "x1":  # only the elements that sit within that error of a bf16 rounding boundary may round the other way
            d = d + G.bf16_flip_charge(ref.a_pre, stage) @ ref.w_eff.abs().t()
    if kw.get("rms_eps", 0.0) > 0.0:
        d = d + (K * 2.0 ** -25 + 4 * U) * ref.mag
    pre, out = ref.pre, ref.out
    if epi == GELU:
        e = 1.13 * d + (4.7e-7 if fast else libm4("erff gelu", torch.nn.functional.gelu, G.gelu64, pre))
    elif epi == TANH:
        e = d + libm4("tanhf", torch.tanh, torch.tanh, pre)
    elif epi == RES:
        e = ref.scale.abs()[None, :] * d + U * (ref.scale[None, :] * pre).abs()
    elif epi == GLU:
        M = pre.shape[0]
        g4, d4 = pre.reshape(M, N // 64, 2, 32), d.reshape(M, N // 64, 2, 32)
        v, gt, sg = g4[:, :, 0], g4[:, :, 1], torch.sigmoid(g4[:, :, 1])
        fn = 3 * 2.0 ** -23 * sg if fast else libm4("expf sigmoid", torch.sigmoid, torch.sigmoid, gt)
        e = (sg * d4[:, :, 0] + v.abs() * d4[:, :, 1] / 4 + v.abs() * fn + U * (v * sg).abs()).reshape(M, N // 2)
    elif epi == ROPE:
        c, s, partner = ref.rope_cs
        rc = c.shape[1]
        e = d.clone()
        e[:, :rc] = c.abs() * d[:, :rc] + s.abs() * d[:, partner] + U * ((pre[:, :rc] * c).abs() + (pre[:, partner] * s).abs())
    else:
        e = d
    e = e + U * out.abs()
    tol = {}
    for o in ref.outs:
        if o.role == "raw":
            t = e
        elif o.role == "act":
            t = e + 2e-7 + U * o.ref.abs()
        else:
            continue
        if o.kind == "split":
            t = t + 2.0 ** -17 * o.ref.abs()
        elif o.kind == "bf16":
            t = t + 2.0 ** -8 * o.ref.abs()
        tol[o.name] = t
    return tol


def check(case, ref, got, group, what):
    """Canaries bit for bit, nothing owned left NaN, every value stream inside its bound; exact streams (arg-max pairs) bit for bit."""
    tol = bounds(case, ref)
    for o in ref.outs:
        gb, rb, own = o.bits(got[o.name]), o.bits(o.buf), o.owned()
        assert torch.equal(gb[~own], rb[~own]), f"{group} {what}: {o.name}: words outside the output were written ({int((gb[~own] != rb[~own]).sum())})"
        if o.role == "argmax":
            assert torch.equal(gb, rb), f"{group} {what}: arg-max pairs differ at {int((gb != rb).sum())} words"
            continue
        val = o.values(got[o.name])
        assert bool(torch.isfinite(val).all()), f"{group} {what}: {o.name}: {int((~torch.isfinite(val)).sum())} owned values are not finite"
        if o.role == "stats":
            continue
        ratio = (val - o.ref).abs() / tol[o.name]
        worst = float(ratio.max())
        if worst > WORST.get(group, (0.0, ""))[0]:
            WORST[group] = (worst, f"{what} {o.name}")
        print(f"GEMM-EDGE {group} {what} {o.name}: worst error / tolerance {worst:.3f}")
        assert worst <= 1.0, f"{group} {what}: {o.name}: error / tolerance {worst:.3f} at {tuple(int(i) for i in (ratio == ratio.max()).nonzero()[0])}"


def same_bits(a, b, what):
    for k in a:
        if a[k] is not None:
            x, y = a[k].reshape(-1), b[k].reshape(-1)
            iv = torch.int16 if x.dtype == torch.bfloat16 else torch.int32
            assert torch.equal(x.view(iv), y.view(iv)), f"{what}: {k} differs in {int((x.view(iv) != y.view(iv)).sum())} words"


def same_values(ra, ga, rb, gb, what):
    """The owned values of two runs of one problem under different strides: equal bit for bit."""
    for oa, ob in zip(ra.outs, rb.outs):
        if oa.role in ("raw", "act"):
            va, vb = oa.values(ga[oa.name]), ob.values(gb[ob.name])
            assert torch.equal(va, vb), f"{what}: {oa.name} differs at {int((va != vb).sum())} elements"


def whole(case, group, what, **extra):
    ref, got = reference(case), run(case, **extra)
    check(case, ref, got, group, what)
    return ref, got


# ------------------------------------------------------------------------------------------------ 1. epilogue x store path x tile
MS = (1, 63, 65, 129, 257)
NS = (4, 36, 60, 68, 100, 132, 196, 260)
NS_ODD = (1, 33, 66, 127)
NS_GLU = (64, 128, 192, 320)
EPIS = {"f32": ("none", "gelu", "tanh", "res", "res_scale", "res_inplace", "glu"),
        "x3": ("none", "gelu", "res", "res_scale", "res_inplace", "rope"),
        "x6": ("none", "gelu", "res", "res_scale", "res_inplace", "glu"),
        "f16": ("none", "gelu", "res", "res_scale", "res_inplace", "glu"),
        "x1": ("none", "gelu", "res", "res_scale", "res_inplace", "glu", "rope")}
EPI_KW = {"none": dict(), "gelu": dict(epi=GELU), "tanh": dict(epi=TANH), "res": dict(epi=RES), "res_scale": dict(epi=RES, scale=True),
          "res_inplace": dict(epi=RES, inplace=True), "glu": dict(epi=GLU)}
# store-path variants, each alone against the aligned strides: (name, make() arguments)
VARIANTS = (("ldc odd", dict(sc=5)), ("c_off breaks 16 bytes", dict(c_mis=1)), ("c_off by 8 bytes", dict(c_mis=2)),
            ("ldr odd", dict(sr=7)), ("r_off breaks 16 bytes", dict(r_mis=3)), ("R strides other than C's", dict(sr=24, pads=(8, 12, 44, 24))))


@pytest.mark.parametrize("entry,epi", [(e, p) for e in EPIS for p in EPIS[e]])
def test_epilogues_on_both_store_paths_and_every_tile_shape(entry, epi):
    """Group 1.  Every epilogue of the entry point x every tile override x N over the ragged list (M cycles through 1, 63, 65, 129,
    257 so that every (M, N) pair meets some tile shape), K = 36 (a K tail).  Each case runs twice: with 16-byte aligned strides
    (vector stores) and with ONE misalignment (odd ldc, odd ldr, a C or R offset off 16 bytes, R strides unlike C's): the scalar
    path must give the same values bit for bit, and both must be inside the bound with every canary alive."""
    K = 36
    ns = NS_GLU if epi == "glu" else NS + (NS_ODD if epi != "rope" else ())
    n = 0
    # EPI_ROPE takes 16-byte aligned rows only; without a residual there is no R to misalign; in place R is C
    cands = () if epi == "rope" else (VARIANTS if epi in ("res", "res_scale") else VARIANTS[:3])
    seen = set()  # (tile, M) and (tile, variant) pairs that ran
    for ti, cfg in enumerate(TILES[entry]):
        for ni, N in enumerate(ns):
            # an entry point with one tile shape (bf16x1) crosses M with N; the others cycle M so that every M meets every tile
            for M in (MS if len(TILES[entry]) == 1 else (MS[(ni + ti + len(epi)) % len(MS)],)):
                if epi == "rope":
                    dh = (8, 32, 64)[ni % 3]
                    if N < dh:
                        continue
                    ekw = dict(epi=ROPE, rope=(N // dh * dh if ni % 2 else dh, dh, 3, 50))
                else:
                    ekw = EPI_KW[epi]
                var = cands[n % len(cands)] if cands else None
                n += 1
                seen.update({(cfg, M), (cfg, var[0] if var else None)})
                what = f"{entry} {epi} tile {cfg} M {M} N {N}"
                with tile(entry, cfg):
                    base = make(entry, M, N, K, seed=n, **ekw)
                    rb, gb = whole(base, "1 epilogues", what + " aligned")
                    if var is not None:
                        alt = make(entry, M, N, K, seed=n, **dict(ekw, **var[1]))
                        ra, ga = whole(alt, "1 epilogues", what + " " + var[0])
                        same_values(rb, gb, ra, ga, what + ": " + var[0] + " against aligned strides")
    # what the cycling promises: on every tile shape every M of the list ran (GLU's four N: four of the five), and every variant did
    for cfg in TILES[entry]:
        assert len({m for m in MS if (cfg, m) in seen}) >= min(len(MS), len(ns) - (2 if epi == "rope" else 0)), (cfg, sorted(seen, key=str))
        if len(ns) >= len(cands):
            assert all((cfg, v[0]) in seen for v in cands), (cfg, sorted(seen, key=str))


def test_one_pass_128_tile_is_reached_by_shape():
    """bf16x1 has no tile override: "every tile shape" in groups 1-3 and 6 means its by-shape 64-row tiles, and its 128 x 128 tile is
    taken from 256 tiles of that size on - here 16381 rows x 200 (192 for GLU) columns.  The forms of the other groups on that tile:
    epilogues on both store paths, GLU / ADDVEC / fused RMSNorm (the second launcher), bf16 rows 6 / 7 / 8 with segments whose end
    falls one row before a tile's, the activated copies, a K tail with the 1e30 rows behind each prologue, and the producer's
    LayerNorm statistics."""
    M = 16384 - 3
    for N, K, ekw in ((200, 36, dict()), (200, 36, dict(epi=RES, scale=True, sr=7)), (200, 36, dict(epi=GELU, sc=5)),
                      (192, 36, dict(epi=GLU, c_mis=1)), (200, 36, dict(pro=P_ADD, big_tail=True)), (200, 36, dict(pro=P_ELU, big_tail=True)),
                      (200, 32, dict(rms=True)), (192, 32, dict(rms=True, epi=GLU)), (200, 32, dict(rms=True, epi=GELU)),
                      (200, 36, dict(a_fmt=2, c_mode=8, rps=127)), (200, 36, dict(a_fmt=2, epi=RES, c_mode=7, scale=True, rps=127)),
                      (200, 36, dict(a_fmt=2, c_mode=6, big_tail=True)), (200, 36, dict(c_mode=4, rps=255)), (200, 36, dict(c_mode=7)),
                      (200, 36, dict(epi=RES, c_mode=3, rps=100)), (192, 64, dict(epi=RES, ln_out=True, rps=127)), (200, 64, dict(ln=True))):
        whole(make("x1", M, N, K, seed=5, **ekw), "1 epilogues", f"x1 128-row tiles {N} x {K} {ekw}")


# ------------------------------------------------------------------------------------------------ 2. segments
# 63 / 127 / 255: a segment ends one row before a 64 / 128 / 256-row tile does; 65 / 129: one row after the tile's first
RPS = (1, 3, 5, 37, 64, 100, 128, 200, 63, 65, 127, 129, 255)
SEG_M = {1: 130, 3: 261, 5: 260, 37: 296, 64: 320, 100: 300, 128: 384, 200: 400, 63: 189, 65: 195, 127: 381, 129: 387, 255: 510}
SEG_FORMS = {"f32": (dict(epi=RES, scale=True), dict(epi=GLU), dict(epi=RES, inplace=True)),
             "x3": (dict(epi=RES, scale=True), dict(c_mode=3), dict(c_mode=4), dict(c_mode=1), dict(c_mode=2), dict(a_fmt=1, c_mode=2),
                    dict(a_fmt=1, epi=RES, c_mode=1), dict(a_fmt=1, c_mode=4), dict(epi=RES, c_mode=3)),
             "x6": (dict(epi=RES, scale=True), dict(epi=GLU)),
             "f16": (dict(epi=RES, inplace=True), dict(epi=GLU)),
             "x1": (dict(epi=RES, scale=True), dict(c_mode=4), dict(c_mode=7), dict(a_fmt=2, c_mode=8), dict(a_fmt=2, epi=RES, c_mode=7, scale=True),
                    dict(a_fmt=2, c_mode=6), dict(a_fmt=2, c_mode=0))}


@pytest.mark.parametrize("entry", list(SEG_FORMS))
@pytest.mark.parametrize("rps", RPS)
def test_segments_with_their_own_strides_on_every_tile_shape(entry, rps):
    """Group 2.  M a multiple of rows_per_seg (1, 3, 5: less than the rows a store pass advances; 128 and 200: tiles wholly inside a
    segment next to tiles that straddle one and a ragged last tile; 63, 65, 127, 129, 255: a whole tile with ONE row in the
    neighbouring segment), A / C / R / C2 each with its own segment stride, N = 132
    (a whole column tile and a ragged one), K = 64; residual, activated, split-form and bf16-row flows; every tile shape."""
    M = SEG_M[rps]
    for cfg in TILES[entry]:
        for fi, f in enumerate(SEG_FORMS[entry]):
            N = 128 if f.get("epi") == GLU else 132
            if f.get("epi") == GLU and cfg == 5 and entry == "x6":
                continue
            with tile(entry, cfg):
                whole(make(entry, M, N, 64, rps=rps, seed=rps + fi, **f), "2 segments", f"{entry} rps {rps} tile {cfg} {f}")


@pytest.mark.parametrize("entry", ["f32", "x3", "x6", "f16", "x1"])
def test_overlapping_rows_are_convolutions(entry):
    """Group 2, lda < K: the causal k = 7 convolution's windows (K = 7 lda) and the transposed convolutions' (K = 2 lda; strides 4,
    5, 8 are N = 4, 5, 8 x 24 output columns), three utterances of 37 rows, with a residual, activated outputs and the split-form flow."""
    forms = {"f32": (dict(epi=RES),), "x3": (dict(epi=RES), dict(c_mode=3), dict(c_mode=4), dict(pro=P_ELU, epi=RES)),
             "x6": (dict(epi=RES),), "f16": (dict(epi=RES),), "x1": (dict(epi=RES), dict(c_mode=4), dict(a_fmt=2, c_mode=8), dict(a_fmt=2, epi=RES, c_mode=7))}[entry]
    for cfg in TILES[entry]:
        for f in forms:
            for lda, K, N in ((8, 56, 36), (16, 32, 4 * 24), (16, 32, 5 * 24), (16, 32, 8 * 24)):
                with tile(entry, cfg):
                    whole(make(entry, 111, N, K, rps=37, lda=lda, seed=K + N, **f), "2 segments", f"{entry} windows lda {lda} K {K} N {N} tile {cfg} {f}")
        if entry == "x3":  # split-form rows: 32-channel frames, windows of 2 and of 7 frames
            for f in (dict(c_mode=1), dict(c_mode=2), dict(c_mode=0), dict(epi=RES, c_mode=1)):
                for lda, K, N in ((32, 64, 96), (32, 224, 36)):
                    with tile(entry, cfg):
                        whole(make(entry, 111, N, K, rps=37, lda=lda, a_fmt=1, seed=K, **f), "2 segments", f"x3 split windows K {K} tile {cfg} {f}")


# ------------------------------------------------------------------------------------------------ 3. K tail
KS = (4, 12, 36, 68, 100, 160)


@pytest.mark.parametrize("entry", ["f32", "x3", "x6", "f16", "x1"])
@pytest.mark.parametrize("K", KS)
def test_k_tail_clamped_reads_contribute_nothing(entry, K):
    """Group 3.  K % 32 != 0 (and K < 32): the packed kernels re-read the row's last four elements for the steps past K and rely on
    the zero padding of W there.  Every third row ends in 1e30 x 4 against four zero weight columns: the true contribution is 0, so
    anything the re-read lets through shows at 1e29 against a bound of order 1e-5.  Prologues NONE / ELU / ADDVEC (pro_vec is read
    at the clamped k too, NaN behind its K entries) and bf16 rows on the one-pass kernel."""
    pros = {"f32": (P_NONE, P_ELU, P_ADD), "x3": (P_NONE, P_ELU), "x6": (P_NONE, P_ADD), "f16": (P_NONE, P_ADD), "x1": (P_NONE, P_ELU, P_ADD)}[entry]
    for pro in pros:
        for big in (False, True):
            for M, N in ((70, 68), (5, 132)):
                whole(make(entry, M, N, K, pro=pro, big_tail=big, seed=K), "3 K tail", f"{entry} K {K} pro {pro} big {big} {M}x{N}")
    if entry == "x1":
        for big in (False, True):
            whole(make(entry, 70, 68, K, a_fmt=2, big_tail=big, seed=K), "3 K tail", f"x1 bf16 rows K {K} big {big}")
            whole(make(entry, 70, 68, K, a_fmt=2, c_mode=8, big_tail=big, seed=K), "3 K tail", f"x1 bf16 rows in and out K {K} big {big}")


# ------------------------------------------------------------------------------------------------ 4. tile walk
@pytest.mark.parametrize("entry", ["x3", "x6", "f16", "x1"])
def test_grouped_tile_walk_writes_every_tile_once(entry):
    """Group 4.  group_m 1, 2, 3, 5, 8, 64 at 1, 2, 3, 7, 9 row tiles x 1, 3, 5 column tiles (totals 1 .. 45, primes and
    non-multiples of 8 among them: the part-filled last group and the XCD-contiguous map): bit-identical to group_m = 1, no NaN
    left, canaries alive.  In-place residual: a tile written twice would add its contraction twice."""
    bm, bn = {"x3": (128, 128), "x6": (64, 64), "f16": (64, 64), "x1": (64, 64)}[entry]
    for ntm in (1, 2, 3, 7, 9):
        for ntn in (1, 3, 5):
            M, N = ntm * bm - 5, ntn * bn - 28
            case = make(entry, M, N, 32, epi=RES, inplace=True, seed=ntm * 10 + ntn)
            ref, base = whole(case, "4 tile walk", f"{entry} {ntm}x{ntn} tiles group_m 1", group_m=1)
            for gm in (2, 3, 5, 8, 64):
                got = run(case, group_m=gm)
                same_bits(base, got, f"{entry} {ntm}x{ntn} tiles: group_m {gm} against 1")


def test_grouped_tile_walk_long_k_form():
    for ntm, ntn in ((1, 1), (3, 2), (5, 1)):
        case = make("8p", ntm * 256 - 9, ntn * 256, 64, a_fmt=1, seed=ntm)
        ref, base = whole(case, "4 tile walk", f"8p {ntm}x{ntn} tiles group_m 1", group_m=1)
        for gm in (2, 3, 8):
            same_bits(base, run(case, group_m=gm), f"8p {ntm}x{ntn} tiles: group_m {gm} against 1")


# ------------------------------------------------------------------------------------------------ 5. split-K
SPLIT_FORMS = {"x3": (dict(), dict(epi=GELU), dict(epi=RES, inplace=True), dict(c_mode=3)),
               "x6": (dict(), dict(epi=GELU), dict(epi=RES, inplace=True), dict(epi=GLU)),
               "f16": (dict(), dict(epi=GELU), dict(epi=RES, inplace=True), dict(epi=GLU)),
               "x1": (dict(), dict(epi=GELU), dict(epi=RES, inplace=True), dict(epi=GLU), dict(c_mode=3))}


@pytest.mark.parametrize("entry", list(SPLIT_FORMS))
@pytest.mark.parametrize("ks,K", [(2, 160), (3, 160), (3, 224), (5, 224), (7, 256), (16, 544), (4, 64), (16, 96)])
def test_explicit_split_k(entry, ks, K):
    """Group 5.  An explicit slice count: K-step counts it does not divide (5, 7, 8, 17 steps), more slices than steps (K = 64 with 4,
    K = 96 with 16: trailing empty slices), two row tiles and a ragged last tile in both directions.  Three launches are bit-equal,
    inside the entry point's bound, and leave every ticket at zero.  (ksplit = 1: test_ksplit_one_is_the_unsplit_launch.)"""
    tickets = hip._splitk_buffers()[1]
    bm = 128 if entry == "x3" else 64
    for f in SPLIT_FORMS[entry]:
        M, N = bm + 7, 256 if f.get("epi") == GLU else 200
        case = make(entry, M, N, K, seed=ks + K, **f)
        ref, first = whole(case, "5 split-K", f"{entry} ksplit {ks} K {K} {f}", ksplit=ks)
        assert int(tickets.abs().sum()) == 0, f"{entry} ksplit {ks} K {K} {f}: tickets not back at zero"
        for _ in range(2):
            same_bits(first, run(case, ksplit=ks), f"{entry} ksplit {ks} K {K} {f}: repeated launch")
        assert int(tickets.abs().sum()) == 0


def unsplit(case):
    """The launch with the host's automatic split switched off: the unsplit kernel whatever the shape."""
    old = hip._splitk_enabled
    hip._splitk_enabled = False
    try:
        return run(case)
    finally:
        hip._splitk_enabled = old


@pytest.mark.parametrize("entry", list(SPLIT_FORMS))
def test_ksplit_one_is_the_unsplit_launch(entry):
    """Group 5.  ksplit = 1 against the launch without any split (the automatic choice switched off): bit-equal for EVERY form, since
    the library runs its unsplit kernel for 0 and 1 - also at K = 1024 on a few rows, where a call without the argument is NOT the
    comparand: `_auto_ksplit` splits it (asserted), and a split adds per-slice partial sums in another order."""
    for K in (160, 1024):
        for f in SPLIT_FORMS[entry]:
            M, N = 7, 256 if f.get("epi") == GLU else 200
            case = make(entry, M, N, K, seed=K, **f)
            ref, one = whole(case, "5 split-K", f"{entry} ksplit 1 K {K} {f}", ksplit=1)
            same_bits(one, unsplit(case), f"{entry} K {K} {f}: ksplit 1 against the unsplit launch")
            pieces = {"x3": 2, "x6": 3, "f16": 3, "x1": 1}[entry]
            assert (hip._auto_ksplit(M, N, K, pieces, f.get("epi", NONE)) > 1) == (K == 1024)
    assert int(hip._splitk_buffers()[1].abs().sum()) == 0


def test_split_k_that_does_not_fit_is_refused():
    refused(make("x6", 70, 68, 64), ksplit=65)
    refused(make("x6", 2100, 2100, 32), ksplit=2)  # 33 x 33 tiles of 64 x 64: more than the stream's 1024 tickets
    refused(make("f32", 70, 68, 64), ksplit=2)     # the fp32 kernel has no split-K
    refused(make("f32", 70, 68, 64), group_m=2)
    assert int(hip._splitk_buffers()[1].abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ 6. special outputs
@pytest.mark.parametrize("entry", ["x6", "f16", "x1"])
@pytest.mark.parametrize("M,N", [(70, 200), (129, 2048 + 40), (5, 40), (63, 130), (8192 + 5, 200), (8192 + 5, 2048)])
def test_argmax_partials_at_ragged_shapes_with_exact_ties(entry, M, N):
    """Group 6, c_mode 5.  Small-integer operands: every logit is exact on every entry point, so the pairs are compared bit for bit.
    N is no multiple of 128 (nor of 64: the last group has 8 / 40 / 2 live columns), M is ragged, and duplicated weight rows put exact
    ties inside a group, across a 64-column boundary and into the last partial row tile: the first column wins.  From 8192 rows on
    the launcher takes 128-row tiles (N = 200: 128 x 64) and, with N >= 2048 a multiple of 128, 128 x 128 tiles: other thread
    layouts of the per-64-column reduction, where the tie rule also decides between threads."""
    K = 32
    case = make(entry, M, N, K, c_mode=5, ints=True, wseed=N, seed=M)
    W = case["W"].clone()
    W[min(70, N - 1)] = W[3]          # a tie across the 64-column boundary (for the row's arg-max)
    if N > 20:
        W[17] = W[3]                  # inside a group
        W[N - 1] = W[N - 2]           # in the last (part-filled) group
    if N > 64:
        W[40] = W[3]                  # in the same group, in another thread's 32 columns on the 128 x 64 tile
        case["kw"]["bias"][40] = case["kw"]["bias"][3]
    Wd = W.to(DEV)
    case["W"], case["Wop"] = W, {"x6": hip.pack_w_bf16x6, "f16": hip.pack_w_f16x3, "x1": hip.pack_w_bf16x1}[entry](Wd)
    case["kw"]["bias"][min(70, N - 1)] = case["kw"]["bias"][3]
    if N > 20:
        case["kw"]["bias"][17] = case["kw"]["bias"][3]
        case["kw"]["bias"][N - 1] = case["kw"]["bias"][N - 2]
    ref, got = whole(case, "6 special outputs", f"{entry} arg-max {M}x{N}")
    G_ = -(-N // 64)
    pairs = got["C2"][4: 4 + M * (G_ + 1) * 2].reshape(M, G_ + 1, 2)
    vals, idx = pairs[:, :G_, 0], pairs[:, :G_, 1].contiguous().view(torch.int32).long()
    best = vals.max(dim=1).values
    first = torch.where(vals == best[:, None], idx, torch.full_like(idx, 1 << 30)).min(dim=1).values
    assert torch.equal(first, ref.out.argmax(dim=1)), "combined partials are not torch.argmax of the logits"


@pytest.mark.parametrize("entry", ["x3", "x1"])
def test_ln_stats_out_equals_row_stats_of_the_written_stream(entry):
    """Group 6.  The producer's statistics are bit-equal to sopro_row_stats_f32 run on the stream it wrote, at ragged M, with
    segments (C and R with their own strides) and on every tile shape."""
    for cfg in TILES[entry]:
        for M, rps, N in ((70, None, 128), (111, 37, 192), (257, None, 64), (300, 100, 320)):
            case = make(entry, M, N, 64, epi=RES, scale=True, ln_out=True, rps=rps, seed=M)
            with tile(entry, cfg):
                ref, got = whole(case, "6 special outputs", f"{entry} ln_stats_out {M}x{N} rps {rps} tile {cfg}")
            kw = case["kw"]
            st = torch.full((M * (N // 64) * 2,), NAN, device=DEV)
            hip.row_stats(got["C"].to(DEV), M, N, st, ldx=kw["ldc"], x_seg_stride=kw["c_seg_stride"], rows_per_seg=kw["rows_per_seg"], x_off=kw["c_off"])
            torch.cuda.synchronize()
            mine = got["ln_stats_out"][: M * (N // 64) * 2]
            assert torch.equal(mine.view(torch.int32), st.cpu().view(torch.int32)), f"{entry} {M}x{N} tile {cfg}: statistics differ from row_stats"
            want = ref["ln_stats_out"].ref.reshape(-1)
            # (64 terms per pair, each a few fp32 roundings of a value or of a squared deviation)
            assert float((mine.double() - want).abs().max()) <= 256 * U * (float(ref.out.abs().max()) + 1.0) ** 2


@pytest.mark.parametrize("entry", ["x3", "x1"])
def test_fused_layernorm_consumer_on_every_tile_shape(entry):
    """Group 6.  ln_stats consumer (NONE / GELU / ROPE) with ragged M and N, a row mean far from zero, every tile shape."""
    for cfg in TILES[entry]:
        for fi, f in enumerate((dict(), dict(epi=GELU), dict(epi=ROPE, rope=(64, 32, 2, 40)))):
            for M, N, K in ((70, 100, 64), (257, 132, 128)):
                with tile(entry, cfg):
                    whole(make(entry, M, N, K, ln=True, seed=fi + M, **f), "6 special outputs", f"{entry} ln_stats {M}x{N}x{K} tile {cfg} {f}")


@pytest.mark.parametrize("entry", ["x3", "x1"])
@pytest.mark.parametrize("dh", [8, 32, 64])
def test_rope_epilogue_partial_columns_and_positions(entry, dh):
    """Group 6.  EPI_ROPE with rope_cols < N, a first position > 0 and rope_rows_per_seg (7, 50, 100) that does not divide a tile."""
    for cfg in TILES[entry]:
        for M, N, rcols, rrps in ((65, 132, 64, 7), (257, 196, 128, 50), (300, 68, 64, 100)):
            with tile(entry, cfg):
                whole(make(entry, M, N, 36, epi=ROPE, rope=(rcols, dh, 5, rrps), seed=dh + M), "6 special outputs", f"{entry} rope dh {dh} {M}x{N} tile {cfg}")


# ------------------------------------------------------------------------------------------------ 7. long-K form
@pytest.mark.parametrize("K", [32, 96, 160])
@pytest.mark.parametrize("N", [256, 512])
def test_long_k_form_small_problems_equal_the_tile_kernel(N, K):
    """Group 7.  sopro_gemm_bf16x3_8p from its smallest problem (one 256-column tile, K = 32: one K-tile) up: M = 1, 255, 257 and
    3 x 100 row windows (lda = 32 < K), c_mode 0 / 1 / 2 / 4 - bit-identical to sopro_gemm_bf16x3 on the same operands, inside the
    three-pass bound, canaries alive."""
    for M, rps, lda in ((1, None, None), (255, None, None), (257, None, None), (300, 100, 32 if K > 32 else None)):
        for c_mode in (0, 1, 2, 4):
            case = make("8p", M, N, K, a_fmt=1, c_mode=c_mode, rps=rps, lda=lda, seed=M + c_mode)
            ref, got = whole(case, "7 long-K form", f"8p {M}x{N}x{K} c_mode {c_mode}")
            same_bits(got, run(dict(case, entry="x3")), f"8p against the tile kernel {M}x{N}x{K} c_mode {c_mode}")


def test_long_k_takes_is_consistent_with_the_entry_point():
    """Group 7.  Whatever sopro_gemm_8p_takes accepts, the entry point accepts: each condition it tests is one the entry point
    refuses (with the output untouched), and the size conditions (K >= 1024, >= 128 tiles) only say when the form pays."""
    lib = hip.load()
    g, x = hip.GemmArgs(), hip.SplitExt()
    g.M, g.N, g.K, g.prologue, g.epilogue = 32768, 256, 1024, 0, 0
    x.a_format = 1
    assert lib.sopro_gemm_8p_takes(C.byref(g), C.byref(x)) == 1
    for field, obj, bad in (("a_format", x, 0), ("prologue", g, 1), ("epilogue", g, 1), ("rms_norm", x, 1), ("ksplit", x, 2), ("c_mode", x, 3), ("N", g, 384), ("K", g, 1040)):
        old = getattr(obj, field)
        setattr(obj, field, bad)
        assert lib.sopro_gemm_8p_takes(C.byref(g), C.byref(x)) == 0, field
        setattr(obj, field, old)
    g.K = 992
    assert lib.sopro_gemm_8p_takes(C.byref(g), C.byref(x)) == 0  # too short to pay: still a legal call (the cases above)
    ok = make("8p", 70, 256, 64, a_fmt=1)
    for bad in (dict(epi=GELU), dict(c_mode=3), dict(a_fmt=0)):
        refused(make("8p", 70, 256, 64, **dict(dict(a_fmt=1), **bad)))
    refused(make("8p", 70, 128, 64, a_fmt=1))   # N % 256
    # the operand and output geometry checks of the entry point (its K % 32 and w_rows checks cannot be reached through hip.gemm:
    # the split-form weight rows it passes exist only for K % 32 == 0 and are allocated 128-byte aligned)
    refused(ok, dict(lda=ok["kw"]["lda"] + 4))
    refused(ok, dict(a_seg_stride=ok["kw"]["a_seg_stride"] + 4))
    refused(ok, dict(a_off=ok["kw"]["a_off"] + 4))                                   # A base off 128 bytes
    refused(make("8p", 70, 256, 64, a_fmt=1, sc=8), dict(c_mode=1))                 # split-form C: ldc % 32
    c2 = make("8p", 70, 256, 64, a_fmt=1, c_mode=2)
    refused(c2, dict(ldc2=c2["kw"]["ldc2"] + 4))                                     # split-form C2: ldc2 % 32
    c4 = make("8p", 70, 256, 64, a_fmt=1, c_mode=4)
    refused(c4, dict(ldc2=c4["kw"]["ldc2"] + 1))                                     # activated C2: ldc2 % 4
    refused(c4, dict(ldc2=252))                                                      # ... ldc2 < N
    refused(ok, dict(c_mode=4))                                                      # ... no C2
    whole(ok, "7 long-K form", "8p 70x256x64 after the refusals")


# ------------------------------------------------------------------------------------------------ 8. rejections
def refused(case, dkw=None, **extra):
    """``dkw`` applied on top of a valid case (one change), the operands uploaded, the call made: it raises SoproHipError and
    every word of the device-side output buffers is what was uploaded.  Tensors in ``dkw`` that are on the device already are
    passed as they are (a view that starts off a 16-byte boundary stays one)."""
    bad = dict(case, kw=dict(case["kw"], **(dkw or {})))
    d = lambda t: None if t is None else t.to(DEV)
    Cd, C2d = d(bad["C"]), d(bad["C2"])
    kw = {k: (d(v) if isinstance(v, torch.Tensor) else v) for k, v in bad["kw"].items()}
    if kw.get("rope") is not None:
        r = kw["rope"]
        kw["rope"] = (d(r[0]), d(r[1])) + tuple(r[2:])
    if bad["entry"] == "8p":
        extra = dict(extra, long_k=True)
    with pytest.raises(hip.SoproHipError):
        hip.gemm(d(bad["A"]), bad["Wop"], Cd, R=Cd if bad["inplace"] else d(bad["R"]), C2=C2d, **kw, **extra)
    torch.cuda.synchronize()
    for dev_t, host_t in ((Cd, bad["C"]), (C2d, bad["C2"])):
        if dev_t is not None:
            iv = torch.int16 if host_t.dtype == torch.bfloat16 else torch.int32
            assert torch.equal(dev_t.cpu().reshape(-1).view(iv), host_t.reshape(-1).view(iv)), f"a refused call wrote its output: {dkw} {extra}"


@pytest.mark.parametrize("entry", ["f32", "x3", "x6", "f16", "x1"])
def test_argument_checks_refuse_and_leave_the_output_alone(entry):
    """Group 8.  The argument checks of the entry points that the groups above did not trigger: each is ONE change to a valid call
    with guard rows around every buffer, raises SoproHipError and leaves the output canary untouched.  (The long-K form's are in
    test_long_k_takes_is_consistent_with_the_entry_point.)  Not reachable through hip.gemm, which always passes them valid: a NULL
    args / ext / weight pointer, a packed weight or weight rows off their alignment (the packers allocate them), K % 32 of the
    long-K entry point (no weight rows exist for such a K), a K other than the packed weight's (hip.gemm compares them itself; K = 34
    below is that refusal for the packed entry points and the library's K % 4 for sopro_gemm_f32)."""
    ok = make(entry, 70, 68, 36, epi=RES, scale=True)
    for dkw in (dict(M=0), dict(K=34), dict(rows_per_seg=0), dict(lda=41), dict(a_seg_stride=ok["kw"]["a_seg_stride"] + 2), dict(a_off=ok["kw"]["a_off"] + 1)):
        refused(ok, dkw)
    refused(make(entry, 70, 68, 36), dict(epilogue=RES))  # EPI_RES without R
    if entry != "x3":
        addv = make(entry, 70, 68, 36, pro=P_ADD)
        refused(addv, dict(pro_vec=None))
        refused(addv, dict(pro_vec=torch.zeros(41, device=DEV)[1:]))  # not 16-byte aligned
    refused(make(entry, 70, 68, 36), dict(epilogue=GLU) if entry != "x3" else dict(epilogue=TANH))  # GLU: N % 64; x3: no tanh
    refused(make(entry, 70, 68, 36), dict(epilogue=5))   # the skinny kernel's epilogue
    refused(make(entry, 70, 68, 36), dict(prologue=3))
    if entry == "f32":
        refused(make(entry, 70, 68, 36), dict(epilogue=ROPE))
        refused(make(entry, 70, 68, 36), dict(ldw=38))
        return
    refused(make(entry, 70, 68, 36), dict(), ksplit=65)
    refused(make(entry, 70, 68, 64), dict(dbg=torch.zeros(512, dtype=torch.int64)), ksplit=2)  # the clock-stamp probe is for unsplit launches
    # K rules of the fused norms and the split form, at K = 36
    plain = make(entry, 70, 128, 36)
    if entry in ("x6", "f16", "x1"):
        refused(plain, dict(rms_eps=1e-6))                     # fused RMSNorm: K % 32
        refused(make(entry, 70, 128, 64, pro=P_ADD), dict(rms_eps=1e-6))  # ... and no prologue
        refused(make(entry, 70, 128, 64), dict(rms_eps=1e-6), ksplit=2)    # ... and no split-K
    if entry == "x3":
        refused(plain, dict(rms_eps=1e-6))                                   # fused RMSNorm is not a three-pass feature
    if entry in ("x3", "x1"):
        refused(plain, dict(ln_stats=torch.zeros(70 * 2), ln_eps=1e-5))   # fused LayerNorm: K % 64
        refused(make(entry, 70, 128, 64), dict(ln_stats=torch.zeros(70 * 2), ln_eps=0.0))  # eps > 0
        refused(make(entry, 70, 128, 64, epi=RES), dict(ln_stats=torch.zeros(70 * 2), ln_eps=1e-5))  # epilogue NONE / GELU / ROPE
        refused(make(entry, 70, 100, 64, epi=RES), dict(ln_stats_out=torch.zeros(70 * 4)))  # N % 64
        refused(make(entry, 70, 128, 64), dict(ln_stats_out=torch.zeros(70 * 4)))           # EPI_RES only
        refused(make(entry, 70, 128, 64, epi=RES, sc=5), dict(ln_stats_out=torch.zeros(70 * 4)))  # aligned rows
        rp = make(entry, 70, 132, 36, epi=ROPE, rope=(64, 32, 0, 70))
        for bad in ((64, 128, 0, 70), (64, 24, 0, 70), (48, 32, 0, 70), (192, 32, 0, 70), (64, 32, -1, 70), (64, 32, 0, 0)):
            refused(rp, dict(rope=rp["kw"]["rope"][:2] + bad))
        refused(rp, dict(c_off=rp["kw"]["c_off"] + 1))          # EPI_ROPE: 16-byte aligned output rows
        off4 = lambda n: torch.zeros(n + 1, device=DEV)[1:]    # a device view that starts 4 bytes off its allocation
        cs = rp["kw"]["rope"]
        refused(rp, dict(rope=(off4(cs[0].numel()), cs[1]) + cs[2:]))   # cos table off 16 bytes
        refused(rp, dict(rope=(cs[0], off4(cs[1].numel())) + cs[2:]))   # sin table
        refused(make(entry, 70, 128, 64), dict(ln_stats=off4(70 * 2), ln_eps=1e-5))                         # ln_stats off 8 bytes
        refused(make(entry, 70, 128, 64, epi=RES, ln_out=True), dict(ln_stats_out=off4(70 * 4)))            # ln_stats_out off 8 bytes
        refused(make(entry, 70, 68, 36), dict(c_mode=4))                                                    # c_mode 4 without C2
        refused(make(entry, 70, 68, 36, c_mode=4), dict(ldc2=64))                                           # ... ldc2 < N
        refused(make(entry, 70, 66, 36, sc=2), dict(c_mode=3))  # activated output: N % 4
        refused(make(entry, 70, 68, 36, sc=5), dict(c_mode=3))  # ... aligned rows
    if entry == "x3":
        sp = make(entry, 70, 68, 64, a_fmt=1)
        refused(sp, dict(prologue=P_ELU))
        refused(sp, dict(lda=sp["kw"]["lda"] + 4))
        refused(sp, dict(a_off=sp["kw"]["a_off"] + 4))
        refused(make(entry, 70, 68, 36, a_fmt=0), dict(a_split=True))       # split form: K % 32
        refused(make(entry, 70, 68, 36, sc=8), dict(c_mode=1))   # split-form output: ld % 32
        refused(make(entry, 70, 68, 36, epi=GELU), dict(c_mode=3))  # not an available combination
        refused(make(entry, 70, 68, 36), dict(c_mode=5))
        s2 = make(entry, 70, 68, 36, c_mode=2)
        refused(s2, dict(ldc2=s2["kw"]["ldc2"] + 4))             # split-form C2: ldc2 % 32
        refused(make(entry, 70, 68, 36), dict(c_mode=2))         # ... no C2
    if entry == "x1":
        b8 = make(entry, 70, 68, 36, a_fmt=2, c_mode=8)
        refused(b8, dict(ldc2=64))                               # c_mode 8: ldc2 < N
        refused(make(entry, 70, 68, 36, a_fmt=2, c_mode=7), dict(c_mode=8))   # ... no C2
        # bf16 rows: N % 4 == 0 is what keeps the four-wide scale read of the bf16 RES epilogue inside `scale`
        for c_mode in (6, 7, 8):
            case = make(entry, 70, 66, 36, a_fmt=2, c_mode=7, epi=RES, scale=True)
            refused(case, dict(c_mode=c_mode, N=66))
        refused(make(entry, 70, 68, 36, a_fmt=2, c_mode=7), dict(c_off=make(entry, 70, 68, 36, a_fmt=2, c_mode=7)["kw"]["c_off"] + 2))
        refused(make(entry, 70, 68, 36, a_fmt=2, c_mode=7), dict(prologue=P_ELU))
        refused(make(entry, 70, 68, 36, a_fmt=2, c_mode=7), dict(epilogue=GELU))
        refused(make(entry, 70, 68, 36, c_mode=7), dict(c_mode=6))            # not an available combination
        refused(make(entry, 70, 68, 36), dict(c_mode=1))
        refused(make(entry, 70, 68, 36, a_fmt=2, c_mode=7), dict(lda=42))
    if entry in ("x6", "f16"):
        refused(make(entry, 70, 68, 36), dict(c_mode=3))
        refused(make(entry, 70, 68, 36), dict(prologue=P_ELU))
        am = make(entry, 70, 200, 32, c_mode=5, ints=True)
        refused(am, dict(ldc2=3))                                            # fewer pairs per row than 64-column groups
        refused(am, dict(epilogue=GELU))


# ------------------------------------------------------------------------------------------------ 9. seeded sweep
def draw(entry, rng):
    """One valid (shape, strides, offsets, segments, prologue, epilogue, output mode, tile, group_m) for the entry point."""
    ri = lambda *a: int(torch.randint(*a, (1,), generator=rng))
    pick = lambda xs: xs[ri(0, len(xs))]
    forms = {"f32": [dict(epi=e, pro=p) for e in (NONE, GELU, TANH, RES, GLU) for p in (P_NONE, P_ELU, P_ADD)],
             "x3": [dict(), dict(epi=GELU), dict(epi=RES), dict(pro=P_ELU), dict(pro=P_ELU, epi=RES), dict(c_mode=3), dict(c_mode=4), dict(epi=RES, c_mode=3),
                    dict(c_mode=1), dict(c_mode=2), dict(a_fmt=1), dict(a_fmt=1, c_mode=1), dict(a_fmt=1, c_mode=2), dict(a_fmt=1, c_mode=4),
                    dict(a_fmt=1, epi=RES, c_mode=1), dict(epi=ROPE), dict(ln=True), dict(ln=True, epi=GELU)],
             "x6": [dict(), dict(epi=GELU), dict(epi=RES), dict(pro=P_ADD), dict(epi=GLU), dict(rms=True), dict(rms=True, epi=GELU), dict(rms=True, epi=GLU)],
             "x1": [dict(), dict(epi=GELU), dict(epi=RES), dict(pro=P_ELU), dict(pro=P_ELU, epi=RES), dict(c_mode=3), dict(c_mode=4), dict(epi=RES, c_mode=3),
                    dict(epi=ROPE), dict(ln=True), dict(c_mode=7), dict(a_fmt=2, c_mode=8), dict(a_fmt=2, c_mode=7), dict(a_fmt=2, epi=RES, c_mode=7),
                    dict(a_fmt=2, c_mode=6), dict(a_fmt=2), dict(pro=P_ADD), dict(epi=GLU), dict(rms=True), dict(rms=True, epi=GELU), dict(rms=True, epi=GLU)],
             "8p": [dict(a_fmt=1, c_mode=c) for c in (0, 1, 2, 4)]}
    forms["f16"] = forms["x6"]
    f = dict(pick(forms[entry]))
    epi = f.get("epi", NONE)
    K = pick((32, 64, 96, 128) if (f.get("a_fmt") == 1 or f.get("rms")) else ((64, 128) if f.get("ln") else (4, 12, 32, 36, 64, 68, 96, 100, 128, 160)))
    if entry == "8p":
        N = pick((256, 512))
    elif epi == GLU:
        N = pick(NS_GLU)
    elif epi == ROPE:
        N = pick(NS[1:])
    elif f.get("c_mode", 0) != 0:
        N = pick(NS)
    else:
        N = pick(NS + NS_ODD)
    rps = pick((None, None, 1, 3, 5, 37, 63, 64, 100, 127))
    M = ri(1, 300) if rps is None else rps * ri(1, max(2, 300 // rps))
    if epi == ROPE:
        dh = pick([d for d in (8, 32, 64) if d <= N])
        f["rope"] = (dh * ri(1, N // dh + 1), dh, ri(0, 9), pick((7, 50, 1000)))
    if epi == RES:
        f["scale"] = bool(ri(0, 2))
        f["inplace"] = bool(ri(0, 2)) and f.get("c_mode", 0) == 0
    c_mode = f.get("c_mode", 0)
    free_c = c_mode in (0, 2, 4) and epi != ROPE    # the raw fp32 C takes any stride / offset
    f.update(sa=4 * ri(0, 4), sc=ri(0, 9) if free_c else 4 * ri(0, 3), sr=ri(0, 9) if free_c else 4 * ri(0, 3), s2=4 * ri(0, 4),
             pads=tuple(4 * ri(0, 8) for _ in range(4)) if not free_c else (4 * ri(0, 8), ri(0, 30), ri(0, 30), 4 * ri(0, 8)),
             c_mis=ri(0, 4) if free_c else 0, r_mis=ri(0, 4) if free_c else 0, dense_seg=ri(0, 4) == 0, bias=ri(0, 5) != 0)
    if f.get("inplace"):
        f["sr"], f["r_mis"] = f["sc"], f["c_mis"]
    if rps is not None and f.get("a_fmt", 0) != 1 and not f.get("ln") and not f.get("rms") and ri(0, 3) == 0 and K >= 32 and K % 16 == 0:
        f["lda"] = K // 2  # overlapping rows
    extra = dict(tile=pick(TILES[entry]))
    if entry != "f32":
        extra["group_m"] = pick((None, 1, 2, 3, 8))
    if epi == GLU and entry == "x6" and extra["tile"] == 5:
        extra["tile"] = 0
    return M, N, K, rps, f, extra


@pytest.mark.parametrize("entry", ["f32", "x3", "x6", "x1", "f16", "8p"])
def test_seeded_sweep(entry):
    """Group 9.  150 valid draws per entry point from a fixed seed, the same whole-buffer checks; a failure names its draw."""
    rng = gen(20240 + sum(map(ord, entry)))
    for i in range(150):
        M, N, K, rps, f, extra = draw(entry, rng)
        what = f"{entry} draw {i}: M {M} N {N} K {K} rps {rps} {f} {extra}"
        case = make(entry, M, N, K, rps=rps, seed=i, **f)
        kw = {k: v for k, v in extra.items() if k != "tile" and v is not None}
        with tile(entry, extra["tile"]):
            whole(case, "9 sweep", what, **kw)


def test_zz_worst_ratios_table():
    """Prints what the module measured (`pytest -s`): the worst error / tolerance per group and the fp32-libm errors behind the
    allowances.  Asserts only that the groups ran."""
    for grp in sorted(WORST):
        print(f"GEMM-EDGE-WORST {grp}: {WORST[grp][0]:.3f} at {WORST[grp][1]}")
    for fn in sorted(LIBM):
        print(f"GEMM-EDGE-LIBM {fn}: fp32 torch against float64 {LIBM[fn]:.3e} (x 4 allowed)")
    assert all(v[0] <= 1.0 for v in WORST.values())
