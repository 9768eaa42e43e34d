"""The float64 contraction reference (tests/gemm_ref.py) against independent formulations: torch's own linear / convolution /
activation / normalisation operators, the oracle's RMSNorm and rotate-half RoPE, torch.argmax and torch's bf16 cast.  CPU only."""
import math

import pytest
import torch
import torch.nn.functional as F

import gemm_ref as G
from oracle import sopro_oracle as O
from sopro_amd import pack

NAN = float("nan")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).float()


def canary(n, dtype=torch.float32):
    return torch.full((n,), NAN, dtype=dtype)


def assert_owned_only(o, before):
    """Everything outside the operation's own words is bit for bit what the caller put there; nothing owned is left NaN."""
    own = o.owned()
    assert torch.equal(o.bits(o.buf)[~own], o.bits(before)[~own])
    assert bool(torch.isfinite(o.values(o.buf)).all())


def close64(a, b, tol):
    err = float((a.double() - b.double()).abs().max())
    assert err <= tol, f"max abs err {err:.3e} > {tol:.1e}"


def test_linear_with_slack_offsets_and_segments():
    M, N, K, rps = 12, 10, 8, 4
    A, W, b = rnd(M, K, seed=1), rnd(N, K, seed=2), rnd(N, seed=3)
    lda, a_seg, a_off = K + 4, 4 * (K + 4) + 8, 12
    ldc, c_seg, c_off = N + 3, 4 * (N + 3) + 5, 7
    Ab = canary(a_off + 3 * a_seg)
    st = G.row_starts(M, rps, lda, a_seg, a_off)
    Ab[st[:, None] + torch.arange(K)[None, :]] = A
    Cb = canary(c_off + 3 * c_seg)
    r = G.gemm_ref(Ab, W, Cb, M=M, N=N, K=K, lda=lda, ldc=ldc, bias=b, rows_per_seg=rps, a_seg_stride=a_seg, c_seg_stride=c_seg,
                   a_off=a_off, c_off=c_off)
    want = F.linear(A.double(), W.double(), b.double())
    close64(r.out, want, 1e-13)
    o = r["C"]
    assert_owned_only(o, Cb)
    assert int(o.owned().sum()) == M * N
    close64(o.values(o.buf), want, 2.0 ** -23 * float(want.abs().max()))
    # the same rows through the 3-d view the strides describe
    v = o.buf[c_off:][: 3 * c_seg].reshape(3, c_seg)[:, : rps * ldc].reshape(3, rps, ldc)[:, :, :N].reshape(M, N)
    assert torch.equal(v, want.float())
    close64(r.mag, A.double().abs() @ W.double().abs().t() + b.double().abs(), 1e-13)


def test_causal_conv_and_transposed_conv_through_row_windows():
    B, T, ci, co, k = 2, 9, 4, 6, 7
    x = rnd(B, T, ci, seed=4)
    w, b = rnd(co, ci, k, seed=5), rnd(co, seed=6)
    want = F.conv1d(F.pad(F.elu(x.double()).transpose(1, 2), (k - 1, 0)), w.double(), b.double()).transpose(1, 2)
    buf = torch.zeros(B, k - 1 + T, ci)
    buf[:, k - 1:] = x
    Cb = canary(B * (2 + T) * co)
    r = G.gemm_ref(buf, pack.pack_conv1d(w), Cb, M=B * T, N=co, K=k * ci, lda=ci, bias=b, prologue=G.PRO_ELU, rows_per_seg=T,
                   a_seg_stride=(k - 1 + T) * ci, c_off=2 * co, c_seg_stride=(2 + T) * co, ldc=co)
    close64(r.out.reshape(B, T, co), want, 1e-12)
    got = r["C"].buf.reshape(B, 2 + T, co)
    assert bool(torch.isnan(got[:, :2]).all()) and torch.equal(got[:, 2:], want.float())
    for s in (4, 5, 8):
        wt, bt = rnd(ci, co, 2 * s, seed=7 + s), rnd(co, seed=8)
        y = F.conv_transpose1d(x.double().transpose(1, 2), wt.double(), bt.double(), stride=s)
        want = y[..., : y.shape[-1] - s].transpose(1, 2)
        wp, bp = pack.pack_convtr1d(wt, bt, s)
        buf = torch.zeros(B, 1 + T, ci)
        buf[:, 1:] = x
        Cb = canary(B * (2 + T * s) * co)
        r = G.gemm_ref(buf, wp, Cb, M=B * T, N=s * co, K=2 * ci, lda=ci, bias=bp, rows_per_seg=T, a_seg_stride=(1 + T) * ci,
                       c_off=2 * co, c_seg_stride=(2 + T * s) * co, ldc=s * co)
        close64(r["C"].buf.reshape(B, 2 + T * s, co)[:, 2:], want, 2.0 ** -22 * float(want.abs().max()))


def test_activations_residual_glu_and_prologues():
    M, N, K = 7, 64, 12
    A, W, b = rnd(M, K, seed=10), rnd(N, K, seed=11, scale=0.5), rnd(N, seed=12)
    pre = F.linear(A.double(), W.double(), b.double())
    Cb = canary(M * N)
    close64(G.gemm_ref(A, W, Cb, M=M, N=N, K=K, bias=b, epilogue=G.EPI_GELU).out, F.gelu(pre), 1e-14)
    close64(G.gemm_ref(A, W, Cb, M=M, N=N, K=K, bias=b, epilogue=G.EPI_TANH).out, torch.tanh(pre), 1e-14)
    r = G.gemm_ref(A, W, Cb, M=M, N=N, K=K, bias=b, c_mode=3)
    close64(r["C"].values(r["C"].buf), F.elu(pre), 2.0 ** -23 * float(pre.abs().max()))
    C2 = canary(M * N)
    r = G.gemm_ref(A, W, Cb, M=M, N=N, K=K, bias=b, c_mode=4, C2=C2)
    assert torch.equal(r["C"].buf.reshape(M, N), pre.float()) and torch.equal(r["C2"].buf.reshape(M, N), F.elu(pre).float())
    pv = rnd(K + 4, seed=13)
    pv[K:] = NAN
    close64(G.gemm_ref(A, W, Cb, M=M, N=N, K=K, bias=b, prologue=G.PRO_ADDVEC, pro_vec=pv).out,
            F.linear(A.double() + pv[:K].double(), W.double(), b.double()), 1e-13)
    # residual: other leading dimension and offset than C, a scale with a poisoned tail, then in place
    R, sc = rnd(M, N + 5, seed=14), torch.cat([rnd(N, seed=15), torch.full((3,), NAN)])
    Rb = torch.cat([canary(3), R.reshape(-1)])
    r = G.gemm_ref(A, W, Cb, M=M, N=N, K=K, bias=b, epilogue=G.EPI_RES, R=Rb, ldr=N + 5, r_off=3, scale=sc)
    close64(r.out, R[:, :N].double() + sc[:N].double() * pre, 1e-13)
    Rd = rnd(M, N, seed=16)
    r = G.gemm_ref(A, W, Rd, M=M, N=N, K=K, bias=b, epilogue=G.EPI_RES, R=Rd)
    assert torch.equal(r["C"].buf, (Rd.double() + pre).float())
    assert not torch.equal(r["C"].buf, Rd)  # a copy: the caller's buffer is left alone
    # GLU on the packed [32 value | 32 gate] pairing (pack.pack_glu)
    wp, bp = pack.pack_glu(W, b)
    Gb = canary(M * (N // 2 + 2))
    r = G.gemm_ref(A, wp, Gb, M=M, N=N, K=K, bias=bp, epilogue=G.EPI_GLU, ldc=N // 2 + 2)
    close64(r.out, pre[:, : N // 2] * torch.sigmoid(pre[:, N // 2:]), 1e-14)
    assert_owned_only(r["C"], Gb)
    assert int(r["C"].owned().sum()) == M * N // 2


def test_fused_layernorm_rmsnorm_and_rope_against_torch_and_the_oracle():
    M, N, K = 9, 16, 128
    x, W, b = rnd(M, K, seed=20, scale=3.0) + 1.5, rnd(N, K, seed=21, scale=0.1), rnd(N, seed=22)
    lw, lb = rnd(K, seed=23), rnd(K, seed=24)
    # LayerNorm: statistics pairs per 64 columns in, the norm's weight folded into W and W lnb into the bias
    stats = G.row_stats64(x).float()
    Wf, bf = W.double() * lw.double()[None, :], b.double() + W.double() @ lb.double()
    r = G.gemm_ref(x, Wf.float(), canary(M * N), M=M, N=N, K=K, bias=bf.float(), ln_stats=stats, ln_eps=1e-5)
    want = F.linear(F.layer_norm(x.double(), (K,), lw.double(), lb.double(), 1e-5), W.double(), b.double())
    close64(r.out, want, 1e-5)  # (Wf, bf and the pairs went through fp32)
    # RMSNorm: the oracle's, its weight folded into W
    nw = rnd(K, seed=25)
    r = G.gemm_ref(x, (W.double() * nw.double()[None, :]).float(), canary(M * N), M=M, N=N, K=K, bias=b, rms_eps=1e-6)
    want = F.linear(O.rmsnorm(x, nw, 1e-6).double(), W.double(), b.double())
    close64(r.out, want, 5e-6 * float(want.abs().max()))
    # rotate-half RoPE of the leading heads, positions restarting per utterance
    dh, rcols, pos0, rrps, N2 = 8, 16, 3, 4, 24
    W2, b2 = rnd(N2, K, seed=26, scale=0.1), rnd(N2, seed=27)
    cos, sin = O.rope_cos_sin(torch.arange(pos0 + rrps), dh, 10000.0)  # [positions, dh] (both halves alike)
    ct, st = cos[:, : dh // 2].contiguous(), sin[:, : dh // 2].contiguous()
    r = G.gemm_ref(x, W2, canary(M * N2), M=M, N=N2, K=K, bias=b2, epilogue=G.EPI_ROPE, rope=(ct, st, rcols, dh, pos0, rrps))
    pre = F.linear(x.double(), W2.double(), b2.double())
    pos = pos0 + torch.arange(M) % rrps
    q = pre[:, :rcols].reshape(M, rcols // dh, dh)
    rot = q * cos.double()[pos][:, None, :] + O._rot_half(q) * sin.double()[pos][:, None, :]
    close64(r.out[:, :rcols], rot.reshape(M, rcols), 1e-13)
    close64(r.out[:, rcols:], pre[:, rcols:], 0.0)


def test_argmax_partials_against_torch_argmax():
    M, N, K = 11, 200, 8
    g = torch.Generator().manual_seed(30)
    A = torch.randint(-3, 4, (M, K), generator=g).float()
    W = torch.randint(-2, 3, (N, K), generator=g).float()  # small integers: many exact ties
    C2 = torch.full((M * 5 * 2 + 4,), -7.0)
    r = G.gemm_ref(A, W, None, M=M, N=N, K=K, c_mode=5, C2=C2, ldc2=5, c2_off=2)
    o = r["C2"]
    pairs = o.buf[2: 2 + M * 5 * 2].reshape(M, 5, 2)
    vals, idx = pairs[:, :4, 0], pairs[:, :4, 1].contiguous().view(torch.int32)
    logits = A @ W.t()
    for gi in range(4):
        blk = logits[:, 64 * gi: min(N, 64 * gi + 64)]
        assert torch.equal(idx[:, gi].long(), blk.argmax(dim=1) + 64 * gi)  # first maximum
        assert torch.equal(vals[:, gi], blk.max(dim=1).values)
    # the combination of the partials is the arg-max of the row
    best = vals.max(dim=1).values
    first = torch.where(vals == best[:, None], idx.long(), torch.full_like(idx.long(), 1 << 30)).min(dim=1).values
    assert torch.equal(first, logits.argmax(dim=1))
    assert bool((pairs[:, 4] == -7.0).all()) and bool((o.buf[:2] == -7.0).all())


def test_bf16_rows_and_split_form_against_torchs_cast():
    M, N, K = 6, 36, 32
    A, W, b = rnd(M, K, seed=40), rnd(N, K, seed=41), rnd(N, seed=42)
    A16 = A.to(torch.bfloat16)
    pre = F.linear(A16.double(), W.to(torch.bfloat16).double(), b.double())
    Cb = torch.full((M * (N + 4),), NAN, dtype=torch.bfloat16)
    C2 = torch.full((M * (N + 8),), NAN, dtype=torch.bfloat16)
    r = G.gemm_ref(A16, W, Cb, M=M, N=N, K=K, bias=b, c_mode=8, C2=C2, ldc=N + 4, ldc2=N + 8, round_operands=True)
    close64(r.pre, pre, 1e-13)
    assert torch.equal(r["C"].buf.reshape(M, N + 4)[:, :N], pre.float().to(torch.bfloat16))
    assert torch.equal(r["C2"].buf.reshape(M, N + 8)[:, :N], F.elu(pre).float().to(torch.bfloat16))
    assert bool(torch.isnan(r["C"].buf.reshape(M, N + 4)[:, N:]).all())
    # fp32 rows in, rounded while they are staged: the same product
    close64(G.gemm_ref(A, W, Cb, M=M, N=N, K=K, bias=b, c_mode=6, ldc=N + 4, round_operands=True).pre, pre, 1e-13)
    # split form: round trip, then as an operand and as an output (a part-filled last group of 32 keeps its canaries)
    x = rnd(5, 64, seed=43, scale=100.0)
    s = G.to_split_form(x)
    back = G.from_split_form(s)
    assert float(((back - x.double()).abs() / x.double().abs()).max()) <= 2.0 ** -16
    hi = s.view(torch.bfloat16).reshape(5, 2, 2, 32)[:, :, 0]
    assert torch.equal(hi.reshape(5, 64), x.to(torch.bfloat16))
    As = G.to_split_form(A)
    Cs = canary(M * 64)
    r = G.gemm_ref(As, W, Cs, M=M, N=N, K=K, bias=b, a_split=True, c_mode=1, ldc=64)
    want = F.elu(F.linear(G.from_split_form(As), W.double(), b.double()))
    o = r["C"]
    assert_owned_only(o, Cs)
    assert int(o.owned().sum()) == 2 * M * N
    close64(o.values(o.buf), want, 2.0 ** -16 * float(want.abs().max()))
    dec = G.from_split_form(torch.nan_to_num(o.buf.reshape(M, 64), nan=0.0))  # whole groups of 32 decode like the gather
    close64(dec[:, :32], want[:, :32], 2.0 ** -16 * float(want.abs().max()))


def test_bf16_flip_charge_covers_every_rounding_that_a_perturbation_changes():
    """Where the charge is 0 a value within eps of x rounds to the bf16 number x rounds to; elsewhere the two roundings differ by at
    most the charge (one ulp).  Random values, values next to powers of two, and perturbations of up to the full eps either way."""
    g = torch.Generator().manual_seed(60)
    x = torch.cat([torch.randn(200000, generator=g, dtype=torch.float64) * 3,
                   (2.0 ** torch.randint(-6, 6, (50000,), generator=g).double()) * (1 + torch.randn(50000, generator=g, dtype=torch.float64) * 3e-3)])
    eps = torch.full_like(x, 3e-6) + 2.0 ** -22 * x.abs()
    ch = G.bf16_flip_charge(x, eps)
    assert 0 < int((ch > 0).sum()) < x.numel() // 20  # a small fraction, not everything
    for s in (-1.0, -0.37, 0.5, 1.0):
        diff = (G.bf16_round(x + s * eps) - G.bf16_round(x)).abs()
        # (a perturbation larger than an ulp - tiny x - moves the rounded value by itself: |delta| + one ulp; delta has its own term)
        lim = ch + torch.where(ch > 0, eps, torch.zeros_like(eps))
        assert bool((diff <= lim).all()), f"{int((diff > lim).sum())} roundings change outside the charge"


def test_ln_stats_out_is_the_statistics_of_the_written_stream():
    M, N, K = 5, 128, 8
    A, W, R = rnd(M, K, seed=50), rnd(N, K, seed=51), rnd(M, N, seed=52)
    st = canary(M * 2 * 2 + 6)
    r = G.gemm_ref(A, W, canary(M * N), M=M, N=N, K=K, epilogue=G.EPI_RES, R=R, ln_stats_out=st)
    y = r["C"].buf.reshape(M, N).double()
    got = r["ln_stats_out"].buf[: M * 4].reshape(M, 2, 2).double()
    close64(got[..., 0], y.reshape(M, 2, 64).mean(dim=2), 1e-6)
    close64(got[..., 1], y.reshape(M, 2, 64).var(dim=2, unbiased=False) * 64, 1e-4)
    mean, var = G.ln_from_pairs(got, N)
    close64(mean, y.mean(dim=1), 1e-6)
    close64(var, y.var(dim=1, unbiased=False), 1e-5)
    assert bool(torch.isnan(r["ln_stats_out"].buf[M * 4:]).all())
