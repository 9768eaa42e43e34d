"""The float64 reference of the AR-step contraction (tests/skinny_ref.py) against independent formulations: F.linear, the oracle's
RMSNorm and GLU, F.gelu, torch.tanh, torch's bf16 cast, and - for the ring - a whole sequence of frames against one causal dilated
depthwise F.conv1d over that sequence.  CPU only."""
import pytest
import torch
import torch.nn.functional as F

import skinny_ref as S
from oracle import sopro_oracle as O

NAN = float("nan")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def canary(n, dtype=torch.float32):
    return torch.full((n,), NAN, dtype=dtype)


def close64(a, b, tol):
    err = float((a.double() - b.double()).abs().max())
    assert err <= tol * max(1.0, float(b.double().abs().max())), err


def rows_into(vals, ld, lead=0, tail=0):
    """[B, n] values as rows `ld` apart in a NaN buffer."""
    Bn, n = vals.shape
    buf = canary(lead + Bn * ld + tail)
    buf[lead + torch.arange(Bn)[:, None] * ld + torch.arange(n)[None, :]] = vals
    return buf[lead:] if lead else buf


@pytest.mark.parametrize("K", [384, 1152])
def test_plain_form_against_linear_and_the_activations(K):
    B, N = 5, 19
    g = gen(K)
    x, W, b = torch.randn(B, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g)
    ldx, ldw, ldy, ldr = K + 8, K + 4, N + 3, N + 6
    Xb, Wb, Yb = rows_into(x, ldx), rows_into(W, ldw), canary(B * ldy + 5)
    pre = F.linear(x.double(), W.double(), b.double())
    kw = dict(B=B, N=N, K=K, ldx=ldx, ldw=ldw, ldy=ldy, bias=b)
    r = S.skinny_ref(Xb, Wb, Yb, **kw)
    close64(r["Y"].ref, pre, 1e-13)
    own = r.owned("Y")
    assert int(own.sum()) == B * N and bool(torch.isnan(r.bufs["Y"][~own]).all())
    assert torch.equal(r["Y"].values(r.bufs["Y"]), pre.float().double())
    close64(S.skinny_ref(Xb, Wb, Yb, epilogue=S.EPI_GELU, **kw)["Y"].ref, F.gelu(pre), 1e-13)
    close64(S.skinny_ref(Xb, Wb, Yb, epilogue=S.EPI_TANH, **kw)["Y"].ref, torch.tanh(pre), 1e-13)
    R, sc = torch.randn(B, N, generator=g), torch.randn(N, generator=g)
    r = S.skinny_ref(Xb, Wb, Yb, epilogue=S.EPI_RES, R=rows_into(R, ldr), ldr=ldr, scale=sc, **kw)
    close64(r["Y"].ref, R.double() + sc.double() * pre, 1e-13)
    Yin = rows_into(R, ldy, tail=5)  # in place
    r = S.skinny_ref(Xb, Wb, Yin, epilogue=S.EPI_RES, R=Yin, ldr=ldy, **kw)
    close64(r["Y"].ref, R.double() + pre, 1e-13)
    # magnitudes
    mag, parts = S.skinny_mag(x, W, b)
    close64(mag, x.double().abs() @ W.double().abs().t() + b.double().abs(), 1e-13)
    assert len(parts) == K // 384
    close64(r["Y"].pmag, sum(parts), 1e-13)


def test_k_slices_sum_to_the_whole_and_slice_0_carries_bias_and_residual():
    B, N, K = 3, 17, 1536
    g = gen(1)
    x, W, b, R = torch.randn(B, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g), torch.randn(B, N, generator=g)
    ldy, yps = N + 1, B * (N + 1) + 7
    Yb = canary(4 * yps)
    r = S.skinny_ref(x, W, Yb, B=B, N=N, K=K, ldy=ldy, bias=b, epilogue=S.EPI_RES, R=R, ksplit=1, y_part_stride=yps)
    assert [o.name for o in r.outs] == ["Y0", "Y1", "Y2", "Y3"]
    close64(sum(o.ref for o in r.outs), R.double() + F.linear(x.double(), W.double(), b.double()), 1e-13)
    for s in range(1, 4):
        close64(r[f"Y{s}"].ref, x[:, s * 384:(s + 1) * 384].double() @ W[:, s * 384:(s + 1) * 384].double().t(), 1e-13)
        assert int(r[f"Y{s}"].idx[0, 0]) == s * yps
    assert int(r.owned("Y").sum()) == 4 * B * N
    r0 = S.skinny_ref(x, W, Yb, B=B, N=N, K=K, ldy=ldy, ksplit=1, y_part_stride=yps)  # EPI_NONE: raw partial sums
    close64(sum(o.ref for o in r0.outs), x.double() @ W.double().t(), 1e-13)
    # ksplit = 1 at K = 384 is the unsplit call
    r1 = S.skinny_ref(x, W, Yb, B=B, N=N, K=384, ldx=K, ldw=K, ldy=ldy, bias=b, ksplit=1, y_part_stride=yps)
    assert [o.name for o in r1.outs] == ["Y"]


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
def test_rmsnorm_partial_sums_and_bf16_operands_against_the_oracle(eps):
    B, N, K = 6, 21, 384
    g = gen(2)
    parts = torch.randn(4, B, K, generator=g)
    parts[1:] *= 50.0
    parts[3] = -(parts[1] + parts[2]) + 0.01 * torch.randn(B, K, generator=g)  # large parts that cancel: the order matters
    nw, W, b = 1 + 0.1 * torch.randn(K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g)
    Wf = (W.double() * nw.double()[None, :]).float()
    xin = ((parts[0] + parts[1]) + parts[2]) + parts[3]
    assert not torch.equal(xin, parts.double().sum(0).float())  # (the fp32 order is not the exact sum)
    Yb = canary(B * N)
    kw = dict(B=B, N=N, K=K, bias=b, Xp=parts[1:], np_=3, xp_stride=B * K)
    r = S.skinny_ref(parts[0], Wf, Yb, rms_norm=True, eps=eps, **kw)
    assert torch.equal(r.xin, xin)
    close64(r["Y"].ref, F.linear(O.rmsnorm(xin.double(), nw.double(), eps).double() * 1.0, W.double(), b.double()), 2e-6)  # (the oracle works in fp32)
    want = F.linear(xin.double() * torch.rsqrt((xin.double() ** 2).mean(-1, keepdim=True) + eps), Wf.double(), b.double())
    close64(r["Y"].ref, want, 1e-9)
    close64(S.skinny_ref(parts[0], Wf, Yb, **kw)["Y"].ref, F.linear(xin.double(), Wf.double(), b.double()), 1e-13)
    # bf16 operands: torch's cast of both; the row scale still from the unrounded rows
    r16 = S.skinny_ref(parts[0], Wf, Yb, rms_norm=True, eps=eps, w_layout=2, **kw)
    x16, w16 = xin.to(torch.bfloat16).double(), Wf.to(torch.bfloat16).double()
    close64(r16["Y"].ref, (x16 @ w16.t()) * torch.rsqrt((xin.double() ** 2).mean(-1, keepdim=True) + eps) + b.double(), 1e-9)
    # a zero row: rs = rsqrt(eps), the output is the bias
    z = torch.zeros(1, K)
    rz = S.skinny_ref(z, Wf, canary(N), B=1, N=N, K=K, bias=b, rms_norm=True, eps=eps)
    assert torch.equal(rz["Y"].ref, b.double()[None, :]) and abs(float(rz.rs[0]) * eps ** 0.5 - 1) < 1e-6


def test_aux_set_flags():
    B, N, K, Na = 4, 32, 384, 32
    g = gen(3)
    x, W, Wa = torch.randn(B, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(Na, K, generator=g) * K ** -0.5
    b, ba = torch.randn(N, generator=g), torch.randn(Na, generator=g)
    rsx = x.double() * torch.rsqrt((x.double() ** 2).mean(-1, keepdim=True) + 1e-6)
    for flags in range(4):
        r = S.skinny_ref(x, W, canary(B * N), B=B, N=N, K=K, bias=b, epilogue=S.EPI_GELU, rms_norm=True, aux_W=Wa, aux_tiles=2,
                         aux_bias=ba, aux_Y=canary(B * (Na + 4)), aux_ldy=Na + 4, aux_flags=flags)
        close64(r["Y"].ref, F.gelu(F.linear(rsx, W.double(), b.double())), 1e-9)
        pre = F.linear(x.double() if flags & 1 else rsx, Wa.double(), ba.double())
        close64(r["aux"].ref, pre if flags & 2 else F.gelu(pre), 1e-9)
        assert int(r.owned("aux_Y").sum()) == B * Na


def _glu_frames(ksize, dil, T, B, ring_bcap, seed, D=384):
    g = gen(seed)
    L = (ksize - 1) * dil + 1
    nw = 1 + 0.1 * torch.randn(D, generator=g)
    W, b = torch.randn(2 * D, D, generator=g) * D ** -0.5, torch.randn(2 * D, generator=g)
    dw_w, dw_b = torch.randn(ksize, D, generator=g), torch.randn(D, generator=g)
    xs = torch.randn(T, B, D, generator=g)
    return L, nw, W, b, dw_w, dw_b, xs


@pytest.mark.parametrize("ksize,dil", [(13, 1), (13, 2), (12, 3), (7, 5), (3, 2), (2, 1), (1, 1), (1, 3)])
def test_ring_frames_against_one_causal_dilated_depthwise_convolution(ksize, dil):
    D, B, bcap = 384, 3, 5
    L, nw, W, b, dw_w, dw_b, xs = _glu_frames(ksize, dil, 0, B, bcap, 10 * ksize + dil)
    T = 2 * L + 3
    xs = torch.randn(T, B, D, generator=gen(7))
    Wf = (W.double() * nw.double()[None, :]).float()
    ring = torch.zeros(L * bcap * D)
    ring.view(L, bcap, D)[:, B:] = NAN
    hs, ys = [], []
    for t in range(T):
        r = S.skinny_ref(xs[t], Wf, canary(B * D), B=B, N=2 * D, K=D, bias=b, epilogue=S.EPI_GLU_DW, rms_norm=True, ring=ring, dw_w=dw_w,
                         dw_b=dw_b, step=t, ring_len=L, ring_bcap=bcap, dil=dil, ksize=ksize)
        own = r.owned("ring")
        assert int(own.sum()) == B * D and torch.equal(r.bufs["ring"].view(torch.int32)[~own], ring.view(torch.int32)[~own])
        hs.append(r.glu["h"])
        ys.append(r["Y"].ref - xs[t].double())
        ring = r.bufs["ring"]  # (h rounded to fp32: what the next frame reads)
    h = torch.stack(hs)                                                  # [T, B, D]
    want_h = O.glu(O.rmsnorm(xs.double(), nw.double()).double(), {"g.pro.weight": W.double(), "g.pro.bias": b.double()}, "g")
    close64(h, want_h, 2e-6)                                             # (the oracle's RMSNorm works in fp32)
    conv = F.conv1d(F.pad(h.float().double().permute(1, 2, 0), ((ksize - 1) * dil, 0)), dw_w.double().t().reshape(D, 1, ksize), dw_b.double(),
                    dilation=dil, groups=D).permute(2, 0, 1)             # [T, B, D]
    # the newest tap is the unrounded h, the older ones were rounded to fp32 when they were written
    conv = conv + (h - h.float().double()) * dw_w.double()[ksize - 1][None, None, :]
    close64(torch.stack(ys), conv, 1e-12)


def test_bf16_ring_holds_torchs_cast_and_taps_are_widened():
    D, B, ksize, dil = 384, 2, 3, 2
    L, nw, W, b, dw_w, dw_b, _ = _glu_frames(ksize, dil, 0, B, B, 5)
    x = torch.randn(B, D, generator=gen(6))
    ring = torch.randn(L * B * D, generator=gen(8)).to(torch.bfloat16)
    r = S.skinny_ref(x, W, canary(B * D), B=B, N=2 * D, K=D, bias=b, epilogue=S.EPI_GLU_DW, rms_norm=True, ring=ring, dw_w=dw_w, dw_b=dw_b,
                     step=4, ring_len=L, ring_bcap=B, dil=dil, ksize=ksize, ring_format=1, w_layout=2)
    slot = 4 % L
    assert torch.equal(r.bufs["ring"].view(L, B, D)[slot], r.glu["h"].float().to(torch.bfloat16))
    old = ring.view(L, B, D).double()
    y = old[(4 + 1) % L] * dw_w[0].double() + old[(4 + 1 + dil) % L] * dw_w[1].double() + r.glu["h"] * dw_w[2].double() + dw_b.double()
    close64(r.glu["y"], y, 1e-13)


@pytest.mark.parametrize("N,K,glu", [(1, 32, False), (17, 64, False), (33, 384, False), (8, 32, True), (18, 64, True), (40, 32, True)])
def test_packed_image_is_a_permutation_of_the_rows_with_zero_padding(N, K, glu):
    ldw = K + 4
    W = torch.randn(N, K, generator=gen(N + K))
    Wb = rows_into(W, ldw)
    img = S.pack_skinny_ref(Wb, ldw, N, K, glu, False)
    assert img.numel() == S.skinny_packed_floats(N, K, glu)
    assert float(img.double().sum() - 0) == pytest.approx(float(W.double().sum()), abs=1e-3) and int((img != 0).sum()) == int((W != 0).sum())
    # one element by the header's words: tile t, chunk c, half, lane, e
    D = N // 2
    for (t, c, half, lane, e) in [(0, 0, 0, 0, 0), (0, K // 32 - 1, 1, 63, 3), ((D + 7) // 8 - 1 if glu else (N + 15) // 16 - 1, 0, 1, 17, 2), (0, 0, 0, 9, 1)]:
        i, gq = lane & 15, lane >> 4
        row = (t * 8 + (i & 7) + (D if i >= 8 else 0)) if glu else t * 16 + i
        ok = (t * 8 + (i & 7) < D) if glu else row < N
        k = 32 * c + 8 * gq + 4 * half + e
        got = float(img[(((t * (K // 32) + c) * 2 + half) * 64 + lane) * 4 + e])
        assert got == (float(W[row, k]) if ok else 0.0)
    i16 = S.pack_skinny_ref(Wb, ldw, N, K, glu, True)
    assert i16.dtype == torch.bfloat16 and i16.numel() == img.numel()
    # the bf16 image is the cast of the fp32 image with the two halves of a lane side by side
    v = img.reshape(-1, 2, 64, 4).permute(0, 2, 1, 3).reshape(-1)
    assert torch.equal(i16, v.to(torch.bfloat16))
