"""The float64 references of tests/elementwise_ref.py against independent formulations - the oracle's layers, torch.nn.functional,
numpy - at one ordinary shape each, so that what tests/test_gpu_elementwise.py holds the kernels to is itself checked on the CPU."""
import numpy as np
import torch
import torch.nn.functional as F

import elementwise_ref as R
from oracle import sopro_oracle as O
from sopro_amd import pack

NAN = float("nan")


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def canary(n):
    return torch.full((n,), NAN, dtype=torch.float64)


def close(got, want, atol, what):
    err = float((got.double() - want.double()).abs().max())
    assert err <= atol, f"{what}: {err:.3e} > {atol:.1e}"


def test_norm_references():
    rows, C = 12, 100
    x, w, b = rnd(rows, C, seed=1).double(), (1 + 0.1 * rnd(C, seed=2)).double(), rnd(C, seed=3).double()
    o = R.norm(x.flatten(), C, 0, canary(rows * C), C, w, None, None, None, rows, rows, C, 1e-6, R.NORM_RMS)
    close(o.view(rows, C), O.rmsnorm(x, w).double(), 1e-6, "rmsnorm vs the oracle (fp32)")
    close(o.view(rows, C), x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * w, 1e-13, "rmsnorm")
    o = R.norm(x.flatten(), C, 0, canary(rows * C), C, w, b, None, None, rows, rows, C, 1e-5, R.NORM_LN)
    close(o.view(rows, C), F.layer_norm(x, (C,), w, b, 1e-5), 1e-13, "layernorm")
    # strides, offsets, segments and FiLM together: 4 segments of 3 rows behind 2 pad rows each, rows ldx apart, output ldo apart
    ldx, ldo = C + 8, C + 4
    buf = torch.full((4, 5, ldx), 7.0, dtype=torch.float64)
    buf[:, 2:, :C] = x.view(4, 3, C)
    mul, add = rnd(4, C, seed=4).double(), rnd(4, C, seed=5).double()
    o = R.norm(buf.flatten(), ldx, 5 * ldx, canary(3 + rows * ldo), ldo, w, b, mul.flatten(), add.flatten(), rows, 3, C, 1e-5, R.NORM_LN,
               x_off=2 * ldx, o_off=3)
    want = F.layer_norm(x, (C,), w, b, 1e-5).view(4, 3, C) * mul[:, None] + add[:, None]
    got = o[3:].view(rows, ldo)
    close(got[:, :C], want.reshape(rows, C), 1e-13, "layernorm + film, segmented")
    assert bool(torch.isnan(got[:, C:]).all()) and bool(torch.isnan(o[:3]).all())
    # the fp32 evaluation of the same code is fp32-close: the yardstick of the tolerance
    o32 = R.norm(x.flatten(), C, 0, canary(rows * C), C, w, b, None, None, rows, rows, C, 1e-5, R.NORM_LN, dt=torch.float32)
    o64 = R.norm(x.flatten(), C, 0, canary(rows * C), C, w, b, None, None, rows, rows, C, 1e-5, R.NORM_LN)
    assert o32.dtype == torch.float32 and 0 < R.tolerance(o64, o32) < 2e-5


def test_tolerance_is_four_times_the_larger_of_the_fp32_error_and_the_floor():
    r64 = torch.tensor([1.0, -8.0, NAN], dtype=torch.float64)
    assert R.tolerance(r64, r64.float()) == 4 * 4 * 2.0 ** -24 * 8.0
    r32 = torch.tensor([1.0, -8.0 + 1e-4, NAN])
    assert abs(R.tolerance(r64, r32) - 4 * abs(float(r32[1]) + 8.0)) < 1e-12


def test_row_scalings_and_pools():
    rows, C = 6, 65
    a, x = rnd(rows, C, seed=6, scale=3.0).double(), rnd(rows, C, seed=7).double()
    a[1] *= 1e-3  # ratio above 10: clamped
    a[2] = 0.0
    rms = lambda t: torch.sqrt(t.pow(2).mean(-1, keepdim=True) + 1e-6)  # noqa: E731
    o = R.rms_match(a.flatten(), x.flatten(), canary(rows * C + 2), rows, C)
    close(o[:-2].view(rows, C), a * torch.clamp(rms(x) / rms(a), 0, 10), 1e-13, "rms_match")
    assert float(rms(x)[1] / rms(a)[1]) > 10 and bool(torch.isnan(o[-2:]).all()) and bool((o[2 * C: 3 * C] == 0).all())
    e = rnd(rows, C, seed=8).double()
    e[3] = 0.0
    e[4] *= 1e-9
    o = R.l2norm(e.flatten(), canary(rows * C), rows, C, 1e-6)
    close(o.view(rows, C), F.normalize(e, dim=-1, eps=1e-6), 1e-13, "l2norm")
    o = R.tanh_affine(x.flatten(), canary(rows * C), 1.0, 1.2, rows * C - 1)
    close(o[:-1], torch.from_numpy(1.0 + 1.2 * np.tanh(x.flatten()[:-1].numpy())), 1e-13, "tanh_affine")
    assert bool(torch.isnan(o[-1]))
    pe = rnd(32, C, seed=31).double()
    o = R.add_pos(x[:3].flatten(), pe.flatten(), canary(3 * 20 * C), 3, 20, C, 5)
    close(o.view(3, 20, C), x[:3, None] + pe[None, 5:25], 0.0, "add_pos")
    B, T = 4, 11
    xm, lens = rnd(B, T, C, seed=9).double(), torch.tensor([11, 4, 0, 14], dtype=torch.int32)
    o = R.masked_mean(xm.flatten(), lens, canary(B * C), B, T, C)
    want = torch.stack([xm[i, : min(int(lens[i]), T)].sum(0) / (min(int(lens[i]), T) + 1e-6) for i in range(B)])
    close(o.view(B, C), want, 1e-13, "masked_mean")
    close(R.masked_mean(xm.flatten(), None, canary(B * C), B, T, C).view(B, C), xm.sum(1) / (T + 1e-6), 1e-13, "masked_mean, no lens")
    lg, lens = rnd(B, T, seed=10, scale=30.0).double(), torch.tensor([11, 4, 1, 14], dtype=torch.int32)
    o = R.stats_pool(xm.flatten(), lg.flatten(), lens, canary(B * 2 * C), B, T, C).view(B, 2 * C)
    for i in range(B):  # the module's own form: masked_fill(-1e9), softmax, weighted moments
        n = min(int(lens[i]), T)
        lw = lg[i].clone()
        lw[n:] = -1e9
        aw = torch.from_numpy(np.exp(lw.numpy() - lw.numpy().max()))
        aw = (aw / aw.sum())[:, None]
        mu = (aw * xm[i]).sum(0)
        sd = torch.sqrt((aw * (xm[i] - mu).pow(2)).sum(0).clamp_min(1e-6))
        close(o[i], torch.cat([mu, sd]), 1e-12, f"stats_pool row {i}")
    close(o[2, C:], torch.full((C,), 1e-3, dtype=torch.float64), 1e-15, "stats_pool: one frame -> the floor under the root")


def test_dwconv_reference():
    B, T, C = 3, 50, 8
    for ksize, dil, causal in [(7, 1, False), (11, 8, False), (13, 4, True)]:
        x, wt, b, res = (t.double() for t in (rnd(B, T, C, seed=11), rnd(C, 1, ksize, seed=12), rnd(C, seed=13), rnd(B, T, C, seed=14)))
        total = (ksize - 1) * dil
        left = total if causal else total // 2
        conv = O.dwconv_full(x, wt, b, dil, causal)
        args = (x.flatten(), pack.pack_dw(wt).flatten(), b, res.flatten(), canary(B * T * C))
        close(R.dwconv(*args, None, B, T, C, ksize, dil, left, 0).view(B, T, C), conv, 1e-13, "dwconv")
        close(R.dwconv(*args, None, B, T, C, ksize, dil, left, 1).view(B, T, C), conv + res, 1e-13, "dwconv + res")
        close(R.dwconv(*args, None, B, T, C, ksize, dil, left, 2).view(B, T, C), F.gelu(conv), 1e-13, "dwconv + gelu")
        lens = [50, 17, 0]
        o = R.dwconv(*args, torch.tensor(lens, dtype=torch.int32), B, T, C, ksize, dil, left, 0).view(B, T, C)
        for i, n in enumerate(lens):  # an utterance cut to its own length, as a call of its own
            if n:
                close(o[i, :n], O.dwconv_full(x[i: i + 1, :n], wt, b, dil, causal)[0], 1e-13, f"dwconv ragged {i}")
        close(o[2], b.expand(T, C), 0.0, "dwconv of an empty utterance is the bias")


def test_gather_references():
    V, Q, D, rows = 50, 6, 8, 7
    table = rnd(Q * V + 1, D, seed=15).double()
    tok = torch.randint(0, V, (rows, Q), generator=torch.Generator().manual_seed(16), dtype=torch.int32)
    tok[2, 0], tok[3, 4] = -1, V + 5  # below the table; past its end with the last offset
    cols = [0, 3, 4]
    col, off = torch.tensor(cols, dtype=torch.int32), torch.tensor([0, 3 * V, (Q - 1) * V], dtype=torch.int32)
    wq, base = torch.softmax(rnd(3, seed=17), 0).double(), rnd(rows, D, seed=18).double()
    o = R.codebook_sum(tok.flatten(), Q, col, off, wq, 3, table.flatten(), Q * V + 1, base.flatten(), 0.3, 0.7, canary(rows * D), D, 0,
                       rows, rows, D)
    want = 0.3 * base
    for r in range(rows):
        for j, c in enumerate(cols):
            want[r] += 0.7 * wq[j] * table[min(max(int(off[j]) + int(tok[r, c]), 0), Q * V)]
    close(o.view(rows, D), want, 1e-13, "codebook_sum")
    ids = torch.randint(-3, 60, (2, 9), generator=torch.Generator().manual_seed(19), dtype=torch.int32)
    tt, pe = rnd(50, D, seed=20).double(), pack.sinusoid_table(16, D).double()
    o = R.text_embed(ids.flatten(), torch.tensor([9, 5], dtype=torch.int32), tt.flatten(), 50, pe.flatten(), canary(2 * 9 * D), 2, 9, D)
    want = tt[torch.from_numpy(np.clip(ids.numpy(), 0, 49)).long()] + pe[None, :9]
    want[1, 5:] = 0
    close(o.view(2, 9, D), want, 0.0, "text_embed")


def test_argmax_reference_contract():
    rows, N, ldx = 7, 130, 134
    g = torch.Generator().manual_seed(21)
    x = torch.randint(0, 3, (rows, ldx), generator=g).float()
    out = torch.full((3 * 5,), -7, dtype=torch.int32)
    o = R.argmax_rows(x.flatten(), ldx, out, 5, 3, rows, N)
    want = np.argmax(x[:, :N].numpy(), axis=1)  # numpy: the first of equal maxima
    for r in range(rows):
        assert int(o[(r // 3) * 5 + r % 3]) == int(want[r])
    assert int((o == -7).sum()) == 15 - rows
    x = torch.full((4, 8), float("-inf"))
    x[1, 2], x[1, 5] = NAN, 3.0  # a NaN before the maximum is skipped
    x[2] = NAN  # no non-NaN entry: 0
    x[3, 6], x[3, 7] = 1.0, 1.0
    o = R.argmax_rows(x.flatten(), 8, torch.full((4,), -7, dtype=torch.int32), 1, 1, 4, 8)
    assert o.tolist() == [0, 5, 0, 6]


def test_rope_upsample_final_conv_references():
    H, dh, rps, B = 2, 8, 5, 3
    x = rnd(B * rps, 3 * H * dh, seed=22).double()
    c, s = pack.rope_tables(16, dh, 10000.0)
    o = R.rope(x.flatten(), 3 * H * dh, c.flatten(), s.flatten(), B * rps, rps, 7, H, dh, x_off=H * dh).view(B * rps, -1)
    cos, sin = O.rope_cos_sin(torch.arange(rps) + 7, dh, 10000.0)
    kk = O._heads(x[:, H * dh: 2 * H * dh].reshape(B, rps, H * dh), H)
    want = O._unheads(kk * cos.double() + O._rot_half(kk) * sin.double()).reshape(B * rps, H * dh)
    close(o[:, H * dh: 2 * H * dh], want, 1e-13, "rope")
    assert torch.equal(o[:, : H * dh], x[:, : H * dh]) and torch.equal(o[:, 2 * H * dh:], x[:, 2 * H * dh:])
    T, C = 9, 6
    xu, wu = rnd(B, T, C, seed=23).double(), rnd(C, 1, 4, seed=24).double()
    want = O.causal_convtr1d(xu.transpose(1, 2), wu, None, 2, groups=C).transpose(1, 2)
    seg = (3 + 2 * T) * C + 5
    o = R.upsample2(xu.flatten(), wu.flatten(), canary(B * seg), seg, B, T, C, y_off=3 * C)
    got = torch.stack([o[i * seg + 3 * C: i * seg + (3 + 2 * T) * C] for i in range(B)]).view(B, 2 * T, C)
    close(got, want, 1e-13, "upsample2")
    assert int(torch.isnan(o).sum()) == B * seg - B * 2 * T * C
    Tn = 40
    h, wf, bf = rnd(B, Tn, 64, seed=25).double(), rnd(1, 64, 3, seed=26, scale=0.1).double(), 0.05
    want = O.causal_conv1d(F.elu(h).transpose(1, 2), wf, torch.tensor([bf], dtype=torch.float64))[:, 0]
    hb = torch.zeros(B, 2 + Tn + 1, 64, dtype=torch.float64)
    hb[:, 2: 2 + Tn] = h
    hb[:, 2 + Tn:] = 9.0  # a row past the segment's frames is not read
    o = R.final_conv(hb.flatten(), (3 + Tn) * 64, wf[0].t().contiguous().flatten(), bf, canary(B * (Tn + 3)), Tn + 3, B, Tn)
    close(o.view(B, Tn + 3)[:, :Tn], want, 1e-13, "final conv")
    assert bool(torch.isnan(o.view(B, Tn + 3)[:, Tn:]).all())


def test_word_references():
    p = torch.full((40,), -7, dtype=torch.int32)
    o = R.fill2d(p, 9, 3, 5, 123)
    assert o.view(-1)[:27].view(3, 9)[:, :5].eq(123).all() and int((o == -7).sum()) == 40 - 15
    src = torch.arange(30, dtype=torch.int32)
    o = R.copy2d(p, 9, src, 7, 3, 5)
    assert torch.equal(o[:27].view(3, 9)[:, :5], src[:21].view(3, 7)[:, :5]) and int((o == -7).sum()) == 40 - 15
    B, T, Q, bs, vmax = 3, 5, 4, 9, 2047
    cb0 = torch.randint(0, vmax + 1, (B * bs,), generator=torch.Generator().manual_seed(27), dtype=torch.int32)
    cb0[:4] = torch.tensor([-2, 0, vmax, vmax + 1], dtype=torch.int32)
    o = R.nar_seed(torch.full((B * T * Q,), -7, dtype=torch.int32), Q, cb0, bs, B, T, vmax).view(B, T, Q)
    assert torch.equal(o[..., 0], torch.from_numpy(np.clip(cb0.view(B, bs)[:, :T].numpy(), 0, vmax)))
    assert o[0, :4, 0].tolist() == [0, 0, vmax, vmax] and bool((o[..., 1:] == -7).all())


def test_bf16_rounding_reference():
    g = torch.Generator().manual_seed(28)
    v = torch.cat([rnd(4096, seed=29) * torch.exp(rnd(4096, seed=30) * 8),
                   R.bits_f32(torch.randint(0x00800000, 0x7F800000, (4096,), generator=g)),  # every normal exponent
                   R.bits_f32(torch.tensor([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3FFF8000, 0x7F7FFFFF, 0x7F7F7FFF,
                                            0x00000000, 0x80000000, 0x7F800000, 0xFF800000]))])
    bits = R.cvt_f32_bf16_bits(v, v.numel())
    want = v.to(torch.bfloat16).view(torch.int16).long() & 0xFFFF
    assert torch.equal(bits, want)
    assert bits[-11:].tolist() == [0x3F80, 0x3F82, 0x3F80, 0x3F81, 0x4000, 0x7F80, 0x7F7F, 0x0000, 0x8000, 0x7F80, 0xFF80]
    nan = R.cvt_f32_bf16_bits(torch.tensor([NAN, -NAN]), 2)
    assert bool(torch.isnan(R.cvt_bf16_f32(nan, 2)).all())
    back = R.cvt_bf16_f32(bits, bits.numel())
    assert torch.equal(back, v.to(torch.bfloat16).float())
    assert torch.equal(R.cvt_f32_bf16_bits(back, back.numel()), bits)  # the round trip is exact
