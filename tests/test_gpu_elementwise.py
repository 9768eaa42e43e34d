"""Edge shapes of the row / elementwise kernels of sopro_amd/csrc/elementwise.hip against the float64 references of
tests/elementwise_ref.py (checked on the CPU by tests/test_elementwise_ref.py).

Every test fills its output with a canary (NaN; -7 for integer outputs), gives every leading dimension and segment stride some slack
and asserts (a) the words the operation owns match the reference and (b) every other word is still the canary - an out-of-bounds
write is a failed assertion.  Inputs stay inside the entry points' contracts (tables cover pos0 + rows, padded rows exist where a
kernel reads them): the limits without an API check are not probed.

Float tolerances are computed, not chosen: ``R.tolerance`` = 4 * max(e32, 4 * 2^-24 * max|ref|), e32 = the error of the same formula
evaluated in fp32 by torch on the CPU against its float64 evaluation on the same inputs.  The factor 4 covers the other summation
order (lane-strided partial sums and a shuffle tree) and device rsqrtf / expf / tanhf / __expf being good to a few ulp rather than
correctly rounded.  Integer and copy results are exact.  Each comparison prints ``EDGE-RATIO <op> <error / tolerance>`` before it
asserts; profiles/elementwise_edges.md keeps the worst value per kernel of the first run.

Kernels of the file covered elsewhere (tests/test_gpu_ops.py unless named): argmax_partials_kernel -
test_argmax_partials_order_free_reduction and test_gemm_argmax_epilogue_equals_argmax_of_the_logits; fir1_kernel -
tests/test_gpu_encode.py::test_fir1_matches_conv1d; rvq_assign_kernel -
tests/test_gpu_encode.py::test_rvq_assign_matches_argmin_and_updates_residual; row_stats_kernel -
test_gemm_fused_layernorm_equals_norm_followed_by_the_contraction (its rejection of C % 64 != 0 is checked here).  The stream_batch_*
pair at the end of the file belongs to tests/test_gpu_stream_batch.py."""
import pytest
import torch

import elementwise_ref as R
from sopro_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
F32 = torch.float32


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def i32(v):
    return torch.tensor(v, dtype=torch.int32)


def canary(n):
    return torch.full((int(n),), NAN)


def icanary(n):
    return torch.full((int(n),), -7, dtype=torch.int32)


def check(op, what, got, ref64, ref32, factor=4.0):
    """the words the reference wrote are within the computed tolerance; every other word is still NaN"""
    g = got.detach().cpu().double().flatten()
    used = ~torch.isnan(ref64)
    assert g.numel() == ref64.numel() and bool(used.any())
    assert bool(torch.isnan(g[~used]).all()), f"{op} {what}: a word outside the output lost its canary"
    assert bool(torch.isfinite(g[used]).all()), f"{op} {what}: an output word was not written (or is not finite)"
    tol = R.tolerance(ref64, ref32, factor)
    err = float((g[used] - ref64[used]).abs().max())
    print(f"EDGE-RATIO {op} {err / tol if tol else 0.0:.4f}  ({what}: err {err:.3e}, tol {tol:.3e})")
    assert err <= tol, f"{op} {what}: max abs err {err:.3e} > {tol:.3e}"


def check_int(op, what, got, ref):
    g = got.detach().cpu().flatten()
    assert g.dtype == ref.dtype and torch.equal(g, ref), f"{op} {what}: {(g != ref).nonzero().flatten().tolist()[:8]} differ"


def both(fn, *args, **kw):
    return fn(*args, **kw), fn(*args, **kw, dt=F32)


# ------------------------------------------------------------------------------------------------ norm
def _norm_case(kind, C, rows, *, mean=0.0, film=False, seed=0):
    ldx, ldo = C + 8, C + 4
    rps, nseg = (2, (rows + 1) // 2) if film else (rows, 1)
    x_off, seg = (2 * ldx, (rps + 2) * ldx + 12) if film else (0, 0)
    x = rnd(x_off + nseg * (seg if seg else rows * ldx) + 8, seed=seed) + mean  # the slack holds numbers too: a leak moves the result
    w = 1 + 0.1 * rnd(C, seed=seed + 1)
    b = rnd(C, seed=seed + 2) if kind == hip.NORM_LN else None
    mul, add = (rnd(nseg, C, seed=seed + 3), rnd(nseg, C, seed=seed + 4)) if film else (None, None)
    eps = 1e-5 if kind == hip.NORM_LN else 1e-6
    out = canary(3 + rows * ldo + 5)
    od = dev(out)
    hip.norm(dev(x), od, dev(w), rows=rows, C_=C, eps=eps, kind=kind, b=dev(b), mul=dev(mul), add=dev(add), rows_per_seg=rps, ldx=ldx,
             ldo=ldo, x_off=x_off, o_off=3, x_seg_stride=seg)
    r64, r32 = both(R.norm, x, ldx, seg, out, ldo, w, b, None if mul is None else mul.flatten(), None if add is None else add.flatten(),
                    rows, rps, C, eps, kind, x_off=x_off, o_off=3)
    check("norm", f"kind {kind} C {C} rows {rows} mean {mean} film {film}", od, r64, r32)


@pytest.mark.parametrize("C", [1, 63, 64, 65, 100, 1000, 1024])
@pytest.mark.parametrize("kind", [hip.NORM_RMS, hip.NORM_LN])
def test_norm_widths_rows_and_leading_dimensions(kind, C):
    """C below, at and past a multiple of the 64 lanes, up to the 16-per-lane limit; 1, 3, 5 rows (4 per workgroup); ldx = C + 8,
    ldo = C + 4: a padding lane that leaks into the mean or variance, or a row written at the wrong pitch, fails here"""
    for rows in (1, 3, 5):
        _norm_case(kind, C, rows, seed=100 + C + rows)


def test_norm_layernorm_of_a_row_far_from_zero():
    """row mean 50, unit spread: the variance has to be taken about the mean"""
    _norm_case(hip.NORM_LN, 384, 5, mean=50.0, seed=7)


def test_norm_film_with_a_segmented_source():
    """FiLM mul / add per segment together with x_off, x_seg_stride and rows_per_seg = 2, at C = 100 (5 rows: the last segment is short)"""
    _norm_case(hip.NORM_LN, 100, 5, film=True, seed=8)
    _norm_case(hip.NORM_RMS, 100, 6, film=True, seed=9)


# ------------------------------------------------------------------------------------------------ rms_match, l2norm
@pytest.mark.parametrize("C", [1, 65, 384])
def test_rms_match_below_above_the_clamp_and_zero_rows(C):
    rows = 6
    a, x = rnd(rows, C, seed=10 + C, scale=3.0), rnd(rows, C, seed=11 + C)
    x[0] *= 5.0   # ratio about 1.7: not clamped
    a[1] *= 1e-3  # ratio about 300: clamped to 10
    a[2] = 0.0    # rms(a) = 1e-3: clamped, and the row stays zero
    x[3] = 0.0    # ratio about 3e-4
    rms = lambda t: torch.sqrt(t.double().pow(2).mean(-1) + 1e-6)  # noqa: E731
    ratio = rms(x) / rms(a)
    assert float(ratio[0]) < 10 < float(ratio[1]) and float(ratio[2]) > 10
    out = canary(rows * C + 7)
    od = dev(out)
    hip.rms_match(dev(a), dev(x), od, rows, C)
    check("rms_match", f"C {C}", od, *both(R.rms_match, a.flatten(), x.flatten(), out, rows, C))
    assert bool((od[2 * C: 3 * C] == 0).all())


@pytest.mark.parametrize("C", [1, 65, 192])
def test_l2norm_zero_row_and_norm_below_eps(C):
    rows = 5
    e = rnd(rows, C, seed=20 + C)
    e[1] = 0.0
    e[3] *= 1e-9  # norm about 1e-8 < eps: divided by eps
    out = canary(rows * C + 7)
    od = dev(out)
    hip.l2norm(dev(e), od, rows, C, 1e-6)
    check("l2norm", f"C {C}", od, *both(R.l2norm, e.flatten(), out, rows, C, 1e-6))
    assert bool((od[C: 2 * C] == 0).all())


# ------------------------------------------------------------------------------------------------ masked_mean, stats_pool
@pytest.mark.parametrize("C", [1, 129, 384])
def test_masked_mean_lengths_zero_one_full_and_past_the_end(C):
    """128 threads per block: C = 129 takes a second block with one live lane"""
    B, T = 5, 6
    x = rnd(B, T, C, seed=30 + C)
    for lens in (i32([0, 1, T, T + 3, 3]), None):
        out = canary(B * C + 7)
        od = dev(out)
        hip.masked_mean(dev(x), dev(lens), od, B, T, C)
        check("masked_mean", f"C {C} lens {None if lens is None else lens.tolist()}", od, *both(R.masked_mean, x.flatten(), lens, out, B, T, C))
        if lens is not None:
            assert bool((od[:C] == 0).all())  # no frame: 0 / 1e-6


@pytest.mark.parametrize("C", [1, 257, 384])
@pytest.mark.parametrize("T", [1, 256, 257, 600])
def test_stats_pool_strides_lengths_and_large_logits(T, C):
    """T past 256 takes a second (and third) step of the 256-thread loops for the maximum and the sum; logits of scale 30 overflow
    expf unless the maximum is subtracted; a length of 1 and a row with all its weight on one frame reach the 1e-6 floor under the root"""
    B = 4
    h, lg = rnd(B, T, C, seed=40 + T + C), rnd(B, T, seed=41 + T + C, scale=30.0)
    lg[3, T - 1] = 400.0  # the last frame alone carries row 3 (behind the first 256 when T > 256)
    for lens in (i32([1, T, T + 5, T]), None):
        out = canary(B * 2 * C + 7)
        od = dev(out)
        hip.stats_pool(dev(h), dev(lg), dev(lens), od, B, T, C)
        r64, r32 = both(R.stats_pool, h.flatten(), lg.flatten(), lens, out, B, T, C)
        check("stats_pool", f"T {T} C {C} lens {None if lens is None else lens.tolist()}", od, r64, r32)
        assert float((r64[3 * 2 * C + C: 4 * 2 * C] - 1e-3).abs().max()) < 1e-12  # the floor is reached


# ------------------------------------------------------------------------------------------------ argmax_rows
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130, 2048])
def test_argmax_rows_ties_infinities_nans_and_output_mapping(N):
    """7 rows (4 per workgroup) of values in {0, 1, 2}: ties everywhere, the lowest index has to win in the lane loop and in the shuffle
    tree.  Row 1: the only maxima at n and n + 64 (one lane); row 2: at n and n + 1 with n odd (neighbouring lanes, the lower index
    arrives in the LAST exchange); row 3: all -inf; row 4: NaN before the maximum; row 5: all NaN.  inner = 3, ldo = 5, ldx = N + 4
    with the slack above every value."""
    rows, ldx, inner, ldo = 7, N + 4, 3, 5
    x = torch.randint(0, 3, (rows, ldx), generator=torch.Generator().manual_seed(50 + N)).float()
    x[:, N:] = 9.0
    if N > 64:
        x[1, :N] = 0.0
        x[1, 0] = 1.0
        x[1, N - 65], x[1, N - 1] = 2.0, 2.0
    if N >= 13:
        x[2, :N] = 1.0
        x[2, 11], x[2, 12] = 2.0, 2.0
    x[3, :N] = float("-inf")
    if N >= 8:
        x[4, :N] = 0.0
        x[4, 1], x[4, 3], x[4, N - 2] = NAN, NAN, 2.0
    x[5, :N] = NAN
    out = icanary(3 * ldo + 2)
    od = dev(out)
    hip.argmax_rows(dev(x), od, rows=rows, N=N, ldx=ldx, ldo=ldo, o_off=1, inner=inner)
    ref = out.clone()
    ref[1:] = R.argmax_rows(x.flatten(), ldx, out[1:], ldo, inner, rows, N)
    check_int("argmax_rows", f"N {N}", od, ref)
    assert int((ref == -7).sum()) == out.numel() - rows and ref[1 + 5].item() == 0 and ref[1 + 5 + 2].item() == 0
    if N > 64:
        assert ref[1 + 1].item() == N - 65
    if N >= 13:
        assert ref[1 + 2].item() == 11


# ------------------------------------------------------------------------------------------------ gathers
@pytest.mark.parametrize("D", [4, 384])
def test_codebook_sum_clamps_no_base_and_segmented_output(D):
    V, Q, rows, rps = 20, 4, 7, 3
    rows_t = Q * V + 1
    table = rnd(rows_t, D, seed=60 + D)
    tok = torch.randint(0, V, (rows, Q + 1), generator=torch.Generator().manual_seed(61), dtype=torch.int32)  # ldt = Q + 1
    tok[2, 0], tok[4, 3], tok[6, 3] = -1, V + 5, V  # below row 0; past the last row with the last offset; the last row itself
    col, off, wq = i32([0, 2, 3]), i32([0, 2 * V, 3 * V]), torch.softmax(rnd(3, seed=62), 0)
    ldo, seg = D + 4, 3 * (D + 4) + 8
    for base in (None, rnd(rows, D, seed=63)):
        out = canary(4 + 3 * seg)
        od = dev(out)
        hip.codebook_sum(dev(tok), Q + 1, dev(col), dev(off), dev(wq), dev(table), od, rows=rows, D=D, base=dev(base), alpha=0.3, beta=0.7,
                         ldo=ldo, rows_per_seg=rps, o_seg_stride=seg, o_off=4)
        r64, r32 = both(R.codebook_sum, tok.flatten(), Q + 1, col, off, wq, 3, table.flatten(), rows_t, None if base is None else base.flatten(),
                        0.3, 0.7, out, ldo, seg, rows, rps, D, o_off=4)
        check("codebook_sum", f"D {D} base {base is not None}", od, r64, r32)


@pytest.mark.parametrize("C", [4, 384])
def test_text_embed_clamps_no_lens_and_empty_row(C):
    B, T, rows_t = 3, 5, 30
    ids = torch.randint(0, rows_t, (B, T), generator=torch.Generator().manual_seed(64), dtype=torch.int32)
    ids[0, 1], ids[0, 3], ids[2, 0] = -2, rows_t + 3, rows_t
    table, pe = rnd(rows_t, C, seed=65 + C), rnd(T, C, seed=66 + C)
    for lens in (i32([T, 0, 3]), None):
        out = canary(B * T * C + 8)
        od = dev(out)
        hip.text_embed(dev(ids), dev(lens), dev(table), dev(pe), od, B, T, C)
        r64, r32 = both(R.text_embed, ids.flatten(), lens, table.flatten(), rows_t, pe.flatten(), out, B, T, C)
        check("text_embed", f"C {C} lens {None if lens is None else lens.tolist()}", od, r64, r32)


# ------------------------------------------------------------------------------------------------ add_pos, tanh_affine
@pytest.mark.parametrize("B,T,C", [(1, 1, 1), (1, 5, 51), (2, 2, 64), (1, 1, 257)])
@pytest.mark.parametrize("pos0", [0, 3])
def test_add_pos_around_one_block(pos0, B, T, C):
    """1, 255, 256 and 257 elements (256 per block); the table ends at pos0 + T"""
    rv, table = rnd(B, C, seed=70 + C), rnd(pos0 + T, C, seed=71 + C)
    out = canary(B * T * C + 7)
    od = dev(out)
    hip.add_pos(dev(rv), dev(table), od, B, T, C, pos0)
    check("add_pos", f"{B}x{T}x{C} pos0 {pos0}", od, *both(R.add_pos, rv.flatten(), table.flatten(), out, B, T, C, pos0))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_tanh_affine_around_one_block(n):
    x = rnd(n + 3, seed=72 + n, scale=3.0)
    x[0] = 20.0  # saturated
    out = canary(n + 7)
    od = dev(out)
    hip.tanh_affine(dev(x), od, 1.0, 1.2, n)
    check("tanh_affine", f"n {n}", od, *both(R.tanh_affine, x, out, 1.0, 1.2, n))


# ------------------------------------------------------------------------------------------------ rope, upsample2, final_conv
@pytest.mark.parametrize("segs", [1, 3])
@pytest.mark.parametrize("pos0", [0, 7])
@pytest.mark.parametrize("H", [1, 8])
@pytest.mark.parametrize("dh", [2, 64])
def test_rope_middle_third_in_place(dh, H, pos0, segs):
    """rows of 3 H dh columns (q | k | v), the k third rotated in place: q and v stay bit-identical; tables end at pos0 + rows_per_seg"""
    rps, ldx = 5, 3 * H * dh
    rows = segs * rps
    x = rnd(rows * ldx, seed=80 + dh + H)
    ang = rnd(pos0 + rps, dh // 2, seed=81)
    c, s = torch.cos(ang), torch.sin(ang)
    xd = dev(x.clone())
    hip.rope(xd, dev(c), dev(s), rows=rows, rows_per_seg=rps, pos0=pos0, H=H, dh=dh, ldx=ldx, x_off=H * dh)
    r64, r32 = both(R.rope, x, ldx, c.flatten(), s.flatten(), rows, rps, pos0, H, dh, x_off=H * dh)
    g = xd.cpu().view(rows, 3, H * dh)
    assert torch.equal(g[:, 0], x.view(rows, 3, -1)[:, 0]) and torch.equal(g[:, 2], x.view(rows, 3, -1)[:, 2]), "rope touched q or v"
    mid = lambda t: torch.where(torch.arange(3)[None, :, None] == 1, t.view(rows, 3, H * dh).double(), NAN).flatten()  # noqa: E731
    check("rope", f"dh {dh} H {H} pos0 {pos0} segs {segs}", mid(xd.cpu()), mid(r64), mid(r32))


@pytest.mark.parametrize("C", [1, 512])
@pytest.mark.parametrize("T", [1, 2, 9])
def test_upsample2_first_frame_and_output_segments(T, C):
    """T = 1: only the t > 0 - guarded taps; the output sits behind 3 frames of each segment, segments 5 words further apart"""
    B = 2
    x, w = rnd(B, T, C, seed=90 + T), rnd(C, 4, seed=91 + C)
    seg = (3 + 2 * T) * C + 5
    out = canary(B * seg + 3)
    od = dev(out)
    hip.upsample2(dev(x), dev(w), od, B=B, T=T, C_=C, y_seg_stride=seg, y_off=3 * C)
    check("upsample2", f"T {T} C {C}", od, *both(R.upsample2, x.flatten(), w.flatten(), out, seg, B, T, C, y_off=3 * C))


@pytest.mark.parametrize("T", [1, 2, 255, 256, 257, 513])
def test_final_conv_workgroup_hand_over(T):
    """256 samples per workgroup with a halo of two rows: T = 256 / 257 is where one workgroup hands over to the next; segments of h
    carry 3 rows more than the T + 2 the kernel may read (filled with 50: reading one shows), wav rows are T + 3 apart"""
    B = 2
    hseg, wseg = (T + 2 + 3) * 64, T + 3
    h = rnd(B, T + 5, 64, seed=95 + T)
    h[:, T + 2:] = 50.0
    w, bias = rnd(3, 64, seed=96, scale=0.1), 0.05
    out = canary(B * wseg + 5)
    od = dev(out)
    hip.final_conv(dev(h), dev(w), bias, od, B=B, T=T, h_seg_stride=hseg, wav_seg_stride=wseg)
    check("final_conv", f"T {T}", od, *both(R.final_conv, h.flatten(), hseg, w.flatten(), bias, out, wseg, B, T))


# ------------------------------------------------------------------------------------------------ dwconv
@pytest.mark.parametrize("C", [4, 260])
@pytest.mark.parametrize("B,T,ksize,dil,comb", [(3, 341, 11, 8, False), (16, 64, 11, 8, True), (4, 256, 11, 8, True), (17, 63, 11, 8, False),
                                                (16, 64, 13, 4, False)])
def test_dwconv_on_both_sides_of_the_comb_switch(B, T, ksize, dil, comb, C):
    """The comb form takes ksize 11 (and 7) once B T >= 1024 and T >= 8 dil: B T = 1023 / 1024 and T = 63 / 64 at dil 8 sit on
    either side of each condition, ksize 13 stays on the per-output kernel.  lens holds 0 and 1.  Every case agrees with the float64
    convolution; where the comb form runs it equals, bit for bit, the per-output kernel run one utterance at a time."""
    assert comb == (ksize in (7, 11) and B * T >= 1024 and T >= 8 * dil)
    left = (ksize - 1) * dil // 2
    x, w, b, res = rnd(B, T, C, seed=110 + T), rnd(ksize, C, seed=111), rnd(C, seed=112), rnd(B, T, C, seed=113)
    lens = i32(([0, 1, T, T // 2, T + 2] * 4)[:B])
    xd, wd, bd, rd = dev(x), dev(w), dev(b), dev(res)
    for mode, ln in ((0, lens), (1, None), (2, lens)):
        out = canary(B * T * C + 8)
        od = dev(out)
        kw = dict(C_=C, ksize=ksize, dil=dil, left=left, mode=mode)
        hip.dwconv(xd, wd, bd, od, B=B, T=T, res=rd if mode == 1 else None, lens=dev(ln), **kw)
        r64, r32 = both(R.dwconv, x.flatten(), w.flatten(), b, res.flatten() if mode == 1 else None, out, ln, B, T, C, ksize, dil, left, mode)
        check("dwconv", f"B {B} T {T} k {ksize} C {C} mode {mode} lens {ln is not None}", od, r64, r32)
        if comb:
            for i in range(B):  # one utterance per call: fewer than 1024 rows, the per-output kernel
                one = torch.full((T * C,), NAN, device=DEV)
                hip.dwconv(xd[i].contiguous(), wd, bd, one, B=1, T=T, res=rd[i].contiguous() if mode == 1 else None,
                           lens=None if ln is None else dev(ln[i: i + 1]), **kw)
                assert torch.equal(od[i * T * C: (i + 1) * T * C], one), (mode, i)


# ------------------------------------------------------------------------------------------------ bf16 images
def _bf16_patterns(n):
    """fp32 bit patterns, NORMAL numbers only (subnormal operands are out of scope: the conversion instructions may flush them):
    halfway cases with an even and an odd kept bit, one ulp either side of halfway, a mantissa carry into the exponent, the largest
    finite float (rounds to inf), the largest float that rounds to a finite bf16, +-0, +-inf; then random normals of every exponent"""
    head = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0x3FFF8000, 0x3FFFFFFF,
            0x7F7FFFFF, 0x7F7F7FFF, 0xFF7FFFFF, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00800000, 0x00FF8000, 0x7EFF8000]
    g = torch.Generator().manual_seed(120)
    m = max(0, n - len(head))
    body = torch.randint(0x00800000, 0x7F800000, (m,), generator=g) | (torch.randint(0, 2, (m,), generator=g) << 31)
    return R.bits_f32(torch.cat([torch.tensor(head), body])[:n])


@pytest.mark.parametrize("n", [4, 1028])
def test_cvt_f32_bf16_rounds_to_nearest_even_and_back(n):
    """bits equal to torch's ``.to(torch.bfloat16)`` and to the integer-arithmetic reference; the bf16 -> fp32 image and the round trip
    are exact; dst_off = 4 elements, the words around the image keep the canary.  n = 1028: a second block with one live thread."""
    v = _bf16_patterns(n)
    want = v.to(torch.bfloat16).view(torch.int16).long() & 0xFFFF
    assert torch.equal(want, R.cvt_f32_bf16_bits(v, n))
    dst = torch.full((n + 12,), NAN, dtype=torch.bfloat16, device=DEV)
    hip.cvt_f32_bf16(dev(v), dst, n, dst_off=4)
    bits = dst.cpu().view(torch.int16).long() & 0xFFFF
    assert torch.equal(bits[4: 4 + n], want), (bits[4: 4 + n] != want).nonzero().flatten().tolist()[:8]
    assert bool((bits[:4] == 0x7FC0).all()) and bool((bits[4 + n:] == 0x7FC0).all()), "a word outside the image lost its canary"
    back = canary(n + 8)
    bd = dev(back)
    hip.cvt_bf16_f32(dst[4: 4 + n].clone(), bd, n)
    assert torch.equal(R.f32_bits(bd.cpu()[:n]), R.f32_bits(R.cvt_bf16_f32(want, n))) and bool(torch.isnan(bd[n:]).all())
    again = torch.full((n,), NAN, dtype=torch.bfloat16, device=DEV)
    hip.cvt_f32_bf16(bd, again, n)
    assert torch.equal(again.cpu().view(torch.int16).long() & 0xFFFF, want), "the round trip is not exact"


def test_cvt_nan_stays_nan():
    v = R.bits_f32(torch.tensor([0x7FC00000, 0xFFC00000, 0x7F800001, 0x3F800000]))  # quiet, negative, signalling with a low payload, 1.0
    dst = torch.zeros(4, dtype=torch.bfloat16, device=DEV)
    hip.cvt_f32_bf16(dev(v), dst)
    assert torch.isnan(dst.float().cpu()).tolist() == [True, True, True, False]
    back = torch.zeros(4, device=DEV)
    hip.cvt_bf16_f32(dst, back)
    assert torch.isnan(back.cpu()).tolist() == [True, True, True, False] and float(back[3]) == 1.0


# ------------------------------------------------------------------------------------------------ fill2d, copy2d, nar_seed
@pytest.mark.parametrize("rows,width", [(1, 1), (3, 5), (1, 300), (7, 64)])
def test_fill2d_copy2d_pitched_rows_keep_the_gaps(rows, width):
    dp, sp = width + 3, width + 6
    value = 0x89ABCDEF
    buf = icanary(2 + rows * dp + 4)
    bd = dev(buf)
    hip.fill2d(bd, value, rows=rows, width=width, pitch=dp, p_off=2)
    ref = buf.clone()
    ref[2:] = R.fill2d(buf[2:], dp, rows, width, value - (1 << 32))
    check_int("fill2d", f"{rows}x{width}", bd, ref)
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (1 + rows * sp,), generator=torch.Generator().manual_seed(130 + width), dtype=torch.int32)
    bd = dev(buf)
    hip.copy2d(bd, dev(src), rows=rows, width=width, dpitch=dp, spitch=sp, d_off=2, s_off=1)
    ref = buf.clone()
    ref[2:] = R.copy2d(buf[2:], dp, src[1:], sp, rows, width)
    check_int("copy2d", f"{rows}x{width}", bd, ref)
    assert int((ref == -7).sum()) >= buf.numel() - rows * width


def test_nar_seed_clamps_into_column_zero_only():
    B, T, Q, bs, vmax = 3, 5, 4, 9, 2047
    cb0 = torch.randint(0, vmax + 1, (2 + B * bs,), generator=torch.Generator().manual_seed(140), dtype=torch.int32)
    cb0[2: 6] = i32([-2, 0, vmax, vmax + 1])  # vmax + 1: the EOS code of a row that stopped early
    cb0[2 + T: 2 + bs] = -5  # the history past T is not read
    tok = icanary(B * T * Q + 3)
    td = dev(tok)
    hip.nar_seed(td, dev(cb0), Q=Q, B=B, T=T, vmax=vmax, cb0_bstride=bs, cb0_off=2)
    ref = R.nar_seed(tok, Q, cb0[2:], bs, B, T, vmax)
    check_int("nar_seed", "", td, ref)
    m = ref[: B * T * Q].view(B * T, Q)
    assert m[:4, 0].tolist() == [0, 0, vmax, vmax] and bool((m[:, 1:] == -7).all()) and bool((m[:, 0] >= 0).all())


# ------------------------------------------------------------------------------------------------ rejected arguments
def test_entry_points_reject_what_they_cannot_run():
    """each returns -2 before any launch (the outputs keep their canary)"""
    x, out = dev(rnd(4096, seed=150)), dev(canary(4096))
    w = dev(rnd(1025, seed=151))
    i4 = dev(i32([0, 0, 0, 0]))
    with pytest.raises(hip.SoproHipError):
        hip.norm(x, out, w, rows=1, C_=1025, eps=1e-6)
    with pytest.raises(hip.SoproHipError):
        hip.norm(x, out, w, rows=1, C_=64, eps=1e-6, kind=7)
    with pytest.raises(hip.SoproHipError):
        hip.row_stats(x, 2, 96, out)
    bf = torch.full((64,), NAN, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(hip.SoproHipError):
        hip.cvt_f32_bf16(x, bf, 6)
    with pytest.raises(hip.SoproHipError):
        hip.cvt_f32_bf16(x, bf, 8, dst_off=1)
    with pytest.raises(hip.SoproHipError):
        hip.dwconv(x, w, None, out, B=1, T=8, C_=6, ksize=3, dil=1, left=1)
    with pytest.raises(hip.SoproHipError):
        hip.dwconv(x, w, None, out, B=1, T=8, C_=8, ksize=3, dil=1, left=1, mode=1)
    with pytest.raises(hip.SoproHipError):
        hip.codebook_sum(i4, 1, i4, i4, w, x, out, rows=2, D=6)
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(bf.float()).all())
