"""tests/seanet_ref.py against float64 torch layers, its one-pass model against torch's bf16 casts, and its tolerances against two
things they must tell apart: torch's float32 evaluation of the same layers (inside the three-pass tolerance on every case) and CPU
emulations of two broken kernels (outside it on the banded cases of tests/test_gpu_seanet_edges.py) - the lo plane of one 16-wide K
substep dropped, and the lo plane of one halo row taken from the neighbouring row."""
import pytest
import torch
import torch.nn.functional as F

import gemm_ref as G
import seanet_ref as S
from oracle import sopro_oracle as O
from sopro_amd import pack

OPS = ("res128", "up128", "tail", "uptail")
EDGE_T = {"res128": (1, 2, 5, 33, 65, 129), "up128": (1, 3, 64, 65, 129), "tail": (1, 2, 15, 127, 253), "uptail": (1, 2, 33, 65)}


def unpack_conv1d(wp, ci):
    w = wp.reshape(wp.shape[0], -1, ci).permute(0, 2, 1).contiguous()
    assert torch.equal(pack.pack_conv1d(w), wp)
    return w


def unpack_convtr1d(wp, bp, ci=128, co=64, r=4):
    wt = wp.reshape(r, co, 2, ci).permute(3, 1, 2, 0).flip(2).reshape(ci, co, 2 * r).contiguous()
    w2, b2 = pack.pack_convtr1d(wt, bp[:co], r)
    assert torch.equal(w2, wp) and torch.equal(b2, bp)
    return wt, bp[:co]


def layers(case, dtype, one_pass=False):
    """The operation through conv1d / conv_transpose1d / elu in `dtype`; one_pass: torch's bf16 casts where the kernels round."""
    w, B, T = case["w"], case["B"], case["T"]
    rows_bf16 = case["bf16"]
    cast = (lambda t: t.to(torch.bfloat16).to(dtype)) if one_pass else (lambda t: t)
    x = case["x"].to(torch.bfloat16 if rows_bf16 else torch.float32).to(dtype)  # [B, T, C] as the buffer holds it
    op = case["op"]
    h = x.transpose(1, 2)
    if op in ("up128", "uptail"):
        wt, bt = unpack_convtr1d(w["wu"], w["bu"])
        h = O.causal_convtr1d(cast(h), cast(wt.to(dtype)), bt.to(dtype), 4)
        if op == "up128":
            out = h.transpose(1, 2).reshape(B, T, 256)   # [B, 4 T, 64] -> rows of 4 samples x 64 channels
            return cast(out) if rows_bf16 else out
    ci = 128 if op == "res128" else 64
    w1, w2 = unpack_conv1d(w["w1"], ci).to(dtype), unpack_conv1d(w["w2"], w["w2"].shape[1]).to(dtype)
    y = O.causal_conv1d(cast(F.elu(h)), cast(w1), w["b1"].to(dtype))
    y = O.causal_conv1d(cast(F.elu(y)), cast(w2), w["b2"].to(dtype))
    hp = F.elu(h + y)
    if op == "res128":
        out = hp.transpose(1, 2)
        return cast(out) if rows_bf16 else out
    wf = w["wf"].t().reshape(1, 64, 3).to(dtype)
    return O.causal_conv1d(hp, wf, torch.tensor([w["bf"]], dtype=dtype))[:, 0]


def shaped(ref, like):
    return ref.out.ref.reshape(like.shape)


@pytest.mark.parametrize("op", OPS)
def test_reference_is_the_float64_layers_and_keeps_the_canaries(op):
    for T in EDGE_T[op]:
        for B in (1, 3):
            case = S.make_case(op, B, T, seed=T)
            ref = S.run_ref(case, 3)
            want = layers(case, torch.float64)
            got = shaped(ref, want)
            assert float((got - want).abs().max()) <= 1e-12 * (1.0 + float(want.abs().max())), (op, B, T)
            o = ref.out
            other = ~o.owned()
            assert torch.equal(o.bits(o.buf)[other], o.bits(case["bufs"]["out"])[other])  # every word it does not own: as the caller left it
            assert int(o.owned().sum()) == want.numel() and bool(torch.isfinite(o.values(o.buf)).all())
            assert bool((ref.tol > 0).all()) and bool(torch.isfinite(ref.tol).all())


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("op", OPS)
def test_one_pass_model_is_torchs_bf16_casts(op, bf16):
    for T in EDGE_T[op][:4]:
        case = S.make_case(op, 2, T, bf16=bf16, seed=50 + T)
        ref = S.run_ref(case, 1)
        want = layers(case, torch.float64, one_pass=True)
        if bf16 and op in ("res128", "up128"):  # the output rows are bf16: the buffer holds the rounded values
            got = ref.out.values(ref.out.buf).reshape(want.shape)
            assert torch.equal(got, want), (op, T)
        else:
            assert float((shaped(ref, want) - want).abs().max()) <= 1e-12 * (1.0 + float(want.abs().max())), (op, T)


def _ratio(ref, vals):
    err = (vals.reshape(ref.out.ref.shape).double() - ref.out.ref).abs()
    return float((err / ref.tol.reshape(err.shape)).max())


@pytest.mark.parametrize("op", OPS)
def test_float32_layers_lie_within_the_three_pass_tolerance(op):
    worst = 0.0
    for T in EDGE_T[op]:
        for kw in (dict(), dict(special="tiny"), dict(special="big"), dict(special="bias1"), dict(special="w0"), dict(special="zero"),
                   dict(band=(list(S.SUBSTEPS[op])[0], T)), dict(live=(64, 62))):
            case = S.make_case(op, 2, T, seed=90 + T, **kw)
            r = _ratio(S.run_ref(case, 3), layers(case, torch.float32))
            worst = max(worst, r)
            assert r <= 1.0, (op, T, kw, r)
    print(f"float32 layers / three-pass tolerance, worst: {op} {worst:.3f}")


# ---- two broken kernels, emulated on the operand the product is formed from (three-pass forms: x = hi + lo)
def drop_lo(target, s):
    def hook(name, a, w):
        if name != target:
            return a
        a = a.clone()
        a[..., 16 * s:16 * s + 16] = G.bf16_round(a[..., 16 * s:16 * s + 16])
        return a
    return hook


def halo_lo(target, rows, Cc):
    """Output rows `rows` (the first of a tile): the lo plane of their oldest tap (a halo row of the tile) is its neighbour's."""
    def hook(name, a, w):
        if name != target:
            return a
        a = a.clone()
        for r in rows:
            if r < a.shape[1]:
                near = a[:, r, Cc:2 * Cc]
                a[:, r, :Cc] = G.bf16_round(a[:, r, :Cc]) + (near - G.bf16_round(near))
        return a
    return hook


FIRST = {"res128": "res.c1", "tail": "tail.c1", "up128": "up", "uptail": "up"}
BANDS = [(op, c, s) for op in OPS for c in S.SUBSTEPS[op] for s in range(S.SUBSTEPS[op][c])]


@pytest.mark.parametrize("op,c,s", BANDS)
def test_a_dropped_lo_plane_exceeds_the_tolerance_on_the_banded_weights(op, c, s):
    """Every substep of every contraction: the band makes its sixteen terms the whole product."""
    T = 37 if op != "uptail" else 35
    case = S.make_case(op, 2, T, seed=7 + s, band=(c, s))
    name = {"c1": FIRST[op] if op in ("res128", "tail") else "tail.c1", "c2": "res.c2" if op == "res128" else "tail.c2", "up": "up"}[c]
    ref = S.run_ref(case, 3)
    broken = S.run_ref(case, 3, hook=drop_lo(name, s))
    r = _ratio(ref, broken.out.ref)
    print(f"dropped lo plane / tolerance: {op} {c} substep {s}: {r:.2f}")
    assert r > 1.0, (op, c, s, r)
    other = S.run_ref(case, 3, hook=drop_lo(name, (s + 1) % S.SUBSTEPS[op][c]))  # a dead substep's lo plane changes nothing
    assert _ratio(ref, other.out.ref) == 0.0


@pytest.mark.parametrize("op,tile", [("res128", 64), ("up128", 64), ("tail", 126), ("tail", 14), ("uptail", 32)])
def test_a_halo_rows_neighbouring_lo_plane_exceeds_the_tolerance_on_the_banded_activations(op, tile):
    """One live input row per tile, the halo row: the tile behind the seam reads it through its own staged copy."""
    T = 2 * tile + 3
    up = op in ("up128", "uptail")
    # residual blocks: output row s0 reads samples s0 - 2 (oldest tap; live) and s0 - 1; transposed convolution: A row t0 - 1 = [x[t0 - 2] | x[t0 - 1]]
    case = S.make_case(op, 2, T, seed=3, live=(tile, tile - 2))
    rows = [tile - 1, 2 * tile - 1] if up else [tile, 2 * tile]
    ref = S.run_ref(case, 3)
    broken = S.run_ref(case, 3, hook=halo_lo(FIRST[op], rows, S.CH[op]))
    r = _ratio(ref, broken.out.ref)
    print(f"neighbour's lo plane in a halo row / tolerance: {op} tile {tile}: {r:.2f}")
    assert r > 1.0, (op, tile, r)


# ---- the charge of a staged bf16 value: sound, and capped
def test_the_staging_charge_is_sound_and_a_wide_element_costs_at_most_nine_times_its_error():
    g = torch.Generator().manual_seed(5)
    mag = torch.ldexp(torch.ones(40, dtype=torch.float64), torch.arange(-30, 10))
    a = (mag[:, None] * (1.0 + torch.rand(40, 64, generator=g, dtype=torch.float64))).reshape(-1)
    a = torch.cat([a, -a, G.bf16_round(a), torch.zeros(8, dtype=torch.float64)]).float().double()   # fp32 numbers, as the kernels hold
    worst = 0.0
    for rel in (0.0, 2.0 ** -20, 2.0 ** -12, 2.0 ** -10, 2.0 ** -9, 2.0 ** -8, 2.0 ** -6, 0.5, 3.0, 1e3):
        d = rel * a.abs() + (2e-7 if rel in (2.0 ** -12, 3.0) else 0.0)
        cnt = S._Count()
        charge = S.stage_charge(a, d, cnt)
        wide = d > S.spacing_bf16(a) / 4
        assert bool((charge[wide] <= S.WIDE_CAP * d[wide]).all())
        assert cnt.wide == int(wide.sum()) and cnt.wide_charge <= S.WIDE_CAP * cnt.wide_d
        assert bool((charge[d == 0] == 0).all())
        for t in torch.linspace(-1.0, 1.0, 41, dtype=torch.float64):   # a' anywhere within d of a (an fp32 number)
            moved = (G.bf16_round((a + t * d).float().double()) - G.bf16_round(a)).abs()
            assert bool((moved <= charge).all()), (rel, float(t))
        worst = max(worst, float((charge[wide] / d[wide]).max()) if bool(wide.any()) else 0.0)
    print(f"largest wide charge / carried error on the grid: {worst:.2f} (cap {S.WIDE_CAP})")


@pytest.mark.parametrize("op", OPS)
def test_the_wide_charges_of_every_one_pass_case_stay_under_their_cap(op):
    for bf16 in (False, True):
        for kw in (dict(), dict(special="tiny"), dict(special="zero"), dict(special="bias1"), dict(band=(list(S.SUBSTEPS[op])[0], 1)), dict(live=(32, 30))):
            ref = S.run_ref(S.make_case(op, 2, 67, bf16=bf16, seed=12, **kw), 1)
            assert ref.wide <= ref.staged and ref.wide_charge <= S.WIDE_CAP * ref.wide_d, (op, bf16, kw, ref.wide_charge, ref.wide_d)


# ---- broken kernels of every form (three passes, one pass, bf16 rows)
FORMS = ((3, False), (1, False), (1, True))


def neighbour_substep(target, s, n):
    """Substep s of the staged operand taken from the next substep (a fragment read 32 bytes off)."""
    def hook(name, a, w):
        if name != target:
            return a
        a, t = a.clone(), (s + 1) % n
        a[..., 16 * s:16 * s + 16] = a[..., 16 * t:16 * t + 16]
        return a
    return hook


def contraction_name(op, c):
    return {"c1": "res.c1" if op == "res128" else "tail.c1", "c2": "res.c2" if op == "res128" else "tail.c2", "up": "up"}[c]


@pytest.mark.parametrize("passes,bf16", FORMS)
@pytest.mark.parametrize("op,c,s", BANDS)
def test_a_fragment_from_the_neighbouring_substep_exceeds_the_tolerance_in_every_form(op, c, s, passes, bf16):
    T = 37 if op != "uptail" else 35
    case = S.make_case(op, 2, T, bf16=bf16, seed=7 + s, band=(c, s))
    ref = S.run_ref(case, passes)
    broken = S.run_ref(case, passes, hook=neighbour_substep(contraction_name(op, c), s, S.SUBSTEPS[op][c]))
    r = _ratio(ref, broken.out.ref)
    assert r > 1.0, (op, c, s, passes, bf16, r)


def with_weights(case, **changed):
    c = dict(case)
    c["w"] = dict(case["w"], **changed)
    return c


def swap_pairs(v):
    return v.reshape(-1, 2).flip(1).reshape(-1)


@pytest.mark.parametrize("passes,bf16", FORMS)
@pytest.mark.parametrize("op", OPS)
def test_wrong_biases_taps_and_a_dropped_first_tile_mask_exceed_the_tolerance(op, passes, bf16):
    """Index mistakes of the epilogues, as the operands they amount to: the bias of the neighbouring column, b1 of the other column
    half, the last layer's taps reversed, and ELU(h') of the samples before 0 not zeroed (dense data, and biases of order 1)."""
    for special in (None, "bias1"):
        case = S.make_case(op, 2, 67, bf16=bf16, seed=31, special=special)
        ref, w = S.run_ref(case, passes), case["w"]
        broken = {}
        if op == "res128":
            broken["b2 of the neighbouring column"] = with_weights(case, b2=swap_pairs(w["b2"]))
            broken["b1 of the other column half"] = with_weights(case, b1=w["b1"].roll(32))
        if op in ("up128", "uptail"):
            broken["bias of the neighbouring column"] = with_weights(case, bu=swap_pairs(w["bu"]))
        if op in ("tail", "uptail"):
            broken["taps of the last layer reversed"] = with_weights(case, wf=w["wf"].flip(0))
            broken["b1 of the other column half"] = with_weights(case, b1=w["b1"].roll(16))
        for what, bad in broken.items():
            r = _ratio(ref, S.run_ref(bad, passes).out.ref)
            assert r > 1.0, (op, passes, bf16, special, what, r)
        if op in ("tail", "uptail"):  # samples -2, -1: h = 0, y = ELU(b1), h' = w2 ELU(b1) + b2 - a kernel that does not mask them adds their taps
            one = bf16 or passes == 1
            rnd = G.bf16_round if one else (lambda t: t)
            pad = G.elu64(rnd(G.elu64(w["b1"].double())) @ rnd(w["w2"].double()).t() + w["b2"].double())
            wf = w["wf"].double()
            wav = ref.out.ref.reshape(2, -1).clone()
            wav[:, 0] += pad @ wf[0] + pad @ wf[1]
            if wav.shape[1] > 1:
                wav[:, 1] += pad @ wf[0]
            r = _ratio(ref, wav)
            assert r > 1.0, (op, passes, bf16, special, "first-tile mask dropped", r)
