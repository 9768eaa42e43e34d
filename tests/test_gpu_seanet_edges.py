"""Tile seams, strides, every tiles / trips walk and the one-pass forms of the four fused SEANet decoder files (csrc/seanet_res.hip,
seanet_up.hip, seanet_tail.hip, seanet_uptail.hip) against the float64 reference of tests/seanet_ref.py.

Every case (seanet_ref.make_case) has slack in every stride, NaN canaries in all output slack, in guard words in front of the first
and behind the last segment of every buffer and in every input row past the rows the operation owns (the kernels redirect those
loads to row 0, so a correct kernel never sees them), a finite sentinel that is not 0 in the two front rows of res128's out, and
different data per utterance.  After a launch the WHOLE output buffer is compared with the reference's copy: owned words are held to
the reference's per-element tolerance, all others bit for bit.  Every set_tiles probe is reset in `finally`.

Lengths: the smallest at which the named mechanism exists - res128 / up128: the row groups of four (1..8), the 32-row MFMA halves
(31..37), a whole 64-row tile, a one-row tile behind it, a workgroup whose second or third tile lies past the end (tiles 2, 3 at
T <= 128 / 129, 193); four-wave tail: one 126-sample tile, its seam, a third tile; sixteen-wave tail: one 14-sample wave tile, one
sixteen-tile round of 224 samples, a round past the end, and the 8- and 32-trip walks production picks at size (set_tiles -8, -32);
uptail: the carried rows at the head of an utterance, across a seam inside a workgroup (tiles 0) and across a workgroup boundary
(tiles 1: every tile behind the first starts from a warm-up tile).

Operand families.  Dense: every length x B = 1, 3 x every tiles setting.  Banded weights: one 16-wide K substep of one contraction
live, cycling through every substep of every contraction (in the tail and the fused level the contractions around the band keep one
live term per output, seanet_ref._thin_behind: wav sums everything in front of it) - thinned to B = 2 at one length with two tiles
and the default walk; banded activations: one live input row per tile at the tile's first row, its last row (the newer halo row of
the next tile) and the row before it (the older halo row) - thinned the same way.  Specials (zero rows, +-1e-8 .. -100, 1e3, biases
of order 1, zero weights) at one two-tile length, B = 2.  A seeded sweep of 96 draws over T <= 200.

Tolerances: seanet_ref's module docstring (derived from the reference alone).  Bit-equalities claimed, all exact: every tiles /
trips setting of one kernel; a repeated launch; up128 = sopro_gemm_bf16x3 / x1 on the overlapping-row form; the four-wave tail with
passes = 1 = passes = 3; uptail passes = 1 on fp32 rows that hold bf16 numbers = uptail on bf16 rows; the entry points without a
passes argument = passes 3.  Worst error / tolerance per group as measured on an MI355X: profiles/seanet_edges.md (every
comparison feeds `WORST`; `pytest -s` prints the table last).
"""
import random

import pytest
import torch

import seanet_ref as S
from sopro_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}
COUNT = {"launches": 0, "wide": 0, "staged": 0}
FORMS = ("f32x3", "f32x1", "bf16")   # fp32 rows, three passes | fp32 rows, one pass | bf16 rows (one pass)
LEN_RES = (1, 2, 3, 4, 5, 6, 7, 8, 31, 32, 33, 35, 36, 37, 63, 64, 65, 66, 127, 128, 129, 193)
LEN_TAIL4 = (1, 2, 3, 4, 5, 125, 126, 127, 128, 251, 252, 253, 379)
LEN_TAIL16 = (1, 2, 13, 14, 15, 17, 18, 223, 224, 225, 447, 448, 449, 673)
LEN_UPTAIL = (1, 2, 3, 31, 32, 33, 63, 64, 65, 95, 96, 97, 129)
PROBE = {"res128": "sopro_seanet_res_set_tiles", "up128": "sopro_seanet_up_set_tiles", "tail": "sopro_seanet_tail_set_tiles",
         "uptail": "sopro_seanet_uptail_set_tiles"}


def note(group, ratio, what):
    if ratio > WORST.get(group, (-1.0, ""))[0]:
        WORST[group] = (ratio, what)


def form_of(form):
    return (1 if form != "f32x3" else 3), form == "bf16"


class Run:
    """One case on the device: the operands go over once, every launch gets a fresh copy of the output buffer."""

    def __init__(self, case):
        self.case, self.lib = case, hip.load()
        self.d = {k: v.to(DEV) for k, v in case["bufs"].items()}
        self.w = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in case["w"].items()}
        self.out0 = self.d["out"].clone()

    def call(self, passes=3, entry=None, tweak=None, out=None):
        """-> (return code, the whole output buffer on the CPU).  tweak: dict of argument overrides (refusal tests)."""
        c, w, lib = self.case, self.w, self.lib
        kw = dict(c["kw"], B=c["B"], T=c["T"], passes=passes)
        kw.update(tweak or {})
        xin = self.d["in"]
        o = self.out0.clone() if out is None else out
        es_in, es_out = xin.element_size(), o.element_size()
        p = lambda t: t.data_ptr()  # noqa: E731
        st = torch.cuda.current_stream().cuda_stream
        op, bf16 = c["op"], c["bf16"]
        if op == "res128":
            a = [p(xin) + es_in * kw["h_off"] + kw.get("h_bytes", 0), kw["h_seg_stride"], p(w["w1"]) + kw.get("w1_bytes", 0), p(w["b1"]), p(w["w2"]) + kw.get("w2_bytes", 0), p(w["b2"]),
                 (p(o) + es_out * kw["out_off"] + kw.get("out_bytes", 0)) if not kw.get("in_place") else p(xin) + es_in * kw["h_off"],
                 kw["out_seg_stride"], kw["B"], kw["T"]]
            name = entry or ("sopro_seanet_res128_bf16" if bf16 else "sopro_seanet_res128_p_f32")
            if name.endswith("_p_f32"):
                a.append(kw["passes"])
        elif op == "up128":
            a = [p(xin) + es_in * kw["x_off"] + kw.get("x_bytes", 0), kw["x_seg_stride"], p(w["wu"]) + kw.get("wu_bytes", 0), p(w["bu"]),
                 p(o) + es_out * kw["out_off"] + kw.get("out_bytes", 0), kw["out_seg_stride"], kw["B"], kw["T"]]
            name = entry or ("sopro_seanet_up128_bf16" if bf16 else "sopro_seanet_up128_f32")
            if not bf16:
                a.append(kw["passes"])
        elif op == "tail":
            a = [p(xin) + es_in * kw["h_off"] + kw.get("h_bytes", 0), kw["h_seg_stride"], p(w["w1"]) + kw.get("w1_bytes", 0), p(w["b1"]), p(w["w2"]) + kw.get("w2_bytes", 0), p(w["b2"]), p(w["wf"]) + kw.get("wf_bytes", 0),
                 w["bf"], p(o) + 4 * kw["wav_off"], kw["wav_seg_stride"], kw["B"], kw["T"]]
            name = entry or ("sopro_seanet_tail_bf16" if bf16 else "sopro_seanet_tail_p_f32")
            if name.endswith("_p_f32"):
                a.append(kw["passes"])
        else:
            a = [p(xin) + es_in * kw["x_off"] + kw.get("x_bytes", 0), kw["x_seg_stride"], p(w["wu"]) + kw.get("wu_bytes", 0), p(w["bu"]), p(w["w1"]) + kw.get("w1_bytes", 0), p(w["b1"]), p(w["w2"]) + kw.get("w2_bytes", 0),
                 p(w["b2"]), p(w["wf"]) + kw.get("wf_bytes", 0), w["bf"], p(o) + 4 * kw["wav_off"], kw["wav_seg_stride"], kw["B"], kw["T"]]
            name = entry or ("sopro_seanet_uptail_bf16" if bf16 else "sopro_seanet_uptail_f32")
            if not bf16:
                a.append(kw["passes"])
        rc = getattr(lib, name)(*a, st)
        torch.cuda.synchronize()
        COUNT["launches"] += 1
        return rc, o.cpu()

    def probe(self, tiles):
        getattr(self.lib, PROBE[self.case["op"]])(tiles)


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def check(group, case, run, passes, tiles_list, what, ref_passes=None):
    """Every tiles setting against the reference (whole buffer), all of them the same bits, a repeated launch the same bits."""
    ref = S.run_ref(case, passes if ref_passes is None else ref_passes)
    COUNT["wide"] += ref.wide
    COUNT["staged"] += ref.staged
    first = None
    try:
        for tiles in tiles_list:
            run.probe(tiles)
            rc, got = run.call(passes)
            assert rc == 0, (what, tiles, hip.load().sopro_last_error().decode())
            ratio, changed = S.compare(ref, got)
            print(f"  {group}: {what} tiles {tiles}: worst error / tolerance {ratio:.3f}, words changed outside the output {changed}")
            note(group, ratio, f"{what} tiles {tiles}")
            assert changed == 0, (what, tiles, changed)
            assert ratio <= 1.0, (what, tiles, ratio)
            if first is None:
                first = got
                rc, again = run.call(passes)
                assert rc == 0 and torch.equal(bits(again), bits(first)), (what, tiles, "a repeated launch")
            else:
                assert torch.equal(bits(got), bits(first)), (what, tiles, "tiles settings differ")
    finally:
        run.probe(0)
    return ref, first


# ------------------------------------------------------------------------------------------------ dense, every length
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("form", FORMS)
def test_res128_at_every_length_and_walk(form, B):
    passes, bf16 = form_of(form)
    for T in LEN_RES:
        case = S.make_case("res128", B, T, bf16=bf16, seed=1)
        check(f"res128 {form} dense", case, Run(case), passes, (0, 1, 2, 3), f"T {T} B {B}")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("form", FORMS)
def test_up128_at_every_length_and_walk_and_equals_the_tile_kernel(form, B):
    passes, bf16 = form_of(form)
    for T in LEN_RES:
        case = S.make_case("up128", B, T, bf16=bf16, seed=2)
        run = Run(case)
        ref, got = check(f"up128 {form} dense", case, run, passes, (0, 1, 2, 3), f"T {T} B {B}")
        if not bf16:  # the generic kernel on the overlapping-row form: row t of A = [x[t] | x[t+1]] (lda = 128), the same bits
            kw = case["kw"]
            Wp = hip.pack_w_bf16x3(run.w["wu"]) if passes == 3 else hip.pack_w_bf16x1(run.w["wu"])
            o2 = run.out0.clone()
            hip.gemm(run.d["in"], Wp, o2, M=B * T, N=256, K=256, lda=128, bias=run.w["bu"], rows_per_seg=T, a_seg_stride=kw["x_seg_stride"],
                     a_off=kw["x_off"], c_off=kw["out_off"], c_seg_stride=kw["out_seg_stride"], ldc=256)
            torch.cuda.synchronize()
            assert torch.equal(bits(o2.cpu()), bits(got)), (T, B, "sopro_gemm_bf16x%d" % passes)


@pytest.mark.parametrize("B", [1, 3])
def test_four_wave_tail_at_every_length_and_walk(B):
    """Short inputs run the three-pass four-wave kernel whatever `passes` says: the same bits, held to the three-pass tolerance."""
    for T in LEN_TAIL4:
        case = S.make_case("tail", B, T, seed=3)
        run = Run(case)
        _, got3 = check("tail four-wave dense", case, run, 3, (1, 2, 3), f"T {T} B {B}")
        _, got1 = check("tail four-wave dense", case, run, 1, (1, 2, 3), f"T {T} B {B} passes 1", ref_passes=3)
        assert torch.equal(bits(got1), bits(got3))
        rc, legacy = run.call(entry="sopro_seanet_tail_f32")
        assert rc == 0 and torch.equal(bits(legacy), bits(got3))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("form", FORMS)
def test_sixteen_wave_tail_at_every_length_and_walk(form, B):
    passes, bf16 = form_of(form)
    for T in LEN_TAIL16:
        case = S.make_case("tail", B, T, bf16=bf16, seed=4)
        check(f"tail sixteen-wave {form} dense", case, Run(case), passes, (-1, -3, -8, -32), f"T {T} B {B}")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("form", FORMS)
def test_uptail_at_every_length_and_walk(form, B):
    passes, bf16 = form_of(form)
    for T in LEN_UPTAIL:
        case = S.make_case("uptail", B, T, bf16=bf16, seed=5)
        check(f"uptail {form} dense", case, Run(case), passes, (0, 1, 2, 3), f"T {T} B {B}")


def test_uptail_one_pass_on_fp32_rows_that_hold_bf16_numbers_is_uptail_on_bf16_rows():
    for T in (33, 65):
        c16 = S.make_case("uptail", 2, T, bf16=True, seed=6)
        c32 = S.make_case("uptail", 2, T, bf16=True, seed=6)
        c32["bufs"]["in"], c32["bf16"] = c16["bufs"]["in"].float(), False
        rc16, g16 = Run(c16).call(1)
        rc32, g32 = Run(c32).call(1)
        assert rc16 == 0 and rc32 == 0 and torch.equal(bits(g16), bits(g32)), T


def test_res128_without_a_passes_argument_is_three_passes():
    case = S.make_case("res128", 2, 67, seed=7)
    run = Run(case)
    (rc3, g3), (rc, g) = run.call(3), run.call(entry="sopro_seanet_res128_f32")
    assert rc3 == 0 and rc == 0 and torch.equal(bits(g), bits(g3))


# ------------------------------------------------------------------------------------------------ banded operands
# (name, op, length: two tiles of the kernel and a part of a third, tile, forms, two walks: the default one and another)
KERNELS = [("res128", "res128", 131, 64, FORMS, (0, 2)), ("up128", "up128", 131, 64, FORMS, (0, 2)), ("tail4", "tail", 255, 126, ("f32x3",), (1, 2)),
           ("tail16", "tail", 31, 14, FORMS, (-1, -3)), ("uptail", "uptail", 67, 32, FORMS, (0, 1))]
KERNEL_ARGS = "kid,op,T,tile,forms,walks"
KID = [k[0] for k in KERNELS]


@pytest.mark.parametrize(KERNEL_ARGS, KERNELS, ids=KID)
def test_one_live_k_substep_of_one_contraction(kid, op, T, tile, forms, walks):
    for form in forms:
        passes, bf16 = form_of(form)
        for c, n in S.SUBSTEPS[op].items():
            for s in range(n):
                case = S.make_case(op, 2, T, bf16=bf16, seed=20 + s, band=(c, s))
                check(f"{kid} {form} banded weights", case, Run(case), passes, walks, f"{c} substep {s}")


@pytest.mark.parametrize(KERNEL_ARGS, KERNELS, ids=KID)
def test_one_live_input_row_per_tile(kid, op, T, tile, forms, walks):
    for form in forms:
        passes, bf16 = form_of(form)
        for pos in (0, tile - 1, tile - 2):
            case = S.make_case(op, 2, T, bf16=bf16, seed=40 + pos, live=(tile, pos))
            check(f"{kid} {form} banded activations", case, Run(case), passes, walks, f"live row {pos} of every {tile}")


@pytest.mark.parametrize("special", S.SPECIALS)
@pytest.mark.parametrize(KERNEL_ARGS, KERNELS, ids=KID)
def test_special_values(kid, op, T, tile, forms, walks, special):
    for form in forms:
        passes, bf16 = form_of(form)
        case = S.make_case(op, 2, T, bf16=bf16, seed=60, special=special)
        check(f"{kid} {form} specials", case, Run(case), passes, walks, special)


# ------------------------------------------------------------------------------------------------ seeded sweep
@pytest.mark.parametrize("chunk", range(4))
def test_seeded_sweep(chunk):
    for i in range(24):
        seed = 1000 + 24 * chunk + i
        r = random.Random(seed)
        op = r.choice(("res128", "up128", "tail", "tail", "uptail"))
        form = r.choice(FORMS)
        passes, bf16 = form_of(form)
        B, T = r.randint(1, 3), r.randint(1, 200)
        t16 = op == "tail" and (bf16 or r.random() < 0.6)
        tiles = r.choice((-1, -2, -3, -8, -32)) if t16 else (r.randint(1, 4) if op == "tail" else r.randint(0, 4))
        case = S.make_case(op, B, T, bf16=bf16, seed=seed, slack=r.randint(0, 5), lead=r.randint(0, 3))
        what = f"seed {seed}: {op} {form} B {B} T {T} tiles {tiles}"
        check(f"sweep {op}", case, Run(case), passes, (tiles,), what, ref_passes=3 if (op == "tail" and not t16) else None)


# ------------------------------------------------------------------------------------------------ refusals
def refused(run, what, passes=3, entry=None, **tweak):
    """The call returns an error and leaves every word of the output buffer (and, in place, of the input) as it was."""
    before_in = bits(run.d["in"].cpu()).clone()
    rc, got = run.call(passes, entry=entry, tweak=tweak)
    msg = hip.load().sopro_last_error().decode()
    assert rc == -2 and "bad argument" in msg, (what, rc, msg)   # refused by the argument check, in front of any launch
    assert torch.equal(bits(got), bits(run.out0.cpu())), what
    assert torch.equal(bits(run.d["in"].cpu()), before_in), what
    return msg


@pytest.mark.parametrize("bf16", [False, True])
def test_res128_refusals(bf16):
    run = Run(S.make_case("res128", 3, 37, bf16=bf16, seed=80))
    kw, es = run.case["kw"], 2 if bf16 else 4
    if not bf16:
        refused(run, "passes = 2", passes=2)
        refused(run, "passes = 0", passes=0)
    refused(run, "h misaligned", h_bytes=es)
    refused(run, "out misaligned", out_bytes=2)
    refused(run, "w1 misaligned", w1_bytes=4)
    refused(run, "w2 misaligned", w2_bytes=4)
    refused(run, "h stride % 4 / % 8", h_seg_stride=kw["h_seg_stride"] + (4 if bf16 else 2))
    refused(run, "out stride odd", out_seg_stride=kw["out_seg_stride"] + 1)
    refused(run, "h == out", in_place=True)
    refused(run, "h stride too short", h_seg_stride=(37 + 1) * 128)
    refused(run, "out stride too short", out_seg_stride=(37 + 1) * 128)
    big = (1 << 22) if bf16 else (1 << 21)
    msg = refused(run, "T at the bound", T=big, h_seg_stride=(big + 2) * 128, out_seg_stride=(big + 2) * 128)
    assert "T must stay below" in msg, msg
    refused(run, "T = 0", T=0)


@pytest.mark.parametrize("bf16", [False, True])
def test_up128_refusals(bf16):
    run = Run(S.make_case("up128", 3, 37, bf16=bf16, seed=81))
    kw, es = run.case["kw"], 2 if bf16 else 4
    if not bf16:
        refused(run, "passes = 2", passes=2)
    refused(run, "x misaligned", x_bytes=es)
    refused(run, "out misaligned", out_bytes=2)
    refused(run, "w misaligned", wu_bytes=4)
    refused(run, "x stride % 4 / % 8", x_seg_stride=kw["x_seg_stride"] + (4 if bf16 else 2))
    refused(run, "out stride odd", out_seg_stride=kw["out_seg_stride"] + 1)
    refused(run, "x stride too short", x_seg_stride=37 * 128)
    refused(run, "out stride too short", out_seg_stride=37 * 256 - 8)
    big = (1 << 31) - 128   # the largest T taken is 2^31 - 129
    msg = refused(run, "T at the bound", T=big, x_seg_stride=(big + 1) * 128, out_seg_stride=big * 256)
    assert "T must stay at or below" in msg, msg


@pytest.mark.parametrize("bf16", [False, True])
def test_tail_refusals(bf16):
    run = Run(S.make_case("tail", 3, 37, bf16=bf16, seed=82))
    kw, es = run.case["kw"], 2 if bf16 else 4
    entries = (None,) if bf16 else (None, "sopro_seanet_tail_f32")
    if not bf16:
        refused(run, "passes = 2", passes=2)
    for e in entries:
        refused(run, "h misaligned", entry=e, h_bytes=es)
        for k in ("w1", "w2", "wf"):
            refused(run, k + " misaligned", entry=e, **{k + "_bytes": 4})
        refused(run, "h stride % 4 / % 8", entry=e, h_seg_stride=kw["h_seg_stride"] + (4 if bf16 else 2))
        refused(run, "h stride too short", entry=e, h_seg_stride=(37 + 1) * 64)
        refused(run, "wav stride too short: two workgroups would write the same words", entry=e, wav_seg_stride=36)
        big = (1 << 31) - 1024   # the largest T taken is 2^31 - 1025
        msg = refused(run, "T at the bound", entry=e, T=big, h_seg_stride=(big + 2) * 64, wav_seg_stride=big)
        assert "T must stay at or below" in msg, msg


@pytest.mark.parametrize("bf16", [False, True])
def test_uptail_refusals(bf16):
    run = Run(S.make_case("uptail", 3, 37, bf16=bf16, seed=83))
    kw, es = run.case["kw"], 2 if bf16 else 4
    if not bf16:
        refused(run, "passes = 2", passes=2)
    refused(run, "x misaligned", x_bytes=es)
    for k in ("wu", "w1", "w2"):
        refused(run, k + " misaligned", **{k + "_bytes": 4})
    refused(run, "x stride % 4 / % 8", x_seg_stride=kw["x_seg_stride"] + (4 if bf16 else 2))
    refused(run, "x stride too short", x_seg_stride=37 * 128)
    refused(run, "wav stride too short", wav_seg_stride=4 * 37 - 1)
    big = ((1 << 31) - 1 - 256) // 4 + 1
    msg = refused(run, "T at the bound", T=big, x_seg_stride=(big + 1) * 128, wav_seg_stride=4 * big)
    assert "T must stay at or below" in msg, msg


def test_python_wrappers_take_passes():
    """hip.seanet_tail / hip.seanet_res128 with passes = 1 are the _p_f32 entry points (the sixteen-wave tail through the probe)."""
    for op, tiles in (("res128", 0), ("tail", -1)):
        case = S.make_case(op, 2, 37, seed=84)
        run = Run(case)
        kw, w = case["kw"], run.w
        out = run.out0.clone()
        h = run.d["in"][kw["h_off"]:]
        if op == "res128":
            fn, args = hip.seanet_res128, [h, w["w1"], w["b1"], w["w2"], w["b2"], out[kw["out_off"]:]]
            kws = dict(B=2, T=37, h_seg_stride=kw["h_seg_stride"], out_seg_stride=kw["out_seg_stride"])
        else:
            fn, args = hip.seanet_tail, [h, w["w1"], w["b1"], w["w2"], w["b2"], w["wf"], w["bf"], out[kw["wav_off"]:]]
            kws = dict(B=2, T=37, h_seg_stride=kw["h_seg_stride"], wav_seg_stride=kw["wav_seg_stride"])
        try:
            run.probe(tiles)
            rc, want = run.call(1)
            fn(*args, **kws, passes=1)
            torch.cuda.synchronize()
        finally:
            run.probe(0)
        assert rc == 0 and torch.equal(bits(out.cpu()), bits(want)), op
        with pytest.raises(hip.SoproHipError):
            fn(*args, **kws, passes=2)


def test_zz_print_the_worst_ratios():
    print(f"\nSEANET-EDGE launches: {COUNT['launches']}; staged bf16 values with a carried error: {COUNT['staged']}, of them charged the wide bound: {COUNT['wide']}")
    for grp in sorted(WORST):
        print(f"SEANET-EDGE WORST {grp}: {WORST[grp][0]:.3f}  ({WORST[grp][1]})")
