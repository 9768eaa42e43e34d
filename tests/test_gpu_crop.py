"""Reference crop selection on the GPU: ``hip.speech_crop`` against the float64 restatement (tests/crop_ref.py) on the designed rows
- starts, lengths and output bits, per-block flags and energies, reports - its pass-through, determinism and refusals, and the
engine seam (``reference_waveform`` / ``encode_file`` / ``prepare_reference`` / ``synthesize`` with ``crop=``).

Equality is demanded, not closeness: tests/test_crop_host.py shows on the CPU that no designed row has a block within 1e-3 of its
threshold, and the device's e[f] is within 240 x 2^-24 = 1.4e-5 of the exact sum (the worst case of any order of a sum of 240
non-negative fp32 terms, asserted below), so every a[f] is the restatement's and everything after a[f] is integer.  Measured
deviations per row: profiles/crop_edges.md."""
import ctypes as C
import wave

import numpy as np
import pytest
import torch

import crop_ref as R
from conftest import SEED

pytestmark = pytest.mark.gpu

PAD = 7.5e3     # what stands after a row's length in the input: it must reach no result
CANARY = -3.25  # what stands in ``out`` before the call: it must survive past a row's out_len
E_BOUND = R.H * 2.0 ** -24


def _params(rows):
    from sopro_amd import SpeechCrop

    return [SpeechCrop(r.range_db, r.margin_db, r.clip_level, r.clip_weight) for r in rows]


def _run(rows, W, params=None, width_extra=3):
    """The rows in one call: odd row strides, PAD after each row's length, CANARY in out -> per row (out as numpy, report, (e,
    flags)), and whether the canary is intact."""
    from sopro_amd import hip

    lens = [len(r.x) for r in rows]
    width = max(max(lens), 1) + width_extra
    width += 1 - width % 2  # odd
    wav = np.full((len(rows), width), PAD, np.float32)
    for b, r in enumerate(rows):
        wav[b, : lens[b]] = r.x
    dwav = torch.from_numpy(wav).cuda()
    out = torch.full((len(rows), min(max(lens), W) + 5), CANARY, dtype=torch.float32, device="cuda:0")
    got, out_lens, reps, blks = hip.speech_crop(dwav, lens, _params(rows) if params is None else params, W, out=out, report=True, blocks=True)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (len(rows), min(max(lens), W)) and out_lens == [min(n, W) for n in lens]
    host = out.cpu().numpy()
    intact = all(bool((host[b, out_lens[b]:] == CANARY).all()) for b in range(len(rows)))
    return [(host[b, : out_lens[b]].copy(), reps[b], blks[b]) for b in range(len(rows))], intact


@pytest.fixture(scope="module")
def batch_run():
    """The designed batch: the W = 1920 rows through one multi-row call, the W = H row through its own (shared by the tests below)."""
    rows = R.designed_batch()
    got, ok = {}, True
    for W in sorted({r.W for r in rows}, reverse=True):
        sel = [r for r in rows if r.W == W]
        res, intact = _run(sel, W)
        ok = ok and intact
        got.update({r.name: v for r, v in zip(sel, res)})
    return rows, got, ok


def test_batch_starts_lengths_and_bits_are_the_restatement(batch_run):
    rows, got, intact = batch_run
    assert intact, "the call wrote past a row's out_len"
    for row in rows:
        y, rep, _ = got[row.name]
        p = R.reference(row)[0]
        print(f"{row.name:16s} n={len(row.x):7d} start {rep.start:7d} ({p.start:7d}) out_len {len(y)}")
        assert rep.start == p.start == row.start and len(y) == p.out_len, row.name
        assert np.array_equal(y, row.x[p.start: p.start + p.out_len]), row.name


@pytest.mark.parametrize("row", R.designed_batch(), ids=lambda r: r.name)
def test_single_row_gives_the_bits_it_gives_in_the_batch(row, batch_run):
    _, got, _ = batch_run
    ((y, rep, blk),), intact = _run([row], row.W, width_extra=6)
    assert intact
    yb, repb, blkb = got[row.name]
    assert np.array_equal(y, yb) and rep == repb
    assert np.array_equal(blk[0].view(np.uint32), blkb[0].view(np.uint32)) and np.array_equal(blk[1], blkb[1]), "a row's bits depend on the rows beside it"


def test_block_features_match_the_restatement(batch_run):
    rows, got, _ = batch_run
    print("| row | n | F | active | clipped | max |e_dev - e_64| / e_64 | bound | margin |")
    for row in rows:
        _, _, (e, flags) = got[row.name]
        p = R.reference(row)[0]
        assert len(e) == p.F and len(flags) == p.F, row.name
        assert np.array_equal(flags & 1, p.a) and np.array_equal(flags >> 1, p.c), row.name
        err = np.abs(e.astype(np.float64) - p.e)
        rel = float((err[p.e > 0] / p.e[p.e > 0]).max()) if (p.e > 0).any() else 0.0
        print(f"| {row.name} | {len(row.x)} | {p.F} | {int(p.a.sum())} | {int(p.c.sum())} | {rel:.3e} | {E_BOUND:.3e} | {R.margin(row):.3g} |")
        assert bool((err <= E_BOUND * p.e).all()), (row.name, rel)


def test_more_rows_than_one_launch_group(batch_run):
    """The rows travel to the kernels 64 at a time: 67 rows cross into a second group, whose rows must find their own workspace,
    starts and report slots."""
    rows, got, _ = batch_run
    small = [r for r in rows if r.W == R.W0 and len(r.x) < 10000]
    sel = [small[(5 * i) % len(small)] for i in range(67)]
    res, intact = _run(sel, R.W0)
    assert intact
    for r, (y, rep, blk) in zip(sel, res):
        yb, repb, blkb = got[r.name]
        assert np.array_equal(y, yb) and rep == repb and np.array_equal(blk[0].view(np.uint32), blkb[0].view(np.uint32)) and np.array_equal(blk[1], blkb[1]), r.name


def test_two_calls_give_the_same_bits(batch_run):
    rows, got, _ = batch_run
    sel = [r for r in rows if r.W == R.W0]
    res, _ = _run(sel, R.W0)
    for r, (y, rep, blk) in zip(sel, res):
        yb, repb, blkb = got[r.name]
        assert np.array_equal(y, yb) and rep == repb and np.array_equal(blk[0].view(np.uint32), blkb[0].view(np.uint32)) and np.array_equal(blk[1], blkb[1])


def test_report_matches_the_restatement(batch_run):
    rows, got, _ = batch_run
    for row in rows:
        rep, p = got[row.name][1], R.reference(row)[0]
        print(f"{row.name:16s} {tuple(rep[:7])} level_db {rep.level_db:9.4f} ({p.report.level_db:9.4f})")
        assert tuple(rep[:7]) == tuple(p.report[:7]), row.name
        Wb = row.W // R.H if len(row.x) > row.W else p.F
        if float(p.e[p.k: p.k + Wb].sum()) > 1e-12:  # (below that the + 1e-20 guard decides: ill-conditioned)
            assert abs(rep.level_db - p.report.level_db) <= 0.01, row.name


def test_pass_through_rows_and_empty_rows_in_a_mixed_batch():
    from sopro_amd import SpeechCrop

    by = {r.name: r for r in R.designed_batch()}
    empty = R.Row("empty", np.zeros(0, np.float32), R.W0)
    rows = [by["late"], by["early"], empty, by["nW"], empty, by["clipped_densest"]]
    params = [None, SpeechCrop(), SpeechCrop(), None, None, SpeechCrop()]
    res, intact = _run(rows, R.W0, params=params)
    assert intact
    assert np.array_equal(res[0][0], by["late"].x[: R.W0]), "a None row comes back as its first min(n, W) samples"
    assert np.array_equal(res[3][0], by["nW"].x)
    assert len(res[2][0]) == 0 and len(res[4][0]) == 0
    for b in (1, 5):
        p = R.reference(rows[b])[0]
        assert res[b][1].start == p.start and np.array_equal(res[b][0], rows[b].x[p.start: p.start + R.W0])
    assert [res[b][1] is None for b in range(6)] == [True, False, False, True, True, False]
    assert res[2][1].blocks == 0 and res[0][2] is None


def test_all_none_launches_nothing():
    from sopro_amd import hip

    x = torch.randn(2, 3001, device="cuda:0")
    n0 = hip.crop_calls
    y, lens = hip.speech_crop(x, [3000, 17], None, 1920)
    assert hip.crop_calls == n0 and y.data_ptr() == x.data_ptr() and tuple(y.shape) == (2, 1920) and lens == [1920, 17]


def test_bad_arguments_are_refused_and_nothing_is_launched():
    from sopro_amd import SpeechCrop, hip

    lib = hip.load()
    n, W = 5000, 1920
    x = torch.randn(1, n, device="cuda:0")
    out = torch.full((1, W), CANARY, device="cuda:0")
    starts = torch.full((1,), -7, dtype=torch.int32, device="cuda:0")
    need = int(lib.sopro_crop_workspace_bytes(1, n))
    ws = torch.empty(need // 4, dtype=torch.int32, device="cuda:0")
    lens = (C.c_int32 * 1)(n)

    def call(par=(30.0, 10.0, 0.999, 4.0), ws_bytes=need, win=W, lens_=lens):
        return lib.sopro_crop_rows_f32(x.data_ptr(), n, lens_, (C.c_float * 4)(*par), 1, win, out.data_ptr(), W, starts.data_ptr(), None, None,
                                       ws.data_ptr(), ws_bytes, None)

    assert call(ws_bytes=need - 4) == -2 and b"ws_bytes" in lib.sopro_last_error()
    assert call(par=(90.0, 10.0, 0.999, 4.0)) == -2 and b"range_db" in lib.sopro_last_error()
    assert call(par=(30.0, 50.0, 0.999, 4.0)) == -2 and b"margin_db" in lib.sopro_last_error()
    assert call(par=(30.0, 10.0, 9.0, 4.0)) == -2 and b"clip_level" in lib.sopro_last_error()
    assert call(par=(30.0, 10.0, 0.999, 1.5)) == -2 and b"clip_weight" in lib.sopro_last_error()
    assert call(win=W + 1) == -2 and b"win" in lib.sopro_last_error()
    assert call(lens_=(C.c_int32 * 1)(-1)) == -2 and b"lens" in lib.sopro_last_error()
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and int(starts[0]) == -7, "a refused call launched something"
    with pytest.raises(hip.SoproHipError, match="out must be"):                          # out too narrow
        hip.speech_crop(x, [n], SpeechCrop(), W, out=torch.empty(1, W - 1, device="cuda:0"))
    with pytest.raises(hip.SoproHipError):
        hip.speech_crop(x, [n + 1], SpeechCrop(), W)
    with pytest.raises(hip.SoproHipError, match="win"):
        hip.speech_crop(x, [n], SpeechCrop(), W + 7)
    with pytest.raises(ValueError):
        hip.speech_crop(x, [n], [SpeechCrop(), SpeechCrop()], W)
    with pytest.raises(TypeError):
        hip.speech_crop(x, [n], 30.0, W)
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out == CANARY).any()) and int(starts[0]) == (n - W) // 2  # white noise: no preference


# ---- the engine ----
@pytest.fixture(scope="module")
def enc_np(mc):
    from sopro_amd.weights import synth_mimi_weights
    return synth_mimi_weights(mc, SEED, with_encoder=True)


@pytest.fixture(scope="module")
def etts(cfg, sopro_np, enc_np):
    from conftest import FakeTok
    from sopro_amd import SoproTTS

    return SoproTTS.from_weights(cfg, sopro_np, enc_np, FakeTok(), device="cuda:0")


@pytest.fixture(scope="module")
def offcentre_wav(tmp_path_factory):
    """4 s at 16 kHz as a PCM16 file, so that the resampler runs: the voice over the first 0.15 s (it keeps the energy trim from
    cutting the front) and over 2.8 .. 3.9 s, white noise at 1e-3 elsewhere and a little of it over the voice: the middle is a pause."""
    sr = 16000
    x = R.clip_of(4 * sr, [(0, int(0.15 * sr)), (int(2.8 * sr), int(3.9 * sr))], seed=41, noise=1e-3, sr=sr)
    path = str(tmp_path_factory.mktemp("crop") / "offcentre.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(1), f.setsampwidth(2), f.setframerate(sr)
        f.writeframes(np.round(x * 32767).astype("<i2").tobytes())
    return path


WIN = 12 * 1920  # round(1.0 s * 12.5 fps) frames


def test_reference_waveform_takes_the_restatements_window(etts, offcentre_wav):
    from sopro_amd import CropReport, Denoise, SpeechCrop, hip

    codec, cr = etts.codec, SpeechCrop()
    whole = codec.reference_waveform(offcentre_wav).cpu().numpy()
    p = R.crop_parts(whole, WIN)
    s_c = (len(whole) - WIN) // 2
    print(f"engine clip: n={len(whole)} F={p.F} start {p.start} (centre {s_c}) active {p.report.active} / centre {p.report.centre_active}, margin "
          f"{float(np.abs(p.e / p.thr - 1.0).min()):.3g}")
    assert len(whole) > WIN and p.start > s_c and p.report.active > p.report.centre_active
    n0 = hip.crop_calls
    centre = codec.reference_waveform(offcentre_wav, crop_seconds=1.0)
    assert hip.crop_calls == n0 and np.array_equal(centre.cpu().numpy(), whole[s_c: s_c + WIN]), "crop=None is the centre crop, with nothing launched"
    assert np.array_equal(codec.reference_waveform(offcentre_wav, crop_seconds=1.0, crop=None).cpu().numpy(), whole[s_c: s_c + WIN]) and hip.crop_calls == n0
    sink = []
    got = codec.reference_waveform(offcentre_wav, crop_seconds=1.0, crop=cr, report=sink)
    assert hip.crop_calls == n0 + 1 and got.is_contiguous() and tuple(got.shape) == (WIN,)
    assert np.array_equal(got.cpu().numpy(), whole[p.start: p.start + WIN]) and not torch.equal(got, centre)
    assert len(sink) == 1 and isinstance(sink[0], CropReport) and tuple(sink[0][:7]) == tuple(p.report[:7])
    # with the denoiser: the window of the denoised whole clip, so the denoiser runs first and sees all of it
    D = Denoise()
    clean = codec.reference_waveform(offcentre_wav, denoise=D).cpu().numpy()
    q = R.crop_parts(clean, WIN)
    both = codec.reference_waveform(offcentre_wav, crop_seconds=1.0, denoise=D, crop=cr).cpu().numpy()
    assert np.array_equal(both, clean[q.start: q.start + WIN])
    with pytest.raises(ValueError, match="crop="):
        codec.reference_waveform(offcentre_wav, crop=cr)
    with pytest.raises(ValueError, match="crop="):
        codec.reference_waveform(offcentre_wav, crop_seconds=0.0, crop=cr)


def test_encode_file_and_prepare_reference_with_and_without_crop(etts, offcentre_wav):
    from sopro_amd import CropReport, Denoise, DenoiseReport, SpeechCrop, hip

    codec, cr = etts.codec, SpeechCrop()
    codes_c = codec.encode_file(offcentre_wav, crop_seconds=1.0, crop=cr)
    assert torch.equal(codes_c, codec.encode_waveform(codec.reference_waveform(offcentre_wav, crop_seconds=1.0, crop=cr)))
    n0 = hip.crop_calls
    codes = codec.encode_file(offcentre_wav, crop_seconds=1.0)
    assert torch.equal(codes, codec.encode_waveform(codec.reference_waveform(offcentre_wav, crop_seconds=1.0)))
    ref = etts.prepare_reference(ref_audio_path=offcentre_wav, ref_seconds=1.0)
    ref_none = etts.prepare_reference(ref_audio_path=offcentre_wav, ref_seconds=1.0, crop=None)
    sink = []
    etts.prepare_reference(ref_audio_path=offcentre_wav, ref_seconds=1.0, denoise=Denoise(), report=sink)
    assert hip.crop_calls == n0, "crop=None must launch nothing of the operator"
    assert len(sink) == 1 and isinstance(sink[0], DenoiseReport), "a call without crop= puts what it put before"
    assert torch.equal(ref.ref_tokens_btq, ref_none.ref_tokens_btq) and torch.equal(ref.sv_ref, ref_none.sv_ref) and torch.equal(ref.ref_seq, ref_none.ref_seq)
    assert torch.equal(ref.ref_tokens_btq.reshape(codes.shape).long(), codes)
    assert not torch.equal(codes, codes_c), "the speech window should not encode to the pause's codes"
    ref_c = etts.prepare_reference(ref_audio_path=offcentre_wav, ref_seconds=1.0, crop=cr)
    assert torch.equal(ref_c.ref_tokens_btq.reshape(codes_c.shape).long(), codes_c)
    sink = []
    etts.prepare_reference(ref_audio_path=offcentre_wav, ref_seconds=1.0, denoise=Denoise(), crop=cr, report=sink)
    assert [type(v) for v in sink] == [DenoiseReport, CropReport]


def test_synthesize_with_crop_equals_synthesize_with_the_prepared_reference(etts, offcentre_wav):
    from sopro_amd import SpeechCrop

    cr = SpeechCrop()
    text = "the right stretch"
    etts.tokenizer.table[text] = [1 + (ord(c) % 500) for c in text]
    kw = dict(max_frames=8, seed=7, ref_seconds=1.0)
    ref_c = etts.prepare_reference(ref_audio_path=offcentre_wav, ref_seconds=1.0, crop=cr)
    a = etts.synthesize(text, ref_audio_path=offcentre_wav, crop=cr, **kw)
    b = etts.synthesize(text, ref=ref_c, **kw)
    assert a.numel() > 0 and torch.equal(a, b)
    with pytest.raises(ValueError, match="crop="):
        etts.synthesize(text, ref=ref_c, crop=cr, **kw)
    with pytest.raises(ValueError, match="crop="):
        etts.synthesize(text, ref_audio_path=offcentre_wav, crop=cr, max_frames=8, seed=7, ref_seconds=0.0)
