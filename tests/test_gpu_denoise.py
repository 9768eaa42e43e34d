"""Reference denoising on the GPU: ``hip.denoise`` against the float64 restatement (tests/denoise_ref.py) on the designed rows, its
pass-through, determinism, report and refusals, and the engine seam (``reference_waveform`` / ``encode_file`` / ``prepare_reference``
/ ``synthesize`` with ``denoise=``).

The bar of a row is 8 x the deviation of the restatement's own fp32 run from its float64 run on that row (at least one fp32 ulp of
the row's peak): it comes from the restatement, never from the library.  8, because the device orders its butterflies differently
and contracts to FMAs: a few ulps per stage over 9 stages; a wrong twiddle, window, hop, frame index or minimum-window edge shows
at 1e-3 or more.  Measured deviations per row: profiles/denoise_edges.md."""
import ctypes as C
import wave

import numpy as np
import pytest
import torch

import denoise_ref as R
from conftest import SEED

pytestmark = pytest.mark.gpu

PAD = 7.5e3     # what stands after a row's length in the input: it must reach no result
CANARY = -3.25  # what stands in ``out`` before the call: it must survive past a row's length


def _params(rows):
    from sopro_amd import Denoise

    return [Denoise(r.atten_db, r.bias) for r in rows]


def _run(rows, params=None, report=False, width_extra=3):
    """The rows in one call: odd row strides, PAD after each row's length, CANARY in out -> (out rows as numpy, canary intact, reports)."""
    from sopro_amd import hip

    lens = [len(r.x) for r in rows]
    width = max(max(lens), 1) + width_extra
    width += 1 - width % 2  # odd
    wav = np.full((len(rows), width), PAD, np.float32)
    for b, r in enumerate(rows):
        wav[b, : lens[b]] = r.x
    dwav = torch.from_numpy(wav).cuda()
    out = torch.full((len(rows), width + 2), CANARY, dtype=torch.float32, device="cuda:0")
    got = hip.denoise(dwav, lens, _params(rows) if params is None else params, out=out, report=report)
    reps = None
    if report:
        got, reps = got
    torch.cuda.synchronize()
    assert tuple(got.shape) == (len(rows), max(lens))
    host = out.cpu().numpy()
    intact = all(bool((host[b, lens[b]:] == CANARY).all()) for b in range(len(rows)))
    return [host[b, : lens[b]].copy() for b in range(len(rows))], intact, reps


@pytest.fixture(scope="module")
def batch_run():
    """The designed batch through one multi-row call (shared: the operator, report and pass-through tests read it)."""
    rows = R.designed_batch()
    ys, intact, reps = _run(rows, report=True)
    return rows, ys, intact, reps


def _dev(y, row):
    return float(np.abs(y.astype(np.float64) - R.reference(row)[0].y).max()) if len(row.x) else 0.0


def test_batch_matches_the_restatement(batch_run):
    rows, ys, intact, _ = batch_run
    assert intact, "the call wrote past a row's length"
    worst = []
    for row, y in zip(rows, ys):
        dev, bar, peak = _dev(y, row), R.bar(row), float(np.abs(row.x).max())
        print(f"{row.name:16s} n={len(row.x):6d} dev {dev:.3e} bar {bar:.3e} dev/peak {dev / peak if peak else 0.0:.3e} dev/bar {dev / bar if bar else 0.0:.2f}")
        if dev > bar:
            worst.append((row.name, dev, bar))
    assert not worst, worst


@pytest.mark.parametrize("row", R.designed_batch(), ids=lambda r: r.name)
def test_single_row_matches_the_restatement_and_the_batch(row, batch_run):
    rows, ys, _, _ = batch_run
    (y,), intact, _ = _run([row], width_extra=5)
    assert intact
    dev, bar = _dev(y, row), R.bar(row)
    print(f"{row.name}: dev {dev:.3e} bar {bar:.3e}")
    assert dev <= bar
    assert np.array_equal(y, ys[[r.name for r in rows].index(row.name)]), "a row's bits depend on the rows beside it"


def test_all_zero_row_gives_exact_zeros_and_the_scaled_row_is_finite(batch_run):
    rows, ys, _, _ = batch_run
    by = {r.name: y for r, y in zip(rows, ys)}
    assert np.array_equal(by["all_zero"], np.zeros_like(by["all_zero"]))
    assert bool(np.isfinite(by["scale20"]).all()) and float(np.abs(by["scale20"]).max()) > 1.0


def test_pass_through_rows_and_empty_rows_in_a_mixed_batch():
    from sopro_amd import Denoise

    all_rows = {r.name: r for r in R.designed_batch()}
    rows = [all_rows["len513"], all_rows["voice_white"], R.Row("empty", np.zeros(0, np.float32), 15.0, 3.0), all_rows["len129"],
            R.Row("empty_none", np.zeros(0, np.float32), 15.0, 3.0), all_rows["len12161"]]
    params = [None, Denoise(), Denoise(), None, None, Denoise(0.0, 3.0)]
    ys, intact, reps = _run(rows, params=params, report=True)
    assert intact
    assert np.array_equal(ys[0], rows[0].x) and np.array_equal(ys[3], rows[3].x), "a None row must come back bit for bit"
    assert len(ys[2]) == 0 and len(ys[4]) == 0
    assert _dev(ys[1], rows[1]) <= R.bar(rows[1])
    # atten_db = 0: the gain is 1 everywhere, the row comes back within the bar of its input
    ident = R.Row("len12161_ident", rows[5].x, 0.0, 3.0)
    dev = float(np.abs(ys[5].astype(np.float64) - rows[5].x.astype(np.float64)).max())
    print(f"atten_db = 0: |y - x| {dev:.3e}, bar {R.bar(ident):.3e}")
    assert dev <= R.bar(ident)
    assert reps[0] is None and reps[3] is None and reps[4] is None and reps[1] is not None and reps[5] is not None


def test_all_none_launches_nothing():
    from sopro_amd import hip

    x = torch.randn(2, 301, device="cuda:0")
    n0 = hip.denoise_calls
    y = hip.denoise(x, [300, 17], None)
    assert hip.denoise_calls == n0 and y.data_ptr() == x.data_ptr() and tuple(y.shape) == (2, 300)


def test_two_calls_give_the_same_bits(batch_run):
    rows, ys, _, reps = batch_run
    ys2, _, reps2 = _run(rows, report=True)
    for a, b in zip(ys, ys2):
        assert np.array_equal(a, b)
    assert reps == reps2


def test_report_matches_the_restatement(batch_run):
    rows, ys, _, reps = batch_run
    for row, rep in zip(rows, reps):
        p = R.reference(row)[0]
        print(f"{row.name:16s} input_db {rep.input_db:9.4f} ({p.input_db:9.4f})  removed_db {rep.removed_db:9.4f} ({p.removed_db:9.4f})")
        assert abs(rep.input_db - p.input_db) <= 0.01, row.name
        assert abs(rep.removed_db - p.removed_db) <= 0.01, row.name
        if row.name != "all_zero":
            assert rep.removed_db < 0.0


def test_bad_arguments_are_refused_and_nothing_is_launched():
    from sopro_amd import Denoise, hip

    lib = hip.load()
    n = 1000
    x = torch.randn(1, n, device="cuda:0")
    out = torch.full((1, n), CANARY, device="cuda:0")
    need = int(lib.sopro_denoise_workspace_bytes(1, n))
    ws = torch.empty(need // 8, dtype=torch.int64, device="cuda:0")
    lens = (C.c_int32 * 1)(n)

    def call(par, ws_bytes):
        return lib.sopro_denoise_rows_f32(x.data_ptr(), n, lens, (C.c_float * 2)(*par), 1, out.data_ptr(), n, None, ws.data_ptr(), ws_bytes, None)

    assert call((15.0, 3.0), need - 4) == -2 and b"ws_bytes" in lib.sopro_last_error()  # a workspace that is too small
    assert call((40.5, 3.0), need) == -2 and b"atten_db" in lib.sopro_last_error()      # a parameter out of range, handed over raw
    assert call((15.0, 0.5), need) == -2 and b"bias" in lib.sopro_last_error()
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()), "a refused call launched something"
    with pytest.raises(hip.SoproHipError, match="out must be"):                          # out too narrow
        hip.denoise(x, [n], Denoise(), out=torch.empty(1, n - 1, device="cuda:0"))
    with pytest.raises(hip.SoproHipError):
        hip.denoise(x, [n + 1], Denoise())
    with pytest.raises(ValueError):
        hip.denoise(x, [n], [Denoise(), Denoise()])
    assert call((15.0, 3.0), need) == 0
    torch.cuda.synchronize()
    assert not bool((out == CANARY).any())


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
def noisy_wav(tmp_path_factory):
    """The synthetic voice under white noise at 10 dB as a 16 kHz PCM16 file, so that the resampler runs."""
    sr = 16000
    _, x = R.noisy_voice(2.0, "white", snr=10.0, seed=31, sr=sr)
    path = str(tmp_path_factory.mktemp("dn") / "noisy.wav")
    with wave.open(path, "wb") as f:
        f.setnchannels(1), f.setsampwidth(2), f.setframerate(sr)
        f.writeframes(np.round(x * 32767).astype("<i2").tobytes())
    return path


def test_reference_waveform_is_the_restatement_of_the_resampled_clip(etts, noisy_wav):
    from sopro_amd import Denoise, audio

    codec, D = etts.codec, Denoise(20.0, 2.5)
    wav, sr = audio.load_audio_file(noisy_wav)
    wav = audio.trim_silence_energy(wav, sr)
    x = codec.resample(torch.from_numpy(np.ascontiguousarray(wav)).cuda(), sr, 24000).cpu().numpy()
    row = R.Row("engine_clip", x, D.atten_db, D.bias)
    want = R.reference(row)[0].y
    whole = codec.reference_waveform(noisy_wav, denoise=D).cpu().numpy()
    assert whole.shape == x.shape
    dev = float(np.abs(whole.astype(np.float64) - want).max())
    print(f"engine clip: n={len(x)} dev {dev:.3e} bar {R.bar(row):.3e}")
    assert dev <= R.bar(row)
    win = 12 * 1920  # round(1.0 s * 12.5 fps) frames
    s = (len(x) - win) // 2
    crop = codec.reference_waveform(noisy_wav, crop_seconds=1.0, denoise=D).cpu().numpy()
    assert crop.shape == (win,)
    assert float(np.abs(crop.astype(np.float64) - want[s: s + win]).max()) <= R.bar(row)
    assert np.array_equal(crop, whole[s: s + win]), "the denoiser must run before the crop"
    plain = codec.reference_waveform(noisy_wav).cpu().numpy()
    assert np.array_equal(plain, x)


def test_encode_file_and_prepare_reference_with_and_without_denoise(etts, noisy_wav):
    from sopro_amd import Denoise, DenoiseReport, hip

    codec, D = etts.codec, Denoise()
    codes_d = codec.encode_file(noisy_wav, crop_seconds=1.0, denoise=D)
    assert torch.equal(codes_d, codec.encode_waveform(codec.reference_waveform(noisy_wav, crop_seconds=1.0, denoise=D)))
    n0 = hip.denoise_calls
    codes = codec.encode_file(noisy_wav, crop_seconds=1.0)
    assert torch.equal(codes, codec.encode_file(noisy_wav, crop_seconds=1.0, denoise=None))
    assert torch.equal(codes, codec.encode_waveform(codec.reference_waveform(noisy_wav, crop_seconds=1.0)))
    ref = etts.prepare_reference(ref_audio_path=noisy_wav, ref_seconds=1.0)
    ref_none = etts.prepare_reference(ref_audio_path=noisy_wav, ref_seconds=1.0, denoise=None)
    assert hip.denoise_calls == n0, "denoise=None must launch nothing of the operator"
    assert torch.equal(ref.ref_tokens_btq, ref_none.ref_tokens_btq) and torch.equal(ref.sv_ref, ref_none.sv_ref) and torch.equal(ref.ref_seq, ref_none.ref_seq)
    assert torch.equal(ref.ref_tokens_btq.reshape(codes.shape).long(), codes)
    assert not torch.equal(codes, codes_d), "the denoised clip should not encode to the noisy clip's codes"
    sink = []
    ref_d = etts.prepare_reference(ref_audio_path=noisy_wav, ref_seconds=1.0, denoise=D, report=sink)
    assert len(sink) == 1 and isinstance(sink[0], DenoiseReport) and sink[0].removed_db < 0.0 and np.isfinite(sink[0].input_db)
    assert torch.equal(ref_d.ref_tokens_btq.reshape(codes_d.shape).long(), codes_d)


def test_synthesize_with_denoise_equals_synthesize_with_the_prepared_reference(etts, noisy_wav):
    from sopro_amd import Denoise

    D = Denoise()
    text = "a clean voice"
    etts.tokenizer.table[text] = [1 + (ord(c) % 500) for c in text]
    kw = dict(max_frames=8, seed=7, ref_seconds=1.0)
    ref_d = etts.prepare_reference(ref_audio_path=noisy_wav, ref_seconds=1.0, denoise=D)
    a = etts.synthesize(text, ref_audio_path=noisy_wav, denoise=D, **kw)
    b = etts.synthesize(text, ref=ref_d, **kw)
    assert a.numel() > 0 and torch.equal(a, b)
    with pytest.raises(ValueError, match="denoise="):
        etts.synthesize(text, ref=ref_d, denoise=D, **kw)
