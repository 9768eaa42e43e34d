"""Formant control on the device: ``hip.formant_shift`` / ``hip.FormantState`` (csrc/formant.hip) against the float64 numpy
restatement (tests/formant_ref.py, itself checked on the CPU by tests/test_formant_host.py), and ``formant=`` through the public
entry points.  The operator is fp32 against float64, so that comparison has a tolerance (below); everything else here - rows at
sigma = 1, row independence, chunking, the public paths against the one-shot operator - is exact."""
import numpy as np
import pytest
import torch

import formant_ref as R
from sopro_amd import hip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GREEDY = dict(top_p=0.0, temperature=1.0, anti_loop=False)
PAD = 777.0      # past a row's length in the input: must never reach the output
CANARY = -555.0  # past a row's length in the output: must survive
LENS = (0, 1, 127, 128, 129, 511, 512, 513, 1920, 5000)
SIGMAS = (0.5, 2.0 ** (-3.0 / 12.0), 1.0, 2.0 ** (4.0 / 12.0), 2.0)
# What the device may deviate from the float64 restatement, relative to the row's peak.  The largest deviation over the designed
# rows (noise at every length above, the vowel, a full-scale row; the zero row is exact), measured on an MI355X against
# formant_ref.warp, is 1.212e-06 (the vowel at sigma = 2^(4/12); noise rows 1.2e-07 .. 2.3e-07; profiles/formant_check.md has the
# figure per row), MEASURED below; the test allows 4 x that: the factor covers the spread between inputs of fp32 accumulation over
# 512-point transforms and 32-term cosine sums.
MEASURED = 1.212e-06
TOL = 4.0 * MEASURED


def _inv(sigma) -> float:
    return float(np.float32(1.0 / float(sigma)))


_ROWS = None


def designed_rows():
    """[(name, x float32, inv, float64 reference)], built once: noise at the lengths around a hop and a frame with sigma drawn from
    SIGMAS, the vowel both ways, an all-zero row, a full-scale row."""
    global _ROWS
    if _ROWS is None:
        rng = np.random.default_rng(33)
        rows = []
        for i, n in enumerate(LENS):
            rows.append((f"noise{n}", (0.1 * rng.standard_normal(n)).astype(np.float32), _inv(SIGMAS[i % len(SIGMAS)])))
        v = R.vowel(7000).astype(np.float32)
        rows.append(("vowel_up", v, _inv(SIGMAS[3])))
        rows.append(("vowel_down", v, _inv(SIGMAS[1])))
        rows.append(("all_zero", np.zeros(3000, np.float32), _inv(SIGMAS[0])))
        full = rng.standard_normal(4000)
        rows.append(("full_scale", (full / np.abs(full).max()).astype(np.float32), _inv(SIGMAS[4])))
        rows.append(("noise_wide", (0.1 * rng.standard_normal(3001)).astype(np.float32), _inv(SIGMAS[0])))
        _ROWS = [(name, x, inv, x.astype(np.float64) if inv == 1.0 else R.warp(x, inv)) for name, x, inv in rows]
    return _ROWS


def _on_device(rows, stride):
    """list of 1-D float32 arrays -> the device view [n, stride - 1] of a [n, stride] tensor with PAD past each length"""
    base = np.full((len(rows), stride), PAD, dtype=np.float32)
    for k, r in enumerate(rows):
        base[k, : len(r)] = r
    dev = torch.from_numpy(base).to(DEV)[:, : stride - 1]
    assert dev.stride(0) == stride
    return dev


_BATCH = None


def batch_result():
    """The designed rows through one call (host copy [rows, cap] with the canary past the lengths), computed once."""
    global _BATCH
    if _BATCH is None:
        rows = designed_rows()
        xs = [x for _, x, _, _ in rows]
        lens = [len(x) for x in xs]
        stride = max(lens) + 3
        stride += 1 - stride % 2  # odd: no row but the first starts on a multiple of 4 floats, most not on a multiple of 2
        assert stride % 4 != 0
        wav = _on_device(xs, stride)
        out_buf = torch.full((len(rows), max(lens) + 7), CANARY, device=DEV)
        calls = hip.formant_calls
        out = hip.formant_shift(wav, lens, [inv for _, _, inv, _ in rows], out=out_buf)
        torch.cuda.synchronize()
        assert hip.formant_calls == calls + 1 and tuple(out.shape) == (len(rows), max(lens))
        _BATCH = out_buf.cpu().numpy()
    return _BATCH


def test_the_batch_against_float64():
    got = batch_result()
    worst = 0.0
    for k, (name, x, inv, want) in enumerate(designed_rows()):
        n = len(x)
        y = got[k, :n]
        assert np.isfinite(y).all(), name
        assert (got[k, n:] == CANARY).all(), f"{name}: something past the row's length was written"
        peak = float(np.abs(x).max()) if n else 0.0
        if peak == 0.0:
            assert not y.any(), f"{name}: a zero row gives zeros"
            continue
        err = float(np.abs(y.astype(np.float64) - want).max()) / peak
        print(f"{name}: n={n} inv={inv:.6f} max error / peak = {err:.3e}")
        worst = max(worst, err)
    print(f"largest: {worst:.3e}; allowed {TOL:.3e}")
    assert not (got == PAD).any(), "a sample past a row's length reached the output"
    assert worst <= TOL


def test_rows_at_sigma_one_and_row_independence():
    got = batch_result()
    rows = designed_rows()
    ones = [k for k, r in enumerate(rows) if r[2] == 1.0]
    assert len(ones) >= 2
    for k in ones:
        assert np.array_equal(got[k, : len(rows[k][1])], rows[k][1]), rows[k][0]  # bit for bit
    for k, (name, x, inv, _) in enumerate(rows):  # every row alone: the same bits as in the batch
        if len(x) == 0:
            continue
        alone = hip.formant_shift(torch.from_numpy(x).to(DEV).reshape(1, -1), [len(x)], [inv])
        assert tuple(alone.shape) == (1, len(x)) and np.array_equal(alone.cpu().numpy()[0], got[k, : len(x)]), name
    # a batch in which nothing has work launches nothing and hands the rows back
    wav = torch.from_numpy(rows[9][1]).to(DEV).reshape(1, -1)
    calls = hip.formant_calls
    same = hip.formant_shift(wav, [wav.shape[1]], 1.0)
    assert hip.formant_calls == calls and same.data_ptr() == wav.data_ptr()
    with pytest.raises(ValueError):
        hip.formant_shift(wav, [wav.shape[1]], [2.5])
    with pytest.raises(ValueError):
        hip.formant_shift(wav, [wav.shape[1]], [0.7])  # not an fp32 value: formant_inv was not used


@pytest.mark.parametrize("sizes", [[1, 100, 1920, 37], []], ids=["ragged", "one_chunk"])
def test_chunked_state_equals_one_shot(sizes):
    rows = designed_rows()
    x = np.stack([rows[9][1], rows[9][1][::-1].copy(), rows[9][1]])  # three rows of 5000
    invs = [_inv(SIGMAS[3]), _inv(SIGMAS[0]), 1.0]
    wav = torch.from_numpy(x).to(DEV)
    want = hip.formant_shift(wav, [5000] * 3, invs).cpu()
    st = hip.FormantState(3, invs, DEV)
    out, lens = st.flush()
    assert lens == [0, 0, 0] and out.shape[1] == 0  # a flush with nothing fed yields nothing
    for _ in range(2):  # (the state is fresh after a flush)
        pieces, pos, held_max = [], 0, 0
        for n in sizes + [5000 - sum(sizes)]:
            out, lens = st.feed(wav[:, pos: pos + n])
            pos += n
            assert lens[0] == lens[1] == lens[2] and lens[0] % hip.FM_H == 0 and out.shape[1] == lens[0]
            pieces.append(out)
            held_max = max(held_max, max(st.held))
        out, lens = st.flush()
        pieces.append(out)
        got = torch.cat(pieces, -1).cpu()
        assert held_max < hip.FM_N and tuple(got.shape) == (3, 5000)
        assert torch.equal(got, want)
        assert torch.equal(got[2], wav[2].cpu())
    # per-row lengths: a row that gets nothing in a call keeps what it holds
    st = hip.FormantState(2, invs[:2], DEV)
    a, la = st.feed(wav[:2, :3000], [3000, 1000])
    b, lb = st.feed(wav[:2, 3000:], [2000, 0], flush=True)
    assert la == [2560, 512] and lb == [2440, 488]
    assert torch.equal(torch.cat([a[0, : la[0]], b[0, : lb[0]]]).cpu(), want[0])
    alone = hip.formant_shift(wav[1:2, :1000], [1000], invs[1:2]).cpu()
    assert torch.equal(torch.cat([a[1, : la[1]], b[1, : lb[1]]]).cpu(), alone[0])


def _ref_tq(seed=5):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 2048, size=(24, 32)))


def _warp_of(wav, formant, pitch):
    """the one-shot operator over a finished waveform [1, 1, n]"""
    flat = wav.reshape(1, -1)
    return hip.formant_shift(flat, [flat.shape[1]], [hip.formant_inv(formant, pitch)]).reshape(1, 1, -1)


def test_synthesize_stream_and_batch_with_formant(tts_noeos):
    tts = tts_noeos
    texts = ["a first utterance", "the second one is longer than the first", "third"]
    for t in texts:
        tts.tokenizer.table[t] = [1 + (ord(c) % 500) for c in t]
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(max_frames=14, ref=ref, seed=7)
    calls = hip.formant_calls
    plain = tts.synthesize(texts[0], **kw)
    assert torch.equal(tts.synthesize(texts[0], formant=None, **kw), plain) and torch.equal(tts.synthesize(texts[0], formant=0.0, **kw), plain)
    shifted = tts.synthesize(texts[0], pitch=-3.0, **kw)
    assert torch.equal(tts.synthesize(texts[0], pitch=-3.0, formant=-3.0, **kw), shifted)
    assert hip.formant_calls == calls  # None and formant == pitch: the operator is not entered
    got = tts.synthesize(texts[0], pitch=-3.0, formant=0.0, **kw)
    assert hip.formant_calls == calls + 1
    want = _warp_of(shifted, 0.0, -3.0)
    assert got.shape == shifted.shape and got.is_cuda and torch.equal(got, want) and not torch.equal(got, shifted)
    assert torch.equal(tts.synthesize(texts[0], formant=2.0, **kw), _warp_of(plain, 2.0, 0.0))
    # the stream: the chunked chain, concatenated
    skw = dict(ref=ref, max_frames=14, chunk_frames=6, seed=7)
    whole = torch.cat(list(tts.stream(texts[0], pitch=-3.0, **skw)), -1)
    chunks = list(tts.stream(texts[0], pitch=-3.0, formant=0.0, **skw))
    assert len(chunks) >= 2 and all(c.dim() == 2 and c.shape[0] == 1 and c.is_cuda for c in chunks)
    assert torch.equal(torch.cat(chunks, -1).reshape(1, 1, -1), _warp_of(whole, 0.0, -3.0))
    # a batch: one value per row, None entries allowed
    bkw = dict(max_frames=14, seed=4)
    pitches, formants = [-4.0, 0.0, 2.0], [0.0, None, 2.0]
    calls = hip.formant_calls
    base = tts.synthesize_batch(texts, [ref] * 3, pitch=pitches, **bkw)
    same = tts.synthesize_batch(texts, [ref] * 3, pitch=pitches, formant=[-4.0, None, 2.0], **bkw)
    assert hip.formant_calls == calls and all(torch.equal(a, b) for a, b in zip(base, same))
    got = tts.synthesize_batch(texts, [ref] * 3, pitch=pitches, formant=formants, **bkw)
    assert hip.formant_calls == calls + 1
    assert torch.equal(got[0], _warp_of(base[0], 0.0, -4.0)) and torch.equal(got[1], base[1]) and torch.equal(got[2], base[2])
    one = tts.synthesize_batch(texts, [ref] * 3, formant=3.0, **bkw)
    plain_b = tts.synthesize_batch(texts, [ref] * 3, **bkw)
    assert all(torch.equal(one[b], _warp_of(plain_b[b], 3.0, 0.0)) for b in range(3))
    for bad in (dict(formant=12.5), dict(formant=float("nan")), dict(pitch=-6.0, formant=7.0)):
        with pytest.raises(ValueError):
            tts.synthesize(texts[0], **bad, **kw)
        with pytest.raises(ValueError):
            tts.stream(texts[0], **bad, **skw)
    with pytest.raises(ValueError):
        tts.synthesize_batch(texts, [ref] * 3, formant=[1.0, 2.0], **bkw)


def test_timed_cues_do_not_move_and_lockstep_refuses(tts_noeos):
    tts = tts_noeos
    text = "  so, word timing works !"
    tts.tokenizer.table[text] = [1 + (ord(c) % 500) for c in text]
    spans = [(i, i + 1) for i in range(len(text))]
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(ref=ref, max_frames=14, seed=11)
    res = tts.synthesize_timed(text, token_spans=spans, pitch=-3.0, **kw)
    got = tts.synthesize_timed(text, token_spans=spans, pitch=-3.0, formant=0.0, **kw)
    assert got.words == res.words and got.alignment.path == res.alignment.path
    assert torch.equal(got.wav, tts.synthesize(text, pitch=-3.0, formant=0.0, **kw)) and not torch.equal(got.wav, res.wav)
    tts.tokenizer.table["x"] = [3, 4, 5, 6]
    with pytest.raises(NotImplementedError, match="formant"):
        tts.stream_batch(["x"], [ref], formant=2.0, max_frames=8)
    assert len(list(tts.stream_batch(["x"], [ref], formant=0.0, max_frames=8, **GREEDY))) >= 1
