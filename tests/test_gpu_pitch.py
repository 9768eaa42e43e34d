"""Pitch on the device: ``hip.pitch_shift`` / ``hip.PitchShiftState`` (csrc/pitch.hip) against the numpy restatement
(tests/pitch_ref.py, itself checked on the CPU by tests/test_pitch_host.py), and ``pitch=`` through every public entry point.  Every
comparison is exact: the definition leaves no rounding freedom, so there is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

import longform_ref as R
import pitch_ref as PR
import tsm_ref as T
from conftest import golden
from sopro_amd import align as A
from sopro_amd import hip
from sopro_amd.longform import group_plan, pause_samples, split_text

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GREEDY = dict(top_p=0.0, temperature=1.0, anti_loop=False)
PAD = 777.0      # past a row's length in the input: must never reach the output
CANARY = -555.0  # past a row's out_len in the output: must survive
TILE = hip.PITCH_TILE


def _rows_on_device(rows, stride):
    """list of 1-D float32 arrays -> the device view [n, stride - 1] of a [n, stride] tensor with PAD past each length"""
    base = np.full((len(rows), stride), PAD, dtype=np.float32)
    for k, r in enumerate(rows):
        base[k, : len(r)] = r
    dev = torch.from_numpy(base).to(DEV)[:, : stride - 1]
    assert dev.stride(0) == stride
    return dev


def _check_one_shot(rows, pitches, *, stream=None, stride=None, out_stride=None):
    lens = [len(r) for r in rows]
    stride = stride if stride is not None else max(lens) + 2
    wav = _rows_on_device(rows, stride)
    want = [PR.shift(r, p) for r, p in zip(rows, pitches)]
    cap = max(len(y) for y in want) + 19
    out_buf = torch.full((len(rows), out_stride or cap), CANARY, device=DEV)[:, :cap]
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            out, out_lens = hip.pitch_shift(wav, lens, pitches, out=out_buf)
        stream.synchronize()
    else:
        out, out_lens = hip.pitch_shift(wav, lens, pitches, out=out_buf)
    torch.cuda.synchronize()
    assert out_lens == [len(y) for y in want]
    host = out_buf.cpu()
    for k, y in enumerate(want):
        assert torch.equal(host[k, : len(y)], torch.from_numpy(y)), f"row {k}: {int((host[k, :len(y)] != torch.from_numpy(y)).sum())} samples differ"
        assert bool((host[k, len(y):] == CANARY).all()), f"row {k}: something past out_len was written"
    assert not bool((host == PAD).any()), "a sample past a row's length reached the output"
    return out, out_lens


def _decoder_row(tts, frames=20):
    g = golden("full200")
    toks = torch.from_numpy(g["tokens"][:frames].astype(np.int64))
    wav = tts.codec.decode_full(toks)
    torch.cuda.synchronize()
    x = wav.reshape(-1).cpu().numpy()
    assert x.shape[0] == frames * 1920 and float(np.abs(x).max()) > 0
    return x


def _len_for(out_len, inc):
    """the shortest row whose output has ``out_len`` samples"""
    L = -(-(out_len * inc) // (1 << 32))
    assert PR.out_len(L, inc) == out_len
    return L


def test_operator_on_a_designed_ragged_batch(tts):
    noise = T.noise_with_silence(20000 / T.SR, seed=5, head=3000, tail=2500)
    noise[9000:12000] = 0                                    # a silent stretch inside
    inc5 = PR.inc_of(5.0)
    base = T.harmonic(150.0)
    rows = [T.glide(90.0, 140.0, 30000), noise, np.zeros(8000, np.float32), np.zeros(0, np.float32),
            base[:1], base[:31], base[:33], base[:64], base[:65], _decoder_row(tts), T.harmonic(120.0, seconds=0.5),
            T.glide(200.0, 120.0, _len_for(TILE - 1, inc5)), T.glide(200.0, 120.0, _len_for(TILE, inc5)), T.glide(200.0, 120.0, _len_for(TILE + 1, inc5)),
            T.glide(110.0, 230.0, 25001)]
    pitches = [-12.0, 12.0, -3.3, 5.0, -12.0, 12.0, 0.01, -3.3, 0.0, 0.01, 0.0, 5.0, 5.0, 5.0, -3.3]
    stride = max(len(r) for r in rows) + 3
    assert (stride % 4) != 0
    before = hip.pitch_calls
    out, out_lens = _check_one_shot(rows, pitches, stream=torch.cuda.Stream(device=DEV), stride=stride, out_stride=2 * 30000 + 21)
    assert hip.pitch_calls == before + 1                     # one launch for the whole batch
    assert out_lens[0] == 60000 and out_lens[1] == 10000 and out_lens[3] == 0 and out_lens[4] == 2 and out_lens[11:14] == [TILE - 1, TILE, TILE + 1]
    for k in (8, 10):                                        # pitch 0: the input, bit for bit
        assert out_lens[k] == len(rows[k]) and torch.equal(out[k, : out_lens[k]].cpu(), torch.from_numpy(rows[k]))
    assert not bool(out[2, : out_lens[2]].any())


def test_one_long_row():
    """400 frames in one row at -12 (1 536 000 outputs: n * inc passes 2^50) and at +12 (the widest input span per tile)."""
    g = golden("full200")
    voice = np.asarray(g["wav"], dtype=np.float32).reshape(-1)[: 200 * 1920]
    long_row = np.concatenate([voice, T.glide(100.0, 200.0, 200 * 1920, amp=0.3)])
    assert len(long_row) == 400 * 1920
    for pitch, n_out in ((-12.0, 2 * 400 * 1920), (12.0, 200 * 1920)):
        _, out_lens = _check_one_shot([long_row], [pitch])
        assert out_lens == [n_out]
    assert (n_out * 2 - 1) * (1 << 31) > 1 << 50


@pytest.mark.parametrize("sizes", [[1920], [6 * 1920], [1920, 700, 5000, 1, 479, 11520, 2400]], ids=["c1", "c6", "ragged"])
def test_chunked_state_equals_one_shot_on_the_device(sizes):
    rows = [T.glide(95.0, 170.0, 61440), T.noise_with_silence(2.56, seed=8, head=4000, tail=6000)[:61440], T.harmonic(130.0, seconds=2.6)[:61440]]
    assert all(len(r) == 61440 for r in rows)
    pitches = [-12.0, 4.2, 12.0]
    n_total = 61440
    wav = torch.from_numpy(np.stack(rows)).to(DEV)
    one, one_lens = hip.pitch_shift(wav, [n_total] * 3, pitches)
    st = hip.PitchShiftState(3, pitches, DEV)
    got = [[] for _ in rows]
    i = j = 0
    while i < n_total:
        n = min(sizes[j % len(sizes)], n_total - i)
        j += 1
        l1 = max(0, n - 7)
        lens = [n, l1, n] if len(sizes) > 1 else None                   # ragged: row 1 lags by up to 7 samples per call ...
        out, out_lens = st.feed(wav[:, i: i + n], lens)
        for b in range(3):
            got[b].append(out[b, : out_lens[b]].cpu())
        if lens is not None:                                             # ... and catches up in a call of its own
            fill = torch.zeros(3, n - l1, device=DEV)
            fill[1] = wav[1, i + l1: i + n]
            out, out_lens = st.feed(fill, [0, n - l1, 0])
            for b in range(3):
                got[b].append(out[b, : out_lens[b]].cpu())
        i += n
    out, out_lens = st.flush()
    for b in range(3):
        got[b].append(out[b, : out_lens[b]].cpu())
        y = torch.cat(got[b])
        want = torch.from_numpy(PR.shift(rows[b], pitches[b]))
        assert y.numel() == one_lens[b] == want.numel() and torch.equal(y, one[b, : one_lens[b]].cpu()) and torch.equal(y, want), b
    # the flush left a fresh state: the same rows again, in one piece
    out, out_lens = st.feed(wav, flush=True)
    assert out_lens == one_lens and all(torch.equal(out[b, : one_lens[b]], one[b, : one_lens[b]]) for b in range(3))


def test_bad_arguments_are_refused():
    wav = torch.zeros(2, 1000, device=DEV)
    with pytest.raises(ValueError):
        hip.pitch_shift(wav, [1000, 1000], 12.5)
    with pytest.raises(ValueError):
        hip.pitch_shift(wav, [1000, 1000], [1.0])
    with pytest.raises(hip.SoproHipError):
        hip.pitch_shift(wav, [1000, 1001], 3.0)
    with pytest.raises(hip.SoproHipError):
        hip.pitch_shift(wav, [1000, 1000], -12.0, out=torch.zeros(2, 1999, device=DEV))
    with pytest.raises(hip.SoproHipError):
        hip.pitch_shift(wav.cpu(), [1000, 1000], 3.0)
    with pytest.raises(hip.SoproHipError):
        hip.PitchShiftState(1, 3.0, "cpu")


# ------------------------------------------------------------------------------------------ end to end
TEXT = ("Hello there. This is a rather long sentence, with several clauses, that will not fit in forty characters.\n\n"
        "A new paragraph begins here! Is it fine? Yes.")
MAX_CHARS = 40


def _register(tts, text, max_chars=MAX_CHARS):
    segs = split_text(text, max_chars=max_chars)
    for s in segs:
        tts.tokenizer.table[s.text] = [1 + (ord(c) % 500) for c in s.text]
    return segs


def _ref_tq(seed=5):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 2048, size=(24, 32)))


def _restated(wav, speed=1.0, pitch=0.0):
    return torch.from_numpy(PR.chain(wav.reshape(-1).cpu().numpy(), speed, pitch))


def test_synthesize_and_synthesize_batch_with_pitch(tts_noeos):
    tts = tts_noeos
    texts = ["a first utterance", "the second one is longer than the first", "third"]
    for t in texts:
        tts.tokenizer.table[t] = [1 + (ord(c) % 500) for c in t]
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(max_frames=14, ref=ref)
    p0, t0 = hip.pitch_calls, hip.tsm_calls
    plain = tts.synthesize(texts[0], seed=21, **kw)
    again = tts.synthesize(texts[0], seed=21, pitch=0.0, **kw)
    assert (hip.pitch_calls, hip.tsm_calls) == (p0, t0) and torch.equal(plain, again)  # pitch 0: neither operator is entered
    assert plain.numel() == 15 * 1920
    for speed, pitch in ((1.0, -5.0), (1.0, 3.0), (0.8, 3.0), (1.25, -5.0)):
        got = tts.synthesize(texts[0], seed=21, speed=speed, pitch=pitch, **kw)
        torch.cuda.synchronize()
        want = _restated(plain, speed, pitch)
        assert tuple(got.shape) == (1, 1, want.numel()) and got.is_cuda and torch.equal(got.reshape(-1).cpu(), want), (speed, pitch)
        assert abs(want.numel() - plain.numel() / speed) <= 3
    assert (hip.pitch_calls, hip.tsm_calls) == (p0 + 4, t0 + 4)
    got = tts.synthesize(texts[0], seed=21, speed=2.0, pitch=12.0, **kw)   # speed == rho: the stretch is skipped
    assert (hip.pitch_calls, hip.tsm_calls) == (p0 + 5, t0 + 4) and torch.equal(got.reshape(-1).cpu(), _restated(plain, 2.0, 12.0))
    for bad in (dict(pitch=12.5), dict(pitch=float("nan")), dict(speed=2.0, pitch=-12.0), dict(speed=0.5, pitch=7.0), dict(speed=2.5)):
        with pytest.raises(ValueError):
            tts.synthesize(texts[0], **bad, **kw)
    assert (hip.pitch_calls, hip.tsm_calls) == (p0 + 5, t0 + 4)
    # a batch: one pitch per row, applied to the padded batch in one launch of each operator
    bkw = dict(max_frames=14, seed=4)
    p0, t0 = hip.pitch_calls, hip.tsm_calls
    base = tts.synthesize_batch(texts, [ref] * 3, **bkw)
    same = tts.synthesize_batch(texts, [ref] * 3, pitch=[0.0, 0.0, 0.0], **bkw)
    assert (hip.pitch_calls, hip.tsm_calls) == (p0, t0) and all(torch.equal(a, b) for a, b in zip(base, same))
    pitches = [-4.0, 0.0, 7.0]
    got = tts.synthesize_batch(texts, [ref] * 3, pitch=pitches, **bkw)
    assert (hip.pitch_calls, hip.tsm_calls) == (p0 + 1, t0 + 1)
    for b in range(3):
        want = _restated(base[b], 1.0, pitches[b])
        assert tuple(got[b].shape) == (1, 1, want.numel()) and torch.equal(got[b].reshape(-1).cpu(), want), b
    assert torch.equal(got[1], base[1])                                   # the row at 0 comes back bit for bit
    speeds = [0.9, 1.0, 1.4]
    both = tts.synthesize_batch(texts, [ref] * 3, speed=speeds, pitch=pitches, **bkw)
    assert all(torch.equal(both[b].reshape(-1).cpu(), _restated(base[b], speeds[b], pitches[b])) for b in range(3))
    pb = tts.synthesize_batch(texts, [ref] * 3, pitch=pitches, padded=True, **bkw)
    pb0 = tts.synthesize_batch(texts, [ref] * 3, padded=True, **bkw)
    assert pb.lens == [int(g.shape[-1]) for g in got] and torch.equal(pb.tokens, pb0.tokens) and pb.frames == pb0.frames == [15, 15, 15]
    assert all(torch.equal(pb.wav[b, : pb.lens[b]], got[b].reshape(-1)) for b in range(3))
    assert torch.equal(pb.wav[1, : pb.lens[1]], pb0.wav[1, : pb0.lens[1]])
    with pytest.raises(ValueError):
        tts.synthesize_batch(texts, [ref] * 3, pitch=[1.0, 1.0], **bkw)
    with pytest.raises(ValueError):
        tts.synthesize_batch(texts, [ref] * 3, speed=[1.0, 2.0, 1.0], pitch=[0.0, -12.0, 0.0], **bkw)


@pytest.mark.parametrize("cf", [6, 16])
def test_stream_with_pitch_is_the_chain_of_the_stream(tts_noeos, cf):
    tts = tts_noeos
    text = "a streamed utterance of some length"
    tts.tokenizer.table[text] = [1 + (ord(c) % 500) for c in text]
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq(6))
    kw = dict(ref=ref, max_frames=30, chunk_frames=cf, seed=12)
    p0, t0 = hip.pitch_calls, hip.tsm_calls
    plain = list(tts.stream(text, **kw))
    same = list(tts.stream(text, pitch=0.0, **kw))
    assert (hip.pitch_calls, hip.tsm_calls) == (p0, t0) and len(plain) >= 2
    assert len(same) == len(plain) and all(torch.equal(a, b) for a, b in zip(plain, same))
    whole = torch.cat(plain, -1)
    for speed, pitch in ((1.0, 4.0), (0.7, -6.0), (1.6, 3.0)):
        chunks = list(tts.stream(text, speed=speed, pitch=pitch, **kw))
        assert chunks and all(c.dim() == 2 and c.shape[0] == 1 and c.is_cuda for c in chunks)
        got = torch.cat(chunks, -1).reshape(-1).cpu()
        want = _restated(whole, speed, pitch)
        assert got.numel() == want.numel() and torch.equal(got, want), (speed, pitch)
    assert hip.pitch_calls > p0 and hip.tsm_calls > t0
    with pytest.raises(ValueError):
        tts.stream(text, pitch=-13.0, **kw)
    with pytest.raises(ValueError):
        tts.stream(text, speed=2.0, pitch=-3.0, **kw)


def test_long_form_with_pitch(tts):
    segs = _register(tts, TEXT)
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(max_frames=12, max_chars=MAX_CHARS, seed=3, ref=ref, **GREEDY)
    v, pitch = 1.3, 4.0
    p0, t0 = hip.pitch_calls, hip.tsm_calls
    base = tts.synthesize_long(TEXT, keep_parts=True, **kw)
    assert (hip.pitch_calls, hip.tsm_calls) == (p0, t0)
    res = tts.synthesize_long(TEXT, keep_parts=True, speed=v, pitch=pitch, **kw)
    torch.cuda.synchronize()
    assert hip.pitch_calls == p0 + len(res.groups) and hip.tsm_calls == t0 + len(res.groups) and len(res.parts) == len(segs)
    parts = [PR.chain(p.wav.reshape(-1).cpu().numpy(), v, pitch) for p in base.parts]
    for k, p in enumerate(parts):                                       # parts[k].wav is the shifted row, tokens are untouched
        assert torch.equal(res.parts[k].wav.reshape(-1).cpu(), torch.from_numpy(p)), k
        assert torch.equal(res.parts[k].tokens, base.parts[k].tokens), k
    lens = [len(p) for p in parts]
    rows = np.full((len(parts), max(1, max(lens))), PAD, dtype=np.float32)
    for k, p in enumerate(parts):
        rows[k, : lens[k]] = p
    gaps = [int(round(pause_samples(s.boundary) / v)) for s in segs]    # the pauses follow the rate only
    gaps[-1] = 0
    want, w_edges, w_offs = R.join(rows, lens, gaps)
    assert tuple(res.wav.shape) == (1, 1, want.shape[0]) and torch.equal(res.wav.reshape(-1).cpu(), torch.from_numpy(want))
    assert [list(e) for e in res.edges] == w_edges.tolist()
    assert res.segments == [(segs[k].text, int(w_offs[k]), int(w_offs[k] + w_edges[k, 1] - w_edges[k, 0])) for k in range(len(segs))]
    # streamed pieces concatenate to the one-shot result of the same plan
    pieces = list(tts.stream_long(TEXT, speed=v, pitch=pitch, **kw))
    whole = tts.synthesize_long(TEXT, plan="latency", speed=v, pitch=pitch, **kw)
    assert len(pieces) == len(group_plan(len(segs), "latency"))
    assert torch.equal(torch.cat(pieces, -1), whole.wav.reshape(1, -1))
    # pitch alone: the pauses are what they are without it
    only = tts.synthesize_long(TEXT, pitch=-3.0, **kw)
    gap = lambda r: [b[1] - a[2] for a, b in zip(r.segments, r.segments[1:])]
    assert gap(only) == gap(base) and gap(res) != gap(base)
    with pytest.raises(ValueError):
        tts.synthesize_long(TEXT, pitch=12.5, **kw)
    with pytest.raises(ValueError):
        tts.stream_long(TEXT, speed=2.0, pitch=-12.0, **kw)


def test_service_applies_each_request_s_own_pitch_in_one_batch(tts):
    """``pitch`` is no part of the batching key.  The same request is queued at 0, -4 and +6 (and another text at +2 and speed 1.2):
    all four run as the rows of ONE batch; the row at 0 comes back untouched (both operators are the identity there), so the
    shifted copies of that same row have an exact expectation - the restated chain over the 0 row."""
    from sopro_amd.serving import SynthesisService

    rng = np.random.default_rng(41)
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq(9))
    ids_a = torch.from_numpy(rng.integers(1, 500, size=17))
    ids_b = torch.from_numpy(rng.integers(1, 500, size=9))
    kw = dict(max_frames=12, **GREEDY)
    tts.tokenizer.table["a"], tts.tokenizer.table["b"] = ids_a.tolist(), ids_b.tolist()
    lone_a = tts.synthesize("a", ref=ref, **kw)
    lone_b = tts.synthesize("b", ref=ref, speed=1.2, pitch=2.0, **kw)
    torch.cuda.synchronize()
    svc = SynthesisService(tts, max_batch=4, max_wait_ms=500.0, lanes=2, ar_cus=64, ar_parts=1, ar_shared=False)
    try:
        futs = [svc.submit("", ref, text_ids=ids_a, pitch=0.0, **kw), svc.submit("", ref, text_ids=ids_a, pitch=-4.0, **kw),
                svc.submit("", ref, text_ids=ids_a, pitch=6.0, **kw), svc.submit("", ref, text_ids=ids_b, speed=1.2, pitch=2.0, **kw)]
        got = [f.result(timeout=180) for f in futs]
        assert svc.stats["batches"] == 1 and svc.stats["rows"] == 4
        with pytest.raises(ValueError):
            svc.submit("", ref, text_ids=ids_a, pitch=40.0, **kw)
        with pytest.raises(ValueError):
            svc.submit_long("One. Two.", ref, speed=2.0, pitch=-12.0, **kw)
        with pytest.raises(NotImplementedError):
            svc.submit_stream("", ref, text_ids=ids_a, pitch=1.0, **kw)
    finally:
        svc.close()
    assert got[0].shape == lone_a.shape and float((got[0] - lone_a).abs().max()) <= 1e-4 * float(lone_a.abs().max())
    assert torch.equal(got[1].reshape(-1).cpu(), _restated(got[0], 1.0, -4.0))
    assert torch.equal(got[2].reshape(-1).cpu(), _restated(got[0], 1.0, 6.0))
    assert got[3].shape == lone_b.shape


def test_synthesize_timed_with_pitch(tts_noeos):
    tts = tts_noeos
    text = "  so, word timing works !"
    tts.tokenizer.table[text] = [1 + (ord(c) % 500) for c in text]
    spans = [(i, i + 1) for i in range(len(text))]
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(ref=ref, max_frames=14, seed=11)
    res = tts.synthesize_timed(text, token_spans=spans, **kw)
    for speed, pitch in ((1.0, 3.0), (1.25, -5.0)):
        got = tts.synthesize_timed(text, token_spans=spans, speed=speed, pitch=pitch, **kw)
        assert torch.equal(got.wav, tts.synthesize(text, speed=speed, pitch=pitch, **kw)) and got.alignment.path == res.alignment.path
        step, inc = hip.prosody_step(speed, pitch)
        assert step != 480 << 16
        assert got.words == A.shift_cues(A.stretch_cues(res.words, step), inc)
        assert got.words[-1].end_sample <= got.wav.shape[-1] + 1 and got.words != res.words
    same = tts.synthesize_timed(text, token_spans=spans, pitch=0.0, **kw)
    assert torch.equal(same.wav, res.wav) and same.words == res.words


def test_pitch_is_refused_where_it_is_not_available(tts):
    from sopro_amd.serving import SynthesisService

    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq(9))
    tts.tokenizer.table["x"] = [3, 4, 5, 6]
    with pytest.raises(NotImplementedError):
        tts.stream_batch(["x"], [ref], pitch=1.0, max_frames=8)
    assert len(list(tts.stream_batch(["x"], [ref], pitch=0.0, max_frames=8, **GREEDY))) >= 1
    svc = SynthesisService(tts, mode="continuous", max_batch=3, ar_parts=1, ar_cus=64, max_frames=40, max_text=64, poll_every=8, bulk_batch=2)
    try:
        with pytest.raises(NotImplementedError):
            svc.submit("", ref, text_ids=torch.tensor([3, 4, 5, 6]), pitch=-2.0, max_frames=8, **GREEDY)
        ok = svc.submit("", ref, text_ids=torch.tensor([3, 4, 5, 6]), pitch=0.0, max_frames=8, **GREEDY).result(timeout=120)
        assert ok.dim() == 3
    finally:
        svc.close()
