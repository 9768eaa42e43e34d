"""Speaking rate on the device: ``hip.time_stretch`` / ``hip.TimeStretchState`` (csrc/tsm.hip) against the numpy restatement
(tests/tsm_ref.py, itself checked on the CPU by tests/test_tsm_host.py), and ``speed=`` through every public entry point.  Every
comparison is exact: the definition leaves no rounding freedom, so there is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

import longform_ref as R
import tsm_ref as T
from conftest import golden
from sopro_amd import hip
from sopro_amd.longform import group_plan, pause_samples, split_text

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GREEDY = dict(top_p=0.0, temperature=1.0, anti_loop=False)
PAD = 777.0      # past a row's length in the input: must never reach the output
CANARY = -555.0  # past a row's out_len in the output: must survive


def _rows_on_device(rows, pitch):
    """list of 1-D float32 arrays -> ([n, pitch] numpy with PAD past each length, the device view [n, pitch - 1] with that pitch)"""
    base = np.full((len(rows), pitch), PAD, dtype=np.float32)
    for k, r in enumerate(rows):
        base[k, : len(r)] = r
    dev = torch.from_numpy(base).to(DEV)[:, : pitch - 1]
    assert dev.stride(0) == pitch
    return base, dev


def _check_one_shot(rows, speeds, *, stream=None, pitch=None):
    lens = [len(r) for r in rows]
    pitch = pitch if pitch is not None else max(lens) + 1
    _, wav = _rows_on_device(rows, pitch)
    want = [T.tsm(r, s, True) for r, s in zip(rows, speeds)]
    cap = max(len(y) for y, _ in want) + 19
    out_buf = torch.full((len(rows), cap), CANARY, device=DEV)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            out, out_lens, deltas = hip.time_stretch(wav, lens, speeds, out=out_buf, deltas=True)
        stream.synchronize()
    else:
        out, out_lens, deltas = hip.time_stretch(wav, lens, speeds, out=out_buf, deltas=True)
    torch.cuda.synchronize()
    assert out_lens == [len(y) for y, _ in want]
    assert deltas == [d.tolist() for _, d in want]
    host = out_buf.cpu()
    for k, (y, _) in enumerate(want):
        assert torch.equal(host[k, : len(y)], torch.from_numpy(y)), f"row {k}: {int((host[k, :len(y)] != torch.from_numpy(y)).sum())} samples differ"
        assert bool((host[k, len(y):] == CANARY).all()), f"row {k}: something past out_len was written"
    assert not bool((host == PAD).any()), "a sample past a row's length reached the output"
    return out, out_lens, deltas


def _decoder_row(tts, frames=20):
    g = golden("full200")
    toks = torch.from_numpy(g["tokens"][:frames].astype(np.int64))
    wav = tts.codec.decode_full(toks)
    torch.cuda.synchronize()
    x = wav.reshape(-1).cpu().numpy()
    assert x.shape[0] == frames * 1920 and float(np.abs(x).max()) > 0
    return x


def test_operator_on_a_designed_ragged_batch(tts):
    noise = T.noise_with_silence(20000 / T.SR, seed=5, head=3000, tail=2500)
    noise[9000:12000] = 0                                    # a silent stretch inside
    rows = [T.glide(90.0, 140.0, 30000), T.glide(200.0, 120.0, 25001), noise, np.zeros(8000, np.float32), np.zeros(0, np.float32),
            T.harmonic(150.0)[:300], _decoder_row(tts), T.harmonic(120.0, seconds=0.5), T.harmonic(110.0)[:481], T.harmonic(220.0, seconds=1.0)]
    speeds = [0.5, 2.0, 1.3, 0.75, 1.5, 0.6, 1.17, 1.0, 2.0, 0.5]
    pitch = max(len(r) for r in rows) + 2
    assert (pitch % 4) != 0
    before = hip.tsm_calls
    out, out_lens, deltas = _check_one_shot(rows, speeds, stream=torch.cuda.Stream(device=DEV), pitch=pitch)
    assert hip.tsm_calls == before + 1                       # one launch for the whole batch
    assert out_lens[4] == 0 and out_lens[7] == len(rows[7]) and out_lens[8] == 240
    assert torch.equal(out[7, : out_lens[7]].cpu(), torch.from_numpy(rows[7]))   # speed 1.0: the input, bit for bit
    assert not any(deltas[3]) and not any(deltas[7])
    assert any(deltas[0]) and any(deltas[6]), "the search never moved: this case checks nothing"


def test_operator_on_a_full_size_batch():
    """32 ragged rows of up to 200 frames at mixed speeds and one 400-frame row at speed 0.5 (3200 blocks in one chain)."""
    rng = np.random.default_rng(17)
    g = golden("full200")
    voice = np.asarray(g["wav"], dtype=np.float32).reshape(-1)[: 200 * 1920]
    rows, speeds = [], []
    for k in range(32):
        n = int(rng.integers(40 * 1920, 200 * 1920 + 1))
        kind = k % 4
        if kind == 0:
            x = T.glide(float(rng.uniform(80, 120)), float(rng.uniform(150, 260)), n, amp=0.25)
        elif kind == 1:
            x = voice[:n].copy()
        elif kind == 2:
            x = T.noise_with_silence((n + 10) / T.SR, seed=100 + k, head=int(rng.integers(0, 9000)), tail=int(rng.integers(1, 9000)))[:n]
        else:
            x = (T.glide(140.0, 95.0, n, amp=0.2) + T.noise_with_silence((n + 10) / T.SR, seed=200 + k, head=0, tail=0, amp=0.01)[:n]).astype(np.float32)
        rows.append(np.ascontiguousarray(x[:n], dtype=np.float32))
        speeds.append(float(rng.choice([0.5, 0.8, 0.9, 1.1, 1.25, 1.5, 2.0])) if k else 2.0)
    rows[3] = rows[3][: 200 * 1920 - 3]
    _check_one_shot(rows, speeds)
    long_row = np.concatenate([voice, T.glide(100.0, 200.0, 200 * 1920, amp=0.3)])
    assert len(long_row) == 400 * 1920
    _, out_lens, deltas = _check_one_shot([long_row], [0.5])
    assert out_lens == [2 * 400 * 1920] and len(deltas[0]) == 3200


@pytest.mark.parametrize("sizes", [[1920], [6 * 1920], [16 * 1920], [1920, 700, 5000, 1, 479, 11520, 2400]], ids=["c1", "c6", "c16", "ragged"])
def test_chunked_state_equals_one_shot_on_the_device(sizes):
    rows = [T.glide(95.0, 170.0, 61440), T.noise_with_silence(2.56, seed=8, head=4000, tail=6000)[:61440], T.harmonic(130.0, seconds=2.6)[:61440]]
    assert all(len(r) == 61440 for r in rows)
    speeds = [0.5, 1.3, 2.0]
    n_total = 61440
    wav = torch.from_numpy(np.stack(rows)).to(DEV)
    one, one_lens, one_d = hip.time_stretch(wav, [n_total] * 3, speeds, deltas=True)
    st = hip.TimeStretchState(3, speeds, DEV)
    got, got_d = [[] for _ in rows], [[] for _ in rows]
    i = j = 0
    while i < n_total:
        n = min(sizes[j % len(sizes)], n_total - i)
        j += 1
        l1 = max(0, n - 7)
        lens = [n, l1, n] if len(sizes) > 1 else None                   # ragged: row 1 lags by up to 7 samples per call ...
        chunk = wav[:, i: i + n]
        out, out_lens, d = st.feed(chunk, lens, deltas=True)
        for b in range(3):
            assert out_lens[b] % 480 == 0
            got[b].append(out[b, : out_lens[b]].cpu())
            got_d[b] += d[b]
        if lens is not None:                                             # ... and catches up in a call of its own
            fill = torch.zeros(3, n - l1, device=DEV)
            fill[1] = wav[1, i + l1: i + n]
            out, out_lens, d = st.feed(fill, [0, n - l1, 0], deltas=True)
            for b in range(3):
                got[b].append(out[b, : out_lens[b]].cpu())
                got_d[b] += d[b]
        i += n
    out, out_lens, d = st.flush(deltas=True)
    for b in range(3):
        got[b].append(out[b, : out_lens[b]].cpu())
        got_d[b] += d[b]
        y = torch.cat(got[b])
        assert y.numel() == one_lens[b] and torch.equal(y, one[b, : one_lens[b]].cpu()), b
        assert got_d[b] == one_d[b], b
    want = T.tsm(rows[1], speeds[1])
    assert torch.equal(one[1, : one_lens[1]].cpu(), torch.from_numpy(want))
    # the flush left a fresh state: the same rows again, in one piece
    out, out_lens = st.feed(wav, flush=True)
    assert out_lens == one_lens and all(torch.equal(out[b, : one_lens[b]], one[b, : one_lens[b]]) for b in range(3))


def test_bad_arguments_are_refused():
    wav = torch.zeros(2, 1000, device=DEV)
    with pytest.raises(ValueError):
        hip.time_stretch(wav, [1000, 1000], 2.5)
    with pytest.raises(ValueError):
        hip.time_stretch(wav, [1000, 1000], [1.0])
    with pytest.raises(hip.SoproHipError):
        hip.time_stretch(wav, [1000, 1001], 1.5)
    with pytest.raises(hip.SoproHipError):
        hip.time_stretch(wav, [1000, 1000], 0.5, out=torch.zeros(2, 1999, device=DEV))
    with pytest.raises(hip.SoproHipError):
        hip.time_stretch(wav.cpu(), [1000, 1000], 1.5)


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


def _restated(wav, speed):
    return torch.from_numpy(T.tsm(wav.reshape(-1).cpu().numpy(), speed))


def test_synthesize_and_synthesize_batch_with_speed(tts_noeos):
    tts = tts_noeos
    texts = ["a first utterance", "the second one is longer than the first", "third"]
    for t in texts:
        tts.tokenizer.table[t] = [1 + (ord(c) % 500) for c in t]
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(max_frames=14, ref=ref)
    before = hip.tsm_calls
    plain = tts.synthesize(texts[0], seed=21, **kw)
    again = tts.synthesize(texts[0], seed=21, speed=1.0, **kw)
    assert hip.tsm_calls == before and torch.equal(plain, again)     # speed 1.0: the operator is not entered
    assert plain.numel() == 15 * 1920
    for v in (0.5, 0.8, 1.25, 2.0):
        got = tts.synthesize(texts[0], seed=21, speed=v, **kw)
        torch.cuda.synchronize()
        want = _restated(plain, v)
        assert tuple(got.shape) == (1, 1, want.numel()) and got.is_cuda and torch.equal(got.reshape(-1).cpu(), want), v
    assert hip.tsm_calls == before + 4
    with pytest.raises(ValueError):
        tts.synthesize(texts[0], speed=2.5, **kw)
    with pytest.raises(ValueError):
        tts.synthesize(texts[0], speed=0.0, **kw)
    # a batch: one rate per row, applied to the padded batch in one launch
    bkw = dict(max_frames=14, seed=4)
    before = hip.tsm_calls
    base = tts.synthesize_batch(texts, [ref] * 3, **bkw)
    same = tts.synthesize_batch(texts, [ref] * 3, speed=[1.0, 1.0, 1.0], **bkw)
    assert hip.tsm_calls == before and all(torch.equal(a, b) for a, b in zip(base, same))
    speeds = [0.6, 1.0, 1.9]
    got = tts.synthesize_batch(texts, [ref] * 3, speed=speeds, **bkw)
    assert hip.tsm_calls == before + 1
    for b in range(3):
        want = _restated(base[b], speeds[b])
        assert tuple(got[b].shape) == (1, 1, want.numel()) and torch.equal(got[b].reshape(-1).cpu(), want), b
    assert torch.equal(got[1], base[1])
    one = tts.synthesize_batch(texts, [ref] * 3, speed=1.5, **bkw)
    assert all(torch.equal(one[b].reshape(-1).cpu(), _restated(base[b], 1.5)) for b in range(3))
    pb = tts.synthesize_batch(texts, [ref] * 3, speed=speeds, padded=True, **bkw)
    pb0 = tts.synthesize_batch(texts, [ref] * 3, padded=True, **bkw)
    assert pb.lens == [int(g.shape[-1]) for g in got] and torch.equal(pb.tokens, pb0.tokens) and pb.frames == pb0.frames == [15, 15, 15]
    assert all(torch.equal(pb.wav[b, : pb.lens[b]], got[b].reshape(-1)) for b in range(3))
    with pytest.raises(ValueError):
        tts.synthesize_batch(texts, [ref] * 3, speed=[1.0, 1.0], **bkw)


@pytest.mark.parametrize("cf", [6, 16])
def test_stream_with_speed_is_the_stretch_of_the_stream(tts_noeos, cf):
    tts = tts_noeos
    text = "a streamed utterance of some length"
    tts.tokenizer.table[text] = [1 + (ord(c) % 500) for c in text]
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq(6))
    kw = dict(ref=ref, max_frames=30, chunk_frames=cf, seed=12)
    before = hip.tsm_calls
    plain = list(tts.stream(text, **kw))
    assert hip.tsm_calls == before and len(plain) >= 2
    whole = torch.cat(plain, -1)
    for v in (0.7, 1.6):
        chunks = list(tts.stream(text, speed=v, **kw))
        assert chunks and all(c.dim() == 2 and c.shape[0] == 1 and c.is_cuda for c in chunks)
        assert all(c.shape[1] % 480 == 0 for c in chunks[:-1])         # whole blocks until the flush
        got = torch.cat(chunks, -1).reshape(-1).cpu()
        want = _restated(whole, v)
        assert got.numel() == want.numel() and torch.equal(got, want), v
    assert hip.tsm_calls > before
    with pytest.raises(ValueError):
        tts.stream(text, speed=3.0, **kw)


def test_long_form_with_speed(tts):
    segs = _register(tts, TEXT)
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(max_frames=12, max_chars=MAX_CHARS, seed=3, ref=ref, **GREEDY)
    v = 1.3
    before = hip.tsm_calls
    base = tts.synthesize_long(TEXT, keep_parts=True, **kw)
    assert hip.tsm_calls == before
    res = tts.synthesize_long(TEXT, keep_parts=True, speed=v, **kw)
    torch.cuda.synchronize()
    assert hip.tsm_calls == before + len(res.groups) and len(res.parts) == len(segs)
    parts = [T.tsm(p.wav.reshape(-1).cpu().numpy(), v) for p in base.parts]
    for k, p in enumerate(parts):                                       # parts[k].wav is the stretched row, tokens are untouched
        assert torch.equal(res.parts[k].wav.reshape(-1).cpu(), torch.from_numpy(p)), k
        assert torch.equal(res.parts[k].tokens, base.parts[k].tokens), k
    lens = [len(p) for p in parts]
    rows = np.full((len(parts), max(1, max(lens))), PAD, dtype=np.float32)
    for k, p in enumerate(parts):
        rows[k, : lens[k]] = p
    gaps = [int(round(pause_samples(s.boundary) / v)) for s in segs]
    gaps[-1] = 0
    want, w_edges, w_offs = R.join(rows, lens, gaps)
    assert tuple(res.wav.shape) == (1, 1, want.shape[0]) and torch.equal(res.wav.reshape(-1).cpu(), torch.from_numpy(want))
    assert [list(e) for e in res.edges] == w_edges.tolist()
    assert res.segments == [(segs[k].text, int(w_offs[k]), int(w_offs[k] + w_edges[k, 1] - w_edges[k, 0])) for k in range(len(segs))]
    assert res.wav.shape[-1] < base.wav.shape[-1]
    # streamed pieces concatenate to the one-shot result of the same plan
    pieces = list(tts.stream_long(TEXT, speed=v, **kw))
    whole = tts.synthesize_long(TEXT, plan="latency", speed=v, **kw)
    assert len(pieces) == len(group_plan(len(segs), "latency"))
    assert torch.equal(torch.cat(pieces, -1), whole.wav.reshape(1, -1))
    with pytest.raises(ValueError):
        tts.synthesize_long(TEXT, speed=0.3, **kw)


def test_service_applies_each_request_s_own_speed_in_one_batch(tts):
    """``speed`` is no part of the batching key.  The same request is queued at 1.0, 0.8 and 1.5 (and another text at 1.7): all four
    run as the rows of ONE batch; the row at 1.0 comes back untouched (the operator is the identity there), so the stretched
    copies of that same row have an exact expectation - the restatement of the 1.0 row.  Against a lone ``synthesize`` the service
    is compared as tests/test_gpu_serving.py compares it (another batch shape sums in another order): equal lengths, 1e-4 of
    the peak on the unstretched row."""
    from sopro_amd.serving import SynthesisService

    rng = np.random.default_rng(41)
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq(9))
    ids_a = torch.from_numpy(rng.integers(1, 500, size=17))
    ids_b = torch.from_numpy(rng.integers(1, 500, size=9))
    kw = dict(max_frames=12, **GREEDY)
    tts.tokenizer.table["a"], tts.tokenizer.table["b"] = ids_a.tolist(), ids_b.tolist()
    lone_a = tts.synthesize("a", ref=ref, **kw)
    lone_a15 = tts.synthesize("a", ref=ref, speed=1.5, **kw)
    lone_b17 = tts.synthesize("b", ref=ref, speed=1.7, **kw)
    torch.cuda.synchronize()
    svc = SynthesisService(tts, max_batch=4, max_wait_ms=500.0, lanes=2, ar_cus=64, ar_parts=1, ar_shared=False)
    try:
        futs = [svc.submit("", ref, text_ids=ids_a, speed=1.0, **kw), svc.submit("", ref, text_ids=ids_a, speed=0.8, **kw),
                svc.submit("", ref, text_ids=ids_a, speed=1.5, **kw), svc.submit("", ref, text_ids=ids_b, speed=1.7, **kw)]
        got = [f.result(timeout=180) for f in futs]
        assert svc.stats["batches"] == 1 and svc.stats["rows"] == 4
        with pytest.raises(ValueError):
            svc.submit("", ref, text_ids=ids_a, speed=4.0, **kw)
        with pytest.raises(NotImplementedError):
            svc.submit_stream("", ref, text_ids=ids_a, speed=1.2, **kw)
    finally:
        svc.close()
    assert got[0].shape == lone_a.shape and float((got[0] - lone_a).abs().max()) <= 1e-4 * float(lone_a.abs().max())
    assert torch.equal(got[1].reshape(-1).cpu(), _restated(got[0], 0.8))
    assert torch.equal(got[2].reshape(-1).cpu(), _restated(got[0], 1.5))
    assert got[2].shape == lone_a15.shape and got[3].shape == lone_b17.shape
    print("service vs lone synthesize at 1.5: max |diff| / peak =", float((got[2] - lone_a15).abs().max()) / float(lone_a15.abs().max()))


def test_speed_is_refused_where_it_is_not_available(tts):
    from sopro_amd.serving import SynthesisService

    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq(9))
    tts.tokenizer.table["x"] = [3, 4, 5, 6]
    with pytest.raises(NotImplementedError):
        tts.stream_batch(["x"], [ref], speed=1.2, max_frames=8)
    assert len(list(tts.stream_batch(["x"], [ref], speed=1.0, max_frames=8, **GREEDY))) >= 1
    svc = SynthesisService(tts, mode="continuous", max_batch=3, ar_parts=1, ar_cus=64, max_frames=40, max_text=64, poll_every=8, bulk_batch=2)
    try:
        with pytest.raises(NotImplementedError):
            svc.submit("", ref, text_ids=torch.tensor([3, 4, 5, 6]), speed=1.2, max_frames=8, **GREEDY)
        ok = svc.submit("", ref, text_ids=torch.tensor([3, 4, 5, 6]), speed=1.0, max_frames=8, **GREEDY).result(timeout=120)
        assert ok.dim() == 3
    finally:
        svc.close()
