"""Word timestamps on the device: the path operator against its restatement (tests/align_ref.py, itself checked on the CPU by
tests/test_align_host.py) bit for bit, the scores operator and the engine's teacher-forced replay against the restatement within
tolerances derived from the restatement's own float32 / float64 difference, and the public interface end to end."""
import numpy as np
import pytest
import torch

import align_ref as R
from conftest import FakeTok
from sopro_amd import align as A
from sopro_amd import hip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GREEDY = dict(top_p=0.0, temperature=1.0, anti_loop=False)
CANARY = -7


# ------------------------------------------------------------------------------------------ 1. the path operator
def _designed_scores(rng, shapes, T_cap, S_cap, pitch):
    """A ragged batch: random log-probabilities, every third row small integers (real ties), padding = 999."""
    sc = np.full((len(shapes), T_cap, pitch), 999.0, dtype=np.float32)
    for b, (T, S) in enumerate(shapes):
        if b % 3 == 2:
            sc[b, :T, :S] = -rng.integers(0, 3, size=(T, S)).astype(np.float32)
        else:
            sc[b, :T, :S] = np.log(rng.uniform(1e-6, 1.0, size=(T, S))).astype(np.float32)
    return sc


def _check_paths(sc, shapes, S_cap, stream=None):
    B, T_cap = sc.shape[0], sc.shape[1]
    score = torch.from_numpy(sc).to(DEV)[:, :, :S_cap]
    assert score.stride(1) == sc.shape[2]
    tl, sl = [t for t, _s in shapes], [s for _t, s in shapes]
    path = torch.full((B, T_cap), CANARY, dtype=torch.int32, device=DEV)
    bounds = torch.full((B, S_cap, 2), CANARY, dtype=torch.int32, device=DEV)
    total = torch.full((B,), 777.0, device=DEV)
    status = torch.full((B,), CANARY, dtype=torch.int32, device=DEV)
    n0 = hip.align_calls
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            hip.align_paths(score, tl, sl, path=path, bounds=bounds, total=total, status=status)
        stream.synchronize()
    else:
        hip.align_paths(score, tl, sl, path=path, bounds=bounds, total=total, status=status)
        torch.cuda.synchronize()
    assert hip.align_calls == n0 + 1
    path, bounds, total, status = path.cpu().numpy(), bounds.cpu().numpy(), total.cpu().numpy(), status.cpu().numpy()
    for b, (T, S) in enumerate(shapes):
        w_path, w_bounds, w_total, w_status = R.dp(sc[b, :T, :S])
        assert status[b] == w_status, (b, T, S)
        assert path[b, :T].tolist() == w_path, (b, T, S)
        assert [tuple(v) for v in bounds[b, :S].tolist()] == [tuple(int(x) for x in v) for v in w_bounds], (b, T, S)
        assert total[b].tobytes() == np.float32(w_total).tobytes(), (b, T, S, total[b], w_total)
        assert (path[b, T:] == CANARY).all() and (bounds[b, S:] == CANARY).all(), (b, "something past a length was written")
    return status


def test_path_operator_one_wave_form():
    rng = np.random.default_rng(21)
    shapes = [(80, 57), (57, 57), (20, 1), (0, 5), (30, 40), (80, 12), (64, 33), (1, 1), (9, 0)]
    sc = _designed_scores(rng, shapes, 80, 57, pitch=59)  # rows 59 floats apart: not a multiple of 4
    status = _check_paths(sc, shapes, 57)
    assert status.tolist() == [0, 0, 0, 1, 1, 0, 0, 0, 1]


def test_path_operator_wide_form_on_a_side_stream():
    rng = np.random.default_rng(22)
    shapes = [(2100, 2048), (2048, 2048), (700, 65), (1500, 300), (100, 1000), (900, 129), (0, 7), (300, 1)]
    sc = _designed_scores(rng, shapes, 2100, 2048, pitch=2049)
    status = _check_paths(sc, shapes, 2048, stream=torch.cuda.Stream(device=DEV))
    assert status.tolist() == [0, 0, 0, 0, 1, 0, 1, 0]
    # the same rows cut to 64 text positions take the other form and give the same answer as the restatement again
    small = [(T, min(S, 64)) for T, S in shapes]
    _check_paths(np.ascontiguousarray(sc[:, :, :65]), small, 64)


def test_path_operator_recovers_a_planted_alignment():
    rng = np.random.default_rng(23)
    for S in (40, 300):
        dur = rng.integers(1, 5, size=S)
        want = np.repeat(np.arange(S), dur)
        T = len(want)
        sc = np.full((1, T, S), -4.0, np.float32)
        sc[0, np.arange(T), want] = 0.0
        sc = (sc - rng.uniform(0.0, 0.99, size=sc.shape)).astype(np.float32)
        path, bounds, _total, status = hip.align_paths(torch.from_numpy(sc).to(DEV), [T], [S])
        assert status.tolist() == [0] and path[0].tolist() == want.tolist()
        assert bounds[0, :, 1].tolist() == np.cumsum(dur).tolist()


# ------------------------------------------------------------------------------------------ 2. the scores operator
@pytest.mark.parametrize("T_cap,S_cap,lens", [(50, 70, [(50, 70), (17, 3), (33, 64)]), (11, 1100, [(11, 1100), (5, 257)])], ids=["S70", "S1100"])
def test_scores_operator(T_cap, S_cap, lens):
    g = torch.Generator().manual_seed(31 + S_cap)
    B, D = len(lens), 4 * 96
    layers = [(0b1011, 0), (0b0100, 1), (0b0000, 1), (0b1111, 2)]  # (head mask, mode): written, added to, an empty launch, finished
    n_sel = sum(bin(m).count("1") for m, _ in layers)
    Qs = [torch.randn(B, T_cap, D, generator=g) * 1.5 for _ in layers]
    KVs = [torch.randn(B, S_cap, 2 * D, generator=g) * 1.5 for _ in layers]  # keys are the left half of wider rows, as in the engine
    acc = torch.full((B, T_cap, S_cap), 123.0, device=DEV)
    tl, sl = [t for t, _ in lens], [s for _, s in lens]
    n0 = hip.align_calls
    for (mask, mode), q, kv in zip(layers, Qs, KVs):
        hip.align_scores(q.to(DEV), kv.to(DEV), tl, sl, acc, head_mask=mask, weight=1.0 / n_sel, mode=mode, H=4, ldk=2 * D)
    torch.cuda.synchronize()
    assert hip.align_calls == n0 + 4
    got = acc.cpu()
    tol_all = 0.0
    for b, (T, S) in enumerate(lens):
        ref = {}
        for dt in (torch.float32, torch.float64):
            a = sum(R.scores_layer(q[b, :T], kv[b, :S, :D], m, 1.0 / n_sel, dt) for (m, _), q, kv in zip(layers, Qs, KVs))
            ref[dt] = R.log_scores(a)
        tol = 16.0 * float((ref[torch.float32].double() - ref[torch.float64]).abs().max())
        err = float((got[b, :T, :S] - ref[torch.float32]).abs().max())
        print(f"scores operator S_cap={S_cap} row {b} (T={T}, S={S}): engine |dscore| max {err:.3e}, tolerance 16 x f32-vs-f64 = {tol:.3e}")
        tol_all = max(tol_all, tol)
        assert err <= tol, (b, err, tol)
        assert bool((got[b, T:] == 123.0).all()) and bool((got[b, :, S:] == 123.0).all()), "padding was written"
    assert tol_all > 0


# ------------------------------------------------------------------------------------------ 3. end to end
TEXT_LENS = [24, 13, 7, 18, 1]
MAX_FRAMES = 40


def _ids(n, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(1, 500, size=n))


def _ref_tq(seed=5):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 2048, size=(24, 32)))


def _sharpen(weights, cfg):
    out = dict(weights)
    for i in cfg.ar_xattn_layers:
        k = f"ar.x_attns.{i}.q_proj.weight"
        out[k] = (np.asarray(weights[k]) * np.float32(8.0)).astype(np.float32)
    return out


@pytest.fixture(scope="module")
def sharp(cfg, sopro_np_noeos, mimi_np):
    """The EOS-suppressed checkpoint with the three query projections scaled by 8 (sharper maps) -> (engine, oracle weights)."""
    from oracle import sopro_oracle as O
    from sopro_amd import SoproTTS

    wn = _sharpen(sopro_np_noeos, cfg)
    return SoproTTS.from_weights(cfg, wn, mimi_np, FakeTok(), device=DEV), O.to_torch(wn)


def _end_to_end(tts, w, cfg, bar):
    """``bar``: None = the rule of the scores test (16 x the restatement's float32 / float64 difference, where the CPU probability is
    >= 1e-6), else an absolute bound on |dscore|."""
    from oracle import sopro_oracle as O

    ids = [_ids(n, 40 + i) for i, n in enumerate(TEXT_LENS)]
    ref_tq = _ref_tq()
    ref = tts.prepare_reference(ref_tokens_tq=ref_tq)
    B = len(ids)
    kw = dict(max_frames=MAX_FRAMES, text_ids=ids, padded=True, seed=3, **GREEDY)
    n0 = hip.align_calls
    plain = tts.synthesize_batch([""] * B, [ref] * B, **kw)
    assert hip.align_calls == n0, "a call without alignment= launched the timing kernels"
    sink = []
    timed = tts.synthesize_batch([""] * B, [ref] * B, alignment=sink, **kw)
    torch.cuda.synchronize()
    assert hip.align_calls > n0
    # (a) the audio and the tokens do not know about the sink
    assert timed.lens == plain.lens and timed.frames == plain.frames
    assert torch.equal(timed.tokens, plain.tokens) and torch.equal(timed.wav, plain.wav)
    assert len(sink) == B and all(isinstance(a, A.Alignment) for a in sink)
    eng_scores = tts.model.align_last.cpu()
    oref = O.prepare_reference(ref_tq, w, cfg)
    compared, peaks = 0, []
    for b in range(B):
        T, S = timed.frames[b], TEXT_LENS[b]
        assert T >= MAX_FRAMES >= max(TEXT_LENS) and len(sink[b].path) == T and len(sink[b].token_frames) == S
        prep = O.prepare_conditioning(ids[b], oref, w, cfg, max_frames=MAX_FRAMES, style_strength=float(cfg.style_strength))
        c0 = timed.tokens[b, :T, 0].cpu()
        s32, a32 = R.utterance_scores(w, cfg, prep["cond_ar"][0], c0, prep["txt_seq"][0])
        got = eng_scores[b, :T, :S]
        # (b) the score matrix
        if bar is None:
            s64, _ = R.utterance_scores(w, cfg, prep["cond_ar"][0], c0, prep["txt_seq"][0], dtype=torch.float64)
            tol = 16.0 * float((s32.double() - s64).abs().max())
            where = a32 >= 1e-6
        else:
            tol, where = bar, torch.ones_like(a32, dtype=torch.bool)
        err = float((got - s32)[where].abs().max())
        peak = float(a32.max(dim=-1).values.mean())
        print(f"row {b} (T={T}, S={S}): engine |dscore| max {err:.3e}, tolerance {tol:.3e}, mean max probability {peak:.3f}, "
              f"confidence {sink[b].confidence:.4f}")
        assert err <= tol, (b, err, tol)
        # (c) the path is the restated path through the engine's own scores, exactly
        w_path, w_bounds, w_total, w_status = R.dp(got.numpy())
        assert sink[b].status == w_status == 0
        assert sink[b].path == w_path and [tuple(v) for v in sink[b].token_frames] == [tuple(int(x) for x in v) for v in w_bounds]
        assert np.float32(sink[b].total).tobytes() == np.float32(w_total).tobytes()
        assert sink[b].confidence == pytest.approx(float(np.exp(np.float64(w_total) / T)), rel=1e-6)
        # (d) scored on the CPU matrix, the engine's path is within 2 T tol of the CPU optimum
        cpu = s32.numpy()
        _p, _b, best, _s = R.dp(cpu)
        assert float(R.path_total(cpu, sink[b].path)) >= float(best) - 2.0 * T * tol, b
        compared += 1
        peaks.append(peak)
    assert compared == B  # (e) no row was left out
    return sink, peaks


def test_end_to_end_ordinary_checkpoint(tts_noeos, w_noeos, cfg):
    """|dscore| <= 1e-4: the project's fp32-mode bar (tests/conftest.py)."""
    _end_to_end(tts_noeos, w_noeos, cfg, 1e-4)
    # fewer frames than text positions: the fallback, from the engine
    tts = tts_noeos
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    sink = []
    out = tts.synthesize_batch([""], [ref], text_ids=[_ids(12, 77)], max_frames=8, padded=True, alignment=sink, **GREEDY)
    T = out.frames[0]
    assert T < 12 and sink[0].status == 1 and sink[0].total == 0.0 and sink[0].confidence == 0.0
    assert sink[0].path == [(t * 12) // T for t in range(T)]
    w_path, w_bounds, _t, _s = R.dp(np.zeros((T, 12), np.float32))
    assert sink[0].path == w_path and [tuple(v) for v in sink[0].token_frames] == w_bounds


def test_end_to_end_sharpened_checkpoint(sharp, cfg):
    tts, w = sharp
    _sink, peaks = _end_to_end(tts, w, cfg, None)
    assert peaks[0] > 2.0 / TEXT_LENS[0]  # (the scaled queries do sharpen the maps: this case is not the flat one again)


def test_selected_heads(tts_noeos):
    tts = tts_noeos
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    ids = [_ids(9, 50), _ids(15, 51)]
    kw = dict(max_frames=24, text_ids=ids, padded=True, seed=3, **GREEDY)
    every, one, early = [], [], []
    tts.synthesize_batch([""] * 2, [ref] * 2, alignment=every, **kw)
    s_all = tts.model.align_last.cpu().clone()
    tts.synthesize_batch([""] * 2, [ref] * 2, alignment=one, align_heads=[(5, 2)], **kw)
    s_one = tts.model.align_last.cpu().clone()
    tts.synthesize_batch([""] * 2, [ref] * 2, alignment=early, align_heads=[(1, 0), (1, 3)], **kw)  # (the stack stops after layer 1)
    s_early = tts.model.align_last.cpu().clone()
    assert not torch.equal(s_all[0, :24, :9], s_one[0, :24, :9]) and not torch.equal(s_one[0, :24, :9], s_early[0, :24, :9])
    for s in (s_all, s_one, s_early):  # every one is the log of a distribution over the text
        assert torch.allclose(s[1, :24, :15].exp().sum(-1), torch.ones(24), atol=1e-4)
    for bad in ([(2, 0)], [(1, 4)], [], [3]):
        with pytest.raises(ValueError):
            tts.synthesize_batch([""] * 2, [ref] * 2, alignment=[], align_heads=bad, **kw)


# ------------------------------------------------------------------------------------------ 4. the interface
def _char_tok(tts, text):
    tts.tokenizer.table[text] = [1 + (ord(c) % 500) for c in text]
    return [(i, i + 1) for i in range(len(text))]


def test_synthesize_timed(tts_noeos):
    tts = tts_noeos
    text = "  so, word timing works !"
    spans = _char_tok(tts, text)
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(ref=ref, max_frames=32, seed=11)  # sampled: the sampler's stream is part of the claim
    n0 = hip.align_calls
    want = tts.synthesize(text, **kw)
    assert hip.align_calls == n0
    with pytest.raises(TypeError, match="token_spans="):
        tts.synthesize_timed(text, **kw)  # this tokenizer has no character offsets
    res = tts.synthesize_timed(text, token_spans=spans, **kw)
    assert hip.align_calls > n0
    assert isinstance(res, A.TimedResult) and torch.equal(res.wav, want)
    T, S = len(res.alignment.path), len(spans)
    w_path, w_bounds, _t, w_status = R.dp(tts.model.align_last[0, :T, :S].cpu().numpy())
    assert res.alignment.status == w_status == 0 and res.alignment.path == w_path
    assert res.words == A.word_cues(text, spans, w_bounds)
    assert [c.text for c in res.words] == ["so,", "word", "timing", "works", "!"]
    assert all(0 <= c.start_sample <= c.end_sample <= T * 1920 and c.start_sample % 1920 == 0 for c in res.words)
    assert all(a.end_sample <= b.start_sample for a, b in zip(res.words, res.words[1:]))
    assert res.words[0].start_sample == w_bounds[2][0] * 1920  # the two leading blanks are silence in front of the first word
    # a speaking rate: the same audio as synthesize(speed=...), every cue through map_speed
    fast = tts.synthesize_timed(text, token_spans=lambda t: spans, speed=1.25, **kw)
    assert torch.equal(fast.wav, tts.synthesize(text, speed=1.25, **kw)) and fast.alignment.path == res.alignment.path
    step = hip.tsm_step(1.25)
    assert fast.words == [c._replace(start_sample=A.map_speed(c.start_sample, step), end_sample=A.map_speed(c.end_sample, step)) for c in res.words]
    assert fast.words[-1].end_sample <= int(fast.wav.shape[-1])


LONG_TEXT = "Hello there. This is a rather long sentence, with several clauses, that will not fit.\n\nA new paragraph begins here! Is it fine? Yes."


def test_synthesize_long_word_cues(tts_noeos):
    from sopro_amd.longform import split_text

    tts = tts_noeos
    segs = split_text(LONG_TEXT, max_chars=40)
    for s in segs:
        _char_tok(tts, s.text)
    spans_of = lambda t: [(i, i + 1) for i in range(len(t))]  # noqa: E731
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    longest = max(len(s.text) for s in segs)
    kw = dict(ref=ref, max_chars=40, max_frames=longest + 8, seed=3, **GREEDY)
    n0 = hip.align_calls
    plain = tts.synthesize_long(LONG_TEXT, keep_parts=True, **kw)
    assert hip.align_calls == n0 and plain.words is None
    with pytest.raises(TypeError, match="token_spans="):
        tts.synthesize_long(LONG_TEXT, word_cues=True, **kw)
    for speed in (1.0, 0.8):
        res = tts.synthesize_long(LONG_TEXT, keep_parts=True, word_cues=True, token_spans=spans_of, speed=speed, **kw)
        if speed == 1.0:
            assert torch.equal(res.wav, plain.wav) and res.segments == plain.segments and res.edges == plain.edges
        # the restated mapping: every segment's own alignment (the same rows through synthesize_batch), its cues, the join's edges
        n = len(segs)
        sink = []
        tts.synthesize_batch([s.text for s in segs], [ref] * n, max_frames=kw["max_frames"], seed=3, nonces=[(3 + k) & 0xFFFFFFFF for k in range(n)],
                             row_ids=[0] * n, alignment=sink, **GREEDY)
        sc = tts.model.align_last.cpu().numpy()
        want = []
        step = hip.tsm_step(speed)
        for k, s in enumerate(segs):
            T, S = len(sink[k].path), len(s.text)
            _p, w_bounds, _t, _s = R.dp(sc[k, :T, :S])
            (e0, e1), off = res.edges[k], res.segments[k][1]
            for c in A.word_cues(s.text, spans_of(s.text), w_bounds):
                a, b = (A.map_speed(v, step) if speed != 1.0 else v for v in (c.start_sample, c.end_sample))
                want.append(A.LongWordCue(c.text, c.char_start, c.char_end, off + min(max(a, e0), e1) - e0, off + min(max(b, e0), e1) - e0, k))
        assert res.words == want and len(res.words) == len(LONG_TEXT.split())
        for c in res.words:  # inside the segment's cue range, whole words of the segment's text
            _t, s0, s1 = res.segments[c.segment]
            assert s0 <= c.start_sample <= c.end_sample <= s1 and segs[c.segment].text[c.char_start:c.char_end] == c.text
        starts = [c.start_sample for c in res.words]
        assert starts == sorted(starts) and [c.segment for c in res.words] == sorted(c.segment for c in res.words)


def test_paths_without_timing_launch_nothing_and_refuse_the_keywords(tts_noeos):
    from sopro_amd.serving import SynthesisService

    tts = tts_noeos
    text = "no timing here"
    _char_tok(tts, text)
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(max_frames=12, **GREEDY)
    n0 = hip.align_calls
    tts.synthesize(text, ref=ref, **kw)
    tts.synthesize_batch([text, text], [ref, ref], **kw)
    tts.model.generate_tokens(tts.encode_text(text), ref, **kw)
    chunks = list(tts.stream(text, ref=ref, chunk_frames=6, **kw))
    rows = list(tts.stream_batch([text], [ref], chunk_frames=6, **kw))
    assert chunks and rows and hip.align_calls == n0
    for call in (lambda: tts.stream(text, ref=ref, alignment=[], **kw),
                 lambda: tts.stream(text, ref=ref, word_cues=True, **kw),
                 lambda: tts.stream_batch([text], [ref], alignment=[], **kw),
                 lambda: tts.stream_long(text, ref=ref, word_cues=True, **kw)):
        with pytest.raises(NotImplementedError, match="no word timing"):
            call()
    with SynthesisService(tts, max_batch=4, max_wait_ms=300.0, lanes=1) as svc:
        with pytest.raises(NotImplementedError, match="no word timing"):
            svc.submit(text, ref, alignment=[], **kw)
        with pytest.raises(NotImplementedError, match="no word timing"):
            svc.synthesize(text, ref, word_cues=True, **kw)
        with pytest.raises(TypeError):
            svc.submit(text, ref, no_such_keyword=1, **kw)
    svc = SynthesisService(tts, mode="continuous", max_batch=3, ar_parts=1, ar_cus=64, max_frames=40, max_text=64, poll_every=8, bulk_batch=2)
    try:
        with pytest.raises(NotImplementedError, match="continuous"):
            svc.submit(text, ref, alignment=[], **kw)
    finally:
        svc.close()
    assert hip.align_calls == n0


# ------------------------------------------------------------------------------------------ 5. bf16 mode
def test_bf16_mode_structure(cfg, sopro_np_noeos, mimi_np):
    """No numeric bar in bf16 mode (the tokens come from bf16 operands; the replay itself runs on fp32 operands): the path is monotone,
    starts at 0, ends at S - 1, covers every text position with a frame range, and the fallback is flagged."""
    from sopro_amd import SoproTTS

    tts = SoproTTS.from_weights(cfg, sopro_np_noeos, mimi_np, FakeTok(), device=DEV, precision="bf16")
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    lens = [19, 6, 30]
    sink = []
    out = tts.synthesize_batch([""] * 3, [ref] * 3, text_ids=[_ids(n, 60 + i) for i, n in enumerate(lens)], max_frames=24, padded=True,
                               alignment=sink, **GREEDY)
    for b, S in enumerate(lens):
        T, a = out.frames[b], sink[b]
        assert len(a.path) == T and len(a.token_frames) == S
        if T < S:
            assert a.status == 1 and a.path == [(t * S) // T for t in range(T)]
            continue
        assert a.status == 0 and a.path[0] == 0 and a.path[-1] == S - 1 and 0.0 < a.confidence <= 1.0
        assert all(0 <= y - x <= 1 for x, y in zip(a.path, a.path[1:]))
        assert all(a.path[f0:f1] == [s] * (f1 - f0) and f1 > f0 for s, (f0, f1) in enumerate(a.token_frames))
        assert np.isfinite(a.total)
