"""Streaming word timestamps on the device: ``hip.align_online`` against its restatement (tests/align_online_ref.py, itself checked
on the CPU by tests/test_align_online_host.py) bit for bit after every step, against the offline operator where one window covers
the row, ``AlignStream``'s incremental score rows against ``align_batch``'s, and ``SoproTTS.stream_timed`` end to end."""
import numpy as np
import pytest
import torch

import align_online_ref as O
from sopro_amd import align as A
from sopro_amd import hip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GREEDY = dict(top_p=0.0, temperature=1.0, anti_loop=False)
CANARY = -7
SHAPES = [(63, 63), (60, 40), (150, 57), (200, 300), (40, 1), (1, 1), (0, 5), (130, 1500)]  # (T, S): rows end at different steps
T_CAP, S_CAP = 200, 2048
PITCH = S_CAP + 59  # floats between score rows: odd, so that no row but the first is aligned


def _scores(rng, shapes, T_cap, pitch):
    """A ragged batch: random log-probabilities, every third row small integers (real ties; no -0.0), padding = 999."""
    sc = np.full((len(shapes), T_cap, pitch), 999.0, dtype=np.float32)
    for b, (T, S) in enumerate(shapes):
        if b % 3 == 2:
            sc[b, :T, :S] = (-rng.integers(0, 3, size=(T, S))).astype(np.float32)
        else:
            sc[b, :T, :S] = np.log(rng.uniform(1e-6, 1.0, size=(T, S))).astype(np.float32)
    return sc


@pytest.fixture(scope="module")
def batch():
    """The score batch on the host and on the device, made once and left unchanged."""
    sc = _scores(np.random.default_rng(77), SHAPES, T_CAP, PITCH)
    score = torch.from_numpy(sc).to(DEV)[:, :, :S_CAP]
    assert score.stride(1) == PITCH
    return sc, score


def _run_schedule(sc, score, shapes, chunk, lag, stream=None):
    B, T_cap = sc.shape[0], sc.shape[1]
    rows = [O.Online(S, lag) for _T, S in shapes]
    state = hip.align_online_state(B, DEV)
    path = torch.full((B, T_cap), CANARY, dtype=torch.int32, device=DEV)
    sl = [S for _T, S in shapes]
    t, n_launch = 0, 0
    done = [False] * B
    while not all(done):
        t += chunk
        t1s = [min(t, T) for T, _S in shapes]
        finals = [int(t >= T) for T, _S in shapes]  # a row ends at the step that reaches its length: finals are mixed within a launch
        n0 = hip.align_calls
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                hip.align_online(score, t1s, sl, finals, lag, state, path)
            stream.synchronize()
        else:
            hip.align_online(score, t1s, sl, finals, lag, state, path)
            torch.cuda.synchronize()
        assert hip.align_calls == n0 + 1
        n_launch += 1
        st, pa = state.cpu().numpy(), path.cpu().numpy()
        for b, (T, S) in enumerate(shapes):
            if not done[b]:
                rows[b].step(sc[b, :, :S], t1s[b], bool(finals[b]))
            r = rows[b]
            assert tuple(int(v) for v in st[b, :4]) == r.state(), (chunk, lag, t, b, st[b], r.state())
            assert st[b, 4:5].view(np.float32)[0].tobytes() == np.float32(r.base).tobytes(), (chunk, lag, t, b)
            assert pa[b, : r.c + 1].tolist() == r.path, (chunk, lag, t, b)
            assert (pa[b, r.c + 1:] == CANARY).all(), (chunk, lag, t, b, "something past the committed frontier was written")
            done[b] = done[b] or bool(finals[b])
    for b, (T, S) in enumerate(shapes):
        assert rows[b].c == T - 1 and len(rows[b].path) == T
    return rows, n_launch


@pytest.mark.parametrize("chunk,lag", [(1, 0), (6, 8), (16, 47)])
def test_operator_against_the_restatement(batch, chunk, lag):
    sc, score = batch
    rows, n = _run_schedule(sc, score, SHAPES, chunk, lag)
    assert n == -(-200 // chunk)
    print(f"chunk {chunk}, lag {lag}: statuses {[r.status for r in rows]}, last positions {[r.p for r in rows]}")
    assert rows[4].path == [0] * 40 and rows[5].path == [0] and rows[6].path == [] and rows[6].state() == (-1, -1, 0, 0)


def test_operator_on_a_side_stream(batch):
    sc, score = batch
    _run_schedule(sc, score, SHAPES, 6, 8, stream=torch.cuda.Stream(device=DEV))


def test_one_window_equals_the_offline_operator():
    """Lag 63 on rows of up to 63 frames: one final step, which must be ``hip.align_paths`` in path and total, bit for bit."""
    shapes = [(63, 63), (60, 40), (40, 1), (1, 1), (63, 7), (17, 17), (33, 20)]
    sc = _scores(np.random.default_rng(5), shapes, 63, 64 + 59)
    score = torch.from_numpy(sc).to(DEV)[:, :, :64]
    tl, sl = [T for T, _S in shapes], [S for _T, S in shapes]
    w_path, _bounds, w_total, w_status = hip.align_paths(score, tl, sl)
    B = len(shapes)
    state = hip.align_online_state(B, DEV)
    path = torch.full((B, 63), CANARY, dtype=torch.int32, device=DEV)
    for t in (20, 40, 62):  # nothing can be committed before the row is final
        hip.align_online(score, [min(t, T - 1) for T in tl], sl, [0] * B, 63, state, path)
    assert (path.cpu() == CANARY).all() and state.cpu().tolist() == [[-1, -1, 0, 0, 0]] * B
    hip.align_online(score, tl, sl, [1] * B, 63, state, path)
    torch.cuda.synchronize()
    st, pa, wp, wt = state.cpu().numpy(), path.cpu().numpy(), w_path.cpu().numpy(), w_total.cpu().numpy()
    assert (w_status.cpu().numpy() == 0).all()
    for b, (T, S) in enumerate(shapes):
        assert pa[b, :T].tolist() == wp[b, :T].tolist() and (pa[b, T:] == CANARY).all(), b
        assert st[b, :4].tolist() == [T - 1, S - 1, 0, S - 1], b
        assert st[b, 4:5].view(np.float32)[0].tobytes() == wt[b].tobytes(), b
    # a window of 64 frames is refused on the device: status 3, nothing else written
    sc64 = torch.zeros(1, 64, 4, device=DEV)
    state, path = hip.align_online_state(1, DEV), torch.full((1, 64), CANARY, dtype=torch.int32, device=DEV)
    hip.align_online(sc64, [64], [4], [1], 0, state, path)
    assert state.cpu().tolist() == [[-1, -1, 3, 0, 0]] and (path.cpu() == CANARY).all()


# ------------------------------------------------------------------------------------------ the engine
def _ref_tq():
    return torch.from_numpy(np.random.default_rng(9).integers(0, 2048, size=(24, 32)))


def _char_tok(tts, text):
    tts.tokenizer.table[text] = [1 + (ord(c) % 500) for c in text]
    return [(i, i + 1) for i in range(len(text))]


def test_incremental_scores_equal_align_batch(tts_noeos, cfg):
    """``AlignStream`` over a fixed greedy history of more than 150 frames in chunks of 6 (from frame 138 on the window starts past
    frame 0: the halo), then ``align_batch`` over the same history: the same score rows, bit for bit - for every head, for heads of
    the first attention layer alone (the layers past it only finish the scores) and for one head of the last layer."""
    tts = tts_noeos
    model = tts.model
    ids = torch.tensor([1 + (7 * i) % 500 for i in range(23)])
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    max_frames = 160
    toks = model.generate_tokens(ids, ref, max_frames=max_frames, style_strength=float(cfg.style_strength), **GREEDY)
    hist = [int(v) for v in toks[:, 0].cpu().tolist()]
    T = len(hist)
    assert T >= 150 and int(cfg.rf_ar()) - 1 + 6 < T
    prep = model.prepare_conditioning(ids, ref, max_frames=max_frames, style_strength=float(cfg.style_strength))
    S = int(prep["txt_seq"].shape[1])
    hist_d = torch.zeros(1, max_frames + 1, dtype=torch.long, device=DEV)
    hist_d[0, :T] = torch.tensor(hist)
    for heads in (None, [(1, 0), (1, 3)], [(5, 2)]):
        al = model.align_stream(prep, max_frames=max_frames, lag_frames=8, chunk_frames=6, heads=heads)
        n0 = hip.align_calls
        rows = O.Online(S, 8)
        for t1, final in O.schedule(T, 6, stream=True):
            new = al.step(hist, t1, final)
            if heads is not None:
                continue
            got = al.scores()[0].cpu().numpy()
            assert got.shape == (t1, S)
            assert new == rows.step(got, t1, final), t1      # the path through the rows scored so far, as the restatement walks it
            assert al.state_host == rows.state() and np.float32(al.base).tobytes() == np.float32(rows.base).tobytes()
        assert hip.align_calls > n0 and len(al.path) == T and (heads is not None or al.path == rows.path)
        streamed = al.scores()[0].cpu().clone()
        model.align_batch({"txt_seq": prep["txt_seq"], "text_lens_host": [S]}, {"lens": [T], "B": 1, "hist": hist_d, "cond_ar": prep["cond_ar"]},
                          heads=heads)
        whole = model.align_last[0, :T, :S].cpu()
        diff = float((streamed - whole).abs().max())
        print(f"heads {heads}, T = {T}, S = {S}: streamed score rows against align_batch, max |d| = {diff:.3e}")
        assert torch.allclose(whole.exp().sum(-1), torch.ones(T), atol=1e-4), heads
        assert torch.equal(streamed, whole), heads


TEXT = "  so, streamed word timing works !"


def _cat(chunks):
    chunks = [c for c in chunks if c is not None and c.numel() > 0]
    return torch.cat(chunks, dim=-1) if chunks else torch.zeros(1, 0, device=DEV)


@pytest.mark.parametrize("fxkw", [dict(), dict(speed=1.25, pitch=-2.0), "watermark"], ids=["plain", "speed_pitch", "watermark"])
def test_stream_timed_end_to_end(tts_noeos, fxkw):
    from sopro_amd import Watermark, effects

    tts = tts_noeos
    if fxkw == "watermark":
        fxkw = dict(watermark=Watermark(key=12345, tag=3))
    spans = _char_tok(tts, TEXT)
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(ref=ref, max_frames=44, seed=5, chunk_frames=6, **GREEDY, **fxkw)
    n0 = hip.align_calls
    want = _cat(list(tts.stream(TEXT, **kw)))
    assert hip.align_calls == n0, "stream() launched the timing kernels"
    with pytest.raises(TypeError, match="token_spans="):
        tts.stream_timed(TEXT, **kw)  # this tokenizer has no character offsets
    items = list(tts.stream_timed(TEXT, token_spans=spans, **kw))
    assert hip.align_calls > n0
    assert all(isinstance(it, A.TimedChunk) for it in items)
    assert [it.final for it in items] == [False] * (len(items) - 1) + [True] and all(it.alignment is None for it in items[:-1])
    got = _cat([it.wav for it in items])
    assert got.shape == want.shape and torch.equal(got, want)
    al = items[-1].alignment
    T, S = len(al.path), len(spans)
    assert T >= 44
    # the path: the restatement on the engine's own score rows, with the stream's schedule and the default lag
    sc = tts.model.align_last[0].cpu().numpy()
    assert sc.shape == (T, S)
    row = O.run(sc, 6, 8, stream=True)
    assert al.path == row.path and np.float32(al.total).tobytes() == np.float32(row.base).tobytes()
    assert al.status == (0 if row.path[-1] == S - 1 else 2) and al.token_frames == O.token_frames(row.path, S)
    print(f"T = {T}, S = {S}: status {al.status}, last position {al.path[-1]}, confidence {al.confidence:.4f}")
    # the cues: whole words of the text, ordered, inside the audio, and together what the whole path gives
    words = [c for it in items for c in it.words]
    fx = effects.Effects.of(fxkw.get("speed", 1.0), fxkw.get("pitch", 0.0), None, fxkw.get("watermark"))
    assert words == effects.map_cues(A.word_cues(TEXT, spans, al.token_frames), fx)
    assert [c.text for c in words] == TEXT.split() and all(TEXT[c.char_start:c.char_end] == c.text for c in words)
    starts = [c.start_sample for c in words]
    assert starts == sorted(starts) and all(0 <= c.start_sample <= c.end_sample <= int(got.shape[-1]) for c in words)
    # a cue is reported only once its frames are committed: no later than the item that carries it
    heard = 0
    if not fxkw:
        for it in items:
            heard += int(it.wav.shape[-1])
            assert all(c.end_sample <= heard for c in it.words) or it.final


def test_bf16_mode_structure(cfg, sopro_np_noeos, mimi_np):
    """No numeric bar in bf16 mode (the tokens come from bf16 operands; the replay runs on fp32 operands): the audio is ``stream``'s,
    the path is monotone from position 0 with one entry per frame, the frame ranges tile it, and the cues are the text's words."""
    from conftest import FakeTok
    from sopro_amd import SoproTTS

    tts = SoproTTS.from_weights(cfg, sopro_np_noeos, mimi_np, FakeTok(), device=DEV, precision="bf16")
    spans = _char_tok(tts, TEXT)
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(ref=ref, max_frames=40, seed=5, chunk_frames=6, **GREEDY)
    want = _cat(list(tts.stream(TEXT, **kw)))
    items = list(tts.stream_timed(TEXT, token_spans=spans, lag_frames=4, **kw))
    assert torch.equal(_cat([it.wav for it in items]), want) and items[-1].final
    a = items[-1].alignment
    T, S = len(a.path), len(spans)
    assert T * 1920 == int(want.shape[-1]) and len(a.token_frames) == S and np.isfinite(a.total)
    assert a.path[0] == 0 and all(0 <= y - x <= 1 for x, y in zip(a.path, a.path[1:]))
    assert a.status == (0 if a.path[-1] == S - 1 else 2)
    assert all(a.path[f0:f1] == [s] * (f1 - f0) for s, (f0, f1) in enumerate(a.token_frames))
    assert all((f0, f1) == (T, T) for f0, f1 in a.token_frames[a.path[-1] + 1:]) and all(f1 > f0 for f0, f1 in a.token_frames[: a.path[-1] + 1])
    words = [c for it in items for c in it.words]
    assert [c.text for c in words] == TEXT.split() and words == A.word_cues(TEXT, spans, a.token_frames)
