"""Silence control on the device: ``hip.silence_squeeze`` / ``hip.SilenceState`` (csrc/sil.hip) against the numpy restatement
(tests/sil_ref.py, itself checked on the CPU by tests/test_sil_host.py), and ``silence=`` through every public entry point.
Everything is compared exactly: the definition leaves no rounding freedom.

The synthetic checkpoint's audio has no real silence (hop maxima between 3 and 4.5, a peak near 6), so the engine tests take the
plain output first and put the floor at the 70th percentile of its hop maxima; with a cap of 4 hops and an onset of 2 the
restatement must then find a leading and an interior cut in every row (asserted), and the engine must reproduce it."""
import numpy as np
import pytest
import torch

import sil_ref as R
from sopro_amd import Silence, Watermark, hip
from sopro_amd import align as A
from sopro_amd.longform import group_plan, split_text

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GREEDY = dict(top_p=0.0, temperature=1.0, anti_loop=False)
PAD = 777.0      # past a row's length in the input: must never reach the output
CANARY = -555.0  # past a row's length in the output: must survive
HOP = R.HOP


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sil(thr, cap_h, b):
    return None if cap_h == 0 else Silence(max_pause_ms=10.0 * cap_h, onset_ms=10.0 * b, floor=float(thr))


def _ref(x, s):
    """the restatement of what ``s`` does to the samples x (numpy) -> (y, cuts)"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    return (x.copy(), []) if s is None else R.squeeze(x, np.float32(s.thr), s.cap_hops, s.onset_hops)


def _rows_on_device(rows, stride):
    base = np.full((len(rows), stride), PAD, dtype=np.float32)
    for k, r in enumerate(rows):
        base[k, : len(r)] = r
    dev = torch.from_numpy(base).to(DEV)[:, : stride - 1]
    assert dev.stride(0) == stride
    return dev


@pytest.fixture(scope="module")
def designed():
    """The designed batch and its restated results, made once: [(x, sil, y, cuts)]."""
    rows = R.designed_batch(hip.SIL_PLAN_WORDS * 64)
    out = []
    for x, thr, cap_h, b in rows:
        s = _sil(thr, cap_h, b)
        assert s is None or (np.float32(s.thr) == thr and s.cap_hops == cap_h and s.onset_hops == b)
        y, cuts = _ref(x, s)
        out.append((x, s, y, cuts))
    return out


def test_one_shot_on_the_designed_batch(designed):
    xs = [d[0] for d in designed]
    sils = [d[1] for d in designed]
    lens = [len(x) for x in xs]
    # what the batch is designed to hold
    assert len(xs) == 8 and lens[4] > hip.SIL_PLAN_WORDS * 64 * HOP      # the plan workgroup passes over row 4's bitmap twice
    assert sils[5] is None and len(designed[6][2]) == 0 and lens[6] > 0 and lens[7] == 0
    assert len({(s.thr, s.cap_hops, s.onset_hops) for s in sils if s}) >= 4
    kinds = set()
    for x, _s, _y, cuts in designed:
        kinds |= {"lead" if p == 0 else ("trail" if p + n == len(x) else "mid") for p, n in cuts}
    assert kinds == {"lead", "mid", "trail"}
    stride = max(lens) + 1 + (-max(lens)) % 4  # 1 mod 4: rows 0 and 4 are 16-byte aligned, the others are not
    assert stride % 4 == 1
    wav = _rows_on_device(xs, stride)
    out_buf = torch.full((len(xs), stride), CANARY, device=DEV)[:, : stride - 1]
    before = hip.sil_calls
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out, got_lens, got_cuts = hip.silence_squeeze(wav, lens, sils, out=out_buf)
    s.synchronize()
    assert hip.sil_calls == before + 1                                    # one launch sequence for the whole batch
    host = out_buf.cpu()
    for k, (x, _s, y, cuts) in enumerate(designed):
        print(f"row {k}: {len(x)} -> {got_lens[k]} samples (want {len(y)}), {len(got_cuts[k])} cuts (want {len(cuts)})")
        assert got_lens[k] == len(y) and got_cuts[k] == cuts, k
        diff = int((_bits(host[k, : len(y)]) != _bits(torch.from_numpy(y))).sum())
        assert diff == 0, f"row {k}: {diff} samples differ"
        assert bool((host[k, len(y):] == CANARY).all()), f"row {k}: something past the row's length was written"
    assert tuple(out.shape) == (len(xs), max(got_lens))
    assert torch.equal(_bits(host[5, : lens[5]]), _bits(torch.from_numpy(xs[5])))  # the identity row, bit for bit
    assert not bool((host == PAD).any()), "a sample past a row's length reached the output"
    # nothing to do: nothing is launched
    before = hip.sil_calls
    same, l2, c2 = hip.silence_squeeze(wav, lens, None)
    assert hip.sil_calls == before and same.data_ptr() == wav.data_ptr() and l2 == lens and c2 == [[] for _ in lens]
    # a buffer too small for a row is refused by the host wrapper before any launch
    with pytest.raises(hip.SoproHipError):
        hip.silence_squeeze(wav, lens, sils, out=torch.empty(len(xs), 100, device=DEV))


def _feed_all(st, wav, lens, sizes):
    """rows fed in chunks of ``sizes`` (cycled; a row that has ended gets nothing), then a flush -> per row (samples, cuts)"""
    rows = len(lens)
    got = [[] for _ in range(rows)]
    at, k = 0, 0
    while at < max(lens):
        n = int(sizes[k % len(sizes)])
        cl = [min(max(L - at, 0), n) for L in lens]
        out, ol = st.feed(wav[:, at: at + n], cl)
        for r in range(rows):
            got[r].append(out[r, : ol[r]])
        at += n
        k += 1
    out, ol = st.flush()
    for r in range(rows):
        got[r].append(out[r, : ol[r]])
    return [torch.cat(g).cpu() for g in got], [list(c) for c in st.cuts]


def _check_chunked(designed, idx, got, cuts, what):
    for j, k in enumerate(idx):
        y, want_cuts = designed[k][2], designed[k][3]
        assert got[j].numel() == len(y) and cuts[j] == want_cuts, (what, k, got[j].numel(), len(y))
        assert torch.equal(_bits(got[j]), _bits(torch.from_numpy(y))), (what, k)


def test_chunked_form_equals_one_shot(designed):
    # 1-sample chunks on a short row
    x = R.bursts([("g", 3), ("s", 1), ("g", 5), ("s", 1), ("g", 3)], tail=30, seed=11)
    s1 = Silence(max_pause_ms=30.0, onset_ms=10.0, floor=0.05)
    y, want_cuts = _ref(x, s1)
    assert {p == 0 for p, _n in want_cuts} == {True, False} and want_cuts[-1][0] + want_cuts[-1][1] == len(x)
    st = hip.SilenceState(1, s1, DEV)
    got, cuts = _feed_all(st, torch.from_numpy(x).to(DEV).reshape(1, -1), [len(x)], [1])
    assert cuts[0] == want_cuts and torch.equal(_bits(got[0]), _bits(torch.from_numpy(y)))
    # 1920 x k chunks on the short designed rows, twice through one state: after its flush a state is fresh
    idx = [0, 1, 2, 3, 5, 6, 7]
    xs, sils = [designed[k][0] for k in idx], [designed[k][1] for k in idx]
    lens = [len(v) for v in xs]
    wav = _rows_on_device(xs, max(lens) + 2)
    st = hip.SilenceState(len(idx), sils, DEV)
    for turn in range(2):
        got, cuts = _feed_all(st, wav, lens, [1920 * 2])
        _check_chunked(designed, idx, got, cuts, f"1920 x 2, turn {turn}")
    # random sizes up to 5000, the long row included
    idx = list(range(8))
    xs, sils = [designed[k][0] for k in idx], [designed[k][1] for k in idx]
    lens = [len(v) for v in xs]
    wav = _rows_on_device(xs, max(lens) + 3)
    sizes = np.random.default_rng(3).integers(1, 5001, size=64).tolist()
    before = hip.sil_calls
    got, cuts = _feed_all(hip.SilenceState(len(idx), sils, DEV), wav, lens, sizes)
    assert hip.sil_calls > before
    _check_chunked(designed, idx, got, cuts, "random sizes")


# ------------------------------------------------------------------------------------------ end to end
TEXT = ("Hello there. This is a rather long sentence, with several clauses, that will not fit in forty characters.\n\n"
        "A new paragraph begins here! Is it fine? Yes.")
MAX_CHARS = 40
W1 = Watermark(0x0123456789ABCDEF, 173)
W2 = Watermark(0xFEEDFACECAFEBEEF, 7, -18.0)


def _register(tts, text, max_chars=MAX_CHARS):
    segs = split_text(text, max_chars=max_chars)
    for s in segs:
        tts.tokenizer.table[s.text] = [1 + (ord(c) % 500) for c in s.text]
    return segs


def _ref_tq(seed=5):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 2048, size=(24, 32)))


def _np(wav):
    return wav.detach().reshape(-1).cpu().numpy()


def _floor_sil(*wavs):
    """cap 4 hops, onset 2, the floor at the 70th percentile of the hop maxima of the given plain output"""
    x = np.concatenate([_np(w) for w in wavs])
    m = np.abs(np.pad(x, (0, -len(x) % HOP))).reshape(-1, HOP).max(1)
    return Silence(max_pause_ms=40.0, onset_ms=20.0, floor=float(np.float32(np.percentile(m, 70))))


def _squeezed(wav, s, what):
    """the restatement on a plain output, after asserting that it finds a leading and an interior cut there"""
    x = _np(wav)
    y, cuts = _ref(x, s)
    lead = any(p == 0 for p, _n in cuts)
    mid = any(p > 0 and p + n < len(x) for p, n in cuts)
    print(f"{what}: {len(x)} -> {len(y)} samples, {len(cuts)} cuts, leading {lead}, interior {mid}")
    assert lead and mid, f"{what}: the floor leaves no leading / interior cut to test ({cuts})"
    return y, cuts


def _same(got, y):
    return got.numel() == len(y) and torch.equal(_bits(got.reshape(-1).cpu()), _bits(torch.from_numpy(y)))


def test_synthesize_and_synthesize_batch_with_silence(tts_noeos):
    tts = tts_noeos
    texts = ["first text", "a second, longer text", "third"]
    for t in texts:
        tts.tokenizer.table[t] = [1 + (ord(c) % 500) for c in t]
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(ref=ref, max_frames=40, seed=7)
    c0 = hip.sil_calls
    plain = tts.synthesize(texts[0], **kw)
    assert torch.equal(tts.synthesize(texts[0], silence=None, **kw), plain) and hip.sil_calls == c0
    S = _floor_sil(plain)
    y, _cuts = _squeezed(plain, S, "synthesize")
    got = tts.synthesize(texts[0], silence=S, **kw)
    assert hip.sil_calls == c0 + 1 and got.dim() == 3 and _same(got, y)
    with pytest.raises(TypeError):
        tts.synthesize(texts[0], silence=0.5, **kw)
    # a batch: one setting per row, None entries allowed, the padded batch squeezed in one launch sequence
    bkw = dict(max_frames=36, seed=4)
    base = tts.synthesize_batch(texts, [ref] * 3, **bkw)
    c0 = hip.sil_calls
    same = tts.synthesize_batch(texts, [ref] * 3, silence=[None, None, None], **bkw)
    assert hip.sil_calls == c0 and all(torch.equal(a, b) for a, b in zip(base, same))
    sils = [_floor_sil(base[0]), None, _floor_sil(base[2])]
    assert sils[0].thr != sils[2].thr
    want = [_squeezed(base[b], sils[b], f"batch row {b}") if sils[b] else (_np(base[b]), []) for b in range(3)]
    got = tts.synthesize_batch(texts, [ref] * 3, silence=sils, **bkw)
    assert hip.sil_calls == c0 + 1
    assert torch.equal(_bits(got[1]), _bits(base[1]))                     # the row at None comes back bit for bit
    assert all(_same(got[b], want[b][0]) for b in range(3))
    plain_pb = tts.synthesize_batch(texts, [ref] * 3, padded=True, **bkw)
    pb = tts.synthesize_batch(texts, [ref] * 3, silence=sils, padded=True, **bkw)
    assert plain_pb.cuts is None and pb.cuts == [w[1] for w in want] and pb.lens == [len(w[0]) for w in want]
    assert pb.frames == plain_pb.frames and torch.equal(pb.tokens, plain_pb.tokens)  # what the model produced
    assert all(torch.equal(pb.wav[b, : pb.lens[b]], got[b].reshape(-1)) for b in range(3))
    with pytest.raises(ValueError):
        tts.synthesize_batch(texts, [ref] * 3, silence=[sils[0], None], **bkw)
    # with rate, pitch and a mark: wm_embed(squeeze(apply_prosody(plain)))
    pkw = dict(speed=[1.25, 1.0, 0.8], pitch=[2.0, 0.0, -3.0], **bkw)
    shaped = tts.synthesize_batch(texts, [ref] * 3, **pkw)
    sils = [_floor_sil(shaped[0]), _floor_sil(shaped[1]), None]
    marks = [W1, None, W2]
    got = tts.synthesize_batch(texts, [ref] * 3, silence=sils, watermark=marks, **pkw)
    for b in range(3):
        y = _squeezed(shaped[b], sils[b], f"shaped row {b}")[0] if sils[b] else _np(shaped[b])
        want_b = hip.wm_embed(torch.from_numpy(y).to(DEV).reshape(1, -1), [len(y)], marks[b]).reshape(-1)
        assert got[b].numel() == len(y) and torch.equal(_bits(got[b].reshape(-1)), _bits(want_b)), b


@pytest.mark.parametrize("cf", [6, 16])
def test_squeezed_stream_is_the_squeeze_of_the_plain_stream(tts_noeos, cf):
    tts = tts_noeos
    text = "a streamed utterance of some length"
    tts.tokenizer.table[text] = [1 + (ord(c) % 500) for c in text]
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq(6))
    kw = dict(ref=ref, max_frames=40, chunk_frames=cf, seed=12)
    c0 = hip.sil_calls
    plain = list(tts.stream(text, **kw))
    same = list(tts.stream(text, silence=None, **kw))
    assert hip.sil_calls == c0 and len(same) == len(plain) and all(torch.equal(a, b) for a, b in zip(plain, same))
    whole = torch.cat(plain, -1)
    S = _floor_sil(whole)
    y, _cuts = _squeezed(whole, S, f"stream cf={cf}")
    chunks = list(tts.stream(text, silence=S, **kw))
    assert chunks and all(c.dim() == 2 and c.shape[0] == 1 and c.is_cuda for c in chunks) and hip.sil_calls > c0
    assert _same(torch.cat(chunks, -1), y)
    with pytest.raises(TypeError):
        tts.stream(text, silence="quiet", **kw)


def test_synthesize_timed_with_silence(tts_noeos):
    tts = tts_noeos
    text = "  so, word timing works !"
    tts.tokenizer.table[text] = [1 + (ord(c) % 500) for c in text]
    spans = [(i, i + 1) for i in range(len(text))]
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(ref=ref, max_frames=40, seed=11)
    res = tts.synthesize_timed(text, token_spans=spans, **kw)
    S = _floor_sil(res.wav)
    y, cuts = _squeezed(res.wav, S, "timed")
    got = tts.synthesize_timed(text, token_spans=spans, silence=S, **kw)
    assert _same(got.wav, y) and torch.equal(got.wav, tts.synthesize(text, silence=S, **kw))
    assert got.words == R.squeeze_cues(res.words, cuts) == A.squeeze_cues(res.words, cuts) and got.alignment.path == res.alignment.path
    assert all(0 <= c.start_sample <= c.end_sample <= len(y) for c in got.words)


def test_long_form_with_silence(tts_noeos):
    tts = tts_noeos
    segs = _register(tts, TEXT)
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(max_frames=20, max_chars=MAX_CHARS, seed=3, ref=ref)
    c0 = hip.sil_calls
    base = tts.synthesize_long(TEXT, plan="latency", keep_parts=True, **kw)
    assert hip.sil_calls == c0
    S = _floor_sil(*[p.wav for p in base.parts])
    res = tts.synthesize_long(TEXT, plan="latency", keep_parts=True, silence=S, **kw)
    assert hip.sil_calls == c0 + len(group_plan(len(segs), "latency"))    # one launch sequence per group, before its join
    for k, (a, b) in enumerate(zip(res.parts, base.parts)):                # the rows the join saw are the squeezed rows
        assert _same(a.wav, _ref(_np(b.wav), S)[0]) and torch.equal(a.tokens, b.tokens), k
    n = int(res.wav.shape[-1])
    assert len(res.segments) == len(segs) and n < int(base.wav.shape[-1])
    assert all(0 <= s <= e <= n for _t, s, e in res.segments)
    assert all(res.segments[k][2] <= res.segments[k + 1][1] for k in range(len(segs) - 1))  # monotone
    pieces = list(tts.stream_long(TEXT, silence=S, **kw))
    assert torch.equal(_bits(torch.cat(pieces, -1)), _bits(res.wav.reshape(1, -1)))
    timed = tts.synthesize_long(TEXT, plan="latency", silence=S, word_cues=True, token_spans=lambda t: [(i, i + 1) for i in range(len(t))], **kw)
    assert torch.equal(timed.wav, res.wav) and timed.words
    assert all(0 <= c.start_sample <= c.end_sample <= n for c in timed.words)
    with pytest.raises(TypeError):
        tts.stream_long(TEXT, silence=3, **kw)


def test_service_squeezes_each_request_with_its_own_setting_and_refuses_where_there_is_none(tts_noeos):
    from sopro_amd.serving import SynthesisService

    tts = tts_noeos
    rng = np.random.default_rng(41)
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq(9))
    ids_a = torch.from_numpy(rng.integers(1, 500, size=17))
    kw = dict(max_frames=30, **GREEDY)
    tts.tokenizer.table["x"] = [3, 4, 5, 6]
    direct = tts.synthesize_batch([""], [ref], text_ids=[ids_a], **kw)[0]
    S = _floor_sil(direct)
    S2 = Silence(max_pause_ms=40.0, onset_ms=20.0, floor=S.floor * 1.02)
    with pytest.raises(NotImplementedError):
        tts.stream_batch(["x"], [ref], silence=S, max_frames=8)
    svc = SynthesisService(tts, max_batch=3, max_wait_ms=500.0, lanes=2, ar_cus=64, ar_parts=1, ar_shared=False)
    try:
        futs = [svc.submit("", ref, text_ids=ids_a, **kw), svc.submit("", ref, text_ids=ids_a, silence=S, **kw),
                svc.submit("", ref, text_ids=ids_a, silence=S2, **kw)]
        got = [f.result(timeout=180) for f in futs]
        assert svc.stats["batches"] == 1 and svc.stats["rows"] == 3
        with pytest.raises(TypeError):
            svc.submit("", ref, text_ids=ids_a, silence=0.1, **kw)
        with pytest.raises(NotImplementedError):
            svc.submit_stream("", ref, text_ids=ids_a, silence=S, **kw)
    finally:
        svc.close()
    torch.cuda.synchronize()
    assert _same(got[1], _squeezed(got[0], S, "service")[0]) and _same(got[2], _ref(_np(got[0]), S2)[0])
    n = int(got[0].shape[-1])
    direct_call = hip.silence_squeeze(got[0].reshape(1, -1).expand(2, n).contiguous(), [n, n], [S, S2])[0]  # the operator, called directly
    assert torch.equal(_bits(got[1].reshape(-1)), _bits(direct_call[0, : got[1].numel()]))
    assert torch.equal(_bits(got[2].reshape(-1)), _bits(direct_call[1, : got[2].numel()]))
    svc = SynthesisService(tts, mode="continuous", max_batch=3, ar_parts=1, ar_cus=64, max_frames=40, max_text=64, poll_every=8, bulk_batch=2)
    try:
        with pytest.raises(NotImplementedError):
            svc.submit("", ref, text_ids=torch.tensor([3, 4, 5, 6]), silence=S, max_frames=8, **GREEDY)
    finally:
        svc.close()
