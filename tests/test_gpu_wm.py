"""Watermark on the device: ``hip.wm_embed`` / ``hip.WatermarkState`` / ``hip.wm_detect_rows`` (csrc/wm.hip) against the numpy
restatement (tests/wm_ref.py, itself checked on the CPU by tests/test_wm_host.py), and ``watermark=`` through every public entry
point.  The embedder is compared exactly (its definition leaves no rounding freedom); the detector's sums have no prescribed order,
so f, R and z are compared within the fp32 summation bounds the definition's section on tolerances gives."""
import numpy as np
import pytest
import torch

import tsm_ref as T
import wm_ref as W
from sopro_amd import Watermark, hip
from sopro_amd import watermark as wm
from sopro_amd.longform import group_plan, split_text

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GREEDY = dict(top_p=0.0, temperature=1.0, anti_loop=False)
PAD = 777.0      # past a row's length in the input: must never reach the output
CANARY = -555.0  # past a row's length in the output: must survive
KEY, TAG = 0x0123456789ABCDEF, 173
W1, W2, W3 = Watermark(KEY, TAG), Watermark(KEY ^ (1 << 40), 7, -18.0), Watermark(0xFEEDFACECAFEBEEF, 255)
U = 2.0 ** -24


def _ref(x, m):
    return W.embed(x, None) if m is None else W.embed(x, m.key, m.tag, m.strength_db)


def _source(n, seed=0):
    """n samples with tone, noise, silence and a negative zero in them"""
    x = np.concatenate([T.glide(100.0, 180.0, 9000), np.zeros(1500, np.float32), T.noise_with_silence(0.5, seed=seed + 4, head=0, tail=2000)])
    x = np.tile(x, -(-max(n, 1) // len(x)))[:n].copy()
    if n > 3:
        x[3] = -0.0
    return x


def _rows_on_device(rows, stride):
    base = np.full((len(rows), stride), PAD, dtype=np.float32)
    for k, r in enumerate(rows):
        base[k, : len(r)] = r
    dev = torch.from_numpy(base).to(DEV)[:, : stride - 1]
    assert dev.stride(0) == stride
    return dev


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_embed_on_a_ragged_batch():
    lens = [0, 1, 479, 480, 481, 1919, 8191, 8192, 8193, 20000, hip.WM_TILE - 1, hip.WM_TILE, hip.WM_TILE + 1, 2 * hip.WM_TILE + 960]
    marks = [W1, W2, None, W1, W3, W2, W1, None, W3, W1, W2, W3, W1, W2]
    rows = [_source(n, seed=k) for k, n in enumerate(lens)]
    stride = max(lens) + 3
    assert stride % 4 != 0 and len({(m.key, m.tag) for m in marks if m}) == 3 and len({m.strength_db for m in marks if m}) == 2
    wav = _rows_on_device(rows, stride)
    cap = max(lens) + 19
    out_buf = torch.full((len(rows), cap + 2), CANARY, device=DEV)[:, :cap]
    before = hip.wm_calls()
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = hip.wm_embed(wav, lens, marks, out=out_buf)
    s.synchronize()
    assert hip.wm_calls() == before + 1                       # one launch for the whole batch
    assert tuple(out.shape) == (len(rows), max(lens))
    host = out_buf.cpu()
    for k, (x, m) in enumerate(zip(rows, marks)):
        want = torch.from_numpy(_ref(x, m))
        diff = int((_bits(host[k, : len(x)]) != _bits(want)).sum())
        assert diff == 0, f"row {k} (len {len(x)}): {diff} samples differ"
        assert bool((host[k, len(x):] == CANARY).all()), f"row {k}: something past the row's length was written"
        if m is None:
            assert torch.equal(_bits(host[k, : len(x)]), _bits(torch.from_numpy(x)))
        elif len(x) > 481:
            assert not torch.equal(host[k, : len(x)], torch.from_numpy(x))
    assert not bool((host == PAD).any()), "a sample past a row's length reached the output"
    # no mark at all: nothing is launched
    same = hip.wm_embed(wav, lens, None)
    assert hip.wm_calls() == before + 1 and same.data_ptr() == wav.data_ptr()


@pytest.mark.parametrize("sizes", [[1920], [1920, 700, 5000, 1, 479, 11520, 2400]], ids=["c1", "ragged"])
def test_chunked_state_equals_one_shot_on_the_device(sizes):
    n_total = 30000
    rows = [_source(n_total, seed=k) for k in range(4)]
    marks = [W1, W2, None, W3]
    wav = torch.from_numpy(np.stack(rows)).to(DEV)
    one = hip.wm_embed(wav, [n_total] * 4, marks)
    st = hip.WatermarkState(4, marks, DEV)
    got = [[] for _ in rows]
    longest = 0
    i = j = 0
    while i < n_total:
        n = min(sizes[j % len(sizes)], n_total - i)
        j += 1
        l1 = max(0, n - 7)
        ragged = len(sizes) > 1
        lens = [n, l1, n, 0 if j % 2 else n] if ragged else None         # row 1 lags by up to 7 samples, row 3 sits out every other call ...
        out, out_lens = st.feed(wav[:, i: i + n], lens)
        for b in range(4):
            got[b].append(out[b, : out_lens[b]].cpu())
            assert out_lens[b] % 480 == 0
        if ragged:                                                         # ... and they catch up in a call of their own (rows 0, 2: empty chunks)
            fill = torch.zeros(4, n, device=DEV)
            fill[1, : n - l1] = wav[1, i + l1: i + n]
            fill[3] = wav[3, i: i + n]
            out, out_lens = st.feed(fill, [0, n - l1, 0, n if j % 2 else 0])
            for b in range(4):
                got[b].append(out[b, : out_lens[b]].cpu())
        i += n
        longest = max(longest, i - sum(int(t.numel()) for t in got[0]))
    assert longest <= 1440
    out, out_lens = st.flush()
    for b in range(4):
        got[b].append(out[b, : out_lens[b]].cpu())
        y = torch.cat(got[b])
        want = torch.from_numpy(_ref(rows[b], marks[b]))
        assert y.numel() == n_total and torch.equal(_bits(y), _bits(one[b].cpu())) and torch.equal(_bits(y), _bits(want)), b
    # the flush left a fresh state: the same rows again, in one piece
    out, out_lens = st.feed(wav, flush=True)
    assert out_lens == [n_total] * 4 and torch.equal(_bits(out), _bits(one))


def test_detector_rows_against_the_restatement():
    glide_noise = np.concatenate([T.glide(100, 180, 30000), np.zeros(3000, np.float32), T.noise_with_silence(0.5, seed=4, head=0, tail=2000)])
    rows = [W.embed(T.harmonic(220, 1.0), KEY, TAG),
            W.degrade(W.embed(glide_noise, KEY, TAG)),
            T.harmonic(120, 1.5),
            np.zeros(0, np.float32),
            W.embed(T.harmonic(150, 1.0), KEY, TAG)[:5000],
            np.zeros(9000, np.float32)]
    lens = [len(r) for r in rows]
    wav = _rows_on_device(rows, max(lens) + 3)
    before = hip.wm_calls()
    res, f, R = hip.wm_detect_rows(wav, lens, [KEY] * len(rows), details=True)
    torch.cuda.synchronize()
    assert hip.wm_calls() == before + 1
    f, R = f.cpu().numpy(), R.cpu().numpy()
    rng = np.random.default_rng(2)
    for k, y in enumerate(rows):
        want, d = W.detect(y, KEY, details=True)
        got = res[k]
        print(f"row {k} (len {len(y)}): device {got}\n{'':>17}restated {want}")
        assert got.present == want.present
        # f: a sum of at most 94 fp32 terms in ascending order, each term a correctly rounded quotient (2 ulp allowed)
        bound_f = (94 * U + 2 * 2.0 ** -23) * d["fa"] + 1e-45
        assert np.all(np.abs(f[k].astype(np.float64) - d["f"]) <= bound_f), f"row {k}: f off by {np.abs(f[k] - d['f']).max():.3e}"
        # R at a sampled set of offsets, against the float64 sum over the device's own f: the fp32 summation bound, any order
        offs = sorted({0, 1, W.P - 1, want.offset, (want.offset + W.SHIFT * TAG) % W.P, *rng.integers(0, W.P, 24).tolist()})
        for lane in (0, 1):
            Rw, Ra = W.correlate_at(f[k], d["d"][lane], offs)
            err = np.abs(R[k, lane, offs].astype(np.float64) - Rw)
            assert np.all(err <= W.P * U * Ra + 1e-45), f"row {k} lane {lane}: R off by {err.max():.3e}"
        if len(y) == 0 or not np.any(y):
            assert got == wm.WatermarkResult(False, 0.0, 0, 0, 0.0, 0.0) and not f[k].any() and not R[k].any()
            continue
        for zg, zw in ((got.z_sync, want.z_sync), (got.z_tag, want.z_tag)):
            assert abs(zg - zw) <= 1e-3 * abs(zw), (k, zg, zw)
        if k in (0, 1, 4):                                        # the marked rows
            assert (got.offset, got.tag) == (want.offset, want.tag) and want.tag == TAG
    assert res[0].present and res[1].present and res[1].offset == 5191 and not res[2].present and not res[3].present
    # the public detector: one clip, a list of clips, padded rows; another key finds nothing
    one = wm.detect(torch.from_numpy(rows[0]).reshape(1, 1, -1), KEY, device=DEV)
    assert one == res[0]
    many = wm.detect([rows[0], torch.from_numpy(rows[2]).to(DEV)], KEY)
    assert many[0] == res[0] and many[1] == res[2]
    assert wm.detect(wav, KEY, lens=lens) == res
    assert not wm.detect(rows[0], KEY ^ 1, device=DEV).present


def test_bad_arguments_are_refused():
    wav = torch.zeros(2, 1000, device=DEV)
    before = hip.wm_calls()
    with pytest.raises(TypeError):
        hip.wm_embed(wav, [1000, 1000], KEY)
    with pytest.raises(ValueError):
        hip.wm_embed(wav, [1000, 1000], [W1])
    with pytest.raises(hip.SoproHipError):
        hip.wm_embed(wav, [1000, 1001], W1)
    with pytest.raises(hip.SoproHipError):
        hip.wm_embed(wav, [1000, 1000], W1, out=torch.zeros(2, 999, device=DEV))
    with pytest.raises(hip.SoproHipError):
        hip.wm_embed(wav.cpu(), [1000, 1000], W1)
    with pytest.raises(hip.SoproHipError):
        hip.WatermarkState(1, W1, "cpu")
    with pytest.raises(ValueError):
        hip.wm_detect_rows(wav, [1000, 1000], [KEY])
    with pytest.raises(ValueError):
        wm.detect(wav, KEY)  # padded rows need their lengths
    assert hip.wm_calls() == before


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


def _marked(wav, m):
    return hip.wm_embed(wav.reshape(1, -1), [int(wav.shape[-1])], m).reshape(wav.shape)


def test_synthesize_and_synthesize_batch_with_a_mark(tts_noeos):
    tts = tts_noeos
    texts = ["first text", "a second, longer text", "third"]
    for t in texts:
        tts.tokenizer.table[t] = [1 + (ord(c) % 500) for c in t]
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(ref=ref, max_frames=16, seed=7)
    c0 = hip.wm_calls()
    plain = tts.synthesize(texts[0], **kw)
    assert torch.equal(tts.synthesize(texts[0], watermark=None, **kw), plain) and hip.wm_calls() == c0
    got = tts.synthesize(texts[0], watermark=W1, **kw)
    assert hip.wm_calls() == c0 + 1
    want = _marked(plain, W1)
    assert got.shape == plain.shape and torch.equal(_bits(got), _bits(want)) and not torch.equal(got, plain)
    assert torch.equal(got.reshape(-1).cpu(), torch.from_numpy(_ref(plain.reshape(-1).cpu().numpy(), W1)))
    shaped = tts.synthesize(texts[0], speed=1.25, pitch=2, **kw)
    assert torch.equal(_bits(tts.synthesize(texts[0], speed=1.25, pitch=2, watermark=W2, **kw)), _bits(_marked(shaped, W2)))
    with pytest.raises(TypeError):
        tts.synthesize(texts[0], watermark=KEY, **kw)
    assert isinstance(tts.detect_watermark(got, KEY), wm.WatermarkResult)  # (the test checkpoint's output is not speech: no bar on the score)
    # a batch: one mark per row, None entries allowed, the padded batch marked in one launch
    bkw = dict(max_frames=14, seed=4)
    base = tts.synthesize_batch(texts, [ref] * 3, **bkw)
    c0 = hip.wm_calls()
    same = tts.synthesize_batch(texts, [ref] * 3, watermark=[None, None, None], **bkw)
    assert hip.wm_calls() == c0 and all(torch.equal(a, b) for a, b in zip(base, same))
    marks = [W1, None, W2]
    got = tts.synthesize_batch(texts, [ref] * 3, watermark=marks, **bkw)
    assert hip.wm_calls() == c0 + 1
    assert torch.equal(_bits(got[1]), _bits(base[1]))                     # the row without a mark comes back bit for bit
    for b in (0, 2):
        assert torch.equal(_bits(got[b]), _bits(_marked(base[b], marks[b]))) and not torch.equal(got[b], base[b]), b
    pb = tts.synthesize_batch(texts, [ref] * 3, watermark=marks, padded=True, **bkw)
    assert all(torch.equal(pb.wav[b, : pb.lens[b]], got[b].reshape(-1)) for b in range(3))
    one = tts.synthesize_batch(texts, [ref] * 3, watermark=W3, **bkw)
    assert all(torch.equal(_bits(one[b]), _bits(_marked(base[b], W3))) for b in range(3))
    with pytest.raises(ValueError):
        tts.synthesize_batch(texts, [ref] * 3, watermark=[W1, None], **bkw)


@pytest.mark.parametrize("cf", [6, 16])
def test_marked_stream_is_the_embed_of_the_plain_stream(tts_noeos, cf):
    tts = tts_noeos
    text = "a streamed utterance of some length"
    tts.tokenizer.table[text] = [1 + (ord(c) % 500) for c in text]
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq(6))
    kw = dict(ref=ref, max_frames=24, chunk_frames=cf, seed=12)
    c0 = hip.wm_calls()
    plain = list(tts.stream(text, **kw))
    same = list(tts.stream(text, watermark=None, **kw))
    assert hip.wm_calls() == c0 and len(same) == len(plain) and all(torch.equal(a, b) for a, b in zip(plain, same))
    whole = torch.cat(plain, -1)
    chunks = list(tts.stream(text, watermark=W1, **kw))
    assert chunks and all(c.dim() == 2 and c.shape[0] == 1 and c.is_cuda for c in chunks) and hip.wm_calls() > c0
    assert torch.equal(_bits(torch.cat(chunks, -1)), _bits(_marked(whole, W1)))
    shaped = torch.cat(list(tts.stream(text, speed=0.8, pitch=-3.0, **kw)), -1)
    got = torch.cat(list(tts.stream(text, speed=0.8, pitch=-3.0, watermark=W2, **kw)), -1)
    assert torch.equal(_bits(got), _bits(_marked(shaped, W2)))
    with pytest.raises(TypeError):
        tts.stream(text, watermark="mark", **kw)


def test_long_form_with_a_mark(tts):
    segs = _register(tts, TEXT)
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(max_frames=12, max_chars=MAX_CHARS, seed=3, ref=ref, **GREEDY)
    c0 = hip.wm_calls()
    base = tts.synthesize_long(TEXT, plan="latency", keep_parts=True, **kw)
    assert hip.wm_calls() == c0
    res = tts.synthesize_long(TEXT, plan="latency", keep_parts=True, watermark=W1, **kw)
    assert hip.wm_calls() == c0 + 1                                       # the joined waveform, in one launch
    assert torch.equal(_bits(res.wav), _bits(_marked(base.wav, W1))) and res.segments == base.segments and res.edges == base.edges
    assert all(torch.equal(a.wav, b.wav) for a, b in zip(res.parts, base.parts))  # the batches ran unmarked
    pieces = list(tts.stream_long(TEXT, watermark=W1, **kw))
    assert len(pieces) <= len(group_plan(len(segs), "latency")) + 1
    assert torch.equal(_bits(torch.cat(pieces, -1)), _bits(res.wav.reshape(1, -1)))
    plain_pieces = list(tts.stream_long(TEXT, **kw))
    assert torch.equal(torch.cat(plain_pieces, -1), base.wav.reshape(1, -1))
    with pytest.raises(TypeError):
        tts.stream_long(TEXT, watermark=3, **kw)


def test_synthesize_timed_with_a_mark(tts_noeos):
    tts = tts_noeos
    text = "  so, word timing works !"
    tts.tokenizer.table[text] = [1 + (ord(c) % 500) for c in text]
    spans = [(i, i + 1) for i in range(len(text))]
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(ref=ref, max_frames=14, seed=11)
    res = tts.synthesize_timed(text, token_spans=spans, **kw)
    got = tts.synthesize_timed(text, token_spans=spans, watermark=W1, **kw)
    assert got.words == res.words and got.alignment.path == res.alignment.path
    assert torch.equal(_bits(got.wav), _bits(_marked(res.wav, W1))) and torch.equal(got.wav, tts.synthesize(text, watermark=W1, **kw))


def test_service_marks_each_request_with_its_own_mark_and_refuses_where_there_is_none(tts):
    from sopro_amd.serving import SynthesisService

    rng = np.random.default_rng(41)
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq(9))
    ids_a = torch.from_numpy(rng.integers(1, 500, size=17))
    kw = dict(max_frames=12, **GREEDY)
    tts.tokenizer.table["x"] = [3, 4, 5, 6]
    with pytest.raises(NotImplementedError):
        tts.stream_batch(["x"], [ref], watermark=W1, max_frames=8)
    svc = SynthesisService(tts, max_batch=3, max_wait_ms=500.0, lanes=2, ar_cus=64, ar_parts=1, ar_shared=False)
    try:
        futs = [svc.submit("", ref, text_ids=ids_a, **kw), svc.submit("", ref, text_ids=ids_a, watermark=W1, **kw),
                svc.submit("", ref, text_ids=ids_a, watermark=W2, **kw)]
        got = [f.result(timeout=180) for f in futs]
        assert svc.stats["batches"] == 1 and svc.stats["rows"] == 3
        with pytest.raises(TypeError):
            svc.submit("", ref, text_ids=ids_a, watermark=KEY, **kw)
        with pytest.raises(NotImplementedError):
            svc.submit_stream("", ref, text_ids=ids_a, watermark=W1, **kw)
    finally:
        svc.close()
    torch.cuda.synchronize()
    assert torch.equal(_bits(got[1]), _bits(_marked(got[0], W1))) and torch.equal(_bits(got[2]), _bits(_marked(got[0], W2)))
    svc = SynthesisService(tts, mode="continuous", max_batch=3, ar_parts=1, ar_cus=64, max_frames=40, max_text=64, poll_every=8, bulk_batch=2)
    try:
        with pytest.raises(NotImplementedError):
            svc.submit("", ref, text_ids=torch.tensor([3, 4, 5, 6]), watermark=W1, max_frames=8, **GREEDY)
    finally:
        svc.close()
