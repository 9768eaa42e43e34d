"""Long-form synthesis on the device: the join operator against its numpy restatement (tests/longform_ref.py, itself checked on the
CPU by tests/test_longform_host.py) bit for bit, and ``synthesize_long`` / ``stream_long`` / ``submit_long`` end to end - every
segment against the CPU oracle, the joined waveform against the restatement's join of the engine's own untrimmed parts."""
import numpy as np
import pytest
import torch

import longform_ref as R
from conftest import assert_request_matches_oracle, oracle_request
from sopro_amd import hip
from sopro_amd.longform import group_plan, pause_samples, split_text

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GREEDY = dict(top_p=0.0, temperature=1.0, anti_loop=False)
TEXT = ("Hello there. This is a rather long sentence, with several clauses, that will not fit in forty characters.\n\n"
        "A new paragraph begins here! Is it fine? Yes.")
MAX_CHARS = 40


def _check_operator(wav_np, lens, gaps, *, stream=None, slack=0, **kw):
    want, w_edges, w_offs = R.join(wav_np, lens, gaps, **kw)
    if wav_np.flags["C_CONTIGUOUS"]:
        wav = torch.from_numpy(wav_np).to(DEV)
    else:  # columns of a wider array: keep its row pitch on the device
        wav = torch.from_numpy(wav_np.base).to(DEV)[:, : wav_np.shape[1]]
        assert wav.stride(0) == wav_np.strides[0] // 4
    out_buf = None
    if slack:
        out_buf = torch.full((sum(lens) + sum(gaps) + slack,), -555.0, device=DEV)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            out, edges, offs = hip.join_segments(wav, lens, gaps, out=out_buf, **kw)
        stream.synchronize()
    else:
        out, edges, offs = hip.join_segments(wav, lens, gaps, out=out_buf, **kw)
    assert edges.tolist() == w_edges.tolist()
    assert offs.tolist() == w_offs.tolist()
    assert out.dtype == torch.float32 and tuple(out.shape) == want.shape
    assert torch.equal(out.cpu(), torch.from_numpy(want)), f"{int((out.cpu() != torch.from_numpy(want)).sum())} samples differ"
    if out_buf is not None:
        total = int(w_offs[-1])
        assert bool((out_buf[total:] == -555.0).all()), "something at or past `total` was written"
    return out, edges, offs


@pytest.mark.parametrize("kw", [dict(), dict(trim=False), dict(fade_len=0), dict(fade_len=1), dict(hop=1920), dict(rel=0.5, keep=0, fade_len=7)],
                         ids=["default", "no-trim", "fade0", "fade1", "hop1920", "rel0.5-keep0-fade7"])
def test_join_operator_designed_batch(kw):
    wav_np, lens, gaps = R.designed_batch(3)
    out, edges, offs = _check_operator(wav_np, lens, gaps, **kw)
    assert not bool((out == 777.0).any()), "a sample past a row's length reached the output"
    if not kw:
        assert edges.tolist() == R.DESIGNED_EDGES and int(offs[-1]) == R.DESIGNED_TOTAL


def test_join_operator_clips_at_the_capacity_of_out():
    wav_np, lens, gaps = R.designed_batch(4)
    wav = torch.from_numpy(wav_np).to(DEV)
    buf = torch.full((200000,), -555.0, device=DEV)
    with pytest.raises(hip.SoproHipError, match="157546"):
        hip.join_segments(wav, lens, gaps, out=buf[:1001])
    torch.cuda.synchronize()
    assert bool((buf[1001:] == -555.0).all())
    want, _, _ = R.join(wav_np, lens, gaps)
    assert torch.equal(buf[:1001].cpu(), torch.from_numpy(want[:1001]))  # what fits is still the right prefix


def test_join_operator_full_size_ragged_on_a_side_stream():
    rng = np.random.default_rng(11)
    n_seg, T = 64, 400 * 1920
    base = rng.random((n_seg, T + 1), dtype=np.float32) * 2 - 1   # rows T + 1 apart: row starts are not 16-byte aligned
    wav_np = base[:, :T]
    lens = [int(v) for v in rng.integers(1000, T + 1, size=n_seg)]
    lens[0], lens[5], lens[9], lens[17], lens[40] = T, 1, 0, 4 * 50000 + 1, 4 * 60000 + 3
    assert any(v % 4 for v in lens)
    for k in range(n_seg):
        if k % 7 != 3:  # silent head / tail of random length (some rows keep sound up to their edges)
            h, t = int(rng.integers(0, lens[k] // 2 + 1)), int(rng.integers(0, lens[k] // 3 + 1))
            wav_np[k, :h] = 0.0
            wav_np[k, lens[k] - t: lens[k]] = 0.0
    wav_np[23, : lens[23]] *= np.float32(1e-3)  # a quiet row: the threshold follows the row's own peak
    gaps = [int(v) for v in rng.integers(0, 15000, size=n_seg)]
    _check_operator(wav_np, lens, gaps, stream=torch.cuda.Stream(device=DEV), slack=16)


# ------------------------------------------------------------------------------------------ end to end
def _register(tts, text, max_chars=MAX_CHARS):
    segs = split_text(text, max_chars=max_chars)
    for s in segs:
        tts.tokenizer.table[s.text] = [1 + (ord(c) % 500) for c in s.text]
    return segs


def _ref_tq(seed=5):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 2048, size=(24, 32)))


def _restated_join(res, segs, **kw):
    parts = [p.wav.reshape(-1).cpu().numpy() for p in res.parts]
    lens = [int(p.size) for p in parts]
    rows = np.full((len(parts), max(1, max(lens))), 777.0, dtype=np.float32)
    for k, p in enumerate(parts):
        rows[k, : lens[k]] = p
    gaps = [pause_samples(s.boundary) for s in segs]
    gaps[-1] = 0
    return R.join(rows, lens, gaps, **kw)


def test_synthesize_long_greedy_matches_oracle_and_restated_join(tts, cfg, mc, w, mw):
    segs = _register(tts, TEXT)
    assert 6 <= len(segs) <= 7 and "paragraph" in [s.boundary for s in segs] and "clause" in [s.boundary for s in segs]
    ref_tq = _ref_tq()
    kw = dict(max_frames=12, **GREEDY)
    res = tts.synthesize_long(TEXT, ref_tokens_tq=ref_tq, max_chars=MAX_CHARS, keep_parts=True, seed=3, **kw)
    torch.cuda.synchronize()
    assert res.groups == [len(segs)] and len(res.parts) == len(segs) == len(res.segments) == len(res.edges)
    for k, s in enumerate(segs):
        ids = torch.tensor(tts.tokenizer.table[s.text])
        otoks, owav, oref = oracle_request(ids, ref_tq, w, mw, cfg, mc, **kw)
        assert_request_matches_oracle(res.parts[k].wav, res.parts[k].tokens, otoks, owav, oref, ids, w, mw, cfg, mc, f"segment {k}", **kw)
    want, w_edges, w_offs = _restated_join(res, segs)
    assert tuple(res.wav.shape) == (1, 1, want.shape[0]) and res.wav.is_cuda
    assert torch.equal(res.wav.reshape(-1).cpu(), torch.from_numpy(want))
    assert [list(e) for e in res.edges] == w_edges.tolist()
    assert res.segments == [(segs[k].text, int(w_offs[k]), int(w_offs[k] + w_edges[k, 1] - w_edges[k, 0])) for k in range(len(segs))]
    # more than one group: the same parts, the same joined waveform (a group keeps its last pause, the text's last one is dropped)
    res2 = tts.synthesize_long(TEXT, ref_tokens_tq=ref_tq, max_chars=MAX_CHARS, keep_parts=True, seed=3, plan="throughput", max_rows=3, **kw)
    assert res2.groups == group_plan(len(segs), "throughput", 3) and len(res2.groups) > 1
    want2, w_edges2, w_offs2 = _restated_join(res2, segs)
    assert torch.equal(res2.wav.reshape(-1).cpu(), torch.from_numpy(want2))
    assert [c[1:] for c in res2.segments] == [(int(w_offs2[k]), int(w_offs2[k] + w_edges2[k, 1] - w_edges2[k, 0])) for k in range(len(segs))]
    # a threshold high enough to cut into these (noise-like, synthetic-checkpoint) waveforms: edges, fades and cues move together
    res3 = tts.synthesize_long(TEXT, ref_tokens_tq=ref_tq, max_chars=MAX_CHARS, keep_parts=True, seed=3, trim_db=-2.0, keep_ms=10.0, fade_ms=1.0, **kw)
    want3, w_edges3, w_offs3 = _restated_join(res3, segs, rel=float(np.float32(10.0 ** (-2.0 / 20.0))), keep=1, fade_len=24)
    print("edges at -2 dB:", res3.edges)
    assert torch.equal(res3.wav.reshape(-1).cpu(), torch.from_numpy(want3)) and [list(e) for e in res3.edges] == w_edges3.tolist()
    assert any(e != f for e, f in zip(res3.edges, res.edges)), "nothing was trimmed at -2 dB: this case checks nothing"
    assert [c[1] for c in res3.segments] == [int(v) for v in w_offs3[:-1]]
    # empty text
    empty = tts.synthesize_long("  \n ", ref_tokens_tq=ref_tq)
    assert tuple(empty.wav.shape) == (1, 1, 0) and empty.segments == [] and empty.groups == []
    assert list(tts.stream_long("", ref_tokens_tq=ref_tq)) == []


def test_synthesize_long_seeds(tts_noeos):
    tts = tts_noeos
    segs = _register(tts, TEXT)
    n = len(segs)
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(max_frames=10, top_p=0.9, temperature=1.05, anti_loop=True)
    s = 41
    a = tts.synthesize_long(TEXT, ref=ref, max_chars=MAX_CHARS, seed=s, plan=[n], keep_parts=True, **kw)
    b = tts.synthesize_long(TEXT, ref=ref, max_chars=MAX_CHARS, seed=s, plan=[n], **kw)
    c = tts.synthesize_long(TEXT, ref=ref, max_chars=MAX_CHARS, seed=s + 1, plan=[n], keep_parts=True, **kw)
    assert a.wav.numel() > 0 and torch.equal(a.wav, b.wav) and a.segments == b.segments
    assert not all(torch.equal(x.tokens, y.tokens) for x, y in zip(a.parts, c.parts)), "another seed drew the same tokens everywhere"
    assert a.wav.shape != c.wav.shape or not torch.equal(a.wav, c.wav)
    # one group: the parts are the rows of the one synthesize_batch call with nonce (seed + k) and row id 0 per segment
    batch = tts.synthesize_batch([x.text for x in segs], [ref] * n, seed=s, nonces=[(s + k) & 0xFFFFFFFF for k in range(n)], row_ids=[0] * n, **kw)
    assert len(batch) == n
    for k in range(n):
        assert torch.equal(a.parts[k].wav, batch[k]), k


def test_stream_long_equals_synthesize_long(tts):
    segs = _register(tts, TEXT)
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(max_frames=12, max_chars=MAX_CHARS, seed=9, **GREEDY)
    pieces = list(tts.stream_long(TEXT, ref=ref, **kw))
    whole = tts.synthesize_long(TEXT, ref=ref, plan="latency", **kw)
    assert len(pieces) == len(group_plan(len(segs), "latency")) == len(whole.groups)
    assert all(p.dim() == 2 and p.shape[0] == 1 for p in pieces)
    assert torch.equal(torch.cat(pieces, -1), whole.wav.reshape(1, -1))
    # sampled, too: the generator and the one-shot call draw the same
    kw = dict(max_frames=12, max_chars=MAX_CHARS, seed=10)
    assert torch.equal(torch.cat(list(tts.stream_long(TEXT, ref=ref, **kw)), -1), tts.synthesize_long(TEXT, ref=ref, plan="latency", **kw).wav.reshape(1, -1))


def test_submit_long_matches_synthesize_long_without_trimming(tts):
    from sopro_amd.serving import SynthesisService

    segs = _register(tts, TEXT)
    ref = tts.prepare_reference(ref_tokens_tq=_ref_tq())
    kw = dict(max_frames=12, max_chars=MAX_CHARS, trim_db=None, **GREEDY)
    want = tts.synthesize_long(TEXT, ref=ref, **kw)
    torch.cuda.synchronize()
    svc = SynthesisService(tts, max_batch=4, max_wait_ms=20.0, lanes=2, ar_cus=64, ar_parts=1, ar_shared=False)
    try:
        got = svc.submit_long(TEXT, ref, **kw).result(timeout=180)
        empty = svc.submit_long("", ref).result(timeout=30)
    finally:
        svc.close()
    assert len(got.segments) == len(want.segments) == len(segs)
    assert [(t, e - s) for t, s, e in got.segments] == [(t, e - s) for t, s, e in want.segments]
    assert got.segments == want.segments and got.wav.shape == want.wav.shape
    assert want.wav.numel() > 0
    err = float((got.wav - want.wav).abs().max())
    assert err <= 1e-4 * float(want.wav.abs().max()), err
    assert tuple(empty.wav.shape) == (1, 1, 0) and empty.segments == []
