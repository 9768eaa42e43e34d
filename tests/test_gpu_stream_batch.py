"""Batched streaming on the MI355X: the batched stream decoder (sopro_mimi_decode_stream_batch) against the single-stream one, and
SoproTTS.stream_batch against the reference's streamed fixtures and against each row's own stream()."""
import numpy as np
import pytest
import torch

from conftest import FakeTok, golden

pytestmark = pytest.mark.gpu
GREEDY = dict(top_p=0.0, temperature=1.0, anti_loop=False)


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _err(a, b):
    return float((a.reshape(-1).cpu() - b.reshape(-1).cpu()).abs().max())


# ------------------------------------------------------------------ decoder level
@pytest.mark.parametrize("trim", ["none", "legacy"])
def test_one_row_is_bit_identical_to_the_single_stream_decoder(tts_noeos, trim):
    from sopro_amd.codec import MimiStreamDecoder

    codes = _t(golden("full400")["tokens"].astype(np.int64))[:240]
    dec = MimiStreamDecoder(tts_noeos.codec, trim=trim)
    sst, bst = None, None
    for i in range(0, 240, 6):
        w1, sst = dec.decode_step(codes[i:i + 6], sst)
        (wb,), bst = dec.decode_step_batch([codes[i:i + 6]], bst)
        assert wb.shape == w1.shape == (1, 6 * 1920)
        assert torch.equal(wb, w1), (trim, i)
        assert (bst.pos, bst.kv_len, bst.evict) == (sst.pos, sst.kv_len, sst.evict), i


def _three_rows(tts, trim, stop_after=None, short_last=None):
    """Rows at token offsets 0 / 80 / 160 of full400, 40 chunks of 6 frames; stop_after[r] = last chunk of row r; short_last[r] =
    frames of that last chunk.  Each row against its own MimiStreamDecoder."""
    from sopro_amd.codec import MimiStreamDecoder

    g = golden("full400")
    codes = _t(g["tokens"].astype(np.int64))
    offs = [0, 80, 160]
    stop_after = stop_after or {}
    short_last = short_last or {}
    dec = MimiStreamDecoder(tts.codec, trim=trim)
    singles = [[MimiStreamDecoder(tts.codec, trim=trim), None] for _ in offs]
    bst, order, worst = None, [0, 1, 2], 0.0
    scale = float(np.abs(g["wav"]).max())
    for k in range(40):
        chunks = []
        for r in order:
            last = stop_after.get(r, 39)
            if k > last:
                chunks.append(None)
                continue
            n = short_last.get(r, 6) if k == last else 6
            chunks.append(codes[offs[r] + 6 * k: offs[r] + 6 * k + n])
        wavs, bst = dec.decode_step_batch(chunks, bst)
        for r, c, w in zip(order, chunks, wavs):
            if c is None:
                assert w is None
                continue
            d, st = singles[r]
            want, singles[r][1] = d.decode_step(c, st)
            assert w.shape == want.shape == (1, int(c.shape[0]) * 1920), (k, r)
            worst = max(worst, _err(w, want))
        order = [r for r, c in zip(order, chunks) if c is not None]
    assert worst < 2e-5 * scale, worst
    return bst


@pytest.mark.parametrize("trim", ["none", "legacy"])
def test_three_rows_match_their_own_stream_decoders(tts_noeos, trim):
    st = _three_rows(tts_noeos, trim)
    assert st.rows == 3


@pytest.mark.parametrize("trim", ["none", "legacy"])
def test_rows_leave_the_batch_and_a_ragged_final_chunk(tts_noeos, trim):
    # row 1 leaves after chunk 10, row 0 after chunk 25 with a 3-frame final chunk; row 2 runs all 40
    st = _three_rows(tts_noeos, trim, stop_after={1: 10, 0: 25}, short_last={0: 3})
    assert st.rows == 1


def test_c_stage_batch_decoder_matches_the_python_host(tts_noeos):
    from sopro_amd.codec import MimiStreamDecoder
    from sopro_amd.stages import StageEngine, StageStreamBatchDecoder

    g = golden("full400")
    codes = _t(g["tokens"].astype(np.int64))
    eng = StageEngine(tts_noeos)
    try:
        cdec = StageStreamBatchDecoder(eng, rows=2, cap_rows=1024)
        pdec, pst = MimiStreamDecoder(tts_noeos.codec), None
        worst = 0.0
        for k in range(30):
            chunks = [codes[6 * k: 6 * k + 6], codes[200 + 6 * k: 206 + 6 * k]] if k < 20 else [None, codes[200 + 6 * k: 206 + 6 * k]]
            if k > 20:
                chunks = [codes[200 + 6 * k: 206 + 6 * k]]
            cw = cdec.decode_step(chunks)
            pw, pst = pdec.decode_step_batch(chunks, pst)
            for a, b in zip(cw, pw):
                assert (a is None) == (b is None)
                if a is not None:
                    worst = max(worst, _err(a, b))
        assert worst < 2e-5 * float(np.abs(g["wav"]).max()), worst
        assert (cdec.st.pos, cdec.st.kv_len, cdec.st.rows) == (pst.pos, pst.kv_len, pst.rows)
    finally:
        eng.close()


# ------------------------------------------------------------------ end to end
def _rows(tts, n_extra, seed):
    gi = golden("full200")
    rng = np.random.default_rng(seed)
    ids = [_t(gi["ids"])] + [torch.from_numpy(rng.integers(1, 512, size=int(rng.integers(20, 70)))) for _ in range(n_extra)]
    refs = [tts.prepare_reference(ref_tokens_tq=_t(gi["ref_tq"]))] + [
        tts.prepare_reference(ref_tokens_tq=torch.from_numpy(rng.integers(0, 2048, size=(int(rng.integers(60, 160)), 32)))) for _ in range(n_extra)]
    return ids, refs


def _per_row(steps, B):
    rows = [[] for _ in range(B)]
    for s in steps:
        assert len(s) == B
        for b, c in enumerate(s):
            if c is not None:
                rows[b].append(c)
    return rows


@pytest.mark.parametrize("name,cf,trim", [("stream_c1", 1, "none"), ("stream160", 6, "none"), ("stream_c16", 16, "none"),
                                          ("stream_legacy", 6, "legacy")])
def test_stream_batch_matches_the_reference_and_each_rows_stream(tts_noeos, name, cf, trim):
    g = golden(name)
    tts = tts_noeos
    ids, refs = _rows(tts, 2, seed=cf)
    kw = dict(max_frames=int(g["max_frames"]), style_strength=1.0, chunk_frames=cf, cache_trim=trim, **GREEDY)
    rows = _per_row(list(tts.stream_batch([""] * 3, refs, text_ids=ids, **kw)), 3)
    assert [int(c.shape[1]) for c in rows[0]] == g["chunk_sizes"].tolist()
    assert _err(torch.cat(rows[0], dim=1), _t(g["stream"])) < 1e-4 * float(np.abs(g["stream"]).max())
    for b in (1, 2):
        want = list(tts.stream("", text_ids=ids[b], ref=refs[b], **kw))
        assert [int(c.shape[1]) for c in rows[b]] == [int(c.shape[1]) for c in want], b
        w = torch.cat(want, dim=1)
        assert _err(torch.cat(rows[b], dim=1), w) < 1e-4 * float(w.abs().max()), b


@pytest.fixture(scope="module")
def tts_eos(cfg, sopro_np, mimi_np):
    """The EOS-enabled checkpoint with the EOS logit raised (as the ragged-batch test of the pipeline does): rows end early."""
    from sopro_amd import SoproTTS

    wts = dict(sopro_np)
    hb = sopro_np["ar.head.bias"].copy()
    hb[2048] = 3.9
    wts["ar.head.bias"] = hb
    return SoproTTS.from_weights(cfg, wts, mimi_np, FakeTok(), device="cuda:0")


def test_ragged_ends_match_each_rows_stream(tts_eos):
    tts, cf = tts_eos, 6
    rng = np.random.default_rng(61)
    ids = [torch.from_numpy(rng.integers(0, 512, size=n)) for n in (19, 11, 26, 7, 33, 15)]
    refs = [tts.prepare_reference(ref_tokens_tq=torch.from_numpy(rng.integers(0, 2048, size=(22, 32)))) for _ in ids]
    kw = dict(max_frames=40, style_strength=1.0, chunk_frames=cf, top_p=0.0, temperature=0.8, anti_loop=False, min_gen_frames=6)
    rows = _per_row(list(tts.stream_batch([""] * len(ids), refs, text_ids=ids, **kw)), len(ids))
    lens = []
    for b in range(len(ids)):
        want = list(tts.stream("", text_ids=ids[b], ref=refs[b], **kw))
        sizes = [int(c.shape[1]) for c in want]
        lens.append(sum(sizes) // 1920)
        assert [int(c.shape[1]) for c in rows[b]] == sizes, (b, lens)
        if want:
            w = torch.cat(want, dim=1)
            assert _err(torch.cat(rows[b], dim=1), w) < 1e-4 * float(w.abs().max()), b
    assert len(set(lens)) >= 2 and any(L % cf for L in lens if L < 41), f"inputs are not ragged: {lens}"


def test_sampled_rows_are_reproducible_and_independent_of_order(tts_noeos):
    tts = tts_noeos
    ids, refs = _rows(tts, 2, seed=9)
    seeds = [11, 22, 33]
    kw = dict(max_frames=40, style_strength=1.0, chunk_frames=6, top_p=0.9, temperature=1.05, anti_loop=True)
    a = _per_row(list(tts.stream_batch([""] * 3, refs, text_ids=ids, seeds=seeds, **kw)), 3)
    b = _per_row(list(tts.stream_batch([""] * 3, refs, text_ids=ids, seeds=seeds, **kw)), 3)
    for x, y in zip(a, b):
        assert len(x) == len(y) and all(torch.equal(p, q) for p, q in zip(x, y))
    r = _per_row(list(tts.stream_batch([""] * 3, refs[::-1], text_ids=ids[::-1], seeds=seeds[::-1], **kw)), 3)[::-1]
    for x, y in zip(a, r):
        wx, wy = torch.cat(x, dim=1), torch.cat(y, dim=1)
        assert wx.shape == wy.shape and _err(wx, wy) < 1e-4 * float(wx.abs().max())


# ------------------------------------------------------------------ service
def test_service_streams_concurrent_callers_in_batches(tts_noeos):
    import threading

    from sopro_amd.serving import SynthesisService

    tts = tts_noeos
    ids, refs = _rows(tts, 5, seed=77)
    kw = dict(max_frames=40, style_strength=1.0, chunk_frames=6, **GREEDY)
    want = [torch.cat(list(tts.stream("", text_ids=ids[b], ref=refs[b], **kw)), dim=1) for b in range(5)]
    got, errs = [None] * 5, []
    with pytest.raises(RuntimeError, match="continuous"):
        SynthesisService.submit_stream(type("S", (), {"_closed": False, "engine": object()})(), "", refs[0], text_ids=ids[0])
    with SynthesisService(tts, max_batch=4, max_wait_ms=300.0, lanes=1) as svc:
        go = threading.Barrier(6)

        def reader(b):
            try:
                it = svc.submit_stream("", refs[b], text_ids=ids[b], **kw)
                go.wait()
                got[b] = torch.cat(list(it), dim=1)
            except BaseException as e:  # noqa: BLE001
                errs.append(e)

        def quitter():
            it = svc.submit_stream("", refs[5], text_ids=ids[5], **kw)
            go.wait()
            next(it), next(it)
            it.close()  # stops reading: its row leaves, nobody waits for it

        ts = [threading.Thread(target=reader, args=(b,)) for b in range(5)] + [threading.Thread(target=quitter)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(timeout=300)
        assert not any(t.is_alive() for t in ts) and not errs, errs
        assert svc.stats["stream_batches"] == 2
    for b in range(5):
        assert got[b].shape == want[b].shape and _err(got[b], want[b]) < 1e-4 * float(want[b].abs().max()), b
