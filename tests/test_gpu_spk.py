"""Voice similarity on the device (MI355X only): the ragged, batched Token2SV (``hip.spk_embed_rows``, csrc/spk.hip) and the cosine
stage (``hip.spk_cosine``) against the float64 restatement of tests/spk_ref.py (itself pinned to the reference by
tests/test_spk_host.py), and the public entry points built on them.  Expected values never come from the code under test.

Bars (the rule of the pitch tests): 4x the largest deviation measured on an MI355X over the same rows, recorded in
profiles/spk_check.md; the speaker vector in any case within 5e-6, the bar ``sv_ref`` is held to (tests/test_gpu_pipeline.py), the
cosine within 1e-5."""
import numpy as np
import pytest
import torch

import spk_ref as R
from conftest import FakeTok
from sopro_amd import SoproTTS, VoiceBank, VoiceMatch, hip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V, Q = 2048, 32
# measured on an MI355X (profiles/spk_check.md), x4
BAR_SV, BAR_H, BAR_LOGIT = 4 * 3.862e-8, 4 * 7.933e-8, 4 * 3.804e-8              # designed rows, the synthetic checkpoint (|h| <= 0.49, |logit| <= 0.046)
BAR_SAT_SV, BAR_SAT_H, BAR_SAT_LOGIT = 4 * 1.854e-7, 4 * 1.532e-6, 4 * 4.031e-5  # the saturated checkpoint (|h| <= 8.2, |logit| <= 142)
BAR_COS = 4 * 4.605e-8
SV_CAP, COS_CAP = 5e-6, 1e-5
assert max(BAR_SV, BAR_SAT_SV) <= SV_CAP and BAR_COS <= COS_CAP
GREEDY = dict(top_p=0.0, temperature=1.0, anti_loop=False)


def _dev(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()) if np.asarray(a).size else 0.0


def _strided_tokens(rows_tq, t_cap, pad):
    """The rows in one int32 buffer with an odd row stride and a base 4 bytes off a 16-byte boundary; padding frames hold ``pad``
    (a valid id)."""
    n = len(rows_tq)
    stride = t_cap * Q + 1
    host = torch.full((1 + n * stride,), int(pad), dtype=torch.int32)
    view = torch.as_strided(host, (n, t_cap, Q), (stride, Q, 1), 1)
    for r, t in enumerate(rows_tq):
        view[r, : t.shape[0]] = t.to(torch.int32)
    dev = host.to(DEV)
    tok = torch.as_strided(dev, (n, t_cap, Q), (stride, Q, 1), 1)
    assert tok.stride(0) % 2 == 1 and tok.data_ptr() % 16 != 0
    return tok


class _Case:
    """Rows of given lengths, their float64 Token2SV (computed once, never written again) and what the engine gives for them."""

    def __init__(self, lens, weights, seed):
        g = torch.Generator().manual_seed(seed)
        self.lens = list(lens)
        self.t_cap = max(self.lens)
        self.rows = [torch.randint(0, V, (n, Q), generator=g) for n in self.lens]
        self.sv64, self.h64, self.lg64 = [], [], []
        for t in self.rows:
            if t.shape[0] == 0:
                sv, h, lg = np.zeros(192), np.zeros((0, 192)), np.zeros(0)
            else:
                sv, h, lg = R.token2sv(t.numpy(), weights, V, stages=True)
            for a in (sv, h, lg):
                a.setflags(write=False)
            self.sv64.append(sv), self.h64.append(h), self.lg64.append(lg)

    def tokens(self, pad):
        return _strided_tokens(self.rows, self.t_cap, pad)

    def check(self, eng, bars, what):
        n = len(self.lens)
        buf = torch.full((n + 1, 192 + 3), -777.0, device=DEV)
        sv, h, lg = hip.spk_embed_rows(eng, self.tokens(0), self.lens, debug=True, out=buf[:n])
        torch.cuda.synchronize()
        assert sv.data_ptr() == buf.data_ptr() and tuple(sv.shape) == (n, 192)
        assert bool((buf[n] == -777.0).all()) and bool((buf[:n, 192:] == -777.0).all()), "the canary around sv was written"
        sv, h, lg = sv.cpu().numpy(), h.cpu().numpy(), lg.cpu().numpy()
        assert np.isfinite(sv).all() and np.isfinite(h).all() and np.isfinite(lg).all()
        d_sv = d_h = d_lg = 0.0
        for r, T in enumerate(self.lens):
            # stage by stage: a wrong halo rule shows in h at the frames where it happens
            e_h, e_lg, e_sv = _dev(h[r, :T], self.h64[r]), _dev(lg[r, :T], self.lg64[r]), _dev(sv[r], self.sv64[r])
            print(f"{what} row {r:2d} T={T:3d}: |dh| {e_h:.3e} |dlogit| {e_lg:.3e} |dsv| {e_sv:.3e}")
            assert e_h <= bars[1], (what, "h", r, T, e_h, int(np.abs(h[r, :T] - self.h64[r]).max(1).argmax()))
            assert e_lg <= bars[2], (what, "logit", r, T, e_lg)
            assert e_sv <= min(bars[0], SV_CAP), (what, "sv", r, T, e_sv)
            assert not h[r, T:].any() and not lg[r, T:].any(), (what, r, "debug entries past the row's length were written")
            d_sv, d_h, d_lg = max(d_sv, e_sv), max(d_h, e_h), max(d_lg, e_lg)
        print(f"{what}: max |dsv| {d_sv:.3e}  |dh| {d_h:.3e} (|h| <= {max(float(np.abs(x).max()) for x in self.h64 if x.size):.3g})  "
              f"|dlogit| {d_lg:.3e} (|logit| <= {max(float(np.abs(x).max()) for x in self.lg64 if x.size):.3g})")
        return sv


@pytest.fixture(scope="module")
def designed(sopro_np):
    lens = [n for n, _ in R.designed_rows(hip.SPK_TILE_FRAMES)]
    TF = hip.SPK_TILE_FRAMES
    assert lens == [1, 2, 3, 4, 6, 7, TF - 1, TF, TF + 1, TF + 3, TF + 5, TF + 6, TF + 7, 2 * TF, 2 * TF + 1, 150, 400, 0]
    return _Case(lens, sopro_np, 21)


def test_designed_rows_match_the_restatement(tts, designed):
    sv = designed.check(tts.model.eng, (BAR_SV, BAR_H, BAR_LOGIT), "designed")
    assert not sv[designed.lens.index(0)].any(), "a row without frames must give a zero vector"
    norms = np.sqrt((sv.astype(np.float64) ** 2).sum(1))
    assert np.abs(norms[:-1] - 1.0).max() < 1e-6


def test_padding_never_reaches_a_row(tts, designed):
    eng, c = tts.model.eng, designed
    a = hip.spk_embed_rows(eng, c.tokens(0), c.lens)
    b = hip.spk_embed_rows(eng, c.tokens(V - 1), c.lens)
    assert torch.equal(a, b), "the padding frames' ids changed a speaker vector"
    tok = c.tokens(V - 1)
    for r, T in enumerate(c.lens):
        alone = hip.spk_embed_rows(eng, tok[r: r + 1, : max(T, 1)], [T])
        assert torch.equal(alone[0], a[r]), (r, T, "a row in the batch differs from the same row alone")


def test_two_calls_and_a_side_stream_give_the_same_bits(tts, designed):
    eng, c = tts.model.eng, designed
    tok = c.tokens(0)
    first = hip.spk_embed_rows(eng, tok, c.lens)
    assert torch.equal(first, hip.spk_embed_rows(eng, tok, c.lens))
    torch.cuda.synchronize()
    # tokens and lengths made ON the side stream right in front of the call (a few passes over a buffer many times their size, so
    # the call is queued long before they exist) and nothing on the host waits in between
    s = torch.cuda.Stream(device=DEV)
    big = torch.zeros(64, *tok.shape, dtype=torch.int32, device=DEV)
    lens_src = torch.tensor(c.lens, dtype=torch.int32, device=DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(4):
            big = big + 1
        made = (big.sum(0) - 256 + tok).to(torch.int32).contiguous()
        lens_d = (lens_src + (big[0, 0, 0, 0] - 4)).to(torch.int32)
        side = hip.spk_embed_rows(eng, made, lens_d)
    s.synchronize()
    assert torch.equal(made, tok) and torch.equal(lens_d, lens_src)
    assert torch.equal(side, first)


def test_against_the_shipped_per_voice_path(tts, designed):
    """Two correct fp32 orders of the same arithmetic: each within 5e-6 of the truth, so within 2 x 5e-6 of each other."""
    TF = hip.SPK_TILE_FRAMES
    for T in (7, TF + 1, 150):
        t = designed.rows[designed.lens.index(T)]
        got = tts.speaker_vectors(tokens=t)
        want = tts.model.token2sv(t.unsqueeze(0))
        assert tuple(got.shape) == (1, 192) and got.is_cuda
        assert _dev(got.cpu(), want.cpu()) <= 2 * SV_CAP, T
        assert _dev(got.cpu()[0], designed.sv64[designed.lens.index(T)]) <= BAR_SV


@pytest.fixture(scope="module")
def saturated(cfg, sopro_np, mimi_np):
    """A peaked softmax, a saturated tanh and GELU tails: the last pooling projection x 200, the embedding x 30."""
    wts = dict(sopro_np)
    wts["token2sv.pool.attn.2.weight"] = (sopro_np["token2sv.pool.attn.2.weight"] * np.float32(200.0)).astype(np.float32)
    wts["token2sv.emb.weight"] = (sopro_np["token2sv.emb.weight"] * np.float32(30.0)).astype(np.float32)
    return SoproTTS.from_weights(cfg, wts, mimi_np, FakeTok(), device=DEV), wts


def test_saturated_arithmetic(saturated):
    tts2, wts = saturated
    c = _Case([7, hip.SPK_TILE_FRAMES + 1, 150, 400], wts, 22)
    c.check(tts2.model.eng, (BAR_SAT_SV, BAR_SAT_H, BAR_SAT_LOGIT), "saturated")


def test_cosine_modes():
    rng = np.random.default_rng(8)
    worst = 0.0
    for na, nb in ((1, 1), (33, 65)):
        a, b = rng.standard_normal((na, 192)).astype(np.float32), rng.standard_normal((nb, 192)).astype(np.float32)
        if na > 1:
            a[5], b[7] = 0.0, 0.0                     # zero vectors
            a[9] = b[9] * np.float32(0.5)             # a parallel pair
        ad, bd = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        bank = hip.spk_cosine(ad, bd, bank=True).cpu().numpy()
        assert bank.shape == (na, nb)
        worst = max(worst, _dev(bank, R.cosine_bank(a, b)))
        pair = hip.spk_cosine(ad, bd[:na]).cpu().numpy()
        assert pair.shape == (na,)
        worst = max(worst, _dev(pair, R.cosine(a, b[:na])))
        scaled = hip.spk_cosine(ad * 3.0, bd, bank=True).cpu().numpy()
        worst = max(worst, _dev(scaled, R.cosine_bank(a, b)))
        if na > 1:
            assert not bank[5].any() and not bank[:, 7].any() and pair[5] == 0.0 and pair[7] == 0.0, "a zero vector gives 0.0"
            assert abs(pair[9] - 1.0) <= BAR_COS
            # rows of a wider matrix (a row stride that is not the width)
            wide = torch.zeros(na, 200, device=DEV)
            wide[:, :192] = ad
            assert torch.equal(hip.spk_cosine(wide[:, :192], bd, bank=True).cpu(), torch.from_numpy(bank))
    print(f"cosine: max deviation {worst:.3e}")
    assert worst <= min(BAR_COS, COS_CAP), worst
    with pytest.raises(hip.SoproHipError):
        hip.spk_cosine(torch.zeros(2, 192, device=DEV), torch.zeros(3, 192, device=DEV))
    with pytest.raises(hip.SoproHipError):
        hip.spk_cosine(torch.zeros(2, 192, device=DEV), torch.zeros(2, 64, device=DEV), bank=True)


def test_identify_voice(tts, sopro_np):
    g = torch.Generator().manual_seed(11)
    toks = [torch.randint(0, 2048, (1, T, 32), generator=g) for T in range(5, 13)]
    sv64 = np.stack([R.token2sv(t[0].numpy(), sopro_np, V) for t in toks])
    c64 = R.cosine_bank(sv64, sv64)
    wrong = float((c64 - 2.0 * np.eye(8)).max())
    print(f"identification: best wrong match {wrong:.5f}")
    assert wrong <= 1.0 - 1e-3 and np.abs(np.diag(c64) - 1.0).max() < 1e-12, "the voices of this test are not separable"
    refs = [tts.prepare_reference(ref_tokens_tq=t[0], ref_seconds=0) for t in toks]
    bank = VoiceBank(refs, names=[f"voice{i}" for i in range(8)])
    assert bank.vectors.is_cuda and len(bank) == 8
    for i, t in enumerate(toks):
        hits = tts.identify_voice(voices=bank, tokens=t[0], top=3)
        assert len(hits) == 3 and hits[0].index == i and hits[0].name == f"voice{i}", (i, hits)
        assert hits[0].cosine >= 1.0 - 1e-5 and hits[0].cosine >= hits[1].cosine >= hits[2].cosine
        for h in hits:
            assert abs(h.cosine - c64[i, h.index]) <= COS_CAP, (i, h)
    assert len(tts.identify_voice(voices=refs, tokens=toks[0][0], top=20)) == 8  # (a plain sequence of references; top truncates)
    assert len(tts.identify_voice(voices=bank, tokens=toks[0][0], top=1)) == 1
    with pytest.raises(ValueError):
        tts.identify_voice(voices=bank, tokens=toks[0][0], top=0)
    with pytest.raises(ValueError):
        tts.identify_voice(voices=bank)


# ---------------------------------------------------------------------------------------------- API seams
@pytest.fixture(scope="module")
def tts_eos(cfg, sopro_np, mimi_np):
    """The EOS-enabled checkpoint with the EOS logit raised (as the ragged-batch tests of the pipeline do): rows end early."""
    wts = dict(sopro_np)
    hb = sopro_np["ar.head.bias"].copy()
    hb[2048] = 3.9
    wts["ar.head.bias"] = hb
    return SoproTTS.from_weights(cfg, wts, mimi_np, FakeTok(), device=DEV), wts


def _want_match(tokens_tq, ref, weights):
    T = int(tokens_tq.shape[0])
    if T == 0:
        return VoiceMatch(0.0, 0)
    sv = R.token2sv(tokens_tq.cpu().numpy(), weights, V)
    return VoiceMatch(float(R.cosine(sv[None], ref.sv_ref.double().cpu().numpy().reshape(1, -1))[0]), T)


def _same(got, want):
    assert isinstance(got, VoiceMatch) and got.frames == want.frames and abs(got.cosine - want.cosine) <= COS_CAP, (got, want)


def test_synthesize_batch_and_synthesize_sinks(tts_eos):
    tts, wts = tts_eos
    rng = np.random.default_rng(61)
    ids = [torch.from_numpy(rng.integers(0, 512, size=n)) for n in (19, 11, 26)]
    refs = [tts.prepare_reference(ref_tokens_tq=torch.from_numpy(rng.integers(0, 2048, size=(22, 32)))) for _ in ids]
    kw = dict(max_frames=40, style_strength=1.0, top_p=0.0, temperature=0.8, anti_loop=False, min_gen_frames=6, text_ids=ids, seed=5)
    plain = tts.synthesize_batch([""] * 3, refs, padded=True, **kw)
    sink = ["stale"]
    before = hip.spk_calls
    out = tts.synthesize_batch([""] * 3, refs, padded=True, similarity=sink, **kw)
    assert hip.spk_calls == before + 2  # one Token2SV call and one cosine call for the whole batch
    print("frames:", out.frames, "matches:", sink)
    assert min(out.frames) < 40 and len(set(out.frames)) >= 2, f"no row stopped early: {out.frames}"
    assert out.frames == plain.frames and torch.equal(out.tokens, plain.tokens)
    assert torch.equal(out.wav, plain.wav), "the sink changed the waveforms"
    assert len(sink) == 3
    for b in range(3):
        _same(sink[b], _want_match(out.tokens[b, : out.frames[b]], refs[b], wts))
    # one utterance through synthesize, seeded
    tts.tokenizer.table["one"] = ids[1].tolist()
    kw1 = {k: v for k, v in kw.items() if k != "text_ids"}
    s1 = []
    w1 = tts.synthesize("one", ref=refs[1], similarity=s1, **kw1)
    assert torch.equal(w1, tts.synthesize("one", ref=refs[1], **kw1))
    toks = tts.model.generate_tokens(ids[1], refs[1], **kw1)
    assert int(w1.shape[-1]) == 1920 * int(toks.shape[0]) and len(s1) == 1
    _same(s1[0], _want_match(toks, refs[1], wts))


def test_synthesize_long_voice_match(tts, sopro_np):
    from sopro_amd.longform import split_text

    text = "Hello there. A new paragraph begins here! Is it fine? Yes."
    for s in split_text(text, max_chars=40):
        tts.tokenizer.table[s.text] = [1 + (ord(c) % 500) for c in s.text]
    ref = tts.prepare_reference(ref_tokens_tq=torch.from_numpy(np.random.default_rng(5).integers(0, 2048, size=(24, 32))))
    kw = dict(ref=ref, max_chars=40, keep_parts=True, seed=3, max_frames=12, **GREEDY)
    res = tts.synthesize_long(text, voice_match=True, **kw)
    assert len(res.voice) == len(res.segments) == len(res.parts) >= 3
    for k, p in enumerate(res.parts):
        _same(res.voice[k], _want_match(p.tokens, ref, sopro_np))
    off = tts.synthesize_long(text, **kw)
    assert off.voice is None and torch.equal(off.wav, res.wav)


@pytest.fixture(scope="module")
def tts_enc(cfg, mc, sopro_np):
    """The engine with the codec's encoder side loaded (``wav=`` goes through ``codec.encode_waveform``)."""
    from conftest import SEED
    from sopro_amd.weights import synth_mimi_weights

    return SoproTTS.from_weights(cfg, sopro_np, synth_mimi_weights(mc, SEED, with_encoder=True), FakeTok(), device=DEV)


def test_voice_similarity_of_a_waveform(tts_enc, sopro_np):
    tts = tts_enc
    ref = tts.prepare_reference(ref_tokens_tq=torch.from_numpy(np.random.default_rng(6).integers(0, 2048, size=(24, 32))))
    g = torch.Generator().manual_seed(4)
    clip = (torch.rand(1, 1, 3 * 1920 + 700, generator=g) * 2 - 1) * 0.3
    codes = tts.codec.encode_waveform(clip.reshape(-1))
    assert tuple(codes.shape) == (4, 32)
    _same(tts.voice_similarity(wav=clip, ref=ref), _want_match(codes, ref, sopro_np))
    # tokens, one clip and a padded batch with one reference per row
    _same(tts.voice_similarity(tokens=codes, ref=ref), _want_match(codes, ref, sopro_np))
    batch = torch.stack([codes, codes.flip(0)])
    got = tts.voice_similarity(tokens=batch, lens=[4, 2], ref=[ref, ref])
    assert len(got) == 2
    _same(got[0], _want_match(codes, ref, sopro_np))
    _same(got[1], _want_match(codes.flip(0)[:2], ref, sopro_np))
    assert tts.voice_similarity(tokens=batch, lens=[0, 0], ref=ref) == [VoiceMatch(0.0, 0)] * 2
    for bad in (dict(), dict(wav=clip, tokens=codes), dict(wav=clip, lens=[1])):
        with pytest.raises(ValueError):
            tts.voice_similarity(ref=ref, **bad)
    with pytest.raises(TypeError):
        tts.voice_similarity(tokens=codes, ref=ref.sv_ref)
