"""Voice similarity, host side (no GPU): the float64 restatement of the unpadded Token2SV (tests/spk_ref.py) against the fp32
oracle and the reference-written fixture, the value types and the ranking of sopro_amd/voicematch.py, and the ``similarity=``
sink's argument handling."""
import contextlib
import types

import numpy as np
import pytest
import torch

import spk_ref as R
from conftest import golden
from oracle import sopro_oracle as O
from sopro_amd import SoproTTS, VoiceBank, VoiceHit, VoiceMatch, hip
from sopro_amd import voicematch as VM

# The restatement is float64, the oracle the reference's fp32 arithmetic: what separates them is the oracle's rounding.  A unit vector of
# 192 elements has elements of ~0.07 (half an ulp: 3.7e-9); the error that reaches it through two convs, the pooling and a
# 384-term projection was measured at 4.6e-8 worst over these lengths on the synthetic checkpoint; the bar is 4x that.
BAR = 2e-7
LENGTHS = (1, 2, 3, 4, 6, 7, 31, 32, 33, 38, 64, 65, 150, 200)


def _tokens(T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 2048, (T, 32), generator=g)


def test_restatement_matches_the_fp32_oracle(cfg, w, sopro_np):
    V = int(cfg.codebook_size)
    worst = 0.0
    for T in LENGTHS:
        tok = _tokens(T, 100 + T)
        want = O.token2sv(tok.unsqueeze(0), w, V)[0].double().numpy()
        got = R.token2sv(tok.numpy(), sopro_np, V)
        worst = max(worst, float(np.abs(got - want).max()))
        assert abs(float(np.sqrt((got * got).sum())) - 1.0) < 1e-12
    print(f"restatement vs fp32 oracle: worst |d sv| = {worst:.3e}")
    assert worst <= BAR, worst


def test_restatement_matches_the_reference_fixture(cfg, sopro_np):
    """tests/golden/speaker.npz: the reference's own ``encode_speaker`` under its three crop policies (make_golden_speaker.py)."""
    g = golden("speaker")
    ref_tq = np.asarray(g["ref_tq"])
    T, V = ref_tq.shape[0], int(cfg.codebook_size)
    for name, win in (("default", 150), ("sec4", 50), ("nocrop", T)):  # centre crop, src/sopro/sampling.py:8-13
        s = (T - win) // 2
        got = R.token2sv(ref_tq[s: s + win], sopro_np, V)
        err = float(np.abs(got - np.asarray(g["sv_" + name], np.float64).reshape(-1)).max())
        print(f"restatement vs reference fixture ({name}): {err:.3e}")
        assert err <= BAR, (name, err)


def test_restatement_edge_rows_stay_finite(cfg, sopro_np):
    V = int(cfg.codebook_size)
    one = _tokens(1, 3).numpy()
    sv = R.token2sv(one, sopro_np, V)
    assert np.isfinite(sv).all() and abs(float(np.sqrt((sv * sv).sum())) - 1.0) < 1e-12
    assert R.variance_clamped(one, sopro_np, V) == 192  # T = 1: h == mu, every channel takes the 1e-6 clamp
    const = np.full((40, 32), 7, np.int64)
    sv, h, logit = R.token2sv(const, sopro_np, V, stages=True)
    assert np.isfinite(sv).all() and np.isfinite(h).all() and np.isfinite(logit).all()
    # a constant row is constant away from its ends (three frames of padding per conv reach six frames in)
    assert np.abs(h[6:-6] - h[6]).max() < 1e-12 and np.abs(h[0] - h[6]).max() > 1e-6


def test_restatement_cosine():
    rng = np.random.default_rng(2)
    a, b = rng.standard_normal((5, 192)), rng.standard_normal((7, 192))
    bank = R.cosine_bank(a, b)
    assert bank.shape == (5, 7)
    for i in range(5):
        assert np.allclose(bank[i, :5], [R.cosine(a[i: i + 1], b[n: n + 1])[0] for n in range(5)], atol=1e-15)
    assert R.cosine(np.zeros((1, 4)), np.ones((1, 4)))[0] == 0.0
    assert abs(R.cosine(3.0 * a[:1], a[:1])[0] - 1.0) < 1e-15


def test_designed_rows_cover_the_tile_seams():
    lens = [n for n, _ in R.designed_rows(32)]
    assert lens == [1, 2, 3, 4, 6, 7, 31, 32, 33, 35, 37, 38, 39, 64, 65, 150, 400, 0]


# ---------------------------------------------------------------------------------------------- value types and ranking
def test_voice_match_refuses_bad_values():
    assert VoiceMatch(0.5, 3) == VoiceMatch(0.5, 3) and VoiceMatch(0.0, 0).frames == 0
    for bad in ((float("nan"), 1), (float("inf"), 1), ("0.5", 1), (0.5, -1), (0.5, 1.5), (0.5, True)):
        with pytest.raises(ValueError):
            VoiceMatch(*bad)
    assert [m for m in VM.matches([0.7, 0.9], [4, 0])] == [VoiceMatch(0.7, 4), VoiceMatch(0.0, 0)]


def test_voice_bank_arguments():
    v = [torch.full((192,), float(i + 1)) for i in range(3)]
    bank = VoiceBank(v, names=["a", "b", "c"])
    assert len(bank) == 3 and bank.dim == 192 and bank.vectors.dtype == torch.float32 and bank.vectors.is_contiguous()
    assert VoiceBank(torch.stack(v)).names is None
    # PreparedReference-like objects: their sv_ref, [1, sv_dim] as prepare_reference stores it
    refs = [types.SimpleNamespace(sv_ref=x.reshape(1, -1)) for x in v]
    assert torch.equal(VoiceBank(refs).vectors, bank.vectors)
    assert VM.as_bank(bank) is bank and len(VM.as_bank(refs)) == 3
    assert bank.on("cpu") is bank.vectors
    for bad in ([], torch.zeros(192), [torch.zeros(2, 192)], [torch.zeros(192), torch.zeros(64)], [torch.zeros(4, dtype=torch.long)], [1.0]):
        with pytest.raises(ValueError):
            VoiceBank(bad)
    with pytest.raises(TypeError):
        VoiceBank("voices")
    for names in (["a"], ["a", "b", 3]):
        with pytest.raises(ValueError):
            VoiceBank(v, names=names)


def test_ranking_is_stable_and_ties_go_to_the_lower_index():
    hits = VM.rank([0.2, 0.9, 0.9, -0.1, 0.9], names=list("abcde"), top=4)
    assert hits == [VoiceHit(1, "b", 0.9), VoiceHit(2, "c", 0.9), VoiceHit(4, "e", 0.9), VoiceHit(0, "a", 0.2)]
    assert [h.index for h in VM.rank([0.5, 0.5, 0.5], top=5)] == [0, 1, 2] and VM.rank([0.5], top=1)[0].name is None
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError):
            VM.rank([0.1, 0.2], top=bad)
    with pytest.raises(ValueError):
        VM.rank([0.1, 0.2], names=["a"])


def test_token_rows_arguments():
    t = torch.zeros(5, 32, dtype=torch.long)
    rows, lens, batched = VM.token_rows(t, None, 32)
    assert tuple(rows.shape) == (1, 5, 32) and lens == [5] and not batched
    rows, lens, batched = VM.token_rows(t.unsqueeze(0).expand(3, -1, -1), [5, 0, 2], 32)
    assert lens == [5, 0, 2] and batched
    for tok, ln in ((t.float(), None), (t[:, :31], None), (t, [6]), (t, [1, 2]), (t.unsqueeze(0), [-1]), (t.unsqueeze(0), [1, 2]), (t[0], None)):
        with pytest.raises(ValueError):
            VM.token_rows(tok, ln, 32)


# ---------------------------------------------------------------------------------------------- the sink
class _Tok:
    def encode(self, text):
        return [1, 2, 3]


def _stub_tts(calls):
    """A SoproTTS whose engine halves are stubs: ``synthesize`` runs on the CPU up to the calls under test."""
    def speaker_vectors(tokens_btq, lens):
        calls.append(("speaker_vectors", tuple(tokens_btq.shape), list(lens)))
        return torch.ones(int(tokens_btq.shape[0]), 192)

    model = types.SimpleNamespace(generate_tokens=lambda ids, ref, **kw: torch.zeros(5, 32, dtype=torch.long),
                                  on_stream=lambda bulk=False: contextlib.nullcontext(), speaker_vectors=speaker_vectors, Q=32)
    codec = types.SimpleNamespace(decode_full=lambda tok: torch.zeros(1, 1, 5 * 1920))
    return SoproTTS(model, types.SimpleNamespace(style_strength=1.0, sv_student_dim=192), _Tok(), codec, "cpu")


def test_sinks_refuse_a_non_list():
    tts = SoproTTS.__new__(SoproTTS)  # (refused before anything of the engine is touched)
    for bad in ((), {}, "x", 0):
        with pytest.raises(TypeError, match="similarity"):
            tts.synthesize("hello", ref=object(), similarity=bad)
        with pytest.raises(TypeError, match="similarity"):
            tts.synthesize_batch(["hello"], [object()], similarity=bad)
    VM.sink_of(None, "x")
    VM.sink_of([], "x")


def test_similarity_none_reaches_no_spk_call(monkeypatch):
    calls = []
    monkeypatch.setattr(hip, "spk_embed_rows", lambda *a, **k: calls.append("spk_embed_rows"))

    def fake_cosine(a, b, *, bank=False):
        calls.append(("spk_cosine", tuple(a.shape), tuple(b.shape)))
        return torch.full((int(a.shape[0]),), 0.25)

    monkeypatch.setattr(hip, "spk_cosine", fake_cosine)
    tts = _stub_tts(calls)
    ref = types.SimpleNamespace(sv_ref=torch.ones(1, 192))
    wav = tts.synthesize("hello", ref=ref)
    assert tuple(wav.shape) == (1, 1, 5 * 1920) and calls == []
    sink = ["stale"]
    wav2 = tts.synthesize("hello", ref=ref, similarity=sink)
    assert torch.equal(wav, wav2)
    assert calls == [("speaker_vectors", (1, 5, 32), [5]), ("spk_cosine", (1, 192), (1, 192))]
    assert sink == [VoiceMatch(0.25, 5)]
