"""Word timestamps without a device: the restatement (tests/align_ref.py) against brute force and against the oracle's own blocks,
and the host logic of sopro_amd/align.py on designed strings."""
import numpy as np
import pytest
import torch

import align_ref as R
from sopro_amd import align as A
from sopro_amd import hip


def _check_path(path, bounds, T, S):
    assert len(path) == T and path[0] == 0 and path[-1] == S - 1
    assert all(0 <= path[t] - path[t - 1] <= 1 for t in range(1, T))
    for s, (a, b) in enumerate(bounds):
        assert [t for t in range(T) if path[t] == s] == list(range(a, b))


def test_the_binding_is_there():
    assert callable(hip.align_paths) and callable(hip.align_scores) and isinstance(hip.align_calls, int)
    assert {"sopro_align_scores_f32", "sopro_align_dp_f32", "sopro_align_ws_bytes"} <= set(hip.SYMBOLS)
    lib = hip.load()
    assert lib.sopro_align_ws_bytes(3, 10, 64) == 3 * 10 * 8 and lib.sopro_align_ws_bytes(3, 10, 65) == 3 * 10 * 2 * 8
    assert lib.sopro_align_ws_bytes(1, 1, 2049) == 0
    assert lib.sopro_align_dp_f32(None, 0, 0, None, None, 1, 1, 1, None, 0, None, 0, None, None, None, None) == -2
    assert b"non-NULL" in lib.sopro_last_error()


@pytest.mark.parametrize("seed", range(6))
def test_dp_against_every_monotone_path(seed):
    rng = np.random.default_rng(seed)
    for T, S in [(1, 1), (4, 1), (5, 5), (6, 2), (7, 3), (9, 5), (9, 4), (8, 5)]:
        sc = np.log(rng.uniform(1e-4, 1.0, size=(T, S))).astype(np.float32)
        path, bounds, total, status = R.dp(sc)
        best, who = R.brute(sc)
        assert status == 0
        _check_path(path, bounds, T, S)
        assert np.float32(total) == best and R.path_total(sc, path) == best and path in who, (T, S)


@pytest.mark.parametrize("seed", range(6))
def test_dp_ties_stay(seed):
    """Small integers are exact in fp32, so equal totals are real ties: the path is the best one that stays wherever staying is as
    good, looked at from the last frame backwards."""
    rng = np.random.default_rng(100 + seed)
    n_tied = 0
    for T, S in [(5, 3), (7, 4), (9, 5), (6, 6), (8, 2)]:
        sc = -rng.integers(0, 2, size=(T, S)).astype(np.float32)
        if S > 1:
            sc[:, 1] = sc[:, 0]  # planted: two equal columns leave the frame of the step open
        path, bounds, total, status = R.dp(sc)
        best, who = R.brute(sc)
        _check_path(path, bounds, T, S)
        assert np.float32(total) == best
        n_tied += len(who) > 1
        assert path == max(who, key=lambda p: tuple(reversed(p))), (T, S, who)
    assert n_tied >= 3  # (the case is exercised)
    # a fully flat matrix: every path ties, the chosen one stays as long as it can
    path, _b, total, _s = R.dp(np.zeros((7, 3), np.float32))
    assert path == [0, 1, 2, 2, 2, 2, 2] and total == 0


@pytest.mark.parametrize("seed", range(4))
def test_dp_recovers_planted_alignments(seed):
    rng = np.random.default_rng(200 + seed)
    for S in (1, 3, 17, 70):
        dur = rng.integers(1, 6, size=S)
        want = np.repeat(np.arange(S), dur)
        T = len(want)
        sc = np.full((T, S), -4.0, np.float32)
        sc[np.arange(T), want] = 0.0
        sc = (sc - rng.uniform(0.0, 0.99, size=(T, S))).astype(np.float32)  # on the path > -1, off it < -4
        path, bounds, _total, status = R.dp(sc)
        assert status == 0 and path == want.tolist()
        ends = np.cumsum(dur)
        assert bounds == [(int(e - d), int(e)) for d, e in zip(dur, ends)]


def test_fallback_rows():
    for T, S in [(0, 0), (0, 4), (3, 0), (3, 7), (8, 12), (1, 2)]:
        path, bounds, total, status = R.dp(np.zeros((T, S), np.float32))
        assert status == 1 and total == 0 and len(path) == T and len(bounds) == S
        assert path == [(t * S) // T for t in range(T)] if S else path == [0] * T
        for s, (a, b) in enumerate(bounds):
            assert [t for t in range(T) if path[t] == s] == list(range(a, b)) and 0 <= a <= T
        assert all(bounds[s][0] <= bounds[s + 1][0] for s in range(S - 1))


def test_replay_restates_the_oracle_blocks(cfg, w):
    """align_ref.replay in float32 against the same stack composed from the oracle's public functions."""
    from oracle import sopro_oracle as O

    rng = np.random.default_rng(5)
    T, S, D = 21, 9, int(cfg.d_model)
    cond = torch.from_numpy(rng.standard_normal((T + 1, D)).astype(np.float32))
    txt = torch.from_numpy(rng.standard_normal((S, D)).astype(np.float32))
    toks = rng.integers(0, int(cfg.codebook_size), size=T)
    hidden = []
    qk = R.replay(w, cfg, cond, toks, txt, hidden=hidden)
    prev = torch.tensor([int(cfg.bos_row)] + [int(v) for v in toks[:-1]])
    h = (cond[:T] + w["cb_embed.emb.weight"][prev]).unsqueeze(0)
    for i, dil in enumerate(cfg.ar_dilations):
        h = O.ssm_block(h, w, f"ar.blocks.{i}", dil, True)
        if i in cfg.ar_xattn_layers:
            p = f"ar.x_attns.{i}"
            k, v = O.xattn_kv(txt.unsqueeze(0), w, p, 4)
            q = O._heads(torch.nn.functional.linear(O.rmsnorm(h, w[p + ".nq.weight"]), w[p + ".q_proj.weight"]), 4)
            assert torch.allclose(O._heads(qk[i][0].unsqueeze(0), 4), q, rtol=0, atol=2e-5)
            assert torch.allclose(O._heads(qk[i][1].unsqueeze(0), 4), k, rtol=0, atol=2e-5)
            h = O.text_xattn(h, k, v, None, w, p)
        assert torch.allclose(hidden[i], h[0], rtol=0, atol=5e-5), i
    # the head mean is a distribution over the text, and float64 agrees with float32
    s32, a32 = R.utterance_scores(w, cfg, cond, toks, txt)
    s64, _a = R.utterance_scores(w, cfg, cond, toks, txt, dtype=torch.float64)
    assert torch.allclose(a32.sum(-1), torch.ones(T), atol=1e-5)
    assert float((s32.double() - s64).abs().max()) < 1e-4
    sel, _ = R.utterance_scores(w, cfg, cond, toks, txt, heads=[(1, 0), (5, 3)])
    assert not torch.equal(sel, s32)


# ------------------------------------------------------------------------------------------ sopro_amd/align.py
def test_alignment_confidence():
    a = A.Alignment(path=[0, 0, 1, 1], token_frames=[(0, 2), (2, 4)], total=-4.0)
    assert a.confidence == pytest.approx(np.exp(-1.0)) and a.status == 0
    assert A.Alignment(path=[], token_frames=[], total=0.0, status=1).confidence == 0.0


def test_word_cues_on_designed_strings():
    text = "  Hi, unbelievable world !"
    #        0123456789...
    spans = [(0, 0),                       # BOS
             (2, 4), (4, 5),               # "Hi" "," : punctuation glued to the word
             (5, 8), (8, 14), (14, 18),    # " un" "believ" "able": one word over three tokens, the first with a leading blank
             (18, 24),                     # " world"
             (25, 25)]                     # EOS; "!" has no token
    frames = [(0, 2), (2, 4), (4, 5), (5, 6), (6, 9), (9, 11), (11, 15), (15, 20)]
    cues = A.word_cues(text, spans, frames)
    assert [c.text for c in cues] == ["Hi,", "unbelievable", "world", "!"]
    assert [(c.char_start, c.char_end) for c in cues] == [(2, 5), (6, 18), (19, 24), (25, 26)]
    assert [(c.start_sample, c.end_sample) for c in cues] == [(2 * 1920, 5 * 1920), (5 * 1920, 11 * 1920), (11 * 1920, 15 * 1920), (15 * 1920, 15 * 1920)]
    assert all(text[c.char_start:c.char_end] == c.text for c in cues)
    # a word with no token at the very start sits at 0; a token of blanks only belongs to no word; hop is a parameter
    cues = A.word_cues("a b", [(1, 2), (2, 3)], [(0, 3), (3, 4)], hop=10)
    assert [(c.text, c.start_sample, c.end_sample) for c in cues] == [("a", 0, 0), ("b", 30, 40)]
    assert A.word_cues("", [(0, 0)], [(0, 5)]) == [] and A.word_cues(" \n ", [], []) == []
    with pytest.raises(ValueError):
        A.word_cues("a", [(0, 1)], [])


def test_token_spans_sources():
    class WithOffsets:
        def encode(self, text):
            return [1] + [ord(c) for c in text] + [2]

        def encode_with_offsets(self, text):
            return self.encode(text), [(0, 0)] + [(i, i + 1) for i in range(len(text))] + [(len(text), len(text))]

    assert A.token_spans(WithOffsets(), "ab") == [(0, 0), (0, 1), (1, 2), (2, 2)]

    class FastTok:  # the shape of a Hugging Face fast tokenizer's answer
        is_fast = True

        def __call__(self, text, add_special_tokens=False, return_offsets_mapping=False):
            assert return_offsets_mapping and not add_special_tokens
            out, i = [], 0
            for part in text.split(" "):
                out.append((max(0, i - 1), i + len(part)) if i else (0, len(part)))
                i += len(part) + 1
            return {"input_ids": list(range(len(out))), "offset_mapping": out}

    class Wrapper:
        tok, bos_id, eos_id = FastTok(), 1, 2

    assert A.token_spans(Wrapper(), "ab cd") == [(0, 0), (0, 2), (2, 5), (5, 5)]
    cues = A.word_cues("ab cd", A.token_spans(Wrapper(), "ab cd"), [(0, 1), (1, 3), (3, 4), (4, 6)])
    assert [(c.text, c.start_sample // 1920, c.end_sample // 1920) for c in cues] == [("ab", 1, 3), ("cd", 3, 4)]

    class Bare:
        def encode(self, text):
            return [1, 2]

    with pytest.raises(TypeError, match="token_spans="):
        A.token_spans(Bare(), "ab")


def test_map_speed_is_the_stretch_arithmetic():
    for speed in (0.5, 0.8, 1.0, 1.25, 2.0):
        step = hip.tsm_step(speed)
        for n in (0, 1, 1919, 1920, 48000, 123457):
            assert A.map_speed(n, step) == hip.tsm_out_len(n, step) == (n * 480 * 65536) // step
    assert A.map_speed(48000, hip.tsm_step(1.0)) == 48000
    assert (A.TSM_HS, A.TSM_R, A.HOP) == (hip.TSM_HS, hip.TSM_R, 1920)
    cue = A.WordCue("x", 0, 1, 1920, 3840)
    assert A.stretch_cues([cue], hip.tsm_step(2.0)) == [A.WordCue("x", 0, 1, 960, 1920)]
    # into a joined waveform: clamped to the kept range of the segment, then shifted
    assert A.long_cue(cue, 3, 1000, 2000, 3000) == A.LongWordCue("x", 0, 1, 1000, 2000, 3)
    assert A.long_cue(cue, 0, 0, 0, 9999) == A.LongWordCue("x", 0, 1, 1920, 3840, 0)


def test_timing_keywords_are_refused_where_there_is_no_timing():
    A.refuse_timing({}, "stream")
    kw = {"alignment": None, "word_cues": False, "chunk_frames": 6}
    A.refuse_timing(kw, "stream")
    assert kw == {"chunk_frames": 6}
    for bad in ({"alignment": []}, {"word_cues": True}, {"align_heads": [(1, 0)]}, {"token_spans": [(0, 1)]}):
        with pytest.raises(NotImplementedError, match="no word timing"):
            A.refuse_timing(dict(bad), "stream_batch")
