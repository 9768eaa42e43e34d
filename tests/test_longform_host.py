"""Long-form synthesis, host side (no device): text segmentation, pauses, group plans, the join's C entry points refusing bad
arguments, and the numpy restatement of the join (tests/longform_ref.py, the GPU tests' yardstick) against hand-computed cases."""
import ctypes
import random

import numpy as np
import pytest

import longform_ref as R
from sopro_amd import hip
from sopro_amd.longform import BOUNDARIES, DEFAULT_PAUSES_MS, Segment, group_plan, join_params, pause_samples, split_text


def _normalised(text):
    return " ".join(text.split())


def _rebuild(segs):
    return "".join(s.text + ("" if s.boundary in ("hard", "end") else " ") for s in segs)


def _check_invariants(text, segs, max_chars):
    assert _rebuild(segs) == _normalised(text), (text, segs)
    for i, s in enumerate(segs):
        assert isinstance(s, Segment) and s.text and len(s.text) <= max_chars, (text, s)
        assert s.text == s.text.strip()
        assert s.boundary in BOUNDARIES
        assert (s.boundary == "end") == (i == len(segs) - 1), (text, segs)


LONG_WITH_COMMAS = ", ".join(["the quick brown fox jumps over the lazy dog"] * 16) + "."   # ~ 720 characters, one sentence
LONG_NO_COMMAS = " ".join(["the quick brown fox jumps over the lazy dog"] * 16) + "."
LONG_WORD = "x" * 400

CORPUS = [
    "Hello there. How are you? Fine!",
    "Dr. Smith met Mr. Jones and Mrs. Brown vs. Prof. Plum at St. Mary's, No. 5, etc. and so on. Then they left.",
    "It works, e.g. here and i.e. there. Ms. Green agrees.",
    "J. R. R. Tolkien wrote it. J. K. Rowling did not. The U.S. fleet sailed.",
    "She said \"Stop.\" He did not. (Really?) Yes! 'Truly.' Fine.",
    "Wait... what? Well… fine. No?! Yes!!",
    "Pi is 3.14 and e is 2.718. The price was 3,000 at 12:30. Done.",
    LONG_WITH_COMMAS,
    LONG_NO_COMMAS,
    LONG_WORD,
    "Short. " + LONG_WORD + " tail words here. End.",
    "First paragraph. Still first.\n\nSecond paragraph here.\n \t \n\n Third one without a stop",
    "Windows text.\r\nSame paragraph.\r\n\r\nNext paragraph.\r\n",
    "   leading and trailing   blanks .  ",
    "no terminator at all",
]


@pytest.mark.parametrize("max_chars", [280, 60, 12])
def test_split_text_invariants_on_the_corpus(max_chars):
    for text in CORPUS:
        _check_invariants(text, split_text(text, max_chars=max_chars), max_chars)


def test_split_text_empty_and_blank():
    assert split_text("") == [] and split_text(" \n\t \r\n ") == []
    with pytest.raises(ValueError):
        split_text("a", max_chars=0)


def test_split_text_sentences_abbreviations_initials_quotes():
    t = lambda text, **kw: [tuple(s) for s in split_text(text, **kw)]  # noqa: E731
    assert t("Hello there. How are you? Fine!") == [("Hello there.", "sentence"), ("How are you?", "sentence"), ("Fine!", "end")]
    assert t(CORPUS[1]) == [("Dr. Smith met Mr. Jones and Mrs. Brown vs. Prof. Plum at St. Mary's, No. 5, etc. and so on.", "sentence"),
                            ("Then they left.", "end")]
    assert t(CORPUS[2]) == [("It works, e.g. here and i.e. there.", "sentence"), ("Ms. Green agrees.", "end")]
    assert [s for s, _ in t(CORPUS[3])] == ["J. R. R. Tolkien wrote it.", "J. K. Rowling did not.", "The U.S. fleet sailed."]
    assert [s for s, _ in t(CORPUS[4])] == ["She said \"Stop.\"", "He did not.", "(Really?)", "Yes!", "'Truly.'", "Fine."]
    assert [s for s, _ in t(CORPUS[5])] == ["Wait...", "what?", "Well…", "fine.", "No?!", "Yes!!"]
    assert [s for s, _ in t(CORPUS[6])] == ["Pi is 3.14 and e is 2.718.", "The price was 3,000 at 12:30.", "Done."]
    assert t("mr. lower case is not in the list. Next.")[0] == ("mr.", "sentence")  # the list is case-sensitive as written


def test_split_text_paragraphs_and_newlines():
    segs = split_text(CORPUS[11])
    assert [tuple(s) for s in segs] == [("First paragraph.", "sentence"), ("Still first.", "paragraph"), ("Second paragraph here.", "paragraph"),
                                        ("Third one without a stop", "end")]
    assert [tuple(s) for s in split_text(CORPUS[12])] == [("Windows text.", "sentence"), ("Same paragraph.", "paragraph"), ("Next paragraph.", "end")]
    assert [tuple(s) for s in split_text("one line\nsame paragraph")] == [("one line same paragraph", "end")]


def test_split_text_long_sentences():
    segs = split_text(LONG_WITH_COMMAS)
    assert len(segs) == 3 and [s.boundary for s in segs] == ["clause", "clause", "end"]
    assert all(s.text.endswith(",") for s in segs[:-1])
    # the cut is the LAST clause mark at or below the limit: the next clause would not have fitted
    nxt = LONG_WITH_COMMAS[len(segs[0].text) + 1:]
    assert len(segs[0].text) + 1 + nxt.index(",") + 1 > 280
    segs = split_text(LONG_NO_COMMAS)
    assert [s.boundary for s in segs] == ["space", "space", "end"]
    assert len(segs[0].text) + 1 + len(segs[1].text.split(" ")[0]) > 280  # the next word would not have fitted
    segs = split_text(LONG_WORD)
    assert [tuple(s) for s in segs] == [("x" * 280, "hard"), ("x" * 120, "end")]
    segs = split_text("ab, cd ef", max_chars=4)
    assert [tuple(s) for s in segs] == [("ab,", "clause"), ("cd", "space"), ("ef", "end")]
    assert [tuple(s) for s in split_text("3,000,000 9", max_chars=5)] == [("3,000", "hard"), (",000", "space"), ("9", "end")]  # no blank after the commas


def test_split_text_random_texts():
    rng = random.Random(20240607)
    words = ["a", "the", "Dr.", "e.g.", "cat", "3.14", "J.", "hello", "Mr.", "q" * 50, "No.", "end", "—", "it's"]
    marks = [".", "!", "?", "…", ",", ";", ":", " —", ".\"", "...", "?!", ".)", ""]
    blanks = [" ", " ", " ", "  ", "\n", "\n\n", "\r\n\r\n", "\t", " \n \n ", ""]
    for _ in range(200):
        text = "".join(rng.choice(words) + rng.choice(marks) + rng.choice(blanks) for _ in range(rng.randint(0, 60)))
        mc = rng.choice([8, 25, 60, 280])
        _check_invariants(text, split_text(text, max_chars=mc), mc)


def test_pause_samples():
    assert DEFAULT_PAUSES_MS == {"paragraph": 600, "sentence": 250, "clause": 120, "space": 60, "hard": 0, "end": 0}
    assert [pause_samples(b) for b in ("paragraph", "sentence", "clause", "space", "hard", "end")] == [14400, 6000, 2880, 1440, 0, 0]
    assert pause_samples("sentence", {"sentence": 100}) == 2400 and pause_samples("clause", {"sentence": 100}) == 2880
    with pytest.raises(ValueError):
        pause_samples("comma")
    with pytest.raises(ValueError):
        pause_samples("space", {"space": -1})


def test_group_plan():
    for n in range(0, 101):
        for plan in ("throughput", "latency"):
            for max_rows in (32, 5, 1):
                g = group_plan(n, plan, max_rows)
                assert sum(g) == n and all(1 <= v <= max_rows for v in g), (n, plan, max_rows, g)
    assert group_plan(0, "latency") == [] and group_plan(0, "throughput") == []
    assert group_plan(100, "throughput") == [32, 32, 32, 4]
    assert group_plan(100, "latency") == [1, 2, 4, 8, 16, 32, 32, 5]
    assert group_plan(7, "latency") == [1, 2, 4] and group_plan(8, "latency") == [1, 2, 4, 1]
    assert group_plan(20, "latency", max_rows=6) == [1, 2, 4, 6, 6, 1]
    assert group_plan(6, [1, 5]) == [1, 5]
    for bad in ([1, 4], [6, 0], [7, -1]):
        with pytest.raises(ValueError):
            group_plan(6, bad)
    with pytest.raises(ValueError):
        group_plan(6, "fastest")


def test_join_params():
    p = join_params(-40.0, 30.0, 5.0)
    assert p == dict(hop=240, rel=float(np.float32(0.01)), keep=3, fade_len=120, trim=True)
    assert join_params(None, 30.0, 0.0)["trim"] is False and join_params(None, 30.0, 0.0)["fade_len"] == 0


def test_join_entry_points_refuse_bad_arguments_without_a_device():
    lib = hip.load()
    buf = (ctypes.c_int64 * 64)()  # a host address that must never be touched: every refusal comes before the first launch
    p = ctypes.addressof(buf)
    assert lib.sopro_join_workspace_bytes(7, 96000, 240) == 7 * 400 * 4
    assert lib.sopro_join_workspace_bytes(64, 1, 240) == 64 * 4 and lib.sopro_join_workspace_bytes(2, 0, 240) == 2 * 4
    assert lib.sopro_join_workspace_bytes(0, 96000, 240) == 0 and lib.sopro_join_workspace_bytes(7, 96000, 0) == 0
    edges = lambda **kw: lib.sopro_join_edges_f32(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("wav", p), ("row_stride", 1000), ("lens", p), ("n_seg", 2), ("max_len", 1000), ("hop", 240), ("rel", 0.01), ("keep", 3), ("trim", 1),
        ("ws", p), ("edges", p), ("stream", None))])
    for kw, msg in ((dict(wav=None), b"non-NULL"), (dict(lens=None), b"non-NULL"), (dict(edges=None), b"non-NULL"), (dict(ws=None), b"workspace"),
                    (dict(n_seg=0), b"n_seg"), (dict(n_seg=-3), b"n_seg"), (dict(hop=0), b"hop"), (dict(hop=-240), b"hop"),
                    (dict(row_stride=-1), b"row_stride"), (dict(max_len=-1), b"max_len"), (dict(keep=-1), b"keep")):
        assert edges(**kw) == -2, kw
        assert b"sopro_join_edges_f32" in lib.sopro_last_error() and msg in lib.sopro_last_error(), (kw, lib.sopro_last_error())
    for args in ((None, p, 2, p, None), (p, None, 2, p, None), (p, p, 2, None, None), (p, p, 0, p, None)):
        assert lib.sopro_join_layout_i64(*args) == -2
        assert b"sopro_join_layout_i64" in lib.sopro_last_error()
    mix = lambda **kw: lib.sopro_join_mix_f32(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("wav", p), ("row_stride", 1000), ("edges", p), ("offs", p), ("tab", p), ("fade_len", 120), ("n_seg", 2), ("out", p), ("out_cap", 100),
        ("stream", None))])
    for kw, msg in ((dict(wav=None), b"non-NULL"), (dict(edges=None), b"non-NULL"), (dict(offs=None), b"non-NULL"), (dict(out=None), b"non-NULL"),
                    (dict(tab=None), b"tab"), (dict(fade_len=-1), b"fade_len"), (dict(n_seg=0), b"n_seg"), (dict(row_stride=-5), b"row_stride"),
                    (dict(out_cap=-1), b"out_cap")):
        assert mix(**kw) == -2, kw
        assert b"sopro_join_mix_f32" in lib.sopro_last_error() and msg in lib.sopro_last_error(), (kw, lib.sopro_last_error())


def test_join_wrapper_refuses_host_tensors():
    import torch

    with pytest.raises(hip.SoproHipError, match="no CPU fallback"):
        hip.join_segments(torch.zeros(2, 8), [8, 8], [0, 0])


def test_submit_long_is_a_batch_mode_entry_point():
    from sopro_amd.serving import SynthesisService

    svc = SynthesisService.__new__(SynthesisService)  # (no device here: only the mode check is exercised)
    svc._closed, svc.engine = False, object()
    with pytest.raises(RuntimeError, match="continuous"):
        svc.submit_long("Some text.", None)
    svc._closed = True
    with pytest.raises(RuntimeError, match="closed"):
        svc.submit_long("Some text.", None)


# ------------------------------------------------------------------------------------------ the yardstick itself
def test_fade_table_values():
    t = R.fade_table(2)
    assert t.dtype == np.float32 and np.array_equal(t, np.array([0.5 - 0.5 * np.cos(np.pi / 4), 0.5 + 0.5 * np.cos(np.pi / 4)]).astype(np.float32))
    assert abs(float(t[0]) - 0.14644661) < 1e-7 and abs(float(t[1]) - 0.85355339) < 1e-7
    t = R.fade_table(120)
    assert t.shape == (120,) and np.all(np.diff(t) > 0) and 0 < t[0] < 1e-4 and 1 - 1e-4 < t[-1] < 1
    assert np.array_equal(hip.fade_table(120, "cpu").numpy(), t) and hip.fade_table(0, "cpu") is None


def test_restatement_case_1_edges_with_and_without_keep():
    x = np.zeros(20, np.float32)
    x[8] = 1.0  # hop 2 of five 4-sample hops
    assert R.row_edges(x, 20, hop=4, rel=0.5, keep=0) == (8, 12)
    assert R.row_edges(x, 20, hop=4, rel=0.5, keep=1) == (4, 16)
    assert R.row_edges(x, 20, hop=4, rel=0.5, keep=3) == (0, 20)   # clamped on both sides
    assert R.row_edges(x, 20, hop=4, rel=0.5, keep=0, trim=False) == (0, 20)


def test_restatement_case_2_empty_and_silent_rows():
    x = np.zeros(16, np.float32)
    assert R.row_edges(x, 0, hop=4) == (0, 0) and R.row_edges(x, 16, hop=4) == (0, 0)
    assert R.row_edges(x, 16, hop=4, trim=False) == (0, 16)  # no trimming looks at nothing
    x[3] = -2.0
    assert R.row_edges(x, 3, hop=4, keep=0) == (0, 0)         # the sample past the length is never looked at
    assert R.row_edges(x, 4, hop=4, keep=0) == (0, 4)


def test_restatement_case_3_threshold_is_inclusive_and_relative():
    x = np.zeros(16, np.float32)
    x[1], x[6], x[9], x[14] = 0.25, -1.0, 0.5, 0.49
    assert R.row_edges(x, 16, hop=4, rel=0.5, keep=0) == (4, 12)    # 0.5 >= 0.5 * 1.0 is active, 0.25 and 0.49 are not
    assert R.row_edges(x, 16, hop=4, rel=0.25, keep=0) == (0, 16)
    assert R.row_edges(x * 8, 16, hop=4, rel=0.5, keep=0) == (4, 12)  # relative to the row's own peak


def test_restatement_case_4_ragged_last_hop():
    x = np.zeros(10, np.float32)
    x[9] = 0.125  # hops [0, 4) [4, 8) [8, 10)
    assert R.row_edges(x, 10, hop=4, keep=0) == (8, 10)
    assert R.row_edges(x, 10, hop=4, keep=1) == (4, 10)
    assert R.row_edges(x, 10, hop=240, keep=3) == (0, 10)  # a row shorter than a hop


def test_restatement_case_5_layout_skips_empty_rows_and_their_gaps():
    wav = np.array([[1, 2, 3, 9], [9, 9, 9, 9], [4, 5, 9, 9]], np.float32)
    out, edges, offs = R.join(wav, [3, 0, 2], [5, 7, 9], trim=False, fade_len=0)
    assert edges.tolist() == [[0, 3], [0, 0], [0, 2]] and offs.tolist() == [0, 8, 8, 19]
    assert out.tolist() == [1, 2, 3, 0, 0, 0, 0, 0, 4, 5] + [0] * 9 and out.dtype == np.float32
    out, edges, offs = R.join(np.array([[0, 0, 7, 0, 0, 0, 0, 0]], np.float32), [8], [2], hop=2, rel=0.5, keep=1, fade_len=0)
    assert edges.tolist() == [[0, 6]] and offs.tolist() == [0, 8] and out.tolist() == [0, 0, 7, 0, 0, 0, 0, 0]


def test_restatement_case_6_fades():
    t0, t1 = (float(v) for v in R.fade_table(2))
    ones = np.ones((3, 5), np.float32)
    out, edges, offs = R.join(ones, [5, 3, 1], [1, 0, 0], trim=False, fade_len=2)
    assert offs.tolist() == [0, 6, 9, 10]
    t0h = float(np.float32(R.fade_table(1)[0]))  # fade_len 2 on 3 samples uses F = 1: tab[0] of the SAME table
    assert t0h == 0.5
    assert out.tolist() == [t0, t1, 1.0, t1, t0, 0.0, t0, 1.0, t0, 1.0]
    x = np.array([[3.0, -5.0, 7.0, 11.0]], np.float32)
    out, _, _ = R.join(x, [4], [0], trim=False, fade_len=1)
    assert out.tolist() == [1.5, -5.0, 7.0, 5.5]


def test_restatement_on_the_designed_batch():
    for seed in (0, 1):
        wav, lens, gaps = R.designed_batch(seed)
        out, edges, offs = R.join(wav, lens, gaps)
        assert edges.tolist() == [[11280, 79920], [0, 0], [0, 100], [0, 71047], [95040, 95999], [0, 0], [960, 2880]]
        assert edges.tolist() == R.DESIGNED_EDGES
        assert int(offs[-1]) == 157546 == R.DESIGNED_TOTAL and out.shape == (157546,)
        assert not np.any(out == 777.0)
        assert out[68640: 68640 + 6000].tolist() == [0.0] * 6000  # the pause after row 0
