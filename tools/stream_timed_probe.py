"""What do streamed word cues cost?  ``stream_timed`` beside ``stream`` on the synthetic checkpoint: per-item wall time and time to
the first audio, the same seed and text, the two alternating in one process (profiles/stream_timed_overhead.md is this tool's output).

    python tools/stream_timed_probe.py [--frames 200] [--chunk 6] [--lag 8] [--runs 7] [--text-len 64]
    python tools/stream_timed_probe.py --only-stream --root OTHER_CHECKOUT      # stream() of another (built) commit, the same way

Every item is timed on the host after a device synchronise, so an item's time is the time a consumer waits for it.  One run of each
kind warms every shape up and is not counted."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout to import sopro_amd from (another commit's, built, with --only-stream: stream() there)")
    ap.add_argument("--only-stream", action="store_true", help="time stream() alone (a checkout without stream_timed)")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--chunk", type=int, default=6)
    ap.add_argument("--lag", type=int, default=8)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--text-len", type=int, default=64)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from sopro_amd import SoproTTS
    from sopro_amd.config import MimiDecoderConfig, SoproTTSConfig
    from sopro_amd.weights import synth_mimi_weights, synth_sopro_weights

    class Tok:
        vocab_size = 512

        def encode(self, text):
            return [1 + (ord(c) % 500) for c in text]

    cfg, mc = SoproTTSConfig(), MimiDecoderConfig()
    tts = SoproTTS.from_weights(cfg, synth_sopro_weights(cfg, 512, 1234, suppress_eos=True), synth_mimi_weights(mc, 1234), Tok(), device="cuda:0")
    ref = tts.prepare_reference(ref_tokens_tq=torch.from_numpy(np.random.default_rng(5).integers(0, 2048, size=(24, 32))))
    words = "some words of several lengths to speak aloud in one streamed take".split()
    text = " ".join(words[i % len(words)] for i in range(a.text_len))[: a.text_len]
    spans = [(i, i + 1) for i in range(len(text))]
    kw = dict(ref=ref, max_frames=a.frames - 1, seed=3, chunk_frames=a.chunk, top_p=0.0, temperature=1.0, anti_loop=False)

    def run(timed: bool):
        """-> (seconds to the first audio, [seconds per item], samples, cues, seconds in all)"""
        torch.cuda.synchronize()
        t_start = t_prev = time.perf_counter()
        first, per, n, cues = None, [], 0, 0
        it = tts.stream_timed(text, token_spans=spans, lag_frames=a.lag, **kw) if timed else tts.stream(text, **kw)
        for item in it:
            wav = item.wav if timed else item
            torch.cuda.synchronize()
            now = time.perf_counter()
            if first is None and wav.numel() > 0:
                first = now - t_start
            elif first is not None and not (timed and item.final):  # (the closing item carries no chunk: it counts in the whole take)
                per.append(now - t_prev)
            t_prev = now
            n += int(wav.shape[-1])
            cues += len(item.words) if timed else 0
        return first, per, n, cues, t_prev - t_start

    ms = lambda v: 1e3 * v  # noqa: E731
    if a.only_stream:
        run(False)
        got = [run(False) for _ in range(a.runs)]
        firsts, per, totals = [r[0] for r in got], [v for r in got for v in r[1]], [r[4] for r in got]
        print(f"stream() of {os.path.abspath(a.root)}: {a.frames} frames, chunk_frames={a.chunk}, {a.runs} runs, {got[0][2]} samples")
        print(f"time to first audio {ms(statistics.median(firsts)):.2f} ms ({ms(min(firsts)):.2f} .. {ms(max(firsts)):.2f}), later items "
              f"{ms(statistics.median(per)):.2f} ms ({ms(min(per)):.2f} .. {ms(max(per)):.2f}), whole take {ms(statistics.median(totals)):.1f} ms")
        return
    run(False), run(True)  # warm-up: every shape of both
    res = {False: [], True: []}
    for _ in range(a.runs):
        for timed in (False, True):
            res[timed].append(run(timed))
    assert res[False][0][2] == res[True][0][2], "the two streams differ in length"
    print(f"# stream_timed beside stream: {a.frames} frames, chunk_frames={a.chunk}, lag_frames={a.lag}, {len(text)} text ids, {a.runs} alternating runs")
    print()
    print("| | stream | stream_timed | difference |")
    print("|---|---|---|---|")
    rows = {}
    for timed in (False, True):
        firsts = [r[0] for r in res[timed]]
        per = [v for r in res[timed] for v in r[1]]
        totals = [r[4] for r in res[timed]]
        rows[timed] = (statistics.median(firsts), min(firsts), max(firsts), statistics.median(per), min(per), max(per), statistics.median(totals))
    p, t = rows[False], rows[True]
    print(f"| time to first audio, median (min .. max), ms | {ms(p[0]):.2f} ({ms(p[1]):.2f} .. {ms(p[2]):.2f}) | {ms(t[0]):.2f} ({ms(t[1]):.2f} .. {ms(t[2]):.2f}) | {ms(t[0] - p[0]):+.2f} |")
    print(f"| later items, median (min .. max), ms | {ms(p[3]):.2f} ({ms(p[4]):.2f} .. {ms(p[5]):.2f}) | {ms(t[3]):.2f} ({ms(t[4]):.2f} .. {ms(t[5]):.2f}) | {ms(t[3] - p[3]):+.2f} |")
    print(f"| whole take, median, ms | {ms(p[6]):.1f} | {ms(t[6]):.1f} | {ms(t[6] - p[6]):+.1f} |")
    print()
    print(f"{res[True][0][2]} samples and {res[True][0][3]} cues per take; an item of {a.chunk} frames is {a.chunk * 80} ms of audio.")


if __name__ == "__main__":
    main()
