"""Aggregate throughput of batched streaming (SoproTTS.stream_batch) against sequential single streams (stream()).

At chunk_frames 6 and 200-frame utterances (EOS-suppressed synthetic checkpoint, default sampling: every row runs the whole budget), for
B in {1, 8, 32}: first-chunk latency p50, per-step wall time split into AR / refine / decode, and audio seconds per wall second
against B sequential stream() calls.  Writes one JSON document (default profiles/stream_batch.json).

    python tools/stream_batch_probe.py [--out profiles/stream_batch.json] [--batches 1,8,32] [--frames 200]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


HOW = ("host wall time; step_ms_ar = waiting for a step's tokens (the next chunk's AR frames are issued before the current chunk is "
       "refined and decoded, so they mostly overlap), step_ms_refine / step_ms_decode = the batched refinement and stream decode; "
       "single = sequential stream() calls of the same shape, x_single = audio_s_per_s / single")


class _Tok:
    vocab_size = 512

    def encode(self, text):
        return [1 + (ord(c) % 500) for c in text]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/stream_batch.json")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--cf", type=int, default=6)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    from sopro_amd import SoproTTS
    from sopro_amd.config import MimiDecoderConfig, SoproTTSConfig
    from sopro_amd.weights import synth_mimi_weights, synth_sopro_weights

    cfg, mc = SoproTTSConfig(), MimiDecoderConfig()
    tts = SoproTTS.from_weights(cfg, synth_sopro_weights(cfg, 512, 1234, suppress_eos=True), synth_mimi_weights(mc, 7), _Tok(), device="cuda:0")
    rng = np.random.default_rng(3)
    maxf, cf = int(a.frames) - 1, int(a.cf)  # (max_frames + 1 frames per utterance)
    bs = [int(x) for x in a.batches.split(",")]
    n_rows = max(bs)
    ids = [torch.from_numpy(rng.integers(1, 512, size=int(rng.integers(30, 90)))) for _ in range(n_rows)]
    refs = [tts.prepare_reference(ref_tokens_tq=torch.from_numpy(rng.integers(0, 2048, size=(150, 32)))) for _ in range(n_rows)]
    kw = dict(max_frames=maxf, chunk_frames=cf, style_strength=1.0)
    sr = 24000.0

    def single(b, seed):
        t0 = time.perf_counter()
        first, n = None, 0
        for c in tts.stream("", text_ids=ids[b], ref=refs[b], seed=seed, **kw):
            torch.cuda.synchronize()
            if first is None:
                first = time.perf_counter() - t0
            n += int(c.shape[1])
        return time.perf_counter() - t0, first, n

    def batched(B, seed):
        tm = {}
        t0 = time.perf_counter()
        first, n, steps = None, 0, 0
        for step in tts.stream_batch([""] * B, refs[:B], text_ids=ids[:B], seeds=[seed + b for b in range(B)], timings=tm, **kw):
            torch.cuda.synchronize()
            if first is None:
                first = time.perf_counter() - t0
            steps += 1
            n += sum(int(c.shape[1]) for c in step if c is not None)
        return time.perf_counter() - t0, first, n, steps, tm

    single(0, 1)  # warm-up: recorded graphs, scratch
    for B in bs:
        batched(B, 1)
    res = {"chunk_frames": cf, "frames_per_utterance": maxf + 1, "device": torch.cuda.get_device_name(0), "rows": [],
           "how": HOW}
    # the single-stream rate: B sequential stream() calls
    s_walls, s_firsts, s_samples = [], [], 0
    for r in range(a.reps):
        for b in range(min(4, n_rows)):
            w, f, n = single(b, 100 + r)
            s_walls.append(w)
            s_firsts.append(f)
            s_samples += n
    single_rate = s_samples / sr / sum(s_walls)
    res["single"] = {"audio_s_per_s": round(single_rate, 2), "first_chunk_ms_p50": round(1e3 * float(np.median(s_firsts)), 2),
                     "wall_ms_per_utterance": round(1e3 * float(np.mean(s_walls)), 1)}
    for B in bs:
        walls, firsts, samples, steps_all, tms = [], [], 0, 0, {"ar": 0.0, "refine": 0.0, "decode": 0.0}
        for r in range(a.reps):
            w, f, n, steps, tm = batched(B, 1000 * r)
            walls.append(w)
            firsts.append(f)
            samples += n
            steps_all += steps
            for k in tms:
                tms[k] += tm[k]
        rate = samples / sr / sum(walls)
        res["rows"].append({"B": B, "audio_s_per_s": round(rate, 2), "x_single": round(rate / single_rate, 2),
                            "first_chunk_ms_p50": round(1e3 * float(np.median(firsts)), 2),
                            "step_ms": round(1e3 * sum(walls) / steps_all, 3),
                            "step_ms_ar": round(1e3 * tms["ar"] / steps_all, 3), "step_ms_refine": round(1e3 * tms["refine"] / steps_all, 3),
                            "step_ms_decode": round(1e3 * tms["decode"] / steps_all, 3)})
        print(json.dumps(res["rows"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
