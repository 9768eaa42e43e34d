"""Cost of the reference crop selection on one long recording, beside the resampler call on the same row.

One process.  The row is ``--minutes`` of 16 kHz material (the synthetic voice in stretches, pauses and faint noise between them);
``MimiCodec.resample`` takes it to 24 kHz, ``hip.speech_crop`` picks the 12 s window of the result.  Warm-up, then timed calls, median
(min .. max) of ``--reps``, host clock around each call and a device synchronise; a repeat of each figure at the end brackets the spread inside the process.
The report and the window are compared with the numpy restatement before anything is timed, and the outcome is written down.

    python tools/crop_timing.py [--out profiles/crop_timing.md] [--minutes 10] [--reps 30] [--warmup 5] [--label TEXT]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1234
SR_IN, SR = 16000, 24000
WIN = 150 * 1920  # 12 s at 12.5 frames per second


def timed_host(fn, warmup: int, reps: int):
    """Host clock around a call that ends in a device synchronise (the resampler runs on the codec's own stream and synchronises it
    itself, so events on the current stream would not see it; both calls are timed the same way)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def fmt(t) -> str:
    return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/crop_timing.md")
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import crop_ref as R
    from sopro_amd import SpeechCrop, hip
    from sopro_amd.codec import MimiCodec
    from sopro_amd.config import MimiDecoderConfig
    from sopro_amd.weights import synth_mimi_weights

    n_in = int(a.minutes * 60 * SR_IN)
    rng = np.random.default_rng(SEED)
    spans, t = [], 0
    while t < n_in:  # 0.4 .. 2.5 s of voice, 0.2 .. 3 s of pause
        on, off = int(rng.uniform(0.4, 2.5) * SR_IN), int(rng.uniform(0.2, 3.0) * SR_IN)
        spans.append((t, min(n_in, t + on)))
        t += on + off
    x16 = R.clip_of(n_in, spans, seed=SEED, noise=1e-3, sr=SR_IN).astype(np.float32)
    mc = MimiDecoderConfig()
    codec = MimiCodec(synth_mimi_weights(mc, SEED, with_encoder=True), mc, "cuda:0")
    d16 = torch.from_numpy(x16).cuda()
    x24 = codec.resample(d16, SR_IN, SR).contiguous()
    n = int(x24.numel())
    row = x24.reshape(1, -1)
    out = torch.empty(1, WIN, dtype=torch.float32, device="cuda:0")
    got, lens, reps = hip.speech_crop(row, [n], SpeechCrop(), WIN, out=out, report=True)
    p = R.crop_parts(x24.cpu().numpy(), WIN)
    agree = tuple(reps[0][:7]) == tuple(p.report[:7]) and torch.equal(got[0], x24[p.start: p.start + WIN])
    F = p.F
    t_crop = timed_host(lambda: hip.speech_crop(row, [n], SpeechCrop(), WIN, out=out), a.warmup, a.reps)
    t_res = timed_host(lambda: codec.resample(d16, SR_IN, SR), a.warmup, a.reps)
    t_crop2 = timed_host(lambda: hip.speech_crop(row, [n], SpeechCrop(), WIN, out=out), a.warmup, a.reps)
    t_res2 = timed_host(lambda: codec.resample(d16, SR_IN, SR), a.warmup, a.reps)
    read_mb = n * 4 / 1e6
    lines = ["# Reference crop selection: time of the operator on one long recording, beside the resampler on the same row", "",
             f"Command: `python tools/crop_timing.py --minutes {a.minutes:g} --reps {a.reps} --warmup {a.warmup}`{' (' + a.label + ')' if a.label else ''} on "
             f"{torch.cuda.get_device_name(0)}; median (min .. max) of {a.reps} after {a.warmup} warm-up calls, host clock around one call and a device synchronise, one "
             "process, each figure taken twice.  These are records, not bars: no test asserts a time.", "",
             f"The row: {a.minutes:g} min at 16 kHz ({n_in} samples) -> {n} samples at 24 kHz, {F} blocks of 10 ms, window {WIN} samples (12 s, "
             f"{WIN // R.H} blocks), {F - WIN // R.H + 1} candidates.  The search chose start {reps[0].start} ({reps[0].active} speech blocks against "
             f"{reps[0].centre_active} in the centre crop at {(n - WIN) // 2}); the numpy restatement {'gives the same report and window' if agree else 'DISAGREES: ' + repr(p.report)}.", "",
             "| what | ms | again | note |", "|---|---|---|---|",
             f"| `hip.speech_crop` (blocks, pick, gather: 3 launches) | {fmt(t_crop)} | {fmt(t_crop2)} | reads the row once ({read_mb:.1f} MB): "
             f"{read_mb / 1e3 / (t_crop[0] * 1e-3):.0f} GB/s over the whole call; includes the workspace and starts allocations of the wrapper |",
             f"| `MimiCodec.resample` 16 -> 24 kHz of the same recording | {fmt(t_res)} | {fmt(t_res2)} | the step before it in `reference_waveform` |",
             ""]
    for ln in lines:
        print(ln, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
