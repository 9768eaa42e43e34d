"""Cost of the formant operator beside the decode it follows.

One process, synthetic codec checkpoint, random token batches.  For 32 x 200 frames and 1 x 400 frames: ``codec.decode_batch`` of the
token batch (the yardstick: what produces the rows), then ``hip.formant_shift`` of the decoded batch at sigma 0.5 / 2^(3/12) / 2.0.
Warm-up, then device events around every call, median of ``--reps``.  Writes a markdown table (default profiles/formant_timing.md)
with the command line.  There is no pass mark.

    python tools/formant_timing.py [--out profiles/formant_timing.md] [--reps 20] [--warmup 3]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup: int, reps: int):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/formant_timing.md")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from sopro_amd import hip
    from sopro_amd.codec import MimiCodec
    from sopro_amd.config import MimiDecoderConfig
    from sopro_amd.weights import synth_mimi_weights

    mc = MimiDecoderConfig()
    codec = MimiCodec(synth_mimi_weights(mc, 1234), mc, "cuda:0")
    rng = np.random.default_rng(5)
    lines = ["# Formant operator: time beside the decode it follows", "",
             f"Command: `python tools/formant_timing.py --reps {a.reps} --warmup {a.warmup}` on {torch.cuda.get_device_name(0)}; device events,",
             f"median (min .. max) of {a.reps} after {a.warmup} warm-up calls, one process.  `decode` is `codec.decode_batch` of the token batch,",
             "`warp` is `hip.formant_shift` of its output (two launches: one wave per frame, then the overlap-add; the workspace allocation of",
             "the call is inside the span).  No pass mark.", "",
             "| batch | sigma | frames per row | decode ms | warp ms | warp / decode | us per frame |", "|---|---|---|---|---|---|---|"]
    for B, T in ((32, 200), (1, 400)):
        toks = torch.from_numpy(rng.integers(0, 2048, size=(B, T, int(mc.num_quantizers)))).to("cuda:0")
        with torch.cuda.stream(codec.stream):
            dec = timed(lambda: codec.decode_batch(toks), a.warmup, a.reps)
        wav = codec.decode_batch(toks)
        n = int(wav.shape[1])
        frames = -(-n // hip.FM_H) + 3
        out = torch.empty(B, n, device="cuda:0")
        for sigma in (0.5, 2.0 ** 0.25, 2.0):
            inv = hip.formant_inv(12.0 * float(np.log2(sigma)))
            st = timed(lambda: hip.formant_shift(wav, [n] * B, [inv] * B, out=out), a.warmup, a.reps)
            lines.append(f"| {B} x {T} | {sigma:.4f} | {frames} | {dec[0]:.3f} ({dec[1]:.3f} .. {dec[2]:.3f}) | {st[0]:.3f} ({st[1]:.3f} .. {st[2]:.3f}) | "
                         f"{st[0] / dec[0]:.3f} | {1e3 * st[0] / (B * frames):.3f} |")
            print(lines[-1], flush=True)
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
