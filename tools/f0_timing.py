"""Cost of the pitch tracker beside the decode whose output it reads.

One process, synthetic codec checkpoint, random token batches.  For 32 x 200 frames and 1 x 400 frames: ``codec.decode_batch`` of the
token batch (the yardstick: what produces the rows), then ``hip.f0_track`` of the decoded batch at the default parameters.  Warm-up,
then device events around every call, median of ``--reps``.  Writes a markdown table (default profiles/f0_timing.md) with the command
line.  There is no pass mark.

    python tools/f0_timing.py [--out profiles/f0_timing.md] [--reps 20] [--warmup 3]
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
    ap.add_argument("--out", default="profiles/f0_timing.md")
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
    lines = ["# Pitch tracker: time beside the decode whose output it reads", "",
             f"Command: `python tools/f0_timing.py --reps {a.reps} --warmup {a.warmup}` on {torch.cuda.get_device_name(0)}; device events,",
             f"median (min .. max) of {a.reps} after {a.warmup} warm-up calls, one process.  `decode` is `codec.decode_batch` of the token batch,",
             "`track` is `hip.f0_track` of its output at the default parameters (three launches: the front end with the candidate pick, the",
             "path, the output; the allocation of the workspace and of the three result tensors is inside the span).  `terms` counts the",
             "difference-squares of the definition, 400 lags x 720 samples per frame; the kernel forms each block's share once, a third",
             "of that.  No pass mark.", "",
             "| batch | pitch frames per row | voiced | decode ms | track ms | track / decode | us per pitch frame | definition Gterms / s |",
             "|---|---|---|---|---|---|---|---|"]
    for B, T in ((32, 200), (1, 400)):
        toks = torch.from_numpy(rng.integers(0, 2048, size=(B, T, int(mc.num_quantizers)))).to("cuda:0")
        with torch.cuda.stream(codec.stream):
            dec = timed(lambda: codec.decode_batch(toks), a.warmup, a.reps)
        wav = codec.decode_batch(toks)
        n = int(wav.shape[1])
        frames = (n - hip.F0_SPAN) // hip.F0_H + 1
        st = timed(lambda: hip.f0_track(wav, [n] * B), a.warmup, a.reps)
        nv = int(hip.f0_track(wav, [n] * B)[2].sum())
        terms = B * frames * hip.F0_TMAX * hip.F0_W
        lines.append(f"| {B} x {T} | {frames} | {nv / (B * frames):.3f} | {dec[0]:.3f} ({dec[1]:.3f} .. {dec[2]:.3f}) | {st[0]:.3f} ({st[1]:.3f} .. {st[2]:.3f}) | "
                     f"{st[0] / dec[0]:.3f} | {1e3 * st[0] / (B * frames):.3f} | {terms / st[0] / 1e6:.1f} |")
        print(lines[-1], flush=True)
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
