"""Cost of the silence operator beside the decode whose rows it squeezes.

One process, synthetic codec checkpoint, random tokens: ``codec.decode_batch`` of 32 x 200 frames (the yardstick: what produces the
rows) and ``hip.silence_squeeze`` of the decoded batch (32 x 384 000 samples).  The synthetic audio has no silence of its own, so the
floor is put at the 70th percentile of the batch's hop maxima (cap 4 hops, onset 2: many cuts per row, the expensive case for the
plan and the gather's search) and, for comparison, far above the peak (every row comes out empty: activity and plan only) and far
below the noise (nothing is cut: activity, plan and a plain copy).  Warm-up, then device events around every call, median of
``--reps``.  A call includes the upload of the per-row arguments and the host copy of the lengths and cuts.

    python tools/sil_timing.py [--out profiles/sil_timing.md] [--reps 20] [--warmup 5]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1234


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


def fmt(t) -> str:
    return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/sil_timing.md")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    from sopro_amd import Silence, hip
    from sopro_amd.codec import MimiCodec
    from sopro_amd.config import MimiDecoderConfig
    from sopro_amd.weights import synth_mimi_weights

    mc = MimiDecoderConfig()
    codec = MimiCodec(synth_mimi_weights(mc, SEED), mc, "cuda:0")
    rng = np.random.default_rng(5)
    B, T = 32, 200
    toks = torch.from_numpy(rng.integers(0, 2048, size=(B, T, int(mc.num_quantizers)))).to("cuda:0")
    with torch.cuda.stream(codec.stream):
        dec = timed(lambda: codec.decode_batch(toks), a.warmup, a.reps)
    wav = codec.decode_batch(toks)
    torch.cuda.synchronize()
    n = int(wav.shape[1])
    hop_max = wav.abs().reshape(B, n // hip.SIL_HOP, hip.SIL_HOP).amax(-1).flatten().float().cpu().numpy()
    peak = float(hop_max.max())
    out = torch.empty(B, n, device="cuda:0")
    cases = [("floor at the 70th percentile of the hop maxima", Silence(max_pause_ms=40.0, onset_ms=20.0, floor=float(np.percentile(hop_max, 70)))),
             ("floor above the peak: every row comes out empty", Silence(max_pause_ms=40.0, onset_ms=20.0, floor=2.0 * peak)),
             ("floor below everything: nothing is cut", Silence(max_pause_ms=40.0, onset_ms=20.0, floor=1e-6 * peak))]
    rows = []
    for what, s in cases:
        t = timed(lambda: hip.silence_squeeze(wav, [n] * B, s, out=out), a.warmup, a.reps)
        _o, lens, cuts = hip.silence_squeeze(wav, [n] * B, s, out=out)
        kept = sum(lens)
        mb = 4 * (B * n + kept) / 1e6
        rows.append(f"| squeeze, {what} | {B} x {n} | {fmt(t)} | {t[0] / dec[0]:.4f} | {sum(len(c) for c in cuts)} cuts, {kept / (B * n):.2f} of the "
                    f"samples kept, {mb:.0f} MB read + written: {mb / t[0]:.0f} GB/s |")
    lines = ["# Silence control: time beside the decode whose rows it squeezes", "",
             f"Command: `python tools/sil_timing.py --reps {a.reps} --warmup {a.warmup}` on {torch.cuda.get_device_name(0)}; device events, median",
             f"(min .. max) of {a.reps} after {a.warmup} warm-up calls, one process, ms.  `decode` is `codec.decode_batch` of {B} x {T} frames; `squeeze` is",
             f"`hip.silence_squeeze` of its output ({B} x {n} samples: hop activity, plan, gather over (tile of {hip.SIL_TILE} outputs, row), the upload of",
             "the per-row arguments and the host copy of the lengths and cuts included).  These are records, not bars.", "",
             "| what | shape | ms | of the decode | note |", "|---|---|---|---|---|",
             f"| decode | {B} x {T} frames | {fmt(dec)} | 1 | |", *rows, ""]
    for ln in lines:
        print(ln, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
