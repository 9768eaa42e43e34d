"""Cost of the watermark beside the decode whose rows it marks.

One process, synthetic codec checkpoint, random tokens: ``codec.decode_batch`` of 32 x 200 frames (the yardstick: what produces the
rows), ``hip.wm_embed`` of the decoded batch (32 x 384 000 samples, every row marked; and the same batch with half of the rows
unmarked), ``hip.wm_detect_rows`` of 32 x 72 000 samples (three seconds per clip), and the detector on one clip.  Warm-up, then
device events around every call, median of ``--reps``.  The embedder reads and writes every sample once (98 MB for the batch): the
table gives the achieved GB/s on that count.

    python tools/wm_timing.py [--out profiles/wm_timing.md] [--reps 20] [--warmup 5]
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
    ap.add_argument("--out", default="profiles/wm_timing.md")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    from sopro_amd import Watermark, hip
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
    n = int(wav.shape[1])
    marks = [Watermark(0x0123456789ABCDEF ^ (k % 3), k) for k in range(B)]  # three keys, one tag per row
    out = torch.empty(B, n, device="cuda:0")
    emb = timed(lambda: hip.wm_embed(wav, [n] * B, marks, out=out), a.warmup, a.reps)
    half = [m if k % 2 else None for k, m in enumerate(marks)]
    emb_half = timed(lambda: hip.wm_embed(wav, [n] * B, half, out=out), a.warmup, a.reps)
    mb = 2 * 4 * B * n / 1e6
    clips = out[:, :72000]
    keys = [m.key for m in marks]
    det = timed(lambda: hip.wm_detect_rows(clips, [72000] * B, keys), a.warmup, a.reps)
    det1 = timed(lambda: hip.wm_detect_rows(clips[:1], [72000], keys[:1]), a.warmup, a.reps)
    lines = ["# Watermark: time beside the decode whose rows it marks", "",
             f"Command: `python tools/wm_timing.py --reps {a.reps} --warmup {a.warmup}` on {torch.cuda.get_device_name(0)}; device events, median",
             f"(min .. max) of {a.reps} after {a.warmup} warm-up calls, one process, ms.  `decode` is `codec.decode_batch` of {B} x {T} frames; `embed` is",
             f"`hip.wm_embed` of its output ({B} x {n} samples, one launch over (row, tile of {hip.WM_TILE} samples), the upload of the per-row",
             "arguments included); `detect` is `hip.wm_detect_rows` (block maxima, fold, two 8192 x 8192 correlations per clip, peaks, and the",
             "host copy of the result).  These are records, not bars.", "",
             "| what | shape | ms | of the decode | note |", "|---|---|---|---|---|",
             f"| decode | {B} x {T} frames | {fmt(dec)} | 1 | |",
             f"| embed, every row marked | {B} x {n} | {fmt(emb)} | {emb[0] / dec[0]:.4f} | {mb:.0f} MB read + written: {mb / emb[0]:.0f} GB/s |",
             f"| embed, every other row unmarked | {B} x {n} | {fmt(emb_half)} | {emb_half[0] / dec[0]:.4f} | |",
             f"| detect | {B} x 72000 | {fmt(det)} | {det[0] / dec[0]:.4f} | {det[0] / B:.3f} ms per clip |",
             f"| detect | 1 x 72000 | {fmt(det1)} | {det1[0] / dec[0]:.4f} | |", ""]
    for ln in lines:
        print(ln, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
