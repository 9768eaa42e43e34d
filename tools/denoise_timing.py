"""Cost of the reference denoiser: the operator alone, and ``prepare_reference`` with and without it.

One process, synthetic checkpoints.  Warm-up, then timed calls, median (min .. max) of ``--reps``:
  * ``hip.denoise`` of 1 x 12 s and 32 x 12 s at 24 kHz (the synthetic voice under white noise at 10 dB), device events;
  * ``prepare_reference(ref_audio_path=...)`` of a 12 s, 24 kHz PCM16 clip with ``denoise=`` set and without it, host clock (the call
    ends in a device synchronise and includes reading the file and the energy trim on the host).
``--op-only`` runs only the operator loops, for a kernel trace of their own:
    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/denoise_timing.py --op-only
``--trace DIR/.../t_kernel_trace.csv`` adds the per-kernel medians of that trace to the table (launches told apart by their grid).

    python tools/denoise_timing.py [--out profiles/denoise_timing.md] [--reps 20] [--warmup 5] [--trace CSV] [--label TEXT]
"""
from __future__ import annotations

import argparse
import csv
import os
import statistics
import sys
import tempfile
import time
import wave

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1234
SECONDS, SR = 12.0, 24000


def timed_events(fn, warmup: int, reps: int):
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


def timed_host(fn, warmup: int, reps: int):
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


def kernel_rows(path: str, frames: int):
    """Median duration per (kernel, rows) from a rocprofv3 kernel trace: the launches of the operator carry the row count in a grid
    dimension (report: x; the others: y), in work-items."""
    per = {}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        short = next((k for k in ("dn_analysis_kernel", "dn_track_kernel", "dn_synth_kernel", "dn_ola_kernel", "dn_report_kernel") if k in name), None)
        if short is None:
            continue
        wx = int(r.get("Workgroup_Size_X", 1) or 1)
        gx, gy = int(r.get("Grid_Size_X", 0) or 0), int(r.get("Grid_Size_Y", 1) or 1)
        rows = gx // wx if short == "dn_report_kernel" else gy
        per.setdefault((short, rows), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = []
    for (short, rows), us in sorted(per.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        out.append(f"| {short} | {rows} x {frames} frames | {statistics.median(us):.1f} ({min(us):.1f} .. {max(us):.1f}) | {len(us)} |")
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/denoise_timing.md")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--op-only", action="store_true")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import denoise_ref as R
    from sopro_amd import hip

    has_dn = hasattr(hip, "denoise")  # (the same tool times prepare_reference on a tree without the operator)
    n = int(SECONDS * SR)
    _, x = R.noisy_voice(SECONDS, "white", snr=10.0, seed=5)
    lines = ["# Reference denoising: time of the operator and of prepare_reference with and without it", "",
             f"Command: `python tools/denoise_timing.py --reps {a.reps} --warmup {a.warmup}`{' (' + a.label + ')' if a.label else ''} on "
             f"{torch.cuda.get_device_name(0)}; median (min .. max) of {a.reps} after {a.warmup} warm-up calls, one process.  These are records, not bars.", ""]
    if has_dn:
        from sopro_amd import Denoise

        lines += ["| what | shape | ms | note |", "|---|---|---|---|"]
        for B in (1, 32):
            wav = torch.from_numpy(np.tile(x.astype(np.float32), (B, 1))).cuda()
            out = torch.empty_like(wav)
            t = timed_events(lambda: hip.denoise(wav, [n] * B, Denoise(), out=out), a.warmup, a.reps)
            lines.append(f"| hip.denoise | {B} x {n} samples ({B} x {R.n_frames(n)} frames) | {fmt(t)} | device events; {B * SECONDS / (t[0] * 1e-3):.0f} s of audio per s |")
        lines.append("")
    if not a.op_only:
        from sopro_amd import SoproTTS
        from sopro_amd.config import MimiDecoderConfig, SoproTTSConfig
        from sopro_amd.weights import synth_mimi_weights, synth_sopro_weights

        class Tok:
            vocab_size = 512

            def encode(self, text):
                return [1 + (ord(c) % 500) for c in text]

        cfg, mc = SoproTTSConfig(), MimiDecoderConfig()
        tts = SoproTTS.from_weights(cfg, synth_sopro_weights(cfg, 512, SEED), synth_mimi_weights(mc, SEED, with_encoder=True), Tok(), device="cuda:0")
        path = os.path.join(tempfile.mkdtemp(prefix="denoise_timing_"), "clip.wav")
        with wave.open(path, "wb") as f:
            f.setnchannels(1), f.setsampwidth(2), f.setframerate(SR)
            f.writeframes(np.round(np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())
        lines += ["| what | clip | ms | note |", "|---|---|---|---|"]
        # alternating: plain, denoised, plain again (the two plain figures bracket the run-to-run spread inside this process)
        order = [("prepare_reference, no denoise", None)]
        if has_dn:
            order += [("prepare_reference, denoise=Denoise()", Denoise()), ("prepare_reference, no denoise (again)", None)]
        for what, d in order:
            kw = {"denoise": d} if d is not None else {}
            t = timed_host(lambda: tts.prepare_reference(ref_audio_path=path, **kw), a.warmup, a.reps)
            lines.append(f"| {what} | {SECONDS:g} s, 24 kHz PCM16 | {fmt(t)} | host clock around the call and a device synchronise |")
        lines.append("")
    if a.trace:
        lines += ["Per kernel, from `rocprofv3 --kernel-trace` over `--op-only` (a run of its own; warm-up launches included), microseconds:", "",
                  "| kernel | shape | us | launches |", "|---|---|---|---|", *kernel_rows(a.trace, R.n_frames(n)), ""]
    for ln in lines:
        print(ln, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
