"""Cost of the pitch resampler beside the decode and the stretch it follows, and of a ``synthesize_batch`` call at ``pitch=0``.

Kernel table (the default): one process, synthetic codec checkpoint, random token batches.  For 32 x 200 frames and 1 x 400 frames:
``codec.decode_batch`` of the token batch (the yardstick: what produces the rows), then for pitch -4 / +4 / +12 ``hip.time_stretch``
of the decoded batch at the step ``hip.prosody_step(1.0, pitch)`` gives and ``hip.pitch_shift`` of the stretched batch.  Warm-up,
then device events around every call, median of ``--reps``.

The call (``--batch-json FILE``): a ``synthesize_batch`` of 32 fixed-length rows on the synthetic EOS-suppressed checkpoint, timed
with a host clock around the call (it ends in a stream synchronise); ``pitch=0.0`` is passed where the package has the keyword.
``--tree DIR`` imports the package from another checkout (the parent commit's) so that both are timed by this one script; with
``SOPRO_HIP_LIB`` pointing at one library for both, what differs between them is the host code of the call.  The kernel-table run
takes the files of both, in the order they were measured, and writes them beside each other.

    python tools/pitch_timing.py --batch-json this_1.json
    python tools/pitch_timing.py --batch-json parent_1.json --tree ../parent      (alternate the two, a few times)
    python tools/pitch_timing.py --this this_*.json --parent parent_*.json [--out profiles/pitch_timing.md] [--reps 20] [--warmup 3]
"""
from __future__ import annotations

import argparse
import inspect
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB, SEED = 512, 1234


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


class _Tok:
    vocab_size = VOCAB

    def encode(self, text):
        return [1 + (ord(c) % 500) for c in text]


def batch_call(a) -> None:
    """Time synthesize_batch(32 rows x 200 frames) and write one JSON record."""
    from sopro_amd import SoproTTS
    from sopro_amd.config import MimiDecoderConfig, SoproTTSConfig
    from sopro_amd.weights import synth_mimi_weights, synth_sopro_weights

    cfg, mc = SoproTTSConfig(), MimiDecoderConfig()
    tts = SoproTTS.from_weights(cfg, synth_sopro_weights(cfg, VOCAB, SEED, suppress_eos=True), synth_mimi_weights(mc, SEED), _Tok(), device="cuda:0")
    ref = tts.prepare_reference(ref_tokens_tq=torch.from_numpy(np.random.default_rng(5).integers(0, 2048, size=(24, 32))))
    texts = [f"row {k}: a sentence of ordinary length for the timing of one batch" for k in range(a.rows)]
    kw = dict(max_frames=a.frames, seed=4)
    has_pitch = "pitch" in inspect.signature(SoproTTS.synthesize_batch).parameters
    if has_pitch:
        kw["pitch"] = 0.0
    ms = []
    for k in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = tts.synthesize_batch(texts, [ref] * a.rows, **kw)
        torch.cuda.synchronize()
        if k >= a.warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    rec = dict(rows=a.rows, frames=a.frames, reps=a.reps, warmup=a.warmup, has_pitch=has_pitch, median_ms=statistics.median(ms), min_ms=min(ms),
               max_ms=max(ms), samples=int(out[0].shape[-1]))
    os.makedirs(os.path.dirname(os.path.abspath(a.batch_json)), exist_ok=True)
    with open(a.batch_json, "w") as f:
        json.dump(rec, f)
    print(json.dumps(rec), flush=True)


def kernel_table(a) -> None:
    from sopro_amd import hip
    from sopro_amd.codec import MimiCodec
    from sopro_amd.config import MimiDecoderConfig
    from sopro_amd.weights import synth_mimi_weights

    mc = MimiDecoderConfig()
    codec = MimiCodec(synth_mimi_weights(mc, SEED), mc, "cuda:0")
    rng = np.random.default_rng(5)
    lines = ["# Pitch resampler: time beside the decode and the stretch it follows", "",
             f"Command: `python tools/pitch_timing.py --reps {a.reps} --warmup {a.warmup}` on {torch.cuda.get_device_name(0)}; device events,",
             f"median (min .. max) of {a.reps} after {a.warmup} warm-up calls, one process.  `decode` is `codec.decode_batch` of the token batch,",
             "`stretch` is `hip.time_stretch` of its output at the step of the pitch (speed 1.0), `resample` is `hip.pitch_shift` of the",
             f"stretched batch (one launch over (row, tile of {hip.PITCH_TILE} outputs)).  These are records, not bars.", "",
             "| batch | pitch | outputs per row | decode ms | stretch ms | resample ms | resample / decode | ns per output |", "|---|---|---|---|---|---|---|---|"]
    for B, T in ((32, 200), (1, 400)):
        toks = torch.from_numpy(rng.integers(0, 2048, size=(B, T, int(mc.num_quantizers)))).to("cuda:0")
        with torch.cuda.stream(codec.stream):
            dec = timed(lambda: codec.decode_batch(toks), a.warmup, a.reps)
        wav = codec.decode_batch(toks)
        n = int(wav.shape[1])
        for v in (-4.0, 4.0, 12.0):
            step, inc = hip.prosody_step(1.0, v)
            mid_len = hip.tsm_out_len(n, step)
            mid = torch.empty(B, mid_len, device="cuda:0")
            st = timed(lambda: hip.time_stretch(wav, [n] * B, None, steps=[step] * B, out=mid), a.warmup, a.reps)
            out_len = hip.pitch_out_len(mid_len, inc)
            out = torch.empty(B, out_len, device="cuda:0")
            rs = timed(lambda: hip.pitch_shift(mid, [mid_len] * B, None, incs=[inc] * B, out=out), a.warmup, a.reps)
            lines.append(f"| {B} x {T} | {v:+g} | {out_len} | {fmt(dec)} | {fmt(st)} | {fmt(rs)} | {rs[0] / dec[0]:.3f} | {1e6 * rs[0] / max(1, B * out_len):.3f} |")
            print(lines[-1], flush=True)
    if a.this and a.parent:
        load = lambda paths: [json.load(open(p)) for p in paths]
        this, parent = load(a.this), load(a.parent)
        r0 = this[0]
        lines += ["", f"## `synthesize_batch` at `pitch=0` against the parent commit ({r0['rows']} rows x {r0['frames']} frames)", "",
                  f"`python tools/pitch_timing.py --batch-json FILE [--tree PARENT]`, one process per line, the two trees alternating; host clock around",
                  f"the call (it ends in a stream synchronise), median (min .. max) of {r0['reps']} calls after {r0['warmup']} warm-up calls, ms.  Both trees load",
                  "the same kernel library (the parent's own is this one without pitch.hip), so the lines differ by the host code of the call.", "",
                  "| run | this tree, pitch=0.0 | parent commit |", "|---|---|---|"]
        for k, (t, p) in enumerate(zip(this, parent)):
            lines.append(f"| {k + 1} | {t['median_ms']:.2f} ({t['min_ms']:.2f} .. {t['max_ms']:.2f}) | {p['median_ms']:.2f} ({p['min_ms']:.2f} .. {p['max_ms']:.2f}) |")
        tm, pm = [t["median_ms"] for t in this], [p["median_ms"] for p in parent]
        lines += ["", f"Medians: this tree {min(tm):.2f} .. {max(tm):.2f} ms, parent {min(pm):.2f} .. {max(pm):.2f} ms over the runs; the parent's own run-to-run "
                      f"spread is {max(pm) - min(pm):.2f} ms, the difference of the two means {statistics.mean(tm) - statistics.mean(pm):+.2f} ms."]
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/pitch_timing.md")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch-json", default=None, help="time one synthesize_batch shape and write this JSON file instead of the table")
    ap.add_argument("--tree", default=HERE, help="the checkout whose sopro_amd package is imported (default: this one)")
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--this", nargs="*", default=[], help="--batch-json files of this tree")
    ap.add_argument("--parent", nargs="*", default=[], help="--batch-json files of the parent commit's tree, in the same order")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    if a.batch_json:
        batch_call(a)
    else:
        kernel_table(a)


if __name__ == "__main__":
    main()
