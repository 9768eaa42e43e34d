"""Cost of the similarity sink beside the per-voice path it avoids and the bulk phase it rides on.

One process, synthetic checkpoint (EOS suppressed, so every row runs its full length), random token batches.  For 32 x 200 and
128 x 200 frames:
  * ``batched``: ``model.speaker_vectors`` + the pairwise ``hip.spk_cosine`` on the bulk stream (three launches for the batch), the
    lengths already on the device - device events, and the host clock around the same calls ending in a stream synchronise;
  * ``per voice``: the same rows through ``model.token2sv`` one at a time (eight launches and one synchronise each) - the host clock
    around the loop.  ``token2sv`` and ``sopro_ref_prepare`` are unchanged against the parent commit, so this IS the parent's path;
  * ``bulk phase``: refinement + decoder of ``synthesize_batch`` at that size (its ``timings``: device events on the bulk stream).
The two orders are alternated within one process, warm-up first, medians of ``--reps``.  Writes a markdown table (default
profiles/spk_timing.md) with the command line.  Condition stated there: at 32 x 200 the batched call is faster than the 32 calls.

    python tools/spk_timing.py [--out profiles/spk_timing.md] [--reps 20] [--warmup 3]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def med(xs):
    return f"{statistics.median(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f})"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/spk_timing.md")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bulk-reps", type=int, default=3)
    a = ap.parse_args()
    from sopro_amd import SoproTTS, hip
    from sopro_amd.config import MimiDecoderConfig, SoproTTSConfig
    from sopro_amd.weights import synth_mimi_weights, synth_sopro_weights

    class Tok:
        vocab_size = 512

        def encode(self, text):
            return [1 + (ord(c) % 500) for c in text]

    cfg, mc = SoproTTSConfig(), MimiDecoderConfig()
    tts = SoproTTS.from_weights(cfg, synth_sopro_weights(cfg, 512, 1234, suppress_eos=True), synth_mimi_weights(mc, 1234), Tok(), device="cuda:0")
    m, dev = tts.model, "cuda:0"
    rng = np.random.default_rng(5)
    ref = tts.prepare_reference(ref_tokens_tq=torch.from_numpy(rng.integers(0, 2048, size=(150, 32))))
    lines = ["# Voice similarity: the batched Token2SV beside the per-voice path and the bulk phase", "",
             f"Command: `python tools/spk_timing.py --reps {a.reps} --warmup {a.warmup} --bulk-reps {a.bulk_reps}` on {torch.cuda.get_device_name(0)}, one",
             f"process, clocks as the machine left them (not pinned; every figure follows {a.warmup} warm-up calls of its own shape).  ms, median (min ..",
             f"max) of {a.reps}; the two paths alternate call by call.  `batched` = `model.speaker_vectors` + pairwise `hip.spk_cosine` for the whole",
             "batch on the bulk stream (3 launches), timed by device events and by the host clock around the calls ending in a synchronise;",
             "`per voice` = the same rows through `model.token2sv` one row at a time (8 launches and a synchronise each; the function is",
             "unchanged against the parent commit, so this is the parent's path), host clock around the loop; `bulk phase` = refinement +",
             f"decoder of one `synthesize_batch` of that size (device events, median of {a.bulk_reps}).  The ratios are recorded, not asserted.", "",
             "| rows x frames | batched, device ms | batched, host ms | per voice, host ms | per voice / batched (host) | bulk phase ms | batched / bulk phase |",
             "|---|---|---|---|---|---|---|"]
    ok, notes = None, []
    for B, T in ((32, 200), (128, 200)):
        toks = torch.from_numpy(rng.integers(0, 2048, size=(B, T, 32))).to(dev).to(torch.int32)
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        rows64 = [toks[b: b + 1].long() for b in range(B)]
        ref_m = ref.sv_ref.reshape(1, -1).expand(B, -1).contiguous()

        def batched():
            with torch.cuda.stream(m.bulk_stream):
                return hip.spk_cosine(m.speaker_vectors(toks, lens), ref_m)

        def per_voice():
            return [m.token2sv(r) for r in rows64]

        for _ in range(a.warmup):
            batched()
            per_voice()
        torch.cuda.synchronize()
        # the two paths agree on the rows that are timed (faster and different would not be faster)
        with torch.cuda.stream(m.bulk_stream):
            sv_b = m.speaker_vectors(toks, lens)
        m.bulk_stream.synchronize()
        agree = float((sv_b - torch.cat(per_voice())).abs().max())
        ev_ms, host_ms, pv_ms = [], [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(m.bulk_stream)
            batched()
            e1.record(m.bulk_stream)
            m.bulk_stream.synchronize()
            host_ms.append(1e3 * (time.perf_counter() - t0))
            ev_ms.append(e0.elapsed_time(e1))
            t0 = time.perf_counter()
            per_voice()
            torch.cuda.synchronize()
            pv_ms.append(1e3 * (time.perf_counter() - t0))
        bulk = []
        ids = [torch.from_numpy(rng.integers(1, 500, size=24)) for _ in range(B)]
        for i in range(a.bulk_reps + 1):
            tm = {}
            tts.synthesize_batch([""] * B, [ref] * B, text_ids=ids, max_frames=T, top_p=0.0, temperature=1.0, anti_loop=False, seed=3, timings=tm)
            torch.cuda.synchronize()
            if i:  # (the first pass records the launch sequences of this shape)
                bulk.append(1e3 * (tm["nar"] + tm["mimi"]))
        hb, hp, bk = statistics.median(host_ms), statistics.median(pv_ms), statistics.median(bulk)
        if (B, T) == (32, 200):
            ok = hb < hp
        lines.append(f"| {B} x {T} | {med(ev_ms)} | {med(host_ms)} | {med(pv_ms)} | {hp / hb:.1f} | {med(bulk)} | {statistics.median(ev_ms) / bk:.4f} |")
        print(lines[-1], f"  max |sv batched - sv per voice| = {agree:.2e}", flush=True)
        notes.append(f"{B} x {T}: max |sv batched - sv per voice| = {agree:.2e}")
    lines += ["", "Agreement of the two paths on the timed rows (two fp32 orders): " + "; ".join(notes) + ".", "",
              f"Condition (at 32 x 200 the batched call takes less time than the 32 per-voice calls): {'met' if ok else 'NOT met'}.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
