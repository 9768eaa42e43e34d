"""Long-form synthesis against the caller's loop it replaces, and the join's three launches on their own.

One process, EOS-suppressed synthetic checkpoint (every segment runs its whole frame budget), a text of 64 sentences, max_frames 200,
seeded.  After one warm-up each, with a device synchronise around every timed region:
  (a) loop        the caller's loop over the existing API: synthesize() per segment, .cpu(), numpy concatenate
  (b) long        synthesize_long(plan="throughput")
  (c) first_piece time to the first piece of stream_long (plan "latency": one batch-of-one pass)
  (d) join        sopro_join_edges_f32 / _layout_i64 / _mix_f32 alone, by device events, on the decoder's own 64 x 200-frame batch:
                  GB/s of wav read (edges) and of kept samples read plus out written (mix), beside the ~6.3 TB/s an element-wise
                  kernel can reach on this device
Writes one JSON document (default profiles/longform_probe.json) with the command line.

    python tools/longform_probe.py [--out profiles/longform_probe.json] [--segments 64] [--frames 200] [--reps 3]
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

ACHIEVABLE_GBS = 6300.0


class _Tok:
    vocab_size = 512

    def encode(self, text):
        return [1 + (ord(c) % 500) for c in text]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/longform_probe.json")
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    from sopro_amd import SoproTTS, hip
    from sopro_amd.config import MimiDecoderConfig, SoproTTSConfig
    from sopro_amd.longform import join_params, pause_samples, split_text
    from sopro_amd.weights import synth_mimi_weights, synth_sopro_weights

    cfg, mc = SoproTTSConfig(), MimiDecoderConfig()
    tts = SoproTTS.from_weights(cfg, synth_sopro_weights(cfg, 512, 1234, suppress_eos=True), synth_mimi_weights(mc, 1234), _Tok(), device="cuda:0")
    rng = np.random.default_rng(3)
    ref = tts.prepare_reference(ref_tokens_tq=torch.from_numpy(rng.integers(0, 2048, size=(150, 32))))
    text = " ".join(f"Sentence number {i} of the probe text says a few more words than the one before it did." for i in range(a.segments))
    segs = split_text(text)
    assert len(segs) == a.segments
    kw = dict(max_frames=int(a.frames), seed=int(a.seed))
    sync = torch.cuda.synchronize

    def loop():
        sync()
        t0 = time.perf_counter()
        out = np.concatenate([tts.synthesize(s.text, ref=ref, max_frames=kw["max_frames"], seed=kw["seed"] + k).cpu().numpy().reshape(-1)
                              for k, s in enumerate(segs)])
        sync()
        return time.perf_counter() - t0, out.size

    def long():
        sync()
        t0 = time.perf_counter()
        res = tts.synthesize_long(text, ref=ref, plan="throughput", **kw)
        sync()
        return time.perf_counter() - t0, int(res.wav.numel())

    def first_piece():
        sync()
        t0 = time.perf_counter()
        it = tts.stream_long(text, ref=ref, **kw)
        next(it)
        sync()
        dt = time.perf_counter() - t0
        it.close()
        return dt

    loop(), long(), first_piece()  # warm-up: recorded graphs, scratch, every batch shape of the two plans' first groups
    res = {"argv": sys.argv, "device": torch.cuda.get_device_name(0), "segments": len(segs), "max_frames": int(a.frames), "reps": int(a.reps),
           "how": "host wall time between device synchronises, best and median of `reps` after one warm-up each; join: device events "
                  "around each step (edges = its two launches), median of 20 after 3 warm-ups on the same buffers: a batch below the 256 MB last-level "
                  "cache is read cache-warm, as it is right after the decoder wrote it"}
    for name, fn in (("loop", loop), ("long", long)):
        runs = [fn() for _ in range(a.reps)]
        ts = [r[0] for r in runs]
        res[name] = {"ms_best": round(1e3 * min(ts), 2), "ms_median": round(1e3 * float(np.median(ts)), 2), "samples": runs[0][1],
                     "audio_s_per_s": round(runs[0][1] / 24000.0 / min(ts), 1)}
        print(name, json.dumps(res[name]), flush=True)
    res["long_over_loop"] = round(res["loop"]["ms_best"] / res["long"]["ms_best"], 2)
    fp = [first_piece() for _ in range(a.reps)]
    res["first_piece"] = {"ms_best": round(1e3 * min(fp), 2), "ms_median": round(1e3 * float(np.median(fp)), 2)}
    print("first_piece", json.dumps(res["first_piece"]), flush=True)

    # (d) the join alone, on the decoder's own batch (two 32-row passes side by side: 64 x frames)
    rows = [tts.synthesize_batch([s.text for s in segs[i: i + 32]], [ref] * len(segs[i: i + 32]), max_frames=kw["max_frames"], seed=kw["seed"],
                                 padded=True) for i in range(0, min(64, len(segs)), 32)]
    wav = torch.cat([r.wav for r in rows]).contiguous()
    lens = [n for r in rows for n in r.lens]
    n = len(lens)
    gaps = [pause_samples("sentence")] * n
    jp = join_params(-40.0, 30.0, 5.0)
    lib, dev = hip.load(), wav.device
    args = torch.tensor([lens, gaps], dtype=torch.int32).to(dev)
    meta = torch.empty(2 * n + 1, dtype=torch.int64, device=dev)
    offs_d, edges_d = meta[: n + 1], meta[n + 1:].view(torch.int32)
    ws = torch.empty(int(lib.sopro_join_workspace_bytes(n, max(lens), jp["hop"])) // 4, device=dev)
    out = torch.empty(sum(lens) + sum(gaps), device=dev)
    tab = hip.fade_table(jp["fade_len"], dev)
    s = torch.cuda.current_stream().cuda_stream
    times = {"edges": [], "layout": [], "mix": []}
    for rep in range(23):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        hip._check(lib.sopro_join_edges_f32(wav.data_ptr(), int(wav.stride(0)), args[0].data_ptr(), n, max(lens), jp["hop"], jp["rel"], jp["keep"], 1,
                                            ws.data_ptr(), edges_d.data_ptr(), s), "edges")
        ev[1].record()
        hip._check(lib.sopro_join_layout_i64(edges_d.data_ptr(), args[1].data_ptr(), n, offs_d.data_ptr(), s), "layout")
        ev[2].record()
        hip._check(lib.sopro_join_mix_f32(wav.data_ptr(), int(wav.stride(0)), edges_d.data_ptr(), offs_d.data_ptr(), tab.data_ptr(), jp["fade_len"], n,
                                          out.data_ptr(), int(out.numel()), s), "mix")
        ev[3].record()
        sync()
        if rep >= 3:
            for i, k in enumerate(("edges", "layout", "mix")):
                times[k].append(ev[i].elapsed_time(ev[i + 1]))
    host = meta.cpu()
    total = int(host[n])
    kept = int((host[n + 1:].view(torch.int32).reshape(n, 2)[:, 1] - host[n + 1:].view(torch.int32).reshape(n, 2)[:, 0]).sum())
    med = {k: float(np.median(v)) for k, v in times.items()}
    b_edges, b_mix = 4.0 * sum(lens), 4.0 * (kept + total)
    res["join"] = {"rows": n, "samples_in": sum(lens), "samples_kept": kept, "samples_out": total,
                   "edges_ms": round(med["edges"], 4), "layout_ms": round(med["layout"], 4), "mix_ms": round(med["mix"], 4),
                   "edges_gb_s": round(b_edges / med["edges"] * 1e-6, 1), "mix_gb_s": round(b_mix / med["mix"] * 1e-6, 1),
                   "all_gb_s": round((b_edges + b_mix) / (med["edges"] + med["layout"] + med["mix"]) * 1e-6, 1),
                   "achievable_gb_s": ACHIEVABLE_GBS,
                   "edges_share_of_achievable": round(b_edges / med["edges"] * 1e-6 / ACHIEVABLE_GBS, 3),
                   "share_of_long_ms": round((med["edges"] + med["layout"] + med["mix"]) / res["long"]["ms_best"], 5)}
    print("join", json.dumps(res["join"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
