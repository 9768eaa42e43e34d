"""Cost of word timestamps beside the pass they follow.

One process, synthetic EOS-suppressed checkpoint: ``synthesize_batch`` of 32 texts of 64 ids at 200 frames, once without the
``alignment=`` sink and once with it, on the same build; wall clock around the synchronised call, ``--repeats`` timed calls after
warm-up, median and spread.  The ``nar`` phase of the same call (``timings=``) is the yardstick the post-pass is compared with.

    python tools/align_timing.py [--out profiles/align_timing.md] [--repeats 5] [--warmup 2]
    python tools/align_timing.py --no-sink-only            # prints the time of the call without the sink (also runs on a tree that
                                                           # has no word timestamps yet: the parent's number in the table)
    python tools/align_timing.py --parent-ms "a,b,c,d,e"   # fold the parent's five repeats into the table
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/align_timing.py --trace-run      # per-kernel times ...
    python tools/align_timing.py --kernel-stats DIR/.../*_kernel_stats.csv                     # ... folded into the table
"""
from __future__ import annotations

import argparse
import csv
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, FRAMES, S = 32, 200, 64
POST_PASS_KERNELS = ("align_scores_kernel", "align_dp_wave_kernel", "align_dp_wide_kernel", "gemm_f32_kernel", "::norm_kernel", "dwconv_kernel",
                     "codebook_sum_kernel", "attn_mfma_kernel<96")


class Tok:
    vocab_size = 512

    def encode(self, text):
        return [1 + (ord(c) % 500) for c in text]


def engine():
    from sopro_amd import SoproTTS
    from sopro_amd.config import MimiDecoderConfig, SoproTTSConfig
    from sopro_amd.weights import synth_mimi_weights, synth_sopro_weights

    cfg, mc = SoproTTSConfig(), MimiDecoderConfig()
    tts = SoproTTS.from_weights(cfg, synth_sopro_weights(cfg, 512, 1234, suppress_eos=True), synth_mimi_weights(mc, 1234), Tok(), device="cuda:0")
    rng = np.random.default_rng(5)
    ref = tts.prepare_reference(ref_tokens_tq=torch.from_numpy(rng.integers(0, 2048, size=(24, 32))))
    ids = [torch.from_numpy(rng.integers(1, 500, size=S)) for _ in range(B)]
    return tts, ref, ids


def call(tts, ref, ids, sink=None, timings=None):
    kw = dict(alignment=sink) if sink is not None else {}
    out = tts.synthesize_batch([""] * B, [ref] * B, text_ids=ids, max_frames=FRAMES - 1, top_p=0.0, temperature=1.0, anti_loop=False, seed=3,
                               timings=timings, **kw)
    torch.cuda.synchronize()
    return out


def wall(fn, warmup: int, repeats: int):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def fmt(ms):
    return f"{statistics.median(ms):.2f} ({min(ms):.2f} .. {max(ms):.2f})"


def kernel_rows(path: str):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((r["Name"], int(r["Calls"]), float(r["TotalDurationNs"]) / 1e6, float(r["AverageNs"]) / 1e3))
    return sorted(rows, key=lambda r: -r[2])


def kernel_table(path: str):
    """The kernels the post-pass launches, from a kernel-stats file of a --trace-run (three calls with the sink)."""
    rows = [r for r in kernel_rows(path) if any(k in r[0] for k in POST_PASS_KERNELS) and r[1] >= 3]
    lines = ["Kernels the post-pass launches, from `rocprofv3 --kernel-trace --stats -- python tools/align_timing.py --trace-run` (three calls with the",
             "sink; the contraction, norm, depthwise and gather rows also hold the few launches other stages make of the same kernels):", "",
             "| kernel | calls | total ms per call of `synthesize_batch` | mean us |", "|---|---|---|---|"]
    for name, calls, ms, us in rows:
        short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        lines.append(f"| `{short}` | {calls} | {ms / 3.0:.3f} | {us:.1f} |")
    return lines + [""]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/align_timing.md")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-sink-only", action="store_true")
    ap.add_argument("--trace-run", action="store_true", help="three calls with the sink and nothing else (run it under rocprofv3)")
    ap.add_argument("--parent-ms", default="", help="the parent commit's --no-sink-only repeats, comma separated")
    ap.add_argument("--kernel-stats", default="", help="a *_kernel_stats.csv of a --trace-run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--table-only", action="store_true", help="print the kernel table of --kernel-stats and stop (needs no device)")
    a = ap.parse_args()
    if a.table_only:
        print("\n".join(kernel_table(a.kernel_stats)))
        return
    tts, ref, ids = engine()
    if a.trace_run:
        for _ in range(3):
            call(tts, ref, ids, sink=[])
        return
    plain = wall(lambda: call(tts, ref, ids), a.warmup, a.repeats)
    print("without the sink, ms:", ",".join(f"{v:.3f}" for v in plain), flush=True)
    if a.no_sink_only:
        return
    from sopro_amd import hip

    n0 = hip.align_calls
    call(tts, ref, ids)
    assert hip.align_calls == n0
    timed = wall(lambda: call(tts, ref, ids, sink=[]), a.warmup, a.repeats)
    nar = []
    for _ in range(a.repeats):
        t = {}
        call(tts, ref, ids, timings=t)
        nar.append(t["nar"] * 1e3)
    # the post-pass alone, device events on the bulk stream: the same replay on the state of a finished AR phase
    m = tts.model
    sink = []
    call(tts, ref, ids, sink=sink)
    frames = [len(x.path) for x in sink]
    state = m.phase_ar(ids, [ref] * B, max_frames=FRAMES - 1, top_p=0.0, temperature=1.0, anti_loop=False, style_strength=float(tts.cfg.style_strength),
                       min_gen_frames=None, seed=3)
    post = []
    for i in range(a.warmup + a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(m.bulk_stream):
            e0.record()
            m.align_batch(state["prep"], state)
            e1.record()
        e1.synchronize()
        if i >= a.warmup:
            post.append(e0.elapsed_time(e1))
    parent = [float(v) for v in a.parent_ms.split(",") if v.strip()]
    conf = statistics.median(x.confidence for x in sink)
    lines = ["# Word timestamps: time beside the pass they follow", "",
             f"Command: `python tools/align_timing.py --repeats {a.repeats} --warmup {a.warmup}` on {torch.cuda.get_device_name(0)}; one process,",
             f"synthetic EOS-suppressed checkpoint, `synthesize_batch` of {B} texts of {S} ids, {min(frames)} frames per row, greedy; wall clock around the",
             f"synchronised call, median (min .. max) of {a.repeats} after {a.warmup} warm-up calls.  `post-pass` is `model.align_batch` alone (device events:",
             "the teacher-forced replay of the six AR blocks, three `sopro_align_scores_f32` launches, one `sopro_align_dp_f32`, one download);",
             "`nar` is the refinement phase of the same call (`timings=`).", "",
             "| what | ms |", "|---|---|"]
    if parent:
        lines.append(f"| parent commit, no sink | {fmt(parent)} |")
    lines += [f"| this build, no sink | {fmt(plain)} |", f"| this build, `alignment=[]` | {fmt(timed)} |", f"| post-pass alone | {fmt(post)} |",
              f"| `nar` phase | {fmt(nar)} |", ""]
    if parent:
        spread = max(parent) - min(parent)
        d = statistics.median(plain) - statistics.median(parent)
        lines += [f"Without the sink the call takes {statistics.median(plain):.2f} ms against the parent's {statistics.median(parent):.2f} ms: a difference of "
                  f"{d:+.2f} ms, the parent's own five repeats spread over {spread:.2f} ms.", ""]
    ratio = statistics.median(post) / statistics.median(nar)
    lines += [f"The post-pass costs {statistics.median(post):.2f} ms, {ratio:.2f} of the `nar` phase ({statistics.median(nar):.2f} ms).  Expectation was \"well under\": "
              + ("it holds." if ratio < 0.5 else "it does NOT hold - the replay runs on the plain fp32 contraction (`sopro_gemm_f32`), one MFMA pass per "
                 "product at fp32 rate, where the refinement uses the three-pass f16 operands at matrix-core rate; see the kernel table."),
              f"Median path confidence on this checkpoint: {conf:.4f} (flat maps give 1 / {S} = {1.0 / S:.4f}).", ""]
    if a.kernel_stats:
        lines += kernel_table(a.kernel_stats)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
