"""bench.py's multi-rank path on ONE GPU (SOPRO_BENCH_SHARE_GPU=1: every rank on device 0, gloo for the barrier / MAX):
the launch path the driver uses for N > 1 (torch.distributed.run, one rank per GPU), the per-rank input sharding and the
rank-0 JSON line.  Each rank's output must be what a single-GPU run on that rank's inputs produces.  These runs take --full
(parity, full record); the plain run and --dump-outputs are checked against one of them."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from sopro_amd.wire import float_to_pcm16le

pytestmark = pytest.mark.gpu
SMALL = ["--steps", "2", "--warmup", "1", "--batch", "4", "--frames", "24", "--lanes", "1", "--profile-steps", "0", "--ttfa-runs", "0",
         "--no-cpu-baseline"]


def _run(args, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *args], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, **(env or {})), cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def _bench(extra, env=None):
    r = _run(["--full", *extra], env)
    last = r.stdout.strip().splitlines()[-1]
    assert len(last) < 8192, len(last)  # the driver parses the last stdout line from a bounded buffer (round 5: 21 kB -> parsed = null)
    line = json.loads(last)
    for k in ("metric", "value", "unit", "n_gpus", "config", "roofline", "roofline_more", "cpu_baseline", "parity", "full_record"):
        assert k in line, k
    # everything the compact line leaves out is in the full record (side file + stderr); the line's keys are a subset of it
    full = [ln for ln in r.stderr.splitlines() if ln.startswith("[bench full record] ")]
    assert len(full) == 1
    full = json.loads(full[0][len("[bench full record] "):])
    assert json.load(open(os.path.join(ROOT, line["full_record"]))) == full
    assert full["value"] == line["value"] and full["parity"]["rank_output_sha16"] == line["parity"]["rank_output_sha16"]
    return dict(full, **line)


def test_two_ranks_reproduce_two_single_gpu_runs():
    two = _bench(["--gpus", "2"], env={"SOPRO_BENCH_SHARE_GPU": "1", "MASTER_PORT": "29547"})
    assert two["n_gpus"] == 2 and two["scaling"] == "weak" and two["steps"] == 2
    assert two["parity"]["timed_steps_identical"] and two["parity"]["timed_outputs_finite"]
    hashes = two["parity"]["rank_output_sha16"]
    assert len(hashes) == 2 and hashes[0] != hashes[1]  # the ranks synthesise different utterances
    for r in (0, 1):
        one = _bench(["--gpus", "1", "--input-rank", str(r)])
        assert one["n_gpus"] == 1 and one["parity"]["rank_output_sha16"] == [hashes[r]], r
    # whole-job aggregate: two ranks' audio over the slower rank's time
    assert two["value"] > 0 and abs(two["value"] * two["ms_per_step"] - 2 * 4 * 24 * 0.08 * 1e3) < 1e-3 * two["value"] * two["ms_per_step"]


def test_eight_ranks_on_the_shared_gpu():
    """The 8-GPU launch shape without an 8-GPU box: eight ranks through torch.distributed.run on the one device,
    each with its own inputs, pinned to its own slice of the host cores.  n_gpus == 8, eight distinct output hashes that equal
    the single-rank runs on the same inputs (ranks 0, 3, 7 re-run alone), per-rank host CPU time reported and below the wall
    time of a step (no rank's launch threads are starved)."""
    eight = _bench(["--gpus", "8"], env={"SOPRO_BENCH_SHARE_GPU": "1", "MASTER_PORT": "29549"})
    assert eight["n_gpus"] == 8 and eight["scaling"] == "weak" and eight["steps"] == 2
    assert eight["parity"]["timed_steps_identical"] and eight["parity"]["timed_outputs_finite"]
    hashes = eight["parity"]["rank_output_sha16"]
    assert len(hashes) == 8 and len(set(hashes)) == 8
    for r in (0, 3, 7):
        one = _bench(["--gpus", "1", "--input-rank", str(r)])
        assert one["parity"]["rank_output_sha16"] == [hashes[r]], r
    cpu = eight["host_cpu_s_per_step_by_rank"]
    assert len(cpu) == 8 and all(0.0 < c for c in cpu)
    # CPU seconds per step of any rank stay BELOW the step's wall time: the ranks wait for the device by blocking on its interrupt
    # (hip.set_host_wait at process start; with the runtime's spin wait every waiting thread is a busy core - r03: 3.6x the wall time)
    assert eight["host_wait"].startswith("blocking")
    assert max(cpu) < 1.0 * eight["ms_per_step"] * 1e-3 + 0.02
    assert abs(eight["value"] * eight["ms_per_step"] - 8 * 4 * 24 * 0.08 * 1e3) < 1e-3 * eight["value"] * eight["ms_per_step"]
    assert eight["host_threads"]["torch_intra_op"] == 1


def test_plain_run_times_the_steps_and_dumps_the_last_step(tmp_path):
    """Without --full the line carries the headline only (no parity, rooflines, baseline or full record), and --dump-outputs
    writes the last timed step's waveforms: float32 [batch, frames x 1920], the same samples a --full run hashes."""
    r = _run(["--gpus", "1", "--dump-outputs", str(tmp_path)])
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "audio_seconds_per_second" and line["steps"] == 2 and line["dtype"] == "f32" and line["higher_is_better"]
    assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] - 4 * 24 * 0.08 * 1e3) < 1e-3 * line["value"] * line["ms_per_step"]
    assert line["roofline"] is None and line["parity"] is None and line["cpu_baseline"] is None and "full_record" not in line
    assert not any(ln.startswith("[bench full record] ") for ln in r.stderr.splitlines())
    wav = np.load(tmp_path / "waveforms.npy")
    assert wav.dtype == np.float32 and wav.shape == (4, 24 * 1920) and np.isfinite(wav).all()
    hsh = hashlib.sha256()
    for row in wav:
        hsh.update(float_to_pcm16le(torch.from_numpy(row).reshape(1, -1)))
    full = _bench(["--gpus", "1"])
    assert full["parity"]["rank_output_sha16"] == [hsh.hexdigest()[:16]]
