"""Batched streaming on the host side, without a GPU: the C ABI of the batched stream decoder state (layout, sizes, refusals made
before any launch) and the lockstep chunk schedule of stream_batch against a restatement of the reference's streaming loop."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from sopro_amd import hip
from sopro_amd.streaming import step_plan, stream_schedule


@pytest.fixture(scope="module")
def cpu_engine():
    """An engine handle with the default configs and no tensors (sopro_engine_create touches no device)."""
    from sopro_amd.stages import _cfg_of

    lib = hip.load()
    cfg = _cfg_of(None, None, "f32")
    h = ctypes.c_void_p()
    assert lib.sopro_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    yield lib, h, cfg
    lib.sopro_engine_destroy(h)


def test_batch_state_layout_matches_the_header(tmp_path):
    fields = ["kv", "rows_cap", "rows", "cap_rows", "kv_len", "pos", "evict", "half"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "sopro_hip.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(sopro_mimi_stream_batch));']
    lines += [f'printf("{f} %zu\\n", offsetof(sopro_mimi_stream_batch, {f}));' for f in fields]
    lines += ['printf("max %d\\n", SOPRO_MIMI_STREAM_BATCH_MAX_ROWS);', "return 0;}"]
    src = tmp_path / "sb.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "sb"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(hip.MimiStreamBatch)
    for f in fields:
        assert int(got[f]) == getattr(hip.MimiStreamBatch, f).offset, f
    assert int(got["max"]) == 64
    assert hip.ABI_VERSION == 43 and hip.load().sopro_abi_version() == 43


def test_batch_kv_bytes(cpu_engine):
    lib, h, cfg = cpu_engine
    per_row = cfg.mimi_layers * 2 * 1024 * 2 * cfg.mimi_hidden * 4
    assert per_row == 64 << 20  # 8 layers x 2 halves x 1024 rows x 4 KB
    assert lib.sopro_mimi_stream_batch_kv_bytes(h, 1, 1024) == per_row
    assert lib.sopro_mimi_stream_batch_kv_bytes(h, 32, 1024) == 32 * per_row
    assert lib.sopro_mimi_stream_batch_kv_bytes(h, 3, 4096) == 3 * 4 * per_row
    # one row is the single-stream state's size
    assert lib.sopro_mimi_stream_batch_kv_bytes(h, 1, 777) == lib.sopro_mimi_stream_kv_bytes(h, 777)
    assert lib.sopro_mimi_stream_batch_kv_bytes(h, 0, 1024) == 0 and lib.sopro_mimi_stream_batch_kv_bytes(h, 2, 0) == 0


def test_batch_init_refusals(cpu_engine):
    lib, h, cfg = cpu_engine
    st = hip.MimiStreamBatch()
    fake = 1 << 20  # a 16-byte aligned address that is never dereferenced: init only records it
    for rows, cap, msg in [(0, 1024, b"rows"), (65, 1024, b"rows"), (2, int(cfg.mimi_window) - 1, b"window")]:
        assert lib.sopro_mimi_stream_batch_init(h, ctypes.byref(st), fake, rows, cap) == -2
        assert msg in lib.sopro_last_error()
    assert lib.sopro_mimi_stream_batch_init(h, ctypes.byref(st), fake, 64, int(cfg.mimi_window)) == 0
    assert (st.rows, st.rows_cap, st.kv_len, st.pos, st.evict, st.half) == (64, 64, 0, 0, 1, 0)
    assert lib.sopro_mimi_stream_batch_init(h, ctypes.byref(st), None, 2, 1024) == -2


def test_batch_keep_refusals_and_trim(cpu_engine):
    lib, h, _cfg = cpu_engine
    st = hip.MimiStreamBatch()
    assert lib.sopro_mimi_stream_batch_init(h, ctypes.byref(st), 1 << 20, 4, 1024) == 0

    def keep(*idx):
        arr = (ctypes.c_int32 * max(1, len(idx)))(*idx)
        return lib.sopro_mimi_stream_batch_keep(h, ctypes.byref(st), arr, len(idx), None)

    for idx, msg in [((2, 1), b"increasing"), ((1, 1), b"increasing"), ((0, 4), b"out of range"), ((-1,), b"out of range"),
                     ((), b"n_keep"), ((0, 1, 2, 3, 3), b"n_keep")]:
        assert keep(*idx) == -2, idx
        assert msg in lib.sopro_last_error(), (idx, lib.sopro_last_error())
    assert st.rows == 4 and st.half == 0
    # kv_len == 0: nothing to move, no launch - only the live count changes
    assert keep(0, 2) == 0 and st.rows == 2 and st.half == 0 and st.rows_cap == 4
    assert keep(0, 1) == 0 and st.rows == 2  # the identity
    # legacy policy: as sopro_mimi_stream_trim
    st.kv_len, st.pos = 300, 320
    assert lib.sopro_mimi_stream_batch_trim(ctypes.byref(st), 2) == 0
    assert (st.kv_len, st.pos, st.evict) == (298, 298, 0)
    assert lib.sopro_mimi_stream_batch_trim(ctypes.byref(st), -1) == -2


def test_decode_stream_batch_refuses_a_null_state(cpu_engine):
    lib, h, _cfg = cpu_engine
    assert lib.sopro_mimi_decode_stream_batch(h, None, None, None, 4, None, None) == -2
    assert b"state is NULL" in lib.sopro_last_error()
    st = hip.MimiStreamBatch()
    assert lib.sopro_mimi_stream_batch_init(h, ctypes.byref(st), 1 << 20, 2, 1024) == 0
    # an engine without the decoder's tensors is refused before anything is launched
    assert lib.sopro_mimi_decode_stream_batch(h, 1 << 20, ctypes.byref(st), 1 << 20, 4, 1 << 20, None) == -2


def _reference_chunks(L, cf, nar_ctx):
    """Restatement of the reference's loop (src/sopro/streaming.py:81-131) for a row whose history ends at L frames (first EOS):
    -> [(win_start, new_start, end)] of every yielded chunk."""
    out, emitted = [], 0

    def refine_and_emit(end):
        nonlocal emitted
        if end <= emitted:
            return
        out.append((max(0, emitted - nar_ctx), emitted, end))
        emitted = end

    for T in range(1, L + 1):
        if T % cf == 0:
            refine_and_emit(T)
    if emitted < L:
        refine_and_emit(L)
    return out


@pytest.mark.parametrize("cf", [1, 6, 16])
def test_chunk_schedule_matches_the_reference_loop(cf):
    rng = np.random.default_rng(cf)
    n_frames, nar_ctx = 101, 9
    for trial in range(40):
        B = int(rng.integers(1, 9))
        lens = [int(x) for x in rng.integers(0, n_frames + 1, size=B)]
        if trial == 0:  # EOS at frame 0, on a chunk boundary, mid-chunk, never
            lens = [0, 2 * cf, 2 * cf + max(1, cf // 2) if cf > 1 else 5, n_frames]
        steps = stream_schedule(lens, cf, nar_ctx, n_frames)
        for b, L in enumerate(lens):
            got = [(s["ws"], s["t0"], s["ends"][b]) for s in steps if s["ends"][b] is not None]
            assert got == _reference_chunks(L, cf, nar_ctx), (cf, lens, b)
        # lockstep: every step's rows start at the same frame and share the window start
        for s in steps:
            assert s["ws"] == max(0, s["t0"] - nar_ctx) and s["t1"] - s["t0"] <= cf
            assert all(e is None or s["t0"] < e <= s["t1"] for e in s["ends"])


def test_step_plan_of_one_step():
    assert step_plan(12, 18, [None, 15, 12, 18], 4) == (8, [18, 15, None, 18])
    assert step_plan(0, 6, [None, 0], 40) == (0, [6, None])
