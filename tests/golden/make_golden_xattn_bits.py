"""Bit pin for sopro_xattn_step_f32: ``tests/golden/xattn_step_bits.npz`` holds the outputs Y [H, B, D] of every form of the
one-launch cross-attention block (folded / unfolded keys, fp32 / bf16 storage, cached and non-temporal loads) on the cases listed
in ``tests/test_gpu_attention.py::xattn_golden_outputs``, as written by the library built from the commit BEFORE rows without keys
(klens[b] == 0) were given a defined result.  ``test_xattn_step_outputs_with_keys_are_bit_identical_to_the_recorded_ones`` compares
the current library against them bit for bit; the operands are integer-valued fractions made without any library generator, so the
same bits come out on every host.

Regenerate only when a change is MEANT to move these outputs.  Needs an MI355X and a built library.
Usage:  python tests/golden/make_golden_xattn_bits.py
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np

import test_gpu_attention as T


def main() -> None:
    out = T.xattn_golden_outputs()
    again = T.xattn_golden_outputs()
    for name, y in out.items():
        assert np.isfinite(y).all(), name
        assert np.array_equal(y.view(np.uint32), again[name].view(np.uint32)), f"{name}: not reproducible run to run"
    np.savez_compressed(os.path.join(HERE, "xattn_step_bits.npz"), **out)
    print("wrote xattn_step_bits.npz:", ", ".join(sorted(out)))


if __name__ == "__main__":
    main()
