"""Fixture of what the REFERENCE's checkpoint readers (src/sopro/hub.py:30-52: load_cfg_from_safetensors,
load_state_dict_from_safetensors) return for a checkpoint written by ``sopro_amd.weights.save_sopro_checkpoint`` ->
``tests/golden/reference_reader.json``: the config fields the reference read and their values, every tensor's dtype and shape,
and a hash of ``ar.head.weight``.  tests/test_loader.py checks our writer against it.  Needs a checkout of the reference:

    python tests/golden/make_golden_reference_reader.py <reference checkout>/src
"""
import dataclasses
import hashlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from sopro_amd.config import SoproTTSConfig  # noqa: E402
from sopro_amd.weights import save_sopro_checkpoint, synth_sopro_weights  # noqa: E402

VOCAB, SEED = 64, 4  # tests/test_loader.py


def main(ref_src: str) -> None:
    sys.path.insert(0, ref_src)
    from sopro.hub import load_cfg_from_safetensors, load_state_dict_from_safetensors

    cfg = SoproTTSConfig(style_strength=1.25)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "model.safetensors")
        save_sopro_checkpoint(p, synth_sopro_weights(cfg, VOCAB, SEED), cfg)
        rc = load_cfg_from_safetensors(p)
        sd = load_state_dict_from_safetensors(p)
    out = {"what": "the reference's load_cfg_from_safetensors / load_state_dict_from_safetensors on save_sopro_checkpoint("
                   "synth_sopro_weights(SoproTTSConfig(style_strength=1.25), 64, 4)): config fields read, tensors returned",
           "cfg": json.loads(json.dumps(dataclasses.asdict(rc))),
           "tensors": {k: {"dtype": str(v.dtype), "shape": list(v.shape)} for k, v in sorted(sd.items())},
           "ar_head_weight_sha256": hashlib.sha256(sd["ar.head.weight"].contiguous().numpy().tobytes()).hexdigest()}
    path = os.path.join(ROOT, "tests", "golden", "reference_reader.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(f"wrote {path}: {len(out['cfg'])} config fields, {len(out['tensors'])} tensors")


if __name__ == "__main__":
    main(sys.argv[1])
