"""Which cross-attention heads carry the alignment?  Per-(layer, head) sharpness of a checkpoint, for picking ``align_heads``.

Word timestamps average the attention maps of the AR generator's text cross-attention (layers ``cfg.ar_xattn_layers``, 4 heads each)
and look for the best monotonic path through the result.  How sharp and how monotonic those heads are depends on the checkpoint.
This tool synthesises one utterance with a fixed seed, once per (layer, head) pair and once with all of them, and prints for each:

    mean max p   mean over the frames of the largest attention probability (1 / S for a flat map, 1.0 for a one-hot one)
    monotone     share of frames whose arg-max text position is not behind the previous frame's
    confidence   exp(path score / frames): the geometric mean of the probability along the best monotonic path

    python tools/align_probe.py CHECKPOINT_DIR "Some text to speak." --ref-audio voice.wav
    python tools/align_probe.py CHECKPOINT_DIR "Some text." --ref-tokens voice_tokens.npy     # [T, Q] codec tokens
    python tools/align_probe.py --synthetic "Some text."                                      # the synthetic test checkpoint

Pick the pairs that are sharp AND monotone and pass them as ``align_heads=[(layer, head), ...]``.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("checkpoint", nargs="?", help="directory with model.safetensors, tokenizer files and mimi/ (omit with --synthetic)")
    ap.add_argument("text")
    ap.add_argument("--ref-audio", default=None)
    ap.add_argument("--ref-tokens", default=None, help=".npy of [T, Q] codec tokens")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--max-frames", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from sopro_amd import SoproTTS

    if a.synthetic:
        from sopro_amd.config import MimiDecoderConfig, SoproTTSConfig
        from sopro_amd.weights import synth_mimi_weights, synth_sopro_weights

        class Tok:
            vocab_size = 512

            def encode(self, text):
                return [1 + (ord(c) % 500) for c in text]

        cfg, mc = SoproTTSConfig(), MimiDecoderConfig()
        tts = SoproTTS.from_weights(cfg, synth_sopro_weights(cfg, 512, 1234, suppress_eos=True), synth_mimi_weights(mc, 1234), Tok(), device="cuda:0")
        ref = tts.prepare_reference(ref_tokens_tq=torch.from_numpy(np.random.default_rng(5).integers(0, 2048, size=(24, 32))))
        a.max_frames = min(a.max_frames, 2 * len(a.text) + 8)
    else:
        if a.checkpoint is None or (a.ref_audio is None) == (a.ref_tokens is None):
            ap.error("give a checkpoint directory and exactly one of --ref-audio / --ref-tokens")
        tts = SoproTTS.from_pretrained(a.checkpoint, device="cuda:0")
        toks = torch.from_numpy(np.load(a.ref_tokens)) if a.ref_tokens else None
        ref = tts.prepare_reference(ref_audio_path=a.ref_audio, ref_tokens_tq=toks)
    pairs = [(int(l), h) for l in tts.cfg.ar_xattn_layers for h in range(4)]
    print(f"{'heads':>12} | mean max p | monotone | confidence | status")
    for sel in [None] + [[p] for p in pairs]:
        sink = []
        tts.synthesize_batch([a.text], [ref], max_frames=a.max_frames, seed=a.seed, alignment=sink, align_heads=sel)
        al = sink[0]
        T, S = len(al.path), len(al.token_frames)
        if T == 0:
            print("the utterance has no frames")
            return
        prob = tts.model.align_last[0, :T, :S].exp().cpu()
        peak = prob.max(dim=-1)
        mono = float((peak.indices[1:] >= peak.indices[:-1]).float().mean()) if T > 1 else 1.0
        name = "all" if sel is None else f"({sel[0][0]}, {sel[0][1]})"
        print(f"{name:>12} | {float(peak.values.mean()):10.4f} | {mono:8.3f} | {al.confidence:10.4f} | {al.status}")
    print(f"{T} frames, {S} text positions: a flat map has max p = confidence = {1.0 / S:.4f}")


if __name__ == "__main__":
    main()
