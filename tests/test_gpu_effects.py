"""``sopro_amd.effects`` on the device: the one-shot chain and the chunked chain over a ragged, mixed batch against the numpy
restatements of its stages composed per row (tests/pitch_ref.py, sil_ref.py, wm_ref.py).  Everything is compared exactly."""
import numpy as np
import pytest
import torch

import pitch_ref as P
import sil_ref as S
import wm_ref as W
from sopro_amd import Silence, Watermark, effects, hip
from sopro_amd.effects import Chain, Effects

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEY, TAG = 0x0123456789ABCDEF, 17
SIL = Silence(max_pause_ms=300, onset_ms=30, floor=0.01)
FXS = [Effects.of(1.25, -3.0, SIL, Watermark(key=KEY, tag=TAG)), Effects.of(silence=SIL), Effects.of()]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _counters():
    return (hip.tsm_calls, hip.pitch_calls, hip.sil_calls, hip.wm_calls())


@pytest.fixture(scope="module")
def batch():
    """The three rows, their restated results, and the one-shot result on the device, made once."""
    xs = [S.bursts([("g", 6), ("s", 20), ("g", 45), ("s", 30), ("g", 9)], tail=131, amp=0.3, seed=11),
          S.bursts([("s", 25), ("g", 40), ("s", 15)], tail=1, amp=0.3, seed=12),
          S.bursts([("s", 4)], amp=0.3, seed=13)]
    assert [len(x) for x in xs] == [26531, 19201, 960]
    y0 = P.chain(xs[0], 1.25, -3.0)
    assert len(y0) == 21223
    y0, c0 = S.squeeze(y0, np.float32(0.01), 30, 3)
    assert len(y0) == 20023 and c0 == [(0, 240), (12000, 960)]
    y0 = W.embed(y0, KEY, TAG, -30.0)
    y1, c1 = S.squeeze(xs[1], np.float32(0.01), 30, 3)
    assert len(y1) == 16801 and c1 == [(12480, 2400)]
    wav = torch.full((3, max(len(x) for x in xs) + 5), 777.0)  # (past a row's length: must never reach the output)
    for b, x in enumerate(xs):
        wav[b, : len(x)] = torch.from_numpy(x)
    wav = wav.to(DEV)
    before = _counters()
    out, lens, cuts = effects.apply(wav, [len(x) for x in xs], FXS)
    torch.cuda.synchronize()
    moved = tuple(a - b for a, b in zip(_counters(), before))
    return dict(xs=xs, want=[y0, y1, xs[2]], want_cuts=[c0, c1, []], wav=wav, out=out, lens=lens, cuts=cuts, moved=moved)


def test_one_shot_is_the_restatements_composed(batch):
    assert batch["moved"] == (1, 1, 1, 1)  # every stage was called once for the whole batch
    assert batch["lens"] == [len(y) for y in batch["want"]] == [20023, 16801, 960]
    assert [[tuple(c) for c in row] for row in batch["cuts"]] == batch["want_cuts"]
    for b, y in enumerate(batch["want"]):
        got = batch["out"][b, : batch["lens"][b]].cpu()
        assert torch.equal(_bits(got), _bits(torch.from_numpy(y))), b
    assert torch.equal(_bits(batch["out"][2, :960]), _bits(batch["wav"][2, :960]))  # the plain row, bit for bit


def test_all_plain_batch_is_handed_back(batch):
    before = _counters()
    out, lens, cuts = effects.apply(batch["wav"], [len(x) for x in batch["xs"]], [Effects.of()] * 3)
    assert _counters() == before and cuts is None and lens == [26531, 19201, 960]
    assert out.data_ptr() == batch["wav"].data_ptr() and torch.equal(_bits(out), _bits(batch["wav"][:, : out.shape[1]]))


@pytest.mark.parametrize("chunks", [[11520, 1920, 480, 5000, None], [None]], ids=["chunked", "one-chunk"])
def test_chain_is_row_zero_of_the_one_shot_result(batch, chunks):
    x = batch["wav"][0:1, :26531]
    chain = Chain.of(FXS[0], DEV)
    assert len(chain.stages) == 4
    got, at = [], 0
    for n in chunks:
        n = 26531 - at if n is None else n
        out = chain.feed(x[:, at: at + n])
        at += n
        if out is not None:
            got.append(out.clone())
    assert at == 26531
    out = chain.flush()
    if out is not None:
        got.append(out)
    got = torch.cat(got, dim=1)
    assert tuple(got.shape) == (1, 20023)
    assert torch.equal(_bits(got[0]), _bits(batch["out"][0, :20023]))
    assert [tuple(c) for c in chain.stages[2].cuts[0]] == batch["want_cuts"][0]
