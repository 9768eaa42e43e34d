"""``sopro_amd.effects`` on the host: the one validator, the refusals, the cue mapping and the chunked chain's control flow (with
fake stages on CPU tensors).  What the stages compute is pinned elsewhere (tests/test_*_host.py, tests/test_gpu_effects.py)."""
import dataclasses

import pytest
import torch

from sopro_amd import Silence, Watermark, effects, hip
from sopro_amd import align as A
from sopro_amd.effects import Chain, Effects

SIL = Silence()
MARK = Watermark(0x0123456789ABCDEF, 17)


# ------------------------------------------------------------------------------------------ Effects
def test_of_raises_what_the_checkers_raise():
    for bad in (dict(speed=2.5), dict(speed="fast"), dict(pitch=13), dict(speed=0.5, pitch=12)):
        with pytest.raises(ValueError) as e:
            Effects.of(**bad)
        with pytest.raises(ValueError) as want:
            hip.prosody_step(bad.get("speed", 1.0), bad.get("pitch", 0.0))
        assert str(e.value) == str(want.value)
    with pytest.raises(TypeError, match="sopro_amd.Silence"):
        Effects.of(silence=0.01)
    with pytest.raises(TypeError, match="sopro_amd.Watermark"):
        Effects.of(watermark=123)
    with pytest.raises(Exception):
        Effects.of().speed = 2.0  # frozen


def test_of_holds_the_values_and_what_they_come_to():
    fx = Effects.of(1.25, -3.0, SIL, MARK)
    assert (fx.speed, fx.pitch, fx.silence, fx.watermark) == (1.25, -3.0, SIL, MARK)
    assert (fx.step, fx.inc) == hip.prosody_step(1.25, -3.0)
    assert Effects.of(1.0, 0.0, None, None).plain and Effects.of().plain
    for one in (dict(speed=1.1), dict(pitch=0.5), dict(silence=SIL), dict(watermark=MARK)):
        assert not Effects.of(**one).plain, one
    rows = dataclasses.replace(fx, watermark=None)  # (how the long-form paths ask for unmarked rows)
    assert rows.watermark is None and (rows.speed, rows.pitch, rows.silence, rows.step, rows.inc) == (1.25, -3.0, SIL, fx.step, fx.inc)
    assert Effects(watermark=MARK) == Effects.of(watermark=MARK) and not Effects(watermark=MARK).plain


def test_per_row():
    assert effects.per_row(1.0, 0.0, None, None, 3) == [Effects.of()] * 3
    assert effects.per_row(1.25, 2.0, SIL, MARK, 2) == [Effects.of(1.25, 2.0, SIL, MARK)] * 2
    got = effects.per_row([1.0, 1.5], 0.0, [SIL, None], [None, MARK], 2)
    assert got == [Effects.of(1.0, 0.0, SIL, None), Effects.of(1.5, 0.0, None, MARK)]
    for bad in (dict(speed=[1.0, 1.0]), dict(pitch=[0.0] * 4), dict(silence=[SIL, None]), dict(watermark=[MARK])):
        kw = dict(speed=1.0, pitch=0.0, silence=None, watermark=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            effects.per_row(rows=3, **kw)
    with pytest.raises(ValueError):
        effects.per_row([1.0, 2.5], 0.0, None, None, 2)
    with pytest.raises(TypeError):
        effects.per_row(1.0, 0.0, [SIL, 7], None, 2)


# ------------------------------------------------------------------------------------------ refuse
def test_refuse():
    effects.refuse("x", speed=1.0, pitch=0.0, watermark=None, silence=None)
    effects.refuse("x")
    for one, word in ((dict(speed=1.5), "speaking-rate"), (dict(pitch=-2.0), "pitch"), (dict(watermark=MARK), "watermark"),
                      (dict(silence=SIL), "silence")):
        with pytest.raises(NotImplementedError) as e:
            effects.refuse("the_path", **one)
        assert "the_path has no " + word in str(e.value) and "mode='batch'" in str(e.value)


# ------------------------------------------------------------------------------------------ map_cues
CUTS = [(0, 240), (12000, 960)]


@pytest.mark.parametrize("speed,pitch,cuts", [(1.0, 0.0, None), (1.25, 0.0, None), (1.0, -3.0, None), (1.0, 0.0, CUTS), (1.25, -3.0, CUTS)],
                         ids=["identity", "stretched", "shifted", "cut", "all"])
def test_map_cues_is_the_composition(speed, pitch, cuts):
    words = [A.WordCue("a", 0, 1, 0, 5760), A.WordCue("bc", 2, 4, 5760, 13440), A.WordCue("d", 5, 6, 13440, 21120)]
    fx = Effects.of(speed, pitch)
    want = words
    if speed != 1.0 or pitch != 0.0:  # (a pitch stretches at its own step before it resamples)
        want = A.stretch_cues(want, fx.step)
    if pitch != 0.0:
        want = A.shift_cues(want, fx.inc)
    if cuts is not None:
        want = A.squeeze_cues(want, cuts)
    got = effects.map_cues(words, fx, cuts)
    assert got == want
    if fx.plain and cuts is None:
        assert got is words
    else:
        assert got != words


# ------------------------------------------------------------------------------------------ Chain
class Blocks:
    """A fake stage: applies ``op`` and emits only whole blocks of ``k`` samples, holding the rest until flushed."""

    def __init__(self, k, op, log, name):
        self.k, self.op, self.log, self.name = k, op, log, name
        self.held = torch.zeros(1, 0)

    def feed(self, wav, flush=False):
        self.log.append((self.name, 0 if wav is None else int(wav.shape[-1]), flush))
        if wav is not None:
            self.held = torch.cat([self.held, self.op(wav)], dim=1)
        n = int(self.held.shape[1]) if flush else int(self.held.shape[1]) // self.k * self.k
        out, self.held = self.held[:, :n], self.held[:, n:]
        return out, [n]


def _chain(log):
    return Chain([Blocks(480, lambda w: w + 1.0, log, "one"), Blocks(700, lambda w: w * 2.0, log, "two")])


@pytest.mark.parametrize("chunks", [[1920] * 5, [100, 3000, 1, 6499], [9600]])
def test_chain_is_the_one_shot_result_in_any_chunking(chunks):
    x = torch.arange(9600, dtype=torch.float32).reshape(1, -1)
    log: list = []
    chain = _chain(log)
    got, at = [], 0
    for n in chunks:
        before = len(log)
        out = chain.feed(x[:, at: at + n])
        at += n
        calls = log[before:]
        assert calls[0] == ("one", n, False)
        held_before = sum(c[1] for c in log[:before] if c[0] == "one") % 480
        ready = (held_before + n) // 480 * 480
        # (stage one yields nothing: stage two is not called, and the step yields nothing)
        assert calls[1:] == ([("two", ready, False)] if ready else [])
        if not ready:
            assert out is None
        if out is not None:
            got.append(out)
    before = len(log)
    assert chain.feed(None) is None and chain.feed(x[:, :0]) is None and len(log) == before  # (no stage is called)
    out = chain.flush()
    rest = 9600 - sum(c[1] for c in log[:before] if c[0] == "two")  # what stage one still holds
    # the flush: stage one first, then its output goes into stage two's flushing call
    assert log[before:] == [("one", 0, True), ("two", rest, True)]
    if out is not None:
        got.append(out)
    assert torch.equal(torch.cat(got, dim=1), (x + 1.0) * 2.0)
    assert all(int(g.shape[1]) > 0 for g in got)


def test_chain_without_stages_and_with_a_dry_flush():
    x = torch.arange(10, dtype=torch.float32).reshape(1, -1)
    empty = Chain([])
    assert empty.feed(x) is x and empty.feed(None) is None and empty.flush() is None
    log: list = []
    chain = _chain(log)
    assert chain.flush() is None  # (nothing was fed: every stage is still flushed, in order)
    assert log == [("one", 0, True), ("two", 0, True)]
    assert Chain.of(Effects.of(), "cpu").stages == []  # (no stage has work: nothing is built, nothing needs a device)
