"""The host arithmetic of the word-timing replay (sopro_amd/replay.py) without a device: the head selection, the window a stream step
replays and the token row it is fed."""
import pytest

from sopro_amd import replay as P

LAYERS = (1, 3, 5)


@pytest.mark.parametrize("heads,masks,n_sel,last", [
    (None, {1: 0xF, 3: 0xF, 5: 0xF}, 12, 5),
    ([(5, 2)], {1: 0, 3: 0, 5: 4}, 1, 5),
    ([(1, 0), (1, 3)], {1: 9, 3: 0, 5: 0}, 2, 1),
])
def test_head_selection(heads, masks, n_sel, last):
    sel = P.select_heads(LAYERS, heads)
    assert sel.layers == LAYERS and dict(sel.masks) == masks and (sel.n_sel, sel.last) == (n_sel, last)
    assert dict(sel.modes) == {1: 0, 3: 1, 5: 2} and sel.weight == 1.0 / n_sel
    with pytest.raises(TypeError):
        sel.masks[1] = 0  # the record is shared between a stream's steps: nothing may edit it
    with pytest.raises(AttributeError):
        sel.last = 0


def test_head_selection_of_one_attention_layer():
    sel = P.select_heads((1,), None)
    assert dict(sel.modes) == {1: 0} and dict(sel.masks) == {1: 0xF} and (sel.n_sel, sel.last) == (4, 1)


@pytest.mark.parametrize("heads,match", [([(2, 0)], "layer must be one of"), ([(1, 4)], "head in"), ([], "selects no head"),
                                         ([3], "wants .layer, head. pairs")])
def test_head_selection_refusals(heads, match):
    with pytest.raises(ValueError, match=match):
        P.select_heads(LAYERS, heads)


def _tars():
    return list(range(1, 60)) + [161, 201, 401]


def test_window_properties_for_every_step_inside_the_opened_chunk():
    n = 0
    for halo in (0, 5, 132):
        for chunk in (1, 6, 16, 63):
            for Tar in _tars():
                Wmax = min(max(16, -(-(halo + chunk) // 8) * 8), max(Tar, 1))
                for t0 in range(Tar):
                    for t1 in range(t0 + 1, min(Tar, t0 + chunk) + 1):
                        ws, W = P.window(t0, t1, halo, Wmax, Tar)  # (a refusal here fails the test: the step is inside the chunk)
                        ok = (0 <= ws <= max(0, t0 - halo) and 1 <= W <= Wmax and ws + W <= Tar and t1 <= ws + W
                              and ((W % 8 == 0 and W >= 16) or ws + W == Tar or W == Wmax))
                        assert ok, (halo, chunk, Tar, t0, t1, ws, W)
                        n += 1
    assert n == 386007


def test_window_refuses_a_step_longer_than_the_chunk():
    halo, chunk, Tar = 132, 6, 401
    Wmax = min(max(16, -(-(halo + chunk) // 8) * 8), Tar)
    assert P.window(200, 206, halo, Wmax, Tar, chunk) == (68, 144)
    with pytest.raises(ValueError, match=r"AlignStream: a step of 20 frames \(opened for 6\)"):
        P.window(200, 220, halo, Wmax, Tar, chunk)


def test_token_row():
    V, bos = 8, 99
    hist = [3, -2, 11, 5, 7, 1, 6]  # (codes outside [0, V - 1]: clamped)
    assert P.token_row(hist, 0, 6, 4, bos, V) == [bos, 3, 0, 7, 5, 0]        # rows 0 .. 5 at t1 = 4: row 5 = frame t1 + 1 is 0
    assert P.token_row(hist, 2, 4, 6, bos, V) == [0, 7, 5, 7]                 # a window past frame 0: no bos, hist[1] = -2 -> 0
    assert P.token_row(hist, 3, 5, 4, bos, V) == [7, 5, 0, 0, 0]              # row t1 still reads frame t1 - 1, everything after is 0
    for ws in range(0, 5):
        for t1 in range(1, 7):
            row = P.token_row(hist, ws, 8 - ws, t1, bos, V)
            for r, v in enumerate(row):
                t = ws + r
                assert v == (bos if t == 0 else (min(max(hist[t - 1], 0), V - 1) if t <= t1 else 0)), (ws, t1, t)
