"""Word timestamps, device side (DESIGN.md "Word timestamps"; ``sopro_amd/align.py`` is the host half): the AR stack is replayed
teacher-forced over the generated codebook-0 tokens, and the text cross-attention's queries and keys become alignment scores.

``walk`` is the one place where the replay's launch sequence is written down.  ``align_batch`` runs it over a finished AR phase and
finds the best monotonic path per row; ``AlignStream`` runs it window by window while an utterance is generated, so its score rows
equal ``align_batch``'s bit for bit.  ``select_heads``, ``window`` and ``token_row`` are the host arithmetic of the two.
"""
from __future__ import annotations

from collections import namedtuple
from types import MappingProxyType
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import torch

from . import hip
from .align import Alignment, check_align_window
from .model import RMS_EPS


# The heads whose maps are averaged.  masks: head mask per attention layer; last: the last layer with a selected head (nothing after
# its queries is needed); modes: hip.align_scores' mode per layer (0 writes, 1 adds, 2 adds and finishes); weight = 1 / n_sel.
HeadSelection = namedtuple("HeadSelection", "layers masks n_sel last modes weight")
Scratch = namedtuple("Scratch", "tok xa xb n g f q att")  # the replay's buffers: token rows, x / y, norm, GLU, ff, queries, attention


def select_heads(layers: Sequence[int], heads) -> HeadSelection:
    """(layer, head) pairs -> ``HeadSelection``; ``None``: every head of every attention layer in ``layers`` (no device needed)."""
    layers = tuple(int(i) for i in layers)
    if heads is None:
        masks = {i: 0xF for i in layers}
    else:
        masks = {i: 0 for i in layers}
        for pair in heads:
            try:
                l, h = (int(v) for v in pair)
            except (TypeError, ValueError):
                raise ValueError(f"align_heads wants (layer, head) pairs, got {pair!r}") from None
            if l not in masks or not 0 <= h < 4:
                raise ValueError(f"align_heads: layer must be one of {layers} and head in [0, 4), got {(l, h)}")
            masks[l] |= 1 << h
        if not any(masks.values()):
            raise ValueError("align_heads selects no head")
    n_sel = sum(bin(v).count("1") for v in masks.values())
    modes = {i: (0 if n == 0 else (2 if n == len(layers) - 1 else 1)) for n, i in enumerate(layers)}
    return HeadSelection(layers, MappingProxyType(masks), n_sel, max(i for i in layers if masks[i]), MappingProxyType(modes), 1.0 / n_sel)


def window(t0: int, t1: int, halo: int, Wmax: int, Tar: int, chunk: Optional[int] = None) -> Tuple[int, int]:
    """The rows [ws, ws + W) a stream step replays to score frames [t0, t1): ``halo`` frames of left context, W a multiple of 8 and at
    least 16 (from 16 query rows on the cross-attention runs on one kernel, the one ``align_batch`` has), at most ``Wmax`` (sized at
    open for steps of ``chunk`` frames; only the refusal names it) and inside the ``Tar`` rows of the conditioning."""
    ws = max(0, t0 - halo)
    W = min(max(16, -(-(t1 - ws) // 8) * 8), Wmax)
    if ws + W > Tar:  # (the padding rows must be rows of the conditioning: more left context instead)
        ws = max(0, Tar - W)
        W = Tar - ws
    if t1 - ws > W:
        raise ValueError(f"AlignStream: a step of {t1 - t0} frames (opened for {chunk})")
    return ws, W


def token_row(hist: Sequence[int], ws: int, W: int, t1: int, bos: int, V: int) -> List[int]:
    """The tokens rows [ws, ws + W) are fed: ``bos`` at frame 0, else the previous frame's code clamped to [0, V - 1]; 0 for the
    padding rows past t1 (the causal stack never looks back from them)."""
    return [bos if t == 0 else (min(max(int(hist[t - 1]), 0), V - 1) if t - 1 < t1 else 0) for t in range(ws, ws + W)]


def operands(model) -> Dict[str, Any]:
    """The AR stack's weights in the layouts of the full-sequence operators (made once per model, at the first timed call, and kept on
    it: the lanes of ``clone_lane`` share them, read-only): the GLU projection packed per 64 rows as the contraction's gating epilogue
    reads it (pack.pack_glu; the engine keeps the natural layout for the frame kernels), everything else as it is.  The RMSNorm
    weights are folded into the projections that follow (pack.py), so the norms of the replay run with a vector of ones."""
    ops = getattr(model, "_align_ops", None)
    if ops is None:
        from .pack import pack_glu

        w, dev = model.w, model.device
        zero = dict(dtype=torch.int32, device=dev)
        ops = {"ones": torch.ones(model.D, device=dev), "col": torch.tensor([0], **zero), "off": torch.tensor([0], **zero),
               "wq": torch.ones(1, device=dev)}
        for i in range(len(model.cfg.ar_dilations)):
            ops[f"glu.{i}"] = tuple(t.contiguous() for t in pack_glu(w[f"ar.blocks.{i}.glu.w"], w[f"ar.blocks.{i}.glu.b"]))
        model._align_ops = ops
    return ops


def _scratch(model, prefix: str, B: int, T: int) -> Scratch:
    """The replay's scratch for B x T rows from the model's workspace: ``align.`` for the batch form, ``align.s_`` for a stream."""
    get, M, D = model.ws.get, B * T, model.D
    return Scratch(get(prefix + "tok", (B, T), dtype=torch.int32), get(prefix + "xa", (M, D)), get(prefix + "xb", (M, D)),
                   get(prefix + "n", (M, D)), get(prefix + "g", (M, D)), get(prefix + "f", (M, 4 * D)), get(prefix + "q", (M, D)),
                   get(prefix + "att", (M, D)))


def text_keys(model, i: int, ts: torch.Tensor, nkv: torch.Tensor, kv: torch.Tensor) -> torch.Tensor:
    """Attention layer i's keys (and values) of the text rows ``ts`` into ``kv`` (``nkv``: scratch of ``ts``' shape)."""
    pa, rows, D = f"ar.x_attns.{i}", int(ts.shape[0]), model.D
    hip.norm(ts, nkv, model.w[pa + ".nkv.weight"], rows=rows, C_=D, eps=RMS_EPS)
    hip.gemm(nkv, model.w[pa + ".kv.w"], kv, M=rows, N=2 * D, K=D)
    return kv


def walk(model, sel: HeadSelection, s: Scratch, keys: Callable[[int], torch.Tensor], B: int, T: int, S: int, tl: torch.Tensor,
         sl: torch.Tensor, acc: torch.Tensor, q_off: int = 0) -> None:
    """The AR stack teacher-forced over B x T rows (oracle ``ar_forward_teacher`` without the head), on the current stream: ``s.tok``
    and the conditioning rows in ``s.xb`` become x, the blocks run up to the last selected attention layer's queries, and every
    attention layer's queries (from element ``q_off`` on) and text keys add its share of the scores into ``acc``.  ``keys(i)``
    is called where layer i's keys are needed and returns them, [B, S, 2 D]; ``tl`` / ``sl``: frames and text positions per row."""
    cfg, w, D, ops = model.cfg, model.w, model.D, operands(model)
    M, ksz, ones = B * T, int(cfg.ar_kernel), ops["ones"]
    nb, g, f, q, att = s.n, s.g, s.f, s.q, s.att
    geom = dict(H=4, ldq=D, ldk=2 * D, q_bstride=T * D, k_bstride=S * 2 * D, q_off=q_off)
    hip.codebook_sum(s.tok, 1, ops["col"], ops["off"], ops["wq"], w["cb_embed"], s.xa, rows=M, D=D, base=s.xb, alpha=1.0, beta=1.0)
    x, y = s.xa, s.xb
    kv = None
    for i, dil in enumerate(cfg.ar_dilations):
        p = f"ar.blocks.{i}"
        gw, gb = ops[f"glu.{i}"]
        hip.norm(x, nb, ones, rows=M, C_=D, eps=RMS_EPS)
        hip.gemm(nb, gw, g, M=M, N=2 * D, K=D, bias=gb, epilogue=hip.EPI_GLU)
        hip.dwconv(g, w[p + ".dw.w"], w[p + ".dw.b"], y, B=B, T=T, C_=D, ksize=ksz, dil=int(dil), left=(ksz - 1) * int(dil), mode=1, res=x)
        hip.norm(y, nb, ones, rows=M, C_=D, eps=RMS_EPS)
        hip.gemm(nb, w[p + ".ff1.w"], f, M=M, N=4 * D, K=D, bias=w[p + ".ff1.b"], epilogue=hip.EPI_GELU)
        hip.gemm(f, w[p + ".ff2.w"], x, M=M, N=D, K=4 * D, bias=w[p + ".ff2.b"], epilogue=hip.EPI_RES, R=y)
        if i not in sel.masks:
            continue
        pa = f"ar.x_attns.{i}"
        kv = keys(i)
        hip.norm(x, nb, ones, rows=M, C_=D, eps=RMS_EPS)
        hip.gemm(nb, w[pa + ".qa.w"], q, M=M, N=D, K=D)  # (qa.w = q_proj with RMSNorm_nq's weight folded in)
        hip.align_scores(q, kv, tl, sl, acc, head_mask=sel.masks[i], weight=sel.weight, mode=sel.modes[i], **geom)
        if i == sel.last:
            break
        hip.attention(q, kv, kv, att, B=B, H=4, dh=D // 4, Tq=T, Tk=S, ldq=D, ldk=2 * D, ldv=2 * D, ldo=D, q_bstride=T * D,
                      k_bstride=S * 2 * D, v_bstride=S * 2 * D, o_bstride=T * D, klens=sl, v_off=D)
        hip.gemm(att, w[pa + ".o.w"], y, M=M, N=D, K=D, epilogue=hip.EPI_RES, R=x, scale=w[pa + ".gate_scale"])
        x, y = y, x
    for i in sel.layers:  # the layers past the last selected one add nothing; the last launch still finishes the scores
        if i > sel.last:
            hip.align_scores(q, kv, tl, sl, acc, head_mask=0, weight=0.0, mode=sel.modes[i], **geom)
    if len(sel.layers) == 1:  # (one attention layer: its launch wrote the sum, a second one finishes it)
        hip.align_scores(q, kv, tl, sl, acc, head_mask=0, weight=0.0, mode=2, **geom)


@torch.inference_mode()
def align_batch(model, prep: Dict[str, Any], state: Dict[str, Any], heads=None) -> List[Alignment]:
    """A post-pass over a finished AR phase: ``walk`` over all frames at once on the generated codebook-0 tokens, then
    ``sopro_align_dp_f32`` finds each row's best monotonic path -> one ``Alignment`` per row, in frames.  Runs on the bulk stream;
    ``prep`` (conditioning: ``txt_seq``, ``text_lens_host``) and ``state`` (phase_ar: ``cond_ar``, ``hist``, ``lens``) are only
    read.  ``heads``: the (layer, head) pairs to average, default all 12.  The score matrix of the last call stays in
    ``model.align_last`` ([B, T, S] on the device, valid until the next call)."""
    cfg, dev, D = model.cfg, model.device, model.D
    sel = select_heads(cfg.ar_xattn_layers, heads)
    lens_t = [int(n) for n in state["lens"]]
    lens_s = [int(n) for n in prep["text_lens_host"]]
    B, S = int(state["B"]), int(prep["txt_seq"].shape[1])
    hist, cond = state["hist"], state["cond_ar"]
    Tp = min(max(8, -(-max(lens_t) // 8) * 8), int(hist.shape[1]), int(cond.shape[1]))
    operands(model)  # (made on the caller's stream, which the bulk stream then waits for)
    o_bounds, o_total, o_status = B * Tp, B * Tp + 2 * B * S, B * Tp + 2 * B * S + B  # path | bounds | total | status: one download

    def parts(out):
        return out[:o_bounds].view(B, Tp), out[o_bounds:o_total].view(B, S, 2), out[o_total:o_status].view(torch.float32), out[o_status:]

    get = model.ws.get
    with model.on_stream(bulk=True):
        lens_d = torch.tensor([lens_t, lens_s], dtype=torch.int32).to(dev)
        tl, sl = lens_d[0], lens_d[1]
        s = _scratch(model, "align.", B, Tp)
        s.tok[:, 0] = int(cfg.bos_row)
        if Tp > 1:
            s.tok[:, 1:] = hist[:, : Tp - 1].clamp(0, model.V - 1)  # (codes past a row's own length are never used: the stack is causal)
        s.xb.view(B, Tp, D).copy_(cond[:, :Tp])
        acc = get("align.acc", (B, Tp, S))
        ts = prep["txt_seq"].to(dev).float().contiguous().view(B * S, D)
        nkv, kv = get("align.nkv", (B * S, D)), get("align.kv", (B * S, 2 * D))
        walk(model, sel, s, lambda i: text_keys(model, i, ts, nkv, kv), B, Tp, S, tl, sl, acc)
        dws = get("align.dp_ws", (max(1, int(hip.load().sopro_align_ws_bytes(B, Tp, S)) // 8),), dtype=torch.int64)
        out = get("align.out", (o_status + B,), dtype=torch.int32)
        out.zero_()
        path, bounds, total, status = parts(out)
        hip.align_paths(acc, tl, sl, path=path, bounds=bounds, total=total, status=status, ws=dws)
        host = out.cpu()
    model.align_last = acc
    hp, hb, ht, hs = (t.tolist() for t in parts(host))
    return [Alignment(path=hp[b][: lens_t[b]], token_frames=[tuple(v) for v in hb[b][: lens_s[b]]], total=float(ht[b]), status=int(hs[b]))
            for b in range(B)]


class AlignStream:
    """``align_batch`` for a stream (DESIGN.md "Word timestamps", online form).  At open the text keys of every attention layer in
    use are computed once.  ``step(hist, t1, final)`` runs ``walk`` over the rows ``window`` gives, [ws, ws + W) with
    ws = max(0, t0 - (rf_ar - 1)) and t0 the frames scored so far - exact for the rows from t0 on, because the causal depthwise
    convolution is the stack's only temporal operator -, writes the score rows [t0, t1) into a persistent [1, max_frames + 1, S]
    buffer (``sopro_align_scores_f32`` with the queries offset to row t0 - ws), runs one ``sopro_align_online_f32`` step and downloads
    the row's state and path.  Everything is queued on the model's bulk stream; a step's scratch comes from the model's workspace
    under ``align.s_*`` names (a step ends with a download, so no step reads another's), the score buffer, the text keys and the
    state belong to the stream object."""

    def __init__(self, model, prep: Dict[str, Any], *, max_frames: int, lag_frames: int, chunk_frames: int, heads=None):
        check_align_window(lag_frames, chunk_frames)
        m, cfg, dev, D = model, model.cfg, model.device, model.D
        self.m, self.lag, self.chunk = m, int(lag_frames), int(chunk_frames)
        self.sel = select_heads(cfg.ar_xattn_layers, heads)
        Sp = int(prep["txt_seq"].shape[1])
        self.S = int(prep["text_lens_host"][0]) if prep.get("text_lens_host") is not None else Sp  # (one utterance's prep: no padding)
        if int(prep["txt_seq"].shape[0]) != 1 or not 1 <= self.S <= Sp or Sp > hip.ALIGN_S_MAX:
            raise ValueError(f"AlignStream: one utterance of 1..{hip.ALIGN_S_MAX} text positions, got {tuple(prep['txt_seq'].shape)}")
        self.Sp, self.cond = Sp, prep["cond_ar"]
        self.Tar = min(int(max_frames) + 1, int(self.cond.shape[1]))
        self.halo = int(cfg.rf_ar()) - 1
        self.Wmax = min(max(16, -(-(self.halo + self.chunk) // 8) * 8), max(self.Tar, 1))
        operands(m)  # (made on the caller's stream, which the bulk stream then waits for)
        self.t0, self.c = 0, -1  # frames scored; frames committed - 1 (the device's ``c`` as of the last download)
        self.state_host, self.base, self.path = (-1, -1, 0, 0), 0.0, []
        Tar = self.Tar
        with m.on_stream(bulk=True):
            self.scratch = _scratch(m, "align.s_", 1, self.Wmax)
            # what lives as long as the stream is the stream's own: a later stream of this engine cannot write into it
            self.acc = torch.empty(1, Tar, Sp, device=dev)
            self.out = torch.tensor([-1, -1, 0, 0, 0] + [0] * Tar, dtype=torch.int32).to(dev)  # state | path: one download
            self.state = self.out[: hip.ALIGN_STATE_WORDS].view(1, hip.ALIGN_STATE_WORDS)
            self.pathd = self.out[hip.ALIGN_STATE_WORDS:].view(1, Tar)
            ts = prep["txt_seq"].to(dev).float().contiguous().view(Sp, D)
            nkv = m.ws.get("align.s_nkv", (Sp, D))
            self.kv = {i: text_keys(m, i, ts, nkv, torch.empty(Sp, 2 * D, device=dev)) for i in self.sel.layers if i <= self.sel.last}

    def _scores(self, hist: Sequence[int], t0: int, t1: int, lens: torch.Tensor) -> None:
        """Score rows [t0, t1) from the window [ws, ws + W) (on the bulk stream; ``lens`` = (t1 - t0, S, ...) on the device)."""
        m, s = self.m, self.scratch
        ws, W = window(t0, t1, self.halo, self.Wmax, self.Tar, self.chunk)
        rows = token_row(hist, ws, W, t1, int(m.cfg.bos_row), m.V)
        s.tok[:, :W].copy_(torch.tensor([rows], dtype=torch.int32), non_blocking=False)
        s.xb[:W].copy_(self.cond[0, ws: ws + W])
        walk(m, self.sel, s, self.kv.__getitem__, 1, W, self.Sp, lens[0:1], lens[1:2], self.acc[:, t0:t1], q_off=(t0 - ws) * m.D)

    @torch.inference_mode()
    def step(self, hist: Sequence[int], t1: int, final: bool) -> List[int]:
        """Frames [0, t1) of the codebook-0 history ``hist`` are in (t1 never decreases; ``final``: no more will come) -> the path
        positions of the frames this step committed.  ``state_host`` = (c, p, status, e), ``base`` and ``path`` follow."""
        t1 = min(int(t1), self.Tar)
        t0 = self.t0
        if t1 < t0:
            raise ValueError(f"AlignStream: t1 = {t1} after {t0} frames were scored")
        if t1 - (self.c + 1) > hip.ALIGN_WINDOW_MAX:
            raise ValueError(f"AlignStream: {t1 - (self.c + 1)} uncommitted frames, at most {hip.ALIGN_WINDOW_MAX}")
        if t1 == 0 or (t1 == t0 and not final):
            return []
        nw = hip.ALIGN_STATE_WORDS
        with self.m.on_stream(bulk=True):
            lens = torch.tensor([t1 - t0, self.S, t1, 1 if final else 0], dtype=torch.int32).to(self.m.device)
            if t1 > t0:
                self._scores(hist, t0, t1, lens)
                self.t0 = t1
            hip.align_online(self.acc, lens[2:3], lens[1:2], lens[3:4], self.lag, self.state, self.pathd)
            host = self.out[: nw + t1].cpu()
        c, p, status, e = (int(v) for v in host[:4].tolist())
        self.base = float(host[4:5].view(torch.float32)[0])
        new = host[nw + self.c + 1: nw + c + 1].tolist()
        self.c, self.state_host = c, (c, p, status, e)
        self.path += new
        if final:
            self.m.align_last = self.scores()  # (as after align_batch: the score matrix of the last timed call)
        return new

    def scores(self) -> torch.Tensor:
        """The score rows written so far, [1, t0, S] on the device (a view of the persistent buffer)."""
        return self.acc[:, : self.t0, : self.S]
