"""Plain restatements of the row / elementwise operations of sopro_amd/csrc/elementwise.hip, one short function per C entry point
(the contracts are the prototypes of include/sopro_hip.h).  Every function takes what the entry point takes - FLAT buffers (1-D
tensors, the memory a pointer addresses) with leading dimensions, segment strides, ``lens`` and ``inner`` - plus the element
offsets the wrappers of sopro_amd/hip.py add to a pointer, writes the operation's result into a copy of the flat ``out`` it is given
and returns that copy: words the operation does not own keep whatever the caller put there (a canary).  Each is written from the
operation's definition (the module of the reference model it replaces), evaluated in ``dt`` - float64 by default; the same code at
``dt=torch.float32`` is the straightforward fp32 evaluation that ``tolerance`` takes its yardstick from.
tests/test_elementwise_ref.py checks every function against an independent formulation on the CPU; tests/test_gpu_elementwise.py
compares the kernels with them.  Not imported by the package."""
import torch

NORM_RMS, NORM_LN = 0, 1
F64 = torch.float64


def tolerance(ref64, ref32, factor=4.0):
    """factor * max(e32, floor): e32 = largest error of the fp32 evaluation of the same formula against the float64 one,
    floor = 4 * 2^-24 * max|ref| - both taken over the finite words the two evaluations share (canaries are NaN)."""
    r64, r32 = ref64.double().flatten(), ref32.double().flatten()
    used = torch.isfinite(r64) & torch.isfinite(r32)
    if not bool(used.any()):
        return 0.0
    e32 = float((r64[used] - r32[used]).abs().max())
    floor = 4.0 * 2.0 ** -24 * float(r64[used].abs().max())
    return factor * max(e32, floor)


def _ar(n):
    return torch.arange(int(n), dtype=torch.int64)


def _row_index(rows, rows_per_seg, ld, seg_stride, width, off=0):
    """flat index [rows, width] of row r = segment r // rows_per_seg at ``seg_stride``, row r % rows_per_seg at ``ld``"""
    r = _ar(rows)
    seg = r // rows_per_seg
    base = off + seg * int(seg_stride) + (r - seg * rows_per_seg) * int(ld)
    return base[:, None] + _ar(width)[None, :]


def _lens(lens, B, T):
    return torch.full((B,), T, dtype=torch.int64) if lens is None else lens.long().clamp(max=T)


def _opt(t, dt):
    return None if t is None else t.to(dt)


# ------------------------------------------------------------------------------------------------ norms and row scalings
def norm(x, ldx, x_seg_stride, out, ldo, w, b, mul, add, rows, rows_per_seg, C, eps, kind, x_off=0, o_off=0, dt=F64):
    """RMSNorm (x / sqrt(mean x^2 + eps) * w) or LayerNorm ((x - mean) / sqrt(var + eps) * w), then + b, then the FiLM pair of the
    row's segment: * mul[seg] + add[seg].  Source rows are segmented (x_seg_stride 0 = dense), output rows are ``ldo`` apart."""
    xs = x.to(dt)[_row_index(rows, rows_per_seg, ldx, x_seg_stride if x_seg_stride else rows_per_seg * ldx, C, x_off)]
    if kind == NORM_LN:
        xs = xs - xs.mean(-1, keepdim=True)
    elif kind != NORM_RMS:
        raise ValueError("unknown norm kind")
    y = xs / torch.sqrt(xs.pow(2).mean(-1, keepdim=True) + eps) * w.to(dt)[:C]
    if b is not None:
        y = y + b.to(dt)[:C]
    seg = _ar(rows) // rows_per_seg
    if mul is not None:
        y = y * mul.to(dt).view(-1, C)[seg]
    if add is not None:
        y = y + add.to(dt).view(-1, C)[seg]
    o = out.to(dt).clone()
    o[_row_index(rows, rows, ldo, 0, C, o_off)] = y
    return o


def rms_match(a, x, out, rows, C, dt=F64):
    """a scaled to the RMS of x: a * clamp(rms(x) / rms(a), 0, 10), rms(v) = sqrt(mean v^2 + 1e-6)"""
    av, xv = a.to(dt)[: rows * C].view(rows, C), x.to(dt)[: rows * C].view(rows, C)
    rms = lambda v: torch.sqrt(v.pow(2).mean(-1, keepdim=True) + 1e-6)  # noqa: E731
    o = out.to(dt).clone()
    o[: rows * C] = (av * (rms(xv) / rms(av)).clamp(0.0, 10.0)).flatten()
    return o


def l2norm(x, out, rows, C, eps, dt=F64):
    """x / max(||x||_2, eps) per row"""
    xv = x.to(dt)[: rows * C].view(rows, C)
    o = out.to(dt).clone()
    o[: rows * C] = (xv / xv.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(eps)).flatten()
    return o


def tanh_affine(x, out, c0, c1, n, dt=F64):
    o = out.to(dt).clone()
    o[:n] = c0 + c1 * torch.tanh(x.to(dt)[:n])
    return o


def add_pos(rowvec, table, out, B, T, C, pos0, dt=F64):
    """out[b, t] = rowvec[b] + table[pos0 + t]"""
    o = out.to(dt).clone()
    o[: B * T * C] = (rowvec.to(dt)[: B * C].view(B, 1, C) + table.to(dt).view(-1, C)[pos0: pos0 + T][None]).flatten()
    return o


def masked_mean(x, lens, out, B, T, C, dt=F64):
    """sum over the frames t < lens[b] that exist, over (their number + 1e-6)"""
    mask = (_ar(T)[None, :] < _lens(lens, B, T)[:, None]).to(dt)
    o = out.to(dt).clone()
    o[: B * C] = ((x.to(dt)[: B * T * C].view(B, T, C) * mask[..., None]).sum(1) / (mask.sum(1, keepdim=True) + 1e-6)).flatten()
    return o


def stats_pool(h, logit, lens, out, B, T, C, dt=F64):
    """attentive statistics: a = softmax over the valid frames of logit; out[b] = [sum a h | sqrt(max(sum a (h - mu)^2, 1e-6))]"""
    hv = h.to(dt)[: B * T * C].view(B, T, C)
    valid = _ar(T)[None, :] < _lens(lens, B, T)[:, None]
    a = torch.softmax(logit.to(dt)[: B * T].view(B, T).masked_fill(~valid, float("-inf")), dim=1)[..., None]
    mu = (a * hv).sum(1)
    sd = (a * (hv - mu[:, None]).pow(2)).sum(1).clamp_min(1e-6).sqrt()
    o = out.to(dt).clone()
    o[: B * 2 * C] = torch.cat([mu, sd], -1).flatten()
    return o


# ------------------------------------------------------------------------------------------------ depthwise convolution
def _gelu(v):
    return v * 0.5 * (1.0 + torch.erf(v * 0.7071067811865476))


def dwconv(x, w, bias, res, out, lens, B, T, C, ksize, dil, left, mode, dt=F64):
    """out[b, t, c] = bias[c] + sum_j w[j, c] x[b, t - left + j dil, c] over the source frames inside [0, lens[b]);
    mode 1 adds res, mode 2 applies the erf GELU.  Every t < T is written."""
    xv, wv = x.to(dt)[: B * T * C].view(B, T, C), w.to(dt)[: ksize * C].view(ksize, C)
    xv = xv * (_ar(T)[None, :] < _lens(lens, B, T)[:, None]).to(dt)[..., None]
    y = torch.zeros(B, T, C, dtype=dt)
    for j in range(ksize):
        sh = j * dil - left  # source frame = t + sh
        lo, hi = max(0, -sh), min(T, T - sh)
        if lo < hi:
            y[:, lo:hi] += wv[j] * xv[:, lo + sh: hi + sh]
    if bias is not None:
        y = y + bias.to(dt)[:C]
    if mode == 1:
        y = y + res.to(dt)[: B * T * C].view(B, T, C)
    elif mode == 2:
        y = _gelu(y)
    o = out.to(dt).clone()
    o[: B * T * C] = y.flatten()
    return o


# ------------------------------------------------------------------------------------------------ gathers and arg-max
def codebook_sum(tok, ldt, col, off, wq, nq, table, table_rows, base, alpha, beta, out, ldo, o_seg_stride, rows, rows_per_seg, D,
                 o_off=0, dt=F64):
    """out[row] = alpha * base[row] + beta * sum_q wq[q] * table[clamp(off[q] + tok[row, col[q]], 0, table_rows - 1)]"""
    tv = table.to(dt)[: table_rows * D].view(table_rows, D)
    t = tok.long()[(_ar(rows) * ldt)[:, None] + col.long()[None, :nq]] + off.long()[None, :nq]
    y = beta * (wq.to(dt)[:nq, None] * tv[t.clamp(0, table_rows - 1)]).sum(1)
    if base is not None:
        y = y + alpha * base.to(dt)[: rows * D].view(rows, D)
    o = out.to(dt).clone()
    o[_row_index(rows, rows_per_seg, ldo, o_seg_stride, D, o_off)] = y
    return o


def text_embed(ids, lens, table, table_rows, pe, out, B, T, C, dt=F64):
    """out[b, t] = table[clamp(ids[b, t])] + pe[t] for t < lens[b], zero after"""
    e = table.to(dt)[: table_rows * C].view(table_rows, C)[ids.long()[: B * T].view(B, T).clamp(0, table_rows - 1)]
    y = (e + pe.to(dt)[: T * C].view(1, T, C)) * (_ar(T)[None, :] < _lens(lens, B, T)[:, None]).to(dt)[..., None]
    o = out.to(dt).clone()
    o[: B * T * C] = y.flatten()
    return o


def argmax_rows(x, ldx, out, ldo, inner, rows, N):
    """out[(r // inner) * ldo + r % inner] = index of the largest non-NaN entry of row r, the lowest index among equals;
    0 for a row with no non-NaN entry"""
    o = out.clone()
    xv = x.double()
    for r in range(rows):
        best, bi = None, 0
        for n in range(N):
            v = float(xv[r * ldx + n])
            if v == v and (best is None or v > best):
                best, bi = v, n
        o[(r // inner) * ldo + r % inner] = bi
    return o


# ------------------------------------------------------------------------------------------------ rope, upsample, last conv
def rope(x, ldx, cos_t, sin_t, rows, rows_per_seg, pos0, H, dh, x_off=0, dt=F64):
    """rotate-half RoPE in place on the H heads of dh columns that start at x_off of every row: (a, b) -> (a c - b s, b c + a s)
    for the pair (e, e + dh / 2), angle row pos0 + row % rows_per_seg of the tables [npos, dh / 2]"""
    half = dh // 2
    o = x.to(dt).clone()
    idx = (x_off + _ar(rows) * ldx)[:, None, None] + (_ar(H) * dh)[None, :, None] + _ar(half)[None, None, :]
    pos = pos0 + _ar(rows) % rows_per_seg
    c, s = cos_t.to(dt).view(-1, half)[pos][:, None], sin_t.to(dt).view(-1, half)[pos][:, None]
    a, b = o[idx], o[idx + half]
    o[idx], o[idx + half] = a * c - b * s, b * c + a * s
    return o


def upsample2(x, w, y, y_seg_stride, B, T, C, y_off=0, dt=F64):
    """depthwise transposed conv, kernel 4, stride 2, trimmed to 2 T frames: y[b, 2 t + r] = x[b, t] w[:, r] + x[b, t - 1] w[:, r + 2]"""
    xv, wv = x.to(dt)[: B * T * C].view(B, T, C), w.to(dt)[: C * 4].view(C, 4)
    full = torch.zeros(B, 2 * T + 2, C, dtype=dt)
    for k in range(4):  # frame t contributes x w[:, k] to output frame 2 t + k
        full[:, k: k + 2 * T: 2] += xv * wv[:, k]
    o = y.to(dt).clone()
    o[(y_off + _ar(B) * y_seg_stride)[:, None] + _ar(2 * T * C)[None, :]] = full[:, : 2 * T].reshape(B, -1)
    return o


def final_conv(h, h_seg_stride, w, bias, wav, wav_seg_stride, B, T, dt=F64):
    """wav[b, n] = bias + sum_j sum_c elu(h[b, n + j, c]) w[j, c], j = 0..2, over the PADDED rows of segment b (row p = sample
    p - 2; the two leading rows are the causal pad), 64 channels"""
    hv = h.to(dt)[(_ar(B) * h_seg_stride)[:, None] + _ar((T + 2) * 64)[None, :]].view(B, T + 2, 64)
    e = torch.where(hv > 0, hv, torch.expm1(hv))
    wv = w.to(dt)[:192].view(3, 64)
    y = bias + sum((e[:, j: j + T] * wv[j]).sum(-1) for j in range(3))
    o = wav.to(dt).clone()
    o[(_ar(B) * wav_seg_stride)[:, None] + _ar(T)[None, :]] = y
    return o


# ------------------------------------------------------------------------------------------------ words: fill, copy, seed, bf16
def fill2d(p, pitch, rows, width, value):
    o = p.clone()
    o[(_ar(rows) * pitch)[:, None] + _ar(width)[None, :]] = value
    return o


def copy2d(dst, dpitch, src, spitch, rows, width):
    o = dst.clone()
    o[(_ar(rows) * dpitch)[:, None] + _ar(width)[None, :]] = src[(_ar(rows) * spitch)[:, None] + _ar(width)[None, :]]
    return o


def nar_seed(tokens, Q, cb0, cb0_bstride, B, T, vmax):
    """tokens[b T + t, 0] = clamp(cb0[b, t], 0, vmax) (rows of cb0 are cb0_bstride apart); the other columns are not touched"""
    o = tokens.clone()
    o[_ar(B * T) * Q] = cb0[(_ar(B) * cb0_bstride)[:, None] + _ar(T)[None, :]].clamp(0, vmax).flatten().to(o.dtype)
    return o


def f32_bits(t):
    return t.contiguous().view(torch.int32).long() & 0xFFFFFFFF


def bits_f32(u):
    u = u.long() & 0xFFFFFFFF
    return torch.where(u >= (1 << 31), u - (1 << 32), u).to(torch.int32).view(torch.float32)


def cvt_f32_bf16_bits(src, n):
    """the 16-bit patterns of round-to-nearest-even fp32 -> bf16 (int64 tensor), by integer arithmetic on the fp32 patterns: add
    half an ulp of the kept field, less one when the kept field is even, and drop the low half.  NaN -> a quiet NaN of its sign."""
    u = f32_bits(src[:n].float())
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return torch.where(nan, (u >> 16) | 0x40, r)


def cvt_bf16_f32(bits16, n):
    """bf16 patterns -> the fp32 they denote (exact: the pattern in the high half)"""
    return bits_f32(bits16[:n].long() << 16)
