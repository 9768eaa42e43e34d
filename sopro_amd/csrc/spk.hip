// Ragged, batched Token2SV and the cosine of speaker vectors (include/sopro_hip.h, "voice similarity").
//
// Token2SV (src/sopro/nn/speaker.py:37-61, pooling src/sopro/nn/blocks.py:174-188) of `rows` padded utterances in TWO launches,
// every row computed exactly as its own unpadded utterance (lengths == T, how src/sopro/model.py:158-159 makes sv_ref): frames
// outside [0, len) are zero for BOTH depthwise convs, where the reference's padded batch path masks only before the first and
// after the second.
//
//   spk_frames_kernel  grid (time tile of SPK_TILE_FRAMES frames, row), 384 threads = 8 frames x 48 channel quads = 6 waves.
//     x   = sum_q cw[q] emb[q V + tok[t, q]]          tile + 6 frames of halo on each side (two stacked radius-3 convs)   LDS
//     h1  = GELU(dwconv7(x) + b0), 0 outside [0, len)  tile + 3                                                            LDS
//     h   = GELU(dwconv7(h1) + b3), 0 outside          tile                                           LDS (over x) + workspace
//     logit = w2 . tanh(W1 h + b1) + b2                exact fp32 MFMA (v_mfma_f32_32x32x2_f32), transposed form: wave w owns
//         W1 rows 32 w .. 32 w + 31 as the A operand (fragments straight from global / L2: 147 KB, shared by every workgroup),
//         the tile's 32 frames of h are the B operand (LDS, rows padded to SD + 4 floats so the 16-byte fragment reads of a lane
//         group hit distinct slots).  The accumulator then has the frame on the lane and W1's rows in its registers: the w2
//         contraction is 16 in-register terms, one lane-half exchange and a fixed-order sum of the six waves' partials.
//     LDS at SD = 192: x 44 x 192 x 4 = 33.8 KB (h, 32 x 196 x 4 = 25.1 KB, goes over it once conv 1 has read it), h1 38 x 192 x 4
//     = 29.2 KB, partials 0.8 KB: 63.7 KB, two workgroups per CU.
//   spk_pool_kernel    one workgroup per row: masked softmax, mu, two-pass variance, proj, F.normalize.  Every reduction has a
//     fixed order (time slices combined in index order, wave butterflies): two runs give the same bits; no atomics.
//   spk_cosine_kernel  one wave per output.
#include "common.h"

int sopro_spk_frames_launch(const int32_t* tok, int64_t row_stride, int32_t Q, const int32_t* col, const int32_t* off, const float* cw, const float* emb,
                            int64_t table_rows, int32_t SD, const float* w0, const float* b0, const float* w3, const float* b3, const float* W1,
                            const float* b1, const float* w2, const float* b2, const int32_t* lens, int32_t rows, int32_t t_cap, float* h_ws,
                            float* lg_ws, float* dbg_h, float* dbg_lg, hipStream_t s);
int sopro_spk_pool_launch(const float* h_ws, const float* lg_ws, const int32_t* lens, int32_t rows, int32_t t_cap, int32_t SD, const float* Wp,
                          const float* bp, int32_t svd, float* sv, int64_t sv_stride, hipStream_t s);

namespace {

constexpr int TF = SOPRO_SPK_TILE_FRAMES;
constexpr int NTH = 384;

struct FramesArgs {
  const int32_t *tok, *col, *off, *lens;
  const float *cw, *emb, *w0, *b0, *w3, *b3, *W1, *b1, *w2, *b2;
  float *h_ws, *lg_ws, *dbg_h, *dbg_lg;
  int64_t row_stride, table_rows;
  int32_t Q, t_cap;
};

__device__ __forceinline__ void fma4(float4& acc, const float4& a, const float4& b) {
  acc.x += a.x * b.x; acc.y += a.y * b.y; acc.z += a.z * b.z; acc.w += a.w * b.w;
}

// GELU(sum_tap w[tap] * src[j + tap] + bias) of one channel quad: taps in index order, then the bias, as dwconv_kernel
// (elementwise.hip, activation 2) does; rows of `src` outside the utterance hold zeros, which add nothing
template <int SD>
__device__ __forceinline__ float4 conv7_gelu(const float* src, int j, int cq, const float4 (&wv)[7], const float4& bv) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int tap = 0; tap < 7; ++tap) fma4(acc, *reinterpret_cast<const float4*>(src + (j + tap) * SD + cq * 4), wv[tap]);
  acc.x += bv.x; acc.y += bv.y; acc.z += bv.z; acc.w += bv.w;
  return make_float4(gelu_erf(acc.x), gelu_erf(acc.y), gelu_erf(acc.z), gelu_erf(acc.w));
}

template <int SD>
__global__ __launch_bounds__(NTH) void spk_frames_kernel(const FramesArgs g) {
  static_assert(SD % 32 == 0 && NTH % (SD / 4) == 0 && SD / 32 == NTH / 64, "one wave per 32 rows of W1, whole frames per pass");
  constexpr int NQ = SD / 4, FL = NTH / NQ, LDH = SD + 4;
  constexpr int NX = TF + 12, N1 = TF + 6, NW = NTH / 64;
  static_assert(TF * LDH <= NX * SD, "h goes over x");
  extern __shared__ float4 smem4[];
  float* xs = reinterpret_cast<float*>(smem4);  // [NX][SD]; after conv 1: h [TF][LDH]
  float* h1s = xs + NX * SD;                    // [N1][SD]
  float* part = h1s + N1 * SD;                  // [NW][TF]
  float* hs = xs;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blockIdx.y, t0 = blockIdx.x * TF;
  const int len = min(max(g.lens[r], 0), g.t_cap);
  if (t0 >= len) return;  // (uniform: the whole workgroup leaves)
  const int cq = tid % NQ, fl = tid / NQ;

  // ---- 1. gather and mix (speaker.py:48-54): frames t0 - 6 .. t0 + TF + 5; tokens of frames outside [0, len) are never read
  for (int i = fl; i < NX; i += FL) {
    const int t = t0 - 6 + i;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t >= 0 && t < len) {
      const int32_t* tp = g.tok + (int64_t)r * g.row_stride + (int64_t)t * g.Q;
      for (int q = 0; q < g.Q; ++q) {
        int64_t row = (int64_t)g.off[q] + tp[g.col[q]];
        row = row < 0 ? 0 : (row >= g.table_rows ? g.table_rows - 1 : row);
        const float4 e = *reinterpret_cast<const float4*>(g.emb + row * SD + cq * 4);
        const float s = g.cw[q];
        acc.x += s * e.x; acc.y += s * e.y; acc.z += s * e.z; acc.w += s * e.w;
      }
    }
    *reinterpret_cast<float4*>(xs + i * SD + cq * 4) = acc;
  }
  float4 wv[7], bv;
#pragma unroll
  for (int tap = 0; tap < 7; ++tap) wv[tap] = *reinterpret_cast<const float4*>(g.w0 + tap * SD + cq * 4);
  bv = *reinterpret_cast<const float4*>(g.b0 + cq * 4);
  __syncthreads();

  // ---- 2. h1 on frames t0 - 3 .. t0 + TF + 2: zero outside the utterance, as the unpadded reference pads it (blocks.py:69-73)
  for (int j = fl; j < N1; j += FL) {
    const int t = t0 - 3 + j;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t >= 0 && t < len) o = conv7_gelu<SD>(xs, j, cq, wv, bv);
    *reinterpret_cast<float4*>(h1s + j * SD + cq * 4) = o;
  }
#pragma unroll
  for (int tap = 0; tap < 7; ++tap) wv[tap] = *reinterpret_cast<const float4*>(g.w3 + tap * SD + cq * 4);
  bv = *reinterpret_cast<const float4*>(g.b3 + cq * 4);
  __syncthreads();  // (x is dead from here: h is written over it)

  // ---- 3. h on the tile -> LDS (the contraction's B operand) and the workspace (the pooling kernel's input)
  for (int j = fl; j < TF; j += FL) {
    const int t = t0 + j;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < len) {
      o = conv7_gelu<SD>(h1s, j, cq, wv, bv);
      const int64_t at = ((int64_t)r * g.t_cap + t) * SD + cq * 4;
      *reinterpret_cast<float4*>(g.h_ws + at) = o;
      if (g.dbg_h) *reinterpret_cast<float4*>(g.dbg_h + at) = o;
    }
    *reinterpret_cast<float4*>(hs + j * LDH + cq * 4) = o;
  }
  __syncthreads();

  // ---- 4. logit (blocks.py:168-178).  acc[reg] = (W1 h^T)[n][t] for n = 32 wave + 8 (reg >> 2) + 4 (lane >> 5) + (reg & 3), t = lane & 31.
  // K is summed, so its order inside an 8-wide chunk is free as long as both operands agree (gemm_f32.hip): lanes 0-31 carry
  // k = 8 c + s, lanes 32-63 k = 8 c + 4 + s at step s.
  const int frow = lane & 31, fk = (lane >> 5) * 4;
  const float* ap = g.W1 + (int64_t)(wave * 32 + frow) * SD + fk;
  const float* bp = hs + frow * LDH + fk;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll 6
  for (int c = 0; c < SD / 8; ++c) {
    const float4 a4 = *reinterpret_cast<const float4*>(ap + c * 8);
    const float4 b4 = *reinterpret_cast<const float4*>(bp + c * 8);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, acc, 0, 0, 0);
  }
  float p = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int n0 = wave * 32 + 8 * k + 4 * (lane >> 5);
    const float4 b1v = *reinterpret_cast<const float4*>(g.b1 + n0);
    const float4 w2v = *reinterpret_cast<const float4*>(g.w2 + n0);
    p += w2v.x * tanhf(acc[4 * k + 0] + b1v.x);
    p += w2v.y * tanhf(acc[4 * k + 1] + b1v.y);
    p += w2v.z * tanhf(acc[4 * k + 2] + b1v.z);
    p += w2v.w * tanhf(acc[4 * k + 3] + b1v.w);
  }
  p += __shfl_xor(p, 32, 64);
  if (lane < 32) part[wave * TF + lane] = p;
  __syncthreads();
  if (tid < TF && t0 + tid < len) {
    float s = part[tid];
#pragma unroll
    for (int w = 1; w < NW; ++w) s += part[w * TF + tid];
    s += g.b2[0];
    const int64_t at = (int64_t)r * g.t_cap + t0 + tid;
    g.lg_ws[at] = s;
    if (g.dbg_lg) g.dbg_lg[at] = s;
  }
}

// Attentive statistics pooling (blocks.py:174-188) over t < len, proj (speaker.py:60) and F.normalize(eps 1e-6) (speaker.py:61).
// 256 threads = NS time slices x SD / 4 channel quads: slice s sums frames s, s + NS, ... in order, the slices are added in index
// order.  The variance is the two-pass sum a (h - mu)^2 of the reference, not sum a h^2 - mu^2 (which cancels).
constexpr int POOL_SD_MAX = 256, POOL_SV_MAX = 1024;
__global__ __launch_bounds__(256) void spk_pool_kernel(const float* __restrict__ h_ws, const float* __restrict__ lg_ws, const int32_t* __restrict__ lens,
                                                       int t_cap, int SD, const float* __restrict__ Wp, const float* __restrict__ bp, int svd,
                                                       float* __restrict__ sv, int64_t sv_stride) {
  __shared__ float4 part4[256];
  __shared__ float stat[2 * POOL_SD_MAX];
  __shared__ float ev[POOL_SV_MAX];
  __shared__ float red[4];
  __shared__ float sh_a, sh_b;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int len = min(max(lens[r], 0), t_cap);
  float* out = sv + (int64_t)r * sv_stride;
  if (len == 0) {  // nothing to pool: a zero vector (uniform branch)
    for (int o = tid; o < svd; o += 256) out[o] = 0.f;
    return;
  }
  const float* lg = lg_ws + (int64_t)r * t_cap;
  const float* h = h_ws + (int64_t)r * t_cap * SD;
  float m = -INFINITY;
  for (int t = tid; t < len; t += 256) m = fmaxf(m, lg[t]);
  m = wave_max(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  if (tid == 0) sh_a = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  const float mx = sh_a;
  float s = 0.f;
  for (int t = tid; t < len; t += 256) s += expf(lg[t] - mx);
  s = wave_sum(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (tid == 0) sh_b = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  const float inv = 1.f / sh_b;

  const int NQ = SD >> 2, NS = 256 / NQ;
  const int cq = tid % NQ, sl = tid / NQ;
  const bool on = sl < NS;
  // ---- mu = sum a h
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (on)
    for (int t = sl; t < len; t += NS) {
      const float a = expf(lg[t] - mx) * inv;
      const float4 hv = *reinterpret_cast<const float4*>(h + (int64_t)t * SD + cq * 4);
      acc.x += a * hv.x; acc.y += a * hv.y; acc.z += a * hv.z; acc.w += a * hv.w;
    }
  part4[tid] = acc;
  __syncthreads();
  if (tid < NQ) {
    float4 mu = part4[tid];
    for (int k = 1; k < NS; ++k) {
      const float4 q = part4[k * NQ + tid];
      mu.x += q.x; mu.y += q.y; mu.z += q.z; mu.w += q.w;
    }
    *reinterpret_cast<float4*>(stat + tid * 4) = mu;
  }
  __syncthreads();
  // ---- var = sum a (h - mu)^2, clamped at 1e-6
  const float4 mu = on ? *reinterpret_cast<const float4*>(stat + cq * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (on)
    for (int t = sl; t < len; t += NS) {
      const float a = expf(lg[t] - mx) * inv;
      const float4 hv = *reinterpret_cast<const float4*>(h + (int64_t)t * SD + cq * 4);
      const float dx = hv.x - mu.x, dy = hv.y - mu.y, dz = hv.z - mu.z, dw = hv.w - mu.w;
      acc.x += a * dx * dx; acc.y += a * dy * dy; acc.z += a * dz * dz; acc.w += a * dw * dw;
    }
  part4[tid] = acc;
  __syncthreads();
  if (tid < NQ) {
    float4 v = part4[tid];
    for (int k = 1; k < NS; ++k) {
      const float4 q = part4[k * NQ + tid];
      v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
    }
    stat[SD + tid * 4 + 0] = sqrtf(fmaxf(v.x, 1e-6f));
    stat[SD + tid * 4 + 1] = sqrtf(fmaxf(v.y, 1e-6f));
    stat[SD + tid * 4 + 2] = sqrtf(fmaxf(v.z, 1e-6f));
    stat[SD + tid * 4 + 3] = sqrtf(fmaxf(v.w, 1e-6f));
  }
  __syncthreads();
  // ---- e = proj([mu | std]) + b: one wave per output, lanes stride the 2 SD inputs
  for (int o = wave; o < svd; o += 4) {
    const float* wr = Wp + (int64_t)o * 2 * SD;
    float d = 0.f;
    for (int k = lane; k < 2 * SD; k += 64) d += stat[k] * wr[k];
    d = wave_sum(d);
    if (lane == 0) ev[o] = d + bp[o];
  }
  __syncthreads();
  // ---- F.normalize: e / max(|e|, 1e-6)
  float q = 0.f;
  for (int o = tid; o < svd; o += 256) q += ev[o] * ev[o];
  q = wave_sum(q);
  if (lane == 0) red[wave] = q;
  __syncthreads();
  const float den = fmaxf(sqrtf((red[0] + red[1]) + (red[2] + red[3])), 1e-6f);
  for (int o = tid; o < svd; o += 256) out[o] = ev[o] / den;
}

// out = a . b / max(|a| |b|, 1e-12), one wave per output: pairwise (bank == 0) a[i] with b[i] -> out[i]; bank: a[i] with every b[n]
// -> out[i nb + n].  Both norms are recomputed; a zero vector gives 0.0.
__global__ __launch_bounds__(256) void spk_cosine_kernel(const float* __restrict__ a, int64_t a_stride, int na, const float* __restrict__ b,
                                                         int64_t b_stride, int nb, int dim, int bank, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t o = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t total = bank ? (int64_t)na * nb : na;
  if (o >= total) return;
  const int i = bank ? (int)(o / nb) : (int)o, n = bank ? (int)(o % nb) : (int)o;
  const float* av = a + (int64_t)i * a_stride;
  const float* bv = b + (int64_t)n * b_stride;
  float ab = 0.f, aa = 0.f, bb = 0.f;
  for (int k = lane; k < dim; k += 64) {
    const float x = av[k], y = bv[k];
    ab += x * y; aa += x * x; bb += y * y;
  }
  ab = wave_sum(ab); aa = wave_sum(aa); bb = wave_sum(bb);
  if (lane == 0) out[o] = ab / fmaxf(sqrtf(aa) * sqrtf(bb), 1e-12f);
}

}  // namespace

int sopro_spk_frames_launch(const int32_t* tok, int64_t row_stride, int32_t Q, const int32_t* col, const int32_t* off, const float* cw, const float* emb,
                            int64_t table_rows, int32_t SD, const float* w0, const float* b0, const float* w3, const float* b3, const float* W1,
                            const float* b1, const float* w2, const float* b2, const int32_t* lens, int32_t rows, int32_t t_cap, float* h_ws,
                            float* lg_ws, float* dbg_h, float* dbg_lg, hipStream_t s) {
  SOPRO_CHECK_ARG(SD == 192, "the frames kernel is built for a Token2SV width of 192");
  SOPRO_CHECK_ARG(rows > 0 && rows <= 65535 && t_cap > 0 && Q > 0 && table_rows > 0, "1 <= rows <= 65535, t_cap >= 1");
  SOPRO_CHECK_ARG(aligned16(emb) && aligned16(w0) && aligned16(b0) && aligned16(w3) && aligned16(b3) && aligned16(W1) && aligned16(b1) && aligned16(w2) &&
                      aligned16(h_ws) && (!dbg_h || aligned16(dbg_h)),
                  "weights, workspace and dbg_h must be 16-byte aligned");
  FramesArgs g;
  g.tok = tok; g.col = col; g.off = off; g.lens = lens;
  g.cw = cw; g.emb = emb; g.w0 = w0; g.b0 = b0; g.w3 = w3; g.b3 = b3; g.W1 = W1; g.b1 = b1; g.w2 = w2; g.b2 = b2;
  g.h_ws = h_ws; g.lg_ws = lg_ws; g.dbg_h = dbg_h; g.dbg_lg = dbg_lg;
  g.row_stride = row_stride; g.table_rows = table_rows; g.Q = Q; g.t_cap = t_cap;
  constexpr int SDK = 192;
  constexpr size_t lds = ((size_t)(TF + 12 + TF + 6) * SDK + (size_t)(NTH / 64) * TF) * sizeof(float);
  static_assert(lds <= 64 * 1024, "two workgroups per CU");
  auto kern = spk_frames_kernel<SDK>;
  SOPRO_SET_MAX_LDS_ONCE(kern, lds);
  hipLaunchKernelGGL(kern, dim3((t_cap + TF - 1) / TF, rows), dim3(NTH), lds, s, g);
  SOPRO_LAUNCH_CHECK();
}

int sopro_spk_pool_launch(const float* h_ws, const float* lg_ws, const int32_t* lens, int32_t rows, int32_t t_cap, int32_t SD, const float* Wp,
                          const float* bp, int32_t svd, float* sv, int64_t sv_stride, hipStream_t s) {
  SOPRO_CHECK_ARG(SD > 0 && SD % 4 == 0 && SD <= POOL_SD_MAX && svd > 0 && svd <= POOL_SV_MAX, "Token2SV width <= 256 (a multiple of 4), sv_student_dim <= 1024");
  SOPRO_CHECK_ARG(rows > 0 && t_cap > 0 && sv_stride >= svd, "rows >= 1, t_cap >= 1, sv_stride >= sv_student_dim");
  hipLaunchKernelGGL(spk_pool_kernel, dim3(rows), dim3(256), 0, s, h_ws, lg_ws, lens, t_cap, SD, Wp, bp, svd, sv, sv_stride);
  SOPRO_LAUNCH_CHECK();
}

extern "C" int32_t sopro_spk_tile_frames(void) { return TF; }

extern "C" int sopro_spk_cosine(const float* a, int64_t a_stride, int32_t na, const float* b, int64_t b_stride, int32_t nb, int32_t dim, int32_t bank,
                                float* out, void* stream) {
  SOPRO_CHECK_ARG(a && b && out, "a, b and out must be non-NULL");
  SOPRO_CHECK_ARG(na > 0 && nb > 0 && dim > 0, "na, nb, dim >= 1");
  SOPRO_CHECK_ARG(bank == 0 || bank == 1, "bank is 0 (pairwise) or 1");
  SOPRO_CHECK_ARG(bank || na == nb, "pairwise mode wants na == nb");
  SOPRO_CHECK_ARG((na == 1 || a_stride >= dim) && (nb == 1 || b_stride >= dim), "row strides must be >= dim");
  const int64_t total = bank ? (int64_t)na * nb : na;
  SOPRO_CHECK_ARG(total <= ((int64_t)1 << 31), "too many outputs");
  hipLaunchKernelGGL(spk_cosine_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a, a_stride, na, b, b_stride, nb, dim, bank, out);
  SOPRO_LAUNCH_CHECK();
}
