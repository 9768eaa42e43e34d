// Watermark: a keyed spread-spectrum mark added to the rows of a padded batch, and its detector (contract: include/sopro_hip.h,
// DESIGN.md "Watermark").
// Embed.  Memory-bound and on the path of every marked pass: the grid is (tile of WM_TILE samples, row) and one launch covers the whole
// padded batch.  Per tile:
//   stage   - x[tile - HS .. tile + WM_TILE + HS) into LDS: 16-byte global loads over the aligned body, dwords at the ragged ends, zeros
//             (or the retained tail of a chunked row) outside this call's samples
//   maxima  - the WM_TILE / HS + 2 block maxima of |x| over that span (wave reductions), from which the tile's envelope points follow:
//             no separate envelope pass over the batch
//   mark    - four consecutive samples per lane, in place in LDS: one dword of the carrier table holds their four chips
//   store   - from LDS, so that the global stores are 16 bytes wide whatever the alignment of the row
// A row without a carrier is staged and stored only.  The chunked form keeps (samples emitted, received, tail) per row; the tiles only
// read it, and a second, small launch rewrites it once they are done.
// Detect.  fold: block maxima of every row into the workspace, then one thread per residue walks the row in steps of P (whitening on
// the fly).  corr: both 8192 x 8192 circular correlations of a row as (tile of 1024 offsets, row) workgroups with f and both int8
// templates in LDS; a lane owns four offsets 256 apart, so the lanes of a wave read consecutive words of f and every template word is
// a broadcast shared by eight accumulators.  peak: one workgroup per (lane, row), float64 moments.
#include "common.h"
#include "rows_window.h"

namespace {

constexpr int HS = SOPRO_WM_HS;
constexpr int P = SOPRO_WM_P;
constexpr int WM_TILE = SOPRO_WM_TILE;
constexpr int WM_TAIL = SOPRO_WM_TAIL;
constexpr int WM_BLOCK = 256;
constexpr int WAVES = WM_BLOCK / 64;
constexpr int NB = WM_TILE / HS + 2;   // block maxima a tile needs: blocks kb - 1 .. kb + WM_TILE / HS
constexpr int SPAN = WM_TILE + 2 * HS;
constexpr int64_t LEN_MAX = (int64_t)1 << 30;
static_assert(WM_TILE % HS == 0 && HS % 4 == 0 && P % 4 == 0 && (P & (P - 1)) == 0, "tiles start on the envelope grid and on a carrier dword");
static_assert(HS <= 2 * WM_BLOCK && WM_TAIL >= 3 * HS, "the maxima loop takes two elements per lane; the tail bound of sopro_hip.h");

// state of one row: 4 int64 of header, then WM_TAIL floats
constexpr int H_N = 0, H_RECV = 1, H_BASE = 2;
constexpr int WM_HDR = 4;
constexpr int STATE_WORDS = WM_HDR + WM_TAIL / 2;

struct Row {
  RowWindow w;
  int64_t n0, n1;     // the samples this call emits
  bool overflow;      // they do not fit out_cap
};

// What a call does for a row, from the arguments and the state as the call found it (both kernels of a call derive the same).
__device__ __forceinline__ Row row_setup(int row, const float* in, int64_t in_stride, const int32_t* in_lens, int64_t in_cap, const int64_t* state,
                                         int flush, int64_t out_cap) {
  Row r;
  const int64_t* hdr = state ? state + (int64_t)row * STATE_WORDS : nullptr;
  int64_t n0 = 0, recv0 = 0, base = 0;
  if (hdr) {
    n0 = hdr[H_N];
    recv0 = hdr[H_RECV];
    base = hdr[H_BASE];
    // (a header nobody zeroed: keep every derived index inside the buffers)
    if (n0 < 0 || n0 % HS != 0 || n0 > recv0 || recv0 < 0 || recv0 > LEN_MAX || base < 0 || base > recv0 || recv0 - base > WM_TAIL) n0 = recv0 = base = 0;
  }
  int64_t n_in = in_lens[row];
  n_in = n_in < 0 ? 0 : (n_in > in_cap ? in_cap : n_in);
  n_in = recv0 + n_in > LEN_MAX ? LEN_MAX - recv0 : n_in;
  r.w.in = in + (int64_t)row * in_stride;
  r.w.tail = hdr ? reinterpret_cast<const float*>(hdr + WM_HDR) : nullptr;
  r.w.in_base = recv0;
  r.w.tail_base = hdr ? base : recv0;
  r.w.recv = recv0 + n_in;
  const int64_t n1 = flush ? r.w.recv : (r.w.recv / HS - 1) * HS;  // block k is ready once recv >= (k + 2) HS
  r.n0 = n0;
  r.n1 = n1 < n0 ? n0 : n1;
  r.overflow = r.n1 - r.n0 > out_cap;
  return r;
}

// The definition rounds every operation on its own (see tsm.hip on why this is a pragma and not a set of intrinsics).
#pragma clang fp contract(off)

__global__ __launch_bounds__(WM_BLOCK) void wm_embed_kernel(const float* __restrict__ in, int64_t in_stride, const int32_t* __restrict__ in_lens,
                                                            int64_t in_cap, const int32_t* __restrict__ car_idx, const int8_t* __restrict__ cars,
                                                            int n_cars, const float* __restrict__ alphas, const int64_t* __restrict__ state, int flush,
                                                            const float* __restrict__ tab, float* __restrict__ out, int64_t out_stride, int64_t out_cap,
                                                            int32_t* __restrict__ out_lens) {
  __shared__ __attribute__((aligned(16))) float s_x[SPAN];  // s_x[k] = x[na - HS + k]; the tile's samples are marked in place
  __shared__ float s_tab[HS];
  __shared__ float s_bw[NB][WAVES];
  __shared__ float s_e[NB - 1];  // s_e[q] = e_{kb + q}, kb = na / HS

  const int row = blockIdx.y, tid = threadIdx.x;
  const Row r = row_setup(row, in, in_stride, in_lens, in_cap, state, flush, out_cap);
  if (blockIdx.x == 0 && tid == 0) out_lens[row] = r.overflow ? -1 : (int32_t)(r.n1 - r.n0);
  if (r.overflow) return;  // (every condition up to the barriers is uniform over the workgroup)
  const int64_t na = r.n0 + (int64_t)blockIdx.x * WM_TILE;
  if (na >= r.n1) return;
  const int cnt = (int)(r.n1 - na < WM_TILE ? r.n1 - na : WM_TILE);
  int ci = car_idx[row];
  const bool marked = ci >= 0 && n_cars > 0;
  ci = ci >= n_cars ? n_cars - 1 : ci;

  // the part of the row this tile reads: all of the span for a marked row, its own samples otherwise
  const int64_t i_lo = na - HS;
  const int k_lo = marked ? 0 : HS, k_hi = marked ? SPAN : HS + cnt;
  // [ka, kb): the part of it that lies in this call's samples; the rest is the retained tail or zero
  int64_t ga = i_lo + k_lo > r.w.in_base ? i_lo + k_lo : r.w.in_base, gb = i_lo + k_hi < r.w.recv ? i_lo + k_hi : r.w.recv;
  ga = ga > i_lo + k_hi ? i_lo + k_hi : ga;
  gb = gb < ga ? ga : gb;
  const int ka = (int)(ga - i_lo), kb = (int)(gb - i_lo);
  for (int k = k_lo + tid; k < k_hi; k += WM_BLOCK)
    if (k < ka || k >= kb) s_x[k] = row_at_tail(r.w, i_lo + k);
  if (kb > ka) stage_in<WM_BLOCK>(s_x + ka, r.w.in + (ga - r.w.in_base), kb - ka, tid);
  if (marked)
    for (int k = tid; k < HS; k += WM_BLOCK) s_tab[k] = tab[k];
  __syncthreads();

  if (marked) {
    const int wave = tid >> 6, lane = tid & 63;
    for (int j = 0; j < NB; ++j) {
      float v = fabsf(s_x[j * HS + tid]);
      if (tid + WM_BLOCK < HS) v = fmaxf(v, fabsf(s_x[j * HS + WM_BLOCK + tid]));
      v = wave_max(v);
      if (lane == 0) s_bw[j][wave] = v;
    }
    __syncthreads();
    if (tid < NB - 1) {
      float e = 0.0f;
      for (int w = 0; w < WAVES; ++w) e = fmaxf(e, fmaxf(s_bw[tid][w], s_bw[tid + 1][w]));
      s_e[tid] = e;
    }
    __syncthreads();
    const float alpha = alphas[row];
    const uint32_t* car = reinterpret_cast<const uint32_t*>(cars + (int64_t)ci * P);
    float* s_y = s_x + HS;
    for (int m = 4 * tid; m < cnt; m += 4 * WM_BLOCK) {  // (m + 3 < WM_TILE: a tile's last quad may run past cnt, never past the span)
      const int q = m / HS, rr = m - q * HS;              // (HS is a multiple of 4: the quad lies in one envelope segment)
      const float e0 = s_e[q], diff = s_e[q + 1] - e0;
      const uint32_t chips = car[(uint32_t)((na + m) & (P - 1)) >> 2];  // (na and m are multiples of 4)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float step = s_tab[rr + j] * diff;
        const float g = e0 + step;
        const float cf = 0.5f * (float)(int8_t)(chips >> (8 * j));  // (exact)
        const float ag = alpha * g;
        const float add = ag * cf;
        s_y[m + j] = s_y[m + j] + add;
      }
    }
    __syncthreads();
  }
  store_out<WM_BLOCK>(out + (int64_t)row * out_stride + (na - r.n0), s_x + HS, cnt, tid);  // (na - n0 + cnt <= n1 - n0 <= out_cap)
}

// The end of a chunked call: one workgroup per row rewrites the row's state once every tile of the call has read it (stream order).
constexpr int STATE_BLOCK = 512;

__global__ __launch_bounds__(STATE_BLOCK) void wm_state_kernel(const float* __restrict__ in, int64_t in_stride, const int32_t* __restrict__ in_lens,
                                                               int64_t in_cap, int64_t* __restrict__ state, int flush, int64_t out_cap) {
  __shared__ float s_keep[WM_TAIL];
  const int row = blockIdx.x, tid = threadIdx.x;
  const Row r = row_setup(row, in, in_stride, in_lens, in_cap, state, flush, out_cap);  // (the old header, by value)
  int64_t* hdr = state + (int64_t)row * STATE_WORDS;
  float* tail = reinterpret_cast<float*>(hdr + WM_HDR);
  if (flush || r.overflow) {  // the row is over: a zeroed header is a fresh row (uniform over the workgroup)
    for (int k = tid; k < WM_HDR; k += STATE_BLOCK) hdr[k] = 0;
    return;
  }
  // what the next block may read: everything from (k_next - 1) HS on (never before the current base, never past what was received)
  int64_t nb = r.n1 - HS;
  nb = nb < r.w.tail_base ? r.w.tail_base : nb;
  nb = nb > r.w.recv ? r.w.recv : nb;
  if (r.w.recv - nb > WM_TAIL) nb = r.w.recv - WM_TAIL;  // (unreachable: the bound in sopro_hip.h)
  const int keep = (int)(r.w.recv - nb);
  for (int k = tid; k < keep; k += STATE_BLOCK) s_keep[k] = row_at(r.w, nb + k);
  __syncthreads();  // the old tail has been read
  for (int k = tid; k < keep; k += STATE_BLOCK) tail[k] = s_keep[k];
  if (tid == 0) {
    hdr[H_N] = r.n1;
    hdr[H_RECV] = r.w.recv;
    hdr[H_BASE] = nb;
  }
}

// ---- detector ----
__host__ __device__ __forceinline__ int64_t fold_blocks(int64_t in_cap) { return in_cap / HS + 2; }  // b_j for j <= (L - 1) / HS + 1

__device__ __forceinline__ int64_t row_len(const int32_t* in_lens, int row, int64_t in_cap) {
  const int64_t n = in_lens[row];
  return n < 0 ? 0 : (n > in_cap ? in_cap : n);
}

// ws[row][j] = max |y[n]| over block j of the row (0 past its length): one wave per block
__global__ __launch_bounds__(WM_BLOCK) void wm_blockmax_kernel(const float* __restrict__ in, int64_t in_stride, const int32_t* __restrict__ in_lens,
                                                               int64_t in_cap, float* __restrict__ ws) {
  const int row = blockIdx.y, lane = threadIdx.x & 63;
  const int64_t nbk = fold_blocks(in_cap);
  const int64_t j = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (j >= nbk) return;  // (uniform over the wave)
  const int64_t L = row_len(in_lens, row, in_cap);
  const float* y = in + (int64_t)row * in_stride;
  float v = 0.0f;
  for (int i = lane; i < HS; i += 64) {
    const int64_t n = j * HS + i;
    if (n < L) v = fmaxf(v, fabsf(y[n]));
  }
  v = wave_max(v);
  if (lane == 0) ws[(int64_t)row * nbk + j] = v;
}

// f[row][r] = the sum over m (ascending) of u[r + m P]
__global__ __launch_bounds__(WM_BLOCK) void wm_fold_kernel(const float* __restrict__ in, int64_t in_stride, const int32_t* __restrict__ in_lens,
                                                           int64_t in_cap, const float* __restrict__ tab, const float* __restrict__ ws,
                                                           float* __restrict__ f) {
  __shared__ float s_pk[WAVES];
  const int row = blockIdx.y, tid = threadIdx.x;
  const int64_t nbk = fold_blocks(in_cap);
  const int64_t L = row_len(in_lens, row, in_cap);
  const float* y = in + (int64_t)row * in_stride;
  const float* b = ws + (int64_t)row * nbk;
  float pk = 0.0f;
  for (int64_t j = tid; j < nbk; j += WM_BLOCK) pk = fmaxf(pk, b[j]);
  pk = wave_max(pk);
  if ((tid & 63) == 0) s_pk[tid >> 6] = pk;
  __syncthreads();
  pk = s_pk[0];
  for (int w = 1; w < WAVES; ++w) pk = fmaxf(pk, s_pk[w]);
  const float thr = 1e-3f * pk;
  const int r = blockIdx.x * WM_BLOCK + tid;
  float acc = 0.0f;
  for (int64_t n = r; n < L; n += P) {
    const int64_t k = n / HS;  // k + 1 <= (L - 1) / HS + 1 < nbk
    const int rr = (int)(n - k * HS);
    const float b0 = b[k];
    const float e0 = fmaxf(k > 0 ? b[k - 1] : 0.0f, b0), e1 = fmaxf(b0, b[k + 1]);
    const float diff = e1 - e0;
    const float step = tab[rr] * diff;
    const float g = e0 + step;
    const float w = n > 0 ? y[n] - y[n - 1] : y[0];
    const float u = g > thr ? __fdiv_rn(w, g) : 0.0f;
    acc = acc + u;
  }
  f[(int64_t)row * P + r] = acc;
}

constexpr int CORR_PER = 4;                       // offsets per lane, WM_BLOCK apart
constexpr int CORR_TILE = CORR_PER * WM_BLOCK;    // 1024 offsets per workgroup

// R[row][l][o] = sum_n f[(n + o) mod P] d_l[n].  d is -2, 0 or 2, so every product is exact and the fused step is an add, a subtract
// or nothing in value.
__global__ __launch_bounds__(WM_BLOCK) void wm_corr_kernel(const float* __restrict__ f, const int8_t* __restrict__ dtab, int n_keys,
                                                           const int32_t* __restrict__ key_idx, float* __restrict__ R) {
  __shared__ __attribute__((aligned(16))) float s_f[P];  // 32 KB
  __shared__ uint32_t s_d[2][P / 4];                     // 16 KB: four int8 template values per word
  const int row = blockIdx.y, tid = threadIdx.x;
  int ki = key_idx[row];
  ki = ki < 0 ? 0 : (ki >= n_keys ? n_keys - 1 : ki);
  const float4* fv = reinterpret_cast<const float4*>(f + (int64_t)row * P);
  for (int v = tid; v < P / 4; v += WM_BLOCK) reinterpret_cast<float4*>(s_f)[v] = fv[v];
  const uint32_t* dv = reinterpret_cast<const uint32_t*>(dtab + (int64_t)ki * 2 * P);
  for (int v = tid; v < 2 * (P / 4); v += WM_BLOCK) (&s_d[0][0])[v] = dv[v];
  __syncthreads();

  const int o0 = blockIdx.x * CORR_TILE + tid;
  float acc0[CORR_PER] = {}, acc1[CORR_PER] = {};
  for (int n4 = 0; n4 < P / 4; ++n4) {
    const uint32_t w0 = s_d[0][n4], w1 = s_d[1][n4];  // (the same word for every lane: a broadcast)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d0 = (float)(int8_t)(w0 >> (8 * j)), d1 = (float)(int8_t)(w1 >> (8 * j));
      const int i = o0 + 4 * n4 + j;
#pragma unroll
      for (int q = 0; q < CORR_PER; ++q) {
        const float v = s_f[(i + q * WM_BLOCK) & (P - 1)];  // (consecutive lanes, consecutive words)
        acc0[q] = fmaf(v, d0, acc0[q]);
        acc1[q] = fmaf(v, d1, acc1[q]);
      }
    }
  }
  float* R0 = R + (int64_t)row * 2 * P;
#pragma unroll
  for (int q = 0; q < CORR_PER; ++q) {
    R0[o0 + q * WM_BLOCK] = acc0[q];
    R0[P + o0 + q * WM_BLOCK] = acc1[q];
  }
}

// out[row] = (o_0, o_1, z_0, z_1): one workgroup per (lane, row); the moments in float64 (8192 terms: nothing to save in fp32)
__global__ __launch_bounds__(WM_BLOCK) void wm_peak_kernel(const float* __restrict__ R, int32_t* __restrict__ out) {
  __shared__ double s_sum[WM_BLOCK];
  __shared__ float s_best[WM_BLOCK];
  __shared__ int s_idx[WM_BLOCK];
  const int l = blockIdx.x, row = blockIdx.y, tid = threadIdx.x;
  const float* Rl = R + ((int64_t)row * 2 + l) * P;
  double sum = 0.0;
  float best = Rl[tid];
  int idx = tid;
  for (int o = tid; o < P; o += WM_BLOCK) {  // (ascending: a lane keeps its lowest index on a tie)
    const float v = Rl[o];
    sum += (double)v;
    if (v > best) {
      best = v;
      idx = o;
    }
  }
  s_sum[tid] = sum;
  s_best[tid] = best;
  s_idx[tid] = idx;
  __syncthreads();
  for (int h = WM_BLOCK / 2; h > 0; h >>= 1) {
    if (tid < h) {
      s_sum[tid] += s_sum[tid + h];
      const float vb = s_best[tid + h];
      const int ib = s_idx[tid + h];
      if (vb > s_best[tid] || (vb == s_best[tid] && ib < s_idx[tid])) {
        s_best[tid] = vb;
        s_idx[tid] = ib;
      }
    }
    __syncthreads();
  }
  const double mean = s_sum[0] / (double)P;
  const float top = s_best[0];
  const int at = s_idx[0];
  __syncthreads();  // (s_sum is reused)
  double sq = 0.0;
  for (int o = tid; o < P; o += WM_BLOCK) {
    const double d = (double)Rl[o] - mean;
    sq += d * d;
  }
  s_sum[tid] = sq;
  __syncthreads();
  for (int h = WM_BLOCK / 2; h > 0; h >>= 1) {
    if (tid < h) s_sum[tid] += s_sum[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    const double var = s_sum[0] / (double)P;
    const float z = var > 0.0 ? (float)(((double)top - mean) / sqrt(var)) : 0.0f;
    out[row * 4 + l] = at;
    out[row * 4 + 2 + l] = __float_as_int(z);
  }
}

}  // namespace

int64_t sopro_wm_state_bytes(int32_t rows) { return rows <= 0 ? 0 : (int64_t)rows * STATE_WORDS * (int64_t)sizeof(int64_t); }

int64_t sopro_wm_chunk_out_cap(int64_t in_len) {
  if (in_len < 0 || in_len > LEN_MAX) return -1;
  return in_len + WM_TAIL;
}

int64_t sopro_wm_fold_ws_bytes(int32_t rows, int64_t in_cap) {
  if (rows <= 0 || in_cap < 0 || in_cap > LEN_MAX) return -1;
  return (int64_t)rows * fold_blocks(in_cap) * (int64_t)sizeof(float);
}

int sopro_wm_embed_rows_f32(const float* in, int64_t in_stride, const int32_t* in_lens, int64_t in_cap, const int32_t* car_idx, const int8_t* cars,
                            int32_t n_cars, const float* alphas, int32_t rows, void* state, int32_t flush, const float* tab, float* out,
                            int64_t out_stride, int64_t out_cap, int32_t* out_lens, void* stream) {
  SOPRO_CHECK_ARG(in_lens && car_idx && alphas && tab && out_lens, "in_lens, car_idx, alphas, tab, out_lens must be non-NULL");
  SOPRO_CHECK_ARG(rows > 0 && rows <= 65535, "0 < rows <= 65535");
  SOPRO_CHECK_ARG(n_cars >= 0 && (cars || n_cars == 0), "cars must be non-NULL when n_cars > 0");
  SOPRO_CHECK_ARG(in_cap >= 0 && in_cap <= LEN_MAX, "0 <= in_cap <= 2^30");
  SOPRO_CHECK_ARG(in || in_cap == 0, "in must be non-NULL when in_cap > 0");
  SOPRO_CHECK_ARG(in_stride >= 0 && out_stride >= 0, "strides >= 0");
  SOPRO_CHECK_ARG(out_cap >= 0 && out_cap <= INT32_MAX, "0 <= out_cap < 2^31");
  SOPRO_CHECK_ARG(out || out_cap == 0, "out must be non-NULL when out_cap > 0");
  SOPRO_CHECK_ARG(rows == 1 || out_cap == 0 || out_stride >= out_cap, "out_stride >= out_cap (rows must not overlap)");
  SOPRO_CHECK_ARG(state || flush, "a call without state is the whole row: flush must be set");
  SOPRO_CHECK_ARG(((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(cars)) & 3u) == 0,
                  "in, out, cars must be 4-byte aligned");
  SOPRO_CHECK_ARG((reinterpret_cast<uintptr_t>(state) & 7u) == 0, "state must be 8-byte aligned");
  const int64_t tiles = out_cap > 0 ? (out_cap + WM_TILE - 1) / WM_TILE : 1;
  hipLaunchKernelGGL(wm_embed_kernel, dim3((unsigned)tiles, (unsigned)rows), dim3(WM_BLOCK), 0, (hipStream_t)stream, in, in_stride, in_lens, in_cap,
                     car_idx, cars, n_cars, alphas, static_cast<const int64_t*>(state), flush ? 1 : 0, tab, out, out_stride, out_cap, out_lens);
  if (state)
    hipLaunchKernelGGL(wm_state_kernel, dim3(rows), dim3(STATE_BLOCK), 0, (hipStream_t)stream, in, in_stride, in_lens, in_cap,
                       static_cast<int64_t*>(state), flush ? 1 : 0, out_cap);
  SOPRO_LAUNCH_CHECK();
}

int sopro_wm_fold_rows_f32(const float* in, int64_t in_stride, const int32_t* in_lens, int64_t in_cap, int32_t rows, const float* tab, void* workspace,
                           float* f, void* stream) {
  SOPRO_CHECK_ARG(in_lens && tab && workspace && f, "in_lens, tab, workspace, f must be non-NULL");
  SOPRO_CHECK_ARG(rows > 0 && rows <= 65535, "0 < rows <= 65535");
  SOPRO_CHECK_ARG(in_cap >= 0 && in_cap <= LEN_MAX, "0 <= in_cap <= 2^30");
  SOPRO_CHECK_ARG(in || in_cap == 0, "in must be non-NULL when in_cap > 0");
  SOPRO_CHECK_ARG(in_stride >= 0, "in_stride >= 0");
  SOPRO_CHECK_ARG(((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(f)) & 3u) == 0,
                  "in, workspace, f must be 4-byte aligned");
  const int64_t nbk = fold_blocks(in_cap);
  hipLaunchKernelGGL(wm_blockmax_kernel, dim3((unsigned)((nbk + WAVES - 1) / WAVES), (unsigned)rows), dim3(WM_BLOCK), 0, (hipStream_t)stream, in,
                     in_stride, in_lens, in_cap, static_cast<float*>(workspace));
  hipLaunchKernelGGL(wm_fold_kernel, dim3(P / WM_BLOCK, (unsigned)rows), dim3(WM_BLOCK), 0, (hipStream_t)stream, in, in_stride, in_lens, in_cap, tab,
                     static_cast<const float*>(workspace), f);
  SOPRO_LAUNCH_CHECK();
}

int sopro_wm_corr_rows_f32(const float* f, const int8_t* dtab, int32_t n_keys, const int32_t* key_idx, int32_t rows, float* R, void* stream) {
  SOPRO_CHECK_ARG(f && dtab && key_idx && R, "f, dtab, key_idx, R must be non-NULL");
  SOPRO_CHECK_ARG(rows > 0 && rows <= 65535, "0 < rows <= 65535");
  SOPRO_CHECK_ARG(n_keys > 0, "n_keys > 0");
  SOPRO_CHECK_ARG(aligned16(f), "f must be 16-byte aligned");
  SOPRO_CHECK_ARG(((reinterpret_cast<uintptr_t>(dtab) | reinterpret_cast<uintptr_t>(R)) & 3u) == 0, "dtab, R must be 4-byte aligned");
  hipLaunchKernelGGL(wm_corr_kernel, dim3(P / CORR_TILE, (unsigned)rows), dim3(WM_BLOCK), 0, (hipStream_t)stream, f, dtab, n_keys, key_idx, R);
  SOPRO_LAUNCH_CHECK();
}

int sopro_wm_peak_rows_f32(const float* R, int32_t rows, int32_t* out, void* stream) {
  SOPRO_CHECK_ARG(R && out, "R, out must be non-NULL");
  SOPRO_CHECK_ARG(rows > 0 && rows <= 65535, "0 < rows <= 65535");
  hipLaunchKernelGGL(wm_peak_kernel, dim3(2, (unsigned)rows), dim3(WM_BLOCK), 0, (hipStream_t)stream, R, out);
  SOPRO_LAUNCH_CHECK();
}
