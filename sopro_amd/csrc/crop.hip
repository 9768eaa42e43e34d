// Reference crop selection: the window of a reference waveform with the most speech and the least clipping (contract:
// include/sopro_hip.h "reference crop selection", DESIGN.md "Reference crop selection"; numpy restatement: tests/crop_ref.py).  A call
// is three launches per group of CR_GROUP rows:
//   blocks - one wave per block of H samples: four coalesced dword loads per lane (the row start, the stride and the grid offset have
//            any alignment), the lane's squares added in ascending sample order, one fixed cross-lane tree; e[f] and the clip flag
//   pick   - one workgroup per row: Emax and the smoothed floor by strided walks and an LDS reduction, the threshold, a[f], a chunked
//            workgroup-wide integer prefix sum of a - clip_weight c into the workspace, a max-reduction over the candidates on one
//            packed key (score, -|k - k_c|, -k), then the counts and the level of the chosen and the centre window; starts[b], report
//   gather - copies the chosen window; the start is read from device memory, so the call copies nothing to the host
// A block's energy depends on its own samples only and everything after it is integer or an order-free max / min, so a row has the
// same bits alone and in a batch, and two calls give the same bits.  The row lengths and parameters are host values and travel as
// kernel arguments: a call neither copies nor synchronises.
#include <math.h>

#include "common.h"

namespace {

constexpr int H = SOPRO_CROP_H;
constexpr int CR_GROUP = 64;                    // rows of one launch group (their lengths and parameters are kernel arguments)
constexpr int BLK_BLOCK = 256, BLK_WAVES = BLK_BLOCK / 64;
constexpr int PICK_BLOCK = 256, PICK_WAVES = PICK_BLOCK / 64;
constexpr int SCAN_ITEMS = 4, SCAN_CHUNK = PICK_BLOCK * SCAN_ITEMS;  // blocks of one round of the prefix sum
constexpr int GATHER_BLOCK = 256, GATHER_ITEMS = 4;
constexpr int64_t LEN_MAX = (int64_t)1 << 24;
constexpr int REPORT_WORDS = SOPRO_CROP_REPORT_WORDS;
static_assert(H == 240, "lane j of a block's wave loads samples j, j + 64, j + 128 and (j < 48) j + 192");
// the packed key: score + 2^23 in the high bits, then 2^18 - |k - k_c|, then 2^18 - k
static_assert(SOPRO_CROP_WEIGHT_MAX * (LEN_MAX / H) < (1 << 23) && LEN_MAX / H < (1 << 18), "the key's fields hold every row");

struct Rows {
  int32_t n[CR_GROUP];
  float range_lin[CR_GROUP];   // 10^(-range_db / 10)
  float margin_lin[CR_GROUP];  // 10^(margin_db / 10)
  float clip[CR_GROUP];        // 0: the row is not searched
  int32_t weight[CR_GROUP];
};

// The block grid of a row of n samples under a window of win: o, F, the blocks of a window, the centre candidate
struct Grid {
  int32_t o, F, Wb, kc, sc;
  bool lng;
};
__host__ __device__ __forceinline__ Grid grid_of(int32_t n, int32_t win) {
  Grid g;
  g.lng = n > win;
  g.sc = g.lng ? (n - win) / 2 : 0;
  g.o = g.sc % H;
  g.F = (n - g.o) / H;
  g.Wb = g.lng ? win / H : g.F;
  g.kc = (g.sc - g.o) / H;
  return g;
}

__host__ __device__ __forceinline__ int64_t blocks_cap(int64_t cap) { return cap / H; }
// workspace of one row, in 32-bit words: e [Fc] | flags [Fc] | prefix sums [Fc + 1]
__host__ __device__ __forceinline__ int64_t row_words(int64_t cap) { return 3 * blocks_cap(cap) + 1; }
struct Ws {
  float* e;
  uint32_t* flags;
  int32_t* pre;
};
__device__ __forceinline__ Ws ws_of(void* ws, int64_t row, int64_t cap) {
  const int64_t Fc = blocks_cap(cap);
  Ws w;
  w.e = static_cast<float*>(ws) + row * row_words(cap);
  w.flags = reinterpret_cast<uint32_t*>(w.e + Fc);
  w.pre = reinterpret_cast<int32_t*>(w.e + 2 * Fc);
  return w;
}

// ---- blocks ----
__global__ __launch_bounds__(BLK_BLOCK) void crop_blocks_kernel(const float* __restrict__ wav, int64_t row_stride, Rows rows, int row0, int32_t win,
                                                                void* __restrict__ ws, int64_t cap) {
  const int r = blockIdx.y, j = threadIdx.x & 63;
  const float clip = rows.clip[r];
  if (clip == 0.0f) return;
  const Grid g = grid_of(rows.n[r], win);
  const int32_t f = (int32_t)blockIdx.x * BLK_WAVES + (threadIdx.x >> 6);
  if (f >= g.F) return;  // (uniform over the wave)
  const float* x = wav + (int64_t)(row0 + r) * row_stride + g.o + (int64_t)f * H;
  const float v0 = x[j], v1 = x[j + 64], v2 = x[j + 128], v3 = j < H - 192 ? x[j + 192] : 0.0f;
  float s = v0 * v0;
  s = fmaf(v1, v1, s);
  s = fmaf(v2, v2, s);
  s = fmaf(v3, v3, s);
  s = wave_sum(s);
  const float peak = fmaxf(fmaxf(fabsf(v0), fabsf(v1)), fmaxf(fabsf(v2), fabsf(v3)));
  const bool hit = __ballot(peak >= clip) != 0ull;
  if (j == 0) {
    const Ws w = ws_of(ws, row0 + r, cap);
    w.e[f] = s;
    w.flags[f] = hit ? 2u : 0u;
  }
}

// ---- pick ----
template <class T, class Op>
__device__ __forceinline__ T block_reduce(T v, T* s, Op op) {
  const int t = threadIdx.x;
  __syncthreads();  // (the earlier readers of s are done)
  s[t] = v;
  __syncthreads();
  for (int d = PICK_BLOCK / 2; d > 0; d >>= 1) {
    if (t < d) s[t] = op(s[t], s[t + d]);
    __syncthreads();
  }
  return s[0];
}

__global__ __launch_bounds__(PICK_BLOCK) void crop_pick_kernel(Rows rows, int row0, int32_t win, void* __restrict__ ws, int64_t cap,
                                                               int32_t* __restrict__ starts, int32_t* __restrict__ report,
                                                               uint32_t* __restrict__ blocks) {
  __shared__ double s_red[PICK_BLOCK];  // every reduction's scratch (float, uint64, int and double views of it)
  __shared__ int s_wave[PICK_WAVES];
  const int r = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t row = row0 + r;
  int32_t* rep = report ? report + REPORT_WORDS * row : nullptr;
  const float clip = rows.clip[r];
  const Grid g = grid_of(rows.n[r], win);
  if (clip == 0.0f || g.F == 0) {  // not searched, or no complete block: the head of the row, an empty report
    if (t == 0) starts[row] = 0;
    if (rep && t < REPORT_WORDS) rep[t] = t == REPORT_WORDS - 1 ? __float_as_int(-200.0f) : 0;
    return;
  }
  const int32_t F = g.F, Wb = g.Wb, kc = g.kc;
  const Ws w = ws_of(ws, row, cap);
  // the threshold
  float emax = 0.0f, emin = INFINITY;
  for (int32_t f = t; f < F; f += PICK_BLOCK) emax = fmaxf(emax, w.e[f]);
  if (F >= SOPRO_CROP_SMOOTH) {
    for (int32_t f = t; f + SOPRO_CROP_SMOOTH <= F; f += PICK_BLOCK) {
      float s5 = w.e[f];
#pragma unroll
      for (int u = 1; u < SOPRO_CROP_SMOOTH; ++u) s5 += w.e[f + u];
      emin = fminf(emin, s5 / (float)SOPRO_CROP_SMOOTH);
    }
  } else {
    for (int32_t f = t; f < F; f += PICK_BLOCK) emin = fminf(emin, w.e[f]);
  }
  emax = block_reduce(emax, reinterpret_cast<float*>(s_red), [](float a, float b) { return fmaxf(a, b); });
  emin = block_reduce(emin, reinterpret_cast<float*>(s_red), [](float a, float b) { return fminf(a, b); });
  const float thr = fmaxf(emax * rows.range_lin[r], emin * rows.margin_lin[r]);
  // a[f], and the prefix sums of a - weight c: pre[0] = 0, pre[f + 1] = pre[f] + a[f] - weight c[f]
  const int32_t weight = rows.weight[r];
  uint32_t* blk_e = blocks ? blocks + 2 * blocks_cap(cap) * row : nullptr;  // e [Fc] | flags [Fc]
  uint32_t* blk_f = blocks ? blk_e + blocks_cap(cap) : nullptr;
  int32_t carry = 0, n_act = 0;
  if (t == 0) w.pre[0] = 0;
  for (int32_t base = 0; base < F; base += SCAN_CHUNK) {
    const int32_t f0 = base + t * SCAN_ITEMS;
    int32_t run[SCAN_ITEMS], tot = 0;
#pragma unroll
    for (int u = 0; u < SCAN_ITEMS; ++u) {
      if (f0 + u < F) {
        const float e = w.e[f0 + u];
        const uint32_t c = w.flags[f0 + u] & 2u, a = e > thr ? 1u : 0u;
        w.flags[f0 + u] = c | a;
        if (blocks) blk_e[f0 + u] = __float_as_uint(e), blk_f[f0 + u] = c | a;
        n_act += (int32_t)a;
        tot += (int32_t)a - (c ? weight : 0);
      }
      run[u] = tot;
    }
    int32_t incl = tot;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int32_t up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    __syncthreads();  // (the last round's readers of s_wave are done)
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    int32_t before = carry, all = 0;
#pragma unroll
    for (int q = 0; q < PICK_WAVES; ++q) {
      if (q < wv) before += s_wave[q];
      all += s_wave[q];
    }
    before += incl - tot;
#pragma unroll
    for (int u = 0; u < SCAN_ITEMS; ++u)
      if (f0 + u < F) w.pre[f0 + u + 1] = before + run[u];
    carry += all;
  }
  __syncthreads();  // pre[] and flags[] are read by other threads from here on
  // the candidates
  unsigned long long best = 0ull;
  for (int32_t k = t; k + Wb <= F; k += PICK_BLOCK) {
    const int32_t score = w.pre[k + Wb] - w.pre[k], d = k > kc ? k - kc : kc - k;
    const unsigned long long key = ((unsigned long long)(score + (1 << 23)) << 40) | ((unsigned long long)((1 << 18) - d) << 20) |
                                   (unsigned long long)((1 << 18) - k);
    best = key > best ? key : best;
  }
  best = block_reduce(best, reinterpret_cast<unsigned long long*>(s_red),
                      [](unsigned long long a, unsigned long long b) { return a > b ? a : b; });
  const int32_t kb = (1 << 18) - (int32_t)(best & 0xfffffull);
  const int32_t start = g.lng ? g.o + kb * H : 0;
  if (t == 0) starts[row] = start;
  if (!rep) return;  // (uniform)
  // the report: counts of the chosen and the centre window, the row's active blocks, the chosen window's level
  int32_t cnt[4] = {0, 0, 0, 0};
  double lvl = 0.0;
  for (int32_t i = t; i < Wb; i += PICK_BLOCK) {
    const uint32_t fb = w.flags[kb + i], fc = w.flags[kc + i];
    cnt[0] += (int32_t)(fb & 1u), cnt[1] += (int32_t)(fb >> 1), cnt[2] += (int32_t)(fc & 1u), cnt[3] += (int32_t)(fc >> 1);
    lvl += (double)w.e[kb + i];
  }
  auto add = [](int32_t a, int32_t b) { return a + b; };
#pragma unroll
  for (int q = 0; q < 4; ++q) cnt[q] = block_reduce(cnt[q], reinterpret_cast<int32_t*>(s_red), add);
  n_act = block_reduce(n_act, reinterpret_cast<int32_t*>(s_red), add);
  lvl = block_reduce(lvl, s_red, [](double a, double b) { return a + b; });  // a fixed tree over fixed strided partial sums
  if (t == 0) {
    rep[0] = start, rep[1] = cnt[0], rep[2] = cnt[1], rep[3] = cnt[2], rep[4] = cnt[3], rep[5] = n_act, rep[6] = F;
    rep[7] = __float_as_int((float)(10.0 * log10(lvl / (double)win + 1e-20)));
  }
}

// ---- gather ----
__global__ __launch_bounds__(GATHER_BLOCK) void crop_gather_kernel(const float* __restrict__ wav, int64_t row_stride, Rows rows, int row0, int32_t win,
                                                                   const int32_t* __restrict__ starts, float* __restrict__ out, int64_t out_stride) {
  const int r = blockIdx.y;
  const int32_t n = rows.n[r], len = n < win ? n : win;
  const int64_t row = row0 + r;
  const float* x = wav + row * row_stride + starts[row];
  float* y = out + row * out_stride;
  const int32_t i0 = (int32_t)blockIdx.x * (GATHER_BLOCK * GATHER_ITEMS) + threadIdx.x;
  float v[GATHER_ITEMS];
#pragma unroll
  for (int u = 0; u < GATHER_ITEMS; ++u) v[u] = i0 + u * GATHER_BLOCK < len ? x[i0 + u * GATHER_BLOCK] : 0.0f;
#pragma unroll
  for (int u = 0; u < GATHER_ITEMS; ++u)
    if (i0 + u * GATHER_BLOCK < len) y[i0 + u * GATHER_BLOCK] = v[u];
}

}  // namespace

int64_t sopro_crop_workspace_bytes(int32_t rows, int64_t cap) {
  if (rows <= 0 || cap < 0 || cap > LEN_MAX) return -1;
  return (int64_t)rows * row_words(cap) * (int64_t)sizeof(int32_t);
}

int sopro_crop_rows_f32(const float* wav, int64_t row_stride, const int32_t* lens, const float* params, int32_t rows, int32_t win, float* out,
                        int64_t out_stride, int32_t* starts, int32_t* report, void* blocks, void* ws, int64_t ws_bytes, void* stream) {
  SOPRO_CHECK_ARG(lens && params && starts, "lens, params (host arrays) and starts must be non-NULL");
  SOPRO_CHECK_ARG(rows > 0 && rows <= 65535, "0 < rows <= 65535");
  SOPRO_CHECK_ARG(win > 0 && win % H == 0 && win <= LEN_MAX, "win must be a positive multiple of 240, at most 2^24");
  int64_t cap = 0;
  for (int b = 0; b < rows; ++b) {
    SOPRO_CHECK_ARG(lens[b] >= 0 && lens[b] <= LEN_MAX, "0 <= lens[b] <= 2^24");
    cap = lens[b] > cap ? lens[b] : cap;
    const float *p = params + 4 * b, level = p[2];
    if (level == 0.0f) continue;  // the row is not searched
    SOPRO_CHECK_ARG(p[0] >= SOPRO_CROP_RANGE_MIN && p[0] <= SOPRO_CROP_RANGE_MAX, "6 <= range_db <= 80");
    SOPRO_CHECK_ARG(p[1] >= SOPRO_CROP_MARGIN_MIN && p[1] <= SOPRO_CROP_MARGIN_MAX, "0 <= margin_db <= 40");
    SOPRO_CHECK_ARG(level > 0.0f && level <= SOPRO_CROP_LEVEL_MAX, "0 < clip_level <= 8 (0: the row is not searched)");
    SOPRO_CHECK_ARG(p[3] >= 0.0f && p[3] <= (float)SOPRO_CROP_WEIGHT_MAX && p[3] == floorf(p[3]), "clip_weight must be an integer in 0 .. 64");
  }
  SOPRO_CHECK_ARG(cap == 0 || (wav && out), "wav, out must be non-NULL when a row has samples");
  SOPRO_CHECK_ARG(row_stride >= 0 && out_stride >= 0, "strides >= 0");
  SOPRO_CHECK_ARG(rows == 1 || (row_stride >= cap && out_stride >= (cap < win ? cap : win)),
                  "row_stride >= max(lens) and out_stride >= min(max(lens), win) (rows must not overlap)");
  SOPRO_CHECK_ARG(((reinterpret_cast<uintptr_t>(wav) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(starts) |
                    reinterpret_cast<uintptr_t>(report) | reinterpret_cast<uintptr_t>(blocks)) & 3u) == 0,
                  "wav, out, starts, report, blocks must be 4-byte aligned");
  SOPRO_CHECK_ARG(ws && (reinterpret_cast<uintptr_t>(ws) & 3u) == 0, "ws must be non-NULL and 4-byte aligned");
  SOPRO_CHECK_ARG(ws_bytes >= sopro_crop_workspace_bytes(rows, cap), "ws_bytes < sopro_crop_workspace_bytes(rows, max(lens))");
  hipStream_t s = (hipStream_t)stream;
  for (int row0 = 0; row0 < rows; row0 += CR_GROUP) {
    const int nr = rows - row0 < CR_GROUP ? rows - row0 : CR_GROUP;
    Rows g = {};
    int32_t gcap = 0, fcap = 0;
    for (int r = 0; r < nr; ++r) {
      const float* p = params + 4 * (row0 + r);
      g.n[r] = lens[row0 + r];
      g.clip[r] = p[2];
      if (p[2] != 0.0f) {
        g.range_lin[r] = (float)pow(10.0, -(double)p[0] / 10.0);
        g.margin_lin[r] = (float)pow(10.0, (double)p[1] / 10.0);
        g.weight[r] = (int32_t)p[3];
        const int32_t F = grid_of(g.n[r], win).F;
        fcap = F > fcap ? F : fcap;
      }
      gcap = g.n[r] > gcap ? g.n[r] : gcap;
    }
    if (fcap > 0)
      hipLaunchKernelGGL(crop_blocks_kernel, dim3((unsigned)((fcap + BLK_WAVES - 1) / BLK_WAVES), (unsigned)nr), dim3(BLK_BLOCK), 0, s, wav, row_stride,
                         g, row0, win, ws, cap);
    hipLaunchKernelGGL(crop_pick_kernel, dim3((unsigned)nr), dim3(PICK_BLOCK), 0, s, g, row0, win, ws, cap, starts, report,
                       static_cast<uint32_t*>(blocks));
    const int32_t glen = gcap < win ? gcap : win;
    if (glen > 0)
      hipLaunchKernelGGL(crop_gather_kernel, dim3((unsigned)((glen + GATHER_BLOCK * GATHER_ITEMS - 1) / (GATHER_BLOCK * GATHER_ITEMS)), (unsigned)nr),
                         dim3(GATHER_BLOCK), 0, s, wav, row_stride, g, row0, win, starts, out, out_stride);
  }
  SOPRO_LAUNCH_CHECK();
}
