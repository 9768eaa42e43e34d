// Formant control: a warp of the spectral envelope on whole rows or on rows that arrive in chunks (contract: include/sopro_hip.h
// "formant control", DESIGN.md "Formants"; numpy restatement: tests/formant_ref.py).  A call is two launches per group of FM_GROUP rows:
//   frames - one wave per frame, everything between the samples and the synthesised frame on chip: the windowed 512 samples as 256
//            complex points, the radix-4 FFT and the real-input split of stft256.h; m(k) into LDS; 32 cepstral coefficients (lane =
//            coefficient and half of the bins, table cosines); L at the 257 bins (lane = bin, table cosines) and at k / sigma (cospi of
//            a reduced argument), the clamped gain, Y = X exp(g); the inverse split, the same FFT on the conjugate, 0.5 w
//   ola    - one workgroup per output hop gathers its four frames in ascending f (a row at sigma = 1 is copied instead)
// and, chunked, a third that writes the next state.  A frame's arithmetic depends on its 512 samples and the row's 1 / sigma only, not
// on where in a launch it runs: that is what makes the chunked form equal the one-shot one bit for bit.  Lengths and parameters are
// host values and travel as kernel arguments, so a call neither copies nor synchronises.
#include <math.h>

#include "common.h"
#include "stft256.h"

namespace {

using stft256::cmul;
using stft256::fft256;
using stft256::T_SPLIT;
using stft256::T_TW;
using stft256::T_WIN;
constexpr int N = SOPRO_FM_N, H = SOPRO_FM_H, NB = N / 2 + 1, Q = SOPRO_FM_Q;
constexpr int PRE = N - H;           // samples in front of the first one a call emits: zeros at a row's start
constexpr int STATE = SOPRO_FM_STATE;  // floats of one half of a row's state: PRE emitted samples and up to N - 1 held ones
constexpr int FM_GROUP = 64;         // rows of one launch group (their lengths and parameters are kernel arguments)
constexpr int FFT_BLOCK = 256, FFT_WAVES = FFT_BLOCK / 64, FFT_FRAMES = 4;  // frames per wave of one workgroup
constexpr int OLA_BLOCK = H, UPD_BLOCK = 256;
constexpr int64_t LEN_MAX = (int64_t)1 << 24;
static_assert(N == stft256::N && H == stft256::H && Q == 32, "the transform is 256 complex points on 64 lanes; a lane pair per coefficient");
static_assert(STATE >= PRE + N - 1, "a half of the state holds the history and what is held back");

// tables: stft256's | cos(2 pi i / 512) [512] | l_q (q ? 2 : 1) / 512 [32], made in float64 on the host
constexpr int T_COS = stft256::T_FLOATS, T_LIFT = T_COS + N, T_FLOATS = T_LIFT + Q;
__device__ float g_fm_tab[T_FLOATS];

struct Rows {
  int32_t hlen[FM_GROUP];   // samples the state's current half holds in front of the chunk (PRE zeros without a state)
  int32_t n_new[FM_GROUP];  // samples of the chunk
  int32_t n_out[FM_GROUP];  // samples the call emits
  float inv[FM_GROUP];      // 1 / sigma; 1: the row is copied
};

__host__ __device__ __forceinline__ int64_t frames_of(int64_t n) { return n > 0 ? (n + H - 1) / H + 3 : 0; }

// Sample s >= 0 of the row as the call sees it: the state's samples (zeros without a state), the chunk, zeros.
__device__ __forceinline__ float fetch(const float* hist, int hlen, const float* x, int n_new, int64_t s) {
  if (s < hlen) return hist ? hist[s] : 0.0f;
  s -= hlen;
  return s < n_new ? x[s] : 0.0f;
}

// ---- frames ----
__global__ __launch_bounds__(FFT_BLOCK) void fm_frames_kernel(const float* __restrict__ wav, int64_t row_stride, const float* __restrict__ state,
                                                              int phase, Rows rows, int row0, float* __restrict__ ws, int64_t fcap) {
  __shared__ float s_tab[T_FLOATS];
  __shared__ float2 s_buf[FFT_WAVES][NB + 1];
  __shared__ float s_m[FFT_WAVES][NB + 3], s_L[FFT_WAVES][NB + 3], s_c[FFT_WAVES][Q];
  for (int i = threadIdx.x; i < T_FLOATS; i += FFT_BLOCK) s_tab[i] = g_fm_tab[i];
  __syncthreads();
  const int r = blockIdx.y, j = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n_out = rows.n_out[r], hlen = rows.hlen[r], n_new = rows.n_new[r];
  const float inv = rows.inv[r];
  if (n_out <= 0 || inv == 1.0f) return;
  const int64_t F = frames_of(n_out);
  const float* x = wav + (int64_t)(row0 + r) * row_stride;
  const float* hist = state ? state + ((int64_t)(row0 + r) * 2 + phase) * STATE : nullptr;
  float* fr = ws + (int64_t)(row0 + r) * fcap * N;
  const float* win = s_tab + T_WIN;
  const float2* tw = reinterpret_cast<const float2*>(s_tab + T_TW);
  const float2* sp = reinterpret_cast<const float2*>(s_tab + T_SPLIT);
  const float* ct = s_tab + T_COS;
  const float* lift = s_tab + T_LIFT;
  float2* buf = s_buf[wv];
  float *m = s_m[wv], *L = s_L[wv], *c = s_c[wv];
  for (int q4 = 0; q4 < FFT_FRAMES; ++q4) {
    const int64_t f = ((int64_t)blockIdx.x * FFT_FRAMES + q4) * FFT_WAVES + wv;
    if (f >= F) break;  // (uniform over the wave)
    float2 v[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int i = 2 * (j + 64 * t);
      const int64_t s = f * H + i;
      v[t] = make_float2(fetch(hist, hlen, x, n_new, s) * win[i], fetch(hist, hlen, x, n_new, s + 1) * win[i + 1]);
    }
    fft256(v, buf, tw, j);
    wave_lds_sync();
#pragma unroll
    for (int t = 0; t < 4; ++t) buf[j + 64 * t] = v[t];
    wave_lds_sync();
    // X[k] = E[k] + exp(-2 pi i k / 512) O[k]; E = (Z[k] + conj Z[256 - k]) / 2, O = (Z[k] - conj Z[256 - k]) / 2i.  Lane j keeps
    // bins j + 64 t, t = 0..3, and (lane 0) bin 256.
    float2 X[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      const int k = j + 64 * t;
      X[t] = make_float2(0.0f, 0.0f);
      if (k < NB) {
        const float2 zk = buf[k & 255], zc = buf[(256 - k) & 255];
        const float2 E = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y - zc.y));
        const float2 O = make_float2(0.5f * (zk.y + zc.y), 0.5f * (zc.x - zk.x));
        const float2 p = cmul(sp[k], O);
        X[t] = make_float2(E.x + p.x, E.y + p.y);
        m[k] = 0.5f * logf(X[t].x * X[t].x + X[t].y * X[t].y + SOPRO_FM_EPS);
      }
    }
    wave_lds_sync();
    // c_q, lane = (q, half): the half's bins 1 + half, 3 + half, .. < 256 in ascending order, then the other half's sum
    {
      const int q = j & (Q - 1), half = j >> 5;
      float acc = 0.0f;
      for (int k = 1 + half; k < N / 2; k += 2) acc = fmaf(m[k], ct[(q * k) & (N - 1)], acc);
      acc += __shfl_xor(acc, 32, 64);
      const float ends = m[0] + ((q & 1) ? -m[N / 2] : m[N / 2]);
      if (half == 0) c[q] = (ends + 2.0f * acc) * lift[q];  // l_q c_q, doubled for q >= 1
    }
    wave_lds_sync();
    float cq[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) cq[q] = c[q];
    // L at the bins
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      const int k = j + 64 * t;
      if (k < NB) {
        float a = 0.0f;
#pragma unroll
        for (int q = 0; q < Q; ++q) a = fmaf(cq[q], ct[(q * k) & (N - 1)], a);
        L[k] = a;
      }
    }
    wave_lds_sync();
    // L at k / sigma, the gain, Y -> buf
    const float L_top = L[N / 2];
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      const int k = j + 64 * t;
      if (k < NB) {
        const float kf = (float)k, hi = kf * inv, lo = fmaf(kf, inv, -hi);  // k inv = hi + lo exactly
        float Lw = L_top;
        if (hi < (float)(N / 2)) {
          const float fl = floorf(hi);
          const int xi = (int)fl;
          const float xf = (hi - fl) + lo;
          float a = 0.0f;
#pragma unroll
          for (int q = 0; q < Q; ++q) a = fmaf(cq[q], cospif((float)((q * xi) & (N - 1)) * (2.0f / N) + (float)q * xf * (2.0f / N)), a);
          Lw = a;
        }
        const float g = fminf(fmaxf(Lw - L[k], -SOPRO_FM_GAIN_MAX), SOPRO_FM_GAIN_MAX);
        const float e = expf(g);
        buf[k] = make_float2(X[t].x * e, X[t].y * e);
      }
    }
    wave_lds_sync();
    // Z[k] = E[k] + i O[k]; E = (Y[k] + conj Y[256 - k]) / 2, O = exp(+2 pi i k / 512) (Y[k] - conj Y[256 - k]) / 2.  The inverse
    // transform is the forward one between two conjugations; the imaginary parts of Y[0] and Y[256] drop out, as in an irfft.
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = j + 64 * t;
      float2 yk = buf[k], yc = buf[256 - k];
      if (k == 0) yk.y = 0.0f, yc.y = 0.0f;
      const float2 E = make_float2(0.5f * (yk.x + yc.x), 0.5f * (yk.y - yc.y));
      const float2 D = make_float2(0.5f * (yk.x - yc.x), 0.5f * (yk.y + yc.y));
      const float2 O = cmul(make_float2(sp[k].x, -sp[k].y), D);
      v[t] = make_float2(E.x - O.y, -(E.y + O.x));  // conj(E + i O)
    }
    fft256(v, buf, tw, j);
    // z[i] = conj(v) / 256 holds samples 2 i and 2 i + 1; the frame is 0.5 w irdft
    float2* y = reinterpret_cast<float2*>(fr + f * N);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int i = j + 64 * t;
      y[i] = make_float2(v[t].x * (1.0f / 256.0f) * win[2 * i] * 0.5f, -v[t].y * (1.0f / 256.0f) * win[2 * i + 1] * 0.5f);
    }
    wave_lds_sync();  // (the next frame writes buf, m, L and c)
  }
}

// ---- ola ----
__global__ __launch_bounds__(OLA_BLOCK) void fm_ola_kernel(const float* __restrict__ wav, int64_t row_stride, const float* __restrict__ state,
                                                           int phase, Rows rows, int row0, const float* __restrict__ ws, int64_t fcap,
                                                           float* __restrict__ out, int64_t out_stride) {
  const int r = blockIdx.y, o = threadIdx.x;
  const int64_t hb = blockIdx.x, i = hb * H + o;
  if (i >= rows.n_out[r]) return;
  float y;
  if (rows.inv[r] == 1.0f) {
    const float* hist = state ? state + ((int64_t)(row0 + r) * 2 + phase) * STATE : nullptr;
    y = fetch(hist, rows.hlen[r], wav + (int64_t)(row0 + r) * row_stride, rows.n_new[r], PRE + i);
  } else {
    const float* fr = ws + ((int64_t)(row0 + r) * fcap + hb) * N + o;  // sample PRE + i lies in frames hb .. hb + 3
    y = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; ++t) y += fr[t * N + (3 - t) * H];
  }
  out[(int64_t)(row0 + r) * out_stride + i] = y;
}

// ---- the next state ----
__global__ __launch_bounds__(UPD_BLOCK) void fm_update_kernel(const float* __restrict__ wav, int64_t row_stride, float* __restrict__ state, int phase,
                                                              Rows rows, int row0, int flush) {
  const int r = blockIdx.x;
  const int hlen = rows.hlen[r], n_new = rows.n_new[r], n_out = rows.n_out[r];
  const float* hist = state + ((int64_t)(row0 + r) * 2 + phase) * STATE;
  float* next = state + ((int64_t)(row0 + r) * 2 + (phase ^ 1)) * STATE;
  const int keep = flush ? PRE : hlen + n_new - n_out;  // (the host has checked keep <= STATE)
  for (int i = threadIdx.x; i < keep; i += UPD_BLOCK)
    next[i] = flush ? 0.0f : fetch(hist, hlen, wav + (int64_t)(row0 + r) * row_stride, n_new, (int64_t)n_out + i);
}

// The tables of the device the call runs on: float64 on the host, rounded once, uploaded once (two threads racing on the first call
// both upload the same bytes).
int upload_tables() {
  static unsigned char done[64] = {};
  static float host[T_FLOATS];
  static bool made = false;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  if (done[dev & 63]) return 0;
  if (!made) {
    const double pi = 3.14159265358979323846;
    stft256::make_tables(host);
    for (int i = 0; i < N; ++i) host[T_COS + i] = (float)cos(2.0 * pi * i / N);
    for (int q = 0; q < Q; ++q) host[T_LIFT + q] = (float)(0.5 * (1.0 + cos(pi * q / Q)) * (q ? 2.0 : 1.0) / N);
    made = true;
  }
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_fm_tab), host, sizeof(host)) != hipSuccess) return -1;
  done[dev & 63] = 1;
  return 0;
}

}  // namespace

int64_t sopro_formant_workspace_bytes(int32_t rows, int64_t cap) {
  if (rows <= 0 || cap < 0 || cap > LEN_MAX) return -1;
  return (int64_t)rows * frames_of(cap) * N * (int64_t)sizeof(float);
}

int64_t sopro_formant_state_bytes(int32_t rows) { return rows > 0 ? (int64_t)rows * 2 * STATE * (int64_t)sizeof(float) : -1; }

int64_t sopro_formant_chunk_out_cap(int64_t n) { return n >= 0 ? n + N : -1; }

int sopro_formant_rows_f32(const float* wav, int64_t row_stride, const int32_t* lens, const float* inv, int32_t rows, void* state,
                           const int32_t* held, int32_t phase, int32_t flush, float* out, int64_t out_stride, int64_t out_cap,
                           int32_t* out_lens, void* ws, int64_t ws_bytes, void* stream) {
  SOPRO_CHECK_ARG(lens && inv, "lens, inv must be non-NULL (host arrays)");
  SOPRO_CHECK_ARG(rows > 0 && rows <= 65535, "0 < rows <= 65535");
  SOPRO_CHECK_ARG(!state || held, "held must be non-NULL with a state (host array)");
  SOPRO_CHECK_ARG(phase == 0 || phase == 1, "phase is 0 or 1");
  SOPRO_CHECK_ARG(out_cap >= 0, "out_cap >= 0");
  int64_t in_cap = 0, cap = 0;
  bool any = false;
  for (int b = 0; b < rows; ++b) {
    SOPRO_CHECK_ARG(lens[b] >= 0 && lens[b] <= LEN_MAX, "0 <= lens[b] <= 2^24");
    SOPRO_CHECK_ARG(inv[b] >= 0.5f && inv[b] <= 2.0f, "0.5 <= inv[b] <= 2 (1: the row is copied)");
    SOPRO_CHECK_ARG(!state || (held[b] >= 0 && held[b] < N), "0 <= held[b] < 512");
    const int64_t have = (state ? held[b] : 0) + (int64_t)lens[b];
    const int64_t n_out = (state && !flush) ? (have / H > 3 ? (have / H - 3) * H : 0) : have;
    SOPRO_CHECK_ARG(n_out <= out_cap, "out_lens[b] <= out_cap");
    in_cap = lens[b] > in_cap ? lens[b] : in_cap;
    cap = n_out > cap ? n_out : cap;
    any = any || (n_out > 0 && inv[b] != 1.0f);
  }
  SOPRO_CHECK_ARG(in_cap == 0 || wav, "wav must be non-NULL when a row has samples");
  SOPRO_CHECK_ARG(cap == 0 || out, "out must be non-NULL when a row emits samples");
  SOPRO_CHECK_ARG(row_stride >= 0 && out_stride >= 0, "strides >= 0");
  SOPRO_CHECK_ARG(rows == 1 || (row_stride >= in_cap && out_stride >= cap), "row_stride >= max(lens), out_stride >= max(out_lens) (rows must not overlap)");
  SOPRO_CHECK_ARG(((reinterpret_cast<uintptr_t>(wav) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(state)) & 3u) == 0,
                  "wav, out, state must be 4-byte aligned");
  SOPRO_CHECK_ARG(ws && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0, "ws must be non-NULL and 8-byte aligned");
  SOPRO_CHECK_ARG(ws_bytes >= sopro_formant_workspace_bytes(rows, cap), "ws_bytes < sopro_formant_workspace_bytes(rows, max(out_lens))");
  if (any && upload_tables() != 0) {
    sopro_set_error("%s: the table upload failed", __func__);
    return -1;
  }
  hipStream_t s = (hipStream_t)stream;
  const float* st = static_cast<const float*>(state);
  const int64_t fcap = frames_of(cap);
  for (int row0 = 0; row0 < rows; row0 += FM_GROUP) {
    const int nr = rows - row0 < FM_GROUP ? rows - row0 : FM_GROUP;
    Rows g = {};
    int64_t gcap = 0, gf = 0;
    for (int r = 0; r < nr; ++r) {
      const int b = row0 + r;
      const int64_t have = (state ? held[b] : 0) + (int64_t)lens[b];
      const int64_t n_out = (state && !flush) ? (have / H > 3 ? (have / H - 3) * H : 0) : have;
      g.hlen[r] = PRE + (state ? held[b] : 0);
      g.n_new[r] = lens[b];
      g.n_out[r] = (int32_t)n_out;
      g.inv[r] = inv[b];
      if (out_lens) out_lens[b] = (int32_t)n_out;
      gcap = n_out > gcap ? n_out : gcap;
      if (inv[b] != 1.0f && frames_of(n_out) > gf) gf = frames_of(n_out);
    }
    if (gf > 0) {
      const unsigned fb = (unsigned)((gf + FFT_WAVES * FFT_FRAMES - 1) / (FFT_WAVES * FFT_FRAMES));
      hipLaunchKernelGGL(fm_frames_kernel, dim3(fb, (unsigned)nr), dim3(FFT_BLOCK), 0, s, wav, row_stride, st, phase, g, row0, static_cast<float*>(ws),
                         fcap);
    }
    if (gcap > 0)
      hipLaunchKernelGGL(fm_ola_kernel, dim3((unsigned)((gcap + H - 1) / H), (unsigned)nr), dim3(OLA_BLOCK), 0, s, wav, row_stride, st, phase, g, row0,
                         static_cast<const float*>(ws), fcap, out, out_stride);
    if (state)
      hipLaunchKernelGGL(fm_update_kernel, dim3((unsigned)nr), dim3(UPD_BLOCK), 0, s, wav, row_stride, static_cast<float*>(state), phase, g, row0,
                         flush ? 1 : 0);
  }
  SOPRO_LAUNCH_CHECK();
}
