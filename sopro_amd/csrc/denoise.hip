// Reference denoising: a stationary-noise suppressor on whole rows (contract: include/sopro_hip.h "reference denoising", DESIGN.md
// "Reference denoising"; numpy restatement: tests/denoise_ref.py).  A call is five launches per group of DN_GROUP rows:
//   analysis - one wave per frame: the windowed 512 real samples as 256 complex points, a radix-4 Stockham FFT (four stages, one
//              butterfly per lane and stage, exchanges through the wave's LDS slice), the real-input split pass; X[f][0..256]
//   track    - one lane per (row, bin), three walks over the frames: S and the block prefix minima (ascending), the block suffix
//              minima (descending), then M = min(suffix, prefix), the decision-directed gain and X *= G in place (ascending).  The
//              operands of a walk do not depend on its recurrence: they are loaded DN_AHEAD frames at a time, then the steps run
//   synth    - one wave per frame: the inverse split pass, the same FFT on the conjugate, 0.5 w; the 512 samples of the frame
//              overwrite the frame's own spectrum (514 floats)
//   ola      - one workgroup per output hop gathers its four frames in ascending f, writes the row and the hop's two energy sums
//   report   - one workgroup per row adds the hops' sums in a fixed order (float64) and writes the two levels
// No float atomics and no order that depends on the run: two calls give the same bits.  The row lengths and parameters are host
// values and travel as kernel arguments, so a call neither copies nor synchronises.
#include <math.h>

#include "common.h"
#include "stft256.h"

namespace {

constexpr int N = SOPRO_DN_N, H = SOPRO_DN_H, NB = SOPRO_DN_BINS, HALF = SOPRO_DN_SPAN;
constexpr int PRE = N - H;          // zeros in front of a row
constexpr int WIN = 2 * HALF + 1;   // frames under one minimum
constexpr int SLOT = 2 * NB;        // floats of one frame's spectrum; its 512 samples later
constexpr int DN_GROUP = 64;        // rows of one launch group (their lengths and parameters are kernel arguments)
constexpr int DN_AHEAD = 8;         // frames of one batch of a walk: their operands are loaded, then their steps run
constexpr int FFT_BLOCK = 256, FFT_WAVES = FFT_BLOCK / 64, FFT_FRAMES = 4;  // frames per wave of one workgroup
constexpr int OLA_BLOCK = H, REP_BLOCK = 256;
constexpr int64_t LEN_MAX = (int64_t)1 << 24;
static_assert(N == stft256::N && H == stft256::H && NB == stft256::NB, "the transform is 256 complex points on 64 lanes, four per lane");
static_assert(SLOT >= N, "a frame's samples fit where its spectrum was");

// tables: window [512] | exp(-2 pi i m / 256) [256] | exp(-2 pi i k / 512) [257], made in float64 on the host (stft256.h)
using stft256::cmul;
using stft256::fft256;
using stft256::T_FLOATS;
using stft256::T_SPLIT;
using stft256::T_TW;
using stft256::T_WIN;
__device__ float g_dn_tab[T_FLOATS];

struct Rows {
  int32_t n[DN_GROUP];
  float g_min[DN_GROUP];  // 0: the row is copied through
  float bias[DN_GROUP];
};

__host__ __device__ __forceinline__ int64_t frames_of(int64_t n) { return (n + H - 1) / H + 3; }
// workspace of one row, in floats: spectra / frames [F][514] | A [F][257] | B [F][257] | energy sums [F][2]
__host__ __device__ __forceinline__ int64_t row_floats(int64_t cap) { return frames_of(cap) * (SLOT + 2 * NB + 2); }
struct Ws {
  float *x, *a, *b, *e;
};
__device__ __forceinline__ Ws ws_of(float* ws, int64_t row, int64_t cap) {
  const int64_t F = frames_of(cap);
  Ws w;
  w.x = ws + row * row_floats(cap);
  w.a = w.x + F * SLOT;
  w.b = w.a + F * NB;
  w.e = w.b + F * NB;
  return w;
}

__device__ __forceinline__ void stage_tables(float* s_tab) {
  for (int i = threadIdx.x; i < T_FLOATS; i += FFT_BLOCK) s_tab[i] = g_dn_tab[i];
  __syncthreads();
}

// ---- analysis ----
__global__ __launch_bounds__(FFT_BLOCK) void dn_analysis_kernel(const float* __restrict__ wav, int64_t row_stride, Rows rows, int row0,
                                                                float* __restrict__ ws, int64_t cap) {
  __shared__ float s_tab[T_FLOATS];
  __shared__ float2 s_buf[FFT_WAVES][256];
  stage_tables(s_tab);
  const int r = blockIdx.y, j = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t n = rows.n[r];
  if (n <= 0 || rows.g_min[r] == 0.0f) return;
  const int64_t F = frames_of(n);
  const float* x = wav + (int64_t)(row0 + r) * row_stride;
  const Ws w = ws_of(ws, row0 + r, cap);
  const float* win = s_tab + T_WIN;
  const float2* tw = reinterpret_cast<const float2*>(s_tab + T_TW);
  const float2* sp = reinterpret_cast<const float2*>(s_tab + T_SPLIT);
  float2* buf = s_buf[wv];
  for (int q = 0; q < FFT_FRAMES; ++q) {
    const int64_t f = ((int64_t)blockIdx.x * FFT_FRAMES + q) * FFT_WAVES + wv;
    if (f >= F) break;  // (uniform over the wave)
    float2 v[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int m = 2 * (j + 64 * t);
      const int64_t s = f * H + m - PRE;
      const float e = (s >= 0 && s < n) ? x[s] : 0.0f, o = (s + 1 >= 0 && s + 1 < n) ? x[s + 1] : 0.0f;
      v[t] = make_float2(e * win[m], o * win[m + 1]);
    }
    fft256(v, buf, tw, j);
    wave_lds_sync();
#pragma unroll
    for (int t = 0; t < 4; ++t) buf[j + 64 * t] = v[t];
    wave_lds_sync();
    // X[k] = E[k] + exp(-2 pi i k / 512) O[k]; E = (Z[k] + conj Z[256 - k]) / 2, O = (Z[k] - conj Z[256 - k]) / 2i
    float2* X = reinterpret_cast<float2*>(w.x + f * SLOT);
    for (int k = j; k < NB; k += 64) {
      const float2 zk = buf[k & 255], zc = buf[(256 - k) & 255];
      const float2 E = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y - zc.y));
      const float2 O = make_float2(0.5f * (zk.y + zc.y), 0.5f * (zc.x - zk.x));
      const float2 p = cmul(sp[k], O);
      X[k] = make_float2(E.x + p.x, E.y + p.y);
    }
  }
}

// ---- track ----
// Steps lo <= i < hi of a walk in ascending i: `load(i)` fetches what step i needs and does not depend on the recurrence, so whole
// batches of DN_AHEAD loads are issued before their steps run; the rest goes step by step.  No step is predicated: the walks below
// split their ranges where a step's shape changes, so a batch is straight-line code.
template <class T, class Load, class Step>
__device__ __forceinline__ void walk(int64_t lo, int64_t hi, Load load, Step step) {
  int64_t i = lo;
  for (; i + DN_AHEAD <= hi; i += DN_AHEAD) {
    T v[DN_AHEAD];
#pragma unroll
    for (int u = 0; u < DN_AHEAD; ++u) v[u] = load(i + u);
#pragma unroll
    for (int u = 0; u < DN_AHEAD; ++u) step(i + u, v[u]);
  }
  for (; i < hi; ++i) step(i, load(i));
}

struct GainIn {
  float2 z;
  float m;
};

__global__ __launch_bounds__(64) void dn_track_kernel(Rows rows, int row0, float* __restrict__ ws, int64_t cap) {
  const int r = blockIdx.y, k = blockIdx.x * 64 + threadIdx.x;
  const int64_t n = rows.n[r];
  const float g_min = rows.g_min[r], bias = rows.bias[r];
  if (n <= 0 || g_min == 0.0f || k >= NB) return;
  const int64_t F = frames_of(n);
  const Ws w = ws_of(ws, row0 + r, cap);
  float2* X = reinterpret_cast<float2*>(w.x) + k;  // frame f at X[f * NB]
  float* A = w.a + k;
  float* B = w.b + k;
  const float beta = SOPRO_DN_BETA, alpha = SOPRO_DN_ALPHA;
  const int64_t Fh = F < HALF ? F : HALF;
  // The minimum over |j - f| <= HALF: with j' = j + HALF and +inf outside the row every window is [f, f + 2 HALF] in j', and with
  // blocks of WIN positions it is min(suffix minimum of its block at f, prefix minimum of its block at f + 2 HALF).
  // walk 1, ascending: S -> A[f]; the prefix minimum at j' = f + HALF -> B[j' - 2 HALF] once that is a frame
  float S, g;
  int ph;  // j' mod WIN
  auto load_p = [&](int64_t f) {
    const float2 z = X[f * NB];
    return z.x * z.x + z.y * z.y;
  };
  auto smooth = [&](int64_t f, float P) {
    S = beta * S + (1.0f - beta) * P;
    A[f * NB] = S;
    g = ph == 0 ? S : fminf(g, S);
    ph = ph + 1 == WIN ? 0 : ph + 1;
  };
  S = load_p(0), A[0] = S, g = S, ph = HALF + 1;  // frame 0: S[0] = P[0]
  walk<float>(1, Fh, load_p, smooth);
  walk<float>(HALF, F, load_p, [&](int64_t f, float P) {
    smooth(f, P);
    B[(f - HALF) * NB] = g;
  });
  for (int64_t jp = F + HALF; jp < F + 2 * HALF; ++jp) {  // past the row: +inf
    if (ph == 0) g = INFINITY;
    if (jp >= 2 * HALF) B[(jp - 2 * HALF) * NB] = g;
    ph = ph + 1 == WIN ? 0 : ph + 1;
  }
  // walk 2, descending in j' (i = F + HALF - 1 - j' ascends): the suffix minimum at j' -> A[j'].  Slot j' held S[j'], which was read
  // HALF steps earlier; a batch reads slots at least HALF - DN_AHEAD + 1 below the ones it writes.
  static_assert(HALF >= DN_AHEAD, "the descending walk overwrites S behind its reads");
  float h = INFINITY;
  const int64_t top = F + HALF - 1;
  ph = (int)(top % WIN);
  auto load_s = [&](int64_t i) { return A[(top - i - HALF) * NB]; };  // S[j' - HALF]
  auto suffix = [&](float Sv) {
    h = ph == WIN - 1 ? Sv : fminf(h, Sv);
    ph = ph == 0 ? WIN - 1 : ph - 1;
  };
  // j' = F - 1, the first slot that is a frame, is step HALF; from j' = HALF - 1, step F, S[j' - HALF] lies outside the row
  walk<float>(0, Fh, load_s, [&](int64_t, float Sv) { suffix(Sv); });
  walk<float>(HALF, F, load_s, [&](int64_t i, float Sv) {
    suffix(Sv);
    A[(top - i) * NB] = h;
  });
  for (int64_t jp = Fh - 1; jp >= 0; --jp) A[jp * NB] = h;  // (below j' = HALF: +inf joins, and no block ends there)
  // walk 3, ascending: the gain, X *= G
  float Gp = 0.0f, gam_p = 0.0f;
  auto load_g = [&](int64_t f) {
    GainIn v;
    v.z = X[f * NB];
    v.m = fminf(A[f * NB], B[f * NB]);
    return v;
  };
  auto gain = [&](int64_t f, const GainIn& v, bool first) {
    const float P = v.z.x * v.z.x + v.z.y * v.z.y;
    const float gam = P / fmaxf(bias * v.m, SOPRO_DN_FLOOR);
    const float inst = fmaxf(gam - 1.0f, 0.0f);
    const float xi = first ? inst : alpha * Gp * Gp * gam_p + (1.0f - alpha) * inst;
    const float G = fmaxf(xi / (1.0f + xi), g_min);
    X[f * NB] = make_float2(G * v.z.x, G * v.z.y);
    Gp = G, gam_p = gam;
  };
  gain(0, load_g(0), true);
  walk<GainIn>(1, F, load_g, [&](int64_t f, const GainIn& v) { gain(f, v, false); });
}

// ---- synth ----
__global__ __launch_bounds__(FFT_BLOCK) void dn_synth_kernel(Rows rows, int row0, float* __restrict__ ws, int64_t cap) {
  __shared__ float s_tab[T_FLOATS];
  __shared__ float2 s_buf[FFT_WAVES][NB + 1];
  stage_tables(s_tab);
  const int r = blockIdx.y, j = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t n = rows.n[r];
  if (n <= 0 || rows.g_min[r] == 0.0f) return;
  const int64_t F = frames_of(n);
  const Ws w = ws_of(ws, row0 + r, cap);
  const float* win = s_tab + T_WIN;
  const float2* tw = reinterpret_cast<const float2*>(s_tab + T_TW);
  const float2* sp = reinterpret_cast<const float2*>(s_tab + T_SPLIT);
  float2* buf = s_buf[wv];
  for (int q = 0; q < FFT_FRAMES; ++q) {
    const int64_t f = ((int64_t)blockIdx.x * FFT_FRAMES + q) * FFT_WAVES + wv;
    if (f >= F) break;
    float2* Y = reinterpret_cast<float2*>(w.x + f * SLOT);
    wave_lds_sync();
    for (int k = j; k < NB; k += 64) buf[k] = Y[k];
    wave_lds_sync();
    // Z[k] = E[k] + i O[k]; E = (Y[k] + conj Y[256 - k]) / 2, O = exp(+2 pi i k / 512) (Y[k] - conj Y[256 - k]) / 2.  The inverse
    // transform is the forward one between two conjugations; the imaginary parts of Y[0] and Y[256] drop out, as in an irfft.
    float2 v[4];
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
    // z[m] = conj(v) / 256 holds samples 2m and 2m + 1; the frame is 0.5 w irdft
    float2* y = reinterpret_cast<float2*>(w.x + f * SLOT);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int m = j + 64 * t;
      y[m] = make_float2(v[t].x * (1.0f / 256.0f) * win[2 * m] * 0.5f, -v[t].y * (1.0f / 256.0f) * win[2 * m + 1] * 0.5f);
    }
  }
}

// ---- ola ----
__global__ __launch_bounds__(OLA_BLOCK) void dn_ola_kernel(const float* __restrict__ wav, int64_t row_stride, Rows rows, int row0,
                                                           float* __restrict__ ws, int64_t cap, float* __restrict__ out, int64_t out_stride) {
  __shared__ float s_e[2][OLA_BLOCK / 64];
  const int r = blockIdx.y, o = threadIdx.x;
  const int64_t n = rows.n[r], hb = blockIdx.x;
  if (hb * H >= n) return;
  const Ws w = ws_of(ws, row0 + r, cap);
  const int64_t i = hb * H + o;
  float xs = 0.0f, ds = 0.0f;
  if (i < n) {
    const float x = wav[(int64_t)(row0 + r) * row_stride + i];
    float y = x;
    if (rows.g_min[r] != 0.0f) {
      const float* fr = w.x + hb * SLOT + o;  // sample i + PRE lies in frames hb .. hb + 3
      y = 0.0f;
#pragma unroll
      for (int t = 0; t < 4; ++t) y += fr[t * SLOT + (3 - t) * H];
    }
    out[(int64_t)(row0 + r) * out_stride + i] = y;
    xs = x * x, ds = (x - y) * (x - y);
  }
  xs = wave_sum(xs), ds = wave_sum(ds);
  if ((o & 63) == 0) s_e[0][o >> 6] = xs, s_e[1][o >> 6] = ds;
  __syncthreads();
  if (o == 0) {
    w.e[2 * hb] = s_e[0][0] + s_e[0][1];
    w.e[2 * hb + 1] = s_e[1][0] + s_e[1][1];
  }
}

// ---- report ----
__global__ __launch_bounds__(REP_BLOCK) void dn_report_kernel(Rows rows, int row0, float* __restrict__ ws, int64_t cap, float* __restrict__ report) {
  __shared__ double s_x[REP_BLOCK], s_d[REP_BLOCK];
  const int r = blockIdx.x, t = threadIdx.x;
  const int64_t n = rows.n[r], hops = (n + H - 1) / H;
  const Ws w = ws_of(ws, row0 + r, cap);
  double xs = 0.0, ds = 0.0;
  for (int64_t hb = t; hb < hops; hb += REP_BLOCK) xs += (double)w.e[2 * hb], ds += (double)w.e[2 * hb + 1];
  s_x[t] = xs, s_d[t] = ds;
  __syncthreads();
  for (int s = REP_BLOCK / 2; s > 0; s >>= 1) {
    if (t < s) s_x[t] += s_x[t + s], s_d[t] += s_d[t + s];
    __syncthreads();
  }
  if (t == 0) {
    float* rep = report + 2 * (int64_t)(row0 + r);
    rep[0] = (float)(10.0 * log10(s_x[0] / (double)(n > 0 ? n : 1) + 1e-20));
    rep[1] = (float)(10.0 * log10((s_d[0] + 1e-20) / (s_x[0] + 1e-20)));
  }
}

// The tables of the device the call runs on: float64 on the host, rounded once, uploaded once (as SOPRO_SET_MAX_LDS_ONCE: two
// threads racing on the first call both upload the same bytes).
int upload_tables() {
  static unsigned char done[64] = {};
  static float host[T_FLOATS];
  static bool made = false;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  if (done[dev & 63]) return 0;
  if (!made) {
    stft256::make_tables(host);
    made = true;
  }
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_dn_tab), host, sizeof(host)) != hipSuccess) return -1;
  done[dev & 63] = 1;
  return 0;
}

}  // namespace

int64_t sopro_denoise_workspace_bytes(int32_t rows, int64_t cap) {
  if (rows <= 0 || cap < 0 || cap > LEN_MAX) return -1;
  return (int64_t)rows * row_floats(cap) * (int64_t)sizeof(float);
}

int sopro_denoise_rows_f32(const float* wav, int64_t row_stride, const int32_t* lens, const float* params, int32_t rows, float* out,
                           int64_t out_stride, float* report, void* ws, int64_t ws_bytes, void* stream) {
  SOPRO_CHECK_ARG(lens && params, "lens, params must be non-NULL (host arrays)");
  SOPRO_CHECK_ARG(rows > 0 && rows <= 65535, "0 < rows <= 65535");
  int64_t cap = 0;
  bool any = false;
  for (int b = 0; b < rows; ++b) {
    SOPRO_CHECK_ARG(lens[b] >= 0 && lens[b] <= LEN_MAX, "0 <= lens[b] <= 2^24");
    cap = lens[b] > cap ? lens[b] : cap;
    const float att = params[2 * b], bias = params[2 * b + 1];
    if (bias == 0.0f) continue;  // the row is copied through
    any = true;
    SOPRO_CHECK_ARG(att >= SOPRO_DN_ATTEN_MIN && att <= SOPRO_DN_ATTEN_MAX, "0 <= atten_db <= 40");
    SOPRO_CHECK_ARG(bias >= SOPRO_DN_BIAS_MIN && bias <= SOPRO_DN_BIAS_MAX, "1 <= bias <= 8 (0: the row is copied through)");
  }
  SOPRO_CHECK_ARG(cap == 0 || (wav && out), "wav, out must be non-NULL when a row has samples");
  SOPRO_CHECK_ARG(row_stride >= 0 && out_stride >= 0, "strides >= 0");
  SOPRO_CHECK_ARG(rows == 1 || (row_stride >= cap && out_stride >= cap), "row_stride, out_stride >= max(lens) (rows must not overlap)");
  SOPRO_CHECK_ARG(((reinterpret_cast<uintptr_t>(wav) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(report)) & 3u) == 0,
                  "wav, out, report must be 4-byte aligned");
  SOPRO_CHECK_ARG(ws && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0, "ws must be non-NULL and 8-byte aligned");
  SOPRO_CHECK_ARG(ws_bytes >= sopro_denoise_workspace_bytes(rows, cap), "ws_bytes < sopro_denoise_workspace_bytes(rows, max(lens))");
  if (any && upload_tables() != 0) {
    sopro_set_error("%s: the table upload failed", __func__);
    return -1;
  }
  hipStream_t s = (hipStream_t)stream;
  float* w = static_cast<float*>(ws);
  for (int row0 = 0; row0 < rows; row0 += DN_GROUP) {
    const int nr = rows - row0 < DN_GROUP ? rows - row0 : DN_GROUP;
    Rows g = {};
    int64_t gcap = 0, fcap = 0;
    for (int r = 0; r < nr; ++r) {
      const float att = params[2 * (row0 + r)], bias = params[2 * (row0 + r) + 1];
      g.n[r] = lens[row0 + r];
      g.bias[r] = bias;
      g.g_min[r] = bias == 0.0f ? 0.0f : (float)pow(10.0, -(double)att / 20.0);
      gcap = g.n[r] > gcap ? g.n[r] : gcap;
      if (bias != 0.0f && g.n[r] > 0) fcap = frames_of(g.n[r]) > fcap ? frames_of(g.n[r]) : fcap;
    }
    if (fcap > 0) {
      const unsigned fb = (unsigned)((fcap + FFT_WAVES * FFT_FRAMES - 1) / (FFT_WAVES * FFT_FRAMES));
      hipLaunchKernelGGL(dn_analysis_kernel, dim3(fb, (unsigned)nr), dim3(FFT_BLOCK), 0, s, wav, row_stride, g, row0, w, cap);
      hipLaunchKernelGGL(dn_track_kernel, dim3((NB + 63) / 64, (unsigned)nr), dim3(64), 0, s, g, row0, w, cap);
      hipLaunchKernelGGL(dn_synth_kernel, dim3(fb, (unsigned)nr), dim3(FFT_BLOCK), 0, s, g, row0, w, cap);
    }
    if (gcap > 0)
      hipLaunchKernelGGL(dn_ola_kernel, dim3((unsigned)((gcap + H - 1) / H), (unsigned)nr), dim3(OLA_BLOCK), 0, s, wav, row_stride, g, row0, w, cap,
                         out, out_stride);
    if (report) hipLaunchKernelGGL(dn_report_kernel, dim3((unsigned)nr), dim3(REP_BLOCK), 0, s, g, row0, w, cap, report);
  }
  SOPRO_LAUNCH_CHECK();
}
