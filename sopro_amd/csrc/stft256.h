// The 512 / 128 short-time transform that denoise.hip and formant.hip share: frames of 512 real samples as 256 complex points on the
// 64 lanes of one wave.  The tables (window, twiddles, split factors) are made here in float64; each file keeps its own device copy.
#pragma once
#include <math.h>

#include "common.h"

namespace stft256 {

constexpr int N = 512, H = 128, NB = N / 2 + 1;
// tables: window [512] | exp(-2 pi i m / 256) [256] | exp(-2 pi i k / 512) [257]
constexpr int T_WIN = 0, T_TW = N, T_SPLIT = N + 2 * 256, T_FLOATS = T_SPLIT + 2 * NB;

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// 256-point forward DFT of one wave: lane j enters with points j + 64 t and leaves with outputs j + 64 t (t = 0..3).  Stockham
// autosort, radix 4: stage Ns in 1, 4, 16, 64 twiddles its inputs by exp(-2 pi i t (j mod Ns) / 4 Ns), does the 4-point DFT and
// scatters to (j / Ns) 4 Ns + j mod Ns + t Ns; `buf` is the wave's 256 float2 of LDS.
__device__ __forceinline__ void fft256(float2 (&v)[4], float2* buf, const float2* tw, int j) {
#pragma unroll
  for (int ns = 1; ns <= 64; ns <<= 2) {
    const int k = j & (ns - 1);
    if (ns > 1) {
#pragma unroll
      for (int t = 1; t < 4; ++t) v[t] = cmul(v[t], tw[t * k * (64 / ns)]);
    }
    const float2 a0 = make_float2(v[0].x + v[2].x, v[0].y + v[2].y), a1 = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
    const float2 a2 = make_float2(v[1].x + v[3].x, v[1].y + v[3].y), a3 = make_float2(v[1].y - v[3].y, v[3].x - v[1].x);  // -i (v1 - v3)
    v[0] = make_float2(a0.x + a2.x, a0.y + a2.y);
    v[1] = make_float2(a1.x + a3.x, a1.y + a3.y);
    v[2] = make_float2(a0.x - a2.x, a0.y - a2.y);
    v[3] = make_float2(a1.x - a3.x, a1.y - a3.y);
    if (ns == 64) break;  // (j / 64) 256 + j + 64 t: the outputs are where the lane's inputs were
    const int j0 = ((j & ~(ns - 1)) << 2) + k;
    wave_lds_sync();  // (the slice's earlier readers are done)
#pragma unroll
    for (int t = 0; t < 4; ++t) buf[j0 + t * ns] = v[t];
    wave_lds_sync();
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = buf[j + 64 * t];
  }
}

// The T_FLOATS table values: float64 on the host, rounded once.
inline void make_tables(float* host) {
  const double pi = 3.14159265358979323846;
  for (int i = 0; i < N; ++i) host[T_WIN + i] = (float)sqrt(0.5 * (1.0 - cos(2.0 * pi * i / N)));
  for (int m = 0; m < 256; ++m) host[T_TW + 2 * m] = (float)cos(2.0 * pi * m / 256), host[T_TW + 2 * m + 1] = (float)-sin(2.0 * pi * m / 256);
  for (int k = 0; k < NB; ++k) host[T_SPLIT + 2 * k] = (float)cos(2.0 * pi * k / N), host[T_SPLIT + 2 * k + 1] = (float)-sin(2.0 * pi * k / N);
}

}  // namespace stft256
