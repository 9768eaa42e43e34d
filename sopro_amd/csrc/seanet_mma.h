// Device helpers shared by the fused SEANet decoder kernels (seanet_up.hip, seanet_res.hip, seanet_tail.hip, seanet_uptail.hip):
// the split-bf16 operand forms, the 32x32 MFMA accumulator layout, the LDS row pitches and the weight-stationary K walk.
#pragma once
#include "common.h"

// ---- operands: 8 consecutive bf16 = one 16-byte MFMA A / B fragment of a lane
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ bf16x8 frag(const uint4& v) { return *reinterpret_cast<const bf16x8*>(&v); }

// 8 consecutive fp32 values -> their (hi, lo) fragments (x = hi + lo, split2_bf16 of common.h)
__device__ __forceinline__ void split8(const float* __restrict__ p, uint4& hi, uint4& lo) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  split2_bf16(a.x, a.y, hi.x, lo.x);
  split2_bf16(a.z, a.w, hi.y, lo.y);
  split2_bf16(b.x, b.y, hi.z, lo.z);
  split2_bf16(b.z, b.w, hi.w, lo.w);
}

// NS substeps of a weight row as B fragments: substep s = the 8 values at p + 16 s (p already points at this lane's k half).
// One-pass kernels keep no lo fragments: they hand `wh` in for `wl` as well and nothing is written to it.
template <int PASSES, int NS, int NL>
__device__ __forceinline__ void split_wfrags(const float* __restrict__ p, uint4 (&wh)[NS], uint4 (&wl)[NL]) {
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    uint4 lo;
    split8(p + s * 16, wh[s], lo);
    if (PASSES == 3) wl[s] = lo;
  }
}

// ---- LDS rows: one row of C channels + 16 bytes of padding (the 16-lane ds_read_b128 fragment reads of consecutive rows are
// then conflict free).  Split form: [C hi | C lo] bf16; bf16 rows: C bf16.
constexpr int split_row_bytes(int C) { return 2 * C * 2 + 16; }
constexpr int bf16_row_bytes(int C) { return C * 2 + 16; }

// ---- v_mfma_f32_32x32x16 accumulators: register r of a lane is row acc32_row(r) + 4 * (lane >> 5) of the 32-row block,
// column lane & 31 - lanes 0-31 of a register hold 32 consecutive columns of one row; registers (r, r + 1) of an even r are
// rows (R, R + 1).
constexpr int acc32_row(int r) { return 8 * (r >> 2) + (r & 3); }

// bf16 stores from that layout, 4 bytes per lane: the two lanes of a column pair (c, c + 1) exchange one register of (r, r + 1).
// The even lane keeps row R and takes its neighbour's column for it, the odd lane keeps row R + 1: afterwards (c0, c1) are
// columns (c, c + 1) of this lane's row - 16 lanes write one 64-byte segment of a row per instruction.
__device__ __forceinline__ void pair_cols(float mine0, float mine1, bool odd, float& c0, float& c1) {
  const float got = __shfl_xor(odd ? mine0 : mine1, 1, 64);  // even lane: row R of column c + 1; odd lane: row R + 1 of column c - 1
  c0 = odd ? got : mine0;
  c1 = odd ? mine1 : got;
}

// ---- the weight-stationary K walk: acc[mt] = A[32 mt .. 32 mt + 31, K range] * W^T for the two 32-row tiles of a 64-row LDS
// tile, the weights as register B fragments (wh, wl: substep s of this wave's columns).  `a` = LDS address of this lane's
// fragment of row 0 (row lane & 31, + 16 * (lane >> 5)); rows are ROW bytes apart, the lo plane LO bytes behind the hi plane.
// The K index is tap * 128 + channel: global substep sg = sg0 + s covers tap sg / 8 (LDS row + tap), channels 16 * (sg % 8) ..
// PASSES = 3: lo*hi + hi*lo + hi*hi, PASSES = 1: hi*hi only (`wl` is not read).
// Both row tiles advance together (two independent accumulator chains) and the fragment reads run DEPTH substeps ahead of the
// MFMAs that consume them; the scheduling barriers pin that order (left to itself - or with sched_group_barrier - the compiler
// emits read -> wait -> MFMA per substep: every LDS latency exposed).
template <int PASSES, int NS, int ROW, int LO, int NL>
__device__ __forceinline__ void ws_walk(const unsigned char* a, int sg0, const uint4 (&wh)[NS], const uint4 (&wl)[NL], f32x16 (&acc)[2]) {
  constexpr int DEPTH = 2;
  uint4 ah[DEPTH][2], al[DEPTH][2];
  auto fread = [&](int s, int slot) {
    const int sg = sg0 + s;
    const unsigned char* p = a + (sg >> 3) * ROW + (sg & 7) * 32;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      ah[slot][mt] = *reinterpret_cast<const uint4*>(p + mt * 32 * ROW);
      if (PASSES == 3) al[slot][mt] = *reinterpret_cast<const uint4*>(p + mt * 32 * ROW + LO);
    }
  };
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
#pragma unroll
  for (int s = 0; s < DEPTH; ++s) fread(s, s);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    uint4 ch[2], cl[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) { ch[mt] = ah[s % DEPTH][mt]; if (PASSES == 3) cl[mt] = al[s % DEPTH][mt]; }
    if (PASSES == 3) {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(cl[mt]), frag(wh[s]), acc[mt], 0, 0, 0);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(ch[mt]), frag(wl[s]), acc[mt], 0, 0, 0);
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(ch[mt]), frag(wh[s]), acc[mt], 0, 0, 0);
    if (s + DEPTH < NS) fread(s + DEPTH, s % DEPTH);
    __builtin_amdgcn_sched_barrier(0);
  }
}
