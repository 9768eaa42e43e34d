// The window a chunked row operator (pitch.hip, wm.hip) reads a row through, and the copies between a row and LDS that its tiles
// share.  A row is this call's samples plus the tail the state retained from earlier calls; everything else reads as zero.
// Everything here is inlined into its kernel, and the workgroup size is a template parameter: every kernel compiles to the
// instructions it had with its own copy of this code.  (A row's struct holds the window as a member; deriving from it, or moving the
// state kernels' tail rewrite here, reorders instructions in those kernels.)
#pragma once
#include "common.h"

namespace {

struct RowWindow {
  const float* in;    // this call's samples, absolute positions [in_base, recv)
  const float* tail;  // retained samples, absolute positions [tail_base, in_base)
  int64_t tail_base, in_base, recv;
};

// x[i] of the row outside this call's samples: the retained tail, zero elsewhere
__device__ __forceinline__ float row_at_tail(const RowWindow& r, int64_t i) {
  return (r.tail && i >= r.tail_base && i < r.in_base) ? r.tail[i - r.tail_base] : 0.0f;
}

__device__ __forceinline__ float row_at(const RowWindow& r, int64_t i) {
  if (i < 0 || i >= r.recv) return 0.0f;
  return i >= r.in_base ? r.in[i - r.in_base] : row_at_tail(r, i);
}

// dst[0 .. n) = src[0 .. n) by the whole workgroup, global to LDS: 16-byte loads over the aligned body, dwords at the ragged ends
template <int BLOCK>
__device__ __forceinline__ void stage_in(float* dst, const float* src, int n, int tid) {
  int head = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(src) >> 2) & 3u)) & 3u);
  head = head < n ? head : n;
  const int nv = (n - head) >> 2;
  const int tail0 = head + 4 * nv;
  for (int k = tid; k < head; k += BLOCK) dst[k] = src[k];
  const float4* sv = reinterpret_cast<const float4*>(src + head);
  for (int v = tid; v < nv; v += BLOCK) {
    const float4 q = sv[v];
    float* d = dst + head + 4 * v;
    d[0] = q.x;
    d[1] = q.y;
    d[2] = q.z;
    d[3] = q.w;
  }
  for (int k = tail0 + tid; k < n; k += BLOCK) dst[k] = src[k];
}

// dst[0 .. n) = src[0 .. n), LDS to global, the same way
template <int BLOCK>
__device__ __forceinline__ void store_out(float* dst, const float* src, int n, int tid) {
  int head = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3u)) & 3u);
  head = head < n ? head : n;
  const int nv = (n - head) >> 2;
  const int tail0 = head + 4 * nv;
  for (int k = tid; k < head; k += BLOCK) dst[k] = src[k];
  float4* dv = reinterpret_cast<float4*>(dst + head);
  for (int v = tid; v < nv; v += BLOCK) {
    const float* s = src + head + 4 * v;
    dv[v] = make_float4(s[0], s[1], s[2], s[3]);
  }
  for (int k = tail0 + tid; k < n; k += BLOCK) dst[k] = src[k];
}

}  // namespace
