// Long-form join: a padded decoder batch [n_seg, row_stride] -> one continuous waveform (contract: include/sopro_hip.h, DESIGN.md
// "Long-form synthesis").  Three steps, all enqueued on the caller's stream, nothing allocated, nothing synchronised:
//   edges  - where each row's speech starts and ends (peak envelope per hop, threshold relative to the row's peak)
//   layout - exclusive scan of the kept lengths plus the pauses -> offsets into the output
//   mix    - the kept samples end to end, cuts faded by a host-made table, pauses written as zeros
// Every decision is a maximum or an integer comparison, every output sample one fp32 product: the result does not depend on the
// order of any reduction, so the test compares it bit for bit with a numpy restatement.
#include "common.h"

namespace {

constexpr int JOIN_BLOCK = 256;
constexpr int JOIN_WAVES = JOIN_BLOCK / 64;
constexpr int JOIN_GRID_CAP = 2048;  // memory-bound grids: ~8 workgroups per CU, grid-stride the rest
constexpr int HOPS_PER_ITEM = 4;     // hops one wave has in flight per iteration

__device__ __forceinline__ int32_t row_len(const int32_t* lens, int k, int64_t max_len) {
  const int64_t L = lens[k];
  return (int32_t)(L < 0 ? 0 : (L > max_len ? max_len : L));
}

// This lane's share of max |x[0 .. n)|: 16-byte loads over the aligned body, dwords for the ragged head and tail.
__device__ __forceinline__ float lane_absmax(const float* x, int n, int lane) {
  float m = 0.0f;
  if (n <= 0) return m;
  int head = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(x) >> 2) & 3u)) & 3u);
  head = head < n ? head : n;
  const int nv = (n - head) >> 2;
  const int tail0 = head + 4 * nv;
  if (lane < head) m = fabsf(x[lane]);
  const float4* xv = reinterpret_cast<const float4*>(x + head);
  for (int v = lane; v < nv; v += 64) {
    const float4 q = xv[v];
    m = fmaxf(m, fmaxf(fmaxf(fabsf(q.x), fabsf(q.y)), fmaxf(fabsf(q.z), fabsf(q.w))));
  }
  if (lane < n - tail0) m = fmaxf(m, fabsf(x[tail0 + lane]));
  return m;
}

// hopmax[k * hops_cap + j] = max |x| over hop j of row k, for the hops that hold a valid sample.  One wave per item of
// HOPS_PER_ITEM consecutive hops (their loads are issued before the first reduction), items grid-strided.
__global__ __launch_bounds__(JOIN_BLOCK) void join_hop_max_kernel(const float* __restrict__ wav, int64_t row_stride,
                                                                   const int32_t* __restrict__ lens, int n_seg, int64_t max_len, int hop,
                                                                   int hops_cap, float* __restrict__ hopmax) {
  const int lane = threadIdx.x & 63;
  const int items_per_row = (hops_cap + HOPS_PER_ITEM - 1) / HOPS_PER_ITEM;
  const int64_t n_items = (int64_t)n_seg * items_per_row;
  const int64_t stride = (int64_t)gridDim.x * JOIN_WAVES;
  for (int64_t it = (int64_t)blockIdx.x * JOIN_WAVES + (threadIdx.x >> 6); it < n_items; it += stride) {
    const int k = (int)(it / items_per_row);
    const int j0 = (int)(it - (int64_t)k * items_per_row) * HOPS_PER_ITEM;
    const int32_t L = row_len(lens, k, max_len);
    if ((int64_t)j0 * hop >= L) continue;  // (wave-uniform)
    const float* row = wav + (int64_t)k * row_stride;
    float m[HOPS_PER_ITEM];
#pragma unroll
    for (int h = 0; h < HOPS_PER_ITEM; ++h) {
      const int64_t s = (int64_t)(j0 + h) * hop;
      const int64_t rest = (int64_t)L - s;
      m[h] = lane_absmax(row + s, (int)(rest < hop ? (rest < 0 ? 0 : rest) : hop), lane);
    }
#pragma unroll
    for (int h = 0; h < HOPS_PER_ITEM; ++h) m[h] = wave_max(m[h]);
    if (lane < HOPS_PER_ITEM && (int64_t)(j0 + lane) * hop < L && j0 + lane < hops_cap) {
      float v = m[0];
#pragma unroll
      for (int h = 1; h < HOPS_PER_ITEM; ++h) v = lane == h ? m[h] : v;
      hopmax[(int64_t)k * hops_cap + j0 + lane] = v;
    }
  }
}

// One workgroup per row over its hop maxima: the peak, then the lowest / highest hop at or above rel * peak.
__global__ __launch_bounds__(JOIN_BLOCK) void join_row_edges_kernel(const float* __restrict__ hopmax, const int32_t* __restrict__ lens,
                                                                     int64_t max_len, int hop, int hops_cap, float rel, int keep,
                                                                     int32_t* __restrict__ edges) {
  __shared__ float s_peak[JOIN_WAVES];
  __shared__ int s_first[JOIN_WAVES], s_last[JOIN_WAVES];
  const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int32_t L = row_len(lens, k, max_len);
  int nh = (int)(((int64_t)L + hop - 1) / hop);
  nh = nh < hops_cap ? nh : hops_cap;
  const float* hm = hopmax + (int64_t)k * hops_cap;
  float peak = 0.0f;
  for (int j = tid; j < nh; j += JOIN_BLOCK) peak = fmaxf(peak, hm[j]);
  peak = wave_max(peak);
  if (lane == 0) s_peak[w] = peak;
  __syncthreads();
  peak = s_peak[0];
#pragma unroll
  for (int i = 1; i < JOIN_WAVES; ++i) peak = fmaxf(peak, s_peak[i]);
  const float thr = __fmul_rn(rel, peak);
  int first = INT32_MAX, last = -1;
  for (int j = tid; j < nh; j += JOIN_BLOCK) {
    if (hm[j] >= thr) {
      first = first < j ? first : j;
      last = j;  // (j ascends per thread)
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    first = min(first, __shfl_xor(first, o, 64));
    last = max(last, __shfl_xor(last, o, 64));
  }
  if (lane == 0) {
    s_first[w] = first;
    s_last[w] = last;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int i = 1; i < JOIN_WAVES; ++i) {
      first = min(first, s_first[i]);
      last = max(last, s_last[i]);
    }
    int64_t start = 0, end = 0;
    if (L > 0 && peak > 0.0f && first <= last) {  // (a non-finite threshold can leave no active hop: an empty segment)
      start = ((int64_t)first - keep) * hop;
      end = ((int64_t)last + 1 + keep) * hop;
      start = start < 0 ? 0 : (start > L ? L : start);
      end = end > L ? L : (end < start ? start : end);
    }
    edges[2 * k] = (int32_t)start;
    edges[2 * k + 1] = (int32_t)end;
  }
}

// trim off: every row is kept whole
__global__ void join_whole_rows_kernel(const int32_t* __restrict__ lens, int n_seg, int64_t max_len, int32_t* __restrict__ edges) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n_seg) {
    edges[2 * k] = 0;
    edges[2 * k + 1] = row_len(lens, k, max_len);
  }
}

// offs[0] = 0, offs[k + 1] = offs[k] + (n_k > 0 ? n_k + gaps[k] : 0): one workgroup, 256-wide tiles with a running carry.
__global__ __launch_bounds__(JOIN_BLOCK) void join_layout_kernel(const int32_t* __restrict__ edges, const int32_t* __restrict__ gaps, int n_seg,
                                                                  int64_t* __restrict__ offs) {
  __shared__ int64_t s[JOIN_BLOCK];
  const int tid = threadIdx.x;
  int64_t carry = 0;
  if (tid == 0) offs[0] = 0;
  for (int k0 = 0; k0 < n_seg; k0 += JOIN_BLOCK) {
    const int k = k0 + tid;
    int64_t c = 0;
    if (k < n_seg) {
      const int64_t n = (int64_t)edges[2 * k + 1] - edges[2 * k];
      const int32_t g = gaps[k];
      c = n > 0 ? n + (g > 0 ? g : 0) : 0;
    }
    s[tid] = c;
    __syncthreads();
    for (int o = 1; o < JOIN_BLOCK; o <<= 1) {  // inclusive scan
      const int64_t add = tid >= o ? s[tid - o] : 0;
      __syncthreads();
      s[tid] += add;
      __syncthreads();
    }
    if (k < n_seg) offs[k + 1] = carry + s[tid];
    carry += s[JOIN_BLOCK - 1];
    __syncthreads();
  }
}

// out[0 .. min(total, out_cap)): four consecutive samples per thread.  The tile's first segment comes from a binary search in
// offs on a workgroup-uniform position; from there each thread walks forward (a segment is ~10^5 samples: zero or one step).
__global__ __launch_bounds__(JOIN_BLOCK) void join_mix_kernel(const float* __restrict__ wav, int64_t row_stride, const int32_t* __restrict__ edges,
                                                               const int64_t* __restrict__ offs, const float* __restrict__ tab, int fade_len,
                                                               int n_seg, float* __restrict__ out, int64_t out_cap, int vec_ok) {
  const int64_t total = offs[n_seg];
  const int64_t limit = total < out_cap ? total : out_cap;
  constexpr int64_t TILE = (int64_t)JOIN_BLOCK * 4;
  for (int64_t t0 = (int64_t)blockIdx.x * TILE; t0 < limit; t0 += (int64_t)gridDim.x * TILE) {
    int lo = 0, hi = n_seg - 1;  // largest k with offs[k] <= t0 (of equal offsets the last: the ones before it are empty)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (offs[mid] <= t0) lo = mid;
      else hi = mid - 1;
    }
    int k = lo;
    const int64_t p0 = t0 + 4 * (int64_t)threadIdx.x;
    if (p0 >= limit) continue;
    int64_t o0 = offs[k], o1 = offs[k + 1];
    int32_t st = edges[2 * k], n = edges[2 * k + 1] - st;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int64_t p = p0 + e;
      v[e] = 0.0f;
      if (p >= limit) continue;
      while (p >= o1 && k + 1 < n_seg) {
        ++k;
        o0 = o1;
        o1 = offs[k + 1];
        st = edges[2 * k];
        n = edges[2 * k + 1] - st;
      }
      const int64_t i = p - o0;
      if (i < n) {  // (else: the pause after the segment)
        const int F = fade_len < (n >> 1) ? fade_len : (n >> 1);
        float g = 1.0f;
        if (i < F) g = tab[i];
        else if (i >= n - F) g = tab[n - 1 - i];
        v[e] = __fmul_rn(wav[(int64_t)k * row_stride + st + i], g);
      }
    }
    if (vec_ok && p0 + 4 <= limit) {
      *reinterpret_cast<float4*>(out + p0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (p0 + e < limit) out[p0 + e] = v[e];
    }
  }
}

inline int64_t hops_of(int64_t max_len, int32_t hop) { return max_len <= 0 ? 1 : (max_len + hop - 1) / hop; }

}  // namespace

int64_t sopro_join_workspace_bytes(int32_t n_seg, int64_t max_len, int32_t hop) {
  if (n_seg <= 0 || hop <= 0 || max_len < 0 || max_len > INT32_MAX) return 0;
  return (int64_t)n_seg * hops_of(max_len, hop) * (int64_t)sizeof(float);
}

int sopro_join_edges_f32(const float* wav, int64_t row_stride, const int32_t* lens, int32_t n_seg, int64_t max_len, int32_t hop, float rel,
                         int32_t keep, int32_t trim, void* workspace, int32_t* edges, void* stream) {
  SOPRO_CHECK_ARG(wav && lens && edges, "wav, lens, edges must be non-NULL");
  SOPRO_CHECK_ARG(n_seg > 0, "n_seg > 0");
  SOPRO_CHECK_ARG(hop > 0, "hop > 0");
  SOPRO_CHECK_ARG(row_stride >= 0, "row_stride >= 0");
  SOPRO_CHECK_ARG(max_len >= 0 && max_len <= INT32_MAX, "0 <= max_len < 2^31");
  SOPRO_CHECK_ARG(keep >= 0, "keep >= 0");
  hipStream_t s = (hipStream_t)stream;
  if (!trim) {
    hipLaunchKernelGGL(join_whole_rows_kernel, dim3((n_seg + 255) / 256), dim3(256), 0, s, lens, n_seg, max_len, edges);
    SOPRO_LAUNCH_CHECK();
  }
  SOPRO_CHECK_ARG(workspace, "workspace must be non-NULL (sopro_join_workspace_bytes)");
  SOPRO_CHECK_ARG((reinterpret_cast<uintptr_t>(wav) & 3u) == 0, "wav must be 4-byte aligned");
  const int64_t hops_cap = hops_of(max_len, hop);
  SOPRO_CHECK_ARG(hops_cap <= INT32_MAX, "too many hops per row");
  const int64_t items = (int64_t)n_seg * ((hops_cap + HOPS_PER_ITEM - 1) / HOPS_PER_ITEM);
  const int64_t want = (items + JOIN_WAVES - 1) / JOIN_WAVES;
  const int grid = (int)(want < JOIN_GRID_CAP ? (want < 1 ? 1 : want) : JOIN_GRID_CAP);
  float* hopmax = static_cast<float*>(workspace);
  hipLaunchKernelGGL(join_hop_max_kernel, dim3(grid), dim3(JOIN_BLOCK), 0, s, wav, row_stride, lens, n_seg, max_len, hop, (int)hops_cap, hopmax);
  hipLaunchKernelGGL(join_row_edges_kernel, dim3(n_seg), dim3(JOIN_BLOCK), 0, s, hopmax, lens, max_len, hop, (int)hops_cap, rel, keep, edges);
  SOPRO_LAUNCH_CHECK();
}

int sopro_join_layout_i64(const int32_t* edges, const int32_t* gaps, int32_t n_seg, int64_t* offs, void* stream) {
  SOPRO_CHECK_ARG(edges && gaps && offs, "edges, gaps, offs must be non-NULL");
  SOPRO_CHECK_ARG(n_seg > 0, "n_seg > 0");
  hipLaunchKernelGGL(join_layout_kernel, dim3(1), dim3(JOIN_BLOCK), 0, (hipStream_t)stream, edges, gaps, n_seg, offs);
  SOPRO_LAUNCH_CHECK();
}

int sopro_join_mix_f32(const float* wav, int64_t row_stride, const int32_t* edges, const int64_t* offs, const float* tab, int32_t fade_len,
                       int32_t n_seg, float* out, int64_t out_cap, void* stream) {
  SOPRO_CHECK_ARG(wav && edges && offs && out, "wav, edges, offs, out must be non-NULL");
  SOPRO_CHECK_ARG(n_seg > 0, "n_seg > 0");
  SOPRO_CHECK_ARG(fade_len >= 0, "fade_len >= 0");
  SOPRO_CHECK_ARG(fade_len == 0 || tab, "tab must be non-NULL when fade_len > 0");
  SOPRO_CHECK_ARG(row_stride >= 0, "row_stride >= 0");
  SOPRO_CHECK_ARG(out_cap >= 0, "out_cap >= 0");
  if (out_cap == 0) return 0;
  constexpr int64_t TILE = (int64_t)JOIN_BLOCK * 4;
  const int64_t want = (out_cap + TILE - 1) / TILE;
  const int grid = (int)(want < JOIN_GRID_CAP ? want : JOIN_GRID_CAP);
  hipLaunchKernelGGL(join_mix_kernel, dim3(grid), dim3(JOIN_BLOCK), 0, (hipStream_t)stream, wav, row_stride, edges, offs, tab, fade_len, n_seg, out,
                     out_cap, aligned16(out) ? 1 : 0);
  SOPRO_LAUNCH_CHECK();
}
