// Speaking rate: WSOLA time-scale modification of the rows of a padded batch (contract: include/sopro_hip.h, DESIGN.md "Speaking
// rate").  Rows are independent; the blocks of a row are a serial chain (block k's template starts where block k - 1's copy ended),
// so one workgroup walks one row.  Per block:
//   load    - the candidate region x[a + lo .. a + R + W) and the template x[t .. t + W) into LDS as fp32, their max |x|
//   quantise- both to int8 on the common scale 127 / max; the region as four byte-shifted packed copies, so that every candidate's
//             window starts on a word whatever its offset
//   search  - candidate c per lane: ssd = sum t^2 + sum c^2 - 2 sum t c, three packed int8 dot products per word (v_dot4c_i32_i8)
//   arg-min - over the workgroup on the key ssd << 12 | |d| << 1 | (d < 0): the tie rule is part of the compared integer
//   mix     - y = A + tab * (B - A), three separately rounded fp32 operations
// Every decision is an integer comparison and every sample a fixed chain of fp32 operations: the tests compare bit for bit with a
// numpy restatement.
#include "common.h"

namespace {

constexpr int TSM_W = SOPRO_TSM_W;
constexpr int TSM_HS = SOPRO_TSM_HS;
constexpr int TSM_R = SOPRO_TSM_R;
constexpr int TSM_BLOCK = 512;  // one pass over the <= 481 candidates; measured 256 against 512 in profiles/tsm_timing.md
constexpr int TSM_WAVES = TSM_BLOCK / 64;
constexpr int TSM_REG = TSM_W + 2 * TSM_R;       // 1440: the longest candidate region
constexpr int TSM_REG_WORDS = TSM_REG / 4;       // 360 packed words per shifted copy
constexpr int TSM_COPY_STRIDE = 368;             // words between the copies: 368 % 64 = 48 puts the four copies' 16-word runs of a
                                                 // wave's 64 consecutive candidates on 64 different banks
constexpr int TSM_TM_WORDS = TSM_W / 4;          // 240
constexpr int TSM_TAIL = SOPRO_TSM_TAIL;         // retained input of a chunked row (bound: sopro_hip.h)
constexpr int64_t TSM_STEP_MIN = (int64_t)TSM_HS << 15, TSM_STEP_MAX = (int64_t)TSM_HS << 17;

// state of one row: 8 int64 of header, then two tail buffers of TSM_TAIL floats used in turn (header[4] says which one is current)
constexpr int H_K = 0, H_P = 1, H_RECV = 2, H_BASE = 3, H_BUF = 4;
constexpr int TSM_HDR = 8;

struct RowIn {
  const float* in;     // this call's samples, absolute positions [in_base, recv)
  const float* tail;   // retained samples, absolute positions [tail_base, in_base)
  int64_t tail_base, in_base, recv;
};

// x[i] of the row: zero at or past what has been received (the zero extension of a flush), never outside the two buffers
__device__ __forceinline__ float row_at(const RowIn& r, int64_t i) {
  if (i >= r.recv || i < r.tail_base) return 0.0f;
  return i >= r.in_base ? r.in[i - r.in_base] : r.tail[i - r.tail_base];
}

// The definition rounds every operation on its own.  HIP contracts a * b + c into one fused operation by default, and the
// __fmul_rn / __fadd_rn intrinsics are plain operators that the contraction sees through once inlined: the arithmetic of this file is
// written out under `fp contract(off)` instead.
#pragma clang fp contract(off)

__device__ __forceinline__ int quant(float v, float inv) {
  const int q = (int)rintf(v * inv);
  return q < -127 ? -127 : (q > 127 ? 127 : q);
}

// fl32(A + fl32(g * fl32(B - A))): three roundings
__device__ __forceinline__ float mix3(float A, float B, float g) {
  const float diff = B - A;
  const float prod = g * diff;
  return A + prod;
}

__global__ __launch_bounds__(TSM_BLOCK) void tsm_rows_kernel(const float* __restrict__ in, int64_t in_stride, const int32_t* __restrict__ in_lens,
                                                              int64_t in_cap, const int64_t* __restrict__ steps, int64_t* __restrict__ state, int flush,
                                                              const float* __restrict__ tab, float* __restrict__ out, int64_t out_stride,
                                                              int64_t out_cap, int32_t* __restrict__ out_lens, int32_t* __restrict__ deltas,
                                                              int blocks_cap) {
  __shared__ float s_reg[TSM_REG];
  __shared__ float s_tm[TSM_W];
  __shared__ float s_tab[TSM_HS];
  __shared__ unsigned s_cq[4 * TSM_COPY_STRIDE];
  __shared__ unsigned s_tq[TSM_TM_WORDS];
  __shared__ float s_max[TSM_WAVES];
  __shared__ unsigned long long s_key[TSM_WAVES];

  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int64_t* hdr = state ? state + (int64_t)row * (TSM_HDR + TSM_TAIL) : nullptr;  // (2 * TSM_TAIL floats = TSM_TAIL int64)
  float* tails = hdr ? reinterpret_cast<float*>(hdr + TSM_HDR) : nullptr;
  int64_t k = 0, p_prev = 0, recv0 = 0, tail_base = 0;
  int buf = 0;
  if (hdr) {
    k = hdr[H_K];
    p_prev = hdr[H_P];
    recv0 = hdr[H_RECV];
    tail_base = hdr[H_BASE];
    buf = (int)(hdr[H_BUF] & 1);
    // (a header nobody zeroed: keep every derived index inside the buffers)
    if (k < 0 || p_prev < 0 || recv0 < 0 || tail_base < 0 || tail_base > recv0 || recv0 - tail_base > TSM_TAIL) k = p_prev = recv0 = tail_base = 0;
  }
  int64_t n_in = in_lens[row];
  n_in = n_in < 0 ? 0 : (n_in > in_cap ? in_cap : n_in);
  int64_t step = steps[row];
  step = step < TSM_STEP_MIN ? TSM_STEP_MIN : (step > TSM_STEP_MAX ? TSM_STEP_MAX : step);
  RowIn r;
  r.in = in + (int64_t)row * in_stride;
  r.tail = tails ? tails + buf * TSM_TAIL : nullptr;
  r.tail_base = tail_base;
  r.in_base = recv0;
  r.recv = recv0 + n_in;
  if (!r.tail) r.tail_base = r.in_base;
  const int64_t M = (r.recv * TSM_HS * 65536) / step;  // the output length if the row ended here (used by a flush only)
  const int64_t K = (M + TSM_HS - 1) / TSM_HS;
  float* orow = out + (int64_t)row * out_stride;

  for (int n = tid; n < TSM_HS; n += TSM_BLOCK) s_tab[n] = tab[n];
  __syncthreads();  // (every header word is in registers before the end of the call rewrites it)

  const int64_t k0 = k;
  int64_t written = 0;
  bool overflow = false;
  while (true) {  // (every condition below is uniform over the workgroup)
    const int64_t a = (k * step) >> 16;
    const int64_t t = p_prev + TSM_HS;
    bool ready;
    if (k == 0) ready = flush ? K > 0 : (r.recv >= TSM_HS && M >= TSM_HS);  // (whole: neither zero-extended nor cut, whatever follows)
    else ready = flush ? k < K : r.recv >= (t > a + TSM_R ? t : a + TSM_R) + TSM_W;
    if (!ready) break;
    int64_t cnt = TSM_HS;
    if (flush && (k + 1) * TSM_HS > M) cnt = M - k * TSM_HS;
    if (written + cnt > out_cap) {
      overflow = true;
      break;
    }
    int d_best = 0;
    if (k == 0) {
      for (int n = tid; n < cnt; n += TSM_BLOCK) orow[n] = row_at(r, n);
      p_prev = 0;
    } else {
      const int lo = a < TSM_R ? -(int)a : -TSM_R;
      const int reg_len = TSM_W + TSM_R - lo;  // <= TSM_REG
      __syncthreads();  // the previous block's mix has read s_reg / s_tm
      float m = 0.0f;
      for (int i = tid; i < TSM_REG; i += TSM_BLOCK) {
        const float v = i < reg_len ? row_at(r, a + lo + i) : 0.0f;
        s_reg[i] = v;
        m = fmaxf(m, fabsf(v));
      }
      for (int i = tid; i < TSM_W; i += TSM_BLOCK) {
        const float v = row_at(r, t + i);
        s_tm[i] = v;
        m = fmaxf(m, fabsf(v));
      }
      m = wave_max(m);
      if (lane == 0) s_max[wv] = m;
      __syncthreads();
      m = s_max[0];
#pragma unroll
      for (int i = 1; i < TSM_WAVES; ++i) m = fmaxf(m, s_max[i]);
      if (m > 0.0f) {
        const float inv = 127.0f / m;  // (correctly rounded: hipcc's default for fp32 division)
        for (int it = tid; it < 4 * TSM_REG_WORDS; it += TSM_BLOCK) {  // copy s, word w = the bytes q[4 w + s .. 4 w + s + 3]
          const int s = it / TSM_REG_WORDS, w = it - s * TSM_REG_WORDS;
          unsigned word = 0;
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const int i = 4 * w + s + b;
            const int q = i < TSM_REG ? quant(s_reg[i], inv) : 0;
            word |= (unsigned)(q & 0xff) << (8 * b);
          }
          s_cq[s * TSM_COPY_STRIDE + w] = word;
        }
        for (int w = tid; w < TSM_TM_WORDS; w += TSM_BLOCK) {
          unsigned word = 0;
#pragma unroll
          for (int b = 0; b < 4; ++b) word |= (unsigned)(quant(s_tm[4 * w + b], inv) & 0xff) << (8 * b);
          s_tq[w] = word;
        }
        __syncthreads();
        const int n_cand = TSM_R - lo + 1;  // <= 481
        unsigned long long best = ~0ull;
        for (int c = tid; c < n_cand; c += TSM_BLOCK) {
          const unsigned* cq = s_cq + (c & 3) * TSM_COPY_STRIDE + (c >> 2);
          int tt = 0, cc = 0, tc = 0;
#pragma unroll 8
          for (int j = 0; j < TSM_TM_WORDS; ++j) {
            const int tw = (int)s_tq[j], cw = (int)cq[j];
            tt = __builtin_amdgcn_sdot4(tw, tw, tt, false);
            cc = __builtin_amdgcn_sdot4(cw, cw, cc, false);
            tc = __builtin_amdgcn_sdot4(tw, cw, tc, false);
          }
          const int ssd = tt + cc - 2 * tc;  // >= 0, <= 960 * 254^2
          const int d = c + lo;
          const unsigned long long key = ((unsigned long long)(unsigned)ssd << 12) | (unsigned)((d < 0 ? -d : d) << 1) | (d < 0 ? 1u : 0u);
          best = key < best ? key : best;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const unsigned long long other = __shfl_xor(best, o, 64);
          best = other < best ? other : best;
        }
        if (lane == 0) s_key[wv] = best;
        __syncthreads();
        best = s_key[0];
#pragma unroll
        for (int i = 1; i < TSM_WAVES; ++i) best = s_key[i] < best ? s_key[i] : best;
        const int mag = (int)((best >> 1) & 0x7ff);
        d_best = (best & 1) ? -mag : mag;
      }
      const int off = d_best - lo;  // x[p + n] = s_reg[off + n], off + n <= 2 R + HS - 1 < TSM_REG
      float* o = orow + written;
      for (int n = tid; n < cnt; n += TSM_BLOCK) {
        const float A = s_tm[n], B = s_reg[off + n];
        o[n] = mix3(A, B, s_tab[n]);
      }
      p_prev = a + d_best;
    }
    if (deltas && tid == 0 && k - k0 < blocks_cap) deltas[(int64_t)row * blocks_cap + (k - k0)] = d_best;
    written += cnt;
    ++k;
  }

  if (tid == 0) out_lens[row] = overflow ? -1 : (int32_t)written;
  if (!hdr) return;
  if (flush || overflow) {  // the row is over: a zeroed header is a fresh row
    if (tid < TSM_HDR) hdr[tid] = 0;
    return;
  }
  // what the next block may read: everything from min(t, a - R) on (never before the current base: see the bound in sopro_hip.h)
  int64_t nb = 0;
  if (k > 0) {
    const int64_t a = (k * step) >> 16, t = p_prev + TSM_HS;
    nb = t < a - TSM_R ? t : a - TSM_R;
    nb = nb < r.tail_base ? r.tail_base : nb;
  }
  nb = nb > r.recv ? r.recv : nb;
  if (r.recv - nb > TSM_TAIL) nb = r.recv - TSM_TAIL;  // (unreachable for a call that was not cut short by out_cap)
  float* nt = tails + (buf ^ 1) * TSM_TAIL;
  const int keep = (int)(r.recv - nb);
  for (int i = tid; i < keep; i += TSM_BLOCK) nt[i] = row_at(r, nb + i);
  if (tid == 0) {
    hdr[H_K] = k;
    hdr[H_P] = p_prev;
    hdr[H_RECV] = r.recv;
    hdr[H_BASE] = nb;
    hdr[H_BUF] = buf ^ 1;
  }
}

}  // namespace

int64_t sopro_tsm_out_len(int64_t in_len, int64_t step) {
  if (in_len < 0 || in_len > ((int64_t)1 << 36) || step < TSM_STEP_MIN || step > TSM_STEP_MAX) return -1;
  return (in_len * TSM_HS * 65536) / step;
}

int64_t sopro_tsm_blocks(int64_t out_len) { return out_len <= 0 ? 0 : (out_len + TSM_HS - 1) / TSM_HS; }

int64_t sopro_tsm_chunk_out_cap(int64_t in_len) {
  if (in_len < 0 || in_len > ((int64_t)1 << 36)) return -1;
  return ((in_len + TSM_TAIL) / (TSM_HS / 2) + 4) * TSM_HS;
}

int64_t sopro_tsm_state_bytes(int32_t rows) {
  return rows <= 0 ? 0 : (int64_t)rows * (TSM_HDR + TSM_TAIL) * (int64_t)sizeof(int64_t);
}

int sopro_tsm_rows_f32(const float* in, int64_t in_stride, const int32_t* in_lens, int64_t in_cap, const int64_t* steps, int32_t rows, void* state,
                       int32_t flush, const float* tab, float* out, int64_t out_stride, int64_t out_cap, int32_t* out_lens, int32_t* deltas,
                       int32_t blocks_cap, void* stream) {
  SOPRO_CHECK_ARG(in_lens && steps && out_lens && tab, "in_lens, steps, out_lens, tab must be non-NULL");
  SOPRO_CHECK_ARG(rows > 0, "rows > 0");
  SOPRO_CHECK_ARG(in_cap >= 0 && in_cap <= INT32_MAX, "0 <= in_cap < 2^31");
  SOPRO_CHECK_ARG(in || in_cap == 0, "in must be non-NULL when in_cap > 0");
  SOPRO_CHECK_ARG(in_stride >= 0 && out_stride >= 0, "strides >= 0");
  SOPRO_CHECK_ARG(out_cap >= 0 && out_cap <= INT32_MAX, "0 <= out_cap < 2^31");
  SOPRO_CHECK_ARG(out || out_cap == 0, "out must be non-NULL when out_cap > 0");
  SOPRO_CHECK_ARG(rows == 1 || out_cap == 0 || out_stride >= out_cap, "out_stride >= out_cap (rows must not overlap)");
  SOPRO_CHECK_ARG(state || flush, "a call without state is the whole row: flush must be set");
  SOPRO_CHECK_ARG(!deltas || blocks_cap > 0, "blocks_cap > 0 when deltas is given");
  SOPRO_CHECK_ARG(((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 3u) == 0, "in, out must be 4-byte aligned");
  SOPRO_CHECK_ARG((reinterpret_cast<uintptr_t>(state) & 7u) == 0, "state must be 8-byte aligned");
  hipLaunchKernelGGL(tsm_rows_kernel, dim3(rows), dim3(TSM_BLOCK), 0, (hipStream_t)stream, in, in_stride, in_lens, in_cap, steps,
                     static_cast<int64_t*>(state), flush ? 1 : 0, tab, out, out_stride, out_cap, out_lens, deltas, blocks_cap);
  SOPRO_LAUNCH_CHECK();
}
