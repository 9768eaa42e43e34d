// Pitch: band-limited resampling of the rows of a padded batch at one ratio per row (contract: include/sopro_hip.h, DESIGN.md
// "Pitch").  Unlike the stretch, outputs are independent: the grid is (tile of PITCH_TILE outputs, row) and one launch covers the
// whole padded batch.  Per tile:
//   stage   - the input span x[i_first - 31 .. i_last + 32] (<= 2 TILE + 64 samples at rho = 2) and the row's 257 x 64 bank into LDS:
//             16-byte global loads over the aligned body, dwords at the ragged ends.  The bank's LDS rows are 65 dwords apart: the
//             lanes of a wave read different phase rows at the same tap, and a stride of 64 would put them all on one bank
//   compute - output n per lane: 64 taps in ascending order, c = h0 + f (h1 - h0), acc += c x, every operation rounded on its own
//   store   - through an LDS tile, so that the global stores are 16 bytes wide whatever the alignment of the row
// A row with inc == 2^32 is a copy and never touches the bank.  The chunked form keeps (next output, received, tail) per row; the
// tiles only read it, and a second, small launch rewrites it once they are done.
#include "common.h"
#include "rows_window.h"

namespace {

constexpr int NT = SOPRO_PITCH_NT;
constexpr int HALF = NT / 2;
constexpr int BANK_ROWS = SOPRO_PITCH_P + 1;
constexpr int BANK_STRIDE = NT + 1;  // odd: phase rows p and p' share an LDS bank only when p = p' (mod 32)
constexpr int PITCH_TILE = SOPRO_PITCH_TILE;
constexpr int PITCH_BLOCK = 1024;    // 4 waves per SIMD: what ds_read_b32 needs to reach its rate, and one workgroup fills the CU's LDS
constexpr int SPAN = 2 * PITCH_TILE + NT;
constexpr int LDS_FLOATS = BANK_ROWS * BANK_STRIDE + SPAN + PITCH_TILE;  // 91652 bytes of the CU's 160 KiB
constexpr int PITCH_TAIL = SOPRO_PITCH_TAIL;
constexpr int64_t ONE = (int64_t)1 << 32, INC_MIN = (int64_t)1 << 31, INC_MAX = (int64_t)1 << 33;
constexpr int64_t LEN_MAX = (int64_t)1 << 30;  // (L << 32 stays inside int64, n * inc inside uint64)

// state of one row: 4 int64 of header, then PITCH_TAIL floats
constexpr int H_N = 0, H_RECV = 1, H_BASE = 2;
constexpr int PITCH_HDR = 4;
constexpr int STATE_WORDS = PITCH_HDR + PITCH_TAIL / 2;

struct Row {
  RowWindow w;
  int64_t inc;
  int64_t n0, n1;     // the outputs of this call
  bool overflow;      // they do not fit out_cap
};

// What a call does for a row, from the arguments and the state as the call found it (both kernels of a call derive the same).
__device__ __forceinline__ Row row_setup(int row, const float* in, int64_t in_stride, const int32_t* in_lens, int64_t in_cap, const int64_t* incs,
                                         const int64_t* state, int flush, int64_t out_cap) {
  Row r;
  const int64_t* hdr = state ? state + (int64_t)row * STATE_WORDS : nullptr;
  int64_t n0 = 0, recv0 = 0, base = 0;
  if (hdr) {
    n0 = hdr[H_N];
    recv0 = hdr[H_RECV];
    base = hdr[H_BASE];
    // (a header nobody zeroed: keep every derived index inside the buffers)
    if (n0 < 0 || n0 > 2 * recv0 + 2 || recv0 < 0 || recv0 > LEN_MAX || base < 0 || base > recv0 || recv0 - base > PITCH_TAIL) n0 = recv0 = base = 0;
  }
  int64_t n_in = in_lens[row];
  n_in = n_in < 0 ? 0 : (n_in > in_cap ? in_cap : n_in);
  n_in = recv0 + n_in > LEN_MAX ? LEN_MAX - recv0 : n_in;
  int64_t inc = incs[row];
  inc = inc < INC_MIN ? INC_MIN : (inc > INC_MAX ? INC_MAX : inc);
  r.w.in = in + (int64_t)row * in_stride;
  r.w.tail = hdr ? reinterpret_cast<const float*>(hdr + PITCH_HDR) : nullptr;
  r.w.in_base = recv0;
  r.w.tail_base = hdr ? base : recv0;
  r.w.recv = recv0 + n_in;
  r.inc = inc;
  int64_t n1;
  if (flush) n1 = (r.w.recv << 32) / inc;  // M of the total length
  else n1 = r.w.recv > HALF ? (((r.w.recv - HALF) << 32) + inc - 1) / inc : 0;  // the n with (n * inc >> 32) + 32 < recv
  r.n0 = n0;
  r.n1 = n1 < n0 ? n0 : n1;
  r.overflow = r.n1 - r.n0 > out_cap;
  return r;
}

// The definition rounds every operation on its own (see tsm.hip on why this is a pragma and not a set of intrinsics).
#pragma clang fp contract(off)

__global__ __launch_bounds__(PITCH_BLOCK) void pitch_rows_kernel(const float* __restrict__ in, int64_t in_stride, const int32_t* __restrict__ in_lens,
                                                                  int64_t in_cap, const int64_t* __restrict__ incs,
                                                                  const int32_t* __restrict__ bank_idx, const float* __restrict__ banks, int n_banks,
                                                                  const int64_t* __restrict__ state, int flush, float* __restrict__ out,
                                                                  int64_t out_stride, int64_t out_cap, int32_t* __restrict__ out_lens) {
  extern __shared__ float smem[];
  float* s_bank = smem;
  float* s_x = s_bank + BANK_ROWS * BANK_STRIDE;
  float* s_y = s_x + SPAN;

  const int row = blockIdx.y, tid = threadIdx.x;
  const Row r = row_setup(row, in, in_stride, in_lens, in_cap, incs, state, flush, out_cap);
  if (blockIdx.x == 0 && tid == 0) out_lens[row] = r.overflow ? -1 : (int32_t)(r.n1 - r.n0);
  if (r.overflow) return;  // (every condition up to the barrier is uniform over the workgroup)
  const int64_t na = r.n0 + (int64_t)blockIdx.x * PITCH_TILE;
  if (na >= r.n1) return;
  const int cnt = (int)(r.n1 - na < PITCH_TILE ? r.n1 - na : PITCH_TILE);
  const bool identity = r.inc == ONE;
  const uint64_t inc = (uint64_t)r.inc;

  // the span of the row this tile reads: s_x[k] = x[i_lo + k]
  int64_t i_lo = na;
  int span = cnt;
  if (!identity) {
    i_lo = (int64_t)(((uint64_t)na * inc) >> 32) - (HALF - 1);
    span = (int)((int64_t)(((uint64_t)(na + cnt - 1) * inc) >> 32) + HALF - i_lo + 1);  // <= 2 (TILE - 1) + 1 + 64 <= SPAN
  }
  // [ka, kb): the part of the span that lies in this call's samples; the rest is the retained tail or zero
  const int64_t i_end = i_lo + span;
  int64_t ga = i_lo > r.w.in_base ? i_lo : r.w.in_base, gb = i_end < r.w.recv ? i_end : r.w.recv;
  ga = ga > i_end ? i_end : ga;
  gb = gb < ga ? ga : gb;
  const int ka = (int)(ga - i_lo), kb = (int)(gb - i_lo);
  for (int k = tid; k < span; k += PITCH_BLOCK)
    if (k < ka || k >= kb) s_x[k] = row_at_tail(r.w, i_lo + k);
  if (kb > ka) stage_in<PITCH_BLOCK>(s_x + ka, r.w.in + (ga - r.w.in_base), kb - ka, tid);
  if (!identity) {
    int b = bank_idx[row];
    b = b < 0 ? 0 : (b >= n_banks ? n_banks - 1 : b);
    const float4* src = reinterpret_cast<const float4*>(banks + (int64_t)b * BANK_ROWS * NT);
    for (int q = tid; q < BANK_ROWS * (NT / 4); q += PITCH_BLOCK) {
      const float4 v = src[q];
      float* d = s_bank + (q >> 4) * BANK_STRIDE + (q & 15) * 4;
      d[0] = v.x;
      d[1] = v.y;
      d[2] = v.z;
      d[3] = v.w;
    }
  }
  __syncthreads();

  for (int m = tid; m < cnt; m += PITCH_BLOCK) {
    if (identity) {
      s_y[m] = s_x[m];
      continue;
    }
    const uint64_t pos = (uint64_t)(na + m) * inc;
    const int64_t i = (int64_t)(pos >> 32);
    const uint32_t fr = (uint32_t)pos;
    const int p = (int)(fr >> 24);
    const float f = (float)(fr & 0xFFFFFFu) * 0x1p-24f;  // (both exact)
    const float* b0 = s_bank + p * BANK_STRIDE;
    const float* b1 = b0 + BANK_STRIDE;
    const float* xs = s_x + (int)(i - (HALF - 1) - i_lo);  // xs[63] = x[i + 32]: the last sample of the span at most
    float acc = 0.0f;
#pragma unroll 16
    for (int j = 0; j < NT; ++j) {
      const float h0 = b0[j], h1 = b1[j];
      const float diff = h1 - h0;
      const float step = f * diff;
      const float c = h0 + step;
      const float prod = c * xs[j];
      acc = acc + prod;
    }
    s_y[m] = acc;
  }
  __syncthreads();
  store_out<PITCH_BLOCK>(out + (int64_t)row * out_stride + (na - r.n0), s_y, cnt, tid);  // (na - n0 + cnt <= n1 - n0 <= out_cap)
}

// The end of a chunked call: one workgroup per row rewrites the row's state once every tile of the call has read it (stream order).
constexpr int STATE_BLOCK = PITCH_TAIL;

__global__ __launch_bounds__(STATE_BLOCK) void pitch_state_kernel(const float* __restrict__ in, int64_t in_stride, const int32_t* __restrict__ in_lens,
                                                                   int64_t in_cap, const int64_t* __restrict__ incs, int64_t* __restrict__ state,
                                                                   int flush, int64_t out_cap) {
  __shared__ float s_keep[PITCH_TAIL];
  const int row = blockIdx.x, tid = threadIdx.x;
  const Row r = row_setup(row, in, in_stride, in_lens, in_cap, incs, state, flush, out_cap);  // (the old header, by value)
  int64_t* hdr = state + (int64_t)row * STATE_WORDS;
  float* tail = reinterpret_cast<float*>(hdr + PITCH_HDR);
  if (flush || r.overflow) {  // the row is over: a zeroed header is a fresh row (uniform over the workgroup)
    for (int k = tid; k < PITCH_HDR; k += STATE_BLOCK) hdr[k] = 0;
    return;
  }
  // what the next output may read: everything from i_next - 31 on (never before the current base, never past what was received)
  int64_t nb = (int64_t)(((uint64_t)r.n1 * (uint64_t)r.inc) >> 32) - (HALF - 1);
  nb = nb < r.w.tail_base ? r.w.tail_base : nb;
  nb = nb > r.w.recv ? r.w.recv : nb;
  if (r.w.recv - nb > PITCH_TAIL) nb = r.w.recv - PITCH_TAIL;  // (unreachable: the bound in sopro_hip.h)
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

}  // namespace

int64_t sopro_pitch_out_len(int64_t in_len, int64_t inc) {
  if (in_len < 0 || in_len > LEN_MAX || inc < INC_MIN || inc > INC_MAX) return -1;
  return (in_len << 32) / inc;
}

int64_t sopro_pitch_chunk_out_cap(int64_t in_len) {
  if (in_len < 0 || in_len > LEN_MAX) return -1;
  return 2 * (in_len + NT) + 2;
}

int64_t sopro_pitch_state_bytes(int32_t rows) { return rows <= 0 ? 0 : (int64_t)rows * STATE_WORDS * (int64_t)sizeof(int64_t); }

int sopro_pitch_rows_f32(const float* in, int64_t in_stride, const int32_t* in_lens, int64_t in_cap, const int64_t* incs, const int32_t* bank_idx,
                         const float* banks, int32_t n_banks, int32_t rows, void* state, int32_t flush, float* out, int64_t out_stride,
                         int64_t out_cap, int32_t* out_lens, void* stream) {
  SOPRO_CHECK_ARG(in_lens && incs && bank_idx && banks && out_lens, "in_lens, incs, bank_idx, banks, out_lens must be non-NULL");
  SOPRO_CHECK_ARG(rows > 0 && rows <= 65535, "0 < rows <= 65535");
  SOPRO_CHECK_ARG(n_banks > 0, "n_banks > 0");
  SOPRO_CHECK_ARG(in_cap >= 0 && in_cap <= LEN_MAX, "0 <= in_cap <= 2^30");
  SOPRO_CHECK_ARG(in || in_cap == 0, "in must be non-NULL when in_cap > 0");
  SOPRO_CHECK_ARG(in_stride >= 0 && out_stride >= 0, "strides >= 0");
  SOPRO_CHECK_ARG(out_cap >= 0 && out_cap <= INT32_MAX, "0 <= out_cap < 2^31");
  SOPRO_CHECK_ARG(out || out_cap == 0, "out must be non-NULL when out_cap > 0");
  SOPRO_CHECK_ARG(rows == 1 || out_cap == 0 || out_stride >= out_cap, "out_stride >= out_cap (rows must not overlap)");
  SOPRO_CHECK_ARG(state || flush, "a call without state is the whole row: flush must be set");
  SOPRO_CHECK_ARG(((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 3u) == 0, "in, out must be 4-byte aligned");
  SOPRO_CHECK_ARG((reinterpret_cast<uintptr_t>(banks) & 15u) == 0, "banks must be 16-byte aligned");
  SOPRO_CHECK_ARG((reinterpret_cast<uintptr_t>(state) & 7u) == 0, "state must be 8-byte aligned");
  constexpr size_t lds = (size_t)LDS_FLOATS * sizeof(float);
  SOPRO_SET_MAX_LDS_ONCE(pitch_rows_kernel, lds);
  const int64_t tiles = out_cap > 0 ? (out_cap + PITCH_TILE - 1) / PITCH_TILE : 1;
  hipLaunchKernelGGL(pitch_rows_kernel, dim3((unsigned)tiles, (unsigned)rows), dim3(PITCH_BLOCK), lds, (hipStream_t)stream, in, in_stride, in_lens,
                     in_cap, incs, bank_idx, banks, n_banks, static_cast<const int64_t*>(state), flush ? 1 : 0, out, out_stride, out_cap, out_lens);
  if (state)
    hipLaunchKernelGGL(pitch_state_kernel, dim3(rows), dim3(STATE_BLOCK), 0, (hipStream_t)stream, in, in_stride, in_lens, in_cap, incs,
                       static_cast<int64_t*>(state), flush ? 1 : 0, out_cap);
  SOPRO_LAUNCH_CHECK();
}
