// Last transposed convolution of the SEANet decoder, ConvTranspose1d(128 -> 64, k = 8, s = 4) at the 6 kHz -> 24 kHz level
// (HF:modeling_mimi.py:931-961, the fourth `MimiConvTranspose1d`), as the contraction it is after pack_convtr1d:
//     out[t, r*64 + co] = bias[co] + sum_k A[t, k] * W[r*64 + co, k],   A[t, :] = [ x[t-1, 0..127] | x[t, 0..127] ]   (K = 256)
// i.e. every input row makes one 256-float output row = its four output samples x 64 channels.  3.07 M rows for 32 x 200
// frames: 1.57 GB in, 3.1 GB out, 403 GFLOP.  On the generic tile kernel (gemm_bf16s.hip, 128x128 tiles) this shape is bound
// by its operand stream: with K = 256 a tile runs 8 K-steps, and two thirds of what it pulls through L2 is the SAME 256 KB of
// split weights again (2.26 ms, 178 TFLOP/s fp32-equivalent).
//
// WEIGHT-STATIONARY (the scheme of seanet_res.hip; the K walk itself is ws_walk of seanet_mma.h): the whole weight matrix lives
// in registers as split-bf16 MFMA B fragments for the life of a workgroup - eight waves, wave w owns output columns
// 32w .. 32w+31 over all of K: 16 substeps x (hi, lo) = 128 registers - and the workgroup walks `tiles` consecutive 64-row
// tiles of one utterance.  Per tile only the 65 input
// rows (33 KB, contiguous) come in and 64 KB go out: the kernel runs at the rate of its matrix-core work and its output
// stream.  x is the ACTIVATED input (the producer - sopro_seanet_res128_f32 - applied the ELU): it is split once per element
// while it is staged (LDS row = [128 hi | 128 lo] bf16 + 16 B pad = 528 B, so A row t is LDS rows t, t+1 and the 16-lane
// ds_read_b128 fragment reads are conflict free).  Two LDS tiles: the next tile is requested before and split after the
// current tile's matrix-core work, one barrier per tile.  Accumulators are stored straight from the MFMA layout: lanes 0-31
// of a register hold 32 consecutive columns of one row = one whole 128-byte line.
// Arithmetic: PASSES = 3: lo*hi + hi*lo + hi*hi on v_mfma_f32_32x32x16_bf16, fp32 accumulate (the decoder's three-pass class,
// gemm_bf16s.hip NPL = 2); PASSES = 1: hi*hi only (the engine's bf16 mode).
#include <type_traits>

#include "seanet_mma.h"

namespace {

constexpr int UC = 128;            // input channels
constexpr int UN = 256;            // output columns per input row (4 samples x 64 channels)
constexpr int UTO = 64;            // rows per tile
constexpr int UHR = UTO + 1;       // staged rows
constexpr int up_row_bytes(bool hb) { return hb ? bf16_row_bytes(UC) : split_row_bytes(UC); }
constexpr int up_lds_bytes(bool hb) { return 2 * UHR * up_row_bytes(hb); }  // two tiles: 68.6 KB fp32, 35.4 KB bf16

// x: row p of utterance b at x + b * x_seg_stride + p * 128; A row t = rows t, t+1 (the caller points x at the row BEFORE the
// first sample: a zero pad row).  out: row t at out + b * out_seg_stride + t * 256.
// HB (the bf16 mode's activation flow): x is the ACTIVATED input as bf16 rows (256 bytes per row: half the bytes in), the result
// leaves as bf16 rows (512 bytes per input row: half the bytes out), one MFMA pass on the rounded operands.  Staging is a pure
// 16-byte copy into the hi plane (LDS row = 128 bf16 + 16 B pad = 272 B: A row t is LDS rows t, t+1; the 16-lane ds_read_b128
// fragment reads stay conflict free); the stores go out as column pairs (pair_cols of seanet_mma.h).  Strides count elements.
template <int PASSES, bool HB>
__global__ __launch_bounds__(512, 1) void seanet_up128_kernel(const void* __restrict__ x, int64_t x_seg_stride,
                                                              const float* __restrict__ w, const float* __restrict__ bias,
                                                              void* __restrict__ out, int64_t out_seg_stride, int T, int tiles) {
  static_assert(!HB || PASSES == 1, "bf16 rows are a one-pass (bf16 mode) input form");
  using elem_t = std::conditional_t<HB, unsigned short, float>;
  using piece_t = std::conditional_t<HB, uint4, float4>;      // 16 bytes of a row
  constexpr int ROW = up_row_bytes(HB);
  constexpr int PE = 16 / (int)sizeof(elem_t);                // elements per piece
  constexpr int PSH = HB ? 4 : 5;                             // log2(pieces per row)
  constexpr int NV = ((UHR << PSH) + 511) / 512;              // pieces per thread and tile: 5 (fp32), 3 (bf16)
  extern __shared__ __attribute__((aligned(16))) unsigned char es_all[];  // [2][UHR * ROW], dynamic (fp32: over the 64 KB static limit)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y;
  const int frow = lane & 31, fg = lane >> 5;
  const elem_t* xb = static_cast<const elem_t*>(x) + (int64_t)b * x_seg_stride;
  elem_t* ob = static_cast<elem_t*>(out) + (int64_t)b * out_seg_stride;

  // ---- weights as (hi, lo) B fragments, once per workgroup: n = 32 * wave + (lane & 31), k = 16 * s + 8 * (lane >> 5) .. + 7
  uint4 wh[16], wl[PASSES == 3 ? 16 : 1];
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    uint4 lo;
    split8(w + (int64_t)(wave * 32 + frow) * (2 * UC) + s * 16 + fg * 8, wh[s], lo);
    if (PASSES == 3) wl[s] = lo;
    if ((s & 3) == 3) asm volatile("" ::: "memory");  // four substeps per memory round: all 32 loads at once need 128 more registers
  }
  const float bv = bias[wave * 32 + frow];

  // tile request: rows t0 .. t0 + 64, all loads issued back to back; rows past the end are redirected to row 0 (results of
  // those A rows are never stored), so the loads are branch-free
  piece_t v[NV];
  auto request = [&](int t0) {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const int idx = tid + q * 512;  // piece index
      const int r = idx >> PSH, c = idx & ((1 << PSH) - 1);
      const int p = t0 + r;
      const int pc = (r < UHR && p <= T) ? p : 0;
      v[q] = *reinterpret_cast<const piece_t*>(xb + (int64_t)pc * UC + c * PE);
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const int idx = tid + q * 512;
      const int r = idx >> PSH, c = idx & ((1 << PSH) - 1);
      if (r < UHR) {
        if constexpr (HB) {
          *reinterpret_cast<uint4*>(es_all + buf * (UHR * ROW) + r * ROW + c * 16) = v[q];
        } else {
          uint2 hi, lo;
          split2_bf16(v[q].x, v[q].y, hi.x, lo.x);
          split2_bf16(v[q].z, v[q].w, hi.y, lo.y);
          *reinterpret_cast<uint2*>(es_all + buf * (UHR * ROW) + r * ROW + c * 8) = hi;
          if (PASSES == 3) *reinterpret_cast<uint2*>(es_all + buf * (UHR * ROW) + r * ROW + 2 * UC + c * 8) = lo;
        }
      }
    }
  };

  const int tile0 = (int)blockIdx.x * tiles;
  if (tile0 * UTO >= T) return;
  request(tile0 * UTO);
  stage(0);
  __syncthreads();
  for (int it = 0; it < tiles; ++it) {
    const int t0 = (tile0 + it) * UTO;
    if (t0 >= T) break;  // uniform over the workgroup
    const int cur = it & 1;
    const bool more = it + 1 < tiles && t0 + UTO < T;
    if (more) request(t0 + UTO);

    f32x16 acc[2];
    ws_walk<PASSES, 16, ROW, 2 * UC>(es_all + cur * (UHR * ROW) + frow * ROW + fg * 16, 0, wh, wl, acc);
    // ---- store straight from the accumulator layout (seanet_mma.h)
    elem_t* ot = ob + (int64_t)t0 * UN;  // wave-uniform base + a 32-bit lane offset: no 64-bit address per store
    const bool full = t0 + UTO <= T;
    if constexpr (HB) {
      const bool odd = (lane & 1) != 0;
      const int colp = wave * 32 + (frow & ~1);  // first column of the pair
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
          float c0, c1;
          pair_cols(acc[mt][r] + bv, acc[mt][r + 1] + bv, odd, c0, c1);
          const int row = mt * 32 + acc32_row(r) + (odd ? 1 : 0) + 4 * fg;
          unsigned pk, lo_;
          split2_bf16(c0, c1, pk, lo_);
          if (full || t0 + row < T) *reinterpret_cast<unsigned*>(ot + (int64_t)row * UN + colp) = pk;
        }
    } else {
      const int col = wave * 32 + frow + 4 * fg * UN;
      if (full) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) ot[col + (mt * 32 + acc32_row(r)) * UN] = acc[mt][r] + bv;
      } else {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = mt * 32 + acc32_row(r);
            if (t0 + row + 4 * fg < T) ot[col + row * UN] = acc[mt][r] + bv;
          }
      }
    }
    if (more) stage(cur ^ 1);
    __syncthreads();  // the next tile is staged; every wave is done reading this one (it is rewritten one trip later)
  }
}

int g_up_tiles = 0;

template <int PASSES, bool HB>
int launch_up(const void* x, int64_t x_seg_stride, const float* w, const float* bias, void* out, int64_t out_seg_stride, int32_t B, int32_t T,
              hipStream_t s) {
  const int ntile = (T + UTO - 1) / UTO;
  // enough workgroups for ~4 per CU, as many tiles per workgroup as that leaves (the weight fragments are split once per workgroup)
  int tiles = g_up_tiles ? g_up_tiles : (int)(((int64_t)ntile * B + 1023) / 1024);
  if (tiles < 1) tiles = 1;
  auto kern = seanet_up128_kernel<PASSES, HB>;
  SOPRO_SET_MAX_LDS_ONCE(kern, up_lds_bytes(HB));
  hipLaunchKernelGGL(kern, dim3((unsigned)((ntile + tiles - 1) / tiles), (unsigned)B), dim3(512), up_lds_bytes(HB), s, x, x_seg_stride, w, bias, out,
                     out_seg_stride, T, tiles);
  SOPRO_LAUNCH_CHECK();
}

// What both entry points check about their strides and T: nullptr, or why the call is refused.
// T: t0 = (tile0 + it) * UTO of seanet_up128_kernel is a 32-bit int; the walk ends at the first t0 >= T, so t0 < T + UTO and
// t0 + UTO < T + 128 whatever `tiles` is.  Addresses are 64-bit.
const char* up_refusal(int64_t x_seg_stride, int64_t out_seg_stride, int32_t B, int32_t T) {
  if (B > 1 && (x_seg_stride < (int64_t)(T + 1) * UC || out_seg_stride < (int64_t)T * UN))
    return "segment strides: x holds T + 1 rows of 128 per utterance (one pad row in front), out T rows of 256";
  if (T > INT32_MAX - 128) return "T must stay at or below 2^31 - 129 rows per utterance (32-bit tile row index)";
  return nullptr;
}

}  // namespace

extern "C" int sopro_seanet_up_set_tiles(int tiles) {
  g_up_tiles = tiles > 0 ? tiles : 0;
  return 0;
}

// bf16 rows in, bf16 rows out (the bf16 mode's activation flow; one pass).  x: [B][>= 1 + T][128] bf16 (activated, row 0 of a
// segment = the zero row), out rows of 256 bf16; strides count bf16 elements.
extern "C" int sopro_seanet_up128_bf16(const void* x, int64_t x_seg_stride, const float* w, const float* bias, void* out,
                                       int64_t out_seg_stride, int32_t B, int32_t T, void* stream) {
  SOPRO_CHECK_ARG(x && w && bias && out && B > 0 && T > 0, "bad pointers or sizes");
  SOPRO_CHECK_ARG(aligned16(x) && aligned16(w) && (reinterpret_cast<uintptr_t>(out) & 3u) == 0 && (x_seg_stride & 7) == 0 && (out_seg_stride & 1) == 0,
                  "x, w 16-byte aligned, x segment stride % 8 == 0 (16-byte row pieces), out 4-byte aligned");
  { const char* why = up_refusal(x_seg_stride, out_seg_stride, B, T); SOPRO_CHECK_ARG(!why, why); }
  return launch_up<1, true>(x, x_seg_stride, w, bias, out, out_seg_stride, B, T, (hipStream_t)stream);
}

extern "C" int sopro_seanet_up128_f32(const float* x, int64_t x_seg_stride, const float* w, const float* bias, float* out,
                                      int64_t out_seg_stride, int32_t B, int32_t T, int32_t passes, void* stream) {
  SOPRO_CHECK_ARG(x && w && bias && out && B > 0 && T > 0, "bad pointers or sizes");
  SOPRO_CHECK_ARG(passes == 1 || passes == 3, "passes must be 3 (three-pass split-bf16) or 1 (bf16 mode)");
  SOPRO_CHECK_ARG(aligned16(x) && aligned16(w) && aligned16(out) && (x_seg_stride & 3) == 0 && (out_seg_stride & 3) == 0,
                  "x, w, out must be 16-byte aligned with segment strides % 4 == 0");
  { const char* why = up_refusal(x_seg_stride, out_seg_stride, B, T); SOPRO_CHECK_ARG(!why, why); }
  if (passes == 3) return launch_up<3, false>(x, x_seg_stride, w, bias, out, out_seg_stride, B, T, (hipStream_t)stream);
  return launch_up<1, false>(x, x_seg_stride, w, bias, out, out_seg_stride, B, T, (hipStream_t)stream);
}
