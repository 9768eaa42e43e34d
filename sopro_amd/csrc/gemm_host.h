// Host-side argument checks shared by the tiled contractions' entry points (gemm_f32.hip, gemm_bf16s.hip, gemm_8p.hip): no device code.
#pragma once
#include "common.h"

// SOPRO_CHECK_ARG for a helper that checks on behalf of `who` (an entry point's __func__): the error text names the caller
#define SOPRO_CHECK_AS(who, cond, msg)                        \
  do {                                                        \
    if (!(cond)) {                                            \
      sopro_set_error("%s: bad argument: %s", who, msg);      \
      return -2;                                              \
    }                                                         \
  } while (0)

enum gemm_operands {
  GEMM_F32_ROWS,   // sopro_gemm_f32: fp32 A and W rows, no ext
  GEMM_PACKED_W,   // the tile kernel's families: fp32 (or bf16) A rows, fragment-ordered weight
  GEMM_SPLIT_ROWS  // the long-K form: split-form A and W rows, whose own stricter rules follow at the caller
};

// A zero segment stride means "dense": segments follow each other without padding rows.  Then the checks every contraction makes of its
// sizes, operand pointers and the epilogue's / prologue's own operands.  `w`: the weight the call reads (g.W or the packed one).
inline int gemm_check_basic(const char* who, sopro_gemm_args& g, sopro_gemm_split_ext* ext, const void* w, gemm_operands ops) {
  if (g.a_seg_stride == 0) g.a_seg_stride = (int64_t)g.rows_per_seg * g.lda;
  if (g.c_seg_stride == 0) g.c_seg_stride = (int64_t)g.rows_per_seg * g.ldc;
  if (g.r_seg_stride == 0) g.r_seg_stride = (int64_t)g.rows_per_seg * g.ldr;
  if (ext && ext->c2_seg_stride == 0) ext->c2_seg_stride = (int64_t)g.rows_per_seg * ext->ldc2;
  if (ops == GEMM_SPLIT_ROWS) {
    SOPRO_CHECK_AS(who, g.M > 0 && g.N > 0 && g.K > 0 && g.rows_per_seg > 0, "M, N, K, rows_per_seg must be positive");
    return 0;
  }
  const bool packed = ops == GEMM_PACKED_W;
  SOPRO_CHECK_AS(who, g.M > 0 && g.N > 0 && g.K > 0, "M, N, K must be positive");
  SOPRO_CHECK_AS(who, (g.K & 3) == 0, "K must be a multiple of 4");
  SOPRO_CHECK_AS(who, g.rows_per_seg > 0, "rows_per_seg must be positive");
  SOPRO_CHECK_AS(who, g.A && w && (g.C || (ext && ext->c_mode == 5)), packed ? "A, packed_w, C must be non-NULL" : "A, W, C must be non-NULL");
  SOPRO_CHECK_AS(who, aligned16(g.A) && aligned16(w), packed ? "A and packed_w must be 16-byte aligned" : "A and W must be 16-byte aligned");
  SOPRO_CHECK_AS(who, (g.lda & 3) == 0 && (packed || (g.ldw & 3) == 0) && (g.a_seg_stride & 3) == 0,
                 packed ? "lda, a_seg_stride must be multiples of 4" : "lda, ldw, a_seg_stride must be multiples of 4");
  SOPRO_CHECK_AS(who, g.epilogue != SOPRO_EPI_RES || g.R != nullptr, "EPI_RES needs R");
  SOPRO_CHECK_AS(who, g.prologue != SOPRO_PRO_ADDVEC || (g.pro_vec && aligned16(g.pro_vec)), "PRO_ADDVEC needs an aligned pro_vec");
  SOPRO_CHECK_AS(who, g.epilogue != SOPRO_EPI_GLU || (g.N % 64) == 0, "EPI_GLU needs N % 64 == 0 (packed value/gate blocks)");
  return 0;
}

// Destination rows of the output modes that write something other than plain fp32 C: c_mode 1 / 2 = ELU + split form (to C / to C2 next
// to the fp32 C), 3 / 4 = ELU as fp32 (likewise), 6 / 7 / 8 = bf16 rows (C, C2 for 8 and the skip operand R point at bf16 elements,
// strides count elements).  Which modes an entry point takes at all is its own whitelist.  `n_apart`: N % 4 is refused under a text of
// its own (the three-pass entries); the one-pass entry names N in the row text.
inline int gemm_check_out_rows(const char* who, const sopro_gemm_args& g, const sopro_gemm_split_ext& ext, bool n_apart) {
  if (ext.c_mode >= 6) {
    SOPRO_CHECK_AS(who, (g.N & 3) == 0 && g.C && (reinterpret_cast<uintptr_t>(g.C) & 7u) == 0 && (g.ldc & 3) == 0 && (g.c_seg_stride & 3) == 0 && g.ldc >= g.N,
                   "bf16 output rows must be 8-byte aligned (N, ld, seg stride multiples of 4)");
    SOPRO_CHECK_AS(who, ext.c_mode != 8 || (ext.C2 && (reinterpret_cast<uintptr_t>(ext.C2) & 7u) == 0 && (ext.ldc2 & 3) == 0 && (ext.c2_seg_stride & 3) == 0 && ext.ldc2 >= g.N),
                   "c_mode 8: C2 (the activated bf16 copy) must be given, 8-byte aligned rows");
    SOPRO_CHECK_AS(who, g.epilogue != SOPRO_EPI_RES || ((reinterpret_cast<uintptr_t>(g.R) & 7u) == 0 && (g.ldr & 3) == 0 && (g.r_seg_stride & 3) == 0),
                   "bf16 skip operand rows must be 8-byte aligned");
    return 0;
  }
  if (ext.c_mode < 1 || ext.c_mode > 4) return 0;
  if (n_apart) SOPRO_CHECK_AS(who, (g.N & 3) == 0, "activated output: N % 4 == 0");
  const bool second = ext.c_mode == 2 || ext.c_mode == 4;
  const float* d = second ? ext.C2 : g.C;
  const int64_t ldd = second ? ext.ldc2 : g.ldc, dseg = second ? ext.c2_seg_stride : g.c_seg_stride;
  if (ext.c_mode <= 2)
    SOPRO_CHECK_AS(who, d && (reinterpret_cast<uintptr_t>(d) & 127u) == 0 && (ldd & 31) == 0 && (dseg & 31) == 0 && ldd >= g.N,
                   "split-form output rows must start on 128-byte boundaries (ld, seg stride multiples of 32)");
  else
    SOPRO_CHECK_AS(who, (g.N & 3) == 0 && d && aligned16(d) && (ldd & 3) == 0 && (dseg & 3) == 0 && ldd >= g.N,
                   n_apart ? "activated output rows must be 16-byte aligned (ld, seg stride multiples of 4)"
                           : "activated output rows must be 16-byte aligned (N, ld, seg stride multiples of 4)");
  return 0;
}
