// Prints what the tiled contractions' entry points answer to each class of bad argument their checks name: one line per call with the
// return code and sopro_last_error().  A refusal comes before any launch, so the program needs no GPU - and hides every device from
// itself, because the operand addresses are aligned host dummies: a call that an entry point does take (each spoiled call goes to all
// six) then ends at its first runtime query with -1 instead of launching.  Diff the output of two builds of the library to see that a
// change of the host code refuses the same calls with the same texts:
//   hipcc -I include tools/gemm_refusals.cpp -o gemm_refusals -L sopro_amd -lsopro_hip -Wl,-rpath,$PWD/sopro_amd && ./gemm_refusals
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>

#include "sopro_hip.h"

namespace {

alignas(128) char buf[6][256];
float* at(int i, int off = 0) { return reinterpret_cast<float*>(buf[i] + off); }

struct Case {
  sopro_gemm_args g;
  sopro_gemm_split_ext x;
  const void* w;
};

// a call every family takes: 128 x 256 x 64, fp32 rows, dense
Case good() {
  Case c;
  memset(&c, 0, sizeof(c));
  c.g.A = at(0); c.g.W = at(1); c.g.C = at(2);
  c.g.M = 128; c.g.N = 256; c.g.K = 64;
  c.g.lda = 64; c.g.ldw = 64; c.g.ldc = 256; c.g.ldr = 256;
  c.g.rows_per_seg = 128;
  c.x.ldc2 = 256;
  c.x.acc_scale = 1.f;
  c.w = at(1);
  return c;
}

typedef int (*entry)(const sopro_gemm_args*, const void*, const sopro_gemm_split_ext*, void*);
int f32(const sopro_gemm_args* g, const void* w, const sopro_gemm_split_ext*, void* s) {
  if (!g) return sopro_gemm_f32(nullptr, s);
  sopro_gemm_args a = *g;
  a.W = static_cast<const float*>(w);
  return sopro_gemm_f32(&a, s);
}
int long_k(const sopro_gemm_args* g, const void* w, const sopro_gemm_split_ext* x, void* s) {
  if (!g || !x) return sopro_gemm_bf16x3_8p(g, w, x, s);
  sopro_gemm_split_ext e = *x;
  if (e.a_format == 0) e.a_format = 1;  // (9 asks for fp32 rows)
  if (e.a_format == 9) e.a_format = 0;
  return sopro_gemm_bf16x3_8p(g, w, &e, s);
}

const struct { const char* name; entry fn; } ENTRIES[] = {{"bf16x3", sopro_gemm_bf16x3}, {"bf16x1", sopro_gemm_bf16x1}, {"bf16x6", sopro_gemm_bf16x6},
                                                          {"f16x3", sopro_gemm_f16x3},   {"f32", f32},              {"8p", long_k}};

void run(const char* what, const std::function<void(Case&)>& spoil) {
  for (const auto& e : ENTRIES) {
    Case c = good();
    spoil(c);
    const int rc = e.fn(&c.g, c.w, &c.x, nullptr);
    printf("%-7s %-28s rc %2d  %s\n", e.name, what, rc, rc == -2 ? sopro_last_error() : "(passes the checks)");
  }
}

}  // namespace

int main() {
  setvbuf(stdout, nullptr, _IOLBF, 0);
  setenv("HIP_VISIBLE_DEVICES", "-1", 1);
  setenv("ROCR_VISIBLE_DEVICES", "-1", 1);
  for (const auto& e : ENTRIES) printf("%-7s %-28s rc %2d  %s\n", e.name, "args NULL", e.fn(nullptr, at(1), nullptr, nullptr), sopro_last_error());
  {
    Case c = good();
    printf("%-7s %-28s rc %2d  %s\n", "f16x3", "ext NULL", sopro_gemm_f16x3(&c.g, c.w, nullptr, nullptr), sopro_last_error());
    printf("%-7s %-28s rc %2d  %s\n", "8p", "ext NULL", sopro_gemm_bf16x3_8p(&c.g, c.w, nullptr, nullptr), sopro_last_error());
  }
  // sizes, pointers, strides
  run("M 0", [](Case& c) { c.g.M = 0; });
  run("K 6", [](Case& c) { c.g.K = 6; });
  run("K 48", [](Case& c) { c.g.K = 48; c.x.rms_norm = 1; c.x.rms_eps = 1e-5f; });
  run("rows_per_seg 0", [](Case& c) { c.g.rows_per_seg = 0; });
  run("A NULL", [](Case& c) { c.g.A = nullptr; });
  run("W NULL", [](Case& c) { c.w = nullptr; });
  run("C NULL", [](Case& c) { c.g.C = nullptr; });
  run("A + 4 bytes", [](Case& c) { c.g.A = at(0, 4); });
  run("A + 16 bytes", [](Case& c) { c.g.A = at(0, 16); c.x.a_format = 1; });
  run("W + 16 bytes", [](Case& c) { c.w = at(1, 16); c.g.N = 96; });
  run("lda 6", [](Case& c) { c.g.lda = 6; });
  run("lda 36, split-form A", [](Case& c) { c.g.lda = 36; c.x.a_format = 1; });
  run("ldw 6", [](Case& c) { c.g.ldw = 6; c.g.N = 96; });
  run("N 128", [](Case& c) { c.g.N = 128; });
  // prologues and epilogues
  run("prologue ELU", [](Case& c) { c.g.prologue = SOPRO_PRO_ELU; c.x.a_format = 1; });
  run("prologue ADDVEC, no vector", [](Case& c) { c.g.prologue = SOPRO_PRO_ADDVEC; });
  run("prologue ADDVEC", [](Case& c) { c.g.prologue = SOPRO_PRO_ADDVEC; c.g.pro_vec = at(3); c.x.c_mode = 3; });
  run("prologue 7", [](Case& c) { c.g.prologue = 7; });
  run("epilogue RES, no R", [](Case& c) { c.g.epilogue = SOPRO_EPI_RES; });
  run("epilogue GLU, N 96", [](Case& c) { c.g.epilogue = SOPRO_EPI_GLU; c.g.N = 96; });
  run("epilogue GLU, c_mode 3", [](Case& c) { c.g.epilogue = SOPRO_EPI_GLU; c.x.c_mode = 3; });
  run("epilogue TANH", [](Case& c) { c.g.epilogue = SOPRO_EPI_TANH; });
  run("epilogue 99", [](Case& c) { c.g.epilogue = 99; });
  run("epilogue ROPE, no tables", [](Case& c) { c.g.epilogue = SOPRO_EPI_ROPE; });
  run("epilogue ROPE, dh 12", [](Case& c) { c.g.epilogue = SOPRO_EPI_ROPE; c.x.rope_cos = at(3); c.x.rope_sin = at(4); c.x.rope_dh = 12; });
  // operand formats and output modes
  run("a_format 1", [](Case& c) { c.x.a_format = 1; c.g.epilogue = SOPRO_EPI_GELU; });
  run("a_format 2, prologue ELU", [](Case& c) { c.x.a_format = 2; c.g.prologue = SOPRO_PRO_ELU; });
  run("a_format 2, lda 6", [](Case& c) { c.x.a_format = 2; c.g.lda = 6; });
  run("a_format 2, RES to fp32", [](Case& c) { c.x.a_format = 2; c.g.epilogue = SOPRO_EPI_RES; c.g.R = at(3); });
  run("a_format 9", [](Case& c) { c.x.a_format = 9; });
  run("c_mode 1, C + 16 bytes", [](Case& c) { c.x.c_mode = 1; c.g.C = at(2, 16); });
  run("c_mode 2, no C2", [](Case& c) { c.x.c_mode = 2; });
  run("c_mode 2, ldc2 36", [](Case& c) { c.x.c_mode = 2; c.x.C2 = at(3); c.x.ldc2 = 36; });
  run("c_mode 3, N 6", [](Case& c) { c.x.c_mode = 3; c.g.N = 6; });
  run("c_mode 3, ldc 6", [](Case& c) { c.x.c_mode = 3; c.g.ldc = 6; });
  run("c_mode 3, C + 4 bytes", [](Case& c) { c.x.c_mode = 3; c.g.C = at(2, 4); });
  run("c_mode 4, no C2", [](Case& c) { c.x.c_mode = 4; });
  run("c_mode 4, ldc2 < N", [](Case& c) { c.x.c_mode = 4; c.x.C2 = at(3); c.x.ldc2 = 128; });
  run("c_mode 4, c2 seg stride 6", [](Case& c) { c.x.c_mode = 4; c.x.C2 = at(3); c.x.c2_seg_stride = 6; });
  run("c_mode 5, no C2", [](Case& c) { c.x.c_mode = 5; });
  run("c_mode 5, epilogue GELU", [](Case& c) { c.x.c_mode = 5; c.x.C2 = at(3); c.g.epilogue = SOPRO_EPI_GELU; });
  run("c_mode 6, ldc 6", [](Case& c) { c.x.c_mode = 6; c.g.ldc = 6; });
  run("c_mode 7, RES, R + 4 bytes", [](Case& c) { c.x.c_mode = 7; c.g.epilogue = SOPRO_EPI_RES; c.g.R = at(3, 4); });
  run("c_mode 8, no C2", [](Case& c) { c.x.c_mode = 8; });
  run("c_mode 9", [](Case& c) { c.x.c_mode = 9; });
  // split-K, fused norms
  run("ksplit 65", [](Case& c) { c.x.ksplit = 65; });
  run("ksplit 2, no workspace", [](Case& c) { c.x.ksplit = 2; });  // (refused at the launch, behind the first runtime query: -1 without a device)
  run("ksplit 2 with the probe", [](Case& c) { c.x.ksplit = 2; c.g.dbg = reinterpret_cast<long long*>(at(3)); c.x.a_format = 1; });
  run("RMSNorm", [](Case& c) { c.x.rms_norm = 1; c.x.rms_eps = 1e-5f; c.g.prologue = SOPRO_PRO_ADDVEC; c.g.pro_vec = at(3); });
  run("RMSNorm, ksplit 2", [](Case& c) { c.x.rms_norm = 1; c.x.rms_eps = 1e-5f; c.x.ksplit = 2; });
  run("RMSNorm, eps 0", [](Case& c) { c.x.rms_norm = 1; });
  run("RMSNorm, c_mode 3", [](Case& c) { c.x.rms_norm = 1; c.x.rms_eps = 1e-5f; c.x.c_mode = 3; });
  run("acc_scale 0", [](Case& c) { c.x.acc_scale = 0.f; });
  run("ln_stats, K 32", [](Case& c) { c.x.ln_stats = at(3); c.x.rms_eps = 1e-5f; c.g.K = 32; c.g.lda = 32; });
  run("ln_stats + 4 bytes", [](Case& c) { c.x.ln_stats = at(3, 4); c.x.rms_eps = 1e-5f; });
  run("ln_stats, eps 0", [](Case& c) { c.x.ln_stats = at(3); });
  run("ln_stats, epilogue RES", [](Case& c) { c.x.ln_stats = at(3); c.x.rms_eps = 1e-5f; c.g.epilogue = SOPRO_EPI_RES; c.g.R = at(4); });
  run("ln_stats_out, epilogue NONE", [](Case& c) { c.x.ln_stats_out = at(3); });
  run("ln_stats_out, ldr 6", [](Case& c) { c.x.ln_stats_out = at(3); c.g.epilogue = SOPRO_EPI_RES; c.g.R = at(4); c.g.ldr = 6; });
  return 0;
}
