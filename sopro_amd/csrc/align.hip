// Word timestamps: the attention maps of the AR generator's text cross-attention and the best monotonic path through them
// (contract: include/sopro_hip.h, definition: DESIGN.md "Word timestamps").
//
//   align_scores - one launch per attention layer over (utterance, frame tile): P[h][t, s] = softmax_s(q_t . k_s * scale) for the
//                  selected heads, their weighted sum added to acc[t, s]; the last layer's launch finishes with log(max(acc, 1e-9)).
//                  A thread owns keys s = tid + 256 j and keeps their logits and the head sum in registers; the workgroup only
//                  meets for the two reductions of the softmax (maximum, sum).
//   align_dp     - one workgroup per utterance walks the frames: D[t][s] = score[t][s] + max(D[t-1][s], D[t-1][s-1]), one fp32 add
//                  per cell; the decision "came from s - 1" is one bit per cell, 64 keys' bits are one __ballot word.  Up to 64
//                  keys: one wave, D in a register per lane, the neighbour through a lane shift.  Up to 2048: a double-buffered row
//                  in LDS, one barrier per frame.  The scores of the next frames are loaded ahead of the recurrence.  One lane walks
//                  the bits back, then every frame writes its token's boundaries.
//   align_online - the same recurrence for a stream: one wave per row continues from the last committed cell over the frames that
//                  arrived since (at most 63, so the reachable band is one wave wide), backtracks from the best end it can see and
//                  commits everything but the last `lag` frames; the row's state stays in device memory between the calls.
#include <math.h>

#include "common.h"

namespace {

constexpr int AL_NT = 256;      // threads per workgroup of both kernels' wide forms
constexpr int AL_DH = 96;       // head width (cfg.d_model / 4 heads of the AR text cross-attention)
constexpr int AL_SMAX = 2048;   // keys
constexpr int AL_HMAX = 8;      // heads per layer
constexpr float AL_FLOOR = 1e-9f;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// TT frames x (256 JM) keys per workgroup.  Dynamic LDS: TT * D floats of queries; static: the reductions' scratch.
template <int TT, int JM>
__global__ __launch_bounds__(AL_NT) void align_scores_kernel(const float* __restrict__ Q, int64_t ldq, int64_t q_bstride,
                                                             const float* __restrict__ K, int64_t ldk, int64_t k_bstride,
                                                             const int32_t* __restrict__ tlens, const int32_t* __restrict__ slens,
                                                             int32_t T_cap, int32_t S_cap, int32_t H, float scale, uint32_t head_mask,
                                                             float weight, int32_t mode, float* __restrict__ acc, int64_t ld_acc,
                                                             int64_t acc_bstride) {
  extern __shared__ float4 al_smem4[];
  float* qs = reinterpret_cast<float*>(al_smem4);  // [TT][H * 96]
  __shared__ float red[AL_NT / 64][TT];
  const int b = blockIdx.x, t0 = blockIdx.y * TT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int T = tlens[b], S = slens[b];
  T = T < 0 ? 0 : (T > T_cap ? T_cap : T);
  S = S < 0 ? 0 : (S > S_cap ? S_cap : S);
  if (t0 >= T || S <= 0) return;  // (uniform over the workgroup) padding frames are left as they are
  const int D = H * AL_DH;
  const float* qb = Q + (int64_t)b * q_bstride;
  const float* kb = K + (int64_t)b * k_bstride;
  for (int i = tid; i < TT * (D / 4); i += AL_NT) {
    const int t = i / (D / 4), c4 = i - t * (D / 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t0 + t < T) v = *reinterpret_cast<const float4*>(qb + (int64_t)(t0 + t) * ldq + c4 * 4);
    reinterpret_cast<float4*>(qs)[i] = v;
  }
  __syncthreads();

  float sum[JM][TT];
#pragma unroll
  for (int j = 0; j < JM; ++j)
#pragma unroll
    for (int t = 0; t < TT; ++t) sum[j][t] = 0.f;

  for (int h = 0; h < H; ++h) {
    if (!((head_mask >> h) & 1u)) continue;  // (uniform)
    float l[JM][TT];
#pragma unroll
    for (int j = 0; j < JM; ++j) {
      const int s = tid + AL_NT * j;
#pragma unroll
      for (int t = 0; t < TT; ++t) l[j][t] = 0.f;
      if (s < S) {
        const float4* kp = reinterpret_cast<const float4*>(kb + (int64_t)s * ldk + h * AL_DH);
#pragma unroll
        for (int c8 = 0; c8 < AL_DH / 32; ++c8) {
          float4 kv[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) kv[i] = kp[c8 * 8 + i];
#pragma unroll
          for (int t = 0; t < TT; ++t) {
            const float4* qp = reinterpret_cast<const float4*>(qs + t * D + h * AL_DH + c8 * 32);
            float a = l[j][t];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              const float4 qv = qp[i];
              a = fmaf(qv.x, kv[i].x, a);
              a = fmaf(qv.y, kv[i].y, a);
              a = fmaf(qv.z, kv[i].z, a);
              a = fmaf(qv.w, kv[i].w, a);
            }
            l[j][t] = a;
          }
        }
#pragma unroll
        for (int t = 0; t < TT; ++t) l[j][t] *= scale;
      } else {
#pragma unroll
        for (int t = 0; t < TT; ++t) l[j][t] = -INFINITY;
      }
    }
    // sweep 1: the row maxima
    float mx[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      float m = l[0][t];
#pragma unroll
      for (int j = 1; j < JM; ++j) m = fmaxf(m, l[j][t]);
      mx[t] = wave_max(m);
    }
    __syncthreads();  // (the previous head's sums have been read)
    if (lane == 0) {
#pragma unroll
      for (int t = 0; t < TT; ++t) red[wave][t] = mx[t];
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      float m = red[0][t];
#pragma unroll
      for (int w = 1; w < AL_NT / 64; ++w) m = fmaxf(m, red[w][t]);
      mx[t] = m;
    }
    // sweep 2: exponentials and their sums
    float den[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      float a = 0.f;
#pragma unroll
      for (int j = 0; j < JM; ++j) {
        const float e = (tid + AL_NT * j < S) ? expf(l[j][t] - mx[t]) : 0.f;
        l[j][t] = e;
        a += e;
      }
      den[t] = wave_sum(a);
    }
    __syncthreads();  // (the maxima have been read)
    if (lane == 0) {
#pragma unroll
      for (int t = 0; t < TT; ++t) red[wave][t] = den[t];
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      float a = red[0][t];
#pragma unroll
      for (int w = 1; w < AL_NT / 64; ++w) a += red[w][t];
      const float wn = weight / a;
#pragma unroll
      for (int j = 0; j < JM; ++j) sum[j][t] = fmaf(l[j][t], wn, sum[j][t]);
    }
  }

  float* ab = acc + (int64_t)b * acc_bstride;
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    if (t0 + t >= T) continue;
#pragma unroll
    for (int j = 0; j < JM; ++j) {
      const int s = tid + AL_NT * j;
      if (s >= S) continue;
      float* p = ab + (int64_t)(t0 + t) * ld_acc + s;
      float v = sum[j][t];
      if (mode != 0) v += *p;
      if (mode == 2) v = logf(fmaxf(v, AL_FLOOR));
      *p = v;
    }
  }
}

// The recurrence's one operation is an add that must stay an add (no neighbouring multiply exists here, but the rule of the file is
// the rule of tsm.hip: every operation of the definition is rounded on its own).
#pragma clang fp contract(off)

constexpr int DP_AHEAD = 8;  // frames whose scores are in registers ahead of the recurrence (one wave form)
constexpr int DP_AHEAD_W = 4;  // ... of the wide form (x 8 keys per thread)
constexpr int DP_JM = AL_SMAX / AL_NT;

struct DpOut {
  int32_t* path;
  int32_t* bounds;
  float* total;
  int32_t* status;
};

// rows the recurrence does not apply to: T < S, T == 0 or S == 0
__device__ void dp_fallback(int T, int S, int tid, int nt, int32_t* path, int32_t* bounds, float* total, int32_t* status) {
  for (int t = tid; t < T; t += nt) path[t] = S > 0 ? (int)(((int64_t)t * S) / T) : 0;
  for (int s = tid; s < S; s += nt) {
    const int f = T > 0 ? (int)(((int64_t)s * T + S - 1) / S) : 0;
    const int hit = (T > 0 && f < T && (int)(((int64_t)f * S) / T) == s) ? 1 : 0;
    bounds[2 * s] = f;
    bounds[2 * s + 1] = f + hit;
  }
  if (tid == 0) {
    *total = 0.f;
    *status = 1;
  }
}

// after the forward walk: bits[t * W + (s >> 6)] bit (s & 63) says that cell (t, s) came from (t - 1, s - 1)
__device__ void dp_backtrack(int T, int S, int W, int tid, int nt, const unsigned long long* bits, int32_t* path, int32_t* bounds) {
  __threadfence_block();
  __syncthreads();
  if (tid == 0) {
    int s = S - 1;
    for (int t = T - 1; t > 0; --t) {
      path[t] = s;
      s -= (int)((bits[(int64_t)t * W + (s >> 6)] >> (s & 63)) & 1ull);
    }
    path[0] = s;
  }
  __threadfence_block();
  __syncthreads();
  for (int t = tid; t < T; t += nt) {
    const int s = path[t];
    if (t == 0 || path[t - 1] != s) bounds[2 * s] = t;
    if (t == T - 1 || path[t + 1] != s) bounds[2 * s + 1] = t + 1;
  }
}

__global__ __launch_bounds__(64) void align_dp_wave_kernel(const float* __restrict__ score, int64_t ld, int64_t bstride,
                                                           const int32_t* __restrict__ tlens, const int32_t* __restrict__ slens,
                                                           int32_t T_cap, int32_t S_cap, unsigned long long* __restrict__ ws,
                                                           int32_t* __restrict__ path, int64_t path_ld, int32_t* __restrict__ bounds,
                                                           float* __restrict__ total, int32_t* __restrict__ status) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int T = tlens[b], S = slens[b];
  T = T < 0 ? 0 : (T > T_cap ? T_cap : T);
  S = S < 0 ? 0 : (S > S_cap ? S_cap : S);
  int32_t* pth = path + (int64_t)b * path_ld;
  int32_t* bnd = bounds + (int64_t)b * S_cap * 2;
  if (T < S || T == 0 || S == 0) {
    dp_fallback(T, S, lane, 64, pth, bnd, total + b, status + b);
    return;
  }
  const float* sc = score + (int64_t)b * bstride;
  unsigned long long* bits = ws + (int64_t)b * T_cap;  // one word per frame
  const bool live = lane < S;
  float d = (lane == 0) ? sc[0] : -INFINITY;
  float nxt[DP_AHEAD];
#pragma unroll
  for (int i = 0; i < DP_AHEAD; ++i) nxt[i] = (live && 1 + i < T) ? sc[(int64_t)(1 + i) * ld + lane] : 0.f;
  for (int t = 1; t < T; t += DP_AHEAD) {
    float cur[DP_AHEAD];
#pragma unroll
    for (int i = 0; i < DP_AHEAD; ++i) cur[i] = nxt[i];
#pragma unroll
    for (int i = 0; i < DP_AHEAD; ++i) {  // the loads of the next group do not depend on the chain below
      const int tn = t + DP_AHEAD + i;
      nxt[i] = (live && tn < T) ? sc[(int64_t)tn * ld + lane] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < DP_AHEAD; ++i) {
      if (t + i < T) {  // (uniform)
        float left = __shfl_up(d, 1, 64);
        if (lane == 0) left = -INFINITY;
        const bool take = live && left > d;
        const unsigned long long w = __ballot(take);
        d = live ? cur[i] + (take ? left : d) : -INFINITY;
        if (lane == 0) bits[t + i] = w;
      }
    }
  }
  const float tot = __shfl(d, S - 1, 64);
  if (lane == 0) {
    total[b] = tot;
    status[b] = 0;
  }
  dp_backtrack(T, S, 1, lane, 64, bits, pth, bnd);
}

__global__ __launch_bounds__(AL_NT) void align_dp_wide_kernel(const float* __restrict__ score, int64_t ld, int64_t bstride,
                                                              const int32_t* __restrict__ tlens, const int32_t* __restrict__ slens,
                                                              int32_t T_cap, int32_t S_cap, unsigned long long* __restrict__ ws,
                                                              int32_t* __restrict__ path, int64_t path_ld, int32_t* __restrict__ bounds,
                                                              float* __restrict__ total, int32_t* __restrict__ status) {
  __shared__ float row[2][AL_SMAX + 1];  // row[.][0] = the -inf to the left of key 0; key s at [s + 1]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  int T = tlens[b], S = slens[b];
  T = T < 0 ? 0 : (T > T_cap ? T_cap : T);
  S = S < 0 ? 0 : (S > S_cap ? S_cap : S);
  const int W = (S_cap + 63) >> 6;
  int32_t* pth = path + (int64_t)b * path_ld;
  int32_t* bnd = bounds + (int64_t)b * S_cap * 2;
  if (T < S || T == 0 || S == 0) {
    dp_fallback(T, S, tid, AL_NT, pth, bnd, total + b, status + b);
    return;
  }
  const float* sc = score + (int64_t)b * bstride;
  unsigned long long* bits = ws + (int64_t)b * T_cap * W;
  const int nj = (S + AL_NT - 1) / AL_NT;  // (uniform) key groups in use
  for (int s = tid; s < S; s += AL_NT) row[0][s + 1] = (s == 0) ? sc[0] : -INFINITY;
  if (tid == 0) row[0][0] = row[1][0] = -INFINITY;
  float nxt[DP_AHEAD_W][DP_JM];
#pragma unroll
  for (int i = 0; i < DP_AHEAD_W; ++i)
#pragma unroll
    for (int j = 0; j < DP_JM; ++j) {
      const int s = tid + AL_NT * j;
      nxt[i][j] = (s < S && 1 + i < T) ? sc[(int64_t)(1 + i) * ld + s] : 0.f;
    }
  __syncthreads();
  for (int t = 1; t < T; t += DP_AHEAD_W) {
    float cur[DP_AHEAD_W][DP_JM];
#pragma unroll
    for (int i = 0; i < DP_AHEAD_W; ++i)
#pragma unroll
      for (int j = 0; j < DP_JM; ++j) cur[i][j] = nxt[i][j];
#pragma unroll
    for (int i = 0; i < DP_AHEAD_W; ++i)
#pragma unroll
      for (int j = 0; j < DP_JM; ++j) {
        const int s = tid + AL_NT * j, tn = t + DP_AHEAD_W + i;
        nxt[i][j] = (s < S && tn < T) ? sc[(int64_t)tn * ld + s] : 0.f;
      }
#pragma unroll
    for (int i = 0; i < DP_AHEAD_W; ++i) {
      if (t + i < T) {  // (uniform)
        const float* prev = row[(t + i - 1) & 1];
        float* out = row[(t + i) & 1];
#pragma unroll
        for (int j = 0; j < DP_JM; ++j) {
          if (j < nj) {  // (uniform)
            const int s = tid + AL_NT * j;
            const bool live = s < S;
            const float here = live ? prev[s + 1] : -INFINITY;
            const float left = live ? prev[s] : -INFINITY;
            const bool take = live && left > here;
            const unsigned long long w = __ballot(take);
            if (live) out[s + 1] = cur[i][j] + (take ? left : here);
            if (lane == 0 && (s >> 6) < W) bits[(int64_t)(t + i) * W + (s >> 6)] = w;
          }
        }
        __syncthreads();
      }
    }
  }
  if (tid == 0) {
    total[b] = row[(T - 1) & 1][S];
    status[b] = 0;
  }
  dp_backtrack(T, S, W, tid, AL_NT, bits, pth, bnd);
}

// The online form: one wave per row walks the frames that arrived since the last commit.  Lane l holds band position p + l (the
// committed position and what a step per frame can reach from it: at most 64 positions over 63 frames, whatever S is).  The
// decisions of a frame are one ballot word in LDS; lane 0 walks them back, then every lane stores its frame's position and
// fetches that cell's score, which lane 0 folds into the committed total in frame order.
constexpr int ON_WIN = SOPRO_ALIGN_WINDOW_MAX;

__global__ __launch_bounds__(64) void align_online_kernel(const float* __restrict__ score, int64_t ld, int64_t bstride,
                                                          const int32_t* __restrict__ t1s, const int32_t* __restrict__ slens,
                                                          const int32_t* __restrict__ finals, int32_t T_cap, int32_t S_cap, int32_t lag,
                                                          int32_t* __restrict__ state, int32_t* __restrict__ path, int64_t path_ld) {
  __shared__ unsigned long long bits[ON_WIN];
  __shared__ int32_t pos[ON_WIN];
  const int b = blockIdx.x, lane = threadIdx.x;
  int t1 = t1s[b], S = slens[b];
  t1 = t1 < 0 ? 0 : (t1 > T_cap ? T_cap : t1);
  S = S > S_cap ? S_cap : S;
  const bool fin = finals[b] != 0;
  int32_t* st = state + (int64_t)b * SOPRO_ALIGN_STATE_WORDS;
  const int c = st[0], p = st[1];
  const int a = c + 1, n = t1 - a;
  if (n <= 0 || S <= 0 || c < -1 || p < -1 || p >= S) return;  // (uniform) nothing new, or a state this entry never wrote
  if (!fin && t1 - 1 - lag < a) return;                          // (uniform) nothing can be committed yet
  if (n > ON_WIN) {                                              // (uniform) refused: the band would not fit the wave
    if (lane == 0) st[2] = 3;
    return;
  }
  const float* sc = score + (int64_t)b * bstride;
  const int s = p + lane;
  const bool live = s >= 0 && s < S;
  float d = (lane == 0) ? __int_as_float(st[4]) : -INFINITY;  // the virtual previous row: base at position p
  float nxt[DP_AHEAD];
#pragma unroll
  for (int i = 0; i < DP_AHEAD; ++i) nxt[i] = (live && i < n) ? sc[(int64_t)(a + i) * ld + s] : 0.f;
  for (int k = 0; k < n; k += DP_AHEAD) {
    float cur[DP_AHEAD];
#pragma unroll
    for (int i = 0; i < DP_AHEAD; ++i) cur[i] = nxt[i];
#pragma unroll
    for (int i = 0; i < DP_AHEAD; ++i) {  // the loads of the next group do not depend on the chain below
      const int kn = k + DP_AHEAD + i;
      nxt[i] = (live && kn < n) ? sc[(int64_t)(a + kn) * ld + s] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < DP_AHEAD; ++i) {
      if (k + i < n) {  // (uniform)
        float left = __shfl_up(d, 1, 64);
        if (lane == 0) left = -INFINITY;
        const bool take = live && left > d;
        const unsigned long long w = __ballot(take);
        d = live ? cur[i] + (take ? left : d) : -INFINITY;
        if (lane == 0) bits[k + i] = w;
      }
    }
  }
  // the end: the last position when the row is final and can reach it, else the best cell of the last frame (lowest position on ties)
  int e_lane = -1, status = 0;
  const int last_lane = S - 1 - p;
  if (fin && last_lane < 64) {
    const float v = __shfl(d, last_lane, 64);
    if (v > -INFINITY) e_lane = last_lane;
  }
  if (e_lane < 0) {
    float bv = d;
    int bi = lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    e_lane = bi;
    status = fin ? 2 : 0;
  }
  const int u = fin ? t1 - 1 : t1 - 1 - lag;  // the last frame this step commits (a <= u <= t1 - 1)
  __syncthreads();
  if (lane == 0) {
    int l = e_lane;
    for (int k = n - 1; k >= 0; --k) {
      pos[k] = p + l;
      l -= (int)((bits[k] >> l) & 1ull);
    }
  }
  __syncthreads();
  const int nc = u - a + 1;  // committed frames: 1 .. n
  float v = 0.f;
  int my = 0;
  if (lane < nc) {
    my = pos[lane];
    v = sc[(int64_t)(a + lane) * ld + my];
    path[(int64_t)b * path_ld + a + lane] = my;
  }
  float base = __int_as_float(st[4]);
  for (int k = 0; k < nc; ++k) base = base + __shfl(v, k, 64);  // (uniform; frame order, one fp32 add each)
  const int pu = __shfl(my, nc - 1, 64);
  if (lane == 0) {
    st[0] = u;
    st[1] = pu;
    st[2] = status;
    st[3] = p + e_lane;
    st[4] = __float_as_int(base);
  }
}

}  // namespace

int64_t sopro_align_ws_bytes(int32_t B, int32_t T_cap, int32_t S_cap) {
  if (B <= 0 || T_cap <= 0 || S_cap <= 0 || S_cap > AL_SMAX) return 0;
  return (int64_t)B * T_cap * ((S_cap + 63) / 64) * (int64_t)sizeof(unsigned long long);
}

int sopro_align_scores_f32(const float* Q, int64_t ldq, int64_t q_bstride, const float* K, int64_t ldk, int64_t k_bstride, const int32_t* tlens,
                           const int32_t* slens, int32_t B, int32_t T_cap, int32_t S_cap, int32_t H, int32_t dh, float scale, uint32_t head_mask,
                           float weight, int32_t mode, float* acc, int64_t ld_acc, int64_t acc_bstride, void* stream) {
  SOPRO_CHECK_ARG(Q && K && tlens && slens && acc, "Q, K, tlens, slens, acc must be non-NULL");
  SOPRO_CHECK_ARG(B > 0 && T_cap > 0 && S_cap > 0, "B, T_cap, S_cap > 0");
  SOPRO_CHECK_ARG(S_cap <= AL_SMAX, "S_cap <= 2048");
  SOPRO_CHECK_ARG(dh == AL_DH && H >= 1 && H <= AL_HMAX, "dh == 96 and 1 <= H <= 8");
  SOPRO_CHECK_ARG(mode >= 0 && mode <= 2, "mode in {0, 1, 2}");
  SOPRO_CHECK_ARG((head_mask >> H) == 0, "head_mask has bits past H");
  SOPRO_CHECK_ARG(ldq >= (int64_t)H * dh && ldk >= (int64_t)H * dh && ld_acc >= S_cap, "ldq, ldk >= H * dh and ld_acc >= S_cap");
  SOPRO_CHECK_ARG(ldq % 4 == 0 && ldk % 4 == 0 && q_bstride % 4 == 0 && k_bstride % 4 == 0, "ldq, ldk, q_bstride, k_bstride multiples of 4");
  SOPRO_CHECK_ARG(((reinterpret_cast<uintptr_t>(Q) | reinterpret_cast<uintptr_t>(K)) & 15u) == 0, "Q, K must be 16-byte aligned");
  SOPRO_CHECK_ARG(B == 1 || (q_bstride >= (int64_t)T_cap * ldq && k_bstride >= (int64_t)S_cap * ldk && acc_bstride >= (int64_t)T_cap * ld_acc),
                  "batch strides must cover a row block");
  SOPRO_CHECK_ARG(T_cap <= 65535 * 4, "T_cap too large for one launch");
  const int D = H * dh;
  if (S_cap <= 1024) {
    constexpr int TT = 8;
    hipLaunchKernelGGL((align_scores_kernel<TT, 4>), dim3(B, (T_cap + TT - 1) / TT), dim3(AL_NT), TT * D * sizeof(float), (hipStream_t)stream, Q, ldq,
                       q_bstride, K, ldk, k_bstride, tlens, slens, T_cap, S_cap, H, scale, head_mask, weight, mode, acc, ld_acc, acc_bstride);
  } else {
    constexpr int TT = 4;
    hipLaunchKernelGGL((align_scores_kernel<TT, 8>), dim3(B, (T_cap + TT - 1) / TT), dim3(AL_NT), TT * D * sizeof(float), (hipStream_t)stream, Q, ldq,
                       q_bstride, K, ldk, k_bstride, tlens, slens, T_cap, S_cap, H, scale, head_mask, weight, mode, acc, ld_acc, acc_bstride);
  }
  SOPRO_LAUNCH_CHECK();
}

int sopro_align_dp_f32(const float* score, int64_t ld, int64_t bstride, const int32_t* tlens, const int32_t* slens, int32_t B, int32_t T_cap,
                       int32_t S_cap, void* ws, int64_t ws_bytes, int32_t* path, int64_t path_ld, int32_t* bounds, float* total, int32_t* status,
                       void* stream) {
  SOPRO_CHECK_ARG(score && tlens && slens && ws && path && bounds && total && status, "every pointer must be non-NULL");
  SOPRO_CHECK_ARG(B > 0 && T_cap > 0 && S_cap > 0, "B, T_cap, S_cap > 0");
  SOPRO_CHECK_ARG(S_cap <= AL_SMAX, "S_cap <= 2048");
  SOPRO_CHECK_ARG(ld >= S_cap && path_ld >= T_cap, "ld >= S_cap and path_ld >= T_cap");
  SOPRO_CHECK_ARG(B == 1 || bstride >= (int64_t)T_cap * ld, "bstride must cover T_cap rows");
  SOPRO_CHECK_ARG(ws_bytes >= sopro_align_ws_bytes(B, T_cap, S_cap), "ws_bytes < sopro_align_ws_bytes(B, T_cap, S_cap)");
  SOPRO_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, "ws must be 8-byte aligned");
  if (S_cap <= 64) {
    hipLaunchKernelGGL(align_dp_wave_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, score, ld, bstride, tlens, slens, T_cap, S_cap,
                       static_cast<unsigned long long*>(ws), path, path_ld, bounds, total, status);
  } else {
    hipLaunchKernelGGL(align_dp_wide_kernel, dim3(B), dim3(AL_NT), 0, (hipStream_t)stream, score, ld, bstride, tlens, slens, T_cap, S_cap,
                       static_cast<unsigned long long*>(ws), path, path_ld, bounds, total, status);
  }
  SOPRO_LAUNCH_CHECK();
}

int sopro_align_online_f32(const float* score, int64_t ld, int64_t bstride, const int32_t* t1s, const int32_t* slens, const int32_t* finals,
                           int32_t B, int32_t T_cap, int32_t S_cap, int32_t lag, void* state, int32_t* path, int64_t path_ld, void* stream) {
  SOPRO_CHECK_ARG(score && t1s && slens && finals && state && path, "every pointer must be non-NULL");
  SOPRO_CHECK_ARG(B > 0 && T_cap > 0 && S_cap > 0, "B, T_cap, S_cap > 0");
  SOPRO_CHECK_ARG(S_cap <= AL_SMAX, "S_cap <= 2048");
  SOPRO_CHECK_ARG(lag >= 0, "lag >= 0");
  SOPRO_CHECK_ARG(ld >= S_cap && path_ld >= T_cap, "ld >= S_cap and path_ld >= T_cap");
  SOPRO_CHECK_ARG(B == 1 || bstride >= (int64_t)T_cap * ld, "bstride must cover T_cap rows");
  SOPRO_CHECK_ARG((reinterpret_cast<uintptr_t>(state) & 3u) == 0, "state must be 4-byte aligned");
  hipLaunchKernelGGL(align_online_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, score, ld, bstride, t1s, slens, finals, T_cap, S_cap, lag,
                     static_cast<int32_t*>(state), path, path_ld);
  SOPRO_LAUNCH_CHECK();
}
