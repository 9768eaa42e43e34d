// Pitch tracking: the fundamental frequency of every 10 ms frame of the rows of a padded batch (contract: include/sopro_hip.h "pitch
// tracking", DESIGN.md "Pitch tracking"; numpy restatement: tests/f0_ref.py).  A call is three launches per group of F0_GROUP rows:
//   front - one workgroup per run of G frames: the G + 2 blocks of H samples the run reads and TMAX more are staged in LDS; a thread
//           owns four consecutive lags of one block and walks the block four samples at a time, the lagged samples sliding through
//           registers (two 16-byte LDS reads feed 16 terms); then one wave per frame: the frame's energy, d = p[f] + p[f + 1] + p[f + 2],
//           the prefix sum over the lags (seven lags per lane, one cross-lane scan), the normalisation into LDS, and the candidate pick
//           on the packed key (q, lag) from there: v never goes to memory unless dbg_v asks for it
//   path  - one wave per row: the integer Viterbi recursion over frames in chunks of 64 (in parallel a lane turns a frame's candidates
//           into the 5 x 5 step costs; in sequence lanes 0 .. 4 are the states and the previous totals travel as scalars), one
//           back-pointer word per frame, the backtrace on scalars
//   out   - one thread per frame: the parabolic refinement of the chosen lag, f0 and strength
// sopro_f0_paths runs the pick as a kernel of its own on a given v (one wave per frame), then path and out.
// A partial sum depends on its own block's samples only, a frame on its own three blocks, and everything after v is integer, so a row
// has the same bits alone and in a batch, and two calls give the same bits.  The row lengths and parameters are host values and travel
// as kernel arguments: a call neither copies nor synchronises.
#include <math.h>

#include "common.h"

namespace {

constexpr int H = SOPRO_F0_H, W = SOPRO_F0_W, TMIN = SOPRO_F0_TMIN, TMAX = SOPRO_F0_TMAX, SPAN = SOPRO_F0_SPAN, K = SOPRO_F0_K;
constexpr int NV = TMAX + 1;
constexpr int F0_GROUP = 64;  // rows of one launch group (their lengths and parameters are kernel arguments)
constexpr int G = 8, NB = G + 2;  // frames and blocks of one front workgroup
constexpr int FRONT_BLOCK = 256, FRONT_WAVES = FRONT_BLOCK / 64;
constexpr int LG = 101;                  // lag groups of a block: group g owns the lags 4g .. 4g + 3 (lag 0 and lags past TMAX are not used)
constexpr int PW = 4 * LG;               // row pitch of the partial sums and of v in LDS
constexpr int XS = NB * H + PW + 4;      // staged samples: the last group of the last block reads up to (NB - 1) H + H - 1 + PW - 1 + 4
constexpr int SCAN = 7;                  // lags of one lane in the prefix sum: 64 x 7 >= TMAX
constexpr int CH = 64;                   // frames of one chunk of the path kernel
constexpr int OUT_BLOCK = 256;
constexpr int NS = K + 1;                // states of a frame: unvoiced and the K candidates
constexpr int INF = 1 << 24, INF8 = INF << 3;  // an absent state's cost and total (totals are kept times 8)
constexpr int64_t LEN_MAX = (int64_t)1 << 24;
constexpr int WS_WORDS = K + 3 * K + 1;  // words of a frame in the workspace: keys [K] | v triples [K][3] | back-pointers, then the state
static_assert(W == 3 * H && SPAN == W + TMAX && H % 4 == 0 && K == 4 && TMAX % 4 == 0, "the front end adds three block partials per frame");
static_assert(64 * SCAN >= TMAX && (TMAX - TMIN + 63) / 64 <= 6, "a lane holds its lags of the scan and of the pick in registers");
static_assert(G % FRONT_WAVES == 0, "every wave of the front workgroup has the same number of frames");

struct Rows {
  int32_t n[F0_GROUP];     // samples (sopro_f0_paths: not used)
  int32_t F[F0_GROUP];     // frames
  float gate[F0_GROUP];    // W 10^(floor_db / 10)
  float thr[F0_GROUP];
  int16_t oct[F0_GROUP], unv[F0_GROUP], jump[F0_GROUP], sw[F0_GROUP];
};
struct LTab {
  int16_t l[PW];  // round(256 log2(lag)), lag = 1 .. TMAX; made on the host in double
};

__host__ __device__ __forceinline__ int64_t frames_of(int64_t n) { return n < SPAN ? 0 : (n - SPAN) / H + 1; }
struct Ws {
  uint32_t* keys;  // [fcap][K]: q << 16 | lag by ascending lag, 0 = none
  float* tri;      // [fcap][K][3]: v[lag - 1], v[lag], v[lag + 1]
  uint32_t* bp;    // [fcap]: the predecessor of state s in bits 3s .. 3s + 2; after the backtrace the frame's state
};
__device__ __forceinline__ Ws ws_of(void* ws, int64_t row, int64_t fcap) {
  Ws w;
  w.keys = static_cast<uint32_t*>(ws) + row * fcap * WS_WORDS;
  w.tri = reinterpret_cast<float*>(w.keys + fcap * K);
  w.bp = w.keys + fcap * 4 * K;
  return w;
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t u = (uint32_t)__shfl_xor((int)v, o, 64);
    v = u < v ? u : v;
  }
  return v;
}

// Step 3 of one frame by one wave: v [NV] (LDS or memory), the K smallest keys (q, lag), by ascending lag into keys / tri.
__device__ __forceinline__ void pick_frame(const float* v, float e, float gate, float thr, int oct, const int16_t* lt, uint32_t* keys, float* tri,
                                           int lane) {
  uint32_t mine[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int tau = TMIN + lane + 64 * i;
    mine[i] = 0xffffffffu;
    if (tau < TMAX && e > gate) {
      const float a = v[tau - 1], b = v[tau], c = v[tau + 1];
      if (b < a && b <= c && b < thr) {
        const int q = min(1023, (int)floorf(1024.0f * b)) + ((oct * ((int)lt[tau] - (int)lt[TMIN])) >> 8);
        mine[i] = ((uint32_t)q << 16) | (uint32_t)tau;
      }
    }
  }
  uint32_t got[K], last = 0u;  // (keys are distinct and above 0: the next smallest is the smallest above the last)
#pragma unroll
  for (int k = 0; k < K; ++k) {
    uint32_t m = 0xffffffffu;
#pragma unroll
    for (int i = 0; i < 6; ++i) m = (mine[i] > last && mine[i] < m) ? mine[i] : m;
    m = wave_min_u32(m);
    got[k] = m;
    last = m;
  }
  // by ascending lag (none = 0xffffffff stays last): a five-comparator network on the low halves
  auto lag = [](uint32_t key) { return key == 0xffffffffu ? 0xffffffffu : (key & 0xffffu); };
  auto cswap = [&](uint32_t& a, uint32_t& b) {
    if (lag(a) > lag(b)) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
  };
  cswap(got[0], got[1]), cswap(got[2], got[3]), cswap(got[0], got[2]), cswap(got[1], got[3]), cswap(got[1], got[2]);
  if (lane < K) {
    const uint32_t key = lane == 0 ? got[0] : lane == 1 ? got[1] : lane == 2 ? got[2] : got[3];
    if (key == 0xffffffffu) {
      keys[lane] = 0u;
      tri[3 * lane] = tri[3 * lane + 1] = tri[3 * lane + 2] = 1.0f;
    } else {
      const int tau = (int)(key & 0xffffu);
      keys[lane] = key;
      tri[3 * lane] = v[tau - 1], tri[3 * lane + 1] = v[tau], tri[3 * lane + 2] = v[tau + 1];
    }
  }
}

// ---- front ----
__global__ __launch_bounds__(FRONT_BLOCK) void f0_front_kernel(const float* __restrict__ wav, int64_t row_stride, Rows rows, LTab lt, int row0,
                                                               void* __restrict__ ws, int64_t fcap, float* __restrict__ dbg_v,
                                                               float* __restrict__ dbg_e) {
  __shared__ __attribute__((aligned(16))) float s_x[XS];
  __shared__ __attribute__((aligned(16))) float s_p[NB * PW];
  __shared__ float s_v[G * PW];
  __shared__ int16_t s_lt[PW];
  const int r = blockIdx.y, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int32_t F = rows.F[r], fb = (int32_t)blockIdx.x * G;
  if (fb >= F) return;  // (uniform)
  const int32_t n = rows.n[r];
  const int64_t row = row0 + r;
  const float* x = wav + row * row_stride;
  const int64_t base = (int64_t)fb * H;
  for (int i = t; i < XS; i += FRONT_BLOCK) s_x[i] = base + i < n ? x[base + i] : 0.0f;  // nothing past n is read
  for (int i = t; i < PW; i += FRONT_BLOCK) s_lt[i] = lt.l[i];
  __syncthreads();
  // the partial sums p[b][lag] = sum over the block's samples j, ascending, of (x[j] - x[j + lag])^2
  for (int it = t; it < NB * LG; it += FRONT_BLOCK) {
    const int b = it / LG, g = it - b * LG;
    const float* xa = s_x + b * H;
    const float* xb = xa + 4 * g;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float4 lo = *reinterpret_cast<const float4*>(xb);
    for (int j = 0; j < H; j += 4) {
      const float4 a = *reinterpret_cast<const float4*>(xa + j);
      const float4 hi = *reinterpret_cast<const float4*>(xb + j + 4);
      const float av[4] = {a.x, a.y, a.z, a.w};
      const float bv[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int l = 0; l < 4; ++l) {
          const float df = av[u] - bv[u + l];
          acc[l] = fmaf(df, df, acc[l]);
        }
      }
      lo = hi;
    }
    *reinterpret_cast<float4*>(s_p + b * PW + 4 * g) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  }
  __syncthreads();
  const Ws w = ws_of(ws, row, fcap);
  const float gate = rows.gate[r], thr = rows.thr[r];
  const int oct = rows.oct[r];
  for (int fl = wv; fl < G; fl += FRONT_WAVES) {
    const int32_t f = fb + fl;
    if (f >= F) break;  // (uniform over the wave)
    // e[f]: a lane adds the squares of samples lane, lane + 64, .. in ascending order, then one fixed cross-lane tree
    float e = 0.0f;
    for (int j = lane; j < W; j += 64) {
      const float s = s_x[fl * H + j];
      e = fmaf(s, s, e);
    }
    e = wave_sum(e);
    // d, c: lane owns the lags 1 + 7 lane .. 7 + 7 lane; c = (sum of the lanes before, by a cross-lane scan) + (d of the lane's own lags so far)
    float d[SCAN], c[SCAN], run = 0.0f;
#pragma unroll
    for (int u = 0; u < SCAN; ++u) {
      const int tau = 1 + SCAN * lane + u;
      d[u] = tau <= TMAX ? (s_p[fl * PW + tau] + s_p[(fl + 1) * PW + tau]) + s_p[(fl + 2) * PW + tau] : 0.0f;
      run += d[u];
      c[u] = run;
    }
    float incl = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    const float before = __shfl_up(incl, 1, 64);
    float* v = s_v + fl * PW;
#pragma unroll
    for (int u = 0; u < SCAN; ++u) {
      const int tau = 1 + SCAN * lane + u;
      const float cc = lane == 0 ? c[u] : before + c[u];
      if (tau <= TMAX) v[tau] = cc == 0.0f ? 1.0f : d[u] * (float)tau / cc;
    }
    if (lane == 0) v[0] = 1.0f;
    wave_lds_sync();
    if (dbg_v) {
      float* o = dbg_v + (row * fcap + f) * NV;
      for (int i = lane; i < NV; i += 64) o[i] = v[i];
    }
    if (dbg_e && lane == 0) dbg_e[row * fcap + f] = e;
    pick_frame(v, e, gate, thr, oct, s_lt, w.keys + (int64_t)f * K, w.tri + (int64_t)f * 3 * K, lane);
  }
}

// ---- pick (sopro_f0_paths only) ----
__global__ __launch_bounds__(FRONT_BLOCK) void f0_pick_kernel(const float* __restrict__ v, const float* __restrict__ e, Rows rows, LTab lt, int row0,
                                                              void* __restrict__ ws, int64_t fcap) {
  __shared__ int16_t s_lt[PW];
  const int r = blockIdx.y, t = threadIdx.x, lane = t & 63;
  const int32_t F = rows.F[r], f = (int32_t)blockIdx.x * FRONT_WAVES + (t >> 6);
  for (int i = t; i < PW; i += FRONT_BLOCK) s_lt[i] = lt.l[i];
  __syncthreads();
  if (f >= F) return;  // (uniform over the wave)
  const int64_t row = row0 + r;
  const Ws w = ws_of(ws, row, fcap);
  pick_frame(v + (row * fcap + f) * NV, e[row * fcap + f], rows.gate[r], rows.thr[r], rows.oct[r], s_lt, w.keys + (int64_t)f * K,
             w.tri + (int64_t)f * 3 * K, lane);
}

// ---- path ----
__global__ __launch_bounds__(64) void f0_path_kernel(Rows rows, LTab lt, int row0, void* __restrict__ ws, int64_t fcap, int32_t* __restrict__ nvoiced) {
  __shared__ __attribute__((aligned(16))) int s_add[CH][NS][8];
  __shared__ uint8_t s_arg[CH][8];
  __shared__ int16_t s_lt[PW];
  const int r = blockIdx.x, lane = threadIdx.x;
  const int64_t row = row0 + r;
  const int32_t F = rows.F[r];
  if (F == 0) {
    if (nvoiced && lane == 0) nvoiced[row] = 0;
    return;
  }
  for (int i = lane; i < PW; i += 64) s_lt[i] = lt.l[i];
  const Ws w = ws_of(ws, row, fcap);
  const int jump = rows.jump[r], sw = rows.sw[r], unv = rows.unv[r];
  const int st = lane < NS ? lane : 0;  // (lanes past the states mirror state 0; nothing of theirs is read or stored)
  int tot = 0;                          // the state's total, times 8 (the low three bits carry the predecessor through the minimum)
  wave_lds_sync();
  for (int32_t base = 0; base < F; base += CH) {
    const int cnt = F - base < CH ? F - base : CH;
    // in parallel, a frame per lane: what a step adds for every (state, predecessor), with the state's own cost folded in
    if (lane < cnt) {
      const int32_t f = base + lane;
      int cost[NS], lg[NS], lp[NS];
      cost[0] = unv, lg[0] = lp[0] = 0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const uint32_t key = w.keys[(int64_t)f * K + k], prev = f > 0 ? w.keys[(int64_t)(f - 1) * K + k] : 0u;
        cost[k + 1] = key ? (int)(key >> 16) : INF;
        lg[k + 1] = key ? (int)s_lt[key & 0xffffu] : 0;
        lp[k + 1] = prev ? (int)s_lt[prev & 0xffffu] : 0;
      }
#pragma unroll
      for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int p = 0; p < NS; ++p) {
          const int d = lg[s] > lp[p] ? lg[s] - lp[p] : lp[p] - lg[s];
          const int tr = (s == 0 && p == 0) ? 0 : (s == 0 || p == 0) ? sw : ((jump * d) >> 8);
          int add = cost[s] < INF ? ((tr + cost[s]) << 3) | p : INF8 | p;  // (an absent predecessor carries INF8 in its total)
          if (f == 0) add = p == 0 && cost[s] < INF ? cost[s] << 3 : INF8 | p;  // the first frame: the state's cost alone
          s_add[lane][s][p] = add;
        }
      }
    }
    wave_lds_sync();
    // in sequence: tot[s] = min over p of tot[p] + add[s][p]; the low bits of the minimum are the smallest p that reaches it
    int4 a = *reinterpret_cast<const int4*>(&s_add[0][st][0]);
    int a4 = s_add[0][st][4];
    for (int i = 0; i < cnt; ++i) {
      const int4 c = a;
      const int c4 = a4;
      if (i + 1 < cnt) {  // (the next frame's row is under way while this one is used)
        a = *reinterpret_cast<const int4*>(&s_add[i + 1][st][0]);
        a4 = s_add[i + 1][st][4];
      }
      int best = __builtin_amdgcn_readlane(tot, 0) + c.x;
      best = min(best, __builtin_amdgcn_readlane(tot, 1) + c.y);
      best = min(best, __builtin_amdgcn_readlane(tot, 2) + c.z);
      best = min(best, __builtin_amdgcn_readlane(tot, 3) + c.w);
      best = min(best, __builtin_amdgcn_readlane(tot, 4) + c4);
      tot = best >= INF8 ? INF8 : best & ~7;
      if (lane < NS) s_arg[i][lane] = (uint8_t)(best & 7);
    }
    // once per chunk the smallest total is subtracted: no decision changes, and CH steps add less than INF / 8
    int m = __builtin_amdgcn_readlane(tot, 0);
#pragma unroll
    for (int p = 1; p < NS; ++p) m = min(m, __builtin_amdgcn_readlane(tot, p));
    tot = tot >= INF8 ? INF8 : tot - m;
    wave_lds_sync();
    if (lane < cnt) {
      uint32_t word = 0u;
#pragma unroll
      for (int s = 0; s < NS; ++s) word |= (uint32_t)s_arg[lane][s] << (3 * s);
      w.bp[base + lane] = word;
    }
  }
  // the last frame's state: the smallest total, ties to the smaller state
  int s = 0, m = __builtin_amdgcn_readlane(tot, 0);
#pragma unroll
  for (int p = 1; p < NS; ++p) {
    const int tp = __builtin_amdgcn_readlane(tot, p);
    if (tp < m) m = tp, s = p;
  }
  // the backtrace, a chunk at a time: a lane holds its frame's word, the walk reads it as a scalar; the word becomes the frame's state
  int nv = 0;
  for (int32_t base = ((F - 1) / CH) * CH; base >= 0; base -= CH) {
    const int cnt = F - base < CH ? F - base : CH;
    const uint32_t word_mine = lane < cnt ? w.bp[base + lane] : 0u;  // (a lane reads the word it wrote itself)
    int state_mine = 0;
    for (int i = cnt - 1; i >= 0; --i) {
      if (lane == i) state_mine = s;
      s = (int)(((uint32_t)__builtin_amdgcn_readlane((int)word_mine, i) >> (3 * s)) & 7u);
    }
    if (lane < cnt) w.bp[base + lane] = (uint32_t)state_mine;
    nv += __popcll(__ballot(lane < cnt && state_mine > 0));
  }
  if (nvoiced && lane == 0) nvoiced[row] = nv;
}

// ---- out ----
__global__ __launch_bounds__(OUT_BLOCK) void f0_out_kernel(Rows rows, int row0, const void* __restrict__ ws, int64_t fcap, float* __restrict__ f0,
                                                           float* __restrict__ strength, int64_t out_stride, int32_t* __restrict__ dbg_cands) {
  const int r = blockIdx.y;
  const int32_t f = (int32_t)blockIdx.x * OUT_BLOCK + threadIdx.x;
  if (f >= rows.F[r]) return;
  const int64_t row = row0 + r;
  const Ws w = ws_of(const_cast<void*>(ws), row, fcap);
  const uint32_t* keys = w.keys + (int64_t)f * K;
  if (dbg_cands) {
#pragma unroll
    for (int k = 0; k < K; ++k) dbg_cands[(row * fcap + f) * K + k] = (int32_t)(keys[k] & 0xffffu);
  }
  const int s = (int)w.bp[f];
  float hz = 0.0f, st = 0.0f;
  if (s > 0) {
    const float* tr = w.tri + ((int64_t)f * K + (s - 1)) * 3;
    const float a = tr[0], b = tr[1], c = tr[2];
    const float den = fmaf(-2.0f, b, a) + c;
    float off = den > 0.0f ? 0.5f * (a - c) / den : 0.0f;
    off = fminf(0.5f, fmaxf(-0.5f, off));
    hz = 24000.0f / ((float)(keys[s - 1] & 0xffffu) + off);
    st = 1.0f - fminf(1.0f, b);
  }
  f0[row * out_stride + f] = hz;
  strength[row * out_stride + f] = st;
}

const LTab& ltab() {
  static const LTab tab = [] {
    LTab t = {};
    for (int tau = 1; tau <= TMAX; ++tau) t.l[tau] = (int16_t)lrint(256.0 * log2((double)tau));
    return t;
  }();
  return tab;
}

int64_t ws_bytes_of(int64_t rows, int64_t fcap) { return (rows * fcap * WS_WORDS + 1) * (int64_t)sizeof(int32_t); }

// One row's parameters (threshold, floor_db, octave_cost, jump_cost, switch_cost, unvoiced_cost) into slot r; the message of the first bad one
const char* take_params(const float* p, Rows& g, int r) {
  auto whole = [](float v, float hi) { return v >= 0.0f && v <= hi && v == floorf(v); };
  if (!(p[0] > 0.0f && p[0] <= 1.0f)) return "0 < threshold <= 1";
  if (!(p[1] >= -100.0f && p[1] <= 0.0f)) return "-100 <= floor_db <= 0";
  if (!whole(p[2], (float)SOPRO_F0_COST_MAX)) return "octave_cost must be an integer in 0 .. 1024";
  if (!whole(p[3], (float)SOPRO_F0_JUMP_MAX)) return "jump_cost must be an integer in 0 .. 4096";
  if (!whole(p[4], (float)SOPRO_F0_JUMP_MAX)) return "switch_cost must be an integer in 0 .. 4096";
  if (!whole(p[5], (float)SOPRO_F0_COST_MAX)) return "unvoiced_cost must be an integer in 0 .. 1024";
  g.thr[r] = p[0];
  g.gate[r] = (float)((double)W * pow(10.0, (double)p[1] / 10.0));
  g.oct[r] = (int16_t)p[2], g.jump[r] = (int16_t)p[3], g.sw[r] = (int16_t)p[4], g.unv[r] = (int16_t)p[5];
  return nullptr;
}

}  // namespace

int64_t sopro_f0_workspace_bytes(int32_t rows, int64_t cap) {
  if (rows <= 0 || cap < 0 || cap > LEN_MAX) return -1;
  return ws_bytes_of(rows, frames_of(cap));
}

int sopro_f0_rows_f32(const float* wav, int64_t row_stride, const int32_t* lens, const float* params, int32_t rows, float* f0, float* strength,
                      int64_t out_stride, int32_t* nvoiced, float* dbg_v, float* dbg_e, int32_t* dbg_cands, void* ws, int64_t ws_bytes,
                      void* stream) {
  SOPRO_CHECK_ARG(lens && params && nvoiced, "lens, params (host arrays) and nvoiced must be non-NULL");
  SOPRO_CHECK_ARG(rows > 0 && rows <= 65535, "0 < rows <= 65535");
  int64_t cap = 0;
  Rows scratch = {};
  for (int b = 0; b < rows; ++b) {
    SOPRO_CHECK_ARG(lens[b] >= 0 && lens[b] <= LEN_MAX, "0 <= lens[b] <= 2^24");
    cap = lens[b] > cap ? lens[b] : cap;
    const char* bad = take_params(params + SOPRO_F0_PARAMS * b, scratch, 0);
    SOPRO_CHECK_ARG(!bad, bad);
  }
  const int64_t fcap = frames_of(cap);
  SOPRO_CHECK_ARG(fcap == 0 || (wav && f0 && strength), "wav, f0, strength must be non-NULL when a row has a frame");
  SOPRO_CHECK_ARG(row_stride >= 0 && out_stride >= 0, "strides >= 0");
  SOPRO_CHECK_ARG(rows == 1 || (row_stride >= cap && out_stride >= fcap), "row_stride >= max(lens) and out_stride >= frames(max(lens)) (rows must not overlap)");
  SOPRO_CHECK_ARG(((reinterpret_cast<uintptr_t>(wav) | reinterpret_cast<uintptr_t>(f0) | reinterpret_cast<uintptr_t>(strength) |
                    reinterpret_cast<uintptr_t>(nvoiced) | reinterpret_cast<uintptr_t>(dbg_v) | reinterpret_cast<uintptr_t>(dbg_e) |
                    reinterpret_cast<uintptr_t>(dbg_cands)) & 3u) == 0,
                  "wav, f0, strength, nvoiced, dbg_v, dbg_e, dbg_cands must be 4-byte aligned");
  SOPRO_CHECK_ARG(ws && (reinterpret_cast<uintptr_t>(ws) & 3u) == 0, "ws must be non-NULL and 4-byte aligned");
  SOPRO_CHECK_ARG(ws_bytes >= ws_bytes_of(rows, fcap), "ws_bytes < sopro_f0_workspace_bytes(rows, max(lens))");
  hipStream_t s = (hipStream_t)stream;
  for (int row0 = 0; row0 < rows; row0 += F0_GROUP) {
    const int nr = rows - row0 < F0_GROUP ? rows - row0 : F0_GROUP;
    Rows g = {};
    int32_t fmax = 0;
    for (int r = 0; r < nr; ++r) {
      take_params(params + SOPRO_F0_PARAMS * (row0 + r), g, r);
      g.n[r] = lens[row0 + r];
      g.F[r] = (int32_t)frames_of(g.n[r]);
      fmax = g.F[r] > fmax ? g.F[r] : fmax;
    }
    if (fmax > 0)
      hipLaunchKernelGGL(f0_front_kernel, dim3((unsigned)((fmax + G - 1) / G), (unsigned)nr), dim3(FRONT_BLOCK), 0, s, wav, row_stride, g, ltab(), row0,
                         ws, fcap, dbg_v, dbg_e);
    hipLaunchKernelGGL(f0_path_kernel, dim3((unsigned)nr), dim3(64), 0, s, g, ltab(), row0, ws, fcap, nvoiced);
    if (fmax > 0)
      hipLaunchKernelGGL(f0_out_kernel, dim3((unsigned)((fmax + OUT_BLOCK - 1) / OUT_BLOCK), (unsigned)nr), dim3(OUT_BLOCK), 0, s, g, row0, ws, fcap, f0,
                         strength, out_stride, dbg_cands);
  }
  SOPRO_LAUNCH_CHECK();
}

int sopro_f0_paths(const float* v, const float* e, const int32_t* frames, const float* params, int32_t rows, int32_t fcap, float* f0, float* strength,
                   int64_t out_stride, int32_t* dbg_cands, void* ws, int64_t ws_bytes, void* stream) {
  SOPRO_CHECK_ARG(frames && params, "frames and params (host arrays) must be non-NULL");
  SOPRO_CHECK_ARG(rows > 0 && rows <= 65535, "0 < rows <= 65535");
  SOPRO_CHECK_ARG(fcap >= 0 && fcap <= frames_of(LEN_MAX), "0 <= fcap <= frames(2^24)");
  Rows scratch = {};
  int32_t fall = 0;
  for (int b = 0; b < rows; ++b) {
    SOPRO_CHECK_ARG(frames[b] >= 0 && frames[b] <= fcap, "0 <= frames[b] <= fcap");
    fall = frames[b] > fall ? frames[b] : fall;
    const char* bad = take_params(params + SOPRO_F0_PARAMS * b, scratch, 0);
    SOPRO_CHECK_ARG(!bad, bad);
  }
  SOPRO_CHECK_ARG(fall == 0 || (v && e && f0 && strength), "v, e, f0, strength must be non-NULL when a row has a frame");
  SOPRO_CHECK_ARG(rows == 1 || out_stride >= fall, "out_stride >= max(frames) (rows must not overlap)");
  SOPRO_CHECK_ARG(((reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(f0) | reinterpret_cast<uintptr_t>(strength) |
                    reinterpret_cast<uintptr_t>(dbg_cands)) & 3u) == 0,
                  "v, e, f0, strength, dbg_cands must be 4-byte aligned");
  SOPRO_CHECK_ARG(ws && (reinterpret_cast<uintptr_t>(ws) & 3u) == 0, "ws must be non-NULL and 4-byte aligned");
  SOPRO_CHECK_ARG(ws_bytes >= ws_bytes_of(rows, fcap), "ws_bytes < sopro_f0_workspace_bytes(rows, SPAN + (fcap - 1) H)");
  hipStream_t s = (hipStream_t)stream;
  for (int row0 = 0; row0 < rows; row0 += F0_GROUP) {
    const int nr = rows - row0 < F0_GROUP ? rows - row0 : F0_GROUP;
    Rows g = {};
    int32_t fmax = 0;
    for (int r = 0; r < nr; ++r) {
      take_params(params + SOPRO_F0_PARAMS * (row0 + r), g, r);
      g.F[r] = frames[row0 + r];
      fmax = g.F[r] > fmax ? g.F[r] : fmax;
    }
    if (fmax == 0) continue;
    hipLaunchKernelGGL(f0_pick_kernel, dim3((unsigned)((fmax + FRONT_WAVES - 1) / FRONT_WAVES), (unsigned)nr), dim3(FRONT_BLOCK), 0, s, v, e, g, ltab(),
                       row0, ws, (int64_t)fcap);
    hipLaunchKernelGGL(f0_path_kernel, dim3((unsigned)nr), dim3(64), 0, s, g, ltab(), row0, ws, (int64_t)fcap, (int32_t*)nullptr);
    hipLaunchKernelGGL(f0_out_kernel, dim3((unsigned)((fmax + OUT_BLOCK - 1) / OUT_BLOCK), (unsigned)nr), dim3(OUT_BLOCK), 0, s, g, row0, ws,
                       (int64_t)fcap, f0, strength, out_stride, dbg_cands);
  }
  SOPRO_LAUNCH_CHECK();
}
