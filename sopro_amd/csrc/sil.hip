// Silence control: pauses longer than a cap are squeezed, the lead-in and the tail are trimmed (contract: include/sopro_hip.h,
// DESIGN.md "Silence control").  Memory-bound and on the path of every squeezed pass; a call is three launches (four with a state):
//   act     - (word of 64 hops, row), one wave per word: the lanes read a hop's 240 samples side by side, and one 64-bit ballot per
//             hop says whether any of them reaches the threshold; the wave's 64 answers are one word of the row's activity bitmap
//   plan    - one workgroup per row turns the bitmap into the row's segment table (output position, source position, kind), its cuts
//             and its length.  One-shot: a lane per word; the ends of the runs are bits of `word & ~(word << 1)`, the start of a run is
//             the last set bit before it (a prefix maximum over the words in LDS), the cuts' output positions an LDS prefix sum; the
//             workgroup loops when the row has more than SIL_PLAN_WORDS words.  Chunked: the hop-level state machine of the
//             definition, sequential over the call's bits (one lane), from and to the row's state
//   gather  - (tile of SIL_TILE outputs, row): a lane finds the segment of its four outputs by binary search and copies them, 16
//             bytes at a time where source and destination allow it; the fade hops are computed here
//   state   - (chunked) one workgroup per row rewrites the retained tail once every tile has read it (stream order)
// Both plans write the same table, so there is one gather.  The chunked form reads a virtual row: the retained tail, then the call's
// samples.
#include "common.h"

namespace {

constexpr int HOP = SOPRO_SIL_HOP;
constexpr int SIL_TAIL = SOPRO_SIL_TAIL;
constexpr int SIL_TILE = SOPRO_SIL_TILE;
constexpr int PLAN_WORDS = SOPRO_SIL_PLAN_WORDS;  // = threads of the plan workgroup: one wave
constexpr int ACT_BLOCK = 256, ACT_WAVES = ACT_BLOCK / 64;
constexpr int GATHER_BLOCK = 256;
constexpr int STATE_BLOCK = 256;
constexpr int B_MAX = 16, CAP_MAX = 1000;
constexpr int KEEP_MAX = B_MAX + 2;  // the held hop and a ring of b + 1
constexpr int64_t LEN_MAX = (int64_t)1 << 30;
static_assert(PLAN_WORDS == 64, "the plan workgroup is one wave");
static_assert(SIL_TILE == GATHER_BLOCK * 8, "two quads per lane");
static_assert(KEEP_MAX * HOP + HOP - 1 <= SIL_TAIL && HOP % 4 == 0, "the tail bound of sopro_hip.h; cuts keep 16-byte alignment");

enum { SEG_COPY = 0, SEG_IN = 1, SEG_OUT = 2, SEG_CROSS = 3 };

// state of one row: 8 int64 of header, then SIL_TAIL floats (whole hops first: the held hop, the ring; then the incomplete hop)
constexpr int H_SEEN = 0, H_RUN = 1, H_RECV = 2, H_EMIT = 3, H_THOPS = 4, H_TLEN = 5;
constexpr int SIL_HDR = 8;
constexpr int STATE_WORDS = SIL_HDR + SIL_TAIL / 2;

// workspace of one row, in int64 words: bitmap | the next header | meta (int32 x 32) | segments (int32 x 4 each)
constexpr int M_NSEG = 0, M_OUT = 1, M_NKEEP = 2, M_INC_SRC = 3, M_INC_LEN = 4, M_KEEP = 8;
constexpr int META_WORDS = 16;
struct Lay {
  int64_t wcap, seg_cap, stride;
};
__host__ __device__ __forceinline__ Lay layout(int64_t vcap) {
  Lay l;
  const int64_t nh = (vcap + HOP - 1) / HOP;
  l.wcap = nh / 64 + 1;
  l.seg_cap = nh + 8;  // (a cut needs four hops, a call of the chunked form at most one segment per hop and three more)
  l.stride = l.wcap + SIL_HDR + META_WORDS + 2 * l.seg_cap;
  return l;
}
struct Ws {
  uint64_t* words;
  int64_t* next;
  int32_t* meta;
  int32_t* segs;
  int64_t seg_cap;
};
__device__ __forceinline__ Ws ws_of(void* ws, int row, int64_t vcap) {
  const Lay l = layout(vcap);
  int64_t* base = static_cast<int64_t*>(ws) + (int64_t)row * l.stride;
  Ws w;
  w.words = reinterpret_cast<uint64_t*>(base);
  w.next = base + l.wcap;
  w.meta = reinterpret_cast<int32_t*>(base + l.wcap + SIL_HDR);
  w.segs = reinterpret_cast<int32_t*>(base + l.wcap + SIL_HDR + META_WORDS);
  w.seg_cap = l.seg_cap;
  return w;
}

struct Row {
  const float* in;    // this call's samples: virtual positions [tlen, vlen)
  const float* tail;  // the retained samples: virtual positions [0, tlen)
  int64_t seen, run, recv0, emit0;
  int thops, tlen, n_in;
  int64_t vlen;
  float thr;
  int cap_h, b, a;
  bool ident, bad;
};

// What a call finds for a row, from the arguments and the state as the call found it (every kernel of a call derives the same).
__device__ __forceinline__ Row row_setup(int row, const float* in, int64_t in_stride, const int32_t* in_lens, int64_t in_cap, const float* thr,
                                         const int32_t* cap_h, const int32_t* bs, const int64_t* state) {
  Row r;
  r.thr = thr[row];
  r.cap_h = cap_h[row];
  r.b = bs[row];
  r.a = r.cap_h - r.b;
  r.ident = r.cap_h == 0;
  r.bad = !r.ident && !(r.thr > 0.0f && r.b >= 1 && r.b <= B_MAX && r.cap_h >= r.b + 1 && r.cap_h <= CAP_MAX);
  const int64_t* hdr = state ? state + (int64_t)row * STATE_WORDS : nullptr;
  int64_t seen = 0, run = 0, recv = 0, emit = 0, thops = 0, tlen = 0;
  if (hdr) {
    seen = hdr[H_SEEN], run = hdr[H_RUN], recv = hdr[H_RECV], emit = hdr[H_EMIT], thops = hdr[H_THOPS], tlen = hdr[H_TLEN];
    // (a header nobody zeroed, or one left by other parameters: keep every derived index inside the buffers)
    bool ok = (seen == 0 || seen == 1) && run >= 0 && recv >= 0 && recv <= LEN_MAX && emit >= 0 && emit <= recv && run <= recv / HOP;
    if (ok && (r.ident || r.bad)) ok = thops == 0 && tlen == 0;
    if (ok && !r.ident && !r.bad) {
      const int64_t held = (seen && run >= r.a) ? 1 : 0;
      const int64_t elig = seen ? (run > r.a ? run - r.a : 0) : run;
      ok = thops == held + (elig < r.b + 1 ? elig : r.b + 1) && tlen == thops * HOP + recv % HOP;
    }
    if (!ok) seen = run = recv = emit = thops = tlen = 0;
  }
  int64_t n_in = in_lens[row];
  n_in = n_in < 0 ? 0 : (n_in > in_cap ? in_cap : n_in);
  n_in = recv + n_in > LEN_MAX ? LEN_MAX - recv : n_in;
  r.in = in + (int64_t)row * in_stride;
  r.tail = hdr ? reinterpret_cast<const float*>(hdr + SIL_HDR) : nullptr;
  r.seen = seen, r.run = run, r.recv0 = recv, r.emit0 = emit;
  r.thops = (int)thops, r.tlen = (int)tlen, r.n_in = (int)n_in;
  r.vlen = tlen + n_in;
  return r;
}

__device__ __forceinline__ float v_at(const Row& r, int64_t k) { return k < r.tlen ? r.tail[k] : r.in[k - r.tlen]; }

// ---- act ----
__global__ __launch_bounds__(ACT_BLOCK) void sil_act_kernel(const float* __restrict__ in, int64_t in_stride, const int32_t* __restrict__ in_lens,
                                                            int64_t in_cap, const float* __restrict__ thr, const int32_t* __restrict__ cap_h,
                                                            const int32_t* __restrict__ bs, const int64_t* __restrict__ state, int flush,
                                                            void* __restrict__ ws, int64_t vcap) {
  const int row = blockIdx.y, lane = threadIdx.x & 63;
  const Row r = row_setup(row, in, in_stride, in_lens, in_cap, thr, cap_h, bs, state);
  if (r.ident || r.bad) return;
  const int64_t nhv = flush ? (r.vlen + HOP - 1) / HOP : r.vlen / HOP;
  const int64_t w = (int64_t)blockIdx.x * ACT_WAVES + (threadIdx.x >> 6);
  if (w * 64 >= nhv) return;  // (uniform over the wave; w < wcap since nhv <= ceil(vcap / HOP))
  uint64_t word = 0;
  for (int h = 0; h < 64; ++h) {
    const int64_t lo = (w * 64 + h) * HOP;
    if (lo >= r.vlen || w * 64 + h >= nhv) break;
    const int64_t hi = lo + HOP < r.vlen ? lo + HOP : r.vlen;
    bool any = false;
    for (int64_t i = lo + lane; i < hi; i += 64) any |= fabsf(v_at(r, i)) >= r.thr;  // (a NaN compares false)
    if (__ballot(any) != 0) word |= (uint64_t)1 << h;
  }
  if (lane == 0) ws_of(ws, row, vcap).words[w] = word;
}

// ---- plan ----
__device__ __forceinline__ void put_seg(const Ws& w, int64_t idx, int64_t out, int64_t src, int64_t src2, int kind) {
  if (idx < 0 || idx >= w.seg_cap) return;
  int32_t* s = w.segs + 4 * idx;
  s[0] = (int32_t)out, s[1] = (int32_t)src, s[2] = (int32_t)src2, s[3] = kind;
}
__device__ __forceinline__ void put_cut(int32_t* cuts, int32_t cuts_cap, int row, int64_t idx, int64_t pos, int64_t n) {
  if (idx < 0 || idx >= cuts_cap) return;
  int32_t* c = cuts + ((int64_t)row * cuts_cap + idx) * 2;
  c[0] = (int32_t)pos, c[1] = (int32_t)n;
}
__device__ __forceinline__ int last_bit(uint64_t v) { return 63 - __clzll((long long)v); }  // v != 0

// The result of a row: lengths, the meta words the gather and the state kernel read.
__device__ __forceinline__ void finish(const Ws& w, int row, int64_t n_segs, int64_t out_len, int64_t n_cut, int64_t out_cap, int32_t cuts_cap,
                                       int32_t* out_lens, int32_t* n_cuts) {
  const bool fits = n_segs <= w.seg_cap && out_len <= out_cap && n_cut <= cuts_cap;
  w.meta[M_NSEG] = fits ? (int32_t)n_segs : 0;
  w.meta[M_OUT] = fits ? (int32_t)out_len : -1;
  out_lens[row] = fits ? (int32_t)out_len : -1;
  n_cuts[row] = fits ? (int32_t)n_cut : 0;
}

// One-shot: the whole row is here and nothing is retained.
__global__ __launch_bounds__(PLAN_WORDS) void sil_plan_kernel(const int32_t* __restrict__ in_lens, int64_t in_cap, const float* __restrict__ thr,
                                                              const int32_t* __restrict__ cap_h, const int32_t* __restrict__ bs,
                                                              void* __restrict__ ws, int64_t vcap, int64_t out_cap,
                                                              int32_t* __restrict__ out_lens, int32_t* __restrict__ cuts, int32_t cuts_cap,
                                                              int32_t* __restrict__ n_cuts) {
  __shared__ int64_t s_last[PLAN_WORDS];
  __shared__ int64_t s_cnt[PLAN_WORDS];
  __shared__ int64_t s_rem[PLAN_WORDS];
  const int row = blockIdx.x, t = threadIdx.x;
  const Row r = row_setup(row, nullptr, 0, in_lens, in_cap, thr, cap_h, bs, nullptr);
  const Ws w = ws_of(ws, row, vcap);
  const int64_t L = r.vlen;
  if (r.ident || r.bad) {  // (uniform over the workgroup)
    if (t == 0) {
      put_seg(w, 0, 0, 0, 0, SEG_COPY);
      finish(w, row, 1, r.bad ? out_cap + 1 : L, 0, out_cap, cuts_cap, out_lens, n_cuts);
    }
    return;
  }
  const int64_t nh = (L + HOP - 1) / HOP, W = (nh + 63) / 64;
  const int b = r.b, a = r.a, cap = r.cap_h;
  int64_t c_last = -1, c_cnt = 0, c_rem = 0;  // carried over the passes: the last active hop, cuts and samples removed so far
  for (int64_t wb = 0; wb < W; wb += PLAN_WORDS) {
    const int64_t wi = wb + t;
    const uint64_t word = wi < W ? w.words[wi] : 0;
    const uint64_t before = wi == 0 ? 1 : (wi < W ? w.words[wi - 1] >> 63 : 1);  // (hop -1 counts as active: no run ends at hop 0)
    s_last[t] = word ? wi * 64 + last_bit(word) : -1;
    __syncthreads();
    for (int o = 1; o < PLAN_WORDS; o <<= 1) {  // inclusive prefix maximum
      const int64_t v = t >= o ? s_last[t - o] : -1;
      __syncthreads();
      if (v > s_last[t]) s_last[t] = v;
      __syncthreads();
    }
    int64_t prev_w = t > 0 ? s_last[t - 1] : -1;  // the last active hop before this word
    prev_w = prev_w > c_last ? prev_w : c_last;
    const uint64_t ends = word & ~((word << 1) | before);  // active hops that follow an inactive one
    int64_t cnt = 0, rem = 0;
    for (uint64_t e = ends; e; e &= e - 1) {
      const int h = __ffsll((long long)e) - 1;
      const uint64_t low = word & (((uint64_t)1 << h) - 1);
      const int64_t j1 = wi * 64 + h, j0 = (low ? wi * 64 + last_bit(low) : prev_w) + 1, n = j1 - j0;
      if (j0 == 0 ? n > b + 1 : n > cap) {
        ++cnt;
        rem += (j0 == 0 ? j1 - b - 1 : n - cap) * HOP;
      }
    }
    s_cnt[t] = cnt, s_rem[t] = rem;
    __syncthreads();
    for (int o = 1; o < PLAN_WORDS; o <<= 1) {  // inclusive prefix sums
      const int64_t vc = t >= o ? s_cnt[t - o] : 0, vr = t >= o ? s_rem[t - o] : 0;
      __syncthreads();
      s_cnt[t] += vc, s_rem[t] += vr;
      __syncthreads();
    }
    int64_t k = c_cnt + s_cnt[t] - cnt, R = c_rem + s_rem[t] - rem;  // this word's first cut, and what was removed before it
    for (uint64_t e = ends; e; e &= e - 1) {
      const int h = __ffsll((long long)e) - 1;
      const uint64_t low = word & (((uint64_t)1 << h) - 1);
      const int64_t j1 = wi * 64 + h, j0 = (low ? wi * 64 + last_bit(low) : prev_w) + 1, n = j1 - j0;
      if (j0 == 0) {
        if (n <= b + 1) continue;
        const int64_t f = j1 - b - 1;
        put_cut(cuts, cuts_cap, row, k, 0, f * HOP);
        put_seg(w, 1 + 2 * k, 0, f * HOP, 0, SEG_IN);
        put_seg(w, 2 + 2 * k, HOP, (f + 1) * HOP, 0, SEG_COPY);
        R += f * HOP;
      } else {
        if (n <= cap) continue;
        const int64_t p = j0 + a, q = j1 - b;
        put_cut(cuts, cuts_cap, row, k, p * HOP, (q - p) * HOP);
        put_seg(w, 1 + 2 * k, (p - 1) * HOP - R, (p - 1) * HOP, (q - 1) * HOP, SEG_CROSS);
        R += (q - p) * HOP;
        put_seg(w, 2 + 2 * k, q * HOP - R, q * HOP, 0, SEG_COPY);
      }
      ++k;
    }
    const int64_t n_last = s_last[PLAN_WORDS - 1], n_cnt = s_cnt[PLAN_WORDS - 1], n_rem = s_rem[PLAN_WORDS - 1];
    __syncthreads();  // (the next pass overwrites the arrays)
    c_last = n_last > c_last ? n_last : c_last;
    c_cnt += n_cnt;
    c_rem += n_rem;
  }
  if (t != 0) return;
  put_seg(w, 0, 0, 0, 0, SEG_COPY);
  if (c_last < 0) {  // no active hop: the row comes out empty
    if (L > 0) put_cut(cuts, cuts_cap, row, 0, 0, L);
    finish(w, row, 0, 0, L > 0 ? 1 : 0, out_cap, cuts_cap, out_lens, n_cuts);
    return;
  }
  const int64_t j0 = c_last + 1, n = nh - j0;
  if (n > a) {  // the trailing run
    const int64_t at = (j0 + a) * HOP;
    put_cut(cuts, cuts_cap, row, c_cnt, at, L - at);
    put_seg(w, 1 + 2 * c_cnt, at - HOP - c_rem, at - HOP, 0, SEG_OUT);
    put_seg(w, 2 + 2 * c_cnt, at - c_rem, at, 0, SEG_COPY);  // (empty: the output ends here)
    c_rem += L - at;
    ++c_cnt;
  }
  finish(w, row, 1 + 2 * c_cnt, L - c_rem, c_cnt, out_cap, cuts_cap, out_lens, n_cuts);
}

// Chunked: the hop-level state machine over the bits of this call's virtual row, one lane per row.
struct Emit {
  const Ws* w;
  int64_t n_seg, n_out, n_cut;
  int64_t last_src, last_out;  // of the last segment when that is a copy, else last_src < 0
};
__device__ __forceinline__ void emit_copy(Emit& e, int64_t src, int64_t len) {
  if (len <= 0) return;
  if (!(e.last_src >= 0 && e.last_src + (e.n_out - e.last_out) == src)) {
    put_seg(*e.w, e.n_seg++, e.n_out, src, 0, SEG_COPY);
    e.last_src = src, e.last_out = e.n_out;
  }
  e.n_out += len;
}
__device__ __forceinline__ void emit_fade(Emit& e, int64_t src, int64_t src2, int kind) {
  put_seg(*e.w, e.n_seg++, e.n_out, src, src2, kind);
  e.last_src = -1;
  e.n_out += HOP;
}

__global__ __launch_bounds__(64) void sil_plan_seq_kernel(const int32_t* __restrict__ in_lens, int64_t in_cap, const float* __restrict__ thr,
                                                          const int32_t* __restrict__ cap_h, const int32_t* __restrict__ bs,
                                                          const int64_t* __restrict__ state, int flush, void* __restrict__ ws, int64_t vcap,
                                                          int64_t out_cap, int32_t* __restrict__ out_lens, int32_t* __restrict__ cuts,
                                                          int32_t cuts_cap, int32_t* __restrict__ n_cuts) {
  if (threadIdx.x != 0) return;
  const int row = blockIdx.x;
  const Row r = row_setup(row, nullptr, 0, in_lens, in_cap, thr, cap_h, bs, state);
  const Ws w = ws_of(ws, row, vcap);
  Emit e = {&w, 0, 0, 0, -1, 0};
  for (int k = 0; k < SIL_HDR; ++k) w.next[k] = 0;
  w.meta[M_NKEEP] = 0, w.meta[M_INC_SRC] = 0, w.meta[M_INC_LEN] = 0;
  const int64_t recv1 = r.recv0 + r.n_in;
  if (r.bad) {
    finish(w, row, 0, out_cap + 1, 0, out_cap, cuts_cap, out_lens, n_cuts);
    return;
  }
  if (r.ident) {
    emit_copy(e, 0, r.n_in);
    if (!flush) w.next[H_RECV] = recv1, w.next[H_EMIT] = r.emit0 + e.n_out;
    finish(w, row, e.n_seg, e.n_out, 0, out_cap, cuts_cap, out_lens, n_cuts);
    return;
  }
  const int b = r.b, a = r.a, cap = r.cap_h;
  const int64_t nfull = r.vlen / HOP;
  const int part = (int)(r.vlen - nfull * HOP);
  const int64_t nhv = nfull + ((flush && part > 0) ? 1 : 0);
  const int64_t src0 = r.recv0 / HOP - r.thops;  // source hop of virtual hop v (ring and new hops): src0 + v
  int64_t seen = r.seen, run = r.run;
  int64_t held = (seen && run >= a) ? 0 : -1;  // virtual hop of the held one
  for (int64_t v = r.thops; v < nhv; ++v) {
    const int len = v < nfull ? HOP : part;
    if ((w.words[v >> 6] >> (v & 63)) & 1) {
      const int64_t n = run;
      if (!seen) {
        if (n <= b + 1) {
          emit_copy(e, (v - n) * HOP, n * HOP);
        } else {
          emit_fade(e, (v - b - 1) * HOP, 0, SEG_IN);
          emit_copy(e, (v - b) * HOP, (int64_t)b * HOP);
          put_cut(cuts, cuts_cap, row, e.n_cut++, 0, (src0 + v - b - 1) * HOP);
        }
        seen = 1;
      } else if (n >= a) {
        if (n <= cap) {
          emit_copy(e, held * HOP, HOP);
          emit_copy(e, (v - (n - a)) * HOP, (n - a) * HOP);
        } else {
          emit_fade(e, held * HOP, (v - b - 1) * HOP, SEG_CROSS);
          emit_copy(e, (v - b) * HOP, (int64_t)b * HOP);
          put_cut(cuts, cuts_cap, row, e.n_cut++, (src0 + v - n + a) * HOP, (n - cap) * HOP);
        }
      }
      emit_copy(e, v * HOP, len);
      run = 0, held = -1;
    } else {
      const int64_t q = run++;
      if (seen && q < a - 1) emit_copy(e, v * HOP, len);
      else if (seen && q == a - 1) held = v;
    }
  }
  if (flush) {
    if (!seen) {
      if (recv1 > 0) put_cut(cuts, cuts_cap, row, e.n_cut++, 0, recv1);
    } else if (run == a) {
      emit_copy(e, held * HOP, held < nfull ? HOP : part);
    } else if (run > a) {
      emit_fade(e, held * HOP, 0, SEG_OUT);
      const int64_t at = (src0 + nhv - run + a) * HOP;
      put_cut(cuts, cuts_cap, row, e.n_cut++, at, recv1 - at);
    }
  } else {
    int nk = 0;
    if (seen && run >= a) w.meta[M_KEEP + nk++] = (int32_t)(held * HOP);
    const int64_t elig = seen ? (run > a ? run - a : 0) : run;
    const int rc = (int)(elig < b + 1 ? elig : b + 1);
    for (int k = 0; k < rc; ++k) w.meta[M_KEEP + nk++] = (int32_t)((nfull - rc + k) * HOP);
    w.meta[M_NKEEP] = nk, w.meta[M_INC_SRC] = (int32_t)(nfull * HOP), w.meta[M_INC_LEN] = part;
    w.next[H_SEEN] = seen, w.next[H_RUN] = run, w.next[H_RECV] = recv1, w.next[H_EMIT] = r.emit0 + e.n_out;
    w.next[H_THOPS] = nk, w.next[H_TLEN] = (int64_t)nk * HOP + part;
  }
  finish(w, row, e.n_seg, e.n_out, e.n_cut, out_cap, cuts_cap, out_lens, n_cuts);
}

// The definition rounds every operation on its own (see tsm.hip on why this is a pragma and not a set of intrinsics).
#pragma clang fp contract(off)

// ---- gather ----
__global__ __launch_bounds__(GATHER_BLOCK) void sil_gather_kernel(const float* __restrict__ in, int64_t in_stride, const int32_t* __restrict__ in_lens,
                                                                  int64_t in_cap, const float* __restrict__ thr, const int32_t* __restrict__ cap_h,
                                                                  const int32_t* __restrict__ bs, const int64_t* __restrict__ state,
                                                                  const float* __restrict__ tab, void* __restrict__ ws, int64_t vcap,
                                                                  float* __restrict__ out, int64_t out_stride) {
  const int row = blockIdx.y, tid = threadIdx.x;
  const Ws w = ws_of(ws, row, vcap);
  const int64_t out_len = w.meta[M_OUT];
  const int n_seg = w.meta[M_NSEG];
  const int64_t tile0 = (int64_t)blockIdx.x * SIL_TILE;
  if (tile0 >= out_len || n_seg <= 0) return;  // (out_len < 0: the row did not fit; nothing is written)
  const Row r = row_setup(row, in, in_stride, in_lens, in_cap, thr, cap_h, bs, state);
  float* y = out + (int64_t)row * out_stride;
  const int32_t* segs = w.segs;
  for (int q = 0; q < 2; ++q) {
    const int64_t o = tile0 + ((int64_t)q * GATHER_BLOCK + tid) * 4;
    if (o >= out_len) continue;
    int lo = 0, hi = n_seg - 1;  // the last segment that starts at or before o (segment 0 starts at 0)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (segs[4 * mid] <= o) lo = mid;
      else hi = mid - 1;
    }
    int s = lo;
    const int64_t next = s + 1 < n_seg ? segs[4 * (s + 1)] : out_len;
    const int64_t src = (int64_t)segs[4 * s + 1] + (o - segs[4 * s]);
    if (segs[4 * s + 3] == SEG_COPY && o + 3 < next && o + 3 < out_len && src >= r.tlen) {
      const float* p = r.in + (src - r.tlen);
      if (((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(y + o)) & 15u) == 0) {
        *reinterpret_cast<float4*>(y + o) = *reinterpret_cast<const float4*>(p);
        continue;
      }
    }
    for (int j = 0; j < 4; ++j) {
      const int64_t oe = o + j;
      if (oe >= out_len) break;
      while (s + 1 < n_seg && segs[4 * (s + 1)] <= oe) ++s;
      const int i = (int)(oe - segs[4 * s]);
      const int64_t s1 = (int64_t)segs[4 * s + 1] + i;
      const int kind = segs[4 * s + 3];
      float v = v_at(r, s1);
      if (kind == SEG_IN) {
        v = v * tab[i];
      } else if (kind == SEG_OUT) {
        v = v * tab[HOP - 1 - i];
      } else if (kind == SEG_CROSS) {
        const float u = v * tab[HOP - 1 - i];
        const float t2 = v_at(r, (int64_t)segs[4 * s + 2] + i) * tab[i];
        v = u + t2;
      }
      y[oe] = v;
    }
  }
}

// ---- state ----
__global__ __launch_bounds__(STATE_BLOCK) void sil_state_kernel(const float* __restrict__ in, int64_t in_stride, const int32_t* __restrict__ in_lens,
                                                                int64_t in_cap, const float* __restrict__ thr, const int32_t* __restrict__ cap_h,
                                                                const int32_t* __restrict__ bs, int64_t* __restrict__ state, int flush,
                                                                void* __restrict__ ws, int64_t vcap) {
  __shared__ float s_keep[SIL_TAIL];
  const int row = blockIdx.x, tid = threadIdx.x;
  const Ws w = ws_of(ws, row, vcap);
  int64_t* hdr = state + (int64_t)row * STATE_WORDS;
  float* tail = reinterpret_cast<float*>(hdr + SIL_HDR);
  if (flush || w.meta[M_OUT] < 0) {  // the row is over: a zeroed header is a fresh row (uniform over the workgroup)
    for (int k = tid; k < SIL_HDR; k += STATE_BLOCK) hdr[k] = 0;
    return;
  }
  const Row r = row_setup(row, in, in_stride, in_lens, in_cap, thr, cap_h, bs, state);  // (the old header, by value)
  int nk = w.meta[M_NKEEP];
  nk = nk < 0 ? 0 : (nk > KEEP_MAX ? KEEP_MAX : nk);
  int inc = w.meta[M_INC_LEN];
  inc = inc < 0 ? 0 : (inc > HOP - 1 ? HOP - 1 : inc);
  const int n = nk * HOP + inc;
  for (int k = tid; k < n; k += STATE_BLOCK) {
    const int h = k / HOP;
    const int64_t src = h < nk ? (int64_t)w.meta[M_KEEP + h] + (k - h * HOP) : (int64_t)w.meta[M_INC_SRC] + (k - nk * HOP);
    s_keep[k] = (src >= 0 && src < r.vlen) ? v_at(r, src) : 0.0f;
  }
  __syncthreads();  // the old tail has been read
  for (int k = tid; k < n; k += STATE_BLOCK) tail[k] = s_keep[k];
  for (int k = tid; k < SIL_HDR; k += STATE_BLOCK) hdr[k] = w.next[k];
}

}  // namespace

int64_t sopro_sil_state_bytes(int32_t rows) { return rows <= 0 ? 0 : (int64_t)rows * STATE_WORDS * (int64_t)sizeof(int64_t); }

int64_t sopro_sil_chunk_out_cap(int64_t in_cap) {
  if (in_cap < 0 || in_cap > LEN_MAX) return -1;
  return in_cap + SIL_TAIL;
}

int64_t sopro_sil_ws_bytes(int32_t rows, int64_t max_len) {
  if (rows <= 0 || max_len < 0 || max_len > LEN_MAX + SIL_TAIL) return -1;
  return (int64_t)rows * layout(max_len).stride * (int64_t)sizeof(int64_t);
}

int sopro_sil_rows_f32(const float* in, int64_t in_stride, const int32_t* in_lens, int64_t in_cap, const float* thr, const int32_t* cap_h,
                       const int32_t* b, int32_t rows, void* state, int32_t flush, const float* tab, void* workspace, float* out,
                       int64_t out_stride, int64_t out_cap, int32_t* out_lens, int32_t* cuts, int32_t cuts_cap, int32_t* n_cuts, void* stream) {
  SOPRO_CHECK_ARG(in_lens && thr && cap_h && b && tab && workspace && out_lens && n_cuts, "in_lens, thr, cap_h, b, tab, workspace, out_lens, n_cuts must be non-NULL");
  SOPRO_CHECK_ARG(rows > 0 && rows <= 65535, "0 < rows <= 65535");
  SOPRO_CHECK_ARG(in_cap >= 0 && in_cap <= LEN_MAX, "0 <= in_cap <= 2^30");
  SOPRO_CHECK_ARG(in || in_cap == 0, "in must be non-NULL when in_cap > 0");
  SOPRO_CHECK_ARG(in_stride >= 0 && out_stride >= 0, "strides >= 0");
  SOPRO_CHECK_ARG(out_cap >= 0 && out_cap <= INT32_MAX, "0 <= out_cap < 2^31");
  SOPRO_CHECK_ARG(out || out_cap == 0, "out must be non-NULL when out_cap > 0");
  SOPRO_CHECK_ARG(rows == 1 || out_cap == 0 || out_stride >= out_cap, "out_stride >= out_cap (rows must not overlap)");
  SOPRO_CHECK_ARG(cuts_cap >= 0 && (cuts || cuts_cap == 0), "cuts must be non-NULL when cuts_cap > 0");
  SOPRO_CHECK_ARG(state || flush, "a call without state is the whole row: flush must be set");
  SOPRO_CHECK_ARG(((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(cuts)) & 3u) == 0,
                  "in, out, cuts must be 4-byte aligned");
  SOPRO_CHECK_ARG(((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(workspace)) & 7u) == 0, "state, workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t vcap = state ? in_cap + SIL_TAIL : in_cap;
  const int64_t words = layout(vcap).wcap;
  const int64_t* st = static_cast<const int64_t*>(state);
  hipLaunchKernelGGL(sil_act_kernel, dim3((unsigned)((words + ACT_WAVES - 1) / ACT_WAVES), (unsigned)rows), dim3(ACT_BLOCK), 0, s, in, in_stride, in_lens,
                     in_cap, thr, cap_h, b, st, flush ? 1 : 0, workspace, vcap);
  if (state)
    hipLaunchKernelGGL(sil_plan_seq_kernel, dim3(rows), dim3(64), 0, s, in_lens, in_cap, thr, cap_h, b, st, flush ? 1 : 0, workspace, vcap, out_cap,
                       out_lens, cuts, cuts_cap, n_cuts);
  else
    hipLaunchKernelGGL(sil_plan_kernel, dim3(rows), dim3(PLAN_WORDS), 0, s, in_lens, in_cap, thr, cap_h, b, workspace, vcap, out_cap, out_lens, cuts,
                       cuts_cap, n_cuts);
  if (out_cap > 0)
    hipLaunchKernelGGL(sil_gather_kernel, dim3((unsigned)((out_cap + SIL_TILE - 1) / SIL_TILE), (unsigned)rows), dim3(GATHER_BLOCK), 0, s, in, in_stride,
                       in_lens, in_cap, thr, cap_h, b, st, tab, workspace, vcap, out, out_stride);
  if (state)
    hipLaunchKernelGGL(sil_state_kernel, dim3(rows), dim3(STATE_BLOCK), 0, s, in, in_stride, in_lens, in_cap, thr, cap_h, b, static_cast<int64_t*>(state),
                       flush ? 1 : 0, workspace, vcap);
  SOPRO_LAUNCH_CHECK();
}
