// vsyn_beat.h — rhythm section D: the beat tracker on envelopes already on the device. Semantics: include/vorbis_synth_hip.h,
// "rhythm", D; model: tests/beat_model.py.
//
// Four kernels, one workgroup per segment wherever a step is sequential; the batch is the parallelism there:
//   vsyn_beat_norm_kernel   one workgroup per segment: the two sums of D.1 in their documented order (256 lane-strided partials, then
//                           wave_sum and the waves ascending: DESIGN.md 6t), whether a value is not finite, whether
//                           one is not zero. Leaves sd + FLT_MIN and the segment's flags; a segment without a score (refused, F < 2,
//                           all zero) gets its count and refusal word here and is skipped by the kernels behind.
//   vsyn_beat_score_kernel  grid (tile of 256 frames, segment), a thread per frame: the window (2P + 1 doubles) and the tile's u with
//                           P frames on either side sit in LDS; ls[i] is ONE fma chain with k ascending, w[k] a broadcast and u[i - k]
//                           consecutive doubles across the lanes. A frame outside the segment is a 0.0 in the tile: fma(w, 0, acc)
//                           is acc, bit for bit, so the chain is the one over the k with 0 <= i - k < F. The tile's largest ls goes
//                           to the workspace as an order key (an integer maximum: no order can show).
//   vsyn_beat_dp_kernel     one workgroup per segment, the hot path. thr and i0 from the tiles' keys and an integer minimum. Then the
//                           dynamic programme: cum[i] reads cum[loc] with loc <= i - lo only, so the B = lo frames i .. i + B - 1 are
//                           independent of each other and the workgroup advances B frames a barrier, ceil(F / B) barriers in all.
//                           A wave takes a frame; its lanes stride over the frame's candidates d = lo .. min(2P, i) and keep the
//                           largest s = cum[i - d] + tx[d] with the smallest d among equals, across the lanes by xor rounds with the
//                           same rule (an arg-max with a total order on (s, d): no order of evaluation can show). cum lives in an LDS
//                           ring of R >= 2P + B doubles (a power of two): a step reads ring indices i_b - 2P .. i_b - 1 and writes
//                           i_b .. i_b + B - 1, which alias nothing closer than i_b + B - 1 - R < i_b - 2P. tx sits beside it. cum and
//                           back stream out as they are finished.
//   vsyn_beat_tail_kernel   one workgroup per segment: the local maxima are counted, their median selected exactly (order keys,
//                           eight passes of an 8-bit histogram in LDS per rank: integer counts, order-independent), the tail by an
//                           integer maximum, one short walk along back (the only ordered step, as vsyn_peaks_walk_kernel's is), the
//                           trim over the at most ceil(F / lo) beats, and the kept beats in ascending order.
// No floating-point atomics; nothing depends on the launch geometry or on the segment's place in the batch. Nothing here reads or
// writes stream state, the overlap carry or any synthesis buffer.
#pragma once
#include "vsyn_rhythm.h"
#include "vsyn_wave.h"

#define BEAT_THREADS 256
#define BEAT_WAVES (BEAT_THREADS / 64)
#define BEAT_DP_THREADS 512
#define BEAT_DP_WAVES (BEAT_DP_THREADS / 64)
#define BEAT_MAX_P 2048u
#define BEAT_SCORED 2u  // BeatStat.flags: the segment has a score (finite, F >= 2, not all zero)
#define BEAT_BAD 1u     // ... holds a value that is not finite

struct BeatSeg {
  uint64_t off;     // first value of the segment's envelope, and of its ls, cum, back and beats
  uint64_t mx_off;  // first tile maximum
  uint32_t F, P;    // P = 0: skipped (nothing is written)
  uint32_t lo, ring;      // lo = max(rint(P / 2), 1); ring: a power of two >= 2P + lo
  uint32_t tab_off, tiles;  // its tables (w[2P + 1], tx[2P + 1]) in doubles from the tables' start; tiles of BEAT_THREADS frames
  uint32_t word, pad;       // a refusal word known on the host (3: the period), count 0 with it
};

struct BeatStat {
  double den;  // sd + FLT_MIN
  uint32_t flags, pad;
};

struct BeatCtx {  // launch arguments
  const BeatSeg* seg;
  const double* tab;
  const float* env;
  BeatStat* stat;   // [S]
  uint64_t* tmax;   // the tiles' largest ls, as order keys
  double* ls;       // workspace, or the caller's
  double* cum;
  int32_t* back;
  uint32_t* chain;  // the walk's frames, descending
  double* sq;       // the trim's squares
  uint32_t* beats;
  uint32_t* counts;   // [S]
  uint32_t* refused;  // [S] or NULL
  uint32_t trim;
};

// order key of a finite double: a larger value has a larger key
__device__ __forceinline__ uint64_t beat_key(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double beat_unkey(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? k & 0x7FFFFFFFFFFFFFFFull : ~k));
}

// ------------------------------------------------------------------------------------------------
// D.1: the sums, the flags
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BEAT_THREADS) vsyn_beat_norm_kernel(const BeatCtx A) {
  __shared__ double s_part[BEAT_WAVES];
  const uint32_t g = blockIdx.x, tid = threadIdx.x;
  const BeatSeg sg = A.seg[g];
  if (!sg.P && !sg.word) return;  // (workgroup-uniform) skipped
  if (sg.word) {                  // refused on the host
    if (tid == 0u) {
      A.stat[g] = BeatStat{0.0, 0u, 0u};
      A.counts[g] = 0u;
      if (A.refused) A.refused[g] = sg.word;
    }
    return;
  }
  const float* x = A.env + sg.off;
  const uint32_t F = sg.F;
  double part = 0.0;
  bool bad = false, nz = false;
  for (uint32_t n = tid; n < F; n += BEAT_THREADS) {
    const float v = x[n];
    bad |= (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u;
    nz |= v != 0.f;
    part += (double)v;
  }
  wg_put(part, s_part, WaveSum());  // (the barrier is the flags' __syncthreads_or: the two halves of wg_reduce_all apart)
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  double sum = wg_get<BEAT_WAVES>(s_part, WaveSum(), 0.0);
  const double m = sum / (double)F;
  const int any_nz = __syncthreads_or(nz ? 1 : 0);  // (and s_part is free)
  part = 0.0;
  for (uint32_t n = tid; n < F; n += BEAT_THREADS) {
    const double d = (double)x[n] - m;
    const double q = d * d;  // (rounded before it is added: the build contracts nothing)
    part += q;
  }
  sum = wg_reduce_t0<BEAT_WAVES>(part, s_part, WaveSum(), 0.0);
  if (tid == 0u) {
    const bool scored = !any_bad && any_nz && F >= 2u;
    const double sd = scored ? sqrt(sum / (double)(F - 1u)) : 0.0;
    A.stat[g] = BeatStat{sd + (double)RHY_FLT_MIN, (any_bad ? BEAT_BAD : 0u) | (scored ? BEAT_SCORED : 0u), 0u};
    if (!scored) A.counts[g] = 0u;
    if (A.refused) A.refused[g] = any_bad ? 1u : 0u;
  }
}

// ------------------------------------------------------------------------------------------------
// D.2: the local score and the tiles' maxima
// ------------------------------------------------------------------------------------------------
static inline uint32_t beat_score_lds(uint32_t P) { return 8u * ((2u * P + 2u) + (BEAT_THREADS + 2u * P) + BEAT_WAVES); }

__global__ void __launch_bounds__(BEAT_THREADS) vsyn_beat_score_kernel(const BeatCtx A) {
  extern __shared__ __attribute__((aligned(16))) double s_beat[];
  const uint32_t g = blockIdx.y, tid = threadIdx.x;
  const BeatSeg sg = A.seg[g];
  if (!sg.P || blockIdx.x >= sg.tiles) return;  // (workgroup-uniform)
  const BeatStat st = A.stat[g];
  if (!(st.flags & BEAT_SCORED)) return;
  const uint32_t P = sg.P, F = sg.F, nw = 2u * P + 1u, f0 = blockIdx.x * BEAT_THREADS;
  double* s_w = s_beat;                          // [2P + 1] (+ 1: the next carve stays 16-byte aligned)
  double* s_u = s_beat + (2u * P + 2u);          // [BEAT_THREADS + 2P]: frames f0 - P .. f0 + BEAT_THREADS + P - 1
  uint64_t* s_r = (uint64_t*)(s_u + BEAT_THREADS + 2u * P);  // [BEAT_WAVES]
  const float* x = A.env + sg.off;
  const double* w = A.tab + sg.tab_off;
  for (uint32_t k = tid; k < nw; k += BEAT_THREADS) s_w[k] = w[k];
  for (uint32_t j = tid; j < BEAT_THREADS + 2u * P; j += BEAT_THREADS) {
    const int64_t n = (int64_t)f0 + (int64_t)j - (int64_t)P;
    s_u[j] = n >= 0 && n < (int64_t)F ? (double)x[n] / st.den : 0.0;
  }
  __syncthreads();
  const uint32_t i = f0 + tid;
  uint64_t key = 0ull;
  if (i < F) {
    double acc = 0.0;
    const double* u = s_u + tid + 2u * P;  // u[i - k] for k = kk - P is u[-kk]
    for (uint32_t kk = 0; kk < nw; ++kk) acc = fma(s_w[kk], u[-(int32_t)kk], acc);
    A.ls[sg.off + i] = acc;
    key = beat_key(acc);
  }
  key = wg_reduce_t0<BEAT_WAVES>(key, s_r, WaveMax(), 0ull);
  if (tid == 0u) A.tmax[sg.mx_off + blockIdx.x] = key;
}

// ------------------------------------------------------------------------------------------------
// D.3: the dynamic programme
// ------------------------------------------------------------------------------------------------
static inline uint32_t beat_ring(uint32_t P, uint32_t lo) {
  uint32_t r = 1u;
  while (r < 2u * P + lo) r <<= 1;
  return r;
}
static inline uint32_t beat_dp_lds(uint32_t P, uint32_t ring) { return 8u * (ring + (2u * P + 2u) + 2u * BEAT_DP_WAVES); }

__global__ void __launch_bounds__(BEAT_DP_THREADS) vsyn_beat_dp_kernel(const BeatCtx A) {
  extern __shared__ __attribute__((aligned(16))) double s_beat[];
  const uint32_t g = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const BeatSeg sg = A.seg[g];
  if (!sg.P) return;  // (workgroup-uniform)
  if (!(A.stat[g].flags & BEAT_SCORED)) return;
  const uint32_t P = sg.P, F = sg.F, lo = sg.lo, mask = sg.ring - 1u;
  double* s_ring = s_beat;                               // [ring]
  double* s_tx = s_beat + sg.ring;                       // [2P + 1], by d (+ 1)
  uint64_t* s_r = (uint64_t*)(s_tx + (2u * P + 2u));     // [BEAT_DP_WAVES]
  uint32_t* s_r32 = (uint32_t*)(s_r + BEAT_DP_WAVES);    // [BEAT_DP_WAVES]
  const double* ls = A.ls + sg.off;
  double* cum = A.cum + sg.off;
  int32_t* back = A.back + sg.off;
  const double* tx = A.tab + sg.tab_off + (2u * P + 1u);
  for (uint32_t d = tid; d <= 2u * P; d += BEAT_DP_THREADS) s_tx[d] = tx[d];
  // thr = 0.01 max ls, from the tiles' keys
  uint64_t key = 0ull;
  for (uint32_t t = tid; t < sg.tiles; t += BEAT_DP_THREADS) {
    const uint64_t k = A.tmax[sg.mx_off + t];
    key = k > key ? k : key;
  }
  wg_put(key, s_r, WaveMax());  // (one barrier: s_r is not written again)
  __syncthreads();
  key = wg_get<BEAT_DP_WAVES>(s_r, WaveMax(), 0ull);
  const double thr = 0.01 * beat_unkey(key);
  // i0: the first frame that reaches thr (the maximum does)
  uint32_t first = 0xFFFFFFFFu;
  for (uint32_t i = tid; i < F && first == 0xFFFFFFFFu; i += BEAT_DP_THREADS)
    if (ls[i] >= thr) first = i;
  const uint32_t i0 = wg_reduce_all<BEAT_DP_WAVES>(first, s_r32, WaveMin(), 0xFFFFFFFFu);  // (behind its barriers s_tx is written too)
  const double ninf = -__longlong_as_double(0x7FF0000000000000ll);
  for (uint32_t base = 0; base < F; base += lo) {
    const uint32_t nf = min(lo, F - base);
    for (uint32_t q = wave; q < nf; q += BEAT_DP_WAVES) {  // (wave-uniform)
      const uint32_t i = base + q, hi = min(2u * P, i);
      const double l = ls[i];
      double best_s = ninf;
      uint32_t best_d = 0xFFFFFFFFu;
      for (uint32_t d = lo + lane; d <= hi; d += 64u) {  // d ascending in a lane: > keeps the smaller d among equals
        const double s = s_ring[(i - d) & mask] + s_tx[d];
        if (s > best_s) {
          best_s = s;
          best_d = d;
        }
      }
      for (int o = 32; o >= 1; o >>= 1) {  // (an arg-max on the pair (s, d): the butterfly of wave_reduce with a rule of its own)
        const double os = wave_xor(best_s, o);
        const uint32_t od = wave_xor(best_d, o);
        if (os > best_s || (os == best_s && od < best_d)) {
          best_s = os;
          best_d = od;
        }
      }
      if (lane == 0u) {
        const bool has = best_d != 0xFFFFFFFFu;
        const double c = has ? l + best_s : l;
        s_ring[i & mask] = c;
        cum[i] = c;
        back[i] = has && i >= i0 ? (int32_t)(i - best_d) : -1;
      }
    }
    __syncthreads();  // the step's cum is in the ring
  }
}

// ------------------------------------------------------------------------------------------------
// D.4, D.5: the last beat, the walk, the trim
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool beat_is_max(const double* cum, uint32_t F, uint32_t i) {
  const double c = cum[i];
  return c > cum[i ? i - 1u : 0u] && c >= cum[i + 1u < F ? i + 1u : F - 1u];
}

// the key of rank `rank` (0: the smallest) among the local maxima's: eight passes, most significant byte first
__device__ uint64_t beat_select(const double* cum, uint32_t F, uint32_t rank, uint32_t* s_hist, uint32_t* s_pick) {
  uint64_t prefix = 0ull;
  for (int shift = 56; shift >= 0; shift -= 8) {
    const uint64_t himask = shift == 56 ? 0ull : ~0ull << (shift + 8);
    __syncthreads();  // (the histogram and the pick are free)
    for (uint32_t b = threadIdx.x; b < 256u; b += BEAT_THREADS) s_hist[b] = 0u;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < F; i += BEAT_THREADS) {
      if (!beat_is_max(cum, F, i)) continue;
      const uint64_t k = beat_key(cum[i]);
      if ((k & himask) == prefix) atomicAdd(&s_hist[(uint32_t)(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
      uint32_t b = 0u, r = rank;
      while (b < 255u && r >= s_hist[b]) r -= s_hist[b++];
      s_pick[0] = b;
      s_pick[1] = r;
    }
    __syncthreads();
    prefix |= (uint64_t)s_pick[0] << shift;
    rank = s_pick[1];
  }
  return prefix;
}

__global__ void __launch_bounds__(BEAT_THREADS) vsyn_beat_tail_kernel(const BeatCtx A) {
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_pick[2];
  __shared__ uint32_t s_r32[BEAT_WAVES];
  __shared__ uint32_t s_B;
  __shared__ double s_t;
  const uint32_t g = blockIdx.x, tid = threadIdx.x;
  const BeatSeg sg = A.seg[g];
  if (!sg.P) return;  // (workgroup-uniform)
  if (!(A.stat[g].flags & BEAT_SCORED)) return;
  const uint32_t F = sg.F;
  const double* ls = A.ls + sg.off;
  const double* cum = A.cum + sg.off;
  const int32_t* back = A.back + sg.off;
  uint32_t* chain = A.chain + sg.off;
  double* sq = A.sq + sg.off;
  uint32_t n = 0u;
  for (uint32_t i = tid; i < F; i += BEAT_THREADS) n += beat_is_max(cum, F, i) ? 1u : 0u;
  const uint32_t M = wg_reduce_all<BEAT_WAVES>(n, s_r32, WaveSum(), 0u);
  if (M == 0u) {  // (workgroup-uniform) no local maximum: no beats
    if (tid == 0u) A.counts[g] = 0u;
    return;
  }
  const double lo_v = beat_unkey(beat_select(cum, F, (M - 1u) / 2u, s_hist, s_pick));
  const double med = (M & 1u) ? lo_v : (lo_v + beat_unkey(beat_select(cum, F, M / 2u, s_hist, s_pick))) / 2.0;
  const double need = 0.5 * med;
  uint32_t last = 0u;  // (frame + 1 of the last local maximum that reaches 0.5 med)
  for (uint32_t i = tid; i < F; i += BEAT_THREADS)
    if (beat_is_max(cum, F, i) && cum[i] >= need) last = i + 1u;
  last = wg_reduce_all<BEAT_WAVES>(last, s_r32, WaveMax(), 0u);
  const uint32_t tail = last ? last - 1u : F - 1u;
  if (tid == 0u) {  // the walk: back[b] < b, at most ceil(F / lo) frames
    uint32_t B = 0u;
    for (int32_t b = (int32_t)tail; b >= 0 && B < F; b = back[b]) chain[B++] = (uint32_t)b;
    s_B = B;
  }
  __syncthreads();
  const uint32_t B = s_B;  // beat j is chain[B - 1 - j]
  double t = 0.0;
  if (A.trim) {
    for (uint32_t j = tid; j < B; j += BEAT_THREADS) {
      const double v = ls[chain[B - 1u - j]];
      const double a = j ? 0.5 * ls[chain[B - j]] : 0.0;
      const double c = j + 1u < B ? 0.5 * ls[chain[B - 2u - j]] : 0.0;
      const double sm = (a + v) + c;
      sq[j] = sm * sm;
    }
    __syncthreads();
    if (tid == 0u) {
      double acc = 0.0;
      for (uint32_t j = 0; j < B; ++j) acc += sq[j];
      s_t = 0.5 * sqrt(acc / (double)B);
    }
    __syncthreads();
    t = s_t;
  }
  uint32_t n0 = 0xFFFFFFFFu, n1 = 0u;  // (n1: frame + 1)
  for (uint32_t i = tid; i < F; i += BEAT_THREADS)
    if (ls[i] > t) {
      n0 = min(n0, i);
      n1 = i + 1u;
    }
  n0 = wg_reduce_all<BEAT_WAVES>(n0, s_r32, WaveMin(), 0xFFFFFFFFu);
  n1 = wg_reduce_all<BEAT_WAVES>(n1, s_r32, WaveMax(), 0u);
  if (n1 == 0u) {  // (workgroup-uniform) no frame above t: none is kept
    if (tid == 0u) A.counts[g] = 0u;
    return;
  }
  uint32_t below = 0u, kept = 0u;
  for (uint32_t j = tid; j < B; j += BEAT_THREADS) {
    const uint32_t b = chain[B - 1u - j];
    below += b < n0 ? 1u : 0u;
    kept += b >= n0 && b < n1 ? 1u : 0u;
  }
  below = wg_reduce_all<BEAT_WAVES>(below, s_r32, WaveSum(), 0u);
  kept = wg_reduce_all<BEAT_WAVES>(kept, s_r32, WaveSum(), 0u);
  uint32_t* out = A.beats + sg.off;
  for (uint32_t j = tid; j < kept; j += BEAT_THREADS) out[j] = chain[B - 1u - (below + j)];  // (ascending: the kept ones are consecutive)
  if (tid == 0u) A.counts[g] = kept;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct BeatWs {  // the stage's buffers
  TableUpload tab;
  bool lds_set = false;  // the score and DP kernels' dynamic-LDS limits are raised on this handle's device
  DevBuf<BeatStat> stat;
  DevBuf<uint64_t> tmax;
  DevBuf<double> ls, cum, sq;
  DevBuf<int32_t> back;
  DevBuf<uint32_t> chain;
  // host form: the beats on their way to the host
  DevBuf<uint32_t> beats, counts, refused;
};

static inline int beat_check(const vsyn_beat_spec* p, const char** err) {
  if (!p) return fail(err, VSYN_ERR_INVALID, "beat spec is NULL");
  if (p->options & ~(uint32_t)VSYN_BEAT_TRIM) return fail(err, VSYN_ERR_INVALID, "unknown beat options 0x%x", p->options);
  if (!std::isfinite(p->tightness) || !(p->tightness > 0.0)) return fail(err, VSYN_ERR_INVALID, "beat: tightness must be finite and > 0");
  if (!std::isfinite(p->start_bpm) || !(p->start_bpm > 0.0)) return fail(err, VSYN_ERR_INVALID, "beat: start_bpm must be finite and > 0");
  if (!std::isfinite(p->bpm) || p->bpm < 0.0) return fail(err, VSYN_ERR_INVALID, "beat: bpm must be finite and > 0 (0: estimated per segment)");
  if (p->hop_length < 1) return fail(err, VSYN_ERR_INVALID, "beat hop_length must be >= 1");
  return VSYN_OK;
}

// D.0; 0: outside [1, BEAT_MAX_P]
static inline uint32_t beat_period(const vsyn_beat_spec* p, double bpm, uint32_t rate) {
  const double v = rint(60.0 * ((double)rate / (double)p->hop_length) / bpm);
  return v >= 1.0 && v <= (double)BEAT_MAX_P ? (uint32_t)v : 0u;
}

static inline int beat_check_call(const vsyn_beat_spec* p, uint32_t S, const uint64_t* seg_rows, const uint32_t* periods, const char** err) {
  if (int rc = beat_check(p, err)) return rc;
  if (int rc = rhythm_check_segs(S, seg_rows, err)) return rc;
  if (S && !periods) return fail(err, VSYN_ERR_INVALID, "periods is NULL");
  return VSYN_OK;
}

// Steps D.1 to D.5 on stream s; d_ls, d_cum and d_back may be NULL (the workspace's are used). Caller holds the handle's lock and has
// run beat_check_call.
static inline int beat_launch(BeatWs& ws, int device, const vsyn_beat_spec* p, uint32_t S, const uint64_t* seg_rows, const uint32_t* periods,
                              const float* d_env, uint32_t* d_beats, uint32_t* d_counts, uint32_t* d_refused, double* d_ls, double* d_cum,
                              int32_t* d_back, hipStream_t s, const char** err) {
  if (S == 0) return VSYN_OK;
  const size_t seg_bytes = sizeof(BeatSeg) * (size_t)S;
  std::vector<uint8_t> tab(seg_bytes);
  std::vector<std::pair<uint32_t, uint32_t>> tabs;  // (P, offset in doubles)
  uint32_t tab_doubles = 0, tiles_max = 0, lds_score = 0, lds_dp = 0;
  uint64_t off = 0, mx_off = 0;
  bool any = false;
  for (uint32_t g = 0; g < S; ++g) {
    BeatSeg sg;
    memset(&sg, 0, sizeof(sg));
    sg.off = off;
    sg.mx_off = mx_off;
    off += seg_rows[g];
    if (periods[g] > BEAT_MAX_P) {
      sg.word = 3u;
      any = true;
    } else if (periods[g]) {
      sg.P = periods[g];
      sg.F = (uint32_t)seg_rows[g];
      const uint32_t h = (uint32_t)rint((double)sg.P / 2.0);
      sg.lo = std::max(h, 1u);
      sg.ring = beat_ring(sg.P, sg.lo);
      sg.tiles = (sg.F + BEAT_THREADS - 1u) / BEAT_THREADS;
      sg.tab_off = table_slot(tabs, sg.P, &tab_doubles, 2u * (2u * sg.P + 1u));
      mx_off += sg.tiles;
      tiles_max = std::max(tiles_max, sg.tiles);
      lds_score = std::max(lds_score, beat_score_lds(sg.P));
      lds_dp = std::max(lds_dp, beat_dp_lds(sg.P, sg.ring));
      any = true;
    }
    memcpy(tab.data() + sizeof(BeatSeg) * (size_t)g, &sg, sizeof(sg));
  }
  if (!any) return VSYN_OK;  // every segment is skipped
  tab.resize(seg_bytes + sizeof(double) * (size_t)tab_doubles);
  double* tv = (double*)(tab.data() + seg_bytes);
  for (const auto& pk : tabs) {
    const uint32_t P = pk.first, lo = std::max((uint32_t)rint((double)P / 2.0), 1u);
    double* w = tv + pk.second;
    double* tx = w + (2u * P + 1u);
    for (uint32_t kk = 0; kk <= 2u * P; ++kk) {
      const double z = 32.0 * ((double)kk - (double)P) / (double)P;
      w[kk] = exp(-0.5 * (z * z));
    }
    const double lp = log((double)P);
    for (uint32_t d = 0; d <= 2u * P; ++d) {
      const double q = log((double)std::max(d, lo)) - lp;  // (entries below lo are not read)
      tx[d] = -p->tightness * (q * q);
    }
  }
  HIPCHK(hipSetDevice(device));
  if (int rc = raise_lds_once(ws.lds_set,
                              {{(const void*)vsyn_beat_score_kernel, beat_score_lds(BEAT_MAX_P)},
                               {(const void*)vsyn_beat_dp_kernel, beat_dp_lds(BEAT_MAX_P, beat_ring(BEAT_MAX_P, BEAT_MAX_P / 2u))}},
                              err))
    return rc;
  HIPCHK(ws.stat.ensure(S));
  HIPCHK(ws.tmax.ensure(mx_off + 1u));
  HIPCHK(ws.chain.ensure(off + 1u));
  HIPCHK(ws.sq.ensure(off + 1u));
  if (!d_ls) HIPCHK(ws.ls.ensure(off + 1u));
  if (!d_cum) HIPCHK(ws.cum.ensure(off + 1u));
  if (!d_back) HIPCHK(ws.back.ensure(off + 1u));
  if (int rc = ws.tab.upload(tab, s, err)) return rc;
  BeatCtx A;
  A.seg = (const BeatSeg*)ws.tab.dev.p;
  A.tab = (const double*)(ws.tab.dev.p + seg_bytes);
  A.env = d_env;
  A.stat = ws.stat.p;
  A.tmax = ws.tmax.p;
  A.ls = d_ls ? d_ls : ws.ls.p;
  A.cum = d_cum ? d_cum : ws.cum.p;
  A.back = d_back ? d_back : ws.back.p;
  A.chain = ws.chain.p;
  A.sq = ws.sq.p;
  A.beats = d_beats;
  A.counts = d_counts;
  A.refused = d_refused;
  A.trim = (p->options & VSYN_BEAT_TRIM) ? 1u : 0u;
  VSYN_LAUNCH(vsyn_beat_norm_kernel, dim3(S), dim3(BEAT_THREADS), 0, s, A);
  if (tiles_max) {
    VSYN_LAUNCH(vsyn_beat_score_kernel, dim3(tiles_max, S), dim3(BEAT_THREADS), lds_score, s, A);
    VSYN_LAUNCH(vsyn_beat_dp_kernel, dim3(S), dim3(BEAT_DP_THREADS), lds_dp, s, A);
    VSYN_LAUNCH(vsyn_beat_tail_kernel, dim3(S), dim3(BEAT_THREADS), 0, s, A);
  }
  return VSYN_OK;
}

// ------------------------------------------------------------------------------------------------
// the beat tracker behind the rows of a host chain (vsyn_pcm_chain_beats_host)
// ------------------------------------------------------------------------------------------------
// The checks that need no rows: the two specs and their agreement with the spectral spec.
static inline int beat_chain_check(const vsyn_onset_spec* onset, const vsyn_beat_spec* B, uint32_t n_fft, uint32_t hop, bool center, uint32_t D,
                                   const char** err) {
  if (int rc = onset_check(onset, err)) return rc;
  if (int rc = beat_check(B, err)) return rc;
  if (onset->n_fft != n_fft || onset->hop_length != hop || ((onset->options & VSYN_ONSET_CENTER) != 0) != center)
    return fail(err, VSYN_ERR_INVALID, "beats: the onset spec's n_fft, hop_length and centring must be the spectral spec's");
  if (B->hop_length != hop) return fail(err, VSYN_ERR_INVALID, "beats: the beat spec's hop_length must be the spectral spec's");
  if (D < 1 || D > ONS_MAX_DIM) return fail(err, VSYN_ERR_INVALID, "onset strength takes rows of 1 to %u columns, this kind has %u", ONS_MAX_DIM, D);
  return VSYN_OK;
}

// The envelope, the tempo (with B->bpm == 0: the tempogram mean for ac_size 8 s, its copy to the host, tempo_from_mean), P per segment
// and the beat stage on stream s over the rows at cur ([total][D], seg_rows[S] rows a segment, rates[S] the rows' rates with 0 for a
// skipped segment); the beat frames into the host's words (cap of them), seg_rows rewritten as their counts, bpm_out, rate_out and
// refused_out (each may be NULL) as the header says. Waits for the stream. Caller holds the handle's lock and has run beat_chain_check.
static inline int beat_rows_out(RhythmWs& rw, BeatWs& ws, int device, const vsyn_onset_spec* onset, const vsyn_beat_spec* B, uint32_t D, uint32_t S,
                                const uint32_t* rates, uint64_t* seg_rows, uint64_t total, const float* cur, float* words, uint64_t cap,
                                double* bpm_out, uint32_t* rate_out, uint32_t* refused_out, hipStream_t s, const char** err) {
  const std::vector<uint64_t> F(seg_rows, seg_rows + S);
  std::vector<uint32_t> refused(S, 0u), periods(S, 0u);
  std::vector<double> bpm(S, B->bpm);
  if (int rc = rhythm_check_segs(S, F.data(), err)) return rc;
  if (total > cap) return fail(err, VSYN_ERR_INVALID, "rows buffer too small: %llu words needed", (unsigned long long)total);
  HIPCHK(hipSetDevice(device));
  HIPCHK(rw.env.ensure(total + 1));
  if (int rc = onset_launch(rw, device, onset, D, S, F.data(), cur, rw.env.p, s, err)) return rc;
  if (B->bpm == 0.0) {  // librosa.beat.beat_track's own tempo: feature.tempo with ac_size 8 s, std_bpm 1, max_tempo 320
    const vsyn_tempogram_spec tg = {0u, B->hop_length, VSYN_TG_CENTER | VSYN_TG_NORM_INF, 0u, 8.0};
    const vsyn_tempo_spec ts = {B->start_bpm, 1.0, 320.0};
    std::vector<uint32_t> r(rates, rates + S), W(S, 0u);
    std::vector<uint64_t> Fr(F);
    uint64_t nm = 0;
    for (uint32_t g = 0; g < S; ++g) {
      if (!F[g]) r[g] = 0u;  // nothing to average
      W[g] = r[g] ? tg_win_length(&tg, r[g]) : 0u;
      if (r[g] && !W[g]) {
        refused[g] = 2u;
        r[g] = 0u;
      }
      if (!r[g]) Fr[g] = 0;
      nm += W[g];
    }
    HIPCHK(rw.mean.ensure(nm + 1));
    if (int rc = tg_launch(rw, device, &tg, S, Fr.data(), r.data(), rw.env.p, nullptr, rw.mean.p, s, err)) return rc;
    std::vector<double> m(nm);
    if (nm) HIPCHK(hipMemcpyAsync(m.data(), rw.mean.p, sizeof(double) * nm, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    uint64_t o = 0;
    for (uint32_t g = 0; g < S; ++g) {
      if (!W[g]) continue;
      if (tempo_from_mean(&ts, m.data() + o, W[g], r[g], B->hop_length, &bpm[g], nullptr, nullptr) != VSYN_OK) refused[g] = 1u;  // a mean that is not finite
      o += W[g];
    }
  }
  for (uint32_t g = 0; g < S; ++g) {
    if (!rates[g] || !F[g] || refused[g]) continue;
    periods[g] = beat_period(B, bpm[g], rates[g]);
    if (!periods[g]) refused[g] = 3u;
  }
  HIPCHK(ws.beats.ensure(total + 1));
  HIPCHK(ws.counts.ensure(S));
  HIPCHK(ws.refused.ensure(S));
  HIPCHK(hipMemsetAsync(ws.counts.p, 0, sizeof(uint32_t) * S, s));  // (a skipped segment's count is not written)
  HIPCHK(hipMemsetAsync(ws.refused.p, 0, sizeof(uint32_t) * S, s));
  HIPCHK(ws.stat.ensure(S));
  HIPCHK(hipMemsetAsync(ws.stat.p, 0, sizeof(BeatStat) * S, s));
  if (int rc = beat_launch(ws, device, B, S, F.data(), periods.data(), rw.env.p, ws.beats.p, ws.counts.p, ws.refused.p, nullptr, nullptr, nullptr, s, err))
    return rc;
  std::vector<uint32_t> all(total), counts(S), dev_refused(S);
  std::vector<BeatStat> stat(S);
  if (total) HIPCHK(hipMemcpyAsync(all.data(), ws.beats.p, sizeof(uint32_t) * total, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(counts.data(), ws.counts.p, sizeof(uint32_t) * S, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(dev_refused.data(), ws.refused.p, sizeof(uint32_t) * S, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(stat.data(), ws.stat.p, sizeof(BeatStat) * S, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  uint64_t off = 0, o = 0;
  for (uint32_t g = 0; g < S; ++g) {  // (a count never exceeds the segment's frames)
    if (!refused[g] && dev_refused[g]) refused[g] = dev_refused[g];
    const uint32_t n = refused[g] ? 0u : counts[g];
    memcpy(words + o, all.data() + off, sizeof(uint32_t) * n);
    off += F[g];
    o += n;
    seg_rows[g] = n;
    if (bpm_out) bpm_out[g] = !refused[g] && periods[g] && (stat[g].flags & BEAT_SCORED) ? bpm[g] : 0.0;
    if (rate_out) rate_out[g] = rates[g];
    if (refused_out) refused_out[g] = refused[g];
  }
  return VSYN_OK;
}
