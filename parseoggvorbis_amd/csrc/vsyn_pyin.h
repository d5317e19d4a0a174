// vsyn_pyin.h — pyin: per frame a Viterbi-decoded fundamental frequency, a voiced flag and a voicing probability (pYIN), from planar
// float32 PCM already on the device (librosa.pyin on the mono signal). Semantics: include/vorbis_synth_hip.h, "pyin".
//
// Four kernels on one stream (the per-segment periods, the thresholds, the bin frequencies and the log transition tables are built
// on the host in double):
//   1. vsyn_pyin_offsets_kernel  one workgroup: frames per segment and the exclusive row scan, as the pitch stage's (frames_offsets).
//   2. vsyn_pyin_obs_kernel      grid (tile of FT frames, segment), 256 threads. The frames are staged and d and c computed by the
//                                device functions of vsyn_yin.h, exactly as vsyn_pitch_kernel does. The staged span is dead once d
//                                stands, and its LDS is used again for the lists below. Then per frame, by the whole workgroup:
//                                  a. the troughs in ascending lag: thread t owns the lags t Kc .. (t + 1) Kc - 1, counts its troughs,
//                                     an integer scan of the counts (wave_scan, the waves' totals in ascending order) places them.
//                                  b. thread m (and m + 256, ..) owns threshold t_m: it counts n_m over all troughs, then walks the
//                                     troughs in lag order, PYIN tile rows at a time, with its running count pos, and writes
//                                     below * ((1 - e^-lam) / (1 - e^(-lam n_m)) * e^(-lam pos)) * beta[m] into the LDS tile
//                                     [rows][N | 1]; thread r then adds row r with m ascending: P_k. Work O(K N), no atomics.
//                                  c. g, the first index of the minimum height, by two 64-bit integer minima (bit patterns of h >= 0
//                                     order as values); thread 0 adds no_trough_prob * (the sum of beta[m] with h_g >= t_m, m ascending).
//                                  d. thread k: P_k > 0 gives the bin of step 5. Periods grow with the lag (|shift| < 1, troughs are
//                                     two lags apart), so the bins do not grow, and the candidates of one bin are neighbours among the
//                                     candidates: a candidate whose next candidate has the same bin is dropped (the largest lag
//                                     wins). The winners store obs[f][bin] into the row the workgroup zeroed; thread 0 adds them
//                                     with the lag descending, which is b ascending (the zeros of the dense row add nothing): vp.
//                                Column 2 of the row and vp[f] (float64, for the decode) are written here.
//   3. vsyn_pyin_decode_kernel   one workgroup of 1024 threads per segment, frames in sequence: the Viterbi of step 7. value ping-pongs
//                                in LDS as float64 [2][2B]. Per frame: u[i] = the better of (value[0][i] + log tiny, i) and
//                                (value[1][i] + log tiny, B + i); an inclusive prefix and an inclusive suffix scan of u under the total
//                                order "greater value, then lower state" (two elements a thread, shuffles through the wave, the
//                                waves' totals through LDS) give the out-of-band term of every target: prefix[j - h - 1] and
//                                suffix[j + h + 1]. Target (v', j) then walks its 2 (2h + 1) sources in the band with the log table
//                                (interior row from LDS, the 2h edge rows from global memory) in ascending state order, where only a
//                                strictly greater value replaces, joins that with the two out-of-band candidates, stores
//                                log(obs + tiny) + best and the best source as 2 bytes. The order is total, so the result is that of a
//                                dense sweep with np.argmax's lowest index, whatever the grouping. After the last frame: the
//                                lowest arg-max by the same order through the wave and the waves, and thread 0 walks the back
//                                pointers and writes the states (and columns 0 and 1 of the rows). No floating-point atomics.
//                                This kernel is vsyn_pyin_decode_device's too: there vp comes from a pass over the caller's rows
//                                (thread per frame, b ascending).
//   4. vsyn_pyin_finish_kernel   one workgroup per segment: a segment with a flagged tile is refused (frames_finish, 3 columns). The
//                                decode kernel skips such a segment: its observations are not looked at.
// Memory of the stage per segment of F frames: 8 F B bytes of observations, 4 F B bytes of back pointers (2 bytes for each of the 2B
// states), 8 F bytes of vp.
#pragma once
#include "vsyn_device.h"
#include "vsyn_frames.h"
#include "vsyn_host.h"
#include "vsyn_trim.h"
#include "vsyn_yin.h"

#define PYIN_FT_MAX 64u
#define PYIN_LDS_BUDGET (79u * 1024u)  // as the pitch kernel's
#define PYIN_TILE_BYTES (24u * 1024u)  // the LDS tile of step b, at most
#define PYIN_TILE_ROWS 64u
#define PYIN_MAX_N 1024u
#define PYIN_M (PYIN_MAX_N / PITCH_THREADS)  // thresholds a thread, at most
#define PYIN_NO_BIN 0xFFFFu
#define PYIN_DEC_THREADS 1024
#define PYIN_DEC_WAVES (PYIN_DEC_THREADS / 64)
#define PYIN_NO_STATE 0xFFFFFFFFu

struct PyinCtx {  // launch arguments of the offsets, observation and finishing kernels
  const PitchSeg* seg;  // the periods, as the pitch stage's
  const float* pcm;
  uint64_t plane;
  uint32_t C, S;
  const uint32_t* frames;
  const SegInfo* si;
  uint32_t L, H, FT;
  uint32_t center;
  uint32_t tiles;
  uint32_t N, NS, TR, KM;  // thresholds, the tile's row stride in doubles (N | 1), its rows, the most troughs of a frame
  uint32_t B, lists;       // pitch bins; doubles of LDS in front of d
  double fmin, nb, lam, ntp;  // nb = 12 bps
  const double* thr;       // [N] t_m
  const double* beta;      // [N] beta_probs
  uint32_t* segF;
  uint64_t* segoff;
  uint32_t* flags;
  uint32_t* refused;
  float* rows;             // [segoff[S]][3]
  double* obs;             // [segoff[S]][B]
  double* vp;              // [segoff[S]]
};

__global__ void __launch_bounds__(PITCH_THREADS) vsyn_pyin_offsets_kernel(const PyinCtx A) {
  frames_offsets(A, A.L, [&](uint32_t g) { return A.seg[g].p_max == 0u; });
}

__global__ void __launch_bounds__(PITCH_THREADS) vsyn_pyin_obs_kernel(const PyinCtx A) {
  extern __shared__ double s_pyin[];
  __shared__ uint64_t s_r[PITCH_WAVES];
  __shared__ double s_w[PITCH_WAVES];
  __shared__ uint32_t s_u[PITCH_WAVES];
  const uint32_t g = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const PitchSeg sg = A.seg[g];
  FramesTile t;
  if (frames_tile_head(A, sg.p_max == 0u, t)) return frames_tile_idle(t);
  frames_tile_derive(A, A.L, t);
  const uint32_t L = A.L, W = L / 2u, PL = sg.p_max;
  const uint32_t nf = t.nf, fstep = t.fstep;
  const uint64_t f0 = t.f0;
  float* s_y = (float*)s_pyin;
  double* s_d = s_pyin + A.lists;
  frames_tile_stage(A, t, s_y);
  if (nf == 0u) return;

  yin_difference(s_y, s_d, nf, fstep, W, PL);  // (ends behind a barrier: the span is dead from here on)

  const uint32_t N = A.N, NS = A.NS, TR = A.TR, B = A.B;
  double* s_P = s_pyin;                            // [KM] P_k
  double* s_tile = s_P + A.KM;                     // [TR][NS]
  uint16_t* s_ti = (uint16_t*)(s_tile + (size_t)TR * NS);  // [KM] the troughs' lag indices, ascending
  uint16_t* s_bin = s_ti + A.KM;                   // [KM] a candidate's bin, else PYIN_NO_BIN
  const uint32_t p_min = sg.p_min, n = PL - p_min + 1u;
  const uint32_t Kc = (n + PITCH_THREADS - 1u) / PITCH_THREADS;
  const uint32_t i0 = tid * Kc < n ? tid * Kc : n, i1 = i0 + Kc < n ? i0 + Kc : n;
  const double lam = A.lam;
  double thr[PYIN_M], beta[PYIN_M];
#pragma unroll
  for (uint32_t q = 0; q < PYIN_M; ++q) {
    const uint32_t m = tid + q * PITCH_THREADS;
    thr[q] = m < N ? A.thr[m] : 0.0;
    beta[q] = m < N ? A.beta[m] : 0.0;
  }
  const uint64_t r0 = A.segoff[g] + f0;
  for (uint32_t f = 0; f < nf; ++f) {
    double* d = s_d + (size_t)f * PL;
    yin_normalise(d, PL, p_min, s_w);
    const double* c = d + (p_min - 1u);
    double* obs = A.obs + (size_t)(r0 + f) * B;
    for (uint32_t b = tid; b < B; b += PITCH_THREADS) obs[b] = 0.0;
    // a. the troughs, in ascending lag
    uint32_t cnt = 0;
    for (uint32_t i = i0; i < i1; ++i) cnt += yin_trough(c, i, n) ? 1u : 0u;
    const uint32_t inc = wave_scan(cnt);
    if (lane == 63u) s_u[wave] = inc;
    __syncthreads();
    uint32_t at = inc - cnt, K = 0;
#pragma unroll
    for (uint32_t w = 0; w < PITCH_WAVES; ++w) {
      if (w < wave) at += s_u[w];
      K += s_u[w];
    }
    for (uint32_t i = i0; i < i1; ++i)
      if (yin_trough(c, i, n)) s_ti[at++] = (uint16_t)i;
    __syncthreads();  // (s_u is free again, the list stands)
    if (K == 0u) {    // (workgroup-uniform) no voiced observation
      if (tid == 0) {
        A.rows[3u * (r0 + f) + 2u] = 0.f;
        A.vp[r0 + f] = 0.0;
      }
      continue;
    }
    // b. n_m, then the terms tile by tile and the row sums
    double fact[PYIN_M];
    uint32_t pos[PYIN_M];
#pragma unroll
    for (uint32_t q = 0; q < PYIN_M; ++q) {
      uint32_t nm = 0;
      if (tid + q * PITCH_THREADS < N)
        for (uint32_t k = 0; k < K; ++k) nm += c[s_ti[k]] < thr[q] ? 1u : 0u;
      fact[q] = (1.0 - exp(-lam)) / (1.0 - exp(-lam * (double)nm));  // (nm = 0: never used)
      pos[q] = 0u;
    }
    for (uint32_t k0 = 0; k0 < K; k0 += TR) {
      const uint32_t rows = K - k0 < TR ? K - k0 : TR;
#pragma unroll
      for (uint32_t q = 0; q < PYIN_M; ++q) {
        const uint32_t m = tid + q * PITCH_THREADS;
        if (m < N)
          for (uint32_t r = 0; r < rows; ++r) {
            const bool below = c[s_ti[k0 + r]] < thr[q];
            s_tile[(size_t)r * NS + m] = below ? (fact[q] * exp(-lam * (double)pos[q])) * beta[q] : 0.0;
            pos[q] += below ? 1u : 0u;
          }
      }
      __syncthreads();
      if (tid < rows) {
        const double* row = s_tile + (size_t)tid * NS;
        double acc = 0.0;
        for (uint32_t m = 0; m < N; ++m) acc += row[m];
        s_P[k0 + tid] = acc;
      }
      __syncthreads();
    }
    // c. the lowest trough takes the no-trough mass
    uint64_t low = PITCH_NONE, first = PITCH_NONE;
    for (uint32_t k = tid; k < K; k += PITCH_THREADS) low = trim_min64(low, (uint64_t)__double_as_longlong(c[s_ti[k]]));
    low = pitch_wg_min(low, s_r);
    for (uint32_t k = tid; k < K; k += PITCH_THREADS)
      if ((uint64_t)__double_as_longlong(c[s_ti[k]]) == low) first = trim_min64(first, k);
    first = pitch_wg_min(first, s_r);
    if (first == PITCH_NONE) first = 0ull;  // (a NaN among the c of a segment that is refused anyway)
    if (tid == 0) {
      const double hg = c[s_ti[first]];
      double acc = 0.0;
      for (uint32_t m = 0; m < N; ++m)
        if (!(hg < A.thr[m])) acc += A.beta[m];
      s_P[first] += A.ntp * acc;
    }
    __syncthreads();
    // d. candidates, one winner a bin, the dense row and vp
    for (uint32_t k = tid; k < K; k += PITCH_THREADS) {
      uint32_t bin = PYIN_NO_BIN;
      if (s_P[k] > 0.0) {
        const uint32_t i = s_ti[k];
        const double period = (double)(p_min + i) + yin_shift(c, i, n);
        const double fb = rint(A.nb * log2((sg.sr / period) / A.fmin));
        if (fb < (double)B) bin = fb > 0.0 ? (uint32_t)fb : 0u;  // (clipped to [0, B]; bin B is dropped; a NaN is dropped)
      }
      s_bin[k] = (uint16_t)bin;
    }
    __syncthreads();
    uint32_t win = 0u, nw = 0u;  // (a bit a trough of this thread: K <= 2049 = 8 * 256 + 1)
    for (uint32_t k = tid; k < K; k += PITCH_THREADS, ++nw) {
      const uint32_t bin = s_bin[k];
      bool w = bin != PYIN_NO_BIN;
      if (w)
        for (uint32_t k2 = k + 1u; k2 < K; ++k2) {
          const uint32_t b2 = s_bin[k2];
          if (b2 != PYIN_NO_BIN) {
            w = b2 != bin;
            break;
          }
        }
      win |= w ? 1u << nw : 0u;
    }
    __syncthreads();
    nw = 0;
    for (uint32_t k = tid; k < K; k += PITCH_THREADS, ++nw) {
      if ((win >> nw) & 1u) obs[s_bin[k]] = s_P[k];
      else s_bin[k] = (uint16_t)PYIN_NO_BIN;
    }
    __syncthreads();
    if (tid == 0) {
      double acc = 0.0;
      for (uint32_t k = K; k-- > 0u;)
        if (s_bin[k] != PYIN_NO_BIN) acc += s_P[k];
      const double vp = acc < 0.0 ? 0.0 : acc > 1.0 ? 1.0 : acc;
      A.rows[3u * (r0 + f) + 2u] = (float)vp;
      A.vp[r0 + f] = vp;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(PITCH_THREADS) vsyn_pyin_finish_kernel(const PyinCtx A) { frames_finish(A, 3u); }

// ------------------------------------------------------------------------------------------------
// the Viterbi decode
// ------------------------------------------------------------------------------------------------
struct PyinDecSeg {
  uint32_t h;    // half width of the band
  uint32_t tab;  // offset in doubles of the segment's log table in tabs
};

struct PyinDecCtx {
  const PyinDecSeg* seg;
  const double* tabs;      // per rate: rows [R][w][2] (stay, switch), R = B where B < w, else 2h + 1: rows 0 .. h - 1 the low edge, row h
                           // the interior, rows h + 1 .. 2h the sources B - h .. B - 1
  const float* ftab;       // [B] the bins' frequencies (may be NULL with rows NULL)
  const double* obs;       // [segoff[S]][B]
  const uint32_t* segF;
  const uint64_t* segoff;
  const uint32_t* flags;   // the observation kernel's flag words (NULL: the caller's observations)
  uint32_t tiles;
  uint32_t B;
  uint32_t vp_ready;       // vp stands (the observation kernel wrote it); 0: computed here from obs
  double lt, linit;        // log(tiny), log(1 / (2B) + tiny)
  double* vp;              // [segoff[S]]
  uint16_t* bp;            // [segoff[S]][2B]
  uint32_t* states;        // [segoff[S]] (may be NULL)
  float* rows;             // [segoff[S]][3] (may be NULL)
};

struct PyinBest {
  double v;
  uint32_t s;
};
// the total order of every reduction here: the greater value, then the lower state
__device__ __forceinline__ bool pyin_better(double v, uint32_t s, const PyinBest& b) { return v > b.v || (v == b.v && s < b.s); }
__device__ __forceinline__ PyinBest pyin_max(const PyinBest& a, const PyinBest& b) {
  const bool t = pyin_better(a.v, a.s, b);  // (member by member: a select between the two structs goes through scratch)
  return PyinBest{t ? a.v : b.v, t ? a.s : b.s};
}
__device__ __forceinline__ PyinBest pyin_none() { return PyinBest{-__builtin_inf(), PYIN_NO_STATE}; }
__device__ __forceinline__ PyinBest pyin_up(const PyinBest& a, unsigned o) { return PyinBest{__shfl_up(a.v, o), (uint32_t)__shfl_up((int)a.s, o)}; }
__device__ __forceinline__ PyinBest pyin_down(const PyinBest& a, unsigned o) { return PyinBest{__shfl_down(a.v, o), (uint32_t)__shfl_down((int)a.s, o)}; }
__device__ __forceinline__ PyinBest pyin_xor(const PyinBest& a, int o) { return PyinBest{__shfl_xor(a.v, o), (uint32_t)__shfl_xor((int)a.s, o)}; }

static inline size_t pyin_dec_lds_bytes(uint32_t B, uint32_t w_max) {
  // value [2][2B] | prefix and suffix values [2][B] | interior row [w][2] | the waves' totals [2][WAVES] (values, then states) |
  // prefix and suffix states [2][B] uint16
  return 8u * (4u * (size_t)B + 2u * B + 2u * w_max + 2u * PYIN_DEC_WAVES) + 4u * 2u * PYIN_DEC_WAVES + 2u * 2u * (size_t)B + 16u;
}

__global__ void __launch_bounds__(PYIN_DEC_THREADS) vsyn_pyin_decode_kernel(const PyinDecCtx A) {
  extern __shared__ double s_dec[];
  const uint32_t g = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint32_t F = A.segF[g], B = A.B, NSt = 2u * B;
  if (F == 0u) return;
  if (A.flags) {  // a refused segment: nothing to decode (its rows become NaN in the finishing kernel)
    bool bad = false;
    for (uint32_t i = tid; i < A.tiles; i += PYIN_DEC_THREADS) bad |= A.flags[(size_t)g * A.tiles + i] != 0u;
    if (__syncthreads_or(bad ? 1 : 0)) return;
  }
  const PyinDecSeg sg = A.seg[g];
  const uint32_t h = sg.h, w = 2u * h + 1u;
  const bool full = B < w;  // every row is an edge row
  const double* tab = A.tabs + sg.tab;
  const uint64_t off = A.segoff[g];
  const double* obs = A.obs + (size_t)off * B;
  double* vp = A.vp + off;
  uint16_t* bp = A.bp + (size_t)off * NSt;

  double* s_val = s_dec;                          // [2][2B]
  double* s_pv = s_val + 2u * (size_t)NSt;        // [B] prefix values
  double* s_sv = s_pv + B;                        // [B] suffix values
  double* s_int = s_sv + B;                       // [w][2]
  double* s_wv = s_int + (full ? 0u : 2u * (size_t)w);  // [2][WAVES]
  uint32_t* s_ws = (uint32_t*)(s_wv + 2u * PYIN_DEC_WAVES);  // [2][WAVES]
  uint16_t* s_ps = (uint16_t*)(s_ws + 2u * PYIN_DEC_WAVES);  // [B] prefix states
  uint16_t* s_ss = s_ps + B;                      // [B] suffix states

  if (!full)
    for (uint32_t i = tid; i < 2u * w; i += PYIN_DEC_THREADS) s_int[i] = tab[(size_t)h * w * 2u + i];
  if (!A.vp_ready) {
    for (uint32_t f = tid; f < F; f += PYIN_DEC_THREADS) {
      const double* row = obs + (size_t)f * B;
      double acc = 0.0;
      for (uint32_t b = 0; b < B; ++b) acc += row[b];
      vp[f] = acc < 0.0 ? 0.0 : acc > 1.0 ? 1.0 : acc;
    }
    __threadfence();
  }
  __syncthreads();

  const bool oob = B > h + 1u;  // some target has a source outside its band
  constexpr uint32_t PER = 4u;  // states a thread: 2B <= 4096
  uint32_t cur = 0;
  for (uint32_t t = 0; t < F; ++t) {
    // log(obs + tiny) of this thread's targets (the loads run ahead of the scans)
    const double un = log((1.0 - vp[t]) / (double)B + PITCH_TINY);
    double lo[PER];
#pragma unroll
    for (uint32_t q = 0; q < PER; ++q) {
      const uint32_t s = tid + q * PYIN_DEC_THREADS;
      lo[q] = s < B ? log(obs[(size_t)t * B + s] + PITCH_TINY) : un;
    }
    const double* pv = s_val + (size_t)cur * NSt;
    double* nv = s_val + (size_t)(cur ^ 1u) * NSt;
    if (t == 0u) {
#pragma unroll
      for (uint32_t q = 0; q < PER; ++q) {
        const uint32_t s = tid + q * PYIN_DEC_THREADS;
        if (s < NSt) nv[s] = lo[q] + A.linit;
      }
      __syncthreads();
      cur ^= 1u;
      continue;
    }
    if (oob) {  // (workgroup-uniform)
      const uint32_t e0 = 2u * tid, e1 = e0 + 1u;
      PyinBest a = pyin_none(), b = pyin_none();
      if (e0 < B) a = pyin_max(PyinBest{pv[e0] + A.lt, e0}, PyinBest{pv[B + e0] + A.lt, B + e0});
      if (e1 < B) b = pyin_max(PyinBest{pv[e1] + A.lt, e1}, PyinBest{pv[B + e1] + A.lt, B + e1});
      const PyinBest tot = pyin_max(a, b);
      PyinBest pi = tot, si = tot;  // inclusive through the wave, upwards and downwards
      for (uint32_t o = 1; o < 64u; o <<= 1) {
        const PyinBest u = pyin_up(pi, o), d = pyin_down(si, o);
        if (lane >= o) pi = pyin_max(pi, u);
        if (lane + o < 64u) si = pyin_max(si, d);
      }
      if (lane == 63u) s_wv[wave] = pi.v, s_ws[wave] = pi.s;
      if (lane == 0u) s_wv[PYIN_DEC_WAVES + wave] = si.v, s_ws[PYIN_DEC_WAVES + wave] = si.s;
      PyinBest pe = pyin_up(pi, 1), se = pyin_down(si, 1);  // exclusive
      if (lane == 0u) pe = pyin_none();
      if (lane == 63u) se = pyin_none();
      __syncthreads();
      for (uint32_t x = 0; x < PYIN_DEC_WAVES; ++x) {
        if (x < wave) pe = pyin_max(pe, PyinBest{s_wv[x], s_ws[x]});
        if (x > wave) se = pyin_max(se, PyinBest{s_wv[PYIN_DEC_WAVES + x], s_ws[PYIN_DEC_WAVES + x]});
      }
      const PyinBest p0 = pyin_max(pe, a), p1 = pyin_max(p0, b), q1 = pyin_max(se, b), q0 = pyin_max(q1, a);
      if (e0 < B) s_pv[e0] = p0.v, s_ps[e0] = (uint16_t)p0.s, s_sv[e0] = q0.v, s_ss[e0] = (uint16_t)q0.s;
      if (e1 < B) s_pv[e1] = p1.v, s_ps[e1] = (uint16_t)p1.s, s_sv[e1] = q1.v, s_ss[e1] = (uint16_t)q1.s;
      __syncthreads();
    }
#pragma unroll
    for (uint32_t q = 0; q < PER; ++q) {
      const uint32_t s = tid + q * PYIN_DEC_THREADS;
      if (s >= NSt) continue;
      const uint32_t v1 = s >= B ? 1u : 0u, j = s - v1 * B;
      PyinBest best = pyin_none();
      if (j > h) best = PyinBest{s_pv[j - h - 1u], s_ps[j - h - 1u]};
      if (j + h + 1u < B) {
        const PyinBest x{s_sv[j + h + 1u], s_ss[j + h + 1u]};
        best = pyin_max(x, best);
      }
      // the band in ascending state order, voicing 0 then 1: only a strictly greater value replaces, so the lowest state of a maximum
      // stays. Three runs of sources: the low edge rows and the high edge rows from the table, the interior row from LDS.
      const uint32_t ia = j > h ? j - h : 0u, ie = (j + h < B ? j + h : B - 1u) + 1u;
      const uint32_t i_lo = full ? ie : (h < ie ? (h > ia ? h : ia) : ie);          // [ia, i_lo): rows i
      const uint32_t i_in = full ? ie : (B - h < ie ? (B - h > i_lo ? B - h : i_lo) : ie);  // [i_lo, i_in): the interior row
      double bv = -__builtin_inf();
      uint32_t bs = PYIN_NO_STATE;
#pragma unroll
      for (uint32_t v = 0; v < 2u; ++v) {
        const uint32_t x = v ^ v1, sb = v * B;  // x: 0 the same voicing, 1 the other
        const double* p = pv + sb;
        for (uint32_t i = ia; i < i_lo; ++i) {
          const double c = p[i] + tab[((size_t)i * w + (j + h - i)) * 2u + x];
          if (c > bv) bv = c, bs = sb + i;
        }
        for (uint32_t i = i_lo; i < i_in; ++i) {
          const double c = p[i] + s_int[(j + h - i) * 2u + x];
          if (c > bv) bv = c, bs = sb + i;
        }
        for (uint32_t i = i_in; i < ie; ++i) {
          const double c = p[i] + tab[((size_t)(i - (B - h) + h + 1u) * w + (j + h - i)) * 2u + x];
          if (c > bv) bv = c, bs = sb + i;
        }
      }
      best = pyin_max(best, PyinBest{bv, bs});
      nv[s] = lo[q] + best.v;
      bp[(size_t)t * NSt + s] = (uint16_t)(best.s < NSt ? best.s : 0u);  // (no source beats -inf only among NaN values: state 0)
    }
    __syncthreads();
    cur ^= 1u;
  }
  // the lowest arg-max of the last frame's values
  const double* fv = s_val + (size_t)cur * NSt;
  PyinBest best = pyin_none();
#pragma unroll
  for (uint32_t q = 0; q < PER; ++q) {
    const uint32_t s = tid + q * PYIN_DEC_THREADS;
    if (s < NSt && pyin_better(fv[s], s, best)) best = PyinBest{fv[s], s};
  }
  for (int o = 32; o; o >>= 1) best = pyin_max(best, pyin_xor(best, o));
  if (lane == 0u) s_wv[wave] = best.v, s_ws[wave] = best.s;
  __threadfence();  // (the back pointers, read below by thread 0)
  __syncthreads();
  if (tid != 0u) return;
  best = pyin_none();
  for (uint32_t x = 0; x < PYIN_DEC_WAVES; ++x) best = pyin_max(best, PyinBest{s_wv[x], s_ws[x]});
  uint32_t st = best.s < NSt ? best.s : 0u;
  for (uint32_t t = F; t-- > 0u;) {
    if (A.states) A.states[off + t] = st;
    if (A.rows) {
      float* row = A.rows + 3u * (off + t);
      row[0] = A.ftab[st < B ? st : st - B];
      row[1] = st < B ? 1.f : 0.f;
    }
    if (t) st = bp[(size_t)t * NSt + st];
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct PyinWs {  // the stage's buffers: its own; the PCM is only read
  TableUpload tab;
  bool lds_set = false;
  DevBuf<uint32_t> segF, flags, refused;
  DevBuf<uint64_t> segoff;
  DevBuf<float> rows;  // host form: the rows
  DevBuf<double> obs, vp;
  DevBuf<uint16_t> bp;
};

static inline bool pyin_center(const vsyn_pyin_spec* sp) { return (sp->options & VSYN_PYIN_CENTER) != 0; }
static inline uint32_t pyin_bps(const vsyn_pyin_spec* sp) { return (uint32_t)ceil(1.0 / sp->resolution); }
// B of step 5, in double; 0 when it does not fit 32 bits
static inline uint32_t pyin_bins(const vsyn_pyin_spec* sp) {
  const double b = floor(12.0 * (double)pyin_bps(sp) * log2(sp->fmax / sp->fmin)) + 1.0;
  return b >= 1.0 && b < 4294967295.0 ? (uint32_t)b : 0u;
}
// w of step 6 for rate sr; 0 when it does not fit
static inline uint32_t pyin_width(const vsyn_pyin_spec* sp, uint32_t sr) {
  const double msf = nearbyint(sp->max_transition_rate * 12.0 * (double)sp->hop_length / (double)sr);  // (round half even, as Python's round)
  const double w = msf * (double)pyin_bps(sp) + 1.0;
  return w >= 1.0 && w < 4294967295.0 ? (uint32_t)w : 0u;
}
static inline bool pyin_periods(const vsyn_pyin_spec* sp, uint32_t sr, uint32_t* p_min, uint32_t* p_max) {
  const vsyn_pitch_spec ps = {sp->frame_length, sp->hop_length, 0u, 0u, sp->fmin, sp->fmax, 1.0};
  return pitch_periods(&ps, sr, p_min, p_max);
}

// The checks of step 10, and of every segment's rate (0 = skipped segment).
static inline int pyin_check(const vsyn_pyin_spec* sp, uint32_t S, const uint32_t* rates, const char** err) {
  if (!sp) return fail(err, VSYN_ERR_INVALID, "pyin spec is NULL");
  const vsyn_pitch_spec ps = {sp->frame_length, sp->hop_length, sp->options, 0u, sp->fmin, sp->fmax, 1.0};
  if (int rc = pitch_check(&ps, 0, nullptr, err)) return rc;
  if (sp->n_thresholds < 1 || sp->n_thresholds > PYIN_MAX_N)
    return fail(err, VSYN_ERR_INVALID, "pyin n_thresholds %u outside [1, %u]", sp->n_thresholds, PYIN_MAX_N);
  if (!sp->threshold_probs) return fail(err, VSYN_ERR_INVALID, "pyin threshold_probs is NULL");
  for (uint32_t m = 0; m < sp->n_thresholds; ++m)
    if (!std::isfinite(sp->threshold_probs[m]) || !(sp->threshold_probs[m] >= 0.0))
      return fail(err, VSYN_ERR_INVALID, "pyin threshold_probs[%u] = %g: need finite and >= 0", m, sp->threshold_probs[m]);
  if (!std::isfinite(sp->boltzmann_parameter) || !(sp->boltzmann_parameter > 0.0))
    return fail(err, VSYN_ERR_INVALID, "pyin boltzmann_parameter %g: need finite and > 0", sp->boltzmann_parameter);
  if (!(sp->resolution > 0.0 && sp->resolution < 1.0)) return fail(err, VSYN_ERR_INVALID, "pyin resolution %g outside (0, 1)", sp->resolution);
  if (!std::isfinite(sp->max_transition_rate) || !(sp->max_transition_rate > 0.0))
    return fail(err, VSYN_ERR_INVALID, "pyin max_transition_rate %g: need finite and > 0", sp->max_transition_rate);
  if (!(sp->switch_prob > 0.0 && sp->switch_prob < 1.0)) return fail(err, VSYN_ERR_INVALID, "pyin switch_prob %g outside (0, 1)", sp->switch_prob);
  if (!(sp->no_trough_prob >= 0.0 && sp->no_trough_prob <= 1.0))
    return fail(err, VSYN_ERR_INVALID, "pyin no_trough_prob %g outside [0, 1]", sp->no_trough_prob);
  const uint32_t B = pyin_bins(sp);
  if (B == 0u || 2ull * B > VSYN_PYIN_MAX_STATES)
    return fail(err, VSYN_ERR_INVALID, "pyin: 2 * %u pitch bins above the %u states of a frame", B, VSYN_PYIN_MAX_STATES);
  if (S && !rates) return fail(err, VSYN_ERR_INVALID, "sample_rates is NULL");
  for (uint32_t g = 0; g < S; ++g) {
    if (!rates[g]) continue;
    uint32_t p_min, p_max;
    if (sp->fmax > rates[g] / 2.0) return fail(err, VSYN_ERR_INVALID, "segment %u: fmax %g above sr/2 = %g", g, sp->fmax, rates[g] / 2.0);
    if (!pyin_periods(sp, rates[g], &p_min, &p_max))
      return fail(err, VSYN_ERR_INVALID, "segment %u: fewer than two lags between sr/fmax and min(sr/fmin, frame_length - frame_length/2 - 1)", g);
    const uint32_t w = pyin_width(sp, rates[g]);
    if (w == 0u || !(w & 1u) || w > 2u * VSYN_PYIN_MAX_STATES)
      return fail(err, VSYN_ERR_INVALID, "segment %u: transition width %u at rate %u: need an odd width (an even one is not built)", g, w, rates[g]);
  }
  return VSYN_OK;
}

// loc row i of step 6, normalised: out[k], k = j - i + h for |j - i| <= h; 0 where j is outside [0, B)
static inline void pyin_loc_row(uint32_t B, uint32_t h, uint32_t i, double* out) {
  const uint32_t w = 2u * h + 1u;
  const double half = (double)(w + 1u) / 2.0;
  for (uint32_t k = 0; k < w; ++k) {
    const int64_t j = (int64_t)i + k - h;
    const double dist = (double)(k > h ? k - h : h - k);
    out[k] = j >= 0 && j < (int64_t)B ? (half - dist) / half : 0.0;
  }
  // the sum from the outside in, the two entries of a distance first: rows i and B - 1 - i, mirror images, get the same bits
  double sum = 0.0;
  for (uint32_t d = h; d >= 1u; --d) sum += out[h - d] + out[h + d];
  sum += out[h];
  for (uint32_t k = 0; k < w; ++k) out[k] /= sum;
}
// the log rows of source bin i: out[k][2] = log((1 - s) loc + tiny), log(s loc + tiny)
static inline void pyin_log_row(const vsyn_pyin_spec* sp, uint32_t B, uint32_t h, uint32_t i, double* out) {
  const uint32_t w = 2u * h + 1u;
  std::vector<double> loc(w);
  pyin_loc_row(B, h, i, loc.data());
  for (uint32_t k = 0; k < w; ++k) {
    out[2u * k] = log((1.0 - sp->switch_prob) * loc[k] + PITCH_TINY);
    out[2u * k + 1u] = log(sp->switch_prob * loc[k] + PITCH_TINY);
  }
}
// rows of the device form of the table, and the source bin of its row r
static inline uint32_t pyin_tab_rows(uint32_t B, uint32_t h) { return B < 2u * h + 1u ? B : 2u * h + 1u; }
static inline uint32_t pyin_tab_source(uint32_t B, uint32_t h, uint32_t r) { return B < 2u * h + 1u || r <= h ? r : B - h + (r - h - 1u); }

static inline size_t pyin_obs_lists(uint32_t km, uint32_t tr, uint32_t ns) {  // doubles of LDS the lists of a frame take
  return (size_t)km + (size_t)tr * ns + ((size_t)km * 4u + 7u) / 8u;
}
static inline size_t pyin_span_doubles(uint32_t ft, uint32_t L, uint32_t H) { return ((size_t)(ft - 1u) * std::min(L, H) + L + 1u) >> 1; }

// The decode kernel over the stage's workspace (d_obs NULL: ws.obs, with vp from the observation kernel and the flags) or over the
// caller's observations. tab: the uploaded table's host image, to which the decode's records and tables are appended BEFORE the
// upload by pyin_dec_tables; this launches behind it.
struct PyinDecTables {
  size_t seg, tabs, ftab;  // byte offsets into the table
  uint32_t w_max;
};
static inline PyinDecTables pyin_dec_tables(const vsyn_pyin_spec* sp, uint32_t S, const uint32_t* rates, std::vector<uint8_t>& tab) {
  const uint32_t B = pyin_bins(sp), bps = pyin_bps(sp);
  PyinDecTables o;
  o.w_max = 1u;
  std::vector<PyinDecSeg> seg(S);
  std::vector<std::pair<uint32_t, uint32_t>> placed;
  std::vector<double> tabs;
  for (uint32_t g = 0; g < S; ++g) {
    seg[g] = PyinDecSeg{0u, 0u};
    if (!rates[g]) continue;
    const uint32_t w = pyin_width(sp, rates[g]), h = w / 2u, R = pyin_tab_rows(B, h);
    uint32_t next = (uint32_t)tabs.size();
    const uint32_t at = table_slot(placed, w, &next, R * w * 2u);
    if (next != tabs.size()) {
      tabs.resize(next);
      for (uint32_t r = 0; r < R; ++r) pyin_log_row(sp, B, h, pyin_tab_source(B, h, r), tabs.data() + at + (size_t)r * w * 2u);
    }
    seg[g] = PyinDecSeg{h, at};
    o.w_max = std::max(o.w_max, w);
  }
  std::vector<float> ftab(B);
  for (uint32_t b = 0; b < B; ++b) ftab[b] = (float)(sp->fmin * exp2((double)b / (12.0 * (double)bps)));
  tab.resize(align_up(tab.size(), 8));
  o.seg = tab.size();
  tab.insert(tab.end(), (const uint8_t*)seg.data(), (const uint8_t*)(seg.data() + S));
  tab.resize(align_up(tab.size(), 8));
  o.tabs = tab.size();
  tab.insert(tab.end(), (const uint8_t*)tabs.data(), (const uint8_t*)(tabs.data() + tabs.size()));
  o.ftab = tab.size();
  tab.insert(tab.end(), (const uint8_t*)ftab.data(), (const uint8_t*)(ftab.data() + B));
  tab.resize(align_up(tab.size(), 8));
  return o;
}

static inline int pyin_raise_lds(PyinWs& ws, const char** err) {
  return raise_lds_once(ws.lds_set, {{(const void*)vsyn_pyin_obs_kernel, PYIN_LDS_BUDGET}, {(const void*)vsyn_pyin_decode_kernel, pyin_dec_lds_bytes(VSYN_PYIN_MAX_STATES / 2u, VSYN_PYIN_MAX_STATES / 2u)}}, err);
}

static inline int pyin_dec_launch(PyinWs& ws, const vsyn_pyin_spec* sp, uint32_t S, const PyinDecTables& dt, PyinDecCtx& D, hipStream_t s, const char** err) {
  const uint32_t B = pyin_bins(sp);
  const uint8_t* base = ws.tab.dev.p;
  D.seg = (const PyinDecSeg*)(base + dt.seg);
  D.tabs = (const double*)(base + dt.tabs);
  D.ftab = (const float*)(base + dt.ftab);
  D.B = B;
  D.lt = log(PITCH_TINY);
  D.linit = log(1.0 / (double)(2u * B) + PITCH_TINY);
  D.vp = ws.vp.p;
  D.bp = ws.bp.p;
  // a band wider than the bins is never walked past them: the interior row is only staged where B >= w
  VSYN_LAUNCH(vsyn_pyin_decode_kernel, dim3(S), dim3(PYIN_DEC_THREADS), pyin_dec_lds_bytes(B, std::min(dt.w_max, B)), s, D);
  return VSYN_OK;
}

// Offsets, observation, decode and finishing kernels on stream s; frames from d_frames, else from si. f_max bounds every segment's
// frames, rows_bound the frames of all of them. d_refused [S] may be NULL. Caller holds the handle's lock and has run pyin_check.
static inline int pyin_launch(PyinWs& ws, int device, const vsyn_pyin_spec* sp, uint32_t S, const uint32_t* rates, const float* d_pcm, uint64_t plane,
                              uint32_t C, const uint32_t* d_frames, const SegInfo* si, uint64_t f_max, uint64_t rows_bound, float* d_rows,
                              uint64_t* d_segoff, uint32_t* d_refused, hipStream_t s, const char** err) {
  if (int rc = frames_check_call(S, d_pcm, d_rows, plane, err)) return rc;
  const uint32_t L = sp->frame_length, H = sp->hop_length, N = sp->n_thresholds, B = pyin_bins(sp);
  std::vector<uint8_t> tab(sizeof(PitchSeg) * (size_t)S);
  uint32_t pl = 2u;
  {
    PitchSeg* seg = (PitchSeg*)tab.data();
    for (uint32_t g = 0; g < S; ++g) {
      seg[g] = PitchSeg{(double)rates[g], 0u, 0u};
      if (rates[g]) pyin_periods(sp, rates[g], &seg[g].p_min, &seg[g].p_max);
      pl = std::max(pl, seg[g].p_max);
    }
  }
  // t_m = m * (1 / N), m < N, and t_N = 1: numpy.linspace(0, 1, N + 1)[1:]
  std::vector<double> thr(N);
  const double step = 1.0 / (double)N;
  for (uint32_t m = 1; m < N; ++m) thr[m - 1u] = (double)m * step;
  thr[N - 1u] = 1.0;
  const size_t o_thr = tab.size();
  tab.insert(tab.end(), (const uint8_t*)thr.data(), (const uint8_t*)(thr.data() + N));
  const size_t o_beta = tab.size();
  tab.insert(tab.end(), (const uint8_t*)sp->threshold_probs, (const uint8_t*)(sp->threshold_probs + N));
  const PyinDecTables dt = pyin_dec_tables(sp, S, rates, tab);

  const uint32_t ns = N | 1u, km = pl / 2u + 2u;
  const uint32_t tr = std::max(1u, std::min(PYIN_TILE_ROWS, PYIN_TILE_BYTES / (8u * ns)));
  const size_t lists_min = pyin_obs_lists(km, tr, ns);
  uint32_t ft = PYIN_FT_MAX;
  const auto lds_of = [&](uint32_t f) { return 8u * (std::max(lists_min, pyin_span_doubles(f, L, H)) + (size_t)f * pl); };
  while (ft > 1u && lds_of(ft) > PYIN_LDS_BUDGET) --ft;
  if (lds_of(ft) > PYIN_LDS_BUDGET) return fail(err, VSYN_ERR_INVALID, "pyin: one frame's lists do not fit the workgroup's LDS");
  const auto raise_lds = [&]() -> int { return pyin_raise_lds(ws, err); };
  PyinCtx A;
  if (int rc = frames_begin(ws, device, tab, ft, H, pyin_center(sp), S, d_pcm, plane, C, d_frames, si, f_max, d_rows, d_segoff, d_refused, s, err,
                            raise_lds, A))
    return rc;
  rows_bound = std::max<uint64_t>(rows_bound, 1);
  HIPCHK(ws.obs.ensure(rows_bound * B));
  HIPCHK(ws.vp.ensure(rows_bound));
  HIPCHK(ws.bp.ensure(rows_bound * 2u * B));
  const uint8_t* base = ws.tab.dev.p;
  A.seg = (const PitchSeg*)base;
  A.thr = (const double*)(base + o_thr);
  A.beta = (const double*)(base + o_beta);
  A.L = L;
  A.N = N, A.NS = ns, A.TR = tr, A.KM = km;
  A.B = B;
  A.lists = (uint32_t)std::max(lists_min, pyin_span_doubles(ft, L, H));
  A.fmin = sp->fmin;
  A.nb = 12.0 * (double)pyin_bps(sp);
  A.lam = sp->boltzmann_parameter;
  A.ntp = sp->no_trough_prob;
  A.obs = ws.obs.p;
  A.vp = ws.vp.p;
  VSYN_LAUNCH(vsyn_pyin_offsets_kernel, dim3(1), dim3(FRAMES_THREADS), 0, s, A);
  VSYN_LAUNCH(vsyn_pyin_obs_kernel, dim3(A.tiles, A.S), dim3(FRAMES_THREADS), lds_of(ft), s, A);
  PyinDecCtx D;
  D.obs = ws.obs.p;
  D.segF = A.segF;
  D.segoff = A.segoff;
  D.flags = A.flags;
  D.tiles = A.tiles;
  D.vp_ready = 1u;
  D.states = nullptr;
  D.rows = d_rows;
  if (int rc = pyin_dec_launch(ws, sp, S, dt, D, s, err)) return rc;
  VSYN_LAUNCH(vsyn_pyin_finish_kernel, dim3(A.S), dim3(FRAMES_THREADS), 0, s, A);
  return VSYN_OK;
}

// vsyn_pyin_decode_device behind its checks: seg_rows (host) frames per segment, d_obs the rows back to back.
static inline int pyin_decode_launch(PyinWs& ws, int device, const vsyn_pyin_spec* sp, uint32_t S, const uint32_t* rates, const double* d_obs,
                                     const uint64_t* seg_rows, uint32_t* d_states, hipStream_t s, const char** err) {
  std::vector<uint8_t> tab;
  std::vector<uint64_t> off(S + 1u, 0);
  std::vector<uint32_t> F(S, 0);
  for (uint32_t g = 0; g < S; ++g) {
    F[g] = rates[g] ? (uint32_t)seg_rows[g] : 0u;
    off[g + 1u] = off[g] + seg_rows[g];
  }
  tab.insert(tab.end(), (const uint8_t*)off.data(), (const uint8_t*)(off.data() + S + 1u));
  const size_t o_f = tab.size();
  tab.insert(tab.end(), (const uint8_t*)F.data(), (const uint8_t*)(F.data() + S));
  const PyinDecTables dt = pyin_dec_tables(sp, S, rates, tab);
  HIPCHK(hipSetDevice(device));
  if (int rc = pyin_raise_lds(ws, err)) return rc;
  const uint64_t total = std::max<uint64_t>(off[S], 1);
  HIPCHK(ws.vp.ensure(total));
  HIPCHK(ws.bp.ensure(total * 2u * pyin_bins(sp)));
  if (int rc = ws.tab.upload(tab, s, err)) return rc;
  PyinDecCtx D;
  D.obs = d_obs;
  D.segoff = (const uint64_t*)ws.tab.dev.p;
  D.segF = (const uint32_t*)(ws.tab.dev.p + o_f);
  D.flags = nullptr;
  D.tiles = 0u;
  D.vp_ready = 0u;
  D.states = d_states;
  D.rows = nullptr;
  return pyin_dec_launch(ws, sp, S, dt, D, s, err);
}
