// vsyn_rhythm.h — rhythm: onset strength of spectral rows, onset frames of an envelope, the autocorrelation tempogram and its mean
// over time, all on vectors and rows already on the device. Semantics: include/vorbis_synth_hip.h, "rhythm".
//
// Seven kernels, three stages:
//   A. vsyn_onset_kernel           grid (tile of ONS_FT frames, segment), a wave per frame. The reference row g - lag goes to the wave's
//                                  LDS line as order keys (vsyn_hpss.h: NaN the largest key), lane i takes the bins i, i + 64, ..: the
//                                  bin maximum out of LDS, the difference and its clamp in float64, its partial sum; the 64 partials
//                                  are folded by wave_sum, which leaves the same sum in every lane. Rows are read
//                                  coalesced and once (twice with max_size = 1), nothing is accumulated across frames.
//   B. vsyn_peaks_minmax_kernel    one workgroup per segment: float32 minimum and maximum (order keys again: the order of the reads
//                                  cannot show) and whether a value is not finite.
//      vsyn_peaks_cand_kernel      a thread per frame: tests (a) and (b) from global memory (the windows are a few frames), the 64
//                                  answers of a wave as one ballot word.
//      vsyn_peaks_walk_kernel      one wave per segment: 64 ballot words a read, walked in order by the whole wave (the words are
//                                  wave-uniform after a shuffle), lane 0 stores the accepted frames. The only ordered step.
//   C. vsyn_tempogram_kernel       grid (block of tiles, segment). Per tile of FT frames (FT from W alone, tg_tile): y[FT][W] =
//                                  win * e_pad as float64 in LDS, then the (frame, lag) sums. A thread owns a PAIR of lags, l and
//                                  W - 1 - l, of TG_ILP frames: the two chains together have W + 1 terms whatever l is, so the lanes of
//                                  a wave finish within 64 terms of each other although lag l alone has W - l. y[n] is one address per
//                                  frame (a broadcast), y[n + l] consecutive doubles across the lanes (ascending for l, descending for
//                                  W - 1 - l): ds_read_b64 without a conflict. Each sum is ONE fma chain with n ascending, whatever the
//                                  tile and the thread; the TG_ILP chains of a thread are independent and only hide the fma latency.
//                                  The sums go to ac[FT][W] in LDS; per frame the largest |ac| as a 64-bit integer maximum (a NaN's
//                                  image is the largest); then a thread owns the lags tid, tid + 256, ..: it normalises, rounds,
//                                  stores (coalesced along the lag) and adds the float32 value to its lag's block sum, frames
//                                  ascending. A block's sums go to the workspace.
//      vsyn_tempogram_mean_kernel  a thread per lag: the blocks' sums in ascending order, divided by F'.
// No atomics; every order is a function of W, F' and the stage's parameters. Nothing here reads or writes stream state, the overlap
// carry or any synthesis buffer.
#pragma once
#include "vsyn_device.h"
#include "vsyn_host.h"
#include "vsyn_hpss.h"
#include "vsyn_wave.h"

#define RHY_THREADS 256
#define RHY_WAVES (RHY_THREADS / 64)
#define ONS_FT 16u         // frames of an onset workgroup: ONS_FT / RHY_WAVES per wave
#define ONS_MAX_DIM 256u
#define ONS_MAX_LAG 64u
#define PEAKS_MAX_WIN 4096u
#define TG_ILP 4u          // frames per thread: independent fma chains
#define TG_MIN_W 2u
#define TG_MAX_W 2048u
#define TG_FT_MAX 32u
#define TG_LDS_BUDGET (79u * 1024u)  // dynamic LDS of a tempogram workgroup wherever one tile of TG_ILP frames fits it: two per CU
#define TG_MAX_BLOCKS 128u           // blocks of tiles per segment, at most
#define RHY_FLT_MIN 1.17549435e-38f

// ------------------------------------------------------------------------------------------------
// A. onset strength
// ------------------------------------------------------------------------------------------------
typedef RowSeg OnsSeg;

struct OnsCtx {  // launch arguments
  const OnsSeg* seg;
  const float* rows;  // [rows][D]
  float* env;         // [rows]
  uint32_t D, lag, m, p;
};

__global__ void __launch_bounds__(RHY_THREADS) vsyn_onset_kernel(const OnsCtx A) {
  __shared__ uint32_t sR[RHY_WAVES][ONS_MAX_DIM];
  const OnsSeg sg = A.seg[blockIdx.y];
  const uint32_t F = sg.F, D = A.D, m = A.m, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t f0 = blockIdx.x * ONS_FT;
  if (f0 >= F) return;  // (workgroup-uniform)
  for (uint32_t q = 0; q < ONS_FT / RHY_WAVES; ++q) {
    const uint32_t f = f0 + q * RHY_WAVES + wave;
    const bool live = f < F && f >= A.p + A.lag;  // (wave-uniform) g - lag >= 0
    const float* cur = A.rows + (sg.off + (live ? f - A.p : 0u)) * D;
    const float* ref = A.rows + (sg.off + (live ? f - A.p - A.lag : 0u)) * D;
    if (live && m > 1u)
      for (uint32_t j = lane; j < D; j += 64u) sR[wave][j] = hpss_key(ref[j]);
    __syncthreads();
    double part = 0.0;
    if (live) {
      for (uint32_t j = lane; j < D; j += 64u) {
        float r;
        if (m > 1u) {
          const int32_t k0 = (int32_t)j - (int32_t)(m >> 1);
          uint32_t best = 0u;
          for (uint32_t k = 0; k < m; ++k) best = max(best, sR[wave][hpss_reflect(k0 + (int32_t)k, D)]);
          r = hpss_unkey(best);
        } else {
          r = ref[j];
        }
        const double d = (double)cur[j] - (double)r;
        part += d > 0.0 ? d : (d != d ? d : 0.0);
      }
      part = wave_sum(part);
    }
    if (f < F && lane == 0u) A.env[sg.off + f] = live ? (float)(part / (double)D) : 0.f;
    __syncthreads();  // the line is free for the next frame
  }
}

// ------------------------------------------------------------------------------------------------
// B. onset frames
// ------------------------------------------------------------------------------------------------
struct PeakSeg {
  uint64_t off;   // first value of the segment's envelope (and of its onset list)
  uint64_t woff;  // first ballot word
  uint32_t F, pre_max, post_max, pre_avg, post_avg, wait;  // F = 0: nothing to do
};

struct PeakCtx {  // launch arguments
  const PeakSeg* seg;
  const float* env;
  float* mm;        // [S][2] minimum, maximum
  uint32_t* bad;    // [S] a value is not finite
  uint64_t* cand;   // ballot words
  uint32_t* onsets;
  uint32_t* counts;   // [S]
  uint32_t* refused;  // [S] or NULL
  double delta;
  uint32_t normalize;
};

__global__ void __launch_bounds__(RHY_THREADS) vsyn_peaks_minmax_kernel(const PeakCtx A) {
  __shared__ uint32_t s_lo[RHY_WAVES], s_hi[RHY_WAVES];
  const uint32_t g = blockIdx.x, tid = threadIdx.x;
  const PeakSeg sg = A.seg[g];
  const float* x = A.env + sg.off;
  uint32_t lo = 0xFFFFFFFFu, hi = 0u;
  bool bad = false;
  for (uint32_t i = tid; i < sg.F; i += RHY_THREADS) {
    const float v = x[i];
    bad |= (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u;
    const uint32_t k = hpss_key(v);
    lo = min(lo, k);
    hi = max(hi, k);
  }
  wg_put(lo, s_lo, WaveMin());  // (one barrier for the two, and it is the flag's __syncthreads_or)
  wg_put(hi, s_hi, WaveMax());
  const int any = __syncthreads_or(bad ? 1 : 0);
  if (tid == 0u) {
    lo = wg_get<RHY_WAVES>(s_lo, WaveMin(), 0xFFFFFFFFu);
    hi = wg_get<RHY_WAVES>(s_hi, WaveMax(), 0u);
    A.mm[2u * g] = sg.F ? hpss_unkey(lo) : 0.f;
    A.mm[2u * g + 1u] = sg.F ? hpss_unkey(hi) : 0.f;
    A.bad[g] = any ? 1u : 0u;
  }
}

__global__ void __launch_bounds__(RHY_THREADS) vsyn_peaks_cand_kernel(const PeakCtx A) {
  const uint32_t g = blockIdx.y;
  const PeakSeg sg = A.seg[g];
  const uint32_t F = sg.F, n = blockIdx.x * RHY_THREADS + threadIdx.x;
  if ((n & ~63u) >= F) return;  // (wave-uniform) no word of this wave
  const float* x = A.env + sg.off;
  bool c = false;
  if (n < F && !A.bad[g]) {
    const float xn = x[n];
    const uint32_t a0 = n > sg.pre_max ? n - sg.pre_max : 0u, a1 = min(F, n + sg.post_max);
    c = true;
    for (uint32_t k = a0; k < a1; ++k) c &= !(x[k] > xn);
    if (c) {
      const double mn = (double)A.mm[2u * g], den = ((double)A.mm[2u * g + 1u] - mn) + (double)RHY_FLT_MIN;
      const uint32_t b0 = n > sg.pre_avg ? n - sg.pre_avg : 0u, b1 = min(F, n + sg.post_avg);
      double sum = 0.0;
      for (uint32_t k = b0; k < b1; ++k) sum += A.normalize ? ((double)x[k] - mn) / den : (double)x[k];
      const double un = A.normalize ? ((double)xn - mn) / den : (double)xn;
      c = un >= sum / (double)(b1 - b0) + A.delta;
    }
  }
  const uint64_t word = __ballot(c ? 1 : 0);
  if ((threadIdx.x & 63u) == 0u) A.cand[sg.woff + (n >> 6)] = word;
}

__global__ void __launch_bounds__(64) vsyn_peaks_walk_kernel(const PeakCtx A) {
  const uint32_t g = blockIdx.x, lane = threadIdx.x;
  const PeakSeg sg = A.seg[g];
  const uint32_t bad = A.bad[g];
  if (lane == 0u && A.refused) A.refused[g] = sg.F ? bad : 0u;
  uint32_t count = 0u, last = 0u;
  if (!bad) {
    const uint32_t words = (sg.F + 63u) >> 6;
    uint32_t* out = A.onsets + sg.off;
    for (uint32_t w0 = 0; w0 < words; w0 += 64u) {
      const uint64_t mine = w0 + lane < words ? A.cand[sg.woff + w0 + lane] : 0ull;
      if (__ballot(mine != 0ull) == 0ull) continue;  // (wave-uniform)
      const uint32_t nw = min(64u, words - w0);
      for (uint32_t w = 0; w < nw; ++w) {
        uint64_t word = shfl64(mine, (int)w);
        while (word) {  // (wave-uniform)
          const uint32_t n = ((w0 + w) << 6) + (uint32_t)__ffsll((unsigned long long)word) - 1u;
          word &= word - 1ull;
          if (count == 0u || n - last > sg.wait) {
            if (lane == 0u) out[count] = n;
            ++count;
            last = n;
          }
        }
      }
    }
  }
  if (lane == 0u) A.counts[g] = count;
}

// ------------------------------------------------------------------------------------------------
// C. tempogram
// ------------------------------------------------------------------------------------------------
struct TgSeg {
  uint64_t off;       // first value of the segment's envelope
  uint64_t row_off;   // first float of its (F', W) matrix
  uint64_t part_off;  // first double of its block sums [nb][W]
  uint64_t mean_off;  // first double of its mean
  uint32_t F, Fp, W, FT;
  uint32_t tpb, nb;   // tiles per block, blocks
  uint32_t win_off;   // its window, in floats from the windows' start
  uint32_t pad;
};

struct TgCtx {  // launch arguments
  const TgSeg* seg;
  const float* win;
  const float* env;
  float* rows;     // or NULL
  double* part;    // or NULL (no mean wanted)
  double* mean;
  uint32_t center, norm;
};

// rows per tile: the most (a multiple of TG_ILP, at most TG_FT_MAX) whose y, ac and block sums fit the LDS budget; TG_ILP always
__host__ __device__ __forceinline__ uint32_t tg_lds_bytes(uint32_t ft, uint32_t W) { return 8u * (2u * ft + 1u) * W; }
static inline uint32_t tg_tile(uint32_t W) {
  uint32_t ft = TG_FT_MAX;
  while (ft > TG_ILP && tg_lds_bytes(ft, W) > TG_LDS_BUDGET) ft -= TG_ILP;
  return ft;
}

// e_pad[t - w] of step C.1 for t in [-w, F + w)
__device__ __forceinline__ float tg_pad(const float* e, uint32_t F, uint32_t w, int64_t t) {
  if (t < 0) return (float)((double)(t + (int64_t)w) * ((double)e[0] / (double)w));
  if (t >= (int64_t)F) return (float)((double)((int64_t)w - 1 - (t - (int64_t)F)) * ((double)e[F - 1u] / (double)w));
  return e[t];
}

__global__ void __launch_bounds__(RHY_THREADS) vsyn_tempogram_kernel(const TgCtx A) {
  extern __shared__ double s_tg[];
  __shared__ uint64_t s_r[RHY_WAVES];
  __shared__ double s_mx[TG_FT_MAX];
  const TgSeg sg = A.seg[blockIdx.y];
  const uint32_t W = sg.W, FT = sg.FT, Fp = sg.Fp, tid = threadIdx.x;
  if (blockIdx.x >= sg.nb) return;  // (workgroup-uniform)
  double* s_y = s_tg;                        // [FT][W]
  double* s_ac = s_tg + (size_t)FT * W;      // [FT][W]
  double* s_g = s_tg + 2u * (size_t)FT * W;  // [W]
  const float* e = A.env + sg.off;
  const float* win = A.win + sg.win_off;
  const uint32_t w = A.center ? W / 2u : 0u;
  const uint32_t Lh = (W + 1u) / 2u;  // pairs of lags: l and W - 1 - l, l < Lh
  const uint32_t ntiles = (Fp + FT - 1u) / FT;
  const uint32_t t0 = blockIdx.x * sg.tpb, t1 = min(ntiles, t0 + sg.tpb);
  for (uint32_t l = tid; l < W; l += RHY_THREADS) s_g[l] = 0.0;
  for (uint32_t t = t0; t < t1; ++t) {
    const uint32_t f0 = t * FT, nf = min(FT, Fp - f0);
    // y of the tile's frames
    for (uint32_t u = tid; u < nf * W; u += RHY_THREADS) {
      const uint32_t f = u / W, n = u - f * W;
      s_y[u] = (double)win[n] * (double)tg_pad(e, sg.F, w, (int64_t)(f0 + f + n) - (int64_t)w);
    }
    __syncthreads();
    // ac[f][l]: an item is TG_ILP frames of one pair of lags
    const uint32_t groups = (nf + TG_ILP - 1u) / TG_ILP, items = groups * Lh;
    for (uint32_t q = tid; q < items; q += RHY_THREADS) {
      const uint32_t fg = q / Lh, l = q - fg * Lh, lb = W - 1u - l;
      const double* yf[TG_ILP];
      double acc[TG_ILP];
#pragma unroll
      for (uint32_t r = 0; r < TG_ILP; ++r) {
        const uint32_t f = fg * TG_ILP + r;
        yf[r] = s_y + (size_t)(f < nf ? f : 0u) * W;  // (an idle chain repeats frame 0 and is not stored)
        acc[r] = 0.0;
      }
      for (uint32_t n = 0; n + l < W; ++n) {
#pragma unroll
        for (uint32_t r = 0; r < TG_ILP; ++r) acc[r] = fma(yf[r][n], yf[r][n + l], acc[r]);
      }
#pragma unroll
      for (uint32_t r = 0; r < TG_ILP; ++r) {
        const uint32_t f = fg * TG_ILP + r;
        if (f < nf) s_ac[(size_t)f * W + l] = acc[r];
        acc[r] = 0.0;
      }
      if (lb > l) {
        for (uint32_t n = 0; n + lb < W; ++n) {
#pragma unroll
          for (uint32_t r = 0; r < TG_ILP; ++r) acc[r] = fma(yf[r][n], yf[r][n + lb], acc[r]);
        }
#pragma unroll
        for (uint32_t r = 0; r < TG_ILP; ++r) {
          const uint32_t f = fg * TG_ILP + r;
          if (f < nf) s_ac[(size_t)f * W + lb] = acc[r];
        }
      }
    }
    __syncthreads();
    // the largest |ac| of each frame: the bit images of |x| order as the values do, a NaN's above +Inf's
    if (A.norm) {
      for (uint32_t f = 0; f < nf; ++f) {
        uint64_t mx = 0ull;
        for (uint32_t l = tid; l < W; l += RHY_THREADS) {
          const uint64_t b = (uint64_t)__double_as_longlong(s_ac[(size_t)f * W + l]) & 0x7FFFFFFFFFFFFFFFull;
          mx = b > mx ? b : mx;
        }
        mx = wg_reduce_t0<RHY_WAVES>(mx, s_r, WaveMax(), 0ull);
        if (tid == 0u) s_mx[f] = __longlong_as_double((long long)mx);
        __syncthreads();
      }
    }
    // normalise, round, store, and add to the block's sums: a lag is one thread's, frames ascending
    for (uint32_t l = tid; l < W; l += RHY_THREADS) {
      double gs = s_g[l];
      for (uint32_t f = 0; f < nf; ++f) {
        double v = s_ac[(size_t)f * W + l];
        if (A.norm) {
          const double mx = s_mx[f];
          if (!(mx <= (double)RHY_FLT_MIN)) v /= mx;
        }
        const float o = (float)v;
        if (A.rows) A.rows[sg.row_off + (uint64_t)(f0 + f) * W + l] = o;
        gs += (double)o;
      }
      s_g[l] = gs;
    }
    __syncthreads();  // y and ac are free for the next tile
  }
  if (A.part)
    for (uint32_t l = tid; l < W; l += RHY_THREADS) A.part[sg.part_off + (uint64_t)blockIdx.x * W + l] = s_g[l];
}

__global__ void __launch_bounds__(RHY_THREADS) vsyn_tempogram_mean_kernel(const TgCtx A) {
  const TgSeg sg = A.seg[blockIdx.y];
  const uint32_t l = blockIdx.x * RHY_THREADS + threadIdx.x;
  if (l >= sg.W) return;
  double s = 0.0;
  for (uint32_t b = 0; b < sg.nb; ++b) s += A.part[sg.part_off + (uint64_t)b * sg.W + l];
  A.mean[sg.mean_off + l] = sg.Fp ? s / (double)sg.Fp : __longlong_as_double(0x7FF8000000000000ll);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct RhythmWs {  // the stage's buffers
  TableUpload tab_onset, tab_peaks, tab_tg;
  bool lds_set = false;  // the tempogram kernel's dynamic-LDS limit is raised on this handle's device
  DevBuf<float> mm;
  DevBuf<uint32_t> bad;
  DevBuf<uint64_t> cand;
  DevBuf<double> part;
  // host form: the envelope, and the selected output on its way to the host
  DevBuf<float> env, tg;
  DevBuf<uint32_t> onsets, counts, refused;
  DevBuf<double> mean;
};

static inline int onset_check(const vsyn_onset_spec* p, const char** err) {
  if (!p) return fail(err, VSYN_ERR_INVALID, "onset spec is NULL");
  if (p->options & ~(uint32_t)VSYN_ONSET_CENTER) return fail(err, VSYN_ERR_INVALID, "unknown onset options 0x%x", p->options);
  if (p->lag < 1 || p->lag > ONS_MAX_LAG) return fail(err, VSYN_ERR_INVALID, "onset lag %u outside [1, %u]", p->lag, ONS_MAX_LAG);
  if (p->max_size < 1 || p->max_size > 64u) return fail(err, VSYN_ERR_INVALID, "onset max_size %u outside [1, 64]", p->max_size);
  if (p->n_fft < 1 || p->hop_length < 1) return fail(err, VSYN_ERR_INVALID, "onset n_fft and hop_length must be >= 1");
  return VSYN_OK;
}

static inline int rhythm_check_segs(uint32_t S, const uint64_t* seg_rows, const char** err) { return rows_check_segs(S, seg_rows, 0x3FFFFFFFull, err); }

static inline int onset_check_call(const vsyn_onset_spec* p, uint32_t D, uint32_t S, const uint64_t* seg_rows, const char** err) {
  if (int rc = onset_check(p, err)) return rc;
  if (D < 1 || D > ONS_MAX_DIM) return fail(err, VSYN_ERR_INVALID, "onset strength: dim %u outside [1, %u]", D, ONS_MAX_DIM);
  return rhythm_check_segs(S, seg_rows, err);
}

// Stage A on stream s. Caller holds the handle's lock and has run onset_check_call.
static inline int onset_launch(RhythmWs& ws, int device, const vsyn_onset_spec* p, uint32_t D, uint32_t S, const uint64_t* seg_rows,
                               const float* d_rows, float* d_env, hipStream_t s, const char** err) {
  std::vector<uint8_t> tab(sizeof(OnsSeg) * (size_t)S);
  OnsSeg* seg = (OnsSeg*)tab.data();
  const uint64_t f_max = row_segs_fill(seg, S, seg_rows, nullptr, 1u).f_max;
  if (f_max == 0) return VSYN_OK;
  HIPCHK(hipSetDevice(device));
  if (int rc = ws.tab_onset.upload(tab, s, err)) return rc;
  OnsCtx A;
  A.seg = (const OnsSeg*)ws.tab_onset.dev.p;
  A.rows = d_rows;
  A.env = d_env;
  A.D = D;
  A.lag = p->lag;
  A.m = p->max_size;
  A.p = (p->options & VSYN_ONSET_CENTER) ? (uint32_t)(p->n_fft / (2ull * p->hop_length)) : 0u;
  VSYN_LAUNCH(vsyn_onset_kernel, dim3((uint32_t)((f_max + ONS_FT - 1u) / ONS_FT), S), dim3(RHY_THREADS), 0, s, A);
  return VSYN_OK;
}

// w(t) of step B.1; false: above PEAKS_MAX_WIN
static inline bool peaks_frames(double t, uint32_t rate, uint32_t hop, uint32_t add, uint32_t* out) {
  const double v = floor((t * (double)rate) / (double)hop) + (double)add;
  if (!(v <= (double)PEAKS_MAX_WIN)) return false;
  *out = (uint32_t)v;
  return true;
}

static inline int peaks_check(const vsyn_onset_peaks* p, const char** err) {
  if (!p) return fail(err, VSYN_ERR_INVALID, "peaks spec is NULL");
  if (p->options & ~(uint32_t)VSYN_PEAKS_NORMALIZE) return fail(err, VSYN_ERR_INVALID, "unknown peaks options 0x%x", p->options);
  if (p->hop_length < 1) return fail(err, VSYN_ERR_INVALID, "peaks hop_length must be >= 1");
  const double t[5] = {p->pre_max, p->post_max, p->pre_avg, p->post_avg, p->wait};
  for (int i = 0; i < 5; ++i)
    if (!std::isfinite(t[i]) || t[i] < 0.0) return fail(err, VSYN_ERR_INVALID, "peaks: the window times must be finite and >= 0");
  if (!std::isfinite(p->delta)) return fail(err, VSYN_ERR_INVALID, "peaks: delta must be finite");
  return VSYN_OK;
}

// out[5]: pre_max, post_max, pre_avg, post_avg, wait in frames
static inline int peaks_windows(const vsyn_onset_peaks* p, uint32_t rate, uint32_t* out, const char** err) {
  if (!peaks_frames(p->pre_max, rate, p->hop_length, 0u, out) || !peaks_frames(p->post_max, rate, p->hop_length, 1u, out + 1) ||
      !peaks_frames(p->pre_avg, rate, p->hop_length, 0u, out + 2) || !peaks_frames(p->post_avg, rate, p->hop_length, 1u, out + 3) ||
      !peaks_frames(p->wait, rate, p->hop_length, 0u, out + 4))
    return fail(err, VSYN_ERR_INVALID, "peaks: a window exceeds %u frames at rate %u", PEAKS_MAX_WIN, rate);
  return VSYN_OK;
}

static inline int peaks_check_call(const vsyn_onset_peaks* p, uint32_t S, const uint64_t* seg_rows, const uint32_t* rates, const char** err) {
  if (int rc = peaks_check(p, err)) return rc;
  if (int rc = rhythm_check_segs(S, seg_rows, err)) return rc;
  if (S && !rates) return fail(err, VSYN_ERR_INVALID, "sample_rates is NULL");
  for (uint32_t g = 0; g < S; ++g) {
    uint32_t w[5];
    if (rates[g])
      if (int rc = peaks_windows(p, rates[g], w, err)) return rc;
  }
  return VSYN_OK;
}

// Stage B on stream s. Caller holds the handle's lock and has run peaks_check_call.
static inline int peaks_launch(RhythmWs& ws, int device, const vsyn_onset_peaks* p, uint32_t S, const uint64_t* seg_rows, const uint32_t* rates,
                               const float* d_env, uint32_t* d_onsets, uint32_t* d_counts, uint32_t* d_refused, hipStream_t s, const char** err) {
  if (S == 0) return VSYN_OK;
  std::vector<uint8_t> tab(sizeof(PeakSeg) * (size_t)S);
  PeakSeg* seg = (PeakSeg*)tab.data();
  uint64_t off = 0, words = 0, f_max = 0;
  for (uint32_t g = 0; g < S; ++g) {
    uint32_t w[5] = {0u, 1u, 0u, 1u, 0u};
    if (rates[g]) (void)peaks_windows(p, rates[g], w, nullptr);
    const uint32_t F = rates[g] ? (uint32_t)seg_rows[g] : 0u;
    seg[g] = PeakSeg{off, words, F, w[0], w[1], w[2], w[3], w[4]};
    off += seg_rows[g];
    words += (F + 63u) / 64u;
    f_max = std::max<uint64_t>(f_max, F);
  }
  HIPCHK(hipSetDevice(device));
  HIPCHK(ws.mm.ensure(2u * (size_t)S));
  HIPCHK(ws.bad.ensure(S));
  HIPCHK(ws.cand.ensure(words + 1u));
  if (int rc = ws.tab_peaks.upload(tab, s, err)) return rc;
  PeakCtx A;
  A.seg = (const PeakSeg*)ws.tab_peaks.dev.p;
  A.env = d_env;
  A.mm = ws.mm.p;
  A.bad = ws.bad.p;
  A.cand = ws.cand.p;
  A.onsets = d_onsets;
  A.counts = d_counts;
  A.refused = d_refused;
  A.delta = p->delta;
  A.normalize = (p->options & VSYN_PEAKS_NORMALIZE) ? 1u : 0u;
  VSYN_LAUNCH(vsyn_peaks_minmax_kernel, dim3(S), dim3(RHY_THREADS), 0, s, A);
  if (f_max) {
    VSYN_LAUNCH(vsyn_peaks_cand_kernel, dim3((uint32_t)((f_max + RHY_THREADS - 1u) / RHY_THREADS), S), dim3(RHY_THREADS), 0, s, A);
  }
  VSYN_LAUNCH(vsyn_peaks_walk_kernel, dim3(S), dim3(64), 0, s, A);
  return VSYN_OK;
}

static inline int tg_check(const vsyn_tempogram_spec* p, const char** err) {
  if (!p) return fail(err, VSYN_ERR_INVALID, "tempogram spec is NULL");
  if (p->options & ~(uint32_t)(VSYN_TG_CENTER | VSYN_TG_NORM_INF)) return fail(err, VSYN_ERR_INVALID, "unknown tempogram options 0x%x", p->options);
  if (p->reserved) return fail(err, VSYN_ERR_INVALID, "tempogram: reserved must be 0");
  if (p->hop_length < 1) return fail(err, VSYN_ERR_INVALID, "tempogram hop_length must be >= 1");
  if (p->win_length) {
    if (p->win_length < TG_MIN_W || p->win_length > TG_MAX_W)
      return fail(err, VSYN_ERR_INVALID, "tempogram win_length %u outside [%u, %u]", p->win_length, TG_MIN_W, TG_MAX_W);
  } else if (!std::isfinite(p->ac_size) || !(p->ac_size > 0.0)) {
    return fail(err, VSYN_ERR_INVALID, "tempogram ac_size must be finite and > 0");
  }
  return VSYN_OK;
}

// W for one rate; 0: outside [TG_MIN_W, TG_MAX_W]
static inline uint32_t tg_win_length(const vsyn_tempogram_spec* p, uint32_t rate) {
  if (p->win_length) return p->win_length;
  const double v = floor(p->ac_size * (double)rate / (double)p->hop_length);
  return v >= (double)TG_MIN_W && v <= (double)TG_MAX_W ? (uint32_t)v : 0u;
}

static inline uint64_t tg_rows(bool center, uint32_t W, uint64_t F) { return center ? F : (F >= W ? F - W + 1u : 0u); }

static inline int tg_check_call(const vsyn_tempogram_spec* p, uint32_t S, const uint64_t* seg_rows, const uint32_t* rates, const char** err) {
  if (int rc = tg_check(p, err)) return rc;
  if (int rc = rhythm_check_segs(S, seg_rows, err)) return rc;
  if (!p->win_length) {
    if (S && !rates) return fail(err, VSYN_ERR_INVALID, "sample_rates is NULL");
    for (uint32_t g = 0; g < S; ++g)
      if (rates[g] && !tg_win_length(p, rates[g]))  // (a rate of 0 skips the segment)
        return fail(err, VSYN_ERR_INVALID, "segment %u: floor(ac_size * %u / hop_length) outside [%u, %u]", g, rates[g], TG_MIN_W, TG_MAX_W);
  }
  return VSYN_OK;
}

// Stage C on stream s: rows (d_rows != NULL), mean (d_mean != NULL) or both. Caller holds the handle's lock and has run tg_check_call.
static inline int tg_launch(RhythmWs& ws, int device, const vsyn_tempogram_spec* p, uint32_t S, const uint64_t* seg_rows, const uint32_t* rates,
                            const float* d_env, float* d_rows, double* d_mean, hipStream_t s, const char** err) {
  if (S == 0) return VSYN_OK;
  const bool center = (p->options & VSYN_TG_CENTER) != 0;
  const size_t seg_bytes = sizeof(TgSeg) * (size_t)S;
  std::vector<uint8_t> tab(seg_bytes);
  std::vector<std::pair<uint32_t, uint32_t>> wins;  // (W, offset in floats)
  uint32_t win_floats = 0, nb_max = 0, w_max = 0, lds = 0;
  uint64_t off = 0, row_off = 0, part_off = 0, mean_off = 0;
  for (uint32_t g = 0; g < S; ++g) {
    TgSeg sg;
    memset(&sg, 0, sizeof(sg));
    sg.W = p->win_length ? p->win_length : rates[g] ? tg_win_length(p, rates[g]) : 0u;  // 0: skipped, neither rows nor mean
    sg.F = sg.W ? (uint32_t)seg_rows[g] : 0u;
    sg.Fp = (uint32_t)tg_rows(center, sg.W, sg.F);
    sg.FT = tg_tile(sg.W);
    const uint32_t ntiles = (sg.Fp + sg.FT - 1u) / sg.FT;
    sg.tpb = std::max(1u, (ntiles + TG_MAX_BLOCKS - 1u) / TG_MAX_BLOCKS);
    sg.nb = (ntiles + sg.tpb - 1u) / sg.tpb;
    sg.off = off;
    sg.row_off = row_off;
    sg.part_off = part_off;
    sg.mean_off = mean_off;
    sg.win_off = table_slot(wins, sg.W, &win_floats, sg.W);
    memcpy(tab.data() + sizeof(TgSeg) * (size_t)g, &sg, sizeof(sg));
    off += seg_rows[g];
    row_off += (uint64_t)sg.Fp * sg.W;
    part_off += (uint64_t)sg.nb * sg.W;
    mean_off += sg.W;
    nb_max = std::max(nb_max, sg.nb);
    w_max = std::max(w_max, sg.W);
    lds = std::max(lds, tg_lds_bytes(sg.FT, sg.W));
  }
  tab.resize(seg_bytes + sizeof(float) * (size_t)win_floats);
  float* win = (float*)(tab.data() + seg_bytes);
  for (const auto& wk : wins)
    for (uint32_t n = 0; n < wk.first; ++n) win[wk.second + n] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)n / (double)wk.first));
  HIPCHK(hipSetDevice(device));
  if (int rc = raise_lds_once(ws.lds_set, {{(const void*)vsyn_tempogram_kernel, tg_lds_bytes(TG_ILP, TG_MAX_W)}}, err)) return rc;
  if (d_mean) HIPCHK(ws.part.ensure(part_off + 1u));
  if (int rc = ws.tab_tg.upload(tab, s, err)) return rc;
  TgCtx A;
  A.seg = (const TgSeg*)ws.tab_tg.dev.p;
  A.win = (const float*)(ws.tab_tg.dev.p + seg_bytes);
  A.env = d_env;
  A.rows = d_rows;
  A.part = d_mean ? ws.part.p : nullptr;
  A.mean = d_mean;
  A.center = center ? 1u : 0u;
  A.norm = (p->options & VSYN_TG_NORM_INF) ? 1u : 0u;
  if (nb_max) {
    VSYN_LAUNCH(vsyn_tempogram_kernel, dim3(nb_max, S), dim3(RHY_THREADS), lds, s, A);
  }
  if (d_mean && w_max) {  // (w_max = 0: every segment is skipped)
    VSYN_LAUNCH(vsyn_tempogram_mean_kernel, dim3((w_max + RHY_THREADS - 1u) / RHY_THREADS, S), dim3(RHY_THREADS), 0, s, A);
  }
  return VSYN_OK;
}

// Step C.5 for one mean.
static inline int tempo_from_mean(const vsyn_tempo_spec* t, const double* g, uint32_t W, uint32_t rate, uint32_t hop, double* bpm_out,
                                  uint32_t* lag_out, const char** err) {
  if (!t || !g || !bpm_out) return fail(err, VSYN_ERR_INVALID, "tempo: NULL argument");
  if (!std::isfinite(t->start_bpm) || !(t->start_bpm > 0.0) || !std::isfinite(t->std_bpm) || !(t->std_bpm > 0.0))
    return fail(err, VSYN_ERR_INVALID, "tempo: start_bpm and std_bpm must be finite and > 0");
  if (!std::isfinite(t->max_tempo) || t->max_tempo < 0.0) return fail(err, VSYN_ERR_INVALID, "tempo: max_tempo must be finite and >= 0 (0: no cap)");
  if (W < TG_MIN_W || W > TG_MAX_W || rate < 1 || hop < 1) return fail(err, VSYN_ERR_INVALID, "tempo: win_length outside [2, 2048], or a rate or hop_length of 0");
  for (uint32_t l = 0; l < W; ++l)
    if (!std::isfinite(g[l]) || g[l] < -1e-6) return fail(err, VSYN_ERR_INVALID, "tempo: the mean tempogram is not finite, or below -1e-6, at lag %u", l);
  const double inf = std::numeric_limits<double>::infinity();
  uint32_t first = 0;  // the first lag slower than max_tempo; none (or no cap): 0
  if (t->max_tempo > 0.0)
    for (uint32_t l = 1; l < W; ++l)
      if (60.0 * (double)rate / ((double)hop * (double)l) < t->max_tempo) {
        first = l;
        break;
      }
  const double l2s = log2(t->start_bpm);
  uint32_t best = 0;
  double best_v = -inf;
  for (uint32_t l = 0; l < W; ++l) {
    double prior = -inf;
    if (l >= first && l > 0u) {
      const double z = (log2(60.0 * (double)rate / ((double)hop * (double)l)) - l2s) / t->std_bpm;
      prior = -0.5 * (z * z);
    }
    const double v = log1p(1e6 * g[l]) + prior;
    if (v > best_v) {
      best_v = v;
      best = l;
    }
  }
  *bpm_out = best ? 60.0 * (double)rate / ((double)hop * (double)best) : inf;
  if (lag_out) *lag_out = best;
  return VSYN_OK;
}

// ------------------------------------------------------------------------------------------------
// the stages behind the rows of a host chain (vsyn_pcm_chain_rhythm_host)
// ------------------------------------------------------------------------------------------------
static inline uint32_t rhythm_cols(const vsyn_rhythm_spec* R) {
  return R->output == VSYN_RHYTHM_TEMPOGRAM ? R->tempogram.win_length : R->output == VSYN_RHYTHM_TEMPO_MEAN ? 2u : 1u;
}

// The checks that need no rows: the selector, the specs it reads, and their agreement with the spectral spec.
static inline int rhythm_check(const vsyn_rhythm_spec* R, uint32_t n_fft, uint32_t hop, bool center, uint32_t D, const char** err) {
  if (R->output > VSYN_RHYTHM_TEMPO_MEAN || R->reserved) return fail(err, VSYN_ERR_INVALID, "rhythm: unknown output %u", R->output);
  if (int rc = onset_check(&R->onset, err)) return rc;
  if (R->onset.n_fft != n_fft || R->onset.hop_length != hop || ((R->onset.options & VSYN_ONSET_CENTER) != 0) != center)
    return fail(err, VSYN_ERR_INVALID, "rhythm: the onset spec's n_fft, hop_length and centring must be the spectral spec's");
  if (D < 1 || D > ONS_MAX_DIM) return fail(err, VSYN_ERR_INVALID, "onset strength takes rows of 1 to %u columns, this kind has %u", ONS_MAX_DIM, D);
  if (R->output == VSYN_RHYTHM_ONSETS) {
    if (int rc = peaks_check(&R->peaks, err)) return rc;
    if (R->peaks.hop_length != hop) return fail(err, VSYN_ERR_INVALID, "rhythm: the peak picker's hop_length must be the spectral spec's");
  }
  if (R->output >= VSYN_RHYTHM_TEMPOGRAM) {
    if (int rc = tg_check(&R->tempogram, err)) return rc;
    if (R->tempogram.hop_length != hop) return fail(err, VSYN_ERR_INVALID, "rhythm: the tempogram's hop_length must be the spectral spec's");
    if (R->output == VSYN_RHYTHM_TEMPOGRAM && !R->tempogram.win_length)
      return fail(err, VSYN_ERR_INVALID, "rhythm: tempogram rows need a win_length (one width for the whole call)");
  }
  return VSYN_OK;
}

// The rhythm stages on stream s over the rows at cur ([total][D], seg_rows[S] rows a segment, rates[S] the rows' rates with 0 for a
// skipped segment), the selected output into the host's words (cap of them), seg_rows rewritten as that output's rows, refused[S]
// (may be NULL) 1 for an envelope that is not finite (onsets), 2 for a window length outside [2, 2048] (tempo mean). Waits for the
// stream where the output has to be packed. Caller holds the handle's lock and has run rhythm_check.
static inline int rhythm_rows_out(RhythmWs& ws, int device, const vsyn_rhythm_spec* R, uint32_t D, uint32_t S, const uint32_t* rates, uint64_t* seg_rows,
                                  uint64_t total, const float* cur, float* words, uint64_t cap, uint32_t* refused_out, hipStream_t s, const char** err) {
  const std::vector<uint64_t> F(seg_rows, seg_rows + S);
  if (refused_out) memset(refused_out, 0, sizeof(uint32_t) * S);
  if (int rc = rhythm_check_segs(S, F.data(), err)) return rc;
  HIPCHK(hipSetDevice(device));
  HIPCHK(ws.env.ensure(total + 1));
  if (int rc = onset_launch(ws, device, &R->onset, D, S, F.data(), cur, ws.env.p, s, err)) return rc;
  const char* small = "rows buffer too small: %llu words needed";
  if (R->output == VSYN_RHYTHM_ENVELOPE) {
    if (total > cap) return fail(err, VSYN_ERR_INVALID, small, (unsigned long long)total);
    HIPCHK(hipMemcpyAsync(words, ws.env.p, sizeof(float) * total, hipMemcpyDeviceToHost, s));
    return VSYN_OK;
  }
  if (R->output == VSYN_RHYTHM_ONSETS) {
    if (total > cap) return fail(err, VSYN_ERR_INVALID, small, (unsigned long long)total);
    if (int rc = peaks_check_call(&R->peaks, S, F.data(), rates, err)) return rc;
    HIPCHK(ws.onsets.ensure(total + 1));
    HIPCHK(ws.counts.ensure(S));
    HIPCHK(ws.refused.ensure(S));
    if (int rc = peaks_launch(ws, device, &R->peaks, S, F.data(), rates, ws.env.p, ws.onsets.p, ws.counts.p, ws.refused.p, s, err)) return rc;
    std::vector<uint32_t> all(total), counts(S), refused(S);
    HIPCHK(hipMemcpyAsync(all.data(), ws.onsets.p, sizeof(uint32_t) * total, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(counts.data(), ws.counts.p, sizeof(uint32_t) * S, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(refused.data(), ws.refused.p, sizeof(uint32_t) * S, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    uint64_t off = 0, o = 0;
    for (uint32_t g = 0; g < S; ++g) {  // (a count never exceeds the segment's frames)
      memcpy(words + o, all.data() + off, sizeof(uint32_t) * counts[g]);
      off += F[g];
      o += counts[g];
      seg_rows[g] = counts[g];
      if (refused_out) refused_out[g] = refused[g] ? 1u : 0u;
    }
    return VSYN_OK;
  }
  const bool center = (R->tempogram.options & VSYN_TG_CENTER) != 0;
  if (R->output == VSYN_RHYTHM_TEMPOGRAM) {
    const uint32_t W = R->tempogram.win_length;
    uint64_t need = 0;
    for (uint32_t g = 0; g < S; ++g) need += tg_rows(center, W, F[g]) * W;
    if (need > cap) return fail(err, VSYN_ERR_INVALID, small, (unsigned long long)need);
    HIPCHK(ws.tg.ensure(need + 1));
    if (int rc = tg_launch(ws, device, &R->tempogram, S, F.data(), rates, ws.env.p, ws.tg.p, nullptr, s, err)) return rc;
    if (need) HIPCHK(hipMemcpyAsync(words, ws.tg.p, sizeof(float) * need, hipMemcpyDeviceToHost, s));
    for (uint32_t g = 0; g < S; ++g) seg_rows[g] = tg_rows(center, W, F[g]);
    return VSYN_OK;
  }
  // the mean: W doubles a segment, then its rate as a double, two words each
  std::vector<uint32_t> r(rates, rates + S), Wg(S);
  uint64_t nm = 0, need = 0;
  for (uint32_t g = 0; g < S; ++g) {
    if (!F[g]) r[g] = 0u;  // nothing to average
    Wg[g] = r[g] ? tg_win_length(&R->tempogram, r[g]) : 0u;
    if (r[g] && !Wg[g]) {
      if (refused_out) refused_out[g] = 2u;
      r[g] = 0u;
    }
    nm += Wg[g];
    need += Wg[g] ? 2u * ((uint64_t)Wg[g] + 1u) : 0u;
  }
  if (need > cap) return fail(err, VSYN_ERR_INVALID, small, (unsigned long long)need);
  // (with a win_length the rates are not read: a skipped segment is one of no frames)
  std::vector<uint64_t> Fr(F);
  for (uint32_t g = 0; g < S; ++g)
    if (!r[g]) Fr[g] = 0;
  HIPCHK(ws.mean.ensure(nm + 1));
  if (R->tempogram.win_length) {  // every segment has the call's W on the device, the skipped ones as F' = 0: the layout is S W
    HIPCHK(ws.mean.ensure((uint64_t)S * R->tempogram.win_length + 1));
  }
  if (int rc = tg_launch(ws, device, &R->tempogram, S, Fr.data(), r.data(), ws.env.p, nullptr, ws.mean.p, s, err)) return rc;
  const uint64_t on_dev = R->tempogram.win_length ? (uint64_t)S * R->tempogram.win_length : nm;
  std::vector<double> m(on_dev);
  if (on_dev) HIPCHK(hipMemcpyAsync(m.data(), ws.mean.p, sizeof(double) * on_dev, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  uint64_t off = 0, o = 0;
  for (uint32_t g = 0; g < S; ++g) {
    const uint32_t Wd = R->tempogram.win_length ? R->tempogram.win_length : Wg[g];  // what the segment takes of m
    if (Wg[g]) {
      memcpy(words + o, m.data() + off, sizeof(double) * Wg[g]);
      const double rate = (double)r[g];
      memcpy(words + o + 2u * (uint64_t)Wg[g], &rate, sizeof(double));
      o += 2u * ((uint64_t)Wg[g] + 1u);
    }
    seg_rows[g] = Wg[g] ? Wg[g] + 1u : 0u;
    off += Wd;
  }
  return VSYN_OK;
}
