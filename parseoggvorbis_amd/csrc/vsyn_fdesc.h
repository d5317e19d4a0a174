// vsyn_fdesc.h — frame descriptors: per frame rms, zero-crossing rate, spectral centroid, bandwidth, roll-off and flatness, from
// planar float32 PCM already on the device. Semantics: include/vorbis_synth_hip.h, "frame descriptors".
//
// Three kernels on one stream (the table — per-segment rates, float64 twiddles, float32 window — is built on the host per call):
//   1. vsyn_fdesc_offsets_kernel  one workgroup: per segment its frame count (spec_num_frames) and the exclusive row scan seg_off[S+1]:
//                                 frames_offsets (vsyn_frames.h).
//   2. vsyn_fdesc_kernel<TWL>     grid (tile of FT frames, segment), 256 threads. Dynamic LDS, declared 16-byte aligned, in this order:
//                                   twiddles (cos, sin)[n_fft] float64, TWL only
//                                   S[FT][NB] float64, NB = n_fft / 2 + 1: the magnitudes of the tile's frames
//                                   26 words of 8 bytes for the reductions
//                                   window[n_fft] float32
//                                   the tile's span of the mono signal as float32 (the downmix is done while loading, zeros outside
//                                   [0, T); hop > n_fft: the frames back to back): frames_tile_head / frames_tile_derive / frames_tile_stage
//                                   (vsyn_frames.h), which also write the tile's flag word.
//                                 DFT: the tile's frames are taken in groups of FDESC_ILP, and the (group, bin) items are dealt to
//                                 the threads in order, bin fastest. A thread owns its bin k for the frames of its group and walks
//                                 j = 0 .. n_fft - 1: window[j] and each frame's y[j] are one address per wave (broadcast reads),
//                                 widened to float64 and multiplied (exact); one twiddle read serves the group's frames; re and im
//                                 of every (frame, bin) are ONE fma chain each with j ascending, whatever the tile, the group and the
//                                 thread; the twiddle index (j k) mod n_fft is walked by adding k and subtracting n_fft once when it
//                                 is reached.
//                                 TWL = true reads the twiddles from LDS, TWL = false from the table in global memory (every workgroup
//                                 re-reads the same 16 n_fft bytes: L2). Both read the same table: the bits do not depend on the path.
//                                 Then per frame, by the whole workgroup: the ordered sums below, the roll-off bin by an integer
//                                 minimum through the wave and the four waves (vsyn_wave.h), the zero-crossing count by an integer
//                                 sum, and thread 0 writes the row. No atomics.
//                                 The workgroup also looks at every sample of its share of the segment for an Inf or a NaN
//                                 (trim_not_finite) and stores one flag word per tile.
//   3. vsyn_fdesc_finish_kernel   one workgroup per segment: a segment with a flagged tile is refused: its rows become NaN and its
//                                 word of the refused array 1 (frames_finish).
// Order of the sums over the bins: with K = ceil(NB / 256), thread t owns the bins t K .. min((t + 1) K, NB) - 1 and adds its terms in
// ascending order from 0.0 (its total). The totals go through wg_sum_scan (vsyn_wave.h; the order is DESIGN.md 6t: the wave scan over
// the lane offsets 1, 2, .. 32, a wave's offset the earlier waves' totals in ascending order, a sum over all bins ((w0 + w1) + w2) + w3 of
// the four waves' totals); and c_k = (wave offset + the exclusive lane prefix) + S[first] + .. + S[k], added left to right. A = c_(NB-1). The
// frame's energy (rms) is summed the same way over the samples, K = ceil(n_fft / 256). A function of n_fft alone.
// LDS budget: FDESC_LDS_BUDGET = 79 KiB (80,896 B) of dynamic LDS, so that two workgroups share a CU's 160 KiB beside the
// static LDS of __syncthreads_or; with the twiddles in LDS one frame takes 28 n_fft + 216 bytes, which fits up to n_fft = 2881. Above that the twiddles
// stay in global memory and the workgroup may take FDESC_LDS_WIDE = 156 KiB (159,744 B), one workgroup per CU: one frame at
// n_fft = 8192 takes 8 * (4097 + 26) + 4 * 8192 + 4 * 8192 = 98,520 B. FT is the most frames (at most 64) whose image fits the budget.
// Nothing here reads or writes stream state, the overlap carry or any synthesis buffer; the PCM is only read.
#pragma once
#include "vsyn_device.h"
#include "vsyn_frames.h"
#include "vsyn_host.h"
#include "vsyn_pitch.h"  // pitch_wg_min, PITCH_NONE
#include "vsyn_trim.h"

#define FDESC_THREADS 256
static_assert(FDESC_THREADS == FRAMES_THREADS, "the shared framing helpers stride by the workgroup's size");
#define FDESC_WAVES (FDESC_THREADS / 64)
#define FDESC_ILP 4u                         // frames per thread and twiddle read: 8 independent fma chains
#define FDESC_FT_MAX 64u                     // frames per workgroup, at most
#define FDESC_LDS_BUDGET (79u * 1024u)       // dynamic LDS of a workgroup, twiddles in LDS: two workgroups fit a CU
#define FDESC_LDS_WIDE (156u * 1024u)        // dynamic LDS of a workgroup, twiddles in global memory: one workgroup per CU
#define FDESC_COLS 6u
#define FDESC_TINY 1.1754944e-38             // step 6: below this sum of magnitudes the centroid and the bandwidth are 0
#define FDESC_MIN_FFT 16u
#define FDESC_SUMS 5u                        // sums of the first ordered pass: S, f S, P, ln P, y^2
#define FDESC_WORDS 26u                      // 8-byte words of the reductions in the image: the sums' waves, A, the integer minima, one spare

struct FdescCtx {  // launch arguments
  const double* sr;        // [S] the segment's rate; 0 skips the segment
  const double2* tw;       // [n_fft] (cos, sin)(2 pi m / n_fft)
  const float* win;        // [n_fft]
  const float* pcm;
  uint64_t plane;
  uint32_t C, S;
  const uint32_t* frames;  // PCM frames per segment (caller's, or the resampler's), or
  const SegInfo* si;       // the last submit's SegInfo (total_emit)
  uint32_t N, H, FT;       // n_fft, hop_length, frames per workgroup
  uint32_t center;
  uint32_t tiles;          // workgroups per segment (grid.x): the flags' stride
  double roll, zthr, amin;
  uint32_t* segF;          // [S] frames
  uint64_t* segoff;        // [S+1]
  uint32_t* flags;         // [S][tiles] a sample of the tile's share is not finite
  uint32_t* refused;       // [S]
  float* rows;             // [segoff[S]][6]
};

__global__ void __launch_bounds__(FDESC_THREADS) vsyn_fdesc_offsets_kernel(const FdescCtx A) {
  frames_offsets(A, A.N, [&](uint32_t g) { return A.sr[g] == 0.0; });
}

// Bin k of NR frames a tile step apart (z0: the first one's samples): S into out[0], out[NB], .. One twiddle read serves the NR
// frames; every (frame, bin) is still ONE fma chain per component with j ascending.
template <bool TWL, uint32_t NR>
__device__ __forceinline__ void fdesc_dft(const double2* s_tw, const double2* g_tw, const float* s_win, const float* z0, uint32_t fstep,
                                          uint32_t N, uint32_t k, double* out, uint32_t NB) {
  double re[NR], im[NR];
#pragma unroll
  for (uint32_t r = 0; r < NR; ++r) re[r] = im[r] = 0.0;
  uint32_t idx = 0u;
#pragma unroll 2
  for (uint32_t j = 0; j < N; ++j) {
    const double w = (double)s_win[j];
    const double2 cs = TWL ? s_tw[idx] : g_tw[idx];
    idx += k;  // (k <= n_fft / 2: one subtraction brings it back below n_fft)
    if (idx >= N) idx -= N;
#pragma unroll
    for (uint32_t r = 0; r < NR; ++r) {
      const double v = w * (double)z0[(size_t)r * fstep + j];  // (exact: two float32 factors)
      re[r] = fma(v, cs.x, re[r]);
      im[r] = fma(v, cs.y, im[r]);
    }
  }
#pragma unroll
  for (uint32_t r = 0; r < NR; ++r) out[(size_t)r * NB] = sqrt(fma(re[r], re[r], im[r] * im[r]));
}

template <bool TWL>
__global__ void __launch_bounds__(FDESC_THREADS) vsyn_fdesc_kernel(const FdescCtx A) {
  extern __shared__ __attribute__((aligned(16))) double s_fdesc[];
  const uint32_t g = blockIdx.y, tid = threadIdx.x;
  const double sr = A.sr[g];
  FramesTile t;
  if (frames_tile_head(A, sr == 0.0, t)) return frames_tile_idle(t);
  frames_tile_derive(A, A.N, t);
  const uint32_t N = A.N, H = A.H, NB = N / 2u + 1u;
  const double2* s_tw = (const double2*)s_fdesc;  // (first: the image is declared 16-byte aligned, for the 16-byte twiddle reads)
  double* s_S = s_fdesc + (TWL ? 2u * (size_t)N : 0u);
  double* s_w = s_S + (size_t)A.FT * NB;  // the reductions' words
  double* s_a = s_w + FDESC_SUMS * FDESC_WAVES;
  uint64_t* s_r = (uint64_t*)(s_a + 1);
  float* s_win = (float*)(s_w + FDESC_WORDS);
  float* s_y = s_win + N;
  if (t.nf) {
    if (TWL)
      for (uint32_t u = tid; u < N; u += FDESC_THREADS) ((double2*)s_tw)[u] = A.tw[u];
    for (uint32_t u = tid; u < N; u += FDESC_THREADS) s_win[u] = A.win[u];
  }
  frames_tile_stage(A, t, s_y);
  if (t.nf == 0u) return;

  // S[f][k]: one fma chain per component of (f, k), j ascending. An item is (group of up to FDESC_ILP frames, bin); a wave without one
  // skips the pass (the CU's other workgroup has the SIMD meanwhile).
  const uint32_t items = ((t.nf + FDESC_ILP - 1u) / FDESC_ILP) * NB;
  for (uint32_t q0 = 0; q0 < items; q0 += FDESC_THREADS) {
    if (q0 + (tid & ~63u) >= items) continue;  // (wave-uniform; no barrier inside the loop)
    const uint32_t q = q0 + tid;
    if (q >= items) continue;
    const uint32_t grp = q / NB, k = q - grp * NB, fa = grp * FDESC_ILP;
    const float* z0 = s_y + (size_t)fa * t.fstep;
    double* out = s_S + (size_t)fa * NB + k;
    switch (t.nf - fa) {
      case 1u: fdesc_dft<TWL, 1u>(s_tw, A.tw, s_win, z0, t.fstep, N, k, out, NB); break;
      case 2u: fdesc_dft<TWL, 2u>(s_tw, A.tw, s_win, z0, t.fstep, N, k, out, NB); break;
      case 3u: fdesc_dft<TWL, 3u>(s_tw, A.tw, s_win, z0, t.fstep, N, k, out, NB); break;
      default: fdesc_dft<TWL, FDESC_ILP>(s_tw, A.tw, s_win, z0, t.fstep, N, k, out, NB); break;
    }
  }
  __syncthreads();

  const uint32_t K = (NB + FDESC_THREADS - 1u) / FDESC_THREADS;
  const uint32_t b0 = tid * K < NB ? tid * K : NB, b1 = b0 + K < NB ? b0 + K : NB;  // this thread's bins
  const uint32_t KJ = (N + FDESC_THREADS - 1u) / FDESC_THREADS;
  const uint32_t j0 = tid * KJ < N ? tid * KJ : N, j1 = j0 + KJ < N ? j0 + KJ : N;  // this thread's samples
  const double y_first = (double)pcm_downmix(t.x, A.plane, t.C, t.inv_c, 0ull);  // (F > 0: T > 0) zcr's edge padding
  const double y_last = (double)pcm_downmix(t.x, A.plane, t.C, t.inv_c, t.T - 1u);
  const double dn = (double)N, dnb = (double)NB;
  const uint64_t r0 = A.segoff[g] + t.f0;
  for (uint32_t f = 0; f < t.nf; ++f) {
    const double* S = s_S + (size_t)f * NB;
    const float* z = s_y + (size_t)f * t.fstep;
    const int64_t t0 = (int64_t)((t.f0 + f) * H) - t.pad;  // the frame's first sample
    // the sums of the first pass, and the zero crossings of this thread's samples
    double v[FDESC_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0}, exc[FDESC_SUMS], tot[FDESC_SUMS];
    for (uint32_t kk = b0; kk < b1; ++kk) {
      const double s = S[kk], fk = (double)kk * sr / dn, p = fmax(A.amin, s * s);
      v[0] += s;
      v[1] = fma(fk, s, v[1]);
      v[2] += p;
      v[3] += log(p);
    }
    uint32_t cross = 0u;
    for (uint32_t j = j0; j < j1; ++j) {
      const double y = (double)z[j];
      v[4] = fma(y, y, v[4]);
      if (j == 0u) continue;
      const int64_t ta = t0 + (int64_t)j - 1, tb = ta + 1;
      const double ya = ta < 0 ? y_first : (uint64_t)ta >= t.T ? y_last : (double)z[j - 1u];
      const double yb = tb < 0 ? y_first : (uint64_t)tb >= t.T ? y_last : y;
      const bool sa = ya < 0.0 && fabs(ya) > A.zthr, sb = yb < 0.0 && fabs(yb) > A.zthr;
      cross += sa != sb ? 1u : 0u;
    }
    wg_sum_scan<FDESC_SUMS>(v, exc, tot, s_w);
    cross = wg_reduce_all<FDESC_WAVES>(cross, (uint32_t*)s_r, WaveSum(), 0u);
    // A = c_(NB-1), from the thread that owns the last bin
    {
      double run = exc[0];
      for (uint32_t kk = b0; kk < b1; ++kk) run += S[kk];
      if (b0 < b1 && b1 == NB) *s_a = run;
    }
    __syncthreads();
    const double a = *s_a;
    // k*: the first bin whose cumulative sum reaches theta
    const double theta = A.roll * a;
    uint64_t first = PITCH_NONE;
    {
      double run = exc[0];
      for (uint32_t kk = b0; kk < b1; ++kk) {
        run += S[kk];
        if (run >= theta && first == PITCH_NONE) first = kk;
      }
    }
    first = pitch_wg_min(first, s_r);
    if (first == PITCH_NONE) first = 0ull;  // (a NaN among the S of a segment that is refused anyway)
    const bool silent = a < FDESC_TINY;
    const double cent = silent ? 0.0 : tot[1] / a;
    double v2[1] = {0.0}, e2[1], t2[1];
    for (uint32_t kk = b0; kk < b1; ++kk) {
      const double d = (double)kk * sr / dn - cent;
      v2[0] = fma(S[kk] * d, d, v2[0]);
    }
    wg_sum_scan<1>(v2, e2, t2, s_w);
    if (tid == 0) {
      float* row = A.rows + (size_t)FDESC_COLS * (r0 + f);
      row[0] = (float)sqrt(tot[4] / dn);
      row[1] = (float)((double)cross / dn);
      row[2] = (float)cent;
      row[3] = (float)(silent ? 0.0 : sqrt(t2[0] / a));
      row[4] = (float)((double)first * sr / dn);
      row[5] = (float)(exp(tot[3] / dnb) / (tot[2] / dnb));
    }
  }
}

__global__ void __launch_bounds__(FDESC_THREADS) vsyn_fdesc_finish_kernel(const FdescCtx A) { frames_finish(A, FDESC_COLS); }

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct FdescWs {  // the stage's buffers: its own; the PCM is only read
  TableUpload tab;
  std::vector<uint8_t> fixed;  // the spec's part of the table, (cos, sin)[n] as double | window [n] as float, kept from call to call
  uint32_t fixed_n = 0, fixed_win = 0;
  bool lds_set = false;  // the kernels' dynamic-LDS limits are raised on this handle's device
  DevBuf<uint32_t> segF, flags, refused;
  DevBuf<uint64_t> segoff;
  DevBuf<float> rows;    // host form: the rows
};

// The checks of step 11 that need no launch arguments.
static inline int fdesc_check(const vsyn_fdesc_spec* sp, uint32_t S, const uint32_t* rates, const char** err) {
  if (!sp) return fail(err, VSYN_ERR_INVALID, "frame descriptor spec is NULL");
  if (sp->options & ~VSYN_FDESC_CENTER) return fail(err, VSYN_ERR_INVALID, "unknown frame descriptor options 0x%x", sp->options);
  if (sp->n_fft < FDESC_MIN_FFT || sp->n_fft > TRIM_MAX_FRAME)
    return fail(err, VSYN_ERR_INVALID, "frame descriptor n_fft %u outside [%u, %u]", sp->n_fft, FDESC_MIN_FFT, TRIM_MAX_FRAME);
  if (sp->hop_length < 1) return fail(err, VSYN_ERR_INVALID, "frame descriptor hop_length must be >= 1");
  if (sp->win_length < 1 || sp->win_length > sp->n_fft) return fail(err, VSYN_ERR_INVALID, "win_length %u outside [1, n_fft]", sp->win_length);
  if (!(sp->roll_percent > 0.0 && sp->roll_percent < 1.0)) return fail(err, VSYN_ERR_INVALID, "roll_percent %g outside (0, 1)", sp->roll_percent);
  if (!std::isfinite(sp->zcr_threshold) || !(sp->zcr_threshold >= 0.0))
    return fail(err, VSYN_ERR_INVALID, "zcr_threshold %g must be finite and >= 0", sp->zcr_threshold);
  if (!std::isfinite(sp->amin) || !(sp->amin > 0.0)) return fail(err, VSYN_ERR_INVALID, "amin %g must be finite and > 0", sp->amin);
  if (S && !rates) return fail(err, VSYN_ERR_INVALID, "sample_rates is NULL");
  return VSYN_OK;
}

static inline size_t fdesc_lds_bytes(uint32_t ft, uint32_t n, uint32_t h, bool twl) {
  return 8u * ((size_t)ft * (n / 2u + 1u) + FDESC_WORDS) + (twl ? 16u * (size_t)n : 0u) + 4u * (size_t)n + 4u * ((size_t)(ft - 1u) * std::min(n, h) + n);
}

// twiddles in LDS: when one frame then fits FDESC_LDS_BUDGET
static inline bool fdesc_twiddles_in_lds(uint32_t n, uint32_t h) { return fdesc_lds_bytes(1u, n, h, true) <= FDESC_LDS_BUDGET; }

// frames per workgroup: the most whose image fits the path's LDS budget (as pitch_tile chooses FT); one always fits
static inline uint32_t fdesc_tile(uint32_t n, uint32_t h, bool twl) {
  const size_t budget = twl ? FDESC_LDS_BUDGET : FDESC_LDS_WIDE;
  uint32_t ft = FDESC_FT_MAX;
  while (ft > 1u && fdesc_lds_bytes(ft, n, h, twl) > budget) --ft;
  return ft;
}

// Offsets, descriptor and finishing kernels on stream s; frames from d_frames, else from si. f_max bounds every segment's frames.
// d_refused [S] may be NULL. Caller holds the handle's lock and has run fdesc_check.
static inline int fdesc_launch(FdescWs& ws, int device, const vsyn_fdesc_spec* sp, uint32_t S, const uint32_t* rates, const float* d_pcm,
                               uint64_t plane, uint32_t C, const uint32_t* d_frames, const SegInfo* si, uint64_t f_max, float* d_rows,
                               uint64_t* d_segoff, uint32_t* d_refused, hipStream_t s, const char** err) {
  if (int rc = frames_check_call(S, d_pcm, d_rows, plane, err)) return rc;
  const uint32_t n = sp->n_fft, h = sp->hop_length;
  // the table: (cos, sin)[n] as double | window [n] as float (rebuilt only when n_fft or win_length change) | rates [S] as double
  const size_t off_win = 16u * (size_t)n, off_sr = align_up(off_win + 4u * (size_t)n, 16);
  if (ws.fixed_n != n || ws.fixed_win != sp->win_length) {
    ws.fixed.assign(off_sr, 0);
    twiddle_table(n, (double*)ws.fixed.data());
    hann_centred(n, sp->win_length, (float*)(ws.fixed.data() + off_win));  // the spectral stage's window
    ws.fixed_n = n;
    ws.fixed_win = sp->win_length;
  }
  std::vector<uint8_t> tab(off_sr + 8u * (size_t)S);
  memcpy(tab.data(), ws.fixed.data(), off_sr);
  double* sr = (double*)(tab.data() + off_sr);
  for (uint32_t g = 0; g < S; ++g) sr[g] = (double)rates[g];
  const bool twl = fdesc_twiddles_in_lds(n, h);
  const uint32_t ft = fdesc_tile(n, h, twl);
  const auto raise_lds = [&]() -> int {
    if (ws.lds_set) return VSYN_OK;
    HIPCHK(hipFuncSetAttribute((const void*)vsyn_fdesc_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FDESC_LDS_BUDGET));
    HIPCHK(hipFuncSetAttribute((const void*)vsyn_fdesc_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FDESC_LDS_WIDE));
    ws.lds_set = true;
    return VSYN_OK;
  };
  FdescCtx A;
  if (int rc = frames_begin(ws, device, tab, ft, h, (sp->options & VSYN_FDESC_CENTER) != 0, S, d_pcm, plane, C, d_frames, si, f_max, d_rows, d_segoff,
                            d_refused, s, err, raise_lds, A))
    return rc;
  A.sr = (const double*)(ws.tab.dev.p + off_sr);
  A.tw = (const double2*)ws.tab.dev.p;
  A.win = (const float*)(ws.tab.dev.p + off_win);
  A.N = n;
  A.roll = sp->roll_percent;
  A.zthr = sp->zcr_threshold;
  A.amin = sp->amin;
  return frames_launch(A, vsyn_fdesc_offsets_kernel, twl ? vsyn_fdesc_kernel<true> : vsyn_fdesc_kernel<false>, fdesc_lds_bytes(ft, n, h, twl),
                       vsyn_fdesc_finish_kernel, s, err);
}
