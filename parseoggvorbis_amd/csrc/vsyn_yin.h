// vsyn_yin.h — the front that the YIN kernel (vsyn_pitch.h) and the pYIN kernel (vsyn_pyin.h) share: steps 4 and 5 of "pitch"
// (include/vorbis_synth_hip.h), the float64 difference function of a tile's staged frames and its cumulative-mean normalisation.
// Device functions only, inlined into their kernels; every order of operations is stated in vsyn_pitch.h and exists once, here.
#pragma once
#include "vsyn_device.h"
#include "vsyn_frames.h"
#include "vsyn_wave.h"

#define PITCH_THREADS 256
static_assert(PITCH_THREADS == FRAMES_THREADS, "the shared framing helpers stride by the workgroup's size");
#define PITCH_WAVES (PITCH_THREADS / 64)
#define PITCH_ILP 4u                        // independent fma chains per thread
#define PITCH_TINY 2.2250738585072014e-308  // numpy.finfo(float64).tiny
#define PITCH_NONE 0xFFFFFFFFFFFFFFFFull

struct PitchSeg {  // one segment's periods (host, double): p_max = 0 skips the segment
  double sr;
  uint32_t p_min, p_max;
};

// the minimum of v over the workgroup, for every thread (s_r: PITCH_WAVES words of LDS, free again on return)
__device__ __forceinline__ uint64_t pitch_wg_min(uint64_t v, uint64_t* s_r) {
  return wg_reduce_all<PITCH_WAVES>(v, s_r, WaveMin(), PITCH_NONE);
}

// Step 4 for the nf frames staged in s_y, fstep floats apart: s_d[f * PL + tau - 1] = d[tau], tau = 1 .. PL, one fma chain per
// (f, tau) with j ascending over 1 .. W. Ends behind a barrier.
__device__ __forceinline__ void yin_difference(const float* s_y, double* s_d, uint32_t nf, uint32_t fstep, uint32_t W, uint32_t PL) {
  const uint32_t tid = threadIdx.x;
  const uint32_t items = nf * PL;
  for (uint32_t q0 = 0; q0 < items; q0 += PITCH_ILP * PITCH_THREADS) {
    const float* zf[PITCH_ILP];
    uint32_t tau[PITCH_ILP];
    double acc[PITCH_ILP];
#pragma unroll
    for (uint32_t r = 0; r < PITCH_ILP; ++r) {
      const uint32_t q = q0 + r * PITCH_THREADS + tid;
      const uint32_t qq = q < items ? q : 0u;  // (an idle chain repeats pair 0 and is not stored)
      const uint32_t f = qq / PL;
      tau[r] = qq - f * PL + 1u;
      zf[r] = s_y + (size_t)f * fstep;
      acc[r] = 0.0;
    }
    // (the unroll count is the compiler's own choice from before the loop was shared, written down: inlined from here it chose 4,
    // with 28 more VGPRs in the pitch kernel. It does not touch a chain's order.)
#pragma unroll 2
    for (uint32_t j = 1; j <= W; ++j) {
#pragma unroll
      for (uint32_t r = 0; r < PITCH_ILP; ++r) {
        const double df = (double)zf[r][j] - (double)zf[r][j + tau[r]];  // (j + tau <= W + p_max <= L - 1)
        acc[r] = fma(df, df, acc[r]);
      }
    }
#pragma unroll
    for (uint32_t r = 0; r < PITCH_ILP; ++r) {
      const uint32_t q = q0 + r * PITCH_THREADS + tid;
      if (q < items) s_d[q] = acc[r];
    }
  }
  __syncthreads();
}

// Step 5 for one frame's d [PL], by the whole workgroup: S in the order of vsyn_pitch.h, and c in place of d from p_min on
// (c[i] = d[p_min - 1 + i]). s_w: PITCH_WAVES doubles. Ends behind a barrier.
__device__ __forceinline__ void yin_normalise(double* d, uint32_t PL, uint32_t p_min, double* s_w) {
  const uint32_t tid = threadIdx.x;
  const uint32_t K = (PL + PITCH_THREADS - 1u) / PITCH_THREADS;
  const uint32_t b0 = tid * K < PL ? tid * K : PL, b1 = b0 + K < PL ? b0 + K : PL;  // this thread's lags, as indices tau - 1
  double tot[1] = {0.0}, exc[1], all[1];
  for (uint32_t k = b0; k < b1; ++k) tot[0] += d[k];
  wg_sum_scan<1>(tot, exc, all, s_w);
  double run = exc[0];
  for (uint32_t k = b0; k < b1; ++k) {
    const double dk = d[k];
    run += dk;
    if (k + 1u >= p_min) d[k] = dk / (run / (double)(k + 1u) + PITCH_TINY);
  }
  __syncthreads();
}

// trough[i] of step 6 over c [n], its end rules included
__device__ __forceinline__ bool yin_trough(const double* c, uint32_t i, uint32_t n) {
  const double ci = c[i];
  return i == 0u ? ci < c[1] : i == n - 1u ? ci < c[i - 1u] : (ci < c[i - 1u] && ci <= c[i + 1u]);
}

// the parabolic shift of step 7 at index is of c [n]
__device__ __forceinline__ double yin_shift(const double* c, uint32_t is, uint32_t n) {
  double shift = 0.0;
  if (is > 0u && is < n - 1u) {
    const double a = (c[is + 1u] + c[is - 1u]) - 2.0 * c[is];
    const double b = (c[is + 1u] - c[is - 1u]) * 0.5;
    if (fabs(b) < fabs(a)) shift = -b / a;
  }
  return shift;
}
