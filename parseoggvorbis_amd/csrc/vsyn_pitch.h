// vsyn_pitch.h — pitch: per frame the fundamental frequency (YIN) and the normalised difference at the chosen lag, from planar
// float32 PCM already on the device (librosa.yin on the mono signal). Semantics: include/vorbis_synth_hip.h, "pitch".
//
// Three kernels on one stream (the per-segment periods are built on the host in double, pitch_periods):
//   1. vsyn_pitch_offsets_kernel  one workgroup: per segment its PCM frames, its frame count (spec_num_frames), the exclusive row
//                                 scan seg_off[S+1]: frames_offsets (vsyn_frames.h).
//   2. vsyn_pitch_kernel          grid (tile of FT frames, segment). LDS: the tile's span of the mono signal as float32 (the downmix
//                                 is done while loading, zeros outside [0, T); H > L: the frames back to back), staged by
//                                 frames_tile_head / frames_tile_derive / frames_tile_stage (vsyn_frames.h), then d[FT][p_max] as float64.
//                                 Difference function: the (frame, lag) pairs of the tile are dealt to the threads in order, lag
//                                 fastest, PITCH_ILP pairs per thread PITCH_THREADS apart. A thread owns its lag tau and walks j =
//                                 1 .. W: z[j] is one address per frame (a broadcast read), z[j + tau] consecutive across the lanes
//                                 (ds_read_b32, 32 banks, no conflict inside a frame). Both are widened to float64, the difference
//                                 is exact, and the sum is ONE fma chain with j ascending, whatever the tile and the thread: the
//                                 PITCH_ILP chains of a thread are independent and only hide the fma latency (the workgroup is one
//                                 wave per SIMD, two workgroups per CU at the LDS budget).
//                                 Then per frame, by the whole workgroup: the cumulative sum S (order below), c in place of d,
//                                 the first trough below the threshold and the first minimum by 64-bit integer minima through the
//                                 wave and the four waves (vsyn_wave.h), and thread 0 writes the row. No atomics.
//                                 The workgroup also looks at every sample of its share of the segment for an Inf or a NaN
//                                 (trim_not_finite, the trim stage's test) and stores one flag word per tile (frames_tile_stage).
//                                 The difference function, S, c, the trough test and the parabolic shift are the device functions of
//                                 vsyn_yin.h, which the pYIN kernel (vsyn_pyin.h) calls too.
//   3. vsyn_pitch_finish_kernel   one workgroup per segment: a segment with a flagged tile is refused: its rows become NaN and its
//                                 word of the refused array 1 (frames_finish).
// Order of S: with K = ceil(p_max / PITCH_THREADS), thread t owns the lags t K + 1 .. (t + 1) K. It adds its d in ascending order
// (its total), the totals go through wg_sum_scan<1> (vsyn_wave.h; DESIGN.md 6t: the wave scan over the lane offsets 1, 2, .. 32, a wave's
// offset the sum of the earlier waves' totals in ascending order), and S[tau] = (wave offset + the exclusive lane prefix) + d[first] + .. + d[tau],
// added left to right. A function of p_max alone. Every term is >= 0: the relative error is at most (terms) * 2^-53.
// Nothing here reads or writes stream state, the overlap carry or any synthesis buffer; the PCM is only read.
#pragma once
#include "vsyn_device.h"
#include "vsyn_frames.h"
#include "vsyn_host.h"
#include "vsyn_trim.h"
#include "vsyn_yin.h"

#define PITCH_FT_MAX 64u                    // frames per workgroup, at most
#define PITCH_LDS_BUDGET (79u * 1024u)      // dynamic LDS of a workgroup: two fit a CU's 160 KiB beside their static words

struct PitchCtx {  // launch arguments
  const PitchSeg* seg;
  const float* pcm;
  uint64_t plane;
  uint32_t C, S;
  const uint32_t* frames;  // PCM frames per segment (caller's, or the resampler's), or
  const SegInfo* si;       // the last submit's SegInfo (total_emit)
  uint32_t L, H, FT;       // frame_length, hop_length, frames per workgroup
  uint32_t center;
  uint32_t tiles;          // workgroups per segment (grid.x): the flags' stride
  double thr;              // trough_threshold
  uint32_t* segF;          // [S] frames
  uint64_t* segoff;        // [S+1]
  uint32_t* flags;         // [S][tiles] a sample of the tile's share is not finite
  uint32_t* refused;       // [S]
  float* rows;             // [segoff[S]][2]
};

__global__ void __launch_bounds__(PITCH_THREADS) vsyn_pitch_offsets_kernel(const PitchCtx A) {
  frames_offsets(A, A.L, [&](uint32_t g) { return A.seg[g].p_max == 0u; });
}

__global__ void __launch_bounds__(PITCH_THREADS) vsyn_pitch_kernel(const PitchCtx A) {
  extern __shared__ double s_pitch[];
  __shared__ uint64_t s_r[PITCH_WAVES];
  __shared__ double s_w[PITCH_WAVES];
  const uint32_t g = blockIdx.y, tid = threadIdx.x;
  const PitchSeg sg = A.seg[g];
  FramesTile t;
  if (frames_tile_head(A, sg.p_max == 0u, t)) return frames_tile_idle(t);
  frames_tile_derive(A, A.L, t);
  const uint32_t L = A.L, W = L / 2u, PL = sg.p_max;
  const uint32_t nf = t.nf, fstep = t.fstep;
  const uint64_t f0 = t.f0;
  float* s_y = (float*)s_pitch;
  double* s_d = s_pitch + (((size_t)(A.FT - 1u) * fstep + L + 1u) >> 1);
  frames_tile_stage(A, t, s_y);
  if (nf == 0u) return;

  yin_difference(s_y, s_d, nf, fstep, W, PL);  // d[f][tau - 1], tau = 1 .. PL

  const uint32_t p_min = sg.p_min, n = PL - p_min + 1u;
  const uint64_t r0 = A.segoff[g] + f0;
  for (uint32_t f = 0; f < nf; ++f) {
    double* d = s_d + (size_t)f * PL;
    yin_normalise(d, PL, p_min, s_w);  // S, and c in place of d from p_min on
    // i*: the first trough below the threshold, else the first minimum (c >= 0: its bit pattern orders as its value)
    const double* c = d + (p_min - 1u);
    uint64_t first = PITCH_NONE, low = PITCH_NONE;
    for (uint32_t i = tid; i < n; i += PITCH_THREADS) {
      const double ci = c[i];
      if (yin_trough(c, i, n) && ci < A.thr) first = trim_min64(first, i);
      low = trim_min64(low, (uint64_t)__double_as_longlong(ci));
    }
    first = pitch_wg_min(first, s_r);
    if (first == PITCH_NONE) {  // (workgroup-uniform)
      low = pitch_wg_min(low, s_r);
      for (uint32_t i = tid; i < n; i += PITCH_THREADS)
        if ((uint64_t)__double_as_longlong(c[i]) == low) first = trim_min64(first, i);
      first = pitch_wg_min(first, s_r);
      if (first == PITCH_NONE) first = 0ull;  // (a NaN among the c of a segment that is refused anyway)
    }
    if (tid == 0) {
      const uint32_t is = (uint32_t)first;
      const double shift = yin_shift(c, is, n);
      float* row = A.rows + 2u * (r0 + f);
      row[0] = (float)(sg.sr / ((double)(p_min + is) + shift));
      row[1] = (float)c[is];
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(PITCH_THREADS) vsyn_pitch_finish_kernel(const PitchCtx A) { frames_finish(A, 2u); }

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct PitchWs {  // the stage's buffers: its own; the PCM is only read
  TableUpload tab;
  bool lds_set = false;  // the kernel's dynamic-LDS limit is raised on this handle's device
  DevBuf<uint32_t> segF, flags, refused;
  DevBuf<uint64_t> segoff;
  DevBuf<float> rows;    // host form: the rows
};

// p_min and p_max of step 3 for rate sr, in double; false: fewer than two lags
static inline bool pitch_periods(const vsyn_pitch_spec* sp, uint32_t sr, uint32_t* p_min, uint32_t* p_max) {
  const uint32_t L = sp->frame_length, W = L / 2u;
  const double lo = std::max(floor((double)sr / sp->fmax), 1.0);
  const double hi = std::min(ceil((double)sr / sp->fmin), (double)(L - W - 1u));
  if (!(hi - lo + 1.0 >= 2.0)) return false;
  *p_min = (uint32_t)lo;
  *p_max = (uint32_t)hi;
  return true;
}

// The checks of the spec and of every segment's rate (0 = skipped segment).
static inline int pitch_check(const vsyn_pitch_spec* sp, uint32_t S, const uint32_t* rates, const char** err) {
  if (!sp) return fail(err, VSYN_ERR_INVALID, "pitch spec is NULL");
  if (sp->options & ~VSYN_PITCH_CENTER) return fail(err, VSYN_ERR_INVALID, "unknown pitch options 0x%x", sp->options);
  if (sp->frame_length < 4 || sp->frame_length > TRIM_MAX_FRAME)
    return fail(err, VSYN_ERR_INVALID, "pitch frame_length %u outside [4, %u]", sp->frame_length, TRIM_MAX_FRAME);
  if (sp->hop_length < 1) return fail(err, VSYN_ERR_INVALID, "pitch hop_length must be >= 1");
  if (!std::isfinite(sp->fmin) || !std::isfinite(sp->fmax) || !(sp->fmin > 0.0 && sp->fmin < sp->fmax))
    return fail(err, VSYN_ERR_INVALID, "pitch fmin %g / fmax %g: need 0 < fmin < fmax", sp->fmin, sp->fmax);
  if (!std::isfinite(sp->trough_threshold) || !(sp->trough_threshold > 0.0 && sp->trough_threshold <= 1.0))
    return fail(err, VSYN_ERR_INVALID, "pitch trough_threshold %g outside (0, 1]", sp->trough_threshold);
  if (S && !rates) return fail(err, VSYN_ERR_INVALID, "sample_rates is NULL");
  for (uint32_t g = 0; g < S; ++g) {
    if (!rates[g]) continue;
    uint32_t p_min, p_max;
    if (sp->fmax > rates[g] / 2.0) return fail(err, VSYN_ERR_INVALID, "segment %u: fmax %g above sr/2 = %g", g, sp->fmax, rates[g] / 2.0);
    if (!pitch_periods(sp, rates[g], &p_min, &p_max))
      return fail(err, VSYN_ERR_INVALID, "segment %u: fewer than two lags between sr/fmax and min(sr/fmin, frame_length - frame_length/2 - 1)", g);
  }
  return VSYN_OK;
}

static inline size_t pitch_lds_bytes(uint32_t ft, uint32_t L, uint32_t H, uint32_t pl) {
  return 8u * ((((size_t)(ft - 1u) * std::min(L, H) + L + 1u) >> 1) + (size_t)ft * pl);
}

// frames per workgroup: the most whose span and difference functions fit the LDS budget (as spec_tile chooses FT); one always fits
static inline uint32_t pitch_tile(uint32_t L, uint32_t H, uint32_t pl) {
  uint32_t ft = PITCH_FT_MAX;
  while (ft > 1u && pitch_lds_bytes(ft, L, H, pl) > PITCH_LDS_BUDGET) --ft;
  return ft;
}

// Offsets, pitch and finishing kernels on stream s; frames from d_frames, else from si. f_max bounds every segment's frames.
// d_refused [S] may be NULL. Caller holds the handle's lock and has run pitch_check.
static inline int pitch_launch(PitchWs& ws, int device, const vsyn_pitch_spec* sp, uint32_t S, const uint32_t* rates, const float* d_pcm,
                               uint64_t plane, uint32_t C, const uint32_t* d_frames, const SegInfo* si, uint64_t f_max, float* d_rows,
                               uint64_t* d_segoff, uint32_t* d_refused, hipStream_t s, const char** err) {
  if (int rc = frames_check_call(S, d_pcm, d_rows, plane, err)) return rc;
  const uint32_t L = sp->frame_length, H = sp->hop_length;
  std::vector<uint8_t> tab(sizeof(PitchSeg) * (size_t)S);
  PitchSeg* seg = (PitchSeg*)tab.data();
  uint32_t pl = 2u;
  for (uint32_t g = 0; g < S; ++g) {
    seg[g] = PitchSeg{(double)rates[g], 0u, 0u};
    if (rates[g]) pitch_periods(sp, rates[g], &seg[g].p_min, &seg[g].p_max);
    pl = std::max(pl, seg[g].p_max);
  }
  const uint32_t ft = pitch_tile(L, H, pl);
  const auto raise_lds = [&]() -> int {
    if (ws.lds_set) return VSYN_OK;
    HIPCHK(hipFuncSetAttribute((const void*)vsyn_pitch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PITCH_LDS_BUDGET));
    ws.lds_set = true;
    return VSYN_OK;
  };
  PitchCtx A;
  if (int rc = frames_begin(ws, device, tab, ft, H, (sp->options & VSYN_PITCH_CENTER) != 0, S, d_pcm, plane, C, d_frames, si, f_max, d_rows, d_segoff,
                            d_refused, s, err, raise_lds, A))
    return rc;
  A.seg = (const PitchSeg*)ws.tab.dev.p;
  A.L = L;
  A.thr = sp->trough_threshold;
  return frames_launch(A, vsyn_pitch_offsets_kernel, vsyn_pitch_kernel, pitch_lds_bytes(ft, L, H, pl), vsyn_pitch_finish_kernel, s, err);
}
