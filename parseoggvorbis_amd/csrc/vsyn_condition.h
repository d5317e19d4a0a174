// vsyn_condition.h — PCM conditioning: mono downmix, peak normalisation and pre-emphasis of planar float32 PCM already on the
// device, into one float32 plane per segment. Semantics: include/vorbis_synth_hip.h, "PCM conditioning".
//
// Two kernels on one stream, both on a grid of (tile of COND_TILE frames, segment):
//   1. vsyn_cond_peak_kernel   VSYN_COND_PEAK only. Every thread downmixes its frames (pcm_downmix, vsyn_device.h) and keeps the
//                              largest |bits| as an unsigned integer; the maximum goes through the wave, the
//                              workgroup's four waves (vsyn_wave.h) and one atomicMax per workgroup into the segment's word, which the
//                              host side clears first. A maximum does not depend on the order: the same PCM gives the same bits.
//   2. vsyn_cond_apply_kernel  downmix again, y / p (__fdiv_rn, the IEEE division) when the word holds a finite p > 0, then
//                              z[t] = fmaf(-a, y1[t-1], y1[t]): each thread recomputes y1[t-1] from one more frame on its left, so
//                              there is no chain. A word that is not finite (Inf or NaN in the segment) gives a plane of zeros:
//                              the segment is refused, its word tells the caller. Also writes the frames it used per segment.
// Memory access: when plane_stride is a multiple of 4 every channel plane of a segment has the same offset from a 16-byte
// boundary, m floats. A thread then owns the four frames 4q - m .. 4q - m + 3 (q = its index in the grid row): 16-byte loads from
// every plane, a scalar head (group 0, the m > 0 case) and tail (the group that crosses T). Otherwise the planes' offsets differ
// and no grouping aligns them all: thread i of a tile takes frames i, i + 256, ... with 4-byte loads, a wave's loads contiguous.
// Both forms do the same float32 operations per frame. The output plane is stored 16 bytes at a time where its address allows.
// Nothing here reads or writes stream state, the overlap carry or any synthesis buffer; the PCM is only read.
#pragma once
#include "vsyn_device.h"
#include "vsyn_host.h"
#include "vsyn_wave.h"

#define COND_THREADS 256
#define COND_PER_THREAD 4
#define COND_TILE (COND_THREADS * COND_PER_THREAD)  // frames per workgroup
#define COND_NOT_FINITE 0x7F800000u                  // |bits| from here on: Inf, NaN

struct CondCtx {  // launch arguments
  const float* pcm;
  uint64_t plane;
  uint32_t C, S;
  const uint32_t* frames;  // PCM frames per segment (caller's, or the resampler's), or
  const SegInfo* si;       // the last submit's SegInfo (total_emit)
  float* out;              // [S][out_plane]
  uint64_t out_plane;
  uint32_t* peak;          // [S] max |bits| of the downmix (VSYN_COND_PEAK), else NULL
  uint32_t* out_frames;    // [S] frames written per segment
  uint32_t opts;           // VSYN_COND_*
  float a;                 // pre-emphasis coefficient, rounded once to float32
};

__device__ __forceinline__ uint64_t cond_frames(const CondCtx& A, uint32_t g) {
  return min(min((uint64_t)(A.frames ? A.frames[g] : A.si[g].total_emit), A.plane), A.out_plane);
}

// the planes' common offset from a 16-byte boundary in floats, or 4 when they have none (scalar form)
__device__ __forceinline__ uint32_t cond_misalign(const CondCtx& A) {
  return (A.plane & 3u) ? 4u : (uint32_t)(((uintptr_t)A.pcm >> 2) & 3u);
}

// four frames from t0 of every plane, each component downmixed as pcm_downmix does (same operations, same order)
__device__ __forceinline__ float4 cond_downmix4(const float* x, uint64_t plane, uint32_t C, float inv_c, uint64_t t0) {
  float4 s = *(const float4*)(x + t0);
  for (uint32_t c = 1; c < C; ++c) {
    const float4 v = *(const float4*)(x + (size_t)c * plane + t0);
    s.x += v.x;
    s.y += v.y;
    s.z += v.z;
    s.w += v.w;
  }
  if (C != 1) {
    s.x = s.x * inv_c;
    s.y = s.y * inv_c;
    s.z = s.z * inv_c;
    s.w = s.w * inv_c;
  }
  return s;
}

__device__ __forceinline__ uint32_t cond_abs_bits(float v) { return __float_as_uint(v) & 0x7FFFFFFFu; }

__global__ void __launch_bounds__(COND_THREADS) vsyn_cond_peak_kernel(const CondCtx A) {
  __shared__ uint32_t s_wave[COND_THREADS / 64];
  const uint32_t g = blockIdx.y, tid = threadIdx.x;
  const uint64_t T = cond_frames(A, g);
  const uint64_t tile0 = (uint64_t)blockIdx.x * COND_TILE;
  const uint32_t m = cond_misalign(A);
  if (tile0 >= T + (m & 3u)) return;  // (workgroup-uniform)
  const uint32_t C = A.C;
  const float inv_c = 1.0f / (float)C;
  const float* x = A.pcm + (size_t)g * C * A.plane;
  uint32_t mx = 0u;
  if (m < 4u) {
    const int64_t t0 = (int64_t)(tile0 + 4u * tid) - (int64_t)m;
    if (t0 >= 0 && (uint64_t)t0 + 3u < T) {
      const float4 y = cond_downmix4(x, A.plane, C, inv_c, (uint64_t)t0);
      mx = max(max(cond_abs_bits(y.x), cond_abs_bits(y.y)), max(cond_abs_bits(y.z), cond_abs_bits(y.w)));
    } else {
      for (int k = 0; k < 4; ++k) {
        const int64_t t = t0 + k;
        if (t >= 0 && (uint64_t)t < T) mx = max(mx, cond_abs_bits(pcm_downmix(x, A.plane, C, inv_c, (uint64_t)t)));
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < COND_PER_THREAD; ++k) {
      const uint64_t t = tile0 + (uint32_t)k * COND_THREADS + tid;
      if (t < T) mx = max(mx, cond_abs_bits(pcm_downmix(x, A.plane, C, inv_c, t)));
    }
  }
  mx = wg_reduce_t0<COND_THREADS / 64>(mx, s_wave, WaveMax(), 0u);
  if (tid == 0) {
    if (mx) atomicMax(A.peak + g, mx);  // (the word was cleared: silence leaves it 0)
  }
}

// y -> z for one frame: the peak division, then the pre-emphasis against the frame on its left (y_prev; unused for t = 0)
__device__ __forceinline__ float cond_finish(float y, float y_prev, bool first, float p, bool div, bool pre, float a) {
  const float y1 = div ? __fdiv_rn(y, p) : y;
  if (!pre || first) return y1;
  const float y1p = div ? __fdiv_rn(y_prev, p) : y_prev;
  return fmaf(-a, y1p, y1);
}

__global__ void __launch_bounds__(COND_THREADS) vsyn_cond_apply_kernel(const CondCtx A) {
  const uint32_t g = blockIdx.y, tid = threadIdx.x;
  const uint64_t T = cond_frames(A, g);
  if (blockIdx.x == 0 && tid == 0) A.out_frames[g] = (uint32_t)T;
  const uint64_t tile0 = (uint64_t)blockIdx.x * COND_TILE;
  const uint32_t m = cond_misalign(A);
  if (tile0 >= T + (m & 3u)) return;
  const uint32_t C = A.C;
  const float inv_c = 1.0f / (float)C;
  const float* x = A.pcm + (size_t)g * C * A.plane;
  float* z = A.out + (size_t)g * A.out_plane;
  const uint32_t pb = A.peak ? A.peak[g] : 0u;
  const bool refused = pb >= COND_NOT_FINITE, div = pb != 0u && !refused, pre = (A.opts & VSYN_COND_PREEMPH) != 0;
  const float p = __uint_as_float(pb), a = A.a;
  if (m < 4u) {
    const int64_t t0 = (int64_t)(tile0 + 4u * tid) - (int64_t)m;
    if (t0 >= 0 && (uint64_t)t0 + 3u < T) {
      float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!refused) {
        const float4 y = cond_downmix4(x, A.plane, C, inv_c, (uint64_t)t0);
        const float yl = (pre && t0 > 0) ? pcm_downmix(x, A.plane, C, inv_c, (uint64_t)t0 - 1u) : 0.f;
        r.x = cond_finish(y.x, yl, t0 == 0, p, div, pre, a);
        r.y = cond_finish(y.y, y.x, false, p, div, pre, a);
        r.z = cond_finish(y.z, y.y, false, p, div, pre, a);
        r.w = cond_finish(y.w, y.z, false, p, div, pre, a);
      }
      float* o = z + t0;
      if ((((uintptr_t)o) & 15u) == 0) {
        *(float4*)o = r;
      } else {
        o[0] = r.x;
        o[1] = r.y;
        o[2] = r.z;
        o[3] = r.w;
      }
    } else {
      for (int k = 0; k < 4; ++k) {
        const int64_t t = t0 + k;
        if (t < 0 || (uint64_t)t >= T) continue;
        float r = 0.f;
        if (!refused) {
          const float y = pcm_downmix(x, A.plane, C, inv_c, (uint64_t)t);
          const float yl = (pre && t > 0) ? pcm_downmix(x, A.plane, C, inv_c, (uint64_t)t - 1u) : 0.f;
          r = cond_finish(y, yl, t == 0, p, div, pre, a);
        }
        z[t] = r;
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < COND_PER_THREAD; ++k) {
      const uint64_t t = tile0 + (uint32_t)k * COND_THREADS + tid;
      if (t >= T) continue;
      float r = 0.f;
      if (!refused) {
        const float y = pcm_downmix(x, A.plane, C, inv_c, t);
        const float yl = (pre && t > 0) ? pcm_downmix(x, A.plane, C, inv_c, t - 1u) : 0.f;
        r = cond_finish(y, yl, t == 0, p, div, pre, a);
      }
      z[t] = r;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct CondWs {  // the stage's buffers: its own; the PCM is only read
  DevBuf<float> pcm;                   // host forms: the conditioned mono planes
  DevBuf<uint32_t> peak, frames;       // per segment: max |bits| of the downmix; frames written
  DevBuf<int16_t> s16;                 // vsyn_pcm_condition_host, VSYN_PCM_S16
};

static inline int cond_check(const vsyn_pcm_cond* c, const char** err) {
  if (!c) return fail(err, VSYN_ERR_INVALID, "PCM conditioning spec is NULL");
  if (c->options & ~(VSYN_COND_PEAK | VSYN_COND_PREEMPH)) return fail(err, VSYN_ERR_INVALID, "unknown conditioning options 0x%x", c->options);
  if (c->options & VSYN_COND_PREEMPH) {
    const double a = c->preemphasis;
    if (!std::isfinite(a) || !(a > 0.0 && a < 1.0) || !((float)a > 0.0f && (float)a < 1.0f))
      return fail(err, VSYN_ERR_INVALID, "pre-emphasis coefficient %g outside (0, 1)", a);
  }
  return VSYN_OK;
}

// A NULL handle: without a usable device there is nothing to make one from, and that is what the caller has to hear.
static inline int cond_no_handle(const char** err) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(err, VSYN_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
  return fail(err, VSYN_ERR_INVALID, "handle is NULL");
}

// The stage's kernels on stream s: frames from d_frames, else from si; t_max bounds every segment's frames. d_peak [S] (uint32
// view of the float peaks; NULL: ws.peak) is cleared and filled with VSYN_COND_PEAK only. The frames written go to
// ws.frames. Caller holds the handle's lock and has run cond_check.
static inline int cond_launch(CondWs& ws, int device, const vsyn_pcm_cond* c, uint32_t S, const float* d_pcm, uint64_t plane, uint32_t C,
                       const uint32_t* d_frames, const SegInfo* si, uint64_t t_max, float* d_out, uint64_t out_plane, uint32_t* d_peak,
                       hipStream_t s, const char** err) {
  if (S > 65535u) return fail(err, VSYN_ERR_INVALID, "too many segments (%u > 65535)", S);
  if (((uintptr_t)d_pcm & 3u) || ((uintptr_t)d_out & 3u)) return fail(err, VSYN_ERR_INVALID, "PCM pointers must be 4-byte aligned");
  const uint64_t gx = (std::min(std::min(t_max, plane), out_plane) + 3u + COND_TILE - 1u) / COND_TILE;
  if (gx > 0x7FFFFFFFull) return fail(err, VSYN_ERR_INVALID, "segment too long");
  HIPCHK(hipSetDevice(device));
  HIPCHK(ws.frames.ensure(S));
  const bool peak = (c->options & VSYN_COND_PEAK) != 0;
  if (peak && !d_peak) {
    HIPCHK(ws.peak.ensure(S));
    d_peak = ws.peak.p;
  }
  CondCtx A;
  A.pcm = d_pcm;
  A.plane = plane;
  A.C = C;
  A.S = S;
  A.frames = d_frames;
  A.si = si;
  A.out = d_out;
  A.out_plane = out_plane;
  A.peak = peak ? d_peak : nullptr;
  A.out_frames = ws.frames.p;
  A.opts = c->options;
  A.a = (c->options & VSYN_COND_PREEMPH) ? (float)c->preemphasis : 0.0f;
  const dim3 grid((uint32_t)gx, S);
  if (peak) {
    HIPCHK(hipMemsetAsync(d_peak, 0, sizeof(uint32_t) * S, s));
    VSYN_LAUNCH(vsyn_cond_peak_kernel, grid, dim3(COND_THREADS), 0, s, A);
  }
  VSYN_LAUNCH(vsyn_cond_apply_kernel, grid, dim3(COND_THREADS), 0, s, A);
  return VSYN_OK;
}

// peaks_out[S] (may be NULL) from the workspace's peak words behind the kernels on stream s; zeros without VSYN_COND_PEAK.
static inline int cond_fetch_peaks(const CondWs& ws, const vsyn_pcm_cond* c, uint32_t S, float* peaks_out, hipStream_t s, const char** err) {
  if (!peaks_out || !S) return VSYN_OK;
  if (c->options & VSYN_COND_PEAK) HIPCHK(hipMemcpyAsync(peaks_out, ws.peak.p, sizeof(float) * S, hipMemcpyDeviceToHost, s));
  else memset(peaks_out, 0, sizeof(float) * S);
  return VSYN_OK;
}
