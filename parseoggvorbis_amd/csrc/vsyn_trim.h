// vsyn_trim.h — PCM trimming: cuts the silent head and tail of planar float32 PCM already on the device, into one mono float32
// plane per segment (librosa.effects.trim on the mono signal). Semantics: include/vorbis_synth_hip.h, "PCM trimming".
//
// Three kernels on one stream:
//   1. vsyn_trim_energy_kernel  grid (tile of FT frames, segment). The workgroup stages the downmix (pcm_downmix, vsyn_device.h) of
//                               the tile's span in LDS once: overlapping frames read each sample L / H times, from LDS and not
//                               from HBM. H <= L: one contiguous span of (FT - 1) H + L samples; H > L (frames that do not touch):
//                               the FT frames back to back, L samples each. The four waves take the tile's frames in turn; lane l
//                               of a wave adds the squares of the frame's samples l, l + 64, ... in float64, in ascending order,
//                               and wave_sum (the butterfly of DESIGN.md 6t) makes the frame's sum: its order is a
//                               function of L alone, whatever the tile, the grid and the segment's slot. ms[f] = sum / L goes to
//                               the workspace and to the caller's d_ms. The workgroup also looks at every sample of its share of
//                               the segment (the hops of its frames; the last tile up to T) for an Inf or a NaN, also where no
//                               frame covers it (H > L, the tail), and stores one flag word per tile.
//   2. vsyn_trim_bounds_kernel  one workgroup per segment, behind a finished ms array: the maximum of ms[g][0 .. F) on the doubles'
//                               bit patterns with the sign masked (a maximum has no order; NaN > Inf > finite), the tiles' flags,
//                               then the first and last frame with E = max(ms, 1e-10) > R k (or E >= R) by integer min / max through the wave
//                               and the four waves (vsyn_wave.h). Writes (start, end), out_frames and R. No atomics.
//   3. vsyn_trim_cut_kernel     grid (tile of TRIM_CUT_TILE frames, segment): out[t] = downmix(start + t) for t < end - start.
// Memory access of the cut kernel: a thread owns four output frames that start at a 16-byte boundary of the OUTPUT plane (a
// scalar head and tail around them). start is a multiple of H and otherwise arbitrary, so whether the four input frames of every
// channel plane sit on a 16-byte boundary too differs per segment; it is uniform per workgroup: 16-byte loads (cond_downmix4)
// when they do, four 4-byte loads per plane when not. Both forms do the same float32 operations per frame.
// Nothing here reads or writes stream state, the overlap carry or any synthesis buffer; the PCM is only read.
// The split stage (vsyn_split.h) launches the energy kernel as it is and shares the bounds kernel's reference and predicate.
#pragma once
#include "vsyn_condition.h"
#include "vsyn_device.h"
#include "vsyn_host.h"
#include "vsyn_wave.h"

#define TRIM_THREADS 256
#define TRIM_WAVES (TRIM_THREADS / 64)
#define TRIM_MAX_FRAME 8192u
#define TRIM_FT_MAX 64u                    // frames per energy workgroup, at most
#define TRIM_LDS_FLOATS 16128u             // 63 KiB: within what a workgroup gets without raising the kernel's limit; L <= 8192 fits
#define TRIM_SCAN_SAMPLES 65536u           // H > L: a workgroup's share of the segment is FT * H samples; keep it near this
#define TRIM_CUT_TILE (TRIM_THREADS * 4)   // output frames per cut workgroup
#define TRIM_AMIN_SQ 1e-10                 // librosa's amin = 1e-5 on the amplitude, squared
#define TRIM_ABS64 0x7FFFFFFFFFFFFFFFull
#define TRIM_NOT_FINITE64 0x7FF0000000000000ull  // |bits| from here on: Inf, NaN

struct TrimCtx {  // launch arguments
  const float* pcm;
  uint64_t plane;
  uint32_t C;
  const uint32_t* frames;  // PCM frames per segment (caller's, or the resampler's), or
  const SegInfo* si;       // the last submit's SegInfo (total_emit)
  uint64_t t_cap;          // no segment has more frames than this: what the workspace was sized for
  uint32_t L, H, FT;       // frame_length, hop_length, frames per energy workgroup
  uint32_t tiles;          // energy workgroups per segment (grid.x): the flags' stride
  uint64_t F_max;          // the workspace ms' stride: frames of the longest segment allowed
  double k;                // 10^(-top_db / 10)
  double* ms;              // [S][F_max] workspace
  uint32_t* flags;         // [S][tiles] a sample of the tile's share is not finite
  double* d_ms;            // caller's, d_ms[g * ms_stride + f], or NULL
  uint64_t ms_stride;
  float* out;              // [S][out_plane]
  uint64_t out_plane;
  uint32_t* bounds;        // [S][2] start, end
  uint32_t* out_frames;    // [S] end - start
  double* ref;             // [S] R
};

__host__ __device__ __forceinline__ uint64_t trim_num_frames(uint64_t T, uint32_t L, uint32_t H) {
  if (T == 0) return 0;  // (T >= 1: T + 2 (L / 2) - L >= 0)
  return 1u + (T + 2u * (uint64_t)(L / 2u) - L) / H;
}

// 64-bit minimum and maximum written out: the bit patterns of doubles go through these, and no overload may round them
__device__ __forceinline__ uint64_t trim_min64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t trim_max64(uint64_t a, uint64_t b) { return a > b ? a : b; }

__device__ __forceinline__ uint64_t trim_frames(const TrimCtx& A, uint32_t g) {
  return trim_min64(trim_min64(A.frames ? A.frames[g] : A.si[g].total_emit, A.t_cap), trim_min64(A.plane, A.out_plane));
}

__device__ __forceinline__ bool trim_not_finite(float v) { return (__float_as_uint(v) & 0x7FFFFFFFu) >= COND_NOT_FINITE; }

__global__ void __launch_bounds__(TRIM_THREADS) vsyn_trim_energy_kernel(const TrimCtx A) {
  extern __shared__ float s_y[];
  __shared__ uint32_t s_bad;
  const uint32_t g = blockIdx.y, tid = threadIdx.x;
  const uint64_t T = trim_frames(A, g);
  const uint32_t L = A.L, H = A.H, half = L / 2u;
  const uint64_t F = trim_num_frames(T, L, H);
  const uint64_t f0 = (uint64_t)blockIdx.x * A.FT;
  if (tid == 0) s_bad = 0u;
  if (f0 >= F) {  // (workgroup-uniform) no frames here: the flag word is still this workgroup's to write
    if (tid == 0) A.flags[(size_t)g * A.tiles + blockIdx.x] = 0u;
    return;
  }
  const uint32_t nf = (uint32_t)trim_min64(A.FT, F - f0);
  const bool last = f0 + nf == F;
  const uint32_t C = A.C;
  const float inv_c = 1.0f / (float)C;
  const float* x = A.pcm + (size_t)g * C * A.plane;
  const bool apart = H > L;  // frames that do not touch: staged back to back
  const uint32_t fstep = apart ? L : H, staged = (nf - 1u) * fstep + L;
  const int64_t base = (int64_t)(f0 * H) - (int64_t)half;  // sample index of the first staged float
  bool bad = false;
  for (uint32_t u = tid; u < staged; u += TRIM_THREADS) {
    const int64_t t = apart ? base + (int64_t)(u / L) * H + (u % L) : base + u;
    float v = 0.f;
    if (t >= 0 && (uint64_t)t < T) {
      v = pcm_downmix(x, A.plane, C, inv_c, (uint64_t)t);
      bad |= trim_not_finite(v);
    }
    s_y[u] = v;
  }
  // what of the workgroup's share [base, the next tile's base), the last tile's up to T, was not staged
  {
    const int64_t lo = apart ? (base > 0 ? base : 0) : base + (int64_t)staged;
    const int64_t hi = last ? (int64_t)T : (int64_t)((f0 + nf) * H) - (int64_t)half;
    for (int64_t t = lo + tid; t < hi; t += TRIM_THREADS) {
      if (apart && (uint64_t)(t - base) % H < L) continue;  // inside a frame: seen while it was staged
      bad |= trim_not_finite(pcm_downmix(x, A.plane, C, inv_c, (uint64_t)t));
    }
  }
  __syncthreads();
  if (bad) s_bad = 1u;  // (every writer stores the same word)
  const uint32_t wave = tid >> 6, lane = tid & 63u;
  for (uint32_t j = wave; j < nf; j += TRIM_WAVES) {
    const float* fr = s_y + (size_t)j * fstep;
    double acc = 0.0;
    for (uint32_t i = lane; i < L; i += 64u) {
      const double v = (double)fr[i];
      acc += v * v;
    }
    acc = wave_sum(acc);
    if (lane == 0) {
      const double m = acc / (double)L;
      A.ms[(size_t)g * A.F_max + f0 + j] = m;
      if (A.d_ms) A.d_ms[(size_t)g * A.ms_stride + f0 + j] = m;
    }
  }
  __syncthreads();
  if (tid == 0) A.flags[(size_t)g * A.tiles + blockIdx.x] = s_bad;
}

// The reference of segment g behind its finished ms array, for a whole workgroup of TRIM_THREADS (s_a: TRIM_WAVES words of LDS, free
// again on return): the maximum of ms on its bit patterns (ms >= 0, or not finite and then above every finite one); a flagged tile
// counts as a NaN. trim_refused / trim_ref / trim_loud read the decision off it; the split stage (vsyn_split.h) shares all four.
__device__ __forceinline__ uint64_t trim_segment_max(const TrimCtx& A, uint32_t g, uint64_t F, const double* ms, uint64_t* s_a) {
  const uint32_t tid = threadIdx.x;
  const uint32_t tiles = (uint32_t)((F + A.FT - 1u) / A.FT);
  uint64_t mx = 0ull;
  for (uint64_t f = tid; f < F; f += TRIM_THREADS) mx = trim_max64(mx, (uint64_t)__double_as_longlong(ms[f]) & TRIM_ABS64);
  for (uint32_t i = tid; i < tiles; i += TRIM_THREADS)
    if (A.flags[(size_t)g * A.tiles + i]) mx = trim_max64(mx, TRIM_NOT_FINITE64 | 0x0008000000000000ull);
  return wg_reduce_all<TRIM_WAVES>(mx, s_a, WaveMax(), 0ull);
}
__device__ __forceinline__ bool trim_refused(uint64_t mx) { return mx >= TRIM_NOT_FINITE64; }
__device__ __forceinline__ double trim_ref(uint64_t mx) {
  return trim_refused(mx) ? __longlong_as_double((long long)mx) : fmax(__longlong_as_double((long long)mx), TRIM_AMIN_SQ);
}
// is a frame of mean square m non-silent under R and thr = R k? (E >= R: a loudest frame, also where R k rounds up to R)
__device__ __forceinline__ bool trim_loud(double m, double R, double thr) {
  const double E = fmax(m, TRIM_AMIN_SQ);
  return E > thr || E >= R;
}

__global__ void __launch_bounds__(TRIM_THREADS) vsyn_trim_bounds_kernel(const TrimCtx A) {
  __shared__ uint64_t s_a[TRIM_WAVES], s_b[TRIM_WAVES];
  const uint32_t g = blockIdx.x, tid = threadIdx.x;
  const uint64_t T = trim_frames(A, g);
  const uint64_t F = trim_num_frames(T, A.L, A.H);
  const double* ms = A.ms + (size_t)g * A.F_max;
  const uint64_t mx = trim_segment_max(A, g, F, ms, s_a);
  const bool refused = trim_refused(mx);
  const double R = trim_ref(mx);
  uint64_t first = ~0ull, lastf = 0ull;  // first non-silent frame; last non-silent frame + 1
  if (!refused) {
    const double thr = R * A.k;
    for (uint64_t f = tid; f < F; f += TRIM_THREADS) {
      if (trim_loud(ms[f], R, thr)) {
        first = trim_min64(first, f);
        lastf = trim_max64(lastf, f + 1u);
      }
    }
  }
  wg_put(first, s_a, WaveMin());  // (one barrier for the two)
  wg_put(lastf, s_b, WaveMax());
  __syncthreads();
  if (tid == 0) {
    first = wg_get<TRIM_WAVES>(s_a, WaveMin(), ~0ull);
    lastf = wg_get<TRIM_WAVES>(s_b, WaveMax(), 0ull);
    uint64_t start = 0, end = 0;
    if (lastf) {  // (F >= 1 and not refused: the frame that holds the maximum is there)
      start = first * A.H;
      end = trim_min64(T, lastf * A.H);
    }
    A.bounds[2u * g] = (uint32_t)start;
    A.bounds[2u * g + 1u] = (uint32_t)end;
    A.out_frames[g] = (uint32_t)(end - start);
    A.ref[g] = R;
  }
}

__global__ void __launch_bounds__(TRIM_THREADS) vsyn_trim_cut_kernel(const TrimCtx A) {
  const uint32_t g = blockIdx.y, tid = threadIdx.x;
  const uint64_t start = A.bounds[2u * g], n = A.bounds[2u * g + 1u] - start;
  float* z = A.out + (size_t)g * A.out_plane;
  const uint32_t mo = (uint32_t)(((uintptr_t)z >> 2) & 3u);  // the output plane's offset from a 16-byte boundary, in floats
  const uint64_t tile0 = (uint64_t)blockIdx.x * TRIM_CUT_TILE;
  if (tile0 >= n + mo) return;  // (workgroup-uniform)
  const uint32_t C = A.C;
  const float inv_c = 1.0f / (float)C;
  const float* x = A.pcm + (size_t)g * C * A.plane;
  // do the four input frames under an aligned group of four output frames start at a 16-byte boundary in every plane?
  const bool in16 = (C == 1u || (A.plane & 3u) == 0u) && (((((uintptr_t)x >> 2) + start - mo) & 3u) == 0u);
  const int64_t t0 = (int64_t)(tile0 + 4u * tid) - (int64_t)mo;
  if (t0 >= 0 && (uint64_t)t0 + 3u < n) {
    float4 r;
    if (in16) {
      r = cond_downmix4(x, A.plane, C, inv_c, start + (uint64_t)t0);
    } else {
      r.x = pcm_downmix(x, A.plane, C, inv_c, start + (uint64_t)t0);
      r.y = pcm_downmix(x, A.plane, C, inv_c, start + (uint64_t)t0 + 1u);
      r.z = pcm_downmix(x, A.plane, C, inv_c, start + (uint64_t)t0 + 2u);
      r.w = pcm_downmix(x, A.plane, C, inv_c, start + (uint64_t)t0 + 3u);
    }
    *(float4*)(z + t0) = r;
  } else {
    for (int k = 0; k < 4; ++k) {
      const int64_t t = t0 + k;
      if (t >= 0 && (uint64_t)t < n) z[t] = pcm_downmix(x, A.plane, C, inv_c, start + (uint64_t)t);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct TrimWs {  // the stage's buffers: its own; the PCM is only read
  DevBuf<float> pcm;                   // host forms: the trimmed mono planes
  DevBuf<double> ms, ref;              // per (segment, frame): the mean square; per segment: R
  DevBuf<uint32_t> flags;              // per (segment, energy tile): not finite
  DevBuf<uint32_t> bounds, frames;     // per segment: (start, end); frames written
  DevBuf<int16_t> s16;                 // vsyn_pcm_trim_host, VSYN_PCM_S16
};

static inline int trim_check(const vsyn_pcm_trim* t, const char** err) {
  if (!t) return fail(err, VSYN_ERR_INVALID, "PCM trim spec is NULL");
  if (t->frame_length < 1 || t->frame_length > TRIM_MAX_FRAME)
    return fail(err, VSYN_ERR_INVALID, "trim frame_length %u outside [1, %u]", t->frame_length, TRIM_MAX_FRAME);
  if (t->hop_length < 1) return fail(err, VSYN_ERR_INVALID, "trim hop_length must be >= 1");
  if (!std::isfinite(t->top_db) || !(t->top_db > 0.0 && t->top_db <= 200.0))
    return fail(err, VSYN_ERR_INVALID, "trim top_db %g outside (0, 200]", t->top_db);
  return VSYN_OK;
}

// frames per energy workgroup: the most whose staged samples fit the LDS budget (as spec_tile chooses FT), and for frames that
// do not touch no more than keeps the workgroup's share of the segment near TRIM_SCAN_SAMPLES
static inline uint32_t trim_tile(uint32_t L, uint32_t H) {
  const uint32_t fstep = std::min(L, H);
  uint32_t ft = std::min<uint32_t>(TRIM_FT_MAX, 1u + (TRIM_LDS_FLOATS - L) / fstep);
  if (H > L) ft = std::min(ft, std::max(1u, TRIM_SCAN_SAMPLES / H));
  return ft;
}

// The stage's checks, workspace and launch arguments, and the energy kernel on stream s: frames from d_frames, else from si; t_max
// bounds every segment's frames. *A receives the arguments the kernels behind the energy kernel take (bounds as given; d_ref NULL:
// the workspace's). The split stage (vsyn_split.h) starts here too, on a workspace of its own. Caller holds the handle's lock and
// has run trim_check.
static inline int trim_energy_launch(TrimWs& ws, int device, const vsyn_pcm_trim* tr, uint32_t S, const float* d_pcm, uint64_t plane, uint32_t C,
                              const uint32_t* d_frames, const SegInfo* si, uint64_t t_max, float* d_out, uint64_t out_plane, uint32_t* d_out_frames,
                              uint32_t* d_bounds, double* d_ref, double* d_ms, uint64_t ms_stride, hipStream_t s, TrimCtx* ctx, const char** err) {
  if (S > 65535u) return fail(err, VSYN_ERR_INVALID, "too many segments (%u > 65535)", S);
  if (((uintptr_t)d_pcm & 3u) || ((uintptr_t)d_out & 3u)) return fail(err, VSYN_ERR_INVALID, "PCM pointers must be 4-byte aligned");
  if ((uintptr_t)d_ms & 7u) return fail(err, VSYN_ERR_INVALID, "d_ms must be 8-byte aligned");
  const uint32_t L = tr->frame_length, H = tr->hop_length;
  const uint64_t T = std::min(std::min(t_max, plane), out_plane);
  if (T > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "segment too long");
  const uint64_t F_max = std::max<uint64_t>(trim_num_frames(T, L, H), 1);
  if (d_ms && ms_stride < F_max) return fail(err, VSYN_ERR_INVALID, "ms_stride %llu below %llu frames", (unsigned long long)ms_stride, (unsigned long long)F_max);
  const uint32_t ft = trim_tile(L, H);
  const uint64_t tiles = (F_max + ft - 1u) / ft;
  if (tiles > 0x7FFFFFFFull) return fail(err, VSYN_ERR_INVALID, "segment too long");
  HIPCHK(hipSetDevice(device));
  HIPCHK(ws.ms.ensure((size_t)S * F_max));
  HIPCHK(ws.flags.ensure((size_t)S * tiles));
  HIPCHK(ws.frames.ensure(S));
  if (!d_ref) {
    HIPCHK(ws.ref.ensure(S));
    d_ref = ws.ref.p;
  }
  TrimCtx& A = *ctx;
  A.pcm = d_pcm;
  A.plane = plane;
  A.C = C;
  A.frames = d_frames;
  A.si = si;
  A.t_cap = T;
  A.L = L;
  A.H = H;
  A.FT = ft;
  A.tiles = (uint32_t)tiles;
  A.F_max = F_max;
  A.k = pow(10.0, -tr->top_db / 10.0);
  A.ms = ws.ms.p;
  A.flags = ws.flags.p;
  A.d_ms = d_ms;
  A.ms_stride = ms_stride;
  A.out = d_out;
  A.out_plane = out_plane;
  A.bounds = d_bounds;
  A.out_frames = d_out_frames ? d_out_frames : ws.frames.p;
  A.ref = d_ref;
  const uint32_t fstep = std::min(L, H);
  const size_t lds = sizeof(float) * ((size_t)(ft - 1u) * fstep + L);
  VSYN_LAUNCH(vsyn_trim_energy_kernel, dim3((uint32_t)tiles, S), dim3(TRIM_THREADS), lds, s, A);
  return VSYN_OK;
}

// The stage's kernels on stream s: frames from d_frames, else from si; t_max bounds every segment's frames. d_bounds [S][2],
// d_out_frames [S], d_ref [S] (NULL: the workspace's); d_ms with ms_stride optional. Caller holds the handle's lock and has run
// trim_check.
static inline int trim_launch(TrimWs& ws, int device, const vsyn_pcm_trim* tr, uint32_t S, const float* d_pcm, uint64_t plane, uint32_t C,
                       const uint32_t* d_frames, const SegInfo* si, uint64_t t_max, float* d_out, uint64_t out_plane, uint32_t* d_out_frames,
                       uint32_t* d_bounds, double* d_ref, double* d_ms, uint64_t ms_stride, hipStream_t s, const char** err) {
  if (!d_bounds) {
    HIPCHK(hipSetDevice(device));
    HIPCHK(ws.bounds.ensure(2u * (size_t)S));
    d_bounds = ws.bounds.p;
  }
  TrimCtx A;
  if (int rc = trim_energy_launch(ws, device, tr, S, d_pcm, plane, C, d_frames, si, t_max, d_out, out_plane, d_out_frames, d_bounds, d_ref, d_ms,
                                  ms_stride, s, &A, err))
    return rc;
  const uint64_t gx = (A.t_cap + 3u + TRIM_CUT_TILE - 1u) / TRIM_CUT_TILE;
  VSYN_LAUNCH(vsyn_trim_bounds_kernel, dim3(S), dim3(TRIM_THREADS), 0, s, A);
  VSYN_LAUNCH(vsyn_trim_cut_kernel, dim3((uint32_t)gx, S), dim3(TRIM_THREADS), 0, s, A);
  return VSYN_OK;
}

// bounds_out[S][2] and refs_out[S] (either may be NULL) from the workspace behind the kernels on stream s
static inline int trim_fetch_bounds(const TrimWs& ws, uint32_t S, uint32_t* bounds_out, double* refs_out, hipStream_t s, const char** err) {
  if (!S) return VSYN_OK;
  if (bounds_out) HIPCHK(hipMemcpyAsync(bounds_out, ws.bounds.p, sizeof(uint32_t) * 2u * S, hipMemcpyDeviceToHost, s));
  if (refs_out) HIPCHK(hipMemcpyAsync(refs_out, ws.ref.p, sizeof(double) * S, hipMemcpyDeviceToHost, s));
  return VSYN_OK;
}
