// vsyn_frames.h — what the kernels that cut PCM into frames share: the STFT family (vsyn_spectral.h, vsyn_spectral_lin.h, vsyn_chroma.h,
// vsyn_istft.h) and the pitch, descriptor and constant-Q stages (vsyn_pitch.h, vsyn_fdesc.h, vsyn_cqt.h). Every piece exists once, so that a correction to an
// order of operations reaches every kernel that promises it. All device helpers are inlined into their kernels: no kernel, no launch.
//   frames_len, spec_num_frames   a segment's PCM frames and the frames a framing cuts from them
//   frames_stage_direct           a direct-DFT tile's LDS image head: twiddles, window, the tile's padded mono span (downmix while loading)
//   frames_dft_bin                the re / im sums of one bin over that span for the tile's FT frames: ONE fma chain per component, j
//                                 ascending over the window's support, the twiddle index walked by (j k) mod n_fft
//   frames_power_store            |X|^power of a 256-bin chunk into LDS
//   frames_stockham_twiddles,     the per-pass twiddle runs and the radix-2 Stockham passes between two LDS buffers, forward and
//   frames_stockham<INVERSE>      inverse (conjugated twiddles)
//   frames_tile_head / _derive /  a (tile, segment) workgroup of the pitch and descriptor kernels: its derived quantities, the staged
//   _flag / _stage,               frames, the non-finite flag word; the offsets and finishing kernels' bodies
//   frames_offsets, frames_finish
// A Ctx template parameter is a stage's launch-argument struct; the helpers read the fields that all of them name alike (pcm, plane, C,
// frames, si; for the pitch and descriptor stages also S, H, FT, center, tiles, segF, segoff, flags, refused, rows).
// The host side holds the window and twiddle generators and the launch sequence of the pitch and descriptor stages.
#pragma once
#include "vsyn_device.h"
#include "vsyn_host.h"
#include "vsyn_trim.h"
#include "vsyn_wave.h"

#define FRAMES_THREADS 256  // the workgroup of every kernel here

__host__ __device__ __forceinline__ uint64_t spec_num_frames(uint32_t n, uint32_t hop, bool center, uint64_t T) {
  if (T == 0) return 0;
  const uint64_t tp = T + (center ? 2ull * (n / 2u) : 0ull);
  return tp < n ? 0ull : 1ull + (tp - n) / hop;
}

// PCM frames of segment g: the caller's count, else the last submit's, and at most a plane
template <class Ctx>
__device__ __forceinline__ uint64_t frames_len(const Ctx& A, uint32_t g) {
  return min((uint64_t)(A.frames ? A.frames[g] : A.si[g].total_emit), A.plane);
}

// ------------------------------------------------------------------------------------------------
// direct DFT: any n_fft
// ------------------------------------------------------------------------------------------------
// LDS image head of a direct kernel, in floats: twiddles [2n] | window [n] | span [span] | rest (the kernel's own)
struct FramesDirect {
  const float2* tw;
  const float* win;
  const float* span;
  float* rest;
  uint32_t n, hop, win_len, woff;
};

// Twiddles and window from the table, and span samples of the padded mono signal of the tile that starts at frame f0 of segment g:
// padded index p = f0 * hop + i is PCM frame p - pad (zero outside [0, T)); frames of the tile past the segment's last read the
// zero-filled rest and are never stored. No barrier behind it.
template <class Ctx>
__device__ __forceinline__ FramesDirect frames_stage_direct(const Ctx& A, float* lds, const float2* g_tw, const float* g_win, uint32_t n, uint32_t hop,
                                                            uint32_t span, uint32_t win_len, uint32_t woff, bool center, uint32_t g, uint32_t f0) {
  const uint32_t tid = threadIdx.x;
  float2* s_tw = (float2*)lds;
  float* s_win = lds + 2u * n;
  float* s_span = s_win + n;
  for (uint32_t i = tid; i < n; i += FRAMES_THREADS) {
    s_tw[i] = g_tw[i];
    s_win[i] = g_win[i];
  }
  const uint64_t T = frames_len(A, g);
  const int64_t pad = center ? (int64_t)(n / 2u) : 0;
  const int64_t p0 = (int64_t)f0 * hop - pad;
  const uint32_t C = A.C;
  const float invC = 1.0f / (float)C;
  const float* x = A.pcm + (size_t)g * C * A.plane;
  for (uint32_t i = tid; i < span; i += FRAMES_THREADS) {
    const int64_t t = p0 + (int64_t)i;
    s_span[i] = (t >= 0 && (uint64_t)t < T) ? pcm_downmix(x, A.plane, C, invC, (uint64_t)t) : 0.f;
  }
  return FramesDirect{s_tw, s_win, s_span, s_span + span, n, hop, win_len, woff};
}

// re[f] += sum_j y_f[j] (w[j] cos), im[f] += sum_j y_f[j] (w[j] sin) of bin k for the tile's FT frames: one product w * twiddle per
// component and j, then one fma per frame; re and im are the caller's registers (zeros on entry). The unroll counts of the j loop are
// the compiler's own choices from before the loop was shared, written down: at FT = 16 its choice sits on the unroller's threshold,
// and the rolled loop (no paired LDS reads) takes 44 % longer (profiles/stft_frontend_refactor.txt: session 1 is the rolled loop, 34.7
// against 24.1 ms for mel_power 2048/512; sessions 2 and 3 are these counts, at the parent's time). They do not touch a chain's order.
template <int FT>
__device__ __forceinline__ void frames_dft_bin(const FramesDirect& D, uint32_t k, float (&re)[FT], float (&im)[FT]) {
  const uint32_t n = D.n, hop = D.hop;
  uint32_t idx = (uint32_t)(((uint64_t)D.woff * k) % n);
#pragma unroll(FT <= 1 ? 8 : FT <= 4 ? 4 : 2)
  for (uint32_t j = D.woff; j < D.woff + D.win_len; ++j) {
    const float2 tw = D.tw[idx];
    const float w = D.win[j];
    const float a = w * tw.x, b = w * tw.y;
    const float* sp = D.span + j;
#pragma unroll
    for (int f = 0; f < FT; ++f) {
      const float v = sp[f * hop];
      re[f] = fmaf(v, a, re[f]);
      im[f] = fmaf(v, b, im[f]);
    }
    idx += k;
    if (idx >= n) idx -= n;
  }
}

// This thread's bin of a 256-bin chunk: |X|^power of the FT frames into s_S [FT][256]
template <int FT>
__device__ __forceinline__ void frames_power_store(const float (&re)[FT], const float (&im)[FT], uint32_t power, float* s_S) {
#pragma unroll
  for (int f = 0; f < FT; ++f) {
    const float p = fmaf(re[f], re[f], im[f] * im[f]);
    s_S[f * FRAMES_THREADS + threadIdx.x] = power == 1 ? sqrtf(p) : p;
  }
}

// ------------------------------------------------------------------------------------------------
// radix-2 Stockham transform of M = n_fft / 2 complex points per frame: n_fft a power of two
// ------------------------------------------------------------------------------------------------
// The per-pass twiddle runs from the table's (cos, sin)(2 pi m / n_fft): pass Ns reads s_st[Ns - 1 + k] = (cos, sin)(2 pi k / (2 Ns)),
// k < Ns, at stride 1 whatever its span. No barrier behind it.
__device__ __forceinline__ void frames_stockham_twiddles(const float2* g_tw, float2* s_st, uint32_t M, uint32_t lgM) {
  for (uint32_t e = threadIdx.x; e + 1u < M; e += FRAMES_THREADS) {
    const uint32_t lv = 31u - (uint32_t)__clz((int)(e + 1u)), Ns = 1u << lv, k = e + 1u - Ns;
    s_st[e] = g_tw[k << (lgM - lv)];  // k * n / (2 Ns)
  }
}

// The passes over src [ft][M] (filled; no barrier needed in front), natural order in and out, no bit reversal: butterfly j of a frame
// reads a = src[j], b = src[j + M/2] and writes a + w b, a - w b to dst[j0], dst[j0 + Ns], j0 = 2 (j - k) + k, k = j mod Ns,
// w = exp(-2 pi i k / (2 Ns)), its conjugate for the (unnormalised) inverse. On return src holds the transform and dst is free; ends
// behind a barrier.
template <bool INVERSE>
__device__ __forceinline__ void frames_stockham(const float2* s_st, float2*& src, float2*& dst, uint32_t ft, uint32_t M, uint32_t lgM) {
  const uint32_t half = M >> 1, tot = ft * half;
  for (uint32_t Ns = 1; Ns < M; Ns <<= 1) {
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < tot; q += FRAMES_THREADS) {
      const uint32_t f = q >> (lgM - 1u), j = q & (half - 1u), k = j & (Ns - 1u);
      const float2 w = s_st[Ns - 1u + k];
      const float2* in = src + (size_t)f * M;
      const float2 a = in[j], b = in[j + half];
      const float tr = INVERSE ? w.x * b.x - w.y * b.y : w.x * b.x + w.y * b.y;
      const float ti = INVERSE ? w.x * b.y + w.y * b.x : w.x * b.y - w.y * b.x;
      float2* out = dst + (size_t)f * M + (((j - k) << 1) + k);
      out[0] = make_float2(a.x + tr, a.y + ti);
      out[Ns] = make_float2(a.x - tr, a.y - ti);
    }
    float2* sw = src;
    src = dst;
    dst = sw;
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------
// staged frames with a non-finite flag: the pitch and descriptor stages
// ------------------------------------------------------------------------------------------------
struct FramesTile {  // a (tile, segment) workgroup's share
  uint32_t* flag;          // its word of the flags
  uint64_t F, f0, T;       // the segment's frames, the tile's first, the segment's PCM frames
  uint32_t L, nf;          // frame length; frames of the tile (F = 0, T > 0: tile 0 has none and still looks at the samples)
  bool last, apart;        // the segment's last tile; hop > L: frames that do not touch, staged back to back
  uint32_t fstep, staged;  // floats from a staged frame to the next; floats staged
  int64_t pad, base;       // centre padding; sample index of the first staged float
  const float* x;          // the segment's first plane
  uint32_t C;
  float inv_c;
};

// The workgroup's tile of segment blockIdx.y in three steps. frames_tile_head: its flag word, the segment's frames and the tile's
// first; true (workgroup-uniform) when there is nothing here, the segment skipped or the tile past its frames: the kernel then returns
// through frames_tile_idle, which clears the flag word, still this workgroup's to write. frames_tile_derive: the rest, for frames of L
// samples. (One routine that returns from two places keeps a second test of its result in the kernels' entry code.)
template <class Ctx>
__device__ __forceinline__ bool frames_tile_head(const Ctx& A, bool skipped, FramesTile& t) {
  t.flag = A.flags + (size_t)blockIdx.y * A.tiles + blockIdx.x;
  t.F = A.segF[blockIdx.y];
  t.f0 = (uint64_t)blockIdx.x * A.FT;
  return skipped || (t.f0 >= t.F && blockIdx.x != 0u);
}

__device__ __forceinline__ void frames_tile_idle(const FramesTile& t) {
  if (threadIdx.x == 0) *t.flag = 0u;
}

template <class Ctx>
__device__ __forceinline__ void frames_tile_derive(const Ctx& A, uint32_t L, FramesTile& t) {
  const uint32_t g = blockIdx.y;
  t.T = frames_len(A, g);
  t.L = L;
  t.nf = t.f0 < t.F ? (uint32_t)trim_min64(A.FT, t.F - t.f0) : 0u;
  t.last = t.f0 + A.FT >= t.F;
  t.C = A.C;
  t.inv_c = 1.0f / (float)t.C;
  t.x = A.pcm + (size_t)g * t.C * A.plane;
  t.pad = A.center ? (int64_t)(L / 2u) : 0;
  t.apart = A.H > L;
  t.fstep = t.apart ? L : A.H;
  t.staged = t.nf ? (t.nf - 1u) * t.fstep + L : 0u;
  t.base = (int64_t)(t.f0 * A.H) - t.pad;
}

// The tile's flag word: whether a sample of the workgroup's share of the segment, [its first frame's start, the next tile's), the
// first tile from 0 and the last up to T, is an Inf or a NaN. Called by the whole workgroup; holds one barrier.
template <class Ctx>
__device__ __forceinline__ void frames_tile_flag(const Ctx& A, const FramesTile& t) {
  const uint32_t tid = threadIdx.x;
  const int64_t lo = blockIdx.x == 0u ? 0 : (t.base > 0 ? t.base : 0);
  int64_t hi = t.last ? (int64_t)t.T : (int64_t)((t.f0 + A.FT) * A.H) - t.pad;
  if (hi > (int64_t)t.T) hi = (int64_t)t.T;
  bool bad = false;
  for (int64_t s = lo + tid; s < hi; s += FRAMES_THREADS) bad |= trim_not_finite(pcm_downmix(t.x, A.plane, t.C, t.inv_c, (uint64_t)s));
  const int any = __syncthreads_or(bad ? 1 : 0);
  if (tid == 0) *t.flag = any ? 1u : 0u;
}

// The tile's frames as float32 into s_y (the downmix is done while loading, zeros outside [0, T)), and the flag word: whether a sample
// of the workgroup's share of the segment, [its first frame's start, the next tile's), the first tile from 0 and the last up to T, is
// an Inf or a NaN. Ends behind a barrier.
template <class Ctx>
__device__ __forceinline__ void frames_tile_stage(const Ctx& A, const FramesTile& t, float* s_y) {
  const uint32_t tid = threadIdx.x, L = t.L, H = A.H;
  const bool apart = t.apart;
  const int64_t base = t.base;
  for (uint32_t u = tid; u < t.staged; u += FRAMES_THREADS) {
    const int64_t s = apart ? base + (int64_t)(u / L) * H + (u % L) : base + u;
    s_y[u] = (s >= 0 && (uint64_t)s < t.T) ? pcm_downmix(t.x, A.plane, t.C, t.inv_c, (uint64_t)s) : 0.f;
  }
  frames_tile_flag(A, t);  // (also the barrier behind the staging)
}

// One workgroup: per segment its frame count under frames of L samples (0 where skip(g)) and the exclusive row scan segoff[S+1].
template <class Ctx, class Skip>
__device__ __forceinline__ void frames_offsets(const Ctx& A, uint32_t L, Skip skip) {
  wg_exclusive_scan<FRAMES_THREADS, 1>(A.S, A.segoff, [&](uint32_t g, uint64_t* v) {
    v[0] = skip(g) ? 0ull : spec_num_frames(L, A.H, A.center != 0, frames_len(A, g));
    A.segF[g] = (uint32_t)v[0];
  });
}

// One workgroup per segment: a segment with a flagged tile is refused: its rows of cols columns become NaN and its word of the refused
// array 1.
template <class Ctx>
__device__ __forceinline__ void frames_finish(const Ctx& A, uint32_t cols) {
  const uint32_t g = blockIdx.x, tid = threadIdx.x;
  bool bad = false;
  for (uint32_t i = tid; i < A.tiles; i += FRAMES_THREADS) bad |= A.flags[(size_t)g * A.tiles + i] != 0u;
  const int refused = __syncthreads_or(bad ? 1 : 0);
  if (tid == 0 && A.refused) A.refused[g] = refused ? 1u : 0u;
  if (!refused) return;
  float* rows = A.rows + (uint64_t)cols * A.segoff[g];
  const uint64_t nv = (uint64_t)cols * A.segF[g];
  for (uint64_t i = tid; i < nv; i += FRAMES_THREADS) rows[i] = __uint_as_float(0x7FC00000u);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// The periodic Hann window of win_length, centred in n_fft: its support of out [n_fft]; the rest is the caller's zeros.
static inline void hann_centred(uint32_t n_fft, uint32_t win_length, float* out) {
  float* w = out + (n_fft - win_length) / 2u;
  for (uint32_t i = 0; i < win_length; ++i) w[i] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)i / (double)win_length));
}

// out[2m], out[2m + 1] = (cos, sin)(2 pi m / n), m < n, computed in double
template <typename T>
static inline void twiddle_table(uint32_t n, T* out) {
  for (uint32_t m = 0; m < n; ++m) {
    const double a = 2.0 * M_PI * (double)m / (double)n;
    out[2u * m] = (T)cos(a);
    out[2u * m + 1u] = (T)sin(a);
  }
}

// The refusals of a pitch or descriptor call that need nothing of its spec.
static inline int frames_check_call(uint32_t S, const float* d_pcm, const float* d_rows, uint64_t plane, const char** err) {
  if (S > 65535u) return fail(err, VSYN_ERR_INVALID, "too many segments (%u > 65535)", S);
  if (((uintptr_t)d_pcm & 3u) || ((uintptr_t)d_rows & 3u)) return fail(err, VSYN_ERR_INVALID, "PCM and row pointers must be 4-byte aligned");
  if (plane > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "plane_stride must be below 2^32");
  return VSYN_OK;
}

// Behind frames_check_call and the stage's choice of ft frames per workgroup: the tiles bound, the stage's dynamic-LDS limit
// (raise_lds, called once the device is selected), its buffers, the upload of its table, and the fields of A that every such stage
// has. What points into the table (ws.tab.dev.p) and the stage's own fields are the caller's to fill.
template <class Ws, class Ctx, class RaiseLds>
static inline int frames_begin(Ws& ws, int device, const std::vector<uint8_t>& tab, uint32_t ft, uint32_t hop, bool center, uint32_t S, const float* d_pcm,
                               uint64_t plane, uint32_t C, const uint32_t* d_frames, const SegInfo* si, uint64_t f_max, float* d_rows, uint64_t* d_segoff,
                               uint32_t* d_refused, hipStream_t s, const char** err, RaiseLds raise_lds, Ctx& A) {
  const uint64_t tiles = std::max<uint64_t>((f_max + ft - 1u) / ft, 1);
  if (tiles > 0x7FFFFFFFull || f_max > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "segment too long");
  HIPCHK(hipSetDevice(device));
  if (int rc = raise_lds()) return rc;
  HIPCHK(ws.segF.ensure(S));
  HIPCHK(ws.segoff.ensure((size_t)S + 1));
  HIPCHK(ws.flags.ensure((size_t)S * tiles));
  if (int rc = ws.tab.upload(tab, s, err)) return rc;
  A.pcm = d_pcm;
  A.plane = plane;
  A.C = C;
  A.S = S;
  A.frames = d_frames;
  A.si = si;
  A.H = hop;
  A.FT = ft;
  A.center = center ? 1u : 0u;
  A.tiles = (uint32_t)tiles;
  A.segF = ws.segF.p;
  A.segoff = d_segoff ? d_segoff : ws.segoff.p;
  A.flags = ws.flags.p;
  A.refused = d_refused;
  A.rows = d_rows;
  return VSYN_OK;
}

// The stage's three kernels on stream s: offsets, one workgroup per (tile, segment) with lds bytes of dynamic LDS, finish. The
// constant-Q stage (vsyn_cqt.h) runs gz workgroups per (tile, segment), one per group of bins (blockIdx.z), and for its chroma
// outputs a fold kernel per (tile, segment) in front of the finishing one.
template <class Ctx>
static inline int frames_launch(const Ctx& A, void (*offsets)(Ctx), void (*tile)(Ctx), size_t lds, void (*finish)(Ctx), hipStream_t s, const char** err,
                                uint32_t gz = 1u, void (*fold)(Ctx) = nullptr) {
  VSYN_LAUNCH(offsets, dim3(1), dim3(FRAMES_THREADS), 0, s, A);
  VSYN_LAUNCH(tile, dim3(A.tiles, A.S, gz), dim3(FRAMES_THREADS), lds, s, A);
  if (fold) VSYN_LAUNCH(fold, dim3(A.tiles, A.S), dim3(FRAMES_THREADS), 0, s, A);
  VSYN_LAUNCH(finish, dim3(A.S), dim3(FRAMES_THREADS), 0, s, A);
  return VSYN_OK;
}
