// vsyn_spectral_lin.h — linear-frequency rows (|X|^power, its dB image, the complex STFT) from planar float32 PCM already on the
// device. Semantics: include/vorbis_synth_hip.h, "linear spectra". Design and measurements: DESIGN.md 6k.
//
// The offsets kernel, the table (header, twiddles, window, per-segment rate index; no mel bands) and the workspace are those of
// vsyn_spectral.h. Behind the offsets kernel, one workgroup of 256 threads per (segment, tile of frames), by n_fft alone:
//   vsyn_spec_lin_fft_kernel         n_fft a power of two. Per frame the real-input FFT: z[m] = v[2m] + i v[2m+1] (v = w * y, one
//                                    float32 product), a radix-2 Stockham transform of M = n_fft / 2 points between two LDS buffers
//                                    (log2 M passes of t = w * b; a + t, a - t; natural order in and out, no bit reversal), then the
//                                    untangling pass X[k] = E + w_k O with E, O from Z[k] and conj Z[M - k]. A frame owns its M
//                                    complex words: nothing of one frame enters another's sums. The twiddles sit in LDS twice: per
//                                    pass a compact run of Ns entries (so a pass reads them at stride 1, whatever its span), and
//                                    the n_fft / 2 + 1 entries of the untangling pass. The tile's transforms and one bin's
//                                    untangling are the __device__ helpers spec_lin_fft_tile_run and spec_lin_untangle, which
//                                    the chroma kernel (vsyn_chroma.h) calls as well.
//                                    The per-pass twiddle runs and the passes are frames_stockham_twiddles and frames_stockham<false>
//                                    (vsyn_frames.h), which the inverse (vsyn_istft.h) runs with INVERSE = true.
//   vsyn_spec_lin_direct_kernel<FT>  any other n_fft: frames_stage_direct and frames_dft_bin (vsyn_frames.h: twiddle index walked by
//                                    (j k) mod n_fft, one fma chain per component, j ascending over the window's support), its sums
//                                    stored as bins.
//   vsyn_spec_lin_clamp_kernel       LIN_DB with top_db > 0, after either: the clamp against the segment's maximum, elementwise.
// Nothing here reads or writes stream state, the overlap carry or any synthesis buffer; the PCM is only read.
#pragma once
#include "vsyn_spectral.h"

#define SPEC_LIN_DIRECT_FT 8

// Frames per workgroup of the FFT kernel: 2048 / n_fft, so that a pass has 512 butterflies (two per thread) up to n_fft = 2048;
// at most 64 (n_fft = 16: 256 butterflies), one frame from 2048 on.
__host__ __device__ __forceinline__ uint32_t spec_lin_fft_tile(uint32_t n) { return n >= 2048u ? 1u : (2048u / n > 64u ? 64u : 2048u / n); }
// LDS image of the FFT kernel, in floats (M = n / 2): pass twiddles [M] float2 | untangling twiddles [M + 1] float2 | two buffers
// of [ft][M] float2
__host__ __device__ __forceinline__ uint64_t spec_lin_fft_lds_floats(uint32_t ft, uint32_t n) { return 2ull * n + 2ull + 2ull * ft * n; }
// LDS image of the direct kernel, in floats: FramesDirect's head alone, twiddles [2n] | window [n] | span [(ft-1) hop + n]
__host__ __device__ __forceinline__ uint64_t spec_lin_direct_lds_floats(uint32_t ft, uint32_t n, uint32_t hop) { return 3ull * n + spec_span_len(ft, n, hop); }

// One bin of row r into the kind's layout; returns the dB value of LIN_DB where it is finite (for the segment's maximum), -inf
// otherwise.
__device__ __forceinline__ float spec_lin_emit(const SpecHeader* H, float* rows, uint64_t r, uint32_t k, float re, float im) {
  const uint32_t nb = H->nbins;
  if (H->kind == VSYN_SPEC_STFT) {
    float* p = rows + (r * nb + k) * 2u;
    p[0] = re;
    p[1] = im;
    return -INFINITY;
  }
  const float p = fmaf(re, re, im * im);
  const float S = H->power == 1 ? sqrtf(p) : p;
  if (H->kind == VSYN_SPEC_LIN_POWER) {
    rows[r * nb + k] = S;
    return -INFINITY;
  }
  const float d = 10.0f * log10f(spec_floor(S, H->amin));
  rows[r * nb + k] = d;
  return spec_max_term(d);
}

__device__ __forceinline__ void spec_lin_seg_max(const SpecCtx& A, uint32_t g, float mx) {
  mx = wave_max(mx);
  if ((threadIdx.x & 63u) == 0 && mx > -INFINITY) atomicMax(A.segmax + g, spec_key(mx));
}

// The transforms of one tile, shared by vsyn_spec_lin_fft_kernel and the chroma kernel (vsyn_chroma.h): what spec_lin_fft_tile_run
// leaves in LDS. Z[f * M + m] is frame f's half-size transform, un its untangling twiddles, and spare the other ping-pong buffer
// ([ft][M] float2), free behind the last pass.
struct SpecLinFft {
  const float2* Z;
  const float2* un;
  float2* spare;
};

// Bin k <= M of one frame from its half-size transform Z: X[k] = E + w_k O, E = (Z[k] + conj Z[M-k]) / 2, O = (Z[k] - conj Z[M-k]) / 2i,
// Z[M] = Z[0]; X[M] = Re Z[0] - Im Z[0]
__device__ __forceinline__ void spec_lin_untangle(const float2* Z, const float2* s_un, uint32_t M, uint32_t k, float& re, float& im) {
  const float2 a = Z[k & (M - 1u)], b = Z[(M - k) & (M - 1u)];
  if (k == M) {
    re = a.x - a.y;
    im = 0.f;
  } else {
    const float er = 0.5f * (a.x + b.x), ei = 0.5f * (a.y - b.y);
    const float qr = 0.5f * (a.y + b.y), qi = 0.5f * (b.x - a.x);
    const float2 w = s_un[k];
    re = er + (w.x * qr + w.y * qi);
    im = ei + (w.x * qi - w.y * qr);
  }
}

// The twiddles, the windowed frames f0 .. f0 + nf - 1 of segment g and their Stockham passes, by the whole workgroup; ends behind a
// barrier. LDS image: spec_lin_fft_lds_floats.
__device__ __forceinline__ SpecLinFft spec_lin_fft_tile_run(const SpecCtx& A, const SpecHeader* H, float* lds, uint32_t ft, uint32_t lgM, uint32_t g,
                                                            uint32_t f0, uint32_t nf) {
  const uint32_t tid = threadIdx.x;
  const uint32_t n = H->n, hop = H->hop, win = H->win, woff = H->woff;
  const uint32_t M = n >> 1;
  float2* s_st = (float2*)lds;  // the per-pass twiddle runs
  float2* s_un = s_st + M;      // s_un[k] = (cos, sin)(2 pi k / n), k <= M
  float2* src = s_un + M + 1u;
  float2* dst = src + (size_t)ft * M;
  const float2* g_tw = (const float2*)(A.tab + H->off_tw);
  const float* g_win = (const float*)(A.tab + H->off_win);
  frames_stockham_twiddles(g_tw, s_st, M, lgM);
  for (uint32_t k = tid; k < M; k += SPEC_THREADS) s_un[k] = g_tw[k];
  // z[m] = v[2m] + i v[2m+1], v[j] = w[j] * y_pad[f hop + j] on the window's support and inside the signal, 0 elsewhere; padded
  // index p is PCM frame p - pad. Frames of the tile past nf are zeros and are never stored.
  const uint64_t T = frames_len(A, g);
  const int64_t pad = (H->opts & VSYN_SPEC_CENTER) ? (int64_t)(n / 2u) : 0;
  const uint32_t C = A.C;
  const float invC = 1.0f / (float)C;
  const float* x = A.pcm + (size_t)g * C * A.plane;
  for (uint32_t q = tid; q < ft * M; q += SPEC_THREADS) {
    const uint32_t f = q >> lgM, m = q & (M - 1u);
    float v[2] = {0.f, 0.f};
    if (f < nf) {
      const int64_t p0 = (int64_t)(f0 + f) * hop - pad;
#pragma unroll
      for (uint32_t c = 0; c < 2u; ++c) {
        const uint32_t j = 2u * m + c;
        const int64_t t = p0 + (int64_t)j;
        if (j >= woff && j - woff < win && t >= 0 && (uint64_t)t < T) v[c] = g_win[j] * pcm_downmix(x, A.plane, C, invC, (uint64_t)t);
      }
    }
    src[q] = make_float2(v[0], v[1]);
  }
  frames_stockham<false>(s_st, src, dst, ft, M, lgM);
  return SpecLinFft{src, s_un, dst};
}

__global__ void __launch_bounds__(SPEC_THREADS) vsyn_spec_lin_fft_kernel(const SpecCtx A, const uint32_t ft, const uint32_t lgM) {
  extern __shared__ float lds[];
  const SpecHeader* H = spec_hdr(A.tab);
  const uint32_t g = blockIdx.y, tid = threadIdx.x;
  const uint32_t F = A.segF[g];
  const uint32_t f0 = blockIdx.x * ft;
  if (f0 >= F) return;
  const uint32_t nb = H->nbins, M = H->n >> 1;
  const uint32_t nf = min(ft, F - f0);
  const SpecLinFft T = spec_lin_fft_tile_run(A, H, lds, ft, lgM, g, f0, nf);
  const uint64_t r0 = A.segoff[g] + f0;
  float mx = -INFINITY;
  for (uint32_t q = tid; q < nf * nb; q += SPEC_THREADS) {
    const uint32_t f = q / nb, k = q - f * nb;
    float re, im;
    spec_lin_untangle(T.Z + (size_t)f * M, T.un, M, k, re, im);
    mx = fmaxf(mx, spec_lin_emit(H, A.rows, r0 + f, k, re, im));
  }
  if (H->kind == VSYN_SPEC_LIN_DB) spec_lin_seg_max(A, g, mx);
}

template <int FT>
__global__ void __launch_bounds__(SPEC_THREADS) vsyn_spec_lin_direct_kernel(const SpecCtx A) {
  extern __shared__ float lds[];
  const SpecHeader* H = spec_hdr(A.tab);
  const uint32_t g = blockIdx.y, tid = threadIdx.x;
  const uint32_t F = A.segF[g];
  const uint32_t f0 = blockIdx.x * FT;
  if (f0 >= F) return;
  const uint32_t nb = H->nbins;
  const uint32_t nf = min((uint32_t)FT, F - f0);
  const FramesDirect D = frames_stage_direct(A, lds, (const float2*)(A.tab + H->off_tw), (const float*)(A.tab + H->off_win), H->n, H->hop,
                                             (uint32_t)spec_span_len(FT, H->n, H->hop), H->win, H->woff, (H->opts & VSYN_SPEC_CENTER) != 0, g, f0);
  __syncthreads();
  const uint64_t r0 = A.segoff[g] + f0;
  float mx = -INFINITY;
  for (uint32_t k = tid; k < nb; k += SPEC_THREADS) {
    float re[FT] = {}, im[FT] = {};
    frames_dft_bin<FT>(D, k, re, im);
#pragma unroll
    for (int f = 0; f < FT; ++f)
      if ((uint32_t)f < nf) mx = fmaxf(mx, spec_lin_emit(H, A.rows, r0 + f, k, re[f], -im[f]));
  }
  if (H->kind == VSYN_SPEC_LIN_DB) spec_lin_seg_max(A, g, mx);
}

// LIN_DB: D = max(D, segment's maximum - top_db), over the segment's F * nbins values; a value that is not finite stays.
__global__ void __launch_bounds__(SPEC_THREADS) vsyn_spec_lin_clamp_kernel(const SpecCtx A) {
  const SpecHeader* H = spec_hdr(A.tab);
  const uint32_t g = blockIdx.y;
  const uint64_t total = (uint64_t)A.segF[g] * H->dim;
  if (total == 0) return;
  const float thr = spec_unkey(A.segmax[g]) - H->top_db;
  float* p = A.rows + A.segoff[g] * H->dim;
  for (uint64_t i = (uint64_t)blockIdx.x * SPEC_THREADS + threadIdx.x; i < total; i += (uint64_t)gridDim.x * SPEC_THREADS) p[i] = spec_floor(p[i], thr);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static inline bool spec_lin_pow2(uint32_t n) { return (n & (n - 1u)) == 0u; }

// Frames per workgroup under sp (a linear kind, checked): the FFT kernel's for a power-of-two n_fft, else the most of the direct
// kernel's that fit the LDS; 0 when nothing fits.
static inline uint32_t spec_lin_tile(const vsyn_spectral_spec* sp) {
  if (spec_lin_pow2(sp->n_fft)) return spec_lin_fft_tile(sp->n_fft);
  for (uint32_t ft : {(uint32_t)SPEC_LIN_DIRECT_FT, 1u})
    if (spec_lin_direct_lds_floats(ft, sp->n_fft, sp->hop_length) * 4u <= SPEC_LDS_BUDGET) return ft;
  return 0;
}

// log2 (n_fft / 2) of a power-of-two n_fft: the FFT kernels' lgM
static inline uint32_t spec_lin_lgm(uint32_t n) {
  uint32_t lgM = 0;
  while ((2u << lgM) < n) ++lgM;
  return lgM;
}

// The linear kinds' kernels behind the offsets kernel: FFT or direct on grid with ft frames per workgroup, and the LIN_DB clamp.
static inline int spec_lin_run(const SpecCtx& A, const vsyn_spectral_spec* sp, uint32_t ft, dim3 grid, uint64_t f_max, hipStream_t s, const char** err) {
  const uint32_t n = sp->n_fft;
  if (spec_lin_pow2(n)) {
    VSYN_LAUNCH(vsyn_spec_lin_fft_kernel, grid, dim3(SPEC_THREADS), spec_lin_fft_lds_floats(ft, n) * 4u, s, A, ft, spec_lin_lgm(n));
  } else {
    const size_t lds = spec_lin_direct_lds_floats(ft, n, sp->hop_length) * 4u;
    if (ft == SPEC_LIN_DIRECT_FT) VSYN_LAUNCH(vsyn_spec_lin_direct_kernel<SPEC_LIN_DIRECT_FT>, grid, dim3(SPEC_THREADS), lds, s, A);
    else VSYN_LAUNCH(vsyn_spec_lin_direct_kernel<1>, grid, dim3(SPEC_THREADS), lds, s, A);
  }
  if (sp->kind == VSYN_SPEC_LIN_DB && sp->top_db > 0.0) {
    const uint64_t cx = std::min<uint64_t>((f_max * (n / 2u + 1u) + SPEC_THREADS - 1) / SPEC_THREADS, 4096);
    VSYN_LAUNCH(vsyn_spec_lin_clamp_kernel, dim3((uint32_t)cx, grid.y), dim3(SPEC_THREADS), 0, s, A);
  }
  return VSYN_OK;
}
