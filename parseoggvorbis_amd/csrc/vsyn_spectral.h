// vsyn_spectral.h — mel filterbank / log-mel / dB-mel / MFCC rows from planar float32 PCM already on the device.
// Semantics: include/vorbis_synth_hip.h, "spectral features".
//
// Three kernels on one stream (tables built on the host in double, vorbis_synth_hip.hip spec_build_table):
//   1. vsyn_spec_offsets_kernel  one workgroup: per segment its PCM frames (the caller's d_frames, or the last submit's SegInfo),
//                                its STFT frame count, the exclusive row scan seg_off[S+1]; clears the per-segment dB maxima.
//   2. vsyn_spec_stft_kernel<FT> one workgroup per (segment, tile of FT frames). LDS holds the twiddles cos/sin(2 pi m / n_fft)
//                                (m < n_fft), the window, and the tile's span of the mono signal (the downmix is done while
//                                loading it). A thread owns one bin k of a 256-bin chunk and accumulates the FT frames' real DFT
//                                sums, walking the twiddle index by (j * k) mod n_fft; the chunk's |X|^power goes to LDS and the
//                                mel bands that overlap the chunk take their share from it (sparse per-band weights). The last
//                                chunk ends in the kind's output: M, log10, or 10 log10 (with a per-segment max by atomicMax on
//                                order-preserving integer keys).
//   3. vsyn_spec_finish_kernel   MEL_DB / MFCC only, after 2: the top_db clamp against the segment's max, and for MFCC the
//                                orthonormal DCT-II (host-built matrix) of the clamped dB rows.
// Nothing here reads or writes stream state, the overlap carry or any synthesis buffer; the PCM is only read.
#pragma once
#include "vsyn_device.h"

struct SpecHeader {
  uint32_t kind, opts, n, hop, win, woff, nbins, n_mels;
  uint32_t dim, n_mfcc, power, num_rates, S;
  uint32_t off_tw, off_win, off_band, off_w, off_dct, off_rate;  // byte offsets into the table
  uint32_t pad;
  float log_floor, amin, top_db, pad2;
};
struct SpecBand {  // one mel band of one sample rate: weights w[woff .. woff + cnt) for bins first .. first + cnt - 1
  uint32_t first, cnt, woff, pad;
};
#define SPEC_SKIP 0xFFFFFFFFu  // seg_rate entry of a segment without rows (sample rate 0)

struct SpecCtx {  // launch arguments
  const uint8_t* tab;
  const float* pcm;
  uint64_t plane;
  uint32_t C, S;
  const uint32_t* frames;  // PCM frames per segment (caller's), or
  const SegInfo* si;       // the last submit's SegInfo (total_emit)
  uint32_t* segF;          // [S] STFT frames
  uint64_t* segoff;        // [S+1]
  uint32_t* segmax;        // [S] max dB as an order-preserving key
  float* rows;             // [segoff[S]][dim]
  float* db;               // MFCC: [segoff[S]][n_mels] dB rows before the clamp
};

#define SPEC_THREADS 256
#define SPEC_FIN_ROWS 16

__device__ __forceinline__ const SpecHeader* spec_hdr(const uint8_t* t) { return (const SpecHeader*)t; }

__host__ __device__ __forceinline__ uint64_t spec_num_frames(uint32_t n, uint32_t hop, bool center, uint64_t T) {
  if (T == 0) return 0;
  const uint64_t tp = T + (center ? 2ull * (n / 2u) : 0ull);
  return tp < n ? 0ull : 1ull + (tp - n) / hop;
}

// float -> uint32 with the same order (no NaN here: every dB value is a finite log of a value >= amin > 0)
__device__ __forceinline__ uint32_t spec_key(float x) {
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float spec_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

__global__ void __launch_bounds__(SPEC_THREADS) vsyn_spec_offsets_kernel(const SpecCtx A) {
  const SpecHeader* H = spec_hdr(A.tab);
  const uint32_t* rate = (const uint32_t*)(A.tab + H->off_rate);
  wg_exclusive_scan<SPEC_THREADS, 1>(A.S, A.segoff, [&](uint32_t g, uint64_t* v) {
    const uint64_t T = min((uint64_t)(A.frames ? A.frames[g] : A.si[g].total_emit), A.plane);
    v[0] = rate[g] == SPEC_SKIP ? 0ull : spec_num_frames(H->n, H->hop, (H->opts & VSYN_SPEC_CENTER) != 0, T);
    A.segF[g] = (uint32_t)v[0];
    A.segmax[g] = 0u;  // below every key
  });
}

// LDS image of the STFT kernel, in floats: twiddles [2n] | window [n] | span [(FT-1) hop + n] | |X|^power [FT][256] | M [FT][n_mels]
__host__ __device__ __forceinline__ uint64_t spec_span_len(uint32_t ft, uint32_t n, uint32_t hop) { return (uint64_t)(ft - 1u) * hop + n; }
__host__ __device__ __forceinline__ uint64_t spec_lds_floats(uint32_t ft, uint32_t n, uint32_t hop, uint32_t n_mels) {
  return 3ull * n + spec_span_len(ft, n, hop) + (uint64_t)ft * SPEC_THREADS + (uint64_t)ft * n_mels;
}

template <int FT>
__global__ void __launch_bounds__(SPEC_THREADS) vsyn_spec_stft_kernel(const SpecCtx A) {
  extern __shared__ float lds[];
  const SpecHeader* H = spec_hdr(A.tab);
  const uint32_t g = blockIdx.y, tid = threadIdx.x;
  const uint32_t F = A.segF[g];
  const uint32_t f0 = blockIdx.x * FT;
  if (f0 >= F) return;
  const uint32_t n = H->n, hop = H->hop, nb = H->nbins, NM = H->n_mels, win = H->win, woff = H->woff;
  const uint32_t nf = min((uint32_t)FT, F - f0);
  const uint32_t ri = ((const uint32_t*)(A.tab + H->off_rate))[g];
  const SpecBand* band = (const SpecBand*)(A.tab + H->off_band) + (size_t)ri * NM;
  const float* wts = (const float*)(A.tab + H->off_w);
  float2* s_tw = (float2*)lds;
  float* s_win = lds + 2u * n;
  float* s_span = s_win + n;
  const uint32_t span = (uint32_t)spec_span_len(FT, n, hop);
  float* s_S = s_span + span;
  float* s_M = s_S + FT * SPEC_THREADS;
  const float2* g_tw = (const float2*)(A.tab + H->off_tw);
  const float* g_win = (const float*)(A.tab + H->off_win);
  for (uint32_t i = tid; i < n; i += SPEC_THREADS) {
    s_tw[i] = g_tw[i];
    s_win[i] = g_win[i];
  }
  // the tile's span of the padded mono signal: padded index p = f0 * hop + i is PCM frame p - pad (zero outside [0, T));
  // frames of the tile past nf read the zero-filled rest and are never stored
  const uint64_t T = min((uint64_t)(A.frames ? A.frames[g] : A.si[g].total_emit), A.plane);
  const int64_t pad = (H->opts & VSYN_SPEC_CENTER) ? (int64_t)(n / 2u) : 0;
  const int64_t p0 = (int64_t)f0 * hop - pad;
  const uint32_t C = A.C;
  const float invC = 1.0f / (float)C;
  const float* x = A.pcm + (size_t)g * C * A.plane;
  for (uint32_t i = tid; i < span; i += SPEC_THREADS) {
    const int64_t t = p0 + (int64_t)i;
    s_span[i] = (t >= 0 && (uint64_t)t < T) ? pcm_downmix(x, A.plane, C, invC, (uint64_t)t) : 0.f;
  }
  for (uint32_t i = tid; i < FT * NM; i += SPEC_THREADS) s_M[i] = 0.f;
  __syncthreads();

  for (uint32_t k0 = 0; k0 < nb; k0 += SPEC_THREADS) {
    const uint32_t k = k0 + tid;
    float re[FT], im[FT];
#pragma unroll
    for (int f = 0; f < FT; ++f) re[f] = im[f] = 0.f;
    if (k < nb) {
      uint32_t idx = (uint32_t)(((uint64_t)woff * k) % n);
      for (uint32_t j = woff; j < woff + win; ++j) {
        const float2 tw = s_tw[idx];
        const float w = s_win[j];
        const float a = w * tw.x, b = w * tw.y;
        const float* sp = s_span + j;
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
#pragma unroll
    for (int f = 0; f < FT; ++f) {
      const float p = fmaf(re[f], re[f], im[f] * im[f]);
      s_S[f * SPEC_THREADS + tid] = H->power == 1 ? sqrtf(p) : p;
    }
    __syncthreads();
    const uint32_t kend = min(k0 + SPEC_THREADS, nb);
    for (uint32_t q = tid; q < nf * NM; q += SPEC_THREADS) {
      const uint32_t f = q / NM, m = q - f * NM;
      const SpecBand bd = band[m];
      const uint32_t lo = max(bd.first, k0), hi = min(bd.first + bd.cnt, kend);
      float acc = s_M[f * NM + m];
      for (uint32_t kk = lo; kk < hi; ++kk) acc = fmaf(wts[bd.woff + (kk - bd.first)], s_S[f * SPEC_THREADS + (kk - k0)], acc);
      s_M[f * NM + m] = acc;
    }
    __syncthreads();
  }

  const uint64_t r0 = A.segoff[g] + f0;
  const uint32_t kind = H->kind;
  float mx = -INFINITY;
  for (uint32_t q = tid; q < nf * NM; q += SPEC_THREADS) {
    const uint32_t f = q / NM, m = q - f * NM;
    const float M = s_M[q];
    const uint64_t r = r0 + f;
    if (kind == VSYN_SPEC_MEL_POWER) {
      A.rows[r * NM + m] = M;
    } else if (kind == VSYN_SPEC_LOG_MEL) {
      A.rows[r * NM + m] = log10f(fmaxf(M, H->log_floor));
    } else {
      const float d = 10.0f * log10f(fmaxf(M, H->amin));
      mx = fmaxf(mx, d);
      if (kind == VSYN_SPEC_MEL_DB) A.rows[r * NM + m] = d;
      else A.db[r * NM + m] = d;
    }
  }
  if (kind >= VSYN_SPEC_MEL_DB) {
    for (int o = 32; o; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((tid & 63u) == 0 && mx > -INFINITY) atomicMax(A.segmax + g, spec_key(mx));
  }
}

// MEL_DB: the top_db clamp in place. MFCC: out[r][i] = sum_m dct[i][m] * max(D[r][m], thr), m ascending.
__global__ void __launch_bounds__(SPEC_THREADS) vsyn_spec_finish_kernel(const SpecCtx A) {
  __shared__ float s_d[SPEC_FIN_ROWS * 256];
  const SpecHeader* H = spec_hdr(A.tab);
  const uint32_t g = blockIdx.y, tid = threadIdx.x;
  const uint32_t F = A.segF[g], f0 = blockIdx.x * SPEC_FIN_ROWS;
  if (f0 >= F) return;
  const uint32_t nf = min((uint32_t)SPEC_FIN_ROWS, F - f0), NM = H->n_mels;
  const float thr = H->top_db > 0.f ? spec_unkey(A.segmax[g]) - H->top_db : -INFINITY;
  const uint64_t r0 = A.segoff[g] + f0;
  if (H->kind == VSYN_SPEC_MEL_DB) {
    for (uint32_t q = tid; q < nf * NM; q += SPEC_THREADS) {
      float* p = A.rows + r0 * NM + q;
      *p = fmaxf(*p, thr);
    }
    return;
  }
  for (uint32_t q = tid; q < nf * NM; q += SPEC_THREADS) s_d[q] = fmaxf(A.db[r0 * NM + q], thr);
  __syncthreads();
  const uint32_t D = H->n_mfcc;
  const float* dct = (const float*)(A.tab + H->off_dct);
  for (uint32_t q = tid; q < nf * D; q += SPEC_THREADS) {
    const uint32_t f = q / D, i = q - f * D;
    const float* row = s_d + f * NM;
    const float* c = dct + (size_t)i * NM;
    float acc = 0.f;
    for (uint32_t m = 0; m < NM; ++m) acc = fmaf(c[m], row[m], acc);
    A.rows[(r0 + f) * D + i] = acc;
  }
}
