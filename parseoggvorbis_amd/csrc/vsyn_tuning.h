// vsyn_tuning.h — spectral peaks with parabolic interpolation (librosa.piptrack's arithmetic) and the tuning estimate taken from them
// (librosa.estimate_tuning / pitch_tuning), from planar float32 PCM already on the device. Semantics: include/vorbis_synth_hip.h,
// "tuning estimation". Design and measurements: DESIGN.md 6w.
//
// The offsets kernel, the table of the linear kinds (header, twiddles, window, per-segment rate index) and its workspace are those of
// vsyn_spectral.h; behind the rate index the table carries a PipHeader, one PipRate per distinct rate and the histogram's edges
// (SpecHeader.pad holds the PipHeader's offset, as it holds the ChromaHeader's in a chroma table). Behind the offsets kernel, one
// workgroup of 256 threads (4 waves) per (segment, tile of frames), by n_fft alone:
//   vsyn_piptrack_fft_kernel         n_fft a power of two: spec_lin_fft_tile_run (vsyn_spectral_lin.h), then S[f][k] = |X[k]|^power into
//                                    the spare ping-pong buffer, as the chroma kernel keeps it.
//   vsyn_piptrack_direct_kernel<FT>  any other n_fft: frames_stage_direct and frames_dft_bin (vsyn_frames.h) in chunks of 256 bins; the
//                                    whole rows S [FT][NB] stay in LDS (NB floats a frame: they fit at every n_fft), so that the frame's
//                                    maximum is known before the first peak is judged and no chunk needs a halo.
// Both end in pip_rows, one wave per frame: the frame's maximum and its non-finite flag (wave_max, __any), then the bins 64 at a time
// in ascending order, one lane per bin: the threshold, the peak test against the replicated neighbours, the interpolation. Two outputs
// from that one body: dense (F, NB) pitch and magnitude rows (the caller's), and the frame's peaks as (pitch, mag) records, compacted
// by ballot and prefix popcount in ascending k into the frame's own run of the workspace, cap records a frame (peaks are never
// adjacent, so half the searched range bounds them). No atomics, nothing shared between frames.
//   vsyn_tuning_reduce_kernel        one workgroup per segment over its frames' records: the count n of records with pitch > 0, their
//                                    median magnitude by an exact radix selection on the float32 order keys (8 bits a pass, integer
//                                    counts, as vsyn_beat.h selects; both middle ranks from one walk), the histogram of the selected
//                                    records' residuals (integer LDS atomics) and its first arg-max.
// Nothing here reads or writes stream state, the overlap carry or any synthesis buffer; the PCM is only read.
#pragma once
#include <cfloat>

#include "vsyn_spectral_lin.h"

#define PIP_DIRECT_FT 8
#define TUNE_THREADS 256
#define TUNE_WAVES (TUNE_THREADS / 64)
#define TUNE_MAX_BINS 4096u          // the histogram's limit: its counts sit in LDS
#define TUNE_MAX_PEAKS (1ull << 31)  // records a segment may hold: the reduction counts them in 32 bits

struct PipHeader {
  uint32_t cap, nbin, bpo, off_rate, off_edges;  // records a frame; histogram bins; bins per octave; byte offsets into the table
  float thr;                                     // threshold32
  uint32_t pad[2];
};
struct PipRate {  // one distinct sample rate
  double bin_hz;  // sr / n_fft
  uint32_t k_lo, k_hi;
};

struct PipCtx {  // launch arguments
  SpecCtx A;     // rows is not used
  float* pitch;  // row r's NB values at pitch + r * stride, or NULL: no dense rows
  float* mag;
  uint64_t stride;  // floats from a dense row to the next: NB, or 2 NB where a row holds its pitches and then its magnitudes
  float2* rec;      // [segoff[S]][cap] (pitch, mag), or NULL: no records
  uint32_t* cnt;    // [segoff[S]] records of each frame
  double* tuning;   // [S]
  uint64_t* counts; // [S][2]: n, selected
};

__device__ __forceinline__ const PipHeader* pip_hdr(const uint8_t* t) { return (const PipHeader*)(t + spec_hdr(t)->pad); }

// LDS image of the direct kernel, in floats: FramesDirect's head (twiddles [2n] | window [n] | span [(ft-1) hop + n]) | S [ft][NB]
__host__ __device__ __forceinline__ uint64_t pip_direct_lds_floats(uint32_t ft, uint32_t n, uint32_t hop) {
  return 3ull * n + spec_span_len(ft, n, hop) + (uint64_t)ft * (n / 2u + 1u);
}

// Rows r0 .. r0 + nf - 1 from S [nf][stride] in LDS (nb values a frame), one wave per frame. Called by the whole workgroup behind a
// barrier.
__device__ __forceinline__ void pip_rows(const PipCtx& P, const PipHeader* PH, const PipRate R, const float* s_S, uint32_t stride, uint32_t nb, uint32_t nf,
                                         uint64_t r0) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, cap = PH->cap;
  const float qnan = __uint_as_float(0x7FC00000u);
  for (uint32_t f = wave; f < nf; f += SPEC_THREADS / 64u) {  // (wave-uniform; the tile kernels' waves, not the reduction's TUNE_WAVES)
    const float* S = s_S + (size_t)f * stride;
    float mx = 0.f;
    bool bad = false;
    for (uint32_t k = lane; k < nb; k += 64u) {
      const float v = S[k];
      bad |= !(v <= FLT_MAX);  // Inf or NaN (fmaxf would drop a NaN)
      mx = fmaxf(mx, v);
    }
    bad = __any(bad) != 0;
    const float ref = PH->thr * wave_max(mx);
    const uint64_t r = r0 + f;
    uint32_t count = 0u;
    for (uint32_t k0 = 0; k0 < nb; k0 += 64u) {
      const uint32_t k = k0 + lane;
      float pitch = 0.f, mag = 0.f;
      bool peak = false;
      if (k < nb && !bad) {
        const float s0 = S[k], sm = S[k ? k - 1u : 0u], sp = S[k + 1u < nb ? k + 1u : nb - 1u];
        const float z0 = s0 > ref ? s0 : 0.f, zm = sm > ref ? sm : 0.f, zp = sp > ref ? sp : 0.f;
        peak = k >= R.k_lo && k < R.k_hi && z0 > zm && z0 >= zp;
        if (peak) {
          float a = 0.f, s = 0.f;
          if (k >= 1u && k + 1u < nb) {
            a = 0.5f * (sp - sm);
            float b = (2.0f * s0 - sp) - sm;
            if (fabsf(b) < FLT_MIN) b = b + 1.0f;
            s = a / b;
          }
          pitch = (float)(((double)k + (double)s) * R.bin_hz);
          mag = s0 + (0.5f * a) * s;
        }
      }
      if (P.pitch && k < nb) {
        P.pitch[r * P.stride + k] = bad ? qnan : pitch;
        P.mag[r * P.stride + k] = bad ? qnan : mag;
      }
      if (P.rec) {
        const unsigned long long m = __ballot(peak);
        const uint32_t pos = count + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (peak && pos < cap) P.rec[r * cap + pos] = make_float2(pitch, mag);
        count += (uint32_t)__popcll(m);
      }
    }
    if (P.rec && lane == 0u) P.cnt[r] = min(count, cap);
  }
}

__device__ __forceinline__ PipRate pip_rate(const uint8_t* tab, const SpecHeader* H, const PipHeader* PH, uint32_t g) {
  const uint32_t ri = ((const uint32_t*)(tab + H->off_rate))[g];
  return ((const PipRate*)(tab + PH->off_rate))[ri];
}

__global__ void __launch_bounds__(SPEC_THREADS) vsyn_piptrack_fft_kernel(const PipCtx P, const uint32_t ft, const uint32_t lgM) {
  extern __shared__ float lds[];
  const SpecCtx& A = P.A;
  const SpecHeader* H = spec_hdr(A.tab);
  const PipHeader* PH = pip_hdr(A.tab);
  const uint32_t g = blockIdx.y, tid = threadIdx.x;
  const uint32_t F = A.segF[g];
  const uint32_t f0 = blockIdx.x * ft;
  if (f0 >= F) return;
  const uint32_t n = H->n, nb = H->nbins, M = n >> 1;
  const uint32_t nf = min(ft, F - f0);
  const SpecLinFft T = spec_lin_fft_tile_run(A, H, lds, ft, lgM, g, f0, nf);
  float* s_S = (float*)T.spare;  // [nf][nb]: nf nb <= ft n floats, the buffer's size
  for (uint32_t q = tid; q < nf * nb; q += SPEC_THREADS) {
    const uint32_t f = q / nb, k = q - f * nb;
    float re, im;
    spec_lin_untangle(T.Z + (size_t)f * M, T.un, M, k, re, im);
    const float p = fmaf(re, re, im * im);
    s_S[q] = H->power == 1 ? sqrtf(p) : p;
  }
  __syncthreads();
  pip_rows(P, PH, pip_rate(A.tab, H, PH, g), s_S, nb, nb, nf, A.segoff[g] + f0);
}

template <int FT>
__global__ void __launch_bounds__(SPEC_THREADS) vsyn_piptrack_direct_kernel(const PipCtx P) {
  extern __shared__ float lds[];
  const SpecCtx& A = P.A;
  const SpecHeader* H = spec_hdr(A.tab);
  const PipHeader* PH = pip_hdr(A.tab);
  const uint32_t g = blockIdx.y, tid = threadIdx.x;
  const uint32_t F = A.segF[g];
  const uint32_t f0 = blockIdx.x * FT;
  if (f0 >= F) return;
  const uint32_t nb = H->nbins;
  const uint32_t nf = min((uint32_t)FT, F - f0);
  const FramesDirect D = frames_stage_direct(A, lds, (const float2*)(A.tab + H->off_tw), (const float*)(A.tab + H->off_win), H->n, H->hop,
                                             (uint32_t)spec_span_len(FT, H->n, H->hop), H->win, H->woff, (H->opts & VSYN_SPEC_CENTER) != 0, g, f0);
  float* s_S = D.rest;  // [FT][nb]
  __syncthreads();
  for (uint32_t k = tid; k < nb; k += SPEC_THREADS) {
    float re[FT] = {}, im[FT] = {};
    frames_dft_bin<FT>(D, k, re, im);
#pragma unroll
    for (int f = 0; f < FT; ++f) {
      const float p = fmaf(re[f], re[f], im[f] * im[f]);
      s_S[(uint32_t)f * nb + k] = H->power == 1 ? sqrtf(p) : p;
    }
  }
  __syncthreads();
  pip_rows(P, PH, pip_rate(A.tab, H, PH, g), s_S, nb, nb, nf, A.segoff[g] + f0);
}

// ------------------------------------------------------------------------------------------------
// the reduction
// ------------------------------------------------------------------------------------------------
// r of "tuning estimation" step 7 and its bin of the nbin + 1 edges e, or nbin when r lies in none: shared by the device and the host.
__host__ __device__ __forceinline__ uint32_t tune_bin(float pitch, uint32_t bpo, uint32_t nbin, const double* e) {
  double r = fmod((double)bpo * log2((double)pitch / 27.5), 1.0);
  if (r >= 0.5) r -= 1.0;
  const double t = floor((r + 0.5) * (double)nbin);
  uint32_t i = t < 0.0 ? 0u : t >= (double)nbin ? nbin - 1u : (uint32_t)t;
  if (r < e[i]) {  // the table decides: at most one bin off
    if (i > 0u) --i;
  } else if (r >= e[i + 1u] && i + 1u < nbin) {
    ++i;
  }
  return e[i] <= r && r < e[i + 1u] ? i : nbin;
}

// Every record of the segment with pitch > 0, one wave per frame, the lanes along the frame's run: fn(pitch, mag).
template <class Fn>
__device__ __forceinline__ void tune_each(const PipCtx& P, uint64_t r0, uint32_t F, uint32_t cap, Fn fn) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  for (uint32_t f = wave; f < F; f += TUNE_WAVES) {
    const uint32_t c = min(P.cnt[r0 + f], cap);
    const float2* rec = P.rec + (r0 + f) * cap;
    for (uint32_t j = lane; j < c; j += 64u) {
      const float2 v = rec[j];
      if (v.x > 0.f) fn(v.x, v.y);
    }
  }
}

// The magnitude keys of the ranks rank_a <= rank_b (0: the smallest) among the records with pitch > 0, from one walk: four passes,
// most significant byte first, one sweep over the records each. A pass keeps one histogram per prefix; while the two ranks still share
// their prefix (the common case: the two middle elements of a segment's magnitudes) the second is not counted and the first serves both.
__device__ void tune_select2(const PipCtx& P, uint64_t r0, uint32_t F, uint32_t cap, uint32_t rank_a, uint32_t rank_b, uint32_t* s_hist,
                             uint32_t* s_pick, uint32_t (&key)[2]) {
  uint32_t prefix[2] = {0u, 0u}, rank[2] = {rank_a, rank_b};
  for (int shift = 24; shift >= 0; shift -= 8) {
    const uint32_t himask = shift == 24 ? 0u : ~0u << (shift + 8);
    const bool apart = prefix[0] != prefix[1];  // (workgroup-uniform)
    __syncthreads();  // (the histograms and the picks are free)
    for (uint32_t b = threadIdx.x; b < 512u; b += TUNE_THREADS) s_hist[b] = 0u;
    __syncthreads();
    tune_each(P, r0, F, cap, [&](float, float mag) {
      const uint32_t k = spec_key(mag);
      if ((k & himask) == prefix[0]) atomicAdd(&s_hist[(k >> shift) & 255u], 1u);
      if (apart && (k & himask) == prefix[1]) atomicAdd(&s_hist[256u + ((k >> shift) & 255u)], 1u);
    });
    __syncthreads();
    if (threadIdx.x < 2u) {
      const uint32_t* hist = s_hist + (apart && threadIdx.x ? 256u : 0u);
      uint32_t b = 0u, r = rank[threadIdx.x];
      while (b < 255u && r >= hist[b]) r -= hist[b++];
      s_pick[2u * threadIdx.x] = b;
      s_pick[2u * threadIdx.x + 1u] = r;
    }
    __syncthreads();
    for (uint32_t i = 0; i < 2u; ++i) {
      prefix[i] |= s_pick[2u * i] << shift;
      rank[i] = s_pick[2u * i + 1u];
    }
  }
  key[0] = prefix[0];
  key[1] = prefix[1];
}

__global__ void __launch_bounds__(TUNE_THREADS) vsyn_tuning_reduce_kernel(const PipCtx P) {
  __shared__ uint32_t s_hist[TUNE_MAX_BINS];
  __shared__ uint32_t s_pick[4];
  __shared__ uint32_t s_r32[TUNE_WAVES];
  __shared__ uint64_t s_r64[TUNE_WAVES];
  const uint32_t g = blockIdx.x, tid = threadIdx.x;
  const PipHeader* PH = pip_hdr(P.A.tab);
  const uint32_t F = P.A.segF[g], cap = PH->cap, nbin = PH->nbin, bpo = PH->bpo;
  const uint64_t r0 = P.A.segoff[g];
  const double* e = (const double*)(P.A.tab + PH->off_edges);
  uint32_t c = 0u;
  tune_each(P, r0, F, cap, [&](float, float) { ++c; });
  const uint32_t n = wg_reduce_all<TUNE_WAVES>(c, s_r32, WaveSum(), 0u);
  if (n == 0u) {  // (workgroup-uniform)
    if (tid == 0u) {
      P.tuning[g] = 0.0;
      P.counts[2u * g] = 0ull;
      P.counts[2u * g + 1u] = 0ull;
    }
    return;
  }
  uint32_t mid[2];  // the middle element, or the two of an even count
  tune_select2(P, r0, F, cap, (n - 1u) / 2u, n / 2u, s_hist, s_pick, mid);
  const float thr = (n & 1u) ? spec_unkey(mid[0]) : (spec_unkey(mid[0]) + spec_unkey(mid[1])) / 2.0f;
  __syncthreads();
  for (uint32_t b = tid; b < nbin; b += TUNE_THREADS) s_hist[b] = 0u;
  __syncthreads();
  c = 0u;
  tune_each(P, r0, F, cap, [&](float pitch, float mag) {
    if (!(mag >= thr)) return;
    ++c;
    const uint32_t i = tune_bin(pitch, bpo, nbin, e);
    if (i < nbin) atomicAdd(&s_hist[i], 1u);
  });
  const uint32_t sel = wg_reduce_all<TUNE_WAVES>(c, s_r32, WaveSum(), 0u);  // (its barriers stand behind the histogram as well)
  uint64_t best = 0ull;  // (count, nbin's complement of the bin): the largest count, and among equals the first bin
  for (uint32_t b = tid; b < nbin; b += TUNE_THREADS) best = WaveMax()(best, ((uint64_t)s_hist[b] << 32) | (uint64_t)(0xFFFFFFFFu - b));
  best = wg_reduce_all<TUNE_WAVES>(best, s_r64, WaveMax(), 0ull);
  if (tid == 0u) {
    P.tuning[g] = e[0xFFFFFFFFu - (uint32_t)best];
    P.counts[2u * g] = n;
    P.counts[2u * g + 1u] = sel;
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct TuningWs {  // the stage's own buffers; the table, the frame counts and the row offsets are the spectral stage's (SpectralWs)
  DevBuf<float2> rec;
  DevBuf<uint32_t> cnt;
  DevBuf<double> tuning;
  DevBuf<uint64_t> counts;
};

static inline uint32_t tune_nbin(double resolution) { return (uint32_t)ceil(1.0 / resolution); }

// The checks of "tuning estimation" step 9: the spectral spec as for a linear kind, which it must be, then the estimator's own.
static inline int tuning_check(const vsyn_spectral_spec* sp, const vsyn_tuning_spec* tu, uint32_t S, const uint32_t* rates, const char** err) {
  if (int rc = spec_check(sp, S, rates, err)) return rc;
  if (sp->kind != VSYN_SPEC_LIN_POWER) return fail(err, VSYN_ERR_INVALID, "tuning estimation takes a lin_power spec (kind %u given)", sp->kind);
  if (!tu) return fail(err, VSYN_ERR_INVALID, "tuning spec is NULL");
  if (tu->reserved) return fail(err, VSYN_ERR_INVALID, "tuning spec: reserved must be 0");
  if (!std::isfinite(tu->fmin) || !std::isfinite(tu->fmax)) return fail(err, VSYN_ERR_INVALID, "tuning fmin / fmax must be finite");
  if (!(tu->fmax > std::max(tu->fmin, 0.0))) return fail(err, VSYN_ERR_INVALID, "tuning fmax %g not above fmin %g", tu->fmax, std::max(tu->fmin, 0.0));
  if (!std::isfinite(tu->threshold) || tu->threshold < 0.0) return fail(err, VSYN_ERR_INVALID, "tuning threshold must be finite and >= 0");
  if (!std::isfinite(tu->resolution) || !(tu->resolution > 0.0 && tu->resolution < 1.0))
    return fail(err, VSYN_ERR_INVALID, "tuning resolution must be inside (0, 1)");
  if (ceil(1.0 / tu->resolution) > (double)TUNE_MAX_BINS)
    return fail(err, VSYN_ERR_INVALID, "tuning resolution %g needs more than %u histogram bins", tu->resolution, TUNE_MAX_BINS);
  if (tu->bins_per_octave < 1 || tu->bins_per_octave > 256)
    return fail(err, VSYN_ERR_INVALID, "tuning bins_per_octave %u outside [1, 256]", tu->bins_per_octave);
  return VSYN_OK;
}

// [k_lo, k_hi) of step 2 at rate sr: the bins k < NB with fmin' <= k sr / n_fft < fmax'; k_lo = k_hi = 0 when there is none.
static inline void pip_bins(uint32_t sr, uint32_t n, const vsyn_tuning_spec* tu, uint32_t out[2]) {
  const double lo = std::max(tu->fmin, 0.0), hi = std::min(tu->fmax, (double)sr / 2.0);
  out[0] = out[1] = 0u;
  for (uint32_t k = 0; k < n / 2u + 1u; ++k) {
    const double fk = (double)k * (double)sr / (double)n;
    if (!(lo <= fk && fk < hi)) continue;
    if (out[1] == 0u) out[0] = k;
    out[1] = k + 1u;
  }
}

// e_i = -0.5 + i (1 / nbin), i <= nbin
static inline void tune_edges(uint32_t nbin, double* e) {
  const double w = 1.0 / (double)nbin;
  for (uint32_t i = 0; i <= nbin; ++i) e[i] = -0.5 + (double)i * w;
}

// The reduction of steps 5 to 8 on host arrays (vsyn_pitch_tuning): mags NULL selects every entry with freqs > 0.
static inline int tune_host(const float* freqs, const float* mags, uint64_t n, double resolution, uint32_t bpo, double* tuning, uint64_t counts[2]) {
  std::vector<uint64_t> P;
  for (uint64_t i = 0; i < n; ++i)
    if (freqs[i] > 0.f) P.push_back(i);
  if (P.size() > TUNE_MAX_PEAKS) return VSYN_ERR_INVALID;
  *tuning = 0.0;
  counts[0] = P.size();
  counts[1] = 0;
  if (P.empty()) return VSYN_OK;
  float thr = -INFINITY;
  if (mags) {
    std::vector<float> m(P.size());
    for (size_t i = 0; i < P.size(); ++i) m[i] = mags[P[i]];
    std::sort(m.begin(), m.end());
    const size_t c = m.size();
    thr = (c & 1u) ? m[(c - 1u) / 2u] : (m[(c - 1u) / 2u] + m[c / 2u]) / 2.0f;
  }
  const uint32_t nbin = tune_nbin(resolution);
  std::vector<double> e(nbin + 1u);
  tune_edges(nbin, e.data());
  std::vector<uint64_t> hist(nbin, 0);
  for (uint64_t i : P) {
    if (mags && !(mags[i] >= thr)) continue;
    ++counts[1];
    const uint32_t b = tune_bin(freqs[i], bpo, nbin, e.data());
    if (b < nbin) ++hist[b];
  }
  uint32_t best = 0;
  for (uint32_t b = 1; b < nbin; ++b)
    if (hist[b] > hist[best]) best = b;
  *tuning = e[best];
  return VSYN_OK;
}

// Frames per workgroup under sp (lin_power, checked): the FFT kernel's for a power-of-two n_fft, else the most of the direct
// kernel's that fit the LDS; 0 when nothing fits.
static inline uint32_t pip_tile(const vsyn_spectral_spec* sp) {
  if (spec_lin_pow2(sp->n_fft)) return spec_lin_fft_tile(sp->n_fft);
  for (uint32_t ft : {(uint32_t)PIP_DIRECT_FT, 1u})
    if (pip_direct_lds_floats(ft, sp->n_fft, sp->hop_length) * 4u <= SPEC_LDS_BUDGET) return ft;
  return 0;
}

// The estimator's block behind tab (the linear kinds' table of sp): PipHeader, one PipRate per rate of distinct (spec_build_table's
// list, in the order of the table's rate indices), the edges. Returns cap, the records a frame may need.
static inline uint32_t pip_table(const vsyn_spectral_spec* sp, const vsyn_tuning_spec* tu, const std::vector<uint32_t>& distinct, std::vector<uint8_t>& tab) {
  const uint32_t n = sp->n_fft, nbin = tune_nbin(tu->resolution);
  SpecHeader T;
  memcpy(&T, tab.data(), sizeof(T));
  const size_t off_h = (tab.size() + 15) & ~(size_t)15;
  const size_t off_rate = off_h + sizeof(PipHeader);
  const size_t off_edges = off_rate + sizeof(PipRate) * distinct.size();
  tab.resize(off_edges + 8ull * (nbin + 1u) + 16, 0);
  uint32_t cap = 1u;
  std::vector<PipRate> pr(distinct.size());
  for (size_t r = 0; r < distinct.size(); ++r) {
    uint32_t kk[2];
    pip_bins(distinct[r], n, tu, kk);
    pr[r].bin_hz = (double)distinct[r] / (double)n;
    pr[r].k_lo = kk[0];
    pr[r].k_hi = kk[1];
    cap = std::max(cap, (kk[1] - kk[0] + 1u) / 2u);  // peaks are never adjacent
  }
  T.pad = (uint32_t)off_h;
  memcpy(tab.data(), &T, sizeof(T));
  PipHeader PH = {};
  PH.cap = cap;
  PH.nbin = nbin;
  PH.bpo = tu->bins_per_octave;
  PH.off_rate = (uint32_t)off_rate;
  PH.off_edges = (uint32_t)off_edges;
  PH.thr = (float)tu->threshold;
  memcpy(tab.data() + off_h, &PH, sizeof(PH));
  if (!pr.empty()) memcpy(tab.data() + off_rate, pr.data(), sizeof(PipRate) * pr.size());
  tune_edges(nbin, (double*)(tab.data() + off_edges));
  return cap;
}

static inline int spec_raise_lds(SpectralWs& ws, const char** err);  // vsyn_chroma.h: the dynamic-LDS limit of every tile kernel

// The stage on stream s: the offsets kernel, the tile kernel (FFT or direct), and with d_tuning the reduction. d_pitch / d_mag (both or
// neither) take the dense rows, row_stride floats apart, d_tuning / d_counts (both or neither) the estimate; frames from d_frames, else from si. f_max bounds
// every segment's STFT frames. Caller holds the handle's lock and has run tuning_check.
static inline int pip_launch(SpectralWs& ws, TuningWs& tw, int device, const vsyn_spectral_spec* sp, const vsyn_tuning_spec* tu, uint32_t S,
                             const uint32_t* rates, const float* d_pcm, uint64_t plane, uint32_t C, const uint32_t* d_frames, const SegInfo* si,
                             uint64_t f_max, float* d_pitch, float* d_mag, uint64_t row_stride, uint64_t* d_segoff, double* d_tuning, uint64_t* d_counts, hipStream_t s,
                             const char** err) {
  if (S > 65535u) return fail(err, VSYN_ERR_INVALID, "too many segments (%u > 65535)", S);
  const uint32_t ft = pip_tile(sp), n = sp->n_fft;
  if (!ft) return fail(err, VSYN_ERR_INVALID, "n_fft %u / hop_length %u do not fit the LDS", n, sp->hop_length);
  std::vector<uint8_t> tab;
  std::vector<uint32_t> distinct;
  spec_build_table(sp, S, rates, tab, &distinct);
  const uint32_t cap = pip_table(sp, tu, distinct, tab);
  if (d_tuning && f_max * cap > TUNE_MAX_PEAKS)
    return fail(err, VSYN_ERR_INVALID, "a segment of %llu frames could hold more than 2^31 peaks", (unsigned long long)f_max);
  HIPCHK(hipSetDevice(device));
  if (int rc = spec_raise_lds(ws, err)) return rc;
  HIPCHK(ws.segF.ensure(S));
  HIPCHK(ws.segmax.ensure(S));
  HIPCHK(ws.segoff.ensure((size_t)S + 1));
  if (d_tuning) {
    HIPCHK(tw.rec.ensure((size_t)S * f_max * cap + 1));
    HIPCHK(tw.cnt.ensure((size_t)S * f_max + 1));
  }
  if (int rc = ws.tab.upload(tab, s, err)) return rc;
  PipCtx P;
  P.A.tab = ws.tab.dev.p;
  P.A.pcm = d_pcm;
  P.A.plane = plane;
  P.A.C = C;
  P.A.S = S;
  P.A.frames = d_frames;
  P.A.si = si;
  P.A.segF = ws.segF.p;
  P.A.segoff = d_segoff ? d_segoff : ws.segoff.p;
  P.A.segmax = ws.segmax.p;
  P.A.rows = nullptr;
  P.A.db = nullptr;
  P.pitch = d_pitch;
  P.mag = d_mag;
  P.stride = row_stride;
  P.rec = d_tuning ? tw.rec.p : nullptr;
  P.cnt = d_tuning ? tw.cnt.p : nullptr;
  P.tuning = d_tuning;
  P.counts = d_counts;
  VSYN_LAUNCH(vsyn_spec_offsets_kernel, dim3(1), dim3(SPEC_THREADS), 0, s, P.A);
  if (S == 0) return VSYN_OK;
  if (f_max) {
    const uint64_t gx = (f_max + ft - 1) / ft;
    if (gx > 0x7FFFFFFFull) return fail(err, VSYN_ERR_INVALID, "segment too long");
    const dim3 grid((uint32_t)gx, S);
    if (spec_lin_pow2(n)) {
      VSYN_LAUNCH(vsyn_piptrack_fft_kernel, grid, dim3(SPEC_THREADS), spec_lin_fft_lds_floats(ft, n) * 4u, s, P, ft, spec_lin_lgm(n));
    } else {
      const size_t lds = pip_direct_lds_floats(ft, n, sp->hop_length) * 4u;
      if (ft == PIP_DIRECT_FT) VSYN_LAUNCH(vsyn_piptrack_direct_kernel<PIP_DIRECT_FT>, grid, dim3(SPEC_THREADS), lds, s, P);
      else VSYN_LAUNCH(vsyn_piptrack_direct_kernel<1>, grid, dim3(SPEC_THREADS), lds, s, P);
    }
  }
  if (d_tuning) VSYN_LAUNCH(vsyn_tuning_reduce_kernel, dim3(S), dim3(TUNE_THREADS), 0, s, P);
  return VSYN_OK;
}
