// vsyn_chroma.h — chroma rows (librosa.feature.chroma_stft's arithmetic) and the tonnetz rows computed from them, from planar float32
// PCM already on the device. Semantics: include/vorbis_synth_hip.h, "chroma". Design, bound and measurements: DESIGN.md 6n.
//
// The offsets kernel, the table of the linear kinds (header, twiddles, window, per-segment rate index) and the workspace are those of
// vsyn_spectral.h; behind the rate index the table carries a ChromaHeader, the dense float32 filterbank [rate][n_chroma][NB] and
// phi [6][n_chroma] (SpecHeader.pad holds the ChromaHeader's offset; it is 0 in every other kind's table). With estimated tunings
// (spec_launch's seg_tuning) there is one filterbank per distinct (rate, tuning) pair and a per-segment bank index behind phi. Behind the offsets kernel,
// one workgroup of 256 threads (4 waves) per (segment, tile of frames), by n_fft alone:
//   vsyn_chroma_fft_kernel         n_fft a power of two: spec_lin_fft_tile_run (vsyn_spectral_lin.h), then S[f][k] = |X[k]|^power into
//                                  the spare ping-pong buffer instead of a store of the bins.
//   vsyn_chroma_direct_kernel<FT>  any other n_fft: frames_stage_direct, then frames_dft_bin and frames_power_store (vsyn_frames.h) in chunks
//                                  of 256 bins, S of a chunk in LDS, as the mel kernel (vsyn_spectral.h) runs them.
// Both project with chroma_dot, one wave per (frame, c): lane l runs one fma chain over the bins l, l + 64, ... (ascending) of the
// whole row (FFT kernel) or of the chunk (direct kernel, the chunks' sums added to R[f][c] in ascending order), W read from global
// memory along k, S from LDS, then wave_sum (the butterfly of DESIGN.md 6t). chroma_finish then takes each frame's norm, the
// non-finite rule and, for tonnetz, the 6 x n_chroma product, one wave per frame. No atomics; S and R never leave the workgroup.
// The last of the spectral kinds' headers: behind the chroma kinds' share of the host side stands spec_launch, the one preamble of
// every spectral kind, which sees all three.
// Nothing here reads or writes stream state, the overlap carry or any synthesis buffer; the PCM is only read.
#pragma once
#include <cfloat>

#include "vsyn_spectral_lin.h"
#include "vsyn_tuning.h"  // its tile kernels stand in spec_raise_lds' list

#define CHROMA_DIRECT_FT 8
#define CHROMA_MAX 256  // n_chroma's limit; the LDS images reserve a row of it per frame, so that the tile depends on the spec alone

struct ChromaHeader {
  uint32_t n_chroma, norm, off_w, off_phi;  // byte offsets into the table
  uint32_t off_bank, pad[3];                // the per-segment filterbank index [S]: the rate index itself unless tunings were estimated
};

__device__ __forceinline__ const ChromaHeader* chroma_hdr(const uint8_t* t) { return (const ChromaHeader*)(t + spec_hdr(t)->pad); }

// LDS images in floats: the FFT kernel's of vsyn_spectral_lin.h | R [ft][CHROMA_MAX]; the direct kernel's FramesDirect head (twiddles [2n] |
// window [n] | span [(ft-1) hop + n]) | S [ft][256] | R [ft][CHROMA_MAX]
__host__ __device__ __forceinline__ uint64_t chroma_fft_lds_floats(uint32_t ft, uint32_t n) { return spec_lin_fft_lds_floats(ft, n) + (uint64_t)ft * CHROMA_MAX; }
__host__ __device__ __forceinline__ uint64_t chroma_direct_lds_floats(uint32_t ft, uint32_t n, uint32_t hop) {
  return 3ull * n + spec_span_len(ft, n, hop) + (uint64_t)ft * SPEC_THREADS + (uint64_t)ft * CHROMA_MAX;
}

// sum_k w[k] s[k] over k < cnt by one wave: lane l's fma chain over k = l, l + 64, ... ascending, then wave_sum; every lane returns the sum.
__device__ __forceinline__ float chroma_dot(const float* __restrict__ w, const float* s, uint32_t cnt, uint32_t lane) {
  float acc = 0.f;
  for (uint32_t k0 = lane; k0 < cnt; k0 += 64u * 6u) {  // six loads of each operand in flight, then their fmas in the chain's order
    float wv[6], sv[6];
#pragma unroll
    for (uint32_t u = 0; u < 6u; ++u) {
      const uint32_t k = k0 + 64u * u;
      wv[u] = k < cnt ? w[k] : 0.f;
      sv[u] = k < cnt ? s[k] : 0.f;
    }
#pragma unroll
    for (uint32_t u = 0; u < 6u; ++u)
      if (k0 + 64u * u < cnt) acc = fmaf(wv[u], sv[u], acc);
  }
  return wave_sum(acc);
}

// Rows f0 .. f0 + nf - 1 from R [nf][NC] in LDS, one wave per frame: the norm, the division, the non-finite rule, and for tonnetz the
// second L1 norm and the product with phi (u goes back to the frame's row of s_R). Called by the whole workgroup behind a barrier.
__device__ __forceinline__ void chroma_finish(const SpecHeader* H, const ChromaHeader* CH, const uint8_t* tab, float* s_R, uint32_t nf, uint64_t r0,
                                              float* rows) {
  const uint32_t NC = CH->n_chroma, norm = CH->norm, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const bool tonnetz = H->kind == VSYN_SPEC_TONNETZ;
  const float* phi = (const float*)(tab + CH->off_phi);
  const float qnan = __uint_as_float(0x7FC00000u);
  for (uint32_t fb = 0; fb < nf; fb += SPEC_THREADS / 64u) {
    const uint32_t f = fb + wave;
    const bool act = f < nf;  // wave-uniform
    float* R = s_R + (size_t)f * NC;
    bool bad = false;
    if (act) {
      float v[CHROMA_MAX / 64];
      float s = 0.f, mx = 0.f;
#pragma unroll
      for (uint32_t j = 0; j < CHROMA_MAX / 64; ++j) {
        const uint32_t c = lane + 64u * j;
        v[j] = c < NC ? R[c] : 0.f;
        const float a = fabsf(v[j]);
        bad |= !(a <= FLT_MAX);  // Inf or NaN (fmaxf would drop a NaN)
        mx = fmaxf(mx, a);
        s = s + a;
      }
      bad = __any(bad) != 0;
      mx = wave_max(mx);
      float N = mx;
      if (norm == VSYN_CHROMA_NORM_L1) {
        N = wave_sum(s);
      } else if (norm == VSYN_CHROMA_NORM_L2 && !(mx < FLT_MIN)) {  // mx sqrt(sum (R / mx)^2): the squares neither overflow nor vanish
        s = 0.f;
#pragma unroll
        for (uint32_t j = 0; j < CHROMA_MAX / 64; ++j) {
          const float t = v[j] / mx;
          s = fmaf(t, t, s);
        }
        N = mx * sqrtf(wave_sum(s));
      }
      if (norm != VSYN_CHROMA_NORM_NONE && !bad && !(N < FLT_MIN)) {
#pragma unroll
        for (uint32_t j = 0; j < CHROMA_MAX / 64; ++j) v[j] = v[j] / N;
      }
      if (tonnetz && !bad) {
        float s1 = 0.f;
#pragma unroll
        for (uint32_t j = 0; j < CHROMA_MAX / 64; ++j) s1 = s1 + fabsf(v[j]);
        s1 = wave_sum(s1);
        if (!(s1 < FLT_MIN)) {
#pragma unroll
          for (uint32_t j = 0; j < CHROMA_MAX / 64; ++j) v[j] = v[j] / s1;
        }
      }
#pragma unroll
      for (uint32_t j = 0; j < CHROMA_MAX / 64; ++j) {
        const uint32_t c = lane + 64u * j;
        if (c < NC) {
          if (tonnetz) R[c] = v[j];
          else rows[(r0 + f) * NC + c] = bad ? qnan : v[j];
        }
      }
    }
    if (tonnetz) {  // (uniform over the workgroup)
      __syncthreads();
      if (act && lane < 6u) {
        const float* ph = phi + (size_t)lane * NC;
        float acc = 0.f;
        for (uint32_t c = 0; c < NC; ++c) acc = fmaf(ph[c], R[c], acc);
        rows[(r0 + f) * 6u + lane] = bad ? qnan : acc;
      }
    }
  }
}

__global__ void __launch_bounds__(SPEC_THREADS) vsyn_chroma_fft_kernel(const SpecCtx A, const uint32_t ft, const uint32_t lgM) {
  extern __shared__ float lds[];
  const SpecHeader* H = spec_hdr(A.tab);
  const ChromaHeader* CH = chroma_hdr(A.tab);
  const uint32_t g = blockIdx.y, tid = threadIdx.x;
  const uint32_t F = A.segF[g];
  const uint32_t f0 = blockIdx.x * ft;
  if (f0 >= F) return;
  const uint32_t n = H->n, nb = H->nbins, M = n >> 1, NC = CH->n_chroma;
  const uint32_t nf = min(ft, F - f0);
  const SpecLinFft T = spec_lin_fft_tile_run(A, H, lds, ft, lgM, g, f0, nf);
  float* s_S = (float*)T.spare;                       // [nf][nb]: nf nb <= ft n floats, the buffer's size
  float* s_R = lds + spec_lin_fft_lds_floats(ft, n);  // [nf][NC]
  for (uint32_t q = tid; q < nf * nb; q += SPEC_THREADS) {
    const uint32_t f = q / nb, k = q - f * nb;
    float re, im;
    spec_lin_untangle(T.Z + (size_t)f * M, T.un, M, k, re, im);
    const float p = fmaf(re, re, im * im);
    s_S[q] = H->power == 1 ? sqrtf(p) : p;
  }
  __syncthreads();
  const uint32_t ri = ((const uint32_t*)(A.tab + CH->off_bank))[g];
  const float* W = (const float*)(A.tab + CH->off_w) + (size_t)ri * NC * nb;
  const uint32_t wave = tid >> 6, lane = tid & 63u;
  for (uint32_t p = wave; p < nf * NC; p += SPEC_THREADS / 64u) {
    const uint32_t f = p / NC, c = p - f * NC;
    const float r = chroma_dot(W + (size_t)c * nb, s_S + (size_t)f * nb, nb, lane);
    if (lane == 0) s_R[p] = r;
  }
  __syncthreads();
  chroma_finish(H, CH, A.tab, s_R, nf, A.segoff[g] + f0, A.rows);
}

template <int FT>
__global__ void __launch_bounds__(SPEC_THREADS) vsyn_chroma_direct_kernel(const SpecCtx A) {
  extern __shared__ float lds[];
  const SpecHeader* H = spec_hdr(A.tab);
  const ChromaHeader* CH = chroma_hdr(A.tab);
  const uint32_t g = blockIdx.y, tid = threadIdx.x;
  const uint32_t F = A.segF[g];
  const uint32_t f0 = blockIdx.x * FT;
  if (f0 >= F) return;
  const uint32_t nb = H->nbins, NC = CH->n_chroma;
  const uint32_t nf = min((uint32_t)FT, F - f0);
  const FramesDirect D = frames_stage_direct(A, lds, (const float2*)(A.tab + H->off_tw), (const float*)(A.tab + H->off_win), H->n, H->hop,
                                             (uint32_t)spec_span_len(FT, H->n, H->hop), H->win, H->woff, (H->opts & VSYN_SPEC_CENTER) != 0, g, f0);
  float* s_S = D.rest;                   // [FT][256]
  float* s_R = s_S + FT * SPEC_THREADS;  // [nf][NC]
  for (uint32_t i = tid; i < nf * NC; i += SPEC_THREADS) s_R[i] = 0.f;
  __syncthreads();
  const uint32_t ri = ((const uint32_t*)(A.tab + CH->off_bank))[g];
  const float* W = (const float*)(A.tab + CH->off_w) + (size_t)ri * NC * nb;
  const uint32_t wave = tid >> 6, lane = tid & 63u;
  for (uint32_t k0 = 0; k0 < nb; k0 += SPEC_THREADS) {
    const uint32_t k = k0 + tid;
    float re[FT] = {}, im[FT] = {};
    if (k < nb) frames_dft_bin<FT>(D, k, re, im);
    frames_power_store<FT>(re, im, H->power, s_S);
    __syncthreads();
    const uint32_t cnt = min((uint32_t)SPEC_THREADS, nb - k0);
    for (uint32_t p = wave; p < nf * NC; p += SPEC_THREADS / 64u) {  // (pair p stays with its wave over the chunks)
      const uint32_t f = p / NC, c = p - f * NC;
      const float r = chroma_dot(W + (size_t)c * nb + k0, s_S + f * SPEC_THREADS, cnt, lane);
      if (lane == 0) s_R[p] = s_R[p] + r;
    }
    __syncthreads();
  }
  chroma_finish(H, CH, A.tab, s_R, nf, A.segoff[g] + f0, A.rows);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------

// The filterbank of "chroma" step 2 at rate sr: out[c * NB + k] float32, n_chroma rows of NB = n_fft / 2 + 1. ch is checked.
static inline void chroma_filterbank(uint32_t sr, uint32_t n, const vsyn_spectral_chroma* ch, float* out) {
  const uint32_t NC = ch->n_chroma, nb = n / 2u + 1u;
  const double nc = (double)NC;
  std::vector<double> q(n), bw(n), col(NC);
  const double a16 = 440.0 * exp2(ch->tuning / nc) / 16.0;
  for (uint32_t j = 1; j < n; ++j) q[j] = nc * log2(((double)j * (double)sr / (double)n) / a16);
  q[0] = q[1] - 1.5 * nc;
  for (uint32_t j = 0; j + 1u < n; ++j) bw[j] = std::max(q[j + 1] - q[j], 1.0);
  bw[n - 1u] = 1.0;
  const double h = nearbyint(nc / 2.0);  // ties to even, as numpy.round
  const uint32_t rot = (ch->options & VSYN_CHROMA_BASE_C) ? 3u * (NC / 12u) : 0u;
  for (uint32_t j = 0; j < nb; ++j) {
    double ss = 0.0;
    for (uint32_t c = 0; c < NC; ++c) {
      double d = fmod((q[j] - (double)c) + h + 10.0 * nc, nc);
      if (d < 0.0) d += nc;
      d -= h;
      const double t = 2.0 * d / bw[j];
      col[c] = exp(-0.5 * (t * t));
      ss += col[c] * col[c];
    }
    double nrm = sqrt(ss);
    if (nrm < DBL_MIN) nrm = 1.0;
    double oct = 1.0;
    if (!(ch->options & VSYN_CHROMA_NO_OCT)) {
      const double t = (q[j] / nc - ch->ctroct) / ch->octwidth;
      oct = exp(-0.5 * (t * t));
    }
    for (uint32_t c = 0; c < NC; ++c) {
      const float v = (float)(col[(c + rot) % NC] / nrm * oct);
      out[(size_t)c * nb + j] = fabsf(v) < FLT_MIN ? 0.f : v;
    }
  }
}

// phi of "chroma" step 4: out[i * n_chroma + c] float32
static inline void chroma_phi(uint32_t NC, float* out) {
  static const double sc[6] = {7.0 / 6.0, 7.0 / 6.0, 3.0 / 2.0, 3.0 / 2.0, 2.0 / 3.0, 2.0 / 3.0};
  static const double of[6] = {0.5, 0.0, 0.5, 0.0, 0.5, 0.0};
  static const double rd[6] = {1.0, 1.0, 1.0, 1.0, 0.5, 0.5};
  for (uint32_t i = 0; i < 6u; ++i)
    for (uint32_t c = 0; c < NC; ++c) out[(size_t)i * NC + c] = (float)(rd[i] * cos(M_PI * (sc[i] * (12.0 * (double)c / (double)NC) - of[i])));
}

// Frames per workgroup under sp (a chroma kind, checked): the FFT kernel's for a power-of-two n_fft, else the most of the direct
// kernel's that fit the LDS; 0 when nothing fits.
static inline uint32_t spec_chroma_tile(const vsyn_spectral_spec* sp) {
  if (spec_lin_pow2(sp->n_fft)) {
    const uint32_t ft = spec_lin_fft_tile(sp->n_fft);
    return chroma_fft_lds_floats(ft, sp->n_fft) * 4u <= SPEC_LDS_BUDGET ? ft : 0u;
  }
  for (uint32_t ft : {(uint32_t)CHROMA_DIRECT_FT, 1u})
    if (chroma_direct_lds_floats(ft, sp->n_fft, sp->hop_length) * 4u <= SPEC_LDS_BUDGET) return ft;
  return 0;
}

// The chroma block behind tab (the linear kinds' table of sp): one filterbank per bank and phi. Without seg_tuning a bank is a rate of
// distinct (spec_build_table's list, in the order of the table's rate indices) at ch->tuning, and a segment's bank index is its rate
// index. With seg_tuning [S] (estimated tunings) a bank is a distinct (rate, tuning) pair in the order of first appearance, and the
// per-segment bank index stands behind phi. ch is checked.
static inline int spec_chroma_table(SpectralWs& ws, const vsyn_spectral_spec* sp, const vsyn_spectral_chroma* ch, const std::vector<uint32_t>& distinct,
                                    std::vector<uint8_t>& tab, const char** err, const double* seg_tuning = nullptr) {
  const uint32_t n = sp->n_fft, nb = n / 2u + 1u, NC = ch->n_chroma;
  SpecHeader T;
  memcpy(&T, tab.data(), sizeof(T));
  std::vector<std::pair<uint32_t, double>> banks;
  std::vector<uint32_t> seg_bank;
  if (seg_tuning) {
    std::vector<uint32_t> seg_rate(T.S);
    if (T.S) memcpy(seg_rate.data(), tab.data() + T.off_rate, 4ull * T.S);
    seg_bank.assign(T.S, SPEC_SKIP);
    for (uint32_t g = 0; g < T.S; ++g) {
      if (seg_rate[g] == SPEC_SKIP) continue;
      const std::pair<uint32_t, double> want(distinct[seg_rate[g]], seg_tuning[g]);
      auto it = std::find(banks.begin(), banks.end(), want);
      seg_bank[g] = (uint32_t)(it - banks.begin());
      if (it == banks.end()) banks.push_back(want);
    }
  } else {
    for (uint32_t r : distinct) banks.push_back(std::make_pair(r, ch->tuning));
  }
  const size_t off_ch = (tab.size() + 15) & ~(size_t)15;
  const size_t off_w = off_ch + sizeof(ChromaHeader);
  const size_t off_phi = off_w + 4ull * banks.size() * NC * nb;
  const size_t off_bank = off_phi + 4ull * 6u * NC;
  const size_t total = off_bank + 4ull * seg_bank.size() + 16;
  if (total > 0xFFFFFFFFull)
    return fail(err, VSYN_ERR_INVALID, "too many distinct (sample rate, tuning) pairs (%zu) for one chroma table", banks.size());
  tab.resize(total, 0);
  T.pad = (uint32_t)off_ch;
  T.dim = spec_dim(sp, ch);
  memcpy(tab.data(), &T, sizeof(T));
  const ChromaHeader CH = {NC, ch->norm, (uint32_t)off_w, (uint32_t)off_phi, seg_tuning ? (uint32_t)off_bank : T.off_rate, {0u, 0u, 0u}};
  memcpy(tab.data() + off_ch, &CH, sizeof(CH));
  if (!seg_bank.empty()) memcpy(tab.data() + off_bank, seg_bank.data(), 4 * seg_bank.size());
  // the filterbanks of the last call are kept: a corpus run asks for the same ones submit after submit
  std::vector<double> key = {(double)n, (double)NC, (double)ch->options, ch->ctroct, ch->octwidth};
  for (const auto& b : banks) {
    key.push_back((double)b.first);
    key.push_back(b.second);
  }
  if (key != ws.chroma_key) {
    ws.chroma_key.clear();  // (a throw below leaves no stale bank behind a matching key)
    ws.chroma_bank.resize(banks.size() * NC * nb);
    vsyn_spectral_chroma cb = *ch;
    for (size_t r = 0; r < banks.size(); ++r) {
      cb.tuning = banks[r].second;
      chroma_filterbank(banks[r].first, n, &cb, ws.chroma_bank.data() + r * NC * nb);
    }
    ws.chroma_key = key;
  }
  if (!ws.chroma_bank.empty()) memcpy(tab.data() + off_w, ws.chroma_bank.data(), 4 * ws.chroma_bank.size());
  chroma_phi(NC, (float*)(tab.data() + off_phi));
  return VSYN_OK;
}

// The chroma kinds' kernel behind the offsets kernel: FFT or direct on grid with ft frames per workgroup.
static inline int spec_chroma_run(const SpecCtx& A, const vsyn_spectral_spec* sp, uint32_t ft, dim3 grid, hipStream_t s, const char** err) {
  const uint32_t n = sp->n_fft;
  if (spec_lin_pow2(n)) {
    VSYN_LAUNCH(vsyn_chroma_fft_kernel, grid, dim3(SPEC_THREADS), chroma_fft_lds_floats(ft, n) * 4u, s, A, ft, spec_lin_lgm(n));
  } else {
    const size_t lds = chroma_direct_lds_floats(ft, n, sp->hop_length) * 4u;
    if (ft == CHROMA_DIRECT_FT) VSYN_LAUNCH(vsyn_chroma_direct_kernel<CHROMA_DIRECT_FT>, grid, dim3(SPEC_THREADS), lds, s, A);
    else VSYN_LAUNCH(vsyn_chroma_direct_kernel<1>, grid, dim3(SPEC_THREADS), lds, s, A);
  }
  return VSYN_OK;
}

// ------------------------------------------------------------------------------------------------
// every spectral kind: the launch
// ------------------------------------------------------------------------------------------------
// The dynamic-LDS limit of every kind's tile kernels, once per handle (the device is selected).
static inline int spec_raise_lds(SpectralWs& ws, const char** err) {
  if (ws.lds_set) return VSYN_OK;
  const void* const kernels[12] = {(const void*)vsyn_spec_stft_kernel<16>,
                                  (const void*)vsyn_spec_stft_kernel<4>,
                                  (const void*)vsyn_spec_stft_kernel<1>,
                                  (const void*)vsyn_spec_lin_fft_kernel,
                                  (const void*)vsyn_spec_lin_direct_kernel<SPEC_LIN_DIRECT_FT>,
                                  (const void*)vsyn_spec_lin_direct_kernel<1>,
                                  (const void*)vsyn_chroma_fft_kernel,
                                  (const void*)vsyn_chroma_direct_kernel<CHROMA_DIRECT_FT>,
                                  (const void*)vsyn_chroma_direct_kernel<1>,
                                  (const void*)vsyn_piptrack_fft_kernel,
                                  (const void*)vsyn_piptrack_direct_kernel<PIP_DIRECT_FT>,
                                  (const void*)vsyn_piptrack_direct_kernel<1>};
  for (const void* k : kernels) HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SPEC_LDS_BUDGET));
  ws.lds_set = true;
  return VSYN_OK;
}

// The kernels of a spectral kind on stream s: the offsets kernel, then the kind's own (spec_mel_run, spec_lin_run, spec_chroma_run; ch,
// NULL for the defaults, is read for a chroma kind only); frames from d_frames, else from si. f_max bounds every segment's STFT frames,
// rows_bound the total rows. seg_tuning [S] (a chroma kind only; NULL: ch->tuning for all): each segment's own tuning, the
// filterbanks then per (rate, tuning) pair. Caller holds the handle's lock and has run spec_check.
static inline int spec_launch(SpectralWs& ws, int device, const vsyn_spectral_spec* sp, uint32_t S, const uint32_t* rates, const float* d_pcm, uint64_t plane,
                              uint32_t C, const uint32_t* d_frames, const SegInfo* si, uint64_t f_max, uint64_t rows_bound, float* d_rows,
                              uint64_t* d_segoff, hipStream_t s, const char** err, const vsyn_spectral_chroma* ch = nullptr,
                              const double* seg_tuning = nullptr) {
  if (S > 65535u) return fail(err, VSYN_ERR_INVALID, "too many segments (%u > 65535)", S);
  const bool lin = spec_is_lin(sp), chroma = spec_is_chroma(sp), mfcc = sp->kind == VSYN_SPEC_MFCC;
  const uint32_t ft = lin ? spec_lin_tile(sp) : chroma ? spec_chroma_tile(sp) : spec_tile(sp);
  if (!ft) return fail(err, VSYN_ERR_INVALID, "n_fft %u / hop_length %u do not fit the LDS", sp->n_fft, sp->hop_length);
  std::vector<uint8_t> tab;
  std::vector<uint32_t> distinct;
  spec_build_table(sp, S, rates, tab, &distinct);
  if (chroma)
    if (int rc = spec_chroma_table(ws, sp, spec_chroma_or_defaults(ch), distinct, tab, err, seg_tuning)) return rc;
  HIPCHK(hipSetDevice(device));
  if (int rc = spec_raise_lds(ws, err)) return rc;
  HIPCHK(ws.segF.ensure(S));
  HIPCHK(ws.segmax.ensure(S));
  HIPCHK(ws.segoff.ensure((size_t)S + 1));
  if (mfcc) HIPCHK(ws.db.ensure(rows_bound * sp->n_mels + 1));
  if (int rc = ws.tab.upload(tab, s, err)) return rc;
  SpecCtx A;
  A.tab = ws.tab.dev.p;
  A.pcm = d_pcm;
  A.plane = plane;
  A.C = C;
  A.S = S;
  A.frames = d_frames;
  A.si = si;
  A.segF = ws.segF.p;
  A.segoff = d_segoff ? d_segoff : ws.segoff.p;
  A.segmax = ws.segmax.p;
  A.rows = d_rows;
  A.db = mfcc ? ws.db.p : nullptr;
  VSYN_LAUNCH(vsyn_spec_offsets_kernel, dim3(1), dim3(SPEC_THREADS), 0, s, A);
  if (f_max == 0 || S == 0) return VSYN_OK;
  const uint64_t gx = (f_max + ft - 1) / ft;
  if (gx > 0x7FFFFFFFull) return fail(err, VSYN_ERR_INVALID, "segment too long");
  const dim3 grid((uint32_t)gx, S);
  if (lin) return spec_lin_run(A, sp, ft, grid, f_max, s, err);
  if (chroma) return spec_chroma_run(A, sp, ft, grid, s, err);
  return spec_mel_run(A, sp, ft, grid, f_max, s, err);
}
