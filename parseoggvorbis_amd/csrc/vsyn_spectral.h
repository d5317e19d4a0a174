// vsyn_spectral.h — mel filterbank / log-mel / dB-mel / MFCC rows from planar float32 PCM already on the device.
// Semantics: include/vorbis_synth_hip.h, "spectral features".
//
// Three kernels on one stream (tables built on the host in double, vorbis_synth_hip.hip spec_build_table):
//   1. vsyn_spec_offsets_kernel  one workgroup: per segment its PCM frames (the caller's d_frames, or the last submit's SegInfo),
//                                its STFT frame count, the exclusive row scan seg_off[S+1]; clears the per-segment dB maxima.
//   2. vsyn_spec_stft_kernel<FT> one workgroup per (segment, tile of FT frames). LDS holds the twiddles cos/sin(2 pi m / n_fft)
//                                (m < n_fft), the window, and the tile's span of the mono signal (frames_stage_direct, vsyn_frames.h).
//                                A thread owns one bin k of a 256-bin chunk and accumulates the FT frames' real DFT sums
//                                (frames_dft_bin); the chunk's |X|^power goes to LDS (frames_power_store) and the
//                                mel bands that overlap the chunk take their share from it (sparse per-band weights). The last
//                                chunk ends in the kind's output: M, log10, or 10 log10 (with a per-segment max by atomicMax on
//                                order-preserving integer keys).
//   3. vsyn_spec_finish_kernel   MEL_DB / MFCC only, after 2: the top_db clamp against the segment's max, and for MFCC the
//                                orthonormal DCT-II (host-built matrix) of the clamped dB rows.
// The host side here is the mel kinds' share of a launch: tile, table, kernel pick and finish. spec_launch itself, the one preamble
// of every spectral kind, stands behind the last kind's header (vsyn_chroma.h).
// Nothing here reads or writes stream state, the overlap carry or any synthesis buffer; the PCM is only read.
#pragma once
#include "vsyn_device.h"
#include "vsyn_frames.h"
#include "vsyn_host.h"

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
static_assert(SPEC_THREADS == FRAMES_THREADS, "the shared framing helpers stride by the workgroup's size");
#define SPEC_FIN_ROWS 16

__device__ __forceinline__ const SpecHeader* spec_hdr(const uint8_t* t) { return (const SpecHeader*)t; }

// max(x, floor) that keeps a NaN: fmaxf(NaN, floor) is floor, which would turn a frame that holds a NaN sample into a silent one
__device__ __forceinline__ float spec_floor(float x, float floor) { return x < floor ? floor : x; }
// A dB value as a candidate for its segment's maximum: a value that is not finite takes no part in it (-inf is below every key).
__device__ __forceinline__ float spec_max_term(float d) { return fabsf(d) < INFINITY ? d : -INFINITY; }

// float -> uint32 with the same order (no NaN here: only finite dB values get a key, spec_max_term)
__device__ __forceinline__ uint32_t spec_key(float x) {
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float spec_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

__global__ void __launch_bounds__(SPEC_THREADS) vsyn_spec_offsets_kernel(const SpecCtx A) {
  const SpecHeader* H = spec_hdr(A.tab);
  const uint32_t* rate = (const uint32_t*)(A.tab + H->off_rate);
  wg_exclusive_scan<SPEC_THREADS, 1>(A.S, A.segoff, [&](uint32_t g, uint64_t* v) {
    const uint64_t T = frames_len(A, g);
    v[0] = rate[g] == SPEC_SKIP ? 0ull : spec_num_frames(H->n, H->hop, (H->opts & VSYN_SPEC_CENTER) != 0, T);
    A.segF[g] = (uint32_t)v[0];
    A.segmax[g] = 0u;  // below every key
  });
}

// LDS image of the STFT kernel, in floats: FramesDirect's head (twiddles [2n] | window [n] | span [(FT-1) hop + n]) | |X|^power [FT][256] |
// M [FT][n_mels]
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
  const uint32_t nb = H->nbins, NM = H->n_mels;
  const uint32_t nf = min((uint32_t)FT, F - f0);
  const uint32_t ri = ((const uint32_t*)(A.tab + H->off_rate))[g];
  const SpecBand* band = (const SpecBand*)(A.tab + H->off_band) + (size_t)ri * NM;
  const float* wts = (const float*)(A.tab + H->off_w);
  const FramesDirect D = frames_stage_direct(A, lds, (const float2*)(A.tab + H->off_tw), (const float*)(A.tab + H->off_win), H->n, H->hop,
                                             (uint32_t)spec_span_len(FT, H->n, H->hop), H->win, H->woff, (H->opts & VSYN_SPEC_CENTER) != 0, g, f0);
  float* s_S = D.rest;
  float* s_M = s_S + FT * SPEC_THREADS;
  for (uint32_t i = tid; i < FT * NM; i += SPEC_THREADS) s_M[i] = 0.f;
  __syncthreads();

  for (uint32_t k0 = 0; k0 < nb; k0 += SPEC_THREADS) {
    const uint32_t k = k0 + tid;
    float re[FT] = {}, im[FT] = {};
    if (k < nb) frames_dft_bin<FT>(D, k, re, im);
    frames_power_store<FT>(re, im, H->power, s_S);
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
      A.rows[r * NM + m] = log10f(spec_floor(M, H->log_floor));
    } else {
      const float d = 10.0f * log10f(spec_floor(M, H->amin));
      mx = fmaxf(mx, spec_max_term(d));
      if (kind == VSYN_SPEC_MEL_DB) A.rows[r * NM + m] = d;
      else A.db[r * NM + m] = d;
    }
  }
  if (kind >= VSYN_SPEC_MEL_DB) {
    mx = wave_max(mx);
    if ((tid & 63u) == 0 && mx > -INFINITY) atomicMax(A.segmax + g, spec_key(mx));
  }
}

// MEL_DB: the top_db clamp in place. MFCC: out[r][i] = sum_m dct[i][m] * max(D[r][m], thr), m ascending. The clamp leaves a value
// that is not finite as it is, and so does a threshold that is none (a segment without a finite value).
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
      *p = spec_floor(*p, thr);
    }
    return;
  }
  for (uint32_t q = tid; q < nf * NM; q += SPEC_THREADS) s_d[q] = spec_floor(A.db[r0 * NM + q], thr);
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

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static const uint32_t SPEC_LDS_BUDGET = 160u * 1024u;  // gfx950: 160 KiB of LDS per CU, all of it available to one workgroup

struct SpectralWs {  // the stage's buffers: its own; the PCM is only read
  TableUpload tab;
  bool lds_set = false;                // the dynamic-LDS limit of every kind's kernels is raised on this handle's device (spec_raise_lds)
  std::vector<double> chroma_key;      // what the kept chroma filterbanks were built from (n_fft, the chroma parameters, the (rate, tuning) pairs)
  std::vector<float> chroma_bank;      // [bank][n_chroma][NB]
  DevBuf<uint32_t> segF, segmax;
  DevBuf<uint64_t> segoff;
  DevBuf<float> db, rows;
};

static inline double spec_hz_to_mel(double f, bool htk) {
  if (htk) return 2595.0 * log10(1.0 + f / 700.0);
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
  return f >= min_log_hz ? min_log_mel + log(f / min_log_hz) / logstep : f / f_sp;
}
static inline double spec_mel_to_hz(double m, bool htk) {
  if (htk) return 700.0 * (pow(10.0, m / 2595.0) - 1.0);
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
  return m >= min_log_mel ? min_log_hz * exp(logstep * (m - min_log_mel)) : f_sp * m;
}

// The linear kinds (include/vorbis_synth_hip.h, "linear spectra") read no mel field of the spec.
static inline bool spec_is_lin(const vsyn_spectral_spec* sp) { return sp->kind >= VSYN_SPEC_LIN_POWER && sp->kind <= VSYN_SPEC_STFT; }

// The chroma kinds (include/vorbis_synth_hip.h, "chroma") read the framing fields and power of the spec and a vsyn_spectral_chroma.
static inline bool spec_is_chroma(const vsyn_spectral_spec* sp) { return sp->kind == VSYN_SPEC_CHROMA || sp->kind == VSYN_SPEC_TONNETZ; }
static const vsyn_spectral_chroma SPEC_CHROMA_DEFAULTS = {12u, VSYN_CHROMA_NORM_MAX, VSYN_CHROMA_BASE_C, 0u, 0.0, 5.0, 2.0};
static inline const vsyn_spectral_chroma* spec_chroma_or_defaults(const vsyn_spectral_chroma* ch) { return ch ? ch : &SPEC_CHROMA_DEFAULTS; }

// Columns of a row (vsyn_spectral_dim, vsyn_spectral_chroma_dim): the one formula on the C side; 0 for an unknown kind. ch (NULL:
// the defaults) is read for the chroma kinds only.
static inline uint32_t spec_dim(const vsyn_spectral_spec* sp, const vsyn_spectral_chroma* ch = nullptr) {
  switch (sp->kind) {
    case VSYN_SPEC_CHROMA: return spec_chroma_or_defaults(ch)->n_chroma;
    case VSYN_SPEC_TONNETZ: return 6u;
    case VSYN_SPEC_MEL_POWER:
    case VSYN_SPEC_LOG_MEL:
    case VSYN_SPEC_MEL_DB: return sp->n_mels;
    case VSYN_SPEC_MFCC: return sp->n_mfcc;
    case VSYN_SPEC_LIN_POWER:
    case VSYN_SPEC_LIN_DB: return sp->n_fft / 2u + 1u;
    case VSYN_SPEC_STFT: return 2u * (sp->n_fft / 2u + 1u);
    default: return 0u;
  }
}

// The checks of the spec and of every segment's rate (0 = skipped segment); ch (NULL: the defaults) is read for the chroma kinds only.
static inline int spec_check(const vsyn_spectral_spec* sp, uint32_t S, const uint32_t* rates, const char** err, const vsyn_spectral_chroma* ch = nullptr) {
  if (!sp) return fail(err, VSYN_ERR_INVALID, "spectral spec is NULL");
  if (sp->kind < VSYN_SPEC_MEL_POWER || sp->kind > VSYN_SPEC_TONNETZ) return fail(err, VSYN_ERR_INVALID, "unknown spectral kind %u", sp->kind);
  if (sp->options & ~(VSYN_SPEC_CENTER | VSYN_SPEC_HTK | VSYN_SPEC_NO_NORM)) return fail(err, VSYN_ERR_INVALID, "unknown spectral options 0x%x", sp->options);
  if (sp->n_fft < 16 || sp->n_fft > 8192) return fail(err, VSYN_ERR_INVALID, "n_fft %u outside [16, 8192]", sp->n_fft);
  if (sp->hop_length < 1) return fail(err, VSYN_ERR_INVALID, "hop_length must be >= 1");
  if (sp->win_length < 1 || sp->win_length > sp->n_fft) return fail(err, VSYN_ERR_INVALID, "win_length %u outside [1, n_fft]", sp->win_length);
  if (spec_is_lin(sp)) {  // no mel field is read, and a rate only decides whether its segment is skipped
    if (sp->kind != VSYN_SPEC_STFT && sp->power != 1 && sp->power != 2) return fail(err, VSYN_ERR_INVALID, "power must be 1 or 2");
    if (sp->kind == VSYN_SPEC_LIN_DB && (!(sp->amin > 0.0) || !(sp->top_db >= 0.0))) return fail(err, VSYN_ERR_INVALID, "amin must be > 0 and top_db >= 0");
    if (S && !rates) return fail(err, VSYN_ERR_INVALID, "sample_rates is NULL");
    return VSYN_OK;
  }
  if (spec_is_chroma(sp)) {  // the framing and power as for a linear kind, then the chroma parameters; no mel field is read
    ch = spec_chroma_or_defaults(ch);
    if (sp->power != 1 && sp->power != 2) return fail(err, VSYN_ERR_INVALID, "power must be 1 or 2");
    if (ch->n_chroma < 1 || ch->n_chroma > 256) return fail(err, VSYN_ERR_INVALID, "n_chroma %u outside [1, 256]", ch->n_chroma);
    if (ch->norm > VSYN_CHROMA_NORM_MAX) return fail(err, VSYN_ERR_INVALID, "unknown chroma norm %u", ch->norm);
    if (ch->options & ~(VSYN_CHROMA_BASE_C | VSYN_CHROMA_NO_OCT)) return fail(err, VSYN_ERR_INVALID, "unknown chroma options 0x%x", ch->options);
    if (!std::isfinite(ch->tuning) || !std::isfinite(ch->ctroct)) return fail(err, VSYN_ERR_INVALID, "chroma tuning and ctroct must be finite");
    if (!(ch->options & VSYN_CHROMA_NO_OCT) && !(std::isfinite(ch->octwidth) && ch->octwidth > 0.0))
      return fail(err, VSYN_ERR_INVALID, "chroma octwidth must be finite and > 0");
    if (S && !rates) return fail(err, VSYN_ERR_INVALID, "sample_rates is NULL");
    return VSYN_OK;
  }
  if (sp->n_mels < 1 || sp->n_mels > 256) return fail(err, VSYN_ERR_INVALID, "n_mels %u outside [1, 256]", sp->n_mels);
  if (sp->kind == VSYN_SPEC_MFCC && (sp->n_mfcc < 1 || sp->n_mfcc > sp->n_mels)) return fail(err, VSYN_ERR_INVALID, "n_mfcc %u outside [1, n_mels]", sp->n_mfcc);
  if (sp->power != 1 && sp->power != 2) return fail(err, VSYN_ERR_INVALID, "power must be 1 or 2");
  if (!(sp->fmin >= 0.0) || !(sp->fmax >= 0.0)) return fail(err, VSYN_ERR_INVALID, "fmin / fmax must be >= 0");
  if (sp->kind == VSYN_SPEC_LOG_MEL && !(sp->log_floor > 0.0)) return fail(err, VSYN_ERR_INVALID, "log_floor must be > 0");
  if (sp->kind >= VSYN_SPEC_MEL_DB && (!(sp->amin > 0.0) || !(sp->top_db >= 0.0))) return fail(err, VSYN_ERR_INVALID, "amin must be > 0 and top_db >= 0");
  if (S && !rates) return fail(err, VSYN_ERR_INVALID, "sample_rates is NULL");
  for (uint32_t g = 0; g < S; ++g) {
    if (!rates[g]) continue;
    const double ny = rates[g] / 2.0, fmax = sp->fmax > 0.0 ? sp->fmax : ny;
    if (fmax > ny) return fail(err, VSYN_ERR_INVALID, "segment %u: fmax %g above sr/2 = %g", g, fmax, ny);
    if (!(sp->fmin < fmax)) return fail(err, VSYN_ERR_INVALID, "segment %u: fmin %g not below fmax %g", g, sp->fmin, fmax);
  }
  return VSYN_OK;
}

static inline uint32_t spec_tile(const vsyn_spectral_spec* sp) {  // frames per STFT workgroup: the most that fit the LDS
  for (uint32_t ft : {16u, 4u, 1u})
    if (spec_lds_floats(ft, sp->n_fft, sp->hop_length, sp->n_mels) * 4u <= SPEC_LDS_BUDGET) return ft;
  return 0;
}

// SpecHeader, twiddles, window, per-rate bands and weights, DCT matrix, per-segment rate index. Call after spec_check. rates_out, where
// given, takes the distinct rates in the order of the table's rate indices (first appearance).
static inline void spec_build_table(const vsyn_spectral_spec* sp, uint32_t S, const uint32_t* rates, std::vector<uint8_t>& out,
                                    std::vector<uint32_t>* rates_out = nullptr) {
  const uint32_t n = sp->n_fft, NM = spec_is_lin(sp) || spec_is_chroma(sp) ? 0u : sp->n_mels, nb = n / 2u + 1u;  // a linear or chroma kind: no mel table
  const bool htk = (sp->options & VSYN_SPEC_HTK) != 0, norm = !(sp->options & VSYN_SPEC_NO_NORM);
  std::vector<uint32_t> distinct, seg_rate(S, SPEC_SKIP);
  for (uint32_t g = 0; g < S; ++g) {
    if (!rates[g]) continue;
    auto it = std::find(distinct.begin(), distinct.end(), rates[g]);
    seg_rate[g] = (uint32_t)(it - distinct.begin());
    if (it == distinct.end()) distinct.push_back(rates[g]);
  }
  std::vector<SpecBand> bands;
  std::vector<float> w;
  std::vector<double> hz(NM + 2);
  for (uint32_t sr : distinct) {
    const double fmax = sp->fmax > 0.0 ? sp->fmax : sr / 2.0;
    const double m0 = spec_hz_to_mel(sp->fmin, htk), m1 = spec_hz_to_mel(fmax, htk), step = (m1 - m0) / (double)(NM + 1);
    for (uint32_t i = 0; i < NM + 2; ++i) hz[i] = spec_mel_to_hz(i == NM + 1 ? m1 : m0 + i * step, htk);  // numpy.linspace
    for (uint32_t m = 0; m < NM; ++m) {
      const double lo = hz[m], c = hz[m + 1], hi = hz[m + 2], enorm = norm ? 2.0 / (hi - lo) : 1.0;
      SpecBand b = {0, 0, (uint32_t)w.size(), 0};
      for (uint32_t k = 0; k < nb; ++k) {
        const double fk = (double)k * sr / n;
        const double v = std::max(0.0, std::min((fk - lo) / (c - lo), (hi - fk) / (hi - c))) * enorm;
        if (v > 0.0) {
          if (!b.cnt) b.first = k;
          for (uint32_t z = b.first + b.cnt; z < k; ++z) w.push_back(0.f);  // (a triangle has no holes; kept general)
          b.cnt = k - b.first + 1;
          w.push_back((float)v);
        }
      }
      bands.push_back(b);
    }
  }
  SpecHeader T = {};
  T.kind = sp->kind;
  T.opts = sp->options;
  T.n = n;
  T.hop = sp->hop_length;
  T.win = sp->win_length;
  T.woff = (n - sp->win_length) / 2u;
  T.nbins = nb;
  T.n_mels = NM;
  T.dim = spec_dim(sp);
  T.n_mfcc = sp->kind == VSYN_SPEC_MFCC ? sp->n_mfcc : 0u;
  T.power = sp->power;
  T.num_rates = (uint32_t)distinct.size();
  T.S = S;
  T.log_floor = (float)sp->log_floor;
  T.amin = (float)sp->amin;
  T.top_db = (float)sp->top_db;
  auto al = [](size_t v) { return (uint32_t)((v + 15) & ~(size_t)15); };
  T.off_tw = al(sizeof(SpecHeader));
  T.off_win = al(T.off_tw + 8ull * n);
  T.off_band = al(T.off_win + 4ull * n);
  T.off_w = al(T.off_band + sizeof(SpecBand) * bands.size());
  T.off_dct = al(T.off_w + 4ull * w.size());
  T.off_rate = al(T.off_dct + 4ull * T.n_mfcc * NM);
  out.assign(T.off_rate + 4ull * S + 16, 0);
  memcpy(out.data(), &T, sizeof(T));
  twiddle_table(n, (float*)(out.data() + T.off_tw));
  hann_centred(n, sp->win_length, (float*)(out.data() + T.off_win));
  if (!bands.empty()) memcpy(out.data() + T.off_band, bands.data(), sizeof(SpecBand) * bands.size());
  if (!w.empty()) memcpy(out.data() + T.off_w, w.data(), 4 * w.size());
  float* dct = (float*)(out.data() + T.off_dct);
  for (uint32_t i = 0; i < T.n_mfcc; ++i)
    for (uint32_t m = 0; m < NM; ++m)
      dct[(size_t)i * NM + m] = (float)(sqrt((i ? 2.0 : 1.0) / NM) * cos(M_PI * (double)i * (2.0 * m + 1.0) / (2.0 * NM)));
  if (S) memcpy(out.data() + T.off_rate, seg_rate.data(), 4ull * S);
  if (rates_out) rates_out->swap(distinct);
}

// The mel kinds' kernels behind the offsets kernel: STFT / mel on grid with ft frames per workgroup, and the (MEL_DB, MFCC) finish.
static inline int spec_mel_run(const SpecCtx& A, const vsyn_spectral_spec* sp, uint32_t ft, dim3 grid, uint64_t f_max, hipStream_t s, const char** err) {
  const size_t lds = spec_lds_floats(ft, sp->n_fft, sp->hop_length, sp->n_mels) * 4u;
  if (ft == 16) VSYN_LAUNCH(vsyn_spec_stft_kernel<16>, grid, dim3(SPEC_THREADS), lds, s, A);
  else if (ft == 4) VSYN_LAUNCH(vsyn_spec_stft_kernel<4>, grid, dim3(SPEC_THREADS), lds, s, A);
  else VSYN_LAUNCH(vsyn_spec_stft_kernel<1>, grid, dim3(SPEC_THREADS), lds, s, A);
  if (sp->kind >= VSYN_SPEC_MEL_DB) {
    VSYN_LAUNCH(vsyn_spec_finish_kernel, dim3((uint32_t)((f_max + SPEC_FIN_ROWS - 1) / SPEC_FIN_ROWS), grid.y), dim3(SPEC_THREADS), 0, s, A);
  }
  return VSYN_OK;
}
