// vsyn_cqt.h — the constant-Q / variable-Q transform in direct time-domain form and the chroma_cqt and tonnetz rows folded from it, from
// planar float32 PCM already on the device. Semantics: include/vorbis_synth_hip.h, "constant-Q". Design, bound and measurements:
// DESIGN.md 6v.
//
// Two tables. The wavelets (ws.basis) are built on the host per (spec, distinct (rate, tuning) pairs), kept there and on the device from call to
// call, and uploaded only when that key changes:
//   CqtBin [rate][n_bins] (L_k, h_k, the first pair's index, s_k) | class index [n_bins] (chroma outputs) | float32 pairs (re, im)
// The per-call table (ws.tab) is small: a SpecHeader and a ChromaHeader for chroma_finish (vsyn_chroma.h), phi, and per segment its
// rate index, CQT_SKIP (rate 0) or CQT_REFUSED (step 10).
// Kernels on one stream, through frames_launch (vsyn_frames.h):
//   1. vsyn_cqt_offsets_kernel  one workgroup: F = 1 + T / hop per segment and the exclusive row scan (frames_offsets with frames of
//                               0 samples, centred: the framing whose frame t is the sample t hop).
//   2. vsyn_cqt_kernel          grid (tile of CQT_FT frames, segment, group of CQT_BPW consecutive bins), 256 threads: ONE WAVE PER
//                               BIN. Bins of a group are neighbours in k, so of similar length (a factor 2^(3 / bpo) apart at most),
//                               and a group walks only the chunks its own longest bin (its first) touches: the top octave's
//                               groups run one or two chunks, the bottom group of librosa's defaults twelve, and the bottom octave
//                               is spread over bpo / CQT_BPW workgroups per tile.
//                               The offsets m are cut by one grid for every bin: chunk c is [c K - K/2, (c + 1) K - K/2), K =
//                               VSYN_CQT_CHUNK. Per chunk the workgroup stages the tile's span of the mono signal for the group's
//                               part [ms, me) of the chunk into LDS (the downmix is done while loading, zeros outside [0, T)):
//                               s[f * fstep + (m - ms)] = y[(f0 + f) hop + m], fstep = hop, or the part's width when hop > K
//                               (frames that do not touch are staged back to back and the samples between them never read). LDS:
//                               (CQT_FT - 1) min(hop, K) + K floats, at most 32 KiB, whatever the wavelets' lengths.
//                               Lane l of the bin's wave then walks the bin's offsets of the chunk first + l, first + l + 64, ..: one
//                               coalesced float2 read of the wavelet serves the tile's CQT_FT frames (CQT_FT LDS reads, 2 CQT_FT
//                               fmas); the 2 CQT_FT chains go through wave_sum and are added to the running sums, chunks ascending.
//                               Float32 throughout: the chain of a lane has K / 64 = 16 terms whatever L_k, so the rounding grows
//                               with 16 + 6 + the chunk count (150 u at L = 2^17), not with L (DESIGN.md 6v has the bound).
//                               Lanes 0 .. nf - 1 scale by s_k and store the frames' values: |C|^power, (re, im), or |C| into the
//                               magnitude workspace for the chroma outputs. No atomics.
//                               The group-0 workgroup of a tile also looks at every sample of the tile's share of the segment for
//                               an Inf or a NaN and writes the tile's flag word (frames_tile_flag).
//   3. vsyn_cqt_fold_kernel     chroma outputs only, one workgroup per (tile, segment): R[f][c] = the magnitudes of class c added in
//                               ascending k by one thread, then chroma_finish: the norm, the FLT_MIN rule, tonnetz.
//   4. vsyn_cqt_finish_kernel   one workgroup per segment: a rate-refused segment's rows become NaN and its refused word 2; else
//                               frames_finish (a flagged tile: NaN rows, refused word 1).
// Nothing here reads or writes stream state, the overlap carry or any synthesis buffer; the PCM is only read.
#pragma once
#include <cfloat>

#include "vsyn_chroma.h"
#include "vsyn_device.h"
#include "vsyn_frames.h"
#include "vsyn_host.h"

#define CQT_THREADS 256
static_assert(CQT_THREADS == FRAMES_THREADS && CQT_THREADS == SPEC_THREADS, "the shared framing and chroma helpers stride by the workgroup's size");
#define CQT_WAVES (CQT_THREADS / 64)
#define CQT_FT 8u           // frames per workgroup: accumulator pairs per lane
#define CQT_BPW CQT_WAVES   // bins per workgroup: one wave each
#define CQT_CHUNK ((int32_t)VSYN_CQT_CHUNK)
#define CQT_MAX_BINS 256u
#define CQT_SKIP 0xFFFFFFFFu     // seg entry: rate 0, no rows
#define CQT_REFUSED 0xFFFFFFFEu  // seg entry: step 10, NaN rows
#define CQT_HANN_BW 1.50018310546875

struct CqtBin {
  uint32_t L, h, off;  // support [-h, L - h); index of the first pair
  float s;             // s_k
};

struct CqtCtx {  // launch arguments
  const uint8_t* tab;    // the per-call table
  const uint8_t* basis;  // the wavelet table
  const uint32_t* seg;   // [S] rate index, CQT_SKIP or CQT_REFUSED
  const float* pcm;
  uint64_t plane;
  uint32_t C, S;
  const uint32_t* frames;  // PCM frames per segment (caller's, or the resampler's), or
  const SegInfo* si;       // the last submit's SegInfo (total_emit)
  uint32_t H, FT;          // hop_length, frames per workgroup
  uint32_t center;         // 1: the offsets kernel's framing
  uint32_t tiles;          // workgroups per segment (grid.x): the flags' stride
  uint32_t nb, out, power, cols;
  uint32_t off_cls, off_pairs;  // byte offsets into basis
  uint32_t* segF;               // [S] frames
  uint64_t* segoff;             // [S+1]
  uint32_t* flags;              // [S][tiles] a sample of the tile's share is not finite
  uint32_t* refused;            // [S]
  float* rows;                  // [segoff[S]][cols]
  float* mag;                   // [segoff[S]][nb] chroma outputs: |C|
};

__global__ void __launch_bounds__(CQT_THREADS) vsyn_cqt_offsets_kernel(const CqtCtx A) {
  frames_offsets(A, 0u, [&](uint32_t g) { return A.seg[g] == CQT_SKIP; });
}

__device__ __forceinline__ int32_t cqt_chunk_of(int32_t m) {  // floor((m + K/2) / K)
  const int32_t a = m + CQT_CHUNK / 2;
  return a >= 0 ? a / CQT_CHUNK : -((-a + CQT_CHUNK - 1) / CQT_CHUNK);
}

__global__ void __launch_bounds__(CQT_THREADS) vsyn_cqt_kernel(const CqtCtx A) {
  extern __shared__ float s_cqt[];
  const uint32_t g = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint32_t ri = A.seg[g];
  FramesTile t;
  if (frames_tile_head(A, ri >= CQT_REFUSED, t)) {
    if (blockIdx.z == 0u) frames_tile_idle(t);
    return;
  }
  frames_tile_derive(A, 0u, t);
  if (blockIdx.z == 0u) frames_tile_flag(A, t);  // (workgroup-uniform)
  if (t.nf == 0u) return;

  const CqtBin* bins = (const CqtBin*)A.basis + (size_t)ri * A.nb;
  const float2* pairs = (const float2*)(A.basis + A.off_pairs);
  const uint32_t k0 = blockIdx.z * CQT_BPW, k = k0 + wave;
  const bool have = k < A.nb;  // wave-uniform
  const CqtBin b0 = bins[k0], bk = bins[have ? k : k0];
  const int32_t lo0 = -(int32_t)b0.h, hi0 = (int32_t)b0.L - (int32_t)b0.h;  // the group's offsets: its first bin's, the longest
  const int32_t lok = -(int32_t)bk.h, hik = (int32_t)bk.L - (int32_t)bk.h;  // this wave's
  const int32_t c_first = cqt_chunk_of(lo0), c_last = cqt_chunk_of(hi0 - 1);
  const bool apart = A.H > (uint32_t)CQT_CHUNK;
  float tre[CQT_FT], tim[CQT_FT];
#pragma unroll
  for (uint32_t f = 0; f < CQT_FT; ++f) tre[f] = tim[f] = 0.f;

  for (int32_t c = c_first; c <= c_last; ++c) {
    const int32_t m0 = c * CQT_CHUNK - CQT_CHUNK / 2;
    const int32_t ms = max(m0, lo0), me = min(m0 + CQT_CHUNK, hi0);  // the group's part of the chunk
    const uint32_t w = (uint32_t)(me - ms);
    const uint32_t fstep = apart ? w : A.H;
    const uint32_t staged = (CQT_FT - 1u) * fstep + w;  // (frames of the tile past the segment's last read zeros and are never stored)
    const int64_t base = (int64_t)(t.f0 * A.H) + ms;
    __syncthreads();  // the chunk before is read
    for (uint32_t u = tid; u < staged; u += CQT_THREADS) {
      const int64_t s = apart ? base + (int64_t)(u / w) * A.H + (u % w) : base + u;
      s_cqt[u] = (s >= 0 && (uint64_t)s < t.T) ? pcm_downmix(t.x, A.plane, t.C, t.inv_c, (uint64_t)s) : 0.f;
    }
    __syncthreads();
    const int32_t a = max(ms, lok), e = min(me, hik);  // this bin's offsets of the chunk
    if (!have || a >= e) continue;                     // (wave-uniform; no barrier below)
    float re[CQT_FT], im[CQT_FT];
#pragma unroll
    for (uint32_t f = 0; f < CQT_FT; ++f) re[f] = im[f] = 0.f;
    const float2* bp = pairs + bk.off + (uint32_t)(a - lok);
    const float* sp = s_cqt + (uint32_t)(a - ms);
    const uint32_t n = (uint32_t)(e - a);
#pragma unroll 2
    for (uint32_t i = lane; i < n; i += 64u) {
      const float2 b = bp[i];
      const float* p = sp + i;
#pragma unroll
      for (uint32_t f = 0; f < CQT_FT; ++f) {
        const float v = p[f * fstep];
        re[f] = fmaf(v, b.x, re[f]);
        im[f] = fmaf(v, b.y, im[f]);
      }
    }
#pragma unroll
    for (uint32_t f = 0; f < CQT_FT; ++f) {
      tre[f] = tre[f] + wave_sum(re[f]);
      tim[f] = tim[f] + wave_sum(im[f]);
    }
  }
  if (!have) return;

  const uint64_t r0 = A.segoff[g] + t.f0;
#pragma unroll
  for (uint32_t f = 0; f < CQT_FT; ++f) {
    if (lane != f || f >= t.nf) continue;
    const float re = tre[f] * bk.s, im = tim[f] * bk.s;
    if (A.out == VSYN_CQT_COMPLEX) {
      float* row = A.rows + (r0 + f) * 2u * A.nb + 2u * k;
      row[0] = re;
      row[1] = im;
    } else {
      const float p = fmaf(re, re, im * im);
      if (A.out == VSYN_CQT_MAG) A.rows[(r0 + f) * A.nb + k] = A.power == 1u ? sqrtf(p) : p;
      else A.mag[(r0 + f) * A.nb + k] = sqrtf(p);
    }
  }
}

__global__ void __launch_bounds__(CQT_THREADS) vsyn_cqt_fold_kernel(const CqtCtx A) {
  __shared__ float s_R[CQT_FT * CHROMA_MAX];
  const uint32_t g = blockIdx.y, tid = threadIdx.x;
  if (A.seg[g] >= CQT_REFUSED) return;
  const uint32_t F = A.segF[g], f0 = blockIdx.x * A.FT;
  if (f0 >= F) return;
  const uint32_t nf = min(A.FT, F - f0), nb = A.nb;
  const SpecHeader* H = spec_hdr(A.tab);
  const ChromaHeader* CH = chroma_hdr(A.tab);
  const uint32_t NC = CH->n_chroma;
  const uint32_t* cls = (const uint32_t*)(A.basis + A.off_cls);
  const uint64_t r0 = A.segoff[g] + f0;
  for (uint32_t q = tid; q < nf * NC; q += CQT_THREADS) {
    const uint32_t f = q / NC, c = q - f * NC;
    const float* m = A.mag + (r0 + f) * nb;
    float acc = 0.f;
    for (uint32_t k = 0; k < nb; ++k)
      if (cls[k] == c) acc = acc + m[k];
    s_R[q] = acc;
  }
  __syncthreads();
  chroma_finish(H, CH, A.tab, s_R, nf, r0, A.rows);
}

__global__ void __launch_bounds__(CQT_THREADS) vsyn_cqt_finish_kernel(const CqtCtx A) {
  const uint32_t g = blockIdx.x, tid = threadIdx.x;
  if (A.seg[g] != CQT_REFUSED) return frames_finish(A, A.cols);
  if (tid == 0 && A.refused) A.refused[g] = VSYN_CQT_RATE;
  float* rows = A.rows + (uint64_t)A.cols * A.segoff[g];
  const uint64_t nv = (uint64_t)A.cols * A.segF[g];
  for (uint64_t i = tid; i < nv; i += CQT_THREADS) rows[i] = __uint_as_float(0x7FC00000u);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct CqtWs {  // the stage's buffers: its own; the PCM is only read
  TableUpload tab, basis;
  std::vector<uint8_t> basis_host;  // the wavelet table of basis_key, kept from call to call
  std::vector<double> basis_key;    // the spec's fields and the rates the table holds, in the order of their indices
  uint32_t off_cls = 0, off_pairs = 0;
  DevBuf<uint32_t> segF, flags, refused;
  DevBuf<uint64_t> segoff;
  DevBuf<float> rows, mag;  // host form: the rows; chroma outputs: the magnitudes
};

static inline bool cqt_chroma_out(const vsyn_cqt_spec* sp) { return sp->output == VSYN_CQT_CHROMA || sp->output == VSYN_CQT_TONNETZ; }

// The checks of step 11 that need no rate.
static inline int cqt_check(const vsyn_cqt_spec* sp, uint32_t S, const uint32_t* rates, const char** err) {
  if (!sp) return fail(err, VSYN_ERR_INVALID, "constant-Q spec is NULL");
  if (sp->options & ~(VSYN_CQT_SCALE | VSYN_CQT_BASE_C)) return fail(err, VSYN_ERR_INVALID, "unknown constant-Q options 0x%x", sp->options);
  if (sp->n_bins < 1 || sp->n_bins > CQT_MAX_BINS) return fail(err, VSYN_ERR_INVALID, "n_bins %u outside [1, %u]", sp->n_bins, CQT_MAX_BINS);
  if (sp->bins_per_octave < 1 || sp->bins_per_octave > 256u) return fail(err, VSYN_ERR_INVALID, "bins_per_octave %u outside [1, 256]", sp->bins_per_octave);
  if (sp->hop_length < 1) return fail(err, VSYN_ERR_INVALID, "constant-Q hop_length must be >= 1");
  if (!std::isfinite(sp->fmin) || !(sp->fmin > 0.0)) return fail(err, VSYN_ERR_INVALID, "fmin %g must be finite and > 0", sp->fmin);
  if (!std::isfinite(sp->filter_scale) || !(sp->filter_scale > 0.0))
    return fail(err, VSYN_ERR_INVALID, "filter_scale %g must be finite and > 0", sp->filter_scale);
  if (!std::isfinite(sp->gamma) || !(sp->gamma >= 0.0)) return fail(err, VSYN_ERR_INVALID, "gamma %g must be finite and >= 0", sp->gamma);
  if (!std::isfinite(sp->tuning)) return fail(err, VSYN_ERR_INVALID, "tuning %g must be finite", sp->tuning);
  if (sp->power != 1u && sp->power != 2u) return fail(err, VSYN_ERR_INVALID, "power %u must be 1 or 2", sp->power);
  if (sp->norm > 2u) return fail(err, VSYN_ERR_INVALID, "norm %u must be 0 (none), 1 or 2", sp->norm);
  if (sp->output < VSYN_CQT_MAG || sp->output > VSYN_CQT_TONNETZ) return fail(err, VSYN_ERR_INVALID, "unknown constant-Q output %u", sp->output);
  if (sp->reserved) return fail(err, VSYN_ERR_INVALID, "constant-Q spec: reserved must be 0");
  if (cqt_chroma_out(sp)) {
    if (sp->n_chroma < 1 || sp->n_chroma > CHROMA_MAX) return fail(err, VSYN_ERR_INVALID, "n_chroma %u outside [1, %u]", sp->n_chroma, (uint32_t)CHROMA_MAX);
    if (sp->bins_per_octave % sp->n_chroma) return fail(err, VSYN_ERR_INVALID, "bins_per_octave %u is no multiple of n_chroma %u", sp->bins_per_octave, sp->n_chroma);
    if (sp->chroma_norm > VSYN_CHROMA_NORM_MAX) return fail(err, VSYN_ERR_INVALID, "unknown chroma_norm %u", sp->chroma_norm);
  }
  if (S && !rates) return fail(err, VSYN_ERR_INVALID, "sample_rates is NULL");
  return VSYN_OK;
}

static inline uint32_t cqt_dim(const vsyn_cqt_spec* sp) {
  return sp->output == VSYN_CQT_MAG ? sp->n_bins : sp->output == VSYN_CQT_COMPLEX ? 2u * sp->n_bins : sp->output == VSYN_CQT_CHROMA ? sp->n_chroma : 6u;
}

struct CqtLengths {
  std::vector<double> f, N;
  std::vector<uint32_t> L, h;
  uint64_t total = 0;
  bool refused = false;  // step 10
};

// Steps 1 to 3 and step 10's test at rate sr (> 0); sp is checked.
static inline CqtLengths cqt_lengths(const vsyn_cqt_spec* sp, uint32_t sr) {
  const uint32_t nb = sp->n_bins;
  const double bpo = (double)sp->bins_per_octave;
  CqtLengths o;
  o.f.resize(nb);
  o.N.resize(nb);
  o.L.resize(nb);
  o.h.resize(nb);
  const double f0 = sp->fmin * exp2(sp->tuning / bpo);
  const double r = exp2(1.0 / bpo), alpha = (r * r - 1.0) / (r * r + 1.0), Q = sp->filter_scale / alpha;
  for (uint32_t k = 0; k < nb; ++k) {
    o.f[k] = f0 * exp2((double)k / bpo);
    o.N[k] = (Q * (double)sr) / (o.f[k] + sp->gamma / alpha);
    const double hi = ceil(o.N[k] / 2.0), lo = floor(o.N[k] / 2.0);
    o.h[k] = hi < 4294967295.0 ? (uint32_t)hi : 0xFFFFFFFFu;
    o.L[k] = hi + lo < 4294967295.0 ? (uint32_t)(hi + lo) : 0xFFFFFFFFu;
    o.total += o.L[k];
  }
  o.refused = o.f[nb - 1u] * (1.0 + 0.5 * CQT_HANN_BW / Q) > (double)sr / 2.0;
  return o;
}

// The caps of step 11 for a rate that step 10 does not refuse.
static inline int cqt_check_caps(const CqtLengths& len, uint32_t sr, const char** err) {
  if (len.L[0] > VSYN_CQT_MAX_LENGTH)
    return fail(err, VSYN_ERR_INVALID, "constant-Q: the longest wavelet at %u Hz has %u samples, above %u", sr, len.L[0], VSYN_CQT_MAX_LENGTH);
  if (len.total > VSYN_CQT_MAX_TABLE)
    return fail(err, VSYN_ERR_INVALID, "constant-Q: the wavelets at %u Hz have %llu samples in all, above %u", sr, (unsigned long long)len.total,
                VSYN_CQT_MAX_TABLE);
  return VSYN_OK;
}

// The float32 pairs of bin k (step 4) into out[2 L_k].
static inline void cqt_wavelet(const vsyn_cqt_spec* sp, uint32_t sr, const CqtLengths& len, uint32_t k, float* out) {
  const uint32_t L = len.L[k];
  const double dl = (double)L, f = len.f[k];
  std::vector<double> w(L);
  double s1 = 0.0, s2 = 0.0;
  for (uint32_t j = 0; j < L; ++j) {
    w[j] = 0.5 - 0.5 * cos(2.0 * M_PI * (double)j / dl);
    s1 += w[j];
    s2 += w[j] * w[j];
  }
  const double n = sp->norm == 1u ? s1 : sp->norm == 2u ? sqrt(s2) : 1.0;
  for (uint32_t j = 0; j < L; ++j) {
    const double m = (double)j - (double)len.h[k];
    const double p = 2.0 * M_PI * f * m / (double)sr;
    out[2u * j] = (float)(w[j] * cos(p) / n);
    out[2u * j + 1u] = (float)(-(w[j] * sin(p)) / n);
  }
}

// The chroma class of every bin (step 7); sp is checked, a chroma output.
static inline void cqt_classes(const vsyn_cqt_spec* sp, uint32_t* cls) {
  const uint32_t bpo = sp->bins_per_octave, nc = sp->n_chroma, nm = bpo / nc;
  double m0 = fmod(12.0 * (log2(sp->fmin) - log2(440.0)) + 69.0, 12.0);
  if (m0 < 0.0) m0 += 12.0;
  const double rd = nearbyint(((double)nc / 12.0) * ((sp->options & VSYN_CQT_BASE_C) ? m0 : m0 - 9.0));  // ties to even, as numpy.round
  int64_t roll = (int64_t)rd % (int64_t)nc;
  if (roll < 0) roll += nc;
  for (uint32_t k = 0; k < sp->n_bins; ++k) cls[k] = ((((k % bpo) + nm / 2u) % bpo) / nm + (uint32_t)roll) % nc;
}

// Offsets, transform, fold and finishing kernels on stream s; frames from d_frames, else from si. f_max bounds every segment's rows.
// d_refused [S] may be NULL. seg_tuning [S] (NULL: sp->tuning for all): each segment's own tuning; the wavelet table then holds one
// set of bins per distinct (rate, tuning) pair where it holds one per rate otherwise, and a segment's entry indexes the pairs: the
// kernels read it as they read a rate index. Caller holds the handle's lock and has run cqt_check.
static inline int cqt_launch(CqtWs& ws, int device, const vsyn_cqt_spec* sp, uint32_t S, const uint32_t* rates, const float* d_pcm, uint64_t plane,
                             uint32_t C, const uint32_t* d_frames, const SegInfo* si, uint64_t f_max, float* d_rows, uint64_t* d_segoff,
                             uint32_t* d_refused, hipStream_t s, const char** err, const double* seg_tuning = nullptr) {
  if (int rc = frames_check_call(S, d_pcm, d_rows, plane, err)) return rc;
  const uint32_t nb = sp->n_bins, cols = cqt_dim(sp);
  const bool chroma = cqt_chroma_out(sp);
  // the (rate, tuning) pairs the call computes at, in order of first appearance, and each segment's entry
  typedef std::pair<uint32_t, double> Pair;
  std::vector<Pair> distinct, refused_pairs;
  std::vector<uint32_t> seg(S);
  std::vector<CqtLengths> lens;
  vsyn_cqt_spec sq = *sp;  // the spec at a pair's tuning
  for (uint32_t g = 0; g < S; ++g) {
    if (!rates[g]) {
      seg[g] = CQT_SKIP;
      continue;
    }
    const Pair p(rates[g], seg_tuning ? seg_tuning[g] : sp->tuning);
    if (std::find(refused_pairs.begin(), refused_pairs.end(), p) != refused_pairs.end()) {
      seg[g] = CQT_REFUSED;
      continue;
    }
    const auto it = std::find(distinct.begin(), distinct.end(), p);
    if (it != distinct.end()) {
      seg[g] = (uint32_t)(it - distinct.begin());
      continue;
    }
    sq.tuning = p.second;
    CqtLengths len = cqt_lengths(&sq, p.first);
    if (len.refused) {
      refused_pairs.push_back(p);
      seg[g] = CQT_REFUSED;
      continue;
    }
    if (int rc = cqt_check_caps(len, p.first, err)) return rc;
    seg[g] = (uint32_t)distinct.size();
    distinct.push_back(p);
    lens.push_back(std::move(len));
  }
  // the wavelet table: rebuilt when the spec or the pairs change
  std::vector<double> key = {(double)nb, (double)sp->bins_per_octave, (double)sp->options, (double)sp->norm, (double)(chroma ? sp->n_chroma : 0u),
                             sp->fmin, sp->filter_scale, sp->gamma};
  for (const Pair& p : distinct) {
    key.push_back((double)p.first);
    key.push_back(p.second);
  }
  const bool rebuild = key != ws.basis_key;
  if (rebuild) {
    ws.basis_key.clear();  // (a throw below leaves no stale table behind a matching key)
    const size_t off_cls = sizeof(CqtBin) * distinct.size() * nb, off_pairs = align_up(off_cls + 4u * (size_t)nb, 16);
    uint64_t pairs = 0;
    for (const CqtLengths& l : lens) pairs += l.total;
    if (off_pairs + 8u * pairs > 0xFFFFFFFFull)
      return fail(err, VSYN_ERR_INVALID, "too many distinct (sample rate, tuning) pairs (%zu) for one constant-Q table", distinct.size());
    ws.basis_host.assign(off_pairs + 8u * (size_t)pairs + 16u, 0);
    CqtBin* bins = (CqtBin*)ws.basis_host.data();
    float* pr = (float*)(ws.basis_host.data() + off_pairs);
    uint32_t at = 0;
    for (size_t r = 0; r < distinct.size(); ++r)
      for (uint32_t k = 0; k < nb; ++k) {
        const CqtLengths& l = lens[r];
        bins[r * nb + k] = CqtBin{l.L[k], l.h[k], at, (float)((sp->options & VSYN_CQT_SCALE) ? sqrt(l.N[k]) : l.N[k])};
        cqt_wavelet(sp, distinct[r].first, l, k, pr + 2u * (size_t)at);  // (reads the bin's frequency from l, not the spec's tuning)
        at += l.L[k];
      }
    if (chroma) cqt_classes(sp, (uint32_t*)(ws.basis_host.data() + off_cls));
    ws.off_cls = (uint32_t)off_cls;
    ws.off_pairs = (uint32_t)off_pairs;
  }
  // the per-call table: SpecHeader | ChromaHeader | phi [6][n_chroma] | seg [S]
  const size_t off_ch = align_up(sizeof(SpecHeader), 16), off_phi = off_ch + sizeof(ChromaHeader);
  const size_t off_seg = align_up(off_phi + (chroma ? 4u * 6u * (size_t)sp->n_chroma : 0u), 16);
  std::vector<uint8_t> tab(off_seg + 4u * (size_t)S + 16u, 0);
  SpecHeader T;
  memset(&T, 0, sizeof(T));
  T.kind = sp->output == VSYN_CQT_TONNETZ ? VSYN_SPEC_TONNETZ : VSYN_SPEC_CHROMA;
  T.pad = (uint32_t)off_ch;
  T.dim = cols;
  T.S = S;
  memcpy(tab.data(), &T, sizeof(T));
  const ChromaHeader CH = {chroma ? sp->n_chroma : 0u, sp->chroma_norm, 0u, (uint32_t)off_phi};
  memcpy(tab.data() + off_ch, &CH, sizeof(CH));
  if (chroma) chroma_phi(sp->n_chroma, (float*)(tab.data() + off_phi));
  if (S) memcpy(tab.data() + off_seg, seg.data(), 4u * (size_t)S);

  const uint32_t hop = sp->hop_length;
  CqtCtx A;
  if (int rc = frames_begin(ws, device, tab, CQT_FT, hop, true, S, d_pcm, plane, C, d_frames, si, f_max, d_rows, d_segoff, d_refused, s, err,
                            []() -> int { return VSYN_OK; }, A))  // (32 KiB of dynamic LDS at most: no limit to raise)
    return rc;
  if (rebuild) {
    if (int rc = ws.basis.upload(ws.basis_host, s, err)) return rc;
    ws.basis_key = key;
  } else {
    HIPCHK(hipStreamWaitEvent(s, ws.basis.ev, 0));  // (the upload may have gone down another stream)
  }
  if (chroma) HIPCHK(ws.mag.ensure((size_t)f_max * S * nb + 1));
  A.tab = ws.tab.dev.p;
  A.basis = ws.basis.dev.p;
  A.seg = (const uint32_t*)(ws.tab.dev.p + off_seg);
  A.nb = nb;
  A.out = sp->output;
  A.power = sp->power;
  A.cols = cols;
  A.off_cls = ws.off_cls;
  A.off_pairs = ws.off_pairs;
  A.mag = chroma ? ws.mag.p : nullptr;
  const size_t lds = 4u * ((size_t)(CQT_FT - 1u) * std::min<uint32_t>(hop, VSYN_CQT_CHUNK) + VSYN_CQT_CHUNK);
  return frames_launch(A, vsyn_cqt_offsets_kernel, vsyn_cqt_kernel, lds, vsyn_cqt_finish_kernel, s, err, (nb + CQT_BPW - 1u) / CQT_BPW,
                       chroma ? vsyn_cqt_fold_kernel : nullptr);
}
