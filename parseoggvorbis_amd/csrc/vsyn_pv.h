// vsyn_pv.h — the phase vocoder: complex rows already on the device to the complex rows of a time-stretched signal
// (librosa.phase_vocoder's arithmetic). Semantics: include/vorbis_synth_hip.h, "phase vocoder". Design and measurements: DESIGN.md 6r.
//
// Three launches on one stream behind a table upload (phi [nbins] float64, then one PvSeg per segment):
//   vsyn_pv_kernel<false>  one workgroup of 256 threads per (block of VSYN_PV_BLOCK output rows, tile of 256 bins, segment): a thread
//                          owns one bin and walks its block's output rows in ascending t, adding inc_t from 0.0; the block's sum goes
//                          to the workspace, [blocks][nbins] float64.
//   vsyn_pv_carry_kernel   a thread per (segment, bin): A[0][k] plus that segment's block sums in ascending order; every sum is
//                          replaced by the carry in front of its block.
//   vsyn_pv_kernel<true>   the first kernel's grid and walk again, from the carry: m cos(acc), m sin(acc) of every output row.
// Lanes run along k: a wavefront reads a row's bins and writes an output row's at stride 1, 8 bytes a lane. inc_t is recomputed in
// the emit kernel by the same device function on the same rows, so its bits are the first kernel's. Inside a walk a register
// carries the angle and magnitude of row i_t + 1 to the step that reads it as row i_t (and both while i_t stands still, rate < 1):
// one float64 atan2 per input row and walk. No atomics, no LDS, no scratch; nothing depends on the grid, the tile or the segment's
// place in the batch. The rows are only read.
#pragma once
#include "vsyn_istft.h"

#define PV_THREADS 256u  // (VSYN_PV_BLOCK, the output rows per block of the phase sum, is the header's: a constant of the contract)
#define PV_TWO_PI 6.283185307179586476925286766559  // the double nearest 2 pi, which is 2 * (the double nearest pi)
#define PV_PI 3.141592653589793238462643383279

struct PvSeg {
  uint64_t in_off, out_off;  // first row of the segment in the input and in the output rows
  uint64_t sum_off;          // first block of the segment in the workspace
  uint32_t F, F_out;         // rows in, rows out
  double rate;
};

struct PvCtx {  // launch arguments
  const double* phi;  // [nbins]
  const PvSeg* seg;   // [S]
  const float2* rows;
  float2* out;
  double* sums;  // [blocks][nbins]: block sums, then carries
  uint32_t nb;
};

// Bin k of row i of a segment of F rows at X; rows behind the last read as +0 + 0i.
__device__ __forceinline__ float2 pv_load(const float2* X, uint32_t nb, uint32_t F, uint64_t i, uint32_t k) {
  return i < F ? X[i * nb + k] : make_float2(0.f, 0.f);
}

// atan2(im, re) in float64 with C99's signed zeros spelled out: (+-0, -0) -> +-pi, (+-0, +0) -> +-0.
__device__ __forceinline__ double pv_angle(float2 x) {
  const double re = (double)x.x, im = (double)x.y;
  if (im == 0.0 && re == 0.0) return copysign(signbit(re) ? PV_PI : 0.0, im);
  return atan2(im, re);
}

__device__ __forceinline__ double pv_mag(float2 x) {
  const double re = (double)x.x, im = (double)x.y;
  return sqrt(re * re + im * im);
}

// inc_t from the angles of rows i_t and i_t + 1
__device__ __forceinline__ double pv_inc(double a0, double a1, double phi) {
  const double d = a1 - a0 - phi;
  return phi + (d - PV_TWO_PI * rint(d / PV_TWO_PI));
}

template <bool EMIT>
__global__ void __launch_bounds__(PV_THREADS) vsyn_pv_kernel(const PvCtx P) {
  const PvSeg sg = P.seg[blockIdx.z];
  const uint64_t t0 = (uint64_t)blockIdx.x * VSYN_PV_BLOCK;
  const uint32_t k = blockIdx.y * PV_THREADS + threadIdx.x, nb = P.nb;
  if (t0 >= sg.F_out || k >= nb) return;
  const uint32_t nt = (uint32_t)min((uint64_t)VSYN_PV_BLOCK, (uint64_t)sg.F_out - t0);
  const float2* X = P.rows + sg.in_off * nb;
  float2* Y = P.out + (sg.out_off + t0) * nb + k;
  double* sum = P.sums + (sg.sum_off + blockIdx.x) * nb + k;
  const double phi = P.phi[k];
  double acc = EMIT ? *sum : 0.0;
  uint64_t have = ~0ull;  // the row a0 and g0 belong to
  double a0 = 0.0, a1 = 0.0, g0 = 0.0, g1 = 0.0;
  for (uint32_t u = 0; u < nt; ++u) {
    const double s = (double)(t0 + u) * sg.rate, fl = floor(s);
    const uint64_t i = (uint64_t)fl;
    if (i != have) {
      if (have != ~0ull && i == have + 1u) {
        a0 = a1;
        g0 = g1;
      } else {
        const float2 x = pv_load(X, nb, sg.F, i, k);
        a0 = pv_angle(x);
        if (EMIT) g0 = pv_mag(x);
      }
      const float2 x = pv_load(X, nb, sg.F, i + 1u, k);
      a1 = pv_angle(x);
      if (EMIT) g1 = pv_mag(x);
      have = i;
    }
    if (EMIT) {
      const double alpha = s - fl, m = (1.0 - alpha) * g0 + alpha * g1;
      double sn, cs;
      sincos(acc, &sn, &cs);
      Y[(size_t)u * nb] = make_float2((float)(m * cs), (float)(m * sn));
    }
    acc = acc + pv_inc(a0, a1, phi);
  }
  if (!EMIT) *sum = acc;
}

__global__ void __launch_bounds__(PV_THREADS) vsyn_pv_carry_kernel(const PvCtx P) {
  const PvSeg sg = P.seg[blockIdx.y];
  const uint32_t k = blockIdx.x * PV_THREADS + threadIdx.x, nb = P.nb;
  if (sg.F_out == 0u || k >= nb) return;  // (F_out >= 1 has F >= 1: row 0 is there)
  const uint32_t blocks = (sg.F_out + VSYN_PV_BLOCK - 1u) / VSYN_PV_BLOCK;
  double* sum = P.sums + sg.sum_off * nb + k;
  double c = pv_angle(P.rows[sg.in_off * nb + k]);
  for (uint32_t b = 0; b < blocks; ++b, sum += nb) {
    const double s = *sum;
    *sum = c;
    c = c + s;
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct PvWs {  // the stage's buffers
  TableUpload tab;
  DevBuf<double> sums;  // [blocks][n_fft / 2 + 1]
};

// ceil(rows / rate) in double: len(numpy.arange(0, rows, rate)). 0 for a rate the stage refuses; saturates.
static inline uint64_t pv_num_rows(uint64_t rows, double rate) {
  if (!std::isfinite(rate) || !(rate > 0.0)) return 0;
  const double x = std::ceil((double)rows / rate);
  return x < 18446744073709551616.0 ? (uint64_t)x : ~0ull;
}

// The framing the stage reads of sp (n_fft, hop_length), as the inverse STFT checks it.
static inline int pv_check(const vsyn_spectral_spec* sp, const char** err) {
  if (!sp) return fail(err, VSYN_ERR_INVALID, "spectral spec is NULL");
  vsyn_spectral_spec f = {};
  f.n_fft = f.win_length = sp->n_fft;
  f.hop_length = sp->hop_length;
  return istft_check(&f, err);
}

// The checks of a call; fills f_out[S] and the totals.
static inline int pv_check_call(const vsyn_spectral_spec* sp, uint32_t S, const uint64_t* seg_rows, const double* rates, std::vector<uint64_t>& f_out,
                                uint64_t* total_in, uint64_t* total_out, const char** err) {
  if (int rc = pv_check(sp, err)) return rc;
  if (S > 65535u) return fail(err, VSYN_ERR_INVALID, "too many segments (%u > 65535)", S);
  if (S && !seg_rows) return fail(err, VSYN_ERR_INVALID, "seg_rows is NULL");
  if (S && !rates) return fail(err, VSYN_ERR_INVALID, "rates is NULL");
  f_out.assign(S, 0);
  *total_in = *total_out = 0;
  for (uint32_t g = 0; g < S; ++g) {
    if (!std::isfinite(rates[g]) || !(rates[g] > 0.0)) return fail(err, VSYN_ERR_INVALID, "segment %u: rate %g is not a finite number above 0", g, rates[g]);
    if (seg_rows[g] > ISTFT_MAX_ROWS) return fail(err, VSYN_ERR_INVALID, "segment %u: too many rows", g);
    f_out[g] = pv_num_rows(seg_rows[g], rates[g]);
    if (f_out[g] > ISTFT_MAX_ROWS)
      return fail(err, VSYN_ERR_INVALID, "segment %u: too many rows out (%llu rows at rate %g)", g, (unsigned long long)seg_rows[g], rates[g]);
    *total_in += seg_rows[g];
    *total_out += f_out[g];
  }
  return VSYN_OK;
}

// The stage's kernels on stream s. Caller holds the handle's lock and has run pv_check_call (f_out is its result) and the checks of
// its pointers.
static inline int pv_launch(PvWs& ws, int device, const vsyn_spectral_spec* sp, uint32_t S, const uint64_t* seg_rows, const double* rates,
                            const uint64_t* f_out, const float* d_rows, float* d_out, hipStream_t s, const char** err) {
  const uint32_t n = sp->n_fft, nb = n / 2u + 1u;
  uint64_t blocks = 0, bx = 0;
  for (uint32_t g = 0; g < S; ++g) {
    const uint64_t b = (f_out[g] + VSYN_PV_BLOCK - 1u) / VSYN_PV_BLOCK;
    blocks += b;
    bx = std::max(bx, b);
  }
  if (bx == 0) return VSYN_OK;
  const size_t off_seg = align_up(sizeof(double) * nb, 16);
  std::vector<uint8_t> tab(off_seg + sizeof(PvSeg) * (size_t)S);
  double* phi = (double*)tab.data();
  const double val = 1.0 / ((double)n * (1.0 / PV_TWO_PI));  // numpy.fft.rfftfreq(n_fft, d = 1 / (2 pi))
  for (uint32_t k = 0; k < nb; ++k) phi[k] = (double)sp->hop_length * ((double)k * val);
  PvSeg* seg = (PvSeg*)(tab.data() + off_seg);
  uint64_t in = 0, out = 0, sum = 0;
  for (uint32_t g = 0; g < S; ++g) {
    seg[g] = PvSeg{in, out, sum, (uint32_t)seg_rows[g], (uint32_t)f_out[g], rates[g]};
    in += seg_rows[g];
    out += f_out[g];
    sum += (f_out[g] + VSYN_PV_BLOCK - 1u) / VSYN_PV_BLOCK;
  }
  HIPCHK(hipSetDevice(device));
  HIPCHK(ws.sums.ensure(blocks * nb + 1));
  if (int rc = ws.tab.upload(tab, s, err)) return rc;
  PvCtx P;
  P.phi = (const double*)ws.tab.dev.p;
  P.seg = (const PvSeg*)(ws.tab.dev.p + off_seg);
  P.rows = (const float2*)d_rows;
  P.out = (float2*)d_out;
  P.sums = ws.sums.p;
  P.nb = nb;
  const uint32_t kt = (nb + PV_THREADS - 1u) / PV_THREADS;
  const dim3 grid((uint32_t)bx, kt, S);  // bx <= 2^24: ISTFT_MAX_ROWS / VSYN_PV_BLOCK
  VSYN_LAUNCH(vsyn_pv_kernel<false>, grid, dim3(PV_THREADS), 0, s, P);
  VSYN_LAUNCH(vsyn_pv_carry_kernel, dim3(kt, S), dim3(PV_THREADS), 0, s, P);
  VSYN_LAUNCH(vsyn_pv_kernel<true>, grid, dim3(PV_THREADS), 0, s, P);
  return VSYN_OK;
}
