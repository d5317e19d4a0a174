// vsyn_pcen.h — per-channel energy normalisation (librosa.pcen, max_size = 1) of spectral rows already on the device. Semantics:
// include/vorbis_synth_hip.h, "PCEN".
//
// The smoother M[f] = b S[f] + q M[f-1], M[-1] = 1, is the one stage here that is sequential along a segment's rows. It runs as a
// blocked scan whose decomposition is a function of the segment's rows alone: blocks of PCEN_BLK rows counted from the segment's first
// row, whatever the grid and the segment's place in the batch, so the same rows give the same bits. The host knows every segment's
// row count and uploads one PcenSeg per segment (row offset, offset of its blocks, rows, b, q = 1 - b, q^PCEN_BLK, all in double).
// Three launches on one stream, lanes along the columns in each (contiguous loads and stores):
//   1. vsyn_pcen_part_kernel   per (segment, block but the last, column): the block's zero-state response at its last row, the
//                              recurrence from m = 0 over the block's rows in ascending order, float64 -> part[block][j].
//   2. vsyn_pcen_carry_kernel  per (segment, column), over the blocks in ascending order: carry[0] = 1,
//                              carry[k+1] = part[k] + q^PCEN_BLK carry[k]. The last block's outgoing carry is never formed.
//   3. vsyn_pcen_apply_kernel  per (segment, block, column): from m = carry[k] over the block's rows in ascending order M, the gain
//                              and the compression in float64, one rounding to float32. A thread reads in[f][j] before it writes
//                              out[f][j] and nobody else touches that element: out may be in.
// No atomics. Nothing here reads or writes stream state, the overlap carry or PCM.
#pragma once
#include "vsyn_device.h"
#include "vsyn_host.h"

#define PCEN_THREADS 256
#define PCEN_BLK 64u  // rows per block of the scan

struct PcenSeg : RowBlkSeg {  // blk: the segment's first block in part / carry
  double b, q, qblk;  // the coefficient, 1 - b, q^PCEN_BLK
};

struct PcenCtx {  // launch arguments
  const PcenSeg* seg;
  const float* in;  // [rows][D]
  float* out;       // [rows][D]
  double* part;     // [blocks][D]
  double* carry;    // [blocks][D]
  uint32_t D, mode;  // mode: 0 power = 0, 1 bias = 0, 2 the general form
  float scale;
  double gain, bias, power, eps, log_eps, bias_pow;  // log(eps) and bias^power from the host
};

// Thread layout (row_lane): group ty of workgroup x takes block x G + ty.
// S = float32(X * float32(scale)), one rounding; then one step of the smoother. Both kernels that walk rows go through these two.
__device__ __forceinline__ float pcen_scaled(float x, float scale) { return x * scale; }
__device__ __forceinline__ double pcen_step(double m, double b, double q, float s) { return b * (double)s + q * m; }

// The gain and the compression of one element in librosa's log-space form (include/vorbis_synth_hip.h, "PCEN", step 4).
__device__ __forceinline__ float pcen_value(const PcenCtx& A, float s, double m) {
  const double g = exp(-A.gain * (A.log_eps + log1p(m / A.eps)));
  double y;
  if (A.mode == 0u)
    y = log1p((double)s * g);
  else if (A.mode == 1u)
    y = exp(A.power * (log((double)s) + log(g)));
  else
    y = A.bias_pow * expm1(A.power * log1p((double)s * g / A.bias));
  return (float)y;
}

__global__ void __launch_bounds__(PCEN_THREADS) vsyn_pcen_part_kernel(const PcenCtx A) {
  const PcenSeg sg = A.seg[blockIdx.y];
  const RowLane L = row_lane<PCEN_THREADS>(A.D);
  if (L.ty >= L.G) return;
  const uint32_t nblk = (sg.F + PCEN_BLK - 1u) / PCEN_BLK;
  const uint64_t k = (uint64_t)blockIdx.x * L.G + L.ty;
  if (k + 1u >= nblk) return;  // the last block hands nothing on: every block here has PCEN_BLK rows
  const uint32_t D = A.D;
  for (uint32_t j = L.tx; j < D; j += L.wd) {
    const float* x = A.in + (sg.off + k * PCEN_BLK) * D + j;
    double m = 0.0;
    for (uint32_t f = 0; f < PCEN_BLK; ++f, x += D) m = pcen_step(m, sg.b, sg.q, pcen_scaled(*x, A.scale));
    A.part[(sg.blk + k) * D + j] = m;
  }
}

__global__ void __launch_bounds__(PCEN_THREADS) vsyn_pcen_carry_kernel(const PcenCtx A) {
  const PcenSeg sg = A.seg[blockIdx.y];
  const uint32_t j = blockIdx.x * PCEN_THREADS + threadIdx.x, D = A.D;
  if (j >= D || sg.F == 0) return;
  const uint32_t nblk = (sg.F + PCEN_BLK - 1u) / PCEN_BLK;
  const double* p = A.part + sg.blk * D + j;
  double* c = A.carry + sg.blk * D + j;
  double m = 1.0;
  for (uint32_t k = 0;; ++k) {
    c[(size_t)k * D] = m;
    if (k + 1u >= nblk) break;
    m = p[(size_t)k * D] + sg.qblk * m;
  }
}

__global__ void __launch_bounds__(PCEN_THREADS) vsyn_pcen_apply_kernel(const PcenCtx A) {
  const PcenSeg sg = A.seg[blockIdx.y];
  const RowLane L = row_lane<PCEN_THREADS>(A.D);
  if (L.ty >= L.G) return;
  const uint64_t k = (uint64_t)blockIdx.x * L.G + L.ty;
  if (k * PCEN_BLK >= sg.F) return;
  const uint32_t D = A.D, n = min(PCEN_BLK, sg.F - (uint32_t)(k * PCEN_BLK));
  for (uint32_t j = L.tx; j < D; j += L.wd) {
    const size_t e = (sg.off + k * PCEN_BLK) * D + j;
    const float* x = A.in + e;
    float* y = A.out + e;
    double m = A.carry[(sg.blk + k) * D + j];
    for (uint32_t f = 0; f < n; ++f, x += D, y += D) {
      const float s = pcen_scaled(*x, A.scale);
      m = pcen_step(m, sg.b, sg.q, s);
      *y = pcen_value(A, s, m);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct PcenWs {  // the stage's buffers
  TableUpload tab;
  DevBuf<double> part, carry;  // [blocks][D] each
};

static inline bool pcen_num(double v, bool positive) { return std::isfinite(v) && (positive ? v > 0.0 : v >= 0.0); }

// The checks of the spec that need neither rates nor rows.
static inline int pcen_check(const vsyn_spectral_pcen* p, const char** err) {
  if (!p) return fail(err, VSYN_ERR_INVALID, "pcen spec is NULL");
  if (!pcen_num(p->gain, false)) return fail(err, VSYN_ERR_INVALID, "pcen: gain must be finite and >= 0");
  if (!pcen_num(p->bias, false)) return fail(err, VSYN_ERR_INVALID, "pcen: bias must be finite and >= 0");
  if (!pcen_num(p->power, false)) return fail(err, VSYN_ERR_INVALID, "pcen: power must be finite and >= 0");
  if (!pcen_num(p->eps, true)) return fail(err, VSYN_ERR_INVALID, "pcen: eps must be finite and > 0");
  if (!pcen_num(p->time_constant, true)) return fail(err, VSYN_ERR_INVALID, "pcen: time_constant must be finite and > 0");
  if (!pcen_num(p->scale, true)) return fail(err, VSYN_ERR_INVALID, "pcen: scale must be finite and > 0");
  if (!(p->b == 0.0 || (p->b > 0.0 && p->b <= 1.0))) return fail(err, VSYN_ERR_INVALID, "pcen: b must be 0 (derived) or in (0, 1]");
  return VSYN_OK;
}

// The coefficient of a (checked) spec for rows computed at `rate` every `hop` samples: b as given, else librosa's
// (sqrt(1 + 4 t^2) - 1) / (2 t^2), t = time_constant rate / hop. 0 where none can be formed.
static inline double pcen_b(const vsyn_spectral_pcen* p, uint32_t rate, uint32_t hop) {
  if (p->b != 0.0) return p->b;
  if (!rate || !hop) return 0.0;
  const double t = p->time_constant * (double)rate / (double)hop;
  const double b = (sqrt(1.0 + 4.0 * t * t) - 1.0) / (2.0 * t * t);
  return b > 0.0 && b <= 1.0 ? b : 0.0;
}

// The checks of a call: the spec, and what a derived coefficient needs.
static inline int pcen_check_call(const vsyn_spectral_pcen* p, uint32_t D, uint32_t S, const uint64_t* seg_rows, const uint32_t* rates, uint32_t hop,
                                  const char** err) {
  if (int rc = pcen_check(p, err)) return rc;
  if (D < 1) return fail(err, VSYN_ERR_INVALID, "pcen: dim must be >= 1");
  if (S && !seg_rows) return fail(err, VSYN_ERR_INVALID, "seg_rows is NULL");
  if (p->b == 0.0 && hop < 1) return fail(err, VSYN_ERR_INVALID, "pcen: b = 0 (derived) needs hop_length >= 1");
  if (p->b == 0.0 && S && !rates) return fail(err, VSYN_ERR_INVALID, "pcen: b = 0 (derived) needs the segments' sample rates");
  for (uint32_t g = 0; g < S; ++g) {
    if (seg_rows[g] > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "segment %u: too many rows", g);
    if (seg_rows[g] && (!rates || rates[g]) && pcen_b(p, rates ? rates[g] : 0u, hop) == 0.0)
      return fail(err, VSYN_ERR_INVALID, "segment %u: pcen: no coefficient in (0, 1] from time_constant %g at rate %u, hop %u", g, p->time_constant,
                  rates[g], hop);
  }
  return VSYN_OK;
}

// The stage's kernels on stream s: d_in [rows][D] -> d_out [rows][D], which may be d_in. A segment with rates[g] = 0 (rates != NULL)
// is skipped: its rows are neither read nor written. Caller holds the handle's lock and has run pcen_check_call.
static inline int pcen_launch(PcenWs& ws, int device, const vsyn_spectral_pcen* p, uint32_t D, uint32_t S, const uint64_t* seg_rows, const uint32_t* rates,
                              uint32_t hop, const float* d_in, float* d_out, hipStream_t s, const char** err) {
  if (S > 65535u) return fail(err, VSYN_ERR_INVALID, "too many segments (%u > 65535)", S);
  std::vector<uint8_t> tab(sizeof(PcenSeg) * (size_t)S);
  PcenSeg* seg = (PcenSeg*)tab.data();
  const RowTotals t = row_segs_fill(seg, S, seg_rows, rates, PCEN_BLK);
  for (uint32_t g = 0; g < S; ++g) {
    seg[g].b = seg[g].F ? pcen_b(p, rates ? rates[g] : 0u, hop) : 1.0;
    seg[g].q = 1.0 - seg[g].b;
    seg[g].qblk = pow(seg[g].q, (double)PCEN_BLK);
  }
  const uint64_t blocks = t.blocks, f_max = t.f_max;
  if (f_max == 0) return VSYN_OK;
  HIPCHK(hipSetDevice(device));
  HIPCHK(ws.part.ensure(blocks * D));
  HIPCHK(ws.carry.ensure(blocks * D));
  if (int rc = ws.tab.upload(tab, s, err)) return rc;
  PcenCtx A;
  A.seg = (const PcenSeg*)ws.tab.dev.p;
  A.in = d_in;
  A.out = d_out;
  A.part = ws.part.p;
  A.carry = ws.carry.p;
  A.D = D;
  A.mode = p->power == 0.0 ? 0u : p->bias == 0.0 ? 1u : 2u;
  A.scale = (float)p->scale;
  A.gain = p->gain;
  A.bias = p->bias;
  A.power = p->power;
  A.eps = p->eps;
  A.log_eps = log(p->eps);
  A.bias_pow = pow(p->bias, p->power);
  const uint32_t G = PCEN_THREADS / std::min<uint32_t>(D, PCEN_THREADS);
  const uint64_t nblk = (f_max + PCEN_BLK - 1u) / PCEN_BLK;
  const dim3 grid((uint32_t)((nblk + G - 1u) / G), S), cgrid((D + PCEN_THREADS - 1u) / PCEN_THREADS, S);
  VSYN_LAUNCH(vsyn_pcen_part_kernel, grid, dim3(PCEN_THREADS), 0, s, A);
  VSYN_LAUNCH(vsyn_pcen_carry_kernel, cgrid, dim3(PCEN_THREADS), 0, s, A);
  VSYN_LAUNCH(vsyn_pcen_apply_kernel, grid, dim3(PCEN_THREADS), 0, s, A);
  return VSYN_OK;
}
