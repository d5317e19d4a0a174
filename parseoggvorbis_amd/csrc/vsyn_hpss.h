// vsyn_hpss.h — harmonic-percussive separation (librosa.decompose.hpss) of spectral rows already on the device. Semantics:
// include/vorbis_synth_hip.h, "HPSS".
//
// One kernel, vsyn_hpss_kernel, one pass over the rows. A workgroup takes one tile of a segment: up to HPSS_TF rows (time) by up to
// HPSS_TD columns (bins); the tiles of a segment are balanced (ceil(F / tiles) rows, ceil(D / tiles) columns), so a dimension just
// past a multiple of the tile does not leave a sliver. Five steps with a barrier behind each of the first four:
//   1. stage   the tile's columns with the time halo, (Tf + kh - 1) x Td, into LDS, reflected at the segment's ends while loading,
//              as ORDER KEYS: uint32 images of the floats whose unsigned order is the floats' order (-0 below +0), every NaN as the
//              largest key. The window of an output is then a contiguous run of its line in LDS, and no row of another segment
//              is ever addressed.
//   2. select  out of LDS by sliding ranks, not per output but per STAGED ELEMENT: a lane takes one element a of a line (here a
//              column of the time strip), counts its rank in the first window that holds it (k compares), and slides that window
//              along the line: one element leaves, one enters, two compares a step. Ties are broken by position, so the order
//              is strict and exactly one element of a window has rank k / 2: its lane stores the median of that window. A NaN
//              (the largest key) ranks nothing: its lane sets a flag byte for each of its windows instead. No atomics (a median
//              word has one writer; a flag byte's writers all store 1), and no per-lane window array: the window never leaves
//              LDS, so there is nothing to spill. Cost per line ~ (T + k)(k + 2 min(T, k)) compares against T k^2 for a
//              selection per output: 10 x fewer at k = 63. Lanes run along the columns (consecutive LDS words; the element
//              index is wave-uniform).
//   3. stage   the tile's rows with the bin halo, Tf x (Td + kp - 1), reflected at the row's ends, over the same LDS words.
//   4. select  along bins: lanes along a row's elements (consecutive words again; the loop bounds differ per lane only at the
//              tile's two ends).
//   5. mask and output per element in float64, one rounding to float32, stored coalesced. X is the bin strip's centre.
// The median output runs one direction only.
// The result is a function of the segment's rows alone (a selection, then per-element arithmetic): neither the tiling, the grid nor
// the segment's place in the batch can change a bit. The kernel never writes its input: with d_out = d_in the host sends the
// output to the handle's HPSS workspace and copies it back on the same stream, since a tile's halo is another tile's output.
#pragma once
#include "vsyn_device.h"
#include "vsyn_host.h"

#define HPSS_THREADS 256
#define HPSS_TF 32u    // rows (time) of a tile
#define HPSS_TD 64u    // columns (bins) of a tile: one wave
#define HPSS_KMAX 63u  // largest kernel size
#define HPSS_VR (HPSS_TF + HPSS_KMAX - 1u)  // rows of the time strip
#define HPSS_HC (HPSS_TD + HPSS_KMAX - 1u)  // columns of the bin strip
#define HPSS_NAN_KEY 0xFFFFFFFFu
#define HPSS_MAX_DIM 0x3FFFFFFFu  // rows per segment, and columns: twice the count is an int32 in the reflection

typedef RowSeg HpssSeg;

struct HpssCtx {  // launch arguments
  const HpssSeg* seg;
  const float* in;  // [rows][D]
  float* out;       // [rows][D]
  uint32_t D, ntd;  // columns; column tiles of a segment
  uint32_t kh, kp;
  uint32_t percussive, output;  // vsyn_spectral_hpss.component, .output
  uint32_t mode;                // 0 power = +Inf (hard mask), 1 power = 1, 2 power = 2, 3 pow()
  uint32_t split;               // both margins are 1: a "bad" element's mask is 0.5
  double power, margin_h, margin_p;
};

// The order key of a float and back. Unsigned order of the keys = order of the floats, -0 below +0, -Inf first, +Inf last but for
// the NaNs, which all map to HPSS_NAN_KEY (whose float image is a NaN again).
__device__ __forceinline__ uint32_t hpss_key(float x) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return HPSS_NAN_KEY;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float hpss_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// numpy.pad(mode="symmetric") of an index into [0, n), as often as needed: i mod 2n, and 2n - 1 - that when it is >= n.
__device__ __forceinline__ uint32_t hpss_reflect(int32_t i, uint32_t n) {
  if ((uint32_t)i < n) return (uint32_t)i;
  const int32_t p = 2 * (int32_t)n;
  int32_t m = i % p;
  if (m < 0) m += p;
  return (uint32_t)m >= n ? (uint32_t)(p - 1 - m) : (uint32_t)m;
}

// Step 2 for one staged element: element e of a line of T + k - 1 keys (line[i * es]), against every window w (elements w .. w + k - 1,
// w < T) that holds it. A NaN flags those windows (nanf[w * os] = 1; whoever else writes that byte writes the same 1) and is done: a
// flagged window's median is not read. Any other element stores its key to med[w * os] where its rank is k / 2: over the elements
// of a line each of those words has at most one writer, and exactly one where the window holds no NaN.
__device__ __forceinline__ void hpss_select(const uint32_t* line, uint32_t es, uint32_t e, uint32_t T, uint32_t k, uint32_t* med, uint8_t* nanf,
                                            uint32_t os) {
  const uint32_t ka = line[e * es];
  const uint32_t w0 = e + 1u > k ? e + 1u - k : 0u, w1 = min(e, T - 1u);  // the first and the last window that hold e
  if (ka == HPSS_NAN_KEY) {
    for (uint32_t w = w0; w <= w1; ++w) nanf[w * os] = 1;
    return;
  }
  const uint32_t half = k >> 1;
  uint32_t rank = 0;  // keys of window w0 in front of a in the strict order (key, position)
#pragma unroll 4
  for (uint32_t x = 0; x < k; ++x) {
    const uint32_t i = w0 + x, kb = line[i * es];
    rank += (uint32_t)((kb < ka) | ((kb == ka) & (i < e)));
  }
  // a step: the window's output, then element w leaves (w < e: it stood in front of a on a tie) and element w + k enters (w + k > e:
  // it stands behind a on a tie). Four steps' keys are read ahead of the four outputs, so that their LDS latencies overlap.
  uint32_t w = w0;
  for (; w + 4u <= w1; w += 4u) {
    uint32_t leave[4], enter[4];
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
      leave[q] = line[(w + q) * es];
      enter[q] = line[(w + q + k) * es];
    }
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
      if (rank == half) med[(w + q) * os] = ka;
      rank += (uint32_t)(enter[q] < ka) - (uint32_t)(leave[q] <= ka);
    }
  }
  for (; w < w1; ++w) {
    if (rank == half) med[w * os] = ka;
    rank += (uint32_t)(line[(w + k) * es] < ka) - (uint32_t)(line[w * es] <= ka);
  }
  if (rank == half) med[w1 * os] = ka;
}

// librosa.util.softmask(A, B, power, split_zeros) of one element in float64 (include/vorbis_synth_hip.h, "HPSS", step 2); b is the
// reference median, multiplied by the margin here.
__device__ __forceinline__ double hpss_mask(const HpssCtx& A, float a32, float b32, double margin) {
  const double a0 = (double)a32, b0 = (double)b32 * margin;
  if (A.mode == 0u) return a0 > b0 ? 1.0 : 0.0;
  const double z = (a0 > b0 || a0 != a0) ? a0 : b0;  // max that hands a NaN on, as numpy.maximum does
  if (z < (double)1.17549435e-38f) return A.split ? 0.5 : 0.0;
  double a = a0 / z, b = b0 / z;
  if (A.mode == 2u) {
    a *= a;
    b *= b;
  } else if (A.mode == 3u) {
    a = pow(a, A.power);
    b = pow(b, A.power);
  }
  return a / (a + b);
}

__global__ void __launch_bounds__(HPSS_THREADS) vsyn_hpss_kernel(const HpssCtx A) {
  __shared__ uint32_t sS[HPSS_VR * HPSS_TD];    // the strip: time [Tf + kh - 1][HPSS_TD], then bins [Tf][Td + kp - 1] (dense)
  __shared__ uint32_t sMh[HPSS_TF * HPSS_TD];   // time medians (keys)
  __shared__ uint32_t sMp[HPSS_TF * HPSS_TD];   // bin medians (keys)
  __shared__ uint32_t sNan[2u * HPSS_TF * HPSS_TD / 4u];  // a byte per output: the time window holds a NaN; then the same for the bin window
  static_assert(HPSS_TF * HPSS_HC <= HPSS_VR * HPSS_TD, "the bin strip fits the time strip's words");
  const HpssSeg sg = A.seg[blockIdx.y];
  const uint32_t F = sg.F, D = A.D, kh = A.kh, kp = A.kp, hh = kh >> 1, hp = kp >> 1, tid = threadIdx.x;
  if (F == 0) return;
  // the segment's balanced tiling: a function of F and D alone
  const uint32_t ntf = (F + HPSS_TF - 1u) / HPSS_TF, tfw = (F + ntf - 1u) / ntf, tdw = (D + A.ntd - 1u) / A.ntd;
  const uint32_t tf = blockIdx.x / A.ntd, td = blockIdx.x - tf * A.ntd;
  const uint32_t f0 = tf * tfw, j0 = td * tdw;
  if (tf >= ntf || f0 >= F || j0 >= D) return;
  const uint32_t Tf = min(tfw, F - f0), Td = min(tdw, D - j0);
  const uint32_t R = Tf + kh - 1u, C = Td + kp - 1u;
  const float* in = A.in + sg.off * D;
  uint8_t* nanH = (uint8_t*)sNan;
  uint8_t* nanP = nanH + HPSS_TF * HPSS_TD;
  // the median output needs one direction only; everything else both
  const bool median = A.output == VSYN_HPSS_OUT_MEDIAN, want_h = !median || !A.percussive, want_p = !median || A.percussive;

  for (uint32_t e = tid; e < 2u * HPSS_TF * HPSS_TD / 4u; e += HPSS_THREADS) sNan[e] = 0u;
  if (want_h) {  // (wave-uniform)
    // 1. stage the time strip
    for (uint32_t e = tid; e < R * HPSS_TD; e += HPSS_THREADS) {
      const uint32_t r = e / HPSS_TD, j = e % HPSS_TD;
      uint32_t key = 0u;
      if (j < Td) key = hpss_key(in[(size_t)hpss_reflect((int32_t)(f0 + r) - (int32_t)hh, F) * D + j0 + j]);
      sS[e] = key;
    }
    __syncthreads();
    // 2. select along time: every staged element against the windows that hold it
    for (uint32_t e = tid; e < R * HPSS_TD; e += HPSS_THREADS) {
      const uint32_t r = e / HPSS_TD, j = e % HPSS_TD;
      if (j < Td) hpss_select(sS + j, HPSS_TD, r, Tf, kh, sMh + j, nanH + j, HPSS_TD);
    }
    __syncthreads();
  }
  // 3. stage the bin strip (always: its centre columns are X for step 5)
  for (uint32_t e = tid; e < Tf * C; e += HPSS_THREADS) {
    const uint32_t f = e / C, c = e - f * C;
    sS[e] = hpss_key(in[(size_t)(f0 + f) * D + hpss_reflect((int32_t)(j0 + c) - (int32_t)hp, D)]);
  }
  __syncthreads();
  // 4. select along bins
  if (want_p)
    for (uint32_t e = tid; e < Tf * C; e += HPSS_THREADS) {
      const uint32_t f = e / C, c = e - f * C;
      hpss_select(sS + f * C, 1u, c, Td, kp, sMp + f * HPSS_TD, nanP + f * HPSS_TD, 1u);
    }
  __syncthreads();

  // 5. mask and output
  float* out = A.out + sg.off * D;
  for (uint32_t e = tid; e < Tf * HPSS_TD; e += HPSS_THREADS) {
    const uint32_t f = e / HPSS_TD, j = e % HPSS_TD;
    if (j >= Td) continue;
    const float nan = __uint_as_float(0x7FC00000u);
    float y;
    if (median) {
      y = A.percussive ? (nanP[e] ? nan : hpss_unkey(sMp[e])) : (nanH[e] ? nan : hpss_unkey(sMh[e]));
    } else {
      const float H = nanH[e] ? nan : hpss_unkey(sMh[e]), P = nanP[e] ? nan : hpss_unkey(sMp[e]);
      const double m = A.percussive ? hpss_mask(A, P, H, A.margin_p) : hpss_mask(A, H, P, A.margin_h);
      y = A.output == VSYN_HPSS_OUT_MASK ? (float)m : (float)((double)hpss_unkey(sS[f * C + hp + j]) * m);
    }
    out[(size_t)(f0 + f) * D + j0 + j] = y;
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct HpssWs {  // the stage's buffers
  TableUpload tab;
  DevBuf<float> rows;  // the output of a call whose d_out is its d_in, and of the stage inside a host chain
};

// The checks of the spec that need no rows.
static inline int hpss_check(const vsyn_spectral_hpss* p, const char** err) {
  if (!p) return fail(err, VSYN_ERR_INVALID, "hpss spec is NULL");
  if (!(p->kh & 1u) || p->kh > HPSS_KMAX || !(p->kp & 1u) || p->kp > HPSS_KMAX)
    return fail(err, VSYN_ERR_INVALID, "hpss: kernel sizes must be odd and in [1, %u], got %u and %u", HPSS_KMAX, p->kh, p->kp);
  if (p->component > VSYN_HPSS_PERCUSSIVE) return fail(err, VSYN_ERR_INVALID, "hpss: unknown component %u", p->component);
  if (p->output > VSYN_HPSS_OUT_MEDIAN) return fail(err, VSYN_ERR_INVALID, "hpss: unknown output %u", p->output);
  if (!(p->power > 0.0)) return fail(err, VSYN_ERR_INVALID, "hpss: power must be > 0 (finite or +Inf)");
  if (!(std::isfinite(p->margin_h) && p->margin_h >= 1.0 && std::isfinite(p->margin_p) && p->margin_p >= 1.0))
    return fail(err, VSYN_ERR_INVALID, "hpss: margins must be finite and >= 1");
  return VSYN_OK;
}

// The checks of a call.
static inline int hpss_check_call(const vsyn_spectral_hpss* p, uint32_t D, uint32_t S, const uint64_t* seg_rows, const char** err) {
  if (int rc = hpss_check(p, err)) return rc;
  if (D < 1) return fail(err, VSYN_ERR_INVALID, "hpss: dim must be >= 1");
  if (D > HPSS_MAX_DIM) return fail(err, VSYN_ERR_INVALID, "hpss: dim too large");
  if (int rc = rows_check_segs(S, seg_rows, HPSS_MAX_DIM, err)) return rc;
  const uint64_t ntd = (D + HPSS_TD - 1u) / HPSS_TD;
  for (uint32_t g = 0; g < S; ++g)  // the tiles of a segment are one grid dimension
    if ((seg_rows[g] + HPSS_TF - 1u) / HPSS_TF * ntd > 0x7FFFFFFFull)
      return fail(err, VSYN_ERR_INVALID, "segment %u: too many rows", g);
  return VSYN_OK;
}

// The stage's kernel on stream s: d_in [rows][D] -> d_out [rows][D]. d_out must not overlap d_in (hpss_launch_any handles d_out =
// d_in). skip (may be NULL): a segment with skip[g] = 0 is neither read nor written (the spectral stage's rate of 0). Caller holds the
// handle's lock and has run hpss_check_call.
static inline int hpss_launch(HpssWs& ws, int device, const vsyn_spectral_hpss* p, uint32_t D, uint32_t S, const uint64_t* seg_rows, const uint32_t* skip,
                              const float* d_in, float* d_out, hipStream_t s, const char** err) {
  std::vector<uint8_t> tab(sizeof(HpssSeg) * (size_t)S);
  HpssSeg* seg = (HpssSeg*)tab.data();
  const uint64_t f_max = row_segs_fill(seg, S, seg_rows, skip, 1u).f_max;
  if (f_max == 0) return VSYN_OK;
  HIPCHK(hipSetDevice(device));
  if (int rc = ws.tab.upload(tab, s, err)) return rc;
  HpssCtx A;
  A.seg = (const HpssSeg*)ws.tab.dev.p;
  A.in = d_in;
  A.out = d_out;
  A.D = D;
  A.ntd = (D + HPSS_TD - 1u) / HPSS_TD;
  A.kh = p->kh;
  A.kp = p->kp;
  A.percussive = p->component == VSYN_HPSS_PERCUSSIVE;
  A.output = p->output;
  A.mode = std::isinf(p->power) ? 0u : p->power == 1.0 ? 1u : p->power == 2.0 ? 2u : 3u;
  A.split = p->margin_h == 1.0 && p->margin_p == 1.0;
  A.power = p->power;
  A.margin_h = p->margin_h;
  A.margin_p = p->margin_p;
  const dim3 grid((uint32_t)((f_max + HPSS_TF - 1u) / HPSS_TF * A.ntd), S);
  VSYN_LAUNCH(vsyn_hpss_kernel, grid, dim3(HPSS_THREADS), 0, s, A);
  return VSYN_OK;
}

// hpss_launch for any d_out: with d_out = d_in through the workspace and one device copy back on the same stream.
static inline int hpss_launch_any(HpssWs& ws, int device, const vsyn_spectral_hpss* p, uint32_t D, uint32_t S, const uint64_t* seg_rows,
                                  const float* d_in, float* d_out, hipStream_t s, const char** err) {
  if (d_out != d_in) return hpss_launch(ws, device, p, D, S, seg_rows, nullptr, d_in, d_out, s, err);
  const uint64_t total = seg_total(S, seg_rows);
  HIPCHK(hipSetDevice(device));
  HIPCHK(ws.rows.ensure(total * D));
  if (int rc = hpss_launch(ws, device, p, D, S, seg_rows, nullptr, d_in, ws.rows.p, s, err)) return rc;
  HIPCHK(hipMemcpyAsync(d_out, ws.rows.p, sizeof(float) * total * D, hipMemcpyDeviceToDevice, s));
  return VSYN_OK;
}
