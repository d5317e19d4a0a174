// vsyn_loudness.h — integrated loudness (ITU-R BS.1770 K-weighting, 400 ms blocks, two gates) of planar float32 PCM already on the
// device, and the gain to a target loudness. Semantics: include/vorbis_synth_hip.h, "loudness".
//
// The K-weighting filter is a fourth-order IIR along time with one column per channel: the first stage here whose recurrence has to
// be cut along time. Its state is v = (s1, s2, t1, t2), the two delay elements of each direct-form-II-transposed biquad, and one
// sample takes v to A v + B x with a 4x4 matrix A. The scan's decomposition is a function of the segment's own samples counted from
// its first one: chunks of LOUD_SUB samples, one per lane, LOUD_LANES chunks to a tile, whatever the grid and the segment's place in
// the batch. The host uploads one LoudSeg per segment: its frames, rate, whole hops, offsets into the work arrays, the ten
// coefficients and the powers A^(LOUD_SUB 2^k), k = 0 .. 8, all formed in double on the host. Six launches on one stream:
//   1. vsyn_loud_part_kernel   per (tile but the last, channel, segment): the tile into LDS (rows padded to LOUD_SUB + 1 floats);
//                              every lane runs the cascade from zero over its chunk; the lanes' final states are combined by a
//                              Kogge-Stone scan over the lanes, level k with A^(LOUD_SUB 2^k): w[i] = w[i] + M_k w[i - 2^k]. Lane
//                              255 holds the tile's zero-state response at its end -> part[tile].
//   2. vsyn_loud_carry_kernel  per (channel, segment), tiles ascending: c[0] = 0, c[k+1] = A^(LOUD_TILE) c[k] + part[k].
//   3. vsyn_loud_apply_kernel  per (tile, channel, segment): the tile again; lane 0 starts from c[k], the others from zero; the same
//                              step function and the same scan give every lane the state in front of its chunk; from that the
//                              chunk's K-weighted samples, their squares into two sub-sums (in front of and behind the one hop
//                              boundary a chunk can cross: a hop has at least 400 samples), and the samples themselves as float64
//                              through LDS when asked for.
//   4. vsyn_loud_hops_kernel   one wave per (hop, channel, segment): its chunks' sub-sums, lane l takes chunks l, l + 64, ..., then
//                              a butterfly. The pseudo-hop behind the last whole one exists for the finiteness check alone.
//   5. vsyn_loud_gate_kernel   one workgroup per segment: block means from the hop sums, the absolute gate, the relative gate,
//                              both means (thread t adds blocks t, t + 256, ...; then a fixed LDS tree), the record.
//   6. vsyn_loud_scale_kernel  y = x * g in float32 (zeros for a refused segment), only when a scaled plane is asked for.
// No atomics, nothing to clear in front of the stage, float64 state and sums in a fixed order: the same PCM gives the same bits
// alone and anywhere in a batch. Nothing here reads or writes stream state, the overlap carry or any synthesis buffer.
#pragma once
#include "vsyn_device.h"
#include "vsyn_host.h"
#include "vsyn_wave.h"

#define LOUD_LANES 256u
#define LOUD_SUB 32u                       // samples per lane chunk
#define LOUD_TILE (LOUD_LANES * LOUD_SUB)  // samples per workgroup
#define LOUD_ROW (LOUD_SUB + 1u)           // padded LDS row of a chunk, floats
#define LOUD_LEVELS 8u                     // log2(LOUD_LANES): matrices 0 .. 7 serve the scan, matrix 8 is A^(LOUD_TILE)
#define LOUD_YGRP 16u                      // K-weighted samples per lane staged in LDS at a time
#define LOUD_MIN_RATE 4000u

struct LoudSeg {
  uint64_t T;          // frames measured (0: the segment runs nothing)
  uint64_t tile_off;   // first tile of the segment in part / carry (per channel: times Cs); times LOUD_LANES its first chunk in sub
  uint64_t hop_off;    // first hop sum of the segment (per channel: times Cs); Nh + 1 per channel
  uint64_t z_off;      // first block of the segment in the z series
  uint64_t Nh;         // whole hops
  uint64_t frames;     // the segment's frames whatever its rate: what the scale kernel writes (zeros for a refused segment)
  uint32_t fs, tiles;  // rate (0: refused or skipped), ceil(T / LOUD_TILE)
  double coef[10];     // b0 b1 b2 a1 a2 of the shelf, c0 c1 c2 d1 d2 of the high pass
  double M[LOUD_LEVELS + 1u][16];  // A^(LOUD_SUB 2^k), row-major
};

struct LoudCtx {  // launch arguments
  const LoudSeg* seg;
  const float* pcm;  // [S][C][plane]
  uint64_t plane;
  uint32_t C, Cs, mono, S;  // Cs: channels of the measured signal (C, or 1 for the downmix)
  double* part;             // [tiles][Cs][4]
  double* carry;            // [tiles][Cs][4]
  double* sub;              // per segment [Cs][2][tiles * LOUD_LANES]: a chunk's sub-sum in front of and behind its hop boundary
  double* hops;             // per segment [Cs][Nh + 1]
  vsyn_loudness_record* rec;  // [S]
  double* z;                  // block means back to back, or NULL
  double* weighted;           // [S][Cs][wplane] K-weighted samples, or NULL
  uint64_t wplane;
  float* scaled;  // [S][Cs][splane], or NULL
  uint64_t splane;
  double z_abs, z_target;  // 10^((-70 + 0.691) / 10); 10^((L_t + 0.691) / 10), or 0 without a target
};

// Sample t of channel c of the measured signal of one segment (x = its first plane).
__device__ __forceinline__ float loud_sample(const LoudCtx& A, const float* x, uint32_t c, float inv_c, uint64_t t) {
  return A.mono ? pcm_downmix(x, A.plane, A.C, inv_c, t) : x[(size_t)c * A.plane + t];
}

// One sample through the cascade, each biquad in direct form II transposed with scipy.signal.lfilter's operations in its order.
// Every kernel that filters goes through this one function, so parts and values round alike. Returns the K-weighted sample.
__device__ __forceinline__ double loud_step(double v[4], const double* k, double x) {
  const double y1 = k[0] * x + v[0];
  v[0] = (v[1] + k[1] * x) - k[3] * y1;
  v[1] = k[2] * x - k[4] * y1;
  const double y = k[5] * y1 + v[2];
  v[2] = (v[3] + k[6] * y1) - k[8] * y;
  v[3] = k[7] * y1 - k[9] * y;
  return y;
}

// p + M q, each row ((m0 q0 + m1 q1) + m2 q2) + m3 q3 and then the sum with p.
__device__ __forceinline__ void loud_matvec_add(double w[4], const double* M, const double q[4], const double p[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) w[r] = p[r] + (((M[4 * r] * q[0] + M[4 * r + 1] * q[1]) + M[4 * r + 2] * q[2]) + M[4 * r + 3] * q[3]);
}

// The tile's samples into LDS rows of LOUD_ROW floats, zeros past T: thread t takes samples t, t + 256, ... (a wave's loads
// contiguous), or with 16-byte loads where the channel's plane allows.
__device__ __forceinline__ void loud_load_tile(const LoudCtx& A, const float* x, uint32_t c, uint64_t tile0, uint64_t T, float* s_x) {
  const uint32_t tid = threadIdx.x;
  const float inv_c = 1.0f / (float)A.C;
  const float* xc = x + (size_t)c * A.plane + tile0;
  // (the downmix reads every plane at the same offset: they share channel 0's alignment when the plane stride is a multiple of 4)
  const bool wide = tile0 + LOUD_TILE <= T && (A.mono ? ((((uintptr_t)(x + tile0)) & 15u) == 0 && (A.plane & 3u) == 0) : (((uintptr_t)xc) & 15u) == 0);
  if (wide) {
#pragma unroll
    for (uint32_t r = 0; r < LOUD_SUB / 4u; ++r) {
      const uint32_t n = 4u * (tid + LOUD_LANES * r);
      float4 q;
      if (A.mono) {  // pcm_downmix's operations in its order, four frames at a time
        q = *(const float4*)(x + tile0 + n);
        for (uint32_t ch = 1; ch < A.C; ++ch) {
          const float4 v = *(const float4*)(x + (size_t)ch * A.plane + tile0 + n);
          q.x += v.x;
          q.y += v.y;
          q.z += v.z;
          q.w += v.w;
        }
        q.x = q.x * inv_c;
        q.y = q.y * inv_c;
        q.z = q.z * inv_c;
        q.w = q.w * inv_c;
      } else {
        q = *(const float4*)(xc + n);
      }
      float* o = s_x + (n / LOUD_SUB) * LOUD_ROW + (n % LOUD_SUB);
      o[0] = q.x;
      o[1] = q.y;
      o[2] = q.z;
      o[3] = q.w;
    }
  } else {
    for (uint32_t r = 0; r < LOUD_SUB; ++r) {
      const uint32_t n = tid + LOUD_LANES * r;
      s_x[(n / LOUD_SUB) * LOUD_ROW + (n % LOUD_SUB)] = tile0 + n < T ? loud_sample(A, x, c, inv_c, tile0 + n) : 0.0f;
    }
  }
}

// Inclusive scan of the lanes' states over the workgroup: on return v of lane i is sum_j<=i (A^LOUD_SUB)^(i-j) v_j, every sum in the
// order the levels fix. s_p: [4][LOUD_LANES] doubles. Every thread of the workgroup calls it.
__device__ __forceinline__ void loud_scan(double v[4], const LoudSeg* sg, double* s_p) {
  const uint32_t i = threadIdx.x;
  for (uint32_t k = 0; k < LOUD_LEVELS; ++k) {
    const uint32_t d = 1u << k;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) s_p[r * LOUD_LANES + i] = v[r];
    __syncthreads();
    if (i >= d) {
      double q[4], w[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) q[r] = s_p[r * LOUD_LANES + i - d];
      loud_matvec_add(w, sg->M[k], q, v);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = w[r];
    }
  }
}

__global__ void __launch_bounds__(LOUD_LANES) vsyn_loud_part_kernel(const LoudCtx A) {
  __shared__ float s_x[LOUD_LANES * LOUD_ROW];
  __shared__ double s_p[4 * LOUD_LANES];
  const uint32_t g = blockIdx.z, c = blockIdx.y, k = blockIdx.x, i = threadIdx.x;
  const LoudSeg* sg = A.seg + g;
  if (k + 1u >= sg->tiles) return;  // (workgroup-uniform) the last tile hands nothing on: every tile here is full
  const float* x = A.pcm + (size_t)g * A.C * A.plane;
  loud_load_tile(A, x, c, (uint64_t)k * LOUD_TILE, sg->T, s_x);
  __syncthreads();
  double coef[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) coef[j] = sg->coef[j];
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  const float* row = s_x + i * LOUD_ROW;
#pragma unroll 8
  for (uint32_t t = 0; t < LOUD_SUB; ++t) (void)loud_step(v, coef, (double)row[t]);
  loud_scan(v, sg, s_p);
  if (i == LOUD_LANES - 1u) {
    double* p = A.part + ((sg->tile_off + k) * A.Cs + c) * 4u;
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r] = v[r];
  }
}

__global__ void __launch_bounds__(LOUD_LANES) vsyn_loud_carry_kernel(const LoudCtx A) {
  const uint32_t g = blockIdx.x, c = threadIdx.x;
  const LoudSeg* sg = A.seg + g;
  if (c >= A.Cs) return;
  double m[4] = {0.0, 0.0, 0.0, 0.0};
  for (uint32_t k = 0; k < sg->tiles; ++k) {
    const size_t e = ((sg->tile_off + k) * A.Cs + c) * 4u;
#pragma unroll
    for (int r = 0; r < 4; ++r) A.carry[e + r] = m[r];
    if (k + 1u >= sg->tiles) break;
    double p[4], w[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r] = A.part[e + r];
    loud_matvec_add(w, sg->M[LOUD_LEVELS], m, p);
#pragma unroll
    for (int r = 0; r < 4; ++r) m[r] = w[r];
  }
}

__global__ void __launch_bounds__(LOUD_LANES) vsyn_loud_apply_kernel(const LoudCtx A) {
  // the tile's samples; once every lane holds its chunk in registers, the staging area of the K-weighted samples
  __shared__ __attribute__((aligned(16))) unsigned char s_raw[LOUD_LANES * (LOUD_YGRP + 1u) * sizeof(double)];
  __shared__ double s_p[4 * LOUD_LANES];
  static_assert(sizeof(s_raw) >= LOUD_LANES * LOUD_ROW * sizeof(float), "the tile fits the staging area");
  float* s_x = (float*)s_raw;
  double* s_y = (double*)s_raw;
  const uint32_t g = blockIdx.z, c = blockIdx.y, k = blockIdx.x, i = threadIdx.x;
  const LoudSeg* sg = A.seg + g;
  if (k >= sg->tiles) return;  // (workgroup-uniform)
  const uint64_t T = sg->T, tile0 = (uint64_t)k * LOUD_TILE;
  const float* x = A.pcm + (size_t)g * A.C * A.plane;
  loud_load_tile(A, x, c, tile0, T, s_x);
  __syncthreads();
  double coef[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) coef[j] = sg->coef[j];
  float xs[LOUD_SUB];
#pragma unroll
  for (uint32_t t = 0; t < LOUD_SUB; ++t) xs[t] = s_x[i * LOUD_ROW + t];
  const size_t ce = ((sg->tile_off + k) * A.Cs + c) * 4u;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  if (i == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = A.carry[ce + r];
  }
  double v0[4] = {v[0], v[1], v[2], v[3]};
#pragma unroll
  for (uint32_t t = 0; t < LOUD_SUB; ++t) (void)loud_step(v, coef, (double)xs[t]);
  loud_scan(v, sg, s_p);
  // the state in front of lane i's chunk is what lane i - 1 holds behind its own
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) s_p[r * LOUD_LANES + i] = v[r];
  __syncthreads();
  if (i > 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v0[r] = s_p[r * LOUD_LANES + i - 1u];
  }
  // the chunk's place among the hops: hop(n) = (10 n + 9) / fs; a chunk crosses at most the boundary behind its first sample's hop
  const uint64_t n0 = tile0 + (uint64_t)i * LOUD_SUB;
  const uint32_t nvalid = n0 < T ? (uint32_t)min((uint64_t)LOUD_SUB, T - n0) : 0u;
  const uint64_t hop0 = (10u * n0 + 9u) / sg->fs, edge = ((hop0 + 1u) * sg->fs) / 10u;
  const uint32_t eb = (uint32_t)min((uint64_t)LOUD_SUB, edge - n0);
  double sa = 0.0, sb = 0.0;
  double* wp = A.weighted ? A.weighted + ((size_t)g * A.Cs + c) * A.wplane : nullptr;
  const uint64_t wT = min(T, A.wplane);
#pragma unroll
  for (uint32_t t0 = 0; t0 < LOUD_SUB; t0 += LOUD_YGRP) {
    double ys[LOUD_YGRP];
#pragma unroll
    for (uint32_t j = 0; j < LOUD_YGRP; ++j) {
      const uint32_t t = t0 + j;
      const double y = loud_step(v0, coef, (double)xs[t]);
      ys[j] = y;
      if (t < nvalid) {
        const double q = y * y;
        if (t < eb) sa += q;
        else sb += q;
      }
    }
    if (wp) {  // (workgroup-uniform) through LDS: 16 threads then write 128 contiguous bytes
      __syncthreads();
#pragma unroll
      for (uint32_t j = 0; j < LOUD_YGRP; ++j) s_y[i * (LOUD_YGRP + 1u) + j] = ys[j];
      __syncthreads();
#pragma unroll
      for (uint32_t r = 0; r < LOUD_YGRP; ++r) {
        const uint32_t e = i + LOUD_LANES * r, lane = e / LOUD_YGRP, j = e % LOUD_YGRP;
        const uint64_t n = tile0 + (uint64_t)lane * LOUD_SUB + t0 + j;
        if (n < wT) wp[n] = s_y[lane * (LOUD_YGRP + 1u) + j];
      }
    }
  }
  const uint64_t nsub = (uint64_t)sg->tiles * LOUD_LANES;  // the channel's chunks: first sub-sums [0, nsub), second [nsub, 2 nsub)
  double* sub = A.sub + (sg->tile_off * A.Cs + (uint64_t)c * sg->tiles) * LOUD_LANES * 2u + (uint64_t)k * LOUD_LANES + i;
  sub[0] = sa;
  sub[nsub] = sb;
}

__global__ void __launch_bounds__(256) vsyn_loud_hops_kernel(const LoudCtx A) {
  const uint32_t g = blockIdx.z, c = blockIdx.y, lane = threadIdx.x & 63u;
  const LoudSeg* sg = A.seg + g;
  const uint64_t i = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
  if (sg->fs == 0u || i > sg->Nh) return;  // (wave-uniform)
  const uint64_t lo = (i * sg->fs) / 10u, hi = i < sg->Nh ? ((i + 1u) * sg->fs) / 10u : sg->T;
  double s = 0.0;
  if (hi > lo) {
    const double* sub = A.sub + (sg->tile_off * A.Cs + (uint64_t)c * sg->tiles) * LOUD_LANES * 2u;
    const uint64_t l_lo = lo / LOUD_SUB, l_hi = (hi - 1u) / LOUD_SUB;
    const bool behind = (lo % LOUD_SUB) != 0u;  // the first chunk began in the hop before: its second sub-sum is this hop's
    const uint64_t nsub = (uint64_t)sg->tiles * LOUD_LANES;
    for (uint64_t l = l_lo + lane; l <= l_hi; l += 64u) s += sub[l == l_lo && behind ? nsub + l : l];
  }
  s = wave_sum(s);
  if (lane == 0) A.hops[sg->hop_off * A.Cs + (uint64_t)c * (sg->Nh + 1u) + i] = s;
}

// sum over the workgroup of (v, n) in a fixed tree; every thread returns the totals
__device__ __forceinline__ void loud_wg_sum(double* s_v, uint32_t* s_n, double& v, uint32_t& n) {
  const uint32_t t = threadIdx.x;
  __syncthreads();
  s_v[t] = v;
  s_n[t] = n;
  __syncthreads();
  for (uint32_t d = 128; d; d >>= 1) {
    if (t < d) {
      s_v[t] += s_v[t + d];
      s_n[t] += s_n[t + d];
    }
    __syncthreads();
  }
  v = s_v[0];
  n = s_n[0];
}

// the mean square of block j: its four hops' sums, each over the channels in ascending order, over its own sample count
__device__ __forceinline__ double loud_block(const LoudCtx& A, const LoudSeg* sg, uint64_t j) {
  const double* h = A.hops + sg->hop_off * A.Cs;
  double z = 0.0;
  for (uint32_t q = 0; q < 4u; ++q) {
    double s = h[j + q];
    for (uint32_t c = 1; c < A.Cs; ++c) s += h[(uint64_t)c * (sg->Nh + 1u) + j + q];
    z = q ? z + s : s;
  }
  const uint64_t n = ((j + 4u) * sg->fs) / 10u - (j * sg->fs) / 10u;
  return z / (double)n;
}

__global__ void __launch_bounds__(256) vsyn_loud_gate_kernel(const LoudCtx A) {
  __shared__ double s_v[256];
  __shared__ uint32_t s_n[256];
  const uint32_t g = blockIdx.x, t = threadIdx.x;
  const LoudSeg* sg = A.seg + g;
  vsyn_loudness_record r = {0.0, 0.0, 0u, 0u, 0u, 0.0f, VSYN_LOUD_OK, 0u};
  if (sg->fs == 0u) {
    r.status = VSYN_LOUD_RATE_REFUSED;
    if (t == 0) A.rec[g] = r;
    return;
  }
  const uint64_t Nh = sg->Nh, Nb = Nh >= 4u ? Nh - 3u : 0u;
  r.blocks = (uint32_t)Nb;
  // finiteness: every hop sum of every channel, the pseudo-hop behind the last whole hop included
  const double* h = A.hops + sg->hop_off * A.Cs;
  int bad = 0;
  for (uint64_t e = t; e < (Nh + 1u) * A.Cs; e += 256u) bad |= !isfinite(h[e]);
  bad = __syncthreads_or(bad);
  if (A.z)
    for (uint64_t j = t; j < Nb; j += 256u) A.z[sg->z_off + j] = loud_block(A, sg, j);
  if (bad || Nb == 0u) {
    r.status = bad ? VSYN_LOUD_NOT_FINITE : VSYN_LOUD_TOO_SHORT;
    if (t == 0) A.rec[g] = r;
    return;
  }
  double sum = 0.0;
  uint32_t n = 0u;
  for (uint64_t j = t; j < Nb; j += 256u) {
    const double z = loud_block(A, sg, j);
    if (z > A.z_abs) {
      sum += z;
      ++n;
    }
  }
  loud_wg_sum(s_v, s_n, sum, n);
  r.blocks_abs = n;
  if (n == 0u) {
    r.status = VSYN_LOUD_SILENT;
    if (t == 0) A.rec[g] = r;
    return;
  }
  r.zbar_a = sum / (double)n;
  const double rel = r.zbar_a / 10.0;
  sum = 0.0;
  n = 0u;
  for (uint64_t j = t; j < Nb; j += 256u) {
    const double z = loud_block(A, sg, j);
    if (z > A.z_abs && z > rel) {
      sum += z;
      ++n;
    }
  }
  loud_wg_sum(s_v, s_n, sum, n);
  r.blocks_rel = n;
  r.zbar = sum / (double)n;  // (the largest block is above a tenth of the mean: n >= 1)
  if (A.z_target != 0.0) r.gain = (float)sqrt(A.z_target / r.zbar);
  if (t == 0) A.rec[g] = r;
}

// y = x * g: a thread owns four frames of one channel; 16-byte loads and stores where both planes allow, else frame by frame
__global__ void __launch_bounds__(256) vsyn_loud_scale_kernel(const LoudCtx A) {
  const uint32_t g = blockIdx.z, c = blockIdx.y;
  const LoudSeg* sg = A.seg + g;
  const uint64_t T = min(sg->frames, A.splane), t0 = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 4u;
  if (t0 >= T) return;
  const vsyn_loudness_record r = A.rec[g];
  const bool refused = r.status != VSYN_LOUD_OK;
  const float gain = r.gain, inv_c = 1.0f / (float)A.C;
  const float* x = A.pcm + (size_t)g * A.C * A.plane;
  float* y = A.scaled + ((size_t)g * A.Cs + c) * A.splane + t0;
  const float* xc = x + (size_t)c * A.plane + t0;
  if (!A.mono && t0 + 3u < T && ((((uintptr_t)xc) | ((uintptr_t)y)) & 15u) == 0) {
    float4 q = *(const float4*)xc;
    q.x = refused ? 0.f : q.x * gain;
    q.y = refused ? 0.f : q.y * gain;
    q.z = refused ? 0.f : q.z * gain;
    q.w = refused ? 0.f : q.w * gain;
    *(float4*)y = q;
  } else {
    for (uint32_t j = 0; j < 4u && t0 + j < T; ++j) y[j] = refused ? 0.f : loud_sample(A, x, c, inv_c, t0 + j) * gain;
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct LoudWs {  // the stage's buffers
  TableUpload tab;
  DevBuf<double> part, carry, sub, hops, z;
  DevBuf<vsyn_loudness_record> rec;  // host forms
  DevBuf<float> pcm;                 // host forms: the scaled planes
  DevBuf<int16_t> s16;               // the chain's PCM form, VSYN_PCM_S16
};

#define LOUD_ABS_GATE_LUFS (-70.0)

// The ten coefficients of the K-weighting cascade at rate fs, in double: b0 b1 b2 a1 a2 of the shelf, then of the high pass.
static inline void loud_coefficients(uint32_t fs, double k[10]) {
  {
    const double G = 3.999843853973347, Q = 0.7071752369554196, fc = 1681.974450955533;
    const double K = tan(M_PI * fc / (double)fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    k[0] = (Vh + Vb * K / Q + K * K) / a0;
    k[1] = 2.0 * (K * K - Vh) / a0;
    k[2] = (Vh - Vb * K / Q + K * K) / a0;
    k[3] = 2.0 * (K * K - 1.0) / a0;
    k[4] = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double Q = 0.5003270373238773, fc = 38.13547087602444;
    const double K = tan(M_PI * fc / (double)fs), a0 = 1.0 + K / Q + K * K;
    k[5] = 1.0;
    k[6] = -2.0;
    k[7] = 1.0;
    k[8] = 2.0 * (K * K - 1.0) / a0;
    k[9] = (1.0 - K / Q + K * K) / a0;
  }
}

// Double-double arithmetic for the matrix powers: repeated squaring in plain double loses up to nine digits of A^n near the high
// pass's double pole, which then is the largest error of the whole stage. With 106 bits the table below is the exact
// power rounded once (tests/test_loudness_cpu.py holds it to that against integer arithmetic).
struct LoudDD {
  double hi, lo;
};
static inline LoudDD loud_dd_fast_sum(double a, double b) {  // |a| >= |b| or a = 0
  const double s = a + b;
  return LoudDD{s, b - (s - a)};
}
static inline LoudDD loud_dd_add(LoudDD x, LoudDD y) {
  const double s = x.hi + y.hi, bb = s - x.hi;
  const double e = ((x.hi - (s - bb)) + (y.hi - bb)) + (x.lo + y.lo);
  return loud_dd_fast_sum(s, e);
}
static inline LoudDD loud_dd_mul(LoudDD x, LoudDD y) {
  const double p = x.hi * y.hi;
  const double e = std::fma(x.hi, y.hi, -p) + (x.hi * y.lo + x.lo * y.hi);
  return loud_dd_fast_sum(p, e);
}
// c = a b, 4x4 row-major
static inline void loud_dd_matmul(LoudDD* c, const LoudDD* a, const LoudDD* b) {
  LoudDD r[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      LoudDD t = loud_dd_mul(a[4 * i], b[j]);
      for (int m = 1; m < 4; ++m) t = loud_dd_add(t, loud_dd_mul(a[4 * i + m], b[4 * m + j]));
      r[4 * i + j] = t;
    }
  memcpy(c, r, sizeof(r));
}

// The transition matrix of the cascade's state (s1, s2, t1, t2) and its powers A^(LOUD_SUB 2^k), k = 0 .. LOUD_LEVELS, by squaring.
// A's own elements are the double coefficients and the double differences below: that matrix is the filter the stage scans.
static inline void loud_powers(const double k[10], double M[LOUD_LEVELS + 1u][16]) {
  const double A[16] = {-k[3], 1.0, 0.0, 0.0,                 //
                        -k[4], 0.0, 0.0, 0.0,                 //
                        k[6] - k[8] * k[5], 0.0, -k[8], 1.0,  //
                        k[7] - k[9] * k[5], 0.0, -k[9], 0.0};
  LoudDD P[16];
  for (int e = 0; e < 16; ++e) P[e] = LoudDD{A[e], 0.0};
  for (uint32_t n = 1; n < LOUD_SUB; n <<= 1) loud_dd_matmul(P, P, P);
  for (uint32_t l = 0; l <= LOUD_LEVELS; ++l) {
    for (int e = 0; e < 16; ++e) M[l][e] = P[e].hi;
    loud_dd_matmul(P, P, P);
  }
}

static inline uint64_t loud_num_hops(uint32_t fs, uint64_t T) { return fs ? (uint64_t)(((unsigned __int128)T * 10u) / fs) : 0u; }
static inline uint64_t loud_num_blocks(uint32_t fs, uint64_t T) {
  const uint64_t nh = fs >= LOUD_MIN_RATE ? loud_num_hops(fs, T) : 0u;
  return nh >= 4u ? nh - 3u : 0u;
}

static inline int loud_check(const vsyn_loudness_spec* p, const char** err) {
  if (!p) return fail(err, VSYN_ERR_INVALID, "loudness spec is NULL");
  if (p->options & ~VSYN_LOUD_NORMALIZE) return fail(err, VSYN_ERR_INVALID, "unknown loudness options 0x%x", p->options);
  if (p->channel_mode != VSYN_LOUD_SUM && p->channel_mode != VSYN_LOUD_MONO)
    return fail(err, VSYN_ERR_INVALID, "unknown loudness channel mode %u", p->channel_mode);
  if ((p->options & VSYN_LOUD_NORMALIZE) && !(std::isfinite(p->target) && p->target >= -70.0 && p->target <= 0.0))
    return fail(err, VSYN_ERR_INVALID, "loudness target %g outside [-70, 0] LUFS", p->target);
  return VSYN_OK;
}

// The stage's kernels on stream s over planar PCM [S][C][plane]; rates and frames are the host's, a segment with a rate below
// LOUD_MIN_RATE runs nothing and is refused in its record. d_rec [S]; d_z (block means back to back), d_weighted [S][Cs][wplane]
// and d_scaled [S][Cs][splane] may be NULL. Caller holds the handle's lock and has run loud_check.
static inline int loud_launch(LoudWs& ws, int device, const vsyn_loudness_spec* p, uint32_t S, const uint32_t* rates, const uint64_t* frames,
                              const float* d_pcm, uint64_t plane, uint32_t C, vsyn_loudness_record* d_rec, double* d_z, double* d_weighted,
                              uint64_t wplane, float* d_scaled, uint64_t splane, hipStream_t s, const char** err) {
  if (S == 0) return VSYN_OK;
  if (S > 65535u) return fail(err, VSYN_ERR_INVALID, "too many segments (%u > 65535)", S);
  if (C == 0 || C > 255u) return fail(err, VSYN_ERR_INVALID, "channels outside [1, 255]");
  if ((uintptr_t)d_pcm & 3u) return fail(err, VSYN_ERR_INVALID, "PCM pointers must be 4-byte aligned");
  const uint32_t Cs = p->channel_mode == VSYN_LOUD_MONO ? 1u : C;
  std::vector<uint8_t> tab(sizeof(LoudSeg) * (size_t)S);
  LoudSeg* seg = (LoudSeg*)tab.data();
  uint64_t tiles = 0, hops = 0, blocks = 0, tiles_max = 0, nh_max = 0, f_max = 0;
  uint32_t last_fs = 0;
  double coef[10], M[LOUD_LEVELS + 1u][16];
  for (uint32_t g = 0; g < S; ++g) {
    LoudSeg& q = seg[g];
    memset(&q, 0, sizeof(q));
    q.tile_off = tiles;
    q.hop_off = hops;
    q.z_off = blocks;
    const uint32_t fs = rates[g] >= LOUD_MIN_RATE ? rates[g] : 0u;
    const uint64_t T = std::min(frames[g], plane);
    if (T > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "segment %u: too long", g);
    q.frames = T;
    f_max = std::max(f_max, T);
    if (!fs) {
      hops += 1u;
      continue;
    }
    if (fs != last_fs) {
      loud_coefficients(fs, coef);
      loud_powers(coef, M);
      last_fs = fs;
    }
    q.T = T;
    q.fs = fs;
    q.Nh = loud_num_hops(fs, T);
    q.tiles = (uint32_t)((T + LOUD_TILE - 1u) / LOUD_TILE);
    memcpy(q.coef, coef, sizeof(coef));
    memcpy(q.M, M, sizeof(M));
    tiles += q.tiles;
    hops += q.Nh + 1u;
    blocks += loud_num_blocks(fs, T);
    tiles_max = std::max<uint64_t>(tiles_max, q.tiles);
    nh_max = std::max(nh_max, q.Nh);
  }
  HIPCHK(hipSetDevice(device));
  HIPCHK(ws.part.ensure(tiles * Cs * 4u + 1u));
  HIPCHK(ws.carry.ensure(tiles * Cs * 4u + 1u));
  HIPCHK(ws.sub.ensure(tiles * Cs * LOUD_LANES * 2u + 2u));
  HIPCHK(ws.hops.ensure(hops * Cs + 1u));
  if (int rc = ws.tab.upload(tab, s, err)) return rc;
  LoudCtx A;
  A.seg = (const LoudSeg*)ws.tab.dev.p;
  A.pcm = d_pcm;
  A.plane = plane;
  A.C = C;
  A.Cs = Cs;
  A.mono = p->channel_mode == VSYN_LOUD_MONO && C > 1u ? 1u : 0u;  // (the downmix of one channel is that channel)
  A.S = S;
  A.part = ws.part.p;
  A.carry = ws.carry.p;
  A.sub = ws.sub.p;
  A.hops = ws.hops.p;
  A.rec = d_rec;
  A.z = d_z;
  A.weighted = d_weighted;
  A.wplane = wplane;
  A.scaled = d_scaled;
  A.splane = splane;
  A.z_abs = pow(10.0, (LOUD_ABS_GATE_LUFS + 0.691) / 10.0);
  A.z_target = (p->options & VSYN_LOUD_NORMALIZE) ? pow(10.0, (p->target + 0.691) / 10.0) : 0.0;
  if (tiles_max > 1u) {
    VSYN_LAUNCH(vsyn_loud_part_kernel, dim3((uint32_t)tiles_max - 1u, Cs, S), dim3(LOUD_LANES), 0, s, A);
  }
  if (tiles_max > 0u) {
    VSYN_LAUNCH(vsyn_loud_carry_kernel, dim3(S), dim3(LOUD_LANES), 0, s, A);
    VSYN_LAUNCH(vsyn_loud_apply_kernel, dim3((uint32_t)tiles_max, Cs, S), dim3(LOUD_LANES), 0, s, A);
  }
  VSYN_LAUNCH(vsyn_loud_hops_kernel, dim3((uint32_t)((nh_max + 1u + 3u) / 4u), Cs, S), dim3(256), 0, s, A);
  VSYN_LAUNCH(vsyn_loud_gate_kernel, dim3(S), dim3(256), 0, s, A);
  if (d_scaled && std::min(f_max, splane) > 0u) {
    const uint64_t gx = (std::min(f_max, splane) + 1023u) / 1024u;
    VSYN_LAUNCH(vsyn_loud_scale_kernel, dim3((uint32_t)gx, Cs, S), dim3(256), 0, s, A);
  }
  return VSYN_OK;
}
