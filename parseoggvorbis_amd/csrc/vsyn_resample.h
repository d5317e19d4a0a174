// vsyn_resample.h — polyphase resampling (scipy.signal.resample_poly) of planar float32 PCM already on the device.
// Semantics: include/vorbis_synth_hip.h, "resampling".
//
// Two kernels on one stream (the polyphase tables P[phi][t] are built on the host in double, vorbis_synth_hip.hip rs_build_table):
//   1. vsyn_rs_offsets_kernel  one workgroup: per segment its input frames T (the caller's d_frames, or the last submit's SegInfo,
//                              clamped to the plane), T_out = ceil(T up / down), and two exclusive scans of its work chunks
//                              (channels x ceil(T_out / RS_CHUNK)), one per kernel variant below.
//   2. vsyn_rs_kernel<LDS>     one workgroup per chunk of RS_CHUNK outputs of one (segment, channel), in tiles of RS_TILE: output
//                              j = j0 + r * RS_THREADS + tid (r < RS_PER_THREAD), so a wave's stores are contiguous and its input
//                              reads spread over the banks. LDS = true: the pair's table P (rows zero-padded to K4, a multiple of
//                              4, read as float4) is staged once per workgroup, and per tile the contiguous input span the tile
//                              needs, with 16-byte loads and zeros outside [0, T). LDS = false (table + span above RS_LDS_BUDGET,
//                              e.g. 44056 -> 16000 = 2000 / 5507, a 448 KiB table): P and x come from global memory (L2).
//                              Both compute y[j] = sum_{t < K4} P[phi][t] x[i0 - t] as one fmaf chain, t ascending: the padded
//                              taps are +0 and add nothing, and both variants give the same bits. up == down copies.
// Nothing here reads or writes stream state, the overlap carry or any synthesis buffer; the PCM is only read.
#pragma once
#include "vsyn_device.h"
#include "vsyn_pcm.h"

#define RS_THREADS 256
#define RS_PER_THREAD 4
#define RS_TILE (RS_THREADS * RS_PER_THREAD)  // outputs per tile
#define RS_TILES 8                            // tiles per workgroup: the table is staged once for all of them
#define RS_CHUNK (RS_TILE * RS_TILES)         // outputs per workgroup
#define RS_SKIP 0xFFFFFFFFu                   // seg_pair entry of a segment without output (rate 0)

struct RsPair {      // one distinct (r_in, r_out) pair
  uint32_t up, down; // reduced ratio
  uint32_t k4, h;    // taps per phase, padded to a multiple of 4 (0 for up == down); H = 10 max(up, down)
  uint64_t tab;      // float index of P[up][k4] from the table's base (16-byte aligned)
  uint32_t lds;      // 1: vsyn_rs_kernel<true> (P and one tile's span fit RS_LDS_BUDGET), 0: vsyn_rs_kernel<false>
  uint32_t span4;    // float4s of one tile's input span (LDS variant)
};
struct RsHeader {
  uint32_t num_pairs, S, off_seg, pad;  // RsPair[num_pairs] follows; off_seg: byte offset of seg_pair[S] (uint32, RS_SKIP)
};

struct RsCtx {  // launch arguments
  const uint8_t* tab;
  const float* pcm;
  uint64_t plane;
  uint32_t C, S;
  const uint32_t* frames;  // input frames per segment (caller's), or
  const SegInfo* si;       // the last submit's SegInfo (total_emit)
  float* out;
  uint64_t out_plane;
  uint32_t* in_frames;     // [S] T
  uint32_t* out_frames;    // [S] T_out
  uint64_t* off;           // [2][S+1] chunk scans: [0] vsyn_rs_kernel<true>, [1] vsyn_rs_kernel<false>
};

__host__ __device__ __forceinline__ uint64_t rs_num_frames(uint64_t T, uint32_t up, uint32_t down) {
  return (T * up + down - 1u) / down;  // T < 2^32, up <= 65536: no overflow
}
// One tile's input span in floats, bounded over every tile start: i0 moves by at most ceil((RS_TILE - 1) down / up) over the
// tile, plus K4 - 1 taps behind the first output, plus up to 3 for rounding the span's start down to a multiple of 4.
__host__ __device__ __forceinline__ uint32_t rs_span4(uint32_t up, uint32_t down, uint32_t k4) {
  const uint64_t d = ((uint64_t)(RS_TILE - 1) * down + up - 1u) / up;
  return (uint32_t)((d + k4 + 3u) / 4u + 1u);
}

__device__ __forceinline__ const RsPair* rs_pairs(const uint8_t* t) { return (const RsPair*)(t + sizeof(RsHeader)); }
__device__ __forceinline__ const uint32_t* rs_seg_pair(const uint8_t* t) { return (const uint32_t*)(t + ((const RsHeader*)t)->off_seg); }

__global__ void __launch_bounds__(RS_THREADS) vsyn_rs_offsets_kernel(const RsCtx A) {
  const RsPair* P = rs_pairs(A.tab);
  const uint32_t* sp = rs_seg_pair(A.tab);
  wg_exclusive_scan<RS_THREADS, 2>(A.S, A.off, [&](uint32_t g, uint64_t* v) {
    const uint64_t T = min((uint64_t)(A.frames ? A.frames[g] : A.si[g].total_emit), A.plane);
    uint64_t To = 0;
    if (sp[g] != RS_SKIP) {
      const RsPair p = P[sp[g]];
      To = rs_num_frames(T, p.up, p.down);
      const uint64_t n = (uint64_t)A.C * ((To + RS_CHUNK - 1u) / RS_CHUNK);
      if (p.lds) v[0] = n;
      else v[1] = n;
    }
    A.in_frames[g] = (uint32_t)T;
    A.out_frames[g] = (uint32_t)To;  // < 2^32: checked against out_plane on the host
  });
}

template <bool LDS>
__global__ void __launch_bounds__(RS_THREADS) vsyn_rs_kernel(const RsCtx A) {
  extern __shared__ float4 rs_lds[];
  const uint64_t* off = A.off + (LDS ? 0u : A.S + 1u);
  const uint64_t b = blockIdx.x;
  if (b >= off[A.S]) return;  // the grid is a bound; the scan has the real count
  uint32_t lo = 0, hi = A.S;  // off[lo] <= b < off[hi]: the segment is the last g with off[g] <= b
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= b) lo = mid;
    else hi = mid;
  }
  const uint32_t g = lo, tid = threadIdx.x;
  const RsPair pr = rs_pairs(A.tab)[rs_seg_pair(A.tab)[g]];
  const uint64_t T = A.in_frames[g], To = A.out_frames[g];
  const uint64_t nch = (To + RS_CHUNK - 1u) / RS_CHUNK, local = b - off[g];
  const uint32_t c = (uint32_t)(local / nch);
  const uint64_t jc = (local - (uint64_t)c * nch) * RS_CHUNK, jend = min(jc + RS_CHUNK, To);
  const float* x = A.pcm + ((size_t)g * A.C + c) * A.plane;
  float* y = A.out + ((size_t)g * A.C + c) * A.out_plane;
  if (pr.up == pr.down) {  // ratio 1: the input, bit for bit
    for (uint64_t j = jc + tid; j < jend; j += RS_THREADS) y[j] = x[j];
    return;
  }
  const uint32_t up = pr.up, down = pr.down, k4 = pr.k4, q4 = pr.k4 / 4u;
  const float4* gP = (const float4*)((const float*)A.tab + pr.tab);
  const float4* sP = rs_lds;
  float* sX = (float*)(rs_lds + (size_t)up * q4);
  if (LDS) {
    for (uint32_t q = tid; q < up * q4; q += RS_THREADS) rs_lds[q] = gP[q];
  }
  const bool vec = (((uintptr_t)x) & 15u) == 0;
  for (uint64_t j0 = jc; j0 < jend; j0 += RS_TILE) {
    // c = j down + H = c0 + k down with k = j - j0 < RS_TILE: one 64-bit division per tile, 32-bit ones per output
    const uint64_t c0 = j0 * down + pr.h;
    const uint64_t qb = c0 / up;
    const uint32_t rb = (uint32_t)(c0 - qb * up);
    const uint32_t kn = (uint32_t)min((uint64_t)RS_TILE, jend - j0);
    int64_t a0 = 0;  // LDS: input index of sX[0], a multiple of 4
    if (LDS) {
      a0 = ((int64_t)qb - (int64_t)(k4 - 1u)) & ~(int64_t)3;
      const uint64_t kl = kn - 1u;
      const int64_t e = (int64_t)(qb + (rb + kl * down) / up);  // the last input the tile reads
      const uint32_t m4 = min((uint32_t)((e - a0) / 4 + 1), pr.span4);
      __syncthreads();  // the previous tile's reads of the span are done
      float4* sX4 = (float4*)sX;
      for (uint32_t q = tid; q < m4; q += RS_THREADS) {
        const int64_t i = a0 + 4 * (int64_t)q;
        float4 v;
        if (vec && i >= 0 && i + 3 < (int64_t)T) {
          v = *(const float4*)(x + i);
        } else {
          v.x = (i >= 0 && i < (int64_t)T) ? x[i] : 0.f;
          v.y = (i + 1 >= 0 && i + 1 < (int64_t)T) ? x[i + 1] : 0.f;
          v.z = (i + 2 >= 0 && i + 2 < (int64_t)T) ? x[i + 2] : 0.f;
          v.w = (i + 3 >= 0 && i + 3 < (int64_t)T) ? x[i + 3] : 0.f;
        }
        sX4[q] = v;
      }
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < RS_PER_THREAD; ++r) {
      const uint32_t k = (uint32_t)r * RS_THREADS + tid;
      if (k >= kn) continue;
      const uint32_t cr = rb + k * down;  // < up + RS_TILE * 65536 < 2^27
      const uint32_t phi = cr % up;
      const uint64_t i0 = qb + cr / up;
      float acc = 0.f;
      if (LDS) {
        const float4* p = sP + (size_t)phi * q4;
        const float* xb = sX + (uint32_t)((int64_t)i0 - a0);
        for (uint32_t t = 0; t < q4; ++t) {
          const float4 w = p[t];
          const float* xt = xb - 4u * t;
          acc = fmaf(w.x, xt[0], acc);
          acc = fmaf(w.y, xt[-1], acc);
          acc = fmaf(w.z, xt[-2], acc);
          acc = fmaf(w.w, xt[-3], acc);
        }
      } else {
        const float4* p = gP + (size_t)phi * q4;
        if (i0 >= k4 - 1u && i0 < T) {  // every tap inside [0, T)
          const float* xb = x + i0;
          for (uint32_t t = 0; t < q4; ++t) {
            const float4 w = p[t];
            const float* xt = xb - 4u * t;
            acc = fmaf(w.x, xt[0], acc);
            acc = fmaf(w.y, xt[-1], acc);
            acc = fmaf(w.z, xt[-2], acc);
            acc = fmaf(w.w, xt[-3], acc);
          }
        } else {
          for (uint32_t t = 0; t < q4; ++t) {
            const float4 w = p[t];
            const int64_t i = (int64_t)i0 - 4 * (int64_t)t;
            acc = fmaf(w.x, (i >= 0 && i < (int64_t)T) ? x[i] : 0.f, acc);
            acc = fmaf(w.y, (i - 1 >= 0 && i - 1 < (int64_t)T) ? x[i - 1] : 0.f, acc);
            acc = fmaf(w.z, (i - 2 >= 0 && i - 2 < (int64_t)T) ? x[i - 2] : 0.f, acc);
            acc = fmaf(w.w, (i - 3 >= 0 && i - 3 < (int64_t)T) ? x[i - 3] : 0.f, acc);
          }
        }
      }
      y[j0 + k] = acc;
    }
  }
}

// Planar float32 with frames[S] -> interleaved int16 [S][out_stride][C] (pcm_s16, vsyn_pcm.h), zeros past a segment's frames.
__global__ void __launch_bounds__(256) vsyn_rs_s16_kernel(const float* __restrict__ pcm, uint64_t plane, uint32_t C,
                                                          const uint32_t* __restrict__ frames, int16_t* __restrict__ out, uint64_t out_stride) {
  const uint32_t g = blockIdx.y;
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= out_stride) return;
  const bool in = t < frames[g];
  for (uint32_t c = 0; c < C; ++c)
    out[((size_t)g * out_stride + t) * C + c] = in ? (int16_t)pcm_s16(pcm[((size_t)g * C + c) * plane + t]) : (int16_t)0;
}
