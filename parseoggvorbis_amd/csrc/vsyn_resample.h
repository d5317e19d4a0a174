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
//                              taps are +0 and add nothing to finite input (under an Inf or NaN sample they give NaN, which is why
//                              the header states the sum over K4), and both variants give the same bits. up == down copies.
// Nothing here reads or writes stream state, the overlap carry or any synthesis buffer; the PCM is only read.
#pragma once
#include "vsyn_device.h"
#include "vsyn_host.h"
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

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct ResampleWs {  // the stage's buffers: its own; the PCM is only read
  TableUpload tab;
  bool lds_set = false;                // vsyn_rs_kernel<true>'s dynamic-LDS limit is raised on this handle's device
  DevBuf<uint32_t> inF, outF;
  DevBuf<uint64_t> off;
  DevBuf<float> pcm;                   // host forms: the resampled PCM
  DevBuf<int16_t> s16;                 // vsyn_pcm_resample_host, VSYN_PCM_S16
};

// vsyn_rs_kernel<true> holds one pair's table and one tile's input span in LDS. 80 KiB keeps two of its workgroups on a CU
// (160 KiB) at worst and takes every pair among 8, 11.025, 16, 22.05, 24, 32, 44.1 and 48 kHz but 11.025 <-> 32 kHz (115 / 122
// KiB); 44.1 -> 16 kHz needs 46 KiB. Bigger tables (11.025 <-> 32 kHz; 44056 -> 16000 = 2000 / 5507, 448 KiB) use
// vsyn_rs_kernel<false>.
static const uint32_t RS_LDS_BUDGET = 80u * 1024u;

// The reduced ratio of a pair; false for a pair the contract refuses (a rate of 0, or M above VSYN_RESAMPLE_MAX_M).
static inline bool rs_ratio(uint32_t r_in, uint32_t r_out, uint32_t* up, uint32_t* down) {
  if (!r_in || !r_out) return false;
  const uint32_t g = std::gcd(r_in, r_out);
  *up = r_out / g;
  *down = r_in / g;
  return std::max(*up, *down) <= VSYN_RESAMPLE_MAX_M;
}

static inline double rs_i0(double x) {  // modified Bessel function of the first kind, order 0: sum_k ((x/2)^k / k!)^2
  const double q = 0.25 * x * x;
  double s = 1.0, t = 1.0;
  for (int k = 1; k < 500; ++k) {
    t *= q / ((double)k * (double)k);
    s += t;
    if (t < 1e-17 * s) break;
  }
  return s;
}

// h[0 .. N) of the header's step 2, in double.
static inline void rs_taps(uint32_t up, uint32_t down, std::vector<double>& h) {
  const uint32_t M = std::max(up, down), H = 10u * M, N = 2u * H + 1u;
  h.assign(N, 0.0);
  const double i0b = rs_i0(5.0);
  double S = 0.0;
  for (uint32_t n = 0; n < N; ++n) {
    const double m = (double)n - (double)H, xs = M_PI * m / (double)M, r = 2.0 * n / (double)(N - 1u) - 1.0;
    const double sinc = m == 0.0 ? 1.0 : sin(xs) / xs;
    h[n] = rs_i0(5.0 * sqrt(std::max(0.0, 1.0 - r * r))) / i0b * sinc;
    S += h[n];
  }
  for (uint32_t n = 0; n < N; ++n) h[n] = up * h[n] / S;
}

struct RsPlan {
  std::vector<uint8_t> tab;
  uint64_t chunks[2] = {0, 0};  // grid bounds of vsyn_rs_kernel<true> / <false>
  uint32_t lds_bytes = 0;       // dynamic LDS of vsyn_rs_kernel<true>
};

// RsHeader, RsPair per distinct pair, seg_pair[S], the polyphase tables. rates[g] = 0 skips g; every other pair is valid (checked
// by the caller). plane bounds every segment's input frames.
static inline void rs_build_table(uint32_t S, const uint32_t* rates, uint32_t out_rate, uint32_t C, uint64_t plane, RsPlan& plan) {
  std::vector<uint32_t> seg_pair(S, RS_SKIP), keys;
  std::vector<RsPair> pairs;
  uint64_t taps = 0;
  const uint64_t T_max = std::min<uint64_t>(plane, 0xFFFFFFFFull);
  for (uint32_t g = 0; g < S; ++g) {
    if (!rates[g]) continue;
    auto it = std::find(keys.begin(), keys.end(), rates[g]);
    seg_pair[g] = (uint32_t)(it - keys.begin());
    if (it == keys.end()) {
      keys.push_back(rates[g]);
      RsPair p = {};
      rs_ratio(rates[g], out_rate, &p.up, &p.down);
      p.lds = 1;
      if (p.up != p.down) {
        const uint32_t M = std::max(p.up, p.down), N = 20u * M + 1u, K = (N + p.up - 1u) / p.up;
        p.h = 10u * M;
        p.k4 = (K + 3u) & ~3u;
        p.span4 = rs_span4(p.up, p.down, p.k4);
        p.tab = taps;
        taps += (uint64_t)p.up * p.k4;
        const uint64_t lds = 4ull * ((uint64_t)p.up * p.k4 + 4ull * p.span4);
        p.lds = lds <= RS_LDS_BUDGET;
        if (p.lds) plan.lds_bytes = std::max(plan.lds_bytes, (uint32_t)lds);
      }
      pairs.push_back(p);
    }
    const RsPair& p = pairs[seg_pair[g]];
    plan.chunks[p.lds ? 0 : 1] += (uint64_t)C * ((rs_num_frames(T_max, p.up, p.down) + RS_CHUNK - 1u) / RS_CHUNK);
  }
  auto al = [](size_t v) { return (v + 15) & ~(size_t)15; };
  RsHeader hd = {(uint32_t)pairs.size(), S, 0, 0};
  const size_t off_pairs = sizeof(RsHeader);
  hd.off_seg = (uint32_t)al(off_pairs + sizeof(RsPair) * pairs.size());
  const size_t off_taps = al(hd.off_seg + 4ull * S);
  for (RsPair& p : pairs) p.tab += off_taps / 4u;
  plan.tab.assign(off_taps + 4ull * taps + 16, 0);
  uint8_t* o = plan.tab.data();
  memcpy(o, &hd, sizeof(hd));
  if (!pairs.empty()) memcpy(o + off_pairs, pairs.data(), sizeof(RsPair) * pairs.size());
  if (S) memcpy(o + hd.off_seg, seg_pair.data(), 4ull * S);
  std::vector<double> h;
  for (const RsPair& p : pairs) {
    if (p.up == p.down) continue;
    rs_taps(p.up, p.down, h);
    float* P = (float*)o + p.tab;
    for (uint32_t phi = 0; phi < p.up; ++phi)
      for (uint32_t t = 0; t < p.k4; ++t) {
        const uint64_t n = phi + (uint64_t)t * p.up;
        P[(size_t)phi * p.k4 + t] = n < h.size() ? (float)h[n] : 0.0f;
      }
  }
}

// The checks of every segment's pair (0 = skipped segment).
static inline int rs_check(uint32_t S, const uint32_t* rates, uint32_t out_rate, const char** err) {
  if (!out_rate) return fail(err, VSYN_ERR_INVALID, "out_rate must be >= 1");
  if (S && !rates) return fail(err, VSYN_ERR_INVALID, "in_rates is NULL");
  for (uint32_t g = 0; g < S; ++g) {
    uint32_t up, down;
    if (rates[g] && !rs_ratio(rates[g], out_rate, &up, &down))
      return fail(err, VSYN_ERR_INVALID, "segment %u: %u -> %u Hz reduces to %u / %u, above the limit max(up, down) <= %u", g, rates[g],
                  out_rate, up, down, VSYN_RESAMPLE_MAX_M);
  }
  return VSYN_OK;
}

// Offsets and resample kernels on stream s; frames from d_frames, else from si; the frames written go to d_out_frames (NULL:
// ws.outF). Caller holds the handle's lock and has run rs_check, and out_plane holds every segment's T_out.
static inline int rs_launch(ResampleWs& ws, int device, uint32_t S, const uint32_t* rates, uint32_t out_rate, const float* d_pcm, uint64_t plane, uint32_t C,
                     const uint32_t* d_frames, const SegInfo* si, float* d_out, uint64_t out_plane, uint32_t* d_out_frames, hipStream_t s,
                     const char** err) {
  RsPlan plan;
  rs_build_table(S, rates, out_rate, C, plane, plan);
  if (plan.chunks[0] > 0x7FFFFFFFull || plan.chunks[1] > 0x7FFFFFFFull) return fail(err, VSYN_ERR_INVALID, "too much output for one call");
  HIPCHK(hipSetDevice(device));
  if (!ws.lds_set) {
    HIPCHK(hipFuncSetAttribute((const void*)vsyn_rs_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RS_LDS_BUDGET));
    ws.lds_set = true;
  }
  const std::vector<uint8_t>& tab = plan.tab;
  HIPCHK(ws.inF.ensure(S));
  HIPCHK(ws.outF.ensure(S));
  HIPCHK(ws.off.ensure(2ull * S + 2));
  if (int rc = ws.tab.upload(tab, s, err)) return rc;
  RsCtx A;
  A.tab = ws.tab.dev.p;
  A.pcm = d_pcm;
  A.plane = plane;
  A.C = C;
  A.S = S;
  A.frames = d_frames;
  A.si = si;
  A.out = d_out;
  A.out_plane = out_plane;
  A.in_frames = ws.inF.p;
  A.out_frames = d_out_frames ? d_out_frames : ws.outF.p;
  A.off = ws.off.p;
  VSYN_LAUNCH(vsyn_rs_offsets_kernel, dim3(1), dim3(RS_THREADS), 0, s, A);
  if (plan.chunks[0]) {
    VSYN_LAUNCH(vsyn_rs_kernel<true>, dim3((uint32_t)plan.chunks[0]), dim3(RS_THREADS), plan.lds_bytes, s, A);
  }
  if (plan.chunks[1]) {
    VSYN_LAUNCH(vsyn_rs_kernel<false>, dim3((uint32_t)plan.chunks[1]), dim3(RS_THREADS), 0, s, A);
  }
  return VSYN_OK;
}
