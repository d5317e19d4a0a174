// vsyn_split.h — PCM splitting: the non-silent intervals of planar float32 PCM already on the device, and the mono signal with every
// silent stretch removed (librosa.effects.split on the mono signal, and the concatenation of its slices). Semantics:
// include/vorbis_synth_hip.h, "PCM splitting".
//
// Three kernels on one stream:
//   1. vsyn_trim_energy_kernel  (vsyn_trim.h, as it is) the float64 frame energies ms[f] and the not-finite flags, into this stage's
//                               own workspace.
//   2. vsyn_split_mark_kernel   one workgroup per segment, behind a finished ms array. R and the refusal come from the helpers the
//                               trim bounds kernel uses (trim_segment_max, trim_ref, trim_loud). Then one ordered scan over the
//                               positions f = 0 .. F (F itself stands for the silent frame behind the last one), SPLIT_CHUNK
//                               positions at a time: a thread owns SPLIT_PER consecutive positions, evaluates the predicate for
//                               f - 1 and each of them (no exchange for the edges), and counts its edges (loud(f) != loud(f - 1))
//                               and its non-silent frames; the two counts go through an inclusive wave scan (wave_scan), the four
//                               waves' totals through LDS, and a carry runs from chunk to chunk in a register every thread keeps.
//                               Edges alternate rising, falling, from a rising one: the edge with e edges in front of it is word e
//                               of the segment's interval array, (start_0, end_0, start_1, ...), and holds min(f H, T). The
//                               non-silent frame with c such frames in front of it is entry c of the segment's hop list. Integer
//                               sums only, no atomics: the order is the frames'.
//   3. vsyn_split_gather_kernel grid (tile of SPLIT_TILE output frames, segment), sized by the unsplit T; workgroups past out_frames
//                               leave at once. Output frame t lies in hop t / H of the hop list: out[t] = downmix(hops[t / H] H +
//                               t % H). One division per thread; the thread walks on from there.
// Memory access of the gather kernel: as the trim stage's cut kernel, a thread owns four output frames that start at a 16-byte
// boundary of the OUTPUT plane, with a scalar head and tail. Its four input frames are contiguous unless a hop ends among them, and
// with H a multiple of 4 they sit on a 16-byte boundary in every channel plane for all threads of a workgroup or for none
// (f H + t % H = t mod 4): 16-byte loads (cond_downmix4) then, four 4-byte loads per plane otherwise. Both forms do the same float32
// operations per frame.
// Nothing here reads or writes stream state, the overlap carry or any synthesis buffer; the PCM is only read.
#pragma once
#include "vsyn_trim.h"

#define SPLIT_PER 4u                               // consecutive positions per thread and chunk of the mark kernel
#define SPLIT_CHUNK (TRIM_THREADS * SPLIT_PER)     // positions per chunk
#define SPLIT_TILE (TRIM_THREADS * 4)              // output frames per gather workgroup

struct SplitCtx {  // launch arguments of the mark and gather kernels
  TrimCtx t;               // the energy kernel's, with out / out_plane / out_frames / ref of this stage (bounds unused)
  uint32_t* counts;        // [S] intervals
  uint32_t* iv;            // [S][iv_stride][2] start, end
  uint64_t iv_stride;
  uint32_t* hops;          // [S][F_max] the non-silent frames in order
};

__global__ void __launch_bounds__(TRIM_THREADS) vsyn_split_mark_kernel(const SplitCtx B) {
  __shared__ uint64_t s_a[TRIM_WAVES];
  __shared__ uint32_t s_e[2][TRIM_WAVES], s_l[2][TRIM_WAVES];  // the waves' totals of a chunk: two sets, one __syncthreads per chunk
  const TrimCtx& A = B.t;
  const uint32_t g = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint64_t T = trim_frames(A, g);
  const uint64_t F = trim_num_frames(T, A.L, A.H);
  const double* ms = A.ms + (size_t)g * A.F_max;
  const uint64_t mx = trim_segment_max(A, g, F, ms, s_a);
  const bool refused = trim_refused(mx);
  const double R = trim_ref(mx);
  if (refused || F == 0) {  // (workgroup-uniform)
    if (tid == 0) {
      B.counts[g] = 0u;
      A.out_frames[g] = 0u;
      A.ref[g] = R;
    }
    return;
  }
  const double thr = R * A.k;
  uint32_t* iv = B.iv + (size_t)g * B.iv_stride * 2u;
  uint32_t* hops = B.hops + (size_t)g * A.F_max;
  const uint64_t iv_words = B.iv_stride * 2u;
  uint32_t carry_e = 0u, carry_l = 0u;  // edges and non-silent frames in front of the chunk: the same in every thread
  uint32_t set = 0u;
  for (uint64_t c0 = 0; c0 <= F; c0 += SPLIT_CHUNK, set ^= 1u) {
    const uint64_t f0 = c0 + (uint64_t)tid * SPLIT_PER;
    bool prev = f0 > 0 && f0 - 1u < F && trim_loud(ms[f0 - 1u], R, thr);
    bool loud[SPLIT_PER];
    uint32_t ne = 0u, nl = 0u, edge = 0u;  // edge: bit i, an edge at position f0 + i
#pragma unroll
    for (uint32_t i = 0; i < SPLIT_PER; ++i) {
      const uint64_t f = f0 + i;
      loud[i] = f < F && trim_loud(ms[f], R, thr);
      if (f <= F && loud[i] != prev) {
        edge |= 1u << i;
        ++ne;
      }
      nl += loud[i] ? 1u : 0u;
      prev = loud[i];
    }
    const uint32_t se = wave_scan(ne), sl = wave_scan(nl);  // inclusive
    if (lane == 63u) {
      s_e[set][wave] = se;
      s_l[set][wave] = sl;
    }
    __syncthreads();
    uint32_t e = carry_e + se - ne, l = carry_l + sl - nl;  // in front of this thread's first position
#pragma unroll
    for (uint32_t w = 0; w < TRIM_WAVES; ++w) {
      if (w < wave) {
        e += s_e[set][w];
        l += s_l[set][w];
      }
      carry_e += s_e[set][w];
      carry_l += s_l[set][w];
    }
#pragma unroll
    for (uint32_t i = 0; i < SPLIT_PER; ++i) {
      const uint64_t f = f0 + i;
      if (edge & (1u << i)) {
        if (e < iv_words) iv[e] = (uint32_t)trim_min64(f * A.H, T);  // (e < 2 n <= F + 1: the host has checked the stride)
        ++e;
      }
      if (loud[i]) hops[l++] = (uint32_t)f;  // (l < F <= F_max)
    }
  }
  if (tid == 0) {  // carry_e: every edge, two per interval; carry_l: every non-silent frame, a hop each, the last one up to T
    uint64_t n = (uint64_t)carry_l * A.H;
    if (trim_loud(ms[F - 1u], R, thr)) n -= F * A.H - trim_min64(F * A.H, T);
    B.counts[g] = carry_e >> 1;
    A.out_frames[g] = (uint32_t)n;
    A.ref[g] = R;
  }
}

__global__ void __launch_bounds__(TRIM_THREADS) vsyn_split_gather_kernel(const SplitCtx B) {
  const TrimCtx& A = B.t;
  const uint32_t g = blockIdx.y, tid = threadIdx.x;
  const uint64_t n = A.out_frames[g];
  float* z = A.out + (size_t)g * A.out_plane;
  const uint32_t mo = (uint32_t)(((uintptr_t)z >> 2) & 3u);  // the output plane's offset from a 16-byte boundary, in floats
  const uint64_t tile0 = (uint64_t)blockIdx.x * SPLIT_TILE;
  if (tile0 >= n + mo) return;  // (workgroup-uniform)
  const uint32_t C = A.C, H = A.H;
  const float inv_c = 1.0f / (float)C;
  const float* x = A.pcm + (size_t)g * C * A.plane;
  const uint32_t* hops = B.hops + (size_t)g * A.F_max;
  // with H a multiple of 4 the input frame under output frame t is t mod 4: do the four input frames under an aligned group of four
  // output frames start at a 16-byte boundary in every plane?
  const bool in16 = (H & 3u) == 0u && (C == 1u || (A.plane & 3u) == 0u) && (((((uintptr_t)x >> 2) + 4u - mo) & 3u) == 0u);
  const int64_t t0 = (int64_t)(tile0 + 4u * tid) - (int64_t)mo;
  const uint64_t tf = t0 < 0 ? 0ull : (uint64_t)t0;  // the first frame of the group that exists
  if (tf >= n) return;
  uint32_t j = (uint32_t)(tf / H), r = (uint32_t)(tf - (uint64_t)j * H);  // hop and offset in it (n <= T < 2^32)
  uint64_t src = (uint64_t)hops[j] * H;
  if (t0 >= 0 && (uint64_t)t0 + 3u < n && (uint64_t)r + 3u < H) {
    float4 v;
    if (in16) {
      v = cond_downmix4(x, A.plane, C, inv_c, src + r);
    } else {
      v.x = pcm_downmix(x, A.plane, C, inv_c, src + r);
      v.y = pcm_downmix(x, A.plane, C, inv_c, src + r + 1u);
      v.z = pcm_downmix(x, A.plane, C, inv_c, src + r + 2u);
      v.w = pcm_downmix(x, A.plane, C, inv_c, src + r + 3u);
    }
    *(float4*)(z + t0) = v;
  } else {
    const uint64_t te = trim_min64((uint64_t)(t0 + 4), n);
    for (uint64_t t = tf; t < te; ++t) {
      z[t] = pcm_downmix(x, A.plane, C, inv_c, src + r);
      if (++r == H && t + 1u < te) {  // on to the next hop of the list (t + 1 < n: it is there)
        r = 0u;
        src = (uint64_t)hops[++j] * H;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct SplitWs {  // the stage's buffers: its own, the energy kernel's among them; the PCM is only read
  TrimWs e;                            // ms, flags, ref, frames; pcm and s16: the host forms' joined mono planes
  DevBuf<uint32_t> counts, iv, hops;   // per segment: intervals; (start, end) each; the non-silent frames
};

static inline uint64_t split_max_intervals(uint64_t T, uint32_t L, uint32_t H) { return (trim_num_frames(T, L, H) + 1u) / 2u; }

// The stage's kernels on stream s: frames from d_frames, else from si; t_max bounds every segment's frames. d_out NULL: no gather,
// the intervals alone. d_counts [S], d_iv [S][iv_stride][2], d_out_frames [S], d_ref [S] (each NULL: the workspace's, d_iv then
// with the stride *ws_stride receives); d_ms with ms_stride optional. Caller holds the handle's lock and has run trim_check.
static inline int split_launch(SplitWs& ws, int device, const vsyn_pcm_trim* tr, uint32_t S, const float* d_pcm, uint64_t plane, uint32_t C,
                        const uint32_t* d_frames, const SegInfo* si, uint64_t t_max, float* d_out, uint64_t out_plane, uint32_t* d_out_frames,
                        uint32_t* d_counts, uint32_t* d_iv, uint64_t iv_stride, uint64_t* ws_stride, double* d_ref, double* d_ms,
                        uint64_t ms_stride, hipStream_t s, const char** err) {
  const uint64_t T = std::min(std::min(t_max, plane), d_out ? out_plane : plane);
  const uint64_t need = std::max<uint64_t>(split_max_intervals(std::min<uint64_t>(T, 0xFFFFFFFFull), tr->frame_length, tr->hop_length), 1);
  if (d_iv && iv_stride < need)
    return fail(err, VSYN_ERR_INVALID, "intervals_stride %llu below %llu intervals", (unsigned long long)iv_stride, (unsigned long long)need);
  if (((uintptr_t)d_iv & 3u) || ((uintptr_t)d_counts & 3u)) return fail(err, VSYN_ERR_INVALID, "interval pointers must be 4-byte aligned");
  SplitCtx B;
  if (int rc = trim_energy_launch(ws.e, device, tr, S, d_pcm, plane, C, d_frames, si, t_max, d_out, d_out ? out_plane : plane, d_out_frames, nullptr,
                                  d_ref, d_ms, ms_stride, s, &B.t, err))
    return rc;
  if (!d_counts) {
    HIPCHK(ws.counts.ensure(S));
    d_counts = ws.counts.p;
  }
  if (!d_iv) {
    HIPCHK(ws.iv.ensure((size_t)S * need * 2u));
    d_iv = ws.iv.p;
    iv_stride = need;
  }
  if (ws_stride) *ws_stride = iv_stride;
  HIPCHK(ws.hops.ensure((size_t)S * B.t.F_max));
  B.counts = d_counts;
  B.iv = d_iv;
  B.iv_stride = iv_stride;
  B.hops = ws.hops.p;
  VSYN_LAUNCH(vsyn_split_mark_kernel, dim3(S), dim3(TRIM_THREADS), 0, s, B);
  if (d_out) {
    const uint64_t gx = (B.t.t_cap + 3u + SPLIT_TILE - 1u) / SPLIT_TILE;
    VSYN_LAUNCH(vsyn_split_gather_kernel, dim3((uint32_t)gx, S), dim3(TRIM_THREADS), 0, s, B);
  }
  return VSYN_OK;
}

// counts_out[S], intervals_out[S][iv_stride][2] and refs_out[S] (each may be NULL) from the workspace (its intervals at ws_stride)
// behind the kernels on stream s
static inline int split_fetch(const SplitWs& ws, uint32_t S, uint32_t* counts_out, uint32_t* intervals_out, uint64_t iv_stride, uint64_t ws_stride,
                       double* refs_out, hipStream_t s, const char** err) {
  if (!S) return VSYN_OK;
  if (counts_out) HIPCHK(hipMemcpyAsync(counts_out, ws.counts.p, sizeof(uint32_t) * S, hipMemcpyDeviceToHost, s));
  const uint64_t w = std::min(iv_stride, ws_stride);  // (every count is at most either)
  if (intervals_out && w)
    HIPCHK(hipMemcpy2DAsync(intervals_out, sizeof(uint32_t) * 2u * iv_stride, ws.iv.p, sizeof(uint32_t) * 2u * ws_stride, sizeof(uint32_t) * 2u * w, S,
                            hipMemcpyDeviceToHost, s));
  if (refs_out) HIPCHK(hipMemcpyAsync(refs_out, ws.e.ref.p, sizeof(double) * S, hipMemcpyDeviceToHost, s));
  return VSYN_OK;
}
