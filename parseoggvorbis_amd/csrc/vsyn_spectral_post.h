// vsyn_spectral_post.h — delta / delta-delta columns and per-column mean / variance normalisation of spectral rows already on the
// device. Semantics: include/vorbis_synth_hip.h, "spectral post-processing".
//
// The host knows every segment's row count, so it uploads one PostSeg per segment (row offset, offset of its 16-row blocks, rows)
// with the float32 delta coefficients and, for given statistics, the columns' mu and 1 / max(sigma, std_floor) in double
// (vorbis_synth_hip.hip post_launch). Up to five launches on one stream:
//   1. vsyn_post_delta_kernel   one workgroup per (segment, tile of `tile` rows). The tile's rows of X plus the halo of the
//                               clamped window go through (dynamic) LDS once; a thread owns one output column j of one 16-row block at a
//                               time and walks the block's rows in ascending order: lanes run along j, so a wave's loads and
//                               stores are contiguous, and for D_out < 256 the workgroup's 256 / D_out row groups take different
//                               blocks instead of idling. Writes Y = [X | D_1 | D_2] at pitch D_out and, when statistics are
//                               wanted, the block's float64 column sum.
//   2. vsyn_post_reduce_kernel  per (segment, column): the blocks' partials added in a fixed two-level order (16 interleaved chains,
//                               each in ascending block order, then the chains in order) -> mu, or (second call, on the partials
//                               of 3) sigma -> 1 / max(sigma, std_floor). No atomics: the order is a function of the rows alone.
//   3. vsyn_post_moment_kernel  mean + variance per segment: the blocks' float64 sums of (Y - mu)^2, a second pass over Y (exact on
//                               columns with a large mean and a small spread, which sum(Y^2) - F mu^2 is not).
//   4. vsyn_post_norm_kernel    Y = float((double(Y) - mu) * rinv) in place.
// A block is always 16 rows of its segment, whatever the tile, the grid or the segment's place in the batch: the same rows give
// the same bits. Nothing here reads or writes stream state, the overlap carry or PCM.
#pragma once
#include "vsyn_device.h"
#include "vsyn_host.h"
#include "vsyn_spectral.h"  // SPEC_LDS_BUDGET

#define POST_THREADS 256
#define POST_BLK 16u  // rows per block of partial sums
#define POST_RED_CHAINS 16u  // vsyn_post_reduce_kernel: interleaved chains of block partials per column ...
#define POST_RED_COLS 16u    // ... and columns per workgroup (POST_RED_CHAINS * POST_RED_COLS = POST_THREADS)
#define POST_COEF_FLOATS 132u  // LDS floats in front of the tile's rows: two coefficient vectors of up to 65

typedef RowBlkSeg PostSeg;  // blk: the segment's first block in the partials

struct PostCtx {  // launch arguments
  const PostSeg* seg;
  const float* coef;  // c1[width] | c2[width]
  const float* in;    // [rows][D]
  float* out;         // [rows][Dout]
  double* part;       // [blocks][Dout], or NULL
  double* mu;         // [S or 1][Dout]
  double* rinv;       // [S or 1][Dout]
  uint32_t stat_stride;  // Dout per segment, 0 for given statistics
  uint32_t D, Dout, order, width, tile;
  double std_floor;
};

// Thread layout over a tile (row_lane): group ty takes blocks ty, ty + G, ...
__device__ __forceinline__ uint32_t post_clamp(uint32_t f, uint32_t lo, uint32_t hi) { return min(max(f, lo), hi); }

__global__ void __launch_bounds__(POST_THREADS) vsyn_post_delta_kernel(const PostCtx A) {
  extern __shared__ float s_c[];  // c1, c2 [POST_COEF_FLOATS] | the tile's rows of X
  float* s_x = s_c + POST_COEF_FLOATS;
  const PostSeg sg = A.seg[blockIdx.y];
  const uint32_t F = sg.F, f0 = blockIdx.x * A.tile, tid = threadIdx.x;
  if (f0 >= F) return;
  const uint32_t D = A.D, Dout = A.Dout, W = A.width;
  const uint32_t nrows = min(A.tile, F - f0);
  const uint32_t h = A.order ? (W - 1u) / 2u : 0u;  // the host has refused 0 < F < width when order > 0
  // rows of X the tile reads: its own, and the windows of its rows clamped to [h, F - 1 - h]
  const uint32_t lo = post_clamp(f0, h, F - 1u - h) - h, hi = post_clamp(f0 + nrows - 1u, h, F - 1u - h) + h + 1u;
  const float* x = A.in + (sg.off + lo) * D;
  for (uint32_t i = tid; i < (hi - lo) * D; i += POST_THREADS) s_x[i] = x[i];
  if (A.order)
    for (uint32_t i = tid; i < A.order * W; i += POST_THREADS) s_c[i] = A.coef[i];
  __syncthreads();
  const RowLane L = row_lane<POST_THREADS>(Dout);
  if (L.ty >= L.G) return;
  const uint32_t nblk = (nrows + POST_BLK - 1u) / POST_BLK;
  for (uint32_t b = L.ty; b < nblk; b += L.G) {
    const uint32_t fb = f0 + b * POST_BLK, fe = min(fb + POST_BLK, f0 + nrows);
    for (uint32_t j = L.tx; j < Dout; j += L.wd) {
      const uint32_t o = j / D, d = j - o * D;
      const float* c = s_c + (o ? o - 1u : 0u) * W;
      float* y = A.out + (sg.off + fb) * Dout + j;
      double sum = 0.0;
      for (uint32_t f = fb; f < fe; ++f, y += Dout) {
        float v;
        if (o == 0) {
          v = s_x[(f - lo) * D + d];
        } else {
          const float* p = s_x + (post_clamp(f, h, F - 1u - h) - h - lo) * D + d;
          v = 0.f;
          for (uint32_t k = 0; k < W; ++k) v = fmaf(c[k], p[k * D], v);
        }
        *y = v;
        sum += (double)v;
      }
      if (A.part) A.part[(sg.blk + fb / POST_BLK) * Dout + j] = sum;
    }
  }
}

// part[block][j] = sum over the block's rows of (Y - mu)^2, rows ascending
__global__ void __launch_bounds__(POST_THREADS) vsyn_post_moment_kernel(const PostCtx A) {
  const PostSeg sg = A.seg[blockIdx.y];
  const uint32_t F = sg.F, f0 = blockIdx.x * A.tile, Dout = A.Dout;
  if (f0 >= F) return;
  const uint32_t nrows = min(A.tile, F - f0);
  const RowLane L = row_lane<POST_THREADS>(Dout);
  if (L.ty >= L.G) return;
  const double* mu = A.mu + (size_t)blockIdx.y * A.stat_stride;
  const uint32_t nblk = (nrows + POST_BLK - 1u) / POST_BLK;
  for (uint32_t b = L.ty; b < nblk; b += L.G) {
    const uint32_t fb = f0 + b * POST_BLK, fe = min(fb + POST_BLK, f0 + nrows);
    for (uint32_t j = L.tx; j < Dout; j += L.wd) {
      const double m = mu[j];
      const float* y = A.out + (sg.off + fb) * Dout + j;
      double sum = 0.0;
      for (uint32_t f = fb; f < fe; ++f, y += Dout) {
        const double t = (double)*y - m;
        sum += t * t;
      }
      A.part[(sg.blk + fb / POST_BLK) * Dout + j] = sum;
    }
  }
}

// One workgroup per (segment, POST_RED_COLS columns), a fixed two-level order: chain i of POST_RED_CHAINS adds the partials of
// blocks i, i + POST_RED_CHAINS, ... in ascending order, then the chains are added in ascending order (a chain without a block adds
// 0). second = 0: mu = sum / F, rinv = 1. second = 1: rinv = 1 / max(sqrt(sum / F), std_floor).
__global__ void __launch_bounds__(POST_THREADS) vsyn_post_reduce_kernel(const PostCtx A, const uint32_t second) {
  __shared__ double s_sum[POST_RED_CHAINS][POST_RED_COLS];
  const PostSeg sg = A.seg[blockIdx.y];
  const uint32_t cy = threadIdx.x / POST_RED_COLS, cx = threadIdx.x % POST_RED_COLS;
  const uint32_t j = blockIdx.x * POST_RED_COLS + cx, Dout = A.Dout;
  if (sg.F == 0) return;
  const uint32_t nblk = (sg.F + POST_BLK - 1u) / POST_BLK;
  double sum = 0.0;
  if (j < Dout) {
    const double* p = A.part + sg.blk * Dout + j;
    for (uint32_t b = cy; b < nblk; b += POST_RED_CHAINS) sum += p[(size_t)b * Dout];
  }
  s_sum[cy][cx] = sum;
  __syncthreads();
  if (cy != 0 || j >= Dout) return;
  sum = s_sum[0][cx];
  for (uint32_t i = 1; i < POST_RED_CHAINS; ++i) sum += s_sum[i][cx];
  const size_t q = (size_t)blockIdx.y * A.stat_stride + j;
  const double v = sum / (double)sg.F;
  if (!second) {
    A.mu[q] = v;
    A.rinv[q] = 1.0;
  } else {
    A.rinv[q] = 1.0 / fmax(sqrt(v), A.std_floor);
  }
}

__global__ void __launch_bounds__(POST_THREADS) vsyn_post_norm_kernel(const PostCtx A) {
  const PostSeg sg = A.seg[blockIdx.y];
  const uint32_t F = sg.F, f0 = blockIdx.x * A.tile, Dout = A.Dout;
  if (f0 >= F) return;
  const uint32_t nrows = min(A.tile, F - f0);
  const RowLane L = row_lane<POST_THREADS>(Dout);
  if (L.ty >= L.G) return;
  const size_t s0 = (size_t)blockIdx.y * A.stat_stride;
  const uint32_t nblk = (nrows + POST_BLK - 1u) / POST_BLK;
  for (uint32_t b = L.ty; b < nblk; b += L.G) {
    const uint32_t fb = f0 + b * POST_BLK, fe = min(fb + POST_BLK, f0 + nrows);
    for (uint32_t j = L.tx; j < Dout; j += L.wd) {
      const double m = A.mu[s0 + j], r = A.rinv[s0 + j];
      float* y = A.out + (sg.off + fb) * Dout + j;
      for (uint32_t f = fb; f < fe; ++f, y += Dout) *y = (float)(((double)*y - m) * r);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct PostWs {  // the stage's buffers: a second row buffer (the output rows are wider) and the statistics
  TableUpload tab;
  bool lds_set = false;                // vsyn_post_delta_kernel's dynamic-LDS limit is raised on this handle's device
  DevBuf<float> rows;
  DevBuf<double> part, stat;           // per-block partial sums; mu | rinv per (segment, column)
};

static inline bool post_on(const vsyn_spectral_post* p) { return p->order != 0 || p->norm != VSYN_POST_NORM_NONE; }
static inline bool post_given(const vsyn_spectral_post* p) { return p->norm != VSYN_POST_NORM_NONE && p->stats == VSYN_POST_STATS_GIVEN; }

// The checks of the post spec that need no row counts; the given vectors are read for finiteness only when dout != 0.
static inline int post_check(const vsyn_spectral_post* p, const char** err, uint32_t dout = 0) {
  if (!p) return fail(err, VSYN_ERR_INVALID, "spectral post spec is NULL");
  if (p->order > 2) return fail(err, VSYN_ERR_INVALID, "delta order %u outside [0, 2]", p->order);
  if (p->width < 3 || p->width > VSYN_POST_MAX_WIDTH || !(p->width & 1u))
    return fail(err, VSYN_ERR_INVALID, "delta width %u must be odd and in [3, %u]", p->width, VSYN_POST_MAX_WIDTH);
  if (p->norm > VSYN_POST_NORM_MEAN_VAR) return fail(err, VSYN_ERR_INVALID, "unknown normalisation %u", p->norm);
  if (p->stats > VSYN_POST_STATS_GIVEN) return fail(err, VSYN_ERR_INVALID, "unknown statistics source %u", p->stats);
  if (!(p->std_floor > 0.0) || !std::isfinite(p->std_floor)) return fail(err, VSYN_ERR_INVALID, "std_floor must be finite and > 0");
  if (post_given(p)) {
    const bool var = p->norm == VSYN_POST_NORM_MEAN_VAR;
    if (!p->mean || (var && !p->std)) return fail(err, VSYN_ERR_INVALID, "given statistics: %s is NULL", p->mean ? "std" : "mean");
    for (uint32_t j = 0; j < dout; ++j)
      if (!std::isfinite(p->mean[j]) || (var && !std::isfinite(p->std[j])))
        return fail(err, VSYN_ERR_INVALID, "given statistics: column %u is not finite", j);
  }
  return VSYN_OK;
}

// The post spec of a spectral entry point against its (checked) spectral spec: post_check with the rows' width, after the refusal
// of the stage on rows of a linear kind (its layout holds 256 columns), which comes before the given vectors are read.
static inline int spec_post_check(const vsyn_spectral_spec* spec, const vsyn_spectral_post* post, const char** err,
                                  const vsyn_spectral_chroma* chroma = nullptr) {
  if (int rc = post_check(post, err)) return rc;
  if (spec_is_lin(spec) && post_on(post)) return fail(err, VSYN_ERR_INVALID, "the post stage does not take rows of a linear kind (kind %u)", spec->kind);
  return post_check(post, err, spec_dim(spec, chroma) * (1u + post->order));
}

// A segment shorter than the delta window is refused by name.
static inline int post_check_rows(const vsyn_spectral_post* p, uint32_t S, const uint64_t* seg_rows, const char** err) {
  if (S && !seg_rows) return fail(err, VSYN_ERR_INVALID, "seg_rows is NULL");
  for (uint32_t g = 0; g < S; ++g) {
    if (seg_rows[g] > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "segment %u: too many rows", g);
    if (p->order && seg_rows[g] && seg_rows[g] < p->width)
      return fail(err, VSYN_ERR_INVALID, "segment %u: delta width %u needs %u frames, segment has %llu", g, p->width, p->width,
                  (unsigned long long)seg_rows[g]);
  }
  return VSYN_OK;
}

// The stage's kernels on stream s: d_in [rows][D] -> d_out [rows][D * (1 + order)]. Caller holds the handle's lock, has run post_check (with
// dout) and post_check_rows, and post_on(p) holds.
static inline int post_launch(PostWs& ws, int device, const vsyn_spectral_post* p, uint32_t D, uint32_t S, const uint64_t* seg_rows, const float* d_in,
                       float* d_out, hipStream_t s, const char** err) {
  if (S > 65535u) return fail(err, VSYN_ERR_INVALID, "too many segments (%u > 65535)", S);
  const uint32_t W = p->width, Dout = D * (1u + p->order), hh = p->order ? (W - 1u) / 2u : 0u;
  const bool norm = p->norm != VSYN_POST_NORM_NONE, given = post_given(p), var = p->norm == VSYN_POST_NORM_MEAN_VAR;
  // table: PostSeg[S] | given mu[Dout], rinv[Dout] (double) | c1[W], c2[W] (float)
  const size_t off_stat = sizeof(PostSeg) * S, off_coef = off_stat + (given ? 16ull * Dout : 0ull);
  std::vector<uint8_t> tab(off_coef + 8ull * W);
  PostSeg* seg = (PostSeg*)tab.data();
  const RowTotals t = row_segs_fill(seg, S, seg_rows, nullptr, POST_BLK);
  const uint64_t blocks = t.blocks, f_max = t.f_max;
  if (f_max == 0) return VSYN_OK;
  if (given) {
    double* st = (double*)(tab.data() + off_stat);
    for (uint32_t j = 0; j < Dout; ++j) {
      st[j] = (double)p->mean[j];
      st[Dout + j] = var ? 1.0 / std::max((double)p->std[j], p->std_floor) : 1.0;
    }
  }
  float* coef = (float*)(tab.data() + off_coef);
  double S2 = 0, S4 = 0;
  for (int k = -(int)hh; k <= (int)hh; ++k) {
    S2 += (double)k * k;
    S4 += (double)k * k * k * k;
  }
  for (uint32_t i = 0; i < W && hh; ++i) {
    const double k = (double)i - (double)hh;
    coef[i] = (float)(k / S2);
    coef[W + i] = (float)(2.0 * (W * k * k - S2) / (W * S4 - S2 * S2));
  }
  // the tile: every row group of the workgroup gets a block, at least four blocks, and the LDS image fits
  const uint32_t G = POST_THREADS / std::min<uint32_t>(Dout, POST_THREADS);
  uint32_t nb = G * ((4u + G - 1u) / G);
  const auto lds_of = [&](uint32_t blocks) { return ((size_t)(blocks * POST_BLK + 2u * hh) * D + POST_COEF_FLOATS) * 4u; };
  while (nb > 1u && lds_of(nb) > SPEC_LDS_BUDGET) --nb;
  const uint32_t tile = nb * POST_BLK;
  const size_t lds = lds_of(nb);
  HIPCHK(hipSetDevice(device));
  if (int rc = raise_lds_once(ws.lds_set, {{(const void*)vsyn_post_delta_kernel, SPEC_LDS_BUDGET}}, err)) return rc;
  const bool seg_stats = norm && !given;
  if (seg_stats) {
    HIPCHK(ws.part.ensure(blocks * Dout));
    HIPCHK(ws.stat.ensure(2ull * S * Dout));
  }
  if (int rc = ws.tab.upload(tab, s, err)) return rc;
  PostCtx A;
  A.seg = (const PostSeg*)ws.tab.dev.p;
  A.coef = (const float*)(ws.tab.dev.p + off_coef);
  A.in = d_in;
  A.out = d_out;
  A.part = seg_stats ? ws.part.p : nullptr;
  A.mu = given ? (double*)(ws.tab.dev.p + off_stat) : ws.stat.p;
  A.rinv = given ? A.mu + Dout : ws.stat.p + (size_t)S * Dout;
  A.stat_stride = given ? 0u : Dout;
  A.D = D;
  A.Dout = Dout;
  A.order = p->order;
  A.width = W;
  A.tile = tile;
  A.std_floor = p->std_floor;
  const uint64_t gx = (f_max + tile - 1u) / tile;
  const dim3 grid((uint32_t)gx, S), rgrid((Dout + POST_RED_COLS - 1u) / POST_RED_COLS, S);
  VSYN_LAUNCH(vsyn_post_delta_kernel, grid, dim3(POST_THREADS), lds, s, A);
  if (seg_stats) {
    VSYN_LAUNCH(vsyn_post_reduce_kernel, rgrid, dim3(POST_THREADS), 0, s, A, 0u);
    if (var) {
      VSYN_LAUNCH(vsyn_post_moment_kernel, grid, dim3(POST_THREADS), 0, s, A);
      VSYN_LAUNCH(vsyn_post_reduce_kernel, rgrid, dim3(POST_THREADS), 0, s, A, 1u);
    }
  }
  if (norm) {
    VSYN_LAUNCH(vsyn_post_norm_kernel, grid, dim3(POST_THREADS), 0, s, A);
  }
  return VSYN_OK;
}
