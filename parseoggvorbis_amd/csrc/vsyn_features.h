// vsyn_features.h — the feature matrices of the reference's RETURNN reader (returnn_import.py:74-115, demo_live_extract.py:262-505)
// straight from a batch: no IMDCT, no window, no PCM. Semantics: include/vorbis_synth_hip.h, "feature matrices".
//
// Four kernels on one stream, all reading the batch and the constant block only (the handle's stream state and synthesis workspace
// are not touched):
//   1. vsyn_feat_count_kernel    one workgroup per segment: per packet the row count (from floor_used, the mode's channel_floor and
//                                the kind), the segment's exclusive row scan, the residue offset scan, and the floor_base source (the
//                                last packet at or before this one, inside the segment, with a used biggest-floor channel: a max scan).
//                                Also the PktInfo fields the floor unwrap reads (own, mapping, bad).
//   2. vsyn_feat_offsets_kernel  one workgroup: seg_row_off[S+1] from the per-segment totals.
//   3. vsyn_floor_unwrap_kernel  (vsyn_staged.h, floor1_unwrap_rows) floor-1 step 1 of every used (packet, channel) row.
//   4. vsyn_feat_rows_kernel     one wave64 per (packet, channel) slot, lanes across the output columns: the floor-value check of the
//                                row (the reference's CHECK(floor[i] < 256) over all n entries), then the row itself — posts, the
//                                integer curve evaluated at the gathered x only (floor1_curve_at, the per-bin closed form), or the
//                                residue at the gathered bins.
#pragma once
#include "vsyn_device.h"
#include "vsyn_host.h"
#include "vsyn_staged.h"

// Per-floor gather table, built on the host per call (vorbis_synth_hip.hip, feat_build_table) and read by the rows kernel.
struct FeatFloor {
  uint32_t cnt;     // gather indices kept (columns)
  uint32_t maxidx;  // largest index of the whole list (the reference gathers ALL of it before slicing): checked against n unless clipped
  uint32_t clip;    // 1: indices are clipped to [0, n-1] (xs_from_biggest_floor)
  uint32_t off;     // first index in FeatTab::idx
  float fnum;       // floor-number column: (f + 1) / num_floors - 0.5, in double, rounded
  uint32_t pad[3];
};
struct FeatHeader {
  uint32_t kind, dim, opts, big, num_floors, res_cnt, res_off, pad;
  float scale, clip, fbf, pad2;
};
// layout: FeatHeader, FeatFloor[num_floors], uint32 idx[]; the residue kinds' list (biggest floor's xs[:dim]) at res_off

struct FeatCtx {  // launch arguments
  const uint8_t* cb;
  const uint8_t* tab;
  const vsyn_packet* pk;
  const vsyn_segment* seg;
  const uint16_t* fy;
  const float* res;
  PktInfo* info;
  uint32_t* rowrel;    // [P] rows of the segment in front of the packet
  int32_t* fbsrc;      // [P] floor_base source packet (-1: none yet)
  uint8_t* fbch;       // [P] channel of the packet's last used biggest-floor row (0xFF: none)
  uint64_t* resoff;    // [P] float index of the packet's residue block
  uint64_t* segrows;   // [S]
  uint64_t* segoff;    // [S+1]
  float* rows;
  DevStatus* status;
  uint32_t P, S;
  uint32_t max_seg;    // the launch's max_seg_packets: the rows grid covers no more (a longer segment is flagged, VSYN_ST_BAD_SEGMENT)
};

#define FEAT_THREADS 256
#define FEAT_ROW_WAVES 4

__device__ __forceinline__ const FeatHeader* feat_hdr(const uint8_t* t) { return (const FeatHeader*)t; }
__device__ __forceinline__ const FeatFloor* feat_floor(const uint8_t* t, uint32_t f) { return (const FeatFloor*)(t + sizeof(FeatHeader)) + f; }
__device__ __forceinline__ const uint32_t* feat_idx(const uint8_t* t) {
  return (const uint32_t*)(t + sizeof(FeatHeader) + sizeof(FeatFloor) * feat_hdr(t)->num_floors);
}

// the row mask of a packet: bit c = channel c makes a row
__device__ __forceinline__ uint32_t feat_row_mask(const FeatHeader* T, const MapConst* mc, uint32_t own, uint32_t C) {
  uint32_t m = 0;
  if (T->kind <= VSYN_FEAT_FLOOR_FINAL_YS_RENDERED) {
    for (uint32_t c = 0; c < C; ++c)
      if (((own >> c) & 1u) && (!(T->opts & VSYN_FEAT_ONLY_BIGGEST_FLOOR) || mc->chfloor[c] == T->big)) m |= 1u << c;
  } else if (mc->chfloor[C - 1] == T->big) {
    m = C >= 32 ? 0xFFFFFFFFu : (1u << C) - 1u;
  }
  return m;
}

__global__ void __launch_bounds__(FEAT_THREADS) vsyn_feat_count_kernel(const FeatCtx A) {
  __shared__ uint32_t s_rows[FEAT_THREADS];
  __shared__ uint64_t s_res[FEAT_THREADS];
  __shared__ int32_t s_src[FEAT_THREADS];
  const uint32_t g = blockIdx.x, t = threadIdx.x;
  const ConstHeader* H = hdr_of(A.cb);
  const FeatHeader* T = feat_hdr(A.tab);
  const uint32_t C = H->channels;
  const vsyn_segment sg = A.seg[g];
  if ((uint64_t)sg.first_packet + sg.num_packets > A.P || (sg.residue_off & 3u) || sg.num_packets > A.max_seg) {
    if (t == 0) {
      raise_status(A.status, VSYN_ST_BAD_SEGMENT, sg.first_packet < A.P ? sg.first_packet : 0u);
      A.segrows[g] = 0;
    }
    return;
  }
  const uint32_t cmask = C >= 32 ? 0xFFFFFFFFu : (1u << C) - 1u;
  uint32_t carry_rows = 0;
  uint64_t carry_res = sg.residue_off;
  int32_t carry_src = -1;
  for (uint32_t base = 0; base < sg.num_packets; base += FEAT_THREADS) {
    const uint32_t q = base + t;
    const bool in = q < sg.num_packets;
    const uint32_t p = sg.first_packet + (in ? q : 0u);
    uint32_t rows = 0, n = 0;
    int32_t src = -1;
    if (in) {
      const vsyn_packet k = A.pk[p];
      const bool mode_ok = k.mode < H->num_modes;
      const uint32_t lng = mode_ok ? H->mode_blockflag[k.mode] : 0u;
      n = H->bs[lng];
      PktInfo pi = {};
      pi.n = (uint16_t)n;
      pi.lng = (uint8_t)lng;
      uint8_t qc = 0xFF;
      if (!mode_ok) {
        raise_status(A.status, VSYN_ST_BAD_MODE, p);
        pi.bad = 1;
      } else {
        const uint32_t mapping = H->mode_mapping[k.mode];
        const MapConst* mc = map_of(A.cb, mapping);
        const uint32_t own = k.floor_used & cmask;
        pi.mapping = (uint8_t)mapping;
        pi.own = own;
        pi.used = own;
        rows = (uint32_t)__popc(feat_row_mask(T, mc, own, C));
        for (uint32_t c = 0; c < C; ++c)
          if (((own >> c) & 1u) && mc->chfloor[c] == T->big) qc = (uint8_t)c;
        if (qc != 0xFF) src = (int32_t)p;
      }
      A.info[p] = pi;
      A.fbch[p] = qc;
    }
    // inclusive scans over the chunk (Hillis-Steele in LDS: a few hundred packets per segment, not worth more)
    s_rows[t] = rows;
    s_res[t] = (uint64_t)C * (n / 2u);
    s_src[t] = src;
    __syncthreads();
    for (uint32_t d = 1; d < FEAT_THREADS; d <<= 1) {
      uint32_t r = 0;
      uint64_t e = 0;
      int32_t m = -1;
      if (t >= d) {
        r = s_rows[t - d];
        e = s_res[t - d];
        m = s_src[t - d];
      }
      __syncthreads();
      if (t >= d) {
        s_rows[t] += r;
        s_res[t] += e;
        s_src[t] = max(s_src[t], m);
      }
      __syncthreads();
    }
    if (in) {
      A.rowrel[p] = carry_rows + s_rows[t] - rows;
      A.resoff[p] = carry_res + s_res[t] - (uint64_t)C * (n / 2u);
      A.fbsrc[p] = max(carry_src, s_src[t]);
    }
    carry_rows += s_rows[FEAT_THREADS - 1];
    carry_res += s_res[FEAT_THREADS - 1];
    carry_src = max(carry_src, s_src[FEAT_THREADS - 1]);
    __syncthreads();
  }
  if (t == 0) A.segrows[g] = carry_rows;
}

__global__ void __launch_bounds__(FEAT_THREADS) vsyn_feat_offsets_kernel(const FeatCtx A) {
  wg_exclusive_scan<FEAT_THREADS, 1>(A.S, A.segoff, [&](uint32_t g, uint64_t* v) { v[0] = A.segrows[g]; });
}

// The reference's CHECK(floor[i] < 256) over all n entries of a decoded floor (hpp:586-588): the curve is piecewise linear between the
// flagged posts and flat after the last, so its largest value below n sits on a flagged post with x < n or at x = n - 1.
__device__ __forceinline__ bool feat_floor_value_ok(const FloorConst* fc, const uint16_t* __restrict__ fyrow, uint32_t n, uint32_t lane) {
  bool ok = true;
  for (uint32_t s = lane; s < fc->posts; s += 64u) {
    const uint32_t v = fyrow[fc->sorted_idx[s]];
    if ((v >> 15) && fc->xs_sorted[s] < n && (v & 0x7FFFu) >= 256u) ok = false;
  }
  if (lane == 0 && floor1_curve_at(fc, fyrow, n - 1u) >= 256u) ok = false;
  return !__any(!ok);
}

__global__ void __launch_bounds__(FEAT_ROW_WAVES * 64) vsyn_feat_rows_kernel(const FeatCtx A) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t slot = blockIdx.x * FEAT_ROW_WAVES + (threadIdx.x >> 6);
  const uint32_t g = blockIdx.y;
  const ConstHeader* H = hdr_of(A.cb);
  const FeatHeader* T = feat_hdr(A.tab);
  const uint32_t C = H->channels, stride = H->ys_stride, dim = T->dim;
  const vsyn_segment sg = A.seg[g];
  if ((uint64_t)sg.first_packet + sg.num_packets > A.P || (sg.residue_off & 3u) || sg.num_packets > A.max_seg) return;
  if (slot >= sg.num_packets * C) return;
  const uint32_t p = sg.first_packet + slot / C, c = slot % C;
  const PktInfo pi = A.info[p];
  if (pi.bad) return;
  const MapConst* mc = map_of(A.cb, pi.mapping);
  const uint32_t n = pi.n;
  const bool used = (pi.own >> c) & 1u;
  const FloorConst* fc = floor_of(A.cb, mc->chfloor[c]);
  const uint16_t* fyrow = A.fy + ((size_t)p * C + c) * stride;
  if (used && !feat_floor_value_ok(fc, fyrow, n, lane)) {
    if (lane == 0) raise_status(A.status, VSYN_ST_FLOOR_VALUE, p);
  }
  const uint32_t mask = feat_row_mask(T, mc, pi.own, C);
  if (!((mask >> c) & 1u)) return;
  const uint64_t r = A.segoff[g] + A.rowrel[p] + (uint32_t)__popc(mask & ((1u << c) - 1u));
  float* out = A.rows + r * dim;
  const uint32_t* idx = feat_idx(A.tab);
  if (T->kind <= VSYN_FEAT_FLOOR_FINAL_YS_RENDERED) {
    const bool pos = (T->opts & VSYN_FEAT_FLOOR_ALWAYS_POSITIVE) != 0;
    const uint32_t f = mc->chfloor[c];
    const FeatFloor ff = *feat_floor(A.tab, f);
    const uint32_t o = (T->opts & VSYN_FEAT_INCLUDE_FLOOR_NUMBER) ? 1u : 0u;
    const bool rendered = T->kind == VSYN_FEAT_FLOOR_FINAL_YS_RENDERED;
    const bool oob = rendered && !ff.clip && ff.maxidx >= n;  // IndexError in the reference
    if (oob && lane == 0) raise_status(A.status, VSYN_ST_FEATURE_INDEX, p);
    const uint32_t cnt = rendered ? ff.cnt : min(fc->posts, dim - o);
    for (uint32_t j = lane; j < dim; j += 64u) {
      float v = 0.f;
      if (j < o) {
        v = ff.fnum;
      } else if (j - o < cnt && !oob) {
        uint32_t y;
        if (rendered) {
          uint32_t x = idx[ff.off + (j - o)];
          if (ff.clip) x = min(x, n - 1u);
          y = floor1_curve_at(fc, fyrow, x);
        } else {
          y = fyrow[j - o] & 0x7FFFu;  // final_y * multiplier (exact: the reader's float32(final_y) * multiplier)
        }
        const float yf = (float)y;
        v = pos ? yf / 255.0f : (yf - 127.5f) / 127.5f;
      }
      out[j] = v;
    }
    return;
  }
  // residue kinds: the reader's floor number is the last channel's, which is the biggest floor here
  const uint32_t n2 = n / 2u;
  const bool ignore = (T->opts & VSYN_FEAT_IGNORE_XS) != 0;
  const uint32_t cnt = ignore ? min(n2, dim) : T->res_cnt;
  const FloorConst* fcb = floor_of(A.cb, T->big);
  const int32_t src = T->kind == VSYN_FEAT_RESIDUE_YS_WITH_FLOOR ? A.fbsrc[p] : -1;
  const uint16_t* fbrow = nullptr;
  uint32_t nfb = 0;
  bool bad = false;
  if (src >= 0) {
    const uint32_t qc = A.fbch[src];
    fbrow = A.fy + ((size_t)src * C + qc) * stride;
    nfb = A.info[src].n;
    if (ignore && min(nfb, dim) != cnt) bad = true;  // numpy cannot broadcast floor_base against the row
  }
  if (bad && lane == 0) raise_status(A.status, VSYN_ST_FEATURE_INDEX, p);
  const float* resrow = A.res + A.resoff[p] + (size_t)c * n2;
  const bool lg = (T->opts & VSYN_FEAT_LOG1P_ABS_SPACE) != 0, clp = (T->opts & VSYN_FEAT_CLIP) != 0;
  for (uint32_t j = lane; j < dim; j += 64u) {
    float v = 0.f;
    if (j < cnt && !bad) {
      const uint32_t xi = ignore ? j : idx[T->res_off + j];
      v = resrow[min(xi, n2 - 1u)];
      // log1p / exp evaluated in double and rounded once: the correctly rounded float32 value, which is what numpy's float32 loops
      // give in all but rare cases (the single-precision ocml functions are off by up to 2 ulp, and the product below adds to that)
      if (lg) v = (float)log1p((double)fabsf(v));
      if (fbrow) {
        const uint32_t xf = min(ignore ? j : idx[T->res_off + j], nfb - 1u);
        const float fb = (float)floor1_curve_at(fcb, fbrow, xf) / 255.0f;
        if (lg) v = v + fb * T->fbf;
        else v = v * (float)exp((double)((fb - 1.0f) * T->fbf));
      }
      v = v * T->scale;
      if (clp) v = fminf(fmaxf(v, -T->clip), T->clip);
    }
    out[j] = v;
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct FeatureWs {  // the stage's buffers: its own, so that a features call leaves every synthesis buffer alone
  DevBuf<PktInfo> info;
  DevBuf<uint16_t> fy;
  DevBuf<uint32_t> rowrel;
  DevBuf<int32_t> fbsrc;
  DevBuf<uint8_t> fbch;
  DevBuf<uint64_t> resoff, segrows, segoff;
  TableUpload tab;                     // the gather table
  DevBuf<vsyn_packet> st_pk;           // vsyn_features_host staging
  DevBuf<vsyn_segment> st_seg;
  DevBuf<uint16_t> st_ys;
  DevBuf<float> st_res, st_rows;
};

// scipy.ndimage.zoom(xs as float32, z, order=1, mode="nearest") followed by numpy.round: output length round(L * z) (Python's round);
// input coordinate k * (L - 1) / (out - 1) in double, clamped to [0, L - 1]; linear weights (1 - t, t) summed in double from 0 in
// that order; the float32 result rounded half to even. False where the reference's assert (length == L * z) fails.
static inline bool feat_zoom_round(const std::vector<uint32_t>& xs, double z, std::vector<uint32_t>& out) {
  const size_t L = xs.size();
  const double want = (double)L * z;
  const double outn_d = nearbyint(want);
  if (outn_d != want || outn_d < 1.0 || outn_d > 1e6) return false;
  const size_t outn = (size_t)outn_d;
  const double zf = outn > 1 ? (double)(L - 1) / (double)(outn - 1) : 1.0;
  out.resize(outn);
  for (size_t k = 0; k < outn; ++k) {
    double cc = (double)k * zf;
    cc = std::min(std::max(cc, 0.0), (double)(L - 1));
    const double fl = floor(cc), t = cc - fl;
    const size_t i0 = (size_t)fl, i1 = std::min(i0 + 1, L - 1);
    double v = 0.0 + (1.0 - t) * (double)(float)xs[i0];
    v = v + t * (double)(float)xs[i1];
    const float r = nearbyintf((float)v);
    out[k] = r <= 0.f ? 0u : (uint32_t)r;
  }
  return true;
}

// Validates the spec against the setup (the constant block's header and host copy) and builds the gather table (FeatHeader, FeatFloor[], indices).
static inline int feat_build_table(const ConstHeader& H, const uint8_t* host_const, const vsyn_feature_spec* sp, std::vector<uint8_t>& out, const char** err) {
  if (!sp) return fail(err, VSYN_ERR_INVALID, "feature spec is NULL");
  const bool floor_kind = sp->kind == VSYN_FEAT_FLOOR_FINAL_YS || sp->kind == VSYN_FEAT_FLOOR_FINAL_YS_RENDERED;
  const bool res_kind = sp->kind == VSYN_FEAT_RESIDUE_YS || sp->kind == VSYN_FEAT_RESIDUE_YS_WITH_FLOOR;
  if (!floor_kind && !res_kind) return fail(err, VSYN_ERR_INVALID, "unknown feature kind %u", sp->kind);
  if (sp->output_dim == 0 || sp->output_dim > (1u << 20)) return fail(err, VSYN_ERR_INVALID, "output_dim %u out of range", sp->output_dim);
  const uint32_t floor_opts = VSYN_FEAT_INCLUDE_FLOOR_NUMBER | VSYN_FEAT_ONLY_BIGGEST_FLOOR | VSYN_FEAT_SORTED_XS | VSYN_FEAT_XS_FROM_BIGGEST_FLOOR |
                              VSYN_FEAT_FLOOR_ALWAYS_POSITIVE;
  const uint32_t res_opts = VSYN_FEAT_SORTED_XS | VSYN_FEAT_LOG1P_ABS_SPACE | VSYN_FEAT_IGNORE_XS | VSYN_FEAT_CLIP;
  if (sp->options & ~(floor_kind ? floor_opts : res_opts)) return fail(err, VSYN_ERR_INVALID, "feature options 0x%x do not apply to kind %u", sp->options, sp->kind);
  if ((sp->options & VSYN_FEAT_ONLY_BIGGEST_FLOOR) && (sp->options & VSYN_FEAT_INCLUDE_FLOOR_NUMBER))
    return fail(err, VSYN_ERR_INVALID, "only_biggest_floor excludes include_floor_number");
  if (res_kind && sp->upscale_xs_factor != 1.0) return fail(err, VSYN_ERR_INVALID, "upscale_xs_factor applies to the floor kinds only");
  if (!(sp->upscale_xs_factor > 0.0)) return fail(err, VSYN_ERR_INVALID, "upscale_xs_factor must be > 0");
  const FloorConst* fcs = (const FloorConst*)(host_const + H.off_floor);
  const uint32_t F = H.num_floors, D = sp->output_dim;
  uint32_t big = 0;
  for (uint32_t f = 1; f < F; ++f)
    if (fcs[f].posts > fcs[big].posts) big = f;  // the first of the largest (Python's max)
  const bool sorted = (sp->options & VSYN_FEAT_SORTED_XS) != 0;
  std::vector<std::vector<uint32_t>> xs(F), up(F);
  for (uint32_t f = 0; f < F; ++f) {
    xs[f].assign(fcs[f].xs, fcs[f].xs + fcs[f].posts);
    if (sorted) std::sort(xs[f].begin(), xs[f].end());
    if (floor_kind && sp->upscale_xs_factor != 1.0) {
      if (!feat_zoom_round(xs[f], sp->upscale_xs_factor, up[f]))
        return fail(err, VSYN_ERR_INVALID, "upscale_xs_factor %g: floor %u's %u posts do not zoom to a whole length (the reference asserts)",
                    sp->upscale_xs_factor, f, fcs[f].posts);
    } else {
      up[f] = xs[f];
    }
  }
  if (res_kind && !(sp->options & VSYN_FEAT_IGNORE_XS) && D < fcs[big].posts)
    return fail(err, VSYN_ERR_INVALID, "output_dim %u is below the biggest floor's %u posts: the reference asserts on such rows (use ignore_xs)", D,
                fcs[big].posts);
  FeatHeader T = {};
  T.kind = sp->kind;
  T.dim = D;
  T.opts = sp->options;
  T.big = big;
  T.num_floors = F;
  T.scale = sp->scale;
  T.clip = sp->clip_abs_max;
  T.fbf = sp->floor_base_factor;
  std::vector<FeatFloor> ff(F);
  std::vector<uint32_t> idx;
  const uint32_t o = (sp->options & VSYN_FEAT_INCLUDE_FLOOR_NUMBER) ? 1u : 0u;
  for (uint32_t f = 0; f < F; ++f) {
    std::vector<uint32_t> l;
    FeatFloor& e = ff[f];
    e.fnum = (float)(((double)f + 1.0) / (double)F - 0.5);
    if (sp->options & VSYN_FEAT_XS_FROM_BIGGEST_FLOOR) {
      l = up[big];
      if (f != big) {
        const double mb = (double)*std::max_element(xs[big].begin(), xs[big].end());
        const double mc = (double)*std::max_element(xs[f].begin(), xs[f].end());
        const double factor = nearbyint(mb / mc);  // Python's round() of the ratio (mc == 0: inf, no usable floor)
        for (uint32_t& v : l) v = (factor >= 1.0 && factor < 4294967296.0) ? (uint32_t)(v / (uint64_t)factor) : 0u;  // numpy: x // 0 == 0
      }
      e.clip = 1;
    }
    else l = up[f];
    e.maxidx = l.empty() ? 0u : *std::max_element(l.begin(), l.end());
    e.cnt = D > o ? (uint32_t)std::min<size_t>(l.size(), D - o) : 0u;
    e.off = (uint32_t)idx.size();
    idx.insert(idx.end(), l.begin(), l.begin() + e.cnt);
  }
  T.res_off = (uint32_t)idx.size();
  T.res_cnt = std::min<uint32_t>(fcs[big].posts, D);
  idx.insert(idx.end(), xs[big].begin(), xs[big].begin() + T.res_cnt);
  out.resize(sizeof(FeatHeader) + sizeof(FeatFloor) * F + sizeof(uint32_t) * (idx.size() + 1));
  memcpy(out.data(), &T, sizeof(T));
  memcpy(out.data() + sizeof(T), ff.data(), sizeof(FeatFloor) * F);
  memcpy(out.data() + sizeof(T) + sizeof(FeatFloor) * F, idx.data(), sizeof(uint32_t) * idx.size());
  return VSYN_OK;
}

// The count / offsets kernels (and, with rows != nullptr, the floor unwrap and the rows kernel) on stream s. Of the handle: the
// constant block (header, host copy, device copy), the status words and the floor unwrap's dynamic LDS. Caller holds the handle's lock.
static inline int feat_launch(FeatureWs& ws, int device, const ConstHeader& H, const uint8_t* host_const, const uint8_t* d_const,
                              DevStatus* d_status, uint32_t unwrap_lds_bytes, const vsyn_feature_spec* sp, uint32_t P, const vsyn_packet* d_pk, uint32_t S, const vsyn_segment* d_seg,
                       uint32_t max_seg, const uint16_t* d_ys, const float* d_res, float* d_rows, uint64_t* d_segoff, hipStream_t s,
                       const char** err) {
  std::vector<uint8_t> tab;
  int rc = feat_build_table(H, host_const, sp, tab, err);
  if (rc) return rc;
  if (S > 65535u) return fail(err, VSYN_ERR_INVALID, "too many segments (%u > 65535)", S);
  if (max_seg == 0 || max_seg > P) max_seg = P;
  const uint32_t C = H.channels;
  HIPCHK(hipSetDevice(device));
  HIPCHK(ws.info.ensure(P));
  HIPCHK(ws.fy.ensure((size_t)P * C * H.ys_stride));
  HIPCHK(ws.rowrel.ensure(P));
  HIPCHK(ws.fbsrc.ensure(P));
  HIPCHK(ws.fbch.ensure(P));
  HIPCHK(ws.resoff.ensure(P));
  HIPCHK(ws.segrows.ensure(S));
  HIPCHK(ws.segoff.ensure((size_t)S + 1));
  if (int rc = ws.tab.upload(tab, s, err)) return rc;
  if (P) HIPCHK(hipMemsetAsync(ws.info.p, 0, sizeof(PktInfo) * P, s));  // packets outside every segment: no floor rows to unwrap
  FeatCtx A;
  A.cb = d_const;
  A.tab = ws.tab.dev.p;
  A.pk = d_pk;
  A.seg = d_seg;
  A.fy = ws.fy.p;
  A.res = d_res;
  A.info = ws.info.p;
  A.rowrel = ws.rowrel.p;
  A.fbsrc = ws.fbsrc.p;
  A.fbch = ws.fbch.p;
  A.resoff = ws.resoff.p;
  A.segrows = ws.segrows.p;
  A.segoff = d_segoff ? d_segoff : ws.segoff.p;
  A.rows = d_rows;
  A.status = d_status;
  A.P = P;
  A.S = S;
  A.max_seg = max_seg;
  VSYN_LAUNCH(vsyn_feat_count_kernel, dim3(S), dim3(FEAT_THREADS), 0, s, A);
  VSYN_LAUNCH(vsyn_feat_offsets_kernel, dim3(1), dim3(FEAT_THREADS), 0, s, A);
  if (!d_rows || P == 0 || max_seg == 0) return VSYN_OK;  // (no packet: every segment is empty or flagged by the count kernel)
  const uint32_t rows = P * C;
  VSYN_LAUNCH(vsyn_floor_unwrap_kernel, dim3(std::min<uint32_t>((rows + UNWRAP_THREADS - 1) / UNWRAP_THREADS, 65535u)), dim3(UNWRAP_THREADS), unwrap_lds_bytes, s,
              d_const, P, (const PktInfo*)ws.info.p, d_ys, ws.fy.p, d_status);
  const uint64_t slots = (uint64_t)max_seg * C;
  const uint64_t gx = (slots + FEAT_ROW_WAVES - 1) / FEAT_ROW_WAVES;
  if (gx > 0x7FFFFFFFull) return fail(err, VSYN_ERR_INVALID, "segment too long");
  VSYN_LAUNCH(vsyn_feat_rows_kernel, dim3((uint32_t)gx, S), dim3(FEAT_ROW_WAVES * 64), 0, s, A);
  return VSYN_OK;
}
