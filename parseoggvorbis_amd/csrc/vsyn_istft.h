// vsyn_istft.h — the inverse STFT: complex rows (and an optional real mask) already on the device back to PCM. Semantics:
// include/vorbis_synth_hip.h, "inverse STFT". Design and measurements: DESIGN.md 6q.
//
// A frame kernel and the overlap-add kernel on one stream behind a table upload (the forward table of vsyn_spectral.h: header,
// twiddles, window; then one IstftSeg per segment):
//   vsyn_istft_frames_kernel  one workgroup of 256 threads per (segment, tile of frames), spec_lin_fft_tile's tile and the forward
//                             kernel's LDS image (spec_lin_fft_lds_floats). Per frame the inverse of vsyn_spec_lin_fft_kernel, pass
//                             for pass: the tangling pass builds the half-size spectrum Z[k] from Y[k] and conj Y[M - k] (Y = m X, one
//                             float32 product per component), the same radix-2 Stockham passes run with conjugated twiddles
//                             (frames_stockham<true> behind frames_stockham_twiddles, vsyn_frames.h: the one pass loop of both
//                             directions) between the same two LDS buffers, and z[m] = x[2m] + i x[2m+1]
//                             leaves as v[j] = w[j] * (x[j] / n_fft) into the frame workspace, [rows][n_fft] float32. A frame owns
//                             its M complex words: nothing of one frame enters another's sums.
//   vsyn_istft_masked_kernel  the frame kernel for a chain (vsyn_effects.h): the forward transform of the PCM by spec_lin_fft_tile_run, the
//                             mask applied while untangling, then the tangling pass and the rest in the same LDS; no rows are stored.
//   vsyn_istft_ola_kernel     a thread per output sample t: the frames that cover t in ascending f, their v and w^2 added in float64
//                             in the same walk, one division and one rounding to float32. Lanes run along t, so a frame's words are
//                             read at stride 1.
// No atomics; neither kernel's arithmetic depends on the grid, the tile or the segment's place in the batch. The rows and the mask
// are only read; nothing here touches stream state, the overlap carry or any synthesis buffer.
#pragma once
#include "vsyn_spectral_lin.h"

#define ISTFT_MAX_ROWS 0x3FFFFFFFu  // rows per segment

struct IstftSeg {
  uint64_t off;     // first row of the segment in the row buffers and the frame workspace
  uint32_t F, len;  // rows; output samples
};

struct IstftCtx {  // launch arguments
  const uint8_t* tab;   // spec_build_table's image
  const IstftSeg* seg;  // [S]
  const float2* rows;   // [rows][nbins]
  const float* mask;    // [rows][nbins], or NULL
  float* frames;        // [rows][n_fft]: the windowed frames
  float* out;           // [S][plane]
  uint64_t plane;
  uint32_t* out_frames;  // [S], or NULL
};

// Y[k] of one row: the bin times its mask value, a float32 product per component (the bin itself without a mask).
__device__ __forceinline__ float2 istft_bin(const float2* X, const float* m, uint32_t k) {
  const float2 x = X[k];
  if (!m) return x;
  const float mk = m[k];
  return make_float2(mk * x.x, mk * x.y);
}

// Z[k], k < M, of one frame from its bins a = Y[k] and b = Y[M - k]: Z = (a + conj b) + i w (a - conj b), w = exp(+2 pi i k / n) =
// (c, s). The halves of the forward untangling are left to the final 1 / n_fft. k = 0 reads the real parts of bins 0 and M alone.
__device__ __forceinline__ float2 istft_tangle(float2 a, float2 b, float2 w, uint32_t k) {
  if (k == 0u) a.y = b.y = 0.f;
  const float er = a.x + b.x, ei = a.y - b.y;
  const float dr = a.x - b.x, di = a.y + b.y;
  return make_float2(er - (w.x * di + w.y * dr), ei + (w.x * dr - w.y * di));
}

// v[2m], v[2m+1] = w * (z / n_fft) of the tile's nf frames into the workspace rows r0 ..; 0 outside the window's support.
__device__ __forceinline__ void istft_store(const SpecHeader* H, const float* g_win, const float2* z, float* frames, uint64_t r0, uint32_t nf,
                                            uint32_t lgM) {
  const uint32_t n = H->n, M = n >> 1, win = H->win, woff = H->woff;
  const float inv_n = 1.0f / (float)n;  // a power of two: exact
  for (uint32_t q = threadIdx.x; q < nf * M; q += SPEC_THREADS) {
    const uint32_t f = q >> lgM, m = q & (M - 1u), j = 2u * m;
    const float2 zz = z[q];
    float2 v = make_float2(0.f, 0.f);
    if (j >= woff && j - woff < win) v.x = g_win[j] * (zz.x * inv_n);
    if (j + 1u >= woff && j + 1u - woff < win) v.y = g_win[j + 1u] * (zz.y * inv_n);
    *(float2*)(frames + (r0 + f) * n + j) = v;
  }
}

__global__ void __launch_bounds__(SPEC_THREADS) vsyn_istft_frames_kernel(const IstftCtx A, const uint32_t ft, const uint32_t lgM) {
  extern __shared__ float lds[];
  const SpecHeader* H = spec_hdr(A.tab);
  const IstftSeg sg = A.seg[blockIdx.y];
  const uint32_t f0 = blockIdx.x * ft;
  if (f0 >= sg.F) return;
  const uint32_t nb = H->nbins, M = H->n >> 1;
  const uint32_t nf = min(ft, sg.F - f0);
  float2* s_st = (float2*)lds;
  float2* src = s_st + 2u * M + 1u;  // behind the forward image's untangling twiddles, which this kernel reads from the table
  float2* dst = src + (size_t)ft * M;
  const float2* g_tw = (const float2*)(A.tab + H->off_tw);
  frames_stockham_twiddles(g_tw, s_st, M, lgM);
  // the tangling pass reads its twiddle from the table, once per bin and at stride 1 along k
  const uint64_t r0 = sg.off + f0;
  for (uint32_t q = threadIdx.x; q < ft * M; q += SPEC_THREADS) {
    const uint32_t f = q >> lgM, k = q & (M - 1u);
    float2 Z = make_float2(0.f, 0.f);
    if (f < nf) {
      const float2* X = A.rows + (r0 + f) * nb;
      const float* m = A.mask ? A.mask + (r0 + f) * nb : nullptr;
      Z = istft_tangle(istft_bin(X, m, k), istft_bin(X, m, M - k), g_tw[k], k);
    }
    src[q] = Z;
  }
  frames_stockham<true>(s_st, src, dst, ft, 1u << lgM, lgM);
  istft_store(H, (const float*)(A.tab + H->off_win), src, A.frames, r0, nf, lgM);
}

// The frame kernel from the PCM, for a chain: the forward transform of vsyn_spec_lin_fft_kernel (spec_lin_fft_tile_run on P's PCM), the
// mask applied while untangling, then the tangling pass and the inverse in the same LDS. X is bit for bit what VSYN_SPEC_STFT
// stores, and everything behind it is the frame kernel's arithmetic: the complex bins never leave the workgroup.
__global__ void __launch_bounds__(SPEC_THREADS) vsyn_istft_masked_kernel(const SpecCtx P, const IstftCtx A, const uint32_t ft, const uint32_t lgM) {
  extern __shared__ float lds[];
  const SpecHeader* H = spec_hdr(A.tab);
  const uint32_t g = blockIdx.y;
  const IstftSeg sg = A.seg[g];
  const uint32_t f0 = blockIdx.x * ft;
  if (f0 >= sg.F) return;
  const uint32_t nb = H->nbins, M = H->n >> 1;
  const uint32_t nf = min(ft, sg.F - f0);
  const SpecLinFft T = spec_lin_fft_tile_run(P, H, lds, ft, lgM, g, f0, nf);
  const uint64_t r0 = sg.off + f0;
  for (uint32_t q = threadIdx.x; q < ft * M; q += SPEC_THREADS) {
    const uint32_t f = q >> lgM, k = q & (M - 1u);
    float2 Z = make_float2(0.f, 0.f);
    if (f < nf) {
      const float2* Zf = T.Z + (size_t)f * M;
      const float* m = A.mask + (r0 + f) * nb;
      float2 a, b;
      spec_lin_untangle(Zf, T.un, M, k, a.x, a.y);
      spec_lin_untangle(Zf, T.un, M, M - k, b.x, b.y);
      const float ma = m[k], mb = m[M - k];
      Z = istft_tangle(make_float2(ma * a.x, ma * a.y), make_float2(mb * b.x, mb * b.y), T.un[k], k);
    }
    T.spare[q] = Z;
  }
  float2 *src = T.spare, *dst = (float2*)T.Z;  // (Z is read out: its buffer is the passes' other one)
  frames_stockham<true>((const float2*)lds, src, dst, ft, 1u << lgM, lgM);
  istft_store(H, (const float*)(A.tab + H->off_win), src, A.frames, r0, nf, lgM);
}

// y[t] = (sum_f v_f[t + pad - f hop]) / W[t], W[t] = sum_f w[t + pad - f hop]^2 over the frames whose window support holds t, f
// ascending, both sums in float64 from 0.0; undivided where W <= FLT_MIN; 0 where no frame covers t.
__global__ void __launch_bounds__(SPEC_THREADS) vsyn_istft_ola_kernel(const IstftCtx A) {
  const SpecHeader* H = spec_hdr(A.tab);
  const uint32_t g = blockIdx.y;
  const IstftSeg sg = A.seg[g];
  if (A.out_frames && blockIdx.x == 0 && threadIdx.x == 0) A.out_frames[g] = sg.len;
  const uint64_t t = (uint64_t)blockIdx.x * SPEC_THREADS + threadIdx.x;
  if (t >= sg.len) return;
  const uint32_t n = H->n, hop = H->hop, win = H->win, woff = H->woff;
  const float* g_win = (const float*)(A.tab + H->off_win);
  // frame f holds t at j = q - f hop when woff <= j < woff + win
  const int64_t q = (int64_t)t + ((H->opts & VSYN_SPEC_CENTER) ? (int64_t)(n / 2u) : 0) - (int64_t)woff;
  double acc = 0.0, W = 0.0;
  if (q >= 0 && sg.F) {
    const int64_t lo = q >= (int64_t)win ? (q - (int64_t)win) / (int64_t)hop + 1 : 0;
    const int64_t last = (int64_t)sg.F - 1, hi = q / (int64_t)hop < last ? q / (int64_t)hop : last;
    for (int64_t f = lo; f <= hi; ++f) {
      const uint32_t j = (uint32_t)(q - f * (int64_t)hop) + woff;
      const float w = g_win[j];
      acc += (double)A.frames[(sg.off + (uint64_t)f) * n + j];
      W += (double)w * (double)w;
    }
  }
  A.out[(size_t)g * A.plane + t] = (float)(W > (double)1.17549435e-38f ? acc / W : acc);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct IstftWs {  // the stage's buffers
  TableUpload tab;
  DevBuf<float> frames;  // [rows][n_fft]
  bool lds_set = false;  // the frame kernels' dynamic-LDS limit is raised on this handle's device
};

// The framing of sp as the forward STFT kind reads it: n_fft, hop_length, win_length and the centre option; nothing else of sp is read.
static inline vsyn_spectral_spec istft_framing(const vsyn_spectral_spec* sp) {
  vsyn_spectral_spec f = {};
  f.kind = VSYN_SPEC_STFT;
  f.n_fft = sp->n_fft;
  f.hop_length = sp->hop_length;
  f.win_length = sp->win_length;
  f.options = sp->options & VSYN_SPEC_CENTER;
  return f;
}

// The checks of the spec that need no rows.
static inline int istft_check(const vsyn_spectral_spec* sp, const char** err) {
  if (!sp) return fail(err, VSYN_ERR_INVALID, "spectral spec is NULL");
  const vsyn_spectral_spec f = istft_framing(sp);
  if (int rc = spec_check(&f, 0, nullptr, err)) return rc;
  if (!spec_lin_pow2(f.n_fft))
    return fail(err, VSYN_ERR_INVALID, "istft: n_fft %u is not a power of two (the inverse of the direct-DFT path is not built)", f.n_fft);
  return VSYN_OK;
}

// Samples the rows of a segment cover: librosa.istft's length for length = None.
static inline uint64_t istft_num_samples(const vsyn_spectral_spec* sp, uint64_t rows) {
  if (!rows) return 0;
  return (uint64_t)sp->hop_length * (rows - 1u) + ((sp->options & VSYN_SPEC_CENTER) ? 0u : sp->n_fft);
}

// The checks of a call; fills len[S] (lengths, or what the rows cover) and the totals.
static inline int istft_check_call(const vsyn_spectral_spec* sp, uint32_t S, const uint64_t* seg_rows, const uint64_t* lengths, uint64_t plane,
                                   std::vector<uint64_t>& len, uint64_t* total_rows, uint64_t* f_max, uint64_t* len_max, const char** err) {
  if (int rc = istft_check(sp, err)) return rc;
  if (S && !seg_rows) return fail(err, VSYN_ERR_INVALID, "seg_rows is NULL");
  if (S > 65535u) return fail(err, VSYN_ERR_INVALID, "too many segments (%u > 65535)", S);
  if (plane > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "out_plane_stride must be below 2^32");
  len.assign(S, 0);
  *total_rows = *f_max = *len_max = 0;
  for (uint32_t g = 0; g < S; ++g) {
    if (seg_rows[g] > ISTFT_MAX_ROWS) return fail(err, VSYN_ERR_INVALID, "segment %u: too many rows", g);
    len[g] = lengths ? lengths[g] : istft_num_samples(sp, seg_rows[g]);
    if (len[g] > plane)
      return fail(err, VSYN_ERR_INVALID, "segment %u: out_plane_stride %llu below its %llu samples", g, (unsigned long long)plane, (unsigned long long)len[g]);
    *total_rows += seg_rows[g];
    *f_max = std::max(*f_max, seg_rows[g]);
    *len_max = std::max(*len_max, len[g]);
  }
  return VSYN_OK;
}

// The stage's kernels on stream s. Caller holds the handle's lock and has run istft_check_call (len, total_rows, f_max, len_max are
// its results) and the checks of its pointers. fwd != NULL: the masked variant from fwd's PCM (its pcm, plane, C and frames are read;
// seg_rows are then the centred frame counts of those frames) under d_mask, and d_rows is not read.
static inline int istft_launch(IstftWs& ws, int device, const vsyn_spectral_spec* sp, uint32_t S, const uint64_t* seg_rows, const uint64_t* len,
                               uint64_t total_rows, uint64_t f_max, uint64_t len_max, const float* d_rows, const float* d_mask, float* d_out,
                               uint64_t plane, uint32_t* d_out_frames, hipStream_t s, const char** err, const SpecCtx* fwd = nullptr) {
  if (S == 0 || (len_max == 0 && !d_out_frames)) return VSYN_OK;
  const vsyn_spectral_spec fr = istft_framing(sp);
  const uint32_t n = fr.n_fft, ft = spec_lin_fft_tile(n);
  const uint64_t gx = (f_max + ft - 1) / ft;
  if (gx > 0x7FFFFFFFull) return fail(err, VSYN_ERR_INVALID, "segment too long");
  std::vector<uint8_t> tab;
  spec_build_table(&fr, 0, nullptr, tab);
  const size_t off_seg = align_up(tab.size(), 16);
  tab.resize(off_seg + sizeof(IstftSeg) * (size_t)S);
  IstftSeg* seg = (IstftSeg*)(tab.data() + off_seg);
  uint64_t rows = 0;
  for (uint32_t g = 0; g < S; ++g) {
    seg[g] = IstftSeg{rows, (uint32_t)seg_rows[g], (uint32_t)len[g]};
    rows += seg_rows[g];
  }
  HIPCHK(hipSetDevice(device));
  if (int rc = raise_lds_once(ws.lds_set, {{(const void*)vsyn_istft_frames_kernel, SPEC_LDS_BUDGET}, {(const void*)vsyn_istft_masked_kernel, SPEC_LDS_BUDGET}}, err))
    return rc;
  HIPCHK(ws.frames.ensure(total_rows * n + 1));
  if (int rc = ws.tab.upload(tab, s, err)) return rc;
  IstftCtx A;
  A.tab = ws.tab.dev.p;
  A.seg = (const IstftSeg*)(ws.tab.dev.p + off_seg);
  A.rows = (const float2*)d_rows;
  A.mask = d_mask;
  A.frames = ws.frames.p;
  A.out = d_out;
  A.plane = plane;
  A.out_frames = d_out_frames;
  if (f_max && len_max) {
    const uint32_t lgM = spec_lin_lgm(n);
    const size_t lds = spec_lin_fft_lds_floats(ft, n) * 4u;
    if (fwd) {
      SpecCtx P = *fwd;
      P.tab = A.tab;
      VSYN_LAUNCH(vsyn_istft_masked_kernel, dim3((uint32_t)gx, S), dim3(SPEC_THREADS), lds, s, P, A, ft, lgM);
    } else {
      VSYN_LAUNCH(vsyn_istft_frames_kernel, dim3((uint32_t)gx, S), dim3(SPEC_THREADS), lds, s, A, ft, lgM);
    }
  }
  const uint64_t ox = std::max<uint64_t>((len_max + SPEC_THREADS - 1) / SPEC_THREADS, 1);
  VSYN_LAUNCH(vsyn_istft_ola_kernel, dim3((uint32_t)ox, S), dim3(SPEC_THREADS), 0, s, A);
  return VSYN_OK;
}
