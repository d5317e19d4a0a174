// vsyn_stretch.h — PCM effects: PCM already on the device time-stretched, and with a resampling behind the stretch pitch-shifted
// (librosa.effects.time_stretch / pitch_shift). Semantics: include/vorbis_synth_hip.h, "PCM stretch".
//
// No transform kernel of its own: the launches of four stages on one stream, always centred, on the mono downmix,
//   1. the complex rows (VSYN_SPEC_STFT): vsyn_spec_lin_fft_kernel (vsyn_spectral_lin.h), bit for bit what kind "stft" stores;
//   2. the stretched rows at each segment's rate: the three launches of vsyn_pv.h;
//   3. vsyn_istft_frames_kernel and vsyn_istft_ola_kernel without a mask to nearbyint(T / rate) samples (vsyn_istft.h);
//   4. with a shift, the resampler's launches from shift_from_hz[g] to shift_to_hz (vsyn_resample.h) in a workspace of this stage's;
// and, with VSYN_STRETCH_FIX_LENGTH, vsyn_stretch_deliver_kernel: each segment's first T samples, or all of them and zeros up to T.
// Both sets of rows pass through memory.
#pragma once
#include "vsyn_chroma.h"  // spec_launch
#include "vsyn_istft.h"
#include "vsyn_pv.h"
#include "vsyn_resample.h"

// dst[g][t] = t < have[g] ? src[g][t] : 0 for t < want[g]; want[g] to out_frames[g]. have and want: [S] each, have first.
__global__ void __launch_bounds__(256) vsyn_stretch_deliver_kernel(const float* src, uint64_t src_plane, const uint32_t* have_want, uint32_t S, float* dst,
                                                                   uint64_t dst_plane, uint32_t* out_frames) {
  const uint32_t g = blockIdx.y;
  const uint32_t have = have_want[g], want = have_want[S + g];
  if (out_frames && blockIdx.x == 0 && threadIdx.x == 0) out_frames[g] = want;
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (t >= want) return;
  dst[(size_t)g * dst_plane + t] = t < have ? src[(size_t)g * src_plane + t] : 0.f;
}

struct StretchWs {  // the stage's buffers
  TableUpload tab;             // each segment's frames, for the kernels that read them from the device
  DevBuf<float> rows, rows_out;  // [rows][n_fft / 2 + 1] complex64: the forward rows and the stretched ones
  DevBuf<float> mid, mid2;     // the stretched plane in front of the resampler; the plane in front of the length fix
  DevBuf<uint32_t> mid_frames;
  ResampleWs rs;               // the shift's resampler
  DevBuf<float> pcm;           // the mono plane of the stage inside a host chain
  DevBuf<uint32_t> frames;     // and its frames per segment
  DevBuf<int16_t> s16;
};

static inline vsyn_spectral_spec stretch_framing(const vsyn_pcm_stretch* e) {
  vsyn_spectral_spec f = {};
  f.kind = VSYN_SPEC_STFT;
  f.options = VSYN_SPEC_CENTER;
  f.n_fft = e->n_fft;
  f.hop_length = e->hop_length;
  f.win_length = e->win_length;
  return f;
}

// nearbyint(frames / rate), ties to even: Python's int(round(T / rate)). 0 for a rate the stage refuses; saturates.
static inline uint64_t stretch_num_samples(uint64_t frames, double rate) {
  if (!std::isfinite(rate) || !(rate > 0.0)) return 0;
  const double q = (double)frames / rate;
  double x = std::floor(q);
  const double d = q - x;  // exact
  if (d > 0.5 || (d == 0.5 && std::fmod(x, 2.0) != 0.0)) x += 1.0;
  return x < 18446744073709551616.0 ? (uint64_t)x : ~0ull;
}

// The checks of the spec.
static inline int stretch_check(const vsyn_pcm_stretch* e, const char** err) {
  if (!e) return fail(err, VSYN_ERR_INVALID, "stretch spec is NULL");
  const vsyn_spectral_spec f = stretch_framing(e);
  if (int rc = istft_check(&f, err)) return rc;
  if (e->options & ~VSYN_STRETCH_FIX_LENGTH) return fail(err, VSYN_ERR_INVALID, "stretch: unknown options 0x%x", e->options);
  if (e->reserved) return fail(err, VSYN_ERR_INVALID, "stretch: reserved must be 0");
  return VSYN_OK;
}

// What a segment of T frames has behind the stretch (*len), behind the shift (*res) and as delivered (returned). The caller has
// run stretch_check_call.
static inline uint64_t stretch_frames(const vsyn_pcm_stretch* e, uint64_t T, double rate, uint32_t from_hz, uint64_t* len, uint64_t* res) {
  *len = *res = stretch_num_samples(T, rate);
  uint32_t up, down;
  if (e->shift_to_hz && rs_ratio(from_hz, e->shift_to_hz, &up, &down)) *res = rs_num_frames(*len, up, down);
  return (e->options & VSYN_STRETCH_FIX_LENGTH) ? T : *res;
}

// The checks of a call's per-segment arrays: before anything runs.
static inline int stretch_check_call(const vsyn_pcm_stretch* e, uint32_t S, const double* rates, const uint32_t* from_hz, const char** err) {
  if (int rc = stretch_check(e, err)) return rc;
  if (S > 65535u) return fail(err, VSYN_ERR_INVALID, "too many segments (%u > 65535)", S);
  if (S && !rates) return fail(err, VSYN_ERR_INVALID, "stretch: rates is NULL");
  for (uint32_t g = 0; g < S; ++g)
    if (!std::isfinite(rates[g]) || !(rates[g] > 0.0)) return fail(err, VSYN_ERR_INVALID, "segment %u: stretch rate %g is not a finite number above 0", g, rates[g]);
  if (e->shift_to_hz) {
    if (S && !from_hz) return fail(err, VSYN_ERR_INVALID, "stretch: shift_from_hz is NULL with a shift_to_hz");
    for (uint32_t g = 0; g < S; ++g)
      if (!from_hz[g]) return fail(err, VSYN_ERR_INVALID, "segment %u: stretch: shift_from_hz must be >= 1", g);
    if (int rc = rs_check(S, from_hz, e->shift_to_hz, err)) return rc;
  }
  return VSYN_OK;
}

// The largest of what a segment of T frames has on its way through the stage: a plane of that many frames holds every step.
static inline uint64_t stretch_span(const vsyn_pcm_stretch* e, uint64_t T, double rate, uint32_t from_hz) {
  uint64_t len, res;
  const uint64_t out = stretch_frames(e, T, rate, from_hz, &len, &res);
  return std::max(std::max(T, out), std::max(len, res));
}

// The stage on stream s: d_pcm [S][C][plane], T[g] frames of segment g (host; at most plane), to the mono planes d_out
// [S][out_plane] and each segment's delivered frames to d_out_frames[g] (may be NULL). Caller holds the handle's lock and has run
// stretch_check_call.
static inline int stretch_launch(SpectralWs& sp, PvWs& pv, IstftWs& is, StretchWs& st, int device, const vsyn_pcm_stretch* e, uint32_t S, const uint64_t* T,
                                 const double* rates, const uint32_t* from_hz, const float* d_pcm, uint64_t plane, uint32_t C, float* d_out,
                                 uint64_t out_plane, uint32_t* d_out_frames, hipStream_t s, const char** err) {
  if (S == 0) return VSYN_OK;
  const vsyn_spectral_spec fr = stretch_framing(e);
  const uint32_t nb = fr.n_fft / 2u + 1u;
  const bool shift = e->shift_to_hz != 0, fix = (e->options & VSYN_STRETCH_FIX_LENGTH) != 0;
  std::vector<uint64_t> seg_rows(S), len(S), f_out;
  std::vector<uint32_t> on(S, 1u);
  std::vector<uint8_t> tab(sizeof(uint32_t) * 3u * (size_t)S);
  uint32_t* t_frames = (uint32_t*)tab.data();  // [S] the frames in, [S] what the deliver kernel copies, [S] what it delivers
  uint64_t f_max = 0, len_max = 0, res_max = 0, out_max = 0;
  for (uint32_t g = 0; g < S; ++g) {
    uint64_t res;
    const uint64_t out = stretch_frames(e, T[g], rates[g], shift ? from_hz[g] : 0u, &len[g], &res);
    if (T[g] > plane || T[g] > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "segment %u: %llu frames above the plane stride", g, (unsigned long long)T[g]);
    if (len[g] > 0xFFFFFFFFull || res > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "segment %u: stretched segment too long", g);
    if (out > out_plane)
      return fail(err, VSYN_ERR_INVALID, "segment %u: out_plane_stride %llu below its %llu frames", g, (unsigned long long)out_plane, (unsigned long long)out);
    seg_rows[g] = spec_num_frames(fr.n_fft, fr.hop_length, true, T[g]);
    t_frames[g] = (uint32_t)T[g];
    t_frames[S + g] = (uint32_t)std::min(res, T[g]);
    t_frames[2u * S + g] = (uint32_t)T[g];
    f_max = std::max(f_max, seg_rows[g]);
    len_max = std::max(len_max, len[g]);
    res_max = std::max(res_max, res);
    out_max = std::max(out_max, out);
  }
  if (out_plane > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "out_plane_stride must be below 2^32");
  uint64_t total, total_out;
  if (int rc = pv_check_call(&fr, S, seg_rows.data(), rates, f_out, &total, &total_out, err)) return rc;
  uint64_t fo_max = 0;
  for (uint32_t g = 0; g < S; ++g) fo_max = std::max(fo_max, f_out[g]);
  HIPCHK(hipSetDevice(device));
  HIPCHK(st.rows.ensure(2u * (total * nb + 1)));
  HIPCHK(st.rows_out.ensure(2u * (total_out * nb + 1)));
  if (int rc = st.tab.upload(tab, s, err)) return rc;
  const uint32_t* d_frames = (const uint32_t*)st.tab.dev.p;
  if (int rc = spec_launch(sp, device, &fr, S, on.data(), d_pcm, plane, C, d_frames, nullptr, f_max, total, st.rows.p, nullptr, s, err)) return rc;
  if (int rc = pv_launch(pv, device, &fr, S, seg_rows.data(), rates, f_out.data(), st.rows.p, st.rows_out.p, s, err)) return rc;
  // the inverse into the caller's plane, or into the plane in front of the resampler or the length fix
  float* inv = d_out;
  uint64_t inv_plane = out_plane;
  if (shift || fix) {
    inv_plane = std::max<uint64_t>(len_max, 1);
    HIPCHK(st.mid.ensure((size_t)S * inv_plane + 1));
    HIPCHK(st.mid_frames.ensure(S));
    inv = st.mid.p;
  }
  if (int rc = istft_launch(is, device, &fr, S, f_out.data(), len.data(), total_out, fo_max, len_max, st.rows_out.p, nullptr, inv, inv_plane,
                            shift || fix ? st.mid_frames.p : d_out_frames, s, err))
    return rc;
  const float* last = inv;
  uint64_t last_plane = inv_plane;
  if (shift) {
    float* res = d_out;
    uint64_t res_plane = out_plane;
    if (fix) {
      res_plane = std::max<uint64_t>(res_max, 1);
      HIPCHK(st.mid2.ensure((size_t)S * res_plane + 1));
      res = st.mid2.p;
    }
    if (int rc = rs_launch(st.rs, device, S, from_hz, e->shift_to_hz, inv, inv_plane, 1u, st.mid_frames.p, nullptr, res, res_plane,
                           fix ? nullptr : d_out_frames, s, err))
      return rc;
    last = res;
    last_plane = res_plane;
  }
  if (fix && (out_max || d_out_frames)) {
    const dim3 grid((uint32_t)std::max<uint64_t>((out_max + 255u) / 256u, 1), S);
    VSYN_LAUNCH(vsyn_stretch_deliver_kernel, grid, dim3(256), 0, s, last, last_plane, d_frames + S, S, d_out, out_plane, d_out_frames);
  }
  return VSYN_OK;
}
