// vsyn_effects.h — PCM effects: the harmonic or the percussive component of PCM already on the device, as PCM
// (librosa.effects.harmonic / percussive). Semantics: include/vorbis_synth_hip.h, "PCM effects".
//
// No kernel of its own: four launches of three stages on one stream, always centred,
//   1. |X| rows (VSYN_SPEC_LIN_POWER, power 1) of the mono downmix: vsyn_spec_lin_fft_kernel (vsyn_spectral_lin.h);
//   2. their soft mask (VSYN_HPSS_OUT_MASK): vsyn_hpss_kernel (vsyn_hpss.h);
//   3. vsyn_istft_masked_kernel on the same PCM under that mask, and vsyn_istft_ola_kernel to each segment's own length (vsyn_istft.h).
// The complex bins are never stored: step 3 recomputes the forward transform in the workgroup that inverts it.
#pragma once
#include "vsyn_chroma.h"  // spec_launch
#include "vsyn_hpss.h"
#include "vsyn_istft.h"

struct EffectWs {  // the stage's buffers
  TableUpload tab;           // each segment's frames, for the kernels that read them from the device
  DevBuf<float> mag, mask;   // [rows][n_fft / 2 + 1]
  DevBuf<float> pcm;         // the mono plane of the stage inside a host chain
  DevBuf<uint32_t> frames;   // and its frames per segment
  DevBuf<int16_t> s16;
};

static inline vsyn_spectral_spec effect_framing(const vsyn_pcm_effect* e) {
  vsyn_spectral_spec f = {};
  f.kind = VSYN_SPEC_STFT;
  f.options = VSYN_SPEC_CENTER;
  f.n_fft = e->n_fft;
  f.hop_length = e->hop_length;
  f.win_length = e->win_length;
  return f;
}

// The checks of the spec.
static inline int effect_check(const vsyn_pcm_effect* e, const char** err) {
  if (!e) return fail(err, VSYN_ERR_INVALID, "effect spec is NULL");
  const vsyn_spectral_spec f = effect_framing(e);
  if (int rc = istft_check(&f, err)) return rc;
  if (int rc = hpss_check(&e->hpss, err)) return rc;
  if (e->hpss.output != VSYN_HPSS_OUT_COMPONENT)
    return fail(err, VSYN_ERR_INVALID, "effect: hpss.output must be the component, not the %s", e->hpss.output == VSYN_HPSS_OUT_MASK ? "mask" : "median");
  return VSYN_OK;
}

// The stage on stream s: d_pcm [S][C][plane], T[g] frames of segment g (host; at most plane and out_plane), to the mono planes d_out
// [S][out_plane], exactly T[g] samples each, and T[g] to d_out_frames[g]. rates (may be NULL): a segment with rates[g] = 0 is not
// read and gets T[g] zeros. Caller holds the handle's lock and has run effect_check.
static inline int effect_launch(SpectralWs& sp, HpssWs& hp, IstftWs& is, EffectWs& ef, int device, const vsyn_pcm_effect* e, uint32_t S,
                                const uint64_t* T, const uint32_t* rates, const float* d_pcm, uint64_t plane, uint32_t C, float* d_out,
                                uint64_t out_plane, uint32_t* d_out_frames, hipStream_t s, const char** err) {
  if (S == 0) return VSYN_OK;
  if (S > 65535u) return fail(err, VSYN_ERR_INVALID, "too many segments (%u > 65535)", S);
  vsyn_spectral_spec fr = effect_framing(e);
  const uint32_t nb = fr.n_fft / 2u + 1u;
  std::vector<uint64_t> seg_rows(S), len(T, T + S);
  std::vector<uint32_t> on(S, 1u);
  std::vector<uint8_t> tab(sizeof(uint32_t) * (size_t)S);
  uint64_t total = 0, f_max = 0, len_max = 0;
  for (uint32_t g = 0; g < S; ++g) {
    if (T[g] > plane || T[g] > out_plane || T[g] > 0xFFFFFFFFull)
      return fail(err, VSYN_ERR_INVALID, "segment %u: %llu frames above a plane stride", g, (unsigned long long)T[g]);
    if (rates) on[g] = rates[g];
    seg_rows[g] = on[g] ? spec_num_frames(fr.n_fft, fr.hop_length, true, T[g]) : 0;
    ((uint32_t*)tab.data())[g] = (uint32_t)T[g];
    total += seg_rows[g];
    f_max = std::max(f_max, seg_rows[g]);
    len_max = std::max(len_max, len[g]);
  }
  vsyn_spectral_hpss mk = e->hpss;
  mk.output = VSYN_HPSS_OUT_MASK;
  if (int rc = hpss_check_call(&mk, nb, S, seg_rows.data(), err)) return rc;
  HIPCHK(hipSetDevice(device));
  HIPCHK(ef.mag.ensure(total * nb + 1));
  HIPCHK(ef.mask.ensure(total * nb + 1));
  if (int rc = ef.tab.upload(tab, s, err)) return rc;
  const uint32_t* d_frames = (const uint32_t*)ef.tab.dev.p;
  vsyn_spectral_spec mag = fr;
  mag.kind = VSYN_SPEC_LIN_POWER;
  mag.power = 1;
  if (int rc = spec_launch(sp, device, &mag, S, on.data(), d_pcm, plane, C, d_frames, nullptr, f_max, total, ef.mag.p, nullptr, s, err)) return rc;
  if (int rc = hpss_launch(hp, device, &mk, nb, S, seg_rows.data(), on.data(), ef.mag.p, ef.mask.p, s, err)) return rc;
  SpecCtx P = {};
  P.pcm = d_pcm;
  P.plane = plane;
  P.C = C;
  P.S = S;
  P.frames = d_frames;
  return istft_launch(is, device, &fr, S, seg_rows.data(), len.data(), total, f_max, len_max, nullptr, ef.mask.p, d_out, out_plane, d_out_frames, s, err,
                      &P);
}
