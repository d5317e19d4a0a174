// CorpusDecoder.hpp — many Ogg Vorbis files, many host threads, one GPU  (BASELINE config 5 per GPU).
//
// The reference decodes one file on one thread, packet by packet (src/main.cpp:53-67 -> OggReader::full_read,
// src/ParseOggVorbis.hpp:1400-1409).  At corpus scale the sequential half (Ogg paging, Huffman / VQ entropy decode,
// hpp:1139-1211) is what bounds throughput, and it is independent per file.  So:
//
//   worker threads (T)   each takes the next file, runs the entropy half of the whole file (OggReader with a SynthSink that
//                        collects the PacketBatch instead of touching the GPU)
//   feeder threads (F)   each groups finished files that share a synthesis setup, packs up to `files_per_submit` of them into
//                        ONE C-ABI batch (one segment + one stream slot per file, VSYN_SEG_RESET each) in page-locked buffers
//                        and runs it on its own vsyn_handle; then delivers the PCM per file.  Handles own their HIP stream,
//                        so one feeder's PCIe copies overlap another's kernels and copies in the other direction.
//
// PCM delivery: CorpusCallbacks::gotFilePcm is called on a feeder thread (never two calls at the same time), once per file,
// in no particular file order, with planar channel views that are valid during the call only (the same lifetime rule as
// ParseCallbacks::gotPcmData).  Debug hooks (Callbacks.h) are not
// replayed on this path; use OggReader for that.
#ifndef PARSEOGGVORBIS_AMD_HOST_CORPUSDECODER_HPP_
#define PARSEOGGVORBIS_AMD_HOST_CORPUSDECODER_HPP_

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "ParseOggVorbis.hpp"

struct CorpusItem {  // one Ogg Vorbis file, in memory (the caller keeps it alive during decode_corpus)
  const uint8_t* data;
  size_t len;
};

struct CorpusFileResult {
  OkOrError status;
  uint32_t channels = 0, sample_rate = 0;
  uint32_t audio_packets = 0;
  uint64_t frames = 0;   // PCM frames (samples per channel) produced
  double abs_sum = 0;    // sum |x| over all channels, in double: a cheap content check that does not need the PCM kept
  uint64_t feature_rows = 0;  // CorpusOptions::features / spectral: rows delivered
  uint64_t trim_start = 0, trim_end = 0;  // CorpusOptions::trim: the samples kept, [trim_start, trim_end) of the (resampled) signal
  std::vector<uint32_t> intervals;        // CorpusOptions::split: (start, end) of every non-silent interval, in samples of that signal
  vsyn_loudness_record loudness = {0.0, 0.0, 0u, 0u, 0u, 0.0f, 0u, 0u};  // CorpusOptions::loudness: the file's record
  std::vector<double> loudness_blocks;    // ... and with loudness_blocks its block means z_j
  double bpm = 0;                         // CorpusOptions::beat: the tempo the beat period came from (0.0: no beats to take one from)
  double tuning = 0;                      // a tuning run: the estimate, in fractions of a bin of tuning.bins_per_octave
  uint64_t tuning_counts[2] = {0, 0};     // ... the peaks it was taken from, and those at or above their median magnitude
};

struct CorpusCallbacks {
  virtual ~CorpusCallbacks() {}
  // file_index = index into the items array. Return false to abort the whole run.
  virtual bool gotFilePcm(size_t file_index, const VorbisIdHeader& header, const std::vector<DataRange<const float>>& channelPcms) {
    (void)file_index; (void)header; (void)channelPcms;
    return true;
  }
  // CorpusOptions::pcm_s16: the file's PCM as interleaved host-endian int16 frames (ov_read's conversion, done on the device: half
  // the bytes cross the bus), valid during the call
  virtual bool gotFilePcmS16(size_t file_index, const VorbisIdHeader& header, const int16_t* interleaved, uint64_t frames) {
    (void)file_index; (void)header; (void)interleaved; (void)frames;
    return true;
  }
  // CorpusOptions::features / spectral: the file's feature matrix, num_rows x dim float32 row-major (include/vorbis_synth_hip.h,
  // "feature matrices" / "spectral features"), valid during the call. Called instead of gotFilePcm; a failed file gets no call.
  virtual bool gotFileFeatures(size_t file_index, const VorbisIdHeader& header, const float* rows, uint64_t num_rows, uint32_t dim) {
    (void)file_index; (void)header; (void)rows; (void)num_rows; (void)dim;
    return true;
  }
};

struct CorpusOptions {
  int threads = 0;                  // entropy workers; 0 = std::thread::hardware_concurrency()
  int feeders = 0;                  // GPU feeder threads; 0 = 3
  uint32_t files_per_submit = 64;   // stream slots per GPU submit
  uint32_t max_pending_files = 0;   // entropy-decoded files waiting for the GPU; 0 = 4 * files_per_submit
  int device = 0;                   // HIP ordinal
  bool entropy_only = false;        // diagnostic: run the workers only and count packets (no GPU call, no PCM, frames stay 0)
  bool share_setups = true;         // parse byte-identical setup headers once per run (SetupCache)
  bool checksum = true;             // fill CorpusFileResult::abs_sum (digest computed on the device, vsyn_pcm_abs_sum_host)
  bool pcm_s16 = false;             // deliver interleaved int16 (gotFilePcmS16) instead of planar f32 (SURVEY 8 f-3 on the host path)
  // feature run (features.kind != 0): each file's feature matrix from vsyn_features_host (gotFileFeatures), no synthesis, no PCM.
  // Residue kinds make the workers ship float residue (the VQ stage is off for them).
  vsyn_feature_spec features = {0, 0, 0, 0, 1.0, 1.0f, 0.0f, 1.0f, 0};
  // spectral run (spectral.kind != 0): synthesis as usual but VSYN_SUBMIT_KEEP_PCM, then each file's spectral rows from the PCM on
  // the device (vsyn_pcm_chain_rhythm_host), delivered through gotFileFeatures; no PCM crosses the bus. Excludes features / pcm_s16.
  vsyn_spectral_spec spectral = {0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0};
  // resample_rate != 0: the PCM (f32 or pcm_s16) and the spectral rows are those of each file's PCM resampled on the device from
  // its own rate to resample_rate (include/vorbis_synth_hip.h, "resampling"); frames and sample_rate in the results are the
  // resampled ones, and abs_sum is taken over the delivered f32 PCM (0 for pcm_s16). The mel table and the fmin / fmax check of a
  // spectral run use resample_rate. A file whose reduced ratio exceeds the limit fails alone. Not for feature runs.
  uint32_t resample_rate = 0;
  // spectral run with the post stage (post.order != 0 or post.norm != VSYN_POST_NORM_NONE): delta columns and mean / variance
  // normalisation of each file's rows on the device (include/vorbis_synth_hip.h, "spectral post-processing"); the rows delivered have
  // dim * (1 + order) columns. A file with fewer frames than the delta width fails alone. The default is off: today's rows.
  vsyn_spectral_post post = {0, 9, VSYN_POST_NORM_NONE, VSYN_POST_STATS_SEGMENT, 1e-5, nullptr, nullptr};
  // condition: each file's PCM (resampled first with resample_rate) goes through the conditioning stage on the device
  // (include/vorbis_synth_hip.h, "PCM conditioning": mono downmix, and per cond.options peak normalisation and pre-emphasis). A PCM
  // run then delivers ONE channel (gotFilePcm with one range; gotFilePcmS16 with mono frames whatever the header's channel count;
  // channels = 1 in the results, abs_sum over the delivered plane), a spectral run computes its rows from that plane. A file
  // whose peak is not finite fails alone. Not for feature runs. The default is off: today's output.
  bool condition = false;
  vsyn_pcm_cond cond = {0, 0, 0.0};
  // trim (needs condition: the output is the mono plane): the silent head and tail of each file's downmix are cut on the device in
  // front of the peak and the pre-emphasis (include/vorbis_synth_hip.h, "PCM trimming"). frames in the results are the trimmed
  // ones, trim_start / trim_end the samples kept; a spectral run computes its rows (and "fewer frames than the delta width") from
  // the trimmed plane. A file with a sample that is not finite fails alone. The default is off: today's output.
  bool trim = false;
  vsyn_pcm_trim trim_spec = {2048, 512, 60.0};
  // split (needs condition, excludes trim; its parameters are trim_spec's): every silent stretch of each file's downmix is removed on
  // the device, not the head and the tail alone (include/vorbis_synth_hip.h, "PCM splitting"). frames in the results are those of
  // the joined signal, intervals the non-silent intervals; a spectral run computes its rows from the joined plane. intervals_only
  // (a PCM run with split): the intervals alone; the joined signal is not made, no PCM is delivered, and frames are the unsplit
  // ones. A file with a sample that is not finite fails alone. The default is off: today's output.
  bool split = false, intervals_only = false;
  // pcen (a spectral run of kind mel_power or lin_power): each file's rows go through the PCEN stage on the device between the
  // spectral rows and the post stage (include/vorbis_synth_hip.h, "PCEN"); with pcen_spec.b = 0 the coefficient comes from the rate
  // the rows are computed at (resample_rate, else the file's own) and spectral.hop_length. A spec the stage refuses (another kind
  // among them) is every file's error. The default is off: the rows without the stage.
  bool pcen = false;
  vsyn_spectral_pcen pcen_spec = {0.98, 2.0, 0.5, 0.4, 1e-6, 0.0, 1.0};
  // pitch run (pitch.frame_length != 0): synthesis as usual but VSYN_SUBMIT_KEEP_PCM, then each file's (f0, normalised difference)
  // rows from the PCM on the device (include/vorbis_synth_hip.h, "pitch": vsyn_pcm_pitch_host, resampled first with resample_rate),
  // delivered through gotFileFeatures with dim 2; no PCM crosses the bus. A file whose rate the spec does not fit, and a file with
  // a sample that is not finite, fails alone. Excludes features, spectral, pcm_s16 and the conditioning, trim and split stages.
  vsyn_pitch_spec pitch = {0, 0, 0, 0, 0.0, 0.0, 0.0};
  // pYIN run (pyin.frame_length != 0): as a pitch run, but each file's (f0, voiced, voiced_prob) rows (include/vorbis_synth_hip.h,
  // "pyin": vsyn_pcm_pyin_host), delivered through gotFileFeatures with dim 3; pyin.threshold_probs must stay valid for the run. A
  // file whose rate the spec does not fit (an even transition width among the reasons) fails alone. Excludes what a pitch run
  // excludes, and pitch.
  vsyn_pyin_spec pyin = {0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, nullptr};
  // frame descriptor run (fdesc.n_fft != 0): as a pitch run, but each file's (rms, zcr, centroid, bandwidth, rolloff, flatness) rows
  // (include/vorbis_synth_hip.h, "frame descriptors": vsyn_pcm_fdesc_host), delivered through gotFileFeatures with dim 6. A file with
  // a sample that is not finite fails alone. Excludes what a pitch run excludes, and pitch.
  vsyn_fdesc_spec fdesc = {0, 0, 0, 0, 0.0, 0.0, 0.0};
  // constant-Q run (cqt.n_bins != 0): as a pitch run, but each file's constant-Q, chroma_cqt or tonnetz rows (include/vorbis_synth_hip.h,
  // "constant-Q": vsyn_pcm_cqt_host), delivered through gotFileFeatures with dim vsyn_cqt_dim(&cqt). A file with a sample that is not
  // finite, a file at whose rate the top bin leaves the Nyquist band and a file whose rate makes the wavelets longer than the stage's
  // caps fail alone, by name. Excludes what a pitch run excludes, pitch and fdesc.
  vsyn_cqt_spec cqt = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0};
  // cqt_estimate (a constant-Q run): each file's tuning is estimated first (vsyn_pcm_cqt_est_host with cqt_estimate_spec) and goes to
  // CorpusFileResult::tuning; cqt.tuning is not used.
  bool cqt_estimate = false;
  vsyn_tuning_spec cqt_estimate_spec = {0.0, 0.0, 0.0, 0.0, 0u, 0u};
  // tuning run (tuning.bins_per_octave != 0): as a pitch run, but each file's tuning estimate (include/vorbis_synth_hip.h, "tuning
  // estimation": vsyn_pcm_tuning_host on the STFT of tuning_framing, a lin_power spec) into CorpusFileResult::tuning and
  // tuning_counts; with tuning_rows also the file's piptrack rows, delivered through gotFileFeatures with dim 2 (n_fft / 2 + 1): a
  // row's pitches, then its magnitudes. Excludes what a pitch run excludes, pitch, fdesc and cqt.
  vsyn_spectral_spec tuning_framing = {0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0};
  vsyn_tuning_spec tuning = {0.0, 0.0, 0.0, 0.0, 0u, 0u};
  bool tuning_rows = false;
  // loudness run (loudness): as a pitch run, but each file's integrated loudness record (include/vorbis_synth_hip.h, "loudness":
  // vsyn_pcm_loudness_host, resampled first with resample_rate; loudness_spec.channel_mode picks the planes or their downmix) into
  // CorpusFileResult::loudness, and with loudness_blocks the block means into CorpusFileResult::loudness_blocks; nothing goes to the
  // callbacks and no PCM crosses the bus. A silent file is measured (status VSYN_LOUD_SILENT); a file that is too short, holds a
  // sample that is not finite or has a rate below 4000 Hz fails alone, by name. Excludes what a pitch run excludes, pitch and fdesc.
  // loudness_norm (a PCM run with condition, or a spectral run): each file's mono plane is normalised to loudness_spec.target on
  // the device between the gate and conditioning ("loudness", step 7: VSYN_LOUD_NORMALIZE, VSYN_LOUD_MONO; excludes VSYN_COND_PEAK);
  // the record goes to CorpusFileResult::loudness. A file the stage refuses, a silent one included, fails alone, by name. The
  // default is off: the output without the stage.
  bool loudness = false, loudness_blocks = false, loudness_norm = false;
  vsyn_loudness_spec loudness_spec = {0u, VSYN_LOUD_SUM, 0.0};
  // chroma_given (a spectral run of kind VSYN_SPEC_CHROMA or VSYN_SPEC_TONNETZ): the rows are computed with chroma_spec, else with
  // the default chroma parameters (include/vorbis_synth_hip.h, "chroma"). Another kind does not read them.
  bool chroma_given = false;
  vsyn_spectral_chroma chroma_spec = {12u, VSYN_CHROMA_NORM_MAX, VSYN_CHROMA_BASE_C, 0u, 0.0, 5.0, 2.0};
  // chroma_estimate (a spectral run of a chroma kind without hpss, rhythm or beat): each file's tuning is estimated first on the PCM
  // the chroma kernel sees (vsyn_pcm_chain_chroma_est_host) and goes to CorpusFileResult::tuning; chroma_spec.tuning is not used.
  bool chroma_estimate = false;
  vsyn_tuning_spec chroma_estimate_spec = {0.0, 0.0, 0.0, 0.0, 0u, 0u};
  // hpss (a spectral run of kind mel_power or lin_power): each file's rows go through the HPSS stage on the device between the
  // spectral rows and PCEN (include/vorbis_synth_hip.h, "HPSS"). A spec the stage refuses (another kind, or PCEN on the mask or the
  // median) is every file's error. The default is off: the rows without the stage.
  bool hpss = false;
  vsyn_spectral_hpss hpss_spec = {31u, 31u, VSYN_HPSS_HARMONIC, VSYN_HPSS_OUT_COMPONENT, 2.0, 1.0, 1.0};
  // effect (a PCM run with condition): each file's mono plane is replaced by its harmonic or percussive component on the device
  // between the gate and the loudness normaliser (include/vorbis_synth_hip.h, "PCM effects"). The default is off: the output
  // without the stage.
  bool effect = false;
  vsyn_pcm_effect effect_spec = {2048u, 512u, 2048u, 0u, {31u, 31u, VSYN_HPSS_HARMONIC, VSYN_HPSS_OUT_COMPONENT, 2.0, 1.0, 1.0}};
  // stretch (a PCM run with condition): each file's mono plane is time-stretched at its own rate, and with stretch_spec.shift_to_hz
  // resampled behind that (a pitch shift), in the effect's slot (include/vorbis_synth_hip.h, "PCM stretch"). stretch_rates and
  // stretch_from_hz (the latter only with a shift) hold one value per FILE of the call, indexed by the file's index, and must
  // outlive the run. The default is off: the output without the stage.
  bool stretch = false;
  vsyn_pcm_stretch stretch_spec = {2048u, 512u, 2048u, 0u, 0u, 0u};
  const double* stretch_rates = nullptr;
  const uint32_t* stretch_from_hz = nullptr;
  // rhythm (a spectral run of a kind with 1 to 256 columns): the rows stay on the device and go through the onset stage and what
  // rhythm_spec.output selects behind it (include/vorbis_synth_hip.h, "rhythm"); a file's "rows"
  // are then that output's words (1 column, win_length columns, or 2 for the mean's float64 values). A spec the stages refuse is
  // every file's error; an envelope that is not finite, or a window length outside [2, 2048], is that file's. The default is off.
  bool rhythm = false;
  vsyn_rhythm_spec rhythm_spec = {};
  // beat (a spectral run as for rhythm, which it excludes): the rows stay on the device and go through the onset stage (beat_onset)
  // and the beat tracker (include/vorbis_synth_hip.h, "rhythm", D; vsyn_pcm_chain_beats_host); a file's "rows" are its beat frames,
  // one uint32 word each. A non-finite envelope, a tempo window length outside [2, 2048] and a beat period outside [1, 2048] frames
  // are that file's errors. The default is off.
  bool beat = false;
  vsyn_onset_spec beat_onset = {};
  vsyn_beat_spec beat_spec = {};
};

struct CorpusStats {
  double wall_s = 0;
  double entropy_cpu_s = 0;   // summed over workers
  double gpu_call_s = 0;      // time inside vsyn_submit_host (PCIe both ways + kernels), summed over feeders
  double pack_s = 0;          // feeders: gathering batches into the submit buffers
  double deliver_s = 0;       // feeders: checksums + gotFilePcm
  uint64_t submits = 0, files = 0, audio_packets = 0, frames = 0;
  uint32_t handles = 0;       // distinct synthesis setups seen
  uint64_t setup_parses = 0, setup_reuses = 0;
};

// Decodes every item; results[i] belongs to items[i].  The returned status is an error only if the run itself could not
// proceed (no GPU, callback abort); per-file problems (corrupt file, unsupported stream) are reported in results[i].status
// and do not stop the other files.
OkOrError decode_corpus(const std::vector<CorpusItem>& items, const CorpusOptions& opts, CorpusCallbacks* callbacks,
                        std::vector<CorpusFileResult>& results, CorpusStats* stats);

extern "C" {
// C / ctypes form.  frames_out, abs_sum_out, ok_out: arrays of num_files (any may be NULL).  pcm_out (may be NULL): per file
// either NULL or a buffer of channels * pcm_capacity[i] floats that receives the planar PCM, channel c at c * pcm_capacity[i]
// (a file longer than its capacity is marked failed).  stats_out: 8 doubles {wall_s, entropy_cpu_s, gpu_call_s, pack_s,
// deliver_s, submits, audio_packets, frames} or NULL.
// Returns 0 if the run proceeded (look at ok_out per file), 1 otherwise with *error_out set as for ogg_vorbis_full_read.
int ogg_vorbis_decode_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                             uint32_t files_per_submit, int device, uint64_t* frames_out, double* abs_sum_out, uint8_t* ok_out, float* const* pcm_out,
                             const uint64_t* pcm_capacity, double* stats_out, const char** error_out);
// int16 output (CorpusOptions::pcm_s16): pcm16_out[i] = NULL or room for pcm_capacity_frames[i] interleaved frames
int ogg_vorbis_decode_corpus_s16(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                 uint32_t files_per_submit, int device, uint64_t* frames_out, uint8_t* ok_out, int16_t* const* pcm16_out,
                                 const uint64_t* pcm_capacity_frames, double* stats_out, const char** error_out);
// feature run (CorpusOptions::features = *spec), one pass: rows_out (may be NULL) receives per file NULL (failed, or no rows) or a
// buffer of rows_count_out[i] * spec->output_dim floats allocated by the library, to be released with ogg_vorbis_features_free.
// error_out_per_file (may be NULL): per file NULL or the file's error text, valid until the next call, on the same thread, of this
// function or of the spectral or PCM corpus functions below.
int ogg_vorbis_features_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                               uint32_t files_per_submit, int device, const vsyn_feature_spec* spec, float** rows_out,
                               uint64_t* rows_count_out, uint8_t* ok_out, const char** error_out_per_file,
                               double* stats_out, const char** error_out);
// spectral run (CorpusOptions::spectral = *spec), same output contract as ogg_vorbis_features_corpus (dim =
// vsyn_spectral_dim(spec): n_mfcc for MFCC, n_fft / 2 + 1 for LIN_POWER and LIN_DB, twice that for STFT, n_mels otherwise); rows
// released with ogg_vorbis_features_free. A file whose rate the spec does not fit fails alone (a linear kind fits every rate).
int ogg_vorbis_spectral_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                               uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, float** rows_out,
                               uint64_t* rows_count_out, uint8_t* ok_out, const char** error_out_per_file,
                               double* stats_out, const char** error_out);
// spectral run of the PCM resampled to target_rate (CorpusOptions::resample_rate; 0 = each file's own rate, as
// ogg_vorbis_spectral_corpus). Same output contract as ogg_vorbis_spectral_corpus.
int ogg_vorbis_spectral_corpus_sr(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                  uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, uint32_t target_rate,
                                  float** rows_out, uint64_t* rows_count_out, uint8_t* ok_out, const char** error_out_per_file,
                                  double* stats_out, const char** error_out);
// spectral run followed by the post stage (CorpusOptions::post = *post; target_rate as for ogg_vorbis_spectral_corpus_sr): rows of
// vsyn_spectral_post_dim(spec, post) columns. A file with 0 < frames < post->width (order > 0) fails alone. Same output contract.
int ogg_vorbis_spectral_corpus_post(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                    uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, uint32_t target_rate,
                                    const vsyn_spectral_post* post, float** rows_out, uint64_t* rows_count_out, uint8_t* ok_out,
                                    const char** error_out_per_file, double* stats_out, const char** error_out);
// PCM run: pcm_out (may be NULL) receives per file NULL (failed, or no frames) or a buffer allocated by the library, released
// with ogg_vorbis_features_free: format VSYN_PCM_F32 float32 planar [channels][frames], VSYN_PCM_S16 int16 interleaved
// [frames][channels]. target_rate: 0 = each file's own rate, else CorpusOptions::resample_rate. frames_out, channels_out and
// rate_out (any may be NULL) receive what was delivered; ok_out / error_out_per_file as for ogg_vorbis_features_corpus.
int ogg_vorbis_pcm_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                          uint32_t files_per_submit, int device, uint32_t target_rate, int format, void** pcm_out, uint64_t* frames_out,
                          uint32_t* channels_out, uint32_t* rate_out, uint8_t* ok_out, const char** error_out_per_file, double* stats_out,
                          const char** error_out);
// ogg_vorbis_pcm_corpus through the conditioning stage (CorpusOptions::cond = *cond): pcm_out receives ONE plane per file,
// float32 [frames] or int16 [frames], and channels_out 1. cond = NULL is ogg_vorbis_pcm_corpus.
int ogg_vorbis_pcm_corpus_cond(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                               uint32_t files_per_submit, int device, uint32_t target_rate, int format, const vsyn_pcm_cond* cond,
                               void** pcm_out, uint64_t* frames_out, uint32_t* channels_out, uint32_t* rate_out, uint8_t* ok_out,
                               const char** error_out_per_file, double* stats_out, const char** error_out);
// spectral run whose rows are computed from the conditioned plane: resample (target_rate != 0), condition (cond != NULL), spectral
// rows, post stage (post != NULL). cond = NULL is ogg_vorbis_spectral_corpus_post resp. ogg_vorbis_spectral_corpus_sr. A file whose
// peak is not finite (VSYN_COND_PEAK) fails alone. Same output contract.
int ogg_vorbis_spectral_corpus_cond(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                    uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, uint32_t target_rate,
                                    const vsyn_spectral_post* post, const vsyn_pcm_cond* cond, float** rows_out, uint64_t* rows_count_out,
                                    uint8_t* ok_out, const char** error_out_per_file, double* stats_out, const char** error_out);
// ogg_vorbis_pcm_corpus_cond with the trim in front of the conditioning (CorpusOptions::trim_spec = *trim): one mono plane per file,
// cond = NULL: the trimmed downmix as it is. bounds_out (may be NULL) receives per file (start, end), two uint64 each: the samples
// of the (resampled) signal that were kept; frames_out their count. trim = NULL is ogg_vorbis_pcm_corpus_cond (bounds_out: zeros).
int ogg_vorbis_pcm_corpus_trim(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                               uint32_t files_per_submit, int device, uint32_t target_rate, int format, const vsyn_pcm_cond* cond,
                               const vsyn_pcm_trim* trim, void** pcm_out, uint64_t* frames_out, uint32_t* channels_out, uint32_t* rate_out,
                               uint64_t* bounds_out, uint8_t* ok_out, const char** error_out_per_file, double* stats_out,
                               const char** error_out);
// ogg_vorbis_spectral_corpus_cond with the trim in it: resample, trim, condition (cond != NULL), spectral rows, post stage. A file
// trimmed to fewer frames than post->width (order > 0) fails alone. bounds_out as above. trim = NULL is
// ogg_vorbis_spectral_corpus_cond (bounds_out: zeros).
int ogg_vorbis_spectral_corpus_trim(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                    uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, uint32_t target_rate,
                                    const vsyn_spectral_post* post, const vsyn_pcm_cond* cond, const vsyn_pcm_trim* trim, float** rows_out,
                                    uint64_t* rows_count_out, uint64_t* bounds_out, uint8_t* ok_out, const char** error_out_per_file,
                                    double* stats_out, const char** error_out);
// ogg_vorbis_pcm_corpus_trim with the split in the trim's place (CorpusOptions::split): pcm_out receives each file's joined mono
// plane, frames_out its length. intervals_out (may be NULL) receives per file NULL (failed, or no intervals) or a buffer of
// intervals_count_out[i] (start, end) pairs of uint32 allocated by the library, released with ogg_vorbis_features_free. split =
// NULL is ogg_vorbis_pcm_corpus_cond (no intervals).
int ogg_vorbis_pcm_corpus_split(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                uint32_t files_per_submit, int device, uint32_t target_rate, int format, const vsyn_pcm_cond* cond,
                                const vsyn_pcm_trim* split, void** pcm_out, uint64_t* frames_out, uint32_t* channels_out, uint32_t* rate_out,
                                uint32_t** intervals_out, uint64_t* intervals_count_out, uint8_t* ok_out, const char** error_out_per_file,
                                double* stats_out, const char** error_out);
// ogg_vorbis_spectral_corpus_trim with the split in the trim's place: the rows of the joined plane. A file joined to fewer frames
// than post->width (order > 0) fails alone. frames_out (may be NULL): each file's joined length; intervals_out / intervals_count_out
// as above. split = NULL is ogg_vorbis_spectral_corpus_cond.
int ogg_vorbis_spectral_corpus_split(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                     uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, uint32_t target_rate,
                                     const vsyn_spectral_post* post, const vsyn_pcm_cond* cond, const vsyn_pcm_trim* split, float** rows_out,
                                     uint64_t* rows_count_out, uint64_t* frames_out, uint32_t** intervals_out, uint64_t* intervals_count_out,
                                     uint8_t* ok_out, const char** error_out_per_file, double* stats_out, const char** error_out);
// The spectral run with every stage's spec in one call: resample (target_rate != 0), the gate (gate != NULL: a trim, or with
// gate_is_split != 0 a split), condition (cond != NULL), spectral rows, PCEN (pcen != NULL: CorpusOptions::pcen_spec = *pcen), post
// stage (post != NULL). NULL means off. The outputs are those of ogg_vorbis_spectral_corpus_trim (bounds_out) and of
// ogg_vorbis_spectral_corpus_split (frames_out, intervals_out, intervals_count_out); each may be NULL, and those of the gate that is
// off are zeroed. A PCEN spec the stage refuses is every file's error. Same output contract.
int ogg_vorbis_spectral_corpus_pcen(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                    uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, uint32_t target_rate,
                                    const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post, const vsyn_pcm_cond* cond,
                                    const vsyn_pcm_trim* gate, int gate_is_split, float** rows_out, uint64_t* rows_count_out,
                                    uint64_t* bounds_out, uint64_t* frames_out, uint32_t** intervals_out, uint64_t* intervals_count_out,
                                    uint8_t* ok_out, const char** error_out_per_file, double* stats_out, const char** error_out);
// The loudness run (CorpusOptions::loudness): decode, resample (target_rate != 0), measure; no PCM comes back from the device.
// records_out[num_files] each file's record (zeros for a failed file); with want_blocks != 0 blocks_out[i] is a malloc'd array of
// blocks_count_out[i] block means (ogg_vorbis_features_free; NULL for none), else blocks_out may be NULL; frames_out / rate_out: each
// file's (resampled) length and rate. Same output contract.
int ogg_vorbis_loudness_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                               uint32_t files_per_submit, int device, uint32_t target_rate, const vsyn_loudness_spec* spec, int want_blocks,
                               double** blocks_out, uint64_t* blocks_count_out, vsyn_loudness_record* records_out, uint64_t* frames_out,
                               uint32_t* rate_out, uint8_t* ok_out, const char** error_out_per_file, double* stats_out, const char** error_out);
// The PCM run and the spectral run with every stage's spec in one call, the loudness normaliser among them (loud != NULL:
// CorpusOptions::loudness_norm; NULL means off, as for every other spec): the arguments of ogg_vorbis_pcm_corpus_trim / _split and of
// ogg_vorbis_spectral_corpus_pcen, the gate a trim or with gate_is_split != 0 a split, plus records_out[num_files] (may be NULL),
// each file's loudness record in front of the gain (zeros for a failed file). Same output contract.
int ogg_vorbis_pcm_corpus_loud(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                               uint32_t files_per_submit, int device, uint32_t target_rate, int format, const vsyn_pcm_cond* cond,
                               const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud, void** pcm_out, uint64_t* frames_out,
                               uint32_t* channels_out, uint32_t* rate_out, uint64_t* bounds_out, uint32_t** intervals_out,
                               uint64_t* intervals_count_out, vsyn_loudness_record* records_out, uint8_t* ok_out,
                               const char** error_out_per_file, double* stats_out, const char** error_out);
// ogg_vorbis_pcm_corpus_loud with the effect stage between the gate and the normaliser (effect != NULL: CorpusOptions::effect): one
// mono plane per file, the harmonic or the percussive component of its (resampled, gated) mono signal. effect = NULL is
// ogg_vorbis_pcm_corpus_loud, and with loud = NULL as well the entry that one is without a normaliser.
int ogg_vorbis_pcm_corpus_effects(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                  uint32_t files_per_submit, int device, uint32_t target_rate, int format, const vsyn_pcm_cond* cond,
                                  const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_pcm_effect* effect, const vsyn_loudness_spec* loud,
                                  void** pcm_out, uint64_t* frames_out, uint32_t* channels_out, uint32_t* rate_out, uint64_t* bounds_out,
                                  uint32_t** intervals_out, uint64_t* intervals_count_out, vsyn_loudness_record* records_out, uint8_t* ok_out,
                                  const char** error_out_per_file, double* stats_out, const char** error_out);
// ogg_vorbis_pcm_corpus_effects with the stretch stage in the effect's slot (stretch != NULL: CorpusOptions::stretch): one mono plane
// per file, time-stretched at stretch_rates[i] and, with stretch->shift_to_hz, resampled behind that from shift_from_hz[i] (both
// arrays hold one value per file of the call; shift_from_hz may be NULL without a shift). frames_out[i] is what the stage delivers.
// A spec, a rate or a resampling pair the stage refuses refuses the call by name before anything runs, as does an effect beside
// the stretch. stretch = NULL is ogg_vorbis_pcm_corpus_effects.
int ogg_vorbis_pcm_corpus_stretch(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                  uint32_t files_per_submit, int device, uint32_t target_rate, int format, const vsyn_pcm_cond* cond,
                                  const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_pcm_effect* effect, const vsyn_pcm_stretch* stretch,
                                  const double* stretch_rates, const uint32_t* shift_from_hz, const vsyn_loudness_spec* loud, void** pcm_out,
                                  uint64_t* frames_out, uint32_t* channels_out, uint32_t* rate_out, uint64_t* bounds_out, uint32_t** intervals_out,
                                  uint64_t* intervals_count_out, vsyn_loudness_record* records_out, uint8_t* ok_out,
                                  const char** error_out_per_file, double* stats_out, const char** error_out);
int ogg_vorbis_spectral_corpus_loud(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                    uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, uint32_t target_rate,
                                    const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post, const vsyn_pcm_cond* cond,
                                    const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud, float** rows_out,
                                    uint64_t* rows_count_out, uint64_t* bounds_out, uint64_t* frames_out, uint32_t** intervals_out,
                                    uint64_t* intervals_count_out, vsyn_loudness_record* records_out, uint8_t* ok_out,
                                    const char** error_out_per_file, double* stats_out, const char** error_out);
// ogg_vorbis_spectral_corpus_loud with every stage's spec NULL-able (loud = NULL: no normaliser, records_out zeroed) and the chroma
// parameters of the kinds VSYN_SPEC_CHROMA and VSYN_SPEC_TONNETZ (chroma = NULL: the defaults; not read for another kind): the rows
// are computed with them (CorpusOptions::chroma_given, chroma_spec), dim = vsyn_spectral_chroma_dim(spec, chroma), times
// 1 + post->order with the post stage. A chroma spec the stage refuses refuses the call. Same output contract.
int ogg_vorbis_spectral_corpus_chroma(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                      uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma,
                                      uint32_t target_rate, const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post,
                                      const vsyn_pcm_cond* cond, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud,
                                      float** rows_out, uint64_t* rows_count_out, uint64_t* bounds_out, uint64_t* frames_out,
                                      uint32_t** intervals_out, uint64_t* intervals_count_out, vsyn_loudness_record* records_out, uint8_t* ok_out,
                                      const char** error_out_per_file, double* stats_out, const char** error_out);
// ogg_vorbis_spectral_corpus_chroma with each file's tuning estimated first (estimate != NULL: CorpusOptions::chroma_estimate,
// chroma_estimate_spec; spec must be a chroma kind and estimate->bins_per_octave the chroma parameters' n_chroma): the rows are those
// of that entry called with the file's own estimate, which goes to tuning_out[i] (0.0 for a failed file); estimate = NULL is that
// entry and tuning_out is not written. A spec pair the estimator refuses refuses the call. Same output contract.
int ogg_vorbis_spectral_corpus_chroma_est(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                          uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec,
                                          const vsyn_spectral_chroma* chroma, uint32_t target_rate, const vsyn_spectral_pcen* pcen,
                                          const vsyn_spectral_post* post, const vsyn_pcm_cond* cond, const vsyn_pcm_trim* gate,
                                          int gate_is_split, const vsyn_loudness_spec* loud, const vsyn_tuning_spec* estimate,
                                          float** rows_out, uint64_t* rows_count_out, uint64_t* bounds_out, uint64_t* frames_out,
                                          uint32_t** intervals_out, uint64_t* intervals_count_out, vsyn_loudness_record* records_out,
                                          double* tuning_out, uint8_t* ok_out, const char** error_out_per_file, double* stats_out,
                                          const char** error_out);
// ogg_vorbis_spectral_corpus_chroma with the HPSS stage (hpss != NULL: CorpusOptions::hpss_spec = *hpss) between the spectral rows
// and PCEN; hpss = NULL is that entry. An HPSS spec the stage refuses is every file's error. Same output contract.
int ogg_vorbis_spectral_corpus_hpss(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                    uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma,
                                    uint32_t target_rate, const vsyn_spectral_hpss* hpss, const vsyn_spectral_pcen* pcen,
                                    const vsyn_spectral_post* post, const vsyn_pcm_cond* cond, const vsyn_pcm_trim* gate, int gate_is_split,
                                    const vsyn_loudness_spec* loud, float** rows_out, uint64_t* rows_count_out, uint64_t* bounds_out,
                                    uint64_t* frames_out, uint32_t** intervals_out, uint64_t* intervals_count_out,
                                    vsyn_loudness_record* records_out, uint8_t* ok_out, const char** error_out_per_file, double* stats_out,
                                    const char** error_out);
// ogg_vorbis_spectral_corpus_hpss with the rhythm stages behind PCEN (CorpusOptions::rhythm_spec = *rhythm, which must not be
// NULL), one entry for the four outputs rhythm->output selects: rows_out receives per file that output's words (see
// vsyn_rhythm_spec in include/vorbis_synth_hip.h) and rows_count_out its rows. A post spec that is on refuses the call.
// ogg_vorbis_rhythm_corpus with the beat tracker in the rhythm stages' place (CorpusOptions::beat_onset = *onset, beat_spec = *beat;
// neither may be NULL): rows_out receives per file its beat frames, uint32 words, rows_count_out their count, bpm_out (may be NULL)
// the tempo the period came from (beat->bpm, or the file's own estimate; 0.0 for a file without beats to take one from) and rate_out
// (may be NULL) the rate the rows were computed at. A post spec that is on refuses the call.
int ogg_vorbis_beats_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                            uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma,
                            uint32_t target_rate, const vsyn_spectral_hpss* hpss, const vsyn_spectral_pcen* pcen,
                            const vsyn_spectral_post* post, const vsyn_onset_spec* onset, const vsyn_beat_spec* beat, const vsyn_pcm_cond* cond,
                            const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud, float** rows_out,
                            uint64_t* rows_count_out, double* bpm_out, uint32_t* rate_out, uint64_t* bounds_out, uint64_t* frames_out,
                            uint32_t** intervals_out, uint64_t* intervals_count_out, vsyn_loudness_record* records_out, uint8_t* ok_out,
                            const char** error_out_per_file, double* stats_out, const char** error_out);
int ogg_vorbis_rhythm_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                             uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma,
                             uint32_t target_rate, const vsyn_spectral_hpss* hpss, const vsyn_spectral_pcen* pcen,
                             const vsyn_spectral_post* post, const vsyn_rhythm_spec* rhythm, const vsyn_pcm_cond* cond, const vsyn_pcm_trim* gate,
                             int gate_is_split, const vsyn_loudness_spec* loud, float** rows_out, uint64_t* rows_count_out, uint64_t* bounds_out,
                             uint64_t* frames_out, uint32_t** intervals_out, uint64_t* intervals_count_out, vsyn_loudness_record* records_out,
                             uint8_t* ok_out, const char** error_out_per_file, double* stats_out, const char** error_out);
// The intervals alone (CorpusOptions::intervals_only): decode, resample (target_rate != 0), frame energies, intervals; no PCM comes
// back from the device. frames_out / rate_out: each file's (resampled) length and rate; intervals_out / intervals_count_out as above.
int ogg_vorbis_intervals_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                uint32_t files_per_submit, int device, uint32_t target_rate, const vsyn_pcm_trim* split, uint32_t** intervals_out,
                                uint64_t* intervals_count_out, uint64_t* frames_out, uint32_t* rate_out, uint8_t* ok_out,
                                const char** error_out_per_file, double* stats_out, const char** error_out);
// pitch run (CorpusOptions::pitch = *spec; target_rate as for ogg_vorbis_spectral_corpus_sr): rows_out receives per file NULL
// (failed, or no rows) or a buffer of rows_count_out[i] * 2 floats, (f0 in Hz, normalised difference) per frame, released with
// ogg_vorbis_features_free. frames_out / rate_out: each file's (resampled) length and the rate its rows are computed at.
int ogg_vorbis_pitch_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                            uint32_t files_per_submit, int device, uint32_t target_rate, const vsyn_pitch_spec* spec, float** rows_out,
                            uint64_t* rows_count_out, uint64_t* frames_out, uint32_t* rate_out, uint8_t* ok_out,
                            const char** error_out_per_file, double* stats_out, const char** error_out);
// pYIN run (CorpusOptions::pyin = *spec; target_rate as for ogg_vorbis_pitch_corpus): rows_out receives per file NULL (failed, or
// no rows) or a buffer of rows_count_out[i] * 3 floats, (f0 in Hz, voiced, voiced_prob) per frame, released with
// ogg_vorbis_features_free. An invalid spec refuses the call before any file is touched.
int ogg_vorbis_pyin_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                           uint32_t files_per_submit, int device, uint32_t target_rate, const vsyn_pyin_spec* spec, float** rows_out,
                           uint64_t* rows_count_out, uint64_t* frames_out, uint32_t* rate_out, uint8_t* ok_out,
                           const char** error_out_per_file, double* stats_out, const char** error_out);
// frame descriptor run (CorpusOptions::fdesc = *spec; target_rate as for ogg_vorbis_pitch_corpus): rows_out receives per file NULL
// (failed, or no rows) or a buffer of rows_count_out[i] * 6 floats, (rms, zcr, centroid, bandwidth, rolloff, flatness) per frame,
// released with ogg_vorbis_features_free. An invalid spec refuses the call before any file is touched.
int ogg_vorbis_fdesc_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                            uint32_t files_per_submit, int device, uint32_t target_rate, const vsyn_fdesc_spec* spec, float** rows_out,
                            uint64_t* rows_count_out, uint64_t* frames_out, uint32_t* rate_out, uint8_t* ok_out,
                            const char** error_out_per_file, double* stats_out, const char** error_out);
// constant-Q run (CorpusOptions::cqt = *spec; target_rate as for ogg_vorbis_pitch_corpus): rows_out receives per file NULL (failed,
// or no rows) or a buffer of rows_count_out[i] * vsyn_cqt_dim(spec) floats, released with ogg_vorbis_features_free. An invalid spec
// refuses the call before any file is touched.
int ogg_vorbis_cqt_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                          uint32_t files_per_submit, int device, uint32_t target_rate, const vsyn_cqt_spec* spec, float** rows_out,
                          uint64_t* rows_count_out, uint64_t* frames_out, uint32_t* rate_out, uint8_t* ok_out,
                          const char** error_out_per_file, double* stats_out, const char** error_out);
// ogg_vorbis_cqt_corpus with each file's tuning estimated first (estimate != NULL: CorpusOptions::cqt_estimate, cqt_estimate_spec;
// estimate->bins_per_octave must be spec's): the rows are those of that entry called with the file's own estimate, which goes to
// tuning_out[i] (0.0 for a failed file); estimate = NULL is that entry and tuning_out is not written.
int ogg_vorbis_cqt_corpus_est(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                              uint32_t files_per_submit, int device, uint32_t target_rate, const vsyn_cqt_spec* spec,
                              const vsyn_tuning_spec* estimate, float** rows_out, uint64_t* rows_count_out, uint64_t* frames_out,
                              uint32_t* rate_out, double* tuning_out, uint8_t* ok_out, const char** error_out_per_file, double* stats_out,
                              const char** error_out);
// tuning run (CorpusOptions::tuning_framing = *spec, tuning = *tun, tuning_rows = want_rows != 0; target_rate as for
// ogg_vorbis_pitch_corpus): tuning_out[i] and counts_out[i][2] per file (0 for a failed file; either may be NULL), and with want_rows
// rows_out receives per file NULL or a buffer of rows_count_out[i] * 2 * (n_fft / 2 + 1) floats, released with
// ogg_vorbis_features_free. An invalid spec pair refuses the call.
int ogg_vorbis_tuning_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                             uint32_t files_per_submit, int device, uint32_t target_rate, const vsyn_spectral_spec* spec,
                             const vsyn_tuning_spec* tun, int want_rows, float** rows_out, uint64_t* rows_count_out, uint64_t* frames_out,
                             uint32_t* rate_out, double* tuning_out, uint64_t* counts_out, uint8_t* ok_out, const char** error_out_per_file,
                             double* stats_out, const char** error_out);
void ogg_vorbis_features_free(float* rows);
}

#endif
