// CorpusDecoder.cpp — see CorpusDecoder.hpp.
#include "CorpusDecoder.hpp"

#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <map>
#include <mutex>
#include <numeric>
#include <thread>

namespace {

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// One file after the entropy half.
struct FileRecord {
  void recycle() {  // keep the vectors' capacity: fresh multi-MB allocations per file serialise the workers in the kernel's mm
    status = OkOrError();
    batch.pk.clear();
    batch.ys.clear();
    batch.residue.clear();
    batch.floor_number.clear();
    batch.vq_pk.clear();
    batch.cls.clear();
    batch.entries.clear();
    batch.vq = false;
    batch.residue_floats = 0;
    batch.first = true;
    ys_stride = 0;
    has_audio = false;
    synth = SynthSetup();
  }
  size_t index = 0;
  OkOrError status;
  VorbisIdHeader header;
  SynthSetup synth;
  PacketBatch batch;
  uint32_t ys_stride = 0;
  bool has_audio = false;
};

// Collects the (single) batch of the (single) logical stream of one file.
struct CollectSink : SynthSink {
  FileRecord& rec;
  const VorbisStream* owner = nullptr;
  explicit CollectSink(FileRecord& r) : rec(r) {}
  void prepare(VorbisStream& st) override {  // lend the record's (recycled, capacity-keeping) vectors to the first stream
    if (owner) return;
    owner = &st;
    st.pk_.swap(rec.batch.pk);
    st.ys_.swap(rec.batch.ys);
    st.residue_.swap(rec.batch.residue);
    st.floor_number_.swap(rec.batch.floor_number);
    st.vq_pk_.swap(rec.batch.vq_pk);
    st.cls_.swap(rec.batch.cls);
    st.entries_.swap(rec.batch.entries);
  }
  OkOrError consume(VorbisStream& st, PacketBatch&& b) override {
    if (owner && owner != &st) return OkOrError("corpus path: files with more than one logical Vorbis stream are not supported");
    if (rec.has_audio) return OkOrError("corpus path: stream delivered in more than one batch");
    owner = &st;
    rec.header = st.header;
    rec.ys_stride = st.ys_stride_;
    CHECK_ERR(build_synth_setup(st, rec.synth));
    rec.batch = std::move(b);
    rec.has_audio = true;
    return OkOrError();
  }
};

struct NullCallbacks : ParseCallbacks {};

// The loudness record of a file that has none: the stage is off, or the file failed.
const vsyn_loudness_record NO_LOUDNESS_RECORD = vsyn_loudness_record{0.0, 0.0, 0u, 0u, 0u, 0.0f, 0u, 0u};

bool feature_run(const CorpusOptions& o) { return o.features.kind != 0; }
bool spectral_run(const CorpusOptions& o) { return o.spectral.kind != 0; }
bool pitch_run(const CorpusOptions& o) { return o.pitch.frame_length != 0; }
bool pyin_run(const CorpusOptions& o) { return o.pyin.frame_length != 0; }
bool fdesc_run(const CorpusOptions& o) { return o.fdesc.n_fft != 0; }
bool cqt_run(const CorpusOptions& o) { return o.cqt.n_bins != 0; }
bool tuning_run(const CorpusOptions& o) { return o.tuning.bins_per_octave != 0; }
bool loudness_run(const CorpusOptions& o) { return o.loudness; }
bool post_run(const CorpusOptions& o) { return o.post.order != 0 || o.post.norm != VSYN_POST_NORM_NONE; }
// columns of a spectral run's rows: the kind's dim, times 1 + the delta orders
uint32_t spectral_dim(const CorpusOptions& o) {
  if (o.beat) return 1u;  // a beat frame a row
  if (o.rhythm)  // the words of a row of the selected rhythm output
    return o.rhythm_spec.output == VSYN_RHYTHM_TEMPOGRAM ? o.rhythm_spec.tempogram.win_length : o.rhythm_spec.output == VSYN_RHYTHM_TEMPO_MEAN ? 2u : 1u;
  return vsyn_spectral_chroma_dim(&o.spectral, o.chroma_given ? &o.chroma_spec : nullptr) * (1u + o.post.order);
}
bool feature_needs_residue(const CorpusOptions& o) {
  return o.features.kind == VSYN_FEAT_RESIDUE_YS || o.features.kind == VSYN_FEAT_RESIDUE_YS_WITH_FLOOR;
}

void entropy_decode_file(const CorpusItem& item, FileRecord& rec, SetupCache* cache, bool no_vq) {
  NullCallbacks cb;
  CollectSink sink(rec);
  OggReader reader(cb);
  reader.sink_ = &sink;
  reader.no_vq_ = no_vq;
  reader.setup_cache_ = cache;
  reader.batch_limit_override_ = 0xffffffffu;  // the whole file is one batch; it is cut into runs on the GPU
  rec.status = reader.full_read_from_memory(item.data, item.len);
  if (rec.status.is_error_)  // keep what was decoded before the failure, as the reference's gotPcmData calls would have
    for (auto& kv : reader.streams_) {
      const OkOrError r = kv.second->flush(cb);
      if (r.is_error_) break;
    }
}

// Bounded hand-off between the workers and the feeder.
struct RecordQueue {
  std::mutex mu;
  std::condition_variable not_empty, not_full;
  std::deque<std::unique_ptr<FileRecord>> q;
  std::vector<std::unique_ptr<FileRecord>> free_list;
  size_t cap;
  size_t producers;
  bool aborted = false;
  RecordQueue(size_t cap_, size_t producers_) : cap(cap_), producers(producers_) {}
  bool push(std::unique_ptr<FileRecord> r) {
    std::unique_lock<std::mutex> lk(mu);
    not_full.wait(lk, [&] { return q.size() < cap || aborted; });
    if (aborted) return false;
    q.push_back(std::move(r));
    not_empty.notify_one();
    return true;
  }
  std::unique_ptr<FileRecord> fresh() {
    {
      std::lock_guard<std::mutex> lk(mu);
      if (!free_list.empty()) {
        std::unique_ptr<FileRecord> r = std::move(free_list.back());
        free_list.pop_back();
        return r;
      }
    }
    return std::unique_ptr<FileRecord>(new FileRecord());
  }
  void give_back(std::unique_ptr<FileRecord> r) {
    r->recycle();
    std::lock_guard<std::mutex> lk(mu);
    free_list.push_back(std::move(r));
  }
  void producer_done() {
    std::lock_guard<std::mutex> lk(mu);
    --producers;
    not_empty.notify_all();
  }
  // nullptr: all producers are done and the queue is drained
  std::unique_ptr<FileRecord> pop() {
    std::unique_lock<std::mutex> lk(mu);
    not_empty.wait(lk, [&] { return !q.empty() || producers == 0 || aborted; });
    if (q.empty() || aborted) return nullptr;
    std::unique_ptr<FileRecord> r = std::move(q.front());
    q.pop_front();
    not_full.notify_one();
    return r;
  }
  void abort() {
    std::lock_guard<std::mutex> lk(mu);
    aborted = true;
    not_full.notify_all();
    not_empty.notify_all();
  }
};

// Grow-only page-locked array (contents are rebuilt for every submit, nothing is preserved on growth).
template <typename T>
struct PinnedArray {
  T* p = nullptr;
  size_t cap = 0;
  PinnedArray() {}
  PinnedArray(const PinnedArray&) = delete;
  PinnedArray& operator=(const PinnedArray&) = delete;
  ~PinnedArray() { vsyn_host_free(p); }
  OkOrError ensure(size_t n) {
    if (n <= cap) return OkOrError();
    vsyn_host_free(p);
    p = nullptr;
    cap = 0;
    const size_t want = n + n / 4 + 64;
    const char* err = nullptr;
    void* q = nullptr;
    if (vsyn_host_alloc(want * sizeof(T), &q, &err) != VSYN_OK) return OkOrError(std::string("GPU synthesis layer: ") + (err ? err : "host alloc failed"));
    p = (T*)q;
    cap = want;
    return OkOrError();
  }
  T& operator[](size_t i) { return p[i]; }
};

// Files that share one synthesis setup, the handle serving them and the submit buffers (reused between submits).
struct Group {
  vsyn_handle* handle = nullptr;
  uint32_t channels = 0, bs1 = 0, ys_stride = 0;
  std::vector<std::unique_ptr<FileRecord>> pending;
  PinnedArray<vsyn_packet> pk;
  PinnedArray<vsyn_segment> seg;
  PinnedArray<uint16_t> ys;
  PinnedArray<float> residue, pcm;
  PinnedArray<int16_t> pcm16;  // CorpusOptions::pcm_s16: [S][plane][C]
  PinnedArray<uint32_t> emit;
  bool vq = false;  // files of this group ship classification + entry numbers instead of residue floats
  PinnedArray<float> rows;      // feature run: [P * C][output_dim]
  PinnedArray<uint64_t> seg_rows;
  PinnedArray<vsyn_vq_packet> vq_pk;
  PinnedArray<uint8_t> cls;
  PinnedArray<uint16_t> entries;
  ~Group() {
    if (handle) vsyn_destroy(handle);
  }
};

// sum |x| in double, 8 independent partial sums so that the compiler can keep it in vector registers
double abs_sum_f32(const float* x, uint64_t n) {
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t i = 0;
  for (; i + 8 <= n; i += 8)
    for (int k = 0; k < 8; ++k) acc[k] += (double)__builtin_fabsf(x[i + k]);
  double a = 0;
  for (; i < n; ++i) a += (double)__builtin_fabsf(x[i]);
  for (int k = 0; k < 8; ++k) a += acc[k];
  return a;
}

std::string gpu_status_text(const vsyn_status& st) {
  std::string s = "GPU synthesis check failed (flags";
  if (st.flags & VSYN_ST_FLOOR_RANGE) s += " floor-range";
  if (st.flags & VSYN_ST_FLOOR_VALUE) s += " floor-value";
  if (st.flags & VSYN_ST_GRANULE) s += " granule";
  if (st.flags & VSYN_ST_PLANE_OVERFLOW) s += " plane-overflow";
  if (st.flags & VSYN_ST_BAD_MODE) s += " bad-mode";
  if (st.flags & VSYN_ST_BAD_SEGMENT) s += " bad-segment";
  if (st.flags & VSYN_ST_BAD_VQ) s += " bad-vq";
  // accepted by the reference, refused here: a long block's next_long flag set in front of a short block
  if (st.flags & VSYN_ST_WINDOW_FLAGS) s += " window-flags: next_long set on a long block before a short one";
  if (st.flags & VSYN_ST_FEATURE_INDEX) s += " feature-index: a gather index past its vector";
  return s + ")";
}

struct Feeder {
  const CorpusOptions& opts;
  CorpusCallbacks* callbacks;
  std::vector<CorpusFileResult>& results;
  CorpusStats& stats;
  RecordQueue& queue;
  std::mutex& callbacks_mu;
  std::map<std::string, std::unique_ptr<Group>> groups;

  // Totals of the pending files' batches.
  struct Packed {
    size_t P = 0, rfloats = 0, ncls = 0, nent = 0;
    uint32_t max_p = 0;
  };

  // The pending files' batches into the group's submit buffers, one segment per file (VSYN_SEG_RESET). A synthesis run gives each
  // file a stream slot of its own and ships residue floats, or a VQ group's classifications and entry numbers; a feature run reads
  // no stream state (stream 0) and residue only for the residue kinds (with_res).
  OkOrError pack(Group& g, bool synthesis, bool with_res, Packed& k) {
    const uint32_t C = g.channels, S = (uint32_t)g.pending.size();
    const bool vq = synthesis && g.vq;
    for (const auto& r : g.pending) {
      k.P += r->batch.pk.size();
      k.rfloats += with_res ? r->batch.residue_floats : 0;
      k.ncls += r->batch.cls.size();
      k.nent += r->batch.entries.size();
      k.max_p = std::max<uint32_t>(k.max_p, (uint32_t)r->batch.pk.size());
    }
    CHECK(k.ncls < 0xffffffffu);
    CHECK(k.P < 0xffffffffu);
    CHECK_ERR(g.pk.ensure(k.P));
    CHECK_ERR(g.seg.ensure(S));
    CHECK_ERR(g.ys.ensure(k.P * C * g.ys_stride));
    if (vq) {
      CHECK_ERR(g.vq_pk.ensure(k.P));
      CHECK_ERR(g.cls.ensure(k.ncls));
      CHECK_ERR(g.entries.ensure(k.nent));
    } else if (with_res) {
      CHECK_ERR(g.residue.ensure(k.rfloats));
    }
    size_t p0 = 0, r0 = 0, c0 = 0, e0 = 0;
    for (uint32_t s = 0; s < S; ++s) {
      const PacketBatch& b = g.pending[s]->batch;
      if (synthesis) CHECK(b.vq == g.vq);
      // the staging arrays were sized from pk / residue_floats: a batch whose per-packet vectors disagree with them (a packet
      // that failed half way and was not rolled back) must not be copied
      CHECK(b.ys.size() == b.pk.size() * C * g.ys_stride);
      memcpy(&g.pk[p0], b.pk.data(), b.pk.size() * sizeof(vsyn_packet));
      memcpy(&g.ys[p0 * C * g.ys_stride], b.ys.data(), b.ys.size() * sizeof(uint16_t));
      if (vq) {
        CHECK(b.vq_pk.size() == b.pk.size());
        for (size_t q = 0; q < b.vq_pk.size(); ++q) {  // rebase the file's offsets into the merged arrays
          vsyn_vq_packet v = b.vq_pk[q];
          v.entry_off += e0;
          v.cls_off += (uint32_t)c0;
          g.vq_pk[p0 + q] = v;
        }
        memcpy(&g.cls[c0], b.cls.data(), b.cls.size());
        memcpy(&g.entries[e0], b.entries.data(), b.entries.size() * sizeof(uint16_t));
        c0 += b.cls.size();
        e0 += b.entries.size();
      } else if (with_res) {
        CHECK(!b.vq && b.residue.size() == b.residue_floats);
        memcpy(&g.residue[r0], b.residue.data(), b.residue.size() * sizeof(float));
      }
      vsyn_segment& sg = g.seg[s];
      memset(&sg, 0, sizeof(sg));
      sg.stream = synthesis ? s : 0;  // (no stream state is read or written by a feature run)
      sg.first_packet = (uint32_t)p0;
      sg.num_packets = (uint32_t)b.pk.size();
      sg.flags = VSYN_SEG_RESET;
      sg.residue_off = with_res ? r0 : 0;
      p0 += b.pk.size();
      r0 += with_res ? b.residue_floats : 0;
    }
    return OkOrError();
  }

  // A batch the device flagged: the status does not say which file beyond the first. Re-run the files one by one so that every
  // good file still gets its output and every bad one its own message.
  OkOrError submit_one_by_one(Group& g) {
    std::vector<std::unique_ptr<FileRecord>> files;
    files.swap(g.pending);
    for (auto& f : files) {
      g.pending.clear();
      g.pending.push_back(std::move(f));
      CHECK_ERR(submit(g));
    }
    return OkOrError();
  }

  // Every pending file's result: the batch's status text when the device flagged it (rc VSYN_ERR_STREAM), else what
  // deliver_file(s, record, result) sets and delivers. The records then go back to the queue.
  template <typename DeliverFile>
  OkOrError deliver(Group& g, int rc, const vsyn_status& st, double t2, DeliverFile deliver_file) {
    for (uint32_t s = 0; s < g.pending.size(); ++s) {
      FileRecord& r = *g.pending[s];
      CorpusFileResult& out = results[r.index];
      out.channels = g.channels;
      out.sample_rate = r.header.audio_sample_rate;
      out.audio_packets = (uint32_t)r.batch.pk.size();
      if (rc == VSYN_ERR_STREAM) out.status = OkOrError(gpu_status_text(st));
      else CHECK_ERR(deliver_file(s, r, out));
      stats.audio_packets += r.batch.pk.size();
      stats.files++;
    }
    for (auto& r : g.pending) queue.give_back(std::move(r));
    g.pending.clear();
    stats.deliver_s += now_s() - t2;
    return OkOrError();
  }

  // A rows run's file: rows [row0, row0 + nr) of g.rows to gotFileFeatures, unless its result is an error.
  OkOrError deliver_rows(Group& g, const FileRecord& r, CorpusFileResult& out, uint64_t& row0, uint64_t nr, uint32_t D) {
    out.feature_rows = nr;
    if (callbacks && !out.status.is_error_) {
      std::lock_guard<std::mutex> lk(callbacks_mu);
      if (!callbacks->gotFileFeatures(r.index, r.header, &g.rows[row0 * D], nr, D)) return OkOrError("aborted by gotFileFeatures");
    }
    row0 += nr;
    return OkOrError();
  }

  // Feature run: the pending files' batches through vsyn_features_host, rows delivered per file.
  OkOrError submit_features(Group& g) {
    const uint32_t C = g.channels, S = (uint32_t)g.pending.size(), D = opts.features.output_dim;
    const bool want_res = feature_needs_residue(opts);
    double t0 = now_s();
    Packed k;
    CHECK_ERR(pack(g, false, want_res, k));
    CHECK_ERR(g.rows.ensure(k.P * C * D));
    CHECK_ERR(g.seg_rows.ensure(S));
    double t1 = now_s();
    stats.pack_s += t1 - t0;
    vsyn_status st = {0, 0xffffffffu};
    const char* err = nullptr;
    const int rc = vsyn_features_host(g.handle, &opts.features, (uint32_t)k.P, g.pk.p, S, g.seg.p, g.ys.p, want_res ? g.residue.p : nullptr,
                                      k.rfloats, g.rows.p, (uint64_t)k.P * C, g.seg_rows.p, &st, &err);
    double t2 = now_s();
    stats.gpu_call_s += t2 - t1;
    stats.submits++;
    if (rc == VSYN_ERR_INVALID) {  // the spec does not fit this setup (e.g. output_dim below the biggest floor's posts): the files' problem
      const std::string msg = std::string("features: ") + (err ? err : "refused");
      for (auto& r : g.pending) {
        results[r->index].status = OkOrError(msg);
        stats.files++;
        queue.give_back(std::move(r));
      }
      g.pending.clear();
      return OkOrError();
    }
    if (rc != VSYN_OK && rc != VSYN_ERR_STREAM) return OkOrError(std::string("GPU feature layer: ") + (err ? err : "features failed"));
    if (rc == VSYN_ERR_STREAM && S > 1) return submit_one_by_one(g);
    uint64_t row0 = 0;
    return deliver(g, rc, st, t2, [&](uint32_t s, FileRecord& r, CorpusFileResult& out) {
      out.status = r.status;
      return deliver_rows(g, r, out, row0, g.seg_rows[s], D);
    });
  }

  // What a synthesis run leaves per file after its device stages: frames (the resampled ones in a resampled run), an error of its
  // own (a ratio the resampler refuses, a rate the spectral spec does not fit), and the plane of the PCM the later stages and the
  // delivery read (the synthesis plane, or the resampled one).
  struct Outcome {
    std::vector<uint64_t> frames;
    std::vector<std::string> err;
    std::vector<double> digest;  // per (file, channel), from the device
    std::vector<uint32_t> bounds;  // trim run: per file (start, end)
    std::vector<uint32_t> counts, iv;  // split run: per file its intervals, iv[(s * iv_stride + k) * 2 + {0, 1}]
    uint64_t iv_stride = 0;
    uint64_t plane = 0;
    std::vector<vsyn_loudness_record> loud;  // loudness run: per file its record,
    std::vector<uint64_t> loud_nb;           // its blocks
    std::vector<double> loud_z;              // and with loudness_blocks the block means of all files back to back
    std::vector<double> bpm;                 // beat run: per file the tempo its period came from
    std::vector<double> tuning;              // tuning run: per file the estimate
    std::vector<uint64_t> tuning_counts;     // and its two counts
  };

  // Synthesis of the packed batch. The PCM comes back as f32 planes unless a later stage reads it on the device (VSYN_SUBMIT_KEEP_PCM).
  int synthesize(Group& g, const Packed& k, uint64_t plane, bool keep_pcm, vsyn_status* st, const char** err) {
    const uint32_t S = (uint32_t)g.pending.size();
    const uint32_t sflags = keep_pcm ? VSYN_SUBMIT_KEEP_PCM : 0u;
    float* pcm_out = keep_pcm ? nullptr : g.pcm.p;
    if (!g.vq)
      return vsyn_submit_host(g.handle, (uint32_t)k.P, g.pk.p, S, g.seg.p, g.ys.p, g.residue.p, k.rfloats, pcm_out, plane, g.emit.p, nullptr,
                              sflags, st, err);
    vsyn_vq_batch vqb;
    vqb.packets = g.vq_pk.p;
    vqb.cls = g.cls.p;
    vqb.entries = g.entries.p;
    vqb.num_cls = k.ncls;
    vqb.num_entries = k.nent;
    return vsyn_submit_host_vq(g.handle, (uint32_t)k.P, g.pk.p, S, g.seg.p, g.ys.p, &vqb, nullptr, k.rfloats, pcm_out, plane, g.emit.p,
                               nullptr, sflags, st, err);
  }

  // Without resampling: the int16 PCM (pcm_s16), and the per-(file, channel) digests from the device, where the PCM still is (a
  // host pass over it cost more than the decode's GPU calls).
  OkOrError fetch(Group& g, Outcome& o) {
    const char* err = nullptr;
    if (opts.pcm_s16 && vsyn_pcm_fetch_host(g.handle, VSYN_PCM_S16, g.pcm16.p, o.plane, nullptr, &err) != VSYN_OK)
      return OkOrError(std::string("GPU synthesis layer: ") + (err ? err : "pcm fetch failed"));
    if (opts.checksum) {
      o.digest.resize(g.pending.size() * g.channels);
      if (vsyn_pcm_abs_sum_host(g.handle, o.digest.data(), &err) != VSYN_OK)
        return OkOrError(std::string("GPU synthesis layer: ") + (err ? err : "digest failed"));
    }
    return OkOrError();
  }

  // Resampled run: each file's PCM resampled on the device from its own rate to resample_rate (vsyn_pcm_resample_host, or for a
  // spectral run vsyn_pcm_chain_rhythm_host in spectral_stage); a file whose ratio the contract refuses gets no output and an error
  // of its own.
  OkOrError resample_stage(Group& g, bool spectral, Outcome& o) {
    const uint32_t C = g.channels, S = (uint32_t)g.pending.size(), out_rate = opts.resample_rate;
    std::vector<uint32_t> rates(S, 0u);  // 0: a refused file
    uint64_t rs_plane = 1;
    for (uint32_t s = 0; s < S; ++s) {
      const uint32_t sr = g.pending[s]->header.audio_sample_rate;
      if (vsyn_resample_num_frames(sr, out_rate, 1) == 0) {
        const uint32_t gd = sr ? std::gcd(sr, out_rate) : 1u;
        char buf[160];
        snprintf(buf, sizeof(buf), "resample: %u -> %u Hz reduces to %u / %u, above the limit max(up, down) <= %u", sr, out_rate,
                 out_rate / gd, sr / gd, VSYN_RESAMPLE_MAX_M);
        o.err[s] = buf;
        o.frames[s] = 0;
        continue;
      }
      rates[s] = sr;
      o.frames[s] = vsyn_resample_num_frames(sr, out_rate, std::min<uint64_t>(o.frames[s], o.plane));
      rs_plane = std::max(rs_plane, o.frames[s]);
    }
    o.plane = rs_plane;
    if (spectral) return OkOrError();
    if (opts.pcm_s16) CHECK_ERR(g.pcm16.ensure((size_t)S * C * rs_plane));
    else CHECK_ERR(g.pcm.ensure((size_t)S * C * rs_plane));
    const char* err = nullptr;
    std::vector<uint64_t> got(S);
    const int rc = vsyn_pcm_resample_host(g.handle, S, rates.data(), out_rate, opts.pcm_s16 ? VSYN_PCM_S16 : VSYN_PCM_F32,
                                          opts.pcm_s16 ? (void*)g.pcm16.p : (void*)g.pcm.p, rs_plane, got.data(), &err);
    if (rc != VSYN_OK) return OkOrError(std::string("GPU resample layer: ") + (err ? err : "resample failed"));
    CHECK(got == o.frames);
    return OkOrError();
  }

  // A file the conditioning stage refused (include/vorbis_synth_hip.h, "PCM conditioning", step 2) gets an error of its own.
  void refuse_peaks(const std::vector<float>& peaks, Outcome& o) {
    for (size_t s = 0; s < peaks.size(); ++s)
      if (o.err[s].empty() && !std::isfinite(peaks[s])) o.err[s] = "condition: the peak of the downmixed PCM is not finite";
  }

  // A file the trim stage refused (include/vorbis_synth_hip.h, "PCM trimming", step 6) gets an error of its own.
  void refuse_refs(const std::vector<double>& refs, Outcome& o) {
    for (size_t s = 0; s < refs.size(); ++s)
      if (o.err[s].empty() && !std::isfinite(refs[s])) o.err[s] = "trim: the PCM holds a sample that is not finite";
  }

  // A file the loudness stage refused (include/vorbis_synth_hip.h, "loudness", step 5) gets an error of its own, by name. A silent
  // file is measured, but cannot be normalised.
  void refuse_loud(Outcome& o, bool normalise, const std::vector<uint32_t>& rates) {
    for (size_t s = 0; s < o.loud.size(); ++s) {
      if (!o.err[s].empty()) continue;
      const uint32_t sr = opts.resample_rate && rates[s] ? opts.resample_rate : rates[s];
      char buf[160];
      switch (o.loud[s].status) {
        case VSYN_LOUD_NOT_FINITE: o.err[s] = "loudness: the PCM holds a sample that is not finite"; break;
        case VSYN_LOUD_TOO_SHORT:
          snprintf(buf, sizeof(buf), "loudness: too short: %llu frames at %u Hz are fewer than four hops of 100 ms",
                   (unsigned long long)o.frames[s], sr);
          o.err[s] = buf;
          break;
        case VSYN_LOUD_RATE_REFUSED:
          snprintf(buf, sizeof(buf), "loudness: sample rate %u below 4000 Hz", sr);
          o.err[s] = buf;
          break;
        case VSYN_LOUD_SILENT:
          if (normalise) o.err[s] = "loudness: silent: no block above -70 LUFS, nothing to normalise";
          break;
        default: break;
      }
    }
  }

  // A split run's interval arrays, sized for the longest file of the submit (its unsplit frames).
  void size_intervals(uint32_t S, Outcome& o) {
    uint64_t t_max = 0;
    for (uint32_t s = 0; s < S; ++s) t_max = std::max(t_max, o.frames[s]);
    o.iv_stride = std::max<uint64_t>(vsyn_pcm_split_max_intervals(&opts.trim_spec, t_max), 1);
    o.counts.assign(S, 0u);
    o.iv.assign((size_t)S * o.iv_stride * 2u, 0u);
  }

  // the conditioning spec of a trim run: NULL when the trimmed downmix is delivered as it is
  const vsyn_pcm_cond* trim_cond() const { return opts.cond.options ? &opts.cond : nullptr; }

  // Conditioned PCM run: each file's PCM, resampled first in a resampled run (resample_stage has set the frames and refused what
  // the resampler refuses), through the PCM stages that are on (vsyn_pcm_chain_stretch_host): one mono plane per file comes back.
  OkOrError condition_stage(Group& g, Outcome& o) {
    const uint32_t S = (uint32_t)g.pending.size();
    std::vector<uint32_t> rates(S);
    uint64_t pl = 1;
    for (uint32_t s = 0; s < S; ++s) {
      rates[s] = o.err[s].empty() ? g.pending[s]->header.audio_sample_rate : 0;
      pl = std::max(pl, o.frames[s]);
    }
    // a stretch run: each file's rate and from-rate by its index in the call, and a plane that holds the longest of what a file has
    // on its way through the stage (include/vorbis_synth_hip.h, vsyn_pcm_chain_stretch_host)
    std::vector<double> st_rates(opts.stretch ? S : 0);
    std::vector<uint32_t> st_from(opts.stretch && opts.stretch_spec.shift_to_hz ? S : 0);
    for (uint32_t s = 0; s < S && opts.stretch; ++s) {
      const size_t i = g.pending[s]->index;
      st_rates[s] = opts.stretch_rates[i];
      uint64_t len = vsyn_stretch_num_samples(o.frames[s], st_rates[s]);
      pl = std::max(pl, len);
      if (!st_from.empty()) {
        st_from[s] = opts.stretch_from_hz[i];
        pl = std::max(pl, vsyn_resample_num_frames(st_from[s], opts.stretch_spec.shift_to_hz, len));
      }
    }
    if (opts.pcm_s16) CHECK_ERR(g.pcm16.ensure((size_t)S * pl));
    else if (!opts.intervals_only) CHECK_ERR(g.pcm.ensure((size_t)S * pl));  // (intervals_only: no PCM comes back)
    const char* err = nullptr;
    std::vector<uint64_t> got(S);
    std::vector<float> peaks(S, 0.f);
    const int fmt = opts.pcm_s16 ? VSYN_PCM_S16 : VSYN_PCM_F32;
    void* out = opts.pcm_s16 ? (void*)g.pcm16.p : (void*)g.pcm.p;
    // One call for every run: the widest chain entry, a NULL spec for each stage that is off (the library makes that the entry
    // without the stage, bit for bit). Only the marks of intervals_only have an entry of their own: no PCM comes back from it.
    const bool gated = opts.split || opts.trim, staged = opts.effect || opts.stretch || opts.loudness_norm;
    const bool marks_only = opts.split && opts.intervals_only && !staged;
    // conditioning alone is the mono downmix, whatever its options; behind another stage, options 0 is no conditioning step
    const vsyn_pcm_cond* cond = gated || staged ? trim_cond() : &opts.cond;
    std::vector<double> refs(S);
    if (opts.split) size_intervals(S, o);
    if (opts.trim) o.bounds.assign(2u * (size_t)S, 0u);
    if (opts.loudness_norm) o.loud.assign(S, NO_LOUDNESS_RECORD);
    const int rc =
        marks_only
            ? vsyn_pcm_split_intervals_host(g.handle, &opts.trim_spec, S, rates.data(), opts.resample_rate, got.data(), o.counts.data(), o.iv.data(),
                                            o.iv_stride, refs.data(), &err)
            : vsyn_pcm_chain_stretch_host(g.handle, gated ? &opts.trim_spec : nullptr, opts.split ? 1 : 0, opts.effect ? &opts.effect_spec : nullptr,
                                          opts.stretch ? &opts.stretch_spec : nullptr, opts.stretch ? st_rates.data() : nullptr,
                                          st_from.empty() ? nullptr : st_from.data(), opts.loudness_norm ? &opts.loudness_spec : nullptr, cond, S,
                                          rates.data(), opts.resample_rate, fmt, out, pl, got.data(), opts.trim ? o.bounds.data() : nullptr,
                                          opts.split ? o.counts.data() : nullptr, opts.split ? o.iv.data() : nullptr, o.iv_stride, peaks.data(),
                                          refs.data(), opts.loudness_norm ? o.loud.data() : nullptr, &err);
    if (rc != VSYN_OK) {  // the run's error, named after the outermost stage that is on
      const char *layer = "GPU conditioning layer: ", *what = "conditioning failed";
      if (opts.trim) layer = "GPU trim layer: ", what = "trim failed";
      if (opts.split) layer = "GPU split layer: ", what = "split failed";
      if (opts.loudness_norm) layer = "GPU loudness layer: ", what = "normalisation failed";
      if (opts.effect) layer = "GPU effects layer: ", what = "effect failed";
      if (opts.stretch) layer = "GPU stretch layer: ", what = "effect failed";
      return OkOrError(std::string(layer) + (err ? err : what));
    }
    if (opts.stretch) {  // the stage's frames: the one step behind the gate that changes the count
      for (uint32_t s = 0; s < S; ++s) {
        CHECK(got[s] <= pl);
        o.frames[s] = got[s];
      }
    } else if (gated) {  // the frames delivered are the joined or trimmed ones (marks_only: the unsplit ones)
      for (uint32_t s = 0; s < S; ++s) {
        CHECK(got[s] <= o.frames[s]);
        o.frames[s] = got[s];
      }
    } else {
      CHECK(got == o.frames);
    }
    if (gated) refuse_refs(refs, o);
    if (opts.loudness_norm) refuse_loud(o, true, rates);
    refuse_peaks(peaks, o);
    o.plane = pl;
    return OkOrError();
  }

  // Spectral run: each file's rows from the PCM still on the device, through the stages that are on (vsyn_pcm_chain_rhythm_host); a file whose rate
  // the spec does not fit (fmax above its sr / 2) gets no rows and an error of its own, unless it has one already.
  OkOrError spectral_stage(Group& g, Outcome& o) {
    const uint32_t S = (uint32_t)g.pending.size();
    const bool resample = opts.resample_rate != 0;
    std::vector<uint32_t> rates(S);
    uint64_t spec_rows = 0;
    for (uint32_t s = 0; s < S; ++s) {
      const FileRecord& r = *g.pending[s];
      const uint32_t sr = resample ? opts.resample_rate : r.header.audio_sample_rate;  // the rate the rows are computed at
      const double ny = sr / 2.0, fmax = opts.spectral.fmax > 0.0 ? opts.spectral.fmax : ny;
      const bool lin = opts.spectral.kind >= VSYN_SPEC_LIN_POWER;  // a linear kind reads neither fmin nor fmax
      if (o.err[s].empty() && !lin && !(fmax <= ny && opts.spectral.fmin < fmax)) {
        char buf[160];
        snprintf(buf, sizeof(buf), "spectral: fmin %g / fmax %g do not fit sample rate %u (0 <= fmin < fmax <= sr/2)", opts.spectral.fmin, fmax,
                 sr);
        o.err[s] = buf;
      }
      uint64_t F = o.err[s].empty() ? vsyn_spectral_num_frames(&opts.spectral, std::min<uint64_t>(o.frames[s], o.plane)) : 0;
      if (!opts.trim && !opts.split && opts.post.order && F && F < opts.post.width) {  // fewer frames than the delta window: this file's error, not the submit's
        char buf[96];
        snprintf(buf, sizeof(buf), "spectral: delta width %u needs %u frames, file has %llu", opts.post.width, opts.post.width,
                 (unsigned long long)F);
        o.err[s] = buf;
        F = 0;
      }
      rates[s] = o.err[s].empty() ? r.header.audio_sample_rate : 0;
      spec_rows += F;
    }
    const uint64_t rhythm_words = opts.rhythm ? spec_rows * spectral_dim(opts) + 4098u * (uint64_t)S : 0;  // (the mean: 2 (W + 1) a file)
    CHECK_ERR(g.rows.ensure(opts.rhythm ? rhythm_words + 1 : spec_rows * spectral_dim(opts) + 1));  // (a beat run: a word a frame at most)
    CHECK_ERR(g.seg_rows.ensure(S));
    vsyn_status st;
    const char* err = nullptr;
    std::vector<uint32_t> rhythm_refused(S, 0u);
    std::vector<float> peaks(S);
    std::vector<double> refs(S);
    if (opts.trim) o.bounds.assign(2u * (size_t)S, 0u);  // spec_rows, from the untrimmed frames, bounds the trimmed rows
    std::vector<uint64_t> joined(S, 0);
    if (opts.split) size_intervals(S, o);
    // One call for every run: the widest chain entry, a NULL spec for each stage that is off (the library makes that the entry
    // without the stage, bit for bit), and the outputs of the gate that is on.
    const bool gated = opts.trim || opts.split;
    const vsyn_pcm_cond* cond = gated ? trim_cond() : opts.condition ? &opts.cond : nullptr;
    if (opts.loudness_norm) o.loud.assign(S, NO_LOUDNESS_RECORD);
    int rc;
    if (opts.chroma_estimate) {  // each file's tuning estimated first (the entry refuses the stages it does not take)
      o.tuning.assign(S, 0.0);
      o.tuning_counts.assign(2u * (size_t)S, 0);
      rc = vsyn_pcm_chain_chroma_est_host(
          g.handle, gated ? &opts.trim_spec : nullptr, opts.split ? 1 : 0, opts.loudness_norm ? &opts.loudness_spec : nullptr, cond, &opts.spectral,
          opts.chroma_given ? &opts.chroma_spec : nullptr, opts.pcen ? &opts.pcen_spec : nullptr, post_run(opts) ? &opts.post : nullptr,
          &opts.chroma_estimate_spec, S, rates.data(), opts.resample_rate, g.rows.p, spec_rows, g.seg_rows.p, joined.data(),
          opts.trim ? o.bounds.data() : nullptr, opts.split ? o.counts.data() : nullptr, opts.split ? o.iv.data() : nullptr, o.iv_stride,
          peaks.data(), refs.data(), opts.loudness_norm ? o.loud.data() : nullptr, o.tuning.data(), &st, &err);
    } else if (opts.beat) {  // the beat tracker in the rhythm stages' place: the same chain, the tempo per file beside the refusal words
      o.bpm.assign(S, 0.0);
      rc = vsyn_pcm_chain_beats_host(
          g.handle, gated ? &opts.trim_spec : nullptr, opts.split ? 1 : 0, opts.loudness_norm ? &opts.loudness_spec : nullptr, cond, &opts.spectral,
          opts.chroma_given ? &opts.chroma_spec : nullptr, opts.hpss ? &opts.hpss_spec : nullptr, opts.pcen ? &opts.pcen_spec : nullptr,
          post_run(opts) ? &opts.post : nullptr, &opts.beat_onset, &opts.beat_spec, S, rates.data(), opts.resample_rate, g.rows.p, spec_rows,
          g.seg_rows.p, joined.data(), opts.trim ? o.bounds.data() : nullptr, opts.split ? o.counts.data() : nullptr,
          opts.split ? o.iv.data() : nullptr, o.iv_stride, peaks.data(), refs.data(), opts.loudness_norm ? o.loud.data() : nullptr, o.bpm.data(),
          nullptr, rhythm_refused.data(), &st, &err);
    } else {
      rc = vsyn_pcm_chain_rhythm_host(
          g.handle, gated ? &opts.trim_spec : nullptr, opts.split ? 1 : 0, opts.loudness_norm ? &opts.loudness_spec : nullptr, cond, &opts.spectral,
          opts.chroma_given ? &opts.chroma_spec : nullptr, opts.hpss ? &opts.hpss_spec : nullptr, opts.pcen ? &opts.pcen_spec : nullptr,
          post_run(opts) ? &opts.post : nullptr, opts.rhythm ? &opts.rhythm_spec : nullptr, S, rates.data(), opts.resample_rate, g.rows.p,
          opts.rhythm ? rhythm_words : spec_rows, g.seg_rows.p, joined.data(), opts.trim ? o.bounds.data() : nullptr,
          opts.split ? o.counts.data() : nullptr, opts.split ? o.iv.data() : nullptr, o.iv_stride, peaks.data(), refs.data(),
          opts.loudness_norm ? o.loud.data() : nullptr, rhythm_refused.data(), &st, &err);
    }
    if (rc == VSYN_ERR_INVALID) {  // the spec itself is refused: every file's problem alike
      for (uint32_t s = 0; s < S; ++s) o.err[s] = std::string("spectral: ") + (err ? err : "refused");
      for (uint32_t s = 0; s < S; ++s) g.seg_rows[s] = 0;
    } else if (rc != VSYN_OK) {
      return OkOrError(std::string("GPU spectral layer: ") + (err ? err : "spectral failed"));
    }
    if (gated && rc == VSYN_OK) {
      refuse_refs(refs, o);
      for (uint32_t s = 0; s < S; ++s) {
        if (!o.err[s].empty()) continue;
        o.frames[s] = opts.split ? joined[s] : o.bounds[2u * s + 1u] - o.bounds[2u * s];
        const uint64_t F = vsyn_spectral_num_frames(&opts.spectral, o.frames[s]);
        if (opts.post.order && F && F < opts.post.width) {  // trimmed or joined to fewer frames than the delta window
          char buf[96];
          snprintf(buf, sizeof(buf), "spectral: delta width %u needs %u frames, file has %llu", opts.post.width, opts.post.width,
                   (unsigned long long)F);
          o.err[s] = buf;
        }
      }
    }
    if (opts.condition) refuse_peaks(peaks, o);
    for (uint32_t s = 0; s < S && rc == VSYN_OK; ++s)
      if (o.err[s].empty() && rhythm_refused[s])
        o.err[s] = rhythm_refused[s] == 1u   ? "rhythm: the onset envelope holds a value that is not finite"
                   : rhythm_refused[s] == 2u ? "rhythm: floor(ac_size * rate / hop_length) is outside [2, 2048]"
                                             : "rhythm: the beat period is outside [1, 2048] frames";
    if (opts.loudness_norm && rc == VSYN_OK) refuse_loud(o, true, rates);
    return OkOrError();
  }

  // What a pitch and a frame descriptor run share behind their rates: room for rows rows of cols columns, the call, and an error of
  // its own for a file the stage refuses (a sample that is not finite).
  template <class Call>
  OkOrError framed_rows(Group& g, Outcome& o, uint64_t rows, uint32_t cols, const char* layer, const char* name, Call call) {
    const uint32_t S = (uint32_t)g.pending.size();
    CHECK_ERR(g.rows.ensure(rows * cols + 1));
    CHECK_ERR(g.seg_rows.ensure(S));
    std::vector<uint32_t> refused(S, 0u);
    vsyn_status st;
    const char* err = nullptr;
    if (call(refused.data(), &st, &err) != VSYN_OK) return OkOrError("GPU " + std::string(layer) + " layer: " + (err ? err : std::string(name) + " failed"));
    for (uint32_t s = 0; s < S; ++s)
      if (o.err[s].empty() && refused[s]) o.err[s] = std::string(name) + ": the PCM holds a sample that is not finite";
    return OkOrError();
  }

  // Pitch run: each file's (f0, normalised difference) rows from the PCM still on the device (vsyn_pcm_pitch_host, resampled first in
  // a resampled run); a file whose rate the spec does not fit gets no rows and an error of its own, and so does a file the stage
  // refuses (a sample that is not finite).
  OkOrError pitch_stage(Group& g, Outcome& o) {
    const uint32_t S = (uint32_t)g.pending.size();
    std::vector<uint32_t> rates(S);
    uint64_t rows = 0;
    for (uint32_t s = 0; s < S; ++s) {
      const uint32_t in = g.pending[s]->header.audio_sample_rate;
      const uint32_t sr = opts.resample_rate ? opts.resample_rate : in;  // the rate the rows are computed at
      const uint32_t L = opts.pitch.frame_length;
      const double lo = std::max(std::floor(sr / opts.pitch.fmax), 1.0), hi = std::min(std::ceil(sr / opts.pitch.fmin), (double)(L - L / 2u - 1u));
      if (o.err[s].empty() && !(opts.pitch.fmax <= sr / 2.0 && hi - lo + 1.0 >= 2.0)) {  // "pitch", steps 3 and 10
        char buf[200];
        snprintf(buf, sizeof(buf), "pitch: fmin %g / fmax %g do not fit sample rate %u and frame_length %u (fmax <= sr/2, two lags or more)",
                 opts.pitch.fmin, opts.pitch.fmax, sr, L);
        o.err[s] = buf;
      }
      rates[s] = o.err[s].empty() ? in : 0;
      if (rates[s]) rows += vsyn_pitch_num_frames(&opts.pitch, std::min<uint64_t>(o.frames[s], o.plane));
    }
    return framed_rows(g, o, rows, 2u, "pitch", "pitch", [&](uint32_t* refused, vsyn_status* st, const char** err) {
      return vsyn_pcm_pitch_host(g.handle, &opts.pitch, S, rates.data(), opts.resample_rate, g.rows.p, rows, g.seg_rows.p, refused, st, err);
    });
  }

  // pYIN run: each file's (f0, voiced, voiced_prob) rows (vsyn_pcm_pyin_host), as a pitch run; whether a file's rate fits the spec
  // (fmax <= sr/2, two lags or more, an odd transition width) is vsyn_pyin_transition's answer for that rate, its text the file's error.
  OkOrError pyin_stage(Group& g, Outcome& o) {
    const uint32_t S = (uint32_t)g.pending.size();
    std::vector<uint32_t> rates(S);
    uint64_t rows = 0;
    for (uint32_t s = 0; s < S; ++s) {
      const uint32_t in = g.pending[s]->header.audio_sample_rate;
      const uint32_t sr = opts.resample_rate ? opts.resample_rate : in;  // the rate the rows are computed at
      const char* why = nullptr;
      if (o.err[s].empty() && vsyn_pyin_transition(&opts.pyin, sr, nullptr, nullptr, nullptr, 0, &why) != VSYN_OK) {
        char buf[400];
        snprintf(buf, sizeof(buf), "pyin: the spec does not fit sample rate %u: %s", sr, why ? why : "refused");
        o.err[s] = buf;
      }
      rates[s] = o.err[s].empty() ? in : 0;
      if (rates[s]) rows += vsyn_pyin_num_frames(&opts.pyin, std::min<uint64_t>(o.frames[s], o.plane));
    }
    return framed_rows(g, o, rows, 3u, "pyin", "pyin", [&](uint32_t* refused, vsyn_status* st, const char** err) {
      return vsyn_pcm_pyin_host(g.handle, &opts.pyin, S, rates.data(), opts.resample_rate, g.rows.p, rows, g.seg_rows.p, refused, st, err);
    });
  }

  // Frame descriptor run: each file's (rms, zcr, centroid, bandwidth, rolloff, flatness) rows from the PCM still on the device
  // (vsyn_pcm_fdesc_host, resampled first in a resampled run); a file the stage refuses (a sample that is not finite) gets an error
  // of its own.
  OkOrError fdesc_stage(Group& g, Outcome& o) {
    const uint32_t S = (uint32_t)g.pending.size();
    std::vector<uint32_t> rates(S);
    uint64_t rows = 0;
    for (uint32_t s = 0; s < S; ++s) {
      rates[s] = o.err[s].empty() ? g.pending[s]->header.audio_sample_rate : 0;
      if (rates[s]) rows += vsyn_fdesc_num_frames(&opts.fdesc, std::min<uint64_t>(o.frames[s], o.plane));
    }
    return framed_rows(g, o, rows, 6u, "frame descriptor", "frame descriptors", [&](uint32_t* refused, vsyn_status* st, const char** err) {
      return vsyn_pcm_fdesc_host(g.handle, &opts.fdesc, S, rates.data(), opts.resample_rate, g.rows.p, rows, g.seg_rows.p, refused, st, err);
    });
  }

  // Constant-Q run: each file's rows from the PCM still on the device (vsyn_pcm_cqt_host, resampled first in a resampled run). A file
  // whose rate makes a wavelet or the table longer than the stage's caps gets no rows and an error of its own; so does a file the
  // stage refuses, and the error says whether a sample is not finite or the top bin leaves the Nyquist band at its rate.
  OkOrError cqt_stage(Group& g, Outcome& o) {
    const uint32_t S = (uint32_t)g.pending.size(), cols = vsyn_cqt_dim(&opts.cqt);
    std::vector<uint32_t> rates(S), srs(S);
    uint64_t rows = 0;
    for (uint32_t s = 0; s < S; ++s) {
      const uint32_t in = g.pending[s]->header.audio_sample_rate;
      srs[s] = opts.resample_rate ? opts.resample_rate : in;  // the rate the rows are computed at
      if (o.err[s].empty() && srs[s] && vsyn_cqt_lengths(srs[s], &opts.cqt, nullptr, nullptr) == VSYN_ERR_INVALID) {
        char buf[200];
        snprintf(buf, sizeof(buf), "constant-Q: at sample rate %u the wavelets are longer than the stage's caps (one of %u, all of %u samples)", srs[s],
                 VSYN_CQT_MAX_LENGTH, VSYN_CQT_MAX_TABLE);
        o.err[s] = buf;
      }
      rates[s] = o.err[s].empty() ? in : 0;
      if (rates[s]) rows += vsyn_cqt_num_frames(&opts.cqt, std::min<uint64_t>(o.frames[s], o.plane));
    }
    CHECK_ERR(g.rows.ensure(rows * cols + 1));
    CHECK_ERR(g.seg_rows.ensure(S));
    std::vector<uint32_t> refused(S, 0u);
    vsyn_status st;
    const char* err = nullptr;
    if (opts.cqt_estimate) {
      o.tuning.assign(S, 0.0);
      o.tuning_counts.assign(2u * (size_t)S, 0);
    }
    if (vsyn_pcm_cqt_est_host(g.handle, &opts.cqt, opts.cqt_estimate ? &opts.cqt_estimate_spec : nullptr, S, rates.data(), opts.resample_rate, g.rows.p,
                              rows, g.seg_rows.p, refused.data(), opts.cqt_estimate ? o.tuning.data() : nullptr, &st, &err) != VSYN_OK)
      return OkOrError(std::string("GPU constant-Q layer: ") + (err ? err : "constant-Q failed"));
    for (uint32_t s = 0; s < S; ++s) {
      if (!o.err[s].empty() || !refused[s]) continue;
      if (refused[s] == VSYN_CQT_RATE) {
        char buf[200];
        snprintf(buf, sizeof(buf), "constant-Q: the top bin's pass band leaves the Nyquist band at sample rate %u", srs[s]);
        o.err[s] = buf;
      } else {
        o.err[s] = "constant-Q: the PCM holds a sample that is not finite";
      }
    }
    return OkOrError();
  }

  // Tuning run: each file's estimate, and with tuning_rows its piptrack rows, from the PCM still on the device (vsyn_pcm_tuning_host,
  // resampled first in a resampled run). A frame with a sample that is not finite is NaN in the rows and gives the estimate no peak.
  OkOrError tuning_stage(Group& g, Outcome& o) {
    const uint32_t S = (uint32_t)g.pending.size(), cols = 2u * (opts.tuning_framing.n_fft / 2u + 1u);
    std::vector<uint32_t> rates(S);
    uint64_t rows = 0;
    for (uint32_t s = 0; s < S; ++s) {
      rates[s] = o.err[s].empty() ? g.pending[s]->header.audio_sample_rate : 0;
      if (rates[s] && opts.tuning_rows) rows += vsyn_spectral_num_frames(&opts.tuning_framing, std::min<uint64_t>(o.frames[s], o.plane));
    }
    if (opts.resample_rate && opts.tuning_rows) {  // the rows are those of the resampled frames: the stage's own count
      vsyn_status st0;
      const char* err0 = nullptr;
      CHECK_ERR(g.seg_rows.ensure(S));
      if (vsyn_pcm_tuning_host(g.handle, &opts.tuning_framing, &opts.tuning, S, rates.data(), opts.resample_rate, VSYN_TUNING_ROWS, nullptr, nullptr,
                               nullptr, 0, g.seg_rows.p, &st0, &err0) != VSYN_OK)
        return OkOrError(std::string("GPU tuning layer: ") + (err0 ? err0 : "tuning failed"));
      rows = 0;
      for (uint32_t s = 0; s < S && opts.tuning_rows; ++s) rows += g.seg_rows[s];
    }
    CHECK_ERR(g.rows.ensure(rows * cols + 1));
    CHECK_ERR(g.seg_rows.ensure(S));
    o.tuning.assign(S, 0.0);
    o.tuning_counts.assign(2u * (size_t)S, 0);
    vsyn_status st;
    const char* err = nullptr;
    if (vsyn_pcm_tuning_host(g.handle, &opts.tuning_framing, &opts.tuning, S, rates.data(), opts.resample_rate,
                             opts.tuning_rows ? VSYN_TUNING_ROWS : VSYN_TUNING_ONLY, o.tuning.data(), o.tuning_counts.data(),
                             opts.tuning_rows ? g.rows.p : nullptr, rows, g.seg_rows.p, &st, &err) != VSYN_OK)
      return OkOrError(std::string("GPU tuning layer: ") + (err ? err : "tuning failed"));
    if (!opts.tuning_rows)
      for (uint32_t s = 0; s < S; ++s) g.seg_rows[s] = 0;  // nothing to deliver
    return OkOrError();
  }

  // Loudness run: each file's record (and block means) from the PCM still on the device (vsyn_pcm_loudness_host, resampled first in
  // a resampled run). A silent file is measured; a file the stage refuses gets an error of its own, by name.
  OkOrError loudness_stage(Group& g, Outcome& o) {
    const uint32_t S = (uint32_t)g.pending.size();
    std::vector<uint32_t> rates(S);
    for (uint32_t s = 0; s < S; ++s) rates[s] = o.err[s].empty() ? g.pending[s]->header.audio_sample_rate : 0;
    o.loud.assign(S, NO_LOUDNESS_RECORD);
    o.loud_nb.assign(S, 0);
    vsyn_status st;
    const char* err = nullptr;
    if (opts.loudness_blocks) {  // the size query first: nothing is launched for NULL records
      if (vsyn_pcm_loudness_host(g.handle, &opts.loudness_spec, S, rates.data(), opts.resample_rate, nullptr, nullptr, 0, o.loud_nb.data(), &st, &err) !=
          VSYN_OK)
        return OkOrError(std::string("GPU loudness layer: ") + (err ? err : "loudness failed"));
      uint64_t total = 0;
      for (uint32_t s = 0; s < S; ++s) total += o.loud_nb[s];
      o.loud_z.assign(total + 1, 0.0);
    }
    if (vsyn_pcm_loudness_host(g.handle, &opts.loudness_spec, S, rates.data(), opts.resample_rate, o.loud.data(),
                               opts.loudness_blocks ? o.loud_z.data() : nullptr, o.loud_z.size(), o.loud_nb.data(), &st, &err) != VSYN_OK)
      return OkOrError(std::string("GPU loudness layer: ") + (err ? err : "loudness failed"));
    refuse_loud(o, false, rates);
    return OkOrError();
  }

  // A synthesis run's file: its PCM (or, for a spectral, pitch or frame descriptor run, its rows) to the callbacks.
  OkOrError deliver_pcm(Group& g, uint32_t s, const FileRecord& r, CorpusFileResult& out, const Outcome& o, uint64_t& row0) {
    const uint32_t C = opts.condition ? 1u : g.channels;  // channels delivered
    const bool spectral = spectral_run(opts) || pitch_run(opts) || pyin_run(opts) || fdesc_run(opts) || cqt_run(opts) || tuning_run(opts) || loudness_run(opts);
    const uint64_t frames = o.frames[s], pl = o.plane;
    if (opts.condition) out.channels = 1;
    std::vector<DataRange<const float>> chans(C);
    double acc = 0;
    for (uint32_t c = 0; c < C; ++c) {
      if (!opts.pcm_s16 && !spectral && !opts.intervals_only) {
        const float* x = &g.pcm[((size_t)s * C + c) * pl];
        chans[c] = DataRange<const float>(x, frames);
        if (opts.checksum && o.digest.empty()) acc += abs_sum_f32(x, frames);
      }
      if (opts.checksum && !o.digest.empty()) acc += o.digest[(size_t)s * C + c];
    }
    out.frames = frames;
    if (!o.bounds.empty()) {
      out.trim_start = o.bounds[2u * s];
      out.trim_end = o.bounds[2u * s + 1u];
    }
    if (!o.counts.empty() && o.err[s].empty()) {
      const uint32_t* iv = &o.iv[(size_t)s * o.iv_stride * 2u];
      out.intervals.assign(iv, iv + 2u * (size_t)std::min<uint64_t>(o.counts[s], o.iv_stride));
    }
    out.abs_sum = acc;
    out.status = o.err[s].empty() ? r.status : OkOrError(o.err[s]);
    if (opts.resample_rate) out.sample_rate = opts.resample_rate;
    stats.frames += frames;
    if (o.err[s].empty() && s < o.loud.size()) out.loudness = o.loud[s];
    if (o.err[s].empty() && s < o.bpm.size()) out.bpm = o.bpm[s];
    if (o.err[s].empty() && s < o.tuning.size()) {
      out.tuning = o.tuning[s];
      out.tuning_counts[0] = o.tuning_counts[2u * s];
      out.tuning_counts[1] = o.tuning_counts[2u * s + 1u];
    }
    if (loudness_run(opts)) {  // the record and the block means: nothing goes to the callbacks; row0 counts the blocks in front
      if (o.err[s].empty() && s < o.loud.size()) {
        if (opts.loudness_blocks) out.loudness_blocks.assign(o.loud_z.begin() + row0, o.loud_z.begin() + row0 + o.loud_nb[s]);
      }
      if (s < o.loud_nb.size()) row0 += o.loud_nb[s];
      return OkOrError();
    }
    if (spectral) return deliver_rows(g, r, out, row0, g.seg_rows[s], pitch_run(opts) ? 2u : pyin_run(opts) ? 3u : fdesc_run(opts) ? 6u : cqt_run(opts) ? vsyn_cqt_dim(&opts.cqt) : tuning_run(opts) ? 2u * (opts.tuning_framing.n_fft / 2u + 1u) : spectral_dim(opts));
    if (!callbacks || !o.err[s].empty() || opts.intervals_only) return OkOrError();
    std::lock_guard<std::mutex> lk(callbacks_mu);
    if (opts.pcm_s16) {
      if (!callbacks->gotFilePcmS16(r.index, r.header, &g.pcm16[(size_t)s * pl * C], frames)) return OkOrError("aborted by gotFilePcmS16");
    } else if (!callbacks->gotFilePcm(r.index, r.header, chans)) {
      return OkOrError("aborted by gotFilePcm");
    }
    return OkOrError();
  }

  OkOrError submit(Group& g) {
    if (g.pending.empty()) return OkOrError();
    if (feature_run(opts)) return submit_features(g);
    const uint32_t C = g.channels, S = (uint32_t)g.pending.size();
    const bool pitch = pitch_run(opts), pyin = pyin_run(opts), fdesc = fdesc_run(opts), cqt = cqt_run(opts), loud = loudness_run(opts);
    const bool tune = tuning_run(opts);
    const bool spectral = spectral_run(opts) || pitch || pyin || fdesc || cqt || tune || loud;  // the PCM stays on the device: only the spectral (pitch, descriptor) rows come back
    const bool resample = opts.resample_rate != 0;  // the PCM stays on the device until it is resampled
    const bool cond = opts.condition;               // ... and until it is conditioned
    double t0 = now_s();
    Packed k;
    CHECK_ERR(pack(g, true, true, k));
    const uint64_t plane = (uint64_t)k.max_p * (g.bs1 / 2);
    CHECK_ERR(g.emit.ensure(k.P));
    if (opts.pcm_s16) CHECK_ERR(g.pcm16.ensure((size_t)S * C * plane));
    else if (!spectral && !resample && !cond) CHECK_ERR(g.pcm.ensure((size_t)S * C * plane));
    double t1 = now_s();
    stats.pack_s += t1 - t0;
    vsyn_status st = {0, 0xffffffffu};
    const char* err = nullptr;
    const int rc = synthesize(g, k, plane, opts.pcm_s16 || spectral || resample || cond, &st, &err);
    Outcome o;
    if (rc == VSYN_OK) {
      o.plane = plane;
      o.err.assign(S, std::string());
      o.frames.assign(S, 0);
      size_t q0 = 0;
      for (uint32_t s = 0; s < S; ++s) {  // each file's frames: the sum of its packets' emit
        const size_t np = g.pending[s]->batch.pk.size();
        for (size_t q = 0; q < np; ++q) o.frames[s] += g.emit[q0 + q];
        q0 += np;
        CHECK(o.frames[s] <= plane);
      }
      if (resample) CHECK_ERR(resample_stage(g, spectral || cond, o));
      else if (!cond) CHECK_ERR(fetch(g, o));
      if (cond && !spectral) CHECK_ERR(condition_stage(g, o));
      if (loud) CHECK_ERR(loudness_stage(g, o));
      else if (pitch) CHECK_ERR(pitch_stage(g, o));
      else if (pyin) CHECK_ERR(pyin_stage(g, o));
      else if (fdesc) CHECK_ERR(fdesc_stage(g, o));
      else if (cqt) CHECK_ERR(cqt_stage(g, o));
      else if (tune) CHECK_ERR(tuning_stage(g, o));
      else if (spectral) CHECK_ERR(spectral_stage(g, o));
    }
    double t2 = now_s();
    stats.gpu_call_s += t2 - t1;
    stats.submits++;
    if (rc != VSYN_OK && rc != VSYN_ERR_STREAM) return OkOrError(std::string("GPU synthesis layer: ") + (err ? err : "submit failed"));
    if (rc == VSYN_ERR_STREAM && S > 1) return submit_one_by_one(g);
    uint64_t row0 = 0;
    return deliver(g, rc, st, t2, [&](uint32_t s, FileRecord& r, CorpusFileResult& out) { return deliver_pcm(g, s, r, out, o, row0); });
  }

  OkOrError take(std::unique_ptr<FileRecord> rec) {
    CorpusFileResult& out = results[rec->index];
    if (!rec->has_audio) {  // failed before any audio, or a file without audio packets
      out.status = rec->status;
      out.channels = rec->status.is_error_ ? 0 : rec->header.audio_channels;
      stats.files++;
      queue.give_back(std::move(rec));
      return OkOrError();
    }
    if (opts.entropy_only) {
      out.status = rec->status;
      out.channels = rec->header.audio_channels;
      out.sample_rate = rec->header.audio_sample_rate;
      out.audio_packets = (uint32_t)rec->batch.pk.size();
      stats.audio_packets += rec->batch.pk.size();
      stats.files++;
      queue.give_back(std::move(rec));
      return OkOrError();
    }
    // A file that failed half-way (truncated, corrupt packet) still delivers what was decoded before the failure, as the
    // reference does through gotPcmData before its CHECK fires; the error is kept in the result.
    std::unique_ptr<Group>& gp = groups[rec->synth.key];
    if (!gp) {
      gp.reset(new Group());
      const char* err = nullptr;
      const int rc = vsyn_create(&rec->synth.su, opts.device, opts.files_per_submit, &gp->handle, &err);
      if (rc != VSYN_OK) {
        // a setup the GPU layer rejects is this file's problem; no device at all is everybody's
        std::string msg = std::string("GPU synthesis layer: ") + (err ? err : "vsyn_create failed");
        groups.erase(rec->synth.key);
        if (rc == VSYN_ERR_NO_DEVICE || rc == VSYN_ERR_HIP) return OkOrError(msg);
        out.status = OkOrError(msg);
        stats.files++;
        return OkOrError();
      }
      if (rec->synth.has_vq && !feature_run(opts) && vsyn_attach_vq(gp->handle, &rec->synth.vq, &err) != VSYN_OK) {
        std::string msg = std::string("GPU synthesis layer: ") + (err ? err : "vsyn_attach_vq failed");
        groups.erase(rec->synth.key);
        return OkOrError(msg);
      }
      gp->vq = rec->synth.has_vq;
      gp->channels = rec->header.audio_channels;
      gp->bs1 = rec->header.get_blocksize_1();
      gp->ys_stride = vsyn_ys_stride(gp->handle);
      stats.handles++;
    }
    CHECK(gp->ys_stride == rec->ys_stride);
    gp->pending.push_back(std::move(rec));
    if (gp->pending.size() >= opts.files_per_submit) CHECK_ERR(submit(*gp));
    return OkOrError();
  }

  OkOrError finish() {
    for (auto& kv : groups) CHECK_ERR(submit(*kv.second));
    return OkOrError();
  }
};

}  // namespace

OkOrError decode_corpus(const std::vector<CorpusItem>& items, const CorpusOptions& opts_in, CorpusCallbacks* callbacks,
                        std::vector<CorpusFileResult>& results, CorpusStats* stats_out) {
  CorpusOptions opts = opts_in;
  if (opts.threads <= 0) opts.threads = (int)std::max(1u, std::thread::hardware_concurrency());
  if (opts.feeders <= 0) opts.feeders = 3;
  if (opts.files_per_submit == 0) opts.files_per_submit = 64;
  if (opts.max_pending_files == 0) opts.max_pending_files = 4 * opts.files_per_submit;
  results.assign(items.size(), CorpusFileResult());
  CorpusStats stats;
  const double t_start = now_s();

  SetupCache setup_cache;
  RecordQueue queue(opts.max_pending_files, (size_t)opts.threads);
  std::atomic<size_t> next(0);
  std::atomic<bool> stop(false);
  std::vector<double> worker_cpu((size_t)opts.threads, 0.0);
  std::vector<std::thread> workers;
  for (int t = 0; t < opts.threads; ++t) {
    workers.emplace_back([&, t] {
      for (;;) {
        if (stop.load(std::memory_order_relaxed)) break;
        const size_t i = next.fetch_add(1);
        if (i >= items.size()) break;
        std::unique_ptr<FileRecord> rec = queue.fresh();
        rec->index = i;
        const double t0 = now_s();
        entropy_decode_file(items[i], *rec, opts.share_setups ? &setup_cache : nullptr, feature_needs_residue(opts));
        worker_cpu[(size_t)t] += now_s() - t0;
        if (!queue.push(std::move(rec))) break;
      }
      queue.producer_done();
    });
  }

  // feeder lanes: each owns its handles (one per synthesis setup it meets) and its page-locked submit buffers
  std::mutex callbacks_mu, status_mu;
  OkOrError run_status;
  std::vector<CorpusStats> lane_stats((size_t)opts.feeders);
  std::vector<std::thread> feeders;
  for (int f = 0; f < opts.feeders; ++f) {
    feeders.emplace_back([&, f] {
      Feeder feeder{opts, callbacks, results, lane_stats[(size_t)f], queue, callbacks_mu, {}};
      OkOrError st;
      for (;;) {
        std::unique_ptr<FileRecord> rec = queue.pop();
        if (!rec) break;
        st = feeder.take(std::move(rec));
        if (st.is_error_) break;
      }
      if (!st.is_error_ && !stop.load()) st = feeder.finish();
      if (st.is_error_) {
        stop.store(true);
        queue.abort();
        std::lock_guard<std::mutex> lk(status_mu);
        if (!run_status.is_error_) run_status = st;
      }
    });
  }
  for (std::thread& w : workers) w.join();
  for (std::thread& f : feeders) f.join();
  for (const CorpusStats& l : lane_stats) {
    stats.gpu_call_s += l.gpu_call_s;
    stats.pack_s += l.pack_s;
    stats.deliver_s += l.deliver_s;
    stats.submits += l.submits;
    stats.files += l.files;
    stats.audio_packets += l.audio_packets;
    stats.frames += l.frames;
    stats.handles += l.handles;
  }

  stats.setup_parses = setup_cache.misses;
  stats.setup_reuses = setup_cache.hits;
  stats.wall_s = now_s() - t_start;
  for (double c : worker_cpu) stats.entropy_cpu_s += c;
  if (stats_out) *stats_out = stats;
  return run_status;
}

namespace {

CorpusOptions call_options(int threads, int feeders, uint32_t files_per_submit, int device) {
  CorpusOptions opts;
  opts.threads = threads;
  opts.feeders = feeders;
  opts.files_per_submit = files_per_submit;
  opts.device = device;
  return opts;
}

// decode_corpus over the C form's arrays; stats_out (may be NULL) receives the 8 doubles the header lists.
OkOrError run_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, const CorpusOptions& opts, CorpusCallbacks* callbacks,
                     std::vector<CorpusFileResult>& results, double* stats_out) {
  std::vector<CorpusItem> items(num_files);
  for (size_t i = 0; i < num_files; ++i) items[i] = CorpusItem{datas[i], lens[i]};
  CorpusStats st;
  OkOrError r = decode_corpus(items, opts, callbacks, results, &st);
  if (stats_out) {
    const double v[8] = {st.wall_s, st.entropy_cpu_s, st.gpu_call_s, st.pack_s, st.deliver_s, (double)st.submits, (double)st.audio_packets, (double)st.frames};
    for (int i = 0; i < 8; ++i) stats_out[i] = v[i];
  }
  return r;
}

// The C form's return: 0 with *error_out = NULL, or 1 with *error_out pointing at the run's error text in buf.
int call_result(const OkOrError& r, char (&buf)[256], const char** error_out) {
  if (!r.is_error_) {
    if (error_out) *error_out = nullptr;
    return 0;
  }
  snprintf(buf, sizeof(buf), "%s", r.err_msg_.c_str());
  if (error_out) *error_out = buf;
  return 1;
}

}  // namespace

extern "C" int ogg_vorbis_decode_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                        uint32_t files_per_submit, int device, uint64_t* frames_out, double* abs_sum_out, uint8_t* ok_out, float* const* pcm_out,
                                        const uint64_t* pcm_capacity, double* stats_out, const char** error_out) {
  static char error_buf[256];
  struct CopyOut : CorpusCallbacks {
    float* const* pcm_out;
    const uint64_t* cap;
    std::vector<uint8_t> too_long;
    bool gotFilePcm(size_t i, const VorbisIdHeader&, const std::vector<DataRange<const float>>& ch) override {
      if (!pcm_out || !pcm_out[i]) return true;
      for (size_t c = 0; c < ch.size(); ++c) {
        if (ch[c].size() > cap[i]) {
          too_long[i] = 1;
          return true;
        }
        memcpy(pcm_out[i] + c * cap[i], ch[c].begin(), ch[c].size() * sizeof(float));
      }
      return true;
    }
  } copy_out;
  copy_out.pcm_out = pcm_out;
  copy_out.cap = pcm_capacity;
  copy_out.too_long.assign(num_files, 0);
  std::vector<CorpusFileResult> results;
  const OkOrError r = run_corpus(datas, lens, num_files, call_options(threads, feeders, files_per_submit, device),
                                 pcm_out && pcm_capacity ? &copy_out : nullptr, results, stats_out);
  for (size_t i = 0; i < results.size() && i < num_files; ++i) {
    if (frames_out) frames_out[i] = results[i].frames;
    if (abs_sum_out) abs_sum_out[i] = results[i].abs_sum;
    if (ok_out) ok_out[i] = results[i].status.is_error_ || copy_out.too_long[i] ? 0 : 1;
  }
  return call_result(r, error_buf, error_out);
}

// The same with int16 output (CorpusOptions::pcm_s16): pcm16_out[i] (may be NULL) receives the file's interleaved frames,
// at most pcm_capacity_frames[i] of them (a longer file is marked failed).
extern "C" int ogg_vorbis_decode_corpus_s16(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                            uint32_t files_per_submit, int device, uint64_t* frames_out, uint8_t* ok_out, int16_t* const* pcm16_out,
                                            const uint64_t* pcm_capacity_frames, double* stats_out, const char** error_out) {
  static char error_buf[256];
  CorpusOptions opts = call_options(threads, feeders, files_per_submit, device);
  opts.pcm_s16 = true;
  struct CopyOut : CorpusCallbacks {
    int16_t* const* out;
    const uint64_t* cap;
    std::vector<uint8_t> too_long;
    bool gotFilePcmS16(size_t i, const VorbisIdHeader& h, const int16_t* x, uint64_t frames) override {
      if (!out || !out[i]) return true;
      if (frames > cap[i]) {
        too_long[i] = 1;
        return true;
      }
      memcpy(out[i], x, (size_t)frames * h.audio_channels * sizeof(int16_t));
      return true;
    }
  } copy_out;
  copy_out.out = pcm16_out;
  copy_out.cap = pcm_capacity_frames;
  copy_out.too_long.assign(num_files, 0);
  std::vector<CorpusFileResult> results;
  const OkOrError r = run_corpus(datas, lens, num_files, opts, pcm16_out && pcm_capacity_frames ? &copy_out : nullptr, results, stats_out);
  for (size_t i = 0; i < results.size() && i < num_files; ++i) {
    if (frames_out) frames_out[i] = results[i].frames;
    if (ok_out) ok_out[i] = results[i].status.is_error_ || copy_out.too_long[i] ? 0 : 1;
  }
  return call_result(r, error_buf, error_out);
}

namespace {

// Per calling thread (loader threads may run passes side by side): the error texts of the corpus calls below.
thread_local char corpus_error_buf[256];
thread_local std::vector<std::string> corpus_file_errors;

// Each file's output (rows, or PCM) into a malloc'd buffer of its own: the callbacks never overlap (CorpusCallbacks).
struct MallocOut : CorpusCallbacks {
  void** out = nullptr;
  std::vector<uint8_t> no_mem;
  void* alloc(size_t i, size_t bytes) {  // out[i], or NULL with no_mem[i] set
    void* p = malloc(bytes);
    if (!p) no_mem[i] = 1;
    return out[i] = p;
  }
  bool gotFileFeatures(size_t i, const VorbisIdHeader&, const float* rows, uint64_t n, uint32_t dim) override {
    const size_t bytes = (size_t)n * dim * sizeof(float);
    if (n && alloc(i, bytes)) memcpy(out[i], rows, bytes);
    return true;
  }
  bool gotFilePcm(size_t i, const VorbisIdHeader&, const std::vector<DataRange<const float>>& ch) override {
    const size_t n = ch.empty() ? 0 : ch[0].size();
    if (n && alloc(i, n * ch.size() * sizeof(float)))
      for (size_t c = 0; c < ch.size(); ++c) memcpy((float*)out[i] + c * n, ch[c].begin(), n * sizeof(float));
    return true;
  }
  uint32_t s16_channels = 0;  // channels of the int16 frames delivered; 0: the header's (CorpusOptions::condition delivers one)
  bool gotFilePcmS16(size_t i, const VorbisIdHeader& h, const int16_t* x, uint64_t frames) override {
    const size_t bytes = (size_t)frames * (s16_channels ? s16_channels : h.audio_channels) * sizeof(int16_t);
    if (frames && alloc(i, bytes)) memcpy(out[i], x, bytes);
    return true;
  }
};

// A call refused before the run: every out[i] NULL, 1 with *error_out = msg.
int refuse_call(void** out, size_t num_files, const std::string& msg, const char** error_out) {
  if (out)
    for (size_t i = 0; i < num_files; ++i) out[i] = nullptr;
  return call_result(OkOrError(msg), corpus_error_buf, error_out);
}

// One pass of a run whose files' outputs each come back in a malloc'd buffer (ogg_vorbis_features_free): out[i] NULL for a failed
// file or one without output; ok_out and error_out_per_file per file, and per_file(i, result, bad) for the caller's other arrays.
// name prefixes the out-of-memory error of a file.
template <typename PerFile>
int malloc_corpus(const char* name, const uint8_t* const* datas, const size_t* lens, size_t num_files, CorpusOptions opts, void** out,
                  uint8_t* ok_out, const char** error_out_per_file, double* stats_out, const char** error_out, PerFile per_file) {
  opts.checksum = false;
  if (out)
    for (size_t i = 0; i < num_files; ++i) out[i] = nullptr;
  MallocOut copy_out;
  copy_out.out = out;
  copy_out.s16_channels = opts.condition ? 1u : 0u;
  copy_out.no_mem.assign(num_files, 0);
  std::vector<CorpusFileResult> results;
  const OkOrError r = run_corpus(datas, lens, num_files, opts, out ? &copy_out : nullptr, results, stats_out);
  corpus_file_errors.assign(num_files, std::string());
  for (size_t i = 0; i < results.size() && i < num_files; ++i) {
    const bool bad = results[i].status.is_error_ || copy_out.no_mem[i];
    if (bad && out && out[i]) {
      free(out[i]);
      out[i] = nullptr;
    }
    per_file(i, results[i], bad);
    if (ok_out) ok_out[i] = bad ? 0 : 1;
    if (error_out_per_file) {
      corpus_file_errors[i] = results[i].status.is_error_ ? results[i].status.err_msg_ : (copy_out.no_mem[i] ? std::string(name) + ": out of host memory" : "");
      error_out_per_file[i] = bad ? corpus_file_errors[i].c_str() : nullptr;
    }
  }
  if (r.is_error_ && out)
    for (size_t i = 0; i < num_files; ++i) {
      free(out[i]);
      out[i] = nullptr;
    }
  return call_result(r, corpus_error_buf, error_out);
}

// A file's (start, end) of a trim run into bounds_out[i][2] (zeros for a failed file, and without the stage).
void give_bounds(uint64_t* bounds_out, size_t i, const CorpusFileResult& res, bool bad) {
  if (!bounds_out) return;
  bounds_out[2 * i] = bad ? 0 : res.trim_start;
  bounds_out[2 * i + 1] = bad ? 0 : res.trim_end;
}

// A file's intervals of a split run into a buffer of its own, intervals_out[i] (NULL for a failed file, and without intervals).
void give_intervals(uint32_t** intervals_out, uint64_t* intervals_count_out, size_t i, const CorpusFileResult& res, bool bad) {
  const size_t n = bad ? 0 : res.intervals.size() / 2u;
  if (intervals_count_out) intervals_count_out[i] = n;
  if (!intervals_out) return;
  intervals_out[i] = nullptr;
  if (!n) return;
  intervals_out[i] = (uint32_t*)malloc(res.intervals.size() * sizeof(uint32_t));
  if (intervals_out[i]) memcpy(intervals_out[i], res.intervals.data(), res.intervals.size() * sizeof(uint32_t));
  else if (intervals_count_out) intervals_count_out[i] = 0;
}

// Where a split run's per-file results go (any may be NULL): the joined frames, the interval buffers and their counts.
struct SplitOuts {
  uint64_t* frames_out = nullptr;
  uint32_t** intervals_out = nullptr;
  uint64_t* intervals_count_out = nullptr;
  void clear(size_t num_files) const {  // before the run, and behind a run that failed: no buffer is handed over
    for (size_t i = 0; intervals_out && i < num_files; ++i) {
      free(intervals_out[i]);
      intervals_out[i] = nullptr;
    }
  }
  void begin(size_t num_files) const {
    for (size_t i = 0; intervals_out && i < num_files; ++i) intervals_out[i] = nullptr;
    for (size_t i = 0; intervals_count_out && i < num_files; ++i) intervals_count_out[i] = 0;
  }
};

// What a run with the normaliser asks of its spec (include/vorbis_synth_hip.h, "loudness", step 7).
bool loud_norm_spec_ok(const vsyn_loudness_spec* l, const vsyn_pcm_cond* cond) {
  return l->options == VSYN_LOUD_NORMALIZE && l->channel_mode == VSYN_LOUD_MONO && l->target >= -70.0 && l->target <= 0.0 &&
         !(cond && (cond->options & VSYN_COND_PEAK));
}

// What a run with the effect stage asks of its spec (include/vorbis_synth_hip.h, "PCM effects", step 6).
bool effect_spec_ok(const vsyn_pcm_effect* e) {
  const vsyn_spectral_hpss& p = e->hpss;
  return e->n_fft >= 16 && e->n_fft <= 8192 && !(e->n_fft & (e->n_fft - 1u)) && e->hop_length >= 1 && e->win_length >= 1 &&
         e->win_length <= e->n_fft && (p.kh & 1u) && p.kh <= 63 && (p.kp & 1u) && p.kp <= 63 && p.component <= VSYN_HPSS_PERCUSSIVE &&
         p.output == VSYN_HPSS_OUT_COMPONENT && p.power > 0.0 && std::isfinite(p.margin_h) && p.margin_h >= 1.0 && std::isfinite(p.margin_p) &&
         p.margin_p >= 1.0;
}

// What a run with the stretch stage asks of its spec and its per-file arrays (include/vorbis_synth_hip.h, "PCM stretch", step 9):
// empty, or why the call is refused.
std::string stretch_refusal(const vsyn_pcm_stretch* e, size_t num_files, const double* rates, const uint32_t* from_hz) {
  if (!(e->n_fft >= 16 && e->n_fft <= 8192 && !(e->n_fft & (e->n_fft - 1u)) && e->hop_length >= 1 && e->win_length >= 1 && e->win_length <= e->n_fft &&
        !(e->options & ~VSYN_STRETCH_FIX_LENGTH) && !e->reserved))
    return "invalid stretch spec (n_fft a power of two in [16, 8192], hop_length >= 1, win_length in [1, n_fft], known options)";
  if (num_files && (!rates || (e->shift_to_hz && !from_hz))) return "NULL per-file rates";
  for (size_t i = 0; i < num_files; ++i) {
    if (!std::isfinite(rates[i]) || !(rates[i] > 0.0)) return "file " + std::to_string(i) + ": the rate is not a finite number above 0";
    if (e->shift_to_hz && vsyn_resample_num_frames(from_hz[i], e->shift_to_hz, 1) == 0)
      return "file " + std::to_string(i) + ": resample: " + std::to_string(from_hz[i]) + " -> " + std::to_string(e->shift_to_hz) +
             " Hz is a pair the resampler refuses (a rate of 0, or max(up, down) above " + std::to_string(VSYN_RESAMPLE_MAX_M) + ")";
  }
  return std::string();
}

// One exported rows or PCM corpus call: its files, the options its entry fills through the setters below, and where its per-file
// results go (any output may be NULL). An entry names its outputs, calls the setters of the stages it takes in the order the call's
// refusals are checked in, and ends in rows() or pcm(); the first refusal stands and is the call's answer there. fn is the entry's
// name for the refusal texts of a rows call, and NULL for a PCM call, whose refusals carry fixed names whichever entry was called.
struct CorpusCall {
  const char* fn;
  const uint8_t* const* datas;
  const size_t* lens;
  size_t num_files;
  CorpusOptions opts;
  void** out;                             // per file: the rows, or the PCM
  uint8_t* ok_out;
  const char** error_out_per_file;
  double* stats_out;
  const char** error_out;
  uint64_t* rows_count_out = nullptr;
  uint64_t* frames_out = nullptr;         // a PCM call's frames (a rows call's joined frames are split.frames_out)
  uint32_t* channels_out = nullptr;
  uint32_t* rate_out = nullptr;
  double* bpm_out = nullptr;              // a beat run's tempo per file
  double* tuning_out = nullptr;           // a chroma run's estimated tuning per file
  uint64_t* bounds_out = nullptr;
  SplitOuts split;
  vsyn_loudness_record* records_out = nullptr;
  std::string refusal;

  CorpusCall(const char* fn_, const uint8_t* const* datas_, const size_t* lens_, size_t num_files_, int threads, int feeders,
             uint32_t files_per_submit, int device, void** out_, uint8_t* ok_out_, const char** error_out_per_file_, double* stats_out_,
             const char** error_out_)
      : fn(fn_), datas(datas_), lens(lens_), num_files(num_files_), opts(call_options(threads, feeders, files_per_submit, device)), out(out_),
        ok_out(ok_out_), error_out_per_file(error_out_per_file_), stats_out(stats_out_), error_out(error_out_) {}

  void refuse(const char* pcm_entry, const std::string& why) {
    if (refusal.empty()) refusal = std::string(fn ? fn : pcm_entry) + ": " + why;
  }

  // The outputs of a split, nulled before anything else. The joined frames are written by a split run alone: a call that takes a
  // gate which is no split (split_run = false) has them zeroed here.
  void split_outputs(uint64_t* joined_frames_out, uint32_t** intervals_out, uint64_t* intervals_count_out, bool split_run) {
    split.frames_out = joined_frames_out;
    split.intervals_out = intervals_out;
    split.intervals_count_out = intervals_count_out;
    split.begin(num_files);
    for (size_t i = 0; !split_run && joined_frames_out && i < num_files; ++i) joined_frames_out[i] = 0;
  }

  void spectral(const vsyn_spectral_spec* spec, uint32_t target_rate, const vsyn_spectral_post* post) {
    if (!spec || spec->kind == 0) return refuse(fn, "no spectral kind");
    if (post && !vsyn_spectral_post_dim(spec, post)) return refuse(fn, "invalid spectral or post spec");
    opts.spectral = *spec;
    opts.resample_rate = target_rate;
    if (post) opts.post = *post;
  }
  // the chroma parameters of the entries that take them (NULL: the defaults): they refuse a spec the chroma dimension has no answer for
  void chroma(const vsyn_spectral_chroma* chroma) {
    if (!vsyn_spectral_chroma_dim(&opts.spectral, chroma)) return refuse(fn, "invalid spectral or chroma spec");
    if (chroma) {
      opts.chroma_given = true;
      opts.chroma_spec = *chroma;
    }
  }
  void chroma_estimate(const vsyn_tuning_spec* estimate) {
    if (!estimate) return;
    vsyn_spectral_spec lin = opts.spectral;
    lin.kind = VSYN_SPEC_LIN_POWER;
    const char* why = nullptr;
    if (opts.spectral.kind != VSYN_SPEC_CHROMA && opts.spectral.kind != VSYN_SPEC_TONNETZ) return refuse(fn, "a tuning estimate is for the chroma kinds");
    if (vsyn_tuning_check(&lin, estimate, &why) != VSYN_OK) return refuse(fn, why ? why : "invalid tuning spec");
    opts.chroma_estimate = true;
    opts.chroma_estimate_spec = *estimate;
  }
  void hpss(const vsyn_spectral_hpss* hpss) {
    if (!hpss) return;
    opts.hpss = true;
    opts.hpss_spec = *hpss;
  }
  void pcen(const vsyn_spectral_pcen* pcen) {
    if (!pcen) return;
    opts.pcen = true;
    opts.pcen_spec = *pcen;
  }
  void rhythm(const vsyn_rhythm_spec* rhythm) {
    if (post_run(opts)) return refuse(fn, "delta / normalize are not available with the rhythm stages");
    if (rhythm->output > VSYN_RHYTHM_TEMPO_MEAN || (rhythm->output == VSYN_RHYTHM_TEMPOGRAM && !vsyn_tempogram_tile(rhythm->tempogram.win_length)))
      return refuse(fn, "unknown rhythm output, or tempogram rows without a win_length in [2, 2048]");
    opts.rhythm = true;
    opts.rhythm_spec = *rhythm;
  }
  void beat(const vsyn_onset_spec* onset, const vsyn_beat_spec* beat) {
    if (post_run(opts)) return refuse(fn, "delta / normalize are not available with the beat tracker");
    opts.beat = true;
    opts.beat_onset = *onset;
    opts.beat_spec = *beat;
  }
  void pcm_format(int format, uint32_t target_rate) {
    if (format != VSYN_PCM_F32 && format != VSYN_PCM_S16) return refuse("ogg_vorbis_pcm_corpus", "unknown PCM format " + std::to_string(format));
    opts.pcm_s16 = format == VSYN_PCM_S16;
    opts.resample_rate = target_rate;
  }
  void cond(const vsyn_pcm_cond* cond) {
    if (!cond) return;
    opts.condition = true;
    opts.cond = *cond;
  }
  // the gate: a trim, or with is_split a split in its place; the output is then the trimmed or the joined mono plane
  void gate(const vsyn_pcm_trim* gate, bool is_split) {
    if (!gate) return;
    if (!vsyn_pcm_trim_num_frames(gate, 1))
      return is_split ? refuse("ogg_vorbis_pcm_corpus_split", "invalid split spec") : refuse("ogg_vorbis_pcm_corpus_trim", "invalid trim spec");
    opts.condition = true;
    (is_split ? opts.split : opts.trim) = true;
    opts.trim_spec = *gate;
  }
  // the stages behind the gate; each makes a PCM call deliver one mono plane per file
  void loud(const vsyn_loudness_spec* loud) {
    if (!loud) return;
    if (!loud_norm_spec_ok(loud, opts.condition ? &opts.cond : nullptr))
      return refuse("ogg_vorbis_pcm_corpus_loud", "invalid loudness spec (a target in [-70, 0], the mono downmix, no peak)");
    if (!fn) opts.condition = true;
    opts.loudness_norm = true;
    opts.loudness_spec = *loud;
  }
  void effect(const vsyn_pcm_effect* effect) {
    if (!effect) return;
    if (!effect_spec_ok(effect))
      return refuse("ogg_vorbis_pcm_corpus_effects",
                    "invalid effect spec (n_fft a power of two in [16, 8192], hop_length >= 1, win_length in [1, n_fft], odd kernel sizes up to 63, "
                    "the component as output)");
    opts.condition = opts.effect = true;
    opts.effect_spec = *effect;
  }
  void stretch(const vsyn_pcm_stretch* stretch, const double* stretch_rates, const uint32_t* shift_from_hz) {
    if (!stretch) return;
    if (std::string why = stretch_refusal(stretch, num_files, stretch_rates, shift_from_hz); !why.empty() || opts.effect)
      return refuse("ogg_vorbis_pcm_corpus_stretch", opts.effect ? std::string("a stretch and an hpss effect in one call are not built") : why);
    opts.condition = opts.stretch = true;
    opts.stretch_spec = *stretch;
    opts.stretch_rates = stretch_rates;
    opts.stretch_from_hz = shift_from_hz;
  }

  // The run, or the refusal, and what both leave in the outputs. The joined frames and the intervals are a split run's.
  template <typename PerFile>
  int run(const char* name, PerFile per_file) {
    if (!refusal.empty()) return refuse_call(out, num_files, refusal, error_out);
    const int rc = malloc_corpus(name, datas, lens, num_files, opts, out, ok_out, error_out_per_file, stats_out, error_out,
                                 [&](size_t i, const CorpusFileResult& res, bool bad) {
                                   per_file(i, res, bad);
                                   if (records_out) records_out[i] = bad ? NO_LOUDNESS_RECORD : res.loudness;
                                   give_bounds(bounds_out, i, res, bad);
                                   if (opts.split) give_intervals(split.intervals_out, split.intervals_count_out, i, res, bad);
                                 });
    if (rc) split.clear(num_files);
    return rc;
  }
  int rows(const char* name = "spectral") {  // a rows run (features or spectral, as set in opts)
    return run(name, [&](size_t i, const CorpusFileResult& res, bool bad) {
      if (rows_count_out) rows_count_out[i] = res.feature_rows;
      if (opts.split && split.frames_out) split.frames_out[i] = bad ? 0 : res.frames;
      if (opts.beat && bpm_out) bpm_out[i] = bad ? 0.0 : res.bpm;
      if (opts.beat && rate_out) rate_out[i] = res.sample_rate;
      if (tuning_out) tuning_out[i] = bad ? 0.0 : res.tuning;
    });
  }
  int pcm() {
    return run("pcm", [&](size_t i, const CorpusFileResult& res, bool bad) {
      if (frames_out) frames_out[i] = bad ? 0 : res.frames;
      if (channels_out) channels_out[i] = res.channels;
      if (rate_out) rate_out[i] = res.sample_rate;
    });
  }
};

}  // namespace

extern "C" int ogg_vorbis_features_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                          uint32_t files_per_submit, int device, const vsyn_feature_spec* spec, float** rows_out,
                                          uint64_t* rows_count_out, uint8_t* ok_out, const char** error_out_per_file,
                                          double* stats_out, const char** error_out) {
  if (!spec || spec->kind == 0) return refuse_call((void**)rows_out, num_files, "ogg_vorbis_features_corpus: no feature kind", error_out);
  CorpusCall c("ogg_vorbis_features_corpus", datas, lens, num_files, threads, feeders, files_per_submit, device, (void**)rows_out, ok_out,
               error_out_per_file, stats_out, error_out);
  c.rows_count_out = rows_count_out;
  c.opts.features = *spec;
  return c.rows("features");
}

extern "C" int ogg_vorbis_spectral_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                          uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, float** rows_out,
                                          uint64_t* rows_count_out, uint8_t* ok_out, const char** error_out_per_file,
                                          double* stats_out, const char** error_out) {
  CorpusCall c("ogg_vorbis_spectral_corpus", datas, lens, num_files, threads, feeders, files_per_submit, device, (void**)rows_out, ok_out,
               error_out_per_file, stats_out, error_out);
  c.rows_count_out = rows_count_out;
  c.spectral(spec, 0, nullptr);
  return c.rows();
}

extern "C" int ogg_vorbis_spectral_corpus_sr(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                             uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, uint32_t target_rate,
                                             float** rows_out, uint64_t* rows_count_out, uint8_t* ok_out, const char** error_out_per_file,
                                             double* stats_out, const char** error_out) {
  CorpusCall c("ogg_vorbis_spectral_corpus_sr", datas, lens, num_files, threads, feeders, files_per_submit, device, (void**)rows_out, ok_out,
               error_out_per_file, stats_out, error_out);
  c.rows_count_out = rows_count_out;
  c.spectral(spec, target_rate, nullptr);
  return c.rows();
}

extern "C" int ogg_vorbis_spectral_corpus_post(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                               uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, uint32_t target_rate,
                                               const vsyn_spectral_post* post, float** rows_out, uint64_t* rows_count_out, uint8_t* ok_out,
                                               const char** error_out_per_file, double* stats_out, const char** error_out) {
  if (!post) return refuse_call((void**)rows_out, num_files, "ogg_vorbis_spectral_corpus_post: no post spec", error_out);
  CorpusCall c("ogg_vorbis_spectral_corpus_post", datas, lens, num_files, threads, feeders, files_per_submit, device, (void**)rows_out, ok_out,
               error_out_per_file, stats_out, error_out);
  c.rows_count_out = rows_count_out;
  c.spectral(spec, target_rate, post);
  return c.rows();
}

extern "C" int ogg_vorbis_spectral_corpus_cond(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                               uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, uint32_t target_rate,
                                               const vsyn_spectral_post* post, const vsyn_pcm_cond* cond, float** rows_out,
                                               uint64_t* rows_count_out, uint8_t* ok_out, const char** error_out_per_file, double* stats_out,
                                               const char** error_out) {
  CorpusCall c("ogg_vorbis_spectral_corpus_cond", datas, lens, num_files, threads, feeders, files_per_submit, device, (void**)rows_out, ok_out,
               error_out_per_file, stats_out, error_out);
  c.rows_count_out = rows_count_out;
  c.spectral(spec, target_rate, post);
  c.cond(cond);
  return c.rows();
}

extern "C" int ogg_vorbis_spectral_corpus_trim(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                               uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, uint32_t target_rate,
                                               const vsyn_spectral_post* post, const vsyn_pcm_cond* cond, const vsyn_pcm_trim* trim,
                                               float** rows_out, uint64_t* rows_count_out, uint64_t* bounds_out, uint8_t* ok_out,
                                               const char** error_out_per_file, double* stats_out, const char** error_out) {
  CorpusCall c("ogg_vorbis_spectral_corpus_trim", datas, lens, num_files, threads, feeders, files_per_submit, device, (void**)rows_out, ok_out,
               error_out_per_file, stats_out, error_out);
  c.rows_count_out = rows_count_out;
  c.bounds_out = bounds_out;
  c.spectral(spec, target_rate, post);
  c.cond(cond);
  c.gate(trim, false);
  return c.rows();
}

extern "C" int ogg_vorbis_pcm_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                     uint32_t files_per_submit, int device, uint32_t target_rate, int format, void** pcm_out, uint64_t* frames_out,
                                     uint32_t* channels_out, uint32_t* rate_out, uint8_t* ok_out, const char** error_out_per_file,
                                     double* stats_out, const char** error_out) {
  return ogg_vorbis_pcm_corpus_cond(datas, lens, num_files, threads, feeders, files_per_submit, device, target_rate, format, nullptr, pcm_out,
                                    frames_out, channels_out, rate_out, ok_out, error_out_per_file, stats_out, error_out);
}

extern "C" int ogg_vorbis_pcm_corpus_cond(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                          uint32_t files_per_submit, int device, uint32_t target_rate, int format, const vsyn_pcm_cond* cond,
                                          void** pcm_out, uint64_t* frames_out, uint32_t* channels_out, uint32_t* rate_out, uint8_t* ok_out,
                                          const char** error_out_per_file, double* stats_out, const char** error_out) {
  return ogg_vorbis_pcm_corpus_trim(datas, lens, num_files, threads, feeders, files_per_submit, device, target_rate, format, cond, nullptr,
                                    pcm_out, frames_out, channels_out, rate_out, nullptr, ok_out, error_out_per_file, stats_out, error_out);
}

extern "C" int ogg_vorbis_pcm_corpus_trim(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                          uint32_t files_per_submit, int device, uint32_t target_rate, int format, const vsyn_pcm_cond* cond,
                                          const vsyn_pcm_trim* trim, void** pcm_out, uint64_t* frames_out, uint32_t* channels_out,
                                          uint32_t* rate_out, uint64_t* bounds_out, uint8_t* ok_out, const char** error_out_per_file,
                                          double* stats_out, const char** error_out) {
  CorpusCall c(nullptr, datas, lens, num_files, threads, feeders, files_per_submit, device, pcm_out, ok_out, error_out_per_file, stats_out, error_out);
  c.frames_out = frames_out;
  c.channels_out = channels_out;
  c.rate_out = rate_out;
  c.bounds_out = bounds_out;
  c.pcm_format(format, target_rate);
  c.cond(cond);
  c.gate(trim, false);
  return c.pcm();
}

extern "C" int ogg_vorbis_pcm_corpus_split(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                           uint32_t files_per_submit, int device, uint32_t target_rate, int format, const vsyn_pcm_cond* cond,
                                           const vsyn_pcm_trim* split, void** pcm_out, uint64_t* frames_out, uint32_t* channels_out,
                                           uint32_t* rate_out, uint32_t** intervals_out, uint64_t* intervals_count_out, uint8_t* ok_out,
                                           const char** error_out_per_file, double* stats_out, const char** error_out) {
  CorpusCall c(nullptr, datas, lens, num_files, threads, feeders, files_per_submit, device, pcm_out, ok_out, error_out_per_file, stats_out, error_out);
  c.frames_out = frames_out;
  c.channels_out = channels_out;
  c.rate_out = rate_out;
  c.split_outputs(nullptr, intervals_out, intervals_count_out, true);
  c.pcm_format(format, target_rate);
  c.cond(cond);
  c.gate(split, true);
  return c.pcm();
}

extern "C" int ogg_vorbis_spectral_corpus_split(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                                uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, uint32_t target_rate,
                                                const vsyn_spectral_post* post, const vsyn_pcm_cond* cond, const vsyn_pcm_trim* split,
                                                float** rows_out, uint64_t* rows_count_out, uint64_t* frames_out, uint32_t** intervals_out,
                                                uint64_t* intervals_count_out, uint8_t* ok_out, const char** error_out_per_file,
                                                double* stats_out, const char** error_out) {
  CorpusCall c("ogg_vorbis_spectral_corpus_split", datas, lens, num_files, threads, feeders, files_per_submit, device, (void**)rows_out, ok_out,
               error_out_per_file, stats_out, error_out);
  c.rows_count_out = rows_count_out;
  c.split_outputs(frames_out, intervals_out, intervals_count_out, true);  // (split = NULL: frames_out keeps the caller's bytes)
  c.spectral(spec, target_rate, post);
  c.cond(cond);
  c.gate(split, true);
  return c.rows();
}

extern "C" int ogg_vorbis_spectral_corpus_pcen(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                               uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, uint32_t target_rate,
                                               const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post, const vsyn_pcm_cond* cond,
                                               const vsyn_pcm_trim* gate, int gate_is_split, float** rows_out, uint64_t* rows_count_out,
                                               uint64_t* bounds_out, uint64_t* frames_out, uint32_t** intervals_out,
                                               uint64_t* intervals_count_out, uint8_t* ok_out, const char** error_out_per_file,
                                               double* stats_out, const char** error_out) {
  CorpusCall c("ogg_vorbis_spectral_corpus_pcen", datas, lens, num_files, threads, feeders, files_per_submit, device, (void**)rows_out, ok_out,
               error_out_per_file, stats_out, error_out);
  const bool split = gate && gate_is_split;
  c.rows_count_out = rows_count_out;
  c.bounds_out = bounds_out;
  c.split_outputs(frames_out, intervals_out, intervals_count_out, split);
  c.spectral(spec, target_rate, post);
  c.pcen(pcen);
  c.cond(cond);
  c.gate(gate, split);
  return c.rows();
}

extern "C" int ogg_vorbis_intervals_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                           uint32_t files_per_submit, int device, uint32_t target_rate, const vsyn_pcm_trim* split,
                                           uint32_t** intervals_out, uint64_t* intervals_count_out, uint64_t* frames_out, uint32_t* rate_out,
                                           uint8_t* ok_out, const char** error_out_per_file, double* stats_out, const char** error_out) {
  CorpusCall c(nullptr, datas, lens, num_files, threads, feeders, files_per_submit, device, nullptr, ok_out, error_out_per_file, stats_out, error_out);
  c.frames_out = frames_out;
  c.rate_out = rate_out;
  c.split_outputs(nullptr, intervals_out, intervals_count_out, true);
  if (!split) c.refuse("ogg_vorbis_intervals_corpus", "no split spec");
  c.pcm_format(VSYN_PCM_F32, target_rate);
  c.gate(split, true);
  c.opts.intervals_only = true;  // no joined plane is made, and no PCM is delivered
  return c.pcm();
}

extern "C" int ogg_vorbis_pitch_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                       uint32_t files_per_submit, int device, uint32_t target_rate, const vsyn_pitch_spec* spec, float** rows_out,
                                       uint64_t* rows_count_out, uint64_t* frames_out, uint32_t* rate_out, uint8_t* ok_out,
                                       const char** error_out_per_file, double* stats_out, const char** error_out) {
  if (!spec || !vsyn_pitch_num_frames(spec, 0x7FFFFFFFu))
    return refuse_call((void**)rows_out, num_files, "ogg_vorbis_pitch_corpus: invalid pitch spec", error_out);
  CorpusOptions opts = call_options(threads, feeders, files_per_submit, device);
  opts.pitch = *spec;
  opts.resample_rate = target_rate;
  return malloc_corpus("pitch", datas, lens, num_files, opts, (void**)rows_out, ok_out, error_out_per_file, stats_out, error_out,
                       [&](size_t i, const CorpusFileResult& res, bool bad) {
                         if (rows_count_out) rows_count_out[i] = bad ? 0 : res.feature_rows;
                         if (frames_out) frames_out[i] = bad ? 0 : res.frames;
                         if (rate_out) rate_out[i] = res.sample_rate;
                       });
}

extern "C" int ogg_vorbis_pyin_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                      uint32_t files_per_submit, int device, uint32_t target_rate, const vsyn_pyin_spec* spec, float** rows_out,
                                      uint64_t* rows_count_out, uint64_t* frames_out, uint32_t* rate_out, uint8_t* ok_out,
                                      const char** error_out_per_file, double* stats_out, const char** error_out) {
  if (!spec || !vsyn_pyin_num_frames(spec, 0x7FFFFFFFu))
    return refuse_call((void**)rows_out, num_files, "ogg_vorbis_pyin_corpus: invalid pyin spec", error_out);
  CorpusOptions opts = call_options(threads, feeders, files_per_submit, device);
  opts.pyin = *spec;
  opts.resample_rate = target_rate;
  return malloc_corpus("pyin", datas, lens, num_files, opts, (void**)rows_out, ok_out, error_out_per_file, stats_out, error_out,
                       [&](size_t i, const CorpusFileResult& res, bool bad) {
                         if (rows_count_out) rows_count_out[i] = bad ? 0 : res.feature_rows;
                         if (frames_out) frames_out[i] = bad ? 0 : res.frames;
                         if (rate_out) rate_out[i] = res.sample_rate;
                       });
}

extern "C" int ogg_vorbis_fdesc_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                       uint32_t files_per_submit, int device, uint32_t target_rate, const vsyn_fdesc_spec* spec, float** rows_out,
                                       uint64_t* rows_count_out, uint64_t* frames_out, uint32_t* rate_out, uint8_t* ok_out,
                                       const char** error_out_per_file, double* stats_out, const char** error_out) {
  if (!spec || !vsyn_fdesc_num_frames(spec, 0x7FFFFFFFu))
    return refuse_call((void**)rows_out, num_files, "ogg_vorbis_fdesc_corpus: invalid frame descriptor spec", error_out);
  CorpusOptions opts = call_options(threads, feeders, files_per_submit, device);
  opts.fdesc = *spec;
  opts.resample_rate = target_rate;
  return malloc_corpus("fdesc", datas, lens, num_files, opts, (void**)rows_out, ok_out, error_out_per_file, stats_out, error_out,
                       [&](size_t i, const CorpusFileResult& res, bool bad) {
                         if (rows_count_out) rows_count_out[i] = bad ? 0 : res.feature_rows;
                         if (frames_out) frames_out[i] = bad ? 0 : res.frames;
                         if (rate_out) rate_out[i] = res.sample_rate;
                       });
}

extern "C" int ogg_vorbis_cqt_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                     uint32_t files_per_submit, int device, uint32_t target_rate, const vsyn_cqt_spec* spec, float** rows_out,
                                     uint64_t* rows_count_out, uint64_t* frames_out, uint32_t* rate_out, uint8_t* ok_out,
                                     const char** error_out_per_file, double* stats_out, const char** error_out) {
  if (!spec || !vsyn_cqt_dim(spec)) return refuse_call((void**)rows_out, num_files, "ogg_vorbis_cqt_corpus: invalid constant-Q spec", error_out);
  CorpusOptions opts = call_options(threads, feeders, files_per_submit, device);
  opts.cqt = *spec;
  opts.resample_rate = target_rate;
  return malloc_corpus("cqt", datas, lens, num_files, opts, (void**)rows_out, ok_out, error_out_per_file, stats_out, error_out,
                       [&](size_t i, const CorpusFileResult& res, bool bad) {
                         if (rows_count_out) rows_count_out[i] = bad ? 0 : res.feature_rows;
                         if (frames_out) frames_out[i] = bad ? 0 : res.frames;
                         if (rate_out) rate_out[i] = res.sample_rate;
                       });
}

extern "C" int ogg_vorbis_cqt_corpus_est(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                         uint32_t files_per_submit, int device, uint32_t target_rate, const vsyn_cqt_spec* spec,
                                         const vsyn_tuning_spec* estimate, float** rows_out, uint64_t* rows_count_out, uint64_t* frames_out,
                                         uint32_t* rate_out, double* tuning_out, uint8_t* ok_out, const char** error_out_per_file,
                                         double* stats_out, const char** error_out) {
  if (!spec || !vsyn_cqt_dim(spec)) return refuse_call((void**)rows_out, num_files, "ogg_vorbis_cqt_corpus_est: invalid constant-Q spec", error_out);
  CorpusOptions opts = call_options(threads, feeders, files_per_submit, device);
  if (estimate) {
    const vsyn_spectral_spec lin = {VSYN_SPEC_LIN_POWER, VSYN_SPEC_CENTER, 2048u, 512u, 2048u, 0u, 0u, 1u, 0.0, 0.0, 0.0, 0.0, 0.0};
    const char* why = nullptr;
    if (vsyn_tuning_check(&lin, estimate, &why) != VSYN_OK || estimate->bins_per_octave != spec->bins_per_octave)
      return refuse_call((void**)rows_out, num_files,
                         std::string("ogg_vorbis_cqt_corpus_est: ") + (why ? why : "the estimate's bins_per_octave is not the transform's"), error_out);
    opts.cqt_estimate = true;
    opts.cqt_estimate_spec = *estimate;
  }
  opts.cqt = *spec;
  opts.resample_rate = target_rate;
  return malloc_corpus("cqt", datas, lens, num_files, opts, (void**)rows_out, ok_out, error_out_per_file, stats_out, error_out,
                       [&](size_t i, const CorpusFileResult& res, bool bad) {
                         if (rows_count_out) rows_count_out[i] = bad ? 0 : res.feature_rows;
                         if (frames_out) frames_out[i] = bad ? 0 : res.frames;
                         if (rate_out) rate_out[i] = res.sample_rate;
                         if (estimate && tuning_out) tuning_out[i] = bad ? 0.0 : res.tuning;
                       });
}

extern "C" int ogg_vorbis_tuning_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                        uint32_t files_per_submit, int device, uint32_t target_rate, const vsyn_spectral_spec* spec,
                                        const vsyn_tuning_spec* tun, int want_rows, float** rows_out, uint64_t* rows_count_out,
                                        uint64_t* frames_out, uint32_t* rate_out, double* tuning_out, uint64_t* counts_out, uint8_t* ok_out,
                                        const char** error_out_per_file, double* stats_out, const char** error_out) {
  const char* why = nullptr;
  if (!spec || !tun || vsyn_tuning_check(spec, tun, &why) != VSYN_OK)
    return refuse_call((void**)rows_out, num_files, std::string("ogg_vorbis_tuning_corpus: ") + (why ? why : "invalid spec"), error_out);
  if (want_rows && !rows_out) return refuse_call(nullptr, num_files, "ogg_vorbis_tuning_corpus: rows wanted, rows_out NULL", error_out);
  CorpusOptions opts = call_options(threads, feeders, files_per_submit, device);
  opts.tuning_framing = *spec;
  opts.tuning = *tun;
  opts.tuning_rows = want_rows != 0;
  opts.resample_rate = target_rate;
  return malloc_corpus("tuning", datas, lens, num_files, opts, (void**)rows_out, ok_out, error_out_per_file, stats_out, error_out,
                       [&](size_t i, const CorpusFileResult& res, bool bad) {
                         if (rows_count_out) rows_count_out[i] = bad ? 0 : res.feature_rows;
                         if (frames_out) frames_out[i] = bad ? 0 : res.frames;
                         if (rate_out) rate_out[i] = res.sample_rate;
                         if (tuning_out) tuning_out[i] = bad ? 0.0 : res.tuning;
                         if (counts_out) {
                           counts_out[2 * i] = bad ? 0 : res.tuning_counts[0];
                           counts_out[2 * i + 1] = bad ? 0 : res.tuning_counts[1];
                         }
                       });
}

extern "C" int ogg_vorbis_pcm_corpus_loud(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                          uint32_t files_per_submit, int device, uint32_t target_rate, int format, const vsyn_pcm_cond* cond,
                                          const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud, void** pcm_out,
                                          uint64_t* frames_out, uint32_t* channels_out, uint32_t* rate_out, uint64_t* bounds_out,
                                          uint32_t** intervals_out, uint64_t* intervals_count_out, vsyn_loudness_record* records_out,
                                          uint8_t* ok_out, const char** error_out_per_file, double* stats_out, const char** error_out) {
  return ogg_vorbis_pcm_corpus_effects(datas, lens, num_files, threads, feeders, files_per_submit, device, target_rate, format, cond, gate, gate_is_split,
                                       nullptr, loud, pcm_out, frames_out, channels_out, rate_out, bounds_out, intervals_out, intervals_count_out,
                                       records_out, ok_out, error_out_per_file, stats_out, error_out);
}

extern "C" int ogg_vorbis_pcm_corpus_effects(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                             uint32_t files_per_submit, int device, uint32_t target_rate, int format, const vsyn_pcm_cond* cond,
                                             const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_pcm_effect* effect,
                                             const vsyn_loudness_spec* loud, void** pcm_out, uint64_t* frames_out, uint32_t* channels_out,
                                             uint32_t* rate_out, uint64_t* bounds_out, uint32_t** intervals_out, uint64_t* intervals_count_out,
                                             vsyn_loudness_record* records_out, uint8_t* ok_out, const char** error_out_per_file,
                                             double* stats_out, const char** error_out) {
  return ogg_vorbis_pcm_corpus_stretch(datas, lens, num_files, threads, feeders, files_per_submit, device, target_rate, format, cond, gate, gate_is_split,
                                       effect, nullptr, nullptr, nullptr, loud, pcm_out, frames_out, channels_out, rate_out, bounds_out, intervals_out,
                                       intervals_count_out, records_out, ok_out, error_out_per_file, stats_out, error_out);
}

extern "C" int ogg_vorbis_pcm_corpus_stretch(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                             uint32_t files_per_submit, int device, uint32_t target_rate, int format, const vsyn_pcm_cond* cond,
                                             const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_pcm_effect* effect,
                                             const vsyn_pcm_stretch* stretch, const double* stretch_rates, const uint32_t* shift_from_hz,
                                             const vsyn_loudness_spec* loud, void** pcm_out, uint64_t* frames_out, uint32_t* channels_out,
                                             uint32_t* rate_out, uint64_t* bounds_out, uint32_t** intervals_out, uint64_t* intervals_count_out,
                                             vsyn_loudness_record* records_out, uint8_t* ok_out, const char** error_out_per_file,
                                             double* stats_out, const char** error_out) {
  CorpusCall c(nullptr, datas, lens, num_files, threads, feeders, files_per_submit, device, pcm_out, ok_out, error_out_per_file, stats_out, error_out);
  const bool split = gate && gate_is_split;
  c.frames_out = frames_out;
  c.channels_out = channels_out;
  c.rate_out = rate_out;
  c.bounds_out = bounds_out;
  c.records_out = records_out;
  c.split_outputs(nullptr, intervals_out, intervals_count_out, split);
  c.pcm_format(format, target_rate);
  c.cond(cond);
  c.gate(gate, split);
  c.loud(loud);
  c.effect(effect);
  c.stretch(stretch, stretch_rates, shift_from_hz);
  return c.pcm();
}

extern "C" int ogg_vorbis_spectral_corpus_loud(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                               uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, uint32_t target_rate,
                                               const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post, const vsyn_pcm_cond* cond,
                                               const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud, float** rows_out,
                                               uint64_t* rows_count_out, uint64_t* bounds_out, uint64_t* frames_out, uint32_t** intervals_out,
                                               uint64_t* intervals_count_out, vsyn_loudness_record* records_out, uint8_t* ok_out,
                                               const char** error_out_per_file, double* stats_out, const char** error_out) {
  CorpusCall c("ogg_vorbis_spectral_corpus_loud", datas, lens, num_files, threads, feeders, files_per_submit, device, (void**)rows_out, ok_out,
               error_out_per_file, stats_out, error_out);
  const bool split = gate && gate_is_split;
  c.rows_count_out = rows_count_out;
  c.bounds_out = bounds_out;
  c.records_out = records_out;
  c.split_outputs(frames_out, intervals_out, intervals_count_out, split);
  c.spectral(spec, target_rate, post);
  c.pcen(pcen);
  c.cond(cond);
  c.gate(gate, split);
  c.loud(loud);
  return c.rows();
}

extern "C" int ogg_vorbis_spectral_corpus_chroma(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                                 uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec,
                                                 const vsyn_spectral_chroma* chroma, uint32_t target_rate, const vsyn_spectral_pcen* pcen,
                                                 const vsyn_spectral_post* post, const vsyn_pcm_cond* cond, const vsyn_pcm_trim* gate,
                                                 int gate_is_split, const vsyn_loudness_spec* loud, float** rows_out, uint64_t* rows_count_out,
                                                 uint64_t* bounds_out, uint64_t* frames_out, uint32_t** intervals_out,
                                                 uint64_t* intervals_count_out, vsyn_loudness_record* records_out, uint8_t* ok_out,
                                                 const char** error_out_per_file, double* stats_out, const char** error_out) {
  CorpusCall c("ogg_vorbis_spectral_corpus_chroma", datas, lens, num_files, threads, feeders, files_per_submit, device, (void**)rows_out, ok_out,
               error_out_per_file, stats_out, error_out);
  const bool split = gate && gate_is_split;
  c.rows_count_out = rows_count_out;
  c.bounds_out = bounds_out;
  c.records_out = records_out;
  c.split_outputs(frames_out, intervals_out, intervals_count_out, split);
  c.spectral(spec, target_rate, post);
  c.chroma(chroma);
  c.pcen(pcen);
  c.cond(cond);
  c.gate(gate, split);
  c.loud(loud);
  return c.rows();
}

extern "C" int ogg_vorbis_spectral_corpus_chroma_est(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                                     uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec,
                                                     const vsyn_spectral_chroma* chroma, uint32_t target_rate, const vsyn_spectral_pcen* pcen,
                                                     const vsyn_spectral_post* post, const vsyn_pcm_cond* cond, const vsyn_pcm_trim* gate,
                                                     int gate_is_split, const vsyn_loudness_spec* loud, const vsyn_tuning_spec* estimate,
                                                     float** rows_out, uint64_t* rows_count_out, uint64_t* bounds_out, uint64_t* frames_out,
                                                     uint32_t** intervals_out, uint64_t* intervals_count_out, vsyn_loudness_record* records_out,
                                                     double* tuning_out, uint8_t* ok_out, const char** error_out_per_file, double* stats_out,
                                                     const char** error_out) {
  CorpusCall c("ogg_vorbis_spectral_corpus_chroma_est", datas, lens, num_files, threads, feeders, files_per_submit, device, (void**)rows_out,
               ok_out, error_out_per_file, stats_out, error_out);
  const bool split = gate && gate_is_split;
  c.rows_count_out = rows_count_out;
  c.bounds_out = bounds_out;
  c.records_out = records_out;
  c.tuning_out = estimate ? tuning_out : nullptr;
  c.split_outputs(frames_out, intervals_out, intervals_count_out, split);
  c.spectral(spec, target_rate, post);
  c.chroma(chroma);
  c.chroma_estimate(estimate);
  c.pcen(pcen);
  c.cond(cond);
  c.gate(gate, split);
  c.loud(loud);
  return c.rows();
}

extern "C" int ogg_vorbis_spectral_corpus_hpss(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                               uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec,
                                               const vsyn_spectral_chroma* chroma, uint32_t target_rate, const vsyn_spectral_hpss* hpss,
                                               const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post, const vsyn_pcm_cond* cond,
                                               const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud, float** rows_out,
                                               uint64_t* rows_count_out, uint64_t* bounds_out, uint64_t* frames_out, uint32_t** intervals_out,
                                               uint64_t* intervals_count_out, vsyn_loudness_record* records_out, uint8_t* ok_out,
                                               const char** error_out_per_file, double* stats_out, const char** error_out) {
  CorpusCall c("ogg_vorbis_spectral_corpus_hpss", datas, lens, num_files, threads, feeders, files_per_submit, device, (void**)rows_out, ok_out,
               error_out_per_file, stats_out, error_out);
  const bool split = gate && gate_is_split;
  c.rows_count_out = rows_count_out;
  c.bounds_out = bounds_out;
  c.records_out = records_out;
  c.split_outputs(frames_out, intervals_out, intervals_count_out, split);
  c.spectral(spec, target_rate, post);
  c.chroma(chroma);
  c.pcen(pcen);
  c.hpss(hpss);
  c.cond(cond);
  c.gate(gate, split);
  c.loud(loud);
  return c.rows();
}

extern "C" int ogg_vorbis_rhythm_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                        uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma,
                                        uint32_t target_rate, const vsyn_spectral_hpss* hpss, const vsyn_spectral_pcen* pcen,
                                        const vsyn_spectral_post* post, const vsyn_rhythm_spec* rhythm, const vsyn_pcm_cond* cond,
                                        const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud, float** rows_out,
                                        uint64_t* rows_count_out, uint64_t* bounds_out, uint64_t* frames_out, uint32_t** intervals_out,
                                        uint64_t* intervals_count_out, vsyn_loudness_record* records_out, uint8_t* ok_out,
                                        const char** error_out_per_file, double* stats_out, const char** error_out) {
  if (!rhythm) return refuse_call((void**)rows_out, num_files, "ogg_vorbis_rhythm_corpus: no rhythm spec", error_out);
  CorpusCall c("ogg_vorbis_rhythm_corpus", datas, lens, num_files, threads, feeders, files_per_submit, device, (void**)rows_out, ok_out,
               error_out_per_file, stats_out, error_out);
  const bool split = gate && gate_is_split;
  c.rows_count_out = rows_count_out;
  c.bounds_out = bounds_out;
  c.records_out = records_out;
  c.split_outputs(frames_out, intervals_out, intervals_count_out, split);
  c.spectral(spec, target_rate, post);
  c.chroma(chroma);
  c.pcen(pcen);
  c.hpss(hpss);
  c.rhythm(rhythm);
  c.cond(cond);
  c.gate(gate, split);
  c.loud(loud);
  return c.rows();
}

extern "C" int ogg_vorbis_beats_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                       uint32_t files_per_submit, int device, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma,
                                       uint32_t target_rate, const vsyn_spectral_hpss* hpss, const vsyn_spectral_pcen* pcen,
                                       const vsyn_spectral_post* post, const vsyn_onset_spec* onset, const vsyn_beat_spec* beat,
                                       const vsyn_pcm_cond* cond, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud,
                                       float** rows_out, uint64_t* rows_count_out, double* bpm_out, uint32_t* rate_out, uint64_t* bounds_out,
                                       uint64_t* frames_out, uint32_t** intervals_out, uint64_t* intervals_count_out,
                                       vsyn_loudness_record* records_out, uint8_t* ok_out, const char** error_out_per_file, double* stats_out,
                                       const char** error_out) {
  if (!onset || !beat) return refuse_call((void**)rows_out, num_files, "ogg_vorbis_beats_corpus: no onset or no beat spec", error_out);
  CorpusCall c("ogg_vorbis_beats_corpus", datas, lens, num_files, threads, feeders, files_per_submit, device, (void**)rows_out, ok_out,
               error_out_per_file, stats_out, error_out);
  const bool split = gate && gate_is_split;
  c.rows_count_out = rows_count_out;
  c.bounds_out = bounds_out;
  c.records_out = records_out;
  c.bpm_out = bpm_out;
  c.rate_out = rate_out;
  c.split_outputs(frames_out, intervals_out, intervals_count_out, split);
  c.spectral(spec, target_rate, post);
  c.chroma(chroma);
  c.pcen(pcen);
  c.hpss(hpss);
  c.beat(onset, beat);
  c.cond(cond);
  c.gate(gate, split);
  c.loud(loud);
  return c.rows();
}

extern "C" int ogg_vorbis_loudness_corpus(const uint8_t* const* datas, const size_t* lens, size_t num_files, int threads, int feeders,
                                          uint32_t files_per_submit, int device, uint32_t target_rate, const vsyn_loudness_spec* spec,
                                          int want_blocks, double** blocks_out, uint64_t* blocks_count_out, vsyn_loudness_record* records_out,
                                          uint64_t* frames_out, uint32_t* rate_out, uint8_t* ok_out, const char** error_out_per_file,
                                          double* stats_out, const char** error_out) {
  if (!spec || (spec->options & ~VSYN_LOUD_NORMALIZE) || spec->channel_mode > VSYN_LOUD_MONO ||
      ((spec->options & VSYN_LOUD_NORMALIZE) && !(spec->target >= -70.0 && spec->target <= 0.0)))
    return refuse_call((void**)blocks_out, num_files, "ogg_vorbis_loudness_corpus: invalid loudness spec", error_out);
  if (want_blocks && !blocks_out) return refuse_call(nullptr, num_files, "ogg_vorbis_loudness_corpus: blocks wanted, blocks_out NULL", error_out);
  CorpusOptions opts = call_options(threads, feeders, files_per_submit, device);
  opts.loudness = true;
  opts.loudness_blocks = want_blocks != 0;
  opts.loudness_spec = *spec;
  opts.resample_rate = target_rate;
  return malloc_corpus("loudness", datas, lens, num_files, opts, (void**)blocks_out, ok_out, error_out_per_file, stats_out, error_out,
                       [&](size_t i, const CorpusFileResult& res, bool bad) {
                         if (records_out) records_out[i] = bad ? NO_LOUDNESS_RECORD : res.loudness;
                         if (frames_out) frames_out[i] = bad ? 0 : res.frames;
                         if (rate_out) rate_out[i] = res.sample_rate;
                         const size_t n = bad || !want_blocks ? 0 : res.loudness_blocks.size();
                         if (blocks_count_out) blocks_count_out[i] = n;
                         if (n && blocks_out) {
                           blocks_out[i] = (double*)malloc(n * sizeof(double));
                           if (blocks_out[i]) memcpy(blocks_out[i], res.loudness_blocks.data(), n * sizeof(double));
                           else if (blocks_count_out) blocks_count_out[i] = 0;
                         }
                       });
}

extern "C" void ogg_vorbis_features_free(float* rows) { free(rows); }
