// vorbis_synth_hip.hip — host side of the C-ABI in include/vorbis_synth_hip.h + kernel launches.
// gfx950 (MI355X) only; built by __graft_entry__.build() with
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC
// No CPU compute path exists in this library: without a HIP device every entry point returns
// VSYN_ERR_NO_DEVICE.  The only host arithmetic is the once-per-stream constant block (twiddles, windows,
// floor neighbour tables), which the reference also builds once per stream (mdct.cpp:88-127, hpp:837-862).
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include <stdlib.h>

#include "vsyn_host.h"
#include "vsyn_device.h"
#include "vsyn_staged.h"
#include "vsyn_prep.h"
#include "vsyn_fused.h"
#include "vsyn_fused_u.h"
#include "vsyn_vq.h"
#include "vsyn_pcm.h"
#include "vsyn_features.h"
#include "vsyn_spectral.h"
#include "vsyn_spectral_lin.h"
#include "vsyn_chroma.h"
#include "vsyn_spectral_post.h"
#include "vsyn_pcen.h"
#include "vsyn_hpss.h"
#include "vsyn_istft.h"
#include "vsyn_effects.h"
#include "vsyn_pv.h"
#include "vsyn_rhythm.h"
#include "vsyn_beat.h"
#include "vsyn_loudness.h"
#include "vsyn_resample.h"
#include "vsyn_stretch.h"
#include "vsyn_condition.h"
#include "vsyn_trim.h"
#include "vsyn_split.h"
#include "vsyn_pitch.h"
#include "vsyn_pyin.h"
#include "vsyn_fdesc.h"
#include "vsyn_cqt.h"

static const uint32_t k_inverse_db_bits[256] = {
#include "vorbis_floor1_inverse_db.inc"
};

// Knobs that tests and stress tools use to force cases (tools/README.md): read from the environment once per handle, in vsyn_create.
struct Options {
  uint32_t run_len = 0;           // VSYN_RUN_LEN=<R>: packets per run of the fused kernels (0: fused_pick_run_len plans it)
  bool vq_no_lds_tables = false;  // VSYN_VQ_NO_LDS_TABLES=1: the residue VQ kernel keeps its value tables in global memory
  uint32_t vq_grid = 0;           // VSYN_VQ_GRID=<n>: at most n workgroups of the residue VQ kernel (0: as many as are resident at once)
  bool debug = false;             // VSYN_DEBUG: the setup's kernel choices on stderr
};

static Options options_from_env() {
  Options o;
  const char* e = getenv("VSYN_RUN_LEN");
  if (e && atoi(e) > 0) o.run_len = (uint32_t)atoi(e);
  e = getenv("VSYN_VQ_NO_LDS_TABLES");
  o.vq_no_lds_tables = e && atoi(e);
  e = getenv("VSYN_VQ_GRID");
  if (e && atoi(e) > 0) o.vq_grid = (uint32_t)atoi(e);
  o.debug = getenv("VSYN_DEBUG") != nullptr;
  return o;
}

struct vsyn_handle {
  int device = 0;
  Options opt;
  ConstHeader H{};
  std::vector<uint8_t> host_const;
  uint8_t* d_const = nullptr;
  uint8_t* d_vq = nullptr;             // residue VQ stage: VqHeader, books, residues, maps, value pool (vsyn_attach_vq)
  uint32_t vq_lds_bytes = 0;           // dynamic LDS of the residue VQ kernel
  uint32_t vq_grid = 0;                // workgroups of the VQ kernel that are resident at once (its grid: every wave walks packets)
  uint32_t vq_waves = 1;               // waves per workgroup: 1, or (value tables shared in LDS) several
  bool vq_tables_in_lds = false;
  uint32_t last_S = 0, last_wb = 0;    // segments / workspace half of the most recent submit (vsyn_pcm_interleave_device)
  DevBuf<vsyn_vq_packet> st_vqpk;      // vsyn_submit_host_vq staging
  DevBuf<uint8_t> st_cls;
  DevBuf<uint16_t> st_ent;
  StreamState* d_state = nullptr;
  float* d_carry = nullptr;
  DevStatus* d_status = nullptr;
  FusedTables fused{};
  UTables utab{};
  uint32_t fused_mask = 0;             // what the layout kernel classifies by: bit 0 long-run kernel usable, bit 1 mixed-block runs fused too
  bool u_mixed = false;                // class-2 runs go to the size-generic kernel (vsyn_fused_u.h) instead of fused_run<.., MIXED>
  int num_cus = 256;
  hipStream_t host_stream = nullptr;   // vsyn_submit_host: copies in, kernels, copies out
  hipStream_t side = nullptr;          // the (usually empty) staged work list runs beside the fused kernel
  hipStream_t pre = nullptr;           // layout + floor unwrap of submit i+1 run beside the fused kernel of submit i
  hipEvent_t ev_join = nullptr, ev_self = nullptr;
  hipEvent_t ev_reset = nullptr;       // recorded behind the memset of vsyn_reset_streams
  bool reset_pending = false;          // the next preparation waits for ev_reset
  // Workspace ring: submit i uses slot i % WS_RING. When its preparation kernels run on the internal stream `pre` (beside the previous
  // submit's synthesis kernel) the slot's previous user, submit i - WS_RING, must be done: known from an event recorded on the caller's
  // stream behind every submit whose preparation ran there. WS_RING = 2 on purpose: a deeper ring lets the preparation run further
  // ahead, but then its workgroups land in the MIDDLE of an exact-fit synthesis grid instead of at its start (measured with a ring of 8
  // and an event behind every 4th submit: config 3's synthesis kernel 0.258 instead of 0.242 ms).
  static constexpr uint32_t WS_RING = 2, EV_RING = 2, CNT_RING = 4;
  hipEvent_t ev_pre_done[WS_RING] = {}, ev_ring[EV_RING] = {};
  uint64_t ev_ring_submit[EV_RING] = {~0ull, ~0ull};  // submit index each ring event was recorded behind
  bool pre_done_valid[WS_RING] = {};
  hipStream_t last_pre_stream = nullptr;  // stream the previous submit's preparation ran on (valid iff pre_done_valid[its slot])
  bool last_prep_on_main = false;      // the previous submit's preparation ran on the caller's stream
  bool last_ran_layout = true;         // the previous submit ran vsyn_layout_kernel (it keeps the staged list counters one slot ahead)
  uint64_t long_modes = 0;             // bit m: mode m selects a long block
  uint64_t nsub = 0;                   // submits so far
  uint32_t prep_lds_bytes = 0;         // dynamic LDS of vsyn_prep_kernel: one 32-bit column of the longest floor's posts per thread
  uint32_t unwrap_lds_bytes = 0;       // the same for vsyn_floor_unwrap_kernel
  uint32_t submit_count = 0;
  // workspace
  // per-batch workspace, a ring indexed by the submit number so that the preparation of later submits can run ahead
  DevBuf<uint32_t> ws_list[WS_RING];  // staged work list
  DevBuf<uint32_t> ws_count;    // its counters: a ring of CNT_RING (the layout kernel of submit i clears the slot of submit i+1)
  DevBuf<PktInfo> ws_info[WS_RING];
  DevBuf<SegInfo> ws_seg[WS_RING];
  DevBuf<uint32_t> ws_segmap[WS_RING];
  DevBuf<uint16_t> ws_fy[WS_RING];
  DevBuf<uint8_t> ws_runcls[WS_RING];
  DevBuf<LayoutChunk> ws_chunks;   // look-back records of the chunked layout scan (segments beyond LAYOUT_CHUNK_PACKETS)
  DevBuf<float> ws_env, ws_blk;
  // host-submit staging
  DevBuf<vsyn_packet> st_pk;
  DevBuf<vsyn_segment> st_seg;
  DevBuf<uint16_t> st_ys, st_fy;
  DevBuf<float> st_res, st_pcm, st_env, st_blk;
  DevBuf<uint16_t> st_curve;
  DevBuf<uint32_t> st_emit;
  DevBuf<double> st_sum;               // vsyn_pcm_abs_sum_host
  DevBuf<uint8_t> st_conv;             // vsyn_pcm_fetch_host: interleaved output
  DevBuf<uint32_t> st_frames;
  uint64_t last_host_plane = 0;        // plane_stride of the most recent vsyn_submit_host* (0: none yet)
  // the stages behind synthesis: each owns its workspace, and its launch code sees nothing else of the handle
  FeatureWs ft;                        // vsyn_features.h
  SpectralWs sp;                       // vsyn_spectral.h
  TuningWs tu;                         // vsyn_tuning.h (beside sp: the table and the offsets are the spectral stage's)
  DevBuf<float> tu_rows;               // vsyn_pcm_tuning_host: rows of NB pitches and NB magnitudes
  PostWs pp;                           // vsyn_spectral_post.h
  PcenWs pc;                           // vsyn_pcen.h
  HpssWs hp;                           // vsyn_hpss.h
  IstftWs is;                          // vsyn_istft.h
  EffectWs ef;                         // vsyn_effects.h
  PvWs pv;                             // vsyn_pv.h
  StretchWs st;                        // vsyn_stretch.h
  RhythmWs rh;                         // vsyn_rhythm.h
  BeatWs bt;                           // vsyn_beat.h
  ResampleWs rs;                       // vsyn_resample.h
  CondWs cd;                           // vsyn_condition.h
  TrimWs tr;                           // vsyn_trim.h
  SplitWs sl;                          // vsyn_split.h
  PitchWs pt;                          // vsyn_pitch.h
  PyinWs py;                           // vsyn_pyin.h
  FdescWs fd;                          // vsyn_fdesc.h
  CqtWs cq;                            // vsyn_cqt.h
  LoudWs ld;                           // vsyn_loudness.h
  // profiling
  bool profile = false;
  int profile_which = 1;  // 1 / 2: the fused kernel (steady / mixed workloads: same kernel), 3: residue VQ kernel
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  size_t events_used = 0;
  const char* profile_kernel = "";
  std::mutex mu;
};

// ------------------------------------------------------------------------------------------------
// constant block
// ------------------------------------------------------------------------------------------------
static void host_window(uint32_t bs0, uint32_t bs1, int lng, int prev, int next, float* w) {
  // VorbisModeNumber::precalc, hpp:837-862 (same float/double mix: sinf of a double-computed argument)
  const uint32_t n = lng ? bs1 : bs0;
  if (!lng) prev = next = 0;
  const uint32_t left = (prev ? bs1 : bs0) / 2, right = (next ? bs1 : bs0) / 2;
  const uint32_t left_begin = n / 4 - left / 2, right_begin = n - n / 4 - right / 2;
  for (uint32_t i = 0; i < n; ++i) w[i] = 0.f;
  for (uint32_t i = 0; i < left; ++i) {
    float x = sinf((float)(M_PI_2 * (i + 0.5) / left));
    w[left_begin + i] = sinf((float)(M_PI_2 * x * x));
  }
  for (uint32_t i = left_begin + left; i < right_begin; ++i) w[i] = 1.f;
  for (uint32_t i = 0; i < right; ++i) {
    float x = sinf((float)(M_PI_2 * (right - i - .5) / right));
    w[right_begin + i] = sinf((float)(M_PI_2 * x * x));
  }
}

static int build_const(const vsyn_setup* su, uint32_t max_streams, vsyn_handle* h, const char** err) {
  if (!su) return fail(err, VSYN_ERR_INVALID, "setup is NULL");
  if (su->channels < 1 || su->channels > VSYN_MAX_CHANNELS) return fail(err, VSYN_ERR_INVALID, "channels %u not in 1..%d", su->channels, VSYN_MAX_CHANNELS);
  if (!is_pow2(su->blocksize0) || !is_pow2(su->blocksize1) || su->blocksize0 < VSYN_MIN_BLOCKSIZE ||
      su->blocksize1 > VSYN_MAX_BLOCKSIZE || su->blocksize0 > su->blocksize1)
    return fail(err, VSYN_ERR_INVALID, "blocksizes %u/%u invalid (hpp:1294-1298)", su->blocksize0, su->blocksize1);
  if (su->num_floors < 1 || su->num_floors > VSYN_MAX_TABLES || su->num_mappings < 1 || su->num_mappings > VSYN_MAX_TABLES ||
      su->num_modes < 1 || su->num_modes > VSYN_MAX_TABLES || !su->floors || !su->mappings || !su->modes)
    return fail(err, VSYN_ERR_INVALID, "floor/mapping/mode counts out of range");
  if (max_streams < 1) return fail(err, VSYN_ERR_INVALID, "max_streams must be >= 1");

  ConstHeader& H = h->H;
  memset(&H, 0, sizeof(H));
  H.channels = su->channels;
  H.bs[0] = su->blocksize0;
  H.bs[1] = su->blocksize1;
  H.lg[0] = ilog2(su->blocksize0);
  H.lg[1] = ilog2(su->blocksize1);
  H.num_floors = su->num_floors;
  H.num_mappings = su->num_mappings;
  H.num_modes = su->num_modes;
  H.max_streams = max_streams;

  std::vector<FloorConst> floors(su->num_floors);
  uint32_t maxp = 2;
  for (uint32_t f = 0; f < su->num_floors; ++f) {
    const vsyn_floor1& sf = su->floors[f];
    FloorConst& fc = floors[f];
    memset(&fc, 0, sizeof(fc));
    if (sf.multiplier < 1 || sf.multiplier > 4) return fail(err, VSYN_ERR_INVALID, "floor %u: multiplier %u (hpp:486-492)", f, sf.multiplier);
    if (sf.num_posts < 2 || sf.num_posts > VSYN_MAX_POSTS || !sf.xs) return fail(err, VSYN_ERR_INVALID, "floor %u: %u posts", f, sf.num_posts);
    static const uint32_t range_of[5] = {0, 256, 128, 86, 64};
    fc.mult = sf.multiplier;
    fc.posts = sf.num_posts;
    fc.range = range_of[sf.multiplier];
    maxp = std::max(maxp, sf.num_posts);
    for (uint32_t i = 0; i < sf.num_posts; ++i) {
      if (sf.xs[i] > 0xFFFFu) return fail(err, VSYN_ERR_INVALID, "floor %u: x[%u]=%u too large", f, i, sf.xs[i]);
      fc.xs[i] = (uint16_t)sf.xs[i];
    }
    if (sf.xs[0] != 0) return fail(err, VSYN_ERR_INVALID, "floor %u: xs[0] must be 0 (hpp:449)", f);
    std::vector<uint32_t> order(sf.num_posts);
    for (uint32_t i = 0; i < sf.num_posts; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return sf.xs[a] < sf.xs[b]; });
    for (uint32_t s = 0; s < sf.num_posts; ++s) {
      if (s && sf.xs[order[s]] == sf.xs[order[s - 1]]) return fail(err, VSYN_ERR_INVALID, "floor %u: duplicate x %u (render_line needs x0<x1, Utils.hpp:145)", f, sf.xs[order[s]]);
      fc.sorted_idx[s] = (uint8_t)order[s];
      fc.xs_sorted[s] = (uint16_t)sf.xs[order[s]];
    }
    for (uint32_t i = 2; i < sf.num_posts; ++i) {  // Utils.hpp:60-118
      int lo = -1, hi = -1;
      for (uint32_t j = 0; j < i; ++j) {
        if (sf.xs[j] < sf.xs[i] && (lo < 0 || sf.xs[j] > sf.xs[lo])) lo = (int)j;
        if (sf.xs[j] > sf.xs[i] && (hi < 0 || sf.xs[j] < sf.xs[hi])) hi = (int)j;
      }
      if (lo < 0 || hi < 0) return fail(err, VSYN_ERR_INVALID, "floor %u: post %u has no low/high neighbour (xs[1] must be the maximum)", f, i);
      fc.lo[i] = (uint8_t)lo;
      fc.hi[i] = (uint8_t)hi;
      fc.pk[i].lo = (uint16_t)lo;
      fc.pk[i].hi = (uint16_t)hi;
      fc.pk[i].dxi = (uint16_t)(sf.xs[i] - sf.xs[lo]);
      fc.pk[i].adx = (uint16_t)(sf.xs[hi] - sf.xs[lo]);
      fc.pk[i].inv_adx = 1.0f / (float)(sf.xs[hi] - sf.xs[lo]);
      fc.pk[i].idx = i;
    }
    {
      // posts by depth in the neighbour tree (posts 0 and 1 carry their coded values: depth 0), four of one depth to a group
      std::vector<uint32_t> depth(sf.num_posts, 0);
      uint32_t maxd = 0;
      for (uint32_t i = 2; i < sf.num_posts; ++i) {
        depth[i] = 1u + std::max(depth[fc.lo[i]], depth[fc.hi[i]]);
        maxd = std::max(maxd, depth[i]);
      }
      uint32_t ng = 0;
      for (uint32_t d = 1; d <= maxd; ++d) {
        std::vector<uint32_t> at;
        for (uint32_t i = 2; i < sf.num_posts; ++i)
          if (depth[i] == d) at.push_back(i);
        for (size_t k = 0; k < at.size(); k += 4, ++ng)
          for (uint32_t e = 0; e < 4; ++e) fc.sched[ng][e] = fc.pk[at[std::min(k + e, at.size() - 1)]];
      }
      fc.ngroups = ng;  // <= 63 (one group per post at worst)
    }
    // floors of <= 32 posts take the register chain of vsyn_prep.h, which reads the flag bits a coded post touches — itself and its two
    // neighbours — from the 4th dword of pk[] (sched[] above keeps the post's own index there)
    if (sf.num_posts <= 32)
      for (uint32_t i = 2; i < sf.num_posts; ++i) fc.pk[i].idx = (1u << fc.lo[i]) | (1u << fc.hi[i]) | (1u << i);
  }
  H.ys_stride = (maxp + 3u) & ~3u;
  h->prep_lds_bytes = maxp > 32 ? H.ys_stride * PREP_THREADS * (uint32_t)sizeof(uint32_t) : 16u;  // (floors of <= 32 posts stay in registers)
  h->unwrap_lds_bytes = maxp > 32 ? H.ys_stride * UNWRAP_THREADS * (uint32_t)sizeof(uint32_t) : 16u;

  std::vector<MapConst> maps(su->num_mappings);
  for (uint32_t m = 0; m < su->num_mappings; ++m) {
    const vsyn_mapping& sm = su->mappings[m];
    MapConst& mc = maps[m];
    memset(&mc, 0, sizeof(mc));
    if (sm.num_couplings > 256 || (sm.num_couplings && !sm.couplings) || !sm.channel_floor) return fail(err, VSYN_ERR_INVALID, "mapping %u invalid", m);
    mc.ncoup = sm.num_couplings;
    for (uint32_t k = 0; k < sm.num_couplings; ++k) {
      const vsyn_coupling& c = sm.couplings[k];
      if (c.magnitude == c.angle || c.magnitude >= su->channels || c.angle >= su->channels)
        return fail(err, VSYN_ERR_INVALID, "mapping %u coupling %u invalid (hpp:788-790)", m, k);
      mc.coup[2 * k] = c.magnitude;
      mc.coup[2 * k + 1] = c.angle;
    }
    for (uint32_t c = 0; c < su->channels; ++c) {
      if (sm.channel_floor[c] >= su->num_floors) return fail(err, VSYN_ERR_INVALID, "mapping %u: floor index out of range (hpp:807)", m);
      mc.chfloor[c] = sm.channel_floor[c];
    }
  }
  for (uint32_t k = 0; k < su->num_modes; ++k) {
    if (su->modes[k].mapping >= su->num_mappings) return fail(err, VSYN_ERR_INVALID, "mode %u: mapping out of range (hpp:832)", k);
    H.mode_blockflag[k] = su->modes[k].block_flag ? 1 : 0;
    H.mode_mapping[k] = su->modes[k].mapping;
  }

  // lay the block out
  size_t off = align_up(sizeof(ConstHeader), 256);
  H.off_floor = (uint32_t)off;
  off = align_up(off + sizeof(FloorConst) * floors.size(), 256);
  H.off_map = (uint32_t)off;
  off = align_up(off + sizeof(MapConst) * maps.size(), 256);
  H.off_invdb = (uint32_t)off;
  off = align_up(off + 256 * sizeof(float), 256);
  for (int b = 0; b < 2; ++b) {
    const uint32_t n = H.bs[b];
    H.off_pre[b] = (uint32_t)off;
    off = align_up(off + (n / 4) * sizeof(float2), 256);
    H.off_post[b] = (uint32_t)off;
    off = align_up(off + (n / 4) * sizeof(float2), 256);
    H.off_fft[b] = (uint32_t)off;
    off = align_up(off + (n / 4) * sizeof(float2), 256);
    H.off_win[b] = (uint32_t)off;
    off = align_up(off + 4 * (size_t)n * sizeof(float), 256);
  }
  H.total_bytes = (uint32_t)off;
  h->host_const.assign(off, 0);
  uint8_t* base = h->host_const.data();
  memcpy(base, &H, sizeof(H));
  memcpy(base + H.off_floor, floors.data(), sizeof(FloorConst) * floors.size());
  memcpy(base + H.off_map, maps.data(), sizeof(MapConst) * maps.size());
  memcpy(base + H.off_invdb, k_inverse_db_bits, sizeof(k_inverse_db_bits));
  for (int b = 0; b < 2; ++b) {
    const uint32_t n = H.bs[b], M = n / 2, N4 = n / 4;
    float2* pre = (float2*)(base + H.off_pre[b]);
    float2* post = (float2*)(base + H.off_post[b]);
    float2* tw = (float2*)(base + H.off_fft[b]);
    for (uint32_t k = 0; k < N4; ++k) {  // double precision, stored as f32 (as mdct_init does)
      const double a = -M_PI * (4.0 * k + 1.0) / (4.0 * M);
      pre[k] = make_float2((float)cos(a), (float)sin(a));
      const double p = -M_PI * (double)k / (double)M;
      post[k] = make_float2((float)cos(p), (float)sin(p));
      const double t = -2.0 * M_PI * (double)k / (double)N4;
      tw[k] = make_float2((float)cos(t), (float)sin(t));
    }
    float* win = (float*)(base + H.off_win[b]);
    for (int w = 0; w < 4; ++w) host_window(H.bs[0], H.bs[1], b, w & 1, (w >> 1) & 1, win + (size_t)w * n);
  }
  return VSYN_OK;
}

// ------------------------------------------------------------------------------------------------
// API
// ------------------------------------------------------------------------------------------------
extern "C" {

const char* vsyn_version(void) { return "parseoggvorbis_amd vsyn 0.1 (gfx950)"; }
int vsyn_abi_version(void) { return VSYN_ABI_VERSION; }

int vsyn_create(const vsyn_setup* setup, int device, uint32_t max_streams, vsyn_handle** out, const char** err) {
  if (!out) return fail(err, VSYN_ERR_INVALID, "out is NULL");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(err, VSYN_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU path)");
  if (device < 0 || device >= ndev) return fail(err, VSYN_ERR_NO_DEVICE, "device %d not in 0..%d", device, ndev - 1);
  vsyn_handle* h = new vsyn_handle();
  h->device = device;
  h->opt = options_from_env();
  int rc = build_const(setup, max_streams, h, err);
  if (rc) {
    delete h;
    return rc;
  }
  auto cleanup = [&](int code) {
    vsyn_destroy(h);
    return code;
  };
  hipError_t e;
#define HC(call)                                                                                                       \
  if ((e = (call)) != hipSuccess) {                                                                                    \
    fail(err, VSYN_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e));                                             \
    return cleanup(VSYN_ERR_HIP);                                                                                      \
  }
  HC(hipSetDevice(device));
  hipDeviceProp_t prop;
  HC(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    fail(err, VSYN_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    return cleanup(VSYN_ERR_NO_DEVICE);
  }
  const ConstHeader& H = h->H;
  HC(hipMalloc((void**)&h->d_const, h->host_const.size()));
  HC(hipMemcpy(h->d_const, h->host_const.data(), h->host_const.size(), hipMemcpyHostToDevice));
  HC(hipMalloc((void**)&h->d_state, sizeof(StreamState) * 2 * max_streams));  // two tagged records per slot (vsyn_device.h)
  HC(hipMemset(h->d_state, 0, sizeof(StreamState) * 2 * max_streams));
  const size_t carry_floats = 2ull * max_streams * H.channels * (H.bs[1] / 2);
  HC(hipMalloc((void**)&h->d_carry, carry_floats * sizeof(float)));
  HC(hipMemset(h->d_carry, 0, carry_floats * sizeof(float)));
  HC(hipMalloc((void**)&h->d_status, sizeof(DevStatus)));
  DevStatus init = {0u, 0xFFFFFFFFu};
  HC(hipMemcpy(h->d_status, &init, sizeof(init), hipMemcpyHostToDevice));
  h->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  HC(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
  HC(hipStreamCreateWithFlags(&h->pre, hipStreamNonBlocking));
  HC(hipStreamCreateWithFlags(&h->host_stream, hipStreamNonBlocking));
  // ordering events between this handle's own streams: device-scope release is enough (the one host read,
  // vsyn_sync_status, synchronises its stream); the system-scope fence of a default event costs ~3 us per submit
  const unsigned evf = hipEventDisableTiming | hipEventDisableSystemFence;
  HC(hipEventCreateWithFlags(&h->ev_join, evf));
  HC(hipEventCreateWithFlags(&h->ev_self, evf));
  HC(hipEventCreateWithFlags(&h->ev_reset, evf));
  for (uint32_t k = 0; k < H.num_modes && k < 64; ++k)
    if (H.mode_blockflag[k]) h->long_modes |= 1ull << k;
  for (uint32_t b = 0; b < vsyn_handle::WS_RING; ++b) HC(hipEventCreateWithFlags(&h->ev_pre_done[b], evf));
  for (uint32_t b = 0; b < vsyn_handle::EV_RING; ++b) HC(hipEventCreateWithFlags(&h->ev_ring[b], evf));
  // (the attribute is per kernel, not per handle: only ever raised, to the largest any setup can need — 68 posts x 256 threads x 4 B)
  HC(hipFuncSetAttribute((const void*)vsyn_prep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 68 * PREP_THREADS * 4));
  HC(h->ws_count.ensure(vsyn_handle::CNT_RING));
  HC(hipMemset(h->ws_count.p, 0, sizeof(uint32_t) * vsyn_handle::CNT_RING));
  // A floor whose posts lie outside the domain in which the fused kernels' float32 curve is proven exact (floor_closed_form_ok,
  // vsyn_fused.h: x[1] far beyond the half block) keeps the whole setup on the staged kernels, whose curve is integer.
  const bool curve_ok = floor_closed_form_ok(h->H, h->host_const.data());
  h->fused_mask = curve_ok ? fused_ok_mask(h->H, h->host_const.data()) : 0u;
  if ((e = fused_tables_create(h->H, h->host_const.data(), &h->fused, h->opt.debug)) != hipSuccess) {
    fail(err, VSYN_ERR_HIP, "fused table upload failed: %s", hipGetErrorString(e));
    return cleanup(VSYN_ERR_HIP);
  }
  // The size-generic kernel takes the mixed-block runs of every setup it covers where the 256/2048 kernel has no mixed path.
  if (curve_ok && !(h->fused_mask & 2u) && u_supported(h->H, h->host_const.data())) {
    e = u_tables_create(h->H, h->host_const.data(), &h->utab, h->opt.debug);
    if (e == hipSuccess) {
      h->u_mixed = true;
      h->fused_mask |= 2u;
    } else if (e == hipErrorInvalidValue) {
      // the setup does not fit (its channel waves plus the tables of an 8192-sample block exceed one CU's LDS): staged kernels
      u_tables_destroy(&h->utab);
      (void)hipGetLastError();
    } else {
      fail(err, VSYN_ERR_HIP, "generic fused table upload failed: %s", hipGetErrorString(e));
      return cleanup(VSYN_ERR_HIP);
    }
  }
#undef HC
  *out = h;
  return VSYN_OK;
}

void vsyn_destroy(vsyn_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  vq_stamps_dump();
  prep_stamps_dump();
  fused_stamps_dump();
  fused_tables_destroy(&h->fused);
  u_tables_destroy(&h->utab);
  if (h->side) (void)hipStreamDestroy(h->side);
  if (h->pre) (void)hipStreamDestroy(h->pre);
  if (h->host_stream) (void)hipStreamDestroy(h->host_stream);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->ev_self) (void)hipEventDestroy(h->ev_self);
  if (h->ev_reset) (void)hipEventDestroy(h->ev_reset);
  for (uint32_t b = 0; b < vsyn_handle::WS_RING; ++b)
    if (h->ev_pre_done[b]) (void)hipEventDestroy(h->ev_pre_done[b]);
  for (uint32_t b = 0; b < vsyn_handle::EV_RING; ++b)
    if (h->ev_ring[b]) (void)hipEventDestroy(h->ev_ring[b]);
  if (h->d_const) (void)hipFree(h->d_const);
  if (h->d_vq) (void)hipFree(h->d_vq);
  if (h->d_state) (void)hipFree(h->d_state);
  if (h->d_carry) (void)hipFree(h->d_carry);
  if (h->d_status) (void)hipFree(h->d_status);
  for (auto& ev : h->events) {
    (void)hipEventDestroy(ev.first);
    (void)hipEventDestroy(ev.second);
  }
  delete h;  // (frees every DevBuf: the device is selected and idle)
}

uint32_t vsyn_ys_stride(const vsyn_handle* h) { return h ? h->H.ys_stride : 0; }
uint32_t vsyn_channels(const vsyn_handle* h) { return h ? h->H.channels : 0; }
uint32_t vsyn_fused_paths(const vsyn_handle* h) { return h ? (h->fused_mask | (h->vq_tables_in_lds ? 0x100u : 0u)) : 0; }
size_t vsyn_const_block_bytes(const vsyn_handle* h) { return h ? h->host_const.size() : 0; }

int vsyn_profile_enable(vsyn_handle* h, int on) {
  if (!h) return VSYN_ERR_INVALID;
  h->profile = on != 0;
  if (on >= 1 && on <= 3) h->profile_which = on;
  return VSYN_OK;
}

int vsyn_profile_read(vsyn_handle* h, double* mean_ms, uint32_t* launches, const char** kernel_name) {
  if (!h) return VSYN_ERR_INVALID;
  std::lock_guard<std::mutex> lk(h->mu);
  (void)hipSetDevice(h->device);
  double total = 0;
  for (size_t i = 0; i < h->events_used; ++i) {
    (void)hipEventSynchronize(h->events[i].second);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, h->events[i].first, h->events[i].second);
    total += ms;
  }
  if (mean_ms) *mean_ms = h->events_used ? total / (double)h->events_used : 0.0;
  if (launches) *launches = (uint32_t)h->events_used;
  if (kernel_name) *kernel_name = h->profile_kernel;
  h->events_used = 0;
  return VSYN_OK;
}

static hipError_t profile_begin(vsyn_handle* h, hipStream_t s, const char* name) {
  if (!h->profile) return hipSuccess;
  if (h->events_used == h->events.size()) {
    hipEvent_t a, b;
    const unsigned pf = hipEventDisableSystemFence;  // timestamps only: no cache flush around the timed kernel
    hipError_t e = hipEventCreateWithFlags(&a, pf);
    if (e != hipSuccess) return e;
    e = hipEventCreateWithFlags(&b, pf);
    if (e != hipSuccess) return e;
    h->events.emplace_back(a, b);
  }
  h->profile_kernel = name;
  return hipEventRecord(h->events[h->events_used].first, s);
}
static hipError_t profile_end(vsyn_handle* h, hipStream_t s) {
  if (!h->profile) return hipSuccess;
  hipError_t e = hipEventRecord(h->events[h->events_used].second, s);
  ++h->events_used;
  return e;
}

int vsyn_reset_streams(vsyn_handle* h, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemsetAsync(h->d_state, 0, sizeof(StreamState) * 2 * h->H.max_streams, (hipStream_t)hip_stream));
  // the next preparation reads and writes these records on whichever stream it runs: it waits for the memset
  HIPCHK(hipEventRecord(h->ev_reset, (hipStream_t)hip_stream));
  h->reset_pending = true;
  return VSYN_OK;
}

int vsyn_sync_status(vsyn_handle* h, void* hip_stream, vsyn_status* status, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));
  DevStatus ds;
  HIPCHK(hipMemcpy(&ds, h->d_status, sizeof(ds), hipMemcpyDeviceToHost));
  if (ds.flags) {
    DevStatus init = {0u, 0xFFFFFFFFu};
    HIPCHK(hipMemcpy(h->d_status, &init, sizeof(init), hipMemcpyHostToDevice));
  }
  if (status) {
    status->flags = ds.flags;
    status->first_bad_packet = ds.first_bad_packet;
  }
  if (ds.flags) return fail(err, VSYN_ERR_STREAM, "device flagged the batch: flags=0x%x first_bad_packet=%u", ds.flags, ds.first_bad_packet);
  return VSYN_OK;
}

// d_vq == nullptr: d_residue is the input ("after_residue"). Otherwise d_residue is scratch that the residue VQ kernel
// fills from the entry numbers (after the layout kernel, which provides each packet's offset, beside the floor unwrap).
static int submit_device_impl(vsyn_handle* h, uint32_t P, const vsyn_packet* d_packets, uint32_t S, const vsyn_segment* d_segments,
                              uint32_t max_seg_packets, const uint16_t* d_ys, const vsyn_vq_batch* d_vq, float* d_residue, float* d_pcm,
                              uint64_t plane_stride, uint32_t* d_emit_len, const vsyn_taps* taps, uint32_t flags, void* hip_stream,
                              const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (P == 0 || S == 0) return VSYN_OK;
  if (!d_packets || !d_segments || !d_ys || !d_residue || !d_pcm) return fail(err, VSYN_ERR_INVALID, "NULL batch pointer");
  if (d_vq) {
    if (!h->d_vq) return fail(err, VSYN_ERR_INVALID, "vsyn_attach_vq has not been called on this handle");
    if (!d_vq->packets || (d_vq->num_cls && !d_vq->cls) || (d_vq->num_entries && !d_vq->entries)) return fail(err, VSYN_ERR_INVALID, "NULL vq batch pointer");
  }
  if (max_seg_packets == 0 || max_seg_packets > P) max_seg_packets = P;
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)hip_stream;
  const ConstHeader& H = h->H;
  const uint32_t C = H.channels;

  // ---- 1. plan -------------------------------------------------------------------------------------------------------------------
  // The intermediate-signal taps (after_envelope, pcm_after_mdct) exist only in the staged kernels. The feature taps — the rendered
  // floor curve and the unwrapped posts — do not force them: the posts come from the unwrap kernel either way and
  // the curve from the tap variant of the fused kernel.
  const bool want_taps = taps && (taps->after_envelope || taps->pcm_after_mdct);
  const bool use_u = h->u_mixed;  // (both fused kernels have a floor-curve tap variant)
  const uint32_t fmask = h->fused_mask;
  const bool force_staged = want_taps || (flags & VSYN_SUBMIT_STAGED) || !fmask;
  const uint32_t R = force_staged ? std::min<uint32_t>(max_seg_packets, 1024u)
                                  : fused_pick_run_len(h->opt.run_len, (fmask & 1u) || !use_u ? h->fused.waves_per_cu : (int)h->utab.waves_per_cu,
                                                       S, C, max_seg_packets, h->num_cus);
  const uint32_t runs_per_seg = (max_seg_packets + R - 1) / R;

  // Preparation of the batch (layout scan, floor-1 step 1). The preparation kernel vsyn_prep_kernel (vsyn_prep.h: layout and floor
  // workgroups side by side, no dependencies) runs on the caller's stream whenever it can: every run taken by a fused kernel, no residue
  // VQ stage (its kernel needs the packets' offsets first), no segment longer than PREP_MAX_SEG_PACKETS, no VSYN_SUBMIT_PRE_KERNELS.
  // Otherwise the chained layout and unwrap kernels (vsyn_staged.h) run. They go on the internal stream `pre`, beside the previous
  // submit's synthesis kernel, when VSYN_SUBMIT_INPUTS_READY is set and the batch is not forced staged.
  const bool prep_kernel = !force_staged && (fmask & 2u) && !d_vq && max_seg_packets <= PREP_MAX_SEG_PACKETS && !(flags & VSYN_SUBMIT_PRE_KERNELS);
  hipStream_t ps = !prep_kernel && (flags & VSYN_SUBMIT_INPUTS_READY) && !force_staged ? h->pre : s;
  // chained layout kernel: segments longer than LAYOUT_CHUNK_PACKETS are scanned in chunks (a multiple of R each) chained by a
  // look-back; the usual batch has one chunk per segment
  const uint32_t chunk_packets = max_seg_packets <= LAYOUT_CHUNK_PACKETS ? runs_per_seg * R : (LAYOUT_CHUNK_PACKETS + R - 1u) / R * R;
  const uint32_t chunks_per_seg = (max_seg_packets + chunk_packets - 1u) / chunk_packets;
  // preparation kernel: a workgroup takes whole runs, as many as give about one (packet, channel) row per thread; a batch of short
  // segments (thousands of streams with a few packets each) gets smaller workgroups — whole waves — instead of 256 threads with a
  // handful of rows. A layout workgroup and a floor workgroup per (segment, chunk), dealt in alternating groups of eight (vsyn_prep.h).
  const uint32_t prep_nt = std::min<uint32_t>(PREP_THREADS, std::max<uint32_t>(64u, ((max_seg_packets * C + 63u) / 64u) * 64u));
  const uint32_t prep_chunk_runs = std::max<uint32_t>(1u, std::max<uint32_t>(1u, prep_nt / C) / R);
  const uint32_t prep_chunks_per_seg = (runs_per_seg + prep_chunk_runs - 1u) / prep_chunk_runs;
  const uint64_t prep_wgs = (((uint64_t)S * prep_chunks_per_seg + 7u) / 8u) * 16u;
  // Staged kernels walk the work list the layout kernel built: everything when forced, otherwise only the runs the fused kernel
  // declines (short / mixed blocks, carry-in). In fused mode they run on a forked side stream beside the fused kernel (disjoint
  // outputs) and exit at once when the list is empty. With the mixed-block kernel available every run is taken by one of the two fused
  // kernels (run_class() never answers 0 then; packets with an invalid mode are skipped by both paths): the staged kernels are not
  // launched at all.
  const bool staged_may_work = force_staged || !(fmask & 2u);
  hipStream_t ss = force_staged ? s : h->side;
  // the fused kernels: one wave per (run, channel)
  const uint64_t fused_units = (uint64_t)S * runs_per_seg * C;

  // ---- 2. checks that can refuse the batch, then the allocations ----------------------------------------------------------------
  if (!prep_kernel && (uint64_t)S * chunks_per_seg > 0x7FFFFFFFull) return fail(err, VSYN_ERR_INVALID, "too many layout chunks");
  if (prep_kernel && prep_wgs > 0x7FFFFFF0ull) return fail(err, VSYN_ERR_INVALID, "too many runs");
  if (!force_staged && fused_units > (use_u ? U_MAX_UNITS : FUSED_MAX_UNITS)) return fail(err, VSYN_ERR_INVALID, "too many runs");
  // workspace of this submit: slot i % WS_RING of a ring, so that the preparation of later submits can run ahead of the synthesis
  // kernels (see vsyn_handle)
  const uint64_t isub = h->nsub;
  const uint32_t wb = (uint32_t)(isub % vsyn_handle::WS_RING), wb_prev = (uint32_t)((isub + vsyn_handle::WS_RING - 1u) % vsyn_handle::WS_RING);
  HIPCHK(h->ws_info[wb].ensure((size_t)P + 8));  // (slack: the generic kernel fetches descriptors eight at a time)
  HIPCHK(h->ws_seg[wb].ensure(S));
  HIPCHK(h->ws_segmap[wb].ensure(P));
  HIPCHK(h->ws_list[wb].ensure(2 * (size_t)P + 64));
  uint16_t* fy = taps && taps->floor_final ? taps->floor_final : nullptr;
  if (!fy) {
    HIPCHK(h->ws_fy[wb].ensure((size_t)P * C * H.ys_stride));
    fy = h->ws_fy[wb].p;
  }
  HIPCHK(h->ws_runcls[wb].ensure((size_t)S * runs_per_seg + 16));
  bool clear_chunks = false;  // the look-back records are epoch-tagged: cleared once, when the buffer grows
  if (!prep_kernel && chunks_per_seg > 1 && (size_t)S * chunks_per_seg > h->ws_chunks.cap) {
    HIPCHK(h->ws_chunks.ensure((size_t)S * chunks_per_seg));
    clear_chunks = true;
  }
  float* env = taps && taps->after_envelope ? taps->after_envelope : nullptr;
  float* blk = taps && taps->pcm_after_mdct ? taps->pcm_after_mdct : nullptr;
  if (staged_may_work) {
    // residue floats upper bound (the descriptors are device resident, so the exact sum is not known here)
    const size_t bound = (size_t)P * C * (H.bs[1] / 2);
    if (!env) {
      HIPCHK(h->ws_env.ensure(bound));
      env = h->ws_env.p;
    }
    if (!blk) {
      HIPCHK(h->ws_blk.ensure(2 * bound));
      blk = h->ws_blk.p;
    }
  }
  PktInfo* info = h->ws_info[wb].p;
  SegInfo* sinfo = h->ws_seg[wb].p;
  uint32_t* segmap = h->ws_segmap[wb].p;
  uint32_t* list = h->ws_list[wb].p;

  // ---- 3. take the submit number, order the streams -----------------------------------------------------------------------------
  ++h->nsub;
  uint32_t* cnt = h->ws_count.p + (isub % vsyn_handle::CNT_RING);
  uint32_t* cnt_next = h->ws_count.p + ((isub + 1u) % vsyn_handle::CNT_RING);
  ++h->submit_count;
  // the submit's number tags the stream-state records and the look-back records of the chunked scan; 0 means "never written"
  const uint32_t epoch = (h->submit_count & 0x3FFFFFFFu) ? h->submit_count : ++h->submit_count;
  if (ps != s) {
    // the slot's previous user, submit isub - WS_RING, has to be done: the ring event recorded behind it says so
    if (isub >= vsyn_handle::WS_RING) {
      const uint64_t need = isub - vsyn_handle::WS_RING;
      const uint32_t slot = (uint32_t)(need % vsyn_handle::EV_RING);
      if (h->ev_ring_submit[slot] == need) {
        HIPCHK(hipStreamWaitEvent(ps, h->ev_ring[slot], 0));
      } else {  // that submit's preparation ran on the caller's stream (no record): order behind everything queued there so far
        HIPCHK(hipEventRecord(h->ev_self, s));
        HIPCHK(hipStreamWaitEvent(ps, h->ev_self, 0));
      }
    }
    if (h->last_prep_on_main && isub > 0) {
      // the previous submit left the stream state from a kernel on the caller's stream
      HIPCHK(hipEventRecord(h->ev_self, s));
      HIPCHK(hipStreamWaitEvent(ps, h->ev_self, 0));
    }
  }
  // Consecutive preparations chain through the stream state (abs position, carry parity) and the list-counter ring: when this one
  // runs on another stream than the previous one did (flags differ between submits), that order has to be stated.
  if (h->pre_done_valid[wb_prev] && h->last_pre_stream != ps) HIPCHK(hipStreamWaitEvent(ps, h->ev_pre_done[wb_prev], 0));
  if (h->reset_pending) HIPCHK(hipStreamWaitEvent(ps, h->ev_reset, 0));

  // ---- 4. launch --------------------------------------------------------------------------------------------------------------
  if (!prep_kernel) {
    // the list-counter ring is cleared one submit ahead by the layout kernel; submits that ran none in between break that chain
    if (!h->last_ran_layout) HIPCHK(hipMemsetAsync(h->ws_count.p, 0, sizeof(uint32_t) * vsyn_handle::CNT_RING, ps));
    if (clear_chunks) HIPCHK(hipMemsetAsync(h->ws_chunks.p, 0, h->ws_chunks.cap * sizeof(LayoutChunk), ps));
    const uint32_t lt = std::min(chunk_packets, max_seg_packets) <= LAYOUT_SHORT_PACKETS ? LAYOUT_THREADS_SHORT : LAYOUT_THREADS;
    vsyn_layout_kernel<<<S * chunks_per_seg, lt, layout_lds_bytes(lt, chunk_packets), ps>>>(
        h->d_const, P, d_packets, S, d_segments, plane_stride, info, sinfo, h->d_state, d_emit_len, h->d_status, R, force_staged ? 0u : fmask, list, cnt,
        cnt_next, segmap, h->ws_runcls[wb].p, runs_per_seg, chunk_packets, chunks_per_seg, h->ws_chunks.p, epoch);
    const uint32_t rows = P * C;
    vsyn_floor_unwrap_kernel<<<(rows + UNWRAP_THREADS - 1) / UNWRAP_THREADS, UNWRAP_THREADS, h->unwrap_lds_bytes, ps>>>(h->d_const, P, info, d_ys, fy,
                                                                                                                          h->d_status);
    if (d_vq) {
      if (h->profile_which == 3) HIPCHK(profile_begin(h, ps, "vsyn_residue_vq_kernel"));
      if (h->vq_tables_in_lds)
        vsyn_residue_vq_kernel<true><<<std::min<uint32_t>((P + h->vq_waves - 1u) / h->vq_waves, h->vq_grid), VQ_THREADS * h->vq_waves, h->vq_lds_bytes, ps>>>(
            h->d_const, h->d_vq, P, info, d_vq->packets, d_vq->cls, d_vq->num_cls, d_vq->entries, d_vq->num_entries, d_residue, h->d_status);
      else
        vsyn_residue_vq_kernel<false><<<std::min<uint32_t>(P, h->vq_grid), VQ_THREADS, h->vq_lds_bytes, ps>>>(
            h->d_const, h->d_vq, P, info, d_vq->packets, d_vq->cls, d_vq->num_cls, d_vq->entries, d_vq->num_entries, d_residue, h->d_status);
      if (h->profile_which == 3) HIPCHK(profile_end(h, ps));
    }
  } else {
    PrepCtx pc;
    pc.cb = h->d_const;
    pc.packets = d_packets;
    pc.segs = d_segments;
    pc.ys = d_ys;
    pc.fy = fy;
    pc.info = info;
    pc.sinfo = sinfo;
    pc.state = h->d_state;
    pc.status = h->d_status;
    pc.emit_len = d_emit_len;
    pc.run_cls = h->ws_runcls[wb].p;
    pc.plane_stride = plane_stride;
    pc.long_modes = h->long_modes;
    pc.S = S;
    pc.R = R;
    pc.runs_per_seg = runs_per_seg;
    pc.fused_ok = fmask;
    pc.P = P;
    pc.epoch = epoch;
    pc.chunk_runs = prep_chunk_runs;
    pc.chunks_per_seg = prep_chunks_per_seg;
    vsyn_prep_kernel<<<(uint32_t)prep_wgs, prep_nt, h->prep_lds_bytes, ps>>>(pc);
  }
  if (ps != s) {
    HIPCHK(hipEventRecord(h->ev_pre_done[wb], ps));
    HIPCHK(hipStreamWaitEvent(s, h->ev_pre_done[wb], 0));
  }

  if (staged_may_work) {
    if (!force_staged) {  // the side stream starts behind the preparation
      if (ps != s) {
        HIPCHK(hipStreamWaitEvent(h->side, h->ev_pre_done[wb], 0));
      } else {
        HIPCHK(hipEventRecord(h->ev_self, s));
        HIPCHK(hipStreamWaitEvent(h->side, h->ev_self, 0));
      }
    }
    const uint32_t grid = force_staged ? std::min<uint32_t>(P * C, 256u * 32u) : 512u;
    vsyn_spectrum_kernel<<<std::min<uint32_t>(grid, P), 256, 0, ss>>>(h->d_const, list, cnt, info, d_residue, fy, env,
                                                                      taps ? taps->floor_curve : nullptr, h->d_status);
    if (force_staged) HIPCHK(profile_begin(h, s, "vsyn_imdct_staged_kernel"));
    vsyn_imdct_staged_kernel<<<grid, 256, (size_t)H.bs[1] * 4, ss>>>(h->d_const, list, cnt, info, env, blk);
    if (force_staged) HIPCHK(profile_end(h, s));
    vsyn_overlap_kernel<<<grid, 256, 0, ss>>>(h->d_const, list, cnt, info, d_segments, sinfo, segmap, blk, d_pcm, plane_stride, h->d_carry);
  }
  if (!force_staged) {
    FusedArgs a;
    a.cb = h->d_const;
    a.binseg = h->fused.d_binseg;
    a.lds_image = h->fused.d_lds;
    a.packets = d_packets;
    a.segs = d_segments;
    a.info = info;
    a.sinfo = sinfo;
    a.run_cls = h->ws_runcls[wb].p;
    a.runs_per_seg = runs_per_seg;
    a.residue = d_residue;
    a.curve = taps ? taps->floor_curve : nullptr;
    a.fy = fy;
    a.pcm = d_pcm;
    a.carry = h->d_carry;
    a.status = h->d_status;
    a.plane_stride = plane_stride;
    a.S = S;
    a.R = R;
    a.fused_ok = use_u ? (fmask & 1u) : fmask;
    a.coupling_mode = (uint32_t)h->fused.coupling_mode;
    if (staged_may_work) HIPCHK(hipEventRecord(h->ev_join, h->side));
    // one launch covers the long-run and the mixed-block runs of the 256/2048 kernel (each wave takes the path of its run's class);
    // with the size-generic kernel in charge of the class-2 runs that is a second launch behind it (disjoint outputs)
    const bool time_u = use_u && (h->profile_which == 2 || !(fmask & 1u));
    hipError_t e = hipSuccess;
    if (a.fused_ok) {
      if (!time_u && (h->profile_which == 1 || h->profile_which == 2)) HIPCHK(profile_begin(h, s, a.curve ? "vsyn_fused_tap_kernel" : fused_kernel_name(H)));
      e = fused_launch(H, h->fused, a, s);
      if (e != hipSuccess) return fail(err, VSYN_ERR_HIP, "fused launch failed: %s", hipGetErrorString(e));
      if (!time_u && (h->profile_which == 1 || h->profile_which == 2)) HIPCHK(profile_end(h, s));
    }
    if (use_u) {
      FusedArgs au = a;
      au.fused_ok = fmask;
      if (time_u && (h->profile_which == 1 || h->profile_which == 2)) HIPCHK(profile_begin(h, s, au.curve ? "vsyn_fused_u_tap_kernel" : "vsyn_fused_u_kernel"));
      e = u_launch(H, h->utab, au, s);
      if (e != hipSuccess) return fail(err, VSYN_ERR_HIP, "generic fused launch failed: %s", hipGetErrorString(e));
      if (time_u && (h->profile_which == 1 || h->profile_which == 2)) HIPCHK(profile_end(h, s));
    }
    if (staged_may_work) HIPCHK(hipStreamWaitEvent(s, h->ev_join, 0));
  }

  // ---- 5. record the ordering state for the next submit ------------------------------------------------------------------------
  h->last_ran_layout = !prep_kernel;
  h->last_prep_on_main = ps == s;
  h->pre_done_valid[wb] = ps != s;  // (a preparation on the caller's stream is ordered by that stream itself)
  h->last_pre_stream = ps;
  h->reset_pending = false;
  if (ps != s) {  // (a record costs ~4.6 us between two synthesis kernels)
    const uint32_t slot = (uint32_t)(isub % vsyn_handle::EV_RING);
    HIPCHK(hipEventRecord(h->ev_ring[slot], s));
    h->ev_ring_submit[slot] = isub;
  }
  h->last_S = S;
  h->last_wb = wb;
  HIPCHK(hipGetLastError());
  return VSYN_OK;
}

int vsyn_submit_device(vsyn_handle* h, uint32_t P, const vsyn_packet* d_packets, uint32_t S, const vsyn_segment* d_segments,
                       uint32_t max_seg_packets, const uint16_t* d_ys, const float* d_residue, float* d_pcm,
                       uint64_t plane_stride, uint32_t* d_emit_len, const vsyn_taps* taps, uint32_t flags, void* hip_stream,
                       const char** err) {
  return submit_device_impl(h, P, d_packets, S, d_segments, max_seg_packets, d_ys, nullptr, const_cast<float*>(d_residue), d_pcm, plane_stride,
                            d_emit_len, taps, flags, hip_stream, err);
}

int vsyn_submit_device_vq(vsyn_handle* h, uint32_t P, const vsyn_packet* d_packets, uint32_t S, const vsyn_segment* d_segments,
                          uint32_t max_seg_packets, const uint16_t* d_ys, const vsyn_vq_batch* d_vq, float* d_residue, float* d_pcm,
                          uint64_t plane_stride, uint32_t* d_emit_len, const vsyn_taps* taps, uint32_t flags, void* hip_stream,
                          const char** err) {
  if (!d_vq) return fail(err, VSYN_ERR_INVALID, "vq batch is NULL");
  return submit_device_impl(h, P, d_packets, S, d_segments, max_seg_packets, d_ys, d_vq, d_residue, d_pcm, plane_stride, d_emit_len, taps, flags,
                            hip_stream, err);
}

int vsyn_attach_vq(vsyn_handle* h, const vsyn_vq_setup* vq, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  std::vector<uint8_t> block;
  const std::string why = vq_build_block(vq, h->H, block);
  if (!why.empty()) return fail(err, VSYN_ERR_INVALID, "%s", why.c_str());
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHK(hipSetDevice(h->device));
  // LDS budget of the value-table kernel: one workgroup per CU may take this much. The attribute belongs to the kernel on the current
  // device, not to the handle: one fixed value for every handle, so that a later handle never lowers the limit under an earlier one
  const uint32_t lds_budget = 156u * 1024u;
  HIPCHK(hipFuncSetAttribute((const void*)vsyn_residue_vq_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_budget));
  HIPCHK(hipDeviceSynchronize());  // a previously attached block may still be in use
  if (h->d_vq) (void)hipFree(h->d_vq);
  h->d_vq = nullptr;
  HIPCHK(hipMalloc((void**)&h->d_vq, block.size()));
  HIPCHK(hipMemcpy(h->d_vq, block.data(), block.size(), hipMemcpyHostToDevice));
  const VqHeader* vh = (const VqHeader*)block.data();
  uint32_t lds_off[7];
  const uint32_t wave_bytes = vq_lds_layout(vh->max_slots, vh->max_classes, lds_off);
  h->vq_tables_in_lds = false;
  h->vq_waves = 1;
  if (vh->img_floats && !h->opt.vq_no_lds_tables) {
    // value tables in LDS, one copy per workgroup: k workgroups of w waves per CU, the pair that keeps most waves resident
    const uint32_t tab_bytes = vq_align16(vh->img_floats * 4u);
    hipFuncAttributes fa;
    HIPCHK(hipFuncGetAttributes(&fa, (const void*)vsyn_residue_vq_kernel<true>));
    const uint32_t regs = ((uint32_t)std::max(fa.numRegs, 1) + 7u) / 8u * 8u;  // allocation granule 8, 512 per SIMD lane
    const uint32_t cu_waves = 4u * std::min<uint32_t>(8u, 512u / regs);
    uint32_t best_k = 0, best_w = 0;
    for (uint32_t k = 1; k <= 4; ++k) {
      // (several workgroups per CU: measured co-resident up to 2 x 67 KB, not at 2 x 73 KB — plan those against 128 KB)
      const uint32_t budget = k == 1 ? lds_budget : 128u * 1024u;
      if (budget / k <= tab_bytes + wave_bytes) break;
      const uint32_t w = std::min<uint32_t>({16u, (budget / k - tab_bytes) / wave_bytes, cu_waves / k});
      if (w && k * w > best_k * best_w) best_k = k, best_w = w;
    }
    if (best_w) {
      const uint32_t lds = tab_bytes + best_w * wave_bytes;
      int per_cu = 0;
      HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, vsyn_residue_vq_kernel<true>, (int)(VQ_THREADS * best_w), lds));
      if (per_cu > 0) {
        h->vq_tables_in_lds = true;
        h->vq_waves = best_w;
        h->vq_lds_bytes = lds;
        h->vq_grid = (uint32_t)h->num_cus * (uint32_t)per_cu;
        if (h->opt.debug) fprintf(stderr, "[vsyn] vq: tables in LDS (%u B), %u waves per workgroup, %d workgroups per CU, %u B LDS\n", tab_bytes, best_w, per_cu, lds);
      }
    }
  }
  if (!h->vq_tables_in_lds) {
    h->vq_lds_bytes = wave_bytes;
    int per_cu = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, vsyn_residue_vq_kernel<false>, VQ_THREADS, h->vq_lds_bytes));
    h->vq_grid = (uint32_t)h->num_cus * (uint32_t)std::max(per_cu, 1);
  }
  if (h->opt.vq_grid) h->vq_grid = std::min(h->vq_grid, h->opt.vq_grid);
  // the launch shape of either variant, in one form (tests read it)
  if (h->opt.debug)
    fprintf(stderr, "[vsyn] vq launch: %u workgroups, %u waves per workgroup, %u B LDS, tables in %s\n", h->vq_grid, h->vq_waves, h->vq_lds_bytes,
            h->vq_tables_in_lds ? "LDS" : "global memory");
  return VSYN_OK;
}

// residue != nullptr: floats in. Otherwise vq != nullptr: entry numbers in, floats rebuilt on the device and optionally
// copied back to residue_out.
static int submit_host_impl(vsyn_handle* h, uint32_t P, const vsyn_packet* packets, uint32_t S, const vsyn_segment* segments,
                            const uint16_t* ys, const float* residue, const vsyn_vq_batch* vq, float* residue_out, size_t residue_floats,
                            float* pcm, uint64_t plane_stride, uint32_t* emit_len, const vsyn_taps* taps, uint32_t flags, vsyn_status* status,
                            const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (status) {
    status->flags = 0;
    status->first_bad_packet = 0xFFFFFFFFu;
  }
  if (P == 0 || S == 0) return VSYN_OK;
  const bool keep_pcm = (flags & VSYN_SUBMIT_KEEP_PCM) != 0;
  if (!packets || !segments || !ys || (!residue && !vq) || (!pcm && !keep_pcm)) return fail(err, VSYN_ERR_INVALID, "NULL batch pointer");
  if (vq) {
    if (!h->d_vq) return fail(err, VSYN_ERR_INVALID, "vsyn_attach_vq has not been called on this handle");
    if (!vq->packets || (vq->num_cls && !vq->cls) || (vq->num_entries && !vq->entries)) return fail(err, VSYN_ERR_INVALID, "NULL vq batch pointer");
    for (uint32_t p = 0; p < P; ++p)
      if (vq->packets[p].entry_off + vq->packets[p].num_entries > vq->num_entries || vq->packets[p].cls_off > vq->num_cls)
        return fail(err, VSYN_ERR_INVALID, "vq packet %u points outside the entry / classification arrays", p);
  }
  const ConstHeader& H = h->H;
  const uint32_t C = H.channels;
  // host-visible validation (the device re-checks everything it dereferences)
  uint32_t max_seg = 1;
  for (uint32_t g = 0; g < S; ++g) {
    const vsyn_segment& sg = segments[g];
    if (sg.stream >= H.max_streams || (uint64_t)sg.first_packet + sg.num_packets > P || (sg.residue_off & 3))
      return fail(err, VSYN_ERR_INVALID, "segment %u invalid", g);
    uint64_t need = sg.residue_off;
    for (uint32_t q = 0; q < sg.num_packets; ++q) {
      const uint8_t m = packets[sg.first_packet + q].mode;
      need += (uint64_t)C * ((m < H.num_modes && H.mode_blockflag[m]) ? H.bs[1] : H.bs[0]) / 2;
    }
    if (need > residue_floats) return fail(err, VSYN_ERR_INVALID, "segment %u reads past the residue buffer", g);
    max_seg = std::max(max_seg, sg.num_packets);
  }
  HIPCHK(hipSetDevice(h->device));
  const size_t ys_n = (size_t)P * C * H.ys_stride, pcm_n = (size_t)S * C * plane_stride;
  HIPCHK(h->st_pk.ensure(P));
  HIPCHK(h->st_seg.ensure(S));
  HIPCHK(h->st_ys.ensure(ys_n));
  HIPCHK(h->st_res.ensure(residue_floats + 4));
  HIPCHK(h->st_pcm.ensure(pcm_n));
  HIPCHK(h->st_emit.ensure(P));
  vsyn_taps dt = {nullptr, nullptr, nullptr, nullptr};
  if (taps && taps->after_envelope) {
    HIPCHK(h->st_env.ensure(residue_floats + 4));
    dt.after_envelope = h->st_env.p;
  }
  if (taps && taps->pcm_after_mdct) {
    HIPCHK(h->st_blk.ensure(2 * residue_floats + 8));
    dt.pcm_after_mdct = h->st_blk.p;
  }
  if (taps && taps->floor_final) {
    HIPCHK(h->st_fy.ensure(ys_n));
    dt.floor_final = h->st_fy.p;
  }
  if (taps && taps->floor_curve) {
    HIPCHK(h->st_curve.ensure(residue_floats + 4));
    dt.floor_curve = h->st_curve.p;
  }
  // Everything runs on the handle's own stream, so that several handles driven from several host threads overlap their
  // copies and kernels (the NULL stream would serialise them). With pinned host buffers (vsyn_host_alloc) the copies are
  // direct DMA; pageable buffers work too, staged by the runtime.
  hipStream_t hs = h->host_stream;
  HIPCHK(hipMemcpyAsync(h->st_pk.p, packets, sizeof(vsyn_packet) * P, hipMemcpyHostToDevice, hs));
  HIPCHK(hipMemcpyAsync(h->st_seg.p, segments, sizeof(vsyn_segment) * S, hipMemcpyHostToDevice, hs));
  HIPCHK(hipMemcpyAsync(h->st_ys.p, ys, sizeof(uint16_t) * ys_n, hipMemcpyHostToDevice, hs));
  vsyn_vq_batch dvq;
  if (vq) {
    HIPCHK(h->st_vqpk.ensure(P));
    HIPCHK(h->st_cls.ensure((size_t)vq->num_cls + 16));
    HIPCHK(h->st_ent.ensure((size_t)vq->num_entries + 16));
    HIPCHK(hipMemcpyAsync(h->st_vqpk.p, vq->packets, sizeof(vsyn_vq_packet) * P, hipMemcpyHostToDevice, hs));
    if (vq->num_cls) HIPCHK(hipMemcpyAsync(h->st_cls.p, vq->cls, (size_t)vq->num_cls, hipMemcpyHostToDevice, hs));
    if (vq->num_entries) HIPCHK(hipMemcpyAsync(h->st_ent.p, vq->entries, sizeof(uint16_t) * (size_t)vq->num_entries, hipMemcpyHostToDevice, hs));
    dvq.packets = h->st_vqpk.p;
    dvq.cls = h->st_cls.p;
    dvq.entries = h->st_ent.p;
    dvq.num_cls = vq->num_cls;
    dvq.num_entries = vq->num_entries;
  } else {
    HIPCHK(hipMemcpyAsync(h->st_res.p, residue, sizeof(float) * residue_floats, hipMemcpyHostToDevice, hs));
  }
  HIPCHK(hipMemsetAsync(h->st_pcm.p, 0, sizeof(float) * pcm_n, hs));
  if (dt.floor_final) HIPCHK(hipMemsetAsync(h->st_fy.p, 0, ys_n * sizeof(uint16_t), hs));
  if (dt.floor_curve) HIPCHK(hipMemsetAsync(dt.floor_curve, 0, sizeof(uint16_t) * residue_floats, hs));
  if (dt.after_envelope) HIPCHK(hipMemsetAsync(dt.after_envelope, 0, sizeof(float) * residue_floats, hs));
  if (dt.pcm_after_mdct) HIPCHK(hipMemsetAsync(dt.pcm_after_mdct, 0, sizeof(float) * 2 * residue_floats, hs));
  const bool any_tap = dt.after_envelope || dt.pcm_after_mdct || dt.floor_final || dt.floor_curve;
  int rc = submit_device_impl(h, P, h->st_pk.p, S, h->st_seg.p, max_seg, h->st_ys.p, vq ? &dvq : nullptr, h->st_res.p, h->st_pcm.p, plane_stride,
                              h->st_emit.p, any_tap ? &dt : nullptr, flags & ~(VSYN_SUBMIT_INPUTS_READY | VSYN_SUBMIT_KEEP_PCM), hs, err);
  if (rc) return rc;
  h->last_host_plane = plane_stride;
  if (vq && residue_out) HIPCHK(hipMemcpyAsync(residue_out, h->st_res.p, sizeof(float) * residue_floats, hipMemcpyDeviceToHost, hs));
  // results are queued behind the kernels before the one host wait
  if (!keep_pcm) HIPCHK(hipMemcpyAsync(pcm, h->st_pcm.p, sizeof(float) * pcm_n, hipMemcpyDeviceToHost, hs));
  if (emit_len) HIPCHK(hipMemcpyAsync(emit_len, h->st_emit.p, sizeof(uint32_t) * P, hipMemcpyDeviceToHost, hs));
  if (dt.after_envelope) HIPCHK(hipMemcpyAsync(taps->after_envelope, dt.after_envelope, sizeof(float) * residue_floats, hipMemcpyDeviceToHost, hs));
  if (dt.pcm_after_mdct) HIPCHK(hipMemcpyAsync(taps->pcm_after_mdct, dt.pcm_after_mdct, sizeof(float) * 2 * residue_floats, hipMemcpyDeviceToHost, hs));
  if (dt.floor_final) HIPCHK(hipMemcpyAsync(taps->floor_final, dt.floor_final, sizeof(uint16_t) * ys_n, hipMemcpyDeviceToHost, hs));
  if (dt.floor_curve) HIPCHK(hipMemcpyAsync(taps->floor_curve, dt.floor_curve, sizeof(uint16_t) * residue_floats, hipMemcpyDeviceToHost, hs));
  vsyn_status st;
  rc = vsyn_sync_status(h, hs, &st, err);
  if (status) *status = st;
  return rc;
}

int vsyn_submit_host(vsyn_handle* h, uint32_t P, const vsyn_packet* packets, uint32_t S, const vsyn_segment* segments,
                     const uint16_t* ys, const float* residue, size_t residue_floats, float* pcm, uint64_t plane_stride,
                     uint32_t* emit_len, const vsyn_taps* taps, uint32_t flags, vsyn_status* status, const char** err) {
  if (!residue && P && S) return fail(err, VSYN_ERR_INVALID, "NULL batch pointer");
  return submit_host_impl(h, P, packets, S, segments, ys, residue, nullptr, nullptr, residue_floats, pcm, plane_stride, emit_len, taps, flags, status,
                          err);
}

int vsyn_submit_host_vq(vsyn_handle* h, uint32_t P, const vsyn_packet* packets, uint32_t S, const vsyn_segment* segments,
                        const uint16_t* ys, const vsyn_vq_batch* vq, float* residue_out, size_t residue_floats, float* pcm,
                        uint64_t plane_stride, uint32_t* emit_len, const vsyn_taps* taps, uint32_t flags, vsyn_status* status,
                        const char** err) {
  if (!vq && P && S) return fail(err, VSYN_ERR_INVALID, "vq batch is NULL");
  return submit_host_impl(h, P, packets, S, segments, ys, nullptr, vq, residue_out, residue_floats, pcm, plane_stride, emit_len, taps, flags, status,
                          err);
}

int vsyn_pcm_interleave_device(vsyn_handle* h, int format, const float* d_pcm, uint64_t plane_stride, void* d_out, uint64_t out_stride_frames,
                               uint32_t* d_frames, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (format != VSYN_PCM_S16 && format != VSYN_PCM_F32) return fail(err, VSYN_ERR_INVALID, "unknown PCM format %d", format);
  if (!d_pcm || !d_out || plane_stride == 0 || out_stride_frames == 0) return fail(err, VSYN_ERR_INVALID, "NULL pointer / zero stride");
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->last_S == 0) return fail(err, VSYN_ERR_INVALID, "no submit on this handle yet");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)hip_stream;
  const uint64_t cap = std::min<uint64_t>(std::min(plane_stride, out_stride_frames), 0xFFFFFFFFull);
  const dim3 grid((uint32_t)((cap + 1023) / 1024), h->last_S);
  const SegInfo* si = h->ws_seg[h->last_wb].p;
  if (format == VSYN_PCM_S16)
    VSYN_LAUNCH(vsyn_pcm_interleave_kernel<VSYN_PCM_S16>, grid, dim3(256), 0, s, h->d_const, si, h->last_S, d_pcm, plane_stride, d_out, out_stride_frames, d_frames);
  else
    VSYN_LAUNCH(vsyn_pcm_interleave_kernel<VSYN_PCM_F32>, grid, dim3(256), 0, s, h->d_const, si, h->last_S, d_pcm, plane_stride, d_out, out_stride_frames, d_frames);
  return VSYN_OK;
}

int vsyn_pcm_fetch_host(vsyn_handle* h, int format, void* out, uint64_t out_stride_frames, uint32_t* frames_out, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (format != VSYN_PCM_S16 && format != VSYN_PCM_F32) return fail(err, VSYN_ERR_INVALID, "unknown PCM format %d", format);
  if (!out || out_stride_frames == 0) return fail(err, VSYN_ERR_INVALID, "NULL pointer / zero stride");
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->last_S == 0 || h->last_host_plane == 0) return fail(err, VSYN_ERR_INVALID, "no vsyn_submit_host on this handle yet");
  HIPCHK(hipSetDevice(h->device));
  const size_t elem = format == VSYN_PCM_S16 ? 2 : 4;
  const size_t bytes = (size_t)h->last_S * out_stride_frames * h->H.channels * elem;
  HIPCHK(h->st_conv.ensure(bytes + 16));
  HIPCHK(h->st_frames.ensure(h->last_S));
  hipStream_t s = h->host_stream;
  HIPCHK(hipMemsetAsync(h->st_conv.p, 0, bytes, s));  // frames past a segment's end come back as silence, not as stale staging memory
  const uint64_t cap = std::min<uint64_t>(std::min<uint64_t>(h->last_host_plane, out_stride_frames), 0xFFFFFFFFull);
  const dim3 grid((uint32_t)((cap + 1023) / 1024), h->last_S);
  const SegInfo* si = h->ws_seg[h->last_wb].p;
  if (format == VSYN_PCM_S16)
    VSYN_LAUNCH(vsyn_pcm_interleave_kernel<VSYN_PCM_S16>, grid, dim3(256), 0, s, h->d_const, si, h->last_S, h->st_pcm.p, h->last_host_plane, h->st_conv.p,
                out_stride_frames, h->st_frames.p);
  else
    VSYN_LAUNCH(vsyn_pcm_interleave_kernel<VSYN_PCM_F32>, grid, dim3(256), 0, s, h->d_const, si, h->last_S, h->st_pcm.p, h->last_host_plane, h->st_conv.p,
                out_stride_frames, h->st_frames.p);
  HIPCHK(hipMemcpyAsync(out, h->st_conv.p, bytes, hipMemcpyDeviceToHost, s));
  if (frames_out) HIPCHK(hipMemcpyAsync(frames_out, h->st_frames.p, sizeof(uint32_t) * h->last_S, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return VSYN_OK;
}

int vsyn_pcm_abs_sum_host(vsyn_handle* h, double* out, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (!out) return fail(err, VSYN_ERR_INVALID, "out is NULL");
  std::lock_guard<std::mutex> lk(h->mu);
  if (h->last_S == 0 || h->last_host_plane == 0) return fail(err, VSYN_ERR_INVALID, "no vsyn_submit_host on this handle yet");
  HIPCHK(hipSetDevice(h->device));
  const uint32_t units = h->last_S * h->H.channels;
  HIPCHK(h->st_sum.ensure(units));
  VSYN_LAUNCH(vsyn_pcm_abs_sum_kernel, dim3(units), dim3(256), 0, h->host_stream, h->d_const, h->ws_seg[h->last_wb].p, h->last_S, h->st_pcm.p,
              h->last_host_plane, h->st_sum.p);
  HIPCHK(hipMemcpyAsync(out, h->st_sum.p, sizeof(double) * units, hipMemcpyDeviceToHost, h->host_stream));
  HIPCHK(hipStreamSynchronize(h->host_stream));
  return VSYN_OK;
}

int vsyn_host_alloc(size_t bytes, void** out, const char** err) {
  if (!out) return fail(err, VSYN_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (bytes == 0) return VSYN_OK;
  HIPCHK(hipHostMalloc(out, bytes, hipHostMallocDefault));
  return VSYN_OK;
}

void vsyn_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

int vsyn_imdct_device(vsyn_handle* h, uint32_t n, uint32_t count, const float* d_in, float* d_out, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (count == 0) return VSYN_OK;
  if (!d_in || !d_out) return fail(err, VSYN_ERR_INVALID, "NULL pointer");
  int b;
  if (n == h->H.bs[1]) b = 1;
  else if (n == h->H.bs[0]) b = 0;
  else return fail(err, VSYN_ERR_INVALID, "n=%u is neither blocksize of this handle (%u/%u)", n, h->H.bs[0], h->H.bs[1]);
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)hip_stream;
  hipError_t e = hipSuccess;
  bool done = false;
  HIPCHK(profile_begin(h, s, fused_imdct_kernel_name(n)));
  e = fused_imdct_launch(h->H, h->d_const, h->fused, b, n, count, d_in, d_out, s, &done);
  if (e != hipSuccess) return fail(err, VSYN_ERR_HIP, "imdct launch failed: %s", hipGetErrorString(e));
  if (!done) {
    h->profile_kernel = "vsyn_imdct_plain_kernel";
    const uint32_t grid = std::min<uint32_t>(count, 256u * 16u);
    vsyn_imdct_plain_kernel<<<grid, 256, (size_t)n * 4, s>>>(h->d_const, b, n, count, d_in, d_out);
  }
  HIPCHK(profile_end(h, s));
  HIPCHK(hipGetLastError());
  return VSYN_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// the front-ends after synthesis: the entry points. Each stage's checks, tables, workspace and launch are the host side of its header.
// ------------------------------------------------------------------------------------------------
// The end of a *_host call: vsyn_sync_status on the host stream (which waits for it), the batch's status into *status.
static int sync_status_into(vsyn_handle* h, vsyn_status* status, const char** err) {
  vsyn_status st;
  const int rc = vsyn_sync_status(h, h->host_stream, &st, err);
  if (status) *status = st;
  return rc;
}

extern "C" {

int vsyn_feature_rows_device(vsyn_handle* h, const vsyn_feature_spec* spec, uint32_t P, const vsyn_packet* d_packets, uint32_t S,
                             const vsyn_segment* d_segments, uint32_t max_seg_packets, uint64_t* d_seg_row_off, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (!d_seg_row_off) return fail(err, VSYN_ERR_INVALID, "d_seg_row_off is NULL");
  if (S == 0) return VSYN_OK;
  if ((P && !d_packets) || !d_segments) return fail(err, VSYN_ERR_INVALID, "NULL batch pointer");
  std::lock_guard<std::mutex> lk(h->mu);
  return feat_launch(h->ft, h->device, h->H, h->host_const.data(), h->d_const, h->d_status, h->unwrap_lds_bytes, spec, P, d_packets, S, d_segments,
                     max_seg_packets, nullptr, nullptr, nullptr, d_seg_row_off, (hipStream_t)hip_stream, err);
}

int vsyn_features_device(vsyn_handle* h, const vsyn_feature_spec* spec, uint32_t P, const vsyn_packet* d_packets, uint32_t S,
                         const vsyn_segment* d_segments, uint32_t max_seg_packets, const uint16_t* d_ys, const float* d_residue, float* d_rows,
                         uint64_t* d_seg_row_off, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (!spec) return fail(err, VSYN_ERR_INVALID, "feature spec is NULL");
  if (S == 0) return VSYN_OK;
  const bool res_kind = spec->kind == VSYN_FEAT_RESIDUE_YS || spec->kind == VSYN_FEAT_RESIDUE_YS_WITH_FLOOR;
  if (!d_segments || (P && (!d_packets || !d_ys || !d_rows || (res_kind && !d_residue)))) return fail(err, VSYN_ERR_INVALID, "NULL batch pointer");
  std::lock_guard<std::mutex> lk(h->mu);
  return feat_launch(h->ft, h->device, h->H, h->host_const.data(), h->d_const, h->d_status, h->unwrap_lds_bytes, spec, P, d_packets, S, d_segments,
                     max_seg_packets, d_ys, d_residue, d_rows, d_seg_row_off, (hipStream_t)hip_stream, err);
}

int vsyn_features_host(vsyn_handle* h, const vsyn_feature_spec* spec, uint32_t P, const vsyn_packet* packets, uint32_t S, const vsyn_segment* segments,
                       const uint16_t* ys, const float* residue, size_t residue_floats, float* rows, uint64_t rows_capacity, uint64_t* seg_rows,
                       vsyn_status* status, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  status_reset(status);
  if (!spec) return fail(err, VSYN_ERR_INVALID, "feature spec is NULL");
  if (S && !seg_rows) return fail(err, VSYN_ERR_INVALID, "seg_rows is NULL");
  for (uint32_t g = 0; g < S; ++g) seg_rows[g] = 0;
  if (P == 0 || S == 0) return VSYN_OK;
  const bool res_kind = spec->kind == VSYN_FEAT_RESIDUE_YS || spec->kind == VSYN_FEAT_RESIDUE_YS_WITH_FLOOR;
  if (!packets || !segments || !ys || (res_kind && !residue)) return fail(err, VSYN_ERR_INVALID, "NULL batch pointer");
  {  // the checks of the spec first: they need no device
    std::vector<uint8_t> tab;
    const int rc = feat_build_table(h->H, h->host_const.data(), spec, tab, err);
    if (rc) return rc;
  }
  const ConstHeader& H = h->H;
  const uint32_t C = H.channels;
  uint32_t max_seg = 1;
  for (uint32_t g = 0; g < S; ++g) {
    const vsyn_segment& sg = segments[g];
    if ((uint64_t)sg.first_packet + sg.num_packets > P || (sg.residue_off & 3)) return fail(err, VSYN_ERR_INVALID, "segment %u invalid", g);
    for (uint32_t g2 = 0; g2 < g; ++g2) {
      const vsyn_segment& o = segments[g2];
      if (sg.num_packets && o.num_packets && sg.first_packet < o.first_packet + o.num_packets && o.first_packet < sg.first_packet + sg.num_packets)
        return fail(err, VSYN_ERR_INVALID, "segments %u and %u overlap", g2, g);
    }
    if (res_kind) {
      uint64_t need = sg.residue_off;
      for (uint32_t q = 0; q < sg.num_packets; ++q) {
        const uint8_t m = packets[sg.first_packet + q].mode;
        need += (uint64_t)C * ((m < H.num_modes && H.mode_blockflag[m]) ? H.bs[1] : H.bs[0]) / 2;
      }
      if (need > residue_floats) return fail(err, VSYN_ERR_INVALID, "segment %u reads past the residue buffer", g);
    }
    max_seg = std::max(max_seg, sg.num_packets);
  }
  // the lock covers the whole call, copy-back included: the staging and row buffers are the handle's, and a second host thread on the
  // same handle must not overwrite them before this call has read its rows
  std::lock_guard<std::mutex> lk(h->mu);
  HIPCHK(hipSetDevice(h->device));
  hipStream_t hs = h->host_stream;
  const size_t ys_n = (size_t)P * C * H.ys_stride;
  HIPCHK(h->ft.st_pk.ensure(P));
  HIPCHK(h->ft.st_seg.ensure(S));
  HIPCHK(h->ft.st_ys.ensure(ys_n));
  HIPCHK(hipMemcpyAsync(h->ft.st_pk.p, packets, sizeof(vsyn_packet) * P, hipMemcpyHostToDevice, hs));
  HIPCHK(hipMemcpyAsync(h->ft.st_seg.p, segments, sizeof(vsyn_segment) * S, hipMemcpyHostToDevice, hs));
  HIPCHK(hipMemcpyAsync(h->ft.st_ys.p, ys, sizeof(uint16_t) * ys_n, hipMemcpyHostToDevice, hs));
  if (res_kind) {
    HIPCHK(h->ft.st_res.ensure(residue_floats + 4));
    HIPCHK(hipMemcpyAsync(h->ft.st_res.p, residue, sizeof(float) * residue_floats, hipMemcpyHostToDevice, hs));
  }
  // rows: every (packet, channel) at most once
  const uint64_t max_rows = (uint64_t)P * C, D = spec->output_dim;
  HIPCHK(h->ft.st_rows.ensure(max_rows * D + 1));
  int rc = feat_launch(h->ft, h->device, h->H, h->host_const.data(), h->d_const, h->d_status, h->unwrap_lds_bytes, spec, P, h->ft.st_pk.p, S, h->ft.st_seg.p,
                       max_seg, h->ft.st_ys.p, res_kind ? h->ft.st_res.p : nullptr, h->ft.st_rows.p, nullptr, hs, err);
  if (rc) return rc;
  std::vector<uint64_t> off((size_t)S + 1);
  HIPCHK(hipMemcpyAsync(off.data(), h->ft.segoff.p, sizeof(uint64_t) * (S + 1), hipMemcpyDeviceToHost, hs));
  HIPCHK(hipStreamSynchronize(hs));
  const uint64_t total = off[S];
  for (uint32_t g = 0; g < S; ++g) seg_rows[g] = off[g + 1] - off[g];
  rc = sync_status_into(h, status, err);
  if (rc) return rc;
  if (total > max_rows) return fail(err, VSYN_ERR_HIP, "row count %llu exceeds packets x channels", (unsigned long long)total);
  if (!rows) return VSYN_OK;
  if (total > rows_capacity) return fail(err, VSYN_ERR_INVALID, "rows buffer too small: %llu rows needed", (unsigned long long)total);
  if (total) {
    HIPCHK(hipMemcpyAsync(rows, h->ft.st_rows.p, sizeof(float) * total * D, hipMemcpyDeviceToHost, hs));
    HIPCHK(hipStreamSynchronize(hs));
  }
  return VSYN_OK;
}

uint64_t vsyn_spectral_num_frames(const vsyn_spectral_spec* spec, uint64_t frames) {
  if (spec_check(spec, 0, nullptr, nullptr) != VSYN_OK) return 0;
  return spec_num_frames(spec->n_fft, spec->hop_length, (spec->options & VSYN_SPEC_CENTER) != 0, frames);
}

uint32_t vsyn_spectral_dim(const vsyn_spectral_spec* spec) {
  // (the chroma kinds' width is a chroma parameter, which this function does not take: vsyn_spectral_chroma_dim answers for them)
  if (spec_check(spec, 0, nullptr, nullptr) != VSYN_OK || spec_is_chroma(spec)) return 0;
  return spec_dim(spec);
}

uint32_t vsyn_spectral_lin_tile(const vsyn_spectral_spec* spec) {
  if (spec_check(spec, 0, nullptr, nullptr) != VSYN_OK || !spec_is_lin(spec)) return 0;
  return spec_lin_tile(spec);
}

uint32_t vsyn_spectral_chroma_dim(const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma) {
  if (spec_check(spec, 0, nullptr, nullptr, chroma) != VSYN_OK) return 0;
  return spec_dim(spec, chroma);
}

uint32_t vsyn_spectral_chroma_tile(const vsyn_spectral_spec* spec) {
  if (spec_check(spec, 0, nullptr, nullptr) != VSYN_OK || !spec_is_chroma(spec)) return 0;
  return spec_chroma_tile(spec);
}

int vsyn_chroma_filterbank(uint32_t sample_rate, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma, float* out) {
  if (!out || !sample_rate || spec_check(spec, 0, nullptr, nullptr, chroma) != VSYN_OK || !spec_is_chroma(spec)) return VSYN_ERR_INVALID;
  chroma_filterbank(sample_rate, spec->n_fft, spec_chroma_or_defaults(chroma), out);
  return VSYN_OK;
}

int vsyn_spectral_device(vsyn_handle* h, const vsyn_spectral_spec* spec, uint32_t S, const uint32_t* sample_rates, const float* d_pcm,
                         uint64_t plane_stride, uint32_t channels, const uint32_t* d_frames, float* d_rows, uint64_t* d_seg_row_off,
                         void* hip_stream, const char** err) {
  return vsyn_spectral_chroma_device(h, spec, nullptr, S, sample_rates, d_pcm, plane_stride, channels, d_frames, d_rows, d_seg_row_off, hip_stream,
                                     err);
}

int vsyn_spectral_chroma_device(vsyn_handle* h, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma, uint32_t S,
                                const uint32_t* sample_rates, const float* d_pcm, uint64_t plane_stride, uint32_t channels,
                                const uint32_t* d_frames, float* d_rows, uint64_t* d_seg_row_off, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  int rc = spec_check(spec, S, sample_rates, err, chroma);
  if (rc) return rc;
  if (S == 0) return VSYN_OK;
  if (!d_pcm || !d_frames || !d_rows || plane_stride == 0 || channels == 0 || channels > 255)
    return fail(err, VSYN_ERR_INVALID, "NULL pointer, zero stride or channels outside [1, 255]");
  const uint64_t f_max = spec_num_frames(spec->n_fft, spec->hop_length, (spec->options & VSYN_SPEC_CENTER) != 0, plane_stride);
  std::lock_guard<std::mutex> lk(h->mu);
  return spec_launch(h->sp, h->device, spec, S, sample_rates, d_pcm, plane_stride, channels, d_frames, nullptr, f_max, (uint64_t)S * f_max, d_rows,
                     d_seg_row_off, (hipStream_t)hip_stream, err, chroma);
}


uint32_t vsyn_spectral_post_dim(const vsyn_spectral_spec* spec, const vsyn_spectral_post* post) {
  if (spec_check(spec, 0, nullptr, nullptr) != VSYN_OK || post_check(post, nullptr) != VSYN_OK) return 0;
  if (spec_is_lin(spec) && post_on(post)) return 0;  // refused: spec_post_check
  return spec_dim(spec) * (1u + post->order);
}

int vsyn_spectral_post_device(vsyn_handle* h, const vsyn_spectral_post* post, uint32_t dim, uint32_t S, const uint64_t* seg_rows,
                              const float* d_in, float* d_out, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (dim < 1 || dim > 256) return fail(err, VSYN_ERR_INVALID, "dim %u outside [1, 256]", dim);
  int rc = post_check(post, err, dim * (1u + (post && post->order <= 2 ? post->order : 0u)));
  if (rc) return rc;
  rc = post_check_rows(post, S, seg_rows, err);
  if (rc) return rc;
  const uint64_t total = seg_total(S, seg_rows);
  if (total == 0) return VSYN_OK;
  if (!d_in || !d_out) return fail(err, VSYN_ERR_INVALID, "NULL row pointer");
  if (d_in == d_out && post->order) return fail(err, VSYN_ERR_INVALID, "d_out may be d_in only when order = 0");
  std::lock_guard<std::mutex> lk(h->mu);
  if (!post_on(post)) {  // nothing to compute: the rows as they are
    HIPCHK(hipSetDevice(h->device));
    if (d_in != d_out) HIPCHK(hipMemcpyAsync(d_out, d_in, sizeof(float) * total * dim, hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
    return VSYN_OK;
  }
  return post_launch(h->pp, h->device, post, dim, S, seg_rows, d_in, d_out, (hipStream_t)hip_stream, err);
}

double vsyn_spectral_pcen_b(const vsyn_spectral_pcen* pcen, uint32_t sample_rate, uint32_t hop_length) {
  if (pcen_check(pcen, nullptr) != VSYN_OK) return 0.0;
  return pcen_b(pcen, sample_rate, hop_length);
}

int vsyn_spectral_pcen_device(vsyn_handle* h, const vsyn_spectral_pcen* pcen, uint32_t dim, uint32_t S, const uint64_t* seg_rows,
                              const uint32_t* sample_rates, uint32_t hop_length, const float* d_in, float* d_out, void* hip_stream,
                              const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (int rc = pcen_check_call(pcen, dim, S, seg_rows, sample_rates, hop_length, err)) return rc;
  const uint64_t total = seg_total(S, seg_rows);
  if (total == 0) return VSYN_OK;
  if (!d_in || !d_out) return fail(err, VSYN_ERR_INVALID, "NULL row pointer");
  std::lock_guard<std::mutex> lk(h->mu);
  return pcen_launch(h->pc, h->device, pcen, dim, S, seg_rows, sample_rates, hop_length, d_in, d_out, (hipStream_t)hip_stream, err);
}

int vsyn_spectral_hpss_device(vsyn_handle* h, const vsyn_spectral_hpss* hpss, uint32_t dim, uint32_t S, const uint64_t* seg_rows, const float* d_in,
                              float* d_out, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (int rc = hpss_check_call(hpss, dim, S, seg_rows, err)) return rc;
  const uint64_t total = seg_total(S, seg_rows);
  if (total == 0) return VSYN_OK;
  if (!d_in || !d_out) return fail(err, VSYN_ERR_INVALID, "NULL row pointer");
  std::lock_guard<std::mutex> lk(h->mu);
  return hpss_launch_any(h->hp, h->device, hpss, dim, S, seg_rows, d_in, d_out, (hipStream_t)hip_stream, err);
}

uint64_t vsyn_istft_num_samples(const vsyn_spectral_spec* spec, uint64_t rows) {
  if (istft_check(spec, nullptr) != VSYN_OK) return 0;
  return istft_num_samples(spec, rows);
}

int vsyn_istft_device(vsyn_handle* h, const vsyn_spectral_spec* spec, uint32_t S, const uint64_t* seg_rows, const float* d_rows, const float* d_mask,
                      const uint64_t* lengths, float* d_pcm_out, uint64_t out_plane_stride, uint32_t* d_out_frames, void* hip_stream,
                      const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  std::vector<uint64_t> len;
  uint64_t total, f_max, len_max;
  if (int rc = istft_check_call(spec, S, seg_rows, lengths, out_plane_stride, len, &total, &f_max, &len_max, err)) return rc;
  if (total && !d_rows) return fail(err, VSYN_ERR_INVALID, "NULL row pointer");
  if (len_max && !d_pcm_out) return fail(err, VSYN_ERR_INVALID, "NULL output pointer");
  std::lock_guard<std::mutex> lk(h->mu);
  return istft_launch(h->is, h->device, spec, S, seg_rows, len.data(), total, f_max, len_max, d_rows, d_mask, d_pcm_out, out_plane_stride,
                      d_out_frames, (hipStream_t)hip_stream, err);
}

int vsyn_pcm_hpss_device(vsyn_handle* h, const vsyn_pcm_effect* effect, uint32_t S, const uint64_t* frames, const float* d_pcm, uint64_t plane_stride,
                         uint32_t channels, float* d_pcm_out, uint64_t out_plane_stride, uint32_t* d_out_frames, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (int rc = effect_check(effect, err)) return rc;
  if (S == 0) return VSYN_OK;
  if (!frames || !d_pcm || !d_pcm_out || plane_stride == 0 || out_plane_stride == 0 || channels == 0 || channels > 255)
    return fail(err, VSYN_ERR_INVALID, "NULL pointer, zero stride or channels outside [1, 255]");
  std::lock_guard<std::mutex> lk(h->mu);
  return effect_launch(h->sp, h->hp, h->is, h->ef, h->device, effect, S, frames, nullptr, d_pcm, plane_stride, channels, d_pcm_out, out_plane_stride,
                       d_out_frames, (hipStream_t)hip_stream, err);
}

uint64_t vsyn_pv_num_rows(uint64_t rows, double rate) { return pv_num_rows(rows, rate); }

int vsyn_phase_vocoder_device(vsyn_handle* h, const vsyn_spectral_spec* spec, uint32_t S, const uint64_t* seg_rows, const double* rates,
                              const float* d_rows, float* d_rows_out, uint64_t* seg_rows_out, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  std::vector<uint64_t> f_out;
  uint64_t total, total_out;
  if (int rc = pv_check_call(spec, S, seg_rows, rates, f_out, &total, &total_out, err)) return rc;
  if (total && !d_rows) return fail(err, VSYN_ERR_INVALID, "NULL row pointer");
  if (total_out && !d_rows_out) return fail(err, VSYN_ERR_INVALID, "NULL output pointer");
  for (uint32_t g = 0; g < S && seg_rows_out; ++g) seg_rows_out[g] = f_out[g];
  std::lock_guard<std::mutex> lk(h->mu);
  return pv_launch(h->pv, h->device, spec, S, seg_rows, rates, f_out.data(), d_rows, d_rows_out, (hipStream_t)hip_stream, err);
}

uint64_t vsyn_stretch_num_samples(uint64_t frames, double rate) { return stretch_num_samples(frames, rate); }

int vsyn_pcm_stretch_device(vsyn_handle* h, const vsyn_pcm_stretch* stretch, uint32_t S, const uint64_t* frames, const double* rates,
                            const uint32_t* shift_from_hz, const float* d_pcm, uint64_t plane_stride, uint32_t channels, float* d_pcm_out,
                            uint64_t out_plane_stride, uint32_t* d_out_frames, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (int rc = stretch_check_call(stretch, S, rates, shift_from_hz, err)) return rc;
  if (S == 0) return VSYN_OK;
  if (!frames || !d_pcm || !d_pcm_out || plane_stride == 0 || out_plane_stride == 0 || channels == 0 || channels > 255)
    return fail(err, VSYN_ERR_INVALID, "NULL pointer, zero stride or channels outside [1, 255]");
  std::lock_guard<std::mutex> lk(h->mu);
  return stretch_launch(h->sp, h->pv, h->is, h->st, h->device, stretch, S, frames, rates, shift_from_hz, d_pcm, plane_stride, channels, d_pcm_out,
                        out_plane_stride, d_out_frames, (hipStream_t)hip_stream, err);
}

int vsyn_onset_peak_windows(const vsyn_onset_peaks* peaks, uint32_t sample_rate, uint32_t* out, const char** err) {
  if (int rc = peaks_check(peaks, err)) return rc;
  if (!out || !sample_rate) return fail(err, VSYN_ERR_INVALID, "peaks: out is NULL or the rate is 0");
  uint32_t w[5];
  if (int rc = peaks_windows(peaks, sample_rate, w, err)) return rc;
  memcpy(out, w, sizeof(w));
  return VSYN_OK;
}

uint32_t vsyn_tempogram_win_length(const vsyn_tempogram_spec* spec, uint32_t sample_rate) {
  if (tg_check(spec, nullptr) != VSYN_OK) return 0;
  return tg_win_length(spec, sample_rate);
}

uint32_t vsyn_tempogram_tile(uint32_t win_length) { return win_length < TG_MIN_W || win_length > TG_MAX_W ? 0u : tg_tile(win_length); }

int vsyn_tempo_from_mean(const vsyn_tempo_spec* tempo, const double* g, uint32_t win_length, uint32_t sample_rate, uint32_t hop_length,
                         double* bpm_out, uint32_t* lag_out, const char** err) {
  return tempo_from_mean(tempo, g, win_length, sample_rate, hop_length, bpm_out, lag_out, err);
}

int vsyn_onset_strength_device(vsyn_handle* h, const vsyn_onset_spec* onset, uint32_t dim, uint32_t S, const uint64_t* seg_rows,
                               const float* d_rows, float* d_env, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (int rc = onset_check_call(onset, dim, S, seg_rows, err)) return rc;
  const uint64_t total = seg_total(S, seg_rows);
  if (total == 0) return VSYN_OK;
  if (!d_rows || !d_env) return fail(err, VSYN_ERR_INVALID, "NULL row or envelope pointer");
  std::lock_guard<std::mutex> lk(h->mu);
  return onset_launch(h->rh, h->device, onset, dim, S, seg_rows, d_rows, d_env, (hipStream_t)hip_stream, err);
}

int vsyn_onset_peaks_device(vsyn_handle* h, const vsyn_onset_peaks* peaks, uint32_t S, const uint64_t* seg_rows, const uint32_t* sample_rates,
                            const float* d_env, uint32_t* d_onsets, uint32_t* d_counts, uint32_t* d_refused, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (int rc = peaks_check_call(peaks, S, seg_rows, sample_rates, err)) return rc;
  if (S == 0) return VSYN_OK;
  if (!d_counts) return fail(err, VSYN_ERR_INVALID, "d_counts is NULL");
  const uint64_t total = seg_total(S, seg_rows);
  if (total && (!d_env || !d_onsets)) return fail(err, VSYN_ERR_INVALID, "NULL envelope or onset pointer");
  std::lock_guard<std::mutex> lk(h->mu);
  return peaks_launch(h->rh, h->device, peaks, S, seg_rows, sample_rates, d_env, d_onsets, d_counts, d_refused, (hipStream_t)hip_stream, err);
}

int vsyn_tempogram_device(vsyn_handle* h, const vsyn_tempogram_spec* spec, uint32_t S, const uint64_t* seg_rows, const uint32_t* sample_rates,
                          const float* d_env, float* d_rows, double* d_mean, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (int rc = tg_check_call(spec, S, seg_rows, sample_rates, err)) return rc;
  if (S == 0) return VSYN_OK;
  if (!d_rows && !d_mean) return fail(err, VSYN_ERR_INVALID, "tempogram: neither rows nor mean asked for");
  const uint64_t total = seg_total(S, seg_rows);
  if (total && !d_env) return fail(err, VSYN_ERR_INVALID, "NULL envelope pointer");
  std::lock_guard<std::mutex> lk(h->mu);
  return tg_launch(h->rh, h->device, spec, S, seg_rows, sample_rates, d_env, d_rows, d_mean, (hipStream_t)hip_stream, err);
}

int vsyn_beat_period(const vsyn_beat_spec* beat, double bpm, uint32_t sample_rate, uint32_t* period_out, const char** err) {
  if (int rc = beat_check(beat, err)) return rc;
  if (!period_out || !sample_rate || !std::isfinite(bpm) || !(bpm > 0.0))
    return fail(err, VSYN_ERR_INVALID, "beat period: period_out is NULL, the rate is 0, or the bpm is not finite and > 0");
  *period_out = beat_period(beat, bpm, sample_rate);
  return VSYN_OK;
}

int vsyn_beat_track_device(vsyn_handle* h, const vsyn_beat_spec* beat, uint32_t S, const uint64_t* seg_rows, const uint32_t* periods,
                           const float* d_env, uint32_t* d_beats, uint32_t* d_counts, uint32_t* d_refused, double* d_localscore,
                           double* d_cumscore, int32_t* d_backlink, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (int rc = beat_check_call(beat, S, seg_rows, periods, err)) return rc;
  if (S == 0) return VSYN_OK;
  if (!d_counts) return fail(err, VSYN_ERR_INVALID, "d_counts is NULL");
  const uint64_t total = seg_total(S, seg_rows);
  if (total && (!d_env || !d_beats)) return fail(err, VSYN_ERR_INVALID, "NULL envelope or beat pointer");
  std::lock_guard<std::mutex> lk(h->mu);
  return beat_launch(h->bt, h->device, beat, S, seg_rows, periods, d_env, d_beats, d_counts, d_refused, d_localscore, d_cumscore, d_backlink,
                     (hipStream_t)hip_stream, err);
}

}  // extern "C"

// The stages chained behind the last host submit. The PCM the next stage reads: planar [S][C][plane]; each segment's frames from d_frames, else from si.
struct PcmView {
  const float* pcm;
  uint64_t plane;
  uint32_t C;
  const SegInfo* si;
  const uint32_t* d_frames;
};

// The last host submit's frames per segment into T[S], their maximum into *t_max: SegInfo::total_emit clamped to its plane; with
// out_rate != 0, what segment g has once resampled from rates[g] to out_rate (0 for rates[g] = 0; the caller has run rs_check).
// Caller holds h->mu.
static int last_submit_frames(vsyn_handle* h, uint32_t S, const uint32_t* rates, uint32_t out_rate, uint64_t* T, uint64_t* t_max, const char** err) {
  if (h->last_S == 0 || h->last_host_plane == 0) return fail(err, VSYN_ERR_INVALID, "no vsyn_submit_host on this handle yet");
  if (S != h->last_S) return fail(err, VSYN_ERR_INVALID, "num_segments %u differs from the last submit's %u", S, h->last_S);
  HIPCHK(hipSetDevice(h->device));
  std::vector<SegInfo> si(S);
  HIPCHK(hipMemcpyAsync(si.data(), h->ws_seg[h->last_wb].p, sizeof(SegInfo) * S, hipMemcpyDeviceToHost, h->host_stream));
  HIPCHK(hipStreamSynchronize(h->host_stream));
  *t_max = 0;
  for (uint32_t g = 0; g < S; ++g) {
    T[g] = std::min<uint64_t>(si[g].total_emit, h->last_host_plane);
    uint32_t up, down;
    if (out_rate) T[g] = rates[g] && rs_ratio(rates[g], out_rate, &up, &down) ? rs_num_frames(T[g], up, down) : 0;
    *t_max = std::max(*t_max, T[g]);
  }
  return VSYN_OK;
}

// The gate of a chain: the trim stage, or with split the split stage in its place, and where its read-backs go (host; NULL: not
// wanted). Trim fills bounds [S][2] and refs; split fills frames (the joined ones), counts, intervals [S][stride][2] and refs.
// gather = false (split): the intervals alone, no joined plane.
struct Gate {
  const vsyn_pcm_trim* spec;
  bool split, gather;
  uint32_t* frames;
  uint32_t* bounds;
  uint32_t* counts;
  uint32_t* intervals;
  uint64_t stride;
  double* refs;
};

// The gate as the exported entries name it: a trim with its bounds, or a split (joined) with its counts and intervals. gate = NULL:
// a chain without a gate.
static Gate make_gate(const vsyn_pcm_trim* gate, bool gate_is_split, uint32_t* bounds_out, uint32_t* counts_out, uint32_t* intervals_out,
                      uint64_t intervals_stride, double* refs_out) {
  return gate_is_split ? Gate{gate, true, true, nullptr, nullptr, counts_out, intervals_out, intervals_stride, refs_out}
                       : Gate{gate, false, false, nullptr, bounds_out, nullptr, nullptr, 0, refs_out};
}

// The specs of the stages a chain has (gate, cond: NULL, out_rate: 0 when it has none), in the order every entry checks them.
static int chain_check(const Gate* gate, const vsyn_pcm_cond* cond, uint32_t S, const uint32_t* rates, uint32_t out_rate, const char** err) {
  if (gate)
    if (int rc = trim_check(gate->spec, err)) return rc;
  if (cond)
    if (int rc = cond_check(cond, err)) return rc;
  return out_rate ? rs_check(S, rates, out_rate, err) : VSYN_OK;
}

// The rates the stage behind the chain sees: out_rate for every resampled segment, else the caller's; 0 skips a segment.
static std::vector<uint32_t> stage_rates(uint32_t S, const uint32_t* rates, uint32_t out_rate) {
  std::vector<uint32_t> r(S, 0u);
  for (uint32_t g = 0; g < S && rates; ++g) r[g] = out_rate && rates[g] ? out_rate : rates[g];
  return r;
}

// The rows of a framing (frame length n, hop, centred or not) over each segment's frames T[g], none where rates[g] = 0: into
// seg_rows, their sum and their maximum. A segment of fewer than min_rows rows gets none.
static void count_rows(uint32_t n, uint32_t hop, bool center, uint32_t S, const uint32_t* rates, const uint64_t* T, uint64_t min_rows,
                       uint64_t* seg_rows, uint64_t* total, uint64_t* f_max) {
  *total = *f_max = 0;
  for (uint32_t g = 0; g < S; ++g) {
    seg_rows[g] = rates[g] ? spec_num_frames(n, hop, center, T[g]) : 0;
    if (seg_rows[g] < min_rows) seg_rows[g] = 0;
    *total += seg_rows[g];
    *f_max = std::max(*f_max, seg_rows[g]);
  }
}

// intervals must hold what a segment of t_max frames can have
static int split_check_stride(const Gate& g, uint64_t t_max, const char** err) {
  const uint64_t need = split_max_intervals(t_max, g.spec->frame_length, g.spec->hop_length);
  if (g.intervals && g.stride < need)
    return fail(err, VSYN_ERR_INVALID, "intervals_stride %llu below %llu intervals", (unsigned long long)g.stride, (unsigned long long)need);
  return VSYN_OK;
}

// A chain starts at the last host submit's PCM and advances *v one step per stage, all on the host stream. Every step writes its
// workspace's plane of `plane` frames per segment and channel; clear zeroes that plane first (the step whose plane goes to the
// caller as float: zeros past each segment's frames). t_max bounds every segment's frames. Caller holds h->mu, has run chain_check
// and, between last_submit_frames and the first step, the checks of its own buffers.
static PcmView last_submit_view(vsyn_handle* h) { return PcmView{h->st_pcm.p, h->last_host_plane, h->H.channels, h->ws_seg[h->last_wb].p, nullptr}; }

// every segment from rates[g] to out_rate, into h->rs's planes
static int step_resample(vsyn_handle* h, uint32_t S, const uint32_t* rates, uint32_t out_rate, uint64_t plane, bool clear, PcmView* v, const char** err) {
  hipStream_t hs = h->host_stream;
  const size_t n = (size_t)S * v->C * plane;
  HIPCHK(h->rs.pcm.ensure(n + 1));
  if (clear) HIPCHK(hipMemsetAsync(h->rs.pcm.p, 0, sizeof(float) * n, hs));
  if (int rc = rs_launch(h->rs, h->device, S, rates, out_rate, v->pcm, v->plane, v->C, nullptr, v->si, h->rs.pcm.p, plane, nullptr, hs, err)) return rc;
  *v = PcmView{h->rs.pcm.p, plane, v->C, nullptr, h->rs.outF.p};
  return VSYN_OK;
}

// downmixed and trimmed into h->tr's mono plane, or split and joined into h->sl's; g's read-backs on their way to the host (the
// caller waits before it reads them). The next stage reads the mono plane as 1-channel PCM, with the frames the stage wrote.
static int step_gate(vsyn_handle* h, uint32_t S, const Gate& g, uint64_t plane, uint64_t t_max, bool clear, PcmView* v, const char** err) {
  hipStream_t hs = h->host_stream;
  const size_t n = (size_t)S * plane;
  if (!g.split) {
    HIPCHK(h->tr.pcm.ensure(n + 1));
    if (clear) HIPCHK(hipMemsetAsync(h->tr.pcm.p, 0, sizeof(float) * n, hs));
    if (int rc = trim_launch(h->tr, h->device, g.spec, S, v->pcm, v->plane, v->C, v->d_frames, v->si, t_max, h->tr.pcm.p, plane, nullptr, nullptr,
                             nullptr, nullptr, 0, hs, err))
      return rc;
    if (int rc = trim_fetch_bounds(h->tr, S, g.bounds, g.refs, hs, err)) return rc;
    *v = PcmView{h->tr.pcm.p, plane, 1u, nullptr, h->tr.frames.p};
    return VSYN_OK;
  }
  float* joined = nullptr;
  if (g.gather) {
    HIPCHK(h->sl.e.pcm.ensure(n + 1));
    if (clear) HIPCHK(hipMemsetAsync(h->sl.e.pcm.p, 0, sizeof(float) * n, hs));
    joined = h->sl.e.pcm.p;
  }
  uint64_t ws_stride = 0;
  if (int rc = split_launch(h->sl, h->device, g.spec, S, v->pcm, v->plane, v->C, v->d_frames, v->si, t_max, joined, plane, nullptr, nullptr, nullptr,
                            0, &ws_stride, nullptr, nullptr, 0, hs, err))
    return rc;
  if (int rc = split_fetch(h->sl, S, g.counts, g.intervals, g.stride, ws_stride, g.refs, hs, err)) return rc;
  if (g.frames) HIPCHK(hipMemcpyAsync(g.frames, h->sl.e.frames.p, sizeof(uint32_t) * S, hipMemcpyDeviceToHost, hs));
  *v = PcmView{joined, plane, 1u, nullptr, h->sl.e.frames.p};
  return VSYN_OK;
}

// conditioned into h->cd's mono plane, the peaks on their way to peaks_out; read on as the gate's plane is
static int step_condition(vsyn_handle* h, uint32_t S, const vsyn_pcm_cond* cond, uint64_t plane, uint64_t t_max, bool clear, float* peaks_out,
                          PcmView* v, const char** err) {
  hipStream_t hs = h->host_stream;
  const size_t n = (size_t)S * plane;
  HIPCHK(h->cd.pcm.ensure(n + 1));
  if (clear) HIPCHK(hipMemsetAsync(h->cd.pcm.p, 0, sizeof(float) * n, hs));
  if (int rc = cond_launch(h->cd, h->device, cond, S, v->pcm, v->plane, v->C, v->d_frames, v->si, t_max, h->cd.pcm.p, plane, nullptr, hs, err)) return rc;
  if (int rc = cond_fetch_peaks(h->cd, cond, S, peaks_out, hs, err)) return rc;
  *v = PcmView{h->cd.pcm.p, plane, 1u, nullptr, h->cd.frames.p};
  return VSYN_OK;
}

// the component of the view's mono downmix (T[g] frames, host; rates: 0 skips a segment, may be NULL) into h->ef's mono plane; read
// on as the gate's plane is, with the same frames
static int step_effects(vsyn_handle* h, uint32_t S, const vsyn_pcm_effect* effect, const uint32_t* rates, const uint64_t* T, uint64_t plane, bool clear,
                        PcmView* v, const char** err) {
  hipStream_t hs = h->host_stream;
  const size_t n = (size_t)S * plane;
  HIPCHK(h->ef.pcm.ensure(n + 1));
  HIPCHK(h->ef.frames.ensure(S));
  if (clear) HIPCHK(hipMemsetAsync(h->ef.pcm.p, 0, sizeof(float) * n, hs));
  if (int rc = effect_launch(h->sp, h->hp, h->is, h->ef, h->device, effect, S, T, rates, v->pcm, v->plane, v->C, h->ef.pcm.p, plane, h->ef.frames.p, hs,
                             err))
    return rc;
  *v = PcmView{h->ef.pcm.p, plane, 1u, nullptr, h->ef.frames.p};
  return VSYN_OK;
}

// The stretch stage in a chain.
struct Stretch {
  const vsyn_pcm_stretch* spec;
  const double* rates;       // [S]
  const uint32_t* from_hz;   // [S], NULL without a shift
};

// One chain behind the last host submit, as both chain bodies (pcm_out_host, spectral_host) take it. A stage whose spec is NULL is
// off, out_rate 0 is no resampling, and an output that is NULL is not wanted.
struct Chain {
  uint32_t S;             // the call: the last submit's segments, their rates, and the rate they are resampled to first
  const uint32_t* rates;
  uint32_t out_rate;
  Gate gate;              // the PCM stages, in the order they run
  const vsyn_pcm_effect* effect;
  Stretch stretch;
  const vsyn_loudness_spec* loud;
  const vsyn_pcm_cond* cond;
  const vsyn_spectral_spec* spec;  // the row stages of spectral_host, in the order they run (post and rhythm exclude each other)
  const vsyn_spectral_chroma* chroma;
  const vsyn_spectral_hpss* hpss;
  const vsyn_spectral_pcen* pcen;
  const vsyn_spectral_post* post;
  const vsyn_rhythm_spec* rhythm;
  const vsyn_onset_spec* beat_onset;  // the beat tracker behind the onset stage (vsyn_beat.h), in the rhythm stages' place
  const vsyn_beat_spec* beat;
  double* bpm_out;        // its tempo and the rows' rate per segment [S]
  uint32_t* rate_out;
  uint64_t* frames_out;   // the per-segment outputs [S]: the frames behind the gate (and the stretch), conditioning's peaks, the
  float* peaks_out;       // normaliser's records, the rhythm stages' refusal words
  vsyn_loudness_record* records_out;
  uint32_t* refused_out;
  const vsyn_tuning_spec* estimate;  // a chroma kind with each segment's tuning estimated first (vsyn_tuning.h): chroma->tuning is
  double* tuning_out;                // checked and not used; the estimates [S] go here
};

// the stretched (and shifted) mono downmix of the view (T[g] frames, host) into h->st's mono plane, T[g] replaced by what the stage
// delivers; read on as the gate's plane is, with those frames
static int step_stretch(vsyn_handle* h, uint32_t S, const Stretch& x, uint64_t* T, uint64_t plane, bool clear, PcmView* v, const char** err) {
  hipStream_t hs = h->host_stream;
  const size_t n = (size_t)S * plane;
  HIPCHK(h->st.pcm.ensure(n + 1));
  HIPCHK(h->st.frames.ensure(S));
  if (clear) HIPCHK(hipMemsetAsync(h->st.pcm.p, 0, sizeof(float) * n, hs));
  if (int rc = stretch_launch(h->sp, h->pv, h->is, h->st, h->device, x.spec, S, T, x.rates, x.from_hz, v->pcm, v->plane, v->C, h->st.pcm.p, plane,
                              h->st.frames.p, hs, err))
    return rc;
  for (uint32_t g = 0; g < S; ++g) {
    uint64_t len, res;
    T[g] = stretch_frames(x.spec, T[g], x.rates[g], x.from_hz ? x.from_hz[g] : 0u, &len, &res);
  }
  *v = PcmView{h->st.pcm.p, plane, 1u, nullptr, h->st.frames.p};
  return VSYN_OK;
}

// The normaliser of a chain (loud != NULL): what the chain forms ask of its spec beyond loud_check, before anything is written.
static int chain_loud_check(const vsyn_loudness_spec* loud, const vsyn_pcm_cond* cond, uint32_t S, const uint32_t* rates, const char** err) {
  if (int rc = loud_check(loud, err)) return rc;
  if (!(loud->options & VSYN_LOUD_NORMALIZE)) return fail(err, VSYN_ERR_INVALID, "the loudness step of a chain needs VSYN_LOUD_NORMALIZE and a target");
  if (loud->channel_mode != VSYN_LOUD_MONO) return fail(err, VSYN_ERR_INVALID, "the loudness step of a chain measures the mono downmix (VSYN_LOUD_MONO)");
  if (cond && (cond->options & VSYN_COND_PEAK)) return fail(err, VSYN_ERR_INVALID, "loudness normalisation and VSYN_COND_PEAK exclude each other");
  if (S && !rates) return fail(err, VSYN_ERR_INVALID, "the loudness step needs the segments' sample rates");
  return VSYN_OK;
}

// measured (the view's mono downmix, T[g] frames at rates[g]) and scaled to the target into h->ld's mono plane, the records on their
// way to records_out; read on as the gate's plane is, with the frames the view had
static int step_loudness(vsyn_handle* h, uint32_t S, const vsyn_loudness_spec* loud, const uint32_t* rates, const uint64_t* T, uint64_t plane,
                         bool clear, vsyn_loudness_record* records_out, PcmView* v, const char** err) {
  hipStream_t hs = h->host_stream;
  const size_t n = (size_t)S * plane;
  HIPCHK(h->ld.pcm.ensure(n + 1));
  HIPCHK(h->ld.rec.ensure(S));
  if (clear) HIPCHK(hipMemsetAsync(h->ld.pcm.p, 0, sizeof(float) * n, hs));
  if (int rc = loud_launch(h->ld, h->device, loud, S, rates, T, v->pcm, v->plane, v->C, h->ld.rec.p, nullptr, nullptr, 0, h->ld.pcm.p, plane, hs, err))
    return rc;
  if (records_out) HIPCHK(hipMemcpyAsync(records_out, h->ld.rec.p, sizeof(vsyn_loudness_record) * S, hipMemcpyDeviceToHost, hs));
  *v = PcmView{h->ld.pcm.p, plane, 1u, v->si, v->d_frames};
  return VSYN_OK;
}

// The end of a PCM host form: the view's planes to out as they are (VSYN_PCM_F32: the last step cleared them first), or interleaved
// and converted into s16 (vsyn_pcm_interleave_device's conversion, zeros past each segment's frames) and that; then the call's one wait.
static int pcm_copy_out(vsyn_handle* h, const PcmView& v, uint32_t S, int format, DevBuf<int16_t>& s16, void* out, const char** err) {
  hipStream_t hs = h->host_stream;
  const size_t n = (size_t)S * v.C * v.plane;
  if (format == VSYN_PCM_F32) {
    HIPCHK(hipMemcpyAsync(out, v.pcm, sizeof(float) * n, hipMemcpyDeviceToHost, hs));
  } else {
    HIPCHK(s16.ensure(n + 1));
    const dim3 grid((uint32_t)((v.plane + 255) / 256), S);
    VSYN_LAUNCH(vsyn_rs_s16_kernel, grid, dim3(256), 0, hs, v.pcm, v.plane, v.C, v.d_frames, s16.p, v.plane);
    HIPCHK(hipMemcpyAsync(out, s16.p, sizeof(int16_t) * n, hipMemcpyDeviceToHost, hs));
  }
  HIPCHK(hipStreamSynchronize(hs));
  return VSYN_OK;
}

// The PCM host forms: the steps of c that are present, in the one order they run in; the last of them into a plane of the caller's
// stride, the ones in front of it into planes as long as the longest segment; that plane to out, and the frames behind the gate
// (and the stretch) to c.frames_out.
static int pcm_out_host(vsyn_handle* h, const Chain& c, int format, void* out, uint64_t out_stride_frames, const char** err) {
  const uint32_t S = c.S;
  uint64_t* frames_out = c.frames_out;
  const Gate* gate = c.gate.spec ? &c.gate : nullptr;
  const Stretch* stretch = c.stretch.spec ? &c.stretch : nullptr;
  if (c.effect)
    if (int rc = effect_check(c.effect, err)) return rc;
  if (stretch) {
    if (c.effect) return fail(err, VSYN_ERR_INVALID, "a stretch and an hpss effect in one chain call: their composition is not built");
    if (int rc = stretch_check_call(stretch->spec, S, stretch->rates, stretch->from_hz, err)) return rc;
  }
  if (c.loud)
    if (int rc = chain_loud_check(c.loud, c.cond, S, c.rates, err)) return rc;
  if (int rc = chain_check(gate, c.cond, S, c.rates, c.out_rate, err)) return rc;
  if (format != VSYN_PCM_F32 && format != VSYN_PCM_S16) return fail(err, VSYN_ERR_INVALID, "unknown PCM format %d", format);
  if (S && !frames_out) return fail(err, VSYN_ERR_INVALID, "frames_out is NULL");
  if (c.peaks_out) memset(c.peaks_out, 0, sizeof(float) * S);
  if (c.records_out) memset(c.records_out, 0, sizeof(vsyn_loudness_record) * S);
  // the lock covers the whole call: the stages' workspaces are the handle's, and the PCM must stay that of the last submit
  std::lock_guard<std::mutex> lk(h->mu);
  uint64_t t_max;
  if (int rc = last_submit_frames(h, S, c.rates, c.out_rate, frames_out, &t_max, err)) return rc;
  const uint64_t t_in = t_max;  // the longest segment in front of the stretch; t_max: the longest anywhere in the chain
  std::vector<uint64_t> T_in(frames_out, frames_out + S);
  if (stretch) {  // every plane holds the largest of the input, the stretched, the resampled and the delivered lengths
    for (uint32_t g = 0; g < S; ++g) {
      frames_out[g] = stretch_span(stretch->spec, T_in[g], stretch->rates[g], stretch->from_hz ? stretch->from_hz[g] : 0u);
      t_max = std::max(t_max, frames_out[g]);
    }
  }
  if (!out || S == 0) return VSYN_OK;
  if (t_max > out_stride_frames) return fail(err, VSYN_ERR_INVALID, "out_stride_frames %llu below %llu frames",
                                             (unsigned long long)out_stride_frames, (unsigned long long)t_max);
  if (out_stride_frames > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "out_stride_frames must be below 2^32");
  std::vector<uint32_t> bounds(gate ? 2u * (size_t)S : 0), joined(gate ? S : 0);
  Gate g{};
  if (gate) {
    g = *gate;
    if (g.split)
      if (int rc = split_check_stride(g, t_in, err)) return rc;
    g.frames = joined.data();
    g.bounds = bounds.data();
  }
  // The steps in the order they run in. The last one present delivers: it alone writes a plane of the caller's stride, cleared
  // first when that plane goes out as float32, and its int16 scratch is the call's. A new stage is a name here, at its place.
  enum { RESAMPLE, GATE, EFFECT, STRETCH, LOUDNESS, CONDITION, STEPS };
  const bool present[STEPS] = {c.out_rate != 0, gate != nullptr, c.effect != nullptr, stretch != nullptr, c.loud != nullptr, c.cond != nullptr};
  int last = 0;
  for (int step = 0; step < STEPS; ++step)
    if (present[step]) last = step;
  const bool f32 = format == VSYN_PCM_F32;
  const uint64_t inner = std::max<uint64_t>(t_max, 1);
  const auto plane = [&](int step) { return step == last ? out_stride_frames : inner; };
  const auto clear = [&](int step) { return f32 && step == last; };
  PcmView v = last_submit_view(h);
  DevBuf<int16_t>* s16 = &h->rs.s16;
  if (c.out_rate)
    if (int rc = step_resample(h, S, c.rates, c.out_rate, plane(RESAMPLE), clear(RESAMPLE), &v, err)) return rc;
  if (gate) {
    if (int rc = step_gate(h, S, g, plane(GATE), t_in, clear(GATE), &v, err)) return rc;
    s16 = g.split ? &h->sl.e.s16 : &h->tr.s16;
  }
  // the effect's and the loudness stage's tables need each segment's frames: behind a gate the chain waits here for the gate's read-backs
  std::vector<uint64_t> T;
  if (c.effect || stretch || c.loud) {
    T = T_in;
    if (gate) {
      HIPCHK(hipStreamSynchronize(h->host_stream));
      for (uint32_t s = 0; s < S; ++s) T[s] = g.split ? joined[s] : bounds[2u * s + 1u] - bounds[2u * s];
    }
  }
  if (c.effect) {
    if (int rc = step_effects(h, S, c.effect, c.rates, T.data(), plane(EFFECT), clear(EFFECT), &v, err)) return rc;
    s16 = &h->ef.s16;
  }
  if (stretch) {  // T becomes the stage's frames: the steps behind it see those
    if (int rc = step_stretch(h, S, *stretch, T.data(), plane(STRETCH), clear(STRETCH), &v, err)) return rc;
    s16 = &h->st.s16;
  }
  if (c.loud) {
    const std::vector<uint32_t> ld_rates = stage_rates(S, c.rates, c.out_rate);
    if (int rc = step_loudness(h, S, c.loud, ld_rates.data(), T.data(), plane(LOUDNESS), clear(LOUDNESS), c.records_out, &v, err)) return rc;
    s16 = &h->ld.s16;
  }
  if (c.cond) {
    if (int rc = step_condition(h, S, c.cond, plane(CONDITION), t_max, clear(CONDITION), c.peaks_out, &v, err)) return rc;
    s16 = &h->cd.s16;
  }
  if (int rc = pcm_copy_out(h, v, S, format, *s16, out, err)) return rc;
  if (gate) {
    for (uint32_t s = 0; s < S; ++s) frames_out[s] = g.split ? joined[s] : bounds[2u * s + 1u] - bounds[2u * s];
    if (gate->bounds) memcpy(gate->bounds, bounds.data(), sizeof(uint32_t) * bounds.size());
  }
  for (uint32_t s = 0; s < S && stretch; ++s) frames_out[s] = T[s];
  return VSYN_OK;
}

// The end of a spectral host form: the rows of the view's PCM on the host stream, through the row stages of c (hpss: through the
// HPSS stage into its workspace, where the later stages find them; pcen: through the PCEN stage in place; rhythm: the rows stay on
// the device, and seg_rows becomes the selected output's; post, which the caller has set to NULL when it is off: on to the post
// stage in their place, and its wider rows come back), copied to rows, then the call's wait and status. spec_rates are the rates
// the rows are computed at (0 skips a segment); seg_rows, f_max and total are the host's row counts. Caller holds h->mu.
static int spectral_rows_out(vsyn_handle* h, const Chain& c, const uint32_t* spec_rates, const PcmView& v, uint64_t* seg_rows, uint64_t f_max,
                             uint64_t total, float* rows, uint64_t rows_capacity, vsyn_status* status, const char** err) {
  hipStream_t hs = h->host_stream;
  const uint32_t S = c.S;
  const uint64_t D = spec_dim(c.spec, c.chroma);
  if (c.hpss)
    if (int rc = hpss_check_call(c.hpss, (uint32_t)D, S, seg_rows, err)) return rc;
  HIPCHK(h->sp.rows.ensure(total * D + 1));
  int rc;
  if (c.estimate) {  // the estimate on the PCM the chroma kernel is about to see, at its framing and power; the one extra wait of the form
    vsyn_spectral_spec lin = *c.spec;
    lin.kind = VSYN_SPEC_LIN_POWER;
    HIPCHK(h->tu.tuning.ensure(S));
    HIPCHK(h->tu.counts.ensure(2ull * S));
    rc = pip_launch(h->sp, h->tu, h->device, &lin, c.estimate, S, spec_rates, v.pcm, v.plane, v.C, v.d_frames, v.si, f_max, nullptr, nullptr, 0, nullptr,
                    h->tu.tuning.p, h->tu.counts.p, hs, err);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c.tuning_out, h->tu.tuning.p, sizeof(double) * S, hipMemcpyDeviceToHost, hs));
    HIPCHK(hipStreamSynchronize(hs));
  }
  rc = spec_launch(h->sp, h->device, c.spec, S, spec_rates, v.pcm, v.plane, v.C, v.d_frames, v.si, f_max, total, h->sp.rows.p, nullptr, hs, err,
                   c.chroma, c.estimate ? c.tuning_out : nullptr);
  if (rc) return rc;
  float* cur = h->sp.rows.p;  // where the rows are
  if (c.hpss) {
    HIPCHK(h->hp.rows.ensure(total * D + 1));
    rc = hpss_launch(h->hp, h->device, c.hpss, (uint32_t)D, S, seg_rows, spec_rates, cur, h->hp.rows.p, hs, err);
    if (rc) return rc;
    cur = h->hp.rows.p;
  }
  if (c.pcen) {
    rc = pcen_launch(h->pc, h->device, c.pcen, (uint32_t)D, S, seg_rows, spec_rates, c.spec->hop_length, cur, cur, hs, err);
    if (rc) return rc;
  }
  if (c.rhythm) {  // the rows stay where they are: the selected rhythm output goes to the host in their place
    rc = rhythm_rows_out(h->rh, h->device, c.rhythm, (uint32_t)D, S, spec_rates, seg_rows, total, cur, rows, rows_capacity, c.refused_out, hs, err);
    if (rc) return rc;
    return sync_status_into(h, status, err);
  }
  if (c.beat) {  // as the rhythm stages: the rows stay where they are, the beat frames go to the host in their place
    rc = beat_rows_out(h->rh, h->bt, h->device, c.beat_onset, c.beat, (uint32_t)D, S, spec_rates, seg_rows, total, cur, rows, rows_capacity,
                       c.bpm_out, c.rate_out, c.refused_out, hs, err);
    if (rc) return rc;
    return sync_status_into(h, status, err);
  }
  if (const vsyn_spectral_post* post = c.post) {
    const uint64_t Dout = D * (1u + post->order);
    HIPCHK(h->pp.rows.ensure(total * Dout + 1));
    rc = post_launch(h->pp, h->device, post, (uint32_t)D, S, seg_rows, cur, h->pp.rows.p, hs, err);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(rows, h->pp.rows.p, sizeof(float) * total * Dout, hipMemcpyDeviceToHost, hs));
  } else {
    HIPCHK(hipMemcpyAsync(rows, cur, sizeof(float) * total * D, hipMemcpyDeviceToHost, hs));
  }
  return sync_status_into(h, status, err);
}

// The spectral host forms: the rows of the last host submit's PCM behind the stages of c that are present. Without a gate the rows
// are counted on the host and nothing runs for a NULL rows. With one the chain runs up to the gated plane and waits once for the
// gate's read-backs, the row counts come from those (c.frames_out: the frames behind the gate), and the loudness step, conditioning,
// spectral rows and the row stages follow on the gated plane. (c by value: a post stage that is off is dropped from it.)
static int spectral_host(vsyn_handle* h, Chain c, float* rows, uint64_t rows_capacity, uint64_t* seg_rows, vsyn_status* status, const char** err) {
  const uint32_t S = c.S, out_rate = c.out_rate;
  const uint32_t* rates = c.rates;
  const Gate* gate = c.gate.spec ? &c.gate : nullptr;
  const vsyn_spectral_spec* spec = c.spec;
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (c.loud)  // (first: a refused loudness spec writes nothing, the status included)
    if (int rc = chain_loud_check(c.loud, c.cond, S, rates, err)) return rc;
  status_reset(status);
  if (int rc = chain_check(gate, c.cond, S, rates, out_rate, err)) return rc;
  std::vector<uint32_t> sp_rates = stage_rates(S, rates, out_rate);
  // (NULL rates without a gate are spec_check's to refuse; behind a gate they skip every segment)
  if (int rc = spec_check(spec, S, gate || rates ? sp_rates.data() : nullptr, err, c.chroma)) return rc;
  if (c.estimate) {
    if (!spec_is_chroma(spec)) return fail(err, VSYN_ERR_INVALID, "a tuning estimate is for the chroma kinds, not for kind %u", spec->kind);
    vsyn_spectral_spec lin = *spec;
    lin.kind = VSYN_SPEC_LIN_POWER;
    if (int rc = tuning_check(&lin, c.estimate, 0, nullptr, err)) return rc;
    if (c.estimate->bins_per_octave != spec_chroma_or_defaults(c.chroma)->n_chroma)
      return fail(err, VSYN_ERR_INVALID, "the estimate's bins_per_octave %u is not n_chroma %u: the tuning would be in another unit",
                  c.estimate->bins_per_octave, spec_chroma_or_defaults(c.chroma)->n_chroma);
    if (S && rows && !c.tuning_out) return fail(err, VSYN_ERR_INVALID, "tuning_out is NULL");
    for (uint32_t g = 0; g < S && c.tuning_out; ++g) c.tuning_out[g] = 0.0;
  }
  if (c.hpss) {
    if (int rc = hpss_check(c.hpss, err)) return rc;
    if (spec->kind != VSYN_SPEC_MEL_POWER && spec->kind != VSYN_SPEC_LIN_POWER)
      return fail(err, VSYN_ERR_INVALID, "hpss takes the rows of mel_power or lin_power, not of kind %u", spec->kind);
    if (c.pcen && c.hpss->output != VSYN_HPSS_OUT_COMPONENT)
      return fail(err, VSYN_ERR_INVALID, "pcen takes the hpss component, not its %s", c.hpss->output == VSYN_HPSS_OUT_MASK ? "mask" : "median");
  }
  if (c.pcen) {
    if (int rc = pcen_check(c.pcen, err)) return rc;
    if (spec->kind != VSYN_SPEC_MEL_POWER && spec->kind != VSYN_SPEC_LIN_POWER)
      return fail(err, VSYN_ERR_INVALID, "pcen takes the rows of mel_power or lin_power, not of kind %u (they can be negative)", spec->kind);
    for (uint32_t g = 0; g < S; ++g)
      if (sp_rates[g] && pcen_b(c.pcen, sp_rates[g], spec->hop_length) == 0.0)
        return fail(err, VSYN_ERR_INVALID, "segment %u: pcen: no coefficient in (0, 1] from time_constant %g at rate %u, hop %u", g,
                    c.pcen->time_constant, sp_rates[g], spec->hop_length);
  }
  if (c.post) {
    if (int rc = spec_post_check(spec, c.post, err, c.chroma)) return rc;
    if (!post_on(c.post)) c.post = nullptr;  // off: the rows of the spectral pass, bit for bit
  }
  if (c.rhythm) {
    if (c.post) return fail(err, VSYN_ERR_INVALID, "delta / normalize are not available with the rhythm stages: the onset stage takes their place");
    if (int rc = rhythm_check(c.rhythm, spec->n_fft, spec->hop_length, (spec->options & VSYN_SPEC_CENTER) != 0, spec_dim(spec, c.chroma), err)) return rc;
    if (c.refused_out && S) memset(c.refused_out, 0, sizeof(uint32_t) * S);
  }
  if (c.beat) {
    if (c.post) return fail(err, VSYN_ERR_INVALID, "delta / normalize are not available with the beat tracker: the onset stage takes their place");
    if (int rc = beat_chain_check(c.beat_onset, c.beat, spec->n_fft, spec->hop_length, (spec->options & VSYN_SPEC_CENTER) != 0, spec_dim(spec, c.chroma), err))
      return rc;
    if (c.refused_out && S) memset(c.refused_out, 0, sizeof(uint32_t) * S);
    if (c.bpm_out && S) memset(c.bpm_out, 0, sizeof(double) * S);
    if (c.rate_out && S) memset(c.rate_out, 0, sizeof(uint32_t) * S);
  }
  if (S && !seg_rows) return fail(err, VSYN_ERR_INVALID, "seg_rows is NULL");
  for (uint32_t g = 0; g < S; ++g) seg_rows[g] = 0;
  if (c.peaks_out) memset(c.peaks_out, 0, sizeof(float) * S);
  if (c.records_out) memset(c.records_out, 0, sizeof(vsyn_loudness_record) * S);
  if (gate && gate->bounds) memset(gate->bounds, 0, sizeof(uint32_t) * 2u * S);
  if (gate && gate->refs) memset(gate->refs, 0, sizeof(double) * S);
  // the lock covers the whole call: the stages' workspaces are the handle's, and the PCM must stay that of the last submit
  std::lock_guard<std::mutex> lk(h->mu);
  std::vector<uint64_t> T(S);
  uint64_t total, f_max, t_max;
  if (int rc = last_submit_frames(h, S, rates, out_rate, T.data(), &t_max, err)) return rc;
  if (gate && S == 0) return VSYN_OK;
  if (gate && gate->split)
    if (int rc = split_check_stride(*gate, t_max, err)) return rc;
  t_max = std::max<uint64_t>(t_max, 1);
  if (gate && t_max > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "segment too long");
  PcmView v = last_submit_view(h);  // the spectral pass reads the synthesis PCM with the last submit's SegInfo, or what the chain made of it
  if (gate) {
    std::vector<uint32_t> bounds(2u * (size_t)S), joined(S);
    std::vector<double> refs(S);
    Gate g = *gate;
    g.frames = joined.data();
    g.bounds = bounds.data();
    g.refs = refs.data();
    if (out_rate)
      if (int rc = step_resample(h, S, rates, out_rate, t_max, false, &v, err)) return rc;
    if (int rc = step_gate(h, S, g, t_max, t_max, false, &v, err)) return rc;
    HIPCHK(hipStreamSynchronize(h->host_stream));  // the one read-back of a gated form: the bounds or the joined frames, with the refs (counts, intervals)
    for (uint32_t s = 0; s < S; ++s) {
      T[s] = g.split ? joined[s] : bounds[2u * s + 1u] - bounds[2u * s];
      if (c.frames_out) c.frames_out[s] = T[s];
      if (!std::isfinite(refs[s])) sp_rates[s] = 0u;
    }
    if (gate->bounds) memcpy(gate->bounds, bounds.data(), sizeof(uint32_t) * bounds.size());
    if (gate->refs) memcpy(gate->refs, refs.data(), sizeof(double) * S);
  }
  const bool center = (spec->options & VSYN_SPEC_CENTER) != 0;
  count_rows(spec->n_fft, spec->hop_length, center, S, sp_rates.data(), T.data(), gate && c.post && c.post->order ? c.post->width : 0u, seg_rows, &total,
             &f_max);
  if (gate) {  // gated to nothing, or below the delta width: that segment fails alone
    for (uint32_t s = 0; s < S; ++s)
      if (!seg_rows[s]) sp_rates[s] = 0u;
  } else if (c.post) {  // ungated, a segment below the delta width refuses the call
    if (int rc = post_check_rows(c.post, S, seg_rows, err)) return rc;
  }
  if (!rows || total == 0) return VSYN_OK;
  if (!c.rhythm && !c.beat && total > rows_capacity) return fail(err, VSYN_ERR_INVALID, "rows buffer too small: %llu rows needed", (unsigned long long)total);
  if (!gate && out_rate) {
    if (t_max > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "resampled segment too long");
    if (int rc = step_resample(h, S, rates, out_rate, t_max, false, &v, err)) return rc;
  }
  if (c.loud)
    if (int rc = step_loudness(h, S, c.loud, sp_rates.data(), T.data(), t_max, false, c.records_out, &v, err)) return rc;
  if (c.cond)
    if (int rc = step_condition(h, S, c.cond, t_max, t_max, false, c.peaks_out, &v, err)) return rc;
  return spectral_rows_out(h, c, sp_rates.data(), v, seg_rows, f_max, total, rows, rows_capacity, status, err);
}

// vsyn_pcm_split_intervals_host: the chain up to the split stage's marks; nothing but the frames in front of the stage, the
// counts, the intervals and the refs comes back.
static int split_intervals_host(vsyn_handle* h, const Gate& g, uint32_t S, const uint32_t* rates, uint32_t out_rate, uint64_t* frames_out,
                                const char** err) {
  if (int rc = chain_check(&g, nullptr, S, rates, out_rate, err)) return rc;
  if (S && !frames_out) return fail(err, VSYN_ERR_INVALID, "frames_out is NULL");
  // the lock covers the whole call: the resample and split workspaces are the handle's, and the PCM must stay that of the last submit
  std::lock_guard<std::mutex> lk(h->mu);
  uint64_t t_max;
  if (int rc = last_submit_frames(h, S, rates, out_rate, frames_out, &t_max, err)) return rc;
  if (!g.counts || S == 0) return VSYN_OK;
  if (int rc = split_check_stride(g, t_max, err)) return rc;
  if (t_max > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "segment too long");
  PcmView v = last_submit_view(h);  // resampled into a plane as long as the longest segment, marked there
  if (out_rate)
    if (int rc = step_resample(h, S, rates, out_rate, std::max<uint64_t>(t_max, 1), false, &v, err)) return rc;
  if (int rc = step_gate(h, S, g, 0, t_max, false, &v, err)) return rc;
  HIPCHK(hipStreamSynchronize(h->host_stream));
  return VSYN_OK;
}

static bool pitch_center(const vsyn_pitch_spec* spec) { return (spec->options & VSYN_PITCH_CENTER) != 0; }
static bool fdesc_center(const vsyn_fdesc_spec* spec) { return (spec->options & VSYN_FDESC_CENTER) != 0; }

// The host forms whose rows come from a framing of the PCM as the resampler leaves it (vsyn_pcm_pitch_host, vsyn_pcm_fdesc_host),
// behind their spec checks: frames of n samples every hop, cols columns a row; launch(v, f_max, stream) runs the stage's kernels
// over the view into d_rows and d_refused. rates: what the stage sees (stage_rates, or the caller's own).
template <class Launch>
static int framed_rows_host(vsyn_handle* h, uint32_t n, uint32_t hop, bool center, uint32_t cols, DevBuf<float>& d_rows, DevBuf<uint32_t>& d_refused,
                            Launch launch, uint32_t S, const uint32_t* in_rates, uint32_t out_rate, const uint32_t* rates, float* rows,
                            uint64_t rows_capacity, uint64_t* seg_rows, uint32_t* refused_out, vsyn_status* status, const char** err) {
  if (S && !seg_rows) return fail(err, VSYN_ERR_INVALID, "seg_rows is NULL");
  for (uint32_t g = 0; g < S; ++g) seg_rows[g] = 0;
  if (refused_out) memset(refused_out, 0, sizeof(uint32_t) * S);
  // the lock covers the whole call: the resample workspace and the stage's are the handle's, and the PCM must stay that of the last submit
  std::lock_guard<std::mutex> lk(h->mu);
  std::vector<uint64_t> T(S);
  uint64_t total, f_max, t_max;
  if (int rc = last_submit_frames(h, S, in_rates, out_rate, T.data(), &t_max, err)) return rc;
  t_max = std::max<uint64_t>(t_max, 1);
  count_rows(n, hop, center, S, rates, T.data(), 0, seg_rows, &total, &f_max);
  if (!rows || S == 0) return VSYN_OK;
  if (total > rows_capacity) return fail(err, VSYN_ERR_INVALID, "rows buffer too small: %llu rows needed", (unsigned long long)total);
  if (out_rate && t_max > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "resampled segment too long");
  hipStream_t hs = h->host_stream;
  PcmView v = last_submit_view(h);  // the synthesis PCM with the last submit's SegInfo, or the resampler's planes with its frames
  if (out_rate)
    if (int rc = step_resample(h, S, in_rates, out_rate, t_max, false, &v, err)) return rc;
  HIPCHK(d_rows.ensure(total * cols + 1));
  HIPCHK(d_refused.ensure(S));
  if (int rc = launch(v, f_max, hs)) return rc;
  if (total) HIPCHK(hipMemcpyAsync(rows, d_rows.p, sizeof(float) * total * cols, hipMemcpyDeviceToHost, hs));
  if (refused_out) HIPCHK(hipMemcpyAsync(refused_out, d_refused.p, sizeof(uint32_t) * S, hipMemcpyDeviceToHost, hs));
  return sync_status_into(h, status, err);
}

extern "C" {

uint64_t vsyn_resample_num_frames(uint32_t r_in, uint32_t r_out, uint64_t frames) {
  uint32_t up, down;
  if (!rs_ratio(r_in, r_out, &up, &down)) return 0;
  const unsigned __int128 n = ((unsigned __int128)frames * up + down - 1u) / down;
  return n > (unsigned __int128)UINT64_MAX ? 0 : (uint64_t)n;
}

int vsyn_resample_device(vsyn_handle* h, uint32_t S, const uint32_t* in_rates, uint32_t out_rate, const float* d_pcm, uint64_t plane_stride,
                         uint32_t channels, const uint32_t* d_frames, float* d_out, uint64_t out_plane_stride, uint32_t* d_out_frames,
                         void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  int rc = rs_check(S, in_rates, out_rate, err);
  if (rc) return rc;
  if (S == 0) return VSYN_OK;
  if (!d_pcm || !d_frames || !d_out || !d_out_frames || plane_stride == 0 || channels == 0 || channels > 255)
    return fail(err, VSYN_ERR_INVALID, "NULL pointer, zero stride or channels outside [1, 255]");
  if (out_plane_stride > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "out_plane_stride must be below 2^32");
  const uint64_t T_max = std::min<uint64_t>(plane_stride, 0xFFFFFFFFull);
  for (uint32_t g = 0; g < S; ++g) {
    if (!in_rates[g]) continue;
    const uint64_t need = vsyn_resample_num_frames(in_rates[g], out_rate, T_max);
    if (need > out_plane_stride)
      return fail(err, VSYN_ERR_INVALID, "segment %u: out_plane_stride %llu below %llu frames", g, (unsigned long long)out_plane_stride,
                  (unsigned long long)need);
  }
  std::lock_guard<std::mutex> lk(h->mu);
  return rs_launch(h->rs, h->device, S, in_rates, out_rate, d_pcm, plane_stride, channels, d_frames, nullptr, d_out, out_plane_stride, d_out_frames,
                   (hipStream_t)hip_stream, err);
}

int vsyn_pcm_resample_host(vsyn_handle* h, uint32_t S, const uint32_t* in_rates, uint32_t out_rate, int format, void* out,
                           uint64_t out_stride_frames, uint64_t* frames_out, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (!out_rate) return rs_check(S, in_rates, out_rate, err);  // (0 would mean no resampling to the shared body)
  Chain c{S, in_rates, out_rate};
  c.frames_out = frames_out;
  return pcm_out_host(h, c, format, out, out_stride_frames, err);
}

int vsyn_pcm_spectral_host(vsyn_handle* h, const vsyn_spectral_spec* spec, uint32_t S, const uint32_t* sample_rates, float* rows,
                           uint64_t rows_capacity, uint64_t* seg_rows, vsyn_status* status, const char** err) {
  Chain c{S, sample_rates, 0};
  c.spec = spec;
  return spectral_host(h, c, rows, rows_capacity, seg_rows, status, err);
}

int vsyn_pcm_spectral_post_host(vsyn_handle* h, const vsyn_spectral_spec* spec, const vsyn_spectral_post* post, uint32_t S,
                                const uint32_t* in_rates, uint32_t out_rate, float* rows, uint64_t rows_capacity, uint64_t* seg_rows,
                                vsyn_status* status, const char** err) {
  if (!post) return fail(err, VSYN_ERR_INVALID, "spectral post spec is NULL");
  Chain c{S, in_rates, out_rate};
  c.spec = spec;
  c.post = post;
  return spectral_host(h, c, rows, rows_capacity, seg_rows, status, err);
}

int vsyn_pcm_resample_spectral_host(vsyn_handle* h, const vsyn_spectral_spec* spec, uint32_t S, const uint32_t* in_rates, uint32_t out_rate,
                                    float* rows, uint64_t rows_capacity, uint64_t* seg_rows, vsyn_status* status, const char** err) {
  if (h && !out_rate) {  // out_rate 0 would mean no resampling to the shared body: rs_check refuses it here
    status_reset(status);
    return rs_check(S, in_rates, out_rate, err);
  }
  Chain c{S, in_rates, out_rate};
  c.spec = spec;
  return spectral_host(h, c, rows, rows_capacity, seg_rows, status, err);
}

int vsyn_pcm_cond_spectral_host(vsyn_handle* h, const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec, const vsyn_spectral_post* post,
                                uint32_t S, const uint32_t* in_rates, uint32_t out_rate, float* rows, uint64_t rows_capacity,
                                uint64_t* seg_rows, float* peaks_out, vsyn_status* status, const char** err) {
  if (!h) return cond_no_handle(err);
  Chain c{S, in_rates, out_rate};
  c.cond = cond;
  c.spec = spec;
  c.post = post;
  c.peaks_out = peaks_out;
  return spectral_host(h, c, rows, rows_capacity, seg_rows, status, err);
}

int vsyn_pcm_condition_device(vsyn_handle* h, const vsyn_pcm_cond* cond, uint32_t S, const float* d_pcm, uint64_t plane_stride,
                              uint32_t channels, const uint32_t* d_frames, float* d_out, uint64_t out_plane_stride, float* d_peaks,
                              void* hip_stream, const char** err) {
  if (!h) return cond_no_handle(err);
  int rc = cond_check(cond, err);
  if (rc) return rc;
  if (channels == 0 || channels > 255) return fail(err, VSYN_ERR_INVALID, "channels %u outside [1, 255]", channels);
  if (S == 0) return VSYN_OK;
  if (!d_pcm || !d_frames || !d_out || plane_stride == 0 || out_plane_stride == 0)
    return fail(err, VSYN_ERR_INVALID, "NULL pointer or zero stride");
  if (plane_stride > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "plane_stride must be below 2^32");
  std::lock_guard<std::mutex> lk(h->mu);
  return cond_launch(h->cd, h->device, cond, S, d_pcm, plane_stride, channels, d_frames, nullptr, plane_stride, d_out, out_plane_stride, (uint32_t*)d_peaks,
                     (hipStream_t)hip_stream, err);
}

}  // extern "C"

// The PCM host forms behind vsyn_pcm_resample_host. A chain without a stage is vsyn_pcm_condition_host, which needs its spec.
static int pcm_form_host(vsyn_handle* h, const Chain& c, int format, void* out, uint64_t out_stride_frames, const char** err) {
  if (!h) return cond_no_handle(err);
  if (!c.gate.spec && !c.effect && !c.stretch.spec && !c.loud && !c.cond) return cond_check(c.cond, err);
  return pcm_out_host(h, c, format, out, out_stride_frames, err);
}

extern "C" {

int vsyn_pcm_condition_host(vsyn_handle* h, const vsyn_pcm_cond* cond, uint32_t S, const uint32_t* in_rates, uint32_t out_rate, int format,
                            void* out, uint64_t out_stride_frames, uint64_t* frames_out, float* peaks_out, const char** err) {
  Chain c{S, in_rates, out_rate};
  c.cond = cond;
  c.frames_out = frames_out;
  c.peaks_out = peaks_out;
  return pcm_form_host(h, c, format, out, out_stride_frames, err);
}

uint64_t vsyn_pcm_trim_num_frames(const vsyn_pcm_trim* trim, uint64_t frames) {
  if (trim_check(trim, nullptr) != VSYN_OK) return 0;
  return trim_num_frames(frames, trim->frame_length, trim->hop_length);
}

int vsyn_pcm_trim_device(vsyn_handle* h, const vsyn_pcm_trim* trim, uint32_t S, const float* d_pcm, uint64_t plane_stride, uint32_t channels,
                         const uint32_t* d_frames, float* d_out, uint64_t out_plane_stride, uint32_t* d_out_frames, uint32_t* d_bounds,
                         double* d_ref, double* d_ms, uint64_t ms_stride, void* hip_stream, const char** err) {
  if (!h) return cond_no_handle(err);
  int rc = trim_check(trim, err);
  if (rc) return rc;
  if (channels == 0 || channels > 255) return fail(err, VSYN_ERR_INVALID, "channels %u outside [1, 255]", channels);
  if (S == 0) return VSYN_OK;
  if (!d_pcm || !d_frames || !d_out || !d_out_frames || !d_bounds || plane_stride == 0 || out_plane_stride == 0)
    return fail(err, VSYN_ERR_INVALID, "NULL pointer or zero stride");
  if (plane_stride > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "plane_stride must be below 2^32");
  std::lock_guard<std::mutex> lk(h->mu);
  return trim_launch(h->tr, h->device, trim, S, d_pcm, plane_stride, channels, d_frames, nullptr, plane_stride, d_out, out_plane_stride, d_out_frames,
                     d_bounds, d_ref, d_ms, ms_stride, (hipStream_t)hip_stream, err);
}

int vsyn_pcm_trim_host(vsyn_handle* h, const vsyn_pcm_trim* trim, const vsyn_pcm_cond* cond, uint32_t S, const uint32_t* in_rates,
                       uint32_t out_rate, int format, void* out, uint64_t out_stride_frames, uint64_t* frames_out, uint32_t* bounds_out,
                       float* peaks_out, double* refs_out, const char** err) {
  return vsyn_pcm_chain_host(h, trim, 0, nullptr, cond, S, in_rates, out_rate, format, out, out_stride_frames, frames_out, bounds_out, nullptr, nullptr,
                             0, peaks_out, refs_out, nullptr, err);
}

int vsyn_pcm_trim_spectral_host(vsyn_handle* h, const vsyn_pcm_trim* trim, const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec,
                                const vsyn_spectral_post* post, uint32_t S, const uint32_t* in_rates, uint32_t out_rate, float* rows,
                                uint64_t rows_capacity, uint64_t* seg_rows, uint32_t* bounds_out, float* peaks_out, double* refs_out,
                                vsyn_status* status, const char** err) {
  return vsyn_pcm_trim_spectral_pcen_host(h, trim, cond, spec, nullptr, post, S, in_rates, out_rate, rows, rows_capacity, seg_rows, bounds_out, peaks_out,
                                          refs_out, status, err);
}

int vsyn_pcm_trim_spectral_pcen_host(vsyn_handle* h, const vsyn_pcm_trim* trim, const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec,
                                     const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post, uint32_t S, const uint32_t* in_rates,
                                     uint32_t out_rate, float* rows, uint64_t rows_capacity, uint64_t* seg_rows, uint32_t* bounds_out,
                                     float* peaks_out, double* refs_out, vsyn_status* status, const char** err) {
  return vsyn_pcm_chain_spectral_host(h, trim, 0, nullptr, cond, spec, pcen, post, S, in_rates, out_rate, rows, rows_capacity, seg_rows, nullptr,
                                      bounds_out, nullptr, nullptr, 0, peaks_out, refs_out, nullptr, status, err);
}

uint64_t vsyn_pcm_split_max_intervals(const vsyn_pcm_trim* trim, uint64_t frames) {
  if (trim_check(trim, nullptr) != VSYN_OK) return 0;
  return split_max_intervals(frames, trim->frame_length, trim->hop_length);
}

int vsyn_pcm_split_device(vsyn_handle* h, const vsyn_pcm_trim* trim, uint32_t S, const float* d_pcm, uint64_t plane_stride, uint32_t channels,
                          const uint32_t* d_frames, float* d_out, uint64_t out_plane_stride, uint32_t* d_out_frames, uint32_t* d_counts,
                          uint32_t* d_intervals, uint64_t intervals_stride, double* d_ref, double* d_ms, uint64_t ms_stride, void* hip_stream,
                          const char** err) {
  if (!h) return cond_no_handle(err);
  int rc = trim_check(trim, err);
  if (rc) return rc;
  if (channels == 0 || channels > 255) return fail(err, VSYN_ERR_INVALID, "channels %u outside [1, 255]", channels);
  if (S == 0) return VSYN_OK;
  if (!d_pcm || !d_frames || !d_out || !d_out_frames || !d_counts || !d_intervals || plane_stride == 0 || out_plane_stride == 0)
    return fail(err, VSYN_ERR_INVALID, "NULL pointer or zero stride");
  if (plane_stride > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "plane_stride must be below 2^32");
  std::lock_guard<std::mutex> lk(h->mu);
  return split_launch(h->sl, h->device, trim, S, d_pcm, plane_stride, channels, d_frames, nullptr, plane_stride, d_out, out_plane_stride, d_out_frames,
                      d_counts, d_intervals, intervals_stride, nullptr, d_ref, d_ms, ms_stride, (hipStream_t)hip_stream, err);
}

int vsyn_pcm_split_host(vsyn_handle* h, const vsyn_pcm_trim* trim, const vsyn_pcm_cond* cond, uint32_t S, const uint32_t* in_rates,
                        uint32_t out_rate, int format, void* out, uint64_t out_stride_frames, uint64_t* frames_out, uint32_t* counts_out,
                        uint32_t* intervals_out, uint64_t intervals_stride, float* peaks_out, double* refs_out, const char** err) {
  return vsyn_pcm_chain_host(h, trim, 1, nullptr, cond, S, in_rates, out_rate, format, out, out_stride_frames, frames_out, nullptr, counts_out,
                             intervals_out, intervals_stride, peaks_out, refs_out, nullptr, err);
}

int vsyn_pcm_split_intervals_host(vsyn_handle* h, const vsyn_pcm_trim* trim, uint32_t S, const uint32_t* in_rates, uint32_t out_rate,
                                  uint64_t* frames_out, uint32_t* counts_out, uint32_t* intervals_out, uint64_t intervals_stride,
                                  double* refs_out, const char** err) {
  if (!h) return cond_no_handle(err);
  Gate g = make_gate(trim, true, nullptr, counts_out, intervals_out, intervals_stride, refs_out);
  g.gather = false;
  return split_intervals_host(h, g, S, in_rates, out_rate, frames_out, err);
}

int vsyn_pcm_split_spectral_host(vsyn_handle* h, const vsyn_pcm_trim* trim, const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec,
                                 const vsyn_spectral_post* post, uint32_t S, const uint32_t* in_rates, uint32_t out_rate, float* rows,
                                 uint64_t rows_capacity, uint64_t* seg_rows, uint64_t* frames_out, uint32_t* counts_out, uint32_t* intervals_out,
                                 uint64_t intervals_stride, float* peaks_out, double* refs_out, vsyn_status* status, const char** err) {
  return vsyn_pcm_split_spectral_pcen_host(h, trim, cond, spec, nullptr, post, S, in_rates, out_rate, rows, rows_capacity, seg_rows, frames_out,
                                           counts_out, intervals_out, intervals_stride, peaks_out, refs_out, status, err);
}

int vsyn_pcm_split_spectral_pcen_host(vsyn_handle* h, const vsyn_pcm_trim* trim, const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec,
                                      const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post, uint32_t S, const uint32_t* in_rates,
                                      uint32_t out_rate, float* rows, uint64_t rows_capacity, uint64_t* seg_rows, uint64_t* frames_out,
                                      uint32_t* counts_out, uint32_t* intervals_out, uint64_t intervals_stride, float* peaks_out, double* refs_out,
                                      vsyn_status* status, const char** err) {
  return vsyn_pcm_chain_spectral_host(h, trim, 1, nullptr, cond, spec, pcen, post, S, in_rates, out_rate, rows, rows_capacity, seg_rows, frames_out,
                                      nullptr, counts_out, intervals_out, intervals_stride, peaks_out, refs_out, nullptr, status, err);
}

// The most general PCM and spectral host forms: every stage's spec, NULL for a stage that is off; the gate is a trim, or with
// gate_is_split != 0 a split. An entry with a stage passed as NULL is the entry without that argument: each narrower entry is the
// widest one, vsyn_pcm_chain_stretch_host or vsyn_pcm_chain_rhythm_host, with NULL for what it does not take.
int vsyn_pcm_chain_host(vsyn_handle* h, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud, const vsyn_pcm_cond* cond,
                        uint32_t S, const uint32_t* in_rates, uint32_t out_rate, int format, void* out, uint64_t out_stride_frames,
                        uint64_t* frames_out, uint32_t* bounds_out, uint32_t* counts_out, uint32_t* intervals_out, uint64_t intervals_stride,
                        float* peaks_out, double* refs_out, vsyn_loudness_record* records_out, const char** err) {
  return vsyn_pcm_chain_stretch_host(h, gate, gate_is_split, nullptr, nullptr, nullptr, nullptr, loud, cond, S, in_rates, out_rate, format, out,
                                     out_stride_frames, frames_out, bounds_out, counts_out, intervals_out, intervals_stride, peaks_out, refs_out,
                                     records_out, err);
}

int vsyn_pcm_chain_effects_host(vsyn_handle* h, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_pcm_effect* effect,
                                const vsyn_loudness_spec* loud, const vsyn_pcm_cond* cond, uint32_t S, const uint32_t* in_rates, uint32_t out_rate,
                                int format, void* out, uint64_t out_stride_frames, uint64_t* frames_out, uint32_t* bounds_out, uint32_t* counts_out,
                                uint32_t* intervals_out, uint64_t intervals_stride, float* peaks_out, double* refs_out,
                                vsyn_loudness_record* records_out, const char** err) {
  return vsyn_pcm_chain_stretch_host(h, gate, gate_is_split, effect, nullptr, nullptr, nullptr, loud, cond, S, in_rates, out_rate, format, out,
                                     out_stride_frames, frames_out, bounds_out, counts_out, intervals_out, intervals_stride, peaks_out, refs_out,
                                     records_out, err);
}

// The widest PCM form. The outputs of the gate that is off, and the records without a normaliser, are not written.
int vsyn_pcm_chain_stretch_host(vsyn_handle* h, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_pcm_effect* effect,
                                const vsyn_pcm_stretch* stretch, const double* stretch_rates, const uint32_t* shift_from_hz,
                                const vsyn_loudness_spec* loud, const vsyn_pcm_cond* cond, uint32_t S, const uint32_t* in_rates, uint32_t out_rate,
                                int format, void* out, uint64_t out_stride_frames, uint64_t* frames_out, uint32_t* bounds_out, uint32_t* counts_out,
                                uint32_t* intervals_out, uint64_t intervals_stride, float* peaks_out, double* refs_out,
                                vsyn_loudness_record* records_out, const char** err) {
  Chain c{S, in_rates, out_rate};
  c.gate = make_gate(gate, gate && gate_is_split, bounds_out, counts_out, intervals_out, intervals_stride, refs_out);
  c.effect = effect;
  c.stretch = Stretch{stretch, stretch_rates, stretch && stretch->shift_to_hz ? shift_from_hz : nullptr};
  c.loud = loud;
  c.cond = cond;
  c.frames_out = frames_out;
  c.peaks_out = peaks_out;
  c.records_out = loud ? records_out : nullptr;
  return pcm_form_host(h, c, format, out, out_stride_frames, err);
}

int vsyn_pcm_chain_spectral_host(vsyn_handle* h, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud,
                                 const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec, const vsyn_spectral_pcen* pcen,
                                 const vsyn_spectral_post* post, uint32_t S, const uint32_t* in_rates, uint32_t out_rate, float* rows,
                                 uint64_t rows_capacity, uint64_t* seg_rows, uint64_t* frames_out, uint32_t* bounds_out, uint32_t* counts_out,
                                 uint32_t* intervals_out, uint64_t intervals_stride, float* peaks_out, double* refs_out,
                                 vsyn_loudness_record* records_out, vsyn_status* status, const char** err) {
  return vsyn_pcm_chain_rhythm_host(h, gate, gate_is_split, loud, cond, spec, nullptr, nullptr, pcen, post, nullptr, S, in_rates, out_rate, rows,
                                    rows_capacity, seg_rows, frames_out, bounds_out, counts_out, intervals_out, intervals_stride, peaks_out, refs_out,
                                    records_out, nullptr, status, err);
}

int vsyn_pcm_chain_chroma_host(vsyn_handle* h, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud,
                               const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma,
                               const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post, uint32_t S, const uint32_t* in_rates,
                               uint32_t out_rate, float* rows, uint64_t rows_capacity, uint64_t* seg_rows, uint64_t* frames_out,
                               uint32_t* bounds_out, uint32_t* counts_out, uint32_t* intervals_out, uint64_t intervals_stride, float* peaks_out,
                               double* refs_out, vsyn_loudness_record* records_out, vsyn_status* status, const char** err) {
  return vsyn_pcm_chain_rhythm_host(h, gate, gate_is_split, loud, cond, spec, chroma, nullptr, pcen, post, nullptr, S, in_rates, out_rate, rows,
                                    rows_capacity, seg_rows, frames_out, bounds_out, counts_out, intervals_out, intervals_stride, peaks_out, refs_out,
                                    records_out, nullptr, status, err);
}

int vsyn_pcm_chain_hpss_host(vsyn_handle* h, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud,
                             const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma,
                             const vsyn_spectral_hpss* hpss, const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post, uint32_t S,
                             const uint32_t* in_rates, uint32_t out_rate, float* rows, uint64_t rows_capacity, uint64_t* seg_rows,
                             uint64_t* frames_out, uint32_t* bounds_out, uint32_t* counts_out, uint32_t* intervals_out, uint64_t intervals_stride,
                             float* peaks_out, double* refs_out, vsyn_loudness_record* records_out, vsyn_status* status, const char** err) {
  return vsyn_pcm_chain_rhythm_host(h, gate, gate_is_split, loud, cond, spec, chroma, hpss, pcen, post, nullptr, S, in_rates, out_rate, rows,
                                    rows_capacity, seg_rows, frames_out, bounds_out, counts_out, intervals_out, intervals_stride, peaks_out, refs_out,
                                    records_out, nullptr, status, err);
}

// The widest spectral form. What the narrower entries fixed by handing a NULL stage down, written out: a NULL handle is refused in
// the words of the conditioning entries; the chroma parameters are read for a chroma kind only; the body is given frames_out behind
// a split, or behind any gate with the normaliser, and records_out with the normaliser.
int vsyn_pcm_chain_rhythm_host(vsyn_handle* h, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud,
                               const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma,
                               const vsyn_spectral_hpss* hpss, const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post,
                               const vsyn_rhythm_spec* rhythm, uint32_t S, const uint32_t* in_rates, uint32_t out_rate, float* rows,
                               uint64_t rows_capacity, uint64_t* seg_rows, uint64_t* frames_out, uint32_t* bounds_out, uint32_t* counts_out,
                               uint32_t* intervals_out, uint64_t intervals_stride, float* peaks_out, double* refs_out,
                               vsyn_loudness_record* records_out, uint32_t* refused_out, vsyn_status* status, const char** err) {
  if (!h) return cond_no_handle(err);
  const bool split = gate && gate_is_split;
  Chain c{S, in_rates, out_rate};
  c.gate = make_gate(gate, split, bounds_out, counts_out, intervals_out, intervals_stride, refs_out);
  c.loud = loud;
  c.cond = cond;
  c.spec = spec;
  c.chroma = spec && spec_is_chroma(spec) ? chroma : nullptr;
  c.hpss = hpss;
  c.pcen = pcen;
  c.post = post;
  c.rhythm = rhythm;
  c.frames_out = gate && (loud || split) ? frames_out : nullptr;
  c.peaks_out = peaks_out;
  c.records_out = loud ? records_out : nullptr;
  c.refused_out = refused_out;
  return spectral_host(h, c, rows, rows_capacity, seg_rows, status, err);
}

// vsyn_pcm_chain_chroma_host with each segment's tuning estimated first (estimate NULL: that entry, tuning_out not written).
int vsyn_pcm_chain_chroma_est_host(vsyn_handle* h, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud,
                                   const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma,
                                   const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post, const vsyn_tuning_spec* estimate, uint32_t S,
                                   const uint32_t* in_rates, uint32_t out_rate, float* rows, uint64_t rows_capacity, uint64_t* seg_rows,
                                   uint64_t* frames_out, uint32_t* bounds_out, uint32_t* counts_out, uint32_t* intervals_out,
                                   uint64_t intervals_stride, float* peaks_out, double* refs_out, vsyn_loudness_record* records_out,
                                   double* tuning_out, vsyn_status* status, const char** err) {
  if (!h) return cond_no_handle(err);
  const bool split = gate && gate_is_split;
  Chain c{S, in_rates, out_rate};
  c.gate = make_gate(gate, split, bounds_out, counts_out, intervals_out, intervals_stride, refs_out);
  c.loud = loud;
  c.cond = cond;
  c.spec = spec;
  c.chroma = spec && spec_is_chroma(spec) ? chroma : nullptr;
  c.pcen = pcen;
  c.post = post;
  c.frames_out = gate && (loud || split) ? frames_out : nullptr;
  c.peaks_out = peaks_out;
  c.records_out = loud ? records_out : nullptr;
  c.estimate = estimate;
  c.tuning_out = estimate ? tuning_out : nullptr;
  return spectral_host(h, c, rows, rows_capacity, seg_rows, status, err);
}

// vsyn_pcm_chain_rhythm_host's chain with the beat tracker in the rhythm stages' place (vsyn_beat.h).
int vsyn_pcm_chain_beats_host(vsyn_handle* h, const vsyn_pcm_trim* gate, int gate_is_split, const vsyn_loudness_spec* loud,
                              const vsyn_pcm_cond* cond, const vsyn_spectral_spec* spec, const vsyn_spectral_chroma* chroma,
                              const vsyn_spectral_hpss* hpss, const vsyn_spectral_pcen* pcen, const vsyn_spectral_post* post,
                              const vsyn_onset_spec* onset, const vsyn_beat_spec* beat, uint32_t S, const uint32_t* in_rates, uint32_t out_rate,
                              float* rows, uint64_t rows_capacity, uint64_t* seg_rows, uint64_t* frames_out, uint32_t* bounds_out,
                              uint32_t* counts_out, uint32_t* intervals_out, uint64_t intervals_stride, float* peaks_out, double* refs_out,
                              vsyn_loudness_record* records_out, double* bpm_out, uint32_t* rate_out, uint32_t* refused_out, vsyn_status* status,
                              const char** err) {
  if (!h) return cond_no_handle(err);
  if (!beat || !onset) return fail(err, VSYN_ERR_INVALID, "vsyn_pcm_chain_beats_host needs a beat spec and an onset spec");
  const bool split = gate && gate_is_split;
  Chain c{S, in_rates, out_rate};
  c.gate = make_gate(gate, split, bounds_out, counts_out, intervals_out, intervals_stride, refs_out);
  c.loud = loud;
  c.cond = cond;
  c.spec = spec;
  c.chroma = spec && spec_is_chroma(spec) ? chroma : nullptr;
  c.hpss = hpss;
  c.pcen = pcen;
  c.post = post;
  c.beat_onset = onset;
  c.beat = beat;
  c.bpm_out = bpm_out;
  c.rate_out = rate_out;
  c.frames_out = gate && (loud || split) ? frames_out : nullptr;
  c.peaks_out = peaks_out;
  c.records_out = loud ? records_out : nullptr;
  c.refused_out = refused_out;
  return spectral_host(h, c, rows, rows_capacity, seg_rows, status, err);
}

// ---- pitch (vsyn_pitch.h) ----

uint64_t vsyn_pitch_num_frames(const vsyn_pitch_spec* spec, uint64_t frames) {
  if (pitch_check(spec, 0, nullptr, nullptr) != VSYN_OK) return 0;
  return spec_num_frames(spec->frame_length, spec->hop_length, pitch_center(spec), frames);
}

int vsyn_pitch_device(vsyn_handle* h, const vsyn_pitch_spec* spec, uint32_t S, const uint32_t* sample_rates, const float* d_pcm,
                      uint64_t plane_stride, uint32_t channels, const uint32_t* d_frames, float* d_rows, uint64_t* d_seg_row_off,
                      uint32_t* d_refused, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  int rc = pitch_check(spec, S, sample_rates, err);
  if (rc) return rc;
  if (S == 0) return VSYN_OK;
  if (!d_pcm || !d_frames || !d_rows || plane_stride == 0 || channels == 0 || channels > 255)
    return fail(err, VSYN_ERR_INVALID, "NULL pointer, zero stride or channels outside [1, 255]");
  const uint64_t f_max = spec_num_frames(spec->frame_length, spec->hop_length, pitch_center(spec), plane_stride);
  std::lock_guard<std::mutex> lk(h->mu);
  return pitch_launch(h->pt, h->device, spec, S, sample_rates, d_pcm, plane_stride, channels, d_frames, nullptr, f_max, d_rows, d_seg_row_off,
                      d_refused, (hipStream_t)hip_stream, err);
}

int vsyn_pcm_pitch_host(vsyn_handle* h, const vsyn_pitch_spec* spec, uint32_t S, const uint32_t* in_rates, uint32_t out_rate, float* rows,
                        uint64_t rows_capacity, uint64_t* seg_rows, uint32_t* refused_out, vsyn_status* status, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  status_reset(status);
  if (int rc = chain_check(nullptr, nullptr, S, in_rates, out_rate, err)) return rc;
  const std::vector<uint32_t> pt_rates = stage_rates(S, in_rates, out_rate);
  const uint32_t* rates = out_rate ? pt_rates.data() : in_rates;
  if (int rc = pitch_check(spec, S, rates, err)) return rc;
  return framed_rows_host(
      h, spec->frame_length, spec->hop_length, pitch_center(spec), 2u, h->pt.rows, h->pt.refused,
      [&](const PcmView& v, uint64_t f_max, hipStream_t hs) {
        return pitch_launch(h->pt, h->device, spec, S, rates, v.pcm, v.plane, v.C, v.d_frames, v.si, f_max, h->pt.rows.p, nullptr, h->pt.refused.p, hs, err);
      },
      S, in_rates, out_rate, rates, rows, rows_capacity, seg_rows, refused_out, status, err);
}

// ---- pyin (vsyn_pyin.h) ----

uint64_t vsyn_pyin_num_frames(const vsyn_pyin_spec* spec, uint64_t frames) {
  if (pyin_check(spec, 0, nullptr, nullptr) != VSYN_OK) return 0;
  return spec_num_frames(spec->frame_length, spec->hop_length, pyin_center(spec), frames);
}

uint32_t vsyn_pyin_num_bins(const vsyn_pyin_spec* spec) { return pyin_check(spec, 0, nullptr, nullptr) == VSYN_OK ? pyin_bins(spec) : 0u; }

int vsyn_pyin_transition(const vsyn_pyin_spec* spec, uint32_t sample_rate, uint32_t* width_out, uint32_t* bins_out, double* table,
                         uint64_t table_capacity, const char** err) {
  if (!sample_rate) return fail(err, VSYN_ERR_INVALID, "sample_rate is 0");
  if (int rc = pyin_check(spec, 1, &sample_rate, err)) return rc;
  const uint32_t B = pyin_bins(spec), w = pyin_width(spec, sample_rate);
  if (width_out) *width_out = w;
  if (bins_out) *bins_out = B;
  if (!table) return VSYN_OK;
  if (table_capacity < (uint64_t)B * w * 2u)
    return fail(err, VSYN_ERR_INVALID, "transition table too small: %llu doubles needed", (unsigned long long)B * w * 2u);
  for (uint32_t i = 0; i < B; ++i) pyin_log_row(spec, B, w / 2u, i, table + (size_t)i * w * 2u);
  return VSYN_OK;
}

int vsyn_pyin_device(vsyn_handle* h, const vsyn_pyin_spec* spec, uint32_t S, const uint32_t* sample_rates, const float* d_pcm,
                     uint64_t plane_stride, uint32_t channels, const uint32_t* d_frames, float* d_rows, uint64_t* d_seg_row_off,
                     uint32_t* d_refused, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  int rc = pyin_check(spec, S, sample_rates, err);
  if (rc) return rc;
  if (S == 0) return VSYN_OK;
  if (!d_pcm || !d_frames || !d_rows || plane_stride == 0 || channels == 0 || channels > 255)
    return fail(err, VSYN_ERR_INVALID, "NULL pointer, zero stride or channels outside [1, 255]");
  const uint64_t f_max = spec_num_frames(spec->frame_length, spec->hop_length, pyin_center(spec), plane_stride);
  std::lock_guard<std::mutex> lk(h->mu);
  return pyin_launch(h->py, h->device, spec, S, sample_rates, d_pcm, plane_stride, channels, d_frames, nullptr, f_max, f_max * S, d_rows,
                     d_seg_row_off, d_refused, (hipStream_t)hip_stream, err);
}

int vsyn_pyin_decode_device(vsyn_handle* h, const vsyn_pyin_spec* spec, uint32_t S, const uint32_t* sample_rates, const double* d_obs,
                            const uint64_t* seg_rows, uint32_t* d_states, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (int rc = pyin_check(spec, S, sample_rates, err)) return rc;
  if (int rc = rows_check_segs(S, seg_rows, 0xFFFFFFFFull, err)) return rc;
  if (S == 0) return VSYN_OK;
  if (!d_obs || !d_states || ((uintptr_t)d_obs & 7u) || ((uintptr_t)d_states & 3u))
    return fail(err, VSYN_ERR_INVALID, "NULL or misaligned observation or state pointer");
  std::lock_guard<std::mutex> lk(h->mu);
  return pyin_decode_launch(h->py, h->device, spec, S, sample_rates, d_obs, seg_rows, d_states, (hipStream_t)hip_stream, err);
}

int vsyn_pcm_pyin_host(vsyn_handle* h, const vsyn_pyin_spec* spec, uint32_t S, const uint32_t* in_rates, uint32_t out_rate, float* rows,
                       uint64_t rows_capacity, uint64_t* seg_rows, uint32_t* refused_out, vsyn_status* status, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  status_reset(status);
  if (int rc = chain_check(nullptr, nullptr, S, in_rates, out_rate, err)) return rc;
  const std::vector<uint32_t> py_rates = stage_rates(S, in_rates, out_rate);
  const uint32_t* rates = out_rate ? py_rates.data() : in_rates;
  if (int rc = pyin_check(spec, S, rates, err)) return rc;
  return framed_rows_host(
      h, spec->frame_length, spec->hop_length, pyin_center(spec), 3u, h->py.rows, h->py.refused,
      [&](const PcmView& v, uint64_t f_max, hipStream_t hs) {
        return pyin_launch(h->py, h->device, spec, S, rates, v.pcm, v.plane, v.C, v.d_frames, v.si, f_max, f_max * S, h->py.rows.p, nullptr,
                           h->py.refused.p, hs, err);
      },
      S, in_rates, out_rate, rates, rows, rows_capacity, seg_rows, refused_out, status, err);
}

// ---- frame descriptors (vsyn_fdesc.h) ----

uint64_t vsyn_fdesc_num_frames(const vsyn_fdesc_spec* spec, uint64_t frames) {
  if (fdesc_check(spec, 0, nullptr, nullptr) != VSYN_OK) return 0;
  return spec_num_frames(spec->n_fft, spec->hop_length, fdesc_center(spec), frames);
}

int vsyn_fdesc_device(vsyn_handle* h, const vsyn_fdesc_spec* spec, uint32_t S, const uint32_t* sample_rates, const float* d_pcm,
                      uint64_t plane_stride, uint32_t channels, const uint32_t* d_frames, float* d_rows, uint64_t* d_seg_row_off,
                      uint32_t* d_refused, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  int rc = fdesc_check(spec, S, sample_rates, err);
  if (rc) return rc;
  if (channels == 0 || channels > 255) return fail(err, VSYN_ERR_INVALID, "channels %u outside [1, 255]", channels);
  if (S == 0) return VSYN_OK;
  if (!d_pcm || !d_frames || !d_rows || plane_stride == 0) return fail(err, VSYN_ERR_INVALID, "NULL pointer or zero stride");
  const uint64_t f_max = spec_num_frames(spec->n_fft, spec->hop_length, fdesc_center(spec), plane_stride);
  std::lock_guard<std::mutex> lk(h->mu);
  return fdesc_launch(h->fd, h->device, spec, S, sample_rates, d_pcm, plane_stride, channels, d_frames, nullptr, f_max, d_rows, d_seg_row_off,
                      d_refused, (hipStream_t)hip_stream, err);
}

int vsyn_pcm_fdesc_host(vsyn_handle* h, const vsyn_fdesc_spec* spec, uint32_t S, const uint32_t* in_rates, uint32_t out_rate, float* rows,
                        uint64_t rows_capacity, uint64_t* seg_rows, uint32_t* refused_out, vsyn_status* status, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (int rc = fdesc_check(spec, S, in_rates, err)) return rc;  // (first: an invalid spec writes nothing, the status included)
  status_reset(status);
  if (int rc = chain_check(nullptr, nullptr, S, in_rates, out_rate, err)) return rc;
  const std::vector<uint32_t> fd_rates = stage_rates(S, in_rates, out_rate);
  const uint32_t* rates = out_rate ? fd_rates.data() : in_rates;
  return framed_rows_host(
      h, spec->n_fft, spec->hop_length, fdesc_center(spec), FDESC_COLS, h->fd.rows, h->fd.refused,
      [&](const PcmView& v, uint64_t f_max, hipStream_t hs) {
        return fdesc_launch(h->fd, h->device, spec, S, rates, v.pcm, v.plane, v.C, v.d_frames, v.si, f_max, h->fd.rows.p, nullptr, h->fd.refused.p, hs, err);
      },
      S, in_rates, out_rate, rates, rows, rows_capacity, seg_rows, refused_out, status, err);
}

// ---- constant-Q (vsyn_cqt.h) ----

uint32_t vsyn_cqt_dim(const vsyn_cqt_spec* spec) { return cqt_check(spec, 0, nullptr, nullptr) == VSYN_OK ? cqt_dim(spec) : 0u; }

uint64_t vsyn_cqt_num_frames(const vsyn_cqt_spec* spec, uint64_t frames) {
  if (cqt_check(spec, 0, nullptr, nullptr) != VSYN_OK) return 0;
  return spec_num_frames(0u, spec->hop_length, true, frames);
}

int vsyn_cqt_lengths(uint32_t sample_rate, const vsyn_cqt_spec* spec, double* N, uint32_t* L) {
  if (!sample_rate || cqt_check(spec, 0, nullptr, nullptr) != VSYN_OK) return VSYN_ERR_INVALID;
  const CqtLengths len = cqt_lengths(spec, sample_rate);
  for (uint32_t k = 0; k < spec->n_bins; ++k) {
    if (N) N[k] = len.N[k];
    if (L) L[k] = len.L[k];
  }
  return len.refused ? VSYN_CQT_RATE_REFUSED : cqt_check_caps(len, sample_rate, nullptr);
}

int vsyn_cqt_basis(uint32_t sample_rate, const vsyn_cqt_spec* spec, uint32_t k, float* re_im) {
  if (!sample_rate || !re_im || cqt_check(spec, 0, nullptr, nullptr) != VSYN_OK || k >= spec->n_bins) return VSYN_ERR_INVALID;
  const CqtLengths len = cqt_lengths(spec, sample_rate);
  if (len.refused) return VSYN_CQT_RATE_REFUSED;
  if (int rc = cqt_check_caps(len, sample_rate, nullptr)) return rc;
  cqt_wavelet(spec, sample_rate, len, k, re_im);
  return VSYN_OK;
}

int vsyn_cq_to_chroma(const vsyn_cqt_spec* spec, float* out) {
  if (!out || cqt_check(spec, 0, nullptr, nullptr) != VSYN_OK || !cqt_chroma_out(spec)) return VSYN_ERR_INVALID;
  std::vector<uint32_t> cls(spec->n_bins);
  cqt_classes(spec, cls.data());
  for (uint32_t c = 0; c < spec->n_chroma; ++c)
    for (uint32_t k = 0; k < spec->n_bins; ++k) out[(size_t)c * spec->n_bins + k] = cls[k] == c ? 1.f : 0.f;
  return VSYN_OK;
}

int vsyn_cqt_tile(const vsyn_cqt_spec* spec, uint32_t sample_rate, uint32_t out[3]) {
  (void)sample_rate;
  if (!out || cqt_check(spec, 0, nullptr, nullptr) != VSYN_OK) return VSYN_ERR_INVALID;
  out[0] = CQT_FT;
  out[1] = VSYN_CQT_CHUNK;
  out[2] = CQT_BPW;
  return VSYN_OK;
}

int vsyn_cqt_device(vsyn_handle* h, const vsyn_cqt_spec* spec, uint32_t S, const uint32_t* sample_rates, const float* d_pcm, uint64_t plane_stride,
                    uint32_t channels, const uint32_t* d_frames, float* d_rows, uint64_t* d_seg_row_off, uint32_t* d_refused, void* hip_stream,
                    const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  int rc = cqt_check(spec, S, sample_rates, err);
  if (rc) return rc;
  if (channels == 0 || channels > 255) return fail(err, VSYN_ERR_INVALID, "channels %u outside [1, 255]", channels);
  if (S == 0) return VSYN_OK;
  if (!d_pcm || !d_frames || !d_rows || plane_stride == 0) return fail(err, VSYN_ERR_INVALID, "NULL pointer or zero stride");
  const uint64_t f_max = spec_num_frames(0u, spec->hop_length, true, plane_stride);
  std::lock_guard<std::mutex> lk(h->mu);
  return cqt_launch(h->cq, h->device, spec, S, sample_rates, d_pcm, plane_stride, channels, d_frames, nullptr, f_max, d_rows, d_seg_row_off,
                    d_refused, (hipStream_t)hip_stream, err);
}

int vsyn_pcm_cqt_host(vsyn_handle* h, const vsyn_cqt_spec* spec, uint32_t S, const uint32_t* in_rates, uint32_t out_rate, float* rows,
                      uint64_t rows_capacity, uint64_t* seg_rows, uint32_t* refused_out, vsyn_status* status, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (int rc = cqt_check(spec, S, in_rates, err)) return rc;  // (first: an invalid spec writes nothing, the status included)
  status_reset(status);
  if (int rc = chain_check(nullptr, nullptr, S, in_rates, out_rate, err)) return rc;
  const std::vector<uint32_t> cq_rates = stage_rates(S, in_rates, out_rate);
  const uint32_t* rates = out_rate ? cq_rates.data() : in_rates;
  return framed_rows_host(
      h, 0u, spec->hop_length, true, cqt_dim(spec), h->cq.rows, h->cq.refused,
      [&](const PcmView& v, uint64_t f_max, hipStream_t hs) {
        return cqt_launch(h->cq, h->device, spec, S, rates, v.pcm, v.plane, v.C, v.d_frames, v.si, f_max, h->cq.rows.p, nullptr, h->cq.refused.p, hs, err);
      },
      S, in_rates, out_rate, rates, rows, rows_capacity, seg_rows, refused_out, status, err);
}

// vsyn_pcm_cqt_host with each segment's tuning estimated first: a magnitude STFT of n_fft 2048, hop 512, Hann, centred (librosa.cqt's
// call of estimate_tuning) on the mono signal the transform sees, the estimates read back, then the transform on wavelets per
// distinct (rate, tuning) pair.
int vsyn_pcm_cqt_est_host(vsyn_handle* h, const vsyn_cqt_spec* spec, const vsyn_tuning_spec* estimate, uint32_t S, const uint32_t* in_rates,
                          uint32_t out_rate, float* rows, uint64_t rows_capacity, uint64_t* seg_rows, uint32_t* refused_out, double* tuning_out,
                          vsyn_status* status, const char** err) {
  if (!estimate) return vsyn_pcm_cqt_host(h, spec, S, in_rates, out_rate, rows, rows_capacity, seg_rows, refused_out, status, err);
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (int rc = cqt_check(spec, S, in_rates, err)) return rc;  // (first: an invalid spec writes nothing, the status included)
  const vsyn_spectral_spec lin = {VSYN_SPEC_LIN_POWER, VSYN_SPEC_CENTER, 2048u, 512u, 2048u, 0u, 0u, 1u, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (int rc = tuning_check(&lin, estimate, 0, nullptr, err)) return rc;
  if (estimate->bins_per_octave != spec->bins_per_octave)
    return fail(err, VSYN_ERR_INVALID, "the estimate's bins_per_octave %u is not the transform's %u: the tuning would be in another unit",
                estimate->bins_per_octave, spec->bins_per_octave);
  if (S && rows && !tuning_out) return fail(err, VSYN_ERR_INVALID, "tuning_out is NULL");
  for (uint32_t g = 0; g < S && tuning_out; ++g) tuning_out[g] = 0.0;
  status_reset(status);
  if (int rc = chain_check(nullptr, nullptr, S, in_rates, out_rate, err)) return rc;
  const std::vector<uint32_t> cq_rates = stage_rates(S, in_rates, out_rate);
  const uint32_t* rates = out_rate ? cq_rates.data() : in_rates;
  return framed_rows_host(
      h, 0u, spec->hop_length, true, cqt_dim(spec), h->cq.rows, h->cq.refused,
      [&](const PcmView& v, uint64_t f_max, hipStream_t hs) {
        HIPCHK(h->tu.tuning.ensure(S));
        HIPCHK(h->tu.counts.ensure(2ull * S));
        if (int rc = pip_launch(h->sp, h->tu, h->device, &lin, estimate, S, rates, v.pcm, v.plane, v.C, v.d_frames, v.si,
                                spec_num_frames(lin.n_fft, lin.hop_length, true, v.plane), nullptr, nullptr, 0, nullptr, h->tu.tuning.p, h->tu.counts.p,
                                hs, err))
          return rc;
        HIPCHK(hipMemcpyAsync(tuning_out, h->tu.tuning.p, sizeof(double) * S, hipMemcpyDeviceToHost, hs));
        HIPCHK(hipStreamSynchronize(hs));  // the one extra wait of the form: the wavelets need the numbers
        return cqt_launch(h->cq, h->device, spec, S, rates, v.pcm, v.plane, v.C, v.d_frames, v.si, f_max, h->cq.rows.p, nullptr, h->cq.refused.p, hs, err,
                          tuning_out);
      },
      S, in_rates, out_rate, rates, rows, rows_capacity, seg_rows, refused_out, status, err);
}

// ---- tuning estimation (vsyn_tuning.h) ----

int vsyn_tuning_check(const vsyn_spectral_spec* spec, const vsyn_tuning_spec* tun, const char** err) { return tuning_check(spec, tun, 0, nullptr, err); }

int vsyn_piptrack_bins(uint32_t sample_rate, const vsyn_spectral_spec* spec, const vsyn_tuning_spec* tun, uint32_t out[2]) {
  if (!out || !sample_rate || tuning_check(spec, tun, 0, nullptr, nullptr) != VSYN_OK) return VSYN_ERR_INVALID;
  pip_bins(sample_rate, spec->n_fft, tun, out);
  return VSYN_OK;
}

int vsyn_pitch_tuning(const float* freqs, const float* mags, uint64_t n, double resolution, uint32_t bins_per_octave, double* tuning,
                      uint64_t counts[2]) {
  if ((n && !freqs) || !tuning || !counts) return VSYN_ERR_INVALID;
  if (!std::isfinite(resolution) || !(resolution > 0.0 && resolution < 1.0) || ceil(1.0 / resolution) > (double)TUNE_MAX_BINS) return VSYN_ERR_INVALID;
  if (bins_per_octave < 1 || bins_per_octave > 256) return VSYN_ERR_INVALID;
  return tune_host(freqs, mags, n, resolution, bins_per_octave, tuning, counts);
}

uint32_t vsyn_piptrack_tile(const vsyn_spectral_spec* spec) {
  if (spec_check(spec, 0, nullptr, nullptr) != VSYN_OK || spec->kind != VSYN_SPEC_LIN_POWER) return 0;
  return pip_tile(spec);
}

// what the two device entries share: the checks, then pip_launch with the outputs of one of them
static int tuning_device_call(vsyn_handle* h, const vsyn_spectral_spec* spec, const vsyn_tuning_spec* tun, uint32_t S, const uint32_t* sample_rates,
                              const float* d_pcm, uint64_t plane_stride, uint32_t channels, const uint32_t* d_frames, float* d_pitches, float* d_mags,
                              uint64_t* d_seg_row_off, double* d_tuning, uint64_t* d_counts, void* hip_stream, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (int rc = tuning_check(spec, tun, S, sample_rates, err)) return rc;
  if (S == 0) return VSYN_OK;
  if (!d_pcm || !d_frames || plane_stride == 0 || channels == 0 || channels > 255 || (!d_tuning && (!d_pitches || !d_mags)) || (d_tuning && !d_counts))
    return fail(err, VSYN_ERR_INVALID, "NULL pointer, zero stride or channels outside [1, 255]");
  const uint64_t f_max = spec_num_frames(spec->n_fft, spec->hop_length, (spec->options & VSYN_SPEC_CENTER) != 0, plane_stride);
  std::lock_guard<std::mutex> lk(h->mu);
  return pip_launch(h->sp, h->tu, h->device, spec, tun, S, sample_rates, d_pcm, plane_stride, channels, d_frames, nullptr, f_max, d_pitches, d_mags,
                    spec->n_fft / 2u + 1u, d_seg_row_off, d_tuning, d_counts, (hipStream_t)hip_stream, err);
}

int vsyn_piptrack_device(vsyn_handle* h, const vsyn_spectral_spec* spec, const vsyn_tuning_spec* tun, uint32_t S, const uint32_t* sample_rates,
                         const float* d_pcm, uint64_t plane_stride, uint32_t channels, const uint32_t* d_frames, float* d_pitches, float* d_mags,
                         uint64_t* d_seg_row_off, void* hip_stream, const char** err) {
  return tuning_device_call(h, spec, tun, S, sample_rates, d_pcm, plane_stride, channels, d_frames, d_pitches, d_mags, d_seg_row_off, nullptr, nullptr,
                            hip_stream, err);
}

int vsyn_tuning_device(vsyn_handle* h, const vsyn_spectral_spec* spec, const vsyn_tuning_spec* tun, uint32_t S, const uint32_t* sample_rates,
                       const float* d_pcm, uint64_t plane_stride, uint32_t channels, const uint32_t* d_frames, double* d_tuning, uint64_t* d_counts,
                       void* hip_stream, const char** err) {
  if (h && !d_tuning && S) return fail(err, VSYN_ERR_INVALID, "d_tuning is NULL");
  return tuning_device_call(h, spec, tun, S, sample_rates, d_pcm, plane_stride, channels, d_frames, nullptr, nullptr, nullptr, d_tuning, d_counts,
                            hip_stream, err);
}

int vsyn_pcm_tuning_host(vsyn_handle* h, const vsyn_spectral_spec* spec, const vsyn_tuning_spec* tun, uint32_t S, const uint32_t* in_rates,
                         uint32_t out_rate, uint32_t what, double* tuning, uint64_t* counts, float* rows, uint64_t rows_capacity,
                         uint64_t* seg_rows, vsyn_status* status, const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (int rc = tuning_check(spec, tun, S, in_rates, err)) return rc;  // (first: an invalid spec writes nothing, the status included)
  if (what > VSYN_TUNING_ROWS) return fail(err, VSYN_ERR_INVALID, "unknown tuning output selector %u", what);
  if (S && !seg_rows) return fail(err, VSYN_ERR_INVALID, "seg_rows is NULL");
  status_reset(status);
  if (int rc = chain_check(nullptr, nullptr, S, in_rates, out_rate, err)) return rc;
  const std::vector<uint32_t> rates = stage_rates(S, in_rates, out_rate);
  const bool dense = what == VSYN_TUNING_ROWS;
  // the lock covers the whole call: the resample workspace and the stage's are the handle's, and the PCM must stay that of the last submit
  std::lock_guard<std::mutex> lk(h->mu);
  std::vector<uint64_t> T(S);
  uint64_t total, f_max, t_max;
  if (int rc = last_submit_frames(h, S, in_rates, out_rate, T.data(), &t_max, err)) return rc;
  t_max = std::max<uint64_t>(t_max, 1);
  count_rows(spec->n_fft, spec->hop_length, (spec->options & VSYN_SPEC_CENTER) != 0, S, rates.data(), T.data(), 0, seg_rows, &total, &f_max);
  if (S == 0 || (dense ? !rows : !tuning)) return VSYN_OK;  // the size query
  if (dense && total > rows_capacity) return fail(err, VSYN_ERR_INVALID, "rows buffer too small: %llu rows needed", (unsigned long long)total);
  if (out_rate && t_max > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "resampled segment too long");
  hipStream_t hs = h->host_stream;
  PcmView v = last_submit_view(h);
  if (out_rate)
    if (int rc = step_resample(h, S, in_rates, out_rate, t_max, false, &v, err)) return rc;
  const uint64_t nb = spec->n_fft / 2u + 1u, nv = total * 2u * nb;  // a row: its NB pitches, then its NB magnitudes
  if (dense) HIPCHK(h->tu_rows.ensure(nv + 1));
  if (tuning) {
    HIPCHK(h->tu.tuning.ensure(S));
    HIPCHK(h->tu.counts.ensure(2ull * S));
  }
  if (int rc = pip_launch(h->sp, h->tu, h->device, spec, tun, S, rates.data(), v.pcm, v.plane, v.C, v.d_frames, v.si, f_max,
                          dense ? h->tu_rows.p : nullptr, dense ? h->tu_rows.p + nb : nullptr, 2u * nb, nullptr, tuning ? h->tu.tuning.p : nullptr,
                          tuning ? h->tu.counts.p : nullptr, hs, err))
    return rc;
  if (dense && nv) HIPCHK(hipMemcpyAsync(rows, h->tu_rows.p, sizeof(float) * nv, hipMemcpyDeviceToHost, hs));
  if (tuning) {
    HIPCHK(hipMemcpyAsync(tuning, h->tu.tuning.p, sizeof(double) * S, hipMemcpyDeviceToHost, hs));
    if (counts) HIPCHK(hipMemcpyAsync(counts, h->tu.counts.p, sizeof(uint64_t) * 2u * S, hipMemcpyDeviceToHost, hs));
  }
  return sync_status_into(h, status, err);
}

// ---- loudness (vsyn_loudness.h) ----

uint64_t vsyn_loudness_num_blocks(uint32_t sample_rate, uint64_t frames) { return loud_num_blocks(sample_rate, frames); }

int vsyn_loudness_coefficients(uint32_t sample_rate, double* out) {
  if (!out || sample_rate < LOUD_MIN_RATE) return VSYN_ERR_INVALID;
  loud_coefficients(sample_rate, out);
  return VSYN_OK;
}

int vsyn_loudness_powers(uint32_t sample_rate, double* out) {
  if (!out || sample_rate < LOUD_MIN_RATE) return VSYN_ERR_INVALID;
  double k[10], M[LOUD_LEVELS + 1u][16];
  loud_coefficients(sample_rate, k);
  loud_powers(k, M);
  memcpy(out, M, sizeof(M));
  return VSYN_OK;
}

int vsyn_loudness_device(vsyn_handle* h, const vsyn_loudness_spec* spec, uint32_t S, const uint32_t* sample_rates, const uint64_t* frames,
                         const float* d_pcm, uint64_t plane_stride, uint32_t channels, vsyn_loudness_record* d_records, double* d_z,
                         double* d_weighted, uint64_t weighted_plane_stride, float* d_scaled, uint64_t scaled_plane_stride, void* hip_stream,
                         const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (int rc = loud_check(spec, err)) return rc;
  if (d_scaled && !(spec->options & VSYN_LOUD_NORMALIZE)) return fail(err, VSYN_ERR_INVALID, "a scaled plane needs VSYN_LOUD_NORMALIZE and a target");
  if (S == 0) return VSYN_OK;
  if (!sample_rates || !frames || !d_pcm || !d_records || plane_stride == 0 || channels == 0 || channels > 255)
    return fail(err, VSYN_ERR_INVALID, "NULL pointer, zero stride or channels outside [1, 255]");
  if ((d_weighted && weighted_plane_stride == 0) || (d_scaled && scaled_plane_stride == 0))
    return fail(err, VSYN_ERR_INVALID, "an output plane has a zero stride");
  std::lock_guard<std::mutex> lk(h->mu);
  return loud_launch(h->ld, h->device, spec, S, sample_rates, frames, d_pcm, plane_stride, channels, d_records, d_z, d_weighted,
                     weighted_plane_stride, d_scaled, scaled_plane_stride, (hipStream_t)hip_stream, err);
}

int vsyn_pcm_loudness_host(vsyn_handle* h, const vsyn_loudness_spec* spec, uint32_t S, const uint32_t* in_rates, uint32_t out_rate,
                           vsyn_loudness_record* records, double* z, uint64_t z_capacity, uint64_t* seg_blocks, vsyn_status* status,
                           const char** err) {
  if (!h) return fail(err, VSYN_ERR_INVALID, "handle is NULL");
  if (int rc = loud_check(spec, err)) return rc;  // (first: an invalid spec writes nothing, the status included)
  if (S && !in_rates) return fail(err, VSYN_ERR_INVALID, "in_rates is NULL");
  if (S && !records && !seg_blocks) return fail(err, VSYN_ERR_INVALID, "records and seg_blocks are both NULL");
  status_reset(status);
  if (int rc = chain_check(nullptr, nullptr, S, in_rates, out_rate, err)) return rc;
  const std::vector<uint32_t> rates = stage_rates(S, in_rates, out_rate);
  // the lock covers the whole call: the resample workspace and the stage's are the handle's, and the PCM must stay that of the last submit
  std::lock_guard<std::mutex> lk(h->mu);
  std::vector<uint64_t> T(S);
  uint64_t t_max, total = 0;
  if (int rc = last_submit_frames(h, S, in_rates, out_rate, T.data(), &t_max, err)) return rc;
  for (uint32_t g = 0; g < S; ++g) {
    const uint64_t nb = loud_num_blocks(rates[g], T[g]);
    if (seg_blocks) seg_blocks[g] = nb;
    total += nb;
  }
  if (S == 0 || !records) return VSYN_OK;
  if (z && total > z_capacity) return fail(err, VSYN_ERR_INVALID, "z buffer too small: %llu blocks", (unsigned long long)total);
  t_max = std::max<uint64_t>(t_max, 1);
  if (t_max > 0xFFFFFFFFull) return fail(err, VSYN_ERR_INVALID, "segment too long");
  hipStream_t hs = h->host_stream;
  PcmView v = last_submit_view(h);
  if (out_rate)
    if (int rc = step_resample(h, S, in_rates, out_rate, t_max, false, &v, err)) return rc;
  HIPCHK(h->ld.rec.ensure(S));
  if (z) HIPCHK(h->ld.z.ensure(total + 1));
  if (int rc = loud_launch(h->ld, h->device, spec, S, rates.data(), T.data(), v.pcm, v.plane, v.C, h->ld.rec.p, z ? h->ld.z.p : nullptr, nullptr, 0,
                           nullptr, 0, hs, err))
    return rc;
  HIPCHK(hipMemcpyAsync(records, h->ld.rec.p, sizeof(vsyn_loudness_record) * S, hipMemcpyDeviceToHost, hs));
  if (z && total) HIPCHK(hipMemcpyAsync(z, h->ld.z.p, sizeof(double) * total, hipMemcpyDeviceToHost, hs));
  return sync_status_into(h, status, err);
}

}  // extern "C"
