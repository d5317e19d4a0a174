// vsyn_staged.h — the layout and floor-unwrap pre-kernels (the chained preparation; vsyn_prep.h does both in one kernel; the floor-1
// arithmetic is vsyn_floor1.h's) and the STAGED synthesis kernels:
// any blocksize 64..8192, any channel count / coupling list, every intermediate materialised in HBM so it
// can be handed out as a debug tap (the reference's push_data_* hooks).  Correctness-first; the fused
// kernels in vsyn_fused.h are the speed path.  Compiled with -ffp-contract=off: every a*b+c below is two
// roundings unless written as __builtin_fmaf.
#pragma once
#include <hip/hip_runtime.h>

#include "vsyn_device.h"
#include "vsyn_floor1.h"

// ------------------------------------------------------------------------------------------------
// K0  layout: one workgroup per segment.  Restates the integer bookkeeping of
// VorbisStreamDecodeState::advancePcmOffsetBeginAudioPacket / forwardReadyPcm (hpp:1019-1067) as a scan:
//   natural frames L_q = n_{q-1}/4 + n_q/4 (0 for a stream's first packet, hpp:1021-1027)
//   abs_after_q = max(granule_q, abs_before_q) if granule_q >= 0 (hpp:1028-1044,1056-1057) else abs_before_q + L_q
// plus the residue offset prefix sum and the nonzero propagate (hpp:1174-1180).
// A granule at or ahead of the position is where the reference puts it. One BEHIND the position is refused (VSYN_ST_GRANULE, hpp:1029);
// the max keeps it from moving the position back, so that the packets behind a refused one, which the device still lays out, land
// behind the PCM in front of it instead of over it.
// One packet's step is the map x -> max(lo, x + val) (set: a granule, lo = granule, val = 0) or x -> x + val (no granule, val = L_q);
// such maps compose into the same form: max(lo2, max(lo1, x + v1) + v2) = max(max(lo2, lo1 + v2), x + v1 + v2).
// ------------------------------------------------------------------------------------------------
struct AbsScan {
  int64_t val;
  int set;
  int64_t lo;
};
__device__ __forceinline__ AbsScan abs_combine(AbsScan a, AbsScan b) {  // b after a
  AbsScan r;
  r.val = a.val + b.val;
  r.set = a.set | b.set;
  r.lo = b.set ? (a.set ? max(b.lo, a.lo + b.val) : b.lo) : a.lo + b.val;
  return r;
}
// the step of one packet: its page granule (or -1) and its natural frames L
__device__ __forceinline__ AbsScan abs_element(int64_t granule, int64_t L) {
  AbsScan e;
  e.set = granule >= 0;
  e.val = e.set ? 0 : L;
  e.lo = e.set ? granule : 0;
  return e;
}
// the position behind the packets of e, starting at x
__device__ __forceinline__ int64_t abs_eval(const AbsScan& e, int64_t x) { return e.set ? max(e.lo, x + e.val) : x + e.val; }
__device__ __forceinline__ AbsScan abs_shfl_up(const AbsScan& e, int d) {
  AbsScan o;
  o.val = __shfl_up(e.val, d);
  o.set = __shfl_up(e.set, d);
  o.lo = __shfl_up(e.lo, d);
  return o;
}

// Shared by the layout kernel (which builds the staged list) and the fused kernel (which skips non-fast runs):
// both must take the same decision.
// Which kernel takes a run of packets [qa, qb) of a segment: 1 = fused long-run kernel (every packet it touches, its
// one-packet halo included, is a long block and there is no carry-in from an earlier submit), 2 = fused mixed-block
// kernel (any mix of valid short/long blocks, carry-in allowed), 0 = staged work list. Shared by the layout kernel
// (which builds the list) and the fused kernels (which skip what is not theirs): all three must agree.
__device__ __forceinline__ uint32_t run_class(const ConstHeader* H, const vsyn_packet* __restrict__ spk, uint32_t qa, uint32_t qb,
                                              uint32_t carry_n, uint32_t ok_mask) {
  if (!ok_mask) return 0;
  bool all_long = !(qa == 0 && carry_n), all_valid = true;
  for (uint32_t q = qa ? qa - 1 : 0; q < qb; ++q) {
    const uint32_t m = spk[q].mode;
    const bool valid = m < H->num_modes;
    all_valid = all_valid && valid;
    all_long = all_long && valid && H->mode_blockflag[m];
  }
  if (all_long && (ok_mask & 1u)) return 1;
  if (ok_mask & 2u) return 2;  // the mixed kernel also steps over packets with an invalid mode (PktInfo.bad)
  (void)all_valid;
  return 0;
}

// The same decision from a bitmap in LDS (bit = a valid long block): bits [first, end) are the run's packets, bit first - 1 its
// one-packet halo (for the segment's first run there is none: the carry-in decides). Classifying a run is then a few LDS words
// instead of a serial walk over R+1 descriptors in global memory (which was most of the layout kernel's time, and its
// workgroups sit on wave slots the synthesis kernel of the previous submit is waiting for).
__device__ __forceinline__ uint32_t run_class_bits(const uint32_t* bits, uint32_t first, uint32_t end, uint32_t carry_n, uint32_t ok_mask, bool seg_start) {
  if (!ok_mask) return 0;
  bool all_long = !(seg_start && carry_n);
  const uint32_t lo = seg_start ? first : first - 1u;  // one-packet halo
  for (uint32_t w = lo >> 5; all_long && w <= ((end - 1u) >> 5); ++w) {
    uint32_t need = 0xFFFFFFFFu;
    if (w == (lo >> 5)) need &= 0xFFFFFFFFu << (lo & 31u);
    if (w == ((end - 1u) >> 5)) need &= 0xFFFFFFFFu >> (31u - ((end - 1u) & 31u));
    all_long = (bits[w] & need) == need;
  }
  if (all_long && (ok_mask & 1u)) return 1;
  if (ok_mask & 2u) return 2;
  return 0;
}

// One packet of the scan, shared by the layout kernel and the in-wave preparation of the fused kernels (vsyn_prep.h): everything
// PktInfo holds, from the packet's descriptor, the block size in front of it and the scan's running values (hpp:1019-1067, 1174-1180).
struct PktStep {
  PktInfo pi;
  int64_t abs_after;
  uint32_t raise;  // VSYN_ST_* to raise for this packet (0: none)
};
// (own / used: floor_output_used before and after the nonzero propagate of hpp:1174-1180, see coupling_propagate)
// prev_tail: the block in front is long and its next_long flag is set (prev_tail_of). A smaller block behind it is the one window-flag
// disagreement whose reference result the two-term overlap cannot give (VSYN_ST_WINDOW_FLAGS): raised and skipped like a granule error.
// Like VSYN_ST_BAD_MODE, the later checks of the packet (and the later packets of the segment) still run, so the flag word can hold
// more bits than the oracle's, which stops at the first; the status code and first_bad_packet are the same.
__device__ __forceinline__ PktStep pkt_step_core(const vsyn_packet& k, bool mode_ok, uint32_t lng, uint32_t mapping, uint32_t n, uint32_t prev_n,
                                                 uint32_t prev_tail, int64_t abs_before, int64_t abs0, uint64_t res_off, uint64_t plane_stride,
                                                 uint32_t own, uint32_t used) {
  PktStep r;
  PktInfo pi = {};
  r.raise = mode_ok ? 0u : (uint32_t)VSYN_ST_BAD_MODE;
  const uint32_t L = prev_n ? prev_n / 4 + n / 4 : 0;
  int64_t abs_after = abs_before + L;
  uint32_t emit = L;
  bool bad = !mode_ok;
  if (mode_ok && prev_tail && n < prev_n) {
    r.raise |= VSYN_ST_WINDOW_FLAGS;
    bad = true;
  }
  if (k.granule >= 0) {
    // hpp:1029 (position already past the page granule) and hpp:1041 (packets cannot reach it)
    if (k.granule < abs_before || k.granule > abs_before + (int64_t)L) {
      r.raise |= VSYN_ST_GRANULE;
      bad = true;
      emit = 0;
    } else {
      emit = (uint32_t)(k.granule - abs_before);
    }
    abs_after = k.granule < abs_before ? abs_before : k.granule;  // (a granule behind the position does not move it back: AbsScan)
  }
  const int64_t rel = abs_before - abs0;
  if (rel < 0 || (uint64_t)rel + emit > plane_stride) {
    if (emit) r.raise |= VSYN_ST_PLANE_OVERFLOW;
    if (emit) bad = true;
    emit = 0;
  }
  if (r.raise & VSYN_ST_WINDOW_FLAGS) emit = 0;
  pi.res_off = res_off;
  pi.out_pos = rel < 0 ? 0u : (uint32_t)rel;
  pi.emit = emit;
  pi.n = (uint16_t)n;
  pi.lng = (uint8_t)lng;
  pi.widx = lng ? (uint8_t)((k.prev_long ? 1 : 0) | (k.next_long ? 2 : 0)) : 0;
  pi.mapping = (uint8_t)mapping;
  pi.bad = bad ? 1 : 0;
  pi.own = own;
  pi.used = used;
  r.pi = pi;
  r.abs_after = abs_after;
  return r;
}
// the prev_tail of the block behind a packet: the packet is a valid long block whose next_long byte is non-zero (any non-zero byte is
// true, as in the reference's getWindow(bool, bool))
__device__ __forceinline__ uint32_t prev_tail_of(bool is_long, uint8_t next_long) { return (is_long && next_long) ? 1u : 0u; }
__device__ __forceinline__ PktStep pkt_step(const MapConst* __restrict__ maps, const vsyn_packet& k, bool mode_ok, uint32_t lng, uint32_t mapping,
                                            uint32_t n, uint32_t prev_n, uint32_t prev_tail, int64_t abs_before, int64_t abs0, uint64_t res_off,
                                            uint64_t plane_stride, uint32_t C) {
  const uint32_t chan_mask = C >= 32 ? 0xFFFFFFFFu : ((1u << C) - 1u);
  uint32_t own = k.floor_used & chan_mask, used = own;
  const MapConst* mc = maps + mapping;
  for (uint32_t i = 0; i < mc->ncoup; ++i) {  // hpp:1175-1180
    uint32_t m = mc->coup[2 * i], a = mc->coup[2 * i + 1];
    if (((used >> m) | (used >> a)) & 1u) used |= (1u << m) | (1u << a);
  }
  return pkt_step_core(k, mode_ok, lng, mapping, n, prev_n, prev_tail, abs_before, abs0, res_off, plane_stride, own, used);
}

// A segment is scanned in CHUNKS of chunk_packets packets (a multiple of the run length R, so that a run never straddles two
// chunks), one workgroup per (segment, chunk). With one chunk per segment — every segment of the batch is at most
// LAYOUT_CHUNK_PACKETS long: the usual case — nothing below about look-back runs. Longer segments (ONE long stream is the second
// partitioning of SURVEY 8e) chain their chunks with a decoupled look-back: a chunk publishes the aggregate of its own packets, walks
// back over its predecessors' records until it meets one that already holds an inclusive prefix, and publishes its own inclusive
// prefix. The serial scan of one workgroup per segment made 1 x 65 536 packets run at half the rate of 64 x 1024.
// Block size LAYOUT_THREADS, or one wavefront per chunk (LAYOUT_THREADS_SHORT) when no chunk of the batch has more than
// LAYOUT_SHORT_PACKETS packets: a batch of thousands of short streams would otherwise put four nearly idle waves per segment
// on the chip, next to the synthesis kernel. Dynamic LDS: layout_lds_bytes().
#define LAYOUT_THREADS 256
#define LAYOUT_THREADS_SHORT 64
#define LAYOUT_SHORT_PACKETS 256u
#define LAYOUT_CHUNK_PACKETS 4096u
struct LayoutChunk {          // look-back record of one (segment, chunk); 64 bytes
  uint32_t flag;              // (epoch & 2^30-1) * 4 + 1: aggregate valid, + 2: inclusive prefix valid, + 3: chain lost (no clearing between submits)
  uint32_t pad;
  int64_t agg_val, inc_val;   // AbsScan of the chunk's own packets / of everything up to its end
  uint64_t agg_res, inc_res;  // residue floats likewise
  uint32_t agg_set, inc_set;
  int64_t agg_lo, inc_lo;
};
static inline __host__ __device__ size_t layout_lds_bytes(uint32_t threads, uint32_t chunk_packets) {
  return (size_t)threads * (sizeof(AbsScan) + sizeof(uint64_t)) + (size_t)((chunk_packets + 1u + 31u) / 32u) * 4u + 16u;
}
__global__ void __launch_bounds__(LAYOUT_THREADS)
vsyn_layout_kernel(const uint8_t* __restrict__ cb, uint32_t P, const vsyn_packet* __restrict__ pk, uint32_t S,
                   const vsyn_segment* __restrict__ segs, uint64_t plane_stride, PktInfo* __restrict__ info,
                   SegInfo* __restrict__ sinfo, StreamState* __restrict__ state, uint32_t* __restrict__ emit_len,
                   DevStatus* __restrict__ status, uint32_t R, uint32_t fused_ok, uint32_t* __restrict__ staged_list,
                   uint32_t* __restrict__ staged_count, uint32_t* __restrict__ next_count, uint32_t* __restrict__ seg_of_pkt,
                   uint8_t* __restrict__ run_cls, uint32_t runs_per_seg, uint32_t chunk_packets, uint32_t chunks_per_seg,
                   LayoutChunk* __restrict__ chunks, uint32_t epoch) {
  const ConstHeader* H = hdr_of(cb);
  const uint32_t g = blockIdx.x / chunks_per_seg, ch = blockIdx.x % chunks_per_seg, t = threadIdx.x, NT = blockDim.x;
  if (g >= S) return;
  if (blockIdx.x == 0 && t == 0) *next_count = 0;  // the other submit parity's list counter (no memset node needed)
  const vsyn_segment sg = segs[g];
  const bool seg_ok = sg.stream < H->max_streams && (uint64_t)sg.first_packet + sg.num_packets <= P && (sg.residue_off & 3) == 0;
  const uint32_t cs = ch * chunk_packets;  // first packet of this chunk
  const uint32_t runs_per_chunk = chunk_packets / R;
  if (!seg_ok) {
    if (t == 0 && ch == 0) {
      raise_status(status, VSYN_ST_BAD_SEGMENT, sg.first_packet < P ? sg.first_packet : 0);
      sinfo[g] = SegInfo{0, 0, 0, 0};
    }
    for (uint32_t r = ch * runs_per_chunk + t; r < min(runs_per_seg, (ch + 1u) * runs_per_chunk); r += NT) run_cls[(size_t)g * runs_per_seg + r] = 0xFFu;
    // mark every packet we may safely touch as bad so later kernels skip it
    if ((uint64_t)sg.first_packet + sg.num_packets <= P)
      for (uint32_t q = cs + t; q < min(sg.num_packets, cs + chunk_packets); q += NT) {
        PktInfo pi = {};
        pi.bad = 1;
        pi.n = (uint16_t)H->bs[0];
        info[sg.first_packet + q] = pi;
      }
    return;
  }
  const uint32_t C = H->channels, num = sg.num_packets;
  // runs of this chunk that lie beyond the segment's end
  if (cs >= num && !(ch == 0)) {
    for (uint32_t r = ch * runs_per_chunk + t; r < min(runs_per_seg, (ch + 1u) * runs_per_chunk); r += NT) run_cls[(size_t)g * runs_per_seg + r] = 0xFFu;
    return;
  }
  const uint32_t cn = min(num, cs + chunk_packets) - min(num, cs);  // packets of this chunk
  const bool last_chunk = cs + cn >= num;
  uint32_t st_slot;
  const StreamState st0 = state_read(state, sg.stream, epoch, &st_slot);
  const bool reset = (sg.flags & VSYN_SEG_RESET) != 0;
  const uint32_t carry_n = (!reset && st0.has_prev) ? st0.prev_n : 0;
  const int64_t abs0 = reset ? 0 : (int64_t)st0.abs_total_pos;

  extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];  // layout_lds_bytes(): scan arrays [NT], then the bitmap
  AbsScan* s_abs = (AbsScan*)s_dyn;
  uint64_t* s_res = (uint64_t*)(s_dyn + (size_t)NT * sizeof(AbsScan));
  // bit 0: the packet in front of the chunk (the first run's halo), bit 1 + i: packet cs + i — set = a valid long block
  uint32_t* s_longbits = (uint32_t*)(s_dyn + (size_t)NT * (sizeof(AbsScan) + sizeof(uint64_t)));
  for (uint32_t w = t; w < (cn + 1u + 31u) / 32u; w += NT) s_longbits[w] = 0u;
  __shared__ int64_t s_abs_end;
  __shared__ uint32_t s_last_n, s_last_tail;
  __shared__ AbsScan s_chunk_ex;   // exclusive prefix of this chunk (everything before it in the segment)
  __shared__ uint64_t s_chunk_rex;
  __shared__ uint32_t s_chunk_lost;

  const uint32_t per = (cn + NT - 1) / NT;
  const uint32_t qb = min(cn, t * per), qe = min(cn, qb + per);  // this thread's packets, relative to the chunk
  const vsyn_packet* spk = pk + sg.first_packet;                 // (segment-relative indexing: spk[cs + i])

  // mode -> (block flag, mapping) from LDS, and — when a thread has few packets — its descriptors loaded up front in one
  // burst and kept in registers for both passes: the kernel is a chain of small dependent loads otherwise, and while it
  // runs its workgroups hold wave slots of 64 CUs
  __shared__ uint8_t s_bf[VSYN_MAX_TABLES], s_mm[VSYN_MAX_TABLES];
  if (t < VSYN_MAX_TABLES) {
    s_bf[t] = H->mode_blockflag[t];
    s_mm[t] = H->mode_mapping[t];
  }
  constexpr uint32_t KEEP = 8;
  const bool keep = per <= KEEP;  // then pass B reuses what pass A loaded
  vsyn_packet kq[KEEP];
  const uint32_t num_modes = H->num_modes, bs0 = H->bs[0], bs1 = H->bs[1];
  uint32_t carry_prev_mode = 0xFFFFFFFFu;  // mode of the packet before this thread's first one (for the block size in front of it)
  uint8_t carry_prev_next = 0;             // and its next_long byte
  if (cs + qb > 0 && qb < cn) {
    carry_prev_mode = spk[cs + qb - 1].mode;
    carry_prev_next = spk[cs + qb - 1].next_long;
  }
  __syncthreads();
  auto n_of_mode = [&](uint32_t m) -> uint32_t { return (m < num_modes && s_bf[m]) ? bs1 : bs0; };
  if (t == 0 && cs > 0) {  // the halo bit of the chunk's first run
    const uint32_t m = spk[cs - 1].mode;
    if (m < num_modes && s_bf[m]) atomicOr(&s_longbits[0], 1u);
  }
  const uint32_t prev_n0 = cs + qb == 0 ? carry_n : (qb < cn ? n_of_mode(carry_prev_mode) : 0);
  const uint32_t prev_tail0 = cs + qb == 0 ? (carry_n ? st0.prev_tail : 0u)
                                           : (qb < cn ? prev_tail_of(carry_prev_mode < num_modes && s_bf[carry_prev_mode], carry_prev_next) : 0u);

  // pass A: per-thread aggregate
  AbsScan agg = {0, 0};
  uint64_t res = 0;
  {
    uint32_t prev_n = prev_n0;
    auto step_a = [&](const vsyn_packet& k) {
      const uint32_t n = n_of_mode(k.mode);
      agg = abs_combine(agg, abs_element(k.granule, prev_n ? (int64_t)(prev_n / 4 + n / 4) : 0));
      res += (uint64_t)C * (n / 2);
      prev_n = n;
    };
    // KEEP descriptors per burst: one exposed round trip per burst instead of one per packet
    for (uint32_t base = qb; base < qe; base += KEEP) {
#pragma unroll
      for (uint32_t j = 0; j < KEEP; ++j)
        if (base + j < qe) kq[j] = spk[cs + base + j];
#pragma unroll
      for (uint32_t j = 0; j < KEEP; ++j)
        if (base + j < qe) step_a(kq[j]);
    }
  }
  // exclusive scan over the thread aggregates: wave-level shuffles, then the wave totals through LDS
  AbsScan chunk_agg;
  uint64_t chunk_res;
  {
    const uint32_t lane = t & 63u, wv = t >> 6, NW = NT >> 6;
    AbsScan inc = agg;
    uint64_t rinc = res;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const AbsScan o = abs_shfl_up(inc, d);
      const uint64_t ro = __shfl_up(rinc, d);
      if ((int)lane >= d) {
        inc = abs_combine(o, inc);
        rinc += ro;
      }
    }
    if (lane == 63) {
      s_abs[wv] = inc;
      s_res[wv] = rinc;
    }
    __syncthreads();
    AbsScan pre = {0, 0};
    uint64_t rpre = 0;
    for (uint32_t w = 0; w < wv; ++w) {
      pre = abs_combine(pre, s_abs[w]);
      rpre += s_res[w];
    }
    chunk_agg = pre;
    chunk_res = rpre;
    for (uint32_t w = wv; w < NW; ++w) {  // (every thread: the chunk's total)
      chunk_agg = abs_combine(chunk_agg, s_abs[w]);
      chunk_res += s_res[w];
    }
    // exclusive = (prefix of earlier waves) o (inclusive of lane-1)
    AbsScan ex = abs_shfl_up(inc, 1);
    uint64_t rex = __shfl_up(rinc, 1);
    if (lane == 0) {
      ex = AbsScan{0, 0, 0};
      rex = 0;
    }
    ex = abs_combine(pre, ex);
    rex += rpre;
    __syncthreads();
    s_abs[t] = ex;
    s_res[t] = rex;
  }
  // chunk chain (segments longer than one chunk only): decoupled look-back over the predecessors' records
  if (chunks_per_seg > 1) {
    if (t == 0) {
      const uint32_t ep = epoch & 0x3FFFFFFFu;  // the tag shares its word with two state bits
      LayoutChunk* mine = chunks + (size_t)g * chunks_per_seg + ch;
      AbsScan ex = {0, 0};
      uint64_t rex = 0;
      bool lost = false;  // a predecessor's record never arrived within the bound
      if (ch > 0) {
        mine->agg_val = chunk_agg.val;
        mine->agg_set = (uint32_t)chunk_agg.set;
        mine->agg_lo = chunk_agg.lo;
        mine->agg_res = chunk_res;
        __hip_atomic_store(&mine->flag, ep * 4u + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        AbsScan run = {0, 0};  // aggregate of the chunks between the record in hand and this chunk
        uint64_t rrun = 0;
        for (uint32_t pc = ch; pc-- > 0;) {
          LayoutChunk* pr = chunks + (size_t)g * chunks_per_seg + pc;
          uint32_t f;
          uint32_t spins = 0;
          while (((f = __hip_atomic_load(&pr->flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) >> 2) != ep || (f & 3u) == 0u) {
            __builtin_amdgcn_s_sleep(8);
            if (++spins > (1u << 24)) {  // (bounded: a predecessor that never arrives cannot hang the device; the batch is flagged)
              lost = true;
              break;
            }
          }
          if ((f & 3u) == 3u) lost = true;  // a predecessor gave up: so does everything behind it, at once
          if (lost) break;
          if ((f & 3u) == 2u) {
            AbsScan a = {pr->inc_val, (int)pr->inc_set, pr->inc_lo};
            ex = abs_combine(a, run);
            rex = pr->inc_res + rrun;
            break;
          }
          AbsScan a = {pr->agg_val, (int)pr->agg_set, pr->agg_lo};
          run = abs_combine(a, run);
          rrun += pr->agg_res;
        }
      }
      if (lost) raise_status(status, VSYN_ST_BAD_SEGMENT, sg.first_packet);
      s_chunk_lost = lost ? 1u : 0u;
      const AbsScan incl = abs_combine(ex, chunk_agg);
      mine->inc_val = incl.val;
      mine->inc_set = (uint32_t)incl.set;
      mine->inc_lo = incl.lo;
      mine->inc_res = rex + chunk_res;
      __hip_atomic_store(&mine->flag, ep * 4u + (lost ? 3u : 2u), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      s_chunk_ex = ex;
      s_chunk_rex = rex;
    }
  } else if (t == 0) {
    s_chunk_ex = AbsScan{0, 0};
    s_chunk_rex = 0;
    s_chunk_lost = 0u;
  }
  __syncthreads();
  if (s_chunk_lost) {
    // the chain broke in front of this chunk (flagged above): its positions are unknown — mark its packets bad and its runs absent
    // instead of laying them out from a record that was never validated
    for (uint32_t r = ch * runs_per_chunk + t; r < min(runs_per_seg, (ch + 1u) * runs_per_chunk); r += NT) run_cls[(size_t)g * runs_per_seg + r] = 0xFFu;
    for (uint32_t q = cs + t; q < cs + cn; q += NT) {
      PktInfo pi = {};
      pi.bad = 1;
      pi.n = (uint16_t)H->bs[0];
      info[sg.first_packet + q] = pi;
      if (emit_len) emit_len[sg.first_packet + q] = 0;
    }
    if (t == 0 && last_chunk) sinfo[g] = SegInfo{0, 0, 0, 0};
    return;
  }

  // pass B
  {
    AbsScan pre = abs_combine(s_chunk_ex, s_abs[t]);
    int64_t abs_before = abs_eval(pre, abs0);
    uint64_t res_off = sg.residue_off + s_chunk_rex + s_res[t];
    uint32_t prev_n = prev_n0, prev_tail = prev_tail0;
    auto step_b = [&](uint32_t ql, const vsyn_packet& k) {  // ql: index inside the chunk
      const uint32_t q = cs + ql;
      const uint32_t p = sg.first_packet + q;
      const bool mode_ok = k.mode < num_modes;
      const uint32_t lng = mode_ok && s_bf[k.mode] ? 1u : 0u;
      const uint32_t n = lng ? bs1 : bs0;
      const PktStep ps = pkt_step(map_of(cb, 0), k, mode_ok, lng, mode_ok ? s_mm[k.mode] : 0u, n, prev_n, prev_tail, abs_before, abs0, res_off,
                                  plane_stride, C);
      // (one flag at a time, in the order the checks are made: first_bad_packet is a minimum over packets, the flags an OR)
      if (ps.raise & VSYN_ST_BAD_MODE) raise_status(status, VSYN_ST_BAD_MODE, p);
      if (ps.raise & VSYN_ST_WINDOW_FLAGS) raise_status(status, VSYN_ST_WINDOW_FLAGS, p);
      if (ps.raise & VSYN_ST_GRANULE) raise_status(status, VSYN_ST_GRANULE, p);
      if (ps.raise & VSYN_ST_PLANE_OVERFLOW) raise_status(status, VSYN_ST_PLANE_OVERFLOW, p);
      info[p] = ps.pi;
      if (mode_ok && lng) atomicOr(&s_longbits[(ql + 1u) >> 5], 1u << ((ql + 1u) & 31u));
      seg_of_pkt[p] = g;
      if (emit_len) emit_len[p] = ps.pi.emit;
      if (q == num - 1) {
        s_abs_end = ps.abs_after;
        s_last_n = n;
        s_last_tail = prev_tail_of(mode_ok && lng, k.next_long);
      }
      abs_before = ps.abs_after;
      res_off += (uint64_t)C * (n / 2);
      prev_n = n;
      prev_tail = prev_tail_of(mode_ok && lng, k.next_long);
    };
    for (uint32_t base = qb; base < qe; base += KEEP) {
      if (!keep) {
#pragma unroll
        for (uint32_t j = 0; j < KEEP; ++j)
          if (base + j < qe) kq[j] = spk[cs + base + j];
      }
#pragma unroll
      for (uint32_t j = 0; j < KEEP; ++j)
        if (base + j < qe) step_b(base + j, kq[j]);
    }
  }
  __syncthreads();

  // pass C: classify the chunk's runs of R packets. A run goes to the fused long-block kernel iff every packet it touches
  // (its one-packet halo included) is a valid long block and any carry-in is a long block; all other runs are
  // appended to the staged work list (entry = packet index | emit << 31; halo packets carry emit = 0).
  {
    const uint32_t nruns = (num + R - 1) / R;
    for (uint32_t r = ch * runs_per_chunk + t; r < min(runs_per_seg, (ch + 1u) * runs_per_chunk); r += NT) {
      const uint32_t qa = r * R, qb2 = min(num, qa + R);
      // (bitmap positions: packet q of the chunk at bit q - cs + 1; the halo of the chunk's first run at bit 0)
      const uint32_t cls = r >= nruns ? 0xFFu  // 0xFF: no such run
                                      : run_class_bits(s_longbits, qa - cs + 1u, qb2 - cs + 1u, qa == 0 ? carry_n : 0u, fused_ok, qa == 0);
      run_cls[(size_t)g * runs_per_seg + r] = (uint8_t)cls;  // the fused kernels read this instead of re-deriving it
      if (r >= nruns || cls) continue;
      const bool prev_fast = qa > 0 && run_class(H, spk, qa - R, qa, carry_n, fused_ok) != 0;
      const uint32_t cnt = (qb2 - qa) + (prev_fast ? 1u : 0u);
      uint32_t at = atomicAdd(staged_count, cnt);
      if (prev_fast) staged_list[at++] = sg.first_packet + qa - 1;  // IMDCT only: the overlap of `qa` reads its block
      for (uint32_t q = qa; q < qb2; ++q) staged_list[at++] = (sg.first_packet + q) | 0x80000000u;
    }
  }
  if (t == 0 && (last_chunk || num == 0)) {
    SegInfo si;
    si.has_carry = carry_n ? 1u : 0u;
    si.carry_n = carry_n;
    si.parity_in = reset ? 0u : st0.parity;
    if (num == 0) {
      si.total_emit = 0;
      sinfo[g] = si;
      if (reset) state_write(state, sg.stream, st_slot, StreamState{0, 0, 0, 0, 0}, epoch);
      return;
    }
    si.total_emit = (uint32_t)(s_abs_end - abs0);
    sinfo[g] = si;
    StreamState ns;
    ns.abs_total_pos = (uint64_t)s_abs_end;
    ns.has_prev = 1;
    ns.prev_n = s_last_n;
    ns.prev_tail = s_last_tail;
    ns.parity = si.parity_in ^ 1u;
    ns.tag = 0;
    state_write(state, sg.stream, st_slot, ns, epoch);
  }
}

// ------------------------------------------------------------------------------------------------
// K1  floor-1 step 1 (hpp:521-559): one thread per (packet, channel) row, floor1_unwrap_rows (vsyn_floor1.h) as in
// vsyn_prep_kernel. Dynamic LDS: vsyn_handle::unwrap_lds_bytes (a column of the longest floor per thread when it has more than 32 posts).
// ------------------------------------------------------------------------------------------------
#define UNWRAP_THREADS 128
__global__ void __launch_bounds__(UNWRAP_THREADS)
vsyn_floor_unwrap_kernel(const uint8_t* __restrict__ cb, uint32_t P, const PktInfo* __restrict__ info, const uint16_t* __restrict__ ys,
                         uint16_t* __restrict__ fy_out, DevStatus* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_rows[];  // [posts of the longest floor, rounded up to 4][UNWRAP_THREADS]
  const ConstHeader* H = hdr_of(cb);
  const uint32_t C = H->channels, stride = __builtin_amdgcn_readfirstlane(H->ys_stride), t = threadIdx.x;
  const uint32_t rows = P * C;
  // (the trip count is the same for the whole workgroup: floor1_unwrap_rows votes across the wave, rows past the end take part inactive)
  for (uint32_t base = blockIdx.x * UNWRAP_THREADS; base < rows; base += gridDim.x * UNWRAP_THREADS) {
    const uint32_t row = base + t, p = row / C, c = row - p * C;
    bool act = false;
    uint32_t fl_id = 0xFFFFFFFFu;
    if (row < rows) {
      const PktInfo pi = info[p];
      act = !pi.bad && ((pi.own >> c) & 1u);
      if (act) fl_id = map_of(cb, pi.mapping)->chfloor[c];
    }
    floor1_unwrap_rows(cb, ys, fy_out, status, act, fl_id, p, row, stride, (floor1_lds_u32*)s_rows + t, UNWRAP_THREADS);
  }
}

// ------------------------------------------------------------------------------------------------
// K2 (staged)  inverse coupling (hpp:1213-1241) + floor product (hpp:1243-1255): one thread per bin,
// all channels of the bin handled by the same thread (couplings chain across channels), in place in `env`.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void inverse_couple(float& m, float& a) {  // hpp:1220-1239 as selects (see couple2)
  const float d = m > 0.f ? a : -a;
  const float x = m - d, y = m + d;
  const bool ap = a > 0.f;
  a = ap ? x : m;
  m = ap ? m : y;
}

__global__ void __launch_bounds__(256)
vsyn_spectrum_kernel(const uint8_t* __restrict__ cb, const uint32_t* __restrict__ list, const uint32_t* __restrict__ count,
                     const PktInfo* __restrict__ info, const float* __restrict__ residue, const uint16_t* __restrict__ fy,
                     float* __restrict__ env, uint16_t* __restrict__ curve_tap, DevStatus* __restrict__ status) {
  const ConstHeader* H = hdr_of(cb);
  const uint32_t total = *count;
  for (uint32_t li = blockIdx.x; li < total; li += gridDim.x) {  // grid-stride over the staged work list
  const uint32_t p = list[li] & 0x7FFFFFFFu;
  const PktInfo pi = info[p];
  if (pi.bad) continue;
  const uint32_t n2 = pi.n / 2u, C = H->channels;
  for (uint32_t i = threadIdx.x; i < n2; i += 256) {
  const float* src = residue + pi.res_off;
  float* dst = env + pi.res_off;
  for (uint32_t c = 0; c < C; ++c) dst[(size_t)c * n2 + i] = src[(size_t)c * n2 + i];
  const MapConst* mc = map_of(cb, pi.mapping);
  for (uint32_t k = mc->ncoup; k > 0; --k) {  // reverse order, hpp:1214
    const uint32_t m = mc->coup[2 * (k - 1)], a = mc->coup[2 * (k - 1) + 1];
    float mv = dst[(size_t)m * n2 + i], av = dst[(size_t)a * n2 + i];
    inverse_couple(mv, av);
    dst[(size_t)m * n2 + i] = mv;
    dst[(size_t)a * n2 + i] = av;
  }
  const float* invdb = invdb_of(cb);
  for (uint32_t c = 0; c < C; ++c) {
    if (!((pi.used >> c) & 1u)) continue;
    float f = 0.f;  // propagated-but-undecoded floor: floor_outputs stays zero (hpp:1159, 1169)
    if ((pi.own >> c) & 1u) {
      const FloorConst* fc = floor_of(cb, mc->chfloor[c]);
      const uint32_t v = floor1_curve_at(fc, fy + ((size_t)p * C + c) * H->ys_stride, i);
      if (curve_tap) curve_tap[pi.res_off + (size_t)c * n2 + i] = (uint16_t)min(v, 65535u);  // "floor1 floor", hpp:585
      if (v >= 256u) {  // hpp:587
        raise_status(status, VSYN_ST_FLOOR_VALUE, p);
        f = 0.f;
      } else {
        f = invdb[v];
      }
    }
    dst[(size_t)c * n2 + i] *= f;
  }
  }
  }
}

// ------------------------------------------------------------------------------------------------
// K3 (staged)  IMDCT for any n = 64..8192: one workgroup per block, radix-2 Stockham FFT of n/4 complex
// points in LDS.  Computes what mdct_backward (mdct.cpp:433-527) computes, by a different factorisation:
//   c[k]  = (X[2k] + i X[M-1-2k]) * exp(-i pi (4k+1) / (4M)),  M = n/2, k < n/4
//   Cf    = FFT_{n/4}(c);  d[m] = Cf[m] * exp(-i pi m / M)
//   u[2m] = Re d[m], u[M-1-2m] = -Im d[m]                     (u = DCT-IV of X)
//   y[i]  = u[i+M/2] (i < M/2);  -u[3M/2-1-i] (M/2 <= i < 3M/2);  -u[i-3M/2] (i >= 3M/2)
// Twiddles are computed in double on the host and stored as f32 (like mdct_init, mdct.cpp:101-110).
// Results agree with the reference to ~1e-7 * |output| (gate: 1e-5 abs at |pcm| <= 1, compare-debug-out.py:90).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(__builtin_fmaf(a.x, b.x, -(a.y * b.y)), __builtin_fmaf(a.x, b.y, a.y * b.x));
}

__device__ void imdct_block_lds(const uint8_t* __restrict__ cb, int b, uint32_t n, const float* __restrict__ X,
                                float* __restrict__ y, float2* bufA, float2* bufB) {
  const uint32_t M = n / 2, N4 = n / 4, T = blockDim.x, t = threadIdx.x;
  const float2* pre = pre_of(cb, b);
  const float2* post = post_of(cb, b);
  const float2* tw = fft_of(cb, b);
  for (uint32_t k = t; k < N4; k += T) bufA[k] = cmul(make_float2(X[2 * k], X[M - 1 - 2 * k]), pre[k]);
  __syncthreads();
  float2* src = bufA;
  float2* dst = bufB;
  for (uint32_t Ns = 1; Ns < N4; Ns <<= 1) {
    const uint32_t tstride = N4 / (2 * Ns);
    for (uint32_t j = t; j < N4 / 2; j += T) {
      const uint32_t k = j & (Ns - 1);
      const float2 v0 = src[j];
      const float2 v1 = cmul(src[j + N4 / 2], tw[k * tstride]);
      const uint32_t o = ((j - k) << 1) + k;
      dst[o] = make_float2(v0.x + v1.x, v0.y + v1.y);
      dst[o + Ns] = make_float2(v0.x - v1.x, v0.y - v1.y);
    }
    __syncthreads();
    float2* tmp = src;
    src = dst;
    dst = tmp;
  }
  float* u = (float*)dst;  // M floats == N4 float2
  for (uint32_t m = t; m < N4; m += T) {
    const float2 d = cmul(src[m], post[m]);
    u[2 * m] = d.x;
    u[M - 1 - 2 * m] = -d.y;
  }
  __syncthreads();
  for (uint32_t i = t; i < n; i += T) {
    float v;
    if (i < M / 2) v = u[i + M / 2];
    else if (i < 3 * M / 2) v = -u[3 * M / 2 - 1 - i];
    else v = -u[i - 3 * M / 2];
    y[i] = v;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(256)
vsyn_imdct_staged_kernel(const uint8_t* __restrict__ cb, const uint32_t* __restrict__ list, const uint32_t* __restrict__ count,
                         const PktInfo* __restrict__ info, const float* __restrict__ env, float* __restrict__ blk) {
  extern __shared__ __align__(16) uint8_t lds_raw[];
  const ConstHeader* H = hdr_of(cb);
  const uint32_t C = H->channels, total = *count * C;
  for (uint32_t w = blockIdx.x; w < total; w += gridDim.x) {
    const uint32_t p = list[w / C] & 0x7FFFFFFFu, c = w % C;
    const PktInfo pi = info[p];
    if (pi.bad) continue;
    const uint32_t n = pi.n;
    float2* bufA = (float2*)lds_raw;
    float2* bufB = bufA + n / 4;
    imdct_block_lds(cb, pi.lng, n, env + pi.res_off + (size_t)c * (n / 2), blk + 2 * pi.res_off + (size_t)c * n, bufA, bufB);
  }
}

// plain [count][n/2] -> [count][n] (BASELINE config 2), generic version
__global__ void __launch_bounds__(256)
vsyn_imdct_plain_kernel(const uint8_t* __restrict__ cb, int b, uint32_t n, uint32_t count, const float* __restrict__ in,
                        float* __restrict__ out) {
  extern __shared__ __align__(16) uint8_t lds_raw[];
  float2* bufA = (float2*)lds_raw;
  float2* bufB = bufA + n / 4;
  for (uint32_t blk = blockIdx.x; blk < count; blk += gridDim.x)
    imdct_block_lds(cb, b, n, in + (size_t)blk * (n / 2), out + (size_t)blk * n, bufA, bufB);
}

// ------------------------------------------------------------------------------------------------
// K4 (staged)  window + overlap-add + PCM hand-off (hpp:1008-1059) as a gather: emitted sample s of packet q
//   = fl( fl(prev[n_prev/2 + s] * w_prev[n_prev/2 + s]) + fl(cur[j] * w_cur[j]) ),  j = n_cur/2 - L + s,
// each term present only where its block covers the sample (tests/test_oracle_vs_ref.py pins this against
// the reference's sliding buffer).  Mul and add are rounded separately, as `buf += pcm*window` is upstream.
// The last packet of a segment also stores its windowed right half as the stream's carry.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
vsyn_overlap_kernel(const uint8_t* __restrict__ cb, const uint32_t* __restrict__ list, const uint32_t* __restrict__ count,
                    const PktInfo* __restrict__ info, const vsyn_segment* __restrict__ segs, const SegInfo* __restrict__ sinfo,
                    const uint32_t* __restrict__ seg_of_pkt, const float* __restrict__ blk, float* __restrict__ pcm,
                    uint64_t plane_stride, float* __restrict__ carry) {
  const ConstHeader* H = hdr_of(cb);
  const uint32_t C = H->channels, total = *count * C;
  for (uint32_t w = blockIdx.x; w < total; w += gridDim.x) {
  const uint32_t entry = list[w / C], c = w % C;
  if (!(entry >> 31)) continue;  // halo entry: block only
  const uint32_t p = entry & 0x7FFFFFFFu;
  const uint32_t g = seg_of_pkt[p];
  const PktInfo pi = info[p];
  if (pi.bad) continue;
  for (uint32_t s = threadIdx.x; s < H->bs[1] / 2; s += 256) {
  const vsyn_segment sg = segs[g];
  const SegInfo si = sinfo[g];
  const uint32_t q = p - sg.first_packet, n = pi.n, half1 = H->bs[1] / 2;
  const float* cur = blk + 2 * pi.res_off + (size_t)c * n;
  const float* wc = win_of(cb, pi.lng, pi.widx);
  const size_t carry_half = (size_t)H->max_streams * C * half1;

  // prev block (or carry)
  uint32_t n_prev = 0;
  const float* prev = nullptr;
  const float* wp = nullptr;
  const float* cin = nullptr;
  if (q > 0) {
    const PktInfo pp = info[p - 1];
    if (!pp.bad) {
      n_prev = pp.n;
      prev = blk + 2 * pp.res_off + (size_t)c * n_prev;
      wp = win_of(cb, pp.lng, pp.widx);
    }
  } else if (si.has_carry) {
    n_prev = si.carry_n;
    cin = carry + si.parity_in * carry_half + ((size_t)sg.stream * C + c) * half1;
  }
  if (s < pi.emit && n_prev) {
    const uint32_t L = n_prev / 4 + n / 4;
    float acc = 0.f;
    const uint32_t ip = n_prev / 2 + s;
    if (ip < n_prev) acc = acc + (cin ? cin[s] : prev[ip] * wp[ip]);
    const int32_t j = (int32_t)(n / 2) - (int32_t)L + (int32_t)s;
    if (j >= 0) acc = acc + cur[j] * wc[j];
    pcm[((size_t)g * C + c) * plane_stride + pi.out_pos + s] = acc;
  }
  if (q == sg.num_packets - 1 && s < n / 2) {
    float* cout = carry + (si.parity_in ^ 1u) * carry_half + ((size_t)sg.stream * C + c) * half1;
    cout[s] = cur[n / 2 + s] * wc[n / 2 + s];
  }
  }
  }
}

