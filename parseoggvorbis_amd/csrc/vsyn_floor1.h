// vsyn_floor1.h — floor-1 (hpp:416-589) on the device: step 1, the unwrap of a row's coded posts into amplitudes, for
// vsyn_prep_kernel (vsyn_prep.h) and vsyn_floor_unwrap_kernel (vsyn_staged.h); step 2, the integer curve at one bin, for the staged
// and feature kernels. Neighbour indices come precomputed from the setup (Utils.hpp:60-118 depend on xs only). uint32 wrap-around
// semantics as in the reference (y_t = uint32_t).
#pragma once
#include <hip/hip_runtime.h>

#include "vsyn_device.h"

typedef __attribute__((address_space(3))) uint32_t floor1_lds_u32;

__device__ __forceinline__ uint32_t render_point_u32(uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, uint32_t X) {
  // Utils.hpp:122-137
  uint32_t adx = x1 - x0;
  bool up = y1 >= y0;
  uint32_t ady = up ? y1 - y0 : y0 - y1;
  uint32_t off = (ady * (X - x0)) / adx;
  return up ? y0 + off : y0 - off;
}

// Floor-1 step 1 (hpp:521-559) of the rows held by the lanes with `act` set: row gid = (packet p, channel c) of the coded rows `ys`
// into the output rows `fy` (both `stride` posts apart), floor number fl_id (any mix of floors: rows of one floor are processed together
// so that the schedule comes through the scalar unit). Every lane of the wave calls it, active or not (__ballot / readlane inside).
// Output row: final_y * multiplier (saturated to 15 bits) | step2_flag << 15, header order; a row with a prediction out of range
// (hpp:536) raises VSYN_ST_FLOOR_RANGE and is written as 0x8000 in every post (flat zero curve, all flagged: harmless).
// The prediction render_point(xs[lo], fy[lo], xs[hi], fy[hi], xs[i]) has the post geometry folded into the per-floor constants
// dxi = xs[i] - xs[lo] and inv = 1 / (xs[hi] - xs[lo]): off = (|dy| * dxi) / adx exactly, as floor((prod + 0.5) * inv) while
// prod = |dy| * dxi < 2^21 (in-range amplitudes on posts up to 8192: prod <= 255 * 8191; the format allows posts up to 32767, whose
// larger products take the integer division like absurd coded values do), where prod + 0.5 is exact and the rounding of the
// product (<= 2.4e-7 * prod / adx) stays inside the 0.5 / adx guard band; else the integer division.
// Floors of more than 32 posts: the row's posts live in LDS, col[post * NT] (32-bit amplitudes, the thread's own column of NT threads:
// conflict-free, no synchronisation), and are worked on in GROUPS of four mutually independent posts (FloorConst::sched): twelve LDS
// reads in flight together, four chains of arithmetic side by side, four writes. Evaluation order differs from the header's, the
// values do not: a post depends on its two neighbours only, and those sit in earlier groups. Shorter floors: a register array.
__device__ __forceinline__ void floor1_unwrap_rows(const uint8_t* cb, const uint16_t* ys, uint16_t* fy, DevStatus* status, const bool act,
                                                   const uint32_t fl_id, const uint32_t p, const size_t gid, const uint32_t stride,
                                                   floor1_lds_u32* const col, const uint32_t NT) {
  const FloorConst* const floors = (const FloorConst*)(cb + hdr_of(cb)->off_floor);
  typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
  typedef const __attribute__((address_space(4))) u32x16* const_grp;
  typedef const __attribute__((address_space(4))) uint32_t* kptr;
  uint64_t todo = __ballot(act);
  while (todo) {
    const uint32_t f = __builtin_amdgcn_readlane(fl_id, (uint32_t)__builtin_ctzll(todo));
    const bool mine = act && fl_id == f;
    todo &= ~__ballot(mine);
    const FloorConst* fc = floors + f;
    const uint32_t posts = *(kptr)(uintptr_t)&fc->posts, range = *(kptr)(uintptr_t)&fc->range, mult = *(kptr)(uintptr_t)&fc->mult;
    const uint32_t ngroups = *(kptr)(uintptr_t)&fc->ngroups;
    if (!mine) continue;  // (divergent from here on: the lanes of this floor)
    if (posts <= 32u) {
      // Up to 32 posts (every floor libvorbis writes for the common modes): the row in a register array indexed by the wave-uniform
      // neighbour numbers, one post at a time in header order, the per-post constants by scalar loads of four posts, one load ahead.
      // Measured on config 3 (29 posts, two waves per SIMD): 620 cycles per post with round 3's first form of the chain (~70 instructions
      // per post, a wave vote and two divergent branches in it), the kernel 20.7 us; 19.3 us with the form below. The grouped forms
      // further down / with this array cost 1.7x / 2x per post (an access to the array is an s_set_gpr_idx mode switch; four chains
      // side by side do not make up for it).
      uint32_t fr[32];
      const uint2* in8 = (const uint2*)(ys + gid * stride);
      uint2 win[8];
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) {
        win[j] = make_uint2(0u, 0u);
        if (j * 4 < posts) win[j] = in8[j];
      }
      uint32_t flags = 3;
      bool bad = false;
      // The chain runs on the float form of the prediction's division (exact while |dy| * dx < 2^21: always, for amplitudes in range) and
      // only NOTES a larger product; a row that saw one (absurd coded values) is redone with the integer division afterwards. No
      // wave-level vote and no divergent branch inside the chain: ~50 instead of ~70 instructions per post, and the chain is what this
      // kernel's time is.
      typedef const __attribute__((address_space(4))) u32x16* const_pk4;
      for (int attempt = 0; attempt < 2; ++attempt) {
        const bool exact = attempt == 1;
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
          fr[4 * j + 0] = win[j].x & 0xFFFFu;
          fr[4 * j + 1] = win[j].x >> 16;
          fr[4 * j + 2] = win[j].y & 0xFFFFu;
          fr[4 * j + 3] = win[j].y >> 16;
        }
        flags = 3;
        bad = false;
        uint32_t big_acc = 0;
        auto step = [&](const uint32_t i, const uint32_t kx, const uint32_t ky, const uint32_t kz, const uint32_t touched) {
          const uint32_t lo = kx & 0xFFFFu, hi = kx >> 16;
          const uint32_t val = fr[i], ylo = fr[lo], yhi = fr[hi];
          const uint32_t dxi = ky & 0xFFFFu, adx = ky >> 16;
          const bool up = yhi >= ylo;
          const uint32_t ady = up ? yhi - ylo : ylo - yhi;
          const uint32_t prod = ady * dxi;
          uint32_t off;
          if (exact) {
            off = prod / adx;
          } else {
            off = (uint32_t)(((float)prod + 0.5f) * __uint_as_float(kz));  // == prod / adx while prod < 2^21 (above)
            big_acc |= prod >> 21;
          }
          const uint32_t predicted = up ? ylo + off : ylo - off;
          const bool ok = predicted <= range;  // hpp:536
          const uint32_t pr = ok ? predicted : 0u;
          // hpp:540-556 without branches: m = the smaller room; beyond 2 m the value counts linearly from the nearer edge (d resp. -d - 1),
          // below it it is the zig-zag code of the offset (even: + val / 2, odd: - (val + 1) / 2 = ~(val >> 1))
          const uint32_t high_room = range - pr;
          const uint32_t m = min(high_room, pr);
          const uint32_t d = val - m;
          const uint32_t dbig = high_room > pr ? d : ~d;
          const uint32_t dsmall = (val >> 1) ^ (0u - (val & 1u));
          const uint32_t delta = val >= 2u * m ? dbig : dsmall;
          const uint32_t fn = val == 0 ? pr : pr + delta;
          flags |= val != 0 ? touched : 0u;  // (1 << lo) | (1 << hi) | (1 << i), from the table
          bad = bad || !ok;
          fr[i] = bad ? 0u : fn;  // after the first out-of-range prediction the row is dropped; keep the chain tame
        };
        u32x16 kn = *(const_pk4)(uintptr_t)&fc->pk[2];
        for (uint32_t i = 2; i < posts; i += 4) {
          const u32x16 kq = kn;
          kn = *(const_pk4)(uintptr_t)&fc->pk[i + 4];  // (pk[] has 66 entries)
          step(i, kq[0], kq[1], kq[2], kq[3]);
          if (i + 1 < posts) step(i + 1, kq[4], kq[5], kq[6], kq[7]);
          if (i + 2 < posts) step(i + 2, kq[8], kq[9], kq[10], kq[11]);
          if (i + 3 < posts) step(i + 3, kq[12], kq[13], kq[14], kq[15]);
        }
        if (exact || !__any(big_acc != 0u)) break;
        if (big_acc == 0u) break;  // (only the rows that saw a large product are redone)
      }
      uint2* out8 = (uint2*)(fy + gid * stride);
      if (bad) raise_status(status, VSYN_ST_FLOOR_RANGE, p);
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) {
        if (j * 4 >= posts) break;
        uint32_t w[4];
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) {
          const uint32_t i = 4 * j + e;
          uint32_t v = fr[i] * mult;  // hpp:573,578
          if (v > 0x7FFFu || fr[i] > 0x7FFFu) v = 0x7FFFu;
          w[e] = i < posts ? (bad ? 0x8000u : (v | (((flags >> i) & 1u) << 15))) : 0u;
        }
        out8[j] = make_uint2(w[0] | (w[1] << 16), w[2] | (w[3] << 16));
      }
      continue;
    }
    {
      const uint2* in8 = (const uint2*)(ys + gid * stride);
      for (uint32_t j = 0; j * 4 < posts; ++j) {
        const uint2 w = in8[j];
        col[(4 * j + 0) * NT] = w.x & 0xFFFFu;
        col[(4 * j + 1) * NT] = w.x >> 16;
        col[(4 * j + 2) * NT] = w.y & 0xFFFFu;
        col[(4 * j + 3) * NT] = w.y >> 16;
      }
    }
    uint64_t flags_lo = 3;
    uint32_t flag_64 = 0;
    bool bad = false;
    u32x16 kn = *(const_grp)(uintptr_t)&fc->sched[0][0];
    for (uint32_t gi = 0; gi < ngroups; ++gi) {
      const u32x16 kq = kn;
      kn = *(const_grp)(uintptr_t)&fc->sched[gi + 1u < VSYN_SCHED_GROUPS ? gi + 1u : gi][0];  // one group ahead
      uint32_t val[4], ylo[4], yhi[4], fn[4], prod[4], off[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        val[e] = col[kq[4 * e + 3] * NT];
        ylo[e] = col[(kq[4 * e] & 0xFFFFu) * NT];
        yhi[e] = col[(kq[4 * e] >> 16) * NT];
      }
      bool any_big = false;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t dxi = kq[4 * e + 1] & 0xFFFFu;
        const bool up = yhi[e] >= ylo[e];
        const uint32_t ady = up ? yhi[e] - ylo[e] : ylo[e] - yhi[e];
        prod[e] = ady * dxi;
        // == prod / adx while prod < 2^21 (above); the rare larger products take the integer division below
        off[e] = (uint32_t)(((float)prod[e] + 0.5f) * __uint_as_float(kq[4 * e + 2]));
        any_big = any_big || prod[e] >= (1u << 21) || ady >= 65536u;
      }
      if (__any(any_big)) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool up = yhi[e] >= ylo[e];
          const uint32_t ady = up ? yhi[e] - ylo[e] : ylo[e] - yhi[e];
          if (prod[e] >= (1u << 21) || ady >= 65536u) off[e] = prod[e] / (kq[4 * e + 1] >> 16);
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool up = yhi[e] >= ylo[e];
        const uint32_t predicted = up ? ylo[e] + off[e] : ylo[e] - off[e];
        const bool ok = predicted <= range;  // hpp:536
        const uint32_t pr = ok ? predicted : 0u;
        const uint32_t high_room = range - pr, low_room = pr;
        const uint32_t room = min(high_room, low_room) * 2;
        const uint32_t big = high_room > low_room ? val[e] - low_room + pr : pr - val[e] + high_room - 1;
        const uint32_t small = (val[e] & 1u) ? pr - (val[e] + 1) / 2 : pr + val[e] / 2;
        fn[e] = val[e] == 0 ? pr : (val[e] >= room ? big : small);
        const uint32_t lo = kq[4 * e] & 0xFFFFu, hi = kq[4 * e] >> 16, i = kq[4 * e + 3];  // lo, hi < i <= 64
        const uint64_t touched = (1ull << lo) | (1ull << hi) | (i < 64u ? 1ull << i : 0ull);
        flags_lo |= val[e] != 0 ? touched : 0ull;
        flag_64 |= (val[e] != 0 && i >= 64u) ? 1u : 0u;
        bad = bad || !ok;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) col[kq[4 * e + 3] * NT] = bad ? 0u : fn[e];  // (a row with an out-of-range prediction is dropped: keep the chain tame)
    }
    uint2* out8 = (uint2*)(fy + gid * stride);
    if (bad) raise_status(status, VSYN_ST_FLOOR_RANGE, p);
    for (uint32_t j = 0; j * 4 < posts; ++j) {
      uint32_t w[4];
#pragma unroll
      for (uint32_t e = 0; e < 4; ++e) {
        const uint32_t i = 4 * j + e;
        const uint32_t fv = i < posts ? col[i * NT] : 0u;
        uint32_t v = fv * mult;  // hpp:573,578
        if (v > 0x7FFFu || fv > 0x7FFFu) v = 0x7FFFu;  // wrapped / absurd amplitude: renders >= 256 -> FLOOR_VALUE later
        const uint32_t fl = i < 64 ? (uint32_t)((flags_lo >> i) & 1ull) : (i == 64 ? flag_64 : 0u);
        w[e] = i < posts ? (bad ? 0x8000u : (v | (fl << 15))) : 0u;
      }
      out8[j] = make_uint2(w[0] | (w[1] << 16), w[2] | (w[3] << 16));
    }
  }
}

// floor-1 step 2 for ONE bin (hpp:563-589): value of the piecewise-linear integer curve at x.
// render_line's DDA (Utils.hpp:143-183) equals render_point per x (tests/test_oracle_vs_ref.py::test_render_helpers).
// Generic linear walk over the sorted posts; the fused kernels use a precomputed segment table instead.
__device__ __forceinline__ uint32_t floor1_curve_at(const FloorConst* fc, const uint16_t* __restrict__ fyrow, uint32_t x) {
  uint32_t lx = 0, ly = fyrow[fc->sorted_idx[0]] & 0x7FFFu;
  for (uint32_t s = 1; s < fc->posts; ++s) {
    const uint32_t v = fyrow[fc->sorted_idx[s]];
    if (!(v >> 15)) continue;
    const uint32_t hx = fc->xs_sorted[s], hy = v & 0x7FFFu;
    if (x < hx) return render_point_u32(lx, ly, hx, hy, x);
    lx = hx;
    ly = hy;
  }
  return ly;  // flat extension, hpp:583-584
}
