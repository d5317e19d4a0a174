// vsyn_host.h — what every host section shares: the error text, HIPCHK, grow-only device buffers, per-call table uploads.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <numeric>
#include <utility>
#include <vector>

#include "vsyn_device.h"

#ifndef M_PI
#define M_PI 3.14159265358979323846264338327
#endif
#ifndef M_PI_2
#define M_PI_2 1.57079632679489661923
#endif

static thread_local char g_err[512];

static inline int fail(const char** err, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  if (err) *err = g_err;
  return code;
}

#define HIPCHK(call)                                                                                      \
  do {                                                                                                    \
    hipError_t e_ = (call);                                                                               \
    if (e_ != hipSuccess)                                                                                 \
      return fail(err, VSYN_ERR_HIP, "%s:%d: %s failed: %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
  } while (0)

template <typename T>
struct DevBuf {  // grow-only device buffer
  T* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t n) {
    if (n <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = n + n / 8 + 64;
    hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
    if (e == hipSuccess) cap = want;
    return e;
  }
  ~DevBuf() {  // (vsyn_destroy selects the device before the handle goes away)
    if (p) (void)hipFree(p);
  }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
};

// A table built on the host per call and uploaded asynchronously from a page-locked copy. One instance per front-end: each keeps
// buffers of its own.
struct TableUpload {
  DevBuf<uint8_t> dev;
  uint8_t* host = nullptr;  // page-locked copy of the table (the upload is asynchronous)
  size_t host_cap = 0;
  hipEvent_t ev = nullptr;  // recorded behind the upload: the host copy is reused only after it
  bool ev_valid = false;
  int upload(const std::vector<uint8_t>& tab, hipStream_t s, const char** err) {
    HIPCHK(dev.ensure(tab.size()));
    if (!ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    if (ev_valid) HIPCHK(hipEventSynchronize(ev));  // the previous upload has read the host copy
    if (host_cap < tab.size()) {
      if (host) HIPCHK(hipHostFree(host));
      host = nullptr;
      host_cap = 0;
      HIPCHK(hipHostMalloc((void**)&host, tab.size() + 4096, hipHostMallocDefault));
      host_cap = tab.size() + 4096;
    }
    memcpy(host, tab.data(), tab.size());
    HIPCHK(hipMemcpyAsync(dev.p, host, tab.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(ev, s));
    ev_valid = true;
    return VSYN_OK;
  }
  ~TableUpload() {  // (as DevBuf's: vsyn_destroy selects the device before the handle goes away; not copyable, as DevBuf is not)
    if (ev) (void)hipEventDestroy(ev);
    if (host) (void)hipHostFree(host);
  }
};

// Launch and return the launch's error from the calling function (the text names the file and line of the site).
#define VSYN_LAUNCH(kernel, grid, block, lds, stream, ...)              \
  do {                                                                  \
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);  \
    HIPCHK(hipGetLastError());                                          \
  } while (0)

// Raise the dynamic-LDS limits of a stage's kernels, once per handle (flag: the workspace's word for it; the device is selected).
struct LdsLimit {
  const void* kernel;
  size_t bytes;
};
static inline int raise_lds_once(bool& flag, std::initializer_list<LdsLimit> limits, const char** err) {
  if (flag) return VSYN_OK;
  for (const LdsLimit& l : limits) HIPCHK(hipFuncSetAttribute(l.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.bytes));
  flag = true;
  return VSYN_OK;
}

// The per-segment records of the stages that walk rows [rows][D] segment by segment: the segment's first row and its rows, and for
// the stages that cut a segment into blocks of rows its first block. A stage whose record carries more derives from one of them (the
// kernels read the same bytes) or keeps a record and a loop of its own.
struct RowSeg {
  uint64_t off;  // first row of the segment in the row buffers
  uint32_t F, pad;
};
struct RowBlkSeg {
  uint64_t off;  // first row of the segment in the row buffers
  uint64_t blk;  // first block of the segment in the stage's per-block buffers
  uint32_t F, pad;
};
// Thread layout of a workgroup of THREADS over rows of D columns: wd lanes along the columns, G = THREADS / wd row groups; this thread
// is lane tx of group ty (a thread with ty >= G has no group).
struct RowLane {
  uint32_t wd, G, ty, tx;
};
template <uint32_t THREADS>
__device__ __forceinline__ RowLane row_lane(uint32_t D) {
  RowLane L;
  L.wd = min(D, THREADS);
  L.G = THREADS / L.wd;
  L.ty = threadIdx.x / L.wd;
  L.tx = threadIdx.x - L.ty * L.wd;
  return L;
}
struct RowTotals {
  uint64_t rows = 0, blocks = 0, f_max = 0;  // all rows (skipped segments' too), the live segments' blocks, the longest live segment
};
static inline void row_seg_set(RowSeg& r, const RowTotals& t, uint32_t F) { r.off = t.rows, r.F = F, r.pad = 0u; }
static inline void row_seg_set(RowBlkSeg& r, const RowTotals& t, uint32_t F) { r.off = t.rows, r.blk = t.blocks, r.F = F, r.pad = 0u; }
// seg[g] for g < S from seg_rows; live (may be NULL): a segment with live[g] = 0 keeps its place but has F = 0. blk_len: rows a block.
template <class Seg>
static inline RowTotals row_segs_fill(Seg* seg, uint32_t S, const uint64_t* seg_rows, const uint32_t* live, uint32_t blk_len) {
  RowTotals t;
  for (uint32_t g = 0; g < S; ++g) {
    const uint64_t F = live && !live[g] ? 0u : seg_rows[g];
    row_seg_set(seg[g], t, (uint32_t)F);
    t.rows += seg_rows[g];
    t.blocks += (F + blk_len - 1u) / blk_len;
    t.f_max = std::max(t.f_max, F);
  }
  return t;
}

static inline uint64_t seg_total(uint32_t S, const uint64_t* seg_rows) {
  uint64_t total = 0;
  for (uint32_t g = 0; g < S; ++g) total += seg_rows[g];
  return total;
}

// The refusals every call over seg_rows[S] shares, in this order.
static inline int rows_check_segs(uint32_t S, const uint64_t* seg_rows, uint64_t max_rows, const char** err) {
  if (S && !seg_rows) return fail(err, VSYN_ERR_INVALID, "seg_rows is NULL");
  if (S > 65535u) return fail(err, VSYN_ERR_INVALID, "too many segments (%u > 65535)", S);
  for (uint32_t g = 0; g < S; ++g)
    if (seg_rows[g] > max_rows) return fail(err, VSYN_ERR_INVALID, "segment %u: too many rows", g);
  return VSYN_OK;
}

// Tables shared by the segments of one key, laid out back to back: the offset of key's table among those already placed (key,
// offset), else it is placed at *next, which grows by len.
static inline uint32_t table_slot(std::vector<std::pair<uint32_t, uint32_t>>& placed, uint32_t key, uint32_t* next, uint32_t len) {
  for (const auto& p : placed)
    if (p.first == key) return p.second;
  placed.push_back(std::make_pair(key, *next));
  *next += len;
  return placed.back().second;
}

static inline bool is_pow2(uint32_t v) { return v && !(v & (v - 1)); }
static inline uint32_t ilog2(uint32_t v) {
  uint32_t r = 0;
  while ((1u << r) < v) ++r;
  return r;
}
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

static inline void status_reset(vsyn_status* status) {
  if (status) {
    status->flags = 0;
    status->first_bad_packet = 0xFFFFFFFFu;
  }
}
