// vsyn_host.h — what every host section shares: the error text, HIPCHK, grow-only device buffers, per-call table uploads.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <numeric>
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
