// vsyn_wave.h — the reductions and scans of the stage kernels, written once. Device templates only; no kernel, no LDS of its own.
// The orders below are part of every stage's contract ("Reduction and scan orders"); the numpy models in tests/ follow them.
//   wave_sum / wave_min / wave_max  the xor butterfly over the lane offsets 32, 16, .. 1: v = op(v, the partner's v) each round, and
//                                   every lane of the wave ends with the same result.
//   wave_scan                       inclusive Hillis-Steele over the lane offsets 1, 2, .. 32: if (lane >= o) inc += the value o below.
//   wg_put / wg_get                 the second level: the wave step and one LDS word per wave, then (behind the caller's barrier) the
//                                   words folded in ascending order onto the identity: ((identity op w[0]) op w[1]) op ..
//   wg_reduce_all / wg_reduce_t0    both levels. _all: the result in every thread, two barriers, scratch free again on return.
//                                   _t0: the result in thread 0 alone, one barrier, scratch still in use on return.
//   wg_sum_scan<M>                  M ordered sums over a workgroup of four waves at once: wave_scan of the threads' totals, the waves'
//                                   totals through LDS, a wave's offset the sum of the earlier waves' totals in ascending order,
//                                   exc = wave offset + exclusive lane prefix, tot = ((w[0] + w[1]) + w[2]) + w[3].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// 64-bit shuffles from two 32-bit ones
__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int o) {
  return ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, o);
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
  return ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)v, src);
}
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, unsigned d) {
  return ((uint64_t)(uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d) << 32) | (uint32_t)__shfl_up((int)(uint32_t)v, d);
}

// the partner's value of one butterfly round, and the value o lanes below, by type
__device__ __forceinline__ float wave_xor(float v, int o) { return __shfl_xor(v, o); }
__device__ __forceinline__ double wave_xor(double v, int o) { return __shfl_xor(v, o); }
__device__ __forceinline__ uint32_t wave_xor(uint32_t v, int o) { return (uint32_t)__shfl_xor((int)v, o); }
__device__ __forceinline__ uint64_t wave_xor(uint64_t v, int o) { return shfl_xor64(v, o); }
__device__ __forceinline__ double wave_up(double v, unsigned o) { return __shfl_up(v, o); }
__device__ __forceinline__ uint32_t wave_up(uint32_t v, unsigned o) { return __shfl_up(v, o); }

struct WaveSum {
  template <typename T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct WaveMin {
  __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
  __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); }
  __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return min(a, b); }
  __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return a < b ? a : b; }
};
struct WaveMax {
  __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
  __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
  __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return max(a, b); }
  __device__ __forceinline__ uint64_t operator()(uint64_t a, uint64_t b) const { return a > b ? a : b; }
};

template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
  for (int o = 32; o; o >>= 1) v = op(v, wave_xor(v, o));
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, WaveSum()); }
template <typename T>
__device__ __forceinline__ T wave_min(T v) { return wave_reduce(v, WaveMin()); }
template <typename T>
__device__ __forceinline__ T wave_max(T v) { return wave_reduce(v, WaveMax()); }

template <typename T>
__device__ __forceinline__ T wave_scan(T v) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t o = 1; o < 64u; o <<= 1) {
    const T up = wave_up(v, o);
    if (lane >= o) v += up;
  }
  return v;
}

template <typename T>
struct WaveSame {  // (keeps an argument out of the deduction of T: the identity converts to the value's type)
  typedef T type;
};

// the wave step, and the wave's word into scratch[WAVES]; returns the wave's result
template <typename T, typename Op>
__device__ __forceinline__ T wg_put(T v, T* scratch, Op op) {
  v = wave_reduce(v, op);
  if ((threadIdx.x & 63u) == 0u) scratch[threadIdx.x >> 6] = v;
  return v;
}
// behind a barrier: the waves' words in ascending order
template <uint32_t WAVES, typename T, typename Op>
__device__ __forceinline__ T wg_get(const T* scratch, Op op, typename WaveSame<T>::type identity) {
  T r = identity;
#pragma unroll
  for (uint32_t w = 0; w < WAVES; ++w) r = op(r, scratch[w]);
  return r;
}
template <uint32_t WAVES, typename T, typename Op>
__device__ __forceinline__ T wg_reduce_all(T v, T* scratch, Op op, typename WaveSame<T>::type identity) {
  wg_put(v, scratch, op);
  __syncthreads();
  const T r = wg_get<WAVES>(scratch, op, identity);
  __syncthreads();
  return r;
}
template <uint32_t WAVES, typename T, typename Op>
__device__ __forceinline__ T wg_reduce_t0(T v, T* scratch, Op op, typename WaveSame<T>::type identity) {
  wg_put(v, scratch, op);
  __syncthreads();
  return threadIdx.x == 0u ? wg_get<WAVES>(scratch, op, identity) : identity;
}

// v = this thread's totals; exc = the sum of the totals of the threads in front of it, tot = the sum of all of them, for every thread
// (s_w: M * 4 doubles of LDS, free again on return). Every thread of a workgroup of 256 calls it.
template <uint32_t M>
__device__ __forceinline__ void wg_sum_scan(const double (&v)[M], double (&exc)[M], double (&tot)[M], double* s_w) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t m = 0; m < M; ++m) {
    const double inc = wave_scan(v[m]);
    if (lane == 63u) s_w[m * 4u + wave] = inc;
    const double e = __shfl_up(inc, 1);
    exc[m] = lane == 0u ? 0.0 : e;
  }
  __syncthreads();
#pragma unroll
  for (uint32_t m = 0; m < M; ++m) {
    const double* w = s_w + m * 4u;
    double woff = 0.0;
    for (uint32_t i = 0; i < wave; ++i) woff += w[i];
    exc[m] = woff + exc[m];
    tot[m] = ((w[0] + w[1]) + w[2]) + w[3];
  }
  __syncthreads();
}
