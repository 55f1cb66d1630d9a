// Shared helpers of the evaluation kernels (sr_pose_eval, sr_cloud_eval, sr_depth_eval, sr_sort, sr_cloud_voxel,
// sr_sparsify, sr_cloud_render, sr_two_view): the tests on exponent bits, the fixed reduction tree, the scan and the histogram
// slot that their contracts define "to the bit", once.  Included after sr_common.h by those eight files only.
//
// Header code is compiled under the including object's flags, so every object keeps the semantics it had with its
// own copy: sr_cloud_voxel.o, sr_sparsify.o, sr_cloud_render.o and sr_two_view.o are built with -ffp-contract=off -fhonor-nans
// (the tests on the exponent bits must see NaNs there, and sr::xform_point must stay unfused), the others as they
// always were (Makefile).
#pragma once

#include <string.h>

#include "sr_common.h"

namespace sr {

// ---------------------------------------------------------------- bit patterns and tests on them
constexpr uint32_t QNAN_BITS = 0x7fc00000u;  // the quiet NaN every "no value" output holds
constexpr uint32_t PINF_BITS = 0x7f800000u;

__device__ inline float quiet_nan() { return __uint_as_float(QNAN_BITS); }
__device__ inline float pos_inf() { return __uint_as_float(PINF_BITS); }

// on the bits of an fp32 value; the float overloads forward through __float_as_uint
__device__ inline bool bits_nonfinite(uint32_t b) { return (b & 0x7f800000u) == 0x7f800000u; }
__device__ inline bool bits_finite(uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; }
__device__ inline bool bits_nan(uint32_t b) { return (b & 0x7fffffffu) > 0x7f800000u; }
__device__ inline bool bits_positive_finite(uint32_t b) { return b > 0u && b < 0x7f800000u; }
__device__ inline bool bits_nonfinite(float x) { return bits_nonfinite(__float_as_uint(x)); }
__device__ inline bool bits_finite(float x) { return bits_finite(__float_as_uint(x)); }
__device__ inline bool bits_nan(float x) { return bits_nan(__float_as_uint(x)); }
__device__ inline bool bits_positive_finite(float x) { return bits_positive_finite(__float_as_uint(x)); }
__device__ inline bool bits_nonfinite64(double x) {
  return ((uint64_t)__double_as_longlong(x) & 0x7ff0000000000000ull) == 0x7ff0000000000000ull;
}

// the same on the host, through memcpy (host code is built with -fno-honor-nans too)
inline bool positive_finite(float x) {
  uint32_t u;
  memcpy(&u, &x, sizeof(u));
  return u > 0u && u < 0x7f800000u;
}
inline bool is_nan(float x) {
  uint32_t u;
  memcpy(&u, &x, sizeof(u));
  return (u & 0x7fffffffu) > 0x7f800000u;
}
inline bool finite64(double x) {
  uint64_t u;
  memcpy(&u, &x, sizeof(u));
  return (u & 0x7fffffffffffffffull) < 0x7ff0000000000000ull;
}

inline int64_t align16(int64_t b) { return (b + 15) & ~int64_t(15); }

// order-preserving key of an fp32 bit pattern and its inverse: ascending key is ascending value, -0 before +0
__device__ inline uint32_t key32(uint32_t b) { return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ inline uint32_t unkey32(uint32_t k) { return (k >> 31) ? (k ^ 0x80000000u) : ~k; }

// histogram slot of a finite, non-negative value: k <= fl32(x / len) < k + 1, the rest in n_bins; always in [0, n_bins]
__device__ inline int hist_slot(float x, float len, int n_bins) {
  const float q = __fdiv_rn(x, len);
  if (!(q < (float)n_bins)) return n_bins;
  return min(max((int)q, 0), n_bins);
}

// ---------------------------------------------------------------- workgroup reduction, scan, LDS histogram
// Sums of NV fp64 values over a workgroup of T threads in a fixed tree (smem: NV * T doubles), the last entry a
// maximum instead if LAST_MAX; the results in every thread.  The leading barrier lets smem be reused at once.
template <int T, int NV, bool LAST_MAX = false>
__device__ inline void block_reduce(double (&v)[NV], double* smem) {
  const int t = threadIdx.x;
  __syncthreads();
#pragma unroll
  for (int e = 0; e < NV; ++e) smem[e * T + t] = v[e];
  __syncthreads();
  for (int s = T / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int e = 0; e < NV; ++e) {
        const double o = smem[e * T + t + s];
        if (LAST_MAX && e == NV - 1) {
          if (o > smem[e * T + t]) smem[e * T + t] = o;
        } else {
          smem[e * T + t] += o;
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < NV; ++e) v[e] = smem[e * T];
}

// Exclusive scan of one value per thread over a workgroup of T threads (Hillis-Steele in smem[T]); the total in
// every thread's `total`.
template <int T>
__device__ inline uint32_t block_exclusive(uint32_t v, uint32_t* smem, uint32_t& total) {
  const int t = threadIdx.x;
  __syncthreads();
  smem[t] = v;
  __syncthreads();
  for (int off = 1; off < T; off <<= 1) {
    const uint32_t o = t >= off ? smem[t - off] : 0u;
    __syncthreads();
    smem[t] += o;
    __syncthreads();
  }
  total = smem[T - 1];
  return smem[t] - v;
}

// Exclusive scan of a row of n values by one workgroup, in chunks of 4 T: four values per lane, a scan of the
// lanes' sums, the carry to the next chunk in a register.  store(e, x) gets carry + the sum of load(0 .. e - 1);
// returns carry + the row's total, in every thread.  load and store may name the same memory (an element is read
// and written by the same lane).
template <int T, typename Index, typename Load, typename Store>
__device__ inline uint32_t scan_row(Index n, uint32_t carry, uint32_t* smem, Load load, Store store) {
  const int t = threadIdx.x;
  for (Index c0 = 0; c0 < n; c0 += 4 * T) {
    const Index e0 = c0 + 4 * t;
    uint32_t v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = e0 + u < n ? load(e0 + u) : 0u;
    uint32_t total;
    uint32_t run = carry + block_exclusive<T>(v[0] + v[1] + v[2] + v[3], smem, total);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (e0 + u < n) store(e0 + u, run);
      run += v[u];
    }
    carry += total;
  }
  return carry;
}

// An LDS histogram of n slots: cleared, and its non-zero slots added to a global one with one integer atomic each
// (the caller puts the barriers between the clear, its own adds and the flush)
template <int T>
__device__ inline void hist_clear(uint32_t* s_hist, int n) {
  for (int e = threadIdx.x; e < n; e += T) s_hist[e] = 0;
}
template <int T>
__device__ inline void hist_flush(const uint32_t* s_hist, uint32_t* hist, int n) {
  for (int e = threadIdx.x; e < n; e += T) {
    const uint32_t v = s_hist[e];
    if (v) atomicAdd(&hist[e], v);
  }
}

// ---------------------------------------------------------------- points
// fl32(s (R p) + t) from the fp32 point and the fp64 [13] = scale, R row-major, t: fp64, left to right, rounded
// to fp32 once.  The one transform of sr_cloud_nn, sr_cloud_voxel and sr_cloud_render.  __dmul_rn / __dadd_rn are
// plain * and + in the HIP headers, so whether they stay unfused is the including object's -ffp-contract:
// sr_cloud_voxel.o and sr_cloud_render.o are built with it off (bit for bit what numpy computes), sr_cloud_eval.o
// as it always was.
__device__ inline void xform_point(const double* __restrict__ x, float& px, float& py, float& pz) {
  const double a = (double)px, b = (double)py, c = (double)pz;
  float o[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double rp = __dadd_rn(__dadd_rn(__dmul_rn(x[1 + 3 * r], a), __dmul_rn(x[2 + 3 * r], b)), __dmul_rn(x[3 + 3 * r], c));
    o[r] = (float)__dadd_rn(__dmul_rn(x[0], rp), x[10 + r]);
  }
  px = o[0], py = o[1], pz = o[2];
}

// the point at p, transformed if xform is given; true if it is non-finite before or after
__device__ inline bool load_point(const float* __restrict__ p, const double* __restrict__ xform, float& x, float& y, float& z) {
  x = p[0], y = p[1], z = p[2];
  bool bad = bits_nonfinite(x) || bits_nonfinite(y) || bits_nonfinite(z);
  if (xform) {
    xform_point(xform, x, y, z);
    bad = bad || bits_nonfinite(x) || bits_nonfinite(y) || bits_nonfinite(z);
  }
  return bad;
}

}  // namespace sr

// The two checks every entry point with a workspace makes, under its own name: the size, then the alignment.
#define SR_CHECK_WORKSPACE(name, ptr, bytes, need)                                                                  \
  do {                                                                                                              \
    SR_CHECK((bytes) >= (need), SR_EINVAL, name ": workspace of %lld bytes, %lld needed", (long long)(bytes),       \
             (long long)(need));                                                                                    \
    SR_CHECK(((uintptr_t)(ptr) & 15) == 0, SR_EINVAL, name ": the workspace must be 16-byte aligned");              \
  } while (0)
