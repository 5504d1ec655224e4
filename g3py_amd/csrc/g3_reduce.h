// Block reductions whose summation order is part of the library's contract (device functions only).  The four scalars of a
// log-likelihood and the diagonal statistics are computed by several kernels (g3_api.hip, g3_potrf.hip, g3_drawsb.hip) that
// must agree bit for bit: a chain member gives the bits of the single evaluation.  The order is defined here, once:
// a thread's own elements in its kernel's loop, wave_* over the 64 lanes, then the waves' partials in the order 0, 1, 2, ...
#pragma once
#include <hip/hip_runtime.h>

// wave reductions in a fixed order (lane 0 holds the result); min / max propagate NaN like numpy
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    T u = __shfl_down(v, o, 64);
    v = (u < v || u != u) ? u : v;  // NaN propagates like numpy.min
  }
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    T u = __shfl_down(v, o, 64);
    v = (u > v || u != u) ? u : v;
  }
  return v;
}

// the partials of NW waves (lane 0's wave_* results, in LDS) combined by ONE thread, wave 0 first
template <int NW>
__device__ __forceinline__ double waves_sum(const double* s) {
  double t = 0.0;
  for (int w = 0; w < NW; ++w) t += s[w];
  return t;
}
template <int NW>
__device__ __forceinline__ double waves_min(const double* s) {
  double t = s[0];
  for (int w = 0; w < NW; ++w) t = (s[w] < t || s[w] != s[w]) ? s[w] : t;
  return t;
}
template <int NW>
__device__ __forceinline__ double waves_max(const double* s) {
  double t = s[0];
  for (int w = 0; w < NW; ++w) t = (s[w] > t || s[w] != s[w]) ? s[w] : t;
  return t;
}

// ---- the four scalars of a log-likelihood: sum log L_ii, a^T a, #non-finite a, #bad diagonal entries
struct LogpTerms {
  double ld_sum = 0, ss = 0, nf = 0, bd = 0;
  __device__ __forceinline__ void diag(double d) {     // one diagonal entry of the factor
    ld_sum += log(d);
    if (!(d > 0.0) || __builtin_isinf(d)) bd += 1;
  }
  __device__ __forceinline__ void rhs(double v) {      // one entry of a = L^-1 delta
    ss += v * v;
    if (v != v || __builtin_isinf(v)) nf += 1;
  }
  // Across the NW waves of the workgroup (every thread calls it): red[k][w] = wave w's partial of scalar k, behind a barrier.
  // Scalar k of the block is then waves_sum<NW>(red[k]), on whichever thread the kernel gives it to.
  template <int NW>
  __device__ __forceinline__ void to_waves(double (*red)[NW], int lane, int wave) {
    ld_sum = wave_sum(ld_sum); ss = wave_sum(ss); nf = wave_sum(nf); bd = wave_sum(bd);
    if (lane == 0) { red[0][wave] = ld_sum; red[1][wave] = ss; red[2][wave] = nf; red[3][wave] = bd; }
    __syncthreads();
  }
};
