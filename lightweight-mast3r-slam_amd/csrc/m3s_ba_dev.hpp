// Device helpers shared by the BA kernel files: ba.hip (linearisation), ba_sparse.hip and ba_dense.hip (the two
// solves of the pose system). Each translation unit compiles them under its own flags.
#pragma once
#include "m3s_common.hpp"
#include "m3s_ba.h"

#define BA_NSUM 36  // doubles per edge-sum / partial row: 28 of the upper 7x7 normal block, 7 of the gradient, 1 pad

namespace m3s {

// lanes of one wave exchanging data through LDS: a compiler memory barrier (the hardware returns a
// wave's LDS accesses in order)
__device__ __forceinline__ void wave_sync() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ double bcast_lane(double v, int src) {
  int2 x = *reinterpret_cast<int2*>(&v);
  x.x = __builtin_amdgcn_readlane(x.x, src);
  x.y = __builtin_amdgcn_readlane(x.y, src);
  return *reinterpret_cast<double*>(&x);
}

// 1/sqrt(d) for d > 0: the v_rsq_f64 estimate (~2^-22 relative) refined by ONE Newton step (~2^-44): the pivot
// chains are latency-bound (a dependent v_fma_f64 costs ~13 ns on gfx950, measured by scripts/micro/mfma_f64.hip),
// and 1e-13 relative pivots are far inside the 1e-5 pose contract (the LAPACK parity test bounds the solve at 2e-6
// of the step).
__device__ __forceinline__ double rsqrt_nr(double d) {
  const double y = __builtin_amdgcn_rsq(d);
  return fma(y, fma(-0.5 * d * y, y, 0.5), y);
}

// Assembly of the pose system: thread t of the block of item b (b < nL: factor block b, 49 elements; else rhs block
// row b - nL, 7 elements) owns element li of the 36 edge sums (the normal block is stored upper: index of (min, max)).
// False for a thread with no element.
__device__ __forceinline__ bool ba_asm_element(int b, int nL, int t, int* li) {
  if (b < nL) {
    const int rr = t / 7, cc = t - 7 * (t / 7);
    const int lo = min(rr, cc), hi = max(rr, cc);
    *li = lo * 7 - lo * (lo - 1) / 2 + (hi - lo);
    return t < 49;
  }
  *li = 28 + t;
  return t < 7;
}

// the inverse of ba_asm_element's map: (row, column), r <= c, of element t < 28 of the upper-stored 7x7 normal block
__device__ __forceinline__ void tri_rc(int t, int* r, int* c) {
  int row = 0;
  while (t >= 7 - row) {
    t -= 7 - row;
    row++;
  }
  *r = row;
  *c = row + t;
}

// that element: the contributions of the plan's CSR row of item b, added strictly in CSR order (deterministic:
// identical on every rank and in both solves); the indices and values of 4 entries in flight at a time
__device__ __forceinline__ double ba_asm_sum(const BaArgs& a, int b, int nL, int li) {
  const int* ptr = b < nL ? a.asm_ptr + b : a.rhs_ptr + (b - nL);
  const int* ent = b < nL ? a.asm_ent : a.rhs_ent;
  double s = 0.0;
  const int kb = ptr[0], ke = ptr[1];
  int k = kb;
  for (; k + 4 <= ke; k += 4) {
    int e[4];
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) e[u] = ent[k + u];
#pragma unroll
    for (int u = 0; u < 4; u++) v[u] = a.edge_sums[(size_t)(e[u] >> 1) * BA_NSUM + li];
#pragma unroll
    for (int u = 0; u < 4; u++) s += ((e[u] & 1) ? -1.0 : 1.0) * v[u];
  }
  for (; k < ke; k++) {
    const int e = ent[k];
    s += ((e & 1) ? -1.0 : 1.0) * a.edge_sums[(size_t)(e >> 1) * BA_NSUM + li];
  }
  return s;
}

// The tail of a solve, run by every thread of its one-workgroup kernel (any multiple of 64 threads up to 1024; the
// thread count fixes the order of the |dx| sum): dx = -x in pose order (0 when the factorisation failed: the
// reference's silent zero step), the Sim(3) retraction of the poses k >= 1, the |dx| early exit and the iteration
// count. x holds XS doubles per column, 7 used. stalled (a bounded wait timed out) is sticky until the next plan:
// the loop ends and the host reports M3S_ESTALL. *a.info is left to the caller.
template <int XS>
__device__ __forceinline__ void ba_finish_step(const BaArgs& a, const double* x, int K, float delta_thresh,
                                               bool failed, bool stalled) {
  __shared__ float s_n2[1024 / 64];
  const int n = a.nb * 7;
  float n2 = 0.0f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int j = i / 7, m = i - 7 * (i / 7);
    const float d = failed ? 0.0f : (float)(-x[(size_t)j * XS + m]);
    a.dx[a.perm[j] * 7 + m] = d;
    n2 += d * d;
  }
  __syncthreads();
  for (int k = 1 + threadIdx.x; k < K; k += blockDim.x) {
    float Tw[8], xi[7];
    for (int c = 0; c < 8; c++) Tw[c] = a.Twc[k * 8 + c];
    for (int c = 0; c < 7; c++) xi[c] = a.dx[(k - 1) * 7 + c];
    retrSim3_d(xi, Tw);  // fp64 retraction (m3s_common.hpp: fp32 expSim3 cancels for small steps)
    for (int c = 0; c < 8; c++) a.Twc[k * 8 + c] = Tw[c];
  }
  n2 = wave_sum(n2);
  if ((threadIdx.x & 63) == 0) s_n2[threadIdx.x >> 6] = n2;
  __syncthreads();
  if (threadIdx.x == 0) {
    float sum = 0.0f;
    for (int q = 0; q < (int)blockDim.x / 64; q++) sum += s_n2[q];
    *a.iters += 1;
    if (sqrtf(sum) < delta_thresh) *a.done = 1;
    if (stalled) {
      *a.stalled = 1;
      *a.done = 1;
    }
  }
}

}  // namespace m3s
