// Iterative projection core shared by proj_occlusion_kernel (matching.hip) and the fused refine tile kernel
// (refine.hip): one source for both, and both files are compiled with -ffp-contract=off -fno-slp-vectorize, so the two
// launches round every operation identically (p1 / valid are bit-identical between the fused and the unfused path).
//
// Reference semantics:
//   iter_proj_kernel                    backend/src/matching_kernels.cu:119-275
//   occlusion check                     matching.py:68-76
#pragma once
#include "m3s_half.hpp"

namespace m3s {

// torch.linalg.vector_norm / F.normalize of an fp32 3-vector in the reference's rounding: sqrt(fma(z, z, fma(y, y,
// x * x))) (pinned bit for bit against the reference run's golden rays / pts; oracle m3o_norm3)
__device__ __forceinline__ float norm3_ref(float x, float y, float z) {
  return sqrtf(__builtin_fmaf(z, z, __builtin_fmaf(y, y, x * x)));
}

// max of each of R runs of nparts prep partials (the refine screen's descriptor-norm bound; with the int8 screen also
// the max component and the max 1-norm) by one wave, every lane gets m[0..R)
// (R x 16 loads per lane in flight at once: one at a time, the 1024 partials of a 512x512 image were 16 dependent
// round trips in front of the wave's own pixels; the max is order-independent, NaN included, so every wave that
// reduces the same partials gets the same bits)
template <int R>
__device__ __forceinline__ void reduce_cnorm_wave(const float* __restrict__ part, int nparts, float* m) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int r = 0; r < R; r++) m[r] = 0.0f;
  for (int base = lane; base < nparts; base += 64 * 16) {
    float v[R][16];
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
      for (int k = 0; k < 16; k++) v[r][k] = part[(size_t)r * nparts + min(base + 64 * k, nparts - 1)];
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
      for (int k = 0; k < 16; k++) m[r] = fmaxf_nan(m[r], v[r][k]);
  }
#pragma unroll
  for (int r = 0; r < R; r++)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m[r] = fmaxf_nan(m[r], __shfl_xor(m[r], off, 64));
}

// ... into cmax[0], by the first wave of one block of the launch between prep and refine (proj_occlusion)
__device__ __forceinline__ void reduce_cnorm(const float* __restrict__ part, int nparts, float* __restrict__ cmax) {
  float m;
  reduce_cnorm_wave<1>(part, nparts, &m);
  if ((threadIdx.x & 63) == 0) *cmax = m;
}

// ------------------------------------------------------------------------------------------
// iter_proj core (matching_kernels.cu:139-273), one point per lane.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void bilin_w(float u, float v, int& u11, int& v11, float w[4]) {
  u11 = (int)floorf(u);
  v11 = (int)floorf(v);
  const float du = u - (float)u11;
  const float dv = v - (float)v11;
  // (1.0-du)*dv etc. are evaluated in double by the reference (:161-164). u, v >= 1 after clamping,
  // so du, dv are multiples of ulp(u) >= 2^-23 and 1-du, 1-dv are exact in float; the double
  // product of two exact floats is then rounded once to float — the same value as this float
  // product (no fp64 needed, bit-identical).
  const float cu = 1.0f - du, cv = 1.0f - dv;
  w[0] = du * dv;
  w[1] = cu * dv;
  w[2] = du * cv;
  w[3] = cu * cv;
}

// The four corners' 9 channels: channels 0..7 as four packed fp32 pairs (each element rounds as the scalar
// expression w0 r11 + w1 r12 + w2 r21 + w3 r22 does: -ffp-contract=off, no fma; the loads land in even-aligned
// register pairs and the weights broadcast by op_sel, so no moves), channel 8 scalar
__device__ __forceinline__ void bilin_sample9(const float* __restrict__ img, int W, int u11, int v11, const float w[4],
                                              float* out) {
  typedef float wf2 __attribute__((ext_vector_type(2)));
  // two 18-float runs, (v11, u11 .. u11 + 1) and the row below, from one 32-bit offset each (u11, v11 lie inside the
  // image and the launchers require 9 H W < 2^31): the corners are immediate offsets of the two run pointers
  const unsigned o = (unsigned)(v11 * W + u11) * 9u;
  const float* r22 = img + o;
  const float* r21 = r22 + 9;
  const float* r12 = img + (o + 9u * (unsigned)W);
  const float* r11 = r12 + 9;
  const wf2 w0 = {w[0], w[0]}, w1 = {w[1], w[1]}, w2 = {w[2], w[2]}, w3 = {w[3], w[3]};
  auto ld2 = [](const float* q) {
    wf2 r;
    r.x = q[0];
    r.y = q[1];
    return r;
  };
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    const wf2 o = w0 * ld2(r11 + j) + w1 * ld2(r12 + j) + w2 * ld2(r21 + j) + w3 * ld2(r22 + j);
    out[j] = o.x;
    out[j + 1] = o.y;
  }
  out[8] = w[0] * r11[8] + w[1] * r12[8] + w[2] * r21[8] + w[3] * r22[8];
}

// One LM iteration (matching_kernels.cu:185-270 loop body) on the carried state. LAST (the fused kernel's final
// iteration): the occlusion test's X11 gather at both possible final pixels, the accepted step's and the kept one's,
// is issued beside the iteration's own sample, so its round trip is not one more link after the loop; xo gets the
// one the accept / reject picks (matching.py:68-76 reads X11 at the final .long() pixel).
struct LmState {
  float u, v, lambda, cost, e0, e1, e2;
  float s[9];
  bool conv;
};

template <bool LAST>
__device__ __forceinline__ void lm_iter(LmState& m, const float* __restrict__ img, int H, int W, const float p[3],
                                        float cost_thresh, const float* __restrict__ X11b, float* xo) {
  const float* s = m.s;
  float A00 = s[3] * s[3] + s[4] * s[4] + s[5] * s[5];
  const float A01 = s[3] * s[6] + s[4] * s[7] + s[5] * s[8];
  float A11 = s[6] * s[6] + s[7] * s[7] + s[8] * s[8];
  const float b0 = -(m.e0 * s[3] + m.e1 * s[4] + m.e2 * s[5]);
  const float b1 = -(m.e0 * s[6] + m.e1 * s[7] + m.e2 * s[8]);
  A00 += m.lambda;
  A11 += m.lambda;
  const float det_inv = 1.0f / (A00 * A11 - A01 * A01);
  float u_new = m.u + det_inv * (A11 * b0 - A01 * b1);
  float v_new = m.v + det_inv * (-A01 * b0 + A00 * b1);
  u_new = fminf(fmaxf(u_new, 1.0f), (float)(W - 2));
  v_new = fminf(fmaxf(v_new, 1.0f), (float)(H - 2));
  float xa[3], xb[3];
  if constexpr (LAST) {
    const float* qa = X11b + ((size_t)(int)v_new * W + (int)u_new) * 3;  // .long() truncation; u, v >= 1
    const float* qb = X11b + ((size_t)(int)m.v * W + (int)m.u) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      xa[c] = qa[c];
      xb[c] = qb[c];
    }
  }
  int u11, v11;
  float w[4], t[9];
  bilin_w(u_new, v_new, u11, v11, w);
  bilin_sample9(img, W, u11, v11, w, t);
  const float r_norm_inv = 1.0f / sqrtf(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
  const float f0 = t[0] * r_norm_inv - p[0];
  const float f1 = t[1] * r_norm_inv - p[1];
  const float f2 = t[2] * r_norm_inv - p[2];
  const float new_cost = f0 * f0 + f1 * f1 + f2 * f2;
  if (new_cost < m.cost) {
    m.u = u_new;
    m.v = v_new;
#pragma unroll
    for (int k = 0; k < 9; k++) m.s[k] = t[k];
    m.e0 = f0;
    m.e1 = f1;
    m.e2 = f2;
    m.conv = new_cost < cost_thresh;
    m.cost = new_cost;
    m.lambda = (float)((double)m.lambda * 0.1);
    if constexpr (LAST) {
#pragma unroll
      for (int c = 0; c < 3; c++) xo[c] = xa[c];
    }
  } else {
    m.lambda = (float)((double)m.lambda * 10.0);
    m.conv = m.cost < cost_thresh;
    if constexpr (LAST) {
#pragma unroll
      for (int c = 0; c < 3; c++) xo[c] = xb[c];
    }
  }
}

// OCC: X11b non-null, xo gets X11 at the final (.long()) pixel, gathered during the last iteration (lm_iter<true>).
template <bool OCC>
__device__ __forceinline__ void iter_proj_point(const float* __restrict__ img, int H, int W, const float p[3],
                                                float& u, float& v, bool& conv, int max_iter, float lambda_init,
                                                float cost_thresh, const float* __restrict__ X11b = nullptr,
                                                float* xo = nullptr) {
  LmState m;
  m.u = fminf(fmaxf(u, 1.0f), (float)(W - 2));
  m.v = fminf(fmaxf(v, 1.0f), (float)(H - 2));
  m.lambda = lambda_init;
  m.conv = conv;
  // The reference samples (u, v) at the top of every iteration and (u_new, v_new) for the new cost.
  // The top-of-loop sample always equals the previous iteration's accepted sample (u_new) or its own
  // previous value (rejected), so the 9-channel sample is carried instead of refetched: one
  // dependent gather per iteration instead of two, identical values.
  int u11, v11;
  float w[4];
  if constexpr (OCC) {
    if (max_iter <= 0) {  // no iteration: the occlusion pixel is the clamped start, gathered beside its sample
      const float* q = X11b + ((size_t)(int)m.v * W + (int)m.u) * 3;
#pragma unroll
      for (int c = 0; c < 3; c++) xo[c] = q[c];
    }
  }
  bilin_w(m.u, m.v, u11, v11, w);
  bilin_sample9(img, W, u11, v11, w, m.s);
  // The residual e and cost of the carried sample are carried too: an accepted step's (f, new_cost)
  // are exactly what the next iteration would recompute from the same sample (bit-identical).
  // 1.0/r_norm in double then float == IEEE float division (53 >= 2*24+2, innocuous double rounding)
  const float r_norm_inv = 1.0f / sqrtf(m.s[0] * m.s[0] + m.s[1] * m.s[1] + m.s[2] * m.s[2]);
  m.e0 = m.s[0] * r_norm_inv - p[0];
  m.e1 = m.s[1] * r_norm_inv - p[1];
  m.e2 = m.s[2] * r_norm_inv - p[2];
  m.cost = m.e0 * m.e0 + m.e1 * m.e1 + m.e2 * m.e2;
  if constexpr (OCC) {
    for (int i = 0; i < max_iter - 1; i++) lm_iter<false>(m, img, H, W, p, cost_thresh, nullptr, nullptr);
    if (max_iter > 0) lm_iter<true>(m, img, H, W, p, cost_thresh, X11b, xo);
  } else {
    for (int i = 0; i < max_iter; i++) lm_iter<false>(m, img, H, W, p, cost_thresh, nullptr, nullptr);
  }
  u = m.u;
  v = m.v;
  conv = m.conv;
}

// lin_to_pixel (matching.py:18-22) with Python floor semantics for any i0 sign; 32-bit division for the indices
// inside [0, 2^31) (the same quotient and remainder)
__device__ __forceinline__ void lin_to_pixel_f(int64_t i0, int W, float& u, float& v) {
  if (i0 >= 0 && i0 <= 0x7fffffff) {
    const unsigned q = (unsigned)i0 / (unsigned)W;
    u = (float)((unsigned)i0 - q * (unsigned)W);
    v = (float)q;
    return;
  }
  int64_t vq = i0 / W, uq = i0 % W;
  if (uq < 0) {
    uq += W;
    vq -= 1;
  }
  u = (float)uq;
  v = (float)vq;
}

}  // namespace m3s
