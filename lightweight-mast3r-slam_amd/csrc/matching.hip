// Dense projective matching for MI355X (gfx950): prep (ray image + gradients), iterative
// projection (LM over a bilinear ray image), occlusion test and coarse-to-fine descriptor refine.
//
// Reference semantics:
//   prep_for_iter_proj + img_gradient   /root/reference/mast3r_slam/matching.py:25-49, image.py:5-38
//   iter_proj_kernel                    backend/src/matching_kernels.cu:119-275
//   occlusion check                     matching.py:68-76
//   refine_matches_kernel (c10::Half)   backend/src/matching_kernels.cu:25-81
//   pixel_to_lin                        matching.py:13-15
//
// This file is compiled with -ffp-contract=off: the refine score must round every half product and
// every half add separately (c10::Half operator* / operator+), which a contracted v_fma_f16 breaks.
#include "m3s_proj.hpp"
#include "m3s_match.h"

namespace m3s {

// Refine tile path: D11 (B,H,W,24) f32 -> f16 (RNE, == torch .half()) of pixel n into image b's three chunk planes
// (H,W,8) (one 16-B store per plane: lanes store consecutive pixels); returns the sum of squares of its f16 values
// (the refine screen's norm bound, refine.hip; 0 past the image). The loads are split from the conversion so the
// prep kernel issues them first, under the ray halo's loads and stencil (desc_load, then desc_planar).
// (unconditional: a pixel past the image loads pixel N - 1 and stores nothing, so no branch join waits on the loads)
__device__ __forceinline__ void desc_load(const float* __restrict__ D11, int b, int n, int N, float4 v[6]) {
  const float4* src = reinterpret_cast<const float4*>(D11 + ((size_t)b * N + min(n, N - 1)) * 24);
#pragma unroll
  for (int k = 0; k < 6; k++) v[k] = src[k];
}

// Q8: also the int8 copy for the refine screen's levels d >= 2 (refine.hip ScreenI8), quantised from the f16
// value so a host restatement is exact: c8 = clamp(rint(127 c_h), -127, 127) (127 c_h is exact in fp32, rint is RNE).
// Per image two planes: channels 0..15 as (H,W,16) bytes, then channels 16..23 as (H,W,8) bytes, so a window row
// of either plane is one contiguous run for 16-byte LDS DMA. amax / c1: the pixel's max |c_h,k| and sum |c_h,k|
// (the int8 bound's inputs; NaN-propagating like the norm).
template <bool Q8>
__device__ __forceinline__ float desc_planar(const float4 v[6], h1* __restrict__ D11h, signed char* __restrict__ D8,
                                             int b, int n, int N, float& amax, float& c1) {
  float ss = 0.0f;
  amax = c1 = 0.0f;
  if (n < N) {
    const size_t plane = (size_t)N * 8;
    h1* dst = D11h + (size_t)b * 3 * plane + (size_t)n * 8;
    unsigned w8[6];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float4 v0 = v[2 * c], v1 = v[2 * c + 1];
      h1 r[8] = {(h1)v0.x, (h1)v0.y, (h1)v0.z, (h1)v0.w, (h1)v1.x, (h1)v1.y, (h1)v1.z, (h1)v1.w};
      *reinterpret_cast<uint4*>(dst + c * plane) = *reinterpret_cast<uint4*>(r);
#pragma unroll
      for (int k = 0; k < 8; k++) ss += (float)r[k] * (float)r[k];
      if constexpr (Q8) {
        w8[2 * c] = w8[2 * c + 1] = 0u;
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const float x = (float)r[k];
          amax = fmaxf_nan(amax, fabsf(x));
          c1 += fabsf(x);
          const int qi = (int)rintf(fminf(fmaxf(127.0f * x, -127.0f), 127.0f));
          w8[2 * c + (k >> 2)] |= (unsigned)(qi & 0xff) << (8 * (k & 3));
        }
      }
    }
    if constexpr (Q8) {
      signed char* d8 = D8 + (size_t)b * N * 24;
      *reinterpret_cast<uint4*>(d8 + (size_t)n * 16) = uint4{w8[0], w8[1], w8[2], w8[3]};
      *reinterpret_cast<uint2*>(d8 + (size_t)N * 16 + (size_t)n * 8) = uint2{w8[4], w8[5]};
    }
  }
  return ss;
}

// ------------------------------------------------------------------------------------------
// prep: rays = X/max(|X|,1e-12); gx, gy = Scharr/32 with reflect padding; out (B,H,W,9).
// One 16x16 tile per 256-thread block, normalised rays of an 18x18 halo staged in LDS.
// Also converts D11 (B,H,W,F) f32 -> f16 (RNE, == torch .half()) for the same pixels: planar (refine tile path, one
// pixel per thread) with the tile's descriptor-norm partial max |D11h[pixel]|_2 into cnorm_part (nullable), else in
// the (B,H,W,F) layout of the per-pixel refine kernels.
// ------------------------------------------------------------------------------------------
#define PREP_T 16
// DMODE: 0 no descriptors, 1 planar (refine tile path), 2 the (B,H,W,F) row layout, 3 planar plus the int8 screen copy
// D8 and its two bound partials (cnorm_part then holds three runs of one float per block: max |c|_2, max |c_k|,
// max |c|_1); a template argument so the planar path's descriptor loads, issued first, cross no branch join (a
// runtime `if` made the compiler convert them, and so wait for them, right behind the loads)
template <int DMODE>
__global__ void __launch_bounds__(256) prep_rays_kernel(const float* __restrict__ X11, float* __restrict__ rays9,
                                                        const float* __restrict__ D11, h1* __restrict__ D11h, int H,
                                                        int W, int F, float* __restrict__ cnorm_part,
                                                        signed char* __restrict__ D8) {
  __shared__ float tile[(PREP_T + 2) * (PREP_T + 2) * 3];
  const int b = blockIdx.z;
  const int u0 = blockIdx.x * PREP_T, v0 = blockIdx.y * PREP_T;
  const float* Xb = X11 + (size_t)b * H * W * 3;
  const int lx = threadIdx.x % PREP_T, ly = threadIdx.x / PREP_T;
  const int x = u0 + lx, y = v0 + ly;
  constexpr bool planar_d = DMODE == 1 || DMODE == 3, q8 = DMODE == 3;
  const int dn = (x < W && y < H) ? y * W + x : H * W;
  // the 18x18 halo: 324 pixels, two per thread at most (256 threads); both loads issued before either is used
  constexpr int HALO = (PREP_T + 2) * (PREP_T + 2);
  static_assert(HALO <= 2 * 256, "prep halo: two pixels per thread");
  float hv[2][3];
#pragma unroll
  for (int r = 0; r < 2; r++) {
    const int t = min((int)threadIdx.x + 256 * r, HALO - 1);
    const int hy = t / (PREP_T + 2), hx = t % (PREP_T + 2);
    int yy = v0 + hy - 1, xx = u0 + hx - 1;
    // reflect padding (F.pad mode="reflect"): -1 -> 1, H -> H-2
    yy = yy < 0 ? -yy : (yy >= H ? 2 * H - 2 - yy : yy);
    xx = xx < 0 ? -xx : (xx >= W ? 2 * W - 2 - xx : xx);
    yy = min(max(yy, 0), H - 1);
    xx = min(max(xx, 0), W - 1);
    const float* p = Xb + ((size_t)yy * W + xx) * 3;
    hv[r][0] = p[0];
    hv[r][1] = p[1];
    hv[r][2] = p[2];
  }
  // then the pixel's descriptor loads (vmcnt retires in order: behind the halo's, so the stencil waits only for those)
  float4 dv[6];
  if constexpr (planar_d) desc_load(D11, b, dn, H * W, dv);
#pragma unroll
  for (int r = 0; r < 2; r++) {
    const int t = threadIdx.x + 256 * r;
    if (t < HALO) {
      const float a = hv[r][0], c = hv[r][1], d = hv[r][2];
      const float n = fmaxf(norm3_ref(a, c, d), 1e-12f);
      tile[t * 3 + 0] = a / n;
      tile[t * 3 + 1] = c / n;
      tile[t * 3 + 2] = d / n;
    }
  }
  __syncthreads();
  if (x < W && y < H) {
    float* o = rays9 + (((size_t)b * H + y) * W + x) * 9;
#define T3(dy, dx, c) tile[(((ly + 1 + (dy)) * (PREP_T + 2)) + (lx + 1 + (dx))) * 3 + (c)]
#pragma unroll
    for (int c = 0; c < 3; c++) {
      o[c] = T3(0, 0, c);
      // gx kernel (1/32)[[-3,0,3],[-10,0,10],[-3,0,3]]; gy its transpose (image.py:10-24), in the reference's
      // depthwise conv2d order: a row-major FMA chain over all 9 taps, zero taps included (bit-exact against the
      // reference run's rays: tests/golden/matching_48x64.npz, oracle m3o_img_gradient)
      const float t00 = T3(-1, -1, c), t01 = T3(-1, 0, c), t02 = T3(-1, 1, c), t10 = T3(0, -1, c), t11 = T3(0, 0, c),
                  t12 = T3(0, 1, c), t20 = T3(1, -1, c), t21 = T3(1, 0, c), t22 = T3(1, 1, c);
      float gx = -0.09375f * t00;
      gx = __builtin_fmaf(0.0f, t01, gx);
      gx = __builtin_fmaf(0.09375f, t02, gx);
      gx = __builtin_fmaf(-0.3125f, t10, gx);
      gx = __builtin_fmaf(0.0f, t11, gx);
      gx = __builtin_fmaf(0.3125f, t12, gx);
      gx = __builtin_fmaf(-0.09375f, t20, gx);
      gx = __builtin_fmaf(0.0f, t21, gx);
      gx = __builtin_fmaf(0.09375f, t22, gx);
      float gy = -0.09375f * t00;
      gy = __builtin_fmaf(-0.3125f, t01, gy);
      gy = __builtin_fmaf(-0.09375f, t02, gy);
      gy = __builtin_fmaf(0.0f, t10, gy);
      gy = __builtin_fmaf(0.0f, t11, gy);
      gy = __builtin_fmaf(0.0f, t12, gy);
      gy = __builtin_fmaf(0.09375f, t20, gy);
      gy = __builtin_fmaf(0.3125f, t21, gy);
      gy = __builtin_fmaf(0.09375f, t22, gy);
      o[3 + c] = gx;
      o[6 + c] = gy;
    }
#undef T3
  }
  if constexpr (planar_d) {
    float amax, c1;
    const float ss = desc_planar<q8>(dv, D11h, D8, b, dn, H * W, amax, c1);
    if (cnorm_part != nullptr) {
      // the tile's max |D11h[pixel]|_2, one partial per block (every block of the fused refine launch reduces them
      // itself; on the three-launch path proj_occlusion does, before refine reads the bound); NaN / inf descriptors give a NaN / inf partial, which switches the screen off for every lane
      constexpr int NP = q8 ? 3 : 1;
      __shared__ float s_max[NP][4];
      float pm[3] = {sqrtf(ss), amax, c1};
#pragma unroll
      for (int p = 0; p < NP; p++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) pm[p] = fmaxf_nan(pm[p], __shfl_xor(pm[p], off, 64));
        if ((threadIdx.x & 63) == 0) s_max[p][threadIdx.x >> 6] = pm[p];
      }
      __syncthreads();
      if (threadIdx.x < NP) {
        const int p = threadIdx.x;
        const size_t nparts = (size_t)gridDim.x * gridDim.y * gridDim.z;
        cnorm_part[p * nparts + ((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] =
            fmaxf_nan(fmaxf_nan(s_max[p][0], s_max[p][1]), fmaxf_nan(s_max[p][2], s_max[p][3]));
      }
    }
  } else if constexpr (DMODE == 2) {
    // f32 -> f16 of this tile's descriptor rows (B,H,W,F), 4 channels per lane-step (the per-pixel kernels'
    // layout; the refine tile path's planar layout is written by the proj launch, desc_planar above)
    for (int t = threadIdx.x; t < PREP_T * PREP_T * (F / 4); t += blockDim.x) {
      const int pix = t / (F / 4), q = t % (F / 4);
      const int xx = u0 + pix % PREP_T, yy = v0 + pix / PREP_T;
      if (xx < W && yy < H) {
        const size_t off = (((size_t)b * H + yy) * W + xx) * F + q * 4;
        const float4 v = *reinterpret_cast<const float4*>(D11 + off);
        h1 r[4] = {(h1)v.x, (h1)v.y, (h1)v.z, (h1)v.w};
        *reinterpret_cast<uint2*>(D11h + off) = *reinterpret_cast<uint2*>(r);
      }
    }
  }
}

// (reduce_cnorm, the iter_proj core and lin_to_pixel_f: m3s_proj.hpp, shared with the fused refine tile kernel)

// Reference-signature kernel: rays (B,H,W,9), pts (B,N,3) normalised, p_init (B,N,2) f32.
__global__ void __launch_bounds__(256) iter_proj_kernel(const float* __restrict__ rays, const float* __restrict__ pts,
                                                        const float* __restrict__ p_init, float* __restrict__ p_new,
                                                        uint8_t* __restrict__ converged, int H, int W, int N,
                                                        int max_iter, float lambda_init, float cost_thresh) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (n >= N) return;
  const size_t bn = (size_t)b * N + n;
  const float p[3] = {pts[bn * 3 + 0], pts[bn * 3 + 1], pts[bn * 3 + 2]};
  float u = p_init[bn * 2 + 0], v = p_init[bn * 2 + 1];
  bool conv = false;
  iter_proj_point<false>(rays + (size_t)b * H * W * 9, H, W, p, u, v, conv, max_iter, lambda_init, cost_thresh);
  p_new[bn * 2 + 0] = u;
  p_new[bn * 2 + 1] = v;
  converged[bn] = conv;
}

// Fused: normalise X21 on the fly, p_init from idx_init (or identity), LM projection, .long()
// truncation, occlusion test against raw X11 (matching.py:68-76). Writes p1 (B,N,2) int32 and
// valid (B,N) u8.
__global__ void __launch_bounds__(256) proj_occlusion_kernel(
    const float* __restrict__ rays, const float* __restrict__ X11, const float* __restrict__ X21,
    const int64_t* __restrict__ idx_init, int* __restrict__ p1, uint8_t* __restrict__ valid, int H, int W,
    int max_iter, float lambda_init, float cost_thresh, float dist_thresh, const float* __restrict__ cnorm_part,
    int nparts, float* __restrict__ cmax, int nruns) {
  const int N = H * W;
  if (cmax != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 64)
    for (int r = 0; r < nruns; r++) reduce_cnorm(cnorm_part + (size_t)r * nparts, nparts, cmax + r);
  // contiguous pixel runs per XCD: each XCD's L2 then holds the rays rows its LM gathers touch
  const int n = xcd_remap(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (n >= N) return;
  const size_t bn = (size_t)b * N + n;
  const float x = X21[bn * 3 + 0], y = X21[bn * 3 + 1], z = X21[bn * 3 + 2];
  const float nrm = fmaxf(norm3_ref(x, y, z), 1e-12f);  // F.normalize (matching.py:44)
  const float p[3] = {x / nrm, y / nrm, z / nrm};
  float u, v;
  lin_to_pixel_f(idx_init != nullptr ? idx_init[bn] : (int64_t)n, W, u, v);
  bool conv = false;
  float Xg[3];  // X11 at the final pixel, gathered during the last LM iteration
  iter_proj_point<true>(rays + (size_t)b * H * W * 9, H, W, p, u, v, conv, max_iter, lambda_init, cost_thresh,
                        X11 + (size_t)b * H * W * 3, Xg);
  const int pu = (int)u, pv = (int)v;  // .long() truncation; u,v >= 1 after clamping
  const float dx = Xg[0] - x, dy = Xg[1] - y, dz = Xg[2] - z;
  const float d = norm3_ref(dx, dy, dz);  // torch.linalg.norm (matching.py:71-73)
  p1[bn * 2 + 0] = pu;
  p1[bn * 2 + 1] = pv;
  valid[bn] = conv && (d < dist_thresh);
}

// ------------------------------------------------------------------------------------------
// refine (matching_kernels.cu:36-80) with c10::Half step rounding: each product and each
// partial sum rounds to binary16 (v_pk_mul_f16 / v_add_f16 are correctly rounded, == Half ops).
// ------------------------------------------------------------------------------------------
template <int F>
__device__ __forceinline__ h1 score_f16(const h2* q, const h1* __restrict__ c) {
  h2 cv[F / 2];
  const uint4* c4 = reinterpret_cast<const uint4*>(c);
#pragma unroll
  for (int k = 0; k < F / 8; k++) {
    const uint4 t = c4[k];
    cv[4 * k + 0] = *reinterpret_cast<const h2*>(&t.x);
    cv[4 * k + 1] = *reinterpret_cast<const h2*>(&t.y);
    cv[4 * k + 2] = *reinterpret_cast<const h2*>(&t.z);
    cv[4 * k + 3] = *reinterpret_cast<const h2*>(&t.w);
  }
  h1 s = (h1)0.0f;
#pragma unroll
  for (int k = 0; k < F / 2; k++) {
    const h2 pr = q[k] * cv[k];
    s = s + pr.x;
    s = s + pr.y;
  }
  return s;
}

// The levels of one query: score(pix) is candidate pixel pix's score, start the running max's first value, the
// reference's numeric_limits<scalar_t>::min()
template <class S, class Score>
__device__ __forceinline__ void refine_point(int H, int W, int radius, int dilation_max, S start, int& u0, int& v0,
                                             Score score) {
  S max_score = start;
  int u_new = u0, v_new = v0;
  for (int d = dilation_max; d > 0; d--) {
    const int rd = radius * d;
    const int diam = 2 * rd + 1;
    for (int i = 0; i < diam; i += d) {
      const int u = u0 - rd + i;
      for (int j = 0; j < diam; j += d) {
        const int v = v0 - rd + j;
        if (v >= 0 && v < H && u >= 0 && u < W) {
          const S s = score((size_t)v * W + u);
          if (s > max_score) {
            max_score = s;
            u_new = u;
            v_new = v;
          }
        }
      }
    }
    u0 = u_new;
    v0 = v_new;
  }
}
// ... with the c10::Half score; the start value is numeric_limits<c10::Half>::min() == Half() == +0
template <int F>
__device__ __forceinline__ void refine_point_f16(const h1* __restrict__ img, int H, int W, const h2* q, int radius,
                                                 int dilation_max, int& u0, int& v0) {
  refine_point(H, W, radius, dilation_max, (h1)0.0f, u0, v0,
               [&](size_t pix) { return score_f16<F>(q, img + pix * F); });
}

// Reference signature: D11 (B,H,W,F) f16, D21 (B,N,F) f16, p1 (B,N,2) i64 -> p1_new (B,N,2) i64.
template <int F>
__global__ void __launch_bounds__(256) refine_f16_kernel(const h1* __restrict__ D11, const h1* __restrict__ D21,
                                                         const int64_t* __restrict__ p1, int64_t* __restrict__ p1_new,
                                                         int H, int W, int N, int radius, int dilation_max) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (n >= N) return;
  const size_t bn = (size_t)b * N + n;
  h2 q[F / 2];
  load_query<F, false>(D21, bn, q);
  int u0 = (int)p1[bn * 2 + 0], v0 = (int)p1[bn * 2 + 1];
  refine_point_f16<F>(D11 + (size_t)b * H * W * F, H, W, q, radius, dilation_max, u0, v0);
  p1_new[bn * 2 + 0] = u0;
  p1_new[bn * 2 + 1] = v0;
}

// Fused tail: D21 f32 converted in-register, p1 int32 from proj_occlusion, writes idx = u + W*v.
template <int F>
__global__ void __launch_bounds__(256) refine_lin_kernel(const h1* __restrict__ D11h, const float* __restrict__ D21,
                                                         const int* __restrict__ p1, int64_t* __restrict__ idx_out,
                                                         int H, int W, int radius, int dilation_max) {
  const int N = H * W;
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (n >= N) return;
  const size_t bn = (size_t)b * N + n;
  h2 q[F / 2];
  load_query<F, true>(D21, bn, q);
  int u0 = p1[bn * 2 + 0], v0 = p1[bn * 2 + 1];
  refine_point_f16<F>(D11h + (size_t)b * H * W * F, H, W, q, radius, dilation_max, u0, v0);
  idx_out[bn] = (int64_t)u0 + (int64_t)W * v0;
}

// fp32 instantiation of the reference kernel (AT_DISPATCH float): fp32 MACs, max starts at FLT_MIN.
__global__ void __launch_bounds__(256) refine_f32_kernel(const float* __restrict__ D11, const float* __restrict__ D21,
                                                         const int64_t* __restrict__ p1, int64_t* __restrict__ p1_new,
                                                         int H, int W, int F, int N, int radius, int dilation_max) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (n >= N) return;
  const size_t bn = (size_t)b * N + n;
  const float* q = D21 + bn * F;
  const float* img = D11 + (size_t)b * H * W * F;
  int u0 = (int)p1[bn * 2 + 0], v0 = (int)p1[bn * 2 + 1];
  refine_point(H, W, radius, dilation_max, 1.17549435e-38f /* FLT_MIN */, u0, v0, [&](size_t pix) {
    const float* c = img + pix * F;
    float s = 0.0f;
    for (int k = 0; k < F; k++) s += q[k] * c[k];
    return s;
  });
  p1_new[bn * 2 + 0] = u0;
  p1_new[bn * 2 + 1] = v0;
}

}  // namespace m3s

// ------------------------------------------------------------------------------------------
// launchers (declared in m3s_match.h, called from abi_match.cpp)
// ------------------------------------------------------------------------------------------
// D11 (nullable): convert the descriptors too, planar (refine tile path, F = 24; cnorm_part nullable: the tile
// partials of the screen's norm bound, B * tiles floats) or in the (B,H,W,F) layout (per-pixel refine kernels).
// D8 (nullable; needs cnorm_part): the planar path also writes the int8 screen copy (B x 24 N bytes) and cnorm_part
// holds 3 x B * tiles floats (norm, max component, max 1-norm)
extern "C" hipError_t m3s_launch_prep(const float* X11, float* rays9, const float* D11, void* D11h, int B, int H,
                                      int W, int F, int planar, float* cnorm_part, void* D8, hipStream_t s) {
  dim3 grid((W + PREP_T - 1) / PREP_T, (H + PREP_T - 1) / PREP_T, B);
  auto k = D11 == nullptr ? m3s::prep_rays_kernel<0>
           : !planar      ? m3s::prep_rays_kernel<2>
           : (D8 != nullptr && cnorm_part != nullptr) ? m3s::prep_rays_kernel<3> : m3s::prep_rays_kernel<1>;
  hipLaunchKernelGGL(k, grid, dim3(256), 0, s, X11, rays9, D11, reinterpret_cast<m3s::h1*>(D11h), H, W, F,
                     cnorm_part, reinterpret_cast<signed char*>(D8));
  return hipGetLastError();
}

extern "C" int m3s_prep_parts(int B, int H, int W) {
  return B * ((W + PREP_T - 1) / PREP_T) * ((H + PREP_T - 1) / PREP_T);
}

extern "C" hipError_t m3s_launch_iter_proj(const float* rays, const float* pts, const float* p_init, float* p_new,
                                           uint8_t* conv, int B, int H, int W, int N, int max_iter, float lambda_init,
                                           float cost_thresh, hipStream_t s) {
  if ((size_t)9 * H * W >= ((size_t)1 << 31)) return hipErrorInvalidValue;  // bilin_sample9's 32-bit offsets
  dim3 grid((N + 255) / 256, B);
  hipLaunchKernelGGL(m3s::iter_proj_kernel, grid, dim3(256), 0, s, rays, pts, p_init, p_new, conv, H, W, N,
                     max_iter, lambda_init, cost_thresh);
  return hipGetLastError();
}

extern "C" hipError_t m3s_launch_proj_occlusion(const float* rays, const float* X11, const float* X21,
                                                const int64_t* idx_init, int* p1, uint8_t* valid, int B, int H, int W,
                                                int max_iter, float lambda_init, float cost_thresh, float dist_thresh,
                                                const float* cnorm_part, int nparts, float* cmax, int nruns,
                                                hipStream_t s) {
  if ((size_t)9 * H * W >= ((size_t)1 << 31)) return hipErrorInvalidValue;  // bilin_sample9's 32-bit offsets
  // cmax (nullable): one wave reduces prep's tile partials into the refine screen's bound (nruns = 3 with the int8
  // screen copy: cmax[0..2] = norm, max component, max 1-norm)
  dim3 grid((H * W + 255) / 256, B);
  hipLaunchKernelGGL(m3s::proj_occlusion_kernel, grid, dim3(256), 0, s, rays, X11, X21, idx_init, p1, valid, H, W,
                     max_iter, lambda_init, cost_thresh, dist_thresh, cnorm_part, nparts, cmax, nruns);
  return hipGetLastError();
}

// the one place the per-pixel refine kernels' F becomes a template argument: launch(std::integral_constant<int, F>{})
template <class L>
static hipError_t refine_with_F(int F, L&& launch) {
  switch (F) {
    case 16: launch(std::integral_constant<int, 16>{}); break;
    case 24: launch(std::integral_constant<int, 24>{}); break;
    case 32: launch(std::integral_constant<int, 32>{}); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

extern "C" hipError_t m3s_launch_refine_f16(const void* D11, const void* D21, const int64_t* p1, int64_t* p1_new, int B,
                                            int H, int W, int F, int N, int radius, int dilation_max, hipStream_t s) {
  dim3 grid((N + 255) / 256, B);
  const m3s::h1* a = reinterpret_cast<const m3s::h1*>(D11);
  const m3s::h1* q = reinterpret_cast<const m3s::h1*>(D21);
  if (N == H * W &&
      m3s_launch_refine_tile(D11, D21, p1, p1_new, B, H, W, F, radius, dilation_max, 0, nullptr, nullptr, s) ==
          hipSuccess)
    return hipSuccess;  // tiled LDS path (query n is pixel n of the grid)
  return refine_with_F(F, [&](auto f) {
    hipLaunchKernelGGL(m3s::refine_f16_kernel<decltype(f)::value>, grid, dim3(256), 0, s, a, q, p1, p1_new, H, W, N,
                       radius, dilation_max);
  });
}

extern "C" hipError_t m3s_launch_refine_f32(const float* D11, const float* D21, const int64_t* p1, int64_t* p1_new,
                                            int B, int H, int W, int F, int N, int radius, int dilation_max,
                                            hipStream_t s) {
  dim3 grid((N + 255) / 256, B);
  hipLaunchKernelGGL(m3s::refine_f32_kernel, grid, dim3(256), 0, s, D11, D21, p1, p1_new, H, W, F, N, radius,
                     dilation_max);
  return hipGetLastError();
}

extern "C" hipError_t m3s_launch_refine_lin(const void* D11h, const float* D21, const int* p1, int64_t* idx_out, int B,
                                            int H, int W, int F, int radius, int dilation_max, const float* cmax,
                                            const void* D8, hipStream_t s) {
  dim3 grid((H * W + 255) / 256, B);
  const m3s::h1* a = reinterpret_cast<const m3s::h1*>(D11h);
  // tiled LDS path exactly when m3s_refine_tile_ok (prep wrote the PLANAR D11h then)
  if (radius > 0 && m3s_refine_tile_ok(B, H, W, F, radius, dilation_max))
    return m3s_launch_refine_tile(D11h, D21, p1, idx_out, B, H, W, F, radius, dilation_max, 1, cmax, D8, s);
  return refine_with_F(F, [&](auto f) {
    hipLaunchKernelGGL(m3s::refine_lin_kernel<decltype(f)::value>, grid, dim3(256), 0, s, a, D21, p1, idx_out, H, W,
                       radius, dilation_max);
  });
}
