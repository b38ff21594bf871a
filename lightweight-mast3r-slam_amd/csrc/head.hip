// Dense head tail: from the ViT head's raw output to the matcher's X, C, D, Q in one streaming launch. Replaces the
// tail of MASt3R's Cat_MLP_LocalFeatures_DPT_Pts3d.forward and postprocess (catmlp_dpt_head.py:25-39,82-95), the
// regressions of dust3r/heads/postprocess.py:22-55 and the downsample of mast3r_slam/mast3r_utils.py:69-78.
//
// Two input layouts, one pixel per lane in both:
//   CAT     a (B, 4 + F + tc, H, W), the argument of the reference's postprocess. Consecutive lanes take consecutive
//           kept pixels, so every channel plane is read in coalesced rows.
//   TOKENS  a = pts (B, 4, H, W), the DPT output, and feat (B, S, (F + tc) 256), the MLP output before transpose /
//           view / pixel_shuffle: channel c of pixel (y, x) is feat[b, (y/16)(W/16) + x/16, c 256 + (y%16) 16 + x%16].
//           One block per 16 x 16 patch, lane = pixel in the patch: each channel is a coalesced 1-KiB read, and a
//           patch row writes 16 x 4 F contiguous bytes of D. A stepped-over pixel's lane exits before it reads.
// Channels: 0..2 xyz, 3 the conf logit l_c, then F descriptor channels, then the desc_conf logit l_q when tc.
// Only the pixels [::step, ::step] are read and written: H' = ceil(H / step), W' = ceil(W / step).
//
// The arithmetic, fp32 in exactly this order (this file is built with -ffp-contract=off):
//   d  = sqrt((x x + y y) + z z)                    no rescaling
//   X  = (xyz / (d < 1e-8 ? 1e-8 : d)) * expm1(d)   a NaN d stays NaN (torch's clip propagates NaN; fmaxf would not)
//   C  = c_lo + (e > c_span ? c_span : e), e = exp(l_c)        a NaN logit gives NaN likewise
//   Q  = the same with q_lo, q_span on l_q when tc, else C's bits
//   n2 = (s0 + s1) + (s2 + s3), s_j = the squares of channels j, j + 4, j + 8, ... added in that order
//   D  = desc / sqrt(n2)                            no clamp: a zero descriptor gives NaN, as in the reference
// sqrt and the divisions are correctly rounded; exp and expm1 are the device library's (not correctly rounded).
//
// A pure stream: 4 (4 + F + tc) bytes in and as many out per kept pixel, every one once. A lane issues all its loads
// before the first dependent operation (lesson 1). No LDS, no barrier, no cross-lane traffic; every
// array is below 2^31 elements (abi_head.cpp), offsets are 64-bit anyway.
// Ordinary loads and stores, not non-temporal ones (measured, DESIGN section 4 "Head tail"): a lane's 16-byte D stores
// are 4 F bytes apart, so a 128-byte line is completed by several store instructions, and with the non-temporal hint
// the launch took 2.5 times as long (49.8 against 20.4 us at 512 x 512); non-temporal loads were 3-16 % slower than
// ordinary ones. A variant with four pixels per lane and 16-byte accesses throughout was no faster either (18.5 us
// against 17.6), so the one-pixel kernel is the only one.
#include "m3s_common.hpp"
#include "m3s_head.h"

#include "../../include/m3s.h"

namespace m3s {

typedef float f4v __attribute__((ext_vector_type(4)));

// e = exp(l) clipped from above like torch's clip(max=span), then shifted: NaN in, NaN out
__device__ __forceinline__ float head_conf(float l, float lo, float span) {
  const float e = expf(l);
  return lo + (e > span ? span : e);
}

// FP: the descriptor width rounded up to a multiple of HEAD_F_GROUP (the registers a lane keeps); VEC: 16-byte D stores
template <int LAYOUT, int FP, bool VEC>
__global__ __launch_bounds__(HEAD_BLOCK) void head_post_kernel(const HeadArgs a) {
  const int F = a.F, tc = a.tc;
  const unsigned step = (unsigned)a.step;
  unsigned b, y, x;  // the input pixel
  size_t o;          // the output pixel (b Ho + oy) Wo + ox
  const float* q;    // the lane's first descriptor channel
  size_t qs;         // elements between its channels
  const size_t plane = (size_t)a.H * a.W;
  if constexpr (LAYOUT == M3S_HEAD_CAT) {
    const unsigned gid = blockIdx.x * (unsigned)HEAD_BLOCK + threadIdx.x;
    if (gid >= (unsigned)a.B * (unsigned)a.Ho * (unsigned)a.Wo) return;  // below 2^31 (abi_head.cpp)
    const unsigned t = gid / (unsigned)a.Wo, ox = gid - t * (unsigned)a.Wo;
    b = t / (unsigned)a.Ho;
    y = (t - b * (unsigned)a.Ho) * step, x = ox * step;
    o = gid;
    q = a.a + ((size_t)b * (4 + F + tc) + 4) * plane + (size_t)y * a.W + x;
    qs = plane;
  } else {
    const unsigned pw = (unsigned)a.W / HEAD_PATCH, ph = (unsigned)a.H / HEAD_PATCH;
    const unsigned t = blockIdx.x / pw, px = blockIdx.x - t * pw;  // gridDim.x = B ph pw exactly
    b = t / ph;
    const unsigned py = t - b * ph;
    y = py * HEAD_PATCH + (threadIdx.x >> 4), x = px * HEAD_PATCH + (threadIdx.x & 15);
    if (step > 1 && (y % step != 0 || x % step != 0)) return;  // a stepped-over pixel is not read
    o = ((size_t)b * a.Ho + y / step) * a.Wo + x / step;
    q = a.feat + ((size_t)b * ph * pw + (size_t)py * pw + px) * ((size_t)(F + tc) * (HEAD_PATCH * HEAD_PATCH)) +
        threadIdx.x;
    qs = HEAD_PATCH * HEAD_PATCH;
  }
  const float* p = a.a + (size_t)b * (LAYOUT == M3S_HEAD_CAT ? 4 + F + tc : 4) * plane + (size_t)y * a.W + x;

  // every load of the lane, before any arithmetic on them
  const float vx = p[0], vy = p[plane], vz = p[2 * plane], lc = p[3 * plane];
  // a padding channel (c >= F) reads the last real one again and drops it: the loads stay unconditional, so none of
  // them waits behind a branch
  float d[FP];
#pragma unroll
  for (int c = 0; c < FP; c++) d[c] = q[(size_t)(c < F ? c : F - 1) * qs];
  const float lq = q[(size_t)(F - 1 + tc) * qs];  // without tc: the last channel again, unused
  // the scheduler may not sink a load below the arithmetic: it would wait a second time for memory there
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int c = 0; c < FP; c++) d[c] = c < F ? d[c] : 0.0f;

  // points
  const float dist = sqrtf((vx * vx + vy * vy) + vz * vz);
  const float den = dist < 1e-8f ? 1e-8f : dist;
  const float em = expm1f(dist);
  float* X = a.X + 3 * o;
  X[0] = (vx / den) * em;
  X[1] = (vy / den) * em;
  X[2] = (vz / den) * em;

  // confidences
  const float conf = head_conf(lc, a.c_lo, a.c_span);
  a.C[o] = conf;
  a.Q[o] = tc ? head_conf(lq, a.q_lo, a.q_span) : conf;

  // descriptor: the padding channels are zeros and add nothing to the sums
  float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int c = 0; c < FP; c++) s[c & 3] = s[c & 3] + d[c] * d[c];
  const float nrm = sqrtf((s[0] + s[1]) + (s[2] + s[3]));
  float* D = a.D + o * (size_t)F;
  if constexpr (VEC) {
#pragma unroll
    for (int c = 0; c < FP; c += 4)
      if (c < F)  // F % 4 == 0: whole chunks
        *reinterpret_cast<f4v*>(D + c) = f4v{d[c] / nrm, d[c + 1] / nrm, d[c + 2] / nrm, d[c + 3] / nrm};
  } else {
#pragma unroll
    for (int c = 0; c < FP; c++)
      if (c < F) D[c] = d[c] / nrm;
  }
}

template <int LAYOUT, int FP>
static void head_launch_fp(const HeadArgs* a, dim3 grid, hipStream_t s) {
  if (a->vec) hipLaunchKernelGGL((head_post_kernel<LAYOUT, FP, true>), grid, dim3(HEAD_BLOCK), 0, s, *a);
  else hipLaunchKernelGGL((head_post_kernel<LAYOUT, FP, false>), grid, dim3(HEAD_BLOCK), 0, s, *a);
}

template <int LAYOUT>
static void head_launch(const HeadArgs* a, hipStream_t s) {
  const unsigned blocks = LAYOUT == M3S_HEAD_CAT
                              ? (unsigned)(((int64_t)a->B * a->Ho * a->Wo + HEAD_BLOCK - 1) / HEAD_BLOCK)
                              : (unsigned)((int64_t)a->B * (a->H / HEAD_PATCH) * (a->W / HEAD_PATCH));
  const dim3 grid(blocks);
  switch ((a->F + HEAD_F_GROUP - 1) / HEAD_F_GROUP) {
    case 1: head_launch_fp<LAYOUT, 8>(a, grid, s); break;
    case 2: head_launch_fp<LAYOUT, 16>(a, grid, s); break;
    case 3: head_launch_fp<LAYOUT, 24>(a, grid, s); break;
    default: head_launch_fp<LAYOUT, 32>(a, grid, s); break;
  }
}

}  // namespace m3s

static_assert(HEAD_MAX_F == 4 * HEAD_F_GROUP && HEAD_BLOCK == HEAD_PATCH * HEAD_PATCH, "head_launch's cases");

extern "C" hipError_t m3s_launch_head_post(const HeadArgs* a, hipStream_t s) {
  if (a->layout == M3S_HEAD_CAT) m3s::head_launch<M3S_HEAD_CAT>(a, s);
  else m3s::head_launch<M3S_HEAD_TOKENS>(a, s);
  return hipGetLastError();
}
