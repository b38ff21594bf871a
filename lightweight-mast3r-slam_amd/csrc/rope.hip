// RoPE2D: the 2-D rotary position embedding of the MASt3R ViT's attentions, in place on q or k. Replaces the
// reference's CUDA extension `curope` (croco/models/curope/kernels.cu:17-108; its CPU statement curope.cpp:12-47).
//
// A token's head row of D = 4 Q elements is [u_y | v_y | u_x | v_x], Q each. For axis a (0 = y, 1 = x) and t < Q:
//   u' = u c - v s,  v' = v c + u s,  c, s = cos, sin(fwd pos[a] / base^(t / Q)).
// The reference evaluates powf, cosf and sinf per lane; here c and s come from a cached table (abi_rope.cpp: fp64 on
// the host, rounded once to fp32) for positions in [0, ROPE_TABLE_P), and from fp64 device trig of the same formula
// for every other position. The arithmetic is fp32 exactly as written (this file is built with -ffp-contract=off):
// two products and one subtraction or addition per output, then one round-to-nearest-even to the token dtype.
//
// A pure stream: every element is read once and written once. A lane owns one chunk of u (16 bytes on the vector
// path, one element on the scalar path) and the matching chunk of v, Q elements further on; it loads its table chunk
// once and rotates up to ROPE_MAX_HPL heads with it. Consecutive lanes cover the chunks of u_y, then u_x, then the
// next head group, so a wave's loads cover whole head rows. No LDS, no cross-lane traffic, 64-bit offsets.
#include "m3s_common.hpp"
#include "m3s_rope.h"

namespace m3s {

// storage types and their fp32 conversions (to_f32 exact; from_f32 round-to-nearest-even)
struct RopeF32 {
  typedef float T;
  static __device__ __forceinline__ float to_f32(T x) { return x; }
  static __device__ __forceinline__ T from_f32(float x) { return x; }
};
struct RopeF16 {
  typedef _Float16 T;
  static __device__ __forceinline__ float to_f32(T x) { return (float)x; }
  static __device__ __forceinline__ T from_f32(float x) { return (_Float16)x; }
};
struct RopeBF16 {
  typedef __bf16 T;  // gfx950 converts in hardware (v_cvt_pk_bf16_f32)
  static __device__ __forceinline__ float to_f32(T x) { return (float)x; }
  static __device__ __forceinline__ T from_f32(float x) { return (__bf16)x; }
};

// E elements as one global access: 16 bytes on the vector path (E = 16 / sizeof(T)), the element itself for E = 1
template <typename T, int E>
struct RopeChunk {
  T v[E];
};
template <typename T, int E>
__device__ __forceinline__ RopeChunk<T, E> rope_load(const T* p) {
  if constexpr (E == 1) {
    return RopeChunk<T, 1>{{*p}};
  } else {
    static_assert(sizeof(T) * E == 16, "a vector chunk is 16 bytes");
    return __builtin_bit_cast(RopeChunk<T, E>, *reinterpret_cast<const uint4*>(p));
  }
}
template <typename T, int E>
__device__ __forceinline__ void rope_store(T* p, const RopeChunk<T, E>& c) {
  if constexpr (E == 1) *p = c.v[0];
  else *reinterpret_cast<uint4*>(p) = __builtin_bit_cast(uint4, c);
}

// The slow path of a position outside the table: the table's formula with fp64 device trig, rounded to fp32. Kept
// out of line: no ViT position reaches it, and inlined its argument reduction would set the kernel's registers.
template <int E>
__device__ __noinline__ void rope_trig_f64(int64_t p, const double* inv, float* cs, float* sn) {
#pragma unroll
  for (int j = 0; j < E; j++) {
    const double ang = (double)p * inv[j];
    cs[j] = (float)cos(ang);
    sn[j] = (float)sin(ang);
  }
}

template <typename X, int E>
__global__ __launch_bounds__(ROPE_BLOCK) void rope2d_kernel(const RopeArgs a) {
  typedef typename X::T T;
  const int64_t gid = (int64_t)blockIdx.x * ROPE_BLOCK + threadIdx.x;
  if (gid >= a.lanes) return;
  // gid = ((token * HG + head group) * 2 + axis) * cq + chunk
  const int cq = a.Q / E;
  const uint32_t per_tok = (uint32_t)a.HG * 2u * (uint32_t)cq;
  int64_t tok, b;
  uint32_t r;
  if (a.lanes <= 0x7fffffff) {  // uniform: the 32-bit divisions of every ViT shape
    tok = (uint32_t)gid / per_tok;
    r = (uint32_t)gid - (uint32_t)tok * per_tok;
    b = (uint32_t)tok / (uint32_t)a.N;
  } else {
    tok = gid / per_tok;
    r = (uint32_t)(gid - tok * per_tok);
    b = tok / a.N;
  }
  const int64_t n = tok - b * a.N;
  const int hg = (int)(r / (2u * cq));
  const uint32_t r2 = r - (uint32_t)hg * 2u * cq;
  const int ax = r2 >= (uint32_t)cq;
  const int t0 = (int)(r2 - (ax ? cq : 0)) * E;

  const int64_t p = a.pos[tok * 2 + ax];
  float cs[E], sn[E];
  if ((uint64_t)p < (uint64_t)ROPE_TABLE_P) {
    const float* tc = a.tab.cos + (size_t)p * a.Q + t0;
    const float* ts = a.tab.sin + (size_t)p * a.Q + t0;
    if constexpr (E == 1) {
      cs[0] = *tc;
      sn[0] = *ts;
    } else {
#pragma unroll
      for (int j = 0; j < E; j += 4) {
        const float4 c4 = *reinterpret_cast<const float4*>(tc + j), s4 = *reinterpret_cast<const float4*>(ts + j);
        cs[j] = c4.x, cs[j + 1] = c4.y, cs[j + 2] = c4.z, cs[j + 3] = c4.w;
        sn[j] = s4.x, sn[j + 1] = s4.y, sn[j + 2] = s4.z, sn[j + 3] = s4.w;
      }
    }
  } else {
    float c64[E], s64[E];  // the out-of-line call's memory operands: cs and sn themselves stay in registers
    rope_trig_f64<E>(p, a.tab.inv + t0, c64, s64);
#pragma unroll
    for (int j = 0; j < E; j++) cs[j] = c64[j], sn[j] = s64[j];
  }

  T* row = static_cast<T*>(a.tokens) + b * a.stride_b + n * a.stride_n + (int64_t)ax * 2 * a.Q + t0;
  for (int h = hg; h < a.H; h += a.HG) {
    T* pu = row + (int64_t)h * a.D;
    T* pv = pu + a.Q;
    const RopeChunk<T, E> u = rope_load<T, E>(pu), v = rope_load<T, E>(pv);
    RopeChunk<T, E> un, vn;
#pragma unroll
    for (int j = 0; j < E; j++) {
      const float uf = X::to_f32(u.v[j]), vf = X::to_f32(v.v[j]);
      un.v[j] = X::from_f32(uf * cs[j] - vf * sn[j]);
      vn.v[j] = X::from_f32(vf * cs[j] + uf * sn[j]);
    }
    rope_store<T, E>(pu, un);
    rope_store<T, E>(pv, vn);
  }
}

template <typename X>
static void rope_launch(const RopeArgs* a, hipStream_t s) {
  const dim3 grid((unsigned)((a->lanes + ROPE_BLOCK - 1) / ROPE_BLOCK)), block(ROPE_BLOCK);
  if (a->vec) hipLaunchKernelGGL((rope2d_kernel<X, 16 / (int)sizeof(typename X::T)>), grid, block, 0, s, *a);
  else hipLaunchKernelGGL((rope2d_kernel<X, 1>), grid, block, 0, s, *a);
}

}  // namespace m3s

extern "C" hipError_t m3s_launch_rope2d(const RopeArgs* a, hipStream_t s) {
  if (a->dtype == 0) m3s::rope_launch<m3s::RopeF16>(a, s);
  else if (a->dtype == 1) m3s::rope_launch<m3s::RopeF32>(a, s);
  else m3s::rope_launch<m3s::RopeBF16>(a, s);
  return hipGetLastError();
}
