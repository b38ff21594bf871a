// Global bundle adjustment (keyframe Sim(3) poses, pointmap edges) for MI355X (gfx950): the linearisation half, from
// the per-call point records to the per-edge sums. The solve of the pose system those sums assemble into is
// ba_sparse.hip (block-sparse, the default) or ba_dense.hip.
//
// Reference semantics:
//   point_align_kernel / ray_align_kernel / calib_proj_kernel
//                     /root/reference/mast3r_slam/backend/src/gn_kernels.cu:455-723, 813-1138, 1231-1543
//   host GN loop      gn_kernels.cu:725-811, 1140-1228, 1546-1637
//
// MI355X design (not a translation):
//   * ba_lin: (edge, point-chunk) blocks. Because Ji = -Jj and Jj = A_i J_local with a per-edge
//     7x7 adjoint map A_i (gn_kernels.cu:277-297 is linear in the row), each lane accumulates only
//     the 28-entry local normal matrix L = sum w J J^T and the 7-entry v = sum w e J in registers
//     (instead of 105 + 14 transformed entries, products/sums in fp64, structural zeros skipped)
//     and the per-edge transform is applied once.
//   * ba_edge: per-edge fp64 reduction of the chunk partials and M = A L A^T, g = A v.
//     The (E,36) edge-sum rows are the only data a multi-GPU run all-reduces.
#include "m3s_ba.h"  // the launchers defined here
#include "m3s_ba_dev.hpp"

namespace m3s {

// the two calib modes share the record format, the pack and the rows; they differ only in how the linearisation forms
// X_j: read whole (BA_MODE_CALIB: the caller constrained the points to their pixel rays) or built from the raw
// point's depth and the plan's ray tables (BA_MODE_CALIB_RAW)
constexpr bool ba_is_calib(int mode) { return mode == BA_MODE_CALIB || mode == BA_MODE_CALIB_RAW; }

// ------------------------------------------------------------------------------------------
// linearisation
// ------------------------------------------------------------------------------------------
// MASK: the row's structurally nonzero Jacobian entries (bit c). Products with a structural zero are skipped:
// for finite weights they add an exact +-0 to the sum, so the result is unchanged (the reference computes
// them; ~45% of the FMAs in rays mode). Products and sums in fp32 (packed: two points per instruction) over
// runs of BA_RUN_LEN rounds per slot, each run then added to the fp64 accumulators (the kernel is VALU-issue
// bound; fp64 products put no measurable accuracy gain against the fp64 truth once runs are short).
#ifndef BA_RUN_LEN  // rounds per fp32 run (points per slot): 8 -> 16 took C5 2.25 -> 2.19 ms, C4 1.91 -> 1.83 ms.
// Round 5: 64 (a chunk is <= 48 rounds, so one fp32 run per slot and chunk, flushed once): with the fp64 retraction and
// relative pose (m3s_common.hpp) the fp32 runs no longer carry the error budget: every BA fixture <= 3.5e-6 from the
// fp64 truth (16: <= 7.2e-6; scripts/ba_acc.py), linearisation -2 % (C5 2.28 -> 2.22 ms, C4 1.86 -> 1.82 ms in
// scripts/ba_exp.py spans; profiles/r05_ba_runlen.txt)
#define BA_RUN_LEN 64
#endif
template <unsigned MASK>
__device__ __forceinline__ void acc_local_f2(f2* L, f2* v, const f2 J[7], f2 w, f2 e) {
  int l = 0;
#pragma unroll
  for (int c = 0; c < 7; c++) {
    const f2 wj = w * J[c];
#pragma unroll
    for (int d = c; d < 7; d++) {
      if ((MASK >> c) & (MASK >> d) & 1u) L[l] = __builtin_elementwise_fma(wj, J[d], L[l]);
      l++;
    }
    if ((MASK >> c) & 1u) v[c] = __builtin_elementwise_fma(wj, e, v[c]);
  }
}

// huber weight (gn_kernels.cu:172-175, k = 1.345 as a double) of two residuals. The reference's quotient is
// the double division k / |r| rounded to float; here the float quotient of the two-float k = KH + KL by |r|,
// refined by one FMA residual step (equal to the double route but for a rounding tie within ~2^-48), so no
// fp64 division sequence runs for every row (the select evaluated it unconditionally).
__device__ __forceinline__ f2 huber_ba2(f2 r) {
  constexpr float KH = 1.345f;
  constexpr float KL = (float)(1.345 - (double)1.345f);
  const f2 ra = {fabsf(r.x), fabsf(r.y)};
  const f2 y = {__builtin_amdgcn_rcpf(ra.x), __builtin_amdgcn_rcpf(ra.y)};
  const f2 q0 = KH * y;
  const f2 e = __builtin_elementwise_fma(-q0, ra, f2{KH, KH}) + KL;
  const f2 q = __builtin_elementwise_fma(e, y, q0);
  // |r| < k -> 1, else k/|r| (<= 1): min(1, q), with |r| = 0 (q NaN from rcp(0) * 0) -> 1 by min's NaN rule
  return f2{fminf(1.0f, q.x), fminf(1.0f, q.y)};
}

// 1/sqrt(x) and 1/x of two values: the hardware estimates (~1 ulp) refined by one Newton step each (packed), which
// takes out the estimates' bias against the reference's IEEE sqrtf and divisions: without it the K = 256 EuRoC rays
// graph sat 1.14e-5 from the fp64 truth (6.8e-6 with it, for +2 % linearisation time; scripts/ba_acc.py)
__device__ __forceinline__ f2 rsq2(f2 x) {
  const f2 y = {__builtin_amdgcn_rsqf(x.x), __builtin_amdgcn_rsqf(x.y)};
  return y * __builtin_elementwise_fma(-0.5f * x * y, y, f2{1.5f, 1.5f});
}
__device__ __forceinline__ f2 rcp2(f2 x) {
  const f2 y = {__builtin_amdgcn_rcpf(x.x), __builtin_amdgcn_rcpf(x.y)};
  return y * __builtin_elementwise_fma(-x, y, f2{2.0f, 2.0f});
}

// Two choices of the rows, measured on MI355X (scripts/ba_acc.py) against their plain forms: the per-point Sim(3)
// action as X + (D X + t) with the per-edge D = s R - I (3 packed FMAs + an add per component instead of the
// quaternion expression's 12 ops under -ffp-contract=off), and explicit FMAs in the calib rows' product-sums (pixel
// projection, the (1 + x^2) Jacobian terms): lin C5 2.20 -> 1.94 ms, C4 1.88 -> 1.80 ms; every BA fixture <= 8e-6
// from the fp64 truth (max: K=256 EuRoC rays 8.0e-6). FMAs in the rays rows gained 1.4 % and cost accuracy (EuRoC
// 8.6e-6): not used.

// The fp64 accumulation is split between the two lanes of a lane pair (even lane: sums 0..17, odd lane: 18..34). At
// a flush a lane hands the partner the run sums the partner owns (DPP swaps) and adds its own and the partner's fp32
// run sums of both points in fp64: the same BA_RUN_LEN-point fp32 runs as with per-lane accumulators (folding a
// lane's two points in fp32 first took the 6-KF rays fixture to 1.6e-5 from the fp64 truth, over the 1e-5 contract),
// half the fp64 values to move through LDS.
#ifndef BA_LIN_WAVES  // waves per SIMD the linearisation is compiled for (VGPR budget 512 / waves)
#define BA_LIN_WAVES 3
#endif
#define BA_PAIR_HALF 18  // sums owned per lane of a pair (35 = 18 + 17)

__device__ __forceinline__ float dpp_swap1(float x) {  // quad_perm [1,0,3,2]: the value of lane ^ 1
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, false));
}

// each lane of the pair (lane ^ 1) adds the fp32 run sums (28 L + 7 v, both points) of the sums it owns, its
// own and the partner's, into its fp64 accumulators
__device__ __forceinline__ void pair_flush(double* acc, const f2* fL, const f2* fv, bool odd) {
  const f2 z2 = {0.0f, 0.0f};
#pragma unroll
  for (int m = 0; m < BA_PAIR_HALF; m++) {
    const f2 lo = m < 28 ? fL[m] : fv[m - 28];
    const int c = BA_PAIR_HALF + m;
    const f2 hi = c < 28 ? fL[c] : (c < 35 ? fv[c - 28] : z2);
    const f2 own = odd ? hi : lo;
    const f2 give = odd ? lo : hi;  // the partner owns the other half
    const f2 got = {dpp_swap1(give.x), dpp_swap1(give.y)};
    acc[m] += (double)own.x;
    acc[m] += (double)own.y;
    acc[m] += (double)got.x;
    acc[m] += (double)got.y;
  }
}

// the pack's per-edge streams (valid, idx, Q, C_j) are read once per call: non-temporal
#define BA_NT_LOAD(ptr) __builtin_nontemporal_load(ptr)
// The per-call point records, built once per gauss_newton call (the GN iterations only move the poses), so that the
// per-iteration gathers, int64 index loads and threshold tests leave the linearisation loop. The record of point k of
// shard edge e, rec[e][k], with Xi = Xs[i][valid ? idx : 0] (gn_kernels.cu reads index 0 for an invalid match):
//   points  {Xi ; sw}                                               16 B
//   rays    {Xi / |Xi| ; sw}, |Xi| in the slot's second array       16 B + 4 B (computed with the linearisation's own
//           instruction sequence, so the rows are bit-identical to normalising there)
//   calib   {u_t | v_t << 16, log z_i (NaN if z_i <= z_eps), sw}    12 B (the lin kernel streams E x N records every
//           iteration: a quarter less HBM traffic)
// sw = sqrt(q) when the match is valid and q > Q_thresh, c_i > C_thresh, c_j > C_thresh, else 0 (gn_kernels.cu:880-906)
// When the plan reuses records (m3s_ba_make_plan_reuse) only the edges of a.pack_list are packed, each into its slot.
// the record of a matched point from its gathered X_i (ind: its pixel in keyframe i) and its folded validity;
// rays: *n = |Xi|
template <int MODE>
__device__ __forceinline__ float4 pack_finish(const BaParams& p, const float* Xi, int64_t ind, float q, bool valid,
                                              float* n) {
  // hardware sqrt (<= 1 ulp): parity is checked against the fp64 truth (1e-5)
  const float sw = valid ? __builtin_amdgcn_sqrtf(q) : 0.0f;
  if constexpr (ba_is_calib(MODE)) {
    const int ind32 = (int)ind;  // < H*W < 2^31: 32-bit division
    const unsigned v_t = (unsigned)(ind32 / p.W), u_t = (unsigned)ind32 - v_t * (unsigned)p.W;  // W, H < 2^16 (plan)
    // log z_i once per call (the same __logf the linearisation applied every iteration), NaN marks z_i <= z_eps
    const float zi = Xi[2];
    return make_float4(__builtin_bit_cast(float, u_t | (v_t << 16)), zi > p.z_eps ? __logf(zi) : __builtin_nanf(""),
                       sw, 0.0f);
  } else if constexpr (MODE == BA_MODE_RAYS) {
    const f2 X[3] = {f2{Xi[0], Xi[0]}, f2{Xi[1], Xi[1]}, f2{Xi[2], Xi[2]}};
    const f2 n2 = X[0] * X[0] + X[1] * X[1] + X[2] * X[2];
    const f2 inv = rsq2(n2);
    *n = (n2 * inv).x;
    return make_float4((inv * X[0]).x, (inv * X[1]).x, (inv * X[2]).x, sw);
  } else {
    return make_float4(Xi[0], Xi[1], Xi[2], sw);
  }
}

// the record of point k of shard edge e (ix, jx: its pose ranks), every load in order (the fused pack of the first
// linearisation, ba_lin_kernel<PACK>); the per-edge streams are non-temporal
template <int MODE>
__device__ __forceinline__ float4 pack_record(const BaArgs& a, const BaParams& p, int e, int ix, int jx, int k,
                                              float* n) {
  const size_t g = (size_t)(e + p.edge_offset) * p.N + k;
  const bool vm = BA_NT_LOAD(&a.valid[g]) != 0;
  const int64_t ind = vm ? BA_NT_LOAD(&a.idx[g]) : 0;
  const float* Xi = a.Xkf[ix] + (size_t)ind * 3;
  const float q = BA_NT_LOAD(&a.Q[g]);
  const bool valid = vm && (q > p.Q_thresh) && (a.Ckf[ix][ind] * a.Cscale[ix] > p.C_thresh) &&
                     (BA_NT_LOAD(&a.Ckf[jx][k]) * a.Cscale[jx] > p.C_thresh);
  return pack_finish<MODE>(p, Xi, ind, q, valid, n);
}

// a record as stored (pack_record) -> as computed on: calib {u_t, v_t, log z_i, sw} (exact: integers < 2^16)
template <int MODE>
__device__ __forceinline__ float4 rec_expand(float4 r) {
  if constexpr (ba_is_calib(MODE)) {
    const unsigned uv = __builtin_bit_cast(unsigned, r.x);
    return make_float4((float)(uv & 0xffffu), (float)(uv >> 16), r.y, r.z);
  } else {
    return r;
  }
}
template <int MODE>
__device__ __forceinline__ void rec_store(float4* slot, int k, float4 r) {
  // records: streamed out once per call (non-temporal, like the pack's input streams)
  if constexpr (ba_is_calib(MODE)) {
    // three 4-B stores, 12 B by construction: a vec3 store may legally be widened to 16 B, which would overwrite the
    // next record's first word (the backend merges these into one dwordx3)
    float* d = reinterpret_cast<float*>(slot) + 3 * (size_t)k;
    __builtin_nontemporal_store(r.x, d);
    __builtin_nontemporal_store(r.y, d + 1);
    __builtin_nontemporal_store(r.z, d + 2);
  } else {
    typedef float f4v __attribute__((ext_vector_type(4)));
    __builtin_nontemporal_store(f4v{r.x, r.y, r.z, r.w}, reinterpret_cast<f4v*>(slot + k));
  }
}
template <int MODE>
__device__ __forceinline__ float4 rec_load(const float4* slot, int k) {
  if constexpr (ba_is_calib(MODE)) {
    const float3 c = reinterpret_cast<const float3*>(slot)[k];
    return make_float4(c.x, c.y, c.z, 0.0f);
  } else {
    return slot[k];
  }
}

// record slot s (m3s_ba.h ba_rec_slot_bytes): N records, then the rays' |Xi| at rec + N
__device__ __forceinline__ float4* rec_of_slot(const BaArgs& a, int s, int N) {
  return reinterpret_cast<float4*>(reinterpret_cast<char*>(a.rec) + (size_t)s * ba_rec_slot_bytes(N));
}

// One block per tile of BA_PACK_TILE points of one edge: the edge's slot, ranks, keyframe pointers and confidence
// scales are block-uniform (scalar loads, once per block, not per point). A lane takes BA_PACK_UNROLL points per trip
// (256 apart): every per-point stream load (valid, idx, Q, C_j; non-temporal, unconditional at a clamped index) is
// issued first, then the X_i / C_i gathers, then the stores, so a point's chain is two loads deep and the trip's
// points overlap. Tiles in XCD-contiguous order: the blocks of XCD x (blockIdx % 8 == x) take the x-th eighth of
// the tile list, whose edges the plan orders by source keyframe, so an XCD gathers its own source keyframes' X_i / C_i.
#ifndef BA_PACK_TILE
#define BA_PACK_TILE 4096
#endif
#ifndef BA_PACK_UNROLL
#define BA_PACK_UNROLL 4
#endif
template <int MODE>
__global__ void __launch_bounds__(256) ba_pack_kernel(BaArgs a, BaParams p, int n_pack, int tiles_per_edge) {
  constexpr int U = BA_PACK_UNROLL;
  const int N = p.N;
  const int n_tiles = n_pack * tiles_per_edge;
  const int tile = (blockIdx.x % 8) * (gridDim.x / 8) + blockIdx.x / 8;  // gridDim.x: a multiple of 8
  if (tile >= n_tiles) return;
  const int t = tile / tiles_per_edge, c = tile - t * tiles_per_edge;
  const int e = a.pack_list ? a.pack_list[t] : t;
  const int ix = a.ii_rank[e], jx = a.jj_rank[e];
  const float* __restrict__ Xi = a.Xkf[ix];
  const float* __restrict__ Ci = a.Ckf[ix];
  const float* __restrict__ Cj = a.Ckf[jx];
  const float si = a.Cscale[ix], sj = a.Cscale[jx];
  float4* rec = rec_of_slot(a, a.rec_slot ? a.rec_slot[e] : e, N);
  const size_t g0 = (size_t)(e + p.edge_offset) * N;
  const int k_begin = c * BA_PACK_TILE, k_end = min(N, k_begin + BA_PACK_TILE);
  for (int k0 = k_begin + (int)threadIdx.x; k0 < k_end; k0 += 256 * U) {
    unsigned char vm[U];
    int64_t id[U];
    float q[U], cj[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int k = min(k0 + 256 * u, k_end - 1);
      vm[u] = BA_NT_LOAD(&a.valid[g0 + k]);
      id[u] = BA_NT_LOAD(&a.idx[g0 + k]);
      q[u] = BA_NT_LOAD(&a.Q[g0 + k]);
      cj[u] = BA_NT_LOAD(&Cj[k]);
    }
    float X[U][3], ci[U];
    int64_t ind[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      ind[u] = vm[u] ? id[u] : 0;  // gn_kernels.cu reads index 0 for an invalid match
      if constexpr (MODE == BA_MODE_CALIB_RAW) {
        X[u][0] = X[u][1] = 0.0f;  // the calib record holds only log z_i: x_i, y_i (off the pixel ray here) are not read
      } else {
        X[u][0] = Xi[(size_t)ind[u] * 3];
        X[u][1] = Xi[(size_t)ind[u] * 3 + 1];
      }
      X[u][2] = Xi[(size_t)ind[u] * 3 + 2];
      ci[u] = Ci[ind[u]];
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int k = k0 + 256 * u;
      if (k >= k_end) continue;
      const bool valid = vm[u] && (q[u] > p.Q_thresh) && (ci[u] * si > p.C_thresh) && (cj[u] * sj > p.C_thresh);
      float n = 0.0f;
      rec_store<MODE>(rec, k, pack_finish<MODE>(p, X[u], ind[u], q[u], valid, &n));
      if constexpr (MODE == BA_MODE_RAYS) __builtin_nontemporal_store(n, reinterpret_cast<float*>(rec + N) + k);
    }
  }
}

// Record reuse: keyframe k's points and confidences against the library's copy from the previous plan (exact bit
// compare, 3N + N words), dirty[k] = 1 on any difference and the copy refreshed. One block row per keyframe; a
// null entry (a keyframe no edge of this shard touches) is skipped. 16-B accesses where the buffers allow.
__device__ __forceinline__ bool cmp_refresh(const unsigned* __restrict__ src, unsigned* __restrict__ dst, size_t n) {
  bool diff = false;
  const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, st = (size_t)gridDim.x * blockDim.x;
  if (n % 4 == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (size_t i = t0; i < n / 4; i += st) {
      const uint4 v = s4[i], d = d4[i];
      if (v.x != d.x || v.y != d.y || v.z != d.z || v.w != d.w) {
        d4[i] = v;
        diff = true;
      }
    }
  } else {
    for (size_t i = t0; i < n; i += st)
      if (dst[i] != src[i]) {
        dst[i] = src[i];
        diff = true;
      }
  }
  return diff;
}

__global__ void __launch_bounds__(256) ba_kf_compare_kernel(const BaKfCopy* __restrict__ kf, int N, uint8_t* dirty) {
  const int k = blockIdx.y;
  const BaKfCopy c = kf[k];
  if (c.copy == nullptr) return;
  unsigned* sx = reinterpret_cast<unsigned*>(c.copy);
  bool diff = cmp_refresh(reinterpret_cast<const unsigned*>(c.X), sx, (size_t)3 * N);
  diff |= cmp_refresh(reinterpret_cast<const unsigned*>(c.C), sx + (size_t)3 * N, (size_t)N);
  if (__any(diff) && (threadIdx.x & 63) == 0) dirty[k] = 1;
}

// ba_lin_kernel's parts ----------------------------------------------------------------------
__device__ __forceinline__ float uniform_f(float x) {  // a block-uniform value, pinned in an SGPR
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
}
// The block-uniform state of the edge between the poses of ranks ix and jx: T_ij as the map Y = X + (D X + t) of a
// point of keyframe j into keyframe i, D and t in SGPRs (the packed FMAs read them as scalar operands)
struct LinEdge {
  float D[9], t[3];  // D = s R - I, row-major
  __device__ __forceinline__ LinEdge(const BaArgs& a, int ix, int jx) {
    // T_ij in double (relSim3_d): in fp32 its translation t_j - t_i rounds at |t_i| (metres), an error coherent over
    // every point of the edge (C4 EuRoC graph: 2.6e-6 -> 5e-7 from the fp64 truth, scripts/ba_prec_exp.py)
    double Td[8];
    relSim3_d(a.Twc + ix * 8, a.Twc + jx * 8, Td);
    // the linear map of actSO3 (Y = X + 2w q x X + 2 q x (q x X), any |q|) times s, in fp64 once per block, kept as its
    // difference from the identity, D = s R - I: small for the near-identity relative poses of co-visible keyframes, so
    // rounding it to fp32 costs far less than rounding s R (ill-conditioned 6-KF fixtures: 1.6-1.8e-5 from the truth)
    const double x = Td[3], y = Td[4], z = Td[5], w = Td[6], sc = Td[7];
    const double R[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w),       2.0 * (x * z + y * w),
                         2.0 * (x * y + z * w),       1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w),
                         2.0 * (x * z - y * w),       2.0 * (y * z + x * w),       1.0 - 2.0 * (x * x + y * y)};
#pragma unroll
    for (int c = 0; c < 9; c++) D[c] = uniform_f((float)(sc * R[c] - ((c % 4 == 0) ? 1.0 : 0.0)));
#pragma unroll
    for (int c = 0; c < 3; c++) t[c] = uniform_f((float)Td[c]);
  }
  // actSim3 (gn_kernels.cu:207-219) as the edge's map X + (D X + t): three packed FMAs and an add per component
  __device__ __forceinline__ void act(const f2 Xj[3], f2 Y[3]) const {
#pragma unroll
    for (int c = 0; c < 3; c++)
      Y[c] = Xj[c] + __builtin_elementwise_fma(
                         f2{D[3 * c], D[3 * c]}, Xj[0],
                         __builtin_elementwise_fma(f2{D[3 * c + 1], D[3 * c + 1]}, Xj[1],
                                                   __builtin_elementwise_fma(f2{D[3 * c + 2], D[3 * c + 2]}, Xj[2],
                                                                             f2{t[c], t[c]})));
  }
};
struct RunSums {  // a lane's fp32 run sums, one slot per point of its pair
  f2 L[28], v[7];
  __device__ __forceinline__ void clear() { *this = RunSums{}; }
};
// the block's fp64 sums (tot) and the room a flush transposes through; each array 16-B aligned, as LDS arrays are
struct LinLds {
  alignas(16) double fl[BA_PAIR_HALF][256];
  alignas(16) double red[35][7];
  alignas(16) double tot[BA_NSUM];
};

// A run's fp32 sums into the block's fp64 sums, and the run sums cleared: the lanes of a pair trade the halves they
// own (pair_flush: fp64 adds from 0 in a per-lane accumulator's order), then the pair sums are transposed through LDS
// (fl: conflict-free, one column per thread), 7 threads per sum add its 128 lanes and then the 7 partials in order: ~40
// instructions per thread, not a 6-level fp64 shuffle butterfly per sum (~110 VALU per sum and wave, ~15 % of the
// kernel). A chunk is at most BA_RUN_LEN rounds (ba_chunks): this runs once per block and no fp64 accumulator is live
// across the point loop: its VGPRs carry the next round's prefetched records. Block-uniform (barriers, and the pair
// flush swaps between lanes): every thread of the block must reach every flush.
__device__ __forceinline__ void lin_flush(RunSums& s, LinLds& lds) {
  const int t = threadIdx.x;
  double acc[BA_PAIR_HALF] = {};
  pair_flush(acc, s.L, s.v, t & 1);
#pragma unroll
  for (int m = 0; m < BA_PAIR_HALF; m++) lds.fl[m][t] = acc[m];
  __syncthreads();
  if (t < 35 * 7) {  // sum c: even lanes own 0..17, odd lanes 18..34
    const int c = t / 7, part = t - 7 * c;
    const int par = c >= BA_PAIR_HALF ? 1 : 0, m = c - BA_PAIR_HALF * par;
    double r = 0.0;
    for (int i = part; i < 128; i += 7) r += lds.fl[m][2 * i + par];
    lds.red[c][part] = r;
  }
  __syncthreads();
  if (t < 35) {
    double r = lds.tot[t];
#pragma unroll
    for (int q = 0; q < 7; q++) r += lds.red[t][q];
    lds.tot[t] = r;
  }
  s.clear();
}

// The rows of one round, one function per residual model: two points per lane, every per-point float operation on both
// at once as one packed fp32 instruction (v_pk_fma/mul/add_f32; float2 lanes), the transcendentals per component. Y:
// points of keyframe j in keyframe i (LinEdge::act); Rx, Ry, Rz: the records' fields as computed on; sqq: sqrt(q) or 0
__device__ __forceinline__ void rows_points(const BaParams& p, const f2 Y[3], f2 Rx, f2 Ry, f2 Rz, f2 sqq, RunSums& s) {
  const f2 err[3] = {Y[0] - Rx, Y[1] - Ry, Y[2] - Rz};
  const f2 sw = p.inv_a * sqq, wc = sw * sw;
  const f2 z2 = {0.0f, 0.0f}, o2 = {1.0f, 1.0f};
  const f2 J0[7] = {o2, z2, z2, z2, Y[2], -Y[1], Y[0]};
  const f2 J1[7] = {z2, o2, z2, -Y[2], z2, Y[0], Y[1]};
  const f2 J2[7] = {z2, z2, o2, Y[1], -Y[0], z2, Y[2]};
  acc_local_f2<0b1110001>(s.L, s.v, J0, huber_ba2(sw * err[0]) * wc, err[0]);  // {0,4,5,6}
  acc_local_f2<0b1101010>(s.L, s.v, J1, huber_ba2(sw * err[1]) * wc, err[1]);  // {1,3,5,6}
  acc_local_f2<0b1011100>(s.L, s.v, J2, huber_ba2(sw * err[2]) * wc, err[2]);  // {2,3,4,6}
}
// (Rx, Ry, Rz) = ri = Xi / |Xi| and n1i = |Xi| (pack_finish: the same operations, once per call)
__device__ __forceinline__ void rows_rays(const BaParams& p, const f2 Y[3], f2 Rx, f2 Ry, f2 Rz, f2 n1i, f2 sqq,
                                          RunSums& s) {
  const f2 n2j = Y[0] * Y[0] + Y[1] * Y[1] + Y[2] * Y[2];
  const f2 n1j_inv = rsq2(n2j);
  const f2 n1j = n2j * n1j_inv;
  const f2 rj[3] = {n1j_inv * Y[0], n1j_inv * Y[1], n1j_inv * Y[2]};
  const f2 err[4] = {rj[0] - Rx, rj[1] - Ry, rj[2] - Rz, n1j - n1i};
  const f2 swr = p.inv_a * sqq, swd = p.inv_b * sqq;
  const f2 wr = swr * swr, wd = swd * swd;
  const f2 n3 = n1j_inv * rcp2(n2j);
  const f2 dxx = n1j_inv - Y[0] * Y[0] * n3, dyy = n1j_inv - Y[1] * Y[1] * n3, dzz = n1j_inv - Y[2] * Y[2] * n3;
  const f2 dxy = -Y[0] * Y[1] * n3, dxz = -Y[0] * Y[2] * n3, dyz = -Y[1] * Y[2] * n3;
  const f2 z2 = {0.0f, 0.0f};
  const f2 J0[7] = {dxx, dxy, dxz, z2, rj[2], -rj[1], z2};
  const f2 J1[7] = {dxy, dyy, dyz, -rj[2], z2, rj[0], z2};
  const f2 J2[7] = {dxz, dyz, dzz, rj[1], -rj[0], z2, z2};
  const f2 J3[7] = {rj[0], rj[1], rj[2], z2, z2, z2, n1j};
  acc_local_f2<0b0110111>(s.L, s.v, J0, huber_ba2(swr * err[0]) * wr, err[0]);  // {0,1,2,4,5}
  acc_local_f2<0b0101111>(s.L, s.v, J1, huber_ba2(swr * err[1]) * wr, err[1]);  // {0,1,2,3,5}
  acc_local_f2<0b0011111>(s.L, s.v, J2, huber_ba2(swr * err[2]) * wr, err[2]);  // {0,1,2,3,4}
  acc_local_f2<0b1000111>(s.L, s.v, J3, huber_ba2(swd * err[3]) * wd, err[3]);  // {0,1,2,6}
}
// both calib modes; lzi: log z_i, NaN where z_i <= z_eps (pack_finish)
__device__ __forceinline__ void rows_calib(const BaParams& p, const f2 Y[3], f2 u_t, f2 v_t, f2 lzi, f2 sqq,
                                           RunSums& s) {
  const auto valid_z = (Y[2] > p.z_eps) & (lzi == lzi);
  const f2 z2 = {0.0f, 0.0f};
  const f2 zj_inv = valid_z ? f2{__builtin_amdgcn_rcpf(Y[2].x), __builtin_amdgcn_rcpf(Y[2].y)} : z2;
  const f2 zj_log = valid_z ? f2{__logf(Y[2].x), __logf(Y[2].y)} : z2;
  const f2 zi_log = valid_z ? lzi : z2;
  const f2 xz = Y[0] * zj_inv, yz = Y[1] * zj_inv;
  const f2 u = __builtin_elementwise_fma(f2{p.fx, p.fx}, xz, f2{p.cx, p.cx}),
           vv = __builtin_elementwise_fma(f2{p.fy, p.fy}, yz, f2{p.cy, p.cy});
  const float ub = (float)p.pixel_border, uh = (float)(p.W - 1 - p.pixel_border),
              vh = (float)(p.H - 1 - p.pixel_border);
  const auto valid = (u > ub) & (u < uh) & (vv > ub) & (vv < vh) & valid_z;
  const f2 err[3] = {u - u_t, vv - v_t, zj_log - zi_log};
  const f2 swp = valid ? p.inv_a * sqq : z2;
  const f2 swd = valid ? p.inv_b * sqq : z2;
  const f2 wp = swp * swp, wd = swd * swd;
  const float fx = p.fx, fy = p.fy;
  const f2 o2 = {1.0f, 1.0f};
  const f2 J0[7] = {fx * zj_inv, z2, -fx * xz * zj_inv, -fx * xz * yz, fx * __builtin_elementwise_fma(xz, xz, o2),
                    -fx * yz, z2};
  const f2 J1[7] = {z2, fy * zj_inv, -fy * yz * zj_inv, -fy * __builtin_elementwise_fma(yz, yz, o2), fy * xz * yz,
                    fy * xz, z2};
  const f2 J2[7] = {z2, z2, zj_inv, yz, -xz, z2, o2};
  acc_local_f2<0b0111101>(s.L, s.v, J0, huber_ba2(swp * err[0]) * wp, err[0]);  // {0,2,3,4,5}
  acc_local_f2<0b0111110>(s.L, s.v, J1, huber_ba2(swp * err[1]) * wp, err[1]);  // {1,2,3,4,5}
  acc_local_f2<0b1011100>(s.L, s.v, J2, huber_ba2(swd * err[2]) * wd, err[2]);  // {2,3,4,6}
}
// the part the models share. R0, R1: the records as computed on (rec_expand); a missing second point (!has1) is the
// first again with weight 0: exact zeros unless the first's own row is non-finite, which poisons the sums anyway
// (another point as filler changed the rays sums)
template <int MODE>
__device__ __forceinline__ void rows(const BaParams& p, const LinEdge& edge, const float4& R0, const float4& R1,
                                     f2 nI, const f2 Xj[3], bool has1, RunSums& s) {
  const f2 Rx = {R0.x, R1.x}, Ry = {R0.y, R1.y}, Rz = {R0.z, R1.z};
  // sqrt(q), 0 for an invalid match (ba_pack) and for the missing second point of a ragged tail
  const f2 sqq = {R0.w, has1 ? R1.w : 0.0f};
  f2 Y[3];
  edge.act(Xj, Y);
  if constexpr (MODE == BA_MODE_POINTS) rows_points(p, Y, Rx, Ry, Rz, sqq, s);
  else if constexpr (MODE == BA_MODE_RAYS) rows_rays(p, Y, Rx, Ry, Rz, nI, sqq, s);
  else rows_calib(p, Y, Rx, Ry, Rz, sqq, s);
}
// raw calib: LDS room for the plan's pixel-ray tables (x_of_u then y_of_v); only the raw-calib instances allocate it
#ifndef BA_RAY_LDS
#define BA_RAY_LDS 2048  // floats: 8 KB on top of the 38 KB of the flush, three blocks per CU still fit its 160 KB
#endif
// Raw calib: the pixels of a lane's two points, round by round. X_j = (z_j x_of_u[u], z_j y_of_v[v], z_j) from the raw
// point's depth and the plan's ray tables (constrain_points_to_ray's values: one rounded product per component, z_j * 1
// exact). (pu, pv): the pixel of the lane's first point of the coming round, one division per lane in init; a round
// adds the block-uniform (su, sv) = (stride % W, stride / W) with one wrap test; the second point is (hu, hv) further.
// Contract: init once, by every thread of the block (RAYLDS: a barrier), then next once per round, in round order from
// the round at k_begin. A lane past the chunk's end (its rows are skipped) may walk past the last image row: its v is
// clamped so that the loads stay inside the tables. RAYLDS: init first copies the tables into LDS (the launcher picks
// this instance when W + H <= BA_RAY_LDS floats: every configured size), the look-ups are then LDS reads, which leave
// the vector-memory pipe to the record and z_j streams; larger images read through the cache.
template <bool RAYLDS>
struct PixWalk {
  int pu = 0, pv = 0, su = 0, sv = 0, hu = 0, hv = 0, W = 0, vmax = 0;
  const float* tab = nullptr;  // x_of_u (W floats) then y_of_v (H floats)
  __device__ __forceinline__ void init(const BaArgs& a, const BaParams& p, int k_begin) {
    const int kk = k_begin + (int)threadIdx.x, half = (int)blockDim.x;
    W = p.W;
    vmax = p.H - 1;
    tab = a.ray_tab;
    if constexpr (RAYLDS) {
      __shared__ float s_ray[BA_RAY_LDS];
      for (int i = (int)threadIdx.x; i < W + p.H; i += half) s_ray[i] = a.ray_tab[i];
      __syncthreads();
      tab = s_ray;
    }
    pv = kk / W;
    pu = kk - pv * W;
    hv = half / W;
    hu = half - hv * W;
    sv = (2 * half) / W;
    su = 2 * half - sv * W;
  }
  // the table entries of the round's two points (a missing second point repeats the first, as in rows), then the step
  __device__ __forceinline__ void next(bool has1, f2& xu, f2& yv) {
    int u1 = pu + hu, v1 = pv + hv;
    if (u1 >= W) {
      u1 -= W;
      v1++;
    }
    if (!has1) {
      u1 = pu;
      v1 = pv;
    }
    xu = f2{tab[pu], tab[u1]};
    yv = f2{tab[W + min(pv, vmax)], tab[W + min(v1, vmax)]};
    pu += su;
    pv += sv;
    if (pu >= W) {
      pu -= W;
      pv++;
    }
  }
};
// z_j is loaded through a global-memory pointer: a pointer read from the keyframe table is generic to the compiler,
// and a flat load counts against the LDS / scalar-memory counter too, which returns out of order: the wait for this
// round's z_j then also waited for the next round's prefetch issued just before it (the whole latency, every round)
typedef const float __attribute__((address_space(1))) * gfloat_p;
struct LinChunk {        // what a block streams:
  float4* rec;           // its edge's record slot
  float* rec_n;          // rays: |Xi|, behind the records
  const float* Xj_base;  // the target keyframe's points
  gfloat_p Zj_base;      // raw calib: their z alone
  int k_begin, k_end;    // its chunk of them
};
// A lane's two points of the round that starts at k00, k00 + threadIdx.x and blockDim.x further. live: the first exists
// (else the lane skips the rows); has1: so does the second. k0, k1: where the lane loads, always inside the chunk
// (a dead lane at k_begin, a missing second point at the first again)
struct RoundPts {
  int k0, k1;
  bool live, has1;
  __device__ __forceinline__ RoundPts(const LinChunk& c, int k00) {
    const int k = k00 + (int)threadIdx.x, bd = (int)blockDim.x;
    live = k < c.k_end;
    has1 = k + bd < c.k_end;
    k0 = live ? k : c.k_begin;
    k1 = k0 + bd < c.k_end ? k0 + bd : k0;
  }
};
struct Round {    // what a lane holds of one round before its rows
  float4 R0, R1;  // the records as stored
  f2 nI;          // rays: |Xi| of both points
  f2 Xj[3];       // raw calib: {x_of_u[u], y_of_v[v], z_j}, multiplied out in lin_round
};
template <int MODE>  // X_j of the round's points; raw calib: z_j alone (Xj[0], Xj[1] come from PixWalk::next)
__device__ __forceinline__ void round_xj(const LinChunk& c, const RoundPts& pt, Round& r) {
  if constexpr (MODE == BA_MODE_CALIB_RAW) {
    r.Xj[2] = f2{c.Zj_base[(size_t)pt.k0 * 3], c.Zj_base[(size_t)pt.k1 * 3]};
  } else {
#pragma unroll
    for (int d = 0; d < 3; d++) r.Xj[d] = f2{c.Xj_base[(size_t)pt.k0 * 3 + d], c.Xj_base[(size_t)pt.k1 * 3 + d]};
  }
}
// a round from the stored records: every load unconditional (RoundPts), so that it can be issued a round ahead
template <int MODE, bool RAYLDS>
__device__ __forceinline__ void round_fetch(const LinChunk& c, int k00, PixWalk<RAYLDS>& pix, Round& r) {
  const RoundPts pt(c, k00);
  r.R0 = rec_load<MODE>(c.rec, pt.k0);
  r.R1 = rec_load<MODE>(c.rec, pt.k1);
  if constexpr (MODE == BA_MODE_RAYS) r.nI = f2{c.rec_n[pt.k0], c.rec_n[pt.k1]};
  round_xj<MODE>(c, pt, r);
  if constexpr (MODE == BA_MODE_CALIB_RAW) pix.next(pt.has1, r.Xj[0], r.Xj[1]);
}
// a live lane's round from the match data (fused pack): its records built, stored for later iterations, kept; in order
template <int MODE>
__device__ __forceinline__ void round_pack(const BaArgs& a, const BaParams& p, int e, int ix, int jx,
                                           const LinChunk& c, const RoundPts& pt, Round& r) {
  float n0 = 0.0f, n1 = 0.0f;
  r.R0 = pack_record<MODE>(a, p, e, ix, jx, pt.k0, &n0);
  n1 = n0;
  if (pt.has1) r.R1 = pack_record<MODE>(a, p, e, ix, jx, pt.k1, &n1);
  else r.R1 = r.R0;
  rec_store<MODE>(c.rec, pt.k0, r.R0);
  if (pt.has1) rec_store<MODE>(c.rec, pt.k1, r.R1);
  if constexpr (MODE == BA_MODE_RAYS) {
    c.rec_n[pt.k0] = n0;
    if (pt.has1) c.rec_n[pt.k1] = n1;
    r.nI = f2{n0, n1};
  }
  round_xj<MODE>(c, pt, r);
}
template <int MODE>  // the rows of round r of a live lane; kept apart from rows on purpose (BA)
__device__ __forceinline__ void lin_round(const BaParams& p, const LinEdge& edge, Round& r, bool has1, RunSums& s) {
  if constexpr (MODE == BA_MODE_CALIB_RAW) {
    r.Xj[0] = r.Xj[2] * r.Xj[0];
    r.Xj[1] = r.Xj[2] * r.Xj[1];
  }
  rows<MODE>(p, edge, rec_expand<MODE>(r.R0), rec_expand<MODE>(r.R1), r.nI, r.Xj, has1, s);
}
// the end of a round, for every thread of the block (lin_flush's contract): after BA_RUN_LEN rounds the run is flushed
__device__ __forceinline__ void run_step(int& run, RunSums& s, LinLds& lds) {
  if (++run == BA_RUN_LEN) {
    run = 0;
    lin_flush(s, lds);
  }
}

// One block per (edge, chunk of its points), two points per lane and round. PACK: the first GN iteration of a call that
// packs every edge builds each point's record itself (pack_record, the same values) and stores it for the later ones:
// the pack's gathers (HBM-bound) run under this kernel's VALU-bound rows instead of as a separate launch before it.
template <int MODE, bool PACK, bool RAYLDS = false>  // specialised per residual type: one mode's registers, not the union of three
__global__ void __launch_bounds__(256, BA_LIN_WAVES) ba_lin_kernel(BaArgs a, BaParams p) {
  if (*a.done) return;
  // the plan's block table: edges grouped by target keyframe, consecutive blocks on one XCD (xcd_remap)
  const int code = a.lin_tab[xcd_remap(blockIdx.x, gridDim.x)];
  const int e = code / p.chunks, chunk = code - e * p.chunks;
  const int ix = a.ii_rank[e], jx = a.jj_rank[e];
  const LinEdge edge(a, ix, jx);
  __shared__ LinLds lds;
  if (threadIdx.x < BA_NSUM) lds.tot[threadIdx.x] = 0.0;
  float4* const rec = rec_of_slot(a, a.rec_slot ? a.rec_slot[e] : e, p.N);
  const float* const Xj = a.Xkf[jx];
  const int per = (p.N + p.chunks - 1) / p.chunks, k_begin = chunk * per;
  const LinChunk c = {rec,     reinterpret_cast<float*>(rec + p.N), Xj, (gfloat_p)(Xj + 2),
                      k_begin, min(p.N, k_begin + per)};
  PixWalk<RAYLDS> pix;
  if constexpr (MODE == BA_MODE_CALIB_RAW) pix.init(a, p, c.k_begin);
  RunSums sums = {};
  int run = 0;
  if constexpr (PACK) {  // in order: a round's records are built, stored and used
    for (int k00 = c.k_begin; k00 < c.k_end; k00 += 2 * blockDim.x) {
      const RoundPts pt(c, k00);
      Round cur;
      if constexpr (MODE == BA_MODE_CALIB_RAW) pix.next(pt.has1, cur.Xj[0], cur.Xj[1]);
      if (pt.live) {
        round_pack<MODE>(a, p, e, ix, jx, c, pt, cur);
        lin_round<MODE>(p, edge, cur, pt.has1, sums);
      }
      run_step(run, sums, lds);
    }
  } else {
    // software-pipelined: a lane loads the next round's records and X_j before it computes this round's rows, so the
    // loads' HBM latency runs under the VALU work (3 waves per SIMD are too few to hide it alone). Every load is
    // unconditional (round_fetch): the hand-over nxt -> cur is then a load's only use while in flight, after the rows.
    Round cur;
    round_fetch<MODE>(c, c.k_begin, pix, cur);
    for (int k00 = c.k_begin; k00 < c.k_end; k00 += 2 * blockDim.x) {
      Round nxt;
      round_fetch<MODE>(c, k00 + 2 * blockDim.x, pix, nxt);
      const RoundPts pt(c, k00);
      if (pt.live) lin_round<MODE>(p, edge, cur, pt.has1, sums);
      run_step(run, sums, lds);
      cur = nxt;
    }
  }
  lin_flush(sums, lds);
  if (threadIdx.x < 35) a.partials[(size_t)code * BA_NSUM + threadIdx.x] = lds.tot[threadIdx.x];  // its own entry
}

// per-edge: sum chunk partials, M = A L A^T, g = A v with A the adjoint-inverse map of T_i.
// Writes edge_sums[(e + edge_offset) * 36 + {0..27: M upper, 28..34: g}].
__global__ void __launch_bounds__(64) ba_edge_kernel(BaArgs a, BaParams p, int E_local) {
  if (*a.done) return;
  const int e = blockIdx.x;
  if (e >= E_local) return;
  __shared__ double s_L[7][7], s_v[7], s_A[7][7], s_AL[7][7];
  const int t = threadIdx.x;
  if (t < 35) {
    // the chunk partials in chunk order, eight loads in flight at a time (one at a time they were a chain of
    // dependent round trips per edge); clamped loads past the last chunk are not added
    double s = 0.0;
    const double* pe = a.partials + (size_t)e * p.chunks * BA_NSUM + t;
    for (int c0 = 0; c0 < p.chunks; c0 += 8) {
      double v[8];
#pragma unroll
      for (int k = 0; k < 8; k++) v[k] = pe[(size_t)min(c0 + k, p.chunks - 1) * BA_NSUM];
#pragma unroll
      for (int k = 0; k < 8; k++)
        if (c0 + k < p.chunks) s += v[k];
    }
    if (t < 28) {
      int r, c;
      tri_rc(t, &r, &c);
      s_L[r][c] = s;
      s_L[c][r] = s;
    } else {
      s_v[t - 28] = s;
    }
  }
  if (t < 7) {  // column t of A: adj_inv_row(e_t) (linear map, gn_kernels.cu:277-297), in float as the reference
    const int ix = a.ii_rank[e];
    float Ti[8];
    for (int c = 0; c < 8; c++) Ti[c] = a.Twc[ix * 8 + c];
    float X[7] = {0, 0, 0, 0, 0, 0, 0}, Y[7];
    X[t] = 1.0f;
    adj_inv_row(Ti, X, Y);
    for (int r = 0; r < 7; r++) s_A[r][t] = (double)Y[r];
  }
  __syncthreads();
  if (t < 49) {
    const int r = t / 7, c = t % 7;
    double s = 0.0;
    for (int k = 0; k < 7; k++) s += s_A[r][k] * s_L[k][c];
    s_AL[r][c] = s;
  }
  __syncthreads();
  double* out = a.edge_sums + (size_t)(e + p.edge_offset) * BA_NSUM;
  if (t < 28) {
    int r, c;
    tri_rc(t, &r, &c);
    double s = 0.0;
    for (int k = 0; k < 7; k++) s += s_AL[r][k] * s_A[c][k];
    out[t] = s;
  } else if (t < 35) {
    const int r = t - 28;
    double s = 0.0;
    for (int k = 0; k < 7; k++) s += s_A[r][k] * s_v[k];
    out[t] = s;
  }
}

}  // namespace m3s

// the one place the run-time mode becomes a template argument: f(std::integral_constant<int, MODE>{}) launches
template <class F>
static hipError_t ba_with_mode(int mode, F&& f) {
  switch (mode) {
    case BA_MODE_POINTS: return f(std::integral_constant<int, BA_MODE_POINTS>{});
    case BA_MODE_RAYS: return f(std::integral_constant<int, BA_MODE_RAYS>{});
    case BA_MODE_CALIB: return f(std::integral_constant<int, BA_MODE_CALIB>{});
    case BA_MODE_CALIB_RAW: return f(std::integral_constant<int, BA_MODE_CALIB_RAW>{});
  }
  return hipErrorInvalidValue;
}

extern "C" hipError_t m3s_launch_ba_kf_compare(const BaKfCopy* kf, int Kp, int N, uint8_t* dirty, hipStream_t s) {
  if (Kp <= 0) return hipSuccess;
  const unsigned bx = (unsigned)std::min<size_t>(((size_t)4 * N + 255) / 256, 64);
  hipLaunchKernelGGL(m3s::ba_kf_compare_kernel, dim3(bx, Kp), dim3(256), 0, s, kf, N, dirty);
  return hipGetLastError();
}

extern "C" hipError_t m3s_launch_ba_pack(const BaArgs* a, const BaParams* p, int n_pack, hipStream_t s) {
  if (n_pack <= 0) return hipSuccess;
  const int tiles = (p->N + BA_PACK_TILE - 1) / BA_PACK_TILE;
  const size_t blocks = ((size_t)n_pack * tiles + 7) & ~(size_t)7;  // a multiple of 8: the XCD-contiguous tile order
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  const dim3 g((unsigned)blocks);
  return ba_with_mode(p->mode, [&](auto mode) {
    hipLaunchKernelGGL(m3s::ba_pack_kernel<decltype(mode)::value>, g, dim3(256), 0, s, *a, *p, n_pack, tiles);
    return hipGetLastError();
  });
}

// pack (first iteration of a call whose pack was deferred): the linearisation also builds and stores the records
extern "C" hipError_t m3s_launch_ba_lin(const BaArgs* a, const BaParams* p, int E_local, int pack, hipStream_t s) {
  if (E_local <= 0) return hipSuccess;
  const dim3 g(E_local * p->chunks);
  return ba_with_mode(p->mode, [&](auto mode) {
    constexpr int M = decltype(mode)::value;
    constexpr bool RAW = M == BA_MODE_CALIB_RAW;         // raw calib has a second instance, for ray tables that fit LDS
    const bool lds = RAW && p->W + p->H <= BA_RAY_LDS;  // (for the other modes both names below are the one instance)
    void (*lin)(BaArgs, BaParams) =
        pack ? (lds ? m3s::ba_lin_kernel<M, true, RAW> : m3s::ba_lin_kernel<M, true, false>)
             : (lds ? m3s::ba_lin_kernel<M, false, RAW> : m3s::ba_lin_kernel<M, false, false>);
    hipLaunchKernelGGL(lin, g, dim3(256), 0, s, *a, *p);
    hipLaunchKernelGGL(m3s::ba_edge_kernel, dim3(E_local), dim3(64), 0, s, *a, *p, E_local);
    return hipGetLastError();
  });
}
