// Per-frame tracking Gauss-Newton (Sim(3), pointmap residuals) for MI355X (gfx950).
//
// Reference semantics:
//   FrameTracker.track pre-GN setup    /root/reference/mast3r_slam/tracker.py:35-70, 129-154
//   FrameTracker.solve                 tracker.py:156-171 (+ nonlinear_optimizer.huber :28-33)
//   opt_pose_ray_dist_sim3             tracker.py:173-214 (geometry.act_Sim3 :45-52, point_to_ray_dist :17-34)
//   opt_pose_calib_sim3                tracker.py:216-266 (geometry.project_calib :63-104,
//                                      constrain_points_to_ray / backproject :37-42, 107-115)
//   check_convergence                  nonlinear_optimizer.py:5-25
//   keyframe fusion + selection stats  tracker.py:95-114, frame.py:41-77 (weighted_pointmap)
//
// Device pipeline per frame, no host synchronisation inside:
//   track_init   : zero the unique(idx[valid]) byte map, the setup counters and the GN hand-off words (only for a
//                  workspace the previous frame's fuse launch has not left clean)
//   track_setup  : (M3S_TRACK_FOLD_SETUP=0 only; by default the GN launch does this itself) state <- T_CkCf =
//                  T_WCk^-1 T_WCf; gather Xf[idx], Qk = sqrt(Qff[idx] Qkf), validity masks, a 32-byte per-point GN
//                  record, counts (valid_opt, valid_kf) and the byte map
//   gn_loop      : ONE persistent launch runs every GN iteration. Per iteration every block accumulates the 28 (H
//                  upper) + 7 (g) + 1 (cost) sums of its points in fp64 and publishes them write-through (sc1); the
//                  blocks of an XCD shard hand their partials to the shard's last arriver, which publishes the shard
//                  sum; every block then polls the 8 shard sums, adds them, solves the 7x7 system, retracts
//                  T <- Exp(tau) T and applies the convergence test itself, so all blocks hold the same T and nothing
//                  is broadcast. Block 0 writes the final state with T_WCf = T_WCk T_CkCf (also to the caller's
//                  T_out). The folded launch also counts unique(idx[valid]) from the byte map while the first solve
//                  runs, and its last block to leave publishes the frame's result to the host mirror
//                  (M3S_TRACK_PUBLISH_GN). The phases are listed above gn_loop_kernel.
//   fuse         : keyframe X <- (C X + C' T_CkCf Xkf) / (C + C'), C += C'; clears the GN hand-off words and the
//                  counters for the next frame; with M3S_TRACK_PUBLISH_GN=0 (or the separate setup) it also counts
//                  the byte map and publishes
#include "m3s_common.hpp"
#include "m3s_track.h"

namespace m3s {

#define GN_NSUM 36

// lietorch group product with the product quaternion re-normalised (RxSO3 ctor), float.
__device__ __forceinline__ void sim3_mul_norm(const float* A, const float* B, float* C) {
  float q[4];
  quat_comp(&A[3], &B[3], q);
  const float ni = __builtin_amdgcn_rsqf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  float t[3];
  actSO3(&A[3], &B[0], t);
  C[0] = A[0] + A[7] * t[0];
  C[1] = A[1] + A[7] * t[1];
  C[2] = A[2] + A[7] * t[2];
  C[3] = q[0] * ni;
  C[4] = q[1] * ni;
  C[5] = q[2] * ni;
  C[6] = q[3] * ni;
  C[7] = A[7] * B[7];
}

__device__ __forceinline__ void sim3_inv(const float* A, float* C) {
  const float qi[4] = {-A[3], -A[4], -A[5], A[6]};
  const float si = 1.0f / A[7];
  float t[3];
  actSO3(qi, &A[0], t);
  C[0] = -si * t[0];
  C[1] = -si * t[1];
  C[2] = -si * t[2];
  C[3] = qi[0];
  C[4] = qi[1];
  C[5] = qi[2];
  C[6] = qi[3];
  C[7] = si;
}

// the grid zeroes the unique-idx byte map, the setup counters and the GN tickets / granules (the state itself is
// initialised by track_setup's first thread, or written whole by the folded GN launch: nothing reads it before)
__global__ void __launch_bounds__(256) track_init_kernel(uint4* flags, int n16, unsigned long long* cnt, unsigned* tick) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n16) flags[i] = make_uint4(0u, 0u, 0u, 0u);
  if (i < M3S_TRACK_SHARDS * 16) cnt[i] = 0ull;
  for (int j = i; j < M3S_TRACK_TICK_WORDS; j += gridDim.x * blockDim.x) tick[j] = 0u;  // tickets + granules
}

// T_CkCf = T_WCk^-1 * T_WCf (tracker.py:180/225): the pose the GN iterations start from
__device__ __forceinline__ void initial_T_CkCf(const float* T_WCk, const float* T_WCf, float* T) {
  float Tk[8], Tf[8], Ti[8];
#pragma unroll
  for (int c = 0; c < 8; c++) {
    Tk[c] = T_WCk[c];
    Tf[c] = T_WCf[c];
  }
  sim3_inv(Tk, Ti);
  sim3_mul_norm(Ti, Tf, T);
}

// state <- {0, T = T_CkCf, T_WCk, old_cost = inf}
__device__ void track_state_init(TrackState* st, const float* T_WCf, const float* T_WCk) {
  *st = TrackState{};
  float T[8];
  initial_T_CkCf(T_WCk, T_WCf, T);
  for (int c = 0; c < 8; c++) {
    st->T[c] = T[c];
    st->T_WCk[c] = T_WCk[c];
  }
  st->old_cost = __builtin_inf();
}

// ------------------------------------------------------------------------------------------
// The 32-byte GN record of a point (r0, r1), its validity for the solve (valid_opt) and for the keyframe stats
// (valid_kf), and the unique-match byte map entry.
// The byte-map mark. wt: write-through (sc1), for a GN launch that counts the map itself: its readers sit on other
// XCDs inside the same launch, where a plain store is still in this XCD's L2 (no kernel boundary writes it back).
__device__ __forceinline__ void mark_flag(uint8_t* flags, int64_t i, bool wt) {
  if (wt)
    __hip_atomic_store(&flags[i], (uint8_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else
    flags[i] = 1;
}

// rays record: [Xf, rd_k = (Xk/|Xk|, |Xk|), sqrtQ*valid]
__device__ __forceinline__ void rays_record(const float* xf, const float* xk, float sq, float4& r0, float4& r1) {
  const float d = sqrtf(xk[0] * xk[0] + xk[1] * xk[1] + xk[2] * xk[2]);
  const float di = 1.0f / d;
  r0 = make_float4(xf[0], xf[1], xf[2], di * xk[0]);
  r1 = make_float4(di * xk[1], di * xk[2], d, sq);
}

// the opt_pose_* surface (p.direct): Qff = Qk, valid_match = valid, Xf pre-gathered, calib measurements given
__device__ __forceinline__ void direct_record(const TrackArgs& a, const TrackParams& p, int n, float4& r0, float4& r1,
                                              bool& valid) {
  valid = a.valid_match[n] != 0;
  const float sq = valid ? sqrtf(a.Qff[n]) : 0.0f;
  const float* Xf = a.Xf + (size_t)n * 3;
  if (p.mode == 0) {
    rays_record(Xf, a.Xk + (size_t)n * 3, sq, r0, r1);
  } else {
    const float* m = a.meas_k + (size_t)n * 3;
    r0 = make_float4(Xf[0], Xf[1], Xf[2], m[0]);
    r1 = make_float4(m[1], m[2], a.valid_meas[n] ? 1.0f : 0.0f, sq);
  }
}

// the tracker's own point n matched to frame pixel i (tracker.py:35-70, 129-154), from its loaded inputs: Xf[i],
// Xk[n], Qff[i], Qkf[n], the confidence sums Cf[i], Ck[n] and the match flag
__device__ __forceinline__ void matched_record(const TrackParams& p, const float* xf, const float* xk, float qff,
                                               float qkf, float cf, float ck, bool vm, int64_t i, int n, float4& r0,
                                               float4& r1, bool& valid_opt, bool& valid_kf) {
  const float qk = sqrtf(qff * qkf);
  const float cfa = cf / p.Nf;  // frame.get_average_conf(): C / N
  const float cka = ck / p.Nk;
  valid_opt = vm && (cfa > p.C_conf) && (cka > p.C_conf) && (qk > p.Q_conf);
  valid_kf = vm && (qk > p.Q_conf);
  const float sq = valid_opt ? sqrtf(qk) : 0.0f;
  if (p.mode == 0) {
    rays_record(xf, xk, sq, r0, r1);
  } else {  // calib: constrain_points_to_ray at pixel idx, meas_k = [u_n, v_n, log z_k]
    const int i32 = (int)i, vi = i32 / p.W;  // 32-bit: i < H*W
    const float uf = (float)(i32 - vi * p.W), vf = (float)vi;
    const float zf = xf[2];
    const float xc = zf * ((uf - p.cx) / p.fx);
    const float yc = zf * ((vf - p.cy) / p.fy);
    const float zk = xk[2];
    const bool vmeas = zk > p.depth_eps;
    const int vnn = n / p.W;
    const float un = (float)(n - vnn * p.W), vn = (float)vnn;
    r0 = make_float4(xc, yc, zf, vmeas ? un : 0.0f);
    r1 = make_float4(vmeas ? vn : 0.0f, vmeas ? logf(zk) : 0.0f, vmeas ? 1.0f : 0.0f, sq);
  }
}

// The records of K points of one thread, and its valid counts added to v_opt / v_kf. A point at nn >= N gets a zero
// record and counts, stores and marks nothing. Matched points are built as one batch: every point's own loads first
// (idx, Qkf, Ck, the match flag, Xk), then every gather at idx (Qff, Cf, Xf), then the math, then the byte-map
// stores, with no branch between the points (a point at nn >= N computes point N - 1 again): one point after another
// stacked each point's two dependent round trips and the branches around them up in front of the first iteration.
template <int K>
__device__ __forceinline__ void setup_points(const TrackArgs& a, const TrackParams& p, const int (&nn)[K],
                                             float4 (&r0)[K], float4 (&r1)[K], int& v_opt, int& v_kf, bool wt_flags) {
  const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (p.direct) {
#pragma unroll
    for (int u = 0; u < K; u++) {
      r0[u] = r1[u] = z;
      if (nn[u] < p.N) {
        bool valid;
        direct_record(a, p, nn[u], r0[u], r1[u], valid);
        v_opt += valid ? 1 : 0;
        v_kf += valid ? 1 : 0;
      }
    }
    return;
  }
  int n[K];
  bool act[K];
  int64_t i[K];
  float qkf[K], ck[K], xk[K][3];
  bool vm[K];
#pragma unroll
  for (int u = 0; u < K; u++) {
    act[u] = nn[u] < p.N;
    n[u] = act[u] ? nn[u] : p.N - 1;
    i[u] = a.idx[n[u]];
    qkf[u] = a.Qkf[n[u]];
    ck[u] = a.Ck[n[u]];
    vm[u] = a.valid_match[n[u]] != 0;
#pragma unroll
    for (int c = 0; c < 3; c++) xk[u][c] = a.Xk[(size_t)n[u] * 3 + c];
  }
  float qff[K], cf[K], xf[K][3];
#pragma unroll
  for (int u = 0; u < K; u++) {
    qff[u] = a.Qff[i[u]];
    cf[u] = a.Cf[i[u]];
#pragma unroll
    for (int c = 0; c < 3; c++) xf[u][c] = a.Xf[i[u] * 3 + c];
  }
#pragma unroll
  for (int u = 0; u < K; u++) {
    float4 q0, q1;
    bool valid_opt, valid_kf;
    matched_record(p, xf[u], xk[u], qff[u], qkf[u], cf[u], ck[u], vm[u], i[u], n[u], q0, q1, valid_opt, valid_kf);
    v_opt += (act[u] && valid_opt) ? 1 : 0;
    v_kf += (act[u] && valid_kf) ? 1 : 0;
    r0[u] = act[u] ? q0 : z;
    r1[u] = act[u] ? q1 : z;
  }
#pragma unroll
  for (int u = 0; u < K; u++)
    if (act[u] && vm[u]) mark_flag(a.flags, i[u], wt_flags);  // benign same-value races; popcounted after the solve
}

__global__ void __launch_bounds__(256) track_setup_kernel(TrackArgs a, TrackParams p) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n == 0) track_state_init(a.state, a.T_WCf, a.T_WCk);
  int v_opt = 0, v_kf = 0;
  if (n < p.N) {
    const int nn[1] = {n};
    float4 r0[1], r1[1];
    setup_points<1>(a, p, nn, r0, r1, v_opt, v_kf, false);
    float4* rec = reinterpret_cast<float4*>(a.rec) + 2 * (size_t)n;
    rec[0] = r0[0];
    rec[1] = r1[0];
  }
  // block-reduce the two counters into one packed 64-bit add on this block's XCD shard: one counter word
  // for all 1024 blocks serialises the adds (~11 ns each, MI355X_MICROARCH.md "fanin")
  __shared__ unsigned long long s_cnt[4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const unsigned long long bo = __ballot(v_opt), bk = __ballot(v_kf);
  if (lane == 0) s_cnt[wid] = ((unsigned long long)__popcll(bk) << 32) | (unsigned long long)__popcll(bo);
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long v = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (v) atomicAdd(&a.cnt[16 * (blockIdx.x % M3S_TRACK_SHARDS)], v);
  }
}

// the setup counters summed over the shards: low 32 bits n_valid_opt, high 32 bits n_valid_kf
__device__ __forceinline__ unsigned long long track_counts(const unsigned long long* cnt) {
  unsigned long long v = 0;
#pragma unroll
  for (int s = 0; s < M3S_TRACK_SHARDS; s++) v += cnt[16 * s];
  return v;
}

__device__ __forceinline__ bool track_skipped(unsigned n_valid_opt, const TrackParams& p) {
  return (float)n_valid_opt / (float)p.N < p.min_match_frac;  // tracker.py:67-70
}

// 7x7 Cholesky solve H tau = g in fp32 (torch.linalg.cholesky / cholesky_solve on the float32 H of
// tracker.py:168-169); false when H is not positive definite (torch raises). The normal equations
// themselves are accumulated in fp64; only this tiny serial tail runs in fp32, where div/sqrt are
// short instruction sequences (the fp64 ones dominated the single-lane tail).
__device__ bool chol7(const double Hd[7][7], const double gd[7], double tau[7]) {
  float L[7][7], Li[7];  // Li = 1 / L_jj (hardware rsq of the pivot: no divides on the chain)
  for (int j = 0; j < 7; j++) {
    float d = (float)Hd[j][j];
    for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k];
    if (!(d > 0.0f)) return false;
    const float dinv = __builtin_amdgcn_rsqf(d);
    L[j][j] = d * dinv;
    Li[j] = dinv;
    for (int i = j + 1; i < 7; i++) {
      float s = (float)Hd[i][j];
      for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
      L[i][j] = s * dinv;
    }
  }
  float y[7], t[7];
  for (int i = 0; i < 7; i++) {
    float s = (float)gd[i];
    for (int k = 0; k < i; k++) s -= L[i][k] * y[k];
    y[i] = s * Li[i];
  }
  for (int i = 6; i >= 0; i--) {
    float s = y[i];
    for (int k = i + 1; k < 7; k++) s -= L[k][i] * t[k];
    t[i] = s * Li[i];
  }
  for (int i = 0; i < 7; i++) tau[i] = t[i];
  return true;
}

template <typename V>
__device__ __forceinline__ void wt(V* p, V v) {  // write-through (sc1) store
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one thread: H, g, cost -> tau -> T update + convergence (tracker.py:156-171, 186-209). Pure: every block's
// thread 0 runs it on the same sums and gets the same result, and block 0 alone writes the final state after the
// loop, so no state byte is written from several XCDs.
struct GnStep {
  float T[8];
  double cost;
  int iter, done, status;
};

__device__ GnStep gn_step(const TrackParams& p, const double* sum, const float* T, int iter, double old) {
  GnStep r;
  for (int c = 0; c < 8; c++) r.T[c] = T[c];
  double H[7][7], g[7], tau[7];
  int l = 0;
  for (int c = 0; c < 7; c++)
    for (int d = c; d < 7; d++) {
      H[c][d] = sum[l];
      H[d][c] = sum[l];
      l++;
    }
  for (int c = 0; c < 7; c++) g[c] = sum[28 + c];
  r.cost = sum[35];
  r.iter = iter;
  r.done = 1;
  r.status = M3S_TRACK_CHOLESKY_FAILED;
  if (!chol7(H, g, tau)) return r;
  float tf[7];
  float tn2 = 0.0f;
  for (int c = 0; c < 7; c++) {
    tf[c] = (float)tau[c];
    tn2 += tf[c] * tf[c];
  }
  float E[8];
  expSim3(tf, E);
  sim3_mul_norm(E, T, r.T);  // T_CkCf.retr(tau) = Exp(tau) * T_CkCf
  r.iter = iter + 1;
  // |(old - cost) / old| < rel_error without the divide; inf - x < inf * r is false on the first step,
  // like the reference's inf/inf = nan
  const bool conv = (fabs(old - r.cost) < (double)p.rel_error * fabs(old)) || (tn2 < p.delta_norm * p.delta_norm);
  r.done = conv || r.iter >= p.max_iters;
  r.status = conv ? M3S_TRACK_OK : (r.done ? M3S_TRACK_MAX_ITERS : M3S_TRACK_RUNNING);
  return r;
}

#ifdef M3S_GN_STAMPS  // (experiment builds only) s_memrealtime stamps of every block: [iteration][block][phase]
#define GN_NSTAMP (8 * 256 * 8)
__device__ unsigned long long g_gn_stamps[GN_NSTAMP];
#define GN_STAMP(it, k)                                                                              \
  do {                                                                                               \
    if (threadIdx.x == 0 && (it) < 8 && blockIdx.x < 256)                                            \
      g_gn_stamps[((it) * 256 + blockIdx.x) * 8 + (k)] = __builtin_amdgcn_s_memrealtime();           \
  } while (0)
#else
#define GN_STAMP(it, k) \
  do {              \
  } while (0)
#endif

typedef __attribute__((address_space(1))) double gdouble;
typedef __attribute__((address_space(1))) int gint;
typedef __attribute__((address_space(1))) unsigned gu32;
typedef __attribute__((address_space(1))) unsigned long long gull;

#ifndef GN_THREADS
#define GN_THREADS 256  // threads of a GN block (one block per CU)
#endif
#define GN_PPT (1024 / GN_THREADS)  // points per thread per round (1024 per block): record loads issued before any math

// ---- the 36 fp64 sums of a wave, reduce-scattered over its lanes (deterministic, no LDS) ----
// Six half-exchange steps (m3s_common.hpp: swap_add<32>, swap_add<16>, then dpp_step by row_ror:8, row_half_mirror
// and the two quad_perms). At every step a lane keeps one half of its current sums and adds the partner's copy of
// that half. Afterwards lane gn_lane_of(c) holds the wave's total of sum c (the other 28 lanes hold padding zeros).
// Fixed order: identical in every block and every run.

// lane holding sum c after wave_sum36 (c < 36)
__device__ __forceinline__ int gn_lane_of(int c) {
  const int r = c / 9, k = c - 9 * r;  // 16-lane row r, position k of {0,1,2,4,5,8,9,10,12}
  const int pos = (k < 3) ? k : (k < 5) ? k + 1 : (k < 8) ? k + 3 : 12;
  return 16 * r + pos;
}

__device__ __forceinline__ double wave_sum36(double (&v)[GN_NSUM], int lane) {
#pragma unroll
  for (int i = 0; i < 18; i++) v[i] = swap_add<32>(v[i], v[i + 18]);
#pragma unroll
  for (int i = 0; i < 9; i++) v[i] = swap_add<16>(v[i], v[i + 9]);
  dpp_step<9, 0>(v, lane & 8);
  dpp_step<5, 1>(v, lane & 4);
  dpp_step<3, 2>(v, lane & 2);
  dpp_step<2, 3>(v, lane & 1);
  return v[0];
}

// ---- the residual rows of two points per lane (float2 lanes: packed fp32 instructions). Every per-point operation
// is written once and applied elementwise to the pair, so each point rounds as it would alone. The row products are
// accumulated in fp32 (packed FMAs, one rounding per product-sum) over the thread's points and added to the fp64 sums
// once per iteration (gn_flush): half the instructions of fp64 product-sums at the GN launch's one wave per SIMD ----
__device__ __forceinline__ f2 g2sqrt(f2 x) { return f2{sqrtf(x.x), sqrtf(x.y)}; }
__device__ __forceinline__ f2 g2fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

// accumulate one whitened row (tracker.py:156-166): robust = si*sqrt(huber(si*r)); A = robust*J; b = robust*r.
// MASK: the row's structurally nonzero Jacobian entries (bit c; the calib rows of chain_row2 have constant
// -0 entries): their products add an exact +-0 to the sums and are skipped (a non-finite row still turns the
// structurally nonzero entries into NaN, so a failing solve still fails). The scale entry J[6] of a ray or pixel
// row is zero in exact arithmetic only; it is masked as well (gn_pair).
template <unsigned MASK = 0x7fu>
__device__ __forceinline__ void acc_row2(f2* acc, const f2 J[7], f2 r, f2 si, float k) {
  const f2 wr = si * r;
  const f2 ra = {fabsf(wr.x), fabsf(wr.y)};
  const f2 hub = {ra.x < k ? 1.0f : k / ra.x, ra.y < k ? 1.0f : k / ra.y};
  const f2 rob = si * g2sqrt(hub);
  f2 A[7];
#pragma unroll
  for (int c = 0; c < 7; c++) A[c] = rob * J[c];
  const f2 b = rob * r;
  int l = 0;
#pragma unroll
  for (int c = 0; c < 7; c++) {
#pragma unroll
    for (int d = c; d < 7; d++) {
      if ((MASK >> c) & (MASK >> d) & 1u) acc[l] = g2fma(A[c], A[d], acc[l]);
      l++;
    }
  }
#pragma unroll
  for (int c = 0; c < 7; c++)
    if ((MASK >> c) & 1u) acc[28 + c] = g2fma(-A[c], b, acc[28 + c]);  // g = -A^T b
  acc[35] = g2fma(0.5f * b, b, acc[35]);
}

// J = -(d h / d Y) [I, -[Y]x, Y]; dh is a 3-vector row of the measurement Jacobian
__device__ __forceinline__ void chain_row2(const f2 dh[3], const f2 Y[3], f2 J[7]) {
  // S = -skew(Y) = [[0, z, -y], [-z, 0, x], [y, -x, 0]] (geometry.act_Sim3 dpC_dR)
  J[0] = -dh[0];
  J[1] = -dh[1];
  J[2] = -dh[2];
  J[3] = -(dh[1] * -Y[2] + dh[2] * Y[1]);
  J[4] = -(dh[0] * Y[2] + dh[2] * -Y[0]);
  J[5] = -(dh[0] * -Y[1] + dh[1] * Y[0]);
  J[6] = -(dh[0] * Y[0] + dh[1] * Y[1] + dh[2] * Y[2]);
}

// points a and b (b = a with weight 0 when the thread has no second point: exact zeros unless a's own row is
// non-finite, which poisons the sums anyway)
__device__ __forceinline__ void gn_pair(const TrackParams& p, const float* T, float4 a0, float4 a1, float4 b0,
                                        float4 b1, f2* acc) {
  const f2 X[3] = {f2{a0.x, b0.x}, f2{a0.y, b0.y}, f2{a0.z, b0.z}};
  f2 Y[3];
  actSim3_2(T, X, Y);
  const f2 sq = {a1.w, b1.w};
  if (p.mode == 0) {
    const f2 d = g2sqrt(Y[0] * Y[0] + Y[1] * Y[1] + Y[2] * Y[2]);
    const f2 di = 1.0f / d;
    const f2 di2 = di * di;
    const f2 rr[3] = {di * Y[0], di * Y[1], di * Y[2]};
    const f2 res[4] = {f2{a0.w, b0.w} - rr[0], f2{a1.x, b1.x} - rr[1], f2{a1.y, b1.y} - rr[2],
                        f2{a1.z, b1.z} - d};
    const f2 si_r = p.c_a * sq, si_d = p.c_b * sq;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      f2 dh[3];
#pragma unroll
      for (int m = 0; m < 3; m++) dh[m] = di * ((k == m ? 1.0f : 0.0f) - di2 * (Y[k] * Y[m]));
      f2 J[7];
      chain_row2(dh, Y, J);
      // J[6] = -(dh . Y) is zero: a point's ray does not change with its length. Its fp32 value is rounding noise
      // (~1e-7) that the ray rows' weight, 1e7 times the distance row's (sigma_dist / sigma_ray squared), adds to
      // the scale's gradient, which only the distance rows determine: at N = 63 it moved the scale by 2.3e-5
      acc_row2<0b0111111u>(acc, J, res[k], si_r, p.huber_k);
    }
    f2 J[7];
    chain_row2(rr, Y, J);
    acc_row2(acc, J, res[3], si_d, p.huber_k);
  } else {
    const f2 x = Y[0], y = Y[1], z = Y[2];
    const f2 pu = p.K[0] * x + p.K[1] * y + p.K[2] * z;
    const f2 pv = p.K[3] * x + p.K[4] * y + p.K[5] * z;
    const f2 pw = p.K[6] * x + p.K[7] * y + p.K[8] * z;
    const f2 u = pu / pw, v = pv / pw;
    const bool vz0 = z.x > p.depth_eps, vz1 = z.y > p.depth_eps;
    const f2 logz = {vz0 ? logf(z.x) : 0.0f, vz1 ? logf(z.y) : 0.0f};
    const float ub = p.pixel_border, uh = (float)(p.W - 1) - p.pixel_border, vh = (float)(p.H - 1) - p.pixel_border;
    const bool ok0 = (u.x > ub) && (u.x < uh) && (v.x > ub) && (v.x < vh) && vz0 && (a1.z != 0.0f);
    const bool ok1 = (u.y > ub) && (u.y < uh) && (v.y > ub) && (v.y < vh) && vz1 && (b1.z != 0.0f);
    const f2 vf = {ok0 ? 1.0f : 0.0f, ok1 ? 1.0f : 0.0f};
    const f2 si_p = vf * (p.c_a * sq), si_z = vf * (p.c_b * sq);
    const f2 zi = 1.0f / z;
    const f2 res[3] = {f2{a0.w, b0.w} - u, f2{a1.x, b1.x} - v, f2{a1.y, b1.y} - logz};
    const f2 z2 = {0.0f, 0.0f};
    f2 dh[3], J[7];
    dh[0] = p.K[0] * zi;
    dh[1] = z2;
    dh[2] = (-p.K[0] * x * zi) * zi;
    chain_row2(dh, Y, J);
    // the pixel rows' J[6] = -(dh . Y) is zero too (a projection does not change with the point's scale)
    acc_row2<0b0111101u>(acc, J, res[0], si_p, p.huber_k);
    dh[0] = z2;
    dh[1] = p.K[4] * zi;
    dh[2] = (-p.K[4] * y * zi) * zi;
    chain_row2(dh, Y, J);
    acc_row2<0b0111110u>(acc, J, res[1], si_p, p.huber_k);
    dh[0] = z2;
    dh[1] = z2;
    dh[2] = zi;
    chain_row2(dh, Y, J);
    acc_row2<0b1011100u>(acc, J, res[2], si_z, p.huber_k);
  }
}

// the thread's fp32 pair sums into its fp64 sums
__device__ __forceinline__ void gn_flush(double* acc, const f2* a2) {
#pragma unroll
  for (int c = 0; c < GN_NSUM; c++) acc[c] += (double)a2[c].x + (double)a2[c].y;
}

// ---- the unique-match count inside the folded GN launch (M3S_TRACK_PUBLISH_GN, the default) ----
// Once a block has seen the iteration-0 shard sums, every block's marks are in memory: they were stored write-through
// and drained (the vmcnt(0) in front of each block's iteration-0 ticket), and every shard sum follows all of its
// shard's tickets. Waves 1..3 of every block then count and clear the map with sc1 loads and stores while wave 0's
// first lane runs the iteration-0 solve: entry i of the n16 16-byte entries belongs to counting thread i % (blocks x
// 192), and the thread that counted an entry clears it. The block's count waits in LDS and rides the block's arrival
// at the publish tickets (the kernel's tail): nothing of it is on the hand-off chain.
#define GN_COUNT_THREADS (GN_THREADS - 64)
static_assert(GN_THREADS > 64, "the map is counted by the waves that do not solve");

__device__ __forceinline__ int map_popc_clear(gull* fl, int i, unsigned long long m0, unsigned long long m1) {
  __hip_atomic_store(&fl[2 * (size_t)i], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&fl[2 * (size_t)i + 1], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return __popcll(m0) + __popcll(m1);
}

__device__ __forceinline__ void map_load(gull* fl, int i, unsigned long long& m0, unsigned long long& m1) {
  m0 = __hip_atomic_load(&fl[2 * (size_t)i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  m1 = __hip_atomic_load(&fl[2 * (size_t)i + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// entries first, first + stride, ... < n16
__device__ __forceinline__ int map_count_clear(gull* fl, int first, int n16, int stride) {
  int cnt = 0;
  for (int i = first; i < n16; i += stride) {
    unsigned long long m0, m1;
    map_load(fl, i, m0, m1);
    cnt += map_popc_clear(fl, i, m0, m1);
  }
  return cnt;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---- the persistent GN launch ----
// All GN iterations in ONE launch (nparts <= 256 blocks, sized by the occupancy query so every block is
// resident). Per iteration:
//   1. every block accumulates its points' 36 fp64 sums (gn_accumulate), reduce-scatters them in each wave
//      (wave_sum36) and adds the 4 waves' totals in LDS (fixed order), publishes the block partial with write-through
//      (sc1) stores into the iteration's slot and takes a ticket on its XCD shard (blocks b and b + 8 share one)
//      (gn_block_partial);
//   2. the shard's last arriver loads its shard's partials with sc1 loads (no acquire fence: every partial byte
//      was stored sc1 and drained before its ticket, MI355X_MICROARCH.md "Valid forms" row 1), sums them in
//      block order and publishes the shard sum as 72 tagged 8-byte granules {32-bit half, iteration} (gn_shard_sum);
//   3. every block polls the 8 shard sums (one wave, sc1 loads: gn_poll), adds them in shard order (gn_frame_sums)
//      and solves the 7x7 system, retracts and tests convergence itself (gn_solve): the same instructions on the
//      same bytes, so every block holds the same T bit for bit, and no broadcast hop or serial last-block tail sits
//      on the chain.
// Spins are bounded: a stalled hand-off ends the frame with status STALLED (the host raises), never a hang.
//
// SETUP (folded setup, M3S_TRACK_FOLD_SETUP=1): no track_setup launch. Every block derives the initial T_CkCf
// itself (initial_T_CkCf), builds its points' records in the first iteration (setup_points: the first round into
// registers, later rounds also into the record buffer for the later iterations), and adds its valid counts to the
// shard counters before its iteration-0 ticket; the skip test (tracker.py:67-70) then reads the counters after the
// iteration-0 hand-off, before the first solve. Without it the launch starts from the state, the records and the
// counters that track_setup left. Either way block 0 writes the whole final state (gn_final_state).
//
// PUBLISH (SETUP launches with pub.mirror set): the launch also counts the unique-match map (above) and publishes
// the frame's result. Every block leaves through one tail, whatever ended it (converged, max iterations, skipped,
// Cholesky failure, stalled hand-off): its thread 0 arrives once, with a relaxed add that never waits, at its XCD
// shard's ticket (256 arrivals at one word would queue for ~3 us, MI355X_MICROARCH.md "fanin"), and the arrival that
// completes a shard arrives for it at the top ticket. The added word carries the block's unique-match count and a
// stalled mark besides the arrival, so the arrival that completes the top ticket holds the frame's n_unique in the
// value its add returned. Every block holds the same final state in registers, so that arriver builds the TrackState
// itself, writes the host mirror and releases the generation at system scope, then re-arms the top ticket (the shard
// tickets lie in the counter lines the fuse launch clears). A frame that ended before the count ran (skipped, or
// stalled at iteration 0) counts and clears the map in the tail.

// a block's place in the grid, in the hand-off and in the map count
struct GnGeom {
  int lane, wid;
  int shard, nsh;        // this block's XCD shard, and the shards in use
  unsigned per;          // blocks in this shard
  int stride, n00;       // the thread's points: n00 + k * stride
  bool pubgn, ucount;    // PUBLISH: the launch publishes the result, and counts the byte map (direct mode has none)
  int n16, ct, cstride;  // the map's 16-byte entries; this thread's first as a counting thread (waves 1..), its stride
};

// the block's LDS: the sums on their way through the hand-off, and the solving thread's result
struct GnShared {
  double w[GN_THREADS / 64][64];  // per-wave totals (wave_sum36 lanes)
  double sum[GN_NSUM];            // the frame's sums
  double grp[7][GN_NSUM];         // shard-last: the 7 row groups' sums
  double shard[M3S_TRACK_SHARDS][GN_NSUM];
  float T[8];  // the solving lane's new T_CkCf
  int last, stop, fin;
};

// what only a SETUP launch keeps in LDS (the separate-setup instance never touches it, so it gets none)
struct GnSetupShared {
  unsigned long long cnt[GN_THREADS / 64];  // per-wave valid counts, then the frame's in cnt[0]
  int ucnt[GN_THREADS / 64];                // PUBLISH: per-wave unique-match counts (waves 1..)
};

// The frame's GN result so far: the same values in every block. Every thread holds T and counts; what a solve
// returns besides T (old, cost, iters, its status) only thread 0, which writes the final state.
struct GnRun {
  float T[8];         // T_CkCf
  double old, cost;   // the convergence test's previous cost (inf before the first solve), the last solve's cost
  int iters, status;
  unsigned long long counts;  // (n_valid_kf << 32) | n_valid_opt
};

// the thread's first-round records (every point at 512x512: 4 per thread), in registers for all iterations (only the
// poses change between iterations), and its valid counts (SETUP, iteration 0)
struct GnRecs {
  float4 c0[GN_PPT], c1[GN_PPT];
  int v_opt, v_kf;
};

// The final TrackState from the block's registers (thread 0): track_state_init's fields plus the GN result. Block 0
// also stores it, and the poses into the caller's T_out: plain stores of a single writer, read by the fuse launch
// after this one.
__device__ __forceinline__ TrackState gn_final_state(const TrackArgs& a, const GnRun& r) {
  const bool solved = r.status == M3S_TRACK_OK || r.status == M3S_TRACK_MAX_ITERS;
  TrackState v{};
#pragma unroll
  for (int c = 0; c < 8; c++) v.T_WCk[c] = a.T_WCk[c];
  v.n_valid_opt = (int)(unsigned)r.counts;
  v.n_valid_kf = (int)(unsigned)(r.counts >> 32);
  v.done = 1;
  v.status = r.status;
  // a frame is skipped before its first solve: T is still the initial pose, iters and cost are still zero
  v.iter = r.iters;
  v.last_cost = r.cost;
  v.old_cost = r.status == M3S_TRACK_SKIPPED ? __builtin_inf() : r.cost;
#pragma unroll
  for (int c = 0; c < 8; c++) v.T[c] = r.T[c];
  if (solved) sim3_mul_norm(v.T_WCk, r.T, v.T_WCf);  // T_WCf = T_WCk * T_CkCf
  if (blockIdx.x == 0) {
    if (solved && a.T_out != nullptr)
      for (int c = 0; c < 8; c++) {
        a.T_out[c] = v.T_WCf[c];
        a.T_out[8 + c] = r.T[c];
      }
    *a.state = v;
  }
  return v;
}

// Prologue: the initial pose (SETUP) or the state track_setup left, the block's geometry and the first round's
// records (built, or loaded). False: nothing to iterate (separate setup only: the frame is done already, or skipped).
template <bool SETUP>
__device__ __forceinline__ bool gn_prologue(const TrackArgs& a, const TrackParams& p, const TrackPublish& pub,
                                            GnGeom& g, GnRun& r, GnRecs& f) {
  r.counts = 0;
  r.iters = 0;
  r.status = M3S_TRACK_RUNNING;
  r.cost = 0.0;
  if constexpr (SETUP) {
    initial_T_CkCf(a.T_WCk, a.T_WCf, r.T);
    r.old = __builtin_inf();
  } else {
    const TrackState* st = a.state;
    if (st->done) return false;
    r.counts = track_counts(a.cnt);
#pragma unroll
    for (int c = 0; c < 8; c++) r.T[c] = st->T[c];
    r.old = st->old_cost;
  }
  if (!SETUP && track_skipped((unsigned)r.counts, p)) {
    r.status = M3S_TRACK_SKIPPED;
    if (blockIdx.x == 0 && threadIdx.x == 0) gn_final_state(a, r);
    return false;
  }
  const unsigned nblk = gridDim.x;
  g.lane = threadIdx.x & 63;
  g.wid = threadIdx.x >> 6;
  g.shard = blockIdx.x % M3S_TRACK_SHARDS;
  g.nsh = (int)min(nblk, (unsigned)M3S_TRACK_SHARDS);
  g.per = (nblk - g.shard + M3S_TRACK_SHARDS - 1) / M3S_TRACK_SHARDS;
  g.stride = nblk * GN_THREADS;
  g.n00 = blockIdx.x * GN_THREADS + threadIdx.x;
  g.pubgn = SETUP && pub.mirror != nullptr;
  g.ucount = g.pubgn && !p.direct;
  g.n16 = (p.N + 15) / 16;
  g.ct = blockIdx.x * GN_COUNT_THREADS + (int)threadIdx.x - 64;
  g.cstride = gridDim.x * GN_COUNT_THREADS;
  f.v_opt = f.v_kf = 0;
  if constexpr (SETUP) {  // built in one batch
    int nn[GN_PPT];
#pragma unroll
    for (int u = 0; u < GN_PPT; u++) nn[u] = g.n00 + u * g.stride;
    setup_points<GN_PPT>(a, p, nn, f.c0, f.c1, f.v_opt, f.v_kf, g.ucount);
  } else {
    const float4* rec = reinterpret_cast<const float4*>(a.rec);
#pragma unroll
    for (int u = 0; u < GN_PPT; u++) {
      const int n = min(g.n00 + u * g.stride, p.N - 1);
      f.c0[u] = rec[2 * (size_t)n];
      f.c1[u] = rec[2 * (size_t)n + 1];
    }
  }
  return true;
}

// Accumulate: the thread's points, round by round (GN_PPT record loads issued before any math), into acc. The later
// rounds of a SETUP launch's iteration 0 build their records here and store them for the later iterations.
template <bool SETUP>
__device__ __forceinline__ void gn_accumulate(const TrackArgs& a, const TrackParams& p, const GnGeom& g,
                                              const GnRun& r, GnRecs& f, int it, double (&acc)[GN_NSUM]) {
  const float4* rec = reinterpret_cast<const float4*>(a.rec);
  const int stride = g.stride;
#pragma unroll
  for (int c = 0; c < GN_NSUM; c++) acc[c] = 0.0;
  f2 a2[GN_NSUM];
#pragma unroll
  for (int c = 0; c < GN_NSUM; c++) a2[c] = f2{0.0f, 0.0f};
  auto pair = [&](int na, const float4& xa0, const float4& xa1, const float4& xb0, const float4& xb1) {
    if (na >= p.N) return;
    if (na + stride < p.N) {
      gn_pair(p, r.T, xa0, xa1, xb0, xb1, a2);
    } else {  // no second point: the first again with weight 0
      float4 z1 = xa1;
      z1.w = 0.0f;
      gn_pair(p, r.T, xa0, xa1, xa0, z1, a2);
    }
  };
#pragma unroll
  for (int u = 0; u < GN_PPT; u += 2) pair(g.n00 + u * stride, f.c0[u], f.c1[u], f.c0[u + 1], f.c1[u + 1]);
  for (int n0 = g.n00 + GN_PPT * stride; n0 < p.N; n0 += GN_PPT * stride) {
    float4 r0[GN_PPT], r1[GN_PPT];
    if (SETUP && it == 0) {  // built here, stored for the later iterations (read back by this same thread)
#pragma unroll
      for (int u = 0; u < GN_PPT; u++) {
        const int nn[1] = {n0 + u * stride};
        float4 q0[1], q1[1];
        setup_points<1>(a, p, nn, q0, q1, f.v_opt, f.v_kf, g.ucount);
        r0[u] = q0[0];
        r1[u] = q1[0];
        if (nn[0] < p.N) {
          float4* w = reinterpret_cast<float4*>(a.rec) + 2 * (size_t)nn[0];
          w[0] = q0[0];
          w[1] = q1[0];
        }
      }
    } else {
#pragma unroll
      for (int u = 0; u < GN_PPT; u++) {
        const int n = min(n0 + u * stride, p.N - 1);
        r0[u] = rec[2 * (size_t)n];
        r1[u] = rec[2 * (size_t)n + 1];
      }
    }
#pragma unroll
    for (int u = 0; u < GN_PPT; u += 2) pair(n0 + u * stride, r0[u], r1[u], r0[u + 1], r1[u + 1]);
  }
  gn_flush(acc, a2);
}

// Block partial: the waves' sums (wave_sum36) added in wave order by 36 threads and stored write-through into this
// iteration's slot; SETUP, iteration 0: the block's valid counts added to its shard's counter. Everything is drained
// (vmcnt(0)) before thread 0 takes the shard ticket; sh.last: this block completed its shard's round.
template <bool SETUP>
__device__ __forceinline__ void gn_block_partial(const TrackArgs& a, const GnGeom& g, GnShared& sh, GnSetupShared& ss,
                                                 const GnRecs& f, int it, double (&acc)[GN_NSUM]) {
  sh.w[g.wid][g.lane] = wave_sum36(acc, g.lane);
  if (SETUP && it == 0) {  // the wave's valid counts, packed (n_valid_kf << 32) | n_valid_opt like track_setup's
    unsigned long long c = ((unsigned long long)(unsigned)f.v_kf << 32) | (unsigned)f.v_opt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if (g.lane == 0) ss.cnt[g.wid] = c;
  }
  __syncthreads();
  if (SETUP && it == 0 && threadIdx.x == 0) {  // before this block's ticket (the vmcnt(0) below drains it)
    unsigned long long c = 0;
#pragma unroll
    for (int w = 0; w < GN_THREADS / 64; w++) c += ss.cnt[w];
    if (c) __hip_atomic_fetch_add(&a.cnt[16 * g.shard], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  gdouble* part = (gdouble*)(a.partials + (size_t)(it % GN_SLOTS) * GN_MAX_BLOCKS * GN_PSTRIDE);
  if (threadIdx.x < GN_NSUM) {
    const int l = gn_lane_of(threadIdx.x);
    double v = sh.w[0][l];
#pragma unroll
    for (int w = 1; w < GN_THREADS / 64; w++) v += sh.w[w][l];
    __hip_atomic_store(&part[(size_t)blockIdx.x * GN_PSTRIDE + threadIdx.x], v, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  GN_STAMP(it, 2);
  if (threadIdx.x == 0) {  // the shard ticket (monotonic within the frame: it + 1 rounds of `per` arrivals)
    const unsigned t = __hip_atomic_fetch_add((gu32*)&a.tick[32 * g.shard], 1u, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_AGENT);
    sh.last = t == (unsigned)(it + 1) * g.per - 1;
    sh.stop = 0;
  }
}

// the shard-sum granules of iteration `it`: [2 parities][8 shards][72] x {half, tag}
__device__ __forceinline__ gu32* gn_granules(const TrackArgs& a, int it) {
  return (gu32*)(a.tick + M3S_TRACK_GRANULES) + 2 * ((it & 1) * M3S_TRACK_SHARDS * 2 * GN_NSUM);
}

// Shard sum (the shard's last arriver): the shard's partial rows (blocks shard, shard + 8, ...) summed in block
// order and published as 72 granules: the lower / upper 32 bits of each sum, tagged it + 1.
__device__ __forceinline__ void gn_shard_sum(const TrackArgs& a, const GnGeom& g, GnShared& sh, int it) {
  GN_STAMP(it, 3);
  const gdouble* part = (const gdouble*)(a.partials + (size_t)(it % GN_SLOTS) * GN_MAX_BLOCKS * GN_PSTRIDE);
  // thread (c, grp) walks column c over rows grp, grp + 7, ... with sc1 loads, then the 7 group sums in order
  if (threadIdx.x < 7 * GN_NSUM) {  // <= 32 rows per shard: at most 5 per thread, all loads in flight at once
    const int c = threadIdx.x % GN_NSUM, grp = threadIdx.x / GN_NSUM;
    double v[5];
#pragma unroll
    for (int k = 0; k < 5; k++) {
      const unsigned row = grp + 7 * k;
      v[k] = row < g.per ? __hip_atomic_load(&part[(size_t)(g.shard + 8 * row) * GN_PSTRIDE + c], __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT)
                         : 0.0;
    }
    sh.grp[grp][c] = (((v[0] + v[1]) + v[2]) + v[3]) + v[4];
  }
  __syncthreads();
  if (threadIdx.x < 2 * GN_NSUM) {
    const int c = threadIdx.x >> 1;
    const double v = (((((sh.grp[0][c] + sh.grp[1][c]) + sh.grp[2][c]) + sh.grp[3][c]) + sh.grp[4][c]) + sh.grp[5][c]) +
                     sh.grp[6][c];
    const unsigned long long bits = __builtin_bit_cast(unsigned long long, v);
    const unsigned half = (threadIdx.x & 1) ? (unsigned)(bits >> 32) : (unsigned)bits;
    __hip_atomic_store((gull*)&gn_granules(a, it)[2 * (g.shard * 2 * GN_NSUM + threadIdx.x)],
                       ((unsigned long long)(it + 1) << 32) | half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  GN_STAMP(it, 4);
}

// Poll (wave 0): every shard's 72 granules (lane l: granules l, l + 64, ... of the nsh x 72) into sh.shard, until
// every tag is this iteration's. A poll round issues all of a lane's granule loads before it looks at any: one load,
// its wait and its tag test at a time made each round nine dependent round trips. The spin is bounded: a lost
// hand-off (~0.25 s) sets sh.stop.
__device__ __forceinline__ void gn_poll(const TrackArgs& a, const GnGeom& g, GnShared& sh, int it) {
  const gu32* gran = gn_granules(a, it);
  const int ng = g.nsh * 2 * GN_NSUM;
  constexpr int GPL = (M3S_TRACK_SHARDS * 2 * GN_NSUM + 63) / 64;  // granules per lane, at most
  unsigned spins = 0;
  for (;;) {
    bool ok = true;
    unsigned long long gv[GPL];
#pragma unroll
    for (int k = 0; k < GPL; k++)
      gv[k] = __hip_atomic_load((gull*)&gran[2 * min(g.lane + 64 * k, ng - 1)], __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int k = 0; k < GPL; k++) {
      const int i = g.lane + 64 * k;
      if (i < ng) {
        if ((unsigned)(gv[k] >> 32) != (unsigned)(it + 1)) {
          ok = false;
        } else {
          unsigned* w = reinterpret_cast<unsigned*>(&sh.shard[0][0]);
          w[i] = (unsigned)gv[k];  // lo/hi words in place: granule i = shard i / 72, sum (i % 72) / 2, half i % 2
        }
      }
    }
    if (__all(ok)) break;
    __builtin_amdgcn_s_sleep(1);
    if (++spins > (1u << 22)) {  // the host raises on status STALLED
      if (g.lane == 0) sh.stop = 1;
      break;
    }
  }
}

// Frame sums: the shard sums added in shard order into sh.sum. SETUP, iteration 0: also the frame's valid counts
// into r.counts. Every block's counts were added before its iteration-0 ticket, and every shard sum polled follows
// all of its shard's tickets: the counters are complete (device-scope loads). True: the frame is skipped
// (tracker.py:67-70).
template <bool SETUP>
__device__ __forceinline__ bool gn_frame_sums(const TrackArgs& a, const TrackParams& p, const GnGeom& g, GnShared& sh,
                                              GnSetupShared& ss, GnRun& r, int it) {
  if (threadIdx.x < GN_NSUM) {
    const int c = threadIdx.x;
    double v = sh.shard[0][c];
    for (int k = 1; k < g.nsh; k++) v += sh.shard[k][c];
    sh.sum[c] = v;
  }
  if (!(SETUP && it == 0)) return false;
  if (threadIdx.x == 0) {
    // the eight loads first, then the sum: written as c += load, the compiler kept each atomic load behind the
    // previous one's wait (eight dependent round trips before the first solve)
    unsigned long long cv[M3S_TRACK_SHARDS], c = 0;
#pragma unroll
    for (int k = 0; k < M3S_TRACK_SHARDS; k++)
      cv[k] = __hip_atomic_load(&a.cnt[16 * k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int k = 0; k < M3S_TRACK_SHARDS; k++) c += cv[k];
    ss.cnt[0] = c;
  }
  __syncthreads();
  r.counts = ss.cnt[0];
  return track_skipped((unsigned)r.counts, p);
}

// Solve (thread 0): the new T and the done flag into LDS for the block, the rest of the step into r
__device__ __forceinline__ void gn_solve(const TrackParams& p, GnShared& sh, GnRun& r, int it) {
  const GnStep s = gn_step(p, sh.sum, r.T, it, r.old);
  for (int c = 0; c < 8; c++) sh.T[c] = s.T[c];
  sh.fin = s.done;
  r.old = s.cost;
  r.cost = s.cost;
  r.iters = s.iter;
  r.status = s.status;
}

// Map count (waves 1.., while thread 0 solves): this thread's entries counted and cleared, the first from the
// halves m0, m1 loaded before the barrier; the wave's count into ss.ucnt
__device__ __forceinline__ void gn_count_map(const TrackArgs& a, const GnGeom& g, GnSetupShared& ss,
                                             unsigned long long m0, unsigned long long m1) {
  gull* fl = (gull*)a.flags;
  int c = 0;
  // the loaded halves are first touched here: without this the popcount, and with it the wait for the loads,
  // moved up to the loads, in front of the barrier the solving lane waits at
  asm volatile("" : "+v"(m0), "+v"(m1));
  if (g.ct < g.n16) c = map_popc_clear(fl, g.ct, m0, m1) + map_count_clear(fl, g.ct + g.cstride, g.n16, g.cstride);
  c = wave_sum_int(c);
  if (g.lane == 0) ss.ucnt[g.wid] = c;
}

// Tail: every block leaves through here. PUBLISH: a block whose map count has not run does it now; thread 0 arrives
// for the block, and the last arrival of all publishes. Block 0 writes the final state (gn_final_state).
__device__ __forceinline__ void gn_tail(const TrackArgs& a, const TrackPublish& pub, const GnGeom& g, GnSetupShared& ss,
                                        const GnRun& r, bool counted) {
  if (g.pubgn) {  // no block waits for another here
    if (g.ucount && !counted && g.wid > 0) {
      const int c = wave_sum_int(map_count_clear((gull*)a.flags, g.ct, g.n16, g.cstride));
      if (g.lane == 0) ss.ucnt[g.wid] = c;
    }
    __syncthreads();
  }
  // every block holds the same values; with PUBLISH the last block to arrive publishes them
  if (threadIdx.x != 0 || !(blockIdx.x == 0 || g.pubgn)) return;
  // the arrival word: {unique-match count : 32, stalled blocks : 16, arrivals : 16}. A block adds its own to its
  // shard's ticket; the add that completes a shard carries the shard's totals on to the top ticket, and the add
  // that completes the top ticket has the frame's: the counts travel in the returned values, so the publisher
  // loads nothing
  unsigned long long arrive = 0ull, ticket = 0ull;
  if (g.pubgn) {
    unsigned tot = 0u;
    if (g.ucount) {
#pragma unroll
      for (int w = 1; w < GN_THREADS / 64; w++) tot += (unsigned)ss.ucnt[w];
    }
    arrive = ((unsigned long long)tot << 32) | (r.status == M3S_TRACK_STALLED ? 0x10000ull : 0ull) | 1ull;
    ticket = __hip_atomic_fetch_add(&a.cnt[16 * g.shard + M3S_TRACK_UNIQUE_WORD], arrive, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
  }
  const TrackState v = gn_final_state(a, r);
  ticket += arrive;
  if (g.pubgn && (ticket & 0xffffull) == g.per) {  // this shard is complete: one arrival at the top ticket for it
    const unsigned long long up = (ticket & ~0xffffull) | 1ull;
    const unsigned long long top =
        __hip_atomic_fetch_add((gull*)pub.ticket, up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + up;
    if ((top & 0xffffull) == (unsigned long long)g.nsh) {  // every block of every shard has arrived
      TrackState h = v;
      h.n_unique = (int)(unsigned)(top >> 32);
      if (((top >> 16) & 0xffffull) != 0ull) h.status = M3S_TRACK_STALLED;  // some block lost a hand-off
      pub.mirror->s = h;
      __hip_atomic_store(&pub.mirror->gen, pub.gen, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store((gull*)pub.ticket, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed
    }
  }
}

template <bool SETUP>
__global__ void __launch_bounds__(GN_THREADS) gn_loop_kernel(TrackArgs a, TrackParams p, TrackPublish pub) {
  __shared__ GnShared sh;
  __shared__ GnSetupShared ss;
  GnGeom g;
  GnRun r;
  GnRecs f;
  if (!gn_prologue<SETUP>(a, p, pub, g, r, f)) return;
  bool counted = false;
  for (int it = 0; it < p.max_iters; it++) {
    GN_STAMP(it, 0);
    double acc[GN_NSUM];
    gn_accumulate<SETUP>(a, p, g, r, f, it, acc);
    GN_STAMP(it, 1);
    gn_block_partial<SETUP>(a, g, sh, ss, f, it, acc);
    __syncthreads();
    if (sh.last) gn_shard_sum(a, g, sh, it);
    if (threadIdx.x < 64) gn_poll(a, g, sh, it);
    __syncthreads();
    if (sh.stop) {
      if (threadIdx.x == 0) {
        wt(&a.state->status, M3S_TRACK_STALLED);
        wt(&a.state->done, 1);
      }
      if (!g.pubgn) return;
      r.status = M3S_TRACK_STALLED;  // PUBLISH: through the tail, so the frame is published and the host raises
      break;
    }
    GN_STAMP(it, 5);
    // PUBLISH: waves 1.. issue the load of their first map entry here and use it while thread 0 solves
    const bool cnow = SETUP && g.ucount && it == 0;
    unsigned long long m0 = 0ull, m1 = 0ull;
    if (cnow && g.wid > 0 && g.ct < g.n16) map_load((gull*)a.flags, g.ct, m0, m1);
    if (gn_frame_sums<SETUP>(a, p, g, sh, ss, r, it)) {
      r.status = M3S_TRACK_SKIPPED;
      break;
    }
    __syncthreads();
    if (threadIdx.x == 0)
      gn_solve(p, sh, r, it);
    else if (cnow && g.wid > 0)  // (the rest of wave 0 idles)
      gn_count_map(a, g, ss, m0, m1);
    __syncthreads();
    if (cnow) counted = true;  // ss.ucnt keeps the block's count until its arrival in the tail
    GN_STAMP(it, 6);
#pragma unroll
    for (int c = 0; c < 8; c++) r.T[c] = sh.T[c];
    const bool fin = sh.fin != 0;
    __syncthreads();  // sh.T / sh.fin are rewritten in the next iteration
    if (fin) break;
  }
  gn_tail(a, pub, g, ss, r, counted);
}

// keyframe.update_pointmap(T_CkCf.act(Xkf), Ckf), weighted_pointmap (frame.py:74-77). Runs only if the GN launch
// finished with a pose (so it can be enqueued before the host reads the state back). Out of place like the
// reference (new X_canon / C tensors); X_out may alias X_in.
#define FUSE_COUNT_BLOCKS 32

// Thread 0 of each counting block arrives after its own n_unique add (the acq_rel ticket orders it); the
// last of the FUSE_COUNT_BLOCKS blocks to arrive copies the final state (n_unique now
// complete) to the host mirror and releases the call's generation at system scope.
__device__ void publish_state(const TrackState* st, TrackPublish pub) {
  if (__hip_atomic_fetch_add(pub.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) != FUSE_COUNT_BLOCKS - 1)
    return;
  TrackState v = *st;
  v.n_unique = __hip_atomic_load(&const_cast<TrackState*>(st)->n_unique, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
  pub.mirror->s = v;
  __hip_atomic_store(&pub.mirror->gen, pub.gen, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(pub.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // every counting block arrived
}

// The counting blocks also leave the frame's scratch clean for the next frame on this workspace (the host then
// skips track_init): the unique-idx byte map (each entry zeroed by the thread that counted it), the setup
// counters, the GN shard tickets and granules (the publish ticket is re-armed by its last arriver). When the GN
// launch has counted, cleared the map and published (pub.mirror null, no n_unique, clean_map 0), these blocks only
// clear the tickets, granules and counters: that stays behind the kernel boundary, because GN blocks poll them until
// they exit.
__global__ void __launch_bounds__(256) fuse_kernel(const TrackState* __restrict__ st, FuseArgs f,
                                                   int N, uint8_t* __restrict__ flags, int* __restrict__ n_unique,
                                                   TrackPublish pub, int clean_map, unsigned* __restrict__ tick,
                                                   unsigned long long* __restrict__ cnt_words) {
  const bool solved = st->done != 0;
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.x < FUSE_COUNT_BLOCKS) {
    const int tcb = blockIdx.x * 256 + threadIdx.x;  // thread among the counting blocks
    for (int j = tcb; j < M3S_TRACK_TICK_WORDS; j += FUSE_COUNT_BLOCKS * 256)
      if (j < M3S_TRACK_PUBLISH_TICKET || j >= M3S_TRACK_GRANULES) tick[j] = 0u;
    if (tcb < M3S_TRACK_SHARDS * 16) cnt_words[tcb] = 0ull;
    const bool count = solved && n_unique != nullptr;
    if (count || clean_map) {
      // |unique(idx[valid])| (tracker.py:106-108): popcount of the byte map track_setup wrote (0/1 bytes,
      // 16-B padded), here after the solve instead of on the first GN iteration's critical path. A few
      // blocks reduce in LDS and add once each: one device-scope atomic per block, not per wave.
      __shared__ int s_cnt[4];
      uint4* fl = reinterpret_cast<uint4*>(flags);
      const int n16 = (N + 15) / 16;
      int cnt = 0;
      for (int i = tcb; i < n16; i += FUSE_COUNT_BLOCKS * 256) {
        const uint4 v = fl[i];
        cnt += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
        if (clean_map) fl[i] = make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
      if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
      __syncthreads();
      if (threadIdx.x == 0 && count) {
        const int tot = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (tot) atomicAdd(n_unique, tot);
      }
    }
    if (threadIdx.x == 0 && pub.mirror != nullptr) publish_state(st, pub);
  }
  if (!solved) return;
  if (f.X_in == nullptr || !(st->status == M3S_TRACK_OK || st->status == M3S_TRACK_MAX_ITERS)) return;
  if (n >= N) return;
  if (n == 0) {  // the store slot's counters (SharedKeyframes.__setitem__ of the fused record, frame.py:271-289)
    if (f.slot_N != nullptr) *f.slot_N = f.N_new;
    if (f.slot_N_updates != nullptr) *f.slot_N_updates = f.N_updates_new;
    if (f.slot_dirty != nullptr) *f.slot_dirty = 1;
  }
  float T[8];
#pragma unroll
  for (int c = 0; c < 8; c++) T[c] = st->T[c];
  const float X[3] = {f.Xkf[3 * (size_t)n], f.Xkf[3 * (size_t)n + 1], f.Xkf[3 * (size_t)n + 2]};
  float Y[3];
  actSim3(T, X, Y);
  const float c0 = f.C_in[n], c1 = f.Ckf[n];
  const float den = c0 + c1;
  float Xo[3];
#pragma unroll
  for (int k = 0; k < 3; k++) Xo[k] = (c0 * f.X_in[3 * (size_t)n + k] + c1 * Y[k]) / den;
#pragma unroll
  for (int k = 0; k < 3; k++) f.X_out[3 * (size_t)n + k] = Xo[k];
  f.C_out[n] = den;
  if (f.Ck_avg != nullptr) f.Ck_avg[n] = den / f.Nk_new;  // keyframe.get_average_conf()
  if (f.Cf_avg != nullptr) f.Cf_avg[n] = f.Cf[n] / f.Nf;  // frame.get_average_conf()
}

}  // namespace m3s

extern "C" hipError_t m3s_launch_track_init(const TrackArgs* a, int N, hipStream_t s) {
  const int n16 = (N + 15) / 16;  // the byte map is carved with a 16-B padded length
  hipLaunchKernelGGL(m3s::track_init_kernel, dim3((n16 + 255) / 256), dim3(256), 0, s,
                     reinterpret_cast<uint4*>(a->flags), n16, a->cnt, a->tick);
  return hipGetLastError();
}

extern "C" hipError_t m3s_launch_track_setup(const TrackArgs* a, const TrackParams* p, hipStream_t s) {
  hipLaunchKernelGGL(m3s::track_setup_kernel, dim3((p->N + 255) / 256), dim3(256), 0, s, *a, *p);
  return hipGetLastError();
}

// Blocks of gn_loop_kernel that can be resident at once on the current device (occupancy query x CUs,
// cached per device): the persistent launch's grid never exceeds it, so on an otherwise idle GPU every block
// is resident; work of other streams only delays blocks (finite kernels), and the bounded spin catches the rest.
extern "C" int m3s_track_max_parts(void) {
  static int cache[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 1;
  if (dev >= 0 && dev < 64 && cache[dev] > 0) return cache[dev];
  int per_cu = 0, per_cu_fold = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(m3s::gn_loop_kernel<false>),
                                                   GN_THREADS, 0) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_fold,
                                                   reinterpret_cast<const void*>(m3s::gn_loop_kernel<true>),
                                                   GN_THREADS, 0) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return 1;
  per_cu = per_cu_fold < per_cu ? per_cu_fold : per_cu;  // either variant's grid is fully resident
  const int n = per_cu * cus > 1 ? per_cu * cus : 1;
  if (dev >= 0 && dev < 64) cache[dev] = n;
  return n;
}

// one persistent launch runs every GN iteration; fold: the setup runs inside it (gn_loop_kernel<true>, no track_setup
// launch before it)
// pub->mirror set (folded launches only): the launch also counts the unique matches and publishes the result, and the
// fuse launch behind it gets no mirror and no count
extern "C" hipError_t m3s_launch_track_iters(const TrackArgs* a, const TrackParams* p, int nparts, int fold,
                                             const TrackPublish* pub, hipStream_t s) {
  if (nparts < 1 || nparts > GN_MAX_BLOCKS) return hipErrorInvalidValue;  // <= 32 blocks per XCD shard (the shard-last loads)
  if (!fold && pub->mirror != nullptr) return hipErrorInvalidValue;
  if (fold)
    hipLaunchKernelGGL(m3s::gn_loop_kernel<true>, dim3(nparts), dim3(GN_THREADS), 0, s, *a, *p, *pub);
  else
    hipLaunchKernelGGL(m3s::gn_loop_kernel<false>, dim3(nparts), dim3(GN_THREADS), 0, s, *a, *p, *pub);
  return hipGetLastError();
}

// fusion (f->X_in non-null) and/or the unique-match count (count: the state's n_unique from the byte map)
extern "C" hipError_t m3s_launch_fuse(const TrackArgs* a, const FuseArgs* f, int count, int N, const TrackPublish* pub,
                                      hipStream_t s) {
  const int grid = (N + 255) / 256 > FUSE_COUNT_BLOCKS ? (N + 255) / 256 : FUSE_COUNT_BLOCKS;  // every counting block publishes
  // count: the byte map was written by track_setup (fused path), so it is counted and cleared
  hipLaunchKernelGGL(m3s::fuse_kernel, dim3(grid), dim3(256), 0, s, a->state, *f, N, a->flags,
                     count ? &a->state->n_unique : nullptr, *pub, count, a->tick, a->cnt);
  return hipGetLastError();
}

#ifdef M3S_GN_STAMPS
extern "C" int m3s_debug_gn_stamps(unsigned long long* out) {
  (void)hipDeviceSynchronize();
  const int rc = hipMemcpyFromSymbol(out, HIP_SYMBOL(m3s::g_gn_stamps), sizeof(unsigned long long) * GN_NSTAMP) == hipSuccess ? 0 : -1;
  static unsigned long long z[GN_NSTAMP];  // zeros: cleared for the next frame (shard-last stamps are sparse)
  (void)hipMemcpyToSymbol(HIP_SYMBOL(m3s::g_gn_stamps), z, sizeof(z));
  return rc;
}
#endif
