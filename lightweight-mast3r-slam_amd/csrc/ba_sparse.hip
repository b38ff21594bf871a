// Block-sparse solve of the BA pose system (SparseBlock update_lhs/rhs + SimplicialLLT solve, gn_kernels.cu:57-159,
// and pose_retr_kernel, gn_kernels.cu:415-453), pattern analysed once per plan on the host (ba_pattern.cpp:
// minimum-degree order, 7x7-block factor pattern, elimination-tree levels, per-level update lists). The system is
// assembled from the per-edge sums of the linearisation (ba.hip); ba_dense.hip is the other solve of the same system.
//
// ba_assemble_kernel: one 64-lane block per factor block (fill blocks are written as zeros, so the
// factor storage needs no clearing) and one per rhs block row; contributions summed in the plan's
// fixed edge order (deterministic: identical on every rank, so every rank solves an identical system and
// keeps identical poses).
//
// ba_sparse_factor_kernel: ONE workgroup of 16 waves factors, solves and retracts. The work is a few
// MFLOP, so what bounds it is the dependency chain through the elimination tree, not throughput; in one
// workgroup every hand-off is a __syncthreads (tens of ns) instead of a cross-CU flag (1-3 us each,
// MI355X_MICROARCH.md "handoff-flag"), and the factor (<= 1 MB at K = 256) stays in this CU's L1/L2.
// Level by level of the elimination tree:
//   A. every column of the level (one wave each): 7x7 Cholesky of the diagonal block (lane-redundant,
//      in registers), then one lane per row of its off-diagonal blocks and of its rhs block solves
//      x L_jj^T = a  -> L_ij, and the forward substitution y_j = L_jj^-1 b_j;
//   B. every column j that the level's columns update (one wave each, sources in ascending order):
//      L(i,j) -= L_ik L_jk^T for the rows i >= j of column k, and b_j -= L_jk y_k (right-looking, so
//      the update work of a level runs in parallel instead of on the chain of the column it feeds).
// Then the back substitution x_j = L_jj^-T (y_j - sum_i L_ij^T x_i), levels from the root down; then
// dx = -x in pose order (0 on a failed pivot: the reference's silent zero step), the Sim(3) retraction
// and the |dx| early exit on the device: no host synchronisation inside the GN loop.
// The kernel body is a sequence of parts: sp_stage_tables, sp_init_flags, then either the dataflow schedule
// (sp_flow_factor, sp_flow_back: per-wave task lists, flags instead of barriers) or the level-synchronous loops
// (sp_level_factor, sp_level_back), then sp_finish. Both schedules run the same per-task code (sp_column_task,
// sp_back_column), as do the launched wide steps (ba_sparse_step_kernel): the factor is bit-identical across them.
#include "m3s_ba.h"  // the launchers defined here
#include "m3s_ba_dev.hpp"
#include "ba_pattern.h"  // the host-built half of the plan: BaFlowView (the schedule's layout), BaStepRec, BA_BS_* flags
#include <cstring>

namespace m3s {

__global__ void __launch_bounds__(64) ba_assemble_kernel(BaArgs a, int nL) {
  if (*a.done) return;
  const int b = blockIdx.x, t = threadIdx.x;  // item b: factor block b, or rhs block row b - nL
  if (b == 0 && t == 0) *a.bad = 0;  // the multi-workgroup factor steps of this solve start clean
  int li;
  if (!ba_asm_element(b, nL, t, &li)) return;
  double* out = b < nL ? a.L + (size_t)b * 64 + (t / 7) * 8 + (t - 7 * (t / 7)) : a.y + (size_t)(b - nL) * 8 + t;
  *out = ba_asm_sum(a, b, nL, li);
}

constexpr int SP_WAVES = 16;                 // waves of the factor workgroup
static_assert(SP_WAVES == M3S_BA_SP_WAVES, "the host's schedules assume the kernel's wave count");

// one 8-double row of a factor block (64-B aligned) as four 16-B accesses
__device__ __forceinline__ void ld_row(double (&v)[8], const double* p) {
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const double2 t = reinterpret_cast<const double2*>(p)[q];
    v[2 * q] = t.x;
    v[2 * q + 1] = t.y;
  }
}
__device__ __forceinline__ void st_row(double* p, const double (&v)[8]) {
#pragma unroll
  for (int q = 0; q < 4; q++) reinterpret_cast<double2*>(p)[q] = make_double2(v[2 * q], v[2 * q + 1]);
}

#ifdef M3S_SP_STAMPS  // (experiment builds only) s_memrealtime after every barrier of the factor kernel
__device__ unsigned long long g_sp_stamps[4096];
#define SPST(k)                                                                               \
  do {                                                                                        \
    if (threadIdx.x == 0 && (k) < 3000) g_sp_stamps[k] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#define FST(k)                                                                              \
  do {                                                                                      \
    if (lane == 0) g_sp_stamps[3000 + (k)] = __builtin_amdgcn_s_memrealtime();            \
  } while (0)
#define TST(k)                                                                                   \
  do {                                                                                           \
    if (lane == 0 && (k) < 2000) g_sp_stamps[1000 + (k)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define TST(k) ((void)0)
#define SPST(k) ((void)0)
#define FST(k) ((void)0)
#endif

// the plan's loop tables: the LDS-staged sections of BA_SYM_SECTIONS (ba_pattern.h), typed as in BaArgs
struct SpTables {
#define SP_MEMBER(name, src, lds, cap) decltype(BaArgs::name) name;
  BA_SYM_SECTIONS(SP_MEMBER)  // (only the LDS-staged ones are set and read)
#undef SP_MEMBER
};

// the loop tables at `base`: the plan's table region [plan_lo, plan_lo + plan_bytes) staged to `base` (LDS), or
// base = plan_lo itself (global)
__device__ __forceinline__ SpTables sp_tables(const BaArgs& a, const int* base) {
  const int* g = reinterpret_cast<const int*>(a.plan_lo);
  SpTables T = {};
#define SP_REBASE(name, src, lds, cap) \
  if (lds) T.name = reinterpret_cast<decltype(T.name)>(base + (reinterpret_cast<const int*>(a.name) - g));
  BA_SYM_SECTIONS(SP_REBASE)
#undef SP_REBASE
  return T;
}

// One wave's task: column j, its factor blocks [b0, b1) (diagonal first) and the source range gr of the update
// group it applies. A factor task (A) applies j's pull group, the group of its children's level, if it has one
// (has_g); an update task (B) always applies its own group. From the plan tables (factor kernel) or from one task
// record built with the plan (wide steps).
struct SpTask {
  int j, b0, b1;
  bool has_g;
  int2 gr;
};
__device__ __forceinline__ SpTask sp_task_of_column(const SpTables& T, int j) {
  const int g = T.pull_grp[j];
  const int4 gq = g >= 0 ? T.grp[g] : make_int4(0, 0, 0, 0);
  return SpTask{j, T.col_ptr[j], T.col_ptr[j + 1], g >= 0, make_int2(gq.y, gq.z)};
}
__device__ __forceinline__ SpTask sp_task_of_group(const SpTables& T, int g) {
  const int4 gq = T.grp[g];
  return SpTask{gq.x, T.col_ptr[gq.x], T.col_ptr[gq.x + 1], true, make_int2(gq.y, gq.z)};
}
// the host's restatement of the two above for a launched task (ba_pattern.h ba_step_rec)
__device__ __forceinline__ SpTask sp_task_of_record(const BaStepRec& r) {
  return SpTask{r.j, r.b0, r.b1, r.g >= 0, make_int2(r.src0, r.src1)};
}

// the rows of a column: row p < 7 (noff + 1) is row p % 7 of the column's block p / 7 (block 0 = the
// diagonal block), row 7 (noff + 1) is the rhs block y_j
__device__ __forceinline__ double* sp_row_addr(const BaArgs& a, int b0, int noff, int j, int p) {
  return p < 7 * (noff + 1) ? a.L + (size_t)(b0 + p / 7) * 64 + (p - 7 * (p / 7)) * 8 : a.y + (size_t)j * 8;
}

// the source row of row p of column j for one group source (pl: block of L_jk, k, sidx offset): row p % 7
// of the block of column k at the same block row, y_k for the rhs row, nullptr where struct(k) misses it
__device__ __forceinline__ const double* sp_src_addr(const BaArgs& a, const SpTables& T, const int4& pl, int noff,
                                                     int p) {
  if (p == 7 * (noff + 1)) return a.y + (size_t)pl.y * 8;
  const int sb = T.sidx[pl.z + p / 7];
  return sb >= 0 ? a.L + (size_t)sb * 64 + (p - 7 * (p / 7)) * 8 : nullptr;
}

// v[0..6] -= x L_jk^T with L_jk (49 doubles, row-major 7x7) in LDS: a short dependency tree per output
__device__ __forceinline__ void sp_apply(double (&v)[8], const double (&x)[8], const double* bjk) {
#pragma unroll
  for (int c = 0; c < 7; c++) {
    const double* bc = bjk + c * 7;
    const double p0 = fma(x[0], bc[0], x[1] * bc[1]);
    const double p1 = fma(x[2], bc[2], x[3] * bc[3]);
    const double p2 = fma(x[4], bc[4], x[5] * bc[5]);
    v[c] -= (p0 + p1) + fma(x[6], bc[6], p2);
  }
}

__device__ __forceinline__ double sp_ljk(const BaArgs& a, int blk, int lane) {
  return lane < 49 ? a.L[(size_t)blk * 64 + (lane / 7) * 8 + lane - 7 * (lane / 7)] : 0.0;
}

// one source's step on a held row: the lane's element bv of L_jk into the wave's LDS row bjk (once the previous
// source's reads of it are done), then v -= x L_jk^T where struct(k) has the row (s != nullptr)
__device__ __forceinline__ void sp_stage_apply(double* bjk, double bv, int lane, const double* s, double (&v)[8],
                                               const double (&x)[8]) {
  wave_sync();
  if (lane < 49) bjk[lane] = bv;
  wave_sync();
  if (s) sp_apply(v, x, bjk);
}

// apply the sources of group range gr to the rows p1 = lane and p2 = lane + 64 of column j held in v1 / v2
// (rows beyond nrow are idle). Columns of at most 64 rows (the common case) issue the next source's
// loads before the current one is applied.
__device__ __forceinline__ void sp_group_regs(const BaArgs& a, const SpTables& T, int2 gr, int noff, int nrow,
                                              double (&v1)[8], double (&v2)[8], int lane, double* bjk) {
  if (gr.x >= gr.y) return;
  const int p1 = lane, p2 = lane + 64;
  if (nrow <= 64) {
    int4 pl = T.src[gr.x];
    const double* s1 = p1 < nrow ? sp_src_addr(a, T, pl, noff, p1) : nullptr;
    double bv = sp_ljk(a, pl.x, lane);
    double x1[8];
    if (s1) ld_row(x1, s1);
    for (int e = gr.x; e < gr.y; e++) {
      const bool more = e + 1 < gr.y;
      const double* n1 = nullptr;
      double nbv = 0.0, y1[8];
      if (more) {
        const int4 nl = T.src[e + 1];
        n1 = p1 < nrow ? sp_src_addr(a, T, nl, noff, p1) : nullptr;
        nbv = sp_ljk(a, nl.x, lane);
        if (n1) ld_row(y1, n1);
      }
      sp_stage_apply(bjk, bv, lane, s1, v1, x1);
      s1 = n1;
      bv = nbv;
#pragma unroll
      for (int c = 0; c < 8; c++) x1[c] = y1[c];
    }
  } else {
    for (int e = gr.x; e < gr.y; e++) {
      const int4 pl = T.src[e];
      const double* s1 = sp_src_addr(a, T, pl, noff, p1);
      const double* s2 = p2 < nrow ? sp_src_addr(a, T, pl, noff, p2) : nullptr;
      const double bv = sp_ljk(a, pl.x, lane);
      double x1[8], x2[8];
      if (s1) ld_row(x1, s1);
      if (s2) ld_row(x2, s2);
      sp_stage_apply(bjk, bv, lane, s1, v1, x1);
      if (s2) sp_apply(v2, x2, bjk);
    }
  }
  wave_sync();
}

// rows p >= 128 of the task's column (columns with more than 17 off-diagonal blocks), one pass of 64 rows at a
// time: the task's sources applied, then (when inv != nullptr) the triangular solve with L_jj
__device__ __forceinline__ void sp_rows_extra(const BaArgs& a, const SpTables& T, const SpTask& k, int noff, int nrow,
                                              bool has_g, const double* lo, const double* inv, int lane, double* bjk) {
  for (int base = 128; base < nrow; base += 64) {
    const int p = base + lane;
    const bool act = p < nrow;
    double v[8];
    double* tp = act ? sp_row_addr(a, k.b0, noff, k.j, p) : nullptr;
    if (act) ld_row(v, tp);
    if (has_g) {
      for (int e = k.gr.x; e < k.gr.y; e++) {
        const int4 pl = T.src[e];
        const double bv = sp_ljk(a, pl.x, lane);
        const double* sp = act ? sp_src_addr(a, T, pl, noff, p) : nullptr;
        double x[8];
        if (sp) ld_row(x, sp);
        sp_stage_apply(bjk, bv, lane, sp, v, x);
      }
      wave_sync();
    }
    if (inv) {  // x L_jj^T = a, right-looking
#pragma unroll
      for (int m = 0; m < 7; m++) {
        v[m] *= inv[m];
#pragma unroll
        for (int c = m + 1; c < 7; c++) v[c] = fma(-v[m], lo[c * (c - 1) / 2 + m], v[c]);
      }
    }
    if (act) st_row(tp, v);
  }
}

// One task (one wave): lane p holds row p of the column (v1) and row p + 64 (v2), loaded and stored once; the
// task's group sources are applied first.
// FACTOR (A): then the register-row factorisation: the diagonal rows' right-looking Cholesky steps are, for the rows
// below them, the triangular solve L_ij = A_ij L_jj^-T, and for the rhs row the forward substitution
// y_j = L_jj^-1 b_j. Diagonal block afterwards: lower = L_jj, column 7 = 1/L_mm.
// !FACTOR (B): the update group alone.
template <bool FACTOR>
__device__ __forceinline__ void sp_column_task(const BaArgs& a, const SpTables& T, const SpTask& k, int lane,
                                               double* bjk, int* bad) {
  const int noff = k.b1 - k.b0 - 1, nrow = 7 * (noff + 1) + 1;
  const bool has1 = lane < nrow, has2 = lane + 64 < nrow;
  double v1[8], v2[8];
  double* p1 = has1 ? sp_row_addr(a, k.b0, noff, k.j, lane) : nullptr;
  double* p2 = has2 ? sp_row_addr(a, k.b0, noff, k.j, lane + 64) : nullptr;
  if (has1) ld_row(v1, p1);
  if (has2) ld_row(v2, p2);
  const bool has_g = !FACTOR || k.has_g;
  if (has_g) sp_group_regs(a, T, k.gr, noff, nrow, v1, v2, lane, bjk);
  double inv[7], lo[21];
  if constexpr (FACTOR) {
    bool fail = false;
#pragma unroll
    for (int m = 0; m < 7; m++) {
      double d = bcast_lane(v1[m], m);
      if (!(d > 0.0)) {  // not positive definite: the step is discarded (dx = 0), as SimplicialLLT's info
        fail = true;
        d = 1.0;
      }
      inv[m] = rsqrt_nr(d);
      const double l1 = v1[m] * inv[m], l2 = v2[m] * inv[m];
      v1[m] = lane == m ? d * inv[m] : l1;
      v2[m] = l2;
#pragma unroll
      for (int c = m + 1; c < 7; c++) {
        const double lc = bcast_lane(l1, c);
        lo[c * (c - 1) / 2 + m] = lc;
        v1[c] = fma(-l1, lc, v1[c]);
        v2[c] = fma(-l2, lc, v2[c]);
      }
    }
    if (fail && lane == 0) atomicOr(bad, BA_BAD_LLT);
    if (lane < 7) {  // 1/L_mm in column 7 of the diagonal block (used by the back substitution)
      double iv = inv[0];
#pragma unroll
      for (int m = 1; m < 7; m++) iv = lane == m ? inv[m] : iv;
      v1[7] = iv;
    }
  }
  if (has1) st_row(p1, v1);
  if (has2) st_row(p2, v2);
  if (nrow > 128) sp_rows_extra(a, T, k, noff, nrow, has_g, FACTOR ? lo : nullptr, FACTOR ? inv : nullptr, lane, bjk);
}

// ---- dataflow schedule (ba_pattern.h ba_flow_schedule): flags in LDS instead of a barrier per level ----
// Producers publish with a workgroup-scope release (their global stores of factor blocks, or LDS writes of x,
// complete first); consumers spin on an acquire load. All waves of the workgroup share one CU and its L1.
__device__ __forceinline__ int flow_ld(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void flow_st(int* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The wave waits until no lane's pending() holds. Spins are bounded (~2^20 polls, tens of ms): a schedule that could
// not complete sets the STALL bit of `bad` (BA_BAD_STALL: dx = 0, the GN loop ends, and the host returns M3S_ESTALL)
// instead of hanging the workgroup. A wait abandoned because another wave already failed (a non-positive pivot,
// BA_BAD_LLT) is not a stall. False when the wait was given up either way.
constexpr int FLOW_MAX_SPINS = 1 << 20;
template <class Pending>
__device__ __forceinline__ bool flow_spin(Pending pending, int lane, int* bad) {
  int spins = 0;
  while (__ballot(pending()) != 0) {
    __builtin_amdgcn_s_sleep(1);
    if (*(volatile int*)bad) return false;  // already failed (or stalled) elsewhere: stop waiting
    if (++spins > FLOW_MAX_SPINS) {
      if (lane == 0) atomicOr(bad, BA_BAD_STALL);
      return false;
    }
  }
  return true;
}

// wait until every source column of group range gr is factored and `cnt` reads q; wave-uniform.
// force_stall (M3S_BA_FORCE_STALL, tests only): the wait is never satisfied.
__device__ __forceinline__ void flow_wait_task(const SpTables& T, int2 gr, const int* fac, const int* cnt, int q,
                                               int lane, int* bad, bool force_stall) {
  const int ns = gr.y - gr.x;
  for (int base = 0; base == 0 || base < ns; base += 63) {
    const bool cs = lane < 63 && base + lane < ns;
    const int k = cs ? T.src[gr.x + base + lane].y : 0;
    const bool cc = lane == 63 && base == 0;
    if (!flow_spin([&] { return (cs && flow_ld(&fac[k]) == 0) || (cc && flow_ld(cnt) != q) || force_stall; }, lane,
                   bad))
      return;
  }
}

// back substitution of column j: x_j = L_jj^-T (y_j - sum_{i in struct(j)} L_ij^T x_i); X = the solution
// (LDS when it fits), 8 doubles per column. Lane (q, m) sums column m of the blocks b0 + 1 + q, + 9, ... in that
// order, then the 9 partial sums in a fixed order (deterministic). Dataflow schedule (xd: the x-done flags): the
// lane's first two blocks are loaded ahead of the `wait` for x of struct(j), and xd[j] is published. Level-synchronous
// loop: xd = nullptr (the barriers order the columns). Same arithmetic in the same order either way (bit-identical x).
__device__ __forceinline__ void sp_back_column(const BaArgs& a, const SpTables& T, double* X, int* xd, int j,
                                               bool wait, int lane, double* red, int* bad) {
  const int b0 = T.col_ptr[j], b1 = T.col_ptr[j + 1];
  const int q = lane / 7, m = lane - 7 * (lane / 7);
  const double* D = a.L + (size_t)b0 * 64;
  double dl[8][8];  // L_jj (lower) and 1/L_mm (column 7), issued before the sums
#pragma unroll
  for (int r = 0; r < 7; r++) {
    double row[8];
    ld_row(row, D + r * 8);
#pragma unroll
    for (int c = 0; c < 8; c++) dl[r][c] = row[c];
  }
  const double yv = lane < 7 ? a.y[(size_t)j * 8 + lane] : 0.0;
  int b = b0 + 1 + q;
  double acc = 0.0;
  if (xd) {
    const int bA = b, bB = b + 9;
    const bool hA = lane < 63 && bA < b1, hB = lane < 63 && bB < b1;
    double LA[7], LB[7];
#pragma unroll
    for (int r = 0; r < 7; r++) {
      LA[r] = hA ? a.L[(size_t)bA * 64 + m + r * 8] : 0.0;
      LB[r] = hB ? a.L[(size_t)bB * 64 + m + r * 8] : 0.0;
    }
    const int iA = hA ? T.rowL[bA] : 0, iB = hB ? T.rowL[bB] : 0;
    for (int base = b0 + 1; wait && (base == b0 + 1 || base < b1); base += 64) {
      const bool c = base + lane < b1;
      const int i = c ? T.rowL[base + lane] : 0;
      if (!flow_spin([&] { return c && flow_ld(&xd[i]) == 0; }, lane, bad)) break;
    }
    if (hA) {
      const double* xi = X + (size_t)iA * 8;
#pragma unroll
      for (int r = 0; r < 7; r++) acc = fma(LA[r], xi[r], acc);
    }
    if (hB) {
      const double* xi = X + (size_t)iB * 8;
#pragma unroll
      for (int r = 0; r < 7; r++) acc = fma(LB[r], xi[r], acc);
    }
    b += 18;
  }
  if (lane < 63)
    for (; b < b1; b += 9) {
      const double* Lb = a.L + (size_t)b * 64 + m;
      const double* xi = X + (size_t)T.rowL[b] * 8;
#pragma unroll
      for (int r = 0; r < 7; r++) acc = fma(Lb[r * 8], xi[r], acc);
    }
  red[lane] = acc;
  wave_sync();
  if (lane < 7) {
    double sacc = yv;
#pragma unroll
    for (int qq = 0; qq < 9; qq++) sacc -= red[qq * 7 + lane];  // fixed order: deterministic
    red[lane] = sacc;
  }
  wave_sync();
  double z[7];
#pragma unroll
  for (int mm = 0; mm < 7; mm++) z[mm] = red[mm];
  double x[7];
#pragma unroll
  for (int mm = 6; mm >= 0; mm--) {
    double vv = z[mm];
#pragma unroll
    for (int p = mm + 1; p < 7; p++) vv = fma(-dl[p][mm], x[p], vv);
    x[mm] = vv * dl[mm][7];
  }
  if (lane == 0) {
#pragma unroll
    for (int mm = 0; mm < 7; mm++) X[(size_t)j * 8 + mm] = x[mm];
    if (xd) flow_st(&xd[j], 1);
  }
  wave_sync();
}

// One wide factor step l of the elimination tree (its level's factor tasks + the update groups whose sources
// sit one level below) as a multi-workgroup launch: one wave per task, the same per-task code and therefore
// the same arithmetic as inside ba_sparse_factor_kernel (bit-identical factor). The launch boundary orders
// the steps. The leaf end of a minimum-degree tree is wide (one workgroup's 16 waves took ~12 rounds per
// step there), the root end a chain of single columns, which stays inside the one-workgroup kernel.
// Each task reads one 32-B record built with the plan (sp_task_of_record), in the same round trip as the early-exit
// flag: the level / column / group table lookups that used to precede the column's own loads (four dependent global
// round trips) are gone.
__global__ void __launch_bounds__(64) ba_sparse_step_kernel(BaArgs a, int rec_base, int na, int xcd_stride) {
  __shared__ double s_red[64];
  const int lane = threadIdx.x;
  // xcd_stride 8 (M3S_BA_XCD0, default): only the blocks dispatched to XCD 0 (blockIdx % 8 == 0) work, so every
  // step and the one-workgroup kernel share one XCD's L2
  if (xcd_stride > 1 && blockIdx.x % xcd_stride != 0) return;
  const int task = blockIdx.x / xcd_stride;
  const BaStepRec r = a.step_rec[rec_base + task];
  if (*a.done) return;
  const SpTables T = sp_tables(a, reinterpret_cast<const int*>(a.plan_lo));
  if (task < na) sp_column_task<true>(a, T, sp_task_of_record(r), lane, s_red, a.bad);
  else sp_column_task<false>(a, T, sp_task_of_record(r), lane, s_red, a.bad);
}

// ---- ba_sparse_factor_kernel in parts: each is called once, in this order, by every thread of the workgroup ----

// the plan's LDS-staged sections [plan_lo, plan_lo + plan_bytes) into s_plan: every thread's loads in flight at once
__device__ __forceinline__ void sp_stage_tables(const BaArgs& a, int* s_plan) {
  const int4* src = reinterpret_cast<const int4*>(a.plan_lo);
  int4* dst = reinterpret_cast<int4*>(s_plan);
  const int n16 = (a.plan_bytes + 15) / 16;
  int4 tmp[8];
  for (int i0 = 0; i0 < n16; i0 += 8 * 1024) {
#pragma unroll
    for (int u = 0; u < 8; u++) tmp[u] = src[min(i0 + u * 1024 + (int)threadIdx.x, n16 - 1)];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int i = i0 + u * 1024 + (int)threadIdx.x;
      if (i < n16) dst[i] = tmp[u];
    }
  }
}

// the dataflow flags (LDS, after x), one word per column each
struct SpFlags {
  int* app;  // update groups landed on the column
  int* fac;  // the column is factored
  int* xd;   // its x is solved
};
// fac starts from the global schedule's fac_init (the staged copy is not visible before the barrier that follows)
__device__ __forceinline__ void sp_init_flags(const BaArgs& a, const SpFlags& F, int nb) {
  const int* fac_init = BaFlowView{a.sched, SP_WAVES, nb}.fac_init();
  for (int i = threadIdx.x; i < nb; i += 1024) {
    F.app[i] = 0;
    F.fac[i] = fac_init[i];
    F.xd[i] = 0;
  }
}

// dataflow factor walk: wave w walks its own task list (step order); a task waits only for its inputs
__device__ __forceinline__ void sp_flow_factor(const BaArgs& a, const SpTables& T, const BaFlowView& S,
                                               const SpFlags& F, int w, int lane, double* red, int* bad) {
  const int2* wl = reinterpret_cast<const int2*>(S.wl_task());
  for (int t = S.wl_ptr()[w]; t < S.wl_ptr()[w + 1]; t++) {
    const int2 tk = wl[t];  // {column j, or -1 - update group; the count of groups j took before this task}
    if (tk.x >= 0) {
      const SpTask k = sp_task_of_column(T, tk.x);
      flow_wait_task(T, k.gr, F.fac, &F.app[k.j], tk.y, lane, bad, a.force_stall);
      TST(2 * t);
      sp_column_task<true>(a, T, k, lane, red, bad);
      if (lane == 0) flow_st(&F.fac[k.j], 1);
    } else {
      const SpTask k = sp_task_of_group(T, -1 - tk.x);
      flow_wait_task(T, k.gr, F.fac, &F.app[k.j], tk.y, lane, bad, a.force_stall);
      TST(2 * t);
      sp_column_task<false>(a, T, k, lane, red, bad);
      if (lane == 0) flow_st(&F.app[k.j], tk.y + 1);
    }
    TST(2 * t + 1);
    wave_sync();
  }
}

// dataflow back substitution: wave w's columns, parents first, each waiting on the x-done flags of its struct
__device__ __forceinline__ void sp_flow_back(const BaArgs& a, const SpTables& T, const BaFlowView& S, double* X,
                                             const SpFlags& F, int w, int lane, double* red, int* bad) {
  const int* bs_col = S.bs_col();
  for (int t = S.bs_ptr()[w]; t < S.bs_ptr()[w + 1]; t++) {
    const int code = bs_col[t];
    sp_back_column(a, T, X, F.xd, code & BA_BS_COL, (code & BA_BS_NOWAIT) == 0, lane, red, bad);
    FST(t);
  }
}

// level-synchronous factor, steps [wide_steps, nlev]. Step l: factor the columns of level l (each pulls its
// children's-level updates first) beside the push updates of level l-1 into the columns above level l; a barrier
// ends every step
__device__ __forceinline__ void sp_level_factor(const BaArgs& a, const SpTables& T, int w, int lane, double* red,
                                                int* bad) {
  const int nlev = a.nlev;
  for (int l = a.wide_steps; l <= nlev; l++) {
    const int c0 = l < nlev ? T.lev_ptr[l] : 0, na = l < nlev ? T.lev_ptr[l + 1] - c0 : 0;
    const int t0 = T.grp_ptr[l], nt = T.grp_ptr[l + 1] - t0;
    for (int task = w; task < na + nt; task += SP_WAVES) {
      if (task < na) sp_column_task<true>(a, T, sp_task_of_column(T, T.lev_col[c0 + task]), lane, red, bad);
      else sp_column_task<false>(a, T, sp_task_of_group(T, t0 + task - na), lane, red, bad);
    }
    __syncthreads();
    SPST(2 + l);
  }
}

// level-synchronous back substitution, levels from the root down; runs of single-column levels stay on wave 0 with
// no barrier between them (LT, X in LDS: a wave's LDS accesses are ordered)
template <bool LT>
__device__ __forceinline__ void sp_level_back(const BaArgs& a, const SpTables& T, double* X, int w, int lane,
                                              double* red, int* bad) {
  const int nlev = a.nlev;
  for (int l = nlev - 1; l >= 0; l--) {
    const int c0 = T.lev_ptr[l], c1 = T.lev_ptr[l + 1];
    for (int c = c0 + w; c < c1; c += SP_WAVES) sp_back_column(a, T, X, nullptr, T.lev_col[c], false, lane, red, bad);
    const bool chain = LT && c1 - c0 == 1 && l > 0 && T.lev_ptr[l] - T.lev_ptr[l - 1] == 1;
    if (!chain) {
      __syncthreads();
      SPST(3 + nlev + (nlev - 1 - l));
    }
  }
}

// dx = -x in pose order (0 on a failed pivot or a stall), the retraction and the early exit; the multi-workgroup
// factor launches (the wide steps) report through *a.bad
__device__ __forceinline__ void sp_finish(const BaArgs& a, const double* X, int K, float delta_thresh, int bad) {
  const int ext_bad = a.wide_steps > 0 ? *(volatile int*)a.bad : 0;
  const bool failed = bad != 0 || ext_bad != 0;
  ba_finish_step<8>(a, X, K, delta_thresh, failed, ((bad | ext_bad) & BA_BAD_STALL) != 0);
  if (threadIdx.x == 0) *a.info = failed ? 1 : 0;
}

template <bool LT>  // LT: the loop tables and x fit in LDS (index lookups are ds_reads), else global
__global__ void __launch_bounds__(1024) ba_sparse_factor_kernel(BaArgs a, int K, int nL, float delta_thresh) {
  if (*a.done) return;
  __shared__ __attribute__((aligned(16))) int s_plan[LT ? SP_PLAN_BYTES / 4 : 4];
  __shared__ double s_red[SP_WAVES][64];  // per-wave staging: L_jk and the back-substitution sums
  __shared__ int s_bad;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  SPST(0);
  if constexpr (LT) sp_stage_tables(a, s_plan);
  const int xoff = ((a.plan_bytes + 15) & ~15) / 4;  // ints: x follows the tables, the flags follow x
  double* X = LT ? reinterpret_cast<double*>(s_plan + xoff) : a.xs;
  const SpTables T = sp_tables(a, LT ? static_cast<const int*>(s_plan) : reinterpret_cast<const int*>(a.plan_lo));
  const int nb = a.nb;
  const SpFlags F = {s_plan + xoff + 16 * nb, s_plan + xoff + 17 * nb, s_plan + xoff + 18 * nb};
  const bool flow = LT && a.flow;
  if (flow) sp_init_flags(a, F, nb);
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  SPST(1);
  if (flow) {
    const BaFlowView S{T.sched, SP_WAVES, nb};
    sp_flow_factor(a, T, S, F, w, lane, s_red[w], &s_bad);
    __syncthreads();
    SPST(2 + a.nlev);
    sp_flow_back(a, T, S, X, F, w, lane, s_red[w], &s_bad);
  } else {
    sp_level_factor(a, T, w, lane, s_red[w], &s_bad);
    sp_level_back<LT>(a, T, X, w, lane, s_red[w], &s_bad);
  }
  __syncthreads();
  SPST(3 + 2 * a.nlev);
  sp_finish(a, X, K, delta_thresh, s_bad);
  SPST(4 + 2 * a.nlev);
}

}  // namespace m3s

#ifdef M3S_SP_STAMPS
extern "C" int m3s_debug_sp_stamps(unsigned long long* out) {
  (void)hipDeviceSynchronize();
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(m3s::g_sp_stamps), sizeof(unsigned long long) * 4096) == hipSuccess ? 0 : -1;
}
#endif

// XCD affinity of the solve (M3S_BA_XCD0, default on): every multi-workgroup factor step and the one-workgroup kernel
// (block 0) run on XCD 0, so each step reads the previous one's blocks from that XCD's L2 instead of across the
// fabric. Measured (scripts/gpu_r05_xcd.sh, same box, two pairs): solve C5 0.393 -> 0.375 ms, C4 0.424 -> 0.409 ms.
// The stride assumes the round-robin workgroup dispatch over 8 XCDs of an MI3xx part in SPX mode (one device = the
// whole package): it is used only when the device is a gfx94x / gfx950 that reports at least 8 x 32 CUs. A partition
// (CPX: one XCD per device, 32 CUs) or any other part gets stride 1, where the 7 of 8 idle blocks would be wasted
// dispatches and the L2 locality would not exist.
static int ba_xcd_stride() {
  static const int xs = [] {
    const char* e = getenv("M3S_BA_XCD0");
    if (e && atoi(e) == 0) return 1;
    int dev = 0, cus = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 1;
    cus = prop.multiProcessorCount;
    const bool mi3xx = strncmp(prop.gcnArchName, "gfx94", 5) == 0 || strncmp(prop.gcnArchName, "gfx950", 6) == 0;
    return (mi3xx && cus >= 8 * 32 && cus % 8 == 0) ? 8 : 1;
  }();
  return xs;
}

// assembly (nL factor blocks + nb rhs rows), the wide steps (steps[l]: ba_pattern.h BaWideStep), then the one-workgroup
// factor / solve / retraction
extern "C" hipError_t m3s_launch_ba_solve(const BaArgs* a, int K, int nL, float delta_thresh, const BaWideStep* steps,
                                          hipStream_t s) {
  const int xs = ba_xcd_stride();
  // the assembly stays spread over every XCD: pinned to XCD 0 (32 CUs, item-strided) it took longer than the L2 reads
  // it saved the first step (solve C5 0.381 vs 0.375 ms)
  if (a->nb > 0) hipLaunchKernelGGL(m3s::ba_assemble_kernel, dim3(nL + a->nb), dim3(64), 0, s, *a, nL);
  for (int l = 0; l < a->wide_steps; l++)
    if (steps[l].tasks > 0)
      hipLaunchKernelGGL(m3s::ba_sparse_step_kernel, dim3(steps[l].tasks * xs), dim3(64), 0, s, *a, steps[l].base,
                         steps[l].na, xs);
  // the tables, x and the flags in LDS when they fit (m3s_ba.h ba_sp_lds_bytes), else the global-table instance
  if (m3s::ba_sp_lds_bytes(a->plan_bytes, a->nb, a->flow != 0) <= (size_t)m3s::SP_PLAN_BYTES)
    hipLaunchKernelGGL(m3s::ba_sparse_factor_kernel<true>, dim3(1), dim3(1024), 0, s, *a, K, nL, delta_thresh);
  else
    hipLaunchKernelGGL(m3s::ba_sparse_factor_kernel<false>, dim3(1), dim3(1024), 0, s, *a, K, nL, delta_thresh);
  return hipGetLastError();
}
