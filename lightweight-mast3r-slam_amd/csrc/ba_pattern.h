// Host-side symbolic analysis of the BA pose system (internal, not ABI).
//
// The reference assembles the pose system as Eigen triplets and factors it with SimplicialLLT
// (/root/reference/mast3r_slam/backend/src/gn_kernels.cu:57-159), re-analysing the pattern on every GN
// iteration. Here the pattern is analysed ONCE per plan, at 7x7-block granularity (one block per
// keyframe pose), and the numeric factorisation of every GN iteration runs on the device
// (ba_sparse_factor_kernel, ba_sparse.hip):
//   * ordering: minimum degree on the keyframe graph (ties to the lowest index), which keeps the fill of
//     the long chain + loop-closure graphs of SLAM small (K = 256 chess graph: 1922 factor blocks
//     instead of 32640 dense, elimination tree height 68 instead of 255);
//   * the factor's block columns, their levels in the elimination tree (a column's level is one more
//     than its highest child's), and the update work grouped per (source level, target column): one
//     wave owns each group (sources ascending), so every column's update order is fixed
//     (deterministic: identical on every rank); a column's children's-level group runs inside its own
//     factor task, right before it factors;
//   * the assembly CSR in factor-block order: the contributions (edge*2 + sign) of each block, in edge
//     order, and the rhs contributions per (new) block row.
#pragma once
#include <cstddef>
#include <string>
#include <vector>

#ifdef __HIPCC__  // this header is also compiled by a plain host compiler (ba_pattern.cpp, scripts/ba_flow_check.cpp)
#define BA_HD __host__ __device__
#else
#define BA_HD
#endif

struct BaPattern {
  int nb = 0;    // block columns (poses without the pinned one)
  int nL = 0;    // factor blocks (diagonal included)
  int nlev = 0;  // elimination-tree levels
  bool too_dense = false;  // the update source map outgrew max_sidx: the build stopped early (tables incomplete)
  std::vector<int> perm;      // (nb) new column -> old (pin-removed) pose index
  std::vector<int> col_ptr;   // (nb+1) factor blocks of column j: [col_ptr[j], col_ptr[j+1]), first = diagonal
  std::vector<int> rowL;      // (nL) block row (new index) of each factor block
  std::vector<int> lev_ptr;   // (nlev+1) into lev_col
  std::vector<int> lev_col;   // (nb) columns grouped by level, ascending within a level
  std::vector<int> grp_ptr;   // (nlev+2) into grp: the update groups of step s (sources at level s-1)
  std::vector<int> grp;       // int4 {target column j, src begin, src end, 0}; the factor tasks' own groups follow
  std::vector<int> pull_grp;  // (nb) group of column j's children's level, run by its factor task, or -1
  std::vector<int> src;       // int4 {block of L_jk in column k, k, sidx offset, 0}
  std::vector<int> sidx;      // per group source, per block b of column j: the block of column k at row rowL[b], or -1
  std::vector<int> asm_ptr;   // (nL+1) into asm_ent
  std::vector<int> asm_ent;   // edge*2 + (1 if the block takes -M)
  std::vector<int> rhs_ptr;   // (nb+1) per new block row, into rhs_ent
  std::vector<int> rhs_ent;   // edge*2 + (1 if the row takes -g)
};

// ri, rj: dense pose ranks (pin 0 = rank 0 is fixed) of the E directed edges; Kp poses. max_sidx bounds the
// update source map (the plan's table capacity, < INT_MAX): past it the build stops with too_dense set, before a
// dense large graph can exhaust host memory.
void ba_build_pattern(const int* ri, const int* rj, int E, int Kp, BaPattern* P, size_t max_sidx = (size_t)1 << 30);

// Dataflow schedule of the one-workgroup part of the numeric factorisation (steps [wide, nlev]) and of the whole
// back substitution: instead of a barrier per elimination-tree level, every wave of the workgroup walks its own
// task list and waits only on the tasks its inputs come from (flags in LDS). Lists come from a list-scheduling
// simulation over the task graph (estimated task costs, a penalty for a cross-wave hand-off), tasks in step order
// within every list, so the earliest unfinished task is always runnable (no deadlock). Per target column the
// update groups still apply in step order (a per-column counter), so the factor is bit-identical to the
// level-synchronous schedule.
#define BA_BS_NOWAIT (1 << 30)
#define BA_BS_COL 0xFFFFFF
// Returns the simulated finish time (us) of the factor part (the cost model's estimate).
double ba_flow_schedule(const BaPattern& P, int wide, int waves, std::vector<int>* sched);

// The schedule's layout (ints), the one place that knows it: the host fills it, the kernel and the checker read it
// and the plan's capacity bound sizes it through this view.
//   [wl_ptr waves+1] [bs_ptr waves+1] [fac_init nb] [wl_task 2 x ntask] [bs_col nb]
// wl_ptr / bs_ptr: each wave's range of wl_task / bs_col; ntask = wl_ptr[waves].
// wl_task = {code, q}: code >= 0 factors column code after q update groups landed on it; code < 0 runs update
// group -1 - code once q earlier groups landed on its target. fac_init[k] = 1 for columns factored by the
// multi-workgroup steps [0, wide). bs_col: back-substitution columns per wave, descending (parents first).
// bs_col entries carry BA_BS_NOWAIT when the wave's previous column is the parent (or the column is a root): struct(j)
// minus the parent lies in struct(parent), which the parent already waited for, so x_j needs no wait; the column is
// the low 24 bits.
template <class Int>
struct BaFlowViewT {
  Int* s;
  int waves, nb;
  BA_HD Int* wl_ptr() const { return s; }
  BA_HD Int* bs_ptr() const { return s + waves + 1; }
  BA_HD Int* fac_init() const { return s + 2 * (waves + 1); }
  BA_HD Int* wl_task() const { return s + 2 * (waves + 1) + nb; }
  BA_HD int ntask() const { return s[waves]; }
  BA_HD Int* bs_col() const { return s + 2 * (waves + 1) + nb + 2 * s[waves]; }
  BA_HD static size_t ints(int waves, size_t nb, size_t ntask) { return 2 * ((size_t)waves + 1) + nb + 2 * ntask + nb; }
};
using BaFlowView = BaFlowViewT<const int>;

// ---- the symbolic half of a BA plan: everything the solve needs from the host, as one packed image ----
#ifndef M3S_BA_SP_WAVES
#define M3S_BA_SP_WAVES 16  // waves of the one-workgroup sparse factorisation (ba_sparse.hip) and of its cost model
#endif
constexpr int BA_MAX_WIDE_STEPS = 40;
namespace m3s {
constexpr int SP_PLAN_BYTES = 144 * 1024;  // LDS of the one-workgroup factor kernel: the plan's loop tables and x
// What that kernel keeps in LDS for a plan: the loop tables (plan_bytes: the LDS-staged sections below; padded to
// 16 B), x (8 doubles per column) and, for the dataflow schedule, 3 flag words per column. A plan that needs more
// than SP_PLAN_BYTES runs the global-table instance, level-synchronously: the host (ba_build_plan) drops its
// schedule by this rule and the launcher (m3s_launch_ba_solve) picks the instance by it.
inline size_t ba_sp_lds_bytes(size_t plan_bytes, int nb, bool flow) {
  return ((plan_bytes + 15) & ~(size_t)15) + (size_t)nb * 64 + (flow ? (size_t)nb * 12 : 0);
}
}  // namespace m3s

// One task of a launched wide step (ba_sparse_step_kernel): what sp_task_of_column / sp_task_of_group would read
// from the tables, so a launched task starts with its column's own loads. The writer and the device reader
// (sp_task_of_record, ba_sparse.hip) name the fields; their order exists here only.
struct alignas(16) BaStepRec {
  int j, b0, b1;   // column, its factor blocks [b0, b1)
  int g;           // the group the task applies (a factor task: its pull group, or -1)
  int src0, src1;  // that group's source range (0, 0 without one)
  int pad[2];
};
static_assert(sizeof(BaStepRec) == 32, "two int4 per task record");
inline BaStepRec ba_step_rec(const BaPattern& S, int j, int g) {
  const int* gq = g >= 0 ? &S.grp[4 * (size_t)g] : nullptr;
  return BaStepRec{j, S.col_ptr[j], S.col_ptr[j + 1], g, gq ? gq[1] : 0, gq ? gq[2] : 0, {0, 0}};
}
struct BaWideStep {
  int base, na, tasks;  // first task record, factor tasks (update groups follow), all tasks
};

// The image's sections in packing order, the ONE list of them: X(BaArgs member, source in BaPlanSources, staged into
// LDS by the factor kernel, worst-case ints given nb, nLmax, E, max_pairs, waves). The packing loop, the BaArgs
// pointers (abi_ba.cpp with_symbolic), the LDS-staged range [plan_lo, plan_lo + plan_bytes) and the capacity bound
// all expand it. The LDS-staged sections must stay contiguous (sp_tables rebases them by one offset).
#define BA_SYM_SECTIONS(X)                                                                                 \
  X(perm, S.perm, 0, nb)                                                                                   \
  X(col_ptr, S.col_ptr, 1, nb + 1)                                                                         \
  X(rowL, S.rowL, 1, nLmax)                                                                                \
  X(lev_ptr, S.lev_ptr, 1, nb + 1)                                                                         \
  X(lev_col, S.lev_col, 1, nb)                                                                             \
  X(grp_ptr, S.grp_ptr, 1, nb + 2)                                                                         \
  X(grp, S.grp, 1, 4 * nLmax)                                                                              \
  X(pull_grp, S.pull_grp, 1, nb)                                                                           \
  X(src, S.src, 1, 4 * nLmax)                                                                              \
  X(sidx, S.sidx, 1, max_pairs)                                                                            \
  X(sched, sched, 1, BaFlowView::ints(waves, nb, nb + nLmax)) /* a task per column and per update group */ \
  X(asm_ptr, S.asm_ptr, 0, nLmax + 1)                                                                      \
  X(asm_ent, S.asm_ent, 0, 4 * E)                                                                          \
  X(rhs_ptr, S.rhs_ptr, 0, nb + 1)                                                                         \
  X(rhs_ent, S.rhs_ent, 0, 2 * E)                                                                          \
  X(step_rec, step_rec, 0, 8 * 2 * nb * (nb + 1 < BA_MAX_WIDE_STEPS ? nb + 1 : BA_MAX_WIDE_STEPS))
#define BA_SEC_ENUM(name, src, lds, cap) BA_SEC_##name,
enum { BA_SYM_SECTIONS(BA_SEC_ENUM) BA_SYM_NSEC };
#undef BA_SEC_ENUM
// ints the symbolic sections can take at most (m3s_ba_workspace_size reserves them)
inline size_t ba_sym_capacity_ints(size_t nb, size_t nLmax, size_t E, size_t max_pairs, int waves) {
  size_t n = 0;
#define BA_SEC_CAP(name, src, lds, cap) n += (cap);
  BA_SYM_SECTIONS(BA_SEC_CAP)
#undef BA_SEC_CAP
  return n;
}

// what the sections are packed from (kept only by callers that ask for it: the host checker)
struct BaPlanSources {
  BaPattern S;
  std::vector<int> sched;     // BaFlowView layout, empty without the dataflow schedule
  std::vector<int> step_rec;  // BaStepRec per task of steps [0, min(nlev + 1, BA_MAX_WIDE_STEPS))
};
struct BaPlanOptions {
  bool has_dense = false;  // the dense solve is available (its workspace exists)
  int solver = 0;          // 0: the measured cost rule, 1: sparse, 2: dense (M3S_BA_SOLVER)
  bool wide_by_thr = false;  // the wide steps reach the last one with more than wide_thr tasks (M3S_BA_WIDE), else by cost
  int wide_thr = 0;
  bool flow = true;        // dataflow schedule (M3S_BA_FLOW)
  size_t max_pairs = (size_t)1 << 30;  // bound of the update source map (ba_build_pattern max_sidx)
  size_t capacity = ~(size_t)0;        // bytes the image may take
};
struct BaSymPlan {
  std::vector<char> image;  // the sections, each at off[BA_SEC_*] (16-B aligned), as uploaded
  size_t off[BA_SYM_NSEC] = {0};
  int nb = 0, nlev = 0, nL = 0, wide_steps = 0, dense = 0, flow = 0;
  int plan_lo_off = 0, plan_bytes = 0;  // the LDS-staged sections: [first's offset, last's end)
  BaWideStep steps[BA_MAX_WIDE_STEPS] = {};
};
// ranks ri / rj of all E edges -> the plan: pattern, the sparse / dense cost rule, the wide split, the task records,
// the schedule with its LDS-fit rule, and the packed image. False with *err set when the pattern outgrows the tables.
bool ba_build_plan(const int* ri, const int* rj, int E, int Kp, const BaPlanOptions& opt, BaSymPlan* Y,
                   std::string* err, BaPlanSources* keep = nullptr);
