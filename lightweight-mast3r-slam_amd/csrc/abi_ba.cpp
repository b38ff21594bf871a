// C ABI of libm3s.so (include/m3s.h): bundle adjustment. The plan (rank remap, record reuse, linearisation table,
// one upload), the symbolic worker (its thread, generation and upload; what it computes is ba_build_plan), and the
// linearise / solve entry points. Kernels live in ba.hip (linearisation), ba_sparse.hip and ba_dense.hip (the solves),
// the pattern analysis and the plan's host-built half (the BA_SYM_SECTIONS image) in ba_pattern.cpp.
#include "abi_common.h"

#include <algorithm>
#include <future>
#include <map>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "m3s_ba.h"
#include "ba_pattern.h"

using namespace m3s_abi;

// The pixel-ray tables of raw calib (m3s_ba_calib_rays): x_of_u[u] = (float(u) - cx) / fx, y_of_v[v] = (float(v) - cy)
// / fy, each one fp32 subtraction then one correctly rounded fp32 division: geometry.backproject's operation order on a
// torch device with K on that device, so z * table entry is constrain_points_to_ray's value bit for bit. The volatile
// intermediates pin that order: no reciprocal-multiply, no fused or widened evaluation whatever the host flags.
void m3s_abi::ba_calib_rays(const m3s_ba_config* cfg, float* x_of_u, float* y_of_v) {
  for (int u = 0; u < cfg->width; u++) {
    volatile float d = (float)u - cfg->cx;
    volatile float q = d / cfg->fx;
    x_of_u[u] = q;
  }
  for (int v = 0; v < cfg->height; v++) {
    volatile float d = (float)v - cfg->cy;
    volatile float q = d / cfg->fy;
    y_of_v[v] = q;
  }
}

namespace {

struct BaPlanImpl {
  BaArgs a;
  BaParams p;
  int Kp, N, E, e0, e1;
  int n_targets;  // distinct target keyframes j among this shard's edges (their X_j slabs are streamed per iteration)
  float delta_thresh;
  size_t edge_sums_off, edge_sums_bytes;
  void* ws;
  unsigned long long sym_gen;  // the PlanSym (symbolic half) this plan owns, by generation
  int n_packed, n_dirty;       // edges the pack wrote, keyframes found changed (record reuse; all without it)
};
static_assert(sizeof(BaPlanImpl) <= sizeof(m3s_ba_plan), "m3s_ba_plan too small");

// points of one keyframe per linearisation block: 24576 x 12 B = 295 KB of X_j, so the ~100 blocks an XCD
// runs at once (the edges of a few target keyframes, same chunk) share their X_j slabs in its 4 MiB L2. Small
// graphs (the early-sequence global optimisations) would leave most CUs idle at that length: their chunks
// shrink (down to 4096 points, 8 rounds per lane) until E x chunks reaches 512 blocks. A function of the
// FULL edge count, so every rank of a sharded solve cuts its edges exactly like the unsharded one.
// M3S_BA_CHUNK_POINTS (tests): a fixed chunk length instead.
constexpr int BA_CHUNK_POINTS = 24576, BA_CHUNK_MIN_POINTS = 4096, BA_LIN_MIN_BLOCKS = 512;
int ba_chunks(int N, int E) {
  const int base = std::max(1, (N + BA_CHUNK_POINTS - 1) / BA_CHUNK_POINTS);
  if (const char* f = getenv("M3S_BA_CHUNK_POINTS")) {
    const int len = std::max(256, atoi(f));
    return std::max(1, (N + len - 1) / len);
  }
  if ((int64_t)E * base >= BA_LIN_MIN_BLOCKS || E <= 0) return base;
  const int most = std::max(1, (N + BA_CHUNK_MIN_POINTS - 1) / BA_CHUNK_MIN_POINTS);
  return std::max(base, std::min(most, (BA_LIN_MIN_BLOCKS + E - 1) / E));
}

constexpr int BA_DENSE_MAX_POSES = 1025;  // dense fallback workspace: (2n+1) n doubles, ~0.8 GB at this size

// factor blocks of the densest possible pattern (every pose coupled to every other)
inline size_t ba_max_blocks(int Kp) {
  const size_t nb = (size_t)std::max(0, Kp - 1);
  return nb * (nb + 1) / 2;
}

// the plan's host-built tables, uploaded in ONE copy: rank arrays, keyframe pointer tables and the
// symbolic factorisation (ba_pattern.h BA_SYM_SECTIONS), packed at their actual sizes into a region sized for the
// worst case
constexpr int BA_BLOB_SECTIONS = 9 + BA_SYM_NSEC;
// update pairs (source block row -> target block) the plan can hold: every pattern up to K ~ 600, and the
// sparse patterns of larger graphs
inline size_t ba_max_pairs(int Kp) {
  const size_t nb = (size_t)std::max(0, Kp - 1);
  return std::min(nb * nb * nb / 6 + nb * nb + 64, 32 * ba_max_blocks(Kp) + 64);
}
size_t ba_blob_capacity(int Kp, int N, int E, int chunks) {
  const size_t nb = (size_t)std::max(0, Kp - 1);
  const size_t ints = 2 * (size_t)E +       // the ranks
                      (size_t)E * chunks +  // the linearisation block table
                      2 * (size_t)E +       // record slots and the pack list (record reuse)
                      ba_sym_capacity_ints(nb, ba_max_blocks(Kp), E, ba_max_pairs(Kp), M3S_BA_SP_WAVES);
  return ints * 4 + (size_t)Kp * (8 + 8 + 4) + ba_ray_tab_floats(N) * 4 + BA_BLOB_SECTIONS * 16;
}

size_t ba_carve(Carver& c, int Kp, int N, int E, int chunks, BaArgs* a, size_t* es_off, void** blob) {
  const int nb = std::max(0, Kp - 1);
  // record slots (worst case: a shard packs only its own edges), each N records + the rays' N |Xi|
  a->rec = c.take<float4>((size_t)E * ba_rec_slot_bytes(N) / 16);
  a->partials = c.take<double>((size_t)E * chunks * 36);
  *es_off = c.off;
  a->edge_sums = c.take<double>((size_t)E * 36);
  a->L = c.take<double>(std::max<size_t>(ba_max_blocks(Kp), 1) * 64);
  a->y = c.take<double>((size_t)std::max(nb, 1) * 8);
  a->xs = c.take<double>((size_t)std::max(nb, 1) * 8);
  a->dx = c.take<float>((size_t)std::max(nb, 1) * 7);
  // the dense fallback's system (graphs up to BA_DENSE_MAX_POSES poses)
  const size_t n = (size_t)nb * 7;
  a->H = Kp <= BA_DENSE_MAX_POSES ? c.take<double>(std::max<size_t>((2 * n + 1) * n, 1)) : nullptr;
  a->info = c.take<int>(8);
  a->done = a->info + 1;
  a->iters = a->info + 2;
  *blob = c.take<char>(ba_blob_capacity(Kp, N, E, chunks));
  return c.off;
}

// Record reuse across plans on one workspace (m3s_ba_make_plan_reuse). The backend solves once per new keyframe
// (main.py:150-155): the edge set only grows and tracking changes only the keyframes it fuses into, so most edges'
// point records are still valid in the workspace. Per workspace: the record slot of every directed edge (by the
// caller's edge uid), a copy of every keyframe's points and confidences as last packed (by keyframe uid) for the
// next plan's exact compare, and the parameters the records depend on besides those.
struct RecCache {
  bool valid = false;
  int N = 0, mode = -1, W = 0;
  float Q_thresh = 0.0f, C_thresh = 0.0f, z_eps = 0.0f;
  std::unordered_map<int64_t, int> slot_of;  // edge uid -> record slot (shard-local)
  std::unordered_map<int64_t, int> copy_of;  // keyframe uid -> copy index
  std::vector<uint32_t> scale;               // per copy: bits of the Cscale its records were packed with
  std::vector<char> primed;                  // per copy: compared (and so filled) at least once
  float* copies = nullptr;                   // device: cap x 4N floats (X then C)
  int cap = 0, used = 0;
  BaKfCopy* table = nullptr;                 // device: tcap entries
  BaKfCopy* table_h = nullptr;               // pinned host staging of the table
  uint8_t* dirty = nullptr;                  // device: tcap flags
  uint8_t* dirty_h = nullptr;                // pinned host: tcap flags
  int tcap = 0;
  void reset_maps() {
    slot_of.clear();
    copy_of.clear();
    scale.clear();
    primed.clear();
    used = 0;
  }
  void free_tables() {
    if (table) (void)hipFree(table);
    if (dirty) (void)hipFree(dirty);
    if (table_h) (void)hipHostFree(table_h);
    if (dirty_h) (void)hipHostFree(dirty_h);
    table = nullptr;
    dirty = nullptr;
    table_h = nullptr;
    dirty_h = nullptr;
    tcap = 0;
  }
  void free_all() {
    if (copies) (void)hipFree(copies);
    copies = nullptr;
    cap = 0;
    free_tables();
    reset_maps();
    valid = false;
  }
  // room for `fresh` more keyframe copies of `per` floats each (geometric growth, keeping the ones in use)
  int grow_copies(int fresh, size_t per, hipStream_t s) {
    if (used + fresh <= cap) return M3S_OK;
    const int ncap = std::max(used + fresh, cap + cap / 2 + 8);
    float* nc = nullptr;
    HIP_TRY(hipStreamSynchronize(s), "ba sync");
    HIP_TRY(hipMalloc((void**)&nc, sizeof(float) * per * ncap), "ba keyframe copies");
    if (used) HIP_TRY(hipMemcpy(nc, copies, sizeof(float) * per * used, hipMemcpyDeviceToDevice),
                      "ba keyframe copies");
    if (copies) (void)hipFree(copies);
    copies = nc;
    cap = ncap;
    return M3S_OK;
  }
  // compare tables (device + pinned host) of at least Kp entries
  int grow_tables(int Kp, hipStream_t s) {
    if (Kp <= tcap) return M3S_OK;
    HIP_TRY(hipStreamSynchronize(s), "ba sync");
    free_tables();
    const int tc = std::max(Kp, 64);
    HIP_TRY(hipMalloc((void**)&table, sizeof(BaKfCopy) * tc), "ba reuse table");
    HIP_TRY(hipMalloc((void**)&dirty, tc), "ba reuse flags");
    HIP_TRY(hipHostMalloc((void**)&table_h, sizeof(BaKfCopy) * tc, hipHostMallocDefault), "ba reuse table");
    HIP_TRY(hipHostMalloc((void**)&dirty_h, tc, hipHostMallocDefault), "ba reuse flags");
    tcap = tc;
    return M3S_OK;
  }
};
std::mutex g_rec_mu;
std::map<const void*, RecCache> g_rec;  // by workspace (map nodes never move)

// rank remap (gn_kernels.cu:161-170): unique(cat(ii,jj)) sorted; searchsorted. False (ri / rj unset) when there are
// more unique keyframe ids than the Kp poses.
bool rank_remap(const int64_t* ii, const int64_t* jj, int E, int Kp, std::vector<int>* ri, std::vector<int>* rj) {
  std::vector<int64_t> u(ii, ii + E);
  u.insert(u.end(), jj, jj + E);
  std::sort(u.begin(), u.end());
  u.erase(std::unique(u.begin(), u.end()), u.end());
  if ((int)u.size() > Kp) return false;
  ri->resize(E);
  rj->resize(E);
  for (int e = 0; e < E; e++) {
    (*ri)[e] = (int)(std::lower_bound(u.begin(), u.end(), ii[e]) - u.begin());
    (*rj)[e] = (int)(std::lower_bound(u.begin(), u.end(), jj[e]) - u.begin());
  }
  return true;
}

}  // namespace

extern "C" size_t m3s_ba_workspace_size(int Kp, int N, int E) {
  Carver c(nullptr);
  BaArgs a;
  size_t off;
  void* blob;
  return ba_carve(c, Kp, N, E, ba_chunks(N, E), &a, &off, &blob);
}

extern "C" int m3s_ba_pattern_stats(const int64_t* ii, const int64_t* jj, int E, int Kp, int* stats) {
  M3S_CHECK(ii && jj && stats && E >= 0 && Kp >= 1, "ba pattern: bad arguments");
  std::vector<int> ri, rj;
  M3S_CHECK(rank_remap(ii, jj, E, Kp, &ri, &rj), "ba pattern: more unique keyframe ids than poses");
  BaPattern P;
  M3S_CHECK(Kp <= M3S_BA_MAX_POSES, "ba pattern: at most 4096 poses (M3S_BA_MAX_POSES)");
  ba_build_pattern(ri.data(), rj.data(), E, Kp, &P, ba_max_pairs(Kp));
  if (P.too_dense) return fail(M3S_EINVAL, "ba pattern: too dense for the plan tables");
  stats[0] = P.nL;
  stats[1] = P.nlev;
  stats[2] = (int)P.grp.size() / 4;
  stats[3] = (int)P.src.size() / 4;
  stats[4] = (int)P.sidx.size();
  stats[5] = (int)std::count_if(P.pull_grp.begin(), P.pull_grp.end(), [](int g) { return g >= 0; });
  return M3S_OK;
}

extern "C" int m3s_ba_calib_rays(const m3s_ba_config* cfg, float* x_of_u, float* y_of_v) {
  M3S_CHECK(cfg && x_of_u && y_of_v, "ba calib rays: null argument");
  M3S_CHECK(cfg->width > 0 && cfg->height > 0 && cfg->width < 65536 && cfg->height < 65536,
            "ba calib rays: width and height must be in [1, 65535]");
  ba_calib_rays(cfg, x_of_u, y_of_v);
  return M3S_OK;
}

namespace {
// The symbolic half of a plan (ordering, factor pattern, levels, update groups, assembly CSR; ba_pattern.h) and
// the solve schedule derived from it. It is needed only from the first m3s_ba_solve on, so it is built on a host
// worker thread while the device packs the point records and runs the first linearisation: the host analysis
// (~0.6 ms at K = 256) leaves the replicated, unsharded part of a multi-GPU solve. m3s_ba_solve (or
// m3s_ba_plan_info) joins it once and uploads its tables. One per workspace (a new plan on the same workspace
// first joins the previous one); `gen` ties a plan to it.
struct PlanSym {
  unsigned long long gen = 0;
  std::future<int> fut;
  bool joined = false, uploaded = false;
  int rc = M3S_OK;
  std::string err;
  BaSymPlan plan;  // worker output (read by the main thread only after the join): ba_build_plan's
  bool pack_deferred = false;    // the plan's pack runs inside its first linearisation (set at plan time, under g_sym_mu)
  char* dst = nullptr;  // device destination (the blob region after the plan's own tables)
};
std::mutex g_sym_mu;
std::map<const void*, std::unique_ptr<PlanSym>> g_sym;  // by workspace
unsigned long long g_sym_gen = 0;

// the plan options the environment sets (tests and experiments): M3S_BA_SOLVER=sparse|dense forces one factorisation,
// M3S_BA_WIDE=t sets the wide split, M3S_BA_FLOW=0 (A/B experiments) the level-synchronous loops
BaPlanOptions plan_options(int Kp, bool has_dense, size_t capacity) {
  BaPlanOptions o;
  o.has_dense = has_dense;
  if (const char* solver = getenv("M3S_BA_SOLVER"))
    o.solver = !strcmp(solver, "sparse") ? 1 : !strcmp(solver, "dense") ? 2 : 0;
  if (const char* w = getenv("M3S_BA_WIDE")) {
    o.wide_by_thr = true;
    o.wide_thr = atoi(w);
  }
  o.flow = env_flag("M3S_BA_FLOW", true);
  o.max_pairs = ba_max_pairs(Kp);
  o.capacity = capacity;
  return o;
}

// worker: ranks ri / rj (all E edges) -> the packed symbolic tables and the factor schedule
int build_symbolic(PlanSym* Y, std::vector<int> ri, std::vector<int> rj, int E, int Kp, BaPlanOptions opt) {
  return ba_build_plan(ri.data(), rj.data(), E, Kp, opt, &Y->plan, &Y->err) ? M3S_OK : M3S_EINVAL;
}

// the plan's PlanSym, joined (with `upload`, its tables enqueued on `s` the first time); nullptr + g_err on failure
PlanSym* plan_symbolic(const BaPlanImpl* P, hipStream_t s, bool upload, int* rc) {
  std::lock_guard<std::mutex> lock(g_sym_mu);
  auto it = g_sym.find(P->ws);
  if (it == g_sym.end() || it->second->gen != P->sym_gen) {
    *rc = fail(M3S_EINVAL, "ba: this plan was superseded by a newer plan on the same workspace");
    return nullptr;
  }
  PlanSym* Y = it->second.get();
  if (!Y->joined) {
    Y->rc = Y->fut.get();
    Y->joined = true;
  }
  if (upload && !Y->uploaded && Y->rc == M3S_OK) {
    Y->uploaded = true;
    if (!Y->plan.image.empty()) {
      static const UploadNames names = {"ba symbolic upload", "ba symbolic upload", "ba symbolic upload"};
      const UploadSec image = {Y->plan.image.data(), Y->plan.image.size(), nullptr};
      if ((Y->rc = stage_upload(&image, 1, Y->dst, s, names)) != M3S_OK) Y->err = g_err;
      std::vector<char>().swap(Y->plan.image);
    }
  }
  if (Y->rc != M3S_OK) {
    *rc = fail(Y->rc, Y->err);
    return nullptr;
  }
  *rc = M3S_OK;
  return Y;
}

// P->a with the symbolic tables of Y
BaArgs with_symbolic(const BaPlanImpl* P, const PlanSym* Y) {
  BaArgs a = P->a;
  const char* d = Y->dst;
  const BaSymPlan& S = Y->plan;
#define BA_SEC_ARG(name, src, lds, cap) a.name = reinterpret_cast<decltype(a.name)>(d + S.off[BA_SEC_##name]);
  BA_SYM_SECTIONS(BA_SEC_ARG)
#undef BA_SEC_ARG
  a.plan_lo = d + S.plan_lo_off;
  a.plan_bytes = S.plan_bytes;
  a.nb = S.nb;
  a.nlev = S.nlev;
  a.wide_steps = S.wide_steps;
  a.flow = S.flow;
  return a;
}

// What the four plan entry points pass on: the keyframe sources as host arrays of Kp entries (rows of the stacked
// tensors, or each keyframe's own buffers) and the caller's arguments.
struct PlanIn {
  const m3s_ba_config* cfg;
  float* Twc;
  const float *const *Xh, *const *Ch;
  const float* scale_h;
  int Kp, N;
  const int64_t *ii, *jj;
  int E, e0, e1;
  const int64_t* idx;
  const uint8_t* valid;
  const float* Q;
  float delta_thresh;
  float* dx_out;
  const m3s_ba_reuse* reuse;  // nullable: no record reuse
  void* workspace;
  size_t workspace_bytes;
  m3s_ba_plan* plan;
  void* stream;
};

// Keyframe sources -> the plan's device tables: run() is the sequence of steps, the members what they hand on.
struct PlanBuild : PlanIn {
  explicit PlanBuild(const PlanIn& in) : PlanIn(in) {}
  BaPlanImpl P;
  hipStream_t s;
  int chunks, EL;               // point chunks per edge, this shard's edges
  void* blob;                   // the workspace region of the uploaded tables
  PlanSym* Y;                   // this plan's symbolic half
  RecCache* RC = nullptr;       // record reuse: the workspace's cache, else null
  bool calib;
  std::vector<uint8_t> kdirty;  // per keyframe: changed since the workspace's previous plan (all without reuse)
  std::vector<int> rc_ci;       // record reuse: copy index of each keyframe
  std::vector<int> ri, rj;      // ranks of all E edges
  std::vector<int> lin_tab, slot, pack;
  std::vector<float> ray_tab;
  size_t total, capacity;       // bytes of the plan's own tables, of the whole blob
  int check();
  int reuse_prepare();
  int ranks();
  int reuse_compare();
  void lin_table();
  void slots();
  int upload();
  int fill();
  int pack_or_defer();
  int run();
};

int PlanBuild::check() {
  M3S_CHECK(cfg && plan, "ba: null argument");
  M3S_CHECK(cfg->mode >= 0 && cfg->mode <= M3S_BA_MODE_CALIB_RAW,
            "ba: mode must be 0 (points), 1 (rays), 2 (calib) or 3 (calib, raw points)");
  static_assert(M3S_BA_MODE_CALIB_RAW == BA_MODE_CALIB_RAW, "m3s.h and m3s_ba.h name the same mode");
  calib = cfg->mode == BA_MODE_CALIB || cfg->mode == BA_MODE_CALIB_RAW;
  M3S_CHECK(Kp >= 1 && N >= 1 && E >= 0, "ba: bad sizes");
  M3S_CHECK(0 <= e0 && e0 <= e1 && e1 <= E, "ba: bad shard range");
  // the workspace reserves the factor and plan tables of the densest pattern (m3s_ba_workspace_size knows no
  // edges): nb(nb+1)/2 blocks of 512 B, 4.3 GB at this cap
  M3S_CHECK(Kp <= M3S_BA_MAX_POSES, "ba: at most 4096 poses (M3S_BA_MAX_POSES)");
  if (calib) M3S_CHECK(cfg->width > 0 && cfg->height > 0 && (int64_t)cfg->width * cfg->height == N,
                       "ba calib: height*width must equal the points per keyframe");
  if (calib)  // the 12-B calib record holds the matched pixel as u | v << 16 (ba.hip pack_record)
    M3S_CHECK(cfg->width < 65536 && cfg->height < 65536, "ba calib: width and height must be below 65536");
  if (workspace_bytes < m3s_ba_workspace_size(Kp, N, E)) return fail(M3S_ESPACE, "ba: workspace too small");
  return M3S_OK;
}

// a previous plan on this workspace: its worker must be done before the workspace is rewritten
PlanSym* plan_supersede(void* workspace, unsigned long long* gen) {
  std::lock_guard<std::mutex> lock(g_sym_mu);
  auto& slot = g_sym[workspace];
  if (slot && !slot->joined && slot->fut.valid()) slot->fut.wait();
  slot.reset(new PlanSym());
  slot->gen = *gen = ++g_sym_gen;
  return slot.get();
}

// record reuse: the workspace's cache, reset when the parameters its records depend on changed, with room for this
// plan's keyframes and a copy index for each (rc_ci). A plain plan invalidates whatever was cached.
int PlanBuild::reuse_prepare() {
  {
    std::lock_guard<std::mutex> lock(g_rec_mu);
    if (reuse) {
      RC = &g_rec[workspace];
    } else {
      auto it = g_rec.find(workspace);  // a plain plan repacks every slot: whatever was cached there is gone
      if (it != g_rec.end()) it->second.valid = false;
    }
  }
  if (!RC) return M3S_OK;
  const int64_t* kf_uid = reuse->kf_uid;
  const bool same = RC->valid && RC->N == N && RC->mode == cfg->mode && RC->Q_thresh == cfg->Q_thresh &&
                    RC->C_thresh == cfg->C_thresh &&
                    (!calib || (RC->W == cfg->width && RC->z_eps == cfg->z_eps));
  if (!same) {
    RC->reset_maps();
    RC->N = N;
    RC->mode = cfg->mode;
    RC->Q_thresh = cfg->Q_thresh;
    RC->C_thresh = cfg->C_thresh;
    RC->W = cfg->width;
    RC->z_eps = cfg->z_eps;  // calib records hold log z_i, or NaN where z_i <= z_eps
  }
  RC->valid = false;  // until this plan is complete
  std::vector<int> ci(Kp, -1);
  int fresh = 0;
  for (int k = 0; k < Kp; k++) fresh += RC->copy_of.count(kf_uid[k]) ? 0 : 1;
  if (int rc = RC->grow_copies(fresh, (size_t)4 * N, s)) return rc;  // 4N floats per keyframe copy
  if (int rc = RC->grow_tables(Kp, s)) return rc;
  for (int k = 0; k < Kp; k++) {
    auto it = RC->copy_of.find(kf_uid[k]);
    if (it == RC->copy_of.end()) {
      ci[k] = RC->used++;
      RC->copy_of.emplace(kf_uid[k], ci[k]);
      RC->scale.push_back(__builtin_bit_cast(uint32_t, scale_h[k]));
      RC->primed.push_back(0);
    } else {
      ci[k] = it->second;
      for (int q = 0; q < k; q++)
        if (ci[q] == ci[k]) return fail(M3S_EINVAL, "ba reuse: duplicate keyframe uid");
    }
  }
  rc_ci.swap(ci);
  return M3S_OK;
}

// the edge lists read back from the device -> ranks of all E edges (ri, rj)
int PlanBuild::ranks() {
  std::vector<int64_t> hii(E), hjj(E);
  if (E > 0) {
    HIP_TRY(hipMemcpyAsync(hii.data(), ii, sizeof(int64_t) * E, hipMemcpyDeviceToHost, s), "ba ii readback");
    HIP_TRY(hipMemcpyAsync(hjj.data(), jj, sizeof(int64_t) * E, hipMemcpyDeviceToHost, s), "ba jj readback");
  }
  if (E > 0) HIP_TRY(hipStreamSynchronize(s), "ba sync");
  if (!rank_remap(hii.data(), hjj.data(), E, Kp, &ri, &rj))
    return fail(M3S_EINVAL, "ba: more unique keyframe ids in ii/jj than poses in Twc");
  return M3S_OK;
}

// record reuse: which keyframes changed since the workspace's previous plan (exact device compare). Only the
// keyframes of this shard's edges: only their records can be reused here (a sharded solve compares ~1/world of the
// keyframes per rank). A keyframe's scale and copy change only when it is compared; one compared for the first time
// is dirty whatever its copy holds.
int PlanBuild::reuse_compare() {
  std::vector<char> usedk(Kp, 0);
  for (int e = e0; e < e1; e++) usedk[ri[e]] = usedk[rj[e]] = 1;
  for (int k = 0; k < Kp; k++) {
    const int c = rc_ci[k];
    if (!usedk[k]) {
      kdirty[k] = 0;
      RC->table_h[k] = BaKfCopy{nullptr, nullptr, nullptr};
      continue;
    }
    const uint32_t sb = __builtin_bit_cast(uint32_t, scale_h[k]);
    kdirty[k] = !RC->primed[c] || RC->scale[c] != sb;  // the average-confidence scale 1/N changed: its records did too
    RC->scale[c] = sb;
    RC->primed[c] = 1;
    RC->table_h[k] = BaKfCopy{Xh[k], Ch[k], RC->copies + (size_t)4 * N * c};
  }
  HIP_TRY(hipMemcpyAsync(RC->table, RC->table_h, sizeof(BaKfCopy) * Kp, hipMemcpyHostToDevice, s), "ba reuse table");
  HIP_TRY(hipMemsetAsync(RC->dirty, 0, Kp, s), "ba reuse flags");
  HIP_TRY(m3s_launch_ba_kf_compare(RC->table, Kp, N, RC->dirty, s), "ba keyframe compare launch");
  HIP_TRY(hipMemcpyAsync(RC->dirty_h, RC->dirty, Kp, hipMemcpyDeviceToHost, s), "ba reuse flags readback");
  HIP_TRY(hipStreamSynchronize(s), "ba sync");
  for (int k = 0; k < Kp; k++) kdirty[k] |= RC->dirty_h[k];
  return M3S_OK;
}

// linearisation block table: this shard's edges grouped by target keyframe j, chunk-major within a
// group, so consecutive blocks (dealt to one XCD by xcd_remap) read the same X_j slab
void PlanBuild::lin_table() {
  std::vector<int> order(e1 - e0);
  for (int e = 0; e < e1 - e0; e++) order[e] = e;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return rj[e0 + x] < rj[e0 + y]; });
  lin_tab.reserve((size_t)(e1 - e0) * chunks);
  for (size_t g0 = 0; g0 < order.size();) {
    size_t g1 = g0;
    while (g1 < order.size() && rj[e0 + order[g1]] == rj[e0 + order[g0]]) g1++;
    for (int c = 0; c < chunks; c++)
      for (size_t t = g0; t < g1; t++) lin_tab.push_back(order[t] * chunks + c);
    g0 = g1;
  }
  std::vector<char> seen(Kp, 0);
  for (int e = e0; e < e1; e++) P.n_targets += seen[rj[e]] ? 0 : (seen[rj[e]] = 1);
}

// record slots: an edge keeps the slot of its uid when that slot is still inside this shard's record range and
// repacks there only if one of its keyframes changed; new edges take free slots and pack. Without reuse every edge
// packs into its own slot.
void PlanBuild::slots() {
  if (RC) {
    const int64_t* edge_uid = reuse->edge_uid;
    slot.assign(EL, -1);
    std::vector<char> taken(EL, 0), need(EL, 0);
    for (int t = 0; t < EL; t++) {
      auto it = RC->slot_of.find(edge_uid[e0 + t]);
      if (it != RC->slot_of.end() && it->second < EL && !taken[it->second]) {
        slot[t] = it->second;
        taken[slot[t]] = 1;
        need[t] = kdirty[ri[e0 + t]] || kdirty[rj[e0 + t]];
      }
    }
    for (int t = 0, f = 0; t < EL; t++) {
      if (slot[t] >= 0) continue;
      while (taken[f]) f++;
      slot[t] = f;
      taken[f] = 1;
      need[t] = 1;
    }
    RC->slot_of.clear();
    for (int t = 0; t < EL; t++) RC->slot_of[edge_uid[e0 + t]] = slot[t];
    for (int t = 0; t < EL; t++)
      if (need[t]) pack.push_back(t);
  } else {
    for (int t = 0; t < EL; t++) pack.push_back(t);
  }
  // the pack order: grouped by source keyframe (ba_pack_kernel splits it into eighths, one per XCD, so an XCD's L2
  // holds the points and confidences of its own source keyframes; the records land in their slots whatever the order)
  std::stable_sort(pack.begin(), pack.end(), [&](int x, int y) { return ri[e0 + x] < ri[e0 + y]; });
}

// the tables the pack and the linearisation read, in ONE upload ahead of the pack; the symbolic tables follow
// in the same blob (their own upload, at the first solve)
int PlanBuild::upload() {
  // raw calib: the pixel-ray tables the linearisation builds X_j from (x_of_u then y_of_v, W + H floats)
  if (cfg->mode == BA_MODE_CALIB_RAW) {
    ray_tab.resize((size_t)cfg->width + cfg->height);
    ba_calib_rays(cfg, ray_tab.data(), ray_tab.data() + cfg->width);
  }
  const UploadSec secs[] = {
      {ri.data() + e0, sizeof(int) * EL, (const void**)&P.a.ii_rank},
      {rj.data() + e0, sizeof(int) * EL, (const void**)&P.a.jj_rank},
      {Xh, sizeof(const float*) * Kp, (const void**)&P.a.Xkf},
      {Ch, sizeof(const float*) * Kp, (const void**)&P.a.Ckf},
      {scale_h, sizeof(float) * Kp, (const void**)&P.a.Cscale},
      {lin_tab.data(), sizeof(int) * lin_tab.size(), (const void**)&P.a.lin_tab},
      {slot.data(), sizeof(int) * slot.size(), (const void**)&P.a.rec_slot},
      {pack.data(), sizeof(int) * pack.size(), (const void**)&P.a.pack_list},
      {ray_tab.data(), sizeof(float) * ray_tab.size(), (const void**)&P.a.ray_tab},
  };
  constexpr int nsec = sizeof(secs) / sizeof(secs[0]);
  static_assert(nsec + BA_SYM_NSEC == BA_BLOB_SECTIONS, "blob sections");
  total = upload_bytes(secs, nsec);
  capacity = ba_blob_capacity(Kp, N, E, chunks);
  if (total > capacity) return fail(M3S_EINVAL, "ba: plan tables exceed the workspace blob");
  static const UploadNames names = {"ba stage", "ba upload", "ba stage record"};
  if (int rc = stage_upload(secs, nsec, blob, s, names)) return rc;
  if (ray_tab.empty()) P.a.ray_tab = nullptr;
  if (!RC) P.a.rec_slot = nullptr;  // every edge packs into its own slot (the pack list is the source-keyframe order)
  Y->dst = static_cast<char*>(blob) + total;
  return M3S_OK;
}

// clear the solve's status words and the edge sums, then fill the kernels' arguments and parameters
int PlanBuild::fill() {
  HIP_TRY(hipMemsetAsync(P.a.info, 0, 8 * sizeof(int), s), "ba memset");
  HIP_TRY(hipMemsetAsync(P.a.edge_sums, 0, P.edge_sums_bytes > 0 ? P.edge_sums_bytes : 8, s), "ba memset");
  P.a.bad = P.a.info + 3;
  P.a.stalled = P.a.info + 4;
  P.a.force_stall = env_flag("M3S_BA_FORCE_STALL", false);
  P.a.Twc = Twc;
  P.a.idx = idx;
  P.a.valid = valid;
  P.a.Q = Q;
  P.p.mode = cfg->mode;
  P.p.N = N;
  P.p.chunks = chunks;
  P.p.edge_offset = e0;
  // gn_kernels.cu:546, 905-906, 1341-1342: const float sigma_inv = 1.0/sigma (double division)
  P.p.inv_a = (float)(1.0 / (double)cfg->sigma_a);
  P.p.inv_b = cfg->mode == 0 ? 0.0f : (float)(1.0 / (double)cfg->sigma_b);
  P.p.C_thresh = cfg->C_thresh;
  P.p.Q_thresh = cfg->Q_thresh;
  P.p.fx = cfg->fx;
  P.p.fy = cfg->fy;
  P.p.cx = cfg->cx;
  P.p.cy = cfg->cy;
  P.p.H = cfg->height;
  P.p.W = cfg->width;
  P.p.pixel_border = cfg->pixel_border;
  P.p.z_eps = cfg->z_eps;
  P.Kp = Kp;
  P.N = N;
  P.E = E;
  P.e0 = e0;
  P.e1 = e1;
  P.delta_thresh = delta_thresh;
  P.ws = workspace;
  P.a.dx = dx_out ? dx_out : P.a.dx;
  // per-call point records of this shard's edges: the matched point, its pixel and the folded validity
  // weight do not change across GN iterations (only the poses do)
  P.n_packed = RC ? (int)pack.size() : e1 - e0;
  P.n_dirty = 0;
  for (int k = 0; k < Kp; k++) P.n_dirty += kdirty[k];
  return M3S_OK;
}

// M3S_BA_FUSED_PACK=1 (opt-in): when every shard edge packs, the pack's gathers run inside the first
// linearisation (ba_lin_kernel<PACK>) instead of their own launch. Measured slower at C5 (pack 4.3 ms + lin 1.9 ms
// -> one 8.3 ms launch: the gathers' latency at the linearisation's 3 waves per SIMD), so off by default
int PlanBuild::pack_or_defer() {
  const bool defer = P.n_packed == EL && EL > 0 && env_flag("M3S_BA_FUSED_PACK", false);
  if (defer) {
    std::lock_guard<std::mutex> lock(g_sym_mu);
    Y->pack_deferred = true;
  } else {
    Span sp("ba_pack", s);
    HIP_TRY(m3s_launch_ba_pack(&P.a, &P.p, P.n_packed, s), "ba pack launch");
  }
  if (RC) RC->valid = true;
  return M3S_OK;
}

int PlanBuild::run() {
  if (int rc = check()) return rc;
  memset(&P, 0, sizeof(P));
  s = (hipStream_t)stream;
  chunks = ba_chunks(N, E);
  EL = e1 - e0;
  Carver c(workspace);
  ba_carve(c, Kp, N, E, chunks, &P.a, &P.edge_sums_off, &blob);
  P.edge_sums_bytes = (size_t)E * 36 * sizeof(double);
  Y = plan_supersede(workspace, &P.sym_gen);
  kdirty.assign(Kp, 1);
  if (int rc = reuse_prepare()) return rc;
  if (int rc = ranks()) return rc;
  if (RC)
    if (int rc = reuse_compare()) return rc;
  lin_table();
  slots();
  if (int rc = upload()) return rc;
  if (int rc = fill()) return rc;
  if (int rc = pack_or_defer()) return rc;
  // the symbolic analysis of ALL E edges (every rank builds the identical system) runs on a host worker while
  // the device packs and linearises
  Y->fut = std::async(std::launch::async, build_symbolic, Y, std::move(ri), std::move(rj), E, Kp,
                      plan_options(Kp, P.a.H != nullptr, capacity - total));
  memcpy(plan->opaque, &P, sizeof(P));
  return M3S_OK;
}

int ba_make_plan_impl(const PlanIn& in) { return PlanBuild(in).run(); }
}  // namespace

extern "C" int m3s_ba_make_plan_reuse(const m3s_ba_config* cfg, float* Twc, const float* Xs, const float* Cs, int Kp,
                                      int N, const int64_t* ii, const int64_t* jj, int E, int e0, int e1,
                                      const int64_t* idx, const uint8_t* valid, const float* Q, float delta_thresh,
                                      float* dx_out, const m3s_ba_reuse* reuse, void* workspace,
                                      size_t workspace_bytes, m3s_ba_plan* plan, void* stream) {
  M3S_CHECK(!reuse || (reuse->edge_uid && reuse->kf_uid), "ba reuse: null uid array");
  M3S_CHECK(Xs && Cs && Kp >= 1 && N >= 1, "ba: null Xs/Cs or bad sizes");
  std::vector<const float*> xh(Kp), ch(Kp);
  std::vector<float> sh(Kp, 1.0f);  // stacked Cs is already the average confidence
  for (int k = 0; k < Kp; k++) {
    xh[k] = Xs + (size_t)k * N * 3;
    ch[k] = Cs + (size_t)k * N;
  }
  return ba_make_plan_impl(PlanIn{cfg, Twc, xh.data(), ch.data(), sh.data(), Kp, N, ii, jj, E, e0, e1, idx, valid, Q,
                                  delta_thresh, dx_out, reuse, workspace, workspace_bytes, plan, stream});
}

extern "C" int m3s_ba_make_plan_kf_reuse(const m3s_ba_config* cfg, float* Twc, const m3s_ba_keyframes* kf, int Kp,
                                         int N, const int64_t* ii, const int64_t* jj, int E, int e0, int e1,
                                         const int64_t* idx, const uint8_t* valid, const float* Q, float delta_thresh,
                                         float* dx_out, const m3s_ba_reuse* reuse, void* workspace,
                                         size_t workspace_bytes, m3s_ba_plan* plan, void* stream) {
  M3S_CHECK(!reuse || (reuse->edge_uid && reuse->kf_uid), "ba reuse: null uid array");
  M3S_CHECK(kf && kf->X && kf->C && kf->N_avg && Kp >= 1 && N >= 1, "ba: null keyframe table or bad sizes");
  std::vector<float> sh(Kp);
  for (int k = 0; k < Kp; k++) {
    M3S_CHECK(kf->X[k] && kf->C[k], "ba: null keyframe buffer");
    M3S_CHECK(kf->N_avg[k] > 0.0f, "ba: keyframe fusion count N must be positive");
    sh[k] = conf_scale(kf->N_avg[k]);
  }
  return ba_make_plan_impl(PlanIn{cfg, Twc, kf->X, kf->C, sh.data(), Kp, N, ii, jj, E, e0, e1, idx, valid, Q,
                                  delta_thresh, dx_out, reuse, workspace, workspace_bytes, plan, stream});
}

extern "C" int m3s_ba_make_plan(const m3s_ba_config* cfg, float* Twc, const float* Xs, const float* Cs, int Kp, int N,
                                const int64_t* ii, const int64_t* jj, int E, int e0, int e1, const int64_t* idx,
                                const uint8_t* valid, const float* Q, float delta_thresh, float* dx_out,
                                void* workspace, size_t workspace_bytes, m3s_ba_plan* plan, void* stream) {
  return m3s_ba_make_plan_reuse(cfg, Twc, Xs, Cs, Kp, N, ii, jj, E, e0, e1, idx, valid, Q, delta_thresh, dx_out,
                                nullptr, workspace, workspace_bytes, plan, stream);
}

extern "C" int m3s_ba_make_plan_kf(const m3s_ba_config* cfg, float* Twc, const m3s_ba_keyframes* kf, int Kp, int N,
                                   const int64_t* ii, const int64_t* jj, int E, int e0, int e1, const int64_t* idx,
                                   const uint8_t* valid, const float* Q, float delta_thresh, float* dx_out,
                                   void* workspace, size_t workspace_bytes, m3s_ba_plan* plan, void* stream) {
  return m3s_ba_make_plan_kf_reuse(cfg, Twc, kf, Kp, N, ii, jj, E, e0, e1, idx, valid, Q, delta_thresh, dx_out,
                                   nullptr, workspace, workspace_bytes, plan, stream);
}

extern "C" int m3s_ba_reuse_info(const m3s_ba_plan* plan, int* packed_edges, int* changed_keyframes) {
  M3S_CHECK(plan && packed_edges && changed_keyframes, "ba: null argument");
  const BaPlanImpl* P = reinterpret_cast<const BaPlanImpl*>(plan->opaque);
  *packed_edges = P->n_packed;
  *changed_keyframes = P->n_dirty;
  return M3S_OK;
}

extern "C" int m3s_ba_plan_release(const void* workspace) {
  std::unique_ptr<PlanSym> Y;
  {
    std::lock_guard<std::mutex> lock(g_sym_mu);
    auto it = g_sym.find(workspace);
    if (it == g_sym.end()) return M3S_OK;
    Y = std::move(it->second);
    g_sym.erase(it);
  }
  if (Y && !Y->joined && Y->fut.valid()) Y->fut.wait();  // the worker writes into Y: done before it is freed
  return M3S_OK;
}

extern "C" int m3s_ba_plan_count(void) {
  std::lock_guard<std::mutex> lock(g_sym_mu);
  return (int)g_sym.size();
}

extern "C" int m3s_ba_reuse_release(const void* workspace) {
  m3s_ba_plan_release(workspace);
  std::lock_guard<std::mutex> lock(g_rec_mu);
  auto it = g_rec.find(workspace);
  if (it == g_rec.end()) return M3S_OK;
  it->second.free_all();
  g_rec.erase(it);
  return M3S_OK;
}

extern "C" int m3s_ba_edge_sums(const m3s_ba_plan* plan, size_t* byte_offset, size_t* byte_count) {
  M3S_CHECK(plan && byte_offset && byte_count, "ba: null argument");
  const BaPlanImpl* P = reinterpret_cast<const BaPlanImpl*>(plan->opaque);
  *byte_offset = P->edge_sums_off;
  *byte_count = P->edge_sums_bytes;
  return M3S_OK;
}

extern "C" int m3s_ba_plan_info(const m3s_ba_plan* plan, int* info) {
  M3S_CHECK(plan && info, "ba: null argument");
  const BaPlanImpl* P = reinterpret_cast<const BaPlanImpl*>(plan->opaque);
  int rc;
  const PlanSym* Y = plan_symbolic(P, nullptr, false, &rc);  // joins the symbolic analysis
  if (Y == nullptr) return rc;
  info[0] = P->p.chunks;
  info[1] = Y->plan.nL;
  info[2] = Y->plan.nlev;
  info[3] = Y->plan.wide_steps;
  info[4] = Y->plan.dense;
  info[5] = P->n_targets;
  info[6] = P->e1 - P->e0;
  info[7] = P->Kp;
  info[8] = info[9] = info[10] = info[11] = info[12] = 0;  // round 5's opt-in solver phases (removed in round 6)
  return M3S_OK;
}

extern "C" int m3s_ba_linearize(const m3s_ba_plan* plan, void* stream) {
  M3S_CHECK(plan, "ba: null plan");
  const BaPlanImpl* P = reinterpret_cast<const BaPlanImpl*>(plan->opaque);
  hipStream_t s = (hipStream_t)stream;
  // a shard writes only its own rows: clear the rest so the caller's all-reduce sums fresh rows
  if ((P->e0 > 0 || P->e1 < P->E) && P->edge_sums_bytes > 0)
    HIP_TRY(hipMemsetAsync(P->a.edge_sums, 0, P->edge_sums_bytes, s), "ba memset");
  int pack = 0;  // this plan's first linearisation also packs (see ba_make_plan_impl)
  {
    std::lock_guard<std::mutex> lock(g_sym_mu);
    auto it = g_sym.find(P->ws);
    if (it != g_sym.end() && it->second->gen == P->sym_gen && it->second->pack_deferred) {
      pack = 1;
      it->second->pack_deferred = false;
    }
  }
  Span sp(pack ? "ba_lin_pack" : "ba_linearize", s);
  HIP_TRY(m3s_launch_ba_lin(&P->a, &P->p, P->e1 - P->e0, pack, s), "ba linearize launch");
  return M3S_OK;
}

extern "C" int m3s_ba_solve(const m3s_ba_plan* plan, void* stream) {
  M3S_CHECK(plan, "ba: null plan");
  const BaPlanImpl* P = reinterpret_cast<const BaPlanImpl*>(plan->opaque);
  hipStream_t s = (hipStream_t)stream;
  int rc;
  const PlanSym* Y = plan_symbolic(P, s, true, &rc);  // the first solve joins the host worker and uploads its tables
  if (Y == nullptr) return rc;
  const BaArgs a = with_symbolic(P, Y);
  Span sp("ba_solve", s);
  HIP_TRY(Y->plan.dense ? m3s_launch_ba_solve_dense(&a, P->Kp, Y->plan.nL, P->delta_thresh, s)
                        : m3s_launch_ba_solve(&a, P->Kp, Y->plan.nL, P->delta_thresh, Y->plan.steps, s),
          "ba solve launch");
  return M3S_OK;
}

extern "C" int m3s_ba_iterations(const m3s_ba_plan* plan, int* iters_out, void* stream) {
  M3S_CHECK(plan && iters_out, "ba: null argument");
  const BaPlanImpl* P = reinterpret_cast<const BaPlanImpl*>(plan->opaque);
  hipStream_t s = (hipStream_t)stream;
  int st[3];  // iters, bad, stalled (info + 2 .. + 4)
  HIP_TRY(hipMemcpyAsync(st, P->a.iters, sizeof(st), hipMemcpyDeviceToHost, s), "ba readback");
  HIP_TRY(hipStreamSynchronize(s), "ba sync");
  *iters_out = st[0];
  if (st[2] != 0)
    return fail(M3S_ESTALL, "ba: a factor-schedule hand-off stalled (bounded wait timed out); poses were not updated "
                            "by the stalled iteration and the loop stopped");
  return M3S_OK;
}

extern "C" int m3s_gauss_newton(const m3s_ba_config* cfg, float* Twc, const float* Xs, const float* Cs, int Kp, int N,
                                const int64_t* ii, const int64_t* jj, int E, const int64_t* idx,
                                const uint8_t* valid, const float* Q, int max_iter, float delta_thresh, float* dx_out,
                                int* iters_out, void* workspace, size_t workspace_bytes, void* stream) {
  M3S_CHECK(max_iter >= 0, "ba: max_iter must be >= 0");
  m3s_ba_plan plan;
  int rc = m3s_ba_make_plan(cfg, Twc, Xs, Cs, Kp, N, ii, jj, E, 0, E, idx, valid, Q, delta_thresh, dx_out, workspace,
                            workspace_bytes, &plan, stream);
  if (rc != M3S_OK) return rc;
  if (dx_out && Kp > 1)
    HIP_TRY(hipMemsetAsync(dx_out, 0, sizeof(float) * (size_t)(Kp - 1) * 7, (hipStream_t)stream), "ba memset");
  for (int it = 0; it < max_iter; it++) {
    if ((rc = m3s_ba_linearize(&plan, stream)) != M3S_OK) return rc;
    if ((rc = m3s_ba_solve(&plan, stream)) != M3S_OK) return rc;
  }
  // one readback per call (the reference's host loop syncs every iteration): the iteration count and the
  // schedule-stall check (M3S_ESTALL), so a stalled solve is an error, never silently unoptimised poses
  int iters_local = 0;
  return m3s_ba_iterations(&plan, iters_out ? iters_out : &iters_local, stream);
}
