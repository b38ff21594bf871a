// C ABI of libm3s.so (include/m3s.h): tracking (m3s_track*). Kernels live in track.hip.
#include "abi_common.h"

#include <algorithm>
#include <map>
#include <mutex>

#include "m3s_track.h"

using namespace m3s_abi;

// Per host thread: the frame result mirror in fine-grained pinned memory (the fuse launch writes it).
static TrackMirror* pinned_mirror() {
  static thread_local TrackMirror* h = nullptr;
  if (h == nullptr) {
    void* p = nullptr;
    if (hipHostMalloc(&p, sizeof(TrackMirror), hipHostMallocCoherent | hipHostMallocPortable) != hipSuccess)
      return nullptr;
    h = static_cast<TrackMirror*>(p);
    memset(h, 0, sizeof(TrackMirror));
  }
  return h;
}

// Wait for generation `gen` in the mirror: a spin on the host-coherent word (no interrupt wake-up, no
// D2H copy kernel), with a stream query every 1024 polls so a failed or drained stream ends the wait.
static int wait_published(const TrackMirror* m, unsigned gen, hipStream_t s) {
  for (unsigned spin = 1;; spin++) {
    if (__atomic_load_n(&m->gen, __ATOMIC_ACQUIRE) == gen) return M3S_OK;
    if ((spin & 1023u) == 0) {
      const hipError_t q = hipStreamQuery(s);
      if (q == hipSuccess) {
        if (__atomic_load_n(&m->gen, __ATOMIC_ACQUIRE) == gen) return M3S_OK;
        return fail(M3S_EHIP, "track: stream drained without publishing the frame state");
      }
      if (q != hipErrorNotReady) return fail(M3S_EHIP, std::string("track sync: ") + hipGetErrorString(q));
    }
    __builtin_ia32_pause();
  }
}

// workspaces whose frame scratch the last fuse launch cleared: workspace -> {the workspace's size, the image size N
// of that frame}. The scratch layout (track_carve) depends on N: a frame of another size wrote its records and
// partials where this size's byte map lies (a 48x64 frame left 5540 stale map entries under a following 512x512
// frame's unique-match count), so the record holds only for the same N. Dropped by m3s_track_release (the caller
// frees or repurposes the workspace).
namespace {
struct TrackClean {
  size_t bytes;
  int N;
};
}  // namespace
static std::mutex g_track_clean_mu;
static std::map<const void*, TrackClean> g_track_clean;

extern "C" int m3s_track_release(const void* workspace) {
  std::lock_guard<std::mutex> lock(g_track_clean_mu);
  g_track_clean.erase(workspace);
  return M3S_OK;
}

static int track_nparts(int N) { return std::max(1, std::min(GN_MAX_BLOCKS, (N + 1023) / 1024)); }  // <= 1 block per CU

namespace {
struct TrackWs {
  TrackState* state;
  unsigned long long* cnt;
  unsigned* tick;
  uint8_t* flags;
  double* partials;
  float* rec;
};
}  // namespace

static size_t track_carve(Carver& c, int N, TrackWs* w) {
  w->state = c.take<TrackState>(1);
  w->cnt = c.take<unsigned long long>(M3S_TRACK_SHARDS * 16);
  w->tick = c.take<unsigned>(M3S_TRACK_TICK_WORDS);
  w->flags = c.take<uint8_t>(((size_t)N + 15) / 16 * 16);
  w->partials = c.take<double>((size_t)GN_SLOTS * GN_MAX_BLOCKS * GN_PSTRIDE);
  w->rec = c.take<float>((size_t)N * 8);
  return c.off;
}

extern "C" size_t m3s_track_workspace_size(int N) {
  Carver c(nullptr);
  TrackWs w;
  return track_carve(c, N, &w);
}

static int track_check(const m3s_track_inputs* in, const m3s_track_config* cfg, const m3s_track_result* result) {
  M3S_CHECK(in && cfg && result, "track: null argument");
  M3S_CHECK(cfg->H >= 1 && cfg->W >= 1, "track: bad image size");
  M3S_CHECK(cfg->mode == 0 || cfg->mode == 1, "track: mode must be 0 (rays) or 1 (calib)");
  M3S_CHECK(cfg->max_iters >= 1, "track: max_iters must be >= 1");
  if (in->direct) {
    M3S_CHECK(in->valid_match && in->Xf && in->Qff && in->T_WCf && in->T_WCk, "track: null input pointer");
    M3S_CHECK(cfg->mode == 0 ? in->Xk != nullptr : (in->meas_k && in->valid_meas_k),
              "track direct: rays needs Xk, calib needs meas_k/valid_meas_k");
  } else {
    M3S_CHECK(in->idx_f2k && in->valid_match && in->Xf && in->Cf && in->Qff && in->Xk && in->Ck && in->Qkf &&
                  in->T_WCf && in->T_WCk,
              "track: null input pointer");
    M3S_CHECK(in->Nf > 0 && in->Nk > 0, "track: fusion counts must be positive");
  }
  return M3S_OK;
}

static TrackArgs track_args(const TrackWs& w, const m3s_track_inputs* in, float* T_out_dev) {
  TrackArgs a;
  a.state = w.state;
  a.flags = w.flags;
  a.partials = w.partials;
  a.rec = w.rec;
  a.cnt = w.cnt;
  a.tick = w.tick;
  a.idx = in->idx_f2k;
  a.valid_match = in->valid_match;
  a.Xf = in->Xf;
  a.Cf = in->Cf;
  a.Qff = in->Qff;
  a.Xk = in->Xk;
  a.Ck = in->Ck;
  a.Qkf = in->Qkf;
  a.meas_k = in->meas_k;
  a.valid_meas = in->valid_meas_k;
  a.T_out = T_out_dev;
  a.T_WCf = in->T_WCf;
  a.T_WCk = in->T_WCk;
  return a;
}

static int track_params(const m3s_track_inputs* in, const m3s_track_config* cfg, int N, TrackParams* out) {
  TrackParams& p = *out;
  memset(&p, 0, sizeof(p));
  p.N = N;
  p.H = cfg->H;
  p.W = cfg->W;
  p.mode = cfg->mode;
  p.Nf = in->direct ? 1.0f : in->Nf;
  p.Nk = in->direct ? 1.0f : in->Nk;
  p.direct = in->direct != 0;
  p.C_conf = cfg->C_conf;
  p.Q_conf = cfg->Q_conf;
  p.min_match_frac = in->direct ? -1.0f : cfg->min_match_frac;  // opt_pose_* never skips
  p.c_a = (float)(1.0 / (double)cfg->sigma_a);  // tracker.py:175-176: python 1/sigma cast to float32
  p.c_b = (float)(1.0 / (double)cfg->sigma_b);
  p.huber_k = cfg->huber_k;
  p.rel_error = cfg->rel_error;
  p.delta_norm = cfg->delta_norm;
  p.max_iters = cfg->max_iters;
  p.pixel_border = cfg->pixel_border;
  p.depth_eps = cfg->depth_eps;
  for (int i = 0; i < 9; i++) p.K[i] = cfg->K[i];
  p.fx = cfg->K[0];
  p.fy = cfg->K[4];
  p.cx = cfg->K[2];
  p.cy = cfg->K[5];
  if (p.mode == 1) M3S_CHECK(p.fx != 0.0f && p.fy != 0.0f, "track: calib mode needs K");
  return M3S_OK;
}

// the fuse launch's keyframe-fusion arguments (all null: the launch fuses nothing)
static int track_fuse_args(const m3s_track_fuse_args* fuse, FuseArgs* out) {
  FuseArgs& fa = *out;
  fa = FuseArgs{};
  if (!(fuse && fuse->Xk_canon)) return M3S_OK;
  M3S_CHECK(fuse->Ck_sum && fuse->Xkf && fuse->Ckf, "track: fusion needs Ck_sum, Xkf, Ckf");
  M3S_CHECK(!fuse->Ck_avg_out || fuse->Nk_new > 0.0f, "track: Ck_avg_out needs Nk_new > 0");
  M3S_CHECK(!fuse->Cf_avg_out || (fuse->Cf && fuse->Nf > 0.0f), "track: Cf_avg_out needs Cf and Nf > 0");
  fa.X_in = fuse->Xk_canon;
  fa.C_in = fuse->Ck_sum;
  fa.Xkf = fuse->Xkf;
  fa.Ckf = fuse->Ckf;
  fa.X_out = fuse->Xk_out ? fuse->Xk_out : const_cast<float*>(fuse->Xk_canon);
  fa.C_out = fuse->Ck_out ? fuse->Ck_out : const_cast<float*>(fuse->Ck_sum);
  fa.Cf = fuse->Cf;
  fa.Ck_avg = fuse->Ck_avg_out;
  fa.Cf_avg = fuse->Cf_avg_out;
  fa.Nk_new = fuse->Nk_new;
  fa.Nf = fuse->Nf;
  fa.slot_N = fuse->slot_N;
  fa.slot_N_updates = fuse->slot_N_updates;
  fa.slot_dirty = fuse->slot_dirty;
  fa.N_new = fuse->N_new;
  fa.N_updates_new = fuse->N_updates_new;
  return M3S_OK;
}

extern "C" int m3s_track(const m3s_track_inputs* in, const m3s_track_config* cfg, const m3s_track_fuse_args* fuse,
                         int first_chunk, float* T_out_dev, m3s_track_result* result, void* workspace,
                         size_t workspace_bytes, void* stream) {
  if (int rc = track_check(in, cfg, result)) return rc;
  const int N = cfg->H * cfg->W;
  if (workspace_bytes < m3s_track_workspace_size(N)) return fail(M3S_ESPACE, "track: workspace too small");
  Carver c(workspace);
  TrackWs w;
  track_carve(c, N, &w);
  TrackArgs a = track_args(w, in, T_out_dev);
  TrackParams p;
  if (int rc = track_params(in, cfg, N, &p)) return rc;
  hipStream_t s = (hipStream_t)stream;
  FuseArgs fa;
  if (int rc = track_fuse_args(fuse, &fa)) return rc;
  // the previous frame's fuse launch left this workspace's scratch clean (byte map of n16 entries, counters,
  // tickets): track_init runs only for a fresh / grown / failed workspace
  bool clean = false;
  {
    std::lock_guard<std::mutex> lock(g_track_clean_mu);
    auto it = g_track_clean.find(workspace);
    clean = it != g_track_clean.end() && it->second.bytes == workspace_bytes && it->second.N == N;
    g_track_clean.erase(workspace);  // dirty until this call has published
  }
  if (!clean) HIP_TRY(m3s_launch_track_init(&a, N, s), "track init launch");
  // the per-point setup runs inside the GN launch's first iteration (gn_loop_kernel<true>: no track_setup launch);
  // M3S_TRACK_FOLD_SETUP=0 keeps the separate track_setup launch (A/B)
  const int fold = env_flag("M3S_TRACK_FOLD_SETUP", true);
  if (!fold) {
    Span sp("track_setup", s);
    HIP_TRY(m3s_launch_track_setup(&a, &p, s), "track setup launch");
  }
  (void)first_chunk;  // ignored (include/m3s.h)
  const int nparts = std::min(track_nparts(N), m3s_track_max_parts());  // every block co-resident
  TrackMirror* mirror = pinned_mirror();
  if (mirror == nullptr) return fail(M3S_EHIP, "track: pinned result mirror allocation failed");
  static thread_local unsigned gen = 0;
  TrackPublish pub{mirror, a.tick + M3S_TRACK_PUBLISH_TICKET, ++gen};
  const TrackPublish no_pub{nullptr, pub.ticket, 0u};
  // The folded GN launch counts the unique matches and publishes the result itself, from its last block to leave:
  // no kernel boundary and no second counting pass between the last solve and the host seeing the result.
  // M3S_TRACK_PUBLISH_GN=0 keeps the count and the publish in the fuse launch (A/B), as does the separate setup.
  const bool pub_gn = fold && env_flag("M3S_TRACK_PUBLISH_GN", true);
  {
    Span sp("gn_iters", s);
    HIP_TRY(m3s_launch_track_iters(&a, &p, nparts, fold, pub_gn ? &pub : &no_pub, s), "track iterate launch");
  }
  // keyframe.update_pointmap(T_CkCf.act(Xkf), Ckf) after a successful solve (tracker.py:91-101): enqueued
  // before the readback, it runs only if the solve finished with a pose. It also clears the GN hand-off words and
  // the counters for the next frame (behind the kernel boundary: GN blocks poll them until they exit) and, when the
  // GN launch has not, counts the byte map and publishes. The call returns once the result is published (the fusion
  // blocks may still be running: later work on this stream is ordered after them).
  HIP_TRY(m3s_launch_fuse(&a, &fa, (p.direct || pub_gn) ? 0 : 1, N, pub_gn ? &no_pub : &pub, s), "track fuse launch");
  if (int rc = wait_published(mirror, pub.gen, s)) return rc;
  const TrackState& hs = mirror->s;
  if (hs.status == M3S_TRACK_STALLED)  // the scratch stays unrecorded: the next call on it runs track_init
    return fail(M3S_EHIP, "track: the persistent GN launch's hand-off stalled (its blocks were not co-resident); "
                          "no pose for this frame");
  {
    std::lock_guard<std::mutex> lock(g_track_clean_mu);
    // this frame's launches clear what it dirtied: the byte map by whoever counted it, the rest by the fuse launch,
    // which the next frame's kernels are stream-ordered behind
    g_track_clean[workspace] = {workspace_bytes, N};
  }
  memcpy(result->T_WCf, hs.T_WCf, sizeof(result->T_WCf));
  memcpy(result->T_CkCf, hs.T, sizeof(result->T_CkCf));
  result->cost = hs.last_cost;
  result->iters = hs.iter;
  result->status = hs.status;
  result->n_valid_opt = hs.n_valid_opt;
  result->n_valid_kf = hs.n_valid_kf;
  result->n_unique = hs.n_unique;
  result->N = N;
  return M3S_OK;
}
