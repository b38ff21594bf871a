// C ABI of libm3s.so (include/m3s.h): the map export (evaluate.py:47-70). Kernels live in map.hip.
#include "abi_common.h"

#include <cmath>
#include <vector>

#include "m3s_map.h"

using namespace m3s_abi;

namespace {
constexpr int MAP_MAX_BLOCKS = 1 << 23;  // one block per MAP_TILE pixels: the grid of both passes

struct MapWs {
  MapHeader* header;
  unsigned long long* dropped;  // behind the header, in its 256-byte slot (voxel stage)
  uint64_t* mask;
  uint32_t* bcnt;
  int64_t* boff;
  int64_t* kcnt;
  char* tab_count;  // C pointers, scales (uploaded by the count)
  char* tab_write;  // X pointers, rgb pointers, ray tables (uploaded by the write)
};

inline int map_bpk(int N) { return (N + MAP_TILE - 1) / MAP_TILE; }
inline size_t map_tab_count_bytes(int Kp) { return (size_t)Kp * 8 + 16 + (size_t)Kp * 4 + 16; }
inline size_t map_tab_write_bytes(int Kp, int N) {
  return 2 * ((size_t)Kp * 8 + 16) + ba_ray_tab_floats(N) * 4 + 16;
}

size_t map_carve(Carver& c, int Kp, int N, MapWs* w) {
  const size_t E = (size_t)Kp * map_bpk(N);
  MapHeaderSlot* slot = c.take<MapHeaderSlot>(1);  // one 256-byte slot, as the bare header took
  w->header = slot ? &slot->h : nullptr;
  w->dropped = slot ? &slot->dropped : nullptr;
  w->mask = c.take<uint64_t>(E * MAP_WORDS);
  w->bcnt = c.take<uint32_t>(E);
  w->boff = c.take<int64_t>(E + 1);
  w->kcnt = c.take<int64_t>((size_t)Kp + 1);
  w->tab_count = c.take<char>(map_tab_count_bytes(Kp));
  w->tab_write = c.take<char>(map_tab_write_bytes(Kp, N));
  return c.off;
}

bool map_sizes_ok(int Kp, int N) {
  return Kp >= 1 && Kp <= M3S_BA_MAX_POSES && N >= 1 && N <= (1 << 28) && (int64_t)Kp * map_bpk(N) <= MAP_MAX_BLOCKS;
}

// the arguments both passes share
MapArgs map_args(const m3s_map_config* cfg, const MapWs& w, int Kp, int N) {
  MapArgs a{};
  a.Kp = Kp;
  a.N = N;
  a.bpk = map_bpk(N);
  a.thresh = cfg->c_conf_threshold;
  a.header = w.header;
  a.mask = w.mask;
  a.bcnt = w.bcnt;
  a.boff = w.boff;
  a.kcnt = w.kcnt;
  return a;
}

// the argument checks both entry points share; no device is touched
int map_check(const m3s_map_config* cfg, const m3s_ba_keyframes* kf, int Kp, int N, const void* ws, size_t ws_bytes) {
  M3S_CHECK(cfg, "map: null config");
  M3S_CHECK(cfg->layout == M3S_MAP_SOA || cfg->layout == M3S_MAP_PLY, "map: layout must be M3S_MAP_SOA or M3S_MAP_PLY");
  M3S_CHECK(cfg->calib == 0 || cfg->calib == 1, "map: calib must be 0 or 1");
  M3S_CHECK(map_sizes_ok(Kp, N), "map: bad Kp or N");
  if (cfg->calib) {
    M3S_CHECK(cfg->height > 0 && cfg->width > 0 && cfg->height < 65536 && cfg->width < 65536,
              "map: calib needs 0 < height, width < 65536");
    M3S_CHECK((int64_t)cfg->height * cfg->width == N, "map: calib needs N == height * width");
  }
  M3S_CHECK(kf && kf->X && kf->C && kf->N_avg, "map: null keyframe table");
  M3S_CHECK(ws, "map: null workspace");
  if (ws_bytes < m3s_map_workspace_size(Kp, N)) return fail(M3S_ESPACE, "map: workspace too small");
  return M3S_OK;
}

// calib: the pixel-ray tables x_of_u (width) then y_of_v (height) of the write pass and the voxel stage; else empty
std::vector<float> map_ray_tab(const m3s_map_config* cfg) {
  std::vector<float> ray_tab;
  if (cfg->calib) {
    m3s_ba_config bc{};
    bc.fx = cfg->fx, bc.fy = cfg->fy, bc.cx = cfg->cx, bc.cy = cfg->cy;
    bc.height = cfg->height, bc.width = cfg->width;
    ray_tab.resize((size_t)cfg->width + cfg->height);
    ba_calib_rays(&bc, ray_tab.data(), ray_tab.data() + cfg->width);
  }
  return ray_tab;
}

// slots of the voxel table for `total` rows: a power of two >= 2 total, at least 1024; 0 if that overflows
uint64_t map_voxel_slots(int64_t total) {
  if (total < 0 || total > (int64_t)1 << 57) return 0;
  uint64_t slots = 1024;
  while (slots < 2 * (uint64_t)total) slots <<= 1;
  return slots;
}

const UploadNames kMapUpload = {"map stage", "map upload", "map stage record"};
}  // namespace

extern "C" size_t m3s_map_workspace_size(int Kp, int N) {
  if (!map_sizes_ok(Kp, N)) return 0;
  Carver c(nullptr);
  MapWs w;
  return map_carve(c, Kp, N, &w);
}

extern "C" int m3s_map_count(const m3s_map_config* cfg, const m3s_ba_keyframes* kf, int Kp, int N, int64_t* counts_out,
                             int64_t* total_out, void* ws, size_t ws_bytes, void* stream) {
  const int rc = map_check(cfg, kf, Kp, N, ws, ws_bytes);
  if (rc != M3S_OK) return rc;
  M3S_CHECK(total_out, "map: null total_out");
  std::vector<float> sh(Kp);
  for (int k = 0; k < Kp; k++) {
    M3S_CHECK(kf->C[k], "map: null keyframe buffer");
    M3S_CHECK(kf->N_avg[k] > 0.0f, "map: keyframe fusion count N must be positive");
    sh[k] = conf_scale(kf->N_avg[k]);
  }
  Carver c(ws);
  MapWs w;
  map_carve(c, Kp, N, &w);
  hipStream_t s = (hipStream_t)stream;
  MapArgs a = map_args(cfg, w, Kp, N);
  // a count that fails half way leaves no header a write would accept
  HIP_TRY(hipMemsetAsync(w.header, 0, sizeof(MapHeader), s), "map header reset");
  const UploadSec secs[] = {
      {kf->C, sizeof(const float*) * Kp, (const void**)&a.C},
      {sh.data(), sizeof(float) * Kp, (const void**)&a.scale},
  };
  const int up = stage_upload(secs, 2, w.tab_count, s, kMapUpload);
  if (up != M3S_OK) return up;
  {
    Span sp("map_count", s);
    HIP_TRY(m3s_launch_map_count(&a, s), "map count launch");
  }
  std::vector<int64_t> kc((size_t)Kp + 1);
  HIP_TRY(hipMemcpyAsync(kc.data(), w.kcnt, sizeof(int64_t) * kc.size(), hipMemcpyDeviceToHost, s), "map counts copy");
  HIP_TRY(hipStreamSynchronize(s), "map count sync");
  if (counts_out) memcpy(counts_out, kc.data(), sizeof(int64_t) * Kp);
  *total_out = kc[Kp];
  return M3S_OK;
}

extern "C" int m3s_map_write(const m3s_map_config* cfg, const m3s_ba_keyframes* kf, const float* Twc,
                             const uint8_t* const* rgb, int Kp, int N, void* out, uint8_t* out_rgb, int64_t capacity,
                             void* ws, size_t ws_bytes, void* stream) {
  const int rc = map_check(cfg, kf, Kp, N, ws, ws_bytes);
  if (rc != M3S_OK) return rc;
  M3S_CHECK(Twc, "map: null poses");
  M3S_CHECK(capacity >= 0 && (out || capacity == 0), "map: null output");
  M3S_CHECK(((uintptr_t)out & 3) == 0 && ((uintptr_t)out_rgb & 3) == 0, "map: outputs must be 4-byte aligned");
  if (cfg->layout == M3S_MAP_SOA)
    M3S_CHECK((rgb != nullptr) == (out_rgb != nullptr), "map: SOA colours need both rgb and out_rgb, or neither");
  else
    M3S_CHECK(out_rgb == nullptr, "map: the PLY layout has no separate colour output");
  for (int k = 0; k < Kp; k++) M3S_CHECK(kf->X[k] && (!rgb || rgb[k]), "map: null keyframe buffer");
  Carver c(ws);
  MapWs w;
  map_carve(c, Kp, N, &w);
  hipStream_t s = (hipStream_t)stream;
  // the count this write belongs to: its header, read back (32 B; orders after the stream's earlier work)
  MapHeader h;
  HIP_TRY(hipMemcpyAsync(&h, w.header, sizeof(h), hipMemcpyDeviceToHost, s), "map header copy");
  HIP_TRY(hipStreamSynchronize(s), "map header sync");
  M3S_CHECK(h.magic == MAP_MAGIC, "map: no m3s_map_count preceded this write on the workspace");
  uint32_t tb;
  memcpy(&tb, &cfg->c_conf_threshold, 4);
  M3S_CHECK(h.Kp == Kp && h.N == N && h.thresh_bits == tb, "map: shapes or threshold differ from the workspace's count");
  M3S_CHECK(capacity >= h.total, "map: capacity below the counted total");
  if (h.total == 0) return M3S_OK;
  MapArgs a = map_args(cfg, w, Kp, N);
  a.calib = cfg->calib;
  a.W = cfg->calib ? cfg->width : 0;
  a.layout = cfg->layout;
  a.capacity = capacity;
  a.Twc = Twc;
  a.out = out;
  a.out_rgb = out_rgb;
  const std::vector<float> ray_tab = map_ray_tab(cfg);
  const UploadSec secs[] = {
      {kf->X, sizeof(const float*) * Kp, (const void**)&a.X},
      {rgb, rgb ? sizeof(const uint8_t*) * Kp : 0, (const void**)&a.rgb},
      {ray_tab.data(), sizeof(float) * ray_tab.size(), (const void**)&a.ray_tab},
  };
  const int up = stage_upload(secs, 3, w.tab_write, s, kMapUpload);
  if (up != M3S_OK) return up;
  if (!rgb) a.rgb = nullptr;
  {
    Span sp("map_write", s);
    HIP_TRY(m3s_launch_map_write(&a, s), "map write launch");
  }
  return M3S_OK;
}

extern "C" size_t m3s_map_voxel_table_size(int64_t total) {
  return (size_t)map_voxel_slots(total) * sizeof(MapVoxSlot);
}

extern "C" int m3s_map_voxel(const m3s_map_config* cfg, const m3s_ba_keyframes* kf, const float* Twc, int Kp, int N,
                             float voxel_size, void* table, size_t table_bytes, int64_t* counts_out,
                             int64_t* total_out, int64_t* dropped_out, void* ws, size_t ws_bytes, void* stream) {
  const int rc = map_check(cfg, kf, Kp, N, ws, ws_bytes);
  if (rc != M3S_OK) return rc;
  M3S_CHECK(Twc, "map: null poses");
  M3S_CHECK(total_out, "map: null total_out");
  M3S_CHECK(std::isfinite(voxel_size) && voxel_size > 0.0f, "map: voxel_size must be finite and positive");
  M3S_CHECK(table, "map: null voxel table");
  M3S_CHECK(((uintptr_t)table & 15) == 0, "map: the voxel table must be 16-byte aligned");
  M3S_CHECK((int64_t)Kp * N < ((int64_t)1 << 32), "map: the voxel stage needs Kp * N < 2^32");
  std::vector<float> sh(Kp);
  for (int k = 0; k < Kp; k++) {
    M3S_CHECK(kf->X[k] && kf->C[k], "map: null keyframe buffer");
    M3S_CHECK(kf->N_avg[k] > 0.0f, "map: keyframe fusion count N must be positive");
    sh[k] = conf_scale(kf->N_avg[k]);
  }
  Carver c(ws);
  MapWs w;
  map_carve(c, Kp, N, &w);
  hipStream_t s = (hipStream_t)stream;
  // the count this stage belongs to: the write's header check
  MapHeader h;
  HIP_TRY(hipMemcpyAsync(&h, w.header, sizeof(h), hipMemcpyDeviceToHost, s), "map header copy");
  HIP_TRY(hipStreamSynchronize(s), "map header sync");
  M3S_CHECK(h.magic == MAP_MAGIC, "map: no m3s_map_count preceded the voxel stage on the workspace");
  uint32_t tb;
  memcpy(&tb, &cfg->c_conf_threshold, 4);
  M3S_CHECK(h.Kp == Kp && h.N == N && h.thresh_bits == tb, "map: shapes or threshold differ from the workspace's count");
  const uint64_t slots = map_voxel_slots(h.total);
  M3S_CHECK(slots > 0, "map: counted total out of range");
  if (table_bytes < slots * sizeof(MapVoxSlot)) return fail(M3S_ESPACE, "map: voxel table too small for the counted total");
  if (h.total == 0) {
    if (counts_out) memset(counts_out, 0, sizeof(int64_t) * Kp);
    *total_out = 0;
    if (dropped_out) *dropped_out = 0;
    return M3S_OK;
  }
  MapArgs a = map_args(cfg, w, Kp, N);
  a.calib = cfg->calib;
  a.W = cfg->calib ? cfg->width : 0;
  a.Twc = Twc;
  a.vox_r = 1.0f / voxel_size;
  a.vtab = static_cast<MapVoxSlot*>(table);
  a.vox_mask = slots - 1;
  a.dropped = w.dropped;
  const std::vector<float> ray_tab = map_ray_tab(cfg);
  // the count's tables again (C pointers, scales: the caller's table need not be the count's allocation), and the
  // write's X pointers and ray tables, each through its own staging region
  const UploadSec secs_c[] = {
      {kf->C, sizeof(const float*) * Kp, (const void**)&a.C},
      {sh.data(), sizeof(float) * Kp, (const void**)&a.scale},
  };
  int up = stage_upload(secs_c, 2, w.tab_count, s, kMapUpload);
  if (up != M3S_OK) return up;
  const UploadSec secs_w[] = {
      {kf->X, sizeof(const float*) * Kp, (const void**)&a.X},
      {ray_tab.data(), sizeof(float) * ray_tab.size(), (const void**)&a.ray_tab},
  };
  up = stage_upload(secs_w, 2, w.tab_write, s, kMapUpload);
  if (up != M3S_OK) return up;
  HIP_TRY(hipMemsetAsync(table, 0xff, slots * sizeof(MapVoxSlot), s), "map voxel table reset");
  // the header and the dropped counter behind it: a stage that fails half way leaves no header a write would accept
  // (the re-scan writes it again)
  HIP_TRY(hipMemsetAsync(w.header, 0, sizeof(MapHeaderSlot), s), "map header reset");
  {
    Span sp("map_voxel", s);
    HIP_TRY(m3s_launch_map_voxel(&a, s), "map voxel launch");
  }
  std::vector<int64_t> kc((size_t)Kp + 1);
  unsigned long long dropped = 0;
  HIP_TRY(hipMemcpyAsync(kc.data(), w.kcnt, sizeof(int64_t) * kc.size(), hipMemcpyDeviceToHost, s), "map counts copy");
  HIP_TRY(hipMemcpyAsync(&dropped, w.dropped, sizeof(dropped), hipMemcpyDeviceToHost, s), "map dropped copy");
  HIP_TRY(hipStreamSynchronize(s), "map voxel sync");
  if (counts_out) memcpy(counts_out, kc.data(), sizeof(int64_t) * Kp);
  *total_out = kc[Kp];
  if (dropped_out) *dropped_out = (int64_t)dropped;
  return M3S_OK;
}
