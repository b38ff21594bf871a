// What the abi_*.cpp translation units of libm3s.so share: error plumbing, workspace carving, the per-kernel timing
// spans, the boolean environment toggles and the per-device pinned upload stage. Not part of the C ABI
// (include/m3s.h); nothing here is exported from the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/m3s.h"

namespace m3s_abi __attribute__((visibility("hidden"))) {

extern thread_local std::string g_err;  // m3s_last_error's text (abi_common.cpp)

int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* where);

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* b) : base(static_cast<char*>(b)) {}
  template <typename T>
  T* take(size_t count) {
    T* p = reinterpret_cast<T*>(base ? base + off : nullptr);
    off += align256(sizeof(T) * (count > 0 ? count : 1));
    return p;
  }
};

#define M3S_CHECK(cond, msg)                 \
  do {                                       \
    if (!(cond)) return fail(M3S_EINVAL, msg); \
  } while (0)

#define HIP_TRY(expr, where)                \
  do {                                      \
    hipError_t _e = (expr);                 \
    if (_e != hipSuccess) return hip_fail(_e, where); \
  } while (0)

// ---- per-kernel HIP-event timing (bench.py reads it; off by default, zero cost when off) ----
extern bool g_timing;
struct Span {
  hipStream_t s;
  hipEvent_t a = nullptr, b = nullptr;
  const char* name;
  Span(const char* n, hipStream_t st) : s(st), name(n) {
    if (g_timing) begin();
  }
  ~Span() {
    if (g_timing && a != nullptr) end();
  }
  void begin();
  void end();
};

// A boolean environment toggle, read per call (tests flip them between calls): unset -> dflt, "0" -> off, any other
// value -> on.
inline bool env_flag(const char* name, bool dflt) {
  const char* v = getenv(name);
  return v == nullptr ? dflt : strcmp(v, "0") != 0;
}

// ---- host tables -> device through the per-device pinned stage ----
// One section of an upload: `bytes` from `src`, packed at the next 16-byte offset; *dst (nullable) receives its
// device address.
struct UploadSec {
  const void* src;
  size_t bytes;
  const void** dst;
};
// the hip_fail `where` strings of the three steps an upload can fail in
struct UploadNames {
  const char *reserve, *copy, *record;
};
size_t upload_bytes(const UploadSec* secs, int nsec);  // the packed size: every section padded to 16 bytes
// Pack the sections into the stage (reused once its previous upload has landed), copy them to `dev` in one
// hipMemcpyAsync on `s` (none when every section is empty) and record the stage's landed event behind it.
int stage_upload(const UploadSec* secs, int nsec, void* dev, hipStream_t s, const UploadNames& names);

// ---- shared by the BA plan (abi_ba.cpp, which defines ba_calib_rays) and the map export (abi_map.cpp) ----
// The pixel-ray tables of raw calib (m3s_ba_calib_rays): x_of_u (width floats), y_of_v (height floats)
void ba_calib_rays(const m3s_ba_config* cfg, float* x_of_u, float* y_of_v);
// The factor that turns a keyframe's confidence sum into its average: torch's C / N on a device tensor is
// C * float32(1/N) (Frame.get_average_conf, frame.py:93-94). One definition for the BA pack and the map export.
inline float conf_scale(float n_avg) { return 1.0f / n_avg; }
// floats of the raw-calib pixel-ray tables (W + H with W H = N, so at most N + 1; W, H < 65536)
inline size_t ba_ray_tab_floats(int N) { return (size_t)N + 1 < (size_t)2 * 65535 ? (size_t)N + 1 : (size_t)2 * 65535; }

}  // namespace m3s_abi
