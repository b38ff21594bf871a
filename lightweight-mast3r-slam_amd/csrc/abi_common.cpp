// C ABI of libm3s.so (include/m3s.h), the part every subsystem shares: the last-error text, the per-kernel timing
// spans, the pinned upload stage, the ABI version and the measured-peak probe. The subsystems' entry points (argument
// validation, workspace carving, host-side planning and launch sequencing) live in abi_match.cpp, abi_track.cpp,
// abi_ba.cpp, abi_retrieval.cpp, abi_map.cpp and abi_rope.cpp; the kernels in the .hip files. No torch types anywhere.
#include "abi_common.h"

#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

#include "m3s_peaks.h"

namespace m3s_abi {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int hip_fail(hipError_t e, const char* where) {
  return fail(M3S_EHIP, std::string(where) + ": " + hipGetErrorString(e));
}

// Events come from a pool that is created once and recycled by m3s_timing_reset: creating events
// per launch costs host time inside the measured loop.
namespace {
struct TimedSpan {
  hipEvent_t a, b;
};
}  // namespace
static std::map<std::string, std::vector<TimedSpan>> g_spans;
static std::vector<hipEvent_t> g_event_pool;  // free events
bool g_timing = false;

static hipEvent_t pool_event() {
  if (g_event_pool.empty()) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
  }
  hipEvent_t e = g_event_pool.back();
  g_event_pool.pop_back();
  return e;
}

void Span::begin() {
  a = pool_event();
  b = pool_event();
  if (a == nullptr || b == nullptr) {
    a = b = nullptr;
    return;
  }
  (void)hipEventRecord(a, s);
}

void Span::end() {
  (void)hipEventRecord(b, s);
  g_spans[name].push_back({a, b});
}

// pinned staging for the table uploads; reused across uploads once the previous one has landed
namespace {
struct PlanStage {
  std::mutex mu;
  char* buf = nullptr;
  size_t cap = 0;
  hipEvent_t landed = nullptr;
  bool pending = false;
};
}  // namespace
// one staging buffer + event per device: an event recorded on another device's stream would fail, and plans
// for different GPUs need not serialise on one mutex
static PlanStage& plan_stage() {
  static std::mutex map_mu;
  static std::map<int, PlanStage> stages;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(map_mu);
  return stages[dev];  // std::map nodes never move
}
// With st.mu held: wait until the previous upload through the stage has landed and make it hold `bytes`.
static hipError_t stage_reserve(PlanStage& st, size_t bytes) {
  hipError_t e = hipSuccess;
  if (st.pending) e = hipEventSynchronize(st.landed);
  st.pending = false;
  if (e == hipSuccess && !st.landed) e = hipEventCreateWithFlags(&st.landed, hipEventDisableTiming);
  if (e == hipSuccess && st.cap < bytes) {
    if (st.buf) (void)hipHostFree(st.buf);
    st.buf = nullptr;
    st.cap = 0;
    const size_t want = std::max(bytes, (size_t)1 << 20);
    e = hipHostMalloc((void**)&st.buf, want, hipHostMallocDefault);
    if (e == hipSuccess) st.cap = want;
  }
  return e;
}

size_t upload_bytes(const UploadSec* secs, int nsec) {
  size_t total = 0;
  for (int i = 0; i < nsec; i++) total += (secs[i].bytes + 15) & ~(size_t)15;
  return total;
}

int stage_upload(const UploadSec* secs, int nsec, void* dev, hipStream_t s, const UploadNames& names) {
  const size_t total = upload_bytes(secs, nsec);
  PlanStage& st = plan_stage();
  std::lock_guard<std::mutex> lock(st.mu);
  HIP_TRY(stage_reserve(st, total), names.reserve);
  size_t off = 0;
  for (int i = 0; i < nsec; i++) {
    if (secs[i].bytes) memcpy(st.buf + off, secs[i].src, secs[i].bytes);
    if (secs[i].dst) *secs[i].dst = static_cast<char*>(dev) + off;
    off += (secs[i].bytes + 15) & ~(size_t)15;
  }
  if (total) HIP_TRY(hipMemcpyAsync(dev, st.buf, total, hipMemcpyHostToDevice, s), names.copy);
  HIP_TRY(hipEventRecord(st.landed, s), names.record);
  st.pending = true;
  return M3S_OK;
}

}  // namespace m3s_abi

using namespace m3s_abi;

extern "C" void m3s_timing_enable(int on) {
  g_timing = on != 0;
  while (g_timing && g_event_pool.size() < 1024) {  // pre-create outside any timed loop
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) break;
    g_event_pool.push_back(e);
  }
}

extern "C" void m3s_timing_reset(void) {
  for (auto& kv : g_spans)
    for (auto& sp : kv.second) {
      g_event_pool.push_back(sp.a);
      g_event_pool.push_back(sp.b);
    }
  g_spans.clear();
}

// total milliseconds and span count recorded under `name` (synchronises the recorded events)
extern "C" int m3s_timing_query(const char* name, double* total_ms, int* count) {
  *total_ms = 0.0;
  *count = 0;
  auto it = g_spans.find(name);
  if (it == g_spans.end()) return M3S_OK;
  for (auto& sp : it->second) {
    HIP_TRY(hipEventSynchronize(sp.b), "timing sync");
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, sp.a, sp.b), "timing elapsed");
    *total_ms += ms;
    *count += 1;
  }
  return M3S_OK;
}

extern "C" int m3s_abi_version(void) { return M3S_ABI_VERSION; }
extern "C" const char* m3s_last_error(void) { return g_err.c_str(); }

// measured peak (bench roofline context only)
extern "C" int m3s_peak_fma_f32(float* out_dev, int blocks, int iters, void* stream) {
  M3S_CHECK(out_dev && blocks > 0 && iters > 0, "peak: bad argument");
  HIP_TRY(m3s_launch_peak_fma_f32(out_dev, blocks, iters, (hipStream_t)stream), "peak launch");
  return M3S_OK;
}
