// C ABI of libm3s.so (include/m3s.h): RoPE2D, the `curope` operator surface of the MASt3R ViT (curope.cpp:49-65,
// kernels.cu:17-108). The kernel lives in rope.hip; this file owns the cos / sin tables and their per-device cache.
#include "abi_common.h"

#include <cmath>
#include <cstdint>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "m3s_rope.h"

using namespace m3s_abi;

namespace {

// The table's one statement, host fp64: inv[t] = double(fwd) / pow(double(base), double(t) / Q), and for p < P the
// angle a = p inv[t], cos[p Q + t] = float(cos(a)), sin[p Q + t] = float(sin(a)). Fills what is not null. Both the
// device table (rope_table) and m3s_rope2d_table come from here.
void rope_fill(float base, float fwd, int Q, int P, float* cos_out, float* sin_out, double* inv_out) {
  for (int t = 0; t < Q; t++) {
    const double inv = (double)fwd / std::pow((double)base, (double)t / Q);
    if (inv_out) inv_out[t] = inv;
    for (int p = 0; p < P; p++) {
      const double a = p * inv;
      if (cos_out) cos_out[(size_t)p * Q + t] = (float)std::cos(a);
      if (sin_out) sin_out[(size_t)p * Q + t] = (float)std::sin(a);
    }
  }
}

uint32_t float_bits(float x) {
  uint32_t b;
  memcpy(&b, &x, 4);
  return b;
}

// (device, base bits, fwd bits, Q) -> the device table; entries live until m3s_rope2d_release on their device
typedef std::tuple<int, uint32_t, uint32_t, int> RopeKey;
struct RopeEntry {
  void* buf = nullptr;
  RopeTable tab{};
};
std::mutex g_rope_mu;
std::map<RopeKey, RopeEntry> g_rope_tables;

// The table of (base, fwd, Q) on the current device; built and uploaded synchronously on first use (not legal
// inside a stream capture: m3s_rope2d_prepare beforehand).
int rope_table(float base, float fwd, int Q, hipStream_t s, RopeTable* out) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev), "rope device query");
  const RopeKey key(dev, float_bits(base), float_bits(fwd), Q);
  std::lock_guard<std::mutex> lock(g_rope_mu);
  auto it = g_rope_tables.find(key);
  if (it != g_rope_tables.end()) {
    *out = it->second.tab;
    return M3S_OK;
  }
  const size_t n = (size_t)ROPE_TABLE_P * Q;
  // one host image of the allocation: cos | sin | inv (n floats each, then Q doubles; 2 n floats keep inv 8-aligned)
  std::vector<char> host(2 * n * sizeof(float) + (size_t)Q * sizeof(double));
  float* hc = reinterpret_cast<float*>(host.data());
  double* hi = reinterpret_cast<double*>(host.data() + 2 * n * sizeof(float));
  rope_fill(base, fwd, Q, ROPE_TABLE_P, hc, hc + n, hi);
  RopeEntry e;
  HIP_TRY(hipMalloc(&e.buf, host.size()), "rope table alloc");
  hipError_t err = hipMemcpyAsync(e.buf, host.data(), host.size(), hipMemcpyHostToDevice, s);
  if (err == hipSuccess) err = hipStreamSynchronize(s);  // the pageable host image dies with this call
  if (err != hipSuccess) {
    (void)hipFree(e.buf);
    return hip_fail(err, "rope table upload");
  }
  e.tab.cos = static_cast<const float*>(e.buf);
  e.tab.sin = e.tab.cos + n;
  e.tab.inv = reinterpret_cast<const double*>(e.tab.sin + n);
  g_rope_tables[key] = e;
  *out = e.tab;
  return M3S_OK;
}

bool rope_params_ok(float base, float fwd, int Q) {
  return std::isfinite(base) && base > 0.0f && std::isfinite(fwd) && Q >= 1 && Q <= (1 << 20);
}

}  // namespace

extern "C" int m3s_rope2d_table(float base, float fwd, int Q, int P, float* cos_out, float* sin_out) {
  M3S_CHECK(rope_params_ok(base, fwd, Q), "rope2d: base must be finite and positive, fwd finite, 1 <= Q <= 2^20");
  M3S_CHECK(P >= 0 && (int64_t)P * Q <= ((int64_t)1 << 30), "rope2d: bad table rows P");
  M3S_CHECK(P == 0 || (cos_out && sin_out), "rope2d: null table output");
  rope_fill(base, fwd, Q, P, cos_out, sin_out, nullptr);
  return M3S_OK;
}

extern "C" int m3s_rope2d_prepare(float base, float fwd, int Q, void* stream) {
  M3S_CHECK(rope_params_ok(base, fwd, Q), "rope2d: base must be finite and positive, fwd finite, 1 <= Q <= 2^20");
  RopeTable tab;
  return rope_table(base, fwd, Q, (hipStream_t)stream, &tab);
}

extern "C" int m3s_rope2d_release(void) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev), "rope device query");
  std::lock_guard<std::mutex> lock(g_rope_mu);
  hipError_t err = hipSuccess;
  for (auto it = g_rope_tables.begin(); it != g_rope_tables.end();) {
    if (std::get<0>(it->first) == dev) {
      const hipError_t e = hipFree(it->second.buf);  // waits for the device's launches that read it
      if (err == hipSuccess) err = e;
      it = g_rope_tables.erase(it);
    } else {
      ++it;
    }
  }
  if (err != hipSuccess) return hip_fail(err, "rope table free");
  return M3S_OK;
}

extern "C" int m3s_rope2d(int dtype, void* tokens, int64_t stride_b, int64_t stride_n, const int64_t* pos, int B, int N,
                          int H, int D, float base, float fwd, void* stream) {
  M3S_CHECK(dtype >= 0 && dtype <= 2, "rope2d: dtype must be 0 (f16), 1 (f32) or 2 (bf16)");
  M3S_CHECK(B >= 0 && N >= 0 && H >= 0 && D >= 0, "rope2d: negative size");
  M3S_CHECK(D % 4 == 0, "rope2d: token dim must be multiple of 4");
  if ((int64_t)B * N * H == 0 || D == 0) return M3S_OK;
  M3S_CHECK(tokens && pos, "rope2d: null pointer");
  const int Q = D / 4;
  M3S_CHECK(rope_params_ok(base, fwd, Q), "rope2d: base must be finite and positive, fwd finite, D <= 2^22");
  M3S_CHECK((int64_t)B * N < ((int64_t)1 << 40), "rope2d: B * N must be below 2^40");
  const size_t es = dtype == 1 ? 4 : 2;
  M3S_CHECK(((uintptr_t)tokens & (es - 1)) == 0 && ((uintptr_t)pos & 7) == 0, "rope2d: misaligned pointer");

  RopeArgs a{};
  a.tokens = tokens;
  a.pos = pos;
  a.stride_b = stride_b, a.stride_n = stride_n;
  a.B = B, a.N = N, a.H = H, a.D = D, a.Q = Q;
  a.dtype = dtype;
  // the vector path: whole 16-byte chunks per quarter, and every row start a lane can reach 16-byte aligned (the
  // head stride D and the quarter offsets then are too)
  a.vec = (Q * es) % 16 == 0 && ((uintptr_t)tokens & 15) == 0 && ((uint64_t)stride_b * es) % 16 == 0 &&
          ((uint64_t)stride_n * es) % 16 == 0;
  const int64_t per_head = 2 * (int64_t)(a.vec ? Q / (16 / es) : Q);  // lanes of one token's head row
  // heads per lane: as many (up to ROPE_MAX_HPL) as leave at least 49,152 lanes, 768 waves or three per CU (the ViT's
  // shapes then keep a table chunk for two heads in f32 and for one or two in f16)
  int hpl = ROPE_MAX_HPL;
  while (hpl > 1 && (int64_t)B * N * ((H + hpl - 1) / hpl) * per_head < 49152) hpl >>= 1;
  a.HG = (H + hpl - 1) / hpl;
  M3S_CHECK((int64_t)a.HG * per_head <= 0x7fffffff, "rope2d: H * D too large");
  a.lanes = (int64_t)B * N * a.HG * per_head;
  M3S_CHECK((a.lanes + ROPE_BLOCK - 1) / ROPE_BLOCK <= 0x7fffffff, "rope2d: too many tokens for one launch");

  hipStream_t s = (hipStream_t)stream;
  const int rc = rope_table(base, fwd, Q, s, &a.tab);
  if (rc != M3S_OK) return rc;
  {
    Span sp("rope2d", s);
    HIP_TRY(m3s_launch_rope2d(&a, s), "rope2d launch");
  }
  return M3S_OK;
}
