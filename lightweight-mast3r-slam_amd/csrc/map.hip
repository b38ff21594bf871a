// Map export (m3s_map_count / m3s_map_write, include/m3s.h): the confidence-filtered world point cloud of the
// keyframes, in keyframe order and pixel order, read from the keyframes' own buffers.
// Replaces the per-keyframe host loop of the reference's evaluate.save_reconstruction
// (mast3r_slam/evaluate.py:47-70): constrain_points_to_ray, T_WC.act, three .cpu().numpy() copies, a
// boolean index per keyframe and a final concatenate.
//
// Three launches. Pass A (map_count_kernel) reads only C: every wave ballots its 64 pixels into one validity word
// (1 bit per point) and every block of MAP_TILE pixels stores its valid count. map_scan_kernel, one workgroup, turns
// the block counts into 64-bit first-row offsets, per-keyframe counts and the total. Pass B (map_write_kernel) takes
// validity from the stored words ONLY: the keyframes live in buffers a tracking process fuses into concurrently, and a
// mask re-derived from a changed C would disagree with the offsets. Output rows are placed by offset + rank (wave64
// mbcnt on the validity word), so the order is deterministic and no atomic append is needed.
//
// Built with -ffp-contract=off: the world point is Sim3.act's fp32 operation sequence (m3s/sim3.py:27-31,121-125),
// one rounding per operation, which is m3s::actSim3 without contraction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "m3s_common.hpp"
#include "m3s_map.h"

namespace m3s {

// ---- pass A: validity words + block counts ----
__global__ void __launch_bounds__(256) map_count_kernel(MapArgs a) {
  __shared__ int s_cnt[MAP_WORDS];
  const int blk = blockIdx.x;
  const int k = blk / a.bpk, b = blk - k * a.bpk;
  const float* __restrict__ C = a.C[k];
  const float inv = a.scale[k];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < MAP_WORDS / 4; j++) {
    const int w = j * 4 + wave;
    const int n = b * MAP_TILE + w * 64 + lane;
    bool v = false;
    if (n < a.N) v = C[n] * inv > a.thresh;  // strict: NaN drops
    const unsigned long long word = __ballot(v);
    if (lane == 0) {
      a.mask[(size_t)blk * MAP_WORDS + w] = word;
      s_cnt[w] = __popcll(word);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
#pragma unroll
    for (int i = 0; i < MAP_WORDS; i++) c += s_cnt[i];
    a.bcnt[blk] = (uint32_t)c;
  }
}

// ---- exclusive scan of the block counts: one workgroup, tiles of 1024 entries with a running carry ----
__global__ void __launch_bounds__(1024) map_scan_kernel(MapArgs a) {
  __shared__ long long s_wave[16];
  const int E = a.Kp * a.bpk;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long carry = 0;
  for (int base = 0; base < E; base += 1024) {
    const int i = base + (int)threadIdx.x;
    const long long v = i < E ? (long long)a.bcnt[i] : 0;
    long long inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const long long t = __shfl_up(inc, off, 64);
      if (lane >= off) inc += t;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    long long wbase = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 16; w++) {
      const long long s = s_wave[w];
      if (w < wave) wbase += s;
      tot += s;
    }
    if (i < E) a.boff[i] = carry + wbase + inc - v;
    carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) a.boff[E] = carry;
  __syncthreads();
  for (int k = threadIdx.x; k < a.Kp; k += 1024)
    a.kcnt[k] = a.boff[(size_t)(k + 1) * a.bpk] - a.boff[(size_t)k * a.bpk];
  if (threadIdx.x == 0) {
    a.kcnt[a.Kp] = carry;
    MapHeader h;
    h.magic = MAP_MAGIC;
    h.Kp = a.Kp;
    h.N = a.N;
    h.thresh_bits = __float_as_uint(a.thresh);
    h.pad = 0;
    h.total = carry;
    *a.header = h;
  }
}

// Copy the LDS byte stream s[a, a + nb) to g[a, a + nb), g 4-byte aligned and s its image (s[i] <-> g[i]): the aligned
// interior as dwords, the up-to-3 head and tail bytes as byte stores (the neighbouring block owns the other bytes of
// those dwords, so a dword store there would race).
__device__ __forceinline__ void map_flush(const unsigned char* s, unsigned char* g, int a, int nb) {
  const int e = a + nb;
  const int d0 = (a + 3) >> 2, d1 = e >> 2;
  const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
  uint32_t* g4 = reinterpret_cast<uint32_t*>(g);
  for (int d = d0 + (int)threadIdx.x; d < d1; d += (int)blockDim.x) g4[d] = s4[d];
  const int h_end = min(4 * d0, e);
  if (threadIdx.x < 4) {
    const int i = a + (int)threadIdx.x;
    if (i < h_end) g[i] = s[i];
  } else if (threadIdx.x < 8) {
    const int i = max(4 * d1, h_end) + (int)threadIdx.x - 4;
    if (i < e) g[i] = s[i];
  }
}

constexpr int MAP_RGB_BASE = MAP_TILE * 12;       // SOA staging: xyz rows, then the rgb byte stream
constexpr int MAP_LDS_BYTES = MAP_TILE * 15 + 16;  // PLY: 4 + 15 TILE; SOA: 12 TILE + 4 + 3 TILE

// ---- pass B: transform + compact, validity from the stored words ----
template <int LAYOUT, bool CALIB>
__global__ void __launch_bounds__(256) map_write_kernel(MapArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char s_buf[MAP_LDS_BYTES];
  __shared__ unsigned long long s_word[MAP_WORDS];
  const int blk = blockIdx.x;
  const int k = blk / a.bpk, b = blk - k * a.bpk;
  const long long off = a.boff[blk];
  // rows of this block inside the caller's capacity (the ABI rejects capacity < total; the clamp also keeps a
  // workspace that was overwritten since its count from reaching past the output)
  const long long room = a.capacity - off;
  const long long want = a.boff[blk + 1] - off;
  const int nrows = (int)max(0ll, min(min(want, room), (long long)MAP_TILE));
  if (off < 0 || nrows <= 0) return;
  if (threadIdx.x < MAP_WORDS) s_word[threadIdx.x] = a.mask[(size_t)blk * MAP_WORDS + threadIdx.x];
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* __restrict__ X = a.X[k];
  const uint8_t* __restrict__ rgb = a.rgb ? a.rgb[k] : nullptr;
  float T[8];
#pragma unroll
  for (int c = 0; c < 8; c++) T[c] = a.Twc[(size_t)k * 8 + c];
  const int aP = (int)((15 * off) & 3), a3 = (int)((3 * off) & 3);

#pragma unroll
  for (int j = 0; j < MAP_WORDS / 4; j++) {
    const int w = j * 4 + wave;
    const unsigned long long word = s_word[w];
    int pre = 0;
    for (int i = 0; i < w; i++) pre += __popcll(s_word[i]);
    const int rank = pre + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(word >> 32),
                                                          __builtin_amdgcn_mbcnt_lo((unsigned)word, 0u));
    const int n = b * MAP_TILE + w * 64 + lane;
    if (((word >> lane) & 1ull) == 0 || rank >= nrows || n >= a.N) continue;
    float p[3], y[3];
    if constexpr (CALIB) {
      const float z = X[(size_t)n * 3 + 2];
      const int v = n / a.W, u = n - v * a.W;
      p[0] = z * a.ray_tab[u];
      p[1] = z * a.ray_tab[a.W + v];
      p[2] = z;
    } else {
      p[0] = X[(size_t)n * 3 + 0];
      p[1] = X[(size_t)n * 3 + 1];
      p[2] = X[(size_t)n * 3 + 2];
    }
    actSim3(T, p, y);
    unsigned char c0 = 0, c1 = 0, c2 = 0;
    if (rgb) {
      c0 = rgb[(size_t)n * 3 + 0];
      c1 = rgb[(size_t)n * 3 + 1];
      c2 = rgb[(size_t)n * 3 + 2];
    }
    if constexpr (LAYOUT == 1) {  // PLY record: x, y, z little-endian f32, then r, g, b
      unsigned char* r = s_buf + aP + 15 * rank;
      __builtin_memcpy(r, y, 12);
      r[12] = c0;
      r[13] = c1;
      r[14] = c2;
    } else {
      float* r = reinterpret_cast<float*>(s_buf) + 3 * rank;
      r[0] = y[0];
      r[1] = y[1];
      r[2] = y[2];
      if (rgb) {
        unsigned char* q = s_buf + MAP_RGB_BASE + a3 + 3 * rank;
        q[0] = c0;
        q[1] = c1;
        q[2] = c2;
      }
    }
  }
  __syncthreads();
  if constexpr (LAYOUT == 1) {
    map_flush(s_buf, static_cast<unsigned char*>(a.out) + (15 * off - aP), aP, 15 * nrows);
  } else {
    map_flush(s_buf, static_cast<unsigned char*>(a.out) + 12 * off, 0, 12 * nrows);
    if (rgb) map_flush(s_buf + MAP_RGB_BASE, a.out_rgb + (3 * off - a3), a3, 3 * nrows);
  }
}

}  // namespace m3s

extern "C" hipError_t m3s_launch_map_count(const MapArgs* a, hipStream_t s) {
  const int E = a->Kp * a->bpk;
  hipLaunchKernelGGL(m3s::map_count_kernel, dim3(E), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(m3s::map_scan_kernel, dim3(1), dim3(1024), 0, s, *a);
  return hipGetLastError();
}

extern "C" hipError_t m3s_launch_map_write(const MapArgs* a, hipStream_t s) {
  const dim3 grid(a->Kp * a->bpk), block(256);
  if (a->layout == 1) {
    if (a->calib) hipLaunchKernelGGL((m3s::map_write_kernel<1, true>), grid, block, 0, s, *a);
    else hipLaunchKernelGGL((m3s::map_write_kernel<1, false>), grid, block, 0, s, *a);
  } else {
    if (a->calib) hipLaunchKernelGGL((m3s::map_write_kernel<0, true>), grid, block, 0, s, *a);
    else hipLaunchKernelGGL((m3s::map_write_kernel<0, false>), grid, block, 0, s, *a);
  }
  return hipGetLastError();
}
