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
// m3s_map_voxel is an optional stage between the two: map_vox_insert_kernel enters every stored row into a hash table
// keyed by its world-frame voxel, where the most confident row wins; map_vox_thin_kernel clears the bits of the
// losers; map_scan_kernel runs again. The write pass then works unchanged on the thinned mask.
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

// The world point of pixel n of a keyframe (points X, pose T): the point itself, or with CALIB the point of its depth on
// its pixel's ray, through actSim3. The one copy of this arithmetic: the write pass emits it, the voxel stage bins it.
template <bool CALIB>
__device__ __forceinline__ void map_world_point(const MapArgs& a, const float* __restrict__ X, const float* T, int n,
                                                float* y) {
  float p[3];
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
    float y[3];
    map_world_point<CALIB>(a, X, T, n, y);
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

// ---- voxel stage (m3s_map_voxel): between the count and the write, thin the stored mask to one row per voxel ----
// The voxel key of a world point: q_c = floorf(y_c * r) per coordinate, biased by 2^20 and packed x << 42 | y << 21 | z
// (below 2^63, so never MAP_VOX_EMPTY). false: y is not finite or a q_c lies outside [-2^20, 2^20) (an overflowed
// or NaN product fails the range test too); the row then reaches no voxel.
__device__ __forceinline__ bool map_voxel_key(const float* y, float r, unsigned long long* key) {
  unsigned long long kk = 0;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float q = floorf(y[c] * r);
    const bool in = isfinite(y[c]) && q >= -MAP_VOX_RANGE && q < MAP_VOX_RANGE;
    kk = (kk << 21) | (unsigned long long)((in ? (int)q : 0) + (1 << 20));
    ok = ok && in;
  }
  *key = kk;
  return ok;
}

__device__ __forceinline__ unsigned long long map_fmix64(unsigned long long h) {  // murmur3's 64-bit finaliser
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}

// Insert: one lane per stored validity bit. The slot of the row's voxel is claimed by a compare-and-swap on its key
// (ours if it returns empty or the key itself), then the row competes by a 64-bit atomic minimum on `best` with
// (~ordered(conf) << 32) | g, ordered() the usual monotone map of the float's bits to unsigned: the minimum is the
// largest confidence and, among equal ones, the smallest g. g < 2^32 - 1 (the ABI checks Kp N < 2^32), so no value
// equals the free slot's all-ones. The table is touched through atomics only. The probe visits every slot at most
// once: a table that is fuller than its contract (at most half) loses rows, it cannot hang or write out of bounds.
template <bool CALIB>
__global__ void __launch_bounds__(256) map_vox_insert_kernel(MapArgs a) {
  const int blk = blockIdx.x;
  if (a.bcnt[blk] == 0) return;
  const int k = blk / a.bpk, b = blk - k * a.bpk;
  const float* __restrict__ X = a.X[k];
  const float* __restrict__ C = a.C[k];
  const float inv = a.scale[k];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float T[8];
#pragma unroll
  for (int c = 0; c < 8; c++) T[c] = a.Twc[(size_t)k * 8 + c];
#pragma unroll
  for (int j = 0; j < MAP_WORDS / 4; j++) {
    const int w = j * 4 + wave;
    const unsigned long long word = a.mask[(size_t)blk * MAP_WORDS + w];
    const int n = b * MAP_TILE + w * 64 + lane;
    unsigned long long key = MAP_VOX_EMPTY, val = MAP_VOX_EMPTY;  // a lane without a row: no real key equals it
    if (((word >> lane) & 1ull) != 0 && n < a.N) {
      float y[3];
      map_world_point<CALIB>(a, X, T, n, y);
      unsigned long long kk;
      if (map_voxel_key(y, a.vox_r, &kk)) {
        const uint32_t g = (uint32_t)((unsigned long long)k * (unsigned long long)a.N + (unsigned long long)n);
        const uint32_t cb = __float_as_uint(C[n] * inv);
        const uint32_t ord = cb ^ ((cb >> 31) ? 0xffffffffu : 0x80000000u);
        key = kk;
        val = ((unsigned long long)(~ord) << 32) | g;
      }
    }
    // Neighbouring pixels often share a voxel: the first lane of a run of equal keys takes the run's minimum (a
    // doubling reduction; the minimum is idempotent, so equal keys met across a gap merge harmlessly and the lane
    // behind the gap still enters its own) and is the only one of the run to touch the table.
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned long long k2 = __shfl_down(key, off, 64);
      const unsigned long long v2 = __shfl_down(val, off, 64);
      if (lane + off < 64 && k2 == key && v2 < val) val = v2;
    }
    const unsigned long long kprev = __shfl_up(key, 1, 64);
    if (key == MAP_VOX_EMPTY || (lane > 0 && kprev == key)) continue;
    unsigned long long h = map_fmix64(key) & a.vox_mask;
    for (unsigned long long i = 0; i <= a.vox_mask; i++) {
      const unsigned long long old = atomicCAS(&a.vtab[h].key, MAP_VOX_EMPTY, key);
      if (old == MAP_VOX_EMPTY || old == key) {
        atomicMin(&a.vtab[h].best, val);
        break;
      }
      h = (h + 1) & a.vox_mask;
    }
  }
}

// Thin: one lane per stored bit. The key is recomputed and probed for with plain loads (the insert launch is
// complete); the bit stays only if the voxel's `best` names this g. A valid row that reaches no voxel (not finite,
// out of range, or not found because X changed under the export or the insert lost it) is cleared and counted in
// *dropped, one atomic per block. Every block rewrites its own validity words and its bcnt; the probe ends at the
// key, at a free slot, or after one lap of the table.
template <bool CALIB>
__global__ void __launch_bounds__(256) map_vox_thin_kernel(MapArgs a) {
  __shared__ int s_cnt[MAP_WORDS], s_drop[MAP_WORDS];
  const int blk = blockIdx.x;
  if (a.bcnt[blk] == 0) return;
  const int k = blk / a.bpk, b = blk - k * a.bpk;
  const float* __restrict__ X = a.X[k];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float T[8];
#pragma unroll
  for (int c = 0; c < 8; c++) T[c] = a.Twc[(size_t)k * 8 + c];
#pragma unroll
  for (int j = 0; j < MAP_WORDS / 4; j++) {
    const int w = j * 4 + wave;
    const unsigned long long word = a.mask[(size_t)blk * MAP_WORDS + w];
    const int n = b * MAP_TILE + w * 64 + lane;
    const bool valid = ((word >> lane) & 1ull) != 0 && n < a.N;
    bool keep = false, found = false;
    if (valid) {
      float y[3];
      map_world_point<CALIB>(a, X, T, n, y);
      unsigned long long key;
      if (map_voxel_key(y, a.vox_r, &key)) {
        const uint32_t g = (uint32_t)((unsigned long long)k * (unsigned long long)a.N + (unsigned long long)n);
        unsigned long long h = map_fmix64(key) & a.vox_mask;
        for (unsigned long long i = 0; i <= a.vox_mask; i++) {
          const ulonglong2 slot = *reinterpret_cast<const ulonglong2*>(&a.vtab[h]);  // key, best: one 16-byte load
          if (slot.x == key) {
            found = true;
            keep = (uint32_t)slot.y == g;
            break;
          }
          if (slot.x == MAP_VOX_EMPTY) break;
          h = (h + 1) & a.vox_mask;
        }
      }
    }
    const unsigned long long kept = __ballot(keep);
    const unsigned long long lost = __ballot(valid && !found);
    if (lane == 0) {
      a.mask[(size_t)blk * MAP_WORDS + w] = kept;
      s_cnt[w] = __popcll(kept);
      s_drop[w] = __popcll(lost);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0, d = 0;
#pragma unroll
    for (int i = 0; i < MAP_WORDS; i++) c += s_cnt[i], d += s_drop[i];
    a.bcnt[blk] = (uint32_t)c;
    if (d) atomicAdd(a.dropped, (unsigned long long)d);
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

// insert, thin, then the count's scan again: it rewrites the offsets, the per-keyframe counts, the total and the header
extern "C" hipError_t m3s_launch_map_voxel(const MapArgs* a, hipStream_t s) {
  const dim3 grid(a->Kp * a->bpk), block(256);
  if (a->calib) {
    hipLaunchKernelGGL((m3s::map_vox_insert_kernel<true>), grid, block, 0, s, *a);
    hipLaunchKernelGGL((m3s::map_vox_thin_kernel<true>), grid, block, 0, s, *a);
  } else {
    hipLaunchKernelGGL((m3s::map_vox_insert_kernel<false>), grid, block, 0, s, *a);
    hipLaunchKernelGGL((m3s::map_vox_thin_kernel<false>), grid, block, 0, s, *a);
  }
  hipLaunchKernelGGL(m3s::map_scan_kernel, dim3(1), dim3(1024), 0, s, *a);
  return hipGetLastError();
}
