// Internal (non-ABI) structs and launchers shared by map.hip and abi_map.cpp. The public C ABI is include/m3s.h.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#define MAP_TILE 1024                     // pixels per block: 256 lanes x 4, 16 validity words
#define MAP_WORDS (MAP_TILE / 64)         // validity words per block
#define MAP_MAGIC 0x6d33736d61703037ull   // header tag of a completed count
#define MAP_VOX_EMPTY 0xffffffffffffffffull  // voxel table: the key (and the best) of a free slot
#define MAP_VOX_RANGE 1048576.0f             // voxel coordinates lie in [-2^20, 2^20): 21 biased bits each

// first bytes of the workspace: written by the scan kernel once the offsets of a count are complete
struct MapHeader {
  uint64_t magic;
  int Kp, N;
  uint32_t thresh_bits;
  int pad;
  int64_t total;
};

// The header's 256-byte slot of the workspace: the voxel stage keeps its dropped-row counter behind the header.
struct MapHeaderSlot {
  MapHeader h;
  unsigned long long dropped;
};

// One slot of the voxel stage's open-addressing table (m3s_map_voxel): `key` packs the three biased 21-bit voxel
// coordinates (x << 42 | y << 21 | z), `best` is the minimum over the voxel's rows of
// (~ordered(conf) << 32) | g with g = k N + n: the largest confidence, then the smallest global index.
struct alignas(16) MapVoxSlot {
  unsigned long long key, best;
};

struct MapArgs {
  int Kp, N, bpk;           // keyframes, pixels per keyframe, blocks per keyframe (ceil(N / MAP_TILE))
  float thresh;
  int calib, W, layout;
  int64_t capacity;         // rows the caller's output holds
  MapHeader* header;
  uint64_t* mask;           // (Kp * bpk * MAP_WORDS) validity words, bit l of word w = pixel 64 w + l of its keyframe
  uint32_t* bcnt;           // (Kp * bpk) valid pixels per block
  int64_t* boff;            // (Kp * bpk + 1) exclusive scan of bcnt: first output row of each block, then the total
  int64_t* kcnt;            // (Kp + 1) rows per keyframe, then the total
  const float* const* C;    // (Kp) -> (N) confidence sums
  const float* scale;       // (Kp) float32(1 / N_avg)
  const float* const* X;    // (Kp) -> (N,3) points
  const uint8_t* const* rgb;  // (Kp) -> (N,3) colours, or null
  const float* Twc;         // (Kp,8)
  const float* ray_tab;     // calib: x_of_u (W) then y_of_v (H)
  void* out;                // SOA: (M,3) f32; PLY: (M,15) bytes
  uint8_t* out_rgb;         // SOA: (M,3) u8 or null
  // voxel stage only
  float vox_r;              // float32(1) / float32(voxel_size)
  MapVoxSlot* vtab;         // (vox_mask + 1) slots, all bytes 0xff before the insert
  uint64_t vox_mask;        // slots - 1, slots a power of two
  unsigned long long* dropped;  // valid rows that reached no voxel (non-finite, out of range, or not found)
};

extern "C" {
hipError_t m3s_launch_map_count(const MapArgs* a, hipStream_t s);
hipError_t m3s_launch_map_write(const MapArgs* a, hipStream_t s);
hipError_t m3s_launch_map_voxel(const MapArgs* a, hipStream_t s);  // insert, thin, re-scan
}
