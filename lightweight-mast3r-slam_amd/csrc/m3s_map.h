// Internal (non-ABI) structs and launchers shared by map.hip and abi_map.cpp. The public C ABI is include/m3s.h.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#define MAP_TILE 1024                     // pixels per block: 256 lanes x 4, 16 validity words
#define MAP_WORDS (MAP_TILE / 64)         // validity words per block
#define MAP_MAGIC 0x6d33736d61703037ull   // header tag of a completed count

// first bytes of the workspace: written by the scan kernel once the offsets of a count are complete
struct MapHeader {
  uint64_t magic;
  int Kp, N;
  uint32_t thresh_bits;
  int pad;
  int64_t total;
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
};

extern "C" {
hipError_t m3s_launch_map_count(const MapArgs* a, hipStream_t s);
hipError_t m3s_launch_map_write(const MapArgs* a, hipStream_t s);
}
