// Internal (non-ABI) structs and the launcher shared by rope.hip and abi_rope.cpp. The public C ABI is include/m3s.h.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#define ROPE_TABLE_P 1024  // positions [0, ROPE_TABLE_P) come from the table; every other one takes the fp64 slow path
#define ROPE_BLOCK 256     // lanes per block
#define ROPE_MAX_HPL 4     // heads one lane rotates with the table chunk it loaded once

// One cached table of a (device, base, fwd, Q): a single device allocation, cos then sin then inv.
struct RopeTable {
  const float* cos;   // (ROPE_TABLE_P, Q): float(cos(p inv[t]))
  const float* sin;   // (ROPE_TABLE_P, Q): float(sin(p inv[t]))
  const double* inv;  // (Q): double(fwd) / pow(double(base), double(t) / Q)
};

struct RopeArgs {
  void* tokens;        // (B,N,H,D) of the dtype, element strides stride_b, stride_n, D, 1
  const int64_t* pos;  // (B,N,2) y then x
  int64_t stride_b, stride_n;
  int B, N, H, D, Q;   // Q = D / 4
  int dtype;           // 0 f16, 1 f32, 2 bf16
  int vec;             // 1: 16-byte chunks (abi_rope.cpp checked the alignment conditions), 0: one element per lane
  int HG;              // head groups: a lane rotates heads hg, hg + HG, ... (at most ROPE_MAX_HPL of them)
  int64_t lanes;       // B N HG 2 (Q / chunk elements)
  RopeTable tab;
};

extern "C" {
hipError_t m3s_launch_rope2d(const RopeArgs* a, hipStream_t s);
}
