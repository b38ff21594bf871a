// Internal (non-ABI) struct and the launcher shared by head.hip and abi_head.cpp. The public C ABI is include/m3s.h.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#define HEAD_BLOCK 256   // lanes per block; layout TOKENS: one block per 16 x 16 patch, lane = pixel in the patch
#define HEAD_PATCH 16    // the ViT's patch edge (pixel_shuffle factor), the only one layout TOKENS takes
#define HEAD_MAX_F 32    // descriptor channels a lane keeps in registers
#define HEAD_F_GROUP 8   // the kernel is instantiated per descriptor width rounded up to a multiple of this

struct HeadArgs {
  const float* a;     // CAT: out (B, 4 + F + tc, H, W); TOKENS: pts (B, 4, H, W)
  const float* feat;  // TOKENS: (B, S, (F + tc) 256), S = (H / 16)(W / 16); CAT: unused
  float *X, *C, *D, *Q;  // (B,Ho,Wo,3), (B,Ho,Wo), (B,Ho,Wo,F), (B,Ho,Wo)
  int layout;         // M3S_HEAD_CAT / M3S_HEAD_TOKENS
  int B, H, W, F, tc, step;
  int Ho, Wo;         // ceil(H / step), ceil(W / step)
  int vec;            // 1: D rows are written in 16-byte stores (F % 4 == 0 and D 16-byte aligned: abi_head.cpp)
  float c_lo, c_span; // conf: C = c_lo + min(exp(l), c_span), c_span = float(vmax - vmin)
  float q_lo, q_span; // desc_conf likewise (read only when tc)
};

extern "C" {
hipError_t m3s_launch_head_post(const HeadArgs* a, hipStream_t s);
}
