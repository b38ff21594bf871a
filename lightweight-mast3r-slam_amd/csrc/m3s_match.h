// Internal (non-ABI) launchers of matching.hip and refine.hip, called from abi_match.cpp (and, for the tile path,
// from matching.hip). The public C ABI is include/m3s.h.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

extern "C" {
// ---- matching.hip ----
hipError_t m3s_launch_prep(const float* X11, float* rays9, const float* D11, void* D11h, int B, int H, int W, int F,
                           int planar, float* cnorm_part, void* D8, hipStream_t s);
int m3s_prep_parts(int B, int H, int W);  // tile partials m3s_launch_prep writes to cnorm_part
hipError_t m3s_launch_iter_proj(const float* rays, const float* pts, const float* p_init, float* p_new, uint8_t* conv,
                                int B, int H, int W, int N, int max_iter, float lambda_init, float cost_thresh,
                                hipStream_t s);
hipError_t m3s_launch_proj_occlusion(const float* rays, const float* X11, const float* X21, const int64_t* idx_init,
                                     int* p1, uint8_t* valid, int B, int H, int W, int max_iter, float lambda_init,
                                     float cost_thresh, float dist_thresh, const float* cnorm_part, int nparts,
                                     float* cmax, int nruns, hipStream_t s);
hipError_t m3s_launch_refine_f16(const void* D11, const void* D21, const int64_t* p1, int64_t* p1_new, int B, int H,
                                 int W, int F, int N, int radius, int dilation_max, hipStream_t s);
hipError_t m3s_launch_refine_f32(const float* D11, const float* D21, const int64_t* p1, int64_t* p1_new, int B, int H,
                                 int W, int F, int N, int radius, int dilation_max, hipStream_t s);
hipError_t m3s_launch_refine_lin(const void* D11h, const float* D21, const int* p1, int64_t* idx_out, int B, int H,
                                 int W, int F, int radius, int dilation_max, const float* cmax, const void* D8,
                                 hipStream_t s);
// ---- refine.hip ----
int m3s_refine_tile_ok(int B, int H, int W, int F, int radius, int dilation_max);
hipError_t m3s_launch_refine_tile(const void* D11h, const void* D21, const void* p1, void* out, int B, int H, int W,
                                  int F, int radius, int dilation_max, int fused, const float* cmax, const void* D8,
                                  hipStream_t s);
hipError_t m3s_launch_refine_tile_proj(const void* D11h, const float* D21, int64_t* idx_out, uint8_t* valid,
                                       const float* rays9, const float* X11, const float* X21, const int64_t* idx_init,
                                       int B, int H, int W, int F, int radius, int dilation_max, int max_iter,
                                       float lambda_init, float cost_thresh, float dist_thresh,
                                       const float* cnorm_part, int nparts, const void* D8, hipStream_t s);
}
