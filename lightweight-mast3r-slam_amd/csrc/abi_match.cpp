// C ABI of libm3s.so (include/m3s.h): the reference matching operators and the fused match. Kernels live in
// matching.hip and refine.hip.
#include "abi_common.h"
#include "m3s_match.h"

using namespace m3s_abi;

// ------------------------------------------------------------------------------------------
// reference operators
// ------------------------------------------------------------------------------------------
extern "C" int m3s_iter_proj(const float* rays, const float* pts, const float* p_init, float* p_new,
                             uint8_t* converged, int B, int H, int W, int C, int N, int max_iter, float lambda_init,
                             float cost_thresh, void* stream) {
  M3S_CHECK(B >= 0 && N >= 0 && H >= 3 && W >= 3, "iter_proj: image must be at least 3x3");
  M3S_CHECK(C == 9, "iter_proj: rays_img_with_grad must have 9 channels (ray, gx, gy)");
  M3S_CHECK(max_iter >= 0, "iter_proj: max_iter must be >= 0");
  if (B == 0 || N == 0) return M3S_OK;
  M3S_CHECK(rays && pts && p_init && p_new && converged, "iter_proj: null pointer");
  HIP_TRY(m3s_launch_iter_proj(rays, pts, p_init, p_new, converged, B, H, W, N, max_iter, lambda_init, cost_thresh,
                               (hipStream_t)stream),
          "iter_proj launch");
  return M3S_OK;
}

extern "C" int m3s_refine_matches(int dtype, const void* D11, const void* D21, const int64_t* p1, int64_t* p1_new,
                                  int B, int H, int W, int F, int N, int radius, int dilation_max, void* stream) {
  M3S_CHECK(B >= 0 && N >= 0 && H >= 1 && W >= 1, "refine_matches: bad shape");
  M3S_CHECK(radius >= 0 && dilation_max >= 0, "refine_matches: radius/dilation_max must be >= 0");
  if (B == 0 || N == 0) return M3S_OK;
  M3S_CHECK(D11 && D21 && p1 && p1_new, "refine_matches: null pointer");
  if (dtype == 0) {
    M3S_CHECK(F == 16 || F == 24 || F == 32, "refine_matches: f16 path supports F in {16,24,32}");
    HIP_TRY(m3s_launch_refine_f16(D11, D21, p1, p1_new, B, H, W, F, N, radius, dilation_max, (hipStream_t)stream),
            "refine_matches launch");
  } else if (dtype == 1) {
    M3S_CHECK(F >= 1, "refine_matches: F must be >= 1");
    HIP_TRY(m3s_launch_refine_f32((const float*)D11, (const float*)D21, p1, p1_new, B, H, W, F, N, radius,
                                  dilation_max, (hipStream_t)stream),
            "refine_matches launch");
  } else {
    return fail(M3S_EINVAL, "refine_matches: dtype must be 0 (f16) or 1 (f32)");
  }
  return M3S_OK;
}

// ------------------------------------------------------------------------------------------
// fused match
// ------------------------------------------------------------------------------------------
namespace {
struct MatchWs {
  float* rays9;   // (B,H,W,9) rays + gradients
  void* D11h;     // f16: (B,3,H,W,8) chunk planes on the refine tile path, else (B,H,W,F)
  int* p1;        // (B,N,2) int32
  float* cpart;   // the refine screen's bounds, prep's tile partials: three runs of m3s_prep_parts floats (max
                  // |c|_2; with the int8 copy also max |c_k| and max |c|_1)
  float* cmax;    // ... reduced by the proj launch (refine.hip SCREEN): three floats, one per run
  void* D8;       // int8 screen copy of the descriptors (refine.hip ScreenI8): per image (H,W,16) then
                  // (H,W,8) bytes, 16 bytes of slack behind the last (a row-end DMA lane reads one pixel past it)
};
}  // namespace

static size_t match_carve(Carver& c, int B, int H, int W, int F, MatchWs* w) {
  w->rays9 = c.take<float>((size_t)B * H * W * 9);
  w->D11h = c.take<uint16_t>((size_t)B * H * W * F);
  w->p1 = c.take<int>((size_t)B * H * W * 2);
  w->cpart = c.take<float>((size_t)3 * m3s_prep_parts(B, H, W));
  w->cmax = c.take<float>(3);
  w->D8 = c.take<uint8_t>((size_t)B * H * W * 24 + 16);
  return c.off;
}

extern "C" size_t m3s_match_workspace_size(int B, int H, int W, int F) {
  Carver c(nullptr);
  MatchWs w;
  return match_carve(c, B, H, W, F, &w);
}

extern "C" int m3s_match(const float* X11, const float* X21, const float* D11, const float* D21,
                         const int64_t* idx_init, int64_t* idx_out, uint8_t* valid_out, int B, int H, int W, int F,
                         int max_iter, float lambda_init, float cost_thresh, float dist_thresh, int radius,
                         int dilation_max, void* workspace, size_t workspace_bytes, void* stream) {
  M3S_CHECK(B >= 1 && H >= 3 && W >= 3, "match: image must be at least 3x3");
  M3S_CHECK(F == 16 || F == 24 || F == 32, "match: descriptor dim must be 16, 24 or 32");
  M3S_CHECK(X11 && X21 && D11 && D21 && idx_out && valid_out, "match: null pointer");
  M3S_CHECK(max_iter >= 0 && radius >= 0 && dilation_max >= 0, "match: negative parameter");
  if (workspace_bytes < m3s_match_workspace_size(B, H, W, F)) return fail(M3S_ESPACE, "match: workspace too small");
  Carver c(workspace);
  MatchWs w;
  match_carve(c, B, H, W, F, &w);
  hipStream_t s = (hipStream_t)stream;
  // the refine tile kernel reads prep's chunk-planar D11h (refine.hip); the per-pixel fallback the (H,W,F) one
  const int planar = radius > 0 && m3s_refine_tile_ok(B, H, W, F, radius, dilation_max);
  // bound-screened refine (refine.hip): prep publishes the descriptor-norm bound; M3S_REFINE_SCREEN=0 scores every
  // candidate with the exact chain instead (same results, bit for bit; read per call so tests can compare both)
  const bool screen = env_flag("M3S_REFINE_SCREEN", true) && planar;
  // the screen's levels d >= 2 on an int8 copy of the descriptors (refine.hip ScreenI8; same results,
  // bit for bit). M3S_REFINE_SCREEN8=0 keeps the f16 screen at every level and writes no copy
  const bool screen8 = screen && F == 24 && env_flag("M3S_REFINE_SCREEN8", true);
  void* const D8 = screen8 ? w.D8 : nullptr;
  {
    Span sp("prep_rays", s);
    // the f16 descriptors: the tile path's chunk planes (+ the screen's tile partials) or the (B,H,W,F) layout
    HIP_TRY(m3s_launch_prep(X11, w.rays9, radius > 0 ? D11 : nullptr, w.D11h, B, H, W, F, planar,
                            screen ? w.cpart : nullptr, D8, s),
            "match prep launch");
  }
  // the tile path runs the projection search inside the refine launch (refine.hip FUSE_PROJ: two launches per match,
  // no p1 round trip; same idx / valid bit for bit). M3S_MATCH_FUSE_PROJ=0 (read per call so tests can compare both)
  // restores the proj_occlusion launch
  const bool fuse = planar && env_flag("M3S_MATCH_FUSE_PROJ", true) && (size_t)9 * H * W < ((size_t)1 << 31);
  if (fuse) {
    Span sp("refine_lin", s);
    HIP_TRY(m3s_launch_refine_tile_proj(w.D11h, D21, idx_out, valid_out, w.rays9, X11, X21, idx_init, B, H, W, F, radius,
                                        dilation_max, max_iter, lambda_init, cost_thresh, dist_thresh,
                                        screen ? w.cpart : nullptr, m3s_prep_parts(B, H, W), D8, s),
            "match fused proj + refine launch");
    return M3S_OK;
  }
  {
    Span sp("proj_occlusion", s);
    HIP_TRY(m3s_launch_proj_occlusion(w.rays9, X11, X21, idx_init, w.p1, valid_out, B, H, W, max_iter, lambda_init,
                                      cost_thresh, dist_thresh, w.cpart, m3s_prep_parts(B, H, W),
                                      screen ? w.cmax : nullptr, screen8 ? 3 : 1, s),
            "match proj launch");
  }
  // radius == 0: the refine loop is empty and the kernel only writes idx = pixel_to_lin(p1)
  // (matching.py:78-88); D11h is never read then.
  {
    Span sp("refine_lin", s);
    HIP_TRY(m3s_launch_refine_lin(w.D11h, D21, w.p1, idx_out, B, H, W, F, radius, radius > 0 ? dilation_max : 0,
                                  screen ? w.cmax : nullptr, D8, s),
            "match refine launch");
  }
  return M3S_OK;
}
