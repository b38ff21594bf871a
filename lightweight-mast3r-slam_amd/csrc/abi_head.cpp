// C ABI of libm3s.so (include/m3s.h): the dense head tail, from the ViT head's raw output to X, C, D, Q
// (catmlp_dpt_head.py:25-39,82-95, dust3r/heads/postprocess.py:22-55, mast3r_utils.py:69-78). The kernel lives in
// head.hip; this file validates the call and turns the confidence bounds into the kernel's two fp32 constants.
#include "abi_common.h"

#include <cmath>
#include <cstdint>

#include "m3s_head.h"

using namespace m3s_abi;

namespace {

// ('exp', vmin, vmax): any finite vmin, any vmax > vmin (inf included)
bool head_bounds_ok(double vmin, double vmax) { return std::isfinite(vmin) && vmax > vmin; }

}  // namespace

extern "C" int m3s_head_post(int layout, const float* a, const float* feat, int B, int H, int W, int F, int two_confs,
                             int step, double conf_vmin, double conf_vmax, double dconf_vmin, double dconf_vmax,
                             float* X, float* C, float* D, float* Q, void* stream) {
  M3S_CHECK(layout == M3S_HEAD_CAT || layout == M3S_HEAD_TOKENS, "head_post: layout must be 0 (CAT) or 1 (TOKENS)");
  M3S_CHECK(B >= 0 && H >= 0 && W >= 0, "head_post: negative size");
  M3S_CHECK(F >= 1 && F <= HEAD_MAX_F, "head_post: F must be in 1..32");
  M3S_CHECK(step >= 1, "head_post: step must be at least 1");
  M3S_CHECK(layout != M3S_HEAD_TOKENS || (H % HEAD_PATCH == 0 && W % HEAD_PATCH == 0),
            "head_post: layout TOKENS needs H and W to be multiples of 16");
  M3S_CHECK(head_bounds_ok(conf_vmin, conf_vmax), "head_post: conf bounds need a finite vmin and vmax > vmin");
  M3S_CHECK(!two_confs || head_bounds_ok(dconf_vmin, dconf_vmax),
            "head_post: desc_conf bounds need a finite vmin and vmax > vmin");
  const int tc = two_confs ? 1 : 0;
  // the largest input (all channels of CAT; feat and pts of TOKENS are parts of it) and the largest output, D
  if (B == 0 || H == 0 || W == 0) return M3S_OK;
  const int64_t limit = (int64_t)1 << 31, bh = (int64_t)B * H;
  M3S_CHECK(bh < limit && bh * W * (4 + F + tc) < limit, "head_post: every array must hold fewer than 2^31 elements");
  M3S_CHECK(a && X && C && D && Q && (layout == M3S_HEAD_CAT || feat), "head_post: null pointer");
  M3S_CHECK((((uintptr_t)a | (uintptr_t)feat | (uintptr_t)X | (uintptr_t)C | (uintptr_t)D | (uintptr_t)Q) & 3) == 0,
            "head_post: misaligned pointer");

  HeadArgs h{};
  h.a = a, h.feat = feat;
  h.X = X, h.C = C, h.D = D, h.Q = Q;
  h.layout = layout;
  h.B = B, h.H = H, h.W = W, h.F = F, h.tc = tc, h.step = step;
  h.Ho = (int)(((int64_t)H + step - 1) / step), h.Wo = (int)(((int64_t)W + step - 1) / step);
  h.vec = F % 4 == 0 && ((uintptr_t)D & 15) == 0;  // torch: vmin + x.exp().clip(max=vmax - vmin) with Python-float bounds: the difference is taken in double, and both
  // scalars are rounded to fp32 where they meet the fp32 tensor
  h.c_lo = (float)conf_vmin, h.c_span = (float)(conf_vmax - conf_vmin);
  h.q_lo = tc ? (float)dconf_vmin : h.c_lo, h.q_span = tc ? (float)(dconf_vmax - dconf_vmin) : h.c_span;

  hipStream_t s = (hipStream_t)stream;
  {
    Span sp("head_post", s);
    HIP_TRY(m3s_launch_head_post(&h, s), "head_post launch");
  }
  return M3S_OK;
}
