// C ABI of libm3s.so (include/m3s.h): the frame ingest, the reference's create_frame -> resize_img (frame.py:111-122,
// mast3r_utils.py:245-289). The kernels live in ingest.hip; this file owns the geometry, the coefficient tables of
// Pillow's fixed-point resampler (host fp64, one statement for the device tables and m3s_ingest_table) and their
// per-device cache.
#include "abi_common.h"

#include <cmath>
#include <cstdint>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "m3s_ingest.h"

// the filters' and the weights' fp64 products and sums as written: no contraction
#pragma clang fp contract(off)

using namespace m3s_abi;

namespace {

const int INGEST_MAX_SIDE = 16384;

double ingest_sinc(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return std::sin(x) / x;
}

double ingest_filter(int filter, double x) {
  if (filter == M3S_INGEST_LANCZOS) {
    if (-3.0 <= x && x < 3.0) return ingest_sinc(x) * ingest_sinc(x / 3);
    return 0.0;
  }
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

struct IngestAxis {
  double scale, fs, support;
  int ksize;
};

IngestAxis ingest_axis(int in, int out, int filter) {
  IngestAxis ax;
  ax.scale = (double)in / (double)out;
  ax.fs = ax.scale < 1.0 ? 1.0 : ax.scale;
  ax.support = (filter == M3S_INGEST_LANCZOS ? 3.0 : 2.0) * ax.fs;
  ax.ksize = (int)std::ceil(ax.support) * 2 + 1;
  return ax;
}

// the taps [xmin, xmin + n) of output xx; returns its center
double ingest_bounds(const IngestAxis& ax, int in, int xx, int* xmin, int* n) {
  const double center = (xx + 0.5) * ax.scale;
  int lo = (int)(center - ax.support + 0.5);
  if (lo < 0) lo = 0;
  int hi = (int)(center + ax.support + 0.5);
  if (hi > in) hi = in;
  *xmin = lo, *n = hi - lo;
  return center;
}

// The table's one statement: outputs [o0, o1) of the axis in -> out. xmin and n take o1 - o0 entries; k takes ksize
// of them per output, zero behind its n taps: tap x of output xx at k[(xx - o0) ksize + x], or tap-major at
// k[x (o1 - o0) + (xx - o0)]. Both the device tables (ingest_plan) and m3s_ingest_table come from here.
void ingest_fill(int in, int out, int filter, int o0, int o1, int32_t* xmin, int32_t* n, int32_t* k, int ksize,
                 bool tap_major) {
  const IngestAxis ax = ingest_axis(in, out, filter);
  const double ss = 1.0 / ax.fs;
  const int cnt = o1 - o0;
  std::vector<double> w((size_t)ax.ksize);
  for (int xx = o0; xx < o1; xx++) {
    int lo, m;
    const double center = ingest_bounds(ax, in, xx, &lo, &m);
    double ww = 0.0;
    for (int x = 0; x < m; x++) {
      w[x] = ingest_filter(filter, (x + lo - center + 0.5) * ss);
      ww += w[x];
    }
    const int i = xx - o0;
    xmin[i] = lo, n[i] = m;
    for (int x = 0; x < ksize; x++) {
      int32_t q = 0;
      if (x < m) {
        double v = w[x];
        if (ww != 0.0) v /= ww;
        q = v < 0 ? (int32_t)(-0.5 + v * (double)(1 << INGEST_PRECISION_BITS))
                  : (int32_t)(0.5 + v * (double)(1 << INGEST_PRECISION_BITS));
      }
      k[tap_major ? (size_t)x * cnt + i : (size_t)i * ksize + x] = q;
    }
  }
}

// nullptr when the geometry is fine, else what is wrong with it
const char* ingest_geometry(int H1, int W1, int size, int square_ok, m3s_ingest_geom* g) {
  if (size != 512 && size != 224) return "ingest: size must be 512 or 224";
  if (H1 < 1 || W1 < 1 || H1 > INGEST_MAX_SIDE || W1 > INGEST_MAX_SIDE) return "ingest: H1 and W1 must be in 1..16384";
  const int S = W1 > H1 ? W1 : H1;
  int64_t L = 512;
  if (size == 224) {
    const double r1 = (double)W1 / (double)H1, r2 = (double)H1 / (double)W1;
    L = (int64_t)std::nearbyint((double)size * (r1 > r2 ? r1 : r2));
  }
  const int64_t Wr = (int64_t)std::nearbyint((double)((int64_t)W1 * L) / (double)S);
  const int64_t Hr = (int64_t)std::nearbyint((double)((int64_t)H1 * L) / (double)S);
  const int64_t cx = Wr / 2, cy = Hr / 2;
  int64_t halfw, halfh;
  if (size == 224) {
    halfw = halfh = cx < cy ? cx : cy;
  } else {
    halfw = ((2 * cx) / 16) * 8, halfh = ((2 * cy) / 16) * 8;
    if (!square_ok && Wr == Hr) halfh = 3 * halfw / 4;  // halfw is a multiple of 8: exact
  }
  if (halfw <= 0 || halfh <= 0) return "ingest: the crop is empty";
  g->resized_w = (int)Wr, g->resized_h = (int)Hr;
  g->filter = S > L ? M3S_INGEST_LANCZOS : M3S_INGEST_BICUBIC;
  g->crop_x0 = (int)(cx - halfw), g->crop_y0 = (int)(cy - halfh);
  g->crop_x1 = (int)(cx + halfw), g->crop_y1 = (int)(cy + halfh);
  g->out_w = (int)(2 * halfw), g->out_h = (int)(2 * halfh);
  g->scale_w = (double)W1 / (double)Wr, g->scale_h = (double)H1 / (double)Hr;
  g->half_crop_w = (double)(Wr - g->out_w) / 2, g->half_crop_h = (double)(Hr - g->out_h) / 2;
  return nullptr;
}

// What a geometry fixes of the two launches, without the tables: which source rows the horizontal pass computes, the
// mid image's row pitch and the LDS its widest segment stages.
struct IngestShape {
  m3s_ingest_geom g;
  int ident_h, ident_v;
  int r0, nrows;  // source rows [r0, r0 + nrows) feed the crop's rows
  int pitch;
  int ksize_h, ksize_v;
  unsigned lds_bytes;
};

const char* ingest_shape(int H1, int W1, int size, int square_ok, IngestShape* sh) {
  const char* bad = ingest_geometry(H1, W1, size, square_ok, &sh->g);
  if (bad) return bad;
  const m3s_ingest_geom& g = sh->g;
  sh->ident_h = g.resized_w == W1, sh->ident_v = g.resized_h == H1;
  // ingest_v gives a lane four whole bytes of an output row. Every crop width is a multiple of 4 (size 512: of 16;
  // size 224: the short side resizes to 224, so the crop is 224 wide); a geometry that broke this is refused here.
  if (g.out_w % 4 != 0) return "ingest: the crop's width is not a multiple of 4";
  sh->pitch = g.out_w * 3;
  sh->ksize_h = sh->ksize_v = 0;
  if (sh->ident_v) {
    sh->r0 = g.crop_y0, sh->nrows = g.out_h;
  } else {
    const IngestAxis ax = ingest_axis(H1, g.resized_h, g.filter);
    int lo, m, lo2, m2;
    ingest_bounds(ax, H1, g.crop_y0, &lo, &m);
    ingest_bounds(ax, H1, g.crop_y1 - 1, &lo2, &m2);
    sh->r0 = lo, sh->nrows = lo2 + m2 - lo;
    sh->ksize_v = ax.ksize;
  }
  int span = 0;  // source columns of the widest segment
  for (int c0 = 0; c0 < g.out_w; c0 += INGEST_BLOCK) {
    const int c1 = c0 + INGEST_BLOCK < g.out_w ? c0 + INGEST_BLOCK : g.out_w;
    int s = c1 - c0;
    if (!sh->ident_h) {
      const IngestAxis ax = ingest_axis(W1, g.resized_w, g.filter);
      int lo, m, lo2, m2;
      ingest_bounds(ax, W1, g.crop_x0 + c0, &lo, &m);
      ingest_bounds(ax, W1, g.crop_x0 + c1 - 1, &lo2, &m2);
      s = lo2 + m2 - lo;
      sh->ksize_h = ax.ksize;
    }
    if (s > span) span = s;
  }
  sh->lds_bytes = (unsigned)((span * 3 + 8 + 3) & ~3);  // up to 3 bytes in front for the dword alignment, 3 behind
  if (sh->lds_bytes > INGEST_MAX_LDS) return "ingest: a segment's source span does not fit the LDS";
  return nullptr;
}

// (device, H1, W1, size, square_ok) -> the device tables; entries live until m3s_ingest_release on their device
typedef std::tuple<int, int, int, int, int> IngestKey;
struct IngestPlan {
  IngestShape sh;
  void* buf = nullptr;  // xmin_h | n_h | k_h | ymin_v | n_v | k_v, int32 each
  const int32_t *xmin_h = nullptr, *n_h = nullptr, *k_h = nullptr, *ymin_v = nullptr, *n_v = nullptr, *k_v = nullptr;
};
std::mutex g_ingest_mu;
std::map<IngestKey, IngestPlan> g_ingest_plans;

// The plan of a geometry (`sh` its shape, which the caller has computed) on the current device; built and uploaded synchronously on first use (not legal inside a
// stream capture: m3s_ingest_prepare beforehand).
int ingest_plan(int H1, int W1, int size, int square_ok, const IngestShape& sh, hipStream_t s, IngestPlan* out) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev), "ingest device query");
  const IngestKey key(dev, H1, W1, size, square_ok ? 1 : 0);
  std::lock_guard<std::mutex> lock(g_ingest_mu);
  auto it = g_ingest_plans.find(key);
  if (it != g_ingest_plans.end()) {
    *out = it->second;
    return M3S_OK;
  }
  const m3s_ingest_geom& g = sh.g;
  const size_t nh = sh.ident_h ? 0 : (size_t)g.out_w, nv = sh.ident_v ? 0 : (size_t)g.out_h;
  // one host image of the allocation
  std::vector<int32_t> host(2 * nh + nh * sh.ksize_h + 2 * nv + nv * sh.ksize_v + 1);
  int32_t* xmin_h = host.data();
  int32_t* n_h = xmin_h + nh;
  int32_t* k_h = n_h + nh;
  int32_t* ymin_v = k_h + nh * sh.ksize_h;
  int32_t* n_v = ymin_v + nv;
  int32_t* k_v = n_v + nv;
  if (nh) ingest_fill(W1, g.resized_w, g.filter, g.crop_x0, g.crop_x1, xmin_h, n_h, k_h, sh.ksize_h, true);
  if (nv) {
    ingest_fill(H1, g.resized_h, g.filter, g.crop_y0, g.crop_y1, ymin_v, n_v, k_v, sh.ksize_v, false);
    for (size_t y = 0; y < nv; y++) ymin_v[y] -= sh.r0;  // rows of the mid image
  }
  IngestPlan p;
  p.sh = sh;
  const size_t bytes = host.size() * sizeof(int32_t);
  HIP_TRY(hipMalloc(&p.buf, bytes), "ingest table alloc");
  hipError_t err = hipMemcpyAsync(p.buf, host.data(), bytes, hipMemcpyHostToDevice, s);
  if (err == hipSuccess) err = hipStreamSynchronize(s);  // the pageable host image dies with this call
  if (err != hipSuccess) {
    (void)hipFree(p.buf);
    return hip_fail(err, "ingest table upload");
  }
  const int32_t* d = static_cast<const int32_t*>(p.buf);
  p.xmin_h = d, p.n_h = d + nh, p.k_h = d + 2 * nh;
  p.ymin_v = p.k_h + nh * sh.ksize_h, p.n_v = p.ymin_v + nv, p.k_v = p.n_v + nv;
  g_ingest_plans[key] = p;
  *out = p;
  return M3S_OK;
}

size_t ingest_workspace(const IngestShape& sh, int B) { return align256((size_t)B * sh.nrows * sh.pitch); }

}  // namespace

extern "C" int m3s_ingest_geometry(int H1, int W1, int size, int square_ok, m3s_ingest_geom* out) {
  M3S_CHECK(out != nullptr, "ingest: null geometry output");
  m3s_ingest_geom g{};
  const char* bad = ingest_geometry(H1, W1, size, square_ok, &g);
  if (bad) return fail(M3S_EINVAL, bad);
  *out = g;
  return M3S_OK;
}

extern "C" int m3s_ingest_table(int in, int out, int filter, int32_t* xmin, int32_t* n, int32_t* k, int ksize) {
  M3S_CHECK(filter == M3S_INGEST_BICUBIC || filter == M3S_INGEST_LANCZOS, "ingest: filter must be 0 (bicubic) or 1 (lanczos)");
  M3S_CHECK(in >= 1 && out >= 1 && in <= (1 << 24) && out <= (1 << 24), "ingest: table lengths must be in 1..2^24");
  M3S_CHECK(xmin && n && k, "ingest: null table output");
  M3S_CHECK(ksize >= ingest_axis(in, out, filter).ksize, "ingest: ksize below 2 ceil(support) + 1");
  M3S_CHECK((int64_t)out * ksize <= ((int64_t)1 << 30), "ingest: table too large");
  ingest_fill(in, out, filter, 0, out, xmin, n, k, ksize, false);
  return M3S_OK;
}

extern "C" int m3s_ingest_prepare(int H1, int W1, int size, int square_ok, void* stream) {
  IngestShape sh;
  const char* bad = ingest_shape(H1, W1, size, square_ok, &sh);
  if (bad) return fail(M3S_EINVAL, bad);
  IngestPlan p;
  return ingest_plan(H1, W1, size, square_ok, sh, (hipStream_t)stream, &p);
}

extern "C" int m3s_ingest_release(void) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev), "ingest device query");
  std::lock_guard<std::mutex> lock(g_ingest_mu);
  hipError_t err = hipSuccess;
  for (auto it = g_ingest_plans.begin(); it != g_ingest_plans.end();) {
    if (std::get<0>(it->first) == dev) {
      const hipError_t e = hipFree(it->second.buf);  // waits for the device's launches that read it
      if (err == hipSuccess) err = e;
      it = g_ingest_plans.erase(it);
    } else {
      ++it;
    }
  }
  if (err != hipSuccess) return hip_fail(err, "ingest table free");
  return M3S_OK;
}

extern "C" size_t m3s_ingest_workspace_size(int H1, int W1, int size, int square_ok, int B) {
  IngestShape sh;
  if (B < 0 || B > 65535 || ingest_shape(H1, W1, size, square_ok, &sh) != nullptr) return 0;
  return ingest_workspace(sh, B > 0 ? B : 1);
}

extern "C" int m3s_ingest(const m3s_ingest_args* args, void* workspace, size_t workspace_bytes, void* stream) {
  M3S_CHECK(args != nullptr, "ingest: null args");
  const m3s_ingest_args& in = *args;
  M3S_CHECK(in.src_dtype == M3S_INGEST_U8 || in.src_dtype == M3S_INGEST_F32, "ingest: src_dtype must be 0 (u8) or 1 (f32)");
  M3S_CHECK(in.B >= 0 && in.B <= 65535, "ingest: B must be in 0..65535");
  M3S_CHECK(in.downsample >= 1, "ingest: downsample must be at least 1");
  IngestShape sh;
  const char* bad = ingest_shape(in.H1, in.W1, in.size, in.square_ok, &sh);
  if (bad) return fail(M3S_EINVAL, bad);
  const int64_t elem = in.src_dtype == M3S_INGEST_F32 ? 4 : 1;
  M3S_CHECK(in.row_stride >= (int64_t)in.W1 * 3 * elem, "ingest: row_stride below a row's bytes");
  if (in.B == 0) return M3S_OK;
  M3S_CHECK(in.src != nullptr, "ingest: null source");
  if (in.src_dtype == M3S_INGEST_F32)
    M3S_CHECK(((uintptr_t)in.src & 3) == 0 && (in.row_stride & 3) == 0, "ingest: misaligned float source");
  M3S_CHECK(((uintptr_t)in.img & 3) == 0 && ((uintptr_t)in.uimg & 3) == 0, "ingest: misaligned float output");
  M3S_CHECK(workspace != nullptr && ((uintptr_t)workspace & 3) == 0, "ingest: null or misaligned workspace");
  if (workspace_bytes < ingest_workspace(sh, in.B)) return fail(M3S_ESPACE, "ingest: workspace too small");

  hipStream_t s = (hipStream_t)stream;
  IngestPlan p;
  const int rc = ingest_plan(in.H1, in.W1, in.size, in.square_ok, sh, s, &p);
  if (rc != M3S_OK) return rc;
  const m3s_ingest_geom& g = sh.g;

  IngestHArgs h{};
  h.src = in.src, h.f32 = in.src_dtype == M3S_INGEST_F32;
  h.row_stride = in.row_stride, h.img_stride = in.row_stride * in.H1;
  h.B = in.B, h.r0 = sh.r0, h.nrows = sh.nrows, h.Wc = g.out_w;
  h.ident = sh.ident_h, h.x0 = g.crop_x0;
  h.xmin = p.xmin_h, h.n = p.n_h, h.k = p.k_h;
  h.mid = static_cast<uint8_t*>(workspace), h.pitch = sh.pitch, h.lds_bytes = sh.lds_bytes;

  IngestVArgs v{};
  v.mid = h.mid, v.pitch = sh.pitch, v.nrows = sh.nrows;
  v.B = in.B, v.Wc = g.out_w, v.Hc = g.out_h;
  v.ident = sh.ident_v;
  v.ymin = p.ymin_v, v.n = p.n_v, v.k = p.k_v, v.ksize = sh.ksize_v;
  v.ds = in.downsample, v.Hd = (g.out_h + v.ds - 1) / v.ds, v.Wd = (g.out_w + v.ds - 1) / v.ds;
  v.img = in.img, v.uimg = in.uimg, v.rgb = in.rgb_u8;
  {
    Span sp("ingest", s);
    HIP_TRY(m3s_launch_ingest_h(&h, s), "ingest_h launch");
    HIP_TRY(m3s_launch_ingest_v(&v, s), "ingest_v launch");
  }
  return M3S_OK;
}
