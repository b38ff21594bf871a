// Frame ingest: from a decoded HWC image to the ViT's input, the reference's create_frame -> resize_img
// (mast3r_slam/frame.py:111-122, mast3r_utils.py:245-289: Pillow resize, centre crop, ImgNorm, the / 255 copy).
//
// Pillow's 8-bit resampler is fixed point: per axis a table of int32 coefficients with 22 fractional bits
// (abi_ingest.cpp fills it in host fp64), and per output byte
//   out = clamp((2^21 + sum_x k[x] pix[xmin + x]) >> 22, 0, 255)   in int32, arithmetic shift.
// The horizontal pass runs first into a uint8 image, the vertical pass reads that image; an axis that keeps its length
// is copied. Both kernels compute exactly that, so the bytes are Pillow's. The tail is fp32 with one rounding per
// operation (this file is built with -ffp-contract=off): img = ((float(u) / 255) - 0.5) / 0.5, uimg = float(u) / 255.
//
// ingest_h: one block per (segment of INGEST_BLOCK crop columns, source row the crop reads, image). The block stages the
//   source bytes its segment's taps span in LDS, aligned dwords from global (floats are converted to bytes on the way,
//   once per element, not per tap), then one lane per output column reads its taps back from LDS. The table is
//   tap-major, so a wave's coefficient loads are contiguous.
// ingest_v: channel-blind, a mid row is a flat run of 3 Wc bytes. One lane takes four consecutive bytes of an output
//   row, one dword load per tap; the row's xmin, n and taps are uniform over the block (scalar loads). The lane then
//   writes its four bytes to rgb_u8 and their floats to the planar img and the interleaved, downsampled uimg.
#include "m3s_common.hpp"
#include "m3s_ingest.h"

namespace m3s {

__device__ __forceinline__ uint32_t ingest_clip8(int acc) {
  const int v = acc >> INGEST_PRECISION_BITS;  // arithmetic
  return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// numpy's uint8(x * 255) on [0, 1]: one fp32 product, truncated; outside that range clamped, NaN to 0
__device__ __forceinline__ uint32_t ingest_f32_to_u8(float x) {
  const float v = x * 255.0f;
  if (!(v > 0.0f)) return 0u;
  if (v >= 255.0f) return 255u;
  return (uint32_t)(int)v;
}

__global__ __launch_bounds__(INGEST_BLOCK) void ingest_h_kernel(const IngestHArgs a) {
  extern __shared__ uint32_t ingest_lds[];
  const int c0 = (int)blockIdx.x * INGEST_BLOCK;
  const int c1 = min(c0 + INGEST_BLOCK, a.Wc);
  const int row = (int)blockIdx.y, b = (int)blockIdx.z;
  // the source columns [s0, s1) this segment's taps read (xmin and xmin + n do not decrease with the column)
  int s0, s1;
  if (a.ident) {
    s0 = a.x0 + c0, s1 = a.x0 + c1;
  } else {
    s0 = a.xmin[c0], s1 = a.xmin[c1 - 1] + a.n[c1 - 1];
  }
  const char* rowp = static_cast<const char*>(a.src) + (int64_t)b * a.img_stride + (int64_t)(a.r0 + row) * a.row_stride;
  const int nb = (s1 - s0) * 3;  // bytes to stage
  int shift = 0;                 // LDS byte offset of source byte 3 s0
  if (a.f32) {
    const float* f = reinterpret_cast<const float*>(rowp) + (int64_t)s0 * 3;
    for (int w = (int)threadIdx.x; w * 4 < nb; w += INGEST_BLOCK) {
      uint32_t pk = 0;
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (w * 4 + j < nb) pk |= ingest_f32_to_u8(f[w * 4 + j]) << (8 * j);
      ingest_lds[w] = pk;
    }
  } else {
    // aligned dwords of [lo, hi); the first and the last one may reach outside the row: those go byte by byte
    const uint8_t* first = reinterpret_cast<const uint8_t*>(rowp) + (int64_t)s0 * 3;
    shift = (int)(reinterpret_cast<uintptr_t>(first) & 3);
    const uint8_t* base = first - shift;  // 4-byte aligned; byte e of the window is source byte e - shift
    const int lo = shift, hi = shift + nb;
    const int nw = (hi + 3) >> 2;
    for (int w = (int)threadIdx.x; w < nw; w += INGEST_BLOCK) {
      const int e = w * 4;
      uint32_t v = 0;
      if (e >= lo && e + 4 <= hi) {
        v = *reinterpret_cast<const uint32_t*>(base + e);
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (e + j >= lo && e + j < hi) v |= (uint32_t)base[e + j] << (8 * j);
      }
      ingest_lds[w] = v;
    }
  }
  __syncthreads();
  const int col = c0 + (int)threadIdx.x;
  if (col >= c1) return;
  const uint8_t* lds = reinterpret_cast<const uint8_t*>(ingest_lds) + shift;
  uint8_t* out = a.mid + ((size_t)b * a.nrows + row) * a.pitch + (size_t)col * 3;
  if (a.ident) {
    const uint8_t* p = lds + (int)threadIdx.x * 3;
    out[0] = p[0], out[1] = p[1], out[2] = p[2];
    return;
  }
  const int xmin = a.xmin[col], n = a.n[col];
  const uint8_t* p = lds + (xmin - s0) * 3;
  const int32_t* k = a.k + col;
  int acc0 = 1 << (INGEST_PRECISION_BITS - 1), acc1 = acc0, acc2 = acc0;
  for (int x = 0; x < n; x++) {
    const int kk = k[(size_t)x * a.Wc];
    acc0 += kk * (int)p[3 * x];
    acc1 += kk * (int)p[3 * x + 1];
    acc2 += kk * (int)p[3 * x + 2];
  }
  out[0] = (uint8_t)ingest_clip8(acc0), out[1] = (uint8_t)ingest_clip8(acc1), out[2] = (uint8_t)ingest_clip8(acc2);
}

__global__ __launch_bounds__(INGEST_BLOCK) void ingest_v_kernel(const IngestVArgs a) {
  const int rowbytes = a.Wc * 3;  // a multiple of 4: every crop width is a multiple of 4 (abi_ingest.cpp checks it)
  const int j0 = ((int)blockIdx.x * INGEST_BLOCK + (int)threadIdx.x) * 4;  // first of the lane's four bytes of the row
  if (j0 >= rowbytes) return;
  const int y = (int)blockIdx.y, b = (int)blockIdx.z;
  const uint8_t* mid = a.mid + (size_t)b * a.nrows * a.pitch + j0;
  uint32_t u[4];
  if (a.ident) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(mid + (size_t)y * a.pitch);
#pragma unroll
    for (int i = 0; i < 4; i++) u[i] = (w >> (8 * i)) & 255u;
  } else {
    const int ymin = a.ymin[y], n = a.n[y];
    const int32_t* k = a.k + (size_t)y * a.ksize;
    int acc[4];
#pragma unroll
    for (int i = 0; i < 4; i++) acc[i] = 1 << (INGEST_PRECISION_BITS - 1);
    for (int x = 0; x < n; x++) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(mid + (size_t)(ymin + x) * a.pitch);
      const int kk = k[x];
#pragma unroll
      for (int i = 0; i < 4; i++) acc[i] += kk * (int)((w >> (8 * i)) & 255u);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) u[i] = ingest_clip8(acc[i]);
  }

  const size_t rowi = (size_t)b * a.Hc + y;
  if (a.rgb) {
    uint8_t* d = a.rgb + rowi * rowbytes + j0;
    if ((reinterpret_cast<uintptr_t>(d) & 3) == 0) {
      *reinterpret_cast<uint32_t*>(d) = u[0] | (u[1] << 8) | (u[2] << 16) | (u[3] << 24);
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++) d[i] = (uint8_t)u[i];
    }
  }
  const bool urow = a.uimg != nullptr && y % a.ds == 0;
  if (!a.img && !urow) return;
  int px = j0 / 3, c = j0 - 3 * px;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float f = (float)u[i] / 255.0f;
    if (a.img) a.img[(((size_t)b * 3 + c) * a.Hc + y) * a.Wc + px] = (f - 0.5f) / 0.5f;
    if (urow && px % a.ds == 0) a.uimg[((((size_t)b * a.Hd + y / a.ds) * a.Wd) + px / a.ds) * 3 + c] = f;
    if (++c == 3) c = 0, px++;
  }
}

}  // namespace m3s

extern "C" hipError_t m3s_launch_ingest_h(const IngestHArgs* a, hipStream_t s) {
  const dim3 grid((unsigned)((a->Wc + INGEST_BLOCK - 1) / INGEST_BLOCK), (unsigned)a->nrows, (unsigned)a->B);
  hipLaunchKernelGGL(m3s::ingest_h_kernel, grid, dim3(INGEST_BLOCK), a->lds_bytes, s, *a);
  return hipGetLastError();
}

extern "C" hipError_t m3s_launch_ingest_v(const IngestVArgs* a, hipStream_t s) {
  const int dwords = (a->Wc * 3 + 3) / 4;
  const dim3 grid((unsigned)((dwords + INGEST_BLOCK - 1) / INGEST_BLOCK), (unsigned)a->Hc, (unsigned)a->B);
  hipLaunchKernelGGL(m3s::ingest_v_kernel, grid, dim3(INGEST_BLOCK), 0, s, *a);
  return hipGetLastError();
}
