// Internal (non-ABI) structs and the launchers shared by ingest.hip and abi_ingest.cpp. The public C ABI is include/m3s.h.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#define INGEST_BLOCK 256         // lanes per block: output columns of ingest_h, dwords of an output row of ingest_v
#define INGEST_PRECISION_BITS 22 // fractional bits of a coefficient
#define INGEST_MAX_LDS 65536     // bytes of dynamic LDS a launch may ask for without opting in

// The horizontal pass: source rows [r0, r0 + nrows) and the crop's Wc columns -> mid, nrows rows of `pitch` bytes per image.
struct IngestHArgs {
  const void* src;      // (B, H1, W1, 3) u8 or f32
  int f32;              // 0: bytes, 1: floats, converted as uint8(x * 255) while staging
  int64_t row_stride;   // bytes
  int64_t img_stride;   // bytes
  int B, r0, nrows, Wc;
  int ident;            // 1: the axis keeps its length: column col is source column x0 + col, copied
  int x0;
  const int32_t* xmin;  // (Wc) first source column of an output column's taps
  const int32_t* n;     // (Wc) its tap count
  const int32_t* k;     // (ksize, Wc) tap-major: neighbouring lanes read neighbouring words
  uint8_t* mid;
  int pitch;            // bytes of a mid row: 3 Wc, a multiple of 4
  unsigned lds_bytes;   // staged source bytes of the widest segment, with room for the dword alignment
};

// The vertical pass and the tail: mid -> img, uimg, rgb_u8 (each nullable).
struct IngestVArgs {
  const uint8_t* mid;
  int pitch, nrows;
  int B, Wc, Hc;
  int ident;            // 1: the axis keeps its length: output row y is mid row y, copied
  const int32_t* ymin;  // (Hc) first mid row of an output row's taps
  const int32_t* n;     // (Hc)
  const int32_t* k;     // (Hc, ksize) row-major: a row's taps are uniform over its lanes
  int ksize;
  int ds, Hd, Wd;       // uimg keeps pixels with y % ds == 0 and x % ds == 0: (B, Hd, Wd, 3)
  float* img;           // (B, 3, Hc, Wc)
  float* uimg;
  uint8_t* rgb;         // (B, Hc, Wc, 3)
};

extern "C" {
hipError_t m3s_launch_ingest_h(const IngestHArgs* a, hipStream_t s);
hipError_t m3s_launch_ingest_v(const IngestVArgs* a, hipStream_t s);
}
