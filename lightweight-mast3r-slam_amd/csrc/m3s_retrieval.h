// Internal (non-ABI) tile constants and launchers shared by retrieval.hip and abi_retrieval.cpp. The public C ABI is
// include/m3s.h.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#define RQ_NQT 19                 // query column tiles (16 queries) per group
#define RQ_QG (RQ_NQT * 16)       // 304 queries per group
#define RQ_ROWS 256               // codebook rows per block: 8 waves x 32

extern "C" {
hipError_t m3s_launch_rq_prep(const float* X, int R, int D, int S, int ntiles, int inner_n, uint4* frag, int Rp,
                              float pad_value, float* nrm, hipStream_t s);
hipError_t m3s_launch_rq_topk(const uint4* cfrag, const float* cn, const uint4* qfrag, const float* qn, int S, int nblk,
                              int groups, int M, int k, unsigned long long* cand, int64_t* out, hipStream_t s);
}
