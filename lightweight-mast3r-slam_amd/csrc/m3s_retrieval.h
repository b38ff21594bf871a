// Internal (non-ABI) tile constants and launchers shared by retrieval.hip and abi_retrieval.cpp. The public C ABI is
// include/m3s.h.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#include "../../include/m3s.h"

#define RQ_NQT 19                 // query column tiles (16 queries) per group
#define RQ_QG (RQ_NQT * 16)       // 304 queries per group
#define RQ_ROWS 256               // codebook rows per block: 8 waves x 32

extern "C" {
hipError_t m3s_launch_rq_prep(const float* X, int R, int D, int S, int ntiles, int inner_n, uint4* frag, int Rp,
                              float pad_value, float* nrm, hipStream_t s);
hipError_t m3s_launch_rq_topk(const uint4* cfrag, const float* cn, const uint4* qfrag, const float* qn, int S, int nblk,
                              int groups, int M, int k, unsigned long long* cand, int64_t* out, hipStream_t s);
}

// ---- ASMK database (asmk.hip, the m3s_asmk_* entries of abi_retrieval.cpp) ----
#define ASMK_MAX_KEYS 4096        // M * k keys of one image: the sort's LDS array and the query word list of the score
#define ASMK_MAX_TOPK M3S_ASMK_MAX_TOPK

extern "C" {
hipError_t m3s_launch_asmk_sort(const int64_t* ids, int M, int k, int use_cols, int C, int32_t* words, int32_t* seg,
                                int32_t* rows, int32_t* count, hipStream_t s);
hipError_t m3s_launch_asmk_aggregate(const float* feat, const float* cent, int D, int slots, const int32_t* words,
                                     const int32_t* seg, const int32_t* rows, const int32_t* count, uint32_t* codes,
                                     hipStream_t s);
hipError_t m3s_launch_asmk_score(const float* tab, const uint32_t* db_codes, const int32_t* db_words,
                                 const int32_t* img_ptr, const int32_t* norm, int D, int n_images,
                                 const uint32_t* q_codes, const int32_t* q_words, const int32_t* q_count, int max_q,
                                 double* scores, hipStream_t s);
hipError_t m3s_launch_asmk_topk(const double* scores, int n, int k, double min_thresh, m3s_asmk_result* res,
                                hipStream_t s);
hipError_t m3s_launch_asmk_append(const uint32_t* codes, const int32_t* words, const int32_t* count, int max_count,
                                  int D, int n, long long max_entries, uint32_t* db_codes, int32_t* db_words,
                                  int32_t* img_ptr, int32_t* norm, hipStream_t s);
}
