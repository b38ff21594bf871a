// ASMK retrieval database on the device (include/m3s.h, the m3s_asmk_* section): what the reference's
// RetrievalDatabase.update does around quantize_custom on the host (asmk/kernel.py aggregate_image, asmk/inverted_file.py
// IVF.search / IVF.add, cython/hamming.pyx, asmk/functional.py asmk_kernel; binary kernel, no idf).
//
// The database is a forward file: entries (code, word) in insertion order and img_ptr (n + 1) entry offsets, because
// every image adds its entries in one piece. An image's score is a sum over its own segment: one workgroup per image,
// no atomics, a fixed reduction order. It visits the same (query word, entry) pairs as the inverted file.
//
// Built with -ffp-contract=off: a bit of a code is the sign of a fp32 sum, so the residual des - centroid is rounded
// before it is added, and the rows are added in ascending row order like numpy's sum over the outer axis.
#include "m3s_common.hpp"
#include "m3s_retrieval.h"

namespace m3s {

// ---- sort / unique: one workgroup. Keys (word << 12 | row) sorted in LDS (bitonic), then one scan that drops a
// repeated (word, row) key and numbers the words. Writes words (nq), seg (nq + 1) offsets into rows, rows, *count.
__global__ void __launch_bounds__(1024) asmk_sort_kernel(const int64_t* __restrict__ ids, int M, int k, int use_cols,
                                                         int C, int P, int32_t* __restrict__ words,
                                                         int32_t* __restrict__ seg, int32_t* __restrict__ rows,
                                                         int32_t* __restrict__ count) {
  __shared__ uint32_t s_key[ASMK_MAX_KEYS];
  __shared__ int s_wave[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = M * use_cols;
  for (int i = tid; i < P; i += 1024) {
    uint32_t key = 0xffffffffu;  // padding sorts last; a real key of that value is equal to it, so order is unaffected
    if (i < n) {
      const int row = i / use_cols, col = i - row * use_cols;
      long long w = ids[(size_t)row * k + col];
      w = w < 0 ? 0 : (w >= C ? C - 1 : w);  // ids come from the quantiser (0 .. C-1); never index outside the codebook
      key = ((uint32_t)w << 12) | (uint32_t)row;
    }
    s_key[i] = key;
  }
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1)
    for (int j = size >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += 1024) {
        const int i = 2 * t - (t & (j - 1)), l = i + j;
        const uint32_t a = s_key[i], b = s_key[l];
        const bool up = (i & size) == 0;
        if ((a > b) == up) {
          s_key[i] = b;
          s_key[l] = a;
        }
      }
      __syncthreads();
    }
  // four consecutive positions per thread; keep = not a repeat of the previous key, ws = first key of its word
  int keep[4], ws[4], local = 0;
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int i = 4 * tid + u;
    keep[u] = ws[u] = 0;
    if (i < n) {
      const uint32_t key = s_key[i];
      const bool first = i == 0;
      const uint32_t prev = first ? 0u : s_key[i - 1];
      keep[u] = first || key != prev;
      ws[u] = first || (key >> 12) != (prev >> 12);
      local += keep[u] + (ws[u] << 16);
    }
  }
  int v = local;  // inclusive wave scan of the packed (ws << 16 | keep) counts: both stay below 2^13
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  if (lane == 63) s_wave[wave] = v;
  __syncthreads();
  int base = 0, total = 0;
  for (int w = 0; w < 16; w++) {
    if (w < wave) base += s_wave[w];
    total += s_wave[w];
  }
  int run = base + v - local;  // exclusive
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int i = 4 * tid + u;
    if (i < n) {
      const uint32_t key = s_key[i];
      const int r = run & 0xffff, slot = run >> 16;
      if (ws[u]) {
        words[slot] = (int32_t)(key >> 12);
        seg[slot] = r;
      }
      if (keep[u]) rows[r] = (int32_t)(key & 0xfffu);
      run += keep[u] + (ws[u] << 16);
    }
  }
  if (tid == 0) {
    const int nq = total >> 16;
    seg[nq] = total & 0xffff;
    *count = nq;
  }
}

// ---- aggregate + binarise: one workgroup per unique-word slot (grid = the host's bound M * use_cols; slots >= *count
// exit). Lanes own consecutive dims; a wave's ballot holds 64 consecutive dims = two code words, bit-reversed into
// hamming.pyx's MSB-first order (dim d -> word d / 32, bit 31 - d % 32).
__global__ void __launch_bounds__(256) asmk_aggregate_kernel(const float* __restrict__ feat,
                                                             const float* __restrict__ cent, int D,
                                                             const int32_t* __restrict__ words,
                                                             const int32_t* __restrict__ seg,
                                                             const int32_t* __restrict__ rows,
                                                             const int32_t* __restrict__ count,
                                                             uint32_t* __restrict__ codes) {
  const int slot = blockIdx.x;
  if (slot >= *count) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int W = D >> 5;
  const float* c = cent + (size_t)words[slot] * D;
  const int r0 = seg[slot], r1 = seg[slot + 1];
  for (int base = 0; base < D; base += 256) {
    const int d = base + tid;
    float acc = 0.0f;
    if (d < D) {
      const float cd = c[d];
      for (int r = r0; r < r1; r++) acc += feat[(size_t)rows[r] * D + d] - cd;
    }
    const unsigned long long mask = __ballot(d < D && acc > 0.0f);
    if (lane == 0) {
      const int w = d >> 5;
      if (w < W) codes[(size_t)slot * W + w] = __brev((uint32_t)mask);
      if (w + 1 < W) codes[(size_t)slot * W + w + 1] = __brev((uint32_t)(mask >> 32));
    }
  }
}

// ---- score: one workgroup per database image. The query's sorted unique words sit in LDS; every entry of the image
// finds its word there by binary search, h = popcount(q ^ e) indexes the (D + 1)-entry table of powf(sim, alpha)
// (0 where sim < similarity_threshold), the term is rounded to fp32 after the fp64 division by sqrt(norm)
// (inverted_file.py:103, an in-place f32 /= f64) and summed in fp64: per thread in entry order, then a fixed tree.
__global__ void __launch_bounds__(256) asmk_score_kernel(const float* __restrict__ tab,
                                                         const uint32_t* __restrict__ db_codes,
                                                         const int32_t* __restrict__ db_words,
                                                         const int32_t* __restrict__ img_ptr,
                                                         const int32_t* __restrict__ norm, int D,
                                                         const uint32_t* __restrict__ q_codes,
                                                         const int32_t* __restrict__ q_words,
                                                         const int32_t* __restrict__ q_count, int max_q,
                                                         double* __restrict__ scores) {
  __shared__ int32_t s_word[ASMK_MAX_KEYS];
  __shared__ double s_red[256];
  const int tid = threadIdx.x, img = blockIdx.x;
  const int W = D >> 5;
  int nq = *q_count;
  nq = nq < 0 ? 0 : (nq > max_q ? max_q : nq);
  for (int i = tid; i < nq; i += 256) s_word[i] = q_words[i];
  __syncthreads();
  const int e0 = img_ptr[img], e1 = img_ptr[img + 1];
  const double sqn = sqrt((double)norm[img]);
  double acc = 0.0;
  for (int e = e0 + tid; e < e1; e += 256) {
    const int32_t w = db_words[e];
    int lo = 0, hi = nq;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_word[mid] < w) lo = mid + 1;
      else hi = mid;
    }
    if (lo < nq && s_word[lo] == w) {
      const uint32_t* q = q_codes + (size_t)lo * W;
      const uint32_t* x = db_codes + (size_t)e * W;
      int h = 0;
      if ((W & 3) == 0) {
        for (int j = 0; j < W; j += 4) {
          const uint4 a = *reinterpret_cast<const uint4*>(q + j), b = *reinterpret_cast<const uint4*>(x + j);
          h += __popc(a.x ^ b.x) + __popc(a.y ^ b.y) + __popc(a.z ^ b.z) + __popc(a.w ^ b.w);
        }
      } else {
        for (int j = 0; j < W; j++) h += __popc(q[j] ^ x[j]);
      }
      const float term = (float)((double)tab[h] / sqn);
      acc += (double)term;
    }
  }
  s_red[tid] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) s_red[tid] += s_red[tid + s];
    __syncthreads();
  }
  // the reference's q_norm_factor is a float32 count and np.sqrt of it a float32 (inverted_file.py:94,106)
  if (tid == 0) scores[img] = s_red[0] / (double)sqrtf((float)nq);
}

// ---- top-k: one workgroup, rank by counting. Descending score, ties -> lower index, NaN first like torch.topk;
// then the `> min_thresh` filter of retrieval_database.py:65-66.
__device__ __forceinline__ bool asmk_before(double a, int ia, double b, int ib) {  // a ranks before b
  const bool na = a != a, nb = b != b;
  if (na || nb) return (na && !nb) || (na && nb && ia < ib);
  return a > b || (a == b && ia < ib);
}

__global__ void __launch_bounds__(256) asmk_topk_kernel(const double* __restrict__ scores, int n, int k,
                                                        double min_thresh, m3s_asmk_result* __restrict__ res) {
  __shared__ int s_idx[ASMK_MAX_TOPK];
  __shared__ double s_val[ASMK_MAX_TOPK];
  const int tid = threadIdx.x;
  const int kk = k < n ? k : n;
  for (int i = tid; i < n; i += 256) {
    const double si = scores[i];
    int rank = 0;
    for (int j = 0; j < n; j++) rank += (j != i && asmk_before(scores[j], j, si, i)) ? 1 : 0;
    if (rank < kk) {
      s_idx[rank] = i;
      s_val[rank] = si;
    }
  }
  __syncthreads();
  if (tid == 0) {
    int cnt = 0;
    for (int r = 0; r < kk; r++)
      if (s_val[r] > min_thresh) {
        res->idx[cnt] = s_idx[r];
        res->score[cnt] = s_val[r];
        cnt++;
      }
    res->count = cnt;
  }
}

// ---- append: the aggregate's entries go to img_ptr[n]; img_ptr[n + 1] and norm[n] are written here, so the host
// never reads a count (it checks capacity with the bound max_count). Entries past max_entries are never written.
__global__ void __launch_bounds__(256) asmk_append_kernel(const uint32_t* __restrict__ codes,
                                                          const int32_t* __restrict__ words,
                                                          const int32_t* __restrict__ count, int max_count, int D,
                                                          int n, long long max_entries,
                                                          uint32_t* __restrict__ db_codes,
                                                          int32_t* __restrict__ db_words, int32_t* __restrict__ img_ptr,
                                                          int32_t* __restrict__ norm) {
  const int W = D >> 5;
  const int base = img_ptr[n];
  int nb = *count;
  nb = nb < 0 ? 0 : (nb > max_count ? max_count : nb);
  if ((long long)base + nb > max_entries) nb = max_entries > base ? (int)(max_entries - base) : 0;
  const int t = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
  for (int i = t; i < nb * W; i += stride) db_codes[(size_t)base * W + i] = codes[i];
  for (int i = t; i < nb; i += stride) db_words[base + i] = words[i];
  if (t == 0) {
    img_ptr[n + 1] = base + nb;
    norm[n] = nb;
  }
}

}  // namespace m3s

extern "C" hipError_t m3s_launch_asmk_sort(const int64_t* ids, int M, int k, int use_cols, int C, int32_t* words,
                                           int32_t* seg, int32_t* rows, int32_t* count, hipStream_t s) {
  int P = 64;
  while (P < M * use_cols) P <<= 1;
  hipLaunchKernelGGL(m3s::asmk_sort_kernel, dim3(1), dim3(1024), 0, s, ids, M, k, use_cols, C, P, words, seg, rows,
                     count);
  return hipGetLastError();
}

extern "C" hipError_t m3s_launch_asmk_aggregate(const float* feat, const float* cent, int D, int slots,
                                                const int32_t* words, const int32_t* seg, const int32_t* rows,
                                                const int32_t* count, uint32_t* codes, hipStream_t s) {
  hipLaunchKernelGGL(m3s::asmk_aggregate_kernel, dim3(slots), dim3(256), 0, s, feat, cent, D, words, seg, rows, count,
                     codes);
  return hipGetLastError();
}

extern "C" hipError_t m3s_launch_asmk_score(const float* tab, const uint32_t* db_codes, const int32_t* db_words,
                                            const int32_t* img_ptr, const int32_t* norm, int D, int n_images,
                                            const uint32_t* q_codes, const int32_t* q_words, const int32_t* q_count,
                                            int max_q, double* scores, hipStream_t s) {
  hipLaunchKernelGGL(m3s::asmk_score_kernel, dim3(n_images), dim3(256), 0, s, tab, db_codes, db_words, img_ptr, norm, D,
                     q_codes, q_words, q_count, max_q, scores);
  return hipGetLastError();
}

extern "C" hipError_t m3s_launch_asmk_topk(const double* scores, int n, int k, double min_thresh,
                                           m3s_asmk_result* res, hipStream_t s) {
  hipLaunchKernelGGL(m3s::asmk_topk_kernel, dim3(1), dim3(256), 0, s, scores, n, k, min_thresh, res);
  return hipGetLastError();
}

extern "C" hipError_t m3s_launch_asmk_append(const uint32_t* codes, const int32_t* words, const int32_t* count,
                                             int max_count, int D, int n, long long max_entries, uint32_t* db_codes,
                                             int32_t* db_words, int32_t* img_ptr, int32_t* norm, hipStream_t s) {
  int blocks = (max_count * (D >> 5) + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 256 ? 256 : blocks);
  hipLaunchKernelGGL(m3s::asmk_append_kernel, dim3(blocks), dim3(256), 0, s, codes, words, count, max_count, D, n,
                     max_entries, db_codes, db_words, img_ptr, norm);
  return hipGetLastError();
}
