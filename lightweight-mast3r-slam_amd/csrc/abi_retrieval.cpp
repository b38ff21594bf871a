// C ABI of libm3s.so (include/m3s.h): retrieval codebook quantization (retrieval_database.py:96-105). Kernels live in
// retrieval.hip.
#include "abi_common.h"
#include "m3s_retrieval.h"

using namespace m3s_abi;

namespace {
inline int rq_steps(int D) { return (D + 31) / 32; }
inline int rq_rows_padded(int C) { return (C + RQ_ROWS - 1) / RQ_ROWS * RQ_ROWS; }
inline int rq_groups(int M) { return (M + RQ_QG - 1) / RQ_QG; }

struct CodebookWs {
  uint4* frag;  // (Cp/16 tiles) x S x {hi, lo} x 64 lanes (rq_prep_kernel)
  float* cn;    // (Cp) squared norms
};

size_t codebook_carve(Carver& c, int C, int D, CodebookWs* w) {
  const size_t Cp = (size_t)rq_rows_padded(C);
  w->frag = c.take<uint4>(Cp / 16 * rq_steps(D) * 128);
  w->cn = c.take<float>(Cp);
  return c.off;
}

struct QuantizeWs {
  uint4* qfrag;
  float* qn;
  unsigned long long* cand;
};

size_t quantize_carve(Carver& c, int C, int D, int M, int k, QuantizeWs* w) {
  const int G = rq_groups(M);
  w->qfrag = c.take<uint4>((size_t)G * rq_steps(D) * RQ_NQT * 128);
  w->qn = c.take<float>((size_t)G * RQ_QG);
  w->cand = c.take<unsigned long long>((size_t)G * (rq_rows_padded(C) / RQ_ROWS) * RQ_QG * k);
  return c.off;
}
}  // namespace

extern "C" size_t m3s_codebook_size(int C, int D) {
  if (C <= 0 || D <= 0) return 0;
  Carver c(nullptr);
  CodebookWs w;
  return codebook_carve(c, C, D, &w);
}

extern "C" int m3s_codebook_prepare(const float* centroids, int C, int D, void* codebook, size_t codebook_bytes,
                                    void* stream) {
  M3S_CHECK(centroids && codebook, "codebook: null argument");
  M3S_CHECK(C > 0 && D > 0, "codebook: C and D must be positive");
  M3S_CHECK((long long)rq_rows_padded(C) * rq_steps(D) * 32 < (1ll << 31), "codebook: too large");
  if (codebook_bytes < m3s_codebook_size(C, D)) return fail(M3S_ESPACE, "codebook: buffer too small");
  Carver c(codebook);
  CodebookWs w;
  codebook_carve(c, C, D, &w);
  hipStream_t s = (hipStream_t)stream;
  const int Cp = rq_rows_padded(C);
  HIP_TRY(m3s_launch_rq_prep(centroids, C, D, rq_steps(D), Cp / 16, RQ_ROWS / 16, w.frag, Cp, __builtin_inff(), w.cn,
                             s),
          "codebook prep launch");
  return M3S_OK;
}

extern "C" size_t m3s_quantize_workspace_size(int C, int D, int M, int k) {
  if (C <= 0 || D <= 0 || M <= 0 || k <= 0) return 0;
  Carver c(nullptr);
  QuantizeWs w;
  return quantize_carve(c, C, D, M, k, &w);
}

extern "C" int m3s_quantize(const void* codebook, int C, int D, const float* qvecs, int M, int k, int64_t* topk_out,
                            void* workspace, size_t workspace_bytes, void* stream) {
  M3S_CHECK(codebook && qvecs && topk_out && workspace, "quantize: null argument");
  M3S_CHECK(C > 0 && D > 0 && M > 0, "quantize: C, D and M must be positive");
  M3S_CHECK(k >= 1 && k <= 8, "quantize: k (multiple_assignment) must be in 1..8");
  M3S_CHECK(k <= C, "quantize: k larger than the codebook (torch.topk: selected index k out of range)");
  M3S_CHECK(rq_groups(M) < 65536, "quantize: too many query rows");
  if (workspace_bytes < m3s_quantize_workspace_size(C, D, M, k)) return fail(M3S_ESPACE, "quantize: workspace too small");
  Carver cb(const_cast<void*>(codebook));
  CodebookWs book;
  codebook_carve(cb, C, D, &book);
  Carver c(workspace);
  QuantizeWs w;
  quantize_carve(c, C, D, M, k, &w);
  hipStream_t s = (hipStream_t)stream;
  const int G = rq_groups(M), S = rq_steps(D);
  HIP_TRY(m3s_launch_rq_prep(qvecs, M, D, S, G * RQ_NQT, RQ_NQT, w.qfrag, G * RQ_QG, 0.0f, w.qn, s),
          "quantize prep launch");
  {
    Span sp("quantize_topk", s);
    HIP_TRY(m3s_launch_rq_topk(book.frag, book.cn, w.qfrag, w.qn, S, rq_rows_padded(C) / RQ_ROWS, G, M, k, w.cand,
                               topk_out, s),
            "quantize topk launch");
  }
  return M3S_OK;
}
