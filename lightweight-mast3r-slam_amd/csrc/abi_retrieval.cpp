// C ABI of libm3s.so (include/m3s.h): retrieval codebook quantization (retrieval_database.py:96-105, kernels in
// retrieval.hip) and the device-resident ASMK database around it (retrieval_database.py:43-166, kernels in asmk.hip).
#include "abi_common.h"
#include "m3s_retrieval.h"

#include <cmath>
#include <vector>

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

// ---- the device-resident ASMK database (include/m3s.h, the m3s_asmk_* section). Kernels live in asmk.hip. ----
namespace {
struct AsmkDbSecs {
  float* table;
  uint32_t* codes;
  int32_t *words, *img_ptr, *norm;
  double* scores;
};

size_t asmk_db_carve(Carver& c, int D, int max_images, int64_t max_entries, AsmkDbSecs* w) {
  w->table = c.take<float>((size_t)D + 1);
  w->codes = c.take<uint32_t>((size_t)max_entries * (D / 32));
  w->words = c.take<int32_t>((size_t)max_entries);
  w->img_ptr = c.take<int32_t>((size_t)max_images + 1);
  w->norm = c.take<int32_t>((size_t)max_images);
  w->scores = c.take<double>((size_t)max_images);
  return c.off;
}

bool asmk_db_shape_ok(int D, int max_images, int64_t max_entries) {
  return D > 0 && D % 32 == 0 && max_images > 0 && max_entries > 0 && max_entries * (D / 32) < (1ll << 31);
}

// One aggregate of an image: the outputs and the sort's row lists
struct AsmkAgg {
  uint32_t* codes;
  int32_t *words, *count, *seg, *rows;
};

void asmk_agg_carve(Carver& c, int D, int keys, AsmkAgg* a, bool with_outputs) {
  if (with_outputs) {
    a->codes = c.take<uint32_t>((size_t)keys * (D / 32));
    a->words = c.take<int32_t>((size_t)keys);
    a->count = c.take<int32_t>(1);
  }
  a->seg = c.take<int32_t>((size_t)keys + 1);
  a->rows = c.take<int32_t>((size_t)keys);
}

struct AsmkWs {
  AsmkAgg scratch;  // m3s_asmk_aggregate: seg and rows only (the caller owns the outputs)
  AsmkAgg q, b;     // m3s_asmk_update: the k_query and the k_build aggregate
  int64_t* ids;
  void* quant;
  size_t quant_bytes;
};

size_t asmk_carve(Carver& c, int C, int D, int M, int k, AsmkWs* w) {
  const int keys = M * k;
  asmk_agg_carve(c, D, keys, &w->scratch, false);
  asmk_agg_carve(c, D, keys, &w->q, true);
  asmk_agg_carve(c, D, keys, &w->b, true);
  w->ids = c.take<int64_t>((size_t)keys);
  w->quant_bytes = m3s_quantize_workspace_size(C, D, M, k);
  w->quant = c.take<char>(w->quant_bytes);
  return c.off;
}

// The limits of the sort's 32-bit (word << 12 | row) keys and its LDS array
int asmk_check_shape(int C, int D, int M, int k, int use_cols) {
  M3S_CHECK(C > 0 && D > 0 && M > 0, "asmk: C, D and M must be positive");
  M3S_CHECK(D % 32 == 0, "asmk: D must be a multiple of 32 (the packed binary codes)");
  M3S_CHECK(C <= (1 << 20), "asmk: the codebook must not exceed 2^20 words");
  M3S_CHECK(k >= 1 && k <= 8, "asmk: k (multiple_assignment) must be in 1..8");
  M3S_CHECK(use_cols >= 1 && use_cols <= k, "asmk: use_cols must be in 1..k (build multiple_assignment <= query's)");
  M3S_CHECK(M <= ASMK_MAX_KEYS && (long long)M * k <= ASMK_MAX_KEYS, "asmk: M and M * k must not exceed 4096");
  return M3S_OK;
}

int asmk_check_db(const m3s_asmk_db* db) {
  M3S_CHECK(db && db->buf, "asmk: null database");
  M3S_CHECK(asmk_db_shape_ok(db->D, db->max_images, db->max_entries), "asmk: bad database shape");
  M3S_CHECK(db->table && db->codes && db->words && db->img_ptr && db->norm && db->scores,
            "asmk: database not initialised (m3s_asmk_db_init)");
  M3S_CHECK(db->n_images >= 0 && db->n_images <= db->max_images && db->entries_bound >= 0 &&
                db->entries_bound <= db->max_entries,
            "asmk: database bookkeeping out of range");
  return M3S_OK;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int asmk_run_aggregate(const float* centroids, int C, int D, const float* features, int M, const int64_t* ids, int k,
                       int use_cols, const AsmkAgg& a, hipStream_t s) {
  HIP_TRY(m3s_launch_asmk_sort(ids, M, k, use_cols, C, a.words, a.seg, a.rows, a.count, s), "asmk sort launch");
  HIP_TRY(m3s_launch_asmk_aggregate(features, centroids, D, M * use_cols, a.words, a.seg, a.rows, a.count, a.codes, s),
          "asmk aggregate launch");
  return M3S_OK;
}

// Room for another image of at most `bound` entries? Nothing is launched when there is not.
int asmk_check_room(const m3s_asmk_db* db, int bound) {
  if (db->n_images >= db->max_images) return fail(M3S_ESPACE, "asmk: database full (max_images)");
  if (db->entries_bound + bound > db->max_entries) return fail(M3S_ESPACE, "asmk: database full (max_entries)");
  return M3S_OK;
}

int asmk_run_append(m3s_asmk_db* db, const uint32_t* codes, const int32_t* words, const int32_t* count, int bound,
                    hipStream_t s) {
  HIP_TRY(m3s_launch_asmk_append(codes, words, count, bound, db->D, db->n_images, db->max_entries, db->codes,
                                 db->words, db->img_ptr, db->norm, s),
          "asmk append launch");
  db->n_images += 1;
  db->entries_bound += bound;
  return M3S_OK;
}
}  // namespace

extern "C" size_t m3s_asmk_db_size(int D, int max_images, int64_t max_entries) {
  if (!asmk_db_shape_ok(D, max_images, max_entries)) return 0;
  Carver c(nullptr);
  AsmkDbSecs w;
  return asmk_db_carve(c, D, max_images, max_entries, &w);
}

extern "C" int m3s_asmk_db_init(m3s_asmk_db* db, float alpha, float similarity_threshold, void* stream) {
  M3S_CHECK(db && db->buf, "asmk init: null database");
  M3S_CHECK(asmk_db_shape_ok(db->D, db->max_images, db->max_entries),
            "asmk init: D must be a positive multiple of 32, max_images and max_entries positive");
  if (db->bytes < m3s_asmk_db_size(db->D, db->max_images, db->max_entries))
    return fail(M3S_ESPACE, "asmk init: buffer too small");
  Carver c(db->buf);
  AsmkDbSecs w;
  asmk_db_carve(c, db->D, db->max_images, db->max_entries, &w);
  // sim and powf(sim, alpha) take D + 1 values: kernel.py:62-63 (a C float division in hamming.pyx:42, then
  // -2 x + 1 on the float32 array) and functional.py:13-14 (np.power of float32 by the scalar alpha), in those fp32
  // operations. -2 x is exact, so a contracted multiply-add rounds like the separate operations. A pair below the
  // threshold adds nothing, like the masked-out entries of the reference.
  const int D = db->D;
  std::vector<float> tab((size_t)D + 1);
  for (int h = 0; h <= D; h++) {
    const float nh = (float)h / (float)D;
    const float sim = -2.0f * nh + 1.0f;
    tab[h] = sim >= similarity_threshold ? powf(sim, alpha) : 0.0f;
  }
  hipStream_t s = (hipStream_t)stream;
  const UploadSec sec = {tab.data(), tab.size() * sizeof(float), nullptr};
  const int rc = stage_upload(&sec, 1, w.table, s, {"asmk table stage", "asmk table upload", "asmk table event"});
  if (rc != M3S_OK) return rc;
  HIP_TRY(hipMemsetAsync(w.img_ptr, 0, sizeof(int32_t), s), "asmk img_ptr reset");
  db->table = w.table;
  db->codes = w.codes;
  db->words = w.words;
  db->img_ptr = w.img_ptr;
  db->norm = w.norm;
  db->scores = w.scores;
  db->n_images = 0;
  db->entries_bound = 0;
  return M3S_OK;
}

extern "C" size_t m3s_asmk_workspace_size(int C, int D, int M, int k) {
  if (C <= 0 || D <= 0 || D % 32 != 0 || M <= 0 || k <= 0 || (long long)M * k > ASMK_MAX_KEYS) return 0;
  Carver c(nullptr);
  AsmkWs w;
  return asmk_carve(c, C, D, M, k, &w);
}

extern "C" int m3s_asmk_aggregate(const float* centroids, int C, int D, const float* features, int M,
                                  const int64_t* ids, int k, int use_cols, uint32_t* codes, int32_t* words,
                                  int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
  M3S_CHECK(centroids && features && ids && codes && words && count && workspace, "asmk aggregate: null argument");
  if (int rc = asmk_check_shape(C, D, M, k, use_cols)) return rc;
  if (workspace_bytes < m3s_asmk_workspace_size(C, D, M, k)) return fail(M3S_ESPACE, "asmk aggregate: workspace too small");
  Carver c(workspace);
  AsmkWs w;
  asmk_carve(c, C, D, M, k, &w);
  AsmkAgg a = w.scratch;
  a.codes = codes;
  a.words = words;
  a.count = count;
  return asmk_run_aggregate(centroids, C, D, features, M, ids, k, use_cols, a, (hipStream_t)stream);
}

extern "C" int m3s_asmk_search(const m3s_asmk_db* db, const uint32_t* q_codes, const int32_t* q_words,
                               const int32_t* q_count, int max_q, double* scores, void* stream) {
  if (int rc = asmk_check_db(db)) return rc;
  M3S_CHECK(q_codes && q_words && q_count && scores, "asmk search: null argument");
  M3S_CHECK(max_q >= 1 && max_q <= ASMK_MAX_KEYS, "asmk search: max_q must be in 1..4096");
  M3S_CHECK(aligned16(q_codes), "asmk search: q_codes must be 16-byte aligned");
  M3S_CHECK(db->n_images > 0, "asmk search: empty database");
  HIP_TRY(m3s_launch_asmk_score(db->table, db->codes, db->words, db->img_ptr, db->norm, db->D, db->n_images, q_codes,
                                q_words, q_count, max_q, scores, (hipStream_t)stream),
          "asmk score launch");
  return M3S_OK;
}

extern "C" int m3s_asmk_add(m3s_asmk_db* db, const uint32_t* codes, const int32_t* words, const int32_t* count,
                            int max_count, void* stream) {
  if (int rc = asmk_check_db(db)) return rc;
  M3S_CHECK(codes && words && count, "asmk add: null argument");
  M3S_CHECK(max_count >= 1 && max_count <= ASMK_MAX_KEYS, "asmk add: max_count must be in 1..4096");
  if (int rc = asmk_check_room(db, max_count)) return rc;
  return asmk_run_append(db, codes, words, count, max_count, (hipStream_t)stream);
}

extern "C" int m3s_asmk_update(const void* codebook, const float* centroids, int C, m3s_asmk_db* db,
                               const float* features, int M, int k_query, int k_build, int k, double min_thresh,
                               int add_after_query, m3s_asmk_result* result, void* workspace, size_t workspace_bytes,
                               void* stream) {
  if (int rc = asmk_check_db(db)) return rc;
  M3S_CHECK(codebook && centroids && features && result && workspace, "asmk update: null argument");
  const int D = db->D;
  if (int rc = asmk_check_shape(C, D, M, k_query, k_build)) return rc;
  M3S_CHECK(k_query <= C, "asmk update: k_query larger than the codebook");
  M3S_CHECK(k >= 1 && k <= ASMK_MAX_TOPK, "asmk update: k must be in 1..64");
  if (workspace_bytes < m3s_asmk_workspace_size(C, D, M, k_query))
    return fail(M3S_ESPACE, "asmk update: workspace too small");
  if (add_after_query)
    if (int rc = asmk_check_room(db, M * k_build)) return rc;
  Carver c(workspace);
  AsmkWs w;
  asmk_carve(c, C, D, M, k_query, &w);
  hipStream_t s = (hipStream_t)stream;
  Span sp("asmk_update", s);
  const int n = db->n_images;
  int id_cols = k_query;  // the row stride of w.ids
  if (n > 0) {
    if (int rc = m3s_quantize(codebook, C, D, features, M, k_query, w.ids, w.quant, w.quant_bytes, stream)) return rc;
    if (int rc = asmk_run_aggregate(centroids, C, D, features, M, w.ids, k_query, k_query, w.q, s)) return rc;
    HIP_TRY(m3s_launch_asmk_score(db->table, db->codes, db->words, db->img_ptr, db->norm, D, n, w.q.codes, w.q.words,
                                  w.q.count, M * k_query, db->scores, s),
            "asmk score launch");
    HIP_TRY(m3s_launch_asmk_topk(db->scores, n, k, min_thresh, result, s), "asmk topk launch");
  } else {
    HIP_TRY(hipMemsetAsync(&result->count, 0, sizeof(int32_t), s), "asmk result reset");
    if (add_after_query) {  // nothing was queried: a fresh k_build quantisation (retrieval_database.py:149-154)
      id_cols = k_build;
      if (int rc = m3s_quantize(codebook, C, D, features, M, k_build, w.ids, w.quant, w.quant_bytes, stream)) return rc;
    }
  }
  if (add_after_query) {
    if (int rc = asmk_run_aggregate(centroids, C, D, features, M, w.ids, id_cols, k_build, w.b, s)) return rc;
    if (int rc = asmk_run_append(db, w.b.codes, w.b.words, w.b.count, M * k_build, s)) return rc;
  }
  return M3S_OK;
}
