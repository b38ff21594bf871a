"""The ASMK update in numpy, in the forward-file formulation the device uses (not a test module).

The reference keeps an inverted file (one growable list per visual word, ``asmk/inverted_file.py``) and scores a query
word by word. The device keeps the entries in insertion order with per-image offsets and scores image by image. Both
visit the same (query word, database entry) pairs, so the scores agree up to the order of the fp64 sum; the golden
fixture ``tests/golden/asmk_update.npz`` (written from the reference's own kernel and inverted file) pins that, and
``tests/test_asmk.py`` checks this file against it. The GPU tests then use this file where the fixture cannot serve
(the device quantiser's own ids, edge cases).
"""
import numpy as np


def popcount32(x):
    x = np.asarray(x, dtype=np.uint32)
    return np.unpackbits(x.view(np.uint8).reshape(x.shape + (4,)), axis=-1).sum(axis=-1, dtype=np.int64)


def aggregate(des, word_ids, centroids):
    """``ASMKKernel.aggregate_image`` + ``binarize_and_pack_2D``: (codes (nq, D / 32) uint32, words (nq) int32 sorted).
    Per unique word the fp32 residuals des[row] - centroid[word] of its rows (ascending, a row once) are added one
    after another; bit = sum > 0, dim d in word d // 32 at bit 31 - d % 32."""
    des = np.asarray(des, dtype=np.float32)
    word_ids = np.asarray(word_ids)
    D = des.shape[1]
    assert D % 32 == 0
    words = np.unique(word_ids)
    codes = np.empty((len(words), D // 32), dtype=np.uint32)
    for i, w in enumerate(words):
        acc = np.zeros(D, dtype=np.float32)
        for r in np.flatnonzero((word_ids == w).any(axis=1)):
            acc = acc + (des[r] - centroids[w])
        codes[i] = np.packbits(acc > 0, bitorder="big").view(">u4").astype(np.uint32)
    return codes, words.astype(np.int32)


def sim_table(D, alpha, similarity_threshold):
    """powf(sim, alpha) for h = 0 .. D in the reference's fp32 operations, 0 where sim < similarity_threshold."""
    nh = np.arange(D + 1, dtype=np.float32) / np.float32(D)
    sim = np.float32(-2) * nh + np.float32(1)
    with np.errstate(invalid="ignore"):
        p = np.power(sim, np.float32(alpha))
    return np.where(sim >= np.float32(similarity_threshold), p, np.float32(0)).astype(np.float32)


class ForwardDb:
    """Entries in insertion order: codes (E, D / 32) uint32, words (E) int32, img_ptr (n + 1)."""

    def __init__(self, centroids, k_query, k_build, alpha=3.0, similarity_threshold=0.0):
        self.centroids = np.asarray(centroids, dtype=np.float32)
        self.D = self.centroids.shape[1]
        self.k_query, self.k_build = k_query, k_build
        self.tab = sim_table(self.D, alpha, similarity_threshold)
        self.codes = np.zeros((0, self.D // 32), dtype=np.uint32)
        self.words = np.zeros(0, dtype=np.int32)
        self.img_ptr = np.zeros(1, dtype=np.int32)

    @property
    def n_images(self):
        return len(self.img_ptr) - 1

    def add(self, codes, words):
        self.codes = np.concatenate([self.codes, codes])
        self.words = np.concatenate([self.words, words])
        self.img_ptr = np.append(self.img_ptr, np.int32(len(self.words)))

    def search(self, q_codes, q_words):
        """(n_images) float64 scores: per image the sum over its entries whose word the query holds."""
        scores = np.zeros(self.n_images, dtype=np.float64)
        for i in range(self.n_images):
            e0, e1 = self.img_ptr[i], self.img_ptr[i + 1]
            w = self.words[e0:e1]
            pos = np.searchsorted(q_words, w)
            hit = (pos < len(q_words)) & (q_words[np.minimum(pos, len(q_words) - 1)] == w)
            h = popcount32(self.codes[e0:e1][hit] ^ q_codes[pos[hit]]).sum(axis=1)
            term = (self.tab[h].astype(np.float64) / np.sqrt(np.float64(e1 - e0))).astype(np.float32)
            scores[i] = term.astype(np.float64).sum()
        return scores / np.float64(np.sqrt(np.float32(len(q_words))))

    def update(self, des, ids_query, add_after_query, k, min_thresh=0.0, ids_build=None):
        """``RetrievalDatabase.update`` after prep_features, given the quantiser's word ids: ``ids_query`` (M, k_query)
        when the database holds an image, else ``ids_build`` (M, k_build). Returns (index list, scores or None)."""
        inds, scores = [], None
        if self.n_images > 0:
            scores = self.search(*aggregate(des, ids_query, self.centroids))
            inds = rank(scores, k, min_thresh)
            ids_build = ids_query[:, :self.k_build]
        if add_after_query:
            self.add(*aggregate(des, ids_build, self.centroids))
        return inds, scores


def rank(scores, k, min_thresh):
    """torch.topk(scores, min(k, n)): NaN first (the lower index first among them), then descending with ties to the
    lower index; then the ``> min_thresh`` filter, which no NaN passes."""
    scores = np.asarray(scores, dtype=np.float64)
    nan = np.isnan(scores)
    order = np.lexsort((np.arange(len(scores)), np.where(nan, 0.0, -scores), ~nan))[:min(k, len(scores))]
    return [int(i) for i in order if scores[i] > min_thresh]


# ---- the golden fixture tests/golden/asmk_update.npz (tests/golden/make_golden_asmk.py) ----
CASES = ("A", "B", "C")
RTOL, ATOL = 1e-6, 1e-12  # scores: non-negative terms a few fp32 ulps apart (powf, one rounded division), fp64 sums


def asmk_params(k_query, k_build, alpha=3.0, similarity_threshold=0.0, binary=True, use_idf=False):
    """The reference's asmk params dict (mast3r/retrieval/processor.py:91-96) with the free parameters set."""
    return {"build_ivf": {"kernel": {"binary": binary}, "ivf": {"use_idf": use_idf},
                          "quantize": {"multiple_assignment": k_build}, "aggregate": {}},
            "query_ivf": {"quantize": {"multiple_assignment": k_query}, "aggregate": {}, "search": {"topk": None},
                          "similarity": {"similarity_threshold": similarity_threshold, "alpha": alpha}}}


_INPUTS = {}


def load_case(g, name):
    """The case's regenerated inputs and shapes; g = the loaded fixture."""
    from m3s.synthetic import asmk_sequence

    seed, C, D, M, kq, kb, n, K = (int(x) for x in g[f"{name}_case"])
    if name not in _INPUTS:
        c, feats = asmk_sequence(seed, C, D, M, n)
        np.testing.assert_allclose([c.astype(np.float64).sum(), feats.astype(np.float64).sum()], g[f"{name}_checksum"],
                                   rtol=0, atol=1e-9)  # inputs regenerated bit-identically
        c.setflags(write=False)
        feats.setflags(write=False)
        _INPUTS[name] = (c, feats)
    c, feats = _INPUTS[name]
    lists = [[int(x) for x in row if x >= 0] for row in g[f"{name}_lists"]]
    return dict(C=C, D=D, M=M, kq=kq, kb=kb, n=n, K=K, min_thresh=float(g[f"{name}_min_thresh"]), c=c, feats=feats,
                lists=lists, ids=[g[f"{name}_ids{i}"].astype(np.int64) for i in range(n)])


def assert_fixture_aggregate(g, name, i, k, codes, words):
    """codes / words equal the reference's aggregate of image i over k columns (codes by sha256 where stored so)."""
    import hashlib

    assert (np.asarray(words) == g[f"{name}_words{i}_k{k}"]).all(), (name, i, k)
    codes = np.ascontiguousarray(codes, dtype="<u4")
    key = f"{name}_codes{i}_k{k}"
    if key in g:
        assert codes.shape == g[key].shape and (codes == g[key]).all(), (name, i, k)
    else:
        assert hashlib.sha256(codes.tobytes()).digest() == g[key + "_sha256"].tobytes(), (name, i, k)
