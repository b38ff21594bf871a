"""GPU: the ASMK database kernels (csrc/asmk.hip) through ``m3s.retrieval.AsmkDatabase`` at the shapes where each of
their branches runs.

The cases, their builders and the expectations (all from tests/asmk_ref.py) are in tests/asmk_edge_cases.py;
tests/test_asmk_edges_host.py shows on the CPU that every case reaches the branch it is named for: the sort's padded
sizes up to the two-pass P = 4096, all 16 waves of the scan, key bit 31, the repeat filter deciding inside a thread and
across waves, one word with 4096 rows, the order of a word's adds (309 rows whose sum is rounding error alone), every
code-word layout from D = 32 to 288 and 1024, both popcount paths, images of 4096 entries against 4096 query words,
the append's stride loop, an image without entries, more than 256 images, k = 64, NaN scores, 4096 keys through the
fused update.

Exact (``array_equal``): codes, words, counts, ``img_ptr``, the exported database, every returned list and its
``last_scores``, the scores of ``exact_scores_*`` (D a power of two, alpha 3, norms powers of four: every term is a
dyadic rational and the fp64 sum exact in any order) and of ``topk_ties`` (one table value each), the positions of
the NaNs. Within ``asmk_ref.RTOL`` / ``ATOL`` (a few fp32 ulps per term, fp64 sums): the scores of ``big_append``,
``empty_image`` (its 0.0 exact), ``topk_nan`` (alpha 2.5) and the fused update. Every comparison covers every
element: no share of allowed mismatches, and no image is left out.

Mutation check (by hand on a copy, not committed; selection or arithmetic changes of asmk.hip with every index in
bounds, the sort mutations with the written word and row clamped so that a misplaced padding key stays inside the
arrays; one run per mutation of this file, 31 tests, and of tests/test_gpu_asmk.py, 15 tests, the only other GPU
tests that launch these kernels; unmutated both are green):
  (a) the bitonic step compares the keys as ``int32_t``: 1 red (``high_words``); the earlier suite stays green;
  (b) one pass of the bitonic pair loop (``t < 1024`` only): 7 red (``p4096_first``, ``full_distinct``, ``k8_full``,
      ``dup_in_row``, ``high_words``, both fused updates); ``full_one_word`` stays green, its keys arrive sorted;
      the earlier suite stays green;
  (c) ``keep[u] = 1``: 1 red (``dup_in_row``); the earlier suite stays green;
  (d) a word's rows added in descending order: 2 red (``order_sensitive_288``, ``_1024``); the earlier suite stays
      green, also ``full_one_word`` and ``k8_full`` here (Gaussian rows of one scale: no sum close enough to zero);
  (e) ``asmk_topk_kernel`` skips the images i >= 256: 2 red (``topk_ties``, ``topk_nan``); the earlier suite stays
      green;
  (f) ``asmk_before`` without its NaN branch: 1 red (``topk_nan``); the earlier suite stays green;
  (g) ``asmk_append_kernel`` without the stride loop's further passes: 1 red (``big_append``); the earlier suite stays
      green;
  (h) the score's vector path reads the first ``uint4`` of an entry only: 2 red (``exact_scores_256``,
      ``big_append``); the earlier suite is red too (fixture C, D = 1024: its search and its fused update).
"""
import numpy as np
import pytest
import torch

import asmk_edge_cases as E
import asmk_ref as R

pytestmark = pytest.mark.gpu


def _dev(x, dtype=None):
    return torch.as_tensor(np.array(x), dtype=dtype).cuda()  # a copy: the cases are read-only


def _count(n):
    return _dev(np.array([n], np.int32))


_BOOKS = {}


def _db(c, kq=1, kb=1, alpha=3.0, thr=0.0):
    """A fresh database on the case's codebook; one Codebook per distinct centroid array."""
    from m3s.retrieval import AsmkDatabase, Codebook

    if id(c) not in _BOOKS:
        _BOOKS[id(c)] = (c, Codebook(_dev(c)))
    return AsmkDatabase(_BOOKS[id(c)][1], R.asmk_params(kq, kb, alpha, thr))


def _assert_export(db, ref):
    codes, words, img_ptr = db.export()
    assert np.array_equal(img_ptr, ref.img_ptr) and np.array_equal(words, ref.words)
    assert codes.shape == ref.codes.shape and np.array_equal(codes, ref.codes)


# ---- A. sort and aggregate ----
@pytest.mark.parametrize("name", E.AGG_NAMES)
def test_aggregate_case_exact(name):
    cs = E.agg(name)
    db = _db(cs.c)
    ids = _dev(cs.ids)
    args = (ids,) if cs.use_cols == cs.ids.shape[1] else (ids, cs.use_cols)
    codes, words, count = db.aggregate(_dev(cs.des), *args)
    n = int(count.item())
    assert n == len(cs.words), f"{name}: count {n}, expected {len(cs.words)}"
    words = words[:n].cpu().numpy()
    codes = codes[:n].cpu().numpy().view(np.uint32)
    assert np.array_equal(words, cs.words), f"{name}: words differ first at {np.flatnonzero(words != cs.words)[:5]}"
    bad = np.argwhere(codes != cs.codes)
    assert len(bad) == 0, (f"{name}: {len(bad)} of {codes.size} code words differ; first (slot, word) "
                           f"{bad[:5].tolist()}, {int(R.popcount32(codes ^ cs.codes).sum())} bits")


# ---- B. add and search ----
def _fill(db, cs):
    for codes, words, n in cs.images:
        db.add(_dev(codes.view(np.int32)), _dev(words), _count(n))


def _search(db, cs):
    scores = db.search(_dev(cs.q_codes.view(np.int32)), _dev(cs.q_words), _count(len(cs.q_words))).cpu().numpy()
    assert scores.dtype == np.float64 and scores.shape == cs.scores.shape
    return scores


@pytest.mark.parametrize("D", E.EXACT_D)
def test_exact_scores(D):
    cs = E.search(f"exact_scores_{D}")
    db = _db(cs.c)
    _fill(db, cs)
    scores = _search(db, cs)
    print(f"exact_scores_{D}: largest difference {np.abs(scores - cs.scores).max():.3e}")
    assert np.array_equal(scores, cs.scores), (scores.tolist(), cs.scores.tolist())
    _assert_export(db, cs.ref)


def test_big_append():
    cs = E.search("big_append")
    db = _db(cs.c)
    _fill(db, cs)
    _assert_export(db, cs.ref)
    scores = _search(db, cs)
    print(f"big_append: largest relative difference {np.abs(scores / cs.scores - 1).max():.3e}")
    np.testing.assert_allclose(scores, cs.scores, rtol=R.RTOL, atol=R.ATOL)


def test_empty_image():
    cs = E.search("empty_image")
    db = _db(cs.c)
    _fill(db, cs)
    _assert_export(db, cs.ref)
    assert db.n_images == 3 and db.export()[2].tolist() == [0, 10, 10, 17]
    scores = _search(db, cs)
    assert scores[1] == 0.0 and not np.signbit(scores[1])
    np.testing.assert_allclose(scores, cs.scores, rtol=R.RTOL, atol=R.ATOL)
    alone = _db(cs.c)  # the neighbours alone score the same, bit for bit
    for i in (0, 2):
        alone.add(_dev(cs.images[i][0].view(np.int32)), _dev(cs.images[i][1]), _count(cs.images[i][2]))
    assert np.array_equal(_search(alone, cs._replace(scores=cs.scores[[0, 2]])), scores[[0, 2]])


# ---- C. top-k ----
def _topk_db(cs):
    db = _db(cs.c, 1, 1, cs.alpha, cs.thr)
    codes, words, one = _dev(cs.codes.view(np.int32)), _dev(np.full(len(cs.codes), cs.w0, np.int32)), _count(1)
    for i in range(len(cs.codes)):
        db.add(codes[i:i + 1], words[i:i + 1], one)
    assert db.n_images == len(cs.codes)
    return db


def _run_topk(cs):
    db = _topk_db(cs)
    feat = _dev(cs.feat)
    assert db.codebook.quantize(feat, 1).cpu().numpy().tolist() == [[cs.w0]]
    for k, t, want in cs.runs:
        got = db.update_features(feat, False, k, t)
        scores = db.scores().cpu().numpy()
        assert got == want, f"{cs.name} k={k} min_thresh={t}: {got} != {want}"
        assert np.array_equal(db.last_scores, scores[got])
        yield k, t, scores
    assert db.n_images == len(cs.codes)  # add_after_query=False


def test_topk_ties():
    cs = E.topk("topk_ties")
    for k, t, scores in _run_topk(cs):
        assert np.array_equal(scores, cs.scores), f"k={k} min_thresh={t}"


def test_topk_nan():
    cs = E.topk("topk_nan")
    for k, t, scores in _run_topk(cs):
        assert np.array_equal(np.isnan(scores), np.isnan(cs.scores)), f"k={k} min_thresh={t}"
        np.testing.assert_allclose(scores, cs.scores, rtol=R.RTOL, atol=R.ATOL, equal_nan=True)


# ---- D. the fused update at the key limit ----
@pytest.mark.parametrize("name", E.UPDATE_NAMES)
def test_update_at_the_key_limit(name):
    cs = E.update(name)
    db = _db(cs.c, cs.kq, cs.kb)
    ref = R.ForwardDb(cs.c, cs.kq, cs.kb)
    for i, f in enumerate(cs.feats):
        feat = _dev(f)
        ids = db.codebook.quantize(feat, cs.kq if i > 0 else cs.kb).cpu().numpy()
        assert np.array_equal(ids, cs.ids[i]), (name, i)  # the margin is ten times the quantiser's tolerance
        got = db.update_features(feat, True, cs.K, cs.min_thresh)
        want, want_scores = ref.update(f, ids, True, cs.K, cs.min_thresh, ids_build=ids)  # the device's own ids
        assert got == want == cs.lists[i], (name, i)
        if i > 0:
            scores = db.scores().cpu().numpy()
            assert np.array_equal(want_scores, cs.scores[i])
            np.testing.assert_allclose(scores, want_scores, rtol=R.RTOL, atol=R.ATOL)
            assert np.array_equal(db.last_scores, scores[got])
    assert db.n_images == len(cs.feats)
    _assert_export(db, ref)
    _assert_export(db, cs.ref)
