"""The device-resident ASMK database on the GPU: ``m3s.retrieval.AsmkDatabase`` / ``DatabaseMixin`` against the
reference's fixture (``tests/golden/asmk_update.npz``) and the numpy forward-file restatement (``tests/asmk_ref.py``,
itself pinned to the fixture by ``tests/test_asmk.py``).

Codes, words, ``img_ptr`` and the returned lists are exact. Scores: every term is non-negative and at most a few fp32
ulps from the reference's (``powf`` against numpy's, one rounded division), the sums are fp64, hence rtol 1e-6 with
atol 1e-12 (``asmk_ref.RTOL`` / ``ATOL``).
"""
import numpy as np
import pytest
import torch

import asmk_ref as R

pytestmark = pytest.mark.gpu


def _dev(x, dtype=None):
    return torch.as_tensor(np.array(x), dtype=dtype).cuda()  # a copy: the shared inputs are read-only


def _trim(codes, words, count):
    n = int(count.item())
    return codes[:n].cpu().numpy().view(np.uint32), words[:n].cpu().numpy()


def _db(case_or_c, kq, kb, **kw):
    from m3s.retrieval import AsmkDatabase

    return AsmkDatabase(_dev(case_or_c), R.asmk_params(kq, kb), **kw)


def _assert_export(db, ref):
    codes, words, img_ptr = db.export()
    assert (img_ptr == ref.img_ptr).all() and (words == ref.words).all() and (codes == ref.codes).all()


@pytest.mark.parametrize("name", R.CASES)
def test_aggregate_is_bit_exact_with_reference_fixture(golden, name):
    g = golden("asmk_update.npz")
    case = R.load_case(g, name)
    db = _db(case["c"], case["kq"], case["kb"])
    for i in range(case["n"]):
        ids, feat = _dev(case["ids"][i]), _dev(case["feats"][i])
        for k in ((case["kq"], case["kb"]) if i > 0 else (case["kb"],)):
            R.assert_fixture_aggregate(g, name, i, k, *_trim(*db.aggregate(feat, ids, k)))  # the first k columns
            R.assert_fixture_aggregate(g, name, i, k, *_trim(*db.aggregate(feat, ids[:, :k].contiguous())))


@pytest.mark.parametrize("name", R.CASES)
def test_search_matches_reference_scores(golden, name):
    """A database built with ``add`` from the reference's word ids, searched with every query of the case."""
    g = golden("asmk_update.npz")
    case = R.load_case(g, name)
    db = _db(case["c"], case["kq"], case["kb"])
    for i in range(case["n"]):
        ids, feat = _dev(case["ids"][i]), _dev(case["feats"][i])
        if i > 0:
            scores = db.search(*db.aggregate(feat, ids)).cpu().numpy()
            assert scores.dtype == np.float64 and scores.shape == (i,)
            np.testing.assert_allclose(scores, g[f"{name}_scores{i}"], rtol=R.RTOL, atol=R.ATOL)
        db.add(*db.aggregate(feat, ids, case["kb"]))
    assert db.n_images == case["n"]


@pytest.mark.parametrize("name", R.CASES)
def test_update_features_over_the_sequence(golden, name):
    """The fused call over the whole sequence. Against ``asmk_ref`` fed the device quantiser's own ids everything is
    compared; against the fixture's lists wherever the device's ids equal the reference's for that image and every
    earlier one (the inputs keep the nearest centroids 1e-3 apart, ten times the quantiser's tolerance, so no image is
    expected to be left out; at most one per case is allowed)."""
    g = golden("asmk_update.npz")
    case = R.load_case(g, name)
    db = _db(case["c"], case["kq"], case["kb"])
    ref = R.ForwardDb(case["c"], case["kq"], case["kb"])
    same, left_out = True, 0
    for i in range(case["n"]):
        feat = _dev(case["feats"][i])
        ids = db.codebook.quantize(feat, case["kq"] if i > 0 else case["kb"]).cpu().numpy()
        got = db.update_features(feat, True, case["K"], case["min_thresh"])
        want, want_scores = ref.update(case["feats"][i], ids, True, case["K"], case["min_thresh"], ids_build=ids)
        assert got == want, (name, i)
        if i > 0:
            scores = db.scores().cpu().numpy()
            np.testing.assert_allclose(scores, want_scores, rtol=R.RTOL, atol=R.ATOL)
            np.testing.assert_allclose(db.last_scores, scores[got], rtol=0, atol=0)
        same = same and (ids[:, :case["kb"]] == case["ids"][i][:, :case["kb"]]).all()
        if same and (ids == case["ids"][i]).all():
            assert got == case["lists"][i], (name, i)
            if i > 0:
                np.testing.assert_allclose(scores, g[f"{name}_scores{i}"], rtol=R.RTOL, atol=R.ATOL)
        else:
            left_out += 1
    print(f"case {name}: {left_out} of {case['n']} images left out of the fixture comparison")
    assert left_out <= 1
    assert db.n_images == case["n"]
    _assert_export(db, ref)


# ---- edge cases: expected values from asmk_ref; C = 64, D = 96 or 128, M <= 40 ----
def _small(D=96, M=24, n=4, seed=31, C=64):
    from m3s.synthetic import asmk_sequence

    return asmk_sequence(seed, C, D, M, n)


def test_feature_equal_to_its_centroid_gives_zero_bits():
    c, feats = _small(D=96, M=8, n=1)
    des = c[[3, 7, 7, 20]].copy()  # residuals exactly 0, also as the sum of two rows
    des[3, :50] += np.float32(0.25)  # and a row whose first 50 residuals are positive
    ids = np.array([[3], [7], [7], [20]])
    db = _db(c, 1, 1)
    codes, words = _trim(*db.aggregate(_dev(des), _dev(ids)))
    want_codes, want_words = R.aggregate(des, ids, c)
    assert words.tolist() == [3, 7, 20] == want_words.tolist()
    assert (codes[:2] == 0).all() and codes[2].tolist() == [0xffffffff, 0xffffc000, 0] and (codes == want_codes).all()


def test_half_distance_pair_and_image_without_common_word():
    """h == D / 2: sim == 0 >= similarity_threshold, so the pair is kept and contributes 0. An image that shares no
    word with the query scores exactly 0.0 and ``min_thresh = 0`` filters it."""
    D, W = 128, 4
    c, _ = _small(D=D, M=8, n=1)
    db = _db(c, 2, 1)
    ref = R.ForwardDb(c, 2, 1)
    half = np.array([0xffffffff, 0xffffffff, 0, 0], np.uint32)
    images = ((np.stack([half, np.zeros(W, np.uint32)]), np.array([5, 9], np.int32)),  # h = D / 2 and h = 0
              (np.stack([half]), np.array([5], np.int32)),  # only the h = D / 2 pair: 0.0
              (np.zeros((3, W), np.uint32), np.array([40, 41, 42], np.int32)))  # no common word: 0.0
    for codes, words in images:
        db.add(_dev(codes.view(np.int32)), _dev(words), _dev(np.array([len(words)], np.int32)))
        ref.add(codes, words)
    q_codes, q_words = np.zeros((3, W), np.uint32), np.array([5, 9, 11], np.int32)
    scores = db.search(_dev(q_codes.view(np.int32)), _dev(q_words), _dev(np.array([3], np.int32))).cpu().numpy()
    want = ref.search(q_codes, q_words)
    assert ref.tab[D // 2] == 0 and want[0] > 0 and want[1] == 0 and want[2] == 0
    np.testing.assert_allclose(scores, want, rtol=R.RTOL, atol=R.ATOL)
    assert scores[1] == 0.0 and scores[2] == 0.0
    _assert_export(db, ref)


def test_update_flow_edge_cases():
    c, feats = _small(D=96, M=24, n=4)
    kq, kb = 3, 1
    db = _db(c, kq, kb)
    ref = R.ForwardDb(c, kq, kb)
    ids = [db.codebook.quantize(_dev(f), kq).cpu().numpy() for f in feats]
    # the first update on an empty database: [] with one image added
    assert db.n_images == 0 and db.update_features(_dev(feats[0]), True, 3, 0.0) == [] and db.n_images == 1
    ref.update(feats[0], None, True, 3, 0.0, ids_build=ids[0][:, :kb])
    # two database images added from identical features: equal scores, the lower index first
    for _ in range(2):
        db.update_features(_dev(feats[1]), True, 3, 0.0)
        ref.update(feats[1], ids[1], True, 3, 0.0)
    _assert_export(db, ref)
    # add_after_query=False leaves the database as it was; k larger than n_images
    before = db.export()
    got = db.update_features(_dev(feats[2]), False, 10, 0.0)
    want, want_scores = ref.update(feats[2], ids[2], False, 10, 0.0)
    scores = db.scores().cpu().numpy()
    np.testing.assert_allclose(scores, want_scores, rtol=R.RTOL, atol=R.ATOL)
    assert scores[1] == scores[2] and got == want and got.index(1) < got.index(2) and len(got) <= 3
    assert db.n_images == 3 and all((a == b).all() for a, b in zip(before, db.export()))
    # an image sharing no word is filtered by min_thresh = 0 (a score of 0.0 is not > 0)
    assert got == [int(i) for i in R.rank(want_scores, 10, 0.0)] and all(scores[i] > 0 for i in got)
    # min_thresh above every score
    assert db.update_features(_dev(feats[2]), False, 3, float(scores.max()) * 1.01) == []
    assert db.update_features(_dev(feats[2]), False, 3, float(np.sort(scores)[-2])) == [int(scores.argmax())]
    # two identical runs: bit-identical scores
    db.update_features(_dev(feats[3]), False, 3, 0.0)
    s1 = db.scores().cpu().numpy()
    db.update_features(_dev(feats[3]), False, 3, 0.0)
    assert (s1 == db.scores().cpu().numpy()).all()
    # an image sharing no word with the query scores exactly 0.0, and min_thresh = 0 filters it
    rng = np.random.default_rng(5)
    fa = c[50:56] + np.float32(0.01) * rng.standard_normal((6, 96)).astype(np.float32)
    fb = c[0:6] + np.float32(0.01) * rng.standard_normal((6, 96)).astype(np.float32)
    one = _db(c, 1, 1)
    assert one.update_features(_dev(fa), True, 3, 0.0) == []
    assert one.update_features(_dev(fb), True, 3, 0.0) == [] and one.scores().tolist() == [0.0]
    assert one.update_features(_dev(fb), True, 3, 0.0) == [1] and one.scores()[0].item() == 0.0
    assert one.update_features(_dev(fb), True, 3, -1.0) == [1, 2, 0]  # equal scores: the lower index first
    with pytest.raises(RuntimeError):
        db.update_features(_dev(feats[3][:, :64]), False, 3, 0.0)  # wrong D
    with pytest.raises(RuntimeError):
        db.update_features(_dev(feats[3]), False, 65, 0.0)  # k > 64


def test_free_parameters_alpha_threshold_and_build_assignments():
    """alpha, similarity_threshold and k_build are free: a non-integer exponent, a positive threshold and two build
    assignments (the append then takes the first two of four columns)."""
    from m3s.retrieval import AsmkDatabase

    c, feats = _small(D=128, M=40, n=5, seed=33)
    kq, kb, alpha, thr = 4, 2, 2.5, 0.125
    db = AsmkDatabase(_dev(c), R.asmk_params(kq, kb, alpha, thr))
    ref = R.ForwardDb(c, kq, kb, alpha, thr)
    assert (ref.tab[:57] > 0).all() and (ref.tab[57:] == 0).all()  # sim = 1 - h / 64 >= 0.125 up to h = 56
    for i, f in enumerate(feats):
        ids = db.codebook.quantize(_dev(f), kq if i > 0 else kb).cpu().numpy()
        got = db.update_features(_dev(f), True, 3, 0.0)
        want, want_scores = ref.update(f, ids, True, 3, 0.0, ids_build=ids)
        assert got == want
        if i > 0:
            np.testing.assert_allclose(db.scores().cpu().numpy(), want_scores, rtol=R.RTOL, atol=R.ATOL)
    _assert_export(db, ref)


def test_growth_keeps_the_database():
    from m3s.retrieval import AsmkDatabase

    class Tight(AsmkDatabase):
        ENTRIES_PER_IMAGE = 30  # 4 x 30 entries: the entry room fills as well as the image table

    c, feats = _small(D=96, M=33, n=9, seed=32)
    small = Tight(_dev(c), R.asmk_params(3, 1), max_images=4)
    roomy = _db(c, 3, 1)
    for f in feats:
        assert small.update_features(_dev(f), True, 3, 0.0) == roomy.update_features(_dev(f), True, 3, 0.0)
        assert (small.scores() == roomy.scores()).all()
    assert small.n_images == roomy.n_images == 9 and small._db.max_images > 4
    assert all((a == b).all() for a, b in zip(small.export(), roomy.export()))


def test_database_mixin_gives_the_reference_lists(golden):
    from types import SimpleNamespace

    from m3s.retrieval import DatabaseMixin

    g = golden("asmk_update.npz")
    case = R.load_case(g, "A")

    class Host(DatabaseMixin):
        def __init__(self):
            self.centroids = _dev(case["c"])
            self.asmk = SimpleNamespace(params=R.asmk_params(case["kq"], case["kb"]))
            self.kf_counter, self.kf_ids = 0, []

        def prep_features(self, feat):
            return feat

    host = Host()
    ref = R.ForwardDb(case["c"], case["kq"], case["kb"])
    kq_params = {"quantize": {"multiple_assignment": case["kq"]}}
    ids = [host.quantize_custom(_dev(f), kq_params).cpu().numpy() for f in case["feats"]]
    same = np.cumprod([(a[:, :b.shape[1]] == b).all() for a, b in zip(ids, case["ids"])])
    for i in range(case["n"]):
        frame = SimpleNamespace(feat=_dev(case["feats"][i:i + 1]))
        got = host.update(frame, True, case["K"], case["min_thresh"])
        want, _ = ref.update(case["feats"][i], ids[i], True, case["K"], case["min_thresh"],
                             ids_build=ids[i][:, :case["kb"]])
        assert got == want
        if same[i]:
            assert got == case["lists"][i]
    assert same.sum() >= case["n"] - 1
    assert host.kf_counter == case["n"] and host.kf_ids == list(range(case["n"]))
    # query / add_to_database, the reference's two halves of update
    ranks, ranked, topk = host.query(case["feats"][0].copy(), None)
    assert ranks.shape == ranked.shape == (1, case["n"]) and topk.shape == (case["M"], case["kq"])
    assert (np.diff(ranked[0]) <= 0).all()
    host.add_to_database(case["feats"][0].copy(), None, topk)
    assert host.kf_counter == case["n"] + 1 and host._m3s_database().n_images == case["n"] + 1
