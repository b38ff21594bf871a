"""CPU: the cases of the BA linearisation edge suite (tests/ba_edge_cases.py) reach what they are named for.

Every predicate is a function of the case and the oracle's fp64 truth only; tests/test_gpu_ba_edges.py then runs the
same cases through csrc/ba.hip. rho, rho_ref: ba_edge_cases.rho / rho_ref (BA, "edge shapes").
"""
import numpy as np
import pytest

import ba_edge_cases as B
import oracle.oracle as O

ALL = B.case_modes()
LIVE = [(n, m) for n, m in ALL if not B.SPECS[n]["zero"]]


def test_device_layout_identities():
    """The device row's M is Hs[3] (= Hs[0] = -Hs[1] = -Hs[2]^T) and its g is gs[1] (= -gs[0]) of the reference layout,
    on the fp64 output; the blocks that pair the two poses agree with M up to the order of a row's two products."""
    c = B.build("n513")
    for mode in B.MODES:
        Hs, gs, chi2 = B.truth_blocks(c, mode)
        assert np.array_equal(Hs[3], Hs[0]) and np.array_equal(gs[1], -gs[0])
        assert np.array_equal(Hs[3], np.swapaxes(Hs[3], 1, 2)) and np.array_equal(Hs[1], np.swapaxes(Hs[2], 1, 2))
        np.testing.assert_allclose(Hs[1], -Hs[3], rtol=0, atol=1e-13 * np.abs(Hs[3]).max())
        row = O.edge_row_from_blocks(Hs, gs)
        iu = np.triu_indices(7)
        assert np.array_equal(row[:, :28], Hs[3][:, iu[0], iu[1]]) and np.array_equal(row[:, 28:35], gs[1])
        assert not row[:, 35].any() and (chi2 > 0).all()
        H2, g2 = O.ba_linearize_f64(*B._args(c, mode))
        assert np.array_equal(H2, Hs) and np.array_equal(g2, gs)


@pytest.mark.parametrize("name,mode", ALL)
def test_reference_is_a_usable_yardstick(name, mode):
    """rho_ref is finite and below 1e-4 (a larger value means an ill-conditioned case), and the numpy point table
    the predicates use adds up to the oracle's own chi2."""
    c = B.build(name)
    r = B.rho_ref(c, mode)
    print(f"{name} {mode}: rho_ref {r:.2e}")
    assert np.isfinite(r) and r < 1e-4
    t = B.point_table(c, mode)
    _, chi2 = B.truth(c, mode)
    np.testing.assert_allclose(B.chi2_numpy(t), chi2, rtol=1e-6, atol=0)


@pytest.mark.parametrize("name,mode", LIVE)
def test_edges_are_densely_weighted(name, mode):
    """At least half of every edge's points carry weight under the case's own thresholds; Q lies on both sides of its
    threshold and at least 1 % away from it; weighted rows fall on both sides of Huber's k for every row type."""
    c = B.build(name)
    t = B.point_table(c, mode)
    share = t["weighted"].mean(1)
    print(f"{name} {mode}: weighted share per edge {np.round(share, 3).tolist()}")
    assert (share >= 0.5).all()
    qt = c["thresh"]["Q_thresh"]
    assert (np.abs(c["Q"] - qt) >= 0.01 * qt).all()
    assert B.only_fails(t, "Q").any() and (t["tests"]["Q"].sum(1) > 0).all()
    r = np.abs(t["r"][t["weighted"]])
    for row in range(r.shape[1]):
        assert (r[:, row] < B.HUBER_K).any() and (r[:, row] > B.HUBER_K).any(), f"row {row}"


@pytest.mark.parametrize("name,mode", [(n, m) for n, m in LIVE if B.SPECS[n]["tails"]])
def test_tails_carry_weight_and_show_in_the_metric(name, mode):
    """Every region of the case (a chunk's last round, the lane before a missing second point, the second points, the
    last pack tile and trip, the points after round 64) holds a weighted point on every edge, and losing one such
    point moves the fp64 truth by more than 8 rho_ref: twice the device's bound, so a kernel that drops or doubles
    the region cannot pass."""
    c = B.build(name)
    t = B.point_table(c, mode)
    ref = B.rho_ref(c, mode)
    R = B.regions(c)
    assert R
    for rname, mask in R.items():
        assert ((t["weighted"] & mask).sum(1) > 0).all(), rname
        s = B.sensitivity(c, mode, mask)
        print(f"{name} {mode} {rname}: {int(mask.sum())} points, one lost -> rho {s.min():.2e} (8 rho_ref {8 * ref:.2e})")
        assert (s > 8 * ref).all(), rname


def test_named_shapes_have_their_regions():
    n = {k: sorted(B.regions(B.build(k))) for k in B.SPECS}
    assert "second_points" not in n["n7"] and "second_points" not in n["n15"] and "second_points" not in n["n256"]
    assert B.regions(B.build("n257"))["second_points"].sum() == 1
    assert B.regions(B.build("n511"))["second_points"].sum() == 255
    assert B.regions(B.build("n511"))["chunk0.lane_before_missing_second"][255]
    assert B.regions(B.build("n512"))["second_points"].sum() == 256 and len(n["n512"]) == 2
    assert B.regions(B.build("n513"))["chunk0.last_round"].sum() == 1
    assert [B.chunk_ranges(B.build("n1300c5"))[k] for k in (0, 4)] == [(0, 260), (1040, 1300)]
    assert B.regions(B.build("n1300c5"))["second_points"].sum() == 20
    assert B.chunk_ranges(B.build("n1300c6"))[5] == (1085, 1300) and "second_points" not in n["n1300c6"]
    assert B.regions(B.build("n4100"))["last_pack_tile"].sum() == 4
    assert B.regions(B.build("n5123"))["last_pack_trip"].sum() == 3
    assert B.regions(B.build("n33000"))["after_round_64"].sum() == 33000 - 64 * 512
    assert "after_round_64" not in n["n5123"]


@pytest.mark.parametrize("name", ["C513", "C1300c5"])
def test_confidence_plants_decide(name):
    """C_thresh = 0.5: on every edge some points are rejected by c_i alone and some by c_j alone, on disjoint point sets
    per keyframe; every other confidence is >= 0.505. Zero-copy form (fusion counts 1, 3, 2): the plants of the count-3
    keyframe have sum 1.2 (average 0.4 < 0.5 < sum) and unplanted points of the count-2 keyframe have sum 1.2 (0.6), so
    a missing confidence scale accepts the first and the other keyframe's scale rejects the second."""
    c = B.build(name)
    src, tgt = c["planted"]["c_src"], c["planted"]["c_tgt"]
    assert not (src & tgt).any() and src.any(1).all() and tgt.any(1).all()
    assert (c["Cs"][~(src | tgt)] >= np.float32(0.505)).all() and (c["Cs"][src | tgt] <= np.float32(0.4)).all()
    for mode in B.MODES:
        t = B.point_table(c, mode)
        assert (B.only_fails(t, "c_i").sum(1) > 0).all() and (B.only_fails(t, "c_j").sum(1) > 0).all()
    n = np.array(B.NFUSE, np.float32)
    csum = c["Cs"] * n[:, None]
    assert (csum[1][src[1] | tgt[1]] > 0.5).all()
    plain = ~(src[2] | tgt[2]) & (c["Cs"][2] == np.float32(0.6))
    assert plain.any() and (csum[2][plain] * (np.float32(1) / n[1]) < 0.5).all()
    for k in range(3):   # the average the stacked form sees decides as the sum times 1 / count does
        assert np.array_equal(csum[k] / n[k] > np.float32(0.5), csum[k] * (np.float32(1) / n[k]) > np.float32(0.5))


@pytest.mark.parametrize("name", ["calib4100", "tum4100"])
def test_calib_plants_decide(name):
    """pixel_border = 2 rejects points on every edge that pass every other test, and no point that passes the others
    projects within 0.25 px of a border line. calib4100: so do the planted source depths (0, negative, just below
    z_eps) and the planted target points that land behind camera i. tum4100: fx != fy, principal point off centre."""
    c = B.build(name)
    t = B.point_table(c, "calib")
    assert (B.only_fails(t, "border").sum(1) > 0).all()
    rest = np.logical_and.reduce([v for k, v in t["tests"].items() if k != "border"])
    b = c["thresh"]["pixel_border"]
    for val, lines in ((t["u"], (b, c["W"] - 1 - b)), (t["v"], (b, c["H"] - 1 - b))):
        for line in lines:
            assert (np.abs(val[rest] - line) >= 0.25).all()
    if name == "calib4100":
        assert (B.only_fails(t, "z_i").sum(1) > 0).all() and (B.only_fails(t, "z_j").sum(1) > 0).all()
        z = c["X"][c["planted"]["depth"]][:, 2]
        assert (z == 0).any() and (z < 0).any() and ((z > 0) & (z < c["thresh"]["z_eps"])).any()
    else:
        K = c["K"]
        assert K[0, 0] != K[1, 1] and abs(K[0, 2] - c["W"] / 2) > 0.1 and abs(K[1, 2] - c["H"] / 2) > 0.1


def test_ids_are_not_ranks():
    c = B.build("ids513")
    assert sorted(set(c["ii"]) | set(c["jj"])) == [2, 5, 9] and c["Twc"].shape[0] == 3
    seen = list(dict.fromkeys(np.stack((c["ii"], c["jj"]), 1).reshape(-1).tolist()))
    assert seen != sorted(seen) and not np.array_equal(c["rank_i"], c["ii"])
    assert np.array_equal(np.array([2, 5, 9])[c["rank_i"]], c["ii"])
    assert np.array_equal(np.array([2, 5, 9])[c["rank_j"]], c["jj"])


@pytest.mark.parametrize("mode", ["points", "rays"])
def test_zero_residual_case_is_exactly_zero(mode):
    """Two bit-identical keyframes, every pixel matched to itself: g and chi2 are exactly 0 in the fp64 truth and in
    both orders of the fp32 restatement, M is not."""
    c = B.build("zero513")
    assert np.array_equal(c["Twc"][0], c["Twc"][1]) and np.array_equal(c["X"][0], c["X"][1])
    assert np.abs(c["Twc"][0] - np.array([0, 0, 0, 0, 0, 0, 1, 1])).max() > 0.5 and c["Twc"][0, 7] != 1
    row, chi2 = B.truth(c, mode)
    assert not chi2.any() and not row[:, 28:35].any() and (row[:, B.DIAG] > 0).all()
    for r in B.refs32(c, mode):
        assert not r[:, 28:35].any()
