"""CPU: pin the oracle (tests' checker) against the golden vectors produced by the reference's own
Python glue (tests/golden/make_golden.py). These tests never touch the product path."""
import numpy as np
import pytest

import oracle.oracle as O


def test_half_conversion_matches_ieee_rne():
    rng = np.random.default_rng(0)
    vals = np.concatenate([
        rng.standard_normal(200000).astype(np.float32),
        (rng.standard_normal(100000) * 1e-5).astype(np.float32),  # f16 subnormal range
        (rng.standard_normal(50000) * 3e4).astype(np.float32),  # near overflow
        np.array([0.0, -0.0, 65504.0, 65520.0, 65519.99, 2 ** -24, 2 ** -25, 2 ** -25 * 1.0001, np.inf, -np.inf],
                 np.float32),
    ])
    ours = O.to_half_bits(vals)
    with np.errstate(over="ignore"):
        ref = vals.astype(np.float16).view(np.uint16)
    assert np.array_equal(ours, ref)


def test_prep_restatement_matches_reference(golden):
    g = golden("matching_48x64.npz")
    rays, pts, p_init = O.prep_for_iter_proj(g["X11"], g["X21"], None)
    # bit for bit: torch's CPU vector_norm / depthwise conv2d order (FMA chains, m3s_oracle.c m3o_normalize3 /
    # m3o_img_gradient)
    np.testing.assert_array_equal(rays, g["rays"])
    np.testing.assert_array_equal(pts, g["pts"])
    np.testing.assert_array_equal(p_init, g["p_init"])


def test_iter_proj_oracle_on_reference_prep(golden):
    g = golden("matching_48x64.npz")
    p, c = O.iter_proj(g["rays"], g["pts"], g["p_init"], 10, 1e-8, 1e-6)
    np.testing.assert_array_equal(p, g["p_new"])
    np.testing.assert_array_equal(c, g["converged"])


def test_match_glue_restatement_matches_reference(golden):
    g = golden("matching_48x64.npz")
    idx, valid = O.match(g["X11"], g["X21"], g["D11"], g["D21"])
    # reference glue + oracle kernels vs the restated glue + oracle kernels: bit for bit (the prep is pinned above)
    np.testing.assert_array_equal(idx, g["idx"])
    np.testing.assert_array_equal(valid, g["valid"])
    idx_w, valid_w = O.match(g["X11"], g["X21"], g["D11"], g["D21"], g["idx_init"])
    np.testing.assert_array_equal(idx_w, g["idx_warm"])
    np.testing.assert_array_equal(valid_w, g["valid_warm"])


def test_refine_half_emulation_properties(golden):
    g = golden("matching_48x64.npz")
    p1 = np.stack((g["p_new"][..., 0].astype(np.int64), g["p_new"][..., 1].astype(np.int64)), -1)
    h = O.refine_matches(g["D11h"], O.to_half_bits(g["D21"].reshape(1, -1, 24)), p1, 3, 5)
    f = O.refine_matches(g["D11"], g["D21"].reshape(1, -1, 24), p1, 3, 5, half=False)
    # fp16 step rounding vs fp32: same winner almost everywhere, never outside the image
    assert (h != f).any(-1).mean() < 0.05
    assert h[..., 0].min() >= 0 and h[..., 0].max() < 64 and h[..., 1].min() >= 0 and h[..., 1].max() < 48
    # radius 0 / dilation 0 is the identity
    np.testing.assert_array_equal(O.refine_matches(g["D11h"], O.to_half_bits(g["D21"].reshape(1, -1, 24)), p1, 0, 5), p1)


@pytest.mark.parametrize("mode", ["rays", "calib"])
def test_tracker_restatement_matches_reference(golden, mode):
    g = golden("optpose_32x48.npz")
    H, W = 32, 48
    if mode == "rays":
        Tf, Tr, _ = O.track_rays(g["Xf"], g["Xk"], g["T_WCf"][0], g["T_WCk"][0], g["Qk"], g["valid"])
    else:
        Tf, Tr, _ = O.track_calib(g["Xf_c"], g["Xk"], g["T_WCf"][0], g["T_WCk"][0], g["Qk"], g["valid"], g["meas"],
                                  g["vmeas"], g["K"], (H, W))
    # the pose contract (1e-5); measured 1.4e-6 (rays) and 1.0e-7 (calib) against the reference run's poses
    np.testing.assert_allclose(Tf, g[f"{mode}_T_WCf"][0], atol=1e-5)
    np.testing.assert_allclose(Tr, g[f"{mode}_T_CkCf"][0], atol=1e-5)


@pytest.mark.parametrize("mode", ["points", "rays", "calib"])
def test_ba_rows_match_reference_geometry(golden, mode):
    """Oracle BA residual/Jacobian/weights vs H, g built from the reference's geometry.py."""
    g = golden("ba_rows.npz")
    Xs = g["Xs"]
    N = Xs.shape[1]
    Twc = np.stack((np.array([0, 0, 0, 0, 0, 0, 1, 1], np.float32), g["Tj"]))
    sig = {"points": (0.05, 0.0), "rays": (0.003, 10.0), "calib": (1.0, 10.0)}[mode]
    p = O.ba_params(mode, sig[0], sig[1], 0.0, 1.5, K=g["K"], height=int(g["H"]), width=int(g["W"]),
                    pixel_border=-10, z_eps=1e-6)
    Cs = np.full((2, N), 2.0, np.float32)
    Hs, gs = O.ba_linearize(mode, Twc, Xs, Cs, np.array([0]), np.array([1]), g["idx"][None], g["valid"][None],
                            g["q"][None], p)
    Href, gref = g[f"{mode}_H"], g[f"{mode}_g"]
    scale = np.abs(Href).max()
    np.testing.assert_allclose(Hs[3, 0], Href, rtol=0, atol=2e-5 * scale)  # H_jj (adjoint = I)
    np.testing.assert_allclose(Hs[0, 0], Href, rtol=0, atol=2e-5 * scale)  # H_ii = H_jj
    np.testing.assert_allclose(Hs[1, 0], -Href, rtol=0, atol=2e-5 * scale)  # H_ij = -H_jj
    gsc = np.abs(gref).max()
    np.testing.assert_allclose(gs[1, 0], gref, rtol=0, atol=2e-5 * gsc)
    np.testing.assert_allclose(gs[0, 0], -gref, rtol=0, atol=2e-5 * gsc)


@pytest.mark.parametrize("mode", ["rays", "calib"])
def test_oracle_ba_reproduces_reference_factor_graph(golden, mode):
    """Reference FactorGraph.solve_GN_* (two-way edges, pin, write-back) driving the oracle backend."""
    g = golden("ba_6kf_24x32.npz")
    sig = (0.003, 10.0) if mode == "rays" else (1.0, 10.0)
    Xs = g["Xs"]
    H, W = 24, 32
    if mode == "calib":
        Xs = O.backproject_constrain(Xs, g["K"], (H, W))
    p = O.ba_params(mode, sig[0], sig[1], 0.0, 1.5, K=g["K"], height=H, width=W, pixel_border=-10, z_eps=1e-6)
    ii = np.concatenate((g["ii"], g["jj"]))
    jj = np.concatenate((g["jj"], g["ii"]))
    T, dx, its = O.gauss_newton(mode, g["Twc0"], Xs, g["Cs"][..., 0], ii, jj, g["idx2"], g["valid2"][..., 0],
                                g["Q2"][..., 0], p, 10, 1e-8)
    np.testing.assert_allclose(T, g[f"{mode}_Twc"], atol=1e-5)


@pytest.mark.parametrize("mode", ["rays", "calib"])
def test_reference_order_fp32_within_1e5_of_fp64_truth(golden, mode):
    """SURVEY §8 a-note 6: the reference's fp32 per-point order (golden, via the reference glue) sits
    within 1e-5 of the fp64 truth of the same algorithm (oracle/Makefile F64 build)."""
    g = golden("ba_6kf_24x32.npz")
    sig = (0.003, 10.0) if mode == "rays" else (1.0, 10.0)
    H, W = 24, 32
    Xs = g["Xs"] if mode == "rays" else O.backproject_constrain(g["Xs"], g["K"], (H, W))
    p = O.ba_params(mode, sig[0], sig[1], 0.0, 1.5, K=g["K"], height=H, width=W, pixel_border=-10, z_eps=1e-6)
    ii = np.concatenate((g["ii"], g["jj"]))
    jj = np.concatenate((g["jj"], g["ii"]))
    T64, _, its = O.gauss_newton_f64(mode, g["Twc0"], Xs, g["Cs"][..., 0], ii, jj, g["idx2"], g["valid2"][..., 0],
                                     g["Q2"][..., 0], p, 10, 1e-8)
    assert its == 10
    np.testing.assert_allclose(g[f"{mode}_Twc"], T64, atol=1e-5)


@pytest.mark.parametrize("mode", ["rays", "calib"])
def test_reference_sum_order_mode(golden, mode):
    """oracle set_ref_order(1): the BA sums in the reference kernels' own fp32 order (256 per-thread float
    accumulators + the float blockReduce tree, gn_kernels.cu:36-55, 531-723): on the 6-KF fixture (768-point edges,
    three points per thread) it stays close to the default fp64-sum mode and is a different order (not
    bit-identical); the full-size C4 comparison it exists for is in DESIGN.md §2."""
    g = golden("ba_6kf_24x32.npz")
    sig = (0.003, 10.0) if mode == "rays" else (1.0, 10.0)
    H, W = 24, 32
    Xs = g["Xs"] if mode == "rays" else O.backproject_constrain(g["Xs"], g["K"], (H, W))
    p = O.ba_params(mode, sig[0], sig[1], 0.0, 1.5, K=g["K"], height=H, width=W, pixel_border=-10, z_eps=1e-6)
    ii = np.concatenate((g["ii"], g["jj"]))
    jj = np.concatenate((g["jj"], g["ii"]))
    args = (g["Twc0"], Xs, g["Cs"][..., 0], ii, jj, g["idx2"], g["valid2"][..., 0], g["Q2"][..., 0], p, 10, 1e-8)
    T_def, _, _ = O.gauss_newton(mode, *args)
    O.set_ref_order(1)
    try:
        T_ref, _, _ = O.gauss_newton(mode, *args)
    finally:
        O.set_ref_order(0)
    # two fp32 sum orders on this ill-conditioned fixture: 3e-5, as the suite's other fp32-vs-fp32 pose checks
    np.testing.assert_allclose(T_ref, T_def, atol=3e-5)
    assert not np.array_equal(T_ref, T_def)


def test_oracle_ba_converges_on_consistent_problem():
    rng = np.random.default_rng(0)
    N = 1024
    Xj = rng.standard_normal((N, 3)).astype(np.float32) * 0.5 + np.array([0, 0, 3.0], np.float32)
    Tj = np.array([0.2, -0.1, 0.3, 0.0, 0.1494381, 0.0, 0.9887711, 1.1], np.float32)
    Xi = np.zeros_like(Xj)
    perm = rng.permutation(N)
    Xi[perm] = np.stack([O.sim3_act(Tj.astype(np.float64), Xj[k].astype(np.float64)) for k in range(N)])
    inv = np.empty(N, np.int64)
    inv[perm] = np.arange(N)
    Twc_gt = np.stack((np.array([0, 0, 0, 0, 0, 0, 1, 1], np.float32), Tj))
    Twc0 = Twc_gt.copy()
    Twc0[1, :3] += [0.03, -0.02, 0.01]
    Twc0[1, 7] *= 1.03
    for mode, sa, sb in (("points", 0.05, 0.0), ("rays", 0.003, 10.0)):
        T, dx, its = O.gauss_newton(mode, Twc0, np.stack((Xi, Xj)), np.full((2, N), 2.0, np.float32),
                                    np.array([0, 1]), np.array([1, 0]), np.stack((perm, inv)),
                                    np.ones((2, N), np.uint8), np.full((2, N), 2.0, np.float32),
                                    O.ba_params(mode, sa, sb), 10, 1e-8)
        np.testing.assert_allclose(T, Twc_gt, atol=2e-6)


@pytest.mark.parametrize("cfg", ["C1", "C2"])
def test_match_restatement_matches_reference_at_config_size(golden, cfg):
    """Bit for bit at the BASELINE config sizes (512x512 C1, 384x512 TUM-shaped C2): the reference run's prep
    (rays, pts) and its full match (its torch glue + the oracle's kernels), stored as sha256 digests by
    tests/golden/make_golden.py gen_match_digest, against the oracle's restated glue on the same regenerated pair.
    The GPU config tests then hold the HIP match to the oracle bit for bit on the same pairs."""
    import hashlib

    from m3s.synthetic import make_pair, tum_fr1_intrinsics

    g = golden("match_digest.npz")
    H, W = (int(v) for v in g[f"{cfg}_shape"])
    P = make_pair(H, W, seed=11, K=tum_fr1_intrinsics(H, W) if cfg == "C2" else None)
    X, D = P["X"].numpy(), P["D"].numpy()
    rays, pts, _ = O.prep_for_iter_proj(X[:1], X[1:], None)
    np.testing.assert_array_equal(rays[0, 0], g[f"{cfg}_rays_row0"])
    idx, valid = O.match(X[:1], X[1:], D[:1], D[1:])
    dig = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    for k, v in (("rays", rays), ("pts", pts), ("idx", idx), ("valid", valid)):
        assert dig(v) == str(g[f"{cfg}_{k}_sha256"]), f"{cfg} {k} differs from the reference run"


def test_batched_warm_match_restatement_matches_reference(golden):
    """C3w: a batch of two TUM-shaped 384x512 pairs matched from a warm start with out-of-range entries
    (synthetic.make_warm_batch), the batched call of global_opt's loop-closure matching: the oracle's prep (rays,
    pts, p_init from idx_init) and match equal the reference run's bytes (gen_match_digest's C3w digests)."""
    import hashlib

    from m3s.synthetic import make_warm_batch, tum_fr1_intrinsics

    g = golden("match_digest.npz")
    H, W = (int(v) for v in g["C3w_shape"])
    X11, X21, D11, D21, init = (t.numpy() for t in make_warm_batch(H, W, (21, 22), K=tum_fr1_intrinsics(H, W)))
    rays, pts, p_init = O.prep_for_iter_proj(X11, X21, init)
    np.testing.assert_array_equal(rays[0, 0], g["C3w_rays_row0"])
    idx, valid = O.match(X11, X21, D11, D21, init)
    dig = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    for k, v in (("rays", rays), ("pts", pts), ("p_init", p_init), ("idx", idx), ("valid", valid)):
        assert dig(v) == str(g[f"C3w_{k}_sha256"]), f"C3w {k} differs from the reference run"


@pytest.mark.parametrize("case", ["S1", "S2"])
def test_track_sequence_restatement_matches_reference(golden, case):
    """Three frames tracked in sequence against one keyframe at the bench's shape (512x512, the bench's pairs,
    idx_f2k warm start, each frame starting at the previous pose, weighted_pointmap fusion accumulating); S1 calib
    (the headline mode), S2 rays. The oracle chain (tests/track_chain.py oracle_track_seq) against the reference's
    own FrameTracker.track run (gen_track_seq): GN step counts and new_kf equal, poses and the fused keyframe
    within the 1e-5 contract."""
    from m3s.synthetic import make_pair
    from track_chain import oracle_track_seq

    g = golden("track_seq.npz")
    H, W = (int(v) for v in g[f"{case}_shape"])
    pairs = [make_pair(H, W, seed=int(s)) for s in g[f"{case}_seeds"]]
    frames, kX, kC, kN = oracle_track_seq(pairs, H, W, "calib" if bool(g[f"{case}_calib"]) else "rays")
    sub = g[f"{case}_sub"]
    for k, (Tf, it, new_kf) in enumerate(frames):
        print(f"{case} frame {k}: pose err vs the reference run {np.abs(Tf - g[f'{case}_f{k}_T_WCf'][0]).max():.2e}, "
              f"iters {it} / {int(g[f'{case}_f{k}_iters'])}")
        assert it == int(g[f"{case}_f{k}_iters"]) and new_kf == bool(g[f"{case}_f{k}_new_kf"])
        np.testing.assert_allclose(Tf, g[f"{case}_f{k}_T_WCf"][0], atol=1e-5)
    assert kN == int(g[f"{case}_kf_N"])
    np.testing.assert_allclose(kX[sub], g[f"{case}_kf_X_sub"], atol=1e-5, rtol=1e-5)
    np.testing.assert_allclose(kC[sub], g[f"{case}_kf_C_sub"][:, 0], rtol=1e-6)


@pytest.mark.parametrize("case", ["C1_rays", "C1_calib", "C2_calib"])
def test_track_restatement_matches_reference_at_config_size(golden, case):
    """The oracle's tracker chain (tests/track_chain.py: O.match, fp64 opt_pose_*, weighted_pointmap fusion) against
    the reference's own FrameTracker.track run at the config sizes (tests/golden/make_golden.py gen_track_config:
    its torch glue and fp32 GN on the same pair): the same GN step count and new_kf decision, the frame pose within
    the 1e-5 contract, the fused keyframe points (every 997th) within 1e-5 absolute + relative."""
    from m3s.synthetic import make_pair, tum_fr1_intrinsics
    from track_chain import oracle_track

    g = golden("track_config.npz")
    H, W = (int(v) for v in g[f"{case}_shape"])
    mode = "rays" if case.endswith("rays") else "calib"
    P = make_pair(H, W, seed=11, K=tum_fr1_intrinsics(H, W) if case.startswith("C2") else None)
    _, _, Tf, kX, it = oracle_track(P, mode, H, W)
    print(f"{case}: pose err vs the reference run {np.abs(Tf - g[f'{case}_T_WCf'][0]).max():.2e}, "
          f"kf X err {np.abs(kX[g[f'{case}_sub']] - g[f'{case}_kf_X_sub']).max():.2e}, iters {it} / {g[f'{case}_iters']}")
    assert it == int(g[f"{case}_iters"])
    np.testing.assert_allclose(Tf, g[f"{case}_T_WCf"][0], atol=1e-5)
    np.testing.assert_allclose(kX[g[f"{case}_sub"]], g[f"{case}_kf_X_sub"], atol=1e-5, rtol=1e-5)


def test_ba_chi2_bounds_the_gradient(golden):
    """m3o_ba_linearize_chi2 (both builds, both orders of the fp32 one): per edge chi2 = sum w e^2 bounds the gradient,
    chi2 >= g_a^2 / M_aa for every a (Cauchy-Schwarz: g_a = sum w e J_a, M_aa = sum w J_a^2), and is exactly 0 on an
    edge with no weighted point. Hs and gs are those of m3o_ba_linearize, bit for bit. The sums the inequality holds
    for exactly are of real products; each stored product carries one rounding of its format, hence the slack of a
    few roundings (1e-6 fp32, 1e-14 fp64) on edges whose rows are far from parallel."""
    g = golden("ba_6kf_24x32.npz")
    H, W = 24, 32
    ii, jj = np.concatenate((g["ii"], g["jj"])), np.concatenate((g["jj"], g["ii"]))
    valid = g["valid2"][..., 0].copy()
    valid[3] = False    # an edge with no weighted point
    sig = {"points": (0.05, 0.0), "rays": (0.003, 10.0), "calib": (1.0, 10.0)}
    for mode in ("points", "rays", "calib"):
        Xs = O.backproject_constrain(g["Xs"], g["K"], (H, W)) if mode == "calib" else g["Xs"]
        p = O.ba_params(mode, *sig[mode], 0.0, 1.5, K=g["K"], height=H, width=W, pixel_border=-10, z_eps=1e-6)
        args = (mode, g["Twc0"], Xs, g["Cs"][..., 0], ii, jj, g["idx2"], valid, g["Q2"][..., 0], p)
        outs = [(O.ba_linearize_chi2_f64(*args), 1e-14)]
        for order in (0, 1):
            O.set_ref_order(order)
            try:
                Hs, gs = O.ba_linearize(*args)
                out = O.ba_linearize_chi2(*args)
            finally:
                O.set_ref_order(0)
            assert np.array_equal(out[0], Hs) and np.array_equal(out[1], gs)
            outs.append((out, 1e-6))
        weighted = 0
        for (Hs, gs, chi2), slack in outs:
            assert chi2.shape == (ii.shape[0],) and chi2[3] == 0.0 and not Hs[:, 3].any() and not gs[:, 3].any()
            M, gv = Hs[3], gs[1]
            for e in np.flatnonzero(chi2 > 0):
                d = np.diagonal(M[e])
                assert (d > 0).all()
                assert (chi2[e] * (1 + slack) >= gv[e] ** 2 / d).all(), (mode, e)
            weighted = int((chi2 > 0).sum())
        assert weighted >= 10
