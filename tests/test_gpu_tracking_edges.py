"""GPU: the tracking kernels (csrc/track.hip) against the fp64 reference at ragged sizes and with invalid points.

The cases, their builders and references are in tests/track_edge_cases.py; tests/test_tracking_edges_host.py checks on
the CPU that they reach the branches they are meant to reach and are well conditioned. Which shape reaches which
code path: DESIGN.md, tracking, "edge shapes".

Tolerances: poses 1e-5 absolute against the fp64 reference (the project's contract, BASELINE.json north_star; it is a
statement about the kernels because the inputs' own rounding moves the reference by < 1e-6, host test); fused points
atol 1e-5 + rtol 1e-5 (tests/test_gpu_tracking.py); counts, status, iterations, C and the average confidences exact.

Measured on an MI355X (max |pose - reference| over T_WCf and T_CkCf, printed by every test; rays / calib):

  direct, 1 iteration     N=7 1.2e-6 | 63 2.6e-7 / 1.5e-6 | 255 3.0e-7 / 1.0e-6 | 259 2.6e-7 / 1.8e-7 |
                          1023 3.9e-7 / 2.9e-7 | 1025 4.0e-7 / 6.1e-7 | 9595 2.6e-7 / 3.3e-7 | 57360 3.2e-7 / 1.5e-7 |
                          263171 4.5e-7 (rays) | 263165 2.3e-7 (calib)
  direct, 4 iterations    N=7 5.0e-7 | 63 2.2e-7 / 1.4e-7 | 255 9.2e-8 / 9.4e-8 | 259 9.0e-8 / 6.4e-8 |
  (3 at N ~ 263k)         1023 5.2e-8 / 1.3e-7 | 1025 6.0e-8 / 5.9e-8 | 9595 1.3e-7 / 1.1e-7 | 57360 6.5e-8 / 5.3e-8 |
                          263171 7.2e-8 (rays) | 263165 2.1e-7 (calib)
  direct, 50 iterations   N=1025 rays 5.7e-8
  direct to convergence   255 9.2e-8 / 7.6e-8 | 1025 7.3e-8 / 5.9e-8 | 9595 8.5e-8 / 1.2e-7 (iterations as the reference)
  matched (pose; fused X relative)
                          15x17 5.6e-8; 1.4e-7 / 1.1e-7; 1.4e-7 | 25x41 1.8e-7; 1.8e-7 / 1.3e-7; 1.9e-7 |
                          95x101 1.1e-7; 2.3e-7 / 3.4e-7; 1.7e-7 | 239x240 calib 6.6e-8; 2.2e-7 |
                          515x511 rays 1.2e-7; 3.3e-7
  skip boundary, 52 points 1.7e-7

Before gn_pair masked the structurally zero scale column of the ray and pixel rows, this suite measured
2.3e-5 at rays N = 63 and at matched rays 15x17, 9.3e-6 at rays N = 259 and 7.6e-6 at rays N = 1023.

Mutation check (by hand, not committed): the lone-point branch of gn_accumulate's ``pair`` keeping the duplicate's
weight turned 30 of these tests red, ``n16 = N / 16`` in gn_prologue 13, and gn_pair without its ``a1.z != 0`` term 23.
"""
import numpy as np
import pytest
import torch

import track_edge_cases as E

pytestmark = pytest.mark.gpu

STATUS = {1: "ok", 2: "max_iters", 3: "cholesky", 4: "skipped"}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cfg(**kw):
    from m3s.config import config

    config["tracking"].update(kw)


def _run_direct(c, **cfg):
    """opt_pose_* on a direct case -> (T_WCf, T_CkCf (8,) float32 arrays, the TrackResult)."""
    from m3s.sim3 import Sim3
    from m3s.tracker import FrameTracker

    _cfg(**cfg)
    tr = FrameTracker(None, None, "cuda")
    Tf0, Tk = Sim3(_cuda(c["T_WCf"]).view(1, 8)), Sim3(_cuda(c["T_WCk"]).view(1, 8))
    Xf, Xk, Qk, valid = _cuda(c["Xf"]), _cuda(c["Xk"]), _cuda(c["Qk"]), _cuda(c["valid"])
    if c["mode"] == "rays":
        Tf, Tr = tr.opt_pose_ray_dist_sim3(Xf, Xk, Tf0, Tk, Qk, valid)
    else:
        Tf, Tr = tr.opt_pose_calib_sim3(Xf, Xk, Tf0, Tk, Qk, valid, _cuda(c["meas"]), _cuda(c["vmeas"]), _cuda(c["K"]),
                                        c["img_size"])
    return Tf.data.cpu().numpy().reshape(8), Tr.data.cpu().numpy().reshape(8), tr.last_result


def _pose_err(Tf, Tr, rf, rr):
    return max(float(np.abs(Tf - rf).max()), float(np.abs(Tr - rr).max()))


def _run_matched(c, monkeypatch, **cfg):
    """FrameTracker.track on a matched case, the matcher replaced by the case's matches. Returns a dict: the return
    triple, the TrackResult, the frame's pose, and the keyframe after the call."""
    import m3s.tracker as T
    from m3s.config import config
    from m3s.frame import Frame, Keyframes
    from m3s.sim3 import Sim3

    config["use_calib"] = c["mode"] == "calib"
    _cfg(**dict(E.matched_cfg(c["mode"]), **cfg))
    H, W = c["img_size"]
    kf = Frame(0, (H, W), T_WC=Sim3(_cuda(c["T_WCk"]).view(1, 8)))
    kf.K = _cuda(c["K"])
    kf.X_canon, kf.C, kf.N, kf.N_updates = _cuda(c["kf_X"]), _cuda(c["kf_C"]).view(-1, 1), c["kf_N"], c["kf_N"]
    kfs = Keyframes()
    kfs.append(kf)
    frame = Frame(1, (H, W), T_WC=Sim3(_cuda(c["T_WCf"]).view(1, 8)))
    col = lambda k: _cuda(c[k]).view(-1, 1)
    ret = (_cuda(c["idx"])[None], _cuda(c["valid_match"]).view(1, -1, 1), _cuda(c["Xff"]), col("Cff"), col("Qff"),
           _cuda(c["Xkf"]), col("Ckf"), col("Qkf"))
    monkeypatch.setattr(T, "mast3r_match_asymmetric", lambda *a, **k: ret)
    tr = T.FrameTracker(None, kfs, "cuda")
    new_kf, info, reloc = tr.track(frame)
    r = tr.last_result
    return {"new_kf": new_kf, "info": info, "reloc": reloc, "res": r, "T_WCf": frame.T_WC.data.cpu().numpy().reshape(8),
            "T_CkCf": np.array(list(r.T_CkCf), np.float32), "kf": kf, "X": kf.X_canon.cpu().numpy(),
            "C": kf.C.cpu().numpy().reshape(-1),
            "bits": (bool(new_kf), bool(reloc), list(r.T_WCf), list(r.T_CkCf), r.cost, r.iters, r.status, r.n_valid_opt,
                     r.n_valid_kf, r.n_unique, kf.X_canon.cpu().numpy().tobytes(), kf.C.cpu().numpy().tobytes())}


def _check_counts(g, ref):
    r = g["res"]
    assert (STATUS[r.status], r.iters, r.n_valid_opt, r.n_valid_kf, r.n_unique) == (
        ref["status"], ref["iters"], ref["n_valid_opt"], ref["n_valid_kf"], ref["n_unique"])


def _grid_note(N):
    """The GN grid the launcher takes for N points (csrc/abi_track.cpp: ceil(N / 1024) blocks, at most 256 and at
    most the resident blocks), printed so the record shows which path ran."""
    from m3s import _lib

    mp = int(_lib.load().m3s_track_max_parts())
    return f"max_parts {mp}, nparts {min(mp, min(256, (N + 1023) // 1024))}"


FIXED = [pytest.param(m, n, s, it, id=f"{m}-{n}-it{it}") for m, n, s in E.direct_cases()
         for it in ((1, 3) if n in E.BIG else (1, 4))] + [pytest.param("rays", 1025, (1, 1025), 50, id="rays-1025-it50")]


@pytest.mark.parametrize("mode,N,shape,iters", FIXED)
def test_direct_fixed_iterations(mode, N, shape, iters):
    """opt_pose_* with both convergence thresholds zero runs exactly max_iters steps; against the reference's
    fixed_iters of the same value, so no threshold coincidence enters. max_iters = 1: one linearisation and solve."""
    seed = E.seed_of("direct", mode, N)
    c = E.build_direct(mode, *shape, seed)
    rf, rr, _, _ = E.ref_direct_cached(mode, *shape, seed, iters)
    Tf, Tr, res = _run_direct(c, rel_error=0.0, delta_norm=0.0, max_iters=iters)
    print(f"direct fixed {mode} N={N} iters={iters}: pose err {_pose_err(Tf, Tr, rf, rr):.2e} ({_grid_note(N)})")
    assert res.iters == iters and STATUS[res.status] == "max_iters"
    np.testing.assert_allclose(Tf, rf, atol=1e-5)
    np.testing.assert_allclose(Tr, rr, atol=1e-5)


@pytest.mark.parametrize("mode,N", [(m, n) for n in E.CONVERGE_N for m in ("rays", "calib")])
def test_direct_to_convergence(mode, N):
    """Default thresholds: the same number of iterations as the reference (its steps keep the convergence margin,
    host test) and the same poses."""
    shape = E.SHAPES[N][0 if mode == "rays" else 1]
    seed = E.seed_of("direct", mode, N)
    c = E.build_direct(mode, *shape, seed)
    rf, rr, rit, _ = E.ref_direct_cached(mode, *shape, seed, None)
    Tf, Tr, res = _run_direct(c)
    print(f"direct converge {mode} N={N}: iters {res.iters} / {rit}, pose err {_pose_err(Tf, Tr, rf, rr):.2e}")
    assert res.iters == rit and STATUS[res.status] == "ok"
    np.testing.assert_allclose(Tf, rf, atol=1e-5)
    np.testing.assert_allclose(Tr, rr, atol=1e-5)


def _matched(mode, shape):
    N = shape[0] * shape[1]
    seed = E.seed_of("matched", mode, N)
    fixed = 3 if N in E.BIG else None
    cfg = {} if fixed is None else {"rel_error": 0.0, "delta_norm": 0.0, "max_iters": fixed}
    return E.build_matched(mode, *shape, seed), E.ref_matched_cached(mode, *shape, seed, fixed)[0], cfg


@pytest.mark.parametrize("mode,shape", [pytest.param(m, s, id=f"{m}-{s[0]}x{s[1]}") for m, s in E.MATCHED])
def test_matched_track(monkeypatch, mode, shape):
    """FrameTracker.track on crafted matches (duplicates, marks in the last map entry, wrong matches, points behind
    the camera, invalid keyframe depths, confidences on both sides of C_conf and Q_conf) against
    oracle_track_from_matches."""
    c, ref, cfg = _matched(mode, shape)
    g = _run_matched(c, monkeypatch, **cfg)
    err = _pose_err(g["T_WCf"], g["T_CkCf"], ref["T_WCf"], ref["T_CkCf"])
    xerr = float((np.abs(g["X"] - ref["X"]) / (1.0 + np.abs(ref["X"]))).max())
    print(f"matched {mode} {shape}: {STATUS[g['res'].status]} in {g['res'].iters} / {ref['iters']}, counts "
          f"{g['res'].n_valid_opt} {g['res'].n_valid_kf} {g['res'].n_unique}, pose err {err:.2e}, fused X err "
          f"{xerr:.2e} ({_grid_note(c['N'])})")
    assert (bool(g["new_kf"]), len(g["info"]), bool(g["reloc"])) == (ref["new_kf"], 6, False)
    _check_counts(g, ref)
    np.testing.assert_allclose(g["T_WCf"], ref["T_WCf"], atol=1e-5)
    np.testing.assert_allclose(g["T_CkCf"], ref["T_CkCf"], atol=1e-5)
    np.testing.assert_allclose(g["X"], ref["X"], atol=1e-5, rtol=1e-5)
    assert np.array_equal(g["C"], ref["C"])
    assert np.array_equal(g["info"][1].cpu().numpy().reshape(-1), ref["Ck_avg"])
    assert np.array_equal(g["info"][3].cpu().numpy().reshape(-1), ref["Cf_avg"])
    assert g["kf"].N == c["kf_N"] + 1


@pytest.mark.parametrize("publish_gn", ["1", "0"])
def test_skip_boundary_and_next_frame(monkeypatch, publish_gn):
    """25x41, min_match_frac 0.05: 52 valid-opt points (0.0507) are tracked, 51 (0.0498) return (False, [], True)
    and leave the keyframe alone; the skipped frame marked the unique-match map (hundreds of valid matches), and the
    next normal frame on the same workspace reports the exact n_unique."""
    monkeypatch.setenv("M3S_TRACK_PUBLISH_GN", publish_gn)
    c52, c51 = E.skip_case(52), E.skip_case(51)
    ref = E.ref_matched(c52)
    g = _run_matched(c52, monkeypatch)
    assert not g["reloc"] and g["res"].n_valid_opt == 52
    _check_counts(g, ref)
    print(f"skip boundary publish_gn={publish_gn}: 52 points tracked, pose err "
          f"{_pose_err(g['T_WCf'], g['T_CkCf'], ref['T_WCf'], ref['T_CkCf']):.2e}")
    np.testing.assert_allclose(g["T_WCf"], ref["T_WCf"], atol=1e-5)
    g = _run_matched(c51, monkeypatch)
    assert (g["new_kf"], g["info"], g["reloc"]) == (False, [], True)
    assert STATUS[g["res"].status] == "skipped" and g["res"].n_valid_opt == 51
    assert np.array_equal(g["X"], c51["kf_X"]) and np.array_equal(g["C"], c51["kf_C"]) and g["kf"].N == c51["kf_N"]
    c, ref, _ = _matched("rays", (25, 41))
    g = _run_matched(c, monkeypatch)
    _check_counts(g, ref)
    np.testing.assert_allclose(g["T_WCf"], ref["T_WCf"], atol=1e-5)


VARIANTS = (("1", "1"), ("1", "0"), ("0", "1"))  # (M3S_TRACK_FOLD_SETUP, M3S_TRACK_PUBLISH_GN)


@pytest.mark.parametrize("kind,mode,shape", [pytest.param("matched", m, s, id=f"matched-{m}-{s[0]}x{s[1]}")
                                             for s in ((25, 41), (95, 101)) for m in ("rays", "calib")] +
                         [pytest.param("direct", "rays", (1, 1025), id="direct-rays-1025"),
                          pytest.param("direct", "calib", (25, 41), id="direct-calib-1025")])
def test_launch_variants_bit_identical(monkeypatch, kind, mode, shape):
    """Folded setup with the publish in the GN launch (the default), with the publish in the fuse launch, and the
    separate setup launch give the same bits at ragged sizes: poses, cost, iterations, status, the three counts,
    fused X and C."""
    from m3s.config import reset_config

    outs = []
    for fold, pub in VARIANTS:
        monkeypatch.setenv("M3S_TRACK_FOLD_SETUP", fold)
        monkeypatch.setenv("M3S_TRACK_PUBLISH_GN", pub)
        reset_config()
        if kind == "matched":
            c, _, cfg = _matched(mode, shape)
            outs.append(_run_matched(c, monkeypatch, **cfg)["bits"])
        else:
            _, _, r = _run_direct(E.build_direct(mode, *shape, E.seed_of("direct", mode, 1025)))
            outs.append((list(r.T_WCf), list(r.T_CkCf), r.cost, r.iters, r.status, r.n_valid_opt, r.n_valid_kf))
    assert outs[0] == outs[1], "publish in the fuse launch differs"
    assert outs[0] == outs[2], "separate setup differs"


def test_workspace_reuse_across_ragged_sizes(monkeypatch):
    """95x101, then 25x41, then 95x101 on one tracker workspace (its scratch is laid out per image size): the first and
    the third result are bit-identical and all three have the reference's counts."""
    big, small = _matched("calib", (95, 101)), _matched("rays", (25, 41))
    outs = []
    for c, ref, cfg in (big, small, big):
        from m3s.config import reset_config

        reset_config()
        g = _run_matched(c, monkeypatch, **cfg)
        _check_counts(g, ref)
        outs.append(g["bits"])
    assert outs[0] == outs[2]
