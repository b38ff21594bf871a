"""GPU: the raw-calib BA mode (m3s_ba_config.mode = 3) and the zero-copy solve_GN_calib built on it.

Mode 3 reads the keyframes' raw X_canon and constrains X_j to its pixel ray in the kernels; it must give the poses
of mode 2 on constrain_points_to_ray(points) bit for bit. The points of make_graph and of the golden fixture already
lie exactly on their pixel rays, so every test first moves x and y off them (a kernel that ignored the constraint
would otherwise pass) and asserts that it did.
"""
import ctypes

import numpy as np
import pytest
import torch

import oracle.oracle as O

pytestmark = pytest.mark.gpu

NFUSE = [1, 3, 2, 7, 1, 5]  # fusion counts N > 1 mixed in (average confidence C / N)
ITERS, DELTA = 10, 1e-8


def _tum_like(H, W):
    """TUM freiburg1 calibration (640x480) scaled per axis: fx != fy, a principal point off the image centre."""
    sx, sy = 640.0 / W, 480.0 / H
    return torch.tensor([[517.3 / sx, 0.0, 318.6 / sx], [0.0, 516.5 / sy, 255.3 / sy], [0.0, 0.0, 1.0]],
                        dtype=torch.float32)


def _off_ray(Xs, seed):
    """x and y times 1 + 0.05 randn (seeded): the points leave their pixel rays, the depths stay."""
    gen = torch.Generator().manual_seed(seed)
    X = Xs.clone()
    X[..., :2] *= 1.0 + 0.05 * torch.randn(X[..., :2].shape, generator=gen)
    return X


def _overlapping(G, idx, valid):
    """make_graph's cameras stand 60 (6 keyframes) or 90 degrees (4) apart: at 3x5 and 2x640 pixels no point of one
    keyframe falls inside another's image, every match is invalid, every weight is zero and the solve is a no-op that
    any kernel passes. For such a graph the cameras start close together instead (identity plus 2 cm of seeded noise,
    keyframe 0 exact), 80 % of the matches are valid and nine in ten of them match a pixel to itself (the rest keep
    make_graph's match): a solve that moves the poses and stays finite (checked with the oracle on the CPU)."""
    gen = torch.Generator().manual_seed(3)
    valid = valid | (torch.rand(valid.shape, generator=gen) < 0.8)
    own = torch.arange(idx.shape[1]).expand_as(idx)
    idx = torch.where(torch.rand(idx.shape, generator=gen) < 0.1, idx, own)
    n = G["Twc0"].shape[0]
    T0 = torch.zeros(n, 8)
    T0[:, 6:] = 1.0
    T0[1:, :3] = 0.02 * torch.randn(n - 1, 3, generator=gen)
    return dict(G, Twc0=T0), idx, valid


_CASES = {}


def _case(n_kf, H, W, centred=True):
    """One raw-point graph per shape, built once and shared (tensors on the device, never modified):
    raw X list, stacked constrained X, confidence sums, stacked average confidences, fusion counts, edges, K."""
    key = (n_kf, H, W, centred)
    if key not in _CASES:
        from m3s.geometry import constrain_points_to_ray
        from m3s.synthetic import make_graph, two_way

        G = make_graph(n_kf=n_kf, H=H, W=W, seed=5)
        ii, jj, idx, valid, Q = two_way(G)
        if not valid.any():
            G, idx, valid = _overlapping(G, idx, valid)
        ii, jj, idx, valid, Q = (t.cuda().contiguous() for t in (ii, jj, idx, valid, Q))
        valid, Q = valid.reshape(idx.shape).contiguous(), Q.reshape(idx.shape).contiguous()
        K = (G["K"] if centred else _tum_like(H, W)).cuda()
        raw = _off_ray(G["Xs"], 100 + H * W).cuda()
        cons = constrain_points_to_ray((H, W), raw, K)  # on the device, K on the device: true divisions
        assert float((raw - cons).abs().max()) > 1e-3  # the perturbation (or the other K) moved them off the rays
        nf = NFUSE[:n_kf]
        C_sum = [(G["Cs"][k].cuda() * float(n)).contiguous() for k, n in enumerate(nf)]
        Cs = torch.stack([c / n for c, n in zip(C_sum, nf)])  # get_average_conf, stacked
        _CASES[key] = dict(G=G, H=H, W=W, K=K, raw=[raw[k].contiguous() for k in range(n_kf)], cons=cons, C_sum=C_sum,
                           Cs=Cs, nf=nf, edges=(ii, jj, idx, valid, Q), Twc0=G["Twc0"].cuda())
    return _CASES[key]


def _solve(c, Xs, Cs, keyframes=None):
    """gauss_newton_sharded("calib"): stacked (Xs, Cs) or zero-copy (keyframes) -> (poses, dx)."""
    from m3s.config import config
    from m3s.dist_ba import gauss_newton_sharded

    T = c["Twc0"].clone()
    dx = gauss_newton_sharded("calib", T, Xs, Cs, *c["edges"], config["local_opt"], ITERS, DELTA, K=c["K"],
                              height=c["H"], width=c["W"], keyframes=keyframes)[0]
    torch.cuda.synchronize()
    return T, dx


def _raw(c, X_list=None):
    return _solve(c, None, None, keyframes=(X_list if X_list is not None else c["raw"], c["C_sum"], c["nf"]))


def _stacked(c, Xs=None):
    return _solve(c, c["cons"] if Xs is None else Xs, c["Cs"])


# (keyframes, H, W, centred K)
PARITY = [
    pytest.param(6, 3, 5, True, id="3x5"),            # N = 15: one partial round, second point of the pair missing
    pytest.param(6, 48, 66, True, id="48x66"),        # division-sensitive; W does not divide the round stride
    pytest.param(6, 48, 66, False, id="48x66-tum"),   # fx != fy, principal point off centre
    pytest.param(4, 2, 640, True, id="2x640"),        # W larger than a round of 512 points
    pytest.param(6, 128, 192, True, id="128x192"),    # several chunks: a chunk starts in the middle of a row
    pytest.param(4, 8, 2048, True, id="8x2048"),      # W + H beyond the LDS room: the tables are read through the cache
]


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("n_kf,H,W,centred", PARITY)
def test_raw_plan_equals_stacked_constrained(n_kf, H, W, centred, fused, monkeypatch):
    """The zero-copy raw plan == the stacked plan on constrain_points_to_ray(raw), bit for bit, 10 iterations, with
    the pack as its own launch and fused into the first linearisation."""
    monkeypatch.setenv("M3S_BA_FUSED_PACK", fused)
    c = _case(n_kf, H, W, centred)
    T_a, dx_a = _stacked(c)
    T_b, dx_b = _raw(c)
    assert torch.isfinite(T_b).all() and not torch.equal(T_b, c["Twc0"])
    assert torch.equal(T_a, T_b) and torch.equal(dx_a, dx_b)
    if (H, W) == (128, 192):
        chunks, per = _plan_chunks(c)
        assert chunks > 1 and per % W != 0  # the second chunk starts inside an image row


def _plan_chunks(c):
    """(linearisation chunks per edge, points per chunk) of the raw plan of this case."""
    from m3s import _lib
    from m3s.config import config
    from m3s.dist_ba import HipShard, ba_config

    ii = c["edges"][0]
    sh = HipShard(ba_config("calib_raw", config["local_opt"], c["K"], c["H"], c["W"]), c["Twc0"].clone(), None, None,
                  *c["edges"], DELTA, 0, ii.shape[0], keyframes=(c["raw"], c["C_sum"], c["nf"]))
    info = (ctypes.c_int * 13)()
    _lib.check(sh.lib.m3s_ba_plan_info(ctypes.byref(sh.plan), info))
    N = c["H"] * c["W"]
    return info[0], (N + info[0] - 1) // info[0]


def test_mode2_on_raw_points_differs():
    """Sensitivity: plain calib run directly on the raw stacked points gives other poses than the raw mode, so these
    inputs can tell a kernel that constrains from one that does not."""
    c = _case(6, 48, 66)
    T_raw, _ = _raw(c)
    T_m2, _ = _stacked(c, torch.stack(c["raw"]))
    assert not torch.equal(T_raw, T_m2)
    assert float((T_raw - T_m2).abs().max()) > 1e-4


def test_depth_edge_cases_equal_stacked():
    """Depths of 0, below 0 and just below depth_eps in two keyframes (a few hundred each): still bit-equal to the
    stacked path and finite."""
    from m3s.config import config
    from m3s.geometry import constrain_points_to_ray

    c = _case(6, 48, 66)
    eps = float(config["local_opt"]["depth_eps"])
    raw = torch.stack(c["raw"]).clone()
    gen = torch.Generator().manual_seed(9)
    N = raw.shape[1]
    for kf in (1, 4):
        pick = torch.randperm(N, generator=gen)[:600].cuda()
        raw[kf, pick[:200], 2] = 0.0
        raw[kf, pick[200:400], 2] = -0.7
        raw[kf, pick[400:], 2] = 0.9 * eps
    assert torch.isfinite(raw).all()
    cons = constrain_points_to_ray((c["H"], c["W"]), raw, c["K"])
    T_a, dx_a = _stacked(c, cons)
    T_b, dx_b = _raw(c, [raw[k].contiguous() for k in range(raw.shape[0])])
    assert torch.isfinite(T_b).all() and torch.isfinite(dx_b).all()
    assert torch.equal(T_a, T_b) and torch.equal(dx_a, dx_b)


def test_stacked_raw_plan_equals_keyframe_table():
    """m3s_ba_make_plan with the raw points stacked and mode 3 == the pointer-table plan: the mode does not depend
    on the entry point."""
    from m3s import _lib
    from m3s.config import config
    from m3s.dist_ba import ba_config

    c = _case(6, 48, 66)
    T_b, dx_b = _raw(c)
    lib = _lib.load()
    cfg = ba_config("calib_raw", config["local_opt"], c["K"], c["H"], c["W"])
    ii, jj, idx, valid, Q = c["edges"]
    Xs, Cs = torch.stack(c["raw"]).contiguous(), c["Cs"].reshape(len(c["raw"]), -1).contiguous()
    Kp, N, E = Xs.shape[0], Xs.shape[1], ii.shape[0]
    T = c["Twc0"].clone()
    dx = torch.zeros((Kp - 1, 7), dtype=torch.float32, device="cuda")
    ws = torch.empty(lib.m3s_ba_workspace_size(Kp, N, E), dtype=torch.uint8, device="cuda")
    plan = _lib.BaPlan()
    s = _lib.stream_ptr(torch.device("cuda"))
    _lib.check(lib.m3s_ba_make_plan(ctypes.byref(cfg), _lib.ptr(T), _lib.ptr(Xs), _lib.ptr(Cs), Kp, N, _lib.ptr(ii),
                                    _lib.ptr(jj), E, 0, E, _lib.ptr(idx), _lib.ptr(valid), _lib.ptr(Q), DELTA,
                                    _lib.ptr(dx), _lib.ptr(ws), ws.numel(), ctypes.byref(plan), s))
    for _ in range(ITERS):
        _lib.check(lib.m3s_ba_linearize(ctypes.byref(plan), s))
        _lib.check(lib.m3s_ba_solve(ctypes.byref(plan), s))
    it = ctypes.c_int()
    _lib.check(lib.m3s_ba_iterations(ctypes.byref(plan), ctypes.byref(it), s))
    lib.m3s_ba_plan_release(_lib.ptr(ws))
    assert torch.equal(T, T_b) and torch.equal(dx, dx_b)


def test_raw_mode_vs_fp64_truth():
    """The project's contract: within 1e-5 of the oracle's fp64 truth on backproject_constrain(raw)."""
    from m3s.config import config

    c = _case(6, 48, 66)
    H, W = c["H"], c["W"]
    lo = config["local_opt"]
    Kn = c["K"].cpu().numpy()
    Xc = O.backproject_constrain(torch.stack(c["raw"]).cpu().numpy(), Kn, (H, W))
    p = O.ba_params("calib", lo["sigma_pixel"], lo["sigma_depth"], lo["C_conf"], lo["Q_conf"], K=Kn, height=H, width=W,
                    pixel_border=lo["pixel_border"], z_eps=lo["depth_eps"])
    ii, jj, idx, valid, Q = (t.cpu().numpy() for t in c["edges"])
    T64, _, _ = O.gauss_newton_f64("calib", c["Twc0"].cpu().numpy().astype(np.float64), Xc.astype(np.float64),
                                   c["Cs"].cpu().numpy()[..., 0].astype(np.float64), ii, jj, idx, valid,
                                   Q.astype(np.float64), p, ITERS, DELTA)
    T, _ = _raw(c)
    err = float(np.abs(T.cpu().numpy() - T64).max())
    print(f"raw calib 6-KF 48x66: max pose error vs fp64 truth {err:.2e} (contract 1e-5)")
    assert err <= 1e-5


def _factor_graph(g, X_raw, K, H, W, n_edges=None, poses=None):
    """FactorGraph over the golden 6-keyframe graph as test_factor_graph_matches_reference builds it, with the given
    keyframe points; the first n_edges undirected edges."""
    from m3s.frame import Frame, Keyframes
    from m3s.global_opt import FactorGraph
    from m3s.sim3 import Sim3

    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kfs = Keyframes()
    for k in range(6):
        T0 = d(g["Twc0"][k]).view(1, 8) if poses is None else poses[k].view(1, 8).clone()
        f = Frame(k, (H, W), T_WC=Sim3(T0))
        f.X_canon = X_raw[k].clone()
        f.C = d(g["Cs"][k]) * float(NFUSE[k])
        f.N = NFUSE[k]
        kfs.append(f)
    fg = FactorGraph(None, kfs, K=K, device="cuda")
    E = g["ii"].shape[0]
    n = E if n_edges is None else n_edges
    fg.ii, fg.jj = d(g["ii"][:n]), d(g["jj"][:n])
    fg.idx_ii2jj, fg.idx_jj2ii = d(g["idx2"][:E][:n]), d(g["idx2"][E:][:n])
    fg.valid_match_j, fg.valid_match_i = d(g["valid2"][:E][:n]), d(g["valid2"][E:][:n])
    fg.Q_ii2jj, fg.Q_jj2ii = d(g["Q2"][:E][:n]), d(g["Q2"][E:][:n])
    return fg, kfs


def _poses(kfs):
    return torch.stack([kfs[k].T_WC.data.reshape(8) for k in range(len(kfs))])


def _golden_raw(golden):
    from m3s.geometry import constrain_points_to_ray

    g = golden("ba_6kf_24x32.npz")
    H, W = 24, 32
    K = torch.from_numpy(g["K"]).float().cuda()
    raw = _off_ray(torch.from_numpy(g["Xs"]), 77).cuda()
    assert float((raw - constrain_points_to_ray((H, W), raw, K)).abs().max()) > 1e-3
    return g, raw, K, H, W


def _forbidden(*a, **k):
    raise AssertionError("the zero-copy calib solve must not stack or constrain the keyframe points")


def test_factor_graph_solves_calib_without_copies(golden, monkeypatch):
    """solve_GN_calib reads the keyframes in place (get_poses_points and constrain_points_to_ray never run) and gives
    the poses of the stacked path bit for bit; a CPU K or a non-contiguous X_canon takes the stacked path."""
    import m3s.global_opt as GO

    g, raw, K, H, W = _golden_raw(golden)
    monkeypatch.setenv("M3S_BA_CALIB_ZERO_COPY", "0")
    fg_s, kfs_s = _factor_graph(g, raw, K, H, W)
    fg_s.solve_GN_calib()
    want = _poses(kfs_s)
    monkeypatch.setenv("M3S_BA_CALIB_ZERO_COPY", "1")

    fg, kfs = _factor_graph(g, raw, K, H, W)
    with monkeypatch.context() as m:
        m.setattr(GO.FactorGraph, "get_poses_points", _forbidden)
        m.setattr(GO, "constrain_points_to_ray", _forbidden)
        fg.solve_GN_calib()
    got = _poses(kfs)
    assert torch.isfinite(got).all() and not torch.equal(got[1:], torch.from_numpy(g["Twc0"]).cuda()[1:])
    assert torch.equal(got, want)

    # the stacked path still runs where the zero-copy one does not qualify
    calls = []
    orig = GO.FactorGraph.get_poses_points

    def counted(self, uniq):
        calls.append(1)
        return orig(self, uniq)

    monkeypatch.setattr(GO.FactorGraph, "get_poses_points", counted)
    fg_c, kfs_c = _factor_graph(g, raw, K.cpu(), H, W)  # K as a CPU tensor
    fg_c.solve_GN_calib()
    assert len(calls) == 1 and torch.isfinite(_poses(kfs_c)).all()
    assert not torch.equal(_poses(kfs_c)[1:], torch.from_numpy(g["Twc0"]).cuda()[1:])
    fg_n, kfs_n = _factor_graph(g, raw, K, H, W)
    wide = torch.zeros((H * W, 4), dtype=torch.float32, device="cuda")
    wide[:, :3] = raw[2]
    kfs_n[2].X_canon = wide[:, :3]  # one keyframe's points non-contiguous
    assert not kfs_n[2].X_canon.is_contiguous()
    fg_n.solve_GN_calib()
    assert len(calls) == 2
    assert torch.equal(_poses(kfs_n), want)  # same data, so the same poses by the stacked path


def test_factor_graph_record_reuse_on_raw_keyframes(golden, monkeypatch):
    """Two successive zero-copy solves on one graph; between them one keyframe is overwritten (X_canon, C, N, as a
    fusion does) and one edge is appended. The second solve repacks only what changed and equals a fresh stacked solve
    of the same state bit for bit."""
    g, raw, K, H, W = _golden_raw(golden)
    E = g["ii"].shape[0]
    monkeypatch.setenv("M3S_BA_CALIB_ZERO_COPY", "1")
    fg, kfs = _factor_graph(g, raw, K, H, W, n_edges=E - 1)
    assert set(g["ii"][:E - 1].tolist()) | set(g["jj"][:E - 1].tolist()) == set(range(6))
    fg.solve_GN_calib()
    assert fg.ba_info["packed_edges"] == 2 * (E - 1)
    # a fusion into keyframe 3: new points (off the rays again), new confidence sum, one more fused frame
    X3 = _off_ray(kfs[3].X_canon.cpu(), 78).cuda()
    C3 = kfs[3].C * 1.25
    N3 = kfs[3].N + 1
    kfs[3].X_canon, kfs[3].C, kfs[3].N = X3, C3, N3
    full, _ = _factor_graph(g, raw, K, H, W)  # the same graph with the appended edge
    for name in ("ii", "jj", "idx_ii2jj", "idx_jj2ii", "valid_match_j", "valid_match_i", "Q_ii2jj", "Q_jj2ii"):
        setattr(fg, name, getattr(full, name))
    start = _poses(kfs).clone()

    monkeypatch.setenv("M3S_BA_CALIB_ZERO_COPY", "0")
    raw2 = raw.clone()
    raw2[3] = X3
    fg_s, kfs_s = _factor_graph(g, raw2, K, H, W, poses=start)
    kfs_s[3].C, kfs_s[3].N = C3.clone(), N3
    fg_s.solve_GN_calib()
    want = _poses(kfs_s)
    monkeypatch.setenv("M3S_BA_CALIB_ZERO_COPY", "1")

    fg.solve_GN_calib()
    got = _poses(kfs)
    assert torch.equal(got, want) and not torch.equal(got, start)
    assert 0 < fg.ba_info["packed_edges"] < 2 * E
    n3 = int(((fg.ii == 3) | (fg.jj == 3)).sum())
    last_touches_3 = int(fg.ii[-1]) == 3 or int(fg.jj[-1]) == 3
    assert fg.ba_info["packed_edges"] == 2 * (n3 + (0 if last_touches_3 else 1))
    assert fg.ba_info["changed_keyframes"] == 1


def test_raw_mode_rejects_bad_sizes():
    """Mode 3 checks its sizes like calib: N != H * W, or W >= 65536, is M3S_EINVAL (RuntimeError), nothing runs."""
    from m3s.config import config
    from m3s.dist_ba import HipShard, ba_config

    c = _case(6, 3, 5)
    E = c["edges"][0].shape[0]
    kf = (c["raw"], c["C_sum"], c["nf"])
    for H, W in ((3, 4), (5, 5)):
        T = c["Twc0"].clone()
        with pytest.raises(RuntimeError, match="m3s error -1"):
            HipShard(ba_config("calib_raw", config["local_opt"], c["K"], H, W), T, None, None, *c["edges"], DELTA, 0, E,
                     keyframes=kf)
        torch.cuda.synchronize()
        assert torch.equal(T, c["Twc0"])
    # W = 65536, H = 1, N = 65536: the sizes agree, the width does not fit the 16-bit pixel of the record
    N = 65536
    X = [torch.ones((N, 3), dtype=torch.float32, device="cuda") for _ in range(2)]
    C = [torch.ones((N,), dtype=torch.float32, device="cuda") for _ in range(2)]
    ii, jj = torch.tensor([0, 1], device="cuda"), torch.tensor([1, 0], device="cuda")
    idx = torch.arange(N, device="cuda").repeat(2, 1).contiguous()
    valid = torch.ones((2, N), dtype=torch.bool, device="cuda")
    Q = torch.full((2, N), 2.0, dtype=torch.float32, device="cuda")
    T = c["Twc0"][:2].clone()
    for mode in ("calib_raw", "calib"):
        with pytest.raises(RuntimeError, match="m3s error -1"):
            HipShard(ba_config(mode, config["local_opt"], c["K"], 1, N), T, None, None, ii, jj, idx, valid, Q, DELTA, 0,
                     2, keyframes=(X, C, [1, 1]))
    torch.cuda.synchronize()
    assert torch.equal(T, c["Twc0"][:2])
