"""GPU parity: global BA (gauss_newton_{points,rays,calib}, FactorGraph, edge-sharded split API).

The oracle is the C restatement of gn_kernels.cu in fp64 "truth" mode; poses must agree to 1e-5.
"""
import numpy as np
import pytest
import torch

import oracle.oracle as O
from ba_solve_cases import host_solve_from_edge_sums as _host_solve_from_edge_sums

pytestmark = pytest.mark.gpu

SIG = {"points": (0.05, 0.0), "rays": (0.003, 10.0), "calib": (1.0, 10.0)}


def _graph_inputs(g, mode, H, W):
    Xs = g["Xs"]
    if mode == "calib":
        Xs = O.backproject_constrain(Xs, g["K"], (H, W))
    ii = np.concatenate((g["ii"], g["jj"]))
    jj = np.concatenate((g["jj"], g["ii"]))
    return Xs, ii, jj


def _call(mode, Twc, Xs, Cs, ii, jj, idx, valid, Q, K, H, W, max_iter=10, delta=1e-8):
    import mast3r_slam_backends as B

    c = lambda a, dt=None: (torch.from_numpy(np.ascontiguousarray(a)) if dt is None
                            else torch.from_numpy(np.ascontiguousarray(a)).to(dt)).cuda()
    args = (c(Xs), c(Cs), c(ii), c(jj), c(idx), c(valid, torch.bool), c(Q))
    T = c(Twc)
    sa, sb = SIG[mode]
    if mode == "rays":
        dx = B.gauss_newton_rays(T, *args, sa, sb, 0.0, 1.5, max_iter, delta)[0]
    elif mode == "points":
        dx = B.gauss_newton_points(T, *args, sa, 0.0, 1.5, max_iter, delta)[0]
    else:
        Xs_, Cs_, ii_, jj_, idx_, v_, Q_ = args
        dx = B.gauss_newton_calib(T, Xs_, Cs_, c(K), ii_, jj_, idx_, v_, Q_, H, W, -10, 1e-6, sa, sb, 0.0, 1.5,
                                  max_iter, delta)[0]
    return T.cpu().numpy(), dx.cpu().numpy()


@pytest.mark.parametrize("mode", ["points", "rays", "calib"])
def test_gauss_newton_vs_oracle(golden, mode):
    g = golden("ba_6kf_24x32.npz")
    H, W = 24, 32
    Xs, ii, jj = _graph_inputs(g, mode, H, W)
    sa, sb = SIG[mode]
    p = O.ba_params(mode, sa, sb, 0.0, 1.5, K=g["K"], height=H, width=W, pixel_border=-10, z_eps=1e-6)
    T_ref, dx_ref, _ = O.gauss_newton(mode, g["Twc0"], Xs, g["Cs"][..., 0], ii, jj, g["idx2"], g["valid2"][..., 0],
                                      g["Q2"][..., 0], p, 10, 1e-8)
    T, dx = _call(mode, g["Twc0"], Xs, g["Cs"], ii, jj, g["idx2"], g["valid2"], g["Q2"], g["K"], H, W)
    T64, _, _ = O.gauss_newton_f64(mode, g["Twc0"], Xs, g["Cs"][..., 0], ii, jj, g["idx2"], g["valid2"][..., 0],
                                   g["Q2"][..., 0], p, 10, 1e-8)
    print(f"6-KF gauss_newton_{mode}: max pose error vs fp64 truth {np.abs(T - T64).max():.2e}, "
          f"vs fp32 oracle {np.abs(T - T_ref).max():.2e}")
    # this 24x32 fixture graph is ill-conditioned (pixel-quantised matches); after 10 iterations fp32
    # accumulating implementations (the reference's too) sit ~1e-5 from the fp64 truth
    np.testing.assert_allclose(T, T_ref, atol=3e-5)
    # SURVEY §8 a-note 6: the contract is 1e-5 against the fp64 truth, every mode (points included)
    np.testing.assert_allclose(T, T64, atol=1e-5)
    assert dx.shape == (5, 7)
    np.testing.assert_allclose(dx, dx_ref, atol=3e-5)
    # one iteration: the linearisation + solve itself, relative to the step size
    T1, dx1 = _call(mode, g["Twc0"], Xs, g["Cs"], ii, jj, g["idx2"], g["valid2"], g["Q2"], g["K"], H, W, max_iter=1)
    T1r, dx1r, _ = O.gauss_newton(mode, g["Twc0"], Xs, g["Cs"][..., 0], ii, jj, g["idx2"], g["valid2"][..., 0],
                                  g["Q2"][..., 0], p, 1, 1e-8)
    # (first step from the perturbed start: |dx| ~ 0.4 with cond(H) ~ 1e4, so fp32 rounding of the
    #  per-point rows shows at ~1e-4 of the step)
    np.testing.assert_allclose(dx1, dx1r, rtol=0, atol=5e-4 * np.abs(dx1r).max())


@pytest.mark.parametrize("mode", ["rays", "calib"])
def test_factor_graph_matches_reference(golden, mode):
    """m3s.global_opt.FactorGraph vs the reference FactorGraph (golden, oracle backend)."""
    from m3s.frame import Frame, Keyframes
    from m3s.global_opt import FactorGraph
    from m3s.sim3 import Sim3

    g = golden("ba_6kf_24x32.npz")
    H, W = 24, 32
    kfs = Keyframes()
    for k in range(6):
        f = Frame(k, (H, W), T_WC=Sim3(torch.from_numpy(g["Twc0"][k]).view(1, 8).cuda()))
        f.X_canon = torch.from_numpy(g["Xs"][k]).cuda()
        f.C = torch.from_numpy(g["Cs"][k]).cuda()
        f.N = 1
        kfs.append(f)
    fg = FactorGraph(None, kfs, K=torch.from_numpy(g["K"]).cuda(), device="cuda")
    E = g["ii"].shape[0]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    fg.ii, fg.jj = d(g["ii"]), d(g["jj"])
    fg.idx_ii2jj, fg.idx_jj2ii = d(g["idx2"][:E]), d(g["idx2"][E:])
    fg.valid_match_j, fg.valid_match_i = d(g["valid2"][:E]), d(g["valid2"][E:])
    fg.Q_ii2jj, fg.Q_jj2ii = d(g["Q2"][:E]), d(g["Q2"][E:])
    (fg.solve_GN_rays if mode == "rays" else fg.solve_GN_calib)()
    got = np.stack([kfs[k].T_WC.data.cpu().numpy()[0] for k in range(6)])
    # SURVEY §8 a-note 6: the contract is 1e-5 against the fp64 truth of the same algorithm (the
    # fp32 reference order itself sits 7-8e-6 from it on this ill-conditioned 6-KF fixture, see
    # test_oracle.py); against the reference-glue golden the two fp32 roundings add up: 2e-5.
    sig = (0.003, 10.0) if mode == "rays" else (1.0, 10.0)
    Xs = g["Xs"] if mode == "rays" else O.backproject_constrain(g["Xs"], g["K"], (H, W))
    p = O.ba_params(mode, sig[0], sig[1], 0.0, 1.5, K=g["K"], height=H, width=W, pixel_border=-10, z_eps=1e-6)
    ii2 = np.concatenate((g["ii"], g["jj"]))
    jj2 = np.concatenate((g["jj"], g["ii"]))
    T64, _, _ = O.gauss_newton_f64(mode, g["Twc0"], Xs, g["Cs"][..., 0], ii2, jj2, g["idx2"], g["valid2"][..., 0],
                                   g["Q2"][..., 0], p, 10, 1e-8)
    print(f"6-KF FactorGraph {mode}: max pose error vs fp64 truth {np.abs(got - T64).max():.2e} (contract 1e-5)")
    np.testing.assert_allclose(got, T64, atol=1e-5)
    assert np.abs(got - T64).max() <= 8e-6  # the shipped kernel's margin (1.5e-6 rays, 6.2e-6 calib this round)
    np.testing.assert_allclose(got, g[f"{mode}_Twc"], atol=2e-5)


def test_sharded_split_api_single_process_equals_full(golden):
    """Two shards linearised in one process + a host-side sum == the unsharded solve (the exact
    protocol the RCCL path runs, with the all-reduce done by hand)."""
    from m3s.config import config
    from m3s.dist_ba import HipShard, ba_config, shard_range

    g = golden("ba_6kf_24x32.npz")
    H, W = 24, 32
    Xs, ii, jj = _graph_inputs(g, "rays", H, W)
    E = ii.shape[0]
    c = lambda a, dt=None: (torch.from_numpy(np.ascontiguousarray(a)) if dt is None
                            else torch.from_numpy(np.ascontiguousarray(a)).to(dt)).cuda()
    cfg = ba_config("rays", config["local_opt"])
    Twcs = [c(g["Twc0"]) for _ in range(2)]
    shards = [HipShard(cfg, Twcs[r], c(Xs), c(g["Cs"][..., 0]), c(ii), c(jj), c(g["idx2"]),
                       c(g["valid2"][..., 0], torch.bool), c(g["Q2"][..., 0]), 1e-8, *shard_range(E, r, 2))
              for r in range(2)]
    for _ in range(10):
        for s in shards:
            s.linearize()
        total = shards[0].edge_sums + shards[1].edge_sums
        for s in shards:
            s.edge_sums.copy_(total)
            s.solve()
    T_full, _ = _call("rays", g["Twc0"], Xs, g["Cs"], ii, jj, g["idx2"], g["valid2"], g["Q2"], g["K"], H, W)
    a, b = Twcs[0].cpu().numpy(), Twcs[1].cpu().numpy()
    assert np.array_equal(a, b)  # identical systems -> bit-identical poses on every rank
    np.testing.assert_allclose(a, T_full, atol=1e-6)


def test_ba_converges_to_ground_truth_on_consistent_graph():
    rng = np.random.default_rng(0)
    N = 4096
    Xj = rng.standard_normal((N, 3)).astype(np.float32) * 0.5 + np.array([0, 0, 3.0], np.float32)
    Tj = np.array([0.2, -0.1, 0.3, 0.0, 0.1494381, 0.0, 0.9887711, 1.1], np.float32)
    perm = rng.permutation(N)
    Xi = np.zeros_like(Xj)
    Xi[perm] = np.stack([O.sim3_act(Tj.astype(np.float64), Xj[k].astype(np.float64)) for k in range(N)])
    inv = np.empty(N, np.int64)
    inv[perm] = np.arange(N)
    Twc_gt = np.stack((np.array([0, 0, 0, 0, 0, 0, 1, 1], np.float32), Tj))
    Twc0 = Twc_gt.copy()
    Twc0[1, :3] += [0.03, -0.02, 0.01]
    Twc0[1, 7] *= 1.03
    for mode in ("points", "rays"):
        T, dx = _call(mode, Twc0, np.stack((Xi, Xj)), np.full((2, N, 1), 2.0, np.float32), np.array([0, 1]),
                      np.array([1, 0]), np.stack((perm, inv)), np.ones((2, N, 1), bool),
                      np.full((2, N, 1), 2.0, np.float32), None, 0, 0)
        np.testing.assert_allclose(T, Twc_gt, atol=2e-6)


def test_growing_backend_workspace_releases_plan_state():
    """mast3r_slam_backends caches its BA workspace under "ba" and regrows it as E grows; each
    dropped buffer's library plan state must be released with it (m3s_ba_plan_release), or the host table image of
    every replaced workspace stays in the library for good. Replays a growing graph and watches the plan count."""
    from m3s import _lib

    from m3s.synthetic import make_graph, two_way

    lib = _lib.load()
    G = make_graph(n_kf=12, H=8, W=12, seed=4)
    ii, jj, idx, valid, Q = (t.numpy() for t in two_way(G))
    counts = []
    for n_kf in range(3, 13):  # every solve adds a keyframe and its edges: the workspace regrows
        e = np.flatnonzero((ii < n_kf) & (jj < n_kf))
        _call("rays", G["Twc0"].numpy()[:n_kf], G["Xs"].numpy()[:n_kf], G["Cs"].numpy()[:n_kf], ii[e], jj[e], idx[e],
              valid[e], Q[e], None, 0, 0, max_iter=2)
        counts.append(lib.m3s_ba_plan_count())
    torch.cuda.synchronize()
    assert max(counts) - min(counts) <= 1, f"BA plan state grows with the replaced workspaces: {counts}"


def test_singular_system_returns_zero_step():
    """No valid matches -> H singular -> LLT fails -> dx = 0 and Twc unchanged (gn_kernels.cu:147-150)."""
    N = 256
    Xs = np.random.default_rng(0).standard_normal((3, N, 3)).astype(np.float32) + np.array([0, 0, 3], np.float32)
    Twc0 = np.tile(np.array([0, 0, 0, 0, 0, 0, 1, 1], np.float32), (3, 1))
    Twc0[1, 0] = 0.1
    ii, jj = np.array([0, 1]), np.array([1, 2])
    idx = np.tile(np.arange(N), (2, 1))
    T, dx = _call("rays", Twc0, Xs, np.full((3, N, 1), 2.0, np.float32), ii, jj, idx, np.zeros((2, N, 1), bool),
                  np.full((2, N, 1), 2.0, np.float32), None, 0, 0)
    assert np.all(dx == 0) and np.array_equal(T, Twc0)


def test_single_keyframe_is_a_noop():
    N = 64
    Xs = np.ones((1, N, 3), np.float32)
    Twc0 = np.array([[0, 0, 0, 0, 0, 0, 1, 1]], np.float32)
    T, dx = _call("rays", Twc0, Xs, np.full((1, N, 1), 2.0, np.float32), np.array([0]), np.array([0]),
                  np.zeros((1, N), np.int64), np.ones((1, N, 1), bool), np.full((1, N, 1), 2.0, np.float32), None, 0, 0)
    assert dx.shape == (0, 7) and np.array_equal(T, Twc0)


@pytest.mark.parametrize("solver", ["sparse", "dense"])
@pytest.mark.parametrize("n_kf", [48, 97])
def test_pose_solve_matches_lapack_on_large_graph(n_kf, solver, monkeypatch):
    """Both device factorisations against LAPACK on the same assembled system, one GN step from the
    device's own edge sums: the block-sparse one (elimination-tree levels, update groups, columns of
    more than 128 rows on these fill-heavy random-loop graphs) and the dense fallback (panels,
    look-ahead trailing tiles, carried inverse rows, ragged last panel)."""
    monkeypatch.setenv("M3S_BA_SOLVER", solver)
    from m3s.config import config
    from m3s.dist_ba import HipShard, ba_config
    from m3s.synthetic import make_graph, two_way

    G = make_graph(n_kf=n_kf, H=12, W=16, seed=3)
    ii, jj, idx, valid, Q = two_way(G)
    dev = torch.device("cuda")
    cfg = ba_config("rays", config["local_opt"])
    Twc = G["Twc0"].to(dev).contiguous()
    sh = HipShard(cfg, Twc, G["Xs"].to(dev).contiguous(), G["Cs"][..., 0].to(dev).contiguous(), ii.to(dev),
                  jj.to(dev), idx.to(dev).contiguous(), valid[..., 0].to(dev).contiguous(),
                  Q[..., 0].to(dev).contiguous(), 0.0, 0, ii.shape[0])
    sh.linearize()
    es = sh.edge_sums.view(-1, 36).cpu().numpy().copy()
    sh.solve()
    dx = sh.dx.cpu().numpy().reshape(-1)
    ref = _host_solve_from_edge_sums(es, ii.numpy(), jj.numpy())
    assert dx.shape == ref.shape == ((n_kf - 1) * 7,)
    # fp64 factorisation, fp32 output: relative to the step size
    np.testing.assert_allclose(dx, ref, rtol=0, atol=2e-6 * np.abs(ref).max())


@pytest.mark.parametrize("mode", ["rays", "calib"])
def test_ba_medium_graph_vs_fp64_truth(mode):
    """A 24-keyframe graph (consecutive + retrieval-like loop edges, 5% outlier matches, 80% valid) at
    48x64: the full device GN loop (pack, linearisation, several panel launches, carried L^-T) against
    the fp64 truth build of the oracle, 1e-5 on the poses (SURVEY §8c a-note 6)."""
    from m3s.synthetic import make_graph, two_way

    G = make_graph(n_kf=24, H=48, W=64, seed=5)
    ii, jj, idx, valid, Q = (t.numpy() for t in two_way(G))
    H, W = 48, 64
    K = G["K"].numpy()
    Xs = G["Xs"].numpy()
    if mode == "calib":
        Xs = O.backproject_constrain(Xs, K, (H, W))
    Cs = G["Cs"].numpy()
    sa, sb = SIG[mode]
    p = O.ba_params(mode, sa, sb, 0.0, 1.5, K=K, height=H, width=W, pixel_border=-10, z_eps=1e-6)
    T_ref, _, _ = O.gauss_newton_f64(mode, G["Twc0"].numpy().astype(np.float64), Xs.astype(np.float64),
                                     Cs[..., 0].astype(np.float64), ii, jj, idx, valid[..., 0],
                                     Q[..., 0].astype(np.float64), p, 10, 1e-8)
    T, dx = _call(mode, G["Twc0"].numpy(), Xs, Cs, ii, jj, idx, valid, Q, K, H, W)
    assert np.isfinite(T).all()
    np.testing.assert_allclose(T, T_ref, atol=1e-5)


@pytest.mark.parametrize("mode", ["rays", "calib"])
def test_ba_full_chunk_runs_vs_fp64_truth(mode, monkeypatch):
    """6 keyframes at 128x192 = 24576 points per edge, one full linearisation chunk: every lane loads 48 point
    rounds, the most a production chunk holds (BA_RUN_LEN is 64 rounds), flushed into the fp64 sums once, at the
    chunk's end (the smaller graphs end after a few rounds). Poses within 1e-5 of the oracle's fp64 truth.

    make_graph's six cameras stand 60 degrees apart: 2.0 % of this graph's points carry weight (a valid match with
    Q > 1.5), on 10 of its 22 edges, so the 48-round fp32 runs add mostly exact zeros. The densely weighted version,
    with the edge sums themselves compared with fp64 and a chunk of 65 rounds: tests/test_gpu_ba_edges.py."""
    from m3s.synthetic import make_graph, two_way

    # the production chunk length of large graphs (small graphs get shorter chunks, abi_ba.cpp ba_chunks)
    monkeypatch.setenv("M3S_BA_CHUNK_POINTS", "24576")
    H, W = 128, 192
    G = make_graph(n_kf=6, H=H, W=W, seed=11)
    ii, jj, idx, valid, Q = (t.numpy() for t in two_way(G))
    K = G["K"].numpy()
    Xs = G["Xs"].numpy()
    if mode == "calib":
        Xs = O.backproject_constrain(Xs, K, (H, W))
    Cs = G["Cs"].numpy()
    sa, sb = SIG[mode]
    p = O.ba_params(mode, sa, sb, 0.0, 1.5, K=K, height=H, width=W, pixel_border=-10, z_eps=1e-6)
    T_ref, _, _ = O.gauss_newton_f64(mode, G["Twc0"].numpy().astype(np.float64), Xs.astype(np.float64),
                                     Cs[..., 0].astype(np.float64), ii, jj, idx, valid[..., 0],
                                     Q[..., 0].astype(np.float64), p, 10, 1e-8)
    T, dx = _call(mode, G["Twc0"].numpy(), Xs, Cs, ii, jj, idx, valid, Q, K, H, W)
    assert np.isfinite(T).all()
    print(f"full-chunk 6-KF 128x192 {mode}: max pose error vs fp64 truth {np.abs(T - T_ref).max():.2e} (contract 1e-5)")
    np.testing.assert_allclose(T, T_ref, atol=1e-5)
    assert np.abs(T - T_ref).max() <= 8e-6  # the shipped kernel's margin (7.2e-6 rays, 5.2e-6 calib this round)


@pytest.mark.gpu
def test_zero_copy_keyframe_plan_equals_stacked(golden):
    """m3s_ba_make_plan_kf (keyframes' own X_canon / C-sum buffers) == the stacked plan
    of get_poses_points, bit for bit, including the average confidence C / N with N > 1."""
    from m3s.config import config
    from m3s.dist_ba import gauss_newton_sharded

    g = golden("ba_6kf_24x32.npz")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    K = g["Xs"].shape[0]
    Nfuse = [1, 3, 2, 7, 1, 5]
    X_list = [d(g["Xs"][k]) for k in range(K)]
    C_sum = [d(g["Cs"][k]) * float(n) for k, n in enumerate(Nfuse)]        # keyframe confidence sums
    Cs = torch.stack([c / n for c, n in zip(C_sum, Nfuse)])                # get_average_conf, stacked
    Xs = torch.stack(X_list)
    ii2, jj2 = d(np.concatenate((g["ii"], g["jj"]))), d(np.concatenate((g["jj"], g["ii"])))
    args = (ii2, jj2, d(g["idx2"]), d(g["valid2"]), d(g["Q2"]), config["local_opt"], 10, 1e-8)
    T_a, T_b = d(g["Twc0"]), d(g["Twc0"])
    dx_a = gauss_newton_sharded("rays", T_a, Xs, Cs, *args)[0]
    dx_b = gauss_newton_sharded("rays", T_b, None, None, *args, keyframes=(X_list, C_sum, Nfuse))[0]
    assert torch.equal(T_a, T_b) and torch.equal(dx_a, dx_b)
    with pytest.raises(RuntimeError):
        gauss_newton_sharded("rays", d(g["Twc0"]), None, None, *args, keyframes=(X_list, C_sum, [1, 0, 1, 1, 1, 1]))


def test_rccl_all_reduce_path_equals_unsharded(tmp_path):
    """The RCCL leg of the edge-sharded BA (m3s/dist_ba.py run_sharded: one dist.all_reduce of the fp64 edge-sum
    table per GN iteration, replacing the reference's host loop gn_kernels.cu:1181-1225) executed on the GPU: a
    fresh child process initialises the "nccl" (RCCL) process group at world size 1 before any other GPU call,
    runs gauss_newton_sharded through the all-reduce, and must match the unsharded
    mast3r_slam_backends.gauss_newton_rays bit for bit (tests/rccl_child.py)."""
    import os
    import socket
    import subprocess
    import sys

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, "-u", os.path.join(repo, "tests", "rccl_child.py")], env=env, cwd=repo,
                       capture_output=True, text=True, timeout=240)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "RCCL_BA_OK" in r.stdout


def test_factor_schedule_stall_raises_not_silent(monkeypatch):
    """A dataflow hand-off wait of the device factorisation that times out (a schedule fault) is an error
    (M3S_ESTALL -> RuntimeError), never the silent dx = 0 of a non-positive pivot (gn_kernels.cu:142-150, which
    test_singular_system_returns_zero_step keeps). M3S_BA_FORCE_STALL makes every dataflow wait unsatisfiable;
    the bounded spin (~2^20 polls) then gives up. The next plan without it solves normally."""
    from m3s.config import config
    from m3s.dist_ba import HipShard, ba_config, gauss_newton_sharded
    from m3s.synthetic import make_graph, two_way

    monkeypatch.setenv("M3S_BA_SOLVER", "sparse")
    G = make_graph(n_kf=48, H=12, W=16, seed=3)
    ii, jj, idx, valid, Q = two_way(G)
    dev = torch.device("cuda")
    cfg = ba_config("rays", config["local_opt"])
    args = lambda T: (cfg, T, G["Xs"].to(dev).contiguous(), G["Cs"][..., 0].to(dev).contiguous(), ii.to(dev),
                      jj.to(dev), idx.to(dev).contiguous(), valid[..., 0].to(dev).contiguous(),
                      Q[..., 0].to(dev).contiguous(), 0.0, 0, ii.shape[0])
    monkeypatch.setenv("M3S_BA_FORCE_STALL", "1")
    T0 = G["Twc0"].to(dev).contiguous()
    sh = HipShard(*args(T0))
    sh.linearize()
    sh.solve()
    with pytest.raises(RuntimeError, match="stall"):
        sh.iterations()
    assert torch.equal(T0, G["Twc0"].to(dev))  # the stalled iteration did not move the poses
    # the full call surfaces it too
    with pytest.raises(RuntimeError, match="stall"):
        gauss_newton_sharded("rays", G["Twc0"].to(dev).contiguous(), G["Xs"].to(dev).contiguous(),
                             G["Cs"][..., 0].to(dev).contiguous(), ii.to(dev), jj.to(dev), idx.to(dev).contiguous(),
                             valid[..., 0].to(dev).contiguous(), Q[..., 0].to(dev).contiguous(), config["local_opt"],
                             2, 1e-8)
    monkeypatch.delenv("M3S_BA_FORCE_STALL")
    T1 = G["Twc0"].to(dev).contiguous()
    sh = HipShard(*args(T1))
    sh.linearize()
    sh.solve()
    assert sh.iterations() == 1 and not torch.equal(T1, G["Twc0"].to(dev))


@pytest.mark.parametrize("n_kf", [48, 97])
def test_sparse_solve_schedules_are_bit_identical(n_kf, monkeypatch):
    """Every schedule of the block-sparse solve (ba_sparse.hip) runs the same per-task arithmetic in the same order:
    poses and dx after two GN iterations are bit-identical across M3S_BA_FLOW in {1, 0} (dataflow flags / a barrier
    per level) crossed with M3S_BA_WIDE in {unset, 0, 1000000} (the launch-cost split / every step a
    ba_sparse_step_kernel launch / every step inside the one-workgroup kernel). 48 keyframes (47 columns, 500 factor
    blocks, 26 levels, ~33 KB of loop tables): the LDS instance of ba_sparse_factor_kernel, with the dataflow schedule
    and columns of more than 128 rows. 97 keyframes (96 columns, 1612 blocks, 49 levels, ~160 KB of tables, over the
    144 KB the kernel keeps in LDS): the global-table instance and its level-synchronous back substitution."""
    from m3s.config import config
    from m3s.dist_ba import gauss_newton_sharded
    from m3s.synthetic import make_graph, two_way

    monkeypatch.setenv("M3S_BA_SOLVER", "sparse")
    G = make_graph(n_kf=n_kf, H=12, W=16, seed=3)
    ii, jj, idx, valid, Q = two_way(G)
    d = lambda t: t.cuda().contiguous()
    args = (d(G["Xs"]), d(G["Cs"][..., 0]), d(ii), d(jj), d(idx), d(valid[..., 0]), d(Q[..., 0]), config["local_opt"],
            2, 0.0)
    out = {}
    for flow in ("1", "0"):
        for wide in (None, "0", "1000000"):
            monkeypatch.setenv("M3S_BA_FLOW", flow)
            if wide is None:
                monkeypatch.delenv("M3S_BA_WIDE", raising=False)
            else:
                monkeypatch.setenv("M3S_BA_WIDE", wide)
            T = d(G["Twc0"])
            dx = gauss_newton_sharded("rays", T, *args)[0]
            out[flow, wide] = (T.cpu().numpy(), dx.cpu().numpy())
    T0, dx0 = out["1", None]
    assert np.isfinite(T0).all() and np.abs(dx0).max() > 0 and not np.array_equal(T0, G["Twc0"].numpy())
    for key, (T, dx) in out.items():
        assert np.array_equal(T, T0) and np.array_equal(dx, dx0), key


@pytest.mark.parametrize("mode", ["points", "rays", "calib"])
def test_pack_fused_into_first_linearisation_is_bit_identical(mode, monkeypatch):
    """A call that packs every edge builds the point records inside its first linearisation (ba_lin_kernel<PACK>,
    the same pack_record values) instead of a separate ba_pack launch: poses and dx bit-identical to the separate
    pack (the default; M3S_BA_FUSED_PACK=1 opts in), on a 24-keyframe graph with ragged chunks."""
    from m3s.synthetic import make_graph, two_way

    G = make_graph(n_kf=24, H=48, W=66, seed=8)
    ii, jj, idx, valid, Q = (t.numpy() for t in two_way(G))
    K = G["K"].numpy()
    Xs = G["Xs"].numpy()
    if mode == "calib":
        Xs = O.backproject_constrain(Xs, K, (48, 66))
    out = []
    for fused in ("1", "0"):
        monkeypatch.setenv("M3S_BA_FUSED_PACK", fused)
        out.append(_call(mode, G["Twc0"].numpy(), Xs, G["Cs"].numpy(), ii, jj, idx, valid, Q, K, 48, 66))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("mode", ["points", "rays", "calib"])
def test_pack_tiles_with_ragged_last_tile(mode, monkeypatch):
    """The pack kernel's tiles (ba.hip ba_pack_kernel: one block per 4096 points of one edge, 4 points per lane per
    trip, loads at a clamped index) on 72x100 = 7200 points per edge: one full tile and a ragged one whose last
    trip is partly past the edge. Its records must equal the fused pack's (ba_lin_kernel<PACK>: pack_record, one
    point at a time, every load in order) bit for bit, and the poses sit within 1e-5 of the fp64 truth.

    6.8 % of this graph's points carry weight (a valid match with Q > 1.5), on 14 of its 38 edges; the ragged tile's
    32 tail points carry weight on 5 edges. The densely weighted version, with the edge sums themselves compared with
    fp64 (two pack tiles, a last tile of 4 points, a ragged trip): tests/test_gpu_ba_edges.py, cases n4100, n5123."""
    from m3s.synthetic import make_graph, two_way

    H, W = 72, 100
    G = make_graph(n_kf=8, H=H, W=W, seed=13)
    ii, jj, idx, valid, Q = (t.numpy() for t in two_way(G))
    K = G["K"].numpy()
    Xs = G["Xs"].numpy()
    if mode == "calib":
        Xs = O.backproject_constrain(Xs, K, (H, W))
    out = []
    for fused in ("1", "0"):
        monkeypatch.setenv("M3S_BA_FUSED_PACK", fused)
        out.append(_call(mode, G["Twc0"].numpy(), Xs, G["Cs"].numpy(), ii, jj, idx, valid, Q, K, H, W))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    sa, sb = SIG[mode]
    p = O.ba_params(mode, sa, sb, 0.0, 1.5, K=K, height=H, width=W, pixel_border=-10, z_eps=1e-6)
    Cs = G["Cs"].numpy()
    T_ref, _, _ = O.gauss_newton_f64(mode, G["Twc0"].numpy().astype(np.float64), Xs.astype(np.float64),
                                     Cs[..., 0].astype(np.float64), ii, jj, idx, valid[..., 0],
                                     Q[..., 0].astype(np.float64), p, 10, 1e-8)
    np.testing.assert_allclose(out[1][0], T_ref, atol=1e-5)


@pytest.mark.timeout(300)
def test_sharded_hip_path_world2(tmp_path):
    """the product's sharded BA (HipShard over libm3s.so + run_sharded) at N = 2. Two fresh
    processes (gloo, both ranks on cuda:0, started before any GPU call in them: tests/sharded_child.py) each
    linearise half of the 48-keyframe graph's edges into the shared (E, 36) fp64 edge-sum table, all-reduce it and
    solve. Rays and calib, fresh and with record reuse (first call packs every shard edge, the second none): poses
    and dx are bit-identical across ranks, between fresh and reuse, and to the unsharded gauss_newton_* (reference
    call site global_opt.py:123-226)."""
    import os
    import socket
    import subprocess
    import sys

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    procs = []
    for r in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(r), WORLD_SIZE="2",
                   LOCAL_RANK="0", OUT_DIR=str(tmp_path))
        procs.append(subprocess.Popen([sys.executable, "-u", os.path.join(repo, "tests", "sharded_child.py")],
                                      env=env, cwd=repo, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=240)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        print(o[-2000:])
        assert p.returncode == 0 and f"SHARDED_OK rank {r}" in o, o[-3000:]
    R = [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2)]
    E = int(R[0]["E"])
    for mode in ("rays", "calib"):
        for key in ("T", "dx"):
            ref = R[0][f"{mode}_un_{key}"]
            for r in range(2):
                for v in ("", "_reuse0", "_reuse1"):
                    got = R[r][f"{mode}{v}_{key}"]
                    assert np.array_equal(got, ref), f"{mode}{v} {key} rank {r}: {np.abs(got - ref).max()}"
        assert not np.array_equal(R[0][f"{mode}_T"], R[0]["Twc0"]), "BA did not move the poses"
        # rank r packs only its own shard's edges on the first reuse call, none on the second
        assert int(R[0][f"{mode}_reuse0_packed"]) + int(R[1][f"{mode}_reuse0_packed"]) == E
        assert int(R[0][f"{mode}_reuse1_packed"]) == 0 and int(R[1][f"{mode}_reuse1_packed"]) == 0
