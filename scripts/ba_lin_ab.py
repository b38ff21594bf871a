"""Bit identity of the BA linearisation between two builds of libm3s (M3S_LIB selects the library; this tree's by
default): a fixed list of cases, one SHA-1 each of the (E,36) edge sums after the first linearisation, of Twc after 10
iterations and of dx after 10 iterations. Run it once per library, each in a fresh process, and compare the lines.

usage: [M3S_LIB=...] python scripts/ba_lin_ab.py [--only A,B,...] [--spans N] [--json FILE]

The cases reach every branch of ba_lin_kernel (points / rays / calib / raw calib, separate and fused pack):
  A  24 keyframes 48x66, every mode                B  the same in 244-point chunks (no lane has a second point)
  C  6 keyframes 128x192, 48 rounds, one flush     D  4 keyframes 72x512 in one 72-round chunk (the in-loop flush)
  E  the raw-calib shapes of tests/test_gpu_ba_calib_raw.py through the zero-copy keyframe plan
  F  two shards of the golden 6-keyframe graph (a non-zero edge offset)
  G  record reuse: a second plan that adds an edge (record slots, a partial pack list)
  H  the two 256-keyframe graphs of scripts/ba_exp.py; --spans N also prints the median ba_linearize span of N calls
A case counts only if its edge sums are finite and non-zero and its poses moved: asserted."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "lightweight-mast3r-slam_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, _p)
import torch  # noqa: E402

from m3s import _lib  # noqa: E402
from m3s.config import config  # noqa: E402
from m3s.dist_ba import HipShard, RecordCache, ba_config, shard_range  # noqa: E402
from m3s.geometry import constrain_points_to_ray  # noqa: E402
from m3s.synthetic import chess_poses, euroc_poses, make_graph, make_traj_graph, two_way  # noqa: E402

ITERS = 10
OUT = {}


def sha(t):
    return hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def solve(name, shards, Twcs, Twc0, env=None):
    """The GN loop of test_sharded_split_api_single_process_equals_full over these shards (one: the plain solve)."""
    torch.cuda.synchronize()
    first = None
    for it in range(ITERS):
        for s in shards:
            s.linearize()
        if it == 0:
            torch.cuda.synchronize()
            first = [s.edge_sums.clone() for s in shards]
        if len(shards) > 1:
            total = sum(s.edge_sums for s in shards)
            for s in shards:
                s.edge_sums.copy_(total)
        for s in shards:
            s.solve()
    torch.cuda.synchronize()
    T, dx = Twcs[0], shards[0].dx
    for es in first:
        assert torch.isfinite(es).all() and float(es.abs().sum()) > 0, f"{name}: edge sums empty or not finite"
    assert torch.isfinite(T).all() and not torch.equal(T, Twc0), f"{name}: the poses did not move"
    assert all(torch.equal(T, t) for t in Twcs)
    if env:
        name += "/" + ",".join(f"{k[4:]}={v}" for k, v in sorted(env.items()))
    OUT[name] = dict(edge_sums_sha1=[sha(es) for es in first], twc_sha1=sha(T), dx_sha1=sha(dx))
    print(name, " ".join(OUT[name]["edge_sums_sha1"]), OUT[name]["twc_sha1"], OUT[name]["dx_sha1"], flush=True)


def one(name, cfg, Twc0, Xs, Cs, edges, env=None, keyframes=None, **kw):
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        T = Twc0.clone()
        E = edges[0].shape[0]
        solve(name, [HipShard(cfg, T, Xs, Cs, *edges, 0.0, 0, E, keyframes=keyframes, **kw)], [T], Twc0, env)
    finally:
        for k in env or {}:
            del os.environ[k]


def synthetic(n_kf, H, W, seed):
    """make_graph with both edge directions on the device; the overlapping recipe of test_gpu_ba_calib_raw.py where the
    cameras see nothing of each other."""
    from test_gpu_ba_calib_raw import _overlapping

    G = make_graph(n_kf=n_kf, H=H, W=W, seed=seed)
    ii, jj, idx, valid, Q = two_way(G)
    if not valid.any():
        G, idx, valid = _overlapping(G, idx, valid)
    ii, jj, idx = (t.cuda().contiguous() for t in (ii, jj, idx))
    valid, Q = valid.reshape(idx.shape).cuda().contiguous(), Q.reshape(idx.shape).cuda().contiguous()
    Xs, Cs, K = G["Xs"].cuda().contiguous(), G["Cs"][..., 0].cuda().contiguous(), G["K"].cuda()
    return dict(Xs=Xs, Cs=Cs, K=K, edges=(ii, jj, idx, valid, Q), Twc0=G["Twc0"].cuda(), H=H, W=W,
                cons=constrain_points_to_ray((H, W), Xs, K).contiguous())


def modes(tag, g, which, envs):
    for mode in which:
        cfg = ba_config(mode, config["local_opt"], K=g["K"], height=g["H"], width=g["W"])
        kf = None
        Xs = g["cons"] if mode == "calib" else g["Xs"]
        if mode == "calib_raw":  # the keyframes' own raw points, zero-copy
            kf, Xs = ([x.contiguous() for x in g["Xs"]], [c.contiguous() for c in g["Cs"]], [1] * len(g["Xs"])), None
        for env in envs:
            one(f"{tag}/{mode}", cfg, g["Twc0"], Xs, None if kf else g["Cs"], g["edges"], env, keyframes=kf)


def fused(**env):
    return [dict(env, M3S_BA_FUSED_PACK=f) for f in ("0", "1")]


def case_A():
    modes("A_kf24_48x66", synthetic(24, 48, 66, 5), ("points", "rays", "calib"), fused())


def case_B():
    modes("B_kf24_48x66", synthetic(24, 48, 66, 5), ("points", "rays", "calib"), fused(M3S_BA_CHUNK_POINTS="256"))


def case_C():
    modes("C_kf6_128x192", synthetic(6, 128, 192, 11), ("rays", "calib"), fused(M3S_BA_CHUNK_POINTS="24576"))


def case_D():
    modes("D_kf4_72x512", synthetic(4, 72, 512, 5), ("rays", "calib_raw"), fused(M3S_BA_CHUNK_POINTS="36864"))


def case_E():
    from test_gpu_ba_calib_raw import PARITY, _case

    for prm in PARITY:
        n_kf, H, W, centred = prm.values
        c = _case(n_kf, H, W, centred)
        cfg = ba_config("calib_raw", config["local_opt"], K=c["K"], height=H, width=W)
        for env in fused():
            one(f"E_raw_{prm.id}", cfg, c["Twc0"], None, None, c["edges"], env, keyframes=(c["raw"], c["C_sum"], c["nf"]))


def case_F():
    g = np.load(os.path.join(REPO, "tests", "golden", "ba_6kf_24x32.npz"))
    d = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda() if dt else \
        torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ii, jj = np.concatenate((g["ii"], g["jj"])), np.concatenate((g["jj"], g["ii"]))
    E = ii.shape[0]
    cfg = ba_config("rays", config["local_opt"])
    Twcs = [d(g["Twc0"]) for _ in range(2)]
    shards = [HipShard(cfg, Twcs[r], d(g["Xs"]), d(g["Cs"][..., 0]), d(ii), d(jj), d(g["idx2"]),
                       d(g["valid2"][..., 0], torch.bool), d(g["Q2"][..., 0]), 0.0, *shard_range(E, r, 2))
              for r in range(2)]
    solve("F_two_shards_6kf_24x32/rays", shards, Twcs, d(g["Twc0"]))


def case_G():
    g = synthetic(6, 24, 32, 5)
    ii = g["edges"][0]
    E = ii.shape[0]
    keep = torch.tensor([e for e in range(E) if e % (E // 2) != E // 2 - 1], device="cuda")  # all but the last pair
    cache = RecordCache()
    kf_uid = np.arange(g["Xs"].shape[0], dtype=np.int64)
    for mode in ("rays", "calib"):
        cfg = ba_config(mode, config["local_opt"], K=g["K"], height=g["H"], width=g["W"])
        Xs = g["cons"] if mode == "calib" else g["Xs"]
        first = tuple(t[keep].contiguous() for t in g["edges"])
        one(f"G_reuse_first/{mode}", cfg, g["Twc0"], Xs, g["Cs"], first, reuse=(keep.cpu().numpy(), kf_uid), cache=cache)
        T = g["Twc0"].clone()
        sh = HipShard(cfg, T, Xs, g["Cs"], *g["edges"], 0.0, 0, E, reuse=(np.arange(E, dtype=np.int64), kf_uid),
                      cache=cache)
        assert sh.reuse_info()[0] == 2, sh.reuse_info()  # only the added pair packs, into new slots
        solve(f"G_reuse_added_edge/{mode}", [sh], [T], g["Twc0"])
        del sh
        cache.release()


def case_H(spans=0):
    dev = torch.device("cuda")
    lib = _lib.load()
    for traj, mode, H, W in (("chess", "calib", 384, 512), ("euroc", "rays", 320, 512)):
        G = make_traj_graph((chess_poses if traj == "chess" else euroc_poses)(256), H, W, seed=1, device=dev)
        edges = (G["ii"], G["jj"], G["idx"].contiguous(), G["valid"][..., 0].contiguous(), G["Q"][..., 0].contiguous())
        Xs, Cs = G["Xs"].contiguous(), G["Cs"][..., 0].contiguous()
        if mode == "calib":
            Xs = constrain_points_to_ray((H, W), Xs, G["K"]).contiguous()
        cfg = ba_config(mode, config["local_opt"], K=G["K"], height=H, width=W)
        name = f"H_exp_{traj}_{mode}_K256_{H}x{W}"
        one(name, cfg, G["Twc0"], Xs, Cs, edges)
        ms_all = []
        for _ in range(spans):  # the ba_linearize span (ms per iteration) of one 10-iteration call
            T = G["Twc0"].clone()
            sh = HipShard(cfg, T, Xs, Cs, *edges, 0.0, 0, edges[0].shape[0])
            torch.cuda.synchronize()
            lib.m3s_timing_reset()
            lib.m3s_timing_enable(1)
            for _ in range(ITERS):
                sh.linearize()
                sh.solve()
            torch.cuda.synchronize()
            lib.m3s_timing_enable(0)
            ms, cnt = ctypes.c_double(), ctypes.c_int()
            _lib.check(lib.m3s_timing_query(b"ba_linearize", ms, cnt))
            ms_all.append(ms.value / max(cnt.value, 1))
            del sh
        if spans:
            OUT[name]["ms_lin_per_iter_calls"] = ms_all
            OUT[name]["ms_lin_per_iter"] = sorted(ms_all)[len(ms_all) // 2]
            print(name, "ba_linearize ms per iteration, median of", spans, "calls:", OUT[name]["ms_lin_per_iter"])
        del G, edges, Xs, Cs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="A,B,C,D,E,F,G,H")
    ap.add_argument("--spans", type=int, default=0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    print("library:", os.environ.get("M3S_LIB", "this tree's"), flush=True)
    for c in args.only.split(","):
        if c == "H":
            case_H(args.spans)
        else:
            globals()["case_" + c]()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(OUT, f, indent=1)


if __name__ == "__main__":
    main()
