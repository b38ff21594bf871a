"""End-to-end time of FactorGraph.solve_GN_calib on the C5-shaped graph (the 256-keyframe chess graph, 384x512, calib,
10 iterations: the graph bench.py's BA leg builds), for an A/B of the zero-copy calib solve against its parent.

usage: python scripts/ba_calib_zero_copy_ab.py [--kf 256] [--iters 10] [--label NAME] [--out FILE]

One process = one run. HIP events bracket the whole solve_GN_calib call (stack / constrain copies or pointer table,
plan, pack, iterations, pose write-back):
  fresh   a first solve on a new FactorGraph (every edge packs);
  reuse   the next solve on the same graph after the newest keyframe was re-fused (record reuse: only its edges pack);
each with torch.cuda.max_memory_allocated over the call (less what was allocated before it), and, from a separate
solve with the library's span timing on, ba_linearize per iteration (m3s_timing_query). The script uses only the
FactorGraph surface, so the same file runs on a checkout of the parent commit; M3S_BA_CALIB_ZERO_COPY=0 selects the
stacked path on this tree. Prints one JSON line (and appends it to --out)."""
import argparse
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "lightweight-mast3r-slam_amd"))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kf", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--label", default="tree")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from m3s import _lib
    from m3s.config import config
    from m3s.frame import Frame, Keyframes
    from m3s.global_opt import FactorGraph
    from m3s.sim3 import Sim3
    from m3s.synthetic import chess_poses, make_traj_graph

    dev = torch.device("cuda:0")
    H, W = args.height, args.width
    config["local_opt"]["max_iters"] = args.iters
    config["local_opt"]["delta_norm"] = 0.0  # no early exit: every run does the same work
    G = make_traj_graph(chess_poses(args.kf), H, W, seed=1, device=dev)
    Eu = G["E_und"]
    X_new = (G["Xs"][-1] * 1.0001).contiguous()  # the newest keyframe after another fusion

    def graph():
        kfs = Keyframes()
        for k in range(args.kf):
            f = Frame(k, (H, W), T_WC=Sim3(G["Twc0"][k].view(1, 8).clone()))
            f.X_canon, f.C, f.N = G["Xs"][k].clone(), G["Cs"][k].clone(), 1
            kfs.append(f)
        fg = FactorGraph(None, kfs, K=G["K"], device=dev)
        fg.ii, fg.jj = G["ii"][:Eu], G["jj"][:Eu]
        fg.idx_ii2jj, fg.idx_jj2ii = G["idx"][:Eu], G["idx"][Eu:]
        fg.valid_match_j, fg.valid_match_i = G["valid"][:Eu], G["valid"][Eu:]
        fg.Q_ii2jj, fg.Q_jj2ii = G["Q"][:Eu], G["Q"][Eu:]
        return fg, kfs

    def reset_poses(kfs):
        for k in range(args.kf):
            kfs[k].T_WC = Sim3(G["Twc0"][k].view(1, 8).clone())

    def timed_solve(fg):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fg.solve_GN_calib()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), (torch.cuda.max_memory_allocated() - base) / 2**20

    def refuse(kfs, flip):
        kfs[args.kf - 1].X_canon = (X_new if flip else G["Xs"][-1]).clone()

    # warm-up: allocator, staging buffers, code objects
    fg, kfs = graph()
    timed_solve(fg)
    del fg, kfs

    fg, kfs = graph()
    fresh_ms, fresh_mib = timed_solve(fg)
    poses_fresh = torch.stack([kfs[k].T_WC.data.reshape(8) for k in range(args.kf)])
    reuse_ms, reuse_mib, packed = [], [], None
    for r in range(3):
        reset_poses(kfs)
        refuse(kfs, r % 2 == 0)
        ms, mib = timed_solve(fg)
        reuse_ms.append(ms)
        reuse_mib.append(mib)
        packed = fg.ba_info.get("packed_edges")
    # the linearisation's span per iteration, in a solve of its own (the spans add events to the stream)
    lib = _lib.load()
    reset_poses(kfs)
    refuse(kfs, False)
    lib.m3s_timing_reset()
    lib.m3s_timing_enable(1)
    fg.solve_GN_calib()
    torch.cuda.synchronize()
    lib.m3s_timing_enable(0)
    ms, cnt = ctypes.c_double(), ctypes.c_int()
    _lib.check(lib.m3s_timing_query(b"ba_linearize", ms, cnt))
    out = dict(label=args.label, kf=args.kf, H=H, W=W, iters=args.iters, edges=int(2 * Eu),
               zero_copy_env=os.environ.get("M3S_BA_CALIB_ZERO_COPY"), fresh_ms=fresh_ms, fresh_peak_mib=fresh_mib,
               reuse_ms=sorted(reuse_ms)[1], reuse_ms_all=reuse_ms, reuse_peak_mib=max(reuse_mib),
               reuse_packed_edges=packed, ba_linearize_ms_per_iter=ms.value / max(cnt.value, 1),
               ba_linearize_count=cnt.value, pose_checksum=float(poses_fresh.double().abs().sum()))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
