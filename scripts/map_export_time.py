"""Time of the map export (m3s.evaluate.world_points / save_reconstruction) on one MI355X against its two baselines.

usage: python scripts/map_export_time.py [--kf 256] [--height 384] [--width 512] [--runs 10] [--warmup 3] [--out FILE]

Inputs: --kf synthetic keyframes of --height x --width from m3s.synthetic.SceneReplay over the chess trajectory
(ray-cast pointmaps + noise, confidences 1 + Exp(mean 4)), calib mode, threshold 1.5, random host colours (uimg).
Every leg is bracketed by HIP events on the current stream (they cover the host work between the launches too) and by
the wall clock; --runs timed runs after --warmup warm-ups, the median reported:
  kernels_soa / kernels_ply   m3s_map_count + m3s_map_write alone, colours already on the device (a viewer's case);
                              also split into the library's own spans map_count / map_write (m3s_timing_query)
  world_points_soa / _ply     the public call, colours converted from the host uimg and uploaded (3 B per pixel)
  world_points_soa_nocolor    geometry only
  save_reconstruction         world_points(layout="ply") + header + one device-to-host copy + the file write
  torch                       world_points_torch: the reference's formulation in torch ops on the device
  numpy_loop                  the reference's per-keyframe host loop restated (evaluate.py:50-68): constrain and act on
                              the device, three .cpu().numpy() copies, boolean index, np.concatenate
Bytes per time is given against the issue's traffic model of 47 B per input point (4 B count pass, 28 B in and at most
15 B out for the write pass). Prints one JSON line and writes it to --out (default profiles/map_export_time.json)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "lightweight-mast3r-slam_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

MODEL_BYTES_PER_POINT = 47


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kf", type=int, default=256)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=1.5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "map_export_time.json"))
    args = ap.parse_args()

    from m3s import _lib, evaluate
    from m3s.config import config
    from m3s.frame import Frame, Keyframes
    from m3s.geometry import constrain_points_to_ray
    from m3s.sim3 import Sim3
    from m3s.synthetic import SceneReplay, chess_poses

    dev = torch.device("cuda:0")
    H, W, Kf, thr = args.height, args.width, args.kf, args.threshold
    N = H * W
    config["use_calib"] = True
    scene = SceneReplay(chess_poses(Kf), H, W, device=dev)
    g = torch.Generator().manual_seed(0)
    kfs = Keyframes()
    for k in range(Kf):
        f = Frame(k, (H, W), T_WC=Sim3(scene.Twc0[k].view(1, 8).clone()))
        f.X_canon, f.C = scene.keyframe(k)
        f.N, f.K = 1, scene.K
        f.uimg = torch.rand(H, W, 3, generator=g)
        kfs.append(f)
    del scene
    print(f"inputs ready: {Kf} keyframes of {H}x{W}", flush=True)

    def timed(fn, runs=args.runs, warmup=args.warmup):
        ev, wall = [], []
        for r in range(warmup + runs):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if r >= warmup:
                ev.append(a.elapsed_time(b))
                wall.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ev), statistics.median(wall)

    # ---- the two passes alone, colours resident on the device ----
    lib = _lib.load()
    frames = [kfs[k] for k in range(Kf)]
    table = evaluate.keyframe_table([f.X_canon for f in frames], [f.C for f in frames], [f.N for f in frames])
    Twc = torch.stack([f.T_WC.data.reshape(8) for f in frames]).contiguous()
    rgb = torch.stack([evaluate._colors_u8(f) for f in frames]).to(dev)
    rgb_list = list(rgb)
    ws = torch.zeros(lib.m3s_map_workspace_size(Kf, N), dtype=torch.uint8, device=dev)
    mcs = {lay: evaluate.map_config(thr, lay, frames[0].K, (H, W)) for lay in ("soa", "ply")}
    _, M = evaluate.map_count(mcs["soa"], table, Kf, N, ws, dev)
    out_xyz = torch.empty((M, 3), dtype=torch.float32, device=dev)
    out_rgb = torch.empty((M, 3), dtype=torch.uint8, device=dev)
    out_ply = torch.empty((M, 15), dtype=torch.uint8, device=dev)

    def kernels(lay):
        evaluate.map_count(mcs[lay], table, Kf, N, ws, dev)
        if lay == "soa":
            evaluate.map_write(mcs[lay], table, Twc, rgb_list, Kf, N, out_xyz, out_rgb, M, ws, dev)
        else:
            evaluate.map_write(mcs[lay], table, Twc, rgb_list, Kf, N, out_ply, None, M, ws, dev)

    res = {}
    for lay in ("soa", "ply"):
        res[f"kernels_{lay}_ms"], res[f"kernels_{lay}_wall_ms"] = timed(lambda: kernels(lay))
        spans = {}
        for name in (b"map_count", b"map_write"):
            vals = []
            for _ in range(args.runs):  # spans add events to the stream: runs of their own
                lib.m3s_timing_reset()
                lib.m3s_timing_enable(1)
                kernels(lay)
                torch.cuda.synchronize()
                lib.m3s_timing_enable(0)
                ms, cnt = ctypes.c_double(), ctypes.c_int()
                _lib.check(lib.m3s_timing_query(name, ms, cnt))
                vals.append(ms.value)
            spans[name.decode()] = statistics.median(vals)
        lib.m3s_timing_reset()
        res[f"span_map_count_{lay}_ms"], res[f"span_map_write_{lay}_ms"] = spans["map_count"], spans["map_write"]
        print(f"kernels {lay}: {res[f'kernels_{lay}_ms']:.3f} ms, spans {spans}", flush=True)
    del out_xyz, out_rgb, out_ply, rgb, rgb_list, ws

    # ---- the public calls ----
    res["world_points_soa_ms"], res["world_points_soa_wall_ms"] = timed(lambda: evaluate.world_points(kfs, thr))
    res["world_points_ply_ms"], res["world_points_ply_wall_ms"] = timed(
        lambda: evaluate.world_points(kfs, thr, layout="ply"))
    res["world_points_soa_nocolor_ms"], res["world_points_soa_nocolor_wall_ms"] = timed(
        lambda: evaluate.world_points(kfs, thr, colors=False))
    print(f"world_points: soa {res['world_points_soa_ms']:.1f} ms, ply {res['world_points_ply_ms']:.1f} ms, "
          f"geometry only {res['world_points_soa_nocolor_ms']:.3f} ms", flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        res["save_reconstruction_ms"], res["save_reconstruction_wall_ms"] = timed(
            lambda: evaluate.save_reconstruction(tmp, "map.ply", kfs, thr))
    print(f"save_reconstruction: {res['save_reconstruction_wall_ms']:.1f} ms wall", flush=True)

    # ---- baselines ----
    res["torch_ms"], res["torch_wall_ms"] = timed(lambda: evaluate.world_points_torch(kfs, thr))
    print(f"torch: {res['torch_ms']:.1f} ms", flush=True)

    def numpy_loop():
        pointclouds, colors = [], []
        for i in range(len(kfs)):
            kf = kfs[i]
            X = constrain_points_to_ray((H, W), kf.X_canon[None], kf.K).squeeze(0)
            pW = kf.T_WC.act(X).cpu().numpy().reshape(-1, 3)
            color = (kf.uimg.cpu().numpy() * 255).astype(np.uint8).reshape(-1, 3)
            valid = kf.get_average_conf().cpu().numpy().astype(np.float32).reshape(-1) > thr
            pointclouds.append(pW[valid])
            colors.append(color[valid])
        return np.concatenate(pointclouds, axis=0), np.concatenate(colors, axis=0)

    res["numpy_loop_ms"], res["numpy_loop_wall_ms"] = timed(numpy_loop)
    print(f"numpy loop: {res['numpy_loop_wall_ms']:.1f} ms wall", flush=True)

    # same rows from all three (the kernel against torch within fp32 rounding, the mask exactly)
    pts, cols, counts = evaluate.world_points(kfs, thr)
    tp, tc, tcounts = evaluate.world_points_torch(kfs, thr)
    npts, ncols = numpy_loop()
    assert torch.equal(counts, tcounts) and torch.equal(cols, tc) and np.array_equal(ncols, cols.cpu().numpy())
    max_diff = float((pts - tp).abs().max())

    model = MODEL_BYTES_PER_POINT * Kf * N
    actual = Kf * N * 4 + 2 * Kf * N // 8 + M * (12 + 3) + M * 15  # C, mask out + in, valid X + rgb rows, rows out
    out = dict(kf=Kf, H=H, W=W, calib=True, threshold=thr, points_in=Kf * N, M=M, runs=args.runs, warmup=args.warmup,
               model_bytes=model, moved_bytes_estimate=actual,
               kernels_soa_model_gbps=model / res["kernels_soa_ms"] / 1e6,
               kernels_ply_model_gbps=model / res["kernels_ply_ms"] / 1e6,
               kernels_ply_moved_gbps=actual / res["kernels_ply_ms"] / 1e6,
               max_abs_diff_vs_torch=max_diff, **res)
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
