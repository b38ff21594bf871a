"""Time of the voxel-grid thinning of the map export (m3s_map_voxel, the voxel_size keyword of
m3s.evaluate.world_points / save_reconstruction) on one MI355X.

usage: python scripts/map_voxel_time.py [--kf 256] [--height 384] [--width 512] [--voxel-sizes 0.005 0.011]
                                        [--runs 10] [--warmup 3] [--torch-runs 3] [--out FILE]

Inputs: those of scripts/map_export_time.py (--kf synthetic keyframes of --height x --width from
m3s.synthetic.SceneReplay over the chess trajectory, calib mode, threshold 1.5, random host colours).
Every leg is bracketed by HIP events on the current stream and by the wall clock; --runs timed runs after --warmup
warm-ups, the median reported. Per voxel size:
  rows_in / rows_out / dropped   the counted rows, the thinned rows, the rows that reached no voxel
  table_bytes                    m3s_map_voxel_table_size(rows_in)
  voxel_ms                       m3s_map_voxel alone (table reset, uploads, insert, thin, re-scan, counts read back) on a
                                 workspace whose count is restored by a device copy outside the timed bracket;
                                 span_map_voxel_ms: the library's own span around the three launches
  table_atomics / atomics_per_s  the 64-bit atomics the insert issues, over the span: one compare-and-swap and one
                                 minimum per run of equal voxel keys on neighbouring lanes of a wave (the kernel merges
                                 such a run before it touches the table), the runs counted here in torch from the
                                 torch formulation's points. Probes past the first slot add compare-and-swaps and the
                                 span also holds the thin kernel and the re-scan, so the rate is a lower bound
  kernels_ms                     count + voxel + write (PLY layout), colours resident on the device
  world_points_ms                the public call (colours converted and uploaded), PLY layout;
                                 world_points_nocolor_ms: geometry only (SOA layout, colors=False)
  save_reconstruction_ms         world_points(layout="ply", voxel_size=) + header + device-to-host copy + file write
  torch_ms                       world_points_torch(voxel_size=): the rule in torch ops (torch.unique + stable sorts)
and once, for comparison, the unthinned legs of this build: kernels_unfiltered_ms, world_points_unfiltered_ms,
world_points_nocolor_unfiltered_ms, save_reconstruction_unfiltered_ms and the file sizes. Prints one JSON line and writes it to --out (default profiles/map_voxel_time.json)."""
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
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kf", type=int, default=256)
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--voxel-sizes", type=float, nargs="+", default=[0.005, 0.011])
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-runs", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=1.5)
    ap.add_argument("--probe", action="store_true", help="only rows in / out per voxel size, nothing timed or written")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "map_voxel_time.json"))
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

    def timed(fn, runs=args.runs, warmup=args.warmup, before=None):
        ev, wall = [], []
        for r in range(warmup + runs):
            if before is not None:
                before()
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

    lib = _lib.load()
    frames = [kfs[k] for k in range(Kf)]
    table = evaluate.keyframe_table([f.X_canon for f in frames], [f.C for f in frames], [f.N for f in frames])
    Twc = torch.stack([f.T_WC.data.reshape(8) for f in frames]).contiguous()
    ws = torch.zeros(lib.m3s_map_workspace_size(Kf, N), dtype=torch.uint8, device=dev)
    mc = evaluate.map_config(thr, "ply", frames[0].K, (H, W))
    _, M = evaluate.map_count(mc, table, Kf, N, ws, dev)
    table_bytes = evaluate.map_voxel_table_size(M)
    vox = torch.empty(table_bytes, dtype=torch.uint8, device=dev)

    if args.probe:
        for vs in args.voxel_sizes:
            evaluate.map_count(mc, table, Kf, N, ws, dev)
            _, M2, dropped = evaluate.map_voxel(mc, table, Twc, Kf, N, vs, vox, ws, dev)
            print(f"voxel {vs}: {M} rows -> {M2} ({M / max(M2, 1):.2f}x), dropped {dropped}", flush=True)
        return

    def insert_runs(vs):
        """Runs of equal voxel keys on neighbouring lanes (pixels of one 64-pixel word) among the rows that reach a
        voxel: what the insert kernel enters into the table after its in-wave merge."""
        r = torch.tensor(evaluate._voxel_scale(vs), dtype=torch.float32, device=dev)
        runs = 0
        for f in frames:
            X = constrain_points_to_ray((H, W), f.X_canon.reshape(-1, 3)[None], f.K)[0]
            pW = f.T_WC.act(X).reshape(-1, 3)
            q = torch.floor(pW * r)
            ok = (f.get_average_conf().reshape(-1) > thr) & torch.isfinite(pW).all(dim=1) & (
                (q >= -2.0 ** 20) & (q < 2.0 ** 20)).all(dim=1)
            b = torch.where(ok[:, None], q, torch.zeros_like(q)).to(torch.int64) + (1 << 20)
            key = (b[:, 0] << 42) | (b[:, 1] << 21) | b[:, 2]
            merged = torch.zeros_like(ok)
            merged[1:] = ok[1:] & ok[:-1] & (key[1:] == key[:-1])
            merged[::64] = False  # lane 0 of a wave has no neighbour before it
            runs += int((ok & ~merged).sum())
        return runs

    rgb = torch.stack([evaluate._colors_u8(f) for f in frames]).to(dev)
    rgb_list = list(rgb)
    out_ply = torch.empty((M, 15), dtype=torch.uint8, device=dev)
    ws_counted = ws.clone()  # the workspace as the count left it

    def kernels(vs):
        evaluate.map_count(mc, table, Kf, N, ws, dev)
        rows = M
        if vs is not None:
            _, rows, _ = evaluate.map_voxel(mc, table, Twc, Kf, N, vs, vox, ws, dev)
        evaluate.map_write(mc, table, Twc, rgb_list, Kf, N, out_ply, None, rows, ws, dev)

    res = {"kernels_unfiltered_ms": timed(lambda: kernels(None))[0]}
    print(f"unfiltered kernels: {res['kernels_unfiltered_ms']:.3f} ms", flush=True)
    sizes = []
    for vs in args.voxel_sizes:
        r = {"voxel_size": vs, "rows_in": M, "table_bytes": table_bytes}
        ws.copy_(ws_counted)
        _, r["rows_out"], r["dropped"] = evaluate.map_voxel(mc, table, Twc, Kf, N, vs, vox, ws, dev)
        r["voxel_ms"], r["voxel_wall_ms"] = timed(lambda: evaluate.map_voxel(mc, table, Twc, Kf, N, vs, vox, ws, dev),
                                                  before=lambda: ws.copy_(ws_counted))
        vals = []
        for _ in range(args.runs):  # spans add events to the stream: runs of their own
            ws.copy_(ws_counted)
            lib.m3s_timing_reset()
            lib.m3s_timing_enable(1)
            evaluate.map_voxel(mc, table, Twc, Kf, N, vs, vox, ws, dev)
            torch.cuda.synchronize()
            lib.m3s_timing_enable(0)
            ms, cnt = ctypes.c_double(), ctypes.c_int()
            _lib.check(lib.m3s_timing_query(b"map_voxel", ms, cnt))
            vals.append(ms.value)
        lib.m3s_timing_reset()
        r["span_map_voxel_ms"] = statistics.median(vals)
        r["table_atomics"] = 2 * insert_runs(vs)
        r["atomics_per_s"] = r["table_atomics"] / (r["span_map_voxel_ms"] * 1e-3)
        r["kernels_ms"], r["kernels_wall_ms"] = timed(lambda: kernels(vs))
        print(f"voxel {vs}: {M} -> {r['rows_out']} rows ({M / max(r['rows_out'], 1):.2f}x), dropped {r['dropped']}; "
              f"voxel stage {r['voxel_ms']:.3f} ms (launches {r['span_map_voxel_ms']:.3f} ms, "
              f"{r['table_atomics'] / 1e6:.1f} M atomics, {r['atomics_per_s'] / 1e9:.1f} G/s), count + voxel + write {r['kernels_ms']:.3f} ms", flush=True)
        sizes.append(r)
    del out_ply, rgb, rgb_list, ws, ws_counted, vox

    # ---- the public calls ----
    res["world_points_unfiltered_ms"], res["world_points_unfiltered_wall_ms"] = timed(
        lambda: evaluate.world_points(kfs, thr, layout="ply"))
    res["world_points_nocolor_unfiltered_ms"], _ = timed(lambda: evaluate.world_points(kfs, thr, colors=False))
    print(f"world_points unfiltered: {res['world_points_unfiltered_ms']:.1f} ms, geometry only "
          f"{res['world_points_nocolor_unfiltered_ms']:.3f} ms", flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        res["save_reconstruction_unfiltered_ms"], res["save_reconstruction_unfiltered_wall_ms"] = timed(
            lambda: evaluate.save_reconstruction(tmp, "map.ply", kfs, thr))
        res["file_bytes_unfiltered"] = os.path.getsize(os.path.join(tmp, "map.ply"))
        print(f"save_reconstruction unfiltered: {res['save_reconstruction_unfiltered_wall_ms']:.1f} ms wall", flush=True)
        for r in sizes:
            vs = r["voxel_size"]
            r["world_points_ms"], r["world_points_wall_ms"] = timed(
                lambda: evaluate.world_points(kfs, thr, layout="ply", voxel_size=vs))
            r["world_points_nocolor_ms"], _ = timed(lambda: evaluate.world_points(kfs, thr, colors=False, voxel_size=vs))
            r["save_reconstruction_ms"], r["save_reconstruction_wall_ms"] = timed(
                lambda: evaluate.save_reconstruction(tmp, "thin.ply", kfs, thr, voxel_size=vs))
            r["file_bytes"] = os.path.getsize(os.path.join(tmp, "thin.ply"))
            print(f"voxel {vs}: world_points {r['world_points_ms']:.1f} ms, geometry only "
                  f"{r['world_points_nocolor_ms']:.3f} ms, save_reconstruction "
                  f"{r['save_reconstruction_wall_ms']:.1f} ms wall, {r['file_bytes']} B", flush=True)
    _lib._WS.clear()  # the cached table: room for the torch formulation's temporaries

    # ---- the torch formulation, and the same rows from both ----
    for r in sizes:
        vs = r["voxel_size"]
        r["torch_ms"], r["torch_wall_ms"] = timed(lambda: evaluate.world_points_torch(kfs, thr, voxel_size=vs),
                                                  runs=args.torch_runs, warmup=1)
        print(f"voxel {vs}: torch {r['torch_ms']:.1f} ms", flush=True)
        pts, cols, counts = evaluate.world_points(kfs, thr, voxel_size=vs)
        tp, tc, tcounts = evaluate.world_points_torch(kfs, thr, voxel_size=vs)
        # the torch rows round their points on their own (within fp32 rounding of the kernel's), so a point next to a
        # cell face can fall on the other side: the counts agree closely, not exactly
        r["torch_rows_out"] = int(tp.shape[0])
        del pts, cols, counts, tp, tc, tcounts
        _lib._WS.clear()

    out = dict(kf=Kf, H=H, W=W, calib=True, threshold=thr, points_in=Kf * N, M=M, runs=args.runs, warmup=args.warmup,
               torch_runs=args.torch_runs, sizes=sizes, **res)
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
