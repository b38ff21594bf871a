"""The segment between the last GN solve and the host seeing the published frame result, per tracked frame.

Two modes:
  run     python scripts/publish_segment.py run OUT.json [frames]
          (under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python ...`): tracks `frames` 512x512 calib
          frames like the bench and stamps the return of every m3s_track call (the host has just seen the published
          generation) on CLOCK_MONOTONIC, CLOCK_BOOTTIME and CLOCK_REALTIME.
  report  python scripts/publish_segment.py report OUT.json DIR [skip]
          matches the k-th m3s_track return with the k-th gn_loop / fuse_kernel rows of the kernel trace and prints
          the medians of: GN end -> fuse start, fuse start -> host saw the result, GN end -> host saw the result,
          host saw the result -> next prep_rays start, and the two kernels' durations. The host clock used is the
          one whose stamps fall nearest the fuse launch (the trace's clock domain)."""
import csv
import glob
import json
import os
import sys
import time

import numpy as np

CLOCKS = ("CLOCK_MONOTONIC", "CLOCK_BOOTTIME", "CLOCK_REALTIME")


def run(out, frames):
    import torch

    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, ".."))
    sys.path.insert(0, os.path.join(here, "..", "lightweight-mast3r-slam_amd"))
    from m3s import _lib, tracker
    from m3s.config import config
    from m3s.frame import Frame, Keyframes
    from m3s.sim3 import Sim3
    from m3s.synthetic import SyntheticModel, make_pair

    lib = _lib.load()
    orig_track = lib.m3s_track
    ids = [getattr(time, c) for c in CLOCKS]
    stamps = []

    class LibProxy:
        def __getattr__(self, n):
            return getattr(lib, n)

        def m3s_track(self, *a):
            r = orig_track(*a)
            stamps.append([time.clock_gettime_ns(i) for i in ids])
            return r

    proxy = LibProxy()
    _lib.load = lambda: proxy
    dev = torch.device("cuda:0")
    H = W = 512
    config["use_calib"] = True
    pairs = [make_pair(H, W, seed=r) for r in range(6)]
    model = SyntheticModel(pairs, dev)
    kf = Frame(0, (H, W), T_WC=Sim3.Identity(1, device=dev))
    kf.K = pairs[0]["K"].to(dev)
    kf.update_pointmap(pairs[0]["Xk"].to(dev), pairs[0]["Ck"].to(dev))
    kfs = Keyframes()
    kfs.append(kf)
    tr = tracker.FrameTracker(model, kfs, dev)
    for i in range(frames):
        tr.track(Frame(i, (H, W), T_WC=kf.T_WC))
    torch.cuda.synchronize()
    json.dump({"clocks": CLOCKS, "stamps": stamps}, open(out, "w"))


def report(out, trace_dir, skip):
    rec = json.load(open(out))
    st = np.array(rec["stamps"], dtype=np.int64)
    f = glob.glob(f"{trace_dir}/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    span = lambda key: np.array([(int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows
                                 if key in r["Kernel_Name"]], dtype=np.int64)
    gn, fuse, prep = span("gn_loop"), span("fuse_kernel"), span("prep_rays")
    assert len(gn) == len(fuse) == len(st), (len(gn), len(fuse), len(st))
    k = int(np.argmin([abs(np.median(st[:, c] - fuse[:, 0])) for c in range(st.shape[1])]))
    seen = st[:, k]
    med = lambda v: float(np.median(v[skip:])) / 1e3
    p = lambda v, q: float(np.percentile(v[skip:], q)) / 1e3
    series = {
        "GN end -> fuse start": fuse[:, 0] - gn[:, 1],
        "fuse start -> host saw result": seen - fuse[:, 0],
        "GN end -> host saw result": seen - gn[:, 1],
        "GN start -> host saw result": seen - gn[:, 0],
        "gn_loop duration": gn[:, 1] - gn[:, 0],
        "fuse_kernel duration": fuse[:, 1] - fuse[:, 0],
    }
    if len(prep) == len(st):
        series["host saw result -> next prep_rays start"] = prep[1:, 0] - seen[:-1]
        series["prep_rays start -> next prep_rays start"] = prep[1:, 0] - prep[:-1, 0]
    print(f"{len(st)} frames, first {skip} skipped; host clock matching the trace: {rec['clocks'][k]}")
    for name, v in series.items():
        print(f"{name:42s} median {med(v):8.2f} us  p10 {p(v, 10):8.2f}  p90 {p(v, 90):8.2f}")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 400)
    else:
        report(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 100)
