"""Time of the frame ingest on one MI355X box: from an image in host memory to the ViT-ready (1,3,H,W) device tensor,
m3s.ingest.ingest (upload of the image as it is, then the two HIP launches of m3s_ingest) against the host statement
(m3s.ingest.resize_img: Pillow, the torch tail) plus the upload of its result, on the same box in the same run.

usage: python scripts/ingest_time.py [--inner 20] [--runs 9] [--warmup 2] [--out FILE]

Three sources: 640 x 480 uint8, 640 x 480 float32 (what the reference's loaders hand to create_frame) and 1920 x 1080
uint8. A window is --inner back-to-back calls, each ending in a device synchronise, on the host's clock: both paths
start from host memory, so the host's share counts. The two paths alternate window by window; the median of --runs
windows is reported with its minimum and maximum. device_us is the same for a source already on the device (the two
launches and the output allocations, no upload); span_us is the library's own span `ingest` (m3s_timing_query: events
around the two launches), in calls of its own. The host statement's time depends on the box's CPU and on what else
runs there. Before timing, the two paths' outputs are compared for equality at every point. Prints one JSON line and
writes it to --out (default profiles/ingest_time.json)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "lightweight-mast3r-slam_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

POINTS = [("640x480_u8", 480, 640, "uint8"), ("640x480_f32", 480, 640, "float32"), ("1920x1080_u8", 1080, 1920, "uint8")]


def make_image(H, W):
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    return ((y * 131 + x * 71 + c * 57 + ((x * y) % 251) * 3 + ((x * x + y) >> 2)) & 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ingest_time.json"))
    args = ap.parse_args()

    import PIL

    from m3s import _lib
    from m3s.ingest import ingest, resize_img

    assert torch.cuda.is_available(), "ingest_time needs a HIP device"
    dev = torch.device("cuda:0")
    lib = _lib.load()

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.inner):
            fn()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / args.inner  # us per call

    points = []
    for name, H, W, dtype in POINTS:
        u8 = make_image(H, W)
        src = u8 if dtype == "uint8" else u8.astype(np.float32) / np.float32(255.0)
        src_dev = torch.from_numpy(src).to(dev)

        hip = lambda: ingest(src, 512, downsample=1, device=dev)[0]  # noqa: E731
        host = lambda: resize_img(src, 512)["img"].to(dev)  # noqa: E731
        on_dev = lambda: ingest(src_dev, 512, downsample=1, device=dev)[0]  # noqa: E731
        a, b = hip(), host()
        torch.cuda.synchronize()
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), name

        hip_us, host_us, dev_us = [], [], []
        for r in range(args.warmup + args.runs):
            h, t, d = window(hip), window(host), window(on_dev)
            if r >= args.warmup:
                hip_us.append(h)
                host_us.append(t)
                dev_us.append(d)
        spans = []
        for _ in range(args.runs):  # spans add events to the stream: calls of their own
            lib.m3s_timing_reset()
            lib.m3s_timing_enable(1)
            on_dev()
            torch.cuda.synchronize()
            lib.m3s_timing_enable(0)
            ms, cnt = ctypes.c_double(), ctypes.c_int()
            _lib.check(lib.m3s_timing_query(b"ingest", ms, cnt))
            spans.append(ms.value * 1e3)
        lib.m3s_timing_reset()
        p = dict(source=name, H=H, W=W, dtype=dtype, out_shape=list(a.shape), upload_bytes=int(src.nbytes),
                 hip_us=statistics.median(hip_us), hip_us_min=min(hip_us), hip_us_max=max(hip_us),
                 host_us=statistics.median(host_us), host_us_min=min(host_us), host_us_max=max(host_us),
                 device_us=statistics.median(dev_us), span_us=statistics.median(spans), outputs_equal=True)
        p["host_over_hip"] = p["host_us"] / p["hip_us"]
        points.append(p)
        print(f"{name}: device path {p['hip_us']:.0f} us/frame (on-device source {p['device_us']:.0f} us, span "
              f"{p['span_us']:.1f} us), host statement + upload {p['host_us']:.0f} us/frame, x{p['host_over_hip']:.1f}",
              flush=True)

    out = dict(device=torch.cuda.get_device_name(0), cpus=os.cpu_count(), torch_threads=torch.get_num_threads(),
               pillow=PIL.__version__, inner=args.inner, runs=args.runs, warmup=args.warmup,
               baseline_is="m3s.ingest.resize_img (Pillow + torch ops on the host) and the upload of its tensor",
               points=points, hip_faster_at_all_points=all(p["hip_us"] < p["host_us"] for p in points))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
