"""Time of RoPE2D on one MI355X: curope.rope_2d (m3s_rope2d, the HIP kernel) against m3s.rope.rope2d_torch (the same
operator in plain torch ops) on the same device.

usage: python scripts/rope2d_time.py [--inner 200] [--runs 15] [--warmup 3] [--out FILE]

Three shapes of the MASt3R ViT-L at 512 x 384 (768 patches), each in f32 and f16: six points.
  encoder_self   B=1 N=768 H=16 D=64, the q slice of the fused (B,N,3,H,D) qkv buffer (token stride 3 H D)
  decoder_self   B=2 N=768 H=12 D=64, the same strided slice
  decoder_cross  B=2 N=768 H=12 D=64, dense
Positions are the patch grid (y, x) of 24 x 32. A window is --inner back-to-back calls between two HIP events on
the stream, so a call's figure includes the launch gaps a ViT would see between consecutive small kernels; the median
of --runs windows is reported, the two implementations alternating window by window. kernel_us is the library's own
span rope2d (m3s_timing_query: events around the one launch), in calls of its own; the implied GB/s sets the
operator's 2 B N H D sizeof(dtype) bytes against it. rope2d_torch is OUR torch statement of the operator (about 12
launches, no host sync), NOT the reference's slow class, which is not on the GPU machine and adds a host sync per call.
Before timing, the kernel's result is checked against rope2d_torch's at every point. Prints one JSON line and writes it
to --out (default profiles/rope2d_time.json)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "lightweight-mast3r-slam_amd"))
import torch  # noqa: E402

SHAPES = [("encoder_self", 1, 768, 16, 64, True), ("decoder_self", 2, 768, 12, 64, True),
          ("decoder_cross", 2, 768, 12, 64, False)]
BASE, F0 = 100.0, 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rope2d_time.json"))
    args = ap.parse_args()

    import curope
    from m3s import _lib
    from m3s.rope import rope2d_torch

    assert torch.cuda.is_available(), "rope2d_time needs a HIP device"
    dev = torch.device("cuda:0")
    lib = _lib.load()

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.inner  # us per call

    points = []
    for name, B, N, H, D, strided in SHAPES:
        yy, xx = torch.meshgrid(torch.arange(24), torch.arange(32), indexing="ij")
        pos = torch.stack([yy.reshape(-1), xx.reshape(-1)], dim=-1)[None].expand(B, N, 2).contiguous().to(dev)
        for dtype in (torch.float32, torch.float16):
            g = torch.Generator().manual_seed(1)
            if strided:
                buf = torch.randn(B, N, 3, H, D, generator=g).to(dtype).to(dev)
                tok = buf[:, :, 0]
            else:
                buf = torch.randn(B, N, H, D, generator=g).to(dtype).to(dev)
                tok = buf
            # same result first (fp32 statement against the kernel: fp32 rounding of the products, then the dtype's)
            want = rope2d_torch(tok, pos, BASE, F0).float()
            got = tok.clone() if not strided else buf.clone()[:, :, 0]
            curope.rope_2d(got, pos, BASE, F0)
            tol = 1e-5 if dtype == torch.float32 else 4e-3
            err = float((got.float() - want).abs().max() / want.abs().max())
            assert err <= tol, (name, dtype, err)

            hip = lambda: curope.rope_2d(tok, pos, BASE, F0)  # noqa: E731
            ref = lambda: rope2d_torch(tok, pos, BASE, F0)  # noqa: E731
            hip_us, ref_us = [], []
            for r in range(args.warmup + args.runs):
                h, t = window(hip), window(ref)
                if r >= args.warmup:
                    hip_us.append(h)
                    ref_us.append(t)
            spans = []
            for _ in range(args.runs):  # spans add events to the stream: calls of their own
                lib.m3s_timing_reset()
                lib.m3s_timing_enable(1)
                hip()
                torch.cuda.synchronize()
                lib.m3s_timing_enable(0)
                ms, cnt = ctypes.c_double(), ctypes.c_int()
                _lib.check(lib.m3s_timing_query(b"rope2d", ms, cnt))
                spans.append(ms.value * 1e3)
            lib.m3s_timing_reset()
            nbytes = 2 * B * N * H * D * tok.element_size()
            p = dict(shape=name, B=B, N=N, H=H, D=D, strided=strided, dtype=str(dtype).replace("torch.", ""),
                     bytes=nbytes, hip_us=statistics.median(hip_us), hip_us_min=min(hip_us), hip_us_max=max(hip_us),
                     torch_us=statistics.median(ref_us), torch_us_min=min(ref_us), torch_us_max=max(ref_us),
                     kernel_us=statistics.median(spans), max_rel_diff=err)
            p["torch_over_hip"] = p["torch_us"] / p["hip_us"]
            p["kernel_gbps"] = nbytes / (p["kernel_us"] * 1e-6) / 1e9
            p["call_gbps"] = nbytes / (p["hip_us"] * 1e-6) / 1e9
            points.append(p)
            print(f"{name} {p['dtype']}: hip {p['hip_us']:.2f} us/call (kernel span {p['kernel_us']:.2f} us, "
                  f"{p['kernel_gbps']:.0f} GB/s), torch {p['torch_us']:.2f} us/call, x{p['torch_over_hip']:.1f}",
                  flush=True)

    out = dict(device=torch.cuda.get_device_name(0), base=BASE, F0=F0, inner=args.inner, runs=args.runs,
               warmup=args.warmup, baseline_is="m3s.rope.rope2d_torch (our torch statement), not the reference's class",
               points=points, hip_faster_at_all_points=all(p["hip_us"] < p["torch_us"] for p in points),
               min_torch_over_hip=min(p["torch_over_hip"] for p in points),
               max_torch_over_hip=max(p["torch_over_hip"] for p in points))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    assert out["hip_faster_at_all_points"], "curope.rope_2d must beat rope2d_torch at every point"


if __name__ == "__main__":
    main()
