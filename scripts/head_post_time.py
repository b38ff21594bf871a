"""Time of the dense head tail on one MI355X: from the DPT output and the MLP output of one view to the stacked X, C,
D, Q of a two-view window, three ways on the same device in the same run.

usage: python scripts/head_post_time.py [--inner 50] [--runs 15] [--warmup 3] [--out FILE]

Shapes 512 x 512, 384 x 512, 320 x 512, F = 24, two_confs, modes ('exp', -inf, inf) / ('exp', 1, inf) / ('exp', 0, inf),
img_downsample 1. Every leg starts from pts (1, 4, H, W) and feat (1, S, 25 * 256) per view and ends with the stacked
(2, H, W, .) arrays that mast3r_asymmetric_inference returns (mast3r_utils.py:210-216):
  head_tail     m3s.head.head_tail (layout TOKENS), each view written into its slot through out=: one launch per view
  postprocess   torch's transpose / view / pixel_shuffle / cat, then m3s.head.postprocess (layout CAT, what the hook's
                postprocess binding alone gives), then [0] and the four torch.stack
  torch_tail    m3s.head.head_tail_torch, the stock tail in torch ops, then [0] and the four torch.stack
A window is --inner two-view frames back to back between two HIP events on the stream, so a figure includes the launch
gaps the ViT's stream would see; the median of --runs windows is reported per VIEW, the three legs alternating window by
window. kernel_us is the library's own span head_post (m3s_timing_query: events around the one launch) in calls of
their own; the implied bytes/s set the 232 B/px a view must move (116 in, 116 out) against it. head_tail_torch is OUR
torch statement of the tail, not the reference's module, which is not on the GPU machine. Before timing, the three
results are compared. Prints one JSON line and writes it to --out (default profiles/head_post_time.json)."""
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
import torch.nn.functional as F  # noqa: E402

SHAPES = [(512, 512), (384, 512), (320, 512)]
FD = 24
INF = float("inf")
DEPTH, CONF, DCONF = ("exp", -INF, INF), ("exp", 1, INF), ("exp", 0, INF)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "head_post_time.json"))
    args = ap.parse_args()

    from m3s import _lib, head

    assert torch.cuda.is_available(), "head_post_time needs a HIP device"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    modes = dict(two_confs=True, conf_mode=CONF, desc_conf_mode=DCONF)

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / (2 * args.inner)  # us per view

    points = []
    for H, W in SHAPES:
        g = torch.Generator().manual_seed(1)
        S = (H // 16) * (W // 16)
        views = [(torch.randn(1, 4, H, W, generator=g).to(dev), torch.randn(1, S, (FD + 1) * 256, generator=g).to(dev))
                 for _ in range(2)]
        stacked = tuple(torch.empty((2, H, W) + t, device=dev) for t in ((3,), (), (FD,), ()))

        def fused():
            for v, (pts, feat) in enumerate(views):
                head.head_tail(pts, feat, H, W, out=tuple(t[v:v + 1] for t in stacked), **modes)
            return stacked

        def stack(res):
            return tuple(torch.stack([r[k][0] for r in res]) for k in ("pts3d", "conf", "desc", "desc_conf"))

        def cat_post():
            res = []
            for pts, feat in views:
                local = F.pixel_shuffle(feat.transpose(-1, -2).view(1, -1, H // 16, W // 16), 16)
                res.append(head.postprocess(torch.cat([pts, local], dim=1), DEPTH, CONF, desc_dim=FD, desc_mode="norm",
                                            two_confs=True, desc_conf_mode=DCONF))
            return stack(res)

        def torch_tail():
            res = [dict(zip(("pts3d", "conf", "desc", "desc_conf"), head.head_tail_torch(pts, feat, H, W, **modes)))
                   for pts, feat in views]
            return stack(res)

        a, b, c = [t.clone() for t in fused()], cat_post(), torch_tail()
        diffs = []
        for x, y, z in zip(a, b, c):
            assert torch.equal(x, y), "TOKENS and CAT must agree bit for bit"
            diffs.append(float(((x - z).abs() / z.abs().clamp_min(1e-30)).max()))
        assert max(diffs) < 1e-4, diffs

        legs = dict(head_tail=fused, postprocess=cat_post, torch_tail=torch_tail)
        us = {k: [] for k in legs}
        for r in range(args.warmup + args.runs):
            for k, fn in legs.items():
                t = window(fn)
                if r >= args.warmup:
                    us[k].append(t)
        spans = []
        for _ in range(args.runs):  # spans add events to the stream: calls of their own
            lib.m3s_timing_reset()
            lib.m3s_timing_enable(1)
            fused()
            torch.cuda.synchronize()
            lib.m3s_timing_enable(0)
            ms, cnt = ctypes.c_double(), ctypes.c_int()
            _lib.check(lib.m3s_timing_query(b"head_post", ms, cnt))
            assert cnt.value == 2
            spans.append(ms.value * 1e3 / 2)
        lib.m3s_timing_reset()
        nbytes = 2 * 4 * (4 + FD + 1) * H * W  # per view
        p = dict(H=H, W=W, F=FD, bytes_per_view=nbytes, kernel_us=statistics.median(spans), max_rel_diff_vs_torch=max(diffs))
        for k in legs:
            p[k + "_us"], p[k + "_us_min"], p[k + "_us_max"] = statistics.median(us[k]), min(us[k]), max(us[k])
        p["kernel_tbps"] = nbytes / (p["kernel_us"] * 1e-6) / 1e12
        p["call_tbps"] = nbytes / (p["head_tail_us"] * 1e-6) / 1e12
        p["torch_over_head_tail"] = p["torch_tail_us"] / p["head_tail_us"]
        p["torch_over_postprocess"] = p["torch_tail_us"] / p["postprocess_us"]
        points.append(p)
        print(f"{H}x{W}: head_tail {p['head_tail_us']:.1f} us/view (kernel span {p['kernel_us']:.1f} us, "
              f"{p['kernel_tbps']:.2f} TB/s), postprocess {p['postprocess_us']:.1f}, torch tail {p['torch_tail_us']:.1f}, "
              f"x{p['torch_over_head_tail']:.1f}", flush=True)

    out = dict(device=torch.cuda.get_device_name(0), inner=args.inner, runs=args.runs, warmup=args.warmup,
               baseline_is="m3s.head.head_tail_torch (our torch statement of the stock tail), not the reference's module",
               unit="us per view, median of the windows", points=points,
               head_tail_faster_at_all_shapes=all(p["head_tail_us"] < p["torch_tail_us"] for p in points),
               postprocess_faster_at_all_shapes=all(p["postprocess_us"] < p["torch_tail_us"] for p in points))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
