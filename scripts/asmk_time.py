"""Time of the device-resident ASMK database update (m3s.retrieval.AsmkDatabase.update_features) on one MI355X.

usage: python scripts/asmk_time.py [--C 65536] [--D 1024] [--M 300] [--images 256] [--runs 50] [--warmup 5] [--out FILE]

One workload: a --C x --D codebook, --M local features per frame, a database of --images images, the reference's
parameters (k_query 5, k_build 1, alpha 3, threshold 0; retrieval k 3; min_thresh 0 instead of the config's 5e-3, so
that the returned list is not empty on these synthetic features, whose scores are ~1e-3). Inputs come from
m3s.synthetic.asmk_sequence (margin 0: no distance check at this codebook size). The database is filled through
update_features itself, then one further frame is queried:
  update_query       update_features(add_after_query=False): HIP events on the stream around the call (the device
                     span, host work between the launches included) and the wall clock to the returned list (the
                     readback included); also the library's own span asmk_update (m3s_timing_query), in runs of its own
  update_query_add   the same with add_after_query=True (the reference backend's call; the database grows by one
                     image per run)
  quantize           Codebook.quantize(k = 5) alone, the part that was on the device before
  host_numpy         tests/asmk_ref.py ForwardDb.update on the same features, the device's word ids and the exported
                     database: OUR numpy restatement of the forward-file formulation, NOT the reference's loop over an
                     inverted file (the reference does not travel to the GPU machine). Wall clock, --host-runs runs.
The medians are reported; the device list must equal the host's and the scores agree to rtol 1e-6. Prints one JSON
line and writes it to --out (default profiles/asmk_update_time.json)."""
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
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--C", type=int, default=65536)
    ap.add_argument("--D", type=int, default=1024)
    ap.add_argument("--M", type=int, default=300)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "asmk_update_time.json"))
    args = ap.parse_args()

    import asmk_ref as R
    from m3s import _lib
    from m3s.retrieval import AsmkDatabase
    from m3s.synthetic import asmk_sequence

    dev = torch.device("cuda:0")
    KQ, KB, K, THR = 5, 1, 3, 0.0
    c, feats = asmk_sequence(7, args.C, args.D, args.M, args.images + 1, margin=0)
    db = AsmkDatabase(torch.from_numpy(c).to(dev), R.asmk_params(KQ, KB), max_images=512)
    dfeats = torch.from_numpy(feats).to(dev)
    for i in range(args.images):
        db.update_features(dfeats[i], True, K, THR)
    torch.cuda.synchronize()
    q = dfeats[args.images]
    print(f"inputs ready: {db.n_images} images, {int(db.export()[2][-1])} entries", flush=True)

    def timed(fn, runs=args.runs, warmup=args.warmup):
        ev, wall = [], []
        for r in range(warmup + runs):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if r >= warmup:
                ev.append(a.elapsed_time(b))
                wall.append((t1 - t0) * 1e3)
        return statistics.median(ev), statistics.median(wall)

    lib = _lib.load()
    res = {}
    res["quantize_ms"], res["quantize_wall_ms"] = timed(lambda: db.codebook.quantize(q, KQ))
    res["update_query_ms"], res["update_query_wall_ms"] = timed(lambda: db.update_features(q, False, K, THR))
    spans = []
    for _ in range(args.runs):  # spans add events to the stream: runs of their own
        lib.m3s_timing_reset()
        lib.m3s_timing_enable(1)
        db.update_features(q, False, K, THR)
        torch.cuda.synchronize()
        lib.m3s_timing_enable(0)
        ms, cnt = ctypes.c_double(), ctypes.c_int()
        _lib.check(lib.m3s_timing_query(b"asmk_update", ms, cnt))
        spans.append(ms.value)
    lib.m3s_timing_reset()
    res["span_asmk_update_ms"] = statistics.median(spans)
    print(f"update (query): {res['update_query_ms']:.3f} ms device, {res['update_query_wall_ms']:.3f} ms wall, "
          f"span {res['span_asmk_update_ms']:.3f} ms; quantize alone {res['quantize_ms']:.3f} ms", flush=True)

    # ---- the host formulation on the same inputs (before the timed adds change the database) ----
    got = db.update_features(q, False, K, THR)
    scores = db.scores().cpu().numpy()
    ids = db.codebook.quantize(q, KQ).cpu().numpy()
    ref = R.ForwardDb(c, KQ, KB)
    ref.codes, ref.words, ref.img_ptr = db.export()
    qf = feats[args.images]
    host = []
    for _ in range(args.host_runs):
        t0 = time.perf_counter()
        want, want_scores = ref.update(qf, ids, False, K, THR)
        host.append((time.perf_counter() - t0) * 1e3)
    res["host_numpy_wall_ms"] = statistics.median(host)
    assert got == want, (got, want)
    np.testing.assert_allclose(scores, want_scores, rtol=R.RTOL, atol=R.ATOL)
    print(f"host numpy restatement: {res['host_numpy_wall_ms']:.1f} ms wall; list {got}", flush=True)

    res["update_query_add_ms"], res["update_query_add_wall_ms"] = timed(lambda: db.update_features(q, True, K, THR))
    print(f"update (query + add): {res['update_query_add_ms']:.3f} ms device, "
          f"{res['update_query_add_wall_ms']:.3f} ms wall", flush=True)

    out = dict(C=args.C, D=args.D, M=args.M, images=args.images, k_query=KQ, k_build=KB, k=K, min_thresh=THR,
               runs=args.runs, warmup=args.warmup, host_runs=args.host_runs, unique_query_words=int(len(np.unique(ids))),
               entries=int(ref.img_ptr[-1]), returned=got,
               host_is="tests/asmk_ref.py (our numpy restatement of the forward file), not the reference's loop",
               host_over_update_wall=res["host_numpy_wall_ms"] / res["update_query_wall_ms"],
               update_over_quantize=res["update_query_ms"] / res["quantize_ms"], **res)
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
