"""Alternating A/B of bench.py between library builds (the method of profiles/match_no_list_ab.json), one job on one GPU.

    python scripts/refine_screen8_ab.py OUT.json ROUNDS SERIES NAME=LIB[,ENV=VAL..] NAME=LIB ...

SERIES: plain (python bench.py --gpus 1 --steps 100 --warmup 10) or spans (the same with --full and the other legs
off, for kernels_us). Every round runs the builds in the order given, each in a fresh process with M3S_LIB = LIB
("-": the tree's library) and the extra environment. By convention the first and last builds are the parent
(parent, new.., parent_again). The bound is fixed before the runs by its definition: [min, max] of the two parent
series' medians of ms_per_step, widened on both sides by the larger of their sample standard deviations; a build
gains only if its median lies below that band. A run that fails ends the job.
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_once(series, lib, extra):
    env = dict(os.environ)
    env.pop("M3S_LIB", None)
    if lib != "-":
        env["M3S_LIB"] = os.path.abspath(lib)
    env.update(extra)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "100", "--warmup", "10"]
    if series == "spans":
        cmd += ["--full", "--no-cpu", "--no-ba", "--no-peaks", "--no-retrieval", "--no-store"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-2000:])
        raise SystemExit(f"bench.py failed with {p.returncode}")
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)


def find_kernels_us(r):
    """kernels_us wherever the bench line keeps it"""
    if isinstance(r, dict):
        if "kernels_us" in r:
            return r["kernels_us"]
        for v in r.values():
            k = find_kernels_us(v)
            if k is not None:
                return k
    return None


def main():
    out, rounds, series = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    builds = []
    for spec in sys.argv[4:]:
        name, rest = spec.split("=", 1)
        parts = rest.split(",")
        builds.append((name, parts[0], dict(p.split("=", 1) for p in parts[1:])))
    runs = []
    for rnd in range(1, rounds + 1):
        for name, lib, extra in builds:
            r = run_once(series, lib, extra)
            rec = {"round": rnd, "build": name, "value": r["value"], "ms_per_step": r["ms_per_step"]}
            k = find_kernels_us(r)
            if k is not None:
                rec["kernels_us"] = {n: k[n] for n in ("prep_rays", "refine_lin", "gn_iters") if n in k}
            runs.append(rec)
            print(json.dumps(rec), flush=True)
        with open(out + ".partial", "w") as f:  # what a job that is cut short leaves behind
            json.dump(runs, f)
    names = [b[0] for b in builds]
    ms = {n: [r["ms_per_step"] for r in runs if r["build"] == n] for n in names}
    med = {n: statistics.median(v) for n, v in ms.items()}
    sd = {n: statistics.stdev(v) if len(v) > 1 else 0.0 for n, v in ms.items()}
    pa, pb = names[0], names[-1]
    widen = max(sd[pa], sd[pb])
    band = [min(med[pa], med[pb]) - widen, max(med[pa], med[pb]) + widen]
    res = {"series": series, "rounds": rounds, "builds": {n: {"lib": l, "env": e} for n, l, e in builds},
           "runs": runs, "ms_per_step": {"medians": med, "stdev": sd, "band": band,
                                         "verdict": {n: ("below" if med[n] < band[0] else "above" if med[n] > band[1]
                                                         else "inside") for n in names[1:-1]}}}
    if all("kernels_us" in r for r in runs):
        res["kernels_us_medians"] = {
            n: {k: statistics.median(r["kernels_us"][k] for r in runs if r["build"] == n)
                for k in runs[0]["kernels_us"]} for n in names}
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    os.remove(out + ".partial")
    print(json.dumps({k: res[k] for k in res if k != "runs"}))


if __name__ == "__main__":
    main()
