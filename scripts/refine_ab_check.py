"""Two library builds side by side on match(): output hashes, or the M3S_REFINE_STATS counters (not a test).

    python scripts/refine_ab_check.py hashes   PARENT_LIB TREE_LIB [OUT.json]
    python scripts/refine_ab_check.py counters PARENT_STATS_LIB TREE_STATS_LIB [OUT.json]

hashes: SHA-1 of idx and valid at 512x512, 384x512 and 50x70, each cold and with a random warm start, under default,
M3S_REFINE_SCREEN8=0, M3S_REFINE_SCREEN=0 and M3S_MATCH_FUSE_PROJ=0.
counters (builds with -DM3S_REFINE_STATS, scripts/build_variant.sh): the 64 counters of one match() call on the 512x512
seed-0 pair and on ladder_0p03, lane_fallback and layouts_d3 of tests/refine_screen8_cases.py, under default and
M3S_REFINE_SCREEN8=0: per level d the window outlier lanes [2d] and waves [2d + 1], the survivors' sum [32 + 2d] and
per-wave maximum [33 + 2d]. Equal outputs alone do not show an unchanged screen: a looser threshold gives the same idx.

Each build runs in one fresh process (M3S_LIB); this process only starts them, prints the two columns and exits 1 on
a difference. A child that fails ends the job.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = (("default", {}), ("screen8_off", {"M3S_REFINE_SCREEN8": "0"}), ("screen_off", {"M3S_REFINE_SCREEN": "0"}),
        ("unfused", {"M3S_MATCH_FUSE_PROJ": "0"}))
SWITCHES = ("M3S_REFINE_SCREEN8", "M3S_REFINE_SCREEN", "M3S_MATCH_FUSE_PROJ")


def child(mode):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "lightweight-mast3r-slam_amd"), os.path.join(ROOT, "tests")]
    import numpy as np
    import torch

    from m3s import _lib
    from m3s.config import config
    from m3s.matching import match
    from m3s.synthetic import make_pair

    def run(args, env):
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        idx, valid = match(*args)
        torch.cuda.synchronize()
        return idx.cpu().numpy(), valid.cpu().numpy()

    out = {}
    if mode == "hashes":
        for (h, w) in ((512, 512), (384, 512), (50, 70)):
            P = make_pair(h, w, seed=0)
            X, D = P["X"].cuda(), P["D"].cuda()
            warm = torch.from_numpy(np.random.default_rng(5).integers(0, h * w, size=(1, h * w))).cuda()
            for start, extra in (("cold", []), ("warm", [warm])):
                for name, env in ENVS:
                    idx, valid = run([X[:1], X[1:], D[:1], D[1:]] + extra, env)
                    out[f"{h}x{w} {start} {name}"] = [hashlib.sha1(idx.tobytes()).hexdigest(),
                                                      hashlib.sha1(valid.tobytes()).hexdigest()]
    else:
        import refine_screen8_cases as C

        lib = _lib.load()
        cases = dict(C.gpu_cases())
        P = make_pair(512, 512, seed=0)
        runs = [("512x512 seed 0", [P["X"][:1], P["X"][1:], P["D"][:1], P["D"][1:]], 5)]
        for n in ("ladder_0p03", "lane_fallback", "layouts_d3"):
            c = cases[n]
            runs.append((n, [torch.from_numpy(np.ascontiguousarray(c[k])) for k in ("X11", "X21", "D11", "D21")],
                         c["dilation_max"]))
        buf = (ctypes.c_ulonglong * 64)()
        for n, args, dmax in runs:
            config["matching"]["dilation_max"] = dmax
            args = [a.cuda() for a in args]
            for name, env in ENVS[:2]:
                assert lib.m3s_debug_refine_stats(buf, 1) == 0
                run(args, env)
                assert lib.m3s_debug_refine_stats(buf, 1) == 0
                out[f"{n} {name}"] = list(buf)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    mode, libs = sys.argv[1], sys.argv[2:4]
    if mode.startswith("child-"):
        return child(mode[6:])
    cols = []
    for lib in libs:
        env = dict(os.environ, M3S_LIB=os.path.abspath(lib))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "child-" + mode], env=env, capture_output=True,
                           text=True, timeout=240)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-2000:])
            raise SystemExit(f"{lib}: child failed with {p.returncode}")
        cols.append(json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]))
    equal = True
    for k in cols[0]:
        a, b = cols[0][k], cols[1].get(k)
        equal &= a == b
        if mode == "hashes":
            print(f"{k:32s} {a[0][:12]} {a[1][:12]} | {b[0][:12]} {b[1][:12]} {'==' if a == b else '!='}")
        else:
            nz = [i for i in range(64) if a[i] or b[i]]
            print(f"{k}: {'equal' if a == b else 'DIFFERENT'}")
            for i in nz:
                print(f"   [{i:2d}] {a[i]:10d} {b[i]:10d}")
    print("all equal" if equal else "DIFFERENT")
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as f:
            json.dump({"mode": mode, "parent": cols[0], "tree": cols[1], "equal": equal}, f, indent=1)
    raise SystemExit(0 if equal else 1)


if __name__ == "__main__":
    main()
