"""Survivor census of the refine screen, f16 rule against the int8 rule (CPU only).

Extends the replay of scripts/refine_window_stats.py: the oracle's projection search gives the start centres, then the
levels d = dmax..1 run with the exact c10::Half chain deciding every level (the oracle's rounding per step, so the
centres follow the kernel's path), and per level both survivor rules are applied to the same candidates:

  f16   S = fp32 dot of the half operands (v_dot2c's value to ~1e-7), survivors S >= max(ms - B, lmax - 2 B)
  int8  S8 = sum q8 c8 (exact), survivors S8 >= T8, the integer threshold of refine.hip ScreenI8 from
        B8 = B + E8 (tests/refine_screen8_cases.py has the restatement)

with the centre dropped after the first level, as the kernel does. Every lane is counted (the kernel scores window
outliers in place without a screen: a few hundred lanes of 262144 at 512 x 512). Reported per level: survivors per
pixel and the mean over waves (32 x 2 pixels) of the per-wave maximum, which is the survivor loop's trip count x 2.
The replay also asserts what the screen's proof promises: the exact scan's winner survives both rules.

    python scripts/refine_screen8_census.py [H W] [seed ...]      (default 512 512, the bench's seeds 1000 and 1003)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lightweight-mast3r-slam_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import oracle as O  # noqa: E402  (test infrastructure: the reference restatement)
import refine_screen8_cases as C  # noqa: E402
from m3s import synthetic  # noqa: E402

K8 = 127.0 * 127.0


def census(H, W, seed, dmax=5):
    """per level d: dict(f16=(per pixel, per-wave max), int8=(...)); raises if a rule loses the exact winner"""
    p = synthetic.make_pair(H, W, seed=seed)
    X = p["X"].numpy()
    D = p["D"].numpy()
    N = H * W
    D11h = C.half(D[0])
    qh = C.half(D[1]).reshape(N, 24)
    rays, pts, p_init = O.prep_for_iter_proj(X[:1], X[1:2])
    p_new, _ = O.iter_proj(rays, pts, p_init, 10, 1e-8, 1e-6)
    p1 = p_new.astype(np.int64)[0]
    cu, cv = p1[:, 0].copy(), p1[:, 1].copy()
    c64 = D11h.astype(np.float64)
    cmax = np.linalg.norm(c64, axis=-1).max()
    amax, c1max = np.abs(c64).max(), np.abs(c64).sum(-1).max()
    qok = np.abs(qh).max(-1) <= 1.0
    assert amax <= 1.0, "the int8 rule needs every |c_h,k| <= 1 (the kernel takes the f16 screen otherwise)"
    c8 = C.quantise8(D11h)
    q8 = C.quantise8(qh)
    B = C.bound_B(qh, cmax)
    B8 = B + C.bound_E8(q8, c1max)
    vv, uu = np.divmod(np.arange(N), W)
    wave = ((vv // 8) * ((W + 31) // 32) + uu // 32) * 4 + (vv % 8) // 2
    _, wave = np.unique(wave, return_inverse=True)
    nw = wave.max() + 1
    ms = np.zeros(N, np.float32)
    out = {}
    ar = np.arange(N)
    for d in range(dmax, 0, -1):
        off = np.arange(-3, 4) * d
        u = cu[:, None, None] + off[None, :, None]  # scan order: u outer, v inner
        v = cv[:, None, None] + off[None, None, :]
        ok = np.broadcast_to((u >= 0) & (u < W) & (v >= 0) & (v < H), (N, 7, 7)).reshape(N, 49)
        lin = (np.broadcast_to(np.clip(v, 0, H - 1), (N, 7, 7)) * W
               + np.broadcast_to(np.clip(u, 0, W - 1), (N, 7, 7))).reshape(N, 49)
        sh = np.zeros((N, 49), np.float32)
        sd = np.zeros((N, 49), np.float64)
        si = np.zeros((N, 49), np.int64)
        for k in range(24):
            ck = D11h[..., k].reshape(-1)[lin]
            sh = C.half(sh + C.half(qh[:, k, None] * ck))
            sd += qh[:, k, None].astype(np.float64) * ck
            si += q8[:, k, None].astype(np.int64) * c8[..., k].reshape(-1)[lin]
        first = d == dmax
        cand = ok.copy()  # candidates that can win
        if not first:
            cand[:, 24] = False
        # f16 rule
        sdf = sd.astype(np.float32)
        lmax = np.where(cand, sdf, -np.inf).max(1)
        T = np.maximum(ms - B, lmax - 2 * B)
        surv = cand & (sdf >= T[:, None])
        # int8 rule (integer threshold, rounded towards more survivors)
        lmax8 = np.where(cand, si, -(1 << 40)).max(1)
        tms = np.floor((ms.astype(np.float64) - B8) * K8) - 1
        T8 = np.maximum(tms, np.floor(lmax8 - 2 * B8 * K8) - 1)
        surv8 = cand & ((si >= T8[:, None]) | ~qok[:, None])
        # the exact scan: first maximum in scan order, strict '>' against the running max
        shm = np.where(ok, sh, -np.inf)
        best = np.argmax(shm, axis=1)
        m = shm[ar, best]
        win = m > ms
        assert surv[ar, best][win].all(), f"d={d}: the f16 rule lost an exact winner"
        assert surv8[ar, best][win].all(), f"d={d}: the int8 rule lost an exact winner"
        res = {}
        for name, s in (("f16", surv), ("int8", surv8)):
            ns = s.sum(1)
            wmax = np.zeros(nw)
            np.maximum.at(wmax, wave, ns)
            res[name] = (ns.mean(), wmax.mean())
        out[d] = res
        ms = np.where(win, m, ms).astype(np.float32)
        cu = np.where(win, cu - 3 * d + (best // 7) * d, cu)
        cv = np.where(win, cv - 3 * d + (best % 7) * d, cv)
    return out


def main(argv):
    H, W = (int(argv[0]), int(argv[1])) if len(argv) >= 2 else (512, 512)
    seeds = [int(a) for a in argv[2:]] or [1000, 1003]
    print(f"refine screen survivor census, {H}x{W}, dilation 5 -> 1, f16 rule -> int8 rule")
    print("survivors per pixel | mean per-wave maximum | growth of the per-wave maximum (go: below 2 = one trip)")
    for seed in seeds:
        r = census(H, W, seed)
        print(f"seed {seed}:")
        for d in sorted(r, reverse=True):
            (fp, fw), (ip, iw) = r[d]["f16"], r[d]["int8"]
            verdict = "go" if iw - fw < 2.0 else "no"
            print(f"  d={d}: {fp:5.2f} -> {ip:5.2f} | {fw:4.1f} -> {iw:4.1f} | +{iw - fw:4.2f} {verdict}")


if __name__ == "__main__":
    main(sys.argv[1:])
