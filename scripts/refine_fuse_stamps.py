"""Per-block stamps of the fused projection + refine launch (a -DM3S_REFINE_BSTAMPS build of refine.hip, chosen with
M3S_LIB; -DRT_D21_PLACE=0|1|2 picks where the D21 row loads are issued): kernel span, block durations and the split
into the LM phase (kernel start -> projection done) and the rest (tile flow, levels, store) at 512x512."""
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "lightweight-mast3r-slam_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from m3s import _lib  # noqa: E402
from m3s.matching import match  # noqa: E402
from m3s.synthetic import make_pair  # noqa: E402

lib = _lib.load()
P = make_pair(512, 512, seed=0)
X, D = P["X"].cuda(), P["D"].cuda()
nb = 512 * 512 // 256
buf = (ctypes.c_ulonglong * (8192 * 4))()
rows = []
for rep in range(8):
    match(X[:1], X[1:], D[:1], D[1:])
    torch.cuda.synchronize()
    lib.m3s_debug_refine_bstamps(buf)
    a = np.frombuffer(buf, dtype=np.uint64).reshape(8192, 4)[:nb].astype(np.float64)
    t0 = a[:, 0].min()
    start, end, lm = (a[:, 0] - t0) / 100.0, (a[:, 1] - t0) / 100.0, (a[:, 3] - t0) / 100.0  # us (100 MHz)
    if rep >= 3:  # warm
        rows.append((end.max(), start.max(), np.median(lm - start), (lm - start).max(), lm.max(),
                     np.median(end - lm), (end - lm).max(), np.median(end - start)))
r = np.array(rows)
names = ("kernel span", "last block start", "LM phase median", "LM phase max", "last LM end", "levels median",
         "levels max", "block median")
print(os.environ.get("M3S_LIB", "in-tree library"), f"({len(rows)} launches, us: median over launches [min..max])")
for k, n in enumerate(names):
    print(f"  {n:18s} {np.median(r[:, k]):7.1f}  [{r[:, k].min():.1f} .. {r[:, k].max():.1f}]")
