"""Per-block stamps of the fused projection + refine launch (a -DM3S_REFINE_BSTAMPS build of refine.hip, chosen with
M3S_LIB): kernel span, block durations and the split into the LM phase (kernel start -> projection done) and the rest
(tile flow, levels, store) at 512x512. The D21 row loads are issued behind the LM loop; the placements it was compared
with (profiles/match_fuse_proj_trace.txt) build at the tag refine-experiments-r6."""
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
rows, ranks = [], []


def by_age_rank(a, start, end):
    """median block duration by age rank within the block's CU. The CU is (XCD = block index mod 8: the dispatcher
    deals blocks to the XCDs in turn; SE_ID, SH_ID, CU_ID of the HW_ID stamp: bits 15:13, 12, 11:8); the rank orders
    the CU's blocks by start stamp, then block index (the arbiter's age is the dispatch order). Only CUs that hold
    exactly four blocks of the launch count."""
    hw = a[:, 2].astype(np.int64)
    key = (np.arange(len(a)) % 8) * 65536 + (hw & 0xff00)
    out = [[] for _ in range(4)]
    for k in np.unique(key):
        i = np.nonzero(key == k)[0]
        if len(i) != 4:
            continue
        i = i[np.lexsort((i, start[i]))]
        for r in range(4):
            out[r].append(end[i[r]] - start[i[r]])
    return [float(np.median(o)) if o else float("nan") for o in out], len(out[0])


for rep in range(8):
    match(X[:1], X[1:], D[:1], D[1:])
    torch.cuda.synchronize()
    lib.m3s_debug_refine_bstamps(buf)
    a = np.frombuffer(buf, dtype=np.uint64).reshape(8192, 4)[:nb].astype(np.float64)
    t0 = a[:, 0].min()
    start, end, lm = (a[:, 0] - t0) / 100.0, (a[:, 1] - t0) / 100.0, (a[:, 3] - t0) / 100.0  # us (100 MHz)
    if rep >= 3:  # warm
        rows.append((end.max(), start.max(), np.median(lm - start), (lm - start).max(), lm.max(),
                     np.median(end - lm), (end - lm).max(), np.median(end - start), (end - start).max(),
                     (end - start).min()))
        ranks.append(by_age_rank(a, start, end))
r = np.array(rows)
names = ("kernel span", "last block start", "LM phase median", "LM phase max", "last LM end", "levels median",
         "levels max", "block median", "block max", "block min")
print(os.environ.get("M3S_LIB", "in-tree library"), f"({len(rows)} launches, us: median over launches [min..max])")
for k, n in enumerate(names):
    print(f"  {n:18s} {np.median(r[:, k]):7.1f}  [{r[:, k].min():.1f} .. {r[:, k].max():.1f}]")
rk = np.array([x[0] for x in ranks])
print(f"  block duration by age rank within its CU ({ranks[-1][1]} CUs with four blocks), median over launches:")
print("   ", "  ".join(f"rank {k}: {np.median(rk[:, k]):6.1f}" for k in range(4)))
