"""Device side of the BA pose-solve edge suite (tests/test_gpu_ba_solve_edges.py; not collected by pytest): a HipShard
on a case's graph with a handful of points per keyframe, whose edge-sum table the test writes itself (no
linearisation), and one solve of it.

Run as a script it is the child process of test_xcd_affinity_off_is_bit_identical: the XCD stride of the launched
factor steps (M3S_BA_XCD0, csrc/ba_sparse.hip ba_xcd_stride) is read once per process, so the other setting needs a
process of its own. It solves every case named on the command line under the environment it was started with and
writes dx, Twc and the plan's wide_steps to OUT_DIR/solve.npz."""
import ctypes
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "lightweight-mast3r-slam_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import ba_solve_cases as C  # noqa: E402

NPTS = 8  # points per keyframe: the pack must run on something, the solve never reads it


def _cuda(a, dtype=None):
    t = torch.from_numpy(np.array(a, copy=True, order="C"))  # (the cases' arrays are read-only)
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


class Shard:
    """A rays-mode HipShard over directed edges ii, jj and Kp poses at C.twc0, built under the current environment
    (M3S_BA_SOLVER and the schedule variables are read while the plan is built: the plan is joined here).
    info: nL, nlev, wide_steps, dense of the plan."""

    def __init__(self, ii, jj, Kp, delta_thresh=0.0):
        from m3s import _lib
        from m3s.config import config
        from m3s.dist_ba import HipShard, ba_config

        E = len(ii)
        rng = np.random.default_rng(5)
        X = (rng.standard_normal((Kp, NPTS, 3)) * 0.3 + np.array([0.0, 0.0, 3.0])).astype(np.float32)
        self.Twc0 = C.twc0(Kp)
        self.Twc = _cuda(self.Twc0)
        self.E = E
        self.sh = HipShard(ba_config("rays", config["local_opt"]), self.Twc, _cuda(X),
                           _cuda(np.full((Kp, NPTS), 2.0, np.float32)), _cuda(ii), _cuda(jj),
                           _cuda(np.tile(np.arange(NPTS, dtype=np.int64), (E, 1))),
                           _cuda(np.ones((E, NPTS), bool), torch.bool), _cuda(np.full((E, NPTS), 2.0, np.float32)),
                           float(delta_thresh), 0, E)
        info = (ctypes.c_int * 13)()
        _lib.check(self.sh.lib.m3s_ba_plan_info(ctypes.byref(self.sh.plan), info))
        self.info = {"nL": info[1], "nlev": info[2], "wide_steps": info[3], "dense": info[4]}

    def solve(self, table):
        """Write the (E, 36) table into the shard's edge sums and solve once: (dx (n,), Twc (Kp, 8), iterations)."""
        assert table.shape == (self.E, 36)
        self.sh.edge_sums.copy_(_cuda(table).view(-1))
        self.sh.solve()
        it = self.sh.iterations()  # one readback: raises on a schedule stall (M3S_ESTALL)
        return self.sh.dx.cpu().numpy().reshape(-1).copy(), self.Twc.cpu().numpy().copy(), it


def main(names):
    out = {}
    for name in names:
        s = Shard(*C.graph(name))
        dx, T, it = s.solve(C.edge_sums(name))
        assert it == 1
        out[f"{name}_dx"], out[f"{name}_T"], out[f"{name}_wide"] = dx, T, np.int64(s.info["wide_steps"])
    np.savez(os.path.join(os.environ["OUT_DIR"], "solve.npz"), **out)
    print("BA_SOLVE_CHILD_OK", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
