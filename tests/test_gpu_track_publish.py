"""The tracked frame's result published from the GN launch (M3S_TRACK_PUBLISH_GN, default on) against the
publish-from-fuse path (M3S_TRACK_PUBLISH_GN=0).

Only where the unique-match count and the publish run changes, not the arithmetic, so every comparison between the two
settings is bitwise: poses, status, iterations, cost, the three counts, the fused keyframe, both average confidences
and the store slot's counters. n_unique is also checked against |unique(idx[valid])| computed on the host.

Shapes: 3x5 (one padded 16-byte map entry, one block, seven XCD shards empty), 48x64 (3 blocks, fewer than the 8
shards), 96x136 (13056 points: the map's 816 entries are no multiple of the counting threads, 13 blocks over 8 shards)."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ENV = "M3S_TRACK_PUBLISH_GN"


@contextlib.contextmanager
def _captured_matches():
    """idx_f2k / valid_match of every track() call, as the tracker got them from the matcher."""
    import m3s.tracker as T

    cap = {}
    orig = T.mast3r_match_asymmetric

    def capture(*a, **k):
        out = orig(*a, **k)
        cap["idx"], cap["valid"] = out[0], out[1]
        return out

    T.mast3r_match_asymmetric = capture
    try:
        yield cap
    finally:
        T.mast3r_match_asymmetric = orig


_PAIRS = {}


def _pair(H, W, seed):
    from m3s.synthetic import make_pair

    if (H, W, seed) not in _PAIRS:
        # the default 3.3-pixel flow would carry most of a 3x5 image out of view: a sub-pixel one there
        kw = {"flow": (0.4, -0.3), "rot_deg": 0.2} if min(H, W) < 8 else {}
        _PAIRS[(H, W, seed)] = make_pair(H, W, seed=seed, **kw)
    return _PAIRS[(H, W, seed)]


class Rig:
    """One keyframe and one tracker at H x W; every rig shares the library's one tracking workspace per stream."""

    def __init__(self, H, W, calib, seeds=(0,), store=None):
        from m3s.config import config
        from m3s.frame import Frame, Keyframes
        from m3s.sim3 import Sim3
        from m3s.synthetic import SyntheticModel
        from m3s.tracker import FrameTracker

        self.H, self.W, self.calib = H, W, calib
        config["use_calib"] = calib
        pairs = [_pair(H, W, s) for s in seeds]
        if store is None:
            self.kf = Frame(0, (H, W), T_WC=Sim3.Identity(1, device="cuda"))
            self.kf.K = pairs[0]["K"].cuda()
            self.kf.update_pointmap(pairs[0]["Xk"].cuda(), pairs[0]["Ck"].cuda())
            self.kfs = Keyframes()
            self.kfs.append(self.kf)
        else:
            self.kf, self.kfs = None, store
        self.tr = FrameTracker(SyntheticModel(pairs, "cuda"), self.kfs, "cuda")
        self.n = 0

    def step(self):
        """Track one frame; the record of everything the two publish paths must agree on."""
        from m3s.config import config
        from m3s.frame import Frame
        from m3s.sim3 import Sim3

        config["use_calib"] = self.calib
        self.n += 1
        frame = Frame(self.n, (self.H, self.W), T_WC=Sim3.Identity(1, device="cuda"))
        with _captured_matches() as cap:
            new_kf, info, reloc = self.tr.track(frame)
        r = self.tr.last_result
        idx, v = cap["idx"].reshape(-1), cap["valid"].reshape(-1).bool()
        host_unique = int(torch.unique(idx[v]).numel())
        assert r.n_unique == host_unique, (self.H, self.W, r.n_unique, host_unique)
        kf = self.kfs[len(self.kfs) - 1]
        rec = {"new_kf": bool(new_kf), "reloc": bool(reloc), "T_WCf": list(r.T_WCf), "T_CkCf": list(r.T_CkCf),
               "cost": np.float64(r.cost).tobytes(), "iters": r.iters, "status": r.status, "n_valid_kf": r.n_valid_kf,
               "n_valid_opt": r.n_valid_opt, "n_unique": r.n_unique, "frame_T_WC": frame.T_WC.data.cpu().clone(),
               "kf_X": kf.X_canon.cpu().clone(), "kf_C": kf.C.cpu().clone(), "kf_N": int(kf.N)}
        if not reloc:
            rec["Ck_avg"], rec["Cf_avg"] = info[1].cpu().clone(), info[3].cpu().clone()
        return rec


def _same(a, b, what=""):
    assert type(a) is type(b), what
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], f"{what}.{k}")
    elif isinstance(a, (list, tuple)) and a and isinstance(a[0], (dict, list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{what}[{i}]")
    elif torch.is_tensor(a):
        assert torch.equal(a, b), what
    else:
        assert a == b, (what, a, b)


def _both(monkeypatch, run, extra_env=None):
    """run() under the fuse-launch publish ("0") and the GN-launch publish ("1"); returns both outputs, compared."""
    from m3s.config import reset_config

    outs = []
    for setting in ("0", "1"):
        monkeypatch.setenv(ENV, setting)
        for k, v in (extra_env or {}).items():
            monkeypatch.setenv(k, v)
        reset_config()
        outs.append(run())
    _same(outs[0], outs[1], "publish_gn 0 vs 1")
    return outs


@pytest.mark.parametrize("H,W,calib", [(3, 5, False), (48, 64, False), (48, 64, True), (96, 136, False)])
def test_publish_from_gn_bit_identical(monkeypatch, H, W, calib):
    def run():
        rig = Rig(H, W, calib)
        return [rig.step(), rig.step()]

    old, new = _both(monkeypatch, run)
    if H >= 48:  # tracked, not skipped (at 3x5 whatever the tracker decides is compared, and the count is checked)
        assert all(not r["reloc"] and r["iters"] >= 1 for r in new)


def test_publish_when_gn_ends_at_iteration_0(monkeypatch):
    """max_iters = 1: no second hand-off; the count made during the iteration-0 solve is all there is."""
    from m3s.config import config

    def run():
        config["tracking"]["max_iters"] = 1
        rig = Rig(48, 64, False)
        return [rig.step(), rig.step()]

    old, new = _both(monkeypatch, run)
    assert all(r["iters"] == 1 and not r["reloc"] for r in new)


def test_publish_skipped_frame_and_the_next(monkeypatch):
    """A skipped frame (min_match_frac above any achievable fraction) is published with its counts, fuses nothing,
    and leaves the scratch clean: the next frame on the same workspace is right (counted in the GN launch's tail)."""
    from m3s import _lib
    from m3s.config import config

    def run():
        rig = Rig(48, 64, False, seeds=(0, 1))
        X0, C0 = rig.kf.X_canon.clone(), rig.kf.C.clone()
        config["tracking"]["min_match_frac"] = 2.0
        skipped = rig.step()
        assert skipped["reloc"] and skipped["status"] == _lib.TRACK_SKIPPED
        assert torch.equal(rig.kf.X_canon, X0) and torch.equal(rig.kf.C, C0) and rig.kf.N == 1
        config["tracking"]["min_match_frac"] = 0.05
        tracked = rig.step()
        assert not tracked["reloc"]
        return [skipped, tracked, rig.step()]

    _both(monkeypatch, run)


def test_publish_cholesky_failure(monkeypatch):
    """No valid residual (H = 0): the failed frame is published from the iteration-0 exit."""
    from m3s import _lib
    from m3s.config import config

    def run():
        config["tracking"]["min_match_frac"] = 0.0
        config["tracking"]["Q_conf"] = 1e9
        rig = Rig(48, 64, False)
        failed = rig.step()
        assert failed["reloc"] and failed["status"] == _lib.TRACK_CHOLESKY_FAILED
        config["tracking"]["Q_conf"] = 1.5
        return [failed, rig.step()]

    _both(monkeypatch, run)


def test_publish_sequence_across_image_sizes(monkeypatch):
    """Four frames at 48x64, one at 96x136, then 48x64 again, all on one workspace: counts and poses equal the
    fuse-launch path at every frame (the scratch is re-initialised when the size changes, and clean otherwise)."""

    def run():
        small = Rig(48, 64, True, seeds=(0, 1, 2))
        out = [small.step() for _ in range(4)]
        out.append(Rig(96, 136, True).step())
        out.append(small.step())
        return out

    old, new = _both(monkeypatch, run)
    assert all(not r["reloc"] for r in new)


def test_publish_with_store_slot(monkeypatch):
    """Fusion into a SharedKeyframes slot: the slot's X, C, N, N_updates and is_dirty equal the fuse-launch path's."""
    import multiprocessing as mp

    from m3s.config import config
    from m3s.frame import Frame, SharedKeyframes
    from m3s.sim3 import Sim3

    H, W = 48, 64
    P = _pair(H, W, 0)
    manager = mp.get_context("spawn").Manager()

    def run():
        config["use_calib"] = True
        kfs = SharedKeyframes(manager, H, W, buffer=4, device="cuda", feat_dim=64)
        kf = Frame(0, (H, W), T_WC=Sim3.Identity(1, device="cuda"))
        kf.K = P["K"].cuda()
        kf.update_pointmap(P["Xk"].cuda(), P["Ck"].cuda())
        g = torch.Generator().manual_seed(3)
        kf.img = torch.rand(3, H, W, generator=g).cuda()
        kf.uimg = torch.rand(H, W, 3, generator=g)
        kf.img_shape = torch.tensor([[H, W]], dtype=torch.int).cuda()
        kf.img_true_shape = kf.img_shape.clone()
        kf.feat = torch.rand(1, H * W // 256, 64, generator=g).cuda()
        kf.pos = torch.randint(0, 100, (1, H * W // 256, 2), generator=g).cuda()
        kfs.append(kf)
        kfs.set_intrinsics(P["K"].cuda())
        kfs.get_dirty_idx()  # clean
        rig = Rig(H, W, True, store=kfs)
        recs = [rig.step() for _ in range(3)]
        torch.cuda.synchronize()
        slot = {k: getattr(kfs, k).cpu().clone() for k in ("X", "C", "N", "N_updates", "is_dirty", "T_WC")}
        assert int(slot["N"][0]) == 4 and int(slot["N_updates"][0]) == 4 and bool(slot["is_dirty"][0])
        return [recs, slot]

    try:
        _both(monkeypatch, run)
    finally:
        manager.shutdown()


@pytest.mark.parametrize("mode", ["rays", "calib"])
def test_publish_direct_mode_unchanged(golden, monkeypatch, mode):
    """opt_pose_* (no byte map, no count): the same poses from either publish path, within the golden contract."""
    from m3s.sim3 import Sim3
    from m3s.tracker import FrameTracker

    g = golden("optpose_32x48.npz")
    d = lambda k: torch.from_numpy(g[k]).cuda()

    def run():
        tr = FrameTracker(None, None, "cuda")
        if mode == "rays":
            Tf, Tr = tr.opt_pose_ray_dist_sim3(d("Xf"), d("Xk"), Sim3(d("T_WCf")), Sim3(d("T_WCk")), d("Qk"), d("valid"))
        else:
            Tf, Tr = tr.opt_pose_calib_sim3(d("Xf_c"), d("Xk"), Sim3(d("T_WCf")), Sim3(d("T_WCk")), d("Qk"),
                                            d("valid"), d("meas"), d("vmeas"), d("K"), (32, 48))
        r = tr.last_result
        return {"T_WCf": Tf.data.cpu().clone(), "T_CkCf": Tr.data.cpu().clone(), "iters": r.iters, "status": r.status,
                "cost": np.float64(r.cost).tobytes(), "n_unique": r.n_unique}

    old, new = _both(monkeypatch, run)
    np.testing.assert_allclose(new["T_WCf"].numpy(), g[f"{mode}_T_WCf"], atol=1e-5)
    np.testing.assert_allclose(new["T_CkCf"].numpy(), g[f"{mode}_T_CkCf"], atol=1e-5)


def test_publish_with_separate_setup(monkeypatch):
    """M3S_TRACK_FOLD_SETUP=0 with the new publish asked for: the separate-setup launch has no in-launch count, so the
    result comes from the fuse launch, equal to the old path with either setup."""

    def run():
        rig = Rig(48, 64, False, seeds=(0, 1))
        return [rig.step(), rig.step()]

    old_sep, new_sep = _both(monkeypatch, run, extra_env={"M3S_TRACK_FOLD_SETUP": "0"})
    monkeypatch.setenv("M3S_TRACK_FOLD_SETUP", "1")
    monkeypatch.setenv(ENV, "0")
    _same(run(), new_sep, "folded old path vs separate setup with the new publish")
