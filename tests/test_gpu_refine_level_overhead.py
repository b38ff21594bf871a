"""GPU parity of the refine tile kernel's level-start exchanges (csrc/refine.hip level_window and tile_flow): the
bbox of the inlier centres as minima of packed signed 16-bit pairs and the tile's displacement sums, both reduced over
the wave by DPP and permlane swaps (m3s_common.hpp wave_reduce2) instead of LDS permutes.

Every case compares idx and valid, bit for bit, with the CPU oracle (oracle.oracle.match) for the fused default, for
the exact scan (M3S_REFINE_SCREEN=0) and for the separate projection launch with the unfused tile instance
(M3S_MATCH_FUSE_PROJ=0), and runs the same centres through the reference operator (refine_matches, the int64 p1
instance of the same level code). No tolerances anywhere.

The geometry of the constructed cases is a plane seen by a pinhole camera, and the frame's points are the keyframe's
own points gathered at chosen target pixels, with the warm start on the target: the projection search stays there, so
the centres the levels start from are the targets (checked on the host first, under the oracle alone):
  * last columns of 8x32767 / last rows of 32767x3: the 16-bit fields at their limit (max + 3 d passes 32767);
  * scattered targets on 40x70: covers that do not fit the 40x64 window, and tiles whose lanes split to the two image
    borders so that no lane is an inlier of the tile's mean displacement (the "no inlier" branch with active lanes);
  * a uniform shift: every cover fits the packed d = 1 and the double-buffered d = 2 windows.
9x33 has three almost empty tiles, with waves that have no active lane (the sentinels alone).
"""
import numpy as np
import pytest
import torch

import oracle.oracle as O
import test_gpu_refine_prio as prio

pytestmark = pytest.mark.gpu

TW, TH = 32, 8  # the kernel's tile (refine.hip RT_TW, RT_TH)
F = 24


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(args):
    from m3s.matching import match

    idx, valid = match(*args)
    torch.cuda.synchronize()
    return idx.cpu().numpy().copy(), valid.cpu().numpy().copy()


def _check(monkeypatch, ref, X11, X21, D11, D21, idx_init=None, p1=None):
    """ref = the oracle's (idx, valid). The fused default, the exact scan and the unfused launches on the same device
    tensors; then the reference operator from the centres p1 (linear (B,N); default: the oracle's own)"""
    import mast3r_slam_backends as B
    from m3s.config import config

    dmax = int(config["matching"]["dilation_max"])
    args = [_dev(X11), _dev(X21), _dev(D11), _dev(D21)]
    if idx_init is not None:
        args.append(_dev(idx_init))
    for var in (None, "M3S_REFINE_SCREEN", "M3S_MATCH_FUSE_PROJ"):
        if var is not None:
            monkeypatch.setenv(var, "0")
        got = _run(args)
        if var is not None:
            monkeypatch.delenv(var)
        np.testing.assert_array_equal(got[0], ref[0], err_msg=f"idx, {var}=0")
        np.testing.assert_array_equal(got[1], ref[1], err_msg=f"valid, {var}=0")
    b, H, W, _ = D11.shape
    if p1 is None:
        p1 = O.match_diag(X11, X21, D11, D21, idx_init, dilation_max=dmax)["p1"]
    p1 = np.stack((p1 % W, p1 // W), -1).astype(np.int64)
    (op,) = B.refine_matches(_dev(D11).half(), _dev(D21.reshape(b, H * W, F)).half(), _dev(p1), 3, dmax)
    op = op.cpu().numpy()
    np.testing.assert_array_equal(op[..., 0] + W * op[..., 1], ref[0], err_msg="refine_matches")


def _oracle(X11, X21, D11, D21, idx_init=None):
    from m3s.config import config

    d = O.match_diag(X11, X21, D11, D21, idx_init, dilation_max=int(config["matching"]["dilation_max"]))
    return (d["idx"], d["valid"]), d["p1"]


# ---- synthetic pairs: one tile, the smallest image, partial tiles, every dilation_max ----
@pytest.mark.parametrize("H,W", [(8, 32), (3, 3), (9, 33)])
def test_tiles(monkeypatch, H, W):
    X11, X21, D11, D21 = prio._pairs(1, H, W, seed=70)
    ref, p1 = _oracle(X11, X21, D11, D21)
    _check(monkeypatch, ref, X11, X21, D11, D21, p1=p1)


@pytest.mark.parametrize("dmax", [1, 2, 3, 4, 5, 6, 7, 8])
def test_each_dilation_max(monkeypatch, dmax):
    from m3s.config import config

    config["matching"]["dilation_max"] = dmax
    X11, X21, D11, D21 = prio._pairs(1, 20, 45, seed=71)
    ref, p1 = _oracle(X11, X21, D11, D21)
    _check(monkeypatch, ref, X11, X21, D11, D21, p1=p1)


# ---- the constructed geometry ----
def _plane(H, W):
    """points of a fronto-parallel plane with a gentle depth ramp (H,W,3): distinct, smoothly varying rays"""
    f = 0.9 * max(H, W)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    z = 2.0 + 0.1 * u / W + 0.05 * v / H
    return np.stack(((u - W / 2) / f * z, (v - H / 2) / f * z, z), -1).astype(np.float32)


def _descriptors(H, W, tu, tv, seed):
    """white unit descriptors for the keyframe; the frame's are its target's, with noise"""
    rng = np.random.default_rng(seed)
    D11 = rng.standard_normal((H, W, F), dtype=np.float32)
    D11 /= np.linalg.norm(D11, axis=-1, keepdims=True)
    D21 = D11[tv, tu] + 0.05 * rng.standard_normal((H, W, F), dtype=np.float32)
    return D11[None], D21[None]


def _targeted(H, W, tu, tv, seed):
    """the pair whose pixel (v, u) matches keyframe pixel (tv, tu)[v, u], warm-started there; the oracle's result
    and a host check that the levels start from the targets"""
    X11 = _plane(H, W)
    X21 = X11[tv, tu]
    D11, D21 = _descriptors(H, W, tu, tv, seed)
    idx_init = (tu + W * tv).reshape(1, -1).astype(np.int64)
    ref, p1 = _oracle(X11[None], X21[None], D11, D21, idx_init)
    cu, cv = (p1[0] % W).reshape(H, W), (p1[0] // W).reshape(H, W)
    assert (np.abs(cu - tu) <= 1).all() and (np.abs(cv - tv) <= 1).all()  # the search stayed on the targets
    return (X11[None], X21[None], D11, D21, idx_init), ref, p1, cu, cv


def _tile_bounds(cu, cv):
    """per tile: min / max of the centres (u and v)"""
    H, W = cu.shape
    out = []
    for y in range(0, H, TH):
        for x in range(0, W, TW):
            a, b = cu[y:y + TH, x:x + TW], cv[y:y + TH, x:x + TW]
            out.append((a.min(), a.max(), b.min(), b.max()))
    return np.array(out)


def test_last_columns_16bit_limit(monkeypatch):
    from m3s.config import config

    config["matching"]["dilation_max"] = 8
    H, W = 8, 32767
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    tu = np.minimum(W - TW + u % TW, W - 1)
    args, ref, p1, cu, cv = _targeted(H, W, tu, v, seed=72)
    tb = _tile_bounds(cu, cv)
    assert (tb[:, 1] + 3 * 8 > 32767).all() and (tb[:, 1] < W).all()  # max + 3 d does not fit 16 bits, in every tile
    _check(monkeypatch, ref, *args, p1=p1)


def test_last_rows_16bit_limit(monkeypatch):
    from m3s.config import config

    config["matching"]["dilation_max"] = 8
    H, W = 32767, 3
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    tv = np.minimum(H - TH + v % TH, H - 1)
    args, ref, p1, cu, cv = _targeted(H, W, u, tv, seed=73)
    tb = _tile_bounds(cu, cv)
    assert (tb[:, 3] + 3 * 8 > 32767).all() and (tb[:, 3] < H).all()
    _check(monkeypatch, ref, *args, p1=p1)


def test_scattered_warm_start(monkeypatch):
    H, W = 40, 70
    rng = np.random.default_rng(74)
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    tu, tv = rng.integers(0, W, (H, W)), rng.integers(0, H, (H, W))
    # the first row of tiles: a tile's left half goes to the right border, its right half to the left one
    tu[:TH] = np.where(u[:TH] % TW < TW // 2, W - 6 + u[:TH] % 6, u[:TH] % 6)
    tv[:TH] = v[:TH]
    args, ref, p1, cu, cv = _targeted(H, W, tu, tv, seed=75)
    # host check, the kernel's integer arithmetic: the tile's flow is the truncated mean displacement, an inlier lies
    # within 16 px of pixel + flow. No lane of the two full split tiles is one; the random tiles' covers do not fit
    # 64 columns
    for x in (0, TW):
        du, dv = (cu - u)[:TH, x:x + TW], (cv - v)[:TH, x:x + TW]
        fu, fv = int(du.sum() / du.size), int(dv.sum() / dv.size)  # C division truncates toward zero
        assert not ((np.abs(du - fu) <= 16) & (np.abs(dv - fv) <= 16)).any()
    tb = _tile_bounds(cu[TH:], cv[TH:])
    assert (tb[:, 1] - tb[:, 0] + 1 + 6 > 64).all()  # even at d = 1
    _check(monkeypatch, ref, *args, p1=p1)


def test_coherent_warm_start(monkeypatch):
    H, W = 24, 70
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    tu, tv = np.clip(u + 5, 0, W - 1), np.clip(v - 3, 0, H - 1)
    args, ref, p1, cu, cv = _targeted(H, W, tu, tv, seed=76)
    # host check: the start covers fit the packed window (48 x 17 at d = 1) with the room the levels' moves can take
    # (3 d per level; the refine's result stays within 2 px of the target's neighbourhood on these descriptors)
    tb = _tile_bounds(cu, cv)
    assert (tb[:, 1] - tb[:, 0] + 1 <= TW + 2).all() and (tb[:, 3] - tb[:, 2] + 1 <= TH + 2).all()
    _check(monkeypatch, ref, *args, p1=p1)


# ---- descriptors: ties everywhere, no survivor after the first level, a query without a usable bound ----
@pytest.fixture(scope="module")
def geometry():
    X11, X21, D11, D21 = prio._pairs(1, prio.H16, prio.W64, seed=64)
    p1 = O.match_diag(X11, X21, D11, D21)["p1"][0]
    return X11, X21, p1 % prio.W64, p1 // prio.W64


def test_every_wave_skips_after_the_first_level(monkeypatch, geometry):
    """test_gpu_refine_prio's peaked construction (with its host checks), through this file's wider comparison"""
    monkeypatch.setattr(prio, "_check", _check)
    prio.test_peaked_descriptors_every_wave_skips(monkeypatch, geometry)


def test_constant_descriptors_every_mask_bit_live(monkeypatch, geometry):
    """... and its constant construction: every candidate ties, so every column and every mask bit is live"""
    monkeypatch.setattr(prio, "_check", _check)
    prio.test_constant_descriptors_every_candidate_survives(monkeypatch, geometry)


def test_non_finite_descriptor(monkeypatch):
    H, W = 16, 40
    X11, X21, D11, D21 = prio._pairs(1, H, W, seed=77)
    D21 = D21.copy()
    D21[0, 5, 7, 3] = np.inf      # a non-finite query: no usable bound, every candidate survives (all scores inf / NaN)
    D21[0, 9, 33] *= 30000.0      # a finite one past the overflow guard: the exact chain decides among all 49
    # host check: |q| cmax of the two queries is outside the screen's range (refine.hip screen_bound: <= 16384)
    with np.errstate(over="ignore", invalid="ignore"):
        pq = (prio._bound(D11[0], D21[0].reshape(-1, F)) - 2.0 ** -18) / 0.0125
    assert not np.isfinite(pq[5 * W + 7]) and pq[9 * W + 33] > 16384 and (np.delete(pq, [5 * W + 7, 9 * W + 33]) < 2).all()
    ref, p1 = _oracle(X11, X21, D11, D21)
    _check(monkeypatch, ref, X11, X21, D11, D21, p1=p1)
