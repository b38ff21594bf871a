"""GPU parity: the projection search run inside the refine launch (default) equals the three-launch path.

m3s_match's tile path runs normalise X21 -> LM projection -> occlusion test -> coarse-to-fine refine in one launch
(refine.hip, the fused refine_tile_kernel instance); M3S_MATCH_FUSE_PROJ=0 restores proj_occlusion_kernel + the
unfused refine launch. Both run the same source for the projection (csrc/m3s_proj.hpp) under the same compiler
flags, so idx and valid must be equal bit for bit, and equal to the oracle where test_gpu_matching.py compares to it.
No tolerances anywhere.
"""
import numpy as np
import pytest
import torch

import oracle.oracle as O

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(args):
    from m3s.matching import match

    idx, valid = match(*args)
    torch.cuda.synchronize()
    return idx.cpu().numpy().copy(), valid.cpu().numpy().copy()


def _both(monkeypatch, X11, X21, D11, D21, idx_init=None):
    """(idx, valid) of the three-launch path and of the fused default on the same device tensors"""
    args = [_dev(X11), _dev(X21), _dev(D11), _dev(D21)]
    if idx_init is not None:
        args.append(_dev(idx_init))
    monkeypatch.setenv("M3S_MATCH_FUSE_PROJ", "0")
    unfused = _run(args)
    monkeypatch.delenv("M3S_MATCH_FUSE_PROJ")
    fused = _run(args)
    return unfused, fused


def _assert_same(unfused, fused, ref=None):
    np.testing.assert_array_equal(fused[0], unfused[0])
    np.testing.assert_array_equal(fused[1], unfused[1])
    if ref is not None:
        np.testing.assert_array_equal(fused[0], ref[0])
        np.testing.assert_array_equal(fused[1], ref[1])


def _pairs(B, H, W, seed):
    from m3s.synthetic import make_pair

    Ps = [make_pair(H, W, seed=seed + b) for b in range(B)]
    return tuple(np.stack([p[k][i].numpy() for p in Ps]) for k, i in (("X", 0), ("X", 1), ("D", 0), ("D", 1)))


def test_golden_cold_and_warm(monkeypatch, golden):
    g = golden("matching_48x64.npz")
    un, fu = _both(monkeypatch, g["X11"], g["X21"], g["D11"], g["D21"])
    _assert_same(un, fu, (g["idx"], g["valid"]))
    un, fu = _both(monkeypatch, g["X11"], g["X21"], g["D11"], g["D21"], g["idx_init"])
    _assert_same(un, fu, (g["idx_warm"], g["valid_warm"]))


@pytest.mark.parametrize("H,W", [(8, 32), (9, 33)])
def test_single_and_partial_tiles(monkeypatch, H, W):
    """8x32: one full tile. 9x33: four tiles, three of them one pixel wide or high."""
    X11, X21, D11, D21 = _pairs(1, H, W, seed=40)
    un, fu = _both(monkeypatch, X11, X21, D11, D21)
    _assert_same(un, fu, O.match(X11, X21, D11, D21))


@pytest.mark.parametrize("shape,dmax", [((2, 50, 70), 5), ((1, 40, 96), 3), ((1, 33, 47), 1)])
def test_ragged_and_batched(monkeypatch, shape, dmax):
    """Partial tiles, batch > 1, the double-buffered (d = 2) and packed (d = 1) window paths."""
    from m3s.config import config

    B, H, W = shape
    config["matching"]["dilation_max"] = dmax
    X11, X21, D11, D21 = _pairs(B, H, W, seed=30)
    un, fu = _both(monkeypatch, X11, X21, D11, D21)
    _assert_same(un, fu, O.match(X11, X21, D11, D21, dilation_max=dmax))


@pytest.fixture(scope="module")
def scattered():
    """96x128 pair with a random warm start and the oracle's result for it (computed once)"""
    H, W = 96, 128
    X11, X21, D11, D21 = _pairs(1, H, W, seed=21)
    init = np.random.default_rng(3).integers(0, H * W, size=(1, H * W)).astype(np.int64)
    return (X11, X21, D11, D21, init), O.match(X11, X21, D11, D21, idx_init=init)


def test_scattered_warm_start(monkeypatch, scattered):
    """Every lane a window outlier: the unfused and the fused tile instance each score all of them in place."""
    inputs, ref = scattered
    un, fu = _both(monkeypatch, *inputs)
    _assert_same(un, fu, ref)


def test_every_lane_an_outlier_at_the_coarsest_levels(monkeypatch):
    """dilation_max = 8: at d = 8 and d = 7 a grid spans 6 d + 1 = 49 and 43 rows and the window holds at most 40, so
    every active lane of every wave is a window outlier at the first two levels and is scored in place, in the unfused
    and the fused tile instance and in the reference operator's. 16x64 is the smallest image with full tiles in both
    directions. White unit descriptors: each coarse level moves most pixels (the oracle's dilation_max 8 and 7 results
    differ on 74 % of them; with the smooth synthetic descriptors they are identical), so a dropped or mis-ordered
    level shows."""
    import mast3r_slam_backends as B
    from m3s.config import config

    config["matching"]["dilation_max"] = 8
    H, W = 16, 64
    X11, X21, _, _ = _pairs(1, H, W, seed=60)
    rng = np.random.default_rng(8)
    D11, D21 = (rng.standard_normal((1, H, W, 24)) for _ in range(2))
    D11, D21 = ((d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32) for d in (D11, D21))
    ref = O.match(X11, X21, D11, D21, dilation_max=8)
    un, fu = _both(monkeypatch, X11, X21, D11, D21)
    _assert_same(un, fu, ref)
    # the reference operator from the oracle's own centres
    p1 = O.match_diag(X11, X21, D11, D21, dilation_max=8)["p1"]
    p1 = np.stack((p1 % W, p1 // W), -1).astype(np.int64)
    (op,) = B.refine_matches(_dev(D11).half(), _dev(D21.reshape(1, H * W, 24)).half(), _dev(p1), 3, 8)
    op = op.cpu().numpy()
    np.testing.assert_array_equal(op[..., 0] + W * op[..., 1], ref[0])


@pytest.mark.parametrize("max_iter", [0, 1])
def test_lm_iteration_edge_cases(monkeypatch, max_iter):
    """max_iter 0: the occlusion pixel is the clamped start; 1: the LAST-only iteration."""
    from m3s.config import config

    config["matching"]["max_iter"] = max_iter
    X11, X21, D11, D21 = _pairs(1, 50, 70, seed=33)
    init = np.random.default_rng(8).integers(0, 50 * 70, size=(1, 50 * 70)).astype(np.int64)
    _assert_same(*_both(monkeypatch, X11, X21, D11, D21))
    _assert_same(*_both(monkeypatch, X11, X21, D11, D21, init))


def test_screen_off(monkeypatch):
    X11, X21, D11, D21 = _pairs(1, 50, 70, seed=34)
    monkeypatch.setenv("M3S_REFINE_SCREEN", "0")
    un, fu = _both(monkeypatch, X11, X21, D11, D21)
    _assert_same(un, fu, O.match(X11, X21, D11, D21))
    monkeypatch.setenv("M3S_REFINE_SCREEN", "1")
    _assert_same(un, _both(monkeypatch, X11, X21, D11, D21)[1])


def test_nan_descriptor(monkeypatch):
    """One NaN pixel in D11: every block's own reduction of the norm partials must give NaN, which switches the
    screen off for every lane (as the projection launch's single reduction does). The exact scan
    (M3S_REFINE_SCREEN=0) is the reference."""
    X11, X21, D11, D21 = _pairs(1, 96, 128, seed=3)
    D11 = D11.copy()
    D11[0, 5, 7, 3] = np.nan
    un, fu = _both(monkeypatch, X11, X21, D11, D21)
    _assert_same(un, fu)
    monkeypatch.setenv("M3S_REFINE_SCREEN", "0")
    exact_un, exact_fu = _both(monkeypatch, X11, X21, D11, D21)
    _assert_same(exact_un, exact_fu)
    _assert_same(exact_un, fu)


def test_changing_shapes_on_one_workspace(monkeypatch):
    """48x64, 96x128, 48x64 in a row on the cached workspace: nothing stale between shapes."""
    small, large = _pairs(1, 48, 64, seed=50), _pairs(1, 96, 128, seed=51)
    monkeypatch.setenv("M3S_MATCH_FUSE_PROJ", "0")
    ref = [_run([_dev(a) for a in p]) for p in (small, large)]
    monkeypatch.delenv("M3S_MATCH_FUSE_PROJ")
    for p, r in ((small, ref[0]), (large, ref[1]), (small, ref[0])):
        _assert_same(r, _run([_dev(a) for a in p]))
