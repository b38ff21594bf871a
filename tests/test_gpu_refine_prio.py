"""GPU parity of the refine tile kernel's per-level shortcuts (csrc/refine.hip): the screen's accumulators seeded
from chunk 0's first product instead of zeroed, the wave-uniform skip of the mask and the survivor code when no lane
can hold a survivor, and the wave issue priorities (which change no value).

Every case compares the fused match's idx / valid with the CPU oracle's and with the same call's exact scan
(M3S_REFINE_SCREEN=0). No tolerances anywhere. Two constructed 16x64 inputs aim at the skip:
  * peaked: every D21 row is the D11 row of a pixel on the first level's candidate grid and the D11 rows are random
    unit vectors, so after the first level no candidate comes within the screen's bound of the running max and every
    wave takes the skip at d = 4 .. 1;
  * constant: one descriptor everywhere, so every in-image candidate ties and survives at every level, no wave may
    take the skip, and the strict-'>' scan must keep the first candidate in scan order.
Both claims are checked on the host first, with the kernel's bound B = 0.0125 |q| cmax 1.001 + 2^-18 in numpy.
"""
import numpy as np
import pytest
import torch

import oracle.oracle as O

pytestmark = pytest.mark.gpu

R, G = 3, 7


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(args):
    from m3s.matching import match

    idx, valid = match(*args)
    torch.cuda.synchronize()
    return idx.cpu().numpy().copy(), valid.cpu().numpy().copy()


def _check(monkeypatch, ref, X11, X21, D11, D21, idx_init=None):
    """the fused default and the exact scan on the same device tensors, both against ref = (idx, valid)"""
    args = [_dev(X11), _dev(X21), _dev(D11), _dev(D21)]
    if idx_init is not None:
        args.append(_dev(idx_init))
    monkeypatch.delenv("M3S_REFINE_SCREEN", raising=False)
    got = _run(args)
    monkeypatch.setenv("M3S_REFINE_SCREEN", "0")
    exact = _run(args)
    monkeypatch.delenv("M3S_REFINE_SCREEN")
    for k in (0, 1):
        np.testing.assert_array_equal(got[k], ref[k])
        np.testing.assert_array_equal(exact[k], ref[k])


def _pairs(B, H, W, seed):
    from m3s.synthetic import make_pair

    Ps = [make_pair(H, W, seed=seed + b) for b in range(B)]
    return tuple(np.stack([p[k][i].numpy() for p in Ps]) for k, i in (("X", 0), ("X", 1), ("D", 0), ("D", 1)))


def test_golden_cold_and_warm(monkeypatch, golden):
    g = golden("matching_48x64.npz")
    _check(monkeypatch, (g["idx"], g["valid"]), g["X11"], g["X21"], g["D11"], g["D21"])
    _check(monkeypatch, (g["idx_warm"], g["valid_warm"]), g["X11"], g["X21"], g["D11"], g["D21"], g["idx_init"])


@pytest.mark.parametrize("H,W", [(8, 32), (9, 33)])
def test_single_and_partial_tiles(monkeypatch, H, W):
    X11, X21, D11, D21 = _pairs(1, H, W, seed=60)
    _check(monkeypatch, O.match(X11, X21, D11, D21), X11, X21, D11, D21)


@pytest.mark.parametrize("shape,dmax", [((2, 50, 70), 5), ((1, 33, 47), 1)])
def test_ragged_and_batched(monkeypatch, shape, dmax):
    from m3s.config import config

    B, H, W = shape
    config["matching"]["dilation_max"] = dmax
    X11, X21, D11, D21 = _pairs(B, H, W, seed=62)
    _check(monkeypatch, O.match(X11, X21, D11, D21, dilation_max=dmax), X11, X21, D11, D21)


# ---- the constructed inputs ----
def _half(x):
    return x.astype(np.float16).astype(np.float64)


def _level_scores(D11, q, cu, cv, d):
    """fp64 scores of the half-rounded operands for the 49 candidates of level d around (cu, cv) (N,), scan order
    (u outer, v inner): (N, 49) scores and the in-image mask"""
    H, W, _ = D11.shape
    i, j = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
    u = cu[:, None] + (i.reshape(-1)[None] - R) * d
    v = cv[:, None] + (j.reshape(-1)[None] - R) * d
    ok = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    c = _half(D11)[np.clip(v, 0, H - 1), np.clip(u, 0, W - 1)]
    return np.einsum("nk,nck->nc", _half(q), c), ok


def _bound(D11, q):
    cmax = np.sqrt((_half(D11) ** 2).sum(-1)).max()
    return 0.0125 * np.sqrt((_half(q) ** 2).sum(-1)) * cmax * 1.001 + 2.0 ** -18


H16, W64 = 16, 64


@pytest.fixture(scope="module")
def geometry():
    """the 16x64 pair's points and the projection search's centres (the oracle's, computed once)"""
    X11, X21, D11, D21 = _pairs(1, H16, W64, seed=64)
    p1 = O.match_diag(X11, X21, D11, D21)["p1"][0]
    return X11, X21, p1 % W64, p1 // W64


def test_peaked_descriptors_every_wave_skips(monkeypatch, geometry):
    X11, X21, cu, cv = geometry
    rng = np.random.default_rng(5)
    D11 = rng.standard_normal((H16, W64, 24))
    D11 = (D11 / np.linalg.norm(D11, axis=-1, keepdims=True)).astype(np.float32)
    # the true match: candidate (4, 2) of the first level's grid (d = 5) where that lies inside the image, else the
    # centre itself (candidate (3, 3))
    tu, tv = cu + 5, cv - 5
    out = (tu < 0) | (tu >= W64) | (tv < 0) | (tv >= H16)
    tu, tv = np.where(out, cu, tu), np.where(out, cv, tv)
    D21 = D11[tv, tu]
    # host check of the construction, with margins that cover every rounding of either scoring (2B + 1e-3):
    B = _bound(D11, D21)
    s5, ok5 = _level_scores(D11, D21, cu, cv, 5)
    self_score = np.einsum("nk,nk->n", _half(D21), _half(D21))
    s5 = np.where(ok5, s5, -np.inf)
    assert (np.sort(s5, axis=1)[:, -2] < self_score - 2 * B - 1e-3).all()  # first level: the true match alone wins
    assert (np.abs(s5.max(axis=1) - self_score) < 1e-9).all() and (self_score > 2 * B + 1e-3).all()
    survivors = 0
    for d in (4, 3, 2, 1):  # later levels: centred on the true match, no other candidate within the bound of its score
        s, ok = _level_scores(D11, D21, tu, tv, d)
        ok[:, G * G // 2] = False
        survivors += int((ok & (s >= (self_score - 2 * B - 1e-3)[:, None])).sum())
    assert survivors == 0
    ref = O.match(X11, X21, D11[None], D21.reshape(1, H16, W64, 24))
    np.testing.assert_array_equal(ref[0][0], tu + W64 * tv)
    _check(monkeypatch, ref, X11, X21, D11[None], D21.reshape(1, H16, W64, 24))


def test_constant_descriptors_every_candidate_survives(monkeypatch, geometry):
    X11, X21, cu, cv = geometry
    c = np.random.default_rng(6).standard_normal(24)
    c = (c / np.linalg.norm(c)).astype(np.float32)
    D11 = np.broadcast_to(c, (1, H16, W64, 24)).copy()
    D21 = D11.copy()
    # host check: every in-image candidate ties the level's best (a[c] = lmax >= T for any B >= 0), and the tie is
    # positive, so the first level's first in-image candidate in scan order wins and nothing beats it afterwards
    s, ok = _level_scores(D11[0], D21[0].reshape(-1, 24), cu, cv, 5)
    assert (s == s[0, 0]).all() and s[0, 0] > 0.5
    first = np.argmax(ok, axis=1)  # u outer, v inner
    eu, ev = cu + (first // G - R) * 5, cv + (first % G - R) * 5
    ref = O.match(X11, X21, D11, D21)
    np.testing.assert_array_equal(ref[0][0], eu + W64 * ev)
    _check(monkeypatch, ref, X11, X21, D11, D21)
