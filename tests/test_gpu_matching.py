"""GPU parity: matching kernels (iter_proj, refine_matches, fused match) vs the oracle / golden vectors.

Tolerances: none. The oracle's prep (m3o_normalize3 / m3o_img_gradient) is bit-exact against the reference run's
torch glue (golden rays / pts), the HIP prep follows the same fp32 FMA order, and the LM iteration, the occlusion
distance and the c10::Half refine are restated operation for operation: p_new, converged, idx and valid are
asserted equal, bit for bit (round 6; earlier rounds allowed <= 1e-4 of pixels to flip, which the fp64 oracle prep
caused: scripts/match_mismatch.py, profiles/r06_match_census.txt).
"""
import numpy as np
import pytest
import torch

import oracle.oracle as O

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def test_iter_proj_matches_golden(golden):
    import mast3r_slam_backends as B

    g = golden("matching_48x64.npz")
    p_new, conv = B.iter_proj(_dev(g["rays"]), _dev(g["pts"]), _dev(g["p_init"]), 10, 1e-8, 1e-6)
    p = p_new.cpu().numpy()
    c = conv.cpu().numpy()
    assert conv.dtype == torch.bool and p_new.dtype == torch.float32
    np.testing.assert_array_equal(p, g["p_new"])
    np.testing.assert_array_equal(c, g["converged"])


def test_iter_proj_ragged_n():
    """N not a multiple of 16/256 (the reference kernel would read out of bounds)."""
    import mast3r_slam_backends as B

    P = __import__("m3s.synthetic", fromlist=["make_pair"]).make_pair(20, 28, seed=4)
    X = P["X"].numpy()
    rays, pts, p_init = O.prep_for_iter_proj(X[:1], X[1:], None)
    n = 333
    pts, p_init = pts[:, :n], p_init[:, :n]
    ref_p, ref_c = O.iter_proj(rays, pts, p_init, 10, 1e-8, 1e-6)
    p_new, conv = B.iter_proj(_dev(rays), _dev(pts), _dev(p_init), 10, 1e-8, 1e-6)
    np.testing.assert_array_equal(p_new.cpu().numpy(), ref_p)
    np.testing.assert_array_equal(conv.cpu().numpy(), ref_c)


@pytest.mark.parametrize("half", [True, False])
def test_refine_matches_bit_exact_vs_oracle(golden, half):
    import mast3r_slam_backends as B

    g = golden("matching_48x64.npz")
    p1 = g["p_new"].astype(np.int64)
    D21 = g["D21"].reshape(1, -1, 24)
    if half:
        ref = O.refine_matches(g["D11h"], O.to_half_bits(D21), p1, 3, 5)
        out = B.refine_matches(_dev(g["D11"], torch.float16), _dev(D21, torch.float16), _dev(p1), 3, 5)[0]
    else:
        ref = O.refine_matches(g["D11"], D21, p1, 3, 5, half=False)
        out = B.refine_matches(_dev(g["D11"]), _dev(D21), _dev(p1), 3, 5)[0]
    assert out.dtype == torch.int64
    got = out.cpu().numpy()
    if half:
        np.testing.assert_array_equal(got, ref)  # c10::Half step rounding reproduced exactly
    else:
        assert (got != ref).any(-1).mean() <= 1e-3  # fp32 sum order may differ (FMA)


def test_refine_border_and_radius_zero():
    import mast3r_slam_backends as B

    rng = np.random.default_rng(1)
    H, W, F = 16, 24, 24
    D11 = rng.standard_normal((2, H, W, F)).astype(np.float32)
    D21 = rng.standard_normal((2, H * W, F)).astype(np.float32)
    p1 = np.stack(np.meshgrid(np.arange(W), np.arange(H), indexing="xy"), -1).reshape(1, -1, 2).repeat(2, 0)
    p1 = p1.astype(np.int64)
    for radius, dil in ((3, 5), (1, 1), (0, 5), (2, 0)):
        ref = O.refine_matches(D11, D21, p1, radius, dil)
        out = B.refine_matches(_dev(D11, torch.float16), _dev(D21, torch.float16), _dev(p1), radius, dil)[0]
        np.testing.assert_array_equal(out.cpu().numpy(), ref)


def test_contiguity_error_like_reference(golden):
    import mast3r_slam_backends as B

    g = golden("matching_48x64.npz")
    rays = _dev(g["rays"]).transpose(1, 2)
    with pytest.raises(RuntimeError, match="must be contiguous"):
        B.iter_proj(rays, _dev(g["pts"]), _dev(g["p_init"]), 10, 1e-8, 1e-6)


def test_fused_match_matches_golden(golden):
    from m3s.matching import match

    g = golden("matching_48x64.npz")
    idx, valid = match(_dev(g["X11"]), _dev(g["X21"]), _dev(g["D11"]), _dev(g["D21"]))
    assert idx.shape == (1, 48 * 64) and valid.shape == (1, 48 * 64, 1)
    np.testing.assert_array_equal(idx.cpu().numpy(), g["idx"])
    np.testing.assert_array_equal(valid.cpu().numpy(), g["valid"])
    idx_w, valid_w = match(_dev(g["X11"]), _dev(g["X21"]), _dev(g["D11"]), _dev(g["D21"]), _dev(g["idx_init"]))
    np.testing.assert_array_equal(idx_w.cpu().numpy(), g["idx_warm"])
    np.testing.assert_array_equal(valid_w.cpu().numpy(), g["valid_warm"])


@pytest.mark.parametrize("shape", [(96, 128, 2), (128, 160, 1)])
def test_fused_match_vs_oracle_batched(shape):
    from m3s.matching import match
    from m3s.synthetic import make_pair

    H, W, B = shape
    Ps = [make_pair(H, W, seed=10 + b) for b in range(B)]
    X11 = np.stack([p["X"][0].numpy() for p in Ps])
    X21 = np.stack([p["X"][1].numpy() for p in Ps])
    D11 = np.stack([p["D"][0].numpy() for p in Ps])
    D21 = np.stack([p["D"][1].numpy() for p in Ps])
    ref_idx, ref_valid = O.match(X11, X21, D11, D21)
    idx, valid = match(_dev(X11), _dev(X21), _dev(D11), _dev(D21))
    np.testing.assert_array_equal(idx.cpu().numpy(), ref_idx)
    np.testing.assert_array_equal(valid.cpu().numpy(), ref_valid)


@pytest.mark.parametrize("shape,dmax", [((2, 50, 70), 5), ((1, 40, 96), 3), ((1, 64, 64), 8), ((1, 33, 47), 1)])
def test_fused_match_ragged_and_dilations_vs_oracle(shape, dmax):
    """Partial refine tiles (H % 8, W % 32 != 0), batch > 1 and every dilation specialisation."""
    from m3s.config import config
    from m3s.matching import match
    from m3s.synthetic import make_pair

    B, H, W = shape
    config["matching"]["dilation_max"] = dmax
    Ps = [make_pair(H, W, seed=30 + b) for b in range(B)]
    X11 = np.stack([p["X"][0].numpy() for p in Ps])
    X21 = np.stack([p["X"][1].numpy() for p in Ps])
    D11 = np.stack([p["D"][0].numpy() for p in Ps])
    D21 = np.stack([p["D"][1].numpy() for p in Ps])
    ref_idx, ref_valid = O.match(X11, X21, D11, D21, dilation_max=dmax)
    idx, valid = match(_dev(X11), _dev(X21), _dev(D11), _dev(D21))
    np.testing.assert_array_equal(idx.cpu().numpy(), ref_idx)
    np.testing.assert_array_equal(valid.cpu().numpy(), ref_valid)


def test_fused_match_scattered_warm_start_vs_oracle():
    """A random warm start scatters the LM results, so many refine centres fall outside their tile's
    LDS window: exercises the in-place outlier scoring (refine.hip level_outliers, one wave-level per outlier) against
    the oracle's sequential scan, in the fused match and through the reference op."""
    from m3s.matching import match
    from m3s.synthetic import make_pair

    H, W = 96, 128
    P = make_pair(H, W, seed=21)
    X11, X21 = P["X"][:1].numpy(), P["X"][1:].numpy()
    D11, D21 = P["D"][:1].numpy(), P["D"][1:].numpy()
    init = np.random.default_rng(3).integers(0, H * W, size=(1, H * W)).astype(np.int64)
    ref_idx, ref_valid = O.match(X11, X21, D11, D21, idx_init=init)
    idx, valid = match(_dev(X11), _dev(X21), _dev(D11), _dev(D21), _dev(init))
    np.testing.assert_array_equal(idx.cpu().numpy(), ref_idx)
    np.testing.assert_array_equal(valid.cpu().numpy(), ref_valid)
    # reference op on the same scattered centres: bit-exact c10::Half refine
    rays, pts, p_init = O.prep_for_iter_proj(X11, X21, init)
    p_new, _ = O.iter_proj(rays, pts, p_init, 10, 1e-8, 1e-6)
    p1 = p_new.astype(np.int64)
    ref = O.refine_matches(D11, D21.reshape(1, H * W, -1), p1, 3, 5)
    import mast3r_slam_backends as B

    (got,) = B.refine_matches(_dev(D11).half(), _dev(D21.reshape(1, H * W, -1)).half(), _dev(p1), 3, 5)
    np.testing.assert_array_equal(got.cpu().numpy(), ref)


def test_fused_match_full_size_properties():
    """512x512 (BASELINE configs[0] shape): properties that do not need the oracle at full size."""
    from m3s.matching import match
    from m3s.synthetic import make_pair

    P = make_pair(512, 512, seed=0)
    X, D = P["X"].cuda(), P["D"].cuda()
    idx, valid = match(X[:1], X[1:], D[:1], D[1:])
    i = idx.cpu().numpy()[0]
    v = valid.cpu().numpy()[0, :, 0]
    assert i.min() >= 0 and i.max() < 512 * 512
    assert v.mean() > 0.8  # most synthetic pixels have a true match inside the image
    # the matched pixel is within ~2 px of the analytic ground-truth flow
    u1, v1 = P["flow"]
    gt = np.stack((u1.numpy().reshape(-1), v1.numpy().reshape(-1)), -1)
    got = np.stack((i % 512, i // 512), -1)
    inside = v & (gt[:, 0] > 2) & (gt[:, 0] < 509) & (gt[:, 1] > 2) & (gt[:, 1] < 509)
    err = np.abs(got[inside] - gt[inside]).max(-1)
    assert np.median(err) <= 1.0 and (err > 3).mean() < 0.01
    # deterministic: second call identical
    idx2, valid2 = match(X[:1], X[1:], D[:1], D[1:])
    assert torch.equal(idx, idx2) and torch.equal(valid, valid2)
