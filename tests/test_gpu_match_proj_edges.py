"""GPU: the front half of ``match`` (prep_rays_kernel, the LM projection search of csrc/m3s_proj.hpp, the occlusion
test, lin_to_pixel_f) and the per-pixel fallback kernels of csrc/matching.hip against the oracle, exactly.

The cases and the oracle's results for them are in tests/match_proj_cases.py; tests/test_match_proj_host.py proves on
the CPU that each case does what it is for. Every projection case carries D21 = 0, which makes the refine the
identity, so ``idx`` is the projection's truncated centre itself and a centre one pixel off fails the comparison
(with the scene's own descriptors the refine hides it: the host file measures both).

Each projection case runs through four device paths:
  fused     the default: prep_rays_kernel<1> + the refine tile launch with the projection in its prologue
  unfused   M3S_MATCH_FUSE_PROJ=0: prep_rays_kernel<1> + proj_occlusion_kernel + the refine tile launch
  radius0   config radius 0: prep_rays_kernel<0> + proj_occlusion_kernel + the pass-through refine_lin_kernel
  op        mast3r_slam_backends.iter_proj on the oracle's prep arrays: p_new as floats, before the truncation

Every comparison is ``assert_array_equal`` against the oracle: no tolerance, no pixel left out. The one exception is
the fp32 refine instance, which may differ from the oracle on at most 1e-3 of the pixels (its sum order), as in
test_gpu_matching.py::test_refine_matches_bit_exact_vs_oracle.

Mutation check (by hand on a copy, not committed; arithmetic-only changes, of 239 tests):
  * ``lin_to_pixel_f`` without the floor correction of negative indices: 6 red (warm/range and warm/huge on the three
    match paths; the op path takes p_init as floats);
  * eps 1e-11 in the fused prologue's X21 normalisation only: 1 red (degen/x21_tiny, fused);
  * ``d <= dist_thresh`` in proj_occlusion_kernel only: 2 red (occ/threshold, unfused and radius0);
  * ``refine_point`` starting at level min(dilation_max, 9): 2 red (dil/10 through the op and through match);
  * lambda x 9 for a rejected step: 128 red, among them every lm case at max_iter 3 and 10 and every warm case on all
    four paths; size/3x40, 17x65, 9x33, 16x16 and b2_12x20 only on the op path (the truncated centres hide it).
A build whose three normalisations propagate a NaN norm as torch's clamp_min does passes all 239: DESIGN.md section 2.
"""
import numpy as np
import pytest
import torch

import match_proj_cases as E

pytestmark = pytest.mark.gpu

PATHS = ("fused", "unfused", "radius0", "op")


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))  # a copy: the cases are read-only
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _match(cs, monkeypatch, path):
    from m3s.config import config
    from m3s.matching import match

    config["matching"].update(cs.params)
    if path == "radius0":
        config["matching"]["radius"] = 0
    if path == "unfused":
        monkeypatch.setenv("M3S_MATCH_FUSE_PROJ", "0")
    else:
        monkeypatch.delenv("M3S_MATCH_FUSE_PROJ", raising=False)
    args = [_dev(cs.X11), _dev(cs.X21), _dev(cs.D11), _dev(cs.D21)]
    if cs.idx_init is not None:
        args.append(_dev(cs.idx_init))
    idx, valid = match(*args)
    assert idx.dtype == torch.int64 and valid.dtype == torch.bool
    return idx.cpu().numpy(), valid.cpu().numpy()


def _report(what, got, ref):
    bad = np.argwhere(got != ref)
    return (f"{what}: {len(bad)} of {got.size} differ; first {bad[:5].tolist()}, got "
            f"{[got[tuple(b)] for b in bad[:5]]}, expected {[ref[tuple(b)] for b in bad[:5]]}")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", E.PROJ_NAMES)
def test_projection_case_equals_oracle(monkeypatch, name, path):
    cs = E.case(name)
    if path == "op":
        import mast3r_slam_backends as B

        k = E.match_kwargs(cs)
        rays, pts, p_init, ref_p, ref_c = E.expected_iter_proj(name)
        p_new, conv = B.iter_proj(_dev(rays), _dev(pts), _dev(p_init), k["max_iter"], k["lambda_init"],
                                  k["convergence_thresh"])
        assert p_new.dtype == torch.float32 and conv.dtype == torch.bool
        got_p, got_c = p_new.cpu().numpy(), conv.cpu().numpy()
        assert np.array_equal(got_p, ref_p), _report(f"{name} p_new", got_p, ref_p)
        assert np.array_equal(got_c, ref_c), _report(f"{name} converged", got_c, ref_c)
        return
    ref_idx, ref_valid = E.expected_match(name, 0 if path == "radius0" else 3)
    idx, valid = _match(cs, monkeypatch, path)
    assert np.array_equal(idx, ref_idx), _report(f"{name} {path} idx", idx, ref_idx)
    assert np.array_equal(valid, ref_valid), _report(f"{name} {path} valid", valid, ref_valid)


@pytest.mark.parametrize("shape", [(2, 8), (8, 2)])
def test_images_under_3x3_are_rejected(shape):
    import mast3r_slam_backends as B
    from m3s.matching import match

    H, W = shape
    X = torch.ones((1, H, W, 3), device="cuda")
    D = torch.ones((1, H, W, 24), device="cuda")
    with pytest.raises(RuntimeError, match="at least 3x3"):
        match(X, X, D, D)
    rays = torch.ones((1, H, W, 9), device="cuda")
    pts = torch.ones((1, H * W, 3), device="cuda")
    with pytest.raises(RuntimeError, match="at least 3x3"):
        B.iter_proj(rays, pts, torch.ones((1, H * W, 2), device="cuda"), 10, 1e-8, 1e-6)


# ------------------------------------------------------------------------------------------------
# fallback kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.FALLBACK_NAMES)
def test_fallback_op_equals_oracle(name):
    """mast3r_slam_backends.refine_matches: refine_f16_kernel<16 / 24 / 32> at F != 24, dilation_max > 8, radius != 3
    or N != H W; the LDS tile kernel at N = H W with centres outside the image; refine_f32_kernel at F = 5"""
    import mast3r_slam_backends as B

    fb = E.fallback(name)
    ref = E.expected_refine(name)
    dt = torch.float16 if fb.half else torch.float32
    (out,) = B.refine_matches(_dev(fb.D11, dt), _dev(fb.D21, dt), _dev(fb.p1), fb.radius, fb.dilation_max)
    assert out.dtype == torch.int64
    got = out.cpu().numpy()
    if fb.half:
        assert np.array_equal(got, ref), _report(name, got, ref)
    else:
        share = float((got != ref).any(-1).mean())
        print(f"{name}: fp32 refine differs from the oracle on {share:.2e} of the pixels")
        assert share <= 1e-3  # fp32 sum order may differ (FMA)


@pytest.mark.parametrize("name", E.FALLBACK_MATCH_NAMES)
def test_fallback_match_equals_oracle(name):
    """match at F = 16 / 32, dilation_max 9 / 10, radius 1 / 2 / 4: prep_rays_kernel<2> (row-layout descriptors),
    proj_occlusion_kernel, refine_lin_kernel<F>"""
    from m3s.config import config
    from m3s.matching import match

    fb = E.fallback(name)
    H, W = fb.X11.shape[1:3]
    config["matching"]["radius"] = fb.radius
    config["matching"]["dilation_max"] = fb.dilation_max
    ref_idx, ref_valid = E.expected_fallback_match(name)
    idx, valid = match(_dev(fb.X11), _dev(fb.X21), _dev(fb.D11), _dev(fb.D21.reshape(1, H, W, -1)))
    idx, valid = idx.cpu().numpy(), valid.cpu().numpy()
    assert np.array_equal(idx, ref_idx), _report(f"{name} idx", idx, ref_idx)
    assert np.array_equal(valid, ref_valid), _report(f"{name} valid", valid, ref_valid)


def test_half_op_rejects_other_widths():
    import mast3r_slam_backends as B

    D11 = torch.zeros((1, 8, 8, 20), dtype=torch.float16, device="cuda")
    D21 = torch.zeros((1, 64, 20), dtype=torch.float16, device="cuda")
    p1 = torch.zeros((1, 64, 2), dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="F in"):
        B.refine_matches(D11, D21, p1, 3, 5)
