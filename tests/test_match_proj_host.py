"""The match front-half edge cases themselves, on the CPU alone (no device): the conditions that keep
tests/test_gpu_match_proj_edges.py from passing vacuously. With the oracle only, for the cases of
tests/match_proj_cases.py:

* the method: with D21 = 0 the refine is the identity, so a one-pixel error of the projection's centre on 1 % of the
  points changes ``idx`` on exactly those points; with the scene's own descriptors it changes ``idx`` on fewer than a
  tenth of them (printed: the gap the zero-query construction closes);
* the noisy ray images keep the LM loop alive: at every iteration 1 .. 10 at least 5 % of the points move and at
  least 5 % do not, and on the finer noise the converged share lies strictly between 10 % and 90 %;
* the warm starts decode outside the clamp interval for at least a quarter of the points and change the result on
  at least 5 % of them;
* the parameter extremes do what they are for, every degenerate case changes the oracle's output on at least one
  pixel, and the occlusion scene holds at least 8 converged pixels at each of the three distances around the
  threshold and at least 8 of each kind that only one of the two conditions of ``valid`` decides;
* white descriptors make every level pair the fallback cases rely on differ on at least 25 % of the pixels;
* ``oracle.normalize`` equals ``torch.nn.functional.normalize`` bit for bit, NaN positions included.

Each test prints the counts it asserts (``pytest -s``).
"""
import numpy as np
import pytest
import torch

import match_proj_cases as E
import oracle.oracle as O


def _by_family(f):
    return [n for n in E.PROJ_NAMES if n.startswith(f + "/")]


def test_names_are_unique_and_cases_well_formed():
    assert len(set(E.PROJ_NAMES)) == len(E.PROJ_NAMES) and len(set(E.FALLBACK_NAMES)) == len(E.FALLBACK_NAMES)
    for name in E.PROJ_NAMES:
        cs = E.case(name)
        B, H, W, _ = cs.X11.shape
        assert B * H * W <= 48 * 64, name  # quick on the device and in the oracle
        assert cs.X21.shape == (B, H, W, 3) and cs.D11.shape == cs.D21.shape == (B, H, W, 24)
        assert not cs.D21.any() and np.isfinite(cs.D11).all()
        assert all(a.dtype == np.float32 for a in (cs.X11, cs.X21, cs.D11, cs.D21))
        assert cs.idx_init is None or (cs.idx_init.shape == (B, H * W) and cs.idx_init.dtype == np.int64)
        assert set(cs.params) <= set(E.DEFAULTS)


@pytest.mark.parametrize("name", E.PROJ_NAMES)
def test_zero_query_refine_is_the_identity(name):
    """idx of the full match (refine at radius 3, dilation_max 5 over a white D11) is pixel_to_lin of the truncated
    centre, and the centre lies in the clamp interval"""
    cs = E.case(name)
    W, H = cs.X11.shape[2], cs.X11.shape[1]
    idx, valid = E.expected_match(name)
    idx0, valid0 = E.expected_match(name, 0)
    np.testing.assert_array_equal(idx, idx0)
    np.testing.assert_array_equal(valid, valid0)
    _, _, _, p_new, _ = E.expected_iter_proj(name)
    np.testing.assert_array_equal(idx, O.pixel_to_lin(p_new.astype(np.int64), W))
    assert (p_new[..., 0] >= 1).all() and (p_new[..., 0] <= W - 2).all()
    assert (p_new[..., 1] >= 1).all() and (p_new[..., 1] <= H - 2).all()


def test_method_zero_queries_show_a_one_pixel_centre_error():
    """The gap this suite closes, on a 48x64 synthetic pair"""
    from m3s.synthetic import make_pair

    H, W = 48, 64
    P = make_pair(H, W, seed=0)
    X, D = P["X"].numpy(), P["D"].numpy()
    rays, pts, p_init = O.prep_for_iter_proj(X[:1], X[1:], None)
    p1 = O.iter_proj(rays, pts, p_init, 10, 1e-8, 1e-6)[0].astype(np.int64)
    rng = np.random.default_rng(0)
    hit = np.zeros(H * W, bool)
    hit[rng.choice(H * W, size=H * W // 100, replace=False)] = True
    step = np.array([[1, 0], [-1, 0], [0, 1], [0, -1]], np.int64)[rng.integers(0, 4, size=H * W)]
    p1x = p1.copy()
    p1x[0, hit] += step[hit]  # centres lie in [1, W-2] x [1, H-2]: still inside the image
    D21 = D[1:].reshape(1, H * W, -1)
    zero = np.zeros_like(D21)
    lin = lambda p: O.pixel_to_lin(p, W)[0]
    assert np.array_equal(lin(O.refine_matches(D[:1], zero, p1, 3, 5)), lin(p1))
    changed_zero = lin(O.refine_matches(D[:1], zero, p1x, 3, 5)) != lin(p1)
    changed_own = lin(O.refine_matches(D[:1], D21, p1x, 3, 5)) != lin(O.refine_matches(D[:1], D21, p1, 3, 5))
    print(f"perturbed {int(hit.sum())} of {H * W} centres by one pixel: idx changes on {int(changed_zero.sum())} with "
          f"zero queries, on {int(changed_own.sum())} with the scene's own D21")
    assert np.array_equal(changed_zero, hit)
    assert changed_own.sum() < hit.sum() / 10


@pytest.mark.parametrize("key", list(E.NOISY))
def test_noisy_scene_keeps_every_lm_iteration_live(key):
    X11, X21 = E.noisy_scene(*E.NOISY[key])
    rays, pts, p_init = O.prep_for_iter_proj(X11, X21, None)
    n = pts.shape[1]
    prev, conv = O.iter_proj(rays, pts, p_init, 0, 1e-8, 1e-6)
    for k in range(1, 11):
        p, conv = O.iter_proj(rays, pts, p_init, k, 1e-8, 1e-6)
        moved = int((p != prev).any(-1).sum())
        print(f"{key} sigma {E.NOISY[key][0]}: iteration {k} moved {moved}, unmoved {n - moved} of {n}")
        assert moved >= 0.05 * n and n - moved >= 0.05 * n
        prev = p
    share = float(conv.mean())
    print(f"{key}: converged share after 10 iterations {share:.3f}")
    if key == "s04":
        assert 0.1 < share < 0.9
    # the device cases are these scenes
    for it in E.LM_ITERS:
        cs = E.case(f"lm/{key}_it{it}")
        assert np.array_equal(cs.X11, X11) and cs.params == {"max_iter": it}


@pytest.mark.parametrize("kind", E.WARM_KINDS)
def test_warm_start_decodes_outside_and_decides_the_result(kind):
    cs = E.case("warm/" + kind)
    H, W = cs.X11.shape[1:3]
    N = H * W
    i = cs.idx_init[0]
    miss = float(E.clamp_interval_miss(cs.idx_init, H, W).mean())
    idx, _ = E.expected_match(cs.name)
    cold = O.match(cs.X11, cs.X21, cs.D11, cs.D21)[0]
    differs = float((idx != cold).mean())
    print(f"warm/{kind}: start outside the clamp interval {miss:.3f}, result differs from the cold one {differs:.3f}")
    if kind != "one_interior":
        assert miss >= 0.25
    assert differs >= 0.05
    if kind == "range":
        assert i.min() == -3 * N and i.max() == 4 * N and {-1, -N - 1} <= set(i.tolist())
        assert ((i < 0).mean() > 0.25) and ((i >= N).mean() > 0.25)
    if kind == "huge":
        assert {2 ** 40 + 7, -(2 ** 40 + 7), 2 ** 31 - 1, 2 ** 31} <= set(i.tolist())
        # floor semantics: the decoded column of a negative index lies in [0, W)
        p = O.lin_to_pixel(i, W)
        assert (p[:, 0] >= 0).all() and (p[:, 0] < W).all() and (p[i < 0, 1] < 0).all()
    if kind.startswith("one"):
        assert len(set(i.tolist())) == 1
    if kind == "border":
        assert i[:4].tolist() == [0, W - 1, N - W, N - 1]
        u, v = i % W, i // W
        assert ((u == 0) | (u == W - 1) | (v == 0) | (v == H - 1)).all()
        assert all((v == r).any() for r in (0, H - 1)) and all((u == c).any() for c in (0, W - 1))


def test_parameter_extremes():
    res = {}
    for name in _by_family("param"):
        _, valid = E.expected_match(name)
        _, _, p_init, p_new, conv = E.expected_iter_proj(name)
        H, W = E.case(name).X11.shape[1:3]
        start = np.clip(p_init, 1, [W - 2, H - 2]).astype(np.float32)
        res[name.split("/")[1]] = (float(valid.mean()), float(conv.mean()), float((p_new == start).all(-1).mean()))
        print(f"{name}: valid {res[name.split('/')[1]][0]:.3f}, converged {res[name.split('/')[1]][1]:.3f}, "
              f"frozen at the start {res[name.split('/')[1]][2]:.3f}")
    assert res["lambda_init=1e+06"][2] >= 0.9 and res["lambda_init=0"][2] <= 0.1
    assert res["convergence_thresh=0"][0] == 0 and res["convergence_thresh=0"][1] == 0
    assert res["convergence_thresh=1e+30"][1] == 1
    assert 0.1 < res["convergence_thresh=1e-06"][0] < res["convergence_thresh=1e+30"][0] < 0.9
    assert res["dist_thresh=0"][0] == 0 and res["dist_thresh=0"][1] > 0.1
    assert res["dist_thresh=inf"][0] == res["dist_thresh=inf"][1] > 0.1  # valid is the converged flag alone
    assert res["dist_thresh=0.1"][0] > 0.1


@pytest.mark.parametrize("name", _by_family("degen"))
def test_degenerate_case_changes_the_oracles_output(name):
    H, W, seed = E.CLEAN
    X11, X21 = E.scene(1, H, W, seed)
    cs = E.case(name)
    clean = O.match(X11, X21, cs.D11, cs.D21)
    idx, valid = E.expected_match(name)
    di, dv = int((idx != clean[0]).sum()), int((valid != clean[1]).sum())
    print(f"{name}: idx differs from the clean scene's on {di} pixels, valid on {dv}")
    assert di + dv >= 1
    if name.startswith("degen/const"):
        rays = E.expected_iter_proj(name)[0]
        assert not rays[..., 3:].any()  # zero gradients: A = lambda I


def test_occlusion_scene_sits_on_the_threshold():
    cs = E.case("occ/threshold")
    dg = O.match_diag(cs.X11, cs.X21, cs.D11, cs.D21)
    conv, d = dg["conv"], dg["d"]
    thr = np.float32(0.1)
    for k, t in E.occlusion_targets().items():
        n = int((conv & (d == t)).sum())
        print(f"occ: converged pixels with d {k} float32(0.1) exactly ({t!r}): {n}")
        assert n >= 8
    a, b = int((~conv & (d < thr)).sum()), int((conv & (d > thr)).sum())
    print(f"occ: conv false with d below the threshold {a}, conv true with d above it {b}")
    assert a >= 8 and b >= 8
    np.testing.assert_array_equal(dg["valid"][..., 0], conv & (d < thr))


def test_white_descriptors_make_every_level_count():
    def share(a, b):
        return float((a != b).any(-1).mean())

    pairs = [("dilation_max 9 against 8", E.expected_refine("dil/9"), E.expected_refine("dil/9", dilation_max=8)),
             ("dilation_max 10 against 9", E.expected_refine("dil/10"), E.expected_refine("dil/10", dilation_max=9))]
    pairs += [(f"radius {r} against 3", E.expected_refine(f"radius/{r}"), E.expected_refine(f"radius/{r}", radius=3))
              for r in (1, 2, 4)]
    pairs += [(f"F = {F} against the start", E.expected_refine(f"F/{F}"), E.fallback(f"F/{F}").p1) for F in (16, 32)]
    for what, a, b in pairs:
        s = share(a, b)
        print(f"white descriptors, {what}: differ on {s:.3f} of the pixels")
        assert s >= 0.25
    np.testing.assert_array_equal(E.expected_refine("dil/0"), E.fallback("dil/0").p1)
    # the route through match gives the op's result on the oracle's centres
    for name in E.FALLBACK_MATCH_NAMES:
        fb = E.fallback(name)
        W = fb.D11.shape[2]
        np.testing.assert_array_equal(E.expected_fallback_match(name)[0], O.pixel_to_lin(E.expected_refine(name), W))


@pytest.mark.parametrize("name", ["ragged/333", "tile_outside/near", "tile_outside/far", "f32/5"])
def test_outside_centres_move_in_or_stay_out(name):
    fb = E.fallback(name)
    H, W = fb.D11.shape[1:3]
    r = E.expected_refine(name)
    out = lambda p: (p[..., 0] < 0) | (p[..., 0] >= W) | (p[..., 1] < 0) | (p[..., 1] >= H)
    moved, stay = float((r != fb.p1).any(-1).mean()), float(out(r).mean())
    print(f"{name}: {float(out(fb.p1).mean()):.3f} of the centres start outside the image, {moved:.3f} move, "
          f"{stay:.3f} stay outside")
    assert moved >= 0.5 and stay >= 0.05
    np.testing.assert_array_equal(r[out(r)], fb.p1[out(r)])  # a result outside the image is the untouched start
    if name == "tile_outside/far":
        assert (np.abs(fb.p1) > 32767).any(-1).mean() >= 0.05
        assert {-32769, -32768, 32767, 32768} <= set(fb.p1.reshape(-1).tolist())
    if name == "ragged/333":
        assert fb.p1.shape[1] == 333 != H * W and E.fallback("ragged/1").p1.shape[1] == 1


def test_oracle_normalize_is_torchs_bit_for_bit():
    x = E.NORMALIZE_ROWS
    got = O.normalize(x)
    ref = torch.nn.functional.normalize(torch.from_numpy(x), dim=-1).numpy()
    for row, g, r in zip(x, got, ref):
        print(f"normalize {row}: oracle {g}, torch {r}")
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    np.testing.assert_array_equal(got[ok].view(np.uint32), ref[ok].view(np.uint32))
    assert np.isnan(ref[3]).all() and np.isnan(ref[4]).all()  # one NaN component: three NaNs
    # and on ordinary points, where the change must not show: the golden rays / pts stay bit-exact (test_oracle.py)
    pts = np.random.default_rng(0).standard_normal((4096, 3)).astype(np.float32)
    ref = torch.nn.functional.normalize(torch.from_numpy(pts), dim=-1).numpy()
    np.testing.assert_array_equal(O.normalize(pts).view(np.uint32), ref.view(np.uint32))
