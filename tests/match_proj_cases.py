"""Edge cases of the front half of ``match`` (test infrastructure, CPU only: numpy and the oracle, no device code).

The front half is prep_rays_kernel, the LM projection search (csrc/m3s_proj.hpp: ``proj_occlusion_kernel`` and the
fused refine launch's prologue), the occlusion test, ``lin_to_pixel_f`` and the per-pixel fallback kernels of
csrc/matching.hip. Shared by tests/test_match_proj_host.py (which proves on the CPU that every case does what it is
for) and tests/test_gpu_match_proj_edges.py (which runs the device paths on them and compares exactly).

Projection cases (``case(name)``, names in ``PROJ_NAMES``) carry ``D21 = 0``. Every candidate of the refine then
scores +0, and +0 never beats the running maximum under the strict ``>``: the refine is the identity and ``idx`` is
``pixel_to_lin`` of the projection's truncated centre, so a centre that is one pixel off shows in ``idx`` itself.
(With the scene's own descriptors the refine pulls nearly every centre back to the same peak and hides it.) ``D11``
stays an ordinary white unit descriptor image: the refine still runs all its levels on it.

Families:
  size      the smallest images, one past a prep tile / two refine tiles, exactly one prep tile, B = 2
  lm        Gaussian noise on X11 (sigma 0.1 and 0.04 on 24x40) makes a ray image rough enough that every one of the
            ten LM iterations both accepts and rejects steps; max_iter 0, 1, 2, 3, 10
  warm      idx_1_to_2_init far outside [0, N), at the 2^31 boundary of lin_to_pixel_f's two branches, all on one
            pixel, on the border; on the sigma 0.1 scene, where the start decides the result
  param     lambda_init, convergence_thresh, dist_thresh at their extremes
  degen     constant X11 (zero gradients, A = lambda I, with lambda_init 0 a NaN step), zero / NaN / inf pixels in X11
            (interior, corner and border row, so the reflect padding of the gradient stencil carries them) and in X21,
            X21 points with a norm below F.normalize's eps
  occ       X21 = s X11 with s nudged by ulps until the occlusion distance is float32(0.1) exactly, or one of its two
            neighbours

Fallback cases (``fallback(name)``, names in ``FALLBACK_NAMES``) use white unit descriptors for both images, on which
every level of the coarse-to-fine search moves most pixels, so a dropped level shows.
"""
import collections
import functools

import numpy as np

import oracle.oracle as O

f32 = np.float32
DEFAULTS = dict(max_iter=10, lambda_init=1e-8, convergence_thresh=1e-6, dist_thresh=0.1)

# name, family, X11 / X21 (B,H,W,3), D11 / D21 (B,H,W,24), idx_init (B,H*W) int64 or None, params: the entries of
# config["matching"] (and keyword arguments of oracle.match) that differ from DEFAULTS
Case = collections.namedtuple("Case", "name family X11 X21 D11 D21 idx_init params")


def _pair(H, W, seed, Fd=24):
    from m3s.synthetic import make_pair

    X = make_pair(H, W, Fd=Fd, seed=seed)["X"].numpy()
    return X[0].copy(), X[1].copy()


def scene(B, H, W, seed):
    """X11, X21 (B,H,W,3) of B synthetic pairs with different content (seeds seed, seed + 1, ..)"""
    Xs = [_pair(H, W, seed + b) for b in range(B)]
    return np.stack([x[0] for x in Xs]), np.stack([x[1] for x in Xs])


def white(shape, seed):
    """white unit descriptors (..., F) fp32"""
    d = np.random.default_rng(seed).standard_normal(shape)
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(f32)


def noisy_scene(sigma, seed=0, H=24, W=40):
    """A pair whose ray image is rough: Gaussian noise of ``sigma`` on X11 (depth about 2)"""
    X11, X21 = scene(1, H, W, 70)
    rng = np.random.default_rng(seed)
    return (X11 + f32(sigma) * rng.standard_normal(X11.shape).astype(f32)).astype(f32), X21


# the noisy scenes of the lm / warm families: (sigma, seed)
NOISY = {"s10": (0.1, 0), "s04": (0.04, 0)}
LM_ITERS = (0, 1, 2, 3, 10)
CLEAN = (24, 40, 80)  # H, W, seed of the smooth scene of the param / degen families
# degenerate pixel positions (u, v) on the CLEAN scene. The scene's flow is (+3.3, -2.7): the points of the top rows
# and the right columns of image 2 project past the top / right border and are clamped to row 1 / column W - 2, so the
# top-right corner and the top row are the border positions whose stencil taps the search actually reads.
POSITIONS = {"interior": (17, 11), "corner": (39, 0), "border": (21, 0)}
KINDS = ("zero", "nan", "nan1", "inf1")


def _degenerate_pixel(kind, px, comp):
    px = px.copy()
    if kind == "zero":
        px[:] = 0.0
    elif kind == "nan":
        px[:] = np.nan
    elif kind == "nan1":
        px[comp] = np.nan
    elif kind == "inf1":
        px[comp] = np.inf
    else:
        raise KeyError(kind)
    return px


def clamp_interval_miss(idx_init, H, W):
    """per point: the decoded start pixel (oracle.lin_to_pixel) lies outside the clamp interval [1, W-2] x [1, H-2]"""
    p = O.lin_to_pixel(np.asarray(idx_init), W)
    return (p[..., 0] < 1) | (p[..., 0] > W - 2) | (p[..., 1] < 1) | (p[..., 1] > H - 2)


def _warm_init(kind, H, W):
    N = H * W
    n = np.arange(N, dtype=np.int64)
    if kind == "range":  # anywhere in [-3N, 4N], the ends and the two -1 cases included
        i = np.random.default_rng(5).integers(-3 * N, 4 * N + 1, size=N).astype(np.int64)
        i[:6] = [-1, -N - 1, -3 * N, 4 * N, 0, N]
    elif kind == "huge":  # both branches of lin_to_pixel_f and its floor semantics for negative values
        vals = np.array([2 ** 40 + 7, -(2 ** 40 + 7), 2 ** 31 - 1, 2 ** 31, -(2 ** 31), -(2 ** 31) - 1, 2 ** 31 + W + 3],
                        np.int64)
        i = np.where(n % 2 == 0, n, vals[(n // 2) % len(vals)])
    elif kind == "one_corner":  # every point starts on the last pixel
        i = np.full(N, N - 1, np.int64)
    elif kind == "one_interior":  # every point starts on one interior pixel
        i = np.full(N, (H // 2) * W + W // 2, np.int64)
    elif kind == "border":  # the four corners first, then round the border rows and columns
        u, v = n % W, n // W
        ring = n[(u == 0) | (u == W - 1) | (v == 0) | (v == H - 1)]
        corners = np.array([0, W - 1, N - W, N - 1], np.int64)
        ring = np.concatenate((corners, ring[~np.isin(ring, corners)]))
        i = ring[n % len(ring)]
    else:
        raise KeyError(kind)
    return i[None].copy()


WARM_KINDS = ("range", "huge", "one_corner", "one_interior", "border")

OCC_SHAPE = (48, 64, 90)  # H, W, seed
OCC_ULPS = 40
OCC_FAR = 4  # every OCC_FAR-th class: d far above the threshold


def occlusion_targets(dist_thresh=0.1):
    t = f32(dist_thresh)
    return {"below": np.nextafter(t, f32(0)), "equal": t, "above": np.nextafter(t, f32(1))}


def _occlusion_scene():
    """X21 = X11 * s (the directions unchanged, so the search lands where it would for a plain copy); s starts from
    1 +- dist_thresh / |X11| and is nudged by up to OCC_ULPS ulps so that norm3(X11[p1] - X21) hits the point's target
    (class n % OCC_FAR: below, equal, above; class 3: s = 1 +- 2 dist_thresh / |X11|, far above). p1 comes from a first
    oracle run; the border pixels keep s = 1 (clamped centres: not converged, d about a pixel's spacing)."""
    H, W, seed = OCC_SHAPE
    X11, _ = scene(1, H, W, seed)
    N = H * W
    n = np.arange(N)
    u, v = n % W, n // W
    inner = (u >= 1) & (u <= W - 2) & (v >= 1) & (v <= H - 2)
    nrm = O.norm3(X11).reshape(-1)
    sign = np.where((u + v) % 2 == 0, 1.0, -1.0)
    cls = n % OCC_FAR
    s0 = np.where(inner, 1.0 + sign * np.where(cls == 3, 0.2, 0.1) / nrm, 1.0).astype(f32)
    Xf = X11.reshape(-1, 3)
    D0 = np.zeros((1, H, W, 24), f32)
    first = O.match_diag(X11, (Xf * s0[:, None]).reshape(1, H, W, 3).astype(f32), D0, D0)
    Xg = Xf[first["p1"][0]]
    want = np.array(list(occlusion_targets().values()) + [np.inf], f32)[cls]
    s = s0.copy()
    found = ~inner | (cls == 3)
    for k in sorted(range(-OCC_ULPS, OCC_ULPS + 1), key=abs):
        sk = s0.copy()
        for _ in range(abs(k)):
            sk = np.nextafter(sk, f32(np.inf if k > 0 else -np.inf))
        d = O.norm3(Xg - (Xf * sk[:, None]).astype(f32))
        hit = ~found & (d == want)
        s[hit] = sk[hit]
        found |= hit
    return X11, (Xf * s[:, None]).reshape(1, H, W, 3).astype(f32)


def _build(name):
    family, _, rest = name.partition("/")
    params, init = {}, None
    if family == "size":
        shape = {"3x3": (1, 3, 3), "3x40": (1, 3, 40), "40x3": (1, 40, 3), "4x5": (1, 4, 5), "17x65": (1, 17, 65),
                 "9x33": (1, 9, 33), "16x16": (1, 16, 16), "b2_12x20": (2, 12, 20)}[rest]
        X11, X21 = scene(*shape, seed=60)
    elif family == "lm":
        key, it = rest.split("_it")
        X11, X21 = noisy_scene(*NOISY[key])
        params["max_iter"] = int(it)
    elif family == "warm":
        X11, X21 = noisy_scene(*NOISY["s10"])
        init = _warm_init(rest, *X11.shape[1:3])
    elif family == "param":
        key, val = rest.split("=")
        X11, X21 = scene(1, 20, 28, 75)
        params[key] = float(val)
    elif family == "degen":
        H, W, seed = CLEAN
        X11, X21 = scene(1, H, W, seed)
        if rest.startswith("const"):  # the ray (0, 0, 1): every stencil product is exact, the gradients are zero
            X11[:] = np.array([0.0, 0.0, 2.0], f32)
            if rest == "const_lam0":
                params["lambda_init"] = 0.0
        elif rest == "flat":  # a constant whose stencil sums leave rounding residue: gradients of about 1e-9
            X11[:] = np.array([0.3, -0.2, 2.0], f32)
        elif rest.startswith("x11_"):
            _, kind, pos = rest.split("_")
            u, v = POSITIONS[pos]
            X11[0, v, u] = _degenerate_pixel(kind, X11[0, v, u], list(POSITIONS).index(pos))
        elif rest.startswith("x21_tiny"):
            X21[0, 11, 17] = [3e-13, -4e-13, 0.0]  # norm 5e-13: divided by eps, not by the norm
            X21[0, 5, 30] = [1e-30, 0.0, 0.0]  # the square underflows to 0
        elif rest.startswith("x21_"):  # the three positions at once: X21 feeds no stencil
            kind = rest.split("_")[1]
            for c, (u, v) in enumerate(((17, 11), (0, 0), (21, H - 1))):
                X21[0, v, u] = _degenerate_pixel(kind, X21[0, v, u], c)
        else:
            raise KeyError(name)
    elif family == "occ":
        X11, X21 = _occlusion_scene()
    else:
        raise KeyError(name)
    B, H, W, _ = X11.shape
    D11 = white((B, H, W, 24), seed=11)
    cs = Case(name, family, np.ascontiguousarray(X11, f32), np.ascontiguousarray(X21, f32), D11,
              np.zeros_like(D11), init, params)
    for a in cs[2:7]:
        if a is not None:
            a.setflags(write=False)
    return cs


PROJ_NAMES = (
    ["size/" + s for s in ("3x3", "3x40", "40x3", "4x5", "17x65", "9x33", "16x16", "b2_12x20")]
    + [f"lm/{k}_it{it}" for k in NOISY for it in LM_ITERS]
    + ["warm/" + k for k in WARM_KINDS]
    + [f"param/lambda_init={v}" for v in ("0", "1e-08", "1", "1e+06")]
    + [f"param/convergence_thresh={v}" for v in ("0", "1e-06", "1e+30")]
    + [f"param/dist_thresh={v}" for v in ("0", "0.1", "inf")]
    + ["degen/const", "degen/const_lam0", "degen/flat"]
    + [f"degen/x11_{k}_{p}" for k in KINDS for p in POSITIONS]
    + [f"degen/x21_{k}" for k in KINDS] + ["degen/x21_tiny"]
    + ["occ/threshold"]
)


@functools.lru_cache(maxsize=None)
def case(name):
    return _build(name)


def match_kwargs(cs):
    return {**DEFAULTS, **cs.params}


@functools.lru_cache(maxsize=None)
def expected_match(name, radius=3):
    """(idx, valid) of oracle.match on the case (radius 3: the zero-query refine, dilation_max 5; radius 0: none)"""
    cs = case(name)
    return O.match(cs.X11, cs.X21, cs.D11, cs.D21, cs.idx_init, radius=radius, dilation_max=5, **match_kwargs(cs))


@functools.lru_cache(maxsize=None)
def expected_iter_proj(name):
    """(rays, pts, p_init, p_new, converged): oracle.prep_for_iter_proj's arrays and oracle.iter_proj on them"""
    cs = case(name)
    k = match_kwargs(cs)
    rays, pts, p_init = O.prep_for_iter_proj(cs.X11, cs.X21, cs.idx_init)
    p_new, conv = O.iter_proj(rays, pts, p_init, k["max_iter"], k["lambda_init"], k["convergence_thresh"])
    return rays, pts, p_init, p_new, conv


# ------------------------------------------------------------------------------------------------
# fallback kernels: refine_lin_kernel / refine_f16_kernel at F = 16, 32 and at dilation_max > 8 or radius != 3,
# the reference op with N != H W, the tile path with centres outside the image, the fp32 op
# ------------------------------------------------------------------------------------------------
# name, X11 / X21 (for the route through match; None: op only), D11 (B,H,W,F), D21 (B,N,F), p1 (B,N,2) int64 (the
# centres handed to the op), radius, dilation_max, half
Fallback = collections.namedtuple("Fallback", "name X11 X21 D11 D21 p1 radius dilation_max half")
FB_SHAPE = (32, 64)


def outside_p1(rng, B, N, lo=-9, hi=40):
    return rng.integers(lo, hi + 1, size=(B, N, 2)).astype(np.int64)


def _build_fallback(name):
    H, W = FB_SHAPE
    kind, _, rest = name.partition("/")
    rng = np.random.default_rng(17)
    X11 = X21 = None
    radius, dmax, half = 3, 5, True
    if kind in ("F", "dil", "radius"):  # the whole image, centres from the oracle's projection: match and the op
        F = int(rest) if kind == "F" else 24
        dmax = int(rest) if kind == "dil" else 5
        radius = int(rest) if kind == "radius" else 3
        a, b = _pair(H, W, 95, Fd=F)
        X11, X21 = a[None], b[None]
        D11, D21 = white((1, H, W, F), 21), white((1, H * W, F), 22)
        rays, pts, p_init = O.prep_for_iter_proj(X11, X21, None)
        p1 = O.iter_proj(rays, pts, p_init, 10, 1e-8, 1e-6)[0].astype(np.int64)
    elif kind == "ragged":  # the reference op with N != H W queries on 20x28, a sixth of the centres stay outside
        N = int(rest)
        H, W = 20, 28
        D11, D21 = white((1, H, W, 24), 23), white((1, N, 24), 24)
        p1 = outside_p1(rng, 1, N)
    elif kind == "tile_outside":  # N = H W, F = 24, radius 3: the LDS tile path with centres outside the image
        H, W = 24, 40
        D11, D21 = white((2, H, W, 24), 25), white((2, H * W, 24), 26)
        p1 = outside_p1(rng, 2, H * W, -9, 50)
        if rest == "far":  # past the signed 16-bit range of level_window's packed bbox
            far = rng.random((2, H * W)) < 0.1
            p1[far] = rng.choice(np.array([-40000, -32769, -32768, 32767, 32768, 40000], np.int64), size=(int(far.sum()), 2))
    elif kind == "f32":  # the fp32 op at a width no half instance has
        D11, D21 = white((1, H, W, 5), 27), white((1, H * W, 5), 28)
        p1 = outside_p1(rng, 1, H * W, -9, 70)
        half = False
    else:
        raise KeyError(name)
    fb = Fallback(name, X11, X21, D11, D21, p1, radius, dmax, half)
    for a in fb[1:6]:
        if a is not None:
            a.setflags(write=False)
    return fb


FALLBACK_NAMES = (["F/16", "F/32", "dil/9", "dil/10", "dil/0", "radius/1", "radius/2", "radius/4"]
                  + ["ragged/333", "ragged/1", "tile_outside/near", "tile_outside/far", "f32/5"])
# the cases that also go through match (the others reach their kernel through the reference op only)
FALLBACK_MATCH_NAMES = ["F/16", "F/32", "dil/9", "dil/10", "radius/1", "radius/2", "radius/4"]


@functools.lru_cache(maxsize=None)
def fallback(name):
    return _build_fallback(name)


@functools.lru_cache(maxsize=None)
def expected_refine(name, radius=None, dilation_max=None):
    """oracle.refine_matches on the case (or at another radius / dilation_max, for the host file's level pairs)"""
    fb = fallback(name)
    return O.refine_matches(fb.D11, fb.D21, fb.p1, fb.radius if radius is None else radius,
                            fb.dilation_max if dilation_max is None else dilation_max, half=fb.half)


@functools.lru_cache(maxsize=None)
def expected_fallback_match(name):
    fb = fallback(name)
    H, W = fb.X11.shape[1:3]
    return O.match(fb.X11, fb.X21, fb.D11, fb.D21.reshape(1, H, W, -1), radius=fb.radius,
                   dilation_max=fb.dilation_max)


# ------------------------------------------------------------------------------------------------
# normalisation: the rows oracle.normalize must share with torch.nn.functional.normalize, bit for bit
# ------------------------------------------------------------------------------------------------
NORMALIZE_ROWS = np.array([
    [0.0, 0.0, 0.0],
    [3e-13, -4e-13, 0.0],            # norm below eps
    [1e-30, 0.0, 0.0],               # the square underflows
    [np.nan, 1.0, 2.0],              # one NaN component: torch's clamp_min propagates the NaN norm
    [1.0, np.nan, 2.0],
    [np.nan, np.nan, np.nan],
    [np.inf, 1.0, 2.0],
    [1.0, -np.inf, 2.0],
    [3e19, -2e19, 1e19],             # squares overflow
    [3e19, 1.0, 0.0],
    [0.3, -0.2, 2.0],
    [-1.5, 0.25, 0.125],
    [1e-6, 2e-6, -3e-6],
], f32)
