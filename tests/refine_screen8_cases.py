"""Cases and the numpy restatement for the int8 pre-screen of the refine levels d >= 2 (refine.hip ScreenI8).

Restatement (exact, from the half-rounded values, as prep_rays_kernel and screen_bound8 compute them):
  quantise8(x_h)  = clamp(rint(127 x_h), -127, 127), rint = round-half-even; 127 x_h is exact in fp32
  S8              = sum q8_k c8_k (int32, exact)
  E8              = (0.5 / 127) (c1max + |q8|_1 / 127),  c1max = max over the image of |c_h|_1
  B               = 0.0125 |q_h|_2 cmax + 2^-18,         cmax  = max over the image of |c_h|_2
  B8              = B + E8 bounds |S_half - S8 / 127^2| when every |q_h,k| <= 1 and |c_h,k| <= 1
S_half is the c10::Half chain: from +0, s = half(s + half(q_k c_k)) over k = 0..23, with the oracle's f32 -> f16.

GPU cases: `gpu_cases()` yields (name, dict) with X11, X21, D11, D21 (1,H,W,.) float32, idx_init (or None) and
dilation_max; what each reaches is in its `reaches` string (the issue's table, the smallest shape for each branch).
"""
import numpy as np

import oracle.oracle as O

TW, TH = 32, 8  # refine tile
ONE_FILL_ROWS, ONE_FILL_COLS = 30, 56  # the int8 window that holds both planes (refine.hip RT_8ROWS, RT_8COLS)
WIN_ROWS, WIN_COLS = 40, 64
GPU_CASE_NAMES = ("smooth_48x64", "border_50x70", "scattered_96x128", "frame_fallback", "lane_fallback", "constant",
                  "ladder_0p03", "nan", "inf", "layouts_d3")


def half(x):
    """f32 -> f16 -> f32 with the oracle's conversion (RNE, == torch .half())"""
    x = np.ascontiguousarray(x, np.float32)
    return O.to_half_bits(x).view(np.float16).astype(np.float32).reshape(x.shape)


def quantise8(xh):
    """int8 code of a half-rounded value (float32 array holding half values)"""
    xh = np.asarray(xh, np.float32)
    return np.clip(np.rint(np.float32(127.0) * xh), -127, 127).astype(np.int32)


def half_chain(qh, ch):
    """c10::Half chain over the last axis of half-valued float32 arrays (broadcast), the oracle's rounding per step"""
    qh, ch = np.broadcast_arrays(np.asarray(qh, np.float32), np.asarray(ch, np.float32))
    s = np.zeros(qh.shape[:-1], np.float32)
    for k in range(qh.shape[-1]):
        s = half(s + half(qh[..., k] * ch[..., k]))
    return s


def s8(q8, c8):
    return (np.asarray(q8, np.int64) * np.asarray(c8, np.int64)).sum(-1)


def bound_B(qh, cmax):
    """today's bound |S_half - S_dot2| (and so |S_half - S_real|), in float64 from the half values"""
    return 0.0125 * np.linalg.norm(np.asarray(qh, np.float64), axis=-1) * cmax + 2.0 ** -18


def bound_E8(q8, c1max):
    return (0.5 / 127.0) * (c1max + np.abs(np.asarray(q8, np.float64)).sum(-1) / 127.0)


# ------------------------------------------------------------------------------------------
# host operand pairs for the bound test
# ------------------------------------------------------------------------------------------
def bound_pairs(n_random=120000, seed=0):
    """(q, c) float32 arrays (n, 24) with every |component| <= 1 after half rounding: random pairs at several
    scales, components at exactly +-1, zeros, half subnormals, and sign patterns that make every quantisation error
    add up (components just below an RNE midpoint of the quantiser against full-scale partners)."""
    rng = np.random.default_rng(seed)
    qs, cs = [], []

    def add(q, c):
        qs.append(np.asarray(q, np.float32).reshape(-1, 24))
        cs.append(np.asarray(c, np.float32).reshape(-1, 24))

    n = n_random // 4
    add(rng.uniform(-1, 1, (n, 24)), rng.uniform(-1, 1, (n, 24)))  # dense, |x| up to 1
    u = rng.standard_normal((2, n, 24))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    add(u[0], u[1])  # unit vectors (the descriptors' scale)
    add(rng.uniform(-1, 1, (n, 24)) * 10.0 ** rng.uniform(-6, 0, (n, 1)),
        rng.uniform(-1, 1, (n, 24)) * 10.0 ** rng.uniform(-6, 0, (n, 1)))  # mixed scales down to subnormal products
    add(np.sign(rng.standard_normal((n, 24))) * rng.choice([0.0, 1.0], (n, 24)),
        np.sign(rng.standard_normal((n, 24))) * rng.choice([0.0, 1.0], (n, 24)))  # exactly +-1 and zeros
    # half subnormals (below 2^-14) and the smallest one
    sub = rng.uniform(-1, 1, (2000, 24)) * 2.0 ** -15
    add(sub, rng.uniform(-1, 1, (2000, 24)))
    add(np.full((1, 24), 2.0 ** -24), np.full((1, 24), 1.0))
    add(np.zeros((1, 24)), np.ones((1, 24)))
    # worst-case signs: c just below a quantiser midpoint (error -> +0.5 / 127 each) against q = +-1 of one sign
    # pattern, then the same with the roles swapped and with alternating signs
    mids = (np.arange(0, 127)[:, None] + 0.5) / 127.0  # (127, 1)
    for eps in (-2.0 ** -12, 2.0 ** -12):
        cm = np.clip(np.broadcast_to(mids + eps, (127, 24)), -1, 1)
        for sgn in (np.ones(24), -np.ones(24), np.where(np.arange(24) % 2, -1.0, 1.0)):
            add(np.broadcast_to(sgn, (127, 24)), cm * sgn)
            add(cm * sgn, np.broadcast_to(sgn, (127, 24)))
            add(cm, cm * sgn)
    q, c = np.concatenate(qs), np.concatenate(cs)
    return half(q), half(c)


# ------------------------------------------------------------------------------------------
# GPU cases
# ------------------------------------------------------------------------------------------
def _pair(H, W, seed, **kw):
    from m3s.synthetic import make_pair

    P = make_pair(H, W, seed=seed, **kw)
    return dict(X11=P["X"][:1].numpy(), X21=P["X"][1:].numpy(), D11=P["D"][:1].numpy().copy(),
                D21=P["D"][1:].numpy().copy(), idx_init=None, dilation_max=5)


def first_level_covers(case):
    """(rows, cols) per 32 x 8 tile of the first level's cover (bbox of the projected centres +- 3 d): what decides the
    int8 window layout at d = dilation_max. From the oracle's projection search."""
    X11, X21 = case["X11"], case["X21"]
    _, H, W, _ = X11.shape
    d = case["dilation_max"]
    rays, pts, p_init = O.prep_for_iter_proj(X11, X21, case["idx_init"])
    p_new, _ = O.iter_proj(rays, pts, p_init, 10, 1e-8, 1e-6)
    p1 = p_new.astype(np.int64)[0]
    cu, cv = p1[:, 0], p1[:, 1]
    vv, uu = np.divmod(np.arange(H * W), W)
    ntx = (W + TW - 1) // TW
    tile = (vv // TH) * ntx + uu // TW
    nt = tile.max() + 1
    cnt = np.bincount(tile, minlength=nt)
    fu = np.trunc(np.bincount(tile, cu - uu, nt) / cnt).astype(np.int64)
    fv = np.trunc(np.bincount(tile, cv - vv, nt) / cnt).astype(np.int64)
    inl = (np.abs(cu - uu - fu[tile]) <= 16) & (np.abs(cv - vv - fv[tile]) <= 16)
    big = 1 << 30
    mn = np.full((2, nt), big)
    mx = np.full((2, nt), -big)
    for a, c in enumerate((cu, cv)):
        np.minimum.at(mn[a], tile[inl], c[inl])
        np.maximum.at(mx[a], tile[inl], c[inl])
    return mx[1] - mn[1] + 6 * d + 1, mx[0] - mn[0] + 6 * d + 1


def gpu_cases():
    rng = np.random.default_rng(17)
    out = []

    c = _pair(48, 64, 1)
    c["reaches"] = "the int8 path at d >= 2 on a smooth normalised pair"
    out.append(("smooth_48x64", c))

    c = _pair(50, 70, 2)
    c["reaches"] = "border tiles and candidates outside the image"
    out.append(("border_50x70", c))

    c = _pair(96, 128, 21)
    c["idx_init"] = np.random.default_rng(3).integers(0, 96 * 128, size=(1, 96 * 128)).astype(np.int64)
    c["reaches"] = "window outliers scored in place beside int8 levels (scattered warm start)"
    out.append(("scattered_96x128", c))

    c = _pair(48, 64, 3)
    c["D11"][0, 20, 30, 5] = 1.5
    c["reaches"] = "frame-wide f16 fallback: one D11 component of 1.5"
    out.append(("frame_fallback", c))

    c = _pair(48, 64, 4)
    c["D21"][0, ::3, ::5, 2] = 1.25
    c["D21"][0, 1::7, 3::4, 11] = -1.5
    c["reaches"] = "the lane-level keep-everything path: queries with a component above 1"
    out.append(("lane_fallback", c))

    c = _pair(48, 64, 5)
    c["D11"][:] = c["D11"][0, 0, 0]
    c["D21"][:] = c["D11"][0, 0, 0]
    c["reaches"] = "constant descriptors: every candidate ties, all survive"
    out.append(("constant", c))

    # scores on a 0.03 ladder: D11 = s(u, v) w with a flat unit w (|w_k| = 1 / sqrt(24): 127 c_k is 15..26, so the int8
    # codes are coarse), q = w, s = 0.60 + 0.03 ((3 u + 5 v) mod 7) and a 0.002 ripple against exact ties. The level's
    # best and its runner-up are 0.03 apart: outside the f16 band (0.025), inside the int8 band (0.094)
    c = _pair(48, 64, 6)
    H, W = 48, 64
    w = np.where(rng.random(24) < 0.5, -1.0, 1.0) / np.sqrt(24.0)
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    s = 0.60 + 0.03 * ((3 * uu + 5 * vv) % 7) + 0.002 * rng.random((H, W))
    c["D11"][0] = (s[..., None] * w).astype(np.float32)
    c["D21"][0] = (w + 0.003 * rng.standard_normal((H, W, 24))).astype(np.float32)
    c["reaches"] = "candidates 0.03 apart: inside the int8 band, outside the f16 band, the exact chain decides"
    out.append(("ladder_0p03", c))

    c = _pair(48, 64, 7)
    c["D11"][0, 5, 7, 3] = np.nan
    c["reaches"] = "a NaN descriptor: screen off as today"
    out.append(("nan", c))

    c = _pair(48, 64, 8)
    c["D11"][0, 40, 50, 0] = np.inf
    c["D21"][0, 10, 10, 4] = np.inf
    c["reaches"] = "inf descriptors: screen off as today"
    out.append(("inf", c))

    # first level d = 3 with an 8 degree rotation: a full 32-pixel tile's centres spread over ~5 rows, its cover
    # (8 + 5 + 18 rows) passes the one-fill window's 30 rows and takes two fills; the 6-pixel-wide tiles of the last
    # column (W = 70) spread under a row and take the one fill. test_layout_case_reaches_both checks this premise.
    c = _pair(50, 70, 9, rot_deg=8.0)
    c["dilation_max"] = 3
    c["reaches"] = "both int8 window layouts at d = 3: one fill (narrow tiles) and two fills (full tiles)"
    out.append(("layouts_d3", c))
    return out
