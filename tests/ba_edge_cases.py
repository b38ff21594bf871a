"""Cases, fp64 truth, metric and reach predicates of the BA linearisation edge suite (numpy on the CPU, no GPU import).

tests/test_ba_edges_host.py checks every predicate below on the CPU; tests/test_gpu_ba_edges.py runs the cases through
csrc/ba.hip (ba_pack_kernel, ba_lin_kernel, ba_edge_kernel) and compares the (E, 36) edge-sum table, edge by edge, with
the fp64 build of the oracle. Which shape reaches which path: DESIGN.md, BA, "edge shapes".

Geometry: three cameras 6 degrees apart on make_graph's circle (60 keyframes per turn) inside its box room, pointmaps
ray-cast, matches by reprojection with 5 % random outliers and 90 % of the in-view matches valid, so that most points
of every edge carry weight ("weighted": the match is valid and passes every threshold of the case). The whole graph is
then moved by one Sim(3) (relative poses unchanged), so that keyframe 0 is far from the identity, each keyframe has a
scale of its own, and the poses are perturbed as make_graph perturbs them.

Huber: the sigmas of a case and mode are chosen so that k = 1.345 sits at the median whitened residual of each row
family (with the production sigmas the distance and depth rows never reach k), so every row type has weighted rows
on both sides of k at every size.
"""
import math

import numpy as np

import oracle.oracle as O

MODES = ("points", "rays", "calib")
HUBER_K = 1.345
ROUND = 512          # points per round of a linearisation block: 256 lanes, two points per lane
LANES = 256
PACK_TILE, PACK_TRIP = 4096, 1024   # ba_pack_kernel: points per block, points per trip (4 per lane)
RUN_LEN = 64         # rounds per fp32 run (BA_RUN_LEN)
IU = np.triu_indices(7)
DIAG = np.flatnonzero(IU[0] == IU[1])
DEFAULT_THRESH = dict(C_thresh=0.0, Q_thresh=1.5, pixel_border=-10, z_eps=1e-6)
DEFAULT_SIGMA = {"points": (0.05, 0.0), "rays": (0.003, 10.0), "calib": (1.0, 10.0)}
NFUSE = (1, 3, 2)    # fusion counts of the zero-copy form, by pose rank


def _spec(H, W, seed, chunk_points=None, chunks=1, n_kf=3, modes=MODES, cond=None, ids=None, zero=False, anchor=None,
          step=0.15, twist=2.0):
    # tails: the case is named for the regions of regions(). Not with a pixel border of 2: the last image rows, which
    # every tail lies in, are then outside the border and never carry weight
    return dict(tails=cond not in ("calib", "tum") and not zero, H=H, W=W, seed=seed, chunk_points=chunk_points, chunks=chunks, n_kf=n_kf, modes=modes, cond=cond,
                ids=ids, zero=zero, anchor=H * W - 1 if anchor is None else anchor, step=step,
                twist=0.0 if H == 1 else twist)


# name -> spec. chunk_points: the M3S_BA_CHUNK_POINTS the case runs under (None: default chunking); chunks: the chunk
# count that gives (asserted on the device from m3s_ba_plan_info). anchor: the pixel the cameras move along the ray of
# (see _graph; default the last one); step, twist: metres and degrees from one camera to the next.
SPECS = {
    # shapes, default thresholds
    "n7": _spec(1, 7, 1),
    "n15": _spec(3, 5, 1),
    "n256": _spec(16, 16, 1, anchor=0),
    "n257": _spec(1, 257, 1, step=0.01),
    "n511": _spec(7, 73, 1),
    "n512": _spec(16, 32, 1),
    "n513": _spec(19, 27, 1),
    "n1300c5": _spec(26, 50, 1, chunk_points=300, chunks=5, anchor=4),
    "n1300c6": _spec(26, 50, 1, chunk_points=256, chunks=6),
    "n4100": _spec(41, 100, 1, chunks=2),
    "n5123": _spec(47, 109, 1, chunks=2),
    "n33000": _spec(150, 220, 1, chunk_points=40000, chunks=1, n_kf=2, modes=("rays", "calib")),
    # thresholds
    "C513": _spec(19, 27, 2, cond="C"),
    "C1300c5": _spec(26, 50, 2, chunk_points=300, chunks=5, cond="C", anchor=4),
    "calib4100": _spec(41, 100, 2, chunks=2, modes=("calib",), cond="calib"),
    "tum4100": _spec(41, 100, 3, chunks=2, modes=("calib",), cond="tum"),
    # keyframe ids that are not ranks, in an order other than their order of appearance
    "ids513": _spec(19, 27, 4, ids=(9, 2, 5)),
    # two identical keyframes, every pixel matched to itself
    "zero513": _spec(19, 27, 5, n_kf=2, modes=("points", "rays"), zero=True),
}
SHAPE_CASES = [n for n in SPECS if n.startswith("n")]
THRESH_CASES = ["C513", "C1300c5", "calib4100", "tum4100"]
BIT_CASES = ["C513", "C1300c5"]


def case_modes(names=None):
    return [(n, m) for n in (names or SPECS) for m in SPECS[n]["modes"]]


# ------------------------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------------------------
def _quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate((a * math.sin(angle / 2), [math.cos(angle / 2)]))


def _raycast_box(origin, dirs, half=3.0):
    """Distance along unit dirs (N,3) from origin to the inside wall of [-half, half]^3."""
    t = np.full(dirs.shape[0], np.inf)
    for a in range(3):
        d = np.where(np.abs(dirs[:, a]) < 1e-9, 1e-9, dirs[:, a])
        for wall in (-half, half):
            ta = (wall - origin[a]) / d
            t = np.where(ta > 0, np.minimum(t, ta), t)
    return t


def tum_like(H, W):
    """TUM freiburg1 calibration (640x480) scaled per axis: fx != fy, a principal point off the image centre."""
    sx, sy = 640.0 / W, 480.0 / H
    return np.array([[517.3 / sx, 0.0, 318.6 / sx], [0.0, 516.5 / sy, 255.3 / sy], [0.0, 0.0, 1.0]], np.float32)


def centred(H, W):
    f = 0.8 * W
    return np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]], np.float32)


_SCALES = (2.0, 0.85, 1.2)                                   # the keyframes' own scales (2.0: an exact inverse)
_MOVE = np.concatenate(([1.5, -0.7, 0.9], _quat((0.3, -0.5, 0.8), math.radians(40.0)), [1.3]))


def _project(K, X):
    with np.errstate(divide="ignore", invalid="ignore"):
        return K[0, 0] * X[:, 0] / X[:, 2] + K[0, 2], K[1, 1] * X[:, 1] / X[:, 2] + K[1, 2]


def _graph(spec, K, rng, force):
    """Poses (ground truth and perturbed), pointmaps in each keyframe's own scale, and the directed edges' matches.

    The cameras stand on the ray of the anchor pixel, ``step`` apart, each turned by ``twist`` about that ray against
    the one before: the anchor pixel maps to itself between any two of them and the flow grows with the distance from
    it, so the points next to the anchor (the last point, a chunk's tail) stay in view in both directions of an edge,
    which no sideways motion allows."""
    H, W, n_kf = spec["H"], spec["W"], spec["n_kf"]
    N = H * W
    K64 = K.astype(np.float64)
    v, u = np.divmod(np.arange(N), W)
    rays = np.stack(((u - K64[0, 2]) / K64[0, 0], (v - K64[1, 2]) / K64[1, 1], np.ones(N)), -1)
    p0, q0 = np.array([0.3, -0.2, -0.5]), _quat((0.05, 1.0, 0.02), 0.7)
    axis = O._qrot(q0, rays[spec["anchor"]][None])[0]
    axis /= np.linalg.norm(axis)
    T_gt, Xs = [], []
    for k in range(n_kf):
        n = 0 if spec["zero"] else k
        s = _SCALES[0] if spec["zero"] else _SCALES[k]
        t = p0 + n * spec["step"] * axis
        q = O._qmul(_quat(axis, math.radians(n * spec["twist"])), q0)
        T = np.concatenate((t, q / np.linalg.norm(q), [s]))
        dirs = O._qrot(T[3:7], rays)
        dist = _raycast_box(t, dirs / np.linalg.norm(dirs, axis=-1, keepdims=True))
        Xs.append(rays * (dist / np.linalg.norm(rays, axis=-1))[:, None] / s)    # metric camera points / own scale
        T_gt.append(O.sim3_mul(_MOVE, T))
    T_gt, Xs = np.stack(T_gt), np.stack(Xs)
    if spec["zero"]:
        # the two identical poses' relative pose must be the identity exactly, in any precision and order of the
        # quaternion product: a rotation about one coordinate axis (every cross term is an exact zero) and a scale
        # with an exact inverse
        T_gt[:] = np.concatenate(([1.5, -0.7, 0.9], _quat((0.0, 1.0, 0.0), math.radians(40.0)), [2.0]))
    T0 = T_gt.copy()
    for k in range(1, n_kf):
        if spec["zero"]:
            break
        xi = np.concatenate((0.02 * rng.standard_normal(3), math.radians(1.0) * rng.standard_normal(3),
                             [0.01 * rng.standard_normal()]))
        T0[k] = O.sim3_retr(T_gt[k], xi)
    pairs = [(k, k + 1) for k in range(n_kf - 1)]
    pairs = pairs + [(j, i) for i, j in pairs]
    E = len(pairs)
    idx, valid = np.zeros((E, N), np.int64), np.zeros((E, N), bool)
    for e, (i, j) in enumerate(pairs):      # for each pixel of j its pixel in i
        if spec["zero"]:
            idx[e], valid[e] = np.arange(N), True
            continue
        Xi = O.sim3_act(O.sim3_mul(O.sim3_inv(T_gt[i]), T_gt[j]), Xs[j])
        pu, pv = _project(K64, Xi)
        inb = (Xi[:, 2] > 0.1) & (pu >= -0.49) & (pu <= W - 0.51) & (pv >= -0.49) & (pv <= H - 0.51)
        lin = np.clip(np.rint(pu), 0, W - 1).astype(np.int64) + W * np.clip(np.rint(pv), 0, H - 1).astype(np.int64)
        out = rng.random(N) < 0.05
        keep = rng.random(N) < 0.95
        rnd = rng.integers(0, N, N)
        out[force], keep[force] = False, True
        idx[e] = np.where(out, rnd, lin)
        valid[e] = inb & keep
    Q = 1.0 + rng.exponential(4.0, (E, N))
    Q[:, force] += 1.0
    return T_gt, T0, Xs, pairs, idx, valid, Q


def _plant(rng, pool, frac):
    pool = np.asarray(pool)
    return rng.permutation(pool)[: max(1, int(round(frac * len(pool))))]


_CASES = {}


def build(name):
    """The case ``name``: a dict of float32 / int64 numpy arrays, built once and never modified.

    Twc (Kp,8), X (Kp,N,3) the keyframes' pointmaps (on their pixel rays), Cs (Kp,N) average confidences, ii / jj (E,)
    keyframe ids, rank_i / rank_j their pose ranks, idx / valid / Q (E,N), K, H, W, N, thresh (the thresholds), sigma
    (mode -> (sigma_a, sigma_b)), chunk_points, chunks."""
    if name in _CASES:
        return _CASES[name]
    spec = SPECS[name]
    rng = np.random.default_rng(1000 + spec["seed"] + 7919 * spec["H"] * spec["W"])
    H, W, n_kf = spec["H"], spec["W"], spec["n_kf"]
    N = H * W
    K = tum_like(H, W) if spec["cond"] == "tum" else centred(H, W)
    # the points a region of at most four points consists of get good matches (valid, no outlier, Q >= 2): the case is
    # named for exactly them
    small = [m for m in regions(dict(N=N, chunks=spec["chunks"])).values() if m.sum() <= 4]
    force = np.flatnonzero(np.logical_or.reduce(small)) if small else np.zeros(0, np.int64)
    T_gt, T0, Xs, pairs, idx, valid, Q = _graph(spec, K, rng, force)
    thresh = dict(DEFAULT_THRESH)
    Cs = 1.0 + rng.exponential(4.0, (n_kf, N))
    planted = {}
    if spec["cond"] == "C":
        # averages: unplanted >= 0.505, a class at exactly 0.6 (zero-copy: sum 1.2 with count 2 in keyframe 2), planted
        # 0.3 (0.4 in keyframe 1: sum 1.2 with count 3). Planted in the source keyframe at matched pixels and in the
        # target keyframe, on disjoint point sets; the forced points stay unplanted.
        thresh["C_thresh"] = 0.5
        Cs = 0.505 + 0.1 * rng.exponential(4.0, (n_kf, N))
        Cs[rng.random((n_kf, N)) < 0.1] = 0.6
        free = np.ones((n_kf, N), bool)
        free[:, force] = False
        for e, (i, j) in enumerate(pairs):
            free[i, idx[e][force]] = False
        low = {0: 0.3, 1: 0.4, 2: 0.3}
        src = np.zeros((n_kf, N), bool)
        for e, (i, j) in enumerate(pairs):          # source side: pixels of keyframe i that valid points match
            hit = np.unique(idx[e][valid[e]])
            hit = hit[free[i, hit] & ~src[i, hit]]
            src[i, _plant(rng, hit, 0.05)] = True
        tgt = np.zeros((n_kf, N), bool)
        for k in range(n_kf):                        # target side: other points of the keyframe
            tgt[k, _plant(rng, np.flatnonzero(free[k] & ~src[k]), 0.07)] = True
        for k in range(n_kf):
            Cs[k, src[k] | tgt[k]] = low[k]
        planted = {"c_src": src, "c_tgt": tgt}
    if spec["cond"] in ("calib", "tum"):
        thresh["pixel_border"] = 2
    if spec["cond"] == "calib":
        # depths of 0, below 0 and just below z_eps: as X_i (the gathered source point) they fail z_i > z_eps, as X_j
        # (the streamed target point) they land at or behind camera i
        free = np.ones((n_kf, N), bool)
        free[:, force] = False
        for e, (i, j) in enumerate(pairs):
            free[i, idx[e][force]] = False
        dep = np.zeros((n_kf, N), bool)
        for k in range(n_kf):
            pick = _plant(rng, np.flatnonzero(free[k]), 0.06)
            third = len(pick) // 3
            Xs[k, pick[:third], 2] = 0.0
            Xs[k, pick[third:2 * third], 2] = -0.7
            Xs[k, pick[2 * third:], 2] = 0.9 * thresh["z_eps"]
            dep[k, pick] = True
        planted = {"depth": dep}
    Q = np.where(np.abs(Q - thresh["Q_thresh"]) < 0.01 * thresh["Q_thresh"], 1.6, Q)
    ids = np.arange(n_kf) if spec["ids"] is None else np.array(spec["ids"])
    order = np.argsort(ids)                    # pose rank r holds the keyframe with the r-th smallest id
    ii = np.array([ids[i] for i, j in pairs], np.int64)
    jj = np.array([ids[j] for i, j in pairs], np.int64)
    uniq = ids[order]
    c = dict(name=name, spec=spec, H=H, W=W, N=N, K=K, E=len(pairs), Kp=n_kf,
             Twc=T0[order].astype(np.float32), X=Xs[order].astype(np.float32), Cs=Cs[order].astype(np.float32),
             ii=ii, jj=jj, rank_i=np.searchsorted(uniq, ii), rank_j=np.searchsorted(uniq, jj), idx=idx, valid=valid,
             Q=Q.astype(np.float32), thresh=thresh, chunk_points=spec["chunk_points"], chunks=spec["chunks"],
             planted={k: v[order] for k, v in planted.items()}, sigma={})
    # decisions of the calib rows that a rounding could flip are taken out of the case: a projection within 0.25 px of
    # a border line, a target depth within reach of z_eps
    if "calib" in spec["modes"] and not spec["zero"]:
        t = point_table(c, "calib", sigma=(1.0, 1.0))
        b = thresh["pixel_border"]
        near = np.zeros_like(c["valid"])
        for val, lines in ((t["u"], (b, W - 1 - b)), (t["v"], (b, H - 1 - b))):
            for line in lines:
                near |= np.abs(val - line) < 0.25
        near |= (t["Yz"] > -1e-3) & (t["Yz"] < 0.05)
        c["valid"] = c["valid"] & ~near
    for mode in spec["modes"]:
        c["sigma"][mode] = DEFAULT_SIGMA[mode]
        if spec["zero"]:
            continue
        t = point_table(c, mode, sigma=(1.0, 1.0))
        sig = []
        for rows in _FAMILIES[mode]:
            r = np.abs(t["r"][..., rows][t["weighted"]])
            sig.append(float(np.float32(float(f"{np.median(r) / HUBER_K:.2g}"))) if r.size else 1.0)
        c["sigma"][mode] = (sig[0], sig[1] if len(sig) > 1 else 0.0)
    _CASES[name] = c
    return c


_FAMILIES = {"points": ([0, 1, 2],), "rays": ([0, 1, 2], [3]), "calib": ([0, 1], [2])}   # rows by sigma


def mode_X(c, mode):
    """The stacked points the mode runs on: calib expects them constrained to their pixel rays."""
    return O.backproject_constrain(c["X"], c["K"], (c["H"], c["W"])) if mode == "calib" else c["X"]


def params(c, mode, sigma=None):
    sa, sb = sigma or c["sigma"][mode]
    t = c["thresh"]
    return O.ba_params(mode, sa, sb, t["C_thresh"], t["Q_thresh"], K=c["K"], height=c["H"], width=c["W"],
                       pixel_border=t["pixel_border"], z_eps=t["z_eps"])


def local_opt(c, mode, base):
    """A copy of config["local_opt"] carrying the case's thresholds and sigmas."""
    cfg = dict(base)
    t = c["thresh"]
    cfg.update(C_conf=t["C_thresh"], Q_conf=t["Q_thresh"], pixel_border=t["pixel_border"], depth_eps=t["z_eps"])
    sa, sb = c["sigma"][mode]
    cfg.update({"points": dict(sigma_point=sa), "rays": dict(sigma_ray=sa, sigma_dist=sb),
                "calib": dict(sigma_pixel=sa, sigma_depth=sb)}[mode])
    return cfg


# ------------------------------------------------------------------------------------------------------------------
# fp64 per-point table (numpy): which points carry weight, their whitened residuals, which test rejects which point
# ------------------------------------------------------------------------------------------------------------------
def point_table(c, mode, sigma=None, valid=None):
    """Per edge and point, in fp64 from the case's fp32 inputs: weighted (E,N) bool, r (E,N,rows) whitened residuals,
    tests (name -> (E,N) bool, True = the point passes that test), and for calib u, v, Yz."""
    sa, sb = sigma or c["sigma"][mode]
    X = mode_X(c, mode).astype(np.float64)
    T = c["Twc"].astype(np.float64)
    Cs = c["Cs"].astype(np.float64)
    th = c["thresh"]
    valid = c["valid"] if valid is None else valid
    E, N = c["E"], c["N"]
    nrow = 4 if mode == "rays" else 3
    out = dict(weighted=np.zeros((E, N), bool), r=np.zeros((E, N, nrow)), tests={}, u=np.zeros((E, N)),
               v=np.zeros((E, N)), Yz=np.zeros((E, N)))
    tests = {k: np.ones((E, N), bool) for k in ("match", "Q", "c_i", "c_j", "border", "z_i", "z_j")}
    for e in range(E):
        i, j = c["rank_i"][e], c["rank_j"][e]
        Y = O.sim3_act(O.sim3_mul(O.sim3_inv(T[i]), T[j]), X[j])
        ind = np.where(valid[e], c["idx"][e], 0)
        Xi = X[i][ind]
        q = c["Q"][e].astype(np.float64)
        tests["match"][e] = valid[e]
        tests["Q"][e] = q > np.float32(th["Q_thresh"])
        tests["c_i"][e] = Cs[i][ind] > np.float32(th["C_thresh"])
        tests["c_j"][e] = Cs[j] > np.float32(th["C_thresh"])
        sq = np.sqrt(q)
        with np.errstate(divide="ignore", invalid="ignore"):
            if mode == "points":
                r = (sq / sa)[:, None] * (Y - Xi)
            elif mode == "rays":
                ni, nj = np.linalg.norm(Xi, axis=-1), np.linalg.norm(Y, axis=-1)
                r = np.concatenate(((sq / sa)[:, None] * (Y / nj[:, None] - Xi / ni[:, None]),
                                    ((sq / sb) * (nj - ni))[:, None]), -1)
            else:
                K = c["K"].astype(np.float64)
                zi_ok, zj_ok = Xi[:, 2] > np.float32(th["z_eps"]), Y[:, 2] > np.float32(th["z_eps"])
                vz = zi_ok & zj_ok
                zinv = np.where(vz, 1.0 / np.where(vz, Y[:, 2], 1.0), 0.0)
                pu, pv = K[0, 0] * (Y[:, 0] * zinv) + K[0, 2], K[1, 1] * (Y[:, 1] * zinv) + K[1, 2]
                b = th["pixel_border"]
                tests["border"][e] = (pu > b) & (pu < c["W"] - 1 - b) & (pv > b) & (pv < c["H"] - 1 - b)
                tests["z_i"][e], tests["z_j"][e] = zi_ok, zj_ok
                lz = np.where(vz, np.log(np.where(vz, Y[:, 2], 1.0)) - np.log(np.where(vz, Xi[:, 2], 1.0)), 0.0)
                r = np.stack(((sq / sa) * (pu - ind % c["W"]), (sq / sa) * (pv - ind // c["W"]), (sq / sb) * lz), -1)
                # the projection itself (not zeroed where z fails), for the margins of build()
                out["u"][e], out["v"][e] = _project(K, Y)
                out["Yz"][e] = Y[:, 2]
        out["r"][e] = r
    out["tests"] = tests
    out["weighted"] = np.logical_and.reduce(list(tests.values()))
    return out


def only_fails(t, name):
    """Points that the test ``name`` alone rejects: removing its threshold would give them weight."""
    others = [v for k, v in t["tests"].items() if k != name]
    return np.logical_and.reduce(others) & ~t["tests"][name]


def chi2_numpy(t):
    """chi2 of the table: sum over the weighted rows of huber(r) r^2."""
    ra = np.abs(t["r"])
    w = np.where(ra < HUBER_K, 1.0, HUBER_K / np.maximum(ra, 1e-300))
    return np.where(t["weighted"][..., None], w * t["r"] ** 2, 0.0).sum((1, 2))


# ------------------------------------------------------------------------------------------------------------------
# truth, fp32 restatement, metric
# ------------------------------------------------------------------------------------------------------------------
_TRUTH, _REF = {}, {}


def _args(c, mode, valid=None):
    return (mode, c["Twc"], mode_X(c, mode), c["Cs"], c["rank_i"], c["rank_j"], c["idx"],
            c["valid"] if valid is None else valid, c["Q"], params(c, mode))


def truth_blocks(c, mode):
    """(Hs (4,E,7,7), gs (2,E,7), chi2 (E,)) of the fp64 build, reference layout."""
    return O.ba_linearize_chi2_f64(*_args(c, mode))


def truth(c, mode, valid=None):
    """(row64 (E,36) in the device's layout, chi2_64 (E,)) of the fp64 build of the oracle."""
    key = (c["name"], mode)
    if valid is None and key in _TRUTH:
        return _TRUTH[key]
    Hs, gs, chi2 = O.ba_linearize_chi2_f64(*_args(c, mode, valid))
    res = (O.edge_row_from_blocks(Hs, gs), chi2)
    if valid is None:
        _TRUTH[key] = res
    return res


def refs32(c, mode):
    """The fp32 restatement's rows in its two orders: per-point fp32 products summed in fp64, and the reference's own
    order (256 float accumulators and the float block reduction)."""
    rows = []
    for order in (0, 1):
        O.set_ref_order(order)
        try:
            Hs, gs = O.ba_linearize(*_args(c, mode))
        finally:
            O.set_ref_order(0)
        rows.append(O.edge_row_from_blocks(Hs, gs))
    return rows


def rho(row, t):
    """Per edge max(rho_M, rho_g) of the rows ``row`` (E,>=35) against the truth t = (row64, chi2_64):
    rho_M = max |M - M64|_ab / sqrt(M64_aa M64_bb), rho_g = max |g - g64|_a / sqrt(M64_aa chi2_64). Where a denominator
    is 0 (an edge without a weighted point, a zero diagonal entry, chi2 = 0) the entry must be exactly 0.0: inf if not."""
    row64, chi2 = t
    d = np.sqrt(row64[:, DIAG])
    den = np.concatenate((d[:, IU[0]] * d[:, IU[1]], d * np.sqrt(chi2)[:, None]), 1)
    err = np.abs(np.asarray(row, np.float64)[:, :35] - row64[:, :35])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(den > 0, err / den, np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isfinite(np.asarray(row, np.float64)[:, :35]), r, np.inf)
    return r.max(1)


def rho_ref(c, mode):
    """The larger rho of the fp32 restatement in its two orders against the truth, over the case's edges."""
    key = (c["name"], mode)
    if key not in _REF:
        t = truth(c, mode)
        _REF[key] = float(max(rho(r, t).max() for r in refs32(c, mode)))
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------------
# regions: the points whose loss or doubling an index mistake of the kernels would cause
# ------------------------------------------------------------------------------------------------------------------
def chunk_ranges(c):
    per = -(-c["N"] // c["chunks"])
    return [(k * per, min(c["N"], (k + 1) * per)) for k in range(c["chunks"])]


def regions(c):
    """name -> (N,) bool. Per chunk: its last round, and the first point of the lane whose second point is the first
    one past the chunk (k_end - 256: ``has1`` off by one doubles it). The second-point halves of all rounds. The last
    pack tile and its last trip. The points after round 64 of a chunk (after the in-loop flush)."""
    N = c["N"]
    k = np.arange(N)
    R = {}
    second, late = np.zeros(N, bool), np.zeros(N, bool)
    for n, (b, e) in enumerate(chunk_ranges(c)):
        last = (e - b - 1) // ROUND
        R[f"chunk{n}.last_round"] = (k >= b + last * ROUND) & (k < e)
        rem = e - b - last * ROUND
        if LANES <= rem < ROUND:
            R[f"chunk{n}.lane_before_missing_second"] = k == e - LANES
        inside = (k >= b) & (k < e)
        second |= inside & ((k - b) % ROUND >= LANES)
        late |= inside & (k - b >= RUN_LEN * ROUND)
    if second.any():
        R["second_points"] = second
    if late.any():
        R["after_round_64"] = late
    if N > PACK_TILE:
        t0 = (N - 1) // PACK_TILE * PACK_TILE
        R["last_pack_tile"] = k >= t0
        R["last_pack_trip"] = k >= t0 + (N - t0 - 1) // PACK_TRIP * PACK_TRIP
    return R


def sensitivity(c, mode, mask):
    """Per edge: the rho, against the unmodified truth, of the truth recomputed with ``valid`` cleared on the edge's
    first weighted point inside ``mask`` (nan where the edge has none)."""
    t = point_table(c, mode)
    valid = c["valid"].copy()
    has = np.zeros(c["E"], bool)
    for e in range(c["E"]):
        hit = np.flatnonzero(t["weighted"][e] & mask)
        if hit.size:
            valid[e, hit[0]] = False
            has[e] = True
    row, _ = truth(c, mode, valid)
    return np.where(has, rho(row, truth(c, mode)), np.nan)
