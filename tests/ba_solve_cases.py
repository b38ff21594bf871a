"""Cases of the BA pose-solve edge suite (numpy only): graphs whose factor *shape* steers csrc/ba_sparse.hip and
csrc/ba_dense.hip into each of their paths, edge-sum tables to solve on them, the LAPACK truth, failure variants and
the reach predicates. tests/test_ba_solve_host.py checks the cases on the CPU, tests/test_gpu_ba_solve_edges.py runs
them on the device. Which case reaches which path, and the measured figures: DESIGN.md, BA, "solve edge shapes".

A case is a directed edge list ii, jj (int64 keyframe ids) and the pose count Kp; the pose of the lowest id is pinned,
as in the product. The solve assembles the 7 (Kp - 1) system from one 36-double row per directed edge:
columns 0..27 the upper triangle of a symmetric 7x7 block M_e (np.triu_indices(7) order), 28..34 a gradient g_e, 35 pad.
"""
import functools

import numpy as np

IU = np.triu_indices(7)
SOLVERS = ("sparse", "dense")


# ---------------------------------------------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------------------------------------------
def _two_way(und):
    a = np.array([e[0] for e in und], np.int64)
    b = np.array([e[1] for e in und], np.int64)
    return np.concatenate((a, b)), np.concatenate((b, a))


def _loops(K, seed):
    """Consecutive edges plus three random earlier keyframes per keyframe from the fifth on (the loop edges of
    m3s.synthetic.make_graph), both directions."""
    rng = np.random.default_rng(seed)
    und = [(k - 1, k) for k in range(1, K)]
    for k in range(4, K):
        for c in sorted(rng.choice(k - 1, 3, replace=False).tolist()):
            if (c, k) not in und:
                und.append((c, k))
    return _two_way(und) + (K,)


# multi9: keyframe ids that are no ranks (pose rank = position among the sorted ids; 3 is pinned), edges in rank
# terms: a chain and two loops in both directions, then the irregular ones
MULTI9_IDS = (3, 5, 8, 11, 17, 22, 25, 31, 40)
_MULTI9_RANK_EDGES = (
    [(a, b) for a, b in ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (2, 6), (1, 8))]
    + [(b, a) for a, b in ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (2, 6), (1, 8))]
    + [(2, 1)]    # a duplicated directed edge
    + [(5, 3)]    # one direction only
    + [(4, 4)]    # a self-loop on a free pose
    + [(0, 4)]    # the pinned pose on the ii side only
    + [(7, 0)]    # the pinned pose on the jj side only
)


def _multi9():
    order = np.random.default_rng(90).permutation(len(_MULTI9_RANK_EDGES))  # listed out of order
    ids = np.array(MULTI9_IDS, np.int64)
    e = np.array(_MULTI9_RANK_EDGES, np.int64)[order]
    return ids[e[:, 0]], ids[e[:, 1]], len(MULTI9_IDS)


_GRAPHS = {
    "k2": lambda: _two_way([(0, 1)]) + (2,),
    "pinstar12": lambda: _two_way([(0, k) for k in range(1, 12)]) + (12,),
    "chain40": lambda: _two_way([(k - 1, k) for k in range(1, 40)]) + (40,),
    "hub72": lambda: _two_way([(0, 1)] + [(1, k) for k in range(2, 72)]) + (72,),
    "clique30": lambda: _two_way([(a, b) for b in range(30) for a in range(b)]) + (30,),
    "dense10": lambda: _loops(10, 10),
    "dense11": lambda: _loops(11, 11),
    "dense56": lambda: _loops(56, 56),
    "dense65": lambda: _loops(65, 65),
    "dense74": lambda: _loops(74, 74),
    "multi9": _multi9,
}
CASES = tuple(_GRAPHS)
FAIL_CASES = ("clique30", "chain40", "dense74")
FAIL_VARIANTS = ("neg_root", "neg_leaf", "nan_block")


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def graph(name):
    """(ii, jj, Kp): directed edges as int64 keyframe ids (read-only) and the pose count."""
    ii, jj, Kp = _GRAPHS[name]()
    return _frozen(ii, jj) + (Kp,)


def ranks(ii, jj):
    """Pose rank of every edge end minus the pinned pose (gn_kernels.cu:161-170: position among the sorted unique
    ids, pin 1): -1 is the pinned pose."""
    u = np.unique(np.concatenate((ii, jj)))
    return np.searchsorted(u, ii) - 1, np.searchsorted(u, jj) - 1


# ---------------------------------------------------------------------------------------------------------------
# edge sums
# ---------------------------------------------------------------------------------------------------------------
def _seed(name):
    return 1000 + CASES.index(name)


def random_table(E, rng):
    """(E, 36): M_e = Q diag(lambda) Q^T, Q a random orthogonal 7x7, lambda uniform in [1, 4]; g_e standard normal."""
    es = np.zeros((E, 36))
    for e in range(E):
        Q, R = np.linalg.qr(rng.standard_normal((7, 7)))
        Q = Q * np.sign(np.diag(R))
        M = (Q * rng.uniform(1.0, 4.0, 7)) @ Q.T
        es[e, :28] = (0.5 * (M + M.T))[IU]
        es[e, 28:35] = rng.standard_normal(7)
    return es


@functools.lru_cache(maxsize=None)
def edge_sums(name, variant=0):
    """The case's (E, 36) table (read-only); variant > 0: another table on the same graph."""
    es = random_table(len(graph(name)[0]), np.random.default_rng(_seed(name) + 100 * variant))
    return _frozen(es)[0]


def twc0(Kp):
    """(Kp, 8) float32: a fixed non-identity Sim(3) (t, unit q, s) per pose."""
    rng = np.random.default_rng(7)
    t = rng.uniform(-2.0, 2.0, (Kp, 3))
    q = rng.standard_normal((Kp, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    s = rng.uniform(0.8, 1.25, (Kp, 1))
    return np.concatenate((t, q, s), 1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# truth
# ---------------------------------------------------------------------------------------------------------------
def block(row):
    """The symmetric 7x7 block of one table row."""
    M = np.zeros((7, 7))
    M[IU] = row[:28]
    return M + np.triu(M, 1).T


def assemble(es, ii, jj):
    """fp64 host assembly of the pose system from the (E,36) edge-sum table (the rule of gn_kernels.cu:71-113 with
    pin 1: H_ii += M, H_ij = H_ji -= M, H_jj += M; g_i -= g, g_j += g; rows of the pinned pose dropped). A self-loop
    takes all four block terms on its one diagonal block, which cancel, as do its two gradient terms; a duplicated
    edge counts twice. Returns H (n, n), g (n), n = 7 (unique ids - 1)."""
    ri, rj = ranks(ii, jj)
    n = (len(np.unique(np.concatenate((ii, jj)))) - 1) * 7
    Hs, g = np.zeros((n, n)), np.zeros(n)
    for e in range(es.shape[0]):
        M = block(es[e])
        gv = es[e, 28:35]
        a, b = ri[e], rj[e]
        if a >= 0:
            Hs[7 * a:7 * a + 7, 7 * a:7 * a + 7] += M
            g[7 * a:7 * a + 7] -= gv
        if b >= 0:
            Hs[7 * b:7 * b + 7, 7 * b:7 * b + 7] += M
            g[7 * b:7 * b + 7] += gv
        if a >= 0 and b >= 0:
            Hs[7 * a:7 * a + 7, 7 * b:7 * b + 7] -= M
            Hs[7 * b:7 * b + 7, 7 * a:7 * a + 7] -= M
    return Hs, g


def host_solve_from_edge_sums(es, ii, jj):
    """fp64 host assembly of the pose system from the (E,36) edge-sum table (the rule of
    gn_kernels.cu:71-113 with pin 1: H_ii += M, H_ij = H_ji -= M, H_jj += M; g_i -= g, g_j += g)
    and dx = -H^-1 g by numpy (LAPACK)."""
    Hs, g = assemble(es, ii, jj)
    return -np.linalg.solve(Hs, g)


@functools.lru_cache(maxsize=None)
def system(name, variant=0):
    """(H, g, dx, cond(H)) of the case's table, read-only."""
    ii, jj, _ = graph(name)
    H, g = assemble(edge_sums(name, variant), ii, jj)
    dx = -np.linalg.solve(H, g)
    return _frozen(H, g, dx) + (float(np.linalg.cond(H)),)


COND_CAP = 1e5


def bound(ref, cond):
    """Elementwise bound on |dx - ref| of a device solve: the rounding of the fp32 output, 2^-24 |ref_i|, plus the
    documented accuracy of the device's pivots (rsqrt_nr / rcp_nr, one Newton step, about 2^-44 relative) carried
    through a system of condition number cond, with a factor 4 for the accumulation over a 7-step pivot block,
    relative to max|ref|. LAPACK's own error, cond 2^-53, is 500 times smaller and has no term."""
    return 2.0 ** -24 * np.abs(ref) + 4.0 * cond * 2.0 ** -44 * np.abs(ref).max()


def error_ratio(dx, ref, cond):
    """The worst |dx - ref| / bound over the elements (<= 1 passes)."""
    return float((np.abs(np.asarray(dx, np.float64).reshape(-1) - ref) / bound(ref, cond)).max())


# ---------------------------------------------------------------------------------------------------------------
# symbolic elimination and reach predicates
# ---------------------------------------------------------------------------------------------------------------
def symbolic(ii, jj, Kp):
    """Plain-Python restatement of the plan's symbolic analysis (csrc/ba_pattern.cpp): minimum-degree elimination of
    the pose graph without the pinned pose, exact degrees, ties to the lowest index. Returns a dict: perm (new column
    -> pose index without the pin), struct (per new column its off-diagonal block rows, ascending), lev (per column),
    nL, nlev, groups {(source level, target column): sources ascending}, and the counts m3s_ba_pattern_stats reports
    as stats = (nL, nlev, groups, sources, source-map entries, pull groups)."""
    ri, rj = ranks(ii, jj)
    nb = Kp - 1
    adj = [set() for _ in range(nb)]
    for a, b in zip(ri.tolist(), rj.tolist()):
        if a >= 0 and b >= 0 and a != b:
            adj[a].add(b)
            adj[b].add(a)
    alive, order, nbrs = set(range(nb)), [], {}
    while alive:
        v = min(alive, key=lambda x: (len(adj[x]), x))
        order.append(v)
        alive.remove(v)
        nv = set(adj[v])
        nbrs[v] = nv
        for a in nv:
            adj[a] |= nv
            adj[a] -= {a, v}
        adj[v] = set()
    pos = {v: k for k, v in enumerate(order)}
    S = [sorted(pos[a] for a in nbrs[order[j]]) for j in range(nb)]
    lev = [0] * nb
    for j in range(nb):
        if S[j]:
            lev[S[j][0]] = max(lev[S[j][0]], lev[j] + 1)
    groups = {}
    for k in range(nb):
        for j in S[k]:
            groups.setdefault((lev[k], j), []).append(k)
    nsrc = sum(len(v) for v in groups.values())
    sidx = sum(len(v) * (len(S[j]) + 1) for (_, j), v in groups.items())
    pulls = sum(1 for (l, j) in groups if l == lev[j] - 1)
    nL, nlev = nb + sum(len(s) for s in S), (max(lev) + 1 if nb else 0)
    return {"perm": order, "struct": S, "lev": lev, "nL": nL, "nlev": nlev, "groups": groups,
            "stats": (nL, nlev, len(groups), nsrc, sidx, pulls)}


@functools.lru_cache(maxsize=None)
def reach(name):
    """What the plan of the case must report and the factor shapes its kernels then meet: nL, nlev, dense (the flag
    under each M3S_BA_SOLVER), stats (m3s_ba_pattern_stats), noff (the set of off-diagonal block counts of the factor
    columns: the row regime of sp_column_task and the block count of sp_back_column), max_group (the most sources of
    one update group: flow_wait_task loops in chunks of 63), single_levels (levels of one column), n = 7 (Kp - 1)."""
    ii, jj, Kp = graph(name)
    s = symbolic(ii, jj, Kp)
    width = [0] * s["nlev"]
    for l in s["lev"]:
        width[l] += 1
    return {"nL": s["nL"], "nlev": s["nlev"], "dense": {"sparse": 0, "dense": 1}, "stats": s["stats"],
            "noff": frozenset(len(c) for c in s["struct"]),
            "max_group": max((len(v) for v in s["groups"].values()), default=0),
            "single_levels": sum(1 for w in width if w == 1), "n": 7 * (Kp - 1), "nb": Kp - 1}


def rows_of(noff):
    """Rows of a factor column with noff off-diagonal blocks: 7 per block, the diagonal block included, and the rhs."""
    return 7 * (noff + 1) + 1


# ---------------------------------------------------------------------------------------------------------------
# failure variants: a modified copy of a case's table on which the factorisation must fail
# ---------------------------------------------------------------------------------------------------------------
def permuted(H, perm):
    """H in the plan's elimination order (7x7 blocks by perm)."""
    p = (7 * np.asarray(perm)[:, None] + np.arange(7)[None, :]).reshape(-1)
    return H[np.ix_(p, p)]


def _perm(name):
    ii, jj, Kp = graph(name)
    return symbolic(ii, jj, Kp)["perm"]


def _edge_at(name, pose):
    """An edge with the free pose `pose` (index without the pin) on one end and another pose on the other, the pinned
    pose preferred (its M_e then enters one diagonal block only): (edge, other end or -1)."""
    ii, jj, _ = graph(name)
    ri, rj = ranks(ii, jj)
    best = None
    for e, (a, b) in enumerate(zip(ri.tolist(), rj.tolist())):
        if a == b or pose not in (a, b):
            continue
        o = b if a == pose else a
        if o < 0:
            return e, -1
        best = best if best is not None else (e, o)
    return best


def _first_bad_pivot(Hp):
    """Index of the first non-positive (or NaN) pivot of a right-looking Cholesky of Hp, or -1."""
    A = np.array(Hp, copy=True)
    for k in range(A.shape[0]):
        d = A[k, k]
        if not d > 0.0:
            return k
        c = A[k + 1:, k] / np.sqrt(d)
        A[k + 1:, k + 1:] -= np.outer(c, c)
    return -1


def _downdate(name, pose, k_fail):
    """Subtract c from entry (6, 6) of one edge's M_e at `pose` so that pivot k_fail of the permuted system, the last
    scalar pivot of that pose's column, turns negative while every pivot before it stays positive. The change is
    H - c v v^T with v = e_(pose,6) - e_(other,6) (the other term absent for the pinned pose): the leading block of
    order k has determinant det(H_k) (1 - c v_k^T H_k^-1 v_k), so pivot k_fail changes sign at
    c* = 1 / (v^T H_(k_fail+1)^-1 v) and the block before it, where it holds a part of v, later, at c1; c sits halfway
    between (at 1.5 c* when that is nearer)."""
    ii, jj, _ = graph(name)
    es = np.array(edge_sums(name), copy=True)
    H = system(name)[0]
    perm = _perm(name)
    e, other = _edge_at(name, pose)
    v = np.zeros(H.shape[0])
    v[7 * pose + 6] = 1.0
    if other >= 0:
        v[7 * other + 6] = -1.0
    p = (7 * np.asarray(perm)[:, None] + np.arange(7)[None, :]).reshape(-1)
    Hp, vp = H[np.ix_(p, p)], v[p]
    k1 = k_fail + 1
    c_star = 1.0 / (vp[:k1] @ np.linalg.solve(Hp[:k1, :k1], vp[:k1]))
    c = 1.5 * c_star
    if np.any(vp[:k_fail] != 0.0):
        c1 = 1.0 / (vp[:k_fail] @ np.linalg.solve(Hp[:k_fail, :k_fail], vp[:k_fail]))
        c = min(c, 0.5 * (c_star + c1))
    es[e, 27] -= c  # entry (6, 6), the last of the upper triangle
    Hn = permuted(assemble(es, ii, jj)[0], perm)
    assert _first_bad_pivot(Hn) == k_fail, (name, pose, k_fail, _first_bad_pivot(Hn))
    return es


def fail_pivot(name, variant):
    """The scalar pivot of the permuted system at which neg_root / neg_leaf fail."""
    nb = graph(name)[2] - 1
    return 7 * nb - 1 if variant == "neg_root" else 6


@functools.lru_cache(maxsize=None)
def failing_table(name, variant):
    """neg_root: exactly the last pivot of the permuted system non-positive, every leading principal minor before it
    positive (the failure happens at the root column only). neg_leaf: the same at pivot 6, the last of the first
    column, a level-0 column. nan_block: NaN in entry (2, 4) of the M_e of one edge between two free poses."""
    perm = _perm(name)
    if variant == "neg_root":
        es = _downdate(name, perm[-1], fail_pivot(name, variant))
    elif variant == "neg_leaf":
        es = _downdate(name, perm[0], fail_pivot(name, variant))
    else:
        ii, jj, _ = graph(name)
        ri, rj = ranks(ii, jj)
        e = next(e for e in range(len(ii)) if ri[e] >= 0 and rj[e] >= 0 and ri[e] != rj[e])
        es = np.array(edge_sums(name), copy=True)
        es[e, IU[0].tolist().index(2) + 2] = np.nan  # row 2 of the upper triangle starts at (2, 2): + 2 -> (2, 4)
    return _frozen(es)[0]


# ---------------------------------------------------------------------------------------------------------------
# retraction
# ---------------------------------------------------------------------------------------------------------------
def ulp32(x):
    """The spacing of fp32 at |x| (elementwise)."""
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)
