"""Edge cases of the codebook quantiser (test infrastructure, CPU only: numpy, no device code).

The case tables, the input builder, the fp64 expectation, a numpy restatement of the kernel's arithmetic and the
predicates that say which branch of csrc/retrieval.hip a case reaches, shared by tests/test_quantize_edges_host.py
(which checks on the CPU that every case is separated and reaches its branch) and tests/test_gpu_quantize_edges.py
(which runs ``Codebook.quantize`` on them and compares indices exactly).

``build(seed, C, D, words, k, dup, scale, exact, margin)``: unit-norm Gaussian centroids (``synthetic.retrieval_inputs``)
times ``scale``; ``dup`` = {source row: rows that are bit-copies of it}. Query i is ``c[w] + 0.35 scale u[w] +
0.35 scale g`` for the word w = words[i] the caller names (the recipe of ``synthetic.asmk_sequence``), or ``c[w]``
itself with ``exact``. A query is redrawn until its k + 1 smallest *distinct* fp64 distances are at least
``margin * scale**2`` apart, so a quantiser whose distance error is well below the margin must return exactly the
expected indices. The centroids depend on (seed, C, D, dup, scale) only, so cases of one seed share their codebook.

Expected indices: fp64 l2 over the unique centroids (each group of bit-identical rows represented by its lowest
row), expanded to all rows so that duplicates tie exactly (a BLAS product of the full matrix need not give bit-equal
columns), the k smallest with ties to the lower row.

Layout restated from csrc/retrieval.hip: blocks of 256 codebook rows; inside a block, row r belongs to lane slot
(r // 32, (r % 16) // 4) (wave, 16-lane group; 32 slots of 8 rows); tau of a query is the k-th smallest of the 32 slot
minima; every distance <= tau enters the candidate list of RQ_CAP = 24 entries; a longer list takes the fallback
(exhaustive per-lane insertion and merges). Queries come in groups of 304 (19 tiles of 16). The final merge folds the
block lists beyond 64 * RQ_ML = 256 blocks (C > 65536) into the first list of their lane.
"""
import collections
import functools

import numpy as np

f32 = np.float32
ROWS, QG, QTILE, CAP, NSLOT, MERGE_BLOCKS = 256, 304, 16, 24, 32, 256

Case = collections.namedtuple("Case", "name family c q topk l2 k scale margin words")


def _unit(rng, n, D):
    x = rng.standard_normal((n, D)).astype(f32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x


def centroids(seed, C, D, dup=None, scale=1.0):
    """(c, u): the fp32 centroids (scaled, duplicate rows copied) and the unit word directions of the queries."""
    rng = np.random.default_rng(seed)
    c, u = _unit(rng, C, D), _unit(rng, C, D)
    c = (c * f32(scale)).astype(f32)
    for src, rows in (dup or {}).items():
        c[np.asarray(rows)] = c[src]
    return c, u


def representatives(c):
    """rep[r]: the lowest row whose bits equal row r's."""
    bits = np.ascontiguousarray(c, dtype=f32).view(np.uint32)
    _, first, inv = np.unique(bits, axis=0, return_index=True, return_inverse=True)
    return first[np.asarray(inv).reshape(-1)]


def _expand(c):
    """(rows of the unique centroids (ascending), position of every row's representative among them)."""
    rep = representatives(c)
    uniq = np.unique(rep)
    return uniq, np.searchsorted(uniq, rep)


def l2_unique(c, q, uniq):
    c64, q64 = c[uniq].astype(np.float64), q.astype(np.float64)
    return (np.sum(q64 * q64, axis=1)[:, None] + np.sum(c64 * c64, axis=1)[None, :]) - 2.0 * (q64 @ c64.T)


def topk(l2, k):
    """The k smallest per row in ascending order, ties to the lower index (a stable sort)."""
    return np.argsort(l2, axis=1, kind="stable")[:, :k].astype(np.int64)


def separated(l2u, k, thr):
    """Per query: the k + 1 smallest distances over the unique centroids are pairwise at least thr apart."""
    kk = min(k + 1, l2u.shape[1])
    if kk < 2:
        return np.ones(len(l2u), bool)
    near = np.sort(np.partition(l2u, kk - 1, axis=1)[:, :kk], axis=1)
    return np.diff(near, axis=1).min(axis=1) >= thr


def build(seed, C, D, words, k, dup=None, scale=1.0, exact=False, margin=1e-3):
    """-> (centroids (C, D) fp32, queries (M, D) fp32, expected_topk (M, k) int64, l2 (M, C) fp64)."""
    c, u = centroids(seed, C, D, dup, scale)
    w = np.asarray(words, dtype=np.int64).reshape(-1)
    assert w.size and w.min() >= 0 and w.max() < C and 1 <= k <= min(8, C)
    uniq, pos = _expand(c)
    thr = margin * float(scale) ** 2
    rng = np.random.default_rng([seed, 1])
    a = f32(0.35) * f32(scale)

    def draw(ws):
        return c[ws].copy() if exact else (c[ws] + a * u[ws] + a * _unit(rng, len(ws), D)).astype(f32)

    q = draw(w)
    todo = np.arange(len(w))
    for _ in range(200):
        todo = todo[~separated(l2_unique(c, q[todo], uniq), k, thr)]
        if len(todo) == 0 or exact:
            break
        q[todo] = draw(w[todo])
    assert len(todo) == 0, f"quantize_edge_cases.build: {len(todo)} queries not separated"
    l2 = l2_unique(c, q, uniq)[:, pos]
    return c, q, topk(l2, k), l2


# ---- the kernel's arithmetic in numpy ----
def bf16_rne(x):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32 (bf16_rne_bits)."""
    b = np.ascontiguousarray(x, dtype=f32).view(np.uint32)
    b = b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))
    return (b & np.uint32(0xFFFF0000)).view(f32)


def split(x):
    hi = bf16_rne(x)
    return hi, bf16_rne(x - hi)


def norms_f32(x):
    """|x_r|^2 as rq_prep_kernel sums it: lane l takes columns l + 64 j, four accumulators over full 256-column
    rounds and the first alone over the rest, (s0 + s1) + (s2 + s3), a 64-lane xor butterfly (retrieval.hip is
    built without contraction: the products round before they are added)."""
    R, D = x.shape
    n = -(-D // 256)
    sq = np.zeros((R, n * 256), f32)
    sq[:, :D] = x * x
    sq = sq.reshape(R, n, 4, 64)
    lane = np.arange(64)
    s = np.zeros((R, 4, 64), f32)
    for i in range(n):
        full = (256 * i + lane + 192 < D)[None, :]
        for j in range(4):
            s[:, j] += np.where(full, sq[:, i, j], f32(0))
            s[:, 0] += np.where(full, f32(0), sq[:, i, j])
    t = (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])
    for off in (32, 16, 8, 4, 2, 1):
        t = t + t[:, lane ^ off]
    return t[:, 0].copy()


def emulate(c, q):
    """(M, C) fp32 distances as rq_gemm_topk_kernel forms them: per 32-column step the products c_hi q_hi, c_hi q_lo,
    c_lo q_hi accumulated in fp32 (each product of two bf16 is exact in fp32; the order of the 32 additions inside a
    step is numpy's, not the matrix cores'), then (|q|^2 + |c|^2) - 2 acc with the fp32 norms. Computed over the
    unique centroids and expanded: bit-identical rows give bit-identical distances, as on the device, where every
    row runs the same instructions on the same operands."""
    uniq, pos = _expand(c)
    cu = c[uniq]
    D = c.shape[1]
    S = -(-D // 32)
    cp, qp = np.zeros((len(cu), 32 * S), f32), np.zeros((len(q), 32 * S), f32)
    cp[:, :D], qp[:, :D] = cu, q
    (ch, cl), (qh, ql) = split(cp), split(qp)
    acc = np.zeros((len(q), len(cu)), f32)
    for s in range(S):
        k = slice(32 * s, 32 * s + 32)
        acc = acc + qh[:, k] @ ch[:, k].T
        acc = acc + ql[:, k] @ ch[:, k].T
        acc = acc + qh[:, k] @ cl[:, k].T
    d = (norms_f32(q)[:, None] + norms_f32(cu)[None, :]) - f32(2) * acc
    assert d.dtype == f32
    return d[:, pos]


# ---- reach predicates ----
def lane_slot(r):
    """(wave, 16-lane group) holding codebook row r in its block."""
    r = r % ROWS
    return r // 32, (r % 16) // 4


def fallback_by_tail(C, k):
    """The last block has more than RQ_CAP real rows in fewer than k lane slots: tau = +inf, every real row is a
    candidate and the list overflows."""
    n = C % ROWS
    return n > CAP and len({lane_slot(r) for r in range(n)}) < k


def list_lengths(l2, k):
    """(M, nblk) candidate list lengths of the threshold filter, from the fp64 distances: tau = the k-th smallest
    of the 32 slot minima of the block (+inf rows past C), the rows with a finite distance <= tau."""
    M, C = l2.shape
    nblk = -(-C // ROWS)
    x = np.full((M, nblk * ROWS), np.inf)
    x[:, :C] = l2
    # local row = 32 wave + 16 r + 4 group + i
    smin = x.reshape(M, nblk, 8, 2, 4, 4).min(axis=(3, 5)).reshape(M, nblk, NSLOT)
    tau = np.sort(smin, axis=2)[:, :, k - 1]
    x = x.reshape(M, nblk, ROWS)
    return ((x <= tau[:, :, None]) & np.isfinite(x)).sum(axis=2)


def fallback_by_ties(case):
    """Per query: more than RQ_CAP tied rows of one block at one of the distances of its expected k nearest."""
    l2, nblk = case.l2, -(-case.l2.shape[1] // ROWS)
    out = np.zeros(len(l2), bool)
    for m in range(len(l2)):
        for v in np.unique(l2[m, case.topk[m]]):
            rows = np.flatnonzero(l2[m] == v)
            out[m] |= len(rows) > CAP and np.bincount(rows // ROWS, minlength=nblk).max() > CAP
    return out


# ---- the case tables ----
def spread(M, C, start=7):
    """M words stepping through the codebook by 53 rows: every block of a small codebook is aimed at."""
    return (start + 53 * np.arange(M)) % C


KSTEPS = [(8, 1), (24, 2), (32, 3), (33, 4), (160, 5), (192, 6), (224, 7), (384, 8), (416, 6)]  # (D, k); C 300, M 40
GROUPS_M = [1, 16, 17, 304, 305, 609]  # C 300, D 64, k 2
TAILS = [(8, 8), (25, 5), (25, 8), (40, 8), (44, 8), (45, 8), (257, 5), (281, 8), (300, 8), (301, 8), (300, 7)]  # (C, k)
TAILS_FALLBACK = {(25, 5), (25, 8), (40, 8), (44, 8), (281, 8), (300, 8)}
TIES_K = [8, 5, 1]
BIG_K = [8, 1]
SCALES = [3.0, 0.01]
PLUMB = [(305, 8), (1, 1), (609, 2), (40, 8)]  # (M, k) on the codebook of the groups family
POW2 = [(160, 5), (416, 6)]  # the ksteps cases run again with both arrays times 2^12 and 2^-12

TIES_DUP = {
    3: [17, 40, 41] + list(range(60, 76)) + [77, 100, 130, 131, 160, 190] + list(range(200, 212)) + [222, 255],
    5: [128, 250] + list(range(256, 286)),
    9: list(range(20, 39)),
}
# positions of the queries aimed at a duplicate group's source row: in both query groups (304 on), and sharing their
# 16-query tiles with ordinary queries
TIES_AT = {3: [0, 5, 100, 303, 304, 309, 329], 5: [1, 17, 200, 305, 320], 9: [2, 33, 250, 306, 321]}
TIES_FIRST = {3: [3, 17, 40, 41, 60, 61, 62, 63], 5: [5, 128, 250, 256, 257, 258, 259, 260]}

BIG_C = 82000
BIG_DUP = {700: [66000, 70000, 81999], 12: [40000, 65536]}

SEED = {"ksteps": 11, "groups": 21, "tails": 31, "ties": 41, "big": 51, "scale": 61, "exact": 71}


def _tails_words(C):
    w = spread(40, C)
    w[:2] = [C - 1, (C - 1) // ROWS * ROWS]  # the last block's last and first row
    return w


def _ties_words():
    w = spread(330, 300)
    for src, at in TIES_AT.items():
        w[at] = src
    return w


def _big_words():
    hi = 65536 + (11 + 409 * np.arange(40)) % (BIG_C - 65536)
    hi[:6] = [65536, 66000, 70000, 81999, 81920, 81999]
    lo = (3 + 2731 * np.arange(24)) % 65536
    lo[:5] = [12, 700, 40000, 0, 65535]
    w = np.concatenate([hi, lo])
    return w[np.random.default_rng(SEED["big"]).permutation(len(w))]


def exact_words(seed, C, D, k, M, margin=1e-3):
    """The first M words of a seeded permutation whose own centroid, taken as the query, is separated."""
    c, _ = centroids(seed, C, D)
    uniq, _ = _expand(c)
    order = np.random.default_rng([seed, 2]).permutation(C)
    ok = separated(l2_unique(c, c[order], uniq), k, margin)
    assert ok.sum() >= M
    return order[ok][:M]


def _specs():
    """name -> (family, build arguments or the name of the case whose build it shares, k of the case): a case with
    a smaller k than its build's takes the same queries and the leading columns of the expectation (separated for
    k + 1 implies separated for less)."""
    s = {}
    for D, k in KSTEPS:
        s[f"ksteps-D{D}-k{k}"] = ("ksteps", dict(seed=SEED["ksteps"], C=300, D=D, words=spread(40, 300), k=k), k)
    for M in GROUPS_M:
        s[f"groups-M{M}"] = ("groups", dict(seed=SEED["groups"], C=300, D=64, words=spread(M, 300), k=2), 2)
    for C, k in TAILS:
        s[f"tails-C{C}-k{k}"] = ("tails", dict(seed=SEED["tails"], C=C, D=32, words=_tails_words(C), k=k), k)
    s["ties-k8"] = ("ties", dict(seed=SEED["ties"], C=300, D=96, words=_ties_words(), k=8, dup=TIES_DUP), 8)
    s["ties-k5"] = ("ties", "ties-k8", 5)
    s["ties-k1"] = ("ties", "ties-k8", 1)
    s["big-k8"] = ("big", dict(seed=SEED["big"], C=BIG_C, D=32, words=_big_words(), k=8, dup=BIG_DUP), 8)
    s["big-k1"] = ("big", "big-k8", 1)
    for sc in SCALES:
        s[f"scale-{sc}"] = ("scale", dict(seed=SEED["scale"], C=300, D=160, words=spread(40, 300), k=5, scale=sc), 5)
    s["exact"] = ("exact", dict(seed=SEED["exact"], C=300, D=96, words=exact_words(SEED["exact"], 300, 96, 3, 64), k=3,
                                exact=True), 3)
    for M, k in PLUMB:
        if (M, k) != (609, 2):  # that one is groups-M609
            s[f"plumb-M{M}-k{k}"] = ("plumb", dict(seed=SEED["groups"], C=300, D=64, words=spread(M, 300, 11), k=k), k)
    assert [n for n in s if n.startswith("ties")] == [f"ties-k{k}" for k in TIES_K]
    assert [n for n in s if n.startswith("big")] == [f"big-k{k}" for k in BIG_K]
    return s


SPECS = _specs()
NAMES = list(SPECS)
FAMILIES = ("ksteps", "groups", "tails", "ties", "big", "scale", "exact", "plumb")


def names(family):
    return [n for n in NAMES if SPECS[n][0] == family]


def plumb_name(M, k):
    return "groups-M609" if (M, k) == (609, 2) else f"plumb-M{M}-k{k}"


@functools.lru_cache(maxsize=None)
def _built(key):
    out = build(**SPECS[key][1])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    family, kw, k = SPECS[name]
    key = name
    if isinstance(kw, str):  # the case shares the build of another (ties, big): same arrays, fewer columns
        key, kw = kw, SPECS[kw][1]
    c, q, top, l2 = _built(key)
    return Case(name, family, c, q, top[:, :k], l2, k, float(kw.get("scale", 1.0)), 1e-3, np.asarray(kw["words"]))
