"""Edge cases of the ASMK database kernels (test infrastructure, CPU only: numpy, no device code).

The named, seeded cases, their builders and the predicates that say which branch of csrc/asmk.hip a case reaches,
shared by tests/test_asmk_edges_host.py (which checks on the CPU that every case reaches its branch and that the
expectation is pinned where the case needs it to be) and tests/test_gpu_asmk_edges.py (which runs the cases through
``m3s.retrieval.AsmkDatabase``). Every expected value comes from tests/asmk_ref.py (``aggregate``, ``ForwardDb``,
``sim_table``, ``rank``); every array handed out is read-only.

Four families:

A ``agg(name)``     hand-made word ids for ``aggregate`` (no quantiser): the sort's padded sizes P, the scan's wave
                    carries, the repeat filter, key bit 31, the add order of a word's rows, every code-word layout.
B ``search(name)``  explicit (codes, words, count) images for ``add`` and one query for ``search``: scores that are
                    exact in any summation order, the append's stride loop, an image without entries.
C ``topk(name)``    300 one-entry images on one word with chosen Hamming weights and a one-feature query, so that
                    every score is one table value: ties, zeros, a maximum beyond index 256, NaN scores.
D ``update(name)``  the fused update at the 4096-key limit, word ids from the fp64 distances.

Layout restated from csrc/asmk.hip. Sort: one workgroup of 1024 threads, keys ``word << 12 | row`` padded to P (64
doubled until it holds M * use_cols); a thread makes P / 2048 passes per bitonic step; the scan gives thread t the
sorted positions 4 t .. 4 t + 3, so a wave holds 256 positions; a key equal to its predecessor is dropped.
Aggregate: one workgroup of 256 threads per word, dims in passes of 256, a wave's ballot = two code words. Score:
uint4 popcounts when W = D / 32 is a multiple of 4, else word by word. Top-k: 256 threads stride over the images.
Append: at most 256 blocks of 256 threads, so more than 65536 code words take the stride loop.
"""
import collections
import functools

import numpy as np

import asmk_ref as R

f32 = np.float32
MAX_KEYS, SORT_THREADS, APPEND_THREADS, TOPK_THREADS = 4096, 1024, 256 * 256, 256

AggCase = collections.namedtuple("AggCase", "name family c des ids use_cols codes words")
SearchCase = collections.namedtuple("SearchCase", "name family c alpha thr images q_codes q_words scores ref")
TopkCase = collections.namedtuple("TopkCase", "name family c alpha thr w0 h codes feat q_code scores runs")
UpdateCase = collections.namedtuple("UpdateCase", "name family c feats kq kb K min_thresh ids lists scores ref")


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


@functools.lru_cache(maxsize=None)
def centroids(C, D):
    """Unit-norm Gaussian centroids; they depend on (C, D) only, so cases of one shape share their codebook."""
    c = np.random.default_rng([7, C, D]).standard_normal((C, D)).astype(f32)
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    return _freeze(c)


# ---- reach predicates ----
def sort_P(n):
    """The padded size m3s_launch_asmk_sort chooses for n keys."""
    P = 64
    while P < n:
        P <<= 1
    return P


def sort_passes(n):
    """Passes of a thread over the P / 2 pairs of a bitonic step."""
    return -(-(sort_P(n) // 2) // SORT_THREADS)


def scan_waves(n):
    """Waves whose threads hold a key in the scan (four positions per thread, 64 threads per wave)."""
    return -(-n // 256)


def sorted_keys(ids, use_cols):
    ids = np.asarray(ids)[:, :use_cols].astype(np.uint64)
    rows = np.arange(len(ids), dtype=np.uint64)[:, None]
    keys = ((ids << np.uint64(12)) | rows).reshape(-1)
    assert (keys < 2 ** 32).all()
    return np.sort(keys.astype(np.uint32))


def dropped_positions(keys):
    """Sorted positions whose key repeats its predecessor: what the repeat filter drops (keep = 0)."""
    return 1 + np.flatnonzero(keys[1:] == keys[:-1])


def rows_per_slot(cs):
    """Rows of every unique word, in the order of the slots (a row that names the word twice counts once)."""
    ids = cs.ids[:, :cs.use_cols]
    return np.array([int((ids == w).any(axis=1).sum()) for w in cs.words])


def popcount_path(D):
    return "vector" if (D // 32) % 4 == 0 else "scalar"


def append_strides(max_count, D):
    """Does asmk_append_kernel's grid of at most 65536 threads loop over the code words?"""
    return max_count * (D // 32) > APPEND_THREADS


# ---- A. sort and aggregate ----
DIMS = (32, 64, 96, 160, 256, 288)
HIGH_WORDS = (0, 1, 2 ** 19 - 1, 2 ** 19, 2 ** 19 + 1, 2 ** 20 - 2, 2 ** 20 - 1)
ORDER_WORD, ORDER_ROWS = 37, 309


def _agg_case(name, c, des, ids, use_cols=None):
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    des = np.ascontiguousarray(des, dtype=f32)
    use_cols = ids.shape[1] if use_cols is None else use_cols
    codes, words = R.aggregate(des, ids[:, :use_cols], c)
    _freeze(des, ids, codes, words)
    return AggCase(name, "A", c, des, ids, use_cols, codes, words)


def _features(rng, M, D):
    return rng.standard_normal((M, D)).astype(f32)


def _sort_case(name, seed, M, D, C=1024, words=None):
    rng = np.random.default_rng([11, seed])
    ids = rng.integers(0, C, size=(M, 1)) if words is None else np.asarray(words).reshape(M, 1)
    return _agg_case(name, centroids(C, D), _features(rng, M, D), ids)


def _k8_ids():
    rng = np.random.default_rng([11, 8])
    return np.stack([rng.permutation(64)[:8] for _ in range(512)])  # eight distinct words per row


def _dup_ids():
    """Rows 0 .. 246 name word 0 once, rows 247 and 248 eight times: sorted positions 0 .. 246 single keys, 247 .. 254
    row 247 (one kept), 255 row 248's kept key and 256 .. 262 its repeats: a drop at i % 256 == 0 (and i % 4 == 0),
    decided by a key that another wave's thread holds. Further rows repeat a word twice or three times."""
    rng = np.random.default_rng([11, 9])
    M = 300
    ids = np.stack([1 + rng.permutation(63)[:8] for _ in range(M)])  # distinct words 1 .. 63
    ids[np.arange(247), rng.integers(0, 8, size=247)] = 0
    ids[247:249] = 0
    for r in range(249, M, 2):  # 2x
        a, b = rng.permutation(8)[:2]
        ids[r, a] = ids[r, b]
    for r in range(250, M, 6):  # 3x
        a, b, d = rng.permutation(8)[:3]
        ids[r, a] = ids[r, d] = ids[r, b]
    return ids


def _high_case():
    rng = np.random.default_rng([11, 10])
    M, D, C = 4096, 32, 2 ** 20
    c = np.zeros((C, D), f32)  # only the used rows are filled
    used = np.array(HIGH_WORDS)
    c[used] = centroids(64, D)[:len(used)]
    _freeze(c)
    ids = used[rng.integers(0, len(used), size=M)]
    ids[:len(used)] = used[::-1]  # every word occurs, the highest on row 0 as well
    ids[4095] = 2 ** 20 - 1
    return _agg_case("high_words", c, _features(rng, M, D), ids.reshape(M, 1))


def order_rows(ids):
    return np.flatnonzero((np.asarray(ids) == ORDER_WORD).any(axis=1))


def _order_case(D):
    """One word with 309 rows whose residuals cancel in exact arithmetic: 150 rows of magnitudes 1e-3, 1 and 1e4 and
    their negatives, shuffled, with three (1e8, 1, -1e8) triples of consecutive rows among them. What is left is
    rounding error, so the signs of the sums depend on the order of the adds. 21 rows of other words lie between."""
    rng = np.random.default_rng([11, 12, D])
    c = centroids(64, D)
    half = 150
    mag = rng.choice(np.array([1e-3, 1, 1e4], f32), size=(half, D))
    sign = rng.choice(np.array([-1, 1], f32), size=(half, D))
    v = (mag * (1 + rng.random((half, D), dtype=f32)) * sign).astype(f32)
    body = np.concatenate([v, -v])[rng.permutation(2 * half)]
    parts, prev = [], 0
    for t in sorted(rng.choice(np.arange(20, 2 * half - 20), 3, replace=False)):
        s = rng.choice(np.array([-1, 1], f32), size=D)
        parts += [body[prev:t], np.stack([f32(1e8) * s, rng.choice(np.array([-1, 1], f32), size=D), f32(-1e8) * s])]
        prev = t
    res = np.concatenate(parts + [body[prev:]]).astype(f32)
    assert len(res) == ORDER_ROWS
    M = ORDER_ROWS + 21
    other = np.sort(rng.choice(np.arange(1, M - 1), 21, replace=False))
    ids = np.full(M, ORDER_WORD)
    ids[other] = rng.integers(0, ORDER_WORD, size=21)
    des = _features(rng, M, D)
    des[ids == ORDER_WORD] = c[ORDER_WORD][None] + res
    return _agg_case(f"order_sensitive_{D}", c, des, ids.reshape(M, 1))


def _dims_case(D):
    rng = np.random.default_rng([11, 13, D])
    ids = np.stack([20 + rng.permutation(12)[:3] for _ in range(24)])  # 12 words, about six rows each
    return _agg_case(f"dims_{D}", centroids(64, D), _features(rng, 24, D), ids)


def _k8_case(name, use_cols):
    rng = np.random.default_rng([11, 8, 1])
    return _agg_case(name, centroids(64, 96), _features(rng, 512, 96), _k8_ids(), use_cols)


def _dup_case():
    rng = np.random.default_rng([11, 9, 1])
    return _agg_case("dup_in_row", centroids(64, 96), _features(rng, 300, 96), _dup_ids())


AGG = {
    "one_key": lambda: _sort_case("one_key", 1, 1, 32),
    "p64_full": lambda: _sort_case("p64_full", 2, 64, 64),
    "p128_first": lambda: _sort_case("p128_first", 3, 65, 64),
    "scan_wave_edge_256": lambda: _sort_case("scan_wave_edge_256", 4, 256, 96),
    "scan_wave_edge_257": lambda: _sort_case("scan_wave_edge_257", 5, 257, 96),
    "p2048_full": lambda: _sort_case("p2048_full", 6, 2048, 32),
    "p4096_first": lambda: _sort_case("p4096_first", 7, 2049, 32),
    "full_distinct": lambda: _sort_case("full_distinct", 8, 4096, 32, C=8192,
                                        words=np.random.default_rng([11, 80]).permutation(8192)[:4096]),
    "full_one_word": lambda: _sort_case("full_one_word", 9, 4096, 32, words=np.full(4096, 777)),
    "k8_full": lambda: _k8_case("k8_full", 8),
    "use_cols_3": lambda: _k8_case("use_cols_3", 3),
    "dup_in_row": _dup_case,
    "high_words": _high_case,
    "order_sensitive_288": lambda: _order_case(288),
    "order_sensitive_1024": lambda: _order_case(1024),
}
AGG.update({f"dims_{D}": functools.partial(_dims_case, D) for D in DIMS})
AGG_NAMES = list(AGG)


@functools.lru_cache(maxsize=None)
def agg(name):
    return AGG[name]()


# ---- B. add and search ----
EXACT_D = (32, 64, 128, 256)
EXACT_SIZES = (1, 4, 16, 64, 256, 1024, 4096)  # powers of four: sqrt(norm) is a power of two


def _codes(rng, n, W):
    return rng.integers(0, 2 ** 32, size=(n, W), dtype=np.uint64).astype(np.uint32)


def _flip_masks(rng, h, D):
    """(len(h), D / 32) uint32 masks with exactly h[i] bits set."""
    bits = np.argsort(rng.random((len(h), D)), axis=1) < np.asarray(h)[:, None]
    return np.packbits(bits, axis=1, bitorder="big").view(">u4").astype(np.uint32)


def _image(rng, C, D, n, q_codes, q_words, h_first=None):
    """n entries on distinct words in shuffled order: about half of them words of the query, with Hamming distances
    drawn from 0 .. D (the first hit at ``h_first``), the others words the query does not hold."""
    nh = -(-n // 2)
    rest = np.setdiff1d(np.arange(C), q_words)
    words = np.concatenate([rng.choice(q_words, nh, replace=False), rng.choice(rest, n - nh, replace=False)])
    codes = _codes(rng, n, D // 32)
    h = rng.integers(0, D + 1, size=nh)
    if h_first is not None:
        h[0] = h_first
    codes[:nh] = q_codes[np.searchsorted(q_words, words[:nh])] ^ _flip_masks(rng, h, D)
    p = rng.permutation(n)
    return np.ascontiguousarray(codes[p]), words[p].astype(np.int32), n


def _search_case(name, C, D, nq, sizes, seed, alpha=3.0, thr=0.0, empty_at=None):
    rng = np.random.default_rng([13, seed])
    c = centroids(C, D)
    q_words = np.sort(rng.choice(C, nq, replace=False)).astype(np.int32)
    q_codes = _codes(rng, nq, D // 32)
    ref = R.ForwardDb(c, 1, 1, alpha, thr)
    images = []
    for i, n in enumerate(sizes):
        if i == empty_at:  # rows that a count of 0 keeps out of the database
            img = (np.full((n, D // 32), 0xdeadbeef, np.uint32), q_words[:n].copy(), 0)
        else:
            img = _image(rng, C, D, n, q_codes, q_words, h_first=i % (D // 2))
        _freeze(img[0], img[1])
        images.append(img)
        ref.add(img[0][:img[2]], img[1][:img[2]])
    scores = ref.search(q_codes, q_words)
    _freeze(q_codes, q_words, scores, ref.codes, ref.words, ref.img_ptr)
    return SearchCase(name, "B", c, alpha, thr, images, q_codes, q_words, scores, ref)


SEARCH = {f"exact_scores_{D}": functools.partial(_search_case, f"exact_scores_{D}", 8192, D, 4096, EXACT_SIZES, D)
          for D in EXACT_D}
SEARCH["big_append"] = lambda: _search_case("big_append", 4096, 1024, 2048, (4096, 5, 300), 1)
SEARCH["empty_image"] = lambda: _search_case("empty_image", 64, 96, 20, (10, 4, 7), 2, empty_at=1)
SEARCH_NAMES = list(SEARCH)


@functools.lru_cache(maxsize=None)
def search(name):
    return SEARCH[name]()


def permuted_scores(cs, seed):
    """The reference scores with every image's entries in another random order."""
    rng = np.random.default_rng([13, 99, seed])
    ref = R.ForwardDb(cs.c, 1, 1, cs.alpha, cs.thr)
    for codes, words, n in cs.images:
        p = rng.permutation(n)
        ref.add(codes[:n][p], words[:n][p])
    return ref.search(cs.q_codes, cs.q_words)


# ---- C. top-k ----
TOPK_N, TOPK_D, TOPK_W0 = 300, 128, 21
TOPK_K = (1, 3, 64)


def topk_weights():
    """Hamming distance of image i to the all-ones query code. Scores fall with h; h = 64 scores 0; h > 64 scores 0
    with the threshold at 0 and NaN with it at -1 and alpha 2.5."""
    i = np.arange(TOPK_N)
    h = np.empty(TOPK_N, np.int64)
    h[:100] = 10  # a run of 100 equal scores
    h[100:150] = 64  # zeros (sim = 0)
    h[150:170] = 100  # sim < 0
    h[170:256] = 5 + i[170:256] % 7
    h[256:] = 3  # the best run lies beyond the first 256 images ...
    h[280] = 0  # ... with the strict maximum inside it
    h[290] = 10
    h[270] = 128  # sim = -1
    return h


def _topk_case(name, alpha, thr, thresholds):
    D, W = TOPK_D, TOPK_D // 32
    c = centroids(64, D)
    h = topk_weights()
    bits = np.ones((TOPK_N, D), bool)
    for i in range(TOPK_N):
        bits[i, (i + np.arange(h[i])) % D] = False  # h zeros, at positions that move with i
    codes = np.packbits(bits, axis=1, bitorder="big").view(">u4").astype(np.uint32)
    feat = (c[TOPK_W0] + f32(0.01))[None].astype(f32)
    ids = np.array([[TOPK_W0]])
    ref = R.ForwardDb(c, 1, 1, alpha, thr)
    for i in range(TOPK_N):
        ref.add(codes[i:i + 1], np.array([TOPK_W0], np.int32))
    q_code, q_word = R.aggregate(feat, ids, c)
    assert q_word.tolist() == [TOPK_W0]
    scores = ref.search(q_code, q_word)
    runs = []
    for k in TOPK_K:
        for t in thresholds(ref.tab):
            want, s = ref.update(feat[0:1], ids, False, k, t)
            assert np.array_equal(s, scores, equal_nan=True)
            runs.append((k, float(t), want))
    _freeze(h, codes, feat, q_code, scores)
    return TopkCase(name, "C", c, alpha, thr, TOPK_W0, h, codes, feat, q_code, scores, runs)


TOPK = {
    # below every score, 0 (the zeros drop out), a score that is present (strict >), above every score
    "topk_ties": lambda: _topk_case("topk_ties", 3.0, 0.0, lambda tab: (-1.0, 0.0, float(tab[5]), 2.0)),
    "topk_nan": lambda: _topk_case("topk_nan", 2.5, -1.0, lambda tab: (-1.0, 0.0)),
}
TOPK_NAMES = list(TOPK)


@functools.lru_cache(maxsize=None)
def topk(name):
    return TOPK[name]()


# ---- D. the fused update at the key limit ----
UPDATE_SHAPE = (41, 64, 96, 512, 3)  # asmk_sequence(seed, C, D, M, n)
UPDATE = {"update_k8_k8": (8, 8), "update_k8_k3": (8, 3)}
UPDATE_NAMES = list(UPDATE)


def distances64(c, f):
    c64, q = c.astype(np.float64), f.astype(np.float64)
    return (np.sum(q * q, axis=1)[:, None] + np.sum(c64 * c64, axis=1)[None, :]) - 2.0 * (q @ c64.T)


@functools.lru_cache(maxsize=None)
def update_inputs():
    from m3s.synthetic import asmk_sequence

    return _freeze(*asmk_sequence(*UPDATE_SHAPE))


@functools.lru_cache(maxsize=None)
def update(name):
    """Word ids from the fp64 distances (the k nearest, ascending): the inputs keep the nine nearest 1e-3 apart, ten
    times the quantiser's tolerance, so the device's quantiser must assign the same."""
    kq, kb = UPDATE[name]
    c, feats = update_inputs()
    K, min_thresh = 3, 0.0
    ref = R.ForwardDb(c, kq, kb)
    ids, lists, scores = [], [], []
    for i, f in enumerate(feats):
        idx = np.argsort(distances64(c, f), axis=1, kind="stable")[:, :kq if i > 0 else kb]
        got, s = ref.update(f, idx, True, K, min_thresh, ids_build=idx)
        ids.append(_freeze(idx))
        lists.append(got)
        scores.append(s if s is None else _freeze(s))
    _freeze(ref.codes, ref.words, ref.img_ptr)
    return UpdateCase(name, "D", c, feats, kq, kb, K, min_thresh, ids, lists, scores, ref)


FAMILIES = {"A": AGG_NAMES, "B": SEARCH_NAMES, "C": TOPK_NAMES, "D": UPDATE_NAMES}
