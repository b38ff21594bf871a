"""The ASMK edge cases themselves, on the CPU alone (no device): the conditions that keep
tests/test_gpu_asmk_edges.py from passing vacuously. For the cases of tests/asmk_edge_cases.py:

A. every aggregate case reaches the branch it is named for: the padded size P the launcher chooses, the passes per
   bitonic step, the waves that hold a key in the scan, key bit 31, the keys the repeat filter drops and where, the
   slots and the rows per slot, the code-word layout. For the one-word cases the reference's row-by-row adds equal
   numpy's own axis-0 sum, and adding the rows in descending order changes at least a quarter of the code bits of the
   order-sensitive word.
B. the exact scores are exact: the table is (D - 2h)^3 / D^3, every norm a power of four, and the reference's fp64
   sums are bit-identical after a random permutation of each image's entries. Both popcount paths, the append's
   stride loop and the image without entries are reached.
C. more than 256 images, the strict maximum beyond index 256, tie runs cut by k, thresholds on both sides of a score
   that is present, NaN scores that take the leading slots; ``asmk_ref.rank`` agrees with ``torch.topk`` on NaNs.
D. the nine nearest fp64 distances of every feature are 1e-3 apart (so the device's quantiser must assign the
   expected ids and no image is left out), and 4096 keys are sorted.
"""
import numpy as np
import pytest

import asmk_edge_cases as E
import asmk_ref as R

# name: (M, k, use_cols, D, P, passes per bitonic step, waves holding a key)
AGG_REACH = {
    "one_key": (1, 1, 1, 32, 64, 1, 1),
    "p64_full": (64, 1, 1, 64, 64, 1, 1),
    "p128_first": (65, 1, 1, 64, 128, 1, 1),
    "scan_wave_edge_256": (256, 1, 1, 96, 256, 1, 1),
    "scan_wave_edge_257": (257, 1, 1, 96, 512, 1, 2),
    "p2048_full": (2048, 1, 1, 32, 2048, 1, 8),
    "p4096_first": (2049, 1, 1, 32, 4096, 2, 9),
    "full_distinct": (4096, 1, 1, 32, 4096, 2, 16),
    "full_one_word": (4096, 1, 1, 32, 4096, 2, 16),
    "k8_full": (512, 8, 8, 96, 4096, 2, 16),
    "use_cols_3": (512, 8, 3, 96, 2048, 1, 6),
    "dup_in_row": (300, 8, 8, 96, 4096, 2, 10),
    "high_words": (4096, 1, 1, 32, 4096, 2, 16),
    "order_sensitive_288": (330, 1, 1, 288, 512, 1, 2),
    "order_sensitive_1024": (330, 1, 1, 1024, 512, 1, 2),
}
AGG_REACH.update({f"dims_{D}": (24, 3, 3, D, 128, 1, 1) for D in E.DIMS})


def test_case_tables():
    assert list(AGG_REACH) == E.AGG_NAMES
    assert list(E.FAMILIES) == ["A", "B", "C", "D"]
    assert E.SEARCH_NAMES == [f"exact_scores_{D}" for D in (32, 64, 128, 256)] + ["big_append", "empty_image"]
    assert E.TOPK_NAMES == ["topk_ties", "topk_nan"] and E.UPDATE_NAMES == ["update_k8_k8", "update_k8_k3"]
    assert [E.sort_P(n) for n in (1, 64, 65, 2048, 2049, 4096)] == [64, 64, 128, 2048, 4096, 4096]
    assert [E.sort_passes(n) for n in (1, 2048, 2049, 4096)] == [1, 1, 2, 2]
    assert [E.scan_waves(n) for n in (1, 256, 257, 4096)] == [1, 1, 2, 16]


# ---- A ----
@pytest.mark.parametrize("name", E.AGG_NAMES)
def test_a_aggregate_case_reaches_its_branch(name):
    cs = E.agg(name)
    M, k, use_cols, D, P, passes, waves = AGG_REACH[name]
    C = len(cs.c)
    assert cs.des.shape == (M, D) and cs.ids.shape == (M, k) and cs.use_cols == use_cols and cs.c.shape[1] == D
    assert cs.des.dtype == np.float32 and cs.ids.dtype == np.int64 and cs.codes.dtype == np.uint32
    assert cs.ids.min() >= 0 and cs.ids.max() < C <= 2 ** 20 and M * k <= E.MAX_KEYS  # inside the contract
    assert not any(a.flags.writeable for a in (cs.c, cs.des, cs.ids, cs.codes, cs.words))
    n = M * use_cols
    keys = E.sorted_keys(cs.ids, use_cols)
    drops = E.dropped_positions(keys)
    rows = E.rows_per_slot(cs)
    assert (E.sort_P(n), E.sort_passes(n), E.scan_waves(n)) == (P, passes, waves)
    assert cs.codes.shape == (len(cs.words), D // 32) and (np.diff(cs.words) > 0).all()
    assert np.array_equal(np.unique(keys >> 12), cs.words) and rows.sum() == n - len(drops)
    bit31 = bool((keys >> 31).any())
    print(f"A {name}: n={n} P={P} passes={passes} waves={waves} bit31={bit31} dropped={len(drops)} "
          f"slots={len(rows)} rows/slot {rows.min()}..{rows.max()} W={D // 32}")
    assert bit31 == (name == "high_words")
    assert (len(drops) > 0) == (name == "dup_in_row")
    if name in ("p64_full", "p2048_full", "full_distinct", "full_one_word", "k8_full", "high_words"):
        assert n == P  # no padding
    if name in ("scan_wave_edge_257", "p4096_first", "p128_first"):
        assert n == P // 2 + 1  # the first size of the next P
    if name == "scan_wave_edge_257":
        assert (keys[256] >> 12) > (keys[0] >> 12) and len(rows) > 64  # the second wave starts at a carried count
    if name == "full_distinct":
        assert len(rows) == 4096 and (rows == 1).all() and (keys & 0xfff).max() == 4095
    if name == "full_one_word":
        assert rows.tolist() == [4096] and (keys & 0xfff).tolist() == list(range(4096))
    if name in ("k8_full", "use_cols_3"):
        assert len(rows) == 64 and rows.min() >= 2 and cs.ids.shape[1] == 8
    if name.startswith("order_sensitive"):
        assert rows[cs.words.tolist().index(E.ORDER_WORD)] == E.ORDER_ROWS >= 300 and len(rows) > 1


def test_a_use_cols_takes_the_leading_columns_of_a_wider_row():
    full, three = E.agg("k8_full"), E.agg("use_cols_3")
    assert np.array_equal(full.ids, three.ids) and np.array_equal(full.des, three.des) and full.c is three.c
    assert np.array_equal(full.words, three.words) and not np.array_equal(full.codes, three.codes)
    # reading the ids with the row stride use_cols instead of k names other rows
    wrong = full.ids.reshape(-1)[:512 * 3].reshape(512, 3)
    assert not np.array_equal(wrong, three.ids[:, :3])
    assert not np.array_equal(R.aggregate(three.des, wrong, three.c)[0], three.codes)


def test_a_dup_in_row_drops_inside_a_thread_and_across_threads_and_waves():
    cs = E.agg("dup_in_row")
    keys = E.sorted_keys(cs.ids, 8)
    drops = E.dropped_positions(keys)
    mult = np.array([np.unique(r, return_counts=True)[1].max() for r in cs.ids])
    assert {2, 3, 8} <= set(mult.tolist()) and (mult == 1).sum() >= 200
    assert len(drops) == int(sum(len(r) - len(set(r)) for r in cs.ids.tolist()))
    at4, at256 = drops[drops % 4 == 0], drops[drops % 256 == 0]
    print(f"A dup_in_row: {len(drops)} keys dropped, {len(at4)} at i % 4 == 0, at i % 256 == 0: {at256.tolist()}, "
          f"{(drops % 4 != 0).sum()} inside a thread")
    assert len(at4) >= 1 and 256 in at256 and (drops % 4 != 0).any()
    # drops lie in several waves, so the kept counts carried from wave to wave differ from the key counts
    assert len(set((drops // 256).tolist())) >= 3
    # without the filter a row would be added more than once: other codes
    ids = cs.ids
    acc_twice = np.zeros(cs.des.shape[1], np.float32)
    for r in np.flatnonzero((ids == 0).any(axis=1)):
        for _ in range(int((ids[r] == 0).sum())):
            acc_twice = acc_twice + (cs.des[r] - cs.c[0])
    once = cs.codes[cs.words.tolist().index(0)]
    assert not np.array_equal(np.packbits(acc_twice > 0, bitorder="big").view(">u4").astype(np.uint32), once)


def test_a_high_words_need_an_unsigned_order():
    cs = E.agg("high_words")
    assert sorted(set(cs.ids.reshape(-1).tolist())) == list(E.HIGH_WORDS) == cs.words.tolist()
    assert cs.ids[4095, 0] == 2 ** 20 - 1 and len(cs.c) == 2 ** 20
    keys = E.sorted_keys(cs.ids, 1)
    assert keys[-1] == 0xffffffff  # word 2^20 - 1, row 4095: the padding's own value, and no padding here
    assert (keys >> 31).sum() > 1000 and (keys >> 31 == 0).sum() > 1000
    signed = np.sort(keys.view(np.int32)).view(np.uint32)
    assert not np.array_equal(signed, keys) and (signed[0] >> 12) == 2 ** 19
    used = np.zeros(2 ** 20, bool)
    used[list(E.HIGH_WORDS)] = True
    assert not cs.c[~used].any() and cs.c[used].any(axis=1).all()


def _row_sum_codes(res):
    return np.packbits(np.sum(res, axis=0) > 0, bitorder="big").view(">u4").astype(np.uint32)


def _sequential(res):
    acc = np.zeros(res.shape[1], np.float32)
    for r in res:
        acc = acc + r
    return acc


@pytest.mark.parametrize("name", ["order_sensitive_288", "order_sensitive_1024", "full_one_word"])
def test_a_row_order_is_pinned(name):
    cs = E.agg(name)
    w = E.ORDER_WORD if name.startswith("order") else 777
    rows = np.flatnonzero((cs.ids == w).any(axis=1))
    res = cs.des[rows] - cs.c[w]
    assert res.dtype == np.float32
    code = cs.codes[cs.words.tolist().index(w)]
    assert np.array_equal(_row_sum_codes(res), code)  # the reference's adds one after another = numpy's axis-0 sum
    assert np.array_equal(np.sum(res, axis=0), _sequential(res))
    if name.startswith("order"):
        mags = np.abs(res)
        assert (mags > 5e7).any() and (mags < 3e-3).any() and (mags > 5e3).sum() > 1000
        D = res.shape[1]
        desc = _sequential(res[::-1])
        flipped = float(((desc > 0) != (np.sum(res, axis=0) > 0)).mean())
        print(f"A {name}: {len(rows)} rows, descending order flips {flipped:.3f} of {D} code bits")
        assert flipped >= 0.25


@pytest.mark.parametrize("rows,D", [(4096, 1024), (2049, 96), (300, 288)])
def test_a_reference_adds_rows_like_numpys_outer_sum(rows, D):
    rng = np.random.default_rng([3, rows, D])
    c = E.centroids(64, D)
    des = (rng.standard_normal((rows, D)) * 10.0 ** rng.integers(-3, 5, size=(rows, 1))).astype(np.float32)
    codes, words = R.aggregate(des, np.full((rows, 1), 5), c)
    assert words.tolist() == [5] and np.array_equal(codes[0], _row_sum_codes(des - c[5]))


def test_a_dims_cover_every_code_word_layout():
    assert [D // 32 for D in E.DIMS] == [1, 2, 3, 5, 8, 9]
    # one word: half a ballot; D = 288: a second pass of 256 dims of which 32 are real (half of one wave's ballot)
    assert E.DIMS[0] == 32 and 288 - 256 == 32 and {D % 64 for D in E.DIMS} == {0, 32}
    for D in E.DIMS:
        cs = E.agg(f"dims_{D}")
        rows = E.rows_per_slot(cs)
        assert len(rows) == 12 and rows.sum() == 72 and rows.max() >= 4
        assert all(len(set(r)) == 3 for r in cs.ids.tolist())
        ones = R.popcount32(cs.codes).sum() / cs.codes.size / 32
        assert 0.35 < ones < 0.65  # both signs everywhere, the last code word included
        assert 0 < R.popcount32(cs.codes[:, -1].copy()).sum() < 32 * len(rows)


# ---- B ----
@pytest.mark.parametrize("D", E.EXACT_D)
def test_b_exact_scores_are_exact(D):
    cs = E.search(f"exact_scores_{D}")
    h = np.arange(D + 1, dtype=np.float64)
    want = np.where(h <= D / 2, (D - 2 * h) ** 3 / D ** 3, 0.0)
    tab = R.sim_table(D, 3.0, 0.0)
    assert cs.alpha == 3.0 and cs.thr == 0.0 and np.array_equal(tab.astype(np.float64), want)
    assert np.array_equal(cs.ref.tab, tab)
    sizes = [n for _, _, n in cs.images]
    assert sizes == list(E.EXACT_SIZES) and all(4 ** round(np.log(n) / np.log(4)) == n for n in sizes)
    assert len(cs.q_words) == 4096 and (np.diff(cs.q_words) > 0).all() and np.sqrt(np.float32(4096)) == 64
    assert np.array_equal(np.diff(cs.ref.img_ptr), sizes) and max(sizes) == 16 * 256  # 16 entries per thread
    path = E.popcount_path(D)
    assert path == ("vector" if D in (128, 256) else "scalar")
    hits, dist = 0, set()
    for codes, words, n in cs.images:
        assert len(set(words.tolist())) == n and (n < 16 or (np.diff(words) < 0).any())  # distinct, not sorted
        pos = np.searchsorted(cs.q_words, words)
        hit = cs.q_words[np.minimum(pos, 4095)] == words
        assert hit.sum() == -(-n // 2)  # hits and misses of the binary search
        hits += int(hit.sum())
        dist |= set(R.popcount32(codes[hit] ^ cs.q_codes[pos[hit]]).sum(axis=1).tolist())
    assert {0, D // 2, D} <= dist and len(dist) > D // 2
    assert (cs.scores > 0).all() and len(set(cs.scores.tolist())) == len(sizes)
    # every term is a dyadic rational with at most 39 bits between the largest sum and the smallest unit
    assert np.array_equal(cs.scores * 2.0 ** 33, np.round(cs.scores * 2.0 ** 33))
    for seed in range(3):
        assert np.array_equal(E.permuted_scores(cs, seed), cs.scores)
    print(f"B exact_scores_{D}: W={D // 32} {path} popcount, {hits} hits over {sum(sizes)} entries, "
          f"{len(dist)} distinct distances")


def test_b_second_uint4_matters_at_256():
    """D = 256 has two uint4 per entry: distances confined to the first would give other scores."""
    cs = E.search("exact_scores_256")
    ref = R.ForwardDb(cs.c, 1, 1)
    for codes, words, n in cs.images:
        half = codes.copy()
        pos = np.minimum(np.searchsorted(cs.q_words, words), 4095)
        half[:, 4:] = cs.q_codes[pos][:, 4:]
        ref.add(half, words)
    assert (ref.search(cs.q_codes, cs.q_words)[1:] != cs.scores[1:]).all()  # image 0 is one entry at h = 0


def test_b_big_append_takes_the_stride_loop():
    cs = E.search("big_append")
    counts = [n for _, _, n in cs.images]
    assert counts == [4096, 5, 300] and cs.c.shape == (4096, 1024)
    assert [E.append_strides(len(w), 1024) for _, w, _ in cs.images] == [True, False, False]
    assert 4096 * 32 == 131072 > 65536
    # nothing else in the family reaches it
    assert not any(E.append_strides(len(w), D) for D in E.EXACT_D for _, w, _ in E.search(f"exact_scores_{D}").images)
    assert np.array_equal(cs.ref.img_ptr, [0, 4096, 4101, 4401]) and cs.ref.codes.shape == (4401, 32)
    # the second pass copies other values than the first
    first = cs.images[0][0].reshape(-1)
    assert not np.array_equal(first[:65536], first[65536:])
    assert (cs.scores > 0).all() and E.popcount_path(1024) == "vector"


def test_b_empty_image_between_two_images():
    cs = E.search("empty_image")
    assert [n for _, _, n in cs.images] == [10, 0, 7] and len(cs.images[1][1]) == 4
    assert cs.ref.img_ptr.tolist() == [0, 10, 10, 17]
    assert cs.scores[1] == 0.0 and cs.scores[0] > 0 and cs.scores[2] > 0
    # its rows would score if they were taken
    taken = R.ForwardDb(cs.c, 1, 1)
    taken.add(*cs.images[1][:2])
    assert np.isin(cs.images[1][1], cs.q_words).all()
    alone = R.ForwardDb(cs.c, 1, 1)
    for i in (0, 2):
        alone.add(*cs.images[i][:2])
    assert np.array_equal(alone.search(cs.q_codes, cs.q_words), cs.scores[[0, 2]])
    assert E.popcount_path(96) == "scalar"


# ---- C ----
def test_c_topk_ties_layout():
    cs = E.topk("topk_ties")
    n = len(cs.scores)
    assert n == 300 > E.TOPK_THREADS and cs.codes.shape == (300, 4)
    assert (cs.q_code == 0xffffffff).all() and cs.q_code.shape == (1, 4)  # every residual positive
    assert np.array_equal(R.popcount32(~cs.codes).sum(axis=1), cs.h)
    assert np.array_equal(cs.scores, R.sim_table(128, 3.0, 0.0)[cs.h].astype(np.float64))  # one table value each
    assert int(cs.scores.argmax()) == 280 and (cs.scores == cs.scores.max()).sum() == 1
    assert (cs.scores == 0).sum() == 71 and (cs.scores[:100] == cs.scores[0]).all()
    ks = sorted({k for k, _, _ in cs.runs})
    ts = sorted({t for _, t, _ in cs.runs})
    assert ks == [1, 3, 64] and len(cs.runs) == 12
    assert ts[0] < cs.scores.min() and ts[-1] > cs.scores.max() and ts[2] in cs.scores and ts[1] == 0.0
    by = {(k, t): got for k, t, got in cs.runs}
    assert by[1, ts[0]] == [280] and by[3, ts[0]] == [280, 256, 257]
    full = by[64, ts[0]]
    assert len(full) == 64 and min(full[:42]) >= 256  # the 42 best lie beyond the first 256 images
    last = cs.scores[full[-1]]
    assert (cs.scores == last).sum() > (cs.scores[full] == last).sum() >= 2  # k cuts a run of equal scores ...
    cut = np.flatnonzero(cs.scores == last)
    assert [i for i in full if cs.scores[i] == last] == cut[:(cs.scores[full] == last).sum()].tolist()  # ... by index
    assert len(by[64, ts[2]]) < 64 and all(cs.scores[i] > ts[2] for i in by[64, ts[2]])
    assert (cs.scores[full] == ts[2]).any()  # a selected score equal to the threshold is dropped
    assert all(by[k, ts[-1]] == [] for k in ks)
    print(f"C topk_ties: {n} images, thresholds {ts}, list lengths {[len(g) for _, _, g in cs.runs]}")


def test_c_topk_nan_layout():
    cs = E.topk("topk_nan")
    nan = np.isnan(cs.scores)
    assert cs.alpha == 2.5 and cs.thr == -1.0 and np.array_equal(nan, cs.h > 64) and nan.sum() == 21
    assert nan[270] and nan[150:170].all() and np.isfinite(cs.scores[~nan]).all()
    by = {(k, t): got for k, t, got in cs.runs}
    assert by[1, -1.0] == [] and by[3, -1.0] == []  # only NaNs are selected
    assert by[64, -1.0][:3] == [280, 256, 257] and len(by[64, -1.0]) == 64 - 21  # finite scores follow the NaNs
    assert len(by[64, 0.0]) == 43 and all(cs.scores[i] > 0 for i in by[64, 0.0])
    print(f"C topk_nan: {int(nan.sum())} NaN scores, list lengths {[len(g) for _, _, g in cs.runs]}")


def test_c_rank_orders_nan_like_torch_topk():
    import torch

    rng = np.random.default_rng(17)
    for n, k in ((300, 64), (300, 3), (40, 40), (7, 1)):
        s = rng.permutation(n).astype(np.float64) / n - 0.25  # no ties among the finite values
        s[rng.choice(n, max(1, n // 10), replace=False)] = np.nan
        got = torch.topk(torch.from_numpy(s), k).indices.tolist()
        m = min(k, int(np.isnan(s).sum()))
        assert m >= 1 and np.isnan(s[got[:m]]).all() and not np.isnan(s[got[m:]]).any()  # torch: NaN first
        assert R.rank(s, k, -np.inf) == got[m:]  # the filter removes the NaNs; what follows them is torch's order
    # NaNs take the leading slots: with as many NaNs as k nothing is left
    s = np.array([0.5, np.nan, 0.7, np.nan, 0.1])
    assert R.rank(s, 2, -np.inf) == [] and R.rank(s, 3, -np.inf) == [2] and R.rank(s, 5, 0.2) == [2, 0]
    assert R.rank(np.array([0.3, 0.9, 0.3]), 3, 0.0) == [1, 0, 2]  # without NaN as before


# ---- D ----
def test_d_quantiser_margin_and_key_counts():
    c, feats = E.update_inputs()
    assert c.shape == (64, 96) and feats.shape == (3, 512, 96)
    gap = min(float(np.diff(np.sort(E.distances64(c, f), axis=1)[:, :9], axis=1).min()) for f in feats)
    print(f"D: smallest gap among the nine nearest fp64 distances {gap:.4e}")
    assert gap >= 1e-3
    for name, (kq, kb) in E.UPDATE.items():
        cs = E.update(name)
        assert [i.shape for i in cs.ids] == [(512, kb), (512, kq), (512, kq)] and kq == 8
        assert 512 * kq == E.MAX_KEYS == E.sort_P(512 * kq) and E.sort_passes(512 * kb) == (2 if kb == 8 else 1)
        assert all(len(set(r)) == len(r) for i in cs.ids for r in i.tolist())
        assert cs.lists[0] == [] and cs.scores[0] is None and cs.lists[1] == [0] and sorted(cs.lists[2]) == [0, 1]
        assert cs.ref.n_images == 3 and cs.ref.img_ptr[-1] == len(cs.ref.words)
        print(f"D {name}: lists {cs.lists}, entries per image {np.diff(cs.ref.img_ptr).tolist()}")
    a, b = E.update("update_k8_k8"), E.update("update_k8_k3")
    assert np.array_equal(a.ids[1], b.ids[1]) and np.array_equal(a.ids[0][:, :3], b.ids[0])
    assert not np.array_equal(a.ref.img_ptr, b.ref.img_ptr)
