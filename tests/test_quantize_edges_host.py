"""The quantiser edge cases themselves, on the CPU alone (no device): the conditions that keep
tests/test_gpu_quantize_edges.py from passing vacuously. For every case of tests/quantize_edge_cases.py:

* the generator separated every query: the k + 1 smallest distinct fp64 distances are at least margin * scale^2
  apart, so no query is left out of any comparison (the cap on excluded queries is zero);
* the numpy restatement of the kernel's arithmetic (bf16 hi/lo split, three products per 32-column step in fp32,
  fp32 norms) selects exactly the expected indices and its largest distance error over scale^2 stays below
  margin / 4 (printed);
* the cases reach the branches they are meant to reach: the tau = +inf fallback exactly at the tails that should
  take it, the tie fallback in both query groups and in tiles shared with ordinary queries, ranks on both sides of
  the merge's fold at C > 65536, every k template and the k-step counts at the unroll's residues.

Emulated distance error over scale^2, the largest of each family (printed by the first test): ksteps 2.3e-5 (at
D = 8; 1.2e-5 from D = 24 on), groups 7.3e-6, tails 1.3e-5, ties 5.8e-6, big 1.5e-5, scale 4.0e-6, exact 1.3e-5,
plumb 6.8e-6. The margin is 1e-3. The emulation's order of additions inside a step is not the matrix cores', so these
estimate the device's error and do not measure it.
"""
import numpy as np
import pytest

import quantize_edge_cases as E


@pytest.mark.parametrize("name", E.NAMES)
def test_case_is_separated_and_emulates(name):
    cs = E.case(name)
    C, D = cs.c.shape
    M = len(cs.q)
    assert cs.q.shape == (M, D) and cs.topk.shape == (M, cs.k) and cs.l2.shape == (M, C)
    assert cs.c.dtype == cs.q.dtype == np.float32 and cs.topk.dtype == np.int64 and cs.l2.dtype == np.float64
    assert np.isfinite(cs.c).all() and np.isfinite(cs.q).all()
    thr = cs.margin * cs.scale ** 2
    # separation, from the returned l2 alone: the distinct values of every row
    rep = E.representatives(cs.c)
    uniq = np.unique(rep)
    assert E.separated(cs.l2[:, uniq], cs.k, thr).all(), "a query is not separated"
    # the expectation: ascending distances, ties (equal fp64 values) in ascending row order, nothing nearer left out
    rows = np.arange(M)[:, None]
    dk = cs.l2[rows, cs.topk]
    assert (np.diff(dk, axis=1) >= 0).all()
    assert ((np.diff(dk, axis=1) > 0) | (np.diff(cs.topk, axis=1) > 0)).all()
    rest = cs.l2.copy()
    rest[rows, cs.topk] = np.inf
    if cs.k < C:
        nxt = rest.min(axis=1)
        assert (nxt >= dk[:, -1]).all()
        tie = nxt == dk[:, -1]  # cut inside a tie group: the rows left out are higher
        assert (rest.argmin(axis=1)[tie] > cs.topk[tie, -1]).all()
    # duplicates tie exactly, also in the emulation
    assert np.array_equal(cs.l2, cs.l2[:, rep])
    emu = E.emulate(cs.c, cs.q)
    assert np.array_equal(emu, emu[:, rep])
    err = float(np.abs(emu.astype(np.float64) - cs.l2).max()) / cs.scale ** 2
    print(f"{name}: C={C} D={D} M={M} k={cs.k} emulated distance error / scale^2 {err:.2e} (margin {cs.margin:g})")
    assert err < cs.margin / 4
    assert np.array_equal(E.topk(emu, cs.k), cs.topk)


def test_emulation_split_is_rne_bf16():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-3, 1.0 + 2.0 ** -9, 0.0], np.float32)
    hi, lo = E.split(x)
    # 1 + 2^-8 is halfway between bf16 1 and 1 + 2^-7: even -> 1; 1 + 3 * 2^-8 is halfway: even -> 1 + 2^-6
    assert hi[:4].tolist() == [1.0, 1.0, 1.015625, -1.0]
    assert ((hi.view(np.uint32) | lo.view(np.uint32)) & 0xFFFF == 0).all()
    assert (np.abs(x - hi) <= np.abs(x) * 2.0 ** -8).all() and (np.abs(x - hi - lo) <= np.abs(x) * 2.0 ** -16).all()
    n = E.norms_f32(np.arange(1, 601, dtype=np.float32).reshape(2, 300) / 64)
    assert np.allclose(n, ((np.arange(1, 601).reshape(2, 300) / 64.0) ** 2).sum(axis=1), rtol=1e-6)


def test_lane_slots_restate_the_layout():
    """Thread (wave w, lane) holds rows 32 w + 4 (lane >> 4) + 16 r + i of its block (row0 of the epilogue)."""
    seen = {}
    for w in range(8):
        for lane in range(64):
            for r in range(2):
                for i in range(4):
                    row = 32 * w + 4 * (lane >> 4) + 16 * r + i
                    assert E.lane_slot(row) == (w, lane >> 4) == E.lane_slot(row + 256)
                    seen.setdefault(row, (w, lane >> 4))
    assert sorted(seen) == list(range(256))


# tails that do not take the tau = +inf fallback: how many of the 40 tail-block lists still pass the cap by their data
TAILS_OVER = {(8, 8): 0, (45, 8): 23, (257, 5): 0, (301, 8): 15, (300, 7): 4}


@pytest.mark.parametrize("C,k", E.TAILS)
def test_tails_reach(C, k):
    cs = E.case(f"tails-C{C}-k{k}")
    want = (C, k) in E.TAILS_FALLBACK
    assert E.fallback_by_tail(C, k) == want
    n = E.list_lengths(cs.l2, k)
    assert n.shape == (40, -(-C // 256))
    # the filter's list of the tail block, from the fp64 distances: every real row when tau = +inf. With k slots
    # filled tau is the largest slot minimum, finite: some lists still pass the cap by their data, the others take
    # the ordinary sort on a partly filled block
    over = n[:, -1] > E.CAP
    print(f"tails C={C} k={k}: {int(over.sum())} of 40 tail-block lists over the cap")
    if want:
        assert (n[:, -1] == C % 256).all() and over.all()
    else:
        # the kernel redoes only the queries whose own list passed the cap (cnt > RQ_CAP), so the others keep the
        # ordinary sort's result even in a tile that takes the fallback: the split of the fixed seed, and at least
        # 15 of the 40 on the ordinary path
        assert int(over.sum()) == TAILS_OVER[C, k] and (~over).sum() >= 15
        assert (n[:, -1] >= min(k, C % 256)).all()
    assert (cs.topk >= 256).any() == (C > 256)
    if k == C:
        assert (np.sort(cs.topk, axis=1) == np.arange(C)).all()


def test_tails_table():
    assert {ck for ck in E.TAILS if E.fallback_by_tail(*ck)} == E.TAILS_FALLBACK
    assert E.fallback_by_tail(300, 8) and not E.fallback_by_tail(301, 8) and not E.fallback_by_tail(300, 7)
    assert not E.fallback_by_tail(24, 8) and E.fallback_by_tail(25, 5) and not E.fallback_by_tail(25, 4)
    assert not E.fallback_by_tail(256, 8) and not E.fallback_by_tail(512, 8)
    # the ksteps and scale families run C = 300 as well: k = 8 takes the tail fallback, the others do not
    assert [E.fallback_by_tail(300, k) for _, k in E.KSTEPS] == [False] * 7 + [True, False]


@pytest.mark.parametrize("k", E.TIES_K)
def test_ties_reach(k):
    cs = E.case(f"ties-k{k}")
    tied = E.fallback_by_ties(cs)
    n = E.list_lengths(cs.l2, k)
    at = {src: np.array(p) for src, p in E.TIES_AT.items()}
    if k in (8, 5):
        assert tied.any()
    # the two groups above the cap overflow the list of their block for the queries aimed at them, at every k
    assert tied[at[3]].all() and (n[at[3], 0] > E.CAP).all()
    assert tied[at[5]].all() and (n[at[5], 1] > E.CAP).all() and (n[at[5], 0] <= E.CAP).all()
    # the 20 copies tie under the cap: the ordinary sort orders them
    assert not tied[at[9]].any() and (n[at[9], 0] >= min(k, 6)).all() and (n[at[9], 0] <= E.CAP).all()
    assert (tied & (np.arange(len(tied)) >= E.QG)).sum() >= 4
    tiles = np.arange(len(tied)) // E.QTILE
    ordinary = ~tied & (n[:, 0] <= E.CAP)  # in block 0 (at k = 8 the tail block's tau is +inf for every query)
    mixed = [t for t in np.unique(tiles) if tied[tiles == t].any() and ordinary[tiles == t].any()]
    assert mixed and any(t >= E.QG // E.QTILE for t in mixed) and any(t < E.QG // E.QTILE for t in mixed)
    print(f"ties k={k}: {int(tied.sum())} tied queries, {int((~ordinary).sum())} with a list over the cap, "
          f"tiles with both kinds {[int(t) for t in mixed]}")
    for src, first in E.TIES_FIRST.items():
        assert (cs.topk[at[src]] == np.array(first[:k])).all()
    assert (cs.topk[at[9]][:, :k] == np.array([9] + list(range(20, 39)))[:k]).all()
    # a tie group cut by k, and ties across the two blocks
    if k == 8:
        assert (cs.l2[at[5][0], cs.topk[at[5][0]]] == cs.l2[at[5][0], 285]).all()


def test_big_reach():
    cs = E.case("big-k8")
    assert cs.c.shape[0] == 82000 and -(-82000 // 256) == 321 > E.MERGE_BLOCKS
    assert (cs.words >= 65536).sum() == 40 and (cs.words < 65536).sum() == 24
    both = ((cs.topk >= 65536).any(axis=1) & (cs.topk < 65536).any(axis=1)).sum()
    fold2 = (cs.topk >= 256 * 320).any(axis=1).sum()  # block 320: the second list folded into lane 0's first
    folded = (cs.topk // 256 >= E.MERGE_BLOCKS).any(axis=1).sum()
    print(f"big: {both} queries rank on both sides of row 65536, {folded} rank a folded block, {fold2} block 320")
    assert both >= 20 and fold2 >= 1 and folded >= 40
    # the duplicate groups tie across folded and unfolded lists, in row order
    w700 = np.flatnonzero(np.isin(cs.words, [700, 66000, 70000, 81999]))
    w12 = np.flatnonzero(np.isin(cs.words, [12, 40000, 65536]))
    assert len(w700) >= 4 and len(w12) >= 3
    assert (cs.topk[w700, :4] == [700, 66000, 70000, 81999]).all()
    assert (cs.topk[w12, :3] == [12, 40000, 65536]).all()
    # inside one merge lane: lane l holds the lists of blocks l, l + 64, l + 128, l + 192 and folds blocks l + 256
    # and l + 320 into the first. Rows 12 (block 0) and 65536 (block 256) tie and meet in lane 0's first list, so
    # the queries at that group rank an unfolded and a folded key of one list, in row order
    blk = cs.topk // 256
    assert (blk[w12, 0] == 0).all() and (blk[w12, 2] == 256).all() and 256 % 64 == 0
    same_lane = [bool(((b[:, None] % 64 == b[None, :] % 64) & (b[:, None] >= 256) & (b[None, :] < 256)).any()) for b in blk]
    print(f"big: {sum(same_lane)} queries rank a folded and an unfolded block of one merge lane")
    assert all(same_lane[i] for i in w12)
    # k = 1 is the first column of the same queries. Every lane's first list holds the K keys of a block below 64
    # before the fold, so a winner in a folded block went to the head of an unfolded list, and a winner in a block
    # below 64 kept the head against the folded keys
    one = E.case("big-k1")
    assert np.array_equal(one.topk, cs.topk[:, :1]) and np.array_equal(one.q, cs.q)
    assert (one.topk >= 65536).sum() >= 30 and (one.topk < 65536).sum() >= 20
    assert (one.topk // 256 < 64).sum() >= 4


def test_templates_and_steps():
    S = [-(-D // 32) for D, _ in E.KSTEPS]
    assert S == [1, 1, 1, 2, 5, 6, 7, 12, 13]
    assert {s % 6 for s in S} == {0, 1, 2, 5}
    ks = {E.case(n).k for n in E.NAMES}
    assert ks == set(range(1, 9))
    assert {k for _, k in E.KSTEPS} == set(range(1, 9))
    assert any(D % 8 for D, _ in E.KSTEPS) and any(D % 32 and not D % 8 for D, _ in E.KSTEPS)
    # query groups: 1, 2 and 3, padded rows, a group of one row, and both blocks aimed at
    assert [-(-M // E.QG) for M in E.GROUPS_M] == [1, 1, 1, 1, 2, 3]
    for M in E.GROUPS_M:
        cs = E.case(f"groups-M{M}")
        assert len(cs.q) == M and (M < 16 or ((cs.words >= 256).any() and (cs.words < 256).any()))
        assert M < 16 or ((cs.topk[:, 0] >= 256).any() and (cs.topk[:, 0] < 256).any())


def test_exact_and_scale_cases():
    cs = E.case("exact")
    assert np.array_equal(cs.q, cs.c[cs.words]) and (cs.topk[:, 0] == cs.words).all()
    assert (cs.l2[np.arange(64), cs.words] < 1e-12).all() and len(set(cs.words.tolist())) == 64
    emu = E.emulate(cs.c, cs.q)
    assert (emu[np.arange(64), cs.words] > 0).all()  # the split drops a positive lo lo term: no negative distance
    a, b = E.case("scale-3.0"), E.case("scale-0.01")
    assert abs(np.linalg.norm(a.c, axis=1).mean() - 3.0) < 1e-3 and abs(np.linalg.norm(b.c, axis=1).mean() - 0.01) < 1e-5
    assert a.scale == 3.0 and b.scale == 0.01


def test_cases_of_one_seed_share_their_codebook():
    base = E.case("groups-M609")
    for M, k in E.PLUMB:
        cs = E.case(E.plumb_name(M, k))
        assert np.array_equal(cs.c, base.c) and len(cs.q) == M and cs.k == k
    assert E.case("ties-k5").c is E.case("ties-k8").c
