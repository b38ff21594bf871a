"""Host checks of the BA pose-solve edge cases (tests/ba_solve_cases.py): every case is a well-conditioned SPD
system, reaches the factor shape it is named for (asserted from a plain-Python elimination that must agree with the
plan's own analysis, m3s_ba_pattern_stats), and every failure variant fails where it says. No GPU."""
import numpy as np
import pytest

import ba_solve_cases as C


@pytest.mark.parametrize("name", C.CASES)
def test_case_is_spd_and_well_conditioned(name):
    """H symmetric positive definite with cond(H) <= 1e5: under that cap the solve bound (ba_solve_cases.bound) is
    dominated by the rounding of the fp32 output."""
    H, g, dx, cond = C.system(name)
    ii, jj, Kp = C.graph(name)
    assert H.shape == (7 * (Kp - 1),) * 2 and np.array_equal(H, H.T)
    np.linalg.cholesky(H)
    print(f"{name}: n {H.shape[0]}, E {len(ii)}, cond(H) {cond:.3g}, max|dx| {np.abs(dx).max():.3g}")
    assert cond <= C.COND_CAP
    # the second term of the bound stays below the first at max|dx|
    assert 4.0 * cond * 2.0 ** -44 < 2.0 ** -24
    # the retraction of such a step stays far inside fp32 (exp(sigma), sigma = dx[:, 6])
    assert np.abs(dx).max() < 40.0
    assert np.allclose(H @ dx, -g, rtol=0, atol=1e-9 * np.abs(g).max() * cond)


@pytest.mark.parametrize("name", C.CASES)
def test_reach_predicates_match_the_plan_analysis(name):
    """The plain-Python elimination and csrc/ba_pattern.cpp agree on factor blocks, levels, update groups, sources,
    source-map entries and pull groups."""
    from m3s import _lib

    ii, jj, Kp = C.graph(name)
    r = C.reach(name)
    got = _lib.ba_pattern_stats(ii, jj, Kp)
    print(f"{name}: nL {got[0]} nlev {got[1]} groups {got[2]} sources {got[3]} sidx {got[4]} pulls {got[5]}; "
          f"noff {sorted(r['noff'])}, largest group {r['max_group']}")
    assert got == r["stats"] and got[0] == r["nL"] and got[1] == r["nlev"]


def test_structured_cases_reach_their_paths():
    r = {n: C.reach(n) for n in C.CASES}
    # one column
    assert r["k2"]["nb"] == 1 and r["k2"]["n"] == 7 and r["k2"]["nL"] == 1 and r["k2"]["nlev"] == 1
    # no off-diagonal block: one level, empty grp / src / sidx
    p = r["pinstar12"]
    assert p["nlev"] == 1 and p["nL"] == p["nb"] == 11 and p["stats"][2:] == (0, 0, 0, 0) and p["noff"] == {0}
    # a pure chain: every level a single column
    c = r["chain40"]
    assert c["nlev"] == c["nb"] == 39 and c["nL"] == 2 * c["nb"] - 1 and c["single_levels"] == c["nlev"]
    assert c["noff"] == {0, 1}
    # a hub: one update group of more than 63 sources (flow_wait_task's second chunk). Minimum degree takes the 69
    # lowest leaves first, then the hub (a tie with the last leaf goes to the lower index), so the hub's pull group has
    # 69 sources and the last leaf sits one level above it
    h = r["hub72"]
    assert h["max_group"] == 69 and h["max_group"] >= 64 and h["nlev"] == 3
    # a clique: every count of off-diagonal blocks from 0 to 28
    q = r["clique30"]
    assert q["nL"] == q["nb"] * (q["nb"] + 1) // 2 and q["nlev"] == q["nb"] == 29
    assert q["noff"] == frozenset(range(29))


def test_clique_columns_sit_on_every_row_regime_boundary():
    """sp_column_task: rows = 7 (noff + 1) + 1. noff 8: 64 rows, the rhs row on lane 63, the last of the prefetching
    loop; 9: the first with two rows per lane; 17: 127 rows, the last without an extra pass; 18: 134 rows, one extra
    pass; 27 and 28: more than 192 rows, two extra passes. sp_back_column: 0, 1..9, 10..18 and more than 18 blocks."""
    noff = C.reach("clique30")["noff"]
    assert {8, 9, 17, 18, 26, 27, 28} <= noff
    assert C.rows_of(8) == 64 and C.rows_of(9) == 71 and C.rows_of(17) == 127 and C.rows_of(18) == 134
    passes = lambda k: max(0, -(-(C.rows_of(k) - 128) // 64))
    assert passes(17) == 0 and passes(18) == 1 and passes(26) == 1 and passes(27) == 2 and passes(28) == 2
    assert {0} <= noff and {1, 9} <= noff and {10, 18} <= noff and {19, 28} <= noff


def test_dense_cases_sit_on_the_panel_boundaries():
    n = {k: C.reach(k)["n"] for k in C.CASES}
    assert n["dense10"] == 63 and n["dense11"] == 70            # a single ragged panel; one panel and 6 columns
    assert n["dense56"] == 385 and n["dense56"] % 64 == 1       # a last panel of one column
    assert n["dense65"] == 448 and n["dense65"] % 64 == 0       # the tile row that holds only the rhs row
    assert n["dense74"] == 511 and n["dense74"] % 64 == 63      # a last panel of 63 columns
    assert max(n.values()) == 511
    assert all(v < 256 for k, v in n.items() if k in ("k2", "pinstar12", "dense10", "dense11", "multi9", "clique30"))


def test_multi9_holds_every_irregular_edge():
    ii, jj, Kp = C.graph("multi9")
    ids = sorted(set(ii.tolist()) | set(jj.tolist()))
    assert ids == list(C.MULTI9_IDS) and Kp == 9 and ids != list(range(9))
    first = [int(np.flatnonzero((ii == k) | (jj == k))[0]) for k in ids]
    assert first != sorted(first)  # the ids do not appear in rank order
    pairs = list(zip(ii.tolist(), jj.tolist()))
    pin = ids[0]
    assert any(pairs.count(p) == 2 for p in pairs)                                   # a duplicated directed edge
    assert any(a != b and (b, a) not in pairs and pin not in (a, b) for a, b in pairs)  # one direction only
    assert any(a == b and a != pin for a, b in pairs)                                # a self-loop on a free pose
    assert any(a == pin for a, b in pairs) and any(b == pin for a, b in pairs)       # the pin on either side
    # the self-loop adds nothing and the duplicate counts twice (the rule of ba_solve_cases.assemble)
    es = C.edge_sums("multi9")
    H = C.system("multi9")[0]
    loop = pairs.index(next(p for p in pairs if p[0] == p[1]))
    keep = np.arange(len(pairs)) != loop
    assert np.allclose(C.assemble(es[keep], ii[keep], jj[keep])[0], H, rtol=0, atol=1e-12)
    dup = max(i for i, p in enumerate(pairs) if pairs.count(p) == 2)
    keep = np.arange(len(pairs)) != dup
    assert not np.allclose(C.assemble(es[keep], ii[keep], jj[keep])[0], H, rtol=0, atol=1e-3)


@pytest.mark.parametrize("variant", C.FAIL_VARIANTS)
@pytest.mark.parametrize("name", C.FAIL_CASES)
def test_failure_variants_fail_where_they_say(name, variant):
    ii, jj, Kp = C.graph(name)
    perm = C.symbolic(ii, jj, Kp)["perm"]
    good = C.permuted(C.system(name)[0], perm)
    np.linalg.cholesky(good)
    es = C.failing_table(name, variant)
    assert es.shape == C.edge_sums(name).shape and (es != C.edge_sums(name)).sum() == 1
    Hp = C.permuted(C.assemble(es, ii, jj)[0], perm)
    with pytest.raises(np.linalg.LinAlgError):
        L = np.linalg.cholesky(Hp)
        # a LAPACK whose potrf does not test its pivots for NaN (OpenBLAS) returns a NaN factor instead of an error
        if variant == "nan_block" and np.isnan(np.diag(L)).any():
            raise np.linalg.LinAlgError("NaN pivot")
    if variant == "nan_block":
        assert np.isnan(Hp).sum() == 8  # entries (2, 4) and (4, 2) of both diagonal blocks and of both blocks between
        return
    k = C.fail_pivot(name, variant)
    L = np.linalg.cholesky(Hp[:k, :k])  # every leading principal minor before the failing pivot is positive
    piv = Hp[k, k] - np.sum(np.linalg.solve(L, Hp[:k, k]) ** 2)
    d0 = np.diag(np.linalg.cholesky(good)) ** 2
    print(f"{name} {variant}: pivot {k} = {piv:.3g} (was {d0[k]:.3g}), smallest pivot before it "
          f"{np.diag(L).min() ** 2:.3g} (was {d0[:k].min():.3g})")
    # macroscopic on both sides: the device's pivots (relative error about cond 2^-44) cannot land on the other one
    assert piv < -0.05 * d0[k] and np.diag(L).min() ** 2 > 0.05 * d0[:k].min()
    lev = C.symbolic(ii, jj, Kp)["lev"]
    assert (lev[0] == 0 and k == 6) if variant == "neg_leaf" else k == Hp.shape[0] - 1


def test_back_substitution_wait_loop_beyond_64_blocks_is_unreachable():
    """sp_back_column's x-done wait continues at ``base += 64`` only for a column of more than 64 off-diagonal blocks
    under the dataflow schedule, which needs the loop tables in LDS (SP_PLAN_BYTES = 144 KB, csrc/m3s_ba.h). The rows
    of such a column form a clique among the later columns, so its factor holds a 66-column clique at least, and the
    source map (sidx) of that alone, (m - 1) m (m + 1) / 6 ints at m = 66, is larger than the LDS budget."""
    from m3s import _lib

    m = 66
    ii, jj = C._two_way([(a, b) for b in range(m + 1) for a in range(b)])
    stats = _lib.ba_pattern_stats(ii, jj, m + 1)
    assert max(len(s) for s in C.symbolic(ii, jj, m + 1)["struct"]) == 65
    assert stats[4] == (m - 1) * m * (m + 1) // 6
    assert 4 * stats[4] > 144 * 1024
